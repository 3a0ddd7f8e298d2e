"""K3, the scattered -> regular-grid interpolation kernel, and everything that drives it: the per-shape workspace cache, the
one-device entries, the check that the walk kernel serves a certified mesh, and the slab-wise protocol that shards the
star passes of ONE field over several ranks (two all-gathers, bounded by time-outs).
"""
import ctypes
import os

import numpy as np

from . import _native as nat
from .memory import DeviceBuffer, _lib, _ptr, _size_query
from .args import _DT_CODE, mask_bytes
from .sharding import slab_payload_entries, bounded_call

_ws_cache = {}


def _workspace(h, w, C, stream=None):
    """Scatter workspace for fields of this shape -- one per (shape, stream): calls on different streams may overlap, and
    each then needs bucket lists and an owner map of its own."""
    key = (h, w, getattr(stream, "value", stream) or 0)
    ws = _ws_cache.get(key)
    if ws is None:
        n = _size_query(_lib().ofl_scatter_workspace_bytes, h, w, C)
        if len(_ws_cache) > 6:
            _ws_cache.clear()
        ws = _ws_cache[key] = DeviceBuffer(n)
    return ws


def walk_check(cert, launch, stream=None):
    """Does the walk kernel FIND every node of the mesh that `cert` says is the triangulation?  That depends on the field and
    the sign only, so it is asked once per certificate: `launch(counter)` enqueues the caller's ofl_scatter_certified_dev
    launch with a device counter of lost nodes, one read-back answers.  Yes is remembered (`_walk_checked`: later launches run
    without any synchronisation); no clears `certified` -- the Delaunay path from now on.  -> is the mesh still certified."""
    cnt = DeviceBuffer.zeros(16, stream)
    launch(cnt.ptr)
    if int(cnt.to_host((1,), np.uint32, stream)[0]) == 0:
        cert._walk_checked = True
    else:
        cert.certified = 0
    return bool(cert.certified)


def scatter_linear(flow, sign, pmask, vals, C, vmask, h, w, query, out, valid, valid_rule, point_precision=0,
                   stream=None, cert=None, drops_points=False):
    """K3: scattered -> regular-grid linear interpolation.  Replaces utils.py:237-258 (and, with `query`,
    flow_class.py:1398-1410).  Raises ValueError("No points given") like qhull when nothing is kept.
    cert: a MeshCert of this very (flow, sign, point_precision) without point mask; when it certifies the mesh the
    asynchronous one-kernel entry is taken (no workspace, no read-back).  drops_points: pmask is KNOWN to hold zeros
    (the flow's statistics say so); like a certificate that says "not certified" this spares the entry its own certificate
    pass (OFL_SCATTER_UNCERTIFIED)."""
    if cert is not None and cert.certified and pmask is None and query is None:
        def certified(counter):
            nat.check(_lib().ofl_scatter_certified_dev(flow.ptr, sign, point_precision, _ptr(vals), C, _ptr(vmask), h, w, 0, h,
                                                       _ptr(out), _ptr(valid), valid_rule, ctypes.byref(cert), counter, stream))
        if getattr(cert, "_walk_checked", False):
            certified(None)
            return (h * w, 0, 0)
        if walk_check(cert, certified, stream):             # asked with the real launch: on yes its result stands
            return (h * w, 0, 0)
    if (cert is not None and not cert.certified and pmask is None) or (drops_points and pmask is not None):
        valid_rule |= nat.SCATTER_UNCERTIFIED          # the certificate pass has been run for this field: not again per call
    ws = _workspace(h, w, C, stream)
    info = (ctypes.c_uint64 * 3)()
    nat.check(_lib().ofl_scatter_linear_dev(flow.ptr, sign, point_precision, _ptr(pmask), _ptr(vals), C, _ptr(vmask),
                                            h, w, _ptr(query), _ptr(out), _ptr(valid), valid_rule, ws.ptr, ws.nbytes,
                                            info, stream))
    return tuple(info)


def scatter_linear_f64(flow, sign, pmask, vals, C, vmask, h, w, out, valid, valid_rule, point_precision=0, stream=None):
    """K3 with float64 values at the grid nodes (float64 targets of apply_flow 's', utils.py:253-258)."""
    ws = _workspace(h, w, C, stream)
    info = (ctypes.c_uint64 * 3)()
    nat.check(_lib().ofl_scatter_linear_f64_dev(flow.ptr, sign, point_precision, _ptr(pmask), _ptr(vals), C, _ptr(vmask),
                                                h, w, _ptr(out), _ptr(valid), valid_rule, ws.ptr, ws.nbytes, info, stream))
    return tuple(info)


def scatter_rows(flow, sign, pmask, vals, C, vmask, h, w, row0, rows, out_rows, valid_rows, valid_rule=0,
                 point_precision=0, stream=None):
    """K3 on one row band of a field split over several GPUs (SURVEY 8e, config 5 as loaded): all inputs are the
    replicated H x W arrays; only rows [row0, row0 + rows) of the result are produced."""
    ws = _workspace(h, w, C, stream)
    info = (ctypes.c_uint64 * 3)()
    nat.check(_lib().ofl_scatter_rows_dev(flow.ptr, sign, point_precision, _ptr(pmask), _ptr(vals), C, _ptr(vmask),
                                          h, w, row0, rows, _ptr(out_rows), _ptr(valid_rows), valid_rule, ws.ptr, ws.nbytes,
                                          info, stream))
    return tuple(info)


SLAB_LIST_HEAD = 16          # bytes before the first record of a slab list (entries, error bits, 0, 0)
SLAB_RECORD = 64             # bytes per unfinished site
SLAB_ERR_LIST = 32           # error bit of a list head: the rank's unfinished sites did not fit its list (kErrSlabList)


def slab_list_bytes(entries):
    return SLAB_LIST_HEAD + SLAB_RECORD * int(entries)


def comm_allgather(send_ptr, recv, nbytes, stream=None):
    """ncclAllGather of `nbytes` per rank over the live communicator (send may be the rank's own slot of recv)."""
    nat.check(_lib().ofl_comm_allgather(send_ptr, recv.ptr, nbytes, stream))


def scatter_slab_stars(flow, sign, pmask, h, w, row0, rows, list_ptr, list_bytes, point_precision=0, stream=None, ws=None):
    """Step 1 of the slab-wise scatter (include/ofl.h, ofl_scatter_slab_stars_dev): bins, the stars around rows
    [row0, row0 + rows) and -- at list_ptr (device) -- the unfinished sites of those rows.  The workspace keeps the star
    state for scatter_slab_finish: `ws` (a DeviceBuffer the caller holds on to across both steps, as scatter_slab does) or
    the cached one of this (shape, stream) -- then no other scatter call of that shape on that stream in between, and
    nothing that makes the cache drop it (step 2 refuses a workspace without step 1's stamp)."""
    ws = ws if ws is not None else _workspace(h, w, 0, stream)
    nat.check(_lib().ofl_scatter_slab_stars_dev(flow.ptr, sign, point_precision, _ptr(pmask),
                                                h, w, row0, rows, list_ptr, list_bytes, ws.ptr, ws.nbytes, stream))


def scatter_slab_finish(flow, sign, vals, C, vmask, h, w, row0, rows, lists, list_bytes, n_lists, out_rows, valid_rows,
                        valid_rule=0, point_precision=0, stream=None, ws=None):
    """Step 2: the gathered lists of all ranks -> unfinished stars, owner map and result of the band."""
    ws = ws if ws is not None else _workspace(h, w, 0, stream)
    info = (ctypes.c_uint64 * 3)()
    nat.check(_lib().ofl_scatter_slab_finish_dev(flow.ptr, sign, point_precision, _ptr(vals), C, _ptr(vmask), h, w, row0, rows,
                                                 lists.ptr, list_bytes, n_lists, _ptr(out_rows), _ptr(valid_rows), valid_rule,
                                                 ws.ptr, ws.nbytes, info, stream))
    return tuple(info)


def _slab_timeout():
    return float(os.environ.get("OFL_SLAB_TIMEOUT", "120"))


def scatter_slab(flow, sign, pmask, vals, C, vmask, h, w, row0, rows, out_rows, valid_rows, rank=0, world=1, valid_rule=0,
                 point_precision=0, stream=None, entries=1 << 17, gather=comm_allgather, timeout=None):
    """One row band of a ref-'s' warp whose mesh does not certify, with the star passes sharded over `world` ranks
    (SURVEY 8e, config 5): step 1 into a list of up to `entries` records, the exchange, step 2.  The exchange is two
    all-gathers -- the 16-byte list heads first, then (one read-back of the counts later) only as many 64-byte records per
    rank as the fullest list holds: config 5 at 8K leaves 75 000 sites unfinished in all, 1 MB per rank instead of the
    8 MiB the buffers are sized for.  `gather(send_ptr, recv_buffer, nbytes, stream)` defaults to RCCL over the live
    communicator (sharding.host_allgather(dist) goes through the host instead: rehearsals with ranks that share a GPU).
    Bands concatenate to scatter_linear's result bit for bit.

    Every rank of `world` MUST call this, whatever its band: a rank with an EMPTY band (rows == 0: more ranks than 8-row
    tiles) skips both steps but takes part in both gathers with an empty list; a rank whose step 1 fails joins them with an
    error head and raises afterwards, so that its peers fail with it instead of waiting for it.  When some rank's list
    overflowed (`entries` too small: large holes, hull sites of an 8K field) every rank sees the same counts in the gathered
    heads and all of them repeat the exchange ONCE with lists sized for the fullest.  Each gather -- and the read-back that
    waits for it -- is bounded by `timeout` seconds (default: OFL_SLAB_TIMEOUT, 120): a rank left alone in the collective
    ends its process with exit code 3 (sharding.bounded_call) instead of hanging for ever."""
    if world <= 1 and (row0 != 0 or rows != h):
        raise ValueError("scatter_slab: a band of a field needs the other ranks' lists")
    world = max(int(world), 1)
    timeout = _slab_timeout() if timeout is None else timeout
    ws = _workspace(h, w, 0, stream)               # held across both steps: whatever the exchange does to the cache, step 2 finds step 1's state
    for attempt in range(2):
        nb = slab_list_bytes(entries)
        mine = DeviceBuffer(nb)
        failed = None
        if rows > 0:
            try:
                scatter_slab_stars(flow, sign, pmask, h, w, row0, rows, mine.ptr, nb, point_precision, stream, ws)
            except nat.NativeError as e:            # the peers are on their way into the gathers: join them, then raise
                failed = e
        if rows <= 0 or failed is not None:
            head = np.array([0, SLAB_ERR_LIST if failed is not None else 0, 0, 0], np.uint32)
            nat.check(_lib().ofl_upload(mine.ptr, head.ctypes.data, SLAB_LIST_HEAD, stream))
            nat.check(_lib().ofl_stream_sync(stream))
        if world == 1:
            if failed is not None:
                raise failed
            return scatter_slab_finish(flow, sign, vals, C, vmask, h, w, row0, rows, mine, nb, 1, out_rows, valid_rows,
                                       valid_rule, point_precision, stream, ws)
        heads = DeviceBuffer(SLAB_LIST_HEAD * world)

        def exchange_heads():
            gather(mine.ptr, heads, SLAB_LIST_HEAD, stream)
            return heads.to_host((world, SLAB_LIST_HEAD // 4), np.uint32, stream)
        hw = bounded_call(exchange_heads, timeout, "the all-gather of the slab list heads")
        counts, errs = hw[:, 0], hw[:, 1]
        if attempt == 0 and int(counts.max()) > entries and not errs.any():
            # some rank's list overflowed; every rank reads the same heads and takes this branch together
            entries = int(counts.max()) + 1024
            continue
        m = slab_payload_entries(counts, entries)
        nb2 = slab_list_bytes(m)
        lists = DeviceBuffer(nb2 * world)

        def exchange_lists():
            gather(mine.ptr, lists, nb2, stream)
            nat.check(_lib().ofl_stream_sync(stream))
        bounded_call(exchange_lists, timeout, "the all-gather of the slab lists")
        if failed is not None:
            raise failed
        if rows <= 0:
            return (0, 0, 0)
        # (error bits in a peer's head -- a refused point set, a step 1 that failed there -- reach step 2 with the lists: it
        # blanks this band and raises here as well, include/ofl.h)
        return scatter_slab_finish(flow, sign, vals, C, vmask, h, w, row0, rows, lists, nb2, world, out_rows, valid_rows,
                                   valid_rule, point_precision, stream, ws)


def scatter_host(flow, target, pmask, vmask=None):
    """apply_flow(flow, target, 's', mask) for host arrays (utils.py:237-258; `flow` may already be a DeviceBuffer
    holding the float32 vectors): target (H, W, C) of any numeric
    dtype is interpolated in float32/float64 on the device, then rounded / cast back like the reference.
    Returns (warped, valid or None); valid = float32(interpolated vmask) == 1 (flow_class.py:668)."""
    h, w, C = target.shape
    n = h * w * C
    fbuf = flow if isinstance(flow, DeviceBuffer) else DeviceBuffer.from_host(np.ascontiguousarray(flow, np.float32))
    pm = DeviceBuffer.from_host(mask_bytes(pmask)) if pmask is not None else None
    vm = DeviceBuffer.from_host(mask_bytes(vmask)) if vmask is not None else None
    valid = DeviceBuffer(h * w) if vmask is not None else None
    if target.dtype == np.float64:                                           # griddata's own precision end to end
        vals = DeviceBuffer.from_host(np.ascontiguousarray(target))
        out = DeviceBuffer(n * 8)
        scatter_linear_f64(fbuf, +1, pm, vals, C, vm, h, w, out, valid, 0)
        v = valid.to_host((h, w), np.uint8).view(np.bool_) if valid is not None else None
        return out.to_host((h, w, C), np.float64), v
    native = target.dtype in _DT_CODE and target.dtype != np.float32         # the casts of utils.py:253 / :258 run on the device
    integer = np.issubdtype(target.dtype, np.integer)
    if native:
        raw = DeviceBuffer.from_host(np.ascontiguousarray(target))
        vals = DeviceBuffer(n * 4)
        nat.check(_lib().ofl_convert_dev(raw.ptr, _DT_CODE[target.dtype], vals.ptr, nat.F32, n, None))
    else:
        vals = DeviceBuffer.from_host(np.ascontiguousarray(target, np.float32))
    out = DeviceBuffer(n * 4)
    # integer targets: values AND the concatenated mask channel are np.round-ed before the cast (utils.py:256-257)
    scatter_linear(fbuf, +1, pm, vals, C, vm, h, w, None, out, valid, (nat.SCATTER_ROUND | 2) if integer else 0)
    if native:
        back = DeviceBuffer(n * target.dtype.itemsize)
        nat.check(_lib().ofl_convert_dev(out.ptr, nat.F32, back.ptr, _DT_CODE[target.dtype], n, None))
        res = back.to_host((h, w, C), target.dtype)
    else:
        res = out.to_host((h, w, C), np.float32).astype(target.dtype)       # already rounded for integer targets
    v = valid.to_host((h, w), np.uint8).view(np.bool_) if valid is not None else None
    return res, v


def scatter_query(pos_flow_buf, sign, vals_buf, C, h, w, query_xy, pmask=None):
    """griddata(points, values, query) for sparse float64 query points (utils.py:603, 614).
    Returns (values float64 [n, C], found bool [n])."""
    q = np.ascontiguousarray(query_xy, np.float64)
    n = q.shape[0]
    dq = DeviceBuffer.from_host(q)
    out = DeviceBuffer(max(n, 1) * C * 8)
    found = DeviceBuffer(max(n, 1))
    ws = _workspace(h, w, C)
    nat.check(_lib().ofl_scatter_query_dev(pos_flow_buf.ptr, sign, 0, _ptr(pmask),
                                           vals_buf.ptr, C, h, w, dq.ptr, n, out.ptr, found.ptr, ws.ptr, ws.nbytes, None))
    return out.to_host((n, C), np.float64), found.to_host((n,), np.uint8).view(np.bool_)


def scatter_query_resident(pos_flow_buf, sign, vals_buf, h, w, query, n):
    """scatter_query with the queries already on the device, and the answers left there: (values float64 [n][2] as (u, v),
    found uint8 [n]) DeviceBuffers."""
    vals, found = DeviceBuffer(n * 16), DeviceBuffer(n)
    ws = _workspace(h, w, 2)
    nat.check(_lib().ofl_scatter_query_dev(pos_flow_buf.ptr, sign, 0, None, vals_buf.ptr, 2, h, w, query.ptr, n, vals.ptr,
                                           found.ptr, ws.ptr, ws.nbytes, None))
    return vals, found
