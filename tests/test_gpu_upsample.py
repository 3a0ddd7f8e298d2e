"""K17 (ofl_upsample.hip): convex upsampling on the device, against tests/upsample_ref.py (the definition restated operation for
operation in NumPy float32) and through every layer: the raw ABI, DeviceFlow.upsample_convex, DeviceFlowBatch.upsample_convex,
Flow.upsample_convex, upsample_flow_convex and the host entry.  Every comparison of vectors is byte equality.  Outputs are
written into 0xA5-filled buffers whose bytes around the output must survive, inputs are read back unchanged, and the logits
and the coarse mask also sit one element (2 or 4 bytes, 1 byte) off their buffers' alignment.

The kernel's tile is T coarse pixels of ONE coarse row -- T = 64 in the planar layout, 128 / f = 16, 32, 64 in channels-last --
and a planar block holds min(f, 4) sub-rows, so the coarse shapes of upsample_ref.SHAPES are a single pixel, smaller than a
window, wave tails at 64, ragged against every tile ((4, 37), (2, 65)) and more than two tiles per axis ((3, 200), (5, 130));
nothing of workload size.

The C entry takes no channel count (the logits are 9 f^2 channels by definition), so "a channel count off by one" is refused
where the count exists: by args.upsample_args under DeviceFlow.upsample_convex, before anything is launched."""
import functools
import itertools

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
import consistency_ref as C
from devmem import guarded, place, read_guarded
import interop_ref as R
import upsample_ref as U

pytestmark = pytest.mark.gpu
nat = of.native
GUARD = 64
ELEMS = ("float32", "float16", "bfloat16")
LAYOUTS = ("chw", "hwc")
EL = {"float32": nat.EL_F32, "float16": nat.EL_F16, "bfloat16": nat.EL_BF16}
LAY = {"chw": nat.TENSOR_NCHW, "hwc": nat.TENSOR_NHWC}


def raw_call(v, m, x, elem, layout, f, want_mask=True, shifted=False):
    """ofl_upsample_convex_dev on host arrays: v (h, w, 2) or (n, h, w, 2), m likewise, x the logits as stored, logical
    (..., 9 f^2, h, w) -> (out_vecs, out_mask | None) on the host.  shifted: the logits sit one element and the coarse mask
    one byte into their buffers."""
    v, m = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(m, np.uint8)
    batch = v.shape[0] if v.ndim == 4 else 1
    h, w = v.shape[-3:-1]
    xm = U.to_layout(x, layout)
    arrays = (v, m, xm)
    keep = [place(a, s) for a, s in zip(arrays, (0, 1 if shifted else 0, xm.itemsize if shifted else 0))]
    if shifted:
        assert keep[2][1] % 16 == xm.itemsize and keep[1][1] % 2 == 1
    n = batch * f * h * f * w
    d_v = guarded(n * 8, GUARD, GUARD)
    d_m = guarded(n, GUARD, GUARD) if want_mask else None
    nat.check(nat.load().ofl_upsample_convex_dev(keep[0][1], keep[1][1], keep[2][1], EL[elem], LAY[layout], h, w, batch, f,
                                                 d_v.ptr + GUARD, None if d_m is None else d_m.ptr + GUARD, None))
    full = ((batch,) if v.ndim == 4 else ()) + (f * h, f * w)
    res = (read_guarded(d_v, GUARD, n * 8, GUARD, np.float32, full + (2,)), read_guarded(d_m, GUARD, n, GUARD, np.uint8, full) if want_mask else None)
    for kept, a in zip(keep, arrays):                                   # the inputs are unchanged
        got = kept[0].to_host((kept[0].nbytes,), np.uint8)[kept[1] - kept[0].ptr:][:a.nbytes]
        assert got.tobytes() == a.tobytes(), "an input was written"
    return res


def same(got, want, what):
    """out_vecs byte for byte, out_mask (where asked for) as integers"""
    assert got[0].shape == want[0].shape, what
    assert got[0].tobytes() == np.ascontiguousarray(want[0]).tobytes(), what
    if got[1] is not None:
        assert got[1].dtype == want[1].dtype
        np.testing.assert_array_equal(got[1], want[1], err_msg=what)


@functools.lru_cache(maxsize=None)
def case(shape, f, elem, spread, seed=0):
    """(v, m, logits as stored in 'chw', expected) of one generated case, computed once and shared; read-only"""
    v, m = U.vectors(shape, seed), U.coarse_mask(shape, seed)
    x, bf = U.stored(U.logits(shape, f, spread, seed), elem)
    want = U.upsample(v, m, x, f, bf)
    for a in (v, m, x) + want:
        a.setflags(write=False)
    return v, m, x, want


# ---------------------------------------------------------------------------------------------- 1: the raw ABI against the restatement
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("f", U.FACTORS)
def test_shapes(gpu, f, elem, layout):
    for k, shape in enumerate(U.SHAPES):
        for j, spread in enumerate(U.SPREADS):
            if j != k % 3 and shape not in ((2, 65), (4, 37)):         # every spread on two shapes, one spread on the others
                continue
            v, m, x, want = case(shape, f, elem, spread)
            got = raw_call(v, m, x, elem, layout, f, want_mask=(k + j) % 3 != 0, shifted=(k + j) % 2 == 1)
            same(got, want, "{} f{} {} {} spread {}".format(shape, f, elem, layout, spread))
    if elem == "float32" and f == 8:
        x = case((4, 37), 8, "float32", 200.0)[2].reshape(9, 64, 4, 37)
        t = x - x.max(0)
        assert (t < -87).any() and ((t > -87) & (t < -60)).any()       # the cut-off is met from both sides


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("f", U.FACTORS)
def test_a_batch_equals_its_items(gpu, f, layout):
    for k, shape in enumerate(((5, 130), (4, 37), (1, 1))):
        elem = ELEMS[(k + f) % 3]
        items = [case(shape, f, elem, 32.0, seed) for seed in (0, 1, 2)]
        v, m, x = (np.stack([it[i] for it in items]) for i in (0, 1, 2))
        assert not np.array_equal(v[0], v[1]) and not np.array_equal(x[1], x[2])
        got = raw_call(v, m, x, elem, layout, f, shifted=k % 2 == 0)
        for i, it in enumerate(items):
            same((got[0][i], got[1][i]), it[3], "item {} of {} f{} {}".format(i, shape, f, layout))
            same(raw_call(it[0], it[1], it[2], elem, layout, f), (got[0][i], got[1][i]), "single call {}".format(i))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("f", U.FACTORS)
def test_special_logits(gpu, f, layout):
    shape = (3, 70)
    v, m = U.vectors(shape), U.coarse_mask(shape)
    rng = np.random.default_rng(f)
    # all equal, in every element type
    for elem, value in (("float32", 0.0), ("float16", -3.5), ("bfloat16", 7.0)):
        x, bf = U.stored(np.full((9 * f * f,) + shape, value, np.float32), elem)
        same(raw_call(v, m, x, elem, layout, f, shifted=True), U.upsample(v, m, x, f, bf), "all equal " + elem)
    # float16 at its largest finite values: t = -131008 on the far side of the cut-off
    x = rng.choice(np.array([65504.0, -65504.0, 65472.0, 0.0], np.float16), (9 * f * f,) + shape)
    same(raw_call(v, m, x, "float16", layout, f), U.upsample(v, m, x, f), "float16 +-65504")


# ---------------------------------------------------------------------------------------------- 2: known answers on the device
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("f", U.FACTORS)
def test_known_answers(gpu, f, layout):
    shape = (4, 5)
    v = U.vectors(shape)
    v[v == 0] = 1.5
    ones = np.ones(shape, np.uint8)
    taps = U._taps(v, f, np.float32)
    # uniform logits: (sum of the nine u_k in order) / 9
    acc = taps[0].copy()
    for k in range(1, 9):
        acc = acc + taps[k]
    want = np.repeat(np.repeat(acc / np.float32(9.0), f, 0), f, 1)
    got = raw_call(v, ones, np.zeros((9 * f * f,) + shape, np.float32), "float32", layout, f)
    assert got[0].tobytes() == np.ascontiguousarray(want).tobytes() and got[1].all()
    # one-hot logits: exactly f * v of that neighbour, exactly 0 for a tap outside the frame
    for k, (elem, low) in itertools.product(range(9), (("float32", -1e4), ("float16", -6e4))):
        x = np.full((9, f, f) + shape, low, np.float32)
        x[k] = 0.0
        x, bf = U.stored(x.reshape((9 * f * f,) + shape), elem)
        got = raw_call(v, ones, x, elem, layout, f, want_mask=False)[0]
        dy, dx = k // 3 - 1, k % 3 - 1
        for y, xx in ((0, 0), (3, 4), (0, 2), (2, 0), (2, 2)):         # two corners, two edges, the interior
            inside = 0 <= y + dy < shape[0] and 0 <= xx + dx < shape[1]
            one = v[y + dy, xx + dx] * np.float32(f) if inside else np.zeros(2, np.float32)
            block = got[f * y:f * y + f, f * xx:f * xx + f]
            assert block.tobytes() == np.broadcast_to(one, (f, f, 2)).astype(np.float32).tobytes(), (k, elem, y, xx)


# ---------------------------------------------------------------------------------------------- 3: refusals
def test_refusals_write_nothing(gpu):
    lib = nat.load()
    shape, f = (3, 5), 2
    v, m, x, _ = case(shape, f, "float32", 1.0)
    kv, km, kx = place(v), place(m), place(x)
    n = f * f * shape[0] * shape[1]
    d_v, d_m = guarded(n * 8, GUARD, GUARD), guarded(n, GUARD, GUARD)
    ov, om = d_v.ptr + GUARD, d_m.ptr + GUARD
    good = dict(vecs=kv[1], mask=km[1], logits=kx[1], elem=nat.EL_F32, layout=nat.TENSOR_NCHW, h=3, w=5, batch=1, factor=2,
                out_vecs=ov, out_mask=om)
    order = ("vecs", "mask", "logits", "elem", "layout", "h", "w", "batch", "factor", "out_vecs", "out_mask")
    bad = [dict(factor=3), dict(factor=0), dict(factor=16), dict(elem=nat.EL_F64), dict(elem=7), dict(layout=2),
           dict(h=4096, factor=8), dict(w=16384), dict(h=0), dict(w=-1), dict(batch=0), dict(batch=65536),
           dict(vecs=None), dict(mask=None), dict(logits=None), dict(out_vecs=None),
           dict(vecs=kv[1] + 4), dict(out_vecs=ov + 4), dict(logits=kx[1] + 2),
           dict(out_vecs=kv[1]), dict(out_mask=km[1])]
    for change in bad:
        a = dict(good, **change)
        assert lib.ofl_upsample_convex_dev(*[a[k] for k in order], None) == nat.E_INVALID, change
    host = dict(good, vecs=v.ctypes.data, mask=m.ctypes.data, logits=x.ctypes.data)
    out_v, out_m = np.full((6, 10, 2), 7.0, np.float32), np.full((6, 10), 9, np.uint8)
    for change in (dict(factor=3), dict(elem=nat.EL_F64), dict(h=4096, factor=8), dict(logits=None), dict(vecs=None)):
        a = dict(host, out_vecs=out_v.ctypes.data, out_mask=out_m.ctypes.data, **change)
        assert lib.ofl_upsample_convex(*[a[k] for k in order]) == nat.E_INVALID, change
    assert (out_v == 7.0).all() and (out_m == 9).all()
    dev.sync()
    for buf in (d_v, d_m):
        assert (buf.to_host((buf.nbytes,), np.uint8) == 0xA5).all(), "a refused call wrote"
    for kept, a in ((kv, v), (km, m), (kx, x)):
        assert kept[0].to_host((a.nbytes,), np.uint8).tobytes() == a.tobytes()
    # a channel count off by one is refused where the count exists, before any launch
    field = dev.DeviceFlow.from_host(v, 't', m)
    for c in (35, 37):
        with pytest.raises(ValueError, match="36 weight channels, got {}".format(c)):
            field.upsample_convex(dev.DeviceTensor.from_host(np.zeros((c, 3, 5), np.float32)), 2)
    with pytest.raises(ValueError, match="factor must be"):
        field.upsample_convex(dev.DeviceTensor.from_host(np.zeros((81, 3, 5), np.float32)), 3)
    with pytest.raises(TypeError):
        field.upsample_convex(np.zeros((36, 3, 5), np.float32), 2)
    with pytest.raises(ValueError, match=r"\(C, h, w\)"):
        field.upsample_convex(dev.DeviceTensor.from_host(np.zeros((1, 36, 3, 5), np.float32)), 2)


# ---------------------------------------------------------------------------------------------- 4: the layers
@pytest.mark.parametrize("f", U.FACTORS)
def test_every_layer_gives_the_same_bytes(gpu, f):
    shape, n = (5, 70), 3
    items = [case(shape, f, "float16", 32.0, seed) for seed in range(n)]
    v, m, x = (np.stack([it[i] for it in items]) for i in (0, 1, 2))
    fine = (f * shape[0], f * shape[1])
    for layout in LAYOUTS:
        for ref in ('t', 's'):
            d = dev.DeviceFlow.from_host(v[0], ref, m[0]).upsample_convex(dev.DeviceTensor.from_host(U.to_layout(x[0], layout), layout), f)
            assert isinstance(d, dev.DeviceFlow) and d.shape == fine and d.ref == ref
            gv, gm = d.to_host()
            same((gv, gm.view(np.uint8)), items[0][3], "DeviceFlow " + layout)
        weights = dev.DeviceTensor.from_host(U.to_layout(x, layout), layout)
        batch = DeviceFlowBatch.from_flows([of.Flow(v[i], 's', m[i].astype(bool)) for i in range(n)])
        for b in (batch, batch.pack()):
            out = b.upsample_convex(weights, f)
            assert isinstance(out, DeviceFlowBatch) and (out.n, out.shape, out.ref, out.packed) == (n, fine, 's', False)
            gv, gm = out.vecs.to_host((n,) + fine + (2,), np.float32), out.mask.to_host((n,) + fine, np.uint8)
            for i in range(n):
                same((gv[i], gm[i]), items[i][3], "DeviceFlowBatch {} item {}".format(layout, i))
        with pytest.raises(ValueError, match="batch of 3"):
            batch.upsample_convex(dev.DeviceTensor.from_host(U.to_layout(x[:2], layout), layout), f)
    # bfloat16 through the tensor class
    xb, _ = U.stored(U.logits(shape, f, 8.0), "bfloat16")
    d = dev.DeviceFlow.from_host(v[0], 't', m[0]).upsample_convex(dev.DeviceTensor.from_host(xb, 'chw', 'bfloat16'), f)
    gv, gm = d.to_host()
    same((gv, gm.view(np.uint8)), U.upsample(v[0], m[0], xb, f, True), "bfloat16 DeviceTensor")
    # the host forms
    for xx in (x[0], x[0].astype(np.float32)):
        want = items[0][3]
        flow = of.Flow(v[0], 's', m[0].astype(bool)).upsample_convex(xx, f)
        assert isinstance(flow, of.Flow) and flow.ref == 's' and flow.shape == fine and flow.mask.dtype == np.bool_
        same((flow.vecs, flow.mask.view(np.uint8)), want, "Flow")
        gv, gm = of.upsample_flow_convex(v[0], m[0].astype(bool), xx, f)
        same((gv, gm.view(np.uint8)), want, "upsample_flow_convex")
    out_v, out_m = np.empty((n,) + fine + (2,), np.float32), np.empty((n,) + fine, np.uint8)
    xh = U.to_layout(x, 'hwc')
    nat.check(nat.load().ofl_upsample_convex(v.ctypes.data, m.ctypes.data, xh.ctypes.data, nat.EL_F16, nat.TENSOR_NHWC,
                                             shape[0], shape[1], n, f, out_v.ctypes.data, out_m.ctypes.data))
    for i in range(n):
        same((out_v[i], out_m[i]), items[i][3], "ofl_upsample_convex item {}".format(i))


# ---------------------------------------------------------------------------------------------- 5: one chain entered from outside
class Foreign:
    """a C-contiguous host array as device memory of "another framework" (tests/test_gpu_interop.py)"""

    def __init__(self, arr):
        assert arr.flags.c_contiguous
        self.buf = dev.DeviceBuffer.from_host(arr)
        self.__cuda_array_interface__ = R.cai_dict(arr, self.buf.ptr)


def test_a_chain_from_a_networks_output_to_an_exported_array(gpu):
    shape, f, n = (6, 9), 4, 2
    fine = (f * shape[0], f * shape[1])
    rng = np.random.default_rng(5)
    fwd = (np.array([0.5, -0.25]) + rng.standard_normal((n,) + shape + (2,)) * 0.02).astype(np.float32)      # nearly a translation:
    bwd = (-fwd + rng.standard_normal(fwd.shape) * 0.02).astype(np.float32)                                  # consistent inside
    xf, xb = (U.logits((n,) + shape, f, 8.0, seed).reshape(9 * f * f, n, *shape).transpose(1, 0, 2, 3).astype(np.float16) for seed in (0, 1))
    ones = np.ones(shape, np.uint8)
    up = []
    for vecs, x in ((fwd, xf), (bwd, xb)):
        coarse = DeviceFlowBatch.from_external(Foreign(np.ascontiguousarray(vecs.transpose(0, 3, 1, 2))), 't', layout='chw')
        weights = dev.DeviceTensor.from_external(Foreign(np.ascontiguousarray(x)))
        assert (coarse.n, coarse.shape) == (n, shape) and weights.shape == (n, 9 * f * f) + shape and weights.dtype == 'float16'
        up.append(coarse.upsample_convex(weights, f))
    want = [[U.upsample(vecs[i], ones, np.ascontiguousarray(x[i]), f) for i in range(n)] for vecs, x in ((fwd, xf), (bwd, xb))]
    for k in (0, 1):
        gv, gm = up[k].vecs.to_host((n,) + fine + (2,), np.float32), up[k].mask.to_host((n,) + fine, np.uint8)
        for i in range(n):
            same((gv[i], gm[i]), want[k][i], "upsampled field {} of batch {}".format(i, k))
    consistent, covered = up[0].consistency(up[1])
    got_c, got_v = consistent.to_host((n,) + fine, np.uint8), covered.to_host((n,) + fine, np.uint8)
    for i in range(n):
        wc, wv = C.consistency(want[0][i][0], want[0][i][1], want[1][i][0], want[1][i][1], -1)[:2]
        assert np.array_equal(got_v[i].astype(bool), wv) and np.array_equal(got_c[i].astype(bool), wc)
    assert got_c.any() and got_v.any()
    out = up[0].export()
    assert out.__cuda_array_interface__["shape"] == (n,) + fine + (2,) and out.__cuda_array_interface__["typestr"] == '<f4'
    assert out.to_host().tobytes() == np.stack([want[0][i][0] for i in range(n)]).tobytes()
