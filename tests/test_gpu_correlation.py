"""K18 (ofl_correlation.hip): the correlation lookup on the device, against tests/correlation_ref.py (the definition restated
operation for operation in NumPy float32) and through every layer: the raw ABI, DeviceCorrelation, DeviceTensor.correlation,
of.correlation_lookup and the host entry.  Every comparison is byte equality.  Outputs (the pooled levels included) are
written into 0xA5-filled buffers whose bytes around the output must survive, inputs are read back unchanged, and in every
second case f2 sits one element off its buffer's 16-byte alignment (which sends the call to the element-by-element kernel).

The kernel's tile is 32 pixels of ONE row, a wave takes every fourth pixel; the channels go 64 (element by element), 128 or
256 (four per load, C <= 128, C <= 256 or any C) a pass.  correlation_ref.GRIDS are a single pixel, smaller than a window,
ragged against the tile ((3, 70): two tiles and six pixels; (17, 33): one pixel past a tile), and channel_counts() puts C on
both sides of V L = 64; test_every_channel_route adds the counts that take the four-group and the any-C kernel.  Nothing is of workload size."""
import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
import correlation_ref as K
import devmem
from devmem import guarded, read_guarded
import interop_ref as R
import tensor_ref as T

pytestmark = pytest.mark.gpu
nat = of.native
GUARD = 64
EL = {"float32": nat.EL_F32, "float16": nat.EL_F16, "bfloat16": nat.EL_BF16}
NP = {"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}
PAIRS = [("float32", "float32"), ("float16", "float16"), ("bfloat16", "bfloat16"), ("float16", "float32"), ("bfloat16", "float32"),
         ("float32", "float16"), ("bfloat16", "float16")]
FIELDS = ("none", "zero", "shift", "random", "borders", "outside", "far", "huge")


def place(arr, shift=0):
    """devmem.place that also keeps the array, for `unchanged` -> (buffer, address, array)"""
    arr = np.ascontiguousarray(arr)
    return devmem.place(arr, shift) + (arr,)


def unchanged(kept):
    buf, ptr, arr = kept
    got = buf.to_host((buf.nbytes,), np.uint8)[ptr - buf.ptr:][:arr.nbytes]
    assert got.tobytes() == arr.tobytes(), "an input was written"


def depth(shape):
    """the levels a grid has: down to the one that is a single pixel wide or high"""
    h, w = shape
    levels = 1
    while h >= 2 and w >= 2 and levels < 8:
        h, w, levels = h >> 1, w >> 1, levels + 1
    return levels


def raw_lookup(f1, dt1, f2, dt2, flow, sign, r, levels, scale, order, quant, shifted=False):
    """ofl_avgpool2_dev and ofl_corr_lookup_dev on host arrays.  f1, f2: as stored, channels last, (H, W, C) or (N, H, W, C);
    flow: None, (H, W, 2) -- shared by all items -- or (N, H, W, 2).  -> (out, [pooled levels 1 ...]) on the host.
    shifted: f2 sits one element into its buffer."""
    lib = nat.load()
    batched = f1.ndim == 4
    n = f1.shape[0] if batched else 1
    h, w, c = f1.shape[-3:]
    keep = [place(f1), place(f2, np.dtype(NP[dt2]).itemsize if shifted else 0)]
    if shifted:
        assert keep[1][1] % 16 == np.dtype(NP[dt2]).itemsize
    if flow is not None:
        keep.append(place(np.ascontiguousarray(flow, np.float32)))
    shared = flow is None or flow.ndim == 3
    level_ptr, level_dt, pooled = [keep[1][1]], [dt2], []
    for l in range(1, levels):
        hl, wl = h >> l, w >> l
        buf = guarded(n * hl * wl * c * 4, GUARD, GUARD)
        nat.check(lib.ofl_avgpool2_dev(level_ptr[-1], EL[level_dt[-1]], n, c, h >> (l - 1), w >> (l - 1), buf.ptr + GUARD, None))
        pooled.append((buf, (n, hl, wl, c)))
        level_ptr.append(buf.ptr + GUARD)
        level_dt.append("float32")
    nch = (2 * r + 1) ** 2
    total = levels * nch
    out = guarded(n * total * h * w * 4, GUARD, GUARD)
    for l in range(levels):
        nat.check(lib.ofl_corr_lookup_dev(keep[0][1], EL[dt1], level_ptr[l], EL[level_dt[l]], n, c, h, w, h >> l, w >> l, l,
                                          None if flow is None else keep[2][1], 1 if shared else 0, sign, r, np.float32(scale),
                                          nat.CORR_XY if order == "xy" else nat.CORR_YX, quant, out.ptr + GUARD, total, l * nch, None))
    res = read_guarded(out, GUARD, n * total * h * w * 4, GUARD, np.float32, (n, total, h, w))
    levels_host = [read_guarded(b, GUARD, int(np.prod(s)) * 4, GUARD, np.float32, s) for b, s in pooled]
    for k in keep:
        unchanged(k)
    return (res if batched else res[0]), levels_host


def expected(f1, dt1, f2, dt2, flow, sign, r, levels, scale, order, quant):
    """-> (out, [pooled levels 1 ...]) of the restatement, for one item or a batch"""
    a, b = K.widen(f1, dt1), K.widen(f2, dt2)
    if a.ndim == 3:
        pyr = K.pyramid(b, levels)
        return K.lookup(a, b, flow, sign, r, levels, scale, order, quant, pyr), pyr[1:]
    pyr = K.pyramid(b, levels)
    pick = lambda i: None if flow is None else (flow if flow.ndim == 3 else flow[i])
    out = np.stack([K.lookup(a[i], b[i], pick(i), sign, r, levels, scale, order, quant, [p[i] for p in pyr]) for i in range(a.shape[0])])
    return out, pyr[1:]


def same(got, want, what):
    assert got[0].shape == want[0].shape, what
    assert len(got[1]) == len(want[1]), what
    for l, (g, x) in enumerate(zip(got[1], want[1])):
        assert g.reshape(x.shape).tobytes() == np.ascontiguousarray(x).tobytes(), "{}: pooled level {}".format(what, l + 1)
    assert got[0].tobytes() == np.ascontiguousarray(want[0]).tobytes(), what


def plan():
    """the cases of test_shapes: (grid, C, field, r, order, quant, levels, shifted), every grid with every channel count"""
    cases = []
    for gi, grid in enumerate(K.GRIDS):
        for ci, c in enumerate(K.channel_counts()):
            i = gi * len(K.channel_counts()) + ci
            levels = depth(grid) if c <= K.V * K.L else min(depth(grid), 2)
            k = i // len(FIELDS)                                # the k-th time this field comes up
            cases.append((grid, c, FIELDS[i % len(FIELDS)], 1 + (i + k) % 4, ("xy", "yx")[(i // 2) % 2], (i + k) % 2, levels,
                          (i + gi) % 2 == 1))
    return cases


def test_the_plan_covers_what_it_should():
    cases = plan()
    assert [depth(g) for g in K.GRIDS] == [1, 2, 3, 2, 5]
    assert {c[2] for c in cases} == set(FIELDS) and {c[3] for c in cases} == {1, 2, 3, 4}
    assert {(c[4], c[5]) for c in cases} == {("xy", 0), ("xy", 1), ("yx", 0), ("yx", 1)}
    assert {(c[7], c[1] % 4 == 0) for c in cases} == {(False, False), (False, True), (True, False), (True, True)}
    for field in FIELDS:                                        # every field meets both quant modes and several radii
        assert {c[5] for c in cases if c[2] == field} == {0, 1}, field


# ---------------------------------------------------------------------------------------------- 1: the raw ABI against the restatement
@pytest.mark.parametrize("dt1,dt2", PAIRS)
def test_shapes(gpu, dt1, dt2):
    for k, (grid, c, field, r, order, quant, levels, shifted) in enumerate(plan()):
        f1, f2 = K.features(grid, c, dt1, 0), K.features(grid, c, dt2, 1)
        flow = None if field == "none" else K.fields(grid, r)[field]
        sign = 1 if k % 2 else -1
        scale = K.default_scale(c) if k % 3 else np.float32(1.0)
        what = "{} C={} {} r={} {} quant={} levels={} shifted={} {}/{}".format(grid, c, field, r, order, quant, levels, shifted, dt1, dt2)
        got = raw_lookup(f1, dt1, f2, dt2, flow, sign, r, levels, scale, order, quant, shifted)
        same(got, expected(f1, dt1, f2, dt2, flow, sign, r, levels, scale, order, quant), what)
        if field in ("outside", "far", "huge"):                 # wholly outside: exactly 0 (level 0 for "outside", which halves with the level)
            assert not got[0][:(2 * r + 1) ** 2 if field == "outside" else None].any(), what


@pytest.mark.parametrize("c", (132, 192, 256, 260, 515, 516))
def test_every_channel_route(gpu, c):
    """128 < C <= 256 in multiples of 4 takes the kernel that holds four groups of f1 per lane (132: the third group in one lane
    only; 192: the fourth group absent; 256: full); C > 256 the one that re-reads f1 (260: the third pass holds one group;
    516: four passes and a bit); C = 515, or a shifted f2, goes by element, nine passes"""
    grid, r = (2, 35), 2
    for dt1, dt2, shifted in (("float16", "float16", False), ("float32", "bfloat16", True), ("bfloat16", "float32", False)):
        f1, f2 = K.features(grid, c, dt1, 2), K.features(grid, c, dt2, 3)
        flow = K.fields(grid, r)["random"]
        got = raw_lookup(f1, dt1, f2, dt2, flow, 1, r, 2, K.default_scale(c), "xy", nat.QUANT_EXACT, shifted)
        same(got, expected(f1, dt1, f2, dt2, flow, 1, r, 2, K.default_scale(c), "xy", nat.QUANT_EXACT), "C={} {}/{}".format(c, dt1, dt2))


# ---------------------------------------------------------------------------------------------- 2: known answers, independent of the restatement
@pytest.mark.parametrize("dt", ("float32", "float16"))
def test_known_answers(gpu, dt):
    for h, w in ((3, 4), (5, 7)):
        c = h * w
        f2 = np.eye(c, dtype=np.float32).reshape(h, w, c).astype(NP[dt])             # f2[p, idx(p)] = 1
        f1 = K.features((h, w), c, dt, 7)
        a = K.widen(f1, dt)
        scale = np.float32(0.5)
        for r, sign, order, quant, (fu, fv) in ((1, 1, "xy", 1, (1.0, -1.0)), (2, -1, "yx", 0, (2.0, 1.0)), (3, 1, "yx", 1, (0.0, 0.0)),
                                                (4, -1, "xy", 1, (-1.0, 3.0))):
            flow = np.broadcast_to(np.array([fu, fv], np.float32), (h, w, 2))
            got = raw_lookup(f1, dt, f2, dt, flow, sign, r, 1, scale, order, quant)[0].reshape(2 * r + 1, 2 * r + 1, h, w)
            want = np.zeros_like(got)
            for y in range(h):
                for x in range(w):
                    for ox in range(-r, r + 1):
                        for oy in range(-r, r + 1):
                            xx, yy = x + sign * int(fu) + ox, y + sign * int(fv) + oy
                            if 0 <= xx < w and 0 <= yy < h:
                                k = (ox + r, oy + r) if order == "xy" else (oy + r, ox + r)
                                want[k + (y, x)] = scale * (a[y, x, yy * w + xx] + np.float32(0.0))      # the blend adds + 0.0 * w
            assert got.tobytes() == want.tobytes(), (h, w, r, sign, order, quant)
    # f1 = f2, scale 1, no flow: the centre channel is sum_c f^2 in the stated order
    for c in (5, 64, 100):
        f = K.features((4, 6), c, dt, 9)
        got = raw_lookup(f, dt, f, dt, None, 1, 2, 1, np.float32(1.0), "xy", 1, shifted=c == 64)[0]
        a = K.widen(f, dt)
        assert got[12].tobytes() == K.dot(a, a).tobytes(), c


# ---------------------------------------------------------------------------------------------- 3: batches
def test_a_batch_equals_its_items_and_a_shared_field_its_copies(gpu):
    grid, c, r, levels, n = (5, 38), 70, 3, 2, 3
    for dt1, dt2 in (("float16", "float16"), ("float32", "float32")):
        f1 = np.stack([K.features(grid, c, dt1, s) for s in range(n)])
        f2 = np.stack([K.features(grid, c, dt2, 10 + s) for s in range(n)])
        flows = np.stack([K.fields(grid, r + s)["random"] for s in range(n)])
        assert not np.array_equal(flows[0], flows[1])
        args = (-1, r, levels, K.default_scale(c), "xy", nat.QUANT_EXACT)
        batch = raw_lookup(f1, dt1, f2, dt2, flows, *args)
        same(batch, expected(f1, dt1, f2, dt2, flows, *args), "batch")
        shared = raw_lookup(f1, dt1, f2, dt2, flows[1], *args, shifted=True)
        copies = raw_lookup(f1, dt1, f2, dt2, np.stack([flows[1]] * n), *args)
        assert shared[0].tobytes() == copies[0].tobytes()
        for i in range(n):
            single = raw_lookup(f1[i], dt1, f2[i], dt2, flows[i], *args)
            assert single[0].tobytes() == batch[0][i].tobytes(), i
        assert shared[0][1].tobytes() == batch[0][1].tobytes()


# ---------------------------------------------------------------------------------------------- 4: refusals
def test_refusals_write_nothing(gpu):
    lib = nat.load()
    h, w, c, r = 4, 6, 8, 1
    f1, f2, flow = K.features((h, w), c, "float32", 0), K.features((h, w), c, "float32", 1), K.fields((h, w), r)["random"]
    k1, k2, kf = place(f1), place(f2), place(flow)
    out = guarded(2 * 9 * h * w * 4, GUARD, GUARD)
    pooled = guarded(2 * 3 * c * 4, GUARD, GUARD)
    good = dict(f1=k1[1], elem1=nat.EL_F32, f2=k2[1], elem2=nat.EL_F32, N=1, C=c, H=h, W=w, Hl=h, Wl=w, level=0, flow=kf[1], shared=1,
                sign=1, r=r, scale=np.float32(1.0), order=nat.CORR_XY, quant=nat.QUANT_EXACT, out=out.ptr + GUARD, total=18, first=9)
    order = ("f1", "elem1", "f2", "elem2", "N", "C", "H", "W", "Hl", "Wl", "level", "flow", "shared", "sign", "r", "scale", "order",
             "quant", "out", "total", "first")
    assert lib.ofl_corr_lookup_dev(*[good[k] for k in order], None) == nat.OK
    dev.sync()
    nat.check(lib.ofl_memset(out.ptr, 0xA5, out.nbytes, None))
    bad = [dict(f1=None), dict(f2=None), dict(out=None), dict(elem1=nat.EL_F64), dict(elem2=nat.EL_F64), dict(elem1=7), dict(elem2=-1),
           dict(order=2), dict(quant=2), dict(sign=0), dict(r=0), dict(r=5), dict(N=0), dict(N=65536), dict(C=0), dict(C=65536),
           dict(H=0), dict(W=32767), dict(Hl=0, level=3), dict(Hl=h - 1), dict(Wl=w + 1), dict(level=1), dict(level=8), dict(level=-1),
           dict(first=10), dict(first=-1), dict(total=8, first=0), dict(out=k1[1]), dict(out=k2[1]), dict(out=kf[1]),
           dict(f1=k1[1] + 2), dict(f2=k2[1] + 1), dict(out=out.ptr + GUARD + 2), dict(flow=kf[1] + 4)]
    for change in bad:
        a = dict(good, **change)
        assert lib.ofl_corr_lookup_dev(*[a[k] for k in order], None) == nat.E_INVALID, change
    for args in ((None, nat.EL_F32, 1, c, h, w, pooled.ptr + GUARD), (k2[1], nat.EL_F64, 1, c, h, w, pooled.ptr + GUARD),
                 (k2[1], nat.EL_F32, 1, c, 1, w, pooled.ptr + GUARD), (k2[1], nat.EL_F32, 1, c, h, 1, pooled.ptr + GUARD),
                 (k2[1], nat.EL_F32, 0, c, h, w, pooled.ptr + GUARD), (k2[1], nat.EL_F32, 1, c, h, w, None),
                 (k2[1], nat.EL_F32, 1, c, h, w, k2[1]), (k2[1], nat.EL_F32, 1, c, h, w, pooled.ptr + GUARD + 2)):
        assert lib.ofl_avgpool2_dev(*args, None) == nat.E_INVALID, args
    host_out = np.full((1, 18, h, w), 7.0, np.float32)
    host = dict(f1=f1.ctypes.data, elem1=nat.EL_F32, f2=f2.ctypes.data, elem2=nat.EL_F32, N=1, C=c, H=h, W=w, levels=2,
                flow=flow.ctypes.data, shared=1, sign=1, r=r, scale=np.float32(1.0), order=nat.CORR_XY, quant=nat.QUANT_EXACT,
                out=host_out.ctypes.data)
    horder = ("f1", "elem1", "f2", "elem2", "N", "C", "H", "W", "levels", "flow", "shared", "sign", "r", "scale", "order", "quant", "out")
    for change in (dict(levels=0), dict(levels=9), dict(levels=4), dict(r=5), dict(elem2=nat.EL_F64), dict(f1=None), dict(out=None),
                   dict(order=3)):
        a = dict(host, **change)
        assert lib.ofl_corr_lookup(*[a[k] for k in horder]) == nat.E_INVALID, change
    assert (host_out == 7.0).all()
    dev.sync()
    for buf in (out, pooled):
        assert (buf.to_host((buf.nbytes,), np.uint8) == 0xA5).all(), "a refused call wrote"
    for kept in (k1, k2, kf):
        unchanged(kept)
    # the Python layers refuse before any launch
    t1 = dev.DeviceTensor.from_host(np.moveaxis(f1, -1, 0))
    with pytest.raises(ValueError, match="the same shape"):
        of.DeviceCorrelation.build(t1, dev.DeviceTensor.from_host(np.zeros((c, h, w + 1), np.float32)))
    with pytest.raises(ValueError, match="level 3 of a 4 x 6 grid is empty"):
        of.DeviceCorrelation.build(t1, t1, levels=4)
    corr = of.DeviceCorrelation.build(t1, t1, levels=2)
    with pytest.raises(ValueError, match="radius must be"):
        corr.lookup(radius=5)
    with pytest.raises(TypeError, match="flow needs to be a DeviceFlow"):
        corr.lookup(flow)
    with pytest.raises(ValueError, match="the same height and width"):
        corr.lookup(dev.DeviceFlow.from_host(np.zeros((h, w + 1, 2), np.float32), 't', np.ones((h, w + 1), bool)))
    with pytest.raises(ValueError, match="a batch of 1 fields"):
        corr.lookup(DeviceFlowBatch.from_flows([of.Flow(flow, 't')] * 2))


# ---------------------------------------------------------------------------------------------- 5: the layers
def test_every_layer_gives_the_same_bytes(gpu):
    grid, c, r, levels, n = (6, 37), 20, 2, 2, 2
    h, w = grid
    flows = np.stack([K.fields(grid, r + s)["random"] for s in range(n)])
    for dt1, dt2 in (("float16", "float16"), ("float32", "bfloat16"), ("float16", "float32")):
        f1 = np.stack([K.features(grid, c, dt1, s) for s in range(n)])
        f2 = np.stack([K.features(grid, c, dt2, 20 + s) for s in range(n)])
        tensor = lambda a, dt, layout, item=None: dev.DeviceTensor.from_host(
            np.ascontiguousarray((a if item is None else a[item]) if layout == 'hwc' else np.moveaxis(a if item is None else a[item], -1, -3)),
            layout, 'bfloat16' if dt == 'bfloat16' else None)
        for ref, sign in (('s', 1), ('t', -1)):
            for order, quant in (("xy", nat.QUANT_EXACT), ("yx", nat.QUANT_OPENCV)):
                want = raw_lookup(f1, dt1, f2, dt2, flows, sign, r, levels, K.default_scale(c), order, quant)[0]
                want_shared = raw_lookup(f1, dt1, f2, dt2, flows[0], sign, r, levels, K.default_scale(c), order, quant)[0]
                want_none = raw_lookup(f1, dt1, f2, dt2, None, sign, r, levels, K.default_scale(c), order, quant)[0]
                batch = DeviceFlowBatch.from_flows([of.Flow(flows[i], ref) for i in range(n)])
                one = dev.DeviceFlow.from_host(flows[0], ref, np.ones(grid, bool))
                for l1, l2 in (("chw", "chw"), ("hwc", "chw"), ("chw", "hwc")):
                    corr = of.DeviceCorrelation.build(tensor(f1, dt1, l1), tensor(f2, dt2, l2), levels)
                    assert corr.levels == levels
                    for flow, expect in ((batch, want), (one, want_shared), (None, want_none)):
                        out = corr.lookup(flow, r, None, order, quant)
                        assert isinstance(out, dev.DeviceTensor) and (out.shape, out.dtype, out.layout) == ((n, levels * 25, h, w), 'float32', 'chw')
                        assert out.to_host().tobytes() == expect.tobytes(), (dt1, dt2, ref, order, l1, l2)
                single = tensor(f1, dt1, "chw", 0).correlation(tensor(f2, dt2, "hwc", 0), one, r, levels, None, order, quant)
                assert single.shape == (levels * 25, h, w) and single.to_host().tobytes() == want_shared[0].tobytes()
        # the host forms: exact taps only
        if dt2 != "bfloat16":
            want = raw_lookup(f1, dt1, f2, dt2, flows[0], 1, r, levels, K.default_scale(c), "xy", nat.QUANT_EXACT)[0]
            got = of.correlation_lookup(np.moveaxis(f1[1], -1, 0), np.moveaxis(f2[1], -1, 0), flows[0], 's', r, levels)
            assert got.dtype == np.float32 and got.tobytes() == want[1].tobytes()
            got = of.correlation_lookup(np.moveaxis(f1[0], -1, 0), np.moveaxis(f2[0], -1, 0), None, 't', r, levels, 2.0, 'yx')
            assert got.tobytes() == raw_lookup(f1[0], dt1, f2[0], dt2, None, -1, r, levels, 2.0, "yx", nat.QUANT_EXACT)[0].tobytes()
        out = np.empty((n, levels * 25, h, w), np.float32)
        nat.check(nat.load().ofl_corr_lookup(f1.ctypes.data, EL[dt1], f2.ctypes.data, EL[dt2], n, c, h, w, levels, flows.ctypes.data, 0,
                                             -1, r, K.default_scale(c), nat.CORR_YX, nat.QUANT_OPENCV, out.ctypes.data))
        assert out.tobytes() == raw_lookup(f1, dt1, f2, dt2, flows, -1, r, levels, K.default_scale(c), "yx", nat.QUANT_OPENCV)[0].tobytes()


# ---------------------------------------------------------------------------------------------- 6: one chain entered from outside
class Foreign:
    """a C-contiguous host array as device memory of "another framework" (tests/test_gpu_interop.py)"""

    def __init__(self, arr):
        assert arr.flags.c_contiguous
        self.buf = dev.DeviceBuffer.from_host(arr)
        self.__cuda_array_interface__ = R.cai_dict(arr, self.buf.ptr)


def test_a_chain_from_foreign_tensors_to_a_cost_volume(gpu):
    """PWC-Net's step: the second frame's features warped by the current flow, then the local cost volume"""
    grid, c, r = (9, 14), 12, 4
    rng = np.random.default_rng(11)
    a1 = rng.standard_normal((c,) + grid).astype(np.float16)
    a2 = rng.standard_normal((c,) + grid).astype(np.float16)
    vecs = T.flow('wobble', grid) * np.float32(0.7) + np.float32(0.3)
    t1, t2 = dev.DeviceTensor.from_external(Foreign(a1)), dev.DeviceTensor.from_external(Foreign(a2))
    warped, valid = dev.DeviceFlow.from_host(vecs, 't', np.ones(grid, bool)).apply_tensor(t2)
    cost = t1.correlation(warped, flow=None, radius=r, levels=1, order='yx')
    assert cost.shape == (81,) + grid
    want_warp, _ = T.warp(a2, 'float16', 'chw', vecs, np.ones(grid, bool))
    assert warped.to_host().tobytes() == want_warp.tobytes()
    want = K.lookup(np.moveaxis(a1, 0, -1).astype(np.float32), np.moveaxis(want_warp, 0, -1).astype(np.float32), None, 1, r, 1, None, "yx")
    assert cost.to_host().tobytes() == want.tobytes()
    assert np.abs(want).max() > 0
