"""K19 (ofl_match.hip): global matching on the device, against tests/match_ref.py (the definition restated in NumPy) and
through every layer: the raw ABI, DeviceCorrelation.match, DeviceTensor.match, of.global_match and the host entry.  Outputs
are written into 0xA5-filled buffers whose bytes around the output must survive, inputs are read back unchanged, and in
every second case both tensors sit one element off their buffers' 16-byte alignment (which sends the call to the
element-by-element kernel).

1  Integer-valued features: every partial sum of a dot is an exact float32 integer, so D is exact in any accumulation order
   and everything after it is stated: vectors, mask, confidence and index equal the restatement BYTE FOR BYTE, in all three
   element types.  This is also the check of the operand lane maps of the three MFMAs (f1 != f2, H != W).
2  Random float features: within match_ref.bound of the float64 definition.  For float32 the bound is derived; the 16-bit
   MFMA's internal accumulation order is not documented, the same derived bound (any order, every addition rounded) is used
   and FACTOR_16 is the place where a measured factor would go -- it is 1: the derived bound held on the device.
3  Every layer gives the same bytes; reverse, 't', batches, layouts, mixed dtypes.

The kernel's tile is 32 keys; the four waves of a workgroup share 32 queries -- or 64, two blocks a wave, once the launch
still has a workgroup per CU (test_integer_features_two_query_blocks_a_wave) -- and take tile j mod 4 (a round is 128 keys);
a lane's keys span 28, so W >= 28 wraps once and W < 28 divides.  match_ref.GRIDS: one pixel; 31 / 32 / 33 keys; (5, 7) and
(3, 27) with W < 28, (3, 28) on the other side; (2, 64) one round exactly, (5, 26) a round and two keys; (3, 70) six tiles and
a bit (wave 0 and 1 take a second tile, 2 and 3 do not: 7 query blocks); (17, 33) and (24, 40): 18 and 30 query blocks, 8 / 7
tiles a wave.  match_ref.CHANNELS: both sides of the 16-bit step 16 and the float32 chunk 4, of the register-held limits
(float32 64 / 68, 16-bit 128 / 136), odd counts (element by element), 512.  Nothing is of workload size."""
import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
import devmem
from devmem import guarded, read_guarded
import match_ref as M

pytestmark = pytest.mark.gpu
nat = of.native
GUARD = 64
EL = {"float32": nat.EL_F32, "float16": nat.EL_F16, "bfloat16": nat.EL_BF16}
NP = {"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}
DTYPES = ("float32", "float16", "bfloat16")
FACTOR_16 = 1.0                 # times the derived bound for float16 / bfloat16 (see 2 above)


def place(arr, shift=0):
    arr = np.ascontiguousarray(arr)
    return devmem.place(arr, shift) + (arr,)


def unchanged(kept):
    buf, ptr, arr = kept
    got = buf.to_host((buf.nbytes,), np.uint8)[ptr - buf.ptr:][:arr.nbytes]
    assert got.tobytes() == arr.tobytes(), "an input was written"


def raw_match(f1, f2, dt, scale=None, sign=1, min_conf=0.0, shifted=False, extras=True):
    """ofl_global_match_dev on host arrays as stored, channels last, (H, W, C) or (N, H, W, C) -> (vecs, mask, conf, index)
    on the host (conf, index None without extras).  shifted: both tensors sit one element into their buffers."""
    batched = f1.ndim == 4
    n = f1.shape[0] if batched else 1
    h, w, c = f1.shape[-3:]
    item = np.dtype(NP[dt]).itemsize
    keep = [place(f1, item if shifted else 0), place(f2, item if shifted else 0)]
    assert all(k[1] % 16 == (item if shifted else 0) for k in keep)
    px = n * h * w
    scale = M.default_scale(c) if scale is None else np.float32(scale)
    ov, om = guarded(px * 8, GUARD, GUARD), guarded(px, GUARD, GUARD)
    oc, oi = (guarded(px * 4, GUARD, GUARD), guarded(px * 4, GUARD, GUARD)) if extras else (None, None)
    nat.check(nat.load().ofl_global_match_dev(keep[0][1], keep[1][1], EL[dt], n, c, h, w, scale, sign, np.float32(min_conf),
                                              ov.ptr + GUARD, om.ptr + GUARD, oc.ptr + GUARD if extras else None,
                                              oi.ptr + GUARD if extras else None, None))
    shape = (n, h, w) if batched else (h, w)
    out = (read_guarded(ov, GUARD, px * 8, GUARD, np.float32, shape + (2,)), read_guarded(om, GUARD, px, GUARD, np.uint8, shape),
           read_guarded(oc, GUARD, px * 4, GUARD, np.float32, shape) if extras else None,
           read_guarded(oi, GUARD, px * 4, GUARD, np.int32, shape) if extras else None)
    for k in keep:
        unchanged(k)
    return out


def same(got, want, what):
    for name, g, x in zip(("vecs", "mask", "conf", "index"), got, want):
        assert g.shape == x.shape and g.tobytes() == np.ascontiguousarray(x).tobytes(), "{}: {}".format(what, name)


def plan():
    """the cases of test_integer_features: (grid, C, reach, shifted).  (5, 7) and (3, 70) meet every channel count, the other
    grids every fourth, rotating; reach and shift alternate so that each route meets both."""
    cases = []
    for gi, grid in enumerate(M.GRIDS):
        for ci, c in enumerate(M.CHANNELS):
            if grid in ((5, 7), (3, 70)) or (ci + gi) % 4 == 0:
                i = len(cases)
                cases.append((grid, c, (2, 8)[(i // 2 + gi) % 2], i % 2 == 1))
    return cases


def test_the_plan_covers_what_it_should():
    cases = plan()
    assert {c[0] for c in cases} == set(M.GRIDS) and {c[1] for c in cases} == set(M.CHANNELS)
    assert {(c[2], c[3]) for c in cases} == {(2, False), (2, True), (8, False), (8, True)}
    for held in (True, False):                                  # aligned, C % 8 == 0, on both sides of 64 and 128, in both ranges
        for limit in (64, 128):
            assert {c[2] for c in cases if not c[3] and c[1] % 8 == 0 and (c[1] <= limit) == held} == {2, 8}, (held, limit)
    assert len(cases) <= 80


# ---------------------------------------------------------------------------------------------- 1: byte equality on integer features
@pytest.mark.parametrize("dt", DTYPES)
def test_integer_features(gpu, dt):
    for grid, c, reach, shifted in plan():
        f1, f2 = M.int_features(grid, c, dt, reach, 0), M.int_features(grid, c, dt, reach, 1)
        scale = None if reach == 2 else 1.0                     # reach 8 at scale 1: logits in the thousands, most tiles cut
        sign = 1 if (c + grid[1]) % 2 else -1
        what = "{} C={} reach={} shifted={} {}".format(grid, c, reach, shifted, dt)
        got = raw_match(f1, f2, dt, scale, sign, 0.0, shifted)
        want = M.match(M.widen(f1, dt), M.widen(f2, dt), scale, sign)
        same(got, want, what)
        assert np.isfinite(got[0]).all() and got[1].all(), what
        if grid == (1, 1):
            assert not got[0].any() and got[2][0, 0] == 1.0 and got[3][0, 0] == 0


@pytest.mark.parametrize("dt", DTYPES)
def test_integer_features_two_query_blocks_a_wave(gpu, dt):
    """A wave holds two query blocks (64 queries a workgroup) once that leaves a workgroup per CU: 64 items of a small grid get
    there.  (5, 41): 205 queries, the last workgroup's second block lies wholly beyond H W; (4, 65): 260, four queries in a
    fifth workgroup.  An item alone takes one block a wave and must give the same bytes."""
    import re
    cus = int(re.search(r"(\d+) CUs", nat.device_name()).group(1))
    n = 64
    for k, (grid, c) in enumerate((((5, 41), 20), ((4, 65), 128), ((5, 41), 136), ((4, 65), 3), ((5, 41), 64), ((4, 65), 72))):
        assert n * -(-grid[0] * grid[1] // 64) >= cus, "this machine would not take the two-block kernel"
        reach, shifted = (2, 8)[k % 2], k % 3 == 1
        f1 = np.stack([M.int_features(grid, c, dt, reach, 2 * i) for i in range(n)])
        f2 = np.stack([M.int_features(grid, c, dt, reach, 2 * i + 1) for i in range(n)])
        scale = None if reach == 2 else 1.0
        got = raw_match(f1, f2, dt, scale, 1, 0.0, shifted)
        want = M.match_batch(M.widen(f1, dt), M.widen(f2, dt), scale=scale)
        same(got, want, "{} C={} reach={} shifted={} {}".format(grid, c, reach, shifted, dt))
        alone = raw_match(f1[5], f2[5], dt, scale, 1, 0.0, shifted)
        assert all(alone[j].tobytes() == got[j][5].tobytes() for j in range(4))


# ---------------------------------------------------------------------------------------------- 2: random features against float64
@pytest.mark.parametrize("dt", DTYPES)
def test_random_features_are_within_the_bound_of_float64(gpu, dt):
    worst = 0.0
    factor = 1.0 if dt == "float32" else FACTOR_16
    for gi, grid in enumerate(((1, 33), (5, 7), (3, 28), (3, 70), (17, 33), (24, 40))):
        h, w = grid
        for ci, c in enumerate(M.CHANNELS):
            if (ci + gi) % 3:
                continue
            f1, f2 = M.features(grid, c, dt, 2 * ci), M.features(grid, c, dt, 2 * ci + 1)
            a, b = M.widen(f1, dt), M.widen(f2, dt)
            scale = None if ci % 2 else 1.0
            sc = M.default_scale(c) if scale is None else np.float32(scale)
            vecs, mask, conf, index = raw_match(f1, f2, dt, scale, 1, 0.0, (ci + gi) % 2 == 1)
            want, conf64, s64 = M.match64(a, b, scale)
            mag = M.magnitude(a, b)
            bound, cbound = factor * M.bound(c, h, w, sc, mag), factor * M.conf_bound(c, h, w, sc, mag)
            err = float(np.abs(vecs.astype(np.float64) - want).max())
            cerr = float((np.abs(conf.astype(np.float64) - conf64) / conf64).max())
            worst = max(worst, err / bound, cerr / cbound)
            print("{} C={} {}: error {:.3e} of bound {:.3e}, confidence {:.3e} of {:.3e}".format(grid, c, dt, err, bound, cerr, cbound))
            assert err <= bound and cerr <= cbound, (grid, c, dt, err, bound, cerr, cbound)
            delta = (c + 1) * M.EPS * float(sc) * mag
            assert ((index >= 0) & (index < h * w)).all() and mask.all()
            assert (s64[np.arange(h * w), index.ravel()] >= s64.max(1) - 2 * factor * delta).all(), (grid, c, dt)
    print("{}: worst ratio to the bound {:.3f}".format(dt, worst))


# ---------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("dt", DTYPES)
def test_known_answers(gpu, dt):
    conv = lambda a: np.ascontiguousarray(M.K.R.from_f32(a, dt))
    # all-zero features: index 0, confidence 1 / (H W) as rounded, the mean coordinate
    for (h, w), shifted in (((1, 1), False), ((3, 5), True), ((6, 40), False)):
        z = conv(np.zeros((h, w, 8), np.float32))
        vecs, mask, conf, index = raw_match(z, z, dt, None, 1, 0.0, shifted)
        gy, gx = np.mgrid[:h, :w]
        assert not index.any() and mask.all()
        assert conf.tobytes() == np.full((h, w), np.float32(1.0) / np.float32(h * w), np.float32).tobytes()
        assert np.array_equal(vecs[..., 0], np.float32((w - 1) / 2) - gx) and np.array_equal(vecs[..., 1], np.float32((h - 1) / 2) - gy)
    # a duplicated key: the lower index
    f1, f2 = M.widen(M.int_features((4, 9), 6, "float32", 2, 1), "float32"), M.widen(M.int_features((4, 9), 6, "float32", 2, 2), "float32")
    f2[3, 4] = f2[1, 2] = 3 * f1[2, 2]
    assert raw_match(conv(f1), conv(f2), dt)[3][2, 2] == 11
    # a shift, one-hot features, the other logits 100 below
    shape, (dx, dy) = (5, 7), (2, 1)
    h, w = shape
    f1, f2 = (conv(a) for a in M.one_hot_pair(shape, (dx, dy)))
    gy, gx = np.mgrid[:h, :w]
    inside = (gx + dx < w) & (gy + dy < h)
    for sign in (1, -1):
        vecs, mask, conf, index = raw_match(f1, f2, dt, 100.0, sign, 1.0, sign < 0)
        assert np.array_equal(index, ((gy + dy) % h) * w + (gx + dx) % w)
        assert (conf == 1.0).all() and mask.all()                                   # min_conf = 1 and conf = 1: >=
        assert np.array_equal(vecs[inside], np.broadcast_to(np.float32([sign * dx, sign * dy]), (inside.sum(), 2)))
    # min_conf between two confidences that occur
    f1, f2 = M.features((5, 7), 8, dt, 0), M.features((5, 7), 8, dt, 1)
    conf = raw_match(f1, f2, dt)[2]
    order = np.sort(conf.ravel())
    assert order[10] < order[11]
    thr = np.float32((np.float64(order[10]) + np.float64(order[11])) / 2)
    vecs, mask, conf2, _ = raw_match(f1, f2, dt, None, 1, thr)
    assert conf2.tobytes() == conf.tobytes() and mask.sum() == 35 - 11 and np.array_equal(mask != 0, conf >= thr)
    assert np.array_equal(raw_match(f1, f2, dt, None, 1, order[11], extras=False)[1] != 0, conf >= order[11])


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing(gpu):
    lib = nat.load()
    h, w, c = 4, 6, 8
    f1, f2 = M.features((h, w), c, "float32", 0), M.features((h, w), c, "float32", 1)
    k1, k2 = place(f1), place(f2)
    px = h * w
    ov, om, oc, oi = guarded(px * 8, GUARD, GUARD), guarded(px, GUARD, GUARD), guarded(px * 4, GUARD, GUARD), guarded(px * 4, GUARD, GUARD)
    good = dict(f1=k1[1], f2=k2[1], elem=nat.EL_F32, N=1, C=c, H=h, W=w, scale=np.float32(1.0), sign=1, min_conf=np.float32(0.0),
                vecs=ov.ptr + GUARD, mask=om.ptr + GUARD, conf=oc.ptr + GUARD, index=oi.ptr + GUARD)
    order = ("f1", "f2", "elem", "N", "C", "H", "W", "scale", "sign", "min_conf", "vecs", "mask", "conf", "index")
    assert lib.ofl_global_match_dev(*[good[k] for k in order], None) == nat.OK
    dev.sync()
    for buf in (ov, om, oc, oi):
        nat.check(lib.ofl_memset(buf.ptr, 0xA5, buf.nbytes, None))
    bad = [dict(f1=None), dict(f2=None), dict(vecs=None), dict(mask=None), dict(elem=nat.EL_F64), dict(elem=7), dict(elem=-1),
           dict(sign=0), dict(sign=2), dict(min_conf=np.float32(-0.5)), dict(min_conf=np.float32(np.nan)), dict(N=0), dict(N=65536),
           dict(C=0), dict(C=513), dict(H=0), dict(W=32767), dict(vecs=k1[1]), dict(mask=k2[1]), dict(conf=k1[1]), dict(index=k2[1]),
           dict(conf=ov.ptr + GUARD), dict(index=oc.ptr + GUARD), dict(f1=k1[1] + 2), dict(f2=k2[1] + 1), dict(vecs=ov.ptr + GUARD + 4),
           dict(conf=oc.ptr + GUARD + 2), dict(index=oi.ptr + GUARD + 1)]
    for change in bad:
        a = dict(good, **change)
        assert lib.ofl_global_match_dev(*[a[k] for k in order], None) == nat.E_INVALID, change
    hv, hm = np.full((h, w, 2), 7.0, np.float32), np.full((h, w), 7, np.uint8)
    host = dict(good, f1=f1.ctypes.data, f2=f2.ctypes.data, vecs=hv.ctypes.data, mask=hm.ctypes.data, conf=None, index=None)
    for change in (dict(elem=nat.EL_F64), dict(f1=None), dict(vecs=None), dict(sign=0), dict(C=513), dict(min_conf=np.float32(np.nan))):
        a = dict(host, **change)
        assert lib.ofl_global_match(*[a[k] for k in order]) == nat.E_INVALID, change
    assert (hv == 7.0).all() and (hm == 7).all()
    dev.sync()
    for buf in (ov, om, oc, oi):
        assert (buf.to_host((buf.nbytes,), np.uint8) == 0xA5).all(), "a refused call wrote"
    for kept in (k1, k2):
        unchanged(kept)


# ---------------------------------------------------------------------------------------------- 3: the layers
def test_every_layer_gives_the_same_bytes(gpu):
    grid, c, n = (6, 37), 20, 3
    h, w = grid
    tensor = lambda a, dt, layout, item=None: dev.DeviceTensor.from_host(
        np.ascontiguousarray((a if item is None else a[item]) if layout == 'hwc' else np.moveaxis(a if item is None else a[item], -1, -3)),
        layout, 'bfloat16' if dt == 'bfloat16' else None)
    for dt in DTYPES:
        f1 = np.stack([M.features(grid, c, dt, s) for s in range(n)])
        f2 = np.stack([M.features(grid, c, dt, 20 + s) for s in range(n)])
        fwd = raw_match(f1, f2, dt)
        bwd = raw_match(f2, f1, dt)
        neg = raw_match(f1, f2, dt, None, -1)
        assert neg[0].tobytes() == (-fwd[0]).tobytes() and all(neg[k].tobytes() == fwd[k].tobytes() for k in (1, 2, 3))      # 't' = -'s'
        assert fwd[0].tobytes() != bwd[0].tobytes()
        for i in range(n):                                                           # item i of a batch is the item alone
            single = raw_match(f1[i], f2[i], dt, shifted=i == 1)
            assert all(single[k].tobytes() == fwd[k][i].tobytes() for k in range(4)), (dt, i)
        thr = np.float32(np.median(raw_match(f1, f2, dt, 2.0)[2]))                    # a confidence that occurs at scale 2
        cut = raw_match(f1, f2, dt, 2.0, 1, thr)
        for l1, l2 in (("chw", "chw"), ("hwc", "chw"), ("chw", "hwc")):               # planar and channels-last inputs agree
            corr = of.DeviceCorrelation.build(tensor(f1, dt, l1), tensor(f2, dt, l2), 2)
            flow = corr.match()
            assert isinstance(flow, DeviceFlowBatch) and (flow.n, flow.shape, flow.ref) == (n, grid, 's')
            assert flow.vecs.to_host((n, h, w, 2), np.float32).tobytes() == fwd[0].tobytes()
            assert flow.mask.to_host((n, h, w), np.uint8).tobytes() == fwd[1].tobytes()
            flow, conf, index = corr.match('t', None, True, None, True, True)        # reverse = the tensors swapped
            assert flow.ref == 't' and flow.vecs.to_host((n, h, w, 2), np.float32).tobytes() == (-bwd[0]).tobytes()
            assert conf.to_host((n, h, w), np.float32).tobytes() == bwd[2].tobytes()
            assert index.to_host((n, h, w), np.int32).tobytes() == bwd[3].tobytes()
            flow, conf = corr.match(scale=2.0, min_confidence=float(thr), return_confidence=True)
            assert flow.vecs.to_host((n, h, w, 2), np.float32).tobytes() == cut[0].tobytes()
            assert flow.mask.to_host((n, h, w), np.uint8).tobytes() == cut[1].tobytes() and 0 < cut[1].sum() < cut[1].size
            assert conf.to_host((n, h, w), np.float32).tobytes() == cut[2].tobytes()
        one, index = tensor(f1, dt, "chw", 1).match(tensor(f2, dt, "hwc", 1), return_index=True)
        assert isinstance(one, dev.DeviceFlow) and one.shape == grid and one.ref == 's'
        assert one.vecs.to_host((h, w, 2), np.float32).tobytes() == fwd[0][1].tobytes()
        assert index.to_host((h, w), np.int32).tobytes() == fwd[3][1].tobytes()
        back = tensor(f1, dt, "hwc", 2).match(tensor(f2, dt, "chw", 2), 't', reverse=True)
        assert back.vecs.to_host((h, w, 2), np.float32).tobytes() == (-bwd[0][2]).tobytes()
        # the host forms
        if dt != "bfloat16":
            got, conf, index = of.global_match(np.moveaxis(f1[1], -1, 0), np.moveaxis(f2[1], -1, 0), return_confidence=True, return_index=True)
            assert isinstance(got, of.Flow) and got.ref == 's' and got.vecs.tobytes() == fwd[0][1].tobytes() and got.mask.all()
            assert conf.tobytes() == fwd[2][1].tobytes() and index.tobytes() == fwd[3][1].tobytes()
            got = of.global_match(np.moveaxis(f1[0], -1, 0), np.moveaxis(f2[0], -1, 0), 't', 2.0, float(thr))
            assert got.ref == 't' and got.vecs.tobytes() == (-cut[0][0]).tobytes() and np.array_equal(got.mask, cut[1][0] != 0)
        hv, hm = np.empty((n, h, w, 2), np.float32), np.empty((n, h, w), np.uint8)
        hc, hi = np.empty((n, h, w), np.float32), np.empty((n, h, w), np.int32)
        nat.check(nat.load().ofl_global_match(f1.ctypes.data, f2.ctypes.data, EL[dt], n, c, h, w, M.default_scale(c), 1, np.float32(0.0),
                                              hv.ctypes.data, hm.ctypes.data, hc.ctypes.data, hi.ctypes.data))
        same((hv, hm, hc, hi), fwd, "host entry " + dt)
    # mixed dtypes, which build accepts for lookup, raise with both names
    a, b = M.features(grid, c, "float16", 0), M.features(grid, c, "float32", 1)
    corr = of.DeviceCorrelation.build(tensor(a, "float16", "hwc"), tensor(b, "float32", "hwc"), 1)
    with pytest.raises(ValueError, match="the same dtype, got float16 and float32"):
        corr.match()
    with pytest.raises(ValueError, match="Input is not 's' or 't'"):
        of.DeviceCorrelation.build(tensor(b, "float32", "hwc"), tensor(b, "float32", "hwc"), 1).match('x')
    with pytest.raises(TypeError, match="reverse needs to be a boolean"):
        of.DeviceCorrelation.build(tensor(b, "float32", "hwc"), tensor(b, "float32", "hwc"), 1).match(reverse=1)


def test_a_forward_backward_pair_feeds_the_consistency_check(gpu):
    """the chain the feature exists for: match both ways, then K13 on the two fields"""
    shape, (dx, dy) = (6, 9), (2, 1)
    f1, f2 = M.one_hot_pair(shape, (dx, dy))
    t1, t2 = dev.DeviceTensor.from_host(f1, 'hwc'), dev.DeviceTensor.from_host(f2, 'hwc')
    corr = of.DeviceCorrelation.build(t1, t2, 1)
    fwd, bwd = corr.match('s', 100.0), corr.match('s', 100.0, reverse=True)
    consistent = fwd.consistency(bwd)[0].to_host(shape, np.uint8)
    gy, gx = np.mgrid[:shape[0], :shape[1]]
    inside = (gx + dx < shape[1]) & (gy + dy < shape[0])
    assert (consistent[inside] != 0).all()
