"""K16 (ofl_median.hip): the mask-aware median filter on the device, against tests/median_ref.py (the definition by brute force)
and through every layer: the raw ABI, DeviceFlow.median, DeviceFlowBatch.median, Flow.median, median_flow and the host entry.
Every output word is a moved input word: every comparison is byte equality or array_equal.  Outputs are written into
0xA5-filled buffers whose bytes around the output must survive, inputs are read back unchanged, masks also sit at odd
addresses.  The kernel's tile is 64 x 16 pixels, so the shapes of median_ref.SHAPES are smaller than a window, ragged against
a tile and more than two tiles in each axis; no larger tile, no further shapes."""
import itertools

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
import consistency_ref as C
from devmem import guarded, place, read_guarded
import fill_ref as F
import median_ref as M

pytestmark = pytest.mark.gpu
nat = of.native
GUARD = 64
COMBOS = list(itertools.product((False, True), repeat=3))          # valid, only, out_mask: the eight instantiations per ksize


def raw_call(vecs, mask, valid, only, shape, ksize, min_count=1, batch=1, want_mask=True, mask_shift=0, out_shift=0):
    """ofl_median_dev on host arrays -> (out_vecs, out_mask | None) on the host.  mask sits mask_shift bytes, valid
    mask_shift + 2 and only mask_shift + 4 bytes into their buffers, out_mask out_shift bytes into its own."""
    h, w = shape
    n = batch * h * w
    arrays = (vecs, mask, valid, only)
    keep = [None if a is None else place(a, s) for a, s in zip(arrays, (0, mask_shift, mask_shift + 2, mask_shift + 4))]
    if mask_shift % 2:
        assert keep[1][1] % 2 == 1
    d_v = guarded(n * 8, GUARD)
    d_m = guarded(n, GUARD, out_shift) if want_mask else None
    addr = lambda k: None if k is None else k[1]
    nat.check(nat.load().ofl_median_dev(addr(keep[0]), addr(keep[1]), addr(keep[2]), addr(keep[3]), h, w, batch, ksize, min_count,
                                        d_v.ptr, None if d_m is None else d_m.ptr + out_shift, None))
    full = (batch, h, w) if batch > 1 else (h, w)
    res = (read_guarded(d_v, 0, n * 8, GUARD, np.float32, full + (2,)), read_guarded(d_m, out_shift, n, GUARD, np.uint8, full) if want_mask else None)
    for kept, a in zip(keep, arrays):                                   # the inputs are unchanged
        if kept is not None:
            a = np.ascontiguousarray(a)
            got = kept[0].to_host((kept[0].nbytes,), np.uint8)[kept[1] - kept[0].ptr:][:a.nbytes]
            assert got.tobytes() == a.tobytes(), "an input was written"
    return res


def same(got, want, what):
    """out_vecs byte for byte, out_mask (where asked for) as integers"""
    assert got[0].tobytes() == np.ascontiguousarray(want[0]).tobytes(), what
    if got[1] is not None:
        assert got[1].dtype == want[1].dtype
        np.testing.assert_array_equal(got[1], want[1], err_msg=what)


def extras(shape, seed=41):
    rng = np.random.default_rng(seed + shape[0] * 7 + shape[1])
    return (rng.random(shape) < 0.7).astype(np.uint8), (rng.random(shape) < 0.5).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- 1: the raw ABI against the restatement
@pytest.mark.parametrize("ksize", M.KSIZES)
def test_shapes(gpu, ksize):
    for k, shape in enumerate(M.SHAPES):
        v = M.vectors(shape)
        valid, only = extras(shape)
        for j, name in enumerate(("random50", "all")):
            m = M.mask(name, shape)
            what = "{} {} k{}".format(shape, name, ksize)
            same(raw_call(v, m, None, None, shape, ksize, mask_shift=(k + j) % 2, out_shift=(3, 0, 1)[k % 3]), M.expected(name, shape, ksize), what)
            use_valid, use_only, want_mask = COMBOS[(3 * k + 5 * j + ksize) % 8]
            want = M.median(v, m, ksize, valid if use_valid else None, only if use_only else None, 2)
            same(raw_call(v, m, valid if use_valid else None, only if use_only else None, shape, ksize, 2, want_mask=want_mask, mask_shift=1),
                 want, what + " {}".format((use_valid, use_only, want_mask)))
    # 1 x 1: its own median, or nothing
    v = M.vectors((1, 1))
    got = raw_call(v, np.ones((1, 1), np.uint8), None, None, (1, 1), ksize)
    assert got[0].tobytes() == v.tobytes() and got[1].tolist() == [[1]]
    got = raw_call(v, np.zeros((1, 1), np.uint8), None, None, (1, 1), ksize)
    assert got[0].tobytes() == v.tobytes() and got[1].tolist() == [[0]]


@pytest.mark.parametrize("ksize", M.KSIZES)
def test_masks_with_and_without_valid_only_and_out_mask(gpu, ksize):
    shape = (33, 65)                                                   # three tiles down, two across, both ragged
    v = M.vectors(shape)
    valid, only = extras(shape)
    for name in M.MASKS:
        m = M.mask(name, shape)
        plain = M.expected(name, shape, ksize)
        for k, (use_valid, use_only, want_mask) in enumerate(COMBOS):
            va, on = valid if use_valid else None, only if use_only else None
            want = plain if va is None and on is None else M.median(v, m, ksize, va, on)
            got = raw_call(v, m, va, on, shape, ksize, want_mask=want_mask, mask_shift=k % 2, out_shift=k % 3)
            assert (got[1] is not None) is want_mask
            same(got, want, "{} k{} {}".format(name, ksize, (use_valid, use_only, want_mask)))
        n = plain[2]
        if name == "random5" and ksize == 3:
            assert (n == 0).mean() >= 1 / 3
        if name == "checker" and ksize == 3:
            assert set(np.unique(n[1:-1, 1:-1])) == {4, 5}             # 4 around an unset centre: an even count, the lower median
        if name == "none":
            got = raw_call(v, m, None, None, shape, ksize)
            assert got[0].tobytes() == v.tobytes() and not got[1].any()
        if name == "one":
            got = raw_call(v, m, None, None, shape, ksize)
            r = ksize // 2
            y, x = np.argwhere(m)[0]
            assert int(got[1].sum()) == ksize * ksize and got[1][y - r:y + r + 1, x - r:x + r + 1].all()
            assert got[0][y - r:y + r + 1, x - r:x + r + 1].tobytes() == np.broadcast_to(v[y, x], (ksize, ksize, 2)).tobytes()
    # valid bytes other than 0 / 1 are ANDed bit by bit with the mask byte; only is compared with 0
    m = np.full(shape, 1, np.uint8)
    same(raw_call(v, m, np.where(valid == 1, 3, 2).astype(np.uint8), np.where(only == 1, 0x80, 0).astype(np.uint8), shape, ksize),
         M.median(v, m, ksize, valid, only), "bitwise")


@pytest.mark.parametrize("ksize", M.KSIZES)
def test_special_values_and_min_count(gpu, ksize):
    shape = (67, 259)
    v = M.vectors(shape)
    words = v.view(np.uint32)
    assert all((words == s).sum() > 20 for s in M.SPECIAL)            # NaNs of both signs and several payloads, +-Inf, +-0.0, denormals
    valid, only = extras(shape)
    for min_count in (1, 2, ksize * ksize, ksize * ksize // 2):
        for name in ("all", "random50"):
            want = M.expected(name, shape, ksize, min_count)
            got = raw_call(v, M.mask(name, shape), None, None, shape, ksize, min_count, mask_shift=1, out_shift=1)
            same(got, want, "{} k{} min_count {}".format(name, ksize, min_count))
            if name == "all":
                assert got[1].all() == (min_count <= (ksize // 2 + 1) ** 2) and got[1][ksize:-ksize, ksize:-ksize].all()   # the corners see (r + 1)^2
        m = M.mask("random50", shape)
        same(raw_call(v, m, valid, only, shape, ksize, min_count), M.median(v, m, ksize, valid, only, min_count), "valid, only")
    # every output word is a word of the input
    got = raw_call(v, M.mask("random5", shape), None, None, shape, ksize)
    assert np.isin(got[0].view(np.uint32), words).all()
    assert sum(int((got[0].view(np.uint32) == s).sum()) for s in M.SPECIAL[:5]) > 20                # NaN payloads came through


# ---------------------------------------------------------------------------------------------- 2: batches
@pytest.mark.parametrize("shape", [(5, 7), (33, 65)])
def test_three_fields_in_one_launch_equal_three_launches(gpu, shape):
    assert shape[0] * shape[1] % 2 == 1                                # every second field sits at an odd address
    names = ("random50", "all", "random5")
    vs = [M.vectors(shape, seed) for seed in (1, 2, 3)]
    ms = [M.mask(name, shape, seed=k) for k, name in enumerate(names)]
    valids, onlys = zip(*[extras(shape, seed) for seed in (1, 2, 3)])
    for ksize in M.KSIZES:
        for use, min_count in ((False, 1), (True, 1), (True, 3)):
            va, on = (np.stack(valids), np.stack(onlys)) if use else (None, None)
            got = raw_call(np.stack(vs), np.stack(ms), va, on, shape, ksize, min_count, batch=3, out_shift=1)
            for i in range(3):
                single = raw_call(vs[i], ms[i], valids[i] if use else None, onlys[i] if use else None, shape, ksize, min_count)
                assert got[0][i].tobytes() == single[0].tobytes() and got[1][i].tobytes() == single[1].tobytes(), (i, ksize, use)
                same(single, M.median(vs[i], ms[i], ksize, valids[i] if use else None, onlys[i] if use else None, min_count), "field {}".format(i))
        # a neighbour in memory that is all NaN and all valid leaves no trace
        nan = np.full(shape + (2,), np.float32(np.nan))
        got = raw_call(np.stack([vs[0], nan, vs[2]]), np.stack([ms[0], np.ones(shape, np.uint8), ms[2]]), None, None, shape, ksize, batch=3)
        for i in (0, 2):
            same((got[0][i], got[1][i]), M.median(vs[i], ms[i], ksize), "beside NaNs, field {}".format(i))
        assert got[0][1].tobytes() == nan.tobytes() and got[1][1].all()


def test_raw_entry_refuses_bad_arguments_without_launching(gpu):
    lib = nat.load()
    h, w = 6, 9
    n = h * w
    vec, msk, aux = dev.DeviceBuffer.zeros(n * 8 + 64), dev.DeviceBuffer.zeros(n + 8), dev.DeviceBuffer.zeros(n + 8)
    outs = [guarded(n * 8, GUARD), guarded(n, GUARD)]
    o_v, o_m = [b.ptr for b in outs]

    def call(vecs=vec.ptr, mask=msk.ptr, valid=None, only=None, h=h, w=w, batch=1, ksize=3, min_count=1, out_vecs=o_v, out_mask=o_m):
        return lib.ofl_median_dev(vecs, mask, valid, only, h, w, batch, ksize, min_count, out_vecs, out_mask, None)

    for kw in (dict(vecs=None), dict(mask=None), dict(out_vecs=None), dict(h=0), dict(w=0), dict(h=-1), dict(batch=0), dict(batch=65536),
               dict(ksize=1), dict(ksize=4), dict(ksize=9), dict(ksize=0), dict(ksize=-3),
               dict(min_count=0), dict(min_count=10), dict(ksize=5, min_count=26), dict(ksize=7, min_count=50), dict(min_count=-1),
               dict(vecs=vec.ptr + 4), dict(out_vecs=o_v + 4), dict(vecs=vec.ptr + 1),
               dict(out_vecs=vec.ptr), dict(out_vecs=vec.ptr + 8), dict(out_vecs=vec.ptr + n * 8 - 8), dict(vecs=vec.ptr + 8, out_vecs=vec.ptr),
               dict(out_mask=msk.ptr), dict(out_mask=msk.ptr + n - 1), dict(valid=aux.ptr + 1, out_mask=aux.ptr + 3),
               dict(only=aux.ptr, out_mask=aux.ptr + 1), dict(out_mask=vec.ptr + 16), dict(out_mask=o_v + 8)):
        assert call(**kw) == nat.E_INVALID, kw
        assert "ofl_median" in nat.last_error(), kw
    assert lib.ofl_median(None, None, None, None, h, w, 1, 3, 1, None, None) == nat.E_INVALID and "ofl_median" in nat.last_error()
    dev.sync()
    for b in outs:
        assert (b.to_host((b.nbytes,), np.uint8) == 0xA5).all()             # nothing was launched
    # ranges that only touch are fine
    assert call(out_vecs=vec.ptr + 8, h=1, w=1) == nat.OK
    assert call() == nat.OK
    dev.sync()
    assert not outs[1].to_host((n,), np.uint8).any()                        # an empty mask: no member anywhere


# ---------------------------------------------------------------------------------------------- 3: the methods
def test_all_layers_agree(gpu):
    shape = (33, 65)
    h, w = shape
    v, m = M.vectors(shape, specials=False), M.mask("random50", shape)
    valid, only = extras(shape)
    for ksize, use_valid, use_only, min_count in ((5, False, False, None), (3, True, False, 2), (7, True, True, None), (5, False, True, 4)):
        va, on = valid if use_valid else None, only if use_only else None
        w_v, w_m, _ = M.median(v, m, ksize, va, on, 1 if min_count is None else min_count)
        d_valid = dev.DeviceBuffer.from_host(valid) if use_valid else None
        d_only = dev.DeviceBuffer.from_host(only) if use_only else None
        flow = dev.DeviceFlow.from_host(v, 's', m)
        # DeviceFlow.median
        res = flow.median(ksize, valid=d_valid, only=d_only, min_count=min_count)
        assert isinstance(res, dev.DeviceFlow) and res.shape == shape and res.ref == 's'
        g_v, g_m = res.to_host()
        assert g_v.tobytes() == w_v.tobytes() and np.array_equal(g_m.view(np.uint8), w_m)
        i_v, i_m = flow.to_host()
        assert i_v.tobytes() == v.tobytes() and np.array_equal(i_m.view(np.uint8), m)         # the inputs are unchanged
        # DeviceFlowBatch.median: this field and its mirror image in one launch
        v2, m2, valid2, only2 = (a[::-1, ::-1].copy() for a in (v, m, valid, only))
        batch = DeviceFlowBatch.from_flows([of.Flow(v, 's', m.astype(bool)), of.Flow(v2, 's', m2.astype(bool))])
        b_valid = dev.DeviceBuffer.from_host(np.stack([valid, valid2])) if use_valid else None
        b_only = dev.DeviceBuffer.from_host(np.stack([only, only2])) if use_only else None
        b_res = batch.median(ksize, valid=b_valid, only=b_only, min_count=min_count)
        assert isinstance(b_res, DeviceFlowBatch) and (b_res.n, b_res.shape, b_res.ref) == (2, shape, 's')
        x_v, x_m, _ = M.median(v2, m2, ksize, valid2 if use_valid else None, only2 if use_only else None, 1 if min_count is None else min_count)
        b_v, b_m = b_res.vecs.to_host((2, h, w, 2), np.float32), b_res.mask.to_host((2, h, w), np.uint8)
        assert b_v[0].tobytes() == w_v.tobytes() and b_v[1].tobytes() == x_v.tobytes()
        assert np.array_equal(b_m[0], w_m) and np.array_equal(b_m[1], x_m)
        flows = b_res.to_flows()
        assert flows[1].vecs.tobytes() == x_v.tobytes() and np.array_equal(flows[1].mask, x_m.astype(bool))
        # Flow.median and median_flow
        host = of.Flow(v, 't', m.astype(bool))
        for h_valid, h_only in (((valid, only), (valid.astype(bool), only.astype(bool))) if use_valid and use_only else ((va, on),)):
            f = host.median(ksize, valid=h_valid if use_valid else None, only=h_only if use_only else None, min_count=min_count)
            assert isinstance(f, of.Flow) and f.ref == 't' and f.shape == shape and f.vecs.tobytes() == w_v.tobytes()
            assert f.mask.dtype == np.bool_ and np.array_equal(f.mask, w_m.astype(bool))
        a_v, a_m = of.median_flow(v, m.astype(bool), ksize, valid=va, only=on, min_count=min_count)
        assert a_v.tobytes() == w_v.tobytes() and a_m.dtype == np.bool_ and np.array_equal(a_m, w_m.astype(bool))
        # the host entry
        o_v, o_m = np.full((h, w, 2), 7, np.float32), np.full((h, w), 7, np.uint8)
        nat.check(nat.load().ofl_median(v.ctypes.data, m.ctypes.data, None if va is None else va.ctypes.data, None if on is None else on.ctypes.data,
                                        h, w, 1, ksize, 1 if min_count is None else min_count, o_v.ctypes.data, o_m.ctypes.data))
        assert o_v.tobytes() == w_v.tobytes() and np.array_equal(o_m, w_m)
    assert flow.median().to_host()[0].tobytes() == M.median(v, m, 5)[0].tobytes()              # the default window is 5


def test_method_errors(gpu):
    f = dev.DeviceFlow.zero((6, 9), 't')
    with pytest.raises(TypeError, match="valid"):
        f.median(valid=np.ones((6, 9), np.uint8))
    with pytest.raises(TypeError, match="only"):
        f.median(only=np.ones((6, 9), np.uint8))
    with pytest.raises(ValueError, match="only"):
        f.median(only=dev.DeviceBuffer(6 * 9).view(0, 6 * 9 - 1))
    with pytest.raises(ValueError):
        f.median(4)
    with pytest.raises(TypeError):
        f.median(True)
    with pytest.raises(ValueError):
        f.median(3, min_count=10)
    b = DeviceFlowBatch.from_flows([of.Flow.zero((6, 9), 't')] * 2)
    with pytest.raises(ValueError, match="valid"):
        b.median(valid=dev.DeviceBuffer(6 * 9).view(0, 6 * 9))
    with pytest.raises(TypeError):
        b.median(only=f)
    with pytest.raises(ValueError):
        b.median(6)
    res = f.median()
    assert res.to_host()[1].all() and not res.to_host()[0].any()


@pytest.mark.parametrize("ref", ['s', 't'])
def test_fill_then_median_of_the_holes(gpu, ref):
    """the chain this kernel exists for, without leaving the device: f.fill(valid=consistent).median(5, only=holes), against
    the two restatements chained (the approximate-inverse pair of consistency_ref)"""
    shape, sign = (37, 131), (1 if ref == 's' else -1)
    (f, fm, b, bm), (consistent, covered, residual, counts) = C.case(2, shape, sign, nat.QUANT_OPENCV)
    holes = ((np.asarray(fm).astype(np.uint8) & np.asarray(consistent).astype(np.uint8)) == 0).astype(np.uint8)
    assert 100 < holes.sum() < holes.size
    fwd, bwd = dev.DeviceFlow.from_host(f, ref, fm), dev.DeviceFlow.from_host(b, ref, bm)
    d_con, _ = fwd.consistency(bwd)
    d_holes = dev.DeviceBuffer.from_host(holes)
    res = fwd.fill(valid=d_con).median(5, only=d_holes)
    assert isinstance(res, dev.DeviceFlow) and res.ref == ref and res.shape == shape
    w_v, w_m, _, _ = F.fill(f, fm, consistent)
    x_v, x_m, _ = M.median(w_v, w_m, 5, None, holes)
    g_v, g_m = res.to_host()
    assert g_v.tobytes() == x_v.tobytes() and np.array_equal(g_m.view(np.uint8), x_m)
    keep = holes == 0
    assert g_v[keep].tobytes() == np.ascontiguousarray(f)[keep].tobytes() and (g_v.view(np.uint32) != w_v.view(np.uint32)).sum() > 20
