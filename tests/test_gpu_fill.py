"""K15 (ofl_fill.hip): masked-out vectors from the nearest valid pixel on the device, against tests/fill_ref.py (the definition
by brute force) and through every layer: the raw ABI, DeviceFlow.fill, DeviceFlowBatch.fill, mask_distance, Flow.fill and
fill_flow.  Everything is an exact integer or a moved byte: every comparison is array_equal or byte equality.  Outputs are
written into 0xA5-filled buffers whose bytes around the output must survive; masks also sit at odd addresses."""
import itertools

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
import consistency_ref as C
from devmem import guarded, place, read_guarded
import fill_ref as F

pytestmark = pytest.mark.gpu
nat = of.native
GUARD = 64
ALL_OUTPUTS = (True, True, True, True)                     # out_vecs, out_mask, index, d2


def workspace(shape, batch):
    n = dev._size_query(nat.load().ofl_fill_workspace_bytes, shape[0], shape[1], batch)
    assert n == batch * shape[0] * shape[1] * 2                      # the header's formula
    return dev.DeviceBuffer(n), n


def raw_call(vecs, mask, valid, shape, batch=1, max_d2=-1, outputs=ALL_OUTPUTS, mask_shift=0, out_shift=0):
    """ofl_fill_dev on host arrays -> (out_vecs | None, out_mask | None, index | None, d2 | None) on the host.  The inputs
    masks sit mask_shift bytes (and valid mask_shift + 2 bytes) into their buffers, out_mask out_shift bytes into its own."""
    h, w = shape
    n = batch * h * w
    want_v, want_m, want_i, want_d = outputs
    keep = [place(vecs) if want_v else None, place(mask, mask_shift), place(valid, mask_shift + 2) if valid is not None else None]
    if mask_shift:
        assert keep[1][1] % 2 == 1
    work, nbytes = workspace(shape, batch)
    d_v = guarded(n * 8, GUARD) if want_v else None
    d_m = guarded(n, GUARD, out_shift) if want_m else None
    d_i = guarded(n * 4, GUARD) if want_i else None
    d_d = guarded(n * 4, GUARD) if want_d else None
    ptr = lambda b, s=0: None if b is None else b.ptr + s
    nat.check(nat.load().ofl_fill_dev(keep[0][1] if want_v else None, keep[1][1], keep[2][1] if valid is not None else None, h, w, batch,
                                      max_d2, work.ptr, nbytes, ptr(d_v), ptr(d_m, out_shift), ptr(d_i), ptr(d_d), None))
    full = (batch, h, w) if batch > 1 else (h, w)
    res = (read_guarded(d_v, 0, n * 8, GUARD, np.float32, full + (2,)) if want_v else None,
           read_guarded(d_m, out_shift, n, GUARD, np.uint8, full) if want_m else None,
           read_guarded(d_i, 0, n * 4, GUARD, np.int32, full) if want_i else None,
           read_guarded(d_d, 0, n * 4, GUARD, np.uint32, full) if want_d else None)
    # the inputs are unchanged
    for kept, a in zip(keep, (vecs, mask, valid)):
        if kept is not None:
            a = np.ascontiguousarray(a)
            got = kept[0].to_host((kept[0].nbytes,), np.uint8)[kept[1] - kept[0].ptr:][:a.nbytes]
            assert got.tobytes() == a.tobytes(), "an input was written"
    return res


def same(got, want, what):
    """the outputs present equal the restatement's: vectors byte for byte, the rest as integers"""
    g_v, g_m, g_i, g_d = got
    w_v, w_m, w_i, w_d = want
    if g_v is not None:
        assert g_v.tobytes() == np.ascontiguousarray(w_v).tobytes(), what
    for g, w in ((g_m, w_m), (g_i, w_i), (g_d, w_d)):
        if g is not None:
            assert g.dtype == w.dtype
            np.testing.assert_array_equal(g, w, err_msg=what)


# ---------------------------------------------------------------------------------------------- 1: the raw ABI against the restatement
@pytest.mark.parametrize("shape", F.SHAPES)
def test_raw_entry_against_the_reference(gpu, shape):
    h, w = shape
    v = F.vectors(shape)
    for k, name in enumerate(F.mask_names()):
        m = F.mask(name, shape)
        want = F.expected(name, shape)
        what = "{} {}".format(shape, name)
        got = raw_call(v, m, None, shape, mask_shift=k % 2, out_shift=(3, 0, 1)[k % 3])
        same(got, want, what)
        if name == "all":
            assert got[0].tobytes() == v.tobytes() and got[1].all() and not got[3].any()           # NaN, Inf and -0.0 included
            assert np.array_equal(got[2].ravel(), np.arange(h * w))
        if name == "none":
            assert (got[2] == -1).all() and (got[3] == 0xFFFFFFFF).all() and not got[1].any() and got[0].tobytes() == v.tobytes()
        if name.startswith("corner"):
            assert int(got[3].max()) == (h - 1) ** 2 + (w - 1) ** 2, what
            assert got[0].tobytes() == np.broadcast_to(v.reshape(-1, 2)[np.flatnonzero(m)[0]], (h, w, 2)).tobytes()
    # 1 x 1 without a source is the "none" case above, with one the "all" case


@pytest.mark.parametrize("shape", [(48, 80), (31, 97)])
def test_max_d2(gpu, shape):
    v = F.vectors(shape)
    for name in ("random50", "random5", "random05", "lattice2", "lattice3", "lattice4"):
        m = F.mask(name, shape)
        for max_d2 in F.MAX_D2:
            same(raw_call(v, m, None, shape, max_d2=max_d2, mask_shift=1), F.expected(name, shape, max_d2), "{} {} {}".format(shape, name, max_d2))
    # one source: 25 takes the pixels (3, 4) and (4, 3) away, 24 does not
    m = F.mask("corner0", shape)
    for max_d2, reach in ((24, False), (25, True)):
        got = raw_call(v, m, None, shape, max_d2=max_d2)
        same(got, F.expected("corner0", shape, max_d2), "corner0 {}".format(max_d2))
        for y, x in ((3, 4), (4, 3), (5, 0), (0, 5)):
            assert bool(got[1][y, x]) is reach and int(got[2][y, x]) == (0 if reach else -1) and int(got[3][y, x]) == (25 if reach else 0xFFFFFFFF)
            assert got[0][y, x].tobytes() == (v[0, 0] if reach else v[y, x]).tobytes()
        assert got[1][4, 2] and got[3][4, 2] == 20 and not got[1][4, 4]


def test_valid_takes_sources_away(gpu):
    """a pixel whose own mask is 1 but whose valid is 0 is no source: it is overwritten from its nearest source"""
    shape = (31, 97)
    v = F.vectors(shape)
    rng = np.random.default_rng(23)
    valid = (rng.random(shape) < 0.4).astype(np.uint8)
    for name, max_d2 in (("all", -1), ("random50", -1), ("random50", 2), ("lattice2", 1), ("none", -1)):
        m = F.mask(name, shape)
        want = F.fill(v, m, valid, max_d2)
        got = raw_call(v, m, valid, shape, max_d2=max_d2, mask_shift=1)
        same(got, want, "{} {}".format(name, max_d2))
        same(raw_call(v, m, valid, shape, max_d2=max_d2), want, "{} {} aligned".format(name, max_d2))
        if name == "all":
            taken = (m == 1) & (valid == 0)
            assert taken.sum() > 1000 and got[1].all() and (got[3][taken] > 0).all() and not got[3][valid == 1].any()
            assert np.array_equal(got[0].reshape(-1, 2).view(np.uint64).ravel(), v.reshape(-1, 2).view(np.uint64).ravel()[got[2].ravel()])
    # valid bytes other than 0 / 1 are ANDed bit by bit with the mask byte
    m, odd = np.full(shape, 1, np.uint8), np.where(valid == 1, 3, 2).astype(np.uint8)
    same(raw_call(v, m, odd, shape), F.fill(v, m, valid), "bitwise")


@pytest.mark.parametrize("max_d2", [-1, 25])
def test_every_combination_of_outputs(gpu, max_d2):
    shape = (31, 97)
    v, m = F.vectors(shape), F.mask("random5", shape)
    want = F.expected("random5", shape, max_d2)
    n = 0
    for outputs in itertools.product((True, False), repeat=4):
        if not outputs[0] and not outputs[2] and not outputs[3]:
            continue                                                   # refused: test_raw_entry_refuses_bad_arguments
        got = raw_call(v, m, None, shape, max_d2=max_d2, outputs=outputs, out_shift=1)
        assert [g is not None for g in got] == list(outputs)
        same(got, want, str(outputs))
        n += 1
    assert n == 14


@pytest.mark.parametrize("shape", [(1, 32766), (32766, 1)])
def test_strips(gpu, shape):
    """one source at one end, then at the other: offsets up to 32765 beside the -32768 sentinel in a 1 x 32766 row, a scan of
    32765 rows in a 32766 x 1 column.  The expectation is a closed form: every pixel takes the source, d2 = distance^2."""
    n = 32766
    v = F.vectors(shape)
    for at in (0, n - 1):
        m = np.zeros(n, np.uint8)
        m[at] = 1
        d2 = ((np.arange(n, dtype=np.int64) - at) ** 2).astype(np.uint32).reshape(shape)
        want = (np.broadcast_to(v.reshape(n, 2)[at], (n, 2)).reshape(shape + (2,)), np.ones(shape, np.uint8),
                np.full(shape, at, np.int32), d2)
        same(raw_call(v, m.reshape(shape), None, shape, mask_shift=1), want, "{} source at {}".format(shape, at))
        # a limit cuts the strip: 100 px
        cut = d2 <= 10000
        got = raw_call(v, m.reshape(shape), None, shape, max_d2=10000)
        want = (np.where(cut[..., None], want[0], v), cut.astype(np.uint8), np.where(cut, at, -1).astype(np.int32),
                np.where(cut, d2, 0xFFFFFFFF).astype(np.uint32))
        same(got, want, "{} source at {}, cut".format(shape, at))
        assert cut.sum() == 101
    # no source at all: the sentinel alone
    got = raw_call(v, np.zeros(shape, np.uint8), None, shape)
    assert not got[1].any() and (got[2] == -1).all() and (got[3] == 0xFFFFFFFF).all() and got[0].tobytes() == v.tobytes()


# ---------------------------------------------------------------------------------------------- 2: batches
def test_three_fields_in_one_launch_equal_three_launches(gpu):
    shape = (31, 97)
    assert shape[0] * shape[1] % 2 == 1                                # every second field sits at an odd address
    names = ("random5", "lattice3", "pair")
    rng = np.random.default_rng(29)
    vs = [F.vectors(shape, seed) for seed in (1, 2, 3)]
    ms = [F.mask(name, shape) for name in names]
    valids = [(rng.random(shape) < 0.7).astype(np.uint8) for _ in names]
    for valid, max_d2 in ((None, -1), (valids, -1), (valids, 24)):
        got = raw_call(np.stack(vs), np.stack(ms), None if valid is None else np.stack(valid), shape, batch=3, max_d2=max_d2, out_shift=1)
        for i in range(3):
            single = raw_call(vs[i], ms[i], None if valid is None else valid[i], shape, max_d2=max_d2)
            for g, s in zip(got, single):
                assert g[i].tobytes() == s.tobytes(), (i, max_d2)
            same(single, F.fill(vs[i], ms[i], None if valid is None else valid[i], max_d2), "field {}".format(i))


def test_raw_entry_refuses_bad_arguments_without_launching(gpu):
    lib = nat.load()
    h, w = 6, 9
    n = h * w
    vec, msk = dev.DeviceBuffer.zeros(n * 8), dev.DeviceBuffer.zeros(n)
    work, nbytes = workspace((h, w), 1)
    outs = [guarded(n * 8, GUARD), guarded(n, GUARD), guarded(n * 4, GUARD), guarded(n * 4, GUARD)]
    o_v, o_m, o_i, o_d = [b.ptr for b in outs]

    def call(vecs=vec.ptr, mask=msk.ptr, valid=None, h=h, w=w, batch=1, max_d2=-1, ws=work.ptr, ws_bytes=nbytes, out_vecs=o_v, out_mask=o_m,
             index=o_i, d2=o_d):
        return lib.ofl_fill_dev(vecs, mask, valid, h, w, batch, max_d2, ws, ws_bytes, out_vecs, out_mask, index, d2, None)

    for kw in (dict(mask=None), dict(vecs=None), dict(out_vecs=None), dict(vecs=None, out_vecs=None, index=None, d2=None),
               dict(vecs=None, out_vecs=None, out_mask=None, index=None, d2=None), dict(h=0), dict(w=0), dict(h=-1), dict(h=32767), dict(w=32767),
               dict(batch=0), dict(batch=65536), dict(max_d2=-2), dict(max_d2=-2 ** 31), dict(ws=None), dict(ws_bytes=nbytes - 1), dict(ws_bytes=0),
               dict(ws=work.ptr + 1), dict(vecs=vec.ptr + 4), dict(out_vecs=o_v + 4), dict(index=o_i + 2), dict(d2=o_d + 1),
               dict(out_vecs=vec.ptr), dict(out_mask=msk.ptr), dict(valid=msk.ptr + 1, out_mask=msk.ptr + 1)):
        assert call(**kw) == nat.E_INVALID, kw
        assert "ofl_fill" in nat.last_error(), kw
    size = dev.ctypes.c_size_t(0)
    assert lib.ofl_fill_workspace_bytes(0, 9, 1, dev.ctypes.byref(size)) == nat.E_INVALID
    assert lib.ofl_fill_workspace_bytes(6, 32767, 1, dev.ctypes.byref(size)) == nat.E_INVALID
    assert lib.ofl_fill_workspace_bytes(6, 9, 65536, dev.ctypes.byref(size)) == nat.E_INVALID
    assert lib.ofl_fill_workspace_bytes(6, 9, 1, None) == nat.E_INVALID
    assert lib.ofl_fill_workspace_bytes(32766, 32766, 2, dev.ctypes.byref(size)) == nat.OK and size.value == 2 * 32766 * 32766 * 2
    dev.sync()
    for b in outs:
        assert (b.to_host((b.nbytes,), np.uint8) == 0xA5).all()             # nothing was launched
    assert call() == nat.OK
    assert (outs[2].to_host((n,), np.int32) == -1).all()                    # an empty mask: no source


# ---------------------------------------------------------------------------------------------- 3: the methods
def finite(v):
    return np.where(np.isfinite(v), v, np.float32(2)).astype(np.float32)     # a Flow refuses NaN / Inf


def test_all_layers_agree(gpu):
    shape = (31, 97)
    h, w = shape
    rng = np.random.default_rng(31)
    v, m = finite(F.vectors(shape)), F.mask("random5", shape)
    valid = (rng.random(shape) < 0.6).astype(np.uint8)
    for use_valid, max_dist in ((False, None), (True, None), (True, 5), (False, 1.5)):
        max_d2 = dev.fill_args(max_dist)
        assert max_d2 == {None: -1, 5: 25, 1.5: 2}[max_dist]
        va = valid if use_valid else None
        w_v, w_m, w_i, w_d = F.fill(v, m, va, max_d2)
        d_valid = dev.DeviceBuffer.from_host(valid) if use_valid else None
        flow = dev.DeviceFlow.from_host(v, 's', m)
        # DeviceFlow.fill
        res, index, d2 = flow.fill(valid=d_valid, max_dist=max_dist, return_index=True, return_d2=True)
        assert isinstance(res, dev.DeviceFlow) and res.shape == shape and res.ref == 's'
        g_v, g_m = res.to_host()
        assert g_v.tobytes() == w_v.tobytes() and np.array_equal(g_m.view(np.uint8), w_m)
        assert np.array_equal(index.to_host(shape, np.int32), w_i) and np.array_equal(d2.to_host(shape, np.uint32), w_d)
        plain = flow.fill(valid=d_valid, max_dist=max_dist)
        assert isinstance(plain, dev.DeviceFlow) and plain.to_host()[0].tobytes() == w_v.tobytes()
        only_d2 = flow.fill(valid=d_valid, max_dist=max_dist, return_d2=True)
        assert len(only_d2) == 2 and np.array_equal(only_d2[1].to_host(shape, np.uint32), w_d)
        # the inputs are unchanged
        i_v, i_m = flow.to_host()
        assert i_v.tobytes() == v.tobytes() and np.array_equal(i_m.view(np.uint8), m)
        # DeviceFlowBatch.fill: this field and its mirror image in one launch
        v2, m2, valid2 = v[::-1, ::-1].copy(), m[::-1, ::-1].copy(), valid[::-1, ::-1].copy()
        batch = DeviceFlowBatch.from_flows([of.Flow(v, 's', m.astype(bool)), of.Flow(v2, 's', m2.astype(bool))])
        b_valid = dev.DeviceBuffer.from_host(np.stack([valid, valid2])) if use_valid else None
        b_res, b_index = batch.fill(valid=b_valid, max_dist=max_dist, return_index=True)
        assert isinstance(b_res, DeviceFlowBatch) and (b_res.n, b_res.shape, b_res.ref) == (2, shape, 's')
        x_v, x_m, x_i, _ = F.fill(v2, m2, valid2 if use_valid else None, max_d2)
        b_v, b_m = b_res.vecs.to_host((2, h, w, 2), np.float32), b_res.mask.to_host((2, h, w), np.uint8)
        assert b_v[0].tobytes() == w_v.tobytes() and b_v[1].tobytes() == x_v.tobytes()
        assert np.array_equal(b_m[0], w_m) and np.array_equal(b_m[1], x_m)
        assert np.array_equal(b_index.to_host((2, h, w), np.int32), np.stack([w_i, x_i]))
        flows = batch.fill(valid=b_valid, max_dist=max_dist).to_flows()
        assert flows[1].vecs.tobytes() == x_v.tobytes() and np.array_equal(flows[1].mask, x_m.astype(bool))
        # mask_distance: the sources as one mask
        src = F.sources(m, va).astype(np.uint8)
        index, d2 = dev.mask_distance(dev.DeviceBuffer.from_host(np.stack([src, src[::-1, ::-1]])), shape, batch=2, max_dist=max_dist)
        assert np.array_equal(index.to_host((2, h, w), np.int32), np.stack([w_i, x_i]))
        assert np.array_equal(d2.to_host((2, h, w), np.uint32)[0], w_d)
        index, d2 = dev.mask_distance(dev.DeviceBuffer.from_host(src), shape, max_dist=max_dist)
        assert np.array_equal(index.to_host(shape, np.int32), w_i) and np.array_equal(d2.to_host(shape, np.uint32), w_d)
        # Flow.fill and fill_flow
        host = of.Flow(v, 't', m.astype(bool))
        for h_valid in ((valid, valid.astype(bool)) if use_valid else (None,)):
            f, h_i, h_d = host.fill(valid=h_valid, max_dist=max_dist, return_index=True, return_d2=True)
            assert isinstance(f, of.Flow) and f.ref == 't' and f.vecs.tobytes() == w_v.tobytes() and np.array_equal(f.mask, w_m.astype(bool))
            assert h_i.dtype == np.int32 and h_d.dtype == np.uint32 and np.array_equal(h_i, w_i) and np.array_equal(h_d, w_d)
            assert f.mask.dtype == np.bool_
        f = host.fill(valid=va, max_dist=max_dist)
        assert isinstance(f, of.Flow) and f.vecs.tobytes() == w_v.tobytes()
        a_v, a_m = of.fill_flow(v, m.astype(bool), valid=va, max_dist=max_dist)
        assert a_v.tobytes() == w_v.tobytes() and a_m.dtype == np.bool_ and np.array_equal(a_m, w_m.astype(bool))


def test_method_errors(gpu):
    f = dev.DeviceFlow.zero((6, 9), 't')
    with pytest.raises(TypeError):
        f.fill(valid=np.ones((6, 9), np.uint8))
    with pytest.raises(ValueError):
        f.fill(valid=dev.DeviceBuffer(6 * 9).view(0, 6 * 9 - 1))
    with pytest.raises(ValueError):
        f.fill(max_dist=-1)
    with pytest.raises(TypeError):
        f.fill(max_dist=True)
    b = DeviceFlowBatch.from_flows([of.Flow.zero((6, 9), 't')] * 2)
    with pytest.raises(ValueError):
        b.fill(valid=dev.DeviceBuffer(6 * 9).view(0, 6 * 9))
    with pytest.raises(TypeError):
        b.fill(valid=f)
    with pytest.raises(ValueError):
        dev.mask_distance(dev.DeviceBuffer(64).view(0, 53), (6, 9))
    with pytest.raises(ValueError):
        dev.mask_distance(dev.DeviceBuffer(64), (6, 9), batch=0)
    with pytest.raises(TypeError):
        dev.mask_distance(np.ones((6, 9), np.uint8), (6, 9))
    res = f.fill()
    assert res.to_host()[1].all() and not res.to_host()[0].any()


@pytest.mark.parametrize("ref", ['s', 't'])
def test_consistency_then_fill(gpu, ref):
    """the chain this kernel exists for, without leaving the device: f.consistency(b) -> f.fill(valid=consistent), against the
    same chain of the two restatements (the approximate-inverse pair of consistency_ref)"""
    shape, sign = (37, 131), (1 if ref == 's' else -1)
    (f, fm, b, bm), (consistent, covered, residual, counts) = C.case(2, shape, sign, nat.QUANT_OPENCV)
    assert 0 < counts[1] < shape[0] * shape[1]
    fwd, bwd = dev.DeviceFlow.from_host(f, ref, fm), dev.DeviceFlow.from_host(b, ref, bm)
    d_con, d_cov = fwd.consistency(bwd)
    for max_dist, max_d2 in ((None, -1), (3, 9)):
        filled, index = fwd.fill(valid=d_con, max_dist=max_dist, return_index=True)
        w_v, w_m, w_i, _ = F.fill(f, fm, consistent, max_d2)
        g_v, g_m = filled.to_host()
        assert g_v.tobytes() == w_v.tobytes() and np.array_equal(g_m.view(np.uint8), w_m)
        assert np.array_equal(index.to_host(shape, np.int32), w_i)
        assert filled.ref == ref and (max_d2 >= 0 or w_m.all()) and (w_i != np.arange(w_i.size).reshape(shape)).sum() > 100
