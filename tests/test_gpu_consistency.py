"""K13 (ofl_consistency.hip): the forward-backward check on the device, bit for bit against tests/consistency_ref.py (the
oracle restated), against the fused compose kernel on the device itself, and through every layer: the raw ABI,
DeviceFlow.consistency, DeviceFlowBatch.consistency, Flow.consistency and flow_consistency.  Nothing here has a tolerance:
masks, residual bits and counts are compared with array_equal."""
import itertools

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
import consistency_ref as C

pytestmark = pytest.mark.gpu
nat = of.native


def up(a):
    a = np.ascontiguousarray(a)
    return dev.DeviceBuffer.from_host(a.view(np.uint8) if a.dtype == np.bool_ else a)


def raw_call(bufs, sign, shape, batch=1, alpha=C.ALPHA, beta=C.BETA, quant=nat.QUANT_OPENCV, covered=True, residual=True, counts=True):
    """ofl_consistency_dev on uploaded (f, fm, b, bm) -> (consistent, covered | None, residual | None, counts | None) on the host"""
    h, w = shape
    n = batch * h * w
    f, fm, b, bm = bufs
    d_con = dev.DeviceBuffer(n)
    d_cov = dev.DeviceBuffer(n) if covered else None
    d_res = dev.DeviceBuffer(n * 4) if residual else None
    d_cnt = dev.DeviceBuffer.zeros(batch * 8) if counts else None
    ptr = lambda x: None if x is None else x.ptr
    nat.check(nat.load().ofl_consistency_dev(f.ptr, fm.ptr, b.ptr, bm.ptr, sign, h, w, batch, np.float32(alpha), np.float32(beta),
                                             d_con.ptr, ptr(d_cov), ptr(d_res), ptr(d_cnt), quant, None))
    full = (batch, h, w) if batch > 1 else (h, w)
    return (d_con.to_host(full, np.uint8),
            d_cov.to_host(full, np.uint8) if covered else None,
            d_res.to_host(full, np.float32) if residual else None,
            d_cnt.to_host((batch, 2), np.uint32) if counts else None)


def same_bits(got, want, what):
    np.testing.assert_array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32), err_msg=what)


# ---------------------------------------------------------------------------------------------- 1: the raw ABI against the restatement
@pytest.mark.parametrize("shape", C.SHAPES)
def test_raw_entry_against_the_reference(gpu, shape):
    for sign, quant in itertools.product(C.SIGNS, C.QUANTS):
        inputs, (consistent, covered, residual, counts) = C.case(1, shape, sign, quant)
        bufs = [up(a) for a in inputs]
        # every output present, every optional output absent, and each absent alone
        for k, (cv, rs, cn) in enumerate([(True, True, True), (False, False, False), (False, True, True), (True, False, True), (True, True, False)]):
            what = "{} sign {} quant {} outputs {}".format(shape, sign, quant, (cv, rs, cn))
            g_con, g_cov, g_res, g_cnt = raw_call(bufs, sign, shape, quant=quant, covered=cv, residual=rs, counts=cn)
            np.testing.assert_array_equal(g_con, consistent.astype(np.uint8), err_msg=what)
            if cv:
                np.testing.assert_array_equal(g_cov, covered.astype(np.uint8), err_msg=what)
            if rs:
                same_bits(g_res, residual, what)
            if cn:
                assert tuple(int(v) for v in g_cnt[0]) == counts, what
                assert int(g_cnt[0][1]) == int(g_con.sum()) and (not cv or int(g_cnt[0][0]) == int(g_cov.sum())), what
        # the inputs are unchanged
        for buf, a in zip(bufs, inputs):
            np.testing.assert_array_equal(buf.to_host(a.shape, np.uint8 if a.dtype == np.bool_ else a.dtype),
                                          a.view(np.uint8) if a.dtype == np.bool_ else a)


def test_unaligned_even_width_takes_the_generic_path(gpu):
    """an even width whose buffers sit at odd addresses cannot use the two-pixel path: same result"""
    shape, sign, quant = (19, 70), -1, nat.QUANT_OPENCV
    inputs, (consistent, covered, residual, counts) = C.case(1, shape, sign, quant)
    f, fm, b, bm = [up(a) for a in inputs]
    n = shape[0] * shape[1]
    shifted = dev.DeviceBuffer(n + 1)
    nat.check(nat.load().ofl_copy_dev(shifted.ptr + 1, fm.ptr, n, None))
    out = dev.DeviceBuffer(2 * n + 4)
    d_con, d_cov = out.view(1, n), out.view(n + 2 + (n & 1) + 1, n)
    assert d_con.ptr % 2 == 1 and d_cov.ptr % 2 == 1
    nat.check(nat.load().ofl_consistency_dev(f.ptr, shifted.ptr + 1, b.ptr, bm.ptr, sign, shape[0], shape[1], 1, np.float32(C.ALPHA),
                                             np.float32(C.BETA), d_con.ptr, d_cov.ptr, None, None, quant, None))
    np.testing.assert_array_equal(d_con.to_host(shape, np.uint8), consistent.astype(np.uint8))
    np.testing.assert_array_equal(d_cov.to_host(shape, np.uint8), covered.astype(np.uint8))


# ---------------------------------------------------------------------------------------------- 2: against the compose kernel
@pytest.mark.parametrize("shape", C.SHAPES)
def test_covered_and_residual_equal_the_compose_kernel(gpu, shape):
    h, w = shape
    for sign, quant in itertools.product(C.SIGNS, C.QUANTS):
        inputs, _ = C.case(1, shape, sign, quant)
        f, fm, b, bm = [up(a) for a in inputs]
        out, mout = dev.DeviceBuffer(h * w * 8), dev.DeviceBuffer(h * w)
        nat.check(nat.load().ofl_compose3_dev(b.ptr, bm.ptr, f.ptr, fm.ptr, sign, h, w, 1, out.ptr, mout.ptr, None, quant, None))
        _, g_cov, g_res, _ = raw_call((f, fm, b, bm), sign, shape, quant=quant)
        o, m = out.to_host((h, w, 2), np.float32), mout.to_host((h, w), np.uint8)
        np.testing.assert_array_equal(g_cov, m)
        mag = np.sqrt(o[..., 0] * o[..., 0] + o[..., 1] * o[..., 1])
        same_bits(g_res, np.where(m != 0, mag, np.float32(0)).astype(np.float32), "{} {} {}".format(shape, sign, quant))


# ---------------------------------------------------------------------------------------------- 3: batches
@pytest.mark.parametrize("shape", [(19, 70), (5, 7)])
def test_three_pairs_in_one_launch_equal_three_launches(gpu, shape):
    sign, quant = -1, nat.QUANT_OPENCV
    cases = [C.case(seed, shape, sign, quant) for seed in (1, 2, 3)]
    stacked = [up(np.stack([c[0][k] for c in cases])) for k in range(4)]
    g_con, g_cov, g_res, g_cnt = raw_call(stacked, sign, shape, batch=3, quant=quant)
    for i, (inputs, (consistent, covered, residual, counts)) in enumerate(cases):
        s_con, s_cov, s_res, s_cnt = raw_call([up(a) for a in inputs], sign, shape, quant=quant)
        np.testing.assert_array_equal(g_con[i], s_con)
        np.testing.assert_array_equal(g_cov[i], s_cov)
        same_bits(g_res[i], s_res, "pair {}".format(i))
        np.testing.assert_array_equal(g_cnt[i], s_cnt[0])
        np.testing.assert_array_equal(g_con[i], consistent.astype(np.uint8))
        assert tuple(int(v) for v in g_cnt[i]) == counts


def make_batch(vecs, masks, ref):
    n, h, w = masks.shape
    b = DeviceFlowBatch(n, (h, w), ref)
    v, m = np.ascontiguousarray(vecs, np.float32), np.ascontiguousarray(masks).view(np.uint8)
    nat.check(nat.load().ofl_upload(b.vecs.ptr, v.ctypes.data, v.nbytes, None))
    nat.check(nat.load().ofl_upload(b.mask.ptr, m.ctypes.data, m.nbytes, None))
    dev.sync()
    return b


@pytest.mark.parametrize("ref", ['s', 't'])
def test_batch_method_packed_and_unpacked(gpu, ref):
    shape, sign = (19, 70), (1 if ref == 's' else -1)
    cases = [C.case(seed, shape, sign, nat.QUANT_OPENCV) for seed in (1, 2, 3)]
    fwd = make_batch(np.stack([c[0][0] for c in cases]), np.stack([c[0][1] for c in cases]), ref)
    bwd = make_batch(np.stack([c[0][2] for c in cases]), np.stack([c[0][3] for c in cases]), ref)
    results = []
    for fb, bb in ((fwd, bwd), (fwd.pack(), bwd.pack())):
        if fb.packed:                  # a packed batch must answer from its bit planes
            fb._mask = bb._mask = None
        con, cov, res, cnt = fb.consistency(bb, return_residual=True, return_counts=True)
        results.append((con.to_host((3,) + shape, np.uint8), cov.to_host((3,) + shape, np.uint8), res.to_host((3,) + shape, np.float32), cnt))
        assert len(fb.consistency(bb)) == 2 and len(fb.consistency(bb, return_residual=True)) == 3
    for i, (_, (consistent, covered, residual, counts)) in enumerate(cases):
        for con, cov, res, cnt in results:
            np.testing.assert_array_equal(con[i], consistent.astype(np.uint8))
            np.testing.assert_array_equal(cov[i], covered.astype(np.uint8))
            same_bits(res[i], residual, "pair {}".format(i))
            assert cnt.shape == (3, 2) and tuple(int(v) for v in cnt[i]) == counts
    other = make_batch(np.zeros((2,) + shape + (2,)), np.ones((2,) + shape, bool), ref)
    with pytest.raises(ValueError):
        fwd.consistency(other)
    with pytest.raises(ValueError):
        fwd.consistency(make_batch(np.zeros((3,) + shape + (2,)), np.ones((3,) + shape, bool), 't' if ref == 's' else 's'))
    with pytest.raises(TypeError):
        fwd.consistency(fwd.field(0))


# ---------------------------------------------------------------------------------------------- 4: the methods
@pytest.mark.parametrize("alpha_beta", [(None, None), (0, 0)])
def test_integer_translation_through_the_device_method(gpu, alpha_beta):
    f, fm, b, bm = C.translation()
    fwd, bwd = dev.DeviceFlow.from_host(f, 's', fm), dev.DeviceFlow.from_host(b, 's', bm)
    con, cov, res, (n_cov, n_con) = fwd.consistency(bwd, *alpha_beta, return_residual=True, return_counts=True)
    con, cov = con.to_host((37, 131), np.uint8), cov.to_host((37, 131), np.uint8)
    assert (n_cov, n_con) == (4480, 4480) and isinstance(n_cov, int)
    np.testing.assert_array_equal(con, cov)
    assert cov[2:, :128].all() and int(cov.sum()) == 4480
    assert not res.to_host((37, 131), np.float32).any()


@pytest.mark.parametrize("quant", C.QUANTS)
@pytest.mark.parametrize("ref", ['s', 't'])
def test_rotation_through_the_device_method(gpu, ref, quant):
    f, fm, b, bm = C.rotation(ref)
    want = C.consistency(f, fm, b, bm, 1 if ref == 's' else -1, quant=quant)
    fwd, bwd = dev.DeviceFlow.from_host(f, ref, fm), dev.DeviceFlow.from_host(b, ref, bm)
    con, cov, res = fwd.consistency(bwd, return_residual=True, quant=quant)
    con, cov, res = con.to_host((37, 131), np.uint8), cov.to_host((37, 131), np.uint8), res.to_host((37, 131), np.float32)
    np.testing.assert_array_equal(con, cov)
    assert cov.sum() > 1000 and res.max() < 0.05
    np.testing.assert_array_equal(cov, want[1].astype(np.uint8))
    same_bits(res, want[2], "rotation {} {}".format(ref, quant))


@pytest.mark.parametrize("ref", ['s', 't'])
def test_host_methods_equal_the_device_method(gpu, ref):
    shape, sign = (37, 131), (1 if ref == 's' else -1)
    (f, fm, b, bm), (consistent, covered, residual, counts) = C.case(2, shape, sign, nat.QUANT_OPENCV, 0.02, 0.25)
    fwd, bwd = dev.DeviceFlow.from_host(f, ref, fm), dev.DeviceFlow.from_host(b, ref, bm)
    d_con, d_cov, d_res = fwd.consistency(bwd, 0.02, 0.25, return_residual=True)
    d_con, d_cov, d_res = d_con.to_host(shape, np.uint8), d_cov.to_host(shape, np.uint8), d_res.to_host(shape, np.float32)
    np.testing.assert_array_equal(d_con, consistent.astype(np.uint8))
    h_con, h_cov, h_res = of.Flow(f, ref, fm).consistency(of.Flow(b, ref, bm), alpha=0.02, beta=0.25, return_residual=True)
    assert h_con.dtype == h_cov.dtype == np.bool_ and h_res.dtype == np.float32 and h_con.shape == h_res.shape == shape
    np.testing.assert_array_equal(h_con.view(np.uint8), d_con)
    np.testing.assert_array_equal(h_cov.view(np.uint8), d_cov)
    same_bits(h_res, d_res, ref)
    assert len(of.Flow(f, ref, fm).consistency(of.Flow(b, ref, bm))) == 2
    # arrays in: masks are dropped, so compare with all-valid device fields
    a_con, a_cov = of.flow_consistency(f, b, ref, alpha=0.02, beta=0.25)
    e_con, e_cov = dev.DeviceFlow.from_host(f, ref).consistency(dev.DeviceFlow.from_host(b, ref), 0.02, 0.25)
    np.testing.assert_array_equal(a_con.view(np.uint8), e_con.to_host(shape, np.uint8))
    np.testing.assert_array_equal(a_cov.view(np.uint8), e_cov.to_host(shape, np.uint8))
    # the inputs of the device call are unchanged
    v, m = fwd.to_host()
    np.testing.assert_array_equal(v, f)
    np.testing.assert_array_equal(m, fm)
    v, m = bwd.to_host()
    np.testing.assert_array_equal(v, b)
    np.testing.assert_array_equal(m, bm)


# ---------------------------------------------------------------------------------------------- 5: errors
def test_method_errors(gpu):
    f = dev.DeviceFlow.zero((6, 9), 't')
    with pytest.raises(ValueError, match="'t'.*'s'"):
        f.consistency(dev.DeviceFlow.zero((6, 9), 's'))
    with pytest.raises(ValueError, match=r"\(6, 9\).*\(6, 10\)"):
        f.consistency(dev.DeviceFlow.zero((6, 10), 't'))
    with pytest.raises(TypeError):
        f.consistency(of.Flow.zero((6, 9), 't'))
    with pytest.raises(ValueError):
        f.consistency(f, alpha=-1)
    with pytest.raises(ValueError):
        f.consistency(f, beta=float('nan'))
    with pytest.raises(TypeError):
        f.consistency(f, alpha=True)


def test_raw_entry_refuses_bad_arguments_without_launching(gpu):
    lib = nat.load()
    n = 6 * 9
    f, fm, out = dev.DeviceBuffer.zeros(n * 8), dev.DeviceBuffer.zeros(n), dev.DeviceBuffer.zeros(n)
    nat.check(lib.ofl_memset(out.ptr, 7, n, None))
    a, b = np.float32(C.ALPHA), np.float32(C.BETA)

    def call(sign=1, batch=1, h=6, w=9, alpha=a, beta=b, quant=nat.QUANT_OPENCV, f_ptr=f.ptr, out_ptr=out.ptr):
        return lib.ofl_consistency_dev(f_ptr, fm.ptr, f.ptr, fm.ptr, sign, h, w, batch, alpha, beta, out_ptr, None, None, None, quant, None)

    for kw in (dict(sign=0), dict(sign=2), dict(batch=0), dict(batch=65536), dict(h=0), dict(w=-1), dict(alpha=np.float32(-1)),
               dict(beta=np.float32('nan')), dict(alpha=np.float32('inf')), dict(quant=7), dict(f_ptr=None), dict(out_ptr=None)):
        assert call(**kw) == nat.E_INVALID, kw
        assert "ofl_consistency" in nat.last_error()
    dev.sync()
    assert (out.to_host((n,), np.uint8) == 7).all()          # nothing was launched
    assert call() == nat.OK
    assert not out.to_host((n,), np.uint8).any()             # zero fields with empty masks: nothing is covered
