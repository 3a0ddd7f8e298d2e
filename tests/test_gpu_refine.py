"""K23 (ofl_refine.hip): the variational refinement of a field on the device, bit for bit against tests/refine_ref.py (the
oracle's gather plus float32 NumPy in the stated order), against K21 on the device itself, and through every layer: the raw
ABI, DeviceFlow.refine, DeviceFlowBatch.refine, Flow.refine and refine_flow.  Nothing here has a tolerance: vectors are
compared through their bits (a NaN keeps its payload), masks and `data` with array_equal.  The setup tile is 64 x 16:
(19, 70) and (37, 131) cross its seams raggedly, (64, 256) is an exact multiple; refine_ref.holes() puts edges into
non-domain pixels on both colours and on the seams."""
import itertools

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
import interop_ref as R
import nonfinite_cases as NF
import refine_ref as Rf
import tensor_ref as T

pytestmark = pytest.mark.gpu
nat = of.native
F32, U8 = np.float32, np.uint8
EL = {'float32': nat.EL_F32, 'float16': nat.EL_F16, 'bfloat16': nat.EL_BF16}
LAYOUT = {'chw': nat.TENSOR_NCHW, 'hwc': nat.TENSOR_NHWC}
ITERATIONS = [(1, 1), (2, 3), (5, 5)]                     # (fixed_point, sor)


def up(a):
    a = np.ascontiguousarray(a)
    return dev.DeviceBuffer.from_host(a.view(U8) if a.dtype == np.bool_ else a)


def ptr(x):
    return None if x is None else x.ptr


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def raw_call(near, far, dtype, layout, f, fm, sign, near_mask=None, far_mask=None, valid=None, quant=nat.QUANT_OPENCV, data=True, **kw):
    """ofl_refine_dev on host arrays: near, far planar (n, c, h, w) as stored in `dtype`, uploaded in the memory order of
    `layout`; f (n, h, w, 2), masks (n, h, w) -> (vecs (n, h, w, 2), data (n, h, w) | None) on the host"""
    n, c, h, w = near.shape
    px = n * h * w
    prm = Rf.settings(**kw)
    d_near, d_far = up(Rf.in_layout(near, layout)), up(Rf.in_layout(far, layout))
    d_f, d_fm = up(np.ascontiguousarray(f, F32)), up(fm)
    d_nm, d_am, d_va = (None if m is None else up(m) for m in (near_mask, far_mask, valid))
    work, d_out = dev.DeviceBuffer(29 * px), dev.DeviceBuffer(px * 8)
    d_data = dev.DeviceBuffer(px) if data else None
    nat.check(nat.load().ofl_refine_dev(d_near.ptr, d_far.ptr, EL[dtype], LAYOUT[layout], n, c, h, w, d_f.ptr, d_fm.ptr, sign,
                                        ptr(d_nm), ptr(d_am), ptr(d_va), prm['alpha'], prm['delta'], prm['zeta'], prm['eps'],
                                        prm['fixed_point'], prm['sor'], prm['omega'], work.ptr, 29 * px, d_out.ptr, ptr(d_data), quant, None))
    return d_out.to_host((n, h, w, 2), F32), d_data.to_host((n, h, w), U8) if data else None


def check(got, want, what):
    vecs, data = got
    assert np.array_equal(bits(vecs), bits(want['vecs'])), "{}: vecs, {} of {} words differ".format(
        what, int((bits(vecs) != bits(want['vecs'])).sum()), vecs.size)
    if data is not None:
        np.testing.assert_array_equal(data, want['data'].astype(U8), err_msg="{}: data".format(what))


def run_case(shape, sign, quant, layout, dtype, c, n=1, seed=1, masked=False, **kw):
    k = Rf.case(seed, shape, sign, quant, c, dtype, n, masked, tuple(sorted(kw.items())))
    got = raw_call(k['near'], k['far'], dtype, layout, k['f'], k['fm'], sign, k['near_mask'], k['far_mask'], k['valid'], quant, **kw)
    check(got, k['want'], (shape, sign, quant, layout, dtype, c, n, masked, kw))
    return got, k


# ---------------------------------------------------------------------------------------------- 1: channels x layout x dtype
def rotation(c):
    """the six (dtype, layout) of channel count c with their (sign, quant, (fixed_point, sor), omega, masked): over the four
    channel counts every dtype and layout meets both signs, both quant, all three iteration pairs, both omega and both
    mask settings"""
    out = []
    for i, (dtype, layout) in enumerate(itertools.product(T.DTYPES, T.LAYOUTS)):
        k = c - 1
        out.append((Rf.SIGNS[(i + k) % 2], Rf.QUANTS[(i // 2 + k // 2) % 2], ITERATIONS[(i + k) % 3], (1.6, 1.0)[(i // 3 + k) % 2],
                    bool((i + k // 2) % 2), layout, dtype))
    return out


def test_the_rotation_reaches_every_setting():
    seen = [r for c in (1, 2, 3, 4) for r in rotation(c)]
    assert len(seen) == 24
    for dtype, layout in itertools.product(T.DTYPES, T.LAYOUTS):
        mine = [r for r in seen if r[5:] == (layout, dtype)]
        assert len(mine) == 4
        for col, values in enumerate((Rf.SIGNS, Rf.QUANTS, ITERATIONS, (1.6, 1.0), (False, True))):
            assert {r[col] for r in mine} == set(values), (dtype, layout, col)


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_every_channel_count_layout_and_dtype(gpu, c):
    for sign, quant, (fixed_point, sor), omega, masked, layout, dtype in rotation(c):
        run_case((19, 70), sign, quant, layout, dtype, c, masked=masked, fixed_point=fixed_point, sor=sor, omega=omega)


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_planar_and_channels_last_give_identical_bytes(gpu, dtype):
    for c in (1, 3, 4):
        (a, da), _ = run_case((19, 70), -1, nat.QUANT_OPENCV, 'chw', dtype, c, fixed_point=2, sor=3)
        (b, db), _ = run_case((19, 70), -1, nat.QUANT_OPENCV, 'hwc', dtype, c, fixed_point=2, sor=3)
        assert a.tobytes() == b.tobytes() and da.tobytes() == db.tobytes()


# ---------------------------------------------------------------------------------------------- 2: shapes
# at every shape each sign, quant, layout, dtype, iteration pair and mask setting occurs at least once
THIN = [(1, nat.QUANT_OPENCV, 'chw', 'float32', 3, False, dict()),
        (-1, nat.QUANT_EXACT, 'hwc', 'float16', 1, True, dict(fixed_point=2, sor=3, omega=1.0)),
        (1, nat.QUANT_EXACT, 'chw', 'bfloat16', 4, True, dict(fixed_point=1, sor=1)),
        (-1, nat.QUANT_OPENCV, 'hwc', 'float32', 2, False, dict(fixed_point=2, sor=3, alpha=5.0, delta=2.0, zeta=0.5, eps=0.01))]


@pytest.mark.parametrize("shape", Rf.TINY + Rf.SHAPES, ids=lambda s: "{}x{}".format(*s))
def test_shapes(gpu, shape):
    for sign, quant, layout, dtype, c, masked, kw in THIN:
        run_case(shape, sign, quant, layout, dtype, c, masked=masked, **kw)


# ---------------------------------------------------------------------------------------------- 3: properties on the device
def test_outside_the_domain_every_vector_keeps_its_bits(gpu):
    (vecs, data), k = run_case((37, 131), 1, nat.QUANT_OPENCV, 'chw', 'float32', 3, masked=True)
    dom = k['fm'] & k['valid'].astype(bool)
    same = (bits(vecs) == bits(k['f'])).all(axis=-1)
    assert same[~dom].all() and (~dom).sum() > 200 and (~same[dom]).mean() > 0.5
    assert not data.astype(bool)[~dom].any()


def test_alpha_zero_without_a_data_term_returns_the_input(gpu):
    k = Rf.case(2, (37, 131), 1, nat.QUANT_OPENCV, 3)
    f = k['f'].copy()
    f[0, 0, 0], f[0, 20, 64] = (-0.0, 0.0), (0.0, -0.0)
    vecs, data = raw_call(k['near'], k['far'], 'float32', 'chw', f, k['fm'], 1, far_mask=np.zeros((1, 37, 131), U8), alpha=0)
    assert not data.any() and np.array_equal(bits(vecs), bits(f))
    # valid all zero: no domain at all, non-finite vectors come back too
    f[0, 5, 5] = (np.nan, np.inf)
    vecs, data = raw_call(k['near'], k['far'], 'float32', 'hwc', f, k['fm'], 1, valid=np.zeros((1, 37, 131), U8))
    assert not data.any() and np.array_equal(bits(vecs), bits(f))


@pytest.mark.parametrize("ref", ['s', 't'])
def test_data_is_k21s_covered_eroded_by_the_4_neighbours(gpu, ref):
    """on an all-domain field; both computed on the device"""
    shape, sign, c = (37, 131), (1 if ref == 's' else -1), 3
    k = Rf.case(5, shape, sign, nat.QUANT_OPENCV, c, masked=True)
    near, far = (dev.DeviceTensor.from_host(np.ascontiguousarray(k[name][0]), 'chw') for name in ('near', 'far'))
    flow = dev.DeviceFlow.from_host(k['f'][0], ref)                              # mask None: all valid
    nm, am = up(k['near_mask'][0]), up(k['far_mask'][0])
    _, data = flow.refine(near, far, near_mask=nm, far_mask=am, return_data=True)
    _, covered = flow.photometric(near, far, near_mask=nm, far_mask=am)
    data, cov = data.to_host(shape, U8).astype(bool), covered.to_host(shape, U8).astype(bool)
    pad = np.pad(cov, 1, constant_values=True)                                   # a neighbour outside the frame does not count
    eroded = cov & pad[:-2, 1:-1] & pad[2:, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:]
    np.testing.assert_array_equal(data, eroded)
    assert 0.3 < data.mean() < cov.mean() < 1


# ---------------------------------------------------------------------------------------------- 4: non-finite values
def test_non_finite_image_values(gpu):
    shape, sign, c = (19, 70), 1, 3
    k = Rf.case(7, shape, sign, nat.QUANT_EXACT, c)
    near, far = k['near'].copy(), k['far'].copy()
    near[0, 1, 9, 30], near[0, 2, 16, 63] = np.nan, np.inf
    far[0, 2, 5, 50], far[0, 0, 12, 20] = np.nan, -np.inf
    want = Rf.restate(near, far, k['f'], k['fm'], sign, quant=nat.QUANT_EXACT)
    for layout in T.LAYOUTS:
        got = raw_call(near, far, 'float32', layout, k['f'], k['fm'], sign, quant=nat.QUANT_EXACT)
        check(got, want, layout)
        assert np.isfinite(got[0]).all() and got[1].sum() < k['want']['data'].sum()


@pytest.mark.parametrize("kind", ['random', 'shift'])
def test_non_finite_vectors(gpu, kind):
    """fields with NaN and Inf vectors (nonfinite_cases): they lie outside the domain, keep their bits and spread nowhere"""
    B, h, w = shape = (1, 19, 70)
    k = NF.case(shape, kind, 'sprinkle')
    c, sign = 2, k['sign']
    rng = np.random.default_rng(h + w)
    far = (128 + rng.standard_normal((B, c, h, w)) * 40).astype(F32)
    near = (128 + rng.standard_normal((B, c, h, w)) * 40).astype(F32)
    bad = ~np.isfinite(k['fb']).all(axis=-1)
    assert bad.any()
    for quant, layout in itertools.product(Rf.QUANTS, T.LAYOUTS):
        want = Rf.restate(near, far, k['fb'], k['mb'], sign, far_mask=k['ma'], quant=quant)
        got = raw_call(near, far, 'float32', layout, k['fb'], k['mb'], sign, far_mask=k['ma'], quant=quant)
        check(got, want, (kind, quant, layout))
        assert np.array_equal(bits(got[0])[bad], bits(k['fb'])[bad]) and np.isfinite(got[0][~bad]).all()
        assert (bits(got[0]) != bits(k['fb'])).any()


# ---------------------------------------------------------------------------------------------- 5: batches
@pytest.mark.parametrize("layout", T.LAYOUTS)
def test_a_batch_equals_its_single_calls(gpu, layout):
    shape, sign, c, n = (37, 131), -1, 3, 3
    k = Rf.case(8, shape, sign, nat.QUANT_OPENCV, c, 'float16', n, True)
    near, far = (dev.DeviceTensor.from_host(Rf.in_layout(k[name], layout), layout) for name in ('near', 'far'))
    batch = DeviceFlowBatch.from_flows([of.Flow(k['f'][i], 't', k['fm'][i]) for i in range(n)])
    masks = dict(near_mask=up(k['near_mask']), far_mask=up(k['far_mask']), valid=up(k['valid']))
    out, data = batch.refine(near, far, fixed_point=2, sor=3, return_data=True, **masks)
    assert isinstance(out, DeviceFlowBatch) and (out.n, out.shape, out.ref) == (n, shape, 't')
    vecs, data = out.vecs.to_host((n,) + shape + (2,), F32), data.to_host((n,) + shape, U8)
    np.testing.assert_array_equal(out.mask.to_host((n,) + shape, U8), k['fm'].astype(U8))
    want = Rf.restate(R.to_f32(k['near'], 'float16'), R.to_f32(k['far'], 'float16'), k['f'], k['fm'], sign, near_mask=k['near_mask'],
                      far_mask=k['far_mask'], valid=k['valid'], fixed_point=2, sor=3)
    check((vecs, data), want, "batch")
    for i in range(n):
        one_near, one_far = (dev.DeviceTensor.from_host(Rf.in_layout(k[name][i:i + 1], layout, False), layout) for name in ('near', 'far'))
        single, d1 = dev.DeviceFlow.from_host(k['f'][i], 't', k['fm'][i]).refine(
            one_near, one_far, fixed_point=2, sor=3, return_data=True, near_mask=up(k['near_mask'][i]), far_mask=up(k['far_mask'][i]),
            valid=up(k['valid'][i]))
        assert single.vecs.to_host(shape + (2,), F32).tobytes() == vecs[i].tobytes() and d1.to_host(shape, U8).tobytes() == data[i].tobytes()
    assert len({vecs[i].tobytes() for i in range(n)}) == n


# ---------------------------------------------------------------------------------------------- 6: every layer
@pytest.mark.parametrize("ref", ['s', 't'])
def test_host_forms_equal_the_device_form(gpu, ref):
    shape, sign, c = (37, 131), (1 if ref == 's' else -1), 3
    k = Rf.case(9, shape, sign, nat.QUANT_OPENCV, c, masked=True)
    want = k['want']
    near, far = Rf.in_layout(k['near'], 'hwc', False), Rf.in_layout(k['far'], 'hwc', False)
    f, fm, nm, am, va = k['f'][0], k['fm'][0], k['near_mask'][0], k['far_mask'][0], k['valid'][0]
    flow = dev.DeviceFlow.from_host(f, ref, fm)
    # a float32 DeviceImage is an 'hwc' tensor
    out, data = flow.refine(dev.DeviceImage.from_host(near), dev.DeviceImage.from_host(far), near_mask=up(nm), far_mask=up(am),
                            valid=up(va), return_data=True)
    assert isinstance(out, dev.DeviceFlow) and (out.shape, out.ref) == (shape, ref)
    d_vecs, d_data = out.vecs.to_host(shape + (2,), F32), data.to_host(shape, U8)
    check((d_vecs[None], d_data[None]), want, "device")
    np.testing.assert_array_equal(out.mask.to_host(shape, U8), fm.astype(U8))
    # the raw ABI
    check(raw_call(k['near'], k['far'], 'float32', 'chw', k['f'], k['fm'], sign, k['near_mask'], k['far_mask'], k['valid']), want, "raw")
    # Flow.refine: channels last, planar, one plane
    h_out, h_data = of.Flow(f, ref, fm).refine(near, far, near_mask=nm, far_mask=am.astype(bool), valid=va, return_data=True)
    assert isinstance(h_out, of.Flow) and h_out.ref == ref and np.array_equal(h_out.mask, fm) and h_data.dtype == np.bool_
    assert h_out.vecs.tobytes() == d_vecs.tobytes() and h_data.tobytes() == d_data.tobytes()
    p_out = of.Flow(f, ref, fm).refine(k['near'][0], k['far'][0], near_mask=nm, far_mask=am, valid=va, layout='chw')
    assert p_out.vecs.tobytes() == d_vecs.tobytes()
    g_out = of.Flow(f, ref, fm).refine(k['near'][0, 0], k['far'][0, 0], alpha=10, sor=2)
    one = Rf.restate(k['near'][:, :1], k['far'][:, :1], f, fm, sign, alpha=10, sor=2)
    assert np.array_equal(bits(g_out.vecs), bits(one['vecs'][0]))
    # arrays in, with and without the mask
    a = of.refine_flow(f, near, far, ref, fm, near_mask=nm, far_mask=am, valid=va)
    assert a.dtype == F32 and a.tobytes() == d_vecs.tobytes()
    full = Rf.restate(k['near'], k['far'], f, np.ones(shape, bool), sign)
    assert np.array_equal(bits(of.refine_flow(f, near, far, ref)), bits(full['vecs'][0]))
    # calling again re-warps: the second call is the restatement of the first call's result
    again = out.refine(dev.DeviceImage.from_host(near), dev.DeviceImage.from_host(far))
    second = Rf.restate(k['near'], k['far'], d_vecs, fm, sign)
    assert np.array_equal(bits(again.vecs.to_host(shape + (2,), F32)), bits(second['vecs'][0]))


def test_the_raw_host_entry(gpu):
    shape, sign, c, dtype, n = (19, 70), -1, 4, 'float16', 2
    h, w = shape
    k = Rf.case(6, shape, sign, nat.QUANT_EXACT, c, dtype, n, True)
    prm = Rf.settings()
    for layout in T.LAYOUTS:
        near, far = Rf.in_layout(k['near'], layout), Rf.in_layout(k['far'], layout)
        f, fm = np.ascontiguousarray(k['f'], F32), np.ascontiguousarray(k['fm']).view(U8)
        out, data = np.empty((n, h, w, 2), F32), np.empty((n, h, w), U8)
        nat.check(nat.load().ofl_refine(near.ctypes.data, far.ctypes.data, EL[dtype], LAYOUT[layout], n, c, h, w, f.ctypes.data, fm.ctypes.data,
                                        sign, k['near_mask'].ctypes.data, k['far_mask'].ctypes.data, k['valid'].ctypes.data,
                                        prm['alpha'], prm['delta'], prm['zeta'], prm['eps'], prm['fixed_point'], prm['sor'], prm['omega'],
                                        out.ctypes.data, data.ctypes.data, nat.QUANT_EXACT))
        check((out, data), k['want'], layout)


def test_uint8_images_equal_their_float32_conversion(gpu):
    shape = (19, 70)
    rng = np.random.default_rng(3)
    k = Rf.case(3, shape, -1, nat.QUANT_OPENCV, 3)
    img0 = np.clip(np.rint(Rf.in_layout(k['near'], 'hwc', False)), 0, 255).astype(np.uint8)
    img1 = np.clip(np.rint(Rf.in_layout(k['far'], 'hwc', False) + rng.uniform(-2, 2, shape + (3,))), 0, 255).astype(np.uint8)
    a = of.refine_flow(k['f'][0], img0, img1, 't', k['fm'][0])
    b = of.refine_flow(k['f'][0], img0.astype(F32), img1.astype(F32), 't', k['fm'][0])
    want = Rf.restate(np.moveaxis(img0.astype(F32), -1, 0)[None], np.moveaxis(img1.astype(F32), -1, 0)[None], k['f'][0], k['fm'][0], -1)
    assert a.tobytes() == b.tobytes() and np.array_equal(bits(a), bits(want['vecs'][0])) and (bits(a) != bits(k['f'][0])).any()


# ---------------------------------------------------------------------------------------------- 7: errors
def test_method_errors(gpu):
    prefix = "Error refining flow: "
    f = dev.DeviceFlow.zero((6, 9), 't')
    t = lambda shape, layout='chw', dtype=np.float32: dev.DeviceTensor.from_host(np.zeros(shape, dtype), layout)
    a = t((3, 6, 9))
    with pytest.raises(ValueError, match=prefix + "the tensors need the same shape"):
        f.refine(a, t((4, 6, 9)))
    with pytest.raises(TypeError, match=prefix + "the tensors need the same dtype, got float32 and float16"):
        f.refine(a, t((3, 6, 9), dtype=np.float16))
    with pytest.raises(ValueError, match=prefix + "the tensors need the same layout, got 'chw' and 'hwc'"):
        f.refine(t((6, 6, 6)), dev.DeviceTensor(a.buf, (6, 6, 6), 'float32', 'hwc'))
    with pytest.raises(ValueError, match=prefix + r"tensors and flow need the same height and width, got \(6, 9\) and \(6, 10\)"):
        dev.DeviceFlow.zero((6, 10), 't').refine(a, a)
    with pytest.raises(TypeError, match=prefix + "near needs to be a DeviceTensor or a float32 DeviceImage, got ndarray"):
        f.refine(np.zeros((3, 6, 9), F32), a)
    with pytest.raises(ValueError, match=prefix + r"the tensors need 1 to 4 channels \(grey, two-plane, RGB, RGBA\), got 5"):
        f.refine(t((5, 6, 9)), t((5, 6, 9)))
    with pytest.raises(ValueError, match=prefix + r"one field takes tensors of shape \(C, H, W\) or \(1, C, H, W\)"):
        f.refine(t((2, 3, 6, 9)), t((2, 3, 6, 9)))
    with pytest.raises(ValueError, match=prefix + r"omega must lie in \(0, 2\)"):
        f.refine(a, a, omega=2)
    with pytest.raises(ValueError, match=prefix + r"sor must be in \[1, 32\], got 33"):
        f.refine(a, a, sor=33)
    with pytest.raises(TypeError, match=prefix + "eps must be a number or None"):
        f.refine(a, a, eps=True)
    with pytest.raises(TypeError, match=prefix + "valid needs to be a DeviceBuffer"):
        f.refine(a, a, valid=np.ones((6, 9), U8))
    with pytest.raises(ValueError, match=prefix + "far_mask needs to hold 54 bytes"):
        f.refine(a, a, far_mask=dev.DeviceBuffer(10))
    b = DeviceFlowBatch.from_flows([of.Flow.zero((6, 9), 't')] * 2)
    with pytest.raises(ValueError, match=prefix + r"a batch of 2 fields takes tensors of shape \(2, C, H, W\)"):
        b.refine(a, a)
    with pytest.raises(ValueError, match=prefix + "valid needs to hold 108 bytes"):
        b.refine(t((2, 3, 6, 9)), t((2, 3, 6, 9)), valid=dev.DeviceBuffer(54))
    assert f.refine(t((1, 3, 6, 9)), t((1, 3, 6, 9))).vecs.to_host((6, 9, 2), F32).tobytes() == bytes(6 * 9 * 8)


def test_raw_entry_refuses_bad_arguments_without_launching(gpu):
    lib = nat.load()
    n = 6 * 9
    t, f, fm = dev.DeviceBuffer.zeros(n * 5 * 4), dev.DeviceBuffer.zeros(n * 8), dev.DeviceBuffer.zeros(n)
    out, data, work = dev.DeviceBuffer.zeros(n * 8 + 8), dev.DeviceBuffer.zeros(n), dev.DeviceBuffer.zeros(29 * n + 8)
    nat.check(lib.ofl_memset(out.ptr, 7, n * 8, None))
    nat.check(lib.ofl_memset(data.ptr, 7, n, None))
    p = Rf.settings()

    def call(near=t.ptr, far=t.ptr, elem=nat.EL_F32, layout=nat.TENSOR_NCHW, N=1, C=3, h=6, w=9, flow=f.ptr, fmask=fm.ptr, sign=1,
             alpha=p['alpha'], delta=p['delta'], zeta=p['zeta'], eps=p['eps'], fixed_point=5, sor=5, omega=p['omega'],
             ws=work.ptr, ws_bytes=29 * n, o=out.ptr, quant=nat.QUANT_OPENCV):
        return lib.ofl_refine_dev(near, far, elem, layout, N, C, h, w, flow, fmask, sign, None, None, None, alpha, delta, zeta, eps,
                                  fixed_point, sor, omega, ws, ws_bytes, o, data.ptr, quant, None)

    for kw in (dict(near=None), dict(far=None), dict(flow=None), dict(fmask=None), dict(o=None), dict(elem=nat.EL_F64), dict(elem=9),
               dict(layout=2), dict(N=0), dict(N=65536), dict(C=0), dict(C=5), dict(h=0), dict(w=32767), dict(sign=0),
               dict(alpha=F32(-1)), dict(alpha=F32('nan')), dict(alpha=F32('inf')), dict(delta=F32(-1)), dict(delta=F32('nan')),
               dict(zeta=F32(0)), dict(zeta=F32(-0.1)), dict(zeta=F32(1e-30)), dict(zeta=F32(1e30)), dict(zeta=F32('nan')),
               dict(eps=F32(0)), dict(eps=F32(-0.1)), dict(eps=F32(1e-30)), dict(eps=F32('inf')),
               dict(fixed_point=0), dict(fixed_point=33), dict(sor=0), dict(sor=33),
               dict(omega=F32(0)), dict(omega=F32(2)), dict(omega=F32('nan')), dict(quant=7),
               dict(ws=None), dict(ws_bytes=29 * n - 1), dict(ws=work.ptr + 4), dict(near=t.ptr + 2), dict(flow=f.ptr + 4), dict(o=out.ptr + 4),
               dict(o=f.ptr), dict(ws=out.ptr), dict(o=t.ptr)):
        assert call(**kw) == nat.E_INVALID, kw
        assert "ofl_refine" in nat.last_error(), kw
    dev.sync()
    assert (out.to_host((n * 8,), U8) == 7).all() and (data.to_host((n,), U8) == 7).all()         # nothing was launched
    assert call() == nat.OK
    assert not out.to_host((n * 2,), F32).any() and not data.to_host((n,), U8).any()              # an empty mask: the input comes back
