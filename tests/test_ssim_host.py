"""K26 without a GPU: the known answers of the NumPy restatement (tests/ssim_ref.py) through their bits, the restatement
against the float64 definition within the derived bound, the float64 definition against two independent formulations
(SciPy's separable correlation in Wang's form, torch's avg_pool2d form of ARFlow), args.ssim_args, and the entries
without a device."""
import itertools

import numpy as np
import pytest

import oflibnumpy_amd as of
import census_ref as Cn
import interop_ref as R
import photometric_ref as P
import ssim_ref as Sm
import tensor_ref as T
from oracle import np_oracle as O
from oflibnumpy_amd import _native as nat
from oflibnumpy_amd.args import ssim_args

F32 = np.float32
BOTH = [(K, w) for K in Sm.WINDOWS for w in Sm.WEIGHTS]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- 1: known answers
@pytest.mark.parametrize("sign", Sm.SIGNS)
def test_near_equal_to_the_warped_far_has_no_error(sign):
    """mu_a == mu_b and va == vb == vab bit for bit, 2 x and x + x are the same float: num == den, s = 1, e = +0.0"""
    near, far, f, fm = Cn.translation(sign=sign)
    for K, weights in BOTH:
        r = Sm.restate(near, far, f, fm, sign, K=K, g=Sm.taps(K, weights), tau=0.0)
        cov = r['covered']
        assert cov.sum() == (37 - 2 - 2 * (K // 2)) * (131 - 3 - 2 * (K // 2))
        assert bits(r['e'])[cov].max() == 0 and bits(r['err']).max() == 0 and np.array_equal(r['within'], cov)
        assert (r['s'][cov] == 1).all()
        low = Sm.restate(near, far, f, fm, sign, K=K, g=Sm.taps(K, weights), min_count=1)     # partial windows too
        assert low['covered'].sum() == (37 - 2) * (131 - 3) and bits(low['err']).max() == 0


@pytest.mark.parametrize("c", [1, 2, 4])
def test_two_constant_images_under_a_uniform_window(c):
    shape, a0, b0 = (19, 70), 100.0, 141.0
    near, far = np.full((1, c) + shape, a0, F32), np.full((1, c) + shape, b0, F32)
    f, fm = np.zeros(shape + (2,), F32), np.ones(shape, bool)
    want = Sm.constants(a0, b0)
    assert 0 < want < 0.1
    for K in Sm.WINDOWS:
        r = Sm.restate(near, far, f, fm, 1, K=K, g=Sm.taps(K, 'uniform'), min_count=1)
        assert r['covered'].all() and (bits(r['err']) == bits(want)).all(), K
        n = r['n'].astype(F32)
        for got, exact in zip(r['S'], (n, n * F32(a0), n * F32(b0), n * F32(a0 * a0), n * F32(b0 * b0), n * F32(a0 * b0))):
            assert (bits(got) == bits(exact)).all()


@pytest.mark.parametrize("K, weights", BOTH)
def test_one_differing_pixel_reaches_its_window_and_no_further(K, weights):
    at, r = (18, 60), K // 2
    near, far, f, fm = Cn.translation()
    g = Sm.taps(K, weights)
    clean = Sm.restate(near, far, f, fm, 1, K=K, g=g, min_count=1)
    near = near.copy()
    near[0, :, at[0], at[1]] = 1000.0
    got = Sm.restate(near, far, f, fm, 1, K=K, g=g, min_count=1)
    block = np.zeros((37, 131), bool)
    block[at[0] - r:at[0] + r + 1, at[1] - r:at[1] + r + 1] = True
    assert block.sum() == K * K and clean['covered'][0][block].all()
    np.testing.assert_array_equal(bits(got['err'][0]) != bits(clean['err'][0]), block)
    assert (got['err'][0][block] > 0).all() and np.array_equal(got['covered'], clean['covered'])


@pytest.mark.parametrize("K, min_count", [(3, 9), (5, 13), (7, 1), (7, 49), (11, 61), (11, 121)])
def test_covered_is_k21s_covered_eroded_with_the_centre_counted(K, min_count):
    k = Sm.case(3, (37, 131), 1, O.QUANT_OPENCV, 1, 'float32', K, 'uniform')
    near, far = R.to_f32(k['near'], 'float32'), R.to_f32(k['far'], 'float32')
    cov1 = P.restate(near, far, k['f'], k['fm'], 1)['covered']
    r = Sm.restate(near, far, k['f'], k['fm'], 1, K=K, g=k['g'], min_count=min_count)
    np.testing.assert_array_equal(r['covered'], Sm.eroded(cov1, K, min_count))
    assert not (r['covered'] & ~cov1).any() and (min_count == 1 or r['covered'].sum() < cov1.sum())
    if min_count == 1:
        np.testing.assert_array_equal(r['covered'], cov1)                  # the centre alone is enough
    # counted by hand
    pad = np.pad(cov1[0], K // 2)
    box = sum(pad[dy:dy + 37, dx:dx + 131].astype(int) for dy in range(K) for dx in range(K))
    np.testing.assert_array_equal(r['n'][0], box)
    np.testing.assert_array_equal(r['covered'][0], cov1[0] & (box >= min_count))


@pytest.mark.parametrize("K", Sm.WINDOWS)
def test_uniform_taps_sum_to_the_member_count_bit_for_bit(K):
    k = Sm.case(1, (37, 131), -1, O.QUANT_EXACT, 3, 'float32', K, 'uniform')
    r = Sm.restate(R.to_f32(k['near'], 'float32'), R.to_f32(k['far'], 'float32'), k['f'], k['fm'], -1, K=K, g=k['g'], quant=O.QUANT_EXACT)
    assert (bits(r['S'][0]) == bits(r['n'].astype(F32))).all() and r['n'].min() < K * K == r['n'].max()


def test_a_nan_outside_the_members_does_not_leak_and_one_inside_does():
    k = Sm.case(1, (19, 70), 1, O.QUANT_OPENCV, 1, 'float32', 3, 'uniform')
    near0, far = R.to_f32(k['near'], 'float32'), R.to_f32(k['far'], 'float32')
    kw = dict(K=3, g=k['g'], min_count=1)
    clean = Sm.restate(near0, far, k['f'], k['fm'], 1, **kw)
    hole = np.argwhere(~np.asarray(k['fm']))[0]                             # a pixel the field's mask leaves out: no member
    near = near0.copy()
    near[0, 0, hole[0], hole[1]] = np.nan
    r = Sm.restate(near, far, k['f'], k['fm'], 1, **kw)
    assert np.array_equal(r['covered'], clean['covered']) and not np.isnan(r['err']).any()
    assert (bits(r['err']) == bits(clean['err'])).all()
    y, x = np.argwhere(clean['covered'][0])[40]
    near = near0.copy()
    near[0, 0, y, x] = np.nan
    r = Sm.restate(near, far, k['f'], k['fm'], 1, tau=1.0, **kw)
    bad = np.isnan(r['err'][0])
    assert bad[y, x] and bad.sum() <= 9 and np.array_equal(bad, np.isnan(r['e'][0]) & r['covered'][0])
    assert not r['within'][0][bad].any() and r['covered'][0][bad].all()   # a NaN is covered and never within


# ---------------------------------------------------------------------------------------------- 2: accuracy
GRID = [(3, 'uniform'), (5, 'uniform'), (7, 'uniform'), (11, 'gaussian')]


@pytest.mark.parametrize("shape", Sm.SHAPES, ids=lambda s: "{}x{}".format(*s))
def test_restatement_stays_within_the_derived_bound_of_float64(shape):
    worst_ratio, worst_abs = 0.0, 0.0
    for i, ((K, weights), c) in enumerate(itertools.product(GRID, [1, 3])):
        for sign in Sm.SIGNS:
            quant = Sm.QUANTS[i % 2]
            k = Sm.case(1, shape, sign, quant, c, 'float32', K, weights)
            want, near = k['want'], R.to_f32(k['near'], 'float32')
            amax = float(max(np.abs(near).max(), np.abs(want['warped']).max()))
            e64, _, n64 = Sm.definition64(near, want['warped'], want['cov1'], K, k['g'])
            np.testing.assert_array_equal(n64, want['n'])
            cov = want['covered']
            b = Sm.bound(K, k['g'], c, amax)
            assert 0 < b < 0.5, (K, c, b)                                 # a worst case, but it says something: e lies in [0, 1]
            diff = np.abs(want['e'].astype(np.float64) - e64)[cov]
            worst_ratio, worst_abs = max(worst_ratio, float(diff.max() / b)), max(worst_abs, float(diff.max()))
            assert diff.max() / b <= 1.0, (shape, K, weights, c, sign, float(diff.max()), b)
    print("largest |e32 - e64| at {}: {:.3g} absolute, {:.3g} of the bound".format(shape, worst_abs, worst_ratio))


def _all_valid(shape, c, seed=5):
    """an all-valid field of about 1 px and its pair; -> near, warped (1, c, h, w) float32, cov1"""
    h, w = shape
    rng = np.random.default_rng(seed)
    f = Cn.smooth(rng, h, w, 1.0)
    fm = np.ones(shape, bool)
    near, far = Cn.tensors(rng, 1, c, f, 1, 'float32', 255.0)
    base = P.restate(near, far, f, fm, 1, quant=O.QUANT_EXACT)
    return near, base['warped'], base['covered']


@pytest.mark.parametrize("K, weights", [(7, 'uniform'), (11, 'gaussian')])
def test_float64_definition_agrees_with_scipys_separable_correlation(K, weights):
    """Wang's form: normalised taps, one correlation per axis, the moments as they come"""
    from scipy.ndimage import correlate1d
    c = 3
    near, warped, cov1 = _all_valid((37, 131), c)
    g = Sm.taps(K, weights)
    e64, _, n = Sm.definition64(near, warped, cov1, K, g)
    inside = n[0] == K * K
    assert inside.sum() > 1000
    A, B = near.astype(np.float64).mean(axis=1)[0], warped.astype(np.float64).mean(axis=1)[0]
    wn = g.astype(np.float64) / g.astype(np.float64).sum()
    blur = lambda a: correlate1d(correlate1d(a, wn, axis=0, mode='constant'), wn, axis=1, mode='constant')
    mu_a, mu_b = blur(A), blur(B)
    va, vb, vab = blur(A * A) - mu_a ** 2, blur(B * B) - mu_b ** 2, blur(A * B) - mu_a * mu_b
    c1, c2 = float(Sm.C1), float(Sm.C2)
    s = (2 * mu_a * mu_b + c1) * (2 * vab + c2) / ((mu_a ** 2 + mu_b ** 2 + c1) * (va + vb + c2))
    other = np.clip((1 - s) / 2, 0, 1)
    amax = float(max(np.abs(near).max(), np.abs(warped).max()))
    b = 2 * Sm.bound(K, g, c, amax, u=2.0 ** -53)                          # both sides are within the bound of the exact value
    ratio = float(np.abs(other - e64[0])[inside].max() / b)
    print("K = {} {}: largest |scipy - definition64| / bound = {:.3g} (bound {:.3g})".format(K, weights, ratio, b))
    assert b < 1e-9 and ratio <= 1.0


def test_float64_definition_agrees_with_the_avg_pool2d_form():
    """ARFlow's SSIM term: avg_pool2d(., 3, 1) moments and clamp((1 - SSIM) / 2, 0, 1)"""
    import torch
    from torch.nn.functional import avg_pool2d
    K, c = 3, 3
    near, warped, cov1 = _all_valid((37, 131), c)
    g = Sm.taps(K, 'uniform')
    e64, _, n = Sm.definition64(near, warped, cov1, K, g)
    x = torch.from_numpy(near.astype(np.float64).mean(axis=1))[None]
    y = torch.from_numpy(warped.astype(np.float64).mean(axis=1))[None]
    c1, c2 = float(Sm.C1), float(Sm.C2)
    mu_x, mu_y = avg_pool2d(x, 3, 1), avg_pool2d(y, 3, 1)
    sigma_x, sigma_y = avg_pool2d(x * x, 3, 1) - mu_x * mu_x, avg_pool2d(y * y, 3, 1) - mu_y * mu_y
    sigma_xy = avg_pool2d(x * y, 3, 1) - mu_x * mu_y
    ssim_n = (2 * mu_x * mu_y + c1) * (2 * sigma_xy + c2)
    ssim_d = (mu_x * mu_x + mu_y * mu_y + c1) * (sigma_x + sigma_y + c2)
    other = torch.clamp((1 - ssim_n / ssim_d) / 2, 0, 1)[0, 0].numpy()     # (h - 2, w - 2): the interior
    inside = (n[0] == K * K)[1:-1, 1:-1]
    assert inside.sum() > 1000
    amax = float(max(np.abs(near).max(), np.abs(warped).max()))
    b = 2 * Sm.bound(K, g, c, amax, u=2.0 ** -53)
    ratio = float(np.abs(other - e64[0, 1:-1, 1:-1])[inside].max() / b)
    print("K = 3 uniform: largest |avg_pool2d - definition64| / bound = {:.3g} (bound {:.3g})".format(ratio, b))
    assert b < 1e-9 and ratio <= 1.0


def test_the_bound_is_the_stated_one():
    u = Sm.U
    g = Sm.taps(3, 'uniform')
    assert Sm.gamma(5) == 5 * u / (1 - 5 * u)
    d = Sm.gamma(2)
    e1, e2, w = d + u * (1 + d), (2 * d + d * d) + Sm.gamma(2) * (1 + d) ** 2, Sm.gamma(9)
    q1, q2 = (e1 + w * (1 + e1) + w) / (1 - w), (e2 + w * (1 + e2) + w) / (1 - w)
    M1, M2 = q1 + u * (1 + q1), q2 + u * (1 + q2)
    V = (M2 + (2 * M1 + M1 * M1) + u * (1 + M1) ** 2) * (1 + u) + u
    c1, c2 = float(Sm.C1), float(Sm.C2)
    rL = Sm.gamma(3) + (1 + Sm.gamma(2)) * (2 * 255.0 * M1 / np.sqrt(2 * c1) + 2 * 255.0 ** 2 * M1 * M1 / c1)
    rC = Sm.gamma(2) + (1 + Sm.gamma(2)) * 2 * 255.0 ** 2 * V / c2
    ds = (2 * (rL + rC) + rL * rC) / ((1 - rL) * (1 - rC)) * (1 + Sm.gamma(3)) + Sm.gamma(3)
    assert Sm.bound(3, g, 1, 255.0) == 0.5 * ds * (1 + u) + u
    assert Sm.bound(3, g, 1, 255.0, u=2.0 ** -53) < 1e-10 < 1e-4 < Sm.bound(3, g, 1, 255.0) < Sm.bound(11, Sm.taps(11), 4, 255.0) < 0.1
    assert Sm.bound(3, g, 1, 1e6) == np.inf                                 # it says so where it says nothing


# ---------------------------------------------------------------------------------------------- 3: layout and element type
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_layout_and_widening_do_not_change_the_result(dtype):
    k = Sm.case(2, (19, 70), -1, O.QUANT_OPENCV, 3, dtype, 5, 'uniform', 2)
    want = k['want']
    kw = dict(K=5, g=k['g'], min_count=k['min_count'], tau=k['tau'])
    for layout in T.LAYOUTS:
        near, far = Sm.in_layout(k['near'], layout), Sm.in_layout(k['far'], layout)
        got = Sm.ssim(near, far, dtype, layout, k['f'], k['fm'], -1, **kw)
        np.testing.assert_array_equal(bits(got['err']), bits(want['err']))
        np.testing.assert_array_equal(got['covered'], want['covered'])
        np.testing.assert_array_equal(got['within'], want['within'])
        assert got['counts'] == want['counts']


# ---------------------------------------------------------------------------------------------- 4: ssim_args
def test_ssim_args_defaults_and_values():
    window, taps, c1, c2, min_count, thr = ssim_args()
    assert (window, min_count, thr) == (11, 121, None) and taps.dtype == F32 and taps.shape == (11,)
    assert type(c1) is F32 and type(c2) is F32 and c1 == F32(6.5025) and c2 == F32(58.5225)
    assert c1 == Sm.C1 and c2 == Sm.C2 and taps.tobytes() == Sm.taps(11, 'gaussian', 1.5).tobytes()
    assert abs(float(taps.astype(np.float64).sum()) - 1.0) <= 2.0 ** -24 and (taps == taps[::-1]).all() and taps.argmax() == 5
    for K in (3, 5, 7, 11):
        for sigma in (0.5, 1.5, 4.0):
            t = ssim_args(K, sigma=sigma)[1]
            assert t.tobytes() == Sm.taps(K, 'gaussian', sigma).tobytes() and (t > 0).all()
            assert abs(float(t.astype(np.float64).sum()) - 1.0) <= 2.0 ** -24, (K, sigma)
    window, taps, c1, c2, min_count, thr = ssim_args(np.int32(3), 'uniform', data_range=1.0, k1=0.02, k2=0.06, min_count=np.int64(5), threshold=np.float64(0.25))
    assert (window, min_count) == (3, 5) and taps.tobytes() == np.ones(3, F32).tobytes() and type(thr) is F32 and thr == F32(0.25)
    assert c1 == F32(0.02 ** 2) and c2 == F32(0.06 ** 2)
    assert ssim_args(7, 'uniform')[4] == 49 and ssim_args(5)[4] == 25 and ssim_args(threshold=0)[5] == 0


@pytest.mark.parametrize("kw, exc, text", [
    (dict(window=4), ValueError, "window must be 3, 5, 7 or 11, got 4"),
    (dict(window=9), ValueError, "window must be 3, 5, 7 or 11, got 9"),
    (dict(window=13), ValueError, "window must be 3, 5, 7 or 11, got 13"),
    (dict(window=3.0), TypeError, "window must be an integer, got float"),
    (dict(window=True), TypeError, "window must be an integer, got bool"),
    (dict(weights='box'), ValueError, "weights must be 'gaussian' or 'uniform', got 'box'"),
    (dict(weights=1), TypeError, "weights must be a string, got int"),
    (dict(weights='uniform', sigma=1.5), ValueError, "sigma belongs to weights 'gaussian' and must be None with weights 'uniform'"),
    (dict(sigma=0), ValueError, "sigma must be finite and positive, got 0"),
    (dict(sigma=-1.5), ValueError, "sigma must be finite and positive"),
    (dict(sigma=float('nan')), ValueError, "sigma must be finite and positive"),
    (dict(sigma=float('inf')), ValueError, "sigma must be finite and positive"),
    (dict(sigma=0.05), ValueError, "sigma must leave every tap of window 11 positive in float32"),
    (dict(sigma='1.5'), TypeError, "sigma must be a number or None, got str"),
    (dict(sigma=True), TypeError, "sigma must be a number or None, got bool"),
    (dict(data_range=0), ValueError, "data_range must be finite and positive, got 0"),
    (dict(data_range=-255), ValueError, "data_range must be finite and positive"),
    (dict(data_range=float('inf')), ValueError, "data_range must be finite and positive"),
    (dict(data_range=None), TypeError, "data_range must be a number, got NoneType"),
    (dict(data_range=1e30), ValueError, "(k1 * data_range)^2 must be finite and positive in float32"),
    (dict(k1=0), ValueError, "k1 must be finite and positive, got 0"),
    (dict(k1=float('nan')), ValueError, "k1 must be finite and positive"),
    (dict(k1=1e-30), ValueError, "(k1 * data_range)^2 must be finite and positive in float32"),
    (dict(k1=True), TypeError, "k1 must be a number, got bool"),
    (dict(k2=-0.03), ValueError, "k2 must be finite and positive"),
    (dict(k2=[0.03]), TypeError, "k2 must be a number, got list"),
    (dict(k2=1e-30), ValueError, "(k2 * data_range)^2 must be finite and positive in float32"),
    (dict(min_count=0), ValueError, "min_count must be in [1, 121] for window 11, got 0"),
    (dict(window=3, min_count=10), ValueError, "min_count must be in [1, 9] for window 3, got 10"),
    (dict(min_count=2.0), TypeError, "min_count must be an integer or None, got float"),
    (dict(min_count=True), TypeError, "min_count must be an integer or None, got bool"),
    (dict(threshold=-1), ValueError, "threshold must be finite and not negative, got -1"),
    (dict(threshold=float('nan')), ValueError, "threshold must be finite and not negative"),
    (dict(threshold=1e300), ValueError, "threshold must be finite and not negative"),
    (dict(threshold=False), TypeError, "threshold must be a number or None, got bool"),
])
def test_ssim_args_rejects(kw, exc, text):
    with pytest.raises(exc) as e:
        ssim_args(**kw)
    assert str(e.value).startswith("Error computing structural similarity: ") and text in str(e.value)


# ---------------------------------------------------------------------------------------------- 5: the host forms, no device
def test_host_forms_refuse_bad_arrays_before_any_native_call():
    prefix = "Error computing structural similarity: "
    h = of.Flow.zero((6, 9), 't')
    z = lambda *shape, dtype=F32: np.zeros(shape, dtype)
    with pytest.raises(ValueError, match=prefix + "the arrays need the same shape"):
        h.ssim(z(6, 9, 3), z(6, 9, 4))
    with pytest.raises(TypeError, match=prefix + "the arrays need the same dtype"):
        h.ssim(z(6, 9, 3), z(6, 9, 3, dtype=np.float16))
    with pytest.raises(ValueError, match=prefix + "arrays and flow need the same height and width"):
        h.ssim(z(6, 8, 3), z(6, 8, 3))
    with pytest.raises(ValueError, match=prefix + r"the tensors need 1 to 4 channels \(grey, two-plane, RGB, RGBA\), got 5"):
        h.ssim(z(6, 9, 5), z(6, 9, 5))
    with pytest.raises(TypeError, match=prefix + "far needs to have dtype float32, float16 or uint8, got float64"):
        h.ssim(z(6, 9, 3), z(6, 9, 3, dtype=np.float64))
    with pytest.raises(TypeError, match=prefix + "near needs to be a numpy array, got list"):
        h.ssim([[0.0]], z(6, 9))
    with pytest.raises(ValueError, match=prefix + "layout must be 'chw' or 'hwc'"):
        h.ssim(z(6, 9, 3), z(6, 9, 3), layout='nhwc')
    with pytest.raises(ValueError, match=prefix + r"near needs to have shape \(H, W\)"):
        h.ssim(z(1, 1, 6, 9, 3), z(1, 1, 6, 9, 3))
    with pytest.raises(ValueError, match=prefix + "weights must be"):
        of.ssim_error(z(6, 9, 2), z(6, 9), z(6, 9), 't', weights='hann')
    with pytest.raises(ValueError, match=prefix + "window must be"):       # the settings are looked at first
        h.ssim(z(6, 9, 5), z(6, 9, 5), window=9)
    assert 'ssim_error' in of.flow_operations.__all__ and of.ssim_error is of.flow_operations.ssim_error
    assert nat.SSIM_MAX_C == 4 and "ofl_ssim_dev" in nat.SIGNATURES and "ofl_ssim" in nat.SIGNATURES


def test_entries_without_a_device():
    if nat.device_count() > 0:
        pytest.skip("a GPU is present")
    f = of.Flow.zero((4, 6), 't')
    img = np.zeros((4, 6, 3), np.uint8)
    with pytest.raises(nat.NoDeviceError):
        f.ssim(img, img)
    with pytest.raises(nat.NoDeviceError):
        of.ssim_error(np.zeros((4, 6, 2), F32), img, img, 't', window=3, weights='uniform', threshold=0.5)
    lib, g = nat.load(), Sm.taps(11)
    assert lib.ofl_ssim_dev(None, None, nat.EL_F32, nat.TENSOR_NCHW, 1, 3, 4, 6, None, None, 1, 1, None, None, 11, g.ctypes.data,
                            Sm.C1, Sm.C2, 121, F32(0), None, None, None, None, nat.QUANT_OPENCV, None) == nat.E_NODEVICE
    assert lib.ofl_ssim(None, None, nat.EL_F32, nat.TENSOR_NCHW, 1, 3, 4, 6, None, None, 1, 1, None, None, 11, g.ctypes.data,
                        Sm.C1, Sm.C2, 121, F32(0), None, None, None, None, nat.QUANT_OPENCV) == nat.E_NODEVICE
