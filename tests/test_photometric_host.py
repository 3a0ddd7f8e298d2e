"""K21 without a GPU: the NumPy restatement (tests/photometric_ref.py) against the float64 definition within the derived
bounds, its independence of layout and element type, the known answers, and args.photometric_args."""
import itertools

import numpy as np
import pytest

import interop_ref as R
import photometric_ref as P
import tensor_ref as T
from oracle import np_oracle as O
from oflibnumpy_amd import _native as nat
from oflibnumpy_amd.args import photometric_args, photometric_host_array, PHOTO_EPS

F32 = np.float32


# ---------------------------------------------------------------------------------------------- 1: the float64 bound
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "{}x{}".format(*s))
def test_restatement_stays_within_the_derived_bound_of_float64(shape):
    worst = {}
    for sign, quant, c, metric in itertools.product(P.SIGNS, P.QUANTS, [1, 3, 5, 33], P.METRICS):
        k = P.case(1, shape, sign, quant, c, 'float32', metric)
        want = k['want']
        e64 = P.definition64(R.to_f32(k['near'], 'float32'), want['warped'], metric)
        rel, absolute = P.bound(c, metric)
        cov = want['covered']
        assert cov.any()
        ratio = np.abs(want['e'].astype(np.float64) - e64)[cov] / (rel * np.abs(e64[cov]) + absolute + 1e-300)
        worst[metric] = max(worst.get(metric, 0.0), float(ratio.max()))
        assert ratio.max() <= 1.0, (shape, sign, quant, c, metric, float(ratio.max()))
    print("largest |e32 - e64| / bound at {}: {}".format(shape, worst))


def test_the_bound_is_the_stated_one():
    u = 2.0 ** -24
    assert P.bound(3, 'l1') == (5 * u / (1 - 5 * u), 0.0)
    assert P.bound(33, 'l2')[0] == 38 * u / (1 - 38 * u) and P.bound(33, 'charbonnier')[0] == 39 * u / (1 - 39 * u)


def test_the_channel_sum_is_the_stated_order():
    """130 channels: lane 0 of the deal takes the groups 0, 16 and 32; powers of two make every partial sum visible"""
    t = (np.arange(130, dtype=np.float64) % 7 + 1).astype(F32)[:, None] * F32(2.0 ** -20) + F32(1.0)
    p = [F32(0)] * 16
    for c in range(130):
        p[(c // 4) % 16] = F32(p[(c // 4) % 16] + t[c, 0])
    s = F32(F32(F32(F32(p[0] + p[8]) + F32(p[4] + p[12])) + F32(F32(p[2] + p[10]) + F32(p[6] + p[14]))) +
            F32(F32(F32(p[1] + p[9]) + F32(p[5] + p[13])) + F32(F32(p[3] + p[11]) + F32(p[7] + p[15]))))
    assert P.channel_sum(t)[0].view(np.uint32) == s.view(np.uint32)
    # fewer than 16 groups: the empty partial sums are +0.0 and change nothing
    assert P.channel_sum(t[:5])[0] == F32(F32(F32(F32(t[0, 0] + t[1, 0]) + t[2, 0]) + t[3, 0]) + t[4, 0])


# ---------------------------------------------------------------------------------------------- 2: layout and element type
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_layout_and_widening_do_not_change_the_result(dtype):
    k = P.case(2, (19, 70), -1, O.QUANT_OPENCV, 5, dtype, 'charbonnier', n=2)
    want = k['want']
    for layout in T.LAYOUTS:
        near, far = P.in_layout(k['near'], layout), P.in_layout(k['far'], layout)
        got = P.photometric(near, far, dtype, layout, k['f'], k['fm'], -1, metric='charbonnier', tau=k['tau'])
        wide = P.photometric(R.to_f32(near, dtype), R.to_f32(far, dtype), 'float32', layout, k['f'], k['fm'], -1,
                             metric='charbonnier', tau=k['tau'])
        for r in (got, wide):
            np.testing.assert_array_equal(r['err'].view(np.uint32), want['err'].view(np.uint32))
            np.testing.assert_array_equal(r['covered'], want['covered'])
            np.testing.assert_array_equal(r['within'], want['within'])
            assert r['counts'] == want['counts']


# ---------------------------------------------------------------------------------------------- 3: known answers
@pytest.mark.parametrize("sign", P.SIGNS)
@pytest.mark.parametrize("metric", P.METRICS[:2])
def test_integer_translation_has_no_error(sign, metric):
    near, far, f, fm = P.translation(sign=sign)
    r = P.restate(near, far, f, fm, sign, metric=metric, tau=0.0)
    assert not r['err'].any() and r['err'].view(np.uint32).max() == 0
    assert r['counts'] == [((37 - 2) * (131 - 3),) * 2]
    rows, cols = np.nonzero(r['covered'][0])
    assert (rows.max() - rows.min() + 1, cols.max() - cols.min() + 1) == (35, 128)
    np.testing.assert_array_equal(r['within'], r['covered'])


@pytest.mark.parametrize("quant", P.QUANTS)
def test_l1_of_one_channel_against_zero_is_the_magnitude_of_the_warp(quant):
    k = P.case(3, (37, 131), -1, quant, 1)
    far = R.to_f32(k['far'], 'float32')
    r = P.restate(np.zeros_like(far), far, k['f'], k['fm'], -1, quant=quant)
    warped, valid = T.warp(far, 'float32', 'chw', k['f'], k['fm'], quant=quant)
    np.testing.assert_array_equal(r['covered'][0], valid)
    np.testing.assert_array_equal(r['err'].view(np.uint32), np.where(valid, np.abs(warped[0, 0]), F32(0)).astype(F32)[None].view(np.uint32))


# ---------------------------------------------------------------------------------------------- 4: photometric_args
def test_photometric_args_defaults_and_values():
    code, eps, thr = photometric_args()
    assert code == nat.PHOTO_L1 and type(eps) is F32 and eps == F32(PHOTO_EPS) == F32(1e-3) and thr is None
    assert photometric_args('l2')[0] == nat.PHOTO_L2 and photometric_args('charbonnier', 0.5, 2)[0] == nat.PHOTO_CHARBONNIER
    code, eps, thr = photometric_args('charbonnier', 0, np.float64(0.1))
    assert eps == 0 and type(thr) is F32 and thr == F32(0.1)
    assert photometric_args(threshold=np.int64(3))[2] == F32(3)


@pytest.mark.parametrize("kw, exc, text", [
    (dict(metric='L1'), ValueError, "metric must be 'l1', 'l2' or 'charbonnier', got 'L1'"),
    (dict(metric=1), TypeError, "metric must be a string, got int"),
    (dict(metric=None), TypeError, "metric must be a string, got NoneType"),
    (dict(eps=-1e-3), ValueError, "eps must be finite and not negative, got -0.001"),
    (dict(eps=float('nan')), ValueError, "eps must be finite and not negative"),
    (dict(eps=float('inf')), ValueError, "eps must be finite and not negative"),
    (dict(eps=1e39), ValueError, "eps must be finite and not negative"),
    (dict(eps=True), TypeError, "eps must be a number or None, got bool"),
    (dict(eps='1'), TypeError, "eps must be a number or None, got str"),
    (dict(threshold=-1), ValueError, "threshold must be finite and not negative, got -1"),
    (dict(threshold=float('nan')), ValueError, "threshold must be finite and not negative"),
    (dict(threshold=1e300), ValueError, "threshold must be finite and not negative"),
    (dict(threshold=False), TypeError, "threshold must be a number or None, got bool"),
    (dict(threshold=[1.0]), TypeError, "threshold must be a number or None, got list"),
])
def test_photometric_args_rejects(kw, exc, text):
    with pytest.raises(exc) as e:
        photometric_args(**kw)
    assert str(e.value).startswith("Error computing photometric error: ") and text in str(e.value)


def test_host_arrays():
    img = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)
    a = photometric_host_array(img, 'hwc', "near")
    assert a.dtype == F32 and a.shape == (2, 4, 3) and np.array_equal(a, img)
    assert photometric_host_array(np.zeros((2, 4), F32), 'hwc', "near").shape == (2, 4, 1)
    assert photometric_host_array(np.zeros((2, 4), np.float16), 'chw', "far").shape == (1, 2, 4)
    with pytest.raises(TypeError, match="Error computing photometric error: far needs to have dtype float32, float16 or uint8, got float64"):
        photometric_host_array(np.zeros((2, 4)), 'hwc', "far")
    with pytest.raises(TypeError, match="near needs to be a numpy array, got list"):
        photometric_host_array([1.0], 'hwc', "near")
    with pytest.raises(ValueError, match="layout must be 'chw' or 'hwc'"):
        photometric_host_array(np.zeros((2, 4), F32), 'nhwc', "near")
    with pytest.raises(ValueError, match="near needs to have shape"):
        photometric_host_array(np.zeros((2,), F32), 'hwc', "near")
