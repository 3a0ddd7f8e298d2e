"""K22 without a GPU: the NumPy restatement (tests/census_ref.py) against the float64 definition within the derived bounds,
its summation order, its independence of layout and element type, the known answers, args.census_args, and the raw
entries without a device."""
import itertools

import numpy as np
import pytest

import oflibnumpy_amd as of
import census_ref as Cn
import interop_ref as R
import photometric_ref as P
import tensor_ref as T
from oracle import np_oracle as O
from oflibnumpy_amd import _native as nat
from oflibnumpy_amd.args import census_args, census_channels, CENSUS_NOISE, CENSUS_KNEE

F32 = np.float32


# ---------------------------------------------------------------------------------------------- 1: the float64 bound
@pytest.mark.parametrize("shape", Cn.SHAPES, ids=lambda s: "{}x{}".format(*s))
def test_restatement_stays_within_the_derived_bound_of_float64(shape):
    worst, risky_px = {}, 0
    for i, (K, c, (mode, delta)) in enumerate(itertools.product(Cn.WINDOWS, [1, 3, 4], [('soft', 0.0), ('hard', 0.0), ('hard', 2.0)])):
        sign, quant = Cn.SIGNS[i % 2], Cn.QUANTS[(i // 2) % 2]
        k = Cn.case(1, shape, sign, quant, c, 'float32', K, mode, 1, delta)
        want, near = k['want'], R.to_f32(k['near'], 'float32')
        amax = float(max(np.abs(near).max(), np.abs(want['warped']).max()))
        e64, n64, risky = Cn.definition64(near, want['warped'], want['cov1'], K, mode, k['p0'], k['p1'], guard=Cn.margin(c, amax))
        np.testing.assert_array_equal(n64, want['n'])
        rel, absolute = Cn.bound(K, mode, c, amax)
        use = want['covered'] & ~risky
        assert use.sum() >= 0.5 * want['covered'].sum(), (shape, K, c, mode, delta, int(use.sum()), int(want['covered'].sum()))
        ratio = np.abs(want['e'].astype(np.float64) - e64)[use] / (rel * np.abs(e64[use]) + absolute + 1e-300)
        worst[mode] = max(worst.get(mode, 0.0), float(ratio.max()))
        risky_px += int((risky & want['covered']).sum())
        assert ratio.max() <= 1.0, (shape, K, c, mode, delta, float(ratio.max()))
    print("largest |e32 - e64| / bound at {}: {}; covered pixels left out near the dead zone's edge: {}".format(shape, worst, risky_px))


def test_the_bound_is_the_stated_one():
    u = 2.0 ** -24
    assert Cn.bound(7, 'hard', 3) == (u / (1 - u), 0.0)
    assert Cn.margin(3, 2.0) == 2 * (5 * u / (1 - 5 * u)) * 2.0
    rel, absolute = Cn.bound(5, 'soft', 1, amax=255.0)
    d_rho = Cn.margin(1, 255.0) / np.sqrt(float(F32(0.81))) + Cn.gamma(4)
    d_g = 2 * d_rho + 2 * u
    assert rel == Cn.gamma(24) and absolute == (4 * d_g + d_g * d_g + 4 * u) / float(F32(0.1)) + Cn.gamma(2)


# ---------------------------------------------------------------------------------------------- 2: the order of the sum
def _hand_sum(rows):
    """rows: lists of float32 in ascending dx, rows in ascending dy -> the stated order, written out"""
    S = F32(0)
    for row in rows:
        r = F32(0)
        for t in row:
            r = F32(r + t)
        S = F32(S + r)
    return S


@pytest.mark.parametrize("K", [3, 5])
def test_the_window_sum_is_the_stated_order(K):
    """1 + 2^-24 rounds back to 1 (a tie, to even) while 2^-24 + 2^-24 + 1 does not.  Two examples: in the first the top
    row holds tiny terms LEFT of a 1, so the order inside a row shows; in the second the tiny terms are alone in their
    rows, BELOW a row that holds the 1, so the order of the rows shows."""
    r, one, tiny, zero = K // 2, F32(1), F32(2.0 ** -24), F32(0)
    offsets = [(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx or dy]
    in_row = {(dx, dy): (one if dx == r else tiny) if dy == -r else zero for dx, dy in offsets}
    of_rows = {(dx, dy): (one if dx == 0 else zero) if dy == -r else (tiny if dx == -r else zero) for dx, dy in offsets}
    for t, (right, flipped_dx, flipped_dy) in ((in_row, (F32(1 + (K - 1) * 2.0 ** -24), one, F32(1 + (K - 1) * 2.0 ** -24))),
                                               (of_rows, (one, one, F32(1 + (K - 1) * 2.0 ** -24)))):
        rows = [[t[dx, dy] for dx in range(-r, r + 1) if dx or dy] for dy in range(-r, r + 1)]
        got = Cn.ordered_sum({k: np.array([v], F32) for k, v in t.items()}, K)[0]
        assert got.view(np.uint32) == _hand_sum(rows).view(np.uint32) == right.view(np.uint32)
        assert _hand_sum([row[::-1] for row in rows]) == flipped_dx and _hand_sum(rows[::-1]) == flipped_dy
    # the offsets of the restatement's own loop: an intensity pattern whose rows are flipped in B disagrees in sign at
    # every offset but the K - 1 of the centre's own row
    A = np.arange(K * K, dtype=F32).reshape(1, K, K)
    e, n = Cn.window_mean(A, A[:, ::-1].copy(), np.ones((1, K, K), bool), K, 'hard', F32(0), F32(0))
    assert n[0, r, r] == K * K - 1 and e[0, r, r] == F32(F32(K * K - K) / F32(K * K - 1))


def test_the_channel_mean_is_the_stated_order():
    t = np.array([1.0, 2.0 ** -24, 2.0 ** -24, -0.0], F32).reshape(1, 4, 1, 1)
    assert Cn.intensity(t)[0, 0, 0] == F32(F32(F32(F32(F32(0) + t[0, 0, 0, 0]) + t[0, 1, 0, 0]) + t[0, 2, 0, 0]) * F32(0.25)) == F32(0.25)
    assert Cn.intensity(t[:, ::-1].copy())[0, 0, 0] == F32(F32(1 + 2.0 ** -23) * F32(0.25))
    minus = Cn.intensity(np.full((1, 1, 1, 1), -0.0, F32))                  # the sum starts at +0.0: -0.0 comes out as +0.0
    assert minus.view(np.uint32)[0, 0, 0] == 0
    assert Cn.intensity(np.ones((1, 3, 1, 1), F32))[0, 0, 0] == F32(F32(3) * F32(1.0 / 3.0))


# ---------------------------------------------------------------------------------------------- 3: layout and element type
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("mode", Cn.MODES)
def test_layout_and_widening_do_not_change_the_result(dtype, mode):
    k = Cn.case(2, (19, 70), -1, O.QUANT_OPENCV, 3, dtype, 5, mode, 2)
    want = k['want']
    kw = dict(K=5, mode=mode, p0=k['p0'], p1=k['p1'], min_count=k['min_count'], tau=k['tau'])
    for layout in T.LAYOUTS:
        near, far = Cn.in_layout(k['near'], layout), Cn.in_layout(k['far'], layout)
        got = Cn.census(near, far, dtype, layout, k['f'], k['fm'], -1, **kw)
        wide = Cn.census(R.to_f32(near, dtype), R.to_f32(far, dtype), 'float32', layout, k['f'], k['fm'], -1, **kw)
        for r in (got, wide):
            np.testing.assert_array_equal(r['err'].view(np.uint32), want['err'].view(np.uint32))
            np.testing.assert_array_equal(r['covered'], want['covered'])
            np.testing.assert_array_equal(r['within'], want['within'])
            assert r['counts'] == want['counts']


# ---------------------------------------------------------------------------------------------- 4: known answers
@pytest.mark.parametrize("sign", Cn.SIGNS)
def test_a_gain_and_an_offset_cost_nothing(sign):
    near, far, f, fm = Cn.translation(sign=sign, lo=64)
    near = near * F32(0.5) + F32(16)                                       # exact: halves of small integers
    r = Cn.restate(near, far, f, fm, sign, K=7, mode='hard', p0=0.0, tau=0.0)
    cov = r['covered']
    assert cov.sum() == (37 - 2 - 6) * (131 - 3 - 6) and not r['err'].any() and np.array_equal(r['within'], cov)
    assert (P.restate(near, far, f, fm, sign)['err'][cov] > 10).all()     # K21 reads the same pair as an error everywhere


@pytest.mark.parametrize("sign", Cn.SIGNS)
@pytest.mark.parametrize("mode", Cn.MODES)
def test_integer_translation_has_no_distance(sign, mode):
    near, far, f, fm = Cn.translation(sign=sign)
    for K in Cn.WINDOWS:
        r = Cn.restate(near, far, f, fm, sign, K=K, mode=mode, tau=0.0)
        assert r['err'].view(np.uint32).max() == 0 and r['counts'] == [((37 - 2 - 2 * (K // 2)) * (131 - 3 - 2 * (K // 2)),) * 2]


@pytest.mark.parametrize("K", Cn.WINDOWS)
def test_one_differing_pixel_reaches_its_window_and_no_further(K):
    at, r = (18, 60), K // 2
    near, far, f, fm = Cn.reach(at=at)
    got = Cn.restate(near, far, f, fm, 1, K=K, mode='hard', p0=0.0, min_count=1)
    want = np.zeros((37, 131), F32)
    n = got['n'][0]
    want[at[0] - r:at[0] + r + 1, at[1] - r:at[1] + r + 1] = F32(1) / n[at[0] - r:at[0] + r + 1, at[1] - r:at[1] + r + 1].astype(F32)
    want[at] = F32(1)
    assert got['covered'][0, at[0] - r:at[0] + r + 1, at[1] - r:at[1] + r + 1].all() and (n[at] == K * K - 1)
    np.testing.assert_array_equal(got['err'][0].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("K, min_count", [(3, 8), (5, 12), (7, 1), (7, 48)])
def test_covered_is_k21s_covered_eroded_by_the_member_count(K, min_count):
    k = Cn.case(3, (37, 131), 1, O.QUANT_OPENCV, 1, 'float32', K, 'hard')
    near, far = R.to_f32(k['near'], 'float32'), R.to_f32(k['far'], 'float32')
    cov1 = P.restate(near, far, k['f'], k['fm'], 1)['covered']
    r = Cn.restate(near, far, k['f'], k['fm'], 1, K=K, mode='hard', min_count=min_count)
    np.testing.assert_array_equal(r['covered'], Cn.eroded(cov1, K, min_count))
    assert not (r['covered'] & ~cov1).any() and (min_count == 1 or r['covered'].sum() < cov1.sum())


def test_a_window_larger_than_the_frame_covers_nothing_at_the_default():
    k = Cn.case(1, (5, 7), 1, O.QUANT_OPENCV, 3, 'float32', 7, 'soft')
    r = Cn.restate(R.to_f32(k['near'], 'float32'), R.to_f32(k['far'], 'float32'), k['f'], k['fm'], 1, K=7, mode='soft')
    assert not r['covered'].any() and r['err'].view(np.uint32).max() == 0 and k['want']['covered'].any()


def test_a_nan_outside_the_members_does_not_leak():
    k = Cn.case(1, (19, 70), 1, O.QUANT_OPENCV, 1, 'float32', 3, 'soft')
    near = R.to_f32(k['near'], 'float32').copy()
    hole = np.argwhere(~np.asarray(k['fm']))[0]                             # a pixel the field's mask leaves out: no member
    near[0, 0, hole[0], hole[1]] = np.nan
    r = Cn.restate(near, R.to_f32(k['far'], 'float32'), k['f'], k['fm'], 1, K=3, mode='soft', min_count=1)
    assert np.array_equal(r['covered'], Cn.restate(R.to_f32(k['near'], 'float32'), R.to_f32(k['far'], 'float32'), k['f'], k['fm'], 1,
                                                   K=3, mode='soft', min_count=1)['covered'])
    assert not np.isnan(r['err']).any() and np.isnan(r['e'][0, hole[0], hole[1]])


# ---------------------------------------------------------------------------------------------- 5: census_args
def test_census_args_defaults_and_values():
    window, mode, p0, p1, min_count, thr = census_args()
    assert (window, mode, min_count, thr) == (7, nat.CENSUS_SOFT, 48, None)
    assert type(p0) is F32 and type(p1) is F32 and p0 == F32(CENSUS_NOISE) == F32(0.81) and p1 == F32(CENSUS_KNEE) == F32(0.1)
    window, mode, p0, p1, min_count, thr = census_args(3, 'hard')
    assert (window, mode, min_count, thr) == (3, nat.CENSUS_HARD, 8, None) and p0 == 0 and p1 == 0 and type(p0) is F32
    assert census_args(5, 'hard', delta=2, min_count=np.int64(12), threshold=np.float64(0.25)) == (5, nat.CENSUS_HARD, F32(2), F32(0), 12, F32(0.25))
    assert census_args(np.int32(5), 'soft', noise=1, knee=0.5, threshold=0)[2:] == (F32(1), F32(0.5), 24, F32(0))
    assert type(census_args(threshold=1)[5]) is F32
    assert [census_channels(c) for c in (1, 2, 3, 4)] == [1, 2, 3, 4]


@pytest.mark.parametrize("kw, exc, text", [
    (dict(window=4), ValueError, "window must be 3, 5 or 7, got 4"),
    (dict(window=9), ValueError, "window must be 3, 5 or 7, got 9"),
    (dict(window=3.0), TypeError, "window must be an integer, got float"),
    (dict(window=True), TypeError, "window must be an integer, got bool"),
    (dict(mode='ternary'), ValueError, "mode must be 'hard' or 'soft', got 'ternary'"),
    (dict(mode=1), TypeError, "mode must be a string, got int"),
    (dict(mode='soft', delta=1.0), ValueError, "delta belongs to mode 'hard' and must be None with mode 'soft'"),
    (dict(mode='hard', noise=0.81), ValueError, "noise belongs to mode 'soft' and must be None with mode 'hard'"),
    (dict(mode='hard', knee=0.1), ValueError, "knee belongs to mode 'soft' and must be None with mode 'hard'"),
    (dict(mode='hard', delta=-1), ValueError, "delta must be finite and not negative, got -1"),
    (dict(mode='hard', delta=float('nan')), ValueError, "delta must be finite and not negative"),
    (dict(mode='hard', delta=1e39), ValueError, "delta must be finite and not negative"),
    (dict(mode='hard', delta='0'), TypeError, "delta must be a number or None, got str"),
    (dict(noise=0), ValueError, "noise must be finite and positive, got 0"),
    (dict(noise=-0.81), ValueError, "noise must be finite and positive"),
    (dict(noise=1e-60), ValueError, "noise must be finite and positive"),
    (dict(noise=float('inf')), ValueError, "noise must be finite and positive"),
    (dict(noise=True), TypeError, "noise must be a number or None, got bool"),
    (dict(knee=0.0), ValueError, "knee must be finite and positive, got 0.0"),
    (dict(knee=float('nan')), ValueError, "knee must be finite and positive"),
    (dict(knee=[0.1]), TypeError, "knee must be a number or None, got list"),
    (dict(min_count=0), ValueError, "min_count must be in [1, 48] for window 7, got 0"),
    (dict(window=3, min_count=9), ValueError, "min_count must be in [1, 8] for window 3, got 9"),
    (dict(min_count=2.0), TypeError, "min_count must be an integer or None, got float"),
    (dict(min_count=True), TypeError, "min_count must be an integer or None, got bool"),
    (dict(threshold=-1), ValueError, "threshold must be finite and not negative, got -1"),
    (dict(threshold=float('nan')), ValueError, "threshold must be finite and not negative"),
    (dict(threshold=1e300), ValueError, "threshold must be finite and not negative"),
    (dict(threshold=False), TypeError, "threshold must be a number or None, got bool"),
])
def test_census_args_rejects(kw, exc, text):
    with pytest.raises(exc) as e:
        census_args(**kw)
    assert str(e.value).startswith("Error computing census distance: ") and text in str(e.value)


@pytest.mark.parametrize("c", [0, 5, 128])
def test_more_than_four_channels_are_refused_by_name(c):
    with pytest.raises(ValueError) as e:
        census_channels(c)
    assert str(e.value) == "Error computing census distance: the tensors need 1 to 4 channels (grey, two-plane, RGB, RGBA), got {}".format(c)


# ---------------------------------------------------------------------------------------------- 6: without a device
def test_entries_without_a_device():
    if nat.device_count() > 0:
        pytest.skip("a GPU is present")
    f = of.Flow.zero((4, 6), 't')
    img = np.zeros((4, 6, 3), np.uint8)
    with pytest.raises(nat.NoDeviceError):
        f.census(img, img)
    with pytest.raises(nat.NoDeviceError):
        of.census_error(np.zeros((4, 6, 2), F32), img, img, 't', window=3, mode='hard', delta=1, threshold=0.5)
    with pytest.raises(ValueError):                                        # validation comes first
        f.census(img, img, window=4)
    with pytest.raises(ValueError, match="1 to 4 channels"):
        f.census(np.zeros((4, 6, 5), F32), np.zeros((4, 6, 5), F32))
    lib = nat.load()
    assert lib.ofl_census_dev(None, None, nat.EL_F32, nat.TENSOR_NCHW, 1, 3, 4, 6, None, None, 1, 1, None, None, 7, nat.CENSUS_SOFT,
                              F32(0.81), F32(0.1), 48, F32(0), None, None, None, None, nat.QUANT_OPENCV, None) == nat.E_NODEVICE
    assert lib.ofl_census(None, None, nat.EL_F32, nat.TENSOR_NCHW, 1, 3, 4, 6, None, None, 1, 1, None, None, 7, nat.CENSUS_SOFT,
                          F32(0.81), F32(0.1), 48, F32(0), None, None, None, None, nat.QUANT_OPENCV) == nat.E_NODEVICE
