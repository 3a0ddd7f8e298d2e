"""K23 without a GPU: the NumPy restatement (tests/refine_ref.py) on the degenerate shapes, outside the domain and next to
non-finite values; that it refines (the known translation); float32 against float64; args.refine_args; the entries without
a device."""
import numpy as np
import pytest

import oflibnumpy_amd as of
import refine_ref as Rf
from oflibnumpy_amd import _native as nat
from oflibnumpy_amd.args import refine_args, refine_channels, REFINE_DEFAULTS

F32, F64 = np.float32, np.float64


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- 1: degenerate inputs
@pytest.mark.parametrize("shape", Rf.TINY, ids=lambda s: "{}x{}".format(*s))
def test_all_denominators_zero_returns_the_input_bit_for_bit(shape):
    """alpha = 0 takes the smoothness term away and a far_mask of zeros the data term: every A11 + sigma and A22 + sigma is
    0, nothing moves -- not even the sign of a zero"""
    k = Rf.case(2, shape, 1, 0, 2)
    f = k['f'].copy()
    f[0, 0, 0] = (-0.0, 0.0)
    got = Rf.restate(k['near'], k['far'], f, k['fm'], 1, far_mask=np.zeros(shape, np.uint8), alpha=0)
    assert not got['data'].any() and got['dom'].all()
    assert np.array_equal(bits(got['vecs']), bits(f))


@pytest.mark.parametrize("shape", Rf.TINY, ids=lambda s: "{}x{}".format(*s))
def test_degenerate_shapes_run_at_the_defaults(shape):
    want = Rf.case(2, shape, -1, 1, 3)['want']
    assert np.isfinite(want['vecs']).all() and want['vecs'].shape == (1,) + shape + (2,)
    if shape == (1, 1):                                  # no neighbour: gx = gy = 0 and sigma = 0
        assert np.array_equal(bits(want['vecs']), bits(Rf.case(2, shape, -1, 1, 3)['f']))


def test_valid_all_zero_returns_the_field_bit_for_bit():
    k = Rf.case(3, (19, 70), 1, 0, 3)
    f = k['f'].copy()
    f[0, 4, 5], f[0, 9, 60] = (np.nan, 1.0), (-0.0, np.inf)
    got = Rf.restate(k['near'], k['far'], f, k['fm'], 1, valid=np.zeros((19, 70), np.uint8))
    assert not got['dom'].any() and not got['data'].any()
    assert np.array_equal(bits(got['vecs']), bits(f))


def test_outside_the_domain_nothing_changes_and_inside_it_does():
    k = Rf.case(3, (37, 131), -1, 1, 3, masked=True)
    want = k['want']
    dom = k['fm'] & k['valid'].astype(bool)
    assert np.array_equal(want['dom'], dom) and 0.5 < dom.mean() < 0.95
    same = (bits(want['vecs']) == bits(k['f'])).all(axis=-1)
    assert same[~dom].all() and not same[dom].all()
    # the island of holes(): a domain pixel without a neighbour in the domain moves by its data term alone
    y, x = 37 - 4, 131 - 5
    assert dom[0, y, x] and not (dom[0, y - 1, x] | dom[0, y + 1, x] | dom[0, y, x - 1] | dom[0, y, x + 1])


def test_a_nan_vector_leaves_every_other_pixel_finite():
    k = Rf.case(4, (19, 70), 1, 0, 3)
    f = k['f'].copy()
    f[0, 8, 40] = (np.nan, 0.5)
    f[0, 3, 3] = (1.0, -np.inf)
    got = Rf.restate(k['near'], k['far'], f, k['fm'], 1)
    bad = np.zeros((1, 19, 70), bool)
    bad[0, 8, 40] = bad[0, 3, 3] = True
    assert np.isfinite(got['vecs'][~bad]).all() and not got['dom'][bad].any()
    assert np.array_equal(bits(got['vecs'][bad]), bits(f[bad]))


def test_a_nan_image_pixel_leaves_every_other_pixel_finite():
    k = Rf.case(4, (19, 70), 1, 0, 3)
    near, far = k['near'].copy(), k['far'].copy()
    near[0, 1, 9, 30], far[0, 2, 5, 50], far[0, 0, 12, 20] = np.nan, np.nan, np.inf
    got = Rf.restate(near, far, k['f'], k['fm'], 1)
    assert np.isfinite(got['vecs']).all()
    assert not got['data'][0, 9, 30] and got['data'].sum() < k['want']['data'].sum()
    assert (bits(got['vecs']) != bits(k['f'])).any()


# ---------------------------------------------------------------------------------------------- 2: it refines
INITIAL_EPE = 0.7211


@pytest.fixture(scope="module")
def refined():
    """the zero field refined four times on the shifted pair, re-warping by calling again: [(float32 result, float64 result
    of the same call)]"""
    near, far = Rf.shifted_pair()
    f, fm, out = np.zeros((48, 80, 2), F32), np.ones((48, 80), bool), []
    for _ in range(4):
        r32 = Rf.restate(near, far, f, fm, 1)
        r64 = Rf.restate(near, far, f, fm, 1, dt=F64)
        out.append((r32['vecs'], r64['vecs']))
        f = r32['vecs'][0]
    return out


def test_it_refines(refined):
    """the float64 prototype, which sampled `far` analytically, gave 0.269, 0.043, 0.006, 0.0008; with the library's bilinear
    taps (1 / 32 px under QUANT_OPENCV) the restatement gives 0.2674, 0.0708, 0.0364, 0.0274"""
    assert abs(Rf.epe(np.zeros((1, 48, 80, 2), F32)) - INITIAL_EPE) < 1e-4
    errors = [Rf.epe(r32) for r32, _ in refined]
    print("mean end-point error after 1 ... 4 calls:", errors)
    assert errors[0] < 0.5 * INITIAL_EPE
    assert errors[2] < 0.1 * INITIAL_EPE


# ---------------------------------------------------------------------------------------------- 3: float32 against float64
def test_float32_stays_close_to_float64(refined):
    measured = {"call {}".format(i + 1): float(np.abs(r32.astype(F64) - r64).max()) for i, (r32, r64) in enumerate(refined[:3])}
    k = Rf.case(1, (37, 131), 1, 0, 3)
    r64 = Rf.restate(k['near'], k['far'], k['f'], k['fm'], 1, dt=F64)
    measured["(37, 131) with holes"] = float(np.abs(k['want']['vecs'].astype(F64) - r64['vecs']).max())
    print("max |out32 - out64| in px:", measured)
    assert Rf.BOUND_32_64 == 8 * Rf.MEASURED_32_64
    assert max(measured.values()) <= Rf.BOUND_32_64, measured


# ---------------------------------------------------------------------------------------------- 4: refine_args
def test_refine_args_defaults_and_values():
    alpha, delta, zeta, eps, fixed_point, sor, omega = refine_args()
    assert (alpha, delta, zeta, eps, fixed_point, sor, omega) == (F32(20), F32(5), F32(0.1), F32(0.1), 5, 5, F32(1.6))
    assert all(type(v) is F32 for v in (alpha, delta, zeta, eps, omega)) and type(fixed_point) is int and type(sor) is int
    assert REFINE_DEFAULTS == Rf.DEFAULTS
    assert refine_args(0, 0, 1, np.float64(0.001), np.int64(1), 32, 1)[:] == (F32(0), F32(0), F32(1), F32(0.001), 1, 32, F32(1))
    assert [refine_channels(c) for c in (1, 2, 3, 4)] == [1, 2, 3, 4]
    assert Rf.settings() == dict(zip(("alpha", "delta", "zeta", "eps", "fixed_point", "sor", "omega"), refine_args()))


@pytest.mark.parametrize("kw, exc, text", [
    (dict(alpha=-1), ValueError, "alpha must be finite and not negative, got -1"),
    (dict(alpha=float('nan')), ValueError, "alpha must be finite and not negative"),
    (dict(alpha=1e39), ValueError, "alpha must be finite and not negative"),
    (dict(alpha='20'), TypeError, "alpha must be a number or None, got str"),
    (dict(delta=-0.5), ValueError, "delta must be finite and not negative, got -0.5"),
    (dict(delta=float('inf')), ValueError, "delta must be finite and not negative"),
    (dict(delta=True), TypeError, "delta must be a number or None, got bool"),
    (dict(zeta=0), ValueError, "zeta must be finite and positive (its float32 square too), got 0"),
    (dict(zeta=-0.1), ValueError, "zeta must be finite and positive"),
    (dict(zeta=1e-30), ValueError, "zeta must be finite and positive"),
    (dict(zeta=float('nan')), ValueError, "zeta must be finite and positive"),
    (dict(eps=0.0), ValueError, "eps must be finite and positive (its float32 square too), got 0.0"),
    (dict(eps=float('inf')), ValueError, "eps must be finite and positive"),
    (dict(eps=[0.1]), TypeError, "eps must be a number or None, got list"),
    (dict(fixed_point=0), ValueError, "fixed_point must be in [1, 32], got 0"),
    (dict(fixed_point=33), ValueError, "fixed_point must be in [1, 32], got 33"),
    (dict(fixed_point=2.0), TypeError, "fixed_point must be an integer or None, got float"),
    (dict(sor=0), ValueError, "sor must be in [1, 32], got 0"),
    (dict(sor=100), ValueError, "sor must be in [1, 32], got 100"),
    (dict(sor=True), TypeError, "sor must be an integer or None, got bool"),
    (dict(omega=0), ValueError, "omega must lie in (0, 2), got 0"),
    (dict(omega=2), ValueError, "omega must lie in (0, 2), got 2"),
    (dict(omega=-1.6), ValueError, "omega must lie in (0, 2)"),
    (dict(omega=float('nan')), ValueError, "omega must lie in (0, 2)"),
    (dict(omega='sor'), TypeError, "omega must be a number or None, got str"),
])
def test_refine_args_rejects(kw, exc, text):
    with pytest.raises(exc) as e:
        refine_args(**kw)
    assert str(e.value).startswith("Error refining flow: ") and text in str(e.value)


@pytest.mark.parametrize("c", [0, 5, 128])
def test_more_than_four_channels_are_refused_by_name(c):
    with pytest.raises(ValueError) as e:
        refine_channels(c)
    assert str(e.value) == "Error refining flow: the tensors need 1 to 4 channels (grey, two-plane, RGB, RGBA), got {}".format(c)


# ---------------------------------------------------------------------------------------------- 5: the entries
def test_the_host_forms_validate_before_any_device_work():
    f = of.Flow.zero((4, 6), 't')
    img = np.zeros((4, 6, 3), np.uint8)
    with pytest.raises(ValueError, match="omega must lie in"):
        f.refine(img, img, omega=2.5)
    with pytest.raises(ValueError, match="1 to 4 channels"):
        f.refine(np.zeros((4, 6, 5), F32), np.zeros((4, 6, 5), F32))
    with pytest.raises(ValueError, match="Error refining flow: the arrays need the same shape"):
        f.refine(img, np.zeros((4, 6, 4), np.uint8))
    with pytest.raises(TypeError, match="Error refining flow: the arrays need the same dtype"):
        f.refine(img.astype(np.float16), img.astype(F32))
    with pytest.raises(ValueError, match="Error refining flow: arrays and flow need the same height and width"):
        f.refine(np.zeros((4, 7, 3), F32), np.zeros((4, 7, 3), F32))
    with pytest.raises(ValueError, match="Error refining flow: one flow takes one item, got 2"):
        f.refine(np.zeros((2, 4, 6, 3), F32), np.zeros((2, 4, 6, 3), F32))
    with pytest.raises(ValueError, match="Error refining flow: valid needs to have the shape of the flow"):
        f.refine(img, img, valid=np.ones((4, 5), bool))
    with pytest.raises(ValueError, match="Error refining flow: layout must be"):
        of.refine_flow(np.zeros((4, 6, 2), F32), img, img, 't', layout='nhwc')
    if nat.device_count() == 0:
        with pytest.raises(nat.NoDeviceError):
            f.refine(img, img)
        with pytest.raises(nat.NoDeviceError):
            of.refine_flow(np.zeros((4, 6, 2), F32), img, img, 't', alpha=10, sor=3)
        lib = nat.load()
        assert lib.ofl_refine_dev(None, None, nat.EL_F32, nat.TENSOR_NCHW, 1, 3, 4, 6, None, None, 1, None, None, None, F32(20), F32(5),
                                  F32(0.1), F32(0.1), 5, 5, F32(1.6), None, 0, None, None, nat.QUANT_OPENCV, None) == nat.E_NODEVICE
        assert lib.ofl_refine(None, None, nat.EL_F32, nat.TENSOR_NCHW, 1, 3, 4, 6, None, None, 1, None, None, None, F32(20), F32(5),
                              F32(0.1), F32(0.1), 5, 5, F32(1.6), None, None, nat.QUANT_OPENCV) == nat.E_NODEVICE


def test_the_workspace_is_29_bytes_a_pixel():
    import ctypes
    lib, n = nat.load(), ctypes.c_size_t(0)
    assert lib.ofl_refine_workspace_bytes(3, 37, 131, ctypes.byref(n)) == nat.OK and n.value == 29 * 3 * 37 * 131
    assert lib.ofl_refine_workspace_bytes(16, 2160, 3840, ctypes.byref(n)) == nat.OK and n.value == 29 * 16 * 2160 * 3840 > 2 ** 31
    for bad in ((0, 4, 6), (65536, 4, 6), (1, 0, 6), (1, 4, 32767)):
        assert lib.ofl_refine_workspace_bytes(*bad, ctypes.byref(n)) == nat.E_INVALID and "ofl_refine_workspace_bytes" in nat.last_error()
    assert lib.ofl_refine_workspace_bytes(1, 4, 6, None) == nat.E_INVALID
