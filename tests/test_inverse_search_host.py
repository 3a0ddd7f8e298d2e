"""K24 without a GPU: the NumPy restatement (tests/inverse_search_ref.py) on the known translations, float32 against float64,
the consequences of the definition (flat and NaN-ridden patches, the reach of a patch, the clamp, masked-out inits), the
patch grid, args.inverse_search_args / estimate_levels, and the entries without a device."""
import ctypes

import numpy as np
import pytest

import oflibnumpy_amd as of
import inverse_search_ref as I
from oflibnumpy_amd import _native as nat
from oflibnumpy_amd.args import inverse_search_args, inverse_search_channels, patch_origins, estimate_levels

F32, F64 = np.float32, np.float64
bits = I.bits


# ---------------------------------------------------------------------------------------------- 1: it finds the field
@pytest.mark.parametrize("i", range(len(I.KNOWN)))
def test_known_translations_from_the_zero_field(i):
    """the restatement in float32, exact taps, no refinement: below a tenth of the zero field's error (the float64 prototype
    reached 0.018, 0.048 and 0.003 of it).  Reached here: 0.07723 (0.0184 x), 0.03427 (0.0475 x), 0.01943 (0.0030 x)"""
    shape, v, levels, border, zero = I.KNOWN[i]
    got = I.known(i)
    assert abs(I.epe(np.zeros(shape + (2,)), v, border) - zero) < 1e-4
    print("known answer", i, "epe", got['epe'], "of", zero)
    assert got['epe'] < 0.1 * zero and got['mask'].all()


@pytest.mark.parametrize("i", range(len(I.KNOWN)))
def test_float32_stays_next_to_float64(i):
    """the same statement in float64 on the same float32 planes: no patch stops at another iterate (none is excluded), and
    the densified fields differ by less than 8 x the largest difference measured (inverse_search_ref.MEASURED_32_64)"""
    diff, stopped, other_best = I.compare_32_64(i)
    print("float32 - float64", i, diff, "recorded", I.MEASURED_32_64[i], "stopped elsewhere", stopped, "other best iterate", other_best)
    assert stopped == 0
    assert diff <= I.BOUND_32_64 and I.BOUND_32_64 == 8 * 4.1665197937401643e-04
    assert abs(I.known(i, F64)['epe'] - I.known(i)['epe']) < I.BOUND_32_64


def test_the_numpy_sampler_is_the_oracles_gather_bit_for_bit():
    """sample_numpy (what the float64 run samples with) in float32 against the oracle's gather, on vectors that leave the
    frame on every side"""
    k = I.case(1, (19, 70), 1, 1, 1)
    plane = np.ascontiguousarray(k['far'][0, 0])
    oys, oxs = I.origins(19, 8, 3), I.origins(70, 8, 3)
    rng = np.random.default_rng(5)
    U = (rng.standard_normal((len(oys), len(oxs), 2)) * 6).astype(F32)
    U[0, 0], U[-1, -1], U[1, 1] = (-1000, -1000), (1000, 1000), (0.0, 0.0)
    for sign in (1, -1):
        a, b = I.sample_oracle(plane, U, oys, oxs, 8, sign, 1), I.sample_numpy(plane, U, oys, oxs, 8, sign, F32)
        assert np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------- 2: consequences
@pytest.mark.parametrize("patch, stride", [(8, 4), (4, 3)])
def test_a_constant_image_returns_the_init_bit_for_bit(patch, stride):
    shape = (19, 70)
    k = I.case(2, shape, 1, 1, 1)
    flat = np.full((1, 1) + shape, 93.5, F32)
    f = k['f'].copy()
    f[0, 4, 4] = (-0.0, 0.0)
    got = I.restate(flat, flat, f, k['fm'], 1, patch=patch, stride=stride)
    assert np.array_equal(bits(got['patch_vecs']), bits(got['u0'])) and (got['steps'] == 0).all()
    assert (got['patch_ssd'] < 1e-6).all() and got['mask'].all()         # the four weights of a tap need not add up to exactly 1
    # every patch votes with the same weight 1 / floor: a pixel covered by ONE patch returns that patch's u0
    assert np.array_equal(bits(got['vecs'][0, 0, 0]), bits(np.where(got['u0'][0, 0, 0] == 0, F32(0), got['u0'][0, 0, 0])))


@pytest.mark.parametrize("sign", I.SIGNS)
def test_no_patch_moves_farther_than_its_size(sign):
    for patch, stride, shape in ((8, 4, (37, 131)), (4, 2, (19, 70))):
        want = I.case(3, shape, sign, 1, 3, params=(('patch', patch), ('stride', stride)))['want']
        d = want['patch_vecs'].astype(F64) - want['u0']
        assert ((d * d).sum(axis=-1) <= patch * patch).all()
        assert (want['kbest'] > 0).mean() > 0.5 and np.isfinite(want['patch_ssd']).all()


def test_an_init_far_outside_the_frame_takes_the_clamp_path_without_a_nan():
    shape = (19, 70)
    k = I.case(4, shape, 1, 1, 2)
    f = np.full((1,) + shape + (2,), 1000.0, F32)
    f[0, :, 35:] = (-1000.0, 1000.0)
    got = I.restate(k['near'], k['far'], f, None, 1)
    assert np.isfinite(got['vecs']).all() and np.isfinite(got['patch_vecs']).all() and got['mask'].all()
    assert np.isfinite(got['patch_ssd']).all()
    d = got['patch_vecs'].astype(F64) - got['u0']
    assert ((d * d).sum(axis=-1) <= 64).all() and (got['vecs'][..., 1] > 900).all()      # x mixes +1000 and -1000 at the seam


def test_a_nan_in_near_spoils_only_the_patches_that_contain_it():
    shape, patch, stride = (37, 131), 8, 4
    k = I.case(5, shape, 1, 1, 3)
    near = k['near'].copy()
    y, x = 17, 66
    near[0, 1, y, x] = np.nan
    got, clean = I.restate(near, k['far'], k['f'], k['fm'], 1), k['want']
    oys, oxs = np.array(I.origins(shape[0], patch, stride)), np.array(I.origins(shape[1], patch, stride))
    # A(y, x) is NaN: it enters T, r and the sums of a patch that contains it, and gx / gy of a patch that contains a neighbour
    hit_y, hit_x = (oys <= y + 1) & (y - 1 < oys + patch), (oxs <= x + 1) & (x - 1 < oxs + patch)
    hit = hit_y[:, None] & hit_x[None, :]
    has = ((oys <= y) & (y < oys + patch))[:, None] & ((oxs <= x) & (x < oxs + patch))[None, :]
    assert np.array_equal(bits(got['patch_vecs'][0][has]), bits(got['u0'][0][has])) and np.isinf(got['patch_ssd'][0][has]).all()
    assert np.array_equal(bits(got['patch_vecs'][0][~hit]), bits(clean['patch_vecs'][0][~hit]))
    # the densified field: only the pixel itself has a NaN weight; pixels under no touched patch keep their bits
    assert not got['mask'][0, y, x] and got['mask'].sum() == got['mask'].size - 1
    assert np.array_equal(bits(got['vecs'][0, y, x]), bits(np.zeros(2, F32)))
    under = np.zeros(shape, bool)
    for iy, ix in zip(*np.nonzero(hit)):
        under[oys[iy]:oys[iy] + patch, oxs[ix]:oxs[ix] + patch] = True
    assert np.array_equal(bits(got['vecs'][0][~under]), bits(clean['vecs'][0][~under])) and (~under).mean() > 0.8


def test_a_masked_out_or_non_finite_init_vector_reads_as_zero():
    shape = (19, 70)
    k = I.case(6, shape, -1, 1, 1)
    f, fm = k['f'].copy(), k['fm'].copy()
    oys, oxs = I.origins(19, 8, 4), I.origins(70, 8, 4)
    f[0, oys[0] + 4, oxs[1] + 4] = (np.nan, 1.0)
    f[0, oys[1] + 4, oxs[2] + 4] = (2.0, -np.inf)
    fm[0, oys[2] + 4, oxs[3] + 4] = False
    got = I.restate(k['near'], k['far'], f, fm, -1)
    for iy, ix in ((0, 1), (1, 2), (2, 3)):
        assert np.array_equal(bits(got['u0'][0, iy, ix]), bits(np.zeros(2, F32)))
    assert np.isfinite(got['vecs']).all() and got['mask'].all()
    none = I.restate(k['near'], k['far'], None, None, -1)
    zero = I.restate(k['near'], k['far'], np.zeros_like(f), np.ones_like(fm), -1)
    assert np.array_equal(bits(none['vecs']), bits(zero['vecs']))


# ---------------------------------------------------------------------------------------------- 3: the patch grid
@pytest.mark.parametrize("patch", [4, 8])
def test_the_patch_grid_covers_every_pixel_and_ends_at_the_border(patch):
    for n in (patch, patch + 1, 2 * patch - 1, 21):
        for stride in (1, 3, patch):
            org = patch_origins(n, patch, stride)
            assert org == I.origins(n, patch, stride)
            assert org[0] == 0 and org[-1] == n - patch and org == sorted(set(org))
            assert all(b - a <= stride for a, b in zip(org, org[1:]))
            covered = np.zeros(n, int)
            for o in org:
                covered[o:o + patch] += 1
            assert (covered >= 1).all() and covered.max() <= -(-patch // stride) + 1
            # K24's closed form: origin(i) = min(i * stride, n - patch)
            assert org == [min(i * stride, n - patch) for i in range(len(org))]
            groups = I.patch_groups(org, patch)
            assert sorted(int(i) for g in groups for i in g) == list(range(len(org)))
    with pytest.raises(ValueError, match="holds no patch"):
        patch_origins(patch - 1, patch, 1)


# ---------------------------------------------------------------------------------------------- 4: arguments
def test_inverse_search_args_defaults():
    assert inverse_search_args() == (8, 4, 12, True, F32(1.0)) and type(inverse_search_args()[4]) is F32
    assert inverse_search_args(4, 4, 32, False, 0.5) == (4, 4, 32, False, F32(0.5))
    assert dict(zip(("patch", "stride", "iterations", "normalise", "floor"), inverse_search_args())) == I.DEFAULTS


@pytest.mark.parametrize("kw, exc, text", [
    (dict(patch=6), ValueError, "patch must be 4 or 8, got 6"),
    (dict(patch=16), ValueError, "patch must be 4 or 8, got 16"),
    (dict(patch=8.0), TypeError, "patch must be an integer, got float"),
    (dict(patch=True), TypeError, "patch must be an integer, got bool"),
    (dict(stride=0), ValueError, "stride must be in [1, patch = 8], got 0"),
    (dict(stride=9), ValueError, "stride must be in [1, patch = 8], got 9"),
    (dict(patch=4, stride=5), ValueError, "stride must be in [1, patch = 4], got 5"),
    (dict(stride='4'), TypeError, "stride must be an integer, got str"),
    (dict(iterations=0), ValueError, "iterations must be in [1, 32], got 0"),
    (dict(iterations=33), ValueError, "iterations must be in [1, 32], got 33"),
    (dict(iterations=None), TypeError, "iterations must be an integer, got NoneType"),
    (dict(normalise=1), TypeError, "normalise must be a bool, got int"),
    (dict(floor=0), ValueError, "floor must be finite and positive"),
    (dict(floor=-1.0), ValueError, "floor must be finite and positive"),
    (dict(floor=float('nan')), ValueError, "floor must be finite and positive"),
    (dict(floor=float('inf')), ValueError, "floor must be finite and positive"),
    (dict(floor=1e-60), ValueError, "floor must be finite and positive"),
    (dict(floor=1e39), ValueError, "floor must be finite and positive"),
    (dict(floor=True), TypeError, "floor must be a number, got bool"),
    (dict(floor=[1.0]), TypeError, "floor must be a number, got list"),
])
def test_inverse_search_args_rejects(kw, exc, text):
    with pytest.raises(exc) as e:
        inverse_search_args(**kw)
    assert str(e.value).startswith("Error searching flow: ") and text in str(e.value)


@pytest.mark.parametrize("c", [0, 5, 128])
def test_more_than_four_channels_are_refused_by_name(c):
    with pytest.raises(ValueError) as e:
        inverse_search_channels(c)
    assert str(e.value) == "Error searching flow: the tensors need 1 to 4 channels (grey, two-plane, RGB, RGBA), got {}".format(c)


def test_the_size_rule_of_estimate_flow():
    assert estimate_levels((128, 192)) == 4                     # 16 x 24 at the coarsest level; 8 x 12 would be too small
    assert estimate_levels((128, 192), patch=4) == 5
    assert estimate_levels((2160, 3840)) == 5                   # 2160 = 2^4 * 135
    assert estimate_levels((1080, 1920)) == 4
    assert estimate_levels((4096, 4096)) == 6
    assert estimate_levels((17, 16)) == 1 and estimate_levels((100, 192)) == 3
    assert estimate_levels((128, 192), 2) == 2 and estimate_levels((128, 192), 1) == 1
    for shape, levels in (((100, 192), 4), ((128, 192), 5), ((64, 96), 4), ((130, 192), 3)):
        with pytest.raises(ValueError, match="Error estimating flow: .*pad"):
            estimate_levels(shape, levels)
    with pytest.raises(ValueError, match="Error estimating flow: .*pad"):
        estimate_levels((15, 200))
    with pytest.raises(ValueError, match=r"levels must be in \[1, 6\], got 7"):
        estimate_levels((4096, 4096), 7)
    with pytest.raises(ValueError, match=r"levels must be in \[1, 6\], got 0"):
        estimate_levels((128, 192), 0)
    with pytest.raises(TypeError, match="levels must be an integer or None, got float"):
        estimate_levels((128, 192), 2.0)


# ---------------------------------------------------------------------------------------------- 5: halve and the entries
def test_halve_drops_an_odd_row_and_column_and_rounds_once():
    a = np.arange(2 * 5 * 7, dtype=F32).reshape(2, 5, 7)
    h = I.halve(a)
    assert h.shape == (2, 2, 3) and h[0, 0, 0] == (0 + 1 + 7 + 8) / 4 and h[1, 1, 2] == (53 + 54 + 60 + 61) / 4
    half = I.halve(np.array([[[1.0, 1.001], [1.002, 1.003]]], np.float16), 'float16')
    assert half.dtype == np.float16 and half.shape == (1, 1, 1)


def test_the_host_forms_validate_before_any_device_work():
    f = of.Flow.zero((16, 24), 't')
    img = np.zeros((16, 24, 3), np.uint8)
    with pytest.raises(ValueError, match="Error searching flow: patch must be 4 or 8"):
        f.inverse_search(img, img, patch=5)
    with pytest.raises(ValueError, match="1 to 4 channels"):
        f.inverse_search(np.zeros((16, 24, 5), F32), np.zeros((16, 24, 5), F32))
    with pytest.raises(ValueError, match="Error searching flow: the arrays need the same shape"):
        f.inverse_search(img, np.zeros((16, 24, 4), np.uint8))
    with pytest.raises(TypeError, match="Error searching flow: the arrays need the same dtype"):
        f.inverse_search(img.astype(np.float16), img.astype(F32))
    with pytest.raises(ValueError, match="Error searching flow: arrays and flow need the same height and width"):
        f.inverse_search(np.zeros((16, 25, 3), F32), np.zeros((16, 25, 3), F32))
    with pytest.raises(ValueError, match="Error searching flow: a 6 x 24 flow holds no patch of 8"):
        of.Flow.zero((6, 24), 't').inverse_search(np.zeros((6, 24), F32), np.zeros((6, 24), F32))
    with pytest.raises(ValueError, match="Error searching flow: layout must be"):
        of.inverse_search_flow(np.zeros((16, 24, 2), F32), img, img, 't', layout='nhwc')
    with pytest.raises(ValueError, match="Error estimating flow: .*pad"):
        of.estimate_flow(np.zeros((100, 192), F32), np.zeros((100, 192), F32), levels=4)
    with pytest.raises(ValueError, match="Error estimating flow: the images need the same shape"):
        of.estimate_flow(np.zeros((32, 32), F32), np.zeros((32, 48), F32))
    with pytest.raises(ValueError, match="Error estimating flow: init needs the shape"):
        of.estimate_flow(np.zeros((32, 32), F32), np.zeros((32, 32), F32), init=np.zeros((16, 16, 2), F32))
    if nat.device_count() == 0:
        with pytest.raises(nat.NoDeviceError):
            f.inverse_search(img, img)
        with pytest.raises(nat.NoDeviceError):
            of.estimate_flow(np.zeros((32, 32), F32), np.zeros((32, 32), F32))
        with pytest.raises(nat.NoDeviceError):
            of.halve_tensor(np.zeros((3, 4, 6), F32))
        lib = nat.load()
        assert lib.ofl_inverse_search_dev(None, None, nat.EL_F32, nat.TENSOR_NCHW, 1, 3, 16, 24, None, None, 1, 8, 4, 12, 1, F32(1),
                                          None, 0, None, None, None, None, nat.QUANT_EXACT, None) == nat.E_NODEVICE
        assert lib.ofl_inverse_search(None, None, nat.EL_F32, nat.TENSOR_NCHW, 1, 3, 16, 24, None, None, 1, 8, 4, 12, 1, F32(1),
                                      None, None, None, None, nat.QUANT_EXACT) == nat.E_NODEVICE
        assert lib.ofl_tensor_halve_dev(None, nat.EL_F32, nat.TENSOR_NCHW, 1, 3, 16, 24, None, None) == nat.E_NODEVICE


def test_the_workspace_is_two_planes_and_twelve_bytes_a_patch():
    lib, n = nat.load(), ctypes.c_size_t(0)
    for (N, h, w, patch, stride) in ((3, 37, 131, 8, 4), (1, 8, 8, 8, 8), (2, 19, 70, 4, 3), (8, 2160, 3840, 8, 4)):
        ny, nx = len(patch_origins(h, patch, stride)), len(patch_origins(w, patch, stride))
        assert lib.ofl_inverse_search_workspace_bytes(N, h, w, patch, stride, ctypes.byref(n)) == nat.OK
        assert n.value == 8 * N * h * w + 12 * N * ny * nx
    for bad in ((0, 16, 16, 8, 4), (65536, 16, 16, 8, 4), (1, 7, 16, 8, 4), (1, 16, 3, 4, 4), (1, 16, 32767, 8, 4), (1, 16, 16, 6, 4),
                (1, 16, 16, 8, 0), (1, 16, 16, 8, 9)):
        assert lib.ofl_inverse_search_workspace_bytes(*bad, ctypes.byref(n)) == nat.E_INVALID
        assert "ofl_inverse_search_workspace_bytes" in nat.last_error()
    assert lib.ofl_inverse_search_workspace_bytes(1, 16, 16, 8, 4, None) == nat.E_INVALID
