"""Flow.visualise / visualise_flow on the host side: argument checks that run before any device work, the exported name,
no CPU fallback, the scale's order statistics, and the NumPy restatement (visualise_ref) against the colours and the
mask-border rule the reference documents.  No GPU needed."""
import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import _native as nat
from oflibnumpy_amd import device as dev
import visualise_ref as R


def uniform(h, w, deg, r=3.0):
    a = np.deg2rad(deg)
    v = np.empty((h, w, 2), np.float32)
    v[..., 0], v[..., 1] = np.float32(r * np.cos(a)), np.float32(r * np.sin(a))
    return v


VECS = uniform(6, 8, 30)


@pytest.mark.parametrize("kwargs, exc", [
    (dict(mode=3), ValueError),
    (dict(mode='RGB'), ValueError),
    (dict(mode=None), ValueError),
    (dict(mode='rgb', show_mask=1), TypeError),
    (dict(mode='rgb', show_mask='yes'), TypeError),
    (dict(mode='hsv', show_mask_borders=0), TypeError),
    (dict(mode='bgr', range_max=np.float32(2)), TypeError),
    (dict(mode='bgr', range_max='2'), TypeError),
    (dict(mode='bgr', range_max=[2]), TypeError),
    (dict(mode='rgb', range_max=0), ValueError),
    (dict(mode='rgb', range_max=-1.5), ValueError),
    (dict(mode='rgb', range_max=False), ValueError),
    (dict(mode='rgb', range_max=float('inf')), ValueError),
    (dict(mode='rgb', range_max=float('nan')), ValueError),
])
def test_argument_errors_before_any_device_work(kwargs, exc):
    # without a GPU a check that came too late would surface as NoDeviceError instead
    with pytest.raises(exc):
        of.Flow(VECS).visualise(**kwargs)
    with pytest.raises(exc):
        dev.visualise_args(kwargs.pop('mode'), **kwargs)


def test_visualise_flow_argument_errors():
    with pytest.raises(ValueError):
        of.visualise_flow(VECS, 'rbg')
    with pytest.raises(TypeError):
        of.visualise_flow(VECS, 'rgb', range_max=np.float32(1))
    with pytest.raises(ValueError):
        of.visualise_flow(VECS, 'rgb', range_max=-2)


def test_accepted_range_types():
    assert dev.visualise_args('rgb', range_max=True) == (nat.VIS_RGB, 0, np.float32(1))
    assert dev.visualise_args('bgr', True, False, 7) == (nat.VIS_BGR, nat.VIS_SHOW_MASK, np.float32(7))
    assert dev.visualise_args('hsv', False, True, np.float64(2.5)) == (nat.VIS_HSV, nat.VIS_MASK_BORDERS, np.float32(2.5))
    assert dev.visualise_args('hsv', True, True)[1:] == (nat.VIS_SHOW_MASK | nat.VIS_MASK_BORDERS, None)
    assert dev.visualise_args('rgb', range_max=1e-30)[2] == np.float32(1e-30)
    assert dev.visualise_args('rgb', range_max=1e39)[2] == np.float32(np.inf)        # what NumPy divides by
    assert dev.visualise_args('rgb', range_max=10 ** 400)[2] == np.float32(np.inf)


def test_visualise_flow_is_exported():
    assert 'visualise_flow' in of.flow_operations.__all__
    assert of.visualise_flow is of.flow_operations.visualise_flow
    assert callable(of.Flow.visualise) and callable(of.DeviceFlow.visualise) and callable(of.DeviceFlowBatch.visualise)
    for name in ('visualise_arrows', 'show', 'show_arrows'):
        assert not hasattr(of.Flow, name), name        # drawing / GUI: out of scope


def test_no_cpu_fallback_for_visualise():
    if nat.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(nat.NoDeviceError):
        of.Flow(VECS).visualise('rgb')
    with pytest.raises(nat.NoDeviceError):
        of.visualise_flow(VECS, 'hsv', range_max=2)


@pytest.mark.parametrize("n", [1, 2, 3, 100, 101, 999, 1000, 1001, 4097, 12345, 1080 * 1920])
def test_percentile_ranks_reproduce_numpy(n):
    a = np.random.default_rng(n).random(n, dtype=np.float32)
    lo, hi, gamma = dev.percentile_ranks(n)
    assert 0 <= lo <= hi < n and isinstance(gamma, np.float32)
    s = np.sort(a)
    d = s[hi] - s[lo]
    got = s[hi] - d * (np.float32(1) - gamma) if gamma >= 0.5 else s[lo] + d * gamma
    assert got == np.percentile(a, 99)


def test_percentile_ranks_large_fields():
    # NumPy's float32 virtual index: gamma is 0 at 4K; past 2**24 pixels n - 1 itself rounds
    assert dev.percentile_ranks(3840 * 2160) == (8211455, 8211456, np.float32(0))
    lo, hi, gamma = dev.percentile_ranks(7680 * 4320)
    assert hi == lo + 1 and lo == int(np.floor(np.float32(7680 * 4320 - 1) * np.float32(0.99)))


def test_reference_colours():
    red = R.visualise(uniform(4, 5, 0), 'hsv')
    assert (red == (0, 255, 255)).all()
    assert (R.visualise(uniform(4, 5, 0), 'rgb') == (255, 0, 0)).all()
    assert (R.visualise(uniform(4, 5, 0), 'bgr') == (0, 0, 255)).all()
    assert (R.visualise(uniform(4, 5, 120), 'hsv')[..., 0] == 60).all()
    assert (R.visualise(uniform(4, 5, 120), 'rgb') == (0, 255, 0)).all()
    assert (R.visualise(uniform(4, 5, 240), 'hsv')[..., 0] == 120).all()
    assert (R.visualise(uniform(4, 5, 240), 'rgb') == (0, 0, 255)).all()
    assert (R.visualise(uniform(4, 5, 240), 'bgr') == (255, 0, 0)).all()


def test_reference_mask_dimming_and_border():
    v = uniform(6, 7, 0)
    mask = np.ones((6, 7), bool)
    mask[:, 4:] = False
    dim = R.visualise(v, 'hsv', mask, show_mask=True)
    assert (dim[~mask][:, 2] == 180).all() and (dim[mask][:, 2] == 255).all()
    both = R.visualise(v, 'hsv', mask, show_mask=True, show_mask_borders=True)
    assert (both[0, 0] == 0).all() and (both[2, 3] == 0).all()        # frame pixel, pixel next to the invalid area
    assert (both[2, 2] == (0, 255, 255)).all()
    assert (R.visualise(v, 'rgb', mask, show_mask_borders=True)[2, 3] == 0).all()


def _rows(*rows):
    return np.array([[c == '#' for c in r] for r in rows])


@pytest.mark.parametrize("mask, border", [
    (_rows("........",       # ring
           ".######.",
           ".######.",
           ".##..##.",
           ".##..##.",
           ".######.",
           ".######.",
           "........"),
     _rows("........",
           ".######.",
           ".#.##.#.",
           ".##..##.",
           ".##..##.",
           ".#.##.#.",
           ".######.",
           "........")),
    (_rows(".......",        # filled rectangle: its inside is not border
           ".#####.",
           ".#####.",
           ".#####.",
           "......."),
     _rows(".......",
           ".#####.",
           ".#...#.",
           ".#####.",
           ".......")),
    (_rows("#####",          # hole: its 4-neighbours and the frame
           "#####",
           "##.##",
           "#####",
           "#####"),
     _rows("#####",
           "#.#.#",
           "##.##",
           "#.#.#",
           "#####")),
    (_rows(".....",          # single pixel
           "..#..",
           "....."),
     _rows(".....",
           "..#..",
           ".....")),
    (_rows("......",         # one-pixel line
           ".####.",
           "......"),
     _rows("......",
           ".####.",
           "......")),
    (_rows("###...",         # region touching the frame
           "###...",
           "###...",
           "......"),
     _rows("###...",
           "#.#...",
           "###...",
           "......")),
])
def test_border_rule(mask, border):
    assert np.array_equal(R.border_pixels(mask), border)
    v = uniform(*mask.shape, 45)
    img = R.visualise(v, 'hsv', mask, show_mask_borders=True)
    assert (img[border] == 0).all()
    assert (img[~border][:, 2] == 255).all()


def test_rgb_conversion_is_float64():
    # h * 6 is float32, the rest float64: the sector value must come from the float64 fraction
    hsv = np.array([[[59.5, 200.0, 255.0], [179.99998, 255.0, 180.0], [0.0, 0.0, 0.0]]], np.float32)
    h = hsv[..., 0] / 180
    assert (h * 6.).dtype == np.float32 and (h * 6. - (h * 6.).astype(np.int64)).dtype == np.float64
    rgb = R.hsv_to_rgb_bytes(hsv)
    assert rgb.dtype == np.uint8 and (rgb[0, 2] == 0).all()
