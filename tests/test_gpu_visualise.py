"""Flow.visualise on the device (K7, ofl_visualise.hip) against the NumPy restatement of the reference (visualise_ref),
bit for bit: every mode x show_mask x show_mask_borders, the exact 99th-percentile scale from 1 pixel to 8K, given
scales, degenerate shapes, batches, the host wrappers, and fields holding NaN / Inf."""
import itertools

import numpy as np
import pytest

from oflibnumpy_amd import device as dev
from oflibnumpy_amd import _native as nat
from oflibnumpy_amd.batch import DeviceFlowBatch
import visualise_ref as R

pytestmark = pytest.mark.gpu

COMBOS = list(itertools.product(('hsv', 'rgb', 'bgr'), (False, True), (False, True)))


def wobble(h, w, seed=0):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    v = np.empty((h, w, 2), np.float32)
    v[..., 0] = 3 * np.sin(x / 7.0 + seed) + 0.5 * np.cos(y / 3.0)
    v[..., 1] = 2 * np.cos(y / 5.0 - seed) - 0.7 * np.sin(x / 11.0)
    return v


def rotation(h, w, deg=7.0):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    cy, cx, a = (h - 1) / 2.0, (w - 1) / 2.0, np.deg2rad(deg)
    v = np.empty((h, w, 2), np.float32)
    v[..., 0] = (np.cos(a) - 1) * (x - cx) - np.sin(a) * (y - cy)
    v[..., 1] = np.sin(a) * (x - cx) + (np.cos(a) - 1) * (y - cy)
    return v


def axes_and_threshold(h=24, w=36):
    """vectors exactly on the axes and components just below / at / above the 1e-3 threshold"""
    th = np.float32(1e-3)
    vals = np.array([0, th, -th, np.nextafter(th, 0), -np.nextafter(th, 0), np.nextafter(th, 1), -np.nextafter(th, 1),
                     2.5, -2.5, 1e-4, -1e-4, 7.0], np.float32)
    rng = np.random.default_rng(3)
    v = vals[rng.integers(0, len(vals), (h, w, 2))]
    v[0, :4] = [[3, 0], [-3, 0], [0, 3], [0, -3]]
    return v


def random_field(h, w, seed=5):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((h, w, 2)) * 4).astype(np.float32)


def random_mask(h, w, seed=6):
    rng = np.random.default_rng(seed)
    m = rng.random((h, w)) > 0.3
    m[h // 4: h // 2, w // 4: w // 2] = False
    return m


FIELDS = {
    'wobble': lambda: (wobble(40, 64), None),
    'rotation': lambda: (rotation(51, 67), None),
    'axes_threshold': lambda: (axes_and_threshold(), random_mask(24, 36, 1)),
    'random_mask': lambda: (random_field(45, 61), random_mask(45, 61)),
}


def device_image(vecs, mask, mode, sm, smb, range_max=None):
    d = dev.DeviceFlow.from_host(vecs, 't', mask)
    img = d.visualise(mode, sm, smb, range_max)
    assert img.shape == vecs.shape[:2] + (3,) and img.dtype == np.uint8
    return img.to_host()


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_bit_exact_every_mode_and_flag(gpu, name):
    vecs, mask = FIELDS[name]()
    for mode, sm, smb in COMBOS:
        want = R.visualise(vecs, mode, mask, sm, smb)
        got = device_image(vecs, mask, mode, sm, smb)
        assert np.array_equal(got, want), (name, mode, sm, smb, int((got != want).any(-1).sum()))


def _shape_of(n):
    return {1: (1, 1), 2: (1, 2), 101: (1, 101), 1000: (25, 40), 1001: (7, 143)}.get(n)


@pytest.mark.parametrize("n", [1, 2, 101, 1000, 1001, 1080 * 1920, 3840 * 2160, 7680 * 4320])
def test_range_is_numpys_percentile(gpu, n):
    shape = _shape_of(n) or {1080 * 1920: (1080, 1920), 3840 * 2160: (2160, 3840), 7680 * 4320: (4320, 7680)}[n]
    vecs = random_field(*shape, seed=n)
    if n >= 1000:
        vecs[::3] = np.round(vecs[::3] * 8) / 8          # many ties among the magnitudes
    f = R.thresholded(vecs)
    mag = R.magnitude(f[..., 0], f[..., 1])
    want = float(np.percentile(mag, 99))
    got = dev.DeviceFlow.from_host(vecs).visualise_range()
    assert got == want, (n, got, want)
    assert got == R.default_range(mag)


def test_range_fallbacks(gpu):
    zero = np.zeros((30, 50, 2), np.float32)
    zero[3, 4] = [5e-4, -5e-4]                             # below the threshold: still an all-zero field
    assert dev.DeviceFlow.from_host(zero).visualise_range() == 1.0
    sparse = np.zeros((100, 100, 2), np.float32)
    sparse.reshape(-1, 2)[::250] = [[3.0, 4.0]] * 40
    sparse[7, 7] = [0, 9.5]
    assert dev.DeviceFlow.from_host(sparse).visualise_range() == 9.5
    for mode, sm, smb in COMBOS[:4]:
        assert np.array_equal(device_image(zero, None, mode, sm, smb), R.visualise(zero, mode, None, sm, smb))
        assert np.array_equal(device_image(sparse, None, mode, sm, smb), R.visualise(sparse, mode, None, sm, smb))


@pytest.mark.parametrize("range_max", [3, True, 1e-30, 0.75, 1e30, 1e39])
def test_given_range(gpu, range_max):
    vecs, mask = random_field(37, 53), random_mask(37, 53)
    for mode, sm, smb in COMBOS:
        with np.errstate(over='ignore'):
            want = R.visualise(vecs, mode, mask, sm, smb, range_max)
        assert np.array_equal(device_image(vecs, mask, mode, sm, smb, range_max), want), (range_max, mode, sm, smb)


@pytest.mark.parametrize("shape", [(5, 7), (9, 1), (1, 9), (1, 1), (3, 5), (2, 2), (17, 33)])
def test_odd_and_thin_shapes(gpu, shape):
    vecs, mask = wobble(*shape, seed=1), random_mask(*shape, seed=2)
    for mode, sm, smb in COMBOS:
        assert np.array_equal(device_image(vecs, mask, mode, sm, smb), R.visualise(vecs, mode, mask, sm, smb)), (shape, mode, sm, smb)


def test_batch_equals_single_calls(gpu):
    h, w = 33, 47                                        # odd H * W: every other field of the batch starts 8 bytes off
    flows, masks = [], []
    for i in range(16):
        kind = i % 4
        v = [wobble(h, w, i), rotation(h, w, 3 + i), random_field(h, w, i), np.zeros((h, w, 2), np.float32)][kind]
        if i == 7:
            v = v * 1e-4                                  # all below the threshold
        flows.append(v.astype(np.float32))
        masks.append(random_mask(h, w, i) if i % 3 else np.ones((h, w), bool))
    from oflibnumpy_amd.flow_class import Flow
    batch = DeviceFlowBatch.from_flows([Flow(v, 't', m) for v, m in zip(flows, masks)])
    singles = [dev.DeviceFlow.from_host(v, 't', m) for v, m in zip(flows, masks)]
    ranges = batch.visualise_range()
    assert [float(r) for r in ranges] == [s.visualise_range() for s in singles]
    for mode, sm, smb in COMBOS:
        for rm in (None, 2.5):
            got = batch.visualise(mode, sm, smb, rm)
            assert got.shape == (16, h, w, 3)
            got = got.to_host()
            for i, s in enumerate(singles):
                assert np.array_equal(got[i], s.visualise(mode, sm, smb, rm).to_host()), (i, mode, sm, smb, rm)
                assert np.array_equal(got[i], R.visualise(flows[i], mode, masks[i], sm, smb, rm)), (i, mode, sm, smb, rm)
    packed = batch.pack()
    assert np.array_equal(packed.visualise('rgb', True, True).to_host(), batch.visualise('rgb', True, True).to_host())


def test_host_wrappers_match_device(gpu):
    import oflibnumpy_amd as of
    vecs, mask = rotation(48, 80), random_mask(48, 80)
    f = of.Flow(vecs, 't', mask)
    d = f.to_device()
    for mode, sm, smb in COMBOS:
        host = f.visualise(mode, sm, smb)
        assert host.shape == (48, 80, 3) and host.dtype == np.uint8
        assert np.array_equal(host, d.visualise(mode, sm, smb).to_host())
    for mode in ('rgb', 'bgr', 'hsv'):
        want = of.Flow(vecs).visualise(mode)
        assert np.array_equal(of.visualise_flow(vecs, mode), want)
        assert np.array_equal(of.visualise_flow(vecs, mode, range_max=4), of.Flow(vecs).visualise(mode, range_max=4))
        assert np.array_equal(want, R.visualise(vecs, mode))
    assert np.array_equal(f.visualise('rgb', None, None, None), f.visualise('rgb'))


def test_full_size_field(gpu):
    vecs = wobble(1080, 1920, 2)
    vecs[::7, ::5] *= 40                                  # outliers beyond the 99th percentile: S clips at 255
    mask = random_mask(1080, 1920, 9)
    for mode, sm, smb in [('rgb', False, False), ('hsv', True, True), ('bgr', True, False)]:
        assert np.array_equal(device_image(vecs, mask, mode, sm, smb), R.visualise(vecs, mode, mask, sm, smb)), (mode, sm, smb)


def test_nan_and_inf_do_not_fault(gpu):
    vecs = wobble(31, 45)
    vecs[3, 4] = [np.nan, 1.0]
    vecs[5, 6] = [np.inf, -np.inf]
    vecs[7, 8] = [-np.nan, np.nan]
    vecs[9, 10, 1] = np.float32(3e38)
    d = dev.DeviceFlow.from_host(vecs, 't', random_mask(31, 45))
    d.visualise_range()
    for mode, sm, smb in COMBOS:
        assert d.visualise(mode, sm, smb).to_host().shape == (31, 45, 3)
    b = DeviceFlowBatch(3, (31, 45), 't')                 # Flow() refuses non-finite vectors: fill the batch directly
    for i in range(3):
        nat.check(nat.load().ofl_upload(b.vecs.ptr + i * vecs.nbytes, vecs.ctypes.data, vecs.nbytes, None))
    nat.check(nat.load().ofl_memset(b.mask.ptr, 1, 3 * 31 * 45, None))
    assert b.visualise('rgb').to_host().shape == (3, 31, 45, 3)
    clean = wobble(31, 45)                                # the device is still fine afterwards
    assert np.array_equal(device_image(clean, None, 'rgb', False, False), R.visualise(clean, 'rgb'))
