"""CPU suite: the host half of the correlation lookup (K18) -- args.corr_args, the ctypes table, the argument checks of
DeviceCorrelation and correlation_lookup -- and the NumPy restatement tests/correlation_ref.py that test_gpu_correlation.py
compares the kernel with, byte for byte: its distance from the float64 definition against the bound derived in
correlation_ref.py, the pooling of odd sizes, the two channel orders, the summation order on a case whose answer depends on
it, and the float64 definition against RAFT's formulation computed by torch."""
import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import args, _native as nat
import correlation_ref as K

DTYPES = ("float32", "float16", "bfloat16")


# ---------------------------------------------------------------------------------------------- restatement against float64
@pytest.mark.parametrize("r", (1, 2, 3, 4))
def test_restatement_is_within_the_derived_bound_of_float64(r):
    shape, levels = (9, 12), 3
    worst = 0.0
    for c in (3, 64, 131):
        flow = K.fields(shape, r)["random"]
        for k, dtype in enumerate(DTYPES):
            f1, f2 = (K.widen(K.features(shape, c, dtype, seed), dtype) for seed in (k, k + 10))
            sign = 1 if (k + r) % 2 else -1
            got = K.lookup(f1, f2, flow, sign, r, levels).astype(np.float64)
            want = K.lookup64(f1, f2, flow, sign, r, levels)
            unit = K.EPS * float(K.default_scale(c)) * K.magnitude(f1, f2)
            n = K.bound(c, levels)
            err = float(np.abs(got - want).max()) / unit
            worst = max(worst, err / n)
            assert err <= n / (1 - n * K.EPS), (r, c, dtype, err, n)
    print("r = {}: worst error {:.3f} of the bound".format(r, worst))
    assert worst > 0.0


def test_the_bound_counts_the_roundings():
    assert K.bound(256, 4) == 6 + 1 + 15 + 4 + 3 + 4 + 1
    assert K.bound(1, 1) == 1 + 3 + 4 + 3 + 4 + 1
    assert K.bound(257, 1) == 1 + 19 + 4 + 3 + 4 + 1


# ---------------------------------------------------------------------------------------------- pooling, orders, summation order
def test_pooling_of_odd_sizes():
    a = np.arange(5 * 5 * 2, dtype=np.float32).reshape(5, 5, 2)
    p = K.pyramid(a, 3)
    assert [x.shape for x in p] == [(5, 5, 2), (2, 2, 2), (1, 1, 2)]
    assert p[1][1, 1, 0] == (a[2, 2, 0] + a[2, 3, 0] + a[3, 2, 0] + a[3, 3, 0]) / 4          # row and column 4 are dropped
    assert p[2][0, 0, 1] == p[1][..., 1].mean()
    with pytest.raises(AssertionError):
        K.pyramid(a, 4)
    # the order of the three additions: (a + b) + (c + d), not a running sum
    q = np.array([[[1.0], [2.0 ** -24]], [[2.0 ** -24], [2.0 ** -24]]], np.float32)
    assert K.pool(q)[0, 0, 0] == np.float32((np.float32(1.0) + np.float32(2.0 ** -24)) + np.float32(2.0 ** -23)) * np.float32(0.25)
    assert K.pool(q)[0, 0, 0] != np.float32(0.25)


def test_both_orders_are_transposes_of_each_other():
    shape, r, levels = (6, 7), 2, 2
    f1, f2 = (K.widen(K.features(shape, 5, "float32", s), "float32") for s in (0, 1))
    flow = K.fields(shape, r)["random"]
    win = 2 * r + 1
    xy = K.lookup(f1, f2, flow, 1, r, levels, order="xy").reshape(levels, win, win, *shape)
    yx = K.lookup(f1, f2, flow, 1, r, levels, order="yx").reshape(levels, win, win, *shape)
    assert xy.tobytes() == np.ascontiguousarray(yx.transpose(0, 2, 1, 3, 4)).tobytes()
    assert xy.tobytes() != yx.tobytes()


def test_the_summation_order_is_the_stated_one():
    # channels 0 .. 3 (group 0 -> partial sum 0) hold 1, e, e, e with e = 2^-24, channel 4 (group 1 -> partial sum 1) holds -1:
    # p0 = ((1 + e) + e) + e = 1 (each e is lost on its own), p1 = -1, the tree gives 0
    e = np.float32(2.0 ** -24)
    a = np.ones((1, 1, 8), np.float32)
    b2 = np.array([1.0, e, e, e, -1.0, 0, 0, 0], np.float32).reshape(1, 1, 8)
    assert K.dot(a, b2)[0, 0] == 0.0                                     # p0 = 1 (the e are lost one by one), p1 = -1
    assert np.float32(np.float32(1.0) + np.float32(3) * e) - np.float32(1.0) != 0.0        # any order that adds the e first differs
    # a partial sum without a channel adds nothing: -0.0 stays -0.0 for every C
    for c in (1, 3, 4, 5, 63, 64, 65, 131):
        z = K.dot(np.full((1, c), -0.0, np.float32), np.ones((1, c), np.float32))
        assert z.tobytes() == np.float32(-0.0).tobytes(), c
    # 20 channels: ((p0 + p1) + (p2 + p3)) + p4
    x = np.random.default_rng(0).standard_normal((3, 20)).astype(np.float32)
    y = np.random.default_rng(1).standard_normal((3, 20)).astype(np.float32)
    p = [None] * 5
    for g in range(5):
        pr = x[:, 4 * g:4 * g + 4] * y[:, 4 * g:4 * g + 4]
        p[g] = ((pr[:, 0] + pr[:, 1]) + pr[:, 2]) + pr[:, 3]
    assert K.dot(x, y).tobytes() == (((p[0] + p[1]) + (p[2] + p[3])) + p[4]).tobytes()


def test_known_answers_of_the_restatement():
    # one-hot f2: level 0 with an integer field returns scale * f1[x, idx(x + f + o)], exactly 0 outside the frame
    h, w = 3, 4
    c = h * w
    f2 = np.eye(c, dtype=np.float32).reshape(h, w, c)
    f1 = np.random.default_rng(3).standard_normal((h, w, c)).astype(np.float32)
    r, scale = 2, np.float32(0.5)
    flow = np.broadcast_to(np.array([1.0, -1.0], np.float32), (h, w, 2))
    for sign in (1, -1):
        for quant in (K.QUANT_EXACT, K.QUANT_OPENCV):
            got = K.lookup(f1, f2, flow, sign, r, 1, scale, "xy", quant).reshape(5, 5, h, w)
            for y in range(h):
                for x in range(w):
                    for ox in range(-r, r + 1):
                        for oy in range(-r, r + 1):
                            xx, yy = x + sign * 1 + ox, y - sign * 1 + oy
                            want = scale * f1[y, x, yy * w + xx] if 0 <= xx < w and 0 <= yy < h else np.float32(0.0)
                            assert got[ox + r, oy + r, y, x] == want


# ---------------------------------------------------------------------------------------------- RAFT's formulation in torch
def test_float64_definition_equals_rafts_formulation():
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    shape, c, r, levels = (8, 11), 6, 3, 3
    h, w = shape
    f1, f2 = (K.widen(K.features(shape, c, "float32", s), "float32") for s in (4, 5))
    flow = K.fields(shape, r)["random"]
    want = K.lookup64(f1, f2, flow, 1, r, levels, 1.0 / np.sqrt(np.float64(c)), "xy")

    fmap1 = torch.from_numpy(f1.astype(np.float64)).permute(2, 0, 1)[None]          # (1, C, H, W)
    fmap2 = torch.from_numpy(f2.astype(np.float64)).permute(2, 0, 1)[None]
    corr = torch.matmul(fmap1.view(1, c, h * w).transpose(1, 2), fmap2.view(1, c, h * w)).view(1, h, w, 1, h, w)
    corr = corr / torch.sqrt(torch.tensor(c, dtype=torch.float64))
    corr = corr.reshape(h * w, 1, h, w)
    pyramid = [corr]
    for _ in range(levels - 1):
        corr = F.avg_pool2d(corr, 2, stride=2)
        pyramid.append(corr)
    gy, gx = np.mgrid[:h, :w]
    # coords1 = coords0 + flow, as float32 sums (the definition's map_coord), channels (x, y)
    coords = np.stack([K.map_coord(gx, flow[..., 0], 1), K.map_coord(gy, flow[..., 1], 1)], 0).astype(np.float64)
    coords = torch.from_numpy(coords)[None].permute(0, 2, 3, 1)                     # (1, H, W, 2)
    out = []
    for i in range(levels):
        corr = pyramid[i]
        dx = torch.linspace(-r, r, 2 * r + 1, dtype=torch.float64)
        dy = torch.linspace(-r, r, 2 * r + 1, dtype=torch.float64)
        delta = torch.stack(torch.meshgrid(dy, dx, indexing="ij"), axis=-1)         # RAFT's CorrBlock.__call__
        centroid_lvl = coords.reshape(h * w, 1, 1, 2) / 2 ** i
        coords_lvl = centroid_lvl + delta.view(1, 2 * r + 1, 2 * r + 1, 2)
        hl, wl = corr.shape[-2:]
        xgrid, ygrid = coords_lvl.split([1, 1], dim=-1)                             # RAFT's bilinear_sampler
        xgrid = 2 * xgrid / (wl - 1) - 1 if wl > 1 else xgrid * 0
        ygrid = 2 * ygrid / (hl - 1) - 1 if hl > 1 else ygrid * 0
        sampled = F.grid_sample(corr, torch.cat([xgrid, ygrid], dim=-1), align_corners=True)
        out.append(sampled.view(1, h, w, -1))
    got = torch.cat(out, dim=-1).permute(0, 3, 1, 2)[0].numpy()
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    # and the other order is a different array
    assert np.abs(got - K.lookup64(f1, f2, flow, 1, r, levels, 1.0 / np.sqrt(np.float64(c)), "yx")).max() > 1e-3 * np.abs(want).max()


# ---------------------------------------------------------------------------------------------- argument checks, ctypes table
def test_corr_args():
    ok = args.corr_args(4, 4, None, 'xy', nat.QUANT_EXACT, 256, (136, 240))
    assert ok == (4, 4, np.float32(0.0625), nat.CORR_XY, nat.QUANT_EXACT) and ok[2].dtype == np.float32
    assert args.corr_args(np.int64(1), 1, 2, 'yx', 0, 3, (1, 1)) == (1, 1, np.float32(2.0), nat.CORR_YX, 0)
    assert args.corr_args(1, 1, None, 'xy', 1, 3, (1, 1))[2] == np.float32(1.0 / np.sqrt(np.float64(3)))
    for bad in (0, 5, -1):
        with pytest.raises(ValueError, match="radius must be in 1 ... 4"):
            args.corr_args(bad, 1, None, 'xy', 1, 8, (8, 8))
    for bad in (0, 9):
        with pytest.raises(ValueError, match="levels must be in 1 ... 8"):
            args.corr_args(4, bad, None, 'xy', 1, 8, (8, 8))
    with pytest.raises(ValueError, match="level 3 of a 8 x 7 grid is empty"):
        args.corr_args(4, 4, None, 'xy', 1, 8, (8, 7))
    args.corr_args(4, 3, None, 'xy', 1, 8, (8, 7))
    with pytest.raises(ValueError, match="order must be 'xy' or 'yx'"):
        args.corr_args(4, 1, None, 'zz', 1, 8, (8, 8))
    with pytest.raises(ValueError, match="quant must be"):
        args.corr_args(4, 1, None, 'xy', 2, 8, (8, 8))
    with pytest.raises(ValueError, match="scale must be finite"):
        args.corr_args(4, 1, float('nan'), 'xy', 1, 8, (8, 8))
    with pytest.raises(ValueError, match="scale must be finite"):
        args.corr_args(4, 1, 1e39, 'xy', 1, 8, (8, 8))
    for kw in (dict(radius=True), dict(radius=2.0), dict(levels=None), dict(quant=1.0), dict(order=1), dict(scale='1'), dict(scale=True)):
        a = dict(radius=4, levels=1, scale=None, order='xy', quant=1, channels=8, shape=(8, 8))
        a.update(kw)
        with pytest.raises(TypeError, match="Error looking up correlation"):
            args.corr_args(**a)


def test_host_form_refuses_before_any_launch():
    a = np.zeros((4, 5, 6), np.float32)
    with pytest.raises(TypeError, match="fmap1 needs to be a numpy array"):
        of.correlation_lookup([1.0], a)
    with pytest.raises(TypeError, match="fmap2 needs to have dtype float32 or float16"):
        of.correlation_lookup(a, a.astype(np.float64))
    with pytest.raises(ValueError, match=r"shape \(C, H, W\)"):
        of.correlation_lookup(a[None], a[None])
    with pytest.raises(ValueError, match="the same shape"):
        of.correlation_lookup(a, np.zeros((4, 5, 7), np.float32))
    with pytest.raises(ValueError, match="radius must be"):
        of.correlation_lookup(a, a, radius=5)
    with pytest.raises(ValueError, match="flow needs to have shape"):
        of.correlation_lookup(a, a, np.zeros((5, 6), np.float32))
    with pytest.raises(TypeError, match="flow needs to be a numpy array"):
        of.correlation_lookup(a, a, [0.0])
    with pytest.raises(ValueError, match="Input is not 's' or 't'"):
        of.correlation_lookup(a, a, ref='x')
    with pytest.raises(TypeError, match="fmap1 needs to be a DeviceTensor"):
        of.DeviceCorrelation.build(a, a)


def test_ctypes_table_has_the_new_symbols():
    assert (nat.CORR_V, nat.CORR_L) == (K.V, K.L) == (4, 16)
    assert hasattr(of, "DeviceCorrelation") and hasattr(of.DeviceTensor, "correlation")
