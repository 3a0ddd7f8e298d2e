"""CPU suite: the host half of the global matching (K19) -- args.match_args, the published constants, the argument checks of
of.global_match and DeviceCorrelation.match -- and the NumPy restatement tests/match_ref.py that test_gpu_match.py compares
the kernel with: its distance from the float64 definition against the bound derived in match_ref.py, the float64 definition
against GMFlow's formulation computed by torch, the summation order on a case whose answer depends on it, and known answers
that are exact.

Largest ratios seen of the restatement's error to the bound (printed by the first test): vectors 0.020, confidence 0.079."""
import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import args, _native as nat
import match_ref as M

DTYPES = ("float32", "float16", "bfloat16")


# ---------------------------------------------------------------------------------------------- restatement against float64
@pytest.mark.parametrize("shape", ((1, 33), (5, 7), (9, 12), (6, 40)))
def test_restatement_is_within_the_derived_bound_of_float64(shape):
    h, w = shape
    worst = worst_conf = 0.0
    for c in (3, 64, 131):
        for k, dtype in enumerate(DTYPES):
            f1, f2 = (M.widen(M.features(shape, c, dtype, seed), dtype) for seed in (k, k + 10))
            sign = 1 if k % 2 else -1
            for scale in (None, 1.0):                                        # 1.0: sharp maxima, most weights cut
                sc = M.default_scale(c) if scale is None else np.float32(scale)
                vecs, mask, conf, index = M.match(f1, f2, scale, sign, dots=M.dots_chain)
                want, conf64, s64 = M.match64(f1, f2, scale, sign)
                mag = M.magnitude(f1, f2)
                b, cb = M.bound(c, h, w, sc, mag), M.conf_bound(c, h, w, sc, mag)
                err = float(np.abs(vecs.astype(np.float64) - want).max())
                cerr = float((np.abs(conf.astype(np.float64) - conf64) / conf64).max())
                worst, worst_conf = max(worst, err / b if b else 0.0), max(worst_conf, cerr / cb)
                assert err <= b and cerr <= cb, (shape, c, dtype, scale, err, b, cerr, cb)
                assert mask.all() and ((index >= 0) & (index < h * w)).all()
                delta = (c + 1) * M.EPS * float(sc) * mag                    # the index is a maximum up to the logits' error
                assert (s64[np.arange(h * w), index.ravel()] >= s64.max(1) - 2 * delta).all()
    print("{}: worst error {:.3f} of the bound, confidence {:.3f}".format(shape, worst, worst_conf))
    assert worst > 0.0 and worst_conf > 0.0


def test_the_bound_counts_what_its_docstring_says():
    eps = M.EPS
    # 960 keys: 30 tiles, 8 for the busiest group, 128 keys a partial sum
    k, n, soft, p = M._parts(16, 24, 40, 0.25, 8.0)
    assert (k, n, p) == (960, 128, 39) and soft == np.expm1(2 * 17 * eps * 0.25 * 8.0)
    first = 2 * 128 + 9 + 2 * np.log(960) + 2 * 2.0
    assert M.bound(16, 24, 40, 0.25, 8.0) == (soft + first * eps / (1 - first * eps) + 2 * 960 * np.exp(-87.0)) * 39
    assert M._parts(1, 1, 1, 1.0, 1.0)[1:] == (16, np.expm1(4 * eps), 0) and M.bound(1, 1, 1, 1.0, 1.0) == 0.0
    assert M._parts(1, 1, 129, 1.0, 1.0)[1] == 32


# ---------------------------------------------------------------------------------------------- GMFlow's formulation in torch
def test_float64_definition_equals_gmflows_formulation():
    torch = pytest.importorskip("torch")
    shape, c = (7, 11), 10
    h, w = shape
    f1, f2 = (M.widen(M.features(shape, c, "float32", s), "float32") for s in (4, 5))
    want, conf, _ = M.match64(f1, f2, 1.0 / np.sqrt(np.float64(c)))
    # global_correlation_softmax of GMFlow's matching.py, in float64 on the CPU
    feature0 = torch.from_numpy(f1.astype(np.float64)).permute(2, 0, 1)[None]         # (1, C, H, W)
    feature1 = torch.from_numpy(f2.astype(np.float64)).permute(2, 0, 1)[None]
    a = feature0.view(1, c, -1).permute(0, 2, 1)
    b = feature1.view(1, c, -1)
    correlation = torch.matmul(a, b).view(1, h, w, h, w) / (c ** 0.5)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    init_grid = torch.stack([xs, ys], 0)[None]                                       # coords_grid: (1, 2, H, W), x first
    grid = init_grid.view(1, 2, -1).permute(0, 2, 1)
    prob = torch.nn.functional.softmax(correlation.view(1, h * w, h * w), dim=-1)
    correspondence = torch.matmul(prob, grid).view(1, h, w, 2).permute(0, 3, 1, 2)
    flow = (correspondence - init_grid)[0].permute(1, 2, 0).numpy()
    assert np.abs(flow - want).max() <= 1e-12 * max(h, w)
    assert np.abs(prob.max(-1).values.view(h, w).numpy() - conf).max() <= 1e-14
    # a restatement with x and y swapped is a different array
    assert np.abs(flow[..., ::-1] - want).max() > 1e-3


# ---------------------------------------------------------------------------------------------- the summation order
def test_the_summation_order_is_the_stated_one():
    e = np.float32(2.0 ** -24)
    # keys 0 and 1 share partial sum P[0][0]: 1 + e loses e, and again for key 2 and 3
    row = np.zeros((1, 300), np.float32)
    row[0, :4] = [1.0, e, e, e]
    assert M.ordered_sum(row)[0] == np.float32(1.0)
    # keys 4 .. 7 are the other half: e + e + e + e = 4 e survives, then 1 + 4 e
    row = np.zeros((1, 300), np.float32)
    row[0, 0], row[0, 4:8] = 1.0, e
    assert M.ordered_sum(row)[0] == np.float32(1.0) + np.float32(4) * e
    # tile 1 is group 1, tile 4 is group 0 again and continues P[0][0]; key 8 is half 0 of tile 0
    row = np.zeros((1, 300), np.float32)
    row[0, 0], row[0, 8], row[0, 128], row[0, 32], row[0, 33] = 1.0, e, e, e, e
    assert M.ordered_sum(row)[0] == np.float32(1.0) + np.float32(2) * e              # ((1 + e) + e) + (e + e)
    # a general case against the formula spelt out
    x = np.random.default_rng(0).random((3, 200)).astype(np.float32)
    pad = np.zeros((3, 256), np.float32)
    pad[:, :200] = x
    s = []
    for w in range(4):
        halves = []
        for hh in range(2):
            acc = np.zeros(3, np.float32)
            for j in (w, w + 4):
                for o in range(32):
                    if (o >> 2) & 1 == hh:
                        acc = acc + pad[:, 32 * j + o]
            halves.append(acc)
        s.append(halves[0] + halves[1])
    assert M.ordered_sum(x).tobytes() == (((s[0] + s[1]) + s[2]) + s[3]).tobytes()
    assert (nat.MATCH_TILE, nat.MATCH_WAVES) == (M.T, M.G) == (32, 4)


# ---------------------------------------------------------------------------------------------- known answers, exact
def test_all_zero_features_give_the_mean_coordinate():
    for h, w in ((1, 1), (3, 5), (6, 40)):
        z = np.zeros((h, w, 4), np.float32)
        vecs, mask, conf, index = M.match(z, z)
        gy, gx = np.mgrid[:h, :w]
        assert not index.any() and mask.all()
        assert conf.tobytes() == np.full((h, w), np.float32(1.0) / np.float32(h * w), np.float32).tobytes()
        assert np.array_equal(vecs[..., 0], np.float32((w - 1) / 2) - gx) and np.array_equal(vecs[..., 1], np.float32((h - 1) / 2) - gy)


def test_a_duplicated_key_gives_the_lower_index():
    f1 = M.widen(M.int_features((4, 9), 6, "float32", 2, 1), "float32")
    f2 = M.widen(M.int_features((4, 9), 6, "float32", 2, 2), "float32")
    f2[3, 4] = f2[1, 2] = 3 * f1[2, 2]                                              # keys 11 and 31 both match query (2, 2) best
    index = M.match(f1, f2)[3]
    assert f1[2, 2].any() and index[2, 2] == 11


def test_a_shift_is_recovered_exactly():
    shape, (dx, dy) = (5, 7), (2, 1)
    h, w = shape
    f1, f2 = M.one_hot_pair(shape, (dx, dy))
    for sign in (1, -1):
        vecs, mask, conf, index = M.match(f1, f2, 100.0, sign)                      # the others are 100 below: cut
        gy, gx = np.mgrid[:h, :w]
        assert np.array_equal(index, ((gy + dy) % h) * w + (gx + dx) % w)
        assert (conf == 1.0).all() and mask.all()
        inside = (gx + dx < w) & (gy + dy < h)
        assert np.array_equal(vecs[inside], np.broadcast_to(np.float32([sign * dx, sign * dy]), (inside.sum(), 2)))


def test_min_confidence_splits_the_mask_between_two_confidences():
    f1, f2 = (M.widen(M.features((5, 7), 8, "float32", s), "float32") for s in (0, 1))
    conf = np.sort(M.match(f1, f2, dots=M.dots_chain)[2].ravel())
    assert conf[10] < conf[11]
    thr = np.float32((np.float64(conf[10]) + np.float64(conf[11])) / 2)
    vecs, mask, conf2, _ = M.match(f1, f2, min_conf=thr, dots=M.dots_chain)
    assert mask.sum() == 35 - 11 and np.array_equal(mask != 0, conf2 >= thr)
    assert np.array_equal(M.match(f1, f2, min_conf=conf[11], dots=M.dots_chain)[1] != 0, conf2 >= conf[11])     # >=, not >


# ---------------------------------------------------------------------------------------------- argument checks
def test_match_args():
    ok = args.match_args(None, None, 256, 'float16', 'float16')
    assert ok == (np.float32(0.0625), np.float32(0.0)) and ok[0].dtype == np.float32 and ok[1].dtype == np.float32
    assert args.match_args(2, 0.5, 3, 'float32', 'float32') == (np.float32(2.0), np.float32(0.5))
    assert args.match_args(None, 1, 3, 'bfloat16', 'bfloat16')[0] == np.float32(1.0 / np.sqrt(np.float64(3)))
    with pytest.raises(ValueError, match="the same dtype, got float16 and float32"):
        args.match_args(None, None, 8, 'float16', 'float32')
    with pytest.raises(ValueError, match="1 ... 512 channels, got 513"):
        args.match_args(None, None, 513, 'float32', 'float32')
    args.match_args(None, None, 512, 'float32', 'float32')
    for bad in (float('nan'), 1e39, float('inf')):
        with pytest.raises(ValueError, match="scale must be finite"):
            args.match_args(bad, None, 8, 'float32', 'float32')
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match=r"min_confidence must be in \[0, 1\]"):
            args.match_args(None, bad, 8, 'float32', 'float32')
    with pytest.raises(ValueError, match="min_confidence must be finite"):
        args.match_args(None, float('nan'), 8, 'float32', 'float32')
    for kw in (dict(scale='1'), dict(scale=True), dict(min_confidence=False), dict(min_confidence=[0.5])):
        a = dict(scale=None, min_confidence=None, channels=8, dtype1='float32', dtype2='float32')
        a.update(kw)
        with pytest.raises(TypeError, match="Error matching features"):
            args.match_args(**a)


def test_host_form_refuses_before_any_launch():
    a = np.zeros((4, 5, 6), np.float32)
    with pytest.raises(TypeError, match="fmap1 needs to be a numpy array"):
        of.global_match([1.0], a)
    with pytest.raises(TypeError, match="fmap2 needs to have dtype float32 or float16"):
        of.global_match(a, a.astype(np.float64))
    with pytest.raises(ValueError, match=r"shape \(C, H, W\)"):
        of.global_match(a[None], a[None])
    with pytest.raises(ValueError, match="the same shape"):
        of.global_match(a, np.zeros((4, 5, 7), np.float32))
    with pytest.raises(ValueError, match="the same dtype, got float32 and float16"):
        of.global_match(a, a.astype(np.float16))
    with pytest.raises(ValueError, match="Input is not 's' or 't'"):
        of.global_match(a, a, ref='x')
    with pytest.raises(ValueError, match="min_confidence must be in"):
        of.global_match(a, a, min_confidence=2.0)
    with pytest.raises(TypeError, match="return_index needs to be a boolean"):
        of.global_match(a, a, return_index=1)
    with pytest.raises(ValueError, match="1 ... 512 channels"):
        of.global_match(np.zeros((513, 2, 2), np.float32), np.zeros((513, 2, 2), np.float32))


def test_the_new_symbols_exist():
    assert hasattr(of, "global_match") and hasattr(of.DeviceCorrelation, "match") and hasattr(of.DeviceTensor, "match")
    assert hasattr(args, "match_args")
    assert "ofl_global_match_dev" in nat.SIGNATURES and "ofl_global_match" in nat.SIGNATURES
