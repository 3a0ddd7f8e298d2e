"""K19 restated in NumPy (the definition of include/ofl.h), plus the inputs the tests of the global matching share.

`match` repeats the kernel operation for operation in float32 from the logits on -- every array operation below rounds once,
nothing is fused, and the three sums run in the order the header states (T = 32 keys a tile, tile j to group j mod 4, two
halves a tile, `ordered_sum`).  The dot products themselves come from the matrix core, whose order inside one instruction
is not stated: `dots_exact` is for integer-valued features, where every partial sum is an exact float32 integer and the
order does not matter -- there the device must equal `match` byte for byte --, `dots_chain` is the channel-ascending chain
acc = float32(acc + a_c b_c) (the product exact, one rounding a step: the float32 MFMA's fmaf chain, up to the double
rounding of going through float64), which is what the CPU tests hold against the bound.  `match64` is the definition in
float64 with np.exp and without the -87 cut.

`bound(c, h, w, scale, mag)`: how far u or v of a float32 evaluation may lie from `match64`, in pixels.  With eps = 2^-24,
K = H W keys, P = max(W - 1, H - 1) (no coordinate and no expected coordinate exceeds it) and mag = max_k sum_c |f1 f2|:
  1 the logits   under the standard model -- products exact, every addition rounded to float32, in ANY order -- a sum of C
                 terms and the product with `scale` carry (C + 1) roundings at most: |s_k - s64_k| <= delta =
                 (C + 1) eps scale mag.
  2 the softmax  logits off by delta at most change every weight ratio by a factor within e^(+-2 delta), so an expected
                 coordinate in [0, P] moves by (e^(2 delta) - 1) P at most.
  3 the sums     every term is >= 0, so a rounded sum is off by (number of additions) eps relative.  A partial sum takes
                 n = 16 ceil(ceil(K / 32) / 4) keys (n additions, the first onto +0 is exact), then 1 addition of the halves
                 and 3 of the groups; ax, ay carry the rounded product e kx on top: l is off by (n + 3) eps, ax by
                 (n + 4) eps, the quotient adds 1 and u = mx - x (|u| <= P) 1:  (2 n + 9) eps P.
    t = s - m    rounded once: e^(t (1 + eta)) = e^t (1 + t eta), so weight k is off by |t_k| eps relative; averaged with the
                 weights p_k = e_k / l this is sum p_k |t_k| = entropy - ln l <= ln K, in ax and again in l:  2 ln(K) eps P.
    exp32        E eps relative (E <= 2, asserted in tests/test_upsample_host.py), in ax and again in l:  2 E eps P.
    the cut      weights below e^-87 are dropped: at most K e^-87 of the total, twice:  2 K e^-87 P.
`bound` adds 1 to 3 with the first-order terms inflated by 1 / (1 - k eps).  `conf_bound` is the same for the relative error
of the confidence 1 / l: (e^(2 delta) - 1) + (n + 3 + ln K + E + 1) eps + K e^-87.

The kernel's tile is 32 keys, four waves share the keys of a block of 32 (or 64) queries (a round is 128 keys), a lane's keys span 28
and wrap once for W >= 28; the channels go 16 (16-bit) or 4 (float32) a chunk, and aligned tensors of C <= 128 (16-bit) or
<= 64 (float32) keep the queries in registers.  GRIDS and CHANNELS are ragged against all of these."""
import numpy as np

import correlation_ref as K
import upsample_ref as U

T, G = 32, 4                       # OFL_MATCH_TILE, OFL_MATCH_WAVES
EPS = 2.0 ** -24
F32 = np.float32
EXP_E = 2.0
#        one pixel; a tile minus / exactly / plus one key; two rows under a tile; W on both sides of 28; one round exactly and
#        plus two keys (W < 28); six tiles and a bit; 18 and 30 query blocks
GRIDS = [(1, 1), (1, 31), (1, 32), (1, 33), (5, 7), (3, 27), (3, 28), (2, 64), (5, 26), (3, 70), (17, 33), (24, 40)]
#        both sides of the 16-bit step (16) and of the float32 chunk (4), of the register-held limits (64 / 68, 128 / 136),
#        the largest; odd counts go element by element
CHANNELS = [1, 3, 8, 15, 16, 17, 20, 32, 64, 68, 100, 128, 130, 136, 256, 512]


def widen(a, dtype):
    return K.widen(a, dtype)


def default_scale(c):
    return K.default_scale(c)


# ---------------------------------------------------------------------------------------------- the dot products
def dots_exact(f1, f2):
    """(H, W, C) x (H, W, C) float32, integer-valued -> D float32 (HW, HW), exact in any order (asserted)"""
    a = np.asarray(f1, np.float32).reshape(-1, f1.shape[-1]).astype(np.float64)
    b = np.asarray(f2, np.float32).reshape(-1, f2.shape[-1]).astype(np.float64)
    assert (a == np.rint(a)).all() and (b == np.rint(b)).all() and (np.abs(a) @ np.abs(b).T).max() < 2.0 ** 24
    return (a @ b.T).astype(np.float32)


def dots_chain(f1, f2):
    """acc = float32(acc + a_c * b_c) from +0 with the channels ascending"""
    a = np.asarray(f1, np.float32).reshape(-1, f1.shape[-1]).astype(np.float64)
    b = np.asarray(f2, np.float32).reshape(-1, f2.shape[-1]).astype(np.float64)
    acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for c in range(a.shape[1]):
        acc = (acc.astype(np.float64) + a[:, c, None] * b[None, :, c]).astype(np.float32)
    return acc


# ---------------------------------------------------------------------------------------------- the restatement
def ordered_sum(e):
    """(Q, K) float32, no negative term -> (Q,): the 2 G partial sums P[w][h] over tiles j = w (mod G) and key offsets
    o = 8 a + 4 h + b in ascending key order from +0, S_w = P[w][0] + P[w][1], ((S_0 + S_1) + S_2) + S_3"""
    e = np.asarray(e, np.float32)
    q, k = e.shape
    kp = -(-k // (G * T)) * G * T
    pad = np.zeros((q, kp), np.float32)                    # a key that does not exist adds +0: no bit changes
    pad[:, :k] = e
    a = pad.reshape(q, kp // (G * T), G, 4, 2, 4)          # [round][w][a][h][b]
    p = np.zeros((q, G, 2), np.float32)
    for j in range(a.shape[1]):
        for aa in range(4):
            for b in range(4):
                p = p + a[:, j, :, aa, :, b]
    s = p[..., 0] + p[..., 1]
    out = ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]
    assert out.dtype == np.float32
    return out


def match(f1, f2, scale=None, sign=1, min_conf=0.0, dots=dots_exact):
    """One item.  f1, f2: float32 (H, W, C) (widened) -> (vecs float32 (H, W, 2), mask uint8, conf float32, index int32)"""
    h, w, c = f1.shape
    scale = default_scale(c) if scale is None else F32(scale)
    ky, kx = np.divmod(np.arange(h * w), w)
    with np.errstate(all="ignore"):
        s = dots(f1, f2) * scale
        m = s.max(1)
        idx = s.argmax(1)                                  # the first of equal maxima
        t = s - m[:, None]
        e = np.where(t < U.CUT, F32(0.0), U.exp32(t))
        l = ordered_sum(e)
        ax, ay = ordered_sum(e * kx.astype(np.float32)), ordered_sum(e * ky.astype(np.float32))
        u, v = ax / l - kx.astype(np.float32), ay / l - ky.astype(np.float32)
        vecs = F32(sign) * np.stack([u, v], -1)
        conf = F32(1.0) / l
    assert s.dtype == np.float32 and vecs.dtype == np.float32 and conf.dtype == np.float32
    return (vecs.reshape(h, w, 2), (conf >= F32(min_conf)).astype(np.uint8).reshape(h, w), conf.reshape(h, w),
            idx.astype(np.int32).reshape(h, w))


def match_batch(f1, f2, **kw):
    """(N, H, W, C) -> the four outputs stacked"""
    outs = [match(f1[i], f2[i], **kw) for i in range(f1.shape[0])]
    return tuple(np.stack([o[k] for o in outs]) for k in range(4))


# ---------------------------------------------------------------------------------------------- the float64 definition
def logits64(f1, f2, scale=None):
    c = f1.shape[-1]
    scale = np.float64(default_scale(c) if scale is None else scale)             # a given scale is taken as it is, in float64
    a = np.asarray(f1, np.float32).reshape(-1, c).astype(np.float64)
    b = np.asarray(f2, np.float32).reshape(-1, c).astype(np.float64)
    return (a @ b.T) * scale


def match64(f1, f2, scale=None, sign=1):
    """-> (vecs float64 (H, W, 2), conf float64 (H, W), logits float64 (HW, HW))"""
    h, w, _ = f1.shape
    s = logits64(f1, f2, scale)
    e = np.exp(s - s.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    ky, kx = np.divmod(np.arange(h * w), w)
    vecs = sign * np.stack([p @ kx.astype(np.float64) - kx, p @ ky.astype(np.float64) - ky], -1)
    return vecs.reshape(h, w, 2), p.max(1).reshape(h, w), s


def magnitude(f1, f2):
    return K.magnitude(f1, f2)


def _parts(c, h, w, scale, mag):
    k = h * w
    n = 16 * -(-(-(-k // T)) // G)
    delta = (c + 1) * EPS * float(scale) * mag
    return k, n, np.expm1(2.0 * delta), max(w - 1, h - 1, 0)


def bound(c, h, w, scale, mag, e=EXP_E):
    """module docstring -> pixels"""
    k, n, soft, p = _parts(c, h, w, scale, mag)
    first = 2 * n + 9 + 2 * np.log(k) + 2 * e
    return (soft + first * EPS / (1 - first * EPS) + 2 * k * np.exp(-87.0)) * p


def conf_bound(c, h, w, scale, mag, e=EXP_E):
    """module docstring -> relative"""
    k, n, soft, _ = _parts(c, h, w, scale, mag)
    first = n + 3 + np.log(k) + e + 1
    return soft + first * EPS / (1 - first * EPS) + k * np.exp(-87.0)


# ---------------------------------------------------------------------------------------------- shared inputs
def features(shape, c, dtype, seed=0):
    """random float features as stored in `dtype` (correlation_ref.features)"""
    return K.features(shape, c, dtype, seed)


def int_features(shape, c, dtype, reach, seed=0):
    """integer-valued features in {-reach ... reach} as stored in `dtype` (exact in all three types)"""
    rng = np.random.default_rng(7000 + seed + 31 * shape[0] + shape[1] + 7 * c + reach)
    a = rng.integers(-reach, reach + 1, shape + (c,)).astype(np.float32)
    return np.ascontiguousarray(K.R.from_f32(a, dtype))


def one_hot_pair(shape, shift):
    """f1: pixel p has a 1 in channel p; f2 = f1 rolled by shift = (dx, dy), so the match of (x, y) is (x + dx, y + dy)
    modulo the frame -> float32 (H, W, HW) twice"""
    h, w = shape
    f1 = np.eye(h * w, dtype=np.float32).reshape(h, w, h * w)
    return f1, np.ascontiguousarray(np.roll(f1, (shift[1], shift[0]), (0, 1)))
