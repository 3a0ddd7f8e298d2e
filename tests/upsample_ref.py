"""K17 restated in NumPy (the definition of include/ofl.h), plus the shapes and inputs the tests of the convex upsampling share.

`upsample` repeats the kernel operation for operation in float32 -- every array operation below rounds once, nothing is
fused --, so the device result is compared with it byte for byte.  `upsample64` is the same definition in float64 with
np.exp (and without the -87 cut-off, which changes a weight by less than e^-87); `upsample_unfold` is the textbook
unfold / softmax / sum / permute / reshape formulation, which pins the channel order and the output pixel order.

The error bound of `upsample` against `upsample64`, with eps = 2^-24 the unit round-off of float32, U = max_k |f v_k| over
the window, and E the relative error of exp32 in units of eps (measured in tests/test_upsample_host.py).  Since one t_k is
0, s >= 1, and a = sum e_k u_k obeys |a| <= U s.  To first order, relative to U for a / s:
    the 9 products e_k u_k       each term is off by eps |e_k u_k|, together at most eps U s             1
    the 8 additions on a         each partial sum is at most U s                                         8
    the 8 additions on s         each partial sum is at most s                                           8
    the division                                                                                         1
    the rounded t_k = x_k - M    exp(t (1 + eta)) = exp(t) (1 + t eta): the weights are off by |t_k| e^{t_k} eps; t = 0 for
                                 the maximum and |t| e^t <= 1 / e for the 8 others, in a and again in s   2 * 8 / e < 6
    exp32                        in a and again in s                                                     2 E
so |upsample - upsample64| <= (24 + 2 E) eps U.  The inputs of the tests are of ordinary magnitude: no term is subnormal.

The kernel's tile is T coarse pixels of ONE coarse row: T = 64 in the planar layout and 128 / f (16, 32, 64) in channels-last;
a planar block holds min(f, 4) sub-rows.  SHAPES are coarse shapes."""
import numpy as np

FACTORS = (2, 4, 8)
SHAPES = [(1, 1), (1, 2), (2, 1), (3, 3), (2, 65), (5, 130), (17, 7), (4, 37), (3, 200)]
#          ragged against every tile: (4, 37), (2, 65); more than two tiles per axis: (3, 200) and (5, 130) (rows are tiles of 1)
SPREADS = (1.0, 32.0, 200.0)
CUT = np.float32(-87.0)
EPS = 2.0 ** -24

_LOG2E, _LN2_HI, _LN2_LO = np.float32(1.44269504), np.float32(0.693359375), np.float32(-2.12194440e-4)
_COEF = [np.float32(1.0) / np.float32(c) for c in (5040.0, 720.0, 120.0, 24.0, 6.0)] + [np.float32(0.5), np.float32(1.0), np.float32(1.0)]
BREAKPOINTS = (np.arange(-126, 1, dtype=np.float64) + 0.5) / float(_LOG2E)      # where rint(t * log2e) changes


def exp32(t):
    """exp(t) for float32 t in [-87, 0] by the kernel's sequence of float32 operations (anything else: garbage, no error)"""
    t = np.asarray(t, np.float32)
    with np.errstate(all="ignore"):
        n = np.rint(t * _LOG2E)
        r = t - n * _LN2_HI
        r = r - n * _LN2_LO
        p = np.full(t.shape, _COEF[0], np.float32)
        for c in _COEF[1:]:
            p = p * r
            p = p + c
        assert p.dtype == np.float32 and n.dtype == np.float32
        bits = p.view(np.uint32) + (n.astype(np.int64).astype(np.uint32) << np.uint32(23))
    return bits.view(np.float32)


def bf16_bits(a):
    """float32 array -> the uint16 bit patterns of its bfloat16 roundings (nearest even; finite inputs)"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def widen(x, bfloat16=False):
    """logits as stored -> float32 (exact): float32, float16, or uint16 bit patterns of bfloat16"""
    x = np.asarray(x)
    if bfloat16:
        return (x.astype(np.uint32) << np.uint32(16)).view(np.float32)
    assert x.dtype in (np.float32, np.float16)
    return x.astype(np.float32)


def _taps(v, f, dtype):
    h, w = v.shape[:2]
    vp = np.zeros((h + 2, w + 2, 2), dtype)
    vp[1:-1, 1:-1] = np.asarray(v, np.float32) * np.float32(f)                  # exact: f is a power of two
    return [vp[k // 3:k // 3 + h, k % 3:k % 3 + w] for k in range(9)]


def _fine(a, f, h, w):
    """(f, f, h, w) indexed [i][j][y][x] -> (f h, f w)"""
    return np.ascontiguousarray(a.transpose(2, 0, 3, 1)).reshape(f * h, f * w)


def out_mask(m, f):
    m = np.asarray(m) != 0
    h, w = m.shape
    ok = np.ones((h + 2, w + 2), bool)
    ok[1:-1, 1:-1] = m
    cm = np.ones((h, w), bool)
    for k in range(9):
        cm &= ok[k // 3:k // 3 + h, k % 3:k % 3 + w]
    return np.repeat(np.repeat(cm, f, 0), f, 1).astype(np.uint8)


def upsample(v, m, x, f, bfloat16=False):
    """-> (out_vecs float32 (f h, f w, 2), out_mask uint8 (f h, f w)); x: logits (9 f^2, h, w) as stored"""
    h, w = np.asarray(v).shape[:2]
    x = widen(x, bfloat16).reshape(9, f, f, h, w)
    u = _taps(v, f, np.float32)
    with np.errstate(all="ignore"):
        big = x[0]
        for k in range(1, 9):
            big = np.maximum(big, x[k])
        s = a0 = a1 = None
        for k in range(9):
            t = x[k] - big
            e = np.where(t < CUT, np.float32(0.0), exp32(t))
            e0, e1 = e * u[k][..., 0], e * u[k][..., 1]
            s, a0, a1 = (e, e0, e1) if k == 0 else (s + e, a0 + e0, a1 + e1)
        o0, o1 = a0 / s, a1 / s
    assert o0.dtype == np.float32 and s.dtype == np.float32
    return np.stack([_fine(o0, f, h, w), _fine(o1, f, h, w)], -1), out_mask(m, f)


def upsample64(v, x, f, bfloat16=False):
    """the definition in float64 with np.exp -> out_vecs float64 (f h, f w, 2)"""
    h, w = np.asarray(v).shape[:2]
    x = widen(x, bfloat16).astype(np.float64).reshape(9, f, f, h, w)
    u = _taps(v, f, np.float64)
    e = np.exp(x - x.max(0))
    s = e.sum(0)
    return np.stack([_fine(sum(e[k] * u[k][..., c] for k in range(9)) / s, f, h, w) for c in (0, 1)], -1)


def window_max(v, f):
    """max_k |f v_k| over the 3 x 3 window, per fine pixel and over both components -> float64 (f h, f w)"""
    u = np.max([np.abs(t).max(-1) for t in _taps(v, f, np.float64)], 0)
    return np.repeat(np.repeat(u, f, 0), f, 1)


def upsample_unfold(v, x, f):
    """RAFT's upsample_flow in NumPy float64: unfold(f * flow, [3, 3], padding=1), softmax over the 9 taps, sum, permute,
    reshape.  v: (h, w, 2); x: (9 f^2, h, w) -> (f h, f w, 2)"""
    h, w = v.shape[:2]
    flow = np.asarray(v, np.float64).transpose(2, 0, 1) * f                        # (2, h, w)
    mask = np.asarray(x, np.float64).reshape(1, 9, f, f, h, w)
    mask = np.exp(mask - mask.max(1, keepdims=True))
    mask = mask / mask.sum(1, keepdims=True)                                     # softmax(dim = 1) of view(1, 9, f, f, h, w)
    padded = np.pad(flow, ((0, 0), (1, 1), (1, 1)))
    unfolded = np.stack([padded[:, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)], 1)      # (2, 9, h, w): unfold's order
    up = (mask * unfolded.reshape(2, 9, 1, 1, h, w)).sum(1)                      # (2, f, f, h, w)
    up = up.transpose(0, 3, 1, 4, 2)                                             # permute(0, 1, 4, 2, 5, 3) without the batch axis
    return up.reshape(2, f * h, f * w).transpose(1, 2, 0)


# ---------------------------------------------------------------------------------------------- shared inputs
def vectors(shape, seed=0):
    """ordinary magnitudes with exact zeros and -0.0 sprinkled in"""
    rng = np.random.default_rng(1000 + seed + 31 * shape[0] + shape[1])
    v = (rng.standard_normal(shape + (2,)) * 6).astype(np.float32)
    z = rng.random(shape + (2,))
    v[z < 0.08] = 0.0
    v[z > 0.94] = -0.0
    return v


def coarse_mask(shape, seed=0):
    """mostly valid, with holes at the four corners, on the edges and in the interior (where the shape has them)"""
    rng = np.random.default_rng(2000 + seed + 31 * shape[0] + shape[1])
    m = (rng.random(shape) < 0.9).astype(np.uint8)
    h, w = shape
    if h * w > 1:
        m[0, 0] = m[-1, -1] = 0
        m[0, w // 2] = m[h // 2, 0] = 0
    if h > 2 and w > 2:
        m[h // 2, w // 2] = 0
        m[0, -1] = m[-1, 0] = 0
    return m


def logits(shape, f, spread, seed=0):
    """float32 logits (9 f^2, h, w), uniform in [-spread / 2, spread / 2]: spread 200 puts taps on both sides of the -87 cut"""
    rng = np.random.default_rng(3000 + seed + 31 * shape[0] + shape[1] + 7 * f + int(spread))
    return ((rng.random((9 * f * f,) + shape) - 0.5) * spread).astype(np.float32)


def stored(x, elem):
    """float32 logits -> (the array as stored, bfloat16 flag): elem 'float32', 'float16' or 'bfloat16' (uint16 bit patterns)"""
    if elem == "bfloat16":
        return bf16_bits(x), True
    return x.astype(np.dtype(elem)), False


def to_layout(x, layout):
    """(…, C, h, w) as stored -> the memory order of `layout` ('chw' or 'hwc'), contiguous"""
    return np.ascontiguousarray(x if layout == "chw" else np.moveaxis(x, -3, -1))
