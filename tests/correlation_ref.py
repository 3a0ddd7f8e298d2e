"""K18 restated in NumPy (the definition of include/ofl.h), plus the inputs the tests of the correlation lookup share.

`lookup` repeats the kernels operation for operation in float32 -- every array operation below rounds once, nothing is
fused --, so the device result is compared with it byte for byte.  `lookup64` is the textbook formulation in float64: the
all-pairs volume by einsum, mean-pooling of the volume, bilinear sampling of the pooled volume with zeros outside.  It takes
the sample position px, py as the definition states it (map_coord, float32, times 2^-l: part of the definition, not an error
of the restatement) and everything after that in float64.

The error bound of `lookup` against `lookup64`, with eps = 2^-24 the unit round-off of float32 and
M = max over all pixel pairs of sum_c |f1_c f2_c| at level 0 (a 2 x 2 mean of f2 cannot exceed it, so M bounds the sum at
every level, and a convex blend of dots cannot exceed it either).  The roundings on the longest path from an input to a
value, each of relative size eps on a quantity bounded by scale * M:
    pooling          2 per level below 0: (a + b), then + (c + d); the product with 0.25 is exact        2 (levels - 1)
    the product      f1_c * f2_c                                                                         1
    the chain        a partial sum holds V ceil(C / (V L)) products at most: one addition fewer        V ceil(C / (V L)) - 1
    the tree         log2(L) additions                                                                   4
    the weights      x0 = 1 - fx, y0 = 1 - fy, w = y0 * x0 (px - floor(px) itself is exact)              3
    the blend        one product and at most three additions per dot                                     4
    the scale                                                                                            1
With k their number, |lookup - lookup64| <= k eps / (1 - k eps) * scale * M (the usual gamma_k of a rounding chain); `bound`
returns k and the tests compare errors in units of eps * scale * M.  The inputs are of ordinary magnitude: nothing is
subnormal.

The kernel's tile is 32 pixels of ONE row, a wave takes every fourth pixel of it, the channels go 64 (element by element),
128 or 256 (four per load) a pass: GRIDS and channel_counts() are ragged against all of these."""
import numpy as np

import interop_ref as R

V, L = 4, 16
QUANT_OPENCV, QUANT_EXACT = 0, 1
EPS = 2.0 ** -24
GRIDS = [(1, 1), (2, 3), (5, 7), (3, 70), (17, 33)]
F32 = np.float32


def channel_counts():
    return [1, 3, V * L - 1, V * L, V * L + 1, 2 * V * L + 3]


def widen(a, dtype):
    """a tensor as stored ('float32', 'float16', or 'bfloat16' as uint16 bit patterns) -> float32, exact"""
    return np.ascontiguousarray(R.to_f32(np.asarray(a), dtype), np.float32)


def default_scale(c):
    return F32(1.0 / np.sqrt(np.float64(c)))


# ---------------------------------------------------------------------------------------------- the restatement
def pool(a):
    """(..., H, W, C) float32 -> (..., H >> 1, W >> 1, C): ((a + b) + (c + d)) * 0.25f, a trailing odd row / column dropped"""
    a = np.asarray(a, np.float32)
    h2, w2 = a.shape[-3] >> 1, a.shape[-2] >> 1
    assert h2 >= 1 and w2 >= 1, "a level of size 0 is refused"
    tl, tr = a[..., 0:2 * h2:2, 0:2 * w2:2, :], a[..., 0:2 * h2:2, 1:2 * w2:2, :]
    bl, br = a[..., 1:2 * h2:2, 0:2 * w2:2, :], a[..., 1:2 * h2:2, 1:2 * w2:2, :]
    out = ((tl + tr) + (bl + br)) * F32(0.25)
    assert out.dtype == np.float32
    return out


def pyramid(f2, levels):
    out = [np.asarray(f2, np.float32)]
    for _ in range(1, levels):
        out.append(pool(out[-1]))
    return out


def dot(a, b):
    """sum over the last axis of a * b in the order of the definition: groups of V channels dealt round-robin to L partial
    sums, each accumulated in ascending channel order, the partial sums added in a pairwise tree that leaves out a partial
    sum without a channel"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    c = a.shape[-1]
    prod = a * b
    parts = []
    for p in range(L):
        acc = None
        for g in range(p, (c + V - 1) // V, L):
            for ch in range(V * g, min(V * g + V, c)):
                acc = prod[..., ch] if acc is None else acc + prod[..., ch]
        parts.append(acc)
    while len(parts) > 1:
        parts = [lo if hi is None else lo + hi for lo, hi in zip(parts[0::2], parts[1::2])]
    assert parts[0].dtype == np.float32
    return parts[0]


def map_coord(grid, flow, sign):
    """NumPy's float32 += int64: the float64 sum rounded once"""
    f = np.asarray(flow, np.float32).astype(np.float64)
    return (grid.astype(np.float64) + f if sign >= 0 else grid.astype(np.float64) - f).astype(np.float32)


def make_tap(px, py, quant):
    """make_tap of ofl_common.h -> (ix, iy as int64, [w0, w1, w2, w3] as float32)"""
    with np.errstate(all="ignore"):
        if quant == QUANT_OPENCV:
            def snap(p):                                            # cv_round_coord: round half even, saturating, NaN -> INT_MIN
                s = np.nan_to_num(np.rint(p * F32(32.0)).astype(np.float64), nan=-2.0 ** 31, posinf=2.0 ** 31, neginf=-2.0 ** 31)
                s = np.clip(s, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)
                return np.clip(s >> 5, -32768, 32767), (s & 31).astype(np.float32) * F32(1.0 / 32.0)
            (ix, fx), (iy, fy) = snap(px), snap(py)
        else:
            flx, fly = np.floor(px), np.floor(py)
            fx, fy = px - flx, py - fly
            ix = np.fmin(np.fmax(flx, F32(-32768.0)), F32(32767.0)).astype(np.int64)
            iy = np.fmin(np.fmax(fly, F32(-32768.0)), F32(32767.0)).astype(np.int64)
        x0, y0 = F32(1.0) - fx, F32(1.0) - fy
        w = [y0 * x0, y0 * fx, fy * x0, fy * fx]
    assert all(v.dtype == np.float32 for v in w)
    return ix, iy, w


def blend4(v00, v01, v10, v11, w):
    s = v00 * w[0]
    s = s + v01 * w[1]
    s = s + v10 * w[2]
    s = s + v11 * w[3]
    return s


def positions(shape, flow, sign, level):
    h, w = shape
    gy, gx = np.mgrid[:h, :w]
    if flow is None:
        flow = np.zeros((h, w, 2), np.float32)
    inv = F32(2.0 ** -level)
    return map_coord(gx, flow[..., 0], sign) * inv, map_coord(gy, flow[..., 1], sign) * inv


def window_dots(f1, f2l, ix, iy, r):
    """the (2r + 2)^2 integer-tap dots of every pixel -> float32 (H, W, 2r + 2, 2r + 2) indexed [y][x][ty][tx]"""
    hl, wl = f2l.shape[:2]
    s = 2 * r + 2
    ty, tx = np.mgrid[:s, :s]
    yy, xx = iy[..., None, None] - r + ty, ix[..., None, None] - r + tx
    inside = (yy >= 0) & (yy < hl) & (xx >= 0) & (xx < wl)
    rows = f2l[np.clip(yy, 0, hl - 1), np.clip(xx, 0, wl - 1)]                    # (H, W, s, s, C)
    with np.errstate(all="ignore"):
        d = dot(f1[:, :, None, None, :], rows)
    return np.where(inside, d, F32(0.0)).astype(np.float32)


def lookup(f1, f2, flow=None, sign=1, radius=4, levels=1, scale=None, order="xy", quant=QUANT_EXACT, pyr=None):
    """One item.  f1, f2: float32 (H, W, C) (widened); flow float32 (H, W, 2) or None -> float32 (levels (2r + 1)^2, H, W).
    pyr: the pyramid of f2, if the caller has it already."""
    f1 = np.asarray(f1, np.float32)
    h, w, c = f1.shape
    r, win = radius, 2 * radius + 1
    scale = default_scale(c) if scale is None else F32(scale)
    pyr = pyramid(f2, levels) if pyr is None else pyr
    out = np.empty((levels, win, win, h, w), np.float32)
    for level in range(levels):
        px, py = positions((h, w), flow, sign, level)
        ix, iy, wts = make_tap(px, py, quant)
        d = window_dots(f1, pyr[level], ix, iy, r)
        with np.errstate(all="ignore"):
            for ox in range(win):
                for oy in range(win):
                    v = blend4(d[:, :, oy, ox], d[:, :, oy, ox + 1], d[:, :, oy + 1, ox], d[:, :, oy + 1, ox + 1], wts) * scale
                    if order == "xy":
                        out[level, ox, oy] = v
                    else:
                        out[level, oy, ox] = v
    return out.reshape(levels * win * win, h, w)


def lookup_batch(f1, f2, flow=None, **kw):
    """f1, f2 (N, H, W, C); flow None, (H, W, 2) shared or (N, H, W, 2) -> (N, levels (2r + 1)^2, H, W)"""
    pick = lambda i: None if flow is None else (flow if flow.ndim == 3 else flow[i])
    return np.stack([lookup(f1[i], f2[i], pick(i), **kw) for i in range(f1.shape[0])])


# ---------------------------------------------------------------------------------------------- the float64 definition
def lookup64(f1, f2, flow=None, sign=1, radius=4, levels=1, scale=None, order="xy"):
    """all-pairs einsum, mean-pooling of the VOLUME, bilinear lookup with zeros outside, in float64 (QUANT_EXACT)"""
    f1, f2 = np.asarray(f1, np.float32), np.asarray(f2, np.float32)
    h, w, c = f1.shape
    r, win = radius, 2 * radius + 1
    scale = np.float64(default_scale(c) if scale is None else scale)            # a given scale is taken as it is, in float64
    vol = np.einsum("yxc,YXc->yxYX", f1.astype(np.float64), f2.astype(np.float64))
    out = np.empty((levels, win, win, h, w), np.float64)
    yi, xi = np.mgrid[:h, :w]
    for level in range(levels):
        if level:
            h2, w2 = vol.shape[2] >> 1, vol.shape[3] >> 1
            vol = vol[:, :, :2 * h2, :2 * w2].reshape(h, w, h2, 2, w2, 2).mean((3, 5))
        hl, wl = vol.shape[2:]
        px, py = (p.astype(np.float64) for p in positions((h, w), flow, sign, level))
        fx0, fy0 = np.floor(px), np.floor(py)
        ax, ay = px - fx0, py - fy0
        padded = np.zeros((h, w, hl + 2, wl + 2))
        padded[:, :, 1:-1, 1:-1] = vol

        def tap(yy, xx):
            yy, xx = np.clip(yy + 1, 0, hl + 1).astype(np.int64), np.clip(xx + 1, 0, wl + 1).astype(np.int64)
            return padded[yi, xi, yy, xx]

        for ox in range(win):
            for oy in range(win):
                x0, y0 = fx0 + (ox - r), fy0 + (oy - r)
                v = ((1 - ay) * ((1 - ax) * tap(y0, x0) + ax * tap(y0, x0 + 1))
                     + ay * ((1 - ax) * tap(y0 + 1, x0) + ax * tap(y0 + 1, x0 + 1))) * scale
                if order == "xy":
                    out[level, ox, oy] = v
                else:
                    out[level, oy, ox] = v
    return out.reshape(levels * win * win, h, w)


def magnitude(f1, f2):
    """M: the largest sum_c |f1_c f2_c| over all pixel pairs at level 0, in float64"""
    a = np.abs(np.asarray(f1, np.float32).astype(np.float64)).reshape(-1, f1.shape[-1])
    b = np.abs(np.asarray(f2, np.float32).astype(np.float64)).reshape(-1, f2.shape[-1])
    return float((a @ b.T).max())


def bound(c, levels):
    """k of the module docstring: the roundings on the longest path"""
    return 2 * (levels - 1) + 1 + (V * -(-c // (V * L)) - 1) + 4 + 3 + 4 + 1


# ---------------------------------------------------------------------------------------------- shared inputs
def features(shape, c, dtype, seed=0):
    """(H, W, C) as stored in `dtype`: ordinary magnitudes with exact zeros, -0.0 and sign changes sprinkled in"""
    rng = np.random.default_rng(5000 + seed + 31 * shape[0] + shape[1] + 7 * c)
    a = rng.standard_normal(shape + (c,)).astype(np.float32)
    z = rng.random(a.shape)
    a[z < 0.05] = 0.0
    a[z > 0.96] = -0.0
    return np.ascontiguousarray(R.from_f32(a, dtype))


def fields(shape, r):
    """name -> float32 (H, W, 2): the flows of the test list"""
    h, w = shape
    rng = np.random.default_rng(6000 + 31 * h + w + r)
    full = lambda u, v: np.broadcast_to(np.array([u, v], np.float32), (h, w, 2)).copy()
    out = {
        "zero": full(0.0, 0.0),
        "shift": full(2.0, -1.0),
        "random": ((rng.random((h, w, 2)) - 0.5) * 2 * (r + 3)).astype(np.float32),
        "outside": full(w + r + 3.0, -(h + r + 2.0)),
        "far": full(1e4, -1e4),
        "huge": full(3e38, -3e38),
    }
    # windows that straddle each border and each corner: every pixel is sent to one of the eight, with a fraction
    targets = np.array([(-0.5, -0.5), (w - 0.5, -0.5), (-0.5, h - 0.5), (w - 0.5, h - 0.5),
                        (w / 2, -0.25), (w / 2, h - 0.75), (-0.25, h / 2), (w - 0.75, h / 2)], np.float32)
    gy, gx = np.mgrid[:h, :w]
    t = targets[(gy * w + gx) % 8]
    out["borders"] = np.stack([t[..., 0] - gx, t[..., 1] - gy], -1).astype(np.float32)
    return out
