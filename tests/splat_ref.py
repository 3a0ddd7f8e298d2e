"""K20 restated in NumPy (the definition of include/ofl.h), plus the inputs the tests of the splat share.

`splat` repeats the kernels operation for operation: the float32 operations in the stated order (every array operation
below rounds once, nothing is fused), np.maximum.at on the int32 keys for the per-target softmax shift, np.add.at on int64
for the fixed-point sums, upsample_ref.exp32 for the exponential.  Integer sums and maxima do not depend on their order, so
the device result is compared with it byte for byte.  `splat64` is the same definition in float64 with np.exp, without the
-87 cut-off and without fixed point; the landing position px = float32(x + u), py, the fractions fx = float32(px - x0), fy (a rounded
difference where the landing is negative) and zs = float32(alpha * z) are inputs of the definition and are taken as `splat`
forms them.

The error bound of `splat` against `splat64` for one target pixel.  eps = 2^-24 is the unit round-off of float32, E the
relative error of exp32 in units of eps (2: include/ofl.h, measured in tests/test_upsample_host.py), K the number of taps
that land on the pixel, F = frac_bits.  Tap i carries the exact weight o_i = w_i e_i (e_i = exp(t_i), t_i = zs_i - zmax <= 0,
relative to the pixel's own maximum, so the largest e is 1) and the value I_i; a = sum o_i I_i, d = sum o_i, out = a / d.
    1 - fx, 1 - fy       one rounding each, the results are at most 1                          2 eps   relative to w_i
    w_i                  the product                                                           1 eps
    t_i                  the rounded difference changes e_i by the factor exp(t_i eta)         |t_i| eps   (softmax)
    exp32                                                                                      E eps       (softmax)
    we_i = w_i e_i       the product (exact when e_i = 1)                                      1 eps
so the float32 weight is o_i (1 + r_i) with |r_i| <= rho_i = (4 + E + |t_i|) eps (4 eps without importance), and the
product val_i = we_i I_i adds one more eps.  Rounding to fixed point moves every weight add by at most 2^-33 and every
value add by at most 2^-(F + 1).  With A, D the sums the restatement holds, as real numbers,
    |A - a| <= sum o_i |I_i| (rho_i + eps) + K 2^-(F + 1)          |D - d| <= sum o_i rho_i + K 2^-33
    A / D - a / d = (A - a) / D - (a / d) (D - d) / D              (an identity)
and the final rounding to float32 adds eps |out| (the float64 operations of the last pass are 2^-29 of that).  Hence
    AVERAGE, SOFTMAX:  |splat - splat64| <= 1.01 (|A - a|max + |a / d| |D - d|max) / D + eps |out|
    SUM:               |splat - splat64| <= 1.01 |A - a|max + eps |out|
where 1.01 covers the products of two of the first-order terms above (each below 100 eps).  The bound is evaluated per
pixel from the landings themselves (`bound`); the inputs of the tests are of ordinary magnitude, no term is subnormal.
`valid` compares D with a threshold, so a pixel whose d lies within |D - d|max of min_weight may differ and is left out."""
import numpy as np

import upsample_ref
from upsample_ref import exp32, bf16_bits, widen, to_layout     # noqa: F401  (shared with the tests)

EPS = 2.0 ** -24
EXP_ERR = 2.0                      # relative error of exp32 in units of EPS
CUT = np.float32(-87.0)
MODES = ("sum", "average", "softmax")
KEY_MIN = np.int32(-2 ** 31)
F32 = np.float32


def float_key(f):
    """the order-preserving int32 key of float32 values that are not NaN; the map is its own inverse"""
    b = np.ascontiguousarray(f, F32).view(np.int32)
    return b ^ ((b >> np.int32(31)) & np.int32(0x7FFFFFFF))


def key_float(k):
    k = np.ascontiguousarray(k, np.int32)
    return (k ^ ((k >> np.int32(31)) & np.int32(0x7FFFFFFF))).view(F32)


class Landings:
    """steps 1 and 2 for one field: per existing tap the source pixel `s`, the target pixel `q`, the bilinear weight `w`
    (float32) and, with an importance, `zs`; `skipped` counts the source pixels that contribute nothing"""

    def __init__(self, v, m, z=None, alpha=1.0):
        v = np.asarray(v, F32)
        h, w = v.shape[:2]
        gy, gx = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing="ij")
        with np.errstate(all="ignore"):
            u, vv = v[..., 0], v[..., 1]
            px, py = gx + u, gy + vv
            ok = (np.asarray(m) != 0) & np.isfinite(u) & np.isfinite(vv) & (np.abs(px) < F32(2.0 ** 30)) & (np.abs(py) < F32(2.0 ** 30))
            zs = None
            if z is not None:
                zs = F32(alpha) * np.asarray(z, F32)
                ok &= np.isfinite(zs)
            assert px.dtype == F32
            px, py = np.where(ok, px, F32(0)), np.where(ok, py, F32(0))
            x0, y0 = np.floor(px), np.floor(py)
            fx, fy = px - x0, py - y0
            hx, hy = F32(1) - fx, F32(1) - fy
            wk = [hx * hy, fx * hy, hx * fy, fx * fy]
        ix, iy = x0.astype(np.int64), y0.astype(np.int64)
        self.shape, self.skipped = (h, w), int((~ok).sum())
        src = np.arange(h * w).reshape(h, w)
        s, q, ws, zz, fxs, fys, ks = [], [], [], [], [], [], []
        for k in range(4):
            tx, ty = ix + (k & 1), iy + (k >> 1)
            ex = ok & (wk[k] != 0) & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
            s.append(src[ex]); q.append((ty * w + tx)[ex]); ws.append(wk[k][ex])
            fxs.append(fx[ex]); fys.append(fy[ex]); ks.append(np.full(int(ex.sum()), k))
            if zs is not None:
                zz.append(zs[ex])
        self.s, self.q, self.w = np.concatenate(s), np.concatenate(q), np.concatenate(ws).astype(F32)
        self.fx, self.fy, self.k = np.concatenate(fxs), np.concatenate(fys), np.concatenate(ks)
        self.zs = np.concatenate(zz).astype(F32) if zs is not None else None

    def factors(self):
        """step 3 -> (e float32 per tap, t float32 per tap or None)"""
        if self.zs is None:
            return np.ones(self.w.shape, F32), None
        zmax = np.full(self.shape[0] * self.shape[1], KEY_MIN, np.int32)
        np.maximum.at(zmax, self.q, float_key(self.zs))
        with np.errstate(all="ignore"):
            t = self.zs - key_float(zmax)[self.q]
            assert t.dtype == F32
            e = np.where(t < CUT, F32(0), exp32(np.where(t < CUT, F32(0), t)))
        return e.astype(F32), t


def _fields(v, m, z, n, shared):
    v, m = np.asarray(v, F32), np.asarray(m)
    if shared:
        return [(v.reshape(v.shape[-3:]), m.reshape(m.shape[-2:]), None if z is None else np.asarray(z, F32).reshape(m.shape[-2:]))]
    assert v.shape[0] == n
    return [(v[i], m[i], None if z is None else np.asarray(z, F32)[i]) for i in range(n)]


def splat(src, v, m, mode, z=None, alpha=1.0, frac_bits=24, min_weight=2.0 ** -10, shared=True):
    """src: float32 (N, C, H, W), the tensor widened to float32 (C may be 0); v, m[, z]: ONE field (H, W, 2), (H, W) when
    `shared`, else N of them.  -> dict(out float32 (N, C, H, W) before the rounding to storage, valid uint8 and weight
    float32 (H, W) or (N, H, W), counters uint32 (2,), acc / den the int64 sums)"""
    assert mode in MODES and (z is not None) == (mode == "softmax")
    src = np.asarray(src, F32)
    n, c, h, w = src.shape
    hw = h * w
    acc, den = np.zeros((n, c, hw), np.int64), np.zeros((n, hw), np.int64)
    skipped = dropped = 0
    fields = _fields(v, m, z, n, shared)
    for f, (fv, fm, fz) in enumerate(fields):
        ld = Landings(fv, fm, fz, alpha)
        skipped += ld.skipped
        e, _ = ld.factors()
        with np.errstate(all="ignore"):
            we = ld.w * e
            assert we.dtype == F32
            dq = np.rint(we.astype(np.float64) * 2.0 ** 32).astype(np.int64)
            for i in (range(n) if shared else [f]):
                np.add.at(den[i], ld.q, dq)
                if c:
                    val = we[None, :] * src[i].reshape(c, hw)[:, ld.s]
                    assert val.dtype == F32
                    d = val.astype(np.float64) * 2.0 ** frac_bits
                    bad = ~(np.abs(d) < 2.0 ** 62)
                    dropped += int(bad.sum())
                    aq = np.rint(np.where(bad, 0.0, d)).astype(np.int64)
                    np.add.at(acc[i], (np.arange(c)[:, None], ld.q[None, :]), aq)
    thr = int(np.rint(np.float64(F32(min_weight)) * 2.0 ** 32))
    with np.errstate(all="ignore"):
        dd, aa = den.astype(np.float64), acc.astype(np.float64)
        weight = (dd * 2.0 ** -32).astype(F32)
        valid = den >= thr
        if mode == "sum":
            out = (aa * 2.0 ** -frac_bits).astype(F32)
        else:
            out = np.where(valid[:, None, :], ((aa / dd[:, None, :]) * 2.0 ** (32 - frac_bits)).astype(F32), F32(0))
    planes = slice(0, 1) if shared else slice(None)
    shape = (h, w) if shared else (n, h, w)
    return dict(out=out.reshape(n, c, h, w), valid=valid[planes].astype(np.uint8).reshape(shape), weight=weight[planes].reshape(shape),
                counters=np.array([skipped, dropped], np.uint32), acc=acc, den=den)


def splat64(src, v, m, mode, z=None, alpha=1.0, frac_bits=24):
    """the definition in float64 for ONE field and src (C, H, W) -> (out float64 (C, H, W), d float64 (H, W), bound float64
    (C, H, W)): out is a / d for 'average' and 'softmax' (nan where d = 0) and a for 'sum'; `bound` is the bound of the module
    docstring on |splat - out|, without its last term eps |out| and with D taken as d - |D - d|max"""
    src = np.asarray(src, np.float64)
    c, h, w = src.shape
    hw = h * w
    ld = Landings(v, m, z, alpha)
    fx, fy = ld.fx.astype(np.float64), ld.fy.astype(np.float64)
    wx, wy = np.where(ld.k & 1, fx, 1 - fx), np.where(ld.k >> 1, fy, 1 - fy)
    o, rho = wx * wy, np.full(ld.q.shape, 4 * EPS)
    if ld.zs is not None:
        zmax = np.full(hw, -np.inf)
        np.maximum.at(zmax, ld.q, ld.zs.astype(np.float64))
        t = ld.zs.astype(np.float64) - zmax[ld.q]
        o, rho = o * np.exp(t), (4 + EXP_ERR + np.abs(t)) * EPS
    vals = src.reshape(c, hw)[:, ld.s]
    a, d, ea, ed, k = np.zeros((c, hw)), np.zeros(hw), np.zeros((c, hw)), np.zeros(hw), np.zeros(hw)
    rows = (np.arange(c)[:, None], ld.q[None, :])
    np.add.at(a, rows, o * vals)
    np.add.at(ea, rows, o * np.abs(vals) * (rho + EPS))
    np.add.at(d, ld.q, o)
    np.add.at(ed, ld.q, o * rho)
    np.add.at(k, ld.q, 1.0)
    ea, ed = ea + k * 2.0 ** -(frac_bits + 1), ed + k * 2.0 ** -33
    with np.errstate(all="ignore"):
        if mode == "sum":
            out, bound = a, 1.01 * ea
        else:
            out = a / d
            bound = 1.01 * (ea + np.abs(out) * ed) / (d - ed)
    return out.reshape(c, h, w), d.reshape(h, w), bound.reshape(c, h, w)


def stored(out, elem):
    """float32 results -> the array as the device stores it: float32, float16, or the uint16 bit patterns of bfloat16
    (ofl_export_flow_dev's rounding: to nearest even, overflow to +-inf)"""
    out = np.asarray(out, F32)
    if elem == "float32":
        return out
    with np.errstate(over="ignore"):
        return bf16_bits(out) if elem == "bfloat16" else out.astype(np.float16)


# ---------------------------------------------------------------------------------------------- shared inputs
def tensor(n, c, shape, seed=0, integers=False):
    """float32 (n, c, h, w) of ordinary magnitude with exact zeros; integers: small integer values"""
    rng = np.random.default_rng(500 + seed + 31 * shape[0] + shape[1] + 7 * c + n)
    if integers:
        return rng.integers(-40, 41, (n, c) + shape).astype(F32)
    t = (rng.standard_normal((n, c) + shape) * 3).astype(F32)
    t[rng.random(t.shape) < 0.05] = 0.0
    return t


def as_stored(t, elem):
    """a float32 tensor -> (the array as stored, its exact float32 widening): `elem` as in `stored`"""
    s = stored(t, elem)
    return s, widen(s, elem == "bfloat16")


def smooth_field(shape, seed=0, amp=3.0):
    """a field of a few pixels that varies slowly, with holes in the mask"""
    h, w = shape
    rng = np.random.default_rng(700 + seed + 31 * h + w)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    a, b, p, q = rng.random(4) * 2 + 0.5
    v = np.stack([amp * np.sin(xx / (3.0 * a) + yy / (5.0 * b) + p), amp * np.cos(xx / (4.0 * b) - yy / (3.5 * a) + q)], -1).astype(F32)
    m = (rng.random(shape) < 0.9).astype(np.uint8)
    return v, m


def random_field(shape, seed=0, amp=4.0):
    rng = np.random.default_rng(900 + seed + 31 * shape[0] + shape[1])
    v = (rng.standard_normal(shape + (2,)) * amp).astype(F32)
    m = (rng.random(shape) < 0.85).astype(np.uint8)
    return v, m


def constant_field(shape, dx, dy):
    v = np.empty(shape + (2,), F32)
    v[..., 0], v[..., 1] = dx, dy
    return v, np.ones(shape, np.uint8)


def importance(shape, seed=0, spread=20.0):
    rng = np.random.default_rng(1100 + seed + 31 * shape[0] + shape[1])
    return ((rng.random(shape) - 0.5) * spread).astype(F32)


def locality_case(shape, seed=0):
    """(v, m, z): a random sub-pixel field whose left half has z about -1000 and whose right half has z about 0"""
    h, w = shape
    rng = np.random.default_rng(1300 + seed + 31 * h + w)
    v = ((rng.random(shape + (2,)) - 0.5) * 1.5).astype(F32)
    z = (rng.standard_normal(shape) * 2).astype(F32)
    z[:, : w // 2] -= F32(1000)
    return v, np.ones(shape, np.uint8), z
