"""NumPy statement of K24 (oflibnumpy_amd/csrc/ofl_inverse_search.hip, include/ofl.h), of ofl_tensor_halve_dev and of the
coarse-to-fine loop of estimate_flow -- a helper of test_inverse_search_host.py and test_gpu_inverse_search.py, not a test.

census_ref.intensity gives A and Bm, the channel means of `near` and of the unwarped `far`.  In float32 every sample S(q, u)
comes from the oracle's bilinear gather of the plane Bm (its taps, weights and blend, as in refine_ref): the patches of the
grid overlap, so they are dealt to groups whose patches do not (patch_groups), and one gather per group samples every patch
of the group with its own vector; the clamp of the position to the frame is put into the vector handed to the gather
(an integer difference where it acts, so the gather's own coordinate is exactly 0 or W - 1).  Everything else is an
explicit NumPy operation in the order of the definition, vectorised over the patches, so the device result is compared
bit for bit:
    Ax = 0.5 (A(q + ex) - A(q - ex)), Ay likewise, a neighbour outside the frame replaced by q;  gx = sign Ax, gy = sign Ay
    origins 0, S, 2 S, ... <= n - P and n - P;  the tree sum adds x[2i] + x[2i + 1] level by level
    u0 = flow at (oy + P / 2, ox + P / 2) if fmask and finite, else +0;  T = A - (sum A) / PP (normalise) or A
    H11 = sum gx gx, H12 = sum gx gy, H22 = sum gy gy, det = H11 H22 - H12 H12
    r = (S - (sum S) / PP) - T;  best = ssd(u0) or +inf;  while det finite and > 0, `iterations` times:
        b1 = sum r gx, b2 = sum r gy;  du = (H22 b1 - H12 b2) / det, dv = (H11 b2 - H12 b1) / det;  u' = u - (du, dv)
        stop if u' is not finite or |u' - u0|^2 > PP;  u <- u';  r, ssd;  ssd < best: best <- ssd, ubest <- u
    densify: w_p = 1 / (d < floor ? floor : d), d = |S(q, u_p) - A(q)|, the patches of q in row-major order, sums from +0;
        out = (sum w u.x / sum w, sum w u.y / sum w), mask = both finite, else (+0, +0) and 0

`search` and `densify` take the arithmetic type and the sampler as arguments: float32 with the oracle's gather is the
definition; float64 is the same statement evaluated in double on the same float32 A, Bm and vectors with sample_numpy, a
NumPy bilinear sampler with exact taps (restate(..., dt=np.float64); test_inverse_search_host.py checks that sample_numpy
in float32 equals the oracle bit for bit).

float32 against float64 with exact taps from the zero field on the three known answers of KNOWN, measured with this file
(deterministic, CPU only): max |out32 - out64| = 5.87e-05, 8.84e-05 and 4.17e-04 px (MEASURED_32_64).  A patch whose two
runs STOP at different iterates would be excluded: the share is 0 in all three.  The difference is not rounding carried
through the steps: 6 %, 12 % and 25 % of the patches keep a different iterate as their best, because the last iterates of a
converged patch tie to within the rounding of their ssd, and those iterates lie some 1e-4 px apart.
test_inverse_search_host.py asserts 8 x the largest, BOUND_32_64 = 3.33e-03 px.  The end-point errors reached (float32):
0.07723, 0.03427 and 0.01943 px from 4.2012, 0.7211 and 6.4637."""
import functools

import numpy as np

import interop_ref as R
import tensor_ref as T
import photometric_ref as P
import census_ref as Cn
import refine_ref as Rf
from consistency_ref import smooth
from oracle import np_oracle as O

F32, F64 = np.float32, np.float64
DEFAULTS = dict(patch=8, stride=4, iterations=12, normalise=True, floor=1.0)
SHAPES = [(8, 8), (8, 21), (19, 70), (37, 131)]
SIGNS, QUANTS = P.SIGNS, P.QUANTS
in_layout = P.in_layout
wave_image = Rf.wave_image
# the known answers: (shape, true shift, levels, border, the zero field's EPE as the issue states it)
KNOWN = [((64, 96), (3.3, -2.6), 1, 8, 4.2012), ((64, 96), (0.6, -0.4), 1, 8, 0.7211), ((128, 192), (5.3, -3.7), 2, 16, 6.4637)]
# max |out32 - out64| in px of the three known answers, in the order of KNOWN (written by the measurement, see the docstring)
MEASURED_32_64 = (5.8719229844683696e-05, 8.840791995173847e-05, 4.1665197937401643e-04)
BOUND_32_64 = 8 * max(MEASURED_32_64)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ------------------------------------------------------------------------------------------------- the patch grid
def origins(n, patch, stride):
    """0, S, 2 S, ... <= n - P, then n - P if it is not the last of them"""
    out = [o for o in range(0, n, stride) if o <= n - patch]
    if out[-1] != n - patch:
        out.append(n - patch)
    return out


def patch_groups(org, patch):
    """the indices of `org` dealt to groups whose origins lie at least `patch` apart (greedy)"""
    groups = []
    for i, o in enumerate(org):
        for g in groups:
            if all(abs(o - org[j]) >= patch for j in g):
                g.append(i)
                break
        else:
            groups.append([i])
    return [np.array(g) for g in groups]


def tree_sum(v):
    """v (..., P, P) -> (...): the values in row-major patch order added pairwise, level by level"""
    x = v.reshape(v.shape[:-2] + (-1,))
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


# ------------------------------------------------------------------------------------------------- the two samplers
def sample_oracle(plane, U, oys, oxs, patch, sign, quant):
    """plane float32 (H, W); U float32 (ny, nx, 2), finite -> S float32 (ny, nx, P, P): the oracle's gather, one call per
    group of patches that do not overlap"""
    h, w = plane.shape
    ys, xs = np.mgrid[:h, :w]
    out = np.empty(U.shape[:2] + (patch, patch), F32)
    ar = np.arange(patch)
    for gy in patch_groups(oys, patch):
        rows = (np.asarray(oys)[gy][:, None] + ar)[:, None, :, None]                   # (gy, 1, P, 1)
        for gx in patch_groups(oxs, patch):
            cols = (np.asarray(oxs)[gx][:, None] + ar)[None, :, None, :]               # (1, gx, 1, P)
            f = np.zeros((h, w, 2), F32)
            f[rows, cols] = U[gy][:, gx][:, :, None, None, :]
            # the clamp of the position, expressed in the vector: an integer difference, exact in the gather's float64 sum
            px = (xs + sign * f[..., 0].astype(F64)).astype(F32)
            py = (ys + sign * f[..., 1].astype(F64)).astype(F32)
            f[..., 0] = np.where(px < 0, sign * (0 - xs), np.where(px > w - 1, sign * (w - 1 - xs), f[..., 0]))
            f[..., 1] = np.where(py < 0, sign * (0 - ys), np.where(py > h - 1, sign * (h - 1 - ys), f[..., 1]))
            g = O.gather_bilinear(plane, f, sign, quant=quant)
            out[gy[:, None], gx[None, :]] = g[rows, cols]
    return out


def sample_numpy(plane, U, oys, oxs, patch, sign, dt):
    """the same with exact taps, written out in NumPy in the type dt: position = q + sign u (float32: rounded once from the
    float64 sum, K12's map_coord), clamped; fx = p - floor(p); weights (1 - fy)(1 - fx), (1 - fy) fx, fy (1 - fx), fy fx;
    a tap at column W or row H counts as +0"""
    h, w = plane.shape
    ar = np.arange(patch)
    X = (np.asarray(oxs)[None, :, None, None] + ar[None, None, None, :]).astype(F64)
    Y = (np.asarray(oys)[:, None, None, None] + ar[None, None, :, None]).astype(F64)
    with np.errstate(all='ignore'):
        px = np.clip((X + sign * U[..., 0].astype(F64)[..., None, None]).astype(dt), dt(0), dt(w - 1))
        py = np.clip((Y + sign * U[..., 1].astype(F64)[..., None, None]).astype(dt), dt(0), dt(h - 1))
        flx, fly = np.floor(px), np.floor(py)
        fx, fy = px - flx, py - fly
        ix, iy = flx.astype(int), fly.astype(int)
        x0, y0 = dt(1) - fx, dt(1) - fy
        pl = np.pad(plane.astype(dt), ((0, 1), (0, 1)))                                 # column W and row H: +0
        s = pl[iy, ix] * (y0 * x0)
        s = s + pl[iy, ix + 1] * (y0 * fx)
        s = s + pl[iy + 1, ix] * (fy * x0)
        s = s + pl[iy + 1, ix + 1] * (fy * fx)
    assert s.dtype == dt
    return s


def make_sampler(plane, oys, oxs, patch, sign, quant, dt):
    if dt == F32:
        return lambda U: sample_oracle(plane, np.ascontiguousarray(U, F32), oys, oxs, patch, sign, quant)
    assert quant == O.QUANT_EXACT, "the float64 statement has exact taps only"
    return lambda U: sample_numpy(plane, U, oys, oxs, patch, sign, dt)


# ------------------------------------------------------------------------------------------------- search and densify
def search(A, sample, u0, oys, oxs, patch, sign, iterations, normalise, dt=F32):
    """A float32 (H, W); sample: U (ny, nx, 2) -> S (ny, nx, P, P) in dt; u0 (ny, nx, 2) -> dict(vecs (ny, nx, 2), ssd (ny, nx)
    in dt, kbest, steps int (ny, nx): the iterate that won (0: u0) and the iterations taken)"""
    pp = patch * patch
    inv, far, half = dt(1.0 / pp), dt(pp), dt(0.5)
    ar = np.arange(patch)
    rows = (np.asarray(oys)[:, None] + ar)[:, None, :, None]
    cols = (np.asarray(oxs)[:, None] + ar)[None, :, None, :]
    with np.errstate(all='ignore'):
        Ad = A.astype(dt)
        Ap = np.pad(Ad, 1, mode='edge')
        Ax, Ay = half * (Ap[1:-1, 2:] - Ap[1:-1, :-2]), half * (Ap[2:, 1:-1] - Ap[:-2, 1:-1])
        gx, gy = ((Ax, Ay) if sign > 0 else (-Ax, -Ay))
        gx, gy, Ac = gx[rows, cols], gy[rows, cols], Ad[rows, cols]
        Tm = Ac - (tree_sum(Ac) * inv)[..., None, None] if normalise else Ac
        H11, H12, H22 = tree_sum(gx * gx), tree_sum(gx * gy), tree_sum(gy * gy)
        det = H11 * H22 - H12 * H12

        def residual(U):
            s = sample(U)
            if normalise:
                s = s - (tree_sum(s) * inv)[..., None, None]
            r = s - Tm
            return r, tree_sum(r * r)

        u0 = u0.astype(dt)
        u, ubest = u0.copy(), u0.copy()
        r, best = residual(u)
        best = np.where(np.isfinite(best), best, dt(np.inf))
        searching = np.isfinite(det) & (det > 0)
        kbest, steps = np.zeros(det.shape, int), np.zeros(det.shape, int)
        for it in range(iterations):
            if not searching.any():
                break
            b1, b2 = tree_sum(r * gx), tree_sum(r * gy)
            du, dv = (H22 * b1 - H12 * b2) / det, (H11 * b2 - H12 * b1) / det
            un = np.stack([u[..., 0] - du, u[..., 1] - dv], axis=-1)
            e = un - u0
            d2 = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]
            searching = searching & np.isfinite(un).all(axis=-1) & ~(d2 > far)
            u = np.where(searching[..., None], un, u)
            rn, ssd = residual(u)
            r = np.where(searching[..., None, None], rn, r)
            win = searching & (ssd < best)
            best, ubest = np.where(win, ssd, best), np.where(win[..., None], u, ubest)
            kbest, steps = np.where(win, it + 1, kbest), np.where(searching, it + 1, steps)
        assert ubest.dtype == dt and best.dtype == dt
    return dict(vecs=ubest, ssd=best, kbest=kbest, steps=steps)


def densify(A, sample, pv, oys, oxs, patch, floor, dt=F32):
    """-> (out (H, W, 2) in dt, mask bool (H, W)): the patches in row-major grid order, every sum from +0"""
    h, w = A.shape
    floor = dt(floor)
    with np.errstate(all='ignore'):
        Ad = A.astype(dt)
        s = sample(pv)
        sw, sx, sy = np.zeros((h, w), dt), np.zeros((h, w), dt), np.zeros((h, w), dt)
        for iy, oy in enumerate(oys):
            for ix, ox in enumerate(oxs):
                win = (slice(oy, oy + patch), slice(ox, ox + patch))
                d = np.abs(s[iy, ix] - Ad[win])
                wgt = dt(1) / np.where(d < floor, floor, d)
                sw[win] = sw[win] + wgt
                sx[win] = sx[win] + wgt * pv[iy, ix, 0]
                sy[win] = sy[win] + wgt * pv[iy, ix, 1]
        out = np.stack([sx / sw, sy / sw], axis=-1)
        ok = np.isfinite(out).all(axis=-1)
        out = np.where(ok[..., None], out, dt(0))
    assert out.dtype == dt
    return out, ok


def restate(near_p, far_p, vecs, fmask, sign, quant=O.QUANT_EXACT, dt=F32, **kw):
    """near_p, far_p: float32 (N, C, H, W), the tensors widened; vecs (H, W, 2) or (N, H, W, 2) or None (the zero field),
    fmask (H, W) or (N, H, W) or None (all set); kw: the parameters that differ from DEFAULTS -> dict(vecs (N, H, W, 2) of
    type dt, mask bool (N, H, W), patch_vecs (N, ny, nx, 2), patch_ssd (N, ny, nx) of type dt, kbest, steps, u0, grid)"""
    p = dict(DEFAULTS, **kw)
    patch, stride = p['patch'], p['stride']
    near_p = np.ascontiguousarray(near_p, F32)
    n, c, h, w = near_p.shape
    oys, oxs = origins(h, patch, stride), origins(w, patch, stride)
    cy, cx = np.array(oys) + patch // 2, np.array(oxs) + patch // 2
    with np.errstate(all='ignore'):
        A, B = Cn.intensity(near_p), Cn.intensity(np.ascontiguousarray(far_p, F32))
    res = dict(vecs=[], mask=[], patch_vecs=[], patch_ssd=[], kbest=[], steps=[], u0=[])
    for i in range(n):
        u0 = np.zeros((len(oys), len(oxs), 2), F32)
        if vecs is not None:
            f = np.broadcast_to(np.asarray(vecs, F32), (n, h, w, 2))[i][cy[:, None], cx[None, :]]
            ok = np.isfinite(f).all(axis=-1)
            if fmask is not None:
                ok &= np.broadcast_to(np.asarray(fmask), (n, h, w))[i].astype(bool)[cy[:, None], cx[None, :]]
            u0 = np.where(ok[..., None], f, F32(0)).astype(F32)
        sample = make_sampler(B[i], oys, oxs, patch, sign, quant, dt)
        s = search(A[i], sample, u0, oys, oxs, patch, sign, p['iterations'], p['normalise'], dt)
        out, mask = densify(A[i], sample, s['vecs'], oys, oxs, patch, F32(p['floor']), dt)
        for key, val in (('vecs', out), ('mask', mask), ('patch_vecs', s['vecs']), ('patch_ssd', s['ssd']), ('kbest', s['kbest']),
                         ('steps', s['steps']), ('u0', u0)):
            res[key].append(val)
    res = {k: np.stack(v) for k, v in res.items()}
    res['grid'] = (len(oys), len(oxs))
    return res


def inverse_search(near, far, dtype, layout, vecs, fmask, sign, **kw):
    """restate() for arrays in the memory order of `layout` and of `dtype` (bfloat16: uint16 patterns), 3 or 4 dimensions"""
    return restate(R.to_f32(T.to_planar(near, layout), dtype), R.to_f32(T.to_planar(far, layout), dtype), vecs, fmask, sign, **kw)


# ------------------------------------------------------------------------------------------------- halve and the pyramid
def halve(planar, dtype='float32'):
    """planar (..., H, W) as stored in `dtype` -> (..., H // 2, W // 2) as stored: ((tl + tr) + (bl + br)) * 0.25 in float32,
    rounded once; an odd last row or column is dropped"""
    a = R.to_f32(planar, dtype)
    h, w = a.shape[-2] // 2 * 2, a.shape[-1] // 2 * 2
    with np.errstate(all='ignore'):
        m = ((a[..., 0:h:2, 0:w:2] + a[..., 0:h:2, 1:w:2]) + (a[..., 1:h:2, 0:w:2] + a[..., 1:h:2, 1:w:2])) * F32(0.25)
    assert m.dtype == F32
    return np.ascontiguousarray(m) if dtype == 'float32' else R.from_f32(m, dtype)


def estimate(near_p, far_p, sign, levels, refine=False, dt=F32, **kw):
    """estimate_flow's loop on float32 planar images (1, C, H, W) from the zero field: halve, per level restate() and, with
    `refine`, refine_ref.restate at its defaults (float32 only), then the oracle's resize by 2 (a float32 step in the float64
    run too) -> dict(vecs (H, W, 2) of type dt, mask (H, W), excluded: the share of patches, over all levels, whose float32
    iterate this run cannot vouch for -- filled in by compare_32_64)"""
    pyramid = [(np.ascontiguousarray(near_p, F32), np.ascontiguousarray(far_p, F32))]
    for _ in range(levels - 1):
        pyramid.append((halve(pyramid[-1][0]), halve(pyramid[-1][1])))
    vecs, mask, runs = None, None, []
    for level in range(levels - 1, -1, -1):
        a, b = pyramid[level]
        r = restate(a, b, vecs, mask, sign, dt=dt, **kw)
        vecs, mask = r['vecs'][0], r['mask'][0]
        runs.append(r)
        if refine:
            assert dt == F32
            vecs = Rf.restate(a, b, vecs, mask, sign)['vecs'][0]
        if level:
            vecs, mask = O.resize_flow(vecs.astype(F32), 2, mask)
    return dict(vecs=vecs, mask=mask, runs=runs)


# ------------------------------------------------------------------------------------------------- the known answers
def shifted_pair(shape, v):
    """near = I, far = I shifted by v, sampled analytically: far(q + v) = I(q) -> (near, far) float32 (1, 1, h, w); the field
    that explains them is v everywhere with reference 's'"""
    ys, xs = np.mgrid[:shape[0], :shape[1]].astype(F64)
    return wave_image(xs, ys).astype(F32)[None, None], wave_image(xs - v[0], ys - v[1]).astype(F32)[None, None]


def epe(vecs, v, border):
    """mean end-point error against v over the pixels at least `border` from the frame"""
    d = np.asarray(vecs, F64)[..., border:-border, border:-border, :] - np.array(v)
    return float(np.sqrt((d * d).sum(axis=-1)).mean())


@functools.lru_cache(maxsize=None)
def known(i, dt=F32):
    """known answer i of KNOWN, from the zero field with exact taps and without refinement, computed once"""
    shape, v, levels, border, zero = KNOWN[i]
    near, far = shifted_pair(shape, v)
    out = estimate(near, far, 1, levels, dt=dt)
    out['epe'] = epe(out['vecs'], v, border)
    return out


def compare_32_64(i):
    """-> (max |out32 - out64| in px over all pixels, the share of patches, over all levels, whose two runs stopped at
    different iterates -- they would be excluded; there are none --, the share whose two runs kept a different iterate as
    the best: a converged patch's last iterates tie to within rounding, and which of them wins is what the difference
    consists of)"""
    a, b = known(i, F32), known(i, F64)
    total = sum(ra['kbest'].size for ra in a['runs'])
    stopped = sum(int((ra['steps'] != rb['steps']).sum()) for ra, rb in zip(a['runs'], b['runs']))
    other_best = sum(int((ra['kbest'] != rb['kbest']).sum()) for ra, rb in zip(a['runs'], b['runs']))
    return float(np.abs(a['vecs'].astype(F64) - b['vecs']).max()), stopped / total, other_best / total


# ------------------------------------------------------------------------------------------------- the input generator
@functools.lru_cache(maxsize=None)
def case(seed, shape, sign, quant, c, dtype='float32', n=1, init=True, params=()):
    """One generated case, computed once and shared, read-only: dict(near, far: planar (n, c, h, w) as stored in `dtype`
    (refine_ref.images: far smooth, near = far gathered along a field plus half a pixel); f (n, h, w, 2): that field plus a
    smooth disturbance of about a pixel, fm (n, h, w) with refine_ref.holes(), or None, None without `init`; kw: dict(params);
    want: restate()'s dict)."""
    h, w = shape
    rng = np.random.default_rng([seed, h, w, c])
    true = np.stack([smooth(rng, h, w, 3.0) for _ in range(n)])
    near, far = Rf.images(rng, c, true, sign, dtype)
    f = fm = None
    if init:
        f = (true + np.stack([smooth(rng, h, w, 1.0) for _ in range(n)])).astype(F32)
        fm = np.stack([np.roll(Rf.holes(shape), i, axis=1) for i in range(n)])
    kw = dict(params)
    want = restate(R.to_f32(near, dtype), R.to_f32(far, dtype), f, fm, sign, quant=quant, **kw)
    out = dict(near=near, far=far, f=f, fm=fm, kw=kw, want=want)
    for a in (near, far, f, fm) + tuple(v for v in want.values() if isinstance(v, np.ndarray)):
        if a is not None:
            a.flags.writeable = False
    return out
