"""NumPy statement of K23 (oflibnumpy_amd/csrc/ofl_refine.hip, include/ofl.h) on top of photometric_ref and census_ref -- a
helper of test_refine_host.py and test_gpu_refine.py, not a test.

photometric_ref.restate gives the warped values w_c (the oracle's bilinear gather, one call per channel plane) and cov1,
K21's `covered`; census_ref.intensity gives A and B.  Everything after that is an explicit NumPy operation in the order of
the definition, vectorised over the pixels of one colour, so the device result is compared bit for bit.  Sums are left to
right; the neighbours are taken in the order up, left, right, down:
    dom = fmask & valid & isfinite(u) & isfinite(v)
    Bx = 0.5 (B(q + ex) - B(q - ex)), By likewise, a neighbour outside the frame replaced by q;  gx = sign Bx, gy = sign By
    Iz = B - A;  n = gx gx + gy gy + zeta2;  data = dom & cov1 & cov1 at the in-frame 4-neighbours & isfinite(gx, gy, Iz)
  each fixed-point iteration, from the current d (initially +0):
    r = Iz + gx du + gy dv;  wD = data ? delta / (n sqrt((r r) / n + eps2)) : +0
    p = wD gx, q = wD gy;  A11 = p gx, A12 = p gy, A22 = q gy, b1 = -(p Iz), b2 = -(q Iz)
    U = u + du, V = v + dv;  Ux = 0.5 (U(q + ex) - U(q - ex)) ..., a neighbour outside the frame or the domain replaced by q
    s = alpha / sqrt(Ux Ux + Uy Uy + Vx Vx + Vy Vy + eps2);  w_k = neighbour k ? 0.5 (s + s_k) : +0;  sigma = +0 + w_0 + ... + w_3
  each sweep, colour (x + y) & 1 = 0 then 1, on the domain pixels of that colour:
    t_k = neighbour k ? w_k ((u_k + du_k) - u) : +0;  du* = (b1 - A12 dv + t_0 + ... + t_3) / (A11 + sigma)
    du_new = du + omega (du* - du);  ok_u = (A11 + sigma != 0) & isfinite(du_new)
    dv* = (b2 - A12 (ok_u ? du* : du) + ...) / (A22 + sigma);  dv_new, ok_v likewise;  du, dv <- the new values where ok
  out = dom ? (du != 0 ? u + du : u, dv != 0 ? v + dv : v) : the input bits

`solve` takes the arithmetic type as an argument: float32 is the definition, float64 the same statement evaluated in double
on the same float32 A, B, cov1 and vectors (restate(..., dt=np.float64)).
float32 against float64 at the defaults, max |out32 - out64| in px, measured with this file (deterministic, CPU only):
    the zero field on the shifted pair of shifted_pair(), calls 1, 2, 3 (each re-warps the float32 result):
        3.60e-07, 1.94e-07, 1.39e-07
    case(1, (37, 131), 1, QUANT_OPENCV, 3): a 3 px field whose mask has holes, moved by 0.9 px in the median: 3.80e-06
test_refine_host.py asserts 8 x the largest of these, BOUND_32_64 = 3.04e-05 px: the margin is for NumPy builds that order sqrt and
divide identically but differ in nothing else."""
import functools

import numpy as np

import interop_ref as R
import tensor_ref as T
import photometric_ref as P
import census_ref as Cn
from consistency_ref import smooth
from oracle import np_oracle as O

F32, F64 = np.float32, np.float64
DEFAULTS = dict(alpha=20.0, delta=5.0, zeta=0.1, eps=0.1, fixed_point=5, sor=5, omega=1.6)
SHAPES = [(19, 70), (37, 131), (64, 256)]
TINY = [(1, 1), (1, 5), (5, 1), (2, 2)]
SIGNS, QUANTS = P.SIGNS, P.QUANTS
NEIGHBOURS = [(-1, 0), (0, -1), (0, 1), (1, 0)]          # (dy, dx): up, left, right, down
UP, LEFT, RIGHT, DOWN = 0, 1, 2, 3
MEASURED_32_64 = 3.7976045117460444e-06
BOUND_32_64 = 8 * MEASURED_32_64
same_floats = P.same_floats
in_layout = P.in_layout
shifted = Cn.shifted


def settings(**kw):
    """the seven parameters as the ABI takes them: float32 and int, defaults where absent"""
    p = dict(DEFAULTS, **kw)
    return dict(alpha=F32(p['alpha']), delta=F32(p['delta']), zeta=F32(p['zeta']), eps=F32(p['eps']),
                fixed_point=int(p['fixed_point']), sor=int(p['sor']), omega=F32(p['omega']))


def solve(A, B, cov1, vecs, dom, sign, prm, dt=F32):
    """A, B float32 (N, H, W); cov1, dom bool (N, H, W); vecs float32 (N, H, W, 2); prm: settings() -> (out (N, H, W, 2) of
    type dt, data bool (N, H, W)); every operation in dt"""
    alpha, delta, omega = dt(prm['alpha']), dt(prm['delta']), dt(prm['omega'])
    zeta2, eps2 = dt(prm['zeta'] * prm['zeta']), dt(prm['eps'] * prm['eps'])          # float32 products, as on the device
    half, zero = dt(0.5), dt(0)
    A, B, u, v = A.astype(dt), B.astype(dt), vecs[..., 0].astype(dt), vecs[..., 1].astype(dt)
    inside = [shifted(np.ones(A.shape, bool), dy, dx, False) for dy, dx in NEIGHBOURS]
    nb = [inside[k] & shifted(dom, dy, dx, False) for k, (dy, dx) in enumerate(NEIGHBOURS)]
    at = lambda a, k: shifted(a, NEIGHBOURS[k][0], NEIGHBOURS[k][1], zero)
    ys, xs = np.mgrid[:A.shape[1], :A.shape[2]]
    with np.errstate(all='ignore'):
        Bn = [np.where(inside[k], at(B, k), B) for k in range(4)]
        Bx, By = half * (Bn[RIGHT] - Bn[LEFT]), half * (Bn[DOWN] - Bn[UP])
        gx, gy = (Bx, By) if sign > 0 else (-Bx, -By)
        Iz = B - A
        n = (gx * gx + gy * gy) + zeta2
        data = dom & cov1 & np.isfinite(gx) & np.isfinite(gy) & np.isfinite(Iz)
        for k, (dy, dx) in enumerate(NEIGHBOURS):
            data &= ~inside[k] | shifted(cov1, dy, dx, False)
        du, dv = np.zeros(A.shape, dt), np.zeros(A.shape, dt)
        for _ in range(prm['fixed_point']):
            r = (Iz + gx * du) + gy * dv
            wD = np.where(data, delta / (n * np.sqrt((r * r) / n + eps2)), zero)
            p, q = wD * gx, wD * gy
            A11, A12, A22, b1, b2 = p * gx, p * gy, q * gy, -(p * Iz), -(q * Iz)
            U, V = u + du, v + dv
            Un = [np.where(nb[k], at(U, k), U) for k in range(4)]
            Vn = [np.where(nb[k], at(V, k), V) for k in range(4)]
            Ux, Uy = half * (Un[RIGHT] - Un[LEFT]), half * (Un[DOWN] - Un[UP])
            Vx, Vy = half * (Vn[RIGHT] - Vn[LEFT]), half * (Vn[DOWN] - Vn[UP])
            s = alpha / np.sqrt((((Ux * Ux + Uy * Uy) + Vx * Vx) + Vy * Vy) + eps2)
            w = [np.where(nb[k], half * (s + at(s, k)), zero) for k in range(4)]
            sigma = np.zeros(A.shape, dt)
            for k in range(4):
                sigma = sigma + w[k]
            for _ in range(prm['sor']):
                for colour in (0, 1):
                    sel = dom & (((xs + ys) & 1) == colour)
                    num_u, num_v = b1 - A12 * dv, None
                    tu = [np.where(nb[k], w[k] * ((at(u, k) + at(du, k)) - u), zero) for k in range(4)]
                    tv = [np.where(nb[k], w[k] * ((at(v, k) + at(dv, k)) - v), zero) for k in range(4)]
                    for k in range(4):
                        num_u = num_u + tu[k]
                    den_u = A11 + sigma
                    du_s = num_u / den_u
                    du_n = du + omega * (du_s - du)
                    ok_u = (den_u != 0) & np.isfinite(du_n)
                    num_v = b2 - A12 * np.where(ok_u, du_s, du)
                    for k in range(4):
                        num_v = num_v + tv[k]
                    den_v = A22 + sigma
                    dv_s = num_v / den_v
                    dv_n = dv + omega * (dv_s - dv)
                    ok_v = (den_v != 0) & np.isfinite(dv_n)
                    du, dv = np.where(sel & ok_u, du_n, du), np.where(sel & ok_v, dv_n, dv)
                    assert du.dtype == dt and dv.dtype == dt
        out = np.stack([np.where(dom & (du != 0), u + du, u), np.where(dom & (dv != 0), v + dv, v)], axis=-1)
    assert out.dtype == dt
    return out, data


def restate(near_p, far_p, vecs, fmask, sign, near_mask=None, far_mask=None, valid=None, quant=O.QUANT_OPENCV, dt=F32, **kw):
    """near_p, far_p: float32 (N, C, H, W), the tensors widened; vecs (H, W, 2) or (N, H, W, 2), fmask and the optional
    masks (H, W) or (N, H, W); kw: the parameters that differ from DEFAULTS -> dict(vecs (N, H, W, 2) of type dt -- the
    float32 result carries the input's bits wherever the definition keeps them --, data, dom, cov1: bool (N, H, W))"""
    near_p = np.ascontiguousarray(near_p, F32)
    n, c, h, w = near_p.shape
    base = P.restate(near_p, far_p, vecs, fmask, sign, near_mask=near_mask, far_mask=far_mask, quant=quant)
    full = lambda a, tail: np.broadcast_to(np.asarray(a), (n, h, w) + tail)
    f = np.ascontiguousarray(full(vecs, (2,)), F32)
    with np.errstate(all='ignore'):
        dom = full(fmask, ()).astype(bool) & np.isfinite(f[..., 0]) & np.isfinite(f[..., 1])
        if valid is not None:
            dom = dom & full(valid, ()).astype(bool)
        A, B = Cn.intensity(near_p), Cn.intensity(base['warped'])
    out, data = solve(A, B, base['covered'], f, dom, sign, settings(**kw), dt)
    return dict(vecs=out, data=data, dom=dom, cov1=base['covered'])


def refine(near, far, dtype, layout, vecs, fmask, sign, **kw):
    """restate() for arrays in the memory order of `layout` and of `dtype` (bfloat16: uint16 patterns), 3 or 4 dimensions"""
    return restate(R.to_f32(T.to_planar(near, layout), dtype), R.to_f32(T.to_planar(far, layout), dtype), vecs, fmask, sign, **kw)


# ------------------------------------------------------------------------------------------------- the input generator
def holes(shape):
    """a field mask whose holes put edges into non-domain pixels on both colours and on the seams of the 64 x 16 tile: a
    block (consistency_ref.masks'), single pixels of either colour next to x = 63 | 64 and y = 15 | 16, and a pixel whose
    four neighbours are all holes"""
    h, w = shape
    m = np.ones(shape, bool)
    if h < 8 or w < 8:
        return m
    m[h // 4:h // 2, w // 8:w // 3] = False
    for y, x in ((15, 63), (16, 63), (15, 64), (16, 65), (3, 63), (4, 64), (15, 5), (16, 6)):
        if y < h and x < w:
            m[y, x] = False
    y, x = h - 4, w - 5                                  # an island: dom, no neighbour in the domain
    m[y - 1, x] = m[y + 1, x] = m[y, x - 1] = m[y, x + 1] = False
    return m


def images(rng, c, f, sign, dtype):
    """(near, far) planar (n, c, h, w) as stored in `dtype` for the fields f (n, h, w, 2), intensities of about 0 ... 255: far
    planes smooth, near = far gathered along the field PLUS a smooth disturbance of about half a pixel (QUANT_EXACT), so
    there is something to refine"""
    n, h, w = f.shape[:3]
    far = np.stack([np.stack([128 + 60 * smooth(rng, h, w, 1.0)[..., 0] for _ in range(c)]) for _ in range(n)]).astype(F32)
    near = np.empty_like(far)
    for i in range(n):
        g = (f[i] + smooth(rng, h, w, 0.5)).astype(F32)
        for k in range(c):
            near[i, k] = O.gather_bilinear(np.ascontiguousarray(far[i, k]), g, sign, quant=O.QUANT_EXACT)
    return P.stored(near, dtype), P.stored(far, dtype)


@functools.lru_cache(maxsize=None)
def case(seed, shape, sign, quant, c, dtype='float32', n=1, masked=False, params=()):
    """One generated case, computed once and shared, read-only: dict(near, far: planar (n, c, h, w) as stored in `dtype`;
    f (n, h, w, 2), fm (n, h, w) with holes(); near_mask, far_mask, valid (n, h, w) uint8 or None (`masked`); kw: dict(params);
    want: restate()'s dict).  The generator asserts for SHAPES that the data term acts on 30 % of the pixels at least and
    that the refinement moves at least half of the domain."""
    h, w = shape
    rng = np.random.default_rng([seed, h, w, c])
    amp = 0.4 if shape in TINY else 3.0
    f = np.stack([smooth(rng, h, w, amp) for _ in range(n)])
    fm = np.stack([np.roll(holes(shape), i, axis=1) for i in range(n)])
    near, far = images(rng, c, f, sign, dtype)
    nm = am = va = None
    if masked:
        nm, am, va = (np.ones((n, h, w), np.uint8) for _ in range(3))
        nm[:, h // 2:h // 2 + 3, w // 2:] = 0
        am[:, :h // 3, w // 2:w // 2 + 9] = 0
        va[:, 2 * h // 3:, :w // 4] = 0
        va[:, ::5, 1::7] = 0
    kw = dict(params)
    want = restate(R.to_f32(near, dtype), R.to_f32(far, dtype), f, fm, sign, near_mask=nm, far_mask=am, valid=va, quant=quant, **kw)
    if shape in SHAPES:
        moved = (want['vecs'].view(np.uint32) != f.view(np.uint32)).any(axis=-1)
        assert want['data'].mean() >= 0.3, ("data share", shape, sign, quant, c, want['data'].mean())
        assert moved[want['dom']].mean() >= 0.5, ("moved share", shape, sign, quant, c)
        assert not moved[~want['dom']].any()
    out = dict(near=near, far=far, f=f, fm=fm, near_mask=nm, far_mask=am, valid=va, kw=kw, want=want)
    for a in (near, far, f, fm, nm, am, va) + tuple(want.values()):
        if a is not None:
            a.flags.writeable = False
    return out


# ------------------------------------------------------------------------------------------------- it refines
TRUE_VECTOR = (0.6, -0.4)


def wave_image(xs, ys):
    """I(x, y) of the known answer, float64"""
    return (128 + 40 * np.sin(2 * np.pi * xs / 23) * np.cos(2 * np.pi * ys / 31) + 30 * np.sin(2 * np.pi * (xs + ys) / 17)
            + 25 * np.cos(2 * np.pi * (xs - 2 * ys) / 41))


def shifted_pair(shape=(48, 80)):
    """near = I, far = I shifted by TRUE_VECTOR, sampled analytically: far(q + TRUE_VECTOR) = I(q) -> (near, far) float32
    (1, 1, h, w); the field that explains them is TRUE_VECTOR everywhere with reference 's'"""
    ys, xs = np.mgrid[:shape[0], :shape[1]].astype(F64)
    near = wave_image(xs, ys)
    far = wave_image(xs - TRUE_VECTOR[0], ys - TRUE_VECTOR[1])
    return near.astype(F32)[None, None], far.astype(F32)[None, None]


def epe(vecs, border=8):
    """mean end-point error against TRUE_VECTOR over the pixels at least `border` from the frame"""
    d = vecs.astype(F64)[..., border:-border, border:-border, :] - np.array(TRUE_VECTOR)
    return float(np.sqrt((d * d).sum(axis=-1)).mean())
