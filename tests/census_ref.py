"""NumPy statement of K22 (oflibnumpy_amd/csrc/ofl_census.hip, include/ofl.h) on top of photometric_ref -- a helper of
test_census_host.py and test_gpu_census.py, not a test.

photometric_ref.restate gives the warped values w_c (the oracle's bilinear gather, one call per channel plane) and cov1,
K21's `covered`.  Everything after that is an explicit float32 NumPy operation in the order of the definition, vectorised
per offset, so the device result is compared bit for bit:
    A = (near_0 + ... + near_(C-1)) * inv_c,  B = (w_0 + ... + w_(C-1)) * inv_c     ascending c from +0.0
    member(q) = q inside the frame & cov1(q)
    a = A(p + d) - A(p),  b = B(p + d) - B(p)           for |dx|, |dy| <= r = K // 2, d != 0
    hard  t = [s(a) != s(b)],  s(v) = 1 if v > delta, -1 if v < -delta, else 0
    soft  rho(v) = v / sqrt(noise + v * v),  g = rho(a) - rho(b),  q = g * g,  t = q / (knee + q)
    t = +0.0 where not member(p + d);  R_dy = sum over ascending dx from +0.0;  S = sum of R_dy over ascending dy from +0.0
    n = member offsets;  covered = cov1 & (n >= min_count);  e = S / float32(n);  within = covered & (e <= tau)

Error bounds of e against the float64 definition evaluated on the SAME float32 near and w_c (u = 2^-24, gamma_k = k u /
(1 - k u)); `amax` is the largest |near_c| or |w_c| of the case, so |A|, |B| <= amax and |a|, |b| <= 2 amax:
  intensity  the first addition to +0.0 is exact; C - 1 additions, the rounding of inv_c, one product:
             |A32 - A64| <= gamma_(C + 1) amax.  A difference adds one rounding of at most u 2 amax to two such errors:
             |a32 - a64| <= 2 gamma_(C + 2) amax =: margin(C, amax), and the same for b.
  hard       s(a) is a comparison and t is 0 or 1; S is an integer of at most 48 and n an integer, both exact in float32;
             the division rounds once: gamma_1 relative -- PROVIDED no sign decision flips.  A decision can flip only where
             ||a64| - delta| <= margin or ||b64| - delta| <= margin at a member offset; definition64 flags the pixels with
             such an offset in their window as `risky`, and they are left out of the comparison (they are counted).
  soft       rho' = noise / (noise + v^2)^(3/2) <= 1 / sqrt(noise): the intensity error moves rho by at most margin /
             sqrt(noise); its evaluation (product, sum of two terms >= 0, square root, quotient) is gamma_4 relative and
             |rho| < 1.  So d_rho = margin / sqrt(noise) + gamma_4.  g: two of these and one rounding, |g| < 2:
             d_g = 2 d_rho + 2 u.  q = g^2 <= 4: d_q = 4 d_g + d_g^2 + 4 u.  t = q / (knee + q) has slope at most 1 / knee and
             two roundings, t < 1: d_t = d_q / knee + gamma_2, ABSOLUTE.  The mean of at most K^2 - 1 terms >= 0: at most
             K^2 - 2 additions that are not exact and one division: gamma_(K^2 - 1) relative on e.
             -> |e32 - e64| <= gamma_(K^2 - 1) e64 + d_t.  This is a worst case over all inputs of that magnitude (the
             slopes 1 / sqrt(noise) and 1 / knee are attained at v = 0 and q = 0 only); what is seen is far below it."""
import functools

import numpy as np

import interop_ref as R
import tensor_ref as T
import photometric_ref as P
from consistency_ref import smooth
from oracle import np_oracle as O

F32 = np.float32
U = 2.0 ** -24
WINDOWS = [3, 5, 7]
MODES = ['hard', 'soft']
NOISE, KNEE = 0.81, 0.1
SHAPES = [(19, 70), (37, 131), (64, 256)]           # where the generator's share conditions hold (see case)
TINY = [(5, 7), (1, 1), (1, 5), (5, 1)]             # index arithmetic only: min_count = 1, no share condition
SIGNS, QUANTS = P.SIGNS, P.QUANTS
same_floats = P.same_floats
in_layout = P.in_layout


def gamma(k):
    return k * U / (1 - k * U)


def params(mode, delta=0.0, noise=NOISE, knee=KNEE):
    """(p0, p1) of the ABI as float32"""
    return (F32(delta), F32(0)) if mode == 'hard' else (F32(noise), F32(knee))


def shifted(a, dy, dx, fill):
    """out[y, x] = a[..., y + dy, x + dx] where that lies inside the frame, else `fill`"""
    h, w = a.shape[-2:]
    out = np.full_like(a, fill)
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        out[..., y0:y1, x0:x1] = a[..., y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def intensity(t):
    """t float32 (N, C, H, W) -> the channel mean in the order of the definition, float32 (N, H, W)"""
    assert t.dtype == F32
    s = np.zeros(t.shape[:1] + t.shape[2:], F32)
    for c in range(t.shape[1]):
        s = s + t[:, c]
    out = s * F32(1.0 / float(t.shape[1]))
    assert out.dtype == F32
    return out


def term(a, b, mode, p0, p1):
    assert a.dtype == F32 and b.dtype == F32 and type(p0) is F32 and type(p1) is F32
    if mode == 'hard':
        sa = (a > p0).astype(np.int8) - (a < -p0).astype(np.int8)
        sb = (b > p0).astype(np.int8) - (b < -p0).astype(np.int8)
        return (sa != sb).astype(F32)
    ra = a / np.sqrt(p0 + a * a)
    rb = b / np.sqrt(p0 + b * b)
    g = ra - rb
    q = g * g
    t = q / (p1 + q)
    assert t.dtype == F32
    return t


def ordered_sum(t, K):
    """t: {(dx, dy): float32 array} of the K^2 - 1 terms -> S in the order of the definition: each row in ascending dx to
    +0.0, the rows in ascending dy to +0.0"""
    r = K // 2
    S = None
    for dy in range(-r, r + 1):
        row = None
        for dx in range(-r, r + 1):
            if dx == 0 and dy == 0:
                continue
            assert t[dx, dy].dtype == F32
            row = (np.zeros_like(t[dx, dy]) if row is None else row) + t[dx, dy]
        S = (np.zeros_like(row) if S is None else S) + row
    assert S.dtype == F32
    return S


def window_mean(A, B, cov1, K, mode, p0, p1):
    """-> (e float32, n int32): S / n in the stated order and the member count, (N, H, W)"""
    r = K // 2
    t, n = {}, np.zeros(A.shape, np.int32)
    for dy, dx in ((dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx or dy):
        member = shifted(cov1, dy, dx, False)
        t[dx, dy] = np.where(member, term(shifted(A, dy, dx, F32(0)) - A, shifted(B, dy, dx, F32(0)) - B, mode, p0, p1), F32(0))
        n += member
    e = ordered_sum(t, K) / n.astype(F32)
    assert e.dtype == F32
    return e, n


def restate(near_p, far_p, vecs, fmask, sign, K=7, mode='soft', p0=None, p1=None, min_count=None, tau=None, near_mask=None,
            far_mask=None, quant=O.QUANT_OPENCV):
    """near_p, far_p: float32 (N, C, H, W), the tensors widened; field and masks as photometric_ref.restate takes them; p0, p1:
    (delta, -) for 'hard', (noise, knee) for 'soft', None for the defaults; min_count None: K^2 - 1.
    -> dict(err float32, covered bool, within bool or None: (N, H, W); counts [(n_covered, n_within)] * N; e: the distance
    before `covered` is applied; n: the member count; cov1: K21's covered; A, B: the intensities; warped)"""
    assert K in WINDOWS and mode in MODES
    d0, d1 = params(mode)
    p0, p1 = F32(d0 if p0 is None else p0), F32(d1 if p1 is None else p1)
    min_count = K * K - 1 if min_count is None else min_count
    base = P.restate(near_p, far_p, vecs, fmask, sign, near_mask=near_mask, far_mask=far_mask, quant=quant)
    cov1 = base['covered']
    with np.errstate(all='ignore'):
        A, B = intensity(np.ascontiguousarray(near_p, F32)), intensity(base['warped'])
        e, n = window_mean(A, B, cov1, K, mode, p0, p1)
        covered = cov1 & (n >= min_count)
        err = np.where(covered, e, F32(0)).astype(F32)
        within = None if tau is None else covered & (e <= F32(tau))
    counts = [(int(covered[i].sum()), 0 if within is None else int(within[i].sum())) for i in range(len(e))]
    return dict(err=err, covered=covered, within=within, counts=counts, e=e, n=n, cov1=cov1, A=A, B=B, warped=base['warped'])


def census(near, far, dtype, layout, vecs, fmask, sign, **kw):
    """restate() for arrays in the memory order of `layout` and of `dtype` (bfloat16: uint16 patterns), 3 or 4 dimensions"""
    return restate(R.to_f32(T.to_planar(near, layout), dtype), R.to_f32(T.to_planar(far, layout), dtype), vecs, fmask, sign, **kw)


def margin(c, amax):
    """the bound of |a32 - a64| of the module docstring"""
    return 2 * gamma(c + 2) * amax


def definition64(near_p, warped, cov1, K, mode, p0, p1, guard=0.0):
    """the definition in float64 on the float32 near, w_c and cov1 -> (e float64, n, risky bool): risky marks the pixels
    with a member offset where |a| or |b| lies within `guard` of the dead zone's edge (hard mode)"""
    r = K // 2
    p0, p1 = np.float64(F32(p0)), np.float64(F32(p1))
    with np.errstate(all='ignore'):
        A, B = near_p.astype(np.float64).mean(axis=1), warped.astype(np.float64).mean(axis=1)
        S, n, risky = np.zeros(A.shape), np.zeros(A.shape, np.int32), np.zeros(A.shape, bool)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dx == 0 and dy == 0:
                    continue
                member = shifted(cov1, dy, dx, False)
                a, b = shifted(A, dy, dx, 0.0) - A, shifted(B, dy, dx, 0.0) - B
                if mode == 'hard':
                    t = (np.sign(a) * (np.abs(a) > p0) != np.sign(b) * (np.abs(b) > p0)).astype(np.float64)
                    risky |= member & ((np.abs(np.abs(a) - p0) <= guard) | (np.abs(np.abs(b) - p0) <= guard))
                else:
                    g = a / np.sqrt(p0 + a * a) - b / np.sqrt(p0 + b * b)
                    t = g * g / (p1 + g * g)
                S += np.where(member, t, 0.0)
                n += member
        return S / n, n, risky


def bound(K, mode, c, amax=1.0, noise=NOISE, knee=KNEE):
    """(relative, absolute) bound of |e32 - e64| of the module docstring; hard mode: outside the risky pixels"""
    if mode == 'hard':
        return gamma(1), 0.0
    d_rho = margin(c, amax) / np.sqrt(float(F32(noise))) + gamma(4)
    d_g = 2 * d_rho + 2 * U
    d_q = 4 * d_g + d_g * d_g + 4 * U
    return gamma(K * K - 1), d_q / float(F32(knee)) + gamma(2)


# ------------------------------------------------------------------------------------------------- the input generator
def tensors(rng, n, c, f, sign, dtype, scale):
    """(near, far) planar (n, c, h, w) as stored in `dtype`: far planes smooth of amplitude 1 plus uniform noise of +-0.2,
    near = far gathered along the field (QUANT_EXACT) plus uniform noise of +-0.05, both times `scale`.  With K21's smooth
    planes alone the hard distance is 0 at most pixels; the noise gives every window an order to compare."""
    h, w = f.shape[:2]
    far = np.stack([np.stack([smooth(rng, h, w, 1.0)[..., 0] + rng.uniform(-0.2, 0.2, (h, w)).astype(F32) for _ in range(c)])
                    for _ in range(n)]).astype(F32)
    near = np.empty_like(far)
    for i in range(n):
        for k in range(c):
            near[i, k] = (O.gather_bilinear(np.ascontiguousarray(far[i, k]), f, sign, quant=O.QUANT_EXACT)
                          + rng.uniform(-0.05, 0.05, (h, w)).astype(F32))
    return P.stored(near * F32(scale), dtype), P.stored(far * F32(scale), dtype)


@functools.lru_cache(maxsize=None)
def case(seed, shape, sign, quant, c, dtype='float32', K=7, mode='soft', n=1, delta=0.0):
    """One generated case, computed once and shared, read-only: dict(near, far: planar (n, c, h, w) as stored in `dtype`;
    f, fm; p0, p1; min_count: (K^2 - 1) / 2, or 1 at the TINY shapes; tau: the float32 median of the restatement's own
    distance over its covered pixels; want: restate()'s dict with that tau).  Intensities are scaled by 255 for 'soft' and
    for 'hard' with a dead zone (`delta` = 2 is the one in use), and left at amplitude 1 for 'hard' with delta = 0.
    The generator asserts, on the restatement alone and for SHAPES, that the covered share of H * W lies in [0.3, 0.95]
    and the within share of the covered pixels in [0.25, 0.75] ('soft') or [0.25, 0.8] ('hard': the distance takes few
    values, so the median holds many pixels), and for 'hard' that at least a quarter of the covered pixels have e > 0."""
    h, w = shape
    rng = np.random.default_rng([seed, h, w, c])
    f, fm = P.field(rng, shape)
    scale = 255.0 if mode == 'soft' or delta > 0 else 1.0
    near, far = tensors(rng, n, c, f, sign, dtype, scale)
    p0, p1 = params(mode, delta)
    min_count = 1 if shape in TINY else (K * K - 1) // 2
    args = (R.to_f32(near, dtype), R.to_f32(far, dtype), f, fm, sign)
    kw = dict(K=K, mode=mode, p0=p0, p1=p1, min_count=min_count, quant=quant)
    first = restate(*args, **kw)
    cov = first['covered']
    tau = F32(np.median(first['e'][cov])) if cov.any() else F32(0)
    want = restate(*args, tau=tau, **kw)
    if shape in SHAPES:
        for i in range(n):
            share = cov[i].sum() / float(h * w)
            assert 0.3 <= share <= 0.95, ("covered share", shape, sign, quant, c, K, mode, share)
            inside = want['within'][i].sum() / float(cov[i].sum())
            assert 0.25 <= inside <= (0.75 if mode == 'soft' else 0.8), ("within share", shape, sign, quant, c, dtype, K, mode, inside)
            if mode == 'hard':
                nonzero = (want['e'][i][cov[i]] > 0).sum() / float(cov[i].sum())
                assert nonzero >= 0.25, ("nonzero share", shape, sign, quant, c, dtype, K, delta, nonzero)
    out = dict(near=near, far=far, f=f, fm=fm, p0=p0, p1=p1, min_count=min_count, tau=tau, want=want)
    for a in (near, far, f, fm) + tuple(v for v in want.values() if isinstance(v, np.ndarray)):
        a.flags.writeable = False
    return out


# ------------------------------------------------------------------------------------------------- the known answers
def translation(shape=(37, 131), v=(3.0, -2.0), c=3, sign=1, seed=0, lo=0):
    """photometric_ref.translation with `far` holding integers lo ... 255 as float32: f = v everywhere, all valid, near = far
    shifted by the integer vector (0 where the sample falls outside) -> (near, far planar (1, c, h, w), f, fm)"""
    h, w = shape
    rng = np.random.default_rng(seed)
    far = rng.integers(lo, 256, (1, c, h, w)).astype(F32)
    near = shifted(far, int(sign * v[1]), int(sign * v[0]), F32(0))
    f = np.broadcast_to(np.array(v, F32), shape + (2,)).copy()
    return near, far, f, np.ones(shape, bool)


def reach(shape=(37, 131), at=(18, 60), sign=1):
    """translation() with ONE differing pixel: `far` is lowest (-1000 in every channel) where the field sends `at`, so B(at) lies
    below all its neighbours, and `near` is highest (+1000) at `at` itself, so A(at) lies above them.  In hard mode every
    ordering that involves `at` is therefore reversed and no other: err is 1 / n at each of the K^2 - 1 pixels around it,
    n / n = 1 at `at`, and 0 elsewhere.  -> (near, far, f, fm)"""
    near, far, f, fm = translation(shape, sign=sign)
    y, x = at
    far[0, :, y + int(sign * f[0, 0, 1]), x + int(sign * f[0, 0, 0])] = -1000.0
    near = shifted(far, int(sign * f[0, 0, 1]), int(sign * f[0, 0, 0]), F32(0))
    near[0, :, y, x] = 1000.0
    return near, far, f, fm


def eroded(cov1, K, min_count):
    """cov1 bool (N, H, W) -> cov1 & (at least min_count of the K^2 - 1 neighbours inside the frame are in cov1): `covered`
    from K21's covered alone, by a box sum over a zero-padded copy"""
    r = K // 2
    pad = np.pad(cov1.astype(np.int32), ((0, 0), (r, r), (r, r)))
    h, w = cov1.shape[1:]
    box = sum(pad[:, r + dy:r + dy + h, r + dx:r + dx + w] for dy in range(-r, r + 1) for dx in range(-r, r + 1))
    return cov1 & (box - cov1 >= min_count)
