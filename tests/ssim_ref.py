"""NumPy statement of K26 (oflibnumpy_amd/csrc/ofl_ssim.hip, include/ofl.h) on top of photometric_ref and census_ref -- a
helper of test_ssim_host.py and test_gpu_ssim.py, not a test.

photometric_ref.restate gives the warped values w_c (the oracle's bilinear gather, one call per channel plane) and cov1,
K21's `covered`; census_ref.intensity the channel means A and B.  Everything after that is an explicit float32 NumPy
operation in the order of the definition, vectorised per offset, so the device result is compared bit for bit:
    member(q) = q inside the frame & cov1(q)
    for dy = -r ... r, for dx = -r ... r (the centre included), q = p + (dx, dy):
        ga = g[dx+r] * A(q);  gb = g[dx+r] * B(q)
        the six terms g[dx+r], ga, gb, ga * A(q), gb * B(q), ga * B(q), each +0.0 where not member(q)
        R^k_dy = the row sum of term k in ascending dx from +0.0
    S^k = g[0] * R^k_(-r) + ... + g[K-1] * R^k_r: one product and one addition a row, ascending dy, from +0.0
    (Wt, Sa, Sb, Saa, Sbb, Sab) = S^0 ... S^5;  n = the members
    mu_a = Sa / Wt;  mu_b = Sb / Wt;  va = Saa / Wt - mu_a mu_a;  vb = Sbb / Wt - mu_b mu_b;  vab = Sab / Wt - mu_a mu_b
    num = (2 (mu_a mu_b) + c1) (2 vab + c2);  den = ((mu_a mu_a + mu_b mu_b) + c1) ((va + vb) + c2)
    s = num / den;  e = (1 - s) * 0.5;  e = 0 where e < 0, 1 where e > 1 (a NaN stays)
    covered = cov1 & (n >= min_count);  err = e where covered else 0;  within = covered & (e <= tau)

THE BOUND of |e32 - e64| (bound()), a worst case over all inputs with |near_c|, |w_c| <= amax and taps > 0, against the
definition in exact arithmetic on the SAME float32 near, w_c and taps.  u is the unit roundoff, gamma_k = k u / (1 - k u).
  intensity   |A^ - A| <= d amax, d = gamma_(C + 1) (census_ref), so |A^| <= (1 + d) amax; the same for B.
  terms       fl(g A^): one rounding, |. - g A| <= g amax e1, e1 = d + u (1 + d).
              fl(fl(g A^) B^): two, |. - g A B| <= g amax^2 e2, e2 = (2 d + d^2) + gamma_2 (1 + d)^2.
  sums        a term passes K - 1 inexact additions in its row (the first is to +0.0), the product by the row's tap and
              K - 1 additions over the rows: a factor (1 + theta), |theta| <= gamma_(2K - 1).  Other formulations (normalised
              taps, one correlation per axis) have at most four roundings more, so w = gamma_(2K + 3) is used throughout:
              Wt^ = Wt (1 + theta_0), |theta_0| <= w;  |Sa^ - Sa| <= Wt amax E1, E1 = e1 + w (1 + e1);
              |Saa^ - Saa| <= Wt amax^2 E2, E2 = e2 + w (1 + e2).  Wt itself cancels: only taps > 0 is used.
  moments     mu^ = fl(Sa^ / Wt^): |mu^ - mu| <= amax M1, M1 = q1 + u (1 + q1), q1 = (E1 + w) / (1 - w);
              |fl(Saa^ / Wt^) - Saa / Wt| <= amax^2 M2, M2 = q2 + u (1 + q2), q2 = (E2 + w) / (1 - w).
              A product of two means: |fl(mu_a^ mu_b^) - mu_a mu_b| <= (|mu_a| + |mu_b|) amax M1 + amax^2 M1^2 + u (...)
              and, with |mu| <= amax, <= amax^2 P, P = (2 M1 + M1^2) + u (1 + M1)^2.
              A variance: |va^ - va| <= amax^2 V, V = (M2 + P) (1 + u) + u -- THE cancellation: Saa / Wt and mu_a^2 are both of
              the size amax^2 and their difference may be 0.  The same V holds for vb and vab.
  factors     taps > 0, so va, vb >= 0, 2 |vab| <= va + vb and 2 |mu_a mu_b| <= mu_a^2 + mu_b^2 in exact arithmetic: with
              X = 2 mu_a mu_b + c1, Z = mu_a^2 + mu_b^2 + c1, Y = 2 vab + c2, W = va + vb + c2:  |X| <= Z, |Y| <= W, |s| <= 1.
              |Z^ - Z| and |X^ - X| <= rL Z,  rL = gamma_3 + (1 + gamma_2) (2 amax M1 / sqrt(2 c1) + 2 amax^2 M1^2 / c1)
                  -- (|mu_a| + |mu_b|) / (mu_a^2 + mu_b^2 + c1) is largest at |mu_a| = |mu_b| = sqrt(c1 / 2): 1 / sqrt(2 c1);
              |W^ - W| and |Y^ - Y| <= rC W,  rC = gamma_2 + (1 + gamma_2) 2 amax^2 V / c2               (W >= c2).
  quotient    |(x + xi)(y + ups) - x y| <= rL + rC + rL rC for |x|, |y| <= 1; the denominator is off by a factor of at least
              (1 - rL)(1 - rC):  D = (2 (rL + rC) + rL rC) / ((1 - rL)(1 - rC));  three roundings (two products, the
              division): |s^ - s| <= ds = D (1 + gamma_3) + gamma_3.
  e           1 - s^ rounds once, |1 - s^| <= 2 + ds; the product by 0.5 is exact; clamping to [0, 1], where the exact e lies,
              brings e^ no further from it:  |e^ - e| <= 0.5 ds (1 + u) + u.
At intensities 0 ... 255 with Wang's constants the variance term rules: 2 amax^2 V / c2 is about 2e-2 at K = 11, C = 3 and
u = 2^-24, which a flat bright window attains in order of magnitude; what generated images show is 2e-5 to 2e-4."""
import functools

import numpy as np

import census_ref as Cn
import interop_ref as R
import photometric_ref as P
import tensor_ref as T
from oracle import np_oracle as O

F32 = np.float32
U = 2.0 ** -24
WINDOWS = [3, 5, 7, 11]
WEIGHTS = ['uniform', 'gaussian']
SHAPES = Cn.SHAPES                                   # where the generator's share conditions hold (see case)
TINY = Cn.TINY                                       # index arithmetic only: min_count = 1, no share condition
SIGNS, QUANTS = P.SIGNS, P.QUANTS
same_floats = P.same_floats
in_layout = P.in_layout
shifted = Cn.shifted
C1, C2 = F32((0.01 * 255.0) ** 2), F32((0.03 * 255.0) ** 2)


def taps(K, weights='gaussian', sigma=1.5):
    """the 1-D window as float32: ones, or exp(-x^2 / (2 sigma^2)) in float64 divided by its sum"""
    if weights == 'uniform':
        return np.ones(K, F32)
    x = np.arange(K, dtype=np.float64) - K // 2
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(F32)


def window_sums(A, B, cov1, K, g):
    """-> (S: the six float32 sums (Wt, Sa, Sb, Saa, Sbb, Sab) in the stated order, n int32), each (N, H, W)"""
    assert A.dtype == F32 and B.dtype == F32 and g.dtype == F32 and g.shape == (K,)
    r = K // 2
    S, n = [np.zeros(A.shape, F32) for _ in range(6)], np.zeros(A.shape, np.int32)
    for dy in range(-r, r + 1):
        row = [np.zeros(A.shape, F32) for _ in range(6)]
        for dx in range(-r, r + 1):
            member = shifted(cov1, dy, dx, False)
            Aq, Bq, gx = shifted(A, dy, dx, F32(0)), shifted(B, dy, dx, F32(0)), g[dx + r]
            ga, gb = gx * Aq, gx * Bq
            terms = (np.full(A.shape, gx, F32), ga, gb, ga * Aq, gb * Bq, ga * Bq)
            for k in range(6):
                assert terms[k].dtype == F32
                row[k] = row[k] + np.where(member, terms[k], F32(0))
            n += member
        for k in range(6):
            S[k] = S[k] + g[dy + r] * row[k]
            assert S[k].dtype == F32
    return S, n


def error_of(S, c1, c2):
    """the six sums -> (e clamped, s): the formula of the definition, one NumPy operation per rounding"""
    Wt, Sa, Sb, Saa, Sbb, Sab = S
    two, one, half = S[0].dtype.type(2), S[0].dtype.type(1), S[0].dtype.type(0.5)
    mu_a, mu_b = Sa / Wt, Sb / Wt
    aa, bb, ab = mu_a * mu_a, mu_b * mu_b, mu_a * mu_b
    va, vb, vab = Saa / Wt - aa, Sbb / Wt - bb, Sab / Wt - ab
    num = (two * ab + c1) * (two * vab + c2)
    den = ((aa + bb) + c1) * ((va + vb) + c2)
    s = num / den
    e = (one - s) * half
    e = np.where(e < 0, S[0].dtype.type(0), np.where(e > 1, one, e))
    assert e.dtype == S[0].dtype and s.dtype == S[0].dtype
    return e, s


def restate(near_p, far_p, vecs, fmask, sign, K=11, g=None, c1=C1, c2=C2, min_count=None, tau=None, near_mask=None,
            far_mask=None, quant=O.QUANT_OPENCV):
    """near_p, far_p: float32 (N, C, H, W), the tensors widened; field and masks as photometric_ref.restate takes them; g: the
    float32 taps, None: Gaussian with sigma 1.5; min_count None: K^2.
    -> dict(err float32, covered bool, within bool or None: (N, H, W); counts [(n_covered, n_within)] * N; e: the error before
    `covered` is applied; s: SSIM before the clamp; n: the member count; cov1: K21's covered; A, B: the intensities; warped;
    S: the six sums)"""
    assert K in WINDOWS
    g = taps(K) if g is None else np.ascontiguousarray(g, F32)
    c1, c2 = F32(c1), F32(c2)
    min_count = K * K if min_count is None else min_count
    base = P.restate(near_p, far_p, vecs, fmask, sign, near_mask=near_mask, far_mask=far_mask, quant=quant)
    cov1 = base['covered']
    with np.errstate(all='ignore'):
        A, B = Cn.intensity(np.ascontiguousarray(near_p, F32)), Cn.intensity(base['warped'])
        S, n = window_sums(A, B, cov1, K, g)
        e, s = error_of(S, c1, c2)
        covered = cov1 & (n >= min_count)
        err = np.where(covered, e, F32(0)).astype(F32)
        within = None if tau is None else covered & (e <= F32(tau))
    counts = [(int(covered[i].sum()), 0 if within is None else int(within[i].sum())) for i in range(len(e))]
    return dict(err=err, covered=covered, within=within, counts=counts, e=e, s=s, n=n, cov1=cov1, A=A, B=B, warped=base['warped'], S=S)


def ssim(near, far, dtype, layout, vecs, fmask, sign, **kw):
    """restate() for arrays in the memory order of `layout` and of `dtype` (bfloat16: uint16 patterns), 3 or 4 dimensions"""
    return restate(R.to_f32(T.to_planar(near, layout), dtype), R.to_f32(T.to_planar(far, layout), dtype), vecs, fmask, sign, **kw)


def definition64(near_p, warped, cov1, K, g, c1=C1, c2=C2):
    """the definition in float64 on the float32 near, w_c, cov1 and taps -> (e float64, s float64, n)"""
    r, g = K // 2, np.asarray(g, F32).astype(np.float64)
    c1, c2 = np.float64(F32(c1)), np.float64(F32(c2))
    with np.errstate(all='ignore'):
        A, B = near_p.astype(np.float64).mean(axis=1), warped.astype(np.float64).mean(axis=1)
        S, n = [np.zeros(A.shape) for _ in range(6)], np.zeros(A.shape, np.int32)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                member = shifted(cov1, dy, dx, False)
                Aq, Bq, wq = shifted(A, dy, dx, 0.0), shifted(B, dy, dx, 0.0), g[dx + r] * g[dy + r]
                for k, t in enumerate((np.ones(A.shape), Aq, Bq, Aq * Aq, Bq * Bq, Aq * Bq)):
                    S[k] += np.where(member, wq * t, 0.0)
                n += member
        e, s = error_of(S, c1, c2)
    return e, s, n


def gamma(k, u=U):
    return k * u / (1 - k * u)


def bound(K, g, c, amax, c1=C1, c2=C2, u=U):
    """the worst-case bound of |e^ - e| of the module docstring, for unit roundoff u; inf where it says nothing"""
    assert (np.asarray(g) > 0).all() and len(g) == K
    amax, c1, c2 = float(amax), float(F32(c1)), float(F32(c2))
    G = lambda k: gamma(k, u)
    d = G(c + 1)
    e1 = d + u * (1 + d)
    e2 = (2 * d + d * d) + G(2) * (1 + d) ** 2
    w = G(2 * K + 3)
    E1, E2 = e1 + w * (1 + e1), e2 + w * (1 + e2)
    q1, q2 = (E1 + w) / (1 - w), (E2 + w) / (1 - w)
    M1, M2 = q1 + u * (1 + q1), q2 + u * (1 + q2)
    Pm = (2 * M1 + M1 * M1) + u * (1 + M1) ** 2
    V = (M2 + Pm) * (1 + u) + u
    rL = G(3) + (1 + G(2)) * (2 * amax * M1 / np.sqrt(2 * c1) + 2 * amax * amax * M1 * M1 / c1)
    rC = G(2) + (1 + G(2)) * 2 * amax * amax * V / c2
    if rL >= 1 or rC >= 1:
        return np.inf
    D = (2 * (rL + rC) + rL * rC) / ((1 - rL) * (1 - rC))
    ds = D * (1 + G(3)) + G(3)
    return 0.5 * ds * (1 + u) + u


# ------------------------------------------------------------------------------------------------- the input generator
@functools.lru_cache(maxsize=None)
def case(seed, shape, sign, quant, c, dtype='float32', K=11, weights='gaussian', n=1):
    """One generated case, computed once and shared, read-only: dict(near, far: planar (n, c, h, w) as stored in `dtype`
    (census_ref.tensors at scale 255); f, fm; g: the taps; c1, c2: Wang's for 0 ... 255; min_count: (K^2 + 1) // 2, or 1 at
    the TINY shapes; tau: the float32 median of the restatement's own error over its covered pixels; want: restate()'s dict
    with that tau).  The generator asserts, on the restatement alone and for SHAPES, that the covered share of H * W lies
    in [0.3, 0.95] and the within share of the covered pixels in [0.25, 0.75]."""
    h, w = shape
    rng = np.random.default_rng([seed, h, w, c])
    f, fm = P.field(rng, shape)
    near, far = Cn.tensors(rng, n, c, f, sign, dtype, 255.0)
    g = taps(K, weights)
    min_count = 1 if shape in TINY else (K * K + 1) // 2
    args = (R.to_f32(near, dtype), R.to_f32(far, dtype), f, fm, sign)
    kw = dict(K=K, g=g, c1=C1, c2=C2, min_count=min_count, quant=quant)
    first = restate(*args, **kw)
    cov = first['covered']
    tau = F32(np.median(first['e'][cov])) if cov.any() else F32(0)
    want = restate(*args, tau=tau, **kw)
    if shape in SHAPES:
        for i in range(n):
            share = cov[i].sum() / float(h * w)
            assert 0.3 <= share <= 0.95, ("covered share", shape, sign, quant, c, K, weights, share)
            inside = want['within'][i].sum() / float(cov[i].sum())
            assert 0.25 <= inside <= 0.75, ("within share", shape, sign, quant, c, dtype, K, weights, inside)
    want.pop('S')
    out = dict(near=near, far=far, f=f, fm=fm, g=g, c1=C1, c2=C2, min_count=min_count, tau=tau, want=want)
    for a in (near, far, f, fm, g) + tuple(v for v in want.values() if isinstance(v, np.ndarray)):
        a.flags.writeable = False
    return out


# ------------------------------------------------------------------------------------------------- the known answers
def constants(a0, b0, c1=C1, c2=C2):
    """e of two constant images of the small integer intensities a0 and b0 under a uniform window: every sum is an exact
    integer (n, n a0, n a0^2, ...), so the means are a0 and b0, the variances exactly 0 and both second factors c2.  What is
    left is the luminance formula on (a0, b0, c1), three operations a side, with both sides multiplied by c2"""
    a0, b0, c1, c2 = F32(a0), F32(b0), F32(c1), F32(c2)
    num = (F32(2) * (a0 * b0) + c1) * c2
    den = ((a0 * a0 + b0 * b0) + c1) * c2
    e = (F32(1) - num / den) * F32(0.5)
    assert type(e) is F32
    return F32(0) if e < 0 else (F32(1) if e > 1 else e)


def eroded(cov1, K, min_count):
    """cov1 & (at least min_count pixels of the K x K window, the centre among them, are in cov1): census_ref.eroded counts
    the neighbours alone, and where cov1 holds the centre is one more"""
    return Cn.eroded(cov1, K, min_count - 1)
