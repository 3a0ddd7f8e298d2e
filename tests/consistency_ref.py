"""NumPy statement of K13 (oflibnumpy_amd/csrc/ofl_consistency.hip, include/ofl.h) on top of the oracle -- a helper of
test_consistency_host.py and test_gpu_consistency.py, not a test.

The forward-backward check samples the backward field b where the forward field f points (the oracle's bilinear gather:
x + sign * f, sign +1 for 's', -1 for 't'), adds the two vectors and compares the squared sum with a bound that grows with
the two squared magnitudes.  Every operation below is an explicit float32 NumPy operation in the order of the definition,
so the device result is compared with array_equal: masks, residual bits and counts.  The restatement checks ITSELF against
the oracle's fused composition each time it runs: its vector sum and `covered` are compose3_raw's out and mask."""
import functools

import numpy as np

from oracle import np_oracle as O

ALPHA, BETA = 0.01, 0.5
SHAPES = [(5, 7), (19, 70), (37, 131), (64, 256)]       # odd and even widths; below, across and exactly on wave and tile edges
SIGNS = [1, -1]
QUANTS = [O.QUANT_OPENCV, O.QUANT_EXACT]
F32 = np.float32


def _same_floats(a, b):
    """identical bits, except that a NaN may carry any payload: which operand's payload a sum of two NaNs hands on depends on the
    order the compiler gives the operands"""
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def consistency(f, fm, b, bm, sign, alpha=ALPHA, beta=BETA, quant=O.QUANT_OPENCV):
    """-> (consistent bool, covered bool, residual float32, (n_covered, n_consistent))"""
    f, b = np.ascontiguousarray(f, F32), np.ascontiguousarray(b, F32)
    fm, bm = np.asarray(fm).astype(bool), np.asarray(bm).astype(bool)
    sampled, whole = O.gather_bilinear(b, f, sign, smask=bm, want_valid=True, quant=quant)      # whole: interpolated mask == 1
    fu, fv, bu, bv = f[..., 0], f[..., 1], sampled[..., 0], sampled[..., 1]
    covered = fm & whole
    ru, rv = fu + bu, fv + bv
    out, mout = O.compose3_raw(b, bm, f, fm, sign, quant)
    assert _same_floats(np.stack([ru, rv], -1), out) and np.array_equal(covered, mout)
    r2 = ru * ru + rv * rv
    s2 = (fu * fu + fv * fv) + (bu * bu + bv * bv)
    lim = F32(alpha) * s2 + F32(beta)
    assert r2.dtype == s2.dtype == lim.dtype == F32
    consistent = covered & (r2 <= lim)
    residual = np.where(covered, np.sqrt(r2), F32(0)).astype(F32)
    return consistent, covered, residual, (int(covered.sum()), int(consistent.sum()))


def near_threshold(f, fm, b, bm, sign, alpha=ALPHA, beta=BETA, quant=O.QUANT_OPENCV, band=0.05):
    """the number of covered pixels with |r2 - lim| <= band * lim, in float64 from the float32 r2 and lim of the definition"""
    f, b = np.ascontiguousarray(f, F32), np.ascontiguousarray(b, F32)
    sampled, whole = O.gather_bilinear(b, f, sign, smask=np.asarray(bm).astype(bool), want_valid=True, quant=quant)
    fu, fv, bu, bv = f[..., 0], f[..., 1], sampled[..., 0], sampled[..., 1]
    ru, rv = fu + bu, fv + bv
    r2 = (ru * ru + rv * rv).astype(np.float64)
    lim = (F32(alpha) * ((fu * fu + fv * fv) + (bu * bu + bv * bv)) + F32(beta)).astype(np.float64)
    return int(((np.abs(r2 - lim) <= band * lim) & np.asarray(fm).astype(bool) & whole).sum())


# ------------------------------------------------------------------------------------------------- the input generator
def smooth(rng, h, w, amp):
    """a 5 x 5 lattice of standard_normal * amp draws, bilinearly upsampled to (h, w, 2), float32"""
    lat = rng.standard_normal((5, 5, 2)) * amp
    ys, xs = np.linspace(0, 4, h), np.linspace(0, 4, w)
    y0, x0 = np.minimum(ys.astype(int), 3), np.minimum(xs.astype(int), 3)
    ty, tx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    top = lat[y0][:, x0] * (1 - tx) + lat[y0][:, x0 + 1] * tx
    bot = lat[y0 + 1][:, x0] * (1 - tx) + lat[y0 + 1][:, x0 + 1] * tx
    return (top * (1 - ty) + bot * ty).astype(F32)


def masks(h, w):
    fm, bm = np.ones((h, w), bool), np.ones((h, w), bool)
    fm[h // 4:h // 2, w // 8:w // 3] = False
    bm[h // 2:3 * h // 4, w // 2:3 * w // 4] = False
    return fm, bm


def pair(seed, shape, sign):
    """(f, fm, b, bm): a smooth forward field of about 5 px (1 px at (5, 7), which is there for the index arithmetic only), its
    approximate inverse plus a smooth disturbance of about 0.8 px that straddles the bound, and two masks with a hole each"""
    h, w = shape
    rng = np.random.default_rng(seed)
    f = smooth(rng, h, w, 1.0 if shape == (5, 7) else 5.0)
    b = (-O.gather_bilinear(f, f, -sign, quant=O.QUANT_EXACT) + smooth(rng, h, w, 0.8)).astype(F32)
    fm, bm = masks(h, w)
    return f, fm, b, bm


@functools.lru_cache(maxsize=None)
def case(seed, shape, sign, quant, alpha=ALPHA, beta=BETA):
    """(inputs, expected) of one generated case, computed once and shared; read-only"""
    inputs = pair(seed, shape, sign)
    want = consistency(*inputs, sign, alpha, beta, quant)
    for a in inputs + want[:3]:
        a.flags.writeable = False
    return inputs, want


# ------------------------------------------------------------------------------------------------- the known answers
def translation(shape=(37, 131), v=(3.0, -2.0)):
    """f = v everywhere, b = -v, all valid: covered is the (H - |v.y|) x (W - |v.x|) pixels whose sample stays inside"""
    f = np.broadcast_to(np.array(v, F32), shape + (2,)).copy()
    return f, np.ones(shape, bool), -f, np.ones(shape, bool)


def rotation(ref, shape=(37, 131), degrees=20.0):
    """rotation by `degrees` about the centre and by -degrees, as from_transforms builds them for reference `ref`"""
    h, w = shape
    c = [(w - 1) / 2, (h - 1) / 2]
    f = O.from_transforms([['rotation', c[0], c[1], degrees]], shape, ref)
    b = O.from_transforms([['rotation', c[0], c[1], -degrees]], shape, ref)
    return f.vecs, f.mask, b.vecs, b.mask
