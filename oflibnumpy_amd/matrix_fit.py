"""Host side of Flow.matrix (reference flow_class.py:797-867): argument validation and the tiny float64 linear algebra
of fitting a 3x3 matrix to a flow field.  Everything O(H * W) -- moments, normal equations, inlier counts, medians of
residuals, sampling of valid pixels -- is a pass of csrc/ofl_fit.hip (K8), reached through the `field` object that
`device.DeviceFlow.matrix` hands to `fit`; only a few dozen sums, counters and sampled pixels ever reach the host.

The reference calls cv2.findHomography / cv2.estimateAffine2D / cv2.estimateAffinePartial2D.  The estimators here follow
the same published scheme with the parameters those calls imply, but are not bit-compatible with OpenCV.
"""
import warnings

import numpy as np

# what the reference's calls imply (OpenCV 4.x defaults): findHomography(src, dst, method) has ransacReprojThreshold = 3,
# maxIters = 2000, confidence = 0.995; estimateAffine2D / estimateAffinePartial2D(src, dst, method=...) have
# ransacReprojThreshold = 3, maxIters = 2000, confidence = 0.99.  LMedS assumes 45 % outliers (calib3d ptsetreg.cpp).
REPROJ_THRESHOLD_SQ = np.float32(3.0 * 3.0)
MAX_ITERS = 2000
CONFIDENCE = {4: 0.99, 6: 0.99, 8: 0.995}
LMEDS_OUTLIER_RATIO = 0.45
MIN_SET = {4: 2, 6: 3, 8: 4}
BATCH = 32                  # models fitted on the host and scored by one launch (ofl_fit_score_dev takes up to 32)
DEFAULT_SEED = 0            # OpenCV's generator is fixed too
MAX_REFINE_STEPS = 10
RANSAC_REFITS = 3           # gated fits that end RANSAC: on the inliers of the best sample, then twice on the inliers of the fit

_ERR = "Error fitting transformation matrix to flow: "


def matrix_args(dof=None, method=None, masked=None, seed=None):
    """Validation of Flow.matrix's arguments (reference flow_class.py:817-847), before any device work:
    -> (dof, method, masked, seed) with the defaults filled in and 'lms' replaced for dof 4 / 6 (with the warning)."""
    dof = 8 if dof is None else dof
    if dof not in [4, 6, 8]:
        raise ValueError(_ERR + "Dof needs to be 4, 6 or 8")
    method = 'ransac' if method is None else method
    if method not in ['lms', 'ransac', 'lmeds']:
        raise ValueError(_ERR + "Method needs to be 'lms', 'ransac', or 'lmeds'")
    masked = True if masked is None else masked
    if not isinstance(masked, bool):
        raise TypeError(_ERR + "Masked needs to be boolean")
    seed = DEFAULT_SEED if seed is None else seed
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0:
        raise TypeError(_ERR + "Seed needs to be a non-negative integer")
    if dof in [4, 6] and method == 'lms':
        method = 'ransac'
        warnings.warn("Method 'lms' (least mean squares) not supported for fitting a transformation matrix with 4 "
                      "or 6 degrees of freedom to the flow - defaulting to 'ransac'")
    return int(dof), method, masked, int(seed)


def update_iters(confidence, outlier_ratio, model_points, max_iters):
    """Iterations after which a sample of inliers has been drawn with probability `confidence` (the rule OpenCV's
    RANSAC and LMedS use, calib3d ptsetreg.cpp RANSACUpdateNumIters)."""
    p = min(max(confidence, 0.0), 1.0)
    ep = min(max(outlier_ratio, 0.0), 1.0)
    tiny = np.finfo(np.float64).tiny
    num = max(1.0 - p, tiny)
    denom = 1.0 - (1.0 - ep) ** model_points
    if denom < tiny:
        return 0
    num, denom = np.log(num), np.log(denom)
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters
    return int(np.rint(num / denom))


# ------------------------------------------------------------------------------ from sums to models
def _moments(s):
    """ofl_fit_moments_dev's sums -> n, means (x, y, X, Y) about the origin and the centred second moments C[i][j]."""
    pos = {}
    t = 0
    for i in range(5):
        for j in range(i, 5):
            pos[(i, j)] = pos[(j, i)] = t
            t += 1
    n = s[pos[(4, 4)]]
    mean = np.array([s[pos[(i, 4)]] / n for i in range(4)])
    C = np.array([[s[pos[(i, j)]] - s[pos[(i, 4)]] * mean[j] for j in range(4)] for i in range(4)])
    return n, mean, C


def _affine_from_moments(s, origin, dof):
    n, mean, C = _moments(s)
    A = np.eye(3)
    if dof == 6:
        G = C[:2, :2]
        if not np.linalg.det(G) > 1e-12 * max(G[0, 0] * G[1, 1], np.finfo(float).tiny):
            raise ValueError(_ERR + "the correspondences are collinear")
        A[0, :2] = np.linalg.solve(G, C[:2, 2])
        A[1, :2] = np.linalg.solve(G, C[:2, 3])
    else:
        den = C[0, 0] + C[1, 1]
        if not den > 0:
            raise ValueError(_ERR + "the correspondences coincide")
        a = (C[0, 2] + C[1, 3]) / den
        b = (C[0, 3] - C[1, 2]) / den
        A[0, :2] = [a, -b]
        A[1, :2] = [b, a]
    o = np.asarray(origin, np.float64)
    A[:2, 2] = (mean[2:] - A[:2, :2] @ mean[:2]) + o - A[:2, :2] @ o
    return A


def _hartley(s, origin):
    """centre and isotropic scale (RMS distance sqrt(2)) of the source and the target points -> (cx, cy, s, cX, cY, S)"""
    n, mean, C = _moments(s)
    vs, vd = (C[0, 0] + C[1, 1]) / n, (C[2, 2] + C[3, 3]) / n
    if not (vs > 0 and vd > 0):
        raise ValueError(_ERR + "the correspondences coincide")
    return np.array([origin[0] + mean[0], origin[1] + mean[1], np.sqrt(2.0 / vs),
                     origin[0] + mean[2], origin[1] + mean[3], np.sqrt(2.0 / vd)])


def _sym(tri, k):
    M = np.zeros((k, k))
    M[np.triu_indices(k)] = tri
    return M + np.triu(M, 1).T


def _denormalise(Hn, norm):
    cx, cy, s, cX, cY, S = norm
    Ts = np.array([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1.0]])
    Tdi = np.array([[1 / S, 0, cX], [0, 1 / S, cY], [0, 0, 1.0]])
    M = Tdi @ Hn @ Ts
    if M[2, 2] != 0:
        M = M / M[2, 2]
    return M


def _homography(field, gate):
    """Normalised DLT on the gated correspondences, then Levenberg-Marquardt on the reprojection error."""
    origin = field.origin
    s = field.moments(gate)
    if s[14] < 4:
        raise ValueError(_ERR + "fewer than 4 correspondences")
    norm = _hartley(s, origin)
    L = _sym(field.dlt(norm, gate)[:45], 9)
    Hn = np.linalg.eigh(L)[1][:, 0].reshape(3, 3)
    if abs(Hn[2, 2]) > 1e-8 * np.abs(Hn).max():
        Hn = _refine(field, norm, Hn / Hn[2, 2], gate)
    return _denormalise(Hn, norm)


def _refine(field, norm, Hn, gate):
    h = Hn.ravel().copy()
    s = field.gn(norm, h, gate)
    cost = s[44]
    if not np.isfinite(s[:45]).all():
        return Hn
    lam = 1e-3
    for _ in range(MAX_REFINE_STEPS):
        JtJ, g = _sym(s[:36], 8), s[36:44]
        try:
            d = np.linalg.solve(JtJ + lam * np.diag(np.diag(JtJ)), -g)
        except np.linalg.LinAlgError:
            break
        h2 = h.copy()
        h2[:8] += d
        s2 = field.gn(norm, h2, gate)
        if np.isfinite(s2[:45]).all() and s2[44] < cost:
            done = cost - s2[44] <= 1e-14 * cost or np.abs(d).max() <= 1e-14 * np.abs(h).max()
            h, s, cost, lam = h2, s2, s2[44], max(lam * 0.1, 1e-9)
            if done:
                break
        else:
            lam *= 10.0
            if lam > 1e6:
                break
    return h.reshape(3, 3)


def _full_fit(field, dof, gate):
    if dof == 8:
        return _homography(field, gate)
    s = field.moments(gate)
    if s[14] < MIN_SET[dof]:
        raise ValueError(_ERR + "fewer than {} correspondences".format(MIN_SET[dof]))
    return _affine_from_moments(s, field.origin, dof)


# ------------------------------------------------------------------------------ minimal sets
def minimal_model(src, dst, dof):
    """The model through 2 / 3 / 4 correspondences (src, dst: (m, 2) float64), or None for a degenerate set."""
    M = np.eye(3)
    with np.errstate(all='ignore'):
        if dof == 4:
            d, D = src[1] - src[0], dst[1] - dst[0]
            den = d[0] * d[0] + d[1] * d[1]
            if not den > 0:
                return None
            a = (d[0] * D[0] + d[1] * D[1]) / den
            b = (d[0] * D[1] - d[1] * D[0]) / den
            M[0, :2] = [a, -b]
            M[1, :2] = [b, a]
            M[:2, 2] = dst[0] - M[:2, :2] @ src[0]
        elif dof == 6:
            d1, d2 = src[1] - src[0], src[2] - src[0]
            cross = d1[0] * d2[1] - d1[1] * d2[0]
            if not abs(cross) > 1e-9 * np.sqrt((d1 @ d1) * (d2 @ d2)):
                return None
            A = np.column_stack([src, np.ones(3)])
            M[0] = np.linalg.solve(A, dst[:, 0])
            M[1] = np.linalg.solve(A, dst[:, 1])
        else:
            A, b = np.zeros((8, 8)), np.zeros(8)
            for i in range(4):
                x, y = src[i]
                X, Y = dst[i]
                A[2 * i] = [x, y, 1, 0, 0, 0, -X * x, -X * y]
                A[2 * i + 1] = [0, 0, 0, x, y, 1, -Y * x, -Y * y]
                b[2 * i], b[2 * i + 1] = X, Y
            try:
                if not np.linalg.cond(A) < 1e14:
                    return None
                M = np.append(np.linalg.solve(A, b), 1.0).reshape(3, 3)
            except np.linalg.LinAlgError:
                return None
    return M if np.isfinite(M).all() else None


def _draw_models(field, rng, n, dof):
    """BATCH minimal sets of valid pixels (ranks among the n valid ones) -> (BATCH, 3, 3) models, zeros where degenerate
    (a zero matrix has residual +Inf everywhere: no inlier, the largest median)."""
    m = MIN_SET[dof]
    ranks = rng.integers(0, n, size=(BATCH, m))
    src, dst = field.sample(ranks.ravel())
    src, dst = src.reshape(BATCH, m, 2), dst.reshape(BATCH, m, 2)
    models = np.zeros((BATCH, 3, 3))
    for i in range(BATCH):
        if len(set(ranks[i].tolist())) < m:
            continue
        M = minimal_model(src[i], dst[i], dof)
        if M is not None:
            models[i] = M
    return models


# ------------------------------------------------------------------------------ the estimators
def fit(field, dof, method, seed, zero=False):
    """The 3x3 float64 matrix.  `field` provides the device passes: origin, moments(gate), dlt(norm, gate),
    gn(norm, model, gate), score(models, thr), median(models, lo, hi), sample(ranks); gate = None or (model, thr).
    zero: every (masked) vector is exactly zero -- the identity, without fitting."""
    m = MIN_SET[dof]
    s = field.moments(None)
    n = int(s[14])
    if n < m:
        raise ValueError(_ERR + "the flow has {} valid vectors, dof {} needs at least {}".format(n, dof, m))
    if zero:
        return np.eye(3)
    if method == 'lms':
        M = _full_fit(field, dof, None)
    else:
        rng = np.random.default_rng(seed)
        field.index()
        best = None
        if method == 'ransac':
            niters, done, best_count = MAX_ITERS, 0, 0
            while done < niters:
                models = _draw_models(field, rng, n, dof)
                counts = field.score(models, REPROJ_THRESHOLD_SQ)
                for i in range(BATCH):
                    if done + i >= niters:
                        break
                    if counts[i] > max(best_count, m - 1):
                        best, best_count = models[i], int(counts[i])
                        niters = update_iters(CONFIDENCE[dof], (n - best_count) / n, m, niters)
                done += BATCH
            thr = REPROJ_THRESHOLD_SQ
        else:
            niters = update_iters(CONFIDENCE[dof], LMEDS_OUTLIER_RATIO, m, MAX_ITERS)
            best_med, done = np.inf, 0
            while done < niters:
                k = min(BATCH, niters - done)
                models = _draw_models(field, rng, n, dof)
                bits = field.median(models[:k], (n - 1) // 2, n // 2)
                vals = bits.view(np.float32).astype(np.float64)
                meds = (vals[:, 0] + vals[:, 1]) / 2
                for i in range(k):
                    if meds[i] < best_med:
                        best, best_med = models[i], meds[i]
                done += BATCH
            if best is not None:
                sigma = 2.5 * 1.4826 * (1 + 5.0 / max(n - m, 1)) * np.sqrt(best_med)
                thr = np.float32(max(sigma, 0.001) ** 2)
        if best is None:
            raise ValueError(_ERR + "no non-degenerate sample of {} correspondences found".format(m))
        M = _full_fit(field, dof, (best, thr))
        if method == 'ransac':
            # a model through 2 - 4 noisy pixels selects a lopsided share of the noise; the inliers of the fit do not
            for _ in range(RANSAC_REFITS - 1):
                M = _full_fit(field, dof, (M, thr))
    if dof != 8:
        M[2] = [0.0, 0.0, 1.0]
    return M
