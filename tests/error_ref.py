"""NumPy statement of K14 (oflibnumpy_amd/csrc/ofl_error.hip, include/ofl.h): an estimated field against a ground truth --
a helper of test_error_host.py and test_gpu_error.py, not a test.

Every per-pixel operation below is an explicit float32 NumPy operation, one per line, in the order of the definition, so the
device's counts, maximum and maps are compared with array_equal.  The float64 sums are math.fsum over the exact terms -- the
correctly rounded sum -- and the device's sums, which are added in a fixed order, are compared within depth(H * W) * 2^-53
of it."""
import functools
import math

import numpy as np

F32 = np.float32
INF = F32(np.inf)

# the settings the generated cases are evaluated with: the defaults (1, 3, 5 px; KITTI's 3 px and 5 %; Sintel's 10, 40) plus a
# fourth threshold and a third edge, so that no slot of the record is idle
THR = np.array([1, 3, 5, 8], F32)
OUT_ABS, OUT_REL = F32(3), F32(0.05)
EDGES = np.array([10, 40, 90], F32)

# the kernel's constants (ofl_error.hip)
CHUNK = 4096                  # pixels per workgroup
PER_THREAD = 16               # terms a thread adds per sum: 4 steps x 4 pixels
BUTTERFLY = 6                 # xor levels of a wave of 64
WAVES = 4                     # wave values of a workgroup of 256 threads, added in order: 3 additions
FINISH_THREADS = 256          # the finishing kernel: thread t takes partials t, t + 256, ...

# (1, 1); less than a wave with a tail of 3; 1330 px; exactly one chunk; 4095 px; one pixel into a second chunk; several
# chunks, the last partial; and more than FINISH_THREADS chunks, so that the finishing loop takes a second trip
SHAPES = [(1, 1), (5, 7), (19, 70), (64, 64), (65, 63), (17, 241), (40, 392), (1040, 1024)]
assert -(-1040 * 1024 // CHUNK) > FINISH_THREADS


def depth(n):
    """the longest chain of additions a term of a float64 sum passes through, as stated in include/ofl.h: a thread's 16 terms,
    six butterfly levels and three additions of wave values in the chunk kernel, then ceil(chunks / 256) partials per thread,
    six levels and three additions in the finishing kernel.  Two of the counted additions (a thread's first, in either kernel)
    add to +0.0 and are exact; they cover the second-order terms of (1 + 2^-53)^depth - 1 <= depth * 2^-53 * (1 + 1e-13)."""
    chunks = -(-n // CHUNK)
    return PER_THREAD + BUTTERFLY + (WAVES - 1) + -(-chunks // FINISH_THREADS) + BUTTERFLY + (WAVES - 1)


def flow_error(est, em, gt, gm, thr=THR, out_abs=OUT_ABS, out_rel=OUT_REL, edges=EDGES, use_est_mask=True):
    """-> dict: the record's fields (counts as ints, `max_epe_bits`, the sums as correctly rounded floats), `epe_map` (float32)
    and `outlier_map` (uint8).  em None: as use_est_mask False."""
    est, gt = np.ascontiguousarray(est, F32), np.ascontiguousarray(gt, F32)
    thr, edges = np.asarray(thr, F32), np.asarray(edges, F32)
    assert thr.shape == (4,) and edges.shape == (3,)
    eu, ev, gu, gv = est[..., 0], est[..., 1], gt[..., 0], gt[..., 1]
    with np.errstate(all='ignore'):
        du = eu - gu
        dv = ev - gv
        uu = du * du
        vv = dv * dv
        e2 = uu + vv
        epe = np.sqrt(e2)
        gg = gu * gu
        hh = gv * gv
        g2 = gg + hh
        g = np.sqrt(g2)
        rel = F32(out_rel) * g
        assert all(a.dtype == F32 for a in (du, dv, uu, vv, e2, epe, gg, hh, g2, g, rel))
        evaluated = np.asarray(gm).astype(bool)
        if use_est_mask and em is not None:
            evaluated = evaluated & np.asarray(em).astype(bool)
        finite = np.isfinite(epe)
        ok = evaluated & finite
        bad = evaluated & ~finite
        over = [ok & (epe > thr[k]) for k in range(4)]
        outlier = ok & (epe > F32(out_abs)) & (epe > rel)
        bin_ = (g >= edges[0]).astype(np.int64) + (g >= edges[1]).astype(np.int64) + (g >= edges[2]).astype(np.int64)
    terms = epe[ok].astype(np.float64)
    return {
        "n": int(ok.sum()), "n_nonfinite": int(bad.sum()), "n_over": [int(o.sum()) for o in over], "n_outlier": int(outlier.sum()),
        "n_bin": [int((ok & (bin_ == k)).sum()) for k in range(4)],
        "max_epe_bits": int(epe[ok].max().view(np.uint32)) if ok.any() else 0,
        "sum_epe": math.fsum(terms), "sum_epe2": math.fsum(terms * terms),           # float64 squares of float32 values: exact
        "sum_bin_epe": [math.fsum(epe[ok & (bin_ == k)].astype(np.float64)) for k in range(4)],
        "epe_map": np.where(ok, epe, F32(0)).astype(F32), "outlier_map": outlier.astype(np.uint8),
        "epe": epe, "ok": ok,
    }


def record_words(want):
    """the uint32 part of the record, in its order"""
    return [want["n"], want["n_nonfinite"]] + want["n_over"] + [want["n_outlier"]] + want["n_bin"] + [want["max_epe_bits"]]


def record_sums(want):
    return [want["sum_epe"], want["sum_epe2"]] + want["sum_bin_epe"]


def stats(want, n_thresholds=3, n_edges=2):
    """the derived statistics of FlowErrorStats from a restated record -> dict"""
    n = want["n"]
    mean = lambda total, count: total / count if count else float('nan')
    return {"n": n, "n_nonfinite": want["n_nonfinite"], "epe": mean(want["sum_epe"], n), "rmse": math.sqrt(mean(want["sum_epe2"], n)) if n else float('nan'),
            "max": float(np.array(want["max_epe_bits"], np.uint32).view(F32)) if n else float('nan'),
            "over": tuple(mean(c, n) for c in want["n_over"][:n_thresholds]), "outlier": mean(want["n_outlier"], n),
            "bins": tuple((c, mean(t, c)) for c, t in zip(want["n_bin"][:n_edges + 1], want["sum_bin_epe"][:n_edges + 1]))}


# ------------------------------------------------------------------------------------------------- the input generator
def up(x):
    """one float32 step above x"""
    return np.nextafter(F32(x), INF)


# planted pixels: (est, gt, est mask, gt mask).  gt = 0 under the ties, so that du, dv are the planted values exactly.
BIG = F32(3e38)
PLANTED = [
    ((2.5, -1.0), (1.0, 1.0), True, False),                # masked out by the ground truth
    ((2.5, -1.0), (1.0, 1.0), False, True),                # masked out by the estimate (counted with use_est_mask False)
    ((np.nan, 0.0), (1.0, 1.0), True, True),               # non-finite estimate
    ((0.0, -np.inf), (1.0, 1.0), True, True),
    ((1.0, 1.0), (np.inf, 0.0), True, True),               # non-finite ground truth under a valid gt mask
    ((1.0, 1.0), (0.0, np.nan), True, True),
    ((BIG, 0.0), (-BIG, 0.0), True, True),                 # du overflows
    ((2e19, 0.0), (-1e19, 0.0), True, True),               # du is finite, du * du overflows
    ((7.0, 8.0), (6.0, 8.0), True, True),                  # g = 10 exactly: the first edge, bin 1
    ((24.0, 33.5), (24.0, 32.0), True, True),              # g = 40 exactly: the second edge, bin 2
    ((54.0, 73.0), (54.0, 72.0), True, True),              # g = 90 exactly: the third edge, bin 3
    ((1.0, 0.0), (0.0, 0.0), True, True),                  # epe = 1, 3, 5, 8 exactly: on a threshold, not over it
    ((3.0, 0.0), (0.0, 0.0), True, True),
    ((3.0, 4.0), (0.0, 0.0), True, True),
    ((0.0, 8.0), (0.0, 0.0), True, True),
    ((up(1), 0.0), (0.0, 0.0), True, True),                # one float32 step above each
    ((up(3), 0.0), (0.0, 0.0), True, True),
    ((0.0, up(5)), (0.0, 0.0), True, True),
    ((0.0, up(8)), (0.0, 0.0), True, True),
    ((3.0, 0.0), (1.0, 0.0), True, True),                  # epe 2, g 1: over the relative bound only
    ((64.0, 80.0), (60.0, 80.0), True, True),              # epe 4, g 100: over the absolute bound only (4 <= 5)
    ((0.0, 0.0), (0.0, 0.0), True, True),                  # gt = 0 and no error
    ((66.0, 88.0), (60.0, 80.0), True, True),              # epe 10, g 100: an outlier in bin 3
]


def pair(seed, shape):
    """(est, em, gt, gm): ground-truth speeds spread over all four bins, an estimate off by 0.3 to 15 px, a tenth of either
    mask cleared, and the PLANTED pixels at seeded places -- the pair's last pixel, which the tail code handles, among them.
    A shape with fewer pixels than planted ones takes as many as fit."""
    h, w = shape
    n = h * w
    rng = np.random.default_rng(seed)
    speed = rng.choice(np.array([3.0, 20.0, 60.0, 120.0]), n) * rng.uniform(0.2, 1.3, n)
    angle = rng.uniform(0, 2 * np.pi, n)
    gt = np.stack([speed * np.cos(angle), speed * np.sin(angle)], -1).astype(F32)
    noise = rng.standard_normal((n, 2)) * rng.choice(np.array([0.3, 2.0, 6.0, 15.0]), n)[:, None]
    est = (gt + noise).astype(F32)
    em, gm = rng.random(n) >= 0.1, rng.random(n) >= 0.1
    order = rng.permutation(n)
    places = [n - 1] + [int(p) for p in order if p != n - 1]
    planted = PLANTED if n >= len(PLANTED) else PLANTED[-1:] + PLANTED[:-1]       # (1, 1) holds the evaluated outlier
    for p, (e, g, me, mg) in zip(places, planted):
        est[p], gt[p], em[p], gm[p] = e, g, me, mg
    return est.reshape(h, w, 2), em.reshape(h, w), gt.reshape(h, w, 2), gm.reshape(h, w)


@functools.lru_cache(maxsize=None)
def case(seed, shape, use_est_mask=True):
    """(inputs, expected) of one generated case under THR, OUT_ABS, OUT_REL, EDGES; computed once and shared; read-only"""
    inputs = pair(seed, tuple(shape))
    want = flow_error(*inputs, use_est_mask=use_est_mask)
    for a in inputs + (want["epe_map"], want["outlier_map"], want["epe"], want["ok"]):
        a.flags.writeable = False
    return inputs, want


def ties(want, thr=THR):
    """(pixels with epe exactly on a threshold, pixels one float32 step above one) among the evaluated pixels, per threshold"""
    epe, ok = want["epe"], want["ok"]
    return [int((ok & (epe == t)).sum()) for t in thr], [int((ok & (epe == up(t))).sum()) for t in thr]
