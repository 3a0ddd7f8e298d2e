"""Flow.matrix on the device (K8, ofl_fit.hip) against the NumPy restatement tests/matrix_ref.py: float64 sums within the
bound of their fixed addition order, counts / medians / samples exactly, matrices end to end."""
import math
import os

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev, matrix_fit, utils
import matrix_ref as R

pytestmark = pytest.mark.gpu

TRANSFORMS = [['translation', 20, 10], ['rotation', 200, 200, 30], ['scaling', 100, 100, 1.1]]
COMBOS = [(4, 'ransac'), (4, 'lmeds'), (6, 'ransac'), (6, 'lmeds'), (8, 'lms'), (8, 'ransac'), (8, 'lmeds')]
AFFINE = np.array([[1.02, -0.03, 1.5], [0.04, 0.97, -2.0], [0, 0, 1.0]])
# largest |device - matrix_ref| / max(1, |matrix_ref|) over test_end_to_end_agrees_with_ref's cases, measured on an MI355X
# (the sample sets, counts and medians are identical, only the float64 sum order differs): see that test's docstring
MEASURED_SUM_ORDER_DIFF = 2.4e-9
MARGIN = 100 * MEASURED_SUM_ORDER_DIFF


def make_field(kind, shape, ref, seed=0):
    """(vecs float32, mask bool or None)"""
    h, w = shape
    rng = np.random.default_rng(seed)
    s = min(h, w) / 40.0 + 0.2
    H = np.array([[1.01, 0.02, 0.3 * s], [-0.015, 0.99, -0.2 * s], [1e-5 / s, -2e-5 / s, 1.0]])
    vecs = of.Flow.from_matrix(H, [h, w], ref).vecs
    mask = None
    if kind == 'noisy':
        vecs = vecs + ((rng.random((h, w, 2)) - .5) * 5).astype(np.float32)
    if kind == 'holes':
        mask = rng.random((h, w)) > 0.3
        mask[h // 3: h // 2, w // 4: w // 2] = False
    if kind in ('four', 'three'):
        mask = np.zeros((h, w), bool)
        mask.ravel()[rng.choice(h * w, 4 if kind == 'four' else 3, replace=False)] = True
    return np.ascontiguousarray(vecs, np.float32), mask, H


def models_for(H, shape):
    h, w = shape
    pole = np.array([[1.0, 0, 0], [0, 1.0, 0], [2.0 / w, 0, -1.0]])          # denominator changes sign at x = w / 2
    return np.array([H, H + 1e-4 * np.arange(9).reshape(3, 3) / 9, np.diag([3.0, -2.0, 1.0]), AFFINE, pole, np.zeros((3, 3))])


def pair(vecs, mask, ref):
    d = dev.DeviceFlow.from_host(vecs, ref, mask)
    return dev.FitField(d.vecs, d.mask if mask is not None else None, d.shape, -1 if ref == 't' else 1), R.Field(vecs, ref, mask), d


# ------------------------------------------------------------------------------ sums
def depth(n):
    """longest addition chain of a sum as built (include/ofl.h K8): a thread's 16 pixels + 3 tail pixels, six butterfly
    levels, three additions of wave sums, one addition per 4096-px workgroup"""
    chunks = max(1, -(-(n // 4) // 1024))
    return 16 + 3 + 6 + 3 + chunks


@pytest.mark.parametrize("shape,kind,ref", [((37, 53), 'smooth', 's'), ((130, 129), 'holes', 't'), ((130, 129), 'noisy', 's'),
                                            ((1, 5), 'smooth', 't')])
def test_sums_within_the_bound_of_their_addition_order(gpu, shape, kind, ref):
    vecs, mask, H = make_field(kind, shape, ref)
    D, F, _ = pair(vecs, mask, ref)
    F.exact = True
    n = shape[0] * shape[1]
    norm = np.array([shape[1] / 2.0, shape[0] / 2.1, 2.0 / shape[1] + 0.01, shape[1] / 1.9, shape[0] / 2.0, 2.0 / shape[0] + 0.02])
    Tn = lambda c, s: np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])
    Hn = Tn(norm[3:5], norm[5]) @ H @ np.linalg.inv(Tn(norm[0:2], norm[2]))
    Hn = Hn / Hn[2, 2] + 1e-3
    for gate in (None, (H + 1e-5, np.float32(0.5)), (AFFINE, np.float32(9.0))):
        for name, args, terms in (("moments", (), F.moments_terms(gate)), ("dlt", (norm,), F.dlt_terms(norm, gate)),
                                  ("gn", (norm, Hn), F.gn_terms(norm, Hn, gate))):
            got = getattr(D, name)(*args, gate=gate)
            again = getattr(D, name)(*args, gate=gate)
            assert got.tobytes() == again.tobytes(), name
            cols = [np.asarray(t) for t in terms]
            assert len(cols) == got.size - 1
            assert got[-1] == F.nonfinite
            for k, col in enumerate(cols):
                want, total = math.fsum(col), math.fsum(np.abs(col))
                bound = depth(n) * 2.0 ** -53 * total
                print(name, k, "diff", abs(got[k] - want), "bound", bound)
                assert abs(got[k] - want) <= bound, (name, k, gate is not None)


def test_sums_count_nonfinite_vectors(gpu):
    vecs, mask, H = make_field('holes', (40, 41), 's')
    vecs[3, 4] = np.nan
    vecs[7, 8, 1] = np.inf
    mask[3, 4] = mask[7, 8] = True
    D, F, _ = pair(vecs, mask, 's')
    s = D.moments()
    assert s[15] == 2 == F.nonfinite and s[14] == F.idx.size


# ------------------------------------------------------------------------------ counts, medians, samples
CASES = [((1, 5), 'smooth', 's', 6), ((7, 1), 'noisy', 't', 6), ((33, 35), 'holes', 's', 32), ((33, 35), 'noisy', 't', 32),
         ((64, 66), 'four', 's', 5), ((64, 66), 'three', 't', 1), ((250, 131), 'noisy', 's', 17),
         ((1080, 1920), 'holes', 't', 4), ((2160, 3840), 'noisy', 's', 3)]


@pytest.mark.parametrize("shape,kind,ref,K", CASES)
def test_counts_medians_and_samples_are_exact(gpu, shape, kind, ref, K):
    vecs, mask, H = make_field(kind, shape, ref)
    D, F, _ = pair(vecs, mask, ref)
    base = models_for(H, shape)
    rng = np.random.default_rng(K)
    models = np.array([base[i % len(base)] + (i // len(base)) * 1e-3 * (rng.random((3, 3)) - .5) for i in range(K)])
    n = F.idx.size
    assert D.moments()[14] == n
    for thr in (np.float32(9.0), np.float32(0.01)):
        assert np.array_equal(D.score(models, thr), F.score(models, thr))
    lo, hi = (n - 1) // 2, n // 2
    assert np.array_equal(D.median(models, lo, hi), F.median(models, lo, hi))
    assert np.array_equal(D.median(models[:1], 0, n - 1), F.median(models[:1], 0, n - 1))
    D.index()
    ranks = np.concatenate([[0, n - 1, n, n + 7], rng.integers(0, n, 60)])
    assert np.array_equal(D.pick(ranks), F.pick(ranks))


# ------------------------------------------------------------------------------ end to end
def reldiff(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def test_end_to_end_agrees_with_ref(gpu):
    """DeviceFlow.matrix == Flow.matrix == get_flow_matrix bit for bit, and all agree with matrix_ref: identical sample
    sets, counts and medians, so only the float64 sum order differs.  Measured on an MI355X over these 42 cases: 0 to 4.5e-14 for
    dof 4 / 6, up to 1.3e-13 for dof 8 on smooth fields and 2.4e-9 (MEASURED_SUM_ORDER_DIFF) for dof 8 on the noisy 't' field,
    where the last Levenberg-Marquardt steps change the cost by less than the sums' rounding and the two sides may stop
    one step apart.  The assertion allows 100 x the maximum."""
    worst = 0.0
    for ref in 'st':
        for kind in ('smooth', 'noisy', 'holes'):
            vecs, mask, _ = make_field(kind, (240, 322), ref, seed=3)
            d = dev.DeviceFlow.from_host(vecs, ref, mask)
            for dof, method in COMBOS:
                got = d.matrix(dof, method)
                assert got.shape == (3, 3) and got.dtype == np.float64
                assert np.array_equal(got, of.Flow(vecs, ref, mask).matrix(dof, method))
                if mask is None:
                    assert np.array_equal(got, of.get_flow_matrix(vecs, ref, dof, method))
                if dof != 8:
                    assert got[2].tolist() == [0.0, 0.0, 1.0]
                want = R.matrix(vecs, ref, mask, dof=dof, method=method)
                worst = max(worst, reldiff(got, want))
                print(ref, kind, dof, method, "device vs ref", reldiff(got, want))
    print("largest device - ref difference", worst)
    assert worst <= MARGIN


@pytest.fixture(scope="module")
def known():
    mat = utils.matrix_from_transforms(TRANSFORMS)
    return mat, {ref: of.Flow.from_matrix(mat, (1000, 2000), ref) for ref in 'st'}


@pytest.mark.parametrize("ref", ['s', 't'])
def test_reference_known_answers(gpu, known, ref):
    """reference tests/test_flow_class.py:609-646"""
    mat, flows = known
    d = flows[ref].to_device()
    for dof, method in COMBOS:
        M = d.matrix(dof, method)
        if dof == 8:
            np.testing.assert_allclose(M, mat, rtol=1e-8, atol=1e-8)
        else:
            np.testing.assert_allclose(M, mat)


def test_reference_noise_and_mask_cases(gpu, known):
    """reference tests/test_flow_class.py:665-708"""
    mat, flows = known
    rng = np.random.default_rng(5)
    noisy = dev.DeviceFlow.from_host(flows['s'].vecs + ((rng.random((1000, 2000, 2)) - .5) * 5).astype(np.float32), 's')
    for dof, method in COMBOS:
        np.testing.assert_allclose(noisy.matrix(dof, method), mat, rtol=0.05, atol=0.05)
    np.testing.assert_allclose(noisy.matrix(6, 'ransac', seed=11), mat, rtol=0.05, atol=0.05)      # another seed
    assert np.array_equal(noisy.matrix(6, 'lmeds', seed=4), noisy.matrix(6, 'lmeds', seed=4))
    mask = np.zeros((1000, 2000), bool)
    mask[:500, :500] = True
    vecs = ((rng.random((1000, 2000, 2)) - 0.5) * 200).astype(np.float32)
    vecs[:500, :500] = flows['s'].vecs[:500, :500]
    flow = of.Flow(vecs, 's', mask)
    with pytest.raises(AssertionError):
        np.testing.assert_allclose(flow.matrix(4, 'lmeds', False), mat)
    np.testing.assert_allclose(flow.matrix(4, 'lmeds', True), mat)
    with pytest.warns(UserWarning):
        assert np.array_equal(flows['s'].matrix(4, 'lms'), flows['s'].matrix(4, 'ransac'))


def test_random_homographies(gpu):
    """reference tests/test_flow_class.py:648-663 with np.random.default_rng(20261017), 1000 cases, atol = rtol = 1e-2: no
    'lms' case may fail, at most 5 % of the 'ransac' / 'lmeds' cases.  matrix_ref alone (tests/golden/matrix_random_fits.npz,
    written by `python tests/matrix_ref.py`) fails 0 / 0 / 0 of 1000.  The device fails no case matrix_ref passes by more
    than the end-to-end margin."""
    mats = R.random_homographies()
    ref_fits = np.load(os.path.join(os.path.dirname(__file__), "golden", "matrix_random_fits.npz"))["fits"]
    fails = dict.fromkeys(R.RANDOM_METHODS, 0)
    for i, m in enumerate(mats):
        d = of.Flow.from_matrix(m, R.RANDOM_SHAPE, 's').to_device()
        for k, method in enumerate(R.RANDOM_METHODS):
            try:
                got = d.matrix(8, method)
            except ValueError:
                got = np.full((3, 3), np.nan)
            ok = np.allclose(got, m, atol=1e-2, rtol=1e-2)
            fails[method] += not ok
            if not ok and np.allclose(ref_fits[i, k], m, atol=1e-2, rtol=1e-2):
                excess = np.abs(got - m) - (1e-2 + 1e-2 * np.abs(m))
                assert np.nanmax(excess) <= MARGIN * max(1.0, np.abs(m).max()), (i, method)
    print("failures", fails)
    assert fails['lms'] == 0 and fails['ransac'] <= 50 and fails['lmeds'] <= 50


# ------------------------------------------------------------------------------ determinism and safety
def test_degenerate_and_nonfinite_fields(gpu):
    vecs, mask, _ = make_field('three', (64, 66), 's')
    with pytest.raises(ValueError):
        dev.DeviceFlow.from_host(vecs, 's', mask).matrix(8, 'lms')
    with pytest.raises(ValueError):
        dev.DeviceFlow.from_host(vecs, 's', np.zeros((64, 66), bool)).matrix(4)
    assert np.array_equal(dev.DeviceFlow.from_host(np.zeros((9, 11, 2), np.float32), 't').matrix(6, 'lmeds'), np.eye(3))
    vecs, _, _ = make_field('noisy', (60, 70), 's')
    vecs[5, 6] = np.nan
    vecs[20:30, 10, 0] = np.inf
    try:
        out = dev.DeviceFlow.from_host(vecs, 's').matrix(8, 'ransac')
        assert out.shape == (3, 3)
    except ValueError:
        pass
