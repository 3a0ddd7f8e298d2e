"""Flow.matrix without a GPU: argument validation (before any device work), the 'lms' warning, NoDeviceError, the export
of get_flow_matrix -- and the NumPy restatement tests/matrix_ref.py held to the reference's own known-answer tolerances
(reference tests/test_flow_class.py:609-689), which ties it to the reference rather than to the code under test."""
import warnings

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import _native as nat, matrix_fit, utils
import matrix_ref as R

TRANSFORMS = [['translation', 20, 10], ['rotation', 200, 200, 30], ['scaling', 100, 100, 1.1]]
COMBOS = [(4, 'ransac'), (4, 'lmeds'), (6, 'ransac'), (6, 'lmeds'), (8, 'lms'), (8, 'ransac'), (8, 'lmeds')]
WARNING = ("Method 'lms' (least mean squares) not supported for fitting a transformation matrix with 4 "
           "or 6 degrees of freedom to the flow - defaulting to 'ransac'")


def test_matrix_argument_validation():
    f = of.Flow.zero((10, 12))
    for call in (f.matrix, lambda *a, **k: of.DeviceFlow(None, None, (10, 12), 't').matrix(*a, **k)):
        with pytest.raises(ValueError, match="Dof needs to be 4, 6 or 8"):
            call(dof=5)
        with pytest.raises(ValueError, match="Method needs to be 'lms', 'ransac', or 'lmeds'"):
            call(dof=4, method='test')
        with pytest.raises(ValueError):
            call(dof='test')
        with pytest.raises(TypeError, match="Masked needs to be boolean"):
            call(dof=4, method='lmeds', masked='test')
    with pytest.raises(TypeError):
        of.DeviceFlow(None, None, (10, 12), 't').matrix(seed=1.5)
    with pytest.raises(ValueError):
        of.get_flow_matrix(f.vecs, 't', dof=3)
    with pytest.raises(ValueError):
        of.get_flow_matrix(f.vecs, 'x')
    assert matrix_fit.matrix_args() == (8, 'ransac', True, matrix_fit.DEFAULT_SEED)
    assert matrix_fit.matrix_args(6, 'lmeds', False, 7) == (6, 'lmeds', False, 7)


def test_lms_falls_back_to_ransac_with_the_reference_warning():
    for dof in (4, 6):
        with pytest.warns(UserWarning) as rec:
            assert matrix_fit.matrix_args(dof, 'lms')[:2] == (dof, 'ransac')
        assert [str(w.message) for w in rec] == [WARNING]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert matrix_fit.matrix_args(8, 'lms')[1] == 'lms'


def test_matrix_needs_a_device():
    if nat.device_count() > 0:
        pytest.skip("a GPU is present")
    f = of.Flow.from_transforms([['rotation', 5, 5, 20]], (16, 20), 't')
    with pytest.raises(nat.NoDeviceError):
        f.matrix()
    with pytest.raises(nat.NoDeviceError), pytest.warns(UserWarning):       # validated and warned first
        f.matrix(4, 'lms')
    with pytest.raises(nat.NoDeviceError):
        of.get_flow_matrix(f.vecs, 't', 6, 'lmeds')
    rc = nat.load().ofl_fit_moments_dev(None, None, 4, 4, 1, None, None, 0.0, None, 0, None, None)
    assert rc == nat.E_NODEVICE


def test_get_flow_matrix_is_exported():
    assert 'get_flow_matrix' in of.flow_operations.__all__ and callable(of.get_flow_matrix)
    assert hasattr(of.Flow, 'matrix') and hasattr(of.DeviceFlow, 'matrix')


def test_update_iters_and_parameters():
    """the iteration rule and the parameters the reference's OpenCV calls imply"""
    assert matrix_fit.REPROJ_THRESHOLD_SQ == np.float32(9) and matrix_fit.MAX_ITERS == 2000
    assert matrix_fit.CONFIDENCE == {4: 0.99, 6: 0.99, 8: 0.995}
    for m, want in ((2, 13), (3, 25), (4, 55)):         # log(1 - conf) / log(1 - 0.55 ** m), rounded
        conf = 0.995 if m == 4 else 0.99
        assert matrix_fit.update_iters(conf, 0.45, m, 2000) == want == R.update_iters(conf, 0.45, m, 2000)
    assert matrix_fit.update_iters(0.99, 0.0, 3, 2000) == 0
    assert matrix_fit.update_iters(0.99, 1.0, 3, 2000) == 2000


@pytest.fixture(scope="module")
def known():
    mat = utils.matrix_from_transforms(TRANSFORMS)
    return mat, {ref: R.Field(of.Flow.from_matrix(mat, (1000, 2000), ref).vecs, ref) for ref in 'st'}


@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("dof,method", COMBOS)
def test_ref_meets_reference_known_answers(known, ref, dof, method):
    """reference tests/test_flow_class.py:609-646: assert_allclose defaults for dof 4 / 6, rtol = atol = 1e-8 for dof 8"""
    mat, fields = known
    M = R.matrix(None, ref, dof=dof, method=method, field=fields[ref])
    if dof == 8:
        np.testing.assert_allclose(M, mat, rtol=1e-8, atol=1e-8)
    else:
        np.testing.assert_allclose(M, mat)
        assert M[2].tolist() == [0.0, 0.0, 1.0]


def test_ref_meets_reference_noise_tolerance(known):
    """reference tests/test_flow_class.py:665-689: (rand - .5) * 5 added, rtol = atol = 0.05"""
    mat, fields = known
    noise = ((np.random.default_rng(5).random((1000, 2000, 2)) - .5) * 5).astype(np.float32)
    field = R.Field(of.Flow.from_matrix(mat, (1000, 2000), 's').vecs + noise, 's')
    for dof, method in COMBOS:
        M = R.matrix(None, 's', dof=dof, method=method, field=field)
        np.testing.assert_allclose(M, mat, rtol=0.05, atol=0.05, err_msg="dof {} {}".format(dof, method))


def test_ref_degenerate_inputs():
    v = np.zeros((6, 7, 2), np.float32)
    assert np.array_equal(R.matrix(v, 's', dof=8, method='lmeds'), np.eye(3))
    v[..., 0] = 1.5
    mask = np.zeros((6, 7), bool)
    mask[2, 3] = True
    with pytest.raises(ValueError):
        R.matrix(v, 's', mask, dof=4)
    assert R.minimal_model(np.zeros((2, 2)), np.ones((2, 2)), 4) is None
    line = np.array([[0., 0.], [1., 1.], [2., 2.]])
    assert R.minimal_model(line, line, 6) is None and matrix_fit.minimal_model(line, line, 6) is None
