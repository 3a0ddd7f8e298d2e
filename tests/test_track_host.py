"""Host half of point tracking on the device (K10): device.track_args raises what the reference raises, and the NumPy
restatement tests/track_ref.py -- to which test_gpu_track.py pins the kernels bit for bit -- gives the answers the
reference's own tests hold (tests/test_utils.py, TestTrackPts; tests/test_flow_class.py, test_track).  No GPU needed."""
import numpy as np
import pytest

from oflibnumpy_amd import device as dev
from oflibnumpy_amd import utils
import track_ref as T

PTS = np.array([[20.5, 10.5], [8.3, 7.2], [120.4, 160.2]])


# ------------------------------------------------------------------------------ track_args
def test_track_args_defaults():
    assert dev.track_args(PTS) == (False, False, False)
    assert dev.track_args(PTS, True, True, True) == (True, True, True)
    assert dev.track_args(PTS.astype(np.float32), None, None, None) == (False, False, False)
    assert dev.track_args(np.array([[20, 10], [8, 7]]), int_out=True) == (True, False, False)
    assert dev.track_args(np.zeros((0, 2))) == (False, False, False)


@pytest.mark.parametrize("kwargs, exc", [
    (dict(pts='test'), TypeError),                                   # wrong pts type
    (dict(pts=[[1.0, 2.0]]), TypeError),
    (dict(pts=np.zeros((10, 10, 2))), ValueError),                   # wrong pts shape
    (dict(pts=np.zeros((3, 2)).transpose()), ValueError),            # pts channel not of size 2
    (dict(pts=np.zeros((3, 2), bool)), TypeError),                   # neither float nor int
    (dict(pts=np.zeros((3, 2), complex)), TypeError),
    (dict(pts=np.zeros((3, 2), np.uint8)), TypeError),               # integers other than int32 / int64
    (dict(pts=PTS, int_out='test'), TypeError),
    (dict(pts=PTS, int_out=1), TypeError),
    (dict(pts=PTS, get_valid_status='test'), TypeError),
    (dict(pts=PTS, s_exact_mode='test'), TypeError),
])
def test_track_args_raise_like_the_reference(kwargs, exc):
    with pytest.raises(exc):
        dev.track_args(**kwargs)


# ------------------------------------------------------------------------------ track_ref against the reference's answers
def test_ref_bilinear_rotation():
    """TestTrackPts.test: rotation by 30 degrees about the origin, 's', default mode, with the reference's tolerances"""
    f_s = utils.from_transforms([['rotation', 0, 0, 30]], (512, 512), 's')
    desired = [[12.5035207776, 19.343266740], [3.58801085141, 10.385382907], [24.1694586156, 198.93726969]]
    np.testing.assert_allclose(T.track(f_s, PTS), desired, atol=1e-1, rtol=1e-2)
    got = T.track(f_s, PTS, int_out=True)
    assert got.dtype == np.dtype('i')
    assert np.abs(got - np.round(desired)).max() <= 1          # the interpolated result, rounded


def test_ref_integer_points_translation():
    """TestTrackPts.test: 's' flow and int points -- an integer translation moves them by exactly that vector"""
    f = utils.from_transforms([['translation', 10, 20]], (512, 512), 's')
    pts = np.array([[20, 10], [8, 7]])
    assert np.array_equal(T.track(f, pts), [[40, 20], [28, 17]])
    assert np.array_equal(T.track(f, pts.astype(np.int32), int_out=True), [[40, 20], [28, 17]])
    assert np.array_equal(T.track(f, pts.astype(np.float64)), [[40.0, 20.0], [28.0, 17.0]])


def test_ref_integer_and_float_points_agree_off_the_last_row_and_column():
    h, w = 37, 53
    f = utils.from_transforms([['rotation', 26, 18, 7], ['translation', 1.5, -2.25]], (h, w), 's')
    r, c = np.meshgrid(np.arange(h - 1), np.arange(w - 1), indexing='ij')
    pts = np.stack([r.ravel(), c.ravel()], axis=-1)
    assert np.array_equal(T.track(f, pts), T.track(f, pts.astype(np.float64)))
    # ON the last row / column the reference's clipped corner weights vanish: the sample is 0, the point stays
    edge = np.array([[h - 1, 5.0], [3.0, w - 1], [h - 1, w - 1]])
    assert np.array_equal(T.track(f, edge), edge)
    assert not np.array_equal(T.track(f, edge.astype(np.int64)), edge)


def test_ref_zero_flow_rule():
    """a flow that is zero under the 1e-3 threshold leaves the points alone -- bitwise, not moved by 5e-4 -- even outside"""
    tiny, small = np.full((9, 11, 2), 5e-4, np.float32), np.full((9, 11, 2), 2e-3, np.float32)
    pts = np.array([[1.25, 2.5], [7.0, 9.75], [-3.0, 40.0]])
    assert np.array_equal(T.track(tiny, pts), pts)
    assert np.array_equal(T.track(tiny, pts.astype(np.int64)), pts.astype(np.int64))
    moved = T.track(small, pts[:2])
    assert np.all(moved > pts[:2]) and np.abs(moved - pts[:2]).max() < 2.1e-3
    with pytest.raises(IndexError):
        T.track(small, pts)


def test_ref_outside_and_status():
    f = utils.from_transforms([['translation', 2, 1]], (9, 11), 's')
    for bad in ([-0.25, 3.0], [np.nan, 3.0], [8.5, 3.0], [3.0, 10.5]):
        with pytest.raises(IndexError):
            T.track(f, np.array([[1.0, 1.0], bad]))
    with pytest.raises(IndexError):
        T.track(f, np.array([[1, 1], [9, 3]]))
    valid = np.zeros((9, 11), bool)
    valid[2, 4] = True
    pts = np.array([[2.5, 3.5], [1.5, 4.5], [2.4, 4.4], [3.5, 4.5]])       # np.round: half to even
    _, status = T.track(f, pts, valid=valid)
    assert status.tolist() == [True, True, True, False]
    assert T.status_lookup(valid, np.array([[-0.6, 4.0], [np.nan, 4.0], [2.0, 10.6]])).tolist() == [False, False, False]


def test_ref_sequence_rules():
    """a point is lost at the first step whose input position is outside, and stays there; the others go on"""
    f = utils.from_transforms([['translation', 0, 3]], (9, 11), 's')          # 3 rows down per step
    pts = np.array([[0.5, 2.0], [3.5, 2.0], [6.5, 2.0]])
    end, lost_at, status, path = T.track_sequence([f, f, f], pts)
    assert lost_at.tolist() == [-1, 2, 1]
    assert np.array_equal(end, [[9.5, 2.0], [9.5, 2.0], [9.5, 2.0]]) and status.tolist() == [True, False, False]
    assert path.shape == (4, 3, 2) and np.array_equal(path[0], pts) and np.array_equal(path[-1], end)
    assert np.array_equal(path[:, 2, 0], [6.5, 9.5, 9.5, 9.5])
    # the sequence of test_gpu_track.py is not vacuous (without status maps, which need the device's valid_source)
    fields = [v for v, _ in T.sequence_fields()]
    end, lost_at, _, path = T.track_sequence(fields, T.sequence_points())
    assert len(set(lost_at.tolist())) >= 4 and (lost_at < 0).mean() >= 0.25
    assert np.array_equal(path[T.SEQ_ZERO_FIELD], path[T.SEQ_ZERO_FIELD + 1])
