"""CPU suite: the host half of the fill (K15) -- args.fill_args, the ctypes table, the argument checks of Flow.fill and
fill_flow -- and the NumPy restatement tests/fill_ref.py that test_gpu_fill.py compares the kernels with: its distances against
SciPy's Euclidean distance transform (the one independent yardstick; SciPy does not pin the ties), its tie rule on
hand-written cases with known answers."""
import numpy as np
import pytest
from scipy import ndimage

import oflibnumpy_amd as of
from oflibnumpy_amd import args
import fill_ref as F


# ---------------------------------------------------------------------------------------------- the restatement's distances
@pytest.mark.parametrize("shape", [(1, 65), (67, 5), (48, 80), (31, 97)])
@pytest.mark.parametrize("name", ["random50", "random5", "random05", "lattice2", "lattice3", "lattice4", "checker", "corner0",
                                  "corner3", "pair"])
def test_distances_equal_scipys_transform(shape, name):
    m = F.mask(name, shape)
    assert m.any()
    _, out_mask, index, d2 = F.expected(name, shape)
    edt = ndimage.distance_transform_edt(m == 0)                     # float64 distances to the nearest zero of ~source
    want = np.rint(edt ** 2).astype(np.int64)
    assert np.array_equal(d2.astype(np.int64), want)
    assert out_mask.all() and (index >= 0).all()
    # an index names a source at exactly that distance
    qy, qx = np.divmod(index.astype(np.int64), shape[1])
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    assert m[qy, qx].all() and np.array_equal((y - qy) ** 2 + (x - qx) ** 2, want)


def test_no_source_and_all_sources():
    for shape in [(1, 1), (3, 129)]:
        v = F.vectors(shape)
        out_vecs, out_mask, index, d2 = F.fill(v, np.zeros(shape, np.uint8))
        assert (index == -1).all() and (d2 == F.FAR).all() and not out_mask.any() and out_vecs.tobytes() == v.tobytes()
        out_vecs, out_mask, index, d2 = F.fill(v, np.ones(shape, np.uint8))
        assert np.array_equal(index.ravel(), np.arange(shape[0] * shape[1])) and not d2.any() and out_mask.all()
        assert out_vecs.tobytes() == v.tobytes()                      # NaN payloads, Inf and -0.0 included


# ---------------------------------------------------------------------------------------------- the tie rule, by hand
def test_ties_go_to_the_smallest_linear_index():
    # 1 x 5, sources at columns 0 and 4: column 2 is 2 px from both -> the smaller column
    _, _, index, d2 = F.fill(None, np.array([[1, 0, 0, 0, 1]], np.uint8))
    assert index.tolist() == [[0, 0, 0, 4, 4]] and d2.tolist() == [[0, 1, 4, 1, 0]]
    # 3 x 3, the four edge midpoints: the centre is 1 px from all four -> the top one (index 1); each corner is 1 px from two
    m = np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], np.uint8)
    _, _, index, d2 = F.fill(None, m)
    assert index.tolist() == [[1, 1, 1], [3, 1, 5], [3, 7, 5]] and d2.tolist() == [[1, 0, 1], [0, 1, 0], [1, 0, 1]]
    # 3 x 3, the four corners: the smaller row wins before the smaller column
    m = np.array([[1, 0, 1], [0, 0, 0], [1, 0, 1]], np.uint8)
    _, _, index, d2 = F.fill(None, m)
    assert index.tolist() == [[0, 0, 2], [0, 0, 2], [6, 6, 8]] and d2.tolist() == [[0, 1, 0], [1, 2, 1], [0, 1, 0]]
    # 3 x 3, a source below left and one to the right at the same distance from (1, 1)... the row above / the same row first
    m = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0]], np.uint8)
    _, _, index, _ = F.fill(None, m)
    assert index[1, 1] == 5 and index[0, 0] == 5 and index[2, 2] == 5   # (0, 0): both at d2 = 5; (2, 2): both at 1 -> row 1


def test_max_d2_and_valid():
    m = np.zeros((5, 9), np.uint8)
    m[0, 0] = 1
    v = F.vectors((5, 9))
    for max_d2, reach in ((24, False), (25, True)):
        out_vecs, out_mask, index, d2 = F.fill(v, m, None, max_d2)
        assert bool(out_mask[4, 3]) is reach and bool(index[4, 3] == 0) is reach            # (3, 4) away: d2 = 25
        assert d2[4, 3] == (25 if reach else F.FAR)
        assert out_vecs[4, 3].tobytes() == (v[0, 0] if reach else v[4, 3]).tobytes()
    out_vecs, out_mask, index, d2 = F.fill(v, m, None, 0)
    assert out_mask.sum() == 1 and out_vecs.tobytes() == v.tobytes()
    # a pixel whose own mask is 1 but whose valid is 0 is overwritten from its nearest source
    mask, valid = np.ones((1, 4), np.uint8), np.array([[1, 0, 0, 1]], np.uint8)
    v = F.vectors((1, 4))
    out_vecs, out_mask, index, d2 = F.fill(v, mask, valid)
    assert index.tolist() == [[0, 0, 3, 3]] and out_mask.all()
    assert out_vecs[0, 1].tobytes() == v[0, 0].tobytes() and out_vecs[0, 2].tobytes() == v[0, 3].tobytes()


# ---------------------------------------------------------------------------------------------- fill_args, the table, the host forms
def test_fill_args_values():
    assert args.fill_args() == -1 and args.fill_args(None) == -1
    assert [args.fill_args(v) for v in (0, 1, 1.5, 5, 1e9)] == [0, 1, 2, 25, 2 ** 31 - 1]
    assert args.fill_args(np.float32(2.5)) == 6 and args.fill_args(np.int64(7)) == 49 and args.fill_args(10 ** 400) == 2 ** 31 - 1
    assert args.fill_args(46340.95) == 2147483646 and args.fill_args(46341) == 2 ** 31 - 1
    assert all(isinstance(args.fill_args(v), int) for v in (None, 0, 2.5))


@pytest.mark.parametrize("bad", [-1, -1e-9, float('nan'), float('inf'), -float('inf'), np.float32('nan'), -10 ** 400])
def test_fill_args_value_errors(bad):
    with pytest.raises(ValueError, match="Error filling flow"):
        args.fill_args(bad)


@pytest.mark.parametrize("bad", ["3", True, np.True_, [3], (3,), np.array([3.0]), 1j, object()])
def test_fill_args_type_errors(bad):
    with pytest.raises(TypeError, match="Error filling flow"):
        args.fill_args(bad)


def test_host_entry_points_check_arguments_before_the_device():
    """Flow.fill and fill_flow raise for bad arguments without a device (this suite has none)"""
    f = of.Flow.zero((4, 6), 't')
    with pytest.raises(ValueError, match=r"\(4, 5\).*\(4, 6\)"):
        f.fill(valid=np.ones((4, 5), bool))
    with pytest.raises(ValueError):
        f.fill(valid=np.ones((4, 6, 1), bool))
    with pytest.raises(TypeError, match="float32"):
        f.fill(valid=np.ones((4, 6), np.float32))
    with pytest.raises(TypeError):
        f.fill(valid=np.ones((4, 6), np.int32))
    with pytest.raises(TypeError):
        f.fill(valid=[[True] * 6] * 4)
    with pytest.raises(ValueError):
        f.fill(max_dist=-1)
    with pytest.raises(TypeError):
        f.fill(max_dist="3")
    with pytest.raises(TypeError):
        f.fill(return_index=1)
    with pytest.raises(TypeError):
        f.fill(return_d2="yes")
    vecs, mask = np.zeros((4, 6, 2), np.float32), np.ones((4, 6), bool)
    with pytest.raises(ValueError):
        of.fill_flow(vecs, mask, valid=np.ones((6, 4), bool))
    with pytest.raises(TypeError):
        of.fill_flow(vecs, mask, valid=np.ones((4, 6), np.float64))
    with pytest.raises(ValueError):
        of.fill_flow(vecs, mask, max_dist=float('nan'))
    assert 'fill_flow' in of.flow_operations.__all__ and of.fill_flow is of.flow_operations.fill_flow
