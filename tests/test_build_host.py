"""CPU suite: the host halves of the DeviceFlow constructors, scaling, padding and cropping (K9, ofl_build.hip).

The kernels are pinned to tests/build_ref.py on the GPU (test_gpu_build.py); here build_ref itself is pinned to the
reference's formulations -- utils.from_matrix bit for bit, np.pad, NumPy slicing -- and the argument checks are shown to raise
the reference's exception types before anything touches the device."""
import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev, utils
from oflibnumpy_amd.batch import DeviceFlowBatch
import build_ref as R


@pytest.mark.parametrize("name", list(R.MATRICES))
@pytest.mark.parametrize("ref", ['s', 't'])
def test_restatement_equals_from_matrix_bit_for_bit(name, ref):
    """matrix_args (the matrix and sign the kernel gets) + the kernel's operation order == utils.from_matrix, -0.0 included"""
    for shape in R.HOST_SHAPES:
        m, sign, got_ref = dev.matrix_args(R.MATRICES[name], shape, ref)
        assert got_ref == ref and sign == (1 if ref == 's' else -1) and m.dtype == np.float64 and m.flags.c_contiguous
        want = utils.from_matrix(R.MATRICES[name], shape, ref)
        got = R.flow_from_matrix(m, shape, sign)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(R.bits(got), R.bits(want)), (name, ref, shape)
        if R.TRANSFORMS[name] is not None:
            np.testing.assert_array_equal(R.bits(utils.from_transforms(R.TRANSFORMS[name], shape, ref)), R.bits(want))


def test_identity_target_reference_is_negative_zero():
    m, sign, _ = dev.matrix_args(np.eye(3), (2, 3), 't')
    got = R.flow_from_matrix(m, (2, 3), sign)
    assert np.array_equal(R.bits(got), R.bits(utils.from_matrix(np.eye(3), (2, 3), 't')))
    assert (R.bits(np.float32(0.0)) != R.bits(np.float32(-0.0))).all()          # the comparison does see the sign of a zero


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_reflection_map_equals_np_pad_symmetric(n):
    idx = np.arange(n)
    for before in range(0, 3 * n + 1):
        for after in (0, 1, n, 3 * n):
            s, inside = R.pad_index(n, before, after, dev._PAD_MODES['symmetric'])
            np.testing.assert_array_equal(s, np.pad(idx, (before, after), mode='symmetric'))
            np.testing.assert_array_equal(inside, np.pad(np.ones(n, bool), (before, after)))
            e, _ = R.pad_index(n, before, after, dev._PAD_MODES['edge'])
            np.testing.assert_array_equal(e, np.pad(idx, (before, after), mode='edge'))


@pytest.mark.parametrize("mode", ['constant', 'edge', 'symmetric'])
def test_pad_and_crop_maps_equal_the_host_flow(mode):
    rng = np.random.default_rng(0)
    v, m = rng.standard_normal((5, 4, 2)).astype(np.float32), rng.random((5, 4)) > 0.3
    f = of.Flow(v, 't', m)
    for p in ([0, 0, 0, 0], [1, 2, 3, 4], [13, 0, 0, 9], [0, 7, 5, 0]):
        want = f.pad(p, mode)
        gv, gm = R.pad(v, m, p, dev._PAD_MODES[mode])
        assert np.array_equal(R.bits(gv), R.bits(want.vecs)) and np.array_equal(gm, want.mask)
    for item in ((slice(2, 5), slice(None)), (slice(None, None, -1), slice(None, None, 3)), (slice(-3, None), slice(-2, None))):
        (r0, rs, rows), (c0, cs, cols) = dev.crop_args(item, f.shape)
        gv, gm = R.crop(v, m, *item)
        assert gv.shape[:2] == (rows, cols)
        assert np.array_equal(gv, f[item].vecs) and np.array_equal(gm, f[item].mask)
        assert np.array_equal(gv[0, 0], v[r0, c0]) and np.array_equal(gv[-1, -1], v[r0 + (rows - 1) * rs, c0 + (cols - 1) * cs])


def test_scale_operand_follows_numpy_promotion():
    shape = (5, 4)
    so = lambda o: dev.scale_operand(o, shape, "multiplying", "Multiplier")
    assert so(0.3) == (0.3, 0.3, 0) and so(-2) == (-2.0, -2.0, 0) and so(np.float64(0.3)) == (0.3, 0.3, 0)
    assert so([0.5, -2.0]) == (0.5, -2.0, 1) and so([2, 3]) == (2.0, 3.0, 1)
    assert so(np.array([3, 7])) == (3.0, 7.0, 1)
    k0, k1, wide = so(np.float32([0.1, 0.7]))
    assert wide == 0 and np.float32(k0) == np.float32(0.1) and np.float32(k1) == np.float32(0.7)
    assert so(np.array([3, 7], np.int16))[2] == 0 and so(np.array([3, 7], np.int32))[2] == 1       # NumPy: float32 / float64
    ones = np.ones((2, 2, 2), np.float32)
    assert (ones * 0.3).dtype == np.float32                                   # a Python number is a weak scalar
    for o in ([0.5, -2.0], [2, 3], np.array([3, 7]), np.float32([0.1, 0.7]), np.array([3, 7], np.int16), np.array([3, 7], np.int32)):
        assert so(o)[2] == int((ones * np.asarray(o)).dtype == np.float64), o


def test_constructor_validation_without_a_device():
    """the cases of the reference's tests/test_utils.py (from_matrix, from_transforms) and the Flow.mask setter"""
    D = dev.DeviceFlow
    shape, eye = (10, 12), np.eye(3)
    with pytest.raises(TypeError):
        D.from_matrix('m', shape, 't')
    with pytest.raises(TypeError):
        D.from_matrix([[1, 0, 0], [0, 1, 0], [0, 0, 1]], shape, 't')
    with pytest.raises(ValueError):
        D.from_matrix(np.eye(4), shape, 't')
    with pytest.raises(ValueError):
        D.from_matrix(np.eye(3)[None], shape, 't')
    for make in (lambda s, r: D.from_matrix(eye, s, r), lambda s, r: D.from_transforms([['translation', 1, 2]], s, r),
                 lambda s, r: D.zero(s, r), lambda s, r: DeviceFlowBatch.from_matrices(eye[None], s, r)):
        with pytest.raises(TypeError):
            make(3, 't')
        with pytest.raises(ValueError):
            make((0, 3), 't')
        with pytest.raises(ValueError):
            make((3, 4, 5), 't')
        with pytest.raises(ValueError):
            make((3.0, 4), 't')
        with pytest.raises(TypeError):
            make(shape, 0)
        with pytest.raises(ValueError):
            make(shape, 'x')
    with pytest.raises(TypeError):
        D.from_transforms('t', shape, 't')
    with pytest.raises(TypeError):
        D.from_transforms(['rotation', 1, 2, 3], shape, 't')
    with pytest.raises(ValueError):
        D.from_transforms([['rotation', 1, 2]], shape, 't')
    with pytest.raises(ValueError):
        D.from_transforms([['shear', 1, 2]], shape, 't')
    with pytest.raises(ValueError):
        D.from_transforms([['translation', 1, 'a']], shape, 't')
    with pytest.raises(ValueError):
        D.from_transforms([['translation']], shape, 't')
    for make in (lambda m: D.from_matrix(eye, shape, 't', m), lambda m: D.zero(shape, 't', m)):
        with pytest.raises(TypeError):
            make('m')
        with pytest.raises(ValueError):
            make(np.ones((10, 12, 1)))
        with pytest.raises(ValueError):
            make(np.ones((11, 12)))
        with pytest.raises(ValueError):
            make(np.full((10, 12), 2))
    with pytest.raises(TypeError):
        DeviceFlowBatch.from_matrices([eye], shape, 't')
    with pytest.raises(ValueError):
        DeviceFlowBatch.from_matrices(eye, shape, 't')
    with pytest.raises(ValueError):
        DeviceFlowBatch.from_matrices(np.zeros((0, 3, 3)), shape, 't')


def test_operator_validation_without_a_device():
    """the error types of Flow._broadcast_operand, Flow.pad and the slicing rules, on a DeviceFlow that holds no buffers"""
    f = dev.DeviceFlow(None, None, (8, 9), 't')
    for op in (lambda o: f * o, lambda o: f / o):
        with pytest.raises(ValueError):
            op([1, 2, 3])
        with pytest.raises(ValueError):      # float('x') raises ValueError in the reference too
            op('x')
        with pytest.raises(TypeError):
            op({})
        with pytest.raises(ValueError):
            op(np.zeros((3, 3)))
        with pytest.raises(ValueError):
            op(np.zeros(3))
        with pytest.raises(TypeError):
            op(np.array(['a', 'b']))
        with pytest.raises(TypeError):
            op(np.array([1j, 2]))
        with pytest.raises(TypeError, match="host Flow"):
            op(np.ones((8, 9)))
        with pytest.raises(TypeError, match="host Flow"):
            op(np.ones((8, 9, 2)))
    with pytest.raises(TypeError):
        {} * f
    with pytest.raises(TypeError, match="host Flow"):
        f ** 2
    with pytest.raises(ValueError):
        f.pad([1, 2, 3, 4], 'wrap')
    with pytest.raises(TypeError):
        f.pad(3)
    with pytest.raises(ValueError):
        f.pad([1, 2, 3])
    with pytest.raises(ValueError):
        f.pad([1., 2, 3, 4])
    with pytest.raises(ValueError):
        f.pad([-1, 2, 3, 4])
    assert f.pad([0, 0, 0, 0]) is f and f.pad((0, 0, 0, 0), 'edge') is f
    for bad in (3, (2, 3), (slice(None), 3), [1, 2], np.arange(3), Ellipsis, (slice(None),) * 3, ()):
        with pytest.raises(TypeError):
            f[bad]
    with pytest.raises(ValueError):
        f[5:2]
    with pytest.raises(ValueError):
        f[:, 9:]
    with pytest.raises(ValueError):
        f[::0]
    assert dev.crop_args(slice(2, 5), (8, 9)) == ((2, 1, 3), (0, 1, 9))
    assert dev.crop_args((slice(None, None, -1), slice(None, None, 3)), (8, 9)) == ((7, -1, 8), (0, 3, 3))
    assert dev.crop_args((slice(10, 2, -3), slice(-2, None)), (33, 130)) == ((10, -3, 3), (128, 1, 2))


def test_new_entries_check_device_and_arguments():
    """no CPU fallback: without a device every new entry answers OFL_E_NODEVICE; with one, NULL pointers are OFL_E_INVALID"""
    from oflibnumpy_amd import _native as nat
    lib = nat.load()
    want = nat.E_NODEVICE
    if nat.device_count() > 0:
        nat.ensure_device()
        want = nat.E_INVALID
    assert lib.ofl_flow_from_matrix_dev(None, 1, 1, 4, 4, None, None) == want
    assert lib.ofl_scale_dev(None, 1.0, 1.0, 0, 0, 16, None, None) == want
    assert lib.ofl_pad_flow_dev(None, None, 4, 4, 1, 1, 1, 1, 0, None, None, None) == want
    assert lib.ofl_crop_flow_dev(None, None, 4, 4, 0, 1, 4, 0, 1, 4, None, None, None) == want
    if want == nat.E_NODEVICE:
        with pytest.raises(nat.NoDeviceError):
            dev.DeviceFlow.from_transforms([['rotation', 5, 5, 20]], (16, 20), 't')
