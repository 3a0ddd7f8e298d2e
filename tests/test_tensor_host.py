"""Host halves of the tensor warp (K12): every argument error is raised before the device is touched -- this file runs
without a GPU -- and the NumPy reference tests/tensor_ref.py agrees with the oracle's multi-channel gather."""
import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import args, device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
import interop_ref as R
import tensor_ref as T

nat = of.native


class Fake:
    """an object that describes device memory which is never touched: every error below comes before the first device call"""

    def __init__(self, view):
        self.__cuda_array_interface__ = R.cai_dict(view, 0x7f0000001000)


def field(shape, ref='t'):
    return dev.DeviceFlow(None, None, shape, ref)


def batch(n, shape, ref='t'):
    return DeviceFlowBatch.wrap(n, shape, ref, None, None)


def test_tensor_args_accepts_and_decodes():
    assert args.tensor_args((7, 5, 9), 'chw', 'float16') == (1, 7, 5, 9, False)
    assert args.tensor_args((3, 7, 5, 9), 'hwc', 'bfloat16', (5, 9)) == (3, 7, 5, 9, True)
    assert args.tensor_logical_shape((5, 9, 7), 'hwc') == (7, 5, 9) and args.tensor_mem_shape((3, 7, 5, 9), 'hwc') == (3, 5, 9, 7)
    assert args.tensor_dtype(np.dtype('int16'), 'bfloat16') == 'bfloat16' and args.tensor_dtype(np.dtype('float32')) == 'float32'
    t = dev.DeviceTensor(None, (3, 7, 5, 9), 'float16', 'hwc')
    assert (t.n, t.channels, t.h, t.w, t.batched, t.nbytes) == (3, 7, 5, 9, True, 3 * 7 * 5 * 9 * 2)


def test_wrong_rank():
    for shape in [(5, 9), (1, 2, 3, 4, 5)]:
        with pytest.raises(ValueError, match="shape"):
            args.tensor_args(shape, 'chw', 'float32')
        with pytest.raises(ValueError, match="shape"):
            dev.DeviceTensor(None, shape, 'float32', 'chw')
        with pytest.raises(ValueError, match="shape"):
            dev.DeviceTensor.from_host(np.zeros(shape, np.float32))
        with pytest.raises(ValueError, match="shape"):
            dev.DeviceTensor.from_external(Fake(np.zeros(shape, np.float32)))


def test_spatial_mismatch():
    t = dev.DeviceTensor(None, (7, 5, 9), 'float32', 'chw')
    with pytest.raises(ValueError, match="same height and width"):
        args.tensor_args(t.shape, 'chw', 'float32', (5, 8))
    with pytest.raises(ValueError, match="same height and width"):
        field((9, 5)).apply_tensor(t)
    tb = dev.DeviceTensor(None, (3, 7, 5, 9), 'float32', 'hwc')
    with pytest.raises(ValueError, match="same height and width"):
        batch(3, (6, 9)).apply_tensors(tb)
    with pytest.raises(ValueError, match="one item per field"):
        batch(4, (5, 9)).apply_tensors(tb)
    with pytest.raises(ValueError, match="one item per field"):
        batch(1, (5, 9)).apply_tensors(t)


def test_wrong_layout_string():
    for layout in ('nchw', 'HWC', None, 0):
        with pytest.raises(ValueError, match="layout"):
            args.tensor_args((7, 5, 9), layout, 'float32')
        with pytest.raises(ValueError, match="layout"):
            dev.DeviceTensor(None, (7, 5, 9), 'float32', layout)
        if layout is not None:
            with pytest.raises(ValueError, match="layout"):
                dev.DeviceTensor.from_host(np.zeros((7, 5, 9), np.float32), layout=layout)
            with pytest.raises(ValueError, match="layout"):
                dev.DeviceTensor.from_external(Fake(np.zeros((7, 5, 9), np.float32)), layout=layout)
    with pytest.raises(ValueError, match="layout"):
        dev.DeviceTensor(None, (7, 5, 9), 'float32', 'chw').export('nhwc')


def test_wrong_dtypes():
    with pytest.raises(TypeError, match="float64"):
        dev.DeviceTensor.from_host(np.zeros((7, 5, 9), np.float64))
    with pytest.raises(TypeError, match="float64"):
        dev.DeviceTensor.from_external(Fake(np.zeros((7, 5, 9), np.float64)))
    with pytest.raises(TypeError):
        dev.DeviceTensor(None, (7, 5, 9), 'float64', 'chw')
    for dt in (np.int16, np.uint16, np.uint8, np.int32):             # an integer array without dtype='bfloat16'
        with pytest.raises(TypeError):
            dev.DeviceTensor.from_host(np.zeros((7, 5, 9), dt))
        with pytest.raises(TypeError):
            dev.DeviceTensor.from_external(Fake(np.zeros((7, 5, 9), dt)))
    for dt in (np.uint8, np.int32, np.float16):                      # dtype='bfloat16' on anything but a 2-byte integer array
        with pytest.raises(TypeError, match="bfloat16"):
            dev.DeviceTensor.from_host(np.zeros((7, 5, 9), dt), dtype='bfloat16')
        with pytest.raises(TypeError, match="bfloat16"):
            dev.DeviceTensor.from_external(Fake(np.zeros((7, 5, 9), dt)), dtype='bfloat16')
    with pytest.raises(TypeError, match="not float16"):
        dev.DeviceTensor.from_host(np.zeros((7, 5, 9), np.float32), dtype='float16')


def test_limits():
    with pytest.raises(ValueError, match="65535"):
        args.tensor_args((65536, 5, 9), 'chw', 'float32')
    with pytest.raises(ValueError, match="65535"):
        args.tensor_args((65536, 2, 5, 9), 'chw', 'float32')
    with pytest.raises(ValueError, match="32766"):
        args.tensor_args((2, 32767, 9), 'chw', 'float32')


def test_s_reference_fields_are_refused():
    t = dev.DeviceTensor(None, (7, 5, 9), 'float32', 'chw')
    with pytest.raises(ValueError, match="'s'-reference"):
        field((5, 9), 's').apply_tensor(t)
    with pytest.raises(ValueError, match="'s'-reference"):
        batch(3, (5, 9), 's').apply_tensors(dev.DeviceTensor(None, (3, 7, 5, 9), 'float32', 'chw'))


def test_the_batch_call_takes_the_opencv_quantisation_only():
    with pytest.raises(ValueError, match="QUANT_OPENCV"):
        batch(3, (5, 9)).apply_tensors(dev.DeviceTensor(None, (3, 7, 5, 9), 'float32', 'chw'), quant=nat.QUANT_EXACT)


def test_copy_false_on_a_strided_source():
    parent = np.zeros((2, 8, 5, 9), np.float16)
    for view in (parent[:, 1::2], parent[:, :, 1:4, 2:7]):
        with pytest.raises(ValueError, match="copy=False"):
            dev.DeviceTensor.from_external(Fake(view), copy=False)
    with pytest.raises(ValueError, match="copy=False"):
        dev.DeviceTensor(None, (7, 5, 9), 'float32', 'chw').export('hwc', copy=False)


def test_the_reference_equals_the_oracles_three_channel_gather(oracle):
    h, w = 37, 53
    chw = T.values((3, h, w), 'float32', seed=1)
    vecs = T.flow('rotation', (h, w))
    fmask, tmask = T.mask((h, w), 2), T.mask((h, w), 3)
    for quant in (oracle.QUANT_OPENCV, oracle.QUANT_EXACT):
        want, ok = oracle.gather_bilinear(R.to_hwc(chw), vecs, -1, smask=tmask, want_valid=True, quant=quant)
        for layout, arr in (('chw', chw), ('hwc', R.to_hwc(chw))):
            got, valid = T.warp(arr, 'float32', layout, vecs, fmask, tmask, quant)
            assert np.array_equal(T.raw(T.to_planar(got, layout)[0]), T.raw(R.to_chw(want)))
            assert np.array_equal(valid, ok & fmask)
    assert not ok.all() and ok.any()
