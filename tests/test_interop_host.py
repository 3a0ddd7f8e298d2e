"""The host half of the exchange with other frameworks (K11): external_args against hand-made interface dicts, layout
inference, and the NumPy restatement of the conversions (tests/interop_ref.py) against torch on the CPU.  No GPU."""
import glob
import os
import re

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
import interop_ref as R


class Obj:
    def __init__(self, **cai):
        base = {"version": 3, "shape": (4, 6, 2), "typestr": "<f4", "data": (0x7f0000001000, False), "strides": None}
        base.update(cai)
        self.__cuda_array_interface__ = base


def test_reads_a_contiguous_and_a_strided_array():
    e = of.external_args(Obj())
    assert (e.ptr, e.shape, e.strides, e.dtype, e.itemsize, e.stream) == (0x7f0000001000, (4, 6, 2), (12, 2, 1), np.float32, 4, None)
    parent = np.zeros((6, 20, 3), np.float16)
    view = parent[1:5, 3::2, :2]
    e = dev.external_args(Obj(**R.cai_dict(view, 4096, version=2)))
    assert e.shape == (4, 9, 2) and e.strides == (60, 6, 1) and e.dtype == np.float16 and e.itemsize == 2
    # a broadcast dimension has stride 0; a dimension of size 1 is normalised to 0 whatever the producer reports
    e = dev.external_args(Obj(shape=(3, 1, 5), typestr="<f8", strides=(0, 123, 8)))
    assert e.strides == (0, 0, 1)
    for ts, dt in (("<f2", np.float16), ("<f8", np.float64), ("|u1", np.uint8), ("|b1", np.bool_), ("<i2", np.int16),
                   ("<u2", np.uint16), ("<i4", np.int32), ("<i8", np.int64), ("=f4", np.float32)):
        assert dev.external_args(Obj(typestr=ts)).dtype == dt


def test_type_errors():
    with pytest.raises(TypeError):
        dev.external_args(np.zeros((4, 6, 2), np.float32))            # no __cuda_array_interface__
    with pytest.raises(TypeError):
        dev.external_args(object())
    for ts in ("<c8", ">f4", "<f16", "|i1", "<u4", "<U3", 7, None):
        with pytest.raises(TypeError):
            dev.external_args(Obj(typestr=ts))
    with pytest.raises(TypeError):
        dev.external_args(Obj(version=1))
    with pytest.raises(TypeError):
        dev.external_args(Obj(), dtype='float16')                      # the array is float32
    with pytest.raises(TypeError):
        dev.external_args(Obj(), dtype='bfloat16')                     # bfloat16 rides in a 2-byte integer array
    with pytest.raises(TypeError):
        dev.external_args(Obj(), stream=1.5)


def test_value_errors():
    with pytest.raises(ValueError):
        dev.external_args(Obj(data=(0, False)))
    with pytest.raises(ValueError):
        dev.external_args(Obj(shape=(4, 0, 2)))
    with pytest.raises(ValueError):
        dev.external_args(Obj(strides=(48, 8, 2)))                     # 2 is no multiple of 4 bytes
    with pytest.raises(ValueError):
        dev.external_args(Obj(strides=(-48, 8, 4)))
    with pytest.raises(ValueError):
        dev.external_args(Obj(strides=(48, 8)))
    with pytest.raises(ValueError):
        dev.external_args(Obj(stream=0))
    with pytest.raises(ValueError):
        dev.external_args(Obj(), stream=0)


def test_bfloat16_rides_in_int16():
    for ts in ("<i2", "<u2"):
        e = dev.external_args(Obj(typestr=ts, strides=(48, 4, 2)), dtype='bfloat16')
        assert e.dtype == 'bfloat16' and e.itemsize == 2 and e.strides == (24, 2, 1)
    assert dev.external_args(Obj(typestr="<i2"), dtype='int16').dtype == np.int16


def test_stream_precedence():
    assert dev.external_args(Obj()).stream is None                                     # legacy default stream
    assert dev.external_args(Obj(version=2)).stream is None
    assert dev.external_args(Obj(stream=None)).stream is None
    assert dev.external_args(Obj(stream=1)).stream is None                             # 1 names the legacy default stream
    assert dev.external_args(Obj(stream=2)).stream == 2                                # the per-thread default stream
    assert dev.external_args(Obj(stream=0x5500)).stream == 0x5500
    assert dev.external_args(Obj(stream=0x5500), stream=0x6600).stream == 0x6600       # the argument wins
    assert dev.external_args(Obj(stream=0x5500), stream=1).stream is None
    assert dev.external_args(Obj(stream=0), stream=0x6600).stream == 0x6600            # ... before the entry is even looked at


def test_layout_inference():
    assert dev.flow_layout((4, 6, 2)) == 'hwc' and dev.flow_layout((2, 4, 6)) == 'chw'
    assert dev.flow_layout((3, 4, 6, 2)) == 'hwc' and dev.flow_layout((3, 2, 4, 6)) == 'chw'
    assert dev.flow_layout((2, 4, 6, 2)) == 'hwc'                      # N = 2 is not looked at
    for shape in ((2, 6, 2), (4, 6, 3), (5, 2, 6, 2)):
        with pytest.raises(ValueError, match="layout"):
            dev.flow_layout(shape)
    assert dev.flow_layout((2, 6, 2), 'hwc') == 'hwc' and dev.flow_layout((2, 6, 2), 'chw') == 'chw'
    with pytest.raises(ValueError):
        dev.flow_layout((4, 6, 2), 'chw')
    with pytest.raises(ValueError):
        dev.flow_layout((4, 6, 2), 'nhwc')


def test_image_layout():
    e = dev.external_args(Obj(shape=(3, 4, 6), typestr="|u1"))
    assert dev.image_layout(e, 'chw') == ((4, 6, 3), (6, 1, 24), False)
    assert dev.image_layout(e) == ((3, 4, 6), (24, 6, 1), True)
    assert dev.image_layout(dev.external_args(Obj(shape=(4, 6), typestr="<f8"))) == ((4, 6, 1), (6, 1, 0), True)
    with pytest.raises(TypeError):
        dev.image_layout(dev.external_args(Obj(typestr="<f2")))
    with pytest.raises(ValueError):
        dev.image_layout(dev.external_args(Obj(shape=(7, 4, 6), typestr="|u1")), 'chw')      # 7 channels to permute
    with pytest.raises(ValueError):
        dev.image_layout(dev.external_args(Obj(shape=(2, 3, 4, 6))))


def test_validation_comes_before_the_device():
    """what can be refused from the dict alone is refused without a device"""
    with pytest.raises(ValueError, match="layout"):
        of.DeviceFlow.from_external(Obj(shape=(2, 6, 2)))
    with pytest.raises(TypeError):
        of.DeviceFlow.from_external(Obj(typestr="<i4"))
    with pytest.raises(ValueError, match="copy=False"):
        of.DeviceFlow.from_external(Obj(shape=(2, 4, 6)), copy=False)
    with pytest.raises(ValueError):
        of.DeviceFlowBatch.from_external(Obj(), 't')                   # three dimensions are no batch
    with pytest.raises(ValueError):
        of.DeviceFlow.from_external(Obj(), ref='x')
    with pytest.raises(ValueError):
        of.DevicePoints.from_external(Obj(shape=(5, 3), typestr="<f8"))
    with pytest.raises(TypeError):
        of.DevicePoints.from_external(Obj(shape=(5, 2), typestr="<f4"))
    with pytest.raises(ValueError, match="copy=False"):
        of.DeviceImage.from_external(Obj(shape=(3, 4, 6)), layout='chw', copy=False)


def test_restatement_of_the_conversions():
    a = R.flow_values((3, 40), 'float32')
    b = R.f32_to_bf16(a)
    back = R.bf16_to_f32(b)
    assert np.array_equal(R.f32_to_bf16(back), b)                      # bfloat16 values are fixed points
    ok = np.isfinite(back) & (np.abs(a) >= 2.0 ** -126)                # normal numbers: half an ulp of 8 significant bits
    assert np.all(np.abs(back[ok] - a[ok]) <= np.abs(a[ok]) * 2.0 ** -8)
    one = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 3.4e38, np.nan, -np.nan, np.inf], np.float32)
    assert R.f32_to_bf16(one).tolist() == [0x3f80, 0x3f82, 0x7f80, 0x7fc0, 0x7fc0, 0x7f80]      # ties to even, overflow, NaN
    chw = R.flow_values((2, 5, 7), 'float64')
    assert np.array_equal(R.import_flow(chw, 'chw', 'float64')[3, 4], chw[:, 3, 4].astype(np.float32))
    v = R.import_flow(chw, 'chw', 'float64')
    assert np.array_equal(R.export_flow(v, 'chw', 'float32'), chw.astype(np.float32))
    img = np.arange(24).reshape(2, 3, 4)
    assert np.array_equal(R.to_chw(R.to_hwc(img)), img) and R.to_hwc(img)[2, 3, 1] == img[1, 2, 3]


def test_bfloat16_restatement_against_torch():
    torch = pytest.importorskip("torch")
    a = np.concatenate([R.flow_values((4096,), 'float32'), np.array([np.nan, np.inf, -np.inf], np.float32),
                        np.random.default_rng(5).integers(0, 1 << 32, 20000, dtype=np.uint32).view(np.float32)])
    want = torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = R.f32_to_bf16(a)
    nan = np.isnan(a)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.all((got[nan] & 0x7fff) > 0x7f80) and np.all((want[nan] & 0x7fff) > 0x7f80)      # NaN stays NaN, whatever its payload
    b = np.arange(1 << 16, dtype=np.uint16)
    back = torch.from_numpy(b.view(np.int16)).view(torch.bfloat16).float().numpy()
    assert np.array_equal(R.bits(R.bf16_to_f32(b)), R.bits(back))
    h = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    ok = ~np.isnan(h)                                                  # (signalling NaN payloads are quietened by some converters)
    assert np.array_equal(R.bits(R.to_f32(h, 'float16'))[ok], R.bits(torch.from_numpy(h).float().numpy())[ok])


def test_the_package_imports_no_framework():
    """the exchange reads and writes a dict of integers: no module of the package imports torch when it is loaded, and the
    modules the exchange lives in do not mention it at all"""
    here = os.path.dirname(os.path.abspath(of.__file__))
    for path in glob.glob(os.path.join(here, "*.py")):
        text = open(path).read()
        assert not re.search(r"^(import|from)\s+(torch|cupy|jax|numba)\b", text, flags=re.M), path
        if os.path.basename(path) in ("device.py", "interop.py", "memory.py", "batch.py", "_native.py", "__init__.py"):
            assert not re.search(r"^\s*(import|from)\s+(torch|cupy|jax|numba)\b", text, flags=re.M), path
