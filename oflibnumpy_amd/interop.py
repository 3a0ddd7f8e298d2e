"""K11: exchange of device-resident fields, masks, images and points with other frameworks.  Ingress and egress over the
CUDA Array Interface (ROCm frameworks expose it under that name).  The package imports no framework: it reads and writes a
dict of integers.
"""
import ctypes

import numpy as np

from . import _native as nat
from .memory import DeviceBuffer, _BufferView, _lib, _ptr, sync
from .args import _DT_CODE
from .kernels import _valid_mask, _mask_buffer

_CAI_TYPES = {'f2': 'float16', 'f4': 'float32', 'f8': 'float64', 'u1': 'uint8', 'b1': 'bool', 'i2': 'int16', 'u2': 'uint16',
              'i4': 'int32', 'i8': 'int64'}
_EL_CODE = {'float16': nat.EL_F16, 'bfloat16': nat.EL_BF16, 'float32': nat.EL_F32, 'float64': nat.EL_F64}
_EL_TYPESTR = {'float16': '<f2', 'bfloat16': '<i2', 'float32': '<f4'}


class External:
    """What external_args reads from an interface dict: `ptr`, `shape`, `strides` in ELEMENTS (0 for a dimension of size 1),
    `dtype` (a NumPy dtype, or the string 'bfloat16'), `itemsize`, `stream` (the producer's stream handle; None = the legacy
    default stream, 2 = the per-thread default stream)."""

    __slots__ = ("ptr", "shape", "strides", "dtype", "itemsize", "stream")

    def __init__(self, ptr, shape, strides, dtype, itemsize, stream):
        self.ptr, self.shape, self.strides, self.dtype, self.itemsize, self.stream = ptr, shape, strides, dtype, itemsize, stream


def external_args(obj, dtype=None, stream=None):
    """`obj.__cuda_array_interface__` (version 2 or 3) -> External.  Pure: no device is touched.
    TypeError: no such attribute, an unsupported version or typestr, a `dtype` the array is not.  ValueError: a null pointer,
    a zero-sized dimension, a negative byte stride or one that is no multiple of the item size, a stream entry of 0.
    dtype='bfloat16' reinterprets a 2-byte integer array (the interface has no bfloat16: t.view(torch.int16)).
    The producer's stream: `stream` (an integer handle) if given, else the interface's 'stream' entry, else the legacy default
    stream; 1 names the legacy default stream, 2 the per-thread default stream, any other value is a handle."""
    cai = getattr(obj, "__cuda_array_interface__", None)
    if not isinstance(cai, dict):
        raise TypeError("Error taking an external array: {} has no __cuda_array_interface__".format(type(obj).__name__))
    if cai.get("version") not in (2, 3):
        raise TypeError("Error taking an external array: __cuda_array_interface__ version {!r} is not 2 or 3".format(cai.get("version")))
    typestr = cai.get("typestr")
    if not isinstance(typestr, str) or typestr[:1] not in ('<', '|', '=') or typestr[1:] not in _CAI_TYPES:
        raise TypeError("Error taking an external array: unsupported typestr {!r}".format(typestr))
    dt = np.dtype(_CAI_TYPES[typestr[1:]])
    if dtype is not None:
        if str(dtype) == 'bfloat16':
            if dt not in (np.int16, np.uint16):
                raise TypeError("Error taking an external array: dtype='bfloat16' reinterprets a 2-byte integer array, got {}".format(dt))
            dt = 'bfloat16'
        elif np.dtype(dtype) != dt:
            raise TypeError("Error taking an external array: the array is {}, not {}".format(dt, np.dtype(dtype)))
    itemsize = 2 if isinstance(dt, str) else dt.itemsize
    shape = tuple(int(v) for v in cai["shape"])
    if any(v <= 0 for v in shape):
        raise ValueError("Error taking an external array: zero-sized dimension in shape {}".format(shape))
    data = cai.get("data")
    ptr = int(data[0]) if isinstance(data, (tuple, list)) and data and data[0] is not None else 0
    if ptr == 0:
        raise ValueError("Error taking an external array: null data pointer")
    strides = cai.get("strides")
    if strides is None:
        strides, run = [], 1
        for v in reversed(shape):
            strides.append(run if v > 1 else 0)
            run *= v
        strides = tuple(reversed(strides))
    else:
        if len(strides) != len(shape):
            raise ValueError("Error taking an external array: {} strides for {} dimensions".format(len(strides), len(shape)))
        out = []
        for v, b in zip(shape, strides):
            b = int(b)
            if v == 1:
                out.append(0)
                continue
            if b < 0:
                raise ValueError("Error taking an external array: negative stride {} (make the view contiguous first)".format(b))
            if b % itemsize:
                raise ValueError("Error taking an external array: byte stride {} is no multiple of the item size {}".format(b, itemsize))
            out.append(b // itemsize)
        strides = tuple(out)
    if stream is not None:
        if isinstance(stream, bool) or not isinstance(stream, int):
            raise TypeError("Error taking an external array: stream must be an integer handle, got {}".format(type(stream).__name__))
        s = stream
    else:
        s = cai.get("stream")
    if s is not None:
        s = int(s)
        if s == 0:
            raise ValueError("Error taking an external array: stream 0 is ambiguous (1 = legacy default, 2 = per-thread default)")
        if s == 1:
            s = None
    return External(ptr, shape, strides, dt, itemsize, s)


def _contiguous(shape, strides):
    run = 1
    for v, st in zip(reversed(shape), reversed(strides)):
        if v > 1 and st != run:
            return False
        run *= v
    return True


def flow_layout(shape, layout=None):
    """'hwc' or 'chw' for vectors of `shape` ((H, W, 2) / (2, H, W), with a leading N for a batch): `layout` checked against
    the shape, or inferred when exactly one of the first and last field dimensions is 2."""
    first, last = shape[-3], shape[-1]
    if layout is None:
        if (first == 2) == (last == 2):
            raise ValueError("Error taking external flow vectors: cannot tell the layout of shape {} -- pass layout='hwc' "
                             "(H, W, 2) or layout='chw' (2, H, W)".format(tuple(shape)))
        return 'chw' if first == 2 else 'hwc'
    if layout not in ('hwc', 'chw'):
        raise ValueError("Error taking external flow vectors: layout must be 'hwc' or 'chw', got {!r}".format(layout))
    if (first if layout == 'chw' else last) != 2:
        raise ValueError("Error taking external flow vectors: shape {} does not have 2 channels in layout '{}'".format(tuple(shape), layout))
    return layout


def image_layout(ext, layout=None):
    """An external image -> ((H, W, C), element strides (row, column, channel), is it C-contiguous [H][W][C])."""
    if ext.dtype not in _DT_CODE:
        raise TypeError("warp targets must be uint8, int16, uint16, float32 or float64 "
                        "(what cv2.remap accepts), got {}".format(ext.dtype))
    if layout not in (None, 'hwc', 'chw'):
        raise ValueError("Error taking an external image: layout must be 'hwc' or 'chw', got {!r}".format(layout))
    if len(ext.shape) == 2 and layout != 'chw':
        shape, st = ext.shape + (1,), ext.strides + (0,)
    elif len(ext.shape) == 3 and layout == 'chw':
        shape, st = ext.shape[1:] + ext.shape[:1], ext.strides[1:] + ext.strides[:1]
    elif len(ext.shape) == 3:
        shape, st = ext.shape, ext.strides
    else:
        raise ValueError("Error taking an external image: shape {} is not (H, W, C), (H, W) or, with layout='chw', (C, H, W)".format(ext.shape))
    contiguous = _contiguous(shape, st)
    if not contiguous and not 1 <= shape[2] <= 6:
        raise ValueError("Error taking an external image: the layout conversion takes 1 to 6 channels, got {}".format(shape[2]))
    return shape, st, contiguous


def _check_device_memory(ext):
    """ValueError unless the first and the last byte the strides reach are device memory of the engine's device; no kernel is
    launched before this has passed.  Only the two ENDS are asked about: a view whose ends lie in two different allocations
    of the device with a gap between them would pass.  The interface gives no allocation to compare against; a producer that
    describes its own array correctly cannot produce such a view."""
    device = nat.ensure_device()
    last = sum((v - 1) * st for v, st in zip(ext.shape, ext.strides)) * ext.itemsize + ext.itemsize - 1
    is_dev, where = ctypes.c_int(0), ctypes.c_int(-1)
    for p in (ext.ptr, ext.ptr + last):
        nat.check(_lib().ofl_pointer_info(p, ctypes.byref(is_dev), ctypes.byref(where)))
        if not is_dev.value:
            raise ValueError("Error taking an external array: address {:#x} is not device memory".format(p))
        if where.value != device:
            raise ValueError("Error taking an external array: address {:#x} is memory of device {}, the engine runs on device {}"
                             .format(p, where.value, device))


def _wait_for(*producers):
    """The library's stream waits (on the device) for each distinct producer stream: ofl_stream_wait_external."""
    for s in set(producers):
        nat.check(_lib().ofl_stream_wait_external(s, None))


def import_flow_launch(src_ptr, elem, strides, n, h, w, mask_ptr, mask_strides, out_vecs, out_mask, counters, stream=None):
    """K11 import (ofl_import_flow_dev); asynchronous.  strides: (field, channel, row, column) in elements; mask_strides:
    (field, row, column); out_vecs / out_mask / counters: buffers or None."""
    ms = mask_strides if mask_strides is not None else (0, 0, 0)
    nat.check(_lib().ofl_import_flow_dev(src_ptr, elem, strides[0], strides[1], strides[2], strides[3], n, h, w, mask_ptr,
                                         ms[0], ms[1], ms[2], _ptr(out_vecs), _ptr(out_mask), _ptr(counters), stream))


def import_flow(vecs, mask, layout, dtype, stream, copy, check_finite, batch):
    """The work behind DeviceFlow.from_external and DeviceFlowBatch.from_external -> (vecs buffer, mask buffer, n, (H, W)); the
    views of an adopted field carry the producer's objects as their `owner`.  Everything that can be refused without the device is refused
    first; then the pointer checks, the stream wait and one launch."""
    ext = external_args(vecs, dtype, stream)
    name = ext.dtype if isinstance(ext.dtype, str) else ext.dtype.name
    if name not in _EL_CODE:
        raise TypeError("Error taking external flow vectors: float16, float32, float64 or (dtype='bfloat16') bfloat16, got {}".format(name))
    if len(ext.shape) != (4 if batch else 3):
        raise ValueError("Error taking external flow vectors: shape {} is not {}".format(
            ext.shape, "(N, H, W, 2) or (N, 2, H, W)" if batch else "(H, W, 2) or (2, H, W)"))
    lay = flow_layout(ext.shape, layout)
    shape, st = (ext.shape, ext.strides) if batch else ((1,) + ext.shape, (0,) + ext.strides)
    n = shape[0]
    if lay == 'hwc':
        (h, w), strides = shape[1:3], (st[0], st[3], st[1], st[2])
    else:
        (h, w), strides = shape[2:4], st
    px = h * w
    mext, mbuf, mstrides = None, None, None
    if mask is not None and not isinstance(mask, (np.ndarray, DeviceBuffer, _BufferView)) and hasattr(mask, "__cuda_array_interface__"):
        mext = external_args(mask, None, stream)
        if mext.dtype not in (np.bool_, np.uint8):
            raise TypeError("Error setting flow mask: an external mask needs to be bool or uint8, got {}".format(mext.dtype))
        if mext.shape != ((n, h, w) if batch else (h, w)):
            raise ValueError("Error setting flow mask: Input has a different shape than the flow vectors")
        mstrides = mext.strides if batch else (0,) + mext.strides
    elif mask is not None:
        if batch:
            if not isinstance(mask, (DeviceBuffer, _BufferView)) or mask.nbytes < n * px:
                raise TypeError("Error setting flow mask: the masks of a batch are an external (N, H, W) array, a DeviceBuffer of "
                                "N * H * W bytes or None")
            mbuf = mask
        else:
            mbuf = _valid_mask(mask, (h, w))
        mstrides = (px, w, 1)
    if not copy:
        if batch or lay != 'hwc' or name != 'float32' or not _contiguous(ext.shape, ext.strides) or ext.ptr % 16:
            raise ValueError("Error taking external flow vectors: copy=False adopts C-contiguous (H, W, 2) float32 at a 16-byte "
                             "aligned address only; anything else needs the converting copy")
        if mext is not None and not _contiguous(mext.shape, mext.strides):
            raise ValueError("Error setting flow mask: copy=False adopts a C-contiguous external mask only")
    _check_device_memory(ext)
    if mext is not None:
        _check_device_memory(mext)
    _wait_for(*([ext.stream] + ([mext.stream] if mext is not None else [])))
    if isinstance(mbuf, np.ndarray):
        mbuf = DeviceBuffer.from_host(mbuf)
    mptr = _ptr(mext if mext is not None else mbuf)
    counters = DeviceBuffer.zeros(16) if check_finite else None
    if copy:
        out_v, out_m = DeviceBuffer(n * px * 8), DeviceBuffer(n * px)
        import_flow_launch(ext.ptr, _EL_CODE[name], strides, n, h, w, mptr, mstrides, out_v, out_m, counters)
    else:
        out_v = _BufferView(ext.ptr, px * 8, owner=vecs)      # the owner rides on the view: whoever shares it keeps the producer alive
        if mext is not None:
            out_m = _BufferView(mext.ptr, px, owner=mask)
        else:
            out_m = mbuf if mbuf is not None else _mask_buffer(None, (h, w))
        if check_finite:
            import_flow_launch(ext.ptr, _EL_CODE[name], strides, n, h, w, mptr, mstrides, None, None, counters)
    if check_finite:
        bad = counters.to_host((2,), np.uint32)
        if bad[0]:
            raise ValueError("Error setting flow vectors: Flow array contains NaN or Inf values")
        if bad[1]:
            raise ValueError("Error setting flow mask: Values must be 0 or 1")
    return out_v, out_m, n, (h, w)


class DeviceArray:
    """A result handed to another framework: a buffer (kept alive by this object), a shape and a typestr behind
    `__cuda_array_interface__` (version 3, C-contiguous, writable, no stream entry).  Reading the attribute synchronises the
    library's stream, once per object: after that the memory holds the result and the consumer needs no further ordering --
    torch.as_tensor(a, device='cuda') ignores a stream entry anyway, and rejects a read-only flag.  The consumer's array
    refers to this object, and so keeps the memory alive."""

    def __init__(self, buf, shape, typestr, owner=None):
        self.buf, self.shape, self.typestr, self._owner = buf, tuple(int(v) for v in shape), typestr, owner
        self._synced = False

    @property
    def __cuda_array_interface__(self):
        if not self._synced:
            sync()
            self._synced = True
        return {"version": 3, "shape": self.shape, "typestr": self.typestr, "data": (self.buf.ptr, False), "strides": None,
                "stream": None}

    def to_host(self):
        dt = np.dtype(self.typestr)
        return self.buf.to_host(self.shape, dt)


def export_buffer(buf, shape, typestr, copy, owner):
    """`buf` as a DeviceArray of `shape` and `typestr` with nothing converted: a device copy in a fresh buffer or, with
    copy=False, a view of the memory itself, which keeps `owner` alive and which the consumer must not write."""
    if not copy:
        return DeviceArray(buf, shape, typestr, owner=owner)
    nbytes = int(np.prod(shape)) * np.dtype(typestr).itemsize
    dst = DeviceBuffer(nbytes)
    nat.check(_lib().ofl_copy_dev(dst.ptr, buf.ptr, nbytes, None))
    return DeviceArray(dst, shape, typestr)


def export_flow(vecs, n, shape, layout, dtype, copy, owner, batch=False):
    """K11 export of `n` fields (ofl_export_flow_dev) -> DeviceArray, with a leading dimension n for a batch."""
    if layout not in ('hwc', 'chw'):
        raise ValueError("Error exporting flow: layout must be 'hwc' or 'chw', got {!r}".format(layout))
    name = 'bfloat16' if str(dtype) == 'bfloat16' else np.dtype(dtype).name
    if name not in _EL_TYPESTR:
        raise TypeError("Error exporting flow: dtype must be float32, float16 or bfloat16, got {}".format(name))
    h, w = shape
    lead = (n,) if batch else ()
    out_shape = lead + ((h, w, 2) if layout == 'hwc' else (2, h, w))
    if not copy:
        if layout != 'hwc' or name != 'float32':
            raise ValueError("Error exporting flow: copy=False hands out the field's own (H, W, 2) float32 memory; "
                             "'{}' {} is a conversion".format(layout, name))
        return export_buffer(vecs, out_shape, '<f4', False, owner)
    itemsize = 4 if name == 'float32' else 2
    dst = DeviceBuffer(n * h * w * 2 * itemsize)
    nat.check(_lib().ofl_export_flow_dev(vecs.ptr, n, h, w, _EL_CODE[name], 1 if layout == 'chw' else 0, dst.ptr, None))
    return DeviceArray(dst, out_shape, _EL_TYPESTR[name])


def export_mask(mask, shape, copy, owner):
    """uint8 0 / 1 masks -> DeviceArray of bool with `shape`: a device copy, or a view of the mask's own memory."""
    return export_buffer(mask, shape, '|b1', copy, owner)
