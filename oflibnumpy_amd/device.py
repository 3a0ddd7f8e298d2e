"""HBM-resident flow fields and the device-side flow algebra.

`DeviceFlow` mirrors the hot-path methods of the reference's `Flow` (apply / switch_ref / invert /
combine_with / valid_target / valid_source / + - neg / is_zero / visualise, and the constructors zero / from_matrix /
from_transforms, * / by a factor, pad and slicing; src/oflibnumpy/flow_class.py) but
keeps vectors and mask in GPU memory between operations, so chains such as combine_with(mode=1)
(1 scatter + 2 gathers, flow_class.py:1369-1370) never cross PCIe.  The host `Flow` class is a thin
upload -> DeviceFlow op -> download wrapper around this module.

This layer is SINGLE-STREAM: recycled buffers (`_Pool`) and the one scatter workspace per shape are handed out as soon
as Python drops them, which is only safe while all work is queued on one stream (the library's default).  The `stream`
arguments exist for callers that manage their own buffers at the C level.

Data layout in HBM: vecs float32 [H][W][2] interleaved (x, y) -- the same layout as the reference,
so a pixel's vector is one 8-byte element and two horizontally adjacent bilinear taps are one
16-byte load; mask uint8 [H][W] (0/1).
"""
import ctypes
import weakref

import numpy as np

from . import _native as nat

DEFAULT_THRESHOLD = 1e-3          # src/oflibnumpy/utils.py:22
_DT_CODE = {np.dtype('uint8'): nat.U8, np.dtype('int16'): nat.I16, np.dtype('uint16'): nat.U16,
            np.dtype('float32'): nat.F32, np.dtype('float64'): nat.F64}


def _lib():
    nat.ensure_device()
    return nat.load()


# ------------------------------------------------------------------------------ memory
class _Pool:
    """Size-bucketed free lists: hipFree synchronises the device, so chained operations recycle
    their intermediates instead of returning them to the driver."""

    def __init__(self):
        self.free = {}
        self.cached_bytes = 0
        self.limit = 64 << 30

    def take(self, nbytes):
        lst = self.free.get(nbytes)
        if lst:
            self.cached_bytes -= nbytes
            return lst.pop()
        p = ctypes.c_void_p()
        try:
            nat.check(_lib().ofl_malloc(ctypes.byref(p), nbytes))
        except nat.NativeError:
            self.trim()
            nat.check(_lib().ofl_malloc(ctypes.byref(p), nbytes))
        return p.value

    def give(self, ptr, nbytes):
        if self.cached_bytes + nbytes > self.limit:
            nat.load().ofl_free(ptr)
            return
        self.free.setdefault(nbytes, []).append(ptr)
        self.cached_bytes += nbytes

    def trim(self):
        lib = nat.load()
        for lst in self.free.values():
            for p in lst:
                lib.ofl_free(p)
        self.free.clear()
        self.cached_bytes = 0


_pool = _Pool()


def empty_cache():
    _pool.trim()


def _release(ptr, nbytes):
    try:
        _pool.give(ptr, nbytes)
    except Exception:       # interpreter shutdown
        pass


class DeviceBuffer:
    """A block of HBM owned by this process (ofl_malloc / pooled)."""

    __slots__ = ("ptr", "nbytes", "_fin", "__weakref__")

    def __init__(self, nbytes):
        self.nbytes = max(int(nbytes), 16)
        self.ptr = _pool.take(self.nbytes)
        self._fin = weakref.finalize(self, _release, self.ptr, self.nbytes)

    @classmethod
    def from_host(cls, arr, stream=None):
        arr = np.ascontiguousarray(arr)
        buf = cls(arr.nbytes)
        if arr.nbytes:
            nat.check(_lib().ofl_upload(buf.ptr, arr.ctypes.data, arr.nbytes, stream))
            # the source array may be a temporary: make the (possibly staged) copy complete now
            nat.check(_lib().ofl_stream_sync(stream))
        return buf

    @classmethod
    def zeros(cls, nbytes, stream=None):
        buf = cls(nbytes)
        nat.check(_lib().ofl_memset(buf.ptr, 0, buf.nbytes, stream))
        return buf

    def to_host(self, shape, dtype, stream=None):
        """Download into a fresh array.  Large results land in page-locked memory from a recycling pool (a DMA at link
        speed; a pageable destination of fresh pages costs 2-3 x as long in page faults) -- the array owns its block and
        returns it to the pool when it is garbage-collected."""
        return _download(self.ptr, shape, dtype, stream)


def _download(ptr, shape, dtype, stream=None):
    """Device memory at `ptr` -> a fresh array (what DeviceBuffer.to_host and _BufferView.to_host do)."""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    if nbytes >= _PINNED_MIN:
        out = _pinned_pool.array(shape, dtype)
        if out is not None:
            nat.check(_lib().ofl_download_async(out.ctypes.data, ptr, nbytes, stream))
            nat.check(_lib().ofl_stream_sync(stream))
            return out
    out = np.empty(shape, dtype)
    if out.nbytes:
        nat.check(_lib().ofl_download(out.ctypes.data, ptr, out.nbytes, stream))
    return out


class _BufferView:
    """An address and a length in memory that somebody else owns: part of a DeviceBuffer, or memory of another framework that a
    field has adopted.  `owner` is whatever keeps that memory alive; it travels with the view, so that every field or image
    that shares the view (relabel, scaling, an exported view) holds the owner too.  A view has no finaliser: the recycling pool
    never receives its pointer."""

    __slots__ = ("ptr", "nbytes", "owner")

    def __init__(self, ptr, nbytes, owner=None):
        self.ptr, self.nbytes, self.owner = ptr, int(nbytes), owner

    def to_host(self, shape, dtype, stream=None):
        return _download(self.ptr, shape, dtype, stream)


class PinnedArray:
    """A NumPy view of page-locked host memory (ofl_host_alloc): transfers from / to it are asynchronous DMA."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(int(v) for v in shape), np.dtype(dtype)
        self.nbytes = max(int(np.prod(self.shape)) * self.dtype.itemsize, 16)
        p = ctypes.c_void_p()
        nat.check(_lib().ofl_host_alloc(ctypes.byref(p), self.nbytes))
        self.ptr = p.value
        self._fin = weakref.finalize(self, nat.load().ofl_host_free, self.ptr)
        buf = (ctypes.c_char * self.nbytes).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=self.dtype, count=int(np.prod(self.shape))).reshape(self.shape)


def load_sintel_device(path, ref='s', stream=None):
    """Sintel .flo (utils.py:447-470) straight onto the device: the payload is read into a pinned buffer and uploaded
    asynchronously on `stream`; returns (DeviceFlow with an all-valid mask, the PinnedArray that must stay alive until
    the stream has passed the upload).  Flow.from_sintel labels such fields 's' (flow_class.py:262-275)."""
    if not isinstance(path, str):
        raise TypeError("Error loading flow from Sintel data: Path needs to be a string")
    with open(path, 'rb') as f:
        if f.read(4) != b'PIEH':
            raise ValueError("Error loading flow from Sintel data: Path not a valid .flo file")
        w = int.from_bytes(f.read(4), 'little')
        h = int.from_bytes(f.read(4), 'little')
        pin = PinnedArray((h, w, 2), '<f4')
        got = f.readinto(memoryview(pin.array).cast('B'))
        if got != h * w * 8:
            raise ValueError("Error loading flow from Sintel data: file is truncated")
    vecs, mask = DeviceBuffer(h * w * 8), DeviceBuffer(h * w)
    nat.check(_lib().ofl_upload(vecs.ptr, pin.ptr, h * w * 8, stream))
    nat.check(_lib().ofl_memset(mask.ptr, 1, h * w, stream))
    return DeviceFlow(vecs, mask, (h, w), ref), pin


def save_sintel_device(path, dflow, stream=None):
    """DeviceFlow -> .flo through a pinned buffer (asynchronous download, one synchronisation before the write)."""
    h, w = dflow.shape
    pin = PinnedArray((h, w, 2), '<f4')
    nat.check(_lib().ofl_download_async(pin.ptr, dflow.vecs.ptr, h * w * 8, stream))
    nat.check(_lib().ofl_stream_sync(stream))
    with open(path, 'wb') as f:
        f.write(b'PIEH')
        f.write(int(w).to_bytes(4, 'little'))
        f.write(int(h).to_bytes(4, 'little'))
        f.write(memoryview(pin.array).cast('B'))


_PINNED_MIN = 1 << 20        # results below 1 MiB stay pageable


class _PinnedBlock:
    __slots__ = ("ptr", "nbytes", "__weakref__")

    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, nbytes


class _PinnedPool:
    """Page-locked host blocks for downloads, recycled by size (hipHostMalloc of 66 MB takes milliseconds)."""

    def __init__(self, limit=8 << 30):
        self.free, self.in_use, self.limit = {}, 0, limit

    def _give(self, ptr, nbytes):
        try:
            self.in_use -= nbytes
            self.free.setdefault(nbytes, []).append(ptr)
        except Exception:       # interpreter shutdown
            pass

    def array(self, shape, dtype):
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        if self.in_use + nbytes > self.limit:
            return None
        lst = self.free.get(nbytes)
        if lst:
            ptr = lst.pop()
        else:
            p = ctypes.c_void_p()
            try:
                nat.check(_lib().ofl_host_alloc(ctypes.byref(p), nbytes))
            except nat.NativeError:
                return None
            ptr = p.value
        self.in_use += nbytes
        block = _PinnedBlock(ptr, nbytes)
        weakref.finalize(block, self._give, ptr, nbytes)
        buf = (ctypes.c_char * nbytes).from_address(ptr)
        buf._block = block                      # the array's base keeps the block alive
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


_pinned_pool = _PinnedPool()


def sync(stream=None):
    nat.check(_lib().ofl_stream_sync(stream))


class DeviceImage:
    """A warp target in HBM: [H][W][C] of uint8 / int16 / uint16 / float32 / float64."""

    def __init__(self, buf, shape, dtype):
        self.buf, self.shape, self.dtype = buf, tuple(shape), np.dtype(dtype)

    @classmethod
    def from_host(cls, arr):
        arr = np.ascontiguousarray(arr)
        if arr.ndim == 2:
            arr = arr[..., None]
        if arr.dtype not in _DT_CODE:
            raise TypeError("warp targets must be uint8, int16, uint16, float32 or float64 "
                            "(what cv2.remap accepts), got {}".format(arr.dtype))
        return cls(DeviceBuffer.from_host(arr), arr.shape, arr.dtype)

    def to_host(self):
        return self.buf.to_host(self.shape, self.dtype)

    @classmethod
    def from_external(cls, img, layout=None, stream=None, copy=True):
        """An image another framework holds in device memory (`img.__cuda_array_interface__`, see external_args): (H, W, C),
        (H, W) or, with layout='chw', (C, H, W), of uint8 / int16 / uint16 / float32 / float64.  A contiguous 'hwc' image is
        one device copy -- or, with copy=False, adopted: the DeviceImage then IS the producer's memory, its buffer view keeps `img` alive and
        must not be written by the producer afterwards.  Any other layout or stride goes through the permute kernel (C up to
        6; copy=False is a ValueError).  The library's stream first waits for the producer's (`stream`: see external_args).
        Asynchronous: until the library's stream has passed the copy (sync()), the producer must leave the source alone."""
        ext = external_args(img, None, stream)
        shape, st, contiguous = image_layout(ext, layout)
        if not copy and not contiguous:
            raise ValueError("Error taking an external image: copy=False needs a C-contiguous (H, W, C) or (H, W) array")
        _check_device_memory(ext)
        _wait_for(ext.stream)
        h, w, c = shape
        if contiguous and not copy:
            return cls(_BufferView(ext.ptr, h * w * c * ext.itemsize, owner=img), shape, ext.dtype)
        buf = DeviceBuffer(h * w * c * ext.itemsize)
        if contiguous:
            nat.check(_lib().ofl_copy_dev(buf.ptr, ext.ptr, h * w * c * ext.itemsize, None))
        else:
            nat.check(_lib().ofl_permute_image_dev(ext.ptr, buf.ptr, ext.itemsize, c, h, w, st[2], st[0], st[1], 1, None))
        return cls(buf, shape, ext.dtype)

    def export(self, layout='hwc', copy=True):
        """-> DeviceArray (`__cuda_array_interface__`; torch.as_tensor(a, device='cuda')): 'hwc' the image as it is -- a device
        copy or, with copy=False, a view of this image's own memory that the consumer must not write --, 'chw' (C, H, W)
        through the permute kernel."""
        if layout not in ('hwc', 'chw'):
            raise ValueError("Error exporting image: layout must be 'hwc' or 'chw', got {!r}".format(layout))
        nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        if layout == 'hwc':
            if not copy:
                return DeviceArray(self.buf, self.shape, self.dtype.str, owner=self)
            buf = DeviceBuffer(nbytes)
            nat.check(_lib().ofl_copy_dev(buf.ptr, self.buf.ptr, nbytes, None))
            return DeviceArray(buf, self.shape, self.dtype.str)
        if not copy:
            raise ValueError("Error exporting image: copy=False hands out the image's own (H, W, C) memory; 'chw' is a conversion")
        if len(self.shape) != 3 or not 1 <= self.shape[2] <= 6:
            raise ValueError("Error exporting image: 'chw' takes one (H, W, C) image with C in 1..6, got shape {}".format(self.shape))
        h, w, c = self.shape
        buf = DeviceBuffer(nbytes)
        nat.check(_lib().ofl_permute_image_dev(self.buf.ptr, buf.ptr, self.dtype.itemsize, c, h, w, h * w, w, 1, 0, None))
        return DeviceArray(buf, (c, h, w), self.dtype.str)


_TRACK_DT = {np.dtype('float64'): nat.TRACK_F64, np.dtype('int32'): nat.TRACK_I32, np.dtype('int64'): nat.TRACK_I64}


def _points_array(arr):
    """A host array of points, checked like track_pts (utils.py:571-574, :592) -> contiguous (n, 2) float64, int32 or int64.
    Other float dtypes become float64; any other dtype -- the narrow integers, which NumPy would add to the float32 vectors
    in float32, included -- is a TypeError (the reference raises it for ref 's' only)."""
    if not isinstance(arr, np.ndarray):
        raise TypeError("Error tracking points: Pts needs to be a numpy array")
    if arr.ndim != 2 or arr.shape[1] != 2:
        raise ValueError("Error tracking points: Pts needs to have shape N-2")
    if np.issubdtype(arr.dtype, np.floating):
        return np.ascontiguousarray(arr, np.float64)
    if arr.dtype in _TRACK_DT:
        return np.ascontiguousarray(arr)
    raise TypeError("Error tracking points: Pts numpy array needs to have a float or int (int32, int64) dtype")


class DevicePoints:
    """(n, 2) points in (row, col) order in HBM: float64, int32 or int64.  What DeviceFlow.track and DeviceFlowBatch.track* take
    and hand back, so that points tracked through a sequence of fields never leave the device."""

    def __init__(self, buf, n, dtype, shape=None):
        self.buf, self.n, self.dtype = buf, int(n), np.dtype(dtype)
        self.shape = (self.n, 2) if shape is None else tuple(shape)      # the batch calls stack results: (fields, n, 2)

    @classmethod
    def from_host(cls, arr):
        arr = _points_array(arr)
        return cls(DeviceBuffer.from_host(arr), arr.shape[0], arr.dtype)

    def to_host(self):
        return self.buf.to_host(self.shape, self.dtype)

    @classmethod
    def from_external(cls, pts, stream=None):
        """Points another framework holds in device memory (`pts.__cuda_array_interface__`): C-contiguous (n, 2) float64,
        int32 or int64 in (row, col) order -> one device copy, after the library's stream has been made to wait for the
        producer's (`stream`: see external_args).  Asynchronous, like DeviceImage.from_external."""
        ext = external_args(pts, None, stream)
        if ext.dtype not in _TRACK_DT:
            raise TypeError("Error tracking points: Pts needs to have a float64 or int (int32, int64) dtype, got {}".format(ext.dtype))
        if len(ext.shape) != 2 or ext.shape[1] != 2:
            raise ValueError("Error tracking points: Pts needs to have shape N-2")
        if not _contiguous(ext.shape, ext.strides):
            raise ValueError("Error tracking points: external points need to be C-contiguous")
        _check_device_memory(ext)
        _wait_for(ext.stream)
        n = ext.shape[0]
        buf = DeviceBuffer(n * 2 * ext.itemsize)
        nat.check(_lib().ofl_copy_dev(buf.ptr, ext.ptr, n * 2 * ext.itemsize, None))
        return cls(buf, n, ext.dtype)

    def export(self, copy=True):
        """-> DeviceArray of this object's shape ((n, 2), or (fields, n, 2) from the batch calls): a device copy or, with
        copy=False, a view of the points' own memory that the consumer must not write."""
        if not copy:
            return DeviceArray(self.buf, self.shape, self.dtype.str, owner=self)
        nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        buf = DeviceBuffer(nbytes)
        nat.check(_lib().ofl_copy_dev(buf.ptr, self.buf.ptr, nbytes, None))
        return DeviceArray(buf, self.shape, self.dtype.str)


# ------------------------------------------------------------------------------ kernels
def gather_bilinear(src, flow_buf, flow_shape, sign, smask=None, fmask=None, want_valid=False,
                    pad=(0, 0), quant=nat.QUANT_OPENCV, arith=nat.ARITH_NATIVE, rule=nat.RULE_EQ1,
                    stream=None):
    """K1: dst = B(src; x + sign*flow) (+ validity).  Replaces apply_flow 't', utils.py:231-236."""
    H, W, C = src.shape
    dst = DeviceImage(DeviceBuffer(H * W * C * src.dtype.itemsize), src.shape, src.dtype)
    valid = DeviceBuffer(H * W) if want_valid else None
    nat.check(_lib().ofl_gather_bilinear_dev(
        src.buf.ptr, _DT_CODE[src.dtype], C, H, W, flow_buf.ptr, flow_shape[0], flow_shape[1],
        pad[0], pad[1], sign, smask.ptr if smask is not None else None,
        fmask.ptr if fmask is not None else None, dst.buf.ptr,
        valid.ptr if valid is not None else None, quant, arith, rule, stream))
    return dst, valid


def gather_bilinear_batch(src, dtype, C, H, W, batch, flow, sign, smask=None, fmask=None, dst=None, valid=None,
                          shared_src=False, shared_smask=False, flow_shape=None, pad=(0, 0),
                          quant=nat.QUANT_OPENCV, arith=nat.ARITH_NATIVE, rule=nat.RULE_EQ1, stream=None):
    """K1 over `batch` fields in ONE launch (ofl_gather_bilinear_batch_dev): buffers hold the fields back to back -- flow
    [B][fH][fW][2], fmask [B][fH][fW], src [B][H][W][C] (or one [H][W][C] image for all with shared_src), smask likewise,
    dst [B][H][W][C], valid [B][H][W].  dst / valid are allocated when not given (valid only if `valid is True`).
    Returns (dst buffer, valid buffer or None)."""
    dtype = np.dtype(dtype)
    fH, fW = flow_shape if flow_shape is not None else (H, W)
    if dst is None:
        dst = DeviceBuffer(batch * H * W * C * dtype.itemsize)
    if valid is True:
        valid = DeviceBuffer(batch * H * W)
    nat.check(_lib().ofl_gather_bilinear_batch_dev(
        src.ptr if src is not None else None, 1 if shared_src else 0, _DT_CODE[dtype], C, H, W, batch, flow.ptr, fH, fW,
        pad[0], pad[1], sign, smask.ptr if smask is not None else None, 1 if shared_smask else 0,
        fmask.ptr if fmask is not None else None, dst.ptr if C else None, valid.ptr if valid is not None else None,
        quant, arith, rule, stream))
    return dst, valid


def gather_rows(src, row0, rows, flow_rows, sign, smask=None, fmask_rows=None, want_valid=False,
                quant=nat.QUANT_OPENCV, arith=nat.ARITH_NATIVE, rule=nat.RULE_EQ1, stream=None):
    """K1 on one row band of a field split over several GPUs: `src` is the replicated
    H x W image, `flow_rows` / `fmask_rows` hold rows [row0, row0 + rows) only; returns the same rows of the
    warped image (and of the valid area)."""
    H, W, C = src.shape
    dst = DeviceImage(DeviceBuffer(rows * W * C * src.dtype.itemsize), (rows, W, C), src.dtype)
    valid = DeviceBuffer(rows * W) if want_valid else None
    nat.check(_lib().ofl_gather_rows_dev(
        src.buf.ptr, _DT_CODE[src.dtype], C, H, W, row0, rows, flow_rows.ptr, sign,
        smask.ptr if smask is not None else None, fmask_rows.ptr if fmask_rows is not None else None,
        dst.buf.ptr, valid.ptr if valid is not None else None, quant, arith, rule, stream))
    return dst, valid


def gather_valid_only(H, W, flow_buf, flow_shape, sign, smask=None, fmask=None, pad=(0, 0),
                      quant=nat.QUANT_OPENCV, rule=nat.RULE_EQ1, stream=None):
    """K1 without image channels: where does a warped all-ones (or smask) image stay == 1?
    (valid_target 't' flow_class.py:1148-1150, valid_source 's' :1179-1183)."""
    valid = DeviceBuffer(H * W)
    nat.check(_lib().ofl_gather_bilinear_dev(
        None, nat.U8, 0, H, W, flow_buf.ptr, flow_shape[0], flow_shape[1], pad[0], pad[1], sign,
        smask.ptr if smask is not None else None, fmask.ptr if fmask is not None else None,
        None, valid.ptr, quant, nat.ARITH_NATIVE, rule, stream))
    return valid


def flow_stats(vecs_buf, mask_buf, n_px, stream=None):
    """K4: OFL_STAT_* bits of one field (utils.py:527-544, flow_class.py:1230-1245)."""
    out = DeviceBuffer(16)
    nat.check(_lib().ofl_flow_stats_dev(vecs_buf.ptr, mask_buf.ptr if mask_buf is not None else None,
                                        n_px, np.float32(DEFAULT_THRESHOLD), out.ptr, stream))
    return int(out.to_host((1,), np.uint32, stream)[0])


def compose3_launch(fa, fb, sign, out, stats_buf=None, stats_offset=0, batch=1, quant=nat.QUANT_OPENCV,
                    stream=None):
    """K2 launch on raw DeviceFlow-like triples; asynchronous.  stats_buf: uint32[batch][8] words."""
    H, W = fa.shape
    sp = None if stats_buf is None else stats_buf.ptr + stats_offset
    nat.check(_lib().ofl_compose3_dev(fa.vecs.ptr, fa.mask.ptr, fb.vecs.ptr, fb.mask.ptr, sign, H, W, batch,
                                      out.vecs.ptr, out.mask.ptr, sp, quant, stream))


def mask_bits_bytes(h, w, batch=1):
    n = ctypes.c_size_t(0)
    nat.check(_lib().ofl_mask_bits_bytes(h, w, batch, ctypes.byref(n)))
    return n.value


def mask_pack(mask_buf, h, w, batch=1, stream=None):
    """uint8 masks [batch][H][W] -> packed bit planes [batch][H][(W + 31) / 32] uint32 (ofl_mask_pack_dev)"""
    bits = DeviceBuffer(mask_bits_bytes(h, w, batch))
    nat.check(_lib().ofl_mask_pack_dev(mask_buf.ptr, h, w, batch, bits.ptr, stream))
    return bits


def mask_unpack(bits_buf, h, w, batch=1, stream=None):
    mask = DeviceBuffer(batch * h * w)
    nat.check(_lib().ofl_mask_unpack_dev(bits_buf.ptr, h, w, batch, mask.ptr, stream))
    return mask


def compose3_bits_launch(fa_vecs, fa_bits, fb_vecs, fb_bits, sign, shape, out_vecs, out_bits, stats_buf=None, stats_offset=0, batch=1, stream=None):
    """K2 on packed mask planes (ofl_compose3_bits_dev); asynchronous."""
    sp = None if stats_buf is None else stats_buf.ptr + stats_offset
    nat.check(_lib().ofl_compose3_bits_dev(fa_vecs.ptr, fa_bits.ptr, fb_vecs.ptr, fb_bits.ptr, sign, shape[0], shape[1], batch,
                                           out_vecs.ptr, out_bits.ptr, sp, stream))


_VIS_MODES = {'hsv': nat.VIS_HSV, 'rgb': nat.VIS_RGB, 'bgr': nat.VIS_BGR}


def visualise_args(mode, show_mask=False, show_mask_borders=False, range_max=None):
    """Validation of Flow.visualise's arguments (flow_class.py:887-892, 917-920, 948-951), on the host before any device
    work: -> (mode code, OFL_VIS_* flags, float32 range or None for the per-field default).  `range_max` must be a
    Python float or int (bool included, NumPy's float32 not), > 0 and -- beyond the reference -- finite."""
    if not isinstance(show_mask, bool):
        raise TypeError("Error visualising flow: show_mask must be a bool, got {}".format(type(show_mask).__name__))
    if not isinstance(show_mask_borders, bool):
        raise TypeError("Error visualising flow: show_mask_borders must be a bool, got {}".format(type(show_mask_borders).__name__))
    rc = None
    if range_max is not None:
        if not isinstance(range_max, (float, int)):
            raise TypeError("Error visualising flow: range_max must be a float or an int, got {}".format(type(range_max).__name__))
        if range_max <= 0:
            raise ValueError("Error visualising flow: range_max must be positive, got {}".format(range_max))
        if isinstance(range_max, float) and not np.isfinite(range_max):
            raise ValueError("Error visualising flow: range_max must be finite, got {}".format(range_max))
        with np.errstate(over='ignore'):        # a finite value beyond float32 divides like NumPy's float32 inf
            rc = np.float32(float(range_max)) if abs(range_max) < 1e300 else np.float32(np.inf)
    if not isinstance(mode, str) or mode not in _VIS_MODES:
        raise ValueError("Error visualising flow: mode must be 'rgb', 'bgr' or 'hsv', got {!r}".format(mode))
    flags = (nat.VIS_SHOW_MASK if show_mask else 0) | (nat.VIS_MASK_BORDERS if show_mask_borders else 0)
    return _VIS_MODES[mode], flags, rc


def track_args(pts, int_out=None, get_valid_status=None, s_exact_mode=None):
    """Validation of Flow.track's arguments (flow_class.py:781-784, utils.py:571-582) with the reference's defaults and
    exception types, on the host before any device work -> (int_out, get_valid_status, s_exact_mode).  `pts`: a
    DevicePoints or an (n, 2) array of a dtype DevicePoints.from_host takes."""
    if not isinstance(pts, DevicePoints):
        _points_array(pts)
    int_out = False if int_out is None else int_out
    get_valid_status = False if get_valid_status is None else get_valid_status
    s_exact_mode = False if s_exact_mode is None else s_exact_mode
    if not isinstance(int_out, bool):
        raise TypeError("Error tracking points: Int_out needs to be a boolean")
    if not isinstance(get_valid_status, bool):
        raise TypeError("Error tracking points: Get_tracked needs to be a boolean")
    if not isinstance(s_exact_mode, bool):
        raise TypeError("Error tracking points: S_exact_mode needs to be a boolean")
    return int_out, get_valid_status, s_exact_mode


def percentile_ranks(n, q=99):
    """(lo, hi, gamma) of np.percentile(a, q) over n float32 values (NumPy 2.x, method 'linear'): the result is
    _lerp(sorted[lo], sorted[hi], gamma).  NumPy works in the array's dtype: q / float32(100), the virtual index
    (n - 1) * q and gamma are float32 (numpy/lib/_function_base_impl.py, percentile / _quantile / _get_indexes)."""
    qq = np.asanyarray(np.true_divide(q, np.float32(100)))
    vi = np.asanyarray((n - 1) * qq)
    prev = np.asanyarray(np.floor(vi))
    if vi >= n - 1:                                      # NumPy then takes the last element twice
        prev = np.asanyarray(-1.0)
    prev = prev.astype(np.intp)
    gamma = np.asanyarray(vi - prev, dtype=vi.dtype)
    lo = n - 1 if prev < 0 else int(prev)
    return lo, min(lo + 1, n - 1) if prev >= 0 else lo, np.float32(gamma)


def visualise_range_launch(vecs, h, w, batch, out, stream=None):
    """K7 range select: out (float32[batch] on the device) <- the default range_max of every field, flow_class.py:910-916.
    Asynchronous."""
    lo, hi, gamma = percentile_ranks(h * w)
    nb = ctypes.c_size_t(0)
    nat.check(_lib().ofl_visualise_workspace_bytes(h, w, batch, ctypes.byref(nb)))
    ws = DeviceBuffer(nb.value)
    nat.check(_lib().ofl_visualise_range_dev(vecs.ptr, h, w, batch, np.float32(DEFAULT_THRESHOLD), lo, hi, gamma,
                                             ws.ptr, ws.nbytes, out.ptr, stream))


def visualise_launch(vecs, mask, h, w, batch, mode, flags, range_buf=None, range_const=None, stream=None):
    """K7 render of `batch` fields -> DeviceImage uint8 (batch, H, W, 3), or (H, W, 3) for batch 1.  The scale comes from
    range_buf (float32[batch] on the device) or, if that is None, from range_const.  Asynchronous."""
    shape = (h, w, 3) if batch == 1 else (batch, h, w, 3)
    img = DeviceImage(DeviceBuffer(batch * h * w * 3), shape, np.uint8)
    nat.check(_lib().ofl_visualise_dev(vecs.ptr, mask.ptr if mask is not None and flags else None, h, w, batch,
                                       np.float32(DEFAULT_THRESHOLD), range_buf.ptr if range_buf is not None else None,
                                       np.float32(1.0 if range_const is None else range_const), mode, flags, img.buf.ptr, stream))
    return img


class FitField:
    """The K8 passes over one HBM-resident field (csrc/ofl_fit.hip), as the object matrix_fit.fit drives: each method
    enqueues one entry of include/ofl.h and reads its few numbers back.  mask: DeviceBuffer or None (every pixel counts);
    gate: None or (3x3 model, float32 squared threshold)."""

    def __init__(self, vecs, mask, shape, sign, stream=None):
        self.vecs, self.mask, self.sign, self.stream = vecs, mask, sign, stream
        self.h, self.w = int(shape[0]), int(shape[1])
        self.origin = ((self.w - 1) / 2.0, (self.h - 1) / 2.0)            # the grid centre
        nb = ctypes.c_size_t(0)
        nat.check(_lib().ofl_fit_workspace_bytes(self.h, self.w, ctypes.byref(nb)))
        self.ws = DeviceBuffer(nb.value)
        self.out = DeviceBuffer(1024)

    def _field(self):
        return (self.vecs.ptr, self.mask.ptr if self.mask is not None else None, self.h, self.w)

    @staticmethod
    def _doubles(values):
        a = np.ascontiguousarray(values, np.float64)
        return a, a.ctypes.data

    def _gate(self, gate):
        if gate is None:
            return None, None, np.float32(0)
        keep, ptr = self._doubles(gate[0])
        return keep, ptr, np.float32(gate[1])

    def _sums(self, entry, count, gate, *params):
        keep, gptr, thr = self._gate(gate)
        held = [self._doubles(p) for p in params]
        nat.check(entry(*self._field(), self.sign, *[p for _, p in held], gptr, thr, self.ws.ptr, self.ws.nbytes,
                        self.out.ptr, self.stream))
        return self.out.to_host((count,), np.float64, self.stream)

    def moments(self, gate=None):
        return self._sums(_lib().ofl_fit_moments_dev, 16, gate, self.origin)

    def dlt(self, norm, gate=None):
        return self._sums(_lib().ofl_fit_dlt_dev, 47, gate, norm)

    def gn(self, norm, model, gate=None):
        return self._sums(_lib().ofl_fit_gn_dev, 47, gate, norm, model)

    def score(self, models, thr):
        m, ptr = self._doubles(models)
        k = m.size // 9
        nat.check(_lib().ofl_fit_score_dev(*self._field(), self.sign, ptr, k, np.float32(thr), self.out.ptr, self.stream))
        return self.out.to_host((k,), np.uint32, self.stream)

    def median(self, models, rank_lo, rank_hi):
        m, ptr = self._doubles(models)
        k = m.size // 9
        out = self.out if k * 8 <= self.out.nbytes else DeviceBuffer(k * 8)
        nat.check(_lib().ofl_fit_median_dev(*self._field(), self.sign, ptr, k, rank_lo, rank_hi, self.ws.ptr, self.ws.nbytes,
                                            out.ptr, self.stream))
        return out.to_host((k, 2), np.uint32, self.stream)

    def index(self):
        nat.check(_lib().ofl_fit_index_dev(*self._field(), self.ws.ptr, self.ws.nbytes, self.stream))

    def pick(self, ranks):
        """pixel indices and gathered records (count, 4) uint32 of the ranks-th valid pixels (after index())"""
        ranks = np.ascontiguousarray(ranks, np.uint32)
        n = ranks.size
        rbuf = DeviceBuffer.from_host(ranks, self.stream)
        idx, rec = DeviceBuffer(n * 4), DeviceBuffer(n * 16)
        nat.check(_lib().ofl_fit_pick_dev(*self._field(), self.ws.ptr, self.ws.nbytes, rbuf.ptr, n, idx.ptr, self.stream))
        nat.check(_lib().ofl_fit_gather_dev(*self._field(), idx.ptr, n, rec.ptr, self.stream))
        return rec.to_host((n, 4), np.uint32, self.stream)

    def sample(self, ranks):
        """-> (src, dst): (count, 2) float64 correspondences of the ranks-th valid pixels"""
        rec = self.pick(ranks)
        idx = rec[:, 0].astype(np.int64)
        grid = np.stack([idx % self.w, idx // self.w], axis=-1).astype(np.float64)
        v = np.ascontiguousarray(rec[:, 1:3]).view(np.float32).astype(np.float64)
        return (grid, grid + v) if self.sign > 0 else (grid - v, grid)


_STATS_KNOW_MASK = 1 << 30        # private flag in DeviceFlow._stats: STAT_MASK_HAS_ZERO has been evaluated


# ------------------------------------------------------------------------------ K9: build / scale / pad / crop
# Host halves of the DeviceFlow constructors and operators: argument checks with the reference's exception types, raised
# before the device is touched.
_PAD_MODES = {'constant': 0, 'edge': 1, 'symmetric': 2}
_N_TRANSFORM_VALUES = {'translation': 2, 'rotation': 3, 'scaling': 3}


def matrix_args(matrix, shape, ref):
    """Validation of utils.from_matrix (utils.py:328-334) -> (the float64 matrix the kernel evaluates, sign, ref): the
    matrix itself and +1 for 's', its pseudo-inverse and -1 for 't' (utils.py:335-344)."""
    from .utils import validate_shape, get_valid_ref
    validate_shape(shape)
    if not isinstance(matrix, np.ndarray):
        raise TypeError("Error creating flow from matrix: Matrix needs to be a numpy array")
    if matrix.shape != (3, 3):
        raise ValueError("Error creating flow from matrix: Matrix needs to be a numpy array of shape (3, 3)")
    ref = get_valid_ref(ref)
    m = matrix if ref == 's' else np.linalg.pinv(matrix)
    return np.ascontiguousarray(m, np.float64), (1 if ref == 's' else -1), ref


def validate_transforms(transform_list, shape):
    """Validation of utils.from_transforms (utils.py:381-420)."""
    from .utils import validate_shape
    validate_shape(shape)
    if not isinstance(transform_list, list):
        raise TypeError("Error creating flow from transforms: Transform_list needs to be a list")
    if not all(isinstance(t, list) for t in transform_list):
        raise TypeError("Error creating flow from transforms: Transform_list needs to be a list of lists")
    if not all(len(t) > 1 for t in transform_list):
        raise ValueError("Error creating flow from transforms: Invalid transforms passed")
    for t in transform_list:
        if t[0] not in _N_TRANSFORM_VALUES:
            raise ValueError("Error creating flow from transforms: Transform '{}' not recognised".format(t[0]))
        if len(t) - 1 != _N_TRANSFORM_VALUES[t[0]]:
            raise ValueError("Error creating flow from transforms: Not enough transform values passed for "
                             "'{}' - expected {}, got {}".format(t[0], _N_TRANSFORM_VALUES[t[0]], len(t) - 1))
        if not all(isinstance(v, (float, int)) for v in t[1:]):
            raise ValueError("Error creating flow from transforms: "
                             "Transform values for '{}' need to be integers or floats".format(t[0]))


def _valid_mask(mask, shape):
    """A constructor's `mask` argument: None, a DeviceBuffer of at least H * W bytes (0 / 1, taken as it is), or a host array
    checked like the Flow.mask setter (flow_class.py:142-161) -> None, the buffer, or uint8 (H, W)."""
    if mask is None:
        return None
    n = int(shape[0]) * int(shape[1])
    if isinstance(mask, (DeviceBuffer, _BufferView)):
        if mask.nbytes < n:
            raise ValueError("Error setting flow mask: Input has a different shape than the flow vectors")
        return mask
    if not isinstance(mask, np.ndarray):
        raise TypeError("Error setting flow mask: Input is not a numpy array")
    if mask.ndim != 2:
        raise ValueError("Error setting flow mask: Input not 2-dimensional")
    if mask.shape != (shape[0], shape[1]):
        raise ValueError("Error setting flow mask: Input has a different shape than the flow vectors")
    if ((mask != 0) & (mask != 1)).any():
        raise ValueError("Error setting flow mask: Values must be 0 or 1")
    return np.ascontiguousarray(mask.astype(np.bool_)).view(np.uint8)


def _mask_buffer(mask, shape):
    if mask is None:
        buf = DeviceBuffer(int(shape[0]) * int(shape[1]))
        nat.check(_lib().ofl_memset(buf.ptr, 1, int(shape[0]) * int(shape[1]), None))
        return buf
    return DeviceBuffer.from_host(mask) if isinstance(mask, np.ndarray) else mask


def flow_from_matrix_launch(mats, n, sign, shape, out, stream=None):
    """K9 constructor: `n` fields [n][H][W][2] into `out` from `mats`, n x 9 float64 on the device.  Asynchronous."""
    nat.check(_lib().ofl_flow_from_matrix_dev(mats.ptr, n, sign, shape[0], shape[1], out.ptr, stream))


def scale_operand(other, shape, verb, noun):
    """The operand of DeviceFlow * and /, checked like Flow._broadcast_operand (flow_class.py:377-443) -> (k0, k1, wide):
    the factors of the two channels and whether NumPy would compute in float64 (np.result_type of float32 and the operand:
    a float64 or integer list / array) or in float32 (a number, which NumPy treats as a weak scalar, or a float32 array)."""
    try:
        k = float(other)
        return k, k, 0
    except TypeError:
        pass
    if isinstance(other, list):
        if len(other) != 2:
            raise ValueError("Error {} flow: {} list not length 2".format(verb, noun))
        arr = np.array(other)
    elif isinstance(other, np.ndarray):
        if other.ndim == 1 and other.size == 2:
            arr = other
        elif (other.ndim == 2 and other.shape == tuple(shape)) or other.shape == tuple(shape) + (2,):
            raise TypeError("Error {} flow: {} arrays of the shape of the flow are not supported on the device; "
                            "use the host Flow (Flow.from_device)".format(verb, noun))
        else:
            raise ValueError("Error {} flow: {} array is not one of the following: size 2, shape of the "
                             "flow object, shape of the flow vectors".format(verb, noun))
    else:
        raise TypeError("Error {} flow: {} cannot be converted to float, or isn't a list or numpy array"
                        .format(verb, noun))
    try:
        res = np.result_type(np.float32, arr.dtype)
    except TypeError:
        res = None
    if res not in (np.float32, np.float64):
        raise TypeError("Error {} flow: {} of dtype {} does not combine with float32 vectors to float32 or float64"
                        .format(verb, noun, arr.dtype))
    return float(arr[0]), float(arr[1]), int(res == np.float64)


def crop_args(item, shape):
    """The index of DeviceFlow[...] -> ((row0, row_step, rows), (col0, col_step, cols)), normalised with slice.indices."""
    if isinstance(item, slice):
        item = (item,)
    if not isinstance(item, tuple) or not 1 <= len(item) <= 2 or not all(isinstance(s, slice) for s in item):
        raise TypeError("Error slicing flow: DeviceFlow takes a slice or a tuple of one or two slices (rows, columns); "
                        "for any other index use the host Flow (Flow.from_device)")
    out = []
    for s, n in zip(item + (slice(None),) * (2 - len(item)), shape):
        start, stop, step = s.indices(n)
        count = len(range(start, stop, step))
        if count == 0:
            raise ValueError("Error slicing flow: the slices select no pixels of the {}x{} field".format(*shape))
        out.append((start, step, count))
    return tuple(out)


# ------------------------------------------------------------------------------ DeviceFlow
class DeviceFlow:
    """(vecs, mask, ref) resident in HBM.  Buffers are immutable once wrapped."""

    def __init__(self, vecs, mask, shape, ref, stats=None):
        self.vecs, self.mask = vecs, mask
        self.shape = (int(shape[0]), int(shape[1]))
        self.ref = ref
        self._stats = stats
        self._stats_buf = None      # the OFL_STAT_* word in HBM, for kernels that read the zero-flow predicate themselves
        self._certs = {}            # (sign, point_precision) -> MeshCert of the warped grid without a point mask

    # -- construction / transfer
    @classmethod
    def empty(cls, shape, ref):
        n = int(shape[0]) * int(shape[1])
        return cls(DeviceBuffer(n * 8), DeviceBuffer(n), shape, ref)

    @classmethod
    def from_host(cls, vecs, ref='t', mask=None):
        vecs = np.ascontiguousarray(vecs, dtype=np.float32)
        h, w = vecs.shape[:2]
        if mask is None:
            m = np.ones((h, w), np.uint8)
        else:
            m = np.ascontiguousarray(mask)
            m = m.view(np.uint8) if m.dtype == np.bool_ else m.astype(np.uint8)
        return cls(DeviceBuffer.from_host(vecs), DeviceBuffer.from_host(m), (h, w), ref)

    @classmethod
    def zero(cls, shape, ref=None, mask=None):
        """Flow.zero (flow_class.py:173-186) in HBM: a memset."""
        from .utils import validate_shape, get_valid_ref
        validate_shape(shape)
        ref, mask = get_valid_ref(ref), _valid_mask(mask, shape)
        return cls(DeviceBuffer.zeros(shape[0] * shape[1] * 8), _mask_buffer(mask, shape), shape, ref)

    @classmethod
    def from_matrix(cls, matrix, shape, ref=None, mask=None):
        """Flow.from_matrix (flow_class.py:188-207, utils.py:319-344) built in HBM: 72 bytes go up, one launch of the
        constructor kernel writes the field -- bit for bit what utils.from_matrix computes on the host.  `mask`: a host array
        (validated like Flow.mask), a uint8 DeviceBuffer [H][W], or None (all valid).  Arguments are validated before the
        device is touched."""
        m, sign, ref = matrix_args(matrix, shape, ref)
        mask = _valid_mask(mask, shape)
        vecs = DeviceBuffer(shape[0] * shape[1] * 8)
        flow_from_matrix_launch(DeviceBuffer.from_host(m), 1, sign, shape, vecs)
        return cls(vecs, _mask_buffer(mask, shape), shape, ref)

    @classmethod
    def from_transforms(cls, transform_list, shape, ref=None, mask=None):
        """Flow.from_transforms (flow_class.py:209-234, utils.py:347-423) built in HBM, see from_matrix."""
        from .utils import matrix_from_transforms
        validate_transforms(transform_list, shape)
        return cls.from_matrix(matrix_from_transforms(transform_list), shape, ref, mask)

    @classmethod
    def from_external(cls, vecs, ref='t', mask=None, layout=None, dtype=None, stream=None, copy=True, check_finite=True):
        """A field another framework holds in device memory, taken without crossing PCIe: `vecs.__cuda_array_interface__`
        (see external_args) describes (H, W, 2) ('hwc') or (2, H, W) ('chw') of float16 / float32 / float64 -- or bfloat16,
        handed over as a 2-byte integer array with dtype='bfloat16' -- with any non-negative strides (views, broadcasts).
        `layout` None infers the layout when exactly one of the first and last dimensions is 2.  `mask`: another such object
        (H, W) of bool or uint8, anything the other constructors take (a host array, a DeviceBuffer), or None (all valid).

        Every foreign pointer is first checked to be memory of this engine's device (ValueError otherwise), the library's
        stream is made to wait for the producer's (`stream`: an integer handle, else the interface's entry, else the legacy
        default stream), then ONE launch converts vectors and mask.  With check_finite (the default) 8 bytes come back, which
        synchronises, and the reference's errors are raised: ValueError "contains NaN or Inf" (counted on the float32 values:
        a float64 beyond the float32 range counts too) and "Values must be 0 or 1".  check_finite=False stays ASYNCHRONOUS:
        nothing is checked, and the producer must leave the source alone until the library's stream has passed the import
        (sync()).

        copy=False ADOPTS the producer's memory instead: only for C-contiguous 'hwc' float32 at a 16-byte aligned address,
        with a C-contiguous 1-byte external mask, a mask of the library's, or none (anything else is a ValueError).  The
        field's buffer views keep the producer's objects alive -- and so does every field that shares them (relabel, * k) --,
        they never enter the library's pool, and -- fields are immutable --
        the producer must NOT write to that memory afterwards.  The check, if asked for, reads the memory without copying."""
        from .utils import get_valid_ref
        ref = get_valid_ref(ref)
        v, m, n, shape = import_flow(vecs, mask, layout, dtype, stream, copy, check_finite, batch=False)
        return cls(v, m, shape, ref)

    def export(self, layout='hwc', dtype='float32', copy=True):
        """The vectors as a DeviceArray (`__cuda_array_interface__`; torch.as_tensor(a, device='cuda')): (H, W, 2) for 'hwc',
        (2, H, W) for 'chw', of float32, float16 or bfloat16 (to nearest even, overflow to +-inf).  bfloat16 goes out as
        int16 ('<i2'), for which the interface has no type: the consumer reinterprets it (t.view(torch.bfloat16)).
        copy=False is accepted only for 'hwc' float32, where nothing is converted: it hands out a view of the field's own
        memory, which the consumer must NOT write (fields are immutable)."""
        return export_flow(self.vecs, 1, self.shape, layout, dtype, copy, self)

    def export_mask(self, copy=True):
        """The mask as a DeviceArray of bool ('|b1'), (H, W); copy=False: a view of the field's own mask, not to be written."""
        return export_mask(self.mask, (self.shape[0], self.shape[1]), copy, self)

    def copy(self):
        """Flow.copy (flow_class.py:277-284): fresh buffers with the same content."""
        out = DeviceFlow.empty(self.shape, self.ref)
        nat.check(_lib().ofl_copy_dev(out.vecs.ptr, self.vecs.ptr, self.n_px * 8, None))
        nat.check(_lib().ofl_copy_dev(out.mask.ptr, self.mask.ptr, self.n_px, None))
        out._stats, out._certs = self._stats, dict(self._certs)
        return out

    def to_host(self):
        """-> (vecs float32 [H,W,2], mask bool [H,W])"""
        h, w = self.shape
        return self.vecs.to_host((h, w, 2), np.float32), self.mask.to_host((h, w), np.uint8).view(np.bool_)    # bytes are 0 / 1

    def relabel(self, ref):
        out = DeviceFlow(self.vecs, self.mask, self.shape, ref, self._stats)
        out._stats_buf = self._stats_buf
        out._certs = self._certs        # same vectors: same warped grid
        return out

    def mesh_cert(self, sign, point_precision=0):
        """Certificate of the grid warped by sign * vecs with every point kept (ofl_scatter_certify_dev): evaluated
        once per field and sign, then the certified scatter entry runs without any synchronisation."""
        key = (sign, point_precision)
        c = self._certs.get(key)
        if c is None:
            h, w = self.shape
            c = nat.MeshCert()
            ws = _workspace(h, w, 0)
            nb = ctypes.c_size_t(0)
            nat.check(_lib().ofl_scatter_diag_bytes(h, w, ctypes.byref(nb)))
            bits = DeviceBuffer(nb.value)          # the cells' Delaunay diagonals, read by the walk kernel; lives with the certificate
            nat.check(_lib().ofl_scatter_certify_dev(self.vecs.ptr, sign, point_precision, None, h, w, ws.ptr, ws.nbytes,
                                                     ctypes.byref(c), bits.ptr, None))
            if c.certified:
                c._diag_buf = bits
            else:
                c.diag_bits = None
            self._certs[key] = c
        return c

    @property
    def n_px(self):
        return self.shape[0] * self.shape[1]

    # -- predicates
    def stats(self):
        if self._stats is None:
            self._stats = flow_stats(self.vecs, self.mask, self.n_px) | _STATS_KNOW_MASK
        return self._stats

    def is_zero(self, thresholded=True, masked=True):
        """Flow.is_zero, flow_class.py:1230-1245."""
        s = self.stats()
        if masked:
            bit = nat.STAT_NONZERO_TH_MASKED if thresholded else nat.STAT_NONZERO_MASKED
        else:
            bit = nat.STAT_NONZERO_TH if thresholded else nat.STAT_NONZERO
        return not (s & bit)

    def get_padding(self):
        """Flow.get_padding (flow_class.py:1197-1228): one min/max reduction over the masked sampling positions."""
        h, w = self.shape
        ext = DeviceBuffer(16)
        nat.check(_lib().ofl_flow_extent_dev(self.vecs.ptr, self.mask.ptr, h, w, -1 if self.ref == 't' else 1,
                                             np.float32(DEFAULT_THRESHOLD), ext.ptr, None))
        min_y, max_y, min_x, max_x = (float(v) for v in ext.to_host((4,), np.float32))
        if not np.isfinite(min_y):
            raise ValueError("zero-size array to reduction operation minimum which has no identity")   # NumPy's error in the reference
        pads = [max(-min_y, 0), max(max_y - (h - 1), 0), max(-min_x, 0), max(max_x - (w - 1), 0)]
        return [int(np.ceil(p)) for p in pads]

    # -- element-wise algebra (Flow.__add__/__sub__/__neg__, flow_class.py:310-375, 479-489)
    def _axpy(self, other, alpha):
        out = DeviceFlow.empty(self.shape, self.ref)
        nat.check(_lib().ofl_axpy_dev(self.vecs.ptr, self.mask.ptr,
                                      other.vecs.ptr if other is not None else None,
                                      other.mask.ptr if other is not None else None,
                                      np.float32(alpha), self.n_px, out.vecs.ptr, out.mask.ptr, None))
        return out

    def __add__(self, other):
        return self._axpy(other, 1.0)

    def __sub__(self, other):
        return self._axpy(other, -1.0)

    def __neg__(self):
        out = self._axpy(None, -1.0)
        out._stats = self._stats            # the zero-flow predicates do not change under negation
        out._certs = {(-sg, pp): c for (sg, pp), c in self._certs.items()}      # x - (-f) is x + f: same warped grid
        return out

    # -- scaling (Flow.__mul__/__truediv__, flow_class.py:377-443) with a number, a list of 2 or an array of size 2
    def _scale(self, other, divide, verb, noun):
        k0, k1, wide = scale_operand(other, self.shape, verb, noun)
        out = DeviceFlow(DeviceBuffer(self.n_px * 8), self.mask, self.shape, self.ref)     # buffers are immutable: the mask is shared
        nat.check(_lib().ofl_scale_dev(self.vecs.ptr, k0, k1, divide, wide, self.n_px, out.vecs.ptr, None))
        return out              # fresh _stats / _certs: scaling moves vectors across the thresholds and changes the warped grid

    def __mul__(self, other):
        return self._scale(other, 0, "multiplying", "Multiplier")

    def __rmul__(self, other):
        try:
            float(other)
        except TypeError:
            return NotImplemented
        return self._scale(other, 0, "multiplying", "Multiplier")

    def __truediv__(self, other):
        return self._scale(other, 1, "dividing", "Divisor")

    def __pow__(self, other):
        raise TypeError("Error exponentiating flow: DeviceFlow has no '**' (NumPy's float32 power cannot be reproduced bit for "
                        "bit on the device); use the host Flow: Flow.from_device(f) ** exponent")

    # -- shape operations
    def pad(self, padding=None, mode=None):
        """Flow.pad (flow_class.py:508-526) in HBM: vectors padded with zeros ('constant'), the border values ('edge') or
        their mirror image ('symmetric'), the mask with 0.  All-zero padding returns `self`."""
        from .utils import get_valid_padding
        mode = 'constant' if mode is None else mode
        if mode not in _PAD_MODES:
            raise ValueError("Error padding flow: Mode should be one of "
                             "'constant', 'edge', 'symmetric', but instead got '{}'".format(mode))
        p = get_valid_padding(padding, "Error padding flow: ")
        if not any(p):
            return self
        h, w = self.shape
        out = DeviceFlow.empty((h + p[0] + p[1], w + p[2] + p[3]), self.ref)
        nat.check(_lib().ofl_pad_flow_dev(self.vecs.ptr, self.mask.ptr, h, w, p[0], p[1], p[2], p[3], _PAD_MODES[mode],
                                          out.vecs.ptr, out.mask.ptr, None))
        return out

    def __getitem__(self, item):
        """Flow.__getitem__ (flow_class.py:297-308) for a slice or a tuple of one or two slices (rows, columns; steps may
        be negative): a strided copy of vectors and mask."""
        (r0, rs, rows), (c0, cs, cols) = crop_args(item, self.shape)
        out = DeviceFlow.empty((rows, cols), self.ref)
        nat.check(_lib().ofl_crop_flow_dev(self.vecs.ptr, self.mask.ptr, self.shape[0], self.shape[1], r0, rs, rows, c0, cs, cols,
                                           out.vecs.ptr, out.mask.ptr, None))
        return out

    def _compose(self, sampled, sign, quant=nat.QUANT_OPENCV):
        """self + B(sampled; x + sign * self) with the masks of a warp followed by an addition: ONE launch of the
        fused compose kernel.  This is `g + g.apply(sampled)` for a 't'-reference g (sign -1) and
        `a + (-a as 't').apply(sampled)` for an 's'-reference a (sign +1) -- the expressions inside mode 1
        (flow_class.py:1369-1370, 1383-1385) -- bit for bit."""
        out = DeviceFlow.empty(self.shape, self.ref)
        compose3_launch(sampled, self, sign, out, quant=quant)
        return out

    # -- warping
    def apply(self, target, consider_mask=True, quant=nat.QUANT_OPENCV, target_mask=None):
        """Flow.apply with a Flow target (flow_class.py:600-603, 632-684): the target's vectors and mask
        are warped together; the result keeps the TARGET's reference.  A `DeviceImage` target returns
        (warped DeviceImage, valid-area DeviceBuffer) -- see apply_image."""
        if isinstance(target, DeviceImage):
            return self.apply_image(target, target_mask, consider_mask, quant)
        if self.ref == 't':
            # utils.py:215-216: a (thresholded-)zero flow returns the target itself.  Under cv2's 1/32-px coordinate
            # snapping the gather of such a flow IS the identity (|v| < 1e-3 snaps to 0), so the test -- a
            # reduction and a host synchronisation -- is only needed for the un-snapped extension mode
            if quant != nat.QUANT_OPENCV and self.is_zero(thresholded=True, masked=False):
                return target._and_mask(self)
            src = DeviceImage(target.vecs, self.shape + (2,), np.float32)
            dst, valid = gather_bilinear(src, self.vecs, self.shape, -1, smask=target.mask, fmask=self.mask,
                                         want_valid=True, quant=quant)
            return DeviceFlow(dst.buf, valid, self.shape, target.ref)
        return self._scatter_flow(target, consider_mask)

    def apply_image(self, image, target_mask=None, consider_mask=True, quant=nat.QUANT_OPENCV):
        """Warp an HBM-resident image [H][W][C] and propagate validity (Flow.apply with an ndarray target and
        return_valid_area=True, flow_class.py:604-695, without padding).  't': any remap dtype, one launch of
        the gather kernel; 's': float32 images through the scatter kernel.  `target_mask`: uint8 DeviceBuffer
        or None (all valid)."""
        h, w = self.shape
        if image.shape[:2] != (h, w):
            raise ValueError("image and flow need the same height and width")
        if self.ref == 't':
            if self.is_zero(thresholded=True, masked=False):        # identity short cut, utils.py:215-216
                valid = DeviceBuffer(self.n_px)
                if target_mask is None:
                    nat.check(_lib().ofl_copy_dev(valid.ptr, self.mask.ptr, self.n_px, None))
                else:
                    _mask_and(self.mask, target_mask, valid, self.n_px)
                return image, valid
            arith, rule = nat.ARITH_NATIVE, nat.RULE_EQ1
            if image.dtype == np.uint8:      # concat dtype of the reference: bool mask -> uint8, default int8 -> int16
                arith, rule = (nat.ARITH_NATIVE, nat.RULE_GE_HALF) if target_mask is not None else (nat.ARITH_FLOAT_RNE, nat.RULE_GT_HALF)
            elif image.dtype == np.int16 or (image.dtype == np.uint16 and target_mask is not None):
                rule = nat.RULE_GT_HALF
            elif image.dtype == np.uint16:
                raise TypeError("uint16 image with the default int8 mask needs an int32 remap, which cv2.remap does not provide")
            return gather_bilinear(image, self.vecs, self.shape, -1, smask=target_mask, fmask=self.mask,
                                   want_valid=True, quant=quant, arith=arith, rule=rule)
        if image.dtype != np.float32:
            raise TypeError("'s'-reference warps of device images need float32 (got {})".format(image.dtype))
        C = image.shape[2]
        vmask = self.mask
        if target_mask is not None:
            vmask = DeviceBuffer(self.n_px)
            _mask_and(target_mask, self.mask, vmask, self.n_px)                  # flow_class.py:643
        if self.is_zero(thresholded=True, masked=False):
            return image, vmask
        out = DeviceImage(DeviceBuffer(self.n_px * C * 4), image.shape, np.float32)
        valid = DeviceBuffer(self.n_px)
        pm = self._point_mask(consider_mask)
        scatter_linear(self.vecs, +1, pm, image.buf, C, vmask, h, w, None, out.buf, valid, 0,
                       cert=self.mesh_cert(+1) if pm is None else None, drops_points=pm is not None)
        return out, valid

    def apply_image_rows(self, image, rank, world, target_mask=None, consider_mask=True, quant=nat.QUANT_OPENCV,
                         gather=None, align=8):
        """This rank's ROW BAND of apply_image when ONE field is split over `world` GPUs (BASELINE config 5):
        flow, masks and image are the replicated H x W arrays, the result holds rows sharding.row_band(H, rank, world, align)
        only -- (DeviceImage rows x W x C, valid rows x W, (row0, row1)); the bands of all ranks concatenate to
        apply_image's result bit for bit.  't': one launch of the gather kernel on the band (nothing is exchanged).  's':
        a field whose mesh certifies resolves its rows in one kernel (nothing is exchanged); any other field takes the
        slab-wise Delaunay path with its one all-gather (`gather`: see scatter_slab; default RCCL)."""
        from .sharding import row_band
        h, w = self.shape
        if image.shape[:2] != (h, w):
            raise ValueError("image and flow need the same height and width")
        r0, r1 = row_band(h, rank, world, align)
        rows = r1 - r0
        C = image.shape[2]
        at = lambda buf, off, n: _BufferView(buf.ptr + off, n)
        if self.ref == 't':
            if rows <= 0:                       # more ranks than 8-row tiles: nothing to compute, and 't' exchanges nothing
                return None, None, (r0, r1)
            arith, rule = nat.ARITH_NATIVE, nat.RULE_EQ1
            if image.dtype == np.uint8:
                arith, rule = (nat.ARITH_NATIVE, nat.RULE_GE_HALF) if target_mask is not None else (nat.ARITH_FLOAT_RNE, nat.RULE_GT_HALF)
            elif image.dtype == np.int16 or (image.dtype == np.uint16 and target_mask is not None):
                rule = nat.RULE_GT_HALF
            elif image.dtype == np.uint16:
                raise TypeError("uint16 image with the default int8 mask needs an int32 remap, which cv2.remap does not provide")
            if self.is_zero(thresholded=True, masked=False):        # identity short cut, utils.py:215-216
                nb = rows * w * C * image.dtype.itemsize
                dst = DeviceImage(DeviceBuffer(nb), (rows, w, C), image.dtype)
                nat.check(_lib().ofl_copy_dev(dst.buf.ptr, image.buf.ptr + r0 * w * C * image.dtype.itemsize, nb, None))
                valid = DeviceBuffer(rows * w)
                if target_mask is None:
                    nat.check(_lib().ofl_copy_dev(valid.ptr, self.mask.ptr + r0 * w, rows * w, None))
                else:
                    _mask_and(at(self.mask, r0 * w, rows * w), at(target_mask, r0 * w, rows * w), valid, rows * w)
                return dst, valid, (r0, r1)
            dst, valid = gather_rows(image, r0, rows, at(self.vecs, r0 * w * 8, rows * w * 8), -1, smask=target_mask,
                                     fmask_rows=at(self.mask, r0 * w, rows * w), want_valid=True, quant=quant, arith=arith, rule=rule)
            return dst, valid, (r0, r1)
        if image.dtype != np.float32:
            raise TypeError("'s'-reference warps of device images need float32 (got {})".format(image.dtype))
        vmask = self.mask
        if target_mask is not None:
            vmask = DeviceBuffer(self.n_px)
            _mask_and(target_mask, self.mask, vmask, self.n_px)                  # flow_class.py:643
        if self.is_zero(thresholded=True, masked=False):
            if rows <= 0:
                return None, None, (r0, r1)
            nb = rows * w * C * 4
            dst = DeviceImage(DeviceBuffer(nb), (rows, w, C), np.float32)
            nat.check(_lib().ofl_copy_dev(dst.buf.ptr, image.buf.ptr + r0 * w * C * 4, nb, None))
            valid = DeviceBuffer(rows * w)
            nat.check(_lib().ofl_copy_dev(valid.ptr, vmask.ptr + r0 * w, rows * w, None))
            return dst, valid, (r0, r1)
        # (a rank with an EMPTY band -- more ranks than 8-row tiles -- still walks through the path decision below: the
        # slab-wise path has two all-gathers that every rank of `world` must join, scatter_slab with rows == 0)
        out = DeviceImage(DeviceBuffer(max(rows, 0) * w * C * 4), (max(rows, 0), w, C), np.float32)
        valid = DeviceBuffer(max(rows, 0) * w)
        pm = self._point_mask(consider_mask)
        cert = self.mesh_cert(+1) if pm is None else None
        if cert is not None and cert.certified and not getattr(cert, "_walk_checked", False):
            # Does the walk kernel find every node of this certified mesh (scatter_linear)?  The answer must be the SAME on
            # every rank -- a rank that went on alone to the slab-wise path would wait for the others in its all-gather --
            # so each rank asks for the whole field once per certificate (validity only: 0.1 ms at 4K), not for its band.
            cnt, scratch = DeviceBuffer.zeros(16), DeviceBuffer(self.n_px)
            nat.check(_lib().ofl_scatter_certified_dev(self.vecs.ptr, +1, 0, None, 0, vmask.ptr, h, w, 0, h,
                                                       None, scratch.ptr, 0, ctypes.byref(cert), cnt.ptr, None))
            if int(cnt.to_host((1,), np.uint32)[0]) == 0:
                cert._walk_checked = True
            else:
                cert.certified = 0
        if cert is not None and cert.certified:
            if rows <= 0:
                return None, None, (r0, r1)
            nat.check(_lib().ofl_scatter_certified_dev(self.vecs.ptr, +1, 0, image.buf.ptr, C, vmask.ptr, h, w, r0, rows,
                                                       out.buf.ptr, valid.ptr, 0, ctypes.byref(cert), None, None))
            return out, valid, (r0, r1)
        if world <= 1:
            scatter_linear(self.vecs, +1, pm, image.buf, C, vmask, h, w, None, out.buf, valid, nat.SCATTER_UNCERTIFIED)
        else:
            scatter_slab(self.vecs, +1, pm, image.buf, C, vmask, h, w, r0, rows, out.buf, valid, rank, world,
                         gather=gather if gather is not None else comm_allgather)
            if rows <= 0:
                return None, None, (r0, r1)
        return out, valid, (r0, r1)

    def resize(self, scale):
        """Flow.resize (flow_class.py:491-506) on HBM-resident data: one launch of the resize kernel."""
        fy, fx = resize_scales(scale)
        h, w = self.shape
        ho, wo = resized_shape(h, w, fy, fx)
        out = DeviceFlow.empty((ho, wo), self.ref)
        nat.check(_lib().ofl_resize_flow_dev(self.vecs.ptr, self.mask.ptr, h, w, ho, wo, 1.0 / fy, 1.0 / fx,
                                             float(np.float32(fx)), float(np.float32(fy)), out.vecs.ptr, out.mask.ptr, None))
        return out

    def visualise(self, mode, show_mask=False, show_mask_borders=False, range_max=None):
        """Flow.visualise (flow_class.py:869-951) on HBM-resident data -> DeviceImage uint8 (H, W, 3), asynchronous: the
        default scale (99th percentile of the magnitudes, with the reference's fallbacks) is selected on the device and read
        there by the render kernel."""
        code, flags, rc = visualise_args(mode, show_mask, show_mask_borders, range_max)
        h, w = self.shape
        rng = None
        if rc is None:
            rng = DeviceBuffer(16)
            visualise_range_launch(self.vecs, h, w, 1, rng)
        return visualise_launch(self.vecs, self.mask, h, w, 1, code, flags, rng, rc)

    def visualise_range(self):
        """The range_max visualise() uses by default, as a Python float (one synchronisation): fixes one scale for a
        sequence of fields."""
        h, w = self.shape
        rng = DeviceBuffer(16)
        visualise_range_launch(self.vecs, h, w, 1, rng)
        return float(rng.to_host((1,), np.float32)[0])

    def matrix(self, dof=None, method=None, masked=None, seed=None):
        """Flow.matrix (flow_class.py:797-867) on HBM-resident data -> (3, 3) float64: the affine (dof 4 / 6) or projective
        (dof 8) matrix fitted to the field by least squares ('lms', dof 8), RANSAC or least median ('lmeds').  Every pass
        over the field runs on the device (K8); the host solves the small systems (matrix_fit).  `seed` seeds the sampling
        of minimal sets: the same field and seed give the same bits.  Not bit-compatible with OpenCV's estimators."""
        from . import matrix_fit
        dof, method, masked, seed = matrix_fit.matrix_args(dof, method, masked, seed)
        field = FitField(self.vecs, self.mask if masked else None, self.shape, -1 if self.ref == 't' else 1)
        return matrix_fit.fit(field, dof, method, seed, zero=self.is_zero(thresholded=False, masked=masked))

    def _stats_word(self):
        """The field's OFL_STAT_* word as a device uint32 (what the tracking kernels read for the zero-flow rule): the cached
        statistics go up as 4 bytes; a field without any gets one asynchronous launch of the statistics kernel."""
        if self._stats_buf is None:
            if self._stats is not None:
                self._stats_buf = DeviceBuffer.from_host(np.array([self._stats & 0x3f], np.uint32))
            else:
                self._stats_buf = DeviceBuffer(16)
                stats_word_launch(self.vecs.ptr, self.mask.ptr, self.n_px, self._stats_buf.ptr)
        return self._stats_buf

    def track(self, pts, int_out=None, get_valid_status=None, s_exact_mode=None):
        """Flow.track (flow_class.py:755-795, utils.py:547-622) on an HBM-resident field: the field is neither uploaded nor
        downloaded.  `pts`: a DevicePoints -- the answer is a DevicePoints (and, with get_valid_status, a uint8 DeviceBuffer
        [n]) -- or an (n, 2) array, which is uploaded, points only, and answered with arrays like the reference.  All four
        paths: ref 's' with integer points, with bilinear sampling and with s_exact_mode, and ref 't'.  Equal to Flow.track
        bit for bit, except that
          - the result is float64 (int32 with int_out) whatever the points' dtype: for a thresholded-zero flow the reference
            hands integer points back as they are;
          - an integer index outside the field raises IndexError, also a negative one that NumPy would wrap around;
          - the status of a point whose rounded position is no pixel of the field is False, where NumPy wraps or raises.
        Raises IndexError for points outside the area on the non-query 's' paths (one 4-byte read-back), like the reference."""
        int_out, get_valid_status, s_exact_mode = track_args(pts, int_out, get_valid_status, s_exact_mode)
        on_host = not isinstance(pts, DevicePoints)
        dp = DevicePoints.from_host(pts) if on_host else pts
        h, w = self.shape
        n = dp.n
        out = DevicePoints(DeviceBuffer(n * (8 if int_out else 16)), n, np.int32 if int_out else np.float64)
        valid = self.valid_source() if get_valid_status else None
        status = DeviceBuffer(n) if get_valid_status else None
        if n:
            words = self._stats_word()
            if self.ref == 's' and (dp.dtype.kind == 'i' or not s_exact_mode):
                outside = DeviceBuffer.zeros(16)
                if dp.dtype.kind == 'i':
                    nat.check(_lib().ofl_track_pixels_dev(self.vecs.ptr, h, w, dp.buf.ptr, _TRACK_DT[dp.dtype], n, words.ptr,
                                                          _ptr(valid), int(int_out), out.buf.ptr, _ptr(status), outside.ptr, None))
                else:
                    track_bilinear_launch(self.vecs.ptr, 1, self.shape, False, dp, words, valid, int_out, out.buf, status,
                                          outside=outside)
                if int(outside.to_host((1,), np.uint32)[0]):
                    raise IndexError("Some points are outside of the data area.")
            else:
                query = track_query_points(dp)
                if self.ref == 's':      # exact mode: values live on the undisplaced regular grid
                    pos, sign = DeviceBuffer.zeros(self.n_px * 8), 1
                else:                    # 't': values live at grid - flow
                    pos, sign = self.vecs, -1
                vals, found = scatter_query_resident(pos, sign, self.vecs, h, w, query, n)
                track_query_epilogue(query, vals, found, n, self.shape, words, valid, -1, status,
                                     out_rc=None if int_out else out.buf, out_int=out.buf if int_out else None)
        if not on_host:
            return (out, status) if get_valid_status else out
        res = out.to_host()
        return (res, status.to_host((n,), np.uint8).view(np.bool_)) if get_valid_status else res

    def _and_mask(self, other):
        """vecs unchanged, mask = self.mask & other.mask (zero-flow identity warp of a Flow target)."""
        out_mask = DeviceBuffer(self.n_px)
        scratch = DeviceBuffer(self.n_px * 8)
        nat.check(_lib().ofl_axpy_dev(self.vecs.ptr, self.mask.ptr, None, other.mask.ptr, np.float32(1.0),
                                      self.n_px, scratch.ptr, out_mask.ptr, None))
        return DeviceFlow(scratch, out_mask, self.shape, self.ref)

    def _point_mask(self, consider_mask=True):
        """The point mask of utils.py:249-251 -- None when every point is kept (same result, and the scatter kernel then
        skips its per-pixel search for dropped neighbours).  Only statistics that come from ofl_flow_stats know the
        mask; predicates taken over from the compose kernel do not."""
        if not consider_mask:
            return None
        if self._stats is None or not (self._stats & _STATS_KNOW_MASK):
            self._stats = flow_stats(self.vecs, self.mask, self.n_px) | _STATS_KNOW_MASK
        return self.mask if (self._stats & nat.STAT_MASK_HAS_ZERO) else None

    def _scatter_flow(self, target, consider_mask=True, sign=1, negate=False):
        """'s'-reference apply of a Flow target: utils.py:237-258 + flow_class.py:634-643, 668.  negate: the target is
        -`target` (its vectors are negated inside the kernel, OFL_SCATTER_NEGATE)."""
        if self.is_zero(thresholded=True, masked=False):
            return (-target if negate else target)._and_mask(self)
        h, w = self.shape
        out = DeviceFlow.empty(self.shape, target.ref)
        if target.mask is self.mask:
            vmask = self.mask                                     # m & m
        else:
            vmask = DeviceBuffer(self.n_px)
            _mask_and(target.mask, self.mask, vmask, self.n_px)  # mask channel, flow_class.py:643
        pm = self._point_mask(consider_mask)
        scatter_linear(self.vecs, sign, pm, target.vecs, 2, vmask, h, w, None, out.vecs, out.mask,
                       nat.SCATTER_NEGATE if negate else 0, cert=self.mesh_cert(sign) if pm is None else None, drops_points=pm is not None)
        return out

    def switch_ref(self):
        """Flow.switch_ref(mode='valid'), flow_class.py:716-726."""
        other = 't' if self.ref == 's' else 's'
        if self.is_zero(thresholded=False):
            return self.relabel(other)
        if self.ref == 's':
            return self.apply(self).relabel('t')
        as_s = self.relabel('s')
        return (-as_s).apply(as_s)

    def invert(self, ref=None):
        """Flow.invert, flow_class.py:735-753."""
        ref = self.ref if ref is None else ref
        if self.ref == 's':
            # s -> s: self.apply(-self) (flow_class.py:746) -- the negation happens inside the scatter kernel
            return self._scatter_flow(self, negate=True) if ref == 's' else (-self).relabel('t')
        if ref == 's':
            return (-self).relabel('s')
        return self.invert('s').switch_ref()

    def combine_with(self, flow, mode, thresholded=False, quant=nat.QUANT_OPENCV):
        """Flow.combine_with, flow_class.py:1338-1424.  Returns `self` / `flow` themselves on the
        reference's zero-flow early exits."""
        if mode == 3:
            return self._combine3(flow, thresholded, quant)
        if self.is_zero(thresholded=thresholded):
            return flow
        if flow.is_zero(thresholded=thresholded):
            return self.invert()
        s = self.ref == 's'
        if mode == 1:
            if s:                                                            # flow_class.py:1369-1370
                g = flow.invert('t')
                return flow - g._compose(self.switch_ref(), -1, quant).apply(self)       # g + g.apply(..), fused
            a = self.switch_ref()                                            # flow_class.py:1383-1385
            res = flow.switch_ref() - a._compose(flow.invert('s'), +1, quant).apply(a)  # a + (-a).apply(..), fused
            return res.switch_ref()
        if s:
            return self.apply(flow - self)                                   # flow_class.py:1390
        return flow - self._resample_to(flow)                                # flow_class.py:1398-1410

    def _combine3(self, flow, thresholded, quant):
        """Mode 3 through the fused kernel K2.  The early-exit predicates of flow_class.py:1339-1354 and
        utils.py:215 are evaluated by the same launch (stat words) and honoured afterwards."""
        if self.ref == 's':
            fa, fb, sign = flow, self, +1          # self + self.invert('t').apply(flow)   (:1418)
        else:
            fa, fb, sign = self, flow, -1          # flow + flow.apply(self)               (:1422)
        out = DeviceFlow.empty(self.shape, self.ref)
        need = fa._stats is None or fb._stats is None
        words = DeviceBuffer.zeros(32) if need else None
        compose3_launch(fa, fb, sign, out, words, quant=quant)
        cert_a = 0
        if need:
            w = words.to_host((8,), np.uint32)
            if fb._stats is None:                       # exact predicates of the streamed field
                fb._stats = sum((1 << k) for k in range(4) if w[4 + k])
            cert_a = (1 if w[0] else 0) | (2 if w[1] else 0)   # certificates "fa is not zero"
        bit = nat.STAT_NONZERO_TH_MASKED if thresholded else nat.STAT_NONZERO_MASKED
        if fa._stats is None and not (cert_a & bit):
            fa.stats()                                  # not certified by the gather: exact pass (K4)
        a_zero = fa.is_zero(thresholded=thresholded) if fa._stats is not None else False
        b_zero = fb.is_zero(thresholded=thresholded)
        self_zero, flow_zero = (b_zero, a_zero) if self.ref == 's' else (a_zero, b_zero)
        if self_zero:
            return flow
        if flow_zero:
            return self
        if fb.is_zero(thresholded=True, masked=False):
            # apply_flow returned the target untouched (utils.py:215-216): plain vector sum
            return fb + fa
        return out

    def _resample_to(self, flow3):
        """Mode 2 / ref 't' (flow_class.py:1398-1410): self sampled from the float32 points x - self onto
        the points x - flow3 (no mask filtering); mask = interpolated mask > 0.99."""
        h, w = self.shape
        out = DeviceFlow.empty(self.shape, 't')
        query = DeviceBuffer(self.n_px * 8)
        grid_minus(flow3.vecs, query, h, w)
        scatter_linear(self.vecs, -1, None, self.vecs, 2, self.mask, h, w, query, out.vecs, out.mask, 1,
                       point_precision=1)
        return out

    def valid_target(self, consider_mask=True, quant=nat.QUANT_OPENCV):
        """flow_class.py:1113-1151 -> uint8 mask buffer."""
        h, w = self.shape
        if self.ref == 't':
            if self.is_zero(thresholded=True, masked=False):
                return self.mask
            return gather_valid_only(h, w, self.vecs, self.shape, -1, fmask=self.mask, quant=quant)
        return self._scatter_mask(+1, consider_mask)

    def valid_source(self, consider_mask=True, quant=nat.QUANT_OPENCV):
        """flow_class.py:1153-1195 -> uint8 mask buffer."""
        h, w = self.shape
        if self.ref == 's':
            if self.is_zero(thresholded=True, masked=False):
                return self.mask
            return gather_valid_only(h, w, self.vecs, self.shape, +1, fmask=self.mask, quant=quant)
        return self._scatter_mask(-1, consider_mask)

    def _scatter_mask(self, sign, consider_mask):
        """apply_flow(+-vecs, mask.astype('f'), 's', mask|None) == 1  (flow_class.py:1140-1141, 1190-1193)."""
        if self.is_zero(thresholded=True, masked=False):
            return self.mask
        h, w = self.shape
        valid = DeviceBuffer(self.n_px)
        pm = self._point_mask(consider_mask)
        scatter_linear(self.vecs, sign, pm, None, 0, self.mask, h, w, None, None, valid, 0,
                       cert=self.mesh_cert(sign) if pm is None else None, drops_points=pm is not None)
        return valid


# ------------------------------------------------------------------------------ small helpers
def _mask_and(a, b, out, n):
    """out = a & b for uint8 masks (flow_class.py:643)."""
    nat.check(_lib().ofl_mask_and_dev(a.ptr, b.ptr, out.ptr, n, None))


def resize_scales(scale, error_string="Error resizing flow: "):
    """Validation of resize_flow's `scale` (utils.py:505-518): returns (vertical, horizontal) factors."""
    if isinstance(scale, (float, int)):
        scale = [scale, scale]
    elif isinstance(scale, (tuple, list)):
        if len(scale) != 2:
            raise ValueError(error_string + "Scale {} must have a length of 2".format(type(scale)))
        if not all(isinstance(item, (float, int)) for item in scale):
            raise ValueError(error_string + "Scale {} items must be integers or floats".format(type(scale)))
    else:
        raise TypeError(error_string + "Scale must be an integer, float, or list or tuple of integers or floats")
    if any(s <= 0 for s in scale):
        raise ValueError(error_string + "Scale values must be larger than 0")
    return float(scale[0]), float(scale[1])


def resized_shape(h, w, fy, fx):
    """cv2.resize(dsize=None, fx, fy): dsize = (cvRound(W * fx), cvRound(H * fy)), round half to even."""
    ho, wo = int(np.rint(h * fy)), int(np.rint(w * fx))
    if ho <= 0 or wo <= 0:
        raise ValueError("Error resizing flow: scale {} leaves no pixels of a {}x{} field".format((fy, fx), h, w))
    return ho, wo


def resize_host(vecs, mask, scale):
    """resize_flow / Flow.resize for host arrays through ofl_resize_flow (upload, one launch, download)."""
    fy, fx = resize_scales(scale)
    vecs = np.ascontiguousarray(vecs, np.float32)
    h, w = vecs.shape[:2]
    ho, wo = resized_shape(h, w, fy, fx)
    out = np.empty((ho, wo, 2), np.float32)
    m = None if mask is None else np.ascontiguousarray(mask).astype(np.uint8)
    mout = None if mask is None else np.empty((ho, wo), np.uint8)
    hp = lambda a: None if a is None else a.ctypes.data
    nat.check(_lib().ofl_resize_flow(hp(vecs), hp(m), h, w, ho, wo, 1.0 / fy, 1.0 / fx,
                                     float(np.float32(fx)), float(np.float32(fy)), hp(out), hp(mout)))
    return out, (None if mout is None else mout.astype(bool))


def grid_minus(vecs, out, h, w):
    """out = float32(grid - vecs): the query positions of mode 2 / ref 't' (flow_class.py:1404-1406)."""
    nat.check(_lib().ofl_grid_offset_dev(vecs.ptr, -1, h, w, out.ptr, None))


_ws_cache = {}


def _workspace(h, w, C, stream=None):
    """Scatter workspace for fields of this shape -- one per (shape, stream): calls on different streams may overlap, and
    each then needs bucket lists and an owner map of its own."""
    key = (h, w, getattr(stream, "value", stream) or 0)
    ws = _ws_cache.get(key)
    if ws is None:
        n = ctypes.c_size_t(0)
        nat.check(_lib().ofl_scatter_workspace_bytes(h, w, C, ctypes.byref(n)))
        if len(_ws_cache) > 6:
            _ws_cache.clear()
        ws = _ws_cache[key] = DeviceBuffer(n.value)
    return ws


def scatter_linear(flow, sign, pmask, vals, C, vmask, h, w, query, out, valid, valid_rule, point_precision=0,
                   stream=None, cert=None, drops_points=False):
    """K3: scattered -> regular-grid linear interpolation.  Replaces utils.py:237-258 (and, with `query`,
    flow_class.py:1398-1410).  Raises ValueError("No points given") like qhull when nothing is kept.
    cert: a MeshCert of this very (flow, sign, point_precision) without point mask; when it certifies the mesh the
    asynchronous one-kernel entry is taken (no workspace, no read-back).  drops_points: pmask is KNOWN to hold zeros
    (the flow's statistics say so); like a certificate that says "not certified" this spares the entry its own certificate
    pass (OFL_SCATTER_UNCERTIFIED)."""
    ptr = lambda b: b.ptr if b is not None else None
    if cert is not None and cert.certified and pmask is None and query is None:
        # The certificate says the mesh IS the triangulation; that the walk kernel also FINDS every node in it is checked on
        # the first launch with this certificate (a device counter, one read-back): which nodes it locates depends on the
        # field and the sign only, so later launches with the same cached certificate run without any synchronisation.
        checked = getattr(cert, "_walk_checked", False)
        cnt = None if checked else DeviceBuffer.zeros(16, stream)
        nat.check(_lib().ofl_scatter_certified_dev(flow.ptr, sign, point_precision, ptr(vals), C, ptr(vmask), h, w, 0, h,
                                                   ptr(out), ptr(valid), valid_rule, ctypes.byref(cert), ptr(cnt), stream))
        if checked or int(cnt.to_host((1,), np.uint32, stream)[0]) == 0:
            cert._walk_checked = True
            return (h * w, 0, 0)
        cert.certified = 0                                  # nodes were lost: this field takes the Delaunay path from now on
    if (cert is not None and not cert.certified and pmask is None) or (drops_points and pmask is not None):
        valid_rule |= nat.SCATTER_UNCERTIFIED          # the certificate pass has been run for this field: not again per call
    ws = _workspace(h, w, C, stream)
    info = (ctypes.c_uint64 * 3)()
    nat.check(_lib().ofl_scatter_linear_dev(flow.ptr, sign, point_precision, ptr(pmask), ptr(vals), C, ptr(vmask),
                                            h, w, ptr(query), ptr(out), ptr(valid), valid_rule, ws.ptr, ws.nbytes,
                                            info, stream))
    return tuple(info)


def scatter_linear_f64(flow, sign, pmask, vals, C, vmask, h, w, out, valid, valid_rule, point_precision=0, stream=None):
    """K3 with float64 values at the grid nodes (float64 targets of apply_flow 's', utils.py:253-258)."""
    ws = _workspace(h, w, C, stream)
    info = (ctypes.c_uint64 * 3)()
    ptr = lambda b: b.ptr if b is not None else None
    nat.check(_lib().ofl_scatter_linear_f64_dev(flow.ptr, sign, point_precision, ptr(pmask), ptr(vals), C, ptr(vmask),
                                                h, w, ptr(out), ptr(valid), valid_rule, ws.ptr, ws.nbytes, info, stream))
    return tuple(info)


def scatter_rows(flow, sign, pmask, vals, C, vmask, h, w, row0, rows, out_rows, valid_rows, valid_rule=0,
                 point_precision=0, stream=None):
    """K3 on one row band of a field split over several GPUs (SURVEY 8e, config 5 as loaded): all inputs are the
    replicated H x W arrays; only rows [row0, row0 + rows) of the result are produced."""
    ws = _workspace(h, w, C, stream)
    info = (ctypes.c_uint64 * 3)()
    ptr = lambda b: b.ptr if b is not None else None
    nat.check(_lib().ofl_scatter_rows_dev(flow.ptr, sign, point_precision, ptr(pmask), ptr(vals), C, ptr(vmask),
                                          h, w, row0, rows, ptr(out_rows), ptr(valid_rows), valid_rule, ws.ptr, ws.nbytes,
                                          info, stream))
    return tuple(info)


SLAB_LIST_HEAD = 16          # bytes before the first record of a slab list (entries, error bits, 0, 0)
SLAB_RECORD = 64             # bytes per unfinished site


def slab_list_bytes(entries):
    return SLAB_LIST_HEAD + SLAB_RECORD * int(entries)


def comm_allgather(send_ptr, recv, nbytes, stream=None):
    """ncclAllGather of `nbytes` per rank over the live communicator (send may be the rank's own slot of recv)."""
    nat.check(_lib().ofl_comm_allgather(send_ptr, recv.ptr, nbytes, stream))


def scatter_slab_stars(flow, sign, pmask, h, w, row0, rows, list_ptr, list_bytes, point_precision=0, stream=None, ws=None):
    """Step 1 of the slab-wise scatter (include/ofl.h, ofl_scatter_slab_stars_dev): bins, the stars around rows
    [row0, row0 + rows) and -- at list_ptr (device) -- the unfinished sites of those rows.  The workspace keeps the star
    state for scatter_slab_finish: `ws` (a DeviceBuffer the caller holds on to across both steps, as scatter_slab does) or
    the cached one of this (shape, stream) -- then no other scatter call of that shape on that stream in between, and
    nothing that makes the cache drop it (step 2 refuses a workspace without step 1's stamp)."""
    ws = ws if ws is not None else _workspace(h, w, 0, stream)
    nat.check(_lib().ofl_scatter_slab_stars_dev(flow.ptr, sign, point_precision, pmask.ptr if pmask is not None else None,
                                                h, w, row0, rows, list_ptr, list_bytes, ws.ptr, ws.nbytes, stream))


def scatter_slab_finish(flow, sign, vals, C, vmask, h, w, row0, rows, lists, list_bytes, n_lists, out_rows, valid_rows,
                        valid_rule=0, point_precision=0, stream=None, ws=None):
    """Step 2: the gathered lists of all ranks -> unfinished stars, owner map and result of the band."""
    ws = ws if ws is not None else _workspace(h, w, 0, stream)
    info = (ctypes.c_uint64 * 3)()
    ptr = lambda b: b.ptr if b is not None else None
    nat.check(_lib().ofl_scatter_slab_finish_dev(flow.ptr, sign, point_precision, ptr(vals), C, ptr(vmask), h, w, row0, rows,
                                                 lists.ptr, list_bytes, n_lists, ptr(out_rows), ptr(valid_rows), valid_rule,
                                                 ws.ptr, ws.nbytes, info, stream))
    return tuple(info)


SLAB_ERR_LIST = 32           # error bit of a list head: the rank's unfinished sites did not fit its list (kErrSlabList)


def _slab_timeout():
    import os
    return float(os.environ.get("OFL_SLAB_TIMEOUT", "120"))


def scatter_slab(flow, sign, pmask, vals, C, vmask, h, w, row0, rows, out_rows, valid_rows, rank=0, world=1, valid_rule=0,
                 point_precision=0, stream=None, entries=1 << 17, gather=comm_allgather, timeout=None):
    """One row band of a ref-'s' warp whose mesh does not certify, with the star passes sharded over `world` ranks
    (SURVEY 8e, config 5): step 1 into a list of up to `entries` records, the exchange, step 2.  The exchange is two
    all-gathers -- the 16-byte list heads first, then (one read-back of the counts later) only as many 64-byte records per
    rank as the fullest list holds: config 5 at 8K leaves 75 000 sites unfinished in all, 1 MB per rank instead of the
    8 MiB the buffers are sized for.  `gather(send_ptr, recv_buffer, nbytes, stream)` defaults to RCCL over the live
    communicator (sharding.host_allgather(dist) goes through the host instead: rehearsals with ranks that share a GPU).
    Bands concatenate to scatter_linear's result bit for bit.

    Every rank of `world` MUST call this, whatever its band: a rank with an EMPTY band (rows == 0: more ranks than 8-row
    tiles) skips both steps but takes part in both gathers with an empty list; a rank whose step 1 fails joins them with an
    error head and raises afterwards, so that its peers fail with it instead of waiting for it.  When some rank's list
    overflowed (`entries` too small: large holes, hull sites of an 8K field) every rank sees the same counts in the gathered
    heads and all of them repeat the exchange ONCE with lists sized for the fullest.  Each gather -- and the read-back that
    waits for it -- is bounded by `timeout` seconds (default: OFL_SLAB_TIMEOUT, 120): a rank left alone in the collective
    ends its process with exit code 3 (sharding.bounded_call) instead of hanging for ever."""
    if world <= 1 and (row0 != 0 or rows != h):
        raise ValueError("scatter_slab: a band of a field needs the other ranks' lists")
    from .sharding import slab_payload_entries, bounded_call
    world = max(int(world), 1)
    timeout = _slab_timeout() if timeout is None else timeout
    ws = _workspace(h, w, 0, stream)               # held across both steps: whatever the exchange does to the cache, step 2 finds step 1's state
    for attempt in range(2):
        nb = slab_list_bytes(entries)
        mine = DeviceBuffer(nb)
        failed = None
        if rows > 0:
            try:
                scatter_slab_stars(flow, sign, pmask, h, w, row0, rows, mine.ptr, nb, point_precision, stream, ws)
            except nat.NativeError as e:            # the peers are on their way into the gathers: join them, then raise
                failed = e
        if rows <= 0 or failed is not None:
            head = np.array([0, SLAB_ERR_LIST if failed is not None else 0, 0, 0], np.uint32)
            nat.check(_lib().ofl_upload(mine.ptr, head.ctypes.data, SLAB_LIST_HEAD, stream))
            nat.check(_lib().ofl_stream_sync(stream))
        if world == 1:
            if failed is not None:
                raise failed
            return scatter_slab_finish(flow, sign, vals, C, vmask, h, w, row0, rows, mine, nb, 1, out_rows, valid_rows,
                                       valid_rule, point_precision, stream, ws)
        heads = DeviceBuffer(SLAB_LIST_HEAD * world)

        def exchange_heads():
            gather(mine.ptr, heads, SLAB_LIST_HEAD, stream)
            return heads.to_host((world, SLAB_LIST_HEAD // 4), np.uint32, stream)
        hw = bounded_call(exchange_heads, timeout, "the all-gather of the slab list heads")
        counts, errs = hw[:, 0], hw[:, 1]
        if attempt == 0 and int(counts.max()) > entries and not errs.any():
            # some rank's list overflowed; every rank reads the same heads and takes this branch together
            entries = int(counts.max()) + 1024
            continue
        m = slab_payload_entries(counts, entries)
        nb2 = slab_list_bytes(m)
        lists = DeviceBuffer(nb2 * world)

        def exchange_lists():
            gather(mine.ptr, lists, nb2, stream)
            nat.check(_lib().ofl_stream_sync(stream))
        bounded_call(exchange_lists, timeout, "the all-gather of the slab lists")
        if failed is not None:
            raise failed
        if rows <= 0:
            return (0, 0, 0)
        # (error bits in a peer's head -- a refused point set, a step 1 that failed there -- reach step 2 with the lists: it
        # blanks this band and raises here as well, include/ofl.h)
        return scatter_slab_finish(flow, sign, vals, C, vmask, h, w, row0, rows, lists, nb2, world, out_rows, valid_rows,
                                   valid_rule, point_precision, stream, ws)


def scatter_host(flow, target, pmask, vmask=None):
    """apply_flow(flow, target, 's', mask) for host arrays (utils.py:237-258; `flow` may already be a DeviceBuffer
    holding the float32 vectors): target (H, W, C) of any numeric
    dtype is interpolated in float32/float64 on the device, then rounded / cast back like the reference.
    Returns (warped, valid or None); valid = float32(interpolated vmask) == 1 (flow_class.py:668)."""
    h, w, C = target.shape
    n = h * w * C
    fbuf = flow if isinstance(flow, DeviceBuffer) else DeviceBuffer.from_host(np.ascontiguousarray(flow, np.float32))
    as_mask = lambda m: np.ascontiguousarray(m).view(np.uint8) if m.dtype == np.bool_ else np.ascontiguousarray(m).astype(np.uint8)
    pm = DeviceBuffer.from_host(as_mask(pmask)) if pmask is not None else None
    vm = DeviceBuffer.from_host(as_mask(vmask)) if vmask is not None else None
    valid = DeviceBuffer(h * w) if vmask is not None else None
    if target.dtype == np.float64:                                           # griddata's own precision end to end
        vals = DeviceBuffer.from_host(np.ascontiguousarray(target))
        out = DeviceBuffer(n * 8)
        scatter_linear_f64(fbuf, +1, pm, vals, C, vm, h, w, out, valid, 0)
        v = valid.to_host((h, w), np.uint8).view(np.bool_) if valid is not None else None
        return out.to_host((h, w, C), np.float64), v
    native = target.dtype in _DT_CODE and target.dtype != np.float32         # the casts of utils.py:253 / :258 run on the device
    integer = np.issubdtype(target.dtype, np.integer)
    if native:
        raw = DeviceBuffer.from_host(np.ascontiguousarray(target))
        vals = DeviceBuffer(n * 4)
        nat.check(_lib().ofl_convert_dev(raw.ptr, _DT_CODE[target.dtype], vals.ptr, nat.F32, n, None))
    else:
        vals = DeviceBuffer.from_host(np.ascontiguousarray(target, np.float32))
    out = DeviceBuffer(n * 4)
    # integer targets: values AND the concatenated mask channel are np.round-ed before the cast (utils.py:256-257)
    scatter_linear(fbuf, +1, pm, vals, C, vm, h, w, None, out, valid, (nat.SCATTER_ROUND | 2) if integer else 0)
    if native:
        back = DeviceBuffer(n * target.dtype.itemsize)
        nat.check(_lib().ofl_convert_dev(out.ptr, nat.F32, back.ptr, _DT_CODE[target.dtype], n, None))
        res = back.to_host((h, w, C), target.dtype)
    else:
        res = out.to_host((h, w, C), np.float32).astype(target.dtype)       # already rounded for integer targets
    v = valid.to_host((h, w), np.uint8).view(np.bool_) if valid is not None else None
    return res, v


def sample_points(flow_buf, h, w, pts_rc):
    """Bilinear flow samples (v, u) at float64 points (row, col): utils.py:161-196 / :605."""
    pts = np.ascontiguousarray(pts_rc, np.float64)
    n = pts.shape[0]
    dp = DeviceBuffer.from_host(pts)
    out = DeviceBuffer(max(n, 1) * 16)
    nat.check(_lib().ofl_sample_points_dev(flow_buf.ptr, h, w, dp.ptr, n, out.ptr, None))
    return out.to_host((n, 2), np.float64)


def scatter_query(pos_flow_buf, sign, vals_buf, C, h, w, query_xy, pmask=None):
    """griddata(points, values, query) for sparse float64 query points (utils.py:603, 614).
    Returns (values float64 [n, C], found bool [n])."""
    q = np.ascontiguousarray(query_xy, np.float64)
    n = q.shape[0]
    dq = DeviceBuffer.from_host(q)
    out = DeviceBuffer(max(n, 1) * C * 8)
    found = DeviceBuffer(max(n, 1))
    ws = _workspace(h, w, C)
    nat.check(_lib().ofl_scatter_query_dev(pos_flow_buf.ptr, sign, 0, pmask.ptr if pmask is not None else None,
                                           vals_buf.ptr, C, h, w, dq.ptr, n, out.ptr, found.ptr, ws.ptr, ws.nbytes, None))
    return out.to_host((n, C), np.float64), found.to_host((n,), np.uint8).view(np.bool_)


# ------------------------------------------------------------------------------ K10: tracking with resident points
def _ptr(buf):
    return buf.ptr if buf is not None else None


def stats_word_launch(vecs_ptr, mask_ptr, n_px, out_ptr, stream=None):
    """K4 into a device uint32 at out_ptr, asynchronous: the OFL_STAT_* word of one field, left in HBM for a kernel to read."""
    nat.check(_lib().ofl_flow_stats_dev(vecs_ptr, mask_ptr, n_px, np.float32(DEFAULT_THRESHOLD), out_ptr, stream))


def track_bilinear_launch(flows_ptr, n_fields, shape, chain, pts, stats, valid, int_out, out, status, outside=None,
                          lost_at=None, path=None, stream=None):
    """K10, ref 's' with bilinear sampling (ofl_track_bilinear_dev); asynchronous.  pts: float64 DevicePoints."""
    if pts.dtype != np.float64:
        raise TypeError("Error tracking points: the bilinear tracking kernel takes float64 points, got {}".format(pts.dtype))
    nat.check(_lib().ofl_track_bilinear_dev(flows_ptr, n_fields, shape[0], shape[1], 1 if chain else 0, pts.buf.ptr, pts.n,
                                            _ptr(stats), _ptr(valid), int(bool(int_out)), out.ptr, _ptr(status),
                                            _ptr(outside), _ptr(lost_at), _ptr(path), stream))


def track_query_points(pts, stream=None):
    """DevicePoints (row, col) -> DeviceBuffer of float64 (x, y) queries for the scatter kernel; asynchronous."""
    query = DeviceBuffer(pts.n * 16)
    nat.check(_lib().ofl_track_query_points_dev(pts.buf.ptr, _TRACK_DT[pts.dtype], pts.n, query.ptr, stream))
    return query


def scatter_query_resident(pos_flow_buf, sign, vals_buf, h, w, query, n):
    """scatter_query with the queries already on the device, and the answers left there: (values float64 [n][2] as (u, v),
    found uint8 [n]) DeviceBuffers."""
    vals, found = DeviceBuffer(n * 16), DeviceBuffer(n)
    ws = _workspace(h, w, 2)
    nat.check(_lib().ofl_scatter_query_dev(pos_flow_buf.ptr, sign, 0, None, vals_buf.ptr, 2, h, w, query.ptr, n, vals.ptr,
                                           found.ptr, ws.ptr, ws.nbytes, None))
    return vals, found


def track_query_epilogue(query, vals, found, n, shape, stats, valid, step, status, out_rc=None, out_int=None, next_query=None,
                         lost_at=None, stream=None):
    """K10 tail of the query paths (ofl_track_query_epilogue_dev); asynchronous."""
    nat.check(_lib().ofl_track_query_epilogue_dev(query.ptr, vals.ptr, found.ptr, n, shape[0], shape[1], _ptr(stats), _ptr(valid),
                                                  step, _ptr(out_rc), _ptr(out_int), _ptr(next_query), _ptr(status),
                                                  _ptr(lost_at), stream))


# ------------------------------------------------------------------------------ K11: exchange with other frameworks
# Ingress and egress over the CUDA Array Interface (ROCm frameworks expose it under that name).  The package imports no
# framework: it reads and writes a dict of integers.
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
    mptr = mext.ptr if mext is not None else _ptr(mbuf)
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
        return DeviceArray(vecs, out_shape, '<f4', owner=owner)
    itemsize = 4 if name == 'float32' else 2
    dst = DeviceBuffer(n * h * w * 2 * itemsize)
    nat.check(_lib().ofl_export_flow_dev(vecs.ptr, n, h, w, _EL_CODE[name], 1 if layout == 'chw' else 0, dst.ptr, None))
    return DeviceArray(dst, out_shape, _EL_TYPESTR[name])


def export_mask(mask, shape, copy, owner):
    """uint8 0 / 1 masks -> DeviceArray of bool with `shape`: a device copy, or a view of the mask's own memory."""
    if not copy:
        return DeviceArray(mask, shape, '|b1', owner=owner)
    nbytes = int(np.prod(shape))
    dst = DeviceBuffer(nbytes)
    nat.check(_lib().ofl_copy_dev(dst.ptr, mask.ptr, nbytes, None))
    return DeviceArray(dst, shape, '|b1')
