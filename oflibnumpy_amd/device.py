"""HBM-resident flow fields and the device-side flow algebra.

`DeviceFlow` mirrors the hot-path methods of the reference's `Flow` (apply / switch_ref / invert /
combine_with / valid_target / valid_source / + - neg / is_zero / visualise, and the constructors zero / from_matrix /
from_transforms, * / by a factor, pad and slicing; src/oflibnumpy/flow_class.py) but
keeps vectors and mask in GPU memory between operations, so chains such as combine_with(mode=1)
(1 scatter + 2 gathers, flow_class.py:1369-1370) never cross PCIe.  The host `Flow` class is a thin
upload -> DeviceFlow op -> download wrapper around this module.

This module holds the four resident classes and the .flo I/O, and it is the public namespace of the whole resident layer:
what the classes are built from is imported below and stays reachable as `device.X`.  It lives in memory.py (the HBM
recycling pool, DeviceBuffer, views, the pinned-host pool), args.py (host-only argument checks and tables), kernels.py
(launch wrappers of the gather, compose, statistics, visualise, fit, build and tracking kernels), scatter.py (the scatter
kernel: workspace cache, walk check, the multi-rank slab protocol) and interop.py (the CUDA Array Interface).

This layer is SINGLE-STREAM: recycled buffers (`_Pool`) and the one scatter workspace per shape are handed out as soon
as Python drops them, which is only safe while all work is queued on one stream (the library's default).  The `stream`
arguments exist for callers that manage their own buffers at the C level.

Data layout in HBM: vecs float32 [H][W][2] interleaved (x, y) -- the same layout as the reference,
so a pixel's vector is one 8-byte element and two horizontally adjacent bilinear taps are one
16-byte load; mask uint8 [H][W] (0/1).
"""
import ctypes

import numpy as np

from . import _native as nat
from .memory import (_lib, _ptr, _size_query, _Pool, _PinnedPool, empty_cache, DeviceBuffer, _BufferView, _download,
                     PinnedArray, sync)
from .args import (DEFAULT_THRESHOLD, _DT_CODE, _TRACK_DT, _PAD_MODES, remap_rules, mask_bytes, _points_array, visualise_args,
                   percentile_ranks, matrix_args, validate_transforms, valid_mask_array, scale_operand, crop_args,
                   resize_scales, resized_shape, tensor_dtype, tensor_args, tensor_mem_shape, tensor_logical_shape,
                   consistency_args, error_args, fill_args, median_args, upsample_args, upsample_weights_array, corr_args,
                   corr_host_array, optional_bool, mask_array_arg, match_args, match_host_array, splat_args, splat_host_array,
                   splat_importance_array, photometric_args, photometric_host_array, census_args, ssim_args, refine_args,
                   inverse_search_args, inverse_search_channels, estimate_levels, pair_channels, pair_host_arrays,
                   sequence_args, SEQUENCE_PREFIX)
from .kernels import (gather_bilinear_batch, gather_valid_only, flow_stats, stats_word_launch, compose3_launch,
                      compose3_bits_launch, mask_bits_bytes, mask_pack, mask_unpack, visualise_range_launch, FitField,
                      flow_from_matrix_launch, _valid_mask, _mask_buffer, _mask_and, resize_host, grid_minus, sample_points,
                      track_bilinear_launch, track_query_points, track_query_epilogue, gather_tensor, tensor_import_launch,
                      tensor_permute_launch, consistency_launch, consistency_host, error_launch, error_host, ERROR_RECORD,
                      FlowErrorStats, fill_launch, fill_host, median_launch, median_host, upsample_launch,
                      upsample_host, avgpool2_launch, corr_lookup_launch, corr_lookup_host, match_launch, match_host, splat_launch, splat_host,
                      photometric_launch, photometric_host, census_launch, census_host, ssim_launch, ssim_host,
                      refine_launch, refine_host, tensor_halve_launch, inverse_search_launch, inverse_search_host,
                      sequence_launch, sequence_host)
from .scatter import (_workspace, walk_check, scatter_linear, scatter_linear_f64, scatter_rows, SLAB_LIST_HEAD, SLAB_RECORD,
                      SLAB_ERR_LIST, slab_list_bytes, comm_allgather, scatter_slab_stars, scatter_slab_finish, _slab_timeout,
                      scatter_slab, scatter_host, scatter_query, scatter_query_resident)
from .interop import (External, external_args, flow_layout, image_layout, _contiguous, _check_device_memory, _wait_for,
                      import_flow_launch, import_flow, DeviceArray, export_buffer, export_flow, export_mask)
from .sharding import row_band
from . import matrix_fit


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
        if layout == 'hwc':
            return export_buffer(self.buf, self.shape, self.dtype.str, copy, self)
        if not copy:
            raise ValueError("Error exporting image: copy=False hands out the image's own (H, W, C) memory; 'chw' is a conversion")
        if len(self.shape) != 3 or not 1 <= self.shape[2] <= 6:
            raise ValueError("Error exporting image: 'chw' takes one (H, W, C) image with C in 1..6, got shape {}".format(self.shape))
        h, w, c = self.shape
        buf = DeviceBuffer(h * w * c * self.dtype.itemsize)
        nat.check(_lib().ofl_permute_image_dev(self.buf.ptr, buf.ptr, self.dtype.itemsize, c, h, w, h * w, w, 1, 0, None))
        return DeviceArray(buf, (c, h, w), self.dtype.str)


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
        return export_buffer(self.buf, self.shape, self.dtype.str, copy, self)


_TENSOR_NP = {'float32': np.dtype('<f4'), 'float16': np.dtype('<f2'), 'bfloat16': np.dtype('<u2')}     # what to_host hands back
_TENSOR_TYPESTR = {'float32': '<f4', 'float16': '<f2', 'bfloat16': '<i2'}                               # what export hands out


class DeviceTensor:
    """A many-channel float warp target in HBM -- a network's feature maps: `shape` is the logical (C, H, W) or (N, C, H, W),
    `layout` the memory order, 'chw' (planar, [N][C][H][W]) or 'hwc' (channels last, [N][H][W][C]), `dtype` 'float32',
    'float16' or 'bfloat16'.  Warped by DeviceFlow.apply_tensor and DeviceFlowBatch.apply_tensors (K12)."""

    def __init__(self, buf, shape, dtype, layout):
        self.n, self.channels, self.h, self.w, self.batched = tensor_args(shape, layout, dtype)
        self.buf, self.shape, self.dtype, self.layout = buf, tuple(int(v) for v in shape), dtype, layout

    @property
    def itemsize(self):
        return 4 if self.dtype == 'float32' else 2

    @property
    def nbytes(self):
        return self.n * self.channels * self.h * self.w * self.itemsize

    @classmethod
    def from_host(cls, arr, layout='chw', dtype=None):
        """A host array in the memory order of `layout` -- (C, H, W) / (N, C, H, W) for 'chw', (H, W, C) / (N, H, W, C) for
        'hwc' -- of float32 or float16, or a 2-byte integer array with dtype='bfloat16'."""
        arr = np.asarray(arr)
        shape = tensor_logical_shape(arr.shape, layout)
        name = tensor_dtype(arr.dtype, dtype)
        tensor_args(shape, layout, name)
        return cls(DeviceBuffer.from_host(np.ascontiguousarray(arr)), shape, name, layout)

    def to_host(self):
        """-> the array in memory order; bfloat16 comes back as uint16 bit patterns."""
        return self.buf.to_host(tensor_mem_shape(self.shape, self.layout), _TENSOR_NP[self.dtype])

    @classmethod
    def from_external(cls, obj, layout=None, dtype=None, stream=None, copy=True):
        """A tensor another framework holds in device memory (`obj.__cuda_array_interface__`, see external_args), in the
        memory order of `layout` ('chw', also the default: (C, H, W) / (N, C, H, W); 'hwc': (H, W, C) / (N, H, W, C)), of
        float32 or float16 -- or bfloat16, handed over as a 2-byte integer array with dtype='bfloat16'.  A contiguous source
        is one device copy -- or, with copy=False, adopted: the DeviceTensor then IS the producer's memory, its buffer view
        keeps `obj` alive and must not be written by the producer afterwards.  A strided source (a channel slice, a crop)
        goes through the import kernel; copy=False is then a ValueError.  The library's stream first waits for the
        producer's (`stream`: see external_args).  Asynchronous, like DeviceImage.from_external."""
        layout = 'chw' if layout is None else layout
        ext = external_args(obj, dtype, stream)
        shape = tensor_logical_shape(ext.shape, layout)
        name = tensor_dtype(ext.dtype)
        n, c, h, w, batched = tensor_args(shape, layout, name)
        contiguous = _contiguous(ext.shape, ext.strides)
        if not copy and not contiguous:
            raise ValueError("Error taking an external tensor: copy=False needs a C-contiguous array in the layout '{}'".format(layout))
        _check_device_memory(ext)
        _wait_for(ext.stream)
        nbytes = n * c * h * w * ext.itemsize
        if contiguous and not copy:
            return cls(_BufferView(ext.ptr, nbytes, owner=obj), shape, name, layout)
        if contiguous:
            buf = DeviceBuffer(nbytes)
            nat.check(_lib().ofl_copy_dev(buf.ptr, ext.ptr, nbytes, None))
        else:
            st = ext.strides if batched else (0,) + ext.strides
            st = st if layout == 'chw' else (st[0], st[3], st[1], st[2])        # -> (item, channel, row, column)
            buf = tensor_import_launch(ext.ptr, name, st, layout, n, c, h, w)
        return cls(buf, shape, name, layout)

    def export(self, layout=None, copy=True):
        """-> DeviceArray (`__cuda_array_interface__`; torch.as_tensor(a, device='cuda')) in the memory order of `layout`
        (None: the tensor's own).  bfloat16 goes out as int16 ('<i2'), like DeviceFlow.export.  The tensor's own layout is a
        device copy or, with copy=False, a view of its memory that the consumer must not write; the other layout goes
        through the permute kernel."""
        layout = self.layout if layout is None else layout
        if layout not in ('chw', 'hwc'):
            raise ValueError("Error exporting tensor: layout must be 'chw' or 'hwc', got {!r}".format(layout))
        out_shape = tensor_mem_shape(self.shape, layout)
        if layout == self.layout:
            return export_buffer(self.buf, out_shape, _TENSOR_TYPESTR[self.dtype], copy, self)
        if not copy:
            raise ValueError("Error exporting tensor: copy=False hands out the tensor's own '{}' memory; '{}' is a conversion"
                             .format(self.layout, layout))
        buf = tensor_permute_launch(self.buf, self.dtype, self.n, self.channels, self.h, self.w, layout == 'hwc')
        return DeviceArray(buf, out_shape, _TENSOR_TYPESTR[self.dtype])

    def halve(self):
        """The next level of an image pyramid: the 2 x 2 mean ((tl + tr) + (bl + br)) * 0.25 of every channel, in float32,
        rounded once to the dtype (ofl_tensor_halve_dev; K18's avgpool arithmetic) -> a DeviceTensor of shape
        (..., H // 2, W // 2) in the same layout and dtype.  An odd last row or column is dropped; H or W below 2 is a
        ValueError.  Asynchronous."""
        if self.h < 2 or self.w < 2:
            raise ValueError("Error halving tensor: a {} x {} tensor has no 2 x 2 mean".format(self.h, self.w))
        buf = tensor_halve_launch(self.buf, self.dtype, self.layout, self.n, self.channels, self.h, self.w)
        return DeviceTensor(buf, self.shape[:-2] + (self.h >> 1, self.w >> 1), self.dtype, self.layout)

    def correlation(self, other, flow=None, radius=4, levels=1, scale=None, order='xy', quant=nat.QUANT_EXACT):
        """The correlation of this tensor's features with those of `other` around every pixel, in one call:
        DeviceCorrelation.build(self, other, levels).lookup(flow, radius, scale, order, quant) (correlation.py, K18).  With
        levels = 1 and flow = None on a tensor that DeviceFlow.apply_tensor has warped this is the cost volume of PWC-Net.
        -> a planar float32 DeviceTensor of levels (2 radius + 1)^2 channels."""
        from .correlation import DeviceCorrelation
        return DeviceCorrelation.build(self, other, levels).lookup(flow, radius, scale, order, quant)

    def match(self, other, ref='s', scale=None, reverse=False, min_confidence=None, return_confidence=False, return_index=False):
        """The global match of this tensor's features in those of `other`, in one call:
        DeviceCorrelation.build(self, other, levels=1).match(...) (correlation.py, K19)."""
        from .correlation import DeviceCorrelation
        return DeviceCorrelation.build(self, other, 1).match(ref, scale, reverse, min_confidence, return_confidence, return_index)


# ------------------------------------------------------------------------------ the launch wrappers that hand back a DeviceImage
def gather_bilinear(src, flow_buf, flow_shape, sign, smask=None, fmask=None, want_valid=False,
                    pad=(0, 0), quant=nat.QUANT_OPENCV, arith=nat.ARITH_NATIVE, rule=nat.RULE_EQ1,
                    stream=None):
    """K1: dst = B(src; x + sign*flow) (+ validity).  Replaces apply_flow 't', utils.py:231-236."""
    H, W, C = src.shape
    dst = DeviceImage(DeviceBuffer(H * W * C * src.dtype.itemsize), src.shape, src.dtype)
    valid = DeviceBuffer(H * W) if want_valid else None
    nat.check(_lib().ofl_gather_bilinear_dev(
        src.buf.ptr, _DT_CODE[src.dtype], C, H, W, flow_buf.ptr, flow_shape[0], flow_shape[1],
        pad[0], pad[1], sign, _ptr(smask), _ptr(fmask), dst.buf.ptr, _ptr(valid), quant, arith, rule, stream))
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
        _ptr(smask), _ptr(fmask_rows), dst.buf.ptr, _ptr(valid), quant, arith, rule, stream))
    return dst, valid


def visualise_launch(vecs, mask, h, w, batch, mode, flags, range_buf=None, range_const=None, stream=None):
    """K7 render of `batch` fields -> DeviceImage uint8 (batch, H, W, 3), or (H, W, 3) for batch 1.  The scale comes from
    range_buf (float32[batch] on the device) or, if that is None, from range_const.  Asynchronous."""
    shape = (h, w, 3) if batch == 1 else (batch, h, w, 3)
    img = DeviceImage(DeviceBuffer(batch * h * w * 3), shape, np.uint8)
    nat.check(_lib().ofl_visualise_dev(vecs.ptr, _ptr(mask) if flags else None, h, w, batch, np.float32(DEFAULT_THRESHOLD),
                                       _ptr(range_buf), np.float32(1.0 if range_const is None else range_const), mode, flags,
                                       img.buf.ptr, stream))
    return img


# ------------------------------------------------------------------------------ DevicePoints' argument check, DeviceFlow
def track_args(pts, int_out=None, get_valid_status=None, s_exact_mode=None):
    """Validation of Flow.track's arguments (flow_class.py:781-784, utils.py:571-582) with the reference's defaults and
    exception types, on the host before any device work -> (int_out, get_valid_status, s_exact_mode).  `pts`: a
    DevicePoints or an (n, 2) array of a dtype DevicePoints.from_host takes."""
    if not isinstance(pts, DevicePoints):
        _points_array(pts)
    int_out = optional_bool(int_out, False, "Error tracking points: Int_out needs to be a boolean")
    get_valid_status = optional_bool(get_valid_status, False, "Error tracking points: Get_tracked needs to be a boolean")
    s_exact_mode = optional_bool(s_exact_mode, False, "Error tracking points: S_exact_mode needs to be a boolean")
    return int_out, get_valid_status, s_exact_mode


_STATS_KNOW_MASK = 1 << 30        # private flag in DeviceFlow._stats: STAT_MASK_HAS_ZERO has been evaluated


class DeviceFlowError:
    """The result of DeviceFlow.error / DeviceFlowBatch.error while it is still on the device: `records` (96 bytes per
    pair, struct ofl_flow_error), and the optional `epe_map` / `outlier_map` DeviceBuffers ([n][H][W] for a batch).
    `read()` is the one read-back: a FlowErrorStats, or a list of n of them for a batch."""

    def __init__(self, records, n, n_thresholds, n_edges, epe_map=None, outlier_map=None):
        self.records, self.n, self.epe_map, self.outlier_map = records, n, epe_map, outlier_map
        self._n_thresholds, self._n_edges = n_thresholds, n_edges

    def read_records(self):
        """the raw records as a NumPy array of kernels.ERROR_RECORD, one per pair (synchronises)"""
        return self.records.to_host((1 if self.n is None else self.n,), ERROR_RECORD)

    def read(self):
        stats = [FlowErrorStats(r, self._n_thresholds, self._n_edges) for r in self.read_records()]
        return stats[0] if self.n is None else stats


def mask_buffer_arg(buf, n_bytes, prefix, name):
    """A device mask argument `name` (the `valid` of DeviceFlow.fill / DeviceFlowBatch.fill, the `valid` or `only` of their
    median): None, or a uint8 buffer (DeviceBuffer or a view) of at least n_bytes bytes -- e.g. `consistent` out of a
    consistency check.  `prefix` opens the message, e.g. "Error filling flow: "."""
    if buf is not None and not isinstance(buf, (DeviceBuffer, _BufferView)):
        raise TypeError("{}{} needs to be a DeviceBuffer of uint8 or None, got {}".format(prefix, name, type(buf).__name__))
    if buf is not None and buf.nbytes < n_bytes:
        raise ValueError("{}{} needs to hold {} bytes, got {}".format(prefix, name, n_bytes, buf.nbytes))
    return buf


def splat_importance(buf, n_px):
    """The `importance` of the splat methods: None, or a float32 buffer (DeviceBuffer or a view) of at least n_px values."""
    if buf is not None and not isinstance(buf, (DeviceBuffer, _BufferView)):
        raise TypeError("Error splatting: importance needs to be a DeviceBuffer of float32 or None, got {}".format(type(buf).__name__))
    if buf is not None and buf.nbytes < 4 * n_px:
        raise ValueError("Error splatting: importance needs to hold {} bytes, got {}".format(4 * n_px, buf.nbytes))
    return buf


def photometric_tensors(near, far, field_shape, batch=None, prefix="Error computing photometric error: ", max_c=None, one_item=False):
    """The `near` and `far` of DeviceFlow.photometric (batch None) or DeviceFlowBatch.photometric (batch n) -> two
    DeviceTensors of one shape, layout and dtype with the height and width of the field, at most max_c channels (None: any
    count) and -- one_item -- a single item.  A float32 DeviceImage [H][W][C] is taken as the channels-last tensor it is, on
    the same buffer.  `prefix` starts the messages (census, refine and inverse_search pass their own)."""
    pair = []
    for name, t in (("near", near), ("far", far)):
        if isinstance(t, DeviceImage):
            if t.dtype != np.float32:
                raise TypeError("{}{} as a DeviceImage needs to be float32, got {}".format(prefix, name, t.dtype))
            t = DeviceTensor(t.buf, (t.shape[2], t.shape[0], t.shape[1]), 'float32', 'hwc')
        if not isinstance(t, DeviceTensor):
            raise TypeError("{}{} needs to be a DeviceTensor or a float32 DeviceImage, got {}".format(prefix, name, type(t).__name__))
        pair.append(t)
    near, far = pair
    if near.shape != far.shape:
        raise ValueError("{}the tensors need the same shape, got {} and {}".format(prefix, near.shape, far.shape))
    if near.dtype != far.dtype:
        raise TypeError("{}the tensors need the same dtype, got {} and {}".format(prefix, near.dtype, far.dtype))
    if near.layout != far.layout:
        raise ValueError("{}the tensors need the same layout, got '{}' and '{}'".format(prefix, near.layout, far.layout))
    if (near.h, near.w) != tuple(field_shape):
        raise ValueError("{}tensors and flow need the same height and width, got {} and {}"
                         .format(prefix, (near.h, near.w), tuple(field_shape)))
    if batch is not None and (not near.batched or near.n != batch):
        raise ValueError("{}a batch of {} fields takes tensors of shape ({}, C, H, W), got {}".format(prefix, batch, batch, near.shape))
    if max_c is not None:
        pair_channels(near.channels, max_c, prefix)
    if one_item and near.n != 1:
        raise ValueError("{}one field takes tensors of shape (C, H, W) or (1, C, H, W), got {}".format(prefix, near.shape))
    return near, far


# One body per operation of the image-pair families K21 ... K24 for DeviceFlow (batch None: ONE field and one of each mask
# serve every item of the tensors, or -- refine, inverse_search -- the tensors hold one item) and DeviceFlowBatch (batch n: item
# i with field i and masks i).  vecs, mask: the buffers of the field(s) of `shape` and reference `ref`; settings: what the
# family's args.*_args returned.  They return the buffers of the launch wrapper; the two classes shape their own results.
def error_map_op(launch, settings, max_c, prefix, vecs, mask, shape, ref, near, far, near_mask, far_mask, return_counts, quant,
                 batch=None):
    """photometric (launch photometric_launch, max_c None), census (census_launch, 4) and ssim (ssim_launch, 4) -> ((err,
    covered[, within]), the counts buffer or None, the number of items)"""
    near, far = photometric_tensors(near, far, shape, batch, prefix, max_c)
    n_bytes = (batch or 1) * shape[0] * shape[1]
    near_mask = mask_buffer_arg(near_mask, n_bytes, prefix, "near_mask")
    far_mask = mask_buffer_arg(far_mask, n_bytes, prefix, "far_mask")
    err, covered, within, counts = launch(
        near.buf, far.buf, near.dtype, near.layout, near.n, near.channels, shape, vecs, mask, batch is None,
        1 if ref == 's' else -1, *settings, near_mask=near_mask, far_mask=far_mask, want_counts=bool(return_counts), quant=quant)
    return (err, covered) + ((within,) if within is not None else ()), counts, near.n


def refine_op(settings, vecs, mask, shape, ref, near, far, near_mask, far_mask, valid, return_data, quant, batch=None):
    """refine -> (vecs, data or None)"""
    prefix = "Error refining flow: "
    near, far = photometric_tensors(near, far, shape, batch, prefix, nat.REFINE_MAX_C, one_item=batch is None)
    n_bytes = (batch or 1) * shape[0] * shape[1]
    near_mask = mask_buffer_arg(near_mask, n_bytes, prefix, "near_mask")
    far_mask = mask_buffer_arg(far_mask, n_bytes, prefix, "far_mask")
    valid = mask_buffer_arg(valid, n_bytes, prefix, "valid")
    return refine_launch(near.buf, far.buf, near.dtype, near.layout, near.n, near.channels, shape, vecs, mask,
                         1 if ref == 's' else -1, *settings, near_mask=near_mask, far_mask=far_mask, valid=valid,
                         want_data=bool(return_data), quant=quant)


def inverse_search_op(settings, vecs, mask, shape, ref, near, far, return_patches, quant, batch=None):
    """inverse_search -> (vecs, mask, patch_vecs or None, patch_ssd or None, (ny, nx))"""
    prefix = "Error searching flow: "
    near, far = photometric_tensors(near, far, shape, batch, prefix, nat.ISEARCH_MAX_C, one_item=batch is None)
    if min(shape) < settings[0]:
        raise ValueError("{}a {} x {} field holds no patch of {}".format(prefix, shape[0], shape[1], settings[0]))
    return inverse_search_launch(near.buf, far.buf, near.dtype, near.layout, near.n, near.channels, shape, vecs, mask,
                                 1 if ref == 's' else -1, *settings, want_patches=bool(return_patches), quant=quant)


def upsample_weights(weights, factor, shape, batch=None):
    """The `weights` of DeviceFlow.upsample_convex (batch None: logical shape (9 f^2, h, w)) or
    DeviceFlowBatch.upsample_convex (batch n: (n, 9 f^2, h, w)) checked against the coarse field's `shape` -> factor."""
    if not isinstance(weights, DeviceTensor):
        raise TypeError("Error upsampling flow: weights need to be a DeviceTensor, got {}".format(type(weights).__name__))
    factor = upsample_args(factor, weights.shape, shape)
    if batch is None and weights.batched:
        raise ValueError("Error upsampling flow: one field takes weights of shape (C, h, w), got {}".format(weights.shape))
    if batch is not None and (not weights.batched or weights.n != batch):
        raise ValueError("Error upsampling flow: a batch of {} fields takes weights of shape ({}, C, h, w), got {}"
                         .format(batch, batch, weights.shape))
    return factor


def mask_distance(mask_buf, shape, batch=1, max_dist=None):
    """The distance transform of `batch` uint8 masks [batch][H][W] in HBM (K15 without vectors, include/ofl.h): -> (index,
    d2) as DeviceBuffers, int32 [batch][H][W] = the linear index qy * W + qx of the nearest non-zero pixel of the same mask
    (among equals the smallest index), -1 where there is none within max_dist, and uint32 [batch][H][W] = its squared
    distance, 0xFFFFFFFF where there is none.  Exact integers; asynchronous."""
    max_d2 = fill_args(max_dist)
    shape = (int(shape[0]), int(shape[1]))
    if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
        raise ValueError("Error filling flow: batch must be a positive integer, got {}".format(batch))
    if not isinstance(mask_buf, (DeviceBuffer, _BufferView)):
        raise TypeError("Error filling flow: mask needs to be a DeviceBuffer of uint8, got {}".format(type(mask_buf).__name__))
    if shape[0] < 1 or shape[1] < 1 or mask_buf.nbytes < batch * shape[0] * shape[1]:
        raise ValueError("Error filling flow: mask needs to hold batch * H * W = {} bytes, got {}"
                         .format(batch * shape[0] * shape[1], mask_buf.nbytes))
    _, _, index, d2 = fill_launch(None, mask_buf, None, shape, max_d2, batch=int(batch), want_mask=False, want_index=True, want_d2=True)
    return index, d2


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
        m = np.ones((h, w), np.uint8) if mask is None else mask_bytes(mask)
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
            bits = DeviceBuffer(_size_query(_lib().ofl_scatter_diag_bytes, h, w))      # the cells' Delaunay diagonals, read by the walk kernel; lives with the certificate
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
        ov, om = (other.vecs.ptr, other.mask.ptr) if other is not None else (None, None)
        nat.check(_lib().ofl_axpy_dev(self.vecs.ptr, self.mask.ptr, ov, om, np.float32(alpha), self.n_px, out.vecs.ptr,
                                      out.mask.ptr, None))
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

    def consistency(self, backward, alpha=None, beta=None, return_residual=False, return_counts=False, quant=nat.QUANT_OPENCV):
        """The forward-backward check of this (forward) field against `backward`, a DeviceFlow of the same shape and the SAME
        reference, in ONE launch of K13 (include/ofl.h): the backward field is sampled where this one points -- at
        x + self for 's', x - self for 't', the taps and blend of the compose kernel -- and per pixel
            covered    = self.mask & [the interpolated backward mask == 1]      (the mask of self + sampled backward)
            consistent = covered & (|self + sampled|^2 <= alpha * (|self|^2 + |sampled|^2) + beta)
            residual   = |self + sampled| where covered, else 0
        in float32 with one rounding per operation.  alpha, beta: None for the usual 0.01 and 0.5 (args.consistency_args).
        This is not a function of the reference and the formula is its definition: there is NO zero-flow short cut in either
        `quant` mode, so under QUANT_EXACT a field below the 1e-3 threshold differs from self + self.apply(backward), while
        covered and the residual's vector equal the fused compose kernel's result always, bit for bit.
        -> (consistent, covered) as uint8 DeviceBuffers [H][W]; return_residual appends the float32 DeviceBuffer [H][W],
        return_counts appends (n_covered, n_consistent) as Python ints -- the only option that synchronises; everything else is
        asynchronous.  The inputs are not modified."""
        alpha, beta = consistency_args(alpha, beta)
        if not isinstance(backward, DeviceFlow):
            raise TypeError("Error checking flow consistency: backward needs to be a DeviceFlow, got {}".format(type(backward).__name__))
        if backward.shape != self.shape:
            raise ValueError("Error checking flow consistency: the fields need the same shape, got {} and {}".format(self.shape, backward.shape))
        if backward.ref != self.ref:
            raise ValueError("Error checking flow consistency: the fields need the same reference, got '{}' and '{}'"
                             .format(self.ref, backward.ref))
        consistent, covered, residual, counts = consistency_launch(
            self.vecs, self.mask, backward.vecs, backward.mask, 1 if self.ref == 's' else -1, self.shape, alpha, beta,
            want_residual=return_residual, want_counts=return_counts, quant=quant)
        res = (consistent, covered) + ((residual,) if return_residual else ())
        if return_counts:
            n = counts.to_host((2,), np.uint32)
            res += ((int(n[0]), int(n[1])),)
        return res

    def photometric(self, near, far, metric='l1', eps=None, threshold=None, near_mask=None, far_mask=None, return_counts=False,
                    quant=nat.QUANT_OPENCV):
        """The photometric (brightness- or feature-constancy) error of this field in ONE launch of K21 (include/ofl.h):
        `near`, the tensor of the field's own frame, against `far`, the tensor of the other frame, sampled where this field
        points -- at x + self for 's', x - self for 't', the taps and blend of apply_tensor -- and reduced over the channels:
            covered = self.mask & near_mask & [the interpolated far_mask == 1]      (apply_tensor's valid, ANDed with near_mask)
            error   = mean_c |near_c - warped far_c| ('l1'), its root mean square ('l2') or mean_c sqrt(d_c^2 + eps^2)
                      ('charbonnier'; eps None: 1e-3) where covered, else 0
        in float32 with one rounding per operation and a summation order that depends on the channel count alone, so both
        layouts give the same bytes.  near, far: DeviceTensors of one shape (C, H, W) or (N, C, H, W), one layout and one
        dtype (float32 / float16 / bfloat16); a float32 DeviceImage is taken as an 'hwc' tensor without a copy.  near_mask,
        far_mask: uint8 DeviceBuffers [H][W] or None.  This one field and these masks serve every item.  Not a function of
        the reference and without a zero-flow short cut in either `quant` mode; works for 's' and 't' fields alike, where
        apply_tensor takes 't' only.
        -> (error, covered): a float32 and a uint8 DeviceBuffer [N][H][W]; `threshold` appends within = covered &
        (error <= threshold) as uint8, return_counts appends [(n_covered, n_within)] * N as Python ints -- the only option
        that synchronises.  `error` is what splat(mode='softmax', importance=error, alpha=-20.0) takes, without a copy.
        Not built: the window metric gradient constancy (the census distance is `census`, SSIM is `ssim`), a mean or percentiles
        of the map, a backward pass, mixed dtypes or layouts, integer tensors, padding offsets.  The inputs are not modified."""
        res, counts, n = error_map_op(photometric_launch, photometric_args(metric, eps, threshold), None,
                                      "Error computing photometric error: ", self.vecs, self.mask, self.shape, self.ref,
                                      near, far, near_mask, far_mask, return_counts, quant)
        return res + ([(int(a), int(b)) for a, b in counts.to_host((n, 2), np.uint32)],) if return_counts else res

    def census(self, near, far, window=7, mode='soft', delta=None, noise=None, knee=None, min_count=None, threshold=None,
               near_mask=None, far_mask=None, return_counts=False, quant=nat.QUANT_OPENCV):
        """The census distance of this field in ONE launch of K22 (include/ofl.h): where photometric compares the values of
        `near` and of `far` sampled where this field points, census compares the ORDER of the intensities -- the channel
        means A of `near` and B of the warped `far` -- in a window x window neighbourhood of the pixel, so a change of
        exposure or gain that keeps the order costs nothing.  Per neighbour d: a = A(p + d) - A(p), b = B(p + d) - B(p) and
            'hard'  1 where sign(a) != sign(b), each sign 0 inside the dead zone |v| <= delta (None: 0)
            'soft'  q / (knee + q) of q = (rho(a) - rho(b))^2, rho(v) = v / sqrt(noise + v^2) -- the ternary census of
                    unsupervised flow; noise None: 0.81, knee None: 0.1, both meant for intensities 0 ... 255
        averaged over the neighbours that are inside the frame and covered as photometric defines it; a pixel is covered
        when photometric covers it and at least min_count neighbours (None: all window^2 - 1, the usual border mask) are.
        near, far, near_mask, far_mask, quant: as in photometric, with 1 to 4 channels.  Not a function of the reference and
        without a zero-flow short cut; works for 's' and 't' fields alike.
        -> (error, covered): a float32 and a uint8 DeviceBuffer [N][H][W]; `threshold` appends within = covered &
        (error <= threshold) as uint8, return_counts appends [(n_covered, n_within)] * N as Python ints -- the only option
        that synchronises.  Not built: more than 4 channels, a per-channel census, luma weights, gradient constancy,
        other windows, a mean of the map, a backward pass.  The inputs are not modified."""
        res, counts, n = error_map_op(census_launch, census_args(window, mode, delta, noise, knee, min_count, threshold),
                                      nat.CENSUS_MAX_C, "Error computing census distance: ", self.vecs, self.mask, self.shape,
                                      self.ref, near, far, near_mask, far_mask, return_counts, quant)
        return res + ([(int(a), int(b)) for a, b in counts.to_host((n, 2), np.uint32)],) if return_counts else res

    def ssim(self, near, far, window=11, weights='gaussian', sigma=None, data_range=255.0, k1=0.01, k2=0.03, min_count=None,
             threshold=None, near_mask=None, far_mask=None, return_counts=False, quant=nat.QUANT_OPENCV):
        """The structural dissimilarity of this field in ONE launch of K26 (include/ofl.h): the local means, variances and
        the covariance of the intensities -- the channel means A of `near` and B of `far` sampled where this field points
        -- in a weighted window x window neighbourhood of the pixel (3, 5, 7 or 11), compared as Wang et al.'s SSIM:
            SSIM  = (2 mu_a mu_b + c1) (2 cov_ab + c2) / ((mu_a^2 + mu_b^2 + c1) (var_a + var_b + c2))
            error = clamp((1 - SSIM) / 2, 0, 1)          so SSIM = 1 - 2 error
        with c1 = (k1 data_range)^2, c2 = (k2 data_range)^2 and population moments.  weights: 'gaussian' (`sigma` None: 1.5;
        the defaults are Wang's 11 x 11 window for intensities 0 ... 255) or 'uniform' (the avg_pool2d form of the SSIM term
        in unsupervised flow; `sigma` stays None).  The window holds the pixels that are inside the frame and covered as
        photometric defines it, the centre among them, and is renormalised to them; a pixel is covered when photometric
        covers it and its window has at least min_count such pixels (None: all window^2, the usual border mask).  Every
        operation is float32; the raw second moments cost 1e-5 to 1e-4 of the error against float64 at intensities 0 ... 255.
        near, far, near_mask, far_mask, quant: as in photometric, with 1 to 4 channels.  Not a function of the reference and
        without a zero-flow short cut; works for 's' and 't' fields alike.
        -> (error, covered): a float32 and a uint8 DeviceBuffer [N][H][W]; `threshold` appends within = covered &
        (error <= threshold) as uint8, return_counts appends [(n_covered, n_within)] * N as Python ints -- the only option
        that synchronises.  `error` feeds splat(importance=) as photometric's does.  Not built: more than 4 channels, a
        per-channel SSIM, luma weights, sample (N - 1) moments, other windows, MS-SSIM, the three components, gradient
        constancy, a mean of the map, PSNR, a backward pass.  The inputs are not modified."""
        res, counts, n = error_map_op(ssim_launch, ssim_args(window, weights, sigma, data_range, k1, k2, min_count, threshold),
                                      nat.SSIM_MAX_C, "Error computing structural similarity: ", self.vecs, self.mask, self.shape,
                                      self.ref, near, far, near_mask, far_mask, return_counts, quant)
        return res + ([(int(a), int(b)) for a, b in counts.to_host((n, 2), np.uint32)],) if return_counts else res

    def refine(self, near, far, alpha=None, delta=None, zeta=None, eps=None, fixed_point=None, sor=None, omega=None,
               near_mask=None, far_mask=None, valid=None, return_data=False, quant=nat.QUANT_OPENCV):
        """This field moved a fraction of a pixel towards where the two images say it belongs: the variational refinement
        of Brox et al. without the gradient-constancy term (K23, include/ofl.h), the step that classical pipelines put
        after matching, `fill` and `median`.  `far` is warped once where this field points (photometric's taps, blend and
        `covered`; channel means as in census) and the increment d of
            sum data * (delta / n) * psi(r^2 / n) + alpha * sum psi(|grad(u + du)|^2 + |grad(v + dv)|^2),  psi(s^2) = sqrt(s^2 + eps^2)
        with r = Iz + gx du + gy dv, n = gx^2 + gy^2 + zeta^2, is found by `fixed_point` lagged-weight updates of `sor`
        red-black SOR sweeps with relaxation `omega`; None takes the defaults 20, 5, 0.1, 0.1, 5, 5, 1.6.  One linearisation:
        call refine again to re-warp.  The domain is self.mask & valid (a uint8 DeviceBuffer [H][W] or None) & finite
        vectors; a pixel outside it keeps its vector bit for bit and is nobody's neighbour; the data term acts where the
        pixel and its 4-neighbours are covered.  near, far, near_mask, far_mask, quant: as in census, one item
        ((C, H, W) or (1, C, H, W)), 1 to 4 channels.  Works for 's' and 't' fields; no zero-flow short cut; every operation
        float32 in a stated order, so the bits are reproducible.
        -> a DeviceFlow of the same shape, reference and mask; return_data appends the uint8 DeviceBuffer [H][W] of the
        pixels with a data term.  Nothing synchronises.  Not built: gradient constancy, per-channel data terms, more than 4
        channels, a loop over warps or a pyramid, edge-aware smoothness, a choice of omega, an energy read-back, a backward
        pass, mixed dtypes or layouts.  The inputs are not modified."""
        out, data = refine_op(refine_args(alpha, delta, zeta, eps, fixed_point, sor, omega), self.vecs, self.mask, self.shape,
                              self.ref, near, far, near_mask, far_mask, valid, return_data, quant)
        res = DeviceFlow(out, self.mask, self.shape, self.ref)          # buffers are immutable: the mask is shared
        return (res, data) if return_data else res

    def inverse_search(self, near, far, patch=8, stride=4, iterations=12, normalise=True, floor=1.0, return_patches=False,
                       quant=nat.QUANT_EXACT):
        """The field the two images ask for near this one: the patch inverse search and the densification of Dense Inverse
        Search (Kroeger et al., ECCV 2016; OpenCV's DISOpticalFlow; K24, include/ofl.h).  Every `patch` x `patch` window
        (4 or 8) on a grid of `stride` (1 ... patch) starts from this field's vector at its centre (+0 where the mask is unset
        or the vector not finite) and takes up to `iterations` (1 ... 32) inverse-compositional Lucas-Kanade translation
        steps on the channel means of `near` and `far`, with the patch means subtracted if `normalise`; it keeps the best
        step and never moves farther than `patch` pixels.  Every pixel then takes the average of the patches covering it,
        weighted by 1 / max(floor, |far there - near|) (raw intensities: floor = 1.0 is meant for 0 ... 255).  near, far: as
        in refine, one item ((C, H, W) or (1, C, H, W)), 1 to 4 channels, H and W at least `patch`.  Works for 's' and 't'
        fields; no zero-flow short cut; every operation float32 in a stated order, every sum of a patch a fixed tree across
        the lanes of a wave, so the bits are reproducible.  `quant` defaults to exact taps, as in correlation: the 1 / 32 px
        tap grid of QUANT_OPENCV is a floor an iterative search cannot get below.
        -> a DeviceFlow of the same shape and reference whose mask is set where the average is finite; return_patches appends
        (patch_vecs float32 DeviceBuffer [ny][nx][2], patch_ssd float32 DeviceBuffer [ny][nx], (ny, nx)).  Nothing
        synchronises.  Not built: OpenCV's propagation between neighbouring patches and its early exits, patches of 12 / 16
        px, per-channel residuals and more than 4 channels, near_mask / far_mask, affine patches, a backward pass; the pyramid
        is estimate_flow.  The inputs are not modified."""
        out, mask, pv, ps, grid = inverse_search_op(inverse_search_args(patch, stride, iterations, normalise, floor), self.vecs,
                                                    self.mask, self.shape, self.ref, near, far, return_patches, quant)
        res = DeviceFlow(out, mask, self.shape, self.ref)
        return (res, pv, ps, grid) if return_patches else res

    def error(self, gt, thresholds=None, outlier=None, speed_edges=None, use_est_mask=True, return_map=False, return_outliers=False):
        """How far this (estimated) field is from the ground truth `gt`, a DeviceFlow of the same shape and reference, in one
        launch of K14 (include/ofl.h) and without leaving HBM: per pixel epe = |self - gt| in float32 with one rounding per
        operation, evaluated where gt.mask (and, with use_est_mask, self.mask) is set and the error is finite.  thresholds: up
        to 4 EPE thresholds (default 1, 3, 5 px); outlier: (absolute, relative) -- a pixel is an outlier when its error exceeds
        both the absolute bound and the relative share of |gt| (default KITTI's 3 px and 5 %); speed_edges: up to 3 ascending
        magnitudes of gt that separate the speed bins (default Sintel's 10, 40); see args.error_args.
        -> a DeviceFlowError: the 96-byte record on the device plus, with return_map / return_outliers, `.epe_map` (float32
        [H][W], the error where evaluated, else 0) and `.outlier_map` (uint8 [H][W]) as DeviceBuffers.  Nothing synchronises
        until `.read()` -> FlowErrorStats.  Not a function of the reference: no angular error, no median.  The inputs are not
        modified."""
        thr, out, edges, n_thr, n_edges = error_args(thresholds, outlier, speed_edges)
        if not isinstance(gt, DeviceFlow):
            raise TypeError("Error evaluating flow error: gt needs to be a DeviceFlow, got {}".format(type(gt).__name__))
        if gt.shape != self.shape:
            raise ValueError("Error evaluating flow error: the fields need the same shape, got {} and {}".format(self.shape, gt.shape))
        if gt.ref != self.ref:
            raise ValueError("Error evaluating flow error: the fields need the same reference, got '{}' and '{}'".format(self.ref, gt.ref))
        records, epe_map, outlier_map = error_launch(self.vecs, self.mask if use_est_mask else None, gt.vecs, gt.mask, self.shape,
                                                     thr, out, edges, want_map=return_map, want_outliers=return_outliers)
        return DeviceFlowError(records, None, n_thr, n_edges, epe_map, outlier_map)

    def fill(self, valid=None, max_dist=None, return_index=False, return_d2=False):
        """The vectors of masked-out pixels replaced by the vector of the nearest valid pixel, in two launches of K15
        (include/ofl.h) and without leaving HBM.  A pixel is a source where self.mask -- and `valid`, a uint8 DeviceBuffer of
        H * W bytes such as `consistent` out of DeviceFlow.consistency, if given -- is set; every pixel takes the 8 bytes of
        the vector of its nearest source (squared Euclidean pixel distance, an exact integer; among equally near sources the
        one with the smallest linear index), provided that one lies within `max_dist` px (None: no limit; args.fill_args).
        A pixel that is not filled keeps its vector.  -> a DeviceFlow of the same shape and reference whose mask is 1 where a
        pixel was filled (sources included); return_index appends the int32 DeviceBuffer [H][W] of the nearest source's
        linear index (-1: none), return_d2 the uint32 DeviceBuffer [H][W] of its squared distance (0xFFFFFFFF: none).
        Not a function of the reference.  Nothing synchronises; the inputs are not modified."""
        max_d2 = fill_args(max_dist)
        valid = mask_buffer_arg(valid, self.n_px, "Error filling flow: ", "valid")
        out_vecs, out_mask, index, d2 = fill_launch(self.vecs, self.mask, valid, self.shape, max_d2,
                                                    want_index=bool(return_index), want_d2=bool(return_d2))
        res = DeviceFlow(out_vecs, out_mask, self.shape, self.ref)
        extra = ((index,) if return_index else ()) + ((d2,) if return_d2 else ())
        return (res,) + extra if extra else res

    def median(self, ksize=5, valid=None, only=None, min_count=None):
        """The vectors median-filtered over a ksize x ksize window (3, 5 or 7), mask-aware, in one launch of K16
        (include/ofl.h) and without leaving HBM.  A pixel is a member where self.mask -- and `valid`, a uint8 DeviceBuffer
        of H * W bytes such as `consistent` out of DeviceFlow.consistency, if given -- is set; every pixel takes, per
        component, the lower median of the members in its window (the frame edge shrinks the window; the centre is a
        member like any other), provided there are at least `min_count` of them (None: 1; args.median_args).  `only`, a
        uint8 DeviceBuffer of H * W bytes, restricts the filter to the pixels where it is set: the others keep vector and
        mask.  A filtered pixel with too few members keeps its vector and gets mask 0.  Every output word is a word of
        the input: nothing is averaged, NaN payloads and -0.0 survive.  -> a DeviceFlow of the same shape and reference.
        Not a function of the reference.  Nothing synchronises; the inputs are not modified."""
        ksize, min_count = median_args(ksize, min_count)
        valid = mask_buffer_arg(valid, self.n_px, "Error filtering flow: ", "valid")
        only = mask_buffer_arg(only, self.n_px, "Error filtering flow: ", "only")
        out_vecs, out_mask = median_launch(self.vecs, self.mask, valid, only, self.shape, ksize, min_count)
        return DeviceFlow(out_vecs, out_mask, self.shape, self.ref)

    def upsample_convex(self, weights, factor=8):
        """This field, a network's coarse flow of shape (h, w), convexly upsampled by `factor` (2, 4 or 8) in one launch of
        K17 (include/ofl.h) and without leaving HBM: `weights`, a DeviceTensor of logical shape (9 f^2, h, w) in either
        layout and of float32, float16 or bfloat16, holds the network's mask logits in RAFT's channel order; every fine
        pixel is the softmax-weighted combination of the 3 x 3 coarse neighbours, times f, with zero padding at the frame
        edge.  The mask of a fine pixel is set where every neighbour inside the frame is valid.  -> a DeviceFlow of shape
        (f h, f w) with the same reference.  Nothing synchronises; the inputs are not modified."""
        factor = upsample_weights(weights, factor, self.shape)
        out_vecs, out_mask = upsample_launch(self.vecs, self.mask, weights.buf, weights.dtype, weights.layout, self.shape, factor)
        return DeviceFlow(out_vecs, out_mask, (factor * self.shape[0], factor * self.shape[1]), self.ref)

    # -- forward warp by splatting (K20)
    def _splat_field(self, what):
        if self.ref != 's':
            raise ValueError("Error splatting: {} pushes values forward along an 's'-reference field; a 't'-reference field "
                             "warps backward, with apply_tensor".format(what))

    def splat(self, tensor, mode='average', importance=None, alpha=1.0, min_weight=None, frac_bits=None, return_weight=False,
              return_counters=False):
        """Forward-warp an HBM-resident DeviceTensor -- (C, H, W) or (N, C, H, W), either layout, float32 / float16 /
        bfloat16 -- by splatting (K20, include/ofl.h): every source pixel adds its channels to the four pixels around where
        this 's'-reference field sends it, with bilinear weights.  mode 'sum' leaves the sums, 'average' divides by the summed
        weight, 'softmax' weights source pixel p by exp(alpha * importance[p]) first -- `importance` a float32 DeviceBuffer
        [H][W], e.g. `residual` out of consistency with a negative alpha, so that among colliding sources the consistent
        one wins.  The sums are int64 fixed point with `frac_bits` fraction bits (None: 24), so the result does not depend
        on the order the atomics arrive in; a target pixel is valid where its summed weight reaches `min_weight` (None:
        2^-10), and an invalid pixel of 'average' / 'softmax' is 0.  This one field splats every item of a batched tensor.
        -> (DeviceTensor of the input's shape, dtype and layout, valid uint8 DeviceBuffer [H][W]); return_weight appends the
        float32 DeviceBuffer [H][W] of summed weights, return_counters appends (skipped source pixels, dropped values) as
        Python ints -- the only option that synchronises.  A 't'-reference field raises ValueError (apply_tensor gathers
        with those).  Not the reference's 's' apply: see apply_image for that.  The inputs are not modified."""
        self._splat_field("splat")
        if not isinstance(tensor, DeviceTensor):
            raise TypeError("Error splatting: tensor needs to be a DeviceTensor, got {}".format(type(tensor).__name__))
        code, alpha, min_weight, frac_bits = splat_args(mode, importance is not None, alpha, min_weight, frac_bits)
        n, c, h, w, _ = tensor_args(tensor.shape, tensor.layout, tensor.dtype, self.shape)
        z = splat_importance(importance, self.n_px)
        dst, valid, weight, counters = splat_launch(tensor.buf, tensor.dtype, tensor.layout, n, c, self.shape, self.vecs, self.mask,
                                                    True, code, alpha, min_weight, frac_bits, z=z, want_weight=bool(return_weight),
                                                    want_counters=bool(return_counters))
        res = (DeviceTensor(dst, tensor.shape, tensor.dtype, tensor.layout), valid) + ((weight,) if return_weight else ())
        if return_counters:
            k = counters.to_host((2,), np.uint32)
            res += ((int(k[0]), int(k[1])),)
        return res

    def coverage(self, importance=None, alpha=1.0, min_weight=None):
        """The range map of this 's'-reference field: how much bilinear weight lands on every pixel -- about 1 where the
        field is a translation, above 1 where it contracts (occlusion), below where it expands, 0 where nothing arrives
        (disocclusion) -- from K20 without channels.  With `importance` (float32 DeviceBuffer [H][W]) the weights are those of
        softmax splatting, relative to the largest importance that reaches the pixel.  -> (weight float32 DeviceBuffer
        [H][W], valid uint8 DeviceBuffer [H][W] = weight >= min_weight).  Nothing synchronises."""
        self._splat_field("coverage")
        mode = 'average' if importance is None else 'softmax'
        code, alpha, min_weight, frac_bits = splat_args(mode, importance is not None, alpha, min_weight, None)
        z = splat_importance(importance, self.n_px)
        _, valid, weight, _ = splat_launch(None, 'float32', 'hwc', 1, 0, self.shape, self.vecs, self.mask, True, code, alpha,
                                           min_weight, frac_bits, z=z, want_weight=True)
        return weight, valid

    def project(self, mode='average', importance=None, alpha=1.0, min_weight=None):
        """This 's'-reference field carried to the other frame: the 't'-reference DeviceFlow whose vector at a pixel is the
        splat (K20; `mode` 'average' or 'softmax' with `importance`) of the vectors of the source pixels that land there --
        the vector buffer is read as an (H, W, 2) float32 tensor, without a copy -- and whose mask is `valid`; fill() closes
        the holes.  Unlike switch_ref, which interpolates exactly over the Delaunay triangulation of the displaced grid (K3)
        and so fills every triangle, this averages what arrives: it is a few streaming launches, it leaves holes where
        nothing lands, and where the field folds it blends the colliding vectors (or, with softmax, prefers the important
        ones) instead of choosing a triangle.  Nothing synchronises."""
        self._splat_field("project")
        if mode == 'sum':
            raise ValueError("Error splatting: project takes mode 'average' or 'softmax': a sum of vectors is not a flow")
        code, alpha, min_weight, frac_bits = splat_args(mode, importance is not None, alpha, min_weight, None)
        z = splat_importance(importance, self.n_px)
        dst, valid, _, _ = splat_launch(self.vecs, 'float32', 'hwc', 1, 2, self.shape, self.vecs, self.mask, True, code, alpha,
                                        min_weight, frac_bits, z=z)
        return DeviceFlow(dst, valid, self.shape, 't')

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
            arith, rule = remap_rules(image.dtype, target_mask is not None)
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

    def apply_tensor(self, tensor, target_mask=None, quant=nat.QUANT_OPENCV):
        """Warp an HBM-resident DeviceTensor -- (C, H, W) or (N, C, H, W), either layout, float32 / float16 / bfloat16 -- and
        propagate validity: every channel is Flow.apply of that plane (flow_class.py:604-695, without padding) from ONE set
        of taps per pixel, one launch of K12; 16-bit tensors are blended in float32 and rounded once.  This one field warps
        every item of a batched tensor.  -> (DeviceTensor, valid-area DeviceBuffer [H][W]).  `target_mask`: uint8
        DeviceBuffer [H][W] or None (all valid).  Reference 't' only: an 's'-reference field pushes a tensor forward with
        splat (K20)."""
        if self.ref != 't':
            raise ValueError("apply_tensor warps with 't'-reference fields only: an 's'-reference field warps a tensor forward "
                             "with splat")
        n, c, h, w, _ = tensor_args(tensor.shape, tensor.layout, tensor.dtype, self.shape)
        if self.is_zero(thresholded=True, masked=False):        # identity short cut, utils.py:215-216
            valid = DeviceBuffer(self.n_px)
            if target_mask is None:
                nat.check(_lib().ofl_copy_dev(valid.ptr, self.mask.ptr, self.n_px, None))
            else:
                _mask_and(self.mask, target_mask, valid, self.n_px)
            return tensor, valid
        dst, valid = gather_tensor(tensor.buf, tensor.dtype, tensor.layout, n, c, h, w, self.vecs, True, -1, smask=target_mask,
                                   smask_shared=True, fmask=self.mask, want_valid=True, quant=quant)
        return DeviceTensor(dst, tensor.shape, tensor.dtype, tensor.layout), valid

    def apply_image_rows(self, image, rank, world, target_mask=None, consider_mask=True, quant=nat.QUANT_OPENCV,
                         gather=None, align=8):
        """This rank's ROW BAND of apply_image when ONE field is split over `world` GPUs (BASELINE config 5):
        flow, masks and image are the replicated H x W arrays, the result holds rows sharding.row_band(H, rank, world, align)
        only -- (DeviceImage rows x W x C, valid rows x W, (row0, row1)); the bands of all ranks concatenate to
        apply_image's result bit for bit.  't': one launch of the gather kernel on the band (nothing is exchanged).  's':
        a field whose mesh certifies resolves its rows in one kernel (nothing is exchanged); any other field takes the
        slab-wise Delaunay path with its one all-gather (`gather`: see scatter_slab; default RCCL)."""
        h, w = self.shape
        if image.shape[:2] != (h, w):
            raise ValueError("image and flow need the same height and width")
        r0, r1 = row_band(h, rank, world, align)
        rows = r1 - r0
        C = image.shape[2]
        if self.ref == 't':
            if rows <= 0:                       # more ranks than 8-row tiles: nothing to compute, and 't' exchanges nothing
                return None, None, (r0, r1)
            arith, rule = remap_rules(image.dtype, target_mask is not None)
            if self.is_zero(thresholded=True, masked=False):        # identity short cut, utils.py:215-216
                nb = rows * w * C * image.dtype.itemsize
                dst = DeviceImage(DeviceBuffer(nb), (rows, w, C), image.dtype)
                nat.check(_lib().ofl_copy_dev(dst.buf.ptr, image.buf.ptr + r0 * w * C * image.dtype.itemsize, nb, None))
                valid = DeviceBuffer(rows * w)
                if target_mask is None:
                    nat.check(_lib().ofl_copy_dev(valid.ptr, self.mask.ptr + r0 * w, rows * w, None))
                else:
                    _mask_and(self.mask.view(r0 * w, rows * w), target_mask.view(r0 * w, rows * w), valid, rows * w)
                return dst, valid, (r0, r1)
            dst, valid = gather_rows(image, r0, rows, self.vecs.view(r0 * w * 8, rows * w * 8), -1, smask=target_mask,
                                     fmask_rows=self.mask.view(r0 * w, rows * w), want_valid=True, quant=quant, arith=arith, rule=rule)
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
            # Does the walk kernel find every node of this certified mesh (scatter.walk_check)?  The answer must be the SAME on
            # every rank -- a rank that went on alone to the slab-wise path would wait for the others in its all-gather --
            # so each rank asks for the whole field once per certificate (validity only: 0.1 ms at 4K), not for its band.
            def whole_field(counter):
                scratch = DeviceBuffer(self.n_px)
                nat.check(_lib().ofl_scatter_certified_dev(self.vecs.ptr, +1, 0, None, 0, vmask.ptr, h, w, 0, h,
                                                           None, scratch.ptr, 0, ctypes.byref(cert), counter, None))
            walk_check(cert, whole_field)
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


# ------------------------------------------------------------------------------ a field out of two images
def estimate_flow(near, far, ref='s', levels=None, patch=8, stride=4, iterations=12, refine=True, refine_args=None, init=None):
    """The flow between two images, estimated on the device without a network: Dense Inverse Search (Kroeger et al., ECCV
    2016; OpenCV's DISOpticalFlow) -- coarse to fine over a pyramid of 2 x 2 means (DeviceTensor.halve), at every level
    DeviceFlow.inverse_search (K24) from the level above and, with `refine`, DeviceFlow.refine (K23; `refine_args`: a dict of
    its settings or None), then resize(2) to the next level.  near: the image of the field's own frame, far: that of the
    other frame -- DeviceTensors of one item ((C, H, W) or (1, C, H, W)) with 1 to 4 channels, one layout and dtype, or
    float32 DeviceImages; intensities 0 ... 255 are what the defaults are meant for.  ref: 's' or 't'.  levels: 1 ... 6 or None,
    the largest count <= 6 such that H and W are divisible by 2^(levels - 1) and the coarsest level measures at least 2 patch
    in both axes; a count that does not meet both is a ValueError (pad the images first).  init: a DeviceFlow of the images'
    shape and of `ref` to start from (resized to the coarsest level) or None, the zero field.
    -> a DeviceFlow of the images' shape.  A plain loop over existing methods: no kernel of its own, nothing synchronises.
    Not built: sizes that are not divisible (pad first), a fused multi-level launch, OpenCV's patch propagation, parity with
    cv2.DISOpticalFlow itself."""
    from .utils import get_valid_ref
    prefix = "Error estimating flow: "
    ref = get_valid_ref(ref)
    for name, t in (("near", near), ("far", far)):
        if not isinstance(t, (DeviceTensor, DeviceImage)):
            raise TypeError("{}{} needs to be a DeviceTensor or a float32 DeviceImage, got {}".format(prefix, name, type(t).__name__))
    shape = (near.h, near.w) if isinstance(near, DeviceTensor) else tuple(near.shape[:2])
    near, far = photometric_tensors(near, far, shape, prefix=prefix)
    inverse_search_channels(near.channels)
    if near.n != 1:
        raise ValueError("{}two images make one field: tensors of shape (C, H, W) or (1, C, H, W), got {}".format(prefix, near.shape))
    settings = inverse_search_args(patch, stride, iterations)
    levels = estimate_levels(shape, levels, settings[0])
    if refine_args is not None and not isinstance(refine_args, dict):
        raise TypeError("{}refine_args needs to be a dict or None, got {}".format(prefix, type(refine_args).__name__))
    if init is not None and (not isinstance(init, DeviceFlow) or init.shape != shape or init.ref != ref):
        raise ValueError("{}init needs to be a DeviceFlow of shape {} and reference '{}'".format(prefix, shape, ref))
    pyramid = [(near, far)]
    for _ in range(levels - 1):
        pyramid.append((pyramid[-1][0].halve(), pyramid[-1][1].halve()))
    coarse = (shape[0] >> (levels - 1), shape[1] >> (levels - 1))
    if init is None:
        flow = DeviceFlow.zero(coarse, ref)
    else:
        flow = init if levels == 1 else init.resize(1.0 / (1 << (levels - 1)))
    for level in range(levels - 1, -1, -1):
        a, b = pyramid[level]
        flow = flow.inverse_search(a, b, patch=patch, stride=stride, iterations=iterations)
        if refine:
            flow = flow.refine(a, b, **(refine_args or {}))
        if level:
            flow = flow.resize(2)
    return flow
