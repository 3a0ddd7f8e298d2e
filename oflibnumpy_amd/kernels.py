"""Thin launch wrappers of the library's kernel families on buffers that are already in HBM: K1 gather, K2 compose, K4
statistics, K7 visualise, K8 matrix fit, K9 build / resize, K10 tracking, K12 tensor warps, K13 consistency, K14 flow error, K15 fill, K16 median filter, K17 convex upsampling, K18 correlation lookup, K19 global matching, K20 splatting, K21 photometric error, K22 census distance, K23 variational refinement, K24 dense inverse search, K25 sequence accumulation and K26 structural similarity.  Each wrapper allocates what the entry needs,
passes pointers and returns buffers; the scatter kernel K3 and its multi-rank protocol live in scatter.py, the exchange
with other frameworks (K11) in interop.py.  The wrappers that hand back a DeviceImage (gather_bilinear, gather_rows,
visualise_launch) stay next to that class in device.py.
"""
import numpy as np

from . import _native as nat
from .memory import DeviceBuffer, _BufferView, _lib, _ptr, _size_query
from .args import (DEFAULT_THRESHOLD, _DT_CODE, _TRACK_DT, _TENSOR_EL, _TENSOR_LAYOUT, percentile_ranks, resize_scales,
                   resized_shape, mask_bytes, valid_mask_array, patch_origins)


def _host_ptr(a):
    """Address of a host array for a host-array entry point, None (NULL: the argument is absent) for None."""
    return None if a is None else a.ctypes.data


# ------------------------------------------------------------------------------ K1: gather
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
        _ptr(src), 1 if shared_src else 0, _DT_CODE[dtype], C, H, W, batch, flow.ptr, fH, fW, pad[0], pad[1], sign,
        _ptr(smask), 1 if shared_smask else 0, _ptr(fmask), _ptr(dst if C else None), _ptr(valid), quant, arith, rule, stream))
    return dst, valid


def gather_valid_only(H, W, flow_buf, flow_shape, sign, smask=None, fmask=None, pad=(0, 0),
                      quant=nat.QUANT_OPENCV, rule=nat.RULE_EQ1, stream=None, valid=None):
    """K1 without image channels: where does a warped all-ones (or smask) image stay == 1?
    (valid_target 't' flow_class.py:1148-1150, valid_source 's' :1179-1183).  -> `valid`, allocated when not given."""
    valid = DeviceBuffer(H * W) if valid is None else valid
    nat.check(_lib().ofl_gather_bilinear_dev(
        None, nat.U8, 0, H, W, flow_buf.ptr, flow_shape[0], flow_shape[1], pad[0], pad[1], sign,
        _ptr(smask), _ptr(fmask), None, valid.ptr, quant, nat.ARITH_NATIVE, rule, stream))
    return valid


# ------------------------------------------------------------------------------ K4: statistics, K2: compose
def flow_stats(vecs_buf, mask_buf, n_px, stream=None):
    """K4: OFL_STAT_* bits of one field (utils.py:527-544, flow_class.py:1230-1245)."""
    out = DeviceBuffer(16)
    nat.check(_lib().ofl_flow_stats_dev(vecs_buf.ptr, _ptr(mask_buf), n_px, np.float32(DEFAULT_THRESHOLD), out.ptr, stream))
    return int(out.to_host((1,), np.uint32, stream)[0])


def compose3_launch(fa, fb, sign, out, stats_buf=None, stats_offset=0, batch=1, quant=nat.QUANT_OPENCV,
                    stream=None):
    """K2 launch on raw DeviceFlow-like triples; asynchronous.  stats_buf: uint32[batch][8] words."""
    H, W = fa.shape
    sp = None if stats_buf is None else stats_buf.ptr + stats_offset
    nat.check(_lib().ofl_compose3_dev(fa.vecs.ptr, fa.mask.ptr, fb.vecs.ptr, fb.mask.ptr, sign, H, W, batch,
                                      out.vecs.ptr, out.mask.ptr, sp, quant, stream))


def mask_bits_bytes(h, w, batch=1):
    return _size_query(_lib().ofl_mask_bits_bytes, h, w, batch)


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


# ------------------------------------------------------------------------------ K13: forward-backward consistency
def consistency_launch(f_vecs, f_mask, b_vecs, b_mask, sign, shape, alpha, beta, batch=1, want_residual=False,
                       want_counts=False, quant=nat.QUANT_OPENCV, stream=None):
    """K13 (ofl_consistency_dev) on `batch` pairs stored back to back; asynchronous.  alpha, beta: float32, from
    args.consistency_args.  -> (consistent, covered, residual or None, counts or None): uint8 [batch][H][W] twice, float32
    [batch][H][W], and the zeroed-then-added uint32 [batch][2] = {covered, consistent} words, all still in HBM."""
    n = batch * shape[0] * shape[1]
    consistent, covered = DeviceBuffer(n), DeviceBuffer(n)
    residual = DeviceBuffer(n * 4) if want_residual else None
    counts = DeviceBuffer.zeros(batch * 8, stream) if want_counts else None
    nat.check(_lib().ofl_consistency_dev(f_vecs.ptr, f_mask.ptr, b_vecs.ptr, b_mask.ptr, sign, shape[0], shape[1], batch,
                                         alpha, beta, consistent.ptr, covered.ptr, _ptr(residual), _ptr(counts), quant, stream))
    return consistent, covered, residual, counts


def consistency_host(f_vecs, f_mask, b_vecs, b_mask, sign, alpha, beta, want_residual=False, quant=nat.QUANT_OPENCV):
    """K13 for host arrays through ofl_consistency (upload, one launch, download) -> (consistent, covered[, residual]):
    bool (H, W) twice and float32 (H, W)."""
    f_vecs, b_vecs = np.ascontiguousarray(f_vecs, np.float32), np.ascontiguousarray(b_vecs, np.float32)
    fm, bm = mask_bytes(f_mask), mask_bytes(b_mask)
    h, w = f_vecs.shape[:2]
    consistent, covered = np.empty((h, w), np.uint8), np.empty((h, w), np.uint8)
    residual = np.empty((h, w), np.float32) if want_residual else None
    nat.check(_lib().ofl_consistency(f_vecs.ctypes.data, fm.ctypes.data, b_vecs.ctypes.data, bm.ctypes.data, sign, h, w, 1,
                                     alpha, beta, consistent.ctypes.data, covered.ctypes.data,
                                     _host_ptr(residual), None, quant))
    res = (consistent.view(np.bool_), covered.view(np.bool_))
    return res + (residual,) if want_residual else res


# ------------------------------------------------------------------------------ K14: an estimate against a ground truth
ERROR_RECORD = np.dtype([("n", np.uint32), ("n_nonfinite", np.uint32), ("n_over", np.uint32, 4), ("n_outlier", np.uint32),
                         ("n_bin", np.uint32, 4), ("max_epe_bits", np.uint32), ("sum_epe", np.float64), ("sum_epe2", np.float64),
                         ("sum_bin_epe", np.float64, 4)])          # struct ofl_flow_error of include/ofl.h, 96 bytes
assert ERROR_RECORD.itemsize == 96


class FlowErrorStats:
    """What one record of K14 says: `n` evaluated pixels and `n_nonfinite` pixels left out for a NaN / Inf (or an
    overflowing) error, `epe` (the mean end-point error), `rmse`, `max`, `over` (the share of pixels above each threshold
    given), `outlier` (the share that exceeds both outlier bounds: KITTI's Fl) and `bins` ((n, mean epe) per speed bin of the
    ground truth: one more than edges given).  A mean over zero pixels is nan."""

    __slots__ = ("n", "n_nonfinite", "epe", "rmse", "max", "over", "outlier", "bins")

    def __init__(self, record, n_thresholds=3, n_edges=2):
        n = int(record["n"])
        mean = lambda total, count: float(total) / count if count else float('nan')
        self.n, self.n_nonfinite = n, int(record["n_nonfinite"])
        self.epe = mean(record["sum_epe"], n)
        self.rmse = float(np.sqrt(mean(record["sum_epe2"], n)))
        self.max = float(np.array(record["max_epe_bits"], np.uint32).view(np.float32)) if n else float('nan')
        self.over = tuple(mean(int(c), n) for c in record["n_over"][:n_thresholds])
        self.outlier = mean(int(record["n_outlier"]), n)
        self.bins = tuple((int(c), mean(t, int(c))) for c, t in zip(record["n_bin"][:n_edges + 1], record["sum_bin_epe"][:n_edges + 1]))

    def _key(self):
        return (self.n, self.n_nonfinite, self.epe, self.rmse, self.max, self.over, self.outlier, self.bins)

    def __eq__(self, other):
        """equal field by field, nan equal to nan (the statistics of an empty evaluation set)"""
        return isinstance(other, FlowErrorStats) and repr(self._key()) == repr(other._key())

    __hash__ = None

    def __repr__(self):
        return "FlowErrorStats(n={}, n_nonfinite={}, epe={!r}, rmse={!r}, max={!r}, over={!r}, outlier={!r}, bins={!r})".format(*self._key())


def error_launch(est_vecs, est_mask, gt_vecs, gt_mask, shape, thr, outlier, edges, batch=1, want_map=False, want_outliers=False,
                 stream=None):
    """K14 (ofl_flow_error_dev) on `batch` pairs stored back to back; asynchronous.  thr, outlier, edges: from
    args.error_args; est_mask None: only the ground truth's mask selects.  The workspace comes from the buffer pool and goes
    back to it on return (one stream).  -> (records, epe_map or None, outlier_map or None): 96 bytes per pair, float32
    [batch][H][W], uint8 [batch][H][W], all still in HBM."""
    lib, n = _lib(), batch * shape[0] * shape[1]
    nbytes = _size_query(lib.ofl_flow_error_workspace_bytes, shape[0], shape[1], batch)
    work, records = DeviceBuffer(nbytes), DeviceBuffer(batch * ERROR_RECORD.itemsize)
    epe_map = DeviceBuffer(n * 4) if want_map else None
    outlier_map = DeviceBuffer(n) if want_outliers else None
    nat.check(lib.ofl_flow_error_dev(est_vecs.ptr, _ptr(est_mask), gt_vecs.ptr, gt_mask.ptr, shape[0], shape[1], batch,
                                     thr.ctypes.data, outlier[0], outlier[1], edges.ctypes.data, work.ptr, nbytes, records.ptr,
                                     _ptr(epe_map), _ptr(outlier_map), stream))
    return records, epe_map, outlier_map


def error_host(est_vecs, est_mask, gt_vecs, gt_mask, thr, outlier, edges, want_map=False, want_outliers=False):
    """K14 for host arrays through ofl_flow_error (upload, launch, download) -> (record, epe_map or None, outlier_map or
    None): one ERROR_RECORD element, float32 (H, W), bool (H, W).  est_mask None: only the ground truth's mask selects."""
    est_vecs, gt_vecs = np.ascontiguousarray(est_vecs, np.float32), np.ascontiguousarray(gt_vecs, np.float32)
    em, gm = (None if est_mask is None else mask_bytes(est_mask)), mask_bytes(gt_mask)
    h, w = est_vecs.shape[:2]
    record = np.zeros(1, ERROR_RECORD)
    epe_map = np.empty((h, w), np.float32) if want_map else None
    outlier_map = np.empty((h, w), np.uint8) if want_outliers else None
    nat.check(_lib().ofl_flow_error(est_vecs.ctypes.data, _host_ptr(em), gt_vecs.ctypes.data, gm.ctypes.data,
                                    h, w, 1, thr.ctypes.data, outlier[0], outlier[1], edges.ctypes.data, record.ctypes.data,
                                    _host_ptr(epe_map), _host_ptr(outlier_map)))
    return record[0], epe_map, None if outlier_map is None else outlier_map.view(np.bool_)


# ------------------------------------------------------------------------------ K15: fill from the nearest valid pixel
def fill_launch(vecs, mask, valid, shape, max_d2, batch=1, want_mask=True, want_index=False, want_d2=False, stream=None):
    """K15 (ofl_fill_dev) on `batch` fields stored back to back; asynchronous.  max_d2: from args.fill_args; valid None: the
    mask alone selects the sources; vecs None: the distance transform of the mask alone (want_index or want_d2 needed).  The
    workspace comes from the buffer pool and goes back to it on return (one stream).  -> (out_vecs or None, out_mask or None,
    index or None, d2 or None): float32 [batch][H][W][2], uint8, int32 and uint32 [batch][H][W], all still in HBM."""
    lib, n = _lib(), batch * shape[0] * shape[1]
    nbytes = _size_query(lib.ofl_fill_workspace_bytes, shape[0], shape[1], batch)
    work = DeviceBuffer(nbytes)
    out_vecs = DeviceBuffer(n * 8) if vecs is not None else None
    out_mask = DeviceBuffer(n) if want_mask else None
    index = DeviceBuffer(n * 4) if want_index else None
    d2 = DeviceBuffer(n * 4) if want_d2 else None
    nat.check(lib.ofl_fill_dev(_ptr(vecs), mask.ptr, _ptr(valid), shape[0], shape[1], batch, max_d2, work.ptr, nbytes,
                               _ptr(out_vecs), _ptr(out_mask), _ptr(index), _ptr(d2), stream))
    return out_vecs, out_mask, index, d2


def fill_host(vecs, mask, valid, max_d2, want_index=False, want_d2=False):
    """K15 for host arrays through ofl_fill (upload, launch, download) -> (vecs float32 (H, W, 2), mask bool (H, W), index
    int32 (H, W) or None, d2 uint32 (H, W) or None).  valid: contiguous uint8 (H, W) or None."""
    vecs, m = np.ascontiguousarray(vecs, np.float32), mask_bytes(mask)
    h, w = vecs.shape[:2]
    out_vecs, out_mask = np.empty((h, w, 2), np.float32), np.empty((h, w), np.uint8)
    index = np.empty((h, w), np.int32) if want_index else None
    d2 = np.empty((h, w), np.uint32) if want_d2 else None
    nat.check(_lib().ofl_fill(vecs.ctypes.data, m.ctypes.data, _host_ptr(valid), h, w, 1, max_d2,
                              out_vecs.ctypes.data, out_mask.ctypes.data, _host_ptr(index), _host_ptr(d2)))
    return out_vecs, out_mask.view(np.bool_), index, d2


# ------------------------------------------------------------------------------ K16: mask-aware median filter
def median_launch(vecs, mask, valid, only, shape, ksize, min_count, batch=1, want_mask=True, stream=None):
    """K16 (ofl_median_dev) on `batch` fields stored back to back; asynchronous, one launch.  ksize, min_count: from
    args.median_args; valid None: the mask alone selects the members; only None: every pixel is filtered.
    -> (out_vecs, out_mask or None): float32 [batch][H][W][2] and uint8 [batch][H][W], still in HBM."""
    n = batch * shape[0] * shape[1]
    out_vecs = DeviceBuffer(n * 8)
    out_mask = DeviceBuffer(n) if want_mask else None
    nat.check(_lib().ofl_median_dev(vecs.ptr, mask.ptr, _ptr(valid), _ptr(only), shape[0], shape[1], batch, ksize, min_count,
                                    out_vecs.ptr, _ptr(out_mask), stream))
    return out_vecs, out_mask


def median_host(vecs, mask, valid, only, ksize, min_count):
    """K16 for host arrays through ofl_median (upload, launch, download) -> (vecs float32 (H, W, 2), mask bool (H, W)).
    valid, only: contiguous uint8 (H, W) or None."""
    vecs, m = np.ascontiguousarray(vecs, np.float32), mask_bytes(mask)
    h, w = vecs.shape[:2]
    out_vecs, out_mask = np.empty((h, w, 2), np.float32), np.empty((h, w), np.uint8)
    nat.check(_lib().ofl_median(vecs.ctypes.data, m.ctypes.data, _host_ptr(valid), _host_ptr(only), h, w, 1, ksize, min_count,
                                out_vecs.ctypes.data, out_mask.ctypes.data))
    return out_vecs, out_mask.view(np.bool_)


# ------------------------------------------------------------------------------ K17: convex upsampling
def upsample_launch(vecs, mask, weights, dtype, layout, shape, factor, batch=1, want_mask=True, stream=None):
    """K17 (ofl_upsample_convex_dev) on `batch` coarse fields of `shape` (h, w) stored back to back; asynchronous, one
    launch.  weights: the buffer of the logits, [batch][9 f^2][h][w] ('chw') or [batch][h][w][9 f^2] ('hwc') of `dtype`;
    factor: from args.upsample_args.  -> (out_vecs, out_mask or None): float32 [batch][f h][f w][2] and uint8
    [batch][f h][f w], still in HBM."""
    n = batch * shape[0] * shape[1] * factor * factor
    out_vecs = DeviceBuffer(n * 8)
    out_mask = DeviceBuffer(n) if want_mask else None
    nat.check(_lib().ofl_upsample_convex_dev(vecs.ptr, mask.ptr, weights.ptr, _TENSOR_EL[dtype], _TENSOR_LAYOUT[layout],
                                             shape[0], shape[1], batch, factor, out_vecs.ptr, _ptr(out_mask), stream))
    return out_vecs, out_mask


def upsample_host(vecs, mask, weights, factor):
    """K17 for host arrays through ofl_upsample_convex (upload, launch, download) -> (vecs float32 (f h, f w, 2), mask bool
    (f h, f w)).  weights: a contiguous float32 or float16 array (9 f^2, h, w)."""
    vecs, m = np.ascontiguousarray(vecs, np.float32), mask_bytes(mask)
    h, w = vecs.shape[:2]
    out_vecs, out_mask = np.empty((factor * h, factor * w, 2), np.float32), np.empty((factor * h, factor * w), np.uint8)
    nat.check(_lib().ofl_upsample_convex(vecs.ctypes.data, m.ctypes.data, weights.ctypes.data, _TENSOR_EL[weights.dtype.name],
                                         nat.TENSOR_NCHW, h, w, 1, factor, out_vecs.ctypes.data, out_mask.ctypes.data))
    return out_vecs, out_mask.view(np.bool_)


# ------------------------------------------------------------------------------ K7: visualise, K8: matrix fit
def visualise_range_launch(vecs, h, w, batch, out, stream=None):
    """K7 range select: out (float32[batch] on the device) <- the default range_max of every field, flow_class.py:910-916.
    Asynchronous."""
    lo, hi, gamma = percentile_ranks(h * w)
    ws = DeviceBuffer(_size_query(_lib().ofl_visualise_workspace_bytes, h, w, batch))
    nat.check(_lib().ofl_visualise_range_dev(vecs.ptr, h, w, batch, np.float32(DEFAULT_THRESHOLD), lo, hi, gamma,
                                             ws.ptr, ws.nbytes, out.ptr, stream))


class FitField:
    """The K8 passes over one HBM-resident field (csrc/ofl_fit.hip), as the object matrix_fit.fit drives: each method
    enqueues one entry of include/ofl.h and reads its few numbers back.  mask: DeviceBuffer or None (every pixel counts);
    gate: None or (3x3 model, float32 squared threshold)."""

    def __init__(self, vecs, mask, shape, sign, stream=None):
        self.vecs, self.mask, self.sign, self.stream = vecs, mask, sign, stream
        self.h, self.w = int(shape[0]), int(shape[1])
        self.origin = ((self.w - 1) / 2.0, (self.h - 1) / 2.0)            # the grid centre
        self.ws = DeviceBuffer(_size_query(_lib().ofl_fit_workspace_bytes, self.h, self.w))
        self.out = DeviceBuffer(1024)

    def _field(self):
        return (self.vecs.ptr, _ptr(self.mask), self.h, self.w)

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


# ------------------------------------------------------------------------------ K9: build / resize, small helpers
def _valid_mask(mask, shape):
    """A constructor's `mask` argument: None, a DeviceBuffer of at least H * W bytes (0 / 1, taken as it is), or a host array
    checked like the Flow.mask setter (args.valid_mask_array) -> None, the buffer, or uint8 (H, W)."""
    if mask is None:
        return None
    if isinstance(mask, (DeviceBuffer, _BufferView)):
        if mask.nbytes < int(shape[0]) * int(shape[1]):
            raise ValueError("Error setting flow mask: Input has a different shape than the flow vectors")
        return mask
    return valid_mask_array(mask, shape)


def _mask_buffer(mask, shape):
    """What _valid_mask returned -> the field's mask buffer: all ones for None, an upload for a host array."""
    if mask is None:
        buf = DeviceBuffer(int(shape[0]) * int(shape[1]))
        nat.check(_lib().ofl_memset(buf.ptr, 1, int(shape[0]) * int(shape[1]), None))
        return buf
    return DeviceBuffer.from_host(mask) if isinstance(mask, np.ndarray) else mask


def flow_from_matrix_launch(mats, n, sign, shape, out, stream=None):
    """K9 constructor: `n` fields [n][H][W][2] into `out` from `mats`, n x 9 float64 on the device.  Asynchronous."""
    nat.check(_lib().ofl_flow_from_matrix_dev(mats.ptr, n, sign, shape[0], shape[1], out.ptr, stream))


def _mask_and(a, b, out, n):
    """out = a & b for uint8 masks (flow_class.py:643)."""
    nat.check(_lib().ofl_mask_and_dev(a.ptr, b.ptr, out.ptr, n, None))


def resize_host(vecs, mask, scale):
    """resize_flow / Flow.resize for host arrays through ofl_resize_flow (upload, one launch, download)."""
    fy, fx = resize_scales(scale)
    vecs = np.ascontiguousarray(vecs, np.float32)
    h, w = vecs.shape[:2]
    ho, wo = resized_shape(h, w, fy, fx)
    out = np.empty((ho, wo, 2), np.float32)
    m = None if mask is None else mask_bytes(mask)
    mout = None if mask is None else np.empty((ho, wo), np.uint8)
    nat.check(_lib().ofl_resize_flow(_host_ptr(vecs), _host_ptr(m), h, w, ho, wo, 1.0 / fy, 1.0 / fx,
                                     float(np.float32(fx)), float(np.float32(fy)), _host_ptr(out), _host_ptr(mout)))
    return out, (None if mout is None else mout.astype(bool))


def grid_minus(vecs, out, h, w):
    """out = float32(grid - vecs): the query positions of mode 2 / ref 't' (flow_class.py:1404-1406)."""
    nat.check(_lib().ofl_grid_offset_dev(vecs.ptr, -1, h, w, out.ptr, None))


def sample_points(flow_buf, h, w, pts_rc):
    """Bilinear flow samples (v, u) at float64 points (row, col): utils.py:161-196 / :605."""
    pts = np.ascontiguousarray(pts_rc, np.float64)
    n = pts.shape[0]
    dp = DeviceBuffer.from_host(pts)
    out = DeviceBuffer(max(n, 1) * 16)
    nat.check(_lib().ofl_sample_points_dev(flow_buf.ptr, h, w, dp.ptr, n, out.ptr, None))
    return out.to_host((n, 2), np.float64)


# ------------------------------------------------------------------------------ K10: tracking with resident points
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


def track_query_epilogue(query, vals, found, n, shape, stats, valid, step, status, out_rc=None, out_int=None, next_query=None,
                         lost_at=None, stream=None):
    """K10 tail of the query paths (ofl_track_query_epilogue_dev); asynchronous."""
    nat.check(_lib().ofl_track_query_epilogue_dev(query.ptr, vals.ptr, found.ptr, n, shape[0], shape[1], _ptr(stats), _ptr(valid),
                                                  step, _ptr(out_rc), _ptr(out_int), _ptr(next_query), _ptr(status),
                                                  _ptr(lost_at), stream))


# ------------------------------------------------------------------------------ K12: many-channel float tensors
def _tensor_bytes(dtype):
    return 4 if dtype == 'float32' else 2


def gather_tensor(src, dtype, layout, n, c, h, w, flow, flow_shared, sign, smask=None, smask_shared=False, fmask=None,
                  want_valid=False, quant=nat.QUANT_OPENCV, stream=None):
    """K12 (ofl_gather_tensor_dev) on `n` items of `c` channels in `layout` ('chw' / 'hwc'); asynchronous.  -> (dst buffer,
    valid buffer or None): valid is [n][H][W], or ONE [H][W] mask when the field and the target mask are shared."""
    dst = DeviceBuffer(n * c * h * w * _tensor_bytes(dtype))
    valid = None
    if want_valid:
        valid = DeviceBuffer(h * w * (1 if flow_shared and (smask is None or smask_shared) else n))
    nat.check(_lib().ofl_gather_tensor_dev(src.ptr, _TENSOR_EL[dtype], _TENSOR_LAYOUT[layout], n, c, h, w, flow.ptr,
                                           1 if flow_shared else 0, sign, _ptr(smask), 1 if smask_shared else 0, _ptr(fmask),
                                           dst.ptr, _ptr(valid), quant, stream))
    return dst, valid


def tensor_import_launch(src_ptr, dtype, strides, layout, n, c, h, w, stream=None):
    """ofl_tensor_import_dev: a strided foreign view, element strides (item, channel, row, column) -> a contiguous buffer."""
    dst = DeviceBuffer(n * c * h * w * _tensor_bytes(dtype))
    nat.check(_lib().ofl_tensor_import_dev(src_ptr, _tensor_bytes(dtype), strides[0], strides[1], strides[2], strides[3],
                                           _TENSOR_LAYOUT[layout], n, c, h, w, dst.ptr, stream))
    return dst


def tensor_permute_launch(src, dtype, n, c, h, w, to_hwc, stream=None):
    """ofl_tensor_permute_dev: contiguous 'chw' -> 'hwc' (to_hwc) or back, into a fresh buffer."""
    dst = DeviceBuffer(n * c * h * w * _tensor_bytes(dtype))
    nat.check(_lib().ofl_tensor_permute_dev(src.ptr, dst.ptr, _tensor_bytes(dtype), n, c, h, w, 1 if to_hwc else 0, stream))
    return dst


def tensor_halve_launch(src, dtype, layout, n, c, h, w, stream=None):
    """ofl_tensor_halve_dev: the 2 x 2 mean of a tensor of either layout -> a fresh buffer of the same layout and dtype with
    h >> 1 rows and w >> 1 columns."""
    dst = DeviceBuffer(n * c * (h >> 1) * (w >> 1) * _tensor_bytes(dtype))
    nat.check(_lib().ofl_tensor_halve_dev(src.ptr, _TENSOR_EL[dtype], _TENSOR_LAYOUT[layout], n, c, h, w, dst.ptr, stream))
    return dst


# ------------------------------------------------------------------------------ K18: on-demand correlation lookup
def avgpool2_launch(src, dtype, n, c, h, w, stream=None):
    """ofl_avgpool2_dev: the 2 x 2 mean of a channels-last tensor [n][h][w][c] of `dtype` -> float32 [n][h >> 1][w >> 1][c]."""
    dst = DeviceBuffer(n * (h >> 1) * (w >> 1) * c * 4)
    nat.check(_lib().ofl_avgpool2_dev(src.ptr, _TENSOR_EL[dtype], n, c, h, w, dst.ptr, stream))
    return dst


def corr_lookup_launch(f1, dtype1, pyramid, n, c, h, w, flow, flow_shared, sign, radius, scale, order, quant, stream=None):
    """K18 (ofl_corr_lookup_dev), one launch per level of `pyramid`, a list of (buffer, dtype) of the channels-last levels
    of f2; f1: the channels-last buffer [n][h][w][c] of `dtype1`; flow: the buffer of the field(s) or None; scale, order,
    quant: from args.corr_args.  Asynchronous.  -> float32 [n][levels (2 radius + 1)^2][h][w], still in HBM."""
    nch = (2 * radius + 1) ** 2
    total = len(pyramid) * nch
    out = DeviceBuffer(n * total * h * w * 4)
    for level, (buf, dtype2) in enumerate(pyramid):
        nat.check(_lib().ofl_corr_lookup_dev(f1.ptr, _TENSOR_EL[dtype1], buf.ptr, _TENSOR_EL[dtype2], n, c, h, w, h >> level, w >> level,
                                             level, _ptr(flow), 1 if flow_shared else 0, sign, radius, scale, order, quant,
                                             out.ptr, total, level * nch, stream))
    return out


def corr_lookup_host(f1, f2, flow, sign, radius, levels, scale, order, quant):
    """K18 for host arrays through ofl_corr_lookup (upload, pyramid, `levels` launches, download): f1, f2 contiguous
    channels-last (n, h, w, c) of float32 or float16, flow float32 (h, w, 2) -- one field for all items -- or None
    -> float32 (n, levels (2 radius + 1)^2, h, w)."""
    n, h, w, c = f1.shape
    out = np.empty((n, levels * (2 * radius + 1) ** 2, h, w), np.float32)
    nat.check(_lib().ofl_corr_lookup(f1.ctypes.data, _TENSOR_EL[f1.dtype.name], f2.ctypes.data, _TENSOR_EL[f2.dtype.name], n, c, h, w,
                                     levels, _host_ptr(flow), 1, sign, radius, scale, order, quant, out.ctypes.data))
    return out


# ------------------------------------------------------------------------------ K19: global matching
def match_launch(f1, f2, dtype, n, c, h, w, scale, sign, min_conf, want_conf=False, want_index=False, stream=None):
    """K19 (ofl_global_match_dev) on `n` pairs of channels-last tensors [n][h][w][c] of `dtype` stored back to back;
    asynchronous, one launch.  scale, min_conf: from args.match_args.  -> (vecs, mask, confidence or None, index or None):
    float32 [n][h][w][2], uint8, float32 and int32 [n][h][w], still in HBM."""
    px = n * h * w
    vecs, mask = DeviceBuffer(px * 8), DeviceBuffer(px)
    conf = DeviceBuffer(px * 4) if want_conf else None
    index = DeviceBuffer(px * 4) if want_index else None
    nat.check(_lib().ofl_global_match_dev(f1.ptr, f2.ptr, _TENSOR_EL[dtype], n, c, h, w, scale, sign, min_conf, vecs.ptr, mask.ptr,
                                          _ptr(conf), _ptr(index), stream))
    return vecs, mask, conf, index


def match_host(f1, f2, scale, sign, min_conf, want_conf=False, want_index=False):
    """K19 for host arrays through ofl_global_match (upload, launch, download): f1, f2 contiguous channels-last (n, h, w, c)
    of one dtype, float32 or float16 -> (vecs float32 (n, h, w, 2), mask bool (n, h, w), confidence float32 (n, h, w) or
    None, index int32 (n, h, w) or None)."""
    n, h, w, c = f1.shape
    vecs, mask = np.empty((n, h, w, 2), np.float32), np.empty((n, h, w), np.uint8)
    conf = np.empty((n, h, w), np.float32) if want_conf else None
    index = np.empty((n, h, w), np.int32) if want_index else None
    nat.check(_lib().ofl_global_match(f1.ctypes.data, f2.ctypes.data, _TENSOR_EL[f1.dtype.name], n, c, h, w, scale, sign, min_conf,
                                      vecs.ctypes.data, mask.ctypes.data, _host_ptr(conf), _host_ptr(index)))
    return vecs, mask.view(np.bool_), conf, index


# ------------------------------------------------------------------------------ K20: forward warp by splatting
def splat_launch(src, dtype, layout, n, c, shape, flow, fmask, flow_shared, mode, alpha, min_weight, frac_bits, z=None,
                 want_valid=True, want_weight=False, want_counters=False, stream=None):
    """K20 (ofl_splat_dev) on `n` items of `c` channels in `layout` ('chw' / 'hwc') of `dtype`; asynchronous: [the max pass,]
    accumulate, finish.  src None with c = 0: only the weight plane is accumulated.  mode, alpha, min_weight, frac_bits: from
    args.splat_args; z: the float32 importance buffer or None.  The workspace comes from the buffer pool and goes back to it
    on return (one stream).  -> (dst or None, valid or None, weight or None, counters or None): valid uint8 and weight
    float32 are ONE [H][W] plane when the field is shared, else [n][H][W]; counters the zeroed-then-added uint32[2], all
    still in HBM."""
    lib, (h, w) = _lib(), shape
    shared = 1 if flow_shared else 0
    planes = h * w * (1 if flow_shared else n)
    nbytes = _size_query(lib.ofl_splat_workspace_bytes, n, c, h, w, shared, mode)
    work = DeviceBuffer(nbytes)
    dst = DeviceBuffer(n * c * h * w * _tensor_bytes(dtype)) if c else None
    valid = DeviceBuffer(planes) if want_valid else None
    weight = DeviceBuffer(planes * 4) if want_weight else None
    counters = DeviceBuffer.zeros(8, stream) if want_counters else None
    nat.check(lib.ofl_splat_dev(_ptr(src), _TENSOR_EL[dtype], _TENSOR_LAYOUT[layout], n, c, h, w, flow.ptr, fmask.ptr, shared,
                                _ptr(z), alpha, mode, frac_bits, min_weight, work.ptr, nbytes, _ptr(dst), _ptr(valid),
                                _ptr(weight), _ptr(counters), stream))
    return dst, valid, weight, counters


def splat_host(src, layout, n, c, vecs, mask, mode, alpha, min_weight, frac_bits, z=None, want_weight=False, want_counters=False):
    """K20 for host arrays through ofl_splat (upload, launches, download): src a contiguous float32 or float16 array in the
    memory order of `layout` (None with c = 0), ONE field (vecs (H, W, 2), mask) for all `n` items, z float32 (H, W) or None
    -> (dst or None, valid bool (H, W), weight float32 (H, W) or None, counters (skipped, dropped) or None)."""
    vecs, m = np.ascontiguousarray(vecs, np.float32), mask_bytes(mask)
    h, w = vecs.shape[:2]
    dst = None if src is None else np.empty_like(src)
    valid = np.empty((h, w), np.uint8)
    weight = np.empty((h, w), np.float32) if want_weight else None
    counters = np.zeros(2, np.uint32) if want_counters else None
    nat.check(_lib().ofl_splat(_host_ptr(src), _TENSOR_EL['float32' if src is None else src.dtype.name], _TENSOR_LAYOUT[layout],
                               n, c, h, w, vecs.ctypes.data, m.ctypes.data, 1, _host_ptr(z), alpha, mode, frac_bits, min_weight,
                               _host_ptr(dst), valid.ctypes.data, _host_ptr(weight), _host_ptr(counters)))
    return dst, valid.view(np.bool_), weight, None if counters is None else (int(counters[0]), int(counters[1]))


# ------------------------------------------------------------------------------ K21 ... K24: what the image-pair families share
def _pair_head(near, far, dtype, layout, n, c, shape):
    """the arguments every native entry of K21 ... K24 begins with; near, far: pointers"""
    return near, far, _TENSOR_EL[dtype], _TENSOR_LAYOUT[layout], n, c, shape[0], shape[1]


def _pair_error_launch(entry, near, far, dtype, layout, n, c, shape, flow, fmask, flow_shared, sign, settings, threshold,
                       near_mask, far_mask, want_err, want_covered, want_counts, quant, stream):
    """K21's, K22's and K26's device entries differ in their `settings` alone: the outputs allocated and the call made once"""
    px = n * shape[0] * shape[1]
    err = DeviceBuffer(px * 4) if want_err else None
    covered = DeviceBuffer(px) if want_covered else None
    within = DeviceBuffer(px) if threshold is not None else None
    counts = DeviceBuffer.zeros(n * 8, stream) if want_counts else None
    nat.check(entry(*_pair_head(near.ptr, far.ptr, dtype, layout, n, c, shape), flow.ptr, fmask.ptr, 1 if flow_shared else 0, sign,
                    _ptr(near_mask), _ptr(far_mask), *settings, np.float32(0) if threshold is None else threshold,
                    _ptr(err), _ptr(covered), _ptr(within), _ptr(counts), quant, stream))
    return err, covered, within, counts


def _pair_error_host(entry, near, far, layout, n, c, vecs, mask, sign, settings, threshold, near_mask, far_mask, quant):
    """the same for their host entries: the result arrays made, the call, and the uint8 maps viewed as bool"""
    vecs, m = np.ascontiguousarray(vecs, np.float32), mask_bytes(mask)
    h, w = vecs.shape[:2]
    err, covered = np.empty((n, h, w), np.float32), np.empty((n, h, w), np.uint8)
    within = np.empty((n, h, w), np.uint8) if threshold is not None else None
    nat.check(entry(*_pair_head(near.ctypes.data, far.ctypes.data, near.dtype.name, layout, n, c, (h, w)), vecs.ctypes.data,
                    m.ctypes.data, 1, sign, _host_ptr(near_mask), _host_ptr(far_mask), *settings,
                    np.float32(0) if threshold is None else threshold, err.ctypes.data, covered.ctypes.data, _host_ptr(within),
                    None, quant))
    res = (err, covered.view(np.bool_))
    return res + (within.view(np.bool_),) if within is not None else res


# ------------------------------------------------------------------------------ K21: photometric error of a warp
def photometric_launch(near, far, dtype, layout, n, c, shape, flow, fmask, flow_shared, sign, metric, eps, threshold=None,
                       near_mask=None, far_mask=None, want_err=True, want_covered=True, want_counts=False,
                       quant=nat.QUANT_OPENCV, stream=None):
    """K21 (ofl_photometric_dev) on `n` items of `c` channels in `layout` ('chw' / 'hwc') of `dtype`: `near` the buffer of the
    field's own frame, `far` that of the other frame; asynchronous, one launch.  flow, fmask, near_mask, far_mask: ONE
    [H][W] each when flow_shared, else n back to back.  metric, eps, threshold: from args.photometric_args (threshold None:
    no `within`).  -> (err or None, covered or None, within or None, counts or None): float32, uint8 and uint8 [n][H][W]
    and the zeroed-then-added uint32 [n][2] = {covered, within} words, all still in HBM."""
    return _pair_error_launch(_lib().ofl_photometric_dev, near, far, dtype, layout, n, c, shape, flow, fmask, flow_shared, sign,
                              (metric, eps), threshold, near_mask, far_mask, want_err, want_covered, want_counts, quant, stream)


def photometric_host(near, far, layout, n, c, vecs, mask, sign, metric, eps, threshold=None, near_mask=None, far_mask=None,
                     quant=nat.QUANT_OPENCV):
    """K21 for host arrays through ofl_photometric (upload, one launch, download): near, far contiguous float32 or float16
    arrays of one dtype in the memory order of `layout`, ONE field (vecs (H, W, 2), mask) and one of each mask (uint8
    (H, W) or None) for all `n` items -> (err float32, covered bool[, within bool]), each (n, H, W)."""
    return _pair_error_host(_lib().ofl_photometric, near, far, layout, n, c, vecs, mask, sign, (metric, eps), threshold,
                            near_mask, far_mask, quant)


# ------------------------------------------------------------------------------ K22: census distance of a warp over a window
def census_launch(near, far, dtype, layout, n, c, shape, flow, fmask, flow_shared, sign, window, mode, p0, p1, min_count,
                  threshold=None, near_mask=None, far_mask=None, want_err=True, want_covered=True, want_counts=False,
                  quant=nat.QUANT_OPENCV, stream=None):
    """K22 (ofl_census_dev) on `n` items of `c` channels (1 to 4) in `layout` ('chw' / 'hwc') of `dtype`; buffers and the
    shared or per-item field and masks as in photometric_launch; asynchronous, one launch.  window, mode, p0, p1, min_count,
    threshold: from args.census_args (threshold None: no `within`).  -> (err or None, covered or None, within or None,
    counts or None): float32, uint8 and uint8 [n][H][W] and the zeroed-then-added uint32 [n][2] = {covered, within} words,
    all still in HBM."""
    return _pair_error_launch(_lib().ofl_census_dev, near, far, dtype, layout, n, c, shape, flow, fmask, flow_shared, sign,
                              (window, mode, p0, p1, min_count), threshold, near_mask, far_mask, want_err, want_covered,
                              want_counts, quant, stream)


def census_host(near, far, layout, n, c, vecs, mask, sign, window, mode, p0, p1, min_count, threshold=None, near_mask=None,
                far_mask=None, quant=nat.QUANT_OPENCV):
    """K22 for host arrays through ofl_census (upload, one launch, download): arrays, field and masks as in
    photometric_host -> (err float32, covered bool[, within bool]), each (n, H, W)."""
    return _pair_error_host(_lib().ofl_census, near, far, layout, n, c, vecs, mask, sign, (window, mode, p0, p1, min_count),
                            threshold, near_mask, far_mask, quant)


# ------------------------------------------------------------------------------ K26: structural similarity of a warp over a window
def ssim_launch(near, far, dtype, layout, n, c, shape, flow, fmask, flow_shared, sign, window, taps, c1, c2, min_count,
                threshold=None, near_mask=None, far_mask=None, want_err=True, want_covered=True, want_counts=False,
                quant=nat.QUANT_OPENCV, stream=None):
    """K26 (ofl_ssim_dev) on `n` items of `c` channels (1 to 4) in `layout` ('chw' / 'hwc') of `dtype`; buffers and the
    shared or per-item field and masks as in photometric_launch; asynchronous, one launch.  window, taps, c1, c2, min_count,
    threshold: from args.ssim_args (taps: the float32 array of the 1-D window, read by the entry during the call; threshold
    None: no `within`).  -> (err or None, covered or None, within or None, counts or None): float32, uint8 and uint8
    [n][H][W] and the zeroed-then-added uint32 [n][2] = {covered, within} words, all still in HBM."""
    taps = np.ascontiguousarray(taps, np.float32)               # alive until the entry has returned
    return _pair_error_launch(_lib().ofl_ssim_dev, near, far, dtype, layout, n, c, shape, flow, fmask, flow_shared, sign,
                              (window, taps.ctypes.data, c1, c2, min_count), threshold, near_mask, far_mask, want_err, want_covered,
                              want_counts, quant, stream)


def ssim_host(near, far, layout, n, c, vecs, mask, sign, window, taps, c1, c2, min_count, threshold=None, near_mask=None,
              far_mask=None, quant=nat.QUANT_OPENCV):
    """K26 for host arrays through ofl_ssim (upload, one launch, download): arrays, field and masks as in
    photometric_host -> (err float32, covered bool[, within bool]), each (n, H, W)."""
    taps = np.ascontiguousarray(taps, np.float32)
    return _pair_error_host(_lib().ofl_ssim, near, far, layout, n, c, vecs, mask, sign, (window, taps.ctypes.data, c1, c2, min_count),
                            threshold, near_mask, far_mask, quant)


# ------------------------------------------------------------------------------ K23: variational refinement of a field
def refine_launch(near, far, dtype, layout, n, c, shape, flow, fmask, sign, alpha, delta, zeta, eps, fixed_point, sor, omega,
                  near_mask=None, far_mask=None, valid=None, want_data=False, quant=nat.QUANT_OPENCV, stream=None):
    """K23 (ofl_refine_dev) on `n` items of `c` channels (1 to 4) in `layout` ('chw' / 'hwc') of `dtype`, item i with field i:
    flow, fmask, near_mask, far_mask, valid lie back to back, [n][H][W]; asynchronous: setup, fixed_point * (1 + 2 * sor)
    solver launches, finish.  alpha ... omega: from args.refine_args.  The workspace comes from the buffer pool and goes back
    to it on return (one stream).  -> (vecs float32 [n][H][W][2], data uint8 [n][H][W] or None), still in HBM."""
    lib, (h, w) = _lib(), shape
    nbytes = _size_query(lib.ofl_refine_workspace_bytes, n, h, w)
    work = DeviceBuffer(nbytes)
    out = DeviceBuffer(n * h * w * 8)
    data = DeviceBuffer(n * h * w) if want_data else None
    nat.check(lib.ofl_refine_dev(*_pair_head(near.ptr, far.ptr, dtype, layout, n, c, shape), flow.ptr, fmask.ptr, sign,
                                 _ptr(near_mask), _ptr(far_mask), _ptr(valid), alpha, delta, zeta, eps, fixed_point, sor, omega,
                                 work.ptr, nbytes, out.ptr, _ptr(data), quant, stream))
    return out, data


def refine_host(near, far, layout, n, c, vecs, mask, sign, alpha, delta, zeta, eps, fixed_point, sor, omega, near_mask=None,
                far_mask=None, valid=None, want_data=False, quant=nat.QUANT_OPENCV):
    """K23 for host arrays through ofl_refine (upload, launches, download): near, far as in photometric_host, vecs
    (n, H, W, 2) or (H, W, 2) with n = 1, and the masks uint8 of n * H * W bytes or None -> (vecs float32 (n, H, W, 2),
    data bool (n, H, W) or None)."""
    vecs, m = np.ascontiguousarray(vecs, np.float32), mask_bytes(mask)
    h, w = vecs.shape[-3:-1]
    out = np.empty((n, h, w, 2), np.float32)
    data = np.empty((n, h, w), np.uint8) if want_data else None
    nat.check(_lib().ofl_refine(*_pair_head(near.ctypes.data, far.ctypes.data, near.dtype.name, layout, n, c, (h, w)),
                                vecs.ctypes.data, m.ctypes.data, sign, _host_ptr(near_mask), _host_ptr(far_mask),
                                _host_ptr(valid), alpha, delta, zeta, eps, fixed_point, sor, omega,
                                out.ctypes.data, _host_ptr(data), quant))
    return out, None if data is None else data.view(np.bool_)


# ------------------------------------------------------------------------------ K24: dense inverse search of a field
def inverse_search_launch(near, far, dtype, layout, n, c, shape, flow, fmask, sign, patch, stride, iterations, normalise, floor,
                          want_patches=False, quant=nat.QUANT_EXACT, stream=None):
    """K24 (ofl_inverse_search_dev) on `n` items of `c` channels (1 to 4) in `layout` ('chw' / 'hwc') of `dtype`, item i with
    field i: flow and fmask lie back to back, [n][H][W], or are None (the zero field); asynchronous: setup, search, densify.
    patch ... floor: from args.inverse_search_args.  The workspace comes from the buffer pool and goes back to it on return
    (one stream).  -> (vecs float32 [n][H][W][2], mask uint8 [n][H][W], patch_vecs float32 [n][ny][nx][2] or None, patch_ssd
    float32 [n][ny][nx] or None, (ny, nx)), still in HBM."""
    lib, (h, w) = _lib(), shape
    ny, nx = len(patch_origins(h, patch, stride)), len(patch_origins(w, patch, stride))
    nbytes = _size_query(lib.ofl_inverse_search_workspace_bytes, n, h, w, patch, stride)
    work = DeviceBuffer(nbytes)
    out, mask = DeviceBuffer(n * h * w * 8), DeviceBuffer(n * h * w)
    pv = DeviceBuffer(n * ny * nx * 8) if want_patches else None
    ps = DeviceBuffer(n * ny * nx * 4) if want_patches else None
    nat.check(lib.ofl_inverse_search_dev(*_pair_head(near.ptr, far.ptr, dtype, layout, n, c, shape), _ptr(flow),
                                         _ptr(fmask), sign, patch, stride, iterations, 1 if normalise else 0, floor,
                                         work.ptr, nbytes, out.ptr, mask.ptr, _ptr(pv), _ptr(ps), quant, stream))
    return out, mask, pv, ps, (ny, nx)


def inverse_search_host(near, far, layout, n, c, vecs, mask, sign, patch, stride, iterations, normalise, floor,
                        want_patches=False, quant=nat.QUANT_EXACT):
    """K24 for host arrays through ofl_inverse_search (upload, launches, download): near, far as in photometric_host, vecs
    (n, H, W, 2) or (H, W, 2) with n = 1 -> (vecs float32 (n, H, W, 2), mask bool (n, H, W), patch_vecs float32
    (n, ny, nx, 2) or None, patch_ssd float32 (n, ny, nx) or None, (ny, nx))."""
    vecs, m = np.ascontiguousarray(vecs, np.float32), mask_bytes(mask)
    h, w = vecs.shape[-3:-1]
    ny, nx = len(patch_origins(h, patch, stride)), len(patch_origins(w, patch, stride))
    out, om = np.empty((n, h, w, 2), np.float32), np.empty((n, h, w), np.uint8)
    pv = np.empty((n, ny, nx, 2), np.float32) if want_patches else None
    ps = np.empty((n, ny, nx), np.float32) if want_patches else None
    nat.check(_lib().ofl_inverse_search(*_pair_head(near.ctypes.data, far.ctypes.data, near.dtype.name, layout, n, c, (h, w)),
                                        vecs.ctypes.data, m.ctypes.data, sign, patch, stride, iterations,
                                        1 if normalise else 0, floor, out.ctypes.data, om.ctypes.data, _host_ptr(pv), _host_ptr(ps), quant))
    return out, om.view(np.bool_), pv, ps, (ny, nx)


# ------------------------------------------------------------------------------ K25: a sequence of fields accumulated into one
def sequence_launch(vecs, mask, sign, shape, length, n_seq=1, want_partials=False, want_lost_at=False, quant=nat.QUANT_OPENCV,
                    stream=None):
    """K25 (ofl_compose_sequence_dev) on `n_seq` sequences of `length` fields each, stored back to back; asynchronous, one
    launch.  -> (out_vecs, out_mask, part_vecs or None, part_masks or None, lost_at or None): float32 [n_seq][H][W][2] and
    uint8 [n_seq][H][W], the partial results float32 [n_seq][length][H][W][2] and uint8 [n_seq][length][H][W], and int32
    [n_seq][H][W], all still in HBM."""
    px = n_seq * shape[0] * shape[1]
    out, mout = DeviceBuffer(px * 8), DeviceBuffer(px)
    pv = DeviceBuffer(px * length * 8) if want_partials else None
    pm = DeviceBuffer(px * length) if want_partials else None
    lost = DeviceBuffer(px * 4) if want_lost_at else None
    nat.check(_lib().ofl_compose_sequence_dev(vecs.ptr, mask.ptr, sign, shape[0], shape[1], length, n_seq, out.ptr, mout.ptr,
                                              _ptr(pv), _ptr(pm), _ptr(lost), quant, stream))
    return out, mout, pv, pm, lost


def sequence_host(vecs, masks, sign, want_partials=False, want_lost_at=False, quant=nat.QUANT_OPENCV):
    """K25 for host arrays through ofl_compose_sequence (upload, one launch, download): vecs (L, H, W, 2), masks (L, H, W),
    ONE sequence -> (vecs float32 (H, W, 2), mask bool (H, W), part_vecs float32 (L, H, W, 2) or None, part_masks bool
    (L, H, W) or None, lost_at int32 (H, W) or None)."""
    vecs, m = np.ascontiguousarray(vecs, np.float32), mask_bytes(masks)
    length, h, w = vecs.shape[:3]
    out, mout = np.empty((h, w, 2), np.float32), np.empty((h, w), np.uint8)
    pv = np.empty((length, h, w, 2), np.float32) if want_partials else None
    pm = np.empty((length, h, w), np.uint8) if want_partials else None
    lost = np.empty((h, w), np.int32) if want_lost_at else None
    nat.check(_lib().ofl_compose_sequence(vecs.ctypes.data, m.ctypes.data, sign, h, w, length, 1, out.ctypes.data,
                                          mout.ctypes.data, _host_ptr(pv), _host_ptr(pm), _host_ptr(lost), quant))
    return out, mout.view(np.bool_), pv, None if pm is None else pm.view(np.bool_), lost
