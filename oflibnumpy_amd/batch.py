"""Batches of independent flow-field pairs (BASELINE.json config 4): one device launch per stack.

`DeviceFlowBatch` keeps B fields of one shape back to back in HBM ([B][H][W][2] float32 + [B][H][W] uint8),
the layout `ofl_compose3_dev` takes with `batch > 1`.  `combine_flows_batch` is the array-level convenience:
it composes the pairs this rank owns (`sharding.shard`) with mode 3 in one launch and honours the
reference's per-pair zero-flow early exits (flow_class.py:1339-1354) from the flag words of that launch.
"""
import numpy as np

from . import _native as nat
from . import device as dev
from . import sharding
from .flow_class import Flow


class DeviceFlowBatch:
    def __init__(self, n, shape, ref, packed=False):
        """packed: the masks live as bit planes (`self.bits`, include/ofl.h: ofl_compose3_bits_dev) instead of bytes -- for chains
        of compositions that stay on the device; `mask` is then produced on demand (unpack)."""
        self.n, self.shape, self.ref = int(n), (int(shape[0]), int(shape[1])), ref
        px = self.shape[0] * self.shape[1]
        self.vecs = dev.DeviceBuffer(self.n * px * 8)
        self.packed = bool(packed)
        if self.packed:
            self.bits = dev.DeviceBuffer(dev.mask_bits_bytes(self.shape[0], self.shape[1], self.n))
            self._mask = None
        else:
            self.bits = None
            self._mask = dev.DeviceBuffer(self.n * px)

    @property
    def mask(self):
        if self._mask is None:
            self._mask = dev.mask_unpack(self.bits, self.shape[0], self.shape[1], self.n)
        return self._mask

    @classmethod
    def wrap(cls, n, shape, ref, vecs, mask, bits=None):
        """A batch on existing buffers: `vecs` and the byte masks `mask`, plus -- `bits` given -- their packed bit planes."""
        b = cls.__new__(cls)
        b.n, b.shape, b.ref, b.vecs, b.packed, b.bits, b._mask = n, shape, ref, vecs, bits is not None, bits, mask
        return b

    def pack(self):
        """the same fields with their masks as bit planes (a copy of the masks only; the vectors are shared)"""
        if self.packed:
            return self
        bits = dev.mask_pack(self._mask, self.shape[0], self.shape[1], self.n)
        return DeviceFlowBatch.wrap(self.n, self.shape, self.ref, self.vecs, self._mask, bits)

    @classmethod
    def from_flows(cls, flows, packed=False):
        flows = list(flows)
        if not flows:
            raise ValueError("empty batch")
        shape, ref = flows[0].shape, flows[0].ref
        if any(f.shape != shape or f.ref != ref for f in flows):
            raise ValueError("all flows of a batch need the same shape and reference")
        b = cls(len(flows), shape, ref)
        px = shape[0] * shape[1]
        lib = nat.load()
        for i, f in enumerate(flows):
            m = dev.mask_bytes(f.mask)
            v = np.ascontiguousarray(f.vecs, np.float32)       # Flow.vecs keeps the layout of its input (astype order 'K')
            nat.check(lib.ofl_upload(b.vecs.ptr + i * px * 8, v.ctypes.data, px * 8, None))
            nat.check(lib.ofl_upload(b.mask.ptr + i * px, m.ctypes.data, px, None))
            nat.check(lib.ofl_stream_sync(None))
        return b.pack() if packed else b

    @classmethod
    def from_matrices(cls, matrices, shape, ref=None):
        """n fields from n transformation matrices ((n, 3, 3), taken as float64), built in HBM: n * 72 bytes go up and ONE
        launch of the constructor kernel writes all fields -- field i is DeviceFlow.from_matrix(matrices[i], shape, ref) bit
        for bit.  Every mask is all valid."""
        if not isinstance(matrices, np.ndarray):
            raise TypeError("Error creating flows from matrices: Matrices need to be a numpy array")
        if matrices.ndim != 3 or matrices.shape[0] == 0 or matrices.shape[1:] != (3, 3):
            raise ValueError("Error creating flows from matrices: Matrices need to be a numpy array of shape (n, 3, 3), n > 0")
        args = [dev.matrix_args(m, shape, ref) for m in matrices]
        sign, ref = args[0][1], args[0][2]
        b = cls(len(args), shape, ref)
        dev.flow_from_matrix_launch(dev.DeviceBuffer.from_host(np.stack([a[0] for a in args])), b.n, sign, b.shape, b.vecs)
        nat.check(nat.load().ofl_memset(b.mask.ptr, 1, b.n * b.shape[0] * b.shape[1], None))
        return b

    @classmethod
    def from_external(cls, vecs, ref, masks=None, layout=None, dtype=None, stream=None, check_finite=True):
        """n fields another framework holds in device memory -- a network's output -- in ONE launch and without crossing
        PCIe: `vecs.__cuda_array_interface__` describes (N, H, W, 2) ('hwc') or (N, 2, H, W) ('chw'); element types, strides,
        `layout`, `dtype`, `stream`, `check_finite` and the errors as in DeviceFlow.from_external.  `masks`: such an object
        (N, H, W) of bool or uint8, a DeviceBuffer of N * H * W bytes, or None (all valid).  Always a copy."""
        from .utils import get_valid_ref
        ref = get_valid_ref(ref)
        v, m, n, shape = dev.import_flow(vecs, masks, layout, dtype, stream, True, check_finite, batch=True)
        return cls.wrap(n, shape, ref, v, m)

    def export(self, layout='hwc', dtype='float32', copy=True):
        """The vectors of all fields as ONE DeviceArray: (N, H, W, 2) for 'hwc', (N, 2, H, W) for 'chw', of float32, float16
        or bfloat16 (as int16) -- see DeviceFlow.export, also for copy=False."""
        return dev.export_flow(self.vecs, self.n, self.shape, layout, dtype, copy, self, batch=True)

    def export_masks(self, copy=True):
        """The masks as a DeviceArray of bool, (N, H, W); copy=False: a view of the batch's own masks, not to be written."""
        return dev.export_mask(self.mask, (self.n,) + self.shape, copy, self)

    def to_flows(self):
        h, w = self.shape
        v = self.vecs.to_host((self.n, h, w, 2), np.float32)
        m = self.mask.to_host((self.n, h, w), np.uint8).view(np.bool_)
        return [Flow(v[i], self.ref, m[i]) for i in range(self.n)]

    def compose3(self, other, quant=nat.QUANT_OPENCV):
        """self[i].combine_with(other[i], mode=3) for every i in ONE launch.
        Returns (DeviceFlowBatch out, flag words uint32 [n][8]) -- see ofl_compose3_dev for the words.  Two PACKED batches
        compose on their bit planes (ofl_compose3_bits_dev) and give a packed result: the same fields, bit for bit."""
        if (self.n, self.shape, self.ref) != (other.n, other.shape, other.ref):
            raise ValueError("batches need the same length, shape and reference")
        fa, fb, sign = (other, self, +1) if self.ref == 's' else (self, other, -1)
        words = dev.DeviceBuffer.zeros(32 * self.n)
        if self.packed and other.packed and quant == nat.QUANT_OPENCV and self.shape[1] % 2 == 0:
            out = DeviceFlowBatch(self.n, self.shape, self.ref, packed=True)
            dev.compose3_bits_launch(fa.vecs, fa.bits, fb.vecs, fb.bits, sign, self.shape, out.vecs, out.bits, words, batch=self.n)
        else:
            out = DeviceFlowBatch(self.n, self.shape, self.ref)
            dev.compose3_launch(fa, fb, sign, out, words, batch=self.n, quant=quant)
        return out, words.to_host((self.n, 8), np.uint32), (fa, fb)

    def consistency(self, backward, alpha=None, beta=None, return_residual=False, return_counts=False, quant=nat.QUANT_OPENCV):
        """self[i].consistency(backward[i], ...) for every i in ONE launch of K13 (DeviceFlow.consistency): `backward` a batch
        of the same length, shape and reference.  -> (consistent, covered) as uint8 DeviceBuffers [n][H][W]; return_residual
        appends the float32 DeviceBuffer [n][H][W], return_counts an (n, 2) uint32 array of (covered, consistent) pixels per
        pair -- the only option that synchronises.  A packed batch is read through its byte masks (`.mask` unpacks on
        demand)."""
        alpha, beta = dev.consistency_args(alpha, beta)
        if not isinstance(backward, DeviceFlowBatch):
            raise TypeError("Error checking flow consistency: backward needs to be a DeviceFlowBatch, got {}".format(type(backward).__name__))
        if (self.n, self.shape, self.ref) != (backward.n, backward.shape, backward.ref):
            raise ValueError("batches need the same length, shape and reference")
        consistent, covered, residual, counts = dev.consistency_launch(
            self.vecs, self.mask, backward.vecs, backward.mask, 1 if self.ref == 's' else -1, self.shape, alpha, beta,
            batch=self.n, want_residual=return_residual, want_counts=return_counts, quant=quant)
        res = (consistent, covered) + ((residual,) if return_residual else ())
        return res + (counts.to_host((self.n, 2), np.uint32),) if return_counts else res

    def photometric(self, near, far, metric='l1', eps=None, threshold=None, near_mask=None, far_mask=None, return_counts=False,
                    quant=nat.QUANT_OPENCV):
        """self[i].photometric(item i of `near`, item i of `far`, ...) for every i in ONE launch of K21
        (DeviceFlow.photometric): near, far DeviceTensors (n, C, H, W) of one layout and dtype, near_mask, far_mask uint8
        DeviceBuffers [n][H][W] (per item) or None.  -> (error float32, covered uint8) as DeviceBuffers [n][H][W];
        `threshold` appends within (uint8), return_counts an (n, 2) uint32 array of (covered, within) pixels per item -- the
        only option that synchronises.  A packed batch is read through its byte masks."""
        res, counts, _ = dev.error_map_op(dev.photometric_launch, dev.photometric_args(metric, eps, threshold), None,
                                          "Error computing photometric error: ", self.vecs, self.mask, self.shape, self.ref,
                                          near, far, near_mask, far_mask, return_counts, quant, batch=self.n)
        return res + (counts.to_host((self.n, 2), np.uint32),) if return_counts else res

    def census(self, near, far, window=7, mode='soft', delta=None, noise=None, knee=None, min_count=None, threshold=None,
               near_mask=None, far_mask=None, return_counts=False, quant=nat.QUANT_OPENCV):
        """self[i].census(item i of `near`, item i of `far`, ...) for every i in ONE launch of K22 (DeviceFlow.census):
        near, far DeviceTensors (n, C, H, W) of one layout and dtype with 1 to 4 channels, near_mask, far_mask uint8
        DeviceBuffers [n][H][W] (per item) or None.  -> (error float32, covered uint8) as DeviceBuffers [n][H][W];
        `threshold` appends within (uint8), return_counts an (n, 2) uint32 array of (covered, within) pixels per item -- the
        only option that synchronises.  A packed batch is read through its byte masks."""
        res, counts, _ = dev.error_map_op(dev.census_launch, dev.census_args(window, mode, delta, noise, knee, min_count, threshold),
                                          nat.CENSUS_MAX_C, "Error computing census distance: ", self.vecs, self.mask, self.shape,
                                          self.ref, near, far, near_mask, far_mask, return_counts, quant, batch=self.n)
        return res + (counts.to_host((self.n, 2), np.uint32),) if return_counts else res

    def ssim(self, near, far, window=11, weights='gaussian', sigma=None, data_range=255.0, k1=0.01, k2=0.03, min_count=None,
             threshold=None, near_mask=None, far_mask=None, return_counts=False, quant=nat.QUANT_OPENCV):
        """self[i].ssim(item i of `near`, item i of `far`, ...) for every i in ONE launch of K26 (DeviceFlow.ssim):
        near, far DeviceTensors (n, C, H, W) of one layout and dtype with 1 to 4 channels, near_mask, far_mask uint8
        DeviceBuffers [n][H][W] (per item) or None.  -> (error float32, covered uint8) as DeviceBuffers [n][H][W], error
        the dissimilarity (1 - SSIM) / 2; `threshold` appends within (uint8), return_counts an (n, 2) uint32 array of
        (covered, within) pixels per item -- the only option that synchronises.  A packed batch is read through its byte
        masks."""
        res, counts, _ = dev.error_map_op(dev.ssim_launch, dev.ssim_args(window, weights, sigma, data_range, k1, k2, min_count, threshold),
                                          nat.SSIM_MAX_C, "Error computing structural similarity: ", self.vecs, self.mask, self.shape,
                                          self.ref, near, far, near_mask, far_mask, return_counts, quant, batch=self.n)
        return res + (counts.to_host((self.n, 2), np.uint32),) if return_counts else res

    def refine(self, near, far, alpha=None, delta=None, zeta=None, eps=None, fixed_point=None, sor=None, omega=None,
               near_mask=None, far_mask=None, valid=None, return_data=False, quant=nat.QUANT_OPENCV):
        """self[i].refine(item i of `near`, item i of `far`, ...) for every i in the SAME launches of K23
        (DeviceFlow.refine): near, far DeviceTensors (n, C, H, W) of one layout and dtype with 1 to 4 channels, near_mask,
        far_mask, valid uint8 DeviceBuffers [n][H][W] (per item) or None.  -> an unpacked DeviceFlowBatch of the same
        length, shape, reference and masks; return_data appends the uint8 DeviceBuffer [n][H][W].  A packed batch is read
        through its byte masks.  Nothing synchronises."""
        out, data = dev.refine_op(dev.refine_args(alpha, delta, zeta, eps, fixed_point, sor, omega), self.vecs, self.mask,
                                  self.shape, self.ref, near, far, near_mask, far_mask, valid, return_data, quant, batch=self.n)
        b = DeviceFlowBatch.wrap(self.n, self.shape, self.ref, out, self.mask)
        return (b, data) if return_data else b

    def inverse_search(self, near, far, patch=8, stride=4, iterations=12, normalise=True, floor=1.0, return_patches=False,
                       quant=nat.QUANT_EXACT):
        """self[i].inverse_search(item i of `near`, item i of `far`, ...) for every i in the SAME launches of K24
        (DeviceFlow.inverse_search): near, far DeviceTensors (n, C, H, W) of one layout and dtype with 1 to 4 channels.
        -> an unpacked DeviceFlowBatch of the same length, shape and reference whose masks are K24's out_mask;
        return_patches appends (patch_vecs float32 DeviceBuffer [n][ny][nx][2], patch_ssd float32 DeviceBuffer [n][ny][nx],
        (ny, nx)).  A packed batch is read through its byte masks.  Nothing synchronises."""
        out, mask, pv, ps, grid = dev.inverse_search_op(dev.inverse_search_args(patch, stride, iterations, normalise, floor),
                                                        self.vecs, self.mask, self.shape, self.ref, near, far, return_patches,
                                                        quant, batch=self.n)
        b = DeviceFlowBatch.wrap(self.n, self.shape, self.ref, out, mask)
        return (b, pv, ps, grid) if return_patches else b

    def combine_sequence(self, length=None, quant=nat.QUANT_OPENCV, return_partials=False, return_lost_at=False):
        """The batch as a SEQUENCE -- field k maps frame k to frame k + 1 -- accumulated into one long-range field in ONE
        launch of K25 (ofl_compose_sequence_dev): per pixel a walk through the fields with the accumulated vector in
        registers, mode 3 of combine_with folded over the sequence, bit for bit,
            ref 's':  F <- F.combine_with(f_k, 3)  for k = 1 ... n - 1
            ref 't':  G <- f_k.combine_with(G, 3)  for k = n - 2 ... 0
        without the zero-flow early exits (as in consistency).  For 't' this right fold is the only association that is a
        per-pixel walk; the left fold, ((f_0 (+) f_1) (+) f_2) ..., interpolates the accumulated field and is NOT what this
        computes.  length: None -- the whole batch is one sequence, the result a DeviceFlow -- or a divisor of n: n / length
        sequences of `length` consecutive fields each, the result an unpacked DeviceFlowBatch of n / length fields.
        return_partials appends an unpacked DeviceFlowBatch of n fields, the accumulated field after each step at the index of
        the field taken last ('s': entry k composes fields 0 ... k of its sequence; 't': entry k composes fields k ...
        length - 1); return_lost_at an int32 DeviceBuffer [n / length][H][W], the index within its sequence of the field at
        which the pixel's mask first became 0, -1 where it is still set at the end.  A packed batch is read through its byte
        masks.  Nothing synchronises."""
        whole = length is None
        length, n_seq, quant, return_partials, return_lost_at = dev.sequence_args(self.n, length, quant, return_partials, return_lost_at)
        out, mout, pv, pm, lost = dev.sequence_launch(self.vecs, self.mask, 1 if self.ref == 's' else -1, self.shape, length, n_seq,
                                                      want_partials=return_partials, want_lost_at=return_lost_at, quant=quant)
        res = dev.DeviceFlow(out, mout, self.shape, self.ref) if whole else DeviceFlowBatch.wrap(n_seq, self.shape, self.ref, out, mout)
        extra = ((DeviceFlowBatch.wrap(self.n, self.shape, self.ref, pv, pm),) if return_partials else ()) + \
                ((lost,) if return_lost_at else ())
        return (res,) + extra if extra else res

    def error(self, gt, thresholds=None, outlier=None, speed_edges=None, use_est_mask=True, return_map=False, return_outliers=False):
        """self[i].error(gt[i], ...) for every i in ONE launch of K14 (DeviceFlow.error): `gt` a batch of the same length,
        shape and reference.  -> a DeviceFlowError whose read() gives a list of n FlowErrorStats (the one read-back, 96 bytes
        per pair) and whose maps, if asked for, are [n][H][W].  A packed batch is read through its byte masks."""
        thr, out, edges, n_thr, n_edges = dev.error_args(thresholds, outlier, speed_edges)
        if not isinstance(gt, DeviceFlowBatch):
            raise TypeError("Error evaluating flow error: gt needs to be a DeviceFlowBatch, got {}".format(type(gt).__name__))
        if (self.n, self.shape, self.ref) != (gt.n, gt.shape, gt.ref):
            raise ValueError("batches need the same length, shape and reference")
        records, epe_map, outlier_map = dev.error_launch(self.vecs, self.mask if use_est_mask else None, gt.vecs, gt.mask, self.shape,
                                                         thr, out, edges, batch=self.n, want_map=return_map, want_outliers=return_outliers)
        return dev.DeviceFlowError(records, self.n, n_thr, n_edges, epe_map, outlier_map)

    def fill(self, valid=None, max_dist=None, return_index=False, return_d2=False):
        """self[i].fill(valid[i], ...) for every i in ONE pair of launches of K15 (DeviceFlow.fill): `valid` a uint8
        DeviceBuffer of n * H * W bytes or None.  -> an unpacked DeviceFlowBatch of the same length, shape and reference,
        plus, on request, the int32 index and the uint32 squared distance as DeviceBuffers [n][H][W]; an index counts
        within its own field.  A packed batch is read through its byte masks.  Nothing synchronises."""
        max_d2 = dev.fill_args(max_dist)
        valid = dev.mask_buffer_arg(valid, self.n * self.shape[0] * self.shape[1], "Error filling flow: ", "valid")
        out_vecs, out_mask, index, d2 = dev.fill_launch(self.vecs, self.mask, valid, self.shape, max_d2, batch=self.n,
                                                        want_index=bool(return_index), want_d2=bool(return_d2))
        b = DeviceFlowBatch.wrap(self.n, self.shape, self.ref, out_vecs, out_mask)
        extra = ((index,) if return_index else ()) + ((d2,) if return_d2 else ())
        return (b,) + extra if extra else b

    def median(self, ksize=5, valid=None, only=None, min_count=None):
        """self[i].median(ksize, valid[i], only[i], min_count) for every i in ONE launch of K16 (DeviceFlow.median): `valid`
        and `only` uint8 DeviceBuffers of n * H * W bytes or None; a window never crosses from one field into the next.
        -> an unpacked DeviceFlowBatch of the same length, shape and reference.  A packed batch is read through its byte
        masks.  Nothing synchronises."""
        ksize, min_count = dev.median_args(ksize, min_count)
        n_bytes = self.n * self.shape[0] * self.shape[1]
        valid = dev.mask_buffer_arg(valid, n_bytes, "Error filtering flow: ", "valid")
        only = dev.mask_buffer_arg(only, n_bytes, "Error filtering flow: ", "only")
        out_vecs, out_mask = dev.median_launch(self.vecs, self.mask, valid, only, self.shape, ksize, min_count, batch=self.n)
        return DeviceFlowBatch.wrap(self.n, self.shape, self.ref, out_vecs, out_mask)

    def upsample_convex(self, weights, factor=8):
        """self[i].upsample_convex(weights[i], factor) for every i in ONE launch of K17 (DeviceFlow.upsample_convex):
        `weights` a DeviceTensor of logical shape (n, 9 f^2, h, w) in either layout.  -> an unpacked DeviceFlowBatch of the
        same length and reference and of shape (f h, f w).  A packed batch is read through its byte masks.  Nothing
        synchronises."""
        factor = dev.upsample_weights(weights, factor, self.shape, batch=self.n)
        out_vecs, out_mask = dev.upsample_launch(self.vecs, self.mask, weights.buf, weights.dtype, weights.layout, self.shape,
                                                 factor, batch=self.n)
        return DeviceFlowBatch.wrap(self.n, (factor * self.shape[0], factor * self.shape[1]), self.ref, out_vecs, out_mask)

    def splat(self, tensor, mode='average', importance=None, alpha=1.0, min_weight=None, frac_bits=None, return_weight=False,
              return_counters=False):
        """self[i].splat(item i of `tensor`, ...) for every i in ONE set of launches of K20 (DeviceFlow.splat; ref 's'
        batches): `tensor` a DeviceTensor (n, C, H, W) in either layout, `importance` a float32 DeviceBuffer [n][H][W] or
        None.  -> (DeviceTensor, valid uint8 DeviceBuffer [n][H][W]); return_weight appends the float32 DeviceBuffer
        [n][H][W], return_counters (skipped source pixels, dropped values) summed over the batch as Python ints -- the only
        option that synchronises.  A packed batch is read through its byte masks."""
        if self.ref != 's':
            raise ValueError("Error splatting: splat pushes values forward along 's'-reference fields; 't'-reference fields "
                             "warp backward, with apply_tensors")
        if not isinstance(tensor, dev.DeviceTensor):
            raise TypeError("Error splatting: tensor needs to be a DeviceTensor, got {}".format(type(tensor).__name__))
        code, alpha, min_weight, frac_bits = dev.splat_args(mode, importance is not None, alpha, min_weight, frac_bits)
        n, c, h, w, batched = dev.tensor_args(tensor.shape, tensor.layout, tensor.dtype, self.shape)
        if not batched or n != self.n:
            raise ValueError("Error splatting: a batch of {} fields takes a tensor of shape ({}, C, H, W), got {}"
                             .format(self.n, self.n, tensor.shape))
        z = dev.splat_importance(importance, self.n * h * w)
        dst, valid, weight, counters = dev.splat_launch(tensor.buf, tensor.dtype, tensor.layout, n, c, self.shape, self.vecs,
                                                        self.mask, False, code, alpha, min_weight, frac_bits, z=z,
                                                        want_weight=bool(return_weight), want_counters=bool(return_counters))
        res = (dev.DeviceTensor(dst, tensor.shape, tensor.dtype, tensor.layout), valid) + ((weight,) if return_weight else ())
        if return_counters:
            k = counters.to_host((2,), np.uint32)
            res += ((int(k[0]), int(k[1])),)
        return res

    def apply_images(self, images, dtype, channels, shared=False, target_masks=None, shared_masks=False, quant=nat.QUANT_OPENCV):
        """self[i].apply(image_i, target_mask_i, return_valid_area=True) for every i in ONE launch of the gather kernel
        (ref 't' batches; Flow.apply, flow_class.py:604-695 without padding).  `images`: a DeviceBuffer holding [n][H][W][C] of
        `dtype` back to back -- or ONE [H][W][C] image warped by every field when `shared`; `target_masks` uint8 [n][H][W] (one
        [H][W] when `shared_masks`) or None.  Returns (warped [n][H][W][C] DeviceBuffer, valid [n][H][W] DeviceBuffer), field
        for field what DeviceFlow.apply_image gives (the dtype rules of the reference's concatenated array, args.remap_rules).
        A field whose vectors are all below the 1e-3 threshold is warped like any other: under cv2's 1/32-px coordinate
        snapping that IS the identity of utils.py:215-216."""
        if self.ref != 't':
            raise ValueError("apply_images batches the gather ('t') warp; 's' fields go through DeviceFlow.apply_image one by one")
        dtype = np.dtype(dtype)
        h, w = self.shape
        arith, rule = dev.remap_rules(dtype, target_masks is not None)
        return dev.gather_bilinear_batch(images, dtype, channels, h, w, self.n, self.vecs, -1, smask=target_masks, fmask=self.mask,
                                         valid=True, shared_src=shared, shared_smask=shared_masks, quant=quant, arith=arith, rule=rule)

    def apply_tensors(self, tensor, target_masks=None, shared_masks=False, quant=nat.QUANT_OPENCV):
        """self[i].apply_tensor(item i of `tensor`, target_mask_i) for every i in ONE launch of K12 (ref 't' batches):
        `tensor` a DeviceTensor (n, C, H, W) in either layout, `target_masks` uint8 [n][H][W] (one [H][W] when
        `shared_masks`) or None.  Returns (DeviceTensor, valid [n][H][W] DeviceBuffer).  Like apply_images this takes no
        zero-flow short cut -- a field below the 1e-3 threshold is warped like any other, which under cv2's 1/32-px coordinate
        snapping IS the identity of utils.py:215-216, value for value (a -0.0 comes back as +0.0, as from the image gather) -- and so only `quant=QUANT_OPENCV` is accepted: without the snapping
        the warp of such a field would not be the identity the single call returns."""
        if self.ref != 't':
            raise ValueError("apply_tensors batches the gather ('t') warp: 's'-reference (scatter) warps of tensors are not supported")
        if quant != nat.QUANT_OPENCV:
            raise ValueError("apply_tensors takes no zero-flow short cut and is the reference's warp under quant=QUANT_OPENCV only; "
                             "use DeviceFlow.apply_tensor field by field (field(i)) for QUANT_EXACT")
        n, c, h, w, batched = dev.tensor_args(tensor.shape, tensor.layout, tensor.dtype, self.shape)
        if not batched or n != self.n:
            raise ValueError("apply_tensors needs a tensor of shape (n, C, H, W) with one item per field, got {} for {} fields"
                             .format(tensor.shape, self.n))
        dst, valid = dev.gather_tensor(tensor.buf, tensor.dtype, tensor.layout, n, c, h, w, self.vecs, False, -1,
                                       smask=target_masks, smask_shared=shared_masks, fmask=self.mask, want_valid=True, quant=quant)
        return dev.DeviceTensor(dst, tensor.shape, tensor.dtype, tensor.layout), valid

    def visualise(self, mode, show_mask=False, show_mask_borders=False, range_max=None):
        """self[i].visualise(...) for every i -> DeviceImage uint8 (n, H, W, 3): ONE range select (each field gets its own
        99th percentile unless `range_max` fixes one scale for all) and ONE render launch, asynchronous."""
        code, flags, rc = dev.visualise_args(mode, show_mask, show_mask_borders, range_max)
        h, w = self.shape
        rng = None
        if rc is None:
            rng = dev.DeviceBuffer(4 * self.n)
            dev.visualise_range_launch(self.vecs, h, w, self.n, rng)
        img = dev.visualise_launch(self.vecs, self.mask if flags else None, h, w, self.n, code, flags, rng, rc)
        img.shape = (self.n, h, w, 3)
        return img

    def visualise_range(self):
        """float32 array (n,): the default range_max of every field (one synchronisation)."""
        h, w = self.shape
        rng = dev.DeviceBuffer(4 * self.n)
        dev.visualise_range_launch(self.vecs, h, w, self.n, rng)
        return rng.to_host((self.n,), np.float32)


    # -- point tracking (K10)
    def field(self, i):
        """Field i as a DeviceFlow on this batch's memory (views: they keep the batch's buffers alive, nothing is copied)."""
        if not 0 <= i < self.n:
            raise IndexError("field {} of a batch of {}".format(i, self.n))
        px = self.shape[0] * self.shape[1]
        return dev.DeviceFlow(self.vecs.view(i * px * 8, px * 8), self.mask.view(i * px, px), self.shape, self.ref)

    def _stats_words(self):
        """uint32 [n] in HBM: the OFL_STAT_* word of every field, one launch of the statistics kernel per field and no
        read-back (the tracking kernels read the zero-flow predicate there).  Evaluated once: the fields are immutable."""
        words = getattr(self, "_words", None)
        if words is None:
            px = self.shape[0] * self.shape[1]
            words = dev.DeviceBuffer(4 * self.n)
            for k in range(self.n):
                dev.stats_word_launch(self.vecs.ptr + k * px * 8, None, px, words.ptr + 4 * k)
            self._words = words
        return words

    def _valid_sources(self):
        """uint8 [n][H][W]: valid_source() of every ref-'s' field, by the gather kernel.  (A thresholded-zero field needs
        no special case: under the gather's 1/32-px snapping its warp is the identity, which leaves its mask.)"""
        h, w = self.shape
        px = h * w
        maps = dev.DeviceBuffer(self.n * px)
        for k in range(self.n):
            dev.gather_valid_only(h, w, self.vecs.view(k * px * 8, px * 8), self.shape, +1, fmask=self.mask.view(k * px, px),
                                  valid=maps.view(k * px, px))
        return maps

    @staticmethod
    def _float_points(pts, what):
        on_host = not isinstance(pts, dev.DevicePoints)
        dp = dev.DevicePoints.from_host(pts) if on_host else pts
        if dp.dtype != np.float64:
            raise TypeError("Error tracking points: {} takes float points, got {}".format(what, dp.dtype))
        return dp, on_host

    def track(self, pts, int_out=None, get_valid_status=None):
        """The SAME points through every field of a ref-'s' batch, independently, in ONE launch: -> (n_fields, n, 2) points
        (float64, int32 with int_out) and, with get_valid_status, an (n_fields, n) status; row i is
        DeviceFlow.track(pts, int_out, get_valid_status) on field i bit for bit (bilinear sampling).  `pts`: float points, a
        DevicePoints (answered with a DevicePoints of shape (n_fields, n, 2) and a uint8 DeviceBuffer) or an (n, 2) array
        (answered with arrays).  Raises IndexError if a point is outside the area, like the single call."""
        int_out, get_valid_status, _ = dev.track_args(pts, int_out, get_valid_status, None)
        if self.ref != 's':
            raise ValueError("Error tracking points: DeviceFlowBatch.track batches the bilinear ('s') step; 't' fields go through "
                             "DeviceFlow.track one by one (field(i)) or through track_sequence")
        dp, on_host = self._float_points(pts, "DeviceFlowBatch.track")
        n, B = dp.n, self.n
        out = dev.DevicePoints(dev.DeviceBuffer(B * n * (8 if int_out else 16)), B * n, np.int32 if int_out else np.float64, (B, n, 2))
        status = dev.DeviceBuffer(B * n) if get_valid_status else None
        if n:
            valid = self._valid_sources() if get_valid_status else None
            outside = dev.DeviceBuffer.zeros(16)
            dev.track_bilinear_launch(self.vecs.ptr, B, self.shape, False, dp, self._stats_words(), valid, int_out, out.buf, status,
                                      outside=outside)
            if int(outside.to_host((1,), np.uint32)[0]):
                raise IndexError("Some points are outside of the data area.")
        if not on_host:
            return (out, status) if get_valid_status else out
        res = out.to_host()
        return (res, status.to_host((B, n), np.uint8).view(np.bool_)) if get_valid_status else res

    def track_sequence(self, pts, int_out=None, get_valid_status=None, return_path=False):
        """Points chained through the batch as a SEQUENCE: field k maps frame k to frame k + 1.  -> (points, lost_at
        [, status][, path]): the final positions (float64, int32 with int_out); lost_at int32 (n,), the step at which a point
        was lost or -1; with get_valid_status the Flow.track status ANDed over the steps, False for lost points; with
        return_path the float64 (n_fields + 1, n, 2) positions before, between and after the steps.

        ref 's' (bilinear sampling): ONE launch takes every point through all fields.  A point whose position before step k is
        outside the area (where a single call raises IndexError) is lost at k: it stays where it is.  The status maps
        (valid_source of every field) are built first, one gather per field.
        ref 't': one resident query and one epilogue per field; a point the interpolation finds no triangle for (which a
        single call moves to (0, 0)) is lost at that step and stays where it is.
        Never raises for points that leave the area.  `pts`: float64 points, a DevicePoints (answered with DevicePoints for
        points and path, DeviceBuffers int32 / uint8 for lost_at and status) or an (n, 2) array (answered with arrays).  The
        fields, and between the steps the points, stay in HBM."""
        int_out, get_valid_status, _ = dev.track_args(pts, int_out, get_valid_status, None)
        # no default to fall back on: None is refused like any other non-bool, as it always was
        return_path = dev.optional_bool(return_path, None, "Error tracking points: Return_path needs to be a boolean")
        dp, on_host = self._float_points(pts, "DeviceFlowBatch.track_sequence")
        n, B = dp.n, self.n
        out = dev.DevicePoints(dev.DeviceBuffer(n * (8 if int_out else 16)), n, np.int32 if int_out else np.float64)
        lost_at = dev.DeviceBuffer(4 * n)
        status = dev.DeviceBuffer(n) if get_valid_status else None
        path = dev.DevicePoints(dev.DeviceBuffer((B + 1) * n * 16), (B + 1) * n, np.float64, (B + 1, n, 2)) if return_path else None
        if n and self.ref == 's':
            valid = self._valid_sources() if get_valid_status else None
            dev.track_bilinear_launch(self.vecs.ptr, B, self.shape, True, dp, self._stats_words(), valid, int_out, out.buf, status,
                                      lost_at=lost_at, path=path.buf if return_path else None)
        elif n:
            self._sequence_t(dp, int_out, out, lost_at, status, path)
        res = [out, lost_at] + ([status] if get_valid_status else []) + ([path] if return_path else [])
        if on_host:
            res[0], res[1] = out.to_host(), lost_at.to_host((n,), np.int32)
            if get_valid_status:
                res[2] = status.to_host((n,), np.uint8).view(np.bool_)
            if return_path:
                res[-1] = path.to_host()
        return tuple(res)

    def _sequence_t(self, dp, int_out, out, lost_at, status, path):
        """track_sequence for ref 't': per field, the scatter kernel's query mode on the resident positions and the epilogue
        kernel, which also writes the next field's queries."""
        h, w = self.shape
        n, B, px = dp.n, self.n, self.shape[0] * self.shape[1]
        words = self._stats_words()
        query = dev.track_query_points(dp)
        if path is not None:
            nat.check(nat.load().ofl_copy_dev(path.buf.ptr, dp.buf.ptr, n * 16, None))
        for k in range(B):
            last = k == B - 1
            vecs = self.vecs.view(k * px * 8, px * 8)
            valid = self.field(k).valid_source() if status is not None else None
            vals, found = dev.scatter_query_resident(vecs, -1, vecs, h, w, query, n)
            nxt = None if last else dev.DeviceBuffer(n * 16)
            out_rc = None
            if path is not None:
                out_rc = path.buf.view((k + 1) * n * 16, n * 16)
            elif last and not int_out:
                out_rc = out.buf
            dev.track_query_epilogue(query, vals, found, n, self.shape, words.view(4 * k, 4), valid, k, status,
                                     out_rc=out_rc, out_int=out.buf if last and int_out else None, next_query=nxt, lost_at=lost_at)
            query = nxt
        if path is not None and not int_out:
            nat.check(nat.load().ofl_copy_dev(out.buf.ptr, path.buf.ptr + B * n * 16, n * 16, None))


def combine_flows_batch(flows_1, flows_2, ref=None, rank=0, world=1, thresholded=False):
    """Mode-3 composition of many independent pairs.  `flows_1[i] (+) flows_2[i]`; inputs are lists of
    `Flow` objects or of (H, W, 2) arrays with reference `ref`.  With world > 1 only the contiguous block of
    pairs owned by `rank` is processed and returned, as a list of (index, Flow)."""
    if len(flows_1) != len(flows_2):
        raise ValueError("need as many first as second flows")
    as_flow = lambda f: f if isinstance(f, Flow) else Flow(f, ref)
    mine = sharding.shard(len(flows_1), rank, world)
    if len(mine) == 0:
        return []
    f1 = [as_flow(flows_1[i]) for i in mine]
    f2 = [as_flow(flows_2[i]) for i in mine]
    b1, b2 = DeviceFlowBatch.from_flows(f1), DeviceFlowBatch.from_flows(f2)
    out, words, (fa, fb) = b1.compose3(b2)
    res = out.to_flows()
    bit = 1 if thresholded else 0                 # OFL_STAT_NONZERO_TH_MASKED / OFL_STAT_NONZERO_MASKED word index
    results = []
    for k, i in enumerate(mine):
        self_f, other_f = f1[k], f2[k]
        a_cert, b_nonzero = words[k][bit], words[k][4 + bit]
        # fa/fb roles: 't' -> fa = self, fb = flow; 's' -> fa = flow, fb = self
        fa_zero = (not a_cert) and (other_f if b1.ref == 's' else self_f).is_zero(thresholded=thresholded)
        fb_zero = not b_nonzero
        self_zero, flow_zero = (fb_zero, fa_zero) if b1.ref == 's' else (fa_zero, fb_zero)
        if self_zero:
            r = other_f
        elif flow_zero:
            r = self_f
        elif not words[k][7]:                      # sampling field thresholded-zero: plain sum (utils.py:215-216)
            r = other_f + self_f if b1.ref == 't' else self_f + other_f
        else:
            r = res[k]
        results.append((i, r))
    return results
