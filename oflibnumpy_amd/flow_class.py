"""The `Flow` class: same public surface, defaults, validation and exception types as the reference's
hot path (src/oflibnumpy/flow_class.py), with every warp executed by the MI355X engine.

A `Flow` owns host NumPy arrays (vecs float32 (H, W, 2), mask bool (H, W), ref 's'/'t') exactly like
the reference.  Its hot-path methods upload once, run the device-side algebra of `device.DeviceFlow`
(all intermediates stay in HBM) and download the result.  Pipelines that must not cross PCIe at all
use `DeviceFlow` directly.

Next-tier row already widened into: `track` / `track_pts`.
Dataset loaders (KITTI, Sintel + mask) are host I/O with a small built-in PNG reader.
Out of scope (not on the hot path): arrow drawing and display (`visualise_arrows`, `show*`).
"""
from __future__ import annotations

import warnings
from typing import Tuple, Union

import numpy as np

from . import _native as nat
from . import device as dev
from .utils import (get_valid_ref, get_valid_padding, validate_shape, from_matrix, from_transforms,
                    load_sintel, load_sintel_mask, load_kitti, is_zero_flow, threshold_vectors, track_pts,
                    _REMAP_DTYPES)

FlowAlias = 'Flow'


class Flow(object):
    _vecs: np.ndarray
    _mask: np.ndarray
    _ref: str

    def __init__(self, flow_vectors: np.ndarray, ref: str = None, mask: np.ndarray = None):
        """flow_vectors (H, W, 2) in OpenCV convention (channel 0 horizontal, 1 vertical), `ref` 't'
        (default) or 's', `mask` bool (H, W) of valid vectors (default all True).
        Reference: flow_class.py:38-51."""
        self.vecs = flow_vectors
        self.ref = ref
        self.mask = mask

    # ------------------------------------------------------------------ attributes
    @property
    def vecs(self) -> np.ndarray:
        return self._vecs

    @vecs.setter
    def vecs(self, input_vecs: np.ndarray):
        # reference flow_class.py:65-81: always a fresh float32 copy
        if not isinstance(input_vecs, np.ndarray):
            raise TypeError("Error setting flow vectors: Input is not a numpy array")
        if input_vecs.ndim != 3:
            raise ValueError("Error setting flow vectors: Input not 3-dimensional")
        if input_vecs.shape[2] != 2:
            raise ValueError("Error setting flow vectors: Input does not have 2 channels")
        if not np.isfinite(input_vecs).all():
            raise ValueError("Error setting flow vectors: Input contains NaN, Inf or -Inf values")
        self._vecs = input_vecs.astype('float32')

    @property
    def ref(self) -> str:
        return self._ref

    @ref.setter
    def ref(self, input_ref: str = None):
        self._ref = get_valid_ref(input_ref)

    @property
    def mask(self) -> np.ndarray:
        return self._mask

    @mask.setter
    def mask(self, input_mask: np.ndarray = None):
        # reference flow_class.py:142-161
        if input_mask is None:
            self._mask = np.ones(self.shape, 'bool')
            return
        if not isinstance(input_mask, np.ndarray):
            raise TypeError("Error setting flow mask: Input is not a numpy array")
        if input_mask.ndim != 2:
            raise ValueError("Error setting flow mask: Input not 2-dimensional")
        if input_mask.shape != self.shape:
            raise ValueError("Error setting flow mask: Input has a different shape than the flow vectors")
        if ((input_mask != 0) & (input_mask != 1)).any():
            raise ValueError("Error setting flow mask: Values must be 0 or 1")
        self._mask = input_mask.astype('bool')

    @property
    def shape(self) -> tuple:
        return self._vecs.shape[:2]

    # ------------------------------------------------------------------ constructors
    @classmethod
    def zero(cls, shape: Union[list, tuple], ref: str = None, mask: np.ndarray = None) -> FlowAlias:
        validate_shape(shape)
        return cls(np.zeros((shape[0], shape[1], 2)), ref, mask)

    @classmethod
    def from_matrix(cls, matrix: np.ndarray, shape: Union[list, tuple], ref: str = None,
                    mask: np.ndarray = None) -> FlowAlias:
        return cls(from_matrix(matrix, shape, ref), ref, mask)

    @classmethod
    def from_transforms(cls, transform_list: list, shape: Union[list, tuple], ref: str = None,
                        mask: np.ndarray = None) -> FlowAlias:
        return cls(from_transforms(transform_list, shape, ref), ref, mask)

    @classmethod
    def from_kitti(cls, path: str, load_valid: bool = None) -> FlowAlias:
        """KITTI uint16 PNG -> flow with reference 's', optionally with the valid pixels as mask
        (reference flow_class.py:237-259)."""
        load_valid = dev.optional_bool(load_valid, True, "Error loading flow from KITTI data: Load_valid needs to be boolean")
        data = load_kitti(path)
        return cls(data[..., :2], 's', data[..., 2].astype('bool')) if load_valid else cls(data[..., :2], 's')

    @classmethod
    def from_sintel(cls, path: str, inv_path: str = None) -> FlowAlias:
        """Sintel .flo (+ optional invalid-pixel PNG) -> flow with reference 's' (reference flow_class.py:262-275)."""
        mask = None if inv_path is None else load_sintel_mask(inv_path)
        return cls(load_sintel(path), 's', mask)

    def copy(self) -> FlowAlias:
        return Flow(self._vecs, self._ref, self._mask)

    def __str__(self) -> str:
        return "Flow object, reference {}, shape {}*{}; ".format(self._ref, *self.shape) + self.__repr__()

    def __getitem__(self, item) -> FlowAlias:
        return Flow(self._vecs.__getitem__(item), self._ref, self._mask.__getitem__(item))

    # ------------------------------------------------------------------ element-wise operators
    def _check_other(self, other, verb, noun):
        if not isinstance(other, (np.ndarray, Flow)):
            raise TypeError("Error {} flow: {} is not a flow object or a numpy array".format(verb, noun))
        if isinstance(other, Flow):
            if self.shape != other.shape:
                raise ValueError("Error {} flow: flow objects are not the same shape".format(verb))
        elif self.shape != other.shape[:2] or other.ndim != 3 or other.shape[2] != 2:
            raise ValueError("Error {} flow: numpy array needs to have the same shape as the flow object, "
                             "3 dimensions overall, and a channel length of 2".format(verb))

    def __add__(self, other: Union[np.ndarray, FlowAlias]) -> FlowAlias:
        # reference flow_class.py:310-341: keeps the left operand's ref, masks are ANDed
        self._check_other(other, "adding to", "Addend")
        if isinstance(other, Flow):
            return Flow(self._vecs + other._vecs, self._ref, np.logical_and(self._mask, other._mask))
        return Flow(self._vecs + other, self._ref, self._mask)

    def __sub__(self, other: Union[np.ndarray, FlowAlias]) -> FlowAlias:
        self._check_other(other, "subtracting from", "Subtrahend")
        if isinstance(other, Flow):
            return Flow(self._vecs - other._vecs, self._ref, np.logical_and(self._mask, other._mask))
        return Flow(self._vecs - other, self._ref, self._mask)

    def _broadcast_operand(self, other, verb, noun):
        """Scalar / list of 2 / array (2,), (H, W) or (H, W, 2) -> something NumPy can broadcast
        (reference flow_class.py:377-477)."""
        try:
            return float(other)
        except TypeError:
            pass
        if isinstance(other, list):
            if len(other) != 2:
                raise ValueError("Error {} flow: {} list not length 2".format(verb, noun))
            return np.array(other)[np.newaxis, np.newaxis, :]
        if isinstance(other, np.ndarray):
            if other.ndim == 1 and other.size == 2:
                return other[np.newaxis, np.newaxis, :]
            if other.ndim == 2 and other.shape == self.shape[:2]:
                return other[:, :, np.newaxis]
            if other.shape == self.shape + (2,):
                return other
            raise ValueError("Error {} flow: {} array is not one of the following: size 2, shape of the "
                             "flow object, shape of the flow vectors".format(verb, noun))
        raise TypeError("Error {} flow: {} cannot be converted to float, or isn't a list or numpy array"
                        .format(verb, noun))

    def __mul__(self, other) -> FlowAlias:
        return Flow(self._vecs * self._broadcast_operand(other, "multiplying", "Multiplier"), self._ref, self._mask)

    def __truediv__(self, other) -> FlowAlias:
        return Flow(self._vecs / self._broadcast_operand(other, "dividing", "Divisor"), self._ref, self._mask)

    def __pow__(self, other) -> FlowAlias:
        return Flow(self._vecs ** self._broadcast_operand(other, "exponentiating", "Exponent"), self._ref, self._mask)

    def __neg__(self) -> FlowAlias:
        return self * -1

    def resize(self, scale: Union[float, int, list, tuple]) -> FlowAlias:
        """Resize the flow field, scaling the vectors accordingly; the mask is resized bilinearly and rounded
        (flow_class.py:491-506)."""
        dev.resize_scales(scale)
        vecs, mask = dev.resize_host(self._vecs, self._mask, scale)
        return Flow(vecs, self._ref, mask)

    def pad(self, padding: Union[list, tuple] = None, mode: str = None) -> FlowAlias:
        """Pad vecs ('constant' zeros, 'edge' or 'symmetric') and the mask with False (flow_class.py:508-526)."""
        mode = 'constant' if mode is None else mode
        if mode not in ('constant', 'edge', 'symmetric'):
            raise ValueError("Error padding flow: Mode should be one of "
                             "'constant', 'edge', 'symmetric', but instead got '{}'".format(mode))
        p = get_valid_padding(padding, "Error padding flow: ")
        vecs = np.pad(self._vecs, ((p[0], p[1]), (p[2], p[3]), (0, 0)), mode=mode)
        mask = np.pad(self._mask, ((p[0], p[1]), (p[2], p[3])))
        return Flow(vecs, self._ref, mask)

    # ------------------------------------------------------------------ device plumbing
    def to_device(self) -> dev.DeviceFlow:
        return dev.DeviceFlow.from_host(self._vecs, self._ref, self._mask)

    @classmethod
    def from_device(cls, dflow: dev.DeviceFlow) -> FlowAlias:
        """Download a device result.  The arrays come out of the kernels as float32 / 0-1 bytes computed from
        already validated inputs, so the constructor's copy-and-validate passes (3 x the PCIe time at 4K) are
        skipped."""
        vecs, mask = dflow.to_host()
        f = cls.__new__(cls)
        f._vecs, f._mask, f._ref = vecs, mask, get_valid_ref(dflow.ref)
        return f

    # ------------------------------------------------------------------ hot path
    def apply(self, target: Union[np.ndarray, FlowAlias], target_mask: np.ndarray = None,
              return_valid_area: bool = None, consider_mask: bool = None,
              padding: Union[list, tuple] = None, cut: bool = None
              ) -> Union[Union[np.ndarray, FlowAlias], Tuple[Union[np.ndarray, FlowAlias], np.ndarray]]:
        """Warp `target` (ndarray (H, W[, C]) or Flow) with this flow.  Arguments, defaults, return
        conventions and raised exception types follow the reference (flow_class.py:528-695)."""
        return_valid_area = dev.optional_bool(return_valid_area, False, "Error applying flow: Return_valid_area needs to be a boolean")
        consider_mask = dev.optional_bool(consider_mask, True, "Error applying flow: Consider_mask needs to be a boolean")
        cut = dev.optional_bool(cut, True, "Error applying flow: Cut needs to be a boolean")
        if padding is None:
            if self.shape[0] != target.shape[0] or self.shape[1] != target.shape[1]:
                raise ValueError("Error applying flow: Flow shape does not match target shape")
        else:
            padding = get_valid_padding(padding, "Error applying flow: ")
            if self.shape[0] + padding[0] + padding[1] != target.shape[0] or \
                    self.shape[1] + padding[2] + padding[3] != target.shape[1]:
                raise ValueError("Error applying flow: Padding values do not match flow and target shape difference")

        return_2d = False
        if isinstance(target, Flow):
            return_flow, t, tmask, default_mask = True, target._vecs, target._mask, False
        elif isinstance(target, np.ndarray):
            return_flow = False
            if target.ndim == 3:
                t = target
            elif target.ndim == 2:
                return_2d, t = True, target[..., np.newaxis]
            else:
                raise ValueError("Error applying flow: Target needs to have the shape H-W (2 dimensions) "
                                 "or H-W-C (3 dimensions)")
            default_mask = target_mask is None
            if default_mask:
                tmask = np.ones(t.shape[:2], bool)
            else:
                if not isinstance(target_mask, np.ndarray):
                    raise TypeError("Error applying flow: Target_mask needs to be a numpy ndarray")
                if target_mask.shape != target.shape[:2]:
                    raise ValueError("Error applying flow: Target_mask needs to match the target shape")
                if target_mask.dtype != bool:
                    raise TypeError("Error applying flow: Target_mask needs to have dtype 'bool'")
                if not return_valid_area:
                    warnings.warn("Warning applying flow: a mask is passed, but return_valid_area is False - so the "
                                  "mask passed will not affect the output, but possibly make the function slower.")
                tmask = target_mask
        else:
            raise ValueError("Error applying flow: Target needs to be either a flow object, or a numpy ndarray")

        with_mask = return_flow or return_valid_area
        pad_tl = (0, 0) if padding is None else (padding[0], padding[2])
        if self._ref == 't':
            warped, valid = self._apply_t(t, tmask, default_mask, with_mask, pad_tl)
        else:
            warped, valid = self._apply_s(t, tmask, with_mask, consider_mask, padding)

        if padding is not None and cut:
            sl = (slice(padding[0], padding[0] + self.shape[0]), slice(padding[2], padding[2] + self.shape[1]))
            warped = warped[sl]
            valid = valid[sl] if valid is not None else None

        if return_flow:
            return Flow(warped, target._ref, valid)
        if return_2d:
            warped = warped[:, :, 0]
        warped = np.ascontiguousarray(warped)
        return (warped, valid) if return_valid_area else warped

    def _apply_t(self, t, tmask, default_mask, with_mask, pad_tl):
        """'t' reference: one launch of the gather kernel K1 (replaces flow_class.py:644-650 +
        cv2.remap).  The reference appends the mask as an extra channel, which fixes the dtype the
        remap runs in; the same arithmetic is selected here without materialising the concat."""
        if t.dtype.type not in _REMAP_DTYPES:
            raise TypeError("Error applying flow: target dtype {} is not supported by the bilinear remap "
                            "(uint8, int16, uint16, float32, float64)".format(t.dtype))
        arith, rule = nat.ARITH_NATIVE, nat.RULE_EQ1
        if with_mask:
            # dtype of np.concatenate((t, mask[..., None])) with mask int8 (default, :615) or bool (:626)
            concat = np.result_type(t.dtype, np.int8 if default_mask else np.bool_)
            if concat.type not in _REMAP_DTYPES:
                raise TypeError("Error applying flow: target dtype {} with a validity mask needs a {} remap, "
                                "which cv2.remap does not provide".format(t.dtype, concat))
            if concat == np.uint8:
                rule = nat.RULE_GE_HALF
            elif concat in (np.int16, np.uint16):
                rule = nat.RULE_GT_HALF
                if t.dtype == np.uint8:
                    arith = nat.ARITH_FLOAT_RNE        # uint8 image inside an int16 concat
        fbuf = dev.DeviceBuffer.from_host(self._vecs)
        if not (dev.flow_stats(fbuf, None, self._vecs.shape[0] * self._vecs.shape[1]) & nat.STAT_NONZERO_TH):
            warped = t                                      # identity short cut, reference utils.py:215-216
            valid = None
            if with_mask:
                valid = np.zeros(t.shape[:2], bool)
                valid[pad_tl[0]:pad_tl[0] + self.shape[0], pad_tl[1]:pad_tl[1] + self.shape[1]] = self._mask
                valid &= tmask.astype(bool)
            return warped, valid
        src = dev.DeviceImage.from_host(t)
        smask = dev.DeviceBuffer.from_host(tmask.astype(np.uint8)) if (with_mask and not default_mask) else None
        fmask = dev.DeviceBuffer.from_host(self._mask.view(np.uint8)) if with_mask else None
        dst, valid = dev.gather_bilinear(src, fbuf, self.shape, -1, smask=smask, fmask=fmask,
                                         want_valid=with_mask, pad=pad_tl, arith=arith, rule=rule)
        warped = dst.to_host()
        valid = valid.to_host(t.shape[:2], np.uint8).view(np.bool_) if with_mask else None
        return warped, valid

    def _apply_s(self, t, tmask, with_mask, consider_mask, padding):
        """'s' reference: scattered -> grid interpolation kernel K3 (replaces flow_class.py:634-660 +
        scipy griddata).  With padding the flow is edge-padded first (flow_class.py:652-659)."""
        flow = self if padding is None else self.pad(padding, mode='edge')
        if with_mask:
            tmask = tmask.astype(bool) & flow._mask                  # flow_class.py:636-643
        fbuf = dev.DeviceBuffer.from_host(flow._vecs)           # uploaded once: zero test and scatter share it
        if not (dev.flow_stats(fbuf, None, flow.shape[0] * flow.shape[1]) & nat.STAT_NONZERO_TH):
            return t, (tmask.copy() if with_mask else None)        # identity short cut, utils.py:215-216
        return dev.scatter_host(fbuf, t, flow._mask if consider_mask else None,
                                vmask=tmask if with_mask else None)

    def switch_ref(self, mode: str = None) -> FlowAlias:
        """Switch between 's' and 't' reference (reference flow_class.py:697-733)."""
        mode = 'valid' if mode is None else mode
        if mode == 'invalid':
            return Flow(self._vecs, 't' if self._ref == 's' else 's', self._mask)
        if mode != 'valid':
            raise ValueError("Error switching flow reference: Mode not recognised, should be 'valid' or 'invalid'")
        d = self.to_device()
        if d.is_zero(thresholded=False):
            return self.switch_ref(mode='invalid')
        return Flow.from_device(d.switch_ref())

    def invert(self, ref: str = None) -> FlowAlias:
        """Inverse flow in the requested reference (reference flow_class.py:735-753)."""
        ref = self._ref if ref is None else get_valid_ref(ref)
        if ref != self._ref:
            return Flow(-self._vecs, ref, self._mask)          # s->t and t->s are a negation only
        return Flow.from_device(self.to_device().invert(ref))

    def track(self, pts: np.ndarray, int_out: bool = None, get_valid_status: bool = None,
              s_exact_mode: bool = None) -> np.ndarray:
        """Warp points (N, 2) in (row, col) order with the flow; optionally also return which points are
        moved by valid vectors to a position inside the flow area (reference flow_class.py:755-795)."""
        get_valid_status = dev.optional_bool(get_valid_status, False, "Error tracking points: Get_tracked needs to be a boolean")
        warped = track_pts(flow=self._vecs, ref=self._ref, pts=pts, int_out=int_out, s_exact_mode=s_exact_mode)
        if get_valid_status:
            status = self.valid_source()[np.round(pts[..., 0]).astype('i'), np.round(pts[..., 1]).astype('i')]
            return warped, status
        return warped

    def valid_target(self, consider_mask: bool = None) -> np.ndarray:
        """Area of the target domain reached by valid vectors (reference flow_class.py:1113-1151)."""
        consider_mask = dev.optional_bool(consider_mask, True, "Error applying flow: Consider_mask needs to be a boolean")
        buf = self.to_device().valid_target(consider_mask)
        return buf.to_host(self.shape, np.uint8).view(np.bool_)

    def valid_source(self, consider_mask: bool = None) -> np.ndarray:
        """Area of the source domain that ends up valid in the target (reference flow_class.py:1153-1195)."""
        consider_mask = dev.optional_bool(consider_mask, True, "Error applying flow: Consider_mask needs to be a boolean")
        buf = self.to_device().valid_source(consider_mask)
        return buf.to_host(self.shape, np.uint8).view(np.bool_)

    def get_padding(self) -> list:
        """[top, bottom, left, right] padding needed so that no valid vector leaves the padded area
        (reference flow_class.py:1197-1228)."""
        return self.to_device().get_padding()

    def is_zero(self, thresholded: bool = None, masked: bool = None) -> bool:
        """All (masked) vectors zero?  (reference flow_class.py:1230-1245)"""
        masked = dev.optional_bool(masked, True, "Error checking whether flow is zero: Masked needs to be a boolean")
        thresholded = dev.optional_bool(thresholded, True, "Error checking whether flow is zero: Thresholded needs to be a boolean")
        return self.to_device().is_zero(thresholded, masked)

    def visualise(self, mode: str, show_mask: bool = None, show_mask_borders: bool = None,
                  range_max: float = None) -> np.ndarray:
        """The flow as a uint8 (H, W, 3) 'rgb' / 'bgr' / 'hsv' image: hue = direction, saturation = magnitude over
        `range_max` (default: the 99th percentile of the magnitudes), invalid areas dimmed with `show_mask`, the mask
        outline black with `show_mask_borders` (reference flow_class.py:869-951).  A non-finite `range_max` raises
        ValueError.  Rendered by the device (DeviceFlow.visualise); arguments are checked before any device work."""
        show_mask = False if show_mask is None else show_mask
        show_mask_borders = False if show_mask_borders is None else show_mask_borders
        dev.visualise_args(mode, show_mask, show_mask_borders, range_max)
        return self.to_device().visualise(mode, show_mask, show_mask_borders, range_max).to_host()

    def matrix(self, dof: int = None, method: str = None, masked: bool = None) -> np.ndarray:
        """The (3, 3) float64 transformation matrix fitted to the flow: `dof` 4 (rotation, translation, scaling), 6 (affine)
        or 8 (homography, the default); `method` 'lms' (dof 8 only, otherwise replaced by 'ransac' with a warning), 'ransac'
        (default) or 'lmeds'; `masked` (default True) ignores vectors where the mask is False (reference
        flow_class.py:797-867).  Fitted by the device (DeviceFlow.matrix): the estimators follow OpenCV's scheme and
        parameters without being bit-compatible with it.  Arguments are checked before any device work."""
        from . import matrix_fit
        dof, method, masked, _ = matrix_fit.matrix_args(dof, method, masked)
        return self.to_device().matrix(dof, method, masked)

    def consistency(self, backward: FlowAlias, alpha: float = None, beta: float = None,
                    return_residual: bool = None) -> Tuple[np.ndarray, ...]:
        """Forward-backward check of this (forward) flow against `backward`, a flow of the same shape and reference:
        the backward flow is sampled where this one points, and a pixel is `covered` where that sample and this vector
        are valid, `consistent` where it is covered and |self + sampled|^2 <= alpha * (|self|^2 + |sampled|^2) + beta
        (defaults 0.01 and 0.5).  -> (consistent, covered) as bool (H, W) arrays, plus the float32 (H, W) residual
        |self + sampled| (0 where not covered) with `return_residual`.  Not a function of the reference; the definition,
        which takes no zero-flow short cut, is DeviceFlow.consistency's.  One upload, one launch, one download."""
        alpha, beta = dev.consistency_args(alpha, beta)
        return_residual = dev.optional_bool(return_residual, False, "Error checking flow consistency: Return_residual needs to be a boolean")
        if not isinstance(backward, Flow):
            raise TypeError("Error checking flow consistency: Backward needs to be of type 'Flow'")
        if self.shape != backward.shape:
            raise ValueError("Error checking flow consistency: Flow fields need to have the same shape, got {} and {}"
                             .format(self.shape, backward.shape))
        if self.ref != backward.ref:
            raise ValueError("Error checking flow consistency: Flow fields need to have the same reference, got '{}' and '{}'"
                             .format(self.ref, backward.ref))
        return dev.consistency_host(self._vecs, self._mask, backward._vecs, backward._mask, 1 if self._ref == 's' else -1,
                                    alpha, beta, return_residual)

    def photometric(self, near: np.ndarray, far: np.ndarray, metric: str = 'l1', eps: float = None, threshold: float = None,
                    near_mask: np.ndarray = None, far_mask: np.ndarray = None, layout: str = 'hwc',
                    quant: int = 0) -> Tuple[np.ndarray, ...]:
        """The photometric (brightness- or feature-constancy) error of this flow: `near`, the image or feature array of the
        flow's own frame, against `far`, that of the other frame, sampled where the flow points and reduced over the
        channels -- the mean absolute difference ('l1'), the root mean square ('l2') or the mean of sqrt(d^2 + eps^2)
        ('charbonnier', eps None: 1e-3).  near, far: arrays of one shape and dtype, (H, W), (H, W, C) or -- layout='chw' --
        (C, H, W), a leading item axis allowed; float32, float16, or uint8 images, which are converted to float32 (exact).
        near_mask, far_mask: bool or uint8 (H, W) arrays or None.  -> (error float32, covered bool), each (H, W) -- or
        (N, H, W) --, plus within = covered & (error <= threshold) as bool with `threshold`.  Works for 's' and 't' flows.
        Not a function of the reference; the definition is DeviceFlow.photometric's.  One upload, one launch, one
        download."""
        prefix = "Error computing photometric error: "
        code, eps, threshold = dev.photometric_args(metric, eps, threshold)
        near, far, n, c, batched = dev.pair_host_arrays(near, far, layout, self.shape, prefix)
        near_mask = None if near_mask is None else dev.mask_array_arg(near_mask, self.shape, prefix, "near_mask")
        far_mask = None if far_mask is None else dev.mask_array_arg(far_mask, self.shape, prefix, "far_mask")
        res = dev.photometric_host(near, far, layout, n, c, self._vecs, self._mask, 1 if self._ref == 's' else -1, code, eps,
                                   threshold, near_mask, far_mask, quant)
        return res if batched else tuple(r[0] for r in res)

    def census(self, near: np.ndarray, far: np.ndarray, window: int = 7, mode: str = 'soft', delta: float = None,
               noise: float = None, knee: float = None, min_count: int = None, threshold: float = None,
               near_mask: np.ndarray = None, far_mask: np.ndarray = None, layout: str = 'hwc',
               quant: int = 0) -> Tuple[np.ndarray, ...]:
        """The census distance of this flow: the order of the intensities (channel means) in a window x window
        neighbourhood of each pixel of `near`, the image of the flow's own frame, against the same in `far`, that of the
        other frame, sampled where the flow points -- 'hard' (share of neighbours whose sign differs, dead zone `delta`) or
        'soft' (the ternary census of unsupervised flow, `noise` None: 0.81, `knee` None: 0.1, for intensities 0 ... 255);
        unlike photometric it ignores a change of exposure or gain.  near, far: arrays as in photometric with 1 to 4
        channels, uint8 images included (converted to float32, exact).  min_count: the valid neighbours a pixel needs, None:
        all window^2 - 1.  -> (error float32, covered bool), each (H, W) -- or (N, H, W) --, plus within = covered &
        (error <= threshold) as bool with `threshold`.  Not a function of the reference; the definition is
        DeviceFlow.census's.  One upload, one launch, one download."""
        prefix = "Error computing census distance: "
        settings = dev.census_args(window, mode, delta, noise, knee, min_count, threshold)
        near, far, n, c, batched = dev.pair_host_arrays(near, far, layout, self.shape, prefix, nat.CENSUS_MAX_C)
        near_mask = None if near_mask is None else dev.mask_array_arg(near_mask, self.shape, prefix, "near_mask")
        far_mask = None if far_mask is None else dev.mask_array_arg(far_mask, self.shape, prefix, "far_mask")
        res = dev.census_host(near, far, layout, n, c, self._vecs, self._mask, 1 if self._ref == 's' else -1, *settings,
                              near_mask=near_mask, far_mask=far_mask, quant=quant)
        return res if batched else tuple(r[0] for r in res)

    def ssim(self, near: np.ndarray, far: np.ndarray, window: int = 11, weights: str = 'gaussian', sigma: float = None,
             data_range: float = 255.0, k1: float = 0.01, k2: float = 0.03, min_count: int = None, threshold: float = None,
             near_mask: np.ndarray = None, far_mask: np.ndarray = None, layout: str = 'hwc',
             quant: int = 0) -> Tuple[np.ndarray, ...]:
        """The structural dissimilarity (1 - SSIM) / 2 of this flow, in [0, 1]: Wang et al.'s SSIM of the intensities
        (channel means) in a weighted window x window neighbourhood (3, 5, 7 or 11) of each pixel of `near`, the image of
        the flow's own frame, against the same in `far`, that of the other frame, sampled where the flow points -- weights
        'gaussian' (`sigma` None: 1.5; the defaults are Wang's 11 x 11 window for intensities 0 ... 255) or 'uniform' (the
        avg_pool2d form of unsupervised flow); c1 = (k1 data_range)^2, c2 = (k2 data_range)^2.  near, far: arrays as in
        photometric with 1 to 4 channels, uint8 images included (converted to float32, exact).  min_count: the valid pixels
        a window needs, the centre among them, None: all window^2.  -> (error float32, covered bool), each (H, W) -- or
        (N, H, W) --, plus within = covered & (error <= threshold) as bool with `threshold`; SSIM itself is 1 - 2 error and
        its mean error[covered].mean().  Not a function of the reference; the definition is DeviceFlow.ssim's.  One upload,
        one launch, one download."""
        prefix = "Error computing structural similarity: "
        settings = dev.ssim_args(window, weights, sigma, data_range, k1, k2, min_count, threshold)
        near, far, n, c, batched = dev.pair_host_arrays(near, far, layout, self.shape, prefix, nat.SSIM_MAX_C)
        near_mask = None if near_mask is None else dev.mask_array_arg(near_mask, self.shape, prefix, "near_mask")
        far_mask = None if far_mask is None else dev.mask_array_arg(far_mask, self.shape, prefix, "far_mask")
        res = dev.ssim_host(near, far, layout, n, c, self._vecs, self._mask, 1 if self._ref == 's' else -1, *settings,
                            near_mask=near_mask, far_mask=far_mask, quant=quant)
        return res if batched else tuple(r[0] for r in res)

    def refine(self, near: np.ndarray, far: np.ndarray, alpha: float = None, delta: float = None, zeta: float = None,
               eps: float = None, fixed_point: int = None, sor: int = None, omega: float = None,
               near_mask: np.ndarray = None, far_mask: np.ndarray = None, valid: np.ndarray = None, return_data: bool = False,
               layout: str = 'hwc', quant: int = 0):
        """This flow moved a fraction of a pixel towards where the two images say it belongs: the variational refinement of
        Brox et al. without the gradient-constancy term, the last step of EpicFlow, DeepFlow, RICFlow and DIS -- one warp
        of `far`, `fixed_point` lagged-weight updates of `sor` red-black SOR sweeps with relaxation `omega`, smoothness
        weight `alpha`, data weight `delta`, normalisation `zeta`, Charbonnier constant `eps` (None: 20, 5, 0.1, 0.1, 5, 5,
        1.6).  Call it again to re-warp.  near, far: arrays as in census (one item, 1 to 4 channels, uint8 images
        included); near_mask, far_mask, valid: bool or uint8 (H, W) arrays or None; vectors where the mask or `valid` is
        unset, or that are not finite, come back unchanged.  -> a Flow of the same reference and mask, plus the bool (H, W)
        array of the pixels with a data term with `return_data`.  The definition is DeviceFlow.refine's.  One upload, the
        launches, one download."""
        prefix = "Error refining flow: "
        settings = dev.refine_args(alpha, delta, zeta, eps, fixed_point, sor, omega)
        near, far, _, c, _ = dev.pair_host_arrays(near, far, layout, self.shape, prefix, nat.REFINE_MAX_C, one_item=True)
        near_mask = None if near_mask is None else dev.mask_array_arg(near_mask, self.shape, prefix, "near_mask")
        far_mask = None if far_mask is None else dev.mask_array_arg(far_mask, self.shape, prefix, "far_mask")
        valid = None if valid is None else dev.mask_array_arg(valid, self.shape, prefix, "valid")
        vecs, data = dev.refine_host(near, far, layout, 1, c, self._vecs, self._mask, 1 if self._ref == 's' else -1, *settings,
                                     near_mask=near_mask, far_mask=far_mask, valid=valid, want_data=bool(return_data), quant=quant)
        out = Flow(vecs[0], self._ref, self._mask.copy())
        return (out, data[0]) if return_data else out

    def inverse_search(self, near: np.ndarray, far: np.ndarray, patch: int = 8, stride: int = 4, iterations: int = 12,
                       normalise: bool = True, floor: float = 1.0, return_patches: bool = False, layout: str = 'hwc',
                       quant: int = 1):
        """The flow the two images ask for near this one: the patch inverse search and the densification of Dense Inverse
        Search (Kroeger et al., ECCV 2016; OpenCV's DISOpticalFlow).  Every `patch` x `patch` window (4 or 8) on a grid of
        `stride` starts from this flow's vector at its centre (zero where the mask is unset or the vector not finite), takes
        up to `iterations` Lucas-Kanade translation steps on the channel means of the images and keeps the best, at most
        `patch` pixels away; every pixel then takes the average of the patches covering it, weighted by
        1 / max(floor, intensity difference).  near, far: arrays as in refine (one item, 1 to 4 channels, uint8 images
        included), at least `patch` high and wide.  -> a Flow of the same reference whose mask is set where the average is
        finite, plus (patch_vecs (ny, nx, 2), patch_ssd (ny, nx), (ny, nx)) with `return_patches`.  The definition is
        DeviceFlow.inverse_search's; the pyramid is estimate_flow.  One upload, three launches, one download."""
        prefix = "Error searching flow: "
        settings = dev.inverse_search_args(patch, stride, iterations, normalise, floor)
        near, far, _, c, _ = dev.pair_host_arrays(near, far, layout, self.shape, prefix, nat.ISEARCH_MAX_C, one_item=True)
        if min(self.shape) < settings[0]:
            raise ValueError("{}a {} x {} flow holds no patch of {}".format(prefix, self.shape[0], self.shape[1], settings[0]))
        vecs, mask, pv, ps, grid = dev.inverse_search_host(near, far, layout, 1, c, self._vecs, self._mask,
                                                           1 if self._ref == 's' else -1, *settings,
                                                           want_patches=bool(return_patches), quant=quant)
        out = Flow(vecs[0], self._ref, mask[0])
        return (out, pv[0], ps[0], grid) if return_patches else out

    def error(self, gt: FlowAlias, thresholds=None, outlier=None, speed_edges=None, use_est_mask: bool = None,
              return_map: bool = None):
        """How far this (estimated) flow is from the ground truth `gt`, a flow of the same shape and reference: the
        end-point error |self - gt| over the pixels where gt.mask (and, unless use_est_mask is False, self.mask) is set and the
        error is finite.  -> FlowErrorStats with n, n_nonfinite, epe (mean), rmse, max, over (share above each of up to 4
        `thresholds`, default 1, 3, 5 px), outlier (share above both bounds of `outlier`, default KITTI's 3 px and 5 % of
        |gt|) and bins ((n, mean epe) per speed bin of gt, `speed_edges` default Sintel's 10, 40); with `return_map` also the
        float32 (H, W) error (0 where not evaluated).  Not a function of the reference; the definition is DeviceFlow.error's.
        One upload, one launch, one download."""
        thr, out, edges, n_thr, n_edges = dev.error_args(thresholds, outlier, speed_edges)
        use_est_mask = dev.optional_bool(use_est_mask, True, "Error evaluating flow error: Use_est_mask needs to be a boolean")
        return_map = dev.optional_bool(return_map, False, "Error evaluating flow error: Return_map needs to be a boolean")
        if not isinstance(gt, Flow):
            raise TypeError("Error evaluating flow error: Gt needs to be of type 'Flow'")
        if self.shape != gt.shape:
            raise ValueError("Error evaluating flow error: Flow fields need to have the same shape, got {} and {}"
                             .format(self.shape, gt.shape))
        if self.ref != gt.ref:
            raise ValueError("Error evaluating flow error: Flow fields need to have the same reference, got '{}' and '{}'"
                             .format(self.ref, gt.ref))
        record, epe_map, _ = dev.error_host(self._vecs, self._mask if use_est_mask else None, gt._vecs, gt._mask, thr, out, edges,
                                            want_map=return_map)
        stats = dev.FlowErrorStats(record, n_thr, n_edges)
        return (stats, epe_map) if return_map else stats

    def fill(self, valid: np.ndarray = None, max_dist: float = None, return_index: bool = None, return_d2: bool = None):
        """This flow with the vectors of masked-out pixels replaced by the vector of the nearest valid pixel: a pixel is a
        source where the mask -- and `valid`, a bool or uint8 (H, W) array, if given -- is set, every pixel takes the vector
        of its nearest source (Euclidean pixel distance; among equally near sources the first in row-major order) if that
        one lies within `max_dist` px (None: no limit), and keeps its own otherwise.  -> a Flow of the same reference whose
        mask is True where a pixel was filled; with `return_index` also the int32 (H, W) linear index of the nearest source
        (-1: none), with `return_d2` the uint32 (H, W) squared distance (0xFFFFFFFF: none).  Not a function of the
        reference; the definition is DeviceFlow.fill's.  One upload, two launches, one download."""
        max_d2 = dev.fill_args(max_dist)
        return_index = dev.optional_bool(return_index, False, "Error filling flow: Return_index needs to be a boolean")
        return_d2 = dev.optional_bool(return_d2, False, "Error filling flow: Return_d2 needs to be a boolean")
        valid = None if valid is None else dev.mask_array_arg(valid, self.shape, "Error filling flow: ", "valid")
        vecs, mask, index, d2 = dev.fill_host(self._vecs, self._mask, valid, max_d2, return_index, return_d2)
        res = Flow(vecs, self._ref, mask)
        extra = ((index,) if return_index else ()) + ((d2,) if return_d2 else ())
        return (res,) + extra if extra else res

    def median(self, ksize: int = 5, valid: np.ndarray = None, only: np.ndarray = None, min_count: int = None) -> FlowAlias:
        """This flow with its vectors median-filtered over a ksize x ksize window (3, 5 or 7), mask-aware: a
        pixel is a member where the mask -- and `valid`, a bool or uint8 (H, W) array, if given -- is set, every pixel
        takes, per component, the lower median of the members in its window if there are at least `min_count` (None: 1)
        of them, and keeps its vector and gets mask False otherwise; `only`, a bool or uint8 (H, W) array, restricts the
        filter to the pixels where it is set.  Nothing is averaged: every output value is a value of the input.  -> a
        Flow of the same reference.  Not a function of the reference; the definition is DeviceFlow.median's.  One upload,
        one launch, one download."""
        ksize, min_count = dev.median_args(ksize, min_count)
        valid = None if valid is None else dev.mask_array_arg(valid, self.shape, "Error filtering flow: ", "valid")
        only = None if only is None else dev.mask_array_arg(only, self.shape, "Error filtering flow: ", "only")
        vecs, mask = dev.median_host(self._vecs, self._mask, valid, only, ksize, min_count)
        return Flow(vecs, self._ref, mask)

    def upsample_convex(self, weights: np.ndarray, factor: int = 8) -> FlowAlias:
        """This flow, a network's coarse output of shape (h, w), convexly upsampled by `factor` (2, 4 or 8): `weights`, a
        float32 or float16 array (9 f^2, h, w), holds the network's mask logits in RAFT's channel order; every fine pixel
        is the softmax-weighted combination of the 3 x 3 coarse neighbours, times f, and is valid where every neighbour
        inside the frame is.  -> a Flow of shape (f h, f w) and the same reference; the definition is
        DeviceFlow.upsample_convex's.  One upload, one launch, one download."""
        weights, factor = dev.upsample_weights_array(weights, factor, self.shape)
        vecs, mask = dev.upsample_host(self._vecs, self._mask, weights, factor)
        return Flow(vecs, self._ref, mask)

    def _splat_host(self, what, array, layout, mode, importance, alpha, min_weight, frac_bits, want_weight, want_counters):
        """the host half of splat / coverage / project: checks, then one upload, the launches of K20, one download"""
        if self._ref != 's':
            raise ValueError("Error splatting: {} pushes values forward along an 's'-reference flow; a 't'-reference flow "
                             "warps backward, with apply".format(what))
        code, alpha, min_weight, frac_bits = dev.splat_args(mode, importance is not None, alpha, min_weight, frac_bits)
        z = dev.splat_importance_array(importance, self.shape)
        n, c = 1, 0
        if array is not None:
            array, n, c, _ = dev.splat_host_array(array, layout, self.shape)
        return dev.splat_host(array, layout, n, c, self._vecs, self._mask, code, alpha, min_weight, frac_bits, z,
                              want_weight, want_counters)

    def splat(self, array: np.ndarray, mode: str = 'average', importance: np.ndarray = None, alpha: float = 1.0,
              min_weight: float = None, frac_bits: int = None, layout: str = 'chw', return_weight: bool = None,
              return_counters: bool = None) -> Tuple[np.ndarray, ...]:
        """Forward-warp `array`, a float32 or float16 array (C, H, W) or (N, C, H, W) -- with layout='hwc' (H, W, C) or
        (N, H, W, C) -- by splatting along this 's'-reference flow: every source pixel adds its channels to the four pixels
        around where the flow sends it, with bilinear weights.  mode 'sum', 'average' or 'softmax' (which needs
        `importance`, a float (H, W) array, and weights source pixel p by exp(alpha * importance[p])).  -> (array of the
        input's shape and dtype, valid bool (H, W)), plus the float32 (H, W) summed weight with `return_weight` and
        (skipped source pixels, dropped values) with `return_counters`.  The definition, with its fixed-point sums, is
        DeviceFlow.splat's; this is not the reference's 's' apply.  One upload, two or three launches, one download."""
        return_weight = dev.optional_bool(return_weight, False, "Error splatting: Return_weight needs to be a boolean")
        return_counters = dev.optional_bool(return_counters, False, "Error splatting: Return_counters needs to be a boolean")
        if array is None:
            raise TypeError("Error splatting: the tensor needs to be a numpy array, got NoneType")
        out, valid, weight, counters = self._splat_host("splat", array, layout, mode, importance, alpha, min_weight, frac_bits,
                                                        return_weight, return_counters)
        return (out, valid) + ((weight,) if return_weight else ()) + ((counters,) if return_counters else ())

    def coverage(self, importance: np.ndarray = None, alpha: float = 1.0, min_weight: float = None) -> Tuple[np.ndarray, np.ndarray]:
        """The range map of this 's'-reference flow: (weight float32 (H, W), valid bool (H, W)) -- how much bilinear weight
        lands on every pixel, and where that reaches `min_weight` (None: 2^-10).  With `importance` the weights are those
        of softmax splatting.  The definition is DeviceFlow.coverage's."""
        _, valid, weight, _ = self._splat_host("coverage", None, 'hwc', 'average' if importance is None else 'softmax', importance,
                                               alpha, min_weight, None, True, False)
        return weight, valid

    def project(self, mode: str = 'average', importance: np.ndarray = None, alpha: float = 1.0, min_weight: float = None) -> FlowAlias:
        """This 's'-reference flow carried to the other frame by splatting its own vectors: a 't'-reference Flow whose mask
        is set where enough weight arrived; fill() closes the holes.  Cheaper than switch_ref and not the same function: see
        DeviceFlow.project."""
        if mode == 'sum':
            raise ValueError("Error splatting: project takes mode 'average' or 'softmax': a sum of vectors is not a flow")
        vecs = np.ascontiguousarray(self._vecs, np.float32)
        out, valid, _, _ = self._splat_host("project", vecs, 'hwc', mode, importance, alpha, min_weight, None, False, False)
        return Flow(out, 't', valid)

    def combine_with(self, flow: FlowAlias, mode: int, thresholded: bool = None) -> FlowAlias:
        """flow_1 (+) flow_2 = flow_3: mode k returns flow_k from the other two (`self` comes first in
        that formula among the two given).  Reference flow_class.py:1247-1424."""
        if not isinstance(flow, Flow):
            raise TypeError("Error combining flows: Flow need to be of type 'Flow'")
        if self.shape != flow.shape:
            raise ValueError("Error combining flows: Flow fields need to have the same shape")
        if self.ref != flow.ref:
            raise ValueError("Error combining flows: Flow fields need to have the same reference")
        if mode not in [1, 2, 3]:
            raise ValueError("Error combining flows: Mode needs to be 1, 2 or 3")
        thresholded = dev.optional_bool(thresholded, False, "Error combining flows: Thresholded needs to be a boolean")

        d_self, d_flow = self.to_device(), flow.to_device()
        res = d_self.combine_with(d_flow, mode, thresholded)
        if res is d_flow:                      # zero-flow early exits hand back the operand itself
            return flow
        if res is d_self:
            return self
        return Flow.from_device(res)
