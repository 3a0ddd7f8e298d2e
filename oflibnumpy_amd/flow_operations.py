"""Array-in / array-out wrappers over the `Flow` hot-path methods (masks are dropped), with the same
names and signatures as the reference's src/oflibnumpy/flow_operations.py:70-284.
Of its visualisation helpers only the arrow and window ones (visualise_definition, visualise_flow_arrows, show_flow,
show_flow_arrows) stay out of scope: they are cv2 drawing and GUI work.  visualise_flow renders on the device."""
from typing import Union

import numpy as np

from .flow_class import Flow

nd = np.ndarray
__all__ = ['combine_flows', 'switch_flow_ref', 'invert_flow', 'valid_target', 'valid_source', 'get_flow_padding',
           'get_flow_matrix', 'visualise_flow', 'flow_consistency', 'flow_error', 'fill_flow', 'median_flow',
           'upsample_flow_convex', 'correlation_lookup', 'global_match', 'splat_flow', 'photometric_error', 'census_error',
           'ssim_error', 'refine_flow', 'inverse_search_flow', 'estimate_flow', 'halve_tensor', 'combine_flow_sequence']


def combine_flows(input_1: Union[Flow, nd], input_2: Union[Flow, nd], mode: int, ref: str = None,
                  thresholded: bool = None) -> Union[Flow, nd]:
    """flow_1 (+) flow_2 = flow_3; `mode` k computes flow_k from the two inputs (in formula order).
    Arrays in -> array out; two Flow objects are still accepted (reference flow_operations.py:153-161)."""
    if isinstance(input_1, Flow) and isinstance(input_2, Flow):
        print("AVOID - future deprecation warning: using combine_flows(flow_obj1, flow_obj2) is deprecated and may "
              "not work anymore in future versions - use flow_obj1.combine_with(flow_obj2) instead. combine_flows() "
              "will be reserved for use with NumPy arrays only.")
        return input_1.combine_with(input_2, mode=mode, thresholded=thresholded)
    return Flow(input_1, ref).combine_with(Flow(input_2, ref), mode=mode, thresholded=thresholded).vecs


def switch_flow_ref(flow: nd, input_ref: str) -> nd:
    """Vectors recalculated for the other reference (reference flow_operations.py:164-174)."""
    return Flow(flow, input_ref).switch_ref().vecs


def invert_flow(flow: nd, input_ref: str, output_ref: str = None) -> nd:
    """Inverse flow vectors (reference flow_operations.py:177-189)."""
    output_ref = input_ref if output_ref is None else output_ref
    return Flow(flow, input_ref).invert(output_ref).vecs


def valid_target(flow: nd, ref: str) -> nd:
    """Boolean valid area in the target domain (reference flow_operations.py:192-210)."""
    return Flow(flow, ref).valid_target()


def valid_source(flow: nd, ref: str) -> nd:
    """Boolean valid area in the source domain (reference flow_operations.py:213-228)."""
    return Flow(flow, ref).valid_source()


def get_flow_padding(flow: nd, ref: str) -> list:
    """Padding [top, bottom, left, right] needed to keep every warped pixel (reference flow_operations.py:231-248)."""
    return Flow(flow, ref).get_padding()


def get_flow_matrix(flow: nd, ref: str, dof: int = None, method: str = None) -> nd:
    """(3, 3) matrix fitted to a flow array: dof 4 / 6 / 8, method 'lms' / 'ransac' / 'lmeds' (reference
    flow_operations.py:251-271)."""
    return Flow(flow, ref).matrix(dof=dof, method=method)


def visualise_flow(flow: nd, mode: str, range_max: float = None) -> nd:
    """uint8 (H, W, 3) 'rgb' / 'bgr' / 'hsv' image of a flow array (reference flow_operations.py:274-284)."""
    return Flow(flow).visualise(mode=mode, range_max=range_max)


def flow_consistency(forward: nd, backward: nd, ref: str, alpha: float = None, beta: float = None) -> tuple:
    """(consistent, covered) bool (H, W) masks of the forward-backward check of two flow arrays (Flow.consistency)."""
    return Flow(forward, ref).consistency(Flow(backward, ref), alpha=alpha, beta=beta)


def flow_error(est: nd, gt: nd, ref: str, gt_mask: nd = None, thresholds=None, outlier=None, speed_edges=None,
               return_map: bool = None):
    """FlowErrorStats of the estimated flow array `est` against the ground-truth array `gt` with its validity mask
    `gt_mask` (None: all valid) -- Flow.error; with `return_map` also the float32 (H, W) end-point error."""
    return Flow(est, ref).error(Flow(gt, ref, gt_mask), thresholds=thresholds, outlier=outlier, speed_edges=speed_edges,
                                return_map=return_map)


def fill_flow(flow: nd, mask: nd, valid: nd = None, max_dist: float = None) -> tuple:
    """(vecs, mask) of the flow array `flow` with the vectors outside `mask` (and outside `valid`, if given) replaced by the
    vector of the nearest pixel inside, within `max_dist` px (None: no limit) -- Flow.fill; the returned bool mask is True
    where a pixel was filled.  Not a function of the reference."""
    filled = Flow(flow, 't', mask).fill(valid=valid, max_dist=max_dist)
    return filled.vecs, filled.mask


def median_flow(flow: nd, mask: nd, ksize: int = 5, valid: nd = None, only: nd = None, min_count: int = None) -> tuple:
    """(vecs, mask) of the flow array `flow` median-filtered over a ksize x ksize window (3, 5 or 7) among the
    pixels inside `mask` (and inside `valid`, if given), at the pixels where `only` is set (None: everywhere), with at
    least `min_count` (None: 1) members per window -- Flow.median.  Not a function of the reference."""
    filtered = Flow(flow, 't', mask).median(ksize=ksize, valid=valid, only=only, min_count=min_count)
    return filtered.vecs, filtered.mask


def upsample_flow_convex(flow: nd, mask: nd, weights: nd, factor: int = 8) -> tuple:
    """(vecs, mask) of the coarse flow array `flow` (h, w, 2) convexly upsampled by `factor` (2, 4 or 8) with the mask
    logits `weights`, a float32 or float16 array (9 factor^2, h, w) in RAFT's channel order -- Flow.upsample_convex.  Not a
    function of the reference."""
    fine = Flow(flow, 't', mask).upsample_convex(weights, factor=factor)
    return fine.vecs, fine.mask


def correlation_lookup(fmap1: nd, fmap2: nd, flow: nd = None, ref: str = 's', radius: int = 4, levels: int = 1,
                       scale: float = None, order: str = 'xy') -> nd:
    """The correlation of the feature maps `fmap1` and `fmap2`, float32 or float16 arrays (C, H, W), looked up around
    x + flow (ref 's') or x - flow (ref 't') on `levels` pyramid levels of fmap2 within `radius` (1 ... 4) -- RAFT's
    CorrBlock without the all-pairs volume; DeviceCorrelation.lookup with the exact taps of grid_sample.  flow: a float32
    array (H, W, 2) in pixels of the feature grid, or None for the window around the pixel itself.  scale: None for
    1 / sqrt(C).  order: 'xy' (RAFT's channel order) or 'yx' (row-major).  -> float32 (levels (2 radius + 1)^2, H, W).
    One upload, `levels` launches, one download."""
    from . import device as dev
    from .utils import get_valid_ref
    sign = 1 if get_valid_ref(ref) == 's' else -1
    f1, shape1 = dev.corr_host_array(fmap1, "fmap1")
    f2, shape2 = dev.corr_host_array(fmap2, "fmap2")
    if shape1 != shape2:
        raise ValueError("Error looking up correlation: the feature maps need the same shape, got {} and {}".format(shape1, shape2))
    radius, levels, scale, order, quant = dev.corr_args(radius, levels, scale, order, dev.nat.QUANT_EXACT, shape1[0], shape1[1:])
    if flow is not None:
        if not isinstance(flow, np.ndarray):
            raise TypeError("Error looking up correlation: flow needs to be a numpy array or None, got {}".format(type(flow).__name__))
        if flow.shape != shape1[1:] + (2,):
            raise ValueError("Error looking up correlation: flow needs to have shape {}, got {}".format(shape1[1:] + (2,), flow.shape))
        flow = np.ascontiguousarray(flow, np.float32)
    return dev.corr_lookup_host(f1, f2, flow, sign, radius, levels, scale, order, quant)[0]


def global_match(fmap1: nd, fmap2: nd, ref: str = 's', scale: float = None, min_confidence: float = None,
                 return_confidence: bool = False, return_index: bool = False):
    """The global match of the feature maps `fmap1` and `fmap2`, arrays (C, H, W) of ONE dtype, float32 or float16: every
    pixel of fmap1 is dotted with every pixel of fmap2, a softmax runs over all H W candidates and the flow is the expected
    coordinate minus the pixel's own -- GMFlow's global matching without the all-pairs volume; DeviceCorrelation.match.
    ref 's': pixel + flow is the match; 't': its negation.  scale: None for 1 / sqrt(C).  The mask of the returned Flow is set
    where the confidence (the softmax probability of the best candidate) is at least `min_confidence` (None: everywhere).
    -> a Flow; with return_confidence / return_index a tuple that also holds the float32 (H, W) confidence and the int32
    (H, W) row-major index of the best candidate.  One upload, one launch, one download."""
    from . import device as dev
    from .utils import get_valid_ref
    ref = get_valid_ref(ref)
    want = [dev.optional_bool(v, False, "Error matching features: {} needs to be a boolean".format(name))
            for name, v in (("return_confidence", return_confidence), ("return_index", return_index))]
    f1, shape1 = dev.match_host_array(fmap1, "fmap1")
    f2, shape2 = dev.match_host_array(fmap2, "fmap2")
    if shape1 != shape2:
        raise ValueError("Error matching features: the feature maps need the same shape, got {} and {}".format(shape1, shape2))
    scale, min_conf = dev.match_args(scale, min_confidence, shape1[0], f1.dtype.name, f2.dtype.name)
    vecs, mask, conf, index = dev.match_host(f1, f2, scale, 1 if ref == 's' else -1, min_conf, want[0], want[1])
    flow = Flow(vecs[0], ref, mask[0])
    extra = tuple(x[0] for x, wanted in ((conf, want[0]), (index, want[1])) if wanted)
    return (flow,) + extra if extra else flow


def splat_flow(flow: nd, target: nd, mask: nd = None, mode: str = 'average', importance: nd = None, alpha: float = 1.0,
               min_weight: float = None, frac_bits: int = None, layout: str = 'chw') -> tuple:
    """(array, valid) of `target`, a float32 or float16 array (C, H, W) or (N, C, H, W) -- with layout='hwc' (H, W, C) or
    (N, H, W, C) --, forward-warped by splatting along the 's'-reference flow array `flow` (H, W, 2) with the mask `mask`
    (None: all valid) -- Flow.splat: mode 'sum', 'average' or 'softmax' with the float (H, W) array `importance`.  Not the
    reference's 's' apply."""
    return Flow(flow, 's', mask).splat(target, mode=mode, importance=importance, alpha=alpha, min_weight=min_weight,
                                       frac_bits=frac_bits, layout=layout)


def photometric_error(flow: nd, near: nd, far: nd, ref: str = None, mask: nd = None, metric: str = 'l1', eps: float = None,
                      threshold: float = None, near_mask: nd = None, far_mask: nd = None, layout: str = 'hwc') -> tuple:
    """(error, covered) -- a float32 map and a bool array, plus the bool array `within` with `threshold` -- of the
    photometric error of the flow array `flow` (H, W, 2) with reference `ref` and mask `mask` (None: all valid): `near`, the
    image or feature array of the flow's own frame, against `far`, that of the other frame, sampled where the flow points
    -- Flow.photometric: metric 'l1', 'l2' or 'charbonnier'; arrays (H, W), (H, W, C) or, with layout='chw', (C, H, W)."""
    return Flow(flow, ref, mask).photometric(near, far, metric=metric, eps=eps, threshold=threshold, near_mask=near_mask,
                                             far_mask=far_mask, layout=layout)


def census_error(flow: nd, near: nd, far: nd, ref: str = None, mask: nd = None, window: int = 7, mode: str = 'soft',
                 delta: float = None, noise: float = None, knee: float = None, min_count: int = None, threshold: float = None,
                 near_mask: nd = None, far_mask: nd = None, layout: str = 'hwc') -> tuple:
    """(error, covered) -- a float32 map and a bool array, plus the bool array `within` with `threshold` -- of the census
    distance of the flow array `flow` (H, W, 2) with reference `ref` and mask `mask` (None: all valid): the order of the
    intensities in a window around each pixel of `near`, the image of the flow's own frame, against that in `far`, sampled
    where the flow points -- Flow.census: mode 'hard' or 'soft', window 3, 5 or 7; arrays (H, W), (H, W, C) or, with
    layout='chw', (C, H, W), 1 to 4 channels."""
    return Flow(flow, ref, mask).census(near, far, window=window, mode=mode, delta=delta, noise=noise, knee=knee,
                                        min_count=min_count, threshold=threshold, near_mask=near_mask, far_mask=far_mask,
                                        layout=layout)


def ssim_error(flow: nd, near: nd, far: nd, ref: str = None, mask: nd = None, window: int = 11, weights: str = 'gaussian',
               sigma: float = None, data_range: float = 255.0, k1: float = 0.01, k2: float = 0.03, min_count: int = None,
               threshold: float = None, near_mask: nd = None, far_mask: nd = None, layout: str = 'hwc') -> tuple:
    """(error, covered) -- a float32 map and a bool array, plus the bool array `within` with `threshold` -- of the structural
    dissimilarity (1 - SSIM) / 2 of the flow array `flow` (H, W, 2) with reference `ref` and mask `mask` (None: all valid):
    Wang et al.'s SSIM in a weighted window around each pixel of `near`, the image of the flow's own frame, against `far`,
    sampled where the flow points -- Flow.ssim: weights 'gaussian' or 'uniform', window 3, 5, 7 or 11; arrays (H, W),
    (H, W, C) or, with layout='chw', (C, H, W), 1 to 4 channels."""
    return Flow(flow, ref, mask).ssim(near, far, window=window, weights=weights, sigma=sigma, data_range=data_range, k1=k1,
                                      k2=k2, min_count=min_count, threshold=threshold, near_mask=near_mask, far_mask=far_mask,
                                      layout=layout)


def refine_flow(flow: nd, near: nd, far: nd, ref: str = None, mask: nd = None, alpha: float = None, delta: float = None,
                zeta: float = None, eps: float = None, fixed_point: int = None, sor: int = None, omega: float = None,
                near_mask: nd = None, far_mask: nd = None, valid: nd = None, layout: str = 'hwc', quant: int = 0) -> nd:
    """The flow array `flow` (H, W, 2) with reference `ref` and mask `mask` (None: all valid) after one variational
    refinement on `near`, the image of the flow's own frame, and `far`, that of the other frame -- Flow.refine: one warp,
    `fixed_point` updates of `sor` red-black SOR sweeps; arrays (H, W), (H, W, C) or, with layout='chw', (C, H, W).
    -> the refined float32 (H, W, 2) array."""
    return Flow(flow, ref, mask).refine(near, far, alpha=alpha, delta=delta, zeta=zeta, eps=eps, fixed_point=fixed_point, sor=sor,
                                        omega=omega, near_mask=near_mask, far_mask=far_mask, valid=valid, layout=layout,
                                        quant=quant).vecs


def inverse_search_flow(flow: nd, near: nd, far: nd, ref: str = None, mask: nd = None, patch: int = 8, stride: int = 4,
                        iterations: int = 12, normalise: bool = True, floor: float = 1.0, layout: str = 'hwc',
                        quant: int = 1) -> nd:
    """The flow array `flow` (H, W, 2) with reference `ref` and mask `mask` (None: all valid) after one dense inverse search
    on `near`, the image of the flow's own frame, and `far`, that of the other frame -- Flow.inverse_search: patches of
    `patch` on a grid of `stride`, `iterations` Lucas-Kanade steps each, then the weighted average per pixel; arrays (H, W),
    (H, W, C) or, with layout='chw', (C, H, W).  -> the float32 (H, W, 2) array; where the average is not finite it is 0."""
    return Flow(flow, ref, mask).inverse_search(near, far, patch=patch, stride=stride, iterations=iterations, normalise=normalise,
                                                floor=floor, layout=layout, quant=quant).vecs


def estimate_flow(img1: nd, img2: nd, ref: str = 't', levels: int = None, patch: int = 8, stride: int = 4,
                  iterations: int = 12, refine: bool = True, refine_args: dict = None, init: Union[Flow, nd] = None,
                  layout: str = 'hwc') -> Flow:
    """The flow from `img1` to `img2`, estimated without a network: Dense Inverse Search, coarse to fine over a pyramid of
    2 x 2 means, with a variational refinement at every level (device.estimate_flow: K24 and K23 on the device, one upload
    and one download).  img1, img2: arrays (H, W), (H, W, C) or, with layout='chw', (C, H, W) of uint8, float32 or float16
    with 1 to 4 channels; intensities 0 ... 255 are what the defaults are meant for.  ref: 't' (vectors sit on the pixels of
    img2) or 's' (on those of img1).  levels: 1 ... 6 or None for the largest count the size allows; H and W must be divisible
    by 2^(levels - 1) and the coarsest level at least 2 patch wide and high, else a ValueError (pad first).  init: a Flow or
    an (H, W, 2) array to start from, or None.  -> a Flow of reference `ref`."""
    from . import device as dev
    from .utils import get_valid_ref
    prefix = "Error estimating flow: "
    ref = get_valid_ref(ref)
    a, b = dev.photometric_host_array(img1, layout, "img1", prefix), dev.photometric_host_array(img2, layout, "img2", prefix)
    if a.shape != b.shape:
        raise ValueError("{}the images need the same shape, got {} and {}".format(prefix, a.shape, b.shape))
    if a.dtype != b.dtype:
        raise TypeError("{}the images need the same dtype, got {} and {}".format(prefix, a.dtype, b.dtype))
    n, c, h, w, batched = dev.tensor_args(dev.tensor_logical_shape(a.shape, layout), layout, a.dtype.name)
    dev.inverse_search_channels(c)
    if n != 1:
        raise ValueError("{}two images make one flow, got {} items".format(prefix, n))
    dev.estimate_levels((h, w), levels, dev.inverse_search_args(patch, stride, iterations)[0])
    if init is not None:
        init = init if isinstance(init, Flow) else Flow(init, ref)
        if init.ref != ref or tuple(init.shape) != (h, w):
            raise ValueError("{}init needs the shape {} and the reference '{}'".format(prefix, (h, w), ref))
        init = dev.DeviceFlow.from_host(init.vecs, ref, init.mask)
    near, far = (a, b) if ref == 's' else (b, a)
    out = dev.estimate_flow(dev.DeviceTensor.from_host(near, layout), dev.DeviceTensor.from_host(far, layout), ref, levels,
                            patch, stride, iterations, refine, refine_args, init)
    vecs, mask = out.to_host()
    return Flow(vecs, ref, mask)


def combine_flow_sequence(flows, ref: str = None, masks: nd = None, quant: int = 0, return_partials: bool = False,
                          return_lost_at: bool = False):
    """The consecutive flows of a sequence -- flow k maps frame k to frame k + 1 -- accumulated into ONE long-range Flow
    (DeviceFlowBatch.combine_sequence: K25, one upload, one launch, one download): mode 3 of combine_with folded over the
    sequence without its zero-flow early exits,
        ref 's':  F <- F.combine_with(flow_k, 3)  for k = 1 ... n - 1
        ref 't':  G <- flow_k.combine_with(G, 3)  for k = n - 2 ... 0
    For 't' this right fold is the only association that is a per-pixel walk; the left fold, ((f_0 (+) f_1) (+) f_2) ...,
    interpolates the accumulated field and is NOT what this computes.  flows: a list of Flow objects of one shape and
    reference, or an (n, H, W, 2) array with the reference `ref` and optional (n, H, W) `masks` (None: all valid).
    -> a Flow; return_partials appends a list of n Flows, the accumulated flow after each step at the index of the flow
    taken last ('s': entry k composes flows 0 ... k; 't': entry k composes flows k ... n - 1); return_lost_at an int32
    (H, W) array, the index of the flow at which the pixel's mask first became False, -1 where it is True at the end.
    Not a function of the reference, whose users write the loop of combine_with calls."""
    from . import device as dev
    prefix = dev.SEQUENCE_PREFIX
    if isinstance(flows, np.ndarray):
        if flows.ndim != 4 or flows.shape[3] != 2 or flows.shape[0] == 0:
            raise ValueError("{}Flows need to be a numpy array of shape (n, H, W, 2), n > 0, got {}".format(prefix, flows.shape))
        if masks is not None:
            if not isinstance(masks, np.ndarray):
                raise TypeError("{}Masks need to be a numpy array or None".format(prefix))
            if masks.shape != flows.shape[:3]:
                raise ValueError("{}Masks need to have shape {}, got {}".format(prefix, flows.shape[:3], masks.shape))
        flows = [Flow(flows[k], ref, None if masks is None else masks[k]) for k in range(flows.shape[0])]
    elif isinstance(flows, (list, tuple)):
        if not flows:
            raise ValueError("{}Flows need to hold at least one flow".format(prefix))
        if not all(isinstance(f, Flow) for f in flows):
            raise TypeError("{}Flows need to be a list of Flow objects or a numpy array".format(prefix))
        if masks is not None:
            raise ValueError("{}Masks go with a numpy array of flows; Flow objects carry their own".format(prefix))
        if any(f.shape != flows[0].shape for f in flows):
            raise ValueError("{}Flow fields need to have the same shape".format(prefix))
        if any(f.ref != flows[0].ref for f in flows):
            raise ValueError("{}Flow fields need to have the same reference".format(prefix))
    else:
        raise TypeError("{}Flows need to be a list of Flow objects or a numpy array".format(prefix))
    _, _, quant, return_partials, return_lost_at = dev.sequence_args(len(flows), None, quant, return_partials, return_lost_at)
    ref = flows[0].ref
    out, mout, pv, pm, lost = dev.sequence_host(np.stack([f.vecs for f in flows]), np.stack([f.mask for f in flows]),
                                                1 if ref == 's' else -1, return_partials, return_lost_at, quant)
    res = (Flow(out, ref, mout),)
    if return_partials:
        res += ([Flow(pv[k], ref, pm[k]) for k in range(len(flows))],)
    if return_lost_at:
        res += (lost,)
    return res if len(res) > 1 else res[0]


def halve_tensor(arr: nd, layout: str = 'chw') -> nd:
    """The 2 x 2 mean of a float32 or float16 array in the memory order of `layout` -- (C, H, W) / (N, C, H, W) for 'chw',
    (H, W, C) / (N, H, W, C) for 'hwc' --: ((tl + tr) + (bl + br)) * 0.25 in float32, rounded once to the dtype; an odd last
    row or column is dropped (DeviceTensor.halve: one upload, one launch, one download)."""
    from . import device as dev
    return dev.DeviceTensor.from_host(arr, layout).halve().to_host()
