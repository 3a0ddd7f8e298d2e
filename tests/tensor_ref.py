"""NumPy statement of K12 (oflibnumpy_amd/csrc/ofl_tensor.hip) on top of the oracle -- a helper of test_tensor_host.py and
test_gpu_tensor.py, not a test.

A C-channel float warp is C one-channel warps: per item and channel the plane goes, as float32, through the oracle's
Flow.apply (`OFlow.apply(..., return_valid_area=True)`, flow_class.py:604-695) -- or, for QUANT_EXACT, through
`gather_bilinear(quant=QUANT_EXACT)` ANDed with the flow mask.  16-bit tensors enter through interop_ref.to_f32 (exact) and
leave through interop_ref.from_f32 (one rounding to nearest even); bfloat16 travels as uint16 bit patterns."""
import numpy as np

import interop_ref as R
from oracle import np_oracle as O

DTYPES = ['float32', 'float16', 'bfloat16']
LAYOUTS = ['chw', 'hwc']
FLOWS = ['wobble', 'rotation', 'integer', 'half', 'outside']


def raw(a):
    """the bit patterns of a tensor array, so that -0.0, NaN payloads and bfloat16 patterns compare as they are"""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.itemsize])


def to_planar(arr, layout):
    """an array in the memory order of `layout`, 3 or 4 dimensions -> (N, C, H, W)"""
    a = arr if arr.ndim == 4 else arr[None]
    return a if layout == 'chw' else np.moveaxis(a, -1, 1)


def from_planar(planar, layout, batched):
    a = planar if layout == 'chw' else np.moveaxis(planar, 1, -1)
    return np.ascontiguousarray(a if batched else a[0])


def values(mem_shape, dtype, seed=0):
    """a finite test tensor (bfloat16: uint16 patterns, no infinities) that starts with interop_ref's special values;
    float32 stays within +-1e4 so that no blend overflows"""
    a = R.flow_values(mem_shape, dtype, seed)
    if dtype == 'float32':
        a = np.clip(a, -1e4, 1e4)
    if dtype == 'bfloat16':
        a = a & np.uint16(0xbfff)           # exponent below 2^1: keeps every blend far from overflow
    return a


def flow(name, shape, seed=0):
    """the test fields, reference 't' (the warp samples at grid - flow)"""
    h, w = shape
    if name == 'wobble':
        y, x = np.mgrid[:h, :w].astype('f')
        a, b = np.random.default_rng(seed).uniform(40, 130, 2)
        return np.stack([3 * np.sin(2 * np.pi * x / a) * np.cos(2 * np.pi * y / b),
                         3 * np.cos(2 * np.pi * x / b) * np.sin(2 * np.pi * y / a)], -1).astype('f')
    if name == 'rotation':                  # 30 degrees about the centre: taps leave the frame on all four sides
        m = O.matrix_from_transforms([['rotation', (w - 1) / 2, (h - 1) / 2, 30]])
        # (built two pixels wide at least and cropped: flow_from_matrix squeezes an axis of length 1 away)
        return np.ascontiguousarray(O.flow_from_matrix(m, (max(h, 2), max(w, 2)), 't')[:h, :w])
    v = {'integer': (2.0, -1.0), 'half': (1.5, -0.5), 'outside': (w + 3.0, -(h + 2.0))}[name]
    return np.broadcast_to(np.array(v, np.float32), (h, w, 2)).copy()


def mask(shape, seed, p=0.05):
    return np.random.default_rng(seed).random(shape) > p


def warp(arr, dtype, layout, vecs, fmask=None, target_mask=None, quant=O.QUANT_OPENCV):
    """The warp of a tensor `arr` (memory order of `layout`, `dtype`) -> (warped array of the same kind, valid bool).
    vecs (H, W, 2) warps every item, or (N, H, W, 2) item by item; fmask / target_mask (H, W) or (N, H, W) or None.
    valid is (H, W) when field and target mask are shared, else (N, H, W)."""
    planar = R.to_f32(to_planar(arr, layout), dtype)
    n, c, h, w = planar.shape
    pick = lambda a, i, nd: None if a is None else (a[i] if a.ndim == nd + 1 else a)
    per_item = vecs.ndim == 4 or (target_mask is not None and target_mask.ndim == 3)
    out = np.empty_like(planar)
    valid = np.empty((n, h, w), bool)
    for i in range(n):
        v, fm, tm = pick(vecs, i, 3), pick(fmask, i, 2), pick(target_mask, i, 2)
        for k in range(c):
            plane = np.ascontiguousarray(planar[i, k])
            if quant == O.QUANT_OPENCV:
                res, ok = O.OFlow(v, 't', fm).apply(plane, tm, return_valid_area=True)
            else:
                res, ok = O.gather_bilinear(plane, v, -1, smask=tm, want_valid=True, quant=O.QUANT_EXACT)
                ok = ok & (np.ones((h, w), bool) if fm is None else fm.astype(bool))
            out[i, k] = res
            if k == 0:
                valid[i] = ok
            else:
                assert np.array_equal(valid[i], ok)
    return from_planar(R.from_f32(out, dtype), layout, arr.ndim == 4), (valid if per_item else valid[0])
