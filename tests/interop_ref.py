"""NumPy restatement of the K11 kernels (oflibnumpy_amd/csrc/ofl_interop.hip) -- a helper of test_interop_host.py and
test_gpu_interop.py, not a test.

The layout moves are transposes, the conversions are NumPy's own astype (float16 / float64 <-> float32: to nearest even,
overflow to inf) except bfloat16, which NumPy does not have: it is stated on the bit pattern here and pinned to torch on the
CPU by test_interop_host.py.  bfloat16 arrays travel as uint16 bit patterns."""
import numpy as np

SHAPES = [(1, 1), (1, 5), (5, 7), (3, 130), (2, 1030)]        # (2, 1030): a row crosses the 1024 pixels of a workgroup
FLOW_DTYPES = ['float16', 'bfloat16', 'float32', 'float64']
IMAGE_DTYPES = ['uint8', 'int16', 'uint16', 'float32', 'float64']


def bits(a):
    """float32 -> uint32 bit patterns, so that -0.0 and NaN payloads count in comparisons"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bf16_to_f32(b):
    """bfloat16 bit patterns (uint16) -> float32: exact, the pattern moves to the upper half"""
    return (np.asarray(b).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16(a):
    """float32 -> bfloat16 bit patterns (uint16), round to nearest even on the bit pattern: add 0x7fff plus the lowest kept
    bit, drop the lower half.  Overflow carries into the exponent and gives inf; every NaN becomes 0x7fc0 (what torch gives)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r[(u & 0x7fffffff) > 0x7f800000] = 0x7fc0
    return r


def to_f32(arr, dtype):
    """a source array of `dtype` (bfloat16: uint16 patterns) -> float32 as the import kernel converts it"""
    if dtype == 'bfloat16':
        return bf16_to_f32(arr)
    with np.errstate(over='ignore'):
        return np.asarray(arr).astype(np.float32)


def from_f32(a, dtype):
    """float32 -> `dtype` as the export kernel converts it (bfloat16: uint16 patterns)"""
    if dtype == 'bfloat16':
        return f32_to_bf16(a)
    with np.errstate(over='ignore'):
        return np.asarray(a, np.float32).astype(dtype)


def import_flow(arr, layout, dtype):
    """(..., H, W, 2) 'hwc' or (..., 2, H, W) 'chw' of `dtype` -> float32 (..., H, W, 2)"""
    v = to_f32(arr, dtype)
    return np.ascontiguousarray(np.moveaxis(v, -3, -1) if layout == 'chw' else v)


def export_flow(vecs, layout, dtype):
    """float32 (..., H, W, 2) -> `dtype` in `layout`, C-contiguous"""
    v = from_f32(vecs, dtype)
    return np.ascontiguousarray(np.moveaxis(v, -1, -3) if layout == 'chw' else v)


def to_hwc(img):
    return np.ascontiguousarray(np.moveaxis(img, 0, -1))


def to_chw(img):
    return np.ascontiguousarray(np.moveaxis(img, -1, 0))


# values every conversion has to get right, planted at the start of each test array
_F16_BITS = [0x0001, 0x03ff, 0x8001, 0x0400, 0x7bff, 0xfbff, 0x8000, 0x3c00, 0x3c01]       # subnormals, smallest normal, +-65504, -0
_F32 = [65504.0, 65519.99, 65520.0, 70000.0, -1e5, 3.3e38, -3.4e38,                         # export overflow: to inf from 65520 on
        1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20,                   # ties (and just above) in float32 -> float16
        1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8 + 2.0 ** -20),                   # ... in float32 -> bfloat16
        2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 6.1e-5, 1e-7, -0.0, 1e-40]                  # half subnormals and below, a float32 subnormal
_F64 = [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50, -(1 + 2.0 ** -24),  # ties (and just above) in float64 -> float32
        1e-40, 1e-46, 2.0 ** -150, 3 * 2.0 ** -150, 3.3e38, -0.0, 0.1]                        # float32 subnormals, underflow


def flow_values(shape, dtype, seed=0):
    """A finite test array of `shape` and `dtype` (bfloat16: uint16 patterns) that starts with the special values."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if dtype == 'bfloat16':
        flat = rng.integers(0, 1 << 16, n, dtype=np.uint16)
        flat[(flat & 0x7f80) == 0x7f80] &= 0xbfff                        # no inf / NaN: clear one exponent bit
        special = np.array([0x0001, 0x007f, 0x8001, 0x0080, 0x7f7f, 0xff7f, 0x8000, 0x3f80], np.uint16)
    elif dtype == 'float16':
        flat = (rng.standard_normal(n) * 5).astype(np.float16)
        special = np.array(_F16_BITS, np.uint16).view(np.float16)
    elif dtype == 'float32':
        flat = (rng.standard_normal(n) * 5).astype(np.float32)
        special = np.array(_F32, np.float32)
    else:
        flat = rng.standard_normal(n) * 5
        special = np.array(_F64, np.float64)
    k = min(n, special.size)
    flat[:k] = special[:k]
    return flat.reshape(shape)


def cai_dict(view, ptr, version=3, stream=None):
    """the __cuda_array_interface__ of a NumPy view whose first element lives at device address `ptr`: NumPy's own shape,
    typestr and byte strides"""
    d = {"version": version, "shape": tuple(view.shape), "typestr": view.dtype.str, "data": (int(ptr), False),
         "strides": None if view.flags.c_contiguous else tuple(view.strides)}
    if version >= 3:
        d["stream"] = stream
    return d
