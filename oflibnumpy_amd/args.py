"""Host halves of the resident layer: argument checks with the reference's exception types and messages, and the small pure
tables and helpers the launch wrappers share.  Nothing here touches the device: the module imports -- and every function
in it runs -- without the native library.
"""
import numpy as np

from . import _native as nat

DEFAULT_THRESHOLD = 1e-3          # src/oflibnumpy/utils.py:22
_DT_CODE = {np.dtype('uint8'): nat.U8, np.dtype('int16'): nat.I16, np.dtype('uint16'): nat.U16,
            np.dtype('float32'): nat.F32, np.dtype('float64'): nat.F64}
_TRACK_DT = {np.dtype('float64'): nat.TRACK_F64, np.dtype('int32'): nat.TRACK_I32, np.dtype('int64'): nat.TRACK_I64}
_TENSOR_EL = {'float32': nat.EL_F32, 'float16': nat.EL_F16, 'bfloat16': nat.EL_BF16}
_TENSOR_LAYOUT = {'chw': nat.TENSOR_NCHW, 'hwc': nat.TENSOR_NHWC}


def remap_rules(dtype, masked):
    """(arith, rule) of an image gather: how the kernel reproduces the dtype of the reference's "concatenated array", the
    image with its mask appended as one more channel for cv2.remap (flow_class.py:615, :626, :644-650).  `masked`: a target
    mask is given -- a bool mask concatenates to the image's own dtype, the default int8 one widens uint8 to int16 and would
    widen uint16 to int32 (TypeError).  The ONE table behind DeviceFlow.apply_image, apply_image_rows and
    DeviceFlowBatch.apply_images."""
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return (nat.ARITH_NATIVE, nat.RULE_GE_HALF) if masked else (nat.ARITH_FLOAT_RNE, nat.RULE_GT_HALF)
    if dtype == np.int16 or (dtype == np.uint16 and masked):
        return nat.ARITH_NATIVE, nat.RULE_GT_HALF
    if dtype == np.uint16:
        raise TypeError("uint16 image with the default int8 mask needs an int32 remap, which cv2.remap does not provide")
    return nat.ARITH_NATIVE, nat.RULE_EQ1


def mask_bytes(mask):
    """A host mask -> contiguous uint8: bool is viewed, anything else cast."""
    m = np.ascontiguousarray(mask)
    return m.view(np.uint8) if m.dtype == np.bool_ else m.astype(np.uint8)


def optional_bool(value, default, message):
    """An optional boolean argument -> bool: None gives `default`, anything but a bool is TypeError(message)."""
    value = default if value is None else value
    if not isinstance(value, bool):
        raise TypeError(message)
    return value


def _is_integer(value):
    """an integer, Python's or NumPy's, and not a bool"""
    return isinstance(value, (int, np.integer)) and not isinstance(value, (bool, np.bool_))


def mask_array_arg(array, shape, prefix, name):
    """A host array given as a mask argument `name` (the `valid` of Flow.fill, the `valid` or `only` of Flow.median) ->
    contiguous uint8 (H, W): a NumPy array of bool or uint8 with the shape of the flow (TypeError for another type or
    dtype, ValueError for another shape).  `prefix` opens the message, e.g. "Error filling flow: "."""
    if not isinstance(array, np.ndarray):
        raise TypeError("{}{} needs to be a numpy array, got {}".format(prefix, name, type(array).__name__))
    if array.dtype != np.bool_ and array.dtype != np.uint8:
        raise TypeError("{}{} needs to have dtype bool or uint8, got {}".format(prefix, name, array.dtype))
    if array.shape != (shape[0], shape[1]):
        raise ValueError("{}{} needs to have the shape of the flow, got {} and {}"
                         .format(prefix, name, array.shape, (shape[0], shape[1])))
    return mask_bytes(array)


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


# -- build / scale / pad / crop: the host halves of the DeviceFlow constructors and operators
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


def valid_mask_array(mask, shape):
    """A host array given as a constructor's `mask`, checked like the Flow.mask setter (flow_class.py:142-161) -> uint8 (H, W)."""
    if not isinstance(mask, np.ndarray):
        raise TypeError("Error setting flow mask: Input is not a numpy array")
    if mask.ndim != 2:
        raise ValueError("Error setting flow mask: Input not 2-dimensional")
    if mask.shape != (shape[0], shape[1]):
        raise ValueError("Error setting flow mask: Input has a different shape than the flow vectors")
    if ((mask != 0) & (mask != 1)).any():
        raise ValueError("Error setting flow mask: Values must be 0 or 1")
    return np.ascontiguousarray(mask.astype(np.bool_)).view(np.uint8)


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


# -- forward-backward consistency (K13)
CONSISTENCY_ALPHA, CONSISTENCY_BETA = 0.01, 0.5        # the usual constants of the check; the caller's to set


def consistency_args(alpha=None, beta=None):
    """Validation of the bound of the forward-backward check, |f + b(x + f)|^2 <= alpha * (|f|^2 + |b|^2) + beta, on the
    host before any device work -> (alpha, beta) as float32, what the kernel computes with.  None gives the defaults 0.01
    and 0.5; a bool or a non-number is a TypeError, a negative or non-finite value (as given, or once rounded to float32)
    a ValueError."""
    out = []
    for name, value, default in (("alpha", alpha, CONSISTENCY_ALPHA), ("beta", beta, CONSISTENCY_BETA)):
        value = default if value is None else value
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
            raise TypeError("Error checking flow consistency: {} must be a number, got {}".format(name, type(value).__name__))
        with np.errstate(over='ignore'):
            v32 = np.float32(float(value)) if abs(value) < 1e300 else np.float32(np.inf if value > 0 else -np.inf)
        if value != value or value < 0 or not np.isfinite(v32):
            raise ValueError("Error checking flow consistency: {} must be finite and not negative, got {}".format(name, value))
        out.append(v32)
    return out[0], out[1]


# -- a sequence of fields accumulated into one (K25)
SEQUENCE_PREFIX = "Error combining flow sequence: "


def sequence_args(n, length=None, quant=0, return_partials=False, return_lost_at=False):
    """Validation of the settings of a sequence accumulation over `n` fields, on the host before any device work
    -> (length, n_seq, quant, return_partials, return_lost_at).  length: None for one sequence of all n fields, else an int
    in 1 ... n that divides n; quant: 0 (the 1/32-px snap) or 1 (exact).  A bool or a non-integer where an integer is due,
    or a non-bool flag, is a TypeError; a value out of range a ValueError."""
    length = n if length is None else length
    for name, value in (("length", length), ("quant", quant)):
        if not _is_integer(value):
            raise TypeError("{}{} needs to be an integer, got {}".format(SEQUENCE_PREFIX, name.capitalize(), type(value).__name__))
    if length < 1 or n % length:
        raise ValueError("{}Length needs to be a positive divisor of the number of flows {}, got {}".format(SEQUENCE_PREFIX, n, length))
    if quant not in (0, 1):
        raise ValueError("{}Quant needs to be 0 (QUANT_OPENCV) or 1 (QUANT_EXACT), got {}".format(SEQUENCE_PREFIX, quant))
    return_partials = optional_bool(return_partials, False, SEQUENCE_PREFIX + "Return_partials needs to be a boolean")
    return_lost_at = optional_bool(return_lost_at, False, SEQUENCE_PREFIX + "Return_lost_at needs to be a boolean")
    return int(length), n // int(length), int(quant), return_partials, return_lost_at


# -- what the image-pair families K21 ... K24 share: their number settings, the channel limit and the two host arrays
def _float32_rounded(value, name, prefix, none_ok=True):
    """a number -> float32, +-inf where float32 cannot hold it; a bool or a non-number is a TypeError (none_ok: the caller
    takes None for a default, and the message says so)"""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise TypeError("{}{} must be a number{}, got {}".format(prefix, name, " or None" if none_ok else "", type(value).__name__))
    with np.errstate(over='ignore', under='ignore'):
        return np.float32(float(value)) if abs(value) < 1e300 else np.float32(np.inf if value > 0 else -np.inf)


def _float32_setting(value, name, prefix, positive=False, none_ok=True, note=""):
    """_float32_rounded, and a ValueError for NaN, a negative value, one that is not finite once rounded to float32 and --
    `positive` -- one that is not above 0 then; `note` follows the rule in that message"""
    v32 = _float32_rounded(value, name, prefix, none_ok)
    if value != value or value < 0 or not np.isfinite(v32) or (positive and not v32 > 0):
        raise ValueError("{}{} must be finite and {}{}, got {}".format(prefix, name, "positive" if positive else "not negative", note, value))
    return v32


def _integer_setting(value, name, prefix, lo=None, hi=None, none_ok=False):
    """an integer -> int; a bool or a non-integer is a TypeError (none_ok as above), a value outside [lo, hi] a ValueError
    (lo None: the caller checks the value, in its own words)"""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise TypeError("{}{} must be an integer{}, got {}".format(prefix, name, " or None" if none_ok else "", type(value).__name__))
    if lo is not None and not lo <= value <= hi:
        raise ValueError("{}{} must be in [{}, {}], got {}".format(prefix, name, lo, hi, value))
    return int(value)


def pair_channels(c, limit, prefix):
    """The channel count of a family that forms channel means (K22, K23, K24): 1 ... limit, else a ValueError that names it."""
    if not 1 <= c <= limit:
        raise ValueError("{}the tensors need 1 to {} channels (grey, two-plane, RGB, RGBA), got {}".format(prefix, limit, c))
    return c


def pair_host_arrays(near, far, layout, field_shape, prefix, max_c=None, one_item=False):
    """The `near` and `far` of Flow.photometric / census / refine / inverse_search -> (near, far, n, c, batched): two
    contiguous arrays (photometric_host_array) of one shape and dtype with the height and width of the flow, at most max_c
    channels (None: any count) and -- one_item -- a single item.  `prefix` starts the messages."""
    near, far = photometric_host_array(near, layout, "near", prefix), photometric_host_array(far, layout, "far", prefix)
    if near.shape != far.shape:
        raise ValueError("{}the arrays need the same shape, got {} and {}".format(prefix, near.shape, far.shape))
    if near.dtype != far.dtype:
        raise TypeError("{}the arrays need the same dtype, got {} and {}".format(prefix, near.dtype, far.dtype))
    n, c, h, w, batched = tensor_args(tensor_logical_shape(near.shape, layout), layout, near.dtype.name)
    if max_c is not None:
        pair_channels(c, max_c, prefix)
    if one_item and n != 1:
        raise ValueError("{}one flow takes one item, got {}".format(prefix, n))
    if (h, w) != tuple(field_shape):
        raise ValueError("{}arrays and flow need the same height and width, got {} and {}".format(prefix, (h, w), tuple(field_shape)))
    return near, far, n, c, batched


# -- photometric error of a warp (K21)
PHOTO_METRICS = {'l1': nat.PHOTO_L1, 'l2': nat.PHOTO_L2, 'charbonnier': nat.PHOTO_CHARBONNIER}
PHOTO_EPS = 1e-3                  # the Charbonnier constant when none is given


def photometric_args(metric='l1', eps=None, threshold=None):
    """Validation of the settings of a photometric error (K21) on the host before any device work -> (metric code, eps,
    threshold): eps as float32, threshold as float32 or None.  metric: 'l1' (mean absolute difference over the channels),
    'l2' (root mean square) or 'charbonnier' (mean of sqrt(d^2 + eps^2)); eps: None for 1e-3, used by 'charbonnier' only;
    threshold: None for no `within` output, else the bound err <= threshold.  A bool or a value of the wrong type is a
    TypeError, an unknown metric or a negative or non-finite value (as given, or once rounded to float32) a ValueError."""
    prefix = "Error computing photometric error: "
    if not isinstance(metric, str):
        raise TypeError("{}metric must be a string, got {}".format(prefix, type(metric).__name__))
    if metric not in PHOTO_METRICS:
        raise ValueError("{}metric must be 'l1', 'l2' or 'charbonnier', got {!r}".format(prefix, metric))
    eps = _float32_setting(PHOTO_EPS if eps is None else eps, "eps", prefix)
    threshold = None if threshold is None else _float32_setting(threshold, "threshold", prefix)
    return PHOTO_METRICS[metric], eps, threshold


def photometric_host_array(a, layout, name, prefix="Error computing photometric error: "):
    """A tensor given to Flow.photometric / photometric_error -> (contiguous array in memory order, layout): a NumPy array
    of float32 or float16, or of uint8 (an image: converted to float32, which is exact), of shape (H, W) -- one channel --,
    (H, W, C) with layout 'hwc' or (C, H, W) with layout 'chw'; a leading item axis makes (N, H, W, C) / (N, C, H, W).
    TypeError for another type or dtype, ValueError for another rank or layout; `prefix` starts the messages (K22 passes its own)."""
    if not isinstance(a, np.ndarray):
        raise TypeError("{}{} needs to be a numpy array, got {}".format(prefix, name, type(a).__name__))
    if layout not in _TENSOR_LAYOUT:
        raise ValueError("{}layout must be 'chw' or 'hwc', got {!r}".format(prefix, layout))
    if a.dtype == np.uint8:
        a = a.astype(np.float32)
    if a.dtype != np.float32 and a.dtype != np.float16:
        raise TypeError("{}{} needs to have dtype float32, float16 or uint8, got {}".format(prefix, name, a.dtype))
    if a.ndim == 2:
        a = a[None] if layout == 'chw' else a[..., None]
    if a.ndim not in (3, 4):
        raise ValueError("{}{} needs to have shape (H, W), {}, got {}".format(
            prefix, name, "(C, H, W) or (N, C, H, W)" if layout == 'chw' else "(H, W, C) or (N, H, W, C)", a.shape))
    return np.ascontiguousarray(a)


# -- census distance of a warp over a window (K22)
CENSUS_MODES = {'hard': nat.CENSUS_HARD, 'soft': nat.CENSUS_SOFT}
CENSUS_WINDOWS = (3, 5, 7)
CENSUS_DELTA, CENSUS_NOISE, CENSUS_KNEE = 0.0, 0.81, 0.1     # the dead zone; the ternary census' constants, for 0 ... 255


def census_args(window=7, mode='soft', delta=None, noise=None, knee=None, min_count=None, threshold=None):
    """Validation of the settings of a census distance (K22) on the host before any device work -> (window, mode code, p0,
    p1, min_count, threshold): p0, p1 as float32 -- (delta, 0) for 'hard', (noise, knee) for 'soft' --, threshold as float32
    or None.  window: 3, 5 or 7; mode: 'hard' (sign census with the dead zone `delta` >= 0, None: 0) or 'soft' (the ternary
    census with `noise` > 0, None: 0.81, and `knee` > 0, None: 0.1); a parameter of the other mode must stay None;
    min_count: the valid neighbours a window needs, 1 ... window^2 - 1, None: all of them; threshold: None for no `within`
    output, else the bound err <= threshold.  A bool or a value of the wrong type is a TypeError, a value out of range or
    not finite (as given, or once rounded to float32) a ValueError."""
    prefix = "Error computing census distance: "
    _integer_setting(window, "window", prefix)
    if window not in CENSUS_WINDOWS:
        raise ValueError("{}window must be 3, 5 or 7, got {}".format(prefix, window))
    if not isinstance(mode, str):
        raise TypeError("{}mode must be a string, got {}".format(prefix, type(mode).__name__))
    if mode not in CENSUS_MODES:
        raise ValueError("{}mode must be 'hard' or 'soft', got {!r}".format(prefix, mode))
    for name, value, wanted in (("delta", delta, 'hard'), ("noise", noise, 'soft'), ("knee", knee, 'soft')):
        if value is not None and mode != wanted:
            raise ValueError("{}{} belongs to mode '{}' and must be None with mode '{}'".format(prefix, name, wanted, mode))
    if mode == 'hard':
        values = (("delta", CENSUS_DELTA if delta is None else delta, False), ("threshold", threshold, False))
    else:
        values = (("noise", CENSUS_NOISE if noise is None else noise, True), ("knee", CENSUS_KNEE if knee is None else knee, True),
                  ("threshold", threshold, False))
    out = {name: None if value is None else _float32_setting(value, name, prefix, positive) for name, value, positive in values}
    full = int(window) * int(window) - 1
    if min_count is None:
        min_count = full
    _integer_setting(min_count, "min_count", prefix, none_ok=True)
    if not 1 <= min_count <= full:
        raise ValueError("{}min_count must be in [1, {}] for window {}, got {}".format(prefix, full, window, min_count))
    p0, p1 = (out["delta"], np.float32(0)) if mode == 'hard' else (out["noise"], out["knee"])
    return int(window), CENSUS_MODES[mode], p0, p1, int(min_count), out["threshold"]


def census_channels(c):
    """The channel count of a census distance (K22): 1 ... 4, else a ValueError that names the limit."""
    return pair_channels(c, nat.CENSUS_MAX_C, "Error computing census distance: ")


# -- structural similarity of a warp over a window (K26)
SSIM_WINDOWS = (3, 5, 7, 11)
SSIM_WEIGHTS = ('gaussian', 'uniform')
SSIM_SIGMA = 1.5                  # Wang et al.'s Gaussian window


def ssim_args(window=11, weights='gaussian', sigma=None, data_range=255.0, k1=0.01, k2=0.03, min_count=None, threshold=None):
    """Validation of the settings of a structural similarity (K26) on the host before any device work -> (window, taps, c1,
    c2, min_count, threshold): taps the float32 array of the 1-D window, c1 = (k1 data_range)^2 and c2 = (k2 data_range)^2
    computed in float64 and rounded to float32, threshold as float32 or None.  window: 3, 5, 7 or 11; weights: 'uniform'
    (every tap 1.0; `sigma` must stay None) or 'gaussian' (exp(-x^2 / (2 sigma^2)) in float64, divided by its sum, rounded
    to float32; `sigma` > 0, None: 1.5); data_range, k1, k2 > 0; min_count: the valid pixels a window needs, the centre
    among them, 1 ... window^2, None: all of them; threshold: None for no `within` output, else the bound err <= threshold.
    A bool or a value of the wrong type is a TypeError, a value out of range or not finite (as given, or once rounded to
    float32) a ValueError."""
    prefix = "Error computing structural similarity: "
    _integer_setting(window, "window", prefix)
    if window not in SSIM_WINDOWS:
        raise ValueError("{}window must be 3, 5, 7 or 11, got {}".format(prefix, window))
    if not isinstance(weights, str):
        raise TypeError("{}weights must be a string, got {}".format(prefix, type(weights).__name__))
    if weights not in SSIM_WEIGHTS:
        raise ValueError("{}weights must be 'gaussian' or 'uniform', got {!r}".format(prefix, weights))
    if sigma is not None and weights != 'gaussian':
        raise ValueError("{}sigma belongs to weights 'gaussian' and must be None with weights '{}'".format(prefix, weights))
    window = int(window)
    if weights == 'uniform':
        taps = np.ones(window, np.float32)
    else:
        _float32_setting(SSIM_SIGMA if sigma is None else sigma, "sigma", prefix, positive=True)
        x = np.arange(window, dtype=np.float64) - window // 2
        g = np.exp(-(x * x) / (2.0 * float(SSIM_SIGMA if sigma is None else sigma) ** 2))
        taps = (g / g.sum()).astype(np.float32)
        if not (np.isfinite(taps).all() and (taps > 0).all()):
            raise ValueError("{}sigma must leave every tap of window {} positive in float32, got {}".format(prefix, window, sigma))
    for name, value in (("data_range", data_range), ("k1", k1), ("k2", k2)):
        _float32_setting(value, name, prefix, positive=True, none_ok=False)
    with np.errstate(over='ignore', under='ignore'):
        c1, c2 = np.float32((float(k1) * float(data_range)) ** 2), np.float32((float(k2) * float(data_range)) ** 2)
    for name, value in (("k1 * data_range", c1), ("k2 * data_range", c2)):
        if not (np.isfinite(value) and value > 0):
            raise ValueError("{}({})^2 must be finite and positive in float32, got {}".format(prefix, name, value))
    threshold = None if threshold is None else _float32_setting(threshold, "threshold", prefix)
    full = window * window
    if min_count is None:
        min_count = full
    _integer_setting(min_count, "min_count", prefix, none_ok=True)
    if not 1 <= min_count <= full:
        raise ValueError("{}min_count must be in [1, {}] for window {}, got {}".format(prefix, full, window, min_count))
    return window, taps, c1, c2, int(min_count), threshold


# -- variational refinement of a field on two images (K23)
REFINE_DEFAULTS = dict(alpha=20.0, delta=5.0, zeta=0.1, eps=0.1, fixed_point=5, sor=5, omega=1.6)


def refine_args(alpha=None, delta=None, zeta=None, eps=None, fixed_point=None, sor=None, omega=None):
    """Validation of the settings of a variational refinement (K23) on the host before any device work -> (alpha, delta,
    zeta, eps as float32, fixed_point, sor as int, omega as float32); None takes the default: 20, 5, 0.1, 0.1, 5, 5, 1.6.
    alpha (smoothness weight), delta (data weight): finite and not negative; zeta (the normalisation of the data term), eps
    (the Charbonnier constant): finite and positive, their float32 squares too; fixed_point, sor: integers 1 ... 32; omega
    (the relaxation factor): in (0, 2).  A bool or a value of the wrong type is a TypeError, a value out of range or not
    finite (as given, or once rounded to float32) a ValueError."""
    prefix = "Error refining flow: "
    given = dict(alpha=alpha, delta=delta, zeta=zeta, eps=eps, fixed_point=fixed_point, sor=sor, omega=omega)
    given = {name: REFINE_DEFAULTS[name] if value is None else value for name, value in given.items()}
    out = {name: _float32_setting(given[name], name, prefix) for name in ("alpha", "delta")}
    square_too = " (its float32 square too)"
    for name in ("zeta", "eps"):
        out[name] = _float32_setting(given[name], name, prefix, positive=True, note=square_too)
        with np.errstate(over='ignore', under='ignore'):
            square = out[name] * out[name]
        if not 0 < square < np.inf:
            raise ValueError("{}{} must be finite and positive{}, got {}".format(prefix, name, square_too, given[name]))
    omega = _float32_rounded(given["omega"], "omega", prefix)
    if not 0 < omega < 2:
        raise ValueError("{}omega must lie in (0, 2), got {}".format(prefix, given["omega"]))
    for name in ("fixed_point", "sor"):
        out[name] = _integer_setting(given[name], name, prefix, 1, nat.REFINE_MAX_ITER, none_ok=True)
    return out["alpha"], out["delta"], out["zeta"], out["eps"], out["fixed_point"], out["sor"], omega


def refine_channels(c):
    """The channel count of a variational refinement (K23): 1 ... 4, else a ValueError that names the limit."""
    return pair_channels(c, nat.REFINE_MAX_C, "Error refining flow: ")


# -- dense inverse search of a field on two images (K24) and the coarse-to-fine estimator on top of it
ISEARCH_PATCHES = (4, 8)
ESTIMATE_MAX_LEVELS = 6


def inverse_search_args(patch=8, stride=4, iterations=12, normalise=True, floor=1.0):
    """Validation of the settings of a dense inverse search (K24) on the host before any device work -> (patch, stride,
    iterations as int, normalise as bool, floor as float32).  patch: 4 or 8; stride: an integer 1 ... patch; iterations: an
    integer 1 ... 32; normalise: a bool (subtract the patch means); floor: the smallest intensity difference a weight of the
    densification divides by, finite and positive (1.0 is meant for intensities 0 ... 255).  A value of the wrong type is a
    TypeError, a value out of range or not finite (as given, or once rounded to float32) a ValueError."""
    prefix = "Error searching flow: "
    for name, value in (("patch", patch), ("stride", stride), ("iterations", iterations)):
        _integer_setting(value, name, prefix)
    if patch not in ISEARCH_PATCHES:
        raise ValueError("{}patch must be 4 or 8, got {}".format(prefix, patch))
    if not 1 <= stride <= patch:
        raise ValueError("{}stride must be in [1, patch = {}], got {}".format(prefix, patch, stride))
    iterations = _integer_setting(iterations, "iterations", prefix, 1, nat.ISEARCH_MAX_ITER)
    if not isinstance(normalise, (bool, np.bool_)):
        raise TypeError("{}normalise must be a bool, got {}".format(prefix, type(normalise).__name__))
    floor = _float32_setting(floor, "floor", prefix, positive=True, none_ok=False, note=" (as float32 too)")
    return int(patch), int(stride), iterations, bool(normalise), floor


def inverse_search_channels(c):
    """The channel count of a dense inverse search (K24): 1 ... 4, else a ValueError that names the limit."""
    return pair_channels(c, nat.ISEARCH_MAX_C, "Error searching flow: ")


def patch_origins(n, patch, stride):
    """The origins of K24's patch grid along an axis of length n >= patch: 0, stride, 2 stride, ... <= n - patch, and n - patch
    itself where the last of them is not, so every pixel lies in a patch."""
    if n < patch:
        raise ValueError("Error searching flow: an axis of {} pixels holds no patch of {}".format(n, patch))
    origins = list(range(0, n - patch + 1, stride))
    if origins[-1] != n - patch:
        origins.append(n - patch)
    return origins


def estimate_levels(shape, levels=None, patch=8):
    """The number of pyramid levels of estimate_flow for images of `shape` (H, W): with `levels` given, an integer 1 ... 6,
    H and W must be divisible by 2^(levels - 1) and the coarsest level must measure at least 2 patch in both axes, else a
    ValueError that names `pad`; None is the largest count <= 6 that meets both conditions (at least one level must)."""
    prefix = "Error estimating flow: "
    h, w = int(shape[0]), int(shape[1])

    def fits(k):
        f = 1 << (k - 1)
        return h % f == 0 and w % f == 0 and h // f >= 2 * patch and w // f >= 2 * patch

    if levels is None:
        good = [k for k in range(1, ESTIMATE_MAX_LEVELS + 1) if fits(k)]
        if not good:
            raise ValueError("{}images of {} x {} are smaller than two patches of {}; pad them first (Flow.pad / np.pad)"
                             .format(prefix, h, w, patch))
        return good[-1]
    if isinstance(levels, (bool, np.bool_)) or not isinstance(levels, (int, np.integer)):
        raise TypeError("{}levels must be an integer or None, got {}".format(prefix, type(levels).__name__))
    if not 1 <= levels <= ESTIMATE_MAX_LEVELS:
        raise ValueError("{}levels must be in [1, {}], got {}".format(prefix, ESTIMATE_MAX_LEVELS, levels))
    if not fits(int(levels)):
        raise ValueError("{}{} levels need a height and width divisible by {} and a coarsest level of at least {} x {} pixels, "
                         "got {} x {}; pad the images first (Flow.pad / np.pad) or take fewer levels"
                         .format(prefix, levels, 1 << (levels - 1), 2 * patch, 2 * patch, h, w))
    return int(levels)


# -- an estimate against a ground truth (K14)
ERROR_THRESHOLDS, ERROR_OUTLIER, ERROR_SPEED_EDGES = (1, 3, 5), (3, 0.05), (10, 40)     # px; KITTI's Fl rule; Sintel's speed bins


def _error_value(name, value):
    """one threshold, bound or edge -> float32; a bool or a non-number is a TypeError, NaN or a negative value a ValueError"""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise TypeError("Error evaluating flow error: {} must be numbers, got {}".format(name, type(value).__name__))
    if value != value or value < 0:
        raise ValueError("Error evaluating flow error: {} must not be NaN or negative, got {}".format(name, value))
    with np.errstate(over='ignore'):
        return np.float32(float(value)) if value < 1e300 else np.float32(np.inf)


def _error_list(name, values, default, most):
    values = default if values is None else values
    if isinstance(values, (int, float, np.integer, np.floating)) and not isinstance(values, (bool, np.bool_)):
        values = (values,)
    if isinstance(values, (str, bytes)) or not isinstance(values, (tuple, list, np.ndarray)):
        raise TypeError("Error evaluating flow error: {} must be a number or a tuple or list of numbers, got {}"
                        .format(name, type(values).__name__))
    if isinstance(values, np.ndarray) and values.ndim != 1:
        raise ValueError("Error evaluating flow error: {} must be one-dimensional".format(name))
    values = [_error_value(name, v.item() if isinstance(v, np.generic) and not isinstance(v, np.bool_) else v) for v in values]
    if len(values) > most:
        raise ValueError("Error evaluating flow error: at most {} {}, got {}".format(most, name, len(values)))
    return values


def error_args(thresholds=None, outlier=None, speed_edges=None):
    """Validation of the settings of the flow-error evaluation (K14) on the host before any device work ->
    (thr float32[4], (out_abs, out_rel) as float32, edges float32[3], n_thresholds, n_edges).  thresholds: up to 4 EPE
    thresholds in px (default 1, 3, 5); outlier: (absolute px, relative share of the ground truth's magnitude), both of
    which an outlier exceeds (default KITTI's 3 px and 5 %); speed_edges: up to 3 ascending magnitudes of the ground truth
    that separate the speed bins (default Sintel's 10, 40).  Unused slots are +inf.  A bool, a string or another non-number
    is a TypeError; NaN, a negative value, too many entries and descending edges are a ValueError."""
    thr = _error_list("thresholds", thresholds, ERROR_THRESHOLDS, 4)
    edges = _error_list("speed_edges", speed_edges, ERROR_SPEED_EDGES, 3)
    out = ERROR_OUTLIER if outlier is None else outlier
    if isinstance(out, (str, bytes)) or not isinstance(out, (tuple, list, np.ndarray)):
        raise TypeError("Error evaluating flow error: outlier must be a pair (absolute, relative), got {}".format(type(out).__name__))
    if len(out) != 2:
        raise ValueError("Error evaluating flow error: outlier must be a pair (absolute, relative), got {} values".format(len(out)))
    out = _error_list("outlier", out, None, 2)
    if any(b < a for a, b in zip(edges, edges[1:])):
        raise ValueError("Error evaluating flow error: speed_edges must be ascending, got {}".format([float(e) for e in edges]))
    pad = lambda v, n: np.array(v + [np.inf] * (n - len(v)), np.float32)
    return pad(thr, 4), (out[0], out[1]), pad(edges, 3), len(thr), len(edges)


# -- masked-out vectors from the nearest valid pixel (K15)
FILL_MAX_D2 = 2 ** 31 - 1


def fill_args(max_dist=None):
    """Validation of the reach of a fill (K15) on the host before any device work -> max_d2, the largest squared distance in
    px^2 a vector may be copied over, as a Python int: None -> -1 (no limit), otherwise min(floor(max_dist^2), 2^31 - 1)
    computed in float64.  A bool or a non-number is a TypeError, a negative or non-finite value a ValueError."""
    if max_dist is None:
        return -1
    if isinstance(max_dist, (bool, np.bool_)) or not isinstance(max_dist, (int, float, np.integer, np.floating)):
        raise TypeError("Error filling flow: max_dist must be a number or None, got {}".format(type(max_dist).__name__))
    try:
        d = np.float64(float(max_dist))
    except OverflowError:                                   # a Python int beyond the float64 range
        d = np.float64(1e300 if max_dist > 0 else -1e300)
    if not np.isfinite(d) or d < 0:
        raise ValueError("Error filling flow: max_dist must be finite and not negative, got {}".format(max_dist))
    with np.errstate(over='ignore'):
        return int(min(np.floor(d * d), np.float64(FILL_MAX_D2)))


# -- mask-aware median filter (K16)
MEDIAN_KSIZES = (3, 5, 7)


def median_args(ksize=5, min_count=None):
    """Validation of the window and the member threshold of a median filter (K16) on the host before any device work
    -> (ksize, min_count) as Python ints: ksize an int in {3, 5, 7}; min_count None -> 1, otherwise an int in
    1 ... ksize^2.  A bool or a non-integer is a TypeError, a value outside its set a ValueError."""
    if not _is_integer(ksize):
        raise TypeError("Error filtering flow: ksize must be an integer, got {}".format(type(ksize).__name__))
    if ksize not in MEDIAN_KSIZES:
        raise ValueError("Error filtering flow: ksize must be 3, 5 or 7, got {}".format(ksize))
    if min_count is None:
        return int(ksize), 1
    if not _is_integer(min_count):
        raise TypeError("Error filtering flow: min_count must be an integer or None, got {}".format(type(min_count).__name__))
    if not 1 <= min_count <= ksize * ksize:
        raise ValueError("Error filtering flow: min_count must be in 1 ... {} for ksize {}, got {}"
                         .format(ksize * ksize, ksize, min_count))
    return int(ksize), int(min_count)


# -- convex upsampling (K17)
UPSAMPLE_FACTORS = (2, 4, 8)


def upsample_args(factor, weights_shape, coarse_shape):
    """Validation of a convex upsampling (K17) on the host before any device work -> factor as a Python int.  `factor`: an
    int in {2, 4, 8} (a bool or a non-integer is a TypeError, another value a ValueError); `weights_shape`: the LOGICAL
    shape of the logits, (C, h, w) or (N, C, h, w), whose channel count must be 9 * factor^2 and whose height and width
    must be those of `coarse_shape`, the (h, w) of the coarse field (ValueError otherwise)."""
    if not _is_integer(factor):
        raise TypeError("Error upsampling flow: factor must be an integer, got {}".format(type(factor).__name__))
    if factor not in UPSAMPLE_FACTORS:
        raise ValueError("Error upsampling flow: factor must be 2, 4 or 8, got {}".format(factor))
    weights_shape = tuple(int(v) for v in weights_shape)
    if len(weights_shape) not in (3, 4):
        raise ValueError("Error upsampling flow: weights of shape {} are not (C, h, w) or (N, C, h, w)".format(weights_shape))
    c, h, w = weights_shape[-3:]
    if c != 9 * factor * factor:
        raise ValueError("Error upsampling flow: factor {} needs {} weight channels, got {}".format(factor, 9 * factor * factor, c))
    if (h, w) != (int(coarse_shape[0]), int(coarse_shape[1])):
        raise ValueError("Error upsampling flow: weights and flow need the same height and width, got {} and {}"
                         .format((h, w), (int(coarse_shape[0]), int(coarse_shape[1]))))
    if h * factor > 32766 or w * factor > 32766:
        raise ValueError("Error upsampling flow: {} x {} times {} is beyond the 32766 x 32766 a flow may have".format(h, w, factor))
    return int(factor)


def upsample_weights_array(weights, factor, coarse_shape):
    """The `weights` of Flow.upsample_convex / upsample_flow_convex -> (contiguous array, factor): a NumPy array (9 f^2, h, w)
    of float32 or float16 (TypeError for another type or dtype; the ValueErrors of upsample_args)."""
    if not isinstance(weights, np.ndarray):
        raise TypeError("Error upsampling flow: weights need to be a numpy array, got {}".format(type(weights).__name__))
    if weights.dtype != np.float32 and weights.dtype != np.float16:
        raise TypeError("Error upsampling flow: weights need to have dtype float32 or float16, got {}".format(weights.dtype))
    factor = upsample_args(factor, weights.shape, coarse_shape)
    if weights.ndim != 3:
        raise ValueError("Error upsampling flow: one field takes weights of shape (C, h, w), got {}".format(weights.shape))
    return np.ascontiguousarray(weights), factor


# -- on-demand correlation lookup (K18)
CORR_ORDERS = {'xy': 0, 'yx': 1}        # OFL_CORR_XY (RAFT's CorrBlock), OFL_CORR_YX (row-major cost volumes)


def corr_args(radius, levels, scale, order, quant, channels, shape):
    """Validation of a correlation lookup (K18) on the host before any device work -> (radius, levels, scale as float32,
    order code, quant).  radius: an int in 1 ... 4; levels: an int in 1 ... 8 whose last pyramid level of `shape` (H, W),
    (H >> levels - 1, W >> levels - 1), must not be empty; scale: None for float32(1 / sqrt(float64(channels))), or a finite
    number; order: 'xy' or 'yx'; quant: 0 (the 1/32-px snap) or 1 (exact).  A bool or a non-number is a TypeError, a value
    outside its set a ValueError."""
    for name, value in (("radius", radius), ("levels", levels), ("quant", quant)):
        if not _is_integer(value):
            raise TypeError("Error looking up correlation: {} must be an integer, got {}".format(name, type(value).__name__))
    if not 1 <= radius <= 4:
        raise ValueError("Error looking up correlation: radius must be in 1 ... 4, got {}".format(radius))
    if not 1 <= levels <= 8:
        raise ValueError("Error looking up correlation: levels must be in 1 ... 8, got {}".format(levels))
    h, w = int(shape[0]), int(shape[1])
    if h >> (levels - 1) < 1 or w >> (levels - 1) < 1:
        raise ValueError("Error looking up correlation: level {} of a {} x {} grid is empty".format(levels - 1, h, w))
    if quant not in (0, 1):
        raise ValueError("Error looking up correlation: quant must be 0 (QUANT_OPENCV) or 1 (QUANT_EXACT), got {}".format(quant))
    if not isinstance(order, str):
        raise TypeError("Error looking up correlation: order must be a string, got {}".format(type(order).__name__))
    if order not in CORR_ORDERS:
        raise ValueError("Error looking up correlation: order must be 'xy' or 'yx', got {!r}".format(order))
    if scale is None:
        scale = np.float32(1.0 / np.sqrt(np.float64(channels)))
    else:
        if isinstance(scale, (bool, np.bool_)) or not isinstance(scale, (int, float, np.integer, np.floating)):
            raise TypeError("Error looking up correlation: scale must be a number or None, got {}".format(type(scale).__name__))
        with np.errstate(over='ignore'):
            scale = np.float32(float(scale)) if abs(scale) < 1e300 else np.float32(np.inf)
        if not np.isfinite(scale):
            raise ValueError("Error looking up correlation: scale must be finite as float32")
    return int(radius), int(levels), scale, CORR_ORDERS[order], int(quant)


def corr_host_array(a, name):
    """A feature map given to correlation_lookup -> (contiguous channels-last array (1, H, W, C), logical shape): a NumPy
    array (C, H, W) of float32 or float16 (TypeError for another type or dtype, ValueError for another rank)."""
    if not isinstance(a, np.ndarray):
        raise TypeError("Error looking up correlation: {} needs to be a numpy array, got {}".format(name, type(a).__name__))
    if a.dtype != np.float32 and a.dtype != np.float16:
        raise TypeError("Error looking up correlation: {} needs to have dtype float32 or float16, got {}".format(name, a.dtype))
    if a.ndim != 3:
        raise ValueError("Error looking up correlation: {} needs to have shape (C, H, W), got {}".format(name, a.shape))
    tensor_args(a.shape, 'chw', a.dtype.name)
    return np.ascontiguousarray(np.moveaxis(a, 0, -1))[None], tuple(a.shape)


# -- global matching (K19)
MATCH_MAX_CHANNELS = 512


def _float32_arg(value, name, prefix):
    """a finite number -> float32 (TypeError for a bool or a non-number, ValueError where float32 cannot hold it)"""
    value = _float32_rounded(value, name, prefix)
    if not np.isfinite(value):
        raise ValueError("{}{} must be finite as float32".format(prefix, name))
    return value


def match_args(scale, min_confidence, channels, dtype1, dtype2):
    """Validation of a global matching (K19) on the host before any device work -> (scale, min_confidence) as float32.
    scale: None for float32(1 / sqrt(float64(channels))), or a finite number; min_confidence: None for 0 (every pixel of the
    mask is set), or a number in [0, 1]; channels: at most 512; dtype1, dtype2: the element types of the two feature maps,
    which must be the same.  A bool or a non-number is a TypeError, a value outside its set a ValueError."""
    prefix = "Error matching features: "
    if dtype1 != dtype2:
        raise ValueError("{}the feature maps need the same dtype, got {} and {}".format(prefix, dtype1, dtype2))
    if not 1 <= channels <= MATCH_MAX_CHANNELS:
        raise ValueError("{}the feature maps must have 1 ... {} channels, got {}".format(prefix, MATCH_MAX_CHANNELS, channels))
    scale = np.float32(1.0 / np.sqrt(np.float64(channels))) if scale is None else _float32_arg(scale, "scale", prefix)
    min_confidence = np.float32(0.0) if min_confidence is None else _float32_arg(min_confidence, "min_confidence", prefix)
    if not 0.0 <= min_confidence <= 1.0:
        raise ValueError("{}min_confidence must be in [0, 1], got {}".format(prefix, min_confidence))
    return scale, min_confidence


def match_host_array(a, name):
    """A feature map given to global_match -> (contiguous channels-last array (1, H, W, C), logical shape): a NumPy array
    (C, H, W) of float32 or float16 (TypeError for another type or dtype, ValueError for another rank)."""
    if not isinstance(a, np.ndarray):
        raise TypeError("Error matching features: {} needs to be a numpy array, got {}".format(name, type(a).__name__))
    if a.dtype != np.float32 and a.dtype != np.float16:
        raise TypeError("Error matching features: {} needs to have dtype float32 or float16, got {}".format(name, a.dtype))
    if a.ndim != 3:
        raise ValueError("Error matching features: {} needs to have shape (C, H, W), got {}".format(name, a.shape))
    tensor_args(a.shape, 'chw', a.dtype.name)
    return np.ascontiguousarray(np.moveaxis(a, 0, -1))[None], tuple(a.shape)


# -- forward warp by splatting (K20)
SPLAT_MODES = {'sum': nat.SPLAT_SUM, 'average': nat.SPLAT_AVERAGE, 'softmax': nat.SPLAT_SOFTMAX}
SPLAT_MIN_WEIGHT = 2.0 ** -10
SPLAT_FRAC_BITS = 24


def splat_args(mode='average', has_importance=False, alpha=1.0, min_weight=None, frac_bits=None):
    """Validation of the settings of a splat (K20) on the host before any device work -> (mode code, alpha, min_weight,
    frac_bits): alpha and min_weight as float32, frac_bits a Python int.  mode: 'sum', 'average' or 'softmax'; softmax needs
    an importance and the two others take none (`has_importance`); alpha: a finite number; min_weight: None for 2^-10, or a
    number in [2^-20, 1]; frac_bits: None for 24, or an int in [0, 40].  A bool or a value of the wrong type is a TypeError,
    a value outside its set a ValueError."""
    prefix = "Error splatting: "
    if not isinstance(mode, str):
        raise TypeError("{}mode must be a string, got {}".format(prefix, type(mode).__name__))
    if mode not in SPLAT_MODES:
        raise ValueError("{}mode must be 'sum', 'average' or 'softmax', got {!r}".format(prefix, mode))
    if mode == 'softmax' and not has_importance:
        raise ValueError("{}mode 'softmax' needs an importance".format(prefix))
    if mode != 'softmax' and has_importance:
        raise ValueError("{}an importance is used by mode 'softmax' only, got mode {!r}".format(prefix, mode))
    alpha = _float32_arg(alpha, "alpha", prefix)
    min_weight = np.float32(SPLAT_MIN_WEIGHT) if min_weight is None else _float32_arg(min_weight, "min_weight", prefix)
    if not 2.0 ** -20 <= min_weight <= 1.0:
        raise ValueError("{}min_weight must be in [2^-20, 1], got {}".format(prefix, min_weight))
    frac_bits = SPLAT_FRAC_BITS if frac_bits is None else frac_bits
    if not _is_integer(frac_bits):
        raise TypeError("{}frac_bits must be an integer or None, got {}".format(prefix, type(frac_bits).__name__))
    if not 0 <= frac_bits <= 40:
        raise ValueError("{}frac_bits must be in [0, 40], got {}".format(prefix, frac_bits))
    return SPLAT_MODES[mode], alpha, min_weight, int(frac_bits)


def splat_host_array(a, layout, field_shape):
    """A tensor given to Flow.splat / splat_flow -> (contiguous array, n, c, batched): a NumPy array of float32 or float16 in
    the memory order of `layout` -- (C, H, W) / (N, C, H, W) for 'chw', (H, W, C) / (N, H, W, C) for 'hwc' -- with the height
    and width of the flow (TypeError for another type or dtype, the ValueErrors of tensor_args)."""
    if not isinstance(a, np.ndarray):
        raise TypeError("Error splatting: the tensor needs to be a numpy array, got {}".format(type(a).__name__))
    if a.dtype != np.float32 and a.dtype != np.float16:
        raise TypeError("Error splatting: the tensor needs to have dtype float32 or float16, got {}".format(a.dtype))
    n, c, _, _, batched = tensor_args(tensor_logical_shape(a.shape, layout), layout, a.dtype.name, field_shape)
    return np.ascontiguousarray(a), n, c, batched


def splat_importance_array(z, shape):
    """The importance given to a host splat -> None, or a contiguous float32 (H, W) array (TypeError for another type,
    ValueError for another shape)."""
    if z is None:
        return None
    if not isinstance(z, np.ndarray):
        raise TypeError("Error splatting: importance needs to be a numpy array or None, got {}".format(type(z).__name__))
    if z.shape != (shape[0], shape[1]):
        raise ValueError("Error splatting: importance needs the shape of the flow {}, got {}".format(tuple(shape), z.shape))
    return np.ascontiguousarray(z, np.float32)


# -- many-channel float tensors (K12)
def tensor_dtype(array_dtype, dtype=None):
    """The element type of a tensor -> 'float32', 'float16' or 'bfloat16'.  `array_dtype`: the dtype of the array that holds
    it (a NumPy dtype, or the string 'bfloat16'); `dtype`: what the caller says it is, or None.  bfloat16, which NumPy does
    not have, is a 2-byte integer array with dtype='bfloat16' (as in interop.external_args); anything but the three is a
    TypeError."""
    if str(array_dtype) == 'bfloat16':
        return 'bfloat16'
    array_dtype = np.dtype(array_dtype)
    if dtype is not None and str(dtype) == 'bfloat16':
        if array_dtype not in (np.int16, np.uint16):
            raise TypeError("Error taking a tensor: dtype='bfloat16' reinterprets a 2-byte integer array, got {}".format(array_dtype))
        return 'bfloat16'
    if dtype is not None and np.dtype(dtype) != array_dtype:
        raise TypeError("Error taking a tensor: the array is {}, not {}".format(array_dtype, np.dtype(dtype)))
    if array_dtype.name not in ('float32', 'float16'):
        raise TypeError("Error taking a tensor: tensors are float32, float16 or (a 2-byte integer array with dtype='bfloat16') "
                        "bfloat16, got {}".format(array_dtype))
    return array_dtype.name


def tensor_args(shape, layout, dtype, field_shape=None):
    """Checks of a tensor's description, on the host -> (n, c, h, w, batched).  `shape`: the LOGICAL shape (C, H, W) or
    (N, C, H, W), whatever the memory order; `layout`: 'chw' or 'hwc', the memory order; `dtype`: one of the three names
    (tensor_dtype); `field_shape`: the (H, W) of the field that is to warp it, or None."""
    if layout not in _TENSOR_LAYOUT:
        raise ValueError("Error taking a tensor: layout must be 'chw' or 'hwc', got {!r}".format(layout))
    if dtype not in _TENSOR_EL:
        raise TypeError("Error taking a tensor: dtype must be float32, float16 or bfloat16, got {}".format(dtype))
    shape = tuple(int(v) for v in shape)
    if len(shape) not in (3, 4):
        raise ValueError("Error taking a tensor: shape {} is not (C, H, W) or (N, C, H, W)".format(shape))
    batched = len(shape) == 4
    n = shape[0] if batched else 1
    c, h, w = shape[-3:]
    if not 1 <= n <= 65535 or not 1 <= c <= 65535:
        raise ValueError("Error taking a tensor: items and channels must be in [1, 65535], got {} and {}".format(n, c))
    if not (1 <= h <= 32766 and 1 <= w <= 32766):
        raise ValueError("Error taking a tensor: height and width must be in [1, 32766], got {} x {}".format(h, w))
    if field_shape is not None and (h, w) != tuple(field_shape):
        raise ValueError("tensor and flow need the same height and width, got {} and {}".format((h, w), tuple(field_shape)))
    return n, c, h, w, batched


def tensor_mem_shape(shape, layout):
    """The logical shape (C, H, W) / (N, C, H, W) -> the shape of the array in memory order."""
    shape = tuple(shape)
    return shape if layout == 'chw' else shape[:-3] + (shape[-2], shape[-1], shape[-3])


def tensor_logical_shape(mem_shape, layout):
    """The shape of an array in memory order -- (C, H, W) / (N, C, H, W) for 'chw', (H, W, C) / (N, H, W, C) for 'hwc' -> the
    logical shape.  Checks the layout string and the rank."""
    if layout not in _TENSOR_LAYOUT:
        raise ValueError("Error taking a tensor: layout must be 'chw' or 'hwc', got {!r}".format(layout))
    mem_shape = tuple(int(v) for v in mem_shape)
    if len(mem_shape) not in (3, 4):
        raise ValueError("Error taking a tensor: shape {} is not {}".format(
            mem_shape, "(C, H, W) or (N, C, H, W)" if layout == 'chw' else "(H, W, C) or (N, H, W, C)"))
    return mem_shape if layout == 'chw' else mem_shape[:-3] + (mem_shape[-1], mem_shape[-3], mem_shape[-2])
