"""NumPy restatement of the reference's Flow.visualise (oflibnumpy flow_class.py:869-951) for the tests, in float32 where
the reference computes in float32 and with its two OpenCV calls restated:

  cv2.cartToPolar(u, v, angleInDegrees=True)  magnitude sqrt(u*u + v*v); angle by OpenCV 4.x fastAtan2 (a degree-7
                                              odd polynomial of min / max over the octant, then folded to [0, 360])
  cv2.findContours + cv2.drawContours(hsv, contours, -1, (0, 0, 0), 1)
                                              H = S = V = 0 on every mask-true pixel that lies on the image frame or
                                              has a mask-false 4-neighbour

Test infrastructure only: the product never imports this module.
"""
import numpy as np

TH = np.float32(1e-3)                       # utils.DEFAULT_THRESHOLD, compared in float32
_DEG = np.float32(180 / np.pi)
P1, P3, P5, P7 = (np.float32(c) * _DEG for c in (0.9997878412794807, -0.3258083974640975,
                                                  0.1555786518463281, -0.04432655554792128))
EPS = np.float32(np.finfo(np.float64).eps)

# HSV -> RGB by sector of the colour wheel: which of the four values (V, P, Q, T) = (1 - s * (0, 1, f, 1 - f)) * v
# goes to red, green and blue
_SECTOR = np.array([[0, 3, 1], [2, 0, 1], [1, 0, 3], [1, 2, 0], [3, 1, 0], [0, 1, 2]])


def thresholded(vecs):
    f = np.array(vecs, dtype=np.float32, copy=True)
    f[(f < TH) & (f > -TH)] = 0
    return f


def magnitude(u, v):
    return np.sqrt(u * u + v * v)


def fast_angle(u, v):
    """degrees in [0, 360], float32 with one rounding per operation"""
    ax, ay = np.abs(u), np.abs(v)
    steep = ~(ax >= ay)
    c = np.where(steep, ax, ay) / (np.where(steep, ay, ax) + EPS)
    c2 = c * c
    a = (((P7 * c2 + P5) * c2 + P3) * c2 + P1) * c
    a = np.where(steep, np.float32(90) - a, a)
    a = np.where(u < 0, np.float32(180) - a, a)
    return np.where(v < 0, np.float32(360) - a, a).astype(np.float32)


def default_range(mag):
    """flow_class.py:910-916: the 99th percentile if > 0, else the maximum if > 0, else 1"""
    p = np.percentile(mag, 99)
    if p > 0:
        return float(p)
    if np.max(mag):
        return float(np.max(mag))
    return 1


def border_pixels(mask):
    m = np.pad(np.asarray(mask, bool), 1, constant_values=False)
    inner = m[:-2, 1:-1] & m[2:, 1:-1] & m[1:-1, :-2] & m[1:-1, 2:]
    return m[1:-1, 1:-1] & ~inner


def hsv_float(vecs, mask=None, show_mask=False, show_mask_borders=False, range_max=None):
    """the float32 (H, W, 3) array the reference builds before its output conversion"""
    f = thresholded(vecs)
    u, v = f[..., 0], f[..., 1]
    mag = magnitude(u, v)
    mask = np.ones(f.shape[:2], bool) if mask is None else np.asarray(mask, bool)
    hsv = np.zeros(f.shape[:2] + (3,), np.float32)
    hsv[..., 0] = np.mod(fast_angle(u, v), 360) / 2
    hsv[..., 2] = 255
    if show_mask:
        hsv[~mask, 2] = 180
    if range_max is None:
        range_max = default_range(mag)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        hsv[..., 1] = np.clip(mag * 255 / range_max, 0, 255)
    if show_mask_borders:
        hsv[border_pixels(mask)] = 0
    return hsv


def hsv_to_rgb_bytes(hsv):
    """the reference's colour-wheel conversion with NumPy's promotions: h * 6 in float32, everything after the int64
    sector index in float64"""
    h, s, v = hsv[..., 0] / 180, hsv[..., 1] / 255, hsv[..., 2] / 255
    h6 = h * 6.
    i = h6.astype(np.int64)
    frac = h6 - i
    s64, v64 = s.astype(np.float64), v.astype(np.float64)
    vals = np.stack([(1 - s64 * x) * v64 for x in (np.zeros_like(frac), np.ones_like(frac), frac, 1. - frac)], axis=-1)
    pick = _SECTOR[i % 6]
    rgb = np.take_along_axis(vals, pick, axis=-1)
    return np.round(rgb * 255).astype(np.uint8)


def visualise(vecs, mode, mask=None, show_mask=False, show_mask_borders=False, range_max=None):
    hsv = hsv_float(vecs, mask, show_mask, show_mask_borders, range_max)
    if mode == 'hsv':
        return np.round(hsv).astype(np.uint8)
    rgb = hsv_to_rgb_bytes(hsv)
    return rgb[..., ::-1] if mode == 'bgr' else rgb
