"""K15 restated in NumPy by brute force (the definition of include/ofl.h), plus the masks and vectors the tests of the fill
share.  Everything is an exact integer: int64 squared distances from every pixel to every source, the minimum, then the
minimum linear index among the minima.  No sort, no SciPy, no tolerance."""
import functools

import numpy as np

FAR = np.uint32(0xFFFFFFFF)
# 1 x 1 ... 2 x 1: the smallest; 1 x 63 ... 3 x 129: the row pass's 64-pixel words; 67 x 5, 48 x 80, 31 x 97: more rows than
# columns, whole words, odd sizes
SHAPES = [(1, 1), (1, 2), (2, 1), (1, 63), (1, 64), (1, 65), (3, 129), (67, 5), (48, 80), (31, 97)]
MAX_D2 = [0, 1, 2, 24, 25]


def sources(mask, valid=None):
    m = np.asarray(mask).astype(np.uint8)
    if valid is not None:
        m = m & np.asarray(valid).astype(np.uint8)
    return m != 0


def fill(vecs, mask, valid=None, max_d2=-1):
    """-> (out_vecs float32 (H, W, 2) or None, out_mask uint8 (H, W), index int32 (H, W), d2 uint32 (H, W))"""
    src = sources(mask, valid)
    h, w = src.shape
    index, d2 = np.full(h * w, -1, np.int32), np.full(h * w, FAR, np.uint32)
    qy, qx = np.nonzero(src)
    qy, qx = qy.astype(np.int64), qx.astype(np.int64)
    lin = qy * w + qx
    if lin.size:
        big = np.int64(h) * w
        step = max(1, (1 << 22) // lin.size)
        for p0 in range(0, h * w, step):
            p = np.arange(p0, min(p0 + step, h * w), dtype=np.int64)
            d = (p[:, None] % w - qx[None, :]) ** 2 + (p[:, None] // w - qy[None, :]) ** 2
            dmin = d.min(axis=1)
            first = np.where(d == dmin[:, None], lin[None, :], big).min(axis=1)
            ok = np.ones_like(dmin, bool) if max_d2 < 0 else dmin <= max_d2
            index[p[ok]] = first[ok]
            d2[p[ok]] = dmin[ok]
    filled = index >= 0
    out_vecs = None
    if vecs is not None:
        words = np.ascontiguousarray(vecs, np.float32).reshape(-1, 2).view(np.uint64).ravel()       # 8 bytes per pixel, moved as they are
        take = np.where(filled, index, np.arange(h * w)).astype(np.int64)
        out_vecs = words[take].view(np.float32).reshape(h, w, 2)
    return out_vecs, filled.astype(np.uint8).reshape(h, w), index.reshape(h, w), d2.reshape(h, w)


# ---------------------------------------------------------------------------------------------- the shared inputs
def vectors(shape, seed=5):
    """random vectors with NaN (two payloads), +-Inf and -0.0 planted: a fill moves bytes, it does not compute"""
    h, w = shape
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((h, w, 2)) * 20).astype(np.float32)
    flat = v.reshape(-1).view(np.uint32)
    special = np.array([0x7FC00000, 0x7FA00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001], np.uint32)
    at = rng.choice(flat.size, min(flat.size, special.size), replace=False)
    flat[at] = special[:at.size]
    return v


def mask_names():
    return (["all", "none", "corner0", "corner1", "corner2", "corner3", "lattice2", "lattice3", "lattice4", "checker", "pair",
             "column", "row", "ring", "rows"] + ["random50", "random5", "random05"])


def mask(name, shape):
    h, w = shape
    m = np.zeros((h, w), np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    if name == "all":
        m[:] = 1
    elif name.startswith("corner"):
        k = int(name[-1])
        m[(h - 1) * (k >> 1), (w - 1) * (k & 1)] = 1
    elif name.startswith("lattice"):
        p = int(name[-1])
        m[::p, ::p] = 1
    elif name == "checker":
        m[(x + y) % 2 == 0] = 1
    elif name == "pair":                                       # symmetric about the centre: a band of exact ties between them
        m[h // 4, w // 4] = m[h - 1 - h // 4, w - 1 - w // 4] = 1
    elif name == "column":
        m[:, w // 2] = 1
    elif name == "row":
        m[h // 2, :] = 1
    elif name == "ring":
        r = max(1, min(h, w) // 3)
        m[np.rint(np.hypot(y - (h - 1) / 2, x - (w - 1) / 2)) == r] = 1
    elif name == "rows":                                       # rows without any source alternate with rows that have one
        for r in range(1, h, 2):
            m[r, (7 * r) % w] = 1
        if h == 1:
            m[0, w // 3] = 1
    elif name.startswith("random"):
        share = {"random50": 0.5, "random5": 0.05, "random05": 0.005}[name]
        m[np.random.default_rng(17 + h * 131 + w).random((h, w)) < share] = 1
        if not m.any():                                        # too few pixels for the share: one source
            m[h // 2, w // 3] = 1
    elif name != "none":
        raise KeyError(name)
    return m


@functools.lru_cache(maxsize=None)
def _expected(name, shape, max_d2):
    out = fill(vectors(shape), mask(name, shape), None, max_d2)
    for a in out:
        a.setflags(write=False)
    return out


def expected(name, shape, max_d2=-1):
    """fill(vectors(shape), mask(name, shape), None, max_d2), computed once per session and read-only"""
    return _expected(name, tuple(shape), int(max_d2))
