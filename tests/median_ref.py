"""K16 restated in NumPy by brute force (the definition of include/ofl.h), plus the masks and vectors the tests of the median
filter share.  Floats become their keys (uint32, a total order), the keys of the k^2 shifted copies of the field are widened
to uint64 with non-members as 1 << 32, sorted, and the rank (n - 1) >> 1 is taken: no float operation, no tolerance."""
import functools

import numpy as np

NONE = np.uint64(1) << np.uint64(32)
SHAPES = [(1, 1), (1, 300), (300, 1), (2, 3), (5, 7), (33, 65), (67, 259), (130, 515)]
KSIZES = (3, 5, 7)
SPECIAL = np.array([0x7FC00000, 0x7FA00001, 0xFFC12345, 0xFFFFFFFF, 0x7FFFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000,
                    0x00000001, 0x80000001, 0x007FFFFF], np.uint32)        # NaNs of both signs, +-Inf, +-0.0, denormals


def key(f):
    """float32 array -> uint32 keys: ascending keys are ascending floats, -0.0 < +0.0, NaNs beyond +-Inf by sign and payload"""
    b = np.ascontiguousarray(f, np.float32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkey(k):
    """the inverse of key -> float32"""
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k >> np.uint32(31), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def members(mask, valid=None):
    m = np.asarray(mask).astype(np.uint8)
    if valid is not None:
        m = m & np.asarray(valid).astype(np.uint8)
    return m != 0


def median(vecs, mask, ksize, valid=None, only=None, min_count=1):
    """-> (out_vecs float32 (H, W, 2), out_mask uint8 (H, W), n int32 (H, W))"""
    vecs = np.ascontiguousarray(vecs, np.float32)
    mem = members(mask, valid)
    h, w = mem.shape
    r = ksize // 2
    keys = np.where(mem[..., None], key(vecs).astype(np.uint64), NONE)
    padded = np.full((h + 2 * r, w + 2 * r, 2), NONE, np.uint64)
    padded[r:r + h, r:r + w] = keys
    window = np.stack([padded[dy:dy + h, dx:dx + w] for dy in range(ksize) for dx in range(ksize)], axis=-1)   # (H, W, 2, k^2)
    n = (window[:, :, 0, :] != NONE).sum(axis=-1).astype(np.int32)
    window.sort(axis=-1)
    rank = (np.maximum(n, 1) - 1) >> 1
    med = np.take_along_axis(window, np.broadcast_to(rank[:, :, None, None], (h, w, 2, 1)).astype(np.int64), axis=-1)[..., 0]
    target = np.ones((h, w), bool) if only is None else np.asarray(only) != 0
    ok = target & (n >= min_count)
    assert (med[ok] != NONE).all()
    out_words = np.where(ok[..., None], unkey(np.where(med == NONE, 0, med).astype(np.uint32)).view(np.uint32), vecs.view(np.uint32))
    out_mask = np.where(target, ok, np.asarray(mask) != 0).astype(np.uint8)
    return out_words.astype(np.uint32).view(np.float32), out_mask, n


# ---------------------------------------------------------------------------------------------- the shared inputs
def vectors(shape, seed=5, specials=True):
    """random vectors, a third of them drawn from a few values so that equal keys abound, with NaNs of distinct payloads and
    both signs, +-Inf, +-0.0 and denormals planted (about one word in eight): a median moves bytes, it does not compute"""
    h, w = shape
    rng = np.random.default_rng(seed + 1000 * h + w)
    v = (rng.standard_normal((h, w, 2)) * 20).astype(np.float32)
    few = rng.random((h, w, 2)) < 0.33
    v[few] = rng.integers(-2, 3, int(few.sum())).astype(np.float32)
    if specials:
        flat = v.reshape(-1).view(np.uint32)
        at = rng.random(flat.size) < 0.125
        at[:min(flat.size, 2)] = True
        flat[at] = rng.choice(SPECIAL, int(at.sum()))
    return v


MASKS = ("all", "random50", "random5", "checker", "none", "one")


def mask(name, shape, seed=0):
    h, w = shape
    m = np.zeros((h, w), np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    if name == "all":
        m[:] = 1
    elif name == "checker":
        m[(x + y) % 2 == 0] = 1
    elif name == "one":
        m[h // 2, w // 3] = 1
    elif name.startswith("random"):
        share = {"random50": 0.5, "random5": 0.05}[name]
        m[np.random.default_rng(17 + seed + h * 131 + w).random((h, w)) < share] = 1
    elif name != "none":
        raise KeyError(name)
    return m


@functools.lru_cache(maxsize=None)
def _expected(name, shape, ksize, min_count):
    out = median(vectors(shape), mask(name, shape), ksize, None, None, min_count)
    for a in out:
        a.setflags(write=False)
    return out


def expected(name, shape, ksize, min_count=1):
    """median(vectors(shape), mask(name, shape), ksize, min_count=min_count), computed once per session and read-only"""
    return _expected(name, tuple(shape), int(ksize), int(min_count))
