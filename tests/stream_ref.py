"""NumPy statement of the streaming kernels of oflibnumpy_amd/csrc/ofl_stats.hip (K4 statistics, K5 axpy, flow extent,
mask and, dtype conversion, grid offset, point sampling) and of the mask packing of ofl_compose3.hip -- a helper of
test_stream_host.py and test_gpu_stream.py, not a test.

Every function is the definition of include/ofl.h in explicit float32 / float64 NumPy operations, in the order of the
definition, so the device result is compared with array_equal on bit views and nothing has a tolerance.  The size lists and
the case generators of the two test files live here too: the host test proves from the restatement alone what the generated
cases reach, the GPU test runs exactly those cases."""
import functools

import numpy as np

from oracle import np_oracle as O

F32, F64 = np.float32, np.float64
TH = F32(1e-3)                                   # DEFAULT_THRESHOLD, compared in float32
NONZERO_MASKED, NONZERO_TH_MASKED, NONZERO, NONZERO_TH, NONFINITE, MASK_HAS_ZERO = 1, 2, 4, 8, 16, 32      # OFL_STAT_*
U8, I16, U16, F32_CODE, F64_CODE = 0, 1, 2, 3, 4   # OFL_U8 .. OFL_F64
DTYPES = {U8: np.uint8, I16: np.int16, U16: np.uint16, F32_CODE: np.float32, F64_CODE: np.float64}
CONVERT_PAIRS = [(s, F32_CODE) for s in (U8, I16, U16, F32_CODE, F64_CODE)] + [(F32_CODE, d) for d in (U8, I16, U16, F64_CODE)]

# ------------------------------------------------------------------------------------------------- sizes (pixels / bytes / shapes)
STATS_WG = 4096                                  # pixels per workgroup of the statistics kernel: 8 chunks x 256 threads x 2 px
STATS_SIZES = [1, 2, 3, 4095, 4096, 4097, 4098, 8191, 8193, 3 * 4096 + 511, 40961]
AXPY_UNIT, AXPY_WG = 256, 1024                   # pixels per wave unit / per workgroup of the axpy kernel
AXPY_SIZES = [1, 3, 255, 256, 257, 1023, 1024, 1025, 5 * 1024 + 77, 33 * 1024 + 255]
AXPY_ALPHAS = [1.0, -1.0, 0.5, 1.0 / 3.0, -2.75]
EXTENT_SHAPES = [(1, 1), (1, 9), (9, 1), (37, 53), (2, 32766), (513, 512)]
EXTENT_GRID_CAP = 1024 * 256                     # threads of the extent kernel's largest grid: a larger field is strided over
MASK_AND_SIZES = [1, 2, 3, 4, 5, 1023, 1024, 1027, 65537]
CONVERT_SIZES = [1, 255, 256, 257, 70001]
GRID_OFFSET_SHAPES = [(1, 1), (1, 300), (300, 1), (37, 53), (2, 32766)]
SAMPLE_FIELDS = [(1, 1), (1, 7), (7, 1), (37, 53)]
SAMPLE_COUNTS = [1, 255, 257, 10000]
PACK_WIDTHS = [1, 31, 32, 33, 45, 64, 96, 130, 4112]
PACK_HEIGHTS = [1, 9]
PACK_BATCHES = [1, 3]


# ------------------------------------------------------------------------------------------------- K4: the statistics word
def stats_word(vecs, mask, th=TH):
    """-> int, the OR of the OFL_STAT_* bits of n vectors (any shape (.., 2)) and n mask bytes, or None for "no mask"."""
    v = np.ascontiguousarray(vecs, F32).reshape(-1, 2)
    n = v.shape[0]
    m = np.ones(n, bool) if mask is None else (np.asarray(mask).reshape(-1) != 0)
    assert m.shape == (n,)
    th = F32(th)
    nz = (v != 0).any(axis=1)
    nzt = (~((v < th) & (v > -th))).any(axis=1)
    finite = bool(np.isfinite(v).all())
    word = ((NONZERO_MASKED if (nz & m).any() else 0) | (NONZERO_TH_MASKED if (nzt & m).any() else 0) |
            (NONZERO if nz.any() else 0) | (NONZERO_TH if nzt.any() else 0) | (0 if finite else NONFINITE) |
            (MASK_HAS_ZERO if mask is not None and not m.all() else 0))
    if n and th == TH:
        # the four zero-flow bits are the oracle's predicates: is_zero_flow (utils.py:527-544) over all vectors and,
        # as Flow.is_zero does (flow_class.py:1244), over vecs[mask]; is_zero_raw is the C form of the same -- on non-finite
        # input too: a NaN component is non-zero and >= threshold in all three
        for thresholded, bit_all, bit_masked in ((False, NONZERO, NONZERO_MASKED), (True, NONZERO_TH, NONZERO_TH_MASKED)):
            assert bool(word & bit_all) == (not O.is_zero_flow(v[None], thresholded)) == (not O.is_zero_raw(v[None], None, thresholded))
            assert (bool(word & bit_masked) == (not O.is_zero_flow(v[m][None], thresholded))
                    == (not O.is_zero_raw(v[None], m[None], thresholded)))
    return word


# ------------------------------------------------------------------------------------------------- K5: out = a + alpha * b
def axpy(a, ma, b, mb, alpha):
    """-> (vectors float32, mask bytes or None): a + float32(alpha) * b as TWO float32 operations (a product, rounded, then a
    sum, rounded), or float32(alpha) * a without b; ma & mb on bytes (ma alone without mb, None without ma)."""
    a, al = np.ascontiguousarray(a, F32), F32(alpha)
    with np.errstate(all='ignore'):
        if b is None:
            out = al * a
        else:
            prod = al * np.ascontiguousarray(b, F32)
            assert prod.dtype == F32
            out = a + prod
    assert out.dtype == F32
    mout = None if ma is None else (np.asarray(ma, np.uint8) if mb is None else np.asarray(ma, np.uint8) & np.asarray(mb, np.uint8))
    return out, mout


def axpy_fused(a, b, alpha):
    """what a contracted multiply-add would give: the exact product (float64 holds it) added in float64, rounded to float32"""
    with np.errstate(all='ignore'):
        return (np.asarray(a, F32).astype(F64) + F64(F32(alpha)) * np.asarray(b, F32).astype(F64)).astype(F32)


# ------------------------------------------------------------------------------------------------- flow extent, grid offset
def positions(vecs, sign):
    """float32((x, y) + sign * vecs): NumPy adds the int64 grid to the float32 array in float64 and rounds once -> (px, py)"""
    v = np.ascontiguousarray(vecs, F32)
    h, w = v.shape[:2]
    ys, xs = np.mgrid[:h, :w]
    px = (xs.astype(F64) + sign * v[..., 0].astype(F64)).astype(F32)
    py = (ys.astype(F64) + sign * v[..., 1].astype(F64)).astype(F32)
    return px, py


def grid_offset(vecs, sign):
    return np.stack(positions(vecs, sign), axis=-1)


def extent(vecs, mask, sign, th=TH):
    """float32 [4] = (min y, max y, min x, max x) of the positions of the thresholded vectors over mask != 0;
    (+inf, -inf, +inf, -inf) when no pixel is masked.  th=None: no thresholding (for the reach assertions only)."""
    v = np.array(vecs, F32)
    if th is not None:
        v[(v < F32(th)) & (v > -F32(th))] = 0        # threshold_vectors, utils.py:310-315, per component
    px, py = positions(v, sign)
    m = np.ones(px.shape, bool) if mask is None else (np.asarray(mask) != 0)
    if not m.any():
        return np.array([np.inf, -np.inf, np.inf, -np.inf], F32)
    return np.array([py[m].min(), py[m].max(), px[m].min(), px[m].max()], F32)


def padding(vecs, mask, sign, th=TH):
    """[top, bottom, left, right] as DeviceFlow.get_padding computes it from the extent (flow_class.py:1221-1227);
    sign -1 for ref 't', +1 for 's'"""
    h, w = np.asarray(vecs).shape[:2]
    min_y, max_y, min_x, max_x = (float(e) for e in extent(vecs, mask, sign, th))
    if not np.isfinite(min_y):
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    return [int(np.ceil(p)) for p in (max(-min_y, 0), max(max_y - (h - 1), 0), max(-min_x, 0), max(max_x - (w - 1), 0))]


# ------------------------------------------------------------------------------------------------- conversion, sampling
def convert(src, dst_dtype):
    with np.errstate(all='ignore'):
        return np.asarray(src).astype(dst_dtype)


def sample_points(flow, pts_rc):
    """float64 [n][2] = (v, u) at (row, col): the reference's bilinear_interpolation on the flipped field (utils.py:605)"""
    return O.bilinear_interpolation(np.ascontiguousarray(flow, F32)[..., ::-1], np.ascontiguousarray(pts_rc, F64))


# ------------------------------------------------------------------------------------------------- mask bit planes
def pack_bits(mask, H, W, batch):
    """uint32 [batch][H][(W + 31) // 32]: bit (x & 31) of word (x >> 5) of a row is set iff the byte is not 0"""
    wpr = (W + 31) // 32
    padded = np.zeros((batch, H, wpr * 32), np.uint8)
    padded[..., :W] = np.asarray(mask).reshape(batch, H, W) != 0
    return np.ascontiguousarray(np.packbits(padded, axis=-1, bitorder='little')).view('<u4').astype(np.uint32)


def unpack_bits(bits, H, W, batch):
    """uint8 [batch][H][W] of 0 / 1, the inverse of pack_bits"""
    b = np.ascontiguousarray(np.asarray(bits, np.uint32).reshape(batch, H, (W + 31) // 32).astype('<u4')).view(np.uint8)
    return np.ascontiguousarray(np.unpackbits(b, axis=-1, bitorder='little')[..., :W])


def pack_paths(H, W, batch):
    """(words packed from two 16-byte loads, words packed byte by byte) for a mask plane at a 16-byte aligned address:
    a word takes the loads when all its 32 bytes are inside the row and start 16-byte aligned"""
    wpr = (W + 31) // 32
    r, k = np.mgrid[:batch * H, :wpr]
    wide = (k * 32 + 32 <= W) & ((r * W + k * 32) % 16 == 0)
    return int(wide.sum()), int((~wide).sum())


# ------------------------------------------------------------------------------------------------- K4 cases
def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.flags.writeable = False
    return arrays


def stats_positions(n):
    """the pixels of the single-cause sweep: the first pixels, both sides of every 512-pixel chunk edge of the first
    workgroup (256 threads x 2 px), both sides of the workgroup edge, the middle and the last two pixels"""
    p = {0, 1, 2, 3, 510, 511, 512, 513, 4094, 4095, 4096, 4097, n // 2, n - 2, n - 1}
    for k in range(1, 9):
        p |= {k * 512 - 1, k * 512}
    return sorted(q for q in p if 0 <= q < n)


SUBNORMAL = np.nextafter(F32(0), F32(1))
BELOW_TH = np.nextafter(TH, F32(0))
# kind -> (vector, mask byte) of the one changed pixel of the sweep; everything else is a zero vector under mask 1
STATS_KINDS = {
    'a': ((0.0, 7e-4), 1),
    'b+': ((TH, 0.0), 1), 'b-': ((-TH, 0.0), 1),
    'c+': ((BELOW_TH, 0.0), 1), 'c-': ((0.0, -BELOW_TH), 1),
    'd': ((SUBNORMAL, 0.0), 1),
    'e': ((0.0, -0.0), 1),
    'f-nan-u': ((np.nan, 0.0), 1), 'f-nan-v': ((0.0, np.nan), 1), 'f+inf': ((np.inf, 0.0), 1), 'f-inf': ((0.0, -np.inf), 1),
    'g': ((0.0, 0.0), 0),
    'h': ((3.0, 0.0), 0),
    'i': ((np.nan, 0.0), 0),
}


@functools.lru_cache(maxsize=None)
def stats_cases():
    """the seeded random cases of the statistics word: [(name, vecs float32 (n, 2), mask uint8 (n,))], read-only"""
    rng = np.random.default_rng(4)
    cases = []

    def add(name, v, m):
        cases.append((name,) + _frozen(np.ascontiguousarray(v, F32), np.ascontiguousarray(m, np.uint8)))

    def small(n):            # non-zero components strictly inside the threshold
        return (rng.uniform(1e-5, 9e-4, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))).astype(F32)

    for n in (5, 4097, 8191, 12345, 40961):
        ones, holes = np.ones(n, np.uint8), (rng.random(n) > 0.3).astype(np.uint8)
        holes[rng.integers(n)] = 0
        p = int(rng.integers(n))                                  # one pixel anywhere, also in a late workgroup
        add("zero/ones/{}".format(n), np.zeros((n, 2)), ones)
        add("zero/holes/{}".format(n), np.zeros((n, 2)), holes)
        add("small/holes/{}".format(n), small(n), holes)
        add("normal/ones/{}".format(n), rng.standard_normal((n, 2)), ones)
        v, m = np.zeros((n, 2), F32), ones.copy()
        v[p], m[p] = (0.0, -2.5), 0
        add("nonzero only under mask 0/{}".format(n), v, m)
        v, m = np.zeros((n, 2), F32), ones.copy()
        v[p], m[p] = (5e-4, 0.0), 0
        add("small only under mask 0/{}".format(n), v, m)
        v = np.zeros((n, 2), F32)
        v[p] = (0.0, 2e-4)
        add("one small vector/ones/{}".format(n), v, ones)
        v, m = small(n), holes.copy()
        v[p, 1], m[p] = np.nan, 0
        add("nan under mask 0 in small/{}".format(n), v, m)
        v = rng.standard_normal((n, 2)).astype(F32)
        v[p, 0] = -np.inf
        add("inf in normal/holes/{}".format(n), v, holes)
    return cases


# ------------------------------------------------------------------------------------------------- K5 cases
@functools.lru_cache(maxsize=None)
def axpy_inputs(n):
    """(a, ma, b, mb) of n pixels: standard normals with planted signed zeros, infinities, NaN and values at both ends of
    the float32 range -- at the start, around the wave-unit and workgroup edges and in the tail when n reaches them; masks of
    0 / 1 with some other non-zero bytes"""
    rng = np.random.default_rng(1000 + n)
    a, b = rng.standard_normal((n, 2)).astype(F32), rng.standard_normal((n, 2)).astype(F32)
    fmax, fmin = np.finfo(F32).max, np.finfo(F32).tiny
    plant = [(0.0, -0.0), (-0.0, 0.0), (np.inf, 1.0), (-np.inf, np.inf), (np.inf, -np.inf), (np.nan, 1.0), (1.0, np.nan),
             (fmax, fmax), (-fmax, 0.9 * fmax), (fmin, fmin), (-fmin, 1.5 * fmin), (fmax, -fmin), (SUBNORMAL, 3 * SUBNORMAL), (0.0, 0.0)]
    flat_a, flat_b = a.reshape(-1), b.reshape(-1)
    for start in (0, 2 * AXPY_UNIT - len(plant) // 2, 2 * AXPY_WG - 3, 2 * (n - n % AXPY_UNIT), 2 * n - len(plant)):
        for k, (pa, pb) in enumerate(plant):
            if 0 <= start + k < 2 * n:
                flat_a[start + k], flat_b[start + k] = pa, pb
    ma, mb = (rng.random(n) > 0.3).astype(np.uint8), (rng.random(n) > 0.3).astype(np.uint8)
    # "valid" bytes other than 1, so that the AND is seen to be one of bytes: 2 & 128 is 0, 255 & 3 is 3, 255 alone stays 255
    ma[rng.random(n) < 0.1], mb[rng.random(n) < 0.1] = 2, 128
    ma[rng.random(n) < 0.1], mb[rng.random(n) < 0.1] = 255, 3
    ma[n - 1], mb[n - 1] = 255, 3                               # one in the tail, or in the last unit
    return _frozen(a, ma, b, mb)


def fused_differs(n, alpha):
    """the number of elements of axpy_inputs(n) where a contracted multiply-add would give other bits than the two roundings"""
    a, _, b, _ = axpy_inputs(n)
    two, one = axpy(a, None, b, None, alpha)[0], axpy_fused(a, b, alpha)
    return int(((two.view(np.uint32) != one.view(np.uint32)) & ~np.isnan(two)).sum())


# ------------------------------------------------------------------------------------------------- extent cases
@functools.lru_cache(maxsize=None)
def extent_cases(shape):
    """[(name, sign, vecs float32 (h, w, 2), mask uint8 (h, w))], read-only.  `towards` below is sign * v, the displacement
    of the position from the grid node, so that each case means the same for both signs."""
    h, w = shape
    n = h * w
    rng = np.random.default_rng(7 * h + w)
    ys, xs = np.mgrid[:h, :w]
    grid = np.stack([xs, ys], -1).astype(F64)
    ones = np.ones((h, w), np.uint8)
    cases = []
    for sign in (1, -1):
        def add(name, towards, m):
            cases.append((name, sign) + _frozen(np.ascontiguousarray(sign * towards, F32), np.ascontiguousarray(m, np.uint8)))

        holes = (rng.random((h, w)) > 0.4).astype(np.uint8)
        holes.reshape(-1)[rng.integers(n)] = 1
        add("random", rng.standard_normal((h, w, 2)) * 3, holes)
        # every component below the threshold; the corner pixels, which hold the extremes, point outwards by 7e-4:
        # thresholded, no padding is needed; unthresholded, one pixel at the top and the left
        t = rng.uniform(-9e-4, 9e-4, (h, w, 2))
        t[0, 0] = (-7e-4, -7e-4)
        add("threshold", t, ones)
        add("negative", -(grid + 2 + rng.random((h, w, 2))), ones)
        add("positive", 1 + rng.random((h, w, 2)) * 5, ones)
        one = np.zeros((h, w), np.uint8)
        one.reshape(-1)[rng.integers(n)] = 1
        add("one pixel", rng.standard_normal((h, w, 2)) * 3, one)
        add("none", rng.standard_normal((h, w, 2)) * 3, np.zeros((h, w), np.uint8))
        t = rng.standard_normal((h, w, 2)) * 3
        t[0, 0] = (-1000.25, -2000.5)
        add("minima at pixel 0", t, ones)
        t = rng.standard_normal((h, w, 2)) * 3
        t[h - 1, w - 1] = (1000.25, 2000.5)
        add("maxima at the last pixel", t, ones)
    return cases


# ------------------------------------------------------------------------------------------------- conversion inputs
@functools.lru_cache(maxsize=None)
def convert_input(src_code, dst_code, n):
    """n source elements of one supported dtype pair: the edge values first, then a sweep, repeated up to n"""
    rng = np.random.default_rng(100 * src_code + 10 * dst_code + n % 7)
    src = DTYPES[src_code]
    if src_code in (U8, I16, U16):
        lo, hi = np.iinfo(src).min, np.iinfo(src).max
        base = np.concatenate([[lo, hi, 0, 1], np.arange(lo, hi + 1)]).astype(src)
    elif src_code == F64_CODE:
        fmax, tiny, sub = F64(np.finfo(F32).max), F64(np.finfo(F32).tiny), F64(SUBNORMAL)
        base = np.concatenate([[1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, -(1 + 2.0 ** -24), 1 + 2.0 ** -24 + 2.0 ** -50, np.inf, -np.inf, np.nan,
                                1e39, -1e39, fmax * (1 + 2.0 ** -26), fmax * (1 + 2.0 ** -24), 0.0, -0.0,
                                1e-40, -1e-40, sub * 0.5, sub * 1.5, -sub * 0.5, sub * 0.75, 1e-46, -1e-46, tiny * (1 - 2.0 ** -25), tiny / 3],
                               rng.standard_normal(200) * 10.0 ** rng.integers(-30, 30, 200)])
    elif dst_code in (U8, I16, U16):
        lo, hi = np.iinfo(DTYPES[dst_code]).min, np.iinfo(DTYPES[dst_code]).max
        frac = {U8: [2.5, 254.999, 0.999, 3.5], I16: [2.5, -2.5, -0.5, 32766.5, -32767.5], U16: [2.5, 65534.5, 0.999]}[dst_code]
        base = np.concatenate([[lo, hi], frac, np.arange(lo, hi + 1)]).astype(F32)
    else:                                           # float32 -> float32 / float64
        fmax, tiny = np.finfo(F32).max, np.finfo(F32).tiny
        base = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, np.nan, fmax, -fmax, tiny, -tiny, SUBNORMAL, -SUBNORMAL, 1e-40], F32),
                               (rng.standard_normal(200) * 10.0 ** rng.integers(-30, 30, 200)).astype(F32)])
    return _frozen(np.ascontiguousarray(np.resize(base, n)))[0]


# ------------------------------------------------------------------------------------------------- grid offset / sampling inputs
@functools.lru_cache(maxsize=None)
def offset_field(shape):
    """vectors of about 1e5, of about 1, subnormals and signed zeros, mixed"""
    h, w = shape
    rng = np.random.default_rng(31 * h + w)
    v = rng.standard_normal((h, w, 2))
    kind = rng.integers(0, 5, (h, w, 2))
    v = np.where(kind == 0, v * 1e5, v)
    v = np.where(kind == 1, 0.0, v)
    v = np.where(kind == 2, -0.0, v)
    v = np.where(kind == 3, np.sign(v) * F64(SUBNORMAL) * rng.integers(1, 9, (h, w, 2)), v).astype(F32)
    return _frozen(v)[0]


@functools.lru_cache(maxsize=None)
def sample_case(shape, n):
    """(flow float32 (h, w, 2), points float64 (n, 2) in (row, col)): random interior points, integer points, points on the last
    row / column / corner, on row 0 / column 0, and just below an integer; every point inside [0, h - 1] x [0, w - 1]"""
    h, w = shape
    rng = np.random.default_rng(1000 * h + w + n)
    flow = (rng.standard_normal((h, w, 2)) * 4).astype(F32)
    i = np.arange(n)
    rnd = rng.random((n, 2)) * [h - 1, w - 1]
    whole = np.stack([rng.integers(0, h, n), rng.integers(0, w, n)], 1).astype(F64)
    below = np.nextafter(np.maximum(whole, 0.0), 0.0)          # 0 stays 0, k >= 1 becomes the float64 just below it
    pts = rnd.copy()
    for cls, (rows, cols) in enumerate([(rnd[:, 0], rnd[:, 1]), (whole[:, 0], whole[:, 1]), (np.full(n, h - 1.0), rnd[:, 1]),
                                        (rnd[:, 0], np.full(n, w - 1.0)), (np.full(n, h - 1.0), np.full(n, w - 1.0)),
                                        (np.zeros(n), rnd[:, 1]), (rnd[:, 0], np.zeros(n)), (below[:, 0], rnd[:, 1]),
                                        (whole[:, 0], below[:, 1]), (below[:, 0], below[:, 1])]):
        sel = i % 10 == cls
        pts[sel, 0], pts[sel, 1] = rows[sel], cols[sel]
    assert ((pts >= 0) & (pts <= [h - 1, w - 1])).all()
    return _frozen(flow, np.ascontiguousarray(pts, F64))


# ------------------------------------------------------------------------------------------------- pack inputs
@functools.lru_cache(maxsize=None)
def pack_masks(H, W, batch):
    """[(name, mask uint8 (batch, H, W))]: random 0 / 1, all ones, all zeros, and non-zero bytes other than 1"""
    rng = np.random.default_rng(H * 10000 + W * 10 + batch)
    rnd = (rng.random((batch, H, W)) > 0.5).astype(np.uint8)
    other = rnd * rng.choice(np.array([1, 2, 128, 255], np.uint8), (batch, H, W))
    return [("random",) + _frozen(rnd), ("ones",) + _frozen(np.ones((batch, H, W), np.uint8)),
            ("zeros",) + _frozen(np.zeros((batch, H, W), np.uint8)), ("bytes 2, 128, 255",) + _frozen(other)]
