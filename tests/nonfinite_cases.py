"""Flow fields with NaN, Inf and out-of-int32 vectors for the kernels that turn a flow vector into an address: K1
(ofl_gather.hip), K2 (ofl_compose3.hip), K12 (ofl_tensor.hip) and K13 (ofl_consistency.hip) -- a helper of
test_nonfinite_cases_host.py and test_gpu_nonfinite.py, not a test.  NumPy only.

The contract (include/ofl.h): a vector with a non-finite component samples nothing -- every tap is outside, the pixel is
invalid -- exactly as in the oracle, whose cv_round_f follows cvtss2si (NaN, Inf and everything beyond int32 -> INT_MIN).

A case is a clean field of test_gpu_compose3_paths._flows, restated here, plus a PLACEMENT of the patterns below:
    'class'   every pattern goes into at least one wave of every class the clean field has.  A wave of the tiled K2 is a
              128 px x 2 row strip of a 128 x 8 tile (ofl_compose3.hip, "Workgroup tile"), or, in a tile whose sampling grid is
              rotated, a 32 px x 8 row block; its class -- all taps inside, all outside, mixed -- is the oracle's, from the taps
              that `taps` below restates.  A mixed wave is the border path: pixel pairs under QUANT_OPENCV, single pixels else.
    'sprinkle' one bad vector every 37th pixel (every pixel of a field smaller than that allows), patterns in turn.

Why none of these inputs can make a kernel touch memory that is not its own (read before the first GPU run):

gather_kernel, compose3_generic_kernel, consistency_pixel, gather_nchw_kernel, gather_nhwc_kernel.  All take their taps from
make_tap, whose ix, iy are saturated to [-32768, 32767] in both quantisations (sat_s16 of an arithmetic shift; fmin / fmax
before the cast, which give -32768 for NaN), so ix + 1 and iy + 1 cannot overflow.  Every tap is then loaded behind
`(unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W` and its offset is 0 otherwise; the offsets of the outputs and of the
streamed flow come from the thread index alone.  NaN weights only reach arithmetic.  gather_nhwc_kernel forms the address of
a tap outside the frame (tensor_index of ix = -32768) but dereferences it only under its in-frame flag.

gather2_kernel (paired K1).  Taps are make_tap's again, saturated.  The wave is classified from them: `in_j` is an unsigned
compare against W - 2 / H - 2, `out_j` signed compares against -1, W, H.  The all-inside path (px_load, gather_px<INSIDE>) is
entered only if every active pixel of the wave has 0 <= ix <= W - 2 and 0 <= iy <= H - 2, so off0 = iy * W + ix and off0 + W + 1
are inside the image, and the padded 8- / 16-byte reads are checked against `total`; a NaN, Inf or far vector gives
ix = +-32768 / 32767, which is never inside, so such a wave takes gather_px<false>, which guards every tap as gather_kernel
does.  __umul24 sees only in-frame y < 32767 and W < 32767.  The flow and flow-mask loads are addressed from the pixel index.

compose3_xpose_kernel (tiled K2).  QUANT_EXACT clamps the tap to [-32768, 32767] with fmin / fmax before the cast (NaN ->
-32768).  QUANT_OPENCV uses s >> 5 UNSATURATED: s is any int32, so the tap lies in [-2^26, 2^26 - 1] and tap + 1 cannot
overflow.  c3_classify: inside needs (unsigned)ix <= W - 2 and (unsigned)iy <= H - 2, which no tap outside [0, W - 2] x [0, H - 2]
passes, so the interior gather (offsets iy * W + ix, + W, reads of 16 B of vectors and 2 or 4 B of mask, the latter only if
ix0 + 3 < W) sees in-frame taps only.  A wave that is all outside loads nothing.  Everything else goes through c3_border_px /
c3_border_pair, which clamp BEFORE they form an offset: ixc = min(max(ix, 0), max(W - 2, 0)), rows min(max(iy, 0), H - 1) and
min(max(iy + 1, 0), H - 1) with iy + 1 <= 2^26, so s0, s1 <= (H - 1) * W + W - 2 < 2^29 fit the 32-bit offsets and 2 * s * 4
bytes < 4 GiB as ofl_compose3_route.h requires; the loaded pair is columns ixc, ixc + 1 <= W - 1 (W >= 2 in the tiled kernel)
and which taps exist is decided by d = ix - ixc in {-1, 0, 1} and the unsigned row tests.  The bit-plane form reads the byte of
bit ixc and of min(ixc + 1, W - 1) in the border path and 4 bytes from the byte of bit ix in the interior, inside the 16 bytes
of slack of ofl_mask_bits_bytes.  The `rotated` decision reads fb at the two ends of the tile's first row and compares floats:
NaN compares false (direct form), Inf true (transposed form); both forms are the same guarded code per pixel.  Stores are
addressed from the thread index.  After this change a NaN coordinate is INT_MIN instead of 0: tap -2^26, outside.
"""
import functools
import zlib

import numpy as np

F32 = np.float32
QUANT_OPENCV, QUANT_EXACT = 0, 1
FINITE = 1.25                                   # the ordinary component of a bad vector
NAN, PINF, NINF = 0x7fc00000, 0x7f800000, 0xff800000
_f = lambda v: int(np.array(v, F32).view(np.uint32))
_BELOW = int(np.nextafter(F32(2.0 ** 26), F32(0)).view(np.uint32))       # the float32 below 2^26
# (name, bits of u, bits of v)
PATTERNS = [
    ('nan_f', NAN, _f(FINITE)), ('f_nan', _f(FINITE), NAN), ('nan_nan', NAN, NAN),
    ('negqnan_payload_f', 0xffc00001, _f(FINITE)), ('snan_f', 0x7f800001, _f(FINITE)),
    ('pinf_f', PINF, _f(FINITE)), ('f_ninf', _f(FINITE), NINF), ('pinf_ninf', PINF, NINF),
    ('p3e9_f', _f(3e9), _f(FINITE)), ('m3e9_f', _f(-3e9), _f(FINITE)),          # times 32: beyond int32
    ('p2_26_f', _f(2.0 ** 26), _f(FINITE)), ('m2_26_f', _f(-2.0 ** 26), _f(FINITE)),      # times 32: exactly 2^31
    ('p2_26_below_f', _BELOW, _f(FINITE)), ('m2_26_below_f', _BELOW | 0x80000000, _f(FINITE)),
]
NAMES = [p[0] for p in PATTERNS]
BITS = np.array([[p[1], p[2]] for p in PATTERNS], np.uint32)
NONFINITE = [i for i, p in enumerate(PATTERNS) if not np.isfinite(np.array(p[1:], np.uint32).view(F32)).all()]

SHAPES = [(2, 16, 256), (3, 21, 200), (2, 13, 130), (2, 13, 131), (1, 1, 1), (1, 3, 5)]
KINDS = ['shift', 'outside', 'rotate', 'random']
PLACEMENTS = ['class', 'sprinkle']
CLASSES = ['inside', 'outside', 'mixed']
TILE_W, TILE_H, XPOSE_ROWS = 128, 8, 6          # ofl_compose3.hip kC3TileW / kC3TileH, ofl_pairs.h kXposeRows


def flows(kind, B, H, W, rng):
    """test_gpu_compose3_paths._flows, restated (that module is a GPU test and is not imported here)"""
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    if kind == 'random':
        return (rng.standard_normal((B, H, W, 2)) * 6).astype('f')
    if kind == 'shift':
        f = np.zeros((B, H, W, 2), 'f')
        f[..., 0], f[..., 1] = 1.3, 0.6
        return f
    if kind == 'outside':
        return np.full((B, H, W, 2), 3.0e4, 'f')
    if kind == 'rotate':
        a = np.deg2rad(35.0)
        cx, cy = W / 2.0, H / 2.0
        u = (np.cos(a) - 1) * (xx - cx) - np.sin(a) * (yy - cy)
        v = np.sin(a) * (xx - cx) + (np.cos(a) - 1) * (yy - cy)
        return np.broadcast_to(np.stack([u, v], -1), (B, H, W, 2)).astype('f').copy()
    raise ValueError(kind)


def taps(f, sign, quant):
    """the oracle's top-left taps (ix, iy as int64) of a field [..., H, W, 2]: map_coord and make_tap of oracle/ofl_oracle.c"""
    H, W = f.shape[-3:-1]
    gy, gx = np.mgrid[0:H, 0:W]
    with np.errstate(all='ignore'):
        px = (gx.astype(np.float64) + sign * f[..., 0].astype(np.float64)).astype(F32)
        py = (gy.astype(np.float64) + sign * f[..., 1].astype(np.float64)).astype(F32)

        def tap(p):
            if quant == QUANT_OPENCV:                # cv_round_f: INT_MIN for NaN and for everything outside int32
                r = np.rint(p * F32(32.0))
                ok = (r >= F32(-2.0 ** 31)) & (r < F32(2.0 ** 31))
                s = np.where(ok, r, F32(-2.0 ** 31)).astype(np.int64)
                return np.clip(s >> 5, -32768, 32767)
            return np.fmin(np.fmax(np.floor(p), F32(-32768.0)), F32(32767.0)).astype(np.int64)
        return tap(px), tap(py)


def rotated_tiles(f):
    """[tiles_y, tiles_x] bool of one field [H, W, 2]: the decision compose3_xpose_kernel takes from the vertical flow at the two
    ends of a tile's first row"""
    H, W = f.shape[:2]
    ty, tx = -(-H // TILE_H), -(-W // TILE_W)
    rot = np.zeros((ty, tx), bool)
    with np.errstate(all='ignore'):
        for j in range(ty):
            for i in range(tx):
                x0, y = i * TILE_W, min(j * TILE_H, H - 1)
                x1 = min(x0 + TILE_W - 1, W - 1)
                rot[j, i] = np.abs(f[y, x1, 1] - f[y, x0, 1]) * F32(128.0) > F32(XPOSE_ROWS * (x1 - x0 + 1))
    return rot


def decision_pixels(f):
    """[H, W] bool: the pixels whose vertical flow decides `rotated` for their tile -- a placement leaves them alone"""
    H, W = f.shape[:2]
    d = np.zeros((H, W), bool)
    for y in range(0, H, TILE_H):
        for x0 in range(0, W, TILE_W):
            d[y, x0] = d[y, min(x0 + TILE_W - 1, W - 1)] = True
    return d


def waves(f, sign, quant):
    """The waves of the tiled K2 over one clean field [H, W, 2] -> a list of (layout, class, [(y, x), ...]): layout 'stream'
    (128 px x 2 rows) or 'block' (32 px x 8 rows, rotated tiles), class by the oracle's taps of the wave's pixels."""
    H, W = f.shape[:2]
    ix, iy = taps(f, sign, quant)
    inside = (ix >= 0) & (ix <= W - 2) & (iy >= 0) & (iy <= H - 2)
    outside = (ix < -1) | (ix >= W) | (iy < -1) | (iy >= H)
    rot = rotated_tiles(f)
    out = []
    for j in range(rot.shape[0]):
        for i in range(rot.shape[1]):
            y0, x0 = j * TILE_H, i * TILE_W
            if rot[j, i]:
                boxes = [(y0, y0 + 8, x0 + 32 * k, x0 + 32 * k + 32) for k in range(4)]
            else:
                boxes = [(y0 + 2 * k, y0 + 2 * k + 2, x0, x0 + TILE_W) for k in range(4)]
            for ya, yb, xa, xb in boxes:
                if ya >= H or xa >= W:
                    continue
                ys, xs = np.mgrid[ya:min(yb, H), xa:min(xb, W)]
                a, o = inside[ys, xs].all(), outside[ys, xs].all()
                cls = 'inside' if a else ('outside' if o else 'mixed')
                out.append(('block' if rot[j, i] else 'stream', cls, list(zip(ys.ravel().tolist(), xs.ravel().tolist()))))
    return out


def put(field, where, pattern):
    """write pattern `pattern` (bits, so that payloads and the signalling NaN arrive as they are) at field[where]"""
    field.view(np.uint32)[where] = BITS[pattern]


def place_class(fb, sign, quant=QUANT_OPENCV):
    """-> (field with bad vectors, bad [B, H, W] int8: pattern index or -1, reach {(layout, class, pattern): count})"""
    out, bad, reach = fb.copy(), np.full(fb.shape[:3], -1, np.int8), {}
    for b in range(fb.shape[0]):
        keep = decision_pixels(fb[b]) if fb.shape[2] % 2 == 0 else np.zeros(fb.shape[1:3], bool)      # (odd widths: the generic kernel)
        by = {}
        for layout, cls, px in waves(fb[b], sign, quant):
            by.setdefault((layout, cls), []).append([p for p in px if not keep[p]])
        for (layout, cls), ws in sorted(by.items()):
            ws = [w for w in ws if w]
            for p in range(len(PATTERNS)):
                if not ws:
                    break
                w = ws[(p + b) % len(ws)]
                free = [q for q in w if bad[b][q] < 0]
                if not free:
                    continue
                q = free[(7 * p + 3) % len(free)]
                put(out[b], q, p)
                bad[b][q] = p
                reach[(layout, cls, p)] = reach.get((layout, cls, p), 0) + 1
    return out, bad, reach


def place_sprinkle(fb):
    """one bad vector every 37th pixel, the patterns in turn; every pixel of a field too small for one round of them"""
    out, bad = fb.copy(), np.full(fb.shape[:3], -1, np.int8)
    n = bad.size
    step = 37 if n >= 37 * len(PATTERNS) else 1
    flat_o, flat_b = out.reshape(-1, 2), bad.reshape(-1)
    for k, i in enumerate(range(0, n, step)):
        p = (k + 2) % len(PATTERNS)                              # (starts at (NaN, NaN): the one pixel of a 1 x 1 field)
        put(flat_o, i, p)
        flat_b[i] = p
    return out, bad


@functools.lru_cache(maxsize=None)
def case(shape, kind, placement, sign=-1):
    """One case, built once and shared, read-only: dict(fa, ma, fb, mb: the bad field and the data it samples; clean: the field
    before the placement; bad: [B, H, W] pattern index or -1; reach: what place_class counted, {} for 'sprinkle')."""
    B, H, W = shape
    rng = np.random.default_rng([B, H, W, zlib.crc32(kind.encode()) & 0xffff])
    fa = (rng.standard_normal((B, H, W, 2)) * 4).astype('f')
    clean = flows(kind, B, H, W, rng)
    ma = (rng.random((B, H, W)) > 0.1).astype(np.uint8)
    mb = (rng.random((B, H, W)) > 0.1).astype(np.uint8)
    if placement == 'class':
        fb, bad, reach = place_class(clean, sign)
    else:
        (fb, bad), reach = place_sprinkle(clean), {}
    c = dict(fa=fa, ma=ma, fb=fb, mb=mb, clean=clean, bad=bad, reach=reach, shape=shape, kind=kind, placement=placement, sign=sign)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return c


def poisoned_source(shape=(2, 13, 130), seed=5):
    """finite flows (border and interior mixed, a few on exact integers so that taps of weight 0 occur) over SAMPLED data with
    NaN, +Inf and -Inf in it -> (fa with bad values, ma, fb, mb)"""
    B, H, W = shape
    rng = np.random.default_rng(seed)
    fa = (rng.standard_normal((B, H, W, 2)) * 4).astype('f')
    fb = (rng.standard_normal((B, H, W, 2)) * 3).astype('f')
    fb[:, ::2, ::3] = np.rint(fb[:, ::2, ::3])                    # integer positions: three taps of weight 0
    fb[:, 1::2, ::5, 0] = np.rint(fb[:, 1::2, ::5, 0])            # integer x only: two taps of weight 0
    flat = fa.reshape(-1)
    k = rng.choice(flat.size, flat.size // 23, replace=False)
    flat.view(np.uint32)[k] = np.array([NAN, PINF, NINF, 0xffc00001], np.uint32)[np.arange(k.size) % 4]
    ma = (rng.random((B, H, W)) > 0.1).astype(np.uint8)
    mb = (rng.random((B, H, W)) > 0.1).astype(np.uint8)
    return fa, ma, fb, mb


def same_floats(got, want):
    """NaN where `want` has NaN (payloads are the processor's own), identical bits everywhere else (+-Inf and -0.0 included)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    nan = np.isnan(want)
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[want.itemsize]
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(u)[~nan], want.view(u)[~nan]))
