"""One case table for the four zero-flow predicates (non-zero / >= 1e-3, under the mask / anywhere; utils.py:527-544,
flow_class.py:1230-1245) -- a helper of test_zero_cases_host.py and test_gpu_zero_predicates.py, not a test.

The predicates are computed in several places: the oracle (orc_is_zero in C, is_zero_flow in NumPy), K4 (ofl_flow_stats_dev) and
the generic compose kernel (stat_bits), and the tiled K2 (running maxima in C3Stat, flushed as flag words).  The reference's
comparisons make a NaN component non-zero AND >= threshold; a producer that takes a float maximum drops it.  Every row here is a
field that is exactly zero except for ONE special value (in one or a few pixels), so the value alone decides the words:

    VALUES      +NaN, -NaN, a payload quiet NaN, the signalling pattern 0x7f800001 (all planted as bits), +-Inf, and as controls
                5e-4, the floats below / at / above the threshold, a subnormal and -0.0;
    PLACEMENTS  u of pixel (0, 0); v of the field's last pixel; u at an odd column (the second pixel of a streamed pair); the
                ragged last column pair and tile row of (50, 258); one pixel per wave row (2 rows x 128 px of a tile), u and v in turn;
    mask        the value under mask 1 (all four words follow it) or only under mask 0 (the masked words stay clear);
    kinds       'fb'        the streamed field, everything else zero (streaming layout unless an Inf sits on a probe pixel);
                'rot'       test_gpu_compose3_flags' fb_unmasked construction: a rotation where mb == 0, zero where mb == 1 (the
                            transposed layout), the value under mb == 1 -- words 6/7 come from the rotation, 4/5 from the value
                            alone -- or, mirrored, under mb == 0 (4/5 clear);
                'fa'        the SAMPLED field holds the value (masked or only under ma == 0), fb zero or a 0.3 px shift.
    SHAPES      (16, 256) whole tiles, (50, 258) ragged tile rows and a ragged column pair, (9, 37) odd W: the generic kernel.

Every row carries its expected booleans per field, computed from O.is_zero_raw.  Nothing here can fault: values only."""
import functools

import numpy as np

import nonfinite_cases as N
from oracle import np_oracle as O

F32 = np.float32
TH = F32(1e-3)
SHAPES = [(16, 256), (50, 258), (9, 37)]
_b = lambda v: int(np.array(v, F32).view(np.uint32))
VALUES = {
    'pnan': 0x7fc00000, 'nnan': 0xffc00000, 'payload': 0x7fc12345, 'snan': 0x7f800001, 'pinf': 0x7f800000, 'ninf': 0xff800000,
    'f5e-4': _b(5e-4), 'below_th': _b(np.nextafter(TH, F32(0))), 'th': _b(TH), 'above_th': _b(np.nextafter(TH, F32(1))),
    'subnormal': 1, 'negzero': 0x80000000,
}
NAN_VALUES = ('pnan', 'nnan', 'payload', 'snan')
NONFINITE_VALUES = NAN_VALUES + ('pinf', 'ninf')
PLACEMENTS = ['u_first', 'v_last', 'odd_x', 'ragged', 'wave_rows']
CONSUMER_PLACEMENTS = ('u_first', 'v_last')      # the rows the end-to-end checks take as operands


def is_tiled(shape):
    """the route of ofl_compose3_dev (ofl_compose3_route.h) at these sizes: even widths take the tiled kernel"""
    return shape[1] % 2 == 0


def pixels(placement, shape):
    """[(y, x, component)] of a placement, or None where the shape has no such place"""
    H, W = shape
    if placement == 'u_first':
        return [(0, 0, 0)]
    if placement == 'v_last':
        return [(H - 1, W - 1, 1)]
    if placement == 'odd_x':
        return [(H // 2, (W // 3) | 1, 0)]
    if placement == 'ragged':                   # columns 256, 257 and rows 48, 49 of (50, 258): the pair's second pixel
        return [(H - 2, W - 1, 1)] if (H % N.TILE_H and W % N.TILE_W == 2) else None
    if placement == 'wave_rows':                # one pixel in every 2-row strip of every tile column, on the strip's odd row
        px = []
        for k, y in enumerate(range(1, H, 2)):
            for x0 in range(0, W, N.TILE_W):
                wd = min(N.TILE_W, W - x0)
                px.append((y, x0 + (37 * k + 5) % wd, k & 1))
        return px
    raise ValueError(placement)


def plant(field, px, value):
    field.view(np.uint32).reshape(field.shape)[tuple(zip(*px))] = VALUES[value]


def rotation(H, W):
    """test_gpu_compose3_flags._rotation: 35 degrees about the centre"""
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    a = np.deg2rad(35.0)
    cx, cy = W / 2.0, H / 2.0
    u = (np.cos(a) - 1) * (xx - cx) - np.sin(a) * (yy - cy)
    v = np.sin(a) * (xx - cx) + (np.cos(a) - 1) * (yy - cy)
    return np.stack([u, v], -1).astype('f')


def predicates(vecs, mask):
    """the four words of one field in OFL_STAT_* order, from the C oracle"""
    return [not O.is_zero_raw(vecs, mask, False), not O.is_zero_raw(vecs, mask, True),
            not O.is_zero_raw(vecs, None, False), not O.is_zero_raw(vecs, None, True)]


def _finite_fa(H, W, rng):
    """finite, non-zero away from the edges, so that fb zero or a sub-pixel shift gathers its content"""
    fa = np.zeros((H, W, 2), 'f')
    fa[2:H - 2, 2:W - 2] = (rng.standard_normal((H - 4, W - 4, 2)) * 4).astype('f')
    return fa


def _row(kind, shape, value, placement, under, **extra):
    H, W = shape
    rng = np.random.default_rng([H, W, list(VALUES).index(value), PLACEMENTS.index(placement), under, len(kind)])
    px = pixels(placement, shape)
    where = tuple(zip(*[(y, x) for y, x, _ in px]))
    fa, ma = _finite_fa(H, W, rng), (rng.random((H, W)) > 0.1).astype(np.uint8)
    mb = (rng.random((H, W)) > 0.3).astype(np.uint8)
    if kind == 'fb':
        fb = np.zeros((H, W, 2), 'f')
        plant(fb, px, value)
        mb[where] = under
    elif kind == 'rot':
        mb = (rng.random((H, W)) > 0.5).astype(np.uint8)
        probe = np.zeros((H, W), bool)            # the pixels the layout decision reads keep their rotation values
        probe[::8, :] = probe[:, ::128] = probe[:, 127::128] = probe[:, W - 1] = True
        mb[probe] = 0
        if placement == 'u_first':                # the first and the last pixel that no layout decision reads
            px = [(1, 1, 0)]
        elif placement == 'v_last':
            y = H - 1 if (H - 1) % 8 else H - 2
            px = [(y, max(x for x in range(W) if not probe[y, x]), 1)]
        px = [p for p in px if not probe[p[0], p[1]]]
        assert px, (shape, placement)
        where = tuple(zip(*[(y, x) for y, x, _ in px]))
        mb[where] = under
        fb = rotation(H, W)
        fb[mb != 0] = 0
        fb[where] = 0                              # the planted pixel is zero but for the value
        plant(fb, px, value)
    elif kind == 'fa':
        fa = np.zeros((H, W, 2), 'f')
        plant(fa, px, value)
        ma[where] = under
        fb = np.zeros((H, W, 2), 'f')
        if extra.get('shift'):
            fb[...] = 0.3
    else:
        raise ValueError(kind)
    name = "{}-{}x{}-{}-{}-m{}{}".format(kind, H, W, value, placement, under, "-shift" if extra.get('shift') else "")
    r = dict(name=name, kind=kind, shape=shape, value=value, placement=placement, under=under, px=px, fa=fa, ma=ma, fb=fb, mb=mb,
             shift=bool(extra.get('shift')), expect_a=predicates(fa, ma), expect_b=predicates(fb, mb),
             nonfinite_a=not np.isfinite(fa).all(), nonfinite_b=not np.isfinite(fb).all())
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return r


@functools.lru_cache(maxsize=None)
def rows(shape):
    """every row of one shape, built once and shared, read-only"""
    out = []
    for placement in PLACEMENTS:
        if pixels(placement, shape) is None:
            continue
        for value in VALUES:
            for under in (1, 0):
                out.append(_row('fb', shape, value, placement, under))
                if is_tiled(shape) and placement in ('u_first', 'v_last', 'wave_rows'):
                    out.append(_row('rot', shape, value, placement, under))
                if placement in ('odd_x', 'wave_rows'):
                    out.append(_row('fa', shape, value, placement, under, shift=False))
                    if under:
                        out.append(_row('fa', shape, value, placement, under, shift=True))
    return out


def all_rows():
    return [r for s in SHAPES for r in rows(s)]


def layouts(r):
    """(tiles in the streaming layout, tiles in the transposed layout) of the tiled kernel on this row's fb"""
    rot = N.rotated_tiles(r['fb'])
    return int((~rot).sum()), int(rot.sum())


@functools.lru_cache(maxsize=64)
def _want(shape, index, sign, quant):
    r = rows(shape)[index]
    out, m = O.compose3_raw(r['fa'], r['ma'], r['fb'], r['mb'], sign, quant)
    m = m.astype(np.uint8)
    out.flags.writeable = m.flags.writeable = False
    return out, m


def want(shape, index, sign, quant):
    """O.compose3_raw of row `index` of rows(shape): (out float32 [H, W, 2], mask uint8 [H, W]), computed once"""
    return _want(shape, index, sign, quant)


def observed(r, sign, quant):
    """Words 0/1 as the fused launch can observe them: [non-zero, >= th] over the FINITE masked vectors of fa that some pixel
    gathers as its top-left tap (ofl.h: "set when a gathered, masked vector of fa is ...").  These the launch must set; a NaN
    tap may set them too, and nothing may set a word whose oracle predicate (expect_a) is false."""
    H, W = r['shape']
    ix, iy = N.taps(r['fb'], sign, quant)
    ok = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    t = np.zeros((H, W), bool)
    t[iy[ok], ix[ok]] = True
    v = r['fa'][t & (r['ma'] != 0)]
    v = np.abs(v[np.isfinite(v).all(-1)])
    return [bool((v > 0).any()), bool((v >= TH).any())]


# ------------------------------------------------------------------------------------------------- consumers: combine_with(mode=3)
PARTNER = 0.3                                    # the finite partner: a constant field, all valid


def consumer_rows(shape):
    """the 'fb' rows whose field serves as one operand of combine_with: (index in rows(shape), row)"""
    return [(i, r) for i, r in enumerate(rows(shape)) if r['kind'] == 'fb' and r['placement'] in CONSUMER_PLACEMENTS]


def partner(shape):
    return np.full(shape + (2,), PARTNER, 'f')


@functools.lru_cache(maxsize=None)
def oracle_combine(shape, index, ref, thresholded, operand_first):
    """O.OFlow.combine_with(mode=3) of (operand, partner) or (partner, operand) -> ('self' | 'flow', None, None) on an early
    exit (the operand the oracle hands back), else ('computed', vecs, mask bool); computed once"""
    r = rows(shape)[index]
    op, pa = O.OFlow(r['fb'], ref, r['mb'].astype(bool)), O.OFlow(partner(shape), ref)
    a, b = (op, pa) if operand_first else (pa, op)
    with np.errstate(all='ignore'):
        res = a.combine_with(b, 3, thresholded)
    if res is a:
        return 'self', None, None
    if res is b:
        return 'flow', None, None
    v, m = np.ascontiguousarray(res.vecs, F32), np.ascontiguousarray(res.mask, bool)
    v.flags.writeable = m.flags.writeable = False
    return 'computed', v, m
