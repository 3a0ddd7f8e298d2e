"""The case table of the image-gather kernels' path tests (tests/test_gather_census_host.py proves on the CPU which branches
each case reaches, tests/test_gpu_gather_paths.py compares the kernels with the oracle on them).

A case is a seeded builder: `build(case)` returns the arrays, `case` itself holds the arguments of the C entry.  The table is
built pairwise, not as a full product: every (type, channels) group walks the same list of (shape, flow kind, flow placement)
and cycles through arithmetic modes, signs and mask combinations with strides that differ per group."""
import zlib

import numpy as np

import gather_census as gc

DTYPES = [gc.U8, gc.I16, gc.U16, gc.F32, gc.F64]
EQ1, GE_HALF, GT_HALF = 0, 1, 2

# (name, quant, arith, rule): uint8 walks the three rows of the DESIGN 3.2 table (fixed point without / with `>= 1/2`, the int16
# concat's float sum rounded half to even with `> 1/2`) and the un-snapped weights; 'fold' marks a folded instantiation
MODES = {
    gc.U8:  [('fix_ge.fold', 0, 0, GE_HALF), ('rne_gt.fold', 0, 1, GT_HALF), ('fix_eq', 0, 0, EQ1), ('exact_ge', 1, 0, GE_HALF),
             ('exact_rne', 1, 1, GT_HALF)],
    gc.I16: [('gt', 0, 0, GT_HALF), ('exact_eq', 1, 0, EQ1)],
    gc.U16: [('gt', 0, 0, GT_HALF), ('exact_ge', 1, 0, GE_HALF)],
    gc.F32: [('eq.fold', 0, 0, EQ1), ('ge', 0, 0, GE_HALF), ('exact_eq', 1, 0, EQ1)],
    gc.F64: [('eq', 0, 0, EQ1), ('exact_gt', 1, 0, GT_HALF)],
}
# (source mask, flow mask, validity)
MASKS = [(False, False, False), (False, False, True), (True, False, True), (False, True, True), (True, True, True)]

# (shape, flow kind, flow placement): 'frame' = the whole frame, 'even' = (3, 2, H - 5, W - 4), 'odd' = (3, 3, H - 5, W - 5)
WALK = [
    ((24, 256), 'shift', 'frame'),       # whole waves, all inside, un-rotated, joined stores
    ((24, 256), 'corner', 'frame'),      # an all-inside wave whose runs end at the image's end
    ((24, 256), 'outside', 'frame'),
    ((24, 256), 'ties', 'even'),
    ((24, 256), 'random', 'odd'),
    ((24, 256), 'shift', 'odd'),
    ((19, 258), 'shift', 'even'),        # W % 4 == 2: per-pair stores, a ragged third tile, ragged rows
    ((19, 258), 'corner', 'frame'),
    ((19, 258), 'outside', 'frame'),
    ((19, 258), 'random', 'odd'),
    ((19, 258), 'ties', 'frame'),
    ((1, 256), 'shift', 'frame'),        # H < 2
    ((1, 256), 'random', 'even1'),
    ((1, 256), 'outside', 'frame'),
    ((2, 128), 'corner', 'frame'),       # the smallest H that can be inside
    ((2, 128), 'random', 'frame'),
    ((17, 129), 'random', 'odd'),        # odd width: the general kernel
    ((17, 129), 'ties', 'frame'),
    ((40, 384), 'shear', 'frame'),       # the transposed form for float32 with 3 / 4 channels
    ((40, 384), 'shear', 'even'),
    ((40, 384), 'shear', 'odd'),
]


def placement(name, H, W):
    if name == 'frame':
        return 0, 0, H, W
    if name == 'even':
        return 3, 2, H - 5, W - 4
    if name == 'even1':                  # (a one-row frame has no room for rows of padding)
        return 0, 2, H, W - 4
    if name == 'odd':
        return 3, 3, H - 5, W - 5
    raise ValueError(name)


def _case(entry, dtype, C, shape, kind, place, mode, sign, masks, **extra):
    H, W = shape
    name, quant, arith, rule = mode
    top, left, fH, fW = placement(place, H, W)
    c = dict(entry=entry, dtype=dtype, C=C, H=H, W=W, kind=kind, place=place, pad_top=top, pad_left=left, fH=fH, fW=fW,
             mode=name, quant=quant, arith=arith, rule=rule, sign=sign, smask=masks[0], fmask=masks[1], valid=masks[2],
             row0=0, rows=H, batch=1, shared=False)
    c.update(extra)
    c['id'] = '{}-{}c{}-{}x{}-{}-{}-{}-s{}-m{}{}{}'.format(entry, dtype, C, H, W, kind, place, name.split('.')[0],
                                                           'p' if sign > 0 else 'n', *[int(m) for m in masks])
    if entry == 'rows':
        c['id'] += '-r{}+{}'.format(c['row0'], c['rows'])
    if entry == 'batch':
        c['id'] += '-shared' if c['shared'] else '-own'
    return c


def _table():
    cases = []
    for ti, dtype in enumerate(DTYPES):
        modes = MODES[dtype]
        for C in (1, 2, 3, 4):
            for i, (shape, kind, place) in enumerate(WALK):
                cases.append(_case('single', dtype, C, shape, kind, place, modes[(i + C) % len(modes)],
                                   (-1, 1)[(i + C + ti) % 2], MASKS[(i + 2 * C + ti) % len(MASKS)]))
        # six channels: the general kernel's runtime channel loop, even and odd width
        for i, (shape, kind, place) in enumerate([((24, 256), 'random', 'even'), ((17, 129), 'shift', 'odd'), ((19, 258), 'ties', 'frame')]):
            cases.append(_case('single', dtype, 6, shape, kind, place, modes[i % len(modes)], (-1, 1)[(i + ti) % 2],
                               MASKS[(i + ti + 2) % len(MASKS)]))
    # the separable uint8 blend and the folded float kernel on the run that ends at the image's end and on the un-rotated grid,
    # pinned by name (the walk above reaches them through its cycling; these do not depend on it)
    for dtype, C, mode in ((gc.U8, 1, 0), (gc.U8, 3, 0), (gc.U8, 3, 1), (gc.U8, 3, 3), (gc.I16, 3, 0), (gc.U16, 3, 0),
                           (gc.F32, 3, 0), (gc.F32, 4, 0), (gc.F32, 3, 1), (gc.F64, 1, 0), (gc.F64, 3, 0)):
        for shape in ((24, 256), (19, 258)):
            for kind in ('shift', 'corner'):
                cases.append(_case('single', dtype, C, shape, kind, 'frame', MODES[dtype][mode], -1, MASKS[4]))
    # the flow mask on the common wave with padding offsets and on the unaligned single loads, with per-pair stores
    for dtype in DTYPES:
        for C in (1, 2, 3, 4):
            mode = MODES[dtype][C % len(MODES[dtype])]
            cases.append(_case('single', dtype, C, (19, 258), 'shift', 'even', mode, -1, MASKS[4]))
            cases.append(_case('single', dtype, C, (19, 258), 'random', 'odd', mode, 1, MASKS[3]))
    # the folded instantiations are kernels of their own per channel count: each meets all three paths and both validity stores
    for dtype, mode in ((gc.U8, 0), (gc.U8, 1), (gc.F32, 0)):
        for C in (1, 2, 3, 4):
            cases.append(_case('single', dtype, C, (24, 256), 'outside', 'frame', MODES[dtype][mode], 1, MASKS[4]))
            cases.append(_case('single', dtype, C, (24, 256), 'shift', 'frame', MODES[dtype][mode], 1, MASKS[2]))
            cases.append(_case('single', dtype, C, (19, 258), 'random', 'frame', MODES[dtype][mode], -1, MASKS[4]))
    # the transposed form and H < 2 with per-pair stores (W % 4 == 2)
    for C in (3, 4):
        for place in ('frame', 'even'):
            cases.append(_case('single', gc.F32, C, (40, 386), 'shear', place, MODES[gc.F32][0], (-1, 1)[C % 2], MASKS[4]))
    for C in (1, 3):
        cases.append(_case('single', gc.U8, C, (1, 258), 'random', 'frame', MODES[gc.U8][0], 1, MASKS[2]))
    # row bands (ofl_gather_rows_dev): bands whose first row and height are no multiples of 8
    for dtype, C, mode in ((gc.U8, 1, 0), (gc.U8, 3, 1), (gc.I16, 3, 0), (gc.U16, 2, 0), (gc.F32, 3, 0), (gc.F32, 1, 1), (gc.F64, 2, 0)):
        for shape in ((24, 256), (19, 258), (17, 129)):
            for j, (row0, rows) in enumerate(((5, 11), (16, 3))):
                if row0 + rows > shape[0]:
                    continue
                for kind in ('shift', 'random'):
                    cases.append(_case('rows', dtype, C, shape, kind, 'frame', MODES[dtype][mode], (-1, 1)[j],
                                       MASKS[4 if kind == 'shift' else 1 + j], row0=row0, rows=rows, pad_top=row0, fH=rows))
    # batches (ofl_gather_bilinear_batch_dev): three fields, own and shared source
    for dtype, C, mode, shape, place in ((gc.U8, 1, 0, (24, 256), 'frame'), (gc.U8, 3, 1, (19, 258), 'even'), (gc.I16, 3, 0, (24, 256), 'odd'),
                                         (gc.F32, 3, 0, (40, 384), 'frame'), (gc.F32, 6, 0, (17, 129), 'odd'), (gc.F64, 1, 0, (19, 258), 'frame')):
        for shared in (False, True):
            cases.append(_case('batch', dtype, C, shape, 'mixed', place, MODES[dtype][mode], -1 if shared else 1, MASKS[4],
                               batch=3, shared=shared))
    seen, out = set(), []
    for c in cases:                      # (a pinned case may repeat one that the walk's cycling already holds)
        if c['id'] not in seen:
            seen.add(c['id'])
            out.append(c)
    return out


def _flow(kind, c, rng, field=0):
    """the flow of one field, on the flow area (fH, fW) placed at (pad_top, pad_left)"""
    H, W, fH, fW, top, left, sign = c['H'], c['W'], c['fH'], c['fW'], c['pad_top'], c['pad_left'], c['sign']
    yy, xx = np.mgrid[0:fH, 0:fW]
    gy, gx = yy + top, xx + left                               # target coordinates of the flow area's pixels
    f = np.zeros((fH, fW, 2), np.float32)
    if kind == 'mixed':
        kind = ('shift', 'random', 'shear' if (c['dtype'] == gc.F32 and c['C'] >= 3) else 'corner')[field]
    if kind == 'shift':                  # interior waves all inside, un-rotated
        f[..., 0], f[..., 1] = 1.3, 0.6
    elif kind == 'shear':                # the vertical component grows by more than kXposeRows (6) source rows over 128 px
        f[..., 0] = 0.3
        f[..., 1] = np.float32(0.08) * gx + np.float32(0.011) * gy      # (a term in y: the rows of a tile carry different vectors)
    elif kind == 'outside':
        f[...] = 3.0e4
    elif kind == 'corner':
        # every pixel of a two-row, 128-px stretch -- one wave: tile rows (0, 1) or (8, 9), the tile at x = 0 or 128 -- aimed at
        # the taps (W - 2, H - 2) plus a fraction; a constant shift elsewhere
        f[..., 0], f[..., 1] = 1.3, 0.6
        y0 = 8 if H >= 18 else 0
        x0 = 128 if W >= 256 else 0
        sel = (gy >= y0) & (gy < y0 + 2) & (gx >= x0) & (gx < x0 + 128)
        frac = rng.integers(1, 32, (fH, fW, 2)) / 32.0
        tx, ty = (W - 2) + frac[..., 0], (H - 2) + frac[..., 1]
        f[..., 0] = np.where(sel, sign * (tx - gx), f[..., 0])
        f[..., 1] = np.where(sel, sign * (ty - gy), f[..., 1])
    elif kind == 'ties':
        # positions on exact 1/2 and 1/64 steps: cvRound's ties in the 1/32-px snap, and weights of 1/2 and 1/4 that put the
        # blends of the small integers of the 'ties' image on exact .5
        step = rng.choice([0.5, 1.0 / 64.0], (fH, fW, 1))
        f[...] = rng.integers(-192, 192, (fH, fW, 2)) * step
    elif kind == 'random':               # border mix; a few vectors far beyond int16
        f[...] = rng.standard_normal((fH, fW, 2)) * 6.0
        far = rng.random((fH, fW)) < 0.01
        f[far] = rng.choice([-1.0e9, 1.0e9], (int(far.sum()), 2))
    else:
        raise ValueError(kind)
    return f


def _image(c, rng):
    H, W, C, dtype = c['H'], c['W'], c['C'], np.dtype(c['dtype'])
    if c['kind'] == 'ties':
        return rng.integers(0, 8, (H, W, C)).astype(dtype)     # sums of four of these over 2 or 4 land on .5 and .25
    if dtype.kind in 'iu':
        info = np.iinfo(dtype)
        return rng.integers(info.min, info.max, (H, W, C), endpoint=True).astype(dtype)
    return (rng.standard_normal((H, W, C)) * 100).astype(dtype)


def build(c):
    """-> dict(src [B or 1, H, W, C], flow [B, fH, fW, 2], smask [B or 1, H, W] or None, fmask [B, fH, fW] or None)"""
    rng = np.random.default_rng(zlib.crc32(c['id'].encode()))
    B = c['batch']
    nsrc = 1 if c['shared'] else B
    src = np.stack([_image(c, rng) for _ in range(nsrc)])
    flow = np.stack([_flow(c['kind'], c, rng, b) for b in range(B)])
    smask = (rng.random((nsrc, c['H'], c['W'])) > 0.15).astype(np.uint8) if c['smask'] else None
    fmask = (rng.random((B, c['fH'], c['fW'])) > 0.15).astype(np.uint8) if c['fmask'] else None
    return dict(src=src, flow=flow, smask=smask, fmask=fmask)


def expected(c, a, oracle):
    """the oracle's image [B, rows, W, C] and validity [B, rows, W] (None when not asked for) of a built case"""
    imgs, vals = [], []
    sl = slice(c['row0'], c['row0'] + c['rows'])
    for b in range(c['batch']):
        s = 0 if c['shared'] else b
        res = oracle.gather_bilinear(a['src'][s], a['flow'][b], c['sign'], smask=None if a['smask'] is None else a['smask'][s],
                                     want_valid=c['valid'], quant=c['quant'], arith=c['arith'], rule=c['rule'],
                                     pad=(c['pad_top'], c['pad_left']))
        img, val = res if c['valid'] else (res, None)
        if val is not None and a['fmask'] is not None:     # the flow mask: valid only inside the flow area and where it is set
            area = np.zeros((c['H'], c['W']), bool)
            area[c['pad_top']:c['pad_top'] + c['fH'], c['pad_left']:c['pad_left'] + c['fW']] = a['fmask'][b] != 0
            val = val & area
        imgs.append(img[sl])
        vals.append(None if val is None else val[sl].astype(np.uint8))
    return np.stack(imgs), (np.stack(vals) if c['valid'] else None)


def census_of(c, a, field=0):
    return gc.census(c['dtype'], c['C'], c['H'], c['W'], a['flow'][field], c['pad_top'], c['pad_left'], c['sign'], c['quant'],
                     c['arith'], c['row0'], c['rows'], c['smask'], c['fmask'], c['valid'])


CASES = _table()
