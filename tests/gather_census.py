"""Which branch of the image-gather kernels (K1, oflibnumpy_amd/csrc/ofl_gather.hip) does each wave of a launch take?

Pure NumPy: neither the product nor the oracle is imported.  The wave-uniform predicates of `gather2_kernel` /
`gather2_core` and the routing of `launch_gather_t` are restated here, so that a test case can PROVE which branch it
reaches before it is compared with the oracle (tests/gather_cases.py, tests/test_gather_census_host.py,
tests/test_gpu_gather_paths.py).  Every rule that depends on a constant of the kernel names it in a comment; a change to
the kernel shows where to follow.

Class tokens of a wave of the paired kernel (a wave with no active pixel is not counted):

  flow:whole | flow:aligned | flow:single | flow:none
        how the wave loads its flow vectors: the `__all(whole)` path / predicated 16-byte pairs / predicated single
        vectors (odd pad_left or odd fW) / no lane inside the flow area
  flow:straddle     a lane's pixel pair has exactly one pixel inside the flow area (with flow:single only)
  rot | norot       float32 with 3 or 4 channels only: the tile's transposed (block) form or the streaming one
  outside | inside | border
        gather2_core's three paths
  h1                H < 2, which forces `inside = false`
  wide | narrow     `inside` waves of the padded run types (6- and 12-byte runs): px_load<WIDE = true / false>
  px | px1          `inside` waves: the two-phase px_load / px_blend form, or float64's one-pixel-at-a-time gather_px<INSIDE>
  group4 | group2   px waves: pixels in flight together (kGroup)
  sep | fix4 | flt  uint8 `inside` waves: the separable fixed-point blend (cv2's snap), the four-tap fixed-point form (un-snapped
                    weights), or the float blend rounded half to even (ARITH_FLOAT_RNE)
  img:joined | img:pair     2- and 6-byte pixel pairs (uint8 with 1 or 3 channels): the store joined across lanes or per pair
  img:own           every other type: each lane stores its own pair
  val:joined | val:pair     the validity store, when validity is asked for
  band              an output band [row0, row0 + rows) that is not the whole frame
  band:odd          ... whose first row is no multiple of the tile's 8 rows
  offset            the flow area does not start at the frame's first pixel (pad_top or pad_left is not 0)
"""
from collections import Counter

import numpy as np

U8, I16, U16, F32, F64 = 'uint8', 'int16', 'uint16', 'float32', 'float64'
QUANT_OPENCV, QUANT_EXACT = 0, 1
ARITH_NATIVE, ARITH_FLOAT_RNE = 0, 1

TILE_W, TILE_H = 128, 8        # gather2_kernel: `tx * 128`, `ty * 8` (K2's kC3TileW / kC3TileH)
LANES_X = 32                   # lanes along x of a tile row; a wave of 64 lanes is two consecutive tile rows
XPOSE_ROWS = 6                 # kXposeRows


def route(dtype, C, H, W, fH, fW):
    """launch_gather_t: the paired kernel takes even widths, 1 - 4 channels and sizes below 4 GiB"""
    size = np.dtype(dtype).itemsize
    if W % 2 == 0 and 1 <= C <= 4 and H * W * C * size < (1 << 32) and fH * fW * 8 < (1 << 32):
        return 'paired'
    return 'general_ct' if C <= 4 else 'general_loop'      # gather_kernel<T, CT = C> / <T, 0>: the runtime channel loop


def _taps(p, quant):
    """top-left tap along one axis of float32 positions p (make_tap)"""
    if quant == QUANT_OPENCV:
        s = np.rint(p.astype(np.float32) * np.float32(32.0)).astype(np.float64)      # cvRound: half to even
        s = np.clip(s, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)                   # v_cvt_i32_f32 saturates
        return np.clip(s >> 5, -32768, 32767), s & 31
    f = np.clip(np.floor(p.astype(np.float32)), -32768.0, 32767.0)
    return f.astype(np.int64), np.zeros(p.shape, np.int64)


def positions(flow, H, W, pad_top, pad_left, sign, row0, rows, hp, wp):
    """float32 sample positions of the band's pixels on a grid padded to whole tiles, and where the flow area is:
    float32(float64(grid) +- float64(flow)), zero flow outside the flow area (utils.py:231-235, Flow.pad 'constant')"""
    fH, fW = flow.shape[:2]
    yy, xx = np.mgrid[0:hp, 0:wp]
    gy = yy + row0
    act = (yy < rows) & (xx < W)
    inflow = act & (gy - pad_top >= 0) & (gy - pad_top < fH) & (xx - pad_left >= 0) & (xx - pad_left < fW)
    f = np.zeros((hp, wp, 2), np.float32)
    f[inflow] = flow[(gy - pad_top)[inflow], (xx - pad_left)[inflow]]
    fd = f.astype(np.float64)
    px = (xx + fd[..., 0] if sign >= 0 else xx - fd[..., 0]).astype(np.float32)
    py = (gy + fd[..., 1] if sign >= 0 else gy - fd[..., 1]).astype(np.float32)
    return px, py, act, inflow, f


def census(dtype, C, H, W, flow, pad_top=0, pad_left=0, sign=-1, quant=QUANT_OPENCV, arith=ARITH_NATIVE,
           row0=0, rows=None, smask=False, fmask=False, valid=False):
    """-> (route, Counter of class token -> waves, Counter of frozenset of tokens -> waves)"""
    dtype = np.dtype(dtype).name
    size = np.dtype(dtype).itemsize
    rows = H if rows is None else rows
    flow = np.asarray(flow, np.float32)
    fH, fW = flow.shape[:2]
    r = route(dtype, C, H, W, fH, fW)
    if r != 'paired':
        return r, Counter(), Counter()
    tiles_x, tiles_y = -(-W // TILE_W), -(-rows // TILE_H)
    hp, wp = tiles_y * TILE_H, tiles_x * TILE_W
    px, py, act, inflow, f = positions(flow, H, W, pad_top, pad_left, sign, row0, rows, hp, wp)
    ix, _ = _taps(px, quant)
    iy, _ = _taps(py, quant)
    in_j = (ix >= 0) & (ix <= W - 2) & (iy >= 0) & (iy <= H - 2)
    out_j = (ix < -1) | (ix >= W) | (iy < -1) | (iy >= H)
    if H < 2:
        in_j[...] = False
    # padded run types: 6- and 12-byte runs (kRB = 2 * CT * sizeof(T)) may be read as 8 / 16 bytes unless they end at the image's end
    krb = 2 * C * size
    padded = size <= 2 and krb in (6, 12)
    wide_j = ((iy + 1) * W + ix) * (C * size) + krb + krb // 3 <= H * W * C * size

    # ---- flow load: always in the streaming layout (a wave = tile rows 2w, 2w + 1; a lane = pixels 2 lx, +1, +64, +65)
    aligned = ((pad_left | fW) & 1) == 0
    def stream(a, how):                      # (hp, wp) -> (tiles_y, 4, tiles_x) over a wave's 2 rows x 128 px
        return how(a.reshape(tiles_y, 4, 2, tiles_x, TILE_W), axis=(2, 4))
    w_act = stream(act, np.any)
    w_whole = aligned & stream(act & inflow, np.all)
    w_anyflow = stream(inflow, np.any)
    pair = inflow.reshape(hp, wp // 2, 2)
    w_straddle = stream(np.repeat(pair[..., 0] != pair[..., 1], 2, axis=1), np.any)

    # ---- transposed form: float32 with 3 or 4 channels (kXp), decided per tile from the first row's two end vectors
    rot_tile = np.zeros((tiles_y, tiles_x), bool)
    if dtype == F32 and C >= 3:
        for ty in range(tiles_y):
            for tx in range(tiles_x):
                x0 = tx * TILE_W
                x1 = min(x0 + TILE_W - 1, W - 1)
                yl = min(ty * TILE_H, rows - 1)
                va, vb = f[yl, x0, 1], f[yl, x1, 1]      # (zero outside the flow area, as the kernel reads it)
                rot_tile[ty, tx] = np.float32(abs(np.float32(vb - va))) * np.float32(128.0) > np.float32(XPOSE_ROWS * (x1 - x0 + 1))

    def block(a, how):                       # wave w of a tile = columns [32 w, 32 w + 32) of its 8 rows -> (tiles_y, tiles_x, 4)
        return how(a.reshape(tiles_y, TILE_H, tiles_x, 4, LANES_X), axis=(1, 4))

    def paths(red):
        any_act = red(act, np.any)
        all_out = red(out_j | ~act, np.all)
        all_in = ~all_out & red(in_j | ~act, np.all)
        all_wide = red(wide_j | ~act, np.all)
        return any_act, all_out, all_in, all_wide
    s_paths = [np.transpose(a, (0, 2, 1)) for a in paths(stream)]      # -> (tiles_y, tiles_x, 4)
    b_paths = paths(block)

    img_store = ('img:joined' if W % 4 == 0 else 'img:pair') if (size == 1 and C in (1, 3)) else 'img:own'      # kPB == 2 || kPB == 6
    val_store = None if not valid else ('val:joined' if W % 4 == 0 else 'val:pair')
    band = (row0, rows) != (0, H)
    sep = dtype == U8 and arith == ARITH_NATIVE and quant == QUANT_OPENCV

    tokens, combos = Counter(), Counter()
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            for w in range(4):
                if not w_act[ty, w, tx]:
                    continue
                t = set()
                # (in the transposed form the flow is loaded in the streaming layout and handed over through LDS: the flow class
                # of streaming wave w and the path class of block wave w are two facts about the same 64 lanes)
                if w_whole[ty, w, tx]:
                    t.add('flow:whole')
                elif not w_anyflow[ty, w, tx]:
                    t.add('flow:none')
                else:
                    t.add('flow:aligned' if aligned else 'flow:single')
                    if w_straddle[ty, w, tx]:
                        t.add('flow:straddle')
                rot = bool(rot_tile[ty, tx])
                if dtype == F32 and C >= 3:
                    t.add('rot' if rot else 'norot')
                any_act, all_out, all_in, all_wide = [a[ty, tx, w] for a in (b_paths if rot else s_paths)]
                if not any_act:              # (a block wave past a ragged tile's last column: every lane idle)
                    t.add('idle')
                elif all_out:
                    t.add('outside')
                elif all_in:
                    t.add('inside')
                    if size == 8:
                        t.add('px1')
                    else:
                        t.add('px')
                        t.add('group2' if (size == 4 and C >= 3) else 'group4')      # PxRun: runs for 8- / 16-bit and float C <= 2
                        if padded:
                            t.add('wide' if all_wide else 'narrow')
                        if dtype == U8:
                            t.add('sep' if sep else ('fix4' if arith == ARITH_NATIVE else 'flt'))
                else:
                    t.add('border')
                if H < 2:
                    t.add('h1')
                t.add(img_store)
                if val_store:
                    t.add(val_store)
                    t.add('smask' if smask else 'nosmask')
                    if fmask:
                        t.add('fmask')
                if band:
                    t.add('band')
                    if row0 % TILE_H:
                        t.add('band:odd')
                if pad_top or pad_left:
                    t.add('offset')
                tokens.update(t)
                combos[frozenset(t)] += 1
    return r, tokens, combos


def summary(tokens):
    """a short, stable label of a census for test ids"""
    order = ['flow:whole', 'flow:aligned', 'flow:single', 'rot', 'norot', 'outside', 'inside', 'border', 'narrow', 'px1',
             'h1', 'img:joined', 'img:pair', 'val:joined', 'val:pair', 'band']
    return '+'.join(k.replace('flow:', '').replace(':', '_') for k in order if tokens.get(k))
