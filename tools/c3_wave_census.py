#!/usr/bin/env python
"""Which of its three paths does each wave of compose3_xpose_kernel take on bench.py's sampling patterns?

    python tools/c3_wave_census.py [--height H] [--width W] [--variant V] [--ref t|s]

CPU only (NumPy; no device, no oracle).  The fields are those of bench.py::make_pair (host Flow.from_transforms); the
kernel's rules are restated here, each next to the name it has in oflibnumpy_amd/csrc/ofl_compose3.hip:

  c3_pos       position = float32(x -/+ u), one float32 operation
  c3_tap       QUANT_OPENCV: top-left tap = rint(32 p) >> 5
  c3_classify  inside:  ix in [0, W - 2] and iy in [0, H - 2];  outside: ix < -1 or ix >= W or iy < -1 or iy >= H
  c3_tile      a wave is tile rows (2 k, 2 k + 1) x 128 px of a 128 x 8 tile: all outside -> nothing fetched, else all
               inside -> interior gather, else border; H < 2 is never inside; pixels beyond the field count as both
  kernel body  a tile whose first row's vertical flow differs by more than kXposeRows = 6 rows per 128 px between its
               two ends takes the transposed layout (c3_sample_block): a wave is then 32 px x 8 rows

Printed per pattern and layout: waves, and the inside / outside / border shares of them.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILE_W, TILE_H, XPOSE_ROWS = 128, 8, 6      # kC3TileW, kC3TileH, kXposeRows


def make_sampling_field(h, w, ref, variant, pattern):
    """(fb, sign): the field bench.py streams and samples with, and the sign of its positions (ref 't': x - u)"""
    from oflibnumpy_amd.utils import from_transforms
    rot = [['rotation', w / 2.0, h / 2.0, -30.0 + 0.5 * variant]]
    f2 = [['scaling', w * 400.0 / 1920.0, h * 300.0 / 1080.0, 0.8 + 0.005 * variant]]
    if pattern == "shift":
        f2 = [['translation', 3.3 + 0.1 * variant, -2.7]]
    f1, f2 = (f2, rot) if pattern == "rot" else (rot, f2)
    return (from_transforms(f2, [h, w], ref), -1) if ref == 't' else (from_transforms(f1, [h, w], ref), +1)


def taps(p):
    """c3_tap<QUANT_OPENCV> of float32 positions"""
    return np.rint(p * np.float32(32.0)).astype(np.int64) >> 5


def census(fb, sign):
    """-> {layout: (waves, inside, outside, border)} for the sampling field fb [H][W][2] float32"""
    H, W = fb.shape[:2]
    ty_n, tx_n = -(-H // TILE_H), -(-W // TILE_W)
    hp, wp = ty_n * TILE_H, tx_n * TILE_W
    f = np.zeros((hp, wp, 2), np.float32)
    f[:H, :W] = fb
    xx = np.arange(wp, dtype=np.float32)[None, :]
    yy = np.arange(hp, dtype=np.float32)[:, None]
    ix = taps(xx + f[..., 0] if sign >= 0 else xx - f[..., 0])
    iy = taps(yy + f[..., 1] if sign >= 0 else yy - f[..., 1])
    act = (np.arange(hp)[:, None] < H) & (np.arange(wp)[None, :] < W)
    in_j = (ix >= 0) & (ix <= W - 2) & (iy >= 0) & (iy <= H - 2) & (H >= 2)
    out_j = (ix < -1) | (ix >= W) | (iy < -1) | (iy >= H)
    in_j, out_j = in_j | ~act, out_j | ~act

    # the kernel body's choice of layout, per tile
    x0 = np.arange(tx_n) * TILE_W
    x1 = np.minimum(x0 + TILE_W - 1, W - 1)
    rows = np.minimum(np.arange(ty_n) * TILE_H, H - 1)
    dv = np.abs(fb[rows][:, x1, 1] - fb[rows][:, x0, 1]).astype(np.float32)
    rotated = dv * np.float32(128.0) > (XPOSE_ROWS * (x1 - x0 + 1)).astype(np.float32)[None, :]      # (ty, tx)

    def stream(a):      # (ty, tx, wave): tile rows (2 k, 2 k + 1) x 128 px
        return a.reshape(ty_n, 4, 2, tx_n, TILE_W).all(axis=(2, 4)).transpose(0, 2, 1)

    def block(a):       # (ty, tx, wave): columns [32 k, 32 k + 32) x 8 rows
        return a.reshape(ty_n, TILE_H, tx_n, 4, 32).all(axis=(1, 4))

    res = {}
    for name, red, sel in (("streaming", stream, ~rotated), ("transposed", block, rotated)):
        outside = red(out_j)
        inside = red(in_j) & ~outside
        sel3 = np.broadcast_to(sel[..., None], outside.shape)
        n = int(sel3.sum())
        res[name] = (n, int((inside & sel3).sum()), int((outside & sel3).sum()), int((~inside & ~outside & sel3).sum()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--variant", type=int, default=0, help="bench.py rotates over variants 0 .. 3 of every pair")
    ap.add_argument("--ref", default="t", choices=["t", "s"])
    args = ap.parse_args()
    h, w = args.height, args.width
    print("# compose3_xpose_kernel<QUANT_OPENCV>: waves per {} x {} field by path (bench.py::make_pair, ref '{}', variant {})".format(
        h, w, args.ref, args.variant))
    print("# {:<8}{:<12}{:>8}{:>10}{:>10}{:>10}".format("pattern", "layout", "waves", "inside", "outside", "border"))
    for pattern in ("scale", "shift", "rot"):
        fb, sign = make_sampling_field(h, w, args.ref, args.variant, pattern)
        res = census(fb, sign)
        total = sum(r[0] for r in res.values())
        for layout, (n, a, b, c) in res.items():
            if n:
                print("  {:<8}{:<12}{:>8}{:>9.2f}%{:>9.2f}%{:>9.2f}%".format(pattern, layout, n, 100.0 * a / n, 100.0 * b / n, 100.0 * c / n))
        print("  {:<8}{:<12}{:>8}{:>9.2f}%{:>9.2f}%{:>9.2f}%".format(
            pattern, "all", total, *(100.0 * sum(r[i] for r in res.values()) / total for i in (1, 2, 3))))


if __name__ == "__main__":
    main()
