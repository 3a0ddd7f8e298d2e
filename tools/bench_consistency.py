#!/usr/bin/env python
"""The forward-backward check (K13, ofl_consistency.hip) against the fused compose kernel on the very same buffers, one JSON
line per variant: 2160 x 3840 with 8 pairs per launch (the headline shape) and 1080 x 1920 with 16.

In ONE process and INTERLEAVED -- every repeat times one launch of each variant, each launch between two HIP events -- over
rotating working sets of at least 3 x 256 MiB (bench_ops.n_sets: no launch finds its bytes in the Infinity Cache):

  consistency_masks       ofl_consistency_dev writing consistent + covered         (8 + 8 + 2 read, 2 written: 20 B/px)
  consistency_residual    the same with the float32 residual                         (24 B/px)
  consistency_masks_odd   masks only on the same buffers read as fields one column narrower: an odd width, which takes the
                          one-pixel-per-lane path (1-byte mask stores) where the even width takes two pixels per lane
  compose3                ofl_compose3_dev with fa = b, fb = f, no flag words         (18 read, 9 written: 27 B/px)
  copy_20Bpx              ofl_copy_dev moving 20 B/px (10 read, 10 written)

The fields are approximate-inverse pairs: a smooth forward field of about 5 px (a 5 x 5 lattice of normal draws, bilinearly
upsampled), its inverse by one sampling step plus a smooth disturbance of about 0.8 px, and a hole in each mask -- the
generator of tests/consistency_ref.py at full size, a different seed per pair.  Every line carries the median, the smallest
and the largest of its repeats; `over_compose3` is median over median, and `compose3_spread` = (max - min) / median of the
compose kernel's own repeats in this run, the margin below which a difference says nothing on a shared machine.

    python tools/bench_consistency.py [--repeats 16] [--out profiles/r12_consistency_bench.jsonl]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np
import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from bench_ops import n_sets
import bench_kit as kit

nat = of.native
ALPHA, BETA = np.float32(0.01), np.float32(0.5)


def smooth(rng, h, w, amp):
    """a 5 x 5 lattice of standard_normal * amp draws, bilinearly upsampled to (h, w, 2), float32"""
    lat = (rng.standard_normal((5, 5, 2)) * amp).astype(np.float32)
    ys, xs = np.linspace(0, 4, h, dtype=np.float32), np.linspace(0, 4, w, dtype=np.float32)
    y0, x0 = np.minimum(ys.astype(int), 3), np.minimum(xs.astype(int), 3)
    ty, tx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    rows = lat[:, x0] * (1 - tx) + lat[:, x0 + 1] * tx            # (5, w, 2)
    return np.ascontiguousarray(rows[y0] * (1 - ty) + rows[y0 + 1] * ty, np.float32)


def upload_pairs(h, w, n, seed, f, fm, b, bm):
    """n generated pairs, reference 't' (sign -1), into the four buffers back to back"""
    lib, px = nat.load(), h * w
    m_f, m_b = np.ones((h, w), np.uint8), np.ones((h, w), np.uint8)
    m_f[h // 4:h // 2, w // 8:w // 3] = 0
    m_b[h // 2:3 * h // 4, w // 2:3 * w // 4] = 0
    for i in range(n):
        rng = np.random.default_rng(seed + i)
        fv = smooth(rng, h, w, 5.0)
        fwd = dev.DeviceFlow.from_host(fv, 't')
        # the approximate inverse: b(y) = -f(y + f(y)), one sampling step on the device
        back, _ = dev.gather_bilinear(dev.DeviceImage(fwd.vecs, (h, w, 2), np.float32), fwd.vecs, (h, w), +1, quant=nat.QUANT_EXACT)
        bv = -back.to_host() + smooth(rng, h, w, 0.8)
        for buf, arr, step in ((f, fv, px * 8), (b, np.ascontiguousarray(bv, np.float32), px * 8), (fm, m_f, px), (bm, m_b, px)):
            nat.check(lib.ofl_upload(buf.ptr + i * step, arr.ctypes.data, step, None))
            nat.check(lib.ofl_stream_sync(None))


def main():
    a, lib, timer, report = kit.start(16)
    for name, h, w, n in (("4k_x8", 2160, 3840, 8), ("1080p_x16", 1080, 1920, 16)):
        px = n * h * w
        k = n_sets(20 * px)
        sets = []
        for s in range(k):
            bufs = {"f": dev.DeviceBuffer(px * 8), "b": dev.DeviceBuffer(px * 8), "fm": dev.DeviceBuffer(px), "bm": dev.DeviceBuffer(px),
                    "con": dev.DeviceBuffer(px), "cov": dev.DeviceBuffer(px), "res": dev.DeviceBuffer(px * 4),
                    "out": dev.DeviceBuffer(px * 8), "mout": dev.DeviceBuffer(px), "c0": dev.DeviceBuffer(px * 10), "c1": dev.DeviceBuffer(px * 10)}
            upload_pairs(h, w, n, 1000 * s + 1, bufs["f"], bufs["fm"], bufs["b"], bufs["bm"])
            nat.check(lib.ofl_memset(bufs["c0"].ptr, 1, px * 10, None))
            sets.append(bufs)

        def consistency(q, width, residual):
            return lambda: nat.check(lib.ofl_consistency_dev(q["f"].ptr, q["fm"].ptr, q["b"].ptr, q["bm"].ptr, -1, h, width, n, ALPHA, BETA,
                                                             q["con"].ptr, q["cov"].ptr, q["res"].ptr if residual else None, None,
                                                             nat.QUANT_OPENCV, None))

        variants = [
            ("consistency_masks", 20, lambda q: consistency(q, w, False)),
            ("consistency_residual", 24, lambda q: consistency(q, w, True)),
            ("consistency_masks_odd", 20, lambda q: consistency(q, w - 1, False)),
            ("compose3", 27, lambda q: (lambda: nat.check(lib.ofl_compose3_dev(q["b"].ptr, q["bm"].ptr, q["f"].ptr, q["fm"].ptr, -1, h, w, n,
                                                                               q["out"].ptr, q["mout"].ptr, None, nat.QUANT_OPENCV, None)))),
            ("copy_20Bpx", 20, kit.copy_variant(px * 10)),
        ]
        ms = kit.interleaved(timer, [(key, make) for key, _, make in variants], sets, a.repeats)
        # the kernel's covered mask is the compose kernel's, also at this size
        q = sets[(a.repeats - 1) % k]
        consistency(q, w, False)()
        same = bool(np.array_equal(q["cov"].to_host((px,), np.uint8), q["mout"].to_host((px,), np.uint8)))
        med, spread = kit.median_ms(ms), kit.spread(ms["compose3"])
        for key, bpp, _ in variants:
            width = w - 1 if key.endswith("_odd") else w
            moved = bpp * n * h * width
            report.line({
                "key": "%s_%s" % (key, name), "shape": [h, width], "pairs": n, "bytes_per_px": bpp, "bytes_moved": int(moved),
                **kit.ms_fields(ms[key]),
                "GBps": round(moved / med[key] / 1e6, 1), "repeats": a.repeats, "rotating_sets": k,
                "over_compose3": round(med[key] / med["compose3"], 3), "compose3_spread": round(spread, 3),
                "covered_equals_compose3_mask": same, "device": nat.device_name()})
        del sets, q
        dev.empty_cache()
    report.write(a.out)


if __name__ == "__main__":
    main()
