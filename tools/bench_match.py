#!/usr/bin/env python
"""Global matching (K19, ofl_match.hip), one JSON line per variant: DeviceCorrelation.match for feature maps (C, H, W) =
(128, 136, 240) (1/8 of 1080p) and (128, 68, 120) in float16, bfloat16 and float32, each with 1 and with 8 items, and
(256, 68, 120) in float16.

In ONE process and INTERLEAVED -- every repeat times one call of each variant, each call between two HIP events -- over 2
rotating working sets:

  match         random normal features at the default scale: logits of unit spread, no key tile is skipped
  match_peaked  (float16, 1 item) f2 = f1 rolled by (5, 3) at scale 2: one sharp maximum per query, every other tile skipped
  copy          ofl_copy_dev: the yardstick

No time is fixed in advance.  Every line carries the median, the smallest and the largest of its repeats.  A match line says
  flop            2 sweeps x 2 N (H W)^2 C
  TFLOPs, share   that rate, and its share of the data sheet's 2.5 PFLOP/s (16-bit) or 157.3 TFLOP/s (float32) matrix peak
  volume_GB       the N (H W)^2 float32 volume the textbook route writes and reads
  volume_copy_ms  one write and one read of that volume at this run's copy rate: the copy moves `copy_bytes` (as many as
                  2 GiB; `copy_scaled` says whether the time was scaled up linearly from it) -- what f1 @ f2^T then softmax
                  cannot avoid, before any arithmetic
  over_volume_copy  the match's time over that
  max_dev_px      at the workload size: the largest deviation of 256 sampled queries of item 0 from the float64 definition,
                  with `bound_px`, tests/match_ref.bound for this shape

    python tools/bench_match.py [--repeats 8] [--out profiles/r18_match_bench.jsonl]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import numpy as np
import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
import bench_kit as kit
import interop_ref as R
import match_ref as M

nat = of.native
SETS = 2
PEAK = {"float16": 2.5e15, "bfloat16": 2.5e15, "float32": 157.3e12}
COPY_CAP = 2 << 30
SAMPLES = 256


def sampled_deviation(f1, f2, dt, scale, vecs, h, w):
    """the largest |device - float64 definition| over SAMPLES queries, in pixels, and the derived bound"""
    a, b = M.widen(f1, dt).reshape(h * w, -1).astype(np.float64), M.widen(f2, dt).reshape(h * w, -1).astype(np.float64)
    q = np.random.default_rng(5).choice(h * w, SAMPLES, replace=False)
    s = (a[q] @ b.T) * np.float64(scale)
    e = np.exp(s - s.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    ky, kx = np.divmod(np.arange(h * w), w)
    want = np.stack([p @ kx.astype(np.float64) - kx[q], p @ ky.astype(np.float64) - ky[q]], -1)
    mag = float((np.abs(a[q]) @ np.abs(b).T).max())
    return float(np.abs(vecs.reshape(h * w, 2)[q].astype(np.float64) - want).max()), float(M.bound(a.shape[1], h, w, scale, mag))


def main():
    a, lib, timer, report = kit.start(8)
    shapes = [(128, 136, 240, dt, n) for dt in ("float16", "bfloat16", "float32") for n in (1, 8)]
    shapes += [(128, 68, 120, dt, n) for dt in ("float16", "bfloat16", "float32") for n in (1, 8)]
    shapes += [(256, 68, 120, "float16", 1)]
    for c, h, w, dt, n in shapes:
        px = h * w
        volume = n * px * px * 4
        copy_bytes = min(volume, COPY_CAP)
        peaked = dt == "float16" and n == 1
        sets, first = [], None
        for s in range(SETS):
            rng = np.random.default_rng(400 + s)
            f1 = np.ascontiguousarray(R.from_f32(rng.standard_normal((h, w, c), np.float32), dt))
            f2 = np.ascontiguousarray(R.from_f32(rng.standard_normal((h, w, c), np.float32), dt))
            q = {"corr": of.DeviceCorrelation(kit.replicate(dev.DeviceBuffer(n * f1.nbytes), f1, n), dt,
                                              [(kit.replicate(dev.DeviceBuffer(n * f2.nbytes), f2, n), dt)], n, c, h, w, True)}
            if peaked:
                rolled = np.ascontiguousarray(np.roll(f1, (3, 5), (0, 1)))
                q["peak"] = of.DeviceCorrelation(q["corr"].f1, dt, [(dev.DeviceBuffer.from_host(rolled), dt)], n, c, h, w, True)
            q["c0"], q["c1"] = dev.DeviceBuffer(copy_bytes), dev.DeviceBuffer(copy_bytes)
            nat.check(lib.ofl_memset(q["c0"].ptr, 1, copy_bytes, None))
            first = first or (f1, f2)
            sets.append(q)
        variants = [("match", lambda q: (lambda: q["corr"].match()))]
        if peaked:
            variants.append(("match_peaked", lambda q: (lambda: q["peak"].match(scale=2.0))))
        variants.append(("copy", kit.copy_variant(copy_bytes)))
        ms = kit.interleaved(timer, variants, sets, a.repeats)
        med = kit.median_ms(ms)
        flop = 2.0 * 2.0 * n * float(px) * px * c
        volume_copy_ms = med["copy"] * (volume / copy_bytes)
        check = {}
        if (h, w) == (136, 240):
            vecs = sets[0]["corr"].match().vecs.to_host((n, h, w, 2), np.float32)[0]
            dev_px, bound_px = sampled_deviation(first[0], first[1], dt, M.default_scale(c), vecs, h, w)
            check = {"sampled_queries": SAMPLES, "max_dev_px": float("%.3e" % dev_px), "bound_px": float("%.3e" % bound_px)}
        for key, _ in variants:
            line = {"key": "%s_%s_c%d_%dx%d_x%d" % (key, dt, c, h, w, n), "features": [c, h, w], "dtype": dt, "items": n,
                    **kit.ms_fields(ms[key]), "repeats": a.repeats, "rotating_sets": SETS, "device": nat.device_name()}
            if key == "copy":
                line.update({"copy_bytes": copy_bytes, "bytes_moved": 2 * copy_bytes,
                             "TBps": round(2 * copy_bytes / (med[key] * 1e-3) / 1e12, 3), "copy_spread": round(kit.spread(ms[key]), 3)})
            else:
                t = med[key] * 1e-3
                line.update({"flop": flop, "TFLOPs": round(flop / t / 1e12, 2), "share_of_matrix_peak": round(flop / t / PEAK[dt], 4),
                             "volume_GB": round(volume / 1e9, 2), "volume_copy_ms": round(volume_copy_ms, 3),
                             "copy_scaled": volume != copy_bytes, "over_volume_copy": round(med[key] / volume_copy_ms, 3)})
                if key == "match":
                    line.update(check)
            report.line(line)
        del sets, q
        dev.empty_cache()
    report.write(a.out)


if __name__ == "__main__":
    main()
