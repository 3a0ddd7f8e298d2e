#!/usr/bin/env python
"""Correlation lookup (K18, ofl_correlation.hip), one JSON line per variant: DeviceCorrelation.build and one lookup at
radius 4 over 4 levels -- RAFT's setting -- for feature maps (C, H, W) = (256, 136, 240) in float16 and float32 (1/8 of 1080p)
and (128, 270, 480) in float16 (1/4 of 1080p), each with 1 and with 8 items.

In ONE process and INTERLEAVED -- every repeat times one call of each variant, each call between two HIP events -- over 2
rotating working sets:

  lookup      DeviceCorrelation.lookup with one random field per item within +-8 px: 4 launches
  build_hwc   DeviceCorrelation.build from channels-last tensors: the three pooling launches
  build_chw   the same from planar tensors: two permutes more (one read and one write of each tensor)
  copy        ofl_copy_dev moving the lookup's output bytes (read once, written once)

No rate is fixed in advance.  Every line carries the median, the smallest and the largest of its repeats.  The lookup's line
also says what the definition's arithmetic and traffic amount to:
  flop            2 (2r + 2)^2 C levels operations per pixel (a product and a sum per channel and integer tap)
  share_fp32_vec  flop / time over the 157.3 TFLOP/s the data sheet gives for float32 vector arithmetic (which counts fused and
                  packed operations; the kernel's products and sums are neither, so half of it is the most it could reach)
  f2_TBps         the (2r + 2)^2 rows of C elements a pixel asks of every level, over time: requested bytes, served mostly by L2
  out_over_copy   time over the copy's; copy_spread = (max - min) / median of the copy's repeats in this run
  all_pairs_GB    what the all-pairs volume and its pooled levels would have taken in float32
`equal_restatement`: the top-left 4 x 8 pixels of the first item equal tests/correlation_ref.py byte for byte.

    python tools/bench_correlation.py [--repeats 12] [--out profiles/r17_correlation_bench.jsonl]
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
from oflibnumpy_amd.batch import DeviceFlowBatch
import bench_kit as kit
import correlation_ref as K

nat = of.native
SETS = 2
RADIUS, LEVELS = 4, 4
CROP = (4, 8)
FP32_VECTOR_PEAK = 157.3e12


def main():
    a, lib, timer, report = kit.start(12)

    def replicated(arr, n):
        """n copies of a host array back to back in one device buffer"""
        return kit.replicate(dev.DeviceBuffer(n * arr.nbytes), arr, n)

    nch = LEVELS * (2 * RADIUS + 1) ** 2
    for c, h, w, dt in ((256, 136, 240, "float16"), (256, 136, 240, "float32"), (128, 270, 480, "float16")):
        for n in (1, 8):
            e = np.dtype(dt).itemsize
            px = h * w
            out_bytes = n * nch * px * 4
            sets, first = [], None
            for s in range(SETS):
                rng = np.random.default_rng(300 + s)
                f1 = rng.standard_normal((h, w, c), np.float32).astype(dt)
                f2 = rng.standard_normal((h, w, c), np.float32).astype(dt)
                flow = ((rng.random((h, w, 2), np.float32) - np.float32(0.5)) * np.float32(16))
                q = {}
                for name, arr in (("f1", f1), ("f2", f2)):
                    q[name, "hwc"] = dev.DeviceTensor(replicated(arr, n), (n, c, h, w), dt, "hwc")
                    q[name, "chw"] = dev.DeviceTensor(replicated(np.moveaxis(arr, -1, 0), n), (n, c, h, w), dt, "chw")
                q["flow"] = DeviceFlowBatch.wrap(n, (h, w), 's', replicated(flow, n), None)
                q["corr"] = of.DeviceCorrelation.build(q["f1", "hwc"], q["f2", "hwc"], LEVELS)
                q["c0"], q["c1"] = dev.DeviceBuffer(out_bytes), dev.DeviceBuffer(out_bytes)
                nat.check(lib.ofl_memset(q["c0"].ptr, 1, out_bytes, None))
                first = first or (f1, f2, flow)
                sets.append(q)
            variants = [
                ("lookup", lambda q: (lambda: q["corr"].lookup(q["flow"], RADIUS))),
                ("build_hwc", lambda q: (lambda: of.DeviceCorrelation.build(q["f1", "hwc"], q["f2", "hwc"], LEVELS))),
                ("build_chw", lambda q: (lambda: of.DeviceCorrelation.build(q["f1", "chw"], q["f2", "chw"], LEVELS))),
                ("copy", kit.copy_variant(out_bytes)),
            ]
            ms = kit.interleaved(timer, variants, sets, a.repeats)
            f1, f2, flow = first
            got = sets[0]["corr"].lookup(sets[0]["flow"], RADIUS).to_host()[0][:, :CROP[0], :CROP[1]]
            want = K.lookup(K.widen(f1[:CROP[0], :CROP[1]], dt), K.widen(f2, dt), flow[:CROP[0], :CROP[1]], 1, RADIUS, LEVELS)
            same = bool(np.ascontiguousarray(got).tobytes() == want.tobytes())
            med, spread = kit.median_ms(ms), kit.spread(ms["copy"])
            taps = (2 * RADIUS + 2) ** 2
            flop = 2.0 * taps * c * LEVELS * px * n
            f2_bytes = float(taps * c * px * n * (e + 4 * (LEVELS - 1)))
            volume = sum(n * px * (h >> l) * (w >> l) * 4 for l in range(LEVELS))
            for key, _ in variants:
                line = {"key": "%s_%s_c%d_%dx%d_x%d" % (key, dt, c, h, w, n), "features": [c, h, w], "dtype": dt, "items": n,
                        "radius": RADIUS, "levels": LEVELS, **kit.ms_fields(ms[key]), "repeats": a.repeats, "rotating_sets": SETS,
                        "device": nat.device_name()}
                if key == "lookup":
                    t = med[key] * 1e-3
                    line.update({"flop": flop, "TFLOPs": round(flop / t / 1e12, 3), "share_fp32_vec": round(flop / t / FP32_VECTOR_PEAK, 4),
                                 "f2_bytes_requested": f2_bytes, "f2_TBps": round(f2_bytes / t / 1e12, 3), "out_bytes": out_bytes,
                                 "out_over_copy": round(med[key] / med["copy"], 2), "copy_spread": round(spread, 3),
                                 "all_pairs_GB": round(volume / 1e9, 2), "equal_restatement": same})
                if key == "copy":
                    line.update({"bytes_moved": 2 * out_bytes, "TBps": round(2 * out_bytes / (med[key] * 1e-3) / 1e12, 3),
                                 "copy_spread": round(spread, 3)})
                report.line(line)
            del sets, q
            dev.empty_cache()
    report.write(a.out)


if __name__ == "__main__":
    main()
