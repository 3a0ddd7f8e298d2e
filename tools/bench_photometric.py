#!/usr/bin/env python
"""The photometric error (K21, ofl_photometric.hip) against a copy of the bytes it must move and against the route it
replaces, one JSON line per variant.  Two configurations, each in both layouts: C = 3 float32 at 2160 x 3840 with 8 items
per launch (images) and C = 128 float16 at 270 x 480 with 8 items (a network's features at 1/8 resolution).

In ONE process and INTERLEAVED -- every repeat times each variant once, between two HIP events, as a run of launches long
enough to last 100 ms -- over rotating working sets of at least 3 x 256 MiB (bench_ops.n_sets):

  photometric      ofl_photometric_dev, L1, writing err + covered: reads 2 C elements + 8 (flow) + 1 (fmask), writes 5 B/px
  copy_same_bytes  ofl_copy_dev moving the same number of bytes (half read, half written): yardstick (a)
  apply_tensor     ofl_gather_tensor_dev on `far` with the same field: the first half of the route a 't' field had before
  copy_result      ofl_copy_dev reading and writing the C-channel result once: the elementwise pass over it, at best
Route (b) is apply_tensor + copy_result, median plus median.  Every field is its own (N fields back to back, reference
't'): a smooth field of about 5 px, the generator of tests/consistency_ref.py at full size, with a hole in its mask; `far`
is random, `near` a copy of it -- the time does not depend on the values.  Every line carries the median, the smallest and
the largest per-launch time of its repeats; `over_copy` and `over_route_b` are median over median, and `copy_spread` =
(max - min) / median of the copy's own repeats in this run, the margin below which a difference says nothing on a shared
machine.

    python tools/bench_photometric.py [--repeats 16] [--out profiles/r20_photometric_bench.jsonl]
"""
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np
import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from bench_ops import n_sets
from bench_consistency import smooth
import bench_kit as kit

nat = of.native
MIN_MS = 100.0                      # every timed repeat lasts at least this long
EL = {'float32': (nat.EL_F32, 4, np.float32), 'float16': (nat.EL_F16, 2, np.float16)}
LAYOUT = {'chw': nat.TENSOR_NCHW, 'hwc': nat.TENSOR_NHWC}


def runs(timer, make, sets):
    """make(working set) -> one launch; -> make'(working set) that launches often enough to last MIN_MS, each launch on the
    next working set of the rotation (starting with the one given), and the count"""
    one = min(timer(make(sets[i % len(sets)])) for i in range(3))
    iters = max(1, int(math.ceil(MIN_MS / max(one, 1e-3))))
    calls = [make(q) for q in sets]

    def many(q):
        first = next(i for i, s in enumerate(sets) if s is q)

        def run():
            for i in range(iters):
                calls[(first + i) % len(calls)]()
        return run
    return many, iters


def main():
    a, lib, timer, report = kit.start(16)
    for name, c, dtype, h, w, n in (("rgb_f32_4k_x8", 3, 'float32', 2160, 3840, 8), ("feat128_f16_270x480_x8", 128, 'float16', 270, 480, 8)):
        el, eb, npdt = EL[dtype]
        px = n * h * w
        moved = px * (2 * c * eb + 8 + 1 + 4 + 1)
        tensor_bytes = px * c * eb
        k = n_sets(moved)
        rng = np.random.default_rng(7)
        fmask = np.ones((h, w), np.uint8)
        fmask[h // 4:h // 2, w // 8:w // 3] = 0
        for layout in ('chw', 'hwc'):
            sets = []
            for s in range(k):
                item = rng.standard_normal(h * w * c, dtype=np.float32).astype(npdt)
                q = {"far": kit.replicate(dev.DeviceBuffer(tensor_bytes), item, n), "near": dev.DeviceBuffer(tensor_bytes),
                     "flow": kit.replicate(dev.DeviceBuffer(px * 8), smooth(rng, h, w, 5.0), n),
                     "fm": kit.replicate(dev.DeviceBuffer(px), fmask, n),
                     "err": dev.DeviceBuffer(px * 4), "cov": dev.DeviceBuffer(px), "dst": dev.DeviceBuffer(tensor_bytes), "valid": dev.DeviceBuffer(px),
                     "c0": dev.DeviceBuffer(max(moved // 2, tensor_bytes)), "c1": dev.DeviceBuffer(max(moved // 2, tensor_bytes))}
                nat.check(lib.ofl_copy_dev(q["near"].ptr, q["far"].ptr, tensor_bytes, None))
                nat.check(lib.ofl_memset(q["c0"].ptr, 1, q["c0"].nbytes, None))
                sets.append(q)
            dev.sync()

            def photometric(q):
                return lambda: nat.check(lib.ofl_photometric_dev(q["near"].ptr, q["far"].ptr, el, LAYOUT[layout], n, c, h, w, q["flow"].ptr,
                                                                 q["fm"].ptr, 0, -1, None, None, nat.PHOTO_L1, np.float32(1e-3), np.float32(0),
                                                                 q["err"].ptr, q["cov"].ptr, None, None, nat.QUANT_OPENCV, None))

            def apply_tensor(q):
                return lambda: nat.check(lib.ofl_gather_tensor_dev(q["far"].ptr, el, LAYOUT[layout], n, c, h, w, q["flow"].ptr, 0, -1, None, 0,
                                                                   q["fm"].ptr, q["dst"].ptr, q["valid"].ptr, nat.QUANT_OPENCV, None))

            table = [("photometric", photometric), ("copy_same_bytes", kit.copy_variant(moved // 2)),
                     ("apply_tensor", apply_tensor), ("copy_result", kit.copy_variant(tensor_bytes))]
            variants, iters = [], {}
            for key, make in table:
                many, iters[key] = runs(timer, make, sets)
                variants.append((key, many))
            total = kit.interleaved(timer, variants, sets, a.repeats)
            ms = {key: [t / iters[key] for t in v] for key, v in total.items()}
            # the kernel's covered mask is K12's valid, also at this size
            q = sets[0]
            photometric(q)()
            apply_tensor(q)()
            same = bool(np.array_equal(q["cov"].to_host((px,), np.uint8), q["valid"].to_host((px,), np.uint8)))
            med, spread = kit.median_ms(ms), kit.spread(ms["copy_same_bytes"])
            route_b = med["apply_tensor"] + med["copy_result"]
            bytes_of = {"photometric": moved, "copy_same_bytes": moved // 2 * 2, "apply_tensor": px * (2 * c * eb + 8 + 1 + 1), "copy_result": 2 * tensor_bytes}
            for key, _ in table:
                report.line({
                    "key": "%s_%s_%s" % (key, name, layout), "shape": [h, w], "items": n, "channels": c, "dtype": dtype, "layout": layout,
                    "bytes_moved": int(bytes_of[key]), **kit.ms_fields(ms[key]), "GBps": round(bytes_of[key] / med[key] / 1e6, 1),
                    "repeats": a.repeats, "launches_per_repeat": iters[key], "timed_ms_per_repeat_min": round(min(total[key]), 1),
                    "rotating_sets": k, "over_copy": round(med[key] / med["copy_same_bytes"], 3), "copy_spread": round(spread, 3),
                    "route_b_ms": round(route_b, 4), "over_route_b": round(med[key] / route_b, 3),
                    "covered_equals_apply_tensor_valid": same, "device": nat.device_name()})
            del sets, q
            dev.empty_cache()
    report.write(a.out)


if __name__ == "__main__":
    main()
