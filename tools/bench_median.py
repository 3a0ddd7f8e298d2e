#!/usr/bin/env python
"""The mask-aware median filter (K16, ofl_median.hip) against a device copy, one JSON line per variant: 2160 x 3840 with 8
fields per launch and 1080 x 1920 with 16.

In ONE process and INTERLEAVED -- every repeat times one call of each variant, each call between two HIP events -- over 2
rotating working sets (each far larger than the Infinity Cache):

  median{3,5,7}_all        every pixel valid: the despeckle of a raw network output; interior waves take the fixed-rank path
  median{3,5,7}_random50   half of the pixels valid at random: every window has its own count
  median{3,5,7}_blobs      about 10 % of the pixels invalid in blobs of radius <= 16 px (the mask of tools/bench_fill.py)
  copy_18Bpx               ofl_copy_dev moving 18 B/px in total (9 read, 9 written)

The filter reads vectors and mask and writes vectors and mask (what DeviceFlow.median asks for): 18 B/px without the halo.
No rate is fixed in advance: the yardstick is the copy in the same run.  One generated field per working set is replicated
into the slots of the batch on the device.  Every line carries the median, the smallest and the largest of its repeats;
`over_copy` is median over median, `copy_spread` = (max - min) / median of the copy's own repeats in this run, and
`within_copy_spread` says whether the variant's median lies within that spread of the copy's.  `equal_restatement`: a
128 x 512 corner of the first field of the timed buffers equals the NumPy restatement of tests/median_ref.py byte for byte.
`host_route_*` is the wall time of what this replaces for ONE 4K field: to_host(), scipy.ndimage.median_filter per
component, to_device().

    python tools/bench_median.py [--repeats 16] [--out profiles/r15_median_bench.jsonl]
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import numpy as np
from scipy import ndimage
import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from bench_fill import blobs
import bench_kit as kit
import median_ref as M

nat = of.native
SETS = 2
KSIZES = (3, 5, 7)
CROP = (128, 512)


def all_valid(h, w, rng):
    return np.ones((h, w), np.uint8)


def random50(h, w, rng):
    return (rng.random((h, w)) < 0.5).astype(np.uint8)


def main():
    a, lib, timer, report = kit.start(16)
    for name, h, w, n in (("4k_x8", 2160, 3840, 8), ("1080p_x16", 1080, 1920, 16)):
        px1, px = h * w, n * h * w
        patterns = [("all", all_valid), ("random50", random50), ("blobs", blobs)]
        sets, first = [], {}
        for s in range(SETS):
            rng = np.random.default_rng(100 + s)
            q = {"vecs": dev.DeviceBuffer(px * 8), "out_vecs": dev.DeviceBuffer(px * 8), "out_mask": dev.DeviceBuffer(px),
                 "c0": dev.DeviceBuffer(px * 9), "c1": dev.DeviceBuffer(px * 9)}
            vecs = rng.standard_normal((h, w, 2), np.float32) * np.float32(8)
            arrays = [("vecs", vecs)]
            for key, make in patterns:
                q[key] = dev.DeviceBuffer(px)
                mask = make(h, w, rng)
                arrays.append((key, mask))
                first.setdefault(key, (vecs, mask))
            for key, arr in arrays:
                kit.replicate(q[key], arr, n)
            nat.check(lib.ofl_memset(q["c0"].ptr, 1, px * 9, None))
            sets.append(q)

        def median(q, key, ksize):
            return lambda: nat.check(lib.ofl_median_dev(q["vecs"].ptr, q[key].ptr, None, None, h, w, n, ksize, 1, q["out_vecs"].ptr,
                                                        q["out_mask"].ptr, None))

        variants = [("median%d_%s" % (k, key), (lambda key, k: lambda q: median(q, key, k))(key, k)) for k in KSIZES for key, _ in patterns]
        variants.append(("copy_18Bpx", kit.copy_variant(px * 9)))
        ms = kit.interleaved(timer, variants, sets, a.repeats)
        # the timed buffers give the restatement's bytes, also at this size (a corner of the first field of the first set)
        same = {}
        ch, cw = CROP
        for k in KSIZES:
            for key, _ in patterns:
                median(sets[0], key, k)()
                got_v = sets[0]["out_vecs"].view(0, px1 * 8).to_host((h, w, 2), np.float32)[:ch, :cw]
                got_m = sets[0]["out_mask"].view(0, px1).to_host((h, w), np.uint8)[:ch, :cw]
                vecs, mask = first[key]
                r = k // 2
                want_v, want_m, _ = M.median(vecs[:ch + r, :cw + r], mask[:ch + r, :cw + r], k)
                same["median%d_%s" % (k, key)] = bool(got_v.tobytes() == np.ascontiguousarray(want_v[:ch, :cw]).tobytes()
                                                      and np.array_equal(got_m, want_m[:ch, :cw]))
        med, spread = kit.median_ms(ms), kit.spread(ms["copy_18Bpx"])
        for key, _ in variants:
            line = {"key": "%s_%s" % (key, name), "shape": [h, w], "fields": n,
                    **kit.ms_fields(ms[key]),
                    "repeats": a.repeats, "rotating_sets": SETS, "over_copy": round(med[key] / med["copy_18Bpx"], 3),
                    "copy_spread": round(spread, 3), "bytes_per_px": 18, "TBps": round(18 * px / med[key] / 1e9, 3),
                    "device": nat.device_name()}
            if key in same:
                line.update({"within_copy_spread": bool(med[key] <= med["copy_18Bpx"] * (1 + spread)),
                             "valid_share": round(float(first[key.split("_", 1)[1]][1].mean()), 4), "equal_restatement": same[key]})
            report.line(line)
        if h == 2160:
            # the route this replaces, one field: over PCIe, SciPy's median filter per component (no masks), back over PCIe
            d_flow = dev.DeviceFlow(sets[0]["vecs"].view(0, px1 * 8), sets[0]["all"].view(0, px1), (h, w), 't')
            t0 = time.perf_counter()
            hv, hm = d_flow.to_host()
            t1 = time.perf_counter()
            filtered = np.stack([ndimage.median_filter(hv[..., c], size=5) for c in (0, 1)], axis=-1)
            t2 = time.perf_counter()
            back = dev.DeviceFlow.from_host(filtered, 't')
            dev.sync()
            t3 = time.perf_counter()
            report.line({"key": "host_route_%s" % name, "shape": [h, w], "fields": 1, "ksize": 5, "to_host_ms": round((t1 - t0) * 1e3, 1),
                         "scipy_median_filter_ms": round((t2 - t1) * 1e3, 1), "to_device_ms": round((t3 - t2) * 1e3, 1),
                         "wall_ms_per_field": round((t3 - t0) * 1e3, 1),
                         "device_ms_per_field": round(med["median5_all"] / n, 4), "device": nat.device_name()})
            del d_flow, back
        del sets, q
        dev.empty_cache()
    report.write(a.out)


if __name__ == "__main__":
    main()
