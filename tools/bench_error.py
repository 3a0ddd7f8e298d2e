#!/usr/bin/env python
"""The flow-error evaluation (K14, ofl_error.hip) against a device copy of the same bytes, one JSON line per variant:
2160 x 3840 with 8 pairs per launch and 1080 x 1920 with 16.

In ONE process and INTERLEAVED -- every repeat times one launch of each variant, each launch between two HIP events -- over
rotating working sets of at least 3 x 256 MiB (bench_ops.n_sets: no launch finds its bytes in the Infinity Cache):

  error_records       ofl_flow_error_dev, records only                     (8 + 8 + 1 + 1 read: 18 B/px, the chunk kernel
                      and the finishing kernel together)
  error_epe_map       the same with the float32 epe_map                      (22 B/px)
  error_records_odd   records only on the same buffers read as fields one row and one column smaller (2159 x 3839): an odd
                      pixel count per pair, so every second pair sits 8 bytes off the 16-byte grid and the launch takes the
                      generic path (8-byte and 1-byte loads).  One column less alone would not do: 2160 * 3839 is still a
                      multiple of 4 and takes the wide path
  copy_18Bpx          ofl_copy_dev moving 18 B/px in total (9 read, 9 written)

The ground truth has speeds in all three Sintel bins and a tenth of each mask cleared; the estimate is off by 0.3 to 15 px.
One generated pair per working set is replicated into the slots of the batch on the device: the kernel has no
data-dependent branch.  Every line carries the median, the smallest and the largest of its repeats; `over_copy` is median
over median, and `copy_spread` = (max - min) / median of the copy's own repeats in this run, the margin below which a
difference says nothing on a shared machine.  `host_route_*` is the wall time of what this replaces for ONE pair: two
to_host() calls (17 B/px each over PCIe) plus the NumPy restatement of tests/error_ref.py.

    python tools/bench_error.py [--repeats 16] [--out profiles/r13_error_bench.jsonl]
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import numpy as np
import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from bench_ops import n_sets
import bench_kit as kit
import error_ref

nat = of.native


def generate(h, w, seed):
    rng = np.random.default_rng(seed)
    n = h * w
    speed = (rng.choice(np.array([3.0, 20.0, 60.0], np.float32), n) * rng.uniform(0.2, 1.3, n).astype(np.float32))
    angle = rng.uniform(0, 2 * np.pi, n).astype(np.float32)
    gt = np.stack([speed * np.cos(angle), speed * np.sin(angle)], -1).astype(np.float32)
    est = gt + rng.standard_normal((n, 2), np.float32) * rng.choice(np.array([0.3, 2.0, 6.0, 15.0], np.float32), n)[:, None]
    em, gm = (rng.random(n) >= 0.1).astype(np.uint8), (rng.random(n) >= 0.1).astype(np.uint8)
    return est.reshape(h, w, 2), em.reshape(h, w), gt.reshape(h, w, 2), gm.reshape(h, w)


def main():
    a, lib, timer, report = kit.start(16)
    thr, (out_abs, out_rel), edges, _, _ = dev.error_args()
    for name, h, w, n in (("4k_x8", 2160, 3840, 8), ("1080p_x16", 1080, 1920, 16)):
        px1, px = h * w, n * h * w
        k = n_sets(18 * px)
        nbytes = dev._size_query(lib.ofl_flow_error_workspace_bytes, h, w, n)
        sets, first = [], None
        for s in range(k):
            q = {"est": dev.DeviceBuffer(px * 8), "gt": dev.DeviceBuffer(px * 8), "em": dev.DeviceBuffer(px), "gm": dev.DeviceBuffer(px),
                 "epe": dev.DeviceBuffer(px * 4), "work": dev.DeviceBuffer(nbytes), "rec": dev.DeviceBuffer(n * 96),
                 "c0": dev.DeviceBuffer(px * 9), "c1": dev.DeviceBuffer(px * 9)}
            pair = generate(h, w, 100 + s)
            first = first or pair
            for key, arr in zip(("est", "em", "gt", "gm"), pair):
                kit.replicate(q[key], arr, n)
            nat.check(lib.ofl_memset(q["c0"].ptr, 1, px * 9, None))
            sets.append(q)

        def error(q, odd, with_map):
            return lambda: nat.check(lib.ofl_flow_error_dev(q["est"].ptr, q["em"].ptr, q["gt"].ptr, q["gm"].ptr, h - odd, w - odd, n, thr.ctypes.data,
                                                            out_abs, out_rel, edges.ctypes.data, q["work"].ptr, nbytes, q["rec"].ptr,
                                                            q["epe"].ptr if with_map else None, None, None))

        variants = [
            ("error_records", 18, lambda q: error(q, 0, False)),
            ("error_epe_map", 22, lambda q: error(q, 0, True)),
            ("error_records_odd", 18, lambda q: error(q, 1, False)),
            ("copy_18Bpx", 18, kit.copy_variant(px * 9)),
        ]
        ms = kit.interleaved(timer, [(key, make) for key, _, make in variants], sets, a.repeats)
        # the records of the timed buffers are the restatement's, also at this size (the first pair of the first set)
        error(sets[0], 0, False)()
        rec = sets[0]["rec"].to_host((n,), dev.ERROR_RECORD)[0]
        want = error_ref.flow_error(*first, thr, out_abs, out_rel, edges)
        same = np.frombuffer(rec.tobytes()[:48], np.uint32).tolist() == error_ref.record_words(want)
        med, spread = kit.median_ms(ms), kit.spread(ms["copy_18Bpx"])
        for key, bpp, _ in variants:
            height, width = (h - 1, w - 1) if key.endswith("_odd") else (h, w)
            moved = bpp * n * height * width
            report.line({
                "key": "%s_%s" % (key, name), "shape": [height, width], "pairs": n, "bytes_per_px": bpp, "bytes_moved": int(moved),
                **kit.ms_fields(ms[key]),
                "TBps": round(moved / med[key] / 1e9, 3), "repeats": a.repeats, "rotating_sets": k,
                "over_copy": round(med[key] / med["copy_18Bpx"], 3), "copy_spread": round(spread, 3),
                "counts_equal_restatement": bool(same), "device": nat.device_name()})
        # the route this replaces, one pair: both fields over PCIe, then NumPy
        d_est = dev.DeviceFlow(sets[0]["est"].view(0, px1 * 8), sets[0]["em"].view(0, px1), (h, w), 't')
        d_gt = dev.DeviceFlow(sets[0]["gt"].view(0, px1 * 8), sets[0]["gm"].view(0, px1), (h, w), 't')
        t0 = time.perf_counter()
        (ev, em), (gv, gm) = d_est.to_host(), d_gt.to_host()
        t1 = time.perf_counter()
        error_ref.flow_error(ev, em, gv, gm, thr, out_abs, out_rel, edges)
        t2 = time.perf_counter()
        report.line({"key": "host_route_%s" % name, "shape": [h, w], "pairs": 1, "to_host_ms": round((t1 - t0) * 1e3, 1),
                     "numpy_ms": round((t2 - t1) * 1e3, 1), "wall_ms_per_pair": round((t2 - t0) * 1e3, 1),
                     "device_ms_per_pair": round(med["error_records"] / n, 4), "device": nat.device_name()})
        del sets, q, d_est, d_gt
        dev.empty_cache()
    report.write(a.out)


if __name__ == "__main__":
    main()
