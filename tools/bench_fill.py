#!/usr/bin/env python
"""The fill from the nearest valid pixel (K15, ofl_fill.hip) against a device copy, one JSON line per variant: 2160 x 3840 with
8 fields per launch and 1080 x 1920 with 16.

In ONE process and INTERLEAVED -- every repeat times one call of each variant (both passes of the fill), each call between two
HIP events -- over 2 rotating working sets (each far larger than the Infinity Cache):

  fill_blobs          about 10 % of the pixels invalid in blobs of radius <= 16 px: what a consistency check leaves
  fill_kitti          the upper third without any source, 20 % random sources below: a sparse ground truth
  fill_one_source     one source per field (1080p only): the outward scan's worst case, reported and not optimised for
  copy_18Bpx          ofl_copy_dev moving 18 B/px in total (9 read, 9 written)

The fill writes vectors and mask (what DeviceFlow.fill asks for).  It moves at least 22 B/px -- the row pass reads the mask
and writes 2 B/px of offsets, the column pass reads them and the vector and writes vector and mask -- plus 2 B per row it
scans.  One generated field per working set is replicated into the slots of the batch on the device.  Every line carries the
median, the smallest and the largest of its repeats; `over_copy` is median over median, and `copy_spread` = (max - min) /
median of the copy's own repeats in this run, the margin below which a difference says nothing on a shared machine.
`d2_equal_scipy`: the squared distances of the first field of the timed buffers equal SciPy's transform.  `host_route_*` is
the wall time of what this replaces for ONE 4K field: to_host(), scipy.ndimage.distance_transform_edt(return_indices=True),
the fancy index, to_device().

    python tools/bench_fill.py [--repeats 16] [--out profiles/r14_fill_bench.jsonl]
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np
from scipy import ndimage
import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
import bench_kit as kit

nat = of.native
SETS = 2


def blobs(h, w, rng, share=0.10, rmax=16):
    """a mask with about `share` of its pixels cleared in discs of radius 4 .. rmax"""
    m = np.ones((h, w), np.uint8)
    count = int(-np.log(1 - share) * h * w / (np.pi * (rmax * rmax + 4 * rmax + 16) / 3.0))     # E[r^2] of a uniform radius
    yy, xx = np.mgrid[-rmax:rmax + 1, -rmax:rmax + 1]
    rr = yy * yy + xx * xx
    for cy, cx, r in zip(rng.integers(0, h, count), rng.integers(0, w, count), rng.integers(4, rmax + 1, count)):
        y0, y1, x0, x1 = max(cy - rmax, 0), min(cy + rmax + 1, h), max(cx - rmax, 0), min(cx + rmax + 1, w)
        disc = rr[y0 - cy + rmax:y1 - cy + rmax, x0 - cx + rmax:x1 - cx + rmax] <= r * r
        m[y0:y1, x0:x1][disc] = 0
    return m


def kitti(h, w, rng):
    m = (rng.random((h, w)) < 0.2).astype(np.uint8)
    m[:h // 3] = 0
    return m


def one_source(h, w, rng):
    m = np.zeros((h, w), np.uint8)
    m[h // 2, w // 2] = 1
    return m


def main():
    a, lib, timer, report = kit.start(16)
    for name, h, w, n in (("4k_x8", 2160, 3840, 8), ("1080p_x16", 1080, 1920, 16)):
        px1, px = h * w, n * h * w
        patterns = [("fill_blobs", blobs), ("fill_kitti", kitti)] + ([("fill_one_source", one_source)] if h == 1080 else [])
        nbytes = dev._size_query(lib.ofl_fill_workspace_bytes, h, w, n)
        sets, first = [], {}
        for s in range(SETS):
            rng = np.random.default_rng(100 + s)
            q = {"vecs": dev.DeviceBuffer(px * 8), "out_vecs": dev.DeviceBuffer(px * 8), "out_mask": dev.DeviceBuffer(px),
                 "work": dev.DeviceBuffer(nbytes), "c0": dev.DeviceBuffer(px * 9), "c1": dev.DeviceBuffer(px * 9)}
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

        def fill(q, key, d2=None):
            return lambda: nat.check(lib.ofl_fill_dev(q["vecs"].ptr, q[key].ptr, None, h, w, n, -1, q["work"].ptr, nbytes, q["out_vecs"].ptr,
                                                      q["out_mask"].ptr, None, None if d2 is None else d2.ptr, None))

        variants = [(key, (lambda key: lambda q: fill(q, key))(key)) for key, _ in patterns]
        variants.append(("copy_18Bpx", kit.copy_variant(px * 9)))
        ms = kit.interleaved(timer, variants, sets, a.repeats)
        # the distances of the timed buffers are SciPy's, also at this size (the first field of the first set)
        same = {}
        d2 = dev.DeviceBuffer(px * 4)
        for key, _ in patterns:
            fill(sets[0], key, d2)()
            got = d2.to_host((h, w), np.uint32)
            want = np.rint(ndimage.distance_transform_edt(first[key][1] == 0) ** 2).astype(np.int64)
            same[key] = bool(np.array_equal(got.astype(np.int64), want))
            filled = sets[0]["out_mask"].to_host((h, w), np.uint8)
            same[key] = same[key] and bool(filled.all())
        del d2
        med, spread = kit.median_ms(ms), kit.spread(ms["copy_18Bpx"])
        for key, _ in variants:
            line = {"key": "%s_%s" % (key, name), "shape": [h, w], "fields": n,
                    **kit.ms_fields(ms[key]),
                    "repeats": a.repeats, "rotating_sets": SETS, "over_copy": round(med[key] / med["copy_18Bpx"], 3),
                    "copy_spread": round(spread, 3), "device": nat.device_name()}
            if key in same:
                line.update({"bytes_per_px_min": 22, "TBps_of_min_bytes": round(22 * px / med[key] / 1e9, 3),
                             "invalid_share": round(float((first[key][1] == 0).mean()), 4), "d2_equal_scipy": same[key]})
            else:
                line.update({"bytes_per_px": 18, "TBps": round(18 * px / med[key] / 1e9, 3)})
            report.line(line)
        if h == 2160:
            # the route this replaces, one field: over PCIe, SciPy's transform with indices, the fancy index, back over PCIe
            vecs, mask = first["fill_blobs"]
            d_flow = dev.DeviceFlow(sets[0]["vecs"].view(0, px1 * 8), sets[0]["fill_blobs"].view(0, px1), (h, w), 't')
            t0 = time.perf_counter()
            hv, hm = d_flow.to_host()
            t1 = time.perf_counter()
            _, (iy, ix) = ndimage.distance_transform_edt(~hm, return_indices=True)
            t2 = time.perf_counter()
            filled = hv[iy, ix]
            t3 = time.perf_counter()
            back = dev.DeviceFlow.from_host(filled, 't')
            dev.sync()
            t4 = time.perf_counter()
            report.line({"key": "host_route_%s" % name, "shape": [h, w], "fields": 1, "to_host_ms": round((t1 - t0) * 1e3, 1),
                         "scipy_edt_ms": round((t2 - t1) * 1e3, 1), "index_ms": round((t3 - t2) * 1e3, 1),
                         "to_device_ms": round((t4 - t3) * 1e3, 1), "wall_ms_per_field": round((t4 - t0) * 1e3, 1),
                         "device_ms_per_field": round(med["fill_blobs"] / n, 4), "device": nat.device_name()})
            del d_flow, back
        del sets, q
        dev.empty_cache()
    report.write(a.out)


if __name__ == "__main__":
    main()
