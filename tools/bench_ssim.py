#!/usr/bin/env python
"""The structural dissimilarity (K26, ofl_ssim.hip) against a copy of the bytes it must move, against the photometric error
(K21) and the hard census (K22) on the same buffers and against the route it replaces on the device, one JSON line per
variant.  Three tensors -- C = 3 float32 planar and channels-last (an image) and C = 1 float16 (a reduced plane) --, two
sizes -- 2160 x 3840 with 8 items per launch and 1080 x 1920 with 16 --; K26 at window 3 and 7 with uniform taps and at
window 11 with Wang's Gaussian, each with the full window as `min_count` (the default).

In ONE process and INTERLEAVED -- every repeat times each variant once, between two HIP events, as a run of launches long
enough to last 100 ms -- over rotating working sets of at least 3 x 256 MiB (bench_ops.n_sets), after a warm-up of every
variant on every set (bench_photometric.runs):

  ssim_u3, ssim_u7, ssim_g11   ofl_ssim_dev writing err + covered: must read 2 C elements + 8 (flow) + 1 (fmask) and write 5 B/px
  copy_same_bytes              ofl_copy_dev moving the same number of bytes (half read, half written): yardstick (a)
  photometric                  ofl_photometric_dev, L1, on the same buffers: yardstick (b)
  census_hard_k3, _k7          ofl_census_dev, hard, at the same window: yardstick (c), for K <= 7
  apply_tensor                 ofl_gather_tensor_dev on `far` with the same field: the first step of the route a 't' field had
  copy_result                  ofl_copy_dev reading and writing the C-channel result once: the transform pass over it, at best
  read_result                  ofl_copy_dev moving as many bytes as the result has: the second read of it, at best
Route (d) is apply_tensor + copy_result + read_result, median plus median plus median.  Every field is its own (N fields
back to back, reference 't'): a smooth field of about 5 px with a hole in its mask; `far` is random with a standard deviation
of 50, `near` a copy of it -- the time does not depend on the values.  Every line carries the median, the smallest and the
largest per-launch time of its repeats; `over_copy`, `over_photometric`, `over_census` (same window) and `over_route_d` are
median over median, and `copy_spread` = (max - min) / median of the copy's own repeats in this run, the margin below which
a difference says nothing on a shared machine.  `halo_factor` is (64 + 2r)(16 + 2r) / 1024, the share of staged pixels per
output pixel, and `lds_reads_per_px` = 3 (K + 3) K / 4, the LDS reads of the window phase per output pixel.

    python tools/bench_ssim.py [--repeats 16] [--out profiles/r26_ssim_bench.jsonl]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np
import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.args import ssim_args
from bench_ops import n_sets
from bench_consistency import smooth
from bench_photometric import runs, EL, LAYOUT
import bench_kit as kit

nat = of.native
SSIM = [("ssim_u3", 3, 'uniform'), ("ssim_u7", 7, 'uniform'), ("ssim_g11", 11, 'gaussian')]
CENSUS = [("census_hard_k3", 3), ("census_hard_k7", 7)]


def main():
    a, lib, timer, report = kit.start(16)
    settings = {key: ssim_args(K, weights) for key, K, weights in SSIM}          # the taps stay alive here
    for name, c, dtype, layout, h, w, n in (("rgb_f32_4k_x8", 3, 'float32', 'chw', 2160, 3840, 8), ("rgb_f32_4k_x8", 3, 'float32', 'hwc', 2160, 3840, 8),
                                            ("rgb_f32_1080p_x16", 3, 'float32', 'chw', 1080, 1920, 16), ("rgb_f32_1080p_x16", 3, 'float32', 'hwc', 1080, 1920, 16),
                                            ("grey_f16_4k_x8", 1, 'float16', 'chw', 2160, 3840, 8), ("grey_f16_1080p_x16", 1, 'float16', 'chw', 1080, 1920, 16)):
        el, eb, npdt = EL[dtype]
        px = n * h * w
        moved = px * (2 * c * eb + 8 + 1 + 4 + 1)
        tensor_bytes = px * c * eb
        k = n_sets(moved)
        rng = np.random.default_rng(7)
        fmask = np.ones((h, w), np.uint8)
        fmask[h // 4:h // 2, w // 8:w // 3] = 0
        sets = []
        for s in range(k):
            item = (rng.standard_normal(h * w * c, dtype=np.float32) * np.float32(50)).astype(npdt)
            q = {"far": kit.replicate(dev.DeviceBuffer(tensor_bytes), item, n), "near": dev.DeviceBuffer(tensor_bytes),
                 "flow": kit.replicate(dev.DeviceBuffer(px * 8), smooth(rng, h, w, 5.0), n),
                 "fm": kit.replicate(dev.DeviceBuffer(px), fmask, n),
                 "err": dev.DeviceBuffer(px * 4), "cov": dev.DeviceBuffer(px), "dst": dev.DeviceBuffer(tensor_bytes), "valid": dev.DeviceBuffer(px),
                 "c0": dev.DeviceBuffer(max(moved // 2, tensor_bytes)), "c1": dev.DeviceBuffer(max(moved // 2, tensor_bytes))}
            nat.check(lib.ofl_copy_dev(q["near"].ptr, q["far"].ptr, tensor_bytes, None))
            nat.check(lib.ofl_memset(q["c0"].ptr, 1, q["c0"].nbytes, None))
            sets.append(q)
        dev.sync()

        def ssim(key):
            K, taps, c1, c2, min_count, _ = settings[key]
            return lambda q: lambda: nat.check(lib.ofl_ssim_dev(
                q["near"].ptr, q["far"].ptr, el, LAYOUT[layout], n, c, h, w, q["flow"].ptr, q["fm"].ptr, 0, -1, None, None,
                K, taps.ctypes.data, c1, c2, min_count, np.float32(0), q["err"].ptr, q["cov"].ptr, None, None, nat.QUANT_OPENCV, None))

        def census(K):
            return lambda q: lambda: nat.check(lib.ofl_census_dev(
                q["near"].ptr, q["far"].ptr, el, LAYOUT[layout], n, c, h, w, q["flow"].ptr, q["fm"].ptr, 0, -1, None, None,
                K, nat.CENSUS_HARD, np.float32(0), np.float32(0), K * K - 1, np.float32(0), q["err"].ptr, q["cov"].ptr, None, None,
                nat.QUANT_OPENCV, None))

        def photometric(q):
            return lambda: nat.check(lib.ofl_photometric_dev(q["near"].ptr, q["far"].ptr, el, LAYOUT[layout], n, c, h, w, q["flow"].ptr,
                                                             q["fm"].ptr, 0, -1, None, None, nat.PHOTO_L1, np.float32(1e-3), np.float32(0),
                                                             q["err"].ptr, q["cov"].ptr, None, None, nat.QUANT_OPENCV, None))

        def apply_tensor(q):
            return lambda: nat.check(lib.ofl_gather_tensor_dev(q["far"].ptr, el, LAYOUT[layout], n, c, h, w, q["flow"].ptr, 0, -1, None, 0,
                                                               q["fm"].ptr, q["dst"].ptr, q["valid"].ptr, nat.QUANT_OPENCV, None))

        table = [(key, ssim(key)) for key, _, _ in SSIM] + [(key, census(K)) for key, K in CENSUS]
        table += [("copy_same_bytes", kit.copy_variant(moved // 2)), ("photometric", photometric), ("apply_tensor", apply_tensor),
                  ("copy_result", kit.copy_variant(tensor_bytes)), ("read_result", kit.copy_variant(tensor_bytes // 2))]
        variants, iters = [], {}
        for key, make in table:
            many, iters[key] = runs(timer, make, sets)
            variants.append((key, many))
        total = kit.interleaved(timer, variants, sets, a.repeats)
        ms = {key: [t / iters[key] for t in v] for key, v in total.items()}
        # the share of pixels with a full covered window, and that no error there is out of [0, 1], also at this size
        q = sets[0]
        share = {}
        for key, _, _ in SSIM:
            ssim(key)(q)()
            e, cv = q["err"].to_host((px,), np.float32), q["cov"].to_host((px,), np.uint8)
            share[key] = round(float(cv.mean()), 4) if bool(((e >= 0) & (e <= 1)).all()) else None
        med, spread = kit.median_ms(ms), kit.spread(ms["copy_same_bytes"])
        route_d = med["apply_tensor"] + med["copy_result"] + med["read_result"]
        bytes_of = {"copy_same_bytes": moved // 2 * 2, "photometric": moved, "apply_tensor": px * (2 * c * eb + 8 + 1 + 1),
                    "copy_result": 2 * tensor_bytes, "read_result": tensor_bytes // 2 * 2}
        window = {key: K for key, K, _ in SSIM}
        same_k = {"ssim_u3": "census_hard_k3", "ssim_u7": "census_hard_k7"}
        for key, _ in table:
            record = {
                "key": "%s_%s_%s" % (key, name, layout), "shape": [h, w], "items": n, "channels": c, "dtype": dtype, "layout": layout,
                "bytes_moved": int(bytes_of.get(key, moved)), **kit.ms_fields(ms[key]),
                "GBps": round(bytes_of.get(key, moved) / med[key] / 1e6, 1),
                "repeats": a.repeats, "launches_per_repeat": iters[key], "timed_ms_per_repeat_min": round(min(total[key]), 1),
                "rotating_sets": k, "over_copy": round(med[key] / med["copy_same_bytes"], 3), "copy_spread": round(spread, 3),
                "over_photometric": round(med[key] / med["photometric"], 3),
                "route_d_ms": round(route_d, 4), "over_route_d": round(med[key] / route_d, 3), "device": nat.device_name()}
            if key in window:
                K, r = window[key], window[key] // 2
                record.update(window=K, halo_factor=round((64 + 2 * r) * (16 + 2 * r) / 1024.0, 3),
                              lds_reads_per_px=round(3 * (K + 3) * K / 4.0, 1), covered_share=share[key])
                if key in same_k:
                    record["over_census"] = round(med[key] / med[same_k[key]], 3)
            report.line(record)
        del sets, q
        dev.empty_cache()
    report.write(a.out)


if __name__ == "__main__":
    main()
