#!/usr/bin/env python
"""The variational refinement (K23, ofl_refine.hip) at its defaults against (a) the census distance (K22, hard, K = 3) on
the same buffers, (b) a copy of the bytes its launch structure must move and (c) the route it replaces, one JSON line per
variant.  Two sizes -- 2160 x 3840 with 8 items per call and 1080 x 1920 with 16 --, C = 3 float32 (an image) in both
layouts and C = 1 float16 (a reduced plane).

In ONE process and INTERLEAVED -- every repeat times each variant once, between two HIP events, as a run of calls long
enough to last 100 ms -- over rotating working sets (bench_ops.n_sets):

  refine_fp{F}_sor{S}   ofl_refine_dev with fixed_point = F, sor = S: 5/5 is the default call; 1/5 and 2/5 differ by one
                        fixed-point iteration of 5 sweeps, 1/1 and 2/1 by one iteration of 1 sweep
  census_hard_k3        ofl_census_dev writing err + covered: the same staging with a window instead of a gradient
  copy                  ofl_copy_dev moving as many bytes as the census call must (half read, half written): the yardstick;
                        its rate prices every byte model below
Derived, median over median:
  setup_finish_ms   2 x fp1_sor1 - fp2_sor1: the setup launch plus the finish launch (the ABI does not time one launch alone)
                    -> (a) over_census
  iteration_ms      fp2_sor5 - fp1_sor5: one fixed-point iteration at the default sor -> (b) over_copy_model, against the
                    copy's rate times MODEL_ITERATION bytes
  Byte model, per pixel and at cache-line granularity: the weights launch reads flags 1 + flow 8 + d 8 + gx, gy,
  Iz 12 and writes wD, s 8 = 37; a half-sweep updates one colour, but the two colours share every cache line, so it reads
  flags 1 + flow 8 + d 8 + gx, gy, Iz, wD, s 20 = 37 and writes d 8 = 45; one iteration moves 37 + 2 sor 45.  Setup reads
  2 C elements + flow 8 + fmask 1 and writes gx, gy, Iz 12 + d 8 + flags 1; finish reads flow 8 + d 8 + flags 1, writes 8.
(c) the host route -- to_host of the field, tests/refine_ref.py (the NumPy restatement, float32) on host images, to_device
of the result -- takes seconds per item, so it is timed ONCE by the wall clock on ONE item of 1080 x 1920 and compared with
the device's time per item at that size; it is not run at 2160 x 3840.  `copy_spread` = (max - min) / median of the copy's
own repeats in this run, the margin below which a difference says nothing on a shared machine; `census_spread` likewise.

    python tools/bench_refine.py [--repeats 16] [--out profiles/r22_refine_bench.jsonl]
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
from bench_consistency import smooth
from bench_photometric import runs, EL, LAYOUT
import bench_kit as kit

nat = of.native
CALLS = [(5, 5), (1, 5), (2, 5), (1, 1), (2, 1)]             # (fixed_point, sor)
WEIGHTS_B, HALF_SWEEP_B = 37, 45                             # bytes per pixel, see the module docstring


def host_route(lib, near, far, layout, flow, h, w):
    """one item: the field down, the restatement, the result up -> wall seconds (the images are on the host already)"""
    from oracle import np_oracle
    np_oracle.build()
    import refine_ref as Rf
    import tensor_ref as T
    d = dev.DeviceFlow.from_host(flow, 't')
    dev.sync()
    t0 = time.perf_counter()
    vecs, mask = d.to_host()
    out = Rf.restate(T.to_planar(near[None], layout), T.to_planar(far[None], layout), vecs, mask, -1)['vecs'][0]
    back = dev.DeviceFlow.from_host(out, 't', mask)
    dev.sync()
    t = time.perf_counter() - t0
    del back
    return t


def main():
    a, lib, timer, report = kit.start(16)
    for name, c, dtype, h, w, n, layouts in (("rgb_f32_4k_x8", 3, 'float32', 2160, 3840, 8, ('chw', 'hwc')),
                                             ("rgb_f32_1080p_x16", 3, 'float32', 1080, 1920, 16, ('chw', 'hwc')),
                                             ("grey_f16_4k_x8", 1, 'float16', 2160, 3840, 8, ('chw',)),
                                             ("grey_f16_1080p_x16", 1, 'float16', 1080, 1920, 16, ('chw',))):
        el, eb, npdt = EL[dtype]
        px = n * h * w
        census_bytes = px * (2 * c * eb + 8 + 1 + 4 + 1)
        setup_finish_bytes = px * (2 * c * eb + 8 + 1 + 12 + 8 + 1) + px * (8 + 8 + 1 + 8)
        tensor_bytes = px * c * eb
        k = n_sets(census_bytes)
        rng = np.random.default_rng(7)
        fmask = np.ones((h, w), np.uint8)
        fmask[h // 4:h // 2, w // 8:w // 3] = 0
        prm = (np.float32(20), np.float32(5), np.float32(0.1), np.float32(0.1))
        for layout in layouts:
            sets, host = [], None
            for s in range(k):
                item = (np.float32(128) + rng.standard_normal(h * w * c, dtype=np.float32) * np.float32(50)).astype(npdt)
                flow = smooth(rng, h, w, 5.0)
                host = host or (item.reshape((c, h, w) if layout == 'chw' else (h, w, c)), flow)
                q = {"far": kit.replicate(dev.DeviceBuffer(tensor_bytes), item, n), "near": dev.DeviceBuffer(tensor_bytes),
                     "flow": kit.replicate(dev.DeviceBuffer(px * 8), flow, n), "fm": kit.replicate(dev.DeviceBuffer(px), fmask, n),
                     "out": dev.DeviceBuffer(px * 8), "ws": dev.DeviceBuffer(29 * px),
                     "err": dev.DeviceBuffer(px * 4), "cov": dev.DeviceBuffer(px),
                     "c0": dev.DeviceBuffer(census_bytes // 2), "c1": dev.DeviceBuffer(census_bytes // 2)}
                nat.check(lib.ofl_copy_dev(q["near"].ptr, q["far"].ptr, tensor_bytes, None))
                nat.check(lib.ofl_memset(q["c0"].ptr, 1, q["c0"].nbytes, None))
                sets.append(q)
            dev.sync()

            def refine(fp, sor):
                return lambda q: lambda: nat.check(lib.ofl_refine_dev(
                    q["near"].ptr, q["far"].ptr, el, LAYOUT[layout], n, c, h, w, q["flow"].ptr, q["fm"].ptr, -1, None, None, None,
                    *prm, fp, sor, np.float32(1.6), q["ws"].ptr, 29 * px, q["out"].ptr, None, nat.QUANT_OPENCV, None))

            def census(q):
                return lambda: nat.check(lib.ofl_census_dev(
                    q["near"].ptr, q["far"].ptr, el, LAYOUT[layout], n, c, h, w, q["flow"].ptr, q["fm"].ptr, 0, -1, None, None,
                    3, nat.CENSUS_HARD, np.float32(0), np.float32(0), 8, np.float32(0), q["err"].ptr, q["cov"].ptr, None, None,
                    nat.QUANT_OPENCV, None))

            table = [("refine_fp%d_sor%d" % fs, refine(*fs)) for fs in CALLS]
            table += [("census_hard_k3", census), ("copy", kit.copy_variant(census_bytes // 2))]
            variants, iters = [], {}
            for key, make in table:
                many, iters[key] = runs(timer, make, sets)
                variants.append((key, many))
            total = kit.interleaved(timer, variants, sets, a.repeats)
            ms = {key: [t / iters[key] for t in v] for key, v in total.items()}
            med = kit.median_ms(ms)
            copy_rate = census_bytes // 2 * 2 / med["copy"]                                   # bytes per millisecond
            copy_spread, census_spread = kit.spread(ms["copy"]), kit.spread(ms["census_hard_k3"])
            setup_finish = 2 * med["refine_fp1_sor1"] - med["refine_fp2_sor1"]
            iteration = med["refine_fp2_sor5"] - med["refine_fp1_sor5"]
            iteration_bytes = px * (WEIGHTS_B + 2 * 5 * HALF_SWEEP_B)
            default_bytes = setup_finish_bytes + 5 * iteration_bytes
            # what the default call did to the field, also at this size: every vector finite, most of the domain moved
            q = sets[0]
            refine(5, 5)(q)()
            got, before = q["out"].to_host((px * 2,), np.float32), q["flow"].to_host((px * 2,), np.float32)
            moved_share = round(float((got != before).mean()), 4) if bool(np.isfinite(got).all()) else None
            common = {"shape": [h, w], "items": n, "channels": c, "dtype": dtype, "layout": layout, "repeats": a.repeats,
                      "rotating_sets": k, "copy_spread": round(copy_spread, 3), "census_spread": round(census_spread, 3),
                      "device": nat.device_name()}
            bytes_of = {"census_hard_k3": census_bytes, "copy": census_bytes // 2 * 2, "refine_fp5_sor5": default_bytes}
            for key, _ in table:
                record = {"key": "%s_%s_%s" % (key, name, layout), **common, **kit.ms_fields(ms[key]),
                          "launches_per_repeat": iters[key], "timed_ms_per_repeat_min": round(min(total[key]), 1)}
                if key in bytes_of:
                    record.update(bytes_moved=int(bytes_of[key]), GBps=round(bytes_of[key] / med[key] / 1e6, 1))
                if key == "refine_fp5_sor5":
                    record.update(over_copy_model=round(med[key] / (default_bytes / copy_rate), 3), moved_share=moved_share,
                                  ms_per_item=round(med[key] / n, 4))
                report.line(record)
            report.line({"key": "setup_finish_%s_%s" % (name, layout), **common, "derived_ms": round(setup_finish, 4),
                         "bytes_moved": int(setup_finish_bytes), "over_census": round(setup_finish / med["census_hard_k3"], 3),
                         "over_copy_model": round(setup_finish / (setup_finish_bytes / copy_rate), 3)})
            report.line({"key": "iteration_sor5_%s_%s" % (name, layout), **common, "derived_ms": round(iteration, 4),
                         "bytes_moved": int(iteration_bytes), "GBps": round(iteration_bytes / iteration / 1e6, 1),
                         "over_copy_model": round(iteration / (iteration_bytes / copy_rate), 3)})
            if (h, w) == (1080, 1920):
                seconds = host_route(lib, host[0].astype(np.float32), host[0].astype(np.float32), layout, host[1], h, w)
                report.line({"key": "host_route_one_item_%s_%s" % (name, layout), **common, "wall_ms_once": round(seconds * 1e3, 1),
                             "device_ms_per_item": round(med["refine_fp5_sor5"] / n, 4),
                             "route_over_device": round(seconds * 1e3 / (med["refine_fp5_sor5"] / n), 1)})
            del sets, q
            dev.empty_cache()
    report.write(a.out)


if __name__ == "__main__":
    main()
