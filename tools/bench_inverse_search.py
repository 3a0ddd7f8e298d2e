#!/usr/bin/env python
"""The dense inverse search (K24, ofl_inverse_search.hip: setup + search + densify) against (a) a copy of the bytes the call
must move and (b) the photometric error (K21, l1) on the same buffers, and (c) estimate_flow as a whole, one JSON line per
variant.  Two sizes -- 2160 x 3840 with 8 items per call and 1080 x 1920 with 16 --, C = 3 float32 planar (an image) and
C = 1 float16 (a reduced plane).  The images are a smooth wave pattern (tests/refine_ref.wave_image, another phase per
channel and working set) and the same pattern shifted by (2.3, -1.6) px; the search starts from the zero field (flow = NULL),
so most patches take all their iterations -- on noise the search would stop after one step and the time would say nothing.

In ONE process and INTERLEAVED -- every repeat times each variant once, between two HIP events, as a run of calls long
enough to last 100 ms -- over rotating working sets (bench_ops.n_sets):

  search_p8_s4      ofl_inverse_search_dev, patch 8, stride 4, 12 iterations: the default call
  search_p8_s8      the same with stride 8: a quarter of the patches, no overlap
  search_p4_s4      patch 4, stride 4: as many patches as the default, a quarter of the pixels each
  photometric_l1    ofl_photometric_dev writing err + covered from the same tensors and a field: one warp of C channels
  copy              ofl_copy_dev moving as many bytes as the default call must (half read, half written): the yardstick
Bytes the call must move, per pixel: 2 C elements read, 8 + 1 written, plus 12 per patch.  (What it does move on top: the
two planes, 8 written and read back by every sample.)
Supposition to confront: one search iteration makes (P / S)^2 photometric-like samples per pixel from a one-channel plane, so
the call should cost about iterations (P / S)^2 x (b): `taps_model` = that product, `over_taps_model` = measured / model.
(c) estimate_flow, whole, with the defaults on ONE item (C = 3 float32 planar): a run of calls by the two events, so the
launch gaps of its Python loop are inside the figure; `ms_per_item`.  Its pattern is stretched by 2^(levels - 2), so that the
coarsest level still sees wavelengths of 8 px and more: at its natural wavelengths the 2 x 2 means of 4 and 5 levels alias the
pattern away, the coarse levels match noise, and a periodic image then locks into the wrong period (an end-point error of
34 px was measured so at 2160 x 3840; the time is the same).
`copy_spread` = (max - min) / median of the copy's own repeats in this run, the margin below which a difference says
nothing on a shared machine; `photometric_spread` likewise.  `epe` = the mean end-point error of item 0's result against
the true shift over the pixels 16 from the frame: the search did find the field at this size.

    python tools/bench_inverse_search.py [--repeats 16] [--out profiles/r23_inverse_search_bench.jsonl]
"""
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import numpy as np
import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.args import patch_origins
from bench_ops import n_sets
from bench_photometric import runs, EL, LAYOUT, MIN_MS
import bench_kit as kit

nat = of.native
SHIFT = (2.3, -1.6)
SEARCHES = [("search_p8_s4", 8, 4), ("search_p8_s8", 8, 8), ("search_p4_s4", 4, 4)]
ITERATIONS = 12


def wave_image(xs, ys):
    """tests/refine_ref.wave_image: the pattern of the known answers"""
    return (128 + 40 * np.sin(2 * np.pi * xs / 23) * np.cos(2 * np.pi * ys / 31) + 30 * np.sin(2 * np.pi * (xs + ys) / 17)
            + 25 * np.cos(2 * np.pi * (xs - 2 * ys) / 41))


def pair(h, w, c, npdt, phase, stretch=1.0):
    """(near, far) planar (c, h, w): far(q + SHIFT) = near(q), channel k and working set `phase` moved along the pattern,
    whose wavelengths (17 to 41 px) are multiplied by `stretch`"""
    ys, xs = np.mgrid[:h, :w].astype(np.float32)
    img = lambda x, y, k: wave_image((x + 7 * k + 13 * phase) / stretch, (y + 5 * k) / stretch)
    near = np.stack([img(xs, ys, k) for k in range(c)])
    far = np.stack([img(xs - SHIFT[0], ys - SHIFT[1], k) for k in range(c)])
    return near.astype(npdt), far.astype(npdt)


def epe_of_item0(lib, out, h, w):
    one = dev.DeviceBuffer(h * w * 8)
    nat.check(lib.ofl_copy_dev(one.ptr, out.ptr, h * w * 8, None))
    d = one.to_host((h, w, 2), np.float32)[16:-16, 16:-16].astype(np.float64) - np.array(SHIFT)
    return round(float(np.sqrt((d * d).sum(axis=-1)).mean()), 4)


def main():
    a, lib, timer, report = kit.start(16)
    for name, c, dtype, h, w, n in (("rgb_f32_4k_x8", 3, 'float32', 2160, 3840, 8), ("rgb_f32_1080p_x16", 3, 'float32', 1080, 1920, 16),
                                    ("grey_f16_4k_x8", 1, 'float16', 2160, 3840, 8), ("grey_f16_1080p_x16", 1, 'float16', 1080, 1920, 16)):
        el, eb, npdt = EL[dtype]
        layout = 'chw'
        px = n * h * w
        patches = {key: n * len(patch_origins(h, p, s)) * len(patch_origins(w, p, s)) for key, p, s in SEARCHES}
        must = {key: px * (2 * c * eb + 8 + 1) + 12 * patches[key] for key, _, _ in SEARCHES}
        photo_bytes = px * (2 * c * eb + 8 + 1 + 4 + 1)
        tensor_bytes = px * c * eb
        ws_bytes = 8 * px + 12 * max(patches.values())
        k = n_sets(must["search_p8_s4"])
        sets = []
        for s in range(k):
            near, far = pair(h, w, c, npdt, s)
            q = {"near": kit.replicate(dev.DeviceBuffer(tensor_bytes), near, n), "far": kit.replicate(dev.DeviceBuffer(tensor_bytes), far, n),
                 "flow": dev.DeviceBuffer.zeros(px * 8), "fm": dev.DeviceBuffer(px),
                 "out": dev.DeviceBuffer(px * 8), "mask": dev.DeviceBuffer(px), "ws": dev.DeviceBuffer(ws_bytes),
                 "err": dev.DeviceBuffer(px * 4), "cov": dev.DeviceBuffer(px),
                 "c0": dev.DeviceBuffer(must["search_p8_s4"] // 2), "c1": dev.DeviceBuffer(must["search_p8_s4"] // 2)}
            nat.check(lib.ofl_memset(q["fm"].ptr, 1, px, None))
            nat.check(lib.ofl_memset(q["c0"].ptr, 1, q["c0"].nbytes, None))
            sets.append(q)
        dev.sync()

        def search(p, s):
            return lambda q: lambda: nat.check(lib.ofl_inverse_search_dev(
                q["near"].ptr, q["far"].ptr, el, LAYOUT[layout], n, c, h, w, None, None, 1, p, s, ITERATIONS, 1, np.float32(1.0),
                q["ws"].ptr, ws_bytes, q["out"].ptr, q["mask"].ptr, None, None, nat.QUANT_EXACT, None))

        def photometric(q):
            return lambda: nat.check(lib.ofl_photometric_dev(q["near"].ptr, q["far"].ptr, el, LAYOUT[layout], n, c, h, w, q["flow"].ptr,
                                                             q["fm"].ptr, 0, 1, None, None, nat.PHOTO_L1, np.float32(1e-3), np.float32(0),
                                                             q["err"].ptr, q["cov"].ptr, None, None, nat.QUANT_EXACT, None))

        table = [(key, search(p, s)) for key, p, s in SEARCHES]
        table += [("photometric_l1", photometric), ("copy", kit.copy_variant(must["search_p8_s4"] // 2))]
        variants, iters = [], {}
        for key, make in table:
            many, iters[key] = runs(timer, make, sets)
            variants.append((key, many))
        total = kit.interleaved(timer, variants, sets, a.repeats)
        ms = {key: [t / iters[key] for t in v] for key, v in total.items()}
        med = kit.median_ms(ms)
        copy_rate = must["search_p8_s4"] // 2 * 2 / med["copy"]                              # bytes per millisecond
        common = {"shape": [h, w], "items": n, "channels": c, "dtype": dtype, "layout": layout, "repeats": a.repeats, "rotating_sets": k,
                  "copy_spread": round(kit.spread(ms["copy"]), 3), "photometric_spread": round(kit.spread(ms["photometric_l1"]), 3),
                  "device": nat.device_name()}
        bytes_of = dict(must, photometric_l1=photo_bytes, copy=must["search_p8_s4"] // 2 * 2)
        geometry = {key: (p, s) for key, p, s in SEARCHES}
        for key, make in table:
            record = {"key": "%s_%s" % (key, name), **common, **kit.ms_fields(ms[key]), "launches_per_repeat": iters[key],
                      "timed_ms_per_repeat_min": round(min(total[key]), 1), "bytes_moved": int(bytes_of[key]),
                      "GBps": round(bytes_of[key] / med[key] / 1e6, 1)}
            if key in geometry:
                p, s = geometry[key]
                model = ITERATIONS * (p / s) ** 2 * med["photometric_l1"]
                make(sets[0])()
                record.update(patch=p, stride=s, iterations=ITERATIONS, patches=patches[key], ms_per_item=round(med[key] / n, 4),
                              over_copy=round(med[key] / (bytes_of[key] / copy_rate), 3),
                              over_photometric=round(med[key] / med["photometric_l1"], 3), taps_model_ms=round(model, 4),
                              over_taps_model=round(med[key] / model, 3), epe=epe_of_item0(lib, sets[0]["out"], h, w))
            report.line(record)
        del sets, q
        dev.empty_cache()
        if c == 3:
            levels = dev.estimate_levels((h, w), None, 8)
            near, far = pair(h, w, c, npdt, 0, stretch=float(1 << (levels - 2)))
            tn, tf = dev.DeviceTensor.from_host(near, 'chw'), dev.DeviceTensor.from_host(far, 'chw')
            call = lambda: dev.estimate_flow(tn, tf)
            one = min(timer(call) for _ in range(3))
            iters_c = max(1, int(math.ceil(MIN_MS / max(one, 1e-3))))

            def many():
                keep = None
                for _ in range(iters_c):
                    keep = call()
                return keep

            times = [timer(many) / iters_c for _ in range(a.repeats)]
            flow = call()
            report.line({"key": "estimate_flow_%s" % name, "shape": [h, w], "items": 1, "channels": c, "dtype": dtype, "layout": 'chw',
                         "levels": levels, "pattern_stretch": 1 << (levels - 2), "repeats": a.repeats, **kit.ms_fields(times), "calls_per_repeat": iters_c,
                         "ms_per_item": round(float(np.median(times)), 4), "spread": round(kit.spread(times), 3),
                         "epe": epe_of_item0(lib, flow.vecs, h, w), "device": nat.device_name()})
            del tn, tf, flow
            dev.empty_cache()
    report.write(a.out)


if __name__ == "__main__":
    main()
