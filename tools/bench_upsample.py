#!/usr/bin/env python
"""Convex upsampling (K17, ofl_upsample.hip) against a device copy, one JSON line per variant: 136 x 240 -> 1088 x 1920 and
270 x 480 -> 2160 x 3840 at factor 8, and 540 x 960 -> 2160 x 3840 at factor 4, 8 items per launch each.

In ONE process and INTERLEAVED -- every repeat times one call of each variant, each call between two HIP events -- over 2
rotating working sets:

  upsample_{f16,f32}_{chw,hwc}   float16 / float32 logits, planar / channels-last; vectors and mask are written
  copy_{f16,f32}                 ofl_copy_dev moving the same number of bytes in total as the upsampling with logits of that
                                 type reads and writes: logits + coarse field (9 B per coarse pixel) + output (9 B per fine
                                 pixel), half of them read and half written

No rate is fixed in advance: the yardstick is the copy in the same run.  One generated item per working set is replicated
into the slots of the batch on the device.  Every line carries the median, the smallest and the largest of its repeats;
`over_copy` is median over median, `copy_spread` = (max - min) / median of the copy's own repeats in this run, and
`within_copy_spread` says whether the variant's median lies within that spread of the copy's.  `equal_restatement`: the
top-left 16 x 64 coarse pixels of the first item of the timed buffers equal the NumPy restatement of tests/upsample_ref.py
byte for byte.

    python tools/bench_upsample.py [--repeats 16] [--out profiles/r16_upsample_bench.jsonl]
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
import upsample_ref as U

nat = of.native
SETS = 2
CROP = (16, 64)
ELEMS = (("f16", np.float16, nat.EL_F16), ("f32", np.float32, nat.EL_F32))
LAYOUTS = (("chw", nat.TENSOR_NCHW), ("hwc", nat.TENSOR_NHWC))


def main():
    a, lib, timer, report = kit.start(16)
    for name, h, w, f, n in (("1080p_f8_x8", 136, 240, 8, 8), ("4k_f8_x8", 270, 480, 8, 8), ("4k_f4_x8", 540, 960, 4, 8)):
        c1, ch = h * w, 9 * f * f
        fine1 = c1 * f * f
        total = {en: n * (ch * c1 * np.dtype(dt).itemsize + 9 * c1 + 9 * fine1) for en, dt, _ in ELEMS}
        sets, first = [], {}
        for s in range(SETS):
            rng = np.random.default_rng(100 + s)
            q = {"vecs": dev.DeviceBuffer(n * c1 * 8), "mask": dev.DeviceBuffer(n * c1), "out_vecs": dev.DeviceBuffer(n * fine1 * 8),
                 "out_mask": dev.DeviceBuffer(n * fine1), "c0": dev.DeviceBuffer(total["f32"] // 2), "c1": dev.DeviceBuffer(total["f32"] // 2)}
            vecs = rng.standard_normal((h, w, 2), np.float32) * np.float32(3)
            mask = (rng.random((h, w)) < 0.95).astype(np.uint8)
            x = (rng.standard_normal((ch, h, w), np.float32) * np.float32(4)).astype(np.float16)      # float16 values in both types
            kit.replicate(q["vecs"], vecs, n)
            kit.replicate(q["mask"], mask, n)
            for en, dt, _ in ELEMS:
                for ln, _ in LAYOUTS:
                    q[en, ln] = dev.DeviceBuffer(n * ch * c1 * np.dtype(dt).itemsize)
                    kit.replicate(q[en, ln], U.to_layout(x.astype(dt), ln), n)
            nat.check(lib.ofl_memset(q["c0"].ptr, 1, q["c0"].nbytes, None))
            first.setdefault("in", (vecs, mask, x))
            sets.append(q)
            del x

        def upsample(q, en, ec, ln, lc):
            return lambda: nat.check(lib.ofl_upsample_convex_dev(q["vecs"].ptr, q["mask"].ptr, q[en, ln].ptr, ec, lc, h, w, n, f,
                                                                 q["out_vecs"].ptr, q["out_mask"].ptr, None))

        variants = [("upsample_%s_%s" % (en, ln), en, (lambda en, ec, ln, lc: lambda q: upsample(q, en, ec, ln, lc))(en, ec, ln, lc))
                    for en, _, ec in ELEMS for ln, lc in LAYOUTS]
        variants += [("copy_%s" % en, en, kit.copy_variant(total[en] // 2)) for en, _, _ in ELEMS]
        ms = kit.interleaved(timer, [(key, make) for key, _, make in variants], sets, a.repeats)
        # the timed buffers give the restatement's bytes, also at this size (a corner of the first item of the first set)
        same = {}
        vecs, mask, x = first["in"]
        yy, xx = min(CROP[0], h - 1), min(CROP[1], w - 1)
        want_v, want_m = U.upsample(vecs[:yy + 1, :xx + 1], mask[:yy + 1, :xx + 1], np.ascontiguousarray(x[:, :yy + 1, :xx + 1]), f)
        for key, en, make in variants[:4]:
            make(sets[0])()
            got_v = sets[0]["out_vecs"].view(0, fine1 * 8).to_host((f * h, f * w, 2), np.float32)[:f * yy, :f * xx]
            got_m = sets[0]["out_mask"].view(0, fine1).to_host((f * h, f * w), np.uint8)[:f * yy, :f * xx]
            same[key] = bool(np.ascontiguousarray(got_v).tobytes() == np.ascontiguousarray(want_v[:f * yy, :f * xx]).tobytes()
                             and np.array_equal(got_m, want_m[:f * yy, :f * xx]))
        med = kit.median_ms(ms)
        for key, en, _ in variants:
            ref = "copy_%s" % en
            spread = kit.spread(ms[ref])
            line = {"key": "%s_%s" % (key, name), "coarse": [h, w], "factor": f, "fine": [f * h, f * w], "items": n,
                    **kit.ms_fields(ms[key]),
                    "repeats": a.repeats, "rotating_sets": SETS, "over_copy": round(med[key] / med[ref], 3),
                    "copy_spread": round(spread, 3), "bytes": int(total[en]), "TBps": round(total[en] / med[key] / 1e9, 3),
                    "device": nat.device_name()}
            if key in same:
                line.update({"within_copy_spread": bool(med[key] <= med[ref] * (1 + spread)), "equal_restatement": same[key]})
            report.line(line)
        del sets, q
        dev.empty_cache()
    report.write(a.out)


if __name__ == "__main__":
    main()
