#!/usr/bin/env python
"""Splatting (K20, ofl_splat.hip) against a device copy, one JSON line per variant and field.

Fields, all 's'-reference: `smooth` (a few pixels, slowly varying), `rotation` (30 degrees about the centre) and `contract`
(every pixel moves three quarters of the way to the centre: 4:1 in each axis, 16 sources per covered target).
Shapes: C = 3 float32 channels-last at 2160 x 3840, C = 128 float16 in both layouts at 136 x 240 and 270 x 480, and `project`
at 2160 x 3840.  Mode 'average' throughout, plus 'softmax' for the C = 3 case.

In ONE process and INTERLEAVED -- every repeat times one call of each variant, each call between two HIP events:

  splat_*      DeviceFlow.splat / project: the workspace clear, [the max pass,] accumulate, finish
  copy         ofl_copy_dev moving the same number of bytes as the splat's inputs and outputs: the tensor in and out, the
               field (9 B per pixel) and valid (1 B per pixel), half of them read and half written.  The int64 workspace
               traffic -- 8 (C + 1) bytes per pixel cleared, added to and read -- is NOT counted: it is the method's cost
  apply_image  the route the C = 3 splat replaces: DeviceFlow.apply_image of the same 's' field (K3, smooth field only)

No rate is fixed in advance: the yardstick is the copy in the same run.  Every line carries the median, the smallest and the
largest of its repeats; `over_copy` is median over median, `copy_spread` = (max - min) / median of the copy's own repeats and
`within_copy_spread` says whether the variant's median lies within that spread of the copy's.

    python tools/bench_splat.py [--repeats 8] [--out profiles/r19_splat_bench.jsonl]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np
import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
import bench_kit as kit

nat = of.native
F32 = np.float32


def fields(h, w):
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    smooth = np.stack([3 * np.sin(xx / 97.0 + yy / 131.0), 3 * np.cos(xx / 113.0 - yy / 89.0)], -1)
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    rot = np.stack([c * (xx - cx) - s * (yy - cy) + cx - xx, s * (xx - cx) + c * (yy - cy) + cy - yy], -1)
    contract = np.stack([0.75 * (cx - xx), 0.75 * (cy - yy)], -1)
    return (("smooth", smooth.astype(F32)), ("rotation", rot.astype(F32)), ("contract", contract.astype(F32)))


def main():
    a, lib, timer, report = kit.start(8)
    cases = (("c3_f32_hwc_4k", 3, 2160, 3840, np.float32, "hwc"), ("c128_f16_chw_136x240", 128, 136, 240, np.float16, "chw"),
             ("c128_f16_hwc_136x240", 128, 136, 240, np.float16, "hwc"), ("c128_f16_chw_270x480", 128, 270, 480, np.float16, "chw"),
             ("c128_f16_hwc_270x480", 128, 270, 480, np.float16, "hwc"), ("project_4k", 2, 2160, 3840, np.float32, "hwc"))
    for name, c, h, w, dt, layout in cases:
        px = h * w
        total = 2 * c * px * np.dtype(dt).itemsize + 10 * px
        rng = np.random.default_rng(7)
        project = name.startswith("project")
        shape = (c, h, w) if layout == "chw" else (h, w, c)
        tensor = None if project else dev.DeviceTensor.from_host((rng.standard_normal(shape, F32) * F32(3)).astype(dt), layout)
        image = dev.DeviceImage(tensor.buf, (h, w, c), np.float32) if c == 3 else None
        z = dev.DeviceBuffer.from_host((rng.standard_normal((h, w), F32) * F32(2))) if c == 3 else None
        q = {"c0": dev.DeviceBuffer(total // 2), "c1": dev.DeviceBuffer(total // 2)}
        nat.check(lib.ofl_memset(q["c0"].ptr, 1, q["c0"].nbytes, None))
        for fname, v in fields(h, w):
            flow = dev.DeviceFlow.from_host(v, 's')
            variants = [("copy", kit.copy_variant(total // 2))]
            if project:
                variants.append(("splat_average", lambda q, flow=flow: flow.project))
            else:
                variants.append(("splat_average", lambda q, flow=flow: (lambda: flow.splat(tensor, 'average'))))
            if c == 3:
                variants.append(("splat_softmax", lambda q, flow=flow: (lambda: flow.splat(tensor, 'softmax', importance=z, alpha=-1.0))))
                if fname == "smooth":
                    variants.append(("apply_image", lambda q, flow=flow: (lambda: flow.apply_image(image))))
            ms = kit.interleaved(timer, variants, [q], a.repeats)
            med, spread = kit.median_ms(ms), kit.spread(ms["copy"])
            for key, _ in variants:
                line = {"key": "%s_%s_%s" % (key, name, fname), "shape": [h, w], "channels": c, "dtype": np.dtype(dt).name, "layout": layout,
                        "field": fname, **kit.ms_fields(ms[key]), "repeats": a.repeats, "over_copy": round(med[key] / med["copy"], 3),
                        "copy_spread": round(spread, 3), "bytes": int(total), "workspace_bytes": int(8 * (c + 1) * px),
                        "TBps": round(total / med[key] / 1e9, 3), "device": nat.device_name()}
                if key != "copy":
                    line["within_copy_spread"] = bool(med[key] <= med["copy"] * (1 + spread))
                report.line(line)
            del flow
        del tensor, image, z, q
        dev.empty_cache()
    report.write(a.out)


if __name__ == "__main__":
    main()
