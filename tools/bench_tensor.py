#!/usr/bin/env python
"""Warping many-channel float tensors (K12, ofl_tensor.hip), one JSON line per entry: float16 (64, 1080, 1920), float32
(128, 540, 960) and 16 x (32, 540, 960) float16 with one field per item, each in both layouts.

  device_ms            ofl_gather_tensor_dev with validity, HIP-event timed over rotating working sets of at least 3 x 256 MiB
                       (bench_ops.n_sets: no launch finds its bytes in the Infinity Cache).  The field is a 10-degree rotation.
  copy_same_bytes_ms   ofl_copy_dev moving the same number of bytes (2 N C H W e + 8 B/px of field + 2 B/px of masks), timed in
                       this run.
  parent_route_ms      the only route there was before: groups of 6 float32 channels through ofl_permute_image_dev, the image
                       gather K1 and ofl_permute_image_dev back -- on a float32 tensor of the same shape, as that route takes
                       no 16-bit storage.  3 launches per group, event timed, host launch gaps included.

    python tools/bench_tensor.py [--iters 10] [--out profiles/r11_tensor_bench.jsonl]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np
import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
from bench_ops import n_sets, timed
from bench_build import copy_rate

nat = of.native


def filled(nbytes):
    buf = dev.DeviceBuffer(nbytes)
    nat.check(nat.load().ofl_memset(buf.ptr, 0x3c, nbytes, None))       # finite in every element type
    return buf


def parent_route(src, dst, layout, n, c, h, w, flows, fmasks, per_item):
    """float32 only: per item and group of up to 6 channels permute -> K1 -> permute"""
    lib = nat.load()
    px = h * w
    for i in range(n):
        flow = flows.view(i * px * 8, px * 8) if per_item else flows
        fmask = fmasks.view(i * px, px) if per_item else fmasks
        for c0 in range(0, c, 6):
            cg = min(6, c - c0)
            if layout == 'chw':
                off, st = ((i * c + c0) * px) * 4, (px, w, 1)
            else:
                off, st = (i * px * c + c0) * 4, (1, w * c, c)
            img = dev.DeviceImage(dev.DeviceBuffer(px * cg * 4), (h, w, cg), np.float32)
            nat.check(lib.ofl_permute_image_dev(src.ptr + off, img.buf.ptr, 4, cg, h, w, st[0], st[1], st[2], 1, None))
            out, _ = dev.gather_bilinear(img, flow, (h, w), -1, fmask=fmask, want_valid=True)
            nat.check(lib.ofl_permute_image_dev(out.buf.ptr, dst.ptr + off, 4, cg, h, w, st[0], st[1], st[2], 0, None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nat.ensure_device()
    lines = []
    for key, dtype, n, c, h, w, per_item in (("f16_64x1080p", 'float16', 1, 64, 1080, 1920, False),
                                             ("f32_128x540p", 'float32', 1, 128, 540, 960, False),
                                             ("f16_16x32x540p", 'float16', 16, 32, 540, 960, True)):
        e, px, nf = (4 if dtype == 'float32' else 2), h * w, (n if per_item else 1)
        m = of.utils.matrix_from_transforms([['rotation', w / 2, h / 2, 10]])
        if per_item:
            b = DeviceFlowBatch.from_matrices(np.stack([m] * n), (h, w), 't')
            flows, fmasks = b.vecs, b.mask
        else:
            f = dev.DeviceFlow.from_matrix(m, (h, w), 't')
            flows, fmasks = f.vecs, f.mask
        moved = 2 * n * c * px * e + nf * px * 8 + 2 * nf * px
        copy_s, _ = copy_rate(moved, a.iters)
        for layout in ('chw', 'hwc'):
            k = n_sets(moved)
            sets = [filled(n * c * px * e) for _ in range(k)]
            s, _, used = timed([(lambda t=t: dev.gather_tensor(t, dtype, layout, n, c, h, w, flows, not per_item, -1, fmask=fmasks,
                                                               want_valid=True)) for t in sets], max(a.iters, 3 * k))
            del sets
            dev.empty_cache()
            src32, dst32 = filled(n * c * px * 4), dev.DeviceBuffer(n * c * px * 4)
            ps, _, _ = timed(lambda: parent_route(src32, dst32, layout, n, c, h, w, flows, fmasks, per_item), 3, warm=1)
            del src32, dst32
            dev.empty_cache()
            line = {"key": "tensor_%s_%s" % (key, layout), "op": "ofl_gather_tensor_dev with validity, %s %s" % (dtype, layout),
                    "items": n, "channels": c, "shape": [h, w], "bytes_moved": int(moved), "device_ms": round(s * 1e3, 4),
                    "GBps": round(moved / s / 1e9, 1), "copy_same_bytes_ms": round(copy_s * 1e3, 4),
                    "share_of_copy_rate": round(copy_s / s, 3), "rotating_sets": used, "parent_route_ms": round(ps * 1e3, 3),
                    "parent_route_over_tensor_kernel": round(ps / s, 2),
                    "note": "parent route: float32 tensor of the same shape, groups of 6 channels, permute + K1 + permute, one "
                            "working set, host launch gaps included", "device": nat.device_name()}
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
