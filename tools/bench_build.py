#!/usr/bin/env python
"""Building, scaling, padding and cropping fields on the device (K9, ofl_build.hip) at 1080p and 4K, one JSON line per entry.

  build_*        DeviceFlow.from_transforms end to end (host matrix, 72-byte upload, constructor kernel, mask memset) against
                 the route it replaces, Flow.from_transforms(...).to_device() (NumPy build on the host + upload), both timed
                 in this run by the wall clock around a device synchronise; and the constructor kernel alone, HIP-event timed,
                 for an affine and a projective matrix, as a share of the rate at which ofl_copy_dev WRITES the same bytes.
  batch_*        DeviceFlowBatch.from_matrices: 16 x 1080p in one launch against 16 single launches.
  scale_* pad_* crop_*   each against ofl_copy_dev of the same number of bytes (read + written), as a share of its rate.

Kernels rotate over distinct working sets of at least 3 x 256 MiB (bench_ops.n_sets), so that no launch finds its bytes in
the Infinity Cache.

    python tools/bench_build.py [--iters 20] [--host-iters 3] [--out profiles/r08_device_build_bench.jsonl]
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
from bench_kit import wall

nat = of.native
TRANSFORMS = [['rotation', 960, 540, -30], ['scaling', 400, 300, 0.9], ['translation', 20, 10]]
PROJECTIVE = np.array([[1.02, 0.01, 3.0], [-0.02, 0.98, -2.0], [1e-5, -2e-5, 1.0]])


def copy_rate(nbytes_moved, iters):
    """ofl_copy_dev moving `nbytes_moved` in all (half read, half written) -> (seconds, sets)"""
    lib, half = nat.load(), nbytes_moved // 2
    k = n_sets(nbytes_moved)
    bufs = [(dev.DeviceBuffer(half), dev.DeviceBuffer(half)) for _ in range(k)]
    for a, _ in bufs:
        nat.check(lib.ofl_memset(a.ptr, 1, half, None))
    s, _, sets = timed([(lambda a=a, b=b: nat.check(lib.ofl_copy_dev(b.ptr, a.ptr, half, None))) for a, b in bufs], max(iters, 3 * k))
    return s, sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nat.ensure_device()
    lib = nat.load()
    lines = []

    def emit(e):
        e["device"] = nat.device_name()
        lines.append(json.dumps(e))
        print(lines[-1], flush=True)

    def kernel_entry(key, op, shape, moved, s, copy_s, sets, **more):
        e = {"key": key, "op": op, "shape": list(shape), "bytes_moved": int(moved), "device_ms": round(s * 1e3, 4),
             "GBps": round(moved / s / 1e9, 1), "copy_same_bytes_ms": round(copy_s * 1e3, 4),
             "share_of_copy_rate": round(copy_s / s, 3), "rotating_sets": sets}
        e.update(more)
        emit(e)

    for name, h, w in (("4k", 2160, 3840), ("1080p", 1080, 1920)):
        shape, n = (h, w), h * w
        # ---- the constructor end to end against the route it replaces
        t_dev = wall(lambda: dev.DeviceFlow.from_transforms(TRANSFORMS, shape, 't'), a.iters, warm=3)
        t_host = wall(lambda: of.Flow.from_transforms(TRANSFORMS, shape, 't').to_device(), a.host_iters, warm=1)
        got = dev.DeviceFlow.from_transforms(TRANSFORMS, shape, 't').to_host()[0]
        want = of.Flow.from_transforms(TRANSFORMS, shape, 't').vecs
        emit({"key": "build_%s_from_transforms" % name, "op": "DeviceFlow.from_transforms vs Flow.from_transforms(...).to_device()",
              "shape": [h, w], "device_route_wall_ms": round(t_dev * 1e3, 4), "host_route_wall_ms": round(t_host * 1e3, 2),
              "speedup": round(t_host / t_dev, 1), "bit_identical": bool(np.array_equal(got.view(np.uint32), want.view(np.uint32))),
              "note": "wall clock per call including a device synchronise; both routes end with the field and an all-ones mask in HBM"})
        del got, want
        # ---- the constructor kernel alone: 8 B/px written, nothing read; the copy that WRITES 8 B/px moves 16
        k = n_sets(8 * n)
        outs = [dev.DeviceBuffer(8 * n) for _ in range(k)]
        copy_s, _ = copy_rate(16 * n, a.iters)
        for label, m in (("affine", dev.matrix_args(of.utils.matrix_from_transforms(TRANSFORMS), shape, 't')[0]),
                         ("projective", np.ascontiguousarray(PROJECTIVE))):
            mats = dev.DeviceBuffer.from_host(m)
            s, _, sets = timed([(lambda o=o: dev.flow_from_matrix_launch(mats, 1, -1, shape, o)) for o in outs], max(a.iters, 3 * k))
            kernel_entry("build_%s_kernel_%s" % (name, label), "ofl_flow_from_matrix_dev, %s matrix" % label, shape, 8 * n, s, copy_s, sets,
                         kernel="flow_from_matrix_kernel", share_of_copy_write_rate=round(copy_s / s, 3),
                         note="store-only: copy_same_bytes_ms is ofl_copy_dev writing the same 8 B/px (and reading 8 more)")
        del outs
        # ---- scale, pad, crop against a copy of the same bytes
        srcs = [dev.DeviceFlow.from_transforms(TRANSFORMS, shape, 't') for _ in range(n_sets(16 * n))]
        copy_s, _ = copy_rate(16 * n, a.iters)
        for label, fn in (("mul_f32", lambda d: d * 0.9), ("div_f32", lambda d: d / 0.9), ("mul_f64", lambda d: d * [0.9, 1.1]),
                          ("div_f64", lambda d: d / [0.9, 1.1])):
            s, _, sets = timed([(lambda d=d: fn(d)) for d in srcs], max(a.iters, 3 * len(srcs)))
            kernel_entry("scale_%s_%s" % (name, label), "DeviceFlow scaling (%s)" % label, shape, 16 * n, s, copy_s, sets, kernel="scale_kernel")
        p = [h // 8, h // 8, w // 8, w // 8]
        no = (h + p[0] + p[1]) * (w + p[2] + p[3])
        for mode in ('constant', 'edge', 'symmetric'):
            moved = 9 * no + 9 * n
            copy_p, _ = copy_rate(moved, a.iters)
            s, _, sets = timed([(lambda d=d: d.pad(p, mode)) for d in srcs], max(a.iters, 3 * len(srcs)))
            kernel_entry("pad_%s_%s" % (name, mode), "DeviceFlow.pad %s, an eighth of the frame on every side" % mode, shape, moved, s, copy_p, sets,
                         kernel="remap_kernel<PadMap>", note="bytes: 9 B per output px written + 9 B per source px read")
        for label, item in (("centre", (slice(h // 8, h - h // 8), slice(w // 8, w - w // 8))), ("flip", (slice(None, None, -1), slice(None, None, -1))),
                            ("stride2", (slice(None, None, 2), slice(None, None, 2)))):
            (_, _, rows), (_, _, cols) = dev.crop_args(item, shape)
            moved = 18 * rows * cols
            copy_c, _ = copy_rate(moved, a.iters)
            s, _, sets = timed([(lambda d=d: d[item]) for d in srcs], max(a.iters, 3 * len(srcs)))
            kernel_entry("crop_%s_%s" % (name, label), "DeviceFlow[...] %s" % label, shape, moved, s, copy_c, sets, kernel="remap_kernel<CropMap>",
                         note="bytes: 9 B per output px read + 9 B written (a strided read fetches more than it uses)")
        del srcs
        dev.empty_cache()

    # ---- 16 x 1080p: one launch against 16
    h, w, B = 1080, 1920, 16
    n = h * w
    mats = np.stack([dev.matrix_args(of.utils.matrix_from_transforms([['rotation', w / 2, h / 2, -30 + 4 * i], ['translation', i, -i]]), (h, w), 't')[0]
                     for i in range(B)])
    dm = dev.DeviceBuffer.from_host(mats)
    singles = [dev._BufferView(dm.ptr + 72 * i, 72) for i in range(B)]
    k = n_sets(B * 8 * n)
    outs = [dev.DeviceBuffer(B * 8 * n) for _ in range(k)]
    s1, _, sets = timed([(lambda o=o: dev.flow_from_matrix_launch(dm, B, -1, (h, w), o)) for o in outs], max(a.iters, 3 * k))

    def sixteen(o):
        for i in range(B):
            dev.flow_from_matrix_launch(singles[i], 1, -1, (h, w), dev._BufferView(o.ptr + i * 8 * n, 8 * n))
    s16, _, _ = timed([(lambda o=o: sixteen(o)) for o in outs], max(a.iters, 3 * k))
    emit({"key": "batch_16x1080p_from_matrices", "op": "ofl_flow_from_matrix_dev, 16 fields of 1080p", "shape": [h, w], "fields": B,
          "bytes_moved": B * 8 * n, "one_launch_ms": round(s1 * 1e3, 4), "sixteen_launches_ms": round(s16 * 1e3, 4),
          "GBps_one_launch": round(B * 8 * n / s1 / 1e9, 1), "speedup": round(s16 / s1, 2), "rotating_sets": sets, "kernel": "flow_from_matrix_kernel"})
    t_b = wall(lambda: DeviceFlowBatch.from_matrices(mats, (h, w), 's'), a.iters, warm=3)
    emit({"key": "batch_16x1080p_from_matrices_wall", "op": "DeviceFlowBatch.from_matrices end to end (one upload, one launch, mask memset)",
          "shape": [h, w], "fields": B, "wall_ms": round(t_b * 1e3, 4)})
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
