#!/usr/bin/env python
"""Taking and handing out device-resident fields (K11, ofl_interop.hip) at 1080p, 4K and 16 x 1080p, one JSON line per entry.

  import_* export_*   the kernels alone, HIP-event timed over rotating working sets of at least 3 x 256 MiB (bench_ops.n_sets:
                      no launch finds its bytes in the Infinity Cache): float32 interleaved, float32 planar, float16 planar and
                      a column-strided float32 view (every second column of a parent twice as wide).  Each as a share of the rate
                      at which ofl_copy_dev moves the same number of bytes (read + written), timed in this run.
  roundtrip_*         DeviceFlow.from_external + export end to end (planar float16 in, planar float16 out, the finiteness check
                      on) against the only route there was before: the producer's buffer downloaded to the host, converted there,
                      DeviceFlow.from_host, to_host, converted back and uploaded.  Wall clock around a device synchronise.

The "foreign" memory is the library's own DeviceBuffer behind an object that exposes __cuda_array_interface__.

    python tools/bench_interop.py [--iters 20] [--host-iters 3] [--out profiles/r10_interop_bench.jsonl]
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
from bench_ops import n_sets, timed
from bench_build import copy_rate
from bench_kit import wall

nat = of.native


class Foreign:
    """a device buffer as another framework would present it"""

    def __init__(self, buf, shape, typestr, strides=None):
        self.buf = buf
        self.__cuda_array_interface__ = {"version": 3, "shape": tuple(shape), "typestr": typestr, "data": (buf.ptr, False),
                                         "strides": strides, "stream": None}


def filled(nbytes):
    buf = dev.DeviceBuffer(nbytes)
    nat.check(nat.load().ofl_memset(buf.ptr, 0x3c, nbytes, None))       # finite in every element type
    return buf


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

    def kernel_entry(key, op, n, h, w, moved, s, copy_s, sets, **more):
        e = {"key": key, "op": op, "fields": n, "shape": [h, w], "bytes_moved": int(moved), "device_ms": round(s * 1e3, 4),
             "GBps": round(moved / s / 1e9, 1), "copy_same_bytes_ms": round(copy_s * 1e3, 4),
             "share_of_copy_rate": round(copy_s / s, 3), "rotating_sets": sets}
        e.update(more)
        emit(e)

    for name, n, h, w in (("1080p", 1, 1080, 1920), ("4k", 1, 2160, 3840), ("16x1080p", 16, 1080, 1920)):
        px = n * h * w
        # ---- import: (label, element code, item size, strides (field, channel, row, column), source bytes, bytes read)
        cases = (("f32_interleaved", nat.EL_F32, 4, (h * w * 2, 1, w * 2, 2), 8 * px, 8 * px),
                 ("f32_planar", nat.EL_F32, 4, (2 * h * w, h * w, w, 1), 8 * px, 8 * px),
                 ("f16_planar", nat.EL_F16, 2, (2 * h * w, h * w, w, 1), 4 * px, 4 * px),
                 ("f32_planar_every_2nd_column", nat.EL_F32, 4, (4 * h * w, 2 * h * w, 2 * w, 2), 16 * px, 16 * px))
        for label, elem, item, strides, src_bytes, read in cases:
            moved = read + 9 * px                               # + 8 B vectors and 1 B mask written per pixel
            k = n_sets(src_bytes + 9 * px)
            sets = [(filled(src_bytes), dev.DeviceBuffer(8 * px), dev.DeviceBuffer(px)) for _ in range(k)]
            copy_s, _ = copy_rate(moved, a.iters)
            s, _, used = timed([(lambda t=t: dev.import_flow_launch(t[0].ptr, elem, strides, n, h, w, None, None, t[1], t[2], None))
                                for t in sets], max(a.iters, 3 * k))
            kernel_entry("import_%s_%s" % (name, label), "ofl_import_flow_dev, %s, no mask source, no counters" % label, n, h, w, moved,
                         s, copy_s, used, kernel="import_flow_kernel",
                         note="bytes: the cache lines the source view touches + 9 B per pixel written" if "2nd" in label else
                              "bytes: source read + 9 B per pixel written")
            del sets
            dev.empty_cache()
        # ---- export: 8 B per pixel read, the destination written
        for label, elem, item, planar in (("f32_interleaved", nat.EL_F32, 4, 0), ("f32_planar", nat.EL_F32, 4, 1),
                                          ("f16_planar", nat.EL_F16, 2, 1)):
            moved = 8 * px + 2 * item * px
            k = n_sets(moved)
            sets = [(filled(8 * px), dev.DeviceBuffer(2 * item * px)) for _ in range(k)]
            copy_s, _ = copy_rate(moved, a.iters)
            s, _, used = timed([(lambda t=t: nat.check(lib.ofl_export_flow_dev(t[0].ptr, n, h, w, elem, planar, t[1].ptr, None)))
                                for t in sets], max(a.iters, 3 * k))
            kernel_entry("export_%s_%s" % (name, label), "ofl_export_flow_dev, %s" % label, n, h, w, moved, s, copy_s, used,
                         kernel="export_flow_kernel")
            del sets
            dev.empty_cache()

    # ---- end to end: a planar float16 field of a network in, the same out
    for name, h, w in (("1080p", 1080, 1920), ("4k", 2160, 3840)):
        rng = np.random.default_rng(0)
        host = (rng.standard_normal((2, h, w)) * 5).astype(np.float16)
        src = Foreign(dev.DeviceBuffer.from_host(host), (2, h, w), '<f2')

        def resident():
            return dev.DeviceFlow.from_external(src, 't').export('chw', 'float16')

        def through_the_host():
            down = src.buf.to_host((2, h, w), np.float16)
            f = dev.DeviceFlow.from_host(np.ascontiguousarray(np.moveaxis(down.astype(np.float32), 0, -1)), 't')
            v, _ = f.to_host()
            return dev.DeviceBuffer.from_host(np.ascontiguousarray(np.moveaxis(v, -1, 0)).astype(np.float16))

        same = bool(np.array_equal(resident().to_host().view(np.uint16), through_the_host().to_host((2, h, w), np.uint16)))
        t_dev = wall(resident, a.iters, warm=3)
        t_host = wall(through_the_host, a.host_iters, warm=1)
        emit({"key": "roundtrip_%s_f16_planar" % name, "op": "from_external + export vs download, from_host, to_host, upload",
              "shape": [h, w], "resident_wall_ms": round(t_dev * 1e3, 4), "host_route_wall_ms": round(t_host * 1e3, 2),
              "speedup": round(t_host / t_dev, 1), "bit_identical": same,
              "note": "wall clock per call including a device synchronise; the resident route includes the finiteness read-back"})
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
