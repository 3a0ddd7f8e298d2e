#!/usr/bin/env python
"""Point tracking on the device (K10, ofl_track.hip) against the host path it complements, one JSON line per entry.

  step_*      one step of N = 1e4, 1e5, 1e6 float points on a 1080p and a 4K ref-'s' field: DeviceFlow.track with resident
              points (DevicePoints in, DevicePoints out, the 4-byte outside counter read back) against Flow.track on the same
              data (field upload, sample, download, NumPy add), both by the wall clock around a device synchronise; and the
              kernel alone, HIP-event timed, as points per second.
  status_*    the same steps with get_valid_status (the device route runs valid_source() -- one gather over the field -- per
              call; the host route uploads the field twice and downloads the whole map).
  seq_*       N points through 16 x 1080p fields: DeviceFlowBatch.track_sequence (one launch) against 16 chained
              DeviceFlow.track calls on resident points and against the 16-call host loop.

No threshold: the host path is the baseline, the file records the ratios.  Every entry also records whether the device result
equals the host result bit for bit.

    python tools/bench_track.py [--iters 20] [--host-iters 3] [--out profiles/r09_track_bench.jsonl]
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
from bench_ops import timed
from bench_kit import wall

nat = of.native
COUNTS = (10 ** 4, 10 ** 5, 10 ** 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nat.ensure_device()
    lines = []

    def emit(e):
        e["device"] = nat.device_name()
        lines.append(json.dumps(e))
        print(lines[-1], flush=True)

    rng = np.random.default_rng(0)
    for name, h, w in (("1080p", 1080, 1920), ("4k", 2160, 3840)):
        flow = of.Flow.from_transforms([['rotation', w / 2, h / 2, -20], ['scaling', w / 3, h / 3, 0.95], ['translation', 12, -7]], (h, w), 's')
        d = flow.to_device()
        d.stats()
        for n in COUNTS:
            pts = rng.random((n, 2)) * (np.array([h, w]) - 1.0)
            dp = dev.DevicePoints.from_host(pts)
            t_dev = wall(lambda: d.track(dp), a.iters, warm=2)
            t_host = wall(lambda: flow.track(pts), a.host_iters, warm=1)
            out, outside = dev.DeviceBuffer(n * 16), dev.DeviceBuffer.zeros(16)
            k_s, _, _ = timed(lambda: dev.track_bilinear_launch(d.vecs.ptr, 1, d.shape, False, dp, d._stats_word(), None, False, out, None,
                                                                outside=outside), max(a.iters, 50), warm=5)
            emit({"key": "step_%s_n%d" % (name, n), "op": "DeviceFlow.track (resident points) vs Flow.track, ref 's', bilinear", "shape": [h, w],
                  "points": n, "device_route_wall_ms": round(t_dev * 1e3, 4), "host_route_wall_ms": round(t_host * 1e3, 3),
                  "speedup": round(t_host / t_dev, 1), "kernel_ms": round(k_s * 1e3, 4), "kernel_Mpoints_per_s": round(n / k_s / 1e6, 1),
                  "kernel": "track_bilinear_kernel<false>", "bit_identical": bool(np.array_equal(d.track(dp).to_host(), flow.track(pts))),
                  "note": "wall clock per call including a device synchronise; the device route reads back the 4-byte outside counter"})
            t_dev = wall(lambda: d.track(dp, get_valid_status=True), a.iters, warm=2)
            t_host = wall(lambda: flow.track(pts, get_valid_status=True), a.host_iters, warm=1)
            (gp, gs), (wp, ws) = d.track(dp, get_valid_status=True), flow.track(pts, get_valid_status=True)
            same = np.array_equal(gp.to_host(), wp) and np.array_equal(gs.to_host((n,), np.uint8), ws.view(np.uint8))
            emit({"key": "status_%s_n%d" % (name, n), "op": "the same with get_valid_status", "shape": [h, w], "points": n,
                  "device_route_wall_ms": round(t_dev * 1e3, 4), "host_route_wall_ms": round(t_host * 1e3, 3),
                  "speedup": round(t_host / t_dev, 1), "bit_identical": bool(same)})
            del dp, out
        del d, flow
        dev.empty_cache()

    # ---- 16 x 1080p: a slow rotation about the centre, points in the central disc (they stay inside the frame)
    h, w, B = 1080, 1920, 16
    mats = np.stack([of.utils.matrix_from_transforms([['rotation', (w - 1) / 2, (h - 1) / 2, 0.5 + 0.02 * i]]) for i in range(B)])
    batch = DeviceFlowBatch.from_matrices(mats, (h, w), 's')
    fields = [batch.field(i) for i in range(B)]
    hosts = batch.to_flows()
    for f in fields:
        f.stats()
    for n in (10 ** 5, 10 ** 6):
        r, phi = 0.45 * h * np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
        pts = np.stack([(h - 1) / 2 + r * np.sin(phi), (w - 1) / 2 + r * np.cos(phi)], axis=-1)
        dp = dev.DevicePoints.from_host(pts)

        def chained():
            p = dp
            for f in fields:
                p = f.track(p)
            return p

        def host_loop():
            p = pts
            for f in hosts:
                p = f.track(p)
            return p

        t_seq = wall(lambda: batch.track_sequence(dp), a.iters, warm=2)
        t_chain = wall(chained, a.iters, warm=2)
        t_host = wall(host_loop, a.host_iters, warm=1)
        got, lost = batch.track_sequence(dp)
        want = host_loop()
        emit({"key": "seq_16x1080p_n%d" % n, "op": "DeviceFlowBatch.track_sequence vs 16 DeviceFlow.track calls vs the 16-call host loop",
              "shape": [h, w], "fields": B, "points": n, "track_sequence_wall_ms": round(t_seq * 1e3, 4),
              "chained_device_calls_wall_ms": round(t_chain * 1e3, 4), "host_loop_wall_ms": round(t_host * 1e3, 2),
              "speedup_vs_chained": round(t_chain / t_seq, 2), "speedup_vs_host": round(t_host / t_seq, 1),
              "lost_points": int((lost.to_host((n,), np.int32) >= 0).sum()),
              "bit_identical": bool(np.array_equal(got.to_host(), want) and np.array_equal(chained().to_host(), want)),
              "kernel": "track_bilinear_kernel<true>"})
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
