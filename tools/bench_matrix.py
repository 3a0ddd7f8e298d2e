#!/usr/bin/env python
"""Flow.matrix on the device (K8, ofl_fit.hip) over rotating working sets (bench_ops.py), 1080p and 4K: every pass alone,
HIP-event timed (the entries only enqueue work), and DeviceFlow.matrix end to end for every dof x method, wall-clock timed
(it reads its sums back between passes, so the wall time is the time a caller waits).  The field is an affine motion with
+-2.5 px of noise and a mask with a hole, so that RANSAC iterates and the gate rejects.  One JSON line per entry.

Algorithmic bytes per pixel: 8 + 1 per read of the field (vectors, mask); the median makes three reads per three models.

    python tools/bench_matrix.py [--iters 20] [--out profiles/r07_matrix_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np
import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev, matrix_fit
from bench_ops import n_sets, timed, entry, affine_flow

READ_BPP = 8 + 1
COMBOS = [(4, 'ransac'), (4, 'lmeds'), (6, 'ransac'), (6, 'lmeds'), (8, 'lms'), (8, 'ransac'), (8, 'lmeds')]
TRANSFORMS = [['translation', 20, 10], ['rotation', 200, 200, 30], ['scaling', 100, 100, 1.1]]


def field(h, w, seed):
    v = affine_flow(TRANSFORMS, h, w, 's')
    v += ((np.random.default_rng(seed).random((h, w, 2)) - .5) * 5).astype(np.float32)
    m = np.ones((h, w), bool)
    m[h // 4: h // 2, w // 3: w // 2] = False
    return v, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    of.native.ensure_device()
    lib = of.native.load()
    lines = []

    def emit(e):
        e["device"] = of.native.device_name()
        lines.append(json.dumps(e))
        print(lines[-1], flush=True)

    M = of.utils.matrix_from_transforms(TRANSFORMS)
    for name, h, w in (("1080p", 1080, 1920), ("4k", 2160, 3840)):
        k = n_sets(READ_BPP * h * w)
        flows = []
        for s in range(k):
            v, m = field(h, w, s)
            flows.append(dev.DeviceFlow.from_host(v, 's', m))
        fits = [dev.FitField(f.vecs, f.mask, f.shape, 1) for f in flows]
        gate = np.ascontiguousarray(M)
        norm = np.array([w / 2.0, h / 2.0, 2.0 / w, w / 2.0, h / 2.0, 2.0 / w])
        origin = np.array(fits[0].origin)
        models32 = np.ascontiguousarray(np.repeat(M[None], 32, 0) + 1e-6 * np.arange(32)[:, None, None])
        n_px = h * w
        p = lambda arr: arr.ctypes.data
        thr = np.float32(9.0)
        passes = [
            ("moments", "fit_sum<moments> + fit_finish", READ_BPP,
             lambda F: lib.ofl_fit_moments_dev(*F._field(), 1, p(origin), None, thr, F.ws.ptr, F.ws.nbytes, F.out.ptr, None)),
            ("moments_gated", "fit_sum<moments> + fit_finish", READ_BPP,
             lambda F: lib.ofl_fit_moments_dev(*F._field(), 1, p(origin), p(gate), thr, F.ws.ptr, F.ws.nbytes, F.out.ptr, None)),
            ("dlt_gated", "fit_sum<dlt> + fit_finish", READ_BPP,
             lambda F: lib.ofl_fit_dlt_dev(*F._field(), 1, p(norm), p(gate), thr, F.ws.ptr, F.ws.nbytes, F.out.ptr, None)),
            ("gn_gated", "fit_sum<gn> + fit_finish", READ_BPP,
             lambda F: lib.ofl_fit_gn_dev(*F._field(), 1, p(norm), p(gate), p(gate), thr, F.ws.ptr, F.ws.nbytes, F.out.ptr, None)),
            ("score_32", "fit_score", READ_BPP,
             lambda F: lib.ofl_fit_score_dev(*F._field(), 1, p(models32), 32, thr, F.out.ptr, None)),
            ("median_3", "fit_med_init + (fit_med_hist + fit_med_select) x3", 3 * READ_BPP,
             lambda F: lib.ofl_fit_median_dev(*F._field(), 1, p(models32), 3, (n_px - 1) // 2, n_px // 2, F.ws.ptr, F.ws.nbytes, F.out.ptr, None)),
            ("index", "fit_count + fit_scan", READ_BPP,
             lambda F: lib.ofl_fit_index_dev(*F._field(), F.ws.ptr, F.ws.nbytes, None)),
        ]
        for key, kernel, bpp, call in passes:
            fns = [(lambda F=F: of.native.check(call(F))) for F in fits]
            dev_s, wall_s, sets = timed(fns, a.iters)
            emit(entry("fit_%s_%s" % (name, key), key, (h, w), bpp, dev_s, wall_s, sets, kernel=kernel))
        for dof, method in COMBOS:
            for f in flows[:2]:
                f.matrix(dof, method)
            t0 = time.perf_counter()
            for i in range(a.iters):
                out = flows[i % k].matrix(dof, method)
            wall = (time.perf_counter() - t0) / a.iters
            e = {"key": "matrix_%s_dof%d_%s" % (name, dof, method), "op": "DeviceFlow.matrix end to end", "shape": [h, w],
                 "wall_ms": round(wall * 1e3, 3), "rotating_sets": k, "max_abs_error": float(np.abs(out - M).max()),
                 "note": "wall clock including the read-backs between passes"}
            emit(e)
        del flows, fits
        dev.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
