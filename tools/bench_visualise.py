#!/usr/bin/env python
"""Flow.visualise on the device (K7, ofl_visualise.hip), HIP-event timed over rotating working sets (bench_ops.py): 1080p
and 4K single fields and 16 x 1080p as one batch, each with the default scale (range select + render) and with a given
range_max (render only).  Rendered with show_mask=True so that the mask is read.  Prints ONE JSON line.

Algorithmic bytes per pixel: 8 per pass of the range select (three passes: 24) and 8 + 1 + 3 for the render (vectors,
mask, RGB bytes) -- 36 with the default scale, 12 with a given one.

    python tools/bench_visualise.py [--iters 30]
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
from bench_ops import n_sets, timed, entry

SELECT_BPP, RENDER_BPP = 3 * 8, 8 + 1 + 3


def field(h, w, seed):
    y = np.arange(h, dtype=np.float32)[:, None]
    x = np.arange(w, dtype=np.float32)[None, :]
    v = np.empty((h, w, 2), np.float32)
    v[..., 0] = 3 * np.sin(x / 37.0 + seed) + 0.5 * np.cos(y / 23.0)
    v[..., 1] = 2 * np.cos(y / 29.0 - seed) - 0.7 * np.sin(x / 41.0)
    return v


def mask(h, w):
    m = np.ones((h, w), bool)
    m[h // 4: h // 2, w // 3: w // 2] = False
    return m


def batch_of(n, h, w, seed):
    b = DeviceFlowBatch(n, (h, w), 't')
    lib, px = of.native.load(), h * w
    v, m = field(h, w, seed), mask(h, w).view(np.uint8)
    for i in range(n):
        of.native.check(lib.ofl_upload(b.vecs.ptr + i * px * 8, v.ctypes.data, px * 8, None))
        of.native.check(lib.ofl_upload(b.mask.ptr + i * px, m.ctypes.data, px, None))
    of.native.check(lib.ofl_stream_sync(None))
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    of.native.ensure_device()
    res = {"device": of.native.device_name(), "iters": a.iters, "show_mask": True, "entries": []}
    cases = [("1080p", 1, 1080, 1920), ("4k", 1, 2160, 3840), ("16x1080p", 16, 1080, 1920)]
    for name, n, h, w in cases:
        px = n * h * w
        k = n_sets(RENDER_BPP * px)
        if n == 1:
            objs = [dev.DeviceFlow.from_host(field(h, w, s), 't', mask(h, w)) for s in range(k)]
        else:
            objs = [batch_of(n, h, w, s) for s in range(k)]
        want = {}
        for key, rm, bpp in (("default", None, SELECT_BPP + RENDER_BPP), ("given", 2.5, RENDER_BPP)):
            fns = [(lambda o=o, rm=rm: o.visualise('rgb', True, False, rm)) for o in objs]
            dev_s, wall_s, sets = timed(fns, a.iters)
            e = entry("vis_%s_%s" % (name, key), "visualise rgb, range %s" % key, (h, w), bpp, dev_s, wall_s, sets,
                      units=n, kernel="vis_hist x3 + vis_select x3 + vis_render" if rm is None else "vis_render")
            res["entries"].append(e)
            want[key] = objs[0].visualise('rgb', True, False, rm).to_host()
        # the select alone (one launch sequence for the whole batch)
        h_, w_ = (h, w)
        outs = [dev.DeviceBuffer(4 * n) for _ in objs]
        fns = [(lambda o=o, r=r: dev.visualise_range_launch(o.vecs, h_, w_, n, r)) for o, r in zip(objs, outs)]
        dev_s, wall_s, sets = timed(fns, a.iters)
        res["entries"].append(entry("vis_%s_select" % name, "range select", (h, w), SELECT_BPP, dev_s, wall_s, sets, units=n,
                                    kernel="vis_init + vis_hist x3 + vis_select x3"))
        res["entries"][-1]["range_max"] = float(outs[0].to_host((n,), np.float32)[0])
        assert want["default"].shape == (((h, w, 3)) if n == 1 else (n, h, w, 3))
        del objs, outs
        dev.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
