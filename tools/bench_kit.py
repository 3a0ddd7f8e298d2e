"""What the per-family benchmark tools (bench_consistency, _error, _fill, _median, _upsample, _correlation) share: the
command line, the two-event timer, the replication of one generated field into the slots of a batch, the interleaved
loop over rotating working sets, the arithmetic of a line's timing fields and the printing and writing of the JSON lines.
The generators, the variant tables, the checks against the restatements and the host routes are the tools' own.
"""
import argparse
import ctypes
import json
import time

import numpy as np
import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev

nat = of.native


def start(repeats):
    """--repeats (default `repeats`) and --out parsed, the device selected -> (arguments, library, timer, report)"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=repeats)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nat.ensure_device()
    return a, nat.load(), event_timer(), Report()


def event_timer():
    """-> timer(call): the device milliseconds of call() between two HIP events.  What call() returns -- buffers a wrapper
    allocated -- lives until the events have been read."""
    lib = nat.load()
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    nat.check(lib.ofl_event_create(ctypes.byref(e0)))
    nat.check(lib.ofl_event_create(ctypes.byref(e1)))

    def timer(call):
        nat.check(lib.ofl_event_record(e0, None))
        keep = call()
        nat.check(lib.ofl_event_record(e1, None))
        nat.check(lib.ofl_event_sync(e1))
        ms = ctypes.c_float()
        nat.check(lib.ofl_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
        del keep
        return ms.value
    return timer


def replicate(buf, arr, n):
    """a host array uploaded once and copied on the device into n slots back to back, from the start of `buf` -> buf"""
    arr = np.ascontiguousarray(arr)
    lib = nat.load()
    nat.check(lib.ofl_upload(buf.ptr, arr.ctypes.data, arr.nbytes, None))
    nat.check(lib.ofl_stream_sync(None))
    for i in range(1, n):
        nat.check(lib.ofl_copy_dev(buf.ptr + i * arr.nbytes, buf.ptr, arr.nbytes, None))
    return buf


def copy_variant(nbytes):
    """the yardstick of every tool: ofl_copy_dev moving nbytes from a working set's "c0" to its "c1" """
    lib = nat.load()
    return lambda q: (lambda: nat.check(lib.ofl_copy_dev(q["c1"].ptr, q["c0"].ptr, nbytes, None)))


def interleaved(timer, variants, sets, repeats):
    """Every repeat times one call of each variant, on the working sets in rotation.  variants: (key, make) pairs, where
    make(working set) gives the call to time (it checks its own return code) -> {key: [milliseconds per repeat]}"""
    ms = {key: [] for key, _ in variants}
    for r in range(-2, repeats):                      # two warm-up rounds over every variant
        for key, make in variants:
            t = timer(make(sets[r % len(sets)]))
            if r >= 0:
                ms[key].append(t)
    return ms


def median_ms(ms):
    return {key: float(np.median(v)) for key, v in ms.items()}


def spread(v):
    """(max - min) / median of one variant's repeats: the margin below which a difference says nothing on a shared machine"""
    return (max(v) - min(v)) / float(np.median(v))


def ms_fields(v):
    """the three timing fields every line carries, in their order"""
    return {"device_ms_median": round(float(np.median(v)), 4), "device_ms_min": round(min(v), 4), "device_ms_max": round(max(v), 4)}


def wall(fn, iters, warm):
    """seconds per call by the host clock, every call followed by a device synchronise (bench_track, bench_build, bench_interop)"""
    for _ in range(warm):
        fn()
        dev.sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
        dev.sync()
    return (time.perf_counter() - t0) / iters


class Report:
    """the JSON lines of one run: printed as they come, written to --out at the end"""

    def __init__(self):
        self.lines = []

    def line(self, record):
        self.lines.append(json.dumps(record))
        print(self.lines[-1], flush=True)

    def write(self, path):
        if path:
            with open(path, "w") as fh:
                fh.write("\n".join(self.lines) + "\n")
