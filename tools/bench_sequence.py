#!/usr/bin/env python
"""The sequence accumulation (K25, ofl_sequence.hip: L fields into one in a single launch) against (a) the chain it replaces
-- L - 1 ping-pong ofl_compose3_dev launches on the very same buffers -- and (b) a copy of the bytes the call must move, one
JSON line per variant.  Two sizes: L = 8 at 2160 x 3840 and L = 16 at 1080 x 1920, one sequence per launch, reference 't'
(sign -1: the walk runs from the last field to the first).  Two patterns:

  drift      the generator of tests/sequence_ref.py at full size: smooth fields of about 3 px (a 5 x 5 lattice of normal
             draws, bilinearly upsampled) plus a constant drift of (1.5, -1.0), a mask hole in every odd-indexed field, another
             seed per field and working set
  rotation   every field the same rotation by 30 / L degrees about the centre, all valid: after L steps the walk samples a
             grid turned by 30 degrees, the compose kernel's hard case

In ONE process and INTERLEAVED -- every repeat times each variant once, between two HIP events, as a run of calls long
enough to last 100 ms -- over rotating working sets (bench_ops.n_sets: no launch finds its bytes in the Infinity Cache):

  sequence            ofl_compose_sequence_dev writing out + mout                          (9 L read, 9 written, per pixel)
  sequence_lost       the same with lost_at                                                 (+ 4 written)
  sequence_partials   the same with the partial results                                     (+ 9 L written)
  sequence_all        partial results and lost_at
  chain               L - 1 launches of ofl_compose3_dev, fa = field k, fb = the accumulated field, no flag words, ping-pong
                      between two result fields                                             (27 (L - 1) per pixel)
  copy_plain          ofl_copy_dev moving 9 L + 9 bytes per pixel (half read, half written): the yardstick of `sequence`
  copy_all            ofl_copy_dev moving 18 L + 13 bytes per pixel: the yardstick of `sequence_all`
`over_chain` is median over median; `over_copy` = measured over the time the copy's rate gives the variant's own bytes (the
plain copy's rate without the partial results, the larger copy's with them); `chain_spread` and `copy_spread` =
(max - min) / median of the chain's and the plain copy's own repeats in this run, the margin below which a difference says
nothing on a shared machine.  `equals_chain`: the fused result and the chain's, vectors and masks, are the same bits at this
size; `valid_share`: the share of pixels still valid at the end.

    python tools/bench_sequence.py [--repeats 16] [--out profiles/r25_sequence_bench.jsonl]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np
import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from bench_ops import n_sets
from bench_consistency import smooth
from bench_photometric import runs
import bench_kit as kit

nat = of.native
SIGN, REF = -1, 't'
DRIFT = np.array([1.5, -1.0], np.float32)


def upload_drift(h, w, length, seed, flows, masks):
    lib, px = nat.load(), h * w
    hole = np.ones((h, w), np.uint8)
    hole[h // 4:h // 2, w // 8:w // 3] = 0
    nat.check(lib.ofl_memset(masks.ptr, 1, length * px, None))
    rng = np.random.default_rng(seed)
    for k in range(length):
        v = np.ascontiguousarray(smooth(rng, h, w, 3.0) + DRIFT, np.float32)
        nat.check(lib.ofl_upload(flows.ptr + k * px * 8, v.ctypes.data, px * 8, None))
        if k % 2:
            nat.check(lib.ofl_upload(masks.ptr + k * px, hole.ctypes.data, px, None))
        nat.check(lib.ofl_stream_sync(None))


def upload_rotation(h, w, length, seed, flows, masks):
    lib = nat.load()
    f = of.Flow.from_transforms([['rotation', (w - 1) / 2, (h - 1) / 2, 30.0 / length]], (h, w), REF)
    kit.replicate(flows, np.ascontiguousarray(f.vecs, np.float32), length)
    nat.check(lib.ofl_memset(masks.ptr, 1, length * h * w, None))


def main():
    a, lib, timer, report = kit.start(16)
    for name, h, w, length in (("4k_L8", 2160, 3840, 8), ("1080p_L16", 1080, 1920, 16)):
        px = h * w
        bpp = {"sequence": 9 * length + 9, "sequence_lost": 9 * length + 13, "sequence_partials": 18 * length + 9,
               "sequence_all": 18 * length + 13, "chain": 27 * (length - 1)}
        half_plain, half_all = px * bpp["sequence"] // 2, px * bpp["sequence_all"] // 2
        k = n_sets(px * bpp["sequence"])
        for pattern, upload in (("drift", upload_drift), ("rotation", upload_rotation)):
            sets = []
            for s in range(k):
                q = {"flows": dev.DeviceBuffer(length * px * 8), "masks": dev.DeviceBuffer(length * px),
                     "out": dev.DeviceBuffer(px * 8), "mout": dev.DeviceBuffer(px), "lost": dev.DeviceBuffer(px * 4),
                     "pv": dev.DeviceBuffer(length * px * 8), "pm": dev.DeviceBuffer(length * px),
                     "ping": (dev.DeviceBuffer(px * 8), dev.DeviceBuffer(px)), "pong": (dev.DeviceBuffer(px * 8), dev.DeviceBuffer(px)),
                     "c0": dev.DeviceBuffer(half_all), "c1": dev.DeviceBuffer(half_all)}
                upload(h, w, length, 1000 * s + 7, q["flows"], q["masks"])
                nat.check(lib.ofl_memset(q["c0"].ptr, 1, half_all, None))
                sets.append(q)
            dev.sync()

            def sequence(partials, lost):
                return lambda q: lambda: nat.check(lib.ofl_compose_sequence_dev(
                    q["flows"].ptr, q["masks"].ptr, SIGN, h, w, length, 1, q["out"].ptr, q["mout"].ptr,
                    q["pv"].ptr if partials else None, q["pm"].ptr if partials else None, q["lost"].ptr if lost else None,
                    nat.QUANT_OPENCV, None))

            def chain(q):
                def run():
                    acc = (q["flows"].ptr + (length - 1) * px * 8, q["masks"].ptr + (length - 1) * px)
                    for i, f in enumerate(range(length - 2, -1, -1)):
                        dst = q["ping"] if i % 2 == 0 else q["pong"]
                        nat.check(lib.ofl_compose3_dev(q["flows"].ptr + f * px * 8, q["masks"].ptr + f * px, acc[0], acc[1], SIGN, h, w, 1,
                                                       dst[0].ptr, dst[1].ptr, None, nat.QUANT_OPENCV, None))
                        acc = (dst[0].ptr, dst[1].ptr)
                return run

            table = [("sequence", sequence(False, False)), ("sequence_lost", sequence(False, True)),
                     ("sequence_partials", sequence(True, False)), ("sequence_all", sequence(True, True)), ("chain", chain),
                     ("copy_plain", kit.copy_variant(half_plain)), ("copy_all", kit.copy_variant(half_all))]
            variants, iters = [], {}
            for key, make in table:
                many, iters[key] = runs(timer, make, sets)
                variants.append((key, many))
            total = kit.interleaved(timer, variants, sets, a.repeats)
            ms = {key: [t / iters[key] for t in v] for key, v in total.items()}
            med = kit.median_ms(ms)
            # the fused result is the chain's, also at this size
            q = sets[0]
            sequence(False, False)(q)()
            chain(q)()
            last = q["ping"] if (length - 2) % 2 == 0 else q["pong"]
            mout = q["mout"].to_host((px,), np.uint8)
            same = bool(np.array_equal(q["out"].to_host((px * 2,), np.uint32), last[0].to_host((px * 2,), np.uint32)) and
                        np.array_equal(mout, last[1].to_host((px,), np.uint8)))
            rate = {"copy_plain": 2 * half_plain / med["copy_plain"], "copy_all": 2 * half_all / med["copy_all"]}   # bytes per ms
            bytes_of = {key: px * v for key, v in bpp.items()}
            bytes_of.update(copy_plain=2 * half_plain, copy_all=2 * half_all)
            common = {"shape": [h, w], "length": length, "pattern": pattern, "ref": REF, "repeats": a.repeats, "rotating_sets": k,
                      "chain_spread": round(kit.spread(ms["chain"]), 3), "copy_spread": round(kit.spread(ms["copy_plain"]), 3),
                      "equals_chain": same, "valid_share": round(float(mout.mean()), 4), "device": nat.device_name()}
            for key, _ in table:
                record = {"key": "%s_%s_%s" % (key, pattern, name), **common, **kit.ms_fields(ms[key]), "launches_per_repeat": iters[key],
                          "timed_ms_per_repeat_min": round(min(total[key]), 1), "bytes_moved": int(bytes_of[key]),
                          "GBps": round(bytes_of[key] / med[key] / 1e6, 1), "over_chain": round(med[key] / med["chain"], 3)}
                if key.startswith("sequence"):
                    yard = "copy_all" if key in ("sequence_partials", "sequence_all") else "copy_plain"
                    record.update(bytes_per_px=bpp[key], over_copy=round(med[key] / (bytes_of[key] / rate[yard]), 3))
                elif key == "chain":
                    record.update(bytes_per_px=bpp[key], over_copy=round(med[key] / (bytes_of[key] / rate["copy_plain"]), 3))
                report.line(record)
            del sets, q
            dev.empty_cache()
    report.write(a.out)


if __name__ == "__main__":
    main()
