#!/usr/bin/env python
"""bench.py -- headline benchmark: Flow.combine_with(mode=3) at 2160 x 3840 float32 (BASELINE.json).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is one pass of the hot path over one synthetic batch of flow-field pairs that is already resident
in HBM: one launch of the fused compose kernel (ofl_compose3_dev, with the reference's zero-flow
predicates evaluated in the same launch).  Steps rotate over `--sets` distinct input/output sets so
that consecutive steps cannot be served from the 256 MiB Infinity Cache.  A plain run sets up, warms up,
times exactly K steps and prints the headline; `--full` adds everything else the line can carry (other
sampling patterns, the other BASELINE configs, strong scaling, the CPU baseline, the check of the fused
predicates).  `--dump-outputs DIR` writes what the last timed step computed as DIR/*.npy.  With N > 1 every rank owns
one GPU and its own pairs (independent units, "weak" scaling, no data-path collective); the only
exchange is the one-off RCCL broadcast of the shared first flow field before the timed region.
Started WITHOUT a launcher (`python bench.py --gpus N`, WORLD_SIZE unset) the process becomes the launcher
itself: it spawns N fresh rank processes before anything touches the GPU and relays rank 0's line.
Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np

H, W = 2160, 3840
BYTES_PER_PX = 27            # 2 x (8 + 1) read + (8 + 1) written
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: 8 TB/s HBM3E peak
TRAFFIC_FILES = ("profiles/r04_compose3_traffic.json", "profiles/r03_compose3_traffic.json", "profiles/r02_compose3_traffic.json", "profiles/r01_compose3_traffic.json")
DUMP_MAX_BYTES = 64 << 20     # --dump-outputs: whole outputs up to this size, else DUMP_SAMPLE_PX seeded pixels
DUMP_SAMPLE_PX = 1 << 21
DUMP_SEED = 20240611


PATTERN = "scale"
ANGLE = -30.0


def make_pair(of, h, w, ref, variant, pattern=None):
    """Synthetic pair of SURVEY.md 8(d) config 2, scaled to the requested size; `variant` perturbs the
    angle/scale slightly so that the rotating sets are not byte-identical.  `pattern` selects what the
    SAMPLING field looks like: "scale" (the config: f2 = scaling 0.8, 36 % of the samples fall outside),
    "shift" (f2 = 3.3 px translation: streaming-friendly gather) or "rot" (f1 and f2 swapped: samples lie
    on a grid rotated by 30 degrees)."""
    pattern = pattern or PATTERN
    ang = ANGLE + 0.5 * variant
    sc = 0.8 + 0.005 * variant
    f1 = of.Flow.from_transforms([['rotation', w / 2.0, h / 2.0, ang]], [h, w], ref)
    f2 = of.Flow.from_transforms([['scaling', w * 400.0 / 1920.0, h * 300.0 / 1080.0, sc]], [h, w], ref)
    if pattern == "shift":
        f2 = of.Flow.from_transforms([['translation', 3.3 + 0.1 * variant, -2.7]], [h, w], ref)
    elif pattern == "rot":
        f1, f2 = f2, f1
    rng = np.random.default_rng(variant)
    m1 = rng.random((h, w)) > 0.05
    m2 = rng.random((h, w)) > 0.05
    return of.Flow(f1.vecs, ref, m1), of.Flow(f2.vecs, ref, m2)


def _rate(fn, budget_s, max_n):
    fn()                                                    # warm-up (page faults, OpenMP pool)
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt > budget_s or n >= max_n:
            return n / dt, n


def cpu_baseline(h, w, ref, budget_s=6.0):
    """The oracle (CPU restatement) timed on this box's host cores on a bounded sample of the same workload, split as
    SURVEY 8(d) asks: the NumPy op sequence of the reference on one thread, and the fused C closed form (OpenMP) on all
    of this GPU's host cores and on one.  `value` is the closest thing to what the reference does on this box: its NumPy
    passes (single-threaded, as NumPy is) around a multi-threaded remap (cv2.remap parallelises internally)."""
    from oracle import np_oracle as O
    O.build()
    import oflibnumpy_amd as of
    cores = min(len(os.sched_getaffinity(0)), 16)            # one GPU's CPU share on this pool
    f1, f2 = make_pair(of, h, w, ref, 0, "scale")
    a, b = O.OFlow(f1.vecs, ref, f1.mask), O.OFlow(f2.vecs, ref, f2.mask)
    fa, fb, sign = (f1, f2, -1) if ref == 't' else (f2, f1, +1)
    raw = lambda: O.compose3_raw(fa.vecs, fa.mask, fb.vecs, fb.mask, sign)
    threads = O.set_threads(cores)
    v_mt, n_mt = _rate(lambda: a.combine_with(b, 3), budget_s, 16)
    c_mt, _ = _rate(raw, budget_s / 2, 64)
    O.set_threads(1)
    v_1, n_1 = _rate(lambda: a.combine_with(b, 3), budget_s, 8)
    c_1, _ = _rate(raw, budget_s / 2, 16)
    O.set_threads(cores)
    return {"value": round(v_mt, 4), "unit": "flow-fields/s", "cores": threads, "kind": "port",
            "sample": "{} x OFlow.combine_with(mode=3) at {}x{} '{}' (NumPy op sequence of the reference, single thread, "
                      "+ C restatement of cv2.remap on {} OpenMP threads)".format(n_mt, h, w, ref, threads),
            "numpy_1thread": {"value": round(v_1, 4), "cores": 1,
                              "sample": "{} x the same with the remap on one thread as well".format(n_1)},
            "c_omp_all_cores": {"value": round(c_mt, 3), "cores": threads,
                                "sample": "oracle/ofl_oracle.c orc_compose3 (fused closed form, no NumPy passes)"},
            "c_1thread": {"value": round(c_1, 3), "cores": 1, "sample": "the same, OMP threads = 1"}}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sets", type=int, default=0, help="distinct HBM-resident input/output sets rotated over "
                                                      "(default: enough to exceed the 256 MiB Infinity Cache twice)")
    ap.add_argument("--batch", type=int, default=8, help="independent flow-field pairs per step (one launch)")
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--ref", default="t", choices=["t", "s"])
    ap.add_argument("--no-stats", action="store_true", help="skip the fused zero-flow predicates (A/B only)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the shift / rot pattern measurements")
    ap.add_argument("--prewarm-ms", type=float, default=250.0,
                    help="untimed launches for at least this long before --warmup/--steps (clock ramp of a cold GPU)")
    ap.add_argument("--pattern", default="scale", choices=["scale", "shift", "rot"],
                    help="sampling pattern of the gather (default: the BASELINE config)")
    ap.add_argument("--angle", type=float, default=-30.0, help="rotation angle of f1 (default: the BASELINE config, -30 deg)")
    ap.add_argument("--min-timed-ms", type=float, default=0.0,
                    help="repeat the K timed steps (each repeat bracketed like the first) until this much GPU time has been "
                         "timed and report the MEDIAN repeat (default 0: the K steps are timed once)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline: the shift / rot patterns, the other BASELINE "
                         "configs, the strong-scaling entries, the CPU baseline and the fused zero-flow predicates "
                         "(the --no-* options narrow it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the vecs and masks of the last step's pairs as DIR/vecs.npy and "
                         "DIR/mask.npy (float32; a fixed, seeded pixel sample when the whole output exceeds 64 MiB)")
    ap.add_argument("--no-configs", action="store_true", help="skip the other BASELINE configs (\"configs\": N = 1 only)")
    ap.add_argument("--no-strong", action="store_true", help="skip the strong-scaling entries (\"strong\": config 4 / 5 over N ranks)")
    ap.add_argument("--configs-budget-s", type=float, default=75.0)
    return ap.parse_args()


def dump_outputs(dirname, out, batch, h, w):
    """What the caller of the timed path receives from the last step: the composed vectors and valid masks of its `batch`
    pairs, as DIR/vecs.npy [batch][.., 2] and DIR/mask.npy [batch][..] (0 / 1), both float32.  Whole fields up to
    DUMP_MAX_BYTES in all; above that the same seeded sample of DUMP_SAMPLE_PX / batch pixel indices (sorted, raster order)
    from every field."""
    from oflibnumpy_amd import _native as nat
    lib = nat.load()
    n = h * w
    idx = None
    if batch * n * 12 > DUMP_MAX_BYTES:
        idx = np.unique(np.random.default_rng(DUMP_SEED).integers(0, n, size=max(1, DUMP_SAMPLE_PX // batch)))
    vecs, mask = [], []
    v = np.empty((n, 2), np.float32)
    m = np.empty(n, np.uint8)
    for j in range(batch):
        nat.check(lib.ofl_download(v.ctypes.data, out.vecs.ptr + j * n * 8, n * 8, None))
        nat.check(lib.ofl_download(m.ctypes.data, out.mask.ptr + j * n, n, None))
        vecs.append(v.reshape(h, w, 2).copy() if idx is None else v[idx])
        mask.append(m.reshape(h, w).astype(np.float32) if idx is None else m[idx].astype(np.float32))
    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, "vecs.npy"), np.stack(vecs))
    np.save(os.path.join(dirname, "mask.npy"), np.stack(mask))


def main():
    args = parse_args()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # launcher mode: nothing below this line has run, the GPU is untouched in this process
        from oflibnumpy_amd import sharding
        raise SystemExit(sharding.spawn_ranks(os.path.abspath(__file__), sys.argv[1:], args.gpus,
                                            timeout=float(os.environ.get("OFL_SPAWN_TIMEOUT", "900"))))
    h, w = args.height, args.width
    global PATTERN, ANGLE
    PATTERN = args.pattern
    ANGLE = args.angle

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit("--gpus {} but WORLD_SIZE {}".format(args.gpus, world))

    # The engine (plain HIP runtime behind a C ABI) is loaded BEFORE torch so that it binds the system
    # ROCm runtime; torch is used for the rendezvous / barrier / max-reduce only (gloo, CPU tensors).
    os.environ.setdefault("OFL_DEVICE", str(local_rank))
    import ctypes
    import oflibnumpy_amd as of
    from oflibnumpy_amd import device as dev, sharding
    nat = of.native
    nat.ensure_device()
    lib = nat.load()

    dist = None
    if world > 1:
        import torch.distributed as dist
        # gloo announces its connections on STDOUT; the contract is ONE JSON line there, so the rendezvous (and a
        # first barrier, which completes the mesh) runs with fd 1 pointing at stderr
        sys.stdout.flush()
        saved_stdout = os.dup(1)
        os.dup2(2, 1)
        try:
            dist.init_process_group("gloo", rank=rank, world_size=world)
            dist.barrier()
        finally:
            sys.stdout.flush()
            os.dup2(saved_stdout, 1)
            os.close(saved_stdout)

    def barrier():
        if dist is not None:
            dist.barrier()

    def device_sync():
        nat.check(lib.ofl_device_sync())

    # ---------------------------------------------------------------- inputs resident in HBM
    ref = args.ref
    B = max(1, args.batch)
    set_bytes = BYTES_PER_PX * h * w * B
    n_sets = args.sets if args.sets > 0 else max(2, -(-(3 * 256 << 20) // set_bytes))
    n = h * w

    class Batch:            # B fields stored back to back: vecs [B][H][W][2] f32, mask [B][H][W] u8
        def __init__(self, mask=None):
            self.vecs, self.mask, self.shape = dev.DeviceBuffer(B * n * 8), (mask or dev.DeviceBuffer(B * n)), (h, w)

        def put(self, i, flow, with_mask=True):
            v = np.ascontiguousarray(flow.vecs, np.float32)
            nat.check(lib.ofl_upload(self.vecs.ptr + i * n * 8, v.ctypes.data, n * 8, None))
            if with_mask:
                m = flow.mask.astype(np.uint8)
                nat.check(lib.ofl_upload(self.mask.ptr + i * n, m.ctypes.data, n, None))
            nat.check(lib.ofl_stream_sync(None))

    sets = []
    pair_cache = {}
    for i in range(n_sets):
        b1, b2, out = Batch(), Batch(), Batch()
        for j in range(B):
            var = (i * B + j) % 4 + 4 * rank          # 4 distinct pairs per rank: the rotation is about where the bytes
            if var not in pair_cache:                  # live (cache residency), not about their values
                pair_cache[var] = make_pair(of, h, w, ref, var)
            f1, f2 = pair_cache[var]
            b1.put(j, f1)
            b2.put(j, f2)
        fa, fb, sign = (b1, b2, -1) if ref == 't' else (b2, b1, +1)
        sets.append((fa, fb, sign, out))

    # ---------------------------------------------------------------- the one exchange step (set-up, untimed)
    rccl_note, rccl_ranks, rccl_bad = ("not needed (1 GPU)" if world == 1 else "skipped (ranks share a GPU)"), 0, 0
    if world > 1 and nat.device_count() < world:
        if rank == 0:
            print("rehearsal: {} ranks share {} GPU(s); the RCCL broadcast is skipped".format(world, nat.device_count()),
                  file=sys.stderr)
    elif world > 1:
        # broadcast a shared source field over xGMI (RCCL) on its OWN stream, so that a stuck collective cannot block the
        # timed launches; the outcome is agreed between the ranks (gloo) and reported in the JSON line.
        import threading
        result = {}
        cstream = ctypes.c_void_p()
        nat.check(lib.ofl_stream_create(ctypes.byref(cstream)))

        def exchange():
            try:
                uid = np.zeros(128, np.uint8)
                if rank == 0:
                    nat.check(lib.ofl_comm_unique_id(uid.ctypes.data))
                uid = np.ascontiguousarray(sharding.broadcast_bytes(dist, uid, 0))
                nat.check(lib.ofl_comm_init(uid.ctypes.data, rank, world))
                nat.check(lib.ofl_comm_broadcast(sets[0][0].vecs.ptr, h * w * 8, 0, cstream))  # first field of the first batch
                nat.check(lib.ofl_comm_broadcast(sets[0][0].mask.ptr, h * w, 0, cstream))
                nat.check(lib.ofl_stream_sync(cstream))
                k = ctypes.c_int(0)
                nat.check(lib.ofl_comm_size(ctypes.byref(k)))
                result["ranks"] = k.value
                result["note"] = "ok"
            except Exception as e:      # noqa: BLE001 - reported, not hidden
                result["note"] = "failed: {}".format(e)

        worker = threading.Thread(target=exchange, daemon=True)
        worker.start()
        worker.join(float(os.environ.get("OFL_RCCL_TIMEOUT", "90")))
        hung = worker.is_alive()
        rccl_note = "timed out" if hung else result.get("note", "failed")
        rccl_ranks = result.get("ranks", 0)
        # 0 = ok, 1 = failed cleanly (the path needs no collective: measured anyway), 2 = a rank is stuck inside RCCL
        rccl_bad = int(sharding.max_over_ranks(dist, [2.0 if hung else (0.0 if rccl_note == "ok" else 1.0)])[0])
        if rccl_note != "ok":
            print("rank {}: RCCL broadcast {}".format(rank, rccl_note), file=sys.stderr)
        if rccl_bad and rccl_note == "ok":
            rccl_note = "ok here, failed on another rank"
    # flag words of every timed launch (<= 64 repeats of the K steps with --min-timed-ms)
    stat_rows = max(64, args.warmup + (65 if args.min_timed_ms > 0 else 1) * args.steps)
    stats = None if args.no_stats else dev.DeviceBuffer.zeros(32 * B * stat_rows)

    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    nat.check(lib.ofl_event_create(ctypes.byref(ev0)))
    nat.check(lib.ofl_event_create(ctypes.byref(ev1)))

    def step(i, which=None):
        fa, fb, sign, out = (which or sets)[i % len(sets)]
        dev.compose3_launch(fa, fb, sign, out, stats, 32 * B * (i % stat_rows) if stats is not None else 0, batch=B)

    def timed(steps, warm, which=None, first=0):
        """`warm` untimed + `steps` timed launches; returns (wall seconds, HIP-event ms per launch) of the timed ones."""
        for i in range(warm):
            step(first + i, which)
        device_sync()
        barrier()
        t0 = time.perf_counter()
        nat.check(lib.ofl_event_record(ev0, None))
        for i in range(warm, warm + steps):
            step(first + i, which)
        nat.check(lib.ofl_event_record(ev1, None))
        device_sync()
        barrier()
        el = time.perf_counter() - t0
        ms = ctypes.c_float()
        nat.check(lib.ofl_event_elapsed_ms(ev0, ev1, ctypes.byref(ms)))
        return el, ms.value / steps

    # untimed, time-based pre-warm: a GPU that has idled through the set-up needs a few hundred ms of work before its
    # clocks settle; the driver's --warmup 5 alone is 2 ms of launches
    prewarm_ms, t0 = 0.0, time.perf_counter()
    while args.prewarm_ms > 0 and prewarm_ms < args.prewarm_ms:
        for i in range(16):
            step(i % 64)
        device_sync()
        prewarm_ms = (time.perf_counter() - t0) * 1e3
    if stats is not None:
        nat.check(lib.ofl_memset(stats.ptr, 0, stats.nbytes, None))

    # EXACTLY K timed steps between barrier + synchronisation, after W warm-up steps.  With --min-timed-ms the K-step region is
    # repeated (the same K steps, no further warm-up) until that much GPU time has been timed, and the line reports the
    # median repeat.
    repeats = []
    first = 0
    while True:
        el, kms = timed(args.steps, args.warmup if not repeats else 0, first=first)
        if dist is not None:
            el, kms = sharding.max_over_ranks(dist, [el, kms])
        repeats.append((el, kms))
        first += args.steps + (args.warmup if len(repeats) == 1 else 0)
        done = sum(r[1] for r in repeats) * args.steps >= args.min_timed_ms or len(repeats) >= 64
        if dist is not None:
            done = sharding.max_over_ranks(dist, [0.0 if done else 1.0])[0] == 0.0      # (all ranks leave the loop together)
        if done:
            break
    order = sorted(range(len(repeats)), key=lambda i: repeats[i][0])
    elapsed, kernel_ms = repeats[order[len(order) // 2]]
    total = first
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, sets[(total - 1) % len(sets)][3], B, h, w)     # the last timed step's outputs

    # the predicates computed inside the timed launches: none of these synthetic flows is zero, so the
    # reference would not have taken an early exit on any step
    if args.full and stats is not None:
        words = stats.to_host((min(total, stat_rows) * B, 8), np.uint32)
        assert words[:, [0, 1, 4, 5, 6, 7]].all(), "unexpected zero-flow predicate"

    # secondary sampling patterns, same launch shape (N = 1 only): "rot" = the two roles swapped (samples on a grid
    # rotated by 30 degrees), "shift" = a 3.3-px translation as the sampling field
    algo_bytes = BYTES_PER_PX * h * w * B
    secondary = {}
    if args.full and world == 1 and not args.no_secondary and PATTERN == "scale":
        rot_sets = [(fb, fa, sign, out) for fa, fb, sign, out in sets]
        tr = of.Flow.from_transforms([['translation', 3.3, -2.7]], [h, w], ref)
        shift_sets = []
        for fa, fb, sign, out in sets:
            sb = Batch(mask=(fb if ref == 't' else fa).mask)
            for j in range(B):
                sb.put(j, tr, with_mask=False)
            shift_sets.append((fa, sb, sign, out) if ref == 't' else (sb, fb, sign, out))
        for name, which in (("rot", rot_sets), ("shift", shift_sets)):
            _, kms = timed(max(20, min(args.steps, 50)), 5, which)
            secondary[name] = {"kernel_ms": round(kms, 5), "frac": round(algo_bytes / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}

    # the buffers of the headline are no longer needed: the other configs want the memory pool to themselves
    del sets
    if secondary:
        del rot_sets, shift_sets
    dev.empty_cache()
    log = lambda msg: print("[bench] " + msg, file=sys.stderr, flush=True)
    configs, strong = None, None
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    if args.full and world == 1 and not args.no_configs and (h, w) == (H, W) and PATTERN == "scale":
        # BASELINE configs 2 - 5 and the Delaunay-path cases on this GPU, rotating sets as the headline (tools/bench_ops.py)
        import bench_ops
        configs = bench_ops.collect(iters=12, budget_s=args.configs_budget_s, log=log)
    if args.full and not args.no_strong and (h, w) == (H, W) and PATTERN == "scale":
        import bench_strong
        strong = bench_strong.run(of, dist, rank, world, comm_ok=(rccl_note == "ok" and rccl_bad == 0), log=log if rank == 0 else (lambda m: None))
    if rank == 0:
        fields = args.steps * world * B
        achieved = algo_bytes / (kernel_ms * 1e-3) / 1e9
        line = {
            "metric": "flow-fields/sec for combine_with mode=3 @{}x{} float32".format(h, w),
            "value": round(fields / elapsed, 2), "unit": "flow-fields/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 5),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": "Flow.combine_with(mode=3), ref '{}', {}x{} float32 vecs + uint8 masks: "
                                   "f1 = rotation(-30 deg about centre), f2 = scaling(0.8), 5% random invalid "
                                   "pixels; {} independent pairs per step (one launch) per GPU, {} rotating HBM-resident "
                                   "sets".format(ref, h, w, B, n_sets),
                       "fields_per_step_per_gpu": B, "fused_zero_flow_predicates": stats is not None, "sampling_pattern": PATTERN,
                       "parallelism": "independent pairs per GPU x{}".format(world), "rccl_broadcast": rccl_note,
                       "rccl_ranks": rccl_ranks, "prewarm_ms": round(prewarm_ms, 1),
                       "parity_note": "bit-identical to oracle/ofl_oracle.c; cv2.remap parity unpinned below 1/32 px (OpenCV absent)"},
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": None,
                         "kernel": "compose3_xpose_kernel", "kernel_ms": round(kernel_ms, 5),
                         "algorithmic_bytes_per_launch": algo_bytes},
            "timed_region": {"repeats": len(repeats), "steps_per_repeat": args.steps, "reported": "median repeat",
                             "gpu_ms_timed": round(sum(r[1] for r in repeats) * args.steps, 2),
                             "kernel_ms_min_max": [round(min(r[1] for r in repeats), 5), round(max(r[1] for r in repeats), 5)]},
        }
        if secondary:
            line["roofline"]["other_patterns"] = secondary
        for rel in TRAFFIC_FILES:
            tpath = os.path.join(ROOT, rel)
            if os.path.exists(tpath) and (h, w) == (H, W):
                # HBM bytes per launch from the committed rocprofv3 PMC passes of THIS sampling pattern (FETCH_SIZE doubled
                # per the gfx950 correction + WRITE_SIZE; tools/prof_bench.sh), scaled from the profiled batch to this run's
                # batch -- a profiler cannot run inside the timed region, so it is not measured in this run
                tj = json.load(open(tpath))
                per_field = tj.get("patterns", {}).get(PATTERN, {}).get("hbm_bytes_per_field") or (tj.get("hbm_bytes_per_field") if PATTERN == "scale" else None)
                if per_field:
                    line["roofline"]["traffic"] = round(per_field * B)
                    line["roofline"]["traffic_source"] = rel
                    for name in secondary:
                        pf = tj.get("patterns", {}).get(name, {}).get("hbm_bytes_per_field")
                        if pf:
                            secondary[name]["traffic"] = round(pf * B)
                    break
        if configs is not None:
            line["configs"] = configs
        if strong is not None:
            line["strong"] = strong
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(h, w, ref)
        print(json.dumps(line), flush=True)
    if dist is not None:
        if rccl_bad >= 2:
            # some rank is still inside RCCL: neither the communicator nor the process group can be torn down in step.
            # Every rank leaves with the same non-zero code (the line above says why); nothing is re-exec'ed.
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(3)
        nat.check(lib.ofl_comm_destroy())      # no-op when no communicator was created
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
