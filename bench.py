#!/usr/bin/env python3
"""Benchmark: mantis3 rig poses/s on MI355X (BASELINE.json metric).

Workload (default, --config 3; BASELINE.json configs[2], the metric's
"1280x720 4-cam batch"): rigs of 4 fisheye cameras at 1280x720 over the
IARC-style grid, shared map (params/map.yaml, 720 landmarks); the full
reference per-camera path (detector -> RPP -> clustering -> scoring ->
particle filter -> shifts -> yaw -> publish gate) plus the rig fusion and the
joint rig Gauss-Newton, batched `--rigs` rigs per step per GPU. Frames are
synthetic, rendered into HBM before timing (inputs resident in HBM); with
`--full` a second leg passes the same frames as pageable host buffers (H2D
inside the timed region) and is reported beside it as `host_ingest`.

Other legs (same JSON contract, own metric names):
  --config 4  BASELINE configs[3]: 8-camera 1920x1080 rigs, camera-sharded
              across the ranks (mantis_process_rig_sharded: RCCL all-gathers
              of the particle-filter flags and camera results, one RCCL
              all-reduce of the J^T J / J^T r accumulators per GN iteration).
              Strong scaling: every rank holds 8/N cameras of every rig.
  --config 2  BASELINE configs[1]: a 1280x720 single-camera stream through
              the full callback, one mantis_process call per frame as the ROS
              node makes (poses/s and p50 latency), the same frames batched
              (mantis_process_batch, the cv::RNG stream carried, identical
              results), and the 256-hypothesis scoring microbatch
              (mantis_score_argmin_dev). Replicas across ranks.
  --config 5  BASELINE configs[4]: 16,200-hypothesis dense grid at 1280x720
              sharded across ranks (mantis_score_argmin, one RCCL all-gather
              of (err, index) per frame). Strong scaling.

Multi-GPU: one process per GPU. Under torchrun (WORLD_SIZE in the env) this
process is one rank. `--gpus N` without torchrun makes this process a
launcher that never touches the GPU: it spawns N ranks of itself with
RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, and prints rank 0's line.
Ranks use torch.distributed over gloo (host) for the barriers, the RCCL
unique-id broadcast and the max-over-ranks time; the data path's collectives
are the library's own RCCL calls. Config 3 rigs are independent units: each
rank processes its own batch (weak scaling, no data-path collective).

A plain config-3 run sets up, warms up, times the `--steps` steps and prints
the result line (value, ms_per_step and what the timed steps themselves give).
`--dump-outputs DIR` writes what the last timed step returned (rank 0's rig and
camera results, one float64 .npy per record field); the frames, the map and
the cv::RNG seed are fixed, so the same arguments give the same inputs.

With `--full` (config 3) also reported: p50 single-rig latency (host submit ->
result, device-resident and host frames), the host-ingest leg, the dominant
kernel's roofline (HIP events on the library stream during the timed region),
and the CPU oracle baseline timed on this host before the GPU is touched
(rank 0, N=1 only): one core and all cores (one frame stream per thread).
"""
import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time

# the rig-latency path (the p50 leg) replays hipGraphs only with the HIP
# runtime's graph packet capture off, set before HIP initialises
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

HBM_PEAK_GBS = 8000.0       # MI355X HBM3E spec (MI355X_MICROARCH.md)
FP64_PEAK_TFLOPS = 78.6     # MI355X FP64 vector spec
# FP64 operations of one ObjPose iteration (one AbsKernel: the 3x3 accumulations,
# OpenCV's one-sided Jacobi SVD, R, t and the error), counted by
# tools/rpp_flops.cpp on the host build of mk_rpp.h (+,-,*,/,sqrt,hypot = 1 each).
# 1704 = what the device executes: the Jacobi noise-phase fast-forward
# (mk_rpp.h jacobi_noise_ff) skips the ~19 sweeps that only shrink the
# rank-deficient row (the full reference sweep count is 4282 per iteration).
FLOPS_PER_OBJPOSE_ITER = 1704
LANDMARKS = 720
FLOPS_PER_PROJ = 51         # BASELINE.md roofline formulas
FLOPS_PER_WINDOW = 200
METRIC3 = "poses/sec + p50 per-frame latency, 1280x720 4-cam batch"


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--config", type=int, default=3, choices=(2, 3, 4, 5))
    p.add_argument("--full", action="store_true",
                   help="config 3: beside the headline figure also the CPU oracle baseline, the p50 single-rig "
                        "latencies, the host-ingest leg and the per-stage / roofline figures (stage events on during "
                        "the timed steps, one isolated step after them)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="config 3: after the timed steps write what the last timed step returned (every rig result "
                        "and camera result of the step, in step order) as DIR/<name>.npy, float64")
    p.add_argument("--stream-frames", type=int, default=1000,
                   help="config 2: frames of the single-camera stream (mantis_process per frame)")
    p.add_argument("--stream-batch", type=int, default=250,
                   help="config 2: frames per mantis_process_batch call in the batched-stream leg")
    p.add_argument("--microbatches", type=int, default=200,
                   help="config 2: timed 256-hypothesis scoring microbatches")
    p.add_argument("--rigs", type=int, default=None,
                   help="rigs per step per GPU (config 3, default 1024 per context) / rigs per step (config 4, "
                        "default 512)")
    p.add_argument("--frames", type=int, default=16, help="config 5: frames per step (16,200 hypotheses each)")
    p.add_argument("--distinct", type=int, default=128, help="distinct rendered rigs (cycled through the batch)")
    p.add_argument("--contexts", type=int, default=6,
                   help="config 3: library contexts per GPU, each driven by its own host thread (one ctx per "
                        "thread, include/mantis.h); the step's rigs are split evenly between them")
    p.add_argument("--contexts4", type=int, default=0,
                   help="config 4: library contexts per rank (each with its own RCCL communicator and host thread); "
                        "0 = 4 at one rank, 1 otherwise")
    p.add_argument("--latency-iters", type=int, default=32,
                   help="single-rig calls of each p50 latency figure (config 3: with --full)")
    p.add_argument("--ingest-steps", type=int, default=1,
                   help="config 3 --full: timed steps of the host-ingest leg (pageable host frames); 0 = skip")
    p.add_argument("--cpu-seconds", type=float, default=8.0,
                   help="--full CPU baseline: seconds of oracle work per leg (1 core, all cores)")
    p.add_argument("--cpu-threads", type=int, default=0,
                   help="CPU baseline all-cores leg: threads (0 = one frame stream per visible host CPU, "
                        "BASELINE.md §3)")
    p.add_argument("--hw-queues", type=int, default=None,
                   help="GPU_MAX_HW_QUEUES for this process (default 4 per context, at most 32: each context has "
                        "a compute and a copy stream, and streams that share a hardware queue serialise; measured "
                        "at 4 contexts: 8 / 16 / 32 queues -> 15.5k / 16.0k / 15.8k rig poses/s)")
    p.add_argument("--no-cpu", action="store_true", help="--full without the CPU baseline")
    p.add_argument("--gn", type=int, default=1,
                   help="joint rig Gauss-Newton after the per-camera pipeline (SURVEY §8 d configs 3/4); "
                        "0 = reference-parity only")
    p.add_argument("--gn-iterations", type=int, default=8)
    p.add_argument("--max-contour-points", type=int, default=None,
                   help="per-frame contour point pool, in 64-point chunks per border (default 98304 at 720p: ~22k "
                        "points used, max seen 28k; 262144 at 1080p); overflow is an error")
    a = p.parse_args()
    if a.rigs is None:
        # config 4: 512 rigs (128 per context at one rank) so the ObjPose chain
        # floor of a launch (~25 ms) is shared by enough frames: 128 / 256 /
        # 512 / 1024 rigs gave 2.3k / 3.3k / 4.2k / 4.8k rig poses/s on 1 GPU
        a.rigs = 1024 * a.contexts if a.config == 3 else 512
    if a.hw_queues is None:
        a.hw_queues = 4 * a.contexts
    if a.max_contour_points is None:
        a.max_contour_points = 262144 if a.config == 4 else 98304
    return a


# ------------------------------------------------------------------ launcher
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch(a):
    """`--gpus N` without torchrun: spawn N ranks of this script (this process
    never touches the GPU), forward rank 0's JSON line; when a rank fails the
    others are stopped and the launcher fails."""
    import tempfile

    port = _free_port()
    procs, logs = [], []
    for r in range(a.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.gpus), LOCAL_WORLD_SIZE=str(a.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        f = tempfile.TemporaryFile(mode="w+")
        logs.append(f)
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=f, stderr=subprocess.STDOUT, text=True))
    codes = [None] * a.gpus
    while any(c is None for c in codes):
        time.sleep(0.2)
        for r, p in enumerate(procs):
            if codes[r] is None:
                codes[r] = p.poll()
        if any(c not in (None, 0) for c in codes):
            for r, p in enumerate(procs):
                if codes[r] is None:
                    p.kill()
                    codes[r] = p.wait()
    outs = []
    for f in logs:
        f.seek(0)
        outs.append(f.read())
        f.close()
    for r, o in enumerate(outs):
        for ln in o.splitlines():
            if r != 0 or not ln.startswith("{"):
                print(f"[rank {r}] {ln}", file=sys.stderr)
    bad = [(r, c) for r, c in enumerate(codes) if c != 0]
    if bad:
        print(f"bench: rank(s) failed (rank, exit code): {bad}", file=sys.stderr)
        return 1
    lines = [ln for ln in outs[0].splitlines() if ln.startswith("{")]
    if not lines:
        print("bench: rank 0 printed no result line", file=sys.stderr)
        return 1
    print(lines[-1], flush=True)
    return 0


class Ranks:
    """torch.distributed over gloo for the host-side bench plumbing (barrier,
    unique-id broadcast, max time); a no-op at world size 1."""

    def __init__(self):
        self.rank = int(os.environ.get("RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.local = int(os.environ.get("LOCAL_RANK", "0"))
        self.dist = None
        if self.world > 1:
            import datetime

            import torch.distributed as tdist

            tdist.init_process_group(backend="gloo", timeout=datetime.timedelta(seconds=300))
            self.dist = tdist

    def barrier(self):
        if self.dist is not None:
            self.dist.barrier()

    def max(self, x):
        if self.dist is None:
            return x
        import torch

        t = torch.tensor([x], dtype=torch.float64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def sum(self, x):
        if self.dist is None:
            return x
        import torch

        t = torch.tensor([x], dtype=torch.float64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return float(t.item())

    def seen(self):
        return self.dist.get_world_size() if self.dist is not None else 1

    def close(self):
        if self.dist is not None:
            self.dist.destroy_process_group()


def die(rk, msg):
    print(f"bench rank {rk.rank}/{rk.world}: {msg}", file=sys.stderr, flush=True)
    sys.exit(1)


def make_ctx(M, rk, **cfg):
    try:
        return M.Mantis(M.default_config(device=rk.local, **cfg))
    except M.MantisError as e:
        die(rk, f"cannot create a library context on device {rk.local} ({e}); this needs an MI355X per rank")


def lib_sha16():
    """First 16 hex digits of the running product library's SHA-256 (hipcc
    output is not bit-reproducible: a rebuild of the same sources differs)."""
    import hashlib

    try:
        return hashlib.sha256(open(os.path.join(ROOT, "mantis_amd", "libmantis_amd.so"), "rb").read()).hexdigest()[:16]
    except OSError:
        return None


def src_sha16(root=None):
    """First 16 hex digits of the SHA-256 over the library's sources (every
    file under mantis_amd/csrc, include/*.h, the Makefile): the build identity
    PMC summaries record. The bench line uses a summary only when it matches,
    so a profile of other code is never mixed in, while a rebuild of the same
    sources (hipcc's output differs byte-wise from build to build) keeps it."""
    import glob
    import hashlib

    root = root or ROOT
    files = sorted(glob.glob(os.path.join(root, "mantis_amd", "csrc", "*")) + glob.glob(os.path.join(root, "include", "*.h"))
                   + [os.path.join(root, "Makefile")])
    h = hashlib.sha256()
    for f in files:
        if os.path.isfile(f):
            h.update(os.path.relpath(f, root).encode() + b"\0" + open(f, "rb").read() + b"\0")
    return h.hexdigest()[:16]


def cpu_model():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def dump_outputs(out_dir, batches):
    """What the last step's mantis_process_batch calls returned, the contexts'
    shares in step order: one float64 array per field of mantis_result
    (rig_<field>.npy, one row per rig) and of mantis_cam_result
    (cam_<field>.npy, one row per camera frame). The 64-bit cv::RNG state is
    split into its high and low 32 bits so that float64 holds it exactly.
    6144 rigs x 4 cameras come to 16 MB."""
    os.makedirs(out_dir, exist_ok=True)
    for prefix, arrs in (("rig", [b.out for b in batches]), ("cam", [b.cam_out for b in batches])):
        rec = np.concatenate([np.frombuffer(x, dtype=np.dtype(x._type_)) for x in arrs])
        for name in rec.dtype.names:
            v = rec[name]
            if v.dtype == np.uint64:
                v = np.stack([v >> np.uint64(32), v & np.uint64(0xFFFFFFFF)], axis=1)
            np.save(os.path.join(out_dir, f"{prefix}_{name}.npy"), np.ascontiguousarray(v, np.float64))


# ------------------------------------------------------------- CPU baseline
def cpu_baseline(a, W, H, cams_per_rig):
    """The oracle (C++17 -O3 restatement of the reference path, test
    infrastructure) on the same synthetic scene, timed on this host BEFORE the
    GPU is touched: (1) one core, frames one at a time as the reference's
    single spinner; (2) all cores: one independent frame stream per thread
    (ctypes releases the GIL inside the oracle), aggregate rig poses/s."""
    from concurrent.futures import ThreadPoolExecutor

    import _oracle as O
    from mantis_amd import synth

    white, red, green = synth.load_map()
    K, D = synth.intrinsics(W, H)
    rng = np.random.default_rng(1000)
    ext = synth.rig_extrinsics(cams_per_rig)
    rigs = []
    for r in range(8):  # the first rigs of rank 0's bench frames (same poses and seeds)
        Twb = synth.random_base_pose(rng)
        frames = []
        for c in range(cams_per_rig):
            Twc = Twb @ ext[c]
            frames.append(synth.render_host(synth.make_cam(Twc[:3, :3], Twc[:3, 3], W, H),
                                            synth.frame_seed(3, r * cams_per_rig + c)))
        rigs.append(frames)

    def stream(k, budget):
        orc = O.Oracle(white, red, green, seed=1)
        n, t0 = 0, time.perf_counter()
        while True:
            for fr in rigs[(k + n) % len(rigs)]:
                orc.process(fr, K, D)
            n += 1
            dt = time.perf_counter() - t0
            if dt >= budget and n >= 2:
                return n, dt

    n1, t1 = stream(0, a.cpu_seconds)
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    P = max(1, a.cpu_threads if a.cpu_threads > 0 else avail)
    quota = None  # the cgroup's CPU quota (cpu.max), which bounds the aggregate whatever the thread count
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if q == "max" else round(int(q) / int(per), 2)
    except (OSError, ValueError):
        pass
    with ThreadPoolExecutor(max_workers=P) as ex:
        t0 = time.perf_counter()
        res = list(ex.map(lambda k: stream(k, a.cpu_seconds), range(P)))
        tall = time.perf_counter() - t0
    nall = sum(n for n, _ in res)
    # cores = the CPUs the P threads could actually use: the visible CPUs capped by the cgroup quota
    cores = P if quota is None else max(1, min(P, int(quota)))
    return {"value": round(nall / tall, 4), "unit": "rig poses/s", "cores": cores, "threads": P, "kind": "port",
            "cpu_model": cpu_model(), "host_cpus_visible": avail, "cgroup_cpu_quota": quota,
            "single_core": {"value": round(n1 / t1, 4), "p50_rig_ms": round(t1 / n1 * 1e3, 1), "rigs": n1},
            "sample": f"oracle/liboracle.so (C++17 -O3, full mantis3 callback per camera) on {len(rigs)} distinct "
                      f"{cams_per_rig}x{W}x{H} rigs of the bench scene: {nall} rigs over {P} threads (one frame "
                      f"stream each) in {tall:.1f} s; 1 core: {n1} rigs in {t1:.1f} s"}


# -------------------------------------------------------------------- config 3
def run_config3(a, rk, cpu):
    import mantis_amd as M
    from mantis_amd import synth

    W, H, CAMS = 1280, 720, 4
    white, red, green = synth.load_map()
    K, D = synth.intrinsics(W, H)
    n_frames = a.rigs * CAMS
    nctx = max(1, min(a.contexts, a.rigs))
    if a.rigs % nctx:
        die(rk, "--rigs must be a multiple of --contexts")
    rigs_ctx = a.rigs // nctx
    ctxs = []
    for _ in range(nctx):
        mc = make_ctx(M, rk, max_cams=rigs_ctx * CAMS, max_width=W, max_height=H, gn_enable=a.gn,
                      gn_iterations=a.gn_iterations, max_contour_points=a.max_contour_points)
        mc.set_map(white, red, green)
        ctxs.append(mc)
    m = ctxs[0]

    # ---- synthetic rigs rendered into HBM once
    rng = np.random.default_rng(1000 + rk.rank)
    ext = synth.rig_extrinsics(CAMS)
    cams, Tbc = [], []
    for r in range(a.distinct):
        Twb = synth.random_base_pose(rng)
        for c in range(CAMS):
            Twc = Twb @ ext[c]
            cams.append(synth.make_cam(Twc[:3, :3], Twc[:3, 3], W, H))
            Tbc.append(ext[c])
    nd = len(cams)
    fb = W * H * 3
    dev = m.device_alloc(nd * fb)
    seeds = [synth.frame_seed(3, i + 100000 * rk.rank) for i in range(nd)]
    m.synth_render(cams, seeds, dev)
    m.synchronize()
    imgs = [M.make_image(None, K, D, T_base_cam=Tbc[i % nd], device_ptr=dev + (i % nd) * fb, width=W, height=H)
            for i in range(n_frames)]
    per_ctx = [imgs[k * rigs_ctx * CAMS:(k + 1) * rigs_ctx * CAMS] for k in range(nctx)]
    batches = [M.Batch(ctxs[k], per_ctx[k], rigs_ctx) for k in range(nctx)]
    from concurrent.futures import ThreadPoolExecutor

    pool = ThreadPoolExecutor(max_workers=nctx)
    # per-context sums of the stage / kernel events over the timed steps
    stage_ms_k, kern_ms_k = [{} for _ in range(nctx)], [{} for _ in range(nctx)]

    def run_steps(bs, k_steps, record=False):
        """k_steps steps: every context's host thread runs its share of each step
        back to back (one C call per step), the contexts concurrently."""
        def worker(k):
            for _ in range(k_steps):
                bs[k].run()
                if record:
                    for name, ms in ctxs[k].kernel_times():  # "stage" or "stage/kernel" (hot stages: one event per kernel)
                        st = name.split("/", 1)[0]
                        stage_ms_k[k][st] = stage_ms_k[k].get(st, 0.0) + ms
                        if "/" in name:
                            kn = name.split("/", 1)[1]
                            kern_ms_k[k][kn] = kern_ms_k[k].get(kn, 0.0) + ms
        for f in [pool.submit(worker, k) for k in range(len(bs))]:
            f.result()

    def barrier_sync():
        rk.barrier()
        for mc in ctxs:
            if mc.h is not None:  # the host-ingest leg closes contexts past 4
                mc.synchronize()

    run_steps(batches, a.warmup)

    # ---- timed region: with --full, stage / kernel events on every context's
    # stream; host CPU time of this process (every context's host thread, the
    # cv::RNG draw threads, the driver's) over the same region
    for mc in ctxs:
        mc.set_profiling(a.full)
    barrier_sync()
    cpu0 = os.times()
    t0 = time.perf_counter()
    run_steps(batches, a.steps, record=a.full)
    barrier_sync()
    el_local = time.perf_counter() - t0
    cpu1 = os.times()
    elapsed = rk.max(el_local)
    for mc in ctxs:
        mc.set_profiling(False)
    if a.dump_outputs and rk.rank == 0:
        dump_outputs(a.dump_outputs, batches)
    host_cpu_s = (cpu1.user - cpu0.user) + (cpu1.system - cpu0.system)
    value = a.rigs * a.steps * rk.world / elapsed
    ms_per_step = elapsed / a.steps * 1e3
    # every step processes the same frames: the last step's records describe each step
    scored = a.steps * sum(c.n_scored for b in batches for c in b.cam_out)
    published = a.steps * sum(r.publish for b in batches for r in b.out)
    published_all = rk.sum(published)  # every rank's published rigs
    # the result line of a plain run: what the timed steps themselves give
    line = {
        "metric": METRIC3,
        "value": round(value, 3), "unit": "rig poses/s", "n_gpus": rk.world, "steps": a.steps,
        "warmup": a.warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f64",
        "data": f"synthetic fisheye grid frames rendered in HBM (SURVEY §8d scene, {a.distinct} distinct rigs "
                f"= {nd * fb / 1e9:.2f} GB cycled), map.yaml landmarks",
        "config": {"workload": "config3: 4-cam 1280x720 rig, shared map, full mantis3 path per camera"
                               + (" + joint rig Gauss-Newton" if a.gn else ""),
                   "rigs_per_step_per_gpu": a.rigs, "cams_per_rig": CAMS, "frames_per_step_per_gpu": n_frames,
                   "contexts_per_gpu": nctx, "resolution": [W, H], "landmarks": LANDMARKS,
                   "parallelism": f"rig-data-parallel x{rk.world}"},
        "ranks_seen": rk.seen(),
        "camera_frames_per_s": round(value * CAMS, 2),
        "published_frac": round(published / max(1, a.rigs * a.steps), 4),
        # SURVEY §8(d)'s "pose" = one published rig pose (the publish gate,
        # PosePub.h:16): the same timed region, counting only rigs whose
        # result passed the gate (why `value` counts every rig)
        "published_rig_poses_per_s": round(published_all / elapsed, 3),
        "host_cpu_s_per_step": round(host_cpu_s / a.steps, 4),
        "host_cpu_note": ("process user+system CPU seconds per step over the timed region (os.times: every "
                          "context's host thread incl. the cv::RNG gaussian draws); / ms_per_step = cores busy"),
        "host_cores_busy": round(host_cpu_s / el_local, 3),
        "lib_sha16": lib_sha16(),
        "src_sha16": src_sha16(),
    }
    if not a.full:
        pool.shutdown()
        for mc in ctxs:
            mc.close()
        return line if rk.rank == 0 else None

    # ---- per-step work counts (every step processes the same frames, so the
    # counters of the last step describe each step): ObjPose iterations of the
    # two RPP queues, scored hypotheses
    frames_step = rigs_ctx * CAMS  # stage events are recorded on context 0's stream, over its frames
    iters = [0, 0]
    for i in range(frames_step):
        fc = m.frame_counters(i)
        iters[0] += int(fc[16])
        iters[1] += int(fc[17])
    scored_per_frame = scored / max(1, a.steps * n_frames)
    slow_per_frame = 80.0
    fast_per_frame = max(0.0, scored_per_frame - slow_per_frame)
    s_fast = LANDMARKS * fast_per_frame
    s_slow = 3700.0 * slow_per_frame

    # ---- roofline of the dominant stage (per launch = one context's step).
    # Durations are HIP events around each kernel of the stage on the stream it
    # is launched on (the hot stages are marked per kernel), averaged over the
    # timed steps AND over every context: dispatch to completion under the other
    # contexts' load, the average rocprofv3 reports over all dispatches of the
    # same command. Context 0 alone is kept beside it: it submits first in every
    # step and its launches finish up to 2.5x sooner than the later contexts'
    # (profiles/r05_duration_sources.txt), which is how r04's line (context 0
    # only) and rocprofv3 (all contexts) came to differ.
    def mean_over_ctx(per):
        keys = set().union(*per)
        return {k: sum(d.get(k, 0.0) for d in per) / (len(per) * a.steps) for k in keys}
    avg, kavg = mean_over_ctx(stage_ms_k), mean_over_ctx(kern_ms_k)
    avg0 = {k: v / a.steps for k, v in stage_ms_k[0].items()}
    kavg0 = {k: v / a.steps for k, v in kern_ms_k[0].items()}
    work = {
        # BGR read once; candidate and strong-root bit planes written
        "canny_nms": ("hbm", frames_step * (3 * W * H + W * H // 4)),
        # candidate and strong bit planes read, edge bits written
        "hysteresis": ("hbm", frames_step * (3 * W * H // 8)),
        # edge bits read once; padded detector bits and mask bits written
        "morph": ("hbm", frames_step * (W * H // 8 + (W + 2) * (H + 2) // 8 + W * H // 8)),
        "components": ("hbm", frames_step * (5 * (W + 2) * (H + 2))),
        "border_trace": ("hbm", frames_step * ((W + 2) * (H + 2) // 8)),
        "contours_quads": ("hbm", frames_step * ((W + 2) * (H + 2) // 8)),
        "rpp_first": ("fp64", iters[0] * FLOPS_PER_OBJPOSE_ITER),
        "rpp_cand": ("fp64", iters[1] * FLOPS_PER_OBJPOSE_ITER),
        "score_pf_yaw": ("valu", frames_step * (FLOPS_PER_PROJ * (s_fast + 37 * slow_per_frame) +
                                                FLOPS_PER_WINDOW * 37 * slow_per_frame)),
    }
    stage_kernels = {"score_pf_yaw": ("k_score_init", "k_score_pf", "k_score_shift_part", "k_score_final"),
                     "canny_nms": ("k_canny_strip<2>", "k_canny_strip<1>", "k_canny"),
                     "hysteresis": ("k_hyst_rec", "k_hyst_band", "k_hyst_seam", "k_hyst_mark", "k_hyst_fix"),
                     "morph": ("k_morph",)}
    digest = lib_sha16()
    src_digest = src_sha16()

    def pmc_for(path):
        """A committed PMC summary, only when it was collected on a library
        built from these very sources (its src_sha16 = this tree's)."""
        try:
            pj = json.load(open(os.path.join(ROOT, path)))
        except (OSError, ValueError):
            return None
        return pj if pj.get("src_sha16") == src_digest else None

    def roofline(stage, avg=avg, kavg=kavg):
        if stage not in avg or stage not in work:
            return None
        kind, amount = work[stage]
        dur_s = avg[stage] * 1e-3
        ks = {k: round(kavg[k], 4) for k in stage_kernels.get(stage, ()) if k in kavg}
        r = {"kernel": stage, "kernels_ms": ks or None, "avg_launch_ms": round(avg[stage], 4), "traffic": None}
        if kind == "hbm":
            achieved = amount / dur_s / 1e9
            r.update({"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                      "frac": round(achieved / HBM_PEAK_GBS, 5), "alg_bytes_per_launch": int(amount)})
            return r
        achieved = amount / dur_s / 1e12
        r.update({"bound": "fp64" if kind == "fp64" else "valu", "achieved": round(achieved, 4),
                  "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / FP64_PEAK_TFLOPS, 5),
                  "alg_flops_per_launch": int(amount)})
        return r

    kern = [k for k in avg if k in work]
    dom = max(kern, key=avg.get) if kern else None  # dominant kernel stage by event time
    roof = roofline(dom) if dom else None
    if roof is not None:
        roof["stages_ms"] = {k: round(v, 4) for k, v in sorted(avg.items(), key=lambda kv: -kv[1])}
        roof["objpose_iterations_per_launch"] = iters
        roof["duration_source"] = ("HIP events around each kernel of the stage on its context's stream, averaged over "
                                   "the timed steps and all %d contexts (sum of kernels_ms; rocprofv3's per-dispatch "
                                   "average of the same command); context0 = the first-submitting context alone" % nctx)
        r0 = roofline(dom, avg0, kavg0)
        roof["context0"] = {"avg_launch_ms": r0["avg_launch_ms"], "kernels_ms": r0["kernels_ms"], "frac": r0["frac"]}
    roof_front = roofline("canny_nms")
    # HBM traffic and VALU issue from PMC summaries of this same build
    # (tools/pmc_score.sh / tools/pmc_traffic.sh write lib_sha16): per launch =
    # per-frame counters x frames_step; null when no summary matches the build
    pmc_path = next((p for p in (os.path.join("profiles", "r06_pmc.json"), os.path.join("profiles", "r05_pmc.json"))
                     if pmc_for(p) is not None), os.path.join("profiles", "r06_pmc.json"))
    pj = pmc_for(pmc_path)
    pmc_k = {} if pj is None else pj["kernels"]
    pmc_fr = None if pj is None else pj["frames_per_launch"]

    def pmc_stage(r, stage):
        """traffic (HBM bytes per launch: FETCH_SIZE x 2 + WRITE_SIZE) and VALU
        issue of the stage's kernels, scaled from the summary's launch size"""
        if r is None or not pmc_k or not pmc_fr:
            return
        kk = [k.split("<")[0] for k in stage_kernels.get(stage, ())]
        kk = [k for k in dict.fromkeys(kk) if k in pmc_k and "FETCH_SIZE_bytes" in pmc_k[k]]
        if not kk:
            return
        sc = frames_step / pmc_fr
        r["traffic"] = int(sum(2 * pmc_k[k]["FETCH_SIZE_bytes"] + pmc_k[k].get("WRITE_SIZE_bytes", 0) for k in kk) * sc)
        vi = sum(pmc_k[k].get("SQ_INSTS_VALU", 0) for k in kk) * sc
        if vi:
            r["valu_instructions_per_launch"] = int(vi)
            # wave64 VALU instruction = 2 cycles on a SIMD-32 (MI355X_MICROARCH.md), 1024 SIMDs at 2.4 GHz
            r["valu_issue_frac"] = round(vi * 2 / (1024 * 2.4e9 * r["avg_launch_ms"] * 1e-3), 4)
        r["pmc_source"] = (pmc_path + " (FETCH_SIZE x 2 + WRITE_SIZE, SQ_INSTS_VALU; per frame x frames_step); "
                           "the x2 is calibrated on gfx950 for every load width the stages issue (4 / 12 / 16 B "
                           "coalesced, 4-B gathers) and WRITE_SIZE is 1x for full-line stores: profiles/r05_pmc_calib.txt")

    if roof is not None and dom == "score_pf_yaw":
        roof["bound_note"] = ("FP32 screen + exact FP64 fallback on the VALU, gathers from L2/MALL: frac counts the "
                              "reference's 51 algorithmic FP64 flops per landmark projection against the FP64 vector "
                              "peak; valu_issue_frac is the VALU issue occupancy from SQ_INSTS_VALU")
    pmc_stage(roof, dom)
    pmc_stage(roof_front, "canny_nms")

    # ---- the same stages with context 0 running alone (one step, after the
    # timed region): the timed-region launch durations above include the
    # other contexts' kernels sharing the CUs; these are the kernels' own
    if nctx > 1 and roof is not None:
        m.set_profiling(True)
        ctxs[0].process(per_ctx[0], rigs_ctx)
        iso_raw = m.kernel_times()
        m.set_profiling(False)
        iso, kiso = {}, {}
        for name, ms in iso_raw:
            st = name.split("/", 1)[0]
            iso[st] = iso.get(st, 0.0) + ms
            if "/" in name:
                kiso[name.split("/", 1)[1]] = ms
        for r, stg in ((roof, dom), (roof_front, "canny_nms")):
            ri = roofline(stg, iso, kiso) if r is not None else None
            if ri is not None:
                r["isolated"] = {"avg_launch_ms": ri["avg_launch_ms"], "kernels_ms": ri["kernels_ms"],
                                 "achieved": ri["achieved"], "frac": ri["frac"],
                                 "note": "context 0 alone, one step after the timed region"}
                if "valu_instructions_per_launch" in r:
                    r["isolated"]["valu_issue_frac"] = round(
                        r["valu_instructions_per_launch"] * 2 / (1024 * 2.4e9 * ri["avg_launch_ms"] * 1e-3), 4)
        roof["stages_ms_isolated"] = {k: round(v, 4) for k, v in sorted(iso.items(), key=lambda kv: -kv[1])}
    path_bytes = n_frames * (6 * W * H + 3 * (s_fast + s_slow))

    # ---- p50 latency of one rig (host submit -> result on host), HBM frames:
    # a stream of different rigs, one call each over the first latency_iters
    # distinct rigs (rounds 1-5 repeated rig 0, whose ObjPose chains are longer
    # than the median rig's; still reported as p50_latency_rig0_ms)
    def p50_of(src, cycle=True):
        lat = []
        nr = max(1, min(a.distinct, a.latency_iters)) if cycle else 1
        for k in range(a.latency_iters):
            r = k % nr
            one = src[r * CAMS:(r + 1) * CAMS]
            t1 = time.perf_counter()
            m.process(one, rigs=1)
            lat.append(time.perf_counter() - t1)
        return float(np.median(lat)) * 1e3

    p50 = p50_of(imgs)
    p50_rig0 = p50_of(imgs, cycle=False)

    # ---- host-ingest leg: the same frames as pageable host BGR buffers (what
    # a ROS drop-in hands over); the H2D staging is inside the timed region
    ingest = None
    host = [np.empty((H, W, 3), np.uint8) for _ in range(nd)]
    for j in range(nd):
        m.d2h(host[j], dev + j * fb)
    himgs = [M.make_image(host[i % nd], K, D, T_base_cam=Tbc[i % nd]) for i in range(n_frames)]
    # host frames need each context's staging buffer (max_cams x 3 W H, allocated
    # on first use): beside the device planes of more than 4 contexts it would not
    # fit in HBM, so the ingest leg runs on 4 of them (the others are closed)
    nin = min(nctx, 4)
    for k in range(nin, nctx):
        ctxs[k].close()
    p50_host = p50_of(himgs)
    if a.ingest_steps > 0:
        hb = [M.Batch(ctxs[k], himgs[k * rigs_ctx * CAMS:(k + 1) * rigs_ctx * CAMS], rigs_ctx) for k in range(nin)]
        run_steps(hb, 1)  # one untimed pass over the host path
        barrier_sync()
        t0 = time.perf_counter()
        run_steps(hb, a.ingest_steps)
        barrier_sync()
        el = rk.max(time.perf_counter() - t0)
        h2d_bytes = nin * rigs_ctx * CAMS * fb * a.ingest_steps
        ingest = {"value": round(nin * rigs_ctx * a.ingest_steps * rk.world / el, 3), "unit": "rig poses/s",
                  "contexts": nin,
                  "ms_per_step": round(el / a.ingest_steps * 1e3, 3), "steps": a.ingest_steps,
                  "h2d_GBps_per_gpu": round(h2d_bytes / el / 1e9, 2),
                  "p50_latency_ms": round(p50_host, 3),
                  "note": "frames passed as pageable host BGR buffers (mem_kind 0); staging H2D inside the timed "
                          "region; never the headline value"}
    del host, himgs
    if a.ingest_steps > 0:
        del hb

    line.update({
        "p50_latency_ms": round(p50, 3),
        "p50_latency_rig0_ms": round(p50_rig0, 3),
        "p50_note": f"one call per rig over {max(1, min(a.distinct, a.latency_iters))} distinct rigs "
                    f"(rig0: rig 0 repeated {a.latency_iters} times, the rounds 1-5 measure)",
        "path_alg_GBps": round(path_bytes * a.steps / elapsed / 1e9, 3),
        "host_ingest": ingest,
        "roofline": roof,
        "roofline_frontend": roof_front,
        "cpu_baseline": cpu,
    })
    pool.shutdown()
    for mc in ctxs:
        mc.close()
    return line if rk.rank == 0 else None


# -------------------------------------------------------------------- config 4
def run_config4(a, rk):
    """8-camera 1920x1080 rigs, camera c on rank c % N (mantis_process_rig_sharded).
    --contexts4 contexts per rank (default 4 at one rank, 1 otherwise), each with
    its own RCCL communicator and host thread, split the step's rigs: one
    context's ObjPose tails overlap the others' image stages as in config 3."""
    import mantis_amd as M
    from mantis_amd import rig as RG
    from mantis_amd import synth

    W, H, CAMS = 1920, 1080, 8
    if rk.world > CAMS:
        die(rk, "config 4 shards 8 cameras: at most 8 ranks")
    K, D = synth.intrinsics(W, H)
    mine = RG.shard_cameras(CAMS, rk.rank, rk.world)
    nl = len(mine)
    nctx = a.contexts4 if a.contexts4 > 0 else (4 if rk.world == 1 else 1)
    nctx = max(1, min(nctx, a.rigs))
    if a.rigs % nctx:
        die(rk, "--rigs must be a multiple of the config-4 contexts")
    rpc = a.rigs // nctx
    ctxs = []
    for k in range(nctx):
        mc = make_ctx(M, rk, max_cams=rpc * nl, max_width=W, max_height=H, gn_enable=a.gn,
                      gn_iterations=a.gn_iterations, max_contour_points=a.max_contour_points)
        mc.set_map(*synth.load_map())
        mc.comm_init(rk.rank, rk.world, rk.dist)  # one communicator per context (same order on every rank)
        ctxs.append(mc)
    m = ctxs[0]
    nranks, _ = m.comm_info()
    rng = np.random.default_rng(4000)  # the same rigs on every rank
    ext = synth.rig_extrinsics(CAMS)
    distinct = min(a.distinct, a.rigs)
    cams, Tbc, seeds = [], [], []
    for r in range(distinct):
        Twb = synth.random_base_pose(rng)
        for c in mine:
            Twc = Twb @ ext[c]
            cams.append(synth.make_cam(Twc[:3, :3], Twc[:3, 3], W, H))
            Tbc.append(ext[c])
            seeds.append(synth.frame_seed(4, r * CAMS + c))
    fb = W * H * 3
    dev = m.device_alloc(len(cams) * fb)
    m.synth_render(cams, seeds, dev)
    m.synchronize()
    nd = len(cams)
    imgs = [M.make_image(None, K, D, T_base_cam=Tbc[i % nd], device_ptr=dev + (i % nd) * fb, width=W, height=H)
            for i in range(a.rigs * nl)]
    per_ctx = [imgs[k * rpc * nl:(k + 1) * rpc * nl] for k in range(nctx)]
    from concurrent.futures import ThreadPoolExecutor

    pool = ThreadPoolExecutor(max_workers=nctx)
    stage_ms, published, gn_its = {}, [0], [0]

    def run_steps(k_steps, record=False):
        def worker(k):
            for _ in range(k_steps):
                rr, _ = ctxs[k].process_sharded(per_ctx[k], rpc, mine, CAMS)
                if record:
                    published[0] += sum(r.publish for r in rr)
                    gn_its[0] += sum(r.gn_iterations for r in rr)
                    if k == 0:
                        for name, ms in m.kernel_times():
                            stage_ms[name] = stage_ms.get(name, 0.0) + ms
        for f in [pool.submit(worker, k) for k in range(nctx)]:
            f.result()

    run_steps(a.warmup)
    m.set_profiling(True)
    rk.barrier()
    for mc in ctxs:
        mc.synchronize()
    t0 = time.perf_counter()
    run_steps(a.steps, record=True)
    for mc in ctxs:
        mc.synchronize()
    rk.barrier()
    elapsed = rk.max(time.perf_counter() - t0)
    m.set_profiling(False)
    lat = []
    for _ in range(a.latency_iters):
        rk.barrier()
        t1 = time.perf_counter()
        m.process_sharded(imgs[:nl], 1, mine, CAMS)
        lat.append(rk.max(time.perf_counter() - t1))
    line = None
    if rk.rank == 0:
        avg = {k: round(v / a.steps, 4) for k, v in sorted(stage_ms.items(), key=lambda kv: -kv[1])}
        frames = rpc * nl
        canny = avg.get("canny_nms")
        roof = None
        if canny:
            alg = frames * (3 * W * H + W * H // 4)
            ach = alg / (canny * 1e-3) / 1e9
            roof = {"bound": "hbm", "kernel": "canny_nms", "achieved": round(ach, 2), "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 5), "traffic": None,
                    "alg_bytes_per_launch": alg, "avg_launch_ms": canny, "stages_ms": avg,
                    "note": "context 0's stage events while the other contexts run"}
        line = {"metric": "8-cam 1920x1080 rig poses/s, camera-sharded (config 4)",
                "value": round(a.rigs * a.steps / elapsed, 3), "unit": "rig poses/s", "n_gpus": rk.world,
                "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(elapsed / a.steps * 1e3, 3),
                "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
                "data": "synthetic fisheye grid frames rendered in HBM, map.yaml landmarks",
                "config": {"workload": "config4: 8-cam 1920x1080 rig, camera c on rank c % N, RCCL all-gathers of "
                                       "PF flags and camera results, RCCL all-reduce of J^T J / J^T r per GN "
                                       "iteration", "rigs_per_step": a.rigs, "cams_per_rank": nl,
                           "contexts_per_rank": nctx, "resolution": [W, H],
                           "parallelism": f"camera-sharded x{rk.world}"},
                "rccl_ranks": nranks, "ranks_seen": rk.seen(),
                "p50_latency_ms": round(float(np.median(lat)) * 1e3, 3),
                "published_frac": round(published[0] / max(1, a.rigs * a.steps), 4),
                "published_rig_poses_per_s": round(published[0] / elapsed, 3),
                "gn_iterations_per_rig": round(gn_its[0] / max(1, a.rigs * a.steps), 3),
                "roofline": roof}
    pool.shutdown()
    for mc in ctxs:
        mc.close()
    return line


# -------------------------------------------------------------------- config 2
def run_config2(a, rk):
    """1280x720 single-camera stream (BASELINE configs[1], SURVEY §8 d config 2)."""
    import mantis_amd as M
    from mantis_amd import dense, synth

    W, H = 1280, 720
    K, D = synth.intrinsics(W, H)
    nf, B = max(1, a.stream_frames), max(1, min(a.stream_batch, a.stream_frames))
    m = make_ctx(M, rk, max_cams=B, max_width=W, max_height=H)
    m.set_map(*synth.load_map())
    rng = np.random.default_rng(2000 + rk.rank)
    nd = min(nf, a.distinct)
    fb = W * H * 3
    dev = m.device_alloc(nd * fb)
    poses = [synth.random_pose(rng) for _ in range(nd)]
    m.synth_render([synth.make_cam(R, pos, W, H) for R, pos in poses],
                   [synth.frame_seed(2, i + 100000 * rk.rank) for i in range(nd)], dev)
    m.synchronize()
    imgs = [M.make_image(None, K, D, device_ptr=dev + (i % nd) * fb, width=W, height=H) for i in range(nf)]
    # (i) the ROS callback: one mantis_process call per frame, cv::RNG carried
    for i in range(min(a.warmup, nf)):
        m.process_motion([imgs[i]])
    m.rng_state = 1
    lat, pub = [], 0
    rk.barrier()
    m.synchronize()
    t0 = time.perf_counter()
    for i in range(nf):
        t1 = time.perf_counter()
        out, _ = m.process_motion([imgs[i]])
        lat.append(time.perf_counter() - t1)
        pub += out.publish
    el_stream = rk.max(time.perf_counter() - t0)
    pub_all = rk.sum(pub)
    rng_stream = m.rng_state
    # (ii) the same frames batched, the RNG stream carried identically
    m.rng_state = 1
    batches = [M.Batch(m, imgs[k:k + B], len(imgs[k:k + B])) for k in range(0, nf, B)]
    rk.barrier()
    t0 = time.perf_counter()
    pub_b = 0
    for b in batches:
        b.run()
        pub_b += sum(r.publish for r in b.out)
    el_batch = rk.max(time.perf_counter() - t0)
    same_rng = m.rng_state == rng_stream and pub_b == pub
    # (iii) 256-hypothesis scoring microbatch (truth + N(0, 0.03 rad / 0.01 m)), fast path, cleaned mask
    R0, p0 = poses[0]
    hyps = [synth.truth_c2w(R0, p0)]
    hr = np.random.default_rng(1)
    while len(hyps) < 256:
        g = hr.normal(size=6)
        Rp = R0 @ synth.rot_z(g[0] * 0.03) @ synth.rot_y(g[1] * 0.03) @ synth.rot_x(g[2] * 0.03)
        hyps.append(synth.truth_c2w(Rp, p0 + g[3:] * 0.01))
    hyps = np.ascontiguousarray(np.array(hyps).reshape(256, 12), np.float64)
    _, mask = m.masks(imgs[0])
    d_h, d_m = m.device_alloc(hyps.nbytes), m.device_alloc(mask.nbytes)
    m.h2d(d_h, hyps)
    m.h2d(d_m, np.ascontiguousarray(mask, np.uint8))
    for _ in range(3):
        m.score_argmin_dev(imgs[0], d_h, 256, 0, False, d_m)
    m.set_profiling(True)
    kt = 0.0
    t0 = time.perf_counter()
    for _ in range(a.microbatches):
        m.score_argmin_dev(imgs[0], d_h, 256, 0, False, d_m)
        kt += dict(m.kernel_times()).get("score_dense", 0.0)
    el_mb = time.perf_counter() - t0
    m.set_profiling(False)
    line = None
    if rk.rank == 0:
        kavg = kt / max(1, a.microbatches)
        alg_b = 6 * W * H + 3 * LANDMARKS * 256  # SURVEY §8 d: 6,082,560 B per microbatch
        flops = FLOPS_PER_PROJ * LANDMARKS * 256
        line = {"metric": "1280x720 single-camera stream, poses/s + p50 per-frame latency (config 2)",
                "value": round(nf * rk.world / el_stream, 3), "unit": "frames/s", "n_gpus": rk.world,
                "steps": nf, "warmup": a.warmup, "ms_per_step": round(el_stream / nf * 1e3, 4),
                "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
                "data": f"synthetic fisheye grid frames rendered in HBM ({nd} distinct), map.yaml landmarks",
                "config": {"workload": "config2: 1280x720 single camera, full mantis3 callback per frame "
                                       "(mantis_process), cv::RNG carried across frames",
                           "frames": nf, "resolution": [W, H], "parallelism": f"replicas x{rk.world}"},
                "p50_latency_ms": round(float(np.median(lat)) * 1e3, 3),
                "p99_latency_ms": round(float(np.percentile(lat, 99)) * 1e3, 3),
                "published_frac": round(pub / nf, 4),
                "published_frames_per_s": round(pub_all / el_stream, 3),
                "batched_stream": {"value": round(nf * rk.world / el_batch, 2), "unit": "frames/s",
                                   "frames_per_call": B, "identical_rng_and_publish_count": bool(same_rng)},
                "microbatch_256": {"value": round(256 * a.microbatches / el_mb, 1), "unit": "hypotheses/s",
                                   "calls": a.microbatches, "ms_per_call": round(el_mb / a.microbatches * 1e3, 4),
                                   "roofline": {"bound": "hbm", "kernel": "k_score_api",
                                                "achieved": round(alg_b / (kavg * 1e-3) / 1e9, 2) if kavg else None,
                                                "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                                "frac": round(alg_b / (kavg * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if kavg else None,
                                                "traffic": None, "alg_bytes_per_launch": alg_b,
                                                "avg_launch_ms": round(kavg, 5),
                                                "fp64_frac": round(flops / (kavg * 1e-3) / 1e12 / FP64_PEAK_TFLOPS, 5) if kavg else None}}}
    m.close()
    return line


# -------------------------------------------------------------------- config 5
def run_config5(a, rk):
    """16,200-hypothesis dense grid per frame, hypotheses sharded across ranks."""
    import mantis_amd as M
    from mantis_amd import dense, synth

    W, H = 1280, 720
    K, D = synth.intrinsics(W, H)
    nf = max(1, a.frames)
    m = make_ctx(M, rk, max_cams=nf, max_width=W, max_height=H)  # a batch call stages every frame of a step
    m.set_map(*synth.load_map())
    m.comm_init(rk.rank, rk.world, rk.dist)
    nranks, _ = m.comm_info()
    rng = np.random.default_rng(2024)
    fb = W * H * 3
    dev = m.device_alloc(nf * fb)
    work = []
    for f in range(nf):
        R, pos = synth.random_pose(rng)
        m.synth_render([synth.make_cam(R, pos, W, H)], [synth.frame_seed(5, f)], dev + f * fb)
        m.synchronize()
        img = M.make_image(None, K, D, device_ptr=dev + f * fb, width=W, height=H)
        _, mask = m.masks(img)
        hyps = dense.config5_hypotheses(R, pos, np.random.default_rng(7 + f))
        lo, hi = dense.shard_range(len(hyps), rk.rank, rk.world)
        mine = np.ascontiguousarray(hyps[lo:hi], np.float64)
        # hypotheses and mask resident in HBM like the frames (mantis_score_argmin_dev)
        d_h = m.device_alloc(max(1, mine.nbytes))
        d_m = m.device_alloc(mask.nbytes)
        if len(mine):
            m.h2d(d_h, mine)
        m.h2d(d_m, np.ascontiguousarray(mask, np.uint8))
        work.append((img, (d_m, d_h), len(mine), lo, len(hyps)))

    # every frame of a step in one call (mantis_score_argmin_batch: one scoring
    # launch over all frames' hypothesis blocks, one argmin per frame, one
    # all-gather of the per-frame pairs)
    imgs5 = [w[0] for w in work]
    hd = [w[1][1] for w in work]
    md = [w[1][0] for w in work]
    ns = [w[2] for w in work]
    bases = [w[3] for w in work]

    def step():
        return m.score_argmin_batch(imgs5, hd, ns, bases, True, md)

    for _ in range(a.warmup):
        step()
    m.set_profiling(True)
    kt = 0.0
    rk.barrier()
    m.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
        kt += dict(m.kernel_times()).get("score_dense", 0.0)
    m.synchronize()
    rk.barrier()
    elapsed = rk.max(time.perf_counter() - t0)
    best0 = step()[0]  # every rank takes part in the exchange
    line = None
    if rk.rank == 0:
        n_h = sum(w[4] for w in work)
        kavg = kt / a.steps  # one launch per step over all frames
        flops = FLOPS_PER_PROJ * float(LANDMARKS) * sum(w[2] for w in work)
        ach = flops / (kavg * 1e-3) / 1e12 if kavg > 0 else 0.0
        line = {"metric": "dense hypothesis scoring (config 5), hypotheses/s",
                "value": round(n_h * a.steps / elapsed, 1), "unit": "hypotheses/s", "n_gpus": rk.world,
                "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(elapsed / a.steps * 1e3, 4),
                "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
                "data": "synthetic fisheye grid frames, hypotheses and masks resident in HBM, map.yaml landmarks",
                "config": {"workload": "config5: 1280x720, 81 shifts x 4 yaws x 50 perturbations per frame, "
                                       "all frames of a step in one mantis_score_argmin_batch call",
                           "frames_per_step": nf, "hypotheses_per_frame": work[0][4], "landmarks": LANDMARKS,
                           "parallelism": f"hypothesis-sharded x{rk.world}"},
                "rccl_ranks": nranks, "ranks_seen": rk.seen(),
                "best_frame0": list(best0),
                "published_note": "no publish gate on this path: every call returns its frames' first-minimum "
                                  "hypotheses (mantis_score_argmin_batch), so hypotheses/s has no published subset",
                "roofline": {"bound": "valu", "kernel": "k_score_api_batch", "achieved": round(ach, 4),
                             "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / FP64_PEAK_TFLOPS, 5),
                             "traffic": None, "avg_launch_ms": round(kavg, 4), "alg_flops_per_launch": int(flops),
                             "bound_note": "FP32 screen + exact FP64 fallback on the VALU (the scorers' kernel body): "
                                           "frac counts the reference's 51 algorithmic FP64 flops per landmark "
                                           "projection against the FP64 vector peak"}}
    m.close()
    return line


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch(a)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus:
        print(f"bench: --gpus {a.gpus} but WORLD_SIZE={world} (run under torchrun with --nproc-per-node "
              f"{a.gpus}, or without torchrun to let bench.py spawn the ranks)", file=sys.stderr)
        return 2
    # before HIP initialises; never below what the environment already grants, at most 32
    try:
        env_q = int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))
    except ValueError:
        env_q = 4
    os.environ["GPU_MAX_HW_QUEUES"] = str(min(32, max(4, env_q, a.hw_queues)))
    if a.dump_outputs and a.config != 3:
        print("bench: --dump-outputs is for config 3", file=sys.stderr)
        return 2
    cpu = None
    if a.full and a.config == 3 and world == 1 and not a.no_cpu:
        try:
            cpu = cpu_baseline(a, 1280, 720, 4)  # before any GPU work: nothing else runs on the host cores
        except Exception as e:  # the oracle is optional on a box without it
            cpu = {"value": None, "unit": "rig poses/s", "cores": 0, "kind": "port", "sample": f"unavailable: {e}"}
    rk = Ranks()
    line = {2: lambda: run_config2(a, rk), 3: lambda: run_config3(a, rk, cpu), 4: lambda: run_config4(a, rk),
            5: lambda: run_config5(a, rk)}[a.config]()
    if line is not None:
        print(json.dumps(line), flush=True)
    rk.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
