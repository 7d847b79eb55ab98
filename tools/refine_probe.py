"""Latency and accuracy of the line refinement (GPU box), by the protocol of
tools/track_latency.py.

Over `rigs` distinct 4-camera 1280x720 rigs with device-resident frames,
after `warmup` calls of each kind, `rounds` alternating blocks of `rigs` calls
of each kind, host submit -> result on host:
  refine         mantis_refine from the truth moved by 2 cm and 1 degree
  track          mantis_track from the same prediction (default parameters)
  track+refine   mantis_track, then mantis_refine from the prior it left
  process        one-rig mantis_process
  process_gn     one-rig mantis_process on a context with cfg.gn_enable = 1
and, from the first block, the median and worst distance of each result to the
synthetic truth; the refinement's two kernels' stage events from a profiled
pass of its own. The yardsticks (track, process) are timed in the same run.

    python tools/refine_probe.py [--rigs 32] [--warmup 10] [--rounds 2] [--out FILE]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

# mantis_process replays hipGraphs on the rig-latency path only with the HIP
# runtime's graph packet capture off, as bench.py's p50 leg runs;
# the refinement captures no graph
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pose_error(T_est, T_true):
    """(translation error in m, rotation error in degrees)"""
    dt = float(np.linalg.norm(T_est[:3, 3] - T_true[:3, 3]))
    c = (np.trace(T_true[:3, :3].T @ T_est[:3, :3]) - 1.0) / 2.0
    return dt, math.degrees(math.acos(max(-1.0, min(1.0, c))))


def quat_T(q, p):
    x, y, z, w = q
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                 [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                 [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = p
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rigs", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2, help="alternating blocks of `rigs` calls of each kind")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import mantis_amd as M
    from mantis_amd import synth

    W, H, CAMS = 1280, 720, 4
    K, D = synth.intrinsics(W, H)
    rng = np.random.default_rng(1000)
    ext = synth.rig_extrinsics(CAMS)
    cams, Tbc, truth, pred = [], [], [], []
    shift = np.eye(4)
    shift[:3, :3] = synth.rot_z(math.radians(1.0))
    shift[:3, 3] = [0.02, 0.0, 0.0]
    for r in range(a.rigs):
        Twb = synth.random_base_pose(rng)
        truth.append(Twb)
        pred.append(Twb @ shift)
        for c in range(CAMS):
            Twc = Twb @ ext[c]
            cams.append(synth.make_cam(Twc[:3, :3], Twc[:3, 3], W, H))
            Tbc.append(ext[c])
    m = M.Mantis(max_cams=CAMS, max_width=W, max_height=H)
    m.set_map(*synth.load_map())
    mg = M.Mantis(max_cams=CAMS, max_width=W, max_height=H, gn_enable=1)
    mg.set_map(*synth.load_map())
    fb = W * H * 3
    dev = m.device_alloc(len(cams) * fb)
    m.synth_render(cams, [synth.frame_seed(3, i) for i in range(len(cams))], dev)
    m.synchronize()
    imgs = [M.make_image(None, K, D, T_base_cam=Tbc[i], device_ptr=dev + i * fb, width=W, height=H)
            for i in range(len(cams))]
    rig = lambda r: imgs[r * CAMS:(r + 1) * CAMS]
    Tof = lambda rr: np.array(rr.T_w_b).reshape(4, 4)

    def refine_call(r):
        m.prior_pose = pred[r]
        t0 = time.perf_counter()
        out, rout = m.refine(rig(r))
        return time.perf_counter() - t0, Tof(rout), rout.refined

    def track_call(r):
        m.prior_pose = pred[r]
        t0 = time.perf_counter()
        out, tout = m.track(rig(r))
        return time.perf_counter() - t0, Tof(tout), tout.tracked

    def track_refine_call(r):
        m.prior_pose = pred[r]
        t0 = time.perf_counter()
        out, tout = m.track(rig(r))  # tracked: the prior is now its pose
        out, rout = m.refine(rig(r))
        return time.perf_counter() - t0, Tof(rout), rout.refined

    def process_call(ctx):
        def call(r):
            ctx.prior_pose = None
            t0 = time.perf_counter()
            out, _ = ctx.process(rig(r), rigs=1)
            T = quat_T(list(out[0].orientation_xyzw), list(out[0].position)) if out[0].publish else None
            return time.perf_counter() - t0, T, out[0].publish
        return call

    kinds = {"refine": refine_call, "track": track_call, "track_refine": track_refine_call,
             "process": process_call(m), "process_gn": process_call(mg)}
    for fn in kinds.values():
        for k in range(a.warmup):
            fn(k % a.rigs)
    lat = {k: [] for k in kinds}
    err = {k: {} for k in kinds}
    good = {k: 0 for k in kinds}
    for rnd in range(a.rounds):
        for name, fn in kinds.items():
            for r in range(a.rigs):
                dt, T, ok = fn(r)
                lat[name].append(dt)
                if rnd == 0:
                    good[name] += int(bool(ok))
                    if ok and T is not None:
                        err[name][r] = pose_error(T, truth[r])
    # stage events of the refinement's kernels: a profiled pass of its own
    m.set_profiling(True)
    st, launches = {}, 0
    for r in range(a.rigs):
        m.prior_pose = pred[r]
        m.refine(rig(r))
        launches = sum(n.startswith("refine_") for n, _ in m.kernel_times())
        for name, ms in m.stage_times():
            st.setdefault(name, []).append(ms)
    m.set_profiling(False)

    def stat(v, i):
        xs = [x[i] for x in v.values()]
        return [round(float(np.median(xs)), 6), round(float(np.max(xs)), 6)] if xs else None

    line = {"rigs": a.rigs, "cams_per_rig": CAMS, "warmup": a.warmup, "calls_each": a.rounds * a.rigs,
            "start_err_m_deg": [round(x, 5) for x in pose_error(pred[0], truth[0])],
            "refine_launches": launches,
            "refine_stage_median_ms_per_call": {k: round(float(np.median(v)), 4) for k, v in st.items()}}
    for name in kinds:
        line[name + "_p50_ms"] = round(float(np.median(lat[name])) * 1e3, 3)
        line[name + "_ok"] = good[name]
        line[name + "_err_m_median_worst"] = stat(err[name], 0)
        line[name + "_err_deg_median_worst"] = stat(err[name], 1)
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")
    m.device_free(dev)
    mg.close()
    m.close()


if __name__ == "__main__":
    main()
