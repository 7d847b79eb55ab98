"""Latency and accuracy of the line refinement with robust rows (GPU box), by
the protocol of tools/refine_probe.py.

Over `rigs` distinct 4-camera 1280x720 rigs with device-resident frames (the
scenes of tools/refine_probe.py), after `warmup` calls of each kind, `rounds`
alternating blocks of `rigs` calls of each kind, host submit -> result on host:
  plain   mantis_refine from the truth moved by 2 cm and 1 degree
  huber   the same call after mantis_refine_set_robust(loss = 1)
  tukey   the same call after mantis_refine_set_robust(loss = 2)
and, from the first block, the median and worst distance of each result to the
synthetic truth, on the clean rigs and on the same rigs with camera 3 rendered
from the base pose displaced by 1.2 cm along y and 0.4 degrees about z (a
camera whose extrinsic has drifted); the stage events of k_refine_step and
k_refine_step_robust from profiled passes of their own. The plain call is the
yardstick, timed in the same run.

    python tools/refine_robust_probe.py [--rigs 32] [--warmup 10] [--rounds 2] [--out FILE]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pose_error(T_est, T_true):
    """(translation error in m, rotation error in degrees)"""
    dt = float(np.linalg.norm(T_est[:3, 3] - T_true[:3, 3]))
    c = (np.trace(T_true[:3, :3].T @ T_est[:3, :3]) - 1.0) / 2.0
    return dt, math.degrees(math.acos(max(-1.0, min(1.0, c))))


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
    shift = np.eye(4)
    shift[:3, :3] = synth.rot_z(math.radians(1.0))
    shift[:3, 3] = [0.02, 0.0, 0.0]
    drift = np.eye(4)
    drift[:3, :3] = synth.rot_z(math.radians(0.4))
    drift[:3, 3] = [0.0, 0.012, 0.0]
    cams, Tbc, truth, pred = {"clean": [], "drifted": []}, [], [], []
    for r in range(a.rigs):
        Twb = synth.random_base_pose(rng)
        truth.append(Twb)
        pred.append(Twb @ shift)
        for c in range(CAMS):
            for kind in cams:
                Twc = (Twb @ drift if kind == "drifted" and c == CAMS - 1 else Twb) @ ext[c]
                cams[kind].append(synth.make_cam(Twc[:3, :3], Twc[:3, 3], W, H))
            Tbc.append(ext[c])
    m = M.Mantis(max_cams=CAMS, max_width=W, max_height=H)
    m.set_map(*synth.load_map())
    fb = W * H * 3
    n = a.rigs * CAMS
    dev = m.device_alloc(2 * n * fb)
    seeds = [synth.frame_seed(3, i) for i in range(n)]
    m.synth_render(cams["clean"], seeds, dev)
    m.synth_render(cams["drifted"], seeds, dev + n * fb)
    m.synchronize()
    imgs = {kind: [M.make_image(None, K, D, T_base_cam=Tbc[i], device_ptr=dev + (s * n + i) * fb, width=W, height=H)
                   for i in range(n)] for s, kind in enumerate(cams)}
    rig = lambda kind, r: imgs[kind][r * CAMS:(r + 1) * CAMS]
    Tof = lambda rr: np.array(rr.T_w_b).reshape(4, 4)
    losses = {"plain": None, "huber": "huber", "tukey": "tukey"}

    def call(loss, scene, r):
        m.set_refine_robust(losses[loss])  # host only: kept outside the timed span
        m.prior_pose = pred[r]
        t0 = time.perf_counter()
        out, rout = m.refine(rig(scene, r))
        return time.perf_counter() - t0, Tof(rout), rout.refined

    for loss in losses:
        for k in range(a.warmup):
            call(loss, "clean", k % a.rigs)
    lat = {k: [] for k in losses}
    for rnd in range(a.rounds):
        for loss in losses:
            for r in range(a.rigs):
                lat[loss].append(call(loss, "clean", r)[0])
    err = {s: {k: {} for k in losses} for s in cams}
    good = {s: {k: 0 for k in losses} for s in cams}
    for scene in cams:
        for loss in losses:
            for r in range(a.rigs):
                _, T, ok = call(loss, scene, r)
                good[scene][loss] += int(bool(ok))
                err[scene][loss][r] = pose_error(T, truth[r])
    # stage events of the step kernels: a profiled pass per form
    m.set_profiling(True)
    st, launches = {}, {}
    for loss in losses:
        for r in range(a.rigs):
            call(loss, "clean", r)
            launches[loss] = sum(nm.startswith("refine_") for nm, _ in m.kernel_times())
            for name, ms in m.stage_times():
                st.setdefault(loss + ":" + name, []).append(ms)
    m.set_profiling(False)
    m.set_refine_robust(None)

    def stat(v, i):
        xs = [x[i] for x in v.values()]
        return [round(float(np.median(xs)), 6), round(float(np.max(xs)), 6)]

    worst = max(err["clean"]["plain"], key=lambda r: err["clean"]["plain"][r][0])
    line = {"rigs": a.rigs, "cams_per_rig": CAMS, "warmup": a.warmup, "calls_each": a.rounds * a.rigs,
            "start_err_m_deg": [round(x, 5) for x in pose_error(pred[0], truth[0])],
            "refine_launches": launches,
            "stage_median_ms_per_call": {k: round(float(np.median(v)), 4) for k, v in st.items()},
            "plain_worst_rig": worst,
            "plain_worst_rig_err_m_deg": {k: [round(x, 6) for x in err["clean"][k][worst]] for k in losses}}
    for loss in losses:
        line[loss + "_p50_ms"] = round(float(np.median(lat[loss])) * 1e3, 3)
        for scene in cams:
            line[f"{scene}_{loss}_ok"] = good[scene][loss]
            line[f"{scene}_{loss}_err_m_median_worst"] = stat(err[scene][loss], 0)
            line[f"{scene}_{loss}_err_deg_median_worst"] = stat(err[scene][loss], 1)
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")
    m.device_free(dev)
    m.close()


if __name__ == "__main__":
    main()
