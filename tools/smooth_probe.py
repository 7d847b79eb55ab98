"""Latency and accuracy of the window smoother (GPU box), by the protocol of
tools/refine_probe.py.

Windows of 8 and 32 views of the four-camera 1280x720 rig with device-resident
frames; the views are chained by the 8 cm / 3 degree step and all start 2 cm /
1 degree off; the middle view is black. After `warmup` calls of each kind,
`rounds` alternating blocks of `calls` calls of each kind, host submit ->
result on host:
  smooth   mantis_smooth_batch on the window (exact motions)
  refine   mantis_refine_batch on the same views as independent rigs
and the stage events of one profiled call per kernel; the blind view's and the
sighted views' errors with exact motions and with motions perturbed at the
default sigmas (1 cm, 0.03 rad). k_smooth_solve alone at N = 32 and 256
(one-camera 322x242 views, one iteration), which is where the chain shows
(--only-solve runs that part alone; `lib` in the line names the library
loaded, so a build under comparison can be given through MANTIS_AMD_LIB).

    python tools/smooth_probe.py [--warmup 3] [--rounds 2] [--calls 10] [--only-solve] [--out profiles/smooth_probe.json]

Appends one JSON line to --out.
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
    dt = float(np.linalg.norm(T_est[:3, 3] - T_true[:3, 3]))
    c = (np.trace(T_true[:3, :3].T @ T_est[:3, :3]) - 1.0) / 2.0
    return dt, math.degrees(math.acos(max(-1.0, min(1.0, c))))


def quat_of(R):
    w = math.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2]) / 2.0
    return [(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w]


def exp_so3(phi):
    th = np.linalg.norm(phi)
    K = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * K @ K


def motion_of(D):
    return list(D[:3, 3]) + quat_of(D[:3, :3])


def trajectory(synth, n, step, start):
    T = [start]
    for _ in range(n - 1):
        T.append(T[-1] @ step)
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--only-solve", action="store_true", help="skip the 1280x720 windows: k_smooth_solve alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_probe.json"))
    a = ap.parse_args()

    import mantis_amd as M
    from mantis_amd import synth

    line = {"lib": os.path.basename(M.LIB_PATH), "warmup": a.warmup, "calls_each": a.rounds * a.calls}
    shift = np.eye(4)
    shift[:3, :3] = synth.rot_z(math.radians(1.0))
    shift[:3, 3] = [0.02, 0.0, 0.0]
    rng = np.random.default_rng(5)

    def window(N, CAMS, W, H, step, start, blind):
        K, D = synth.intrinsics(W, H)
        ext = synth.rig_extrinsics(CAMS)
        truth = trajectory(synth, N, step, start)
        cams = []
        for T in truth:
            for c in range(CAMS):
                Twc = T @ ext[c]
                cams.append(synth.make_cam(Twc[:3, :3], Twc[:3, 3], W, H))
        m = M.Mantis(max_cams=N * CAMS, max_width=W, max_height=H)
        m.set_map(*synth.load_map())
        fb = W * H * 3
        dev = m.device_alloc(len(cams) * fb)
        m.synth_render(cams, [synth.frame_seed(31, i) for i in range(len(cams))], dev)
        m.synchronize()
        black = np.zeros((H, W, 3), np.uint8)
        for k in blind:
            for c in range(CAMS):
                m.h2d(dev + (k * CAMS + c) * fb, black)
        imgs = [M.make_image(None, K, D, T_base_cam=ext[i % CAMS], device_ptr=dev + i * fb, width=W, height=H)
                for i in range(len(cams))]
        T0 = np.array([T @ shift for T in truth])
        exact = np.array([motion_of(step)] * (N - 1))
        noisy = []
        for _ in range(N - 1):
            Nz = np.eye(4)
            Nz[:3, :3] = exp_so3(rng.normal(0, 0.03, 3))
            Nz[:3, 3] = rng.normal(0, 0.01, 3)
            noisy.append(motion_of(step @ Nz))
        return m, dev, imgs, truth, T0, exact, np.array(noisy)

    step = np.eye(4)
    step[:3, :3] = synth.rot_z(math.radians(3.0))
    step[:3, 3] = [0.08, 0.0, 0.0]
    for N in (() if a.only_solve else (8, 32)):
        # the 32-view window turns through 93 degrees inside the arena: a shorter stride keeps it on the map
        st = step.copy()
        if N == 32:
            st[:3, 3] = [0.025, 0.0, 0.0]
        start = np.eye(4)
        start[:3, :3] = synth.rot_z(0.3)
        start[:3, 3] = [-0.3, -0.3, 1.4]
        blind = [N // 2]
        m, dev, imgs, truth, T0, exact, noisy = window(N, 4, 1280, 720, st, start, blind)
        kinds = {"smooth": lambda: m.smooth_batch(imgs, 1, N, T0, exact),
                 "refine": lambda: m.refine_batch(imgs, N, T0)}
        for fn in kinds.values():
            for _ in range(a.warmup):
                fn()
        lat = {k: [] for k in kinds}
        for _ in range(a.rounds):
            for name, fn in kinds.items():
                for _ in range(a.calls):
                    t0 = time.perf_counter()
                    fn()
                    lat[name].append(time.perf_counter() - t0)
        m.set_profiling(True)
        stages = {}
        for name, fn in kinds.items():
            fn()
            acc = {}
            for n_, ms in m.kernel_times():
                acc[n_] = acc.get(n_, 0.0) + ms
            stages[name] = {k: round(v, 4) for k, v in acc.items()}
        m.set_profiling(False)
        own = m.refine_batch(imgs, N, T0)
        rec = {"p50_ms": {k: round(float(np.median(v)) * 1e3, 3) for k, v in lat.items()},
               "stage_ms_per_call": stages,
               "refine_status": [r.status for r in own]}
        for name, mo in (("exact", exact), ("noisy", noisy)):
            res, views = m.smooth_batch(imgs, 1, N, T0, mo)
            errs = [pose_error(np.array(v.T_w_b).reshape(4, 4), truth[k]) for k, v in enumerate(views[0])]
            sighted = [e for k, e in enumerate(errs) if k not in blind]
            rec[name] = {"status": res[0].status, "smoothed": res[0].smoothed, "iterations_run": res[0].iterations_run,
                         "motion_rms": round(res[0].motion_rms[res[0].iterations_run], 4),
                         "blind_err_cm_deg": [round(100 * errs[blind[0]][0], 4), round(errs[blind[0]][1], 4)],
                         "sighted_err_cm_median_worst": [round(100 * float(np.median([e[0] for e in sighted])), 4),
                                                         round(100 * max(e[0] for e in sighted), 4)]}
        line[f"N{N}_C4_1280x720"] = rec
        m.device_free(dev)
        m.close()

    # the solve kernel alone, where the chain's length shows: one-camera 322 x 242 views, one iteration
    small = np.eye(4)
    small[:3, :3] = synth.rot_z(math.radians(1.3))
    small[:3, 3] = [0.003, 0.0, 0.0]
    for N in (32, 256):
        start = np.eye(4)
        start[:3, 3] = [-0.2, -0.2, 1.2]
        m, dev, imgs, truth, T0, exact, noisy = window(N, 1, 322, 242, small, start, [])
        for _ in range(a.warmup):
            m.smooth_batch(imgs, 1, N, T0, exact, iterations=1)
        m.set_profiling(True)
        ms = []
        for _ in range(a.calls):
            res, _ = m.smooth_batch(imgs, 1, N, T0, exact, iterations=1)
            # the first launch of k_smooth_solve is the pass that runs the chain; the second only assembles
            ms.append([t for n_, t in m.kernel_times() if n_.startswith("smooth_solve")])
        m.set_profiling(False)
        line[f"solve_N{N}_C1_322x242"] = {"status": res[0].status,
                                          "chain_pass_ms_p50": round(float(np.median([x[0] for x in ms])), 4),
                                          "final_pass_ms_p50": round(float(np.median([x[1] for x in ms])), 4)}
        m.device_free(dev)
        m.close()

    s = json.dumps(line)
    print(s)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
