"""Latency and accuracy of the extrinsic calibration (GPU box), by the protocol
of tools/refine_probe.py.

`views` views (8 and 32) of one 4-camera 1280x720 rig with device-resident
frames, camera 3 rendered through drift @ ext[3] (tools/refine_robust_probe.py's
drift: 0.4 degrees about z, 1.2 cm along y) while every mantis_image carries the
nominal ext[3]. After `warmup` calls of each kind, `rounds` alternating blocks
of `calls` calls of each kind, host submit -> result on host:
  calib         mantis_calibrate_extrinsics, cameras 1-3 free, from the truth
                moved by 2 cm and 1 degree
  refine_batch  mantis_refine_batch on the same frames from the same poses (the
                yardstick, timed in the same run)
and the stage events of the calibration's three kernels from a profiled call
of its own, the extrinsics' and the poses' distances to the truth before and
after, and mantis_refine_batch's pose error with the given and with the
calibrated extrinsics.

    python tools/calib_probe.py [--views 8 32] [--warmup 5] [--calls 10] [--rounds 2] [--out FILE]
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
    ap.add_argument("--views", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="calls of each kind per block")
    ap.add_argument("--rounds", type=int, default=2, help="alternating blocks of each kind")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import mantis_amd as M
    from mantis_amd import synth

    W, H, CAMS, FREE = 1280, 720, 4, 0b1110
    NV = max(a.views)
    K, D = synth.intrinsics(W, H)
    rng = np.random.default_rng(1000)
    ext = synth.rig_extrinsics(CAMS)
    drift = np.eye(4)
    drift[:3, :3] = synth.rot_z(math.radians(0.4))
    drift[:3, 3] = [0.0, 0.012, 0.0]
    ext_true = [np.array(e) for e in ext]
    ext_true[CAMS - 1] = drift @ ext_true[CAMS - 1]
    shift = np.eye(4)
    shift[:3, :3] = synth.rot_z(math.radians(1.0))
    shift[:3, 3] = [0.02, 0.0, 0.0]
    cams, truth, pred = [], [], []
    for r in range(NV):
        Twb = synth.random_base_pose(rng)
        truth.append(Twb)
        pred.append(Twb @ shift)
        for c in range(CAMS):
            Twc = Twb @ ext_true[c]
            cams.append(synth.make_cam(Twc[:3, :3], Twc[:3, 3], W, H))
    m = M.Mantis(max_cams=NV * CAMS, max_width=W, max_height=H)
    m.set_map(*synth.load_map())
    fb = W * H * 3
    dev = m.device_alloc(len(cams) * fb)
    m.synth_render(cams, [synth.frame_seed(3, i) for i in range(len(cams))], dev)
    m.synchronize()

    def images(exts):
        return [M.make_image(None, K, D, T_base_cam=exts[i % CAMS], device_ptr=dev + i * fb, width=W, height=H)
                for i in range(len(cams))]

    given = images(ext)
    line = {"cams_per_rig": CAMS, "free_cams": FREE, "warmup": a.warmup, "calls_each": a.rounds * a.calls,
            "start_err_m_deg": [round(x, 5) for x in pose_error(pred[0], truth[0])],
            "ext_err_before_m_deg": [[round(x, 5) for x in pose_error(np.array(ext[c]), ext_true[c])] for c in range(CAMS)]}
    for N in a.views:
        imgs, T0 = given[: N * CAMS], np.array(pred[:N])

        def calib_call():
            t0 = time.perf_counter()
            T, res = m.calibrate_extrinsics(imgs, N, T0, FREE)
            return time.perf_counter() - t0, (T, res)

        def refine_call():
            t0 = time.perf_counter()
            out = m.refine_batch(imgs, N, T0)
            return time.perf_counter() - t0, out

        kinds = {"calib": calib_call, "refine_batch": refine_call}
        for fn in kinds.values():
            for _ in range(a.warmup):
                fn()
        lat = {k: [] for k in kinds}
        last = {}
        for _ in range(a.rounds):
            for name, fn in kinds.items():
                for _ in range(a.calls):
                    dt, last[name] = fn()
                    lat[name].append(dt)
        m.set_profiling(True)
        m.calibrate_extrinsics(imgs, N, T0, FREE)
        kern = {}
        for name, ms in m.kernel_times():
            kern[name] = kern.get(name, 0.0) + ms
        launches = len(m.kernel_times())
        m.set_profiling(False)
        T, res = last["calib"]
        E = np.array([list(res.T_base_cam[c]) for c in range(CAMS)]).reshape(CAMS, 4, 4)
        after = m.refine_batch(images(list(E))[: N * CAMS], N, T0)
        t0 = time.perf_counter()
        T10, res10 = m.calibrate_extrinsics(imgs, N, T0, FREE, iterations=10)  # untimed but for this one call
        ms10 = (time.perf_counter() - t0) * 1e3
        E10 = np.array([list(res10.T_base_cam[c]) for c in range(CAMS)]).reshape(CAMS, 4, 4)
        after10 = m.refine_batch(images(list(E10))[: N * CAMS], N, T0)
        perr = lambda Ts: [pose_error(Ts[r], truth[r])[0] for r in range(N)]
        Tof = lambda rr: np.array(rr.T_w_b).reshape(4, 4)
        p50 = {k: float(np.median(v)) * 1e3 for k, v in lat.items()}
        total = sum(kern.values())
        solve = sum(v for k, v in kern.items() if k.startswith("calib_solve"))
        line[f"views_{N}"] = {
            "calib_p50_ms": round(p50["calib"], 3), "refine_batch_p50_ms": round(p50["refine_batch"], 3),
            "status": res.status, "calibrated": res.calibrated, "iterations_run": res.iterations_run,
            "n_obs": list(res.n_obs)[: res.iterations_run + 1],
            "rms_px": [round(v * float(np.float32(K[0, 0])), 4) for v in list(res.rms)[: res.iterations_run + 1]],
            "rms_cam_px": [round(v * float(np.float32(K[0, 0])), 4) for v in list(res.rms_cam)[:CAMS]],
            "launches": launches, "kernel_ms_per_call": {k: round(v, 4) for k, v in kern.items()},
            "solve_share_of_kernels": round(solve / total, 4) if total else None,
            "solve_share_of_call": round(solve / p50["calib"], 4),
            "ext_err_after_m_deg": [[round(x, 5) for x in pose_error(E[c], ext_true[c])] for c in range(CAMS)],
            "pose_err_m_median_worst": {
                "start": [round(float(np.median(perr(T0))), 6), round(float(np.max(perr(T0))), 6)],
                "calib": [round(float(np.median(perr(T))), 6), round(float(np.max(perr(T))), 6)],
                "refine_given_ext": [round(float(np.median(perr([Tof(x) for x in last["refine_batch"]]))), 6),
                                     round(float(np.max(perr([Tof(x) for x in last["refine_batch"]]))), 6)],
                "refine_calibrated_ext": [round(float(np.median(perr([Tof(x) for x in after]))), 6),
                                          round(float(np.max(perr([Tof(x) for x in after]))), 6)]},
            "iterations_10": {
                "one_call_ms": round(ms10, 3), "status": res10.status, "calibrated": res10.calibrated,
                "iterations_run": res10.iterations_run,
                "rms_px": [round(v * float(np.float32(K[0, 0])), 4) for v in list(res10.rms)[: res10.iterations_run + 1]],
                "ext_err_after_m_deg": [[round(x, 5) for x in pose_error(E10[c], ext_true[c])] for c in range(CAMS)],
                "pose_err_m_median_worst": {
                    "calib": [round(float(np.median(perr(T10))), 6), round(float(np.max(perr(T10))), 6)],
                    "refine_calibrated_ext": [round(float(np.median(perr([Tof(x) for x in after10]))), 6),
                                              round(float(np.max(perr([Tof(x) for x in after10]))), 6)]}}}
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
