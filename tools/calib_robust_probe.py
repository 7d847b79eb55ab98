"""Latency and accuracy of the calibrations' robust rows (GPU box), by the
protocol of tools/calib_probe.py.

`views` views (8 and 32) of one 4-camera 1280x720 rig with device-resident
frames rendered through the nominal lenses and extrinsics, except one frame:
view 1, camera 3 is rendered from a camera knocked by 3 cm along y and 1 degree
about z. Every mantis_image carries the nominal K, D and T_base_cam, and every
call starts from the truth moved by 2 cm and 1 degree. For each of the three
calibrations (extrinsic with cameras 1-3 free; intrinsic with all cameras free;
rig with both) after `warmup` calls of each form, `rounds` alternating blocks
of `calls` calls of each form -- plain (the switch off, the yardstick), Huber,
Tukey -- host submit -> result on host, then per form one profiled call of its
own for the stage events per kernel (the two histogram launches are the
`*_hist` stage; the weight staging is what `*_rig` costs beyond the plain
call's), and the distances to the truth at the default 4 iterations and at 10.

    python tools/calib_robust_probe.py [--views 8 32] [--warmup 5] [--calls 10] [--rounds 2] [--out FILE]

--out appends the JSON line to FILE (profiles/calib_robust_probe.json).
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


def dist(kd, x, y):
    r = np.sqrt(x * x + y * y)
    th = np.arctan(r)
    thd = th + kd[4] * th ** 3 + kd[5] * th ** 5 + kd[6] * th ** 7 + kd[7] * th ** 9
    cd = np.where(r > 1e-8, thd / np.where(r > 1e-8, r, 1.0), 1.0)
    return x * cd * kd[0] + kd[2], y * cd * kd[1] + kd[3]


def model_gap(kd, kd_true, w, h):
    gx, gy = np.meshgrid(np.linspace(-2.2, 2.2, 23), np.linspace(-1.3, 1.3, 14))
    ut, vt = dist(kd_true, gx, gy)
    inside = (ut >= 0) & (ut <= w - 1) & (vt >= 0) & (vt <= h - 1)
    u, v = dist(kd, gx, gy)
    return float(np.sqrt(((u - ut) ** 2 + (v - vt) ** 2)[inside].mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="calls of each form per block")
    ap.add_argument("--rounds", type=int, default=2, help="alternating blocks of each form")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()

    import mantis_amd as M
    from mantis_amd import synth

    W, H, CAMS, ALL, FREE_EXT = 1280, 720, 4, 0b1111, 0b1110
    KNOCK_VIEW, KNOCK_CAM = 1, 3
    NV = max(a.views)
    K, D = synth.intrinsics(W, H)
    f32 = lambda v: float(np.float32(v))
    kd0 = np.array([f32(K[0, 0]), f32(K[1, 1]), f32(K[0, 2]), f32(K[1, 2])] + list(D))
    ext = [np.array(e) for e in synth.rig_extrinsics(CAMS)]
    knock = np.eye(4)
    knock[:3, :3] = synth.rot_z(math.radians(1.0))
    knock[:3, 3] = [0.0, 0.03, 0.0]
    shift = np.eye(4)
    shift[:3, :3] = synth.rot_z(math.radians(1.0))
    shift[:3, 3] = [0.02, 0.0, 0.0]
    rng = np.random.default_rng(1000)
    cams, truth, pred = [], [], []
    for r in range(NV):
        Twb = synth.random_base_pose(rng)
        truth.append(Twb)
        pred.append(Twb @ shift)
        for c in range(CAMS):
            Twc = Twb @ (knock if (r, c) == (KNOCK_VIEW, KNOCK_CAM) else np.eye(4)) @ ext[c]
            cams.append(synth.make_cam(Twc[:3, :3], Twc[:3, 3], W, H))
    m = M.Mantis(max_cams=NV * CAMS, max_width=W, max_height=H)
    m.set_map(*synth.load_map())
    fb = W * H * 3
    dev = m.device_alloc(len(cams) * fb)
    m.synth_render(cams, [synth.frame_seed(3, i) for i in range(len(cams))], dev)
    m.synchronize()
    given = [M.make_image(None, K, D, T_base_cam=ext[i % CAMS], device_ptr=dev + i * fb, width=W, height=H)
             for i in range(len(cams))]

    calls = {"calib": lambda imgs, N, T0, **kw: m.calibrate_extrinsics(imgs, N, T0, FREE_EXT, **kw),
             "icalib": lambda imgs, N, T0, **kw: m.calibrate_intrinsics(imgs, N, T0, ALL, **kw),
             "rcalib": lambda imgs, N, T0, **kw: m.calibrate_rig(imgs, N, T0, FREE_EXT, ALL, **kw)}
    kinds = {"calib": 0, "icalib": 1, "rcalib": 2}
    forms = (None, "huber", "tukey")
    name_of = lambda loss: loss or "plain"

    def figures(kind, T, res, N):
        """Distances to the truth of one result."""
        out = {"status": res.status, "calibrated": res.calibrated, "iterations_run": res.iterations_run,
               "rms_px": round(res.rms[res.iterations_run] * kd0[0], 4)}
        perr = [pose_error(T[r], truth[r])[0] for r in range(N)]
        out["pose_err_m_median_worst"] = [round(float(np.median(perr)), 6), round(float(np.max(perr)), 6)]
        out["pose_err_m_knocked_view"] = round(perr[KNOCK_VIEW], 6)
        if kind != "icalib":
            E = np.array([list(res.T_base_cam[c]) for c in range(CAMS)]).reshape(CAMS, 4, 4)
            out["ext_err_m"] = [round(pose_error(E[c], ext[c])[0], 6) for c in range(CAMS)]
        if kind != "calib":
            kds = np.array([list(res.K[c]) + list(res.D[c]) for c in range(CAMS)])
            out["model_gap_px"] = [round(model_gap(kds[c], kd0, W, H), 4) for c in range(CAMS)]
        return out

    line = {"cams_per_rig": CAMS, "free_ext": FREE_EXT, "free_int": ALL, "knocked": [KNOCK_VIEW, KNOCK_CAM],
            "knock_m_deg": [0.03, 1.0], "warmup": a.warmup, "calls_each": a.rounds * a.calls,
            "start_err_m_deg": [round(x, 5) for x in pose_error(pred[0], truth[0])]}
    for N in a.views:
        imgs, T0 = given[: N * CAMS], np.array(pred[:N])
        per_views = {}
        for kind, fn in calls.items():
            def timed(loss, **kw):
                m.set_calib_robust(loss)
                t0 = time.perf_counter()
                out = fn(imgs, N, T0, **kw)
                return time.perf_counter() - t0, out

            for loss in forms:
                for _ in range(a.warmup):
                    timed(loss)
            lat = {loss: [] for loss in forms}
            last = {}
            for _ in range(a.rounds):
                for loss in forms:
                    for _ in range(a.calls):
                        dt, last[loss] = timed(loss)
                        lat[loss].append(dt)
            rec = {}
            for loss in forms:
                m.set_profiling(True)
                timed(loss)
                kern = {}
                for name, ms in m.kernel_times():
                    kern[name] = kern.get(name, 0.0) + ms
                launches = len(m.kernel_times())
                m.set_profiling(False)
                T, res = last[loss]
                _, (T10, res10) = timed(loss, iterations=10)
                entry = {"p50_ms": round(float(np.median(lat[loss])) * 1e3, 3), "launches": launches,
                         "kernel_ms_per_call": {k: round(v, 4) for k, v in kern.items()},
                         "iterations_4": figures(kind, T, res, N), "iterations_10": figures(kind, T10, res10, N)}
                if loss:
                    st = m.calib_robust_stats(kinds[kind])
                    fp = res10.iterations_run
                    entry["iterations_10"].update({
                        "scale": [round(v, 4) for v in list(st.scale)[: fp + 1]],
                        "n_down_zero_obs": [st.n_down[fp], st.n_zero[fp], res10.n_obs[fp]],
                        "mean_weight_view_knocked_min_other": [
                            round(st.sum_w_view[KNOCK_VIEW] / st.n_obs_view[KNOCK_VIEW], 4),
                            round(min(st.sum_w_view[r] / st.n_obs_view[r] for r in range(N) if r != KNOCK_VIEW), 4)],
                        "mean_weight_cam": [round(st.sum_w_cam[c] / res10.n_obs_cam[fp][c], 4) for c in range(CAMS)]})
                rec[name_of(loss)] = entry
            m.set_calib_robust(None)
            per_views[kind] = rec
        line[f"views_{N}"] = per_views
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")
    m.device_free(dev)
    m.close()


if __name__ == "__main__":
    main()
