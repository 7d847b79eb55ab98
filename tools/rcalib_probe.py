"""Latency and accuracy of the rig calibration (GPU box), by the protocol of
tools/icalib_probe.py.

`views` views (8 and 32) of one 4-camera 1280x720 rig with device-resident
frames, every camera rendered through intrinsics beside the nominal ones (1 %
in fx and fy, 2 px in cx and cy, 0.004 in k1, 0.002 in k2, signs from
default_rng(7) per camera) and cameras 1-3 through extrinsics 1.2 cm / 0.69
degrees beside the nominal ones (signs from default_rng(11)), while every
mantis_image carries the nominal K, D and T_base_cam. After `warmup` calls of
each kind, `rounds` alternating blocks of `calls` calls of each kind, host
submit -> result on host:
  rcalib  mantis_calibrate_rig, ext 0b1110, int 0b1111, mask 0xFF, from the
          truth moved by 2 cm and 1 degree
  pair    one mantis_calibrate_extrinsics (cameras 1-3) plus one
          mantis_calibrate_intrinsics (all cameras) on the same frames from
          the same poses (the yardstick, timed in the same run)
and the stage events of the calibration's three kernels from a profiled call
of its own, the model gap, the extrinsics' and the poses' distances to the
truth before and after, and mantis_refine_batch's pose error with the nominal
and with the calibrated rig.

    python tools/rcalib_probe.py [--views 8 32] [--warmup 5] [--calls 10] [--rounds 2] [--out FILE]
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
    ap.add_argument("--calls", type=int, default=10, help="calls of each kind per block")
    ap.add_argument("--rounds", type=int, default=2, help="alternating blocks of each kind")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import mantis_amd as M
    from mantis_amd import synth

    W, H, CAMS, ALL, FREE_EXT = 1280, 720, 4, 0b1111, 0b1110
    NV = max(a.views)
    K, D = synth.intrinsics(W, H)
    f32 = lambda v: float(np.float32(v))
    kd0 = np.array([f32(K[0, 0]), f32(K[1, 1]), f32(K[0, 2]), f32(K[1, 2])] + list(D))
    sg = np.random.default_rng(7)
    kd_true = []
    for c in range(CAMS):
        s = sg.choice([-1.0, 1.0], 8)
        t = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]] + list(D))
        t[:2] *= 1 + 0.01 * s[:2]
        t[2:4] += 2 * s[2:4]
        t[4] += 0.004 * s[4]
        t[5] += 0.002 * s[5]
        kd_true.append(t)
    ext = [np.array(e) for e in synth.rig_extrinsics(CAMS)]
    eg = np.random.default_rng(11)
    ext_true = [ext[0]]
    for c in range(1, CAMS):
        ang = eg.choice([-1, 1], 3) * math.radians(0.4)
        d = np.eye(4)
        d[:3, :3] = synth.rot_z(ang[0]) @ synth.rot_x(ang[1]) @ synth.rot_y(ang[2])
        d[:3, 3] = eg.choice([-1, 1], 3) * 0.012 / math.sqrt(3)
        ext_true.append(d @ ext[c])
    rng = np.random.default_rng(1000)
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
            cam = synth.make_cam(Twc[:3, :3], Twc[:3, 3], W, H)
            cam.fx, cam.fy, cam.cx, cam.cy = kd_true[c][:4]
            for i in range(4):
                cam.k[i] = kd_true[c][4 + i]
            cams.append(cam)
    m = M.Mantis(max_cams=NV * CAMS, max_width=W, max_height=H)
    m.set_map(*synth.load_map())
    fb = W * H * 3
    dev = m.device_alloc(len(cams) * fb)
    m.synth_render(cams, [synth.frame_seed(3, i) for i in range(len(cams))], dev)
    m.synchronize()

    def images(kds, exts):
        out = []
        for i in range(len(cams)):
            kd = kds[i % CAMS]
            Kc = np.array([[kd[0], 0, kd[2]], [0, kd[1], kd[3]], [0, 0, 1.0]])
            out.append(M.make_image(None, Kc, kd[4:], T_base_cam=exts[i % CAMS], device_ptr=dev + i * fb, width=W,
                                    height=H))
        return out

    given = images([kd0] * CAMS, ext)
    gaps = lambda kds: [round(model_gap(kds[c], kd_true[c], W, H), 4) for c in range(CAMS)]
    eerr = lambda E: [[round(v, 5) for v in pose_error(np.array(E[c]), ext_true[c])] for c in range(1, CAMS)]
    line = {"cams_per_rig": CAMS, "free_ext": FREE_EXT, "free_int": ALL, "param_mask": 0xFF, "warmup": a.warmup,
            "calls_each": a.rounds * a.calls, "start_err_m_deg": [round(x, 5) for x in pose_error(pred[0], truth[0])],
            "model_gap_before_px": gaps([kd0] * CAMS), "ext_err_before_m_deg": eerr(ext)}
    for N in a.views:
        imgs, T0 = given[: N * CAMS], np.array(pred[:N])

        def rcalib_call(**kw):
            t0 = time.perf_counter()
            T, res = m.calibrate_rig(imgs, N, T0, FREE_EXT, ALL, **kw)
            return time.perf_counter() - t0, (T, res)

        def pair_call():
            t0 = time.perf_counter()
            m.calibrate_extrinsics(imgs, N, T0, FREE_EXT)
            T, res = m.calibrate_intrinsics(imgs, N, T0, ALL)
            return time.perf_counter() - t0, (T, res)

        kinds = {"rcalib": rcalib_call, "pair": pair_call}
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
        m.calibrate_rig(imgs, N, T0, FREE_EXT, ALL)
        kern = {}
        for name, ms in m.kernel_times():
            kern[name] = kern.get(name, 0.0) + ms
        launches = len(m.kernel_times())
        kern_pair = {}
        m.calibrate_extrinsics(imgs, N, T0, FREE_EXT)
        for name, ms in m.kernel_times():
            kern_pair[name] = kern_pair.get(name, 0.0) + ms
        m.calibrate_intrinsics(imgs, N, T0, ALL)
        for name, ms in m.kernel_times():
            kern_pair[name] = kern_pair.get(name, 0.0) + ms
        m.set_profiling(False)
        T, res = last["rcalib"]
        kds = np.array([list(res.K[c]) + list(res.D[c]) for c in range(CAMS)])
        E = np.array([list(res.T_base_cam[c]) for c in range(CAMS)]).reshape(CAMS, 4, 4)
        before = m.refine_batch(imgs, N, T0)
        after = m.refine_batch(images(list(kds), list(E))[: N * CAMS], N, T0)
        ms10, (T10, res10) = rcalib_call(iterations=10)  # untimed but for this one call
        kds10 = np.array([list(res10.K[c]) + list(res10.D[c]) for c in range(CAMS)])
        E10 = np.array([list(res10.T_base_cam[c]) for c in range(CAMS)]).reshape(CAMS, 4, 4)
        perr = lambda Ts: [pose_error(Ts[r], truth[r])[0] for r in range(N)]
        Tof = lambda rr: np.array(rr.T_w_b).reshape(4, 4)
        mw = lambda e: [round(float(np.median(e)), 6), round(float(np.max(e)), 6)]
        p50 = {k: float(np.median(v)) * 1e3 for k, v in lat.items()}
        fx = kd0[0]
        line[f"views_{N}"] = {
            "rcalib_p50_ms": round(p50["rcalib"], 3), "extrinsics_plus_intrinsics_p50_ms": round(p50["pair"], 3),
            "status": res.status, "calibrated": res.calibrated, "iterations_run": res.iterations_run,
            "n_obs": list(res.n_obs)[: res.iterations_run + 1],
            "rms_px": [round(v * fx, 4) for v in list(res.rms)[: res.iterations_run + 1]],
            "rms_cam_px": [round(v * fx, 4) for v in list(res.rms_cam)[:CAMS]],
            "launches": launches, "kernel_ms_per_call": {k: round(v, 4) for k, v in kern.items()},
            "extrinsics_plus_intrinsics_kernel_ms": {k: round(v, 4) for k, v in kern_pair.items()},
            "model_gap_after_px": gaps(kds), "ext_err_after_m_deg": eerr(E),
            "sigma_fx_fy_cx_cy_px": [[round(math.sqrt(max(res.cov_int[c][9 * e], 0.0)), 4) for e in range(4)]
                                     for c in range(CAMS)],
            "sigma_ext_xyz_m": [[round(math.sqrt(max(res.cov_ext[c][7 * e], 0.0)), 6) for e in range(3)]
                                for c in range(CAMS)],
            "pose_err_m_median_worst": {
                "start": mw(perr(T0)), "rcalib": mw(perr(T)),
                "refine_nominal_rig": mw(perr([Tof(x) for x in before])),
                "refine_calibrated_rig": mw(perr([Tof(x) for x in after]))},
            "iterations_10": {
                "one_call_ms": round(ms10 * 1e3, 3), "status": res10.status, "calibrated": res10.calibrated,
                "iterations_run": res10.iterations_run,
                "rms_px": [round(v * fx, 4) for v in list(res10.rms)[: res10.iterations_run + 1]],
                "model_gap_after_px": gaps(kds10), "ext_err_after_m_deg": eerr(E10),
                "pose_err_m_median_worst": mw(perr(T10))}}
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
