"""Latency of refining the MCL modes in one call (GPU box), by the protocol of
tools/refine_probe.py.

One 4-camera 1280x720 rig with device-resident frames and a set of four
clusters (the truth and three lattice neighbours, each moved by 1.5 cm and 0.5
degrees, with a jitter well inside a cell), stepped once. After `warmup` calls
of each kind, `rounds` alternating blocks of `calls` calls of each kind, host
submit -> result on host, default refine parameters:
  refine_modes     mantis_mcl_refine_modes(apply = 0): 4 modes x 4 cameras, the
                   frames staged once
  modes_batch      mantis_mcl_modes, then mantis_refine_batch on the 4 frames
                   listed once per mode (16 frames on a context of max_cams 16)
both also with the same frames in host memory (rendered by the host renderer:
the batch call then copies every frame once per mode), and, from profiled
passes of their own, the stage events of a call with apply =
1 (a fresh step before each, a correction is applied once per step) for both
recentre paths and two set sizes; the median and worst distance of the modes
and of their refinements to the lattice truth.

    python tools/mcl_refine_probe.py [--calls 32] [--warmup 10] [--rounds 2] [--out FILE]
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

G = 0.32
CELLS = [(0, 0), (1, 0), (0, -1), (1, -1)]


def pose_error(T_est, T_true):
    """(translation error in m, rotation error in degrees)"""
    dt = float(np.linalg.norm(T_est[:3, 3] - T_true[:3, 3]))
    c = (np.trace(T_true[:3, :3].T @ T_est[:3, :3]) - 1.0) / 2.0
    return dt, math.degrees(math.acos(max(-1.0, min(1.0, c))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2, help="alternating blocks of `calls` calls of each kind")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import mantis_amd as M
    from mantis_amd import synth

    W, H, CAMS, MODES = 1280, 720, 4, 4
    K, D = synth.intrinsics(W, H)
    rng = np.random.default_rng(1000)
    ext = synth.rig_extrinsics(CAMS)
    Twb = synth.random_base_pose(rng)
    cams = []
    for c in range(CAMS):
        Twc = Twb @ ext[c]
        cams.append(synth.make_cam(Twc[:3, :3], Twc[:3, 3], W, H))
    m = M.Mantis(max_cams=CAMS * MODES, max_width=W, max_height=H)
    m.set_map(*synth.load_map())
    fb = W * H * 3
    dev = m.device_alloc(CAMS * fb)
    m.synth_render(cams, [synth.frame_seed(3, i) for i in range(CAMS)], dev)
    m.synchronize()
    imgs = [M.make_image(None, K, D, T_base_cam=ext[i], device_ptr=dev + i * fb, width=W, height=H) for i in range(CAMS)]

    shift = np.eye(4)
    shift[:3, :3] = synth.rot_z(math.radians(0.5))
    shift[:3, 3] = [0.015, 0.0, 0.0]

    def truth_of(cell):
        T = Twb.copy()
        T[0, 3] += cell[0] * G
        T[1, 3] += cell[1] * G
        return T

    def cluster_set(n):
        T = np.zeros((n, 4, 4))
        for j in range(n):
            jit = np.eye(4)
            if j >= MODES:
                g = rng.normal(size=6) * 0.005
                jit[:3, :3] = synth.rot_z(g[0]) @ synth.rot_y(g[1]) @ synth.rot_x(g[2])
                jit[:3, 3] = g[3:]
            T[j] = truth_of(CELLS[j % MODES]) @ shift @ jit
        return T

    def stepped(n, frac):
        m.rng_state = 1
        m.mcl_init_particles(cluster_set(n), sigma_rot=0.0, sigma_t=0.0, tau=60000.0, resample_frac=frac)
        _, mo = m.mcl_step(imgs)
        assert mo.lost == 0

    stepped(256, 0.0)

    host = [synth.render_host(cams[i], synth.frame_seed(3, i)) for i in range(CAMS)]
    himgs = [M.make_image(host[i], K, D, T_base_cam=ext[i]) for i in range(CAMS)]

    def refine_modes_call(frames):
        def call():
            t0 = time.perf_counter()
            out = m.mcl_refine_modes(frames, 8)
            return time.perf_counter() - t0, out
        return call

    def modes_batch_call(frames):
        def call():
            t0 = time.perf_counter()
            modes = m.mcl_modes(8)
            Tm = np.array([list(modes.mode[k].T_w_b) for k in range(modes.n_modes)])
            res = m.refine_batch(frames * modes.n_modes, modes.n_modes, Tm)
            return time.perf_counter() - t0, (modes, res)
        return call

    kinds = {"refine_modes": refine_modes_call(imgs), "modes_batch": modes_batch_call(imgs),
             "refine_modes_host": refine_modes_call(himgs), "modes_batch_host": modes_batch_call(himgs)}
    for fn in kinds.values():
        for _ in range(a.warmup):
            fn()
    lat = {k: [] for k in kinds}
    for _ in range(a.rounds):
        for name, fn in kinds.items():
            for _ in range(a.calls):
                lat[name].append(fn()[0])
    _, out = kinds["refine_modes"]()
    _, (modes, res) = kinds["modes_batch"]()
    _, hout = kinds["refine_modes_host"]()
    _, (_, hres) = kinds["modes_batch_host"]()
    host_same = all(bytes(hout.mode[k].refine) == bytes(hres[k]) for k in range(hout.n_modes))
    assert out.n_modes == modes.n_modes == MODES
    same = all(bytes(out.mode[k].refine) == bytes(res[k]) for k in range(MODES))
    err_mode, err_ref = [], []
    for k in range(MODES):
        md = out.modes.mode[k]
        truth = truth_of((md.ix + round((np.array(out.modes.anchor_T_w_b)[3] - Twb[0, 3]) / G),
                          md.iy + round((np.array(out.modes.anchor_T_w_b)[7] - Twb[1, 3]) / G)))
        err_mode.append(pose_error(np.array(md.T_w_b).reshape(4, 4), truth))
        err_ref.append(pose_error(np.array(out.mode[k].refine.T_w_b).reshape(4, 4), truth))

    # stage events of a call with apply = 1: a profiled pass of its own, a fresh step before each call
    stages, launches, moved = {}, {}, {}
    for n in (256, 4096):
        for frac, path in ((0.0, "copy_flip"), (2.0, "in_place")):
            key = f"N{n}_{path}"
            st = {}
            for _ in range(max(a.calls // 4, 4)):
                stepped(n, frac)
                m.set_profiling(True)
                o = m.mcl_refine_modes(imgs, 8, apply=True)
                names = [nm for nm, _ in m.kernel_times()]
                for nm, ms in m.stage_times():
                    st.setdefault(nm, []).append(ms)
                m.set_profiling(False)
                launches[key] = len(names)
                moved[key] = o.n_moved
            stages[key] = {k: round(float(np.median(v)), 4) for k, v in st.items()}

    def stat(v, i):
        xs = [x[i] for x in v]
        return [round(float(np.median(xs)), 6), round(float(np.max(xs)), 6)]

    line = {"modes": MODES, "cams": CAMS, "particles": 256, "warmup": a.warmup, "calls_each": a.rounds * a.calls,
            "refine_modes_p50_ms": round(float(np.median(lat["refine_modes"])) * 1e3, 3),
            "modes_batch_p50_ms": round(float(np.median(lat["modes_batch"])) * 1e3, 3),
            "refine_modes_p90_ms": round(float(np.percentile(lat["refine_modes"], 90)) * 1e3, 3),
            "modes_batch_p90_ms": round(float(np.percentile(lat["modes_batch"], 90)) * 1e3, 3),
            "host_frames_refine_modes_p50_ms": round(float(np.median(lat["refine_modes_host"])) * 1e3, 3),
            "host_frames_modes_batch_p50_ms": round(float(np.median(lat["modes_batch_host"])) * 1e3, 3),
            "host_frames_refine_modes_p90_ms": round(float(np.percentile(lat["refine_modes_host"], 90)) * 1e3, 3),
            "host_frames_modes_batch_p90_ms": round(float(np.percentile(lat["modes_batch_host"], 90)) * 1e3, 3),
            "results_byte_equal": same, "host_frames_results_byte_equal": host_same,
            "refined": [out.mode[k].refine.refined for k in range(MODES)],
            "key_kept": [out.mode[k].key_kept for k in range(MODES)],
            "mode_err_m_median_worst": stat(err_mode, 0), "mode_err_deg_median_worst": stat(err_mode, 1),
            "refined_err_m_median_worst": stat(err_ref, 0), "refined_err_deg_median_worst": stat(err_ref, 1),
            "apply_launches": launches, "apply_n_moved": moved, "apply_stage_median_ms_per_call": stages}
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
