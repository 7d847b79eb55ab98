"""Latency and behaviour of the Monte Carlo localization colour evidence (GPU
box), with the protocol of tools/mcl_latency.py: `rigs` distinct 4-camera
1280x720 rigs, device-resident frames.

  defaults  Ec(truth) and Ec(truth moved one cell along world y) - Ec(truth)
            per rig from the colour record of a two-particle step (enable = 1):
            the figures tools/mcl_color_defaults.py takes from the CPU oracle,
            here from the device, medians and spread.
  latency   the p50 of mantis_mcl_step at N = 256, 1024 and 4096 with enable =
            0 and enable = 2 (a filter started around the moved truth before
            each timed step), host submit -> result on host, in alternating
            blocks; the step's launch list and stage times at N = 1024 with
            colour on from a profiled pass of its own.
  behaviour from a prediction one grid cell (0.32 m) off along world y (the
            axis the green border discriminates) and along x: N = 4096, five
            steps from mantis_mcl_init_lattice(cells 1, 1) around that
            prediction at the library's tau, with enable = 0, 1 and 2: on how
            many rigs the heaviest mode's pose ends within 5 cm of the truth,
            and with colour on the same for the mode chosen by
            mantis_mcl_modes_color in two ways -- the smallest Ec among the
            reported modes, and the heaviest mode among those whose Ec is
            within color_tau of the smallest -- with the median shares; for
            the rigs that see the border at the truth and for those that do
            not.

    python tools/mcl_color_probe.py [--rigs 32] [--warmup 10] [--rounds 2] [--out FILE]
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

DBL_MAX = np.finfo(np.float64).max


def pose_error(T_est, T_true):
    return float(np.linalg.norm(T_est[:3, 3] - T_true[:3, 3]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rigs", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2, help="alternating blocks of `rigs` calls of each kind")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import mantis_amd as M
    from mantis_amd import synth

    W, H, CAMS, G = 1280, 720, 4, 0.32
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

    def moved(T, axis):
        off = T.copy()
        off[axis, 3] += G
        return off

    m = M.Mantis(max_cams=CAMS, max_width=W, max_height=H)
    m.set_map(*synth.load_map())
    fb = W * H * 3
    dev = m.device_alloc(len(cams) * fb)
    m.synth_render(cams, [synth.frame_seed(3, i) for i in range(len(cams))], dev)
    m.synchronize()
    imgs = [M.make_image(None, K, D, T_base_cam=Tbc[i], device_ptr=dev + i * fb, width=W, height=H)
            for i in range(len(cams))]
    rig = lambda r: imgs[r * CAMS:(r + 1) * CAMS]
    p0 = m.mcl_params()
    c0 = m.mcl_color_params()
    tau, min_color = p0.tau, c0.min_color_projections

    # ---- the defaults' figures from the device
    E0, dE, sees = [], [], []
    m.mcl_set_color(1)
    for r in range(a.rigs):
        m.mcl_init_particles(np.array([truth[r], moved(truth[r], 1)]), sigma_rot=0.0, sigma_t=0.0, tau=tau,
                             resample_frac=0.0)
        m.mcl_step(rig(r))
        cr = m.mcl_color_record()
        sees.append(bool(cr["Ec"][0] != DBL_MAX))
        if sees[-1]:
            E0.append(float(cr["Ec"][0]))
            if cr["Ec"][1] != DBL_MAX:
                dE.append(float(cr["Ec"][1] - cr["Ec"][0]))
    qt = lambda v, p: round(float(np.percentile(v, p)), 1) if v else None

    # ---- latency
    def step_call(r, N):
        m.mcl_init(pred[r], 0.02, 0.02, n_particles=N, tau=tau)
        t0 = time.perf_counter()
        m.mcl_step(rig(r))
        return time.perf_counter() - t0

    sizes, enables = (256, 1024, 4096), (0, 2)
    for k in range(a.warmup):
        for e in enables:
            m.mcl_set_color(e)
            for N in sizes:
                step_call(k % a.rigs, N)
    lat = {(e, N): [] for e in enables for N in sizes}
    for rnd in range(a.rounds):
        for N in sizes:
            for e in enables:
                m.mcl_set_color(e)
                for r in range(a.rigs):
                    lat[(e, N)].append(step_call(r, N))
    m.mcl_set_color(2)
    m.set_profiling(True)
    st, names = {}, []
    for r in range(a.rigs):
        m.mcl_init(pred[r], 0.02, 0.02, n_particles=1024, tau=tau)
        m.mcl_step(rig(r))
        names = [n.split("/")[0] for n, _ in m.kernel_times() if n.startswith("mcl_")]
        for name, ms in m.stage_times():
            st.setdefault(name, []).append(ms)
    m.set_profiling(False)

    # ---- behaviour from one cell off
    def run(axis, enable):
        res = {k: {"rigs": 0, "heaviest_mode_within_5cm": 0, "color_mode_within_5cm": 0,
                   "color_gated_mode_within_5cm": 0, "step_mean_within_5cm": 0,
                   "shares": [], "color_shares": [], "cells": []} for k in ("sees_border", "blind")}
        m.mcl_set_color(enable)
        for r in range(a.rigs):
            o = res["sees_border" if sees[r] else "blind"]
            o["rigs"] += 1
            m.mcl_init_lattice(moved(truth[r], axis), 0.03, 0.05, 1, 1, n_particles=4096, tau=tau)
            mo = None
            for _ in range(5):
                _, mo = m.mcl_step(rig(r))
            if mo.lost:
                continue
            mm = m.mcl_modes(8)
            o["step_mean_within_5cm"] += pose_error(np.array(mo.T_w_b).reshape(4, 4), truth[r]) <= 0.05
            if not mm.n_modes:
                continue
            o["heaviest_mode_within_5cm"] += pose_error(np.array(mm.mode[0].T_w_b).reshape(4, 4), truth[r]) <= 0.05
            o["shares"].append(mm.mode[0].share)
            o["cells"].append(mm.n_cells)
            if enable:
                ec, _ = m.mcl_modes_color()
                k = int(np.argmin(ec[:mm.n_modes]))  # DBL_MAX where the mode's best sees too little green
                o["color_mode_within_5cm"] += pose_error(np.array(mm.mode[k].T_w_b).reshape(4, 4), truth[r]) <= 0.05
                o["color_shares"].append(mm.mode[k].share)
                # the modes are in weight order: the first one whose colour error is within color_tau of the least
                k = next(i for i in range(mm.n_modes) if ec[i] <= ec[k] + c0.color_tau)
                o["color_gated_mode_within_5cm"] += pose_error(np.array(mm.mode[k].T_w_b).reshape(4, 4), truth[r]) <= 0.05
        for o in res.values():
            for k in ("shares", "color_shares", "cells"):
                v = o.pop(k)
                o[k[:-1] + "_median"] = round(float(np.median(v)), 4) if v else None
            if not enable:
                o.pop("color_mode_within_5cm")
                o.pop("color_gated_mode_within_5cm")
                o.pop("color_share_median")
        return res

    behaviour = {f"{'xy'[axis]}_enable_{e}": run(axis, e) for axis in (1, 0) for e in (0, 1, 2)}
    m.mcl_set_color(0)
    m.prior_pose = None

    p50 = lambda v: round(float(np.median(v)) * 1e3, 3)
    line = {
        "rigs": a.rigs, "cams_per_rig": CAMS, "warmup": a.warmup, "calls_each": a.rounds * a.rigs, "tau": tau,
        "color_tau": c0.color_tau, "color_miss": c0.color_miss, "min_color_projections": min_color,
        "rigs_seeing_border_at_truth": int(sum(sees)),
        "Ec_truth_median": qt(E0, 50), "Ec_truth_p25": qt(E0, 25), "Ec_truth_p75": qt(E0, 75),
        "Ec_truth_min": qt(E0, 0), "Ec_truth_max": qt(E0, 100),
        "dEc_median": qt(dE, 50), "dEc_p25": qt(dE, 25), "dEc_p75": qt(dE, 75), "dEc_min": qt(dE, 0),
        "dEc_max": qt(dE, 100),
        "mcl_step_p50_ms": {f"enable_{e}": {str(N): p50(lat[(e, N)]) for N in sizes} for e in enables},
        "mcl_launches_color_on": names,
        "mcl_stage_median_ms_n1024_color_on": {k: round(float(np.median(v)), 4) for k, v in st.items()},
        "one_cell_off_n4096_5_steps": behaviour,
    }
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
