"""Latency and behaviour of the Monte Carlo localization modes (GPU box), with
the protocol of tools/mcl_latency.py: `rigs` distinct 4-camera 1280x720 rigs,
device-resident frames.

  latency   the p50 of mantis_mcl_modes (max_modes = 8) and of
            mantis_mcl_select_mode(0) at N = 256, 1024 and 4096 after a step of
            a filter seeded with mantis_mcl_init_lattice(cells 1, 1) around the
            moved truth, host submit -> result on host, beside the p50 of
            mantis_mcl_step itself (a filter started around the moved truth, as
            mcl_latency.py times it), in alternating blocks.
  behaviour from a prediction one grid cell (0.32 m) off, N = 4096, five steps
            from mantis_mcl_init_lattice(cells 1, 1) around that prediction, at
            the library's tau and at tau = 1000: on how many rigs the heaviest
            mode's pose, and the step's mean, end within 5 cm of the truth; and
            the same with mantis_mcl_select_mode(0) after every step.

    python tools/mcl_modes_probe.py [--rigs 32] [--warmup 10] [--rounds 2] [--out FILE]
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

    W, H, CAMS = 1280, 720, 4
    K, D = synth.intrinsics(W, H)
    rng = np.random.default_rng(1000)
    ext = synth.rig_extrinsics(CAMS)
    cams, Tbc, truth, pred, cell = [], [], [], [], []
    shift = np.eye(4)
    shift[:3, :3] = synth.rot_z(math.radians(1.0))
    shift[:3, 3] = [0.02, 0.0, 0.0]
    for r in range(a.rigs):
        Twb = synth.random_base_pose(rng)
        truth.append(Twb)
        pred.append(Twb @ shift)
        off = Twb.copy()
        off[0, 3] += 0.32  # one grid cell along the world's x
        cell.append(off)
        for c in range(CAMS):
            Twc = Twb @ ext[c]
            cams.append(synth.make_cam(Twc[:3, :3], Twc[:3, 3], W, H))
            Tbc.append(ext[c])
    m = M.Mantis(max_cams=CAMS, max_width=W, max_height=H)
    m.set_map(*synth.load_map())
    fb = W * H * 3
    dev = m.device_alloc(len(cams) * fb)
    m.synth_render(cams, [synth.frame_seed(3, i) for i in range(len(cams))], dev)
    m.synchronize()
    imgs = [M.make_image(None, K, D, T_base_cam=Tbc[i], device_ptr=dev + i * fb, width=W, height=H)
            for i in range(len(cams))]
    rig = lambda r: imgs[r * CAMS:(r + 1) * CAMS]
    p0 = M.MantisMclParams()
    M.lib().mantis_default_mcl_params(p0)
    tau = p0.tau

    # ---- latency
    def step_call(r, N):
        m.mcl_init(pred[r], 0.02, 0.02, n_particles=N, tau=tau)
        t0 = time.perf_counter()
        m.mcl_step(rig(r))
        return time.perf_counter() - t0

    def modes_calls(r, N):
        m.mcl_init_lattice(pred[r], 0.02, 0.02, 1, 1, n_particles=N, tau=tau)
        m.mcl_step(rig(r))
        t0 = time.perf_counter()
        mo = m.mcl_modes(8)
        t1 = time.perf_counter()
        try:
            m.mcl_select_mode(0)
        except M.MantisError:  # the mode left no offspring in the resampling
            pass
        t2 = time.perf_counter()
        return t1 - t0, t2 - t1, mo.n_modes

    sizes = (256, 1024, 4096)
    for k in range(a.warmup):
        for N in sizes:
            step_call(k % a.rigs, N)
            modes_calls(k % a.rigs, N)
    lat_s, lat_m, lat_k, nm = ({N: [] for N in sizes} for _ in range(4))
    for rnd in range(a.rounds):
        for N in sizes:
            for r in range(a.rigs):
                lat_s[N].append(step_call(r, N))
            for r in range(a.rigs):
                dm, dk, n = modes_calls(r, N)
                lat_m[N].append(dm)
                lat_k[N].append(dk)
                nm[N].append(n)

    # ---- behaviour from one cell off
    def run(tau_, select):
        ok_mode, ok_mean, shares, cells = 0, 0, [], []
        for r in range(a.rigs):
            m.mcl_init_lattice(cell[r], 0.03, 0.05, 1, 1, n_particles=4096, tau=tau_)
            mo = mm = None
            for _ in range(5):
                _, mo = m.mcl_step(rig(r))
                if mo.lost:
                    continue
                mm = m.mcl_modes(8)
                if select and mm.n_modes:
                    try:
                        m.mcl_select_mode(0)
                    except M.MantisError:  # the mode left no offspring in the resampling
                        pass
            if mo is not None and not mo.lost:
                ok_mean += pose_error(np.array(mo.T_w_b).reshape(4, 4), truth[r]) <= 0.05
                if mm.n_modes:
                    ok_mode += pose_error(np.array(mm.mode[0].T_w_b).reshape(4, 4), truth[r]) <= 0.05
                    shares.append(mm.mode[0].share)
                    cells.append(mm.n_cells)
        return {"heaviest_mode_within_5cm": int(ok_mode), "step_mean_within_5cm": int(ok_mean),
                "heaviest_share_median": round(float(np.median(shares)), 4) if shares else None,
                "n_cells_median": float(np.median(cells)) if cells else None}

    behaviour = {f"tau_{name}{'_select' if sel else ''}": run(t, sel)
                 for name, t in (("default", tau), ("1000", 1000.0)) for sel in (False, True)}
    m.prior_pose = None

    p50 = lambda v: round(float(np.median(v)) * 1e3, 3)
    line = {
        "rigs": a.rigs, "cams_per_rig": CAMS, "warmup": a.warmup, "calls_each": a.rounds * a.rigs, "tau_default": tau,
        "mcl_step_p50_ms": {str(N): p50(lat_s[N]) for N in sizes},
        "mcl_modes_p50_ms": {str(N): p50(lat_m[N]) for N in sizes},
        "mcl_select_mode_p50_ms": {str(N): p50(lat_k[N]) for N in sizes},
        "n_modes_median": {str(N): float(np.median(nm[N])) for N in sizes},
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
