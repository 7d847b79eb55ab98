"""Scale, latency and behaviour of Monte Carlo localization (GPU box).

Over `rigs` distinct 4-camera 1280x720 rigs with device-resident frames:

  tau      the scale of the pooled error around the optimum: per rig
           E(truth moved by 2 cm and 1 degree) - E(truth), both scored as the
           two particles of one mantis_mcl_step; median and spread. The
           library's default tau is this median (include/mantis.h).
  latency  the p50 of mantis_mcl_step at N = 256, 1024 and 4096 (a filter
           started around the moved truth before each timed step), host submit
           -> result on host, beside mantis_track and one-rig mantis_process in
           alternating blocks, so that all see the same machine state; the
           step's launch count and stage times from a profiled pass of its own.
  recovery from a prediction one grid cell (0.32 m) off: the fraction of rigs
           whose estimate is within 5 cm of the truth after 5 steps of a
           4096-particle filter started with sigma_t0 = 0.2 m, and the same
           figure for 5 mantis_track calls from that prediction.

    python tools/mcl_latency.py [--rigs 32] [--warmup 10] [--rounds 2] [--tau T] [--out FILE]

--tau: the tau of the latency and recovery parts (default: the library's).
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
# the localization path captures no graph
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DBL_MAX = np.finfo(np.float64).max


def pose_error(T_est, T_true):
    """(translation error in m, rotation error in degrees)"""
    dt = float(np.linalg.norm(T_est[:3, 3] - T_true[:3, 3]))
    c = (np.trace(T_true[:3, :3].T @ T_est[:3, :3]) - 1.0) / 2.0
    return dt, math.degrees(math.acos(max(-1.0, min(1.0, c))))


def pooled(rec):
    S = rec["sums"].sum(axis=1)
    N = rec["counts"].astype(np.int64).sum(axis=1)
    return np.where(N > 0, S / (np.maximum(N, 1) * 1.1), DBL_MAX)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rigs", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2, help="alternating blocks of `rigs` calls of each kind")
    ap.add_argument("--tau", type=float, default=None)
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
    tau = a.tau if a.tau is not None else p0.tau

    # ---- tau: E(moved truth) - E(truth)
    dE, E0 = [], []
    for r in range(a.rigs):
        m.mcl_init_particles(np.array([truth[r], pred[r]]), sigma_rot=0.0, sigma_t=0.0, tau=1.0, resample_frac=0.0,
                             min_projections=0, record=1)
        m.mcl_step(rig(r))
        E = pooled(m.mcl_record())
        E0.append(float(E[0]))
        dE.append(float(E[1] - E[0]))
    qt = lambda v, p: round(float(np.percentile(v, p)), 1)

    # ---- latency
    def mcl_call(r, N):
        m.mcl_init(pred[r], 0.02, 0.02, n_particles=N, tau=tau)
        t0 = time.perf_counter()
        out, mo = m.mcl_step(rig(r))
        return time.perf_counter() - t0, out, mo

    def track_call(r):
        m.prior_pose = pred[r]
        t0 = time.perf_counter()
        out, tout = m.track(rig(r))
        return time.perf_counter() - t0, out, tout

    def process_call(r):
        m.prior_pose = None
        t0 = time.perf_counter()
        out, _ = m.process(rig(r), rigs=1)
        return time.perf_counter() - t0, out[0]

    sizes = (256, 1024, 4096)
    for k in range(a.warmup):
        for N in sizes:
            mcl_call(k % a.rigs, N)
        track_call(k % a.rigs)
        process_call(k % a.rigs)
    lat = {N: [] for N in sizes}
    lat_t, lat_p, acc, ess = [], [], {N: [] for N in sizes}, {N: [] for N in sizes}
    for rnd in range(a.rounds):
        for N in sizes:
            for r in range(a.rigs):
                dt, out, mo = mcl_call(r, N)
                lat[N].append(dt)
                if rnd == 0 and not mo.lost:
                    acc[N].append(pose_error(np.array(mo.T_w_b).reshape(4, 4), truth[r]))
                    ess[N].append(mo.ess)
        for r in range(a.rigs):
            lat_t.append(track_call(r)[0])
        for r in range(a.rigs):
            lat_p.append(process_call(r)[0])
    m.set_profiling(True)
    st, launches = {}, 0
    for r in range(a.rigs):
        m.mcl_init(pred[r], 0.02, 0.02, n_particles=1024, tau=tau)
        m.mcl_step(rig(r))
        launches = sum(n.startswith("mcl_") for n, _ in m.kernel_times())
        for name, ms in m.stage_times():
            st.setdefault(name, []).append(ms)
    m.set_profiling(False)

    # ---- recovery from one cell off
    ok_mcl, ok_trk, final_ess = 0, 0, []
    for r in range(a.rigs):
        m.mcl_init(cell[r], 0.03, 0.2, n_particles=4096, tau=tau)
        for _ in range(5):
            out, mo = m.mcl_step(rig(r))
        if not mo.lost:
            final_ess.append(mo.ess)
            ok_mcl += pose_error(np.array(mo.T_w_b).reshape(4, 4), truth[r])[0] <= 0.05
        m.prior_pose = cell[r]
        T = cell[r]
        for _ in range(5):
            out, tout = m.track(rig(r))
            if tout.tracked:
                T = np.array(tout.T_w_b).reshape(4, 4)
        ok_trk += pose_error(T, truth[r])[0] <= 0.05
    m.prior_pose = None

    p50 = lambda v: round(float(np.median(v)) * 1e3, 3)
    line = {
        "rigs": a.rigs, "cams_per_rig": CAMS, "warmup": a.warmup, "calls_each": a.rounds * a.rigs,
        "tau_used": tau,
        "dE_median": qt(dE, 50), "dE_p25": qt(dE, 25), "dE_p75": qt(dE, 75), "dE_min": qt(dE, 0), "dE_max": qt(dE, 100),
        "E_truth_median": qt(E0, 50),
        "mcl_step_p50_ms": {str(N): p50(lat[N]) for N in sizes},
        "track_p50_ms": p50(lat_t), "process_p50_ms": p50(lat_p),
        "mcl_launches_after_image_stages": launches,
        "mcl_stage_median_ms_n1024": {k: round(float(np.median(v)), 4) for k, v in st.items()},
        "mcl_median_err_m": {str(N): round(float(np.median([e[0] for e in acc[N]])), 5) for N in sizes if acc[N]},
        "mcl_median_ess": {str(N): round(float(np.median(ess[N])), 1) for N in sizes if ess[N]},
        "recovered_within_5cm_mcl": int(ok_mcl), "recovered_within_5cm_track": int(ok_trk),
        "recovery_final_ess_median": round(float(np.median(final_ess)), 1) if final_ess else None,
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
