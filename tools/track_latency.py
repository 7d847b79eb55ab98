"""Latency and accuracy of rig tracking against the detection path (GPU box).

Over `rigs` distinct 4-camera 1280x720 rigs with device-resident frames,
after `warmup` calls of each kind: the p50 of mantis_track (default
parameters, record = 0; the prior is the truth moved by 2 cm and 1 degree) and
of one-rig mantis_process, host submit -> result on host, alternating blocks
of each so both see the same machine state; the median translation / rotation
error of each to the synthetic truth; the tracking call's launch count and its
stage times (mantis_kernel_times, from a profiled pass of its own).

    python tools/track_latency.py [--rigs 32] [--warmup 20] [--rounds 4] [--out FILE]
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
# the tracking path captures no graph
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

ROOT =os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4, help="alternating blocks of `rigs` calls of each kind")
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
    fb = W * H * 3
    dev = m.device_alloc(len(cams) * fb)
    m.synth_render(cams, [synth.frame_seed(3, i) for i in range(len(cams))], dev)
    m.synchronize()
    imgs = [M.make_image(None, K, D, T_base_cam=Tbc[i], device_ptr=dev + i * fb, width=W, height=H)
            for i in range(len(cams))]
    rig = lambda r: imgs[r * CAMS:(r + 1) * CAMS]

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

    for k in range(a.warmup):
        track_call(k % a.rigs)
    for k in range(a.warmup):
        process_call(k % a.rigs)
    lat_t, lat_p = [], []
    acc_t, acc_p, tracked, published = {}, {}, 0, 0
    for rnd in range(a.rounds):
        for r in range(a.rigs):
            dt, out, tout = track_call(r)
            lat_t.append(dt)
            if rnd == 0:
                tracked += tout.tracked
                acc_t[r] = pose_error(np.array(tout.T_w_b).reshape(4, 4), truth[r])
        for r in range(a.rigs):
            dt, out = process_call(r)
            lat_p.append(dt)
            if rnd == 0 and out.publish:
                published += 1
                acc_p[r] = pose_error(quat_T(list(out.orientation_xyzw), list(out.position)), truth[r])
    # stage times of the tracking call: a profiled pass of its own
    m.set_profiling(True)
    st, launches = {}, 0
    for r in range(a.rigs):
        m.prior_pose = pred[r]
        m.track(rig(r))
        kt = m.kernel_times()
        launches = sum(n.startswith("track_") for n, _ in kt)
        for name, ms in m.stage_times():
            st.setdefault(name, []).append(ms)
    m.set_profiling(False)
    med = lambda v, i: round(float(np.median([x[i] for x in v.values()])), 5) if v else None
    line = {
        "rigs": a.rigs, "cams_per_rig": CAMS, "warmup": a.warmup, "calls_each": a.rounds * a.rigs,
        "track_p50_ms": round(float(np.median(lat_t)) * 1e3, 3),
        "process_p50_ms": round(float(np.median(lat_p)) * 1e3, 3),
        "track_launches_after_image_stages": launches,
        "track_stage_median_ms": {k: round(float(np.median(v)), 4) for k, v in st.items()},
        "tracked": tracked, "published": published,
        "seed_median_err_m_deg": [round(x, 5) for x in pose_error(pred[0], truth[0])],
        "track_median_err_m": med(acc_t, 0), "track_median_err_deg": med(acc_t, 1),
        "process_median_err_m": med(acc_p, 0), "process_median_err_deg": med(acc_p, 1),
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
