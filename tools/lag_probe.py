"""Latency of the fixed-lag window (GPU box), by the protocol of
tools/smooth_probe.py.

The four-camera 1280x720 rig at capacity 8 and 32, views chained by a small
step, every view's start predicted on the device. The window is filled and
slid a few times (warmup); then `rounds` alternating blocks of `calls` calls of
each kind, host submit -> result on host:
  push     mantis_lag_push of the next view (steady state: every push slides)
  batch    mantis_smooth_batch on the views the window holds, from the poses
           it holds, with the prior it carries
once with device-resident frames and once with host frames (a push stages C
frames where the batch call stages N C), and the stage events of one profiled
call of each kind (lag_frames: the C frame copies and the upload; lag_slide:
k_lag_slide).

    python tools/lag_probe.py [--warmup 3] [--rounds 2] [--calls 10] [--out profiles/lag_probe.json]

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


def quat_of(R):
    w = math.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2]) / 2.0
    return [(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lag_probe.json"))
    a = ap.parse_args()

    import mantis_amd as M
    from mantis_amd import synth

    CAMS, W, H = 4, 1280, 720
    line = {"lib": os.path.basename(M.LIB_PATH), "warmup": a.warmup, "calls_each": a.rounds * a.calls}
    K, D = synth.intrinsics(W, H)
    ext = synth.rig_extrinsics(CAMS)
    fb = W * H * 3
    shift = np.eye(4)
    shift[:3, :3] = synth.rot_z(math.radians(1.0))
    shift[:3, 3] = [0.02, 0.0, 0.0]
    for N in (8, 32):
        n_views = N + a.warmup + a.rounds * a.calls + 1
        step = np.eye(4)
        step[:3, :3] = synth.rot_z(math.radians(90.0 / n_views))
        step[:3, 3] = [0.6 / n_views, 0.0, 0.0]
        motion = list(step[:3, 3]) + quat_of(step[:3, :3])
        truth = [np.eye(4)]
        truth[0][:3, :3] = synth.rot_z(0.3)
        truth[0][:3, 3] = [-0.3, -0.3, 1.4]
        for _ in range(n_views - 1):
            truth.append(truth[-1] @ step)
        cams = []
        for T in truth:
            for c in range(CAMS):
                Twc = T @ ext[c]
                cams.append(synth.make_cam(Twc[:3, :3], Twc[:3, 3], W, H))
        m = M.Mantis(max_cams=N * CAMS, max_width=W, max_height=H)
        m.set_map(*synth.load_map())
        dev = m.device_alloc(len(cams) * fb)
        m.synth_render(cams, [synth.frame_seed(31, i) for i in range(len(cams))], dev)
        m.synchronize()
        host = []
        for i in range(len(cams)):
            f = np.zeros((H, W, 3), np.uint8)
            m.d2h(f, dev + i * fb)
            host.append(f)
        rec = {}
        for kind in ("device", "host"):
            def view(k):
                if kind == "device":
                    return [M.make_image(None, K, D, T_base_cam=ext[c], device_ptr=dev + (k * CAMS + c) * fb, width=W,
                                         height=H) for c in range(CAMS)]
                return [M.make_image(host[k * CAMS + c], K, D, T_base_cam=ext[c]) for c in range(CAMS)]

            m.lag_reset(N, CAMS)
            state = {"k": 0, "views": None, "res": None}

            def push():
                k = state["k"]
                state["res"], state["views"], state["info"] = m.lag_push(view(k), None if k == 0 else motion,
                                                                        truth[0] @ shift if k == 0 else None)
                state["k"] = k + 1

            def batch():
                k = state["k"]
                imgs = [im for j in range(k - N, k) for im in view(j)]
                T0 = np.array([np.array(v.T_w_b).reshape(4, 4) for v in state["views"]])
                has, T, cov, _ = state["prior"]
                return m.smooth_batch(imgs, 1, N, T0, np.array([motion] * (N - 1)), T if has else None,
                                      cov if has else None)

            for _ in range(N + a.warmup):
                push()
            state["prior"] = m.lag_prior()
            for _ in range(a.warmup):
                batch()
            lat = {"push": [], "batch": []}
            for _ in range(a.rounds):
                for _ in range(a.calls):
                    t0 = time.perf_counter()
                    push()
                    lat["push"].append(time.perf_counter() - t0)
                state["prior"] = m.lag_prior()
                for _ in range(a.calls):
                    t0 = time.perf_counter()
                    batch()
                    lat["batch"].append(time.perf_counter() - t0)
            m.set_profiling(True)
            stages = {}
            for name, fn in (("batch", batch), ("push", push)):
                fn()
                acc = {}
                for n_, ms in m.kernel_times():
                    acc[n_] = acc.get(n_, 0.0) + ms
                stages[name] = {k: round(v, 4) for k, v in acc.items()}
            m.set_profiling(False)
            r, info = state["res"], state["info"]
            rec[kind] = {"p50_ms": {k: round(float(np.median(v)) * 1e3, 3) for k, v in lat.items()},
                         "stage_ms_per_call": stages, "status": r.status, "smoothed": r.smoothed,
                         "has_prior": info.has_prior, "drop_reason": info.drop_reason, "pushes": info.pushes}
        line[f"N{N}_C4_1280x720"] = rec
        m.device_free(dev)
        m.close()

    s = json.dumps(line)
    print(s)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
