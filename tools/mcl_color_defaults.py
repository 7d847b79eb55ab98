"""The measured defaults of the MCL colour evidence (CPU only, no GPU needed).

Over the `rigs` four-camera 1280x720 synthetic rigs of tools/mcl_latency.py
(the same poses and frame seeds, rendered on the host), with the CPU oracle's
COLOR evaluator (orc_score, fast = 0) on the raw frames:

  color_miss  the median over the rigs of Ec(truth), the pooled colour error
              Ec = sum_c csum / (sum_c cn * 100 * 1.1), among the rigs with at
              least `min_color` green landmarks in view at the truth
  color_tau   the median of Ec(truth moved one grid cell along world y) -
              Ec(truth) among those of them that still see `min_color` there

include/mantis.h MANTIS_MCL_COLOR_MISS_DEFAULT / MANTIS_MCL_COLOR_TAU_DEFAULT
are these medians.

    python tools/mcl_color_defaults.py [--rigs 32] [--min-color 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def c2w12(T_w_c):
    v = np.linalg.inv(T_w_c)
    return np.concatenate([v[:3, :3].reshape(9), v[:3, 3]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rigs", type=int, default=32)
    ap.add_argument("--min-color", type=int, default=10)
    ap.add_argument("--cell", type=float, default=0.32, help="the grid spacing")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import _oracle as O
    from mantis_amd import synth

    W, H, CAMS = 1280, 720, 4
    K, D = synth.intrinsics(W, H)
    rng = np.random.default_rng(1000)
    ext = synth.rig_extrinsics(CAMS)
    orc = O.Oracle(*synth.load_map())

    def pooled(frames, Twb):
        """(Ec or None, pooled green count) of base pose Twb on the rig's frames"""
        S, n = 0, 0
        for c in range(CAMS):
            err, npj = orc.score(frames[c], K, D, c2w12(Twb @ ext[c]), fast=False)
            if npj[0] > 0:
                x = err[0] * npj[0] * 1.1 * 100.0
                assert abs(x - round(x)) < 1e-3
                S += int(round(x))
                n += int(npj[0])
        return (S / (n * 100.0 * 1.1) if n >= max(a.min_color, 1) else None), n

    E0, dE, n0, n1 = [], [], [], []
    for r in range(a.rigs):
        Twb = synth.random_base_pose(rng)
        frames = []
        for c in range(CAMS):
            Twc = Twb @ ext[c]
            frames.append(synth.render_host(synth.make_cam(Twc[:3, :3], Twc[:3, 3], W, H),
                                            synth.frame_seed(3, r * CAMS + c)))
        e0, k0 = pooled(frames, Twb)
        off = Twb.copy()
        off[1, 3] += a.cell  # one grid cell along the world's y
        e1, k1 = pooled(frames, off)
        n0.append(k0)
        n1.append(k1)
        if e0 is None:
            continue
        E0.append(e0)
        if e1 is not None:
            dE.append(e1 - e0)
    qt = lambda v, p: round(float(np.percentile(v, p)), 1)
    line = {
        "rigs": a.rigs, "cams_per_rig": CAMS, "min_color_projections": a.min_color,
        "rigs_seeing_green_at_truth": len(E0), "rigs_seeing_green_one_cell_off": len(dE),
        "green_in_view_at_truth_min_median_max": [int(min(n0)), float(np.median(n0)), int(max(n0))],
        "green_in_view_one_cell_off_min_median_max": [int(min(n1)), float(np.median(n1)), int(max(n1))],
        "Ec_truth_median": qt(E0, 50), "Ec_truth_p25": qt(E0, 25), "Ec_truth_p75": qt(E0, 75),
        "Ec_truth_min": qt(E0, 0), "Ec_truth_max": qt(E0, 100),
        "dEc_median": qt(dE, 50), "dEc_p25": qt(dE, 25), "dEc_p75": qt(dE, 75), "dEc_min": qt(dE, 0),
        "dEc_max": qt(dE, 100), "dEc_negative": int(sum(d <= 0 for d in dE)),
    }
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
