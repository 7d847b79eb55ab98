"""bench.py's plain run and --dump-outputs.

* dump_outputs writes one float64 array per field of the result records, the
  contexts' shares in step order, the 64-bit cv::RNG state split exactly (CPU).
* A plain run (small: 2 contexts x 4 rigs) times exactly --steps steps, prints
  the headline keys without the --full figures, and dumps one row per rig and
  per camera frame of the last timed step (GPU).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("p50_latency_ms", "p50_latency_rig0_ms", "host_ingest", "roofline", "roofline_frontend", "cpu_baseline")


def test_dump_outputs_fields(tmp_path):
    import bench
    import mantis_amd as M

    class FakeBatch:
        pass

    batches = []
    for k in range(2):
        b = FakeBatch()
        b.out = (M.MantisResult * 3)()
        b.cam_out = (M.MantisCamResult * 12)()
        for i in range(3):
            b.out[i].publish = 1
            b.out[i].position[1] = 10 * k + i + 0.5
            b.out[i].rng_state_after = 0xFEDCBA9876543210 - (3 * k + i)
        for i in range(12):
            b.cam_out[i].n_scored = 100 * k + i
            b.cam_out[i].c2w[11] = -float(i)
        batches.append(b)
    bench.dump_outputs(str(tmp_path), batches)
    names = sorted(os.listdir(tmp_path))
    assert names == sorted([f"rig_{n}.npy" for n, _ in M.MantisResult._fields_]
                           + [f"cam_{n}.npy" for n, _ in M.MantisCamResult._fields_])
    arr = {n[:-4]: np.load(tmp_path / n) for n in names}
    assert all(a.dtype == np.float64 for a in arr.values())
    assert arr["rig_position"].shape == (6, 3) and arr["rig_covariance"].shape == (6, 36)
    assert arr["cam_c2w"].shape == (24, 12) and arr["cam_n_scored"].shape == (24,)
    assert arr["rig_position"][:, 1].tolist() == [0.5, 1.5, 2.5, 10.5, 11.5, 12.5]
    assert arr["cam_n_scored"].tolist() == list(range(12)) + list(range(100, 112))
    assert arr["cam_c2w"][:, 11].tolist() == [-float(i) for i in range(12)] * 2
    hi, lo = arr["rig_rng_state_after"].T
    assert [(int(h) << 32) | int(l) for h, l in zip(hi, lo)] == [0xFEDCBA9876543210 - j for j in range(6)]


@pytest.mark.gpu
def test_plain_run_times_steps_and_dumps(tmp_path):
    rigs, steps = 8, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--rigs", str(rigs), "--contexts", "2", "--distinct", "4",
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == 1 and d["unit"] == "rig poses/s" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True and d["metric"].startswith("poses/sec")
    assert d["ms_per_step"] > 0
    # value = rigs per step / time per step (both rounded to 3 decimals in the line)
    assert d["value"] == pytest.approx(rigs / (d["ms_per_step"] * 1e-3), rel=1e-3)
    assert not [k for k in FULL_ONLY if k in d]
    out = tmp_path / "out"
    rig_status, cam_status = np.load(out / "rig_status.npy"), np.load(out / "cam_status.npy")
    assert rig_status.shape == (rigs,) and cam_status.shape == (4 * rigs,)
    assert not rig_status.any() and not cam_status.any()
    pos = np.load(out / "rig_position.npy")
    assert pos.dtype == np.float64 and pos.shape == (rigs, 3) and np.isfinite(pos).all()
    # the dump is the step the line describes: the same published count, quads found in the frames
    assert np.load(out / "rig_publish.npy").sum() == round(d["published_frac"] * rigs)
    assert np.load(out / "cam_n_quads.npy").max() > 0
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) < 64 << 20
