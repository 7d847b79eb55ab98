"""Case generator and comparer of the whole-callback matrix
(test_pipeline_matrix_host.py, test_gpu_pipeline_matrix.py): rendered frames
beyond the bench camera, deterministic and seeded. A plain helper module.

A cell is (lens, frame size): the lenses of _score_cases.LENSES at 1280x720
and 907x505, four views each (VIEWS: altitude and tilt from nadir), and one
frame per lens at the tiny sizes 130x35 and 33x7. A frame is rendered on the
host by synth.render_host from a SynthCam filled by hand with the lens's
float32-rounded K and its D (make_cam only knows the bench lens).

The guard. The device's libm may differ from glibc's by an ulp, about 1e-16
relative, and a case must not sit where that flips a decision: a cluster
threshold, an ObjPose iteration count, a sort order, the publish gate. So the
oracle processes every frame three times, each time in a fresh Oracle(seed=1):
with D, with D[0] and D[1] plus PERTURB = 1e-13, and with both minus it. A
case is kept only if the three runs agree on every integer and integer-valued
record (INT_SCALARS and INT_ARRAYS, the quad corners included) and no entry of hyp_c2w,
pf_c2w, position or orientation_xyzw moves by more than
MOTION = 1e-7 * max(1, |entry|). The perturbation is about 1000 times an ulp's
effect, so a kept case moves by less than 1e-10 under libm differences, inside
the suite's POSE_TOL of 1e-9. A seed that fails moves to the next one
(seeds_moved); the census test asserts the final state. The GPU tests run the
cases in batches with the RNG carried from frame to frame, so the census also
asserts the same guard on every batch run that way (sequence_guard).
"""
import functools
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import _oracle as O
import _score_cases as SC
from mantis_amd import synth

POSE_TOL = 1e-9  # the suite's pose tolerance (test_gpu_parity.POSE_TOL)
PERTURB = 1e-13
MOTION = 1e-7
LENSES = SC.LENSES
SIZES = [(1280, 720), (907, 505)]
TINY = [(130, 35), (33, 7)]
# (name, altitude range [m], tilt-from-nadir range [deg])
VIEWS = [("bench", (1.0, 2.0), (0.0, 25.0)),   # the bench camera's poses
         ("low", (0.35, 0.6), (0.0, 10.0)),    # few, large quads
         ("high", (2.5, 3.5), (0.0, 15.0)),    # many small quads
         ("steep", (1.0, 2.0), (35.0, 50.0))]
# the first base seed of 300 .. 329 at which every class of the census
# (test_pipeline_matrix_host.py) occurs; found with the oracle alone. After a
# change to the renderer, the lenses or the view ranges, redo the search: set
# SEED0 to each candidate in turn and take the first at which
# test_pipeline_matrix_host.py passes.
SEED0, SEED_TRIES = 312, 8
# integer and integer-valued records (the fast errors are integer sums / (n * 1.1))
INT_SCALARS = ("reason", "publish", "n_raw_quads", "n_quads", "n_gen", "n_hyps", "yaw_best", "rng_state_after",
               "best1_err", "pf_err", "n_scored")
INT_ARRAYS = ("quads", "hyp_n", "hyp_err", "pf_iter_err", "shift_err", "top20_err")
POSE_ARRAYS = ("hyp_c2w", "pf_c2w", "position", "orientation_xyzw")


def view_pose(rng, view):
    """(R_wc, pos) of synth.random_pose with the view's altitude and tilt."""
    _, (h0, h1), (t0, t1) = view
    h = rng.uniform(h0, h1)
    yaw = rng.uniform(0, 2 * math.pi)
    tilt = math.radians(t0 + (t1 - t0) * math.sqrt(rng.uniform(0, 1)))
    tdir = rng.uniform(0, 2 * math.pi)
    R = synth.rot_z(yaw) @ synth.NADIR @ synth.rot_x(tilt * math.cos(tdir)) @ synth.rot_y(tilt * math.sin(tdir))
    return R, np.array([rng.uniform(-0.48, 0.48), rng.uniform(-0.48, 0.48), h])


def lens_cam(Kr, D, R_wc, pos, w, h):
    c = synth.SynthCam()
    c.fx, c.fy, c.cx, c.cy = Kr[0, 0], Kr[1, 1], Kr[0, 2], Kr[1, 2]
    for i in range(4):
        c.k[i] = D[i]
    R = np.asarray(R_wc, np.float64).reshape(9)
    for i in range(9):
        c.R_wc[i] = R[i]
    for i in range(3):
        c.pos[i] = pos[i]
    c.w, c.h = w, h
    return c


def render(name, w, h, view_idx, seed):
    """(image, K, D) of one frame: the pose from a Generator seeded by (seed,
    lens, size, view), the floor noise from synth.frame_seed."""
    K, D = SC.lens(name, w, h)
    rng = np.random.default_rng([seed, LENSES.index(name), w, h, view_idx])
    R, pos = view_pose(rng, VIEWS[view_idx])
    img = synth.render_host(lens_cam(SC.k32(K), D, R, pos, w, h), synth.frame_seed(9, seed * 16 + view_idx))
    return img, K, D


def arr(rec, field):
    return np.array(getattr(rec, field))


def _rows(rec, field):
    """The rows of an array record that the frame filled."""
    a = arr(rec, field)
    if field in ("quads", "test_pts"):
        return a[:max(0, min(rec.n_quads, O.ORC_MAX_QUADS))]
    if field in ("hyp_n", "hyp_err", "hyp_c2w"):
        return a[:max(0, min(rec.n_hyps, O.ORC_MAX_HYPS))]
    return a


def guard(recs):
    """(kept, motion) of the three oracle records of one frame: kept iff the
    integer records agree and no pose entry moves by more than MOTION;
    motion is the largest |entry - entry'| / max(1, |entry|) seen."""
    base = recs[0]
    kept, motion = True, 0.0
    for r in recs[1:]:
        for f in INT_SCALARS:
            kept &= getattr(r, f) == getattr(base, f)
        if not kept:
            return False, math.inf
        for f in INT_ARRAYS:
            kept &= np.array_equal(_rows(r, f), _rows(base, f))
        for f in POSE_ARRAYS:
            a, b = _rows(base, f), _rows(r, f)
            if np.isnan(a).any() or np.isnan(b).any():
                return False, math.inf
            if a.size:
                motion = max(motion, float((np.abs(a - b) / np.maximum(1.0, np.abs(a))).max()))
    return bool(kept and motion <= MOTION), motion


_POOL = ThreadPoolExecutor(12)  # oracle passes only (leaf tasks; the oracle releases the GIL)


def _oracle1(args):
    img, K, D, s = args
    Dp = np.array(D, np.float64)
    Dp[:2] += s
    return O.Oracle(*synth.load_map(), seed=1).process(img, K, Dp)


def oracle3(img, K, D):
    """The frame's three oracle records: D, D[:2] + PERTURB, D[:2] - PERTURB."""
    return list(_POOL.map(_oracle1, [(img, K, D, s) for s in (0.0, PERTURB, -PERTURB)]))


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(name, w, h, view_idx):
    """The frame of (lens, size, view) at the first seed that keeps the guard:
    .img .K .D .rec (the oracle's record, fresh Oracle(seed=1)) .seed
    .seeds_moved .motion (largest relative pose motion under the perturbation)
    .moved_motion (that of the seeds passed over; inf = an integer changed)"""
    moved_motion = []
    for k in range(SEED_TRIES):
        img, K, D = render(name, w, h, view_idx, SEED0 + k)
        recs = oracle3(img, K, D)
        ok, motion = guard(recs)
        if ok:
            c = Case()
            c.name, c.w, c.h, c.view, c.img, c.K, c.D, c.rec = name, w, h, VIEWS[view_idx][0], img, K, D, recs[0]
            c.seed, c.seeds_moved, c.motion, c.moved_motion = SEED0 + k, k, motion, moved_motion
            return c
        moved_motion.append(motion)
    raise RuntimeError(f"no seed keeps the guard for case {name} {w}x{h} {VIEWS[view_idx][0]}")


def _cases(keys):
    synth.load_map()
    O.lib()
    with ThreadPoolExecutor(4) as ex:
        return list(ex.map(lambda k: case(*k), keys))


def cell(name, w, h):
    """The 4 cases (one per view) of a (lens, size) cell, in VIEWS order."""
    return _cases([(name, w, h, v) for v in range(len(VIEWS))])


def tiny_cases(w, h):
    """One bench-like frame per lens at a tiny size."""
    return _cases([(n, w, h, 0) for n in LENSES])


def mixed_batch(w, h):
    """One case of every lens at a size, the views taken in turn."""
    return _cases([(n, w, h, i % len(VIEWS)) for i, n in enumerate(LENSES)])


def all_cases():
    return [c for n in LENSES for wh in SIZES for c in cell(n, *wh)] + [c for wh in TINY for c in tiny_cases(*wh)]


def _sequence1(args):
    cases, s = args
    orc = O.Oracle(*synth.load_map(), seed=1)
    recs = []
    for c in cases:
        Dp = np.array(c.D, np.float64)
        Dp[:2] += s
        recs.append(orc.process(c.img, c.K, Dp))
    return recs, orc.rng_state


def oracle_sequence(cases):
    """The oracle's records of the cases processed in order by one
    Oracle(seed=1), carrying its cv::RNG, and the final RNG state."""
    return _sequence1((cases, 0.0))


def sequence_guard(cases):
    """The guard on a batch as the GPU tests run it: from the second frame on
    the particle filter draws from a carried RNG state, not from the fresh
    one the case was kept under. [(kept, motion)] per frame, plus whether the
    final RNG state is the same in the three runs."""
    runs = list(_POOL.map(_sequence1, [(cases, s) for s in (0.0, PERTURB, -PERTURB)]))
    per_frame = [guard([r[0][i] for r in runs]) for i in range(len(cases))]
    return per_frame, runs[0][1] == runs[1][1] == runs[2][1]


def batches():
    """Every batch of test_gpu_pipeline_matrix.py: (tag, cases)."""
    out = [(f"{n} {w}x{h}", cell(n, w, h)) for n in LENSES for (w, h) in SIZES]
    out += [(f"tiny {w}x{h}", tiny_cases(w, h)) for (w, h) in TINY]
    out += [(f"mixed {w}x{h}", mixed_batch(w, h)) for (w, h) in SIZES]
    return out


# ---------------------------------------------------------------- comparer
def _close(g, o, tol, label, rows=None):
    """g within tol * max(1, |o|) of o, NaN and infinities exactly where o has
    them. |o| is the entry's own magnitude, or with rows = k the largest
    magnitude of the entry's row of k values (a translation or position of 3:
    max(1, |t|max), as test_rpp_solve_n_points_matches_oracle takes it for t)."""
    g, o = np.asarray(g, np.float64), np.asarray(o, np.float64)
    assert g.shape == o.shape, f"{label}: shape {g.shape} vs {o.shape}"
    assert np.array_equal(np.isnan(g), np.isnan(o)), f"{label}: NaN in another place than the oracle's"
    inf = np.isinf(o)
    assert np.array_equal(np.isinf(g), inf) and np.array_equal(g[inf], o[inf]), f"{label}: infinities differ"
    fin = np.isfinite(o)
    mag = np.where(fin, np.abs(o), 0.0)
    if rows is not None and o.size:
        mag = np.broadcast_to(mag.reshape(-1, rows).max(axis=1, keepdims=True), (o.size // rows, rows)).reshape(o.shape)
    err = np.abs(g[fin] - o[fin]) / np.maximum(1.0, mag[fin])
    assert (err <= tol).all(), f"{label}: off by {err.max():.3e} x max(1, |ref|), bound {tol:.1e}"


def _close_c2w(g, o, label):
    """Poses (rows of 12: R row-major, then t): every rotation entry within an
    absolute POSE_TOL, t within POSE_TOL * max(1, |t|max) of its own pose, the
    bounds of test_rpp_solve_n_points_matches_oracle."""
    g, o = np.asarray(g, np.float64).reshape(-1, 12), np.asarray(o, np.float64).reshape(-1, 12)
    _close(g[:, :9], o[:, :9], POSE_TOL, f"{label} R")
    assert not (np.abs(o[:, :9]) > 1 + 1e-12).any(), f"{label}: a rotation entry above 1 in the reference"
    _close(g[:, 9:], o[:, 9:], POSE_TOL, f"{label} t", rows=3)


def cmp_record(g, o, label):
    """test_gpu_parity._cmp_debug's fields with two changes: test points within
    1e-12 * max(1, |ref|) (they reach 1e16 off the bench lens; 4,500 ulp, far
    above any libm tan difference) and poses within POSE_TOL * max(1, |ref|):
    rotation and quaternion entries absolute, a translation or position scaled
    by its own largest magnitude (they reach 74 m with the 'off' lens)."""
    assert g.reason == o.reason, f"{label}: reason {g.reason} vs {o.reason}"
    assert g.n_raw_quads == o.n_raw_quads, f"{label}: raw quads {g.n_raw_quads} vs {o.n_raw_quads}"
    assert g.n_quads == o.n_quads, f"{label}: quads {g.n_quads} vs {o.n_quads}"
    n = g.n_quads
    assert np.array_equal(arr(g, "quads")[:n], arr(o, "quads")[:n]), f"{label}: quad corners differ"
    _close(arr(g, "test_pts")[:n], arr(o, "test_pts")[:n], 1e-12, f"{label}: test points")
    assert g.n_gen == o.n_gen, f"{label}: generated hyps {g.n_gen} vs {o.n_gen}"
    assert g.n_hyps == o.n_hyps, f"{label}: clustered hyps {g.n_hyps} vs {o.n_hyps}"
    assert g.rng_state_after == o.rng_state_after, f"{label}: cv::RNG state after the frame differs"
    if o.reason in (1, 2):
        return
    c = g.n_hyps
    _close_c2w(arr(g, "hyp_c2w")[:c], arr(o, "hyp_c2w")[:c], f"{label}: hyp_c2w")
    assert np.array_equal(arr(g, "hyp_n")[:c], arr(o, "hyp_n")[:c]), f"{label}: hyp_n differs"
    assert np.array_equal(arr(g, "hyp_err")[:c], arr(o, "hyp_err")[:c]), f"{label}: hyp_err differs"
    assert g.best1_err == o.best1_err, f"{label}: best1_err {g.best1_err} vs {o.best1_err}"
    assert np.array_equal(arr(g, "pf_iter_err"), arr(o, "pf_iter_err")), f"{label}: pf_iter_err differs"
    _close_c2w(arr(g, "pf_c2w"), arr(o, "pf_c2w"), f"{label}: pf_c2w")
    assert np.array_equal(arr(g, "shift_err"), arr(o, "shift_err")), f"{label}: shift_err differs"
    assert np.array_equal(arr(g, "top20_err"), arr(o, "top20_err")), f"{label}: top20_err differs"
    np.testing.assert_allclose(arr(g, "yaw_err"), arr(o, "yaw_err"), rtol=1e-12, err_msg=f"{label}: yaw_err")
    assert g.yaw_best == o.yaw_best, f"{label}: yaw_best {g.yaw_best} vs {o.yaw_best}"
    assert g.publish == o.publish, f"{label}: publish {g.publish} vs {o.publish}"
    _close(arr(g, "position"), arr(o, "position"), POSE_TOL, f"{label}: position", rows=3)
    _close(arr(g, "orientation_xyzw"), arr(o, "orientation_xyzw"), POSE_TOL, f"{label}: orientation")
    np.testing.assert_allclose(g.pub_error, o.pub_error, rtol=1e-12, err_msg=f"{label}: pub_error")
