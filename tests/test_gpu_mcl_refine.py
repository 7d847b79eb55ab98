"""The modes of the Monte Carlo localization set refined on the grid lines and
the set recentred on them, on the GPU (mantis_mcl_refine_modes) against its
definition (include/mantis.h): the modes against mantis_mcl_modes, every mode's
refinement against mantis_refine_batch on the repeated frames (results and
recorded passes, byte for byte), the moved set against the host build of the
same rule (hc_mcl_recentre of test_mcl_refine_host), what must not change
(the step's record, the log-weights, the prior, the cv::RNG state), the state
machine and the argument errors. The 1280x720 ring scene of test_gpu_mcl and
the constructed four-cluster sets of test_gpu_mcl_modes.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _refine_ref as RR
import test_mcl_refine_host as MRH
from mantis_amd import synth
from test_gpu_mcl import CAMS, W, H, _cloud, _images, _rand, mantis, scene  # noqa: F401 (fixtures)
from test_gpu_mcl_modes import G, KW, PLUS_X, MINUS_Y, TRUTH, YAW90, _clusters, _stepped

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_STATE = 0, 1, 5
POSE_TOL = 1e-9
# what the clusters of the recentre tests share on top of their jitter: 1.5 cm along the base x-axis and 0.5
# degrees of yaw (gaussians drawn yaw, pitch, roll, z, y, x)
OFFSET = _rand([1, 0, 0, 0, 0, 1], math.radians(0.5), 0.015)


@pytest.fixture(scope="module")
def lm(landmark_map):
    return RR.all_landmarks(landmark_map)


def _call(mantis, images, max_modes=8, apply=0, out=None, **kw):
    """The raw call: (status, last error, the record)."""
    import mantis_amd as M

    n = len(images)
    arr = (M.MantisImage * max(n, 1))(*images)
    p = mantis.refine_params()
    for k, v in kw.items():
        setattr(p, k, v)
    out = M.MantisMclRefined() if out is None else out
    st = M.lib().mantis_mcl_refine_modes(mantis.h, arr, n, max_modes, C.byref(p), apply, C.byref(out))
    return st, M.lib().mantis_last_error(mantis.h).decode(), out


def _mode_T(out):
    return np.array([np.array(out.modes.mode[k].T_w_b).reshape(4, 4) for k in range(out.n_modes)])


def _host_inputs(out):
    """(T_ref [8, 4, 4], refined [8]) of a record, as hc_mcl_refine_plan / hc_mcl_recentre take them."""
    T_ref, refined = np.zeros((8, 4, 4)), np.zeros(8, np.int32)
    for k in range(out.n_modes):
        T_ref[k] = np.array(out.mode[k].refine.T_w_b).reshape(4, 4)
        refined[k] = out.mode[k].refine.refined
    return T_ref, refined


def _check_plan(out, apply):
    """applied / key_kept of a record against the host rule on its own modes and refinements."""
    T_ref, refined = _host_inputs(out)
    kept, app, _, _ = MRH.plan(out.modes, T_ref, refined, apply)
    assert [out.mode[k].key_kept for k in range(8)] == list(kept)
    assert [out.mode[k].applied for k in range(8)] == list(app)
    assert (out.status, out.apply, out.n_modes) == (0, apply, out.modes.n_modes)
    for k in range(out.n_modes, 8):
        assert not any(bytes(out.mode[k]))
    return T_ref, refined, app


def _records(mantis, results):
    """Every recorded pass of every rig of the last refine call."""
    return [[mantis.refine_record(k, ps) for ps in range(r.iterations_run + 1)] for k, r in enumerate(results)]


def _same_records(a, b):
    assert len(a) == len(b)
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert len(ra) == len(rb), k
        for pa, pb in zip(ra, rb):
            for x, y in zip(pa, pb):  # T, codes, Sw, Skw, rows, acc28
                assert x.tobytes() == y.tobytes(), k


# ------------------------------------------------------------------ 1. modes
@pytest.mark.parametrize("N", [1, 7, 257, 4096])
def test_modes_are_mcl_modes(mantis, scene, N):
    _stepped(mantis, scene, N)
    imgs = _images(scene, CAMS[:1])
    for mm in (1, 3, 8):
        want = mantis.mcl_modes(mm)
        out = mantis.mcl_refine_modes(imgs, mm, iterations=1)
        assert bytes(out.modes) == bytes(want) and out.n_modes == want.n_modes == min(mm, 4, N)
        assert bytes(mantis.mcl_modes(mm)) == bytes(want)
        _check_plan(out, 0)
        assert out.n_moved == 0
    mantis.mcl_select_mode(out.n_modes - 1)  # the call cached its modes: a commit may follow
    assert np.array_equal(mantis.prior_pose, _mode_T(out)[-1])


# ------------------------------------------------- 2. refinement = the batch call
@pytest.mark.parametrize("cams,odd", [((0,), False), ((0, 3), False), ((0, 3), True)])
def test_refinement_equals_the_batch_call(mantis, scene, lm, landmark_map, cams, odd):
    """4 modes x 1 camera and 4 x 2 = max_cams: the batch call gets the frames
    once per mode; with an odd candidate count the last trip of a block has one
    half idle."""
    w, r, g = landmark_map
    X, nw, nr, ng = lm
    if odd:
        for drop in range(1, 8):
            Xo = np.concatenate([w[drop:], r, g])
            if len(RR.candidates(RR.flags(Xo, 0.08))) % 2 == 1:
                break
        X, nw = np.ascontiguousarray(Xo), len(w) - drop
    try:
        if odd:
            mantis.set_map(w[drop:], r, g)
        kinds, _, _ = _stepped(mantis, scene, 257)
        imgs = _images(scene, cams)
        out = mantis.mcl_refine_modes(imgs, 8, record=1)
        K = out.n_modes
        assert K == 4 and out.mode[0].refine.n_cand % 2 == (1 if odd else 0)
        res = [out.mode[k].refine for k in range(K)]
        recs = _records(mantis, res)
        batch = mantis.refine_batch(imgs * K, K, _mode_T(out), record=1)
        for k in range(K):
            assert bytes(res[k]) == bytes(batch[k]), k
        _same_records(recs, _records(mantis, batch))
        assert any(x.refined for x in res)
        _check_plan(out, 0)
        # the pose once against the host build of the whole iteration: the first mode without a sample near a
        # tie (as test_gpu_refine) among the three clusters that stand on the lattice. The cluster yawed in
        # place starts up to half a cell from any pose the lines agree with: its first passes hold few rows,
        # their solves are ill-conditioned and carry last-bit differences of the rows far past 1e-9
        p = mantis.refine_params()
        f = RR.flags(X, p.landmark_pitch)
        K_, D_ = synth.intrinsics(W, H)
        compared = 0
        for k in range(K):
            if compared or kinds[out.modes.mode[k].best] == YAW90:
                continue
            near = 0
            for T, *_ in recs[k]:
                for c in cams:
                    near += int(RR.obs(T, scene["ext"][c], K_, D_, scene["frames"][c], X, nw, nr, ng, f)[4].sum())
            if near:
                continue
            host = RR.seq(_mode_T(out)[k], [scene["ext"][c] for c in cams], [scene["frames"][c] for c in cams], X, nw, nr,
                          ng, p, K_, D_)
            np.testing.assert_allclose(np.array(res[k].T_w_b), np.array(host.T_w_b), rtol=0, atol=POSE_TOL)
            assert list(res[k].n_obs) == list(host.n_obs)
            assert (res[k].status, res[k].refined, res[k].iterations_run) == (host.status, host.refined,
                                                                              host.iterations_run)
            compared += 1
        assert compared == 1
    finally:
        if odd:
            mantis.set_map(w, r, g)


# --------------------------------------------- 3. more modes than a batch can hold
def test_more_modes_than_max_cams_allows(mantis, scene):
    """4 modes x 3 cameras = 12 frames' worth on a context of max_cams = 8."""
    import mantis_amd as M

    _stepped(mantis, scene, 257)
    imgs = _images(scene)
    out = mantis.mcl_refine_modes(imgs, 8)
    assert out.n_modes == 4
    Tm = _mode_T(out)
    arr = (M.MantisImage * 12)(*(imgs * 4))
    p, res = mantis.refine_params(), (M.MantisRefineResult * 4)()
    assert M.lib().mantis_refine_batch(mantis.h, arr, 4, 3, Tm.ctypes.data, C.byref(p), res) == ERR_ARG
    assert "max_cams" in M.lib().mantis_last_error(mantis.h).decode()
    for k in range(4):
        one = mantis.refine_batch(imgs, 1, Tm[k])[0]
        assert bytes(out.mode[k].refine) == bytes(one), k
    assert any(out.mode[k].refine.refined for k in range(4))


# ------------------------------------------------------------------ 4. recentre
def _grid_node(scene, lm):
    """The grid intersection nearest the truth: a centre of the floor grid's 90 degree symmetry."""
    X = lm[0]
    nodes = X[RR.flags(X, 0.08) == 3][:, :2]
    return nodes[np.argmin(np.linalg.norm(nodes - scene["Twb"][:2, 3], axis=1))]


def _lattice_truth(scene, lm, kind):
    """The pose a cluster's lines put it at: the truth one cell off, or turned
    by 90 degrees about a grid intersection (the turn of test_gpu_mcl_modes, in
    place, is no symmetry of the grid: that cluster has no such pose)."""
    T = scene["Twb"].copy()
    if kind == PLUS_X:
        T[0, 3] += G
    elif kind == MINUS_Y:
        T[1, 3] -= G
    elif kind == YAW90:
        p = _grid_node(scene, lm)
        S = np.eye(4)
        S[:3, :3] = synth.rot_z(math.pi / 2)
        S[:2, 3] = p - S[:2, :2] @ p
        T = S @ T
    return T


def _offset_clusters(scene, lm, N):
    """The clusters of test_gpu_mcl_modes with the yawed one carried to its
    lattice truth, every member then moved by OFFSET in its base frame."""
    T, kinds = _clusters(scene, N)
    T[kinds == YAW90, :3, 3] += _lattice_truth(scene, lm, YAW90)[:3, 3] - scene["Twb"][:3, 3]
    return np.ascontiguousarray(T @ OFFSET), kinds


def _stepped_offset(mantis, scene, lm, N, cams, **over):
    T, kinds = _offset_clusters(scene, lm, N)
    mantis.rng_state = 1
    mantis.mcl_init_particles(T, **{**KW, **over})
    _, mo = mantis.mcl_step(_images(scene, cams))
    rec = mantis.mcl_record()
    assert mo.lost == 0 and np.array_equal(rec["T_pred"], T)
    return kinds, mo, rec


def _same_dict(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_offsets_are_refinable(mantis, scene, lm):
    """mantis_refine_batch alone, from each of the offset mode poses: refined,
    and closer to the lattice truth than the mode's mean, in both measures."""
    cams = CAMS[:2]
    kinds, mo, rec = _stepped_offset(mantis, scene, lm, 257, cams)
    modes = mantis.mcl_modes(8)
    assert modes.n_modes == 4
    Tm = np.array([np.array(modes.mode[k].T_w_b).reshape(4, 4) for k in range(4)])
    res = mantis.refine_batch(_images(scene, cams) * 4, 4, Tm)
    seen = set()
    for k in range(4):
        kind = int(kinds[modes.mode[k].best])
        seen.add(kind)
        truth = _lattice_truth(scene, lm, kind)
        d0, a0 = RR.pose_dist(Tm[k], truth)
        d1, a1 = RR.pose_dist(np.array(res[k].T_w_b).reshape(4, 4), truth)
        print(f"mode {k} kind {kind}: {100 * d0:.3f} cm / {a0:.4f} deg -> {100 * d1:.4f} cm / {a1:.4f} deg")
        assert res[k].status == 0 and res[k].refined == 1
        assert 0.01 < d0 < 0.02 and d1 < d0 and a1 < a0
    assert seen == {TRUTH, PLUS_X, MINUS_Y, YAW90}


@pytest.mark.parametrize("frac", [0.0, 2.0])
@pytest.mark.parametrize("N", [1, 7, 257, 4096])
def test_recentre(mantis, scene, lm, N, frac):
    """resample_frac 0: the set lies in the record's buffer, so the moved set
    goes to the other one; 2: the step resampled, the set moves in place."""
    cams = CAMS[:2]
    imgs = _images(scene, cams)
    color = 1 if frac == 0.0 else 0
    mantis.mcl_set_color(color)
    try:
        kinds, mo, rec = _stepped_offset(mantis, scene, lm, N, cams, resample_frac=frac)
        assert mo.resampled == (1 if frac else 0)
        modes0 = bytes(mantis.mcl_modes(8))
        col0 = (mantis.mcl_color_record(), mantis.mcl_modes_color()) if color else None
        T0, L0 = mantis.mcl_particles()
        prior, state = mantis.prior_pose.copy(), mantis.rng_state
        mantis.set_profiling(1)
        out = mantis.mcl_refine_modes(imgs, 8, apply=True)
        names = [n for n, _ in mantis.kernel_times()]
        mantis.set_profiling(0)
        T_ref, refined, app = _check_plan(out, 1)
        assert bytes(out.modes) == modes0 and out.n_modes == min(4, N)
        assert app[:out.n_modes].all(), "every offset mode is refined inside its cell"
        want, n = MRH.recentre(out.modes, T_ref, refined, 1, T0)
        T1, L1 = mantis.mcl_particles()
        assert T1.tobytes() == want.tobytes()
        assert [out.mode[k].n_moved for k in range(8)] == list(n) and out.n_moved == int(n.sum()) > 0
        if not frac:  # the predicted set itself: every particle with q > 0 of a mode, and the weightless of its cell
            assert all(n[k] >= out.modes.mode[k].n for k in range(out.n_modes))
        assert L1.tobytes() == L0.tobytes()
        assert np.array_equal(mantis.prior_pose, prior) and mantis.rng_state == state
        # one recentre launch after the 2 (I + 1) of the refinement, no image stage
        assert names == ["refine_obs/k_refine_obs", "refine_step/k_refine_step"] * 5 + ["mcl_recentre/k_mcl_recentre"]
        # the last step's record and everything read from it answer as before
        _same_dict(mantis.mcl_record(), rec)
        assert bytes(mantis.mcl_modes(8)) == modes0
        if color:
            _same_dict(mantis.mcl_color_record(), col0[0])
            for a, b in zip(mantis.mcl_modes_color(), col0[1]):
                assert a.tobytes() == b.tobytes()
        assert mantis.mcl_particles()[0].tobytes() == want.tobytes()
        # the moved set is the set: a step with zero sigmas and no motion predicts exactly it
        mantis.mcl_step(imgs)
        assert mantis.mcl_record()["T_pred"].tobytes() == want.tobytes()
    finally:
        mantis.set_profiling(0)
        mantis.mcl_set_color(0)


# ------------------------------------------------------------ 5. nothing applied
def test_nothing_applied(mantis, scene):
    cams = CAMS[:1]
    imgs = _images(scene, cams)
    _stepped(mantis, scene, 257)
    rec = mantis.mcl_record()
    T0, L0 = mantis.mcl_particles()
    prior, state = mantis.prior_pose.copy(), mantis.rng_state

    def unchanged():
        T1, L1 = mantis.mcl_particles()
        assert T1.tobytes() == T0.tobytes() and L1.tobytes() == L0.tobytes()
        assert np.array_equal(mantis.prior_pose, prior) and mantis.rng_state == state
        _same_dict(mantis.mcl_record(), rec)

    out = mantis.mcl_refine_modes(imgs, 8, apply=False)
    assert out.n_modes == 4 and any(out.mode[k].key_kept for k in range(4))
    _check_plan(out, 0)
    assert out.n_moved == 0 and not any(out.mode[k].applied or out.mode[k].n_moved for k in range(8))
    unchanged()
    gated = mantis.mcl_refine_modes(imgs, 8, apply=True, max_rms=1e-9)  # a gate no rms passes: no mode refined
    assert not any(gated.mode[k].refine.refined for k in range(4))
    assert any(gated.mode[k].refine.status == 0 and gated.mode[k].refine.iterations_run == 4 for k in range(4))
    starved = mantis.mcl_refine_modes(imgs, 8, apply=True, min_obs=100000)  # above the row count: every mode STARVED
    assert all(starved.mode[k].refine.status == 1 and starved.mode[k].refine.iterations_run == 0 for k in range(4))
    for o in (gated, starved):
        _check_plan(o, 1)
        assert o.n_moved == 0 and not any(o.mode[k].applied or o.mode[k].key_kept or o.mode[k].n_moved for k in range(8))
        assert bytes(o.modes) == bytes(out.modes)
        unchanged()
    # nothing moved: apply = 1 is still free, and moves
    moved = mantis.mcl_refine_modes(imgs, 8, apply=True)
    assert moved.n_moved > 0 and not np.array_equal(mantis.mcl_particles()[0], T0)
    # a lost step (every camera blind): MANTIS_OK, nothing launched, the entries zero
    mantis.mcl_init_particles(_cloud(scene, 12, 9), **KW)
    blind = _images(scene, cams, ext=[np.eye(4)] * 8)
    mantis.set_profiling(1)  # the stage marks stay the step's own if the call launches nothing
    _, mo = mantis.mcl_step(blind)
    assert mo.lost == 1
    Tl = mantis.mcl_particles()[0]
    st, _, out = _call(mantis, blind, 8, 1)
    mantis.set_profiling(0)
    assert st == OK and (out.status, out.n_modes, out.apply, out.n_moved) == (0, 0, 1, 0)
    assert bytes(out.modes) == bytes(mantis.mcl_modes(8))
    assert not any(bytes(out)[16 + C.sizeof(type(out.modes)):])
    names = [n for n, _ in mantis.kernel_times()]
    assert "mcl_weight/k_mcl_weight" in names and not any(n.startswith(("refine", "mcl_recentre")) for n in names)
    assert np.array_equal(mantis.mcl_particles()[0], Tl)


# ------------------------------------------------------- 6. state and arguments
def test_state_and_arguments(mantis, scene):
    import mantis_amd as M

    L = M.lib()
    imgs = _images(scene, CAMS[:2])
    T, _ = _clusters(scene, 40)
    mantis.mcl_reset()
    assert _call(mantis, imgs)[0] == ERR_STATE  # no set at all
    mantis.mcl_init_particles(T, **KW)
    st, msg, _ = _call(mantis, imgs)
    assert st == ERR_STATE and "mcl" in msg  # no step since the init
    mantis.rng_state = 99
    mantis.mcl_step(imgs)
    state = mantis.rng_state
    T0, L0 = mantis.mcl_particles()
    ring = [M.make_image(scene["frames"][CAMS[c % 3]], *synth.intrinsics(W, H), T_base_cam=scene["ext"][c % 8])
            for c in range(9)]
    small = M.make_image(np.zeros((360, 640, 3), np.uint8), *synth.intrinsics(640, 360))
    nobgr = _images(scene, CAMS[:1])[0]
    nobgr.bgr = None
    bad = [
        (imgs, 0, 1, {}, "max_modes"), (imgs, 9, 1, {}, "max_modes"), (imgs, -1, 1, {}, "max_modes"),
        (imgs, 8, 2, {}, "apply"), (imgs, 8, -1, {}, "apply"),
        (ring, 8, 1, {}, "cams_per_rig"),                # 9 frames
        ([], 8, 1, {}, "cams_per_rig"),                  # none
        ([imgs[0], small], 8, 1, {}, "size"),
        ([nobgr], 8, 1, {}, "bgr8"),
        (imgs, 8, 1, {"struct_size": 8}, "struct_size"),
        (imgs, 8, 1, {"iterations": -1}, "iterations"), (imgs, 8, 1, {"iterations": 11}, "iterations"),
        (imgs, 8, 1, {"half_window": 0}, "half_window"), (imgs, 8, 1, {"half_window": 16}, "half_window"),
        (imgs, 8, 1, {"white_thresh": 0}, "white_thresh"), (imgs, 8, 1, {"white_thresh": 195076}, "white_thresh"),
        (imgs, 8, 1, {"min_weight": 0}, "min_weight"), (imgs, 8, 1, {"min_obs": 5}, "min_obs"),
        (imgs, 8, 1, {"lambda_": -1e-9}, "lambda"), (imgs, 8, 1, {"lambda_": float("nan")}, "lambda"),
        (imgs, 8, 1, {"landmark_pitch": 0.0}, "landmark_pitch"),
        (imgs, 8, 1, {"landmark_pitch": float("inf")}, "landmark_pitch"),
        (imgs, 8, 1, {"max_rms": float("nan")}, "max_rms"), (imgs, 8, 1, {"record": 2}, "record"),
    ]
    mantis.set_profiling(1)
    for images, mm, ap, kw, word in bad:
        st, msg, _ = _call(mantis, images, mm, ap, **kw)
        assert st == ERR_ARG and word in msg, (mm, ap, kw, st, msg)
    arr, p, out = (M.MantisImage * 2)(*imgs), mantis.refine_params(), M.MantisMclRefined()
    for a, b, c in ((None, p, out), (arr, None, out), (arr, p, None)):
        st = L.mantis_mcl_refine_modes(mantis.h, a, 2, 8, None if b is None else C.byref(b), 0,
                                       None if c is None else C.byref(c))
        assert st == ERR_ARG and "null" in L.mantis_last_error(mantis.h).decode()
    # the rejected calls launched and changed nothing: the set, the state, and apply = 1 is still free
    assert mantis.rng_state == state and mantis.mcl_particles()[0].tobytes() == T0.tobytes()
    assert L.mantis_mcl_select_mode(mantis.h, 0) == ERR_STATE  # not even the modes were taken
    first = mantis.mcl_refine_modes(imgs, 8, apply=True, iterations=2)
    names = [n for n, _ in mantis.kernel_times()]
    mantis.set_profiling(0)
    assert names == ["refine_obs/k_refine_obs", "refine_step/k_refine_step"] * 3 + ["mcl_recentre/k_mcl_recentre"]
    assert first.n_moved > 0
    T1, L1 = mantis.mcl_particles()
    assert L1.tobytes() == L0.tobytes() and not np.array_equal(T1, T0)
    # the correction is applied once: a second apply = 1 before the next step is refused, apply = 0 is not
    st, msg, _ = _call(mantis, imgs, 8, 1, iterations=2)
    assert st == ERR_STATE and "recentred" in msg
    assert mantis.mcl_particles()[0].tobytes() == T1.tobytes()
    again = mantis.mcl_refine_modes(imgs, 8, apply=False, iterations=2)
    assert bytes(again.modes) == bytes(first.modes) and again.n_moved == 0
    for k in range(8):
        assert bytes(again.mode[k].refine) == bytes(first.mode[k].refine)
        assert (again.mode[k].key_kept, again.mode[k].applied, again.mode[k].n_moved) == (first.mode[k].key_kept, 0, 0)
    assert mantis.mcl_particles()[0].tobytes() == T1.tobytes() and mantis.rng_state == state
    # a commit works on the moved set; the next step frees apply = 1 again
    mantis.mcl_select_mode(0)
    assert np.array_equal(mantis.prior_pose, np.array(first.modes.mode[0].T_w_b).reshape(4, 4))
    mantis.mcl_step(imgs)
    assert _call(mantis, imgs, 8, 1, iterations=2)[0] == OK
    mantis.prior_pose = None


def test_frames_limit_is_the_cameras_not_the_modes(scene, landmark_map):
    """max_cams = 2: three frames are refused by the field's name, two serve all four modes (4 x 2 > 2)."""
    import mantis_amd as M

    m = M.Mantis(max_cams=2, max_width=W, max_height=H)
    try:
        m.set_map(*landmark_map)
        _stepped(m, scene, 40)
        st, msg, _ = _call(m, _images(scene), 8, 0)
        assert st == ERR_ARG and "max_cams" in msg
        out = m.mcl_refine_modes(_images(scene, CAMS[:2]), 8)
        assert out.n_modes == 4 and any(out.mode[k].refine.refined for k in range(4))
        for k in range(4):
            one = m.refine_batch(_images(scene, CAMS[:2]), 1, _mode_T(out)[k])[0]
            assert bytes(out.mode[k].refine) == bytes(one), k
    finally:
        m.close()


def test_process_undisturbed(mantis, scene, landmark_map):
    """A mantis_process call after the modes were refined and moved still matches the oracle."""
    import _oracle as O
    from test_gpu_parity import _cmp_debug

    import mantis_amd as M

    K, D = synth.intrinsics(W, H)
    _stepped(mantis, scene, 257)
    assert mantis.mcl_refine_modes(_images(scene, CAMS[:1]), 8, apply=True).n_moved > 0
    img = scene["frames"][CAMS[1]]
    mantis.rng_state = 1
    mantis.prior_pose = None
    _, cams = mantis.process([M.make_image(img, K, D)])
    orc = O.Oracle(*landmark_map, seed=1)
    o = orc.process(img, K, D)
    _cmp_debug(mantis.frame_debug(0), o, "after mcl_refine_modes")
    assert cams[0].reason == o.reason and cams[0].publish == o.publish
    assert mantis.rng_state == orc.rng_state
