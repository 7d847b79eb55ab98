"""Monte Carlo localization on the GPU (mantis_mcl_*): the persistent rig
particle filter against its definition (include/mantis.h): every recorded
(particle, camera) scored by the CPU oracle (exact integer sums and counts),
the predicted poses against the numpy form of the motion and diffusion rule,
and the weights, the integer scan, the ancestors and the estimate recomputed in
Python (test_mcl_host's restatements) from the step's record. One 1280x720
synthetic ring rig, three rendered cameras.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _oracle as O
import test_mcl_host as MH
from mantis_amd import synth

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-9
DBL_MAX = np.finfo(np.float64).max
W, H = 1280, 720
CAMS = (0, 3, 5)
TAU = 60000.0  # the scale of E(2 cm, 1 degree off) - E(truth) on these scenes: weights neither flat nor one-hot


@pytest.fixture(scope="module")
def mantis(landmark_map):
    import mantis_amd as M

    m = M.Mantis(max_cams=8, max_width=W, max_height=H)
    m.set_map(*landmark_map)
    yield m
    m.close()


@pytest.fixture(scope="module")
def scene():
    """One base pose seen by cameras 0, 3 and 5 of an 8-camera ring."""
    rng = np.random.default_rng(2025)
    ext = synth.rig_extrinsics(8)
    T = synth.random_base_pose(rng)
    frames = {}
    for c in CAMS:
        Twc = T @ ext[c]
        frames[c] = synth.render_host(synth.make_cam(Twc[:3, :3], Twc[:3, 3], W, H), synth.frame_seed(13, c))
    return {"ext": ext, "Twb": T, "frames": frames, "cleaned": {}}


def _images(scene, cams=CAMS, ext=None):
    import mantis_amd as M

    K, D = synth.intrinsics(W, H)
    return [M.make_image(scene["frames"][c], K, D, T_base_cam=(ext or scene["ext"])[c]) for c in cams]


def _ring_images(scene):
    """8 cameras with 8 extrinsics over the 3 rendered frames."""
    import mantis_amd as M

    K, D = synth.intrinsics(W, H)
    return [M.make_image(scene["frames"][CAMS[c % 3]], K, D, T_base_cam=scene["ext"][c]) for c in range(8)]


def _cleaned(scene, c):
    if c not in scene["cleaned"]:
        img = scene["frames"][c]
        mask = O.clean_mask(O.canny(img))
        out = img.copy()
        out[mask == 0] = 0
        scene["cleaned"][c] = out
    return scene["cleaned"][c]


def _rand(g6, sr, st):
    """Transform(setRPY(roll, pitch, yaw), (x, y, z)) from gaussians drawn yaw, pitch, roll, z, y, x."""
    g = [float(v) for v in g6]
    T = np.eye(4)
    T[:3, :3] = synth.rot_z(g[0] * sr) @ synth.rot_y(g[1] * sr) @ synth.rot_x(g[2] * sr)
    T[:3, 3] = [g[5] * st, g[4] * st, g[3] * st]
    return T


def _cloud(scene, N, seed, sr=0.02, st=0.02):
    """N base poses around the truth (particle 0 = the truth itself)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((N, 4, 4))
    for j in range(N):
        out[j] = scene["Twb"] @ _rand(rng.normal(size=6) if j else np.zeros(6), sr, st)
    return out


def _quat_T(q, p):
    x, y, z, w = q
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                 [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                 [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = p
    return T


def _next(state):
    return ((state & 0xFFFFFFFF) * 4164903690 + (state >> 32)) & 0xFFFFFFFFFFFFFFFF


def _pooled(sums, counts):
    S = sums.astype(np.int64).sum(axis=1)
    N = counts.astype(np.int64).sum(axis=1)
    E = np.full(len(S), DBL_MAX)
    ok = N > 0
    E[ok] = S[ok].astype(np.float64) / (N[ok].astype(np.float64) * 1.1)
    return E, N


def _replay(m, out, mo, frac, tau=TAU, min_projections=10):
    """Everything k_mcl_weight / k_mcl_resample decided, recomputed from the step's record."""
    rec = m.mcl_record()
    N = len(rec["q"])
    E, n = _pooled(rec["sums"], rec["counts"])
    Ln, qn = MH.np_weights(rec["L_before"], E, n, tau, min_projections)
    assert qn is not None and mo.lost == 0 and mo.status == 0 and mo.n_particles == N
    q, cum = rec["q"], rec["cum"]
    assert np.all(np.abs(q.astype(np.int64) - qn.astype(np.int64)) <= 1)  # exp is not correctly rounded
    assert np.array_equal(cum, np.cumsum(q, dtype=np.uint64))
    assert mo.weight_sum == int(cum[-1]) == int(q.astype(object).sum())
    assert mo.best == int(np.argmax(q)) and int(q[mo.best]) == MH.Q1
    assert mo.n_valid == int((q > 0).sum())
    assert mo.best_error == E[mo.best]
    Tm, cov, ess, _ = MH.np_estimate(rec["T_pred"], q)
    np.testing.assert_allclose(mo.ess, ess, rtol=1e-9)
    got_T, got_cov = np.array(mo.T_w_b).reshape(4, 4), np.array(mo.covariance).reshape(6, 6)
    np.testing.assert_allclose(got_T, Tm, atol=POSE_TOL, rtol=0)
    np.testing.assert_allclose(got_cov, cov, atol=1e-9 * np.diag(cov).max(), rtol=0)
    # the published rig and the prior hand-off
    assert out.status == 0 and out.publish == 1 and out.num_particles == N and out.weight == mo.best_error
    assert np.array_equal(np.array(out.covariance), np.array(mo.covariance))
    assert np.array_equal(np.array(out.position), got_T[:3, 3])
    np.testing.assert_allclose(_quat_T(list(out.orientation_xyzw), got_T[:3, 3]), got_T, atol=POSE_TOL, rtol=0)
    assert out.rng_state_after == mo.rng_state_after == m.rng_state
    assert np.array_equal(m.prior_pose, got_T)
    Tn, Lw = m.mcl_particles()
    fin = ~np.isinf(Ln)
    if frac >= 2:
        assert mo.resampled == 1
        assert np.array_equal(rec["ancestors"], MH.py_ancestors(cum, q, mo.U))
        assert np.array_equal(Tn, rec["T_pred"][rec["ancestors"]])
        assert np.all(Lw == 0.0) and np.all(rec["L_after"] == 0.0)
    else:
        assert mo.resampled == 0 and np.all(rec["ancestors"] == -1)
        assert np.array_equal(Tn, rec["T_pred"]) and np.array_equal(Lw, rec["L_after"])
        assert np.array_equal(np.isinf(Lw), ~fin)
        np.testing.assert_allclose(Lw[fin], Ln[fin], rtol=1e-12, atol=0)
    return rec


def test_exact_scoring(mantis, scene, landmark_map):
    """N = 7, C = 3, one step with diffusion: every recorded (particle, camera)
    against the oracle, the predicted poses against T . Delta . rand(g6)."""
    N, sr, st = 7, 0.03, 0.01
    K, D = synth.intrinsics(W, H)
    orc = O.Oracle(*landmark_map)
    T0 = _cloud(scene, N, 1)
    mantis.rng_state = 1
    mantis.mcl_init_particles(T0, sigma_rot=sr, sigma_t=st, tau=TAU, resample_frac=0.0, record=1)
    assert mantis.rng_state == 1, "init_particles draws nothing"
    out, mo = mantis.mcl_step(_images(scene))
    gauss, state = O.gaussians(1, N * 6)
    after = _next(state)
    assert mo.rng_state_after == after == mantis.rng_state and mo.U == after & 0xFFFFFFFF
    rec = _replay(mantis, out, mo, 0.0)
    for j in range(N):
        ref = T0[j] @ _rand(gauss[6 * j: 6 * j + 6], sr, st)
        np.testing.assert_allclose(rec["T_pred"][j], ref, atol=POSE_TOL, rtol=0, err_msg=f"particle {j}")
    for ci, c in enumerate(CAMS):
        ref = np.array([np.linalg.inv(T @ scene["ext"][c]) for T in rec["T_pred"]])
        ref12 = np.concatenate([ref[:, :3, :3].reshape(-1, 9), ref[:, :3, 3]], axis=1)
        np.testing.assert_allclose(rec["c2w"][:, ci], ref12, atol=POSE_TOL, rtol=0)
        err, npj = orc.score(_cleaned(scene, c), K, D, rec["c2w"][:, ci], fast=True)
        assert np.array_equal(rec["counts"][:, ci], npj), f"camera {c}: counts"
        osum = np.where(npj > 0, np.rint(np.where(npj > 0, err, 0.0) * npj * 1.1), 0).astype(np.int64)
        assert np.array_equal(rec["sums"][:, ci], osum), f"camera {c}: sums"
    assert np.all(rec["counts"].sum(axis=1) >= 10)


@pytest.mark.parametrize("N,Cn", [(1, 1), (7, 3), (65, 2), (1025, 1), (4096, 1), (64, 8)],
                         ids=["1x1", "7x3", "65x2", "1025x1", "4096x1", "64x8"])
def test_replay_from_the_record(mantis, scene, N, Cn):
    imgs = _ring_images(scene) if Cn == 8 else _images(scene, CAMS[:Cn])
    T0 = _cloud(scene, N, 100 + N)
    for frac in (2.0, 0.0):
        mantis.rng_state = 1
        mantis.prior_pose = None
        mantis.mcl_init_particles(T0, sigma_rot=0.01, sigma_t=0.005, tau=TAU, resample_frac=frac, record=1)
        out, mo = mantis.mcl_step(imgs)
        rec = _replay(mantis, out, mo, frac)
        assert rec["sums"].shape == (N, Cn) and np.all(rec["L_before"] == 0.0)
    # a second step on carried log-weights (not resampled): the scan and the estimate from L != 0
    out, mo = mantis.mcl_step(imgs)
    rec = _replay(mantis, out, mo, 0.0)
    assert N == 1 or np.any(rec["L_before"] != 0.0)


def test_screen_off_equals_screen_on(mantis, scene, landmark_map):
    """A context created with MANTIS_SCREEN=0 sends every landmark of every
    (particle, camera) through the exact fallback -- the scoring blocks'
    queues overflow, so the in-place path runs, then the drains -- and must
    record the same integer sums and counts and return the same result
    records from the same set and RNG state. 13 particles: a full chunk of 8
    and a tail of 5 per camera."""
    import os

    import mantis_amd as M

    N, Cn = 13, 2
    old = os.environ.get("MANTIS_SCREEN")
    os.environ["MANTIS_SCREEN"] = "0"
    try:
        mx = M.Mantis(max_cams=8, max_width=W, max_height=H)
    finally:
        if old is None:
            del os.environ["MANTIS_SCREEN"]
        else:
            os.environ["MANTIS_SCREEN"] = old
    try:
        mx.set_map(*landmark_map)
        T0 = _cloud(scene, N, 100 + N)
        got = []
        for m in (mx, mantis):
            m.rng_state = 1
            m.prior_pose = None
            m.mcl_init_particles(T0, sigma_rot=0.01, sigma_t=0.005, tau=TAU, resample_frac=2.0, record=1)
            out, mo = m.mcl_step(_images(scene, CAMS[:Cn]))
            got.append((bytes(out), bytes(mo), m.mcl_record(), m.rng_state))
        (ox, mox, rx, sx), (os_, mos, rs, ss) = got
        assert rx["sums"].shape == rs["sums"].shape == (N, Cn)
        assert np.array_equal(rx["sums"], rs["sums"]) and np.array_equal(rx["counts"], rs["counts"])
        assert np.array_equal(rx["c2w"], rs["c2w"]) and np.array_equal(rx["ancestors"], rs["ancestors"])
        assert ox == os_ and mox == mos and sx == ss
    finally:
        mx.close()


def test_carry_over(mantis, scene):
    """Two steps on the same frames, no resampling, no diffusion, no motion."""
    N = 33
    T0 = _cloud(scene, N, 7)
    mantis.mcl_init_particles(T0, sigma_rot=0.0, sigma_t=0.0, tau=TAU, resample_frac=0.0, record=1)
    imgs = _images(scene)
    mantis.mcl_step(imgs)
    r1 = mantis.mcl_record()
    _, L1 = mantis.mcl_particles()
    mantis.mcl_step(imgs)
    r2 = mantis.mcl_record()
    T2, L2 = mantis.mcl_particles()
    assert np.array_equal(r1["T_pred"], T0) and np.array_equal(T2, T0)
    assert np.array_equal(r1["sums"], r2["sums"]) and np.array_equal(r1["counts"], r2["counts"])
    assert np.array_equal(r2["L_before"], L1)
    np.testing.assert_allclose(L2, 2.0 * L1, rtol=1e-12, atol=0)


def test_degenerate_set(mantis, scene):
    """The truth among particles under the floor (every landmark behind their cameras)."""
    N, k = 40, 17
    T0 = np.repeat(scene["Twb"][None], N, axis=0).copy()
    rng = np.random.default_rng(3)
    for j in range(N):
        if j != k:
            T0[j] = T0[j] @ _rand(rng.normal(size=6), 0.05, 0.05)
            T0[j][2, 3] -= 10.0
    mantis.mcl_init_particles(T0, sigma_rot=0.0, sigma_t=0.0, tau=TAU, resample_frac=2.0, record=1)
    out, mo = mantis.mcl_step(_images(scene))
    rec = mantis.mcl_record()
    assert np.all(np.delete(rec["counts"], k, axis=0) == 0) and np.all(np.delete(rec["q"], k) == 0)
    assert mo.n_valid == 1 and mo.best == k and mo.resampled == 1 and mo.ess == 1.0
    assert np.all(rec["ancestors"] == k)
    assert np.array_equal(np.array(mo.T_w_b).reshape(4, 4), T0[k])
    assert np.all(np.array(mo.covariance) == 0.0) and np.all(np.array(out.covariance) == 0.0)
    Tn, Lw = mantis.mcl_particles()
    assert np.array_equal(Tn, np.repeat(T0[k][None], N, axis=0)) and np.all(Lw == 0.0)


def test_lost(mantis, scene):
    """Every camera blind (looking straight up from the base)."""
    N, sr, st = 12, 0.02, 0.01
    ext = [np.eye(4)] * 8
    T0 = _cloud(scene, N, 9)
    imgs = _images(scene)
    # one ordinary step first, so that the log-weights are not all zero
    mantis.mcl_init_particles(T0, sigma_rot=sr, sigma_t=st, tau=TAU, resample_frac=0.0, record=1)
    mantis.mcl_step(imgs)
    T1, L1 = mantis.mcl_particles()
    assert np.any(L1 != 0.0)
    prior = _cloud(scene, 2, 11)[1]
    mantis.prior_pose = prior
    mantis.rng_state = 1
    out, mo = mantis.mcl_step(_images(scene, ext=ext))
    gauss, state = O.gaussians(1, N * 6)
    assert mo.lost == 1 and out.publish == 0 and out.status == 0 and mo.resampled == 0
    assert mo.n_valid == 0 and mo.best == -1 and mo.weight_sum == 0
    assert mantis.rng_state == _next(state) == mo.rng_state_after == out.rng_state_after, "the draws still happen"
    rec = mantis.mcl_record()
    assert np.all(rec["counts"] == 0) and np.all(rec["q"] == 0) and np.all(rec["ancestors"] == -1)
    T2, L2 = mantis.mcl_particles()
    assert np.array_equal(T2, rec["T_pred"]) and np.array_equal(L2, L1)
    for j in range(N):
        np.testing.assert_allclose(T2[j], T1[j] @ _rand(gauss[6 * j: 6 * j + 6], sr, st), atol=POSE_TOL, rtol=0)
    assert np.array_equal(mantis.prior_pose, prior)
    mantis.prior_pose = None


def test_motion(mantis, scene):
    N = 9
    T0 = _cloud(scene, N, 13)
    a = math.radians(2.0)
    q = [0.0, math.sin(a / 2) * 0.6, math.sin(a / 2) * 0.8, math.cos(a / 2)]
    dp = [0.02, -0.01, 0.005]
    imgs = _images(scene)
    mantis.mcl_init_particles(T0, sigma_rot=0.0, sigma_t=0.0, tau=TAU, resample_frac=0.0, record=1)
    mantis.mcl_step(imgs, dp, q)
    Tp = mantis.mcl_record()["T_pred"]
    delta = _quat_T(q, dp)
    for j in range(N):
        np.testing.assert_allclose(Tp[j], T0[j] @ delta, atol=POSE_TOL, rtol=0)
    assert not np.allclose(Tp, T0, atol=1e-4, rtol=0)
    # an unset quaternion (all zeros) and no motion at all: the identity
    for args in (([0.5, 0.5, 0.5], [0, 0, 0, 0]), ()):
        mantis.mcl_init_particles(T0, sigma_rot=0.0, sigma_t=0.0, tau=TAU, resample_frac=0.0, record=1)
        mantis.mcl_step(imgs, *args)
        assert np.array_equal(mantis.mcl_record()["T_pred"], T0)


def test_init_draws_around_the_mean(mantis, scene):
    N, sr0, st0 = 21, 0.2, 0.3
    mantis.rng_state = 1
    mantis.mcl_init(scene["Twb"], sr0, st0, n_particles=N, tau=TAU)
    gauss, state = O.gaussians(1, N * 6)
    assert mantis.rng_state == state, "N x 6 gaussians and nothing else"
    T, L = mantis.mcl_particles()
    assert len(T) == N and np.all(L == 0.0)
    for j in range(N):
        np.testing.assert_allclose(T[j], scene["Twb"] @ _rand(gauss[6 * j: 6 * j + 6], sr0, st0), atol=POSE_TOL, rtol=0)
    with pytest.raises(Exception):
        mantis.mcl_record()  # no step yet
    mantis.mcl_reset()
    assert mantis.rng_state == state, "reset draws nothing"
    with pytest.raises(Exception):
        mantis.mcl_particles()


def test_host_and_device_frames(mantis, scene):
    import mantis_amd as M

    K, D = synth.intrinsics(W, H)
    T0 = _cloud(scene, 50, 17)
    kw = dict(sigma_rot=0.01, sigma_t=0.005, tau=TAU, resample_frac=2.0)
    mantis.rng_state = 1
    mantis.mcl_init_particles(T0, **kw)
    ho, hm = mantis.mcl_step(_images(scene))
    hT, hL = mantis.mcl_particles()
    fb = W * H * 3
    dev = mantis.device_alloc(fb * len(CAMS))
    try:
        imgs = []
        for i, c in enumerate(CAMS):
            mantis.h2d(dev + i * fb, scene["frames"][c])
            imgs.append(M.make_image(None, K, D, T_base_cam=scene["ext"][c], device_ptr=dev + i * fb, width=W, height=H))
        mantis.rng_state = 1
        mantis.mcl_init_particles(T0, **kw)
        do, dm = mantis.mcl_step(imgs)
        dT, dL = mantis.mcl_particles()
    finally:
        mantis.device_free(dev)
    assert bytes(hm) == bytes(dm) and bytes(ho) == bytes(do)
    assert np.array_equal(hT, dT) and np.array_equal(hL, dL)
    with pytest.raises(Exception):
        mantis.mcl_record()  # record = 0


def test_argument_errors(mantis, scene):
    import mantis_amd as M

    L = M.lib()
    imgs = _images(scene)
    arr3 = (M.MantisImage * 3)(*imgs)
    out, mo = M.MantisResult(), M.MantisMclResult()
    mantis.mcl_reset()
    mantis.rng_state = 77
    assert L.mantis_mcl_step(mantis.h, arr3, 3, None, C.byref(out), C.byref(mo)) == 5  # MANTIS_ERR_STATE
    assert "mcl" in L.mantis_last_error(mantis.h).decode()
    T0 = _cloud(scene, 5, 19)
    mantis.mcl_init_particles(T0, sigma_rot=0.01, sigma_t=0.01, tau=TAU, resample_frac=0.0)
    mantis.set_profiling(1)

    def unchanged():
        T, Lw = mantis.mcl_particles()
        return mantis.rng_state == 77 and np.array_equal(T, T0) and np.all(Lw == 0.0)

    big = np.ascontiguousarray(np.repeat(T0[:1], 4097, axis=0))
    bad = [({"n_particles": 0}, "n_particles"), ({"n_particles": 4097}, "n_particles"), ({"tau": 0.0}, "tau"),
           ({"tau": -1.0}, "tau"), ({"tau": float("nan")}, "tau"), ({"tau": float("inf")}, "tau"),
           ({"resample_frac": -0.01}, "resample_frac"), ({"resample_frac": 2.01}, "resample_frac"),
           ({"resample_frac": float("nan")}, "resample_frac"), ({"sigma_t": -1.0}, "sigma"),
           ({"sigma_rot": float("nan")}, "sigma"), ({"struct_size": 8}, "struct_size")]
    for kw, word in bad:
        p = mantis.mcl_params(n_particles=5, tau=TAU)
        for k, v in kw.items():
            setattr(p, k, v)
        for st in (L.mantis_mcl_init_particles(mantis.h, big.ctypes.data, C.byref(p)),
                   L.mantis_mcl_init(mantis.h, big.ctypes.data, 0.1, 0.1, C.byref(p))):
            assert st == 1 and word in L.mantis_last_error(mantis.h).decode(), kw  # MANTIS_ERR_ARG
        assert unchanged(), kw
    p = mantis.mcl_params(n_particles=5, tau=TAU)
    nanT = big.copy()
    nanT[3, 0, 0] = float("nan")
    assert L.mantis_mcl_init_particles(mantis.h, nanT.ctypes.data, C.byref(p)) == 1
    assert L.mantis_mcl_init(mantis.h, big.ctypes.data, float("nan"), 0.1, C.byref(p)) == 1
    assert L.mantis_mcl_init(mantis.h, None, 0.1, 0.1, C.byref(p)) == 1 and unchanged()
    # the step's own arguments
    small = M.make_image(np.zeros((360, 640, 3), np.uint8), *synth.intrinsics(640, 360))
    ring9 = _ring_images(scene) + [imgs[0]]
    mo_nan = M.MantisMotion()
    mo_nan.delta_quat_xyzw[3] = 1.0
    mo_nan.delta_pos[1] = float("nan")
    for images, motion, word in [([imgs[0], small], None, "size"), (ring9, None, "8"), (imgs, mo_nan, "motion"),
                                 ([], None, "n_cams")]:
        n = len(images)
        arr = (M.MantisImage * max(n, 1))(*images)
        st = L.mantis_mcl_step(mantis.h, arr, n, None if motion is None else C.byref(motion), C.byref(out), C.byref(mo))
        assert st == 1 and word in L.mantis_last_error(mantis.h).decode(), word
        assert unchanged(), word
    assert L.mantis_mcl_step(mantis.h, arr3, 3, None, None, C.byref(mo)) == 1 and unchanged()
    # no map: a fresh context
    m2 = M.Mantis(max_cams=1, max_width=W, max_height=H)
    try:
        m2.mcl_init_particles(T0, tau=TAU)
        arr = (M.MantisImage * 1)(imgs[0])
        assert L.mantis_mcl_step(m2.h, arr, 1, None, C.byref(out), C.byref(mo)) == 1
        assert "map" in L.mantis_last_error(m2.h).decode()
    finally:
        m2.close()
    # nothing was launched by the rejected calls: the next step's marks are its own, 4 launches after the image stages
    mantis.mcl_step(imgs)
    names = [n for n, _ in mantis.kernel_times()]
    mantis.set_profiling(0)
    assert [n.split("/")[0] for n in names if n.startswith("mcl_")] == ["mcl_predict", "mcl_score", "mcl_weight",
                                                                        "mcl_resample"]
    assert sum(n.startswith("canny") for n in names) == 1 and sum(n.startswith("morph") for n in names) == 1
    assert mantis.rng_state != 77
