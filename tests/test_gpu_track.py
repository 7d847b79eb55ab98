"""Rig tracking on the GPU (mantis_track / mantis_track_batch): the joint
multi-camera particle filter from a pose prior against its definition
(include/mantis.h): every recorded (particle, camera) scored by the CPU oracle
(exact integer sums and counts), the particles' poses against the numpy form
of the perturbation rule, and pool / pick / gate recomputed in Python from
the recorded integers (bit equality). 1280x720 synthetic rigs: one 8-camera
ring (its cameras also serve as the 1-, 2- and 3-camera rigs) and two more
base poses seen by two cameras.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _oracle as O
from mantis_amd import synth

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-9
DBL_MAX = np.finfo(np.float64).max
W, H = 1280, 720


@pytest.fixture(scope="module")
def mantis(landmark_map):
    import mantis_amd as M

    m = M.Mantis(max_cams=8, max_width=W, max_height=H)
    m.set_map(*landmark_map)
    yield m
    m.close()


def _shift(T):
    """The prediction: the truth moved by 2 cm and turned by 1 degree."""
    d = np.eye(4)
    d[:3, :3] = synth.rot_z(math.radians(1.0))
    d[:3, 3] = [0.02, 0.0, 0.0]
    return T @ d


@pytest.fixture(scope="module")
def scene():
    """frames[r][c]: rig r (base pose Twb[r]) seen by ring camera c; rig 0 by
    all 8, rigs 1 and 2 by cameras 0 and 4."""
    rng = np.random.default_rng(2024)
    ext = synth.rig_extrinsics(8)
    Twb, frames = [], []
    for r in range(3):
        T = synth.random_base_pose(rng)
        Twb.append(T)
        fr = {}
        for c in (range(8) if r == 0 else (0, 4)):
            Twc = T @ ext[c]
            fr[c] = synth.render_host(synth.make_cam(Twc[:3, :3], Twc[:3, 3], W, H), synth.frame_seed(12, 100 * r + c))
        frames.append(fr)
    return {"ext": ext, "Twb": Twb, "frames": frames, "cleaned": {}}


def _images(scene, r, cams, ext=None):
    import mantis_amd as M

    K, D = synth.intrinsics(W, H)
    return [M.make_image(scene["frames"][r][c], K, D, T_base_cam=(ext or scene["ext"])[c]) for c in cams]


def _cleaned(scene, r, c):
    """The frame as the fast evaluator sees it: img.copyTo(out, cleanImageByEdge mask)."""
    key = (r, c)
    if key not in scene["cleaned"]:
        img = scene["frames"][r][c]
        mask = O.clean_mask(O.canny(img))
        out = img.copy()
        out[mask == 0] = 0
        scene["cleaned"][key] = out
    return scene["cleaned"][key]


def _pooled(sums, counts):
    """E = (double)sum(sum_c) / ((double)sum(n_c) * 1.1), DBL_MAX when no landmark; n."""
    S = sums.astype(np.int64).sum(axis=1)
    N = counts.astype(np.int64).sum(axis=1)
    E = np.full(len(S), DBL_MAX)
    ok = N > 0
    E[ok] = S[ok].astype(np.float64) / (N[ok].astype(np.float64) * 1.1)
    return E, N


def _rand(g6, sr, st):
    """Transform(setRPY(roll, pitch, yaw), (x, y, z)) from gaussians drawn yaw, pitch, roll, z, y, x."""
    g = [float(v) for v in g6]
    T = np.eye(4)
    T[:3, :3] = synth.rot_z(g[0] * sr) @ synth.rot_y(g[1] * sr) @ synth.rot_x(g[2] * sr)
    T[:3, 3] = [g[5] * st, g[4] * st, g[3] * st]
    return T


def _replay(m, res, rig, P, I, pred, gauss=None, sr=0.03, st=0.01, min_projections=10, max_error=0.0):
    """Pool, pick, iter_err, iter_pick, error, n_proj, tracked and T_w_b of one
    rig recomputed from its record; with `gauss` (the rig's draws) also every
    particle's pose against the perturbation rule. Returns the records."""
    recs = {}
    T0, c2w0, s0, n0 = m.track_record(rig, -1)
    recs[0] = (T0, c2w0, s0, n0)
    assert len(T0) == 1
    np.testing.assert_allclose(T0[0], pred, atol=POSE_TOL, rtol=0)
    E, N = _pooled(s0, n0)
    cur_err, cur_n, cur_T = E[0], int(N[0]), T0[0]
    assert res.seed_error == cur_err and res.iter_err[0] == cur_err
    for k in range(1, I + 1):
        Tk, c2wk, sk, nk = m.track_record(rig, k)
        recs[k] = (Tk, c2wk, sk, nk)
        assert len(Tk) == P
        if gauss is not None:
            for j in range(P):
                ref = cur_T @ _rand(gauss[((k - 1) * P + j) * 6: ((k - 1) * P + j) * 6 + 6], sr, st)
                np.testing.assert_allclose(Tk[j], ref, atol=POSE_TOL, rtol=0, err_msg=f"iteration {k} particle {j}")
        E, N = _pooled(sk, nk)
        j = int(np.argmin(E))  # the first minimum: argmin by (E, j)
        pick = -1
        if E[j] < cur_err:
            pick, cur_err, cur_n, cur_T = j, E[j], int(N[j]), Tk[j]
        assert res.iter_pick[k - 1] == pick, f"iteration {k}: pick {res.iter_pick[k - 1]} vs {pick}"
        assert res.iter_err[k] == cur_err, f"iteration {k}"
    assert res.error == cur_err and res.n_proj == cur_n
    assert res.n_scored == 1 + P * I
    assert np.array_equal(np.array(res.T_w_b).reshape(4, 4), cur_T)
    want = int(cur_err != DBL_MAX and cur_n >= min_projections and (max_error <= 0 or cur_err <= max_error))
    assert res.tracked == want
    return recs


def test_exact_scoring_every_iteration(mantis, scene, landmark_map):
    """1 rig x 3 cameras, 7 particles (neither a wave nor a block's chunk of
    8), 3 iterations: every recorded (particle, camera) against the oracle."""
    cams, P, I = (0, 3, 5), 7, 3
    K, D = synth.intrinsics(W, H)
    orc = O.Oracle(*landmark_map)
    pred = _shift(scene["Twb"][0])
    mantis.rng_state = 1
    res = mantis.track_batch(_images(scene, 0, cams), 1, pred, particles=P, iterations=I, record=1)[0]
    gauss, state = O.gaussians(1, P * I * 6)
    assert res.status == 0 and res.rng_state_after == state == mantis.rng_state
    recs = _replay(mantis, res, 0, P, I, pred, gauss)
    for k, (Tk, c2wk, sk, nk) in recs.items():
        for ci, c in enumerate(cams):
            ref = np.array([np.linalg.inv(T @ scene["ext"][c]) for T in Tk])
            ref12 = np.concatenate([ref[:, :3, :3].reshape(-1, 9), ref[:, :3, 3]], axis=1)
            np.testing.assert_allclose(c2wk[:, ci], ref12, atol=POSE_TOL, rtol=0)
            err, npj = orc.score(_cleaned(scene, 0, c), K, D, c2wk[:, ci], fast=True)
            assert np.array_equal(nk[:, ci], npj), f"pass {k} camera {c}: counts"
            osum = np.where(npj > 0, np.rint(np.where(npj > 0, err, 0.0) * npj * 1.1), 0).astype(np.int64)
            assert np.array_equal(sk[:, ci], osum), f"pass {k} camera {c}: sums"
    assert res.tracked == 1 and res.error <= res.seed_error


@pytest.mark.parametrize("P,cams,I", [(96, (0,), 2), (64, tuple(range(8)), 2), (1, (0, 4), 3), (50, (0, 4), 0)],
                         ids=["96x1", "64x8", "1-particle", "0-iterations"])
def test_shapes_that_break_loops(mantis, scene, P, cams, I):
    """Two lane rounds in the argmin (96 particles), the 512-task cap on
    max_cams = 8 cameras, one particle, no iteration."""
    pred = _shift(scene["Twb"][0])
    mantis.rng_state = 1
    res = mantis.track_batch(_images(scene, 0, cams), 1, pred, particles=P, iterations=I, record=1)[0]
    gauss, state = O.gaussians(1, P * I * 6)
    assert res.rng_state_after == state == mantis.rng_state
    _replay(mantis, res, 0, P, I, pred, gauss)
    if I == 0:  # the result is the seed, nothing drawn
        assert mantis.rng_state == 1 and res.error == res.seed_error and res.n_scored == 1
        np.testing.assert_allclose(np.array(res.T_w_b).reshape(4, 4), pred, atol=POSE_TOL, rtol=0)
        with pytest.raises(Exception):
            mantis.track_record(0, 1)


def test_screen_off_equals_screen_on(mantis, scene, landmark_map):
    """A context created with MANTIS_SCREEN=0 sends every landmark of every
    (particle, camera) through the exact fallback -- the scoring blocks'
    queues overflow, so the in-place path runs, then the drains -- and must
    record the same integer sums and counts in every pass and return the same
    result record from the same RNG state. 11 particles: a full chunk of 8
    and a tail of 3 per camera."""
    import os

    import mantis_amd as M

    cams, P, I = (0, 3, 5), 11, 2
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
        pred = _shift(scene["Twb"][0])
        got = []
        for m in (mx, mantis):
            m.rng_state = 1
            res = m.track_batch(_images(scene, 0, cams), 1, pred, particles=P, iterations=I, record=1)[0]
            got.append((bytes(res), [m.track_record(0, k) for k in (-1, 1, 2)], m.rng_state))
        (rx, px, sx), (rs, ps, ss) = got
        for k, (a, b) in enumerate(zip(px, ps)):
            assert a[2].shape == b[2].shape == ((1 if k == 0 else P), len(cams))
            assert np.array_equal(a[2], b[2]), f"pass {k}: sums"
            assert np.array_equal(a[3], b[3]), f"pass {k}: counts"
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"pass {k}: poses"
        assert rx == rs and sx == ss
    finally:
        mx.close()


def test_ties(mantis, scene):
    """sigma 0: every particle equals the current pose, none is strictly better."""
    pred = _shift(scene["Twb"][0])
    res = mantis.track_batch(_images(scene, 0, (0, 3, 5)), 1, pred, particles=9, iterations=4, sigma_rot=0.0,
                             sigma_t=0.0, record=1)[0]
    assert list(res.iter_pick) == [-1] * 10
    assert all(e == res.seed_error for e in res.iter_err) and res.error == res.seed_error
    assert np.array_equal(np.array(res.T_w_b).reshape(4, 4), pred)
    _, _, s0, n0 = mantis.track_record(0, -1)
    for k in range(1, 5):
        _, _, sk, nk = mantis.track_record(0, k)
        assert np.array_equal(sk, np.repeat(s0, 9, axis=0)) and np.array_equal(nk, np.repeat(n0, 9, axis=0))


def _blind_ext():
    """A camera looking straight up from the base: every landmark is behind it."""
    return np.eye(4)


def test_blind_cameras(mantis, scene):
    P, I = 5, 2
    pred = _shift(scene["Twb"][0])
    ext = list(scene["ext"])
    ext[4] = _blind_ext()
    mantis.rng_state = 1
    res = mantis.track_batch(_images(scene, 0, (0, 4), ext), 1, pred, particles=P, iterations=I, record=1)[0]
    recs = _replay(mantis, res, 0, P, I, pred)
    for k, (_, _, sk, nk) in recs.items():
        assert np.all(nk[:, 1] == 0) and np.all(sk[:, 1] == 0)
        assert np.all(nk[:, 0] > 0)
    mantis.rng_state = 1
    one =mantis.track_batch(_images(scene, 0, (0,)), 1, pred, particles=P, iterations=I)[0]
    assert bytes(one) == bytes(res), "the pooled error is the seeing camera's alone"
    # both blind: nothing scored, the draws still happen, the prior stays
    ext[0] = _blind_ext()
    mantis.rng_state = 1
    res = mantis.track_batch(_images(scene, 0, (0, 4), ext), 1, pred, particles=P, iterations=I)[0]
    assert res.error == DBL_MAX and res.seed_error == DBL_MAX and res.tracked == 0 and res.n_proj == 0
    assert list(res.iter_pick) == [-1] * 10
    assert mantis.rng_state == O.gaussians(1, P * I * 6)[1] == res.rng_state_after
    mantis.prior_pose = pred
    mantis.rng_state = 1
    out, tout = mantis.track(_images(scene, 0, (0, 4), ext), particles=P, iterations=I)
    assert out.publish == 0 and tout.tracked == 0 and out.num_particles == 1 + P * I
    assert np.array_equal(mantis.prior_pose, pred)
    assert mantis.rng_state == O.gaussians(1, P * I * 6)[1]
    mantis.prior_pose = None


def _batch_inputs(scene):
    imgs, preds = [], []
    for r in range(3):
        imgs += _images(scene, r, (0, 4))
        preds.append(_shift(scene["Twb"][r]))
    return imgs, np.array(preds)


def test_batch_equals_sequence(mantis, scene):
    P, I = 11, 3
    imgs, preds = _batch_inputs(scene)
    mantis.rng_state = 1
    batch = mantis.track_batch(imgs, 3, preds, particles=P, iterations=I)
    mantis.rng_state = 1
    for r in range(3):
        one = mantis.track_batch(imgs[2 * r: 2 * r + 2], 1, preds[r], particles=P, iterations=I)[0]
        for name, _ in type(one)._fields_:
            a, b = getattr(one, name), getattr(batch[r], name)
            if hasattr(a, "__len__"):
                a, b = list(a), list(b)
            assert a == b, f"rig {r}: {name}"
        assert batch[r].rng_state_after == O.gaussians(1, (r + 1) * P * I * 6)[1] == mantis.rng_state
        assert batch[r].tracked == 1


def test_host_and_device_frames(mantis, scene):
    import mantis_amd as M

    K, D = synth.intrinsics(W, H)
    cams = (0, 3, 5)
    pred = _shift(scene["Twb"][0])
    mantis.rng_state = 1
    host = mantis.track_batch(_images(scene, 0, cams), 1, pred, particles=13, iterations=2)[0]
    fb = W * H * 3
    dev = mantis.device_alloc(fb * len(cams))
    try:
        imgs = []
        for i, c in enumerate(cams):
            mantis.h2d(dev + i * fb, scene["frames"][0][c])
            imgs.append(M.make_image(None, K, D, T_base_cam=scene["ext"][c], device_ptr=dev + i * fb, width=W, height=H))
        mantis.rng_state = 1
        devr = mantis.track_batch(imgs, 1, pred, particles=13, iterations=2)[0]
    finally:
        mantis.device_free(dev)
    assert bytes(host) == bytes(devr)


def _quat_T(q, p):
    x, y, z, w = q
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                 [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                 [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = p
    return T


def test_track_plumbing(mantis, scene):
    import mantis_amd as M

    cams = (0, 3, 5)
    imgs = _images(scene, 0, cams)
    arr = (M.MantisImage * 3)(*imgs)
    p = mantis.track_params(particles=6, iterations=2, record=1)
    out, tout = M.MantisResult(), M.MantisTrackResult()
    mantis.prior_pose = None
    st = M.lib().mantis_track(mantis.h, arr, 3, None, C.byref(p), C.byref(out), C.byref(tout))
    assert st == 5 and b"prior" in M.lib().mantis_last_error(mantis.h)  # MANTIS_ERR_STATE
    # prior = the truth moved back by the motion: the prediction is prior @ Transform(delta)
    a = math.radians(1.0)
    q = [0.0, 0.0, math.sin(a / 2), math.cos(a / 2)]
    dp = [0.02, -0.01, 0.005]
    delta = _quat_T(q, dp)
    prior = scene["Twb"][0] @ np.linalg.inv(delta) @ _quat_T([0, 0, math.sin(0.004), math.cos(0.004)], [0.01, 0, 0])
    mantis.prior_pose = prior
    mantis.rng_state = 1
    out, tout = mantis.track(imgs, dp, q, particles=6, iterations=2, record=1)
    T0, _, _, _ = mantis.track_record(0, -1)
    np.testing.assert_allclose(T0[0], prior @ delta, atol=POSE_TOL, rtol=0)
    assert tout.tracked == 1 and out.publish == 1 and out.status == 0
    Tw = np.array(tout.T_w_b).reshape(4, 4)
    assert np.array_equal(mantis.prior_pose, Tw)
    cov = np.array(out.covariance).reshape(6, 6)
    assert np.array_equal(cov, np.diag([tout.error * (1.0 / 600.0)] * 6))  # PosePub.h:47: error * coefficient
    np.testing.assert_allclose(np.diag(cov), tout.error / 600.0, rtol=1e-15)
    assert out.weight == tout.error and out.num_particles == tout.n_scored == 13
    assert out.n_quads == 0 and out.min_yaw_diff == 0 and out.rng_state_after == mantis.rng_state
    np.testing.assert_allclose(np.array(out.position), Tw[:3, 3], atol=0, rtol=0)
    np.testing.assert_allclose(_quat_T(list(out.orientation_xyzw), Tw[:3, 3]), Tw, atol=POSE_TOL, rtol=0)
    # an unset motion (all zeros) and no motion: the prior itself
    mantis.prior_pose = prior
    mantis.track(imgs, [0, 0, 0], [0, 0, 0, 0], particles=6, iterations=1, record=1)
    assert np.array_equal(mantis.track_record(0, -1)[0][0], prior)
    mantis.prior_pose = None


def test_argument_errors(mantis, scene):
    import mantis_amd as M

    L = M.lib()
    ring = _images(scene, 0, range(8))
    pred = np.array([_shift(scene["Twb"][0])] * 3)
    mantis.set_profiling(1)
    mantis.rng_state = 77

    def call(images, rigs, **kw):
        n = len(images)
        arr = (M.MantisImage * n)(*images)
        p = mantis.track_params()
        for k, v in kw.items():
            setattr(p, k, v)
        out = (M.MantisTrackResult * max(rigs, 1))()
        st = L.mantis_track_batch(mantis.h, arr, rigs, n // max(rigs, 1), pred.ctypes.data, C.byref(p), out)
        return st, L.mantis_last_error(mantis.h).decode()

    small = M.make_image(np.zeros((360, 640, 3), np.uint8), *synth.intrinsics(640, 360))
    bad = [
        (ring + [ring[0]], 3, {}, "max_cams"),               # 3 x 3 = 9 frames on max_cams = 8
        (ring + [ring[0]], 1, {}, "cams_per_rig"),           # 9 cameras in one rig
        (ring[:6], 1, {"particles": 96}, "512"),              # 96 x 6 = 576 tasks
        ([ring[0], small], 1, {}, "size"),
        (ring[:2], 1, {"particles": 0}, "particles"),
        (ring[:2], 1, {"particles": 97}, "particles"),
        (ring[:2], 1, {"iterations": -1}, "iterations"),
        (ring[:2], 1, {"iterations": 11}, "iterations"),
        (ring[:2], 1, {"sigma_rot": -0.1}, "sigma"),
        (ring[:2], 1, {"sigma_t": -0.1}, "sigma"),
        (ring[:2], 1, {"sigma_t": float("nan")}, "sigma"),
        (ring[:2], 1, {"struct_size": 8}, "struct_size"),
        (ring[:2], 0, {}, "n_rigs"),
    ]
    for images, rigs, kw, word in bad:
        st, msg = call(images, rigs, **kw)
        assert st == 1 and word in msg, (kw, st, msg)  # MANTIS_ERR_ARG
    assert mantis.rng_state == 77, "a rejected call draws nothing"
    # no map: a fresh context
    m2 = M.Mantis(max_cams=1, max_width=W, max_height=H)
    try:
        arr = (M.MantisImage * 1)(ring[0])
        p = m2.track_params()
        out = M.MantisTrackResult()
        assert L.mantis_track_batch(m2.h, arr, 1, 1, pred.ctypes.data, C.byref(p), C.byref(out)) == 1
        assert "map" in L.mantis_last_error(m2.h).decode()
    finally:
        m2.close()
    # nothing was launched by the rejected calls: the next call's stage marks are
    # exactly its own (image stages, then 2 x iterations + 3 tracking launches)
    mantis.track_batch(ring[:2], 1, pred[0], particles=5, iterations=2)
    names = [n for n, _ in mantis.kernel_times()]
    mantis.set_profiling(0)
    assert sum(n.startswith("track_particles") for n in names) == 4
    assert sum(n.startswith("track_score") for n in names) == 3
    assert sum(n.startswith("canny") for n in names) == 1 and sum(n.startswith("morph") for n in names) == 1


def test_monotone(mantis, scene):
    imgs, preds = _batch_inputs(scene)
    mantis.rng_state = 1
    for res in mantis.track_batch(imgs, 3, preds):
        e = list(res.iter_err)
        assert all(b <= a for a, b in zip(e, e[1:])) and res.error <= res.seed_error and res.error == e[10]
        assert res.tracked == 1 and res.n_scored == 501


def test_process_undisturbed_after_track(mantis, scene, landmark_map):
    """A mantis_process call after a track call still matches the oracle."""
    from test_gpu_parity import _cmp_debug

    import mantis_amd as M

    K, D = synth.intrinsics(W, H)
    mantis.track_batch(_images(scene, 0, (0, 3, 5)), 1, _shift(scene["Twb"][0]), particles=7, iterations=1)
    img = scene["frames"][1][0]
    mantis.rng_state = 1
    mantis.prior_pose = None
    _, cams = mantis.process([M.make_image(img, K, D)])
    orc = O.Oracle(*landmark_map, seed=1)
    o = orc.process(img, K, D)
    _cmp_debug(mantis.frame_debug(0), o, "after track")
    assert cams[0].reason == o.reason and cams[0].publish == o.publish
    assert mantis.rng_state == orc.rng_state
