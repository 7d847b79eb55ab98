"""Line refinement on the GPU (mantis_refine / mantis_refine_batch): every
recorded pass against the host build of the same rules (mk_refine.h through
hc_refine_obs, fed the device's own recorded pose so that a flipped tie cannot
cascade), the MFMA accumulators against numpy sums of the recorded rows, each
step against gn_solve6 on the device's accumulators, the whole call against
hc_refine_seq, the shapes that break loops, the plumbing around the context's
prior and the argument errors. 1280x720 synthetic rigs (tests/_refine_ref.py).
"""
import ctypes as C
import math

import numpy as np
import pytest

import _refine_ref as RR
from mantis_amd import synth

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-9
W, H = RR.W, RR.H_


@pytest.fixture(scope="module")
def mantis(landmark_map):
    import mantis_amd as M

    m = M.Mantis(max_cams=12, max_width=W, max_height=H)
    m.set_map(*landmark_map)
    yield m
    m.close()


@pytest.fixture(scope="module")
def lm(landmark_map):
    return RR.all_landmarks(landmark_map)


@pytest.fixture(scope="module")
def rigs4():
    """Three four-camera rigs; rig 0 is the CPU test's scene."""
    return RR.rig_scene(4, 3)


@pytest.fixture(scope="module")
def ring8():
    return RR.rig_scene(8, 1)


def _images(frames, exts, w=W, h=H, Ks=None, Ds=None):
    import mantis_amd as M

    Ks, Ds = RR.lenses(len(frames), w, h, Ks, Ds)
    return [M.make_image(f, K, D, T_base_cam=e) for f, e, K, D in zip(frames, exts, Ks, Ds)]


def _check_call(m, lm, frames, exts, T0, landmarks=None, Ks=None, Ds=None, whole_call=True, **params):
    """One rig, record = 1: every pass against the host rules; returns the result. Ks, Ds: per-camera lenses
    (default: the bench lens); whole_call = False leaves out the comparison with hc_refine_seq (a cell whose
    iteration the host alone does not reproduce under a 1e-13 change of D, tests/_line_cases.py)."""
    X, nw, nr, ng = landmarks or lm
    h, w = frames[0].shape[:2]
    Cn = len(frames)
    Ks, Ds = RR.lenses(Cn, w, h, Ks, Ds)
    res = m.refine_batch(_images(frames, exts, w, h, Ks, Ds), 1, T0, record=1, **params)[0]
    p = m.refine_params(**params)
    f = RR.flags(X, p.landmark_pitch)
    nc = len(RR.candidates(f))
    assert res.n_cand == nc
    flagged = total = 0
    Ts, accs = [], []
    for k in range(res.iterations_run + 1):
        T, codes, Sw, Skw, rows, acc = m.refine_record(0, k)
        Ts.append(T)
        accs.append(acc)
        assert codes.shape == (Cn * nc,)
        for c in range(Cn):
            hc_, hSw, hSkw, hrows, tie = RR.obs(T, exts[c], Ks[c], Ds[c], frames[c], X, nw, nr, ng, f,
                                                 R=p.half_window, white_thresh=p.white_thresh,
                                                 min_weight=p.min_weight)
            sl = slice(c * nc, (c + 1) * nc)
            ok = tie == 0
            flagged += int((~ok).sum())
            total += nc
            assert np.array_equal(codes[sl][ok], hc_[ok]), f"pass {k} camera {c}: codes"
            assert np.array_equal(Sw[sl][ok], hSw[ok]) and np.array_equal(Skw[sl][ok], hSkw[ok]), f"pass {k} camera {c}"
            np.testing.assert_allclose(rows[sl][ok], hrows[ok], rtol=1e-12, atol=0, err_msg=f"pass {k} camera {c}")
        assert np.all(rows[codes != 0] == 0.0)
        n_obs = int((codes == 0).sum())
        assert res.n_obs[k] == n_obs
        ref = RR.np_acc28(rows)
        np.testing.assert_allclose(acc, ref, rtol=1e-12, atol=1e-14 * np.abs(ref).max())
        assert res.rms[k] == (math.sqrt(acc[27] / n_obs) if n_obs else 0.0)
    assert flagged <= 0.005 * total, (flagged, total)
    assert np.array_equal(Ts[0], np.asarray(T0)), "pass 0 observes at the input pose"
    for k in range(res.iterations_run):
        ok, Tn, d6 = RR.solve6(accs[k], p.lambda_, Ts[k])
        assert ok
        np.testing.assert_allclose(Ts[k + 1], Tn, rtol=0, atol=1e-12, err_msg=f"step {k}")
        np.testing.assert_allclose(np.array(res.delta[k]), d6, rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.array(res.T_w_b).reshape(4, 4), Ts[-1], rtol=0, atol=0)
    if flagged == 0 and whole_call:
        host = RR.seq(T0, exts, frames, X, nw, nr, ng, p, Ks, Ds)
        np.testing.assert_allclose(np.array(res.T_w_b), np.array(host.T_w_b), rtol=0, atol=POSE_TOL)
        assert list(res.n_obs) == list(host.n_obs)
        assert (res.iterations_run, res.refined, res.status) == (host.iterations_run, host.refined, host.status)
        if res.refined:
            # two inversions of normal matrices that differ in their last bits: cond(A) eps, far below 1e-8
            hcov = np.array(host.covariance)
            np.testing.assert_allclose(np.array(res.covariance), hcov, rtol=0, atol=1e-8 * np.abs(hcov).max())
    return res


@pytest.mark.parametrize("shape", ["four-cameras", "one-camera", "eight-cameras", "I=0", "I=10", "R=1", "R=15"])
def test_record_parity(mantis, lm, rigs4, ring8, shape):
    sc = ring8 if shape == "eight-cameras" else rigs4
    cams = {"one-camera": [0], "eight-cameras": list(range(8))}.get(shape, [0, 1, 2, 3])
    params = {"I=0": {"iterations": 0}, "I=10": {"iterations": 10}, "R=1": {"half_window": 1},
              "R=15": {"half_window": 15}}.get(shape, {})
    T = sc["Twb"][0]
    T0 = RR.shift(T)
    res = _check_call(mantis, lm, [sc["frames"][0][c] for c in cams], [sc["ext"][c] for c in cams], T0, **params)
    Tr = np.array(res.T_w_b).reshape(4, 4)
    print(shape, res.status, res.refined, res.iterations_run, list(res.n_obs), RR.pose_dist(T0, T), RR.pose_dist(Tr, T))
    if shape == "I=0":
        assert np.array_equal(Tr, T0) and res.iterations_run == 0 and res.status == 0
    elif shape == "R=1":
        assert res.status in (0, 1, 2)  # a three-sample window holds few lines 2 cm away: whatever the rule says
    else:
        assert res.status == 0 and res.refined == 1 and res.iterations_run == (10 if shape == "I=10" else 4)


def test_odd_candidate_count(mantis, lm, rigs4, landmark_map):
    """A map whose candidate count is odd: the last trip of a block has one half idle."""
    w, r, g = landmark_map
    for drop in range(1, 8):
        X = np.concatenate([w[drop:], r, g])
        nc = len(RR.candidates(RR.flags(X, 0.08)))
        if nc % 2 == 1:
            break
    assert nc % 2 == 1 and nc % 32 != 0
    try:
        mantis.set_map(w[drop:], r, g)
        assert np.array_equal(mantis.line_flags(0.08), RR.flags(X, 0.08))
        landmarks = (np.ascontiguousarray(X), len(w) - drop, len(r), len(g))
        res = _check_call(mantis, lm, rigs4["frames"][0][:3], rigs4["ext"][:3], RR.shift(rigs4["Twb"][0]),
                          landmarks=landmarks)
        assert res.n_cand == nc and res.refined == 1
    finally:
        mantis.set_map(w, r, g)
    assert np.array_equal(mantis.line_flags(0.08), RR.flags(lm[0], 0.08))


@pytest.mark.parametrize("cls,Cn", RR.TAIL_CASES)
def test_trip_loop_tails(mantis, lm, rigs4, landmark_map, cls, Cn):
    """Cn cameras on a map cut until the rig's Cn n_cand rows end the accumulation's trip loop another way
    (RR.ROW_CLASSES, RR.TAIL_CASES; the full map's rigs have 540 rows per camera, so every wave has whole trips
    there). The few rows of the smallest class leave the pass STARVED: its record is written all the same."""
    cut, landmarks, nc = RR.cut_map(landmark_map, cls, per=Cn)
    try:
        mantis.set_map(*cut)
        res = _check_call(mantis, lm, rigs4["frames"][0][:Cn], rigs4["ext"][:Cn], RR.shift(rigs4["Twb"][0]),
                          landmarks=landmarks)
        assert res.n_cand == nc and RR.ROW_CLASSES[cls](Cn * res.n_cand)
        print(cls, nc, res.status, res.iterations_run, list(res.n_obs)[:5])
    finally:
        mantis.set_map(*landmark_map)


def test_line_flags_on_the_context(mantis, lm):
    X = lm[0]
    for pitch in (0.08, 0.32, 0.05, 0.08):
        assert np.array_equal(mantis.line_flags(pitch), RR.np_flags(X, pitch))


def test_blind_cameras(mantis, lm, rigs4):
    fr, ext, T0 = rigs4["frames"][0], list(rigs4["ext"]), RR.shift(rigs4["Twb"][0])
    nc = 540
    ext_b = [ext[0], np.eye(4), ext[2]]  # the middle camera looks straight up: every landmark is behind it
    res = _check_call(mantis, lm, fr[:3], ext_b, T0)
    T, codes, Sw, Skw, rows, acc = mantis.refine_record(0, 0)
    assert np.all(codes[nc: 2 * nc] == 1) and not rows[nc: 2 * nc].any() and not Sw[nc: 2 * nc].any()
    two = mantis.refine_batch(_images([fr[0], fr[2]], [ext[0], ext[2]]), 1, T0, record=1)[0]
    T2, codes2, Sw2, Skw2, rows2, acc2 = mantis.refine_record(0, 0)
    # the sighted cameras' slots are the same bits with or without the blind one between them
    assert np.array_equal(codes[:nc], codes2[:nc]) and np.array_equal(codes[2 * nc:], codes2[nc:])
    assert np.array_equal(rows[:nc], rows2[:nc]) and np.array_equal(rows[2 * nc:], rows2[nc:])
    assert res.n_obs[0] == two.n_obs[0] and res.refined == two.refined == 1
    np.testing.assert_allclose(np.array(res.T_w_b), np.array(two.T_w_b), rtol=0, atol=POSE_TOL)
    # all blind: STARVED in pass 0, the pose unchanged, nothing published, the prior stays
    blind = [np.eye(4)] * 3
    res = _check_call(mantis, lm, fr[:3], blind, T0)
    assert (res.status, res.refined, res.iterations_run, res.n_obs[0]) == (1, 0, 0, 0)
    assert np.array_equal(np.array(res.T_w_b).reshape(4, 4), T0) and not np.array(res.covariance).any()
    with pytest.raises(Exception):
        mantis.refine_record(0, 1)  # the pass did not run
    mantis.prior_pose = T0
    out, rout = mantis.refine(_images(fr[:3], blind))
    assert out.publish == 0 and out.status == 0 and rout.status == 1 and out.num_particles == 0
    assert np.array_equal(mantis.prior_pose, T0)
    mantis.prior_pose = None


def test_small_pitched_frame(mantis, lm):
    """322 x 242 (neither a multiple of 4) with step_bytes > 3 W: staged through the pitch conversion."""
    import mantis_amd as M

    w, h = 322, 242
    sc = RR.rig_scene(2, 1, seed=7, w=w, h=h)
    T0 = RR.shift(sc["Twb"][0])
    res = _check_call(mantis, lm, sc["frames"][0], sc["ext"], T0)
    K, D = synth.intrinsics(w, h)
    imgs, keep = [], []
    for fr, e in zip(sc["frames"][0], sc["ext"]):
        buf = np.full((h, 3 * w + 34), 0xAB, np.uint8)  # rows 1000 bytes apart
        buf[:, : 3 * w] = fr.reshape(h, 3 * w)
        keep.append(buf)
        im = M.make_image(fr, K, D, T_base_cam=e)
        im.bgr = buf.ctypes.data
        im.step_bytes = buf.strides[0]
        imgs.append(im)
    assert imgs[0].step_bytes == 1000 > 3 * w
    pitched = mantis.refine_batch(imgs, 1, T0)[0]
    assert bytes(pitched) == bytes(res)


def test_host_and_device_frames(mantis, rigs4):
    import mantis_amd as M

    K, D = synth.intrinsics(W, H)
    fr, ext, T0 = rigs4["frames"][0], rigs4["ext"], RR.shift(rigs4["Twb"][0])
    host = mantis.refine_batch(_images(fr, ext), 1, T0)[0]
    fb = W * H * 3
    dev = mantis.device_alloc(fb * 4)
    try:
        imgs = []
        for i in range(4):
            mantis.h2d(dev + i * fb, fr[i])
            imgs.append(M.make_image(None, K, D, T_base_cam=ext[i], device_ptr=dev + i * fb, width=W, height=H))
        devr = mantis.refine_batch(imgs, 1, T0)[0]
    finally:
        mantis.device_free(dev)
    assert bytes(host) == bytes(devr) and host.refined == 1


def test_batch_equals_single_calls(mantis, rigs4):
    imgs, T0s = [], []
    for r in range(3):
        imgs += _images(rigs4["frames"][r], rigs4["ext"])
        T0s.append(RR.shift(rigs4["Twb"][r]))
    batch = mantis.refine_batch(imgs, 3, np.array(T0s), record=1)
    recs = [mantis.refine_record(r, 1) for r in range(3)]
    for r in range(3):
        one = mantis.refine_batch(imgs[4 * r: 4 * r + 4], 1, T0s[r], record=1)[0]
        assert bytes(one) == bytes(batch[r]), f"rig {r}"
        for a, b in zip(mantis.refine_record(0, 1), recs[r]):
            assert np.array_equal(a, b)
        assert one.refined == 1
        print(r, RR.pose_dist(T0s[r], rigs4["Twb"][r]), RR.pose_dist(np.array(one.T_w_b).reshape(4, 4), rigs4["Twb"][r]))


def _quat_T(q, p):
    x, y, z, w = q
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                 [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                 [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = p
    return T


def test_refine_plumbing(mantis, rigs4):
    import mantis_amd as M

    fr, ext, Tt = rigs4["frames"][0], rigs4["ext"], rigs4["Twb"][0]
    imgs = _images(fr, ext)
    arr = (M.MantisImage * 4)(*imgs)
    p = mantis.refine_params()
    out, rout = M.MantisResult(), M.MantisRefineResult()
    mantis.prior_pose = None
    st = M.lib().mantis_refine(mantis.h, arr, 4, None, C.byref(p), C.byref(out), C.byref(rout))
    assert st == 5 and b"prior" in M.lib().mantis_last_error(mantis.h)  # MANTIS_ERR_STATE
    # prior = the start moved back by the motion: the refinement starts at prior @ Transform(delta)
    a = math.radians(1.0)
    q = [0.0, 0.0, math.sin(a / 2), math.cos(a / 2)]
    dp = [0.02, -0.01, 0.005]
    delta = _quat_T(q, dp)
    prior = Tt @ np.linalg.inv(delta) @ _quat_T([0, 0, math.sin(0.004), math.cos(0.004)], [0.01, 0, 0])
    mantis.prior_pose = prior
    mantis.rng_state = 4242
    out, rout = mantis.refine(imgs, dp, q, record=1)
    assert mantis.rng_state == 4242 and out.rng_state_after == 4242, "the refinement draws nothing"
    np.testing.assert_allclose(mantis.refine_record(0, 0)[0], prior @ delta, rtol=0, atol=POSE_TOL)
    assert rout.refined == 1 and out.publish == 1 and out.status == 0
    Tw = np.array(rout.T_w_b).reshape(4, 4)
    assert np.array_equal(mantis.prior_pose, Tw)
    assert np.array_equal(np.array(out.covariance), np.array(rout.covariance))
    cov = np.array(out.covariance).reshape(6, 6)
    assert np.array_equal(cov, cov.T) and np.all(np.linalg.eigvalsh(cov) > 0)
    assert out.weight == rout.rms[rout.iterations_run] and out.num_particles == rout.n_obs[rout.iterations_run] > 1000
    np.testing.assert_allclose(np.array(out.position), Tw[:3, 3], atol=0, rtol=0)
    np.testing.assert_allclose(_quat_T(list(out.orientation_xyzw), Tw[:3, 3]), Tw, atol=POSE_TOL, rtol=0)
    d1, a1 = RR.pose_dist(Tw, Tt)
    d0, a0 = RR.pose_dist(prior @ delta, Tt)
    assert d1 < d0 and a1 < a0
    # an unset motion (all zeros) and no motion: the prior itself
    mantis.prior_pose = prior
    mantis.refine(imgs, [0, 0, 0], [0, 0, 0, 0], iterations=1, record=1)
    assert np.array_equal(mantis.refine_record(0, 0)[0], prior)
    # not refined (a gate no rms passes): publish = 0, the prior stays
    mantis.prior_pose = prior
    out, rout = mantis.refine(imgs, max_rms=1e-9)
    assert rout.status == 0 and rout.refined == 0 and out.publish == 0 and np.array_equal(mantis.prior_pose, prior)
    mantis.prior_pose = None


def test_argument_errors(mantis, rigs4, ring8):
    import mantis_amd as M

    L = M.lib()
    ring = _images(ring8["frames"][0], ring8["ext"])
    T0 = np.array([RR.shift(ring8["Twb"][0])] * 3)
    mantis.set_profiling(1)
    mantis.rng_state = 77

    def call(images, rigs, T=T0, **kw):
        n = len(images)
        arr = (M.MantisImage * n)(*images)
        p = mantis.refine_params()
        for k, v in kw.items():
            setattr(p, k, v)
        out = (M.MantisRefineResult * max(rigs, 1))()
        st = L.mantis_refine_batch(mantis.h, arr, rigs, n // max(rigs, 1), T.ctypes.data, C.byref(p), out)
        return st, L.mantis_last_error(mantis.h).decode()

    small = M.make_image(np.zeros((360, 640, 3), np.uint8), *synth.intrinsics(640, 360))
    bad_T = T0.copy()
    bad_T[0, 0, 3] = float("nan")
    bad = [
        (ring + ring[:5], 1, {}, "cams_per_rig"),           # 13 cameras in one rig
        (ring + ring[:7], 3, {}, "max_cams"),               # 3 x 5 = 15 frames on max_cams = 12
        ([ring[0], small], 1, {}, "size"),
        (ring[:2], 0, {}, "n_rigs"),
        (ring[:2], 1, {"struct_size": 8}, "struct_size"),
        (ring[:2], 1, {"iterations": -1}, "iterations"),
        (ring[:2], 1, {"iterations": 11}, "iterations"),
        (ring[:2], 1, {"half_window": 0}, "half_window"),
        (ring[:2], 1, {"half_window": 16}, "half_window"),
        (ring[:2], 1, {"white_thresh": 0}, "white_thresh"),
        (ring[:2], 1, {"white_thresh": 195076}, "white_thresh"),
        (ring[:2], 1, {"min_weight": 0}, "min_weight"),
        (ring[:2], 1, {"min_obs": 5}, "min_obs"),
        (ring[:2], 1, {"lambda_": -1e-9}, "lambda"),
        (ring[:2], 1, {"lambda_": float("nan")}, "lambda"),
        (ring[:2], 1, {"landmark_pitch": 0.0}, "landmark_pitch"),
        (ring[:2], 1, {"landmark_pitch": float("inf")}, "landmark_pitch"),
        (ring[:2], 1, {"max_rms": float("nan")}, "max_rms"),
        (ring[:2], 1, {"record": 2}, "record"),
    ]
    for images, rigs, kw, word in bad:
        st, msg = call(images, rigs, **kw)
        assert st == 1 and word in msg, (kw, st, msg)  # MANTIS_ERR_ARG
    st, msg = call(ring[:2], 1, T=bad_T)
    assert st == 1 and "T_w_b_in" in msg
    f = np.zeros(5, np.uint8)
    assert L.mantis_refine_line_flags(mantis.h, 0.08, f.ctypes.data, 5) == 1
    assert L.mantis_refine_line_flags(mantis.h, -1.0, f.ctypes.data, 5) == 1
    assert "pitch" in L.mantis_last_error(mantis.h).decode()
    assert mantis.rng_state == 77
    # no map: a fresh context
    m2 = M.Mantis(max_cams=1, max_width=W, max_height=H)
    try:
        arr = (M.MantisImage * 1)(ring[0])
        p = m2.refine_params()
        out = M.MantisRefineResult()
        assert L.mantis_refine_batch(m2.h, arr, 1, 1, T0.ctypes.data, C.byref(p), C.byref(out)) == 1
        assert "map" in L.mantis_last_error(m2.h).decode()
    finally:
        m2.close()
    # nothing was launched by the rejected calls: the next call's stage marks are
    # exactly its own 2 (I + 1) launches, and no image stage
    mantis.refine_batch(ring[:2], 1, T0[0], iterations=2)
    names = [n for n, _ in mantis.kernel_times()]
    mantis.set_profiling(0)
    assert sum(n.startswith("refine_obs") for n in names) == 3
    assert sum(n.startswith("refine_step") for n in names) == 3
    assert len(names) == 6, names
    with pytest.raises(Exception):
        mantis.refine_record(0, 0)  # that call kept no record


def test_process_undisturbed_after_refine(mantis, rigs4, landmark_map):
    """A mantis_process call after a refine call still matches the oracle."""
    import _oracle as O
    from test_gpu_parity import _cmp_debug

    import mantis_amd as M

    K, D = synth.intrinsics(W, H)
    mantis.refine_batch(_images(rigs4["frames"][0], rigs4["ext"]), 1, RR.shift(rigs4["Twb"][0]))
    img = rigs4["frames"][1][0]
    mantis.rng_state = 1
    mantis.prior_pose = None
    _, cams = mantis.process([M.make_image(img, K, D)])
    orc = O.Oracle(*landmark_map, seed=1)
    o = orc.process(img, K, D)
    _cmp_debug(mantis.frame_debug(0), o, "after refine")
    assert cams[0].reason == o.reason and cams[0].publish == o.publish
    assert mantis.rng_state == orc.rng_state


def test_refines_on_the_device(mantis, rigs4):
    """The CPU test's scene and condition: closer than the 2 cm / 1 degree start in both, refined = 1."""
    for r in range(3):
        T = rigs4["Twb"][r]
        T0 = RR.shift(T)
        res = mantis.refine_batch(_images(rigs4["frames"][r], rigs4["ext"]), 1, T0)[0]
        Tr = np.array(res.T_w_b).reshape(4, 4)
        d0, a0 = RR.pose_dist(T0, T)
        d1, a1 = RR.pose_dist(Tr, T)
        print(f"rig {r}: {100 * d0:.3f} cm / {a0:.4f} deg -> {100 * d1:.4f} cm / {a1:.4f} deg, n_obs {list(res.n_obs)[:5]}, "
              f"rms x fx {[round(v * 323.15, 3) for v in list(res.rms)[:5]]}")
        assert res.status == 0 and res.refined == 1
        assert d1 < d0 and a1 < a0
