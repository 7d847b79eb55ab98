"""Extrinsic calibration on the GPU (mantis_calibrate_extrinsics): every
recorded pass against the host build of the same rules (mk_calib.h through
hc_calib_obs, fed the device's own recorded poses and extrinsics so that a
flipped tie cannot cascade), the MFMA accumulators against numpy sums of the
recorded rows, each step against hc_calib_end_pass on the device's own
accumulators, the whole call against hc_calib_seq, the shapes that break
loops, equal bytes, the two accuracy conditions of the CPU suite, what the
call must leave untouched and the argument errors. Synthetic rigs of
tests/_refine_ref.py; at most five views.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _calib_ref as CR
import _refine_ref as RR
import _refine_robust_ref as RB
from mantis_amd import synth

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-9
STEP_TOL = 1e-12
W, H = RR.W, RR.H_
FREE = 0b1110


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
def scene():
    return CR.drifted_scene()


@pytest.fixture(scope="module")
def ring8():
    return RR.rig_scene(8, 1)


@pytest.fixture(scope="module")
def pairs5():
    """Five views of a two-camera rig on 640 x 360 frames."""
    return RR.rig_scene(2, 5, seed=11, w=640, h=360)


def _images(frames, exts, Ks=None, Ds=None):
    """frames[r][c] -> view-major mantis_images, every view with the rig's extrinsics."""
    import mantis_amd as M

    h, w = frames[0][0].shape[:2]
    Ks, Ds = RR.lenses(len(exts), w, h, Ks, Ds)
    return [M.make_image(f, Ks[c], Ds[c], T_base_cam=exts[c]) for fr in frames for c, f in enumerate(fr)]


def _check_call(m, lm, frames, exts, T0s, free, landmarks=None, min_obs_cam=None, Ks=None, Ds=None, whole_call=True,
                **params):
    """One call with record = 1: every pass against the host rules; returns (T_out, result). Ks, Ds: per-camera
    lenses (default: the bench lens); whole_call = False leaves out the comparison with hc_calib_seq (a cell
    whose iteration the host alone does not reproduce under a 1e-13 change of D, tests/_line_cases.py)."""
    X, nw, nr, ng = landmarks or lm
    N, Cn = len(frames), len(exts)
    h, w = frames[0][0].shape[:2]
    Ks, Ds = RR.lenses(Cn, w, h, Ks, Ds)
    T_out, res = m.calibrate_extrinsics(_images(frames, exts, Ks, Ds), N, np.array(T0s), free,
                                        min_obs_cam=min_obs_cam, record=1, **params)
    p = m.refine_params(**params)
    cp = m.calib_params(free, **({} if min_obs_cam is None else {"min_obs_cam": min_obs_cam}))
    f = RR.flags(X, p.landmark_pitch)
    nc = len(RR.candidates(f))
    assert (res.n_cand, res.n_rigs, res.n_cams, res.free_cams) == (nc, N, Cn, free)
    flagged = total = 0
    Ts, Es, accs, cnts = [], [], [], []
    for k in range(res.iterations_run + 1):
        Tk, acck, cntk = [], np.zeros((N, Cn, 91)), np.zeros((N, Cn), np.int32)
        for r in range(N):
            T, E, codes, Sw, Skw, rows, acc = m.calib_record(r, k)
            Tk.append(T)
            if r == 0:
                Es.append(E)
            assert np.array_equal(E, Es[k]), "one set of extrinsics per pass"
            assert codes.shape == (Cn * nc,)
            for c in range(Cn):
                hc_, hSw, hSkw, hrows, tie = CR.obs(T, E[c], Ks[c], Ds[c], frames[r][c], X, nw, nr, ng, f,
                                                    free >> c & 1, R=p.half_window, white_thresh=p.white_thresh,
                                                    min_weight=p.min_weight)
                sl = slice(c * nc, (c + 1) * nc)
                ok = tie == 0
                flagged += int((~ok).sum())
                total += nc
                where = f"pass {k} view {r} camera {c}"
                assert np.array_equal(codes[sl][ok], hc_[ok]), where
                assert np.array_equal(Sw[sl][ok], hSw[ok]) and np.array_equal(Skw[sl][ok], hSkw[ok]), where
                np.testing.assert_allclose(rows[sl][ok], hrows[ok], rtol=1e-12, atol=0, err_msg=where)
                if not free >> c & 1:
                    assert not rows[sl][:, 6:12].any(), where
                # both are float64 sums of the same n products, each within n 2^-53 sum |terms| of the exact
                # value (CR.np_acc91's bound): twice that beside the 1e-12 of the value, or an entry whose
                # terms cancel could not be compared at all
                ref, err = CR.np_acc91(rows[sl])
                assert np.all(np.abs(acc[c] - ref) <= 1e-12 * np.abs(ref) + 2 * err), where
                cntk[r, c] = int((codes[sl] == 0).sum())
            assert np.all(rows[codes != 0] == 0.0)
            acck[r] = acc
        Ts.append(np.array(Tk))
        accs.append(acck)
        cnts.append(cntk)
        n_obs = int(cntk.sum())
        assert res.n_obs[k] == n_obs and list(res.n_obs_cam[k])[:Cn] == list(cntk.sum(axis=0))
        rr = sum(acck.reshape(-1, 91)[:, 90].tolist())  # (view, camera) order
        assert res.rms[k] == (math.sqrt(rr / n_obs) if n_obs else 0.0)
    assert flagged <= 0.005 * total, (flagged, total)
    assert np.array_equal(Ts[0], np.array(T0s)) and np.array_equal(Es[0], np.array(exts)), "pass 0 observes the inputs"
    for k in range(res.iterations_run):
        R = CR.new_result(Es[k], free, N)
        fin, Tn, _ = CR.end_pass(accs[k], cnts[k], free, k, p.iterations, p, cp, Ts[k], R)
        assert not fin
        np.testing.assert_allclose(Ts[k + 1], Tn, rtol=0, atol=STEP_TOL, err_msg=f"step {k}: poses")
        np.testing.assert_allclose(Es[k + 1], CR.exts_of(R), rtol=0, atol=STEP_TOL, err_msg=f"step {k}: extrinsics")
        np.testing.assert_allclose(np.array(res.delta_cam[k]), np.array(R.delta_cam[k]), rtol=0, atol=STEP_TOL)
    assert np.array_equal(T_out, Ts[-1]) and np.array_equal(CR.exts_of(res), Es[-1])
    for c in range(Cn):
        if not free >> c & 1:
            assert CR.exts_of(res)[c].tobytes() == np.ascontiguousarray(exts[c], np.float64).tobytes()
    if flagged == 0 and whole_call:
        hT, host = CR.seq(T0s, exts, frames, (X, nw, nr, ng), p, cp, Ks, Ds)
        np.testing.assert_allclose(T_out, hT, rtol=0, atol=POSE_TOL)
        np.testing.assert_allclose(CR.exts_of(res), CR.exts_of(host), rtol=0, atol=POSE_TOL)
        assert list(res.n_obs) == list(host.n_obs)
        assert np.array_equal(np.array(res.n_obs_cam), np.array(host.n_obs_cam))
        assert (res.iterations_run, res.calibrated, res.status) == (host.iterations_run, host.calibrated, host.status)
        if res.calibrated:
            hcov = np.array(host.covariance)
            np.testing.assert_allclose(np.array(res.covariance), hcov, rtol=0, atol=1e-8 * np.abs(hcov).max())
            np.testing.assert_allclose(np.array(res.rms_cam), np.array(host.rms_cam), rtol=1e-9, atol=0)
    return T_out, res


@pytest.mark.parametrize("shape", ["N=3", "N=1", "free=0b1000", "free=0b0111", "I=0", "I=10", "R=1", "R=15"])
def test_record_parity(mantis, lm, scene, shape):
    N = 1 if shape == "N=1" else 3
    free = {"free=0b1000": 0b1000, "free=0b0111": 0b0111}.get(shape, FREE)
    params = {"I=0": {"iterations": 0}, "I=10": {"iterations": 10}, "R=1": {"half_window": 1},
              "R=15": {"half_window": 15}}.get(shape, {})
    T_out, res = _check_call(mantis, lm, scene["frames"][:N], scene["ext"], scene["T0"][:N], free, **params)
    E = CR.exts_of(res)
    print(shape, res.status, res.calibrated, res.iterations_run, list(res.n_obs),
          [RR.pose_dist(E[c], scene["ext_true"][c]) for c in range(4)])
    if shape == "I=0":
        assert np.array_equal(T_out, np.array(scene["T0"])) and np.array_equal(E, np.array(scene["ext"]))
        assert res.iterations_run == 0 and res.status == 0
    elif shape == "R=1":
        assert res.status in (0, 1, 2)  # a three-sample window holds few lines 2 cm away: whatever the rule says
    else:
        assert res.status == 0 and res.calibrated == 1 and res.iterations_run == (10 if shape == "I=10" else 4)


def test_five_views_of_two_cameras(mantis, lm, pairs5):
    T0 = [RR.shift(T) for T in pairs5["Twb"]]
    T_out, res = _check_call(mantis, lm, pairs5["frames"], pairs5["ext"], T0, 0b10)
    assert res.status == 0 and res.iterations_run == 4


def test_eight_cameras_seven_free(mantis, lm, ring8):
    T_out, res = _check_call(mantis, lm, ring8["frames"], ring8["ext"], [RR.shift(ring8["Twb"][0])], 0b11111110)
    assert res.status == 0 and res.calibrated == 1 and res.iterations_run == 4
    assert not any(res.covariance[0]) and all(any(res.covariance[c]) for c in range(1, 8))


def test_odd_candidate_count(mantis, lm, scene, landmark_map):
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
        landmarks = (np.ascontiguousarray(X), len(w) - drop, len(r), len(g))
        T_out, res = _check_call(mantis, lm, [fr[1:] for fr in scene["frames"][:2]], scene["ext"][1:],
                                 scene["T0"][:2], 0b110, landmarks=landmarks)
        assert res.n_cand == nc and res.status == 0
    finally:
        mantis.set_map(w, r, g)


def test_small_pitched_frame(mantis, lm):
    """322 x 242 (neither a multiple of 4) with step_bytes = 1000 > 3 W: staged through the pitch conversion."""
    import mantis_amd as M

    w, h = 322, 242
    sc = RR.rig_scene(2, 2, seed=7, w=w, h=h)
    T0 = [RR.shift(T) for T in sc["Twb"]]
    T_out, res = _check_call(mantis, lm, sc["frames"], sc["ext"], T0, 0b10)
    K, D = synth.intrinsics(w, h)
    imgs, keep = [], []
    for fr in sc["frames"]:
        for f, e in zip(fr, sc["ext"]):
            buf = np.full((h, 3 * w + 34), 0xAB, np.uint8)  # rows 1000 bytes apart
            buf[:, : 3 * w] = f.reshape(h, 3 * w)
            keep.append(buf)
            im = M.make_image(f, K, D, T_base_cam=e)
            im.bgr = buf.ctypes.data
            im.step_bytes = buf.strides[0]
            imgs.append(im)
    assert imgs[0].step_bytes == 1000 > 3 * w
    T2, pitched = mantis.calibrate_extrinsics(imgs, 2, np.array(T0), 0b10)
    assert bytes(pitched) == bytes(res) and T2.tobytes() == T_out.tobytes()


def test_equal_bytes(mantis, scene):
    """Host frames against device frames, and the same call twice."""
    import mantis_amd as M

    K, D = synth.intrinsics(W, H)
    fr, ext, T0 = scene["frames"], scene["ext"], np.array(scene["T0"])
    Th, host = mantis.calibrate_extrinsics(_images(fr, ext), 3, T0, FREE)
    Ta, again = mantis.calibrate_extrinsics(_images(fr, ext), 3, T0, FREE)
    assert bytes(host) == bytes(again) and Th.tobytes() == Ta.tobytes() and host.calibrated == 1
    fb = W * H * 3
    dev = mantis.device_alloc(fb * 12)
    try:
        imgs = []
        for r in range(3):
            for c in range(4):
                i = 4 * r + c
                mantis.h2d(dev + i * fb, fr[r][c])
                imgs.append(M.make_image(None, K, D, T_base_cam=ext[c], device_ptr=dev + i * fb, width=W, height=H))
        Td, devr = mantis.calibrate_extrinsics(imgs, 3, T0, FREE)
    finally:
        mantis.device_free(dev)
    assert bytes(host) == bytes(devr) and Th.tobytes() == Td.tobytes()


def test_calibrates_on_the_device(mantis, lm, scene):
    """The two accuracy conditions of the CPU suite on the device's result."""
    T_out, res = mantis.calibrate_extrinsics(_images(scene["frames"], scene["ext"]), 3, np.array(scene["T0"]), FREE)
    fig = CR.accuracy_checks(T_out, res, lm, scene)
    d0, a0, d1, a1 = fig["cam3"]
    print(f"camera 3: {100 * d0:.3f} cm / {a0:.4f} deg -> {100 * d1:.4f} cm / {a1:.4f} deg; rms_cam x fx "
          f"{[round(v * 323.15, 3) for v in list(res.rms_cam)[:4]]}")
    print("fresh views (given, calibrated) cm:", [(round(100 * a, 4), round(100 * b, 4)) for a, b in fig["fresh"]])
    for r in range(3):
        assert RR.pose_dist(T_out[r], scene["Twb"][r])[0] < RR.pose_dist(scene["T0"][r], scene["Twb"][r])[0]


def test_context_untouched(mantis, scene):
    """rng_state, the prior and the robust setting are neither read nor changed: a mantis_refine_batch and a
    mantis_process after a calibration return the bytes they return before one, the caller's images keep
    their bytes, and the robust switch changes nothing in the calibration."""
    import mantis_amd as M

    K, D = synth.intrinsics(W, H)
    sc = RB.rigs4()
    rimgs = _images([sc["frames"][0]], sc["ext"])
    T0 = RR.shift(sc["Twb"][0])
    prior = sc["Twb"][1]

    def before_after():
        mantis.rng_state = 1
        mantis.prior_pose = None
        rig, cams = mantis.process_motion([M.make_image(sc["frames"][1][0], K, D)])  # mantis_process
        ref = mantis.refine_batch(rimgs, 1, T0)[0]
        return bytes(rig), bytes(cams[0]), bytes(ref), mantis.rng_state

    a = before_after()
    mantis.rng_state = 4242
    mantis.prior_pose = prior
    cimgs = _images(scene["frames"], scene["ext"])
    snap = [bytes(i) for i in cimgs]
    Tc, res = mantis.calibrate_extrinsics(cimgs, 3, np.array(scene["T0"]), FREE)
    assert mantis.rng_state == 4242 and np.array_equal(mantis.prior_pose, prior)
    assert [bytes(i) for i in cimgs] == snap
    mantis.set_refine_robust("tukey")
    try:
        Tr, rob = mantis.calibrate_extrinsics(cimgs, 3, np.array(scene["T0"]), FREE)
    finally:
        mantis.set_refine_robust(None)
    assert bytes(rob) == bytes(res) and Tr.tobytes() == Tc.tobytes()
    assert mantis.rng_state == 4242 and np.array_equal(mantis.prior_pose, prior)
    assert before_after() == a
    mantis.prior_pose = None


def test_starved_and_records(mantis, lm, scene):
    """A blacked-out free camera starves pass 0: the inputs come back, later passes have no record."""
    black = np.zeros_like(scene["frames"][0][0])
    frames = [[black if c == 2 else fr[c] for c in range(4)] for fr in scene["frames"][:2]]
    T_out, res = _check_call(mantis, lm, frames, scene["ext"], scene["T0"][:2], FREE)
    assert (res.status, res.calibrated, res.iterations_run) == (1, 0, 0) and res.n_obs_cam[0][2] == 0
    assert np.array_equal(T_out, np.array(scene["T0"][:2])) and not np.array(res.covariance).any()
    with pytest.raises(Exception):
        mantis.calib_record(0, 1)  # the pass did not run
    with pytest.raises(Exception):
        mantis.calib_record(2, 0)  # no such view
    mantis.calibrate_extrinsics(_images(frames, scene["ext"]), 2, np.array(scene["T0"][:2]), FREE)
    with pytest.raises(Exception):
        mantis.calib_record(0, 0)  # that call kept no record


def test_argument_errors(mantis, scene, ring8):
    import mantis_amd as M

    L = M.lib()
    ring = _images(ring8["frames"], ring8["ext"])
    quad = _images(scene["frames"], scene["ext"])
    T0 = np.array([RR.shift(ring8["Twb"][0])] * 6)
    mantis.set_profiling(1)
    mantis.rng_state = 77

    def call(images, views, T=T0, free=0b10, cp_kw=None, null=None, **kw):
        n = len(images)
        arr = (M.MantisImage * n)(*images)
        p = mantis.refine_params()
        for k, v in kw.items():
            setattr(p, k, v)
        cp = mantis.calib_params(free)
        for k, v in (cp_kw or {}).items():
            setattr(cp, k, v)
        out = M.MantisCalibResult()
        T_out = np.zeros((max(views, 1), 16))
        args = {"cams": arr, "T": T.ctypes.data, "p": C.byref(p), "cp": C.byref(cp), "T_out": T_out.ctypes.data,
                "out": C.byref(out)}
        if null:
            args[null] = None
        st = L.mantis_calibrate_extrinsics(mantis.h, args["cams"], views, n // max(views, 1), args["T"], args["p"],
                                           args["cp"], args["T_out"], args["out"])
        return st, L.mantis_last_error(mantis.h).decode()

    small = M.make_image(np.zeros((360, 640, 3), np.uint8), *synth.intrinsics(640, 360))
    bad_T = T0.copy()
    bad_T[0, 0, 3] = float("nan")
    other = _images(scene["frames"][:2], scene["ext"])
    other[5].T_base_cam[3] += 1e-12  # view 1's camera 1 differs from view 0's in one byte or so
    nan_ext = _images(scene["frames"][:1], scene["ext"])
    nan_ext[2].T_base_cam[7] = float("inf")
    bad = [
        (ring + ring[:5], 1, {}, "cams_per_rig"),                      # 13 cameras in one rig
        (ring + ring[:7], 3, {}, "max_cams"),                          # 3 x 5 = 15 frames on max_cams = 12
        ([ring[0], small], 1, {}, "size"),
        (ring[:2], 0, {}, "n_rigs"),
        (ring[:1], 1, {"free": 0b1}, "cams_per_rig"),                  # one camera: nothing to hold
        (ring[:2], 1, {"free": 0}, "free_cams"),
        (ring[:2], 1, {"free": 0b11}, "free_cams"),                    # no camera held
        (ring[:2], 1, {"free": 0b110}, "free_cams"),                   # a bit above cams_per_rig
        (ring[:2], 1, {"free": -2}, "free_cams"),
        (ring[:2], 1, {"cp_kw": {"min_obs_cam": 5}}, "min_obs_cam"),
        (ring[:2], 1, {"cp_kw": {"struct_size": 8}}, "calib_params.struct_size"),
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
        (ring[:2], 1, {"T": bad_T}, "T_w_b_in"),
        (other, 2, {}, "T_base_cam of a view"),
        (nan_ext, 1, {}, "T_base_cam is not finite"),
    ] + [(ring[:2], 1, {"null": k}, "null") for k in ("cams", "T", "p", "cp", "T_out", "out")]
    for images, views, kw, word in bad:
        st, msg = call(images, views, **kw)
        assert st == 1 and word in msg, (kw, st, msg)  # MANTIS_ERR_ARG
    assert mantis.rng_state == 77
    # 257 views: turned away by its own limit before the frames are counted against max_cams
    st, msg = call(ring[:2] * 257, 257, T=np.tile(T0[:1], (257, 1, 1)))
    assert st == 1 and "n_rigs exceeds 256" in msg, msg
    # no map: a fresh context
    m2 = M.Mantis(max_cams=2, max_width=W, max_height=H)
    try:
        arr = (M.MantisImage * 2)(*ring[:2])
        p, cp = m2.refine_params(), m2.calib_params(0b10)
        out, T_out = M.MantisCalibResult(), np.zeros(16)
        st = L.mantis_calibrate_extrinsics(m2.h, arr, 1, 2, T0.ctypes.data, C.byref(p), C.byref(cp),
                                           T_out.ctypes.data, C.byref(out))
        assert st == 1 and "map" in L.mantis_last_error(m2.h).decode()
    finally:
        m2.close()
    with pytest.raises(Exception):
        mantis.calib_record(0, 0)  # MANTIS_ERR_STATE: nothing recorded on this context since set_profiling
    # nothing was launched by the rejected calls: the next call's stage marks are
    # exactly its own 3 (I + 1) launches, and no image stage
    mantis.calibrate_extrinsics(quad[:4], 1, T0[0], FREE, iterations=2)
    names = [n for n, _ in mantis.kernel_times()]
    mantis.set_profiling(0)
    for stage in ("calib_obs", "calib_rig", "calib_solve"):
        assert sum(n.startswith(stage) for n in names) == 3, names
    assert len(names) == 9, names
