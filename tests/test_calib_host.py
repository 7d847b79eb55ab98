"""Extrinsic calibration on the host (mk_calib.h through hc_calib_*): the
extrinsic's Jacobian against central differences of the observation model, the
end of a pass against numpy's solve of the full (6 N + 6 F) normal system built
from the same accumulators, the covariance against the free block of its
inverse, the gates, and the drifted rig of the issue: three views of the
four-camera 1280 x 720 rig with camera 3 rendered through drift @ ext[3].
"""
import math

import numpy as np
import pytest

import _calib_ref as CR
import _refine_ref as RR
from mantis_amd import synth

FREE = 0b1110


@pytest.fixture(scope="module")
def lm(landmark_map):
    return RR.all_landmarks(landmark_map)


@pytest.fixture(scope="module")
def scene():
    return CR.drifted_scene()


@pytest.fixture(scope="module")
def start_pass(scene, lm):
    """The first pass of the scene on the host: (acc91 [3, 4, 91], cnt [3, 4])."""
    return CR.pass_acc(scene["T0"], scene["ext"], scene["frames"], lm, FREE, RR.default_params())


@pytest.fixture(scope="module")
def calibrated(scene, lm):
    return CR.seq(scene["T0"], scene["ext"], scene["frames"], lm, RR.default_params(), CR.calib_params(FREE))


def test_sizes():
    import ctypes as C

    import mantis_amd as M

    L = CR.hc()
    assert L.hc_sizeof_calib_params() == C.sizeof(M.MantisCalibParams) == 16
    assert L.hc_sizeof_calib_result() == C.sizeof(M.MantisCalibResult)
    a, b = C.c_int32(), C.c_int32()
    M.lib().mantis_calib_sizes(C.byref(a), C.byref(b))
    assert (a.value, b.value) == (C.sizeof(M.MantisCalibParams), C.sizeof(M.MantisCalibResult))
    p = CR.calib_params(0)
    assert (p.struct_size, p.free_cams, p.min_obs_cam) == (16, 0, 60)


def _model_residual(T, E, Xi, nh, m_obs):
    """nh^T (pi(p) - m_obs), p = inverse(E) inverse(T) X: the point-to-line residual with the line's normal held."""
    p = (np.linalg.inv(E) @ np.linalg.inv(T) @ np.append(Xi, 1.0))[:3]
    return float(nh @ (p[:2] / p[2] - m_obs))


def test_jacobians_against_central_differences(scene, lm):
    """J_ext (and J_pose beside it) of every tenth code-0 slot of one camera against central differences of
    the observation model under E <- E D(eps) and T <- T D(delta). Step 1e-6: the truncation error is of the
    order of the step squared (1e-12) and the rounding error 2^-53 / 1e-6 ~ 1e-10, both relative to entries of
    order one; the bound is 1e-7 of the row's largest entry, a thousand times that and a millionth of any
    error in the formula."""
    X, nw, nr, ng = lm
    K, D = synth.intrinsics(RR.W, RR.H_)
    T, E = scene["T0"][0], np.array(scene["ext"][1])
    f = RR.flags(X, 0.08)
    cand = RR.candidates(f)
    codes, Sw, Skw, rows, _ = CR.obs(T, E, K, D, scene["frames"][0][1], X, nw, nr, ng, f, True)
    live = np.flatnonzero(codes == 0)[::10]
    assert len(live) >= 10
    h = 1e-6
    for k in live:
        i = cand[k]
        p, q, m0, nh, Jpi, R_cb = RR.np_geometry(T, E, X[i], 0 if f[i] == 1 else 1)
        m_obs = m0 - rows[k, 12] * nh  # the model's residual at the linearization point is the row's r
        assert abs(_model_residual(T, E, X[i], nh, m_obs) - rows[k, 12]) < 1e-12
        num = np.zeros(12)
        for a in range(6):
            e = np.zeros(6)
            e[a] = h
            num[a] = (_model_residual(RR.exp_right(T, e), E, X[i], nh, m_obs) -
                      _model_residual(RR.exp_right(T, -e), E, X[i], nh, m_obs)) / (2 * h)
            num[6 + a] = (_model_residual(T, RR.exp_right(E, e), X[i], nh, m_obs) -
                          _model_residual(T, RR.exp_right(E, -e), X[i], nh, m_obs)) / (2 * h)
        tol = 1e-7 * np.abs(rows[k, :12]).max()
        np.testing.assert_allclose(rows[k, 6:12], num[6:], rtol=0, atol=tol, err_msg=f"J_ext of candidate {k}")
        np.testing.assert_allclose(rows[k, :6], num[:6], rtol=0, atol=tol, err_msg=f"J_pose of candidate {k}")
        g = nh @ Jpi  # the closed form of include/mantis.h
        px = np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
        np.testing.assert_allclose(rows[k, 6:12], np.concatenate([-g, g @ px]), rtol=1e-12, atol=1e-15)


def test_held_camera_rows(scene, lm):
    """A held camera's J_ext is six zeros, and the other seven entries, the codes and the sums are the
    refinement's own, bit for bit, free or held."""
    X, nw, nr, ng = lm
    K, D = synth.intrinsics(RR.W, RR.H_)
    T, E, img = scene["T0"][1], scene["ext"][2], scene["frames"][1][2]
    f = RR.flags(X, 0.08)
    rc, rSw, rSkw, rrows, rtie = RR.obs(T, E, K, D, img, X, nw, nr, ng, f)
    for free in (False, True):
        codes, Sw, Skw, rows, tie = CR.obs(T, E, K, D, img, X, nw, nr, ng, f, free)
        assert np.array_equal(codes, rc) and np.array_equal(Sw, rSw) and np.array_equal(Skw, rSkw)
        assert np.array_equal(tie, rtie)
        assert np.array_equal(rows[:, :6], rrows[:, :6]) and np.array_equal(rows[:, 12], rrows[:, 6])
        assert not rows[codes != 0].any()
        if free:
            assert np.all(np.abs(rows[codes == 0, 6:12]).max(axis=1) > 0)
        else:
            assert not rows[:, 6:12].any()
    assert (rc == 0).sum() > 100


@pytest.mark.parametrize("free,lam", [(0b1110, 0.0), (0b1000, 0.0), (0b0111, 1e-3)])
def test_end_pass_against_the_full_system(scene, lm, start_pass, free, lam):
    """delta and eps of one step against numpy's solve of the full normal system assembled from the same
    acc91, to 1e-10 of each vector's norm (the issue's bound; cond(S) is in the 10^2 range)."""
    acc, cnt = start_pass
    if free != FREE:  # J_ext columns follow the mask
        acc, cnt = CR.pass_acc(scene["T0"], scene["ext"], scene["frames"], lm, free, RR.default_params())
    p, cp = RR.default_params(lambda_=lam), CR.calib_params(free)
    R = CR.new_result(scene["ext"], free, 3)
    fin, Tn, delta = CR.end_pass(acc, cnt, free, 0, 4, p, cp, scene["T0"], R)
    assert not fin and R.status == 0 and R.iterations_run == 1
    Hm, g = CR.np_normal(acc, free, lam)
    x = np.linalg.solve(Hm, -g)
    fl = CR.free_list(free, 4)
    eps = np.array([list(R.delta_cam[0][c]) for c in fl]).reshape(-1)
    print("cond(H)", np.linalg.cond(Hm), "|delta|", np.linalg.norm(delta), "|eps|", np.linalg.norm(eps))
    assert np.linalg.norm(delta.reshape(-1) - x[:18]) <= 1e-10 * np.linalg.norm(x[:18])
    assert np.linalg.norm(eps - x[18:]) <= 1e-10 * np.linalg.norm(x[18:])
    for c in range(4):
        E0 = np.array(scene["ext"][c])
        En = np.array(list(R.T_base_cam[c])).reshape(4, 4)
        if c in fl:
            np.testing.assert_allclose(En, RR.exp_right(E0, np.array(list(R.delta_cam[0][c]))), rtol=0, atol=1e-14)
        else:
            assert En.tobytes() == np.ascontiguousarray(E0).tobytes() and not any(R.delta_cam[0][c])
    for r in range(3):
        np.testing.assert_allclose(Tn[r], RR.exp_right(scene["T0"][r], delta[r]), rtol=0, atol=1e-14)
    n = int(cnt.sum())
    assert R.n_obs[0] == n and list(R.n_obs_cam[0])[:4] == list(cnt.sum(axis=0))
    assert R.rms[0] == math.sqrt(sum(acc.reshape(-1, 91)[:, 90].tolist()) / n)


def test_covariance_against_the_full_inverse(scene, lm, calibrated):
    """Cov_c against sigma^2 times the diagonal blocks of the free part of numpy's inverse of the full normal
    matrix at the final estimate. Two inversions of matrices that differ in their last bits: cond(H) 2^-53,
    far below the 1e-8 of the largest entry asked here (as the refinement's covariance test)."""
    T_out, R = calibrated
    p, cp = RR.default_params(), CR.calib_params(FREE)
    acc, cnt = CR.pass_acc(list(T_out), list(CR.exts_of(R)), scene["frames"], lm, FREE, p)
    assert int(cnt.sum()) == R.n_obs[R.iterations_run]
    R2 = CR.new_result(CR.exts_of(R), FREE, 3)
    R2.iterations_run = R.iterations_run
    for k in range(11):
        R2.n_obs[k], R2.rms[k] = R.n_obs[k], R.rms[k]
        for c in range(8):
            R2.n_obs_cam[k][c] = R.n_obs_cam[k][c]
    CR.conclude(acc, cnt, FREE, p, cp, R2)
    assert R2.calibrated == 1
    Hm, _ = CR.np_normal(acc, FREE)
    n = int(cnt.sum())
    dof = n - 18 - 18
    rr = acc.reshape(-1, 91)[:, 90].sum()
    inv = np.linalg.inv(Hm)
    for f, c in enumerate([1, 2, 3]):
        ref = rr / dof * inv[18 + 6 * f: 24 + 6 * f, 18 + 6 * f: 24 + 6 * f]
        cov = np.array(list(R2.covariance[c])).reshape(6, 6)
        np.testing.assert_allclose(cov, ref, rtol=0, atol=1e-8 * np.abs(ref).max())
        assert np.array_equal(cov, cov.T) and np.all(np.linalg.eigvalsh(cov) > 0)
        assert np.array_equal(cov, np.array(list(R.covariance[c])).reshape(6, 6)), "hc_calib_seq's own conclusion"
        assert R2.rms_cam[c] == R.rms_cam[c] > 0
    assert not any(R2.covariance[0]) and not any(R2.covariance[4])
    # dof <= 0 and a gate no rms passes: no covariance
    p2 = RR.default_params(max_rms=1e-9)
    CR.conclude(acc, cnt, FREE, p2, cp, R2)
    assert R2.calibrated == 0 and not any(any(R2.covariance[c]) for c in range(8))


def test_zero_iterations_return_the_inputs(scene, lm):
    p, cp = RR.default_params(iterations=0), CR.calib_params(FREE)
    T_out, R = CR.seq(scene["T0"], scene["ext"], scene["frames"], lm, p, cp)
    assert T_out.tobytes() == np.ascontiguousarray(np.array(scene["T0"])).tobytes()
    assert CR.exts_of(R).tobytes() == np.ascontiguousarray(np.array(scene["ext"])).tobytes()
    assert (R.status, R.iterations_run) == (0, 0) and R.n_obs[0] > 1000 and R.rms[0] > 0
    assert (R.n_rigs, R.n_cams, R.free_cams, R.n_cand) == (3, 4, FREE, 540)


def test_starved_gates(scene, lm):
    """One view blacked out: its rows fall below min_obs. One free camera blacked out in every view: its rows
    fall below min_obs_cam while every view keeps three cameras. Either stops pass 0 with the inputs unchanged."""
    p, cp = RR.default_params(), CR.calib_params(FREE)
    black = np.zeros_like(scene["frames"][0][0])
    one_view = [list(fr) for fr in scene["frames"]]
    one_view[1] = [black] * 4
    one_cam = [[black if c == 2 else fr[c] for c in range(4)] for fr in scene["frames"]]
    for name, frames in (("view", one_view), ("camera", one_cam)):
        T_out, R = CR.seq(scene["T0"], scene["ext"], frames, lm, p, cp)
        assert (R.status, R.calibrated, R.iterations_run) == (1, 0, 0), name
        assert T_out.tobytes() == np.ascontiguousarray(np.array(scene["T0"])).tobytes()
        assert CR.exts_of(R).tobytes() == np.ascontiguousarray(np.array(scene["ext"])).tobytes()
        assert not any(any(R.covariance[c]) for c in range(8))
        cams = list(R.n_obs_cam[0])[:4]
        if name == "view":
            assert min(cams) >= cp.min_obs_cam and R.n_obs[0] == sum(cams)
        else:
            assert cams[2] == 0 and min(cams[0], cams[1], cams[3]) > 3 * p.min_obs
    # the held camera blacked out starves nothing: only free cameras have a gate of their own
    held = [[black if c == 0 else fr[c] for c in range(4)] for fr in scene["frames"]]
    T_out, R = CR.seq(scene["T0"], scene["ext"], held, lm, RR.default_params(iterations=1), cp)
    assert R.status != 1 and R.n_obs_cam[0][0] == 0


def test_singular_by_construction():
    """Rows that leave one pose direction unseen make A_r singular; rows whose J_ext has a zero column leave
    A_r positive definite and put an exact zero on S's diagonal. Both stop with SINGULAR and no update."""
    rng = np.random.default_rng(5)
    p, cp = RR.default_params(min_obs=6), CR.calib_params(0b10, min_obs_cam=6)
    exts = [np.eye(4), np.eye(4)]
    T0 = [np.eye(4), np.eye(4)]
    for which in ("A", "S", "none"):
        acc = np.zeros((2, 2, 91))
        cnt = np.full((2, 2), 40, np.int32)
        for r in range(2):
            for c in range(2):
                rows = rng.normal(size=(40, 13))
                if c == 0:
                    rows[:, 6:12] = 0.0  # the held camera
                if which == "A" and r == 1:
                    rows[:, 2] = 0.0
                if which == "S":
                    rows[:, 6 + 3] = 0.0
                acc[r, c] = CR.accumulate(rows)
        R = CR.new_result(exts, 0b10, 2)
        fin, Tn, delta = CR.end_pass(acc, cnt, 0b10, 0, 4, p, cp, T0, R)
        if which == "none":
            assert not fin and R.status == 0 and R.iterations_run == 1 and delta.any()
            continue
        assert fin and R.status == 2 and R.iterations_run == 0, which
        assert np.array_equal(Tn, np.array(T0)) and not delta.any()
        assert np.array_equal(CR.exts_of(R), np.array(exts))
        CR.conclude(acc, cnt, 0b10, p, cp, R)
        assert R.calibrated == 0 and not any(R.covariance[1])


def test_drifted_rig_is_calibrated(scene, lm, calibrated):
    """The issue's scene and both of its accuracy conditions."""
    T_out, R = calibrated
    assert R.iterations_run == 4
    fig = CR.accuracy_checks(T_out, R, lm, scene)
    E = CR.exts_of(R)
    for c in (1, 2):
        d, a = RR.pose_dist(E[c], scene["ext_true"][c])
        print(f"camera {c}: {100 * d:.4f} cm / {a:.4f} deg")
    for r in range(3):
        d0 = RR.pose_dist(scene["T0"][r], scene["Twb"][r])
        d1 = RR.pose_dist(T_out[r], scene["Twb"][r])
        print(f"view {r}: {100 * d0[0]:.3f} cm / {d0[1]:.4f} deg -> {100 * d1[0]:.4f} cm / {d1[1]:.4f} deg")
        assert d1[0] < d0[0] and d1[1] < d0[1]
    d0, a0, d1, a1 = fig["cam3"]
    print(f"camera 3: {100 * d0:.3f} cm / {a0:.4f} deg -> {100 * d1:.4f} cm / {a1:.4f} deg; rms x fx "
          f"{[round(v * 323.15, 3) for v in list(R.rms)[:5]]}; rms_cam x fx {[round(v * 323.15, 3) for v in list(R.rms_cam)[:4]]}")
    print("fresh views (given, calibrated) cm:", [(round(100 * a, 4), round(100 * b, 4)) for a, b in fig["fresh"]])
