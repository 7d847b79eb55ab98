"""Intrinsic calibration on the host (mk_icalib.h through hc_icalib_*): J_int
and J_pose against central differences of the observation model, the rows
beside the refinement's own, the end of a pass against numpy's solve of the
full (6 N + 8 F) normal system built from the same accumulators, the
covariance against the scaled free blocks of its inverse, the gates and exits,
and the scene of the issue: three views of the four-camera 1280 x 720 rig,
every camera rendered through intrinsics 3.8 to 5.8 px rms off the nominal ones.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _icalib_ref as IR
import _refine_ref as RR

ALL = 0b1111


@pytest.fixture(scope="module")
def lm(landmark_map):
    return RR.all_landmarks(landmark_map)


@pytest.fixture(scope="module")
def scene():
    return IR.gap_scene()


@pytest.fixture(scope="module")
def calibrated(scene, lm):
    Ks, Ds = [scene["K"]] * 4, [scene["D"]] * 4
    return IR.seq(scene["T0"], scene["ext"], Ks, Ds, scene["frames"], lm, RR.default_params(), IR.icalib_params(ALL))


def test_sizes():
    import mantis_amd as M

    L = IR.hc()
    assert L.hc_sizeof_icalib_params() == C.sizeof(M.MantisIcalibParams) == 16
    assert L.hc_sizeof_icalib_result() == C.sizeof(M.MantisIcalibResult)
    a, b = C.c_int32(), C.c_int32()
    M.lib().mantis_icalib_sizes(C.byref(a), C.byref(b))
    assert (a.value, b.value) == (C.sizeof(M.MantisIcalibParams), C.sizeof(M.MantisIcalibResult))
    p = IR.icalib_params(0)
    assert (p.struct_size, p.free_cams, p.param_mask, p.min_obs_cam) == (16, 0, 0xFF, 60)


def _undist(kd, P):
    """m with dist_kd(m) = P by Newton on the radius (the fisheye model is radial about (cx, cy))."""
    px, py = (P[0] - kd[2]) / kd[0], (P[1] - kd[3]) / kd[1]
    rd = math.hypot(px, py)
    if rd < 1e-300:
        return np.zeros(2)
    th = rd
    for _ in range(60):
        f = th + kd[4] * th ** 3 + kd[5] * th ** 5 + kd[6] * th ** 7 + kd[7] * th ** 9 - rd
        df = 1 + 3 * kd[4] * th ** 2 + 5 * kd[5] * th ** 4 + 7 * kd[6] * th ** 6 + 9 * kd[7] * th ** 8
        th -= f / df
    return np.array([px, py]) * (math.tan(th) / rd)


def _pose_residual(T, E, Xi, nh, m_obs):
    p = (np.linalg.inv(E) @ np.linalg.inv(T) @ np.append(Xi, 1.0))[:3]
    return float(nh @ (p[:2] / p[2] - m_obs))


def _check_jacobians(T, E, kd, Xi, axis, row, what):
    """The row's J_int against central differences of r(theta) = nh . (m0 - m(theta)), m(theta) the Newton
    solution of dist_theta(m) = P for a fixed pixel P. The rule evaluates J_int at m = m0, so P = dist(m0): the
    line seen where the model puts it. J_pose beside it, as the extrinsic calibration's test. Step 1e-6:
    truncation of the order of the step squared, rounding 2^-53 / 1e-6 ~ 1e-10, both relative to entries of
    order one; the bound is 1e-7 of the row's largest entry."""
    p, q, m0, nh, Jpi, R_cb = RR.np_geometry(T, E, Xi, axis)
    m_obs = m0 - row[14] * nh
    P = IR.np_dist(kd, m0[0], m0[1])
    assert np.abs(_undist(kd, P) - m0).max() < 1e-12
    h = 1e-6
    num = np.zeros(14)
    for a in range(6):
        e = np.zeros(6)
        e[a] = h
        num[a] = (_pose_residual(RR.exp_right(T, e), E, Xi, nh, m_obs) -
                  _pose_residual(RR.exp_right(T, -e), E, Xi, nh, m_obs)) / (2 * h)
    for a in range(8):
        e = np.zeros(8)
        e[a] = h
        rp = float(nh @ (m0 - _undist(IR.np_update(kd, e, 0xFF), P)))
        rm = float(nh @ (m0 - _undist(IR.np_update(kd, -e, 0xFF), P)))
        num[6 + a] = (rp - rm) / (2 * h)
    tol = 1e-7 * np.abs(row[:14]).max()
    np.testing.assert_allclose(row[6:14], num[6:], rtol=0, atol=tol, err_msg=f"J_int of {what}")
    np.testing.assert_allclose(row[:6], num[:6], rtol=0, atol=tol, err_msg=f"J_pose of {what}")


def test_jacobians_against_central_differences(scene, lm):
    """Every tenth code-0 slot of one camera, and of all views and cameras the live slot farthest out towards
    a frame corner: the corner itself lies 734 px from the centre, theta_d = 2.27 rad, behind the camera, so
    the slot of the largest rho stands for it (there G is farthest from the identity)."""
    X, nw, nr, ng = lm
    f = RR.flags(X, 0.08)
    cand = RR.candidates(f)
    axis_of = lambda k: 0 if f[cand[k]] == 1 else 1
    best = None
    for r in range(3):
        for c in range(4):
            T, E, kd = scene["T0"][r], np.array(scene["ext"][c]), scene["kd0"][c]
            codes, Sw, Skw, rows, _ = IR.obs(T, E, kd, scene["frames"][r][c], X, nw, nr, ng, f, True)
            live = np.flatnonzero(codes == 0)
            assert len(live) >= 100
            if (r, c) == (0, 1):
                for k in live[::10]:
                    _check_jacobians(T, E, kd, X[cand[k]], axis_of(k), rows[k], f"candidate {k}")
            for k in live:
                g = RR.np_geometry(T, E, X[cand[k]], axis_of(k))
                u, v = IR.np_dist(kd, g[2][0], g[2][1])
                d = min(math.hypot(u - a, v - b) for a in (0, IR.W) for b in (0, IR.H_))
                if best is None or math.hypot(*g[2]) > best[1]:
                    best = (d, math.hypot(*g[2]), T, E, kd, k, rows[k].copy())
    d, rho, T, E, kd, k, row = best
    print(f"farthest out: rho {rho:.3f}, {d:.1f} px from a corner")
    assert rho > 2.0  # more than 63 degrees off the axis
    _check_jacobians(T, E, kd, X[cand[k]], axis_of(k), row, "the corner candidate")


def test_jacobian_on_the_axis(lm):
    """rho <= 1e-8: a camera straight above a landmark, the image blank but for a line painted through the
    principal point. G = I, c = 1 and the k columns are zero; the K columns against central differences."""
    X, nw, nr, ng = lm
    f = RR.flags(X, 0.08)
    cand = RR.candidates(f)
    k = len(cand) // 2
    i, axis = cand[k], 0 if f[cand[k]] == 1 else 1
    w, h = 320, 240
    kd = np.array([150.0, 151.0, 159.5, 119.25, 0.003, -0.01, 0.005, -0.002])
    T = np.eye(4)
    T[:3, :3] = np.diag([1.0, -1.0, -1.0])
    T[:3, 3] = [X[i][0], X[i][1], X[i][2] + 1.0]
    E = np.eye(4)
    img = np.zeros((h, w, 3), np.uint8)
    # the line's image is the row (axis 0) or the column (axis 1) through (cx, cy): paint it a pixel or two off
    if axis == 0:
        img[int(round(kd[3])) + 1: int(round(kd[3])) + 3, :, :] = 255
    else:
        img[:, int(round(kd[2])) + 1: int(round(kd[2])) + 3, :] = 255
    codes, Sw, Skw, rows, _ = IR.obs(T, E, kd, img, X, nw, nr, ng, f, True)
    assert codes[k] == 0 and rows[k, 14] != 0
    g = RR.np_geometry(T, E, X[i], axis)
    assert math.hypot(*g[2]) <= 1e-8
    nh = g[3]
    np.testing.assert_allclose(rows[k, 6:14], [0, 0, nh[0], nh[1], 0, 0, 0, 0], rtol=0, atol=1e-15)
    assert not rows[k, 10:14].any()
    _check_jacobians(T, E, kd, X[i], axis, rows[k], "the on-axis candidate")


def test_rows_beside_the_refinement(scene, lm):
    """A held camera's J_int is eight zeros, a masked parameter's column is zero in every row, and the other
    seven entries, the codes and the sums are the refinement's own at the same K, D, bit for bit."""
    X, nw, nr, ng = lm
    T, E, img, kd = scene["T0"][1], scene["ext"][2], scene["frames"][1][2], scene["kd0"][2]
    f = RR.flags(X, 0.08)
    rc, rSw, rSkw, rrows, rtie = RR.obs(T, E, scene["K"], scene["D"], img, X, nw, nr, ng, f)
    for free, mask in ((False, 0xFF), (True, 0xFF), (True, 0x3F), (True, 0x0F), (True, 0xF0), (True, 0x01)):
        codes, Sw, Skw, rows, tie = IR.obs(T, E, kd, img, X, nw, nr, ng, f, free, mask)
        assert np.array_equal(codes, rc) and np.array_equal(Sw, rSw) and np.array_equal(Skw, rSkw)
        assert np.array_equal(tie, rtie)
        assert np.array_equal(rows[:, :6], rrows[:, :6]) and np.array_equal(rows[:, 14], rrows[:, 6])
        assert not rows[codes != 0].any()
        for e in range(8):
            col = rows[codes == 0, 6 + e]
            if free and mask >> e & 1:
                assert np.abs(col).max() > 0
            else:
                assert not col.any(), (free, mask, e)
    assert (rc == 0).sum() > 100


def _bound(Hm, x):
    """The forward-error bound of a positive definite solve: 10^3 2^-53 cond_2(H) |x| (the factor covers the
    dimension)."""
    return 1e3 * 2.0 ** -53 * np.linalg.cond(Hm) * np.linalg.norm(x)


@pytest.mark.parametrize("free,mask,lam", [(ALL, 0xFF, 0.0), (ALL, 0xFF, 1e-3), (0b0100, 0xFF, 0.0),
                                           (0b0100, 0xFF, 1e-3), (ALL, 0x3F, 0.0), (ALL, 0x3F, 1e-3),
                                           (ALL, 0x0F, 0.0), (ALL, 0x0F, 1e-3), (ALL, 0xF0, 0.0),
                                           (ALL, 0xF0, 1e-3)])
def test_end_pass_against_the_full_system(scene, lm, free, mask, lam):
    """delta and eps of one step against numpy's solve of the full normal system assembled from the same
    acc120, within the cond-scaled bound; the updates against the rule in numpy."""
    p, ip = RR.default_params(lambda_=lam), IR.icalib_params(free, mask)
    acc, cnt = IR.pass_acc(scene["T0"], scene["ext"], scene["kd0"], scene["frames"], lm, free, mask, p)
    R = IR.new_result(scene["kd0"], free, mask, 3)
    fin, Tn, delta = IR.end_pass(acc, cnt, free, mask, 0, 4, p, ip, scene["T0"], R)
    assert not fin and R.status == 0 and R.iterations_run == 1
    Hm, g = IR.np_normal(acc, free, mask, lam)
    x = np.linalg.solve(Hm, -g)
    fl = IR.free_list(free, 4)
    eps = np.array([list(R.delta_cam[0][c]) for c in fl]).reshape(-1)
    err = np.linalg.norm(np.concatenate([delta.reshape(-1), eps]) - x)
    print("cond(H)", np.linalg.cond(Hm), "|x|", np.linalg.norm(x), "error", err, "bound", _bound(Hm, x))
    assert err <= _bound(Hm, x)
    kds = IR.kds_of(R)
    for c in range(4):
        if c in fl:
            e = np.array(list(R.delta_cam[0][c]))
            assert not e[[k for k in range(8) if not mask >> k & 1]].any()
            want = IR.np_update(scene["kd0"][c], e, mask)
            np.testing.assert_allclose(kds[c], want, rtol=1e-15, atol=0)
            held = [k for k in range(8) if not mask >> k & 1]
            assert kds[c][held].tobytes() == scene["kd0"][c][held].tobytes()
        else:
            assert kds[c].tobytes() == scene["kd0"][c].tobytes() and not any(R.delta_cam[0][c])
    for r in range(3):
        np.testing.assert_allclose(Tn[r], RR.exp_right(scene["T0"][r], delta[r]), rtol=0, atol=1e-14)
    n = int(cnt.sum())
    assert R.n_obs[0] == n and list(R.n_obs_cam[0])[:4] == list(cnt.sum(axis=0))
    assert R.rms[0] == math.sqrt(sum(acc.reshape(-1, IR.ACC)[:, IR.ACC - 1].tolist()) / n)


@pytest.mark.parametrize("mask", [0xFF, 0x3F])
def test_covariance_against_the_full_inverse(scene, lm, mask):
    """Cov_c against sigma^2 times the diagonal blocks of the free part of numpy's inverse of the full normal
    matrix, scaled to natural units, to 1e-8 of the block's largest entry (or the cond-scaled bound of the two
    inversions, if that is larger); zeros in a held parameter's row and column."""
    p, ip = RR.default_params(), IR.icalib_params(ALL, mask)
    acc, cnt = IR.pass_acc(scene["T0"], scene["ext"], scene["kd0"], scene["frames"], lm, ALL, mask, p)
    R = IR.new_result(scene["kd0"], ALL, mask, 3)
    n = int(cnt.sum())
    R.n_obs[0] = n
    for c in range(4):
        R.n_obs_cam[0][c] = int(cnt[:, c].sum())
    rr = sum(acc.reshape(-1, IR.ACC)[:, IR.ACC - 1].tolist())
    R.rms[0] = math.sqrt(rr / n)
    IR.conclude(acc, cnt, ALL, mask, p, ip, R)
    assert R.calibrated == 1
    Hm, _ = IR.np_normal(acc, ALL, mask)
    nfree = bin(mask).count("1")
    dof = n - 18 - 4 * nfree
    inv = np.linalg.inv(Hm)
    cond = np.linalg.cond(Hm)
    for c in range(4):
        kd = scene["kd0"][c]
        sc = np.array([kd[0], kd[1], kd[0], kd[1], 1, 1, 1, 1.0])
        ref = rr / dof * inv[18 + 8 * c: 26 + 8 * c, 18 + 8 * c: 26 + 8 * c] * np.outer(sc, sc)
        for e in range(8):
            if not mask >> e & 1:
                ref[e, :] = 0
                ref[:, e] = 0
        cov = np.array(list(R.covariance[c])).reshape(8, 8)
        # two inversions of matrices that differ in their last bits: relative error cond(H) 2^-53 of the norm
        tol = max(1e-8, 1e3 * 2.0 ** -53 * cond) * np.abs(ref).max()
        np.testing.assert_allclose(cov, ref, rtol=0, atol=tol)
        assert np.array_equal(cov, cov.T)
        fr = [e for e in range(8) if mask >> e & 1]
        assert np.all(np.diag(cov)[fr] > 0)
        assert R.rms_cam[c] > 0
    assert not any(R.covariance[4])
    p2 = RR.default_params(max_rms=1e-9)  # a gate no rms passes: no covariance
    IR.conclude(acc, cnt, ALL, mask, p2, ip, R)
    assert R.calibrated == 0 and not any(any(R.covariance[c]) for c in range(8))
    # one camera held: zeros for it
    R = IR.new_result(scene["kd0"], 0b1011, mask, 3)
    acc2, cnt2 = IR.pass_acc(scene["T0"], scene["ext"], scene["kd0"], scene["frames"], lm, 0b1011, mask, p)
    R.n_obs[0] = n
    for c in range(4):
        R.n_obs_cam[0][c] = int(cnt2[:, c].sum())
    R.rms[0] = math.sqrt(rr / n)
    IR.conclude(acc2, cnt2, 0b1011, mask, p, IR.icalib_params(0b1011, mask), R)
    assert R.calibrated == 1 and not any(R.covariance[2]) and any(R.covariance[3])


def test_zero_iterations_and_masked_parameters(scene, lm):
    """I = 0 returns its inputs bit for bit (K as the float-rounded input); masked parameters and held
    cameras come back bit for bit after four iterations."""
    Ks, Ds = [scene["K"]] * 4, [scene["D"]] * 4
    T_out, R = IR.seq(scene["T0"], scene["ext"], Ks, Ds, scene["frames"], lm, RR.default_params(iterations=0),
                      IR.icalib_params(ALL))
    assert T_out.tobytes() == np.ascontiguousarray(np.array(scene["T0"])).tobytes()
    assert IR.kds_of(R).tobytes() == np.ascontiguousarray(scene["kd0"]).tobytes()
    assert (R.status, R.iterations_run) == (0, 0) and R.n_obs[0] > 1000 and R.rms[0] > 0
    assert (R.n_rigs, R.n_cams, R.free_cams, R.param_mask, R.n_cand) == (3, 4, ALL, 0xFF, 540)
    T_out, R = IR.seq(scene["T0"][:2], scene["ext"], Ks, Ds, scene["frames"][:2], lm, RR.default_params(),
                      IR.icalib_params(0b0110, 0x33))
    assert R.status == 0 and R.iterations_run == 4
    kds = IR.kds_of(R)
    held = [2, 3, 6, 7]
    for c in range(4):
        if c in (1, 2):
            assert kds[c][held].tobytes() == scene["kd0"][c][held].tobytes()
            assert np.all(kds[c][[0, 1, 4, 5]] != scene["kd0"][c][[0, 1, 4, 5]])
        else:
            assert kds[c].tobytes() == scene["kd0"][c].tobytes()
    assert not np.array(R.delta_cam)[:, :, held].any() and not np.array(R.delta_cam)[:, [0, 3]].any()


def test_starved_gates(scene, lm):
    """One view blacked out: its rows fall below min_obs. One free camera blacked out in every view: its rows
    fall below min_obs_cam while every view keeps three cameras. Either stops pass 0 with the inputs unchanged."""
    p, ip = RR.default_params(), IR.icalib_params(ALL)
    Ks, Ds = [scene["K"]] * 4, [scene["D"]] * 4
    black = np.zeros_like(scene["frames"][0][0])
    one_view = [list(fr) for fr in scene["frames"]]
    one_view[1] = [black] * 4
    one_cam = [[black if c == 2 else fr[c] for c in range(4)] for fr in scene["frames"]]
    for name, frames in (("view", one_view), ("camera", one_cam)):
        T_out, R = IR.seq(scene["T0"], scene["ext"], Ks, Ds, frames, lm, p, ip)
        assert (R.status, R.calibrated, R.iterations_run) == (1, 0, 0), name
        assert T_out.tobytes() == np.ascontiguousarray(np.array(scene["T0"])).tobytes()
        assert IR.kds_of(R).tobytes() == np.ascontiguousarray(scene["kd0"]).tobytes()
        assert not any(any(R.covariance[c]) for c in range(8))
        cams = list(R.n_obs_cam[0])[:4]
        if name == "view":
            assert min(cams) >= ip.min_obs_cam and R.n_obs[0] == sum(cams)
        else:
            assert cams[2] == 0 and min(cams[0], cams[1], cams[3]) > 3 * p.min_obs
    # a held camera blacked out starves nothing: only free cameras have a gate of their own
    T_out, R = IR.seq(scene["T0"], scene["ext"], Ks, Ds, one_cam, lm, RR.default_params(iterations=1),
                      IR.icalib_params(0b1011))
    assert R.status != 1 and R.n_obs_cam[0][2] == 0


def _random_acc(rng, N, Cn, free, zero_pose=None, zero_int=None, scale_r=1.0):
    acc = np.zeros((N, Cn, IR.ACC))
    cnt = np.full((N, Cn), 60, np.int32)
    for r in range(N):
        for c in range(Cn):
            rows = rng.normal(size=(60, 15))
            rows[:, 14] *= scale_r
            if not free >> c & 1:
                rows[:, 6:14] = 0.0
            if zero_pose is not None and r == N - 1:
                rows[:, zero_pose] = 0.0
            if zero_int is not None:
                rows[:, 6 + zero_int] = 0.0
            acc[r, c] = IR.accumulate(rows)
    return acc, cnt


def test_singular_and_diverged_by_construction():
    """Rows that leave one pose direction unseen make A_r singular; rows whose J_int has a zero column that
    the mask calls free leave A_r positive definite and put an exact zero on S's diagonal: SINGULAR, no
    update. Residuals a thousand times the Jacobian's size make the step drive fx (1 + eps0) below zero:
    DIVERGED, no update. The same accumulators with that column masked, or small residuals, step."""
    rng = np.random.default_rng(5)
    p, ip = RR.default_params(min_obs=6), IR.icalib_params(0b11, min_obs_cam=8)
    kd0 = np.tile([300.0, 301.0, 320.0, 240.0, 0.003, -0.01, 0.005, -0.002], (2, 1))
    T0 = [np.eye(4), np.eye(4)]
    cases = (("A", {"zero_pose": 2}, 0xFF, 2), ("S", {"zero_int": 3}, 0xFF, 2), ("masked", {"zero_int": 3}, 0xF7, 0),
             ("none", {}, 0xFF, 0), ("diverged", {"scale_r": 1e3}, 0xFF, 3))
    for which, kw, mask, status in cases:
        acc, cnt = _random_acc(rng, 2, 2, 0b11, **kw)
        R = IR.new_result(kd0, 0b11, mask, 2)
        fin, Tn, delta = IR.end_pass(acc, cnt, 0b11, mask, 0, 4, p, ip, T0, R)
        if status == 0:
            assert not fin and R.status == 0 and R.iterations_run == 1 and delta.any(), which
            continue
        assert fin and R.status == status and R.iterations_run == 0, (which, R.status)
        assert np.array_equal(Tn, np.array(T0)) and not delta.any()
        assert IR.kds_of(R).tobytes() == kd0.tobytes() and not np.array(R.delta_cam).any()
        IR.conclude(acc, cnt, 0b11, mask, p, ip, R)
        assert R.calibrated == 0 and not any(R.covariance[1])
    # a NaN accumulator entry in a free camera's II block: no pivot passes, SINGULAR, never a NaN update
    acc, cnt = _random_acc(rng, 2, 2, 0b11)
    acc[0, 1, 119 - 3] = float("nan")  # (13, 13)
    R = IR.new_result(kd0, 0b11, 0xFF, 2)
    fin, Tn, delta = IR.end_pass(acc, cnt, 0b11, 0xFF, 0, 4, p, ip, T0, R)
    assert fin and R.status in (2, 3) and np.array_equal(Tn, np.array(T0)) and IR.kds_of(R).tobytes() == kd0.tobytes()


def test_gap_scene_is_calibrated(scene, lm, calibrated):
    """The issue's scene and its accuracy conditions."""
    T_out, R = calibrated
    assert R.iterations_run == 4
    fig = IR.accuracy_checks(T_out, R, lm, scene)
    print("rms x fx per pass:", [round(v * 323.15, 3) for v in list(R.rms)[:5]], "n_obs", list(R.n_obs)[:5])
    print("rms_cam x fx:", [round(v * 323.15, 3) for v in list(R.rms_cam)[:4]])
    print("sigma of fx, fy, cx, cy (px):", [[round(math.sqrt(R.covariance[c][9 * e]), 4) for e in range(4)]
                                            for c in range(4)])
    assert all(0 < R.covariance[c][0] < 4.0 for c in range(4))
