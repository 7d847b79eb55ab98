"""Rig calibration on the host (mk_rcalib.h through hc_rcalib_*): the 20
Jacobian columns against central differences of the observation model, the
rows beside the two single calibrations' own, the end of a pass against
numpy's solve of the full (6 N + 6 Fe + 8 Fi) normal system built from the
same accumulators, the covariances against the scaled blocks of its inverse,
the gates and exits, and the scene of the issue: three views of the
four-camera 1280 x 720 rig, every camera rendered through intrinsics 3.8 to
5.8 px rms off the nominal ones and cameras 1-3 through extrinsics 1.2 cm /
0.69 degrees off, on which alternating the two single calibrations fails.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _calib_ref as CR
import _icalib_ref as IR
import _rcalib_ref as QR
import _refine_ref as RR

EXT, INT = 0b1110, 0b1111


@pytest.fixture(scope="module")
def lm(landmark_map):
    return RR.all_landmarks(landmark_map)


@pytest.fixture(scope="module")
def scene():
    return QR.joint_scene()


@pytest.fixture(scope="module")
def calibrated(scene, lm):
    Ks, Ds = [scene["K"]] * 4, [scene["D"]] * 4
    return QR.seq(scene["T0"], scene["ext"], Ks, Ds, scene["frames"], lm, RR.default_params(),
                  QR.rcalib_params(EXT, INT))


_ACC = {}


def _pass_acc(scene, lm, fe, fi, mask):
    """The scene's first pass at the start, shared by the cases that differ in lambda only (never written)."""
    key = (fe, fi, mask)
    if key not in _ACC:
        _ACC[key] = QR.pass_acc(scene["T0"], scene["ext"], scene["kd0"], scene["frames"], lm, fe, fi, mask,
                                RR.default_params())
    return _ACC[key]


def test_sizes():
    import mantis_amd as M

    L = QR.hc()
    assert L.hc_sizeof_rcalib_params() == C.sizeof(M.MantisRcalibParams) == 24
    assert L.hc_sizeof_rcalib_result() == C.sizeof(M.MantisRcalibResult)
    a, b = C.c_int32(), C.c_int32()
    M.lib().mantis_rcalib_sizes(C.byref(a), C.byref(b))
    assert (a.value, b.value) == (C.sizeof(M.MantisRcalibParams), C.sizeof(M.MantisRcalibResult))
    p = QR.rcalib_params(0, 0)
    assert (p.struct_size, p.free_ext, p.free_int, p.param_mask, p.min_obs_cam) == (24, 0, 0, 0xFF, 60)


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


def _residual(T, E, Xi, nh, m_obs):
    """nh^T (pi(p) - m_obs), p = inverse(E) inverse(T) X: the point-to-line residual with the line's normal held."""
    p = (np.linalg.inv(E) @ np.linalg.inv(T) @ np.append(Xi, 1.0))[:3]
    return float(nh @ (p[:2] / p[2] - m_obs))


def _check_jacobians(T, E, kd, Xi, axis, row, what):
    """The row's 20 Jacobian columns against central differences. J_pose and J_ext: of the point-to-line
    residual under T <- T D(delta) and E <- E D(eps), the normal held. J_int: of r(theta) = nh . (m0 - m(theta)),
    m(theta) the Newton solution of dist_theta(m) = P for the fixed pixel P = dist(m0). Step 1e-6: truncation of
    the order of the step squared, rounding 2^-53 / 1e-6 ~ 1e-10, both relative to entries of order one; the bound
    is 1e-7 of the row's largest entry."""
    p, q, m0, nh, Jpi, R_cb = RR.np_geometry(T, E, Xi, axis)
    m_obs = m0 - row[20] * nh
    P = IR.np_dist(kd, m0[0], m0[1])
    assert np.abs(_undist(kd, P) - m0).max() < 1e-12
    h = 1e-6
    num = np.zeros(20)
    for a in range(6):
        e = np.zeros(6)
        e[a] = h
        num[a] = (_residual(RR.exp_right(T, e), E, Xi, nh, m_obs) -
                  _residual(RR.exp_right(T, -e), E, Xi, nh, m_obs)) / (2 * h)
        num[6 + a] = (_residual(T, RR.exp_right(E, e), Xi, nh, m_obs) -
                      _residual(T, RR.exp_right(E, -e), Xi, nh, m_obs)) / (2 * h)
    for a in range(8):
        e = np.zeros(8)
        e[a] = h
        rp = float(nh @ (m0 - _undist(IR.np_update(kd, e, 0xFF), P)))
        rm = float(nh @ (m0 - _undist(IR.np_update(kd, -e, 0xFF), P)))
        num[12 + a] = (rp - rm) / (2 * h)
    tol = 1e-7 * np.abs(row[:20]).max()
    for name, sl in (("J_pose", slice(0, 6)), ("J_ext", slice(6, 12)), ("J_int", slice(12, 20))):
        np.testing.assert_allclose(row[sl], num[sl], rtol=0, atol=tol, err_msg=f"{name} of {what}")


def _off_nominal(scene, c):
    """Extrinsics and intrinsics of camera c that both differ from the nominal ones: halfway to the truth."""
    E = RR.exp_right(scene["ext"][c], [0.004, -0.003, 0.002, 0.003, -0.002, 0.004])
    kd = 0.5 * (scene["kd0"][c] + scene["kd_true"][c])
    return E, kd


def test_jacobians_against_central_differences(scene, lm):
    """Every tenth code-0 slot of one camera, and of all views and cameras the live slot of largest rho (where
    G is farthest from the identity), at intrinsics and extrinsics that both differ from nominal."""
    X, nw, nr, ng = lm
    f = RR.flags(X, 0.08)
    cand = RR.candidates(f)
    axis_of = lambda k: 0 if f[cand[k]] == 1 else 1
    best = None
    for r in range(3):
        for c in range(4):
            T = scene["T0"][r]
            E, kd = _off_nominal(scene, c)
            codes, Sw, Skw, rows, _ = QR.obs(T, E, kd, scene["frames"][r][c], X, nw, nr, ng, f, True, True)
            live = np.flatnonzero(codes == 0)
            assert len(live) >= 100
            if (r, c) == (0, 1):
                assert np.abs(kd - scene["kd0"][c]).max() > 0.5 and not np.array_equal(E, scene["ext"][c])
                for k in live[::10]:
                    _check_jacobians(T, E, kd, X[cand[k]], axis_of(k), rows[k], f"candidate {k}")
            for k in live:
                g = RR.np_geometry(T, E, X[cand[k]], axis_of(k))
                if best is None or math.hypot(*g[2]) > best[0]:
                    best = (math.hypot(*g[2]), T, E, kd, k, rows[k].copy())
    rho, T, E, kd, k, row = best
    print(f"largest rho {rho:.3f}")
    assert rho > 2.0  # more than 63 degrees off the axis
    _check_jacobians(T, E, kd, X[cand[k]], axis_of(k), row, "the candidate of largest rho")


def test_jacobian_on_the_axis(lm):
    """rho <= 1e-8: a camera straight above a landmark, the image blank but for a line painted through the
    principal point. G = I, c = 1 and the k columns are zero; the other columns against central differences."""
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
    if axis == 0:
        img[int(round(kd[3])) + 1: int(round(kd[3])) + 3, :, :] = 255
    else:
        img[:, int(round(kd[2])) + 1: int(round(kd[2])) + 3, :] = 255
    codes, Sw, Skw, rows, _ = QR.obs(T, E, kd, img, X, nw, nr, ng, f, True, True)
    assert codes[k] == 0 and rows[k, 20] != 0
    g = RR.np_geometry(T, E, X[i], axis)
    assert math.hypot(*g[2]) <= 1e-8
    nh = g[3]
    np.testing.assert_allclose(rows[k, 12:20], [0, 0, nh[0], nh[1], 0, 0, 0, 0], rtol=0, atol=1e-15)
    assert not rows[k, 16:20].any() and rows[k, 6:12].any()
    _check_jacobians(T, E, kd, X[i], axis, rows[k], "the on-axis candidate")


def test_rows_beside_the_single_calibrations(scene, lm):
    """With free_int's bit clear and a float-representable K, columns 0-11 and 20, the codes and the sums are
    hc_calib_obs' bit for bit; with free_ext's bit clear, columns 0-5 and 12-20 are hc_icalib_obs' (at FP64
    intrinsics no float holds). Held blocks are zero; with both free each block is its own rule's."""
    X, nw, nr, ng = lm
    T, img = scene["T0"][1], scene["frames"][1][2]
    f = RR.flags(X, 0.08)
    E, kd = _off_nominal(scene, 2)
    kd0 = scene["kd0"][2]
    for fe in (False, True):
        cc, cSw, cSkw, crows, ctie = CR.obs(T, E, scene["K"], scene["D"], img, X, nw, nr, ng, f, fe)
        codes, Sw, Skw, rows, tie = QR.obs(T, E, kd0, img, X, nw, nr, ng, f, fe, False)
        assert np.array_equal(codes, cc) and np.array_equal(Sw, cSw) and np.array_equal(Skw, cSkw)
        assert np.array_equal(tie, ctie)
        assert rows[:, :12].tobytes() == np.ascontiguousarray(crows[:, :12]).tobytes()
        assert rows[:, 20].tobytes() == np.ascontiguousarray(crows[:, 12]).tobytes()
        assert not rows[:, 12:20].any() and not rows[codes != 0].any()
        assert rows[codes == 0, 6:12].any() == fe
        assert (cc == 0).sum() > 100
    for fi, mask in ((False, 0xFF), (True, 0xFF), (True, 0x0F), (True, 0xF0), (True, 0x01)):
        ic, iSw, iSkw, irows, itie = IR.obs(T, E, kd, img, X, nw, nr, ng, f, fi, mask)
        codes, Sw, Skw, rows, tie = QR.obs(T, E, kd, img, X, nw, nr, ng, f, False, fi, mask)
        assert np.array_equal(codes, ic) and np.array_equal(Sw, iSw) and np.array_equal(Skw, iSkw)
        assert np.array_equal(tie, itie)
        assert rows[:, :6].tobytes() == np.ascontiguousarray(irows[:, :6]).tobytes()
        assert rows[:, 12:21].tobytes() == np.ascontiguousarray(irows[:, 6:15]).tobytes()
        assert not rows[:, 6:12].any() and not rows[codes != 0].any()
        for e in range(8):
            assert rows[codes == 0, 12 + e].any() == bool(fi and mask >> e & 1), (fi, mask, e)
    cc, _, _, crows, _ = CR.obs(T, E, scene["K"], scene["D"], img, X, nw, nr, ng, f, True)
    ic, _, _, irows, _ = IR.obs(T, E, kd0, img, X, nw, nr, ng, f, True, 0xFF)
    codes, _, _, rows, _ = QR.obs(T, E, kd0, img, X, nw, nr, ng, f, True, True)
    assert np.array_equal(codes, cc) and np.array_equal(codes, ic)
    assert rows[:, :12].tobytes() == np.ascontiguousarray(crows[:, :12]).tobytes()
    assert rows[:, 12:21].tobytes() == np.ascontiguousarray(irows[:, 6:15]).tobytes()


def _bound(Hm, x):
    """The forward-error bound of a positive definite solve: 10^3 2^-53 cond_2(H) |x| (the factor covers the
    dimension)."""
    return 1e3 * 2.0 ** -53 * np.linalg.cond(Hm) * np.linalg.norm(x)


MASKS = [(EXT, INT, 0xFF), (0b1000, 0b0001, 0xFF), (0b0100, 0b0100, 0xFF), (EXT, INT, 0x0F), (EXT, INT, 0xF0)]


@pytest.mark.parametrize("lam", [0.0, 1e-3])
@pytest.mark.parametrize("fe,fi,mask", MASKS)
def test_end_pass_against_the_full_system(scene, lm, fe, fi, mask, lam):
    """delta and eps of one step against numpy's solve of the full normal system assembled from the same
    acc231, within the cond-scaled bound; the updates against the rules in numpy; what is held comes back bit
    for bit."""
    p, rp = RR.default_params(lambda_=lam), QR.rcalib_params(fe, fi, mask)
    acc, cnt = _pass_acc(scene, lm, fe, fi, mask)
    R = QR.new_result(scene["ext"], scene["kd0"], fe, fi, mask, 3)
    fin, Tn, delta = QR.end_pass(acc, cnt, fe, fi, mask, 0, 4, p, rp, scene["T0"], R)
    assert not fin and R.status == 0 and R.iterations_run == 1
    Hm, g = QR.np_normal(acc, fe, fi, mask, lam)
    x = np.linalg.solve(Hm, -g)
    got = np.concatenate([delta.reshape(-1), QR.steps_of(R, 0, fe, fi, 4)])
    err = np.linalg.norm(got - x)
    print(f"ext {fe:#06b} int {fi:#06b} mask {mask:#04x} lambda {lam}: n {len(x)} cond(H) {np.linalg.cond(Hm):.3g} "
          f"|x| {np.linalg.norm(x):.3g} error {err:.3g} bound {_bound(Hm, x):.3g}")
    assert err <= _bound(Hm, x)
    kds, exts = QR.kds_of(R), QR.exts_of(R)
    held = [k for k in range(8) if not mask >> k & 1]
    for c in range(4):
        de, di = np.array(list(R.delta_ext[0][c])), np.array(list(R.delta_int[0][c]))
        if fe >> c & 1:
            assert de.any()
            np.testing.assert_allclose(exts[c], RR.exp_right(scene["ext"][c], de), rtol=0, atol=1e-14)
        else:
            assert not de.any() and exts[c].tobytes() == np.ascontiguousarray(scene["ext"][c]).tobytes()
        if fi >> c & 1:
            assert not di[held].any()
            np.testing.assert_allclose(kds[c], IR.np_update(scene["kd0"][c], di, mask), rtol=1e-15, atol=0)
            assert kds[c][held].tobytes() == scene["kd0"][c][held].tobytes()
        else:
            assert not di.any() and kds[c].tobytes() == scene["kd0"][c].tobytes()
    for r in range(3):
        np.testing.assert_allclose(Tn[r], RR.exp_right(scene["T0"][r], delta[r]), rtol=0, atol=1e-14)
    n = int(cnt.sum())
    assert R.n_obs[0] == n and list(R.n_obs_cam[0])[:4] == list(cnt.sum(axis=0))
    assert R.rms[0] == math.sqrt(sum(acc.reshape(-1, QR.ACC)[:, QR.ACC - 1].tolist()) / n)


def _concluded(acc, cnt, scene, fe, fi, mask, p):
    R = QR.new_result(scene["ext"], scene["kd0"], fe, fi, mask, 3)
    n = int(cnt.sum())
    R.n_obs[0] = n
    for c in range(4):
        R.n_obs_cam[0][c] = int(cnt[:, c].sum())
    rr = sum(acc.reshape(-1, QR.ACC)[:, QR.ACC - 1].tolist())
    R.rms[0] = math.sqrt(rr / n)
    QR.conclude(acc, cnt, fe, fi, mask, p, QR.rcalib_params(fe, fi, mask), R)
    return R, n, rr


@pytest.mark.parametrize("fe,fi,mask", [(EXT, INT, 0xFF), (0b0100, 0b0110, 0x3F)])
def test_covariances_against_the_full_inverse(scene, lm, fe, fi, mask):
    """cov_ext and cov_int against sigma^2 times the diagonal blocks of numpy's inverse of the full normal
    matrix (cov_int scaled to natural units), to 1e-8 of the block's largest entry (or the cond-scaled bound of
    the two inversions, if that is larger); zeros where held, and zeros when not calibrated."""
    p = RR.default_params()
    acc, cnt = _pass_acc(scene, lm, fe, fi, mask)
    R, n, rr = _concluded(acc, cnt, scene, fe, fi, mask, p)
    assert R.calibrated == 1
    Hm, _ = QR.np_normal(acc, fe, fi, mask)
    oe, oi, nn = QR.offsets(fe, fi, 3, 4)
    dof = n - 18 - 6 * len(oe) - bin(mask).count("1") * len(oi)
    inv, cond = np.linalg.inv(Hm), np.linalg.cond(Hm)
    tol_of = lambda ref: max(1e-8, 1e3 * 2.0 ** -53 * cond) * np.abs(ref).max()
    for c in range(4):
        ce, ci = np.array(list(R.cov_ext[c])).reshape(6, 6), np.array(list(R.cov_int[c])).reshape(8, 8)
        if c in oe:
            ref = rr / dof * inv[oe[c]: oe[c] + 6, oe[c]: oe[c] + 6]
            np.testing.assert_allclose(ce, ref, rtol=0, atol=tol_of(ref))
            assert np.array_equal(ce, ce.T) and np.all(np.diag(ce) > 0)
        else:
            assert not ce.any()
        if c in oi:
            kd = scene["kd0"][c]
            sc = np.array([kd[0], kd[1], kd[0], kd[1], 1, 1, 1, 1.0])
            ref = rr / dof * inv[oi[c]: oi[c] + 8, oi[c]: oi[c] + 8] * np.outer(sc, sc)
            for e in range(8):
                if not mask >> e & 1:
                    ref[e, :] = 0
                    ref[:, e] = 0
            np.testing.assert_allclose(ci, ref, rtol=0, atol=tol_of(ref))
            assert np.array_equal(ci, ci.T)
            assert np.all(np.diag(ci)[[e for e in range(8) if mask >> e & 1]] > 0)
        else:
            assert not ci.any()
        assert R.rms_cam[c] > 0
    assert not any(R.cov_ext[4]) and not any(R.cov_int[4])
    R2, _, _ = _concluded(acc, cnt, scene, fe, fi, mask, RR.default_params(max_rms=1e-9))  # a gate no rms passes
    assert R2.calibrated == 0
    assert not any(any(R2.cov_ext[c]) or any(R2.cov_int[c]) for c in range(8))


def test_zero_iterations_and_held_items(scene, lm):
    """I = 0 returns its inputs bit for bit (K as the float-rounded input); cameras held in a mask and masked
    parameters come back bit for bit after four iterations."""
    Ks, Ds = [scene["K"]] * 4, [scene["D"]] * 4
    ext0 = np.ascontiguousarray(np.array(scene["ext"]))
    T_out, R = QR.seq(scene["T0"], scene["ext"], Ks, Ds, scene["frames"], lm, RR.default_params(iterations=0),
                      QR.rcalib_params(EXT, INT))
    assert T_out.tobytes() == np.ascontiguousarray(np.array(scene["T0"])).tobytes()
    assert QR.exts_of(R).tobytes() == ext0.tobytes()
    assert QR.kds_of(R).tobytes() == np.ascontiguousarray(scene["kd0"]).tobytes()
    assert (R.status, R.iterations_run) == (0, 0) and R.n_obs[0] > 1000 and R.rms[0] > 0
    assert (R.n_rigs, R.n_cams, R.free_ext, R.free_int, R.param_mask, R.n_cand) == (3, 4, EXT, INT, 0xFF, 540)
    T_out, R = QR.seq(scene["T0"], scene["ext"], Ks, Ds, scene["frames"], lm, RR.default_params(),
                      QR.rcalib_params(0b1010, 0b0110, 0x33))
    assert R.status == 0 and R.iterations_run == 4
    kds, exts = QR.kds_of(R), QR.exts_of(R)
    held = [2, 3, 6, 7]
    for c in range(4):
        if c in (1, 3):
            assert not np.array_equal(exts[c], ext0[c])
        else:
            assert exts[c].tobytes() == ext0[c].tobytes()
        if c in (1, 2):
            assert kds[c][held].tobytes() == scene["kd0"][c][held].tobytes()
            assert np.all(kds[c][[0, 1, 4, 5]] != scene["kd0"][c][[0, 1, 4, 5]])
        else:
            assert kds[c].tobytes() == scene["kd0"][c].tobytes()
    assert not np.array(R.delta_int)[:, :, held].any() and not np.array(R.delta_int)[:, [0, 3]].any()
    assert not np.array(R.delta_ext)[:, [0, 2]].any() and np.array(R.delta_ext)[:4, [1, 3]].all()


def test_starved_gates(scene, lm):
    """One view blacked out: its rows fall below min_obs. One camera blacked out in every view starves the call
    when it is free in either mask (min_obs_cam) and not when it is held in both. A stop in pass 0 leaves the
    inputs unchanged."""
    p = RR.default_params()
    Ks, Ds = [scene["K"]] * 4, [scene["D"]] * 4
    black = np.zeros_like(scene["frames"][0][0])
    one_view = [list(fr) for fr in scene["frames"]]
    one_view[1] = [black] * 4
    one_cam = [[black if c == 2 else fr[c] for c in range(4)] for fr in scene["frames"]]
    cases = (("view", one_view, EXT, INT), ("ext only", one_cam, 0b0100, 0b0001), ("int only", one_cam, 0b1000, 0b0100))
    for name, frames, fe, fi in cases:
        rp = QR.rcalib_params(fe, fi)
        T_out, R = QR.seq(scene["T0"], scene["ext"], Ks, Ds, frames, lm, p, rp)
        assert (R.status, R.calibrated, R.iterations_run) == (1, 0, 0), name
        assert T_out.tobytes() == np.ascontiguousarray(np.array(scene["T0"])).tobytes()
        assert QR.exts_of(R).tobytes() == np.ascontiguousarray(np.array(scene["ext"])).tobytes()
        assert QR.kds_of(R).tobytes() == np.ascontiguousarray(scene["kd0"]).tobytes()
        assert not any(any(R.cov_ext[c]) or any(R.cov_int[c]) for c in range(8))
        cams = list(R.n_obs_cam[0])[:4]
        if name == "view":
            assert min(cams) >= rp.min_obs_cam and R.n_obs[0] == sum(cams)
        else:
            assert cams[2] == 0 and min(cams[0], cams[1], cams[3]) > 3 * p.min_obs
    T_out, R = QR.seq(scene["T0"], scene["ext"], Ks, Ds, one_cam, lm, RR.default_params(iterations=1),
                      QR.rcalib_params(0b1010, 0b1011))
    assert R.status != 1 and R.n_obs_cam[0][2] == 0


def _random_acc(rng, N, Cn, fe, fi, zero_col=None, zero_last_view=None, scale_r=1.0):
    acc = np.zeros((N, Cn, QR.ACC))
    cnt = np.full((N, Cn), 60, np.int32)
    for r in range(N):
        for c in range(Cn):
            rows = rng.normal(size=(60, 21))
            rows[:, 20] *= scale_r
            if not fe >> c & 1:
                rows[:, 6:12] = 0.0
            if not fi >> c & 1:
                rows[:, 12:20] = 0.0
            if zero_last_view is not None and r == N - 1:
                rows[:, zero_last_view] = 0.0
            if zero_col is not None:
                rows[:, zero_col] = 0.0
            acc[r, c] = QR.accumulate(rows)
    return acc, cnt


def test_singular_and_diverged_by_construction():
    """Rows that leave one pose direction unseen make A_r singular; rows with a zero J_ext column, or a zero
    J_int column that the mask calls free, leave A_r positive definite and put an exact zero on S's diagonal:
    SINGULAR, no update. Residuals a thousand times the Jacobian's size make the step drive fx (1 + eps0) below
    zero: DIVERGED, no update, the extrinsics kept too. The same accumulators with that column masked, or small
    residuals, step."""
    rng = np.random.default_rng(5)
    fe, fi = 0b10, 0b11
    p, rp = RR.default_params(min_obs=6), QR.rcalib_params(fe, fi, min_obs_cam=14)
    kd0 = np.tile([300.0, 301.0, 320.0, 240.0, 0.003, -0.01, 0.005, -0.002], (2, 1))
    ext0 = [np.eye(4), RR.exp_right(np.eye(4), [0.1, 0, 0, 0, 0.2, 0])]
    T0 = [np.eye(4), np.eye(4)]
    cases = (("A", {"zero_last_view": 2}, 0xFF, 2), ("S ext", {"zero_col": 8}, 0xFF, 2),
             ("S int", {"zero_col": 15}, 0xFF, 2), ("masked", {"zero_col": 15}, 0xF7, 0), ("none", {}, 0xFF, 0),
             ("diverged", {"scale_r": 1e3}, 0xFF, 3))
    for which, kw, mask, status in cases:
        acc, cnt = _random_acc(rng, 2, 2, fe, fi, **kw)
        R = QR.new_result(ext0, kd0, fe, fi, mask, 2)
        fin, Tn, delta = QR.end_pass(acc, cnt, fe, fi, mask, 0, 4, p, rp, T0, R)
        if status == 0:
            assert not fin and R.status == 0 and R.iterations_run == 1 and delta.any(), which
            continue
        assert fin and R.status == status and R.iterations_run == 0, (which, R.status)
        assert np.array_equal(Tn, np.array(T0)) and not delta.any()
        assert QR.kds_of(R).tobytes() == kd0.tobytes() and not np.array(R.delta_int).any()
        assert QR.exts_of(R).tobytes() == np.ascontiguousarray(np.array(ext0)).tobytes()
        assert not np.array(R.delta_ext).any()
        QR.conclude(acc, cnt, fe, fi, mask, p, rp, R)
        assert R.calibrated == 0 and not any(R.cov_ext[1]) and not any(R.cov_int[1])
    # a NaN accumulator entry in a free camera's II block: no pivot passes, never a NaN update
    acc, cnt = _random_acc(rng, 2, 2, fe, fi)
    acc[0, 1, QR.ACC - 1 - 3] = float("nan")  # (19, 19)
    R = QR.new_result(ext0, kd0, fe, fi, 0xFF, 2)
    fin, Tn, delta = QR.end_pass(acc, cnt, fe, fi, 0xFF, 0, 4, p, rp, T0, R)
    assert fin and R.status in (2, 3) and np.array_equal(Tn, np.array(T0)) and QR.kds_of(R).tobytes() == kd0.tobytes()
    assert QR.exts_of(R).tobytes() == np.ascontiguousarray(np.array(ext0)).tobytes()


def test_joint_scene_is_calibrated_and_alternation_is_not(scene, lm, calibrated):
    """The issue's scene (ext 0b1110, int 0b1111, 0xFF, I = 4, lambda = 0) through hc_rcalib_seq and its
    accuracy conditions; the alternation of the two single calibrations (16 steps) on the same scene, worse on
    every free camera's extrinsic.

    Measured (host rule): model gap 5.76 / 3.75 / 4.02 / 4.01 px -> 0.368 / 0.189 / 0.181 / 0.259 (worst
    1/15.5); extrinsics 1.12-1.20 cm, 0.69 deg -> 0.088 / 0.124 / 0.106 cm (worst 1/9.7), 0.075 / 0.043 /
    0.091 deg (worst 1/7.6); poses 0.076 / 0.064 / 0.055 cm; fresh views 2.30-3.19 cm -> 0.029-0.078 cm
    (1/38 to 1/89). Alternation: gaps 3.06 / 2.57 / 1.57 / 2.25 px, extrinsics 3.69 / 0.69 / 3.49 cm,
    0.40-0.49 deg, poses 1.86-1.93 cm."""
    T_out, R = calibrated
    assert (R.status, R.calibrated, R.iterations_run) == (0, 1, 4)
    g0, e0, p0 = QR.figures(scene["T0"], scene["ext"], scene["kd0"], scene)
    g1, e1, p1 = QR.figures(T_out, QR.exts_of(R), QR.kds_of(R), scene)
    cm = lambda e: [(round(100 * a, 3), round(b, 3)) for a, b in e]
    print("model gap px, start / joint:", np.round(g0, 3), np.round(g1, 3), "ratios", np.round(np.array(g0) / g1, 1))
    print("extrinsics (cm, deg), start / joint:", cm(e0), cm(e1))
    print("poses cm, start / joint:", np.round(100 * np.array(p0), 3), np.round(100 * np.array(p1), 3))
    print("rms x fx per pass:", [round(v * 323.15, 3) for v in list(R.rms)[:5]], "n_obs", list(R.n_obs)[:5])
    Ta, Ea, ka = QR.alternation(scene, lm)
    g2, e2, p2 = QR.figures(Ta, Ea, ka, scene)
    print("alternation: model gap px", np.round(g2, 3), "extrinsics", cm(e2), "poses cm", np.round(100 * np.array(p2), 3))
    fv = QR.fresh_views()
    p = RR.default_params()
    fresh = []
    for r in range(len(fv["Twb"])):
        T, T0 = fv["Twb"][r], RR.shift(fv["Twb"][r])
        given = IR.refine_with(T0, scene["ext"], scene["kd0"], fv["frames"][r], lm, p)
        calib = IR.refine_with(T0, list(QR.exts_of(R)), QR.kds_of(R), fv["frames"][r], lm, p)
        fresh.append((RR.pose_dist(np.array(given.T_w_b).reshape(4, 4), T)[0],
                      RR.pose_dist(np.array(calib.T_w_b).reshape(4, 4), T)[0], given.refined, calib.refined))
    print("fresh views cm (nominal rig, calibrated rig):", [(round(100 * a, 3), round(100 * b, 4)) for a, b, _, _ in fresh])
    for c in range(4):
        assert g1[c] < g0[c] / 8, (c, g0, g1)
    for c in range(1, 4):
        assert e1[c][0] < e0[c][0] / 5 and e1[c][1] < e0[c][1] / 5, (c, e0, e1)
        assert e2[c][0] > e1[c][0] and e2[c][1] > e1[c][1], (c, e1, e2)  # alternation is worse than the joint solve
    assert QR.exts_of(R)[0].tobytes() == np.ascontiguousarray(scene["ext"][0]).tobytes()
    assert max(p1) < 0.002, p1
    for dg, dc, _, ok in fresh:
        assert ok == 1 and dc < dg / 10, fresh
    assert all(0 < R.cov_int[c][0] < 4.0 for c in range(4)) and all(R.cov_ext[c][0] > 0 for c in (1, 2, 3))
    assert not any(R.cov_ext[0])
