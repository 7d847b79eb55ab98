"""The grid-line matrix on the host (tests/_line_cases.py): the census of its
cells -- final seed, guard, status, pass-0 codes and flagged share, printed per
cell -- and the references that do not need a GPU: the host build of the
observation rule (hc_refine_obs) against its numpy restatement on every cell
and on the constructed slots, the Jacobian columns of every lens against
central differences through the calibrations' own helpers, and the mixed rig
refined by hc_refine_seq with per-camera K and D.
"""
import math
import time

import numpy as np
import pytest

import _icalib_ref as IR
import _line_cases as LC
import _rcalib_ref as QR
import _refine_ref as RR
import _score_cases as SC
from test_rcalib_host import _check_jacobians as check_jacobians_20
from test_rcalib_host import _residual

# (status, refined / calibrated, iterations_run) of the host sequence alone, per cell; every cell not listed is
# OK = (0, 1, 4). STARVED = 1, SINGULAR = 2. The 33x7 frames hold a handful of lines: with the 25-sample window
# (R12) all but `off` starve or are singular in pass 0, x045 after two steps.
OK = (0, 1, 4)
REFINE_STATUS = {
    "strong2-33x7-R2": (1, 0, 0), "x3-33x7-R2": (1, 0, 0),
    "bench-33x7-R12": (2, 0, 0), "d0-33x7-R12": (1, 0, 0), "strong0-33x7-R12": (1, 0, 0),
    "strong1-33x7-R12": (2, 0, 0), "strong2-33x7-R12": (1, 0, 0), "x3-33x7-R12": (1, 0, 0),
    "x045-33x7-R12": (1, 0, 2), "pp_out-33x7-R12": (1, 0, 0),
}
# the x3 lens sees 46 lines in two views of two cameras: below min_obs_cam
CALIB_STATUS = {("rig", "x3"): (1, 0, 0)}
CAP = 0.005


def refine_status(key):
    return REFINE_STATUS.get(LC.cell_id(key), OK)


def calib_status(kind, name):
    return CALIB_STATUS.get((kind, name), OK)


def _pass_poses(c):
    """The poses of the host sequence's passes: the deltas composed (test_seq_refines_a_four_camera_rig)."""
    Ts = [c.T0]
    for k in range(c.host.iterations_run):
        Ts.append(RR.exp_right(Ts[-1], np.array(c.host.delta[k])))
    return Ts


def _refine_obs(c, T, cam):
    X, nw, nr, ng = LC.landmarks()
    f = RR.flags(X, 0.08)
    return RR.obs(T, c.exts[cam], IR.K_of(c.kds[cam]), c.kds[cam][4:], c.frames[cam], X, nw, nr, ng, f, R=c.R)


def test_refinement_census():
    t0 = time.time()
    seen = np.zeros(6, np.int64)
    for key in LC.refine_cell_ids() + ["mixed0", "mixed1", "mixed2"]:
        mixed = isinstance(key, str)
        c = LC.mixed_rig(int(key[-1])) if mixed else LC.refine_cell(*key)
        name = key if mixed else LC.cell_id(key)
        hist = np.zeros(6, np.int64)
        flagged = total = 0
        for k, T in enumerate(_pass_poses(c)):
            for cam in range(len(c.frames)):
                codes, _, _, _, tie = _refine_obs(c, T, cam)
                flagged += int((tie != 0).sum())
                total += len(codes)
                if k == 0:
                    hist += np.bincount(codes, minlength=6)
        seen += hist
        got = (c.host.status, c.host.refined, c.host.iterations_run)
        print(f"{name}: seed {c.seed} guarded {c.guarded} motion {c.motion:.2e} status {got} pass-0 codes "
              f"{hist.tolist()} flagged {flagged}/{total} n_obs {list(c.host.n_obs)[:c.host.iterations_run + 1]}")
        assert c.seeds_moved < LC.SEED_TRIES
        assert got == (OK if mixed else refine_status(key)), name
        assert flagged <= CAP * total, name
        assert hist[0] == c.host.n_obs[0]
        if mixed or (c.w, c.h) in LC.LARGE:
            assert c.guarded, f"{name}: a large cell must keep the whole-call guard"
    print(f"codes over the matrix {seen.tolist()}; {time.time() - t0:.1f} s")
    assert all(seen[k] > 0 for k in (0, 1, 3, 4, 5)), seen  # code 2: test_constructed_slots_on_the_host


def _calib_cells():
    out = [(kind, n, 0xFF) for kind in LC.KINDS for n in LC.LENSES]
    return out + [("int", "bench", 0xF0), ("rig", "bench", 0xF0)] + [(kind, "mixed", 0xFF) for kind in LC.KINDS]


def get_calib_cell(kind, name, mask):
    return LC.mixed_calib_cell(kind) if name == "mixed" else LC.calib_cell(name, kind, mask)


def _calib_obs(c, T, E, kd, img, cam):
    """One camera's pass of the cell's call on the host, the slot guard in the flag where the rows use G."""
    X, nw, nr, ng = LC.landmarks()
    f = RR.flags(X, 0.08)
    p = RR.default_params()
    fe, fi = LC.free_of(c.kind, len(c.exts))
    if c.kind == "ext":
        import _calib_ref as CR

        return CR.obs(T, E, IR.K_of(kd), kd[4:], img, X, nw, nr, ng, f, fe >> cam & 1)
    if c.kind == "int":
        return LC.int_slot_guard(T, E, kd, img, f, fi >> cam & 1, c.mask, p)
    return LC.rig_slot_guard(T, E, kd, img, f, fe >> cam & 1, fi >> cam & 1, c.mask, p)


def test_calibration_census():
    """Pass 0 at the inputs and the last pass at the host's result (the passes between are not returned)."""
    import _calib_ref as CR

    t0 = time.time()
    for kind, name, mask in _calib_cells():
        c = get_calib_cell(kind, name, mask)
        res = c.host
        flagged = ties = total = 0
        hist = np.zeros(6, np.int64)
        E1 = CR.exts_of(res) if kind in ("ext", "rig") else np.array(c.exts)
        kd1 = IR.kds_of(res) if kind in ("int", "rig") else c.kds
        for k, (Ts, Es, kds) in enumerate(((c.T0s, c.exts, c.kds), (c.hT, E1, kd1))):
            for r in range(len(c.frames)):
                for cam in range(len(c.exts)):
                    codes, _, _, rows, flag = _calib_obs(c, Ts[r], Es[cam], kds[cam], c.frames[r][cam], cam)
                    flagged += int((flag != 0).sum())
                    ties += int((flag == 1).sum())
                    total += len(codes)
                    assert np.isfinite(rows).all()
                    if k == 0:
                        hist += np.bincount(codes, minlength=6)
        got = (res.status, res.calibrated, res.iterations_run)
        cap = max(LC.flag_cap(n, kind) for n in c.names)
        print(f"{kind} {name} mask {mask:#x}: seed {c.seed} guarded {c.guarded} motion {c.motion:.2e} status {got} "
              f"pass-0 codes {hist.tolist()} flagged {flagged}/{total} (ties {ties}, cap {cap}) n_obs "
              f"{list(res.n_obs)[:res.iterations_run + 1]}")
        assert c.seeds_moved < LC.SEED_TRIES
        assert got == (OK if name == "mixed" or mask != 0xFF else calib_status(kind, name)), (kind, name)
        assert flagged <= cap * total, (kind, name, flagged, total)
        assert hist[0] == res.n_obs[0]
    print(f"{time.time() - t0:.1f} s")


def _target(i, nw, nr):
    return RR.TARGETS["w" if i < nw else "r" if i < nw + nr else "g"]


def _against_numpy(T, E, kd, img, R, ks, what, with_ties=False, **kw):
    """hc_refine_obs against RR.np_observe on the candidates ks: codes and integer sums exact, rows to
    test_obs_matches_numpy's rtol 1e-12. Returns the codes seen and the number of tie-flagged slots left out."""
    X, nw, nr, ng = LC.landmarks()
    f = RR.flags(X, 0.08)
    cand = RR.candidates(f)
    K, D = IR.K_of(kd), kd[4:]
    codes, Sw, Skw, rows, tie = RR.obs(T, E, K, D, img, X, nw, nr, ng, f, R=R, **kw)
    assert np.all(rows[codes != 0] == 0.0)
    seen, left = set(), 0
    for k in ks:
        if tie[k] and not with_ties:
            left += 1
            continue
        i = cand[k]
        code, sw, skw, row = RR.np_observe(T, E, K, D, img, X[i], 0 if f[i] == 1 else 1, _target(i, nw, nr), R=R, **kw)
        assert (codes[k], Sw[k], Skw[k]) == (code, sw, skw), (what, k, i)
        np.testing.assert_allclose(rows[k], row, rtol=1e-12, atol=0, err_msg=f"{what} candidate {k}")
        seen.add(code)
    return seen, left


@pytest.mark.parametrize("size", LC.REFINE_CELLS, ids=lambda s: f"{s[0]}x{s[1]}-R{s[2]}")
def test_host_build_against_numpy(size):
    """Every fifth candidate of both cameras of every lens at the shifted pose."""
    w, h, R = size
    seen, left, n = set(), 0, 0
    for name in LC.LENSES:
        c = LC.refine_cell(name, w, h, R)
        for cam in range(2):
            s, l = _against_numpy(c.T0, c.exts[cam], c.kds[cam], c.frames[cam], R, range(0, 540, 5),
                                  LC.cell_id((name, *size)))
            seen |= s
            left += l
            n += 108
    print(size, "codes", sorted(seen), "left out", left, "of", n)
    assert left <= CAP * n and 3 in seen and len(seen) >= 3


def test_constructed_slots_on_the_host():
    X, nw, nr, ng = LC.landmarks()
    f = RR.flags(X, 0.08)
    black = np.zeros((240, 320, 3), np.uint8)
    kd = LC.kd_of("bench", 320, 240)
    # code 2 in every slot, in all four rules
    T = LC.no_tangent_pose()
    seen, _ = _against_numpy(T, np.eye(4), kd, black, 12, range(540), "no tangent")
    assert seen == {2}
    import _calib_ref as CR

    for codes, rows in (CR.obs(T, np.eye(4), IR.K_of(kd), kd[4:], black, X, nw, nr, ng, f, True)[0::3],
                        IR.obs(T, np.eye(4), kd, black, X, nw, nr, ng, f, True)[0::3],
                        QR.obs(T, np.eye(4), kd, black, X, nw, nr, ng, f, True, True)[0::3]):
        assert np.all(codes == 2) and not rows.any()
    # the on-axis candidate: the observation itself against numpy (its J_int: test_jacobian_on_the_axis)
    T, E, kda, img, k, nh = LC.on_axis_case()
    # (its samples lie on u = cx = 159.5 or v = cy exactly, a tie by the flag and the same bits on every side)
    seen, left = _against_numpy(T, E, kda, img, 12, [k], "on the axis", with_ties=True)
    assert seen == {0} and left == 0
    # the window's last sample a quarter pixel inside / outside every edge: code 3 exactly outside
    for edge in LC.EDGES:
        for side in ("in", "out"):
            T, kde, k, target, hor = LC.edge_case(edge, side)
            frame = np.zeros((505, 907, 3), np.uint8)
            seen, left = _against_numpy(T, np.eye(4), kde, frame, 12, [k], f"edge {edge} {side}")
            assert left == 0 and seen == ({5} if side == "in" else {3}), (edge, side, seen)


def _fold_rho(kd):
    """rho = tan(theta) at the end of theta_d's first increasing branch, inf if it never folds."""
    t = SC.theta_branch(kd[4:])
    return math.inf if t >= SC.HALF_PI - 1e-9 else math.tan(t)


NEAR_FOLD = 0.1


class NoInverse(Exception):
    pass


def _undist_on_branch(kd, P, th0):
    """m with dist_kd(m) = P on the branch of theta_d that holds th0: Newton on theta from th0 (test_rcalib_host's
    _undist starts at theta = theta_d, which finds the first branch only). Beyond the zero of theta_d the image
    lies on the other side of the principal point, so the radius carries theta_d's sign. NoInverse if the
    iteration does not settle on th0's side of the fold."""
    px, py = (P[0] - kd[2]) / kd[0], (P[1] - kd[3]) / kd[1]
    rd = math.hypot(px, py)
    thd = lambda t: t + kd[4] * t ** 3 + kd[5] * t ** 5 + kd[6] * t ** 7 + kd[7] * t ** 9
    dthd = lambda t: 1 + 3 * kd[4] * t ** 2 + 5 * kd[5] * t ** 4 + 7 * kd[6] * t ** 6 + 9 * kd[7] * t ** 8
    sgn = 1.0 if thd(th0) > 0 else -1.0
    side = dthd(th0) > 0
    th = th0
    for _ in range(60):
        d = dthd(th)
        if d == 0 or not math.isfinite(th):
            raise NoInverse
        th -= (thd(th) - sgn * rd) / d
    if not (0 < th < SC.HALF_PI) or (dthd(th) > 0) != side or abs(thd(th) - sgn * rd) > 1e-14:
        raise NoInverse
    return np.array([px, py]) * (math.tan(th) / (sgn * rd))


def _check_jacobians_on_branch(T, E, kd, Xi, axis, row, what):
    """test_rcalib_host._check_jacobians for a slot within NEAR_FOLD of the fold of theta_d or beyond it, with
    the same bound, 1e-7 of the row's largest entry, and two changes to the reference. The lens is inverted on
    the slot's own branch (_undist_on_branch). And near the fold the helper's central difference at step 1e-6
    fails its own bound: the inverse of the lens has derivatives that grow like powers of |G^-1| (12 to 59 in
    these slots) and the quotient is off by up to 4e-4 of the row's largest entry, four times less at half the
    step: truncation, not the rule. Where that error exceeds the bound, the ratio is asserted here. So the
    reference is the Richardson extrapolation (4 d(h / 2) - d(h)) / 3 of central differences at h = 2.5e-7 and
    h / 2, which cancels the h^2 term; the h^4 term, 7e-7 at 1e-6 in the worst slot, is 3e-9 at 2.5e-7, and
    rounding 2^-53 |G^-1| / h ~ 5e-8 absolute stands against a bound above 1e-6. Raises NoInverse if the lens
    cannot be inverted on the branch for every perturbed parameter set (a slot at the fold itself)."""
    p, q, m0, nh, Jpi, R_cb = RR.np_geometry(T, E, Xi, axis)
    m_obs = m0 - row[20] * nh
    P = IR.np_dist(kd, m0[0], m0[1])
    th0 = math.atan(math.hypot(*m0))
    if np.abs(_undist_on_branch(kd, P, th0) - m0).max() > 1e-10:  # Newton at |G^-1| ~ 50
        raise NoInverse

    def central_int(h):
        num = np.zeros(8)
        for a in range(8):
            e = np.zeros(8)
            e[a] = h
            rp = float(nh @ (m0 - _undist_on_branch(IR.np_update(kd, e, 0xFF), P, th0)))
            rm = float(nh @ (m0 - _undist_on_branch(IR.np_update(kd, -e, 0xFF), P, th0)))
            num[a] = (rp - rm) / (2 * h)
        return num

    num = np.zeros(20)
    h = 1e-6  # the pose and extrinsic columns have no lens in them: the helper's step holds for them
    for a in range(6):
        e = np.zeros(6)
        e[a] = h
        num[a] = (_residual(RR.exp_right(T, e), E, Xi, nh, m_obs) -
                  _residual(RR.exp_right(T, -e), E, Xi, nh, m_obs)) / (2 * h)
        num[6 + a] = (_residual(T, RR.exp_right(E, e), Xi, nh, m_obs) -
                      _residual(T, RR.exp_right(E, -e), Xi, nh, m_obs)) / (2 * h)
    num[12:] = (4 * central_int(1.25e-7) - central_int(2.5e-7)) / 3
    tol = 1e-7 * np.abs(row[:20]).max()
    e1 = np.abs(central_int(1e-6) - row[12:20]).max()
    if e1 > tol:  # the plain quotient misses the bound: by truncation, four times less at half the step
        e2 = np.abs(central_int(5e-7) - row[12:20]).max()
        print(f"{what}: the quotient at 1e-6 is off by {e1 / tol * 1e-7:.2e} of the row, {e1 / e2:.3f} times that "
              f"at 5e-7")
        assert 3.8 < e1 / e2 < 4.2, (what, e1, e2)
    for name, sl in (("J_pose", slice(0, 6)), ("J_ext", slice(6, 12)), ("J_int", slice(12, 20))):
        np.testing.assert_allclose(row[sl], num[sl], rtol=0, atol=tol, err_msg=f"{name} of {what}")


@pytest.mark.parametrize("name", LC.LENSES)
def test_jacobians_per_lens(name):
    """The 20 Jacobian columns (pose, extrinsic, intrinsic) of the rig rule's rows against central differences
    on the view and camera with the most live slots of the lens's intrinsic-calibration cell: every tenth live
    slot, the live slot of largest rho and, for a lens whose theta_d folds inside the frame, the live slot
    nearest the fold, all taken over every live slot, beyond the fold included. One helper covers the three
    calibrations because their rows are the same numbers: test_columns_are_shared asserts per lens that
    hc_calib_obs's extrinsic columns and hc_icalib_obs's intrinsic columns are hc_rcalib_obs's, bit for bit, and
    the pose columns the refinement's. A slot well inside the first branch goes through
    test_rcalib_host._check_jacobians as it is (step 1e-6, bound 1e-7 of the row's largest entry, the figures of
    test_calib_host and test_icalib_host too); a slot within NEAR_FOLD of the fold or beyond it through
    _check_jacobians_on_branch, same bound. The pose columns also within test_refine_host's absolute 1e-8. A
    slot that fails the single-slot guard, or whose lens cannot be inverted on its branch, is left out and
    counted against the cap."""
    X, nw, nr, ng = LC.landmarks()
    f = RR.flags(X, 0.08)
    cand = RR.candidates(f)
    c = LC.calib_cell(name, "int")
    p = RR.default_params()
    best = None
    for r in range(2):
        for cam in range(2):
            got = LC.rig_slot_guard(c.T0s[r], c.exts[cam], c.kds[cam], c.frames[r][cam], f, True, True, 0xFF, p)
            if best is None or (got[0] == 0).sum() > (best[2][0] == 0).sum():
                best = (r, cam, got)
    r, cam, (codes, _, _, rows, flag) = best
    T, E, kd = c.T0s[r], c.exts[cam], c.kds[cam]
    live = np.flatnonzero(codes == 0)
    assert len(live) >= 50
    axis_of = lambda k: 0 if f[cand[k]] == 1 else 1
    rho = {k: math.hypot(*RR.np_geometry(T, E, X[cand[k]], axis_of(k))[2]) for k in live}
    fold = _fold_rho(kd)
    picks = list(live[::10]) + [max(live, key=lambda k: rho[k])]
    beyond = [k for k in live if rho[k] >= fold]
    if math.isfinite(fold):
        picks.append(min(live, key=lambda k: abs(rho[k] - fold)))
        picks += beyond[::5]  # and every fifth slot of the far branch
        print(f"{name}: fold at rho {fold:.4f}, nearest live slot at {rho[picks[len(live[::10]) + 1]]:.4f}, "
              f"{len(beyond)} live slots beyond it")
    left = int((flag[live] != 0).sum())
    cap = LC.flag_cap(name, "rig")
    checked = checked_beyond = 0
    for k in dict.fromkeys(picks):
        if flag[k]:
            continue
        what = f"{name} candidate {k} (rho {rho[k]:.4f})"
        if rho[k] > fold - NEAR_FOLD:
            try:
                _check_jacobians_on_branch(T, E, kd, X[cand[k]], axis_of(k), rows[k], what)
            except NoInverse:
                print(f"{what}: no inverse on its branch, left out")
                left += 1
                continue
            checked_beyond += rho[k] >= fold
        else:
            check_jacobians_20(T, E, kd, X[cand[k]], axis_of(k), rows[k], what)
        # the refinement's pose columns are these, bit for bit; its own bound is absolute
        g = RR.np_geometry(T, E, X[cand[k]], axis_of(k))
        m0, nh = g[2], g[3]

        def fn(d6):
            p = np.linalg.inv(RR.exp_right(T, d6) @ E) @ np.append(X[cand[k]], 1.0)
            return nh @ (p[:2] / p[2] - m0)

        h = 1e-6
        num = np.array([(fn(h * np.eye(6)[a]) - fn(-h * np.eye(6)[a])) / (2 * h) for a in range(6)])
        np.testing.assert_allclose(rows[k, :6], num, rtol=0, atol=1e-8)
        checked += 1
    print(f"{name}: {len(live)} live slots, {left} left out (cap {cap}), largest rho {max(rho.values()):.3f}, "
          f"|J_int| max {np.abs(rows[live, 12:20]).max():.1f}, {checked} checked, {checked_beyond} beyond the fold")
    assert left <= cap * len(live)
    assert checked >= 5 and (not beyond or checked_beyond >= 5)


def test_columns_are_shared():
    """Per lens: the pose columns, codes and sums of the three calibrations' rows are the refinement's, the
    extrinsic columns of hc_calib_obs and the intrinsic columns of hc_icalib_obs are hc_rcalib_obs's, bit for
    bit. So the 20 columns test_jacobians_per_lens checks on the rig rule's rows are every rule's."""
    import _calib_ref as CR

    X, nw, nr, ng = LC.landmarks()
    f = RR.flags(X, 0.08)
    for name in LC.LENSES:
        c = LC.calib_cell(name, "rig")
        T, E, kd, img = c.T0s[1], c.exts[0], c.kds[0], c.frames[1][0]
        K, D = IR.K_of(kd), kd[4:]
        rc, rSw, rSkw, rrows, rtie = RR.obs(T, E, K, D, img, X, nw, nr, ng, f)
        ext = CR.obs(T, E, K, D, img, X, nw, nr, ng, f, True)
        int_ = IR.obs(T, E, kd, img, X, nw, nr, ng, f, True)
        rig = QR.obs(T, E, kd, img, X, nw, nr, ng, f, True, True)
        for rows, last in ((ext, 12), (int_, 14), (rig, 20)):
            codes, Sw, Skw, rw, tie = rows
            assert np.array_equal(codes, rc) and np.array_equal(Sw, rSw) and np.array_equal(Skw, rSkw), name
            assert np.array_equal(rw[:, :6], rrows[:, :6]) and np.array_equal(rw[:, last], rrows[:, 6]), name
        assert np.array_equal(ext[3][:, 6:12], rig[3][:, 6:12]) and np.abs(ext[3][:, 6:12]).max() > 0, name
        assert np.array_equal(int_[3][:, 6:14], rig[3][:, 12:20]) and np.abs(int_[3][:, 6:14]).max() > 0, name


def test_mixed_rig_refines():
    """hc_refine_seq with per-camera K and D on the three mixed rigs, test_seq_refines_a_four_camera_rig's
    condition: status 0, refined, closer to the truth than the start in translation and in rotation. With every
    camera given the first camera's lens the same frames do not refine to it."""
    for r in range(3):
        c = LC.mixed_rig(r)
        res = c.host
        Tr = np.array(res.T_w_b).reshape(4, 4)
        d0, a0 = RR.pose_dist(c.T0, c.T)
        d1, a1 = RR.pose_dist(Tr, c.T)
        print(f"mixed rig {r}: {100 * d0:.3f} cm / {a0:.4f} deg -> {100 * d1:.4f} cm / {a1:.4f} deg, n_obs "
              f"{list(res.n_obs)[:5]}")
        assert res.status == 0 and res.refined == 1 and res.iterations_run == 4 and res.n_cand == 540
        assert d1 < d0 and a1 < a0
        wrong = LC.refine_seq(c.T0, c.exts, np.tile(c.kds[0], (4, 1)), c.frames, RR.default_params())
        dw, aw = RR.pose_dist(np.array(wrong.T_w_b).reshape(4, 4), c.T)
        assert wrong.status != 0 or dw > 2 * d1, (dw, d1)
