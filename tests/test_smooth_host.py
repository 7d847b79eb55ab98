"""Window smoothing on the CPU: the host build of mk_smooth.h (hc_smooth_*)
against numpy -- the three Jacobians against central differences, the block
Cholesky against the dense solve, the marginals against the dense inverse, the
whole call replayed pass by pass against the dense normal system -- and the
properties of the rule: N = 1 is the refinement, a broken chain is its
segments, I = 0 returns its input, the gates, and the blind-view scene.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _refine_ref as RR
import _smooth_ref as SR
from mantis_amd import synth


@pytest.fixture(scope="module")
def lm(landmark_map):
    return RR.all_landmarks(landmark_map)


@pytest.fixture(scope="module")
def blind5():
    """The accuracy scene: five views of the four-camera ring chained by the 8 cm / 3 degree step, view 2 black."""
    return SR.trajectory(5, blind=(2,))


def _rand_pose(rng):
    return synth.random_base_pose(rng)


def _noise(rng, rot=0.05, t=0.02):
    N = np.eye(4)
    N[:3, :3] = SR.np_exp(rng.normal(0, rot, 3))
    N[:3, 3] = rng.normal(0, t, 3)
    return N


def test_struct_sizes_defaults_and_null_arguments():
    import mantis_amd as M

    L = M.lib()
    p = M.MantisSmoothParams()
    L.mantis_default_smooth_params(C.byref(p))
    assert p.struct_size == C.sizeof(M.MantisSmoothParams)
    r = M.MantisRefineParams()
    L.mantis_default_refine_params(C.byref(r))
    for f in ("iterations", "half_window", "white_thresh", "min_weight", "min_obs", "lambda_", "landmark_pitch", "max_rms",
              "record"):
        assert getattr(p, f) == getattr(r, f), f
    assert (p.sigma_row, p.sigma_t, p.sigma_rot) == (0.00127, 0.01, 0.03)
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    L.mantis_smooth_sizes(C.byref(a), C.byref(b), C.byref(c))
    assert a.value == C.sizeof(M.MantisSmoothParams) == SR.hc().hc_sizeof_smooth_params()
    assert b.value == C.sizeof(M.MantisSmoothResult) == SR.hc().hc_sizeof_smooth_result()
    assert c.value == C.sizeof(M.MantisSmoothView) == SR.hc().hc_sizeof_smooth_view()
    assert L.mantis_abi_version() == 5
    L.mantis_default_smooth_params(None)
    L.mantis_smooth_sizes(None, None, None)
    assert L.mantis_smooth_batch(None, None, 1, 1, 1, None, None, None, None, None, None, None) == 1
    assert L.mantis_get_smooth_record(None, 0, 0, 0, None, None, None, None, None, None) == 1
    assert L.mantis_get_smooth_pass(None, 0, 0, None, None, None, None, None) == 1


@pytest.mark.parametrize("case", ["random", "e=0", "theta<1e-8"])
def test_jacobians_against_central_differences(case):
    """de/dx_k, de/dx_k+1 and the prior's de_p/dx_0 against central differences of the numpy residual (step
    1e-6, agreement 1e-7), with the right perturbation T <- T D(x) of the refinement's step."""
    rng = np.random.default_rng({"random": 3, "e=0": 4, "theta<1e-8": 5}[case])
    for trial in range(5):
        Tk, D = _rand_pose(rng), SR.step(*rng.uniform(-0.1, 0.1, 1), yaw_deg=rng.uniform(-10, 10),
                                         dy=rng.uniform(-0.05, 0.05), roll_deg=rng.uniform(-3, 3))
        if case == "random":
            Tn = Tk @ D @ _noise(rng)
        elif case == "e=0":
            Tn = Tk @ D
        else:  # a rotation residual below the small-angle switch, a translation residual of ordinary size
            Tn = Tk @ D @ _noise(rng, rot=2e-9, t=0.02)
        e, Ja, Jb = SR.between(Tk, Tn, D)
        if case == "theta<1e-8":
            assert 0 < np.linalg.norm(e[3:]) < 1e-8
        np.testing.assert_allclose(e, SR.np_between(Tk, Tn, D), rtol=0, atol=1e-12)
        Ja_n = SR.central(lambda d: SR.np_between(RR.exp_right(Tk, d), Tn, D))
        Jb_n = SR.central(lambda d: SR.np_between(Tk, RR.exp_right(Tn, d), D))
        print(case, trial, "between:", np.abs(Ja - Ja_n).max(), np.abs(Jb - Jb_n).max())
        np.testing.assert_allclose(Ja, Ja_n, rtol=0, atol=1e-7)
        np.testing.assert_allclose(Jb, Jb_n, rtol=0, atol=1e-7)
        ok, pe, pJ = SR.prior(Tn, Tk @ D, np.eye(6))  # identity covariance: the factor unwhitened
        assert ok
        np.testing.assert_allclose(pe, SR.np_prior(Tn, Tk @ D), rtol=0, atol=1e-12)
        pJ_n = SR.central(lambda d: SR.np_prior(RR.exp_right(Tn, d), Tk @ D))
        print(case, trial, "prior:", np.abs(pJ - pJ_n).max())
        np.testing.assert_allclose(pJ, pJ_n, rtol=0, atol=1e-7)
    # whitening scales rows 0..2 by wt and rows 3..5 by wr, residual and Jacobians alike
    e2, Ja2, Jb2 = SR.between(Tk, Tn, D, 3.0, 0.25)
    s = np.array([3.0] * 3 + [0.25] * 3)
    assert np.array_equal(e2, s * e) and np.array_equal(Ja2, s[:, None] * Ja) and np.array_equal(Jb2, s[:, None] * Jb)


def test_small_angle_forms():
    """log_so3 and J_r^-1 at theta = 0, just under and just over 1e-8: continuous across the switch."""
    assert np.array_equal(SR.log_so3(np.eye(3)), np.zeros(3))
    assert np.array_equal(SR.jr_inv(np.zeros(3)), np.eye(3))
    ax = np.array([1.0, -2.0, 0.5]) / np.linalg.norm([1.0, -2.0, 0.5])
    for th in (0.999e-8, 1.001e-8, 1e-5, 0.3, 2.5):
        phi = th * ax
        got = SR.log_so3(SR.np_exp(phi))
        np.testing.assert_allclose(got, phi, rtol=0, atol=max(1e-15, 4e-16 * th / max(math.sin(th), 1e-8)))
        K = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]])
        k = 1 / 12 if th < 1e-4 else 1 / th ** 2 - (1 + math.cos(th)) / (2 * th * math.sin(th))
        np.testing.assert_allclose(SR.jr_inv(phi), np.eye(3) + 0.5 * K + k * K @ K, rtol=0, atol=1e-12)
    # a half turn about an axis: the branch that reads the axis from R + I
    for axis in np.eye(3):
        Rm = 2 * np.outer(axis, axis) - np.eye(3)
        np.testing.assert_allclose(np.abs(SR.log_so3(Rm)), math.pi * axis, rtol=0, atol=1e-12)


def test_residual_is_zero_on_the_chain():
    """T_k+1 = T_k Delta_k with the library's own Transform. Where the products are exact (an axis-aligned
    T_k at the origin: R_D^T R_D is exactly symmetric, t_M - t_D exactly zero) the residual is exactly zero;
    at a general pose the products R_k^T (R_k R_D) round, which bounds it by a few ulp of the operands."""
    rng = np.random.default_rng(8)
    for trial in range(4):
        D0 = SR.step(yaw_deg=rng.uniform(-20, 20), dy=rng.uniform(-0.1, 0.1), roll_deg=rng.uniform(-5, 5))
        has, D = SR.transform(SR.motion_of(D0))
        assert has
        for Tk in (np.eye(4), np.diag([-1.0, -1.0, 1.0, 1.0]),
                   np.array([[0, -1.0, 0, 0], [1.0, 0, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])):
            e, _, _ = SR.between(Tk, Tk @ D, D, 0.127, 0.0423)
            assert np.array_equal(e, np.zeros(6)), e
        Tk = _rand_pose(rng)
        e, _, _ = SR.between(Tk, Tk @ D, D)
        assert np.abs(e).max() <= 16 * 2.0 ** -53 * max(1.0, np.abs(Tk[:3, 3]).max()), e
    assert SR.transform(SR.UNSET)[0] is False


def _random_system(rng, N, broken=()):
    """Blocks of a random window: PD row blocks, random factors; `broken` steps have none."""
    acc = np.zeros((N, 28))
    for k in range(N):
        M = rng.normal(0, 1, (40, 7)) * np.array([3, 3, 3, 1, 1, 1, 0.01])
        acc[k] = RR.np_acc28(M)
    has = np.array([0 if k in broken else 1 for k in range(max(N - 1, 0))], np.int32)
    fe = rng.normal(0, 0.01, (max(N - 1, 0), 6)) * has[:, None]
    fJ = rng.normal(0, 1, (max(N - 1, 0), 2, 6, 6)) * has[:, None, None, None]
    return acc, has, fe, fJ


@pytest.mark.parametrize("N,broken", [(1, ()), (2, ()), (7, (3,)), (65, ())])
def test_solve_and_marginals_against_numpy(N, broken):
    rng = np.random.default_rng(100 + N)
    acc, has, fe, fJ = _random_system(rng, N, broken)
    pe, pJ = (rng.normal(0, 0.01, 6), rng.normal(0, 1, (6, 6))) if N == 7 else (None, None)
    Hd, Ho, g = SR.assemble(acc, has, fe, fJ, 1e-3, pe, pJ)
    Hm, gm = SR.dense(Hd, Ho, g)
    Hn, gn = SR.np_system(acc, has, fe, fJ, 1e-3, pe, pJ)
    np.testing.assert_allclose(Hm, Hn, rtol=0, atol=1e-12 * np.abs(Hn).max())
    np.testing.assert_allclose(gm, gn, rtol=0, atol=1e-12 * np.abs(gn).max())
    for k in broken:
        assert not Ho[k].any()
    bad, x = SR.solve(Hd, Ho, g, has)
    assert bad == -1
    xn = -np.linalg.solve(Hm, gm)
    bound = SR.solve_bound(Hm, xn)
    print(N, "solve:", np.linalg.norm(x.reshape(-1) - xn), "bound", bound)
    assert np.linalg.norm(x.reshape(-1) - xn) <= bound
    bad, S = SR.marginals(Hd, Ho, has)
    assert bad == -1
    Hi = np.linalg.inv(Hm)
    for k in range(N):
        blk = Hi[6 * k:6 * k + 6, 6 * k:6 * k + 6]
        assert np.linalg.norm(S[k] - blk) <= SR.solve_bound(Hm, blk), k


def test_solve_reports_the_block_that_is_not_pd():
    rng = np.random.default_rng(9)
    acc, has, fe, fJ = _random_system(rng, 4, broken=(1,))
    acc[2:] = 0  # views 2, 3 see nothing and only one factor ties them: their segment has a gauge
    Hd, Ho, g = SR.assemble(acc, has, fe * 0, fJ, 0.0)
    bad, _ = SR.solve(Hd, Ho, g, has)
    assert bad == 3
    assert SR.marginals(Hd, Ho, has)[0] == 3


def test_prior_covariance_is_checked():
    T = np.eye(4)
    assert SR.prior(T, T, np.eye(6))[0]
    assert not SR.prior(T, T, np.zeros((6, 6)))[0]
    bad = np.eye(6)
    bad[2, 2] = np.nan
    assert not SR.prior(T, T, bad)[0]
    # whitening: sigma_row L_c^-1 with Cov = L_c L_c^T
    rng = np.random.default_rng(2)
    A = rng.normal(0, 1, (6, 6))
    cov = A @ A.T + 0.1 * np.eye(6)
    T0 = synth.random_base_pose(rng)
    Tp = T0 @ _noise(rng)
    ok, e, J = SR.prior(T0, Tp, cov, 0.5)
    ok1, e1, J1 = SR.prior(T0, Tp, np.eye(6), 1.0)
    Wp = 0.5 * np.linalg.inv(np.linalg.cholesky(cov))
    np.testing.assert_allclose(e, Wp @ e1, rtol=0, atol=1e-12)
    np.testing.assert_allclose(J, Wp @ J1, rtol=0, atol=1e-12)


def _frames_of(sc, views):
    return [sc["frames"][k] for k in views]


def test_seq_replayed_against_the_dense_system(lm, blind5):
    """Every pass of hc_smooth_seq, from its own recorded poses, accumulators and factors: the factors again
    from the numpy residual, the step from numpy's dense solve of the stacked normal system, the figures."""
    X, nw, nr, ng = lm
    sc = blind5
    p = SR.default_params(lambda_=1e-6)
    T0 = SR.starts(sc)
    mo = SR.noisy_motions(sc, 0.002, 0.005)
    cov = np.diag([1e-4] * 3 + [1e-4] * 3)
    o = SR.seq(T0, mo, sc["ext"], sc["frames"], X, nw, nr, ng, p, prior_T=sc["Twb"][0], prior_cov=cov)
    r = o.res
    assert o.ok and r.status == 0 and r.iterations_run == 4 and r.n_factors == 4 and r.has_prior == 1
    wt, wr = p.sigma_row / p.sigma_t, p.sigma_row / p.sigma_rot
    s6 = np.array([wt] * 3 + [wr] * 3)
    Ds = [SR.transform(m)[1] for m in mo]
    assert np.array_equal(o.T[0], T0)
    for q in range(r.iterations_run + 1):
        for k in range(4):
            np.testing.assert_allclose(o.e[q, k], s6 * SR.np_between(o.T[q, k], o.T[q, k + 1], Ds[k]), rtol=0, atol=1e-12)
        ok, pe, pJ = SR.prior(o.T[q, 0], sc["Twb"][0], cov, p.sigma_row)
        assert np.array_equal(pe, o.pe[q]) and np.array_equal(pJ, o.pJ[q])
        n, nf, rms, mrms, cost = SR.sums(o.n[q], o.acc[q], [1] * 4, o.e[q], p.sigma_row, o.pe[q])
        rtr, ete = o.acc[q][:, 27].sum(), (o.e[q] ** 2).sum()
        assert (n, nf) == (r.n_obs[q], 4) == (int(o.n[q].sum()), 4)
        assert (rms, mrms, cost) == (r.rms[q], r.motion_rms[q], r.cost[q])
        np.testing.assert_allclose([rms, mrms, cost], [math.sqrt(rtr / n), math.sqrt(ete / 24) / p.sigma_row,
                                                       rtr + ete + (o.pe[q] ** 2).sum()], rtol=1e-12)
        if q == r.iterations_run:
            break
        Hn, gn = SR.np_system(o.acc[q], [1] * 4, o.e[q], o.J[q], p.lambda_, o.pe[q], o.pJ[q])
        xn = -np.linalg.solve(Hn, gn)
        assert np.linalg.norm(o.delta[q].reshape(-1) - xn) <= max(1e-12, SR.solve_bound(Hn, xn)), q
        for k in range(5):
            np.testing.assert_allclose(o.T[q + 1, k], RR.exp_right(o.T[q, k], o.delta[q, k]), rtol=0, atol=1e-12)
    assert np.array_equal(o.poses, o.T[r.iterations_run])
    # the gate and the covariances: the dense inverse of the final system at lambda = 0
    fp = r.iterations_run
    Hn, _ = SR.np_system(o.acc[fp], [1] * 4, o.e[fp], o.J[fp], 0.0, o.pe[fp], o.pJ[fp])
    assert r.dof == r.n_obs[fp] + 24 + 6 - 30 and r.smoothed == 1
    assert r.sigma2 == r.cost[fp] / r.dof
    Hi = np.linalg.inv(Hn)
    for k in range(5):
        B = np.eye(6)
        B[:3, :3] = o.poses[k][:3, :3]
        ref = r.sigma2 * B @ Hi[6 * k:6 * k + 6, 6 * k:6 * k + 6] @ B.T
        cov_k = np.array(o.views[k].covariance).reshape(6, 6)
        np.testing.assert_allclose(cov_k, ref, rtol=0, atol=1e-8 * np.abs(ref).max())
        assert np.array_equal(cov_k, cov_k.T)
    # hc_smooth_conclude on its own, from blocks assembled out of the final pass's record: the call's own bytes,
    # and the gates: max_rms below the final rms, or min_obs above the window's rows, clear `smoothed`
    Hd, Ho, _ = SR.assemble(o.acc[fp], [1] * 4, o.e[fp], o.J[fp], 0.0, o.pe[fp], o.pJ[fp])
    rc, covs = SR.conclude(Hd, Ho, [1] * 4, p.min_obs, p.max_rms, r, o.poses)
    assert (rc.smoothed, rc.dof, rc.sigma2) == (1, r.dof, r.sigma2)
    assert covs.tobytes() == np.array([np.array(v.covariance) for v in o.views]).tobytes()
    rc, covs = SR.conclude(Hd, Ho, [1] * 4, p.min_obs, 0.5 * r.rms[fp], r, o.poses)
    assert rc.smoothed == 0 and not covs.any()
    rc, covs = SR.conclude(Hd, Ho, [1] * 4, r.n_obs[fp] + 1, p.max_rms, r, o.poses)
    assert rc.smoothed == 0 and not covs.any()
    Hz = Hd.copy()
    Hz[2] = 0.0  # a block that is not positive definite
    rc, covs = SR.conclude(Hz, Ho, [1] * 4, p.min_obs, p.max_rms, r, o.poses)
    assert rc.smoothed == 0 and not covs.any()


def test_one_view_is_the_refinement(lm, blind5):
    """N = 1 without a prior: pose, n_obs, rms and delta of hc_refine_seq, byte for byte."""
    X, nw, nr, ng = lm
    sc = blind5
    T0 = RR.shift(sc["Twb"][0])
    for lam in (0.0, 1e-4):
        o = SR.seq([T0], None, sc["ext"], [sc["frames"][0]], X, nw, nr, ng, SR.default_params(lambda_=lam))
        ref = RR.seq(T0, sc["ext"], sc["frames"][0], X, nw, nr, ng, RR.default_params(lambda_=lam))
        r = o.res
        assert (r.status, r.iterations_run, r.n_factors, r.n_views) == (ref.status, ref.iterations_run, 0, 1)
        assert np.array_equal(np.array(o.views[0].T_w_b), np.array(ref.T_w_b))
        assert list(r.n_obs) == list(ref.n_obs) and list(r.rms) == list(ref.rms)
        assert list(r.motion_rms) == [0.0] * 11
        for q in range(r.iterations_run):
            assert np.array_equal(o.delta[q, 0], np.array(ref.delta[q]))
        assert r.smoothed == ref.refined == 1 and r.dof == r.n_obs[4] - 6
        hcov = np.array(ref.covariance)
        np.testing.assert_allclose(np.array(o.views[0].covariance), hcov, rtol=0, atol=1e-8 * np.abs(hcov).max())


def test_a_broken_chain_is_its_segments(lm):
    """Five views whose step 2 is unset against the two windows of its segments: poses to 1e-12."""
    X, nw, nr, ng = lm
    sc = SR.trajectory(5, n_cams=2, w=322, h=242, cfg=19)
    p = SR.default_params()
    T0 = SR.starts(sc)
    mo = SR.noisy_motions(sc, 0.002, 0.005)
    mo[2] = SR.UNSET
    o = SR.seq(T0, mo, sc["ext"], sc["frames"], X, nw, nr, ng, p)
    a = SR.seq(T0[:3], mo[:2], sc["ext"], _frames_of(sc, [0, 1, 2]), X, nw, nr, ng, p)
    b = SR.seq(T0[3:], mo[3:], sc["ext"], _frames_of(sc, [3, 4]), X, nw, nr, ng, p)
    assert o.res.status == a.res.status == b.res.status == 0 and o.res.n_factors == 3
    assert not o.e[:, 2].any() and not o.J[:, 2].any()
    np.testing.assert_allclose(o.poses[:3], a.poses, rtol=0, atol=1e-12)
    np.testing.assert_allclose(o.poses[3:], b.poses, rtol=0, atol=1e-12)
    assert o.res.n_obs[4] == a.res.n_obs[4] + b.res.n_obs[4]


def test_no_iterations_return_the_input(lm, blind5):
    X, nw, nr, ng = lm
    sc = blind5
    T0 = SR.starts(sc)
    o = SR.seq(T0, SR.exact_motions(sc), sc["ext"], sc["frames"], X, nw, nr, ng, SR.default_params(iterations=0))
    assert o.res.status == 0 and o.res.iterations_run == 0
    assert o.poses.tobytes() == T0.tobytes()
    assert o.res.n_obs[0] > 0 and o.views[2].n_obs == 0


def test_starved_and_singular_windows(lm, blind5):
    X, nw, nr, ng = lm
    sc = blind5
    black = [[np.zeros_like(f) for f in fr] for fr in sc["frames"][:3]]
    T0 = SR.starts(sc)[:3]
    mo = SR.exact_motions(sc)[:2]
    o = SR.seq(T0, mo, sc["ext"], black, X, nw, nr, ng, SR.default_params())
    r = o.res
    assert (r.status, r.smoothed, r.iterations_run, r.n_obs[0]) == (SR.STATUS["starved"], 0, 0, 0)
    assert o.poses.tobytes() == T0.tobytes() and not np.array(o.views[0].covariance).any()
    # an all-blind segment at lambda = 0: views 1, 2 are cut off from the sighted view 0 and see nothing
    fr = [sc["frames"][0], black[1], black[2]]
    mo2 = mo.copy()
    mo2[0] = SR.UNSET
    o = SR.seq(T0, mo2, sc["ext"], fr, X, nw, nr, ng, SR.default_params())
    r = o.res
    assert (r.status, r.smoothed, r.iterations_run) == (SR.STATUS["singular"], 0, 0)
    assert r.n_obs[0] == o.views[0].n_obs > 0 and o.poses.tobytes() == T0.tobytes()
    assert not np.array(o.views[1].covariance).any()
    # the same window with a damping term solves: lambda holds the gauge
    o = SR.seq(T0, mo2, sc["ext"], fr, X, nw, nr, ng, SR.default_params(lambda_=1e-3))
    assert o.res.status == 0 and o.res.iterations_run == 4 and o.res.smoothed == 0  # lambda = 0 blocks: not PD


def test_the_blind_view_is_recovered(lm, blind5):
    """The accuracy scene with exact motions. The inputs first: per-view refinement leaves the four sighted
    views refined and view 2 STARVED. Then the smoother: view 2 within a quarter of its start error in
    translation and in angle, each sighted view within 0.01 cm of its own refinement."""
    X, nw, nr, ng = lm
    sc = blind5
    T0 = SR.starts(sc)
    own = [RR.seq(T0[k], sc["ext"], sc["frames"][k], X, nw, nr, ng, RR.default_params()) for k in range(5)]
    for k in (0, 1, 3, 4):
        assert own[k].status == 0 and own[k].refined == 1, k
    assert own[2].status == SR.STATUS["starved"] and np.array_equal(np.array(own[2].T_w_b).reshape(4, 4), T0[2])
    o = SR.seq(T0, SR.exact_motions(sc), sc["ext"], sc["frames"], X, nw, nr, ng, SR.default_params())
    r = o.res
    assert (r.status, r.smoothed, r.iterations_run, r.n_factors) == (0, 1, 4, 4)
    s_t, s_a = RR.pose_dist(T0[2], sc["Twb"][2])
    e_t, e_a = RR.pose_dist(o.poses[2], sc["Twb"][2])
    print(f"blind view: start {s_t * 100:.3f} cm / {s_a:.3f} deg, smoothed {e_t * 100:.4f} cm / {e_a:.4f} deg; "
          f"motion_rms {r.motion_rms[4]:.4f}")
    assert e_t <= 0.25 * s_t and e_a <= 0.25 * s_a
    for k in (0, 1, 3, 4):
        d_t, _ = RR.pose_dist(o.poses[k], np.array(own[k].T_w_b).reshape(4, 4))
        print(f"view {k}: own refinement {RR.pose_dist(np.array(own[k].T_w_b).reshape(4, 4), sc['Twb'][k])[0] * 100:.4f} cm, "
              f"smoothed {RR.pose_dist(o.poses[k], sc['Twb'][k])[0] * 100:.4f} cm, apart {d_t * 100:.4f} cm")
        assert d_t <= 1e-4, k
    # the blind view's covariance says what holds it: wider than its neighbours', far tighter than nothing
    c2 = np.array(o.views[2].covariance).reshape(6, 6)
    c1 = np.array(o.views[1].covariance).reshape(6, 6)
    assert np.all(np.diag(c2) > np.diag(c1)) and np.all(np.diag(c2) > 0)


def test_noisy_odometry_limits_the_blind_view(lm, blind5):
    """The same scene with the motions perturbed at the stated sigmas: the blind view's error is set by the
    odometry and is only printed; the sighted views stay on their own refinements."""
    X, nw, nr, ng = lm
    sc = blind5
    T0 = SR.starts(sc)
    o = SR.seq(T0, SR.noisy_motions(sc), sc["ext"], sc["frames"], X, nw, nr, ng, SR.default_params())
    assert o.res.status == 0 and o.res.smoothed == 1
    e_t, e_a = RR.pose_dist(o.poses[2], sc["Twb"][2])
    print(f"blind view with odometry noise (1 cm, 0.03 rad): {e_t * 100:.3f} cm / {e_a:.3f} deg; "
          f"motion_rms {o.res.motion_rms[4]:.3f}")
    for k in (0, 1, 3, 4):
        own = RR.seq(T0[k], sc["ext"], sc["frames"][k], X, nw, nr, ng, RR.default_params())
        d_t, _ = RR.pose_dist(o.poses[k], np.array(own.T_w_b).reshape(4, 4))
        print(f"view {k}: apart from its own refinement {d_t * 100:.4f} cm")
        assert d_t <= 1e-3, k  # 0.1 cm: the rows' weight against a 1 cm odometry sigma, not a tuned figure
