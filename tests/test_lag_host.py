"""The fixed-lag window's rules on the CPU (mk_smooth.h through the host build):
the Schur complement against a dense solve of the whole system, the prior it
leaves (symmetry, whitener, frame), every drop reason by its own input, the
smallest window, and a whole push sequence replayed on host frames.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _lag_ref as LR
import _refine_ref as RR
import _smooth_ref as SR

EPS = 2.0 ** -53
SIGMA_ROW = 0.00127


@pytest.fixture(scope="module")
def lm(landmark_map):
    return RR.all_landmarks(landmark_map)


def _system(N, with_prior, seed):
    """A random SPD block-tridiagonal system in the smoother's own terms: accumulators (N x 28), whitened
    factors on every step, optionally a prior term on view 0."""
    rng = np.random.default_rng(seed)
    acc = np.zeros((N, 28))
    for k in range(N):
        M = rng.normal(size=(12, 6))
        A = M.T @ M
        acc[k, :21] = A[np.triu_indices(6)]
        acc[k, 21:27] = rng.normal(size=6)
    fe = rng.normal(size=(N - 1, 6))
    fJ = rng.normal(size=(N - 1, 2, 6, 6))
    has = np.ones(N - 1, np.int32)
    pe = rng.normal(size=6) if with_prior else None
    pJ = rng.normal(size=(6, 6)) if with_prior else None
    return acc, has, fe, fJ, pe, pJ


@pytest.mark.parametrize("N", [2, 3, 7])
@pytest.mark.parametrize("with_prior", [False, True])
def test_schur_complement_against_the_whole_system(N, with_prior):
    """x_1 .. x_N-1 of the system with view 0 marginalised equal those of the whole system to 1e3 eps cond2(H)."""
    for seed in range(5):
        acc, has, fe, fJ, pe, pJ = _system(N, with_prior, 100 * N + seed)
        Hd, Ho, g = SR.assemble(acc, has, fe, fJ, 0.0, pe, pJ)
        Hm, gm = SR.dense(Hd, Ho, g)
        whole = -np.linalg.solve(Hm, gm)
        why, Lam, eta = LR.schur(Hd[0], g[0], fJ[0, 0], fJ[0, 1], fe[0])
        assert why == 0
        assert np.array_equal(Lam, Lam.T), "Lambda is symmetric bit for bit"
        # views 1 .. N - 1 alone: factor 0's terms are gone from view 1's blocks, Lambda and eta take their place
        has1 = has[1:]
        Hd1, Ho1, g1 = SR.assemble(acc[1:], has1 if N > 2 else np.zeros(0, np.int32), fe[1:], fJ[1:], 0.0)
        Hd1[0] += Lam
        g1[0] += eta
        Hr, gr = SR.dense(Hd1, Ho1, g1)
        reduced = -np.linalg.solve(Hr, gr)
        bound = 1e3 * EPS * np.linalg.cond(Hm) * np.linalg.norm(whole)
        assert np.abs(reduced - whole[6:]).max() <= bound, (N, with_prior, seed, np.abs(reduced - whole[6:]).max(), bound)


def _pose(rng):
    T = np.eye(4)
    T[:3, :3] = SR.np_exp(rng.normal(0, 0.6, 3))
    T[:3, 3] = rng.normal(0, 1.0, 3)
    return T


def test_prior_covariance_and_whitener():
    """Cov_p is symmetric bit for bit, equals sigma_row^2 B Lambda^-1 B^T, and its whitener gives W^T W Cov_p =
    sigma_row^2 I to 1e3 eps cond2."""
    rng = np.random.default_rng(3)
    for seed in range(8):
        acc, has, fe, fJ, pe, pJ = _system(3, seed % 2 == 1, 500 + seed)
        Hd, Ho, g = SR.assemble(acc, has, fe, fJ, 0.0, pe, pJ)
        T1 = _pose(rng)
        why, Tp, Cov, Wp = LR.marginalize(Hd[0], g[0], fJ[0, 0], fJ[0, 1], fe[0], T1, SIGMA_ROW)
        assert why == 0
        assert np.array_equal(Cov, Cov.T)
        _, Lam, eta = LR.schur(Hd[0], g[0], fJ[0, 0], fJ[0, 1], fe[0])
        B = np.eye(6)
        B[:3, :3] = Tp[:3, :3]
        ref = SIGMA_ROW ** 2 * B @ np.linalg.inv(Lam) @ B.T
        cond = np.linalg.cond(Lam)
        assert np.abs(Cov - ref).max() <= 1e3 * EPS * cond * np.abs(ref).max()
        ok, W2 = LR.whitener(Cov, SIGMA_ROW)
        assert ok and np.array_equal(W2, Wp), "the device's whitener is the batch call's"
        assert np.array_equal(Wp, np.tril(Wp))
        dev = Wp.T @ Wp @ Cov / SIGMA_ROW ** 2 - np.eye(6)
        assert np.abs(dev).max() <= 1e3 * EPS * cond, (np.abs(dev).max(), cond)
        # T_p = T_1 D(x*), x* = -Lambda^-1 eta
        x = -np.linalg.solve(Lam, eta)
        np.testing.assert_allclose(Tp, RR.exp_right(T1, x), rtol=0, atol=1e3 * EPS * cond * max(1.0, np.abs(x).max()))


def test_frame_of_the_prior():
    """The prior factor evaluated at T_1 reads e_p = -(x* with its translation turned to the world frame) to
    first order. The turn is by R of T_p where T_1's would be exact: |(R_p - R_1) x_t| <= |x_r| |x_t| <= |x*|^2 /
    2, and the rotation part is exact (log(Exp(-x_r)) = -x_r), so the bound is |x*|^2 (constant 1; the largest
    ratio seen over these systems is printed) plus the rounding of a pose product."""
    rng = np.random.default_rng(9)
    worst = 0.0
    for seed in range(12):
        acc, has, fe, fJ, pe, pJ = _system(2, seed % 2 == 1, 900 + seed)
        fe *= 0.05 * (1 + seed)  # steps from a few millimetres to a good fraction of a radian
        acc[:, 21:27] *= 0.05 * (1 + seed)
        Hd, Ho, g = SR.assemble(acc, has, fe, fJ, 0.0, pe, pJ)
        T1 = _pose(rng)
        why, Tp, Cov, Wp = LR.marginalize(Hd[0], g[0], fJ[0, 0], fJ[0, 1], fe[0], T1, SIGMA_ROW)
        assert why == 0
        _, Lam, eta = LR.schur(Hd[0], g[0], fJ[0, 0], fJ[0, 1], fe[0])
        x = -np.linalg.solve(Lam, eta)
        if np.linalg.norm(x[3:]) > 2.0:
            continue
        turned = np.concatenate([Tp[:3, :3] @ x[:3], x[3:]])
        ep = SR.np_prior(T1, Tp)
        err = np.abs(ep + turned).max()
        n2 = float(x @ x)
        worst = max(worst, err / n2)
        assert err <= n2 + 1e-12 * (1 + np.abs(x).max()), (seed, err, n2)
    print(f"frame of the prior: largest |e_p + turned x*| / |x*|^2 = {worst:.3f}")
    assert worst > 0


def test_numeric_drop_reasons():
    """H_00, Lambda and Cov_p each refused by its own input; what is left is a zero whitener."""
    I6 = np.eye(6)
    z = np.zeros(6)
    T1 = np.eye(4)
    cases = [
        ("h00", -I6, I6, I6),
        ("h00", np.full((6, 6), np.nan), I6, I6),
        ("lambda", 0.5 * I6, I6, I6),  # H_00 below Ja^T Ja: Lambda = I - 2 I
        ("cov", 2.0 * I6, I6, 1e-160 * I6),  # Lambda ~ 5e-321: its inverse overflows
    ]
    for name, H00, Ja, Jb in cases:
        why, Tp, Cov, Wp = LR.marginalize(H00, z, Ja, Jb, z, T1, SIGMA_ROW)
        assert why == LR.DROPS[name], (name, why)
        assert np.array_equal(Tp, np.eye(4)) and not Cov.any() and not Wp.any()
    why, Tp, Cov, Wp = LR.marginalize(2.0 * I6, z, I6, I6, z, T1, SIGMA_ROW)
    assert why == 0 and np.array_equal(Tp, T1)
    np.testing.assert_allclose(Cov, SIGMA_ROW ** 2 * 2.0 * I6, rtol=1e-15)


def test_predicted_start_is_the_plain_product():
    rng = np.random.default_rng(4)
    T, D = _pose(rng), SR.step()
    np.testing.assert_allclose(LR.predict(T, D), T @ D, rtol=0, atol=4 * EPS * 4)
    assert np.array_equal(LR.predict(T, D)[3], [0, 0, 0, 1])


def test_sizes():
    import mantis_amd as M

    L = LR.hc()
    assert L.hc_sizeof_lag_params() == C.sizeof(M.MantisLagParams)
    assert L.hc_sizeof_lag_info() == C.sizeof(M.MantisLagInfo)


@pytest.fixture(scope="module")
def walk6():
    return SR.trajectory(6, n_cams=1, w=LR.SW, h=LR.SH, cfg=19)


def _pushes(sc, noise=(0.002, 0.005)):
    n = len(sc["frames"])
    mo = np.concatenate([np.zeros((1, 7)), SR.noisy_motions(sc, *noise)])
    return [SR.starts(sc)[k] for k in range(n)], mo


def _same(a, b):
    return bytes(a) == bytes(b)


def test_capacity_two_and_each_push_is_a_batch_call(lm, walk6):
    """Capacity 2 over six views: every push is hc_smooth_seq over the views held, from the poses held, with the
    prior the sequence reports; every slide carries a prior."""
    X, nw, nr, ng = lm
    sc = walk6
    starts, mo = _pushes(sc)
    p = SR.default_params(iterations=2)
    lag = LR.seq(2, sc["frames"], starts, mo, sc["ext"], X, nw, nr, ng, p)
    assert lag.ok
    for q in range(6):
        n, hp, why, slid = lag.info[q]
        assert (n, slid) == (min(q + 1, 2), int(q >= 2))
        assert lag.res[q].status == 0 and why == 0 and hp == int(q >= 2)
        lo = q + 1 - n
        T_in = [LR.pose_of(v) for v in lag.views[q - 1][-(n - 1):]] if n > 1 else []
        T_in.append(starts[q])
        ref = SR.seq(np.array(T_in), mo[lo + 1:q + 1], sc["ext"], sc["frames"][lo:q + 1], X, nw, nr, ng, p,
                     lag.prior_T[q] if hp else None, lag.prior_cov[q] if hp else None)
        assert _same(ref.res, lag.res[q]), q
        assert all(_same(a, b) for a, b in zip(ref.views, lag.views[q])), q


def test_sequence_drop_reasons(lm, walk6):
    """No factor on the step that becomes step 0, and a window that did not end OK: each leaves no prior."""
    X, nw, nr, ng = lm
    sc = walk6
    starts, mo = _pushes(sc)
    p = SR.default_params(iterations=2)
    mo2 = mo.copy()
    mo2[1] = SR.UNSET
    lag = LR.seq(3, sc["frames"][:5], starts[:5], mo2[:5], sc["ext"], X, nw, nr, ng, p)
    assert lag.ok
    assert [tuple(r) for r in lag.info[:, 1:]] == [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, LR.DROPS["no_factor"], 1),
                                                   (1, 0, 1)]
    black = [[np.zeros_like(f) for f in fr] for fr in sc["frames"]]
    frames = black[:2] + sc["frames"][2:5]
    lag = LR.seq(2, frames, starts[:5], mo[:5], sc["ext"], X, nw, nr, ng, p)
    assert [r.status for r in lag.res] == [1, 1, 0, 0, 0]
    info = [tuple(int(v) for v in r) for r in lag.info[:, 1:]]
    assert info[:3] == [(0, 0, 0), (0, 0, 0), (0, LR.DROPS["not_ok"], 1)] and info[4] == (1, 0, 1)
    # push 3 marginalises a black view that had no prior of its own: H_00 = Ja^T Ja, so Lambda is zero but for
    # rounding. Either it is refused, or what is carried weighs nothing (a standard deviation above a metre)
    hp, why, slid = info[3]
    assert slid == 1 and ((hp, why) in [(0, LR.DROPS["lambda"]), (0, LR.DROPS["cov"])] or
                          (hp == 1 and np.linalg.eigvalsh(lag.prior_cov[3]).min() > 1.0)), info[3]
    # a missing start where one is required
    assert not LR.seq(2, sc["frames"][:2], [None, None], mo[:2], sc["ext"], X, nw, nr, ng, p).ok
    assert not LR.seq(2, sc["frames"][:2], [starts[0], None], np.zeros((2, 7)), sc["ext"], X, nw, nr, ng, p).ok


@pytest.mark.parametrize("noisy", [False, True])
def test_replay_of_the_accuracy_scene(lm, noisy):
    """hc_lag_seq over the accuracy scene (twelve one-camera views, capacity 4, views 5 and 6 black), with exact
    motions and with motions off by the default sigmas: every window ends OK and carries a prior from the first
    slide on, every push is hc_smooth_seq over the views held with the prior reported, and the three distances
    per push (lag to H, T to H, lag to T) are printed."""
    X, nw, nr, ng = lm
    sc = LR.accuracy_scene()
    mo = LR.accuracy_motions(sc, noisy)
    lag, table = LR.accuracy_host(sc, mo, X, nw, nr, ng)
    assert lag.ok and [r.status for r in lag.res] == [0] * LR.ACC_VIEWS
    assert [tuple(r) for r in lag.info] == [(min(q + 1, 4), int(q >= 4), 0, int(q >= 4)) for q in range(LR.ACC_VIEWS)]
    p = SR.default_params(iterations=LR.ACC_ITERATIONS)
    q = 8  # the window the black run leads
    T_in = [LR.pose_of(v) for v in lag.views[q - 1][1:]]
    T_in.append(LR.predict(T_in[-1], SR.transform(mo[q])[1]))
    ref = SR.seq(np.array(T_in), mo[q - 2:q + 1], sc["ext"], sc["frames"][q - 3:q + 1], X, nw, nr, ng, p, lag.prior_T[q],
                 lag.prior_cov[q])
    assert _same(ref.res, lag.res[q]) and all(_same(a, b) for a, b in zip(ref.views, lag.views[q]))
    for q, (dl, dt, dlt, black) in table.items():
        print(f"push {q}{' *' if black else ''}: lag-H {dl:.3e}  T-H {dt:.3e}  lag-T {dlt:.3e}")
    # where the black run leads the window, the prior is what holds it
    dl, dt, _, black = table[8]
    assert black and dl < dt
