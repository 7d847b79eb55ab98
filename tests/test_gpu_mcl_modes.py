"""The modes of the Monte Carlo localization set on the GPU
(mantis_mcl_init_lattice / mantis_mcl_modes / mantis_mcl_select_mode) against
their definition (include/mantis.h): k_mcl_modes' answer against the Python
restatement of test_mcl_modes_host on the step's own record, k_mcl_keep's
log-weights against the Python key of every particle, the lattice seeding
against mantis_mcl_init. The 1280x720 three-camera ring scene of test_gpu_mcl.
"""
import ctypes as C
import math

import numpy as np
import pytest

import test_mcl_modes_host as MMH
from mantis_amd import synth
from test_gpu_mcl import CAMS, TAU, _cloud, _images, _rand, mantis, scene  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-9
G = 0.32
OK, ERR_ARG, ERR_STATE = 0, 1, 5
TRUTH, PLUS_X, MINUS_Y, YAW90, OUTSIDE, FLOOR = range(6)
KW = dict(sigma_rot=0.0, sigma_t=0.0, tau=TAU, resample_frac=0.0, record=1, min_projections=1)


def _clusters(scene, N):
    """(poses [N, 4, 4], cluster of each): the truth, one cell off in +x, one
    in -y, the truth yawed 90 degrees in place, two particles 8 cells away and
    some under the floor (three cells off, so that they share no bin with the
    others); beyond the first seven the four scoring clusters in turn with a
    jitter well inside a cell."""
    T0 = scene["Twb"]

    def member(kind, j):
        T = T0.copy()
        if kind == PLUS_X:
            T[0, 3] += G
        elif kind == MINUS_Y:
            T[1, 3] -= G
        elif kind == YAW90:
            T[:3, :3] = synth.rot_z(math.pi / 2) @ T0[:3, :3]
        elif kind == OUTSIDE:
            T[j % 2, 3] += 8 * G if j % 2 == 0 else -8 * G
        elif kind == FLOOR:
            T[2, 3] -= 10.0
            T[1, 3] += 3 * G
        return T

    first = [TRUTH, PLUS_X, MINUS_Y, YAW90, OUTSIDE, OUTSIDE, FLOOR]
    rng = np.random.default_rng(300 + N)
    kinds = np.zeros(N, np.int64)
    T = np.zeros((N, 4, 4))
    for j in range(N):
        kinds[j] = first[j] if j < 7 else (FLOOR if j % 16 == 15 else (TRUTH, PLUS_X, MINUS_Y, YAW90)[j % 4])
        T[j] = member(kinds[j], j)
        if j >= 7:
            T[j] = T[j] @ _rand(rng.normal(size=6), 0.005, 0.005)
    return T, kinds


def _stepped(mantis, scene, N, all_score=True, **over):
    """The constructed set after one step on camera 0: (kinds, step result, record)."""
    T, kinds = _clusters(scene, N)
    mantis.rng_state = 1
    mantis.mcl_init_particles(T, **{**KW, **over})
    _, mo = mantis.mcl_step(_images(scene, CAMS[:1]))
    rec = mantis.mcl_record()
    assert mo.lost == 0 and np.array_equal(rec["T_pred"], T)
    for kind in set(kinds.tolist()) if all_score else ():  # every cluster scores, but the one under the floor
        assert np.any(rec["q"][kinds == kind] > 0) == (kind != FLOOR), kind
    assert np.all(rec["q"][kinds == FLOOR] == 0) and np.all(rec["counts"][kinds == FLOOR] == 0)
    return kinds, mo, rec


def _keys(T, A):
    return np.array([MMH.py_cell_key(T[j], A, G)[:3] for j in range(len(T))])


def _mode_key(m):
    return (m.ix, m.iy, m.yaw_quadrant)


def _status_modes(mantis, max_modes, out):
    import mantis_amd as M

    return M.lib().mantis_mcl_modes(mantis.h, max_modes, None if out is None else C.byref(out))


@pytest.mark.parametrize("N", [1, 7, 257, 4096])
def test_modes_of_a_constructed_set(mantis, scene, N):
    kinds, mo, rec = _stepped(mantis, scene, N)
    got = mantis.mcl_modes(8)
    ref = MMH.py_modes(rec["T_pred"], rec["q"], rec["sums"], rec["counts"], mo.best, 8, G)
    MMH.check_modes(got, ref, 8)
    assert got.weight_sum == mo.weight_sum and got.n_modes == min(4, N)
    assert np.array_equal(np.array(got.anchor_T_w_b).reshape(4, 4), rec["T_pred"][mo.best])
    assert got.n_outside == min(2, max(N - 4, 0)) and got.n_cells == got.n_modes
    assert got.mode[0].best == mo.best and got.mode[0].best_error == mo.best_error
    assert sum(got.mode[i].weight for i in range(got.n_modes)) + got.outside_weight == got.weight_sum
    for mm in (1, 3):  # prefixes of the answer
        part = mantis.mcl_modes(mm)
        assert part.n_modes == min(mm, got.n_modes)
        assert (part.n_cells, part.n_outside, part.weight_sum, part.outside_weight) == (
            got.n_cells, got.n_outside, got.weight_sum, got.outside_weight)
        assert bytes(part.anchor_T_w_b) == bytes(got.anchor_T_w_b)
        for i in range(8):
            if i < part.n_modes:
                assert bytes(part.mode[i]) == bytes(got.mode[i]), (mm, i)
            else:
                assert part.mode[i].n == 0 and part.mode[i].best == -1 and part.mode[i].weight == 0


@pytest.mark.parametrize("N", [65, 1025])
def test_one_mode_is_the_steps_estimate(mantis, scene, N):
    mantis.rng_state = 1
    mantis.mcl_init_particles(_cloud(scene, N, 500 + N), sigma_rot=0.01, sigma_t=0.005, tau=TAU, resample_frac=0.0)
    _, mo = mantis.mcl_step(_images(scene))
    got = mantis.mcl_modes(8)
    assert mo.lost == 0 and got.n_modes == 1 and got.n_cells == 1 and got.n_outside == 0
    m = got.mode[0]
    assert m.share == 1.0 and m.n == mo.n_valid and m.weight == mo.weight_sum == got.weight_sum
    assert _mode_key(m) == (0, 0, 0) and m.best == mo.best and m.best_error == mo.best_error
    np.testing.assert_allclose(np.array(m.T_w_b), np.array(mo.T_w_b), atol=POSE_TOL, rtol=0)
    cov = np.array(mo.covariance).reshape(6, 6)
    np.testing.assert_allclose(np.array(m.covariance).reshape(6, 6), cov, atol=1e-9 * np.diag(cov).max(), rtol=0)


def test_state_and_arguments(mantis, scene):
    import mantis_amd as M

    out = M.MantisMclModes()
    T, _ = _clusters(scene, 40)
    imgs = _images(scene, CAMS[:1])
    mantis.mcl_reset()
    assert _status_modes(mantis, 8, out) == ERR_STATE  # no set at all
    mantis.mcl_init_particles(T, **KW)
    assert _status_modes(mantis, 8, out) == ERR_STATE  # no step since the init
    assert "mcl" in M.lib().mantis_last_error(mantis.h).decode()
    mantis.mcl_step(imgs)
    assert _status_modes(mantis, 8, out) == OK and out.n_modes == 4
    for bad in (0, 9, -1):
        assert _status_modes(mantis, bad, out) == ERR_ARG
    assert _status_modes(mantis, 8, None) == ERR_ARG
    mantis.mcl_init_particles(T, **KW)
    assert _status_modes(mantis, 8, out) == ERR_STATE  # a new init forgets the step
    # a lost step (every camera blind, looking straight up from the base): no modes, and no error
    mantis.mcl_init_particles(_cloud(scene, 12, 9), **KW)
    _, mo = mantis.mcl_step(_images(scene, ext=[np.eye(4)] * 8))
    assert mo.lost == 1
    assert _status_modes(mantis, 8, out) == OK
    assert (out.status, out.n_modes, out.n_cells, out.n_outside, out.weight_sum) == (0, 0, 0, 0, 0)
    assert not np.any(np.array(out.anchor_T_w_b)) and out.mode[0].best == -1
    assert M.lib().mantis_mcl_select_mode(mantis.h, 0) == ERR_ARG  # not below n_modes = 0
    # with and without the record: the same bytes; nothing drawn, nothing moved
    res = []
    for record in (1, 0):
        mantis.rng_state = 1
        mantis.mcl_init_particles(T, **{**KW, "sigma_rot": 0.002, "sigma_t": 0.002, "record": record})
        mantis.mcl_step(imgs)
        state, (Tb, Lb) = mantis.rng_state, mantis.mcl_particles()
        res.append(bytes(mantis.mcl_modes(8)))
        Ta, La = mantis.mcl_particles()
        assert mantis.rng_state == state and np.array_equal(Ta, Tb) and np.array_equal(La, Lb)
    assert res[0] == res[1]


def test_select_mode_not_resampled(mantis, scene):
    import mantis_amd as M

    N = 257
    kinds, mo, rec = _stepped(mantis, scene, N)
    got = mantis.mcl_modes(8)
    assert got.n_modes == 4 and mo.resampled == 0
    T, L0 = mantis.mcl_particles()
    state = mantis.rng_state
    keys = _keys(T, np.array(got.anchor_T_w_b).reshape(4, 4))
    keep = np.all(keys == np.array(_mode_key(got.mode[1])), axis=1)
    assert 0 < keep.sum() < N
    mantis.mcl_select_mode(1)
    T1, L1 = mantis.mcl_particles()
    assert np.array_equal(T1, T) and mantis.rng_state == state
    assert np.all(np.isneginf(L1[~keep])) and L1[keep].tobytes() == L0[keep].tobytes()
    assert np.array_equal(mantis.prior_pose, np.array(got.mode[1].T_w_b).reshape(4, 4))
    # a dropped particle stays dropped: the next step weighs the kept ones alone
    assert np.all(rec["q"][keep] > 0) and keep.sum() == got.mode[1].n
    _, mo2 = mantis.mcl_step(_images(scene, CAMS[:1]))
    assert mo2.lost == 0 and mo2.n_valid == int(keep.sum())
    assert np.all(mantis.mcl_record()["q"][~keep] == 0)
    # the modes were the last step's: a new step forgets them
    assert M.lib().mantis_mcl_select_mode(mantis.h, 0) == ERR_STATE


def test_select_mode_resampled(mantis, scene):
    import mantis_amd as M

    L = M.lib()
    N = 257
    kinds, mo, rec = _stepped(mantis, scene, N, resample_frac=2.0)
    assert mo.resampled == 1
    assert L.mantis_mcl_select_mode(mantis.h, 0) == ERR_STATE  # no modes call yet
    got = mantis.mcl_modes(8)
    T, L0 = mantis.mcl_particles()  # the resampled set
    assert np.array_equal(T, rec["T_pred"][rec["ancestors"]]) and np.all(L0 == 0.0)
    keys = _keys(T, np.array(got.anchor_T_w_b).reshape(4, 4))
    keep = np.all(keys == np.array(_mode_key(got.mode[0])), axis=1)
    assert 0 < keep.sum() < N
    assert L.mantis_mcl_select_mode(mantis.h, 8) == ERR_ARG and L.mantis_mcl_select_mode(mantis.h, -1) == ERR_ARG
    assert L.mantis_mcl_select_mode(mantis.h, got.n_modes) == ERR_ARG
    assert np.array_equal(mantis.mcl_particles()[1], L0)
    mantis.mcl_select_mode(0)
    T1, L1 = mantis.mcl_particles()
    assert np.array_equal(T1, T) and np.all(L1[keep] == 0.0) and np.all(np.isneginf(L1[~keep]))
    assert np.array_equal(mantis.prior_pose, np.array(got.mode[0].T_w_b).reshape(4, 4))
    # the next step resamples from the kept mode alone
    _, mo2 = mantis.mcl_step(_images(scene, CAMS[:1]))
    T2, _ = mantis.mcl_particles()
    assert mo2.resampled == 1 and mo2.n_valid == int(keep.sum())
    assert np.all(_keys(T2, np.array(got.anchor_T_w_b).reshape(4, 4)) == np.array(_mode_key(got.mode[0])))


def test_select_mode_without_offspring(mantis, scene):
    """tau small enough that the truth carries all but a sliver of the weight:
    the other modes exist (q > 0) and leave no offspring in the resampling."""
    import mantis_amd as M

    L = M.lib()
    kinds, mo, rec = _stepped(mantis, scene, 7, all_score=False, resample_frac=2.0, tau=800.0)
    assert mo.resampled == 1 and mo.best == 0 and np.all(rec["ancestors"] == mo.best)
    got = mantis.mcl_modes(8)
    assert got.n_modes >= 2 and _mode_key(got.mode[0]) == (0, 0, 0) and got.mode[1].weight > 0
    T, L0 = mantis.mcl_particles()
    prior = mantis.prior_pose.copy()
    assert np.array_equal(prior, np.array(mo.T_w_b).reshape(4, 4))
    assert L.mantis_mcl_select_mode(mantis.h, 1) == ERR_STATE
    assert "mode" in L.mantis_last_error(mantis.h).decode()
    T1, L1 = mantis.mcl_particles()
    assert np.array_equal(T1, T) and L1.tobytes() == L0.tobytes() and np.array_equal(mantis.prior_pose, prior)
    mantis.mcl_select_mode(0)  # the mode that has them all
    assert np.all(mantis.mcl_particles()[1] == 0.0)
    assert np.array_equal(mantis.prior_pose, np.array(got.mode[0].T_w_b).reshape(4, 4))


def test_init_lattice(mantis, scene):
    import mantis_amd as M

    sr0, st0 = 0.2, 0.05
    for N, cells in [(21, (0, 0)), (4096, (1, 2)), (15, (1, 2))]:
        mantis.rng_state = 1
        mantis.mcl_init(scene["Twb"], sr0, st0, n_particles=N, tau=TAU)
        T0, _ = mantis.mcl_particles()
        state = mantis.rng_state
        mantis.rng_state = 1
        mantis.mcl_init_lattice(scene["Twb"], sr0, st0, cells[0], cells[1], n_particles=N, tau=TAU)
        T, Lw = mantis.mcl_particles()
        assert mantis.rng_state == state and len(T) == N and np.all(Lw == 0.0)
        if cells == (0, 0):
            assert np.array_equal(T, T0)
            continue
        w = 2 * cells[0] + 1
        site = np.arange(N) % (w * (2 * cells[1] + 1))
        ix, iy = site % w - cells[0], site // w - cells[1]
        want = T0.copy()
        want[:, 0, 3] = T0[:, 0, 3] + ix.astype(np.float64) * G
        want[:, 1, 3] = T0[:, 1, 3] + iy.astype(np.float64) * G
        assert np.array_equal(T[:, :3, :3], T0[:, :3, :3]) and np.array_equal(T, want)
        assert len(set(zip(ix.tolist(), iy.tolist()))) == 15
    # too few particles for the sites, cells out of range: nothing changes
    T, _ = mantis.mcl_particles()
    state = mantis.rng_state
    Tm = np.ascontiguousarray(scene["Twb"], np.float64)
    for n, cx, cy in [(14, 1, 2), (4096, 8, 0), (4096, 0, 8), (4096, -1, 0)]:
        p = mantis.mcl_params(n_particles=n, tau=TAU)
        assert M.lib().mantis_mcl_init_lattice(mantis.h, Tm.ctypes.data, sr0, st0, cx, cy, C.byref(p)) == ERR_ARG
        assert mantis.rng_state == state and np.array_equal(mantis.mcl_particles()[0], T)
