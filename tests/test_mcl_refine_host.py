"""Monte Carlo localization, the modes refined and the set recentred, host
side: the plan (which modes are applied, the correction of each) and the move
of a particle of mantis_amd/csrc/mk_mcl_refine.h -- the very functions
mantis_mcl_refine_modes and k_mcl_recentre run -- built for the host
(build/libmantis_hostcheck.so hc_mcl_refine_plan / hc_mcl_recentre) against
plain restatements written here, and the equivariance of a mode's mean under
its correction (test_mcl_modes_host.py_modes on the moved set).
"""
import ctypes as C
import math

import numpy as np
import pytest

import _hostcheck as H
import test_mcl_modes_host as MMH
from mantis_amd import synth

G = MMH.G
Q1 = MMH.Q1
POSE_TOL = 1e-9


def _hc():
    L = H.lib()
    vp = C.c_void_p
    L.hc_mcl_refine_plan.argtypes = [vp, C.c_double, vp, vp, C.c_int, vp, vp, vp, vp]
    L.hc_mcl_refine_plan.restype = None
    L.hc_mcl_recentre.argtypes = [vp, C.c_double, vp, vp, C.c_int, vp, C.c_int, vp]
    L.hc_mcl_recentre.restype = None
    return L


# ---------------------------------------------------------- the rules restated
def py_xf_mul(a, b):
    """The plain product of two rigid 4 x 4 (mk_math.h xf_mul's operation order), in Python floats."""
    o = np.eye(4)
    for i in range(3):
        for j in range(3):
            o[i, j] = float(b[0, j]) * float(a[i, 0]) + float(b[1, j]) * float(a[i, 1]) + float(b[2, j]) * float(a[i, 2])
        o[i, 3] = (float(a[i, 0]) * float(b[0, 3]) + float(a[i, 1]) * float(b[1, 3]) + float(a[i, 2]) * float(b[2, 3])) \
            + float(a[i, 3])
    return o


def py_xf_inverse(a):
    o = np.eye(4)
    o[:3, :3] = a[:3, :3].T
    for i in range(3):
        o[i, 3] = float(o[i, 0]) * -float(a[0, 3]) + float(o[i, 1]) * -float(a[1, 3]) + float(o[i, 2]) * -float(a[2, 3])
    return o


def py_plan(modes, T_ref, refined, apply, g=G):
    """(key_kept [8], applied [8], X [8, 4, 4], bins [8]) of a MantisMclModes record."""
    A = np.array(modes.anchor_T_w_b).reshape(4, 4)
    kept, app, bins = np.zeros(8, np.int32), np.zeros(8, np.int32), np.full(8, -1, np.int32)
    X = np.array([np.eye(4)] * 8)
    for k in range(modes.n_modes):
        m = modes.mode[k]
        b = ((m.iy + 7) * 15 + (m.ix + 7)) * 4 + m.yaw_quadrant
        kept[k] = int(bool(refined[k]) and MMH.py_cell_key(T_ref[k], A, g)[3] == b)
        app[k] = int(bool(apply) and kept[k])
        X[k] = py_xf_mul(T_ref[k], py_xf_inverse(np.array(m.T_w_b).reshape(4, 4)))
        if app[k]:
            bins[k] = b
    return kept, app, X, bins


def py_recentre(modes, T_ref, refined, apply, T, g=G):
    """(the moved set, n_moved [8], the mode each particle moved with or -1)."""
    A = np.array(modes.anchor_T_w_b).reshape(4, 4)
    _, _, X, bins = py_plan(modes, T_ref, refined, apply, g)
    out, n, which = T.copy(), np.zeros(8, np.int32), np.full(len(T), -1)
    for j in range(len(T)):
        b = MMH.py_cell_key(T[j], A, g)[3]
        for k in range(modes.n_modes):
            if bins[k] == b:
                out[j] = py_xf_mul(X[k], T[j])
                n[k] += 1
                which[j] = k
    return out, n, which


# ------------------------------------------------------------------ the calls
def plan(modes, T_ref, refined, apply, g=G):
    T_ref = np.ascontiguousarray(T_ref, np.float64)
    refined = np.ascontiguousarray(refined, np.int32)
    assert T_ref.shape == (8, 4, 4) and refined.shape == (8,)
    kept, app, bins = np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros(8, np.int32)
    X = np.zeros((8, 4, 4))
    _hc().hc_mcl_refine_plan(C.addressof(modes), g, T_ref.ctypes.data, refined.ctypes.data, int(apply), kept.ctypes.data,
                             app.ctypes.data, X.ctypes.data, bins.ctypes.data)
    return kept, app, X, bins


def recentre(modes, T_ref, refined, apply, T, g=G):
    T_ref = np.ascontiguousarray(T_ref, np.float64)
    refined = np.ascontiguousarray(refined, np.int32)
    out = np.ascontiguousarray(T, np.float64).copy()
    n = np.zeros(8, np.int32)
    _hc().hc_mcl_recentre(C.addressof(modes), g, T_ref.ctypes.data, refined.ctypes.data, int(apply), out.ctypes.data,
                          len(out), n.ctypes.data)
    return out, n


def _close(got, want):
    """1e-15 relative: the restatement repeats the operation order, so nothing but the last bit may differ."""
    np.testing.assert_allclose(got, want, rtol=1e-15, atol=1e-15 * np.abs(want).max())


def _small(rng, rot=0.007, t=0.012):
    """A rigid motion of about 0.4 degrees and 1.2 cm."""
    a = rng.normal(size=3) * rot
    X = np.eye(4)
    X[:3, :3] = synth.rot_z(a[0]) @ synth.rot_y(a[1]) @ synth.rot_x(a[2])
    X[:3, 3] = rng.normal(size=3) * t
    return X


EDGE = (2, 0, 0)  # the cell of the single particle 1 mm inside its boundary


def _set(rng, N, edge=True):
    """N poses in four clusters (cells (0,0), (1,0), (0,-1) and (0,0) yawed 90
    degrees) with a jitter well inside a cell, a few far outside the range, and
    (edge) one particle alone in cell (2,0), 1 mm inside its +x boundary.
    Particle 0 is the anchor."""
    A = MMH._pose(0.3, (0.11, -0.07), tilt=0.05)
    T = np.zeros((N, 4, 4))
    for j in range(N):
        d = np.eye(4)
        if j:
            a = rng.normal(size=3) * 0.004
            d[:3, :3] = synth.rot_z(a[0]) @ synth.rot_y(a[1]) @ synth.rot_x(a[2])
            d[:3, 3] = rng.normal(size=3) * 0.004
        kind = j % 4
        if kind == 3:
            d[:3, :3] = synth.rot_z(math.pi / 2) @ d[:3, :3]
        T[j] = A @ d
        if kind == 1:
            T[j, 0, 3] += G
        elif kind == 2:
            T[j, 1, 3] -= G
        if j >= 8 and j % 16 == 9:
            T[j, 0, 3] += 8 * G  # outside
    if edge:
        T[5] = A
        T[5, 0, 3] = A[0, 3] + (2 * G + 0.5 * G - 0.001)
    q = rng.integers(1, Q1, N).astype(np.uint64)
    q[rng.random(N) < 0.2] = 0
    q[0] = Q1
    if edge:
        q[5] = 12345
    counts = rng.integers(1, 700, (N, 2)).astype(np.int32)
    sums = counts.astype(np.int64) * rng.integers(20000, 90000, (N, 2))
    return T, q, sums, counts


def _key(m):
    return (m.ix, m.iy, m.yaw_quadrant)


def _case(N=200, seed=3):
    """The set, its modes and a refinement answer per mode: the mode's pose
    moved by about 1.2 cm / 0.4 degrees; the edge mode's 2 mm further in x, out
    of its cell; the yawed mode not refined."""
    rng = np.random.default_rng(seed)
    T, q, sums, counts = _set(rng, N)
    modes = MMH.modes(T, q, sums, counts, 0, 8)
    assert modes.n_modes == 5 and modes.n_outside > 0
    T_ref, refined = np.array([np.eye(4)] * 8), np.zeros(8, np.int32)
    for k in range(modes.n_modes):
        Tm = np.array(modes.mode[k].T_w_b).reshape(4, 4)
        refined[k] = 1
        if _key(modes.mode[k]) == EDGE:
            assert modes.mode[k].n == 1 and np.array_equal(Tm, T[5])
            T_ref[k] = Tm
            T_ref[k, 0, 3] += 0.002
        else:
            T_ref[k] = _small(rng) @ Tm
            refined[k] = 0 if _key(modes.mode[k]) == (0, 0, 1) else 1
    return T, q, sums, counts, modes, T_ref, refined


# ------------------------------------------------------------------ the tests
def test_struct_sizes_and_null_arguments():
    import mantis_amd as M

    L = M.lib()
    a, b = C.c_int32(), C.c_int32()
    L.mantis_mcl_refine_sizes(C.byref(a), C.byref(b))
    assert a.value == C.sizeof(M.MantisMclModeRefined) and b.value == C.sizeof(M.MantisMclRefined)
    assert M.MantisMclRefined.modes.offset == 16 and M.MantisMclModeRefined.refine.offset == 16
    assert L.mantis_abi_version() == 5
    assert L.mantis_mcl_refine_modes(None, None, 0, 8, None, 0, None) == 1


@pytest.mark.parametrize("apply", [1, 0])
def test_plan(apply):
    T, q, sums, counts, modes, T_ref, refined = _case()
    kept, app, X, bins = plan(modes, T_ref, refined, apply)
    rk, ra, rX, rb = py_plan(modes, T_ref, refined, apply)
    assert np.array_equal(kept, rk) and np.array_equal(app, ra) and np.array_equal(bins, rb)
    _close(X, rX)
    by_key = {_key(modes.mode[k]): k for k in range(modes.n_modes)}
    e, y = by_key[EDGE], by_key[(0, 0, 1)]
    others = [by_key[(0, 0, 0)], by_key[(1, 0, 0)], by_key[(0, -1, 0)]]
    # the refined pose left the cell (ix 2 -> 3): the key is not kept whatever the refinement says
    A = np.array(modes.anchor_T_w_b).reshape(4, 4)
    assert MMH.py_cell_key(T_ref[e], A)[:3] == (3, 0, 0) and refined[e] == 1 and kept[e] == 0 and app[e] == 0
    assert refined[y] == 0 and kept[y] == 0 and app[y] == 0  # not refined: never applied
    assert all(kept[k] == 1 and app[k] == apply for k in others)  # applied together with the two that are not
    assert not kept[modes.n_modes:].any() and not app[modes.n_modes:].any() and np.all(bins[modes.n_modes:] == -1)
    assert np.all(X[modes.n_modes:] == np.eye(4))
    for k in range(modes.n_modes):  # X_k T_mode,k = T_ref,k
        np.testing.assert_allclose(X[k] @ np.array(modes.mode[k].T_w_b).reshape(4, 4), T_ref[k], rtol=0, atol=1e-14)


@pytest.mark.parametrize("N", [1, 7, 200, 4096])
def test_recentre(N):
    rng = np.random.default_rng(40 + N)
    if N >= 200:
        T, q, sums, counts, modes, T_ref, refined = _case(N, seed=N)
    else:
        T, q, sums, counts = _set(rng, N, edge=N > 5)
        modes = MMH.modes(T, q, sums, counts, 0, 8)
        T_ref = np.array([np.eye(4)] * 8)
        for k in range(modes.n_modes):
            T_ref[k] = _small(rng) @ np.array(modes.mode[k].T_w_b).reshape(4, 4)
        refined = np.ones(8, np.int32)
    got, n = recentre(modes, T_ref, refined, 1, T)
    want, rn, which = py_recentre(modes, T_ref, refined, 1, T)
    assert np.array_equal(n, rn)
    moved = which >= 0
    assert moved.any() and n.sum() == moved.sum()
    _close(got[moved], want[moved])
    assert got[~moved].tobytes() == T[~moved].tobytes()  # untouched: byte for byte
    assert not np.array_equal(got[moved], T[moved])
    if N >= 200:
        A = np.array(modes.anchor_T_w_b).reshape(4, 4)
        bins = np.array([MMH.py_cell_key(T[j], A)[3] for j in range(N)])
        assert (bins == MMH.OUTSIDE).sum() > 0 and not moved[bins == MMH.OUTSIDE].any()  # the "outside" bin never moves
        assert not moved[5] and np.any(moved & (q == 0))  # the edge mode stays; a weightless particle moves with its cell
        _, app, _, _ = plan(modes, T_ref, refined, 1)
        for k in range(8):
            assert (n[k] > 0) == bool(app[k])
    # apply = 0, and nothing refined: the set keeps its bytes
    for ap, rf in ((0, refined), (1, np.zeros(8, np.int32))):
        same, n0 = recentre(modes, T_ref, rf, ap, T)
        assert same.tobytes() == T.tobytes() and not n0.any()


@pytest.mark.parametrize("N", [7, 200, 4096])
def test_mean_is_equivariant(N):
    """The modes of the moved set: each applied mode's mean sits on its refined
    pose, with the same particles and the same weight; the rotation block of
    its covariance is unchanged and the translation block turned by X.R."""
    rng = np.random.default_rng(70 + N)
    T, q, sums, counts = _set(rng, N, edge=False)
    if N == 7:
        q[q == 0] = 77  # so few particles: every cluster keeps a member
    before = MMH.py_modes(T, q, sums, counts, 0, 8)
    modes = MMH.modes(T, q, sums, counts, 0, 8)
    assert modes.n_modes == before["n_modes"] == 4
    T_ref = np.array([np.eye(4)] * 8)
    for k in range(4):
        T_ref[k] = _small(rng) @ np.array(modes.mode[k].T_w_b).reshape(4, 4)
    refined = np.array([1, 1, 0, 1, 0, 0, 0, 0], np.int32)
    moved, n = recentre(modes, T_ref, refined, 1, T)
    _, app, X, _ = plan(modes, T_ref, refined, 1)
    assert list(app[:4]) == [1, 1, 0, 1]
    after = MMH.py_modes(moved, q, sums, counts, 0, 8)
    assert after["n_modes"] == 4 and after["weight_sum"] == before["weight_sum"]
    by_best = {e["best"]: e for e in after["modes"]}
    for k, e in enumerate(before["modes"]):
        a = by_best[e["best"]]
        assert (a["n"], a["weight"]) == (e["n"], e["weight"]) == (modes.mode[k].n, modes.mode[k].weight)
        if app[k]:
            np.testing.assert_allclose(a["T"], T_ref[k], rtol=0, atol=POSE_TOL)
            R = X[k][:3, :3]
            tol = 1e-9 * max(np.diag(e["cov"]).max(), 1e-300)
            np.testing.assert_allclose(a["cov"][3:, 3:], e["cov"][3:, 3:], rtol=0, atol=tol)
            np.testing.assert_allclose(a["cov"][:3, :3], R @ e["cov"][:3, :3] @ R.T, rtol=0, atol=tol)
        else:
            assert np.array_equal(a["T"], e["T"]) and n[k] == 0
