"""Monte Carlo localization, the modes of the set, host side: the cell key,
the bin table, the mode order, the lattice site and the per-cell estimate of
mantis_amd/csrc/mk_mcl_modes.h -- the very functions k_mcl_modes / k_mcl_keep
run -- built for the host (build/libmantis_hostcheck.so hc_mcl_cell_key /
hc_mcl_lattice_site / hc_mcl_modes) against Python restatements written here
(big integers for the weights, test_mcl_host.np_estimate for the estimate).
tools/mclmodescheck_main.cpp drives the same rules stand-alone (for a
sanitizer build of the header).
"""
import ctypes as C
import math

import numpy as np
import pytest

import _hostcheck as H
import test_mcl_host as MH
from mantis_amd import synth

DBL_MAX = np.finfo(np.float64).max
POSE_TOL = 1e-9
Q1 = 1 << 40
G = 0.32
OUTSIDE = 900


def _hc():
    L = H.lib()
    vp = C.c_void_p
    L.hc_mcl_cell_key.argtypes = [vp, vp, C.c_double, vp]
    L.hc_mcl_cell_key.restype = None
    L.hc_mcl_lattice_site.argtypes = [C.c_int, C.c_int, C.c_int, vp]
    L.hc_mcl_lattice_site.restype = None
    L.hc_mcl_modes.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, vp]
    L.hc_mcl_modes.restype = None
    return L


# ---------------------------------------------------------- the rules restated
def py_cell_key(T, A, g=G):
    """(ix, iy, k, bin) of pose T against the anchor A (4 x 4 each), in Python floats."""
    ix = math.floor((float(T[0, 3]) - float(A[0, 3])) / g + 0.5)
    iy = math.floor((float(T[1, 3]) - float(A[1, 3])) / g + 0.5)
    h0, h1, a0, a1 = float(T[0, 0]), float(T[1, 0]), float(A[0, 0]), float(A[1, 0])
    c = h0 * a0 + h1 * a1
    s = a0 * h1 - a1 * h0
    if abs(c) >= abs(s):
        k = 0 if c >= 0 else 2
    else:
        k = 1 if s > 0 else 3
    inside = abs(ix) <= 7 and abs(iy) <= 7
    return ix, iy, k, ((iy + 7) * 15 + (ix + 7)) * 4 + k if inside else OUTSIDE


def py_pooled(sums, counts, j):
    n = int(np.asarray(counts[j], np.int64).sum())
    return DBL_MAX if n <= 0 else float(int(np.asarray(sums[j], np.int64).sum())) / (float(n) * 1.1)


def py_modes(T, q, sums, counts, best, max_modes, g=G):
    """The modes of poses T [N, 4, 4] with integer weights q against the anchor
    T[best]: a dict of the header's fields and `modes`, one dict per reported
    mode in mode order (the estimate by np_estimate on the bin's particles)."""
    r = {"n_modes": 0, "n_cells": 0, "n_outside": 0, "weight_sum": 0, "outside_weight": 0, "modes": [],
         "anchor": np.zeros((4, 4)), "bins": np.full(len(T), -1)}
    if best < 0:
        return r
    r["anchor"] = np.array(T[best])
    members = {}
    for j in range(len(T)):
        if int(q[j]) == 0:
            continue
        b = py_cell_key(T[j], T[best], g)[3]
        r["bins"][j] = b
        members.setdefault(b, []).append(j)
        r["weight_sum"] += int(q[j])
    out = members.pop(OUTSIDE, [])
    r["n_outside"] = len(out)
    r["outside_weight"] = sum(int(q[j]) for j in out)
    W = {b: sum(int(q[j]) for j in js) for b, js in members.items()}
    order = sorted(members, key=lambda b: (-W[b], b))
    r["n_cells"] = len(order)
    r["all_bins"] = order
    for b in order[:max_modes]:
        js = members[b]
        qs = np.array([int(q[j]) for j in js], np.uint64)
        Tm, cov, _, first = MH.np_estimate(np.asarray(T)[js], qs)
        jb = js[first]  # the heaviest of the bin, the first on ties
        r["modes"].append({"ix": (b >> 2) % 15 - 7, "iy": (b >> 2) // 15 - 7, "k": b & 3, "n": len(js), "best": jb,
                           "weight": W[b], "share": W[b] / r["weight_sum"], "best_error": py_pooled(sums, counts, jb),
                           "T": Tm, "cov": cov, "bin": b})
    r["n_modes"] = len(r["modes"])
    return r


def check_modes(got, ref, max_modes):
    """A MantisMclModes against py_modes' answer: integers exactly, the estimate to the step's tolerances."""
    assert got.status == 0
    assert (got.n_modes, got.n_cells, got.n_outside) == (ref["n_modes"], ref["n_cells"], ref["n_outside"])
    assert got.n_modes == min(max_modes, ref["n_cells"])
    assert (got.weight_sum, got.outside_weight) == (ref["weight_sum"], ref["outside_weight"])
    assert np.array_equal(np.array(got.anchor_T_w_b).reshape(4, 4), ref["anchor"])
    for i, e in enumerate(ref["modes"]):
        m = got.mode[i]
        assert (m.ix, m.iy, m.yaw_quadrant, m.n, m.best, m.weight) == (e["ix"], e["iy"], e["k"], e["n"], e["best"],
                                                                      e["weight"]), f"mode {i}"
        np.testing.assert_allclose(m.share, e["share"], rtol=1e-12, atol=0)
        assert m.best_error == e["best_error"], f"mode {i}"
        np.testing.assert_allclose(np.array(m.T_w_b).reshape(4, 4), e["T"], atol=POSE_TOL, rtol=0, err_msg=f"mode {i}")
        cov = np.array(m.covariance).reshape(6, 6)
        np.testing.assert_allclose(cov, e["cov"], atol=1e-9 * max(np.diag(e["cov"]).max(), 0.0), rtol=0,
                                   err_msg=f"mode {i}")
        assert np.array_equal(cov, cov.T)
    for i in range(got.n_modes, 8):  # empty records
        m = got.mode[i]
        assert (m.n, m.best, m.weight, m.share) == (0, -1, 0, 0.0)
        assert not np.any(np.array(m.T_w_b)) and not np.any(np.array(m.covariance))


# ------------------------------------------------------------------ the calls
def cell_key(T, A, g=G):
    T, A = np.ascontiguousarray(T, np.float64), np.ascontiguousarray(A, np.float64)
    k = np.zeros(4, np.int32)
    _hc().hc_mcl_cell_key(T.ctypes.data, A.ctypes.data, g, k.ctypes.data)
    return tuple(int(v) for v in k)


def modes(T, q, sums, counts, best, max_modes, g=G):
    import mantis_amd as M

    T = np.ascontiguousarray(T, np.float64)
    q = np.ascontiguousarray(q, np.uint64)
    sums, counts = np.ascontiguousarray(sums, np.int64), np.ascontiguousarray(counts, np.int32)
    out = M.MantisMclModes()
    _hc().hc_mcl_modes(T.ctypes.data, q.ctypes.data, sums.ctypes.data, counts.ctypes.data, len(T), sums.shape[1], best,
                       g, max_modes, C.addressof(out))
    return out


def _pose(yaw, xy=(0.0, 0.0), z=1.2, tilt=0.0):
    T = np.eye(4)
    T[:3, :3] = synth.rot_z(yaw) @ synth.rot_y(tilt)
    T[:3, 3] = [xy[0], xy[1], z]
    return T


def spread_set(rng, N, cells=9):
    """N poses over the lattice cells and yaw quadrants around a random base pose."""
    A = synth.random_base_pose(rng)
    out = np.zeros((N, 4, 4))
    for j in range(N):
        d = np.eye(4)
        a = rng.normal(size=3) * 0.03
        d[:3, :3] = synth.rot_z(a[0] + math.pi / 2 * int(rng.integers(0, 4))) @ synth.rot_y(a[1]) @ synth.rot_x(a[2])
        d[:3, 3] = rng.normal(size=3) * 0.02
        out[j] = A @ d
        out[j, :2, 3] += G * rng.integers(-cells, cells + 1, 2)
    return out


def _inputs(rng, N, Cn=2):
    counts = rng.integers(0, 700, (N, Cn)).astype(np.int32)
    sums = counts.astype(np.int64) * rng.integers(20000, 90000, (N, Cn))
    return sums, counts


# ------------------------------------------------------------------ the tests
def test_struct_sizes_and_null_arguments():
    import mantis_amd as M

    L = M.lib()
    a, b = C.c_int32(), C.c_int32()
    L.mantis_mcl_modes_sizes(C.byref(a), C.byref(b))
    assert a.value == C.sizeof(M.MantisMclMode) and b.value == C.sizeof(M.MantisMclModes)
    assert L.mantis_abi_version() == 5
    assert L.mantis_mcl_init_lattice(None, None, 0.0, 0.0, 0, 0, None) == 1
    assert L.mantis_mcl_modes(None, 8, None) == 1
    assert L.mantis_mcl_select_mode(None, 0) == 1


def test_cell_key_half_cell_offsets():
    """floor(x + 0.5) decides at exactly +-0.5 cell: +0.5 goes up, -0.5 stays (anchor at the origin: exact)."""
    A = _pose(0.0)
    half = 0.5 * G
    assert half / G == 0.5
    cases = [(half, 1), (np.nextafter(half, 0), 0), (-half, 0), (np.nextafter(-half, -1), -1), (3 * half, 2),
             (np.nextafter(3 * half, 0), 1), (0.0, 0)]
    for d, want in cases:
        for axis in (0, 1):
            xy = [0.0, 0.0]
            xy[axis] = d
            T = _pose(0.0, xy)
            key = cell_key(T, A)
            assert key == py_cell_key(T, A) and key[axis] == want and key[1 - axis] == 0, (d, axis)


def test_cell_key_range():
    A = _pose(0.3, (0.11, -0.07))
    for n, inside in [(7, True), (-7, True), (8, False), (-8, False), (100, False), (-100000, False)]:
        for axis in (0, 1):
            T = A.copy()
            T[axis, 3] += n * G
            key = cell_key(T, A)
            assert key == py_cell_key(T, A)
            assert key[axis] == n and (key[3] < OUTSIDE) == inside
    T = A.copy()
    T[0, 3] += 7 * G
    T[1, 3] -= 7 * G
    assert cell_key(T, A) == (7, -7, 0, (0 * 15 + 14) * 4) and cell_key(A, A) == (0, 0, 0, (7 * 15 + 7) * 4)
    far = A.copy()
    far[0, 3] = 1e300  # far past any int: saturated, outside
    assert cell_key(far, A)[3] == OUTSIDE


def test_cell_key_yaw_quadrants():
    rng = np.random.default_rng(1)
    for a0 in (0.0, 0.7, -2.9, math.pi / 4):
        A = _pose(a0, tilt=0.2)
        for k, dyaw in enumerate((0.0, math.pi / 2, math.pi, -math.pi / 2)):  # the four axis headings
            for jitter in (0.0, 0.3, -0.3):
                T = _pose(a0 + dyaw + jitter, tilt=-0.1)
                assert cell_key(T, A) == py_cell_key(T, A) and cell_key(T, A)[2] == k
        for _ in range(50):
            T = _pose(rng.uniform(-4, 4), tilt=rng.uniform(-1, 1))
            assert cell_key(T, A) == py_cell_key(T, A)
    # the 45 degree diagonals with exact ties |c| = |s|: the cosine side wins
    A = np.eye(4)
    v = math.sqrt(0.5)
    for (h0, h1), k in [((v, v), 0), ((-v, v), 2), ((-v, -v), 2), ((v, -v), 0)]:
        T = np.eye(4)
        T[0, 0], T[1, 0] = h0, h1
        assert cell_key(T, A)[2] == k == py_cell_key(T, A)[2]
    # a vertical base x-axis has no heading: c = s = 0 gives quadrant 0
    for up in (1.0, -1.0):
        T = np.eye(4)
        T[:3, :3] = [[0, 0, -up], [0, 1, 0], [up, 0, 0]]
        assert cell_key(T, A)[2] == 0 == py_cell_key(T, A)[2] and cell_key(A, T)[2] == 0


def test_lattice_site_order():
    L = _hc()
    for cx, cy in [(0, 0), (1, 2), (7, 7), (3, 0), (0, 4)]:
        w = 2 * cx + 1
        seen = []
        for s in range(w * (2 * cy + 1)):
            o = np.zeros(2, np.int32)
            L.hc_mcl_lattice_site(s, cx, cy, o.ctypes.data)
            assert (int(o[0]), int(o[1])) == (s % w - cx, s // w - cy)
            seen.append((int(o[0]), int(o[1])))
        assert seen[0] == (-cx, -cy) and seen[-1] == (cx, cy) and len(set(seen)) == len(seen)
        assert seen == [(x, y) for y in range(-cy, cy + 1) for x in range(-cx, cx + 1)]  # x runs fastest


@pytest.mark.parametrize("N", [1, 7, 257, 4096])
def test_modes_of_random_sets(N):
    rng = np.random.default_rng(200 + N)
    T = spread_set(rng, N)
    q = rng.integers(1, Q1 + 1, N).astype(np.uint64)
    q[rng.random(N) < 0.3] = 0
    best = int(rng.integers(0, N))
    q[best] = Q1
    best = int(np.argmax(q))
    sums, counts = _inputs(rng, N)
    full = py_modes(T, q, sums, counts, best, 8)
    assert N < 257 or (full["n_cells"] > 8 and full["n_outside"] > 0)
    assert sum(int(q[j]) for j in range(N)) == full["weight_sum"]
    for mm in (8, 3, 1):
        got = modes(T, q, sums, counts, best, mm)
        check_modes(got, py_modes(T, q, sums, counts, best, mm), mm)
    # the reported bins, the bins past the eighth and the outside add up to S exactly
    got = modes(T, q, sums, counts, best, 8)
    rest = set(full["all_bins"][8:])
    W_rest = sum(int(q[j]) for j in range(N) if full["bins"][j] in rest)
    assert sum(got.mode[i].weight for i in range(got.n_modes)) + W_rest + got.outside_weight == got.weight_sum


def test_every_bin_reported_adds_up():
    """Fewer than 8 cells: sum W_b + outside_weight == weight_sum, exactly."""
    rng = np.random.default_rng(5)
    N = 300
    T = spread_set(rng, N, cells=1)[:N]
    T[:, :3, :3] = T[0, :3, :3]  # one heading: at most 9 cells
    T[N - 5:, 0, 3] += 20 * G  # some outside
    keep = np.array([py_cell_key(T[j], T[0])[3] for j in range(N)])
    cells = sorted(set(keep) - {OUTSIDE})[:6]
    q = rng.integers(1, Q1 + 1, N).astype(np.uint64)
    q[~np.isin(keep, cells + [OUTSIDE])] = 0
    q[0] = Q1
    sums, counts = _inputs(rng, N)
    got = modes(T, q, sums, counts, 0, 8)
    assert got.n_modes == got.n_cells == len(cells) and got.n_outside == 5
    assert sum(got.mode[i].weight for i in range(got.n_modes)) + got.outside_weight == got.weight_sum
    assert got.weight_sum == int(q.astype(object).sum())
    assert sum(got.mode[i].n for i in range(got.n_modes)) + got.n_outside == int((q > 0).sum())
    check_modes(got, py_modes(T, q, sums, counts, 0, 8), 8)


def test_equal_weights_order_by_bin_index():
    A = _pose(0.2, (0.5, 0.5))
    T = np.array([A, A, A, A, A])
    T[1, 0, 3] += G       # bin of (1, 0, 0)
    T[2, 1, 3] -= G       # bin of (0, -1, 0): the lowest index of the three
    T[3, 0, 3] += G + 0.01  # beside particle 1, not on it: a covariance to compare
    T[4] = _pose(0.2 + math.pi / 2, (0.5, 0.5))  # (0, 0, 1)
    q = np.array([Q1, 300, 500, 200, 500], np.uint64)  # W: 2^40 | 500 | 500 | 500
    sums, counts = _inputs(np.random.default_rng(1), 5)
    got = modes(T, q, sums, counts, 0, 8)
    keys = [(got.mode[i].ix, got.mode[i].iy, got.mode[i].yaw_quadrant, got.mode[i].weight) for i in range(4)]
    assert got.n_modes == 4
    assert keys == [(0, 0, 0, Q1), (0, -1, 0, 500), (0, 0, 1, 500), (1, 0, 0, 500)]
    assert got.mode[3].n == 2 and got.mode[3].best == 1
    check_modes(got, py_modes(T, q, sums, counts, 0, 8), 8)
    check_modes(modes(T, q, sums, counts, 0, 2), py_modes(T, q, sums, counts, 0, 2), 2)


def test_heaviest_of_a_bin_first_on_ties():
    rng = np.random.default_rng(9)
    A = _pose(-1.0)
    T = np.array([A] * 6)
    for j in range(6):
        T[j, :3, 3] += rng.normal(size=3) * 0.01
    T[3:, 0, 3] += 2 * G
    q = np.array([Q1, Q1, 7, 900, 12, 900], np.uint64)
    sums, counts = _inputs(rng, 6)
    got = modes(T, q, sums, counts, 0, 8)
    assert got.n_modes == 2 and (got.mode[0].best, got.mode[1].best) == (0, 3)
    assert got.mode[1].best_error == py_pooled(sums, counts, 3)
    check_modes(got, py_modes(T, q, sums, counts, 0, 8), 8)


def test_single_particle_mode_is_that_particle():
    rng = np.random.default_rng(10)
    T = spread_set(rng, 3, cells=0)
    T[1, 0, 3] += 3 * G
    q = np.array([Q1, 12345, 0], np.uint64)
    sums, counts = _inputs(rng, 3)
    got = modes(T, q, sums, counts, 0, 8)
    m = [got.mode[i] for i in range(2)]
    hit = [i for i in range(2) if m[i].best == 1]
    assert got.n_modes == 2 and len(hit) == 1 and m[hit[0]].n == 1
    assert np.array_equal(np.array(m[hit[0]].T_w_b).reshape(4, 4), T[1]) and not np.any(np.array(m[hit[0]].covariance))


def test_everything_outside_has_no_mode():
    rng = np.random.default_rng(11)
    N = 40
    T = spread_set(rng, N, cells=0)
    T[1:, 0, 3] += 8 * G + G * rng.integers(0, 5, N - 1)
    q = rng.integers(1, Q1, N).astype(np.uint64)
    q[0] = 0  # the anchor itself carries no weight: its own cell stays empty
    sums, counts = _inputs(rng, N)
    got = modes(T, q, sums, counts, 0, 8)
    assert got.n_modes == 0 and got.n_cells == 0 and got.n_outside == N - 1
    assert got.outside_weight == got.weight_sum == int(q.astype(object).sum())
    check_modes(got, py_modes(T, q, sums, counts, 0, 8), 8)
    # no anchor at all (a lost step): nothing
    got = modes(T, np.zeros(N, np.uint64), sums, counts, -1, 8)
    assert got.n_modes == 0 and got.weight_sum == 0 and not np.any(np.array(got.anchor_T_w_b))
