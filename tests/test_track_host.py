"""Rig tracking, host side: the C-ABI's host-only entries (defaults, struct
sizes) and the pool / pick / gate rules of mantis_amd/csrc/mk_track.h -- the
very functions k_track_particles runs -- built for the host
(build/libmantis_hostcheck.so hc_track_*) against a few lines of numpy.
tools/trackcheck_main.cpp runs the same cases stand-alone (for a sanitizer
build of mk_track.h).
"""
import ctypes as C

import numpy as np

import _hostcheck as H

DBL_MAX = np.finfo(np.float64).max


def _hc():
    L = H.lib()
    vp = C.c_void_p
    L.hc_track_pool.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
    L.hc_track_pool.restype = None
    L.hc_track_error_of.argtypes = [C.c_int64, C.c_int32]
    L.hc_track_error_of.restype = C.c_double
    L.hc_track_pick.argtypes = [vp, C.c_int, C.c_double]
    L.hc_track_pick.restype = C.c_int
    L.hc_track_gate.argtypes = [C.c_double, C.c_int32, C.c_int32, C.c_double]
    L.hc_track_gate.restype = C.c_int
    L.hc_track_particle.argtypes = [vp, vp, C.c_double, C.c_double, vp, vp, vp]
    L.hc_track_particle.restype = None
    return L


def pool(sums, counts):
    sums = np.ascontiguousarray(sums, np.int64)
    counts = np.ascontiguousarray(counts, np.int32)
    P, Cn = sums.shape
    err = np.zeros(P)
    n = np.zeros(P, np.int32)
    _hc().hc_track_pool(sums.ctypes.data, counts.ctypes.data, P, Cn, err.ctypes.data, n.ctypes.data)
    return err, n


def pick(err, cur):
    err = np.ascontiguousarray(err, np.float64)
    return _hc().hc_track_pick(err.ctypes.data, len(err), cur)


def gate(error, n_proj, min_projections, max_error):
    return _hc().hc_track_gate(error, n_proj, min_projections, max_error)


# the rules in numpy (the issue's definition)
def np_pool(sums, counts):
    s = np.asarray(sums, np.int64).sum(axis=1)
    n = np.asarray(counts, np.int64).sum(axis=1)
    err = np.full(len(s), DBL_MAX)
    ok = n > 0
    err[ok] = s[ok].astype(np.float64) / (n[ok].astype(np.float64) * 1.1)
    return err, n.astype(np.int32)


def np_pick(err, cur):
    j = int(np.argmin(err))  # first minimum: argmin by (E, j)
    return j if err[j] < cur else -1


def np_gate(error, n_proj, min_projections, max_error):
    return int(error != DBL_MAX and n_proj >= min_projections and (max_error <= 0 or error <= max_error))


def test_default_track_params_and_struct_sizes():
    import mantis_amd as M

    L = M.lib()
    p = M.MantisTrackParams()
    L.mantis_default_track_params(None, C.byref(p))
    assert p.struct_size == C.sizeof(M.MantisTrackParams)
    assert (p.particles, p.iterations, p.sigma_rot, p.sigma_t) == (50, 10, 0.03, 0.01)
    assert (p.min_projections, p.record, p.max_error) == (10, 0, 0.0)
    a, b = C.c_int32(), C.c_int32()
    L.mantis_track_sizes(C.byref(a), C.byref(b))
    assert a.value == C.sizeof(M.MantisTrackParams) == p.struct_size
    assert b.value == C.sizeof(M.MantisTrackResult)
    assert L.mantis_abi_version() >= 3
    # null context / arguments are argument errors, not crashes
    assert L.mantis_track_batch(None, None, 1, 1, None, None, None) == 1
    assert L.mantis_track(None, None, 1, None, None, None, None) == 1
    assert L.mantis_get_track_record(None, 0, -1, None, None, None, None, None) == 1


def test_pool_matches_numpy():
    rng = np.random.default_rng(3)
    for P, Cn in [(1, 1), (7, 3), (96, 1), (64, 8)]:
        counts = rng.integers(0, 700, (P, Cn)).astype(np.int32)
        counts[rng.random((P, Cn)) < 0.3] = 0
        sums = counts.astype(np.int64) * rng.integers(0, 3 * 255 * 255 + 1, (P, Cn))
        e, n = pool(sums, counts)
        re, rn = np_pool(sums, counts)
        assert np.array_equal(e, re) and np.array_equal(n, rn)
    # sums past 2^31 and 2^53 / 1.1-free check of the int64 -> double conversion
    sums = np.array([[3 * 255 * 255 * 768, 3 * 255 * 255 * 768]] * 2, np.int64)
    counts = np.array([[768, 768], [768, 0]], np.int32)
    e, n = pool(sums, counts)
    assert np.array_equal(e, np_pool(sums, counts)[0]) and list(n) == [1536, 768]


def test_error_of_is_pool_with_one_camera():
    """The single scorers' error (track::error_of: the pipeline's init, particle
    filter and shifts, the standalone scorer) is the pooled error of one camera."""
    cases = [(0, 0), (5, 0), (0, 1), (3 * 255 * 255, 1), (123456789, 700), (3 * 255 * 255 * 768, 768),
             (1, 3), ((1 << 53) + 1, 7), (10, -1)]
    for s, n in cases:
        e = _hc().hc_track_error_of(s, n)
        pe, pn = pool([[s]], [[n]])
        assert e == pe[0] and pn[0] == n
        assert e == (DBL_MAX if n <= 0 else float(np.float64(s) / (np.float64(n) * 1.1)))


def test_all_blind_cameras():
    sums = np.zeros((5, 4), np.int64)
    counts = np.zeros((5, 4), np.int32)
    e, n = pool(sums, counts)
    assert np.all(e == DBL_MAX) and np.all(n == 0)
    assert pick(e, DBL_MAX) == -1 == np_pick(e, DBL_MAX)  # DBL_MAX is not < DBL_MAX
    assert gate(DBL_MAX, 0, 0, 0.0) == 0 == np_gate(DBL_MAX, 0, 0, 0.0)
    assert gate(DBL_MAX, 100, 10, 0.0) == 0
    # one seeing camera: the pooled error is that camera's alone
    sums[2, 1], counts[2, 1] = 123456, 40
    e, n = pool(sums, counts)
    assert e[2] == 123456.0 / (40.0 * 1.1) and n[2] == 40
    assert pick(e, DBL_MAX) == 2


def test_pick_ties_and_strictness():
    assert pick([5.0, 3.0, 3.0, 4.0], 10.0) == 1  # equal errors: the lowest index
    assert pick([3.0] * 96, 10.0) == 0
    assert pick([7.0, 3.0, 9.0], 3.0) == -1  # equal to the current error: not accepted (strict)
    assert pick([7.0, 3.0, 9.0], np.nextafter(3.0, 4.0)) == 1
    assert pick([DBL_MAX, DBL_MAX], 1.0) == -1
    assert pick([DBL_MAX, 2.0], DBL_MAX) == 1
    rng = np.random.default_rng(4)
    for n in (1, 2, 63, 64, 65, 96):
        for _ in range(20):
            err = rng.integers(0, 6, n).astype(np.float64)  # many ties
            cur = float(rng.integers(0, 6))
            assert pick(err, cur) == np_pick(err, cur)


def test_gate_boundaries():
    assert gate(100.0, 9, 10, 0.0) == 0   # one below min_projections
    assert gate(100.0, 10, 10, 0.0) == 1  # exactly at it
    assert gate(100.0, 10, 10, -1.0) == 1  # max_error <= 0: no error gate
    assert gate(100.0, 10, 10, 100.0) == 1
    assert gate(100.0, 10, 10, np.nextafter(100.0, 0.0)) == 0
    assert gate(0.0, 0, 0, 0.0) == 1
    for args in [(100.0, 9, 10, 0.0), (100.0, 10, 10, 0.0), (5.0, 50, 10, 4.0), (5.0, 50, 10, 5.0),
                 (DBL_MAX, 50, 10, 0.0), (5.0, 50, 10, -3.0)]:
        assert gate(*args) == np_gate(*args)


def test_particle_pose_rule():
    """particle = T * Transform(setRPY(roll, pitch, yaw), (x, y, z)) from
    gaussians drawn yaw, pitch, roll, z, y, x; c2w = inverse(particle @ T_base_cam)."""
    from mantis_amd import synth

    rng = np.random.default_rng(5)
    T = synth.random_base_pose(rng)
    ext = synth.rig_extrinsics(3)[1]
    g = rng.normal(size=6).astype(np.float32)
    sr, st = 0.03, 0.01
    To = np.zeros((4, 4))
    c2w = np.zeros(12)
    Tc, ec = np.ascontiguousarray(T), np.ascontiguousarray(ext)
    _hc().hc_track_particle(Tc.ctypes.data, g.ctypes.data, sr, st, ec.ctypes.data, To.ctypes.data, c2w.ctypes.data)
    yaw, pitch, roll = (float(g[0]) * sr, float(g[1]) * sr, float(g[2]) * sr)
    rnd = np.eye(4)
    rnd[:3, :3] = synth.rot_z(yaw) @ synth.rot_y(pitch) @ synth.rot_x(roll)  # setRPY
    rnd[:3, 3] = [float(g[5]) * st, float(g[4]) * st, float(g[3]) * st]
    ref = T @ rnd
    np.testing.assert_allclose(To, ref, atol=1e-12, rtol=0)
    inv = np.linalg.inv(ref @ ext)
    np.testing.assert_allclose(c2w, np.concatenate([inv[:3, :3].reshape(9), inv[:3, 3]]), atol=1e-12, rtol=0)
    # sigma 0: the particle is the pose itself, bit for bit
    _hc().hc_track_particle(Tc.ctypes.data, g.ctypes.data, 0.0, 0.0, ec.ctypes.data, To.ctypes.data, c2w.ctypes.data)
    assert np.array_equal(To, T)
