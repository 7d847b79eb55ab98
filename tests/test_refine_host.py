"""Line refinement, host side: the rules of mantis_amd/csrc/mk_refine.h -- the
very functions k_refine_obs / k_refine_step run -- built for the host
(build/libmantis_hostcheck.so hc_refine_*) against the rule of include/mantis.h
restated in numpy / plain Python (tests/_refine_ref.py), each reject code
reached by construction, the Jacobian row against finite differences, the
whole iteration on a rendered four-camera rig, the covariance, and the C-ABI's
host-only entries. tools/refinecheck_main.cpp runs the memory-facing cases
stand-alone (for a sanitizer build).
"""
import ctypes as C
import math

import numpy as np
import pytest

import _refine_ref as RR
from mantis_amd import synth

W, H = RR.W, RR.H_


@pytest.fixture(scope="module")
def lm(landmark_map):
    return RR.all_landmarks(landmark_map)


@pytest.fixture(scope="module")
def scene():
    return RR.rig_scene(4, 1)


def test_line_flags(lm):
    X, nw, nr, ng = lm
    f = RR.flags(X, 0.08)
    assert [int((f == k).sum()) for k in (1, 2, 3)] == [270, 270, 180]
    assert np.array_equal(f, RR.np_flags(X, 0.08))
    assert len(RR.candidates(f)) == 540
    # no neighbours: nothing is on a line
    far = np.arange(30, dtype=np.float64).reshape(10, 3) * 1.7
    assert not RR.flags(far, 0.08).any() and not RR.np_flags(far, 0.08).any()
    # another pitch: other flags (0.32 is also the distance between parallel lines; nothing is 0.05 apart)
    g = RR.flags(X, 0.32)
    assert np.array_equal(g, RR.np_flags(X, 0.32)) and not np.array_equal(f, g)
    assert not RR.flags(X, 0.05).any()
    # a hand-made cross: the centre has both bits, the arms one each, the tolerance is 1e-6
    cross = np.array([[0, 0, 0], [0.08, 0, 0], [-0.08, 0, 0], [0, 0.08, 0], [0, -0.08 + 5e-7, 0], [0.5, 0.5, 0],
                      [0.5, 0.58 + 2e-6, 0]], np.float64)
    assert list(RR.flags(cross, 0.08)) == [3, 1, 1, 2, 2, 0, 0] == list(RR.np_flags(cross, 0.08))


def test_obs_matches_numpy(lm, scene):
    """Every 7th candidate of camera 0 at the shifted pose: codes, Sw, Skw equal, rows to rtol 1e-12."""
    X, nw, nr, ng = lm
    K, D = synth.intrinsics(W, H)
    T = RR.shift(scene["Twb"][0])
    f = RR.flags(X, 0.08)
    cand = RR.candidates(f)
    img = scene["frames"][0][0]
    codes, Sw, Skw, rows, tie = RR.obs(T, scene["ext"][0], K, D, img, X, nw, nr, ng, f)
    assert not tie.any(), "the scene has no sample within 1e-9 of a rounding tie"
    seen = set()
    for k in range(0, len(cand), 7):
        i = cand[k]
        tg = RR.TARGETS["w" if i < nw else "r" if i < nw + nr else "g"]
        code, sw, skw, row = RR.np_observe(T, scene["ext"][0], K, D, img, X[i], 0 if f[i] == 1 else 1, tg)
        assert (codes[k], Sw[k], Skw[k]) == (code, sw, skw), (k, i)
        np.testing.assert_allclose(rows[k], row, rtol=1e-12, atol=0, err_msg=f"candidate {k}")
        seen.add(code)
    assert 0 in seen and len(seen) >= 2, seen
    assert np.all(rows[codes != 0] == 0.0)


def _black(h=H, w=W):
    return np.zeros((h, w, 3), np.uint8)


def _sample_px(T, Tbc, K, D, Xi, axis, R):
    p, q, m0, nh, Jpi, R_cb = RR.np_geometry(T, Tbc, Xi, axis)
    s = 1.0 / float(np.float32(K[0, 0]))
    out = []
    for k in range(-R, R + 1):
        u, v = RR.np_distort(K, D, m0[0] + k * s * nh[0], m0[1] + k * s * nh[1])
        out.append((int(np.rint(u)), int(np.rint(v))))
    return out


def test_reject_codes_by_construction(lm, scene):
    X, nw, nr, ng = lm
    K, D = synth.intrinsics(W, H)
    T = scene["Twb"][0]
    ext = scene["ext"][0]
    f = RR.flags(X, 0.08)
    cand = RR.candidates(f)
    R = 12
    base = RR.obs(T, ext, K, D, scene["frames"][0][0], X, nw, nr, ng, f)[0]
    # a white landmark that is observed in the rendered frame, its window well inside
    k0 = next(k for k in range(len(cand)) if base[k] == 0 and cand[k] < nw and
              all(20 <= x < W - 20 and 20 <= y < H - 20
                  for x, y in _sample_px(T, ext, K, D, X[cand[k]], 0 if f[cand[k]] == 1 else 1, R)))
    i0 = cand[k0]
    px = _sample_px(T, ext, K, D, X[i0], 0 if f[i0] == 1 else 1, R)

    def one(img, Tbc=ext, **kw):
        codes, Sw, Skw, rows, _ = RR.obs(T, Tbc, K, D, img, X, nw, nr, ng, f, **kw)
        return int(codes[k0]), int(Sw[k0]), int(Skw[k0]), rows[k0], codes

    # code 1: a camera looking straight up from the base sees every landmark behind it
    code, sw, skw, row, codes = one(_black(), Tbc=np.eye(4))
    assert np.all(codes == 1) and (sw, skw) == (0, 0) and not row.any()
    # code 3: the frame cut so that the window's rightmost / lowest sample is the first pixel outside
    xmax, ymax = max(x for x, _ in px), max(y for _, y in px)
    assert one(np.ascontiguousarray(_black()[:, :xmax]))[0] == 3
    assert one(np.ascontiguousarray(_black()[:ymax, :]))[0] == 3
    assert one(np.ascontiguousarray(_black()[: ymax + 1, : xmax + 1]))[0] == 5  # one more pixel: inside again
    # code 5: a threshold no pixel meets (d2 = 3 everywhere, white_thresh 1, 2, 3), and too little weight
    grey = np.full((H, W, 3), 254, np.uint8)
    for th in (1, 2, 3):
        assert one(grey, white_thresh=th)[:3] == (5, 0, 0)
    code, sw, skw, row, _ = one(grey, white_thresh=4)  # every sample weighs 1, both ends too
    assert (code, sw, skw) == (4, 2 * R + 1, 0)
    # code 4: the line at the window's end, either end
    for end in (0, 2 * R):
        img = _black()
        x, y = px[end]
        img[y, x] = 255
        code, sw, skw, row, _ = one(img)
        assert (code, sw, skw) == (4, 12288, (end - R) * 12288) and not row.any()
    # code 5 by weight: one white pixel inside weighs 12288 < min_weight; code 0 once it is allowed
    img = _black()
    x, y = px[R + 3]
    img[y, x] = 255
    assert one(img)[:3] == (5, 12288, 3 * 12288)
    code, sw, skw, row, _ = one(img, min_weight=12288)
    s = 1.0 / float(np.float32(K[0, 0]))
    assert (code, sw, skw) == (0, 12288, 3 * 12288) and row[6] == -(3.0 * s)
    # two pixels: the weighted centroid, exactly
    x2, y2 = px[R - 2]
    img[y2, x2] = (255, 255, 250)  # d2 = 25
    assert one(img)[0] == 5  # 24551 is still one pixel's worth short of the default min_weight
    code, sw, skw, row, _ = one(img, min_weight=24551)
    assert (code, sw, skw) == (0, 12288 + 12263, 3 * 12288 - 2 * 12263)
    assert row[6] == -((float(skw) / float(sw)) * s)
    # a red and a green landmark answer to their own colours only
    for lo, hi, col in ((nw, nw + nr, (50, 85, 255)), (nw + nr, nw + nr + ng, (50, 255, 85))):
        ks = [k for k in range(len(cand)) if lo <= cand[k] < hi and base[k] in (0, 4, 5)]
        if not ks:
            continue
        k = ks[0]
        i = cand[k]
        pk = _sample_px(T, ext, K, D, X[i], 0 if f[i] == 1 else 1, R)
        if not all(0 <= x < W and 0 <= y < H for x, y in pk):
            continue
        painted = {pk[R - 1], pk[R + 1]}
        hits = sum(s in painted for s in pk)  # neighbouring samples may round to one pixel
        for paint, want in ((col, hits * 12288), ((255, 255, 255), 0)):
            img = _black()
            for x, y in painted:
                img[y, x] = paint
            codes, Sw, Skw, rows, _ = RR.obs(T, ext, K, D, img, X, nw, nr, ng, f)
            assert int(Sw[k]) == want and int(codes[k]) == (0 if want else 5)


def test_jacobian_against_finite_differences(lm, scene):
    """J = d/d(delta) of nh^T (pi(p(T Exp delta)) - m0) at 0, nh held fixed: central differences, h = 1e-6.
    Rounding ~ eps |pi| / h ~ 2e-10, truncation ~ h^2: the bound 1e-8 leaves a factor 50."""
    X, nw, nr, ng = lm
    K, D = synth.intrinsics(W, H)
    T = RR.shift(scene["Twb"][0])
    f = RR.flags(X, 0.08)
    cand = RR.candidates(f)
    n_checked = 0
    for c in (0, 2):
        ext = scene["ext"][c]
        codes, _, _, rows, _ = RR.obs(T, ext, K, D, scene["frames"][0][c], X, nw, nr, ng, f)
        for k in np.flatnonzero(codes == 0)[::40]:
            i = cand[k]
            axis = 0 if f[i] == 1 else 1
            _, _, m0, nh, _, _ = RR.np_geometry(T, ext, X[i], axis)

            def fn(d6):
                Td = RR.exp_right(T, d6)
                p = np.linalg.inv(Td @ ext) @ np.append(X[i], 1.0)
                return nh @ (p[:2] / p[2] - m0)

            h = 1e-6
            num = np.array([(fn(h * np.eye(6)[a]) - fn(-h * np.eye(6)[a])) / (2 * h) for a in range(6)])
            np.testing.assert_allclose(rows[k, :6], num, rtol=0, atol=1e-8)
            n_checked += 1
    assert n_checked >= 10


def test_seq_refines_a_four_camera_rig(lm, scene):
    X, nw, nr, ng = lm
    T = scene["Twb"][0]
    T0 = RR.shift(T)
    res = RR.seq(T0, scene["ext"], scene["frames"][0], X, nw, nr, ng, RR.default_params())
    Tr = np.array(res.T_w_b).reshape(4, 4)
    d0, a0 = RR.pose_dist(T0, T)
    d1, a1 = RR.pose_dist(Tr, T)
    print(f"start {100 * d0:.3f} cm / {a0:.4f} deg -> {100 * d1:.4f} cm / {a1:.4f} deg; n_obs {list(res.n_obs)} "
          f"rms x fx {[round(r * 323.15, 3) for r in res.rms]}")
    assert res.status == 0 and res.refined == 1 and res.iterations_run == 4 and res.n_cand == 540
    assert d1 < d0 and a1 < a0
    # the passes' deltas compose to the result
    Tc = T0
    for k in range(res.iterations_run):
        Tc = RR.exp_right(Tc, np.array(res.delta[k]))
    np.testing.assert_allclose(Tc, Tr, rtol=0, atol=1e-12)
    assert all(res.n_obs[k] == 0 and res.rms[k] == 0 for k in range(5, 11))
    # the gate on the final rms
    tight = RR.seq(T0, scene["ext"], scene["frames"][0], X, nw, nr, ng, RR.default_params(max_rms=res.rms[4] * 0.5))
    assert tight.refined == 0 and tight.status == 0 and np.array_equal(np.array(tight.T_w_b), np.array(res.T_w_b))
    loose = RR.seq(T0, scene["ext"], scene["frames"][0], X, nw, nr, ng, RR.default_params(max_rms=res.rms[4]))
    assert loose.refined == 1


def test_seq_degenerate_cases(lm, scene):
    X, nw, nr, ng = lm
    T0 = RR.shift(scene["Twb"][0])
    # I = 0: one observation pass, the pose comes back bit for bit
    res = RR.seq(T0, scene["ext"], scene["frames"][0], X, nw, nr, ng, RR.default_params(iterations=0))
    assert np.array_equal(np.array(res.T_w_b).reshape(4, 4), T0)
    assert res.status == 0 and res.iterations_run == 0 and res.n_obs[0] > 1000 and res.refined == 1
    assert not np.array(res.delta).any()
    # a blind rig: every camera looks up
    blind = [np.eye(4)] * 4
    res = RR.seq(T0, blind, scene["frames"][0], X, nw, nr, ng, RR.default_params())
    assert res.status == 1 and res.refined == 0 and res.iterations_run == 0 and res.n_obs[0] == 0
    assert np.array_equal(np.array(res.T_w_b).reshape(4, 4), T0)
    assert not np.array(res.covariance).any() and res.rms[0] == 0
    # one camera of a 12 x 12 black frame: singular is STARVED first (no rows at all)
    res = RR.seq(T0, scene["ext"][:1], [np.zeros((12, 12, 3), np.uint8)], X, nw, nr, ng, RR.default_params(),
                 *synth.intrinsics(W, H))
    assert res.status == 1 and res.refined == 0


def test_singular_system():
    """Rows that constrain one direction only: gn_solve6 fails, the gate's covariance is zeros."""
    import mantis_amd as M

    rows = np.zeros((20, 7))
    rows[:, 0] = 1.0
    rows[:, 6] = 0.01
    acc = RR.accumulate(rows)
    assert np.allclose(acc, RR.np_acc28(rows), rtol=1e-14, atol=0)
    ok, Tn, d6 = RR.solve6(acc, 0.0, np.eye(4))
    assert not ok and np.array_equal(Tn, np.eye(4))
    R = M.MantisRefineResult()
    for i in range(16):
        R.T_w_b[i] = np.eye(4).reshape(16)[i]
    R.n_obs[0] = 20
    R.rms[0] = 0.01
    RR.hc().hc_refine_conclude(acc.ctypes.data, 12, 0.0, C.byref(R))
    assert R.refined == 0 and not np.array(R.covariance).any()
    # with a damping the same system solves
    ok, Tn, d6 = RR.solve6(acc, 1e-3, np.eye(4))
    assert ok and abs(d6[0] + 0.2 / (20 + 1e-3)) < 1e-15


def test_covariance(lm, scene):
    X, nw, nr, ng = lm
    K, D = synth.intrinsics(W, H)
    T0 = RR.shift(scene["Twb"][0])
    res = RR.seq(T0, scene["ext"], scene["frames"][0], X, nw, nr, ng, RR.default_params())
    Tr = np.array(res.T_w_b).reshape(4, 4)
    f = RR.flags(X, 0.08)
    rows, n = [], 0
    for c in range(4):
        codes, _, _, r, _ = RR.obs(Tr, scene["ext"][c], K, D, scene["frames"][0][c], X, nw, nr, ng, f)
        rows.append(r)
        n += int((codes == 0).sum())
    acc = RR.accumulate(np.concatenate(rows))
    assert n == res.n_obs[4] and res.rms[4] == math.sqrt(acc[27] / n)
    cov = np.array(res.covariance).reshape(6, 6)
    assert np.array_equal(cov, cov.T)
    assert np.all(np.linalg.eigvalsh(cov) > 0)
    ref, A = RR.np_covariance(acc, n, Tr)
    # both invert A in doubles: the relative error is bounded by a small multiple of cond(A) eps
    tol = 100 * np.linalg.cond(A) * np.finfo(np.float64).eps
    assert tol < 1e-6
    np.testing.assert_allclose(cov, ref, rtol=0, atol=tol * np.abs(ref).max())
    sd = np.sqrt(np.diag(cov))
    print("sigma (m, rad):", sd)
    assert np.all(sd[:3] < 5e-3) and np.all(sd[3:] < 5e-3)  # a measurement's scale, not the set's scatter


def test_struct_sizes_defaults_and_null_arguments():
    import mantis_amd as M

    L = M.lib()
    p = M.MantisRefineParams()
    L.mantis_default_refine_params(C.byref(p))
    assert p.struct_size == C.sizeof(M.MantisRefineParams)
    assert (p.iterations, p.half_window, p.white_thresh, p.min_weight, p.min_obs) == (4, 12, 12288, 24576, 12)
    assert (p.lambda_, p.landmark_pitch, p.max_rms, p.record) == (0.0, 0.08, 0.0, 0)
    a, b = C.c_int32(), C.c_int32()
    L.mantis_refine_sizes(C.byref(a), C.byref(b))
    assert a.value == C.sizeof(M.MantisRefineParams) == RR.hc().hc_sizeof_refine_params()
    assert b.value == C.sizeof(M.MantisRefineResult) == RR.hc().hc_sizeof_refine_result()
    assert L.mantis_abi_version() == 5
    L.mantis_default_refine_params(None)
    L.mantis_refine_sizes(None, None)
    # null context / arguments are argument errors, not crashes
    assert L.mantis_refine_batch(None, None, 1, 1, None, None, None) == 1
    assert L.mantis_refine(None, None, 1, None, None, None, None) == 1
    assert L.mantis_get_refine_record(None, 0, 0, None, None, None, None, None, None) == 1
    assert L.mantis_refine_line_flags(None, 0.08, None, 0) == 1
