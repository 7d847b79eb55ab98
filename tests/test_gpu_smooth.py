"""Window smoothing on the GPU (mantis_smooth_batch): every recorded pass
against the host build of the same rules -- the views' slots against
hc_refine_obs at the device's own recorded poses, the MFMA accumulators against
numpy sums, the factors against hc_smooth_between / hc_smooth_prior, the step
against hc_smooth_solve on blocks assembled from the device's own records, the
figures from the record -- the whole call against hc_smooth_seq, the shapes
that break loops, the plumbing around the context and the argument errors.
Synthetic trajectories (tests/_smooth_ref.py).
"""
import ctypes as C
import math

import numpy as np
import pytest

import _refine_ref as RR
import _smooth_ref as SR
from mantis_amd import synth

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-9
W, H = RR.W, RR.H_
SW, SH = 322, 242


@pytest.fixture(scope="module")
def mantis(landmark_map):
    import mantis_amd as M

    m = M.Mantis(max_cams=20, max_width=W, max_height=H)
    m.set_map(*landmark_map)
    yield m
    m.close()


@pytest.fixture(scope="module")
def small(landmark_map):
    """A context for the 322 x 242 windows (up to 65 one-camera views)."""
    import mantis_amd as M

    m = M.Mantis(max_cams=66, max_width=SW, max_height=SH)
    m.set_map(*landmark_map)
    yield m
    m.close()


@pytest.fixture(scope="module")
def lm(landmark_map):
    return RR.all_landmarks(landmark_map)


@pytest.fixture(scope="module")
def blind5():
    return SR.trajectory(5, blind=(2,))


@pytest.fixture(scope="module")
def small5():
    return SR.trajectory(5, n_cams=2, w=SW, h=SH, cfg=19)


def _images(frames, exts, pitched=None):
    """MantisImage list of frames[k][c] (view-major); pitched: a list that keeps row-padded copies alive
    (step_bytes = 1000 for the 322-wide frames)."""
    import mantis_amd as M

    h, w = frames[0][0].shape[:2]
    K, D = synth.intrinsics(w, h)
    out = []
    for fr in frames:
        for f, e in zip(fr, exts):
            im = M.make_image(f, K, D, T_base_cam=e)
            if pitched is not None:
                buf = np.full((h, 3 * w + 34), 0xAB, np.uint8)
                buf[:, : 3 * w] = f.reshape(h, 3 * w)
                pitched.append(buf)
                im.bgr = buf.ctypes.data
                im.step_bytes = buf.strides[0]
            out.append(im)
    return out


def _check_call(m, lm, frames, exts, T0, motions, prior=None, landmarks=None, pitched=None, **params):
    """One window, record = 1: every pass against the host rules, then the whole call; returns (result, views)."""
    X, nw, nr, ng = landmarks or lm
    N, Cn = len(frames), len(frames[0])
    h, w = frames[0][0].shape[:2]
    K, D = synth.intrinsics(w, h)
    T0 = np.asarray(T0, np.float64).reshape(N, 4, 4)
    pT, pC = prior if prior is not None else (None, None)
    res, views = m.smooth_batch(_images(frames, exts, pitched), 1, N, T0, motions, pT, pC, record=1, **params)
    res, views = res[0], views[0]
    p = m.smooth_params(**params)
    f = RR.flags(X, p.landmark_pitch)
    nc = len(RR.candidates(f))
    assert res.n_cand == nc and res.n_views == N and res.has_prior == int(prior is not None)
    mo = np.zeros((0, 7)) if motions is None else np.asarray(motions, np.float64).reshape(-1, 7)
    tr = [SR.transform(q) for q in mo]
    has = np.array([int(t[0]) for t in tr], np.int32)
    assert res.n_factors == int(has.sum())
    wt, wr = p.sigma_row / p.sigma_t, p.sigma_row / p.sigma_rot
    flagged = total = 0
    T_prev = None
    for q in range(res.iterations_run + 1):
        e, J, pe, pJ, delta = m.smooth_pass_record(0, q)
        Ts, accs, ns = [], [], []
        for k in range(N):
            T, codes, Sw, Skw, rows, acc = m.smooth_record(0, k, q)
            Ts.append(T)
            accs.append(acc)
            assert codes.shape == (Cn * nc,)
            for c in range(Cn):
                hc_, hSw, hSkw, hrows, tie = RR.obs(T, exts[c], K, D, frames[k][c], X, nw, nr, ng, f, R=p.half_window,
                                                     white_thresh=p.white_thresh, min_weight=p.min_weight)
                sl = slice(c * nc, (c + 1) * nc)
                ok = tie == 0
                flagged += int((~ok).sum())
                total += nc
                assert np.array_equal(codes[sl][ok], hc_[ok]), f"pass {q} view {k} camera {c}: codes"
                assert np.array_equal(Sw[sl][ok], hSw[ok]) and np.array_equal(Skw[sl][ok], hSkw[ok]), (q, k, c)
                np.testing.assert_allclose(rows[sl][ok], hrows[ok], rtol=1e-12, atol=0, err_msg=f"pass {q} view {k} cam {c}")
            assert np.all(rows[codes != 0] == 0.0)
            ns.append(int((codes == 0).sum()))
            ref = RR.np_acc28(rows)
            np.testing.assert_allclose(acc, ref, rtol=1e-12, atol=1e-14 * max(np.abs(ref).max(), 1e-300))
        if q == 0:
            assert np.array_equal(np.array(Ts), T0), "pass 0 observes at the input poses"
        for k in range(N - 1):
            if has[k]:
                he, hJa, hJb = SR.between(Ts[k], Ts[k + 1], tr[k][1], wt, wr)
                np.testing.assert_allclose(e[k], he, rtol=1e-12, atol=1e-12, err_msg=f"pass {q} step {k}: e")
                np.testing.assert_allclose(J[k, 0], hJa, rtol=1e-12, atol=1e-12, err_msg=f"pass {q} step {k}: Ja")
                np.testing.assert_allclose(J[k, 1], hJb, rtol=1e-12, atol=1e-12, err_msg=f"pass {q} step {k}: Jb")
            else:
                assert not e[k].any() and not J[k].any()
        if prior is not None:
            okp, hpe, hpJ = SR.prior(Ts[0], pT, pC, p.sigma_row)
            assert okp
            np.testing.assert_allclose(pe, hpe, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(pJ, hpJ, rtol=1e-12, atol=1e-12)
        else:
            assert not pe.any() and not pJ.any()
        n, nf, rms, mrms, cost = SR.sums(ns, accs, has, e, p.sigma_row, pe if prior is not None else None)
        assert (res.n_obs[q], res.n_factors) == (n, nf)
        np.testing.assert_allclose([res.rms[q], res.motion_rms[q], res.cost[q]], [rms, mrms, cost], rtol=1e-14, atol=0)
        if q == res.iterations_run:
            assert not delta.any()
            for k in range(N):
                assert views[k].n_obs == ns[k]
                assert np.array_equal(np.array(views[k].T_w_b).reshape(4, 4), Ts[k])
            break
        Hd, Ho, g = SR.assemble(accs, has, e, J, p.lambda_, pe if prior is not None else None,
                                pJ if prior is not None else None)
        bad, x = SR.solve(Hd, Ho, g, has)
        assert bad == -1
        np.testing.assert_allclose(delta, x, rtol=0, atol=1e-12, err_msg=f"pass {q}: delta")
        T_prev = Ts
        Tn = [m.smooth_record(0, k, q + 1)[0] for k in range(N)]
        for k in range(N):
            np.testing.assert_allclose(Tn[k], RR.exp_right(Ts[k], delta[k]), rtol=0, atol=1e-12, err_msg=f"step {q} view {k}")
    assert flagged <= 0.005 * total, (flagged, total)
    if flagged == 0:
        host = SR.seq(T0, motions, exts, frames, X, nw, nr, ng, p, pT, pC)
        hr = host.res
        assert (res.status, res.smoothed, res.iterations_run, res.dof) == (hr.status, hr.smoothed, hr.iterations_run, hr.dof)
        assert list(res.n_obs) == list(hr.n_obs)
        dev = np.array([np.array(v.T_w_b).reshape(4, 4) for v in views])
        np.testing.assert_allclose(dev, host.poses, rtol=0, atol=POSE_TOL)
        np.testing.assert_allclose(list(res.rms), list(hr.rms), rtol=0, atol=POSE_TOL)
        np.testing.assert_allclose(list(res.motion_rms), list(hr.motion_rms), rtol=0, atol=POSE_TOL)
        np.testing.assert_allclose(list(res.cost), list(hr.cost), rtol=0, atol=POSE_TOL)
        assert res.n_factors == hr.n_factors
        if res.smoothed:
            for k in range(N):
                hcov = np.array(host.views[k].covariance)
                np.testing.assert_allclose(np.array(views[k].covariance), hcov, rtol=0, atol=1e-8 * np.abs(hcov).max())
    return res, views


def _chain(sc, views, noise=(0.002, 0.005)):
    """(frames, T0, motions) of the views `views` (consecutive) of a trajectory, the motions off by `noise`
    so that every factor works at e != 0."""
    mo = SR.noisy_motions(sc, *noise)
    return [sc["frames"][k] for k in views], SR.starts(sc)[list(views)], mo[views[0]: views[-1]]


def test_one_view_equals_refine_batch(mantis, lm, blind5):
    """N = 1: the bytes of mantis_refine_batch on that view (pose, counts, rms, status)."""
    sc = blind5
    T0 = RR.shift(sc["Twb"][0])
    res, views = _check_call(mantis, lm, [sc["frames"][0]], sc["ext"], [T0], None)
    one = mantis.refine_batch(_images([sc["frames"][0]], sc["ext"]), 1, T0)[0]
    assert bytes(views[0].T_w_b) == bytes(one.T_w_b)
    assert list(res.n_obs) == list(one.n_obs) and list(res.rms) == list(one.rms)
    for q in range(one.iterations_run):
        assert mantis.smooth_pass_record(0, q)[4][0].tobytes() == bytes(one.delta[q]), f"delta of pass {q}"
    assert (res.status, res.iterations_run, res.smoothed) == (one.status, one.iterations_run, one.refined) == (0, 4, 1)
    assert res.n_factors == 0 and list(res.motion_rms) == [0.0] * 11 and res.dof == res.n_obs[4] - 6
    hcov = np.array(one.covariance)
    np.testing.assert_allclose(np.array(views[0].covariance), hcov, rtol=0, atol=1e-8 * np.abs(hcov).max())


def test_two_views_one_camera(small, lm, small5):
    fr, T0, mo = _chain(small5, [0, 1])
    res, _ = _check_call(small, lm, [f[:1] for f in fr], small5["ext"][:1], T0, mo)
    assert res.n_factors == 1 and res.status == 0 and res.iterations_run == 4
    print("N=2 C=1:", res.status, res.smoothed, res.iterations_run, list(res.n_obs)[:5], list(res.motion_rms)[:5])


def test_blind_middle_view(mantis, lm, blind5):
    """N = 3, C = 4 at 1280 x 720, the middle view black: its factors hold it."""
    fr, T0, mo = _chain(blind5, [1, 2, 3])
    res, views = _check_call(mantis, lm, fr, blind5["ext"], T0, mo)
    assert (res.status, res.smoothed, res.iterations_run, res.n_factors) == (0, 1, 4, 2)
    assert views[1].n_obs == 0 and views[0].n_obs > 1000 and views[2].n_obs > 1000
    assert np.all(np.diag(np.array(views[1].covariance).reshape(6, 6)) > 0)


def test_broken_chain(small, lm, small5):
    """N = 5, C = 2, step 2 unset: two segments in one system, and the same poses as the segments' own calls."""
    fr, T0, mo = _chain(small5, [0, 1, 2, 3, 4])
    mo = mo.copy()
    mo[2] = SR.UNSET
    res, views = _check_call(small, lm, fr, small5["ext"], T0, mo)
    assert res.status == 0 and res.n_factors == 3
    whole = np.array([np.array(v.T_w_b) for v in views])
    _, a = small.smooth_batch(_images(fr[:3], small5["ext"]), 1, 3, T0[:3], mo[:2])
    _, b = small.smooth_batch(_images(fr[3:], small5["ext"]), 1, 2, T0[3:], mo[3:])
    parts = np.array([np.array(v.T_w_b) for v in a[0] + b[0]])
    np.testing.assert_allclose(whole, parts, rtol=0, atol=1e-12)


def test_prior_from_a_previous_call(mantis, lm, blind5):
    """N = 5 with a prior on view 0 taken from a previous call's view (its pose and covariance)."""
    sc = blind5
    fr, T0, mo = _chain(sc, [0, 1, 2, 3, 4])
    _, first = mantis.smooth_batch(_images(fr[:2], sc["ext"]), 1, 2, T0[:2], mo[:1])
    assert np.array(first[0][0].covariance).any()
    pT = np.array(first[0][0].T_w_b).reshape(4, 4)
    pC = np.array(first[0][0].covariance).reshape(6, 6)
    res, views = _check_call(mantis, lm, fr, sc["ext"], T0, mo, prior=(pT, pC))
    assert (res.status, res.smoothed, res.has_prior, res.n_factors) == (0, 1, 1, 4)
    assert res.dof == res.n_obs[4] + 24 + 6 - 30


def test_sixty_five_views(small, lm):
    """N = 65, C = 1, 322 x 242 frames with step_bytes = 1000, I = 2: the per-view phases of k_smooth_solve
    cross the first wave."""
    steps = [SR.step(dx=0.012, yaw_deg=5.0 if k % 2 else -4.0, dy=0.004 if k % 3 else -0.006) for k in range(64)]
    sc = SR.trajectory(65, n_cams=1, w=SW, h=SH, cfg=23, steps=steps, T0=SR.start_pose(x=-0.4, y=-0.2, h=1.2))
    keep = []
    res, views = _check_call(small, lm, sc["frames"], sc["ext"], SR.starts(sc), SR.noisy_motions(sc, 0.002, 0.005),
                             pitched=keep, iterations=2)
    assert keep[0].strides[0] == 1000 > 3 * SW
    assert res.status == 0 and res.iterations_run == 2 and res.n_factors == 64 and res.n_views == 65
    print("N=65:", res.smoothed, list(res.n_obs)[:3], list(res.rms)[:3], list(res.motion_rms)[:3])


def test_odd_candidate_count(small, lm, small5, landmark_map):
    w, r, g = landmark_map
    for drop in range(1, 8):
        X = np.concatenate([w[drop:], r, g])
        nc = len(RR.candidates(RR.flags(X, 0.08)))
        if nc % 2 == 1:
            break
    assert nc % 2 == 1 and nc % 32 != 0
    fr, T0, mo = _chain(small5, [0, 1, 2])
    try:
        small.set_map(w[drop:], r, g)
        landmarks = (np.ascontiguousarray(X), len(w) - drop, len(r), len(g))
        res, _ = _check_call(small, lm, fr, small5["ext"], T0, mo, landmarks=landmarks)
        assert res.n_cand == nc and res.status == 0
    finally:
        small.set_map(w, r, g)


@pytest.mark.parametrize("cls", list(RR.ROW_CLASSES))
def test_trip_loop_tails(small, lm, small5, landmark_map, cls):
    """One view of one camera on a map cut until its n_cand rows end the accumulation's trip loop another way
    (RR.ROW_CLASSES); the small classes leave the window STARVED, its record written. k_smooth_acc and
    k_refine_step run one accumulation: pass 0's acc28 of the refinement from the same frame and pose has the
    same bytes."""
    cut, landmarks, nc = RR.cut_map(landmark_map, cls)
    fr, ext, T0 = [small5["frames"][0][:1]], small5["ext"][:1], SR.starts(small5)[:1]
    try:
        small.set_map(*cut)
        res, _ = _check_call(small, lm, fr, ext, T0, None, landmarks=landmarks)
        assert res.n_cand == nc and RR.ROW_CLASSES[cls](res.n_cand)
        print(cls, nc, res.status, res.iterations_run, list(res.n_obs)[:5])
        acc = small.smooth_record(0, 0, 0)[5]
        small.refine_batch(_images(fr, ext), 1, T0[0], record=1)
        assert small.refine_record(0, 0)[5].tobytes() == acc.tobytes()
    finally:
        small.set_map(*landmark_map)


@pytest.mark.parametrize("iterations", [0, 10])
def test_iteration_counts(small, lm, small5, iterations):
    fr, T0, mo = _chain(small5, [0, 1, 2])
    res, views = _check_call(small, lm, fr, small5["ext"], T0, mo, iterations=iterations)
    assert res.status == 0 and res.iterations_run == iterations
    if iterations == 0:
        assert np.array([np.array(v.T_w_b) for v in views]).tobytes() == np.ascontiguousarray(T0).tobytes()


def test_windows_calls_and_frames(small, small5):
    """Two windows in one call against two calls; host against device frames; the same call twice: equal bytes."""
    import mantis_amd as M

    sc = small5
    ext = sc["ext"]
    frA, TA, moA = _chain(sc, [0, 1, 2])
    frB, TB, moB = _chain(sc, [2, 3, 4])
    both, vboth = small.smooth_batch(_images(frA + frB, ext), 2, 3, np.concatenate([TA, TB]), np.concatenate([moA, moB]),
                                     record=1)
    recs = [small.smooth_record(wn, 1, 1) for wn in range(2)] + [small.smooth_pass_record(wn, 1) for wn in range(2)]
    for wn, (fr, T, mo) in enumerate([(frA, TA, moA), (frB, TB, moB)]):
        one, vone = small.smooth_batch(_images(fr, ext), 1, 3, T, mo, record=1)
        assert bytes(one[0]) == bytes(both[wn]) and one[0].status == 0
        for k in range(3):
            assert bytes(vone[0][k]) == bytes(vboth[wn][k]), (wn, k)
        for a, b in zip(small.smooth_record(0, 1, 1), recs[wn]):
            assert np.array_equal(a, b)
        for a, b in zip(small.smooth_pass_record(0, 1), recs[2 + wn]):
            assert np.array_equal(a, b)
    again, vagain = small.smooth_batch(_images(frA, ext), 1, 3, TA, moA)
    first, vfirst = small.smooth_batch(_images(frA, ext), 1, 3, TA, moA)
    assert bytes(again[0]) == bytes(first[0]) and all(bytes(a) == bytes(b) for a, b in zip(vagain[0], vfirst[0]))
    K, D = synth.intrinsics(SW, SH)
    fb = SW * SH * 3
    dev = small.device_alloc(fb * 6)
    try:
        imgs = []
        for k in range(3):
            for c in range(2):
                i = 2 * k + c
                small.h2d(dev + i * fb, frA[k][c])
                imgs.append(M.make_image(None, K, D, T_base_cam=ext[c], device_ptr=dev + i * fb, width=SW, height=SH))
        devr, vdev = small.smooth_batch(imgs, 1, 3, TA, moA)
    finally:
        small.device_free(dev)
    assert bytes(devr[0]) == bytes(first[0]) and all(bytes(a) == bytes(b) for a, b in zip(vdev[0], vfirst[0]))


def test_other_entries_undisturbed(small, small5):
    """mantis_refine_batch and mantis_calibrate_extrinsics before and after a smooth call in one context: equal
    bytes; the cv::RNG state and the context's prior pose are untouched."""
    sc = small5
    ext = sc["ext"]
    fr, T0, mo = _chain(sc, [0, 1, 2])
    flat = _images(fr, ext)
    small.rng_state = 4242
    prior = sc["Twb"][1].copy()
    small.prior_pose = prior

    def others():
        r = small.refine_batch(flat, 3, T0, record=1)
        rec = small.refine_record(1, 1)
        Tc, c = small.calibrate_extrinsics(flat, 3, T0, 0b10)
        return [bytes(x) for x in r], [a.tobytes() for a in rec], Tc.tobytes(), bytes(c)

    before = others()
    res, _ = small.smooth_batch(flat, 1, 3, T0, mo, record=1)
    assert res[0].status == 0
    after = others()
    assert before == after
    # the smoother's record outlives the other calls, and theirs outlive it
    small.smooth_record(0, 0, 0)
    assert small.rng_state == 4242 and np.array_equal(small.prior_pose, prior)
    small.prior_pose = None


def test_launch_count_and_record_errors(small, small5):
    import mantis_amd as M

    L = M.lib()
    fr, T0, mo = _chain(small5, [0, 1, 2])
    imgs = _images(fr, small5["ext"])
    fresh = M.Mantis(max_cams=6, max_width=SW, max_height=SH)
    try:
        fresh.set_map(*synth.load_map())
        z = np.zeros(64)
        assert L.mantis_get_smooth_record(fresh.h, 0, 0, 0, z.ctypes.data, None, None, None, None, None) == 5
        assert L.mantis_get_smooth_pass(fresh.h, 0, 0, None, None, z.ctypes.data, None, None) == 5  # MANTIS_ERR_STATE
        fresh.set_profiling(1)
        fresh.smooth_batch(imgs, 1, 3, T0, mo, iterations=2)
        names = [n for n, _ in fresh.kernel_times()]
        fresh.set_profiling(0)
        assert [sum(n.startswith(s) for n in names) for s in ("smooth_obs", "smooth_acc", "smooth_solve")] == [3, 3, 3]
        assert len(names) == 9, names  # 3 (I + 1)
        with pytest.raises(Exception):
            fresh.smooth_record(0, 0, 0)  # that call kept no record
        assert L.mantis_get_smooth_pass(fresh.h, 0, 0, None, None, z.ctypes.data, None, None) == 5
        res, _ = fresh.smooth_batch(imgs, 1, 3, T0, mo, iterations=2, record=1)
        assert res[0].iterations_run == 2
        for wn, k, q in [(1, 0, 0), (-1, 0, 0), (0, 3, 0), (0, -1, 0), (0, 0, 3), (0, 0, -1)]:
            assert L.mantis_get_smooth_record(fresh.h, wn, k, q, z.ctypes.data, None, None, None, None, None) == 1, (wn, k, q)
            assert "out of range" in L.mantis_last_error(fresh.h).decode()
        for wn, q in [(1, 0), (-1, 0), (0, 3), (0, -1)]:
            assert L.mantis_get_smooth_pass(fresh.h, wn, q, None, None, z.ctypes.data, None, None) == 1, (wn, q)
        assert L.mantis_get_smooth_pass(fresh.h, 0, 2, None, None, z.ctypes.data, None, None) == 0
    finally:
        fresh.close()


def test_starved_and_singular_windows(small, lm, small5):
    sc = small5
    black = [[np.zeros_like(f) for f in fr] for fr in sc["frames"][:3]]
    fr, T0, mo = _chain(sc, [0, 1, 2])
    res, views = _check_call(small, lm, black, sc["ext"], T0, mo)
    assert (res.status, res.smoothed, res.iterations_run, res.n_obs[0]) == (SR.STATUS["starved"], 0, 0, 0)
    assert np.array([np.array(v.T_w_b) for v in views]).tobytes() == np.ascontiguousarray(T0).tobytes()
    assert not np.array(views[0].covariance).any()
    with pytest.raises(Exception):
        small.smooth_record(0, 0, 1)  # the pass did not run
    mo2 = mo.copy()
    mo2[0] = SR.UNSET  # views 1, 2: an all-blind segment at lambda = 0
    res, views = _check_call(small, lm, [fr[0], black[1], black[2]], sc["ext"], T0, mo2)
    assert (res.status, res.smoothed, res.iterations_run) == (SR.STATUS["singular"], 0, 0)
    assert res.n_obs[0] == views[0].n_obs > 0
    assert np.array([np.array(v.T_w_b) for v in views]).tobytes() == np.ascontiguousarray(T0).tobytes()


def test_argument_errors(small, small5):
    import mantis_amd as M

    L = M.lib()
    sc = small5
    fr, T0, mo = _chain(sc, [0, 1, 2])
    imgs = _images(fr, sc["ext"])
    small.rng_state = 77
    small.set_profiling(1)
    big = M.make_image(np.zeros((SH - 2, SW - 2, 3), np.uint8), *synth.intrinsics(SW - 2, SH - 2))
    eye = np.eye(6)

    def call(images, wn, N, Cn, T=T0, motions=mo, pT=None, pC=None, out_null=False, **kw):
        n = len(images)
        arr = (M.MantisImage * n)(*images)
        p = small.smooth_params()
        for k, v in kw.items():
            setattr(p, k, v)
        out = (M.MantisSmoothResult * max(wn, 1))()
        vw = (M.MantisSmoothView * max(wn * N, 1))()
        keep = [None if a is None else np.ascontiguousarray(a, np.float64) for a in (T, motions, pT, pC)]
        args = [None if a is None else a.ctypes.data for a in keep]
        st = L.mantis_smooth_batch(small.h, arr, wn, N, Cn, args[0], args[1], args[2], args[3], C.byref(p),
                                   None if out_null else out, vw)
        return st, L.mantis_last_error(small.h).decode()

    nanT, nanM, nanQ = T0.copy(), mo.copy(), mo.copy()
    nanT[1, 0, 3] = float("nan")
    nanM[0, 1] = float("nan")
    nanQ[1, 5] = float("nan")
    notpd = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, -1e-3])
    nancov = eye.copy()
    nancov[0, 0] = float("inf")
    bad = [
        (dict(images=imgs * 43, wn=1, N=257, Cn=1, T=np.tile(T0[:1], (257, 1, 1)), motions=np.tile(mo[:1], (256, 1))), "n_views"),
        (dict(images=imgs * 3, wn=1, N=2, Cn=9, T=T0[:2], motions=mo[:1]), "cams_per_rig"),
        (dict(images=imgs * 12, wn=12, N=3, Cn=2, T=np.tile(T0, (12, 1, 1)), motions=np.tile(mo, (12, 1))), "max_cams"),
        (dict(images=imgs[:5] + [big], wn=1, N=3, Cn=2), "size"),
        (dict(images=imgs, wn=0, N=3, Cn=2), "n_windows"),
        (dict(images=imgs, wn=1, N=3, Cn=2, struct_size=8), "struct_size"),
        (dict(images=imgs, wn=1, N=3, Cn=2, iterations=-1), "iterations"),
        (dict(images=imgs, wn=1, N=3, Cn=2, iterations=11), "iterations"),
        (dict(images=imgs, wn=1, N=3, Cn=2, half_window=0), "half_window"),
        (dict(images=imgs, wn=1, N=3, Cn=2, half_window=16), "half_window"),
        (dict(images=imgs, wn=1, N=3, Cn=2, white_thresh=0), "white_thresh"),
        (dict(images=imgs, wn=1, N=3, Cn=2, min_weight=0), "min_weight"),
        (dict(images=imgs, wn=1, N=3, Cn=2, min_obs=5), "min_obs"),
        (dict(images=imgs, wn=1, N=3, Cn=2, lambda_=-1e-9), "lambda"),
        (dict(images=imgs, wn=1, N=3, Cn=2, landmark_pitch=0.0), "landmark_pitch"),
        (dict(images=imgs, wn=1, N=3, Cn=2, max_rms=float("nan")), "max_rms"),
        (dict(images=imgs, wn=1, N=3, Cn=2, sigma_row=0.0), "sigma_row"),
        (dict(images=imgs, wn=1, N=3, Cn=2, sigma_t=float("inf")), "sigma_t"),
        (dict(images=imgs, wn=1, N=3, Cn=2, sigma_rot=-1.0), "sigma_rot"),
        (dict(images=imgs, wn=1, N=3, Cn=2, record=2), "record"),
        (dict(images=imgs, wn=1, N=3, Cn=2, T=nanT), "T_w_b_in"),
        (dict(images=imgs, wn=1, N=3, Cn=2, motions=nanM), "delta_pos"),
        (dict(images=imgs, wn=1, N=3, Cn=2, motions=nanQ), "delta_quat"),
        (dict(images=imgs, wn=1, N=3, Cn=2, motions=None), "motions"),
        (dict(images=imgs, wn=1, N=3, Cn=2, pT=T0[0], pC=None), "prior_cov"),
        (dict(images=imgs, wn=1, N=3, Cn=2, pT=T0[0], pC=notpd), "prior_cov"),
        (dict(images=imgs, wn=1, N=3, Cn=2, pT=T0[0], pC=nancov), "prior_cov"),
        (dict(images=imgs, wn=1, N=3, Cn=2, pT=nanT[1], pC=eye), "prior_T"),
        (dict(images=imgs, wn=1, N=3, Cn=2, out_null=True), "null"),
    ]
    for kw, word in bad:
        st, msg = call(**kw)
        assert st == 1 and word in msg, (word, st, msg)  # MANTIS_ERR_ARG
    assert small.rng_state == 77
    m2 = M.Mantis(max_cams=6, max_width=SW, max_height=SH)
    try:
        arr = (M.MantisImage * 6)(*imgs)
        p = m2.smooth_params()
        out, vw = M.MantisSmoothResult(), (M.MantisSmoothView * 3)()
        T = np.ascontiguousarray(T0)
        assert L.mantis_smooth_batch(m2.h, arr, 1, 3, 2, T.ctypes.data, mo.ctypes.data, None, None, C.byref(p),
                                     C.byref(out), vw) == 1
        assert "map" in L.mantis_last_error(m2.h).decode()
    finally:
        m2.close()
    # nothing was launched by the rejected calls: the next call's stage marks are exactly its own
    small.smooth_batch(imgs, 1, 3, T0, mo, iterations=1)
    names = [n for n, _ in small.kernel_times()]
    small.set_profiling(0)
    assert len(names) == 6 and all(n.startswith("smooth_") for n in names), names


def test_the_blind_view_is_recovered_on_the_device(mantis, lm, blind5):
    """The CPU test's scene and conditions, on the device."""
    X, nw, nr, ng = lm
    sc = blind5
    T0 = SR.starts(sc)
    imgs = _images(sc["frames"], sc["ext"])
    own = mantis.refine_batch(imgs, 5, T0)
    for k in (0, 1, 3, 4):
        assert own[k].status == 0 and own[k].refined == 1, k
    assert own[2].status == SR.STATUS["starved"]
    for name, mo in (("exact", SR.exact_motions(sc)), ("noisy", SR.noisy_motions(sc))):
        res, views = mantis.smooth_batch(imgs, 1, 5, T0, mo)
        res, views = res[0], views[0]
        assert (res.status, res.smoothed, res.iterations_run, res.n_factors) == (0, 1, 4, 4)
        poses = [np.array(v.T_w_b).reshape(4, 4) for v in views]
        s_t, s_a = RR.pose_dist(T0[2], sc["Twb"][2])
        e_t, e_a = RR.pose_dist(poses[2], sc["Twb"][2])
        print(f"{name} motions: blind view {s_t * 100:.3f} cm / {s_a:.3f} deg -> {e_t * 100:.4f} cm / {e_a:.4f} deg, "
              f"motion_rms {res.motion_rms[4]:.4f}")
        apart = [RR.pose_dist(poses[k], np.array(own[k].T_w_b).reshape(4, 4))[0] for k in (0, 1, 3, 4)]
        print(f"{name} motions: sighted views apart from their own refinement (cm): {[round(100 * a, 4) for a in apart]}")
        if name == "exact":
            assert e_t <= 0.25 * s_t and e_a <= 0.25 * s_a
            assert max(apart) <= 1e-4
