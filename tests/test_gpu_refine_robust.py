"""Robust rows of the line refinement on the GPU (mantis_refine_set_robust,
k_refine_step_robust): every recorded pass against the host build of the same
rules fed the device's own recorded Sw / Skw (keys, median and scale exact,
weights to rtol 1e-14, the counts exact), the weighted MFMA accumulators
against numpy sums of sqrt(w) x the recorded rows, each step against gn_solve6
on the device's accumulators, the whole call against hc_refine_seq_robust; the
shapes that break the selection and the chunked accumulation; batch and modes
against single calls, byte for byte; the switch off; rigs with one drifted
camera; errors and what must stay undisturbed. 1280x720 synthetic rigs
(tests/_refine_ref.py, tests/_refine_robust_ref.py).

Distances to the truth on the rigs with one drifted camera (host build; the
device's figures are printed by test_one_drifted_camera_on_the_device):
plain 0.290 / 0.213 / 0.287 cm, Huber 0.108 / 0.074 / 0.088 cm, Tukey 0.047 /
0.035 / 0.049 cm.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _refine_ref as RR
import _refine_robust_ref as RB
from mantis_amd import synth

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-9
W, H = RR.W, RR.H_
OK, ERR_ARG, ERR_STATE = 0, 1, 5
LOSSES = ["huber", "tukey"]


@pytest.fixture(scope="module")
def mantis(landmark_map):
    import mantis_amd as M

    m = M.Mantis(max_cams=12, max_width=W, max_height=H)
    m.set_map(*landmark_map)
    yield m
    m.close()


@pytest.fixture(autouse=True)
def _switch_off_afterwards(mantis):
    yield
    mantis.set_refine_robust(None)


@pytest.fixture(scope="module")
def lm(landmark_map):
    return RR.all_landmarks(landmark_map)


@pytest.fixture(scope="module")
def rigs4():
    return RB.rigs4()


@pytest.fixture(scope="module")
def ring8():
    return RR.rig_scene(8, 1)


def _images(frames, exts, w=W, h=H, Ks=None, Ds=None):
    import mantis_amd as M

    Ks, Ds = RR.lenses(len(frames), w, h, Ks, Ds)
    return [M.make_image(f, K, D, T_base_cam=e) for f, e, K, D in zip(frames, exts, Ks, Ds)]


def _check_call(m, lm, frames, exts, T0, loss, landmarks=None, Ks=None, Ds=None, **params):
    """One rig with the robust rows on, record = 1: every pass against the host rules; (result, stats).
    Ks, Ds: per-camera lenses (default: the bench lens)."""
    X, nw, nr, ng = landmarks or lm
    h, w = frames[0].shape[:2]
    Cn = len(frames)
    Ks, Ds = RR.lenses(Cn, w, h, Ks, Ds)
    rb = RB.robust_params(loss)
    m.set_refine_robust(loss)
    res = m.refine_batch(_images(frames, exts, w, h, Ks, Ds), 1, T0, record=1, **params)[0]
    st = m.refine_robust_stats(0)
    assert st.loss == rb.loss
    p = m.refine_params(**params)
    f = RR.flags(X, p.landmark_pitch)
    nc = len(RR.candidates(f))
    assert res.n_cand == nc
    flagged = 0
    Ts, accs = [], []
    for k in range(res.iterations_run + 1):
        T, codes, Sw, Skw, rows, acc = m.refine_record(0, k)
        keys, wts = m.refine_robust_record(0, k)
        Ts.append(T)
        accs.append(acc)
        assert codes.shape == keys.shape == wts.shape == (Cn * nc,)
        # the plain record still holds the unweighted rows: the host's, at the device's pose
        for c in range(Cn):
            hc_, hSw, hSkw, hrows, tie = RR.obs(T, exts[c], Ks[c], Ds[c], frames[c], X, nw, nr, ng, f,
                                                 R=p.half_window, white_thresh=p.white_thresh,
                                                 min_weight=p.min_weight)
            sl = slice(c * nc, (c + 1) * nc)
            ok = tie == 0
            flagged += int((~ok).sum())
            assert np.array_equal(codes[sl][ok], hc_[ok]) and np.array_equal(Sw[sl][ok], hSw[ok])
            assert np.array_equal(Skw[sl][ok], hSkw[ok]), f"pass {k} camera {c}"
            np.testing.assert_allclose(rows[sl][ok], hrows[ok], rtol=1e-12, atol=0, err_msg=f"pass {k} camera {c}")
        # keys, median, scale: exact; weights: rtol 1e-14; counts: exact
        assert np.array_equal(keys, RB.keys_of(codes, Sw, Skw)), f"pass {k}: keys"
        host = RB.weights(keys, codes, rb)
        assert st.median_key[k] == host["median"] == RB.py_median(keys, codes), f"pass {k}: median"
        assert st.scale[k] == host["scale"], f"pass {k}: scale"
        np.testing.assert_allclose(wts, host["w"], rtol=1e-14, atol=0, err_msg=f"pass {k}: weights")
        assert not wts[codes != 0].any() and not keys[codes != 0].any()
        n_obs = int((codes == 0).sum())
        assert res.n_obs[k] == n_obs == host["n_obs"]
        assert (st.n_down[k], st.n_zero[k]) == (host["n_down"], host["n_zero"]), f"pass {k}: counts"
        live = codes == 0
        assert (st.n_down[k], st.n_zero[k]) == (int((wts[live] < 1).sum()), int((wts[live] == 0).sum()))
        np.testing.assert_allclose(st.sum_w[k], wts.sum(), rtol=1e-12, atol=0)
        ref = RR.np_acc28(np.sqrt(wts)[:, None] * rows)
        np.testing.assert_allclose(acc, ref, rtol=1e-12, atol=1e-14 * max(np.abs(ref).max(), 1e-300))
        assert res.rms[k] == (math.sqrt(acc[27] / n_obs) if n_obs else 0.0)
    for k in range(res.iterations_run + 1, 11):
        assert (st.median_key[k], st.n_down[k], st.n_zero[k], st.scale[k], st.sum_w[k]) == (0, 0, 0, 0.0, 0.0)
    assert np.array_equal(Ts[0], np.asarray(T0)), "pass 0 observes at the input pose"
    for k in range(res.iterations_run):
        ok, Tn, d6 = RR.solve6(accs[k], p.lambda_, Ts[k])
        assert ok
        np.testing.assert_allclose(Ts[k + 1], Tn, rtol=0, atol=1e-12, err_msg=f"step {k}")
        np.testing.assert_allclose(np.array(res.delta[k]), d6, rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.array(res.T_w_b).reshape(4, 4), Ts[-1], rtol=0, atol=0)
    if flagged == 0:
        host, hst = RB.seq_robust(T0, exts, frames, X, nw, nr, ng, p, rb, Ks, Ds)
        np.testing.assert_allclose(np.array(res.T_w_b), np.array(host.T_w_b), rtol=0, atol=POSE_TOL)
        assert list(res.n_obs) == list(host.n_obs)
        assert (res.iterations_run, res.refined, res.status) == (host.iterations_run, host.refined, host.status)
    return res, st


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("shape", ["four-cameras", "one-camera", "eight-cameras"])
def test_record_parity(mantis, lm, rigs4, ring8, shape, loss):
    """Eight cameras are 4320 slots: three chunks of the accumulation, more slots than histogram bins."""
    sc = ring8 if shape == "eight-cameras" else rigs4
    cams = {"one-camera": [0], "eight-cameras": list(range(8))}.get(shape, [0, 1, 2, 3])
    T = sc["Twb"][0]
    T0 = RR.shift(T)
    res, st = _check_call(mantis, lm, [sc["frames"][0][c] for c in cams], [sc["ext"][c] for c in cams], T0, loss)
    Tr = np.array(res.T_w_b).reshape(4, 4)
    k = res.iterations_run
    print(shape, loss, res.status, res.refined, k, list(res.n_obs)[:5], list(st.n_down)[:5], list(st.n_zero)[:5],
          [round(s, 3) for s in st.scale[:5]], RR.pose_dist(Tr, T))
    assert res.status == 0 and res.refined == 1 and k == 4
    assert st.n_down[k] > 0 and (loss == "tukey" or not any(st.n_zero))
    d0, a0 = RR.pose_dist(T0, T)
    d1, a1 = RR.pose_dist(Tr, T)
    assert d1 < d0 and a1 < a0


@pytest.mark.parametrize("loss", LOSSES)
def test_odd_candidate_count(mantis, lm, rigs4, landmark_map, loss):
    w, r, g = landmark_map
    for drop in range(1, 8):
        X = np.concatenate([w[drop:], r, g])
        nc = len(RR.candidates(RR.flags(X, 0.08)))
        if nc % 2 == 1:
            break
    assert nc % 2 == 1 and nc % 32 != 0
    try:
        mantis.set_map(w[drop:], r, g)
        landmarks = (np.ascontiguousarray(X), len(w) - drop, len(r), len(g))
        res, st = _check_call(mantis, lm, rigs4["frames"][0][:3], rigs4["ext"][:3], RR.shift(rigs4["Twb"][0]), loss,
                              landmarks=landmarks)
        assert res.n_cand == nc and res.refined == 1
    finally:
        mantis.set_map(w, r, g)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("cls,Cn", RR.TAIL_CASES)
def test_trip_loop_tails(mantis, lm, rigs4, landmark_map, cls, Cn, loss):
    """Cn cameras on a map cut until the rig's Cn n_cand rows end the weighted accumulation's trip loop another
    way (RR.ROW_CLASSES, RR.TAIL_CASES), all inside one 2048-row chunk; the eight-camera rig of test_record_parity
    is the case that crosses the chunk and the kept keys. The smallest class leaves the pass STARVED, its record
    written."""
    cut, landmarks, nc = RR.cut_map(landmark_map, cls, per=Cn)
    try:
        mantis.set_map(*cut)
        res, st = _check_call(mantis, lm, rigs4["frames"][0][:Cn], rigs4["ext"][:Cn], RR.shift(rigs4["Twb"][0]), loss,
                              landmarks=landmarks)
        assert res.n_cand == nc and RR.ROW_CLASSES[cls](Cn * res.n_cand)
        print(cls, loss, nc, res.status, res.iterations_run, list(res.n_obs)[:5])
    finally:
        mantis.set_map(*landmark_map)


def _pair_maps(lm, rigs4, T0):
    """Two-landmark maps of neighbours on one white line, seen by camera 0 at T0: one whose two candidates both
    give a row, one where only the first does (the host's codes on the full map: an observation does not depend
    on the other landmarks)."""
    X, nw, nr, ng = lm
    K, D = synth.intrinsics(W, H)
    f = RR.flags(X, 0.08)
    cand = RR.candidates(f)
    codes, _, _, _, tie = RR.obs(T0, rigs4["ext"][0], K, D, rigs4["frames"][0][0], X, nw, nr, ng, f)
    code_of = {i: int(c) for i, c, t in zip(cand, codes, tie) if t == 0}
    both = one = None
    for i in code_of:
        if i >= nw or code_of[i] != 0:
            continue
        axis = 0 if f[i] == 1 else 1
        step = np.zeros(3)
        step[axis] = 0.08
        for j in code_of:
            if j < nw and f[j] == f[i] and np.abs(X[j] - X[i] - step).max() <= 1e-6:
                pair = np.ascontiguousarray(np.stack([X[i], X[j]]))
                if code_of[j] == 0 and both is None:
                    both = pair
                if code_of[j] != 0 and one is None:
                    one = pair
    assert both is not None and one is not None
    return {2: both, 1: one}


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("n_rows", [0, 1, 2])
def test_starved_passes_have_defined_stats(mantis, lm, rigs4, landmark_map, loss, n_rows):
    """n_obs of 0, 1 and 2: the median of nothing is 0, of one row its key, of two the smaller key; the pass is
    STARVED and the pose untouched."""
    T0 = RR.shift(rigs4["Twb"][0])
    fr, ext = rigs4["frames"][0][:1], list(rigs4["ext"][:1])
    empty = np.zeros((0, 3))
    try:
        if n_rows == 0:
            res, st = _check_call(mantis, lm, fr, [np.eye(4)], T0, loss)  # the camera looks up: every slot code 1
        else:
            pair = _pair_maps(lm, rigs4, T0)[n_rows]
            mantis.set_map(pair, empty, empty)
            res, st = _check_call(mantis, lm, fr, ext, T0, loss, landmarks=(pair, 2, 0, 0))
            assert res.n_cand == 2
        keys, wts = mantis.refine_robust_record(0, 0)
        codes = mantis.refine_record(0, 0)[1]
    finally:
        mantis.set_map(*landmark_map)
    assert (res.status, res.refined, res.iterations_run, res.n_obs[0]) == (1, 0, 0, n_rows)
    assert np.array_equal(np.array(res.T_w_b).reshape(4, 4), T0) and not np.array(res.covariance).any()
    if n_rows == 0:
        assert (st.median_key[0], st.scale[0], st.sum_w[0], st.n_down[0], st.n_zero[0]) == (0, 0.25, 0.0, 0, 0)
        assert not keys.any() and not wts.any()
    else:
        live = sorted(int(k) for k, c in zip(keys, codes) if c == 0)
        assert len(live) == n_rows and st.median_key[0] == live[0]
        assert st.scale[0] == max(1.4826 * (live[0] / RB.KEY_UNIT), 0.25) and 0 < st.sum_w[0] <= n_rows
    with pytest.raises(Exception):
        mantis.refine_robust_record(0, 1)  # the pass did not run


@pytest.mark.parametrize("loss", LOSSES)
def test_small_pitched_frame(mantis, lm, loss):
    """322 x 242 with step_bytes = 1000: staged through the pitch conversion, the same bytes as the packed frame."""
    import mantis_amd as M

    w, h = 322, 242
    sc = RR.rig_scene(2, 1, seed=7, w=w, h=h)
    T0 = RR.shift(sc["Twb"][0])
    res, st = _check_call(mantis, lm, sc["frames"][0], sc["ext"], T0, loss)
    K, D = synth.intrinsics(w, h)
    imgs, keep = [], []
    for fr, e in zip(sc["frames"][0], sc["ext"]):
        buf = np.full((h, 3 * w + 34), 0xAB, np.uint8)  # rows 1000 bytes apart
        buf[:, : 3 * w] = fr.reshape(h, 3 * w)
        keep.append(buf)
        im = M.make_image(fr, K, D, T_base_cam=e)
        im.bgr = buf.ctypes.data
        im.step_bytes = buf.strides[0]
        imgs.append(im)
    assert imgs[0].step_bytes == 1000 > 3 * w
    pitched = mantis.refine_batch(imgs, 1, T0)[0]
    assert bytes(pitched) == bytes(res) and bytes(mantis.refine_robust_stats(0)) == bytes(st)
    with pytest.raises(Exception):
        mantis.refine_robust_record(0, 0)  # that call kept no record


@pytest.mark.parametrize("loss", LOSSES)
def test_batch_equals_single_calls(mantis, rigs4, loss):
    imgs, T0s = [], []
    for r in range(3):
        imgs += _images(rigs4["frames"][r], rigs4["ext"])
        T0s.append(RR.shift(rigs4["Twb"][r]))
    mantis.set_refine_robust(loss)
    batch = mantis.refine_batch(imgs, 3, np.array(T0s), record=1)
    stats = [mantis.refine_robust_stats(r) for r in range(3)]
    recs = [mantis.refine_record(r, 1) + mantis.refine_robust_record(r, 1) for r in range(3)]
    assert len({tuple(s.median_key) for s in stats}) == 3, "every rig has its own median"
    for r in range(3):
        one = mantis.refine_batch(imgs[4 * r: 4 * r + 4], 1, T0s[r], record=1)[0]
        assert bytes(one) == bytes(batch[r]), f"rig {r}"
        assert bytes(mantis.refine_robust_stats(0)) == bytes(stats[r]), f"rig {r}"
        for a, b in zip(mantis.refine_record(0, 1) + mantis.refine_robust_record(0, 1), recs[r]):
            assert a.tobytes() == b.tobytes()
        assert one.refined == 1


@pytest.fixture(scope="module")
def mcl_scene():
    """test_gpu_mcl's scene: one base pose seen by cameras 0, 3 and 5 of an 8-camera ring."""
    from test_gpu_mcl import CAMS

    rng = np.random.default_rng(2025)
    ext = synth.rig_extrinsics(8)
    T = synth.random_base_pose(rng)
    frames = {}
    for c in CAMS:
        Twc = T @ ext[c]
        frames[c] = synth.render_host(synth.make_cam(Twc[:3, :3], Twc[:3, 3], W, H), synth.frame_seed(13, c))
    return {"ext": ext, "Twb": T, "frames": frames, "cleaned": {}}


@pytest.mark.parametrize("loss", LOSSES)
def test_modes_equal_the_batch_call(mantis, mcl_scene, loss):
    """mantis_mcl_refine_modes (N = 256, apply = 0) against mantis_refine_batch on the modes' poses."""
    from test_gpu_mcl import _images as mcl_images
    from test_gpu_mcl_modes import _stepped

    _stepped(mantis, mcl_scene, 256)
    imgs = mcl_images(mcl_scene, (0, 3))
    mantis.set_refine_robust(loss)
    out = mantis.mcl_refine_modes(imgs, 8, record=1)
    Kn = out.n_modes
    assert Kn == 4 and out.n_moved == 0
    res = [out.mode[k].refine for k in range(Kn)]
    stats = [mantis.refine_robust_stats(k) for k in range(Kn)]
    recs = [mantis.refine_record(k, 0) + mantis.refine_robust_record(k, 0) for k in range(Kn)]
    T = np.array([np.array(out.modes.mode[k].T_w_b).reshape(4, 4) for k in range(Kn)])
    batch = mantis.refine_batch(imgs * Kn, Kn, T, record=1)
    for k in range(Kn):
        assert bytes(res[k]) == bytes(batch[k]), k
        assert bytes(mantis.refine_robust_stats(k)) == bytes(stats[k]), k
        for a, b in zip(mantis.refine_record(k, 0) + mantis.refine_robust_record(k, 0), recs[k]):
            assert a.tobytes() == b.tobytes()
    assert any(x.refined for x in res) and all(s.loss == RB.LOSSES[loss] for s in stats)


def test_switch_off_returns_the_plain_bytes(mantis, rigs4, landmark_map):
    import mantis_amd as M

    imgs, T0s = [], []
    for r in range(3):
        imgs += _images(rigs4["frames"][r], rigs4["ext"])
        T0s.append(RR.shift(rigs4["Twb"][r]))
    T0s = np.array(T0s)
    fresh = M.Mantis(max_cams=12, max_width=W, max_height=H)
    try:
        fresh.set_map(*landmark_map)
        want = fresh.refine_batch(imgs, 3, T0s, record=1)
        want_rec = fresh.refine_record(1, 2)
        with pytest.raises(Exception):
            fresh.refine_robust_stats(0)  # the switch was never on
    finally:
        fresh.close()
    mantis.set_refine_robust("tukey")
    on = mantis.refine_batch(imgs, 3, T0s, record=1)
    assert any(bytes(a) != bytes(b) for a, b in zip(on, want))
    # while the switch is on the plain record keeps the unweighted rows: pass 0 observes at the same pose
    on_rows = mantis.refine_record(1, 0)[4]
    for off in (lambda: mantis.set_refine_robust(0), lambda: mantis.set_refine_robust(None)):
        mantis.set_refine_robust("huber")
        mantis.refine_batch(imgs[:4], 1, T0s[0])
        off()
        got = mantis.refine_batch(imgs, 3, T0s, record=1)
        for a, b in zip(got, want):
            assert bytes(a) == bytes(b)
        for a, b in zip(mantis.refine_record(1, 2), want_rec):
            assert a.tobytes() == b.tobytes()
        with pytest.raises(Exception):
            mantis.refine_robust_stats(0)  # the last call ran with the switch off
        with pytest.raises(Exception):
            mantis.refine_robust_record(0, 0)
    assert np.array_equal(on_rows, mantis.refine_record(1, 0)[4]), "pass 0: the same unweighted rows on and off"


def test_one_drifted_camera_on_the_device(mantis, rigs4):
    """Camera 3 rendered from a base pose 1.2 cm / 0.4 degrees away: each robust form ends at no more than half
    the plain refinement's distance from the truth, on every rig."""
    bad = RB.contaminated_rigs4()
    for r in range(3):
        T = rigs4["Twb"][r]
        T0 = RR.shift(T)
        imgs = _images(bad[r], rigs4["ext"])
        mantis.set_refine_robust(None)
        plain = mantis.refine_batch(imgs, 1, T0)[0]
        d_plain, a_plain = RR.pose_dist(np.array(plain.T_w_b).reshape(4, 4), T)
        assert plain.refined == 1
        for loss in LOSSES:
            mantis.set_refine_robust(loss)
            res = mantis.refine_batch(imgs, 1, T0)[0]
            st = mantis.refine_robust_stats(0)
            d, a = RR.pose_dist(np.array(res.T_w_b).reshape(4, 4), T)
            print(f"rig {r} {loss}: plain {100 * d_plain:.3f} cm / {a_plain:.3f} deg -> {100 * d:.3f} cm / {a:.3f} deg, "
                  f"down {st.n_down[4]} zero {st.n_zero[4]} of {res.n_obs[4]}")
            assert res.status == 0 and res.refined == 1
            assert d <= 0.5 * d_plain, (r, loss, d, d_plain)


def test_argument_and_state_errors(mantis, rigs4):
    import mantis_amd as M

    L = M.lib()
    imgs = _images(rigs4["frames"][0], rigs4["ext"])
    T0 = RR.shift(rigs4["Twb"][0])
    mantis.set_refine_robust("huber", tuning=2.5)
    mantis.rng_state = 4242
    kept = mantis.refine_batch(imgs, 1, T0)[0]
    bad = [({"struct_size": 8}, "struct_size"), ({"loss": 3}, "loss"), ({"loss": -1}, "loss"),
           ({"tuning": 0.0}, "tuning"), ({"tuning": -1.0}, "tuning"), ({"tuning": float("nan")}, "tuning"),
           ({"tuning": float("inf")}, "tuning"), ({"scale_floor": 0.0}, "scale_floor"),
           ({"scale_floor": -0.25}, "scale_floor"), ({"scale_floor": float("nan")}, "scale_floor")]
    for kw, word in bad:
        p = RB.robust_params("tukey")
        for k, v in kw.items():
            setattr(p, k, v)
        assert L.mantis_refine_set_robust(mantis.h, C.byref(p)) == ERR_ARG, kw
        assert word in L.mantis_last_error(mantis.h).decode(), kw
    # a rejected setting leaves the earlier one: the same bytes again
    assert bytes(mantis.refine_batch(imgs, 1, T0)[0]) == bytes(kept)
    assert mantis.refine_robust_stats(0).loss == 1
    st = M.MantisRefineRobustStats()
    assert L.mantis_get_refine_robust(mantis.h, 0, None) == ERR_ARG
    assert L.mantis_get_refine_robust(mantis.h, 1, C.byref(st)) == ERR_ARG
    assert L.mantis_get_refine_robust(mantis.h, -1, C.byref(st)) == ERR_ARG
    assert L.mantis_get_refine_robust_record(mantis.h, 0, 0, None, None) == ERR_STATE  # no record was kept
    res = mantis.refine_batch(imgs, 1, T0, record=1, iterations=2)[0]
    assert L.mantis_get_refine_robust_record(mantis.h, 0, 0, None, None) == OK
    assert L.mantis_get_refine_robust_record(mantis.h, 1, 0, None, None) == ERR_ARG
    assert L.mantis_get_refine_robust_record(mantis.h, 0, 3, None, None) == ERR_ARG
    assert L.mantis_get_refine_robust_record(mantis.h, 0, -1, None, None) == ERR_ARG
    assert res.iterations_run == 2 and mantis.rng_state == 4242, "the refinement draws nothing"
    # the launches of a call are still 2 (I + 1)
    mantis.set_profiling(1)
    mantis.refine_batch(imgs, 1, T0, iterations=2)
    names = [n for n, _ in mantis.kernel_times()]
    mantis.set_profiling(0)
    assert sum(n.startswith("refine_obs") for n in names) == 3
    assert sum(n == "refine_step/k_refine_step_robust" for n in names) == 3 and len(names) == 6, names


def test_process_undisturbed_after_a_robust_refine(mantis, rigs4, landmark_map):
    """A mantis_process call after a robust refine call still matches the oracle."""
    import _oracle as O
    from test_gpu_parity import _cmp_debug

    import mantis_amd as M

    K, D = synth.intrinsics(W, H)
    mantis.set_refine_robust("tukey")
    mantis.refine_batch(_images(rigs4["frames"][0], rigs4["ext"]), 1, RR.shift(rigs4["Twb"][0]))
    img = rigs4["frames"][1][0]
    mantis.rng_state = 1
    mantis.prior_pose = None
    _, cams = mantis.process([M.make_image(img, K, D)])
    orc = O.Oracle(*landmark_map, seed=1)
    o = orc.process(img, K, D)
    _cmp_debug(mantis.frame_debug(0), o, "after a robust refine")
    assert cams[0].reason == o.reason and cams[0].publish == o.publish
    assert mantis.rng_state == orc.rng_state
