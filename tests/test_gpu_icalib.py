"""Intrinsic calibration on the GPU (mantis_calibrate_intrinsics): every
recorded pass against the host build of the same rules (mk_icalib.h through
hc_icalib_obs, fed the device's own recorded poses and intrinsics so that a
flipped tie cannot cascade), the MFMA accumulators against numpy sums of the
recorded rows, each step against hc_icalib_end_pass on the device's own
accumulators, the whole call against hc_icalib_seq, the shapes that break
loops, equal bytes, the accuracy conditions of the CPU suite, what the call
must leave untouched and the argument errors. Scenes of tests/_icalib_ref.py
and tests/_refine_ref.py; at most five views.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _icalib_ref as IR
import _refine_ref as RR
import _refine_robust_ref as RB
from mantis_amd import synth

pytestmark = pytest.mark.gpu

# the whole call against the host's: the per-pass bound is about 1e-9 at cond 1e7 and the iteration contracts
# near the solution, so it cannot grow; 1e-6 is three orders above that bound and three below the accuracy claimed
POSE_TOL = 1e-6
GAP_TOL = 1e-4
W, H = RR.W, RR.H_
ALL = 0b1111


@pytest.fixture(scope="module")
def mantis(landmark_map):
    import mantis_amd as M

    m = M.Mantis(max_cams=12, max_width=W, max_height=H)
    m.set_map(*landmark_map)
    yield m
    m.close()


@pytest.fixture(scope="module")
def lm(landmark_map):
    return RR.all_landmarks(landmark_map)


@pytest.fixture(scope="module")
def scene():
    return IR.gap_scene()


@pytest.fixture(scope="module")
def ring8():
    return RR.rig_scene(8, 1)


@pytest.fixture(scope="module")
def pairs5():
    """Five views of a two-camera rig on 640 x 360 frames."""
    return RR.rig_scene(2, 5, seed=11, w=640, h=360)


def _images(frames, exts, K=None, D=None, Ks=None, Ds=None):
    """frames[r][c] -> view-major mantis_images, every view with the rig's extrinsics and nominal intrinsics
    (K, D for every camera, or Ks, Ds per camera; default: the bench lens)."""
    import mantis_amd as M

    h, w = frames[0][0].shape[:2]
    if K is not None:
        Ks, Ds = [K] * len(exts), [D] * len(exts)
    Ks, Ds = RR.lenses(len(exts), w, h, Ks, Ds)
    return [M.make_image(f, Ks[c], Ds[c], T_base_cam=exts[c]) for fr in frames for c, f in enumerate(fr)]


def _check_call(m, lm, frames, exts, T0s, free, mask=0xFF, landmarks=None, min_obs_cam=None, Ks=None, Ds=None,
                whole_call=True, slot_guard=None, cap=0.005, gap_span=(2.2, 1.3), **params):
    """One call with record = 1: every pass against the host rules; returns (T_out, result). Ks, Ds: per-camera
    lenses (default: the bench lens); whole_call = False leaves out the comparison with hc_icalib_seq;
    slot_guard(T, E, kd, img, f, free_cam, mask, p) replaces IR.obs and returns its five arrays with the slots
    it leaves out added to the tie flag (1 = a tie, which also drops the whole-call comparison as ever; 2 =
    left out of the row comparison only); cap is the share of flagged slots allowed (tests/_line_cases.py)."""
    X, nw, nr, ng = landmarks or lm
    N, Cn = len(frames), len(exts)
    h, w = frames[0][0].shape[:2]
    Ks, Ds = RR.lenses(Cn, w, h, Ks, Ds)
    kd0 = np.array([IR.kd_of(K, D) for K, D in zip(Ks, Ds)])
    T_out, res = m.calibrate_intrinsics(_images(frames, exts, Ks=Ks, Ds=Ds), N, np.array(T0s), free, param_mask=mask,
                                        min_obs_cam=min_obs_cam, record=1, **params)
    p = m.refine_params(**params)
    ip = IR.icalib_params(free, mask, min_obs_cam)
    f = RR.flags(X, p.landmark_pitch)
    nc = len(RR.candidates(f))
    assert (res.n_cand, res.n_rigs, res.n_cams, res.free_cams, res.param_mask) == (nc, N, Cn, free, mask)
    flagged = ties = total = 0
    Ts, KDs, accs, cnts = [], [], [], []
    for k in range(res.iterations_run + 1):
        Tk, acck, cntk = [], np.zeros((N, Cn, IR.ACC)), np.zeros((N, Cn), np.int32)
        for r in range(N):
            T, KD, codes, Sw, Skw, rows, acc = m.icalib_record(r, k)
            Tk.append(T)
            if r == 0:
                KDs.append(KD)
            assert np.array_equal(KD, KDs[k]), "one set of intrinsics per pass"
            assert codes.shape == (Cn * nc,)
            for c in range(Cn):
                if slot_guard is None:
                    hc_, hSw, hSkw, hrows, tie = IR.obs(T, exts[c], KD[c], frames[r][c], X, nw, nr, ng, f,
                                                        free >> c & 1, mask, R=p.half_window,
                                                        white_thresh=p.white_thresh, min_weight=p.min_weight)
                else:
                    hc_, hSw, hSkw, hrows, tie = slot_guard(T, exts[c], KD[c], frames[r][c], f, free >> c & 1, mask, p)
                sl = slice(c * nc, (c + 1) * nc)
                ok = tie == 0
                flagged += int((~ok).sum())
                ties += int((tie == 1).sum())
                total += nc
                where = f"pass {k} view {r} camera {c}"
                assert np.array_equal(codes[sl][ok], hc_[ok]), where
                assert np.array_equal(Sw[sl][ok], hSw[ok]) and np.array_equal(Skw[sl][ok], hSkw[ok]), where
                np.testing.assert_allclose(rows[sl][ok], hrows[ok], rtol=1e-12, atol=0, err_msg=where)
                if not free >> c & 1:
                    assert not rows[sl][:, 6:14].any(), where
                for e in range(8):
                    if not mask >> e & 1:
                        assert not rows[sl][:, 6 + e].any(), where
                # both are float64 sums of the same n products, each within n 2^-53 sum |terms| of the exact
                # value (IR.np_acc120's bound): twice that beside the 1e-12 of the value, or an entry whose
                # terms cancel could not be compared at all
                ref, err = IR.np_acc120(rows[sl])
                assert np.all(np.abs(acc[c] - ref) <= 1e-12 * np.abs(ref) + 2 * err), where
                cntk[r, c] = int((codes[sl] == 0).sum())
            assert np.all(rows[codes != 0] == 0.0)
            acck[r] = acc
        Ts.append(np.array(Tk))
        accs.append(acck)
        cnts.append(cntk)
        n_obs = int(cntk.sum())
        assert res.n_obs[k] == n_obs and list(res.n_obs_cam[k])[:Cn] == list(cntk.sum(axis=0))
        rr = sum(acck.reshape(-1, IR.ACC)[:, IR.ACC - 1].tolist())  # (view, camera) order
        assert res.rms[k] == (math.sqrt(rr / n_obs) if n_obs else 0.0)
    assert flagged <= cap * total, (flagged, total)
    assert np.array_equal(Ts[0], np.array(T0s)) and np.array_equal(KDs[0], kd0), "pass 0 observes the inputs"
    fl = IR.free_list(free, Cn)
    for k in range(res.iterations_run):
        R = IR.new_result(KDs[k], free, mask, N)
        fin, Tn, delta = IR.end_pass(accs[k], cnts[k], free, mask, k, p.iterations, p, ip, Ts[k], R)
        assert not fin
        Hm, g = IR.np_normal(accs[k], free, mask, p.lambda_)
        eps = np.array([list(R.delta_cam[k][c]) for c in fl]).reshape(-1)
        bound = 1e3 * 2.0 ** -53 * np.linalg.cond(Hm) * np.linalg.norm(np.concatenate([delta.reshape(-1), eps]))
        bound += 1e-15  # the update matrix's own sin / cos
        np.testing.assert_allclose(Ts[k + 1], Tn, rtol=0, atol=bound, err_msg=f"step {k}: poses")
        deps = np.array(res.delta_cam[k]) - np.array(R.delta_cam[k])
        assert np.linalg.norm(deps) <= bound, f"step {k}: eps"
        hk = IR.kds_of(R)
        scale = np.array([hk[:, 0], hk[:, 1], hk[:, 0], hk[:, 1]] + [np.ones(Cn)] * 4).T  # eps is relative in K
        assert np.all(np.abs(KDs[k + 1] - hk) <= bound * scale * (1 + 1e-12) + 1e-13), f"step {k}: intrinsics"
    assert np.array_equal(T_out, Ts[-1]) and np.array_equal(IR.kds_of(res), KDs[-1])
    for c in range(Cn):
        held = [e for e in range(8) if not (free >> c & 1 and mask >> e & 1)]
        assert IR.kds_of(res)[c][held].tobytes() == kd0[c][held].tobytes()
    if ties and whole_call:
        print(f"whole call not compared: {ties} slots within 1e-9 of a rounding tie")
    if ties == 0 and whole_call:
        hT, host = IR.seq(T0s, exts, Ks, Ds, frames, (X, nw, nr, ng), p, ip)
        assert (res.iterations_run, res.status) == (host.iterations_run, host.status)
        assert list(res.n_obs) == list(host.n_obs)
        assert np.array_equal(np.array(res.n_obs_cam), np.array(host.n_obs_cam))
        if res.status == 0:
            np.testing.assert_allclose(T_out, hT, rtol=0, atol=POSE_TOL)
            for c in range(Cn):
                assert IR.model_gap(IR.kds_of(res)[c], IR.kds_of(host)[c], w, h, gap_span) < GAP_TOL
            assert res.calibrated == host.calibrated
    return T_out, res


@pytest.mark.parametrize("shape", ["free=0b1111", "free=0b1000", "free=0b0111", "mask=0x3F", "mask=0x0F", "mask=0xF0",
                                   "I=0", "I=10", "R=1", "R=15"])
def test_record_parity(mantis, lm, scene, shape):
    free = {"free=0b1000": 0b1000, "free=0b0111": 0b0111}.get(shape, ALL)
    mask = {"mask=0x3F": 0x3F, "mask=0x0F": 0x0F, "mask=0xF0": 0xF0}.get(shape, 0xFF)
    params = {"I=0": {"iterations": 0}, "I=10": {"iterations": 10}, "R=1": {"half_window": 1},
              "R=15": {"half_window": 15}}.get(shape, {})
    N = 2 if shape.startswith("mask") or shape.startswith("R=") else 3
    T_out, res = _check_call(mantis, lm, scene["frames"][:N], scene["ext"], scene["T0"][:N], free, mask, **params)
    kds = IR.kds_of(res)
    print(shape, res.status, res.calibrated, res.iterations_run, list(res.n_obs),
          [round(IR.model_gap(kds[c], scene["kd_true"][c]), 4) for c in range(4)])
    if shape == "I=0":
        assert np.array_equal(T_out, np.array(scene["T0"])) and np.array_equal(kds, scene["kd0"])
        assert res.iterations_run == 0 and res.status == 0
    elif shape == "R=1":
        assert res.status in (0, 1, 2, 3)  # a three-sample window holds few lines 2 cm away: whatever the rule says
    elif shape in ("free=0b1111", "I=10", "R=15"):
        assert res.status == 0 and res.calibrated == 1 and res.iterations_run == (10 if shape == "I=10" else 4)
    else:  # part of the gap is held: the rest absorbs what it can, whatever the rule says, and it says it on both
        assert res.status in (0, 2, 3)


def test_one_view_of_one_camera(mantis, lm, scene):
    T_out, res = _check_call(mantis, lm, [scene["frames"][0][:1]], scene["ext"][:1], scene["T0"][:1], 0b1)
    assert res.status in (0, 2, 3) and res.n_cams == 1


def test_five_views_of_two_cameras(mantis, lm, pairs5):
    T0 = [RR.shift(T) for T in pairs5["Twb"]]
    T_out, res = _check_call(mantis, lm, pairs5["frames"], pairs5["ext"], T0, 0b11)
    assert res.status == 0 and res.iterations_run == 4


def test_eight_cameras_all_free(mantis, lm, ring8):
    """The 64 x 64 reduced system."""
    T_out, res = _check_call(mantis, lm, ring8["frames"], ring8["ext"], [RR.shift(ring8["Twb"][0])], 0xFF,
                             lambda_=1e-3)
    assert res.status == 0 and res.iterations_run == 4
    if res.calibrated:
        assert all(any(res.covariance[c]) for c in range(8))


def test_odd_candidate_count(mantis, lm, scene, landmark_map):
    """A map whose candidate count is odd: the last trip of a block has one half idle."""
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
        T_out, res = _check_call(mantis, lm, [fr[1:3] for fr in scene["frames"][:2]], scene["ext"][1:3],
                                 scene["T0"][:2], 0b11, landmarks=landmarks)
        assert res.n_cand == nc and res.status == 0
    finally:
        mantis.set_map(w, r, g)


def test_small_pitched_frame(mantis, lm):
    """322 x 242 (neither a multiple of 4) with step_bytes = 1000 > 3 W: staged through the pitch conversion."""
    import mantis_amd as M

    w, h = 322, 242
    sc = RR.rig_scene(2, 2, seed=7, w=w, h=h)
    T0 = [RR.shift(T) for T in sc["Twb"]]
    T_out, res = _check_call(mantis, lm, sc["frames"], sc["ext"], T0, 0b11)
    K, D = synth.intrinsics(w, h)
    imgs, keep = [], []
    for fr in sc["frames"]:
        for f, e in zip(fr, sc["ext"]):
            buf = np.full((h, 3 * w + 34), 0xAB, np.uint8)  # rows 1000 bytes apart
            buf[:, : 3 * w] = f.reshape(h, 3 * w)
            keep.append(buf)
            im = M.make_image(f, K, D, T_base_cam=e)
            im.bgr = buf.ctypes.data
            im.step_bytes = buf.strides[0]
            imgs.append(im)
    assert imgs[0].step_bytes == 1000 > 3 * w
    T2, pitched = mantis.calibrate_intrinsics(imgs, 2, np.array(T0), 0b11)
    assert bytes(pitched) == bytes(res) and T2.tobytes() == T_out.tobytes()


def test_equal_bytes(mantis, scene):
    """Host frames against device frames, and the same call twice."""
    import mantis_amd as M

    K, D = scene["K"], scene["D"]
    fr, ext, T0 = scene["frames"], scene["ext"], np.array(scene["T0"])
    Th, host = mantis.calibrate_intrinsics(_images(fr, ext), 3, T0, ALL)
    Ta, again = mantis.calibrate_intrinsics(_images(fr, ext), 3, T0, ALL)
    assert bytes(host) == bytes(again) and Th.tobytes() == Ta.tobytes() and host.calibrated == 1
    fb = W * H * 3
    dev = mantis.device_alloc(fb * 12)
    try:
        imgs = []
        for r in range(3):
            for c in range(4):
                i = 4 * r + c
                mantis.h2d(dev + i * fb, fr[r][c])
                imgs.append(M.make_image(None, K, D, T_base_cam=ext[c], device_ptr=dev + i * fb, width=W, height=H))
        Td, devr = mantis.calibrate_intrinsics(imgs, 3, T0, ALL)
    finally:
        mantis.device_free(dev)
    assert bytes(host) == bytes(devr) and Th.tobytes() == Td.tobytes()


def test_calibrates_on_the_device(mantis, lm, scene):
    """The accuracy conditions of the CPU suite on the device's result."""
    T_out, res = mantis.calibrate_intrinsics(_images(scene["frames"], scene["ext"]), 3, np.array(scene["T0"]), ALL)
    assert res.iterations_run == 4
    IR.accuracy_checks(T_out, res, lm, scene)
    print("rms x fx per pass:", [round(v * 323.15, 3) for v in list(res.rms)[:5]])


def test_context_untouched(mantis, scene):
    """rng_state, the prior and the robust setting are neither read nor changed: a mantis_refine_batch, a
    mantis_calibrate_extrinsics and a mantis_process after an intrinsic calibration return the bytes they
    return before one, the caller's images keep their bytes, and the robust switch changes nothing in it."""
    import mantis_amd as M

    K, D = synth.intrinsics(W, H)
    sc = RB.rigs4()
    rimgs = _images([sc["frames"][0]], sc["ext"])
    T0 = RR.shift(sc["Twb"][0])
    prior = sc["Twb"][1]
    cimgs = _images(scene["frames"], scene["ext"])

    def before_after():
        mantis.rng_state = 1
        mantis.prior_pose = None
        rig, cams = mantis.process_motion([M.make_image(sc["frames"][1][0], K, D)])  # mantis_process
        ref = mantis.refine_batch(rimgs, 1, T0)[0]
        Te, ext = mantis.calibrate_extrinsics(cimgs[:8], 2, np.array(scene["T0"][:2]), 0b1110)
        return bytes(rig), bytes(cams[0]), bytes(ref), Te.tobytes(), bytes(ext), mantis.rng_state

    a = before_after()
    mantis.rng_state = 4242
    mantis.prior_pose = prior
    snap = [bytes(i) for i in cimgs]
    Tc, res = mantis.calibrate_intrinsics(cimgs, 3, np.array(scene["T0"]), ALL)
    assert mantis.rng_state == 4242 and np.array_equal(mantis.prior_pose, prior)
    assert [bytes(i) for i in cimgs] == snap
    mantis.set_refine_robust("tukey")
    try:
        Tr, rob = mantis.calibrate_intrinsics(cimgs, 3, np.array(scene["T0"]), ALL)
    finally:
        mantis.set_refine_robust(None)
    assert bytes(rob) == bytes(res) and Tr.tobytes() == Tc.tobytes()
    assert mantis.rng_state == 4242 and np.array_equal(mantis.prior_pose, prior)
    assert before_after() == a
    mantis.prior_pose = None


def test_starved_and_records(mantis, lm, scene):
    """A blacked-out free camera starves pass 0: the inputs come back, later passes have no record."""
    black = np.zeros_like(scene["frames"][0][0])
    frames = [[black if c == 2 else fr[c] for c in range(4)] for fr in scene["frames"][:2]]
    T_out, res = _check_call(mantis, lm, frames, scene["ext"], scene["T0"][:2], ALL)
    assert (res.status, res.calibrated, res.iterations_run) == (1, 0, 0) and res.n_obs_cam[0][2] == 0
    assert np.array_equal(T_out, np.array(scene["T0"][:2])) and not np.array(res.covariance).any()
    assert np.array_equal(IR.kds_of(res), scene["kd0"])
    with pytest.raises(Exception):
        mantis.icalib_record(0, 1)  # the pass did not run
    with pytest.raises(Exception):
        mantis.icalib_record(2, 0)  # no such view
    mantis.calibrate_intrinsics(_images(frames, scene["ext"]), 2, np.array(scene["T0"][:2]), ALL)
    with pytest.raises(Exception):
        mantis.icalib_record(0, 0)  # that call kept no record


def test_argument_errors(mantis, scene, ring8):
    import mantis_amd as M

    L = M.lib()
    ring = _images(ring8["frames"], ring8["ext"])
    quad = _images(scene["frames"], scene["ext"])
    T0 = np.array([RR.shift(ring8["Twb"][0])] * 6)
    mantis.set_profiling(1)
    mantis.rng_state = 77

    def call(images, views, T=T0, free=0b1, ip_kw=None, null=None, **kw):
        n = len(images)
        arr = (M.MantisImage * n)(*images)
        p = mantis.refine_params()
        for k, v in kw.items():
            setattr(p, k, v)
        ip = mantis.icalib_params(free)
        for k, v in (ip_kw or {}).items():
            setattr(ip, k, v)
        out = M.MantisIcalibResult()
        T_out = np.zeros((max(views, 1), 16))
        args = {"cams": arr, "T": T.ctypes.data, "p": C.byref(p), "ip": C.byref(ip), "T_out": T_out.ctypes.data,
                "out": C.byref(out)}
        if null:
            args[null] = None
        st = L.mantis_calibrate_intrinsics(mantis.h, args["cams"], views, n // max(views, 1), args["T"], args["p"],
                                           args["ip"], args["T_out"], args["out"])
        return st, L.mantis_last_error(mantis.h).decode()

    def edited(images, i, fn):
        out = _images(scene["frames"][:2], scene["ext"]) if images is None else list(images)
        fn(out[i])
        return out

    small = M.make_image(np.zeros((360, 640, 3), np.uint8), *synth.intrinsics(640, 360))
    bad_T = T0.copy()
    bad_T[0, 0, 3] = float("nan")

    def setk(i, v):
        return lambda im: im.K.__setitem__(i, v)

    def setd(i, v):
        return lambda im: im.D.__setitem__(i, v)

    def sete(i, dv):
        return lambda im: im.T_base_cam.__setitem__(i, im.T_base_cam[i] + dv)

    fresh = lambda: _images(scene["frames"][:1], scene["ext"])
    bad = [
        (ring + ring[:5], 1, {}, "cams_per_rig"),                      # 13 cameras in one rig
        (ring + ring[:7], 3, {}, "max_cams"),                          # 3 x 5 = 15 frames on max_cams = 12
        ([ring[0], small], 1, {}, "size"),
        (ring[:2], 0, {}, "n_rigs"),
        (ring[:2], 1, {"free": 0}, "free_cams"),
        (ring[:2], 1, {"free": 0b110}, "free_cams"),                   # a bit above cams_per_rig
        (ring[:2], 1, {"free": -2}, "free_cams"),
        (ring[:1], 1, {"free": 0b10}, "free_cams"),
        (ring[:2], 1, {"ip_kw": {"param_mask": 0}}, "param_mask"),
        (ring[:2], 1, {"ip_kw": {"param_mask": 0x100}}, "param_mask"),
        (ring[:2], 1, {"ip_kw": {"param_mask": -1}}, "param_mask"),
        (ring[:2], 1, {"ip_kw": {"min_obs_cam": 7}}, "min_obs_cam"),
        (ring[:2], 1, {"ip_kw": {"struct_size": 8}}, "icalib_params.struct_size"),
        (ring[:2], 1, {"struct_size": 8}, "struct_size"),
        (ring[:2], 1, {"iterations": -1}, "iterations"),
        (ring[:2], 1, {"iterations": 11}, "iterations"),
        (ring[:2], 1, {"half_window": 0}, "half_window"),
        (ring[:2], 1, {"half_window": 16}, "half_window"),
        (ring[:2], 1, {"white_thresh": 0}, "white_thresh"),
        (ring[:2], 1, {"white_thresh": 195076}, "white_thresh"),
        (ring[:2], 1, {"min_weight": 0}, "min_weight"),
        (ring[:2], 1, {"min_obs": 5}, "min_obs"),
        (ring[:2], 1, {"lambda_": -1e-9}, "lambda"),
        (ring[:2], 1, {"lambda_": float("nan")}, "lambda"),
        (ring[:2], 1, {"landmark_pitch": 0.0}, "landmark_pitch"),
        (ring[:2], 1, {"landmark_pitch": float("inf")}, "landmark_pitch"),
        (ring[:2], 1, {"max_rms": float("nan")}, "max_rms"),
        (ring[:2], 1, {"record": 2}, "record"),
        (ring[:2], 1, {"T": bad_T}, "T_w_b_in"),
        (edited(None, 5, sete(3, 1e-12)), 2, {}, "T_base_cam of a view"),  # view 1's camera 1: one byte or so
        (edited(None, 6, setk(2, 642.0)), 2, {}, "K of a view"),
        (edited(None, 7, setd(3, 0.0)), 2, {}, "D of a view"),
        (edited(fresh(), 2, sete(7, float("inf"))), 1, {}, "T_base_cam is not finite"),
        (edited(fresh(), 1, setk(5, float("nan"))), 1, {}, "K is not finite"),
        (edited(fresh(), 3, setd(1, float("inf"))), 1, {}, "D is not finite"),
        (edited(fresh(), 0, setk(0, 0.0)), 1, {}, "fx and fy"),
        (edited(fresh(), 0, setk(4, -300.0)), 1, {}, "fx and fy"),
    ] + [(ring[:2], 1, {"null": k}, "null") for k in ("cams", "T", "p", "ip", "T_out", "out")]
    for images, views, kw, word in bad:
        st, msg = call(images, views, **kw)
        assert st == 1 and word in msg, (kw, st, msg)  # MANTIS_ERR_ARG
    assert mantis.rng_state == 77
    # 257 views: turned away by its own limit before the frames are counted against max_cams
    st, msg = call(ring[:2] * 257, 257, T=np.tile(T0[:1], (257, 1, 1)))
    assert st == 1 and "n_rigs exceeds 256" in msg, msg
    # no map: a fresh context
    m2 = M.Mantis(max_cams=2, max_width=W, max_height=H)
    try:
        arr = (M.MantisImage * 2)(*ring[:2])
        p, ip = m2.refine_params(), m2.icalib_params(0b11)
        out, T_out = M.MantisIcalibResult(), np.zeros(16)
        st = L.mantis_calibrate_intrinsics(m2.h, arr, 1, 2, T0.ctypes.data, C.byref(p), C.byref(ip),
                                           T_out.ctypes.data, C.byref(out))
        assert st == 1 and "map" in L.mantis_last_error(m2.h).decode()
    finally:
        m2.close()
    with pytest.raises(Exception):
        mantis.icalib_record(0, 0)  # MANTIS_ERR_STATE: nothing recorded on this context since set_profiling
    # nothing was launched by the rejected calls: the next call's stage marks are exactly its own
    # 3 (I + 1) launches, and no image stage. One camera with every camera free is legal.
    mantis.calibrate_intrinsics(quad[:1], 1, T0[0], 0b1, iterations=2)
    names = [n for n, _ in mantis.kernel_times()]
    mantis.set_profiling(0)
    for stage in ("icalib_obs", "icalib_rig", "icalib_solve"):
        assert sum(n.startswith(stage) for n in names) == 3, names
    assert len(names) == 9, names
