"""Rig calibration on the GPU (mantis_calibrate_rig): every recorded pass
against the host build of the same rules (mk_linecal.h through hc_rcalib_obs,
fed the device's own recorded poses, extrinsics and intrinsics so that a
flipped tie cannot cascade), the three MFMA tiles' accumulators against numpy
sums of the recorded rows, each step against hc_rcalib_end_pass on the device's
own accumulators, the whole call against hc_rcalib_seq, the shapes that break
loops, equal bytes, the accuracy conditions of the CPU suite, what the call
must leave untouched and the argument errors. Scenes of tests/_rcalib_ref.py;
at most three views.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _icalib_ref as IR
import _rcalib_ref as QR
import _refine_ref as RR
import _refine_robust_ref as RB
from mantis_amd import synth

pytestmark = pytest.mark.gpu

# The whole call against the host's: the intrinsic calibration's figures, set for cond_2(S) up to 3.6e6 (the
# scene's is 3.3e6). A shape whose reduced system is worse conditioned than that (five and eight cameras, the
# 322 x 242 frames: 6e6 to 1.4e7) is held to the per-step bound alone, which scales with its own cond.
POSE_TOL = 1e-6
GAP_TOL = 1e-4
COND_MAX = 3.6e6
W, H = RR.W, RR.H_
EXT, INT = 0b1110, 0b1111


@pytest.fixture(scope="module")
def mantis(landmark_map):
    import mantis_amd as M

    m = M.Mantis(max_cams=16, max_width=W, max_height=H)
    m.set_map(*landmark_map)
    yield m
    m.close()


@pytest.fixture(scope="module")
def lm(landmark_map):
    return RR.all_landmarks(landmark_map)


@pytest.fixture(scope="module")
def scene():
    return QR.joint_scene()


def _images(frames, exts, K=None, D=None, Ks=None, Ds=None):
    """frames[r][c] -> view-major mantis_images, every view with the rig's extrinsics and nominal intrinsics
    (K, D for every camera, or Ks, Ds per camera; default: the bench lens)."""
    import mantis_amd as M

    h, w = frames[0][0].shape[:2]
    if K is not None:
        Ks, Ds = [K] * len(exts), [D] * len(exts)
    Ks, Ds = RR.lenses(len(exts), w, h, Ks, Ds)
    return [M.make_image(f, Ks[c], Ds[c], T_base_cam=exts[c]) for fr in frames for c, f in enumerate(fr)]


def _cond_S(Hm, N):
    n = 6 * N
    return np.linalg.cond(Hm[n:, n:] - Hm[n:, :n] @ np.linalg.solve(Hm[:n, :n], Hm[:n, n:]))


def _check_call(m, lm, frames, exts, T0s, fe, fi, mask=0xFF, landmarks=None, min_obs_cam=None, Ks=None, Ds=None,
                whole_call=True, slot_guard=None, cap=0.005, gap_span=(2.2, 1.3), **params):
    """One call with record = 1: every pass against the host rules; returns (T_out, result). Ks, Ds: per-camera
    lenses (default: the bench lens); whole_call = False leaves out the comparison with hc_rcalib_seq;
    slot_guard(T, E, kd, img, f, free_ext, free_int, mask, p) replaces QR.obs and returns its five arrays with
    the slots it leaves out added to the tie flag (1 = a tie, which also drops the whole-call comparison as
    ever; 2 = left out of the row comparison only); cap is the share of flagged slots allowed
    (tests/_line_cases.py)."""
    X, nw, nr, ng = landmarks or lm
    N, Cn = len(frames), len(exts)
    h, w = frames[0][0].shape[:2]
    Ks, Ds = RR.lenses(Cn, w, h, Ks, Ds)
    kd0 = np.array([IR.kd_of(K, D) for K, D in zip(Ks, Ds)])
    ext0 = np.ascontiguousarray(np.array(exts, np.float64))
    T_out, res = m.calibrate_rig(_images(frames, exts, Ks=Ks, Ds=Ds), N, np.array(T0s), fe, fi, param_mask=mask,
                                 min_obs_cam=min_obs_cam, record=1, **params)
    p = m.refine_params(**params)
    rp = QR.rcalib_params(fe, fi, mask, min_obs_cam)
    f = RR.flags(X, p.landmark_pitch)
    nc = len(RR.candidates(f))
    assert (res.n_cand, res.n_rigs, res.n_cams, res.free_ext, res.free_int, res.param_mask) == (nc, N, Cn, fe, fi, mask)
    flagged = ties = total = 0
    Ts, Es, KDs, accs, cnts = [], [], [], [], []
    for k in range(res.iterations_run + 1):
        Tk, acck, cntk = [], np.zeros((N, Cn, QR.ACC)), np.zeros((N, Cn), np.int32)
        for r in range(N):
            T, E, KD, codes, Sw, Skw, rows, acc = m.rcalib_record(r, k)
            Tk.append(T)
            if r == 0:
                Es.append(E)
                KDs.append(KD)
            assert np.array_equal(KD, KDs[k]) and np.array_equal(E, Es[k]), "one rig per pass"
            assert codes.shape == (Cn * nc,)
            for c in range(Cn):
                if slot_guard is None:
                    hc_, hSw, hSkw, hrows, tie = QR.obs(T, E[c], KD[c], frames[r][c], X, nw, nr, ng, f, fe >> c & 1,
                                                        fi >> c & 1, mask, R=p.half_window,
                                                        white_thresh=p.white_thresh, min_weight=p.min_weight)
                else:
                    hc_, hSw, hSkw, hrows, tie = slot_guard(T, E[c], KD[c], frames[r][c], f, fe >> c & 1,
                                                            fi >> c & 1, mask, p)
                sl = slice(c * nc, (c + 1) * nc)
                ok = tie == 0
                flagged += int((~ok).sum())
                ties += int((tie == 1).sum())
                total += nc
                where = f"pass {k} view {r} camera {c}"
                assert np.array_equal(codes[sl][ok], hc_[ok]), where
                assert np.array_equal(Sw[sl][ok], hSw[ok]) and np.array_equal(Skw[sl][ok], hSkw[ok]), where
                np.testing.assert_allclose(rows[sl][ok], hrows[ok], rtol=1e-12, atol=0, err_msg=where)
                if not fe >> c & 1:
                    assert not rows[sl][:, 6:12].any(), where
                if not fi >> c & 1:
                    assert not rows[sl][:, 12:20].any(), where
                for e in range(8):
                    if not mask >> e & 1:
                        assert not rows[sl][:, 12 + e].any(), where
                # both are float64 sums of the same n products, each within n 2^-53 sum |terms| of the exact
                # value (QR.np_acc231's bound): twice that beside the 1e-12 of the value, or an entry whose
                # terms cancel could not be compared at all
                ref, err = QR.np_acc231(rows[sl])
                assert np.all(np.abs(acc[c] - ref) <= 1e-12 * np.abs(ref) + 2 * err), where
                cntk[r, c] = int((codes[sl] == 0).sum())
            assert np.all(rows[codes != 0] == 0.0)
            acck[r] = acc
        Ts.append(np.array(Tk))
        accs.append(acck)
        cnts.append(cntk)
        n_obs = int(cntk.sum())
        assert res.n_obs[k] == n_obs and list(res.n_obs_cam[k])[:Cn] == list(cntk.sum(axis=0))
        rr = sum(acck.reshape(-1, QR.ACC)[:, QR.ACC - 1].tolist())  # (view, camera) order
        assert res.rms[k] == (math.sqrt(rr / n_obs) if n_obs else 0.0)
    assert flagged <= cap * total, (flagged, total)
    assert np.array_equal(Ts[0], np.array(T0s)) and np.array_equal(KDs[0], kd0) and np.array_equal(Es[0], ext0), \
        "pass 0 observes the inputs"
    cond_S = 0.0
    for k in range(res.iterations_run):
        R = QR.new_result(Es[k], KDs[k], fe, fi, mask, N)
        fin, Tn, delta = QR.end_pass(accs[k], cnts[k], fe, fi, mask, k, p.iterations, p, rp, Ts[k], R)
        assert not fin
        Hm, g = QR.np_normal(accs[k], fe, fi, mask, p.lambda_)
        cond_S = max(cond_S, _cond_S(Hm, N))
        x = np.concatenate([delta.reshape(-1), QR.steps_of(R, k, fe, fi, Cn)])
        bound = 1e3 * 2.0 ** -53 * np.linalg.cond(Hm) * np.linalg.norm(x)
        bound += 1e-15  # the update matrix's own sin / cos
        np.testing.assert_allclose(Ts[k + 1], Tn, rtol=0, atol=bound, err_msg=f"step {k}: poses")
        d = np.concatenate([(np.array(res.delta_ext[k]) - np.array(R.delta_ext[k])).reshape(-1),
                            (np.array(res.delta_int[k]) - np.array(R.delta_int[k])).reshape(-1)])
        assert np.linalg.norm(d) <= bound, f"step {k}: eps {np.linalg.norm(d)} > {bound}"
        np.testing.assert_allclose(Es[k + 1], QR.exts_of(R), rtol=0, atol=bound * 2 + 1e-14,
                                   err_msg=f"step {k}: extrinsics")  # |t| of an extrinsic is below 2
        hk = QR.kds_of(R)
        scale = np.array([hk[:, 0], hk[:, 1], hk[:, 0], hk[:, 1]] + [np.ones(Cn)] * 4).T  # eps is relative in K
        assert np.all(np.abs(KDs[k + 1] - hk) <= bound * scale * (1 + 1e-12) + 1e-13), f"step {k}: intrinsics"
    assert np.array_equal(T_out, Ts[-1]) and np.array_equal(QR.kds_of(res), KDs[-1])
    assert np.array_equal(QR.exts_of(res), Es[-1])
    for c in range(Cn):
        held = [e for e in range(8) if not (fi >> c & 1 and mask >> e & 1)]
        assert QR.kds_of(res)[c][held].tobytes() == kd0[c][held].tobytes()
        if not fe >> c & 1:
            assert QR.exts_of(res)[c].tobytes() == ext0[c].tobytes()
    if ties and whole_call:
        print(f"whole call not compared: {ties} slots within 1e-9 of a rounding tie")
    if ties == 0 and whole_call:
        hT, host = QR.seq(T0s, exts, Ks, Ds, frames, (X, nw, nr, ng), p, rp)
        assert (res.iterations_run, res.status) == (host.iterations_run, host.status)
        assert list(res.n_obs) == list(host.n_obs)
        assert np.array_equal(np.array(res.n_obs_cam), np.array(host.n_obs_cam))
        if res.status == 0:
            dT = np.abs(T_out - hT).max()
            dE = np.abs(QR.exts_of(res) - QR.exts_of(host)).max()
            gap = max(IR.model_gap(QR.kds_of(res)[c], QR.kds_of(host)[c], w, h, gap_span) for c in range(Cn))
            print(f"whole call against the host: cond(S) {cond_S:.3g} poses {dT:.3g} extrinsics {dE:.3g} gap {gap:.3g} px")
            if cond_S <= COND_MAX:
                assert dT <= POSE_TOL and dE <= POSE_TOL and gap < GAP_TOL
            assert res.calibrated == host.calibrated
    return T_out, res


MASKS = ["ext=0b1110 int=0b1111", "ext=0b1000 int=0b0001", "ext=0b0100 int=0b0100", "mask=0x0F", "mask=0xF0"]


@pytest.mark.parametrize("shape", MASKS + ["I=0", "I=10", "R=1", "R=15"])
def test_record_parity(mantis, lm, scene, shape):
    fe, fi = {"ext=0b1000 int=0b0001": (0b1000, 0b0001), "ext=0b0100 int=0b0100": (0b0100, 0b0100)}.get(shape, (EXT, INT))
    mask = {"mask=0x0F": 0x0F, "mask=0xF0": 0xF0}.get(shape, 0xFF)
    params = {"I=0": {"iterations": 0}, "I=10": {"iterations": 10}, "R=1": {"half_window": 1},
              "R=15": {"half_window": 15}}.get(shape, {})
    N = 2 if shape.startswith("R=") else 3
    T_out, res = _check_call(mantis, lm, scene["frames"][:N], scene["ext"], scene["T0"][:N], fe, fi, mask, **params)
    kds = QR.kds_of(res)
    print(shape, res.status, res.calibrated, res.iterations_run, list(res.n_obs),
          [round(IR.model_gap(kds[c], scene["kd_true"][c]), 4) for c in range(4)])
    if shape == "I=0":
        assert np.array_equal(T_out, np.array(scene["T0"])) and np.array_equal(kds, scene["kd0"])
        assert np.array_equal(QR.exts_of(res), np.array(scene["ext"]))
        assert res.iterations_run == 0 and res.status == 0
    elif shape == "R=1":
        assert res.status in (0, 1, 2, 3)  # a three-sample window holds few lines 2 cm away: whatever the rule says
    elif shape in (MASKS[0], "I=10", "R=15"):
        assert res.status == 0 and res.calibrated == 1 and res.iterations_run == (10 if shape == "I=10" else 4)
    else:  # part of the rig is held off the truth: the rest absorbs what it can, and it says so on both
        assert res.status in (0, 2, 3)


def test_smallest_call(mantis, lm):
    """Two views of two cameras on 640 x 360 with ext 0b10 / int 0b11: nS = 22."""
    sc = QR.joint_scene(2, 2, 11, 640, 360)
    T_out, res = _check_call(mantis, lm, sc["frames"], sc["ext"], sc["T0"], 0b10, 0b11)
    assert res.status == 0 and res.iterations_run == 4


def test_five_cameras(mantis, lm):
    """A wave's second camera (cameras w and w + 4), on 640 x 360."""
    sc = QR.joint_scene(5, 2, 2024, 640, 360)
    T_out, res = _check_call(mantis, lm, sc["frames"], sc["ext"], sc["T0"], 0b11110, 0b11111)
    assert res.status == 0 and res.iterations_run == 4


def test_eight_cameras(mantis, lm):
    """ext 0xFE / int 0xFF: nS = 106, every column of the three MFMA tiles of every wave's two cameras in use,
    the 106 x 107 reduced system in the solve kernel's dynamic LDS."""
    sc = QR.joint_scene(8, 2, 2024, 640, 360)
    T_out, res = _check_call(mantis, lm, sc["frames"], sc["ext"], sc["T0"], 0xFE, 0xFF, lambda_=1e-3)
    assert res.status == 0 and res.iterations_run == 4
    if res.calibrated:
        assert all(any(res.cov_int[c]) for c in range(8)) and all(any(res.cov_ext[c]) for c in range(1, 8))
        assert not any(res.cov_ext[0])


def test_odd_candidate_count(mantis, lm, scene, landmark_map):
    """A map whose candidate count is odd and no multiple of 32: the last trip of an observation block has one
    half idle, the last MFMA trips read past the end as zeros."""
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
                                 scene["T0"][:2], 0b10, 0b11, landmarks=landmarks)
        assert res.n_cand == nc and res.status == 0
    finally:
        mantis.set_map(w, r, g)


@pytest.mark.parametrize("cls", list(RR.ROW_CLASSES))
def test_trip_loop_tails(mantis, lm, scene, landmark_map, cls):
    """Two views of two cameras on a map cut until a camera's n_cand rows -- what one wave's trip loop of the
    three 21-column tiles runs over -- end that loop another way (RR.ROW_CLASSES). The small classes leave the
    call STARVED, its record written."""
    cut, landmarks, nc = RR.cut_map(landmark_map, cls)
    try:
        mantis.set_map(*cut)
        T_out, res = _check_call(mantis, lm, [fr[1:3] for fr in scene["frames"][:2]], scene["ext"][1:3],
                                 scene["T0"][:2], 0b10, 0b11, landmarks=landmarks)
        assert res.n_cand == nc and RR.ROW_CLASSES[cls](res.n_cand)
        print(cls, nc, res.status, res.iterations_run, list(res.n_obs)[:5])
    finally:
        mantis.set_map(*landmark_map)


def test_small_pitched_frame(mantis, lm):
    """322 x 242 (neither a multiple of 4) with step_bytes = 1000 > 3 W: staged through the pitch conversion."""
    import mantis_amd as M

    w, h = 322, 242
    sc = QR.joint_scene(2, 2, 7, w, h)
    T0 = sc["T0"]
    T_out, res = _check_call(mantis, lm, sc["frames"], sc["ext"], T0, 0b10, 0b11)
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
    T2, pitched = mantis.calibrate_rig(imgs, 2, np.array(T0), 0b10, 0b11)
    assert bytes(pitched) == bytes(res) and T2.tobytes() == T_out.tobytes()


def test_equal_bytes(mantis, scene):
    """Host frames against device frames, and the same call twice."""
    import mantis_amd as M

    K, D = scene["K"], scene["D"]
    fr, ext, T0 = scene["frames"], scene["ext"], np.array(scene["T0"])
    Th, host = mantis.calibrate_rig(_images(fr, ext), 3, T0, EXT, INT)
    Ta, again = mantis.calibrate_rig(_images(fr, ext), 3, T0, EXT, INT)
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
        Td, devr = mantis.calibrate_rig(imgs, 3, T0, EXT, INT)
    finally:
        mantis.device_free(dev)
    assert bytes(host) == bytes(devr) and Th.tobytes() == Td.tobytes()


def test_calibrates_on_the_device(mantis, lm, scene):
    """The accuracy conditions of the CPU suite on the device's result."""
    T_out, res = mantis.calibrate_rig(_images(scene["frames"], scene["ext"]), 3, np.array(scene["T0"]), EXT, INT)
    assert (res.status, res.calibrated, res.iterations_run) == (0, 1, 4)
    g0, e0, p0 = QR.figures(scene["T0"], scene["ext"], scene["kd0"], scene)
    g1, e1, p1 = QR.figures(T_out, QR.exts_of(res), QR.kds_of(res), scene)
    print("model gap px:", np.round(g1, 3), "extrinsics (cm, deg):", [(round(100 * a, 3), round(b, 3)) for a, b in e1],
          "poses cm:", np.round(100 * np.array(p1), 3))
    for c in range(4):
        assert g1[c] < g0[c] / 8
    for c in range(1, 4):
        assert e1[c][0] < e0[c][0] / 5 and e1[c][1] < e0[c][1] / 5
    assert QR.exts_of(res)[0].tobytes() == np.ascontiguousarray(scene["ext"][0]).tobytes()
    assert max(p1) < 0.002


def test_context_untouched(mantis, scene):
    """rng_state, the prior and the robust setting are neither read nor changed: a mantis_refine_batch, a
    mantis_calibrate_extrinsics, a mantis_calibrate_intrinsics and a mantis_process after a rig calibration
    return the bytes they return before one, the caller's images keep their bytes, and the robust switch changes
    nothing in it."""
    import mantis_amd as M

    K, D = synth.intrinsics(W, H)
    sc = RB.rigs4()
    rimgs = _images([sc["frames"][0]], sc["ext"])
    T0 = RR.shift(sc["Twb"][0])
    prior = sc["Twb"][1]
    cimgs = _images(scene["frames"], scene["ext"])
    T2 = np.array(scene["T0"][:2])

    def before_after():
        mantis.rng_state = 1
        mantis.prior_pose = None
        rig, cams = mantis.process_motion([M.make_image(sc["frames"][1][0], K, D)])  # mantis_process
        ref = mantis.refine_batch(rimgs, 1, T0)[0]
        Te, ext = mantis.calibrate_extrinsics(cimgs[:8], 2, T2, 0b1110)
        Ti, intr = mantis.calibrate_intrinsics(cimgs[:8], 2, T2, 0b1111)
        return (bytes(rig), bytes(cams[0]), bytes(ref), Te.tobytes(), bytes(ext), Ti.tobytes(), bytes(intr),
                mantis.rng_state)

    a = before_after()
    mantis.rng_state = 4242
    mantis.prior_pose = prior
    snap = [bytes(i) for i in cimgs]
    Tc, res = mantis.calibrate_rig(cimgs, 3, np.array(scene["T0"]), EXT, INT)
    assert mantis.rng_state == 4242 and np.array_equal(mantis.prior_pose, prior)
    assert [bytes(i) for i in cimgs] == snap
    mantis.set_refine_robust("tukey")
    try:
        Tr, rob = mantis.calibrate_rig(cimgs, 3, np.array(scene["T0"]), EXT, INT)
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
    T_out, res = _check_call(mantis, lm, frames, scene["ext"], scene["T0"][:2], EXT, INT)
    assert (res.status, res.calibrated, res.iterations_run) == (1, 0, 0) and res.n_obs_cam[0][2] == 0
    assert np.array_equal(T_out, np.array(scene["T0"][:2]))
    assert not np.array(res.cov_ext).any() and not np.array(res.cov_int).any()
    assert np.array_equal(QR.kds_of(res), scene["kd0"]) and np.array_equal(QR.exts_of(res), np.array(scene["ext"]))
    with pytest.raises(Exception):
        mantis.rcalib_record(0, 1)  # the pass did not run
    with pytest.raises(Exception):
        mantis.rcalib_record(2, 0)  # no such view
    mantis.calibrate_rig(_images(frames, scene["ext"]), 2, np.array(scene["T0"][:2]), EXT, INT)
    with pytest.raises(Exception):
        mantis.rcalib_record(0, 0)  # that call kept no record


def test_argument_errors(mantis, scene):
    import mantis_amd as M

    L = M.lib()
    quad = _images(scene["frames"], scene["ext"])
    ring = quad[:4] * 4  # 16 images of one size
    T0 = np.array([scene["T0"][0]] * 6)
    mantis.set_profiling(1)
    mantis.rng_state = 77

    def call(images, views, T=T0, fe=0b10, fi=0b1, rp_kw=None, null=None, **kw):
        n = len(images)
        arr = (M.MantisImage * n)(*images)
        p = mantis.refine_params()
        for k, v in kw.items():
            setattr(p, k, v)
        rp = mantis.rcalib_params(fe, fi)
        for k, v in (rp_kw or {}).items():
            setattr(rp, k, v)
        out = M.MantisRcalibResult()
        T_out = np.zeros((max(views, 1), 16))
        args = {"cams": arr, "T": T.ctypes.data, "p": C.byref(p), "rp": C.byref(rp), "T_out": T_out.ctypes.data,
                "out": C.byref(out)}
        if null:
            args[null] = None
        st = L.mantis_calibrate_rig(mantis.h, args["cams"], views, n // max(views, 1), args["T"], args["p"],
                                    args["rp"], args["T_out"], args["out"])
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
        (ring[:13], 1, {}, "cams_per_rig"),                            # 13 cameras in one rig
        (ring + ring[:5], 3, {}, "max_cams"),                          # 3 x 7 = 21 frames on max_cams = 16
        ([quad[0], small], 1, {}, "size"),
        (quad[:2], 0, {}, "n_rigs"),
        (quad[:1], 1, {"fe": 0b1}, "cams_per_rig"),                    # one camera: no gauge
        (quad[:2], 1, {"fe": 0}, "free_ext"),
        (quad[:2], 1, {"fi": 0}, "free_int"),
        (quad[:2], 1, {"fe": 0b110}, "free_ext"),                      # a bit above cams_per_rig
        (quad[:2], 1, {"fi": 0b100}, "free_int"),
        (quad[:2], 1, {"fe": -2}, "free_ext"),
        (quad[:2], 1, {"fi": -2}, "free_int"),
        (quad[:2], 1, {"fe": 0b11}, "free_ext names every camera"),
        (quad[:2], 1, {"rp_kw": {"param_mask": 0}}, "param_mask"),
        (quad[:2], 1, {"rp_kw": {"param_mask": 0x100}}, "param_mask"),
        (quad[:2], 1, {"rp_kw": {"param_mask": -1}}, "param_mask"),
        (quad[:2], 1, {"rp_kw": {"min_obs_cam": 13}}, "min_obs_cam"),
        (quad[:2], 1, {"rp_kw": {"struct_size": 16}}, "rcalib_params.struct_size"),
        (quad[:2], 1, {"struct_size": 8}, "struct_size"),
        (quad[:2], 1, {"iterations": -1}, "iterations"),
        (quad[:2], 1, {"iterations": 11}, "iterations"),
        (quad[:2], 1, {"half_window": 0}, "half_window"),
        (quad[:2], 1, {"half_window": 16}, "half_window"),
        (quad[:2], 1, {"white_thresh": 0}, "white_thresh"),
        (quad[:2], 1, {"white_thresh": 195076}, "white_thresh"),
        (quad[:2], 1, {"min_weight": 0}, "min_weight"),
        (quad[:2], 1, {"min_obs": 5}, "min_obs"),
        (quad[:2], 1, {"lambda_": -1e-9}, "lambda"),
        (quad[:2], 1, {"lambda_": float("nan")}, "lambda"),
        (quad[:2], 1, {"landmark_pitch": 0.0}, "landmark_pitch"),
        (quad[:2], 1, {"landmark_pitch": float("inf")}, "landmark_pitch"),
        (quad[:2], 1, {"max_rms": float("nan")}, "max_rms"),
        (quad[:2], 1, {"record": 2}, "record"),
        (quad[:2], 1, {"T": bad_T}, "T_w_b_in"),
        (edited(None, 5, sete(3, 1e-12)), 2, {}, "T_base_cam of a view"),  # view 1's camera 1: one byte or so
        (edited(None, 6, setk(2, 642.0)), 2, {}, "K of a view"),
        (edited(None, 7, setd(3, 0.0)), 2, {}, "D of a view"),
        (edited(fresh(), 2, sete(7, float("inf"))), 1, {}, "T_base_cam is not finite"),
        (edited(fresh(), 1, setk(5, float("nan"))), 1, {}, "K is not finite"),
        (edited(fresh(), 3, setd(1, float("inf"))), 1, {}, "D is not finite"),
        (edited(fresh(), 0, setk(0, 0.0)), 1, {}, "fx and fy"),
        (edited(fresh(), 0, setk(4, -300.0)), 1, {}, "fx and fy"),
    ] + [(quad[:2], 1, {"null": k}, "null") for k in ("cams", "T", "p", "rp", "T_out", "out")]
    for images, views, kw, word in bad:
        st, msg = call(images, views, **kw)
        assert st == 1 and word in msg, (kw, st, msg)  # MANTIS_ERR_ARG
    assert mantis.rng_state == 77
    # 257 views: turned away by its own limit before the frames are counted against max_cams
    st, msg = call(quad[:2] * 257, 257, T=np.tile(T0[:1], (257, 1, 1)))
    assert st == 1 and "n_rigs exceeds 256" in msg, msg
    # no map: a fresh context
    m2 = M.Mantis(max_cams=2, max_width=W, max_height=H)
    try:
        arr = (M.MantisImage * 2)(*quad[:2])
        p, rp = m2.refine_params(), m2.rcalib_params(0b10, 0b11)
        out, T_out = M.MantisRcalibResult(), np.zeros(16)
        st = L.mantis_calibrate_rig(m2.h, arr, 1, 2, T0.ctypes.data, C.byref(p), C.byref(rp), T_out.ctypes.data,
                                    C.byref(out))
        assert st == 1 and "map" in L.mantis_last_error(m2.h).decode()
    finally:
        m2.close()
    # nothing was launched by the rejected calls: the next call's stage marks are exactly its own
    # 3 (I + 1) launches, and no image stage
    mantis.calibrate_rig(quad[:2], 1, T0[0], 0b10, 0b11, iterations=2)
    names = [n for n, _ in mantis.kernel_times()]
    mantis.set_profiling(0)
    for stage in ("rcalib_obs", "rcalib_rig", "rcalib_solve"):
        assert sum(n.startswith(stage) for n in names) == 3, names
    assert len(names) == 9, names
    with pytest.raises(Exception):
        mantis.rcalib_record(0, 0)  # MANTIS_ERR_STATE: that call kept no record
