"""Robust rows of the three calibrations on the GPU (mantis_calib_set_robust):
every recorded pass of a call against the host build of the same rule
(mk_linecal.h through hc_linecal_robust_weights, fed the device's own recorded
sums, so that a flipped tie cannot cascade) -- keys, the call-wide median and
scale exact, weights to 1e-14, every count exact, the MFMA accumulators against
numpy sums of sqrt(w) x the recorded rows, each step against the host end of a
pass on the device's own accumulators, the whole call against hc_*_seq_robust
-- on the shapes that break loops; equal bytes; the two switches' independence;
the getters' errors; the launch counts; and the knocked scene's accuracy
conditions on the device's results. Scenes of tests/_calib_robust_ref.py.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _calib_robust_ref as QR
import _icalib_ref as IR
import _refine_ref as RR
import _refine_robust_ref as RB
from mantis_amd import synth

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-9
ERR_ARG, ERR_STATE = 1, 5  # mantis_status
STEP_TOL = 1e-12
W, H = RR.W, RR.H_
FREE = 0b1110
SPECS = {"ext": QR.Spec("ext", free_ext=FREE), "int": QR.Spec("int", free_int=0b1111),
         "rig": QR.Spec("rig", free_ext=FREE, free_int=0b1111)}


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
def knocked():
    return QR.knocked_scene()


def _kds(n, w=W, h=H):
    return np.tile(QR.float_kd(*synth.intrinsics(w, h)), (n, 1))


def _check_call(m, spec, lm, frames, exts, kds, T0s, loss, landmarks=None, **params):
    """One call with the robust rows of `loss` and record = 1: every pass against the host rule; returns
    (T_out, result, stats)."""
    lm = landmarks or lm
    N, Cn = len(frames), len(exts)
    rb = QR.robust_params(loss)
    images = spec.images(frames, exts, kds)
    m.set_calib_robust(None)
    T_plain, plain = spec.calibrate(m, images, N, T0s, record=1, **params)
    rows0 = [spec.record(m, r, 0, exts, kds)[6] for r in range(N)]
    m.set_calib_robust(loss)
    try:
        T_out, res = spec.calibrate(m, images, N, T0s, record=1, **params)
        st = m.calib_robust_stats(spec.kind)
    finally:
        m.set_calib_robust(None)
    p = m.refine_params(**params)
    I = p.iterations
    f = RR.flags(lm[0], p.landmark_pitch)
    nc = len(RR.candidates(f))
    assert (res.n_cand, res.n_rigs, res.n_cams) == (nc, N, Cn)
    assert (st.loss, st.kind, st.n_rigs, st.n_cams) == (rb.loss, spec.index, N, Cn)
    flagged = total = 0
    Ts, Es, KDs, accs, cnts, poss = [], [], [], [], [], []
    last = res.iterations_run
    for k in range(last + 1):
        rec = [spec.record(m, r, k, exts, kds) for r in range(N)]
        rob = [m.calib_robust_record(spec.kind, r, k) for r in range(N)]
        E, KD = rec[0][1], rec[0][2]
        codes = np.array([x[3] for x in rec]).reshape(N, Cn, nc)
        Sw = np.array([x[4] for x in rec]).reshape(N, Cn, nc)
        Skw = np.array([x[5] for x in rec]).reshape(N, Cn, nc)
        rows = np.array([x[6] for x in rec]).reshape(N, Cn, nc, spec.ROW)
        acc = np.array([x[7] for x in rec])
        keys = np.array([x[0] for x in rob]).reshape(N, Cn, nc)
        w = np.array([x[1] for x in rob]).reshape(N, Cn, nc)
        where = f"pass {k}"
        # the unweighted rows: the host's observation at the recorded estimates, and (pass 0) the plain record's
        for r in range(N):
            assert np.array_equal(rec[r][1], E) and np.array_equal(rec[r][2], KD), "one set of estimates per pass"
            for c in range(Cn):
                hcod, hSw, hSkw, hrows, tie = spec.obs(rec[r][0], E[c], KD[c], frames[r][c], lm, f, c, p)
                ok = tie == 0
                flagged += int((~ok).sum())
                total += nc
                assert np.array_equal(codes[r, c][ok], hcod[ok]), where
                assert np.array_equal(Sw[r, c][ok], hSw[ok]) and np.array_equal(Skw[r, c][ok], hSkw[ok]), where
                np.testing.assert_allclose(rows[r, c][ok], hrows[ok], rtol=1e-12, atol=0, err_msg=where)
            if k == 0:
                assert rec[r][6].tobytes() == rows0[r].tobytes(), "the record's rows are the plain record's"
        assert np.all(rows[codes != 0] == 0.0)
        # a, b: keys, median and scale exact, weights to 1e-14
        host = QR.call_weights(codes, Sw, Skw, rb)
        assert np.array_equal(keys, host["keys"]), where
        assert st.median_key[k] == host["median"] and st.scale[k] == host["scale"], where
        np.testing.assert_allclose(w, host["w"], rtol=1e-14, atol=0, err_msg=where)
        assert not w[codes != 0].any() and not keys[codes != 0].any()
        # c: the counts
        live = codes == 0
        cnt = live.sum(axis=2).astype(np.int32)
        assert st.n_down[k] == host["n_down"] == int((w[live] < 1).sum()), where
        assert st.n_zero[k] == host["n_zero"] == int((w[live] == 0).sum()), where
        assert res.n_obs[k] == host["n_obs"] and list(res.n_obs_cam[k])[:Cn] == list(cnt.sum(axis=0)), where
        # d: the sums. sum_w is a float64 sum of n weights in [0, 1]: within n 2^-53 sum w of the exact value
        ws = float(w.sum())
        assert abs(st.sum_w[k] - ws) <= 1e-12 * ws + 2 * w.size * 2.0 ** -53 * ws, where
        wrows = rows * np.sqrt(w)[..., None]
        for r in range(N):
            for c in range(Cn):
                ref, err = spec.np_acc(wrows[r, c])
                assert np.all(np.abs(acc[r, c] - ref) <= 1e-12 * np.abs(ref) + 2 * err), (where, r, c)
        rr = sum(acc.reshape(-1, spec.ACC)[:, -1].tolist())  # (view, camera) order
        assert res.rms[k] == (math.sqrt(rr / host["n_obs"]) if host["n_obs"] else 0.0), where
        Ts.append(np.array([x[0] for x in rec]))
        Es.append(E)
        KDs.append(KD)
        accs.append(acc)
        cnts.append(cnt)
        poss.append(cnt - host["cell_zero"])
        if k == last:  # the per-view and per-camera figures of the last pass run
            wl = np.where(live, w, 0.0)
            assert list(st.n_obs_view)[:N] == list(cnt.sum(axis=1)) and not any(list(st.n_obs_view)[N:])
            assert list(st.n_zero_view)[:N] == list(host["cell_zero"].sum(axis=1))
            assert list(st.n_zero_cam)[:Cn] == list(host["cell_zero"].sum(axis=0))
            for got, ref in ((list(st.sum_w_view)[:N], wl.sum(axis=(1, 2))),
                             (list(st.sum_w_cam)[:Cn], wl.sum(axis=(0, 2)))):
                assert np.all(np.abs(np.array(got) - ref) <= 1e-12 * ref + 2 * w.size * 2.0 ** -53 * ref), where
            assert not any(list(st.sum_w_view)[N:]) and not any(list(st.sum_w_cam)[Cn:])
    assert not any(st.median_key[last + 1:]) and not any(st.sum_w[last + 1:]) and not any(st.scale[last + 1:])
    assert flagged <= 0.005 * total, (flagged, total)
    assert np.array_equal(Ts[0], np.array(T0s)) and np.array_equal(Es[0], np.array(exts)), "pass 0 observes the inputs"
    assert np.array_equal(KDs[0], np.array(kds))
    # e: each step against the host end of a pass on the device's own accumulators
    for k in range(last):
        R = spec.new_result(Es[k], KDs[k], N)
        fin, Tn, _ = spec.end_pass(accs[k], cnts[k], poss[k], k, I, p, Ts[k], R)
        assert not fin
        En, KDn = spec.state_of(R, Es[k], KDs[k])
        np.testing.assert_allclose(Ts[k + 1], Tn, rtol=0, atol=STEP_TOL, err_msg=f"step {k}: poses")
        np.testing.assert_allclose(Es[k + 1], En, rtol=0, atol=STEP_TOL, err_msg=f"step {k}: extrinsics")
        np.testing.assert_allclose(KDs[k + 1], KDn, rtol=1e-12, atol=STEP_TOL, err_msg=f"step {k}: intrinsics")
    if last < I:  # the call stopped: the host gate stops on the same pass with the same status
        R = spec.new_result(Es[last], KDs[last], N)
        fin, _, _ = spec.end_pass(accs[last], cnts[last], poss[last], last, I, p, Ts[last], R)
        assert fin and R.status == res.status
    E_out, KD_out = spec.state_of(res, exts, kds)
    assert np.array_equal(T_out, Ts[-1]) and np.array_equal(E_out, Es[-1]) and np.array_equal(KD_out, KDs[-1])
    # f: the whole call
    if flagged == 0:
        hT, hres, hst = spec.seq(T0s, exts, kds, frames, lm, p, rb)
        hE, hKD = spec.state_of(hres, exts, kds)
        np.testing.assert_allclose(T_out, hT, rtol=0, atol=POSE_TOL)
        np.testing.assert_allclose(E_out, hE, rtol=0, atol=POSE_TOL)
        np.testing.assert_allclose(KD_out, hKD, rtol=1e-9, atol=POSE_TOL)
        assert list(res.n_obs) == list(hres.n_obs) and np.array_equal(np.array(res.n_obs_cam), np.array(hres.n_obs_cam))
        assert (res.iterations_run, res.calibrated, res.status) == (hres.iterations_run, hres.calibrated, hres.status)
        assert list(st.median_key) == list(hst.median_key) and list(st.scale) == list(hst.scale)
        assert list(st.n_down) == list(hst.n_down) and list(st.n_zero) == list(hst.n_zero)
        assert list(st.n_zero_view) == list(hst.n_zero_view) and list(st.n_zero_cam) == list(hst.n_zero_cam)
    return T_out, res, st


@pytest.mark.parametrize("loss", QR.LOSSES)
@pytest.mark.parametrize("kind", QR.KINDS)
def test_three_views_of_four_cameras(mantis, lm, knocked, kind, loss):
    T_out, res, st = _check_call(mantis, SPECS[kind], lm, knocked["frames"], knocked["ext"], knocked["kd"],
                                 knocked["T0"], loss)
    assert res.status == 0 and res.calibrated == 1 and res.iterations_run == 4
    assert st.n_down[4] > 0 and (st.n_zero[4] > 0) == (loss == "tukey")


@pytest.mark.parametrize("kind,loss", [("ext", "huber"), ("rig", "tukey")])
def test_one_view_of_two_cameras(mantis, lm, knocked, kind, loss):
    spec = QR.Spec(kind, free_ext=0b10, free_int=0b11)
    fr = [knocked["frames"][0][:2]]
    T_out, res, st = _check_call(mantis, spec, lm, fr, knocked["ext"][:2], knocked["kd"][:2], knocked["T0"][:1], loss)
    assert res.status == 0 and res.iterations_run == 4


@pytest.mark.parametrize("kind,loss", [("rig", "tukey"), ("int", "huber")])
def test_two_views_of_eight_cameras(mantis, lm, kind, loss):
    """4320 slots per view (the weights of one chunk fill the kernel's LDS) and seven free cameras."""
    sc = RR.rig_scene(8, 2)
    spec = QR.Spec(kind, free_ext=0b11111110, free_int=0b11111111)
    T0 = [RR.shift(T) for T in sc["Twb"]]
    T_out, res, st = _check_call(mantis, spec, lm, sc["frames"], [np.array(e) for e in sc["ext"]], _kds(8), T0, loss)
    assert res.n_cand * 8 == 4320 and res.status == 0 and res.iterations_run == 4


@pytest.mark.parametrize("kind,loss", [("ext", "tukey"), ("int", "huber")])
def test_five_views_of_two_cameras(mantis, lm, kind, loss):
    """Five blocks whose own medians differ: the call's median needs the sum over the blocks."""
    sc = RR.rig_scene(2, 5, seed=11, w=640, h=360)
    spec = QR.Spec(kind, free_ext=0b10, free_int=0b11)
    T0 = [RR.shift(T) if r % 2 else np.array(T) for r, T in enumerate(sc["Twb"])]  # two views start at the truth
    T_out, res, st = _check_call(mantis, spec, lm, sc["frames"], [np.array(e) for e in sc["ext"]], _kds(2, 640, 360),
                                 T0, loss)
    assert res.status == 0 and res.iterations_run == 4
    # pass 0's medians per view differ from the call's
    mantis.set_calib_robust(loss)
    try:
        spec.calibrate(mantis, spec.images(sc["frames"], sc["ext"], _kds(2, 640, 360)), 5, T0, record=1)
        own = []
        for r in range(5):
            keys, w = mantis.calib_robust_record(kind, r, 0)
            rec = spec.record(mantis, r, 0, sc["ext"], _kds(2, 640, 360))
            own.append(RB.py_median(keys, rec[3]))
        med = mantis.calib_robust_stats(kind).median_key[0]
    finally:
        mantis.set_calib_robust(None)
    print("medians: call", med, "views", own)
    assert med not in own and min(own) < med < max(own)


def test_odd_candidate_count(mantis, lm, knocked, landmark_map):
    """A map whose candidate count is odd: the last trip of an observation block has one half idle."""
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
        spec = QR.Spec("ext", free_ext=0b110)
        T_out, res, st = _check_call(mantis, spec, lm, [fr[1:] for fr in knocked["frames"][:2]], knocked["ext"][1:],
                                     knocked["kd"][1:], knocked["T0"][:2], "tukey", landmarks=landmarks)
        assert res.n_cand == nc and res.status == 0
    finally:
        mantis.set_map(w, r, g)


@pytest.mark.parametrize("cls", list(RR.ROW_CLASSES))
def test_trip_loop_tails(mantis, lm, knocked, landmark_map, cls):
    """The rig calibration with Tukey rows, two views of two cameras, on a map cut until a camera's n_cand rows --
    what one wave's weighted trip loop of the three 21-column tiles runs over -- end that loop another way
    (RR.ROW_CLASSES). The small classes leave the call STARVED, its record written."""
    cut, landmarks, nc = RR.cut_map(landmark_map, cls)
    try:
        mantis.set_map(*cut)
        spec = QR.Spec("rig", free_ext=0b10, free_int=0b11)
        T_out, res, st = _check_call(mantis, spec, lm, [fr[:2] for fr in knocked["frames"][:2]], knocked["ext"][:2],
                                     knocked["kd"][:2], knocked["T0"][:2], "tukey", landmarks=landmarks)
        assert res.n_cand == nc and RR.ROW_CLASSES[cls](res.n_cand)
        print(cls, nc, res.status, res.iterations_run, list(res.n_obs)[:5])
    finally:
        mantis.set_map(*landmark_map)


def test_small_pitched_frame(mantis, lm):
    """322 x 242 (neither a multiple of 4) with step_bytes = 1000 > 3 W: staged through the pitch conversion."""
    w, h = 322, 242
    sc = RR.rig_scene(2, 2, seed=7, w=w, h=h)
    T0 = [RR.shift(T) for T in sc["Twb"]]
    spec = QR.Spec("int", free_int=0b11)
    kds = _kds(2, w, h)
    T_out, res, st = _check_call(mantis, spec, lm, sc["frames"], [np.array(e) for e in sc["ext"]], kds, T0, "huber")
    imgs, keep = [], []
    for im, f in zip(spec.images(sc["frames"], sc["ext"], kds), [f for fr in sc["frames"] for f in fr]):
        buf = np.full((h, 3 * w + 34), 0xAB, np.uint8)  # rows 1000 bytes apart
        buf[:, : 3 * w] = f.reshape(h, 3 * w)
        keep.append(buf)
        im.bgr = buf.ctypes.data
        im.step_bytes = buf.strides[0]
        imgs.append(im)
    assert imgs[0].step_bytes == 1000 > 3 * w
    mantis.set_calib_robust("huber")
    try:
        T2, pitched = spec.calibrate(mantis, imgs, 2, T0)
        st2 = mantis.calib_robust_stats("int")
    finally:
        mantis.set_calib_robust(None)
    assert bytes(pitched) == bytes(res) and T2.tobytes() == T_out.tobytes() and bytes(st2) == bytes(st)


@pytest.mark.parametrize("kind,loss,I", [("ext", "tukey", 0), ("rig", "huber", 0), ("ext", "huber", 10),
                                         ("rig", "tukey", 10)])
def test_zero_and_ten_iterations(mantis, lm, knocked, kind, loss, I):
    spec = SPECS[kind]
    T_out, res, st = _check_call(mantis, spec, lm, knocked["frames"], knocked["ext"], knocked["kd"], knocked["T0"],
                                 loss, iterations=I)
    assert res.status == 0 and res.iterations_run == I
    if I == 0:  # every input bit for bit, and the stats of pass 0
        E, kd = spec.state_of(res, knocked["ext"], knocked["kd"])
        assert T_out.tobytes() == np.ascontiguousarray(np.array(knocked["T0"])).tobytes()
        assert E.tobytes() == np.ascontiguousarray(np.array(knocked["ext"])).tobytes()
        assert kd.tobytes() == np.ascontiguousarray(knocked["kd"]).tobytes()
        assert st.median_key[0] > 0 and 0 < st.sum_w[0] < res.n_obs[0] and sum(list(st.n_obs_view)) == res.n_obs[0]


def test_starved_by_the_weights(mantis, lm, knocked):
    """A tuning so small that a view keeps fewer than min_obs rows of positive weight: STARVED on pass 0 by the
    robust gate alone, the inputs back, and the host gate agrees (inside _check_call)."""
    rb_kw = {"tuning": 0.08}
    spec = QR.Spec("ext", free_ext=FREE, min_obs_cam=6)
    codes, Sw, Skw, rows, tie = spec.obs_all(knocked["T0"], knocked["ext"], knocked["kd"], knocked["frames"], lm,
                                             RR.default_params())
    got = QR.call_weights(codes, Sw, Skw, QR.robust_params("tukey", **rb_kw))
    pos = ((codes == 0).sum(axis=2) - got["cell_zero"]).sum(axis=1)
    images = spec.images(knocked["frames"], knocked["ext"], knocked["kd"])
    mantis.set_calib_robust("tukey", **rb_kw)
    try:
        T, res = spec.calibrate(mantis, images, 3, knocked["T0"], min_obs=int(pos.min()) + 1)
        st = mantis.calib_robust_stats("ext")
        T2, res2 = spec.calibrate(mantis, images, 3, knocked["T0"], min_obs=6)
    finally:
        mantis.set_calib_robust(None)
    assert (res.status, res.calibrated, res.iterations_run) == (1, 0, 0)
    assert T.tobytes() == np.ascontiguousarray(np.array(knocked["T0"])).tobytes()
    assert [st.n_obs_view[r] - st.n_zero_view[r] for r in range(3)] == list(pos) and min(st.n_obs_view[:3]) > 300
    assert res2.status != 1 or res2.iterations_run > 0
    T3, res3 = spec.calibrate(mantis, images, 3, knocked["T0"], min_obs=int(pos.min()) + 1)
    assert res3.status == 0, "the plain rule is not starved by that gate"


def _device_images(mantis, spec, frames, exts, kds):
    """(device buffer, images on it): every frame copied to the device."""
    import mantis_amd as M

    h, w = frames[0][0].shape[:2]
    fb, Cn = w * h * 3, len(exts)
    dev = mantis.device_alloc(fb * len(frames) * Cn)
    imgs = []
    for r, fr in enumerate(frames):
        for c, f in enumerate(fr):
            i = Cn * r + c
            mantis.h2d(dev + i * fb, f)
            imgs.append(M.make_image(None, IR.K_of(kds[c]), kds[c][4:], T_base_cam=exts[c], device_ptr=dev + i * fb,
                                     width=w, height=h))
    return dev, imgs


@pytest.mark.parametrize("kind", QR.KINDS)
def test_equal_bytes(mantis, knocked, kind):
    """a, b, c: the same call twice, host frames against device frames, and the switch set to NULL or loss 0
    against a fresh context's plain call."""
    import mantis_amd as M

    spec = SPECS[kind]
    images = spec.images(knocked["frames"], knocked["ext"], knocked["kd"])
    fresh = M.Mantis(max_cams=12, max_width=W, max_height=H)
    try:
        fresh.set_map(*mantis._map)
        T_f, plain = spec.calibrate(fresh, images, 3, knocked["T0"])
    finally:
        fresh.close()
    mantis.set_calib_robust("tukey")
    try:
        T_a, a = spec.calibrate(mantis, images, 3, knocked["T0"])
        st_a = mantis.calib_robust_stats(kind)
        T_b, b = spec.calibrate(mantis, images, 3, knocked["T0"])
        st_b = mantis.calib_robust_stats(kind)
        assert bytes(a) == bytes(b) and T_a.tobytes() == T_b.tobytes() and bytes(st_a) == bytes(st_b)
        assert a.calibrated == 1 and bytes(a) != bytes(plain)
        dev, dimgs = _device_images(mantis, spec, knocked["frames"], knocked["ext"], knocked["kd"])
        try:
            T_d, d = spec.calibrate(mantis, dimgs, 3, knocked["T0"])
            st_d = mantis.calib_robust_stats(kind)
        finally:
            mantis.device_free(dev)
        assert bytes(a) == bytes(d) and T_a.tobytes() == T_d.tobytes() and bytes(st_a) == bytes(st_d)
        for off in (None, 0):
            mantis.set_calib_robust(off)
            T_o, o = spec.calibrate(mantis, images, 3, knocked["T0"])
            assert bytes(o) == bytes(plain) and T_o.tobytes() == T_f.tobytes(), off
            with pytest.raises(Exception):
                mantis.calib_robust_stats(kind)  # that kind's last call ran with the switch off
            mantis.set_calib_robust("tukey")
    finally:
        mantis.set_calib_robust(None)


def test_the_two_switches_are_independent(mantis, knocked):
    """d, e: the refinement's switch changes no calibration byte, with the calibrations' own switch on or off;
    the calibrations' switch changes no mantis_refine_batch byte; rng_state and the prior are untouched."""
    sc = RB.rigs4()
    rimgs = SPECS["ext"].images([sc["frames"][0]], sc["ext"], knocked["kd"])
    T0 = RR.shift(sc["Twb"][0])
    prior = sc["Twb"][1]
    mantis.rng_state = 4242
    mantis.prior_pose = prior
    try:
        for kind in QR.KINDS:
            spec = SPECS[kind]
            images = spec.images(knocked["frames"], knocked["ext"], knocked["kd"])
            for cal in (None, "huber"):
                mantis.set_calib_robust(cal)
                mantis.set_refine_robust(None)
                T_a, a = spec.calibrate(mantis, images, 3, knocked["T0"])
                mantis.set_refine_robust("tukey")
                T_b, b = spec.calibrate(mantis, images, 3, knocked["T0"])
                assert bytes(a) == bytes(b) and T_a.tobytes() == T_b.tobytes(), (kind, cal)
        refs = {}
        for ref in (None, "tukey"):
            mantis.set_refine_robust(ref)
            for cal in (None, "tukey"):
                mantis.set_calib_robust(cal)
                refs[ref, cal] = bytes(mantis.refine_batch(rimgs, 1, T0)[0])
        assert refs[None, None] == refs[None, "tukey"] and refs["tukey", None] == refs["tukey", "tukey"]
        assert refs[None, None] != refs["tukey", None]
        assert mantis.rng_state == 4242 and np.array_equal(mantis.prior_pose, prior)
    finally:
        mantis.set_calib_robust(None)
        mantis.set_refine_robust(None)
        mantis.prior_pose = None


def test_getters_state_and_range_errors(knocked, landmark_map):
    import mantis_amd as M

    L = M.lib()
    m = M.Mantis(max_cams=12, max_width=W, max_height=H)
    try:
        m.set_map(*landmark_map)
        st = M.MantisCalibRobustStats()
        err = lambda: L.mantis_last_error(m.h).decode()
        for kind in range(3):  # no call yet
            assert L.mantis_get_calib_robust(m.h, kind, C.byref(st)) == ERR_STATE and "robust" in err()
            assert L.mantis_get_calib_robust_record(m.h, kind, 0, 0, None, None) == ERR_STATE
        spec = SPECS["ext"]
        images = spec.images(knocked["frames"], knocked["ext"], knocked["kd"])
        # the setter's errors by field; the setting stays
        m.set_calib_robust("huber")
        for field, value, word in (("struct_size", 8, "struct_size"), ("loss", 3, "loss"), ("loss", -1, "loss"),
                                   ("tuning", 0.0, "tuning"), ("tuning", float("nan"), "tuning"),
                                   ("tuning", float("inf"), "tuning"), ("scale_floor", 0.0, "scale_floor"),
                                   ("scale_floor", -1.0, "scale_floor"), ("scale_floor", float("inf"), "scale_floor")):
            p = QR.robust_params("tukey")
            setattr(p, field, value)
            assert L.mantis_calib_set_robust(m.h, C.byref(p)) == ERR_ARG and word in err(), (field, value, err())
        spec.calibrate(m, images, 3, knocked["T0"], record=1)
        assert m.calib_robust_stats("ext").loss == 1, "the rejected settings changed nothing"
        assert L.mantis_get_calib_robust(m.h, 0, None) == ERR_ARG
        assert L.mantis_get_calib_robust(m.h, 3, C.byref(st)) == ERR_ARG
        assert L.mantis_get_calib_robust(m.h, -1, C.byref(st)) == ERR_ARG
        for kind in (1, 2):  # each kind keeps its own
            assert L.mantis_get_calib_robust(m.h, kind, C.byref(st)) == ERR_STATE
        run = m.calib_robust_stats("ext")
        keys, w = m.calib_robust_record("ext", 2, 4)
        for rig, pass_ in ((3, 0), (-1, 0), (0, 5), (0, -1)):
            assert L.mantis_get_calib_robust_record(m.h, 0, rig, pass_, None, None) == ERR_ARG, (rig, pass_)
        assert L.mantis_get_calib_robust_record(m.h, 3, 0, 0, None, None) == ERR_ARG
        assert L.mantis_get_calib_robust_record(m.h, 0, 0, 0, None, None) == 0  # both pointers nullable
        only_w = np.zeros(keys.size)
        assert L.mantis_get_calib_robust_record(m.h, 0, 2, 4, None, only_w.ctypes.data) == 0
        assert np.array_equal(only_w, w)
        # a call without a record keeps the stats and no robust record; a call with the switch off neither
        spec.calibrate(m, images, 3, knocked["T0"])
        assert bytes(m.calib_robust_stats("ext")) == bytes(run)
        assert L.mantis_get_calib_robust_record(m.h, 0, 0, 0, None, None) == ERR_STATE
        m.set_calib_robust(None)
        spec.calibrate(m, images, 3, knocked["T0"], record=1)
        assert L.mantis_get_calib_robust(m.h, 0, C.byref(st)) == ERR_STATE
        assert L.mantis_get_calib_robust_record(m.h, 0, 0, 0, None, None) == ERR_STATE
        m.calib_record(0, 0)  # the plain record is there
    finally:
        m.close()


@pytest.mark.parametrize("kind", QR.KINDS)
def test_launch_counts(mantis, knocked, kind):
    """g: 5 (I + 1) launches with the switch on -- the observations, the two histogram launches, the views, the
    solve -- and 3 (I + 1) with it off."""
    spec = SPECS[kind]
    images = spec.images(knocked["frames"][:1], knocked["ext"], knocked["kd"])
    stem = {"ext": "calib", "int": "icalib", "rig": "rcalib"}[kind]
    mantis.set_profiling(1)
    try:
        for loss, per_pass in ((None, {"obs": 1, "rig": 1, "solve": 1}),
                               ("huber", {"obs": 1, "hist": 2, "rig": 1, "solve": 1})):
            mantis.set_calib_robust(loss)
            spec.calibrate(mantis, images, 1, knocked["T0"][:1], iterations=2)
            names = [n for n, _ in mantis.kernel_times()]
            for stage, n in per_pass.items():
                assert sum(x.startswith(f"{stem}_{stage}/") for x in names) == 3 * n, (loss, names)
            assert len(names) == 3 * sum(per_pass.values()), (loss, names)
    finally:
        mantis.set_profiling(0)
        mantis.set_calib_robust(None)


# ---- accuracy on the knocked scene, on the device's results ----
def _run(mantis, spec, sc, loss, iterations=10):
    mantis.set_calib_robust(loss)
    try:
        T, R = spec.calibrate(mantis, spec.images(sc["frames"], sc["ext"], sc["kd"]), len(sc["frames"]), sc["T0"],
                              iterations=iterations)
        st = mantis.calib_robust_stats(spec.kind) if loss else None
    finally:
        mantis.set_calib_robust(None)
    assert R.status == 0 and R.calibrated == 1 and R.iterations_run == iterations
    return T, R, st


def test_knocked_frame_on_the_device(mantis, knocked):
    """Each robust form ends camera 3's extrinsic at no more than half the plain form's error, and its stats name
    the knocked frame: view 1 and camera 3 have the lowest mean weight."""
    spec = SPECS["ext"]
    T, R, _ = _run(mantis, spec, knocked, None)
    plain = QR.ext_errors(spec.state_of(R, knocked["ext"], knocked["kd"])[0], knocked)
    print("plain: ext cm", [round(100 * e, 3) for e in plain])
    for loss in QR.LOSSES:
        T, R, st = _run(mantis, spec, knocked, loss)
        err = QR.ext_errors(spec.state_of(R, knocked["ext"], knocked["kd"])[0], knocked)
        view = [st.sum_w_view[r] / st.n_obs_view[r] for r in range(3)]
        cam = [st.sum_w_cam[c] / R.n_obs_cam[10][c] for c in range(4)]
        print(f"{loss}: ext cm", [round(100 * e, 3) for e in err], "poses cm",
              [round(100 * e, 2) for e in QR.pose_errors(T, knocked)], "mean weight per view",
              [round(v, 3) for v in view], "per camera", [round(v, 3) for v in cam])
        assert err[3] <= 0.5 * plain[3], (loss, err[3], plain[3])
        assert int(np.argmin(view)) == QR.KNOCK_VIEW and int(np.argmin(cam)) == QR.KNOCK_CAM


def test_clean_scene_on_the_device(mantis):
    """Without the knock each robust form stays within 0.02 cm of the plain form's extrinsic errors."""
    sc = QR.knocked_scene(clean=True)
    spec = SPECS["ext"]
    errs = {loss: np.array(QR.ext_errors(spec.state_of(_run(mantis, spec, sc, loss)[1], sc["ext"], sc["kd"])[0], sc))
            for loss in (None,) + QR.LOSSES}
    for loss in QR.LOSSES:
        print(loss, "clean: ext cm", np.round(100 * errs[loss], 3), "plain", np.round(100 * errs[None], 3))
        assert np.all(np.abs(errs[loss] - errs[None]) <= 0.0002), loss


@pytest.mark.parametrize("kind", ["int", "rig"])
def test_knocked_frame_with_a_perturbed_model(mantis, kind):
    """The knocked frame in the intrinsic and the rig calibration's own scenes: camera 3's model gap (and
    extrinsic), each bound the host build's figure plus a quarter of its distance to the plain form's
    (QR.MODEL_FIGURES)."""
    sc, spec, fig = QR.model_scene(kind), SPECS[kind], QR.MODEL_FIGURES[kind]
    for loss in (None,) + QR.LOSSES:
        T, R, st = _run(mantis, spec, sc, loss)
        E, kd = spec.state_of(R, sc["ext"], sc["kd"])
        gap = IR.model_gap(kd[3], sc["kd_true"][3])
        ext = 100 * RR.pose_dist(np.array(E[3]), np.array(sc["ext_true"][3]))[0]
        print(kind, loss, "camera 3: model gap px", round(gap, 3), "ext cm", round(ext, 3))
        if loss is None:
            assert abs(gap - fig[None][0]) < 0.001
            continue
        assert gap <= QR.margin(fig[loss][0], fig[None][0]), (loss, gap)
        if kind == "rig":
            assert ext <= QR.margin(fig[loss][1], fig[None][1]), (loss, ext)
