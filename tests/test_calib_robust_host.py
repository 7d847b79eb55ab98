"""Robust rows of the three calibrations, host side: the rules of
mantis_amd/csrc/mk_linecal.h that k_linecal_hist and the robust instantiations
of k_linecal_rig / k_linecal_solve run -- the call-wide median, the weights, the
two extra starved gates -- built for the host (hc_linecal_robust_*,
hc_*_seq_robust, hc_*_end_pass_robust) against the rule of include/mantis.h in
Python integers and numpy; every pass of a whole call against numpy's solve of
the full weighted normal system; the switch off (hc_*_seq's bytes); and the
knocked scene of _calib_robust_ref.py: three views of the four-camera rig, the
frame of view 1, camera 3 taken after a knock of 3 cm / 1 degree, cameras 1-3
free, 10 iterations from the 2 cm / 1 degree start.

Figures of this host build on that scene (plain / Huber / Tukey):
  extrinsic calibration   camera 3's extrinsic   0.519 / 0.205 / 0.144 cm
                          the views' poses        0.17 0.21 0.15 / 0.09 0.05 0.07 / 0.07 0.03 0.06 cm
                          clean scene, extrinsics within 0.010 cm of the plain form's
  intrinsic calibration   camera 3's model gap    0.697 / 0.274 / 0.131 px  (IR.gap_scene's lenses)
                          cameras 0-2, worst      0.351 / 0.123 / 0.123 px
  rig calibration         camera 3's extrinsic    1.799 / 0.500 / 0.160 cm  (RC.joint_scene's rig)
                          camera 3's model gap    5.446 / 1.705 / 0.229 px
  mean weight of view 1 / camera 3 against the rest: 0.92 / 0.90 against 0.99 (Huber), 0.88 / 0.86 against 0.97
  (Tukey) in the extrinsic calibration.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _calib_robust_ref as QR
import _icalib_ref as IR
import _rcalib_ref as RC
import _refine_ref as RR
import _refine_robust_ref as RB
from mantis_amd import synth

FREE = 0b1110
SPECS = {"ext": QR.Spec("ext", free_ext=FREE), "int": QR.Spec("int", free_int=0b1111),
         "rig": QR.Spec("rig", free_ext=FREE, free_int=0b1111)}


@pytest.fixture(scope="module")
def lm(landmark_map):
    return RR.all_landmarks(landmark_map)


@pytest.fixture(scope="module")
def knocked():
    return QR.knocked_scene()


@pytest.fixture(scope="module")
def first_pass(knocked, lm):
    """The slots of pass 0 of the knocked scene (extrinsic rows): codes, Sw, Skw [3, 4, 540], rows, tie."""
    return SPECS["ext"].obs_all(knocked["T0"], knocked["ext"], knocked["kd"], knocked["frames"], lm,
                                RR.default_params())


def test_sizes_defaults_and_null_arguments():
    import mantis_amd as M

    L = M.lib()
    a, b = C.c_int32(), C.c_int32()
    L.mantis_calib_robust_sizes(C.byref(a), C.byref(b))
    assert a.value == C.sizeof(M.MantisRefineRobustParams) == 24
    assert b.value == C.sizeof(M.MantisCalibRobustStats) == QR.hc().hc_sizeof_calib_robust_stats()
    assert b.value == 16 + 3 * 44 + 4 + 2 * 88 + 2 * 1024 + 2048 + 32 + 64
    # the existing structs keep their sizes and the ABI its version
    for sizes, structs in ((L.mantis_calib_sizes, (M.MantisCalibParams, M.MantisCalibResult)),
                           (L.mantis_icalib_sizes, (M.MantisIcalibParams, M.MantisIcalibResult)),
                           (L.mantis_rcalib_sizes, (M.MantisRcalibParams, M.MantisRcalibResult)),
                           (L.mantis_refine_robust_sizes, (M.MantisRefineRobustParams, M.MantisRefineRobustStats))):
        sizes(C.byref(a), C.byref(b))
        assert (a.value, b.value) == tuple(C.sizeof(s) for s in structs)
    assert L.mantis_abi_version() == 5
    L.mantis_calib_robust_sizes(None, None)
    p = QR.robust_params("tukey")
    assert (p.loss, p.tuning, p.scale_floor) == (2, 4.685, 0.25)  # the refinement's defaults
    st = M.MantisCalibRobustStats()
    assert L.mantis_calib_set_robust(None, C.byref(p)) == 1 and L.mantis_calib_set_robust(None, None) == 1
    assert L.mantis_get_calib_robust(None, 0, C.byref(st)) == 1
    assert L.mantis_get_calib_robust_record(None, 0, 0, 0, None, None) == 1


def _slots(keys, codes=None, shape=None):
    """Keys as slots of a call: Sw = 2^20 and Skw = key give floor(key 2^20 / 2^20) = key (keys below 2^24 need
    Skw <= 15 Sw: keys below 15 x 2^20 here)."""
    keys = np.asarray(keys, np.int64)
    assert keys.size == 0 or keys.max() <= 15 << 20
    shape = shape or (1, 1, keys.size)
    codes = np.zeros(keys.size, np.int32) if codes is None else np.asarray(codes, np.int32)
    return codes.reshape(shape), np.full(shape, 1 << 20, np.int32), keys.astype(np.int32).reshape(shape)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 12, 4320])
def test_call_wide_median_is_the_lower_one(n):
    rng = np.random.default_rng(300 + n)
    rb = QR.robust_params("huber")
    keys = rng.integers(0, 15 << 20, n)
    shape = (3, 4, n // 12) if n >= 12 else (1, 1, n)
    got = QR.call_weights(*_slots(keys, shape=shape), rb)
    assert got["n_obs"] == n and got["median"] == (sorted(int(k) for k in keys)[(n - 1) // 2] if n else 0)
    assert np.array_equal(got["keys"].reshape(-1), keys.astype(np.uint32))
    # rejected slots do not count, wherever they are and whatever their sums; key and weight 0 there
    codes = rng.integers(0, 3, n).astype(np.int32)
    got = QR.call_weights(*_slots(keys, codes, shape), rb)
    assert got["median"] == RB.py_median(keys, codes) and got["n_obs"] == int((codes == 0).sum())
    dead = codes.reshape(shape) != 0
    assert not got["w"][dead].any() and not got["keys"][dead].any()
    assert got["cell_zero"].sum() == got["n_zero"] and got["cell_down"].sum() == got["n_down"]
    # all keys equal
    same = np.full(n, 123456)
    assert QR.call_weights(*_slots(same, shape=shape), rb)["median"] == (123456 if n else 0)


def test_full_count_of_the_call(first_pass):
    codes, Sw, Skw, rows, tie = first_pass
    assert codes.shape == (3, 4, 540)
    for loss in QR.LOSSES:
        rb = QR.robust_params(loss)
        got = QR.call_weights(codes, Sw, Skw, rb)
        keys, w, m, sigma = QR.np_call_weights(codes, Sw, Skw, rb)
        live = codes == 0
        assert got["n_obs"] == int(live.sum()) > 1500
        assert got["median"] == m == sorted(int(k) for k in keys[live])[(got["n_obs"] - 1) // 2]
        assert got["scale"] == sigma and np.array_equal(got["keys"], keys)
        np.testing.assert_allclose(got["w"], w, rtol=1e-15, atol=0)
        for r in range(3):
            for c in range(4):
                wl = w[r, c][live[r, c]]
                assert got["cell_down"][r, c] == int((wl < 1).sum()) and got["cell_zero"][r, c] == int((wl == 0).sum())
                np.testing.assert_allclose(got["cell_sum_w"][r, c], wl.sum(), rtol=1e-13)


def test_call_wide_median_differs_from_every_views_own(knocked, lm):
    """One view at the truth and one at the shifted start: the call's median lies between the two views' own
    medians and equals neither, so a per-view selection cannot give it."""
    p = RR.default_params()
    Ts = [knocked["Twb"][0], knocked["T0"][2]]
    frames = [QR.knocked_scene(clean=True)["frames"][0], QR.knocked_scene(clean=True)["frames"][2]]
    codes, Sw, Skw, rows, tie = SPECS["ext"].obs_all(Ts, knocked["ext"], knocked["kd"], frames, lm, p)
    rb = QR.robust_params("tukey")
    got = QR.call_weights(codes, Sw, Skw, rb)
    own = [QR.call_weights(codes[r:r + 1], Sw[r:r + 1], Skw[r:r + 1], rb)["median"] for r in range(2)]
    print("medians: call", got["median"], "views", own)
    assert own[0] < got["median"] < own[1]
    keys = RB.keys_of(codes.reshape(-1), Sw.reshape(-1), Skw.reshape(-1))
    assert got["median"] == RB.py_median(keys, codes.reshape(-1))
    # and the weights follow the call's scale, not the views'
    w, m, sigma = RB.np_weights(keys, codes.reshape(-1), rb.loss, rb.tuning, rb.scale_floor)
    assert got["scale"] == sigma > rb.scale_floor
    np.testing.assert_allclose(got["w"].reshape(-1), w, rtol=1e-15, atol=0)


@pytest.mark.parametrize("loss", QR.LOSSES)
def test_weights_against_numpy(loss):
    rng = np.random.default_rng(9)
    keys = np.concatenate([np.abs(rng.normal(0, 0.3, 1500)), rng.uniform(0, 14.9, 300)])
    keys = np.floor(keys * RB.KEY_UNIT).astype(np.int64)
    codes = (rng.random(len(keys)) < 0.2).astype(np.int32) * 4
    shape = (3, 4, 150)
    for kw in ({}, {"scale_floor": 2.0}, {"tuning": 0.7, "scale_floor": 1e-3}):
        rb = QR.robust_params(loss, **kw)
        got = QR.call_weights(*_slots(keys, codes, shape), rb)
        w, m, sigma = RB.np_weights(keys.astype(np.uint32), codes, rb.loss, rb.tuning, rb.scale_floor)
        assert got["median"] == m and got["scale"] == sigma
        assert (sigma == rb.scale_floor) == (kw.get("scale_floor") == 2.0), "one case sits on the floor"
        np.testing.assert_allclose(got["w"].reshape(-1), w, rtol=1e-15, atol=0)
        live = codes == 0
        assert got["n_down"] == int((w[live] < 1).sum()) and got["n_zero"] == int((w[live] == 0).sum())
        assert got["n_pos"] == got["n_obs"] - got["n_zero"] and (got["n_zero"] > 0) == (loss == "tukey")
        np.testing.assert_allclose(got["sum_w"], w.sum(), rtol=1e-13)


def test_weight_at_t_exactly_one():
    """tuning 2 on a scale at its floor of 0.5: t = u exactly, so key 2^20 is t = 1: Huber 1, Tukey 0."""
    one = RB.KEY_UNIT
    keys = np.array([0, 1, one - 1, one, one + 1, 2 * one, 0, 0, 0, 0, 0, 0])
    for loss, at_one, above in (("huber", 1.0, 1.0 / ((one + 1) / one)), ("tukey", 0.0, 0.0)):
        got = QR.call_weights(*_slots(keys, shape=(2, 2, 3)), QR.robust_params(loss, tuning=2.0, scale_floor=0.5))
        w = got["w"].reshape(-1)
        assert got["median"] == 0 and got["scale"] == 0.5
        assert w[0] == 1.0 and w[3] == at_one and w[4] == above and w[5] == (0.5 if loss == "huber" else 0.0)


def test_tally_orders_and_pos():
    """The stats of a pass from its cells: per view in camera order, per camera in view order, the pass's sum the
    views' sums in view order."""
    rng = np.random.default_rng(2)
    N, Cn = 5, 3
    cnt = rng.integers(50, 400, (N, Cn)).astype(np.int32)
    zero = (cnt * rng.random((N, Cn)) * 0.3).astype(np.int32)
    down = zero + 5
    sw = rng.random((N, Cn)) * cnt
    st = QR.tally(down, zero, sw, cnt, 3, 777, 0.5)
    assert st.median_key[3] == 777 and st.scale[3] == 0.5 and not any(st.median_key[:3])
    assert st.n_down[3] == int(down.sum()) and st.n_zero[3] == int(zero.sum())
    views = [sum(sw[r].tolist()) for r in range(N)]
    assert list(st.sum_w_view)[:N] == views and st.sum_w[3] == sum(views)
    assert list(st.sum_w_cam)[:Cn] == [sum(sw[:, c].tolist()) for c in range(Cn)]
    assert list(st.n_obs_view)[:N] == list(cnt.sum(axis=1)) and list(st.n_zero_view)[:N] == list(zero.sum(axis=1))
    assert list(st.n_zero_cam)[:Cn] == list(zero.sum(axis=0))
    assert not any(list(st.n_obs_view)[N:]) and not any(list(st.sum_w_cam)[Cn:])


@pytest.mark.parametrize("kind", QR.KINDS)
def test_starved_gates_of_the_end_of_a_pass(kind):
    """A view, then a free camera, with too few rows of positive weight stop the pass with STARVED; a held
    camera with none does not; the final pass starves nothing."""
    rng = np.random.default_rng(4)
    spec = QR.Spec(kind, free_ext=0b10, free_int=0b10)
    N, Cn = 2, 2
    acc = np.zeros((N, Cn, spec.ACC))
    for r in range(N):
        for c in range(Cn):
            rows = rng.normal(size=(80, spec.ROW)) * 0.1
            if c == 0:
                rows[:, 6:spec.ROW - 1] = 0.0  # the held camera
            acc[r, c] = spec.accumulate(rows)
    cnt = np.full((N, Cn), 80, np.int32)
    p = RR.default_params()  # min_obs 12... the camera gate: min_obs_cam 60
    exts = [np.eye(4)] * 2
    kds = np.tile(QR.float_kd(*synth.intrinsics(RR.W, RR.H_)), (2, 1))
    T0 = [np.eye(4)] * 2

    def end(pos, pass_=0, I=4):
        R = spec.new_result(exts, kds, N)
        fin, Tn, d = spec.end_pass(acc, cnt, pos, pass_, I, p, T0, R)
        return fin, R, Tn

    moc = spec.kparams().min_obs_cam
    fin, R, Tn = end(None)
    assert not fin and R.status == 0 and R.iterations_run == 1, "the plain gate passes"
    fin, R, Tn = end(cnt.copy())
    assert not fin and R.status == 0, "every weight positive"
    view = np.array([[80, 80], [p.min_obs - 6, 5]], np.int32)  # view 1: min_obs - 1 rows of positive weight
    fin, R, Tn = end(view)
    assert fin and R.status == 1 and R.iterations_run == 0 and np.array_equal(Tn, np.array(T0))
    assert R.n_obs[0] == 320 and R.rms[0] == math.sqrt(sum(acc.reshape(-1, spec.ACC)[:, -1].tolist()) / 320)
    cam = np.array([[80, moc // 2], [80, moc - 1 - moc // 2]], np.int32)  # the free camera: min_obs_cam - 1
    fin, R, Tn = end(cam)
    assert fin and R.status == 1
    cam[1, 1] += 1
    assert not end(cam)[0]
    held = np.array([[0, 80], [0, 80]], np.int32)  # the held camera has no gate of its own
    assert not end(held)[0]
    fin, R, Tn = end(view, pass_=4)
    assert fin and R.status == 0 and R.n_obs[4] == 320


@pytest.mark.parametrize("kind", QR.KINDS)
def test_switch_off_is_the_plain_calibration(kind, knocked, lm):
    spec = SPECS[kind]
    p = RR.default_params()
    T_plain, plain = spec.plain_seq(knocked["T0"], knocked["ext"], knocked["kd"], knocked["frames"], lm, p)
    for rb in (None, QR.robust_params(0), QR.robust_params(0, tuning=float("nan"))):
        T, R, st = spec.seq(knocked["T0"], knocked["ext"], knocked["kd"], knocked["frames"], lm, p, rb)
        assert bytes(R) == bytes(plain) and T.tobytes() == T_plain.tobytes()
        assert bytes(st) == bytes(type(st)()), "no stats with the switch off"


@pytest.mark.parametrize("loss", QR.LOSSES)
@pytest.mark.parametrize("kind", QR.KINDS)
def test_every_pass_against_the_full_weighted_system(kind, loss, knocked, lm):
    """hc_*_seq_robust replayed pass by pass: the slots at the pass's estimates, the weights of the rule in numpy
    over all slots of the call, numpy's solve of the full normal system of the weighted rows against the step the
    host rule takes from the same rows (1e-10 of each vector's norm, or the solve's own error bound where that is
    larger: see below), and at the end the whole call's bytes."""
    spec = SPECS[kind]
    I = 3
    p, rb = RR.default_params(iterations=I), QR.robust_params(loss)
    T_seq, R_seq, st = spec.seq(knocked["T0"], knocked["ext"], knocked["kd"], knocked["frames"], lm, p, rb)
    assert R_seq.status == 0 and R_seq.iterations_run == I and st.loss == rb.loss and st.kind == spec.index
    Ts, E, kd = np.array(knocked["T0"]), np.array(knocked["ext"]), np.array(knocked["kd"])
    N, Cn = 3, 4
    for k in range(I + 1):
        codes, Sw, Skw, rows, tie = spec.obs_all(Ts, E, kd, knocked["frames"], lm, p)
        keys, w, m, sigma = QR.np_call_weights(codes, Sw, Skw, rb)
        got = QR.call_weights(codes, Sw, Skw, rb)
        assert st.median_key[k] == m == got["median"] and st.scale[k] == sigma
        live = codes == 0
        assert st.n_down[k] == int((w[live] < 1).sum()) and st.n_zero[k] == int((w[live] == 0).sum())
        np.testing.assert_allclose(st.sum_w[k], w.sum(), rtol=1e-13)
        assert R_seq.n_obs[k] == int(live.sum())
        wrows = rows * np.sqrt(got["w"])[..., None]
        acc = np.array([[spec.accumulate(wrows[r, c]) for c in range(Cn)] for r in range(N)])
        cnt = live.sum(axis=2).astype(np.int32)
        np.testing.assert_allclose(R_seq.rms[k], math.sqrt(acc[:, :, -1].sum() / cnt.sum()), rtol=1e-13)
        if k == I:
            break
        R = spec.new_result(E, kd, N)
        fin, Tn, delta = spec.end_pass(acc, cnt, cnt - got["cell_zero"], k, I, p, Ts, R)
        assert not fin
        Hm, g = spec.np_normal(np.array([[spec.np_acc(wrows[r, c])[0] for c in range(Cn)] for r in range(N)]),
                               p.lambda_)
        x = np.linalg.solve(Hm, -g)
        eps = spec.steps(R, k, Cn)
        # with J_int the full system's condition number is in the 10^6 to 10^8 range and numpy's own solve is no
        # better than the forward-error bound of the intrinsic and rig calibrations' own tests, 10^3 2^-53 cond_2(H)
        # |x|: the bound is that or 1e-10 of the norm, whichever is larger (ext: cond in the 10^2 range, 1e-10)
        own = 0.0 if kind == "ext" else 1e3 * 2.0 ** -53 * np.linalg.cond(Hm) * np.linalg.norm(x)
        e_pose, e_cam = np.linalg.norm(delta.reshape(-1) - x[:6 * N]), np.linalg.norm(eps - x[6 * N:])
        print(f"{kind} {loss} pass {k}: cond(H) {np.linalg.cond(Hm):.3g} errors {e_pose:.2e} {e_cam:.2e} of "
              f"{np.linalg.norm(x[:6 * N]):.2e} {np.linalg.norm(x[6 * N:]):.2e}, the solve's own bound {own:.2e}")
        assert e_pose <= max(1e-10 * np.linalg.norm(x[:6 * N]), own), k
        assert e_cam <= max(1e-10 * np.linalg.norm(x[6 * N:]), own), k
        assert np.array_equal(eps, spec.steps(R_seq, k, Cn)), "the whole call takes the same step"
        Ts = Tn
        E, kd = spec.state_of(R, E, kd)
    E_seq, kd_seq = spec.state_of(R_seq, knocked["ext"], knocked["kd"])
    assert Ts.tobytes() == T_seq.tobytes() and E.tobytes() == E_seq.tobytes() and kd.tobytes() == kd_seq.tobytes()
    # the last pass's per-view and per-camera figures
    wl = np.where(live, w, 0.0)
    assert list(st.n_obs_view)[:N] == list(cnt.sum(axis=1)) and not any(list(st.n_obs_view)[N:])
    np.testing.assert_allclose(list(st.sum_w_view)[:N], wl.sum(axis=(1, 2)), rtol=1e-13)
    np.testing.assert_allclose(list(st.sum_w_cam)[:Cn], wl.sum(axis=(0, 2)), rtol=1e-13)
    assert list(st.n_zero_view)[:N] == list((live & (w == 0)).sum(axis=(1, 2)))
    assert list(st.n_zero_cam)[:Cn] == list((live & (w == 0)).sum(axis=(0, 2)))
    assert not any(st.median_key[I + 1:]) and not any(st.sum_w[I + 1:])


@pytest.mark.parametrize("kind", QR.KINDS)
def test_zero_iterations_return_the_inputs_and_fill_pass_zero(kind, knocked, lm):
    spec = SPECS[kind]
    p = RR.default_params(iterations=0)
    T, R, st = spec.seq(knocked["T0"], knocked["ext"], knocked["kd"], knocked["frames"], lm, p,
                        QR.robust_params("tukey"))
    E, kd = spec.state_of(R, knocked["ext"], knocked["kd"])
    assert T.tobytes() == np.ascontiguousarray(np.array(knocked["T0"])).tobytes()
    assert E.tobytes() == np.ascontiguousarray(np.array(knocked["ext"])).tobytes()
    assert kd.tobytes() == np.ascontiguousarray(knocked["kd"]).tobytes()
    assert (R.status, R.iterations_run) == (0, 0) and R.n_obs[0] > 1000
    assert st.median_key[0] > 0 and st.scale[0] > 0 and 0 < st.sum_w[0] < R.n_obs[0] and st.n_down[0] > 0
    assert sum(list(st.n_obs_view)) == R.n_obs[0]


def test_a_tiny_tuning_starves_a_view_then_a_camera(knocked, lm):
    """Tukey with a tuning so small that only rows within a hair of the line keep a positive weight. With the
    views' gate just above the rows view 1 keeps, that view starves pass 0 while every view has hundreds of
    code-0 rows; with the views' gate at its floor and the cameras' just above what camera 3 keeps, the camera
    starves it."""
    spec = SPECS["ext"]
    rb = QR.robust_params("tukey", tuning=0.08, scale_floor=0.25)  # w > 0 below 0.02 sample steps or so
    codes, Sw, Skw, rows, tie = spec.obs_all(knocked["T0"], knocked["ext"], knocked["kd"], knocked["frames"], lm,
                                             RR.default_params())
    got = QR.call_weights(codes, Sw, Skw, rb)
    cnt = (codes == 0).sum(axis=2)
    pos = cnt - got["cell_zero"]
    per_view, per_cam = pos.sum(axis=1), pos.sum(axis=0)
    print("code-0 rows", cnt.sum(axis=1), cnt.sum(axis=0), "with w > 0", per_view, per_cam)
    assert cnt.sum(axis=1).min() > 300 and per_view.min() >= 6 and per_view.max() < 200
    # a view
    p = RR.default_params(min_obs=int(per_view.min()) + 1)
    T, R, st = QR.Spec("ext", free_ext=FREE, min_obs_cam=6).seq(knocked["T0"], knocked["ext"], knocked["kd"],
                                                                 knocked["frames"], lm, p, rb)
    assert (R.status, R.calibrated, R.iterations_run) == (1, 0, 0) and R.n_obs[0] == int(cnt.sum())
    assert T.tobytes() == np.ascontiguousarray(np.array(knocked["T0"])).tobytes()
    assert st.n_zero[0] == int(got["cell_zero"].sum()) and st.n_obs_view[1] - st.n_zero_view[1] == per_view[1]
    T2, R2, _ = QR.Spec("ext", free_ext=FREE, min_obs_cam=6).seq(knocked["T0"], knocked["ext"], knocked["kd"],
                                                                  knocked["frames"], lm, p, None)
    assert R2.status == 0, "the plain rule is not starved by that gate"
    # a free camera
    free = [c for c in (1, 2, 3)]
    worst = min(int(per_cam[c]) for c in free)
    p = RR.default_params(min_obs=6)
    assert per_view.min() >= 6 and worst >= 6
    T, R, st = QR.Spec("ext", free_ext=FREE, min_obs_cam=worst + 1).seq(knocked["T0"], knocked["ext"], knocked["kd"],
                                                                       knocked["frames"], lm, p, rb)
    assert (R.status, R.iterations_run) == (1, 0)
    T, R, st = QR.Spec("ext", free_ext=FREE, min_obs_cam=worst).seq(knocked["T0"], knocked["ext"], knocked["kd"],
                                                                   knocked["frames"], lm, p, rb)
    assert R.status != 1 or R.iterations_run > 0, "at the gate's own count pass 0 is not starved"


# ---- accuracy on the knocked scene (the figures of the module's docstring) ----
@pytest.fixture(scope="module")
def ext_runs(knocked, lm):
    p = RR.default_params(iterations=10)
    out = {}
    for loss in (None,) + QR.LOSSES:
        rb = None if loss is None else QR.robust_params(loss)
        out[loss] = SPECS["ext"].seq(knocked["T0"], knocked["ext"], knocked["kd"], knocked["frames"], lm, p, rb)
    return out


def test_knocked_frame_extrinsic_calibration(ext_runs, knocked):
    """Each robust form ends camera 3's extrinsic at no more than half the plain form's error."""
    T, R, _ = ext_runs[None]
    plain = QR.ext_errors(SPECS["ext"].state_of(R, knocked["ext"], knocked["kd"])[0], knocked)
    print("plain: ext cm", [round(100 * e, 3) for e in plain], "poses cm",
          [round(100 * e, 2) for e in QR.pose_errors(T, knocked)], "rms x fx", round(R.rms[10] * 323.15, 2))
    for loss in QR.LOSSES:
        T, R, st = ext_runs[loss]
        err = QR.ext_errors(SPECS["ext"].state_of(R, knocked["ext"], knocked["kd"])[0], knocked)
        print(f"{loss}: ext cm", [round(100 * e, 3) for e in err], "poses cm",
              [round(100 * e, 2) for e in QR.pose_errors(T, knocked)], "rms x fx", round(R.rms[10] * 323.15, 2))
        assert R.status == 0 and R.calibrated == 1 and R.iterations_run == 10
        assert err[3] <= 0.5 * plain[3], (loss, err[3], plain[3])
        assert max(QR.pose_errors(T, knocked)) < max(QR.pose_errors(ext_runs[None][0], knocked))


def test_the_stats_name_the_knocked_frame(ext_runs):
    for loss in QR.LOSSES:
        T, R, st = ext_runs[loss]
        fp = R.iterations_run
        view = [st.sum_w_view[r] / st.n_obs_view[r] for r in range(3)]
        cam = [st.sum_w_cam[c] / R.n_obs_cam[fp][c] for c in range(4)]
        print(loss, "mean weight per view", [round(v, 3) for v in view], "per camera", [round(v, 3) for v in cam])
        assert int(np.argmin(view)) == QR.KNOCK_VIEW and int(np.argmin(cam)) == QR.KNOCK_CAM


def test_clean_scene_loses_nothing(lm):
    """Without the knock each robust form stays within 0.02 cm of the plain form's extrinsic errors."""
    sc = QR.knocked_scene(clean=True)
    p = RR.default_params(iterations=10)
    errs = {}
    for loss in (None,) + QR.LOSSES:
        rb = None if loss is None else QR.robust_params(loss)
        T, R, st = SPECS["ext"].seq(sc["T0"], sc["ext"], sc["kd"], sc["frames"], lm, p, rb)
        assert R.status == 0 and R.calibrated == 1
        errs[loss] = np.array(QR.ext_errors(SPECS["ext"].state_of(R, sc["ext"], sc["kd"])[0], sc))
    for loss in QR.LOSSES:
        print(loss, "clean: ext cm", np.round(100 * errs[loss], 3), "plain", np.round(100 * errs[None], 3))
        assert np.all(np.abs(errs[loss] - errs[None]) <= 0.0002), loss


def _model_figures(kind, loss, lm):
    sc = QR.model_scene(kind)
    spec = SPECS[kind]
    rb = None if loss is None else QR.robust_params(loss)
    T, R, st = spec.seq(sc["T0"], sc["ext"], sc["kd"], sc["frames"], lm, RR.default_params(iterations=10), rb)
    assert R.status == 0 and R.calibrated == 1 and R.iterations_run == 10
    E, kd = spec.state_of(R, sc["ext"], sc["kd"])
    gap = [IR.model_gap(kd[c], sc["kd_true"][c]) for c in range(4)]
    ext = [100 * RR.pose_dist(np.array(E[c]), np.array(sc["ext_true"][c]))[0] for c in range(4)]
    print(kind, loss, "model gap px", [round(v, 3) for v in gap], "ext cm", [round(v, 3) for v in ext])
    return gap, ext


def test_knocked_frame_intrinsic_calibration(lm):
    """The same knocked frame in the intrinsic calibration's own perturbed-lens scene: camera 3's model gap. What
    this host build measured (QR.MODEL_FIGURES, the module's docstring), each bound the figure plus a quarter of
    its distance to the plain form's."""
    fig = QR.MODEL_FIGURES["int"]
    gap, _ = _model_figures("int", None, lm)
    assert abs(gap[3] - fig[None][0]) < 0.001
    for loss in QR.LOSSES:
        gap, _ = _model_figures("int", loss, lm)
        assert gap[3] <= QR.margin(fig[loss][0], fig[None][0]), (loss, gap)


def test_knocked_frame_rig_calibration(lm):
    """And in the rig calibration's scene (lenses and extrinsics off nominal): camera 3's extrinsic and model gap,
    bounds by the same rule."""
    fig = QR.MODEL_FIGURES["rig"]
    gap, ext = _model_figures("rig", None, lm)
    assert abs(gap[3] - fig[None][0]) < 0.001 and abs(ext[3] - fig[None][1]) < 0.001
    for loss in QR.LOSSES:
        gap, ext = _model_figures("rig", loss, lm)
        assert gap[3] <= QR.margin(fig[loss][0], fig[None][0]), (loss, gap)
        assert ext[3] <= QR.margin(fig[loss][1], fig[None][1]), (loss, ext)
