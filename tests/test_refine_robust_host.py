"""Robust rows of the line refinement, host side: the rules of
mantis_amd/csrc/mk_refine.h that k_refine_step_robust runs -- key, median,
scale, weight, the starved gate -- built for the host (hc_refine_robust_*)
against the rule of include/mantis.h in Python integers and numpy; the whole
iteration with the switch off (hc_refine_seq's bytes), on rigs with one drifted
camera and on clean rigs; the C-ABI's host-only entries.

Distances to the truth from the 2 cm / 1 degree start (this host build):
  one drifted camera   plain                Huber                Tukey
    rig 0              0.290 cm / 0.071     0.108 cm / 0.034     0.047 cm / 0.023 deg
    rig 1              0.213 cm / 0.054     0.074 cm / 0.018     0.035 cm / 0.009 deg
    rig 2              0.287 cm / 0.072     0.088 cm / 0.019     0.049 cm / 0.011 deg
  clean                0.043 / 0.014 / 0.018 cm   0.024 / 0.012 / 0.008 cm   0.018 / 0.014 / 0.009 cm
"""
import ctypes as C
import math

import numpy as np
import pytest

import _refine_ref as RR
import _refine_robust_ref as RB


@pytest.fixture(scope="module")
def lm(landmark_map):
    return RR.all_landmarks(landmark_map)


def test_key_against_python_integers():
    big = RB.SW_MAX
    cases = [(1, 0), (1, 1), (1, -1), (1, 15), (1, -15), (big, 0), (big, 15 * big), (big, -15 * big), (big, 1),
             (big, -1), (3, 2), (3, -2), (24576, 12345), (24576, -368639), (7, 105)]
    rng = np.random.default_rng(5)
    for _ in range(2000):
        sw = int(rng.integers(1, big + 1))
        cases.append((sw, int(rng.integers(-15 * sw, 15 * sw + 1))))
    for sw, skw in cases:
        assert RB.key(sw, skw) == RB.py_key(sw, skw), (sw, skw)
    assert RB.key(1, 15) == 15 << 20 == RB.key(big, -15 * big) and RB.key(big, 0) == 0
    assert max(RB.py_key(sw, skw) for sw, skw in cases) < 1 << 24


@pytest.mark.parametrize("n", [0, 1, 2, 3, 10, 11, 4320, 4321])
def test_median_is_the_lower_one(n):
    rng = np.random.default_rng(100 + n)
    rb = RB.robust_params("huber")
    keys = rng.integers(0, 1 << 24, n).astype(np.uint32)
    got = RB.weights(keys, None, rb)
    assert got["n_obs"] == n and got["median"] == (sorted(int(k) for k in keys)[(n - 1) // 2] if n else 0)
    # rejected slots do not count, wherever they are and whatever their key
    codes = rng.integers(0, 3, n).astype(np.int32)
    got = RB.weights(keys, codes, rb)
    assert got["median"] == RB.py_median(keys, codes) and got["n_obs"] == int((codes == 0).sum())
    assert not got["w"][codes != 0].any()
    # all keys equal, and many duplicates
    same = np.full(n, 123456, np.uint32)
    assert RB.weights(same, None, rb)["median"] == (123456 if n else 0)
    dup = rng.integers(0, 4, n).astype(np.uint32) << 12
    assert RB.weights(dup, None, rb)["median"] == RB.py_median(dup)


@pytest.mark.parametrize("loss", ["huber", "tukey"])
def test_weights_against_numpy(loss):
    rng = np.random.default_rng(9)
    # a core around 0.3 step and a tail out to 15 steps
    keys = np.concatenate([np.abs(rng.normal(0, 0.3, 1500)), rng.uniform(0, 15, 300)])
    keys = np.floor(keys * RB.KEY_UNIT).astype(np.uint32)
    codes = (rng.random(len(keys)) < 0.2).astype(np.int32) * 4
    for kw in ({}, {"scale_floor": 2.0}, {"tuning": 0.7, "scale_floor": 1e-3}):
        rb = RB.robust_params(loss, **kw)
        got = RB.weights(keys, codes, rb)
        w, m, sigma = RB.np_weights(keys, codes, rb.loss, rb.tuning, rb.scale_floor)
        assert got["median"] == m and got["scale"] == sigma
        assert (sigma == rb.scale_floor) == (kw.get("scale_floor") == 2.0), "one case sits on the floor"
        np.testing.assert_allclose(got["w"], w, rtol=1e-15, atol=0)
        live = codes == 0
        assert got["n_down"] == int((w[live] < 1).sum()) and got["n_zero"] == int((w[live] == 0).sum())
        assert got["n_pos"] == got["n_obs"] - got["n_zero"] and 0 < got["n_down"] <= got["n_obs"]
        assert (got["n_zero"] > 0) == (loss == "tukey")
        np.testing.assert_allclose(got["sum_w"], w.sum(), rtol=1e-13)
        assert np.all((got["w"] >= 0) & (got["w"] <= 1))


def test_weight_at_t_exactly_one():
    """tuning 2 on a scale at its floor of 0.5: t = u exactly, so key 2^20 is t = 1: Huber 1, Tukey 0."""
    one = RB.KEY_UNIT
    keys = np.array([0, 1, one - 1, one, one + 1, 2 * one, 0, 0, 0, 0, 0, 0], np.uint32)  # the median is 0: sigma = floor
    for loss, at_one, below, above in (("huber", 1.0, 1.0, 1.0 / ((one + 1) / one)),
                                        ("tukey", 0.0, (1.0 - ((one - 1) / one) ** 2) ** 2, 0.0)):
        got = RB.weights(keys, None, RB.robust_params(loss, tuning=2.0, scale_floor=0.5))
        assert got["median"] == 0 and got["scale"] == 0.5
        assert got["w"][0] == 1.0 and got["w"][3] == at_one and got["w"][2] == below and got["w"][4] == above
        assert got["w"][5] == (0.5 if loss == "huber" else 0.0)
    # the scale above its floor: 1.4826 x the median offset
    got = RB.weights(np.full(5, 3 * one, np.uint32), None, RB.robust_params("tukey"))
    assert got["scale"] == 1.4826 * 3.0 and got["n_down"] == 5 and got["n_zero"] == 0


def test_too_few_positive_weights_starve_the_pass():
    import mantis_amd as M

    rows = np.zeros((20, 7))
    rows[:, :6] = np.random.default_rng(3).normal(size=(20, 6))
    rows[:, 6] = 0.01
    acc = RR.accumulate(rows)
    L = RB.hc()

    def end(n_obs, n_pos, pass_=0, I=4):
        R = M.MantisRefineResult()
        for i in range(16):
            R.T_w_b[i] = np.eye(4).reshape(16)[i]
        done = L.hc_refine_end_pass_robust(acc.ctypes.data, n_obs, n_pos, pass_, I, 12, 0.0, C.byref(R))
        return done, R

    done, R = end(20, 11)
    assert done == 1 and R.status == 1 and R.iterations_run == 0 and R.n_obs[0] == 20
    assert R.rms[0] == math.sqrt(acc[27] / 20) and np.array_equal(np.array(R.T_w_b).reshape(4, 4), np.eye(4))
    done, R = end(20, 12)
    assert done == 0 and R.status == 0 and R.iterations_run == 1
    done, R = end(11, 11)  # the plain rule's starved pass
    assert done == 1 and R.status == 1 and R.n_obs[0] == 11
    done, R = end(20, 0, pass_=4)  # the final pass solves nothing and starves nothing
    assert done == 1 and R.status == 0 and R.n_obs[4] == 20


def test_switch_off_is_the_plain_refinement(lm):
    X, nw, nr, ng = lm
    sc = RB.rigs4()
    T0 = RR.shift(sc["Twb"][0])
    p = RR.default_params()
    plain = RR.seq(T0, sc["ext"], sc["frames"][0], X, nw, nr, ng, p)
    for rb in (None, RB.robust_params(0), RB.robust_params(0, tuning=float("nan"))):
        off, st = RB.seq_robust(T0, sc["ext"], sc["frames"][0], X, nw, nr, ng, p, rb)
        assert bytes(off) == bytes(plain)
        assert st.loss == 0 and not any(st.n_down) and not any(st.n_zero)
        assert [round(v) for v in st.sum_w] == list(plain.n_obs)  # every weight is 1


def _dist_cm(res, T):
    d, a = RR.pose_dist(np.array(res.T_w_b).reshape(4, 4), T)
    return 100 * d, a


def test_one_drifted_camera(lm):
    """Camera 3 rendered from a base pose 1.2 cm / 0.4 degrees away: each robust form ends at no more than half
    the plain refinement's distance from the truth, on every rig."""
    X, nw, nr, ng = lm
    sc, bad = RB.rigs4(), RB.contaminated_rigs4()
    p = RR.default_params()
    for r in range(3):
        T = sc["Twb"][r]
        T0 = RR.shift(T)
        plain = RR.seq(T0, sc["ext"], bad[r], X, nw, nr, ng, p)
        d_plain, a_plain = _dist_cm(plain, T)
        assert plain.refined == 1
        for loss in ("huber", "tukey"):
            res, st = RB.seq_robust(T0, sc["ext"], bad[r], X, nw, nr, ng, p, RB.robust_params(loss))
            d, a = _dist_cm(res, T)
            k = res.iterations_run
            print(f"rig {r} {loss}: plain {d_plain:.3f} cm / {a_plain:.3f} deg -> {d:.3f} cm / {a:.3f} deg; n_obs "
                  f"{res.n_obs[k]} down {st.n_down[k]} zero {st.n_zero[k]} scale {st.scale[k]:.3f} "
                  f"sum_w {st.sum_w[k]:.1f}")
            assert res.status == 0 and res.refined == 1 and k == 4
            assert d <= 0.5 * d_plain, (r, loss, d, d_plain)
            assert st.loss == RB.LOSSES[loss] and st.n_down[k] > 0 and st.sum_w[k] < res.n_obs[k]


def test_clean_rigs_are_no_worse(lm):
    """Without a drifted camera each robust form ends within 0.1 cm of the truth (the plain form's worst: 0.043)."""
    X, nw, nr, ng = lm
    sc = RB.rigs4()
    p = RR.default_params()
    for r in range(3):
        T = sc["Twb"][r]
        for loss in ("huber", "tukey"):
            res, st = RB.seq_robust(RR.shift(T), sc["ext"], sc["frames"][r], X, nw, nr, ng, p, RB.robust_params(loss))
            d, a = _dist_cm(res, T)
            print(f"rig {r} {loss}: {d:.4f} cm / {a:.4f} deg, scale {[round(s, 3) for s in st.scale[:5]]}")
            assert res.status == 0 and res.refined == 1 and d <= 0.1
            # entries past iterations_run are 0
            assert not any(st.median_key[5:]) and not any(st.scale[5:]) and not any(st.sum_w[5:])


def test_struct_sizes_defaults_and_null_arguments():
    import mantis_amd as M

    L = M.lib()
    for loss, tuning in ((0, 1.345), (1, 1.345), (2, 4.685)):
        p = M.MantisRefineRobustParams()
        L.mantis_default_refine_robust_params(loss, C.byref(p))
        assert (p.struct_size, p.loss, p.tuning, p.scale_floor) == (C.sizeof(M.MantisRefineRobustParams), loss, tuning,
                                                                    0.25)
    a, b = C.c_int32(), C.c_int32()
    L.mantis_refine_robust_sizes(C.byref(a), C.byref(b))
    assert a.value == C.sizeof(M.MantisRefineRobustParams) == RB.hc().hc_sizeof_refine_robust_params() == 24
    assert b.value == C.sizeof(M.MantisRefineRobustStats) == RB.hc().hc_sizeof_refine_robust_stats() == 320
    # the existing structs keep their sizes and the ABI its version
    L.mantis_refine_sizes(C.byref(a), C.byref(b))
    assert (a.value, b.value) == (C.sizeof(M.MantisRefineParams), C.sizeof(M.MantisRefineResult))
    assert L.mantis_abi_version() == 5
    L.mantis_default_refine_robust_params(1, None)
    L.mantis_refine_robust_sizes(None, None)
    p = RB.robust_params("huber")
    assert L.mantis_refine_set_robust(None, C.byref(p)) == 1
    assert L.mantis_refine_set_robust(None, None) == 1
    assert L.mantis_get_refine_robust(None, 0, None) == 1
    assert L.mantis_get_refine_robust_record(None, 0, 0, None, None) == 1
