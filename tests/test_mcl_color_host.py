"""Monte Carlo localization, the colour evidence, host side: the rules of
mantis_amd/csrc/mk_mcl_color.h -- the very functions k_mcl_color and
k_mcl_weight run -- built for the host (build/libmantis_hostcheck.so
hc_mcl_color_*) against numpy restatements written here and the CPU oracle's
COLOR evaluator. tools/mclcolorcheck_main.cpp drives the same rules
stand-alone (for a sanitizer build of mk_mcl_color.h).
"""
import ctypes as C
import math

import numpy as np

import _hostcheck as H
import _oracle as O

DBL_MAX = np.finfo(np.float64).max
GREEN = (50, 255, 85)  # B, G, R


def _hc():
    L = H.lib()
    vp = C.c_void_p
    L.hc_mcl_color_window.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double]
    L.hc_mcl_color_window.restype = C.c_int32
    L.hc_mcl_color_sums.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp]
    L.hc_mcl_color_sums.restype = None
    L.hc_mcl_color_charge.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int32, C.c_double, C.c_double, vp, vp, vp]
    L.hc_mcl_color_charge.restype = None
    L.hc_mcl_color_fold.argtypes = [vp, vp, vp, vp, C.c_int, C.c_double, C.c_int32, vp]
    L.hc_mcl_color_fold.restype = None
    return L


# ---------------------------------------------------------- the rules restated
def np_window(img, u, v):
    """Sum over ox, oy in -5..4 of |pixel - GREEN|^2 at linear offset
    rint(v + oy) W + rint(u + ox); an offset outside the buffer reads 0, 0, 0."""
    Hh, Ww = img.shape[:2]
    flat = img.reshape(-1, 3).astype(np.int64)
    total = 0
    for oy in range(-5, 5):
        y = int(np.rint(v + float(oy)))
        for ox in range(-5, 5):
            x = int(np.rint(u + float(ox)))
            lin = y * Ww + x
            px = flat[lin] if 0 <= lin < Ww * Hh else np.zeros(3, np.int64)
            total += int(((px - np.array(GREEN)) ** 2).sum())
    return total


def np_color_pool(csums, ccounts, min_color):
    """(Ec, n): Ec = sum csum / (sum cn * 100 * 1.1) where sum cn >= min_color (>= 1), DBL_MAX elsewhere."""
    S = np.asarray(csums, np.int64).sum(axis=1)
    n = np.asarray(ccounts, np.int64).sum(axis=1)
    ok = (n >= min_color) & (n > 0)
    Ec = np.full(len(S), DBL_MAX)
    Ec[ok] = S[ok].astype(np.float64) / (n[ok].astype(np.float64) * 100.0 * 1.1)
    return Ec, n.astype(np.int32)


def np_color_charge(Ec, miss, tau):
    return np.where(Ec != DBL_MAX, np.where(Ec != DBL_MAX, Ec, 0.0) / tau, miss / tau)


def np_color_fold(L, E, n, tau, min_projections, charge):
    """(L - E / tau) - charge for the valid particles (by the WHITE counts), -inf for the others."""
    valid = (E != DBL_MAX) & (n >= min_projections)
    return np.where(valid, (L - np.where(valid, E, 0.0) / tau) - charge, -np.inf)


# ------------------------------------------------------------------ the calls
def window(img, u, v):
    img = np.ascontiguousarray(img, np.uint8)
    return _hc().hc_mcl_color_window(img.ctypes.data, img.shape[1], img.shape[0], float(u), float(v))


def color_sums(c2w, green, K, D, img):
    c2w = np.ascontiguousarray(c2w, np.float64).reshape(-1, 12)
    green = np.ascontiguousarray(green, np.float64).reshape(-1, 3)
    K, D = np.ascontiguousarray(K, np.float64).reshape(9), np.ascontiguousarray(D, np.float64).reshape(4)
    img = np.ascontiguousarray(img, np.uint8)
    s, n = np.zeros(len(c2w), np.int64), np.zeros(len(c2w), np.int32)
    _hc().hc_mcl_color_sums(c2w.ctypes.data, len(c2w), green.ctypes.data, len(green), K.ctypes.data, D.ctypes.data,
                            img.ctypes.data, img.shape[1], img.shape[0], s.ctypes.data, n.ctypes.data)
    return s, n


def color_charge(csums, ccounts, min_color, miss, tau):
    csums, ccounts = np.ascontiguousarray(csums, np.int64), np.ascontiguousarray(ccounts, np.int32)
    N, Cn = csums.shape
    Ec, n, ch = np.zeros(N), np.zeros(N, np.int32), np.zeros(N)
    _hc().hc_mcl_color_charge(csums.ctypes.data, ccounts.ctypes.data, N, Cn, min_color, miss, tau, Ec.ctypes.data,
                              n.ctypes.data, ch.ctypes.data)
    return Ec, n, ch


def color_fold(L, E, n, charge, tau, min_projections=10):
    L, E = np.ascontiguousarray(L, np.float64), np.ascontiguousarray(E, np.float64)
    n, charge = np.ascontiguousarray(n, np.int32), np.ascontiguousarray(charge, np.float64)
    out = np.zeros(len(L))
    _hc().hc_mcl_color_fold(L.ctypes.data, E.ctypes.data, n.ctypes.data, charge.ctypes.data, len(L), tau,
                            min_projections, out.ctypes.data)
    return out


# ------------------------------------------------------------------ the tests
def test_default_params_struct_size_and_null_arguments():
    import mantis_amd as M

    L = M.lib()
    p = M.MantisMclColorParams()
    L.mantis_default_mcl_color_params(C.byref(p))
    assert p.struct_size == C.sizeof(M.MantisMclColorParams) == 32
    assert p.enable == 0 and p.min_color_projections == 10 and p.pad == 0
    assert p.color_tau > 0 and math.isfinite(p.color_tau) and p.color_miss >= 0 and math.isfinite(p.color_miss)
    a = C.c_int32()
    L.mantis_mcl_color_sizes(C.byref(a))
    assert a.value == C.sizeof(M.MantisMclColorParams)
    L.mantis_mcl_color_sizes(None)
    L.mantis_default_mcl_color_params(None)
    # a null context is an argument error, not a crash
    assert L.mantis_mcl_set_color(None, C.byref(p)) == 1
    assert L.mantis_mcl_get_color_record(None, None, None, None, None, None, None) == 1
    assert L.mantis_mcl_modes_color(None, None, None) == 1


def test_window_sums_over_every_edge():
    """Random small buffers; windows hanging over the left, right, top and
    bottom edges (a column past the row's end is the next row's first pixel),
    over the buffer's start and its end, and rounding ties at k + 1/2."""
    rng = np.random.default_rng(5)
    seen = set()
    for Ww, Hh in [(23, 17), (10, 10), (7, 31), (3, 3)]:
        img = rng.integers(0, 256, (Hh, Ww, 3), dtype=np.uint8)
        pts = [(0.0, 0.3), (4.9, 4.9), (Ww - 0.01, Hh - 0.01), (Ww - 5.2, Hh - 5.2), (Ww - 4.5, Hh - 4.5),
               (0.5, 1.5), (2.5, 3.5), (-7.3, -6.1), (Ww + 6.6, Hh + 7.7), (Ww / 2.0, -20.0), (Ww / 2.0, Hh + 20.0),
               (Ww - 1.0, Hh - 1.0), (0.0, 0.0)]
        pts += [(rng.uniform(-8, Ww + 8), rng.uniform(-8, Hh + 8)) for _ in range(40)]
        for u, v in pts:
            assert window(img, u, v) == np_window(img, u, v), (Ww, Hh, u, v)
            lo = int(np.rint(v - 5.0)) * Ww + int(np.rint(u - 5.0))
            hi = int(np.rint(v + 4.0)) * Ww + int(np.rint(u + 4.0))
            seen |= {"start"} if lo < 0 <= hi else set()
            seen |= {"end"} if lo < Ww * Hh <= hi else set()
            seen |= {"inside"} if lo >= 0 and hi < Ww * Hh else set()
            seen |= {"outside"} if hi < 0 or lo >= Ww * Hh else set()
    assert seen == {"start", "end", "inside", "outside"}
    # an all-GREEN buffer costs nothing inside and 100 |GREEN|^2 where the whole window is outside
    g = np.zeros((20, 20, 3), np.uint8)
    g[:] = GREEN
    assert window(g, 10.0, 10.0) == 0 and window(g, 10.0, -30.0) == 100 * (50 * 50 + 255 * 255 + 85 * 85)
    assert window(np.zeros((20, 20, 3), np.uint8), 9.0, 9.0) == window(g, 10.0, 40.0)
    # the largest window sum (100 x 135950, under the bound 100 x 3 x 255^2) fits the int32 accumulator
    w = np.zeros((12, 12, 3), np.uint8)
    w[:] = (255, 0, 255)
    assert window(w, 6.0, 6.0) == 100 * (205 * 205 + 255 * 255 + 170 * 170) == 100 * 135950


def test_color_sums_against_the_oracle():
    """(csum, cn) of poses over a green row on a random 96 x 64 frame: counts equal the oracle's, sums its
    COLOR error times n x 1.1 x 100 (the oracle divides each window by 100 in double: recovered by rint)."""
    from mantis_amd import synth

    rng = np.random.default_rng(8)
    Ww, Hh = 96, 64
    D = synth.intrinsics(Ww, Hh)[1]
    K = np.array([[60.0, 0, 48.0], [0, 60.0, 32.0], [0, 0, 1.0]])  # narrow enough that part of the row is out of frame
    img = rng.integers(0, 256, (Hh, Ww, 3), dtype=np.uint8)
    green = np.stack([np.linspace(-1.2, 1.2, 41), np.full(41, 0.6), np.zeros(41)], axis=1)
    white = np.array([[0.0, 0.0, 0.0]])
    orc = O.Oracle(white, white, green)
    c2w = []
    for i in range(60):
        R, pos = synth.random_pose(rng)
        if i % 5 == 4:
            pos = pos + np.array([0.0, 0.0, -3.0])  # under the floor: nothing in front of the camera
        c2w.append(synth.truth_c2w(R, pos))
    c2w = np.array(c2w)
    s, n = color_sums(c2w, green, K, D, img)
    err, npj = orc.score(img, K, D, c2w, fast=False)
    assert np.array_equal(n, npj) and (n == 0).any() and (n >= 10).any() and ((n > 0) & (n < 41)).any()
    x = np.where(npj > 0, err, 0.0) * npj * 1.1 * 100.0
    assert np.abs(x - np.rint(x)).max() < 1e-3
    assert np.array_equal(s, np.rint(x).astype(np.int64))
    assert np.all(s[n == 0] == 0)
    # no green landmarks at all
    s0, n0 = color_sums(c2w, np.zeros((0, 3)), K, D, img)
    assert np.all(s0 == 0) and np.all(n0 == 0)


def test_pooling_and_the_two_charges():
    rng = np.random.default_rng(13)
    N, Cn = 300, 4
    cn = rng.integers(0, 38, (N, Cn)).astype(np.int32)
    cn[rng.random((N, Cn)) < 0.5] = 0
    cs = cn.astype(np.int64) * rng.integers(0, 100 * 195075 + 1, (N, Cn))
    cs[0], cn[0] = 37 * 100 * 195075, 37  # the largest sums
    cn[1] = 0
    cs[1] = 0
    for min_color in (1, 10, 60):
        Ec, n, ch = color_charge(cs, cn, min_color, 9000.0, 2500.0)
        Er, nr = np_color_pool(cs, cn, min_color)
        assert np.array_equal(n, nr) and np.array_equal(Ec, Er)
        assert np.array_equal(ch, np_color_charge(Er, 9000.0, 2500.0))
        defined = Ec != DBL_MAX
        assert defined.any() and (~defined).any(), "both branches of the charge"
        assert np.array_equal(defined, n >= min_color)
        assert np.all(ch[~defined] == 9000.0 / 2500.0) and np.all(ch[defined] == Ec[defined] / 2500.0)
    assert color_charge(cs[:1], cn[:1], 1, 0.0, 1.0)[0][0] == 37 * 100 * 195075 * 4 / (37 * 4 * 100.0 * 1.1)
    # color_miss = 0 is legal: a blind particle then pays nothing
    assert color_charge(cs[1:2], cn[1:2], 1, 0.0, 7.0)[2][0] == 0.0


def test_fold_operation_order():
    """L <- (L - E / tau) - charge: the two roundings in that order, validity by the WHITE counts alone."""
    rng = np.random.default_rng(21)
    N = 4096
    L = -rng.uniform(0, 50, N)
    E = rng.uniform(5000, 150000, N)
    n = rng.integers(0, 40, N).astype(np.int32)
    E[::17] = DBL_MAX
    charge = rng.uniform(0, 9, N)
    tau = 63478.0
    got = color_fold(L, E, n, charge, tau)
    ref = np_color_fold(L, E, n, tau, 10, charge)
    assert np.array_equal(got, ref)
    valid = (E != DBL_MAX) & (n >= 10)
    assert np.all(np.isneginf(got[~valid])) and np.all(np.isfinite(got[valid])) and valid.any() and (~valid).any()
    other = L - (np.where(valid, E, 0.0) / tau + charge)
    assert np.any(got[valid] != other[valid]), "the order of the two subtractions is observable"
    # a zero charge is the step without colour, bit for bit
    import test_mcl_host as MH

    Lw, _, _ = MH.weights(L, E, n, tau)
    assert np.array_equal(color_fold(L, E, n, np.zeros(N), tau), Lw)
