"""The fixed-lag window, test side: ctypes bindings of the host build's hc_lag_*
(mantis_amd/csrc/mk_smooth.h through build/libmantis_hostcheck.so) and the
scenes the CPU and GPU tests share.
"""
import ctypes as C

import numpy as np

import _hostcheck as H
import _refine_ref as RR
import _smooth_ref as SR
from mantis_amd import synth

SW, SH = 322, 242
DROPS = {"kept": 0, "no_factor": 1, "not_ok": 2, "h00": 3, "lambda": 4, "cov": 5}


def hc():
    import mantis_amd as M

    L = SR.hc()
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    L.hc_lag_marginalize.argtypes = [vp] * 6 + [cd] + [vp] * 3
    L.hc_lag_marginalize.restype = ci
    L.hc_lag_marginal.argtypes = [vp] * 6 + [cd] + [vp] * 2
    L.hc_lag_marginal.restype = ci
    L.hc_lag_schur.argtypes = [vp] * 7
    L.hc_lag_schur.restype = ci
    L.hc_lag_whitener.argtypes = [vp, cd, vp]
    L.hc_lag_whitener.restype = ci
    L.hc_lag_predict.argtypes = [vp, vp, vp]
    L.hc_lag_predict.restype = None
    L.hc_lag_seq.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, ci, ci, ci,
                             C.POINTER(M.MantisSmoothParams), vp, vp, vp, vp]
    L.hc_lag_seq.restype = ci
    for f in ("hc_sizeof_lag_params", "hc_sizeof_lag_info"):
        getattr(L, f).restype = ci
    return L


_a = SR._a


def schur(H00, g0, Ja, Jb, e):
    """hc_lag_schur: (reason, Lambda [6, 6], eta [6])."""
    Lam, eta = np.zeros((6, 6)), np.zeros(6)
    why = hc().hc_lag_schur(_a(H00).ctypes.data, _a(g0).ctypes.data, _a(Ja).ctypes.data, _a(Jb).ctypes.data,
                            _a(e).ctypes.data, Lam.ctypes.data, eta.ctypes.data)
    return why, Lam, eta


def marginalize(H00, g0, Ja, Jb, e, T1, sigma_row):
    """hc_lag_marginalize: (reason, T_p [4, 4], Cov_p [6, 6], W_p [6, 6])."""
    Tp, Cov, Wp = np.zeros((4, 4)), np.zeros((6, 6)), np.zeros((6, 6))
    why = hc().hc_lag_marginalize(_a(H00).ctypes.data, _a(g0).ctypes.data, _a(Ja).ctypes.data, _a(Jb).ctypes.data,
                                  _a(e).ctypes.data, _a(T1).ctypes.data, sigma_row, Tp.ctypes.data, Cov.ctypes.data,
                                  Wp.ctypes.data)
    return why, Tp, Cov, Wp


def whitener(cov, sigma_row):
    Wp = np.zeros((6, 6))
    ok = hc().hc_lag_whitener(_a(cov).ctypes.data, sigma_row, Wp.ctypes.data)
    return bool(ok), Wp


def predict(T_newest, D):
    T = np.zeros((4, 4))
    hc().hc_lag_predict(_a(T_newest).ctypes.data, _a(D).ctypes.data, T.ctypes.data)
    return T


class Seq:
    pass


def seq(cap, frames, starts, motions, exts, X, nw, nr, ng, p, prior_T=None, prior_cov=None):
    """hc_lag_seq: frames[push][c], starts[push] (4 x 4 or None), motions[push] (7; row 0 unused). Returns an
    object with .res [push] (MantisSmoothResult), .views [push][held] (MantisSmoothView), .info [push, 4] = views
    held, has_prior, drop_reason, slid, .prior_T [push, 4, 4], .prior_cov [push, 6, 6]."""
    import mantis_amd as M

    n, Cn = len(frames), len(frames[0])
    h, w = frames[0][0].shape[:2]
    K, D = synth.intrinsics(w, h)
    T = np.zeros((n, 16))
    hs = np.zeros(n, np.int32)
    for q, s in enumerate(starts):
        if s is not None:
            T[q] = np.asarray(s, np.float64).reshape(16)
            hs[q] = 1
    mo = _a(motions).reshape(n, 7)
    E = _a(np.array(exts, np.float64).reshape(Cn, 16))
    Ks, Ds = RR.per_camera(K, D, Cn)
    keep = [_a(f, np.uint8) for fr in frames for f in fr]
    ptrs = (C.c_void_p * (n * Cn))(*[k.ctypes.data for k in keep])
    o = Seq()
    res = (M.MantisSmoothResult * n)()
    vw = (M.MantisSmoothView * (n * cap))()
    o.info = np.zeros((n, 4), np.int32)
    pr = np.zeros((n, 52))
    pT = None if prior_T is None else _a(prior_T).reshape(16)
    pC = None if prior_cov is None else _a(prior_cov).reshape(36)
    o.ok = bool(hc().hc_lag_seq(n, cap, T.ctypes.data, hs.ctypes.data, mo.ctypes.data, SR._p(pT), SR._p(pC),
                                E.ctypes.data, Ks.ctypes.data, Ds.ctypes.data, ptrs, Cn, w, h, X.ctypes.data, nw, nr, ng,
                                C.byref(p), C.cast(res, C.c_void_p), C.cast(vw, C.c_void_p), o.info.ctypes.data,
                                pr.ctypes.data))
    o.res = list(res)
    o.views = [[vw[q * cap + k] for k in range(o.info[q, 0])] for q in range(n)]
    o._keep = (res, vw)
    o.prior_T = pr[:, :16].reshape(n, 4, 4)
    o.prior_cov = pr[:, 16:].reshape(n, 6, 6)
    return o


def pose_of(view):
    return np.array(view.T_w_b).reshape(4, 4)


def pose_dist(A, B):
    """Distance of two base poses: translation (map units) + rotation angle (rad)."""
    dR = A[:3, :3].T @ B[:3, :3]
    return float(np.linalg.norm(A[:3, 3] - B[:3, 3]) + np.linalg.norm(SR.np_log(dR)))


# ---- the accuracy scene: twelve one-camera views, capacity 4, views 5 and 6 black ----
ACC_VIEWS, ACC_CAP, ACC_BLIND = 12, 4, (5, 6)
ACC_ITERATIONS = 2
_acc = {}


def accuracy_scene():
    if "sc" not in _acc:
        _acc["sc"] = SR.trajectory(ACC_VIEWS, n_cams=1, w=SW, h=SH, cfg=23, blind=ACC_BLIND)
    return _acc["sc"]


def accuracy_motions(sc, noisy):
    """[push][7], row 0 unused: the steps themselves, or the steps off by the default sigmas (fixed seed)."""
    mo = SR.noisy_motions(sc, 0.01, 0.03, seed=7) if noisy else SR.exact_motions(sc)
    return np.concatenate([np.zeros((1, 7)), mo])


def accuracy_starts(sc):
    """Only the first view starts at a given pose (off by RR.shift); the rest are predicted."""
    return [RR.shift(sc["Twb"][0])] + [None] * (ACC_VIEWS - 1)


def accuracy_compare(sc, mo, pushes, batch):
    """The newest view of every push after the first slide against two batch calls on the same frames: (H) the
    whole history; (T) the last ACC_CAP views with no prior. All three solvers start every view they share from
    the same pose: the one the lag window held for it before the push (for a view that has left, the pose it left
    with), and the new view from the start the push used. With I iterations each, a reference started anywhere
    else (the views' first starts, say) differs from the lag window by what I iterations leave unconverged, not
    by what it knows, and that is orders above the difference this comparison is after. pushes: [(result, views)]
    of the lag sequence; batch(T_in, motions, frames, n_views) -> poses [n, 4, 4] of one window. Returns {push:
    (d(lag, H), d(T, H), d(lag, T), window begins black)}."""
    out, best = {}, {}
    for q in range(ACC_VIEWS):
        lo = max(0, q - ACC_CAP + 1)
        if q >= ACC_CAP:
            start = predict(best[q - 1], SR.transform(mo[q])[1])  # what the push formed on the device
            Hp = batch(np.array([best[k] for k in range(q)] + [start]), mo[1:q + 1], sc["frames"][:q + 1], q + 1)
            Tp = batch(np.array([best[k] for k in range(lo, q)] + [start]), mo[lo + 1:q + 1], sc["frames"][lo:q + 1],
                       ACC_CAP)
            a = pose_of(pushes[q][1][-1])
            out[q] = (pose_dist(a, Hp[-1]), pose_dist(Tp[-1], Hp[-1]), pose_dist(a, Tp[-1]), lo in ACC_BLIND)
        for k, v in zip(range(lo, q + 1), pushes[q][1]):
            best[k] = pose_of(v)
    return out


def accuracy_host(sc, mo, X, nw, nr, ng):
    """The accuracy scene on the host: (lag sequence, accuracy_compare's table)."""
    p = SR.default_params(iterations=ACC_ITERATIONS)
    lag = seq(ACC_CAP, sc["frames"], accuracy_starts(sc), mo, sc["ext"], X, nw, nr, ng, p)

    def batch(T_in, motions, frames, n):
        return SR.seq(T_in, motions, sc["ext"], frames, X, nw, nr, ng, p).poses

    return lag, accuracy_compare(sc, mo, list(zip(lag.res, lag.views)), batch)
