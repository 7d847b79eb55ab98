"""Window smoothing, test side: ctypes bindings of the host build's hc_smooth_*
(mantis_amd/csrc/mk_smooth.h through build/libmantis_hostcheck.so), a numpy
restatement of the factors and of the dense normal system, and the synthetic
trajectories the CPU and GPU tests share.
"""
import ctypes as C
import math

import numpy as np

import _hostcheck as H
import _refine_ref as RR
from mantis_amd import synth

W, H_ = RR.W, RR.H_
STATUS = {"ok": 0, "starved": 1, "singular": 2}


def hc():
    import mantis_amd as M

    L = H.lib()
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    L.hc_smooth_motion.argtypes = [vp, vp, vp]
    L.hc_smooth_motion.restype = ci
    L.hc_smooth_log.argtypes = [vp, vp]
    L.hc_smooth_jr_inv.argtypes = [vp, vp]
    L.hc_smooth_between.argtypes = [vp, vp, vp, cd, cd, vp, vp, vp]
    L.hc_smooth_between.restype = None
    L.hc_smooth_prior.argtypes = [vp, vp, vp, cd, vp, vp]
    L.hc_smooth_prior.restype = ci
    L.hc_smooth_assemble.argtypes = [ci, vp, vp, vp, vp, ci, vp, vp, cd, vp, vp, vp]
    L.hc_smooth_assemble.restype = None
    L.hc_smooth_solve.argtypes = [ci, vp, vp, vp, vp, vp, vp, vp]
    L.hc_smooth_solve.restype = ci
    L.hc_smooth_marginals.argtypes = [ci, vp, vp, vp, vp]
    L.hc_smooth_marginals.restype = ci
    L.hc_smooth_sums.argtypes = [ci, vp, vp, vp, vp, ci, vp, cd, vp, vp]
    L.hc_smooth_sums.restype = None
    L.hc_smooth_conclude.argtypes = [ci, vp, vp, vp, ci, cd, C.POINTER(M.MantisSmoothResult), vp]
    L.hc_smooth_conclude.restype = None
    L.hc_smooth_seq.argtypes = [ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, ci, ci, ci,
                                C.POINTER(M.MantisSmoothParams), C.POINTER(M.MantisSmoothResult), vp] + [vp] * 8
    L.hc_smooth_seq.restype = ci
    for f in ("hc_sizeof_smooth_params", "hc_sizeof_smooth_result", "hc_sizeof_smooth_view"):
        getattr(L, f).restype = ci
    return L


def default_params(**kw):
    import mantis_amd as M

    p = M.MantisSmoothParams()
    M.lib().mantis_default_smooth_params(C.byref(p))
    for k, v in kw.items():
        assert k in dict(M.MantisSmoothParams._fields_), k
        setattr(p, k, v)
    return p


def _a(x, dt=np.float64):
    return np.ascontiguousarray(x, dt)


def _p(a):
    return None if a is None or a.size == 0 else a.ctypes.data


# ---- motions ----
def quat_of(R):
    """xyzw of a rotation matrix with a positive trace (the small steps of the tests)."""
    w = math.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2]) / 2.0
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def motion_of(Dm):
    """delta_pos | delta_quat_xyzw (7) of a 4 x 4 step."""
    return np.concatenate([Dm[:3, 3], quat_of(Dm[:3, :3])])


UNSET = np.zeros(7)  # |q|^2 < 0.5: no factor


def transform(motion):
    """The library's own Transform of a motion (hc_smooth_motion): (has, D [4, 4])."""
    m = _a(motion).reshape(7)
    D = np.zeros((4, 4))
    has = hc().hc_smooth_motion(m[:3].copy().ctypes.data, m[3:].copy().ctypes.data, D.ctypes.data)
    return bool(has), D


def step(dx=0.08, yaw_deg=3.0, dy=0.0, dz=0.0, roll_deg=0.0):
    """The 8 cm / 3 degree step of the issue's scene, in the base frame."""
    D = np.eye(4)
    D[:3, :3] = synth.rot_z(math.radians(yaw_deg)) @ synth.rot_x(math.radians(roll_deg))
    D[:3, 3] = [dx, dy, dz]
    return D


# ---- the factors ----
def log_so3(R):
    phi = np.zeros(3)
    hc().hc_smooth_log(_a(R).ctypes.data, phi.ctypes.data)
    return phi


def jr_inv(phi):
    J = np.zeros((3, 3))
    hc().hc_smooth_jr_inv(_a(phi).ctypes.data, J.ctypes.data)
    return J


def between(Tk, Tk1, D, wt=1.0, wr=1.0):
    """hc_smooth_between: (e [6], Ja [6, 6], Jb [6, 6]), whitened by wt / wr."""
    e, Ja, Jb = np.zeros(6), np.zeros((6, 6)), np.zeros((6, 6))
    hc().hc_smooth_between(_a(Tk).ctypes.data, _a(Tk1).ctypes.data, _a(D).ctypes.data, wt, wr, e.ctypes.data,
                           Ja.ctypes.data, Jb.ctypes.data)
    return e, Ja, Jb


def prior(T0, Tp, cov, sigma_row=1.0):
    """hc_smooth_prior: (ok, e [6], J [6, 6]) whitened by sigma_row L_c^-1."""
    e, J = np.zeros(6), np.zeros((6, 6))
    ok = hc().hc_smooth_prior(_a(T0).ctypes.data, _a(Tp).ctypes.data, _a(cov).ctypes.data, sigma_row, e.ctypes.data,
                              J.ctypes.data)
    return bool(ok), e, J


def np_exp(phi):
    th = np.linalg.norm(phi)
    K = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * K @ K


def np_log(R):
    """Rotation vector by numpy, independent of the library's atan2 form (angles well inside (0, pi))."""
    c = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(v)
    if s < 1e-7:
        return v  # first order: the central differences of the tests stay far above this
    return math.atan2(s, c) / s * v


def np_between(Tk, Tk1, D):
    E = np.linalg.inv(D) @ np.linalg.inv(Tk) @ Tk1
    return np.concatenate([E[:3, 3], np_log(E[:3, :3])])


def np_prior(T0, Tp):
    return np.concatenate([T0[:3, 3] - Tp[:3, 3], np_log(Tp[:3, :3].T @ T0[:3, :3])])


def central(f, h=1e-6):
    """d f(x) / dx at x = 0 over six right-perturbation coordinates, by central differences."""
    cols = []
    for i in range(6):
        d = np.zeros(6)
        d[i] = h
        cols.append((f(d) - f(-d)) / (2 * h))
    return np.array(cols).T


# ---- the system ----
def assemble(acc, has, fe, fJ, lam=0.0, pe=None, pJ=None):
    """hc_smooth_assemble: (Hd [N, 6, 6], Ho [N, 6, 6], g [N, 6])."""
    acc = _a(acc).reshape(-1, 28)
    N = len(acc)
    has = _a(has, np.int32)
    fe, fJ = _a(fe).reshape(-1), _a(fJ).reshape(-1)
    Hd, Ho, g = np.zeros((N, 6, 6)), np.zeros((N, 6, 6)), np.zeros((N, 6))
    hp = pe is not None
    pe_ = _a(pe if hp else np.zeros(6))
    pJ_ = _a(pJ if hp else np.zeros(36))
    hc().hc_smooth_assemble(N, acc.ctypes.data, _p(has), _p(fe), _p(fJ), int(hp), pe_.ctypes.data, pJ_.ctypes.data, lam,
                            Hd.ctypes.data, Ho.ctypes.data, g.ctypes.data)
    return Hd, Ho, g


def solve(Hd, Ho, g, has):
    """hc_smooth_solve: (bad, x [N, 6]); bad = -1 or the first view whose block is not PD."""
    Hd, Ho, g = _a(Hd), _a(Ho), _a(g)
    N = len(Hd)
    has = _a(has, np.int32)
    x, Ld, Lo = np.zeros((N, 6)), np.zeros((N, 36)), np.zeros((N, 36))
    bad = hc().hc_smooth_solve(N, Hd.ctypes.data, Ho.ctypes.data, g.ctypes.data, _p(has), x.ctypes.data, Ld.ctypes.data,
                               Lo.ctypes.data)
    return bad, x


def marginals(Hd, Ho, has):
    Hd, Ho = _a(Hd), _a(Ho)
    N = len(Hd)
    has = _a(has, np.int32)
    S = np.zeros((N, 6, 6))
    bad = hc().hc_smooth_marginals(N, Hd.ctypes.data, Ho.ctypes.data, _p(has), S.ctypes.data)
    return bad, S


def sums(n_obs, acc, has, fe, sigma_row, pe=None):
    """hc_smooth_sums: (n_obs, n_factors, rms, motion_rms, cost) of a pass."""
    acc = _a(acc).reshape(-1, 28)
    N = len(acc)
    n_obs, has, fe = _a(n_obs, np.int32), _a(has, np.int32), _a(fe).reshape(-1)
    out, cnt = np.zeros(3), np.zeros(2, np.int32)
    pe_ = _a(pe if pe is not None else np.zeros(6))
    hc().hc_smooth_sums(N, n_obs.ctypes.data, acc.ctypes.data, _p(has), _p(fe), int(pe is not None), pe_.ctypes.data,
                        sigma_row, out.ctypes.data, cnt.ctypes.data)
    return int(cnt[0]), int(cnt[1]), out[0], out[1], out[2]


def conclude(Hd, Ho, has, min_obs, max_rms, res, poses):
    """hc_smooth_conclude on a copy of `res` (status, iterations_run and the passes' figures filled) with the
    final pass's blocks at lambda = 0 and the views' final poses: (result, covariances [N, 6, 6])."""
    import mantis_amd as M

    Hd, Ho = _a(Hd), _a(Ho)
    N = len(Hd)
    has = _a(has, np.int32)
    r = M.MantisSmoothResult.from_buffer_copy(bytes(res))
    vw = (M.MantisSmoothView * N)()
    for k in range(N):
        vw[k].T_w_b[:] = list(np.asarray(poses[k], np.float64).reshape(16))
    hc().hc_smooth_conclude(N, Hd.ctypes.data, Ho.ctypes.data, _p(has), min_obs, max_rms, C.byref(r),
                            C.cast(vw, C.c_void_p))
    return r, np.array([np.array(v.covariance).reshape(6, 6) for v in vw])


def dense(Hd, Ho, g=None):
    """The dense normal matrix (6 N x 6 N) of the blocks, and g stacked."""
    N = len(Hd)
    Hm = np.zeros((6 * N, 6 * N))
    for k in range(N):
        Hm[6 * k:6 * k + 6, 6 * k:6 * k + 6] = Hd[k]
        if k < N - 1:
            Hm[6 * k + 6:6 * k + 12, 6 * k:6 * k + 6] = Ho[k]
            Hm[6 * k:6 * k + 6, 6 * k + 6:6 * k + 12] = np.asarray(Ho[k]).T
    return Hm, (None if g is None else np.asarray(g).reshape(-1))


def sym28(acc):
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = acc[:21]
    return A + np.triu(A, 1).T


def np_system(acc, has, fe, fJ, lam=0.0, pe=None, pJ=None):
    """The dense normal system from stacked Jacobians, independent of the block assembly."""
    acc = np.asarray(acc).reshape(-1, 28)
    N = len(acc)
    Hm, g = np.zeros((6 * N, 6 * N)), np.zeros(6 * N)
    for k in range(N):
        Hm[6 * k:6 * k + 6, 6 * k:6 * k + 6] += sym28(acc[k]) + lam * np.eye(6)
        g[6 * k:6 * k + 6] += acc[k][21:27]
    for k in range(N - 1):
        if not has[k]:
            continue
        J = np.zeros((6, 6 * N))
        J[:, 6 * k:6 * k + 6] = np.asarray(fJ[k]).reshape(2, 6, 6)[0]
        J[:, 6 * k + 6:6 * k + 12] = np.asarray(fJ[k]).reshape(2, 6, 6)[1]
        Hm += J.T @ J
        g += J.T @ np.asarray(fe[k])
    if pe is not None:
        Hm[:6, :6] += np.asarray(pJ).T @ np.asarray(pJ)
        g[:6] += np.asarray(pJ).T @ np.asarray(pe)
    return Hm, g


def solve_bound(Hm, x):
    """The bound of the linear-algebra comparisons: the larger of 1e-10 of the norm and 1e3 eps cond2(H) |x|."""
    nx = float(np.linalg.norm(x))
    return max(1e-10 * nx, 1e3 * 2.0 ** -53 * np.linalg.cond(Hm) * nx)


# ---- the whole call on the host ----
class Seq:
    pass


def seq(T_in, motions, exts, frames, X, nw, nr, ng, p, prior_T=None, prior_cov=None, K=None, D=None):
    """hc_smooth_seq on one window: frames[k][c]. Returns an object with .res (MantisSmoothResult), .views
    [N] (MantisSmoothView) and the per-pass records .T [P, N, 4, 4], .acc [P, N, 28], .n [P, N], .e [P, N - 1, 6],
    .J [P, N - 1, 2, 6, 6], .pe [P, 6], .pJ [P, 6, 6], .delta [P, N, 6] (P = passes taken)."""
    import mantis_amd as M

    N, Cn = len(frames), len(frames[0])
    h, w = frames[0][0].shape[:2]
    if K is None:
        K, D = synth.intrinsics(w, h)
    T = _a(T_in).reshape(N, 16)
    mo = _a(motions if motions is not None else np.zeros((0, 7))).reshape(-1, 7)
    assert len(mo) == N - 1
    E = _a(np.array(exts, np.float64).reshape(Cn, 16))
    Ks, Ds = RR.per_camera(K, D, Cn)
    keep = [_a(f, np.uint8) for fr in frames for f in fr]
    ptrs = (C.c_void_p * (N * Cn))(*[k.ctypes.data for k in keep])
    P = 11
    o = Seq()
    o.res = M.MantisSmoothResult()
    vw = (M.MantisSmoothView * N)()
    o.T, o.acc, o.n = np.zeros((P, N, 4, 4)), np.zeros((P, N, 28)), np.zeros((P, N), np.int32)
    o.e, o.J = np.zeros((P, max(N - 1, 0), 6)), np.zeros((P, max(N - 1, 0), 2, 6, 6))
    o.pe, o.pJ, o.delta = np.zeros((P, 6)), np.zeros((P, 6, 6)), np.zeros((P, N, 6))
    pT = None if prior_T is None else _a(prior_T).reshape(16)
    pC = None if prior_cov is None else _a(prior_cov).reshape(36)
    # the records are written pass-major with the call's own N, so the arrays above are handed over as flat buffers
    o.ok = bool(hc().hc_smooth_seq(N, T.ctypes.data, _p(mo), _p(pT), _p(pC), E.ctypes.data, Ks.ctypes.data,
                                   Ds.ctypes.data, ptrs, Cn, w, h, X.ctypes.data, nw, nr, ng, C.byref(p),
                                   C.byref(o.res), C.cast(vw, C.c_void_p), o.T.ctypes.data, o.acc.ctypes.data,
                                   o.n.ctypes.data, _p(o.e), _p(o.J), o.pe.ctypes.data, o.pJ.ctypes.data,
                                   o.delta.ctypes.data))
    o.views = list(vw)
    o._keep = vw
    o.poses = np.array([np.array(v.T_w_b).reshape(4, 4) for v in vw])
    return o


# ---- scenes ----
def start_pose(x=-0.20, y=-0.12, h=1.4, yaw=0.3):
    T = np.eye(4)
    T[:3, :3] = synth.rot_z(yaw) @ synth.rot_x(math.radians(2.0)) @ synth.rot_y(math.radians(-1.5))
    T[:3, 3] = [x, y, h]
    return T


_scenes = {}


def trajectory(n_views, n_cams=4, w=W, h=H_, cfg=17, steps=None, blind=(), T0=None):
    """A window: n_views base poses chained by `steps` (default: the 8 cm / 3 degree step), each rendered
    through the ring synth.rig_extrinsics(n_cams); the views in `blind` are black. Cached.
    {"ext", "Twb" [k], "frames" [k][c], "steps" [k] (4 x 4), "motions" [k] (7)}."""
    key = (n_views, n_cams, w, h, cfg, tuple(blind), None if steps is None else len(steps), T0 is None)
    if key in _scenes and steps is None and T0 is None:
        return _scenes[key]
    ext = synth.rig_extrinsics(n_cams)
    steps = [step()] * (n_views - 1) if steps is None else list(steps)
    Twb = [start_pose() if T0 is None else np.array(T0, np.float64)]
    for D in steps:
        Twb.append(Twb[-1] @ D)
    frames = []
    for k, T in enumerate(Twb):
        fr = []
        for c in range(n_cams):
            if k in blind:
                fr.append(np.zeros((h, w, 3), np.uint8))
                continue
            Twc = T @ ext[c]
            fr.append(synth.render_host(synth.make_cam(Twc[:3, :3], Twc[:3, 3], w, h), synth.frame_seed(cfg, 100 * k + c)))
        frames.append(fr)
    sc = {"ext": ext, "Twb": Twb, "frames": frames, "steps": steps, "motions": np.array([motion_of(D) for D in steps])}
    _scenes[key] = sc
    return sc


def exact_motions(sc):
    """Motions whose library Transform chains the scene's poses: the steps themselves (their quaternion's
    rounding, ~1e-16, is far below every tolerance)."""
    return sc["motions"].reshape(-1, 7).copy()


def noisy_motions(sc, sigma_t=0.01, sigma_rot=0.03, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for D in sc["steps"]:
        N = np.eye(4)
        N[:3, :3] = np_exp(rng.normal(0, sigma_rot, 3))
        N[:3, 3] = rng.normal(0, sigma_t, 3)
        out.append(motion_of(D @ N))
    return np.array(out).reshape(-1, 7)


def starts(sc):
    return np.array([RR.shift(T) for T in sc["Twb"]])
