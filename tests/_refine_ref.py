"""Line refinement, test side: ctypes bindings of the host build's hc_refine_*
(mantis_amd/csrc/mk_refine.h through build/libmantis_hostcheck.so), a numpy /
pure-Python restatement of the rules of include/mantis.h, and the synthetic
rigs the CPU and GPU tests share.
"""
import ctypes as C
import math

import numpy as np

import _hostcheck as H
from mantis_amd import synth

W, H_ = 1280, 720
TARGETS = {"w": (255, 255, 255), "r": (50, 85, 255), "g": (50, 255, 85)}


def hc():
    import mantis_amd as M

    L = H.lib()
    vp = C.c_void_p
    L.hc_refine_flags.argtypes = [vp, C.c_int, C.c_double, vp]
    L.hc_refine_flags.restype = None
    L.hc_refine_obs.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int,
                                C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.hc_refine_obs.restype = C.c_int
    L.hc_refine_accumulate.argtypes = [vp, C.c_int, vp]
    L.hc_refine_accumulate.restype = None
    L.hc_refine_seq.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                C.POINTER(M.MantisRefineParams), C.POINTER(M.MantisRefineResult)]
    L.hc_refine_seq.restype = None
    L.hc_gn_solve6.argtypes = [vp, C.c_double, vp, vp]
    L.hc_gn_solve6.restype = C.c_int
    L.hc_refine_conclude.argtypes = [vp, C.c_int, C.c_double, C.POINTER(M.MantisRefineResult)]
    L.hc_refine_conclude.restype = None
    return L


def default_params(**kw):
    import mantis_amd as M

    p = M.MantisRefineParams()
    M.lib().mantis_default_refine_params(C.byref(p))
    for k, v in kw.items():
        assert k in dict(M.MantisRefineParams._fields_), k
        setattr(p, k, v)
    return p


def all_landmarks(landmark_map):
    w, r, g = landmark_map
    return np.ascontiguousarray(np.concatenate([w, r, g]), np.float64), len(w), len(r), len(g)


def flags(X, pitch):
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    f = np.zeros(len(X), np.uint8)
    hc().hc_refine_flags(X.ctypes.data, len(X), float(pitch), f.ctypes.data)
    return f


def np_flags(X, pitch):
    """The rule of include/mantis.h restated: bit 0 = a neighbour at +- pitch along x, bit 1 along y."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    d = X[None, :, :] - X[:, None, :]  # d[i, j] = X_j - X_i
    off = ~np.eye(len(X), dtype=bool)
    same = lambda a: np.abs(a) <= 1e-6
    step = lambda a: (np.abs(a - pitch) <= 1e-6) | (np.abs(a + pitch) <= 1e-6)
    fx = (step(d[:, :, 0]) & same(d[:, :, 1]) & same(d[:, :, 2]) & off).any(axis=1)
    fy = (step(d[:, :, 1]) & same(d[:, :, 0]) & same(d[:, :, 2]) & off).any(axis=1)
    return (fx.astype(np.uint8) | (fy.astype(np.uint8) << 1)).astype(np.uint8)


def candidates(f):
    return [i for i in range(len(f)) if f[i] in (1, 2)]


# The row counts at which a trip loop of the MFMA accumulations ends differently: some waves without a trip, one
# short group, one row past whole trips, one row short of them. (A trip of the 7-column loop is 128 rows, eight
# groups of four per wave; a trip of a calibration's wave is 32 rows of one camera, 16 with the 21-column row.)
ROW_CLASSES = {"rows<16": lambda n: 1 <= n < 16, "16<=rows<128": lambda n: 16 <= n < 128,
               "rows%128=1": lambda n: n > 128 and n % 128 == 1, "rows%128=127": lambda n: n > 128 and n % 128 == 127}
# (class, cameras) of the refinement's cases: three cameras, but for the class below 128 rows, where three cameras
# leave at most 42 candidates, all on the red and green border, whose normal matrix is singular (the plain call
# says SINGULAR, and a weighted one is decided by its last bits); one camera's 127 candidates hold white lines.
TAIL_CASES = [("rows<16", 3), ("16<=rows<128", 1), ("rows%128=1", 3), ("rows%128=127", 3)]


def cut_map(landmark_map, cls, per=1, pitch=0.08):
    """The map with landmarks dropped from the front, as test_odd_candidate_count cuts it, until `per` x its
    candidate count is in the row class `cls`: white ones first, and on into the red and the green, which alone
    still hold 74 candidates. Returns ((w, r, g), (X, nw, nr, ng), n_cand)."""
    w, r, g = landmark_map
    for drop in range(1, len(w) + len(r) + len(g)):
        cut = (w[drop:], r[max(drop - len(w), 0):], g[max(drop - len(w) - len(r), 0):])
        X = np.ascontiguousarray(np.concatenate(cut), np.float64).reshape(-1, 3)
        nc = len(candidates(flags(X, pitch)))
        if ROW_CLASSES[cls](per * nc):
            return cut, (X, len(cut[0]), len(cut[1]), len(cut[2])), nc
    raise AssertionError(f"no cut of the map gives {per} x n_cand in {cls}")


def obs(T, Tbc, K, D, img, X, nw, nr, ng, f, R=12, white_thresh=12288, min_weight=24576):
    """hc_refine_obs: (codes, Sw, Skw, rows [n_cand, 7], tie [n_cand]) of one pass for one camera."""
    T = np.ascontiguousarray(T, np.float64)
    Tbc = np.ascontiguousarray(Tbc, np.float64)
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    D = np.ascontiguousarray(D, np.float64).reshape(4)
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    f = np.ascontiguousarray(f, np.uint8)
    nc = len(candidates(f))
    codes = np.zeros(nc, np.int32)
    Sw = np.zeros(nc, np.int32)
    Skw = np.zeros(nc, np.int32)
    rows = np.zeros((nc, 7))
    tie = np.zeros(nc, np.int32)
    got = hc().hc_refine_obs(T.ctypes.data, Tbc.ctypes.data, K.ctypes.data, D.ctypes.data, img.ctypes.data, w, h,
                             X.ctypes.data, nw, nr, ng, f.ctypes.data, R, white_thresh, min_weight, codes.ctypes.data,
                             Sw.ctypes.data, Skw.ctypes.data, rows.ctypes.data, tie.ctypes.data)
    assert got == nc
    return codes, Sw, Skw, rows, tie


def accumulate(rows):
    rows = np.ascontiguousarray(rows, np.float64).reshape(-1, 7)
    acc = np.zeros(28)
    hc().hc_refine_accumulate(rows.ctypes.data, len(rows), acc.ctypes.data)
    return acc


def np_acc28(rows):
    """Upper triangle of J^T J, J^T r, r^T r from rows [J | r] (numpy sums)."""
    M = np.asarray(rows, np.float64).reshape(-1, 7)
    G = M.T @ M
    return np.concatenate([G[:6, :6][np.triu_indices(6)], G[:6, 6], [G[6, 6]]])


def solve6(acc, lam, T):
    acc = np.ascontiguousarray(acc, np.float64)
    Tn = np.ascontiguousarray(T, np.float64).copy()
    d6 = np.zeros(6)
    ok = hc().hc_gn_solve6(acc.ctypes.data, float(lam), Tn.ctypes.data, d6.ctypes.data)
    return bool(ok), Tn, d6


def per_camera(K, D, Cn):
    """(Ks [Cn, 9], Ds [Cn, 4]) from one K (3 x 3) and D (4) for every camera, or from one of each per camera."""
    Ks, Ds = np.asarray(K, np.float64).reshape(-1, 9), np.asarray(D, np.float64).reshape(-1, 4)
    if len(Ks) == 1:
        Ks = np.tile(Ks, (Cn, 1))
    if len(Ds) == 1:
        Ds = np.tile(Ds, (Cn, 1))
    assert Ks.shape == (Cn, 9) and Ds.shape == (Cn, 4)
    return np.ascontiguousarray(Ks), np.ascontiguousarray(Ds)


def lenses(n, w, h, Ks=None, Ds=None):
    """Per-camera (Ks, Ds) of the GPU checkers: the bench lens of the frame size for every camera unless they
    are given."""
    if Ks is None:
        K, D = synth.intrinsics(w, h)
        Ks, Ds = [K] * n, [D] * n
    assert len(Ks) == len(Ds) == n
    return Ks, Ds


def seq(T_in, exts, imgs, X, nw, nr, ng, p, K=None, D=None):
    """hc_refine_seq on one rig: a MantisRefineResult. K, D: one for every camera, or one per camera."""
    import mantis_amd as M

    Cn = len(imgs)
    h, w = imgs[0].shape[:2]
    if K is None:
        K, D = synth.intrinsics(w, h)
    T = np.ascontiguousarray(T_in, np.float64)
    E = np.ascontiguousarray(np.array(exts, np.float64).reshape(Cn, 16))
    Ks, Ds = per_camera(K, D, Cn)
    keep = [np.ascontiguousarray(i, np.uint8) for i in imgs]
    ptrs = (C.c_void_p * Cn)(*[k.ctypes.data for k in keep])
    out = M.MantisRefineResult()
    hc().hc_refine_seq(T.ctypes.data, E.ctypes.data, Ks.ctypes.data, Ds.ctypes.data, ptrs, Cn, w, h, X.ctypes.data, nw,
                       nr, ng, C.byref(p), C.byref(out))
    return out


# ---- the rule in plain Python / numpy (include/mantis.h) ----
def np_distort(K, D, x, y):
    fx, fy, cx, cy = (float(np.float32(K[0, 0])), float(np.float32(K[1, 1])), float(np.float32(K[0, 2])),
                      float(np.float32(K[1, 2])))
    r = math.sqrt(x * x + y * y)
    th = math.atan(r)
    thd = th + D[0] * th ** 3 + D[1] * th ** 5 + D[2] * th ** 7 + D[3] * th ** 9
    cd = thd / r if r > 1e-8 else 1.0
    return x * cd * fx + cx, y * cd * fy + cy


def np_geometry(T, Tbc, Xi, axis):
    """(p, q, m0, nh, Jpi, R_cb) of steps 1-3, or a reject code."""
    Tcb = np.linalg.inv(Tbc)
    R_cb, t_cb = Tcb[:3, :3], Tcb[:3, 3]
    R_wb, t_wb = T[:3, :3], T[:3, 3]
    q = R_wb.T @ (Xi - t_wb)
    p = R_cb @ q + t_cb
    if p[2] <= 0:
        return 1
    iz = 1.0 / p[2]
    m0 = np.array([p[0] * iz, p[1] * iz])
    Jpi = np.array([[iz, 0, -p[0] * iz * iz], [0, iz, -p[1] * iz * iz]])
    e = np.zeros(3)
    e[axis] = 1.0
    t = Jpi @ (R_cb @ R_wb.T @ e)
    tn = math.hypot(t[0], t[1])
    if tn < 1e-12:
        return 2
    th = t / tn
    nh = np.array([-th[1], th[0]])
    return p, q, m0, nh, Jpi, R_cb


def np_observe(T, Tbc, K, D, img, Xi, axis, target, R=12, white_thresh=12288, min_weight=24576):
    """(code, Sw, Skw, row7) of one observation, the rule of include/mantis.h step by step."""
    g = np_geometry(T, Tbc, Xi, axis)
    zero = np.zeros(7)
    if isinstance(g, int):
        return g, 0, 0, zero
    p, q, m0, nh, Jpi, R_cb = g
    h, w = img.shape[:2]
    s = 1.0 / float(np.float32(K[0, 0]))
    px = []
    for k in range(-R, R + 1):
        u, v = np_distort(K, D, m0[0] + (k * s) * nh[0], m0[1] + (k * s) * nh[1])
        if not (math.isfinite(u) and math.isfinite(v)):
            return 3, 0, 0, zero
        x, y = int(np.rint(u)), int(np.rint(v))  # rint: half to even, as cvRound
        if not (0 <= x < w and 0 <= y < h):
            return 3, 0, 0, zero
        px.append((x, y))
    ws = []
    for x, y in px:
        d2 = sum((int(img[y, x, ch]) - target[ch]) ** 2 for ch in range(3))
        ws.append(max(0, white_thresh - d2))
    Sw = sum(ws)
    Skw = sum(k * wk for k, wk in zip(range(-R, R + 1), ws))
    if ws[0] > 0 or ws[-1] > 0:
        return 4, Sw, Skw, zero
    if Sw < min_weight:
        return 5, Sw, Skw, zero
    d = (Skw / Sw) * s
    hrow = (nh @ Jpi) @ R_cb
    qx = np.array([[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]])
    return 0, Sw, Skw, np.concatenate([-hrow, hrow @ qx, [-d]])


def exp_right(T, d6):
    """T Exp(delta): translation d6[:3], rotation vector d6[3:] (Rodrigues)."""
    w = np.asarray(d6[3:], np.float64)
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        Rm = np.eye(3) + Kx + 0.5 * Kx @ Kx
    else:
        Rm = np.eye(3) + math.sin(th) / th * Kx + (1 - math.cos(th)) / th ** 2 * Kx @ Kx
    Dm = np.eye(4)
    Dm[:3, :3] = Rm
    Dm[:3, 3] = d6[:3]
    return T @ Dm


def np_covariance(acc, n_obs, T):
    """sigma^2 (J^T J)^-1 with the translation block turned to the world frame."""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = acc[:21]
    A = A + np.triu(A, 1).T
    cov = acc[27] / (n_obs - 6) * np.linalg.inv(A)
    B = np.eye(6)
    B[:3, :3] = T[:3, :3]
    return B @ cov @ B.T, A


# ---- scenes ----
def shift(T):
    """The start: the truth moved by 2 cm and turned by 1 degree (the tracking tests' _shift)."""
    d = np.eye(4)
    d[:3, :3] = synth.rot_z(math.radians(1.0))
    d[:3, 3] = [0.02, 0.0, 0.0]
    return T @ d


def pose_dist(A, B):
    """(translation distance, rotation angle in degrees) between two poses."""
    dt = float(np.linalg.norm(A[:3, 3] - B[:3, 3]))
    c = (np.trace(A[:3, :3].T @ B[:3, :3]) - 1.0) / 2.0
    return dt, math.degrees(math.acos(min(1.0, max(-1.0, c))))


def rig_scene(n_cams=4, n_rigs=1, seed=2024, w=W, h=H_, cfg=12):
    """Base poses from default_rng(seed), rendered through every camera of the
    ring synth.rig_extrinsics(n_cams): {"ext", "Twb" [r], "frames" [r][c]}."""
    rng = np.random.default_rng(seed)
    ext = synth.rig_extrinsics(n_cams)
    Twb, frames = [], []
    for r in range(n_rigs):
        T = synth.random_base_pose(rng)
        Twb.append(T)
        fr = []
        for c in range(n_cams):
            Twc = T @ ext[c]
            fr.append(synth.render_host(synth.make_cam(Twc[:3, :3], Twc[:3, 3], w, h), synth.frame_seed(cfg, 100 * r + c)))
        frames.append(fr)
    return {"ext": ext, "Twb": Twb, "frames": frames}
