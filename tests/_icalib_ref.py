"""Intrinsic calibration, test side: ctypes bindings of the host build's
hc_icalib_* (mantis_amd/csrc/mk_icalib.h through build/libmantis_hostcheck.so),
the full normal system of include/mantis.h assembled in numpy, the model gap
between two sets of intrinsics, and the scenes the CPU and GPU tests share.
"""
import ctypes as C
import functools
import math

import numpy as np

import _refine_ref as RR
from mantis_amd import synth

ACC = 120
ROW = 15
TRI = np.triu_indices(ROW)
W, H_ = RR.W, RR.H_


def hc():
    import mantis_amd as M

    L = RR.hc()
    vp = C.c_void_p
    L.hc_icalib_obs.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int,
                                C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.hc_icalib_obs.restype = C.c_int
    L.hc_icalib_accumulate.argtypes = [vp, C.c_int, vp]
    L.hc_icalib_accumulate.restype = None
    L.hc_icalib_end_pass.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_double, vp, C.POINTER(M.MantisIcalibResult), vp]
    L.hc_icalib_end_pass.restype = C.c_int
    L.hc_icalib_seq.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                C.POINTER(M.MantisRefineParams), C.POINTER(M.MantisIcalibParams), vp,
                                C.POINTER(M.MantisIcalibResult)]
    L.hc_icalib_seq.restype = None
    L.hc_icalib_conclude.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                     C.POINTER(M.MantisIcalibResult)]
    L.hc_icalib_conclude.restype = None
    L.hc_sizeof_icalib_params.restype = C.c_int
    L.hc_sizeof_icalib_result.restype = C.c_int
    return L


def icalib_params(free_cams, param_mask=None, min_obs_cam=None):
    import mantis_amd as M

    p = M.MantisIcalibParams()
    M.lib().mantis_default_icalib_params(C.byref(p))
    p.free_cams = free_cams
    if param_mask is not None:
        p.param_mask = param_mask
    if min_obs_cam is not None:
        p.min_obs_cam = min_obs_cam
    return p


# ---- intrinsics as the eight unknowns: fx, fy, cx, cy, k1..k4 ----
def kd_of(K, D):
    """K (3 x 3, rounded to float as the library does) and D as the eight unknowns."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    f32 = lambda v: float(np.float32(v))
    return np.array([f32(K[0, 0]), f32(K[1, 1]), f32(K[0, 2]), f32(K[1, 2])] + list(np.asarray(D, np.float64)))


def K_of(kd):
    return np.array([[kd[0], 0, kd[2]], [0, kd[1], kd[3]], [0, 0, 1.0]])


def kds_of(R):
    """The result's intrinsics: [n_cams, 8]."""
    return np.array([list(R.K[c]) + list(R.D[c]) for c in range(R.n_cams)])


def np_dist(kd, x, y):
    """The fisheye projection of normalized points through the eight intrinsics, in pixels (numpy)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    r = np.sqrt(x * x + y * y)
    th = np.arctan(r)
    thd = th + kd[4] * th ** 3 + kd[5] * th ** 5 + kd[6] * th ** 7 + kd[7] * th ** 9
    cd = np.where(r > 1e-8, thd / np.where(r > 1e-8, r, 1.0), 1.0)
    return x * cd * kd[0] + kd[2], y * cd * kd[1] + kd[3]


def model_gap(kd, kd_true, w=W, h=H_, span=(2.2, 1.3)):
    """rms over the 23 x 14 grid of normalized points whose true image lies in the frame of
    |dist_kd - dist_true|, in pixels. span: the grid's half extent (the bench lens's field; a narrower lens
    needs a narrower grid to keep its points in the frame)."""
    gx, gy = np.meshgrid(np.linspace(-span[0], span[0], 23), np.linspace(-span[1], span[1], 14))
    ut, vt = np_dist(kd_true, gx, gy)
    inside = (ut >= 0) & (ut <= w - 1) & (vt >= 0) & (vt <= h - 1)
    assert inside.sum() > 100
    u, v = np_dist(kd, gx, gy)
    return float(np.sqrt(((u - ut) ** 2 + (v - vt) ** 2)[inside].mean()))


def obs(T, Tbc, kd, img, X, nw, nr, ng, f, free_cam, mask=0xFF, R=12, white_thresh=12288, min_weight=24576):
    """hc_icalib_obs: (codes, Sw, Skw, rows [n_cand, 15], tie [n_cand]) of one pass for one camera."""
    T = np.ascontiguousarray(T, np.float64)
    Tbc = np.ascontiguousarray(Tbc, np.float64)
    kd = np.ascontiguousarray(kd, np.float64).reshape(8)
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    f = np.ascontiguousarray(f, np.uint8)
    nc = len(RR.candidates(f))
    codes = np.zeros(nc, np.int32)
    Sw = np.zeros(nc, np.int32)
    Skw = np.zeros(nc, np.int32)
    rows = np.zeros((nc, ROW))
    tie = np.zeros(nc, np.int32)
    got = hc().hc_icalib_obs(T.ctypes.data, Tbc.ctypes.data, kd.ctypes.data, img.ctypes.data, w, h, X.ctypes.data, nw,
                             nr, ng, f.ctypes.data, R, white_thresh, min_weight, int(bool(free_cam)), int(mask),
                             codes.ctypes.data, Sw.ctypes.data, Skw.ctypes.data, rows.ctypes.data, tie.ctypes.data)
    assert got == nc
    return codes, Sw, Skw, rows, tie


def accumulate(rows):
    rows = np.ascontiguousarray(rows, np.float64).reshape(-1, ROW)
    acc = np.zeros(ACC)
    hc().hc_icalib_accumulate(rows.ctypes.data, len(rows), acc.ctypes.data)
    return acc


def np_acc120(rows):
    """(the upper triangle of M^T M in numpy sums, the bound of those sums' own rounding error:
    n 2^-53 |M|^T |M|, the textbook bound of a float64 dot product of n terms)."""
    M = np.asarray(rows, np.float64).reshape(-1, ROW)
    return (M.T @ M)[TRI], (len(M) * 2.0 ** -53 * (np.abs(M).T @ np.abs(M)))[TRI]


def pass_acc(Ts, exts, kds, frames, lm, free_cams, mask, p):
    """One observation pass on the host: (acc120 [N, C, 120], cnt [N, C]) at the poses Ts and intrinsics kds."""
    X, nw, nr, ng = lm
    N, Cn = len(Ts), len(exts)
    f = RR.flags(X, p.landmark_pitch)
    acc = np.zeros((N, Cn, ACC))
    cnt = np.zeros((N, Cn), np.int32)
    for r in range(N):
        for c in range(Cn):
            codes, _, _, rows, _ = obs(Ts[r], exts[c], kds[c], frames[r][c], X, nw, nr, ng, f, free_cams >> c & 1,
                                       mask, R=p.half_window, white_thresh=p.white_thresh, min_weight=p.min_weight)
            acc[r, c] = accumulate(rows)
            cnt[r, c] = int((codes == 0).sum())
    return acc, cnt


def new_result(kds, free_cams, mask, N, n_cand=0):
    import mantis_amd as M

    R = M.MantisIcalibResult()
    R.n_cand, R.n_rigs, R.n_cams, R.free_cams, R.param_mask = n_cand, N, len(kds), free_cams, mask
    for c, kd in enumerate(kds):
        for k in range(4):
            R.K[c][k] = kd[k]
            R.D[c][k] = kd[4 + k]
    return R


def end_pass(acc, cnt, free_cams, mask, pass_, I, p, ip, Ts, R):
    """hc_icalib_end_pass on R (in / out): (finished, T_next [N, 4, 4], delta [N, 6])."""
    acc = np.ascontiguousarray(acc, np.float64)
    cnt = np.ascontiguousarray(cnt, np.int32)
    N, Cn = cnt.shape
    T = np.ascontiguousarray(np.array(Ts, np.float64).reshape(N, 16)).copy()
    d = np.zeros((N, 6))
    fin = hc().hc_icalib_end_pass(acc.ctypes.data, cnt.ctypes.data, N, Cn, free_cams, mask, pass_, I, p.min_obs,
                                  ip.min_obs_cam, p.lambda_, T.ctypes.data, C.byref(R), d.ctypes.data)
    return bool(fin), T.reshape(N, 4, 4), d


def conclude(acc, cnt, free_cams, mask, p, ip, R):
    acc = np.ascontiguousarray(acc, np.float64)
    cnt = np.ascontiguousarray(cnt, np.int32)
    N, Cn = cnt.shape
    hc().hc_icalib_conclude(acc.ctypes.data, cnt.ctypes.data, N, Cn, free_cams, mask, p.min_obs, ip.min_obs_cam,
                            p.max_rms, C.byref(R))


def seq(T_in, exts, Ks, Ds, frames, lm, p, ip):
    """hc_icalib_seq: (T_out [N, 4, 4], MantisIcalibResult). frames[r][c]; Ks [C, 3, 3], Ds [C, 4]."""
    import mantis_amd as M

    X, nw, nr, ng = lm
    N, Cn = len(frames), len(exts)
    h, w = frames[0][0].shape[:2]
    T = np.ascontiguousarray(np.array(T_in, np.float64).reshape(N, 16))
    E = np.ascontiguousarray(np.array(exts, np.float64).reshape(Cn, 16))
    Ks = np.ascontiguousarray(np.array(Ks, np.float64).reshape(Cn, 9))
    Ds = np.ascontiguousarray(np.array(Ds, np.float64).reshape(Cn, 4))
    keep = [np.ascontiguousarray(frames[r][c], np.uint8) for r in range(N) for c in range(Cn)]
    ptrs = (C.c_void_p * (N * Cn))(*[k.ctypes.data for k in keep])
    T_out = np.zeros((N, 4, 4))
    out = M.MantisIcalibResult()
    hc().hc_icalib_seq(T.ctypes.data, E.ctypes.data, Ks.ctypes.data, Ds.ctypes.data, ptrs, N, Cn, w, h, X.ctypes.data,
                       nw, nr, ng, C.byref(p), C.byref(ip), T_out.ctypes.data, C.byref(out))
    return T_out, out


# ---- the rule in numpy: the full (6 N + 8 F) normal system ----
def sym15(a120):
    G = np.zeros((ROW, ROW))
    G[TRI] = a120
    return G + np.triu(G, 1).T


def free_list(free_cams, Cn):
    return [c for c in range(Cn) if free_cams >> c & 1]


def np_normal(acc, free_cams, mask, lam=0.0):
    """(H, g): the normal matrix over [poses (6 N) | free cameras (8 F)] and the gradient J^T r; a held
    parameter's row and column are the identity's (its J_int column is zero), its gradient 0."""
    N, Cn = acc.shape[:2]
    fl = free_list(free_cams, Cn)
    n = 6 * N + 8 * len(fl)
    Hm, g = np.zeros((n, n)), np.zeros(n)
    for r in range(N):
        P = slice(6 * r, 6 * r + 6)
        for c in range(Cn):
            G = sym15(acc[r, c])
            Hm[P, P] += G[:6, :6]
            g[P] += G[:6, 14]
            if c in fl:
                E = slice(6 * N + 8 * fl.index(c), 6 * N + 8 * fl.index(c) + 8)
                Hm[P, E] += G[:6, 6:14]
                Hm[E, P] += G[6:14, :6]
                Hm[E, E] += G[6:14, 6:14]
                g[E] += G[6:14, 14]
    Hm = Hm + lam * np.eye(n)
    for f in range(len(fl)):
        for e in range(8):
            if not mask >> e & 1:
                Hm[6 * N + 8 * f + e, 6 * N + 8 * f + e] = 1.0
    return Hm, g


def np_update(kd, eps, mask):
    """theta (+) eps of include/mantis.h for the free parameters."""
    out = np.array(kd, np.float64)
    new = [kd[0] * (1 + eps[0]), kd[1] * (1 + eps[1]), kd[2] + kd[0] * eps[2], kd[3] + kd[1] * eps[3]] + \
          [kd[4 + i] + eps[4 + i] for i in range(4)]
    for e in range(8):
        if mask >> e & 1:
            out[e] = new[e]
    return out


# ---- scenes ----
def true_kds(n_cams=4, w=W, h=H_):
    """The nominal intrinsics moved by 1 % in fx and fy, 2 px in cx and cy, 0.004 in k1 and 0.002 in k2, the
    signs from default_rng(7) drawn per camera in camera order: [n_cams, 8]."""
    K, D = synth.intrinsics(w, h)
    nom = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]] + list(D))
    rng = np.random.default_rng(7)
    out = []
    for c in range(n_cams):
        s = rng.choice([-1.0, 1.0], 8)
        t = nom.copy()
        t[0] *= 1 + 0.01 * s[0]
        t[1] *= 1 + 0.01 * s[1]
        t[2] += 2 * s[2]
        t[3] += 2 * s[3]
        t[4] += 0.004 * s[4]
        t[5] += 0.002 * s[5]
        out.append(t)
    return np.array(out)


def _render(Twc, kd, seed, w=W, h=H_):
    cam = synth.make_cam(Twc[:3, :3], Twc[:3, 3], w, h)
    cam.fx, cam.fy, cam.cx, cam.cy = kd[:4]
    for i in range(4):
        cam.k[i] = kd[4 + i]
    return synth.render_host(cam, seed)


def _views(rng, n, n_cams, kds, seed0, w=W, h=H_, cfg=12):
    ext = synth.rig_extrinsics(n_cams)
    Twb, frames = [], []
    for r in range(n):
        T = synth.random_base_pose(rng)
        Twb.append(T)
        frames.append([_render(T @ ext[c], kds[c], synth.frame_seed(cfg, seed0 + 100 * r + c), w, h)
                       for c in range(n_cams)])
    return ext, Twb, frames


@functools.lru_cache(maxsize=None)
def gap_scene(n_cams=4, n_rigs=3, seed=2024, w=W, h=H_):
    """RR.rig_scene's poses, every camera rendered through its true intrinsics: {"ext", "Twb", "frames" [r][c],
    "T0" (the truth moved by 2 cm / 1 degree), "K", "D" (nominal), "kd0" / "kd_true" [C, 8]}."""
    kt = true_kds(n_cams, w, h)
    ext, Twb, frames = _views(np.random.default_rng(seed), n_rigs, n_cams, kt, 0, w, h)
    K, D = synth.intrinsics(w, h)
    return {"ext": ext, "Twb": Twb, "frames": frames, "T0": [RR.shift(T) for T in Twb], "K": K, "D": D,
            "kd0": np.tile(kd_of(K, D), (n_cams, 1)), "kd_true": kt}


@functools.lru_cache(maxsize=None)
def fresh_views(n=4, seed=4242):
    """n fresh views of the four-camera rig through the same true intrinsics: {"Twb", "frames" [r][c]}."""
    _, Twb, frames = _views(np.random.default_rng(seed), n, 4, true_kds(4), 1000)
    return {"Twb": Twb, "frames": frames}


def refine_with(T0, exts, kds, imgs, lm, p):
    """hc_refine_seq of one rig with per-camera intrinsics kds [C, 8] (K is rounded to float there)."""
    import mantis_amd as M

    X, nw, nr, ng = lm
    Cn = len(imgs)
    h, w = imgs[0].shape[:2]
    T = np.ascontiguousarray(T0, np.float64)
    E = np.ascontiguousarray(np.array(exts, np.float64).reshape(Cn, 16))
    Ks = np.ascontiguousarray(np.array([K_of(kd).reshape(9) for kd in kds]))
    Ds = np.ascontiguousarray(np.array([kd[4:] for kd in kds]))
    keep = [np.ascontiguousarray(i, np.uint8) for i in imgs]
    ptrs = (C.c_void_p * Cn)(*[k.ctypes.data for k in keep])
    out = M.MantisRefineResult()
    RR.hc().hc_refine_seq(T.ctypes.data, E.ctypes.data, Ks.ctypes.data, Ds.ctypes.data, ptrs, Cn, w, h, X.ctypes.data,
                          nw, nr, ng, C.byref(p), C.byref(out))
    return out


def accuracy_checks(T_out, R, lm, sc=None):
    """The accuracy conditions of the issue on a result of gap_scene() (all cameras free, mask 0xFF, four
    iterations): calibrated; every camera's model gap below a tenth of its start; every pose within 0.2 cm;
    every fresh view refined by hc_refine_seq with the calibrated intrinsics has refined = 1 and ends at less
    than half its distance with the nominal ones. Returns the figures."""
    sc = sc or gap_scene()
    kds = kds_of(R)
    assert R.status == 0 and R.calibrated == 1, (R.status, R.calibrated)
    gaps = []
    for c in range(4):
        g0, g1 = model_gap(sc["kd0"][c], sc["kd_true"][c]), model_gap(kds[c], sc["kd_true"][c])
        gaps.append((g0, g1))
    poses = [RR.pose_dist(T_out[r], sc["Twb"][r])[0] for r in range(len(sc["Twb"]))]
    print("model gap px (start, end):", [(round(a, 3), round(b, 4)) for a, b in gaps])
    print("poses cm:", [round(100 * d, 4) for d in poses])
    fv = fresh_views()
    p = RR.default_params()
    ratios = []
    for r in range(len(fv["Twb"])):
        T, T0 = fv["Twb"][r], RR.shift(fv["Twb"][r])
        given = refine_with(T0, sc["ext"], sc["kd0"], fv["frames"][r], lm, p)
        calib = refine_with(T0, sc["ext"], kds, fv["frames"][r], lm, p)
        dg = RR.pose_dist(np.array(given.T_w_b).reshape(4, 4), T)[0]
        dc = RR.pose_dist(np.array(calib.T_w_b).reshape(4, 4), T)[0]
        ratios.append((dg, dc, calib.refined))
    print("fresh views (nominal, calibrated) cm:", [(round(100 * a, 4), round(100 * b, 4)) for a, b, _ in ratios])
    for g0, g1 in gaps:
        assert g1 < 0.1 * g0, gaps
    assert max(poses) < 0.002, poses
    for dg, dc, ok in ratios:
        assert ok == 1 and dc < 0.5 * dg, ratios
    return {"gaps": gaps, "poses": poses, "fresh": ratios}
