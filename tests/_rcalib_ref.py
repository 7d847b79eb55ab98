"""Rig calibration, test side: ctypes bindings of the host build's hc_rcalib_*
(mantis_amd/csrc/mk_rcalib.h through build/libmantis_hostcheck.so), the full
normal system of include/mantis.h over (6 N + 6 Fe + 8 Fi) assembled in numpy,
the alternation of the two single calibrations through the same host rule, and
the scenes the CPU and GPU tests share.
"""
import ctypes as C
import functools
import math

import numpy as np

import _icalib_ref as IR
import _refine_ref as RR
from mantis_amd import synth

ACC = 231
ROW = 21
TRI = np.triu_indices(ROW)
W, H_ = RR.W, RR.H_


def hc():
    import mantis_amd as M

    L = IR.hc()
    vp = C.c_void_p
    L.hc_rcalib_obs.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int,
                                C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.hc_rcalib_obs.restype = C.c_int
    L.hc_rcalib_accumulate.argtypes = [vp, C.c_int, vp]
    L.hc_rcalib_accumulate.restype = None
    L.hc_rcalib_end_pass.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_double, vp, C.POINTER(M.MantisRcalibResult), vp]
    L.hc_rcalib_end_pass.restype = C.c_int
    L.hc_rcalib_seq.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                C.POINTER(M.MantisRefineParams), C.POINTER(M.MantisRcalibParams), vp,
                                C.POINTER(M.MantisRcalibResult)]
    L.hc_rcalib_seq.restype = None
    L.hc_rcalib_conclude.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_double, C.POINTER(M.MantisRcalibResult)]
    L.hc_rcalib_conclude.restype = None
    L.hc_sizeof_rcalib_params.restype = C.c_int
    L.hc_sizeof_rcalib_result.restype = C.c_int
    return L


def rcalib_params(free_ext, free_int, param_mask=None, min_obs_cam=None):
    import mantis_amd as M

    p = M.MantisRcalibParams()
    M.lib().mantis_default_rcalib_params(C.byref(p))
    p.free_ext, p.free_int = free_ext, free_int
    if param_mask is not None:
        p.param_mask = param_mask
    if min_obs_cam is not None:
        p.min_obs_cam = min_obs_cam
    return p


def exts_of(R):
    """The result's extrinsics: [n_cams, 4, 4]."""
    return np.array([list(R.T_base_cam[c]) for c in range(R.n_cams)]).reshape(R.n_cams, 4, 4)


kds_of = IR.kds_of


def obs(T, Tbc, kd, img, X, nw, nr, ng, f, free_ext, free_int, mask=0xFF, R=12, white_thresh=12288,
        min_weight=24576):
    """hc_rcalib_obs: (codes, Sw, Skw, rows [n_cand, 21], tie [n_cand]) of one pass for one camera."""
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
    got = hc().hc_rcalib_obs(T.ctypes.data, Tbc.ctypes.data, kd.ctypes.data, img.ctypes.data, w, h, X.ctypes.data, nw,
                             nr, ng, f.ctypes.data, R, white_thresh, min_weight, int(bool(free_ext)),
                             int(bool(free_int)), int(mask), codes.ctypes.data, Sw.ctypes.data, Skw.ctypes.data,
                             rows.ctypes.data, tie.ctypes.data)
    assert got == nc
    return codes, Sw, Skw, rows, tie


def accumulate(rows):
    rows = np.ascontiguousarray(rows, np.float64).reshape(-1, ROW)
    acc = np.zeros(ACC)
    hc().hc_rcalib_accumulate(rows.ctypes.data, len(rows), acc.ctypes.data)
    return acc


def np_acc231(rows):
    """(the upper triangle of M^T M in numpy sums, the bound of those sums' own rounding error:
    n 2^-53 |M|^T |M|, the textbook bound of a float64 dot product of n terms)."""
    M = np.asarray(rows, np.float64).reshape(-1, ROW)
    return (M.T @ M)[TRI], (len(M) * 2.0 ** -53 * (np.abs(M).T @ np.abs(M)))[TRI]


def pass_acc(Ts, exts, kds, frames, lm, free_ext, free_int, mask, p):
    """One observation pass on the host: (acc231 [N, C, 231], cnt [N, C]) at the poses Ts, extrinsics exts and
    intrinsics kds."""
    X, nw, nr, ng = lm
    N, Cn = len(Ts), len(exts)
    f = RR.flags(X, p.landmark_pitch)
    acc = np.zeros((N, Cn, ACC))
    cnt = np.zeros((N, Cn), np.int32)
    for r in range(N):
        for c in range(Cn):
            codes, _, _, rows, _ = obs(Ts[r], exts[c], kds[c], frames[r][c], X, nw, nr, ng, f, free_ext >> c & 1,
                                       free_int >> c & 1, mask, R=p.half_window, white_thresh=p.white_thresh,
                                       min_weight=p.min_weight)
            acc[r, c] = accumulate(rows)
            cnt[r, c] = int((codes == 0).sum())
    return acc, cnt


def new_result(exts, kds, free_ext, free_int, mask, N, n_cand=0):
    import mantis_amd as M

    R = M.MantisRcalibResult()
    R.n_cand, R.n_rigs, R.n_cams = n_cand, N, len(kds)
    R.free_ext, R.free_int, R.param_mask = free_ext, free_int, mask
    for c, kd in enumerate(kds):
        for k in range(4):
            R.K[c][k] = kd[k]
            R.D[c][k] = kd[4 + k]
        for k, v in enumerate(np.asarray(exts[c], np.float64).reshape(16)):
            R.T_base_cam[c][k] = v
    return R


def end_pass(acc, cnt, free_ext, free_int, mask, pass_, I, p, rp, Ts, R):
    """hc_rcalib_end_pass on R (in / out): (finished, T_next [N, 4, 4], delta [N, 6])."""
    acc = np.ascontiguousarray(acc, np.float64)
    cnt = np.ascontiguousarray(cnt, np.int32)
    N, Cn = cnt.shape
    T = np.ascontiguousarray(np.array(Ts, np.float64).reshape(N, 16)).copy()
    d = np.zeros((N, 6))
    fin = hc().hc_rcalib_end_pass(acc.ctypes.data, cnt.ctypes.data, N, Cn, free_ext, free_int, mask, pass_, I,
                                  p.min_obs, rp.min_obs_cam, p.lambda_, T.ctypes.data, C.byref(R), d.ctypes.data)
    return bool(fin), T.reshape(N, 4, 4), d


def conclude(acc, cnt, free_ext, free_int, mask, p, rp, R):
    acc = np.ascontiguousarray(acc, np.float64)
    cnt = np.ascontiguousarray(cnt, np.int32)
    N, Cn = cnt.shape
    hc().hc_rcalib_conclude(acc.ctypes.data, cnt.ctypes.data, N, Cn, free_ext, free_int, mask, p.min_obs,
                            rp.min_obs_cam, p.max_rms, C.byref(R))


def seq(T_in, exts, Ks, Ds, frames, lm, p, rp):
    """hc_rcalib_seq: (T_out [N, 4, 4], MantisRcalibResult). frames[r][c]; Ks [C, 3, 3], Ds [C, 4]."""
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
    out = M.MantisRcalibResult()
    hc().hc_rcalib_seq(T.ctypes.data, E.ctypes.data, Ks.ctypes.data, Ds.ctypes.data, ptrs, N, Cn, w, h, X.ctypes.data,
                       nw, nr, ng, C.byref(p), C.byref(rp), T_out.ctypes.data, C.byref(out))
    return T_out, out


# ---- the rule in numpy: the full (6 N + 6 Fe + 8 Fi) normal system ----
def sym21(a231):
    G = np.zeros((ROW, ROW))
    G[TRI] = a231
    return G + np.triu(G, 1).T


def free_list(mask, Cn):
    return [c for c in range(Cn) if mask >> c & 1]


def offsets(free_ext, free_int, N, Cn):
    """({camera: offset of its extrinsic block}, {camera: offset of its intrinsic block}, n) in the full system:
    poses, then the extrinsic blocks, then the intrinsic blocks."""
    fe, fi = free_list(free_ext, Cn), free_list(free_int, Cn)
    oe = {c: 6 * N + 6 * k for k, c in enumerate(fe)}
    oi = {c: 6 * N + 6 * len(fe) + 8 * k for k, c in enumerate(fi)}
    return oe, oi, 6 * N + 6 * len(fe) + 8 * len(fi)


def np_normal(acc, free_ext, free_int, mask, lam=0.0):
    """(H, g): the normal matrix over [poses (6 N) | extrinsics (6 Fe) | intrinsics (8 Fi)] and the gradient
    J^T r; a held parameter's row and column are the identity's (its J_int column is zero), its gradient 0."""
    N, Cn = acc.shape[:2]
    oe, oi, n = offsets(free_ext, free_int, N, Cn)
    Hm, g = np.zeros((n, n)), np.zeros(n)
    for r in range(N):
        for c in range(Cn):
            G = sym21(acc[r, c])
            idx, col = list(range(6 * r, 6 * r + 6)), list(range(6))
            if c in oe:
                idx += list(range(oe[c], oe[c] + 6))
                col += list(range(6, 12))
            if c in oi:
                idx += list(range(oi[c], oi[c] + 8))
                col += list(range(12, 20))
            Hm[np.ix_(idx, idx)] += G[np.ix_(col, col)]
            g[idx] += G[col, 20]
    Hm = Hm + lam * np.eye(n)
    for c, o in oi.items():
        for e in range(8):
            if not mask >> e & 1:
                Hm[o + e, o + e] = 1.0
    return Hm, g


def steps_of(R, pass_, free_ext, free_int, Cn):
    """The result's camera steps of a pass in the reduced order: the extrinsic blocks, then the intrinsic ones."""
    e = [list(R.delta_ext[pass_][c]) for c in free_list(free_ext, Cn)]
    i = [list(R.delta_int[pass_][c]) for c in free_list(free_int, Cn)]
    return np.array(sum(e, []) + sum(i, []))


# ---- scenes ----
def drifted_exts(ext0):            # camera 0 is the gauge
    rng, out = np.random.default_rng(11), [np.array(ext0[0])]
    for c in range(1, len(ext0)):
        a = rng.choice([-1, 1], 3) * math.radians(0.4)
        d = np.eye(4)
        d[:3, :3] = synth.rot_z(a[0]) @ synth.rot_x(a[1]) @ synth.rot_y(a[2])
        d[:3, 3] = rng.choice([-1, 1], 3) * 0.012 / math.sqrt(3)
        out.append(d @ ext0[c])
    return out


@functools.lru_cache(maxsize=None)
def joint_scene(n_cams=4, n_rigs=3, seed=2024, w=W, h=H_):
    """n_rigs views (synth.random_base_pose(default_rng(seed))) of the n_cams-camera rig, every camera rendered
    through its true intrinsics (IR.true_kds) and cameras 1.. through extrinsics 1.2 cm / 0.69 degrees off nominal:
    {"ext" (nominal), "ext_true", "Twb", "frames" [r][c], "T0" (the truth moved by 2 cm / 1 degree), "K", "D"
    (nominal), "kd0" / "kd_true" [C, 8]}."""
    kt = IR.true_kds(n_cams, w, h)
    ext = synth.rig_extrinsics(n_cams)
    et = drifted_exts(ext)
    rng = np.random.default_rng(seed)
    Twb, frames = [], []
    for r in range(n_rigs):
        T = synth.random_base_pose(rng)
        Twb.append(T)
        frames.append([IR._render(T @ et[c], kt[c], synth.frame_seed(12, 100 * r + c), w, h) for c in range(n_cams)])
    K, D = synth.intrinsics(w, h)
    return {"ext": [np.array(e) for e in ext], "ext_true": et, "Twb": Twb, "frames": frames,
            "T0": [RR.shift(T) for T in Twb], "K": K, "D": D, "kd0": np.tile(IR.kd_of(K, D), (n_cams, 1)),
            "kd_true": kt}


@functools.lru_cache(maxsize=None)
def fresh_views(n=4, seed=4242):
    """n fresh views of the four-camera rig through the true extrinsics and intrinsics (frame seeds
    1000 + 100 r + c): {"Twb", "frames" [r][c]}."""
    kt = IR.true_kds(4)
    et = drifted_exts(synth.rig_extrinsics(4))
    rng = np.random.default_rng(seed)
    Twb, frames = [], []
    for r in range(n):
        T = synth.random_base_pose(rng)
        Twb.append(T)
        frames.append([IR._render(T @ et[c], kt[c], synth.frame_seed(12, 1000 + 100 * r + c)) for c in range(4)])
    return {"Twb": Twb, "frames": frames}


def figures(T_out, exts, kds, sc):
    """(model gap px per camera, (translation m, rotation degrees) of every extrinsic against the truth, pose
    distance m per view) of an estimate on the scene."""
    Cn = len(sc["ext"])
    gaps = [IR.model_gap(kds[c], sc["kd_true"][c]) for c in range(Cn)]
    ext = [RR.pose_dist(np.array(exts[c]), sc["ext_true"][c]) for c in range(Cn)]
    poses = [RR.pose_dist(np.array(T_out[r]), sc["Twb"][r])[0] for r in range(len(sc["Twb"]))]
    return gaps, ext, poses


def alternation(sc, lm, rounds=2, iterations=4):
    """The two single calibrations in turn through the joint host rule with one mask empty (hc_calib_seq cannot
    take per-camera K): `iterations` of extrinsics-only (cameras 1.. free), then of intrinsics-only (all free),
    `rounds` times, each from the other's result. Returns (T [N, 4, 4], exts [C, 4, 4], kds [C, 8])."""
    Cn = len(sc["ext"])
    T, E, kds = np.array(sc["T0"]), np.array(sc["ext"]), np.array(sc["kd0"])
    p = RR.default_params(iterations=iterations)
    all_ = (1 << Cn) - 1
    for _ in range(rounds):
        for fe, fi in ((all_ & ~1, 0), (0, all_)):
            T, R = seq(T, E, [IR.K_of(k) for k in kds], [k[4:] for k in kds], sc["frames"], lm, p,
                       rcalib_params(fe, fi))
            assert R.status == 0 and R.iterations_run == iterations, (fe, fi, R.status)
            E, kds = exts_of(R), kds_of(R)
    return T, E, kds
