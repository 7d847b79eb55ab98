"""Robust rows of the three calibrations, test side: ctypes bindings of the
host build's hc_linecal_robust_* and hc_*_seq_robust / hc_*_end_pass_robust
(mantis_amd/csrc/mk_linecal.h through build/libmantis_hostcheck.so), one
adapter (`Spec`) that lets a test run the same steps on the extrinsic, the
intrinsic and the rig calibration, and the knocked scene the CPU and GPU tests
share: three views of the four-camera rig with one frame (view 1, camera 3)
taken after the camera was knocked by 3 cm and 1 degree.
"""
import ctypes as C
import functools
import math

import numpy as np

import _calib_ref as CR
import _icalib_ref as IR
import _rcalib_ref as RC
import _refine_ref as RR
import _refine_robust_ref as RB
from mantis_amd import synth

KINDS = ("ext", "int", "rig")
LOSSES = ("huber", "tukey")
KNOCK_VIEW, KNOCK_CAM = 1, 3


def hc():
    import mantis_amd as M

    L = RC.hc()
    CR.hc()
    RB.hc()
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    rp, st = C.POINTER(M.MantisRefineRobustParams), C.POINTER(M.MantisCalibRobustStats)
    L.hc_linecal_robust_weights.argtypes = [vp, vp, vp, ci, ci, ci, ci, cd, cd, vp, vp, vp, vp, vp, vp, vp, vp]
    L.hc_linecal_robust_weights.restype = None
    L.hc_linecal_robust_tally.argtypes = [vp, vp, vp, ci, ci, ci, C.c_uint32, cd, st]
    L.hc_linecal_robust_tally.restype = None
    seq = [vp, vp, vp, vp, vp, ci, ci, ci, ci, vp, ci, ci, ci, C.POINTER(M.MantisRefineParams)]
    L.hc_calib_seq_robust.argtypes = seq + [C.POINTER(M.MantisCalibParams), rp, vp, C.POINTER(M.MantisCalibResult), st]
    L.hc_icalib_seq_robust.argtypes = seq + [C.POINTER(M.MantisIcalibParams), rp, vp,
                                             C.POINTER(M.MantisIcalibResult), st]
    L.hc_rcalib_seq_robust.argtypes = seq + [C.POINTER(M.MantisRcalibParams), rp, vp,
                                             C.POINTER(M.MantisRcalibResult), st]
    L.hc_calib_end_pass_robust.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, cd, vp,
                                           C.POINTER(M.MantisCalibResult), vp]
    L.hc_icalib_end_pass_robust.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, cd, vp,
                                            C.POINTER(M.MantisIcalibResult), vp]
    L.hc_rcalib_end_pass_robust.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, cd, vp,
                                            C.POINTER(M.MantisRcalibResult), vp]
    for f in (L.hc_calib_seq_robust, L.hc_icalib_seq_robust, L.hc_rcalib_seq_robust):
        f.restype = None
    for f in (L.hc_calib_end_pass_robust, L.hc_icalib_end_pass_robust, L.hc_rcalib_end_pass_robust,
              L.hc_sizeof_calib_robust_stats):
        f.restype = ci
    return L


robust_params = RB.robust_params


def float_kd(K, D):
    """(fx, fy, cx, cy, k1..k4) with K rounded to float, as every calibration starts."""
    kd = IR.kd_of(K, D)
    kd[:4] = kd[:4].astype(np.float32).astype(np.float64)
    return kd


class Spec:
    """One calibration problem: its kind and masks. ext: free_ext; int: free_int and param_mask; rig: all three."""

    def __init__(self, kind, free_ext=0, free_int=0, param_mask=0xFF, min_obs_cam=None):
        assert kind in KINDS
        self.kind, self.index = kind, KINDS.index(kind)
        self.fe = free_ext if kind != "int" else 0
        self.fi = free_int if kind != "ext" else 0
        self.pm = param_mask if kind != "ext" else 0
        self.min_obs_cam = min_obs_cam
        self.ref = {"ext": CR, "int": IR, "rig": RC}[kind]
        self.ROW, self.ACC = {"ext": (13, 91), "int": (15, 120), "rig": (21, 231)}[kind]
        self.TRI = np.triu_indices(self.ROW)

    # the kind's own params struct
    def kparams(self):
        if self.kind == "ext":
            return CR.calib_params(self.fe, self.min_obs_cam)
        if self.kind == "int":
            return IR.icalib_params(self.fi, self.pm, self.min_obs_cam)
        return RC.rcalib_params(self.fe, self.fi, self.pm, self.min_obs_cam)

    def free_any(self):
        return self.fe | self.fi

    # ---- host rules ----
    def obs(self, T, E, kd, img, lm, f, c, p):
        """(codes, Sw, Skw, rows [n_cand, ROW], tie) of camera c at pose T, extrinsic E, intrinsics kd [8]."""
        X, nw, nr, ng = lm
        kw = {"R": p.half_window, "white_thresh": p.white_thresh, "min_weight": p.min_weight}
        if self.kind == "ext":
            return CR.obs(T, E, IR.K_of(kd), kd[4:], img, X, nw, nr, ng, f, self.fe >> c & 1, **kw)
        if self.kind == "int":
            return IR.obs(T, E, kd, img, X, nw, nr, ng, f, self.fi >> c & 1, self.pm, **kw)
        return RC.obs(T, E, kd, img, X, nw, nr, ng, f, self.fe >> c & 1, self.fi >> c & 1, self.pm, **kw)

    def obs_all(self, Ts, exts, kds, frames, lm, p):
        """One pass's slots on the host: codes, Sw, Skw [N, C, n_cand], rows [N, C, n_cand, ROW], tie."""
        f = RR.flags(lm[0], p.landmark_pitch)
        out = [[self.obs(Ts[r], exts[c], kds[c], frames[r][c], lm, f, c, p) for c in range(len(exts))]
               for r in range(len(Ts))]
        return tuple(np.array([[cam[i] for cam in view] for view in out]) for i in range(5))

    def accumulate(self, rows):
        return self.ref.accumulate(rows)

    def np_acc(self, rows):
        """(M^T M's upper triangle in numpy sums, those sums' own rounding bound n 2^-53 |M|^T |M|)."""
        M = np.asarray(rows, np.float64).reshape(-1, self.ROW)
        return (M.T @ M)[self.TRI], (len(M) * 2.0 ** -53 * (np.abs(M).T @ np.abs(M)))[self.TRI]

    def new_result(self, exts, kds, N):
        if self.kind == "ext":
            return CR.new_result(exts, self.fe, N)
        if self.kind == "int":
            return IR.new_result(kds, self.fi, self.pm, N)
        return RC.new_result(exts, kds, self.fe, self.fi, self.pm, N)

    def state_of(self, R, exts, kds):
        """(extrinsics [C, 4, 4], intrinsics [C, 8]) of a result; what the kind does not estimate stays as given."""
        E = np.array(exts) if self.kind == "int" else self.ref.exts_of(R)
        kd = np.array(kds) if self.kind == "ext" else IR.kds_of(R)
        return E, kd

    def end_pass(self, acc, cnt, pos, pass_, I, p, Ts, R):
        """hc_*_end_pass_robust on R (in / out): (finished, T_next [N, 4, 4], delta [N, 6]); pos None: the plain
        gate."""
        acc = np.ascontiguousarray(acc, np.float64)
        cnt = np.ascontiguousarray(cnt, np.int32)
        pos = None if pos is None else np.ascontiguousarray(pos, np.int32)
        N, Cn = cnt.shape
        T = np.ascontiguousarray(np.array(Ts, np.float64).reshape(N, 16)).copy()
        d = np.zeros((N, 6))
        moc = self.kparams().min_obs_cam
        head = (acc.ctypes.data, cnt.ctypes.data, None if pos is None else pos.ctypes.data, N, Cn)
        tail = (pass_, I, p.min_obs, moc, p.lambda_, T.ctypes.data, C.byref(R), d.ctypes.data)
        L = hc()
        if self.kind == "ext":
            fin = L.hc_calib_end_pass_robust(*head, self.fe, *tail)
        elif self.kind == "int":
            fin = L.hc_icalib_end_pass_robust(*head, self.fi, self.pm, *tail)
        else:
            fin = L.hc_rcalib_end_pass_robust(*head, self.fe, self.fi, self.pm, *tail)
        return bool(fin), T.reshape(N, 4, 4), d

    def np_normal(self, acc, lam=0.0):
        if self.kind == "ext":
            return CR.np_normal(acc, self.fe, lam)
        if self.kind == "int":
            return IR.np_normal(acc, self.fi, self.pm, lam)
        return RC.np_normal(acc, self.fe, self.fi, self.pm, lam)

    def steps(self, R, pass_, Cn):
        """The result's camera steps of a pass in the order of the full system's camera unknowns."""
        if self.kind == "rig":
            return RC.steps_of(R, pass_, self.fe, self.fi, Cn)
        fl = [c for c in range(Cn) if self.free_any() >> c & 1]
        return np.array([list(R.delta_cam[pass_][c]) for c in fl]).reshape(-1)

    def seq(self, T_in, exts, kds, frames, lm, p, rb):
        """hc_*_seq_robust: (T_out [N, 4, 4], the kind's result, MantisCalibRobustStats). rb None = NULL."""
        import mantis_amd as M

        X, nw, nr, ng = lm
        N, Cn = len(frames), len(exts)
        h, w = frames[0][0].shape[:2]
        T = np.ascontiguousarray(np.array(T_in, np.float64).reshape(N, 16))
        E = np.ascontiguousarray(np.array(exts, np.float64).reshape(Cn, 16))
        Ks = np.ascontiguousarray(np.array([IR.K_of(kd) for kd in kds], np.float64).reshape(Cn, 9))
        Ds = np.ascontiguousarray(np.array([kd[4:] for kd in kds], np.float64).reshape(Cn, 4))
        keep = [np.ascontiguousarray(frames[r][c], np.uint8) for r in range(N) for c in range(Cn)]
        ptrs = (C.c_void_p * (N * Cn))(*[k.ctypes.data for k in keep])
        T_out = np.zeros((N, 4, 4))
        out = {"ext": M.MantisCalibResult, "int": M.MantisIcalibResult, "rig": M.MantisRcalibResult}[self.kind]()
        st = M.MantisCalibRobustStats()
        kp = self.kparams()
        fn = getattr(hc(), {"ext": "hc_calib_seq_robust", "int": "hc_icalib_seq_robust",
                            "rig": "hc_rcalib_seq_robust"}[self.kind])
        fn(T.ctypes.data, E.ctypes.data, Ks.ctypes.data, Ds.ctypes.data, ptrs, N, Cn, w, h, X.ctypes.data, nw, nr, ng,
           C.byref(p), C.byref(kp), None if rb is None else C.byref(rb), T_out.ctypes.data, C.byref(out), C.byref(st))
        return T_out, out, st

    def plain_seq(self, T_in, exts, kds, frames, lm, p):
        """hc_*_seq, the plain call: (T_out, result)."""
        Ks, Ds = [IR.K_of(kd) for kd in kds], [kd[4:] for kd in kds]
        if self.kind == "ext":
            return CR.seq(T_in, exts, frames, lm, p, self.kparams(), Ks, Ds)
        return self.ref.seq(T_in, exts, Ks, Ds, frames, lm, p, self.kparams())

    # ---- the device ----
    def images(self, frames, exts, kds):
        import mantis_amd as M

        return [M.make_image(f, IR.K_of(kds[c]), kds[c][4:], T_base_cam=exts[c]) for fr in frames
                for c, f in enumerate(fr)]

    def calibrate(self, m, images, N, T0, **params):
        kw = {} if self.min_obs_cam is None else {"min_obs_cam": self.min_obs_cam}
        if self.kind == "ext":
            return m.calibrate_extrinsics(images, N, np.array(T0), self.fe, **kw, **params)
        if self.kind == "int":
            return m.calibrate_intrinsics(images, N, np.array(T0), self.fi, param_mask=self.pm, **kw, **params)
        return m.calibrate_rig(images, N, np.array(T0), self.fe, self.fi, param_mask=self.pm, **kw, **params)

    def record(self, m, r, k, exts, kds):
        """(T, E [C, 4, 4], KD [C, 8], codes, Sw, Skw, rows, acc [C, ACC]) of view r, pass k; what the kind does
        not record is the call's input."""
        if self.kind == "ext":
            T, E, codes, Sw, Skw, rows, acc = m.calib_record(r, k)
            return T, E, np.array(kds), codes, Sw, Skw, rows, acc
        if self.kind == "int":
            T, KD, codes, Sw, Skw, rows, acc = m.icalib_record(r, k)
            return T, np.array(exts), KD, codes, Sw, Skw, rows, acc
        return m.rcalib_record(r, k)


def call_weights(codes, Sw, Skw, rb):
    """hc_linecal_robust_weights over one pass's slots [N, C, n_cand]: {"keys", "w" (as the input's shape),
    "median", "scale", "n_obs", "n_down", "n_zero", "n_pos", "sum_w", "cell_down", "cell_zero" [N, C] int,
    "cell_sum_w" [N, C]}."""
    codes = np.ascontiguousarray(codes, np.int32)
    Sw = np.ascontiguousarray(Sw, np.int32)
    Skw = np.ascontiguousarray(Skw, np.int32)
    N, Cn, nc = codes.shape
    keys = np.zeros(max(codes.size, 1), np.uint32)
    w = np.zeros(max(codes.size, 1))
    med = C.c_uint32()
    scale, sum_w = C.c_double(), C.c_double()
    counts = np.zeros(4, np.int32)
    cc = np.zeros((N, Cn, 2), np.int32)
    cw = np.zeros((N, Cn))
    hc().hc_linecal_robust_weights(codes.ctypes.data, Sw.ctypes.data, Skw.ctypes.data, N, Cn, nc, rb.loss, rb.tuning,
                                   rb.scale_floor, keys.ctypes.data, w.ctypes.data, C.addressof(med),
                                   C.addressof(scale), counts.ctypes.data, C.addressof(sum_w), cc.ctypes.data,
                                   cw.ctypes.data)
    return {"keys": keys[:codes.size].reshape(codes.shape), "w": w[:codes.size].reshape(codes.shape),
            "median": med.value, "scale": scale.value, "n_obs": int(counts[0]), "n_down": int(counts[1]),
            "n_zero": int(counts[2]), "n_pos": int(counts[3]), "sum_w": sum_w.value, "cell_down": cc[:, :, 0].copy(),
            "cell_zero": cc[:, :, 1].copy(), "cell_sum_w": cw}


def tally(cell_down, cell_zero, cell_sum_w, cnt, pass_, median, sigma, st=None):
    """hc_linecal_robust_tally into st (a fresh MantisCalibRobustStats by default)."""
    import mantis_amd as M

    st = st or M.MantisCalibRobustStats()
    cc = np.ascontiguousarray(np.stack([cell_down, cell_zero], axis=-1), np.int32)
    cw = np.ascontiguousarray(cell_sum_w, np.float64)
    cnt = np.ascontiguousarray(cnt, np.int32)
    N, Cn = cnt.shape
    hc().hc_linecal_robust_tally(cc.ctypes.data, cw.ctypes.data, cnt.ctypes.data, N, Cn, pass_, int(median),
                                 float(sigma), C.byref(st))
    return st


def np_call_weights(codes, Sw, Skw, rb):
    """The rule of include/mantis.h over all slots of the call in Python integers and numpy:
    (keys, weights, median, sigma), keys and weights shaped as the input."""
    shape = np.shape(codes)
    cd, sw, skw = (np.asarray(a).reshape(-1) for a in (codes, Sw, Skw))
    keys = RB.keys_of(cd, sw, skw)
    w, m, sigma = RB.np_weights(keys, cd, rb.loss, rb.tuning, rb.scale_floor)
    return keys.reshape(shape), w.reshape(shape), m, sigma


# ---- scenes ----
def knock():
    """The knocked camera's displacement of the base pose: 3 cm along y and 1 degree about z."""
    d = np.eye(4)
    d[:3, :3] = synth.rot_z(math.radians(1.0))
    d[:3, 3] = [0.0, 0.03, 0.0]
    return d


@functools.lru_cache(maxsize=None)
def knocked_frames(d_key="knock"):
    """RB.rigs4()'s frames with view 1, camera 3 rendered from Twb[1] @ d @ ext[3] (the same frame seed)."""
    sc = RB.rigs4()
    d = knock() if d_key == "knock" else RB.drift()
    out = [list(fr) for fr in sc["frames"]]
    Twc = sc["Twb"][KNOCK_VIEW] @ d @ sc["ext"][KNOCK_CAM]
    out[KNOCK_VIEW][KNOCK_CAM] = synth.render_host(synth.make_cam(Twc[:3, :3], Twc[:3, 3], RR.W, RR.H_),
                                                   synth.frame_seed(12, 100 * KNOCK_VIEW + KNOCK_CAM))
    return out


def knocked_scene(clean=False, d_key="knock"):
    """Three views of the four-camera rig at its nominal (true) extrinsics and intrinsics, one frame knocked
    (clean: none): {"ext", "kd" [C, 8], "Twb", "frames" [r][c], "T0" (the truth moved by 2 cm / 1 degree)}."""
    sc = RB.rigs4()
    K, D = synth.intrinsics(RR.W, RR.H_)
    return {"ext": [np.array(e) for e in sc["ext"]], "kd": np.tile(float_kd(K, D), (4, 1)), "Twb": list(sc["Twb"]),
            "frames": [list(fr) for fr in sc["frames"]] if clean else knocked_frames(d_key),
            "T0": [RR.shift(T) for T in sc["Twb"]]}


def ext_errors(E, sc):
    """Translation distance (m) of every extrinsic to the scene's."""
    return [RR.pose_dist(np.array(E[c]), np.array(sc["ext"][c]))[0] for c in range(len(sc["ext"]))]


def pose_errors(T, sc):
    return [RR.pose_dist(np.array(T[r]), np.array(sc["Twb"][r]))[0] for r in range(len(sc["Twb"]))]


def model_scene(kind, clean=False):
    """The perturbed-model scene of the kind's own tests (IR.gap_scene / RC.joint_scene) with the same frame
    knocked: view 1, camera 3 rendered from Twb[1] @ knock @ its true extrinsic through its true lens."""
    sc = dict(IR.gap_scene() if kind == "int" else RC.joint_scene())
    sc["ext_true"] = sc.get("ext_true", sc["ext"])
    sc["frames"] = [list(fr) for fr in sc["frames"]]
    if not clean:
        Twc = sc["Twb"][KNOCK_VIEW] @ knock() @ sc["ext_true"][KNOCK_CAM]
        sc["frames"][KNOCK_VIEW][KNOCK_CAM] = IR._render(Twc, sc["kd_true"][KNOCK_CAM],
                                                               synth.frame_seed(12, 100 * KNOCK_VIEW + KNOCK_CAM))
    sc["kd"] = np.array([float_kd(IR.K_of(k), k[4:]) for k in sc["kd0"]])
    return sc


def margin(fig, plain):
    """The bound for a robust figure the host build measured: the figure plus a quarter of its distance to the
    plain form's."""
    return fig + 0.25 * (plain - fig)


# What the host build measured on model_scene() at 10 iterations, camera 3: {kind: {loss: (model gap px,
# extrinsic cm)}} (tests/test_calib_robust_host.py asserts the plain figures to 0.001).
MODEL_FIGURES = {"int": {None: (0.697, None), "huber": (0.274, None), "tukey": (0.131, None)},
                 "rig": {None: (5.446, 1.799), "huber": (1.705, 0.500), "tukey": (0.229, 0.160)}}
