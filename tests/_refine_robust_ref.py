"""Robust rows of the line refinement, test side: ctypes bindings of the host
build's hc_refine_robust_* (mantis_amd/csrc/mk_refine.h through
build/libmantis_hostcheck.so), the rule of include/mantis.h restated in Python
integers and numpy, and the contaminated rigs the CPU and GPU tests share.
"""
import ctypes as C
import functools
import math

import numpy as np

import _refine_ref as RR
from mantis_amd import synth

KEY_UNIT = 1 << 20
HUBER, TUKEY = 1, 2
LOSSES = {"huber": HUBER, "tukey": TUKEY}
SW_MAX = 31 * 195075  # a full window of the largest weight


def hc():
    import mantis_amd as M

    L = RR.hc()
    vp = C.c_void_p
    L.hc_refine_robust_key.argtypes = [C.c_int32, C.c_int32]
    L.hc_refine_robust_key.restype = C.c_uint32
    L.hc_refine_robust_weights.argtypes = [vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, vp, vp, vp, vp, vp]
    L.hc_refine_robust_weights.restype = None
    L.hc_refine_seq_robust.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(M.MantisRefineParams), C.POINTER(M.MantisRefineRobustParams),
                                       C.POINTER(M.MantisRefineResult), C.POINTER(M.MantisRefineRobustStats)]
    L.hc_refine_seq_robust.restype = None
    L.hc_refine_end_pass_robust.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                            C.POINTER(M.MantisRefineResult)]
    L.hc_refine_end_pass_robust.restype = C.c_int
    return L


def robust_params(loss, **kw):
    """mantis_default_refine_robust_params(loss), then the overrides."""
    import mantis_amd as M

    p = M.MantisRefineRobustParams()
    M.lib().mantis_default_refine_robust_params(LOSSES.get(loss, loss), C.byref(p))
    for k, v in kw.items():
        assert k in ("tuning", "scale_floor"), k
        setattr(p, k, v)
    return p


def key(Sw, Skw):
    return int(hc().hc_refine_robust_key(int(Sw), int(Skw)))


def py_key(Sw, Skw):
    """floor(|Skw| 2^20 / Sw) in Python's integers."""
    return (abs(int(Skw)) << 20) // int(Sw)


def keys_of(codes, Sw, Skw):
    """The rule applied to recorded slots: the key of every code-0 slot, 0 elsewhere (Python integers)."""
    return np.array([py_key(s, k) if c == 0 else 0 for c, s, k in zip(codes, Sw, Skw)], np.uint32)


def weights(keys, codes, rb):
    """hc_refine_robust_weights: {"w", "median", "scale", "n_obs", "n_down", "n_zero", "n_pos", "sum_w"}."""
    keys = np.ascontiguousarray(keys, np.uint32)
    n = len(keys)
    cd = None if codes is None else np.ascontiguousarray(codes, np.int32)
    w = np.zeros(max(n, 1))
    med = C.c_uint32()
    scale, sum_w = C.c_double(), C.c_double()
    counts = np.zeros(4, np.int32)
    hc().hc_refine_robust_weights(keys.ctypes.data, None if cd is None else cd.ctypes.data, n, rb.loss, rb.tuning,
                                  rb.scale_floor, w.ctypes.data, C.addressof(med), C.addressof(scale),
                                  counts.ctypes.data, C.addressof(sum_w))
    return {"w": w[:n], "median": med.value, "scale": scale.value, "n_obs": int(counts[0]), "n_down": int(counts[1]),
            "n_zero": int(counts[2]), "n_pos": int(counts[3]), "sum_w": sum_w.value}


def py_median(keys, codes=None):
    live = sorted(int(k) for i, k in enumerate(keys) if codes is None or codes[i] == 0)
    return live[(len(live) - 1) // 2] if live else 0


def np_weights(keys, codes, loss, tuning, scale_floor):
    """The rule of include/mantis.h in numpy: (weights with 0 in rejected slots, median, sigma)."""
    keys = np.asarray(keys, np.uint32)
    live = np.ones(len(keys), bool) if codes is None else np.asarray(codes) == 0
    m = py_median(keys, None if codes is None else codes)
    sigma = max(1.4826 * (float(m) / KEY_UNIT), scale_floor)
    t = (keys.astype(np.float64) / KEY_UNIT) / (tuning * sigma)
    if loss == HUBER:
        w = np.where(t <= 1.0, 1.0, 1.0 / np.maximum(t, 1e-300))
    else:
        w = np.where(t < 1.0, (1.0 - t * t) ** 2, 0.0)
    return np.where(live, w, 0.0), m, sigma


def seq_robust(T_in, exts, imgs, X, nw, nr, ng, p, rb, K=None, D=None):
    """hc_refine_seq_robust on one rig: (MantisRefineResult, MantisRefineRobustStats); rb None = NULL."""
    import mantis_amd as M

    Cn = len(imgs)
    h, w = imgs[0].shape[:2]
    if K is None:
        K, D = synth.intrinsics(w, h)
    T = np.ascontiguousarray(T_in, np.float64)
    E = np.ascontiguousarray(np.array(exts, np.float64).reshape(Cn, 16))
    Ks, Ds = RR.per_camera(K, D, Cn)
    keep = [np.ascontiguousarray(i, np.uint8) for i in imgs]
    ptrs = (C.c_void_p * Cn)(*[k.ctypes.data for k in keep])
    out, st = M.MantisRefineResult(), M.MantisRefineRobustStats()
    hc().hc_refine_seq_robust(T.ctypes.data, E.ctypes.data, Ks.ctypes.data, Ds.ctypes.data, ptrs, Cn, w, h,
                              X.ctypes.data, nw, nr, ng, C.byref(p), None if rb is None else C.byref(rb),
                              C.byref(out), C.byref(st))
    return out, st


def drift():
    """The displacement of the contaminated camera's base pose: 0.4 degrees about z and 1.2 cm along y."""
    d = np.eye(4)
    d[:3, :3] = synth.rot_z(math.radians(0.4))
    d[:3, 3] = [0.0, 0.012, 0.0]
    return d


@functools.lru_cache(maxsize=None)
def rigs4():
    """RR.rig_scene(4, 3), rendered once per session."""
    return RR.rig_scene(4, 3)


@functools.lru_cache(maxsize=None)
def contaminated_rigs4(cam=3, cfg=12):
    """rigs4() with camera 3's frame rendered from Twb @ drift() (the same frame
    seed): a camera whose extrinsic has drifted. The frames of rig r, a list."""
    sc = rigs4()
    out = []
    for r, T in enumerate(sc["Twb"]):
        fr = list(sc["frames"][r])
        Twc = T @ drift() @ sc["ext"][cam]
        fr[cam] = synth.render_host(synth.make_cam(Twc[:3, :3], Twc[:3, 3], RR.W, RR.H_),
                                    synth.frame_seed(cfg, 100 * r + cam))
        out.append(fr)
    return out
