"""The workspaces a context grows on demand (csrc/hostbuf.h): a call that needs
more than the context holds frees and reallocates, carries nothing over, and
the calls around it do not notice. Per family one context takes a small, a
large and the small call again, "large" beyond every capacity the small call
set, and every output byte is compared with the same three calls made on three
fresh contexts. Then three create / one-small-call-per-family / destroy cycles
in one process, which must not lower the device's free memory.

The smallest shapes: the 130 x 35 cell of tests/_line_cases.py, 2 cameras,
1 -> 3 -> 1 rigs or views, 2 iterations, windows of 2 -> 4 -> 2 views. An
allocation failure is not provoked here (tools/bufcheck_main.cpp covers the
rule of grow on the CPU).

ensure_gauss grows only under a camera-sharded call of several ranks (one
context's frames stay within max_cams); `process` and the one-rank sharded
call below run through it and regrow the exchange buffers.
"""
import ctypes as C

import numpy as np
import pytest

import _line_cases as LC
import _refine_ref as RR
from mantis_amd import synth

pytestmark = pytest.mark.gpu

W, H = 130, 35
CAMS = 2
SEED = 0x9E3779B97F4A7C15
LINE = dict(iterations=2, half_window=2)


def _ctx(landmark_map, max_cams=8, **cfg):
    import mantis_amd as M

    m = M.Mantis(M.default_config(max_cams=max_cams, max_width=W, max_height=H, **cfg))
    m.set_map(*landmark_map)
    return m


def _blob(x):
    """Every byte of an output: ctypes records whole, arrays as they lie, containers in order."""
    if isinstance(x, (C.Structure, C.Array)):
        return bytes(x)
    if isinstance(x, np.ndarray):
        return x.tobytes()
    if isinstance(x, dict):
        return b"".join(_blob(v) for v in x.values())
    if isinstance(x, (list, tuple)):
        return b"".join(_blob(v) for v in x)
    return repr(x).encode()


def _regrow(landmark_map, calls, setup=None, fresh_calls=None, **ctx_kw):
    """calls: small, large, small. One context through all three against a fresh context each (fresh_calls: what
    the fresh contexts run in their place)."""
    def make():
        m = _ctx(landmark_map, **ctx_kw)
        if setup:
            setup(m)
        return m

    shared = make()
    try:
        got = [_blob(f(shared)) for f in calls]
    finally:
        shared.close()
    for k, f in enumerate(fresh_calls or calls):
        m = make()
        try:
            want = _blob(f(m))
        finally:
            m.close()
        assert len(want) > 0
        assert got[k] == want, f"call {k} of the sequence differs from the same call on a fresh context"
    assert got[0] == got[2]


@pytest.fixture(scope="module")
def rigs():
    """Four views of a two-camera bench rig at 130 x 35: (exts, kds, Twb [4], frames [4][2]); a view doubles as
    a rig of a batch."""
    return LC._rig(["bench"] * CAMS, W, H, LC.SEED0, 900, n_views=4)


def _images(rigs, views):
    import mantis_amd as M

    exts, kds, _, frames = rigs
    return [M.make_image(frames[v][c], LC.IR.K_of(kds[c]), kds[c][4:], T_base_cam=exts[c])
            for v in views for c in range(CAMS)]


def _starts(rigs, views):
    return np.array([RR.shift(rigs[2][v]) for v in views])


SEQ = [[0], [1, 2, 3], [0]]  # the views (rigs) of the small, the large and the small call


def test_track_batch(landmark_map, rigs):
    def call(views):
        def f(m):
            m.rng_state = SEED
            res = m.track_batch(_images(rigs, views), len(views), _starts(rigs, views), particles=4 * len(views),
                                iterations=2, record=1)
            return res, [m.track_record(r, it) for r in range(len(views)) for it in (-1, 1, 2)]
        return f

    _regrow(landmark_map, [call(v) for v in SEQ])


@pytest.mark.parametrize("record", [0, 1])
@pytest.mark.parametrize("loss", [None, "huber"])
def test_refine_batch(landmark_map, rigs, loss, record):
    def call(views, rec):
        def f(m):
            res = m.refine_batch(_images(rigs, views), len(views), _starts(rigs, views), record=rec, **LINE)
            out = [res]
            if loss:
                out.append([m.refine_robust_stats(r) for r in range(len(views))])
            if rec:
                for r, rr in enumerate(res):
                    for p in range(rr.iterations_run + 1):
                        out.append(m.refine_record(r, p))
                        if loss:
                            out.append(m.refine_robust_record(r, p))
            return out
        return f

    _regrow(landmark_map, [call(SEQ[0], 0), call(SEQ[1], record), call(SEQ[2], 0)],
            setup=(lambda m: m.set_refine_robust(loss)) if loss else None)


CALIB_SEQ = [[0, 1], [0, 1, 2, 3], [0, 1]]  # a calibration needs two views; the large one takes four


@pytest.mark.parametrize("loss", [None, "huber"])
@pytest.mark.parametrize("kind", LC.KINDS)
def test_calibrate(landmark_map, rigs, kind, loss):
    fe, fi = LC.free_of(kind, CAMS)

    def call(views, rec):
        def f(m):
            imgs, T0 = _images(rigs, views), _starts(rigs, views)
            if kind == "ext":
                T, res = m.calibrate_extrinsics(imgs, len(views), T0, fe, record=rec, **LINE)
                record = m.calib_record
            elif kind == "int":
                T, res = m.calibrate_intrinsics(imgs, len(views), T0, fi, record=rec, **LINE)
                record = m.icalib_record
            else:
                T, res = m.calibrate_rig(imgs, len(views), T0, fe, fi, record=rec, **LINE)
                record = m.rcalib_record
            out = [T, res]
            if loss:
                out.append(m.calib_robust_stats(kind))
            if rec:
                for v in range(len(views)):
                    for p in range(res.iterations_run + 1):
                        out.append(record(v, p))
                        if loss:
                            out.append(m.calib_robust_record(kind, v, p))
            return out
        return f

    _regrow(landmark_map, [call(CALIB_SEQ[0], 0), call(CALIB_SEQ[1], 1), call(CALIB_SEQ[2], 0)],
            setup=(lambda m: m.set_calib_robust(loss)) if loss else None)


def test_smooth_batch(landmark_map, rigs):
    def call(views, rec):
        def f(m):
            N = len(views)
            Twb = rigs[2]
            mo = np.zeros((N - 1, 7))
            for k in range(N - 1):  # the true step between the views: delta_pos | delta_quat_xyzw
                d = np.linalg.inv(Twb[views[k]]) @ Twb[views[k + 1]]
                mo[k, :3] = d[:3, 3]
                w = 0.5 * np.sqrt(max(0.0, 1.0 + np.trace(d[:3, :3])))
                mo[k, 3:] = [(d[2, 1] - d[1, 2]) / (4 * w), (d[0, 2] - d[2, 0]) / (4 * w),
                             (d[1, 0] - d[0, 1]) / (4 * w), w]
            res, vw = m.smooth_batch(_images(rigs, views), 1, N, _starts(rigs, views), mo, record=rec, **LINE)
            out = [res, vw]
            if rec:
                for p in range(res[0].iterations_run + 1):
                    out.append(m.smooth_pass_record(0, p))
                    out += [m.smooth_record(0, v, p) for v in range(N)]
            return out
        return f

    _regrow(landmark_map, [call(CALIB_SEQ[0], 0), call(CALIB_SEQ[1], 1), call(CALIB_SEQ[2], 0)])


def test_mcl(landmark_map, rigs):
    N = 64

    def call(n, color):
        def f(m):
            m.rng_state = SEED
            m.mcl_set_color(color)
            m.mcl_init(rigs[2][0], 0.02, 0.02, n_particles=n, record=1)
            step = m.mcl_step(_images(rigs, [0]))
            out = [step, m.mcl_modes(), m.mcl_particles(), m.mcl_record()]
            if color:
                out += [m.mcl_color_record(), m.mcl_modes_color()]
            return out
        return f

    _regrow(landmark_map, [call(N, 0), call(4 * N, 2), call(N, 0)])


def _hyps(rigs, n_particles):
    from mantis_amd import dense

    Twc = rigs[2][0] @ rigs[0][0]
    return dense.config5_hypotheses(Twc[:3, :3], Twc[:3, 3], np.random.default_rng(5), n_particles=n_particles)


def test_score_argmin(landmark_map, rigs):
    def call(n_particles):
        return lambda m: m.score_argmin(_images(rigs, [0])[0], _hyps(rigs, n_particles), 7)

    _regrow(landmark_map, [call(1), call(3), call(1)])


def test_score_argmin_batch(landmark_map, rigs):
    def call(views, n_particles):
        def f(m):
            imgs = _images(rigs, views)
            h = np.ascontiguousarray(_hyps(rigs, n_particles), np.float64)
            ptrs = [m.device_alloc(h.nbytes) for _ in imgs]
            try:
                for p in ptrs:
                    m.h2d(p, h)
                return m.score_argmin_batch(imgs, ptrs, [len(h)] * len(imgs), list(range(len(imgs))))
            finally:
                for p in ptrs:
                    m.device_free(p)
        return f

    _regrow(landmark_map, [call([0], 1), call([1, 2, 3], 3), call([0], 1)])


@pytest.mark.parametrize("sharded", [False, True])
def test_process(landmark_map, rigs, sharded):
    """Batches of 2 -> 6 -> 2 frames, plain and through the one-rank sharded call (its exchange buffers grow
    with the rig count), with the rig weighting's job buffers on. A one-rank sharded call returns what the plain
    call returns, and a communicator costs seconds: the fresh contexts of the sharded case make the plain call."""
    def call(views, sharded):
        def f(m):
            m.rng_state = SEED
            if sharded:
                if not getattr(m, "_has_comm", False):
                    m.comm_init(0, 1)
                    m._has_comm = True
                out = m.process_sharded(_images(rigs, views), len(views), list(range(CAMS)), CAMS)
            else:
                out = m.process(_images(rigs, views), len(views))
            rig_out, cam_out = out
            # a frame that ends before scoring (no quadrilateral in these small frames) gets its six counters
            # and nothing else written: the rest of its record is whatever the buffer held
            cams = [r if r.publish else [r.status, r.reason, r.publish, r.n_quads, r.n_hyps, r.n_scored]
                    for r in cam_out]
            return [rig_out, cams, [m.rig_weights(r) for r in range(len(views))], m.rng_state]
        return f

    _regrow(landmark_map, [call(v, sharded) for v in SEQ], fresh_calls=[call(v, False) for v in SEQ], rig_weighting=1,
            particles=4, iterations=2)


def _one_of_each(landmark_map, rigs):
    m = _ctx(landmark_map, rig_weighting=1, particles=4, iterations=2)
    try:
        one, two = [0], [0, 1]
        m.process(_images(rigs, one), 1)
        m.track_batch(_images(rigs, one), 1, _starts(rigs, one), particles=4, iterations=2)
        m.set_refine_robust("huber")
        m.refine_batch(_images(rigs, one), 1, _starts(rigs, one), **LINE)
        m.set_calib_robust("huber")
        fe, fi = LC.free_of("rig", CAMS)
        m.calibrate_extrinsics(_images(rigs, two), 2, _starts(rigs, two), fe, **LINE)
        m.calibrate_intrinsics(_images(rigs, two), 2, _starts(rigs, two), fi, **LINE)
        m.calibrate_rig(_images(rigs, two), 2, _starts(rigs, two), fe, fi, **LINE)
        m.smooth_batch(_images(rigs, two), 1, 2, _starts(rigs, two), np.zeros((1, 7)), **LINE)
        m.mcl_set_color(2)
        m.mcl_init(rigs[2][0], 0.02, 0.02, n_particles=64)
        m.mcl_step(_images(rigs, one))
        m.mcl_modes()
        m.score_argmin(_images(rigs, one)[0], _hyps(rigs, 1))
    finally:
        m.close()


def test_no_leak_over_context_cycles(landmark_map, rigs):
    """Free device memory after the first and after the third create / one small call per family / destroy
    cycle: no drop. Measured before this file's buffers existed (raw pointers, hand-kept free lists): 0 bytes."""
    import torch

    free = []
    for _ in range(3):
        _one_of_each(landmark_map, rigs)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    print(f"free device memory after cycles 1..3: {free}")
    assert free[2] >= free[0], f"free device memory fell by {free[0] - free[2]} bytes over two cycles"
