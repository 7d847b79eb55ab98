"""The fixed-lag window on the GPU (mantis_lag_*): every push against
mantis_smooth_batch over the views it holds (the same kernels on the same bytes:
equal bytes), the marginal against the host rule fed the device's own record,
the predicted start, broken chains, a failed window, the frame kinds, the other
entries in between, the launch count, the argument errors, and the accuracy
scene against two batch calls. 322 x 242 views (tests/_lag_ref.py,
tests/_smooth_ref.py).
"""
import ctypes as C

import numpy as np
import pytest

import _lag_ref as LR
import _refine_ref as RR
import _smooth_ref as SR
from mantis_amd import synth

pytestmark = pytest.mark.gpu

SW, SH = LR.SW, LR.SH


@pytest.fixture(scope="module")
def ctx(landmark_map):
    import mantis_amd as M

    m = M.Mantis(max_cams=12, max_width=SW, max_height=SH)
    m.set_map(*landmark_map)
    yield m
    m.close()


@pytest.fixture(scope="module")
def lm(landmark_map):
    return RR.all_landmarks(landmark_map)


@pytest.fixture(scope="module")
def walk6():
    return SR.trajectory(6, n_cams=1, w=SW, h=SH, cfg=19)


@pytest.fixture(scope="module")
def small5():
    return SR.trajectory(5, n_cams=2, w=SW, h=SH, cfg=19)


def _images(frames, exts, pitched=None):
    """test_gpu_smooth.py's helper: MantisImage list of frames[k][c] (view-major); pitched: a list that keeps
    row-padded copies alive (step_bytes = 1000 for the 322-wide frames)."""
    import mantis_amd as M

    h, w = frames[0][0].shape[:2]
    K, D = synth.intrinsics(w, h)
    out = []
    for fr in frames:
        for f, e in zip(fr, exts):
            im = M.make_image(f, K, D, T_base_cam=e)
            if pitched is not None:
                buf = np.full((h, 3 * w + 34), 0xAB, np.uint8)
                buf[:, : 3 * w] = f.reshape(h, 3 * w)
                pitched.append(buf)
                im.bgr = buf.ctypes.data
                im.step_bytes = buf.strides[0]
            out.append(im)
    return out


def _pushes(sc, noise=(0.002, 0.005)):
    """(starts [push], motions [push][7], row 0 unused) of a trajectory, the motions off by `noise`."""
    n = len(sc["frames"])
    return [SR.starts(sc)[k] for k in range(n)], np.concatenate([np.zeros((1, 7)), SR.noisy_motions(sc, *noise)])


def _blob(res, views):
    return bytes(res) + b"".join(bytes(v) for v in views)


def _sequence(m, sc, cap, starts, mo, prior=None, frames=None, check=True, images=None, between=None, **params):
    """mantis_lag_reset, then one push per view. With `check`, every push is compared with mantis_smooth_batch
    over the views it holds: starts = the poses held before the push + the new view's start (the host rule's
    T_newest Delta where none is given), the same motions, and the prior mantis_lag_get_prior gave before the
    push. Returns [(result, views, info)] and the priors read."""
    frames = sc["frames"] if frames is None else frames
    ext = sc["ext"]
    Cn = len(frames[0])
    params.setdefault("iterations", 2)
    params.setdefault("record", 1)
    pT, pC = prior if prior is not None else (None, None)
    m.lag_reset(cap, Cn, pT, pC, **params)
    out, priors, held = [], [], []  # held: frame index of every view in the window
    prev = []
    for q in range(len(frames)):
        pr = m.lag_prior()
        priors.append(pr)
        imgs = images(q) if images is not None else _images([frames[q]], ext)
        res, views, info = m.lag_push(imgs, None if q == 0 else mo[q], starts[q])
        if len(held) == cap:
            held.pop(0)
            prev = prev[1:]
        held.append(q)
        assert info.n_views == len(held) == res.n_views == len(views) and info.pushes == q + 1
        assert info.slid == int(q >= cap) and info.has_prior == res.has_prior
        assert _blob(res, views) == _blob(res, m.lag_views())
        if check:
            start = starts[q] if starts[q] is not None else LR.predict(prev[-1], SR.transform(mo[q])[1])
            T_in = np.array(prev + [np.asarray(start, np.float64).reshape(4, 4)])
            has, T, cov, why = pr
            assert has == bool(res.has_prior) and why == info.drop_reason, (q, has, why, info.drop_reason)
            bres, bviews = m.smooth_batch(_images([frames[k] for k in held], ext), 1, len(held), T_in,
                                          mo[held[0] + 1:q + 1] if len(held) > 1 else None, T if has else None,
                                          cov if has else None, **params)
            assert bytes(bres[0]) == bytes(res), f"push {q}: result"
            for k, (a, b) in enumerate(zip(bviews[0], views)):
                assert bytes(a) == bytes(b), f"push {q}: view {k}"
        if between is not None:
            between(q)
        prev = [LR.pose_of(v) for v in views]
        out.append((res, views, info))
    return out, priors


@pytest.mark.parametrize("cap", [2, 3])
def test_fill_and_slide_equal_batch_calls(ctx, walk6, cap):
    """Pushes 1 .. N fill the window, pushes N + 1 .. slide it: each equals mantis_smooth_batch over the views
    held, with the prior read before the push."""
    starts, mo = _pushes(walk6)
    out, priors = _sequence(ctx, walk6, cap, starts, mo)
    for q, (res, views, info) in enumerate(out):
        assert res.status == 0 and res.smoothed == 1 and info.drop_reason == 0
        assert res.has_prior == int(q >= cap)
    assert [p[0] for p in priors] == [q >= cap for q in range(6)]


def test_two_cameras_and_a_reset_prior(ctx, small5):
    """C = 2, and a prior on the first view: H_00 carries it at the first slide."""
    sc = small5
    starts, mo = _pushes(sc)
    cov = np.diag([4e-4, 4e-4, 9e-4, 1e-3, 1e-3, 2e-3])
    cov[0, 1] = cov[1, 0] = 1e-4
    out, priors = _sequence(ctx, sc, 3, starts, mo, prior=(sc["Twb"][0], cov))
    assert [int(r.has_prior) for r, _, _ in out] == [1] * 5
    assert priors[0][0] and np.array_equal(priors[0][1], sc["Twb"][0]) and np.array_equal(priors[0][2], cov)
    assert not np.array_equal(priors[3][1], sc["Twb"][0])
    plain, _ = _sequence(ctx, sc, 3, starts, mo, check=False)
    assert _blob(*plain[3][:2]) != _blob(*out[3][:2]), "the reset's prior reaches the first slide"


def test_marginal_equals_the_host_rule_on_the_record(ctx, walk6):
    """mantis_lag_get_prior on a full window: hc_lag_marginalize fed the last push's own recorded blocks."""
    starts, mo = _pushes(walk6)
    out, _ = _sequence(ctx, walk6, 3, starts[:5], mo[:5], frames=walk6["frames"][:5], check=False)
    res, views, info = out[-1]
    p = ctx.smooth_params(iterations=2)
    I = res.iterations_run
    assert I == 2 and info.slid == 1 and res.has_prior == 1
    e, J, pe, pJ, delta = ctx.smooth_pass_record(0, I)
    accs = [ctx.smooth_record(0, k, I)[5] for k in range(3)]
    assert pJ.any(), "this window carried a prior itself"
    Hd, Ho, g = SR.assemble(accs, np.ones(2, np.int32), e, J, 0.0, pe, pJ)
    why, Tp, Cov, Wp = LR.marginalize(Hd[0], g[0], J[0, 0], J[0, 1], e[0], LR.pose_of(views[1]), p.sigma_row)
    has, T, cov, reason = ctx.lag_prior()
    assert has and reason == why == 0
    assert T.tobytes() == Tp.tobytes() and cov.tobytes() == Cov.tobytes()
    assert np.array_equal(cov, cov.T)


def test_predicted_start(ctx, walk6):
    """T_start = NULL: the device's T_newest Delta is the host rule's."""
    starts, mo = _pushes(walk6)
    free = [starts[0]] + [None] * 5
    a, _ = _sequence(ctx, walk6, 3, free, mo)
    given = [starts[0]]
    for q in range(1, 6):
        given.append(LR.predict(LR.pose_of(a[q - 1][1][-1]), SR.transform(mo[q])[1]))
    b, _ = _sequence(ctx, walk6, 3, given, mo, check=False)
    assert [_blob(r, v) for r, v, _ in a] == [_blob(r, v) for r, v, _ in b]


def test_chain_breaks(ctx, walk6):
    """An unset motion on the step that becomes step 0: no prior, and the reason; an unset motion into the new
    view: two segments in one window."""
    starts, mo = _pushes(walk6)
    mo2 = mo.copy()
    mo2[1] = SR.UNSET
    mo2[5] = SR.UNSET
    out, priors = _sequence(ctx, walk6, 3, starts, mo2)
    drops = [(i.has_prior, i.drop_reason) for _, _, i in out]
    assert drops == [(0, 0), (0, 0), (0, 0), (0, LR.DROPS["no_factor"]), (1, 0), (1, 0)]
    assert [r.n_factors for r, _, _ in out] == [0, 0, 1, 2, 2, 1]
    assert all(r.status == 0 for r, _, _ in out)


def test_failed_window(ctx, walk6):
    """Capacity 2, all views black: STARVED. The sighted views that follow: no prior from the failed window, and
    the window after is OK."""
    sc = walk6
    starts, mo = _pushes(sc)
    black = [[np.zeros_like(f) for f in fr] for fr in sc["frames"][:2]]
    out, _ = _sequence(ctx, sc, 2, starts[:5], mo[:5], frames=black + sc["frames"][2:5])
    assert [r.status for r, _, _ in out] == [1, 1, 0, 0, 0]
    assert (out[2][2].has_prior, out[2][2].drop_reason) == (0, LR.DROPS["not_ok"])
    assert (out[4][2].has_prior, out[4][2].drop_reason) == (1, 0)
    # the black view that left at push 3 had no prior of its own: its marginal is zero but for rounding
    i3 = out[3][2]
    assert (i3.has_prior, i3.drop_reason) in [(0, LR.DROPS["lambda"]), (0, LR.DROPS["cov"]), (1, 0)]


def test_frame_kinds_and_released_buffers(ctx, small5):
    """Host, pitched (step_bytes = 1000) and device frames: equal bytes; the caller's buffer overwritten after
    every push changes nothing later."""
    import mantis_amd as M

    sc = small5
    ext = sc["ext"]
    starts, mo = _pushes(sc)
    ref, _ = _sequence(ctx, sc, 3, starts, mo, check=False)
    want = [_blob(r, v) for r, v, _ in ref]
    keep = []
    pit, _ = _sequence(ctx, sc, 3, starts, mo, check=False, images=lambda q: _images([sc["frames"][q]], ext, keep))
    assert keep[0].strides[0] == 1000 and [_blob(r, v) for r, v, _ in pit] == want
    K, D = synth.intrinsics(SW, SH)
    fb = SW * SH * 3
    dev = ctx.device_alloc(2 * fb)
    scratch = [np.zeros((SH, SW, 3), np.uint8) for _ in range(2)]
    try:
        def dev_images(q):
            for c in range(2):
                ctx.h2d(dev + c * fb, sc["frames"][q][c])
            return [M.make_image(None, K, D, T_base_cam=ext[c], device_ptr=dev + c * fb, width=SW, height=SH)
                    for c in range(2)]

        # the same two device buffers serve every push: the window keeps its own copies
        got, _ = _sequence(ctx, sc, 3, starts, mo, check=False, images=dev_images)
        assert [_blob(r, v) for r, v, _ in got] == want

        def host_images(q):
            for c in range(2):
                scratch[c][:] = sc["frames"][q][c]
            return _images([scratch], ext)

        def wipe(q):
            for c in range(2):
                scratch[c][:] = 0x5A

        got, _ = _sequence(ctx, sc, 3, starts, mo, check=False, images=host_images, between=wipe)
        assert [_blob(r, v) for r, v, _ in got] == want
    finally:
        ctx.device_free(dev)


def test_other_entries_between_pushes(ctx, small5):
    """mantis_refine_batch, mantis_smooth_batch and mantis_calibrate_extrinsics between the pushes: the pushes'
    bytes and theirs are unchanged; the cv::RNG state and the context's prior pose are untouched; the same
    sequence after another reset gives the same bytes; a reset with another capacity then works."""
    sc = small5
    ext = sc["ext"]
    starts, mo = _pushes(sc)
    flat = _images(sc["frames"][:3], ext)
    T0 = SR.starts(sc)[:3]
    ctx.rng_state = 4242
    prior = sc["Twb"][1].copy()
    ctx.prior_pose = prior

    def others(q=None):
        r = ctx.refine_batch(flat, 3, T0, record=1)
        rec = ctx.refine_record(1, 1)
        s, v = ctx.smooth_batch(flat, 1, 3, T0, mo[1:3], record=1)
        srec = ctx.smooth_record(0, 1, 1)
        Tc, c = ctx.calibrate_extrinsics(flat, 3, T0, 0b10)
        return ([bytes(x) for x in r], [a.tobytes() for a in rec], _blob(s[0], v[0]), [a.tobytes() for a in srec],
                Tc.tobytes(), bytes(c))

    before = others()
    seen = []
    plain, _ = _sequence(ctx, sc, 3, starts, mo, check=False)
    mixed, _ = _sequence(ctx, sc, 3, starts, mo, check=False, between=lambda q: seen.append(others()))
    again, _ = _sequence(ctx, sc, 3, starts, mo, check=False)
    want = [_blob(r, v) for r, v, _ in plain]
    assert [_blob(r, v) for r, v, _ in mixed] == want and [_blob(r, v) for r, v, _ in again] == want
    assert len(seen) == 5 and all(s == before for s in seen)
    assert ctx.rng_state == 4242 and np.array_equal(ctx.prior_pose, prior)
    ctx.prior_pose = None
    # the record follows the last smooth call: a push, then a batch call, then a push again
    T_last = ctx.smooth_record(0, 2, 2)[0]
    assert np.array_equal(T_last, LR.pose_of(again[-1][1][2]))
    other, _ = _sequence(ctx, sc, 4, starts, mo)
    assert [i.n_views for _, _, i in other] == [1, 2, 3, 4, 4] and other[4][2].has_prior == 1
    back, _ = _sequence(ctx, sc, 3, starts, mo, check=False)
    assert [_blob(r, v) for r, v, _ in back] == want


def test_launch_count(walk6, landmark_map):
    """1 + 3 (I + 1) launches per push by the stage marks, sliding or not; mantis_lag_get_prior adds one launch
    of its own on a full window only."""
    import mantis_amd as M

    sc = walk6
    starts, mo = _pushes(sc)
    m = M.Mantis(max_cams=2, max_width=SW, max_height=SH)
    try:
        m.set_map(*landmark_map)
        m.lag_reset(2, 1, iterations=2, record=0)
        m.set_profiling(1)
        for q in range(4):
            m.lag_push(_images([sc["frames"][q]], sc["ext"]), None if q == 0 else mo[q], starts[q])
            names = [n for n, _ in m.kernel_times()]
            kern = [n for n in names if "/k_" in n]
            assert kern[0] == "lag_slide/k_lag_slide" and len(kern) == 1 + 3 * 3, names
            assert [sum(n.startswith(s) for n in kern) for s in ("smooth_obs", "smooth_acc", "smooth_solve")] == [3, 3, 3]
            assert names[0] == "lag_frames" and len(names) == len(kern) + 1
        m.set_profiling(0)
        with pytest.raises(Exception):
            m.smooth_record(0, 0, 0)  # record = 0 kept none
    finally:
        m.close()


def test_argument_errors(ctx, walk6):
    import mantis_amd as M

    L = M.lib()
    sc = walk6
    starts, mo = _pushes(sc)
    imgs = _images([sc["frames"][0]], sc["ext"])
    arr = (M.MantisImage * 1)(*imgs)
    out, info = M.MantisSmoothResult(), M.MantisLagInfo()
    vw = (M.MantisSmoothView * 4)()

    def push(h, cams=arr, motion=None, T=starts[0], res=out, views=vw):
        keep = [None if a is None else np.ascontiguousarray(a, np.float64) for a in (motion, T)]
        st = L.mantis_lag_push(h, cams, *[None if a is None else a.ctypes.data for a in keep],
                               None if res is None else C.byref(res), views, C.byref(info))
        return st, L.mantis_last_error(h).decode()

    fresh = M.Mantis(max_cams=2, max_width=SW, max_height=SH)
    try:
        fresh.set_map(*synth.load_map())
        st, msg = push(fresh.h)
        assert st == 1 and "reset" in msg
        assert L.mantis_lag_get_prior(fresh.h, None, None, None, None) == 1
        nomap = M.Mantis(max_cams=2, max_width=SW, max_height=SH)
        try:
            nomap.lag_reset(2, 1)
            st, msg = push(nomap.h)
            assert st == 1 and "map" in msg
        finally:
            nomap.close()
    finally:
        fresh.close()

    def reset(pT=None, pC=None, edit=None, **kw):
        p = ctx.lag_params(**kw)
        if edit:
            edit(p)
        keep = [None if a is None else np.ascontiguousarray(a, np.float64) for a in (pT, pC)]
        st = L.mantis_lag_reset(ctx.h, C.byref(p), *[None if a is None else a.ctypes.data for a in keep])
        return st, L.mantis_last_error(ctx.h).decode()

    eye = np.eye(6)
    nanT = starts[0].copy()
    nanT[0, 3] = float("nan")
    bad_resets = [
        (dict(capacity=1), "capacity"), (dict(capacity=257), "capacity"), (dict(cams_per_rig=0), "cams_per_rig"),
        (dict(cams_per_rig=9), "cams_per_rig"), (dict(cams_per_rig=8, capacity=2), None),
        (dict(edit=lambda p: setattr(p, "struct_size", 8)), "struct_size"),
        (dict(edit=lambda p: setattr(p.smooth, "struct_size", 8)), "struct_size"),
        (dict(iterations=11), "iterations"), (dict(half_window=0), "half_window"), (dict(min_obs=5), "min_obs"),
        (dict(lambda_=-1.0), "lambda"), (dict(sigma_row=0.0), "sigma_row"), (dict(sigma_t=float("inf")), "sigma_t"),
        (dict(sigma_rot=-1.0), "sigma_rot"), (dict(record=2), "record"), (dict(pT=starts[0]), "prior_cov"),
        (dict(pT=starts[0], pC=np.diag([1.0, 1, 1, 1, 1, -1e-3])), "prior_cov"), (dict(pT=nanT, pC=eye), "prior_T"),
    ]
    ctx.lag_reset(3, 1, iterations=2)
    first, views0, _ = ctx.lag_push(imgs, None, starts[0])
    for kw, word in bad_resets:
        st, msg = reset(**kw)
        if word is None:
            assert st == 0  # within range (max_cams = 12 holds eight cameras); undone below
            ctx.lag_reset(3, 1, iterations=2)
            ctx.lag_push(imgs, None, starts[0])
            continue
        assert st == 1 and word in msg, (kw, st, msg)
    assert L.mantis_lag_reset(ctx.h, None, None, None) == 1

    ctx.rng_state = 77
    ctx.set_profiling(1)
    small = M.make_image(np.zeros((SH - 2, SW - 2, 3), np.uint8), *synth.intrinsics(SW - 2, SH - 2))
    nanM, nanQ = mo[1].copy(), mo[1].copy()
    nanM[1] = float("nan")
    nanQ[5] = float("nan")
    bad_pushes = [
        (dict(cams=None, motion=mo[1]), "null"), (dict(motion=mo[1], res=None), "null"),
        (dict(motion=mo[1], views=None), "null"), (dict(motion=None), "motion"),
        (dict(cams=(M.MantisImage * 1)(small), motion=mo[1]), "size"), (dict(motion=nanM), "delta_pos"),
        (dict(motion=nanQ), "delta_quat"), (dict(motion=mo[1], T=nanT), "T_start"),
        (dict(motion=SR.UNSET, T=None), "T_start"),
    ]
    for kw, word in bad_pushes:
        st, msg = push(ctx.h, **kw)
        assert st == 1 and word in msg, (kw, st, msg)
    n = C.c_int32(0)
    assert L.mantis_lag_get_views(ctx.h, vw, C.byref(n)) == 1
    # nothing was launched and the window is unchanged: the next push is the second view's, its marks its own
    res, views, info = ctx.lag_push(_images([sc["frames"][1]], sc["ext"]), mo[1], None)
    names = [n for n, _ in ctx.kernel_times()]
    ctx.set_profiling(0)
    assert info.pushes == 2 and info.n_views == 2 and len(names) == 11, names
    assert ctx.rng_state == 77
    ctx.lag_reset(3, 1, iterations=2)
    a, va, _ = ctx.lag_push(imgs, None, starts[0])
    assert _blob(a, va) == _blob(first, views0)
    b, vb, _ = ctx.lag_push(_images([sc["frames"][1]], sc["ext"]), mo[1], None)
    assert _blob(b, vb) == _blob(res, views)
    # a first push without a start
    ctx.lag_reset(3, 1, iterations=2)
    st, msg = push(ctx.h, T=None)
    assert st == 1 and "T_start" in msg


def _accuracy(ctx, lm, noisy):
    """The accuracy scene on the device and on the host: (pushes, device table, host table)."""
    X, nw, nr, ng = lm
    sc = LR.accuracy_scene()
    mo = LR.accuracy_motions(sc, noisy)
    pushes, _ = _sequence(ctx, sc, LR.ACC_CAP, LR.accuracy_starts(sc), mo, check=False, iterations=LR.ACC_ITERATIONS,
                          record=0)

    def batch(T_in, motions, frames, n):
        res, views = ctx.smooth_batch(_images(frames, sc["ext"]), 1, n, T_in, motions, iterations=LR.ACC_ITERATIONS)
        assert res[0].status == 0
        return np.array([LR.pose_of(v) for v in views[0]])

    dev = LR.accuracy_compare(sc, mo, [(r, v) for r, v, _ in pushes], batch)
    _, host = LR.accuracy_host(sc, mo, X, nw, nr, ng)
    return pushes, dev, host


@pytest.mark.parametrize("noisy", [False, True], ids=["exact", "perturbed"])
def test_accuracy_scene_windows_and_distance_to_the_history(ctx, lm, noisy):
    """Twelve one-camera views, capacity 4, views 5 and 6 black, exact motions and motions off by the default
    sigmas: every lag window is OK and carries a prior from the first slide on, and at every push after the first
    slide the newest view is within twice the host's figure (hc_lag_seq against hc_smooth_seq) of
    mantis_smooth_batch over the whole history."""
    pushes, dev, host = _accuracy(ctx, lm, noisy)
    assert [r.status for r, _, _ in pushes] == [0] * LR.ACC_VIEWS
    assert [i.has_prior for _, _, i in pushes] == [int(q >= LR.ACC_CAP) for q in range(LR.ACC_VIEWS)]
    for q in dev:
        print(f"push {q}: lag-H {dev[q][0]:.3e} (host {host[q][0]:.3e})  T-H {dev[q][1]:.3e}  lag-T {dev[q][2]:.3e}")
    for q in dev:
        assert dev[q][0] <= 2.0 * host[q][0], (q, dev[q][0], host[q][0])


@pytest.mark.parametrize("noisy", [False, True], ids=["exact", "perturbed"])
def test_accuracy_scene_lag_is_closer_to_the_history_than_truncation(ctx, lm, noisy):
    """At the pushes whose window begins with a black view (8 and 9), the lag window's newest pose is strictly
    closer to the whole history's (H) than that of the last four views with no prior (T); the three start every
    view they share from the same pose (LR.accuracy_compare). Host figures, d(lag, H) / d(T, H) (translation +
    rotation angle): exact motions 2.044e-9 / 1.062e-7 (push 8), 3.092e-12 / 2.010e-10 (9); perturbed 3.215e-9 /
    3.563e-8 (8), 8.162e-12 / 3.991e-10 (9): the lag window is 11 to 65 times the closer."""
    pushes, dev, host = _accuracy(ctx, lm, noisy)
    black = [q for q in dev if dev[q][3]]
    assert black == [8, 9]
    for q in dev:
        print(f"push {q}: lag-H {dev[q][0]:.6e}  T-H {dev[q][1]:.6e}  T-H - lag-H {dev[q][1] - dev[q][0]:+.3e}")
    for q in black:
        assert dev[q][0] < dev[q][1], (q, dev[q][0], dev[q][1])
