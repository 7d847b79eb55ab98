"""The scorers against the oracle beyond the bench camera: the matrix of
_score_cases.py (9 lenses x 4 frame sizes, blob-noise images, byte masks with
the values 1 / 128 / 255, poses aimed a quarter pixel off every frame edge, on
the optical axis, in and below the floor plane, seeing nothing, arbitrary and
near truth), maps of 1 .. 768 landmarks, the dense argmin, the screen-camera
cache, and the track / MCL rig scorers (tiled mask bits) on a rig whose
cameras carry three different lenses. tests/test_score_matrix_host.py holds
the census that makes these comparisons meaningful: no generated projection
lies within 1e-9 px of a decision threshold, so every comparison is exact and
nothing is skipped at run time.
"""
import math

import numpy as np
import pytest

import _oracle as O
import _score_cases as SC
from mantis_amd import synth

pytestmark = pytest.mark.gpu

DBL_MAX = np.finfo(np.float64).max


@pytest.fixture(scope="module")
def mantis(landmark_map):
    import mantis_amd as M

    m = M.Mantis(max_cams=8, max_width=1280, max_height=720)
    m.set_map(*landmark_map)
    yield m
    m.close()


@pytest.fixture(scope="module")
def orc(landmark_map):
    return O.Oracle(*landmark_map)


def _inputs(c):
    """(image, mask, cleaned image) of a cell's frame size."""
    img = SC.blob_image(c.w, c.h, 1)
    mk = SC.blob_mask(c.w, c.h, 1)
    assert {1, 128, 255} <= set(np.unique(mk).tolist()) and 0.3 < (mk != 0).mean() < 0.7
    return img, mk, SC.cleaned(img, mk)


def _cmp(got, ref, fast, label):
    ge, gn = got
    oe, on = ref
    assert np.array_equal(gn, on), f"{label}: nproj differs at {np.nonzero(gn != on)[0][:8]}"
    if fast:
        assert np.array_equal(ge, oe), f"{label}: err differs at {np.nonzero(ge != oe)[0][:8]}"
    else:
        np.testing.assert_allclose(ge, oe, rtol=1e-13, atol=0, err_msg=label)
    assert np.all(ge[gn == 0] == DBL_MAX)


def test_score_matrix_fast(mantis, orc):
    """Every (lens, size) cell on the yaml map: the fast scorer, unmasked and
    under a byte mask (and, on the 130x35 cells, under an all-zero mask: n > 0
    and every term black), equals the oracle: counts and integer sums."""
    import mantis_amd as M

    for c in SC.all_cells():
        img, mk, cl = _inputs(c)
        im = M.make_image(img, c.K, c.D)
        label = f"{c.name} {c.w}x{c.h}"
        _cmp(mantis.score(im, c.c2w, fast=True), orc.score(img, c.K, c.D, c.c2w, fast=True), True, label)
        _cmp(mantis.score(im, c.c2w, fast=True, mask=mk), orc.score(cl, c.K, c.D, c.c2w, fast=True), True,
             label + " masked")
        if (c.w, c.h) == SC.SIZES[2]:
            zero = np.zeros((c.h, c.w), np.uint8)
            ge, gn = mantis.score(im, c.c2w, fast=True, mask=zero)
            _cmp((ge, gn), orc.score(np.zeros_like(img), c.K, c.D, c.c2w, fast=True), True, label + " zero mask")
            assert np.all(ge[gn > 0] == 3 * 255.0 * 255.0 * gn[gn > 0] / (gn[gn > 0] * 1.1))
        assert (c.kind == 4).sum() == SC.N_NOTHING


def test_score_matrix_color(mantis, orc):
    """The same cells through the COLOR scorer (10 x 10 windows; on the 33x7
    and 130x35 frames most windows cross the buffer's ends and row ends)."""
    import mantis_amd as M

    for c in SC.all_cells():
        img, _, _ = _inputs(c)
        got = mantis.score(M.make_image(img, c.K, c.D), c.c2w, fast=False)
        _cmp(got, orc.score(img, c.K, c.D, c.c2w, fast=False), False, f"{c.name} {c.w}x{c.h} COLOR")


def test_score_map_shapes(mantis, landmark_map):
    """Maps of 768 (a full register trip per half), 767 (unequal halves), 385
    (no green), 65 / 64 / 63, 2 and 1 landmarks (wave 0's half of one landmark
    is empty) on two cells: fast, masked and unmasked, and COLOR."""
    import mantis_amd as M

    try:
        for name, si in (("bench", 0), ("x3", 1)):
            for mname, n, ng in SC.MAP_SHAPES:
                c = SC.cell(name, si, mname)
                mp = SC.get_map(mname)
                mantis.set_map(*mp)
                o = O.Oracle(*mp)
                img, mk, cl = _inputs(c)
                im = M.make_image(img, c.K, c.D)
                label = f"{mname} {c.name} {c.w}x{c.h}"
                _cmp(mantis.score(im, c.c2w, fast=True), o.score(img, c.K, c.D, c.c2w, fast=True), True, label)
                _cmp(mantis.score(im, c.c2w, fast=True, mask=mk), o.score(cl, c.K, c.D, c.c2w, fast=True), True,
                     label + " masked")
                _cmp(mantis.score(im, c.c2w, fast=False), o.score(img, c.K, c.D, c.c2w, fast=False), False,
                     label + " COLOR")
    finally:
        mantis.set_map(*landmark_map)


def test_score_dense_matrix(mantis, orc):
    """mantis_score_argmin on every lens at 1280x720 and 33x7, >= 130
    hypotheses (two 64-hypothesis blocks and part of a third): (minimum,
    base + first index of the minimum) of the oracle's errors. Hypotheses that
    all see nothing score DBL_MAX each and yield (DBL_MAX, base + 0), the
    header's "first index on ties"; -1 is left to n == 0."""
    import mantis_amd as M

    base = 1000
    for name in SC.LENSES:
        for si in (0, 3):
            c = SC.cell(name, si)
            assert len(c.c2w) >= 130
            img, mk, cl = _inputs(c)
            im = M.make_image(img, c.K, c.D)
            for mask, ref_img in ((None, img), (mk, cl)):
                oe, _ = orc.score(ref_img, c.K, c.D, c.c2w, fast=True)
                want = (float(oe.min()), base + int(np.argmin(oe)))
                assert oe.min() < DBL_MAX
                got = mantis.score_argmin(im, c.c2w, base, False, mask)
                assert got == want, (name, c.w, c.h, mask is not None, got, want)
    for si in (0, 3):
        K, D, w, h, c2w = SC.nothing_cell(si)
        img = SC.blob_image(w, h, 1)
        oe, on = orc.score(img, K, D, c2w, fast=True)
        assert np.all(on == 0) and np.all(oe == DBL_MAX) and len(c2w) >= 130
        im = M.make_image(img, K, D)
        assert mantis.score_argmin(im, c2w, base, False, None) == (DBL_MAX, base)
        assert mantis.score_argmin(im, c2w[:1], base + 7, False, None) == (DBL_MAX, base + 7)
        # as two shards: each all DBL_MAX, combined by the library's pick
        a = mantis.score_argmin(im, c2w[:66], base, False, None)
        b = mantis.score_argmin(im, c2w[66:], base + 66, False, None)
        assert a == (DBL_MAX, base) and b == (DBL_MAX, base + 66)
        assert M.argmin_pick([b, a]) == (DBL_MAX, base)
        # a shard that is all DBL_MAX beside one that sees the floor
        c = SC.cell("bench", si)
        oe, _ = orc.score(img, c.K, c.D, c.c2w, fast=True)
        g = mantis.score_argmin(im, c.c2w, base + 130, False, None)
        assert g == (float(oe.min()), base + 130 + int(np.argmin(oe)))
        assert M.argmin_pick([a, g]) == g and M.argmin_pick([g, a]) == g
        assert M.argmin_pick([a, [DBL_MAX, -1]]) == a


def test_screen_cam_cache_eviction(mantis, orc):
    """70 distinct lenses in turn on the 33x7 frame (the context keeps 64
    screen cameras and evicts the oldest), then the first again."""
    import mantis_amd as M

    c = SC.cell("x3", 3)
    img = SC.blob_image(c.w, c.h, 1)
    first = None
    for i in list(range(70)) + [0]:
        K = c.K.copy()
        K[0, 0] *= 1 + 1e-5 * i  # (1e-5 relative: 160 float32 ulps apart)
        K[1, 1] *= 1 - 1e-5 * i
        # a perturbed lens must keep the cell's guard to be comparable
        assert SC.Proj(c.c2w, c.lm, K, c.D, c.w, c.h).guard_violations() == 0, i
        got = mantis.score(M.make_image(img, K, c.D), c.c2w, fast=True)
        _cmp(got, orc.score(img, K, c.D, c.c2w, fast=True), True, f"lens {i}")
        if first is None:
            first = got
    assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])


# ------------------------------------------------- rig scorers, mixed lenses
# Track and MCL read the mask as the tiled bit plane (MaskBits), where the
# (x, y) that exact_term hands to the mask after the cvRound(u) == W wrap
# matter. 640 x 360: its tiled plane, words(640) * tiled_rows(360) * 4 =
# 20 * 384 * 4 = 30,720 bytes, also fits the particle-filter kernel's dynamic
# LDS beside its static part (api.hip: sharedSizeBytes + plane <= 160 KiB), so
# a context of this size stages masks in LDS where the pipeline scores.
RW, RH = 640, 360
RIG_CAMS = (0, 3, 5)
RIG_LENSES = ("x3", "strong0", "off")
SIG_R, SIG_T = 1e-4, 1e-4  # rad, m: ~0.05 px at this lens and range, against the landmark's 0.25 px of room


def _render(Twc, K, D, cam):
    sc = synth.make_cam(Twc[:3, :3], Twc[:3, 3], RW, RH)
    sc.fx, sc.fy, sc.cx, sc.cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    for i in range(4):
        sc.k[i] = D[i]
    return synth.render_host(sc, synth.frame_seed(21, cam))


def _c2w12(T_w_c):
    T = np.linalg.inv(T_w_c)
    return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])


def _rot_about(w, phi):
    """World rotation by phi about the unit axis w (Rodrigues)."""
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + math.sin(phi) * Kx + (1 - math.cos(phi)) * (Kx @ Kx)


def _wrap_pose(Twc, K, D, lm):
    """Camera pose near Twc for which a landmark wraps (u = W - 0.25, so
    cvRound(u) == W and the scorer reads pixel (0, y + 1)) at a row y where the
    frame's own mask differs between (0, y) and (0, y + 1): there a mask read
    at (0, y) instead of (0, y + 1) changes the sum. The mask follows the
    image, so the pose is moved with the two motions that keep the floor point
    seen at (0, y + 1/2) where it is -- a roll about its ray and a step along
    it -- until the landmark nearest the target sits on it; a few rounds, as
    the mask's rows may move by one. Returns (Twc, y, landmark index)."""
    Kr = SC.k32(K)
    for _ in range(6):
        m = O.clean_mask(O.canny(_render(Twc, K, D, RIG_CAMS[0]))) != 0
        rows = np.nonzero(m[1:, 0] != m[:-1, 0])[0]
        rows = rows[(rows > 20) & (rows < RH - 20)]
        assert len(rows), "the x3 camera's mask has no transition in column 0"
        y = int(rows[np.argmin(np.abs(rows - RH // 2))])
        tgt = np.array([RW - 0.25, y + 0.3])
        R, C = Twc[:3, :3], Twc[:3, 3]  # camera -> world, centre
        uv = O.distort((lm - C) @ R, K, D)
        front = ((lm - C) @ R)[:, 2] > 0.1
        li = int(np.argmin(np.where(front, np.linalg.norm(uv - tgt, axis=1), np.inf)))
        if np.abs(uv[li] - tgt).max() < 0.05:
            return Twc, y, li
        w = R @ SC.ray_of_pixel(0.0, y + 0.5, Kr, D)
        Q = C - w * (C[2] / w[2])  # the floor point seen at (0, y + 1/2)

        def pose(phi, s):
            T = np.eye(4)
            T[:3, :3] = _rot_about(w, phi) @ R
            T[:3, 3] = Q + s * (C - Q)
            return T

        def f(x):
            T = pose(x[0], x[1])
            return O.distort(((lm[li] - T[:3, 3]) @ T[:3, :3])[None], K, D)[0] - tgt

        x = np.array([0.0, 1.0])
        for _ in range(30):
            r = f(x)
            if np.abs(r).max() < 1e-9:
                break
            J = np.stack([(f(x + [1e-6, 0]) - r) / 1e-6, (f(x + [0, 1e-6]) - r) / 1e-6], 1)
            x = x - np.linalg.solve(J, r)
        Twc = pose(x[0], x[1])
    raise AssertionError("no pose puts a wrapping landmark on a mask transition of column 0")


def _rig_scene(landmark_map):
    """Base pose from which camera 0 (the x3 lens) sees one landmark at
    u = W - 0.25 on a row where its mask changes in column 0 (_wrap_pose),
    starting from the one of 64 rolls about a first aim that gives the
    worst-placed camera the most landmarks. Frames rendered through each
    camera's own lens; cleaned frames from the oracle's Canny and mask."""
    import mantis_amd as M

    lm = np.vstack(landmark_map)
    ext = synth.rig_extrinsics(8)
    lens = [SC.lens(nm, RW, RH) for nm in RIG_LENSES]
    ray = SC.ray_of_pixel(RW - 0.25, RH // 2 + 0.3, SC.k32(lens[0][0]), lens[0][1])
    X = lm[np.argmin(np.linalg.norm(lm[:, :2] - [0.3, 0.2], axis=1))]
    C = X + np.array([0.35, -0.25, 1.4])
    best = None
    for k in range(64):
        c2w = SC.aimed_pose(X, C, ray, 2 * math.pi * k / 64)
        Tcw = np.eye(4)
        Tcw[:3, :3], Tcw[:3, 3] = c2w[:9].reshape(3, 3), c2w[9:]
        Twb = np.linalg.inv(Tcw) @ np.linalg.inv(ext[RIG_CAMS[0]])
        cnt = []
        for ci, cam in enumerate(RIG_CAMS):
            p = SC.Proj(_c2w12(Twb @ ext[cam])[None], lm, lens[ci][0], lens[ci][1], RW, RH)
            cnt.append(int(p.inside.sum()))
        if best is None or min(cnt) > best[0]:
            best = (min(cnt), Twb)
    Twc0, wrap_row, wrap_lm = _wrap_pose(best[1] @ ext[RIG_CAMS[0]], lens[0][0], lens[0][1], lm)
    Twb = Twc0 @ np.linalg.inv(ext[RIG_CAMS[0]])
    frames, cleaned, images, masks = [], [], [], []
    for ci, cam in enumerate(RIG_CAMS):
        K, D = lens[ci]
        img = _render(Twb @ ext[cam], K, D, cam)
        frames.append(img)
        masks.append(O.clean_mask(O.canny(img)) != 0)
        cleaned.append(SC.cleaned(img, masks[-1]))
        images.append(M.make_image(img, K, D, T_base_cam=ext[cam]))
    return {"Twb": Twb, "lens": lens, "images": images, "cleaned": cleaned, "lm": lm, "ext": ext, "frames": frames,
            "masks": masks, "wrap_row": wrap_row, "wrap_lm": wrap_lm}


@pytest.fixture(scope="module")
def rig(landmark_map):
    import mantis_amd as M

    r = _rig_scene(landmark_map)
    r["m"] = M.Mantis(max_cams=8, max_width=RW, max_height=RH)
    r["m"].set_map(*landmark_map)
    yield r
    r["m"].close()


def _check_rig_record(rig, orc, c2w, sums, counts, label):
    """Every recorded (particle, camera) against the oracle on the cleaned
    frame with the camera's own K and D; returns the numbers of recorded
    (particle, x3 camera) pairs with an in-frame cvRound(u) == W, and of those
    whose row y has a mask that differs between (0, y) and (0, y + 1) and a
    pixel (0, y + 1) that is not black: a mask read at the unwrapped row
    changes their sum."""
    wraps = bites = 0
    for ci in range(len(RIG_CAMS)):
        K, D = rig["lens"][ci]
        pj = SC.Proj(c2w[:, ci], rig["lm"], K, D, RW, RH)
        bad = pj.guard_violations()
        assert bad == 0, (f"{label} camera {ci}: {bad} projections of the recorded poses lie within {SC.GUARD} px of "
                          "a decision threshold: the comparison would not be exact (move the rig fixture's first aim)")
        err, npj = orc.score(rig["cleaned"][ci], K, D, c2w[:, ci], fast=True)
        assert np.array_equal(counts[:, ci], npj), f"{label} camera {ci}: counts"
        osum = np.where(npj > 0, np.rint(np.where(npj > 0, err, 0.0) * npj * 1.1), 0).astype(np.int64)
        assert np.array_equal(sums[:, ci], osum), f"{label} camera {ci}: sums"
        if ci == 0:
            wr = pj.inside & (pj.ru == RW) & (pj.rv + 1 < RH)
            wraps += int(wr.reshape(pj.n, pj.nl).any(axis=1).sum())
            y = pj.rv[wr]
            mk, img = rig["masks"][0], rig["frames"][0]
            bites += int(((mk[y, 0] != mk[np.minimum(y + 1, RH - 1), 0]) & img[np.minimum(y + 1, RH - 1), 0].any(axis=1)).sum())
    return wraps, bites


def test_track_rig_mixed_lenses(rig, orc):
    """mantis_track_batch, 7 particles x 2 iterations on a 3-camera rig with
    the x3 lens, a strong lens and the lens that switches the screen off."""
    m, P, I = rig["m"], 7, 2
    m.rng_state = 1
    res = m.track_batch(rig["images"], 1, rig["Twb"], particles=P, iterations=I, sigma_rot=SIG_R, sigma_t=SIG_T,
                        record=1)[0]
    assert res.status == 0
    wraps = bites = 0
    for k in [-1] + list(range(1, I + 1)):
        Tk, c2wk, sk, nk = m.track_record(0, k)
        assert len(Tk) == (1 if k < 0 else P)
        for ci, cam in enumerate(RIG_CAMS):
            ref = np.array([np.linalg.inv(T @ rig["ext"][cam]) for T in Tk])
            ref12 = np.concatenate([ref[:, :3, :3].reshape(-1, 9), ref[:, :3, 3]], axis=1)
            np.testing.assert_allclose(c2wk[:, ci], ref12, atol=1e-9, rtol=0)
        w, b = _check_rig_record(rig, orc, c2wk, sk, nk, f"pass {k}")
        wraps, bites = wraps + w, bites + b
        assert np.all(nk.sum(axis=1) >= 10)
    assert wraps >= 1, "no recorded (particle, camera) with cvRound(u) == W"
    assert bites >= 1, "no recorded wrap on a row where the mask changes in column 0"


def test_mcl_rig_mixed_lenses(rig, orc):
    """The same rig through mantis_mcl_step / mantis_mcl_get_record, colour off."""
    m, N = rig["m"], 7
    m.rng_state = 1
    m.mcl_set_color(0)
    m.mcl_init_particles(np.repeat(rig["Twb"][None], N, 0), sigma_rot=SIG_R, sigma_t=SIG_T, tau=60000.0,
                         resample_frac=0.0, record=1)
    wraps = bites = 0
    for step in range(2):
        out, mo = m.mcl_step(rig["images"])
        assert mo.status == 0
        rec = m.mcl_record()
        assert rec["sums"].shape == (N, len(RIG_CAMS))
        w, b = _check_rig_record(rig, orc, rec["c2w"], rec["sums"], rec["counts"], f"step {step}")
        wraps, bites = wraps + w, bites + b
    assert wraps >= 1, "no recorded (particle, camera) with cvRound(u) == W"
    assert bites >= 1, "no recorded wrap on a row where the mask changes in column 0"
