"""CPU census of the scoring matrix (_score_cases.py): the condition under
which test_gpu_score_matrix.py means anything, checked with the reference
alone (the oracle's distort, the host build of the screen, numpy).

Census of the committed generator (36 cells, 9 lenses x 4 sizes, 130 .. 170
poses each, yaml map; no cell had to move off its first seed):
  in-frame cvRound(u) == W 569, == 0 2,258, cvRound(v) == 0 23,537, == H 24,568,
  cvRound(u) == W and cvRound(v) == H together 60;
  z <= 0 1,126,858, r > 1 1,443,022, on-axis 357, hypotheses with n == 0 1,118;
  host screen SCR_IN 1,413,048, SCR_OUT 2,084,307, SCR_UNSURE 367,605.
"""
import numpy as np
import pytest

import _hostcheck as H
import _score_cases as SC


@pytest.fixture(scope="module")
def cells():
    return SC.all_cells()


@pytest.fixture(scope="module")
def screen(cells):
    """Per cell: (mismatches, states [n * nl]) of the host screen."""
    out = []
    for c in cells:
        n, nl = len(c.c2w), len(c.lm)
        bad, res = H.screen_check(np.repeat(c.c2w, nl, axis=0), np.tile(c.lm, (n, 1)), c.K, c.D, c.w, c.h)
        out.append((bad, res[:, 0].copy(), res[:, 1].copy()))
    return out


def test_no_case_is_left_out(cells):
    """Every generated projection keeps the 1e-9 px guard, so the GPU tests
    skip nothing at run time; the seeds that had to move are reported."""
    moved = {(c.name, c.w, c.h): c.seeds_moved for c in cells if c.seeds_moved}
    print("seeds moved:", moved)
    for c in cells:
        assert c.proj.guard_violations() == 0, (c.name, c.w, c.h)
        assert len(c.c2w) >= 100, (c.name, c.w, c.h, len(c.c2w))
    for si in range(len(SC.SIZES)):
        SC.nothing_cell(si)  # asserts its own guard and that nothing is seen
    for name, si in (("bench", 0), ("x3", 1)):
        for mname, n, ng in SC.MAP_SHAPES:
            c = SC.cell(name, si, mname)
            assert c.proj.guard_violations() == 0
            w, r, g = SC.get_map(mname)
            assert len(w) + len(r) + len(g) == n and len(g) == ng


def test_every_class_occurs(cells, screen):
    tot = {}
    for c in cells:
        for k, v in c.proj.counts().items():
            tot[k] = tot.get(k, 0) + v
    st = np.concatenate([s[1] for s in screen])
    tot["SCR_OUT"], tot["SCR_IN"], tot["SCR_UNSURE"] = (int((st == k).sum()) for k in (0, 1, 2))
    print("census:", tot)
    for k in ("u_eq_W", "u_eq_0", "v_eq_0", "v_eq_H", "z_le_0", "r_gt_1", "on_axis", "hyp_n0", "SCR_IN", "SCR_OUT",
              "SCR_UNSURE"):
        assert tot[k] >= 20, (k, tot[k])
    assert tot["corner_WH"] >= 5, tot["corner_WH"]


def test_reference_rounds_K_to_float32():
    """K is CV_32F in the reference (get3x3FromVector): the oracle's distort
    and score and the host build must round a K that is no float32 as the
    library's cam_from does, or the census speaks of another camera than the
    one scored."""
    import _oracle as O

    K, D = SC.lens("x3", *SC.SIZES[1])
    Kr = SC.k32(K)
    assert Kr[0, 0] != K[0, 0] and Kr[1, 1] != K[1, 1]
    p = np.random.default_rng(2).uniform(-1, 1, (64, 3)) + [0, 0, 1.5]
    assert np.array_equal(O.distort(p, K, D), O.distort(p, Kr, D))
    assert np.array_equal(H.distort(p, K, D), H.distort(p, Kr, D))
    c = SC.cell("x3", 3)
    orc = O.Oracle(*SC.get_map("yaml"))
    img = SC.blob_image(c.w, c.h, 1)
    for fast in (True, False):
        a, b = orc.score(img, c.K, c.D, c.c2w, fast=fast), orc.score(img, SC.k32(c.K), c.D, c.c2w, fast=fast)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_aimed_targets_land(cells):
    """The bisection on theta_d's first branch sends the aimed landmark to its
    target: some landmark of every aimed pose projects within 1e-9 px of one
    of the cell's targets."""
    for c in cells:
        tg = np.array(SC.targets(c.w, c.h))
        idx = np.nonzero(c.kind == 0)[0]
        u = c.proj.u.reshape(c.proj.n, c.proj.nl)[idx]
        v = c.proj.v.reshape(c.proj.n, c.proj.nl)[idx]
        f = c.proj.front.reshape(c.proj.n, c.proj.nl)[idx]
        d = np.hypot(u[:, :, None] - tg[None, None, :, 0], v[:, :, None] - tg[None, None, :, 1])
        d = np.where(f[:, :, None], d, np.inf)
        assert (d.min(axis=(1, 2)) < 1e-9).all(), (c.name, c.w, c.h, d.min(axis=(1, 2)).max())


def test_screen_per_lens(cells, screen):
    """screen_consts admits every lens but the one chosen to switch the screen
    off; an admitted lens certifies landmarks; the host screen takes no
    decision that differs from the exact projection on the whole matrix."""
    for c, (bad, st, _) in zip(cells, screen):
        ok = H.screen_consts(c.K, c.D)[0]
        assert ok == (c.name != "off"), (c.name, ok)
        assert bad == 0, (c.name, c.w, c.h, bad)
        if ok:
            assert (st == 1).sum() > 0, (c.name, c.w, c.h)
        else:
            assert (st == 1).sum() == 0 and (st == 2).sum() > 0


def test_lens_list_reach():
    """Why the lens list exists: the bench lens at 1280x720 never projects to
    the first or last column; the x3 lens does both."""
    b = SC.cell("bench", 0).proj.counts()
    assert b["u_eq_W"] == 0 and b["u_eq_0"] == 0, b
    x = SC.cell("x3", 0).proj.counts()
    assert x["u_eq_W"] > 0 and x["u_eq_0"] > 0, x
