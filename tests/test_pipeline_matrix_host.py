"""CPU census of the whole-callback matrix (_pipeline_cases.py): the condition
under which test_gpu_pipeline_matrix.py means anything, checked with the
oracle alone.

Census of the committed generator (90 frames: 9 lenses x 2 sizes x 4 views,
plus 9 lenses x 2 tiny sizes; base seed 312; no case had to move off its first
seed, so seeds moved: {}):
  reasons 0 .. 4: 14, 16, 13, 43, 4 frames (reason 4 only with pp_out);
  n_hyps == 1 in 7 frames, n_quads >= 70 in 9, n_raw_quads - n_quads >= 20 in 8
  (at most 46); n_quads 0 .. 78, n_gen 4 .. 308, n_hyps at most 71;
  test points: 109 above 1e15 (d0, steep view: theta_d clamped to pi / 2), the
  largest 1.946e16; 6 in (1e3, 1e15); 439 above 10.
Largest pose motion under the perturbation of D[0], D[1] by +-1e-13 (bound
1e-7 x max(1, |entry|)): 4.222e-10 with a fresh Oracle(seed=1) per frame,
4.467e-10 over the GPU tests' batches with the RNG carried; no integer record
changed in either.
"""
import numpy as np
import pytest

import _pipeline_cases as PC


@pytest.fixture(scope="module")
def cases():
    """Every case of the matrix; the three oracle passes of a case run once
    and are cached for the module (and for the process)."""
    return PC.all_cases()


def test_no_case_is_left_out(cases):
    """Every cell has its 4 views, every tiny size one frame per lens, every
    kept case keeps the guard, and at most 1 seed in 4 per cell had to move."""
    by_cell = {}
    for c in cases:
        by_cell.setdefault((c.name, c.w, c.h), []).append(c)
    assert len(cases) == len(PC.LENSES) * (len(PC.SIZES) * len(PC.VIEWS) + len(PC.TINY))
    for name in PC.LENSES:
        for wh in PC.SIZES:
            assert [c.view for c in by_cell[(name, *wh)]] == [v[0] for v in PC.VIEWS], (name, wh)
        for wh in PC.TINY:
            assert len(by_cell[(name, *wh)]) == 1, (name, wh)
    moved = {(c.name, c.w, c.h, c.view): (c.seeds_moved, c.moved_motion) for c in cases if c.seeds_moved}
    print("seeds moved:", moved)
    print("largest pose motion under the perturbation: %.3e (bound %.1e)" % (max(c.motion for c in cases), PC.MOTION))
    for c in cases:
        assert c.motion <= PC.MOTION, (c.name, c.w, c.h, c.view, c.motion)
        assert c.img.shape == (c.h, c.w, 3)
    for key, cs in by_cell.items():
        tried = sum(c.seeds_moved + 1 for c in cs)
        assert 4 * sum(c.seeds_moved for c in cs) <= tried, (key, [c.seeds_moved for c in cs])


def test_every_class_occurs(cases):
    recs = [c.rec for c in cases]
    reasons = [sum(r.reason == k for r in recs) for k in range(5)]
    tp = [np.abs(PC._rows(r, "test_pts")) for r in recs]
    tot = {
        "frames": len(recs), "reasons_0_to_4": reasons,
        "n_hyps_eq_1": sum(r.n_hyps == 1 for r in recs),
        "n_quads_ge_70": sum(r.n_quads >= 70 for r in recs),
        "dups_ge_20": sum(r.n_raw_quads - r.n_quads >= 20 for r in recs),
        "tp_gt_1e15": int(sum((t > 1e15).sum() for t in tp)),
        "tp_1e3_to_1e15": int(sum(((t > 1e3) & (t < 1e15)).sum() for t in tp)),
        "tp_gt_10": int(sum((t > 10).sum() for t in tp)),
        "tp_max": max(float(t.max()) for t in tp if t.size),
        "n_quads": (min(r.n_quads for r in recs), max(r.n_quads for r in recs)),
        "n_gen": (min(r.n_gen for r in recs if r.reason not in (1, 2)), max(r.n_gen for r in recs)),
        "n_hyps_max": max(r.n_hyps for r in recs),
        "dups_max": max(r.n_raw_quads - r.n_quads for r in recs),
    }
    print("census:", tot)
    assert not any(np.isnan(t).any() for t in tp)
    for k in range(5):
        assert reasons[k] >= 3, (k, reasons)
    for k in ("n_hyps_eq_1", "n_quads_ge_70", "dups_ge_20", "tp_gt_1e15", "tp_1e3_to_1e15"):
        assert tot[k] >= 1, (k, tot[k])


def test_batches_keep_the_guard_with_the_rng_carried(cases):
    """The GPU tests process the cases in batches, the cv::RNG carried from
    frame to frame: every frame of every batch keeps the guard run that way
    too (integer records, the RNG state included, and pose motion)."""
    from concurrent.futures import ThreadPoolExecutor

    bs = PC.batches()
    assert len(bs) == len(PC.LENSES) * len(PC.SIZES) + len(PC.TINY) + len(PC.SIZES)
    with ThreadPoolExecutor(4) as ex:
        res = list(ex.map(lambda b: PC.sequence_guard(b[1]), bs))
    worst = 0.0
    for (tag, cs), (per_frame, same_rng) in zip(bs, res):
        assert same_rng, tag
        for i, (kept, motion) in enumerate(per_frame):
            assert kept, (tag, i, cs[i].view, motion)
            worst = max(worst, motion)
    print("largest pose motion under the perturbation, RNG carried: %.3e (bound %.1e)" % (worst, PC.MOTION))


def test_tiny_frames_return_early(cases):
    """At 130x35 and 33x7 only the early returns occur: no quadrilateral
    (reason 1) or no hypothesis (reason 2)."""
    for c in cases:
        if (c.w, c.h) in PC.TINY:
            assert c.rec.reason in (1, 2), (c.name, c.w, c.h, c.rec.reason)


def test_guard_rejects_a_moved_record(cases):
    """The guard itself: a record with one integer changed, or one pose entry
    moved by 2e-7 relative, is refused; the same records unchanged are kept."""
    import copy

    c = next(c for c in cases if c.rec.reason == 0)
    same = [c.rec, c.rec, c.rec]
    assert PC.guard(same) == (True, 0.0)
    r = copy.deepcopy(c.rec)
    r.hyp_n[0] += 1
    assert not PC.guard([c.rec, c.rec, r])[0]
    r = copy.deepcopy(c.rec)
    r.rng_state_after += 1
    assert not PC.guard([c.rec, r, c.rec])[0]
    r = copy.deepcopy(c.rec)
    r.position[2] += 2e-7 * max(1.0, abs(r.position[2]))
    ok, motion = PC.guard([c.rec, c.rec, r])
    assert not ok and 1e-7 < motion < 3e-7
    r = copy.deepcopy(c.rec)
    r.position[2] += 5e-8
    assert PC.guard([c.rec, c.rec, r])[0]


def test_comparer_bounds(cases):
    """The comparer against records altered by hand: a test point of 1e16 may
    move by 4,000 ulp but not by 2e-12 relative; an integer record not at all;
    a NaN only where the oracle has one. Poses, on the case with the largest
    translation of the matrix (the 'off' lens, low view: 74 m): a rotation or
    quaternion entry may not move by 2e-9 whatever the pose's translation; a
    translation or position may move by half of 1e-9 x its largest magnitude
    but not by twice that."""
    import copy

    def tmax(c):
        return float(np.abs(np.array(c.rec.pf_c2w)[9:]).max()) if c.rec.reason not in (1, 2) else 0.0

    c = max(cases, key=tmax)
    o = c.rec
    T = {f: float(np.abs(v).max()) for f, v in (("hyp", np.array(o.hyp_c2w)[0][9:]), ("pf", np.array(o.pf_c2w)[9:]),
                                                ("pos", np.array(o.position)))}
    print("comparer case:", c.name, c.w, c.h, c.view, T)
    assert min(T.values()) > 2
    PC.cmp_record(o, o, "same")

    def altered(f, base=o):
        r = copy.deepcopy(base)
        f(r)
        return r

    def add(field, i, d, row=None):
        def f(r):
            a = getattr(r, field) if row is None else getattr(r, field)[row]
            a[i] += d
        return f

    def big(r, rel):
        r.test_pts[0][0] = 1e16 * (1 + rel)

    for f in (add("hyp_c2w", 9, 0.5e-9 * T["hyp"], 0), add("pf_c2w", 11, -0.5e-9 * T["pf"]),
              add("position", 0, 0.5e-9 * T["pos"])):
        PC.cmp_record(altered(f), o, "translation, inside")
    ob = altered(lambda r: big(r, 0.0))
    PC.cmp_record(altered(lambda r: big(r, 8e-13), ob), ob, "big test point, inside")
    for f in (lambda r: big(r, 2e-12),
              lambda r: r.test_pts[0].__setitem__(1, float("nan")),
              add("hyp_c2w", 0, 2e-9, 0), add("hyp_c2w", 8, -2e-9, 0), add("pf_c2w", 4, 2e-9),
              add("orientation_xyzw", 3, 2e-9),
              add("hyp_c2w", 9, 2e-9 * T["hyp"], 0), add("pf_c2w", 11, 2e-9 * T["pf"]),
              add("position", 0, 2e-9 * T["pos"]),
              lambda r: r.pf_c2w.__setitem__(11, float("nan")),
              lambda r: r.shift_err.__setitem__(80, r.shift_err[80] * (1 + 1e-15)),
              lambda r: setattr(r, "rng_state_after", r.rng_state_after ^ 1)):
        with pytest.raises(AssertionError):
            PC.cmp_record(altered(f, ob), ob, "altered")
