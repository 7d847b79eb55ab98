"""Whole-callback parity beyond the bench camera: mantis_process with its frame
record against the CPU oracle over the lens x size x view matrix of
_pipeline_cases.py (9 lenses, 1280x720 and 907x505, 4 views; tiny frames;
mixed-lens batches). The stages between the detector and the scorers (the
undistorted test points, RPP, hypothesis generation and clustering, the top-N
sort, the particle filter's seeding, the 81 shifts, the yaw choice and the
publish gate) meet test points up to 2e16, every early return, frames with 2
quads and frames with 300 generated hypotheses here. The census that makes
these cases meaningful is asserted on the CPU (test_pipeline_matrix_host.py).

Measured on an MI355X over every batch of this file: test points below 1e3
off by at most 4.4e-16, those above 1e3 (to 1.9e16) equal bit for bit (bound
1e-12 x max(1, |ref|)); rotation entries of hyp_c2w 8.1e-14 and of pf_c2w
5.3e-14, quaternion entries 3.0e-14 (bound 1e-9 absolute); translations of
hyp_c2w 3.0e-14, of pf_c2w 1.8e-14 and positions 8.3e-14 of
max(1, |t|max), which reaches 74 m (bound 1e-9 of it); every integer record
and cv::RNG state equal.
"""
import os

import numpy as np
import pytest

import _oracle as O
import _pipeline_cases as PC

pytestmark = pytest.mark.gpu

CELLS = [(name, w, h) for name in PC.LENSES for (w, h) in PC.SIZES]
# the switches that force the large-batch kernel shapes on a small batch
# (test_gpu_switches.py's throughput fence, test_gpu_parity.py's
# test_throughput_mode_kernels_match_latency_mode)
LARGE_SHAPES = {"MANTIS_FC_SMALL_FRAMES": "0", "MANTIS_TRACE_LDS_FRAMES": "0"}

_seq_cache = {}


def _sequence(key, make):
    """(cases, oracle records in order with the RNG carried, final RNG state),
    computed once per module for a cell or a batch."""
    if key not in _seq_cache:
        cases = make()
        _seq_cache[key] = (cases,) + PC.oracle_sequence(cases)
    return _seq_cache[key]


def _context(env, n, w, h, landmark_map):
    import mantis_amd as M

    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        m = M.Mantis(max_cams=n, max_width=w, max_height=h)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v
    m.set_map(*landmark_map)
    m.rng_state = 1
    return m


def _check_batch(cases, recs, rng_after, landmark_map, tag, env=None, expect_small=None):
    """One context sized for the batch, rng_state = 1, every case its own
    mantis_image (its own K and D), one rig per frame; every frame record
    against the oracle's, in order."""
    import mantis_amd as M

    w, h = max(c.w for c in cases), max(c.h for c in cases)
    m = _context(env or {}, len(cases), w, h, landmark_map)
    try:
        if expect_small is not None:
            small = int(M.lib().mantis_small_batch_frames(m.h)) >= len(cases)
            assert small == expect_small, f"{tag}: the batch takes the {'latency' if small else 'throughput'} kernels"
        _, cams = m.process([M.make_image(c.img, c.K, c.D) for c in cases], rigs=len(cases))
        for i, (c, o) in enumerate(zip(cases, recs)):
            label = f"{tag} frame {i} ({c.name} {c.w}x{c.h} {c.view}, seed {c.seed})"
            PC.cmp_record(m.frame_debug(i), o, label)
            assert cams[i].reason == o.reason, f"{label}: result reason {cams[i].reason} vs {o.reason}"
            assert cams[i].publish == o.publish, f"{label}: result publish {cams[i].publish} vs {o.publish}"
        assert m.rng_state == rng_after, f"{tag}: cv::RNG stream must advance exactly as the reference's"
    finally:
        m.close()


@pytest.mark.parametrize("name,w,h", CELLS, ids=[f"{n}-{w}x{h}" for n, w, h in CELLS])
def test_callback_matrix(landmark_map, name, w, h):
    """The cell's 4 views as one batch of 4 one-camera rigs against an oracle
    that processes the same frames in order, carrying its RNG."""
    cases, recs, rng_after = _sequence((name, w, h), lambda: PC.cell(name, w, h))
    _check_batch(cases, recs, rng_after, landmark_map, f"{name} {w}x{h}")


def test_callback_tiny_frames(landmark_map):
    """130x35 and 33x7, every lens: only the early returns (no quadrilateral,
    no hypothesis) occur, and the RNG stream does not move."""
    for (w, h) in PC.TINY:
        cases, recs, rng_after = _sequence(("tiny", w, h), lambda: PC.tiny_cases(w, h))
        assert all(o.reason in (1, 2) for o in recs) and rng_after == 1
        _check_batch(cases, recs, rng_after, landmark_map, f"tiny {w}x{h}")


@pytest.mark.parametrize("w,h", PC.SIZES, ids=[f"{w}x{h}" for w, h in PC.SIZES])
def test_mixed_lens_batch(landmark_map, w, h):
    """One frame of every lens in one batch, each mantis_image with its own K
    and D: every stage must index the frame's own camera."""
    cases, recs, rng_after = _sequence(("mixed", w, h), lambda: PC.mixed_batch(w, h))
    assert len({(tuple(c.K.ravel()), tuple(c.D)) for c in cases}) == len(PC.LENSES)
    _check_batch(cases, recs, rng_after, landmark_map, f"mixed {w}x{h}", expect_small=True)


@pytest.mark.parametrize("w,h", PC.SIZES, ids=[f"{w}x{h}" for w, h in PC.SIZES])
def test_callback_matrix_large_batch_shapes(landmark_map, w, h):
    """The mixed-lens batch on a context created under the switches that force
    the large-batch kernel shapes (throughput kernels, border walks from L2)
    on a small batch, against the same oracle records."""
    cases, recs, rng_after = _sequence(("mixed", w, h), lambda: PC.mixed_batch(w, h))
    _check_batch(cases, recs, rng_after, landmark_map, f"mixed {w}x{h} large-batch shapes", env=LARGE_SHAPES,
                 expect_small=False)


def test_rpp_on_census_test_points(landmark_map):
    """mantis.rpp on the matrix's own image points: every census quad whose
    test points exceed 10 in magnitude (up to 2e16) plus 64 ordinary ones,
    with the two square models of test_rpp_batch_matches_oracle, against the
    oracle's RPP. Tells RPP apart from the stages around it."""
    import mantis_amd as M

    big, ordinary = [], []
    for c in PC.all_cases():  # cached: the cases of the tests above
        for q in PC._rows(c.rec, "test_pts"):
            (big if np.abs(q).max() > 10 else ordinary).append(q.reshape(4, 2))
    # the census: 127 such quads, 20 of them with a point above 1e15
    assert len(big) >= 100 and sum(np.abs(q).max() > 1e15 for q in big) >= 10
    pick = np.random.default_rng(17).choice(len(ordinary), 64, replace=False)
    quads = big + [ordinary[i] for i in pick]
    s = 0.16
    sq = [np.array([[s, -s, -s, s], [s, s, -s, -s], [0, 0, 0, 0.0]]),
          np.array([[s, -s, -s, s], [-s, -s, s, s], [0, 0, 0, 0.0]])]
    img_pts, obj_pts, refs = [], [], []
    for q in quads:
        for mdl in sq:
            ip = np.vstack([q[:, 0], q[:, 1], np.ones(4)])
            img_pts.append(q.copy())
            obj_pts.append(mdl.T.copy())
            refs.append(O.rpp(mdl, ip))
    m = M.Mantis(max_cams=1)
    try:
        R, t, e, st = m.rpp(np.array(img_pts), np.array(obj_pts))
    finally:
        m.close()
    bad = []
    for k, (rs, rR, rt, re, code) in enumerate(refs):
        label = f"problem {k} (quad {k // 2}, model {k % 2}, |tp| max {np.abs(img_pts[k]).max():.3g})"
        try:
            assert st[k] == rs, f"{label}: status {st[k]} vs {rs} (oracle code {code})"
            PC._close(R[k], rR, PC.POSE_TOL, f"{label}: R")  # |R| <= 1: an absolute bound
            PC._close(t[k], rt, PC.POSE_TOL, f"{label}: t", rows=3)
            assert np.array_equal(np.isnan(e[k]), np.isnan(re[:2])), f"{label}: NaN error in another place"
            np.testing.assert_allclose(e[k], re[:2], rtol=1e-9, atol=1e-15, err_msg=label)
        except AssertionError as ex:
            bad.append(str(ex).strip().splitlines()[0])
    assert not bad, f"{len(bad)} of {len(refs)} problems differ: " + "; ".join(bad[:8])
