"""The grid-line matrix on the GPU (tests/_line_cases.py; the census of its
cells is test_line_matrix_host.py): mantis_refine_batch, its robust rows and
the three calibrations on lenses, frame sizes and mixed rigs beyond the bench
camera, each call through the checker of its own GPU test file (every recorded
pass against the host build of the same rules at the device's own pose, the
MFMA accumulators against numpy sums, each step against the host's solve, and
under the whole-call guard the whole call against the host sequence), and the
slots no rendered frame reaches: no tangent, the candidate on the optical axis,
and windows that end a quarter pixel inside and outside the frame.
"""
import numpy as np
import pytest

import _icalib_ref as IR
import _line_cases as LC
import _rcalib_ref as QR
import _refine_ref as RR
from test_gpu_calib import _check_call as check_ext
from test_gpu_icalib import _check_call as check_int
from test_gpu_rcalib import _check_call as check_rig
from test_gpu_refine import _check_call as check_refine
from test_gpu_refine import _images as refine_images
from test_gpu_refine_robust import _check_call as check_robust
from test_line_matrix_host import OK, _calib_cells, calib_status, get_calib_cell, refine_status

pytestmark = pytest.mark.gpu

W, H = RR.W, RR.H_
NC = 540


@pytest.fixture(scope="module")
def mantis(landmark_map):
    import mantis_amd as M

    m = M.Mantis(max_cams=12, max_width=W, max_height=H)
    m.set_map(*landmark_map)
    yield m
    m.close()


@pytest.fixture(scope="module")
def lm(landmark_map):
    return RR.all_landmarks(landmark_map)


def _lenses(kds):
    return [IR.K_of(kd) for kd in kds], [np.array(kd[4:]) for kd in kds]


def _refine(mantis, lm, c):
    Ks, Ds = _lenses(c.kds)
    return check_refine(mantis, lm, c.frames, c.exts, c.T0, Ks=Ks, Ds=Ds, whole_call=c.guarded, **c.params)


@pytest.mark.parametrize("key", LC.refine_cell_ids(), ids=LC.cell_id)
def test_refinement_cell(mantis, lm, key):
    c = LC.refine_cell(*key)
    res = _refine(mantis, lm, c)
    print(LC.cell_id(key), res.status, res.refined, res.iterations_run, list(res.n_obs)[:5])
    if c.guarded:
        assert (res.status, res.refined, res.iterations_run) == refine_status(key)
        assert list(res.n_obs) == list(c.host.n_obs)


@pytest.mark.parametrize("loss", ["huber", "tukey"])
@pytest.mark.parametrize("cell", ["mixed", "strong2", "off"])
def test_robust_rows(mantis, lm, cell, loss):
    c = LC.mixed_rig(0) if cell == "mixed" else LC.refine_cell(cell, *LC.CALIB_SIZE, 12)
    Ks, Ds = _lenses(c.kds)
    try:
        res, st = check_robust(mantis, lm, c.frames, c.exts, c.T0, loss, Ks=Ks, Ds=Ds)
    finally:
        mantis.set_refine_robust(None)
    k = res.iterations_run
    print(cell, loss, res.status, res.refined, k, list(res.n_obs)[:5], list(st.n_down)[:5], list(st.n_zero)[:5])
    assert res.status == 0 and res.refined == 1 and k == 4
    assert st.n_down[k] > 0 and (loss == "tukey" or not any(st.n_zero))


def test_mixed_rig_record_parity(mantis, lm):
    for r in range(3):
        c = LC.mixed_rig(r)
        res = _refine(mantis, lm, c)
        assert (res.status, res.refined, res.iterations_run) == OK and list(res.n_obs) == list(c.host.n_obs)
        d0, a0 = RR.pose_dist(c.T0, c.T)
        d1, a1 = RR.pose_dist(np.array(res.T_w_b).reshape(4, 4), c.T)
        assert d1 < d0 and a1 < a0


def test_mixed_batch_equals_single_calls(mantis):
    cells = [LC.mixed_rig(r) for r in range(3)]
    imgs = []
    for c in cells:
        imgs += refine_images(c.frames, c.exts, c.w, c.h, *_lenses(c.kds))
    T0s = np.array([c.T0 for c in cells])
    batch = mantis.refine_batch(imgs, 3, T0s, record=1)
    recs = [[mantis.refine_record(r, k) for k in range(5)] for r in range(3)]
    for r in range(3):
        one = mantis.refine_batch(imgs[4 * r: 4 * r + 4], 1, T0s[r], record=1)[0]
        assert bytes(one) == bytes(batch[r]), f"rig {r}"
        assert one.refined == 1 and one.iterations_run == 4
        for k in range(5):
            for a, b in zip(mantis.refine_record(0, k), recs[r][k]):
                assert np.array_equal(a, b), (r, k)


def test_mixed_rig_without_its_strongest_lens(mantis):
    """test_blind_cameras' property: the slots of the other cameras are the same bits with or without the
    strong0 camera between them (a kernel that read a lens from a neighbouring frame would change them)."""
    c = LC.mixed_rig(0)
    Ks, Ds = _lenses(c.kds)
    mantis.refine_batch(refine_images(c.frames, c.exts, c.w, c.h, Ks, Ds), 1, c.T0, record=1, iterations=0)
    T, codes, Sw, Skw, rows, acc = mantis.refine_record(0, 0)
    keep = [0, 2, 3]
    sub = lambda a: [a[i] for i in keep]
    mantis.refine_batch(refine_images(sub(c.frames), sub(c.exts), c.w, c.h, sub(Ks), sub(Ds)), 1, c.T0, record=1,
                        iterations=0)
    T2, codes2, Sw2, Skw2, rows2, acc2 = mantis.refine_record(0, 0)
    for j, i in enumerate(keep):
        a, b = slice(i * NC, (i + 1) * NC), slice(j * NC, (j + 1) * NC)
        assert np.array_equal(codes[a], codes2[b]) and np.array_equal(rows[a], rows2[b]), i
        assert np.array_equal(Sw[a], Sw2[b]) and np.array_equal(Skw[a], Skw2[b]), i
        assert (codes[a] == 0).sum() > 100


def _gap_span(c):
    """IR.model_gap's grid for the cell: the bench lens's field, a third of it for the x3 lens."""
    return (2.2 / 3, 1.3 / 3) if "x3" in c.names else (2.2, 1.3)


def _calibrate(mantis, lm, c):
    Ks, Ds = _lenses(c.kds)
    Cn = len(c.exts)
    fe, fi = LC.free_of(c.kind, Cn)
    cap = max(LC.flag_cap(n, c.kind) for n in c.names)
    kw = dict(Ks=Ks, Ds=Ds, whole_call=c.guarded)
    if c.kind == "ext":
        return check_ext(mantis, lm, c.frames, c.exts, c.T0s, fe, **kw)
    if c.kind == "int":
        return check_int(mantis, lm, c.frames, c.exts, c.T0s, fi, c.mask, slot_guard=LC.int_slot_guard, cap=cap,
                         gap_span=_gap_span(c), **kw)
    return check_rig(mantis, lm, c.frames, c.exts, c.T0s, fe, fi, c.mask, slot_guard=LC.rig_slot_guard, cap=cap,
                     gap_span=_gap_span(c), **kw)


@pytest.mark.parametrize("cell", _calib_cells(), ids=lambda c: f"{c[0]}-{c[1]}-{c[2]:#x}")
def test_calibration_cell(mantis, lm, cell):
    kind, name, mask = cell
    c = get_calib_cell(kind, name, mask)
    T_out, res = _calibrate(mantis, lm, c)
    print(cell, res.status, res.calibrated, res.iterations_run, list(res.n_obs)[:5])
    if c.guarded:
        want = OK if name == "mixed" or mask != 0xFF else calib_status(kind, name)
        assert (res.status, res.calibrated, res.iterations_run) == want
        assert list(res.n_obs) == list(c.host.n_obs)
    if mask == 0xF0:
        kd = IR.kds_of(res)
        assert kd[:, :4].tobytes() == np.ascontiguousarray(c.kds[:, :4]).tobytes()
        assert np.all(kd[:, 4:6] != c.kds[:, 4:6])


def test_no_tangent_in_all_four_kernels(mantis, lm):
    """The degenerate pose whose every slot is code 2: each call starves in pass 0 with its inputs unchanged."""
    T = LC.no_tangent_pose()
    black = np.zeros((240, 320, 3), np.uint8)
    Ks, Ds = _lenses([LC.kd_of("bench", 320, 240)] * 2)
    I2 = [np.eye(4), np.eye(4)]
    res = check_refine(mantis, lm, [black], I2[:1], T, Ks=Ks[:1], Ds=Ds[:1])
    codes = mantis.refine_record(0, 0)[1]
    assert np.all(codes == 2) and codes.shape == (NC,) and (res.status, res.n_obs[0]) == (1, 0)
    T_out, res = check_ext(mantis, lm, [[black, black]], I2, [T], 0b10, Ks=Ks, Ds=Ds)
    codes = mantis.calib_record(0, 0)[2]
    assert np.all(codes == 2) and codes.shape == (2 * NC,) and res.status == 1 and np.array_equal(T_out[0], T)
    T_out, res = check_int(mantis, lm, [[black]], I2[:1], [T], 0b1, Ks=Ks[:1], Ds=Ds[:1])
    codes = mantis.icalib_record(0, 0)[2]
    assert np.all(codes == 2) and codes.shape == (NC,) and res.status == 1 and np.array_equal(T_out[0], T)
    T_out, res = check_rig(mantis, lm, [[black, black]], I2, [T], 0b10, 0b11, Ks=Ks, Ds=Ds)
    codes = mantis.rcalib_record(0, 0)[3]
    assert np.all(codes == 2) and codes.shape == (2 * NC,) and res.status == 1 and np.array_equal(T_out[0], T)


def test_on_axis_slot(mantis, lm):
    """rho <= 1e-8 in jint on the device, in both kernels that call it: J_int = [0, 0, nh0, nh1, 0, 0, 0, 0]
    within 1e-15 and the slot's other entries the host's. The camera stands straight above a landmark with
    cx = 159.5: the 27 candidates of its grid line have a sample on u = 0 * cdist * fx + cx exactly, a tie by the
    rule's flag and the same bits on both sides (no atan in it), more than the checkers' cap of flagged slots.
    So the record is compared here, every slot of it, ties included."""
    from test_gpu_icalib import _images as int_images
    from test_gpu_rcalib import _images as rig_images

    X, nw, nr, ng = lm
    f = RR.flags(X, 0.08)
    T, E, kd, img, k, nh = LC.on_axis_case()
    Ks, Ds = _lenses([kd, kd])
    want = [0, 0, nh[0], nh[1], 0, 0, 0, 0]
    T_out, res = mantis.calibrate_intrinsics(int_images([[img]], [E], Ks=Ks[:1], Ds=Ds[:1]), 1, np.array([T]), 0b1,
                                             record=1)
    _, KD, codes, Sw, Skw, rows, _ = mantis.icalib_record(0, 0)
    hc_, hSw, hSkw, hrows, _ = IR.obs(T, E, kd, img, X, nw, nr, ng, f, True)
    assert np.array_equal(KD[0], kd) and np.array_equal(codes, hc_) and codes[k] == 0
    assert np.array_equal(Sw, hSw) and np.array_equal(Skw, hSkw)
    np.testing.assert_allclose(rows, hrows, rtol=1e-12, atol=0)
    np.testing.assert_allclose(rows[k, 6:14], want, rtol=0, atol=1e-15)
    assert rows[k, 14] != 0 and res.n_obs[0] == (hc_ == 0).sum() > 0
    T_out, res = mantis.calibrate_rig(rig_images([[img, img]], [E, E], Ks=Ks, Ds=Ds), 1, np.array([T]), 0b10, 0b11,
                                      record=1)
    _, _, KD, codes, Sw, Skw, rows, _ = mantis.rcalib_record(0, 0)
    for cam in range(2):
        hc_, hSw, hSkw, hrows, _ = QR.obs(T, E, kd, img, X, nw, nr, ng, f, cam == 1, True)
        sl = slice(cam * NC, (cam + 1) * NC)
        assert np.array_equal(codes[sl], hc_) and np.array_equal(Sw[sl], hSw) and np.array_equal(Skw[sl], hSkw)
        np.testing.assert_allclose(rows[sl], hrows, rtol=1e-12, atol=0)
        np.testing.assert_allclose(rows[sl][k, 12:20], want, rtol=0, atol=1e-15)
        assert codes[sl][k] == 0


@pytest.mark.parametrize("edge", LC.EDGES)
def test_window_at_the_frame_edge(mantis, lm, edge):
    """Code 3 exactly where the host has it, in all four observation kernels (each carries its own copy of the
    in-frame test): the window's last sample a quarter pixel inside the edge is a weak window (code 5) on a
    black frame, a quarter pixel outside it is code 3."""
    black = np.zeros((505, 907, 3), np.uint8)
    I2 = [np.eye(4), np.eye(4)]
    for side, want in (("in", 5), ("out", 3)):
        T, kd, k, target, horizontal = LC.edge_case(edge, side)
        Ks, Ds = _lenses([kd, kd])
        check_refine(mantis, lm, [black], I2[:1], T, Ks=Ks[:1], Ds=Ds[:1])
        got = [mantis.refine_record(0, 0)[1][k]]
        check_ext(mantis, lm, [[black, black]], I2, [T], 0b10, Ks=Ks, Ds=Ds)
        codes = mantis.calib_record(0, 0)[2]
        got += [codes[k], codes[NC + k]]
        check_int(mantis, lm, [[black]], I2[:1], [T], 0b1, Ks=Ks[:1], Ds=Ds[:1])
        got.append(mantis.icalib_record(0, 0)[2][k])
        check_rig(mantis, lm, [[black, black]], I2, [T], 0b10, 0b11, Ks=Ks, Ds=Ds)
        codes = mantis.rcalib_record(0, 0)[3]
        got += [codes[k], codes[NC + k]]
        assert got == [want] * 6, (edge, side, got)
