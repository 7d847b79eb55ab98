"""Case generator of the scoring matrix (test_score_matrix_host.py,
test_gpu_score_matrix.py): lenses, frame sizes, images, masks, poses and maps
beyond the bench camera, deterministic and seeded. A plain helper module.

A cell is (lens, frame size). Its poses are built so that the scorers' decision
paths run: landmarks aimed a quarter pixel inside and outside every frame edge
and corner, a landmark on the optical axis, cameras in and below the floor
plane, cameras that see nothing, arbitrary SE(3) poses and poses near a truth.

The guard. The device's atan may differ from glibc's by an ulp, which moves a
pixel coordinate by <~ 1e-12 px at these focal lengths, so a generated
projection must not lie within GUARD = 1e-9 px (the suite's POSE_TOL) of a
decision threshold: u = 0, u = W, v = 0, v = H, for in-frame points the
rounding ties k + 1/2 of u and v (the ties of the COLOR window u + ox, v + oy
are the same fractional parts), and z = 0 itself. A coordinate whose
camera-frame component is exactly zero is exempt: then x / z = 0 and
u = 0 * cdist * fx + cx = cx bit for bit on every side, with no atan in it (the
on-axis poses put a whole grid row of landmarks there, and cx = W / 2 is a tie
for odd W). If a seed violates the guard the cell moves to the next seed; the
census test asserts the final state.
"""
import functools
import math

import numpy as np

import _oracle as O
from mantis_amd import synth

GUARD = 1e-9
SIZES = [(1280, 720), (907, 505), (130, 35), (33, 7)]
STRONG = [[0.30, -0.20, 0.08, -0.012], [-0.25, 0.06, -0.004, 0.0002], [0.6, -0.5, 0.2, -0.03]]
D_OFF = [-0.9, 0.0, 0.0, 0.0]  # theta_d not monotone on [0, pi/2]: screen_bounds refuses it, the screen is off
LENSES = ["bench", "d0", "strong0", "strong1", "strong2", "off", "x3", "x045", "pp_out"]
# per cell: 10 targets x N_AIM aimed poses (fewer where the image circle ends before the target)
N_AIM, N_AXIS, N_FLOOR, N_BELOW, N_NOTHING, N_ANY, N_NEAR = 4, 8, 8, 6, 8, 56, 44
HALF_PI = 1.5707963267948966


def lens(name, w, h):
    """(K, D): K as the caller would hand it over, not yet rounded to float32
    (the library's cam_from and the oracle's make_cam both round it; fx of the
    scaled lenses and of every size but 1280x720 is not a float32)."""
    K, D = synth.intrinsics(w, h)
    if name == "d0":
        D = np.zeros(4)
    elif name.startswith("strong"):
        D = np.array(STRONG[int(name[-1])], np.float64)
    elif name == "off":
        D = np.array(D_OFF, np.float64)
    elif name == "x3":
        K[0, 0] *= 3.0
        K[1, 1] *= 3.0
    elif name == "x045":
        K[0, 0] *= 0.45
        K[1, 1] *= 0.45
    elif name == "pp_out":
        K[0, 2] = -0.04 * w
        K[1, 2] = 0.6 * h
    else:
        assert name == "bench", name
    return K, D


def k32(K):
    return np.asarray(K, np.float32).astype(np.float64)


# ------------------------------------------------------------------ images
def blob_image(w, h, seed):
    """Coarse random blocks plus Gaussian noise: nearly every pixel differs
    from its neighbours, so a pixel that is off by one changes the sum."""
    rng = np.random.default_rng([seed, w, h])
    base = rng.integers(0, 256, (h // 4 + 2, w // 4 + 2, 3)).astype(np.float64)
    img = np.repeat(np.repeat(base, 4, 0), 4, 1)[:h, :w]
    return np.clip(img + rng.normal(0, 25, img.shape), 0, 255).astype(np.uint8)


def blob_mask(w, h, seed):
    """Random blob mask of about half density; nonzero = keep, and the nonzero
    values are 1, 128 and 255."""
    rng = np.random.default_rng([seed, w, h, 7])
    keep = rng.integers(0, 2, (h // 3 + 2, w // 3 + 2))
    keep = np.repeat(np.repeat(keep, 3, 0), 3, 1)[:h, :w]
    val = np.array([1, 128, 255], np.uint8)[rng.integers(0, 3, (h, w))]
    return np.where(keep != 0, val, 0).astype(np.uint8)


def cleaned(img, mask):
    """The image the reference scores under a mask: masked pixels black."""
    out = img.copy()
    out[mask == 0] = 0
    return out


# -------------------------------------------------------------------- maps
def make_map(n_total, ng, seed=5):
    """(white, red, green) with n_total landmarks, ng of them green: the yaml
    map's landmarks first (white, red, then green up to ng), the rest seeded
    random floor points in +-1.44 m."""
    white, red, green = synth.load_map()
    rng = np.random.default_rng([seed, n_total, ng])
    g = green[:ng]
    if len(g) < ng:
        g = np.vstack([g, np.c_[rng.uniform(-1.44, 1.44, (ng - len(g), 2)), np.zeros(ng - len(g))]])
    rest = n_total - ng
    w = white[:rest]
    r = red[:max(0, rest - len(w))]
    fill = rest - len(w) - len(r)
    if fill > 0:
        w = np.vstack([w, np.c_[rng.uniform(-1.44, 1.44, (fill, 2)), np.zeros(fill)]])
    return (np.ascontiguousarray(w).reshape(-1, 3), np.ascontiguousarray(r).reshape(-1, 3),
            np.ascontiguousarray(g).reshape(-1, 3))


# (name, total, green): one full register trip per half, unequal halves, COLOR
# without green, around one wave, and the smallest maps (wave 0's half of a
# one-landmark map is empty)
MAP_SHAPES = [("yaml", 720, 37), ("m768", 768, 64), ("m767", 767, 37), ("m385", 385, 0), ("m65", 65, 5), ("m64", 64, 5),
              ("m63", 63, 5), ("m2", 2, 1), ("m1", 1, 1)]


@functools.lru_cache(maxsize=None)
def get_map(name):
    if name == "yaml":
        return synth.load_map()
    for nm, n, ng in MAP_SHAPES:
        if nm == name:
            return make_map(n, ng)
    raise KeyError(name)


def landmarks(name):
    return np.vstack([a.reshape(-1, 3) for a in get_map(name)])


# ------------------------------------------------------------------- poses
def theta_branch(D):
    """End of the first increasing branch of theta_d on [0, pi/2): the first
    zero of theta_d' (bisected), or pi/2."""
    k = np.asarray(D, np.float64)

    def dthd(t):
        x = t * t
        return 1 + 3 * k[0] * x + 5 * k[1] * x ** 2 + 7 * k[2] * x ** 3 + 9 * k[3] * x ** 4

    ts = np.linspace(0, HALF_PI, 20001)
    neg = np.nonzero(dthd(ts) <= 0)[0]
    if len(neg) == 0:
        return HALF_PI
    lo, hi = ts[neg[0] - 1], ts[neg[0]]
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if dthd(mid) > 0:
            lo = mid
        else:
            hi = mid
    return lo


def theta_d(t, D):
    x = t * t
    return t * (1 + D[0] * x + D[1] * x ** 2 + D[2] * x ** 3 + D[3] * x ** 4)


def ray_of_pixel(px, py, Kr, D):
    """Unit ray (camera frame) that the lens sends to pixel (px, py), by
    bisection on theta_d's first increasing branch; None outside the image
    circle. (cv::fisheye::undistortPoints clamps theta_d to pi/2 and misses.)"""
    du, dv = (px - Kr[0, 2]) / Kr[0, 0], (py - Kr[1, 2]) / Kr[1, 1]
    td = math.hypot(du, dv)
    tmax = theta_branch(D)
    if td >= theta_d(tmax, D) * (1 - 1e-9):
        return None
    lo, hi = 0.0, tmax
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if theta_d(mid, D) < td:
            lo = mid
        else:
            hi = mid
    th = 0.5 * (lo + hi)
    s = math.sin(th) / td
    return np.array([du * s, dv * s, math.cos(th)])


def _frame(z, roll):
    """Right-handed orthonormal columns [b1, b2, z], rolled about z."""
    z = z / np.linalg.norm(z)
    a = np.array([1.0, 0, 0]) if abs(z[0]) < 0.9 else np.array([0, 1.0, 0])
    b1 = np.cross(a, z)
    b1 /= np.linalg.norm(b1)
    b2 = np.cross(z, b1)
    c, s = math.cos(roll), math.sin(roll)
    return np.stack([c * b1 + s * b2, -s * b1 + c * b2, z], 1)


def aimed_pose(X, C, ray, roll):
    """c2w (12) whose rotation sends X - C along `ray`."""
    A = _frame(X - C, 0.0)
    B = _frame(ray, roll)
    R = B @ A.T  # world -> camera
    return np.concatenate([R.reshape(9), -R @ C])


def targets(w, h):
    mu, mv = w // 2 + 0.3, h // 2 + 0.3
    q = 0.25
    return [(w - q, mv), (q, mv), (mu, q), (mu, h - q), (w - q, h - q), (q, q),
            (-q, mv), (w + q, mv), (mu, -q), (mu, h + q)]


def random_rotations(rng, n):
    Q = rng.normal(size=(n, 4))
    Q /= np.linalg.norm(Q, axis=1)[:, None]
    a, b, c, d = Q.T
    return np.stack([a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c),
                     2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b),
                     2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d], 1).reshape(-1, 3, 3)


def nothing_poses(rng, n):
    """Cameras above the floor looking up: every landmark behind them."""
    out = []
    for _ in range(n):
        Rwc = synth.rot_z(rng.uniform(0, 2 * math.pi)) @ synth.rot_x(rng.uniform(-0.15, 0.15)) @ synth.rot_y(
            rng.uniform(-0.15, 0.15))
        out.append(synth.truth_c2w(Rwc, np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(1.0, 2.0)])))
    return out


def make_poses(name, w, h, lm, seed):
    """(c2w [n, 12], kind [n]) of one cell; kinds: 0 aimed, 1 on the axis,
    2 floor plane, 3 below the floor, 4 sees nothing, 5 arbitrary, 6 near truth."""
    rng = np.random.default_rng([seed, LENSES.index(name), w, h])
    K, D = lens(name, w, h)
    Kr = k32(K)
    c2w, kind = [], []
    for (tu, tv) in targets(w, h):
        ray = ray_of_pixel(tu, tv, Kr, D)
        if ray is None:
            continue
        for _ in range(N_AIM):
            X = lm[rng.integers(len(lm))]
            C = X + np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.8, 2.0)])
            c2w.append(aimed_pose(X, C, ray, rng.uniform(0, 2 * math.pi)))
            kind.append(0)
    for _ in range(N_AXIS):
        X = lm[rng.integers(len(lm))]
        c2w.append(synth.truth_c2w(synth.NADIR, np.array([X[0], X[1], rng.uniform(0.8, 2.0)])))
        kind.append(1)
    for _ in range(N_FLOOR):
        # centre in the floor plane, optical axis horizontal, rolled about it
        phi, roll = rng.uniform(0, 2 * math.pi), rng.uniform(0, 2 * math.pi)
        Rwc = _frame(np.array([math.cos(phi), math.sin(phi), 0.0]), roll)
        c2w.append(synth.truth_c2w(Rwc, np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), 0.0])))
        kind.append(2)
    for _ in range(N_BELOW):
        Rwc = synth.rot_z(rng.uniform(0, 2 * math.pi)) @ synth.rot_x(rng.uniform(-0.6, 0.6)) @ synth.rot_y(
            rng.uniform(-0.6, 0.6))
        c2w.append(synth.truth_c2w(Rwc, np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), -rng.uniform(0.5, 2.0)])))
        kind.append(3)
    c2w += nothing_poses(rng, N_NOTHING)
    kind += [4] * N_NOTHING
    Rr = random_rotations(rng, N_ANY)
    Cc = rng.uniform(-3, 3, (N_ANY, 3))
    for R, C in zip(Rr, Cc):
        c2w.append(np.concatenate([R.reshape(9), -R @ C]))
        kind.append(5)
    for _ in range(N_NEAR):
        R, pos = synth.random_pose(rng)
        Rp = R @ synth.rot_x(rng.normal() * 0.03) @ synth.rot_y(rng.normal() * 0.03) @ synth.rot_z(rng.normal() * 0.03)
        c2w.append(synth.truth_c2w(Rp, pos + rng.normal(size=3) * 0.01))
        kind.append(6)
    return np.array(c2w), np.array(kind)


# ------------------------------------------------------------------ census
class Proj:
    """Reference projection of every (pose, landmark) pair of a pose set:
    camera-frame points (numpy), pixels (the oracle's distort), decisions."""

    def __init__(self, c2w, lm, K, D, w, h):
        c2w = np.asarray(c2w, np.float64).reshape(-1, 12)
        R = c2w[:, :9].reshape(-1, 3, 3)
        self.rp = np.einsum("nij,lj->nli", R, lm) + c2w[:, None, 9:]
        self.n, self.nl, self.w, self.h = len(c2w), len(lm), w, h
        z = self.rp[..., 2]
        safe = self.rp.reshape(-1, 3).copy()
        self.front = (z > 0).reshape(-1)
        safe[~self.front] = [0.0, 0.0, 1.0]  # never projected by the scorers
        uv = O.distort(safe, K, D)
        self.u, self.v = uv[:, 0], uv[:, 1]
        self.inside = self.front & (self.u < w) & (self.v < h) & (self.u >= 0) & (self.v > 0)
        self.ru = np.rint(np.where(self.inside, self.u, 0)).astype(np.int64)
        self.rv = np.rint(np.where(self.inside, self.v, 0)).astype(np.int64)

    def guard_violations(self):
        """Projections within GUARD of a decision threshold (see the module's
        docstring), as a count."""
        rp = self.rp.reshape(-1, 3)
        f = self.front
        ex_u, ex_v = rp[:, 0] == 0.0, rp[:, 1] == 0.0  # u = cx, v = cy exactly
        bad = np.abs(rp[:, 2]) <= GUARD
        du = np.minimum(np.abs(self.u), np.abs(self.u - self.w))
        dv = np.minimum(np.abs(self.v), np.abs(self.v - self.h))
        bad |= f & ~ex_u & (du <= GUARD)
        bad |= f & ~ex_v & (dv <= GUARD)
        tu = np.abs(np.abs(self.u - np.floor(self.u)) - 0.5)
        tv = np.abs(np.abs(self.v - np.floor(self.v)) - 0.5)
        bad |= self.inside & ~ex_u & (tu <= GUARD)
        bad |= self.inside & ~ex_v & (tv <= GUARD)
        return int(bad.sum())

    def counts(self):
        rp = self.rp.reshape(-1, 3)
        ins = self.inside
        r = np.hypot(rp[:, 0], rp[:, 1]) / np.where(self.front, rp[:, 2], 1.0)
        return {
            "u_eq_W": int((ins & (self.ru == self.w)).sum()),
            "u_eq_0": int((ins & (self.ru == 0)).sum()),
            "v_eq_0": int((ins & (self.rv == 0)).sum()),
            "v_eq_H": int((ins & (self.rv == self.h)).sum()),
            "corner_WH": int((ins & (self.ru == self.w) & (self.rv == self.h)).sum()),
            "z_le_0": int((~self.front).sum()),
            "r_gt_1": int((self.front & (r > 1)).sum()),
            "on_axis": int((self.front & (r <= 1e-8)).sum()),
            "hyp_n0": int((ins.reshape(self.n, self.nl).sum(1) == 0).sum()),
        }


class Cell:
    pass


@functools.lru_cache(maxsize=None)
def cell(name, size_idx, map_name="yaml"):
    """The poses of (lens, size) on a map, at the first seed that keeps the
    guard: .K .D .w .h .c2w .kind .seed .seeds_moved .proj"""
    w, h = SIZES[size_idx]
    K, D = lens(name, w, h)
    lm = landmarks(map_name)
    for seed in range(100, 140):
        c2w, kind = make_poses(name, w, h, lm, seed)
        pj = Proj(c2w, lm, K, D, w, h)
        if pj.guard_violations() == 0:
            c = Cell()
            c.name, c.K, c.D, c.w, c.h, c.c2w, c.kind, c.proj = name, K, D, w, h, c2w, kind, pj
            c.seed, c.seeds_moved, c.lm, c.map_name = seed, seed - 100, lm, map_name
            return c
    raise RuntimeError(f"no seed keeps the guard for cell {name} {w}x{h} {map_name}")


def all_cells():
    return [cell(name, si) for name in LENSES for si in range(len(SIZES))]


@functools.lru_cache(maxsize=None)
def nothing_cell(size_idx, n=130):
    """n hypotheses that all see nothing (bench lens)."""
    w, h = SIZES[size_idx]
    K, D = lens("bench", w, h)
    c2w = np.array(nothing_poses(np.random.default_rng([41, w, h]), n))
    pj = Proj(c2w, landmarks("yaml"), K, D, w, h)
    assert pj.guard_violations() == 0 and not pj.inside.any()
    return K, D, w, h, c2w
