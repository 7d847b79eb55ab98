// Stand-alone check of the rig calibration's rules (mantis_amd/csrc/
// mk_linecal.h at the problem Rig: one observation with J_ext and J_int
// against central differences and beside the slots of the problems Ext and
// Int (the two single calibrations' instantiations), the end of a
// pass -- the three-block reduction (poses | extrinsics | intrinsics) against
// a dense solve of the full normal system, both starved gates, both singular
// exits and the diverged exit --, the gate and the covariances, and the whole
// call on painted grids) on small synthetic frames that are allocated at
// exactly their size, as a program of its own so that it can be built with
// sanitizers and run directly:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o build/rcalibcheck tools/rcalibcheck_main.cpp && build/rcalibcheck
// Exit status 0 and "rcalibcheck ok" when every case holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../mantis_amd/csrc/mk_linecal.h"

namespace rf = mk::refine;
namespace cal = mk::calib;
namespace ic = mk::icalib;
namespace lc = mk::linecal;
using rc = lc::Rig;  // the shared rules at the rig calibration's problem

static void rcalib_seq(const double* T_in, const double* Tbc, const mk::Cam* cams, const uint8_t* const* frames, int N,
                       int C, int W, int H, const double* X, int nw, int nr, const int32_t* cand, int n_cand,
                       const mantis_refine_params& p, const mantis_rcalib_params& rp, double* T_out,
                       mantis_rcalib_result& R, rc::Slot* slots) {
  rc::seq(T_in, Tbc, cams, frames, N, C, W, H, X, nw, nr, cand, n_cand, p, (uint32_t)rp.free_ext, (uint32_t)rp.free_int,
          (uint32_t)rp.param_mask, rp.min_obs_cam, T_out, R, slots);
}

static int g_fail = 0;
static bool g_verbose = false;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      g_fail++;                                                      \
    }                                                                \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd64() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}
static double unif() { return (double)(rnd64() >> 11) / 9007199254740992.0; }

// a camera looking straight down from (x, y, h), yawed by a: T_w_b (the camera is the base)
static void nadir_pose(double x, double y, double h, double a, double* T) {
  const double c = std::cos(a), s = std::sin(a);
  const double R[9] = {c, s, 0, s, -c, 0, 0, 0, -1};  // rot_z(a) * diag(1, -1, -1)
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) T[4 * i + j] = R[3 * i + j];
  T[3] = x; T[7] = y; T[11] = h;
  T[12] = T[13] = T[14] = 0; T[15] = 1;
}
// an extrinsic: yaw a about the base's z, then a tilt b about the camera's x, at the offset (x, y, z)
static void ext_pose(double x, double y, double z, double a, double* E, double b = 0.0) {
  const double c = std::cos(a), s = std::sin(a), cb = std::cos(b), sb = std::sin(b);
  const double M[16] = {c, -s * cb, s * sb, x, s, c * cb, -c * sb, y, 0, sb, cb, z, 0, 0, 0, 1};
  std::memcpy(E, M, sizeof(M));
}
static void mul4(const double* A, const double* B, double* C) {
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      double s = 0;
      for (int k = 0; k < 4; k++) s += A[4 * i + k] * B[4 * k + j];
      C[4 * i + j] = s;
    }
}

// paint the lines y = j pitch and x = j pitch (|j| <= m, each from -len to len) of the floor into a W x H frame of a
// camera at T (camera in the world)
static void paint_grid(std::vector<uint8_t>& img, int W, int H, const double* T, const mk::Cam& cam, double pitch, int m,
                       double len) {
  double Rt[9], t[3];
  rf::pose_parts(T, Rt, t);
  for (int fam = 0; fam < 2; fam++)
    for (int j = -m; j <= m; j++)
      for (int i = -4000; i <= 4000; i++) {
        const double a = i * (len / 4000.0), b = j * pitch;
        const double X[3] = {fam == 0 ? a : b, fam == 0 ? b : a, 0.0};
        const double d[3] = {X[0] - t[0], X[1] - t[1], X[2] - t[2]};
        double p[3];
        for (int r = 0; r < 3; r++) p[r] = Rt[3 * r] * d[0] + Rt[3 * r + 1] * d[1] + Rt[3 * r + 2] * d[2];
        if (!(p[2] > 0)) continue;
        double u, v;
        mk::distort(cam, p[0], p[1], p[2], &u, &v);
        if (!(u > -0.5 && u < W - 0.5 && v > -0.5 && v < H - 0.5)) continue;
        const size_t o = 3 * ((size_t)mk::cv_round(v) * W + mk::cv_round(u));
        img.at(o) = img.at(o + 1) = img.at(o + 2) = 255;
      }
}

// m with dist_cam(m) = (u, v), by Newton on the radius
static void undistort(const mk::Cam& cm, double u, double v, double* m) {
  const double px = (u - cm.cx) / cm.fx, py = (v - cm.cy) / cm.fy, rd = std::sqrt(px * px + py * py);
  if (rd < 1e-300) {
    m[0] = m[1] = 0.0;
    return;
  }
  double th = rd;
  for (int it = 0; it < 60; it++) {
    const double t2 = th * th;
    const double f = th * (1 + t2 * (cm.k[0] + t2 * (cm.k[1] + t2 * (cm.k[2] + t2 * cm.k[3])))) - rd;
    const double df = 1 + t2 * (3 * cm.k[0] + t2 * (5 * cm.k[1] + t2 * (7 * cm.k[2] + t2 * 9 * cm.k[3])));
    th -= f / df;
  }
  m[0] = px * (std::tan(th) / rd);
  m[1] = py * (std::tan(th) / rd);
}

// m0 of the landmark X through pose T and extrinsic E
static bool project(const double* T, const double* E, const double* X, int axis, double* m0) {
  double Rt[9], t[3];
  rf::pose_parts(T, Rt, t);
  mk::GnCam gc;
  rf::gncam_from(E, gc);
  cal::Geom g;
  if (cal::geom(Rt, t, gc, X, axis, true, g)) return false;
  m0[0] = g.g.m0[0];
  m0[1] = g.g.m0[1];
  return true;
}

// Windows against frames of exactly W x H x 3 bytes, the candidate pushed over every edge and corner: the rig
// calibration's slot beside the two single calibrations' (bit for bit where the issue says so), and on the live
// slots the 20 Jacobian columns against central differences (step 1e-6, bound 1e-7 of the row's largest entry).
static void check_rows() {
  const int tg[3] = {255, 255, 255};
  int codes_seen[6] = {0}, diffed = 0;
  double worst = 0;
  for (int R : {1, 15, 12})
    for (int size = 0; size < 3; size++) {
      const int W = size == 0 ? 40 : size == 1 ? 97 : 33, H = size == 0 ? 32 : size == 1 ? 61 : 33;
      const mk::Cam cam{60.0, 61.0, W / 2.0 - 0.25, H / 2.0 + 0.125, {0.003, -0.01, 0.005, -0.002}};
      std::vector<uint8_t> img((size_t)W * H * 3);
      double E[16];
      ext_pose(0.01, -0.02, 0.005, 0.2, E, 0.1);
      mk::GnCam gc;
      rf::gncam_from(E, gc);
      for (int trial = 0; trial < 3000; trial++) {
        if (trial % 50 == 0)
          for (auto& b : img) b = (rnd64() & 3) ? (uint8_t)(rnd64() & 0xff) : 255;
        const double h = 0.5 + unif();
        const int edge = trial % 9;
        const double ex = (edge % 3 - 1) * (W / 2.0) / cam.fx, ey = (edge / 3 - 1) * (H / 2.0) / cam.fy;
        const double jx = (unif() - 0.5) * 40.0 / cam.fx, jy = (unif() - 0.5) * 40.0 / cam.fy;
        double T[16];
        nadir_pose(-(ex + jx) * h, (ey + jy) * h, h, (trial % 7) * 0.9, T);
        if (trial % 11 == 0) T[11] = -T[11];  // under the floor: behind the camera
        const double X[3] = {0, 0, 0};
        const int axis = trial & 1;
        const rf::Window win{R, 3 * 64 * 64, trial % 3 ? 24576 : 1, 0};
        double Rt[9], t[3];
        rf::pose_parts(T, Rt, t);
        const uint32_t mask = trial % 5 == 0 ? 0x5Au : 0xFFu;
        lc::Ext::Slot oc;
        lc::Int::Slot oi;
        lc::Ext::observe(Rt, t, gc, cam, img.data(), W, H, X, axis, tg, win, true, false, 0u, oc, nullptr);
        lc::Int::observe(Rt, t, gc, cam, img.data(), W, H, X, axis, tg, win, false, true, mask, oi, nullptr);
        for (int fe = 0; fe < 2; fe++)
          for (int fi = 0; fi < 2; fi++) {
            rc::Slot o;
            int tie;
            rc::observe(Rt, t, gc, cam, img.data(), W, H, X, axis, tg, win, fe != 0, fi != 0, mask, o, &tie);
            CHECK(o.code == oc.code && o.Sw == oc.Sw && o.Skw == oc.Skw && o.pad == 0);
            CHECK(o.code == oi.code && o.Sw == oi.Sw && o.Skw == oi.Skw);
            CHECK(std::memcmp(o.row, oc.row, 6 * sizeof(double)) == 0 && o.row[20] == oc.row[12] && o.row[20] == oi.row[14]);
            if (fe) CHECK(std::memcmp(o.row + 6, oc.row + 6, 6 * sizeof(double)) == 0);
            if (fi) CHECK(std::memcmp(o.row + 12, oi.row + 6, 8 * sizeof(double)) == 0);
            for (int e = 0; e < 20; e++) CHECK(std::isfinite(o.row[e]));
            for (int e = 0; e < 6; e++)
              if (!fe || o.code) CHECK(o.row[6 + e] == 0.0);
            for (int e = 0; e < 8; e++)
              if (!fi || o.code || !(mask >> e & 1u)) CHECK(o.row[12 + e] == 0.0);
            if (o.code) CHECK(o.row[20] == 0.0 && o.row[0] == 0.0);
          }
        codes_seen[oc.code]++;
        if (oc.code || mask != 0xFFu || trial % 20 != 1) continue;
        // central differences on this live slot
        rc::Slot o;
        rc::observe(Rt, t, gc, cam, img.data(), W, H, X, axis, tg, win, true, true, 0xFFu, o, nullptr);
        cal::Geom g;
        (void)cal::geom(Rt, t, gc, X, axis, true, g);
        const double* nh = g.g.nh;
        const double hstep = 1e-6;
        double num[20], big = 0;
        for (int a = 0; a < 12; a++) {
          double d[6] = {0, 0, 0, 0, 0, 0}, mp[2], mm[2], Tp[16], Tm[16];
          const double* base = a < 6 ? T : E;
          std::memcpy(Tp, base, sizeof(Tp));
          std::memcpy(Tm, base, sizeof(Tm));
          d[a % 6] = hstep;
          cal::right_update(Tp, d);
          d[a % 6] = -hstep;
          cal::right_update(Tm, d);
          const bool ok = a < 6 ? project(Tp, E, X, axis, mp) && project(Tm, E, X, axis, mm)
                                : project(T, Tp, X, axis, mp) && project(T, Tm, X, axis, mm);
          CHECK(ok);
          num[a] = (nh[0] * (mp[0] - mm[0]) + nh[1] * (mp[1] - mm[1])) / (2 * hstep);
        }
        double u, v, th[8];
        mk::distort(cam, g.g.m0[0], g.g.m0[1], 1.0, &u, &v);
        ic::cam_to(cam, th);
        for (int a = 0; a < 8; a++) {
          double e[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tp[8], tm[8], mp[2], mm[2];
          e[a] = hstep;
          CHECK(ic::param_update(th, e, 0xFFu, tp));
          e[a] = -hstep;
          CHECK(ic::param_update(th, e, 0xFFu, tm));
          undistort(ic::cam_of(tp, tp + 4), u, v, mp);
          undistort(ic::cam_of(tm, tm + 4), u, v, mm);
          num[12 + a] = -(nh[0] * (mp[0] - mm[0]) + nh[1] * (mp[1] - mm[1])) / (2 * hstep);
        }
        for (int e = 0; e < 20; e++) big = std::fmax(big, std::fabs(o.row[e]));
        for (int e = 0; e < 20; e++) {
          worst = std::fmax(worst, std::fabs(o.row[e] - num[e]) / big);
          CHECK(std::fabs(o.row[e] - num[e]) <= 1e-7 * big);
        }
        diffed++;
      }
    }
  for (int c : {0, 1, 3, 4, 5}) CHECK(codes_seen[c] > 0);
  CHECK(diffed >= 20);
  if (g_verbose)
    std::printf("rows: codes 0..5 seen %d %d %d %d %d %d; %d slots against central differences, worst %.3g of the row\n",
                codes_seen[0], codes_seen[1], codes_seen[2], codes_seen[3], codes_seen[4], codes_seen[5], diffed, worst);
  int n = 0;
  for (int a = 0; a < rc::kRow; a++)
    for (int b = a; b < rc::kRow; b++) CHECK(rc::tri(a, b) == n++);
  CHECK(n == rc::kAcc && rc::tri(20, 20) == 230 && sizeof(rc::Slot) == 184 && rc::kMaxS == 106);
  lc::Layout l;
  rc::layout(0xFEu, 0xFFu, 8, l);
  int cam, col;
  CHECK(l.Fe == 7 && l.Fi == 8 && l.nS == 106);
  rc::unknown(l, 0, cam, col);
  CHECK(cam == 1 && col == 6);
  rc::unknown(l, 41, cam, col);
  CHECK(cam == 7 && col == 11);
  rc::unknown(l, 42, cam, col);
  CHECK(cam == 0 && col == 12);
  rc::unknown(l, 105, cam, col);
  CHECK(cam == 7 && col == 19);
}

static void random_acc(int N, int C, uint32_t fe, uint32_t fi, uint32_t pm, int zero_last_view, int zero_col,
                       double r_scale, std::vector<double>& acc, std::vector<int32_t>& cnt) {
  acc.assign((size_t)N * C * rc::kAcc, 0.0);
  cnt.assign((size_t)N * C, 60);
  for (int r = 0; r < N; r++)
    for (int c = 0; c < C; c++)
      for (int k = 0; k < 60; k++) {
        double row[21];
        for (int e = 0; e < 21; e++) row[e] = unif() - 0.5;
        row[20] *= r_scale;
        for (int e = 0; e < 6; e++)
          if (!(fe >> c & 1)) row[6 + e] = 0.0;
        for (int e = 0; e < 8; e++)
          if (!(fi >> c & 1) || !(pm >> e & 1)) row[12 + e] = 0.0;
        if (zero_last_view >= 0 && r == N - 1) row[zero_last_view] = 0.0;
        if (zero_col >= 0) row[zero_col] = 0.0;
        rc::accumulate_row(row, acc.data() + (size_t)rc::kAcc * (r * C + c));
      }
}

// x with H x = b by Gaussian elimination with partial pivoting (H: n x n row-major, overwritten)
static bool dense_solve(std::vector<double>& Hm, std::vector<double>& b, int n) {
  for (int k = 0; k < n; k++) {
    int piv = k;
    for (int i = k + 1; i < n; i++)
      if (std::fabs(Hm[(size_t)i * n + k]) > std::fabs(Hm[(size_t)piv * n + k])) piv = i;
    if (Hm[(size_t)piv * n + k] == 0.0) return false;
    if (piv != k) {
      for (int j = 0; j < n; j++) std::swap(Hm[(size_t)k * n + j], Hm[(size_t)piv * n + j]);
      std::swap(b[k], b[piv]);
    }
    for (int i = k + 1; i < n; i++) {
      const double f = Hm[(size_t)i * n + k] / Hm[(size_t)k * n + k];
      for (int j = k; j < n; j++) Hm[(size_t)i * n + j] -= f * Hm[(size_t)k * n + j];
      b[i] -= f * b[k];
    }
  }
  for (int i = n - 1; i >= 0; i--) {
    double s = b[i];
    for (int j = i + 1; j < n; j++) s -= Hm[(size_t)i * n + j] * b[j];
    b[i] = s / Hm[(size_t)i * n + i];
  }
  return true;
}

// the end of a pass on given accumulators: the step against a dense solve of the full normal system over
// [poses | extrinsics | intrinsics], both starved gates, both singular exits, the diverged exit, the final pass,
// the gate and the covariances
static void check_passes() {
  const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const double K0[4] = {300.0, 301.0, 320.0, 240.0}, D0[4] = {0.003, -0.01, 0.005, -0.002};
  for (int shape = 0; shape < 5; shape++) {
    const int N = shape == 0 ? 2 : 3, C = shape == 0 ? 2 : shape <= 2 ? 4 : 8;
    const uint32_t fe = shape == 0 ? 0x2u : shape == 1 ? 0x8u : shape == 2 ? 0x4u : 0xFEu;
    const uint32_t fi = shape == 0 ? 0x3u : shape == 1 ? 0x1u : shape == 2 ? 0x4u : 0xFFu;
    const uint32_t pm = shape == 4 ? 0x3Fu : 0xFFu;
    const double lam = shape == 3 ? 1e-3 : 0.0;
    lc::Layout l;
    rc::layout(fe, fi, C, l);
    const int nS = l.nS, nF = 6 * N + nS;
    int np = 0;
    for (int e = 0; e < 8; e++) np += (int)(pm >> e & 1u);
    std::vector<double> acc, T0((size_t)16 * N), T, E0((size_t)16 * C);
    std::vector<int32_t> cnt;
    for (int r = 0; r < N; r++) std::memcpy(T0.data() + 16 * r, I4, sizeof(I4));
    for (int c = 0; c < C; c++) ext_pose(0.1 * c, -0.05 * c, 0.02, 0.7 * c, E0.data() + 16 * c, 0.3);
    auto fresh = [&](mantis_rcalib_result& R) {
      R = mantis_rcalib_result{};
      for (int c = 0; c < C; c++) {
        std::memcpy(R.K[c], K0, sizeof(K0));
        std::memcpy(R.D[c], D0, sizeof(D0));
        std::memcpy(R.T_base_cam[c], E0.data() + 16 * c, 16 * sizeof(double));
      }
      T = T0;
    };
    auto same_rig = [&](const mantis_rcalib_result& R) {
      for (int c = 0; c < C; c++)
        if (std::memcmp(R.K[c], K0, sizeof(K0)) || std::memcmp(R.D[c], D0, sizeof(D0)) ||
            std::memcmp(R.T_base_cam[c], E0.data() + 16 * c, 16 * sizeof(double)))
          return false;
      return true;
    };
    auto no_steps = [&](const mantis_rcalib_result& R) {
      for (int c = 0; c < 8; c++) {
        for (int e = 0; e < 6; e++)
          if (R.delta_ext[0][c][e] != 0.0) return false;
        for (int e = 0; e < 8; e++)
          if (R.delta_int[0][c][e] != 0.0) return false;
      }
      return true;
    };
    mantis_rcalib_result R;
    std::vector<double> delta((size_t)6 * N);
    // a step against the dense solve of the full system
    random_acc(N, C, fe, fi, pm, -1, -1, 0.01, acc, cnt);
    fresh(R);
    CHECK(!rc::end_pass(acc.data(), cnt.data(), N, C, fe, fi, pm, 0, 4, 12, 14, lam, T.data(), R, delta.data()));
    CHECK(R.status == lc::kOk && R.iterations_run == 1 && R.n_obs[0] == 60 * N * C && R.n_obs_cam[0][C - 1] == 60 * N);
    std::vector<double> Hm((size_t)nF * nF, 0.0), g((size_t)nF, 0.0);
    for (int r = 0; r < N; r++)
      for (int c = 0; c < C; c++) {
        const double* a = acc.data() + (size_t)rc::kAcc * (r * C + c);
        int idx[20], col[20], m = 0;
        for (int e = 0; e < 6; e++) { idx[m] = 6 * r + e; col[m++] = e; }
        for (int j = 0; j < nS; j++) {
          int cam, cc;
          rc::unknown(l, j, cam, cc);
          if (cam == c) { idx[m] = 6 * N + j; col[m++] = cc; }
        }
        for (int x = 0; x < m; x++) {
          for (int y = 0; y < m; y++) Hm[(size_t)idx[x] * nF + idx[y]] += a[rc::tri_sym(col[x], col[y])];
          g[idx[x]] -= a[rc::tri(col[x], 20)];
        }
      }
    for (int i = 0; i < nF; i++) Hm[(size_t)i * nF + i] += lam;
    for (int j = 0; j < nS; j++) {
      int cam, cc;
      rc::unknown(l, j, cam, cc);
      if (cc >= 12 && !(pm >> (cc - 12) & 1u)) Hm[(size_t)(6 * N + j) * nF + 6 * N + j] = 1.0;
    }
    CHECK(dense_solve(Hm, g, nF));
    double err = 0, nx = 0;
    for (int i = 0; i < 6 * N; i++) {
      err += (delta[i] - g[i]) * (delta[i] - g[i]);
      nx += g[i] * g[i];
    }
    for (int j = 0; j < nS; j++) {
      int cam, cc;
      rc::unknown(l, j, cam, cc);
      const double got = cc < 12 ? R.delta_ext[0][cam][cc - 6] : R.delta_int[0][cam][cc - 12];
      err += (got - g[6 * N + j]) * (got - g[6 * N + j]);
      nx += g[6 * N + j] * g[6 * N + j];
    }
    if (g_verbose)
      std::printf("passes N=%d C=%d ext=%#x int=%#x mask=%#x nS=%d: |x| %.3g, against the dense solve %.3g\n", N, C, fe, fi,
                  pm, nS, std::sqrt(nx), std::sqrt(err));
    CHECK(std::sqrt(err) <= 1e-10 * std::sqrt(nx));
    for (int c = 0; c < C; c++) {
      const bool xe = (fe >> c & 1u) != 0, xi = (fi >> c & 1u) != 0;
      const double* e = R.delta_int[0][c];
      CHECK(R.K[c][0] == (xi && (pm & 1u) ? K0[0] * (1.0 + e[0]) : K0[0]));
      CHECK(R.K[c][2] == (xi && (pm & 4u) ? K0[2] + K0[0] * e[2] : K0[2]));
      CHECK(R.D[c][3] == (xi && (pm & 128u) ? D0[3] + e[7] : D0[3]));
      double want[16];
      std::memcpy(want, E0.data() + 16 * c, sizeof(want));
      if (xe) cal::right_update(want, R.delta_ext[0][c]);
      CHECK(std::memcmp(want, R.T_base_cam[c], sizeof(want)) == 0);
      CHECK(xe == (R.delta_ext[0][c][0] != 0.0));
    }
    // the gate and the covariances on the same accumulators
    fresh(R);
    (void)rc::end_pass(acc.data(), cnt.data(), N, C, fe, fi, pm, 0, 0, 12, 14, 0.0, T.data(), R, nullptr);  // the figures
    rc::conclude(acc.data(), cnt.data(), N, C, fe, fi, pm, 12, 14, 0.0, R);
    CHECK(R.calibrated == 1);
    for (int c = 0; c < 8; c++) {
      for (int i = 0; i < 6; i++) {
        const bool fr = c < C && (fe >> c & 1);
        CHECK(fr ? R.cov_ext[c][7 * i] > 0 : R.cov_ext[c][7 * i] == 0.0);
        for (int j = 0; j < 6; j++) {
          CHECK(R.cov_ext[c][6 * i + j] == R.cov_ext[c][6 * j + i]);
          if (!fr) CHECK(R.cov_ext[c][6 * i + j] == 0.0);
        }
      }
      for (int i = 0; i < 8; i++) {
        const bool fr = c < C && (fi >> c & 1) && (pm >> i & 1);
        CHECK(fr ? R.cov_int[c][9 * i] > 0 : R.cov_int[c][9 * i] == 0.0);
        for (int j = 0; j < 8; j++) {
          CHECK(R.cov_int[c][8 * i + j] == R.cov_int[c][8 * j + i]);
          if (!fr) CHECK(R.cov_int[c][8 * i + j] == 0.0);
        }
      }
    }
    rc::conclude(acc.data(), cnt.data(), N, C, fe, fi, pm, 12, 14, 1e-12, R);  // a gate no rms passes
    CHECK(R.calibrated == 0 && R.cov_ext[C - 1][0] == 0.0 && R.cov_int[C - 1][0] == 0.0);
    // the final pass solves nothing, whatever the system
    fresh(R);
    CHECK(rc::end_pass(acc.data(), cnt.data(), N, C, fe, fi, pm, 4, 4, 12, 14, 0.0, T.data(), R, nullptr));
    CHECK(R.status == lc::kOk && R.n_obs[4] == 60 * N * C && T == T0 && same_rig(R));
    // starved: a view below min_obs, then a camera free in either mask below min_obs_cam
    fresh(R);
    CHECK(rc::end_pass(acc.data(), cnt.data(), N, C, fe, fi, pm, 0, 4, 60 * C + 1, 14, 0.0, T.data(), R, nullptr));
    CHECK(R.status == lc::kStarved && R.iterations_run == 0 && T == T0 && same_rig(R));
    for (int c = 0; c < C; c++) {
      std::vector<int32_t> few = cnt;
      for (int r = 0; r < N; r++) few[r * C + c] = 4;  // 4 N < 14 rows of camera c, every view still above min_obs
      fresh(R);
      const bool fin = rc::end_pass(acc.data(), few.data(), N, C, fe, fi, pm, 0, 4, 12, 14, 0.0, T.data(), R, nullptr);
      const bool gated = ((fe | fi) >> c & 1u) != 0;
      CHECK(fin == gated && (R.status == lc::kStarved) == gated);
    }
    // singular A_r: the last view sees nothing of one pose direction
    random_acc(N, C, fe, fi, pm, 2, -1, 0.01, acc, cnt);
    fresh(R);
    CHECK(rc::end_pass(acc.data(), cnt.data(), N, C, fe, fi, pm, 0, 4, 12, 14, 0.0, T.data(), R, nullptr));
    CHECK(R.status == lc::kSingular && R.iterations_run == 0 && T == T0 && same_rig(R) && no_steps(R));
    CHECK(!rc::end_pass(acc.data(), cnt.data(), N, C, fe, fi, pm, 0, 4, 12, 14, 1e-3, T.data(), (fresh(R), R), nullptr));  // damped
    // singular S: A_r fine, one extrinsic direction, then one free intrinsic, unseen by every row
    for (int zc : {8, 15}) {
      random_acc(N, C, fe, fi, pm, -1, zc, 0.01, acc, cnt);
      fresh(R);
      CHECK(rc::end_pass(acc.data(), cnt.data(), N, C, fe, fi, pm, 0, 4, 12, 14, 0.0, T.data(), R, nullptr));
      CHECK(R.status == lc::kSingular && R.iterations_run == 0 && T == T0 && same_rig(R) && no_steps(R));
      R.status = lc::kOk;
      rc::conclude(acc.data(), cnt.data(), N, C, fe, fi, pm, 12, 14, 0.0, R);
      CHECK(R.calibrated == 0 && R.cov_int[C - 1][0] == 0.0);
    }
    // ... and the same accumulators with that parameter held: its diagonal is 1, the step is taken
    fresh(R);
    CHECK(!rc::end_pass(acc.data(), cnt.data(), N, C, fe, fi, pm & ~8u, 0, 4, 12, 14, 0.0, T.data(), R, nullptr));
    CHECK(R.status == lc::kOk && R.K[C - 1][3] == K0[3]);
    // diverged: residuals a thousand times the Jacobian's entries push some fx (1 + eps) or fy below zero. The
    // same rows with r negated negate eps, so of the two signs at least one drives camera fi[0]'s fx below zero.
    int diverged = 0;
    const uint64_t rng0 = g_rng;
    for (double sign : {1.0, -1.0}) {
      g_rng = rng0;
      random_acc(N, C, fe, fi, pm, -1, -1, sign * 1e3, acc, cnt);
      fresh(R);
      const bool fin = rc::end_pass(acc.data(), cnt.data(), N, C, fe, fi, pm, 0, 4, 12, 14, 0.0, T.data(), R, delta.data());
      CHECK(fin == (R.status == lc::kDiverged));
      if (!fin) continue;
      diverged++;
      CHECK(R.iterations_run == 0 && T == T0 && same_rig(R) && no_steps(R));
      rc::conclude(acc.data(), cnt.data(), N, C, fe, fi, pm, 12, 14, 0.0, R);
      CHECK(R.calibrated == 0);
    }
    CHECK(diverged >= 1);
  }
  // no row at all: rms is 0, not 0 / 0
  std::vector<double> acc((size_t)2 * rc::kAcc, 0.0), T(I4, I4 + 16);
  std::vector<int32_t> cnt(2, 0);
  mantis_rcalib_result R{};
  CHECK(rc::end_pass(acc.data(), cnt.data(), 1, 2, 2u, 3u, 0xFFu, 0, 4, 12, 14, 0.0, T.data(), R, nullptr));
  CHECK(R.status == lc::kStarved && R.rms[0] == 0.0 && R.n_obs[0] == 0);
  rc::conclude(acc.data(), cnt.data(), 1, 2, 2u, 3u, 0xFFu, 12, 14, 0.0, R);
  CHECK(R.calibrated == 0 && R.rms_cam[1] == 0.0);
}

// rms over a grid of normalized points of |dist_a - dist_b|, in pixels
static double model_gap(const mk::Cam& a, const mk::Cam& b) {
  double s = 0;
  int n = 0;
  for (int i = -8; i <= 8; i++)
    for (int j = -6; j <= 6; j++) {
      double ua, va, ub, vb;
      mk::distort(a, i * 0.08, j * 0.08, 1.0, &ua, &va);
      mk::distort(b, i * 0.08, j * 0.08, 1.0, &ub, &vb);
      s += (ua - ub) * (ua - ub) + (va - vb) * (va - vb);
      n++;
    }
  return std::sqrt(s / n);
}
static double ext_gap(const double* A, const double* B) {
  double s = 0;
  for (int i = 0; i < 3; i++) s += (A[4 * i + 3] - B[4 * i + 3]) * (A[4 * i + 3] - B[4 * i + 3]);
  return std::sqrt(s);
}

// the whole call on painted grids: N views of a rig of C tilted cameras, every camera rendered through intrinsics
// beside the nominal ones and every camera but the first through an extrinsic beside the nominal one
static void check_seq() {
  const int W = 320, H = 240;
  const mk::Cam nominal{150.0, 150.0, 159.5, 119.5, {0.003, -0.01, 0.005, -0.002}};
  const double pitch = 0.08;
  std::vector<double> X;  // landmarks every pitch / 2 along the lines every 2 pitch: candidates and intersections
  for (int j = -4; j <= 4; j += 2)
    for (int i = -8; i <= 8; i++) {
      X.insert(X.end(), {i * pitch * 0.5, j * pitch, 0.0});
      if (i % 4) X.insert(X.end(), {j * pitch, i * pitch * 0.5, 0.0});
    }
  const int n = (int)X.size() / 3;
  std::vector<uint8_t> flags(n);
  rf::line_flags(X.data(), n, pitch * 0.5, flags.data());
  std::vector<int32_t> cand(n);
  const int nc = rf::candidates(flags.data(), n, cand.data());
  CHECK(nc > 40);
  for (int shape = 0; shape < 3; shape++) {
    const int N = shape == 0 ? 2 : 4, C = shape == 0 ? 2 : shape == 1 ? 4 : 8;
    const uint32_t all = (1u << C) - 1u, fe = all & ~1u, fi = all, pm = 0x0Fu;  // K only on these small frames
    const int Rw = shape == 2 ? 15 : 6;
    std::vector<double> E((size_t)16 * C), Et((size_t)16 * C), T_true((size_t)16 * N), T0((size_t)16 * N),
        T_out((size_t)16 * N);
    std::vector<mk::Cam> truth(C, nominal), cams(C, nominal);
    for (int c = 0; c < C; c++) {
      // tilted: a camera that looks straight down at a plane cannot tell its focal length from its height
      ext_pose(0.012 * c - 0.03, 0.01 * (c % 3) - 0.01, 0.0, 0.7 * c, E.data() + 16 * c, 0.45);
      std::memcpy(Et.data() + 16 * c, E.data() + 16 * c, 16 * sizeof(double));
      if (c) {
        const double d[6] = {c % 2 ? 0.004 : -0.004, c % 3 ? -0.003 : 0.003, 0.002, 0.004, c % 2 ? -0.003 : 0.003, 0.002};
        cal::right_update(Et.data() + 16 * c, d);
      }
      truth[c].fx *= 1.0 + (c % 2 ? 0.008 : -0.008);
      truth[c].fy *= 1.0 + (c % 3 ? -0.008 : 0.008);
      truth[c].cx += c % 2 ? 1.0 : -1.0;
      truth[c].cy += c % 4 < 2 ? 1.0 : -1.0;
    }
    std::vector<std::vector<uint8_t>> imgs((size_t)N * C, std::vector<uint8_t>((size_t)W * H * 3, 0));
    std::vector<const uint8_t*> frames((size_t)N * C);
    for (int r = 0; r < N; r++) {
      // the base tilted differently in every view, at different heights: what separates focal length, height
      // and the extrinsics' offsets on a planar map
      double Tn[16], Tt[16];
      nadir_pose(0.03 - 0.02 * r, -0.02 + 0.015 * r, 0.5 + 0.08 * r, 0.3 + 0.4 * r, Tn);
      ext_pose(0, 0, 0, 0.0, Tt, -0.3 + 0.2 * r);
      mul4(Tn, Tt, T_true.data() + 16 * r);
      const double d0[6] = {0.003, -0.003, 0.001, 0.002, -0.001, 0.003};
      std::memcpy(T0.data() + 16 * r, T_true.data() + 16 * r, 16 * sizeof(double));
      cal::right_update(T0.data() + 16 * r, d0);
      for (int c = 0; c < C; c++) {
        double Twc[16];
        mul4(T_true.data() + 16 * r, Et.data() + 16 * c, Twc);
        paint_grid(imgs[r * C + c], W, H, Twc, truth[c], 2 * pitch, 2, 4 * pitch);
        frames[r * C + c] = imgs[r * C + c].data();
      }
    }
    mantis_refine_params p{};
    p.struct_size = sizeof(p);
    p.iterations = 6;
    p.half_window = Rw;
    p.white_thresh = 3 * 64 * 64;
    p.min_weight = 12288;
    p.min_obs = 12;
    p.lambda = 1e-6;
    p.landmark_pitch = pitch * 0.5;
    mantis_rcalib_params rp{(int32_t)sizeof(mantis_rcalib_params), (int32_t)fe, (int32_t)fi, (int32_t)pm, 14, 0};
    mantis_rcalib_result res;
    std::vector<rc::Slot> slots((size_t)N * C * nc);
    rcalib_seq(T0.data(), E.data(), cams.data(), frames.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p, rp,
                   T_out.data(), res, slots.data());
    double g0 = 0, g1 = 0, e0 = 0, e1 = 0;
    for (int c = 0; c < C; c++) {
      g0 = std::fmax(g0, model_gap(cams[c], truth[c]));
      g1 = std::fmax(g1, model_gap(ic::cam_of(res.K[c], res.D[c]), truth[c]));
      e0 = std::fmax(e0, ext_gap(E.data() + 16 * c, Et.data() + 16 * c));
      e1 = std::fmax(e1, ext_gap(res.T_base_cam[c], Et.data() + 16 * c));
    }
    if (g_verbose)
      std::printf("seq N=%d C=%d R=%d: status %d calibrated %d runs %d n_obs %d..%d  worst gap %.3f -> %.3f px  worst extrinsic "
                  "%.2f -> %.2f mm  rms %.3g -> %.3g\n",
                  N, C, Rw, res.status, res.calibrated, res.iterations_run, res.n_obs[0], res.n_obs[res.iterations_run], g0,
                  g1, 1e3 * e0, 1e3 * e1, res.rms[0], res.rms[res.iterations_run]);
    CHECK(res.status == lc::kOk && res.iterations_run == 6 && res.n_cand == nc && res.n_rigs == N && res.n_cams == C);
    CHECK(res.free_ext == (int32_t)fe && res.free_int == (int32_t)fi && res.param_mask == (int32_t)pm);
    CHECK(res.calibrated == 1 && g1 < g0 && e1 < e0 && res.rms[6] < res.rms[0]);
    CHECK(std::memcmp(res.T_base_cam[0], E.data(), 16 * sizeof(double)) == 0);  // the gauge
    for (int c = 0; c < C; c++)
      for (int e = 0; e < 4; e++) CHECK(res.D[c][e] == nominal.k[e]);
    for (int c = C; c < 8; c++)
      for (int e = 0; e < 4; e++) CHECK(res.K[c][e] == 0.0 && res.D[c][e] == 0.0 && res.T_base_cam[c][e] == 0.0);
    for (size_t k = 0; k < slots.size(); k++)
      if (slots[k].code)
        for (int e = 0; e < 21; e++) CHECK(slots[k].row[e] == 0.0);
    // I = 0: every pose, extrinsic and intrinsic comes back bit for bit
    p.iterations = 0;
    rcalib_seq(T0.data(), E.data(), cams.data(), frames.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p, rp,
                   T_out.data(), res, nullptr);
    CHECK(std::memcmp(T_out.data(), T0.data(), sizeof(double) * 16 * N) == 0 && res.iterations_run == 0);
    for (int c = 0; c < C; c++) {
      double th[8];
      ic::cam_to(nominal, th);
      CHECK(std::memcmp(res.K[c], th, 4 * sizeof(double)) == 0 && std::memcmp(res.D[c], th + 4, 4 * sizeof(double)) == 0);
      CHECK(std::memcmp(res.T_base_cam[c], E.data() + 16 * c, 16 * sizeof(double)) == 0);
    }
    // R = 1: three samples; whatever the rule says, finite
    p.iterations = 3;
    p.half_window = 1;
    rcalib_seq(T_true.data(), Et.data(), truth.data(), frames.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p,
                   rp, T_out.data(), res, nullptr);
    for (size_t e = 0; e < T_out.size(); e++) CHECK(std::isfinite(T_out[e]));
    for (int c = 0; c < C; c++) {
      for (int e = 0; e < 4; e++) CHECK(std::isfinite(res.K[c][e]) && std::isfinite(res.D[c][e]));
      for (int e = 0; e < 16; e++) CHECK(std::isfinite(res.T_base_cam[c][e]));
    }
    // starved: the last view black (a view's gate), then the last camera black in every view (a camera's)
    p.half_window = 6;
    std::vector<uint8_t> black((size_t)W * H * 3, 0);
    std::vector<const uint8_t*> fb = frames;
    for (int c = 0; c < C; c++) fb[(N - 1) * C + c] = black.data();
    rcalib_seq(T0.data(), E.data(), cams.data(), fb.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p, rp,
                   T_out.data(), res, nullptr);
    CHECK(res.status == lc::kStarved && res.calibrated == 0 && std::memcmp(T_out.data(), T0.data(), sizeof(double) * 16 * N) == 0);
    fb = frames;
    for (int r = 0; r < N; r++) fb[r * C + C - 1] = black.data();
    rcalib_seq(T0.data(), E.data(), cams.data(), fb.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p, rp,
                   T_out.data(), res, nullptr);
    CHECK(res.status == lc::kStarved && res.n_obs_cam[0][C - 1] == 0 && res.n_obs[0] > 12 * N);
    CHECK(res.K[C - 1][0] == nominal.fx);
    // no candidates at all
    rcalib_seq(T0.data(), E.data(), cams.data(), frames.data(), N, C, W, H, X.data(), n, 0, cand.data(), 0, p, rp,
                   T_out.data(), res, nullptr);
    CHECK(res.status == lc::kStarved && res.rms[0] == 0.0);
  }
}

int main(int argc, char** argv) {
  g_verbose = argc > 1 && std::strcmp(argv[1], "-v") == 0;
  check_rows();
  check_passes();
  check_seq();
  if (g_fail) {
    std::printf("rcalibcheck: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("rcalibcheck ok\n");
  return 0;
}
