// Stand-alone check of the intrinsic calibration's rules (mantis_amd/csrc/
// mk_linecal.h at the problem Int, mk_icalib.h: one observation with its window over the frame edges and the
// intrinsics' columns, the end of a pass with both starved gates, both
// singular exits and the diverged exit, the gate and the covariance, the
// whole call for N = 1 and 3 views, C = 1 and 8 cameras with all free, R = 1,
// 12 and 15) on small synthetic frames that are allocated at exactly their
// size, as a program of its own so that it can be built with sanitizers and
// run directly:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o build/icalibcheck tools/icalibcheck_main.cpp && build/icalibcheck
// Exit status 0 and "icalibcheck ok" when every case holds.
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
using xi = lc::Int;  // the shared rules at the intrinsic calibration's problem

// the shared rules on the intrinsic calibration's public struct
static bool end_pass(const double* acc, const int32_t* cnt, int N, int C, uint32_t fm, uint32_t pm, int pass, int I,
                     int32_t min_obs, int32_t min_obs_cam, double lambda, double* T, mantis_icalib_result& R,
                     double* delta) {
  return lc::with_state(R, [&](mantis_rcalib_result& w) {
    return xi::end_pass(acc, cnt, N, C, 0u, fm, pm, pass, I, min_obs, min_obs_cam, lambda, T, w, delta);
  });
}
static void conclude(const double* acc, const int32_t* cnt, int N, int C, uint32_t fm, uint32_t pm, int32_t min_obs,
                     int32_t min_obs_cam, double max_rms, mantis_icalib_result& R) {
  lc::with_state(R, [&](mantis_rcalib_result& w) {
    xi::conclude(acc, cnt, N, C, 0u, fm, pm, min_obs, min_obs_cam, max_rms, w);
  });
}
static void icalib_seq(const double* T_in, const double* Tbc, const mk::Cam* cams, const uint8_t* const* frames, int N,
                       int C, int W, int H, const double* X, int nw, int nr, const int32_t* cand, int n_cand,
                       const mantis_refine_params& p, const mantis_icalib_params& ip, double* T_out,
                       mantis_icalib_result& R, xi::Slot* slots) {
  mantis_rcalib_result w;
  xi::seq(T_in, Tbc, cams, frames, N, C, W, H, X, nw, nr, cand, n_cand, p, 0u, (uint32_t)ip.free_cams,
          (uint32_t)ip.param_mask, ip.min_obs_cam, T_out, w, slots);
  lc::narrow(w, R);
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

// windows against frames of exactly W x H x 3 bytes, the candidate pushed over every edge and corner: the
// calibration's slot is the refinement's with the intrinsics' columns between J and r
static void check_windows() {
  const int tg[3] = {255, 255, 255};
  int codes_seen[6] = {0};
  for (int R : {1, 15, 12})
    for (int size = 0; size < 3; size++) {
      const int W = size == 0 ? 40 : size == 1 ? 97 : 33, H = size == 0 ? 32 : size == 1 ? 61 : 33;
      const mk::Cam cam{60.0, 61.0, W / 2.0 - 0.25, H / 2.0 + 0.125, {0.003, -0.01, 0.005, -0.002}};
      std::vector<uint8_t> img((size_t)W * H * 3);
      double E[16];
      ext_pose(0.01, -0.02, 0.005, 0.2, E);
      mk::GnCam gc;
      rf::gncam_from(E, gc);
      for (int trial = 0; trial < 4000; trial++) {
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
        const rf::Window win{R, 3 * 64 * 64, trial % 3 ? 24576 : 1, 0};
        double Rt[9], t[3];
        rf::pose_parts(T, Rt, t);
        rf::Slot o7;
        rf::observe(Rt, t, gc, cam, img.data(), W, H, X, trial & 1, tg, win, o7, nullptr);
        const uint32_t mask = trial % 5 == 0 ? 0x5Au : 0xFFu;
        for (int fr = 0; fr < 2; fr++) {
          xi::Slot o;
          int tie;
          xi::observe(Rt, t, gc, cam, img.data(), W, H, X, trial & 1, tg, win, false, fr != 0, mask, o, &tie);
          CHECK(o.code == o7.code && o.Sw == o7.Sw && o.Skw == o7.Skw && o.pad == 0);
          CHECK(std::memcmp(o.row, o7.row, 6 * sizeof(double)) == 0 && o.row[14] == o7.row[6]);
          bool any = false;
          for (int e = 0; e < 8; e++) {
            CHECK(std::isfinite(o.row[6 + e]));
            if (!(mask >> e & 1u)) CHECK(o.row[6 + e] == 0.0);
            any = any || o.row[6 + e] != 0.0;
          }
          CHECK(any == (fr != 0 && o.code == 0));
          if (fr && o.code == 0 && mask == 0xFFu) {  // the columns of cx and cy are nh^T G^-1: never both zero
            CHECK(o.row[8] != 0.0 || o.row[9] != 0.0);
          }
        }
        codes_seen[o7.code]++;
      }
    }
  for (int c : {0, 1, 3, 4, 5}) CHECK(codes_seen[c] > 0);
  if (g_verbose)
    std::printf("windows: codes 0..5 seen %d %d %d %d %d %d\n", codes_seen[0], codes_seen[1], codes_seen[2],
                codes_seen[3], codes_seen[4], codes_seen[5]);
  CHECK(xi::tri(0, 0) == 0 && xi::tri(0, 14) == 14 && xi::tri(1, 1) == 15 && xi::tri(14, 14) == 119);
  int n = 0;
  for (int a = 0; a < 15; a++)
    for (int b = a; b < 15; b++) CHECK(xi::tri(a, b) == n++);
  // on the axis: G = I, c = 1, the k columns zero
  const mk::Cam cam{60.0, 61.0, 20.0, 16.0, {0.003, -0.01, 0.005, -0.002}};
  const double m0[2] = {0.0, 0.0}, nh[2] = {0.6, -0.8};
  double Ji[8];
  ic::jint(cam, m0, nh, true, 0xFFu, Ji);
  CHECK(Ji[0] == 0.0 && Ji[1] == 0.0 && Ji[2] == 0.6 && Ji[3] == -0.8 && Ji[4] == 0.0 && Ji[7] == 0.0);
  // the restated atan against the library's
  for (int k = 0; k < 2000; k++) {
    const double x = std::exp(40.0 * (unif() - 0.5));
    CHECK(std::fabs(ic::atan_rho(x, 1.0 / x) - std::atan(x)) <= 4e-16 * std::atan(x));
  }
}

static void random_acc(int N, int C, uint32_t fm, uint32_t pm, int zero_pose_col, int zero_int_col, double r_scale,
                       std::vector<double>& acc, std::vector<int32_t>& cnt) {
  acc.assign((size_t)N * C * xi::kAcc, 0.0);
  cnt.assign((size_t)N * C, 60);
  for (int r = 0; r < N; r++)
    for (int c = 0; c < C; c++)
      for (int k = 0; k < 60; k++) {
        double row[15];
        for (int e = 0; e < 15; e++) row[e] = unif() - 0.5;
        row[14] *= r_scale;
        for (int e = 0; e < 8; e++)
          if (!(fm >> c & 1) || !(pm >> e & 1)) row[6 + e] = 0.0;
        if (zero_pose_col >= 0 && r == N - 1) row[zero_pose_col] = 0.0;
        if (zero_int_col >= 0) row[6 + zero_int_col] = 0.0;
        xi::accumulate_row(row, acc.data() + (size_t)xi::kAcc * (r * C + c));
      }
}

// the end of a pass on given accumulators: both starved gates, both singular exits, the diverged exit, the
// final pass, a step against the residual of the full normal equations, the gate and the covariance
static void check_passes() {
  const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const double K0[4] = {300.0, 301.0, 320.0, 240.0}, D0[4] = {0.003, -0.01, 0.005, -0.002};
  for (int shape = 0; shape < 4; shape++) {
    const int N = shape == 0 ? 1 : 3, C = shape == 0 ? 1 : shape == 1 ? 2 : 8;
    const uint32_t fm = shape == 1 ? 0x2u : (1u << C) - 1u;
    const uint32_t pm = shape == 3 ? 0x3Fu : 0xFFu;
    int fcam[8], np = 0;
    const int F = cal::free_list(fm, C, fcam), nS = 8 * F;
    lc::Layout lay;
    xi::layout(0u, fm, C, lay);
    for (int e = 0; e < 8; e++) np += (int)(pm >> e & 1u);
    std::vector<double> acc, T0((size_t)16 * N), T;
    std::vector<int32_t> cnt;
    for (int r = 0; r < N; r++) std::memcpy(T0.data() + 16 * r, I4, sizeof(I4));
    auto fresh = [&](mantis_icalib_result& R) {
      R = mantis_icalib_result{};
      for (int c = 0; c < C; c++) {
        std::memcpy(R.K[c], K0, sizeof(K0));
        std::memcpy(R.D[c], D0, sizeof(D0));
      }
      T = T0;
    };
    auto same_kd = [&](const mantis_icalib_result& R) {
      for (int c = 0; c < C; c++)
        if (std::memcmp(R.K[c], K0, sizeof(K0)) || std::memcmp(R.D[c], D0, sizeof(D0))) return false;
      return true;
    };
    mantis_icalib_result R;
    std::vector<double> delta((size_t)6 * N);
    // a step: the full normal equations hold at (delta, eps)
    random_acc(N, C, fm, pm, -1, -1, 0.01, acc, cnt);
    fresh(R);
    CHECK(!end_pass(acc.data(), cnt.data(), N, C, fm, pm, 0, 4, 12, 12, 0.0, T.data(), R, delta.data()));
    CHECK(R.status == lc::kOk && R.iterations_run == 1 && R.n_obs[0] == 60 * N * C && R.n_obs_cam[0][C - 1] == 60 * N);
    double worst = 0;
    for (int r = 0; r < N; r++)
      for (int i = 0; i < 6; i++) {  // A_r delta_r + E_r eps = -a_r
        const double* av = acc.data() + (size_t)xi::kAcc * C * r;
        double s = 0;
        for (int j = 0; j < 6; j++) s += xi::view_A(av, C, i, j, 0.0) * delta[6 * r + j];
        for (int j = 0; j < nS; j++) s += xi::view_rhs(av, C, lay, i, j) * R.delta_cam[0][fcam[j / 8]][j % 8];
        s += xi::view_rhs(av, C, lay, i, nS);
        worst = std::fmax(worst, std::fabs(s));
      }
    for (int f = 0; f < F; f++)
      for (int i = 0; i < 8; i++) {  // sum_r E_rf^T delta_r + B_f eps_f = -b_f, for the free parameters
        if (!(pm >> i & 1u)) {
          CHECK(R.delta_cam[0][fcam[f]][i] == 0.0);
          continue;
        }
        double s = 0;
        for (int r = 0; r < N; r++) {
          const double* a = acc.data() + (size_t)xi::kAcc * (r * C + fcam[f]);
          for (int k = 0; k < 6; k++) s += a[xi::tri(k, 6 + i)] * delta[6 * r + k];
          for (int j = 0; j < 8; j++) s += a[xi::tri_sym(6 + i, 6 + j)] * R.delta_cam[0][fcam[f]][j];
          s += a[xi::tri(6 + i, 14)];
        }
        worst = std::fmax(worst, std::fabs(s));
      }
    if (g_verbose) std::printf("passes N=%d C=%d F=%d mask=%#x: normal-equation residual %.3g\n", N, C, F, pm, worst);
    CHECK(worst < 1e-9);
    for (int c = 0; c < C; c++) {
      const bool fr = (fm >> c & 1u) != 0;
      const double* e = R.delta_cam[0][c];
      CHECK(R.K[c][0] == (fr && (pm & 1u) ? K0[0] * (1.0 + e[0]) : K0[0]));
      CHECK(R.K[c][2] == (fr && (pm & 4u) ? K0[2] + K0[0] * e[2] : K0[2]));
      CHECK(R.K[c][3] == (fr && (pm & 8u) ? K0[3] + K0[1] * e[3] : K0[3]));
      CHECK(R.D[c][3] == (fr && (pm & 128u) ? D0[3] + e[7] : D0[3]));
      CHECK(R.D[c][2] == (fr && (pm & 64u) ? D0[2] + e[6] : D0[2]));
    }
    // the gate and the covariance on the same accumulators: positive diagonals for the free parameters,
    // symmetric, zeros for held cameras and held parameters
    fresh(R);
    (void)end_pass(acc.data(), cnt.data(), N, C, fm, pm, 0, 0, 12, 12, 0.0, T.data(), R, nullptr);  // the figures
    conclude(acc.data(), cnt.data(), N, C, fm, pm, 12, 12, 0.0, R);
    CHECK(R.calibrated == 1);
    for (int c = 0; c < 8; c++)
      for (int i = 0; i < 8; i++) {
        const bool fr = c < C && (fm >> c & 1) && (pm >> i & 1);
        CHECK(fr ? R.covariance[c][9 * i] > 0 : R.covariance[c][9 * i] == 0.0);
        for (int j = 0; j < 8; j++) {
          CHECK(R.covariance[c][8 * i + j] == R.covariance[c][8 * j + i]);
          if (!fr) CHECK(R.covariance[c][8 * i + j] == 0.0);
        }
      }
    conclude(acc.data(), cnt.data(), N, C, fm, pm, 12, 12, 1e-12, R);  // a gate no rms passes
    CHECK(R.calibrated == 0 && R.covariance[C - 1][0] == 0.0);
    // the final pass solves nothing, whatever the system
    fresh(R);
    CHECK(end_pass(acc.data(), cnt.data(), N, C, fm, pm, 4, 4, 12, 12, 0.0, T.data(), R, nullptr));
    CHECK(R.status == lc::kOk && R.n_obs[4] == 60 * N * C && T == T0 && same_kd(R));
    // starved: a view below min_obs, then a free camera below min_obs_cam
    fresh(R);
    CHECK(end_pass(acc.data(), cnt.data(), N, C, fm, pm, 0, 4, 60 * C + 1, 12, 0.0, T.data(), R, nullptr));
    CHECK(R.status == lc::kStarved && R.iterations_run == 0 && T == T0 && same_kd(R));
    fresh(R);
    CHECK(end_pass(acc.data(), cnt.data(), N, C, fm, pm, 0, 4, 12, 60 * N + 1, 0.0, T.data(), R, nullptr));
    CHECK(R.status == lc::kStarved && R.iterations_run == 0 && same_kd(R));
    conclude(acc.data(), cnt.data(), N, C, fm, pm, 12, 60 * N + 1, 0.0, R);
    CHECK(R.calibrated == 0);
    // singular A_r: the last view sees nothing of one pose direction
    random_acc(N, C, fm, pm, 2, -1, 0.01, acc, cnt);
    fresh(R);
    CHECK(end_pass(acc.data(), cnt.data(), N, C, fm, pm, 0, 4, 12, 12, 0.0, T.data(), R, nullptr));
    CHECK(R.status == lc::kSingular && R.iterations_run == 0 && T == T0 && same_kd(R));
    CHECK(!end_pass(acc.data(), cnt.data(), N, C, fm, pm, 0, 4, 12, 12, 1e-3, T.data(), (fresh(R), R), nullptr));  // damped
    // singular S: A_r fine, one free intrinsic unseen by every row
    random_acc(N, C, fm, pm, -1, 3, 0.01, acc, cnt);
    fresh(R);
    CHECK(end_pass(acc.data(), cnt.data(), N, C, fm, pm, 0, 4, 12, 12, 0.0, T.data(), R, nullptr));
    CHECK(R.status == lc::kSingular && R.iterations_run == 0 && T == T0 && same_kd(R));
    R.status = lc::kOk;
    conclude(acc.data(), cnt.data(), N, C, fm, pm, 12, 12, 0.0, R);
    CHECK(R.calibrated == 0 && R.covariance[C - 1][0] == 0.0);
    // ... and the same accumulators with that parameter held: its diagonal is 1, the step is taken
    fresh(R);
    CHECK(!end_pass(acc.data(), cnt.data(), N, C, fm, pm & ~8u, 0, 4, 12, 12, 0.0, T.data(), R, nullptr));
    CHECK(R.status == lc::kOk && R.K[C - 1][3] == K0[3]);
    // diverged: residuals a thousand times the Jacobian's entries push some fx (1 + eps) or fy below zero
    random_acc(N, C, fm, pm, -1, -1, 1e3, acc, cnt);
    fresh(R);
    CHECK(end_pass(acc.data(), cnt.data(), N, C, fm, pm, 0, 4, 12, 12, 0.0, T.data(), R, delta.data()));
    CHECK(R.status == lc::kDiverged && R.iterations_run == 0 && T == T0 && same_kd(R));
    for (int c = 0; c < 8; c++)
      for (int e = 0; e < 8; e++) CHECK(R.delta_cam[0][c][e] == 0.0);
    conclude(acc.data(), cnt.data(), N, C, fm, pm, 12, 12, 0.0, R);
    CHECK(R.calibrated == 0);
  }
  // param_update on its own: the order of the scaling, the held bits, the three ways to diverge
  const double th[8] = {300, 200, 10, 20, 1, 2, 3, 4}, e1[8] = {0.5, -0.5, 0.1, 0.1, 1, 1, 1, 1};
  double out[8];
  CHECK(ic::param_update(th, e1, 0xFFu, out) && out[0] == 450 && out[1] == 100 && out[2] == 40 && out[3] == 40 && out[7] == 5);
  CHECK(ic::param_update(th, e1, 0xA5u, out) && out[0] == 450 && out[1] == 200 && out[2] == 40 && out[3] == 20 &&
        out[4] == 1 && out[5] == 3 && out[6] == 3 && out[7] == 5);
  const double e2[8] = {-1.0, 0, 0, 0, 0, 0, 0, 0}, e3[8] = {0, 0, 0, 0, 0, INFINITY, 0, 0}, e4[8] = {0, NAN, 0, 0, 0, 0, 0, 0};
  CHECK(!ic::param_update(th, e2, 0xFFu, out) && !ic::param_update(th, e3, 0xFFu, out) && !ic::param_update(th, e4, 0xFFu, out));
  CHECK(ic::param_update(th, e3, 0xDFu, out) && out[5] == 2);
  // no row at all: rms is 0, not 0 / 0
  std::vector<double> acc((size_t)2 * xi::kAcc, 0.0), T(I4, I4 + 16);
  std::vector<int32_t> cnt(2, 0);
  mantis_icalib_result R{};
  CHECK(end_pass(acc.data(), cnt.data(), 1, 2, 3u, 0xFFu, 0, 4, 12, 12, 0.0, T.data(), R, nullptr));
  CHECK(R.status == lc::kStarved && R.rms[0] == 0.0 && R.n_obs[0] == 0);
  conclude(acc.data(), cnt.data(), 1, 2, 3u, 0xFFu, 12, 12, 0.0, R);
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

// the whole call on painted grids: N views of a rig of C nadir cameras, every camera rendered through
// intrinsics beside the nominal ones, all cameras free
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
  for (int shape = 0; shape < 4; shape++) {
    const int N = shape == 0 ? 1 : 3, C = shape == 1 ? 1 : shape >= 2 ? 8 : 2;
    const uint32_t fm = (1u << C) - 1u, pm = shape <= 1 ? 0x0Fu : 0x3Fu;  // two cameras or one: K only; eight: K, k1, k2
    const int Rw = shape == 3 ? 15 : 6;
    std::vector<double> E((size_t)16 * C), T_true((size_t)16 * N), T0((size_t)16 * N), T_out((size_t)16 * N);
    std::vector<mk::Cam> truth(C, nominal), cams(C, nominal);
    for (int c = 0; c < C; c++) {
      // tilted: a camera that looks straight down at a plane cannot tell its focal length from its height
      ext_pose(0.012 * c - 0.03, 0.01 * (c % 3) - 0.01, 0.0, 0.7 * c, E.data() + 16 * c, 0.45);
      truth[c].fx *= 1.0 + (c % 2 ? 0.008 : -0.008);
      truth[c].fy *= 1.0 + (c % 3 ? -0.008 : 0.008);
      truth[c].cx += c % 2 ? 1.0 : -1.0;
      truth[c].cy += c % 4 < 2 ? 1.0 : -1.0;
    }
    std::vector<std::vector<uint8_t>> imgs((size_t)N * C, std::vector<uint8_t>((size_t)W * H * 3, 0));
    std::vector<const uint8_t*> frames((size_t)N * C);
    for (int r = 0; r < N; r++) {
      nadir_pose(0.03 - 0.02 * r, -0.02 + 0.015 * r, 0.6 + 0.02 * r, 0.3 + 0.4 * r, T_true.data() + 16 * r);
      nadir_pose(0.03 - 0.02 * r + 0.003, -0.02 + 0.015 * r - 0.003, 0.6 + 0.02 * r, 0.3 + 0.4 * r + 0.003, T0.data() + 16 * r);
      for (int c = 0; c < C; c++) {
        double Twc[16];
        mul4(T_true.data() + 16 * r, E.data() + 16 * c, Twc);
        paint_grid(imgs[r * C + c], W, H, Twc, truth[c], 2 * pitch, 2, 4 * pitch);
        frames[r * C + c] = imgs[r * C + c].data();
      }
    }
    mantis_refine_params p{};
    p.struct_size = sizeof(p);
    p.iterations = 5;
    p.half_window = Rw;
    p.white_thresh = 3 * 64 * 64;
    p.min_weight = 12288;
    p.min_obs = 12;
    p.lambda = 1e-6;
    p.landmark_pitch = pitch * 0.5;
    mantis_icalib_params ip{(int32_t)sizeof(mantis_icalib_params), (int32_t)fm, (int32_t)pm, 12};
    mantis_icalib_result res;
    std::vector<xi::Slot> slots((size_t)N * C * nc);
    icalib_seq(T0.data(), E.data(), cams.data(), frames.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p, ip,
                   T_out.data(), res, slots.data());
    double g0 = 0, g1 = 0;
    for (int c = 0; c < C; c++) {
      g0 = std::fmax(g0, model_gap(cams[c], truth[c]));
      g1 = std::fmax(g1, model_gap(ic::cam_of(res.K[c], res.D[c]), truth[c]));
    }
    if (g_verbose)
      std::printf("seq N=%d C=%d R=%d mask=%#x: status %d calibrated %d runs %d n_obs %d..%d  worst gap %.3f -> %.3f px  rms %.3g -> %.3g\n",
                  N, C, Rw, pm, res.status, res.calibrated, res.iterations_run, res.n_obs[0],
                  res.n_obs[res.iterations_run], g0, g1, res.rms[0], res.rms[res.iterations_run]);
    CHECK(res.status == lc::kOk && res.iterations_run == 5 && res.n_cand == nc && res.n_rigs == N && res.n_cams == C);
    CHECK(res.free_cams == (int32_t)fm && res.param_mask == (int32_t)pm);
    CHECK(res.calibrated == 1 && g1 < g0 && res.rms[5] < res.rms[0]);
    for (int c = 0; c < C; c++)
      for (int e = 0; e < 4; e++)
        if (!(pm >> (4 + e) & 1u)) CHECK(res.D[c][e] == nominal.k[e]);
    for (int c = C; c < 8; c++)
      for (int e = 0; e < 4; e++) CHECK(res.K[c][e] == 0.0 && res.D[c][e] == 0.0);
    for (size_t k = 0; k < slots.size(); k++)
      if (slots[k].code)
        for (int e = 0; e < 15; e++) CHECK(slots[k].row[e] == 0.0);
    // I = 0: every pose and intrinsic comes back bit for bit
    p.iterations = 0;
    icalib_seq(T0.data(), E.data(), cams.data(), frames.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p, ip,
                   T_out.data(), res, nullptr);
    CHECK(std::memcmp(T_out.data(), T0.data(), sizeof(double) * 16 * N) == 0 && res.iterations_run == 0);
    for (int c = 0; c < C; c++) {
      double th[8];
      ic::cam_to(nominal, th);
      CHECK(std::memcmp(res.K[c], th, 4 * sizeof(double)) == 0 && std::memcmp(res.D[c], th + 4, 4 * sizeof(double)) == 0);
    }
    // R = 1: three samples; whatever the rule says, finite
    p.iterations = 3;
    p.half_window = 1;
    icalib_seq(T_true.data(), E.data(), truth.data(), frames.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p,
                   ip, T_out.data(), res, nullptr);
    for (size_t e = 0; e < T_out.size(); e++) CHECK(std::isfinite(T_out[e]));
    for (int c = 0; c < C; c++)
      for (int e = 0; e < 4; e++) CHECK(std::isfinite(res.K[c][e]) && std::isfinite(res.D[c][e]));
    // starved: the last view black (a view's gate), then the last camera black in every view (a camera's)
    p.half_window = 6;
    std::vector<uint8_t> black((size_t)W * H * 3, 0);
    std::vector<const uint8_t*> fb = frames;
    for (int c = 0; c < C; c++) fb[(N - 1) * C + c] = black.data();
    icalib_seq(T0.data(), E.data(), cams.data(), fb.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p, ip,
                   T_out.data(), res, nullptr);
    CHECK(res.status == lc::kStarved && res.calibrated == 0 && std::memcmp(T_out.data(), T0.data(), sizeof(double) * 16 * N) == 0);
    if (C > 1) {
      fb = frames;
      for (int r = 0; r < N; r++) fb[r * C + C - 1] = black.data();
      icalib_seq(T0.data(), E.data(), cams.data(), fb.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p, ip,
                     T_out.data(), res, nullptr);
      CHECK(res.status == lc::kStarved && res.n_obs_cam[0][C - 1] == 0 && res.n_obs[0] > 12 * N);
      CHECK(res.K[C - 1][0] == nominal.fx);
    }
    // no candidates at all
    icalib_seq(T0.data(), E.data(), cams.data(), frames.data(), N, C, W, H, X.data(), n, 0, cand.data(), 0, p, ip,
                   T_out.data(), res, nullptr);
    CHECK(res.status == lc::kStarved && res.rms[0] == 0.0);
  }
}

int main(int argc, char** argv) {
  g_verbose = argc > 1 && std::strcmp(argv[1], "-v") == 0;
  check_windows();
  check_passes();
  check_seq();
  if (g_fail) {
    std::printf("icalibcheck: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("icalibcheck ok\n");
  return 0;
}
