// Stand-alone check of the extrinsic calibration's rules (mantis_amd/csrc/
// mk_linecal.h at the problem Ext, mk_calib.h: one observation with its window over the frame edges and the
// extrinsic's columns, the end of a pass with its starved and both singular
// exits, the gate and the covariance, the whole call for N = 1 and 3 views,
// C = 2 and 8 cameras with seven free, R = 1 and 15) on small synthetic frames
// that are allocated at exactly their size, as a program of its own so that it
// can be built with sanitizers and run directly:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o build/calibcheck tools/calibcheck_main.cpp && build/calibcheck
// Exit status 0 and "calibcheck ok" when every case holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../mantis_amd/csrc/mk_linecal.h"

namespace rf = mk::refine;
namespace cal = mk::calib;
namespace lc = mk::linecal;
using xc = lc::Ext;  // the shared rules at the extrinsic calibration's problem

// the shared rules on the extrinsic calibration's public struct
static bool end_pass(const double* acc, const int32_t* cnt, int N, int C, uint32_t fm, int pass, int I, int32_t min_obs,
                     int32_t min_obs_cam, double lambda, double* T, mantis_calib_result& R, double* delta) {
  return lc::with_state(R, [&](mantis_rcalib_result& w) {
    return xc::end_pass(acc, cnt, N, C, fm, 0u, 0u, pass, I, min_obs, min_obs_cam, lambda, T, w, delta);
  });
}
static void conclude(const double* acc, const int32_t* cnt, int N, int C, uint32_t fm, int32_t min_obs,
                     int32_t min_obs_cam, double max_rms, mantis_calib_result& R) {
  lc::with_state(R, [&](mantis_rcalib_result& w) {
    xc::conclude(acc, cnt, N, C, fm, 0u, 0u, min_obs, min_obs_cam, max_rms, w);
  });
}
static void calib_seq(const double* T_in, const double* Tbc, const mk::Cam* cams, const uint8_t* const* frames, int N,
                      int C, int W, int H, const double* X, int nw, int nr, const int32_t* cand, int n_cand,
                      const mantis_refine_params& p, const mantis_calib_params& cp, double* T_out, mantis_calib_result& R,
                      xc::Slot* slots) {
  mantis_rcalib_result w;
  xc::seq(T_in, Tbc, cams, frames, N, C, W, H, X, nw, nr, cand, n_cand, p, (uint32_t)cp.free_cams, 0u, 0u, cp.min_obs_cam,
          T_out, w, slots);
  lc::narrow(w, R);
}

static int g_fail = 0;
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
// an extrinsic: yaw a about the base's z, then the offset (x, y, z)
static void ext_pose(double x, double y, double z, double a, double* E) {
  const double c = std::cos(a), s = std::sin(a);
  const double M[16] = {c, -s, 0, x, s, c, 0, y, 0, 0, 1, z, 0, 0, 0, 1};
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
static double ext_dist(const double* A, const double* B) {
  return std::sqrt((A[3] - B[3]) * (A[3] - B[3]) + (A[7] - B[7]) * (A[7] - B[7]) + (A[11] - B[11]) * (A[11] - B[11]));
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
// calibration's slot is the refinement's with the extrinsic's columns between J and r
static void check_windows() {
  const int tg[3] = {255, 255, 255};
  int codes_seen[6] = {0};
  for (int R : {1, 15, 12})
    for (int size = 0; size < 3; size++) {
      const int W = size == 0 ? 40 : size == 1 ? 97 : 33, H = size == 0 ? 32 : size == 1 ? 61 : 33;
      const mk::Cam cam{60.0, 60.0, W / 2.0 - 0.25, H / 2.0 + 0.125, {0.003, -0.01, 0.005, -0.002}};
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
        for (int fr = 0; fr < 2; fr++) {
          xc::Slot o;
          int tie;
          xc::observe(Rt, t, gc, cam, img.data(), W, H, X, trial & 1, tg, win, fr != 0, false, 0u, o, &tie);
          CHECK(o.code == o7.code && o.Sw == o7.Sw && o.Skw == o7.Skw && o.pad == 0);
          CHECK(std::memcmp(o.row, o7.row, 6 * sizeof(double)) == 0 && o.row[12] == o7.row[6]);
          bool any = false;
          for (int e = 6; e < 12; e++) {
            CHECK(std::isfinite(o.row[e]));
            any = any || o.row[e] != 0.0;
          }
          CHECK(any == (fr != 0 && o.code == 0));
          if (fr && o.code == 0) {  // J_pose = J_ext Ad: the translation parts are one rotation apart, of equal length
            const double a = o.row[0] * o.row[0] + o.row[1] * o.row[1] + o.row[2] * o.row[2];
            const double b = o.row[6] * o.row[6] + o.row[7] * o.row[7] + o.row[8] * o.row[8];
            CHECK(std::fabs(a - b) <= 1e-12 * a);
          }
        }
        codes_seen[o7.code]++;
      }
    }
  for (int c : {0, 1, 3, 4, 5}) CHECK(codes_seen[c] > 0);
  std::printf("windows: codes 0..5 seen %d %d %d %d %d %d\n", codes_seen[0], codes_seen[1], codes_seen[2], codes_seen[3],
              codes_seen[4], codes_seen[5]);
  CHECK(xc::tri(0, 0) == 0 && xc::tri(0, 12) == 12 && xc::tri(1, 1) == 13 && xc::tri(12, 12) == 90);
  int n = 0;
  for (int a = 0; a < 13; a++)
    for (int b = a; b < 13; b++) CHECK(xc::tri(a, b) == n++);
}

static void random_acc(int N, int C, uint32_t fm, int zero_pose_col, int zero_ext_col, std::vector<double>& acc,
                       std::vector<int32_t>& cnt) {
  acc.assign((size_t)N * C * xc::kAcc, 0.0);
  cnt.assign((size_t)N * C, 40);
  for (int r = 0; r < N; r++)
    for (int c = 0; c < C; c++)
      for (int k = 0; k < 40; k++) {
        double row[13];
        for (int e = 0; e < 13; e++) row[e] = unif() - 0.5;
        if (!(fm >> c & 1))
          for (int e = 6; e < 12; e++) row[e] = 0.0;
        if (zero_pose_col >= 0 && r == N - 1) row[zero_pose_col] = 0.0;
        if (zero_ext_col >= 0) row[6 + zero_ext_col] = 0.0;
        xc::accumulate_row(row, acc.data() + (size_t)xc::kAcc * (r * C + c));
      }
}

// the end of a pass on given accumulators: both starved gates, both singular exits, the final pass, a step
// against the residual of the full normal equations, the gate and the covariance
static void check_passes() {
  const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  for (int shape = 0; shape < 3; shape++) {
    const int N = shape == 0 ? 1 : 3, C = shape == 2 ? 8 : 2;
    const uint32_t fm = shape == 2 ? 0xfeu : 0x2u;
    int fcam[8];
    const int F = cal::free_list(fm, C, fcam);
    lc::Layout lay;
    xc::layout(fm, 0u, C, lay);
    std::vector<double> acc, T0((size_t)16 * N), T;
    std::vector<int32_t> cnt;
    for (int r = 0; r < N; r++) std::memcpy(T0.data() + 16 * r, I4, sizeof(I4));
    auto fresh = [&](mantis_calib_result& R) {
      R = mantis_calib_result{};
      for (int c = 0; c < C; c++) std::memcpy(R.T_base_cam[c], I4, sizeof(I4));
      T = T0;
    };
    mantis_calib_result R;
    std::vector<double> delta((size_t)6 * N);
    // a step: the full normal equations hold at (delta, eps)
    random_acc(N, C, fm, -1, -1, acc, cnt);
    fresh(R);
    CHECK(!end_pass(acc.data(), cnt.data(), N, C, fm, 0, 4, 12, 12, 0.0, T.data(), R, delta.data()));
    CHECK(R.status == lc::kOk && R.iterations_run == 1 && R.n_obs[0] == 40 * N * C && R.n_obs_cam[0][C - 1] == 40 * N);
    double worst = 0;
    for (int r = 0; r < N; r++)
      for (int i = 0; i < 6; i++) {  // A_r delta_r + E_r eps = -a_r
        double s = 0;
        for (int j = 0; j < 6; j++) s += xc::view_A(acc.data() + (size_t)xc::kAcc * C * r, C, i, j, 0.0) * delta[6 * r + j];
        for (int j = 0; j < 6 * F; j++)
          s += xc::view_rhs(acc.data() + (size_t)xc::kAcc * C * r, C, lay, i, j) * R.delta_cam[0][fcam[j / 6]][j % 6];
        s += xc::view_rhs(acc.data() + (size_t)xc::kAcc * C * r, C, lay, i, 6 * F);
        worst = std::fmax(worst, std::fabs(s));
      }
    for (int f = 0; f < F; f++)
      for (int i = 0; i < 6; i++) {  // sum_r E_rf^T delta_r + B_f eps_f = -b_f
        double s = 0;
        for (int r = 0; r < N; r++) {
          const double* a = acc.data() + (size_t)xc::kAcc * (r * C + fcam[f]);
          for (int k = 0; k < 6; k++) s += a[xc::tri(k, 6 + i)] * delta[6 * r + k];
          for (int j = 0; j < 6; j++) s += a[i <= j ? xc::tri(6 + i, 6 + j) : xc::tri(6 + j, 6 + i)] * R.delta_cam[0][fcam[f]][j];
          s += a[xc::tri(6 + i, 12)];
        }
        worst = std::fmax(worst, std::fabs(s));
      }
    std::printf("passes N=%d C=%d F=%d: normal-equation residual %.3g\n", N, C, F, worst);
    CHECK(worst < 1e-9);
    for (int c = 0; c < C; c++)
      if (!(fm >> c & 1)) CHECK(std::memcmp(R.T_base_cam[c], I4, sizeof(I4)) == 0);
    // the gate and the covariance on the same accumulators: positive diagonals, symmetric, zeros for held cameras
    R.iterations_run = 0;
    conclude(acc.data(), cnt.data(), N, C, fm, 12, 12, 0.0, R);
    CHECK(R.calibrated == 1);
    for (int c = 0; c < 8; c++)
      for (int i = 0; i < 6; i++) {
        const bool fr = c < C && (fm >> c & 1);
        CHECK(fr ? R.covariance[c][7 * i] > 0 : R.covariance[c][7 * i] == 0.0);
        for (int j = 0; j < 6; j++) CHECK(R.covariance[c][6 * i + j] == R.covariance[c][6 * j + i]);
      }
    conclude(acc.data(), cnt.data(), N, C, fm, 12, 12, 1e-12, R);  // a gate no rms passes
    CHECK(R.calibrated == 0 && R.covariance[1][0] == 0.0);
    // the final pass solves nothing, whatever the system
    fresh(R);
    CHECK(end_pass(acc.data(), cnt.data(), N, C, fm, 4, 4, 12, 12, 0.0, T.data(), R, nullptr));
    CHECK(R.status == lc::kOk && R.n_obs[4] == 40 * N * C && T == T0);
    // starved: a view below min_obs, then a free camera below min_obs_cam
    fresh(R);
    CHECK(end_pass(acc.data(), cnt.data(), N, C, fm, 0, 4, 40 * C + 1, 12, 0.0, T.data(), R, nullptr));
    CHECK(R.status == lc::kStarved && R.iterations_run == 0 && T == T0);
    fresh(R);
    CHECK(end_pass(acc.data(), cnt.data(), N, C, fm, 0, 4, 12, 40 * N + 1, 0.0, T.data(), R, nullptr));
    CHECK(R.status == lc::kStarved && R.iterations_run == 0 && std::memcmp(R.T_base_cam[1], I4, sizeof(I4)) == 0);
    conclude(acc.data(), cnt.data(), N, C, fm, 12, 40 * N + 1, 0.0, R);
    CHECK(R.calibrated == 0);
    // singular A_r: the last view sees nothing of one pose direction
    random_acc(N, C, fm, 2, -1, acc, cnt);
    fresh(R);
    CHECK(end_pass(acc.data(), cnt.data(), N, C, fm, 0, 4, 12, 12, 0.0, T.data(), R, nullptr));
    CHECK(R.status == lc::kSingular && R.iterations_run == 0 && T == T0);
    CHECK(!end_pass(acc.data(), cnt.data(), N, C, fm, 0, 4, 12, 12, 1e-3, T.data(), (fresh(R), R), nullptr));  // damped
    // singular S: A_r fine, one extrinsic direction unseen by every row
    random_acc(N, C, fm, -1, 3, acc, cnt);
    fresh(R);
    CHECK(end_pass(acc.data(), cnt.data(), N, C, fm, 0, 4, 12, 12, 0.0, T.data(), R, nullptr));
    CHECK(R.status == lc::kSingular && R.iterations_run == 0 && T == T0);
    for (int c = 0; c < C; c++) CHECK(std::memcmp(R.T_base_cam[c], I4, sizeof(I4)) == 0);
    R.status = lc::kOk;
    conclude(acc.data(), cnt.data(), N, C, fm, 12, 12, 0.0, R);
    CHECK(R.calibrated == 0 && R.covariance[1][0] == 0.0);
  }
  // no row at all: rms is 0, not 0 / 0
  std::vector<double> acc((size_t)2 * xc::kAcc, 0.0), T(I4, I4 + 16);
  std::vector<int32_t> cnt(2, 0);
  mantis_calib_result R{};
  CHECK(end_pass(acc.data(), cnt.data(), 1, 2, 2u, 0, 4, 12, 12, 0.0, T.data(), R, nullptr));
  CHECK(R.status == lc::kStarved && R.rms[0] == 0.0 && R.n_obs[0] == 0);
  conclude(acc.data(), cnt.data(), 1, 2, 2u, 12, 12, 0.0, R);
  CHECK(R.calibrated == 0 && R.rms_cam[1] == 0.0);
}

// the whole call on painted grids: N views of a rig of C nadir cameras, one of the free cameras displaced
static void check_seq() {
  const int W = 320, H = 240;
  const mk::Cam cam{150.0, 150.0, 159.5, 119.5, {0.003, -0.01, 0.005, -0.002}};
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
    const int N = shape == 0 ? 1 : 3, C = shape >= 2 ? 8 : 2;
    const uint32_t fm = C == 8 ? 0xfeu : 0x2u;
    const int Rw = shape == 3 ? 15 : 6;
    std::vector<double> E_true((size_t)16 * C), E_nom, T_true((size_t)16 * N), T0((size_t)16 * N), T_out((size_t)16 * N);
    for (int c = 0; c < C; c++) ext_pose(0.012 * c - 0.03, 0.01 * (c % 3) - 0.01, 0.0, 0.05 * c, E_true.data() + 16 * c);
    E_nom = E_true;
    const int moved = C - 1;  // its nominal extrinsic is 3 mm and 0.004 rad beside the truth
    ext_pose(0.012 * moved - 0.03 + 0.003, 0.01 * (moved % 3) - 0.01 - 0.002, 0.0, 0.05 * moved + 0.004,
             E_nom.data() + 16 * moved);
    std::vector<std::vector<uint8_t>> imgs((size_t)N * C, std::vector<uint8_t>((size_t)W * H * 3, 0));
    std::vector<const uint8_t*> frames((size_t)N * C);
    for (int r = 0; r < N; r++) {
      nadir_pose(0.03 - 0.02 * r, -0.02 + 0.015 * r, 0.6 + 0.02 * r, 0.3 + 0.4 * r, T_true.data() + 16 * r);
      nadir_pose(0.03 - 0.02 * r + 0.003, -0.02 + 0.015 * r - 0.003, 0.6 + 0.02 * r, 0.3 + 0.4 * r + 0.003, T0.data() + 16 * r);
      for (int c = 0; c < C; c++) {
        double Twc[16];
        mul4(T_true.data() + 16 * r, E_true.data() + 16 * c, Twc);
        paint_grid(imgs[r * C + c], W, H, Twc, cam, 2 * pitch, 2, 4 * pitch);
        frames[r * C + c] = imgs[r * C + c].data();
      }
    }
    std::vector<mk::Cam> cams(C, cam);
    mantis_refine_params p{};
    p.struct_size = sizeof(p);
    p.iterations = 5;
    p.half_window = Rw;
    p.white_thresh = 3 * 64 * 64;
    p.min_weight = 12288;
    p.min_obs = 12;
    p.landmark_pitch = pitch * 0.5;
    mantis_calib_params cp{(int32_t)sizeof(mantis_calib_params), (int32_t)fm, 12, 0};
    mantis_calib_result res;
    std::vector<xc::Slot> slots((size_t)N * C * nc);
    calib_seq(T0.data(), E_nom.data(), cams.data(), frames.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p, cp,
                   T_out.data(), res, slots.data());
    const double e0 = ext_dist(E_nom.data() + 16 * moved, E_true.data() + 16 * moved);
    const double e1 = ext_dist(res.T_base_cam[moved], E_true.data() + 16 * moved);
    std::printf("seq N=%d C=%d R=%d: status %d calibrated %d runs %d n_obs %d..%d  camera %d: %.5f -> %.5f m  rms %.3g -> %.3g\n",
                N, C, Rw, res.status, res.calibrated, res.iterations_run, res.n_obs[0], res.n_obs[res.iterations_run],
                moved, e0, e1, res.rms[0], res.rms[res.iterations_run]);
    CHECK(res.status == lc::kOk && res.iterations_run == 5 && res.n_cand == nc && res.n_rigs == N && res.n_cams == C);
    CHECK(res.calibrated == 1 && e1 < e0 && res.rms[5] < res.rms[0]);
    CHECK(std::memcmp(res.T_base_cam[0], E_nom.data(), 16 * sizeof(double)) == 0);
    for (int c = C; c < 8; c++)
      for (int e = 0; e < 16; e++) CHECK(res.T_base_cam[c][e] == 0.0);
    for (size_t k = 0; k < slots.size(); k++)
      if (slots[k].code)
        for (int e = 0; e < 13; e++) CHECK(slots[k].row[e] == 0.0);
    // I = 0: every pose and extrinsic comes back bit for bit
    p.iterations = 0;
    calib_seq(T0.data(), E_nom.data(), cams.data(), frames.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p, cp,
                   T_out.data(), res, nullptr);
    CHECK(std::memcmp(T_out.data(), T0.data(), sizeof(double) * 16 * N) == 0 && res.iterations_run == 0);
    CHECK(std::memcmp(res.T_base_cam, E_nom.data(), sizeof(double) * 16 * C) == 0);
    // R = 1: three samples; whatever the rule says, finite
    p.iterations = 3;
    p.half_window = 1;
    calib_seq(T_true.data(), E_true.data(), cams.data(), frames.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p,
                   cp, T_out.data(), res, nullptr);
    for (size_t e = 0; e < T_out.size(); e++) CHECK(std::isfinite(T_out[e]));
    // starved: the last view black (a view's gate), then the displaced free camera black in every view (a camera's)
    p.half_window = 6;
    std::vector<uint8_t> black((size_t)W * H * 3, 0);
    std::vector<const uint8_t*> fb = frames;
    for (int c = 0; c < C; c++) fb[(N - 1) * C + c] = black.data();
    calib_seq(T0.data(), E_nom.data(), cams.data(), fb.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p, cp,
                   T_out.data(), res, nullptr);
    CHECK(res.status == lc::kStarved && res.calibrated == 0 && std::memcmp(T_out.data(), T0.data(), sizeof(double) * 16 * N) == 0);
    fb = frames;
    for (int r = 0; r < N; r++) fb[r * C + moved] = black.data();
    calib_seq(T0.data(), E_nom.data(), cams.data(), fb.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p, cp,
                   T_out.data(), res, nullptr);
    CHECK(res.status == lc::kStarved && res.n_obs_cam[0][moved] == 0 && res.n_obs[0] > 12 * N);
    CHECK(std::memcmp(res.T_base_cam, E_nom.data(), sizeof(double) * 16 * C) == 0);
    // no candidates at all
    calib_seq(T0.data(), E_nom.data(), cams.data(), frames.data(), N, C, W, H, X.data(), n, 0, cand.data(), 0, p, cp,
                   T_out.data(), res, nullptr);
    CHECK(res.status == lc::kStarved && res.rms[0] == 0.0);
  }
}

int main() {
  check_windows();
  check_passes();
  check_seq();
  if (g_fail) {
    std::printf("calibcheck: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("calibcheck ok\n");
  return 0;
}
