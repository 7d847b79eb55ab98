// Intrinsic calibration (mantis_calibrate_intrinsics, include/mantis.h): a
// joint Gauss-Newton over the base poses of N views of one rig and the eight
// intrinsics (fx, fy, cx, cy, k1..k4) of its free cameras, on the grid lines.
// One observation is the line refinement's (mk_refine.h, steps 1-8) at the
// camera's current intrinsic estimate; its row [J_pose | J_int | r] has 15
// entries. The normal system is solved through the Schur complement of the
// poses, as the extrinsic calibration's (mk_calib.h, whose 6 x 6 pieces, pose
// update and starved gate are used as they are). The rules here are shared by
// the device (k_icalib_obs / k_icalib_rig / k_icalib_solve, icalib_impl.hip)
// and the host build of the CPU tests (hostcheck.cpp hc_icalib_*,
// tools/icalibcheck_main.cpp). Both builds keep -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "mk_calib.h"

namespace mk {
namespace icalib {

constexpr int kMaxCams = refine::kMaxCams;
constexpr int kMaxViews = calib::kMaxViews;
constexpr int kP = 8;                 // intrinsics of a camera: fx, fy, cx, cy, k1..k4
constexpr int kMaxS = kP * kMaxCams;  // unknowns of the reduced system
constexpr int kLd = kMaxS + 1;        // leading dimension of [E | a], Y, the Schur terms and [S | s]
constexpr int kRow = 15;              // [J_pose (6) | J_int (8) | r]
constexpr int kAcc = 120;             // upper triangle of a 15 x 15
constexpr int kOk = 0, kStarved = 1, kSingular = 2, kDiverged = 3;

// one (view, camera, candidate) slot (row: zeros unless code = 0): 136 bytes
struct Slot {
  double row[kRow];
  int32_t code, Sw, Skw, pad;
};

// index of entry (a, b), a <= b < 15, of the upper triangle laid out row by row
MK_HD int tri(int a, int b) { return a * kRow - a * (a - 1) / 2 + (b - a); }
MK_HD int tri_sym(int a, int b) { return a <= b ? tri(a, b) : tri(b, a); }

// the camera's intrinsics as the eight unknowns and back (Cam is fx, fy, cx, cy, k[4])
MK_HD void cam_to(const Cam& cm, double* th) {
  th[0] = cm.fx; th[1] = cm.fy; th[2] = cm.cx; th[3] = cm.cy;
  for (int i = 0; i < 4; i++) th[4 + i] = cm.k[i];
}
MK_HD Cam cam_of(const double* K4, const double* D4) {
  Cam cm;
  cm.fx = K4[0]; cm.fy = K4[1]; cm.cx = K4[2]; cm.cy = K4[3];
  for (int i = 0; i < 4; i++) cm.k[i] = D4[i];
  return cm;
}

// atan of rho > 0 for J_int. J_int has entries that are small by cancellation
// (a line whose normal is nearly orthogonal to G^-1's columns), where one ulp
// of theta shows as 1e-12 of the entry; so both builds take the same
// operations: the device mk_dmath.h's atan_pos, the host its reduction and
// polynomial restated with the same constants (fma is exactly rounded on both).
#if MK_DM_DEVICE
MK_HD double atan_rho(double x, double inv) { return dm::atan_pos(x, inv); }
#else
MK_HD double atan_rho(double x, double inv) {
  static const unsigned long long kC[19] = {
      0xBF23E260BD3237F4ull, 0x3F4B2BB069EFB384ull, 0xBF67952DAF56DE9Bull, 0x3F7D6D43A595C56Full,
      0xBF8C6EA4A57D9582ull, 0x3F967E295F08B19Full, 0xBF9E9AE6FC27006Aull, 0x3FA2C15B5711927Aull,
      0xBFA59976E82D3FF0ull, 0x3FA82D5D6EF28734ull, 0xBFAAE5CE6A214619ull, 0x3FAE1BB48427B883ull,
      0xBFB110E48B207F05ull, 0x3FB3B13657B87036ull, 0xBFB745D119378E4Full, 0x3FBC71C717E1913Cull,
      0xBFC2492492376B7Dull, 0x3FC99999999952CCull, 0xBFD5555555555523ull};
  auto kd = [](unsigned long long b) {
    double d;
    __builtin_memcpy(&d, &b, sizeof(d));
    return d;
  };
  const bool big = x > 1.0;
  const double a = big ? inv : x;
  const double s = a * a;
  double p = kd(0x3EEBA404B5E68A13ull);
  for (int i = 0; i < 19; i++) p = __builtin_fma(s, p, kd(kC[i]));
  const double q = s * p;
  const double red = __builtin_fma(a, q, a);
  return big ? __builtin_fma(kd(0x3FEDD9AD336A0500ull), kd(0x3FFAF154EEB562D6ull), -red) : red;
}
#endif

// J_int = nh^T G^-1 Q at m0 (include/mantis.h): the relative perturbation of
// (fx, fy, cx, cy) and the additive one of k1..k4. A held camera: eight zeros;
// a held parameter (its bit of param_mask clear): a zero.
MK_HD void jint(const Cam& cm, const double* m0, const double* nh, bool free_cam, uint32_t param_mask, double* Ji) {
  if (!free_cam) {
    for (int e = 0; e < kP; e++) Ji[e] = 0.0;
    return;
  }
  const double x = m0[0], y = m0[1];
  const double rho = sqrt(x * x + y * y);
  double c = 1.0, g00 = 1.0, g01 = 0.0, g11 = 1.0, kc[4] = {0.0, 0.0, 0.0, 0.0};
  if (rho > 1e-8) {
    const double ir = 1.0 / rho;
    const double t = atan_rho(rho, ir);
    const double t2 = t * t, t3 = t2 * t, t4 = t2 * t2, t5 = t4 * t, t6 = t3 * t3, t7 = t6 * t, t8 = t4 * t4,
                 t9 = t8 * t;
    const double td = t + cm.k[0] * t3 + cm.k[1] * t5 + cm.k[2] * t7 + cm.k[3] * t9;
    const double tdp = 1.0 + 3.0 * cm.k[0] * t2 + 5.0 * cm.k[1] * t4 + 7.0 * cm.k[2] * t6 + 9.0 * cm.k[3] * t8;
    c = td * ir;
    const double cp = (tdp / (1.0 + rho * rho) - c) * ir;
    const double cr = cp * ir;
    g00 = c + cr * x * x;
    g01 = cr * x * y;
    g11 = c + cr * y * y;
    kc[0] = t3 * ir;
    kc[1] = t5 * ir;
    kc[2] = t7 * ir;
    kc[3] = t9 * ir;
  }
  const double det = g00 * g11 - g01 * g01;
  const double w0 = (nh[0] * g11 - nh[1] * g01) / det, w1 = (nh[1] * g00 - nh[0] * g01) / det;  // nh^T G^-1
  const double wm = w0 * x + w1 * y;
  Ji[0] = w0 * (c * x);
  Ji[1] = w1 * (c * y);
  Ji[2] = w0;
  Ji[3] = w1;
  for (int i = 0; i < 4; i++) Ji[4 + i] = wm * kc[i];
  for (int e = 0; e < kP; e++)
    if (!(param_mask >> e & 1u)) Ji[e] = 0.0;
}

// the 15-entry slot from the refinement's slot of the same observation and J_int
MK_HD void widen(const refine::Slot& s, const double* Ji, Slot& o) {
  for (int e = 0; e < 6; e++) o.row[e] = s.row[e];
  for (int e = 0; e < kP; e++) o.row[6 + e] = s.code ? 0.0 : Ji[e];
  o.row[14] = s.row[6];
  o.code = s.code;
  o.Sw = s.Sw;
  o.Skw = s.Skw;
  o.pad = 0;
}

// One observation on the host: refine::observe at the current intrinsics, then their columns.
MK_HD void observe(const double* Rwb_t, const double* twb, const GnCam& cm, const Cam& cam, const uint8_t* bgr, int W,
                   int H, const double* X, int axis, const int* target, const refine::Window& win, bool free_cam,
                   uint32_t param_mask, Slot& o, int* tie) {
  refine::Slot s;
  refine::observe(Rwb_t, twb, cm, cam, bgr, W, H, X, axis, target, win, s, tie);
  double Ji[kP];
  for (int e = 0; e < kP; e++) Ji[e] = 0.0;
  if (!s.code) {
    refine::Geom g;
    (void)refine::geom(Rwb_t, twb, cm, X, axis, g);
    jint(cam, g.m0, g.nh, free_cam, param_mask, Ji);
  }
  widen(s, Ji, o);
}

MK_HD void accumulate_row(const double* v, double* acc120) {
  int n = 0;
  for (int a = 0; a < kRow; a++)
    for (int b = a; b < kRow; b++) acc120[n++] += v[a] * v[b];
}

// ---- the reduced system. acc: a view's C x 120 (or every view's N x C x 120) ----
// A_r(i, j) = sum_c PP_rc(i, j) in camera order, + lambda on the diagonal
MK_HD double view_A(const double* acc, int C, int i, int j, double lambda) {
  const int e = tri_sym(i, j);
  double s = 0.0;
  for (int c = 0; c < C; c++) s += acc[kAcc * c + e];
  return i == j ? s + lambda : s;
}
// [E_r | a_r](k, j): column j < nS is column j % 8 of PI of free camera j / 8; column nS is sum_c Pr_rc
MK_HD double view_rhs(const double* acc, int C, const int* fcam, int nS, int k, int j) {
  if (j < nS) return acc[kAcc * fcam[j / kP] + tri(k, 6 + j % kP)];
  double s = 0.0;
  for (int c = 0; c < C; c++) s += acc[kAcc * c + tri(k, 14)];
  return s;
}
// the view's Schur term (E_r^T Y_r)(i, j), Y_r = A_r^-1 [E_r | a_r]; Em and Y: 6 x kLd
MK_HD double schur_entry(const double* Em, const double* Y, int i, int j) {
  double s = 0.0;
  for (int k = 0; k < 6; k++) s += Em[kLd * k + i] * Y[kLd * k + j];
  return s;
}
// x = A_r^-1 b for strided columns of leading dimension kLd (calib::chol6_solve)
MK_HD void view_solve(const double* L6, const double* b, double* x) { calib::chol6_solve(L6, b, kLd, x, kLd); }
// [S | s](i, j), i < nS, j <= nS: S = B - sum_r E_r^T A_r^-1 E_r, s = -b + sum_r E_r^T A_r^-1 a_r,
// every sum in view order; a held parameter's diagonal entry of B is exactly 1.
// acc: N x C x 120; Wt: the views' Schur terms, N x kMaxS x kLd.
MK_HD double reduced_entry(const double* acc, const double* Wt, int N, int C, const int* fcam, int nS, int i, int j,
                           double lambda, uint32_t param_mask) {
  double sw = 0.0;
  for (int r = 0; r < N; r++) sw += Wt[((size_t)r * kMaxS + i) * kLd + j];
  const double* a0 = acc + kAcc * fcam[i / kP];
  const size_t vs = (size_t)kAcc * C;
  if (j == nS) {
    double b = 0.0;
    for (int r = 0; r < N; r++) b += a0[vs * r + tri(6 + i % kP, 14)];
    return -b + sw;
  }
  double B = 0.0;
  if (i / kP == j / kP) {
    const int e = tri_sym(6 + i % kP, 6 + j % kP);
    for (int r = 0; r < N; r++) B += a0[vs * r + e];
    if (i == j) {
      B += lambda;
      if (!(param_mask >> (i % kP) & 1u)) B = 1.0;
    }
  }
  return B - sw;
}
// Left-looking Cholesky of S (lower triangle, leading dimension kLd), column j:
// the pivot's square and an entry below it, each by the sequential formula.
// L's diagonal is kept apart (Ld), so L's strict lower triangle may overwrite
// S's in place: entry (i, j) of S is read by its own column only, S's
// diagonal never goes.
MK_HD double cholS_pivot(const double* S, const double* L, int j) {
  double s = S[kLd * j + j];
  for (int k = 0; k < j; k++) s -= L[kLd * j + k] * L[kLd * j + k];
  return s;
}
MK_HD double cholS_below(const double* S, const double* L, int i, int j, double ljj) {
  double s = S[kLd * i + j];
  for (int k = 0; k < j; k++) s -= L[kLd * i + k] * L[kLd * j + k];
  return s / ljj;
}
// x = (L L^T)^-1 b for the n x n factor; b strided, y: n of scratch
MK_HD void cholS_solve(const double* L, const double* Ld, int n, const double* b, int ldb, double* y, double* x) {
  for (int i = 0; i < n; i++) {
    double s = b[ldb * i];
    for (int k = 0; k < i; k++) s -= L[kLd * i + k] * y[k];
    y[i] = s / Ld[i];
  }
  for (int i = n - 1; i >= 0; i--) {
    double s = y[i];
    for (int k = i + 1; k < n; k++) s -= L[kLd * k + i] * x[k];
    x[i] = s / Ld[i];
  }
}
// delta_r = -A_r^-1 (a_r + E_r eps) from the stored Y_r = A_r^-1 [E_r | a_r]
MK_HD void pose_delta(const double* Y, const double* eps, int nS, double* d6) {
  for (int k = 0; k < 6; k++) {
    double s = Y[kLd * k + nS];
    for (int j = 0; j < nS; j++) s += Y[kLd * k + j] * eps[j];
    d6[k] = -s;
  }
}
// theta <- theta (+) eps for the free parameters (fx, fy before the update scale
// cx's and cy's steps); false when the result diverged: fx or fy not finite or
// <= 0, or any updated parameter not finite. th: fx, fy, cx, cy, k1..k4.
MK_HD bool param_update(const double* th, const double* eps, uint32_t param_mask, double* out) {
  for (int e = 0; e < kP; e++) out[e] = th[e];
  if (param_mask & 1u) out[0] = th[0] * (1.0 + eps[0]);
  if (param_mask & 2u) out[1] = th[1] * (1.0 + eps[1]);
  if (param_mask & 4u) out[2] = th[2] + th[0] * eps[2];
  if (param_mask & 8u) out[3] = th[3] + th[1] * eps[3];
  for (int i = 0; i < 4; i++)
    if (param_mask >> (4 + i) & 1u) out[4 + i] = th[4 + i] + eps[4 + i];
  bool ok = out[0] > 0 && out[1] > 0;
  for (int e = 0; e < kP; e++) ok = ok && (out[e] - out[e] == 0.0);  // finite
  return ok;
}

// the starved gate of a pass (the extrinsic calibration's)
MK_HD bool starved(const int32_t* cnt, int N, int C, uint32_t free_cams, int32_t min_obs, int32_t min_obs_cam) {
  return calib::starved(cnt, N, C, free_cams, min_obs, min_obs_cam);
}
// r^T r of a pass, summed in (view, camera) order
MK_HD double sum_rr(const double* acc, int N, int C) {
  double s = 0.0;
  for (int k = 0; k < N * C; k++) s += acc[(size_t)kAcc * k + (kAcc - 1)];
  return s;
}

// ---- host: the views' elimination and the reduced system as plain loops ----
struct Reduced {
  std::vector<double> Y, Wt, S, L, Ld;  // N x 6 x kLd, N x kMaxS x kLd, kMaxS x kLd twice, kMaxS
  int fcam[kMaxCams], F, nS;
};
// 0, or 1 / 2 when some A_r / S is not positive definite
inline int reduce(const double* acc, int N, int C, uint32_t free_cams, uint32_t param_mask, double lambda, Reduced& w) {
  w.F = calib::free_list(free_cams, C, w.fcam);
  w.nS = kP * w.F;
  const int nS = w.nS;
  w.Y.assign((size_t)N * 6 * kLd, 0.0);
  w.Wt.assign((size_t)N * kMaxS * kLd, 0.0);
  w.S.assign((size_t)kMaxS * kLd, 0.0);
  w.L.assign((size_t)kMaxS * kLd, 0.0);
  w.Ld.assign((size_t)kMaxS, 0.0);
  for (int r = 0; r < N; r++) {
    const double* av = acc + (size_t)kAcc * C * r;
    double A[36], L6[36], Em[6 * kLd];
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) A[6 * i + j] = view_A(av, C, i, j, lambda);
    if (!calib::chol6(A, L6)) return 1;
    for (int k = 0; k < 6; k++)
      for (int j = 0; j <= nS; j++) Em[kLd * k + j] = view_rhs(av, C, w.fcam, nS, k, j);
    double* Y = w.Y.data() + (size_t)r * 6 * kLd;
    for (int j = 0; j <= nS; j++) view_solve(L6, Em + j, Y + j);
    double* Wr = w.Wt.data() + (size_t)r * kMaxS * kLd;
    for (int i = 0; i < nS; i++)
      for (int j = 0; j <= nS; j++) Wr[kLd * i + j] = schur_entry(Em, Y, i, j);
  }
  for (int i = 0; i < nS; i++)
    for (int j = 0; j <= nS; j++)
      w.S[kLd * i + j] = reduced_entry(acc, w.Wt.data(), N, C, w.fcam, nS, i, j, lambda, param_mask);
  for (int j = 0; j < nS; j++) {
    const double d = cholS_pivot(w.S.data(), w.L.data(), j);
    if (!(d > 0)) return 2;
    const double ljj = sqrt(d);
    w.Ld[j] = ljj;
    for (int i = j + 1; i < nS; i++) w.L[kLd * i + j] = cholS_below(w.S.data(), w.L.data(), i, j, ljj);
  }
  return 0;
}

// the figures of pass `pass` from its counts and accumulators
inline void tally(const double* acc, const int32_t* cnt, int N, int C, int pass, mantis_icalib_result& R) {
  int32_t n = 0;
  for (int c = 0; c < kMaxCams; c++) R.n_obs_cam[pass][c] = 0;
  for (int r = 0; r < N; r++)
    for (int c = 0; c < C; c++) {
      R.n_obs_cam[pass][c] += cnt[r * C + c];
      n += cnt[r * C + c];
    }
  R.n_obs[pass] = n;
  R.rms[pass] = n > 0 ? sqrt(sum_rr(acc, N, C) / (double)n) : 0.0;
}

// The end of pass `pass` (0 .. I; pass I is the final one and solves nothing)
// from the views' accumulators (N x C x 120) and counts (N x C). Returns true
// when the call is finished (the final pass, STARVED, SINGULAR or DIVERGED);
// otherwise T (N x 16) and R.K / R.D are the next estimates, delta (N x 6,
// nullable) the poses' steps and R.delta_cam[pass] the cameras'.
inline bool end_pass(const double* acc, const int32_t* cnt, int N, int C, uint32_t free_cams, uint32_t param_mask,
                     int pass, int I, int32_t min_obs, int32_t min_obs_cam, double lambda, double* T,
                     mantis_icalib_result& R, double* delta) {
  tally(acc, cnt, N, C, pass, R);
  if (pass >= I) return true;
  if (starved(cnt, N, C, free_cams, min_obs, min_obs_cam)) {
    R.status = kStarved;
    return true;
  }
  Reduced w;
  if (reduce(acc, N, C, free_cams, param_mask, lambda, w)) {
    R.status = kSingular;
    return true;
  }
  double eps[kMaxS], y[kMaxS], next[kMaxCams][kP];
  cholS_solve(w.L.data(), w.Ld.data(), w.nS, w.S.data() + w.nS, kLd, y, eps);
  bool ok = true;
  for (int f = 0; f < w.F; f++) {
    double th[kP];
    cam_to(cam_of(R.K[w.fcam[f]], R.D[w.fcam[f]]), th);
    ok = param_update(th, eps + kP * f, param_mask, next[f]) && ok;
  }
  if (!ok) {
    R.status = kDiverged;
    return true;
  }
  for (int r = 0; r < N; r++) {
    double d6[6];
    pose_delta(w.Y.data() + (size_t)r * 6 * kLd, eps, w.nS, d6);
    calib::right_update(T + 16 * (size_t)r, d6);
    if (delta)
      for (int e = 0; e < 6; e++) delta[6 * (size_t)r + e] = d6[e];
  }
  for (int f = 0; f < w.F; f++) {
    const int c = w.fcam[f];
    for (int e = 0; e < 4; e++) {
      R.K[c][e] = next[f][e];
      R.D[c][e] = next[f][4 + e];
    }
    for (int e = 0; e < kP; e++) R.delta_cam[pass][c][e] = (param_mask >> e & 1u) ? eps[kP * f + e] : 0.0;
  }
  R.iterations_run = pass + 1;
  return false;
}

// Host: the gate, rms_cam and the covariances from the last pass's
// accumulators and counts (include/mantis.h). R.K holds the final intrinsics:
// they scale the covariance to natural units.
inline void conclude(const double* acc, const int32_t* cnt, int N, int C, uint32_t free_cams, uint32_t param_mask,
                     int32_t min_obs, int32_t min_obs_cam, double max_rms, mantis_icalib_result& R) {
  const int fp = R.iterations_run;
  for (int c = 0; c < kMaxCams; c++) {
    R.rms_cam[c] = 0.0;
    for (int e = 0; e < kP * kP; e++) R.covariance[c][e] = 0.0;
  }
  for (int c = 0; c < C; c++) {
    double s = 0.0;
    for (int r = 0; r < N; r++) s += acc[(size_t)kAcc * (r * C + c) + (kAcc - 1)];
    if (R.n_obs_cam[fp][c] > 0) R.rms_cam[c] = sqrt(s / (double)R.n_obs_cam[fp][c]);
  }
  int fcam[kMaxCams];
  const int F = calib::free_list(free_cams, C, fcam);
  int np = 0;
  for (int e = 0; e < kP; e++) np += (int)(param_mask >> e & 1u);
  const int64_t dof = (int64_t)R.n_obs[fp] - 6 * (int64_t)N - (int64_t)np * F;
  R.calibrated = R.status == kOk && !starved(cnt, N, C, free_cams, min_obs, min_obs_cam) &&
                 (max_rms <= 0 || R.rms[fp] <= max_rms) && dof > 0;
  if (!R.calibrated) return;
  Reduced w;
  if (reduce(acc, N, C, free_cams, param_mask, 0.0, w)) {
    R.calibrated = 0;
    return;
  }
  const double sigma2 = sum_rr(acc, N, C) / (double)dof;
  for (int f = 0; f < F; f++) {
    double* cov = R.covariance[fcam[f]];
    const double* K4 = R.K[fcam[f]];
    const double sc[kP] = {K4[0], K4[1], K4[0], K4[1], 1.0, 1.0, 1.0, 1.0};
    for (int col = 0; col < kP; col++) {
      if (!(param_mask >> col & 1u)) continue;
      double e[kMaxS], y[kMaxS], x[kMaxS];
      for (int i = 0; i < w.nS; i++) e[i] = i == kP * f + col ? 1.0 : 0.0;
      cholS_solve(w.L.data(), w.Ld.data(), w.nS, e, 1, y, x);
      for (int i = 0; i < kP; i++)
        if (param_mask >> i & 1u) cov[kP * i + col] = sc[i] * (sigma2 * x[kP * f + i]) * sc[col];
    }
    for (int i = 0; i < kP; i++)  // the two triangles came from different solves: publish one
      for (int j = i + 1; j < kP; j++) cov[kP * j + i] = cov[kP * i + j];
  }
}

// The whole call on the host, rows summed in slot order (slot = camera x
// n_cand + candidate inside a view). frames[r * C + c]: W x H, stride 3 W;
// Tbc: the extrinsics, C x 16; cams: the starting intrinsics (K already
// rounded to float); T_in / T_out: N x 16. slots (nullable): N x C x n_cand
// of the last pass taken.
inline void icalib_seq(const double* T_in, const double* Tbc, const Cam* cams, const uint8_t* const* frames, int N, int C,
                       int W, int H, const double* X, int nw, int nr, const int32_t* cand, int n_cand,
                       const mantis_refine_params& p, const mantis_icalib_params& ip, double* T_out,
                       mantis_icalib_result& R, Slot* slots) {
  R = mantis_icalib_result{};
  R.n_cand = n_cand;
  R.n_rigs = N;
  R.n_cams = C;
  R.free_cams = ip.free_cams;
  R.param_mask = ip.param_mask;
  const uint32_t fm = (uint32_t)ip.free_cams, pm = (uint32_t)ip.param_mask;
  for (int c = 0; c < C; c++) {
    double th[kP];
    cam_to(cams[c], th);
    for (int e = 0; e < 4; e++) {
      R.K[c][e] = th[e];
      R.D[c][e] = th[4 + e];
    }
  }
  for (size_t e = 0; e < 16 * (size_t)N; e++) T_out[e] = T_in[e];
  const refine::Window win{p.half_window, p.white_thresh, p.min_weight, 0};
  std::vector<double> acc((size_t)N * C * kAcc);
  std::vector<int32_t> cnt((size_t)N * C);
  for (int pass = 0; pass <= p.iterations; pass++) {
    for (int r = 0; r < N; r++) {
      double Rt[9], t[3];
      refine::pose_parts(T_out + 16 * (size_t)r, Rt, t);
      for (int c = 0; c < C; c++) {
        GnCam gc;
        refine::gncam_from(Tbc + 16 * c, gc);
        const Cam cm = cam_of(R.K[c], R.D[c]);
        double* a = acc.data() + (size_t)kAcc * (r * C + c);
        for (int e = 0; e < kAcc; e++) a[e] = 0.0;
        int32_t n = 0;
        for (int k = 0; k < n_cand; k++) {
          const int i = cand[k] & 0xffff, axis = cand[k] >> 16;
          int tg[3];
          refine::target_bgr(i, nw, nr, tg);
          Slot o;
          observe(Rt, t, gc, cm, frames[r * C + c], W, H, X + 3 * i, axis, tg, win, (fm >> c & 1) != 0, pm, o, nullptr);
          if (slots) slots[((size_t)r * C + c) * n_cand + k] = o;
          accumulate_row(o.row, a);
          n += o.code == 0;
        }
        cnt[r * C + c] = n;
      }
    }
    if (end_pass(acc.data(), cnt.data(), N, C, fm, pm, pass, p.iterations, p.min_obs, ip.min_obs_cam, p.lambda, T_out,
                 R, nullptr))
      break;
  }
  conclude(acc.data(), cnt.data(), N, C, fm, pm, p.min_obs, ip.min_obs_cam, p.max_rms, R);
}

}  // namespace icalib
}  // namespace mk
