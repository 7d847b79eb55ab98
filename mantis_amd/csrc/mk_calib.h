// Extrinsic calibration (mantis_calibrate_extrinsics, include/mantis.h): a
// joint Gauss-Newton over the base poses of N views of one rig and the
// extrinsics of its free cameras, on the grid lines. One observation is the
// line refinement's (mk_refine.h, steps 1-8) at the camera's current
// extrinsic estimate; its row [J_pose | J_ext | r] has 13 entries. The normal
// system is solved through the Schur complement of the poses. The rules here
// are shared by the device (k_calib_obs / k_calib_rig / k_calib_solve,
// calib_impl.hip) and the host build of the CPU tests (hostcheck.cpp
// hc_calib_*, tools/calibcheck_main.cpp). Both builds keep -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "mk_refine.h"

namespace mk {
namespace calib {

constexpr int kMaxCams = refine::kMaxCams;
constexpr int kMaxViews = 256;
constexpr int kMaxS = 6 * (kMaxCams - 1);  // unknowns of the reduced system: 6 per free camera
constexpr int kLd = kMaxS + 1;             // leading dimension of [E | a], Y, the Schur terms and [S | s]
constexpr int kAcc = 91;                   // upper triangle of a 13 x 13
constexpr int kOk = 0, kStarved = 1, kSingular = 2;

// one (view, camera, candidate) slot: [J_pose (6) | J_ext (6) | r] (zeros unless code = 0): 120 bytes
struct Slot {
  double row[13];
  int32_t code, Sw, Skw, pad;
};

// index of entry (a, b), a <= b < 13, of the upper triangle laid out row by row
MK_HD int tri(int a, int b) { return a * 13 - a * (a - 1) / 2 + (b - a); }

// the free cameras in ascending order: fcam[f] = camera of block f; returns F
MK_HD int free_list(uint32_t free_cams, int C, int* fcam) {
  int F = 0;
  for (int c = 0; c < C; c++)
    if (free_cams >> c & 1) fcam[F++] = c;
  return F;
}

// refine::geom (the same expressions: the same bits) and the extrinsic's
// Jacobian Je = [-g | g [p]x], g = nh^T Jpi, p the point in the camera frame,
// for the right perturbation E <- E D(eps): p' = D^-1 p = p - rho + [p]x phi
// to first order. A held camera (free_cam = false): six zeros.
struct Geom {
  refine::Geom g;
  double Je[6];
};
MK_HD int geom(const double* Rwb_t, const double* twb, const GnCam& cm, const double* X, int axis, bool free_cam,
               Geom& o) {
  refine::Geom& g = o.g;
  const double d[3] = {X[0] - twb[0], X[1] - twb[1], X[2] - twb[2]};
  double q[3], p[3];
  for (int a = 0; a < 3; a++) q[a] = Rwb_t[3 * a] * d[0] + Rwb_t[3 * a + 1] * d[1] + Rwb_t[3 * a + 2] * d[2];
  for (int a = 0; a < 3; a++)
    p[a] = cm.R_cb[3 * a] * q[0] + cm.R_cb[3 * a + 1] * q[1] + cm.R_cb[3 * a + 2] * q[2] + cm.t_cb[a];
  if (!(p[2] > 0)) return refine::kBehind;
  const double iz = 1.0 / p[2];
  g.m0[0] = p[0] * iz;
  g.m0[1] = p[1] * iz;
  const double j02 = -p[0] * iz * iz, j12 = -p[1] * iz * iz;
  const double w[3] = {Rwb_t[axis], Rwb_t[3 + axis], Rwb_t[6 + axis]};
  double v[3];
  for (int a = 0; a < 3; a++) v[a] = cm.R_cb[3 * a] * w[0] + cm.R_cb[3 * a + 1] * w[1] + cm.R_cb[3 * a + 2] * w[2];
  const double tx = iz * v[0] + j02 * v[2], ty = iz * v[1] + j12 * v[2];
  const double tn = sqrt(tx * tx + ty * ty);
  if (!(tn >= 1e-12)) return refine::kNoTangent;
  g.nh[0] = -(ty / tn);
  g.nh[1] = tx / tn;
  const double gg[3] = {g.nh[0] * iz, g.nh[1] * iz, g.nh[0] * j02 + g.nh[1] * j12};
  double h[3];
  for (int b = 0; b < 3; b++) h[b] = gg[0] * cm.R_cb[b] + gg[1] * cm.R_cb[3 + b] + gg[2] * cm.R_cb[6 + b];
  g.J[0] = -h[0];
  g.J[1] = -h[1];
  g.J[2] = -h[2];
  g.J[3] = h[1] * q[2] - h[2] * q[1];
  g.J[4] = -h[0] * q[2] + h[2] * q[0];
  g.J[5] = h[0] * q[1] - h[1] * q[0];
  if (free_cam) {
    o.Je[0] = -gg[0];
    o.Je[1] = -gg[1];
    o.Je[2] = -gg[2];
    o.Je[3] = gg[1] * p[2] - gg[2] * p[1];
    o.Je[4] = -gg[0] * p[2] + gg[2] * p[0];
    o.Je[5] = gg[0] * p[1] - gg[1] * p[0];
  } else {
    for (int e = 0; e < 6; e++) o.Je[e] = 0.0;
  }
  return 0;
}

// the 13-entry slot from the refinement's slot of the same observation and Je
MK_HD void widen(const refine::Slot& s, const double* Je, Slot& o) {
  for (int e = 0; e < 6; e++) o.row[e] = s.row[e];
  for (int e = 0; e < 6; e++) o.row[6 + e] = s.code ? 0.0 : Je[e];
  o.row[12] = s.row[6];
  o.code = s.code;
  o.Sw = s.Sw;
  o.Skw = s.Skw;
  o.pad = 0;
}

// One observation on the host: refine::observe, then the extrinsic's columns.
MK_HD void observe(const double* Rwb_t, const double* twb, const GnCam& cm, const Cam& cam, const uint8_t* bgr, int W,
                   int H, const double* X, int axis, const int* target, const refine::Window& win, bool free_cam, Slot& o,
                   int* tie) {
  refine::Slot s;
  refine::observe(Rwb_t, twb, cm, cam, bgr, W, H, X, axis, target, win, s, tie);
  Geom g;
  for (int e = 0; e < 6; e++) g.Je[e] = 0.0;
  if (!s.code) (void)geom(Rwb_t, twb, cm, X, axis, free_cam, g);
  widen(s, g.Je, o);
}

MK_HD void accumulate_row(const double* v, double* acc91) {
  int n = 0;
  for (int a = 0; a < 13; a++)
    for (int b = a; b < 13; b++) acc91[n++] += v[a] * v[b];
}

// ---- the reduced system. acc: a view's C x 91 (or every view's N x C x 91) ----
// A_r(i, j) = sum_c PP_rc(i, j) in camera order, + lambda on the diagonal
MK_HD double view_A(const double* acc, int C, int i, int j, double lambda) {
  const int e = i <= j ? tri(i, j) : tri(j, i);
  double s = 0.0;
  for (int c = 0; c < C; c++) s += acc[kAcc * c + e];
  return i == j ? s + lambda : s;
}
// [E_r | a_r](k, j): column j < nS is column j % 6 of PE of free camera j / 6; column nS is sum_c Pr_rc
MK_HD double view_rhs(const double* acc, int C, const int* fcam, int nS, int k, int j) {
  if (j < nS) return acc[kAcc * fcam[j / 6] + tri(k, 6 + j % 6)];
  double s = 0.0;
  for (int c = 0; c < C; c++) s += acc[kAcc * c + tri(k, 12)];
  return s;
}
// gn_solve6's Cholesky loop on a row-major 6 x 6; false when it is not positive definite
MK_HD bool chol6(const double* A, double* L) {
  for (int e = 0; e < 36; e++) L[e] = 0.0;
  for (int i = 0; i < 6; i++)
    for (int j = 0; j <= i; j++) {
      double s = A[6 * i + j];
      for (int k = 0; k < j; k++) s -= L[6 * i + k] * L[6 * j + k];
      if (i == j) {
        if (!(s > 0)) return false;
        L[6 * i + i] = sqrt(s);
      } else {
        L[6 * i + j] = s / L[6 * j + j];
      }
    }
  return true;
}
// x = (L L^T)^-1 b; b and x are strided columns
MK_HD void chol6_solve(const double* L, const double* b, int ldb, double* x, int ldx) {
  double y[6];
  for (int i = 0; i < 6; i++) {
    double s = b[ldb * i];
    for (int k = 0; k < i; k++) s -= L[6 * i + k] * y[k];
    y[i] = s / L[6 * i + i];
  }
  for (int i = 5; i >= 0; i--) {
    double s = y[i];
    for (int k = i + 1; k < 6; k++) s -= L[6 * k + i] * x[ldx * k];
    x[ldx * i] = s / L[6 * i + i];
  }
}
// the view's Schur term (E_r^T Y_r)(i, j), Y_r = A_r^-1 [E_r | a_r]; Em and Y: 6 x kLd
MK_HD double schur_entry(const double* Em, const double* Y, int i, int j) {
  double s = 0.0;
  for (int k = 0; k < 6; k++) s += Em[kLd * k + i] * Y[kLd * k + j];
  return s;
}
// [S | s](i, j), i < nS, j <= nS: S = B - sum_r E_r^T A_r^-1 E_r, s = -b + sum_r E_r^T A_r^-1 a_r,
// every sum in view order. acc: N x C x 91; Wt: the views' Schur terms, N x kMaxS x kLd.
MK_HD double reduced_entry(const double* acc, const double* Wt, int N, int C, const int* fcam, int nS, int i, int j,
                           double lambda) {
  double sw = 0.0;
  for (int r = 0; r < N; r++) sw += Wt[((size_t)r * kMaxS + i) * kLd + j];
  const double* a0 = acc + kAcc * fcam[i / 6];
  const size_t vs = (size_t)kAcc * C;
  if (j == nS) {
    double b = 0.0;
    for (int r = 0; r < N; r++) b += a0[vs * r + tri(6 + i % 6, 12)];
    return -b + sw;
  }
  double B = 0.0;
  if (i / 6 == j / 6) {
    const int ii = i % 6, jj = j % 6, e = ii <= jj ? tri(6 + ii, 6 + jj) : tri(6 + jj, 6 + ii);
    for (int r = 0; r < N; r++) B += a0[vs * r + e];
    if (i == j) B += lambda;
  }
  return B - sw;
}
// left-looking Cholesky of S (lower triangle, leading dimension kLd), column j: the pivot's
// square and an entry below it, each by the sequential formula
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
MK_HD void cholS_solve(const double* L, int n, const double* b, int ldb, double* y, double* x) {
  for (int i = 0; i < n; i++) {
    double s = b[ldb * i];
    for (int k = 0; k < i; k++) s -= L[kLd * i + k] * y[k];
    y[i] = s / L[kLd * i + i];
  }
  for (int i = n - 1; i >= 0; i--) {
    double s = y[i];
    for (int k = i + 1; k < n; k++) s -= L[kLd * k + i] * x[k];
    x[i] = s / L[kLd * i + i];
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
// T <- T D(x): gn_solve6's update (Rodrigues rotation x[3..5], translation x[0..2] taken as is)
MK_HD void right_update(double* T, const double* x) {
  const double* w = x + 3;
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  double a, bb;
  if (th < 1e-12) { a = 1.0; bb = 0.5; }
  else { a = sin(th) / th; bb = (1 - cos(th)) / (th * th); }
  double dR[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double s = 0;
      for (int k = 0; k < 3; k++) s += K[i * 3 + k] * K[k * 3 + j];
      dR[i * 3 + j] = (i == j ? 1.0 : 0.0) + a * K[i * 3 + j] + bb * s;
    }
  const double D[16] = {dR[0], dR[1], dR[2], x[0], dR[3], dR[4], dR[5], x[1], dR[6], dR[7], dR[8], x[2], 0, 0, 0, 1};
  double r[16];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      double s = 0;
      for (int k = 0; k < 4; k++) s += T[i * 4 + k] * D[k * 4 + j];
      r[i * 4 + j] = s;
    }
  for (int i = 0; i < 16; i++) T[i] = r[i];
}

// the starved gate of a pass: some view with fewer than min_obs rows over its
// cameras, or some free camera with fewer than min_obs_cam rows over the views
MK_HD bool starved(const int32_t* cnt, int N, int C, uint32_t free_cams, int32_t min_obs, int32_t min_obs_cam) {
  for (int r = 0; r < N; r++) {
    int32_t n = 0;
    for (int c = 0; c < C; c++) n += cnt[r * C + c];
    if (n < min_obs) return true;
  }
  for (int c = 0; c < C; c++) {
    if (!(free_cams >> c & 1)) continue;
    int32_t n = 0;
    for (int r = 0; r < N; r++) n += cnt[r * C + c];
    if (n < min_obs_cam) return true;
  }
  return false;
}
// r^T r of a pass, summed in (view, camera) order
MK_HD double sum_rr(const double* acc, int N, int C) {
  double s = 0.0;
  for (int k = 0; k < N * C; k++) s += acc[(size_t)kAcc * k + 90];
  return s;
}

// ---- host: the views' elimination and the reduced system as plain loops ----
struct Reduced {
  std::vector<double> Y, Wt, S, L;  // N x 6 x kLd, N x kMaxS x kLd, kMaxS x kLd twice
  int fcam[kMaxCams], F, nS;
};
// false when some A_r or S is not positive definite
inline bool reduce(const double* acc, int N, int C, uint32_t free_cams, double lambda, Reduced& w) {
  w.F = free_list(free_cams, C, w.fcam);
  w.nS = 6 * w.F;
  const int nS = w.nS;
  w.Y.assign((size_t)N * 6 * kLd, 0.0);
  w.Wt.assign((size_t)N * kMaxS * kLd, 0.0);
  w.S.assign((size_t)kMaxS * kLd, 0.0);
  w.L.assign((size_t)kMaxS * kLd, 0.0);
  for (int r = 0; r < N; r++) {
    const double* av = acc + (size_t)kAcc * C * r;
    double A[36], L6[36], Em[6 * kLd];
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) A[6 * i + j] = view_A(av, C, i, j, lambda);
    if (!chol6(A, L6)) return false;
    for (int k = 0; k < 6; k++)
      for (int j = 0; j <= nS; j++) Em[kLd * k + j] = view_rhs(av, C, w.fcam, nS, k, j);
    double* Y = w.Y.data() + (size_t)r * 6 * kLd;
    for (int j = 0; j <= nS; j++) chol6_solve(L6, Em + j, kLd, Y + j, kLd);
    double* Wr = w.Wt.data() + (size_t)r * kMaxS * kLd;
    for (int i = 0; i < nS; i++)
      for (int j = 0; j <= nS; j++) Wr[kLd * i + j] = schur_entry(Em, Y, i, j);
  }
  for (int i = 0; i < nS; i++)
    for (int j = 0; j <= nS; j++)
      w.S[kLd * i + j] = reduced_entry(acc, w.Wt.data(), N, C, w.fcam, nS, i, j, lambda);
  for (int j = 0; j < nS; j++) {
    const double d = cholS_pivot(w.S.data(), w.L.data(), j);
    if (!(d > 0)) return false;
    const double ljj = sqrt(d);
    w.L[kLd * j + j] = ljj;
    for (int i = j + 1; i < nS; i++) w.L[kLd * i + j] = cholS_below(w.S.data(), w.L.data(), i, j, ljj);
  }
  return true;
}

// the figures of pass `pass` from its counts and accumulators
inline void tally(const double* acc, const int32_t* cnt, int N, int C, int pass, mantis_calib_result& R) {
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
// from the views' accumulators (N x C x 91) and counts (N x C). Returns true
// when the call is finished (the final pass, STARVED or SINGULAR); otherwise T
// (N x 16) and R.T_base_cam are the next estimates, delta (N x 6, nullable)
// the poses' steps and R.delta_cam[pass] the cameras'.
inline bool end_pass(const double* acc, const int32_t* cnt, int N, int C, uint32_t free_cams, int pass, int I,
                     int32_t min_obs, int32_t min_obs_cam, double lambda, double* T, mantis_calib_result& R,
                     double* delta) {
  tally(acc, cnt, N, C, pass, R);
  if (pass >= I) return true;
  if (starved(cnt, N, C, free_cams, min_obs, min_obs_cam)) {
    R.status = kStarved;
    return true;
  }
  Reduced w;
  if (!reduce(acc, N, C, free_cams, lambda, w)) {
    R.status = kSingular;
    return true;
  }
  double eps[kMaxS], y[kMaxS];
  cholS_solve(w.L.data(), w.nS, w.S.data() + w.nS, kLd, y, eps);
  for (int r = 0; r < N; r++) {
    double d6[6];
    pose_delta(w.Y.data() + (size_t)r * 6 * kLd, eps, w.nS, d6);
    right_update(T + 16 * (size_t)r, d6);
    if (delta)
      for (int e = 0; e < 6; e++) delta[6 * (size_t)r + e] = d6[e];
  }
  for (int f = 0; f < w.F; f++) {
    right_update(R.T_base_cam[w.fcam[f]], eps + 6 * f);
    for (int e = 0; e < 6; e++) R.delta_cam[pass][w.fcam[f]][e] = eps[6 * f + e];
  }
  R.iterations_run = pass + 1;
  return false;
}

// Host: the gate, rms_cam and the covariances from the last pass's
// accumulators and counts. dof = n_obs - 6 N - 6 F; calibrated = status OK, no
// starved gate on that pass, the rms gate, dof > 0 and S (lambda = 0) positive
// definite. Cov_c = (r^T r / dof) (S^-1)_cc, the marginal over the poses;
// order x, y, z, rot-x, rot-y, rot-z of the right perturbation. Otherwise zeros.
inline void conclude(const double* acc, const int32_t* cnt, int N, int C, uint32_t free_cams, int32_t min_obs,
                     int32_t min_obs_cam, double max_rms, mantis_calib_result& R) {
  const int fp = R.iterations_run;
  for (int c = 0; c < kMaxCams; c++) {
    R.rms_cam[c] = 0.0;
    for (int e = 0; e < 36; e++) R.covariance[c][e] = 0.0;
  }
  for (int c = 0; c < C; c++) {
    double s = 0.0;
    for (int r = 0; r < N; r++) s += acc[(size_t)kAcc * (r * C + c) + 90];
    if (R.n_obs_cam[fp][c] > 0) R.rms_cam[c] = sqrt(s / (double)R.n_obs_cam[fp][c]);
  }
  int fcam[kMaxCams];
  const int F = free_list(free_cams, C, fcam);
  const int64_t dof = (int64_t)R.n_obs[fp] - 6 * (int64_t)N - 6 * (int64_t)F;
  R.calibrated = R.status == kOk && !starved(cnt, N, C, free_cams, min_obs, min_obs_cam) &&
                 (max_rms <= 0 || R.rms[fp] <= max_rms) && dof > 0;
  if (!R.calibrated) return;
  Reduced w;
  if (!reduce(acc, N, C, free_cams, 0.0, w)) {
    R.calibrated = 0;
    return;
  }
  const double sigma2 = sum_rr(acc, N, C) / (double)dof;
  for (int f = 0; f < F; f++) {
    double* cov = R.covariance[fcam[f]];
    for (int col = 0; col < 6; col++) {
      double e[kMaxS], y[kMaxS], x[kMaxS];
      for (int i = 0; i < w.nS; i++) e[i] = i == 6 * f + col ? 1.0 : 0.0;
      cholS_solve(w.L.data(), w.nS, e, 1, y, x);
      for (int i = 0; i < 6; i++) cov[6 * i + col] = sigma2 * x[6 * f + i];
    }
    for (int i = 0; i < 6; i++)  // the two triangles came from different solves: publish one
      for (int j = i + 1; j < 6; j++) cov[6 * j + i] = cov[6 * i + j];
  }
}

// The whole call on the host, rows summed in slot order (slot = camera x
// n_cand + candidate inside a view). frames[r * C + c]: W x H, stride 3 W;
// Tbc: the nominal extrinsics, C x 16; T_in / T_out: N x 16. slots (nullable):
// N x C x n_cand of the last pass taken.
inline void calib_seq(const double* T_in, const double* Tbc, const Cam* cams, const uint8_t* const* frames, int N, int C,
                      int W, int H, const double* X, int nw, int nr, const int32_t* cand, int n_cand,
                      const mantis_refine_params& p, const mantis_calib_params& cp, double* T_out,
                      mantis_calib_result& R, Slot* slots) {
  R = mantis_calib_result{};
  R.n_cand = n_cand;
  R.n_rigs = N;
  R.n_cams = C;
  R.free_cams = cp.free_cams;
  const uint32_t fm = (uint32_t)cp.free_cams;
  for (int c = 0; c < C; c++)
    for (int e = 0; e < 16; e++) R.T_base_cam[c][e] = Tbc[16 * c + e];
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
        refine::gncam_from(R.T_base_cam[c], gc);
        double* a = acc.data() + (size_t)kAcc * (r * C + c);
        for (int e = 0; e < kAcc; e++) a[e] = 0.0;
        int32_t n = 0;
        for (int k = 0; k < n_cand; k++) {
          const int i = cand[k] & 0xffff, axis = cand[k] >> 16;
          int tg[3];
          refine::target_bgr(i, nw, nr, tg);
          Slot o;
          observe(Rt, t, gc, cams[c], frames[r * C + c], W, H, X + 3 * i, axis, tg, win, (fm >> c & 1) != 0, o, nullptr);
          if (slots) slots[((size_t)r * C + c) * n_cand + k] = o;
          accumulate_row(o.row, a);
          n += o.code == 0;
        }
        cnt[r * C + c] = n;
      }
    }
    if (end_pass(acc.data(), cnt.data(), N, C, fm, pass, p.iterations, p.min_obs, cp.min_obs_cam, p.lambda, T_out, R,
                 nullptr))
      break;
  }
  conclude(acc.data(), cnt.data(), N, C, fm, p.min_obs, cp.min_obs_cam, p.max_rms, R);
}

}  // namespace calib
}  // namespace mk
