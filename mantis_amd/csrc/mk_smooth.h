// Window smoothing (mantis_smooth_batch, include/mantis.h): the line rows of N
// consecutive views of one rig joined by between-pose factors from the
// service's motions (and an optional prior on view 0) in one block-tridiagonal
// Gauss-Newton. The rows are the refinement's (mk_refine.h); new here are
// log_so3 / J_r^-1, the between and prior factors with their Jacobians for the
// right perturbation of calib::right_update, the assembly of the 6 x 6 blocks,
// the block Cholesky with its substitutions, the window's figures and gates,
// (host) the marginal covariances, and for the fixed-lag window (mantis_lag_*,
// lag_impl.hip) the marginal of the leaving view, the whitener of the prior it
// leaves and the predicted start. Shared by the device (k_smooth_acc /
// k_smooth_solve, smooth_impl.hip; k_lag_slide, lag_impl.hip) and the host
// build of the CPU tests (hostcheck.cpp hc_smooth_* / hc_lag_*,
// tools/smoothcheck_main.cpp, tools/lagcheck_main.cpp). Both builds keep
// -ffp-contract=off, and every sum here runs in a stated order.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "mk_calib.h"
#include "mk_track.h"

namespace mk {
namespace smooth {

constexpr int kMaxViews = calib::kMaxViews;
constexpr int kMaxIterations = refine::kMaxIterations;
constexpr int kOk = refine::kOk, kStarved = refine::kStarved, kSingular = refine::kSingular;

// what a pass needs of mantis_smooth_params
struct Weights {
  double wt, wr;     // sigma_row / sigma_t, sigma_row / sigma_rot
  double sigma_row;  // motion_rms is in units of it
  double lambda;
};

// R (3 x 3) and t of a row-major 4 x 4
MK_HD void rt_of(const double* T, double* R, double* t) {
  for (int a = 0; a < 3; a++) {
    for (int b = 0; b < 3; b++) R[3 * a + b] = T[4 * a + b];
    t[a] = T[4 * a + 3];
  }
}
// A^T B and A^T v of 3 x 3 row-major, sums in ascending index order
MK_HD void mul_tn(const double* A, const double* B, double* o) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) o[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
MK_HD void mul_tv(const double* A, const double* v, double* o) {
  for (int i = 0; i < 3; i++) o[i] = A[i] * v[0] + A[3 + i] * v[1] + A[6 + i] * v[2];
}
MK_HD void mul_nn(const double* A, const double* B, double* o) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) o[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
MK_HD void skew(const double* v, double* K) {
  K[0] = 0; K[1] = -v[2]; K[2] = v[1];
  K[3] = v[2]; K[4] = 0; K[5] = -v[0];
  K[6] = -v[1]; K[7] = v[0]; K[8] = 0;
}

// The rotation vector of R. v = vee(R - R^T) / 2 has |v| = sin(theta) and
// c = (tr R - 1) / 2 = cos(theta): at small angles theta = atan2(|v|, c) keeps
// its digits, where acos(c) loses them. phi = (theta / sin theta) v; below
// sin(theta) = 1e-8 at c > 0 the factor is 1. Near pi (c < 0, sin(theta) <
// 1e-6) v vanishes and the axis comes from the largest column of R + I; from
// there down to about 1e-3 short of pi the direction of v still carries a
// relative error near 1e-16 / sin(theta), up to about 1e-10, which the
// residuals of odometry steps, far from a half turn, never meet.
MK_HD void log_so3(const double* R, double* phi) {
  const double v[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
  const double s = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
  if (c < 0 && s < 1e-6) {
    int m = 0;
    if (R[4] > R[0]) m = 1;
    if (R[8] > R[4 * m]) m = 2;
    double a[3] = {R[m] + (m == 0 ? 1.0 : 0.0), R[3 + m] + (m == 1 ? 1.0 : 0.0), R[6 + m] + (m == 2 ? 1.0 : 0.0)};
    const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const double th = atan2(s, c);
    const double sg = (v[0] * a[0] + v[1] * a[1] + v[2] * a[2]) < 0 ? -1.0 : 1.0;
    for (int i = 0; i < 3; i++) phi[i] = n > 0 ? sg * th * (a[i] / n) : 0.0;
    return;
  }
  const double f = s < 1e-8 ? 1.0 : atan2(s, c) / s;
  for (int i = 0; i < 3; i++) phi[i] = f * v[i];
}

// J_r^-1(phi) = I + [phi]x / 2 + k [phi]x^2, k = 1 / theta^2 - (1 + cos theta) / (2 theta sin theta),
// k = 1 / 12 below theta = 1e-8
MK_HD void jr_inv(const double* phi, double* J) {
  const double th2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
  const double th = sqrt(th2);
  const double k = th < 1e-8 ? 1.0 / 12.0 : 1.0 / th2 - (1.0 + cos(th)) / (2.0 * th * sin(th));
  double K[9], K2[9];
  skew(phi, K);
  mul_nn(K, K, K2);
  for (int e = 0; e < 9; e++) J[e] = (e % 4 == 0 ? 1.0 : 0.0) + 0.5 * K[e] + k * K2[e];
}

// The between factor of step k -> k + 1 with the motion's Transform D:
// M = T_k^-1 T_k+1, E = D^-1 M, e = [t_E ; log R_E], whitened by wt (rows
// 0..2) and wr (rows 3..5). Ja = de/dx_k, Jb = de/dx_k+1 (6 x 6 row-major).
MK_HD void between(const double* Tk, const double* Tk1, const double* D, double wt, double wr, double* e, double* Ja,
                   double* Jb) {
  double Rk[9], tk[3], Rn[9], tn[3], Rd[9], td[3];
  rt_of(Tk, Rk, tk);
  rt_of(Tk1, Rn, tn);
  rt_of(D, Rd, td);
  double RM[9], tM[3], RE[9], tE[3];
  mul_tn(Rk, Rn, RM);
  const double dt[3] = {tn[0] - tk[0], tn[1] - tk[1], tn[2] - tk[2]};
  mul_tv(Rk, dt, tM);
  mul_tn(Rd, RM, RE);
  const double dm[3] = {tM[0] - td[0], tM[1] - td[1], tM[2] - td[2]};
  mul_tv(Rd, dm, tE);
  double phi[3], Ji[9];
  log_so3(RE, phi);
  jr_inv(phi, Ji);
  double Kx[9], RdK[9], RMt[9], JR[9];
  skew(tM, Kx);
  mul_tn(Rd, Kx, RdK);  // R_D^T [t_M]x
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) RMt[3 * i + j] = RM[3 * j + i];
  mul_nn(Ji, RMt, JR);  // J_r^-1 R_M^T
  for (int i = 0; i < 36; i++) Ja[i] = Jb[i] = 0.0;
  for (int i = 0; i < 3; i++) {
    e[i] = wt * tE[i];
    e[3 + i] = wr * phi[i];
    for (int j = 0; j < 3; j++) {
      Jb[6 * i + j] = wt * RE[3 * i + j];
      Jb[6 * (3 + i) + 3 + j] = wr * Ji[3 * i + j];
      Ja[6 * i + j] = wt * -Rd[3 * j + i];
      Ja[6 * i + 3 + j] = wt * RdK[3 * i + j];
      Ja[6 * (3 + i) + 3 + j] = wr * -JR[3 * i + j];
    }
  }
}

// The prior factor on view 0: e = [t_0 - t_p ; log(R_p^T R_0)], J = diag(R_0,
// J_r^-1), both whitened by Wp = sigma_row L_c^-1 (6 x 6 row-major, lower).
MK_HD void prior(const double* T0, const double* Tp, const double* Wp, double* e, double* J) {
  double R0[9], t0[3], Rp[9], tp[3], RE[9], phi[3], Ji[9], r[6], Jr[36];
  rt_of(T0, R0, t0);
  rt_of(Tp, Rp, tp);
  mul_tn(Rp, R0, RE);
  log_so3(RE, phi);
  jr_inv(phi, Ji);
  for (int i = 0; i < 36; i++) Jr[i] = 0.0;
  for (int i = 0; i < 3; i++) {
    r[i] = t0[i] - tp[i];
    r[3 + i] = phi[i];
    for (int j = 0; j < 3; j++) {
      Jr[6 * i + j] = R0[3 * i + j];
      Jr[6 * (3 + i) + 3 + j] = Ji[3 * i + j];
    }
  }
  for (int i = 0; i < 6; i++) {
    double s = 0;
    for (int m = 0; m < 6; m++) s += Wp[6 * i + m] * r[m];
    e[i] = s;
    for (int j = 0; j < 6; j++) {
      double q = 0;
      for (int m = 0; m < 6; m++) q += Wp[6 * i + m] * Jr[6 * m + j];
      J[6 * i + j] = q;
    }
  }
}

// Wp = sigma_row L_c^-1 of a covariance (36, row-major), Cov = L_c L_c^T by
// chol6. False when the covariance is not finite or not positive definite. The
// host forms the whitener of a caller's prior with it, the device (k_lag_slide)
// that of a marginalised one: the same operations, the same bytes.
MK_HD bool prior_whitener(const double* cov, double sigma_row, double* Wp) {
  for (int e = 0; e < 36; e++)
    if (!std::isfinite(cov[e])) return false;
  double L[36];
  if (!calib::chol6(cov, L)) return false;
  for (int c = 0; c < 6; c++)  // column c of L^-1 by forward substitution
    for (int i = 0; i < 6; i++) {
      double s = i == c ? 1.0 : 0.0;
      for (int k = 0; k < i; k++) s -= L[6 * i + k] * Wp[6 * k + c];
      Wp[6 * i + c] = s / L[6 * i + i];
    }
  for (int e = 0; e < 36; e++) {
    Wp[e] *= sigma_row;
    if (!std::isfinite(Wp[e])) return false;
  }
  return true;
}

// ---- The fixed-lag window (mantis_lag_push): view 0 leaves as a prior on view 1 ----
// Why a prior is, or is not, carried into a window (mantis_lag_info.drop_reason)
constexpr int kLagKept = 0;      // a prior is carried, or none was due (the window was not full)
constexpr int kLagNoFactor = 1;  // step 0 had no factor: the chain is broken there
constexpr int kLagNotOk = 2;     // the last push did not end OK
constexpr int kLagH00 = 3;       // H_00 is not positive definite
constexpr int kLagLambda = 4;    // the Schur complement is not positive definite
constexpr int kLagCov = 5;       // Cov_p is not finite or not positive definite

// The marginal of view 0 on view 1, from the final pass's blocks of a window
// that ended OK (lambda = 0): H00 / g0 as assembled (A_0 + Ja^T Ja + the
// prior's term; b_0 + Ja^T e + the prior's), factor 0's whitened Ja, Jb, e and
// view 1's final pose T1.
//   B = Jb^T Ja, L0 = chol6(H00), Y = L0^-1 B^T, z = L0^-1 g0   (two triangular solves)
//   Lambda = Jb^T Jb - Y^T Y,  eta = Jb^T e - Y^T z
//   x* = -Lambda^-1 eta (chol6),  T_p = T1 D(x*) (calib::right_update)
//   Cov_p = sigma_row^2 Lambda^-1 = sigma_row^2 L^-T L^-1, its translation and
//   cross blocks turned to the world frame by R of T_p (B C B^T, B = diag(R_p,
//   I), as conclude turns its covariances).
// Every dot product runs in ascending index order; Lambda and Cov_p are formed
// as upper triangles and mirrored, so both are symmetric bit for bit. (T_p,
// Cov_p) has the shape and frames of mantis_smooth_batch's prior_T / prior_cov.
// This is a first-order marginal at the leaving view's final linearisation
// point: view 1 keeps being relinearised afterwards, and no first-estimate
// Jacobians are kept for it.
// schur0: Lambda (36) and eta (6); kLagKept or kLagH00.
MK_HD int schur0(const double* H00, const double* g0, const double* Ja, const double* Jb, const double* e, double* Lam,
                 double* eta) {
  double L0[36], B[36], Y[36], z[6];
  if (!calib::chol6(H00, L0)) return kLagH00;
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double s = 0;
      for (int r = 0; r < 6; r++) s += Jb[6 * r + i] * Ja[6 * r + j];
      B[6 * i + j] = s;
    }
  for (int c = 0; c < 6; c++)  // column c of Y: L0 Y = B^T
    for (int i = 0; i < 6; i++) {
      double s = B[6 * c + i];
      for (int k = 0; k < i; k++) s -= L0[6 * i + k] * Y[6 * k + c];
      Y[6 * i + c] = s / L0[6 * i + i];
    }
  for (int i = 0; i < 6; i++) {
    double s = g0[i];
    for (int k = 0; k < i; k++) s -= L0[6 * i + k] * z[k];
    z[i] = s / L0[6 * i + i];
  }
  for (int i = 0; i < 6; i++) {
    for (int j = i; j < 6; j++) {
      double s = 0;
      for (int r = 0; r < 6; r++) s += Jb[6 * r + i] * Jb[6 * r + j];
      for (int m = 0; m < 6; m++) s -= Y[6 * m + i] * Y[6 * m + j];
      Lam[6 * i + j] = Lam[6 * j + i] = s;
    }
    double s = 0;
    for (int r = 0; r < 6; r++) s += Jb[6 * r + i] * e[r];
    for (int m = 0; m < 6; m++) s -= Y[6 * m + i] * z[m];
    eta[i] = s;
  }
  return kLagKept;
}
// marginalize: (T_p, Cov_p); kLagKept, or the reason for no prior (Tp / Cov are then not to be used; whether
// Cov_p is finite and positive definite is prior_whitener's verdict, in marginal_prior).
MK_HD int marginalize(const double* H00, const double* g0, const double* Ja, const double* Jb, const double* e,
                      const double* T1, double sigma_row, double* Tp, double* Cov) {
  double Lam[36], eta[6], L[36], Li[36], x[6], S[36];
  if (schur0(H00, g0, Ja, Jb, e, Lam, eta) != kLagKept) return kLagH00;
  if (!calib::chol6(Lam, L)) return kLagLambda;
  for (int i = 0; i < 6; i++) eta[i] = -eta[i];
  calib::chol6_solve(L, eta, 1, x, 1);
  for (int q = 0; q < 16; q++) Tp[q] = T1[q];
  calib::right_update(Tp, x);
  for (int c = 0; c < 6; c++)  // column c of L^-1 by forward substitution
    for (int i = 0; i < 6; i++) {
      double s = i == c ? 1.0 : 0.0;
      for (int k = 0; k < i; k++) s -= L[6 * i + k] * Li[6 * k + c];
      Li[6 * i + c] = s / L[6 * i + i];
    }
  const double s2 = sigma_row * sigma_row;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++) {
      double s = 0;
      for (int m = j; m < 6; m++) s += Li[6 * m + i] * Li[6 * m + j];  // L^-1 is lower: the terms below m = j are zeros
      S[6 * i + j] = S[6 * j + i] = s2 * s;
    }
  double R[9], t[3], M[9];
  rt_of(Tp, R, t);
  for (int i = 0; i < 3; i++)
    for (int b = 0; b < 3; b++) M[3 * i + b] = R[3 * i] * S[b] + R[3 * i + 1] * S[6 + b] + R[3 * i + 2] * S[12 + b];
  for (int i = 0; i < 3; i++) {
    for (int j = i; j < 3; j++) Cov[6 * i + j] = M[3 * i] * R[3 * j] + M[3 * i + 1] * R[3 * j + 1] + M[3 * i + 2] * R[3 * j + 2];
    for (int j = 0; j < 3; j++)
      Cov[6 * i + 3 + j] = R[3 * i] * S[3 + j] + R[3 * i + 1] * S[6 + 3 + j] + R[3 * i + 2] * S[12 + 3 + j];
    for (int j = i; j < 3; j++) Cov[6 * (3 + i) + 3 + j] = S[6 * (3 + i) + 3 + j];
  }
  for (int i = 0; i < 6; i++)
    for (int j = i + 1; j < 6; j++) Cov[6 * j + i] = Cov[6 * i + j];
  return kLagKept;
}

// The prior a slide leaves: marginalize, then the whitener of Cov_p. Wp = 0, Tp
// = I and Cov = 0 with the reason when none is carried (a zero whitener adds
// exact zeros to H_00, g_0 and the cost).
MK_HD int marginal_prior(const double* H00, const double* g0, const double* Ja, const double* Jb, const double* e,
                         const double* T1, double sigma_row, double* Tp, double* Cov, double* Wp) {
  int why = marginalize(H00, g0, Ja, Jb, e, T1, sigma_row, Tp, Cov);
  if (why == kLagKept) {
    bool fin = true;
    for (int q = 0; q < 16; q++) fin = fin && std::isfinite(Tp[q]);
    if (!fin || !prior_whitener(Cov, sigma_row, Wp)) why = kLagCov;
  }
  if (why != kLagKept) {
    for (int q = 0; q < 16; q++) Tp[q] = q % 5 == 0 ? 1.0 : 0.0;
    for (int q = 0; q < 36; q++) Cov[q] = Wp[q] = 0.0;
  }
  return why;
}

// The start of a pushed view when the caller gives none: T_newest Delta by
// xf_mul (mk_math.h), the product of the MCL and track predictions.
MK_HD void predict_start(const double* T_newest, const double* D, double* T) {
  track::xf_to_mat4(xf_mul(track::xf_from_mat4(T_newest), track::xf_from_mat4(D)), T);
}

// H += J^T J and g += J^T e of one 6-row factor, each entry summed over the rows in ascending order
MK_HD void add_jtj(const double* J, const double* e, double* H, double* g) {
  for (int i = 0; i < 6; i++) {
    for (int j = 0; j < 6; j++) {
      double s = 0;
      for (int m = 0; m < 6; m++) s += J[6 * m + i] * J[6 * m + j];
      H[6 * i + j] += s;
    }
    double s = 0;
    for (int m = 0; m < 6; m++) s += J[6 * m + i] * e[m];
    g[i] += s;
  }
}

// The blocks of view k: Hd = A_k + Jb^T Jb (factor k - 1) + Ja^T Ja (factor k)
// + the prior's (k = 0) + lambda I, g likewise, Ho = H_{k+1,k} = Jb^T Ja of
// factor k (zeros without one). fe / fJ: the window's (N - 1) x 6 and
// (N - 1) x 72 ([Ja | Jb]) whitened factors; has[k]: step k has one; pe / pJ:
// the prior's (has_prior).
MK_HD void assemble(int k, int N, const double* acc28, const int32_t* has, const double* fe, const double* fJ,
                    int has_prior, const double* pe, const double* pJ, double lambda, double* Hd, double* Ho,
                    double* g) {
  double h[36], gg[6];  // summed here and stored once: Hd / g may be device memory
  int m = 0;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++) h[6 * i + j] = h[6 * j + i] = acc28[m++];
  for (int i = 0; i < 6; i++) gg[i] = acc28[21 + i];
  if (k > 0 && has[k - 1]) add_jtj(fJ + 72 * (size_t)(k - 1) + 36, fe + 6 * (size_t)(k - 1), h, gg);
  if (k < N - 1 && has[k]) {
    const double *Ja = fJ + 72 * (size_t)k, *Jb = Ja + 36;
    add_jtj(Ja, fe + 6 * (size_t)k, h, gg);
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) {
        double s = 0;
        for (int r = 0; r < 6; r++) s += Jb[6 * r + i] * Ja[6 * r + j];
        Ho[6 * i + j] = s;
      }
  } else {
    for (int e = 0; e < 36; e++) Ho[e] = 0.0;
  }
  if (k == 0 && has_prior) add_jtj(pJ, pe, h, gg);
  for (int i = 0; i < 6; i++) h[6 * i + i] += lambda;
  for (int e = 0; e < 36; e++) Hd[e] = h[e];
  for (int i = 0; i < 6; i++) g[i] = gg[i];
}

// The figures of a pass (thread 0 of the device; the host): n_obs and r^T r in
// view order, then the factors' e^T e in factor order, then the prior's.
struct Sums {
  int32_t n_obs, n_factors;
  double rtr, ete, cost, rms, motion_rms;
};
MK_HD double dot6(const double* e) {
  double s = 0;
  for (int i = 0; i < 6; i++) s += e[i] * e[i];
  return s;
}
// n_obs / rtr: the views' counts and r^T r already summed in view order
MK_HD void window_sums(int N, int32_t n_obs, double rtr, const int32_t* has, const double* fe, int has_prior,
                       const double* pe, double sigma_row, Sums& S) {
  S.n_obs = n_obs;
  S.rtr = rtr;
  S.n_factors = 0;
  S.ete = 0;
  for (int k = 0; k < N - 1; k++)
    if (has[k]) {
      S.n_factors++;
      S.ete += dot6(fe + 6 * (size_t)k);
    }
  S.cost = S.rtr + S.ete;
  if (has_prior) S.cost += dot6(pe);
  S.rms = S.n_obs > 0 ? sqrt(S.rtr / (double)S.n_obs) : 0.0;
  S.motion_rms = S.n_factors > 0 ? sqrt(S.ete / (6.0 * (double)S.n_factors)) / sigma_row : 0.0;
}

// One block step of the Cholesky chain, the order both builds keep:
//   M = Hd - Lp Lp^T (Lp = L_{k,k-1}; coupled), Ld = chol6(M),
//   Lo = Ho Ld^-T (when step k has a factor), y = Ld^-1 (-g - Lp y_prev).
// Every dot product in ascending index order. False: M is not positive definite.
MK_HD bool chain_step(const double* Hd, const double* Ho, const double* g, bool coupled, const double* Lp,
                      const double* yp, bool next, double* Ld, double* Lo, double* y) {
  double M[36];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double s = Hd[6 * i + j];
      if (coupled)
        for (int m = 0; m < 6; m++) s -= Lp[6 * i + m] * Lp[6 * j + m];
      M[6 * i + j] = s;
    }
  if (!calib::chol6(M, Ld)) return false;
  for (int e = 0; e < 36; e++) Lo[e] = 0.0;
  if (next)
    for (int r = 0; r < 6; r++)
      for (int c = 0; c < 6; c++) {
        double s = Ho[6 * r + c];
        for (int m = 0; m < c; m++) s -= Lo[6 * r + m] * Ld[6 * c + m];
        Lo[6 * r + c] = s / Ld[6 * c + c];
      }
  for (int i = 0; i < 6; i++) {
    double s = -g[i];
    if (coupled)
      for (int m = 0; m < 6; m++) s -= Lp[6 * i + m] * yp[m];
    for (int m = 0; m < i; m++) s -= Ld[6 * i + m] * y[m];
    y[i] = s / Ld[6 * i + i];
  }
  return true;
}
// Back substitution of view k: Ld^T x = y - Lo^T x_next (Lo = L_{k+1,k}; coupled = step k has a factor)
MK_HD void back_step(const double* Ld, const double* Lo, const double* y, bool coupled, const double* xn, double* x) {
  for (int i = 5; i >= 0; i--) {
    double s = y[i];
    if (coupled)
      for (int m = 0; m < 6; m++) s -= Lo[6 * m + i] * xn[m];
    for (int m = i + 1; m < 6; m++) s -= Ld[6 * m + i] * x[m];
    x[i] = s / Ld[6 * i + i];
  }
}

// Host: x = -H^-1 g of the block-tridiagonal system (Hd, g per view; Ho[k] =
// H_{k+1,k}; has[k]: step k is coupled). Ld / Lo (N x 36) and x (N x 6) are
// filled. Returns -1, or the first view whose diagonal block is not PD.
inline int solve(int N, const double* Hd, const double* Ho, const double* g, const int32_t* has, double* Ld, double* Lo,
                 double* x) {
  std::vector<double> y(6 * (size_t)N);
  for (int k = 0; k < N; k++) {
    const bool coupled = k > 0 && has[k - 1], next = k < N - 1 && has[k];
    if (!chain_step(Hd + 36 * (size_t)k, Ho + 36 * (size_t)k, g + 6 * (size_t)k, coupled,
                    coupled ? Lo + 36 * (size_t)(k - 1) : nullptr, coupled ? &y[6 * (size_t)(k - 1)] : nullptr, next,
                    Ld + 36 * (size_t)k, Lo + 36 * (size_t)k, &y[6 * (size_t)k]))
      return k;
  }
  for (int k = N - 1; k >= 0; k--) {
    const bool next = k < N - 1 && has[k];
    back_step(Ld + 36 * (size_t)k, Lo + 36 * (size_t)k, &y[6 * (size_t)k], next, next ? x + 6 * (size_t)(k + 1) : nullptr,
              x + 6 * (size_t)k);
  }
  return -1;
}

// Host: the diagonal blocks S_k of H^-1 from the factor, backwards:
// S_N-1 = (L L^T)^-1, S_k = (L_kk L_kk^T)^-1 + G_k^T S_k+1 G_k, G_k = L_{k+1,k} L_kk^-1.
inline void marginals(int N, const double* Ld, const double* Lo, const int32_t* has, double* S) {
  for (int k = N - 1; k >= 0; k--) {
    const double* L = Ld + 36 * (size_t)k;
    double* Sk = S + 36 * (size_t)k;
    double id[36];
    for (int e = 0; e < 36; e++) id[e] = e % 7 == 0 ? 1.0 : 0.0;
    for (int c = 0; c < 6; c++) calib::chol6_solve(L, id + c, 6, Sk + c, 6);
    if (k < N - 1 && has[k]) {
      const double *X = Lo + 36 * (size_t)k, *Sn = S + 36 * (size_t)(k + 1);
      double G[36], SG[36];
      for (int r = 0; r < 6; r++)  // G L = X, columns from the last
        for (int c = 5; c >= 0; c--) {
          double s = X[6 * r + c];
          for (int m = c + 1; m < 6; m++) s -= G[6 * r + m] * L[6 * m + c];
          G[6 * r + c] = s / L[6 * c + c];
        }
      for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
          double s = 0;
          for (int m = 0; m < 6; m++) s += Sn[6 * i + m] * G[6 * m + j];
          SG[6 * i + j] = s;
        }
      for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
          double s = 0;
          for (int m = 0; m < 6; m++) s += G[6 * m + i] * SG[6 * m + j];
          Sk[6 * i + j] += s;
        }
    }
  }
}

// The end of pass `pass` for the window from its figures: fills the result's
// arrays; true when the window is finished before its solve (the final pass or
// STARVED).
MK_HD bool end_sums(const Sums& S, int pass, int I, int32_t min_obs, mantis_smooth_result& R) {
  R.n_obs[pass] = S.n_obs;
  R.rms[pass] = S.rms;
  R.motion_rms[pass] = S.motion_rms;
  R.cost[pass] = S.cost;
  R.n_factors = S.n_factors;
  if (pass >= I) return true;
  if (S.n_obs < min_obs) {
    R.status = kStarved;
    return true;
  }
  return false;
}

// Host: the gate and the marginal covariances from the final pass's blocks at
// lambda = 0 (Hd, Ho: N x 36) and the views' final poses. dof = n_obs + 6
// n_factors + 6 has_prior - 6 N, sigma2 = cost / dof, Cov_k = sigma2 S_k with
// the translation block turned to the world frame by R_wb,k (B S B^T, B =
// diag(R_wb, I)), as refine::conclude. Not smoothed: the covariances are zeros.
inline void conclude(int N, const double* Hd, const double* Ho, const int32_t* has, int32_t min_obs, double max_rms,
                     mantis_smooth_result& R, mantis_smooth_view* V) {
  const int fp = R.iterations_run;
  R.dof = R.n_obs[fp] + 6 * R.n_factors + 6 * R.has_prior - 6 * N;
  R.sigma2 = 0.0;
  R.smoothed = R.status == kOk && R.n_obs[fp] >= min_obs && (max_rms <= 0 || R.rms[fp] <= max_rms) && R.dof > 0;
  for (int k = 0; k < N; k++)
    for (int e = 0; e < 36; e++) V[k].covariance[e] = 0.0;
  if (!R.smoothed) return;
  std::vector<double> Ld(36 * (size_t)N), Lo(36 * (size_t)N), x(6 * (size_t)N), g(6 * (size_t)N, 0.0), S(36 * (size_t)N);
  if (solve(N, Hd, Ho, g.data(), has, Ld.data(), Lo.data(), x.data()) >= 0) {
    R.smoothed = 0;
    return;
  }
  R.sigma2 = R.cost[fp] / (double)R.dof;
  marginals(N, Ld.data(), Lo.data(), has, S.data());
  for (int k = 0; k < N; k++) {
    const double* Sk = &S[36 * (size_t)k];
    double B[6][6] = {{0}}, BC[6][6];
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) B[i][j] = V[k].T_w_b[4 * i + j];
      B[3 + i][3 + i] = 1.0;
    }
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) {
        double s = 0;
        for (int m = 0; m < 6; m++) s += B[i][m] * (R.sigma2 * Sk[6 * m + j]);
        BC[i][j] = s;
      }
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) {
        double s = 0;
        for (int m = 0; m < 6; m++) s += BC[i][m] * B[j][m];
        V[k].covariance[6 * i + j] = s;
      }
    for (int i = 0; i < 6; i++)
      for (int j = i + 1; j < 6; j++) V[k].covariance[6 * j + i] = V[k].covariance[6 * i + j];
  }
}

// Host: what a pass keeps for the tests (hc_smooth_seq's optional record)
struct PassRecord {
  std::vector<double> T, acc28, e, J, pe, pJ, delta;  // N x 16, N x 28, (N-1) x 6, (N-1) x 72, 6, 36, N x 6
  std::vector<int32_t> n_obs;
};

// Host: the whole call of one window on host frames. frames[k * C + c]: W x H,
// stride 3 W. D: (N - 1) x 16 Transforms of the set motions; has[k]: step k is
// set. Tp / Wp: the prior's pose and whitener (has_prior). Rows summed in slot
// order per view, as refine_seq.
inline void smooth_seq(int N, const double* T_in, const double* D, const int32_t* has, int has_prior, const double* Tp,
                       const double* Wp, const GnCam* gcams, const Cam* cams, const uint8_t* const* frames, int C, int W,
                       int H, const double* X, int nw, int nr, const int32_t* cand, int n_cand,
                       const mantis_smooth_params& p, mantis_smooth_result& R, mantis_smooth_view* V,
                       std::vector<PassRecord>* rec) {
  R = mantis_smooth_result{};
  R.n_cand = n_cand;
  R.n_views = N;
  R.has_prior = has_prior;
  for (int k = 0; k < N; k++) {
    V[k] = mantis_smooth_view{};
    for (int e = 0; e < 16; e++) V[k].T_w_b[e] = T_in[16 * (size_t)k + e];
  }
  const refine::Window win{p.half_window, p.white_thresh, p.min_weight, 0};
  const Weights w{p.sigma_row / p.sigma_t, p.sigma_row / p.sigma_rot, p.sigma_row, p.lambda};
  const int NF = N > 1 ? N - 1 : 1;
  std::vector<double> acc(28 * (size_t)N), fe(6 * (size_t)NF), fJ(72 * (size_t)NF), Hd(36 * (size_t)N), Ho(36 * (size_t)N),
      g(6 * (size_t)N), Ld(36 * (size_t)N), Lo(36 * (size_t)N), x(6 * (size_t)N);
  std::vector<int32_t> nobs(N);
  double pe[6] = {0}, pJ[36] = {0};
  if (rec) rec->clear();
  for (int pass = 0; pass <= p.iterations; pass++) {
    for (int k = 0; k < N; k++) {
      double Rt[9], t[3], *a = &acc[28 * (size_t)k];
      refine::pose_parts(V[k].T_w_b, Rt, t);
      for (int e = 0; e < 28; e++) a[e] = 0.0;
      int32_t n = 0;
      for (int c = 0; c < C; c++)
        for (int q = 0; q < n_cand; q++) {
          const int i = cand[q] & 0xffff, axis = cand[q] >> 16;
          int tg[3];
          refine::target_bgr(i, nw, nr, tg);
          refine::Slot o;
          refine::observe(Rt, t, gcams[c], cams[c], frames[(size_t)k * C + c], W, H, X + 3 * i, axis, tg, win, o, nullptr);
          refine::accumulate_row(o.row, a);
          n += o.code == 0;
        }
      nobs[k] = n;
      V[k].n_obs = n;
      V[k].rms = n > 0 ? sqrt(a[27] / (double)n) : 0.0;
    }
    for (int k = 0; k < N - 1; k++) {
      if (has[k]) {
        between(V[k].T_w_b, V[k + 1].T_w_b, D + 16 * (size_t)k, w.wt, w.wr, &fe[6 * (size_t)k], &fJ[72 * (size_t)k],
                &fJ[72 * (size_t)k + 36]);
      } else {
        for (int e = 0; e < 6; e++) fe[6 * (size_t)k + e] = 0.0;
        for (int e = 0; e < 72; e++) fJ[72 * (size_t)k + e] = 0.0;
      }
    }
    if (has_prior) prior(V[0].T_w_b, Tp, Wp, pe, pJ);
    const double lam = pass < p.iterations ? p.lambda : 0.0;
    for (int k = 0; k < N; k++)
      assemble(k, N, &acc[28 * (size_t)k], has, fe.data(), fJ.data(), has_prior, pe, pJ, lam, &Hd[36 * (size_t)k],
               &Ho[36 * (size_t)k], &g[6 * (size_t)k]);
    int32_t n_sum = 0;
    double rtr = 0;
    for (int k = 0; k < N; k++) {
      n_sum += nobs[k];
      rtr += acc[28 * (size_t)k + 27];
    }
    Sums S;
    window_sums(N, n_sum, rtr, has, fe.data(), has_prior, pe, w.sigma_row, S);
    if (rec) {
      PassRecord P;
      for (int k = 0; k < N; k++) P.T.insert(P.T.end(), V[k].T_w_b, V[k].T_w_b + 16);
      P.acc28 = acc;
      P.e.assign(fe.begin(), fe.begin() + 6 * (size_t)(N - 1));
      P.J.assign(fJ.begin(), fJ.begin() + 72 * (size_t)(N - 1));
      P.pe.assign(pe, pe + 6);
      P.pJ.assign(pJ, pJ + 36);
      P.delta.assign(6 * (size_t)N, 0.0);
      P.n_obs = nobs;
      rec->push_back(P);
    }
    if (end_sums(S, pass, p.iterations, p.min_obs, R)) break;
    if (solve(N, Hd.data(), Ho.data(), g.data(), has, Ld.data(), Lo.data(), x.data()) >= 0) {
      R.status = kSingular;
      break;
    }
    for (int k = 0; k < N; k++) calib::right_update(V[k].T_w_b, &x[6 * (size_t)k]);
    if (rec) rec->back().delta = x;
    R.iterations_run = pass + 1;
  }
  conclude(N, Hd.data(), Ho.data(), has, p.min_obs, p.max_rms, R, V);
}

}  // namespace smooth
}  // namespace mk
