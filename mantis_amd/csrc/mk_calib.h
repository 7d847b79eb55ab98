// What belongs to the extrinsic block of the line solver (mk_linecal.h; the
// extrinsic calibration, mantis_calibrate_extrinsics, include/mantis.h, is the
// problem with that block alone): the list of free cameras, the observation's
// geometry with the extrinsic's Jacobian J_ext, the 6 x 6 Cholesky of a view's
// A_r and its solve, and the right update of a pose or an extrinsic. Shared by
// the device (linecal_impl.hip) and the host build of the CPU tests
// (hostcheck.cpp, tools/*calibcheck_main.cpp). Both builds keep
// -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "mk_refine.h"

namespace mk {
namespace calib {

constexpr int kMaxCams = refine::kMaxCams;
constexpr int kMaxViews = 256;

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

}  // namespace calib
}  // namespace mk
