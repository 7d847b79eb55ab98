// What belongs to the intrinsic block of the line solver (mk_linecal.h; the
// intrinsic calibration, mantis_calibrate_intrinsics, include/mantis.h, is the
// problem with that block alone): the eight intrinsics (fx, fy, cx, cy,
// k1..k4) of a camera as unknowns, the atan both builds share, the
// observation's Jacobian J_int and the parameters' update with its DIVERGED
// test. Shared by the device (linecal_impl.hip) and the host build of the CPU
// tests (hostcheck.cpp, tools/*calibcheck_main.cpp). Both builds keep
// -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "mk_calib.h"

namespace mk {
namespace icalib {

constexpr int kMaxCams = refine::kMaxCams;
constexpr int kMaxViews = calib::kMaxViews;
constexpr int kP = 8;  // intrinsics of a camera: fx, fy, cx, cy, k1..k4

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

}  // namespace icalib
}  // namespace mk
