// Monte Carlo localization, the colour evidence (mantis_mcl_set_color /
// mantis_mcl_get_color_record / mantis_mcl_modes_color, include/mantis.h): the
// COLOR sums of a (pose, camera) over the green landmarks, the pooled colour
// error of a particle, its charge and the fold of the charge into the
// log-weight, shared by the device (k_mcl_color / k_mcl_weight,
// mcl_color_impl.hip / mcl_impl.hip) and the host build of the CPU tests
// (hostcheck.cpp hc_mcl_color_*, tools/mclcolorcheck_main.cpp).
//
// Reference: computePointError(..., GREEN, fast = false)
// (HypothesisEvaluation.h:233-266): for every green landmark with z > 0 in
// frame, the 10 x 10 window of the raw frame at linear offset cvRound(v + oy)
// * W + cvRound(u + ox), o in -5..4, no bounds check (an offset outside the
// buffer reads 0, 0, 0: SURVEY Q10). The terms are kept as integers before
// the reference's division by 100: csum = the sum of the window sums, cn = the
// number of scored landmarks. Integers, so any order (and atomics) gives the
// same bits. Both builds keep -ffp-contract=off.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "mk_mcl.h"

namespace mk {
namespace mcl {

constexpr double kColorBias = 1.1;  // COLOR_PROJECTION_BIAS

// squared BGR distance of one pixel to GREEN (50, 255, 85)
MK_HD int color_px_err(int b, int g, int r) {
  const int e0 = b - 50, e1 = g - 255, e2 = r - 85;
  return e0 * e0 + e1 * e1 + e2 * e2;
}

// the window sum of a landmark projected to (u, v) on the raw BGR8 frame
// (stride 3 W): 100 pixels, at most 100 * 195075
MK_HD int32_t color_window_sum(const uint8_t* bgr, int W, int H, double u, double v) {
  const long long npx = (long long)W * H;
  int32_t s = 0;
  for (int oy = 0; oy < 10; oy++) {
    const int y = cv_round(v + (-5.0 + (double)oy));
    for (int ox = 0; ox < 10; ox++) {
      const int x = cv_round(u + (-5.0 + (double)ox));
      const long long lin = (long long)y * W + x;
      int b = 0, g = 0, r = 0;
      if (lin >= 0 && lin < npx) {
        b = bgr[3 * lin];
        g = bgr[3 * lin + 1];
        r = bgr[3 * lin + 2];
      }
      s += color_px_err(b, g, r);
    }
  }
  return s;
}

// (csum, cn) of the pose c2w (world -> camera) in camera cm over the ng green
// landmarks `green` (ng x 3, map order)
MK_HD void color_sums(const Xf& c2w, const double* green, int ng, const Cam& cm, const uint8_t* bgr, int W, int H,
                      long long* csum, int32_t* cn) {
  long long s = 0;
  int32_t n = 0;
  for (int l = 0; l < ng; l++) {
    double rp[3], u, v;
    xf_apply(c2w, green + 3 * l, rp);
    distort(cm, rp[0], rp[1], rp[2], &u, &v);
    if (!(rp[2] > 0 && in_frame(u, v, H, W))) continue;
    s += color_window_sum(bgr, W, H, u, v);
    n++;
  }
  *csum = s;
  *cn = n;
}

// Ec = (double)sum(csum_c) / ((double)sum(cn_c) * 100.0 * 1.1), defined when
// sum(cn_c) >= min_color_projections (>= 1); DBL_MAX otherwise. *n_out = sum(cn_c).
MK_HD double color_pool(const long long* csums, const int32_t* cns, int n_cams, int32_t min_color_projections,
                        int32_t* n_out) {
  long long s = 0;
  int32_t n = 0;
  for (int c = 0; c < n_cams; c++) {
    s += csums[c];
    n += cns[c];
  }
  *n_out = n;
  return n >= min_color_projections && n > 0 ? (double)s / ((double)n * 100.0 * kColorBias) : DBL_MAX;
}

// what the colour costs a particle in log-weight: Ec / color_tau, and the
// error a blind particle is deemed to have where Ec is not defined
MK_HD double color_charge(double Ec, double color_miss, double color_tau) {
  return Ec != DBL_MAX ? Ec / color_tau : color_miss / color_tau;
}

// L <- (L - E / tau) - charge, -inf for a particle that is not valid (by the
// WHITE counts alone: mcl::valid)
MK_HD double log_weight_color(double L, double E, int32_t n, int32_t min_projections, double tau, double charge) {
  return valid(E, n, min_projections) ? (L - E / tau) - charge : -INFINITY;
}

}  // namespace mcl
}  // namespace mk
