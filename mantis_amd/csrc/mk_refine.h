// Line refinement (mantis_refine / mantis_refine_batch, include/mantis.h):
// Gauss-Newton on the grid lines from a pose prior, with no detection. From
// each landmark that lies on exactly one grid line (a candidate) the raw frame
// is sampled along the image normal of that line; the weighted centroid of the
// samples that look like the landmark's set colour is where the line really
// is, and its signed offset is a point-to-line residual for the right-
// perturbation rows of mk_gn.h. The rules here are shared by the device
// (k_refine_obs / k_refine_step, refine_impl.hip; k_refine_step_robust,
// refine_robust_impl.hip) and the host build of the CPU tests (hostcheck.cpp
// hc_refine_*, tools/refinecheck_main.cpp). Both builds keep
// -ffp-contract=off.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "mk_gn.h"

namespace mk {
namespace refine {

constexpr int kMaxCams = 8;
constexpr int kMaxIterations = 10;
constexpr int kMaxHalfWindow = 15;
// mantis_refine_result.status
constexpr int kOk = 0, kStarved = 1, kSingular = 2;
// observation codes: 0 = a row; 1 behind the camera, 2 no tangent, 3 a sample
// outside the frame, 4 the line touches the window's end, 5 too little weight
constexpr int kBehind = 1, kNoTangent = 2, kOutside = 3, kWindowEnd = 4, kWeak = 5;

// one (camera, candidate) slot: the row [J | r] (zeros unless code = 0) and the integer sums
struct Slot {
  double row[7];
  int32_t code, Sw, Skw, pad;
};

// what an observation needs of mantis_refine_params
struct Window {
  int32_t R, white_thresh, min_weight, pad;
};

// bit 0: some other landmark lies at X_i +- (pitch, 0, 0); bit 1: at X_i +- (0, pitch, 0);
// every coordinate within 1e-6
inline void line_flags(const double* X, int n, double pitch, uint8_t* flags) {
  for (int i = 0; i < n; i++) {
    uint8_t f = 0;
    for (int j = 0; j < n; j++) {
      if (j == i) continue;
      const double dx = X[3 * j] - X[3 * i], dy = X[3 * j + 1] - X[3 * i + 1], dz = X[3 * j + 2] - X[3 * i + 2];
      if (!(fabs(dz) <= 1e-6)) continue;
      if ((fabs(dx - pitch) <= 1e-6 || fabs(dx + pitch) <= 1e-6) && fabs(dy) <= 1e-6) f |= 1;
      if ((fabs(dy - pitch) <= 1e-6 || fabs(dy + pitch) <= 1e-6) && fabs(dx) <= 1e-6) f |= 2;
    }
    flags[i] = f;
  }
}
// candidates (flags exactly 1 or 2) in ascending landmark order: cand[k] = landmark | axis << 16
inline int candidates(const uint8_t* flags, int n, int32_t* cand) {
  int k = 0;
  for (int i = 0; i < n; i++)
    if (flags[i] == 1 || flags[i] == 2) {
      if (cand) cand[k] = i | ((flags[i] == 2 ? 1 : 0) << 16);
      k++;
    }
  return k;
}

// inv(T_base_cam) as the rows read it (mk_shard.h mat4_inv_rigid's expressions)
MK_HD void gncam_from(const double* Tbc, GnCam& g) {
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) g.R_cb[3 * i + j] = Tbc[4 * j + i];
    g.t_cb[i] = -(g.R_cb[3 * i] * Tbc[3] + g.R_cb[3 * i + 1] * Tbc[7] + g.R_cb[3 * i + 2] * Tbc[11]);
  }
}
// R_wb^T and t_wb of a row-major 4 x 4 (gn_accumulate_seq's)
MK_HD void pose_parts(const double* Twb, double* Rt, double* t) {
  for (int a = 0; a < 3; a++) {
    for (int b = 0; b < 3; b++) Rt[3 * a + b] = Twb[4 * b + a];
    t[a] = Twb[4 * a + 3];
  }
}

// target colour of landmark i by its set, BGR
MK_HD void target_bgr(int i, int nw, int nr, int* t) {
  if (i < nw) { t[0] = 255; t[1] = 255; t[2] = 255; }
  else if (i < nw + nr) { t[0] = 50; t[1] = 85; t[2] = 255; }
  else { t[0] = 50; t[1] = 255; t[2] = 85; }
}
MK_HD int32_t px_weight(int b, int g, int r, const int* t, int32_t thresh) {
  const int e0 = b - t[0], e1 = g - t[1], e2 = r - t[2];
  const int32_t w = thresh - (e0 * e0 + e1 * e1 + e2 * e2);
  return w > 0 ? w : 0;
}

// steps 1-3 of an observation and the Jacobian row of step 8 (it does not
// depend on the samples): the candidate's normalized image point m0, the unit
// image normal nh of its line and J = [-h | h [q]x], h = (nh^T Jpi) R_cb
struct Geom {
  double m0[2], nh[2], J[6];
};
MK_HD int geom(const double* Rwb_t, const double* twb, const GnCam& cm, const double* X, int axis, Geom& g) {
  const double d[3] = {X[0] - twb[0], X[1] - twb[1], X[2] - twb[2]};
  double q[3], p[3];
  for (int a = 0; a < 3; a++) q[a] = Rwb_t[3 * a] * d[0] + Rwb_t[3 * a + 1] * d[1] + Rwb_t[3 * a + 2] * d[2];
  for (int a = 0; a < 3; a++)
    p[a] = cm.R_cb[3 * a] * q[0] + cm.R_cb[3 * a + 1] * q[1] + cm.R_cb[3 * a + 2] * q[2] + cm.t_cb[a];
  if (!(p[2] > 0)) return kBehind;
  const double iz = 1.0 / p[2];
  g.m0[0] = p[0] * iz;
  g.m0[1] = p[1] * iz;
  const double j02 = -p[0] * iz * iz, j12 = -p[1] * iz * iz;  // Jpi = [[iz, 0, j02], [0, iz, j12]]
  // the line's direction e (world x or y) in the camera: R_cb (R_wb^T e)
  const double w[3] = {Rwb_t[axis], Rwb_t[3 + axis], Rwb_t[6 + axis]};
  double v[3];
  for (int a = 0; a < 3; a++) v[a] = cm.R_cb[3 * a] * w[0] + cm.R_cb[3 * a + 1] * w[1] + cm.R_cb[3 * a + 2] * w[2];
  const double tx = iz * v[0] + j02 * v[2], ty = iz * v[1] + j12 * v[2];
  const double tn = sqrt(tx * tx + ty * ty);
  if (!(tn >= 1e-12)) return kNoTangent;
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
  return 0;
}

// sample k of the window (step 4): its pixel, false when it is not finite or
// outside the frame. (u, v) farther than one pixel outside never round into
// the frame, so they are turned away before the conversion to int.
MK_HD bool sample_px(const Cam& cam, const Geom& g, int k, double s, int W, int H, int* x, int* y, double* uo,
                     double* vo) {
  const double a = (double)k * s;
  double u, v;
  distort(cam, g.m0[0] + a * g.nh[0], g.m0[1] + a * g.nh[1], 1.0, &u, &v);
  if (uo) { *uo = u; *vo = v; }
  if (!(u > -1.0 && u < (double)W + 1.0 && v > -1.0 && v < (double)H + 1.0)) return false;
  *x = cv_round(u);
  *y = cv_round(v);
  return *x >= 0 && *x < W && *y >= 0 && *y < H;
}

// steps 6-8 from the window's sums and its two end weights (outside = some sample failed step 4)
MK_HD void finish(int gcode, bool outside, int32_t w_lo, int32_t w_hi, int32_t Sw, int32_t Skw, int32_t min_weight,
                  double s, const Geom& g, Slot& o) {
  int code = gcode;
  if (!code && outside) code = kOutside;
  if (code) {
    Sw = 0;
    Skw = 0;
  } else if (w_lo > 0 || w_hi > 0) {
    code = kWindowEnd;
  } else if (Sw < min_weight) {
    code = kWeak;
  }
  o.code = code;
  o.Sw = Sw;
  o.Skw = Skw;
  o.pad = 0;
  if (code) {
    for (int e = 0; e < 7; e++) o.row[e] = 0.0;
  } else {
    for (int e = 0; e < 6; e++) o.row[e] = g.J[e];
    o.row[6] = -(((double)Skw / (double)Sw) * s);
  }
}

// One observation, sample by sample (the host's form; the device gives one
// lane to each sample). bgr: W x H, stride 3 W. tie (nullable): set when some
// sample coordinate is within 1e-9 of a rounding tie k + 1/2.
MK_HD void observe(const double* Rwb_t, const double* twb, const GnCam& cm, const Cam& cam, const uint8_t* bgr, int W,
                   int H, const double* X, int axis, const int* target, const Window& win, Slot& o, int* tie) {
  Geom g;
  const int gcode = geom(Rwb_t, twb, cm, X, axis, g);
  const double s = 1.0 / cam.fx;
  int32_t Sw = 0, Skw = 0, w_lo = 0, w_hi = 0;
  bool outside = false;
  if (tie) *tie = 0;
  if (!gcode) {
    int xs[2 * kMaxHalfWindow + 1], ys[2 * kMaxHalfWindow + 1];
    for (int k = -win.R; k <= win.R; k++) {
      double u, v;
      if (!sample_px(cam, g, k, s, W, H, &xs[k + win.R], &ys[k + win.R], &u, &v)) outside = true;
      if (tie && (fabs(fabs(u - floor(u)) - 0.5) <= 1e-9 || fabs(fabs(v - floor(v)) - 0.5) <= 1e-9)) *tie = 1;
    }
    if (!outside)
      for (int k = -win.R; k <= win.R; k++) {
        const uint8_t* px = bgr + 3 * ((size_t)ys[k + win.R] * W + xs[k + win.R]);
        const int32_t w = px_weight(px[0], px[1], px[2], target, win.white_thresh);
        Sw += w;
        Skw += k * w;
        if (k == -win.R) w_lo = w;
        if (k == win.R) w_hi = w;
      }
  }
  finish(gcode, outside, w_lo, w_hi, Sw, Skw, win.min_weight, s, g, o);
}

// acc28 += the 28 entries of one row, as gn_accumulate_seq lays them out
MK_HD void accumulate_row(const double* v, double* acc28) {
  int n = 0;
  for (int a = 0; a < 6; a++)
    for (int b = a; b < 6; b++) acc28[n++] += v[a] * v[b];
  for (int a = 0; a < 6; a++) acc28[21 + a] += v[a] * v[6];
  acc28[27] += v[6] * v[6];
}

// The end of pass `pass` (0 .. I; pass I is the final one and solves nothing)
// from its accumulators and its count of code-0 rows: n_obs, rms, then the
// gates and the step. Returns true when the rig is finished (the final pass,
// STARVED or SINGULAR); otherwise R.T_w_b is the next pose.
MK_HD bool end_pass(const double* acc28, int32_t n_obs, int pass, int I, int32_t min_obs, double lambda,
                    mantis_refine_result& R) {
  R.n_obs[pass] = n_obs;
  R.rms[pass] = n_obs > 0 ? sqrt(acc28[27] / (double)n_obs) : 0.0;
  if (pass >= I) return true;
  if (n_obs < min_obs) {
    R.status = kStarved;
    return true;
  }
  double T[16], d6[6];
  for (int e = 0; e < 16; e++) T[e] = R.T_w_b[e];
  if (!gn_solve6(acc28, lambda, T, d6)) {
    R.status = kSingular;
    return true;
  }
  for (int e = 0; e < 16; e++) R.T_w_b[e] = T[e];
  for (int e = 0; e < 6; e++) R.delta[pass][e] = d6[e];
  R.iterations_run = pass + 1;
  return false;
}

// ---- robust rows (mantis_refine_set_robust, include/mantis.h): the weight of
// a code-0 row from its integer key and the pass's median key. Shared by
// k_refine_step_robust (refine_robust_impl.hip) and the host (robust_pass).
constexpr int kLossNone = 0, kLossHuber = 1, kLossTukey = 2;
constexpr double kKeyUnit = 1048576.0;  // 2^20 keys per sample step

struct Robust {  // what a pass needs of mantis_refine_robust_params
  int32_t loss, pad;
  double tuning, scale_floor;
};

// floor(|Skw| 2^20 / Sw) of a code-0 slot (Sw >= 1, |Skw| <= 15 Sw: below 2^24)
MK_HD uint32_t robust_key(int32_t Sw, int32_t Skw) {
  const int64_t a = Skw < 0 ? -(int64_t)Skw : (int64_t)Skw;
  return (uint32_t)((a << 20) / (int64_t)Sw);
}
MK_HD double robust_scale(uint32_t median_key, double scale_floor) {
  const double s = 1.4826 * ((double)median_key / kKeyUnit);
  return s > scale_floor ? s : scale_floor;
}
MK_HD double robust_weight(uint32_t key, const Robust& rb, double sigma) {
  const double u = (double)key / kKeyUnit, t = u / (rb.tuning * sigma);
  if (rb.loss == kLossHuber) return t <= 1.0 ? 1.0 : 1.0 / t;
  if (rb.loss == kLossTukey) {
    const double a = 1.0 - t * t;
    return t < 1.0 ? a * a : 0.0;
  }
  return 1.0;
}
// end_pass on the weighted accumulators; n_pos = the rows with w > 0: too few of them starve the pass too
MK_HD bool end_pass_robust(const double* acc28, int32_t n_obs, int32_t n_pos, int pass, int I, int32_t min_obs,
                           double lambda, mantis_refine_result& R) {
  if (pass < I && n_obs >= min_obs && n_pos < min_obs) {
    R.n_obs[pass] = n_obs;
    R.rms[pass] = sqrt(acc28[27] / (double)n_obs);  // n_obs >= min_obs > 0
    R.status = kStarved;
    return true;
  }
  return end_pass(acc28, n_obs, pass, I, min_obs, lambda, R);
}

// Host: the robust rule over one pass's slots. keys / weights (n each): 0 in
// rejected slots; the counts and sum_w (in slot order) of the code-0 slots.
struct RobustPass {
  uint32_t median_key;
  int32_t n_obs, n_down, n_zero;
  double scale, sum_w;
};
inline uint32_t robust_median(std::vector<uint32_t>& live) {  // reorders `live`
  if (live.empty()) return 0;
  const size_t k = (live.size() - 1) / 2;
  std::nth_element(live.begin(), live.begin() + k, live.end());
  return live[k];
}
inline void robust_weights(const uint32_t* keys, const int32_t* codes, int n, const Robust& rb, double* weights,
                           RobustPass& P) {
  std::vector<uint32_t> live;
  for (int k = 0; k < n; k++)
    if (!codes || codes[k] == 0) live.push_back(keys[k]);
  P = RobustPass{};
  P.n_obs = (int32_t)live.size();
  P.median_key = robust_median(live);
  P.scale = robust_scale(P.median_key, rb.scale_floor);
  for (int k = 0; k < n; k++) {
    if (codes && codes[k] != 0) {
      weights[k] = 0.0;
      continue;
    }
    const double w = robust_weight(keys[k], rb, P.scale);
    weights[k] = w;
    P.n_down += w < 1.0;
    P.n_zero += w == 0.0;
    P.sum_w += w;
  }
}

// Host: the gate and the covariance from the last pass's accumulators.
// Cov_delta = sigma^2 (J^T J)^-1 by Cholesky, sigma^2 = r^T r / (n_obs - 6),
// its translation block turned from the base frame to the world frame
// (B Cov B^T, B = diag(R_wb, I)); order x, y, z, rot-x, rot-y, rot-z. A
// non-PD J^T J or n_obs <= 6: zeros and refined = 0.
inline void conclude(const double* acc28, int32_t min_obs, double max_rms, mantis_refine_result& R) {
  const int fp = R.iterations_run;
  const int32_t n = R.n_obs[fp];
  R.refined = R.status == kOk && n >= min_obs && (max_rms <= 0 || R.rms[fp] <= max_rms);
  for (int e = 0; e < 36; e++) R.covariance[e] = 0.0;
  double A[6][6], L[6][6] = {{0}};
  int m = 0;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++) A[i][j] = A[j][i] = acc28[m++];
  bool pd = n > 6;
  for (int i = 0; i < 6 && pd; i++)
    for (int j = 0; j <= i; j++) {
      double s = A[i][j];
      for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
      if (i == j) {
        if (!(s > 0) || !std::isfinite(s)) { pd = false; break; }
        L[i][i] = sqrt(s);
      } else {
        L[i][j] = s / L[j][j];
      }
    }
  if (!pd) {
    R.refined = 0;
    return;
  }
  const double sigma2 = acc28[27] / (double)(n - 6);
  double Cd[6][6];
  for (int c = 0; c < 6; c++) {  // column c of (L L^T)^-1
    double y[6], x[6];
    for (int i = 0; i < 6; i++) {
      double s = i == c ? 1.0 : 0.0;
      for (int k = 0; k < i; k++) s -= L[i][k] * y[k];
      y[i] = s / L[i][i];
    }
    for (int i = 5; i >= 0; i--) {
      double s = y[i];
      for (int k = i + 1; k < 6; k++) s -= L[k][i] * x[k];
      x[i] = s / L[i][i];
    }
    for (int i = 0; i < 6; i++) Cd[i][c] = sigma2 * x[i];
  }
  double B[6][6] = {{0}};
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) B[i][j] = R.T_w_b[4 * i + j];
    B[3 + i][3 + i] = 1.0;
  }
  double BC[6][6];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double s = 0;
      for (int k = 0; k < 6; k++) s += B[i][k] * Cd[k][j];
      BC[i][j] = s;
    }
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double s = 0;
      for (int k = 0; k < 6; k++) s += BC[i][k] * B[j][k];
      R.covariance[6 * i + j] = s;
    }
  for (int i = 0; i < 6; i++)  // the two triangles came from different sums: publish one
    for (int j = i + 1; j < 6; j++) R.covariance[6 * j + i] = R.covariance[6 * i + j];
}

// The whole refinement of one rig on the host, rows summed in slot order
// (slot = camera x n_cand + candidate). frames[c]: W x H, stride 3 W. slots
// (nullable): C x n_cand of the last pass taken.
inline void refine_seq(const double* T_in, const GnCam* gcams, const Cam* cams, const uint8_t* const* frames, int C,
                       int W, int H, const double* X, int nw, int nr, const int32_t* cand, int n_cand,
                       const mantis_refine_params& p, mantis_refine_result& R, Slot* slots) {
  R = mantis_refine_result{};
  R.n_cand = n_cand;
  for (int e = 0; e < 16; e++) R.T_w_b[e] = T_in[e];
  const Window win{p.half_window, p.white_thresh, p.min_weight, 0};
  double acc[28];
  for (int pass = 0; pass <= p.iterations; pass++) {
    double Rt[9], t[3];
    pose_parts(R.T_w_b, Rt, t);
    for (int e = 0; e < 28; e++) acc[e] = 0.0;
    int32_t n_obs = 0;
    for (int c = 0; c < C; c++)
      for (int k = 0; k < n_cand; k++) {
        const int i = cand[k] & 0xffff, axis = cand[k] >> 16;
        int tg[3];
        target_bgr(i, nw, nr, tg);
        Slot o;
        observe(Rt, t, gcams[c], cams[c], frames[c], W, H, X + 3 * i, axis, tg, win, o, nullptr);
        if (slots) slots[(size_t)c * n_cand + k] = o;
        accumulate_row(o.row, acc);
        n_obs += o.code == 0;
      }
    if (end_pass(acc, n_obs, pass, p.iterations, p.min_obs, p.lambda, R)) break;
  }
  conclude(acc, p.min_obs, p.max_rms, R);
}

// refine_seq with the robust rows of `rb` (loss 0: refine_seq's bytes). stats
// (nullable): the passes' figures. Per pass: all the slots, then their keys,
// the median and the weights, then sqrt(w) [J | r] summed in slot order.
inline void refine_seq_robust(const double* T_in, const GnCam* gcams, const Cam* cams, const uint8_t* const* frames,
                              int C, int W, int H, const double* X, int nw, int nr, const int32_t* cand, int n_cand,
                              const mantis_refine_params& p, const Robust& rb, mantis_refine_result& R,
                              mantis_refine_robust_stats* stats) {
  R = mantis_refine_result{};
  R.n_cand = n_cand;
  for (int e = 0; e < 16; e++) R.T_w_b[e] = T_in[e];
  if (stats) {
    *stats = mantis_refine_robust_stats{};
    stats->loss = rb.loss;
  }
  const Window win{p.half_window, p.white_thresh, p.min_weight, 0};
  const int n = C * n_cand;
  std::vector<Slot> slots(n > 0 ? n : 1);
  std::vector<uint32_t> keys(n > 0 ? n : 1);
  std::vector<int32_t> codes(n > 0 ? n : 1);
  std::vector<double> w(n > 0 ? n : 1);
  double acc[28];
  for (int pass = 0; pass <= p.iterations; pass++) {
    double Rt[9], t[3];
    pose_parts(R.T_w_b, Rt, t);
    for (int c = 0; c < C; c++)
      for (int k = 0; k < n_cand; k++) {
        const int i = cand[k] & 0xffff, axis = cand[k] >> 16;
        int tg[3];
        target_bgr(i, nw, nr, tg);
        Slot& o = slots[(size_t)c * n_cand + k];
        observe(Rt, t, gcams[c], cams[c], frames[c], W, H, X + 3 * i, axis, tg, win, o, nullptr);
        codes[(size_t)c * n_cand + k] = o.code;
        keys[(size_t)c * n_cand + k] = o.code == 0 ? robust_key(o.Sw, o.Skw) : 0;
      }
    RobustPass P;
    robust_weights(keys.data(), codes.data(), n, rb, w.data(), P);
    for (int e = 0; e < 28; e++) acc[e] = 0.0;
    for (int k = 0; k < n; k++) {
      const double sw = sqrt(w[k]);
      double v[7];
      for (int e = 0; e < 7; e++) v[e] = slots[k].row[e] * sw;
      accumulate_row(v, acc);
    }
    if (stats) {
      stats->median_key[pass] = P.median_key;
      stats->n_down[pass] = P.n_down;
      stats->n_zero[pass] = P.n_zero;
      stats->scale[pass] = P.scale;
      stats->sum_w[pass] = P.sum_w;
    }
    if (end_pass_robust(acc, P.n_obs, P.n_obs - P.n_zero, pass, p.iterations, p.min_obs, p.lambda, R)) break;
  }
  conclude(acc, p.min_obs, p.max_rms, R);
}

}  // namespace refine
}  // namespace mk
