// Rig tracking (mantis_track / mantis_track_batch, include/mantis.h): the
// rules of the joint multi-camera particle filter that are not scoring --
// the pooled error of a base pose over the rig's cameras, the particle choice
// of one iteration, the particle's pose and the gate -- shared by the device
// (k_track_particles, track_impl.hip) and the host build of the CPU tests
// (hostcheck.cpp hc_track_*, tools/trackcheck_main.cpp).
//
// Reference: optimizeHypothesisWithParticleFilter (PoseAdjustment.h:13-60)
// seeded from a motion prediction; its particles are base poses T_w_b and
// each is scored on every camera c with c2w_c = inverse(T_w_b * T_base_cam_c),
// the cameras' exact integer (sum, n) of the fast WHITE evaluator
// (HypothesisEvaluation.h:107-158, 218-227) pooled before the division.
#pragma once
#include <cfloat>
#include <cstdint>

#include "mk_math.h"

namespace mk {
namespace track {

constexpr int kMaxParticles = 96;   // mantis_track_params.particles
constexpr int kMaxIterations = 10;  // mantis_track_params.iterations (iter_err[11], iter_pick[10])
constexpr int kMaxCams = 8;         // cameras per rig
constexpr int kMaxTasks = 512;      // particles x cameras per rig

// The fast evaluator's error of an integer (sum, n): every scorer's rule
// (HypothesisEvaluation.h:218-227), DBL_MAX when no landmark was seen.
MK_HD double error_of(long long sum, int32_t n) { return n <= 0 ? DBL_MAX : (double)sum / ((double)n * 1.1); }

// E = error_of(sum(sum_c), sum(n_c)): the cameras' sums pooled before the
// division; *n_out = sum(n_c). sums / counts: one entry per camera.
MK_HD double pool(const long long* sums, const int32_t* counts, int n_cams, int32_t* n_out) {
  long long s = 0;
  int32_t n = 0;
  for (int c = 0; c < n_cams; c++) {
    s += sums[c];
    n += counts[c];
  }
  *n_out = n;
  return error_of(s, n);
}

// the argmin's order: by (error, particle index)
MK_HD bool before(double e, int j, double be, int bj) { return e < be || (e == be && j < bj); }

// One iteration's choice: the first strict minimum of err[0 .. n), taken only
// when it is strictly below the current error; -1 = the current pose stays.
MK_HD int pick(const double* err, int n, double cur_err) {
  double be = DBL_MAX;
  int bj = 0x7fffffff;
  for (int j = 0; j < n; j++)
    if (before(err[j], j, be, bj)) { be = err[j]; bj = j; }
  return bj < n && be < cur_err ? bj : -1;
}

// tracked: some landmark was scored, at least min_projections of them over
// the rig (MonteCarlo.cpp:220's count gate), and the error within max_error
// (<= 0: no error gate)
MK_HD int gate(double error, int32_t n_proj, int32_t min_projections, double max_error) {
  return error != DBL_MAX && n_proj >= min_projections && (max_error <= 0 || error <= max_error) ? 1 : 0;
}

// Particle = cur * rand, rand = Transform(setRPY(roll, pitch, yaw), (x, y, z))
// from six gaussians drawn yaw, pitch, roll, z, y, x (PoseAdjustment.h:13-23,
// pf_particle's rule with the call's sigmas): the perturbation is applied on
// the right, in the base frame. |g6 * sigma_rot| < 2^30 (basis_from_rpy_small).
MK_HD Xf particle(const Xf& cur, const float* g6, double sigma_rot, double sigma_t) {
  const double yaw = (double)g6[0] * sigma_rot, pitch = (double)g6[1] * sigma_rot, roll = (double)g6[2] * sigma_rot;
  const double tz = (double)g6[3] * sigma_t, ty = (double)g6[4] * sigma_t, tx = (double)g6[5] * sigma_t;
  Xf rnd;
  basis_from_rpy_small(roll, pitch, yaw, rnd.R);
  rnd.t[0] = tx; rnd.t[1] = ty; rnd.t[2] = tz;
  return xf_mul(cur, rnd);
}

// world -> camera of base pose T_w_b in the camera with extrinsics T_base_cam
MK_HD Xf cam_c2w(const Xf& T_w_b, const Xf& T_base_cam) { return xf_inverse(xf_mul(T_w_b, T_base_cam)); }

// row-major 4x4 <-> Xf
MK_HD Xf xf_from_mat4(const double* T) {
  Xf o;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) o.R[i * 3 + j] = T[i * 4 + j];
    o.t[i] = T[i * 4 + 3];
  }
  return o;
}
MK_HD void xf_to_mat4(const Xf& a, double* T) {
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) T[i * 4 + j] = a.R[i * 3 + j];
    T[i * 4 + 3] = a.t[i];
  }
  T[12] = T[13] = T[14] = 0.0;
  T[15] = 1.0;
}

}  // namespace track
}  // namespace mk
