// Monte Carlo localization (mantis_mcl_*, include/mantis.h): the rules of the
// persistent rig particle filter that are not scoring -- the raw draw, the
// likelihood weights in fixed point, the integer scan, the ancestor rule of
// systematic resampling, and the weighted SE(3) mean and covariance -- shared
// by the device (k_mcl_weight / k_mcl_resample, mcl_impl.hip) and the host
// build of the CPU tests (hostcheck.cpp hc_mcl_*, tools/mclcheck_main.cpp).
// The pooled error, the particle's pose and the camera pose are mk_track.h's.
//
// The weights are integers q_j = floor(exp(L_j - Lmax) * 2^40), so their sum S
// and the inclusive cumulative sums c_j are exact whatever order a scan adds
// them in, and the ancestor rule compares integer products: a parallel scan
// and a sequential one give the same ancestors, bit for bit.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "mk_track.h"

namespace mk {
namespace mcl {

constexpr int kMaxParticles = 4096;  // mantis_mcl_params.n_particles
constexpr int kQBits = 40;           // q of the heaviest particle = 2^40; S <= 2^52

// one raw 32-bit output of cv::RNG (RNG::next): the new state, whose low word is the draw
MK_HD uint64_t rng_next(uint64_t s) { return (uint64_t)(uint32_t)s * 4164903690ULL + (s >> 32); }

// a particle takes part in the step's weighting: some landmark was scored and
// at least min_projections of them over the rig
MK_HD bool valid(double E, int32_t n, int32_t min_projections) { return E != DBL_MAX && n >= min_projections; }

// L <- L - E / tau, -inf for a particle that is not valid
MK_HD double log_weight(double L, double E, int32_t n, int32_t min_projections, double tau) {
  return valid(E, n, min_projections) ? L - E / tau : -INFINITY;
}

// q = floor(exp(L - Lmax) * 2^40); L = -inf gives 0, L = Lmax gives 2^40 exactly
MK_HD uint64_t weight_q(double L, double Lmax) {
  if (!(L > -INFINITY)) return 0;
  return (uint64_t)floor(exp(L - Lmax) * (double)(1ULL << kQBits));
}

// 64 x 64 -> 128 bit product and the comparison of two of them
struct U128 {
  uint64_t hi, lo;
};
MK_HD U128 mul64(uint64_t a, uint64_t b) {
  const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
  const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
  U128 r;
  r.lo = (uint64_t)(uint32_t)p00 | (mid << 32);
  r.hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
  return r;
}
MK_HD bool gt128(const U128& a, const U128& b) { return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo); }

// c * N * 2^32 > (U + i * 2^32) * S, exactly (c, S <= 2^52, N <= 2^12: c * N
// <= 2^64 needs the 128-bit product before the shift; i < N, U < 2^32)
MK_HD bool past(uint64_t c, int N, uint32_t U, int i, uint64_t S) {
  U128 l = mul64(c, (uint64_t)N);
  l.hi = (l.hi << 32) | (l.lo >> 32);
  l.lo <<= 32;
  return gt128(l, mul64((uint64_t)U + ((uint64_t)i << 32), S));
}

// Ancestor of new particle i in systematic resampling with the one draw U:
// the first j with c_j N 2^32 > (U + i 2^32) S (cum = the inclusive sums c_j,
// S = c_{N-1} > 0), clamped to `last` = the last particle with q > 0.
// c is non-decreasing, so the first such j is found by bisection.
MK_HD int ancestor(const uint64_t* cum, int N, uint32_t U, int i, int last) {
  const uint64_t S = cum[N - 1];
  int lo = 0, hi = N - 1;  // the answer is in [lo, hi]: c_{N-1} N 2^32 = S N 2^32 > (U + i 2^32) S
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (past(cum[m], N, U, i, S)) hi = m;
    else lo = m + 1;
  }
  return lo < last ? lo : last;
}

// (weight, index) order of `best`: the heaviest particle, the first on ties
MK_HD bool heavier(uint64_t q, int j, uint64_t bq, int bj) { return q > bq || (q == bq && j < bj); }

// quaternion of R with a non-negative dot with `ref` (q and -q are one rotation)
MK_HD Quat quat_toward(const double* R, const Quat& ref) {
  Quat q = basis_to_quat(R);
  if (q.x * ref.x + q.y * ref.y + q.z * ref.z + q.w * ref.w < 0) {
    q.x = -q.x; q.y = -q.y; q.z = -q.z; q.w = -q.w;
  }
  return q;
}

// The mean's first moments about particle `best`, one particle's terms (w =
// q_j / S): m7 += w [t_j - t_best ; q_j - q_best]. The means are then t_best +
// m[0..3) and q_best + m[3..7) (sum of w = 1), so particles that all equal
// `best` have the mean `best` exactly.
MK_HD void mean_terms(const Xf& T, const Xf& Tb, const Quat& qb, double w, double* m7) {
  const Quat q = quat_toward(T.R, qb);
  m7[0] = w * (T.t[0] - Tb.t[0]);
  m7[1] = w * (T.t[1] - Tb.t[1]);
  m7[2] = w * (T.t[2] - Tb.t[2]);
  m7[3] = w * (q.x - qb.x);
  m7[4] = w * (q.y - qb.y);
  m7[5] = w * (q.z - qb.z);
  m7[6] = w * (q.w - qb.w);
}

// The estimate from the reduced moments: t = t_best + m[0..3); the rotation
// of the quaternion sum qs = q_best + m[3..7) (basis_from_quat normalises), or
// best's own basis when that sum's norm is < 1e-12 or `single` (one particle
// carries all the weight: it is the estimate, bit for bit). *qs_out = the sum.
MK_HD Xf mean_pose(const Xf& Tb, const Quat& qb, const double* m7, bool single, Quat* qs_out) {
  Xf o;
  Quat qs;
  qs.x = qb.x + m7[3]; qs.y = qb.y + m7[4]; qs.z = qb.z + m7[5]; qs.w = qb.w + m7[6];
  const double nn = sqrt(qs.x * qs.x + qs.y * qs.y + qs.z * qs.z + qs.w * qs.w);
  if (single || !(nn >= 1e-12)) {
    qs = qb;
    for (int k = 0; k < 9; k++) o.R[k] = Tb.R[k];
  } else {
    basis_from_quat(qs, o.R);
  }
  for (int k = 0; k < 3; k++) o.t[k] = Tb.t[k] + m7[k];
  *qs_out = qs;
  return o;
}

// xi = [t_j - t_mean ; log(R_mean^T R_j)]: translation in the world frame,
// rotation as the right perturbation of the mean. The rotation vector is taken
// from the relative quaternion conj(qs) * q_j (qs = the mean's quaternion, any
// norm): its vector part is written so that q_j = qs gives exactly 0.
MK_HD void xi_of(const Xf& T, const Xf& Tm, const Quat& qs, double* xi) {
  for (int k = 0; k < 3; k++) xi[k] = T.t[k] - Tm.t[k];
  const Quat b = quat_toward(T.R, qs);
  const Quat& a = qs;
  const double w = a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z;  // >= 0
  const double vx = (a.w * b.x - b.w * a.x) - (a.y * b.z - a.z * b.y);
  const double vy = (a.w * b.y - b.w * a.y) - (a.z * b.x - a.x * b.z);
  const double vz = (a.w * b.z - b.w * a.z) - (a.x * b.y - a.y * b.x);
  const double n = sqrt(vx * vx + vy * vy + vz * vz);
  const double k = n > 0 ? 2.0 * atan2(n, w) / n : 0.0;
  xi[3] = vx * k; xi[4] = vy * k; xi[5] = vz * k;
}

// the 21 upper-triangle terms w xi xi^T, row by row ((0,0) .. (0,5), (1,1) ..)
MK_HD void cov_terms(const double* xi, double w, double* c21) {
  int k = 0;
  for (int r = 0; r < 6; r++)
    for (int c = r; c < 6; c++) c21[k++] = w * (xi[r] * xi[c]);
}
MK_HD void cov_expand(const double* c21, double* cov36) {
  int k = 0;
  for (int r = 0; r < 6; r++)
    for (int c = r; c < 6; c++) cov36[r * 6 + c] = cov36[c * 6 + r] = c21[k++];
}

// What one step decides, as the device's result record carries it
struct Outcome {
  int32_t lost, resampled, n_valid, best;
  uint64_t S;
  double ess, best_error;
  Xf mean;
  double cov[36];
};

// One step's bookkeeping after scoring, sequentially (the host form of
// k_mcl_weight + k_mcl_resample): sums / counts N x C, T the predicted poses
// (in / out: gathered by ancestor when resampled), L in / out, and per
// particle q, cum and anc (-1 each when not resampled). Lnew (nullable): the
// log-weights before any reset. Lost (no particle with a finite log-weight):
// L and T stay, q = cum = 0.
inline Outcome step_seq(const long long* sums, const int32_t* counts, int N, int C, Xf* T, double* L, double tau,
                        double resample_frac, int32_t min_projections, uint32_t U, uint64_t* q, uint64_t* cum,
                        int32_t* anc, double* E_out, double* Lnew_out) {
  Outcome o{};
  o.best = -1;
  o.best_error = DBL_MAX;
  double* Ln = new double[N];
  double* E = new double[N];
  double Lmax = -INFINITY;
  for (int j = 0; j < N; j++) {
    int32_t n;
    E[j] = track::pool(sums + (size_t)j * C, counts + (size_t)j * C, C, &n);
    Ln[j] = log_weight(L[j], E[j], n, min_projections, tau);
    if (Ln[j] > Lmax) Lmax = Ln[j];
    anc[j] = -1;
    q[j] = cum[j] = 0;
    if (E_out) E_out[j] = E[j];
    if (Lnew_out) Lnew_out[j] = Ln[j];
  }
  if (!(Lmax > -INFINITY)) {
    o.lost = 1;
    delete[] Ln;
    delete[] E;
    return o;
  }
  uint64_t S = 0, bq = 0;
  int bj = 0x7fffffff, last = 0;
  double q2 = 0;
  for (int j = 0; j < N; j++) {
    q[j] = weight_q(Ln[j], Lmax);
    S += q[j];
    cum[j] = S;
    q2 += (double)q[j] * (double)q[j];
    if (q[j] > 0) { o.n_valid++; last = j; }
    if (heavier(q[j], j, bq, bj)) { bq = q[j]; bj = j; }
  }
  o.S = S;
  o.best = bj;
  o.best_error = E[bj];
  o.ess = (double)S * (double)S / q2;
  const Xf Tb = T[bj];
  const Quat qb = basis_to_quat(Tb.R);
  double m7[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int j = 0; j < N; j++) {
    if (!q[j]) continue;
    double t7[7];
    mean_terms(T[j], Tb, qb, (double)q[j] / (double)S, t7);
    for (int k = 0; k < 7; k++) m7[k] += t7[k];
  }
  Quat qs;
  o.mean = mean_pose(Tb, qb, m7, o.n_valid == 1, &qs);
  double c21[21];
  for (int k = 0; k < 21; k++) c21[k] = 0;
  for (int j = 0; j < N; j++) {
    if (!q[j]) continue;
    double xi[6], t21[21];
    xi_of(T[j], o.mean, qs, xi);
    cov_terms(xi, (double)q[j] / (double)S, t21);
    for (int k = 0; k < 21; k++) c21[k] += t21[k];
  }
  cov_expand(c21, o.cov);
  if (o.ess < resample_frac * (double)N) {
    o.resampled = 1;
    Xf* old = new Xf[N];
    for (int j = 0; j < N; j++) old[j] = T[j];
    for (int i = 0; i < N; i++) {
      anc[i] = ancestor(cum, N, U, i, last);
      T[i] = old[anc[i]];
      L[i] = 0;
    }
    delete[] old;
  } else {
    for (int j = 0; j < N; j++) L[j] = Ln[j];
  }
  delete[] Ln;
  delete[] E;
  return o;
}

}  // namespace mcl
}  // namespace mk
