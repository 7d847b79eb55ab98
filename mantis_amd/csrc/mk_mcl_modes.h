// Monte Carlo localization, the modes of the set (mantis_mcl_init_lattice /
// mantis_mcl_modes / mantis_mcl_select_mode, include/mantis.h): the cell key of
// a pose against the anchor, the bin table and its order, the lattice site of a
// seeded particle and the per-cell estimate, shared by the device (k_mcl_modes /
// k_mcl_keep, mcl_modes_impl.hip) and the host build of the CPU tests
// (hostcheck.cpp hc_mcl_cell_key / hc_mcl_lattice_site / hc_mcl_modes,
// tools/mclmodescheck_main.cpp). The estimate's own rules are mk_mcl.h's.
//
// The floor grid is periodic, so the set may sit in several cells of the
// lattice at once, and in the four headings a square cell cannot tell apart.
// A key is (ix, iy, k): the cell offsets and the yaw quadrant against the
// anchor, particle `best` of the last step's predicted set. FP64 division and
// floor are exact and both builds keep -ffp-contract=off: host and device give
// the same key for the same pose. The bin weights are sums of the integer q:
// exact in any order, also through atomics.
#pragma once
#include "mk_mcl.h"

namespace mk {
namespace mcl {

constexpr int kCellHalf = 7;                      // |ix|, |iy| <= 7 is in range
constexpr int kCellSide = 2 * kCellHalf + 1;      // 15
constexpr int kModeBins = kCellSide * kCellSide * 4;  // 900 in-range bins; bin 900 = outside
constexpr int kMaxModes = 8;

// floor(d / g + 0.5) as an int, saturated far outside the range that matters
MK_HD int32_t cell_index(double d, double g) {
  const double f = floor(d / g + 0.5);
  if (!(f > -1073741824.0)) return -1073741824;  // also NaN
  if (!(f < 1073741824.0)) return 1073741824;
  return (int32_t)f;
}

// yaw quadrant of T against A from the base x-axes projected on the world's xy plane
MK_HD int32_t yaw_quadrant(const Xf& T, const Xf& A) {
  const double h0 = T.R[0], h1 = T.R[3], a0 = A.R[0], a1 = A.R[3];
  const double c = h0 * a0 + h1 * a1, s = a0 * h1 - a1 * h0;
  if (fabs(c) >= fabs(s)) return c >= 0 ? 0 : 2;  // c = s = 0: 0
  return s > 0 ? 1 : 3;
}

MK_HD bool cell_in_range(int32_t ix, int32_t iy) {
  return ix >= -kCellHalf && ix <= kCellHalf && iy >= -kCellHalf && iy <= kCellHalf;
}
MK_HD int32_t cell_bin(int32_t ix, int32_t iy, int32_t k) {
  return cell_in_range(ix, iy) ? ((iy + kCellHalf) * kCellSide + (ix + kCellHalf)) * 4 + k : kModeBins;
}
// an in-range bin back to its key
MK_HD void bin_cell(int32_t bin, int32_t* ix, int32_t* iy, int32_t* k) {
  *k = bin & 3;
  *ix = (bin >> 2) % kCellSide - kCellHalf;
  *iy = (bin >> 2) / kCellSide - kCellHalf;
}

// the key of pose T against the anchor A on a grid of spacing g; returns the bin
MK_HD int32_t cell_key(const Xf& T, const Xf& A, double g, int32_t* ix, int32_t* iy, int32_t* k) {
  *ix = cell_index(T.t[0] - A.t[0], g);
  *iy = cell_index(T.t[1] - A.t[1], g);
  *k = yaw_quadrant(T, A);
  return cell_bin(*ix, *iy, *k);
}

// the heaviest particle of a bin as one integer maximum: mcl::heavier's order
// (q <= 2^40, j < 4096: 52 bits); 0 = no particle
MK_HD uint64_t heaviest_pack(uint64_t q, int j) { return (q << 12) | (uint64_t)(kMaxParticles - 1 - j); }
MK_HD int heaviest_index(uint64_t packed) { return kMaxParticles - 1 - (int)(packed & (uint64_t)(kMaxParticles - 1)); }

// the mode order as one integer maximum: W descending, then the bin index
// ascending (W <= 2^52, bin < 1024: 62 bits); 0 = an empty bin
MK_HD uint64_t mode_order_key(uint64_t W, int32_t bin) { return W ? (W << 10) | (uint64_t)(1023 - bin) : 0; }
MK_HD int32_t mode_order_bin(uint64_t key) { return 1023 - (int32_t)(key & 1023); }

// site s of a (2 cx + 1) x (2 cy + 1) lattice
MK_HD void lattice_site(int s, int cx, int cy, int32_t* ix, int32_t* iy) {
  *ix = s % (2 * cx + 1) - cx;
  *iy = s / (2 * cx + 1) - cy;
}

// What mantis_mcl_modes reports, in the layout of mantis_mcl_mode / mantis_mcl_modes
struct Mode {
  int32_t ix, iy, yaw_quadrant, n, best, pad;
  uint64_t weight;
  double share, best_error;
  double T_w_b[16], covariance[36];
};
struct Modes {
  int32_t status, n_modes, n_cells, n_outside;
  uint64_t weight_sum, outside_weight;
  double anchor_T_w_b[16];
  Mode mode[kMaxModes];
};

MK_HD void mode_clear(Mode& m) {
  m.ix = m.iy = m.yaw_quadrant = m.n = 0;
  m.best = -1;
  m.pad = 0;
  m.weight = 0;
  m.share = 0;
  m.best_error = DBL_MAX;
  for (int k = 0; k < 16; k++) m.T_w_b[k] = 0;
  for (int k = 0; k < 36; k++) m.covariance[k] = 0;
}

// The modes of a set, sequentially (the host form of k_mcl_modes): T the
// predicted poses, q their integer weights, sums / counts N x C, `best` the
// anchor's particle (-1: a lost step, no modes), g the grid spacing.
inline void modes_seq(const Xf* T, const uint64_t* q, const long long* sums, const int32_t* counts, int N, int C,
                      int best, double g, int max_modes, Modes* out) {
  Modes& o = *out;
  o.status = 0;
  o.n_modes = o.n_cells = o.n_outside = 0;
  o.weight_sum = o.outside_weight = 0;
  for (int k = 0; k < 16; k++) o.anchor_T_w_b[k] = 0;
  for (int m = 0; m < kMaxModes; m++) mode_clear(o.mode[m]);
  if (best < 0 || best >= N) return;
  const Xf A = T[best];
  track::xf_to_mat4(A, o.anchor_T_w_b);
  uint64_t* W = new uint64_t[kModeBins + 1]();
  uint64_t* pk = new uint64_t[kModeBins + 1]();
  int32_t* n = new int32_t[kModeBins + 1]();
  int32_t* bin = new int32_t[N];
  for (int j = 0; j < N; j++) {
    bin[j] = -1;
    if (!q[j]) continue;
    int32_t ix, iy, k;
    const int32_t b = bin[j] = cell_key(T[j], A, g, &ix, &iy, &k);
    W[b] += q[j];
    n[b]++;
    const uint64_t p = heaviest_pack(q[j], j);
    if (p > pk[b]) pk[b] = p;
    o.weight_sum += q[j];
  }
  o.n_outside = n[kModeBins];
  o.outside_weight = W[kModeBins];
  for (int b = 0; b < kModeBins; b++) o.n_cells += n[b] > 0;
  for (int m = 0; m < max_modes && m < kMaxModes; m++) {
    uint64_t top = 0;
    for (int b = 0; b < kModeBins; b++) {
      const uint64_t key = mode_order_key(W[b], b);
      if (key > top) top = key;
    }
    if (!top) break;
    const int32_t b = mode_order_bin(top);
    Mode& r = o.mode[m];
    bin_cell(b, &r.ix, &r.iy, &r.yaw_quadrant);
    r.n = n[b];
    r.best = heaviest_index(pk[b]);
    r.weight = W[b];
    r.share = (double)W[b] / (double)o.weight_sum;
    int32_t np;
    r.best_error = track::pool(sums + (size_t)r.best * C, counts + (size_t)r.best * C, C, &np);
    const Xf Tb = T[r.best];
    const Quat qb = basis_to_quat(Tb.R);
    double m7[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < N; j++) {
      if (bin[j] != b) continue;
      double t7[7];
      mean_terms(T[j], Tb, qb, (double)q[j] / (double)W[b], t7);
      for (int k = 0; k < 7; k++) m7[k] += t7[k];
    }
    Quat qs;
    const Xf Tm = mean_pose(Tb, qb, m7, r.n == 1, &qs);
    double c21[21];
    for (int k = 0; k < 21; k++) c21[k] = 0;
    for (int j = 0; j < N; j++) {
      if (bin[j] != b) continue;
      double xi[6], t21[21];
      xi_of(T[j], Tm, qs, xi);
      cov_terms(xi, (double)q[j] / (double)W[b], t21);
      for (int k = 0; k < 21; k++) c21[k] += t21[k];
    }
    track::xf_to_mat4(Tm, r.T_w_b);
    cov_expand(c21, r.covariance);
    W[b] = 0;  // taken
    o.n_modes++;
  }
  delete[] W;
  delete[] pk;
  delete[] n;
  delete[] bin;
}

}  // namespace mcl
}  // namespace mk
