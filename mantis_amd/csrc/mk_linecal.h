// The line solver behind the three calibrations (mantis_calibrate_extrinsics,
// mantis_calibrate_intrinsics, mantis_calibrate_rig, include/mantis.h): one
// joint Gauss-Newton over the base poses of N views of one rig and, per
// camera, the extrinsic of the cameras in free_ext (6 unknowns each) and the
// eight intrinsics of the cameras in free_int, on the grid lines. One
// observation is the line refinement's (mk_refine.h, steps 1-8) at the
// camera's current extrinsic and intrinsics; its row is
//   [J_pose (6) | J_ext (6, if the problem has it) | J_int (8, if it has it) | r]
// and the normal system is solved through the Schur complement of the poses.
// A problem is the pair of flags (has J_ext, has J_int); everything else --
// the row's width, the column offsets, the accumulator's size, the reduced
// system's largest size and leading dimension, the slot -- follows from it:
//
//               row                              width  kAcc  kMaxS
//   Ext  [J_pose | J_ext | r]                      13    91     42
//   Int  [J_pose | J_int | r]                      15   120     64
//   Rig  [J_pose | J_ext | J_int | r]              21   231    106
//
// What belongs to one block only stays where it was: the extrinsic's geometry,
// the 6 x 6 Cholesky and the pose update in mk_calib.h, the intrinsics'
// Jacobian, atan and update in mk_icalib.h. The working state of every call is
// mantis_rcalib_result (a field-for-field superset of the two single
// calibrations' results); narrow() / widen() at the bottom copy the fields to
// and from the public structs. The rules here are shared by the device
// (k_linecal_obs / k_linecal_rig / k_linecal_solve, linecal_impl.hip) and the
// host build of the CPU tests (hostcheck.cpp hc_*calib_*, tools/*calibcheck_
// main.cpp). Both builds keep -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "mk_icalib.h"

namespace mk {
namespace linecal {

constexpr int kMaxCams = refine::kMaxCams;
constexpr int kMaxViews = calib::kMaxViews;
constexpr int kPe = 6, kPi = icalib::kP;
constexpr int kOk = 0, kStarved = 1, kSingular = 2, kDiverged = 3;

// The reduced unknowns: the extrinsic blocks of free_ext (ascending cameras, 6
// each), then the intrinsic blocks of free_int (ascending, 8 each).
struct Layout {
  int32_t Fe, Fi, nS, pad;
  int32_t fe[kMaxCams], fi[kMaxCams];
};

// ---- robust rows (mantis_calib_set_robust, include/mantis.h): the refinement's
// key, scale and weight (refine::robust_key / _scale / _weight, not restated)
// with the median taken over every slot of the call, so one sigma per pass.
// Per (view, camera) the device's k_linecal_rig and the host keep a cell; the
// gates and the stats are formed from the cells in (view, camera) order.
struct RobustCell {
  int32_t n_down, n_zero;  // rows with w < 1, with w == 0
  double sum_w;
};
constexpr int kKindExt = 0, kKindInt = 1, kKindRig = 2;  // mantis_get_calib_robust's `kind`

// the rows with w > 0 per (view, camera): what the two extra starved gates count
MK_HD void robust_pos(const RobustCell* cells, const int32_t* cnt, int n, int32_t* pos) {
  for (int k = 0; k < n; k++) pos[k] = cnt[k] - cells[k].n_zero;
}
// The stats of pass `pass` from its cells (N x C) and counts: the pass's
// figures, and the per-view and per-camera figures of this pass (the last pass
// run leaves them). sum_w_view in camera order, sum_w_cam in view order, the
// pass's sum_w = the views' sums in view order.
MK_HD void robust_tally(const RobustCell* cells, const int32_t* cnt, int N, int C, int pass, uint32_t median_key,
                        double sigma, mantis_calib_robust_stats& st) {
  int32_t down = 0, zero = 0;
  double sw = 0.0;
  for (int c = 0; c < kMaxCams; c++) {
    st.n_zero_cam[c] = 0;
    st.sum_w_cam[c] = 0.0;
  }
  for (int r = 0; r < kMaxViews; r++) {
    st.n_obs_view[r] = st.n_zero_view[r] = 0;
    st.sum_w_view[r] = 0.0;
  }
  for (int r = 0; r < N; r++) {
    for (int c = 0; c < C; c++) {
      const RobustCell& q = cells[r * C + c];
      down += q.n_down;
      zero += q.n_zero;
      st.n_obs_view[r] += cnt[r * C + c];
      st.n_zero_view[r] += q.n_zero;
      st.sum_w_view[r] += q.sum_w;
      st.n_zero_cam[c] += q.n_zero;
      st.sum_w_cam[c] += q.sum_w;
    }
    sw += st.sum_w_view[r];
  }
  st.median_key[pass] = median_key;
  st.scale[pass] = sigma;
  st.n_down[pass] = down;
  st.n_zero[pass] = zero;
  st.sum_w[pass] = sw;
}
// Host: the rule over one pass's slots (view-major, then camera, then
// candidate). keys / weights (N C n_cand each): 0 in rejected slots; cells: N x
// C, sum_w in slot order; P: the call-wide median, sigma and counts.
inline void robust_pass(const int32_t* codes, const int32_t* Sw, const int32_t* Skw, int N, int C, int n_cand,
                        const refine::Robust& rb, uint32_t* keys, double* weights, RobustCell* cells,
                        refine::RobustPass& P) {
  const int n = N * C * n_cand;
  for (int k = 0; k < n; k++) keys[k] = codes[k] == 0 ? refine::robust_key(Sw[k], Skw[k]) : 0u;
  refine::robust_weights(keys, codes, n, rb, weights, P);
  for (int f = 0; f < N * C; f++) {
    RobustCell q{0, 0, 0.0};
    for (int k = f * n_cand; k < (f + 1) * n_cand; k++) {
      if (codes[k] != 0) continue;
      q.n_down += weights[k] < 1.0;
      q.n_zero += weights[k] == 0.0;
      q.sum_w += weights[k];
    }
    cells[f] = q;
  }
}

// ---- host: the views' elimination and the reduced system as plain loops ----
struct Reduced {
  std::vector<double> Y, Wt, S, L, Ld;  // N x 6 x kLd, N x kMaxS x kLd, kMaxS x kLd twice, kMaxS
  Layout l;
};

template <bool kE, bool kI>
struct Problem {
  static_assert(kE || kI, "a problem has J_ext, J_int or both");
  static constexpr bool kExt = kE, kInt = kI;
  static constexpr int kColE = 6, kColI = 6 + (kE ? kPe : 0);
  static constexpr int kRow = kColI + (kI ? kPi : 0) + 1;  // [J_pose | J_ext | J_int | r]
  static constexpr int kColR = kRow - 1;
  static constexpr int kAcc = kRow * (kRow + 1) / 2;       // upper triangle of a kRow x kRow
  static constexpr int kMaxS = (kE ? kPe * (kMaxCams - 1) : 0) + (kI ? kPi * kMaxCams : 0);  // unknowns of the reduced system
  static constexpr int kLd = kMaxS + 1;  // leading dimension of [E | a], Y, the Schur terms and [S | s]

  // one (view, camera, candidate) slot (row: zeros unless code = 0): 120 / 136 / 184 bytes
  struct Slot {
    double row[kRow];
    int32_t code, Sw, Skw, pad;
  };

  // index of entry (a, b), a <= b < kRow, of the upper triangle laid out row by row
  MK_HD static int tri(int a, int b) { return a * kRow - a * (a - 1) / 2 + (b - a); }
  MK_HD static int tri_sym(int a, int b) { return a <= b ? tri(a, b) : tri(b, a); }

  MK_HD static void layout(uint32_t free_ext, uint32_t free_int, int C, Layout& l) {
    for (int c = 0; c < kMaxCams; c++) l.fe[c] = l.fi[c] = 0;
    int fe[kMaxCams], fi[kMaxCams];
    l.Fe = kE ? calib::free_list(free_ext, C, fe) : 0;
    l.Fi = kI ? calib::free_list(free_int, C, fi) : 0;
    for (int f = 0; f < l.Fe; f++) l.fe[f] = fe[f];
    for (int f = 0; f < l.Fi; f++) l.fi[f] = fi[f];
    l.nS = kPe * l.Fe + kPi * l.Fi;
    l.pad = 0;
  }
  // unknown j < nS: its camera and its column of the row
  MK_HD static void unknown(const Layout& l, int j, int& cam, int& col) {
    const int ne = kE ? kPe * l.Fe : 0;
    if (kE && (!kI || j < ne)) {
      cam = l.fe[j / kPe];
      col = kColE + j % kPe;
    } else {
      cam = l.fi[(j - ne) / kPi];
      col = kColI + (j - ne) % kPi;
    }
  }

  // the slot from the refinement's slot of the same observation, Je and Ji
  // (either is not read by a problem without its block)
  MK_HD static void widen(const refine::Slot& s, const double* Je, const double* Ji, Slot& o) {
    for (int e = 0; e < 6; e++) o.row[e] = s.row[e];
    if constexpr (kE)
      for (int e = 0; e < kPe; e++) o.row[kColE + e] = s.code ? 0.0 : Je[e];
    if constexpr (kI)
      for (int e = 0; e < kPi; e++) o.row[kColI + e] = s.code ? 0.0 : Ji[e];
    o.row[kColR] = s.row[6];
    o.code = s.code;
    o.Sw = s.Sw;
    o.Skw = s.Skw;
    o.pad = 0;
  }

  // One observation on the host: refine::observe at the current intrinsics and
  // extrinsic, then the extrinsic's and the intrinsics' columns from one
  // geometry. Without J_ext the geometry is refine::geom itself; calib::geom
  // restates its expressions (the same bits).
  MK_HD static void observe(const double* Rwb_t, const double* twb, const GnCam& cm, const Cam& cam, const uint8_t* bgr,
                            int W, int H, const double* X, int axis, const int* target, const refine::Window& win,
                            bool free_ext, bool free_int, uint32_t param_mask, Slot& o, int* tie) {
    refine::Slot s;
    refine::observe(Rwb_t, twb, cm, cam, bgr, W, H, X, axis, target, win, s, tie);
    calib::Geom g;
    double Ji[kPi];
    for (int e = 0; e < kPe; e++) g.Je[e] = 0.0;
    for (int e = 0; e < kPi; e++) Ji[e] = 0.0;
    if (!s.code) {
      if constexpr (kE) (void)calib::geom(Rwb_t, twb, cm, X, axis, free_ext, g);
      else (void)refine::geom(Rwb_t, twb, cm, X, axis, g.g);
      if constexpr (kI) icalib::jint(cam, g.g.m0, g.g.nh, free_int, param_mask, Ji);
    }
    widen(s, g.Je, Ji, o);
  }

  MK_HD static void accumulate_row(const double* v, double* acc) {
    int n = 0;
    for (int a = 0; a < kRow; a++)
      for (int b = a; b < kRow; b++) acc[n++] += v[a] * v[b];
  }

  // ---- the reduced system. acc: a view's C x kAcc (or every view's N x C x kAcc) ----
  // A_r(i, j) = sum_c PP_rc(i, j) in camera order, + lambda on the diagonal
  MK_HD static double view_A(const double* acc, int C, int i, int j, double lambda) {
    const int e = tri_sym(i, j);
    double s = 0.0;
    for (int c = 0; c < C; c++) s += acc[kAcc * c + e];
    return i == j ? s + lambda : s;
  }
  // [E_r | a_r](k, j): column j < nS is the unknown's column of its camera's PE / PI; column nS is sum_c Pr_rc
  MK_HD static double view_rhs(const double* acc, int C, const Layout& l, int k, int j) {
    if (j < l.nS) {
      int cam, col;
      unknown(l, j, cam, col);
      return acc[kAcc * cam + tri(k, col)];
    }
    double s = 0.0;
    for (int c = 0; c < C; c++) s += acc[kAcc * c + tri(k, kColR)];
    return s;
  }
  // the view's Schur term (E_r^T Y_r)(i, j), Y_r = A_r^-1 [E_r | a_r]; Em and Y: 6 x kLd
  MK_HD static double schur_entry(const double* Em, const double* Y, int i, int j) {
    double s = 0.0;
    for (int k = 0; k < 6; k++) s += Em[kLd * k + i] * Y[kLd * k + j];
    return s;
  }
  // x = A_r^-1 b for strided columns of leading dimension kLd (calib::chol6_solve)
  MK_HD static void view_solve(const double* L6, const double* b, double* x) { calib::chol6_solve(L6, b, kLd, x, kLd); }
  // B(i, j) of the reduced system before the views' terms go: the camera's EE, EI
  // or II entry summed in view order (zero for two cameras), + lambda on the
  // diagonal; a held parameter's diagonal entry is exactly 1
  MK_HD static double reduced_B(const double* acc, int N, int C, const Layout& l, int i, int j, double lambda,
                                uint32_t param_mask) {
    int ci, coli, cj, colj;
    unknown(l, i, ci, coli);
    unknown(l, j, cj, colj);
    double B = 0.0;
    if (ci == cj) {
      const double* a0 = acc + kAcc * ci + tri_sym(coli, colj);
      const size_t vs = (size_t)kAcc * C;
      for (int r = 0; r < N; r++) B += a0[vs * r];
      if (i == j) {
        B += lambda;
        if (kI && coli >= kColI && !(param_mask >> (coli - kColI) & 1u)) B = 1.0;
      }
    }
    return B;
  }
  // [S | s](i, j), i < nS, j <= nS: S = B - sum_r E_r^T A_r^-1 E_r, s = -b + sum_r E_r^T A_r^-1 a_r,
  // every sum in view order. acc: N x C x kAcc; Wt: the views' Schur terms, N x kMaxS x kLd.
  MK_HD static double reduced_entry(const double* acc, const double* Wt, int N, int C, const Layout& l, int i, int j,
                                    double lambda, uint32_t param_mask) {
    double sw = 0.0;
    for (int r = 0; r < N; r++) sw += Wt[((size_t)r * kMaxS + i) * kLd + j];
    if (j == l.nS) {
      int ci, coli;
      unknown(l, i, ci, coli);
      const double* a0 = acc + kAcc * ci + tri(coli, kColR);
      const size_t vs = (size_t)kAcc * C;
      double b = 0.0;
      for (int r = 0; r < N; r++) b += a0[vs * r];
      return -b + sw;
    }
    return reduced_B(acc, N, C, l, i, j, lambda, param_mask) - sw;
  }
  // Left-looking Cholesky of S (lower triangle, leading dimension kLd), column j:
  // the pivot's square and an entry below it, each by the sequential formula.
  // L's diagonal is kept apart (Ld), so L's strict lower triangle may overwrite
  // S's in place: entry (i, j) of S is read by its own column only, S's
  // diagonal never goes.
  MK_HD static double cholS_pivot(const double* S, const double* L, int j) {
    double s = S[kLd * j + j];
    for (int k = 0; k < j; k++) s -= L[kLd * j + k] * L[kLd * j + k];
    return s;
  }
  MK_HD static double cholS_below(const double* S, const double* L, int i, int j, double ljj) {
    double s = S[kLd * i + j];
    for (int k = 0; k < j; k++) s -= L[kLd * i + k] * L[kLd * j + k];
    return s / ljj;
  }
  // x = (L L^T)^-1 b for the n x n factor; b strided, y: n of scratch
  MK_HD static void cholS_solve(const double* L, const double* Ld, int n, const double* b, int ldb, double* y, double* x) {
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
  MK_HD static void pose_delta(const double* Y, const double* eps, int nS, double* d6) {
    for (int k = 0; k < 6; k++) {
      double s = Y[kLd * k + nS];
      for (int j = 0; j < nS; j++) s += Y[kLd * k + j] * eps[j];
      d6[k] = -s;
    }
  }

  // the starved gate of a pass: some view with fewer than min_obs rows over its
  // cameras, or some camera free in either mask with fewer than min_obs_cam
  // rows over the views
  MK_HD static bool starved(const int32_t* cnt, int N, int C, uint32_t free_ext, uint32_t free_int, int32_t min_obs,
                            int32_t min_obs_cam) {
    for (int r = 0; r < N; r++) {
      int32_t n = 0;
      for (int c = 0; c < C; c++) n += cnt[r * C + c];
      if (n < min_obs) return true;
    }
    for (int c = 0; c < C; c++) {
      if (!((free_ext | free_int) >> c & 1)) continue;
      int32_t n = 0;
      for (int r = 0; r < N; r++) n += cnt[r * C + c];
      if (n < min_obs_cam) return true;
    }
    return false;
  }
  // r^T r of a pass, summed in (view, camera) order
  MK_HD static double sum_rr(const double* acc, int N, int C) {
    double s = 0.0;
    for (int k = 0; k < N * C; k++) s += acc[(size_t)kAcc * k + (kAcc - 1)];
    return s;
  }

  // 0, or 1 / 2 when some A_r / S is not positive definite
  static int reduce(const double* acc, int N, int C, uint32_t free_ext, uint32_t free_int, uint32_t param_mask,
                    double lambda, Reduced& w) {
    layout(free_ext, free_int, C, w.l);
    const int nS = w.l.nS;
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
        for (int j = 0; j <= nS; j++) Em[kLd * k + j] = view_rhs(av, C, w.l, k, j);
      double* Y = w.Y.data() + (size_t)r * 6 * kLd;
      for (int j = 0; j <= nS; j++) view_solve(L6, Em + j, Y + j);
      double* Wr = w.Wt.data() + (size_t)r * kMaxS * kLd;
      for (int i = 0; i < nS; i++)
        for (int j = 0; j <= nS; j++) Wr[kLd * i + j] = schur_entry(Em, Y, i, j);
    }
    for (int i = 0; i < nS; i++)
      for (int j = 0; j <= nS; j++)
        w.S[kLd * i + j] = reduced_entry(acc, w.Wt.data(), N, C, w.l, i, j, lambda, param_mask);
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
  static void tally(const double* acc, const int32_t* cnt, int N, int C, int pass, mantis_rcalib_result& R) {
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
  // from the views' accumulators (N x C x kAcc) and counts (N x C). Returns true
  // when the call is finished (the final pass, STARVED, SINGULAR or DIVERGED);
  // otherwise T (N x 16), R.T_base_cam and R.K / R.D are the next estimates,
  // delta (N x 6, nullable) the poses' steps and R.delta_ext[pass] /
  // R.delta_int[pass] the cameras'. With the robust rows acc is the weighted
  // one and pos (N x C, else null) the rows with w > 0: too few of them in a
  // view or a free camera starve the pass too.
  static bool end_pass(const double* acc, const int32_t* cnt, int N, int C, uint32_t free_ext, uint32_t free_int,
                       uint32_t param_mask, int pass, int I, int32_t min_obs, int32_t min_obs_cam, double lambda,
                       double* T, mantis_rcalib_result& R, double* delta, const int32_t* pos = nullptr) {
    tally(acc, cnt, N, C, pass, R);
    if (pass >= I) return true;
    if (starved(cnt, N, C, free_ext, free_int, min_obs, min_obs_cam) ||
        (pos && starved(pos, N, C, free_ext, free_int, min_obs, min_obs_cam))) {
      R.status = kStarved;
      return true;
    }
    Reduced w;
    if (reduce(acc, N, C, free_ext, free_int, param_mask, lambda, w)) {
      R.status = kSingular;
      return true;
    }
    const Layout& l = w.l;
    double eps[kMaxS], y[kMaxS], next[kMaxCams][kPi];
    cholS_solve(w.L.data(), w.Ld.data(), l.nS, w.S.data() + l.nS, kLd, y, eps);
    const double* epi = eps + kPe * l.Fe;
    bool ok = true;
    for (int f = 0; f < l.Fi; f++) {
      double th[kPi];
      icalib::cam_to(icalib::cam_of(R.K[l.fi[f]], R.D[l.fi[f]]), th);
      ok = icalib::param_update(th, epi + kPi * f, param_mask, next[f]) && ok;
    }
    if (!ok) {
      R.status = kDiverged;
      return true;
    }
    for (int r = 0; r < N; r++) {
      double d6[6];
      pose_delta(w.Y.data() + (size_t)r * 6 * kLd, eps, l.nS, d6);
      calib::right_update(T + 16 * (size_t)r, d6);
      if (delta)
        for (int e = 0; e < 6; e++) delta[6 * (size_t)r + e] = d6[e];
    }
    for (int f = 0; f < l.Fe; f++) {
      calib::right_update(R.T_base_cam[l.fe[f]], eps + kPe * f);
      for (int e = 0; e < kPe; e++) R.delta_ext[pass][l.fe[f]][e] = eps[kPe * f + e];
    }
    for (int f = 0; f < l.Fi; f++) {
      const int c = l.fi[f];
      for (int e = 0; e < 4; e++) {
        R.K[c][e] = next[f][e];
        R.D[c][e] = next[f][4 + e];
      }
      for (int e = 0; e < kPi; e++) R.delta_int[pass][c][e] = (param_mask >> e & 1u) ? epi[kPi * f + e] : 0.0;
    }
    R.iterations_run = pass + 1;
    return false;
  }

  // Host: the gate, rms_cam and the covariances from the last pass's
  // accumulators and counts (include/mantis.h). dof = n_obs - 6 N - 6 Fe - P, P
  // the free parameters over the cameras of free_int; calibrated = status OK,
  // no starved gate on that pass, the rms gate, dof > 0 and S (lambda = 0)
  // positive definite. cov_ext[c] / cov_int[c] = (r^T r / dof) (S^-1)_cc, the
  // marginal over the poses; cov_ext in the order x, y, z, rot-x, rot-y, rot-z
  // of the right perturbation; R.K holds the final intrinsics: they scale
  // cov_int to natural units. Otherwise zeros. pos (nullable): end_pass's, of
  // the last pass; its two gates count as starved gates here too.
  static void conclude(const double* acc, const int32_t* cnt, int N, int C, uint32_t free_ext, uint32_t free_int,
                       uint32_t param_mask, int32_t min_obs, int32_t min_obs_cam, double max_rms,
                       mantis_rcalib_result& R, const int32_t* pos = nullptr) {
    const int fp = R.iterations_run;
    for (int c = 0; c < kMaxCams; c++) {
      R.rms_cam[c] = 0.0;
      for (int e = 0; e < kPe * kPe; e++) R.cov_ext[c][e] = 0.0;
      for (int e = 0; e < kPi * kPi; e++) R.cov_int[c][e] = 0.0;
    }
    for (int c = 0; c < C; c++) {
      double s = 0.0;
      for (int r = 0; r < N; r++) s += acc[(size_t)kAcc * (r * C + c) + (kAcc - 1)];
      if (R.n_obs_cam[fp][c] > 0) R.rms_cam[c] = sqrt(s / (double)R.n_obs_cam[fp][c]);
    }
    Layout l;
    layout(free_ext, free_int, C, l);
    int np = 0;
    for (int e = 0; e < kPi; e++) np += (int)(param_mask >> e & 1u);
    const int64_t dof = (int64_t)R.n_obs[fp] - 6 * (int64_t)N - 6 * (int64_t)l.Fe - (int64_t)np * l.Fi;
    R.calibrated = R.status == kOk && !starved(cnt, N, C, free_ext, free_int, min_obs, min_obs_cam) &&
                   !(pos && starved(pos, N, C, free_ext, free_int, min_obs, min_obs_cam)) &&
                   (max_rms <= 0 || R.rms[fp] <= max_rms) && dof > 0;
    if (!R.calibrated) return;
    Reduced w;
    if (reduce(acc, N, C, free_ext, free_int, param_mask, 0.0, w)) {
      R.calibrated = 0;
      return;
    }
    const double sigma2 = sum_rr(acc, N, C) / (double)dof;
    std::vector<double> e(kMaxS), y(kMaxS), x(kMaxS);
    for (int f = 0; f < l.Fe; f++) {
      double* cov = R.cov_ext[l.fe[f]];
      const int o = kPe * f;
      for (int col = 0; col < kPe; col++) {
        for (int i = 0; i < l.nS; i++) e[i] = i == o + col ? 1.0 : 0.0;
        cholS_solve(w.L.data(), w.Ld.data(), l.nS, e.data(), 1, y.data(), x.data());
        for (int i = 0; i < kPe; i++) cov[kPe * i + col] = sigma2 * x[o + i];
      }
      for (int i = 0; i < kPe; i++)  // the two triangles came from different solves: publish one
        for (int j = i + 1; j < kPe; j++) cov[kPe * j + i] = cov[kPe * i + j];
    }
    for (int f = 0; f < l.Fi; f++) {
      double* cov = R.cov_int[l.fi[f]];
      const double* K4 = R.K[l.fi[f]];
      const double sc[kPi] = {K4[0], K4[1], K4[0], K4[1], 1.0, 1.0, 1.0, 1.0};
      const int o = kPe * l.Fe + kPi * f;
      for (int col = 0; col < kPi; col++) {
        if (!(param_mask >> col & 1u)) continue;
        for (int i = 0; i < l.nS; i++) e[i] = i == o + col ? 1.0 : 0.0;
        cholS_solve(w.L.data(), w.Ld.data(), l.nS, e.data(), 1, y.data(), x.data());
        for (int i = 0; i < kPi; i++)
          if (param_mask >> i & 1u) cov[kPi * i + col] = sc[i] * (sigma2 * x[o + i]) * sc[col];
      }
      for (int i = 0; i < kPi; i++)
        for (int j = i + 1; j < kPi; j++) cov[kPi * j + i] = cov[kPi * i + j];
    }
  }

  // The whole call on the host, rows summed in slot order (slot = camera x
  // n_cand + candidate inside a view). frames[r * C + c]: W x H, stride 3 W;
  // Tbc: the starting extrinsics, C x 16; cams: the starting intrinsics (K
  // already rounded to float); T_in / T_out: N x 16. slots (nullable): N x C x
  // n_cand of the last pass taken. A problem without a block takes 0 for its
  // mask (and for param_mask without J_int). rb (nullable; loss 0 is null): the
  // robust rows -- every pass first takes all its slots, then weighs them from
  // the call-wide median and sums sqrt(w) row in slot order; stats (nullable)
  // are filled only then.
  static void seq(const double* T_in, const double* Tbc, const Cam* cams, const uint8_t* const* frames, int N, int C,
                  int W, int H, const double* X, int nw, int nr, const int32_t* cand, int n_cand,
                  const mantis_refine_params& p, uint32_t fe, uint32_t fi, uint32_t pm, int32_t min_obs_cam,
                  double* T_out, mantis_rcalib_result& R, Slot* slots, const refine::Robust* rb = nullptr,
                  mantis_calib_robust_stats* stats = nullptr) {
    if (rb && rb->loss == refine::kLossNone) rb = nullptr;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (rb && stats) {
      stats->loss = rb->loss;
      stats->kind = kE && kI ? kKindRig : kI ? kKindInt : kKindExt;
      stats->n_rigs = N;
      stats->n_cams = C;
    }
    std::memset(&R, 0, sizeof(R));
    R.n_cand = n_cand;
    R.n_rigs = N;
    R.n_cams = C;
    R.free_ext = (int32_t)fe;
    R.free_int = (int32_t)fi;
    R.param_mask = (int32_t)pm;
    for (int c = 0; c < C; c++) {
      double th[kPi];
      icalib::cam_to(cams[c], th);
      for (int e = 0; e < 4; e++) {
        R.K[c][e] = th[e];
        R.D[c][e] = th[4 + e];
      }
      for (int e = 0; e < 16; e++) R.T_base_cam[c][e] = Tbc[16 * c + e];
    }
    for (size_t e = 0; e < 16 * (size_t)N; e++) T_out[e] = T_in[e];
    const refine::Window win{p.half_window, p.white_thresh, p.min_weight, 0};
    std::vector<double> acc((size_t)N * C * kAcc);
    std::vector<int32_t> cnt((size_t)N * C);
    // the robust rows' pass: its slots, codes and sums, keys, weights, cells and rows with w > 0
    const size_t ns = rb ? (size_t)N * C * n_cand : 0;
    std::vector<Slot> all(ns);
    std::vector<int32_t> codes(ns), Sw(ns), Skw(ns), pos(rb ? (size_t)N * C : 0);
    std::vector<uint32_t> keys(ns);
    std::vector<double> wts(ns);
    std::vector<RobustCell> cells(rb ? (size_t)N * C : 0);
    for (int pass = 0; pass <= p.iterations; pass++) {
      for (int r = 0; r < N && rb; r++) {
        double Rt[9], t[3];
        refine::pose_parts(T_out + 16 * (size_t)r, Rt, t);
        for (int c = 0; c < C; c++) {
          GnCam gc;
          refine::gncam_from(R.T_base_cam[c], gc);
          const Cam cm = icalib::cam_of(R.K[c], R.D[c]);
          for (int k = 0; k < n_cand; k++) {
            const int i = cand[k] & 0xffff, axis = cand[k] >> 16;
            int tg[3];
            refine::target_bgr(i, nw, nr, tg);
            const size_t q = ((size_t)r * C + c) * n_cand + k;
            observe(Rt, t, gc, cm, frames[r * C + c], W, H, X + 3 * i, axis, tg, win, (fe >> c & 1) != 0,
                    (fi >> c & 1) != 0, pm, all[q], nullptr);
            codes[q] = all[q].code;
            Sw[q] = all[q].Sw;
            Skw[q] = all[q].Skw;
          }
        }
      }
      if (rb) {
        refine::RobustPass P;
        robust_pass(codes.data(), Sw.data(), Skw.data(), N, C, n_cand, *rb, keys.data(), wts.data(), cells.data(), P);
        for (int f = 0; f < N * C; f++) {
          double* a = acc.data() + (size_t)kAcc * f;
          for (int e = 0; e < kAcc; e++) a[e] = 0.0;
          int32_t n = 0;
          for (int k = 0; k < n_cand; k++) {
            const size_t q = (size_t)f * n_cand + k;
            const double sq = sqrt(wts[q]);
            double v[kRow];
            for (int e = 0; e < kRow; e++) v[e] = all[q].row[e] * sq;
            accumulate_row(v, a);
            n += codes[q] == 0;
          }
          cnt[f] = n;
        }
        if (slots) std::memcpy(slots, all.data(), sizeof(Slot) * ns);
        robust_pos(cells.data(), cnt.data(), N * C, pos.data());
        if (stats) robust_tally(cells.data(), cnt.data(), N, C, pass, P.median_key, P.scale, *stats);
        if (end_pass(acc.data(), cnt.data(), N, C, fe, fi, pm, pass, p.iterations, p.min_obs, min_obs_cam, p.lambda,
                     T_out, R, nullptr, pos.data()))
          break;
        continue;
      }
      for (int r = 0; r < N; r++) {
        double Rt[9], t[3];
        refine::pose_parts(T_out + 16 * (size_t)r, Rt, t);
        for (int c = 0; c < C; c++) {
          GnCam gc;
          refine::gncam_from(R.T_base_cam[c], gc);
          const Cam cm = icalib::cam_of(R.K[c], R.D[c]);
          double* a = acc.data() + (size_t)kAcc * (r * C + c);
          for (int e = 0; e < kAcc; e++) a[e] = 0.0;
          int32_t n = 0;
          for (int k = 0; k < n_cand; k++) {
            const int i = cand[k] & 0xffff, axis = cand[k] >> 16;
            int tg[3];
            refine::target_bgr(i, nw, nr, tg);
            Slot o;
            observe(Rt, t, gc, cm, frames[r * C + c], W, H, X + 3 * i, axis, tg, win, (fe >> c & 1) != 0,
                    (fi >> c & 1) != 0, pm, o, nullptr);
            if (slots) slots[((size_t)r * C + c) * n_cand + k] = o;
            accumulate_row(o.row, a);
            n += o.code == 0;
          }
          cnt[r * C + c] = n;
        }
      }
      if (end_pass(acc.data(), cnt.data(), N, C, fe, fi, pm, pass, p.iterations, p.min_obs, min_obs_cam, p.lambda, T_out,
                   R, nullptr))
        break;
    }
    conclude(acc.data(), cnt.data(), N, C, fe, fi, pm, p.min_obs, min_obs_cam, p.max_rms, R, rb ? pos.data() : nullptr);
  }
};

using Ext = Problem<true, false>;  // mantis_calibrate_extrinsics
using Int = Problem<false, true>;  // mantis_calibrate_intrinsics
using Rig = Problem<true, true>;   // mantis_calibrate_rig

// ---- the working state and the two single calibrations' public structs ----
// The fields every result has, by name (A, B: any two of the three structs).
template <class A, class B>
inline void copy_figures(const A& a, B& b) {
  b.status = a.status;
  b.calibrated = a.calibrated;
  b.iterations_run = a.iterations_run;
  b.n_cand = a.n_cand;
  b.n_rigs = a.n_rigs;
  b.n_cams = a.n_cams;
  std::memcpy(b.n_obs, a.n_obs, sizeof(a.n_obs));
  std::memcpy(b.n_obs_cam, a.n_obs_cam, sizeof(a.n_obs_cam));
  std::memcpy(b.rms, a.rms, sizeof(a.rms));
  std::memcpy(b.rms_cam, a.rms_cam, sizeof(a.rms_cam));
}
// narrow: the public struct of a finished (or running) call, pads zero;
// widen: the working state that narrows back to it, everything else zero
inline void narrow(const mantis_rcalib_result& w, mantis_calib_result& o) {
  std::memset(&o, 0, sizeof(o));
  copy_figures(w, o);
  o.free_cams = w.free_ext;
  std::memcpy(o.T_base_cam, w.T_base_cam, sizeof(o.T_base_cam));
  std::memcpy(o.delta_cam, w.delta_ext, sizeof(o.delta_cam));
  std::memcpy(o.covariance, w.cov_ext, sizeof(o.covariance));
}
inline void widen(const mantis_calib_result& o, mantis_rcalib_result& w) {
  std::memset(&w, 0, sizeof(w));
  copy_figures(o, w);
  w.free_ext = o.free_cams;
  std::memcpy(w.T_base_cam, o.T_base_cam, sizeof(o.T_base_cam));
  std::memcpy(w.delta_ext, o.delta_cam, sizeof(o.delta_cam));
  std::memcpy(w.cov_ext, o.covariance, sizeof(o.covariance));
}
inline void narrow(const mantis_rcalib_result& w, mantis_icalib_result& o) {
  std::memset(&o, 0, sizeof(o));
  copy_figures(w, o);
  o.free_cams = w.free_int;
  o.param_mask = w.param_mask;
  std::memcpy(o.K, w.K, sizeof(o.K));
  std::memcpy(o.D, w.D, sizeof(o.D));
  std::memcpy(o.delta_cam, w.delta_int, sizeof(o.delta_cam));
  std::memcpy(o.covariance, w.cov_int, sizeof(o.covariance));
}
inline void widen(const mantis_icalib_result& o, mantis_rcalib_result& w) {
  std::memset(&w, 0, sizeof(w));
  copy_figures(o, w);
  w.free_int = o.free_cams;
  w.param_mask = o.param_mask;
  std::memcpy(w.K, o.K, sizeof(o.K));
  std::memcpy(w.D, o.D, sizeof(o.D));
  std::memcpy(w.delta_int, o.delta_cam, sizeof(o.delta_cam));
  std::memcpy(w.cov_int, o.covariance, sizeof(o.covariance));
}
// fn on the working state of a single calibration's public struct R, and back
template <class Res, class Fn>
inline auto with_state(Res& R, Fn fn) {
  mantis_rcalib_result w;
  widen(R, w);
  if constexpr (std::is_void_v<decltype(fn(w))>) {
    fn(w);
    narrow(w, R);
  } else {
    auto r = fn(w);
    narrow(w, R);
    return r;
  }
}
static_assert(sizeof(mantis_calib_result::delta_cam) == sizeof(mantis_rcalib_result::delta_ext) &&
                  sizeof(mantis_calib_result::covariance) == sizeof(mantis_rcalib_result::cov_ext) &&
                  sizeof(mantis_icalib_result::delta_cam) == sizeof(mantis_rcalib_result::delta_int) &&
                  sizeof(mantis_icalib_result::covariance) == sizeof(mantis_rcalib_result::cov_int),
              "the working state is a superset of the single calibrations' results");

}  // namespace linecal
}  // namespace mk
