// The three calibrations on the grid lines (mantis_calibrate_extrinsics,
// mantis_calibrate_intrinsics, mantis_calibrate_rig, include/mantis.h): one
// joint Gauss-Newton over the base poses of N views of one rig and the
// extrinsics of the cameras in free_ext and / or the eight intrinsics of the
// cameras in free_int. Included by api.hip after refine_impl.hip: it shares
// the frame staging, the candidate list and the line-flag cache (refine_flags)
// and Landmarks with the refinement. The rules -- one observation with J_ext
// and J_int, the views' elimination, the reduced system, the updates, the gate
// and the covariances -- are in mk_linecal.h (shared with the host build of
// the tests). Every kernel and the driver are templates over the problem P
// (linecal::Ext, Int or Rig: which of the two column blocks a row has).
//
// Device work of one call of I iterations, all on the context stream:
//   per pass k = 0 .. I:  k_linecal_obs    the (view, camera, candidate) slots at
//                                          the poses, extrinsics and intrinsics
//                                          of pass k
//                         k_linecal_rig    per view: M^T M per camera (one MFMA
//                                          tile per wave and camera, three for
//                                          the 21 columns of Rig), A_r's
//                                          Cholesky, Y_r, the view's Schur term
//                         k_linecal_solve  the gates, S and its Cholesky, eps,
//                                          every delta_r, the updates
// = 3 (I + 1) launches, then the copies of the state, the poses and the last
// pass's accumulators. As in refine_impl.hip every hand-off between blocks
// crosses a kernel boundary: no last-block counter, no flag polled inside a
// kernel, no hipGraph capture. Nothing is drawn, no image stage runs.
//
// With the robust rows on (mantis_calib_set_robust) a pass is five launches:
//   k_linecal_obs<P, true>    also stores every slot's key, compact
//   k_linecal_hist<0>         per view: a 4096-bin LDS histogram of the keys' top
//                             12 bits, folded into the pass's table (integer
//                             atomicAdd: the counts do not depend on the order)
//   k_linecal_hist<1>         every block scans that table (the same n, bin and
//                             rank in every block), then its view's low 12 bits
//                             inside the bin, folded into the second table
//   k_linecal_rig<P, true>    scans the second table for the median, forms
//                             sqrt(w) once per row in LDS, the MFMA loops on
//                             row x sqrt(w), the (view, camera) cells
//   k_linecal_solve<P, true>  the gates on the rows with w > 0, the stats
// The tables of all passes are zeroed by one memset before the first pass. The
// kernels of the switch-off call are the <P, false> instantiations: none of
// the robust code is in them.
#include "mk_linecal.h"

namespace mk {

namespace cal = calib;
namespace lc = linecal;

struct LinecalState {  // the call between the launches, and what comes back
  int32_t done, pad;
  mantis_rcalib_result res;  // res.T_base_cam, res.K / res.D = the current extrinsics and intrinsics
};
// What travels between host and device: everything before the covariances, which are the
// host's alone (conclude) and the struct's last 6.4 KB. The rest is 11 KB: the two single
// calibrations' own states were 8 and 10 KB, and a copy of the whole 17.5 KB took each of their
// calls some 35 us longer on the host.
constexpr size_t kLinecalStateBytes = offsetof(LinecalState, res) + offsetof(mantis_rcalib_result, cov_ext);
static_assert(offsetof(mantis_rcalib_result, cov_ext) + sizeof(mantis_rcalib_result::cov_ext) +
                      sizeof(mantis_rcalib_result::cov_int) == sizeof(mantis_rcalib_result),
              "the covariances are the result's last fields");

// the robust rows' buffers (null with the switch off)
struct LinecalRobust {
  uint32_t* keys;     // [pass (record) or one][view][C n_cand], laid out as the slots: the key, kNoKey where rejected
  double* weights;    // the same: the record's weights, or null
  uint32_t* tab;      // [pass][kLinecalTab]: the top digit's table, the low digit's, then n, the top digit, the rank
                      // inside it and the median key; zeroed before the first pass
  lc::RobustCell* cells;             // N x C of the pass
  mantis_calib_robust_stats* stats;  // of the call
  rfn::Robust rb;
};
constexpr int kLinecalTab = 2 * kRobustBins + 4;  // words of a pass's tables
constexpr int kLinecalChunk = 544;  // candidates per camera whose sqrt(w) wait in LDS at a time: 17 trips of 32 rows
                                    // (a whole number of trips of either loop); the full map has 540

struct LinecalArgs {
  const int32_t* cand;  // n_cand: landmark | axis << 16
  LinecalState* st;
  double* T;            // N x 16: the views' current poses
  void* slots;          // P::Slot [pass][view][C n_cand]; pass_slots = the stride between passes (record) or 0
  double* acc;          // N x C x kAcc of the pass
  double* recAcc;       // [pass][N][C][kAcc] (record) or null
  int32_t* cnt;         // N x C code-0 rows
  double* Y;            // N x 6 x kLd: A_r^-1 [E_r | a_r]
  double* Wt;           // N x kMaxS x kLd: the views' Schur terms (lower triangle and the last column)
  int32_t* pd;          // N: A_r was positive definite
  double* recT;         // [pass][N][16]: the poses each pass observed at
  double* recE;         // [pass][C][16]: the extrinsics (problems with J_ext)
  double* recKD;        // [pass][C][8]: the intrinsics (problems with J_int)
  size_t pass_slots;
  int32_t C, n_cand, I, N, min_obs, min_obs_cam;
  uint32_t free_ext, free_int, param_mask;
  lc::Layout l;         // the reduced unknowns
  rfn::Window win;
  double lambda;
  LinecalRobust r;
};

// k_refine_obs' scheme (refine_impl.hip) with the camera's extrinsic and,
// where the problem has J_int, its eight intrinsics read from the call's state
// (they change per pass; without J_int the intrinsics are the staged frame's):
// block (candidate chunk, camera, view), two candidates per wave, one per
// 32-lane half, one distort and one pixel per lane, integer sums by
// __shfl_xor inside the half, J_ext and J_int from the half's geometry and one
// plain store of the slot by lane 0 of the half.
// kR (the robust rows): also the slot's key, compact, for the selection.
template <class P, bool kR = false>
__global__ __launch_bounds__(256) void k_linecal_obs(const FrameDesc* __restrict__ frames, Landmarks lmk, LinecalArgs a,
                                                     int pass) {
  using Slot = typename P::Slot;
  const int chunk = blockIdx.x, cam = blockIdx.y, rig = blockIdx.z;
  const LinecalState& S = *a.st;
  if (S.done) return;  // block-uniform: the call stopped in an earlier pass
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, l = lane & 31;
  const int f = rig * a.C + cam;
  const Cam cm = P::kInt ? icalib::cam_of(S.res.K[cam], S.res.D[cam]) : frames[f].cam;
  const uint8_t* bgr = frames[f].bgr;
  const int W = frames[f].w, H = frames[f].h, npx = W * H;
  GnCam gc;
  rfn::gncam_from(S.res.T_base_cam[cam], gc);
  const bool free_ext = (a.free_ext >> cam & 1u) != 0, free_int = (a.free_int >> cam & 1u) != 0;
  double Rt[9], tw[3];
  rfn::pose_parts(a.T + 16 * (size_t)rig, Rt, tw);
  const double s = 1.0 / cm.fx;
  const int k = l - a.win.R;
  const bool active = l <= 2 * a.win.R;
  Slot* out = (Slot*)a.slots + (size_t)pass * a.pass_slots + (size_t)f * a.n_cand;
  const int c0 = chunk * kRefineCands, c1 = min(c0 + kRefineCands, a.n_cand);
  for (int base = c0 + wave * 2; base < c1; base += 8) {  // wave-uniform trips: every lane reaches the shuffles
    const int ci = base + half;
    const bool live = ci < c1;  // an odd tail: the second half repeats the first's candidate and stores nothing
    const int cv = a.cand[live ? ci : base];
    const int i = cv & 0xffff, axis = cv >> 16;
    int tg[3];
    rfn::target_bgr(i, lmk.nw, lmk.nr, tg);
    cal::Geom g;  // g.Je: set and read only with J_ext
    int gcode;
    if constexpr (P::kExt) gcode = cal::geom(Rt, tw, gc, lmk.xyz + 3 * i, axis, free_ext, g);
    else gcode = rfn::geom(Rt, tw, gc, lmk.xyz + 3 * i, axis, g.g);
    int outside;
    int32_t Sw, Skw, w_lo, w_hi;
    refine_window(cm, bgr, W, H, npx, tg, g.g, gcode, s, k, active, a.win, outside, Sw, Skw, w_lo, w_hi);
    if (l == 0 && live) {
      rfn::Slot o7;
      rfn::finish(gcode, outside != 0, w_lo, w_hi, Sw, Skw, a.win.min_weight, s, g.g, o7);
      double Ji[lc::kPi];
      if constexpr (P::kInt) {
#pragma unroll
        for (int e = 0; e < lc::kPi; e++) Ji[e] = 0.0;
        if (!o7.code) icalib::jint(cm, g.g.m0, g.g.nh, free_int, a.param_mask, Ji);
      }
      Slot o;
      P::widen(o7, g.Je, Ji, o);
      out[ci] = o;
      if constexpr (kR)
        a.r.keys[(size_t)pass * a.pass_slots + (size_t)f * a.n_cand + ci] =
            o7.code ? kNoKey : rfn::robust_key(o7.Sw, o7.Skw);
    }
  }
}

// The selection of the call-wide median key, one block per view, launched twice
// per pass. kPhase 0: the 4096-bin LDS histogram of the top 12 bits of the
// view's keys (keys are below 2^24), folded into the pass's first table.
// kPhase 1: every block loads that table and finds n, the bin of rank (n - 1) /
// 2 and the rank inside the bin -- integers from the same table, so the same in
// every block; block 0 leaves them for k_linecal_rig -- then histograms the low
// 12 bits of its view's keys inside that bin into the second table. Integer
// atomicAdd only; the tables were zeroed before the first pass.
template <int kPhase>
__global__ __launch_bounds__(256) void k_linecal_hist(LinecalArgs a, int pass) {
  __shared__ uint32_t hist[kRobustBins];
  __shared__ uint32_t wsum[4], sel[2];
  const int rig = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  if (a.st->done) return;
  const int rows = a.C * a.n_cand;
  const uint32_t* keys = a.r.keys + (size_t)pass * a.pass_slots + (size_t)rig * rows;
  uint32_t* tab = a.r.tab + (size_t)pass * kLinecalTab;
  uint32_t hi = 0;
  if constexpr (kPhase == 1) {
    for (int i = t; i < kRobustBins; i += 256) hist[i] = tab[i];
    __syncthreads();
    uint32_t own = 0;
#pragma unroll
    for (int b = 0; b < kRobustBins / 256; b++) own += hist[t * (kRobustBins / 256) + b];
#pragma unroll
    for (int q = 32; q >= 1; q >>= 1) own += __shfl_xor(own, q, 64);
    if (lane == 0) wsum[wave] = own;
    __syncthreads();
    const uint32_t n = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();  // robust_select writes wsum
    if (n == 0) return;  // block-uniform: the tables and the words stay zero
    uint32_t rest;
    hi = robust_select(hist, (n - 1) / 2, wsum, sel, &rest);
    if (rig == 0 && t == 0) {
      tab[2 * kRobustBins] = n;
      tab[2 * kRobustBins + 1] = hi;
      tab[2 * kRobustBins + 2] = rest;
    }
  }
  for (int i = t; i < kRobustBins; i += 256) hist[i] = 0;
  __syncthreads();
  for (int r = t; r < rows; r += 256) {
    const uint32_t key = keys[r];  // kNoKey >> 12 is no top digit of a key
    if constexpr (kPhase == 0) {
      if ((key >> 12) < (uint32_t)kRobustBins) atomicAdd(&hist[key >> 12], 1u);
    } else {
      if ((key >> 12) == hi) atomicAdd(&hist[key & (kRobustBins - 1)], 1u);
    }
  }
  __syncthreads();
  uint32_t* out = tab + (kPhase == 0 ? 0 : kRobustBins);
  for (int i = t; i < kRobustBins; i += 256) {
    const uint32_t v = hist[i];
    if (v) atomicAdd(&out[i], v);
  }
}

// The weighted MFMA trips over rows [k0, k1) of one camera's slots (the robust
// instantiation of k_linecal_rig; kk = lane >> 4, m = lane & 15): the plain
// kernel's loops on row r times sq[r - k0], its sqrt(w) -- the same kU trips'
// loads in flight before their MFMAs, the same accumulation order; trips past
// the end add exact zeros. lh and hh: the 21-column row only. (The plain
// kernel keeps its own copy of the loops: run through these helpers, its
// 21-column instantiation measured 1.5 % slower)
template <class P>
__device__ __forceinline__ void linecal_trips(const typename P::Slot* sl, const double* sq, int k0, int k1, int kk,
                                              int m, v4d& ll, v4d& lh, v4d& hh) {
  if constexpr (P::kRow <= 16) {
    constexpr int kU = 8;
    for (int base = k0; base < k1; base += 4 * kU) {
      double v[kU], q[kU];
#pragma unroll
      for (int u = 0; u < kU; u++) {  // the loads only: nothing here waits for one of them
        const int r = base + 4 * u + kk;
        v[u] = (r < k1 && m < P::kRow) ? sl[r].row[m] : 0.0;
        q[u] = r < k1 ? sq[r - k0] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kU; u++) v[u] *= q[u];
#pragma unroll
      for (int u = 0; u < kU; u++) ll = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u], v[u], ll, 0, 0, 0);
    }
  } else {
    constexpr int kHi = P::kRow - 16;  // columns of the high part
    constexpr int kU = 4;
    for (int base = k0; base < k1; base += 4 * kU) {
      double lo[kU], hi[kU], q[kU];
#pragma unroll
      for (int u = 0; u < kU; u++) {  // the loads only: nothing here waits for one of them
        const int r = base + 4 * u + kk;
        lo[u] = r < k1 ? sl[r].row[m] : 0.0;
        hi[u] = (r < k1 && m < kHi) ? sl[r].row[16 + m] : 0.0;
        q[u] = r < k1 ? sq[r - k0] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kU; u++) {
        lo[u] *= q[u];
        hi[u] *= q[u];
      }
#pragma unroll
      for (int u = 0; u < kU; u++) {
        ll = __builtin_amdgcn_mfma_f64_16x16x4f64(lo[u], lo[u], ll, 0, 0, 0);
        lh = __builtin_amdgcn_mfma_f64_16x16x4f64(lo[u], hi[u], lh, 0, 0, 0);
        hh = __builtin_amdgcn_mfma_f64_16x16x4f64(hi[u], hi[u], hh, 0, 0, 0);
      }
    }
  }
}
// the tiles' entries (kk + 4 r, m) into the camera's upper triangle; low.low and high.high are symmetric bit for bit
template <class P>
__device__ __forceinline__ void linecal_store(const v4d& ll, const v4d& lh, const v4d& hh, int kk, int m, double* sa) {
  constexpr int kHi = P::kRow - 16;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int i = kk + 4 * r;
    if (i <= m && m < P::kRow) sa[P::tri(i, m)] = ll[r];
    if constexpr (P::kRow > 16) {
      if (m < kHi) sa[P::tri(i, 16 + m)] = lh[r];
      if (i <= m && m < kHi) sa[P::tri(16 + i, 16 + m)] = hh[r];
    }
  }
}
// the code-0 rows of a camera's nc slots, in every lane of the wave
template <class P>
__device__ __forceinline__ int32_t linecal_count(const typename P::Slot* sl, int nc, int lane) {
  int32_t n = 0;
  for (int r = lane; r < nc; r += 64) n += sl[r].code == 0;
#pragma unroll
  for (int q = 32; q >= 1; q >>= 1) n += __shfl_xor(n, q, 64);
  return n;
}

// One block per view. Wave w builds M^T M of M = [J_pose | J_ext | J_int | r]
// over the n_cand slots of cameras w and w + 4 with v_mfma_f64_16x16x4f64
// (four rows per instruction; the tile's entry (i, j) is in lane (i & 3) * 16
// + j, register i >> 2). A row of at most 16 columns is one tile, eight trips'
// loads in flight. The 21 columns of Rig do not fit one tile: a lane holds
// column m of the low part (columns 0-15) and column 16 + m of the high part
// (columns 16-20, zero for m >= 5), and each group of four rows is three
// MFMAs, low.low, low.high and high.high, four trips in flight. One wave owns
// its tiles, so there is no cross-wave sum. After a barrier the block forms
// A_r and [E_r | a_r] from the tiles, thread 0 factors A_r, one thread per
// column solves Y_r = A_r^-1 [E_r | a_r] and one thread per entry forms the
// lower triangle and the last column of the view's Schur term E_r^T Y_r (what
// k_linecal_solve reads). Pass I solves nothing: it writes the accumulators
// and the counts only.
// kR (the robust rows): the block first scans the pass's second table for the
// median key (every block finds the same one) and sigma. Then, per chunk of
// kLinecalChunk candidates, wave w forms the weights of its two cameras' rows
// -- one row per lane and trip, so the 64-bit division, the FP64 division and
// the root are paid once per row, not once per MFMA lane -- and leaves sqrt(w)
// in LDS for the trips, which run on row x sqrt(w) with the plain loop's trips
// in flight and in its order (a chunk is a whole number of trips). The tiles of
// both cameras stay in registers across the chunks. n_down, n_zero and sum_w of
// a (view, camera) are per-lane sums in row order, then shuffles: a fixed order.
template <class P, bool kR = false>
__global__ __launch_bounds__(256) void k_linecal_rig(LinecalArgs a, int pass) {
  using Slot = typename P::Slot;
  __shared__ double s_acc[lc::kMaxCams * P::kAcc];
  __shared__ double s_A[36], s_L[36];
  __shared__ double s_E[6 * P::kLd], s_Y[6 * P::kLd];
  __shared__ int32_t s_pd;
  const int rig = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  if (a.st->done) return;
  const int C = a.C, nc = a.n_cand, nS = a.l.nS;
  const int kk = lane >> 4, m = lane & 15;
  if constexpr (!kR) {  // the plain loops, spelled out (see linecal_trips)
    for (int cam = wave; cam < C; cam += 4) {  // wave-uniform
      const Slot* sl = (const Slot*)a.slots + (size_t)pass * a.pass_slots + (size_t)(rig * C + cam) * nc;
      double* sa = s_acc + P::kAcc * cam;
      auto count = [&] {  // the camera's code-0 rows
        int32_t n = 0;
        for (int r = lane; r < nc; r += 64) n += sl[r].code == 0;
#pragma unroll
        for (int q = 32; q >= 1; q >>= 1) n += __shfl_xor(n, q, 64);
        if (lane == 0) a.cnt[rig * C + cam] = n;
      };
      // kU trips' loads in flight before their MFMAs (the accumulation order is
      // the plain loop's; trips past the end add exact zeros)
      if constexpr (P::kRow <= 16) {
        v4d acc = {0, 0, 0, 0};
        constexpr int kU = 8;
        for (int base = 0; base < nc; base += 4 * kU) {
          double v[kU];
#pragma unroll
          for (int u = 0; u < kU; u++) {
            const int r = base + 4 * u + kk;
            v[u] = (r < nc && m < P::kRow) ? sl[r].row[m] : 0.0;
          }
#pragma unroll
          for (int u = 0; u < kU; u++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u], v[u], acc, 0, 0, 0);
        }
        count();
#pragma unroll
        for (int r = 0; r < 4; r++) {  // entry (kk + 4 r, m) of the tile; the tile is symmetric bit for bit
          const int i = kk + 4 * r;
          if (i <= m && m < P::kRow) sa[P::tri(i, m)] = acc[r];
        }
      } else {
        constexpr int kHi = P::kRow - 16;  // columns of the high part
        v4d ll = {0, 0, 0, 0}, lh = {0, 0, 0, 0}, hh = {0, 0, 0, 0};
        constexpr int kU = 4;
        for (int base = 0; base < nc; base += 4 * kU) {
          double lo[kU], hi[kU];
#pragma unroll
          for (int u = 0; u < kU; u++) {
            const int r = base + 4 * u + kk;
            lo[u] = r < nc ? sl[r].row[m] : 0.0;
            hi[u] = (r < nc && m < kHi) ? sl[r].row[16 + m] : 0.0;
          }
#pragma unroll
          for (int u = 0; u < kU; u++) {
            ll = __builtin_amdgcn_mfma_f64_16x16x4f64(lo[u], lo[u], ll, 0, 0, 0);
            lh = __builtin_amdgcn_mfma_f64_16x16x4f64(lo[u], hi[u], lh, 0, 0, 0);
            hh = __builtin_amdgcn_mfma_f64_16x16x4f64(hi[u], hi[u], hh, 0, 0, 0);
          }
        }
        count();
#pragma unroll
        for (int r = 0; r < 4; r++) {  // entry (kk + 4 r, m) of each tile; low.low, high.high: symmetric bit for bit
          const int i = kk + 4 * r;
          if (i <= m) sa[P::tri(i, m)] = ll[r];
          if (m < kHi) sa[P::tri(i, 16 + m)] = lh[r];
          if (i <= m && m < kHi) sa[P::tri(16 + i, 16 + m)] = hh[r];
        }
      }
    }
  } else {
    __shared__ double s_sq[lc::kMaxCams * kLinecalChunk];  // first the table's scan: 16 KB of its 34
    __shared__ uint32_t s_wsum[4], s_sel[2];
    static_assert(sizeof(s_sq) >= sizeof(uint32_t) * kRobustBins, "the table's scan fits");
    static_assert(kLinecalChunk % 32 == 0, "a chunk is a whole number of trips");
    const uint32_t* tab = a.r.tab + (size_t)pass * kLinecalTab;
    const uint32_t n_call = tab[2 * kRobustBins];
    uint32_t median = 0;
    if (n_call > 0) {  // block-uniform
      uint32_t* hist = (uint32_t*)s_sq;
      for (int i = t; i < kRobustBins; i += 256) hist[i] = tab[kRobustBins + i];
      __syncthreads();
      uint32_t rest;
      const uint32_t lo = robust_select(hist, tab[2 * kRobustBins + 2], s_wsum, s_sel, &rest);
      median = (tab[2 * kRobustBins + 1] << 12) | lo;
    }  // robust_select ends behind a barrier: s_sq is free
    const double sigma = rfn::robust_scale(median, a.r.rb.scale_floor);
    if (rig == 0 && t == 0) a.r.tab[(size_t)pass * kLinecalTab + 2 * kRobustBins + 3] = median;  // k_linecal_solve's
    const size_t slot0 = (size_t)pass * a.pass_slots + (size_t)rig * C * nc;
    v4d ll[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, lh[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    v4d hh[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    int32_t n_down[2] = {0, 0}, n_zero[2] = {0, 0};
    double sum_w[2] = {0.0, 0.0};
    for (int k0 = 0; k0 < nc; k0 += kLinecalChunk) {  // block-uniform
      const int k1 = min(k0 + kLinecalChunk, nc);
      // every key of the chunk the lane weighs, both cameras', in flight before the first weight
      constexpr int kL = (kLinecalChunk + 63) / 64;
      uint32_t key[2][kL];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int cam = wave + 4 * h;
        const uint32_t* kp = a.r.keys + slot0 + (size_t)cam * nc;
#pragma unroll
        for (int u = 0; u < kL; u++) {
          const int k = k0 + lane + 64 * u;
          key[h][u] = (cam < C && k < k1) ? kp[k] : kNoKey;
        }
      }
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int cam = wave + 4 * h;
        if (cam < C) {  // wave-uniform
          double* wp = a.r.weights ? a.r.weights + slot0 + (size_t)cam * nc : nullptr;
#pragma unroll
          for (int u = 0; u < kL; u++) {  // the lane's rows in ascending order
            const int k = k0 + lane + 64 * u;
            if (k >= k1) continue;
            double w = 0.0;
            if (key[h][u] != kNoKey) {
              w = rfn::robust_weight(key[h][u], a.r.rb, sigma);
              n_down[h] += w < 1.0;
              n_zero[h] += w == 0.0;
              sum_w[h] += w;
            }
            s_sq[cam * kLinecalChunk + (k - k0)] = sqrt(w);  // k - k0 < kLinecalChunk, cam < 8: inside s_sq
            if (wp) wp[k] = w;  // the record: every slot of the pass has one writer
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int cam = wave + 4 * h;
        if (cam < C)
          linecal_trips<P>((const Slot*)a.slots + slot0 + (size_t)cam * nc, s_sq + cam * kLinecalChunk, k0, k1, kk, m,
                           ll[h], lh[h], hh[h]);
      }
      __syncthreads();  // the next chunk overwrites s_sq
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int cam = wave + 4 * h;
      if (cam < C) {
        const int32_t n = linecal_count<P>((const Slot*)a.slots + slot0 + (size_t)cam * nc, nc, lane);
        int32_t d = n_down[h], z = n_zero[h];
        double w = sum_w[h];
#pragma unroll
        for (int q = 32; q >= 1; q >>= 1) {
          d += __shfl_xor(d, q, 64);
          z += __shfl_xor(z, q, 64);
          w += __shfl_xor(w, q, 64);
        }
        if (lane == 0) {
          a.cnt[rig * C + cam] = n;
          a.r.cells[rig * C + cam] = lc::RobustCell{d, z, w};
        }
        linecal_store<P>(ll[h], lh[h], hh[h], kk, m, s_acc + P::kAcc * cam);
      }
    }
  }
  __syncthreads();
  for (int e = t; e < C * P::kAcc; e += 256) {
    const double v = s_acc[e];
    a.acc[(size_t)rig * C * P::kAcc + e] = v;
    if (a.recAcc) a.recAcc[((size_t)pass * a.N + rig) * C * P::kAcc + e] = v;
  }
  if (pass >= a.I) return;  // block-uniform
  if (t < 36) s_A[t] = P::view_A(s_acc, C, t / 6, t % 6, a.lambda);
  for (int e = t; e < 6 * (nS + 1); e += 256) {
    const int k = e / (nS + 1), j = e % (nS + 1);
    s_E[P::kLd * k + j] = P::view_rhs(s_acc, C, a.l, k, j);
  }
  __syncthreads();
  if (t == 0) {
    const int32_t ok = cal::chol6(s_A, s_L) ? 1 : 0;
    s_pd = ok;
    a.pd[rig] = ok;
  }
  __syncthreads();
  if (!s_pd) return;  // k_linecal_solve stops the call: Y_r and the term are not read
  if (t <= nS) P::view_solve(s_L, s_E + t, s_Y + t);
  __syncthreads();
  for (int e = t; e < 6 * (nS + 1); e += 256) {
    const int k = e / (nS + 1), j = e % (nS + 1);
    a.Y[((size_t)rig * 6 + k) * P::kLd + j] = s_Y[P::kLd * k + j];
  }
  for (int e = t; e < nS * (nS + 1); e += 256) {
    const int i = e / (nS + 1), j = e % (nS + 1);
    if (j <= i || j == nS) a.Wt[((size_t)rig * P::kMaxS + i) * P::kLd + j] = P::schur_entry(s_E, s_Y, i, j);
  }
}

// One block. The figures of the pass and its gates; one thread per entry sums
// the views' Schur terms in view order into [S | s]; the left-looking Cholesky
// of S with one barrier per column (every entry by the sequential formula, the
// pivot recomputed by every thread, so the values do not depend on which
// thread computes them and the exit is block-uniform; L's strict lower
// triangle overwrites S's in place, its diagonal is kept apart); eps by thread
// 0; one thread per camera of free_int forms the updated intrinsics and the
// DIVERGED test; then one thread per view forms delta_r from the stored Y_r
// and updates T_r, one per camera of free_ext updates E_c, one per camera of
// free_int stores its intrinsics. [S | s] is the kernel's dynamic LDS (nS rows
// of kLd): Rig's largest, 106 x 107 doubles, is past the static LDS limit. The
// pass record (poses, extrinsics, intrinsics) is written here. kR (the robust
// rows): one thread per view and one per camera sum the cells (camera order,
// view order); the two starved gates also count the rows with w > 0; thread 0
// sums the views' figures in view order into the pass's stats (lc::robust_tally's
// orders), and the per-view and per-camera figures of the pass overwrite the
// last pass's.
template <class P, bool kR = false>
__global__ __launch_bounds__(256) void k_linecal_solve(LinecalArgs a, int pass) {
  extern __shared__ double lcs_S[];  // nS x kLd
  __shared__ double s_rr[lc::kMaxViews * lc::kMaxCams];
  __shared__ double s_d[P::kMaxS], s_eps[P::kMaxS], s_y[P::kMaxS];
  __shared__ double s_next[P::kInt ? lc::kMaxCams : 1][lc::kPi];
  __shared__ int32_t s_view[lc::kMaxViews], s_vpd[lc::kMaxViews], s_camn[lc::kMaxCams], s_ok[lc::kMaxCams], s_stop;
  __shared__ double s_vsw[kR ? lc::kMaxViews : 1];
  __shared__ int32_t s_vdown[kR ? lc::kMaxViews : 1], s_vzero[kR ? lc::kMaxViews : 1], s_czero[kR ? lc::kMaxCams : 1];
  double* s_S = lcs_S;
  LinecalState& S = *a.st;
  if (S.done) return;
  const int t = threadIdx.x, N = a.N, C = a.C, nS = a.l.nS, Fe = a.l.Fe, Fi = a.l.Fi;
  const uint32_t free_any = a.free_ext | a.free_int;
  for (int e = t; e < N * 16; e += 256) a.recT[(size_t)pass * N * 16 + e] = a.T[e];
  if constexpr (P::kExt)
    for (int e = t; e < C * 16; e += 256) a.recE[(size_t)pass * C * 16 + e] = S.res.T_base_cam[e >> 4][e & 15];
  if constexpr (P::kInt)
    for (int e = t; e < C * lc::kPi; e += 256) {
      const int c = e >> 3, q = e & 7;
      a.recKD[(size_t)pass * C * lc::kPi + e] = q < 4 ? S.res.K[c][q] : S.res.D[c][q - 4];
    }
  for (int e = t; e < N * C; e += 256) s_rr[e] = a.acc[(size_t)P::kAcc * e + (P::kAcc - 1)];
  if (t < N) {  // N <= 256 = the block
    int32_t n = 0;
    for (int c = 0; c < C; c++) n += a.cnt[t * C + c];
    s_view[t] = n;
    s_vpd[t] = pass < a.I ? a.pd[t] : 1;
    if constexpr (kR) {
      int32_t d = 0, z = 0;
      double w = 0.0;
      for (int c = 0; c < C; c++) {
        const lc::RobustCell q = a.r.cells[t * C + c];
        d += q.n_down;
        z += q.n_zero;
        w += q.sum_w;
      }
      s_vdown[t] = d;
      s_vzero[t] = z;
      s_vsw[t] = w;
      a.r.stats->n_obs_view[t] = n;
      a.r.stats->n_zero_view[t] = z;
      a.r.stats->sum_w_view[t] = w;
    }
  }
  if (t < C) {
    int32_t n = 0;
    for (int r = 0; r < N; r++) n += a.cnt[r * C + t];
    s_camn[t] = n;
    if constexpr (kR) {
      int32_t z = 0;
      double w = 0.0;
      for (int r = 0; r < N; r++) {
        const lc::RobustCell q = a.r.cells[r * C + t];
        z += q.n_zero;
        w += q.sum_w;
      }
      s_czero[t] = z;
      a.r.stats->n_zero_cam[t] = z;
      a.r.stats->sum_w_cam[t] = w;
    }
  }
  __syncthreads();
  if (t == 0) {
    int32_t n_obs = 0, starved = 0, singular = 0;
    for (int r = 0; r < N; r++) {
      n_obs += s_view[r];
      starved |= s_view[r] < a.min_obs;
      singular |= !s_vpd[r];
    }
    double rr = 0.0;
    for (int e = 0; e < N * C; e++) rr += s_rr[e];  // (view, camera) order
    for (int c = 0; c < C; c++) {
      S.res.n_obs_cam[pass][c] = s_camn[c];
      if (free_any >> c & 1u) starved |= s_camn[c] < a.min_obs_cam;
    }
    S.res.n_obs[pass] = n_obs;
    S.res.rms[pass] = n_obs > 0 ? sqrt(rr / (double)n_obs) : 0.0;
    if constexpr (kR) {
      int32_t down = 0, zero = 0;
      double sw = 0.0;
      for (int r = 0; r < N; r++) {
        down += s_vdown[r];
        zero += s_vzero[r];
        sw += s_vsw[r];
        starved |= s_view[r] - s_vzero[r] < a.min_obs;
      }
      for (int c = 0; c < C; c++)
        if (free_any >> c & 1u) starved |= s_camn[c] - s_czero[c] < a.min_obs_cam;
      const uint32_t median = a.r.tab[(size_t)pass * kLinecalTab + 2 * kRobustBins + 3];
      mantis_calib_robust_stats& st = *a.r.stats;
      st.median_key[pass] = median;
      st.scale[pass] = rfn::robust_scale(median, a.r.rb.scale_floor);
      st.n_down[pass] = down;
      st.n_zero[pass] = zero;
      st.sum_w[pass] = sw;
    }
    int32_t stop = 0;
    if (pass >= a.I) {
      stop = 1;
    } else if (starved) {
      S.res.status = lc::kStarved;
      stop = 1;
    } else if (singular) {
      S.res.status = lc::kSingular;
      stop = 1;
    }
    s_stop = stop;
    if (stop) S.done = 1;
  }
  __syncthreads();
  if (s_stop) return;
  for (int e = t; e < nS * (nS + 1); e += 256) {
    const int i = e / (nS + 1), j = e % (nS + 1);
    if (j <= i || j == nS)  // the lower triangle and s: what the factorization and the solve read
      s_S[P::kLd * i + j] = P::reduced_entry(a.acc, a.Wt, N, C, a.l, i, j, a.lambda, a.param_mask);
  }
  __syncthreads();
  bool bad = false;
  for (int j = 0; j < nS; j++) {
    const double d = P::cholS_pivot(s_S, s_S, j);
    if (!(d > 0)) {
      bad = true;
      break;
    }
    const double ljj = sqrt(d);
    const int i = j + 1 + t;
    if (t == 0) s_d[j] = ljj;
    if (i < nS) s_S[P::kLd * i + j] = P::cholS_below(s_S, s_S, i, j, ljj);
    __syncthreads();
  }
  if (bad) {
    if (t == 0) {
      S.res.status = lc::kSingular;
      S.done = 1;
    }
    return;
  }
  if (t == 0) P::cholS_solve(s_S, s_d, nS, s_S + nS, P::kLd, s_y, s_eps);
  __syncthreads();
  const double* epi = s_eps + (P::kExt ? lc::kPe * Fe : 0);
  if constexpr (P::kInt) {
    if (t < Fi) {
      const int cam = a.l.fi[t];
      double th[lc::kPi], x[lc::kPi], nx[lc::kPi];
      icalib::cam_to(icalib::cam_of(S.res.K[cam], S.res.D[cam]), th);
#pragma unroll
      for (int e = 0; e < lc::kPi; e++) x[e] = epi[lc::kPi * t + e];
      s_ok[t] = icalib::param_update(th, x, a.param_mask, nx) ? 1 : 0;
#pragma unroll
      for (int e = 0; e < lc::kPi; e++) s_next[t][e] = nx[e];
    }
    __syncthreads();
    bool diverged = false;
    for (int f = 0; f < Fi; f++) diverged = diverged || !s_ok[f];  // block-uniform
    if (diverged) {
      if (t == 0) {
        S.res.status = lc::kDiverged;
        S.done = 1;
      }
      return;
    }
  }
  if (t < N) {
    double d6[6], T[16];
    P::pose_delta(a.Y + (size_t)t * 6 * P::kLd, s_eps, nS, d6);
#pragma unroll
    for (int e = 0; e < 16; e++) T[e] = a.T[16 * t + e];
    cal::right_update(T, d6);
#pragma unroll
    for (int e = 0; e < 16; e++) a.T[16 * t + e] = T[e];
  }
  if constexpr (P::kExt) {
    if (t < Fe) {
      const int cam = a.l.fe[t];
      double x[6], E[16];
#pragma unroll
      for (int e = 0; e < 6; e++) x[e] = s_eps[lc::kPe * t + e];
#pragma unroll
      for (int e = 0; e < 16; e++) E[e] = S.res.T_base_cam[cam][e];
      cal::right_update(E, x);
#pragma unroll
      for (int e = 0; e < 16; e++) S.res.T_base_cam[cam][e] = E[e];
#pragma unroll
      for (int e = 0; e < 6; e++) S.res.delta_ext[pass][cam][e] = x[e];
    }
  }
  if constexpr (P::kInt) {
    if (t < Fi) {
      const int cam = a.l.fi[t];
#pragma unroll
      for (int e = 0; e < 4; e++) {
        S.res.K[cam][e] = s_next[t][e];
        S.res.D[cam][e] = s_next[t][4 + e];
      }
#pragma unroll
      for (int e = 0; e < lc::kPi; e++)
        S.res.delta_int[pass][cam][e] = (a.param_mask >> e & 1u) ? epi[lc::kPi * t + e] : 0.0;
    }
  }
  if (t == 0) S.res.iterations_run = pass + 1;
}

}  // namespace mk

namespace {

namespace cal = mk::calib;
namespace lc = mk::linecal;

// what an entry point calls itself: the prefix of its errors, its record, its stage labels
struct LinecalNames {
  const char *prefix, *call, *obs, *rig, *solve, *hist;
};
constexpr LinecalNames kCalibNames{"calib", "calibration", "calib_obs/k_calib_obs", "calib_rig/k_calib_rig",
                                   "calib_solve/k_calib_solve", "calib_hist/k_calib_hist"};
constexpr LinecalNames kIcalibNames{"icalib", "intrinsic calibration", "icalib_obs/k_icalib_obs",
                                    "icalib_rig/k_icalib_rig", "icalib_solve/k_icalib_solve",
                                    "icalib_hist/k_icalib_hist"};
constexpr LinecalNames kRcalibNames{"rcalib", "rig calibration", "rcalib_obs/k_rcalib_obs", "rcalib_rig/k_rcalib_rig",
                                    "rcalib_solve/k_rcalib_solve", "rcalib_hist/k_rcalib_hist"};

mantis_status linecal_fail(Ctx* c, const LinecalNames& nm, const char* what) { return line_fail(c, nm.prefix, what); }

// workspaces for a call of N views x C cameras; robust: the switch is on
template <class P>
mantis_status linecal_workspace(Ctx* c, Ctx::Linecal& k, int N, int C, int I, bool record, bool robust) {
  const size_t slots = (record ? (size_t)I + 1 : 1) * N * C * std::max(c->rf.n_cand, 1);
  const size_t racc = record ? (size_t)(I + 1) * N * C * P::kAcc : 0;
  const size_t rkeys = robust ? slots : 0, rweights = robust && record ? slots : 0;
  const size_t slot_bytes = slots * sizeof(typename P::Slot);
  if (N > k.view_cap || slot_bytes > k.d_slots.capacity() || racc > k.d_recAcc.capacity() ||
      rkeys > k.d_rkeys.capacity() || rweights > k.d_rweights.capacity() || (robust && N > k.rcell_cap))
    HIP_OK(hipStreamSynchronize(c->s));
  if (N > k.view_cap) {
    k.view_cap = 0;
    const size_t n = (size_t)N, nc = n * lc::kMaxCams;
    // pinned: the state, the poses, the accumulators, the counts
    const size_t hb = sizeof(mk::LinecalState) + sizeof(double) * (16 * n + P::kAcc * nc) + sizeof(int32_t) * nc;
    if (k.d_state.alloc(c, 1) || k.d_T.alloc(c, 16 * n) || k.d_acc.alloc(c, P::kAcc * nc) || k.d_cnt.alloc(c, nc) ||
        k.d_Y.alloc(c, n * 6 * P::kLd) || k.d_Wt.alloc(c, n * P::kMaxS * P::kLd) || k.d_pd.alloc(c, n) ||
        k.d_recT.alloc(c, (size_t)(rfn::kMaxIterations + 1) * 16 * n) ||
        (P::kExt && k.d_recE.alloc(c, (size_t)(rfn::kMaxIterations + 1) * 16 * lc::kMaxCams)) ||
        (P::kInt && k.d_recKD.alloc(c, (size_t)(rfn::kMaxIterations + 1) * lc::kPi * lc::kMaxCams)) ||
        k.h_state.alloc(c, hb))
      return MANTIS_ERR_OOM;
    k.view_cap = N;
  }
  if (k.d_slots.grow(c, slot_bytes) || k.d_recAcc.grow(c, racc) || k.d_rkeys.grow(c, rkeys) ||
      k.d_rweights.grow(c, rweights))
    return MANTIS_ERR_OOM;
  if (robust && N > k.rcell_cap) {
    k.rcell_cap = 0;
    if (k.d_rcells.alloc(c, (size_t)N * lc::kMaxCams) ||
        k.d_rtab.alloc(c, (size_t)(rfn::kMaxIterations + 1) * mk::kLinecalTab) || k.d_rstats.alloc(c, 1) ||
        k.h_rstats.alloc(c, sizeof(mantis_calib_robust_stats) + sizeof(lc::RobustCell) * (size_t)N * lc::kMaxCams))
      return MANTIS_ERR_OOM;
    k.rcell_cap = N;
  }
  return MANTIS_OK;
}

// One call on validated arguments: fe / fi / pm are the masks of the blocks the
// problem has (0 for the others). res: the call's working state, concluded.
// kR: the robust rows of c->calib_robust (loss > 0).
template <class P, bool kR>
mantis_status linecal_run(Ctx* c, Ctx::Linecal& k, const LinecalNames& nm, const mantis_image* cams, int32_t N,
                          int32_t C, const double* T_in, const mantis_refine_params* p, uint32_t fe, uint32_t fi,
                          uint32_t pm, int32_t min_obs_cam, double* T_out, mantis_rcalib_result* res) {
  const int I = p->iterations, n = N * C;
  k.rigs = 0;  // no record until this call has finished
  // [S | s] is k_linecal_solve's dynamic LDS; beside the kernel's static arrays
  // (under 20 KB, under 24 KB with the robust rows) only Rig's largest system
  // passes 64 KB and has to be asked for, once per instantiation
  constexpr bool kAskLds = sizeof(double) * P::kMaxS * P::kLd + (kR ? 24 : 20) * 1024 > 64 * 1024;
  if constexpr (kAskLds) {
    if (!k.lds_asked[kR]) {
      k.lds_asked[kR] = true;
      k.lds_ok[kR] = hipFuncSetAttribute((const void*)mk::k_linecal_solve<P, kR>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)(sizeof(double) * P::kMaxS * P::kLd)) == hipSuccess;
    }
    if (!k.lds_ok[kR]) {
      c->err = "rcalib: the device refused k_rcalib_solve's dynamic LDS";
      return MANTIS_ERR_STATE;
    }
  }
  if (mantis_status e = refine_flags(c, p->landmark_pitch)) return e;
  if (mantis_status e = linecal_workspace<P>(c, k, N, C, I, p->record != 0, kR)) return e;
  const int nc = c->rf.n_cand;

  mk::LinecalState* h_st = (mk::LinecalState*)k.h_state.get();
  mantis_calib_robust_stats* h_rstats = (mantis_calib_robust_stats*)k.h_rstats.get();  // null with the robust rows never on
  double* h_T = (double*)(h_st + 1);
  double* h_acc = h_T + 16 * (size_t)k.view_cap;
  int32_t* h_cnt = (int32_t*)(h_acc + (size_t)P::kAcc * k.view_cap * lc::kMaxCams);
  std::memset(h_st, 0, sizeof(*h_st));
  h_st->res.n_cand = nc;
  h_st->res.n_rigs = N;
  h_st->res.n_cams = C;
  h_st->res.free_ext = (int32_t)fe;
  h_st->res.free_int = (int32_t)fi;
  h_st->res.param_mask = (int32_t)pm;
  for (int q = 0; q < C; q++) {
    double th[lc::kPi];
    mk::icalib::cam_to(cam_from(cams[q]), th);  // K rounded to float, D as given
    for (int e = 0; e < 4; e++) {
      h_st->res.K[q][e] = th[e];
      h_st->res.D[q][e] = th[4 + e];
    }
    std::memcpy(h_st->res.T_base_cam[q], cams[q].T_base_cam, sizeof(double) * 16);
  }
  std::memcpy(h_T, T_in, sizeof(double) * 16 * (size_t)N);

  int W, H;
  mantis_status st = stage_frames(c, cams, n, W, H);
  if (st != MANTIS_OK) return st;
  HIP_OK(hipMemcpyAsync(k.d_state, h_st, mk::kLinecalStateBytes, hipMemcpyHostToDevice, c->s));
  HIP_OK(hipMemcpyAsync(k.d_T, h_T, sizeof(double) * 16 * (size_t)N, hipMemcpyHostToDevice, c->s));

  mk::LinecalArgs a{};
  a.cand = c->rf.d_cand;
  a.st = (mk::LinecalState*)k.d_state;
  a.T = k.d_T;
  a.slots = k.d_slots;
  a.acc = k.d_acc;
  a.recAcc = p->record ? k.d_recAcc : nullptr;
  a.cnt = k.d_cnt;
  a.Y = k.d_Y;
  a.Wt = k.d_Wt;
  a.pd = k.d_pd;
  a.recT = k.d_recT;
  a.recE = k.d_recE;
  a.recKD = k.d_recKD;
  a.pass_slots = p->record ? (size_t)n * nc : 0;
  a.C = C;
  a.n_cand = nc;
  a.I = I;
  a.N = N;
  a.min_obs = p->min_obs;
  a.min_obs_cam = min_obs_cam;
  a.free_ext = fe;
  a.free_int = fi;
  a.param_mask = pm;
  P::layout(fe, fi, C, a.l);
  a.win = rfn::Window{p->half_window, p->white_thresh, p->min_weight, 0};
  a.lambda = p->lambda;
  if constexpr (kR) {
    const mantis_refine_robust_params& rp = c->calib_robust;
    a.r.keys = k.d_rkeys;
    a.r.weights = p->record ? k.d_rweights : nullptr;
    a.r.tab = k.d_rtab;
    a.r.cells = (lc::RobustCell*)k.d_rcells;
    a.r.stats = k.d_rstats;
    a.r.rb = rfn::Robust{rp.loss, 0, rp.tuning, rp.scale_floor};
    // the tables of every pass of this call and the stats start from zero: the histogram launches only add
    HIP_OK(hipMemsetAsync(k.d_rtab, 0, sizeof(uint32_t) * (size_t)(I + 1) * mk::kLinecalTab, c->s));
    HIP_OK(hipMemsetAsync(k.d_rstats, 0, sizeof(mantis_calib_robust_stats), c->s));
  }
  const size_t solve_lds = sizeof(double) * (size_t)a.l.nS * P::kLd;
  const Landmarks L = lmk_of(c);
  mark(c, "start");
  const dim3 grid((nc + mk::kRefineCands - 1) / mk::kRefineCands, C, N);
  for (int pass = 0; pass <= I; pass++) {
    if (nc > 0) {
      mk::k_linecal_obs<P, kR><<<grid, 256, 0, c->s>>>(c->d_frames, L, a, pass);
      HIP_OK(hipGetLastError());
    }
    mark(c, nm.obs);
    if constexpr (kR) {
      mk::k_linecal_hist<0><<<N, 256, 0, c->s>>>(a, pass);
      HIP_OK(hipGetLastError());
      mark(c, nm.hist);
      mk::k_linecal_hist<1><<<N, 256, 0, c->s>>>(a, pass);
      HIP_OK(hipGetLastError());
      mark(c, nm.hist);
    }
    mk::k_linecal_rig<P, kR><<<N, 256, 0, c->s>>>(a, pass);
    HIP_OK(hipGetLastError());
    mark(c, nm.rig);
    mk::k_linecal_solve<P, kR><<<1, 256, solve_lds, c->s>>>(a, pass);
    HIP_OK(hipGetLastError());
    mark(c, nm.solve);
  }
  if constexpr (kR) {  // the stats, and behind them the cells of the last pass run (for the gate)
    HIP_OK(hipMemcpyAsync(h_rstats, k.d_rstats, sizeof(mantis_calib_robust_stats), hipMemcpyDeviceToHost, c->s));
    HIP_OK(hipMemcpyAsync(h_rstats + 1, k.d_rcells, sizeof(lc::RobustCell) * (size_t)n, hipMemcpyDeviceToHost, c->s));
  }
  HIP_OK(hipMemcpyAsync(h_st, k.d_state, mk::kLinecalStateBytes, hipMemcpyDeviceToHost, c->s));
  HIP_OK(hipMemcpyAsync(h_T, k.d_T, sizeof(double) * 16 * (size_t)N, hipMemcpyDeviceToHost, c->s));
  HIP_OK(hipMemcpyAsync(h_acc, k.d_acc, sizeof(double) * P::kAcc * (size_t)n, hipMemcpyDeviceToHost, c->s));
  HIP_OK(hipMemcpyAsync(h_cnt, k.d_cnt, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->s));
  HIP_OK(wait_stream(c, n));
  finish_profile(c);
  k.rec_loss = kR ? c->calib_robust.loss : 0;
  if constexpr (kR) {
    std::vector<int32_t> pos((size_t)n);  // the rows with w > 0 of the last pass run
    lc::robust_pos((const lc::RobustCell*)(h_rstats + 1), h_cnt, n, pos.data());
    P::conclude(h_acc, h_cnt, N, C, fe, fi, pm, p->min_obs, min_obs_cam, p->max_rms, h_st->res, pos.data());
    h_rstats->loss = c->calib_robust.loss;
    h_rstats->kind = P::kExt && P::kInt ? lc::kKindRig : P::kInt ? lc::kKindInt : lc::kKindExt;
    h_rstats->n_rigs = N;
    h_rstats->n_cams = C;
  } else {
    P::conclude(h_acc, h_cnt, N, C, fe, fi, pm, p->min_obs, min_obs_cam, p->max_rms, h_st->res);
  }
  *res = h_st->res;
  std::memcpy(T_out, h_T, sizeof(double) * 16 * (size_t)N);
  k.rigs = N;
  k.C = C;
  k.record = p->record;
  k.cands = nc;
  k.runs = h_st->res.iterations_run;
  return MANTIS_OK;
}

// One record of the last call of its kind: T_base_cam / KD only from a problem that recorded them
template <class P>
mantis_status linecal_record(Ctx* c, const Ctx::Linecal& k, const LinecalNames& nm, int32_t rig, int32_t pass,
                             double* T_w_b, double* T_base_cam, double* KD, int32_t* codes, int32_t* Sw, int32_t* Skw,
                             double* rows, double* acc) {
  using Slot = typename P::Slot;
  if (!k.rigs || !k.record) {
    c->err = std::string(nm.prefix) + " record: the last " + nm.call + " kept none (params.record = 1)";
    return MANTIS_ERR_STATE;
  }
  if (rig < 0 || rig >= k.rigs || pass < 0 || pass > k.runs)
    return linecal_fail(c, nm, "record: rig or pass out of range (0 .. iterations_run)");
  const size_t ns = (size_t)k.C * k.cands, pr = (size_t)pass * k.rigs + rig;
  if (T_w_b) HIP_OK(hipMemcpy(T_w_b, k.d_recT + pr * 16, sizeof(double) * 16, hipMemcpyDeviceToHost));
  if (P::kExt && T_base_cam)
    HIP_OK(hipMemcpy(T_base_cam, k.d_recE + (size_t)pass * k.C * 16, sizeof(double) * 16 * k.C, hipMemcpyDeviceToHost));
  if (P::kInt && KD)
    HIP_OK(hipMemcpy(KD, k.d_recKD + (size_t)pass * k.C * lc::kPi, sizeof(double) * lc::kPi * k.C, hipMemcpyDeviceToHost));
  if (acc)
    HIP_OK(hipMemcpy(acc, k.d_recAcc + pr * k.C * P::kAcc, sizeof(double) * P::kAcc * k.C, hipMemcpyDeviceToHost));
  return slots_scatter<Slot, P::kRow>(c, (const Slot*)k.d_slots.get() + pr * ns, ns, codes, Sw, Skw, rows);
}

// ---- the three entry points: each its own validation, then the one driver ----
mantis_status calib_impl(Ctx* c, const mantis_image* cams, int32_t N, int32_t C, const double* T_in,
                         const mantis_refine_params* p, const mantis_calib_params* cp, double* T_out,
                         mantis_calib_result* out) {
  auto calib_fail = [](Ctx* c, const char* what) { return linecal_fail(c, kCalibNames, what); };
  if (!cams || !T_in || !p || !cp || !T_out || !out) return calib_fail(c, "null argument");
  if (cp->struct_size != (int32_t)sizeof(mantis_calib_params)) return calib_fail(c, "calib_params.struct_size mismatch");
  if (N > lc::kMaxViews) return calib_fail(c, "n_rigs exceeds 256");
  if (mantis_status e = refine_check(c, cams, N, C, p)) return e;
  if (C < 2) return calib_fail(c, "cams_per_rig must be >= 2 (one camera held, one free)");
  const uint32_t fm = (uint32_t)cp->free_cams, all = (1u << C) - 1u;
  if (fm & ~all) return calib_fail(c, "free_cams has a bit at or above cams_per_rig");
  if (fm == 0) return calib_fail(c, "free_cams names no camera");
  if (fm == all) return calib_fail(c, "free_cams names every camera: one must be held");
  if (cp->min_obs_cam < 6) return calib_fail(c, "min_obs_cam must be >= 6");
  for (size_t i = 0; i < 16 * (size_t)N; i++)
    if (!std::isfinite(T_in[i])) return calib_fail(c, "T_w_b_in is not finite");
  for (int k = 0; k < C; k++)
    for (int e = 0; e < 16; e++)
      if (!std::isfinite(cams[k].T_base_cam[e])) return calib_fail(c, "T_base_cam is not finite");
  for (int r = 1; r < N; r++)
    for (int k = 0; k < C; k++)
      if (std::memcmp(cams[r * C + k].T_base_cam, cams[k].T_base_cam, sizeof(cams[k].T_base_cam)) != 0)
        return calib_fail(c, "T_base_cam of a view differs from view 0's");
  mantis_rcalib_result res;
  const auto run = c->calib_robust.loss ? linecal_run<lc::Ext, true> : linecal_run<lc::Ext, false>;
  if (mantis_status e = run(c, c->cb, kCalibNames, cams, N, C, T_in, p, fm, 0u, 0u, cp->min_obs_cam, T_out, &res))
    return e;
  lc::narrow(res, *out);
  return MANTIS_OK;
}

// the checks the two calibrations with intrinsics share word for word: finite inputs, one rig in every view
mantis_status linecal_check_cams(Ctx* c, const LinecalNames& nm, const mantis_image* cams, int32_t N, int32_t C,
                                 const double* T_in) {
  for (size_t i = 0; i < 16 * (size_t)N; i++)
    if (!std::isfinite(T_in[i])) return linecal_fail(c, nm, "T_w_b_in is not finite");
  for (int k = 0; k < C; k++) {
    for (int e = 0; e < 16; e++)
      if (!std::isfinite(cams[k].T_base_cam[e])) return linecal_fail(c, nm, "T_base_cam is not finite");
    for (int e = 0; e < 9; e++)
      if (!std::isfinite(cams[k].K[e])) return linecal_fail(c, nm, "K is not finite");
    for (int e = 0; e < 4; e++)
      if (!std::isfinite(cams[k].D[e])) return linecal_fail(c, nm, "D is not finite");
    const mk::Cam cm = cam_from(cams[k]);
    if (!(cm.fx > 0) || !(cm.fy > 0) || !std::isfinite(cm.fx) || !std::isfinite(cm.fy) || !std::isfinite(cm.cx) ||
        !std::isfinite(cm.cy))
      return linecal_fail(c, nm, "K: fx and fy must be > 0 and finite as floats");
  }
  for (int r = 1; r < N; r++)
    for (int k = 0; k < C; k++) {
      const mantis_image &v = cams[r * C + k], &v0 = cams[k];
      if (std::memcmp(v.T_base_cam, v0.T_base_cam, sizeof(v0.T_base_cam)) != 0)
        return linecal_fail(c, nm, "T_base_cam of a view differs from view 0's");
      if (std::memcmp(v.K, v0.K, sizeof(v0.K)) != 0) return linecal_fail(c, nm, "K of a view differs from view 0's");
      if (std::memcmp(v.D, v0.D, sizeof(v0.D)) != 0) return linecal_fail(c, nm, "D of a view differs from view 0's");
    }
  return MANTIS_OK;
}

mantis_status icalib_impl(Ctx* c, const mantis_image* cams, int32_t N, int32_t C, const double* T_in,
                          const mantis_refine_params* p, const mantis_icalib_params* ip, double* T_out,
                          mantis_icalib_result* out) {
  auto icalib_fail = [](Ctx* c, const char* what) { return linecal_fail(c, kIcalibNames, what); };
  if (!cams || !T_in || !p || !ip || !T_out || !out) return icalib_fail(c, "null argument");
  if (ip->struct_size != (int32_t)sizeof(mantis_icalib_params))
    return icalib_fail(c, "icalib_params.struct_size mismatch");
  if (N > lc::kMaxViews) return icalib_fail(c, "n_rigs exceeds 256");
  if (mantis_status e = refine_check(c, cams, N, C, p)) return e;
  const uint32_t fm = (uint32_t)ip->free_cams, all = (1u << C) - 1u;
  if (fm & ~all) return icalib_fail(c, "free_cams has a bit at or above cams_per_rig");
  if (fm == 0) return icalib_fail(c, "free_cams names no camera");
  if (ip->param_mask < 1 || ip->param_mask > 0xFF) return icalib_fail(c, "param_mask outside 1..0xFF");
  if (ip->min_obs_cam < 8) return icalib_fail(c, "min_obs_cam must be >= 8");
  if (mantis_status e = linecal_check_cams(c, kIcalibNames, cams, N, C, T_in)) return e;
  mantis_rcalib_result res;
  const auto run = c->calib_robust.loss ? linecal_run<lc::Int, true> : linecal_run<lc::Int, false>;
  if (mantis_status e = run(c, c->ib, kIcalibNames, cams, N, C, T_in, p, 0u, fm, (uint32_t)ip->param_mask,
                            ip->min_obs_cam, T_out, &res))
    return e;
  lc::narrow(res, *out);
  return MANTIS_OK;
}

mantis_status rcalib_impl(Ctx* c, const mantis_image* cams, int32_t N, int32_t C, const double* T_in,
                          const mantis_refine_params* p, const mantis_rcalib_params* rp, double* T_out,
                          mantis_rcalib_result* out) {
  auto rcalib_fail = [](Ctx* c, const char* what) { return linecal_fail(c, kRcalibNames, what); };
  if (!cams || !T_in || !p || !rp || !T_out || !out) return rcalib_fail(c, "null argument");
  if (rp->struct_size != (int32_t)sizeof(mantis_rcalib_params))
    return rcalib_fail(c, "rcalib_params.struct_size mismatch");
  if (N > lc::kMaxViews) return rcalib_fail(c, "n_rigs exceeds 256");
  if (mantis_status e = refine_check(c, cams, N, C, p)) return e;
  if (C < 2) return rcalib_fail(c, "cams_per_rig must be >= 2 (one extrinsic held, one free)");
  const uint32_t fe = (uint32_t)rp->free_ext, fi = (uint32_t)rp->free_int, all = (1u << C) - 1u;
  if (fe & ~all) return rcalib_fail(c, "free_ext has a bit at or above cams_per_rig");
  if (fi & ~all) return rcalib_fail(c, "free_int has a bit at or above cams_per_rig");
  if (fe == 0) return rcalib_fail(c, "free_ext names no camera");
  if (fi == 0) return rcalib_fail(c, "free_int names no camera");
  if (fe == all) return rcalib_fail(c, "free_ext names every camera: one must be held");
  if (rp->param_mask < 1 || rp->param_mask > 0xFF) return rcalib_fail(c, "param_mask outside 1..0xFF");
  if (rp->min_obs_cam < 14) return rcalib_fail(c, "min_obs_cam must be >= 14");
  if (mantis_status e = linecal_check_cams(c, kRcalibNames, cams, N, C, T_in)) return e;
  const auto run = c->calib_robust.loss ? linecal_run<lc::Rig, true> : linecal_run<lc::Rig, false>;
  return run(c, c->rb, kRcalibNames, cams, N, C, T_in, p, fe, fi, (uint32_t)rp->param_mask, rp->min_obs_cam, T_out,
             out);
}

}  // namespace

extern "C" {

void mantis_default_calib_params(mantis_calib_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(mantis_calib_params);
  p->free_cams = 0;
  p->min_obs_cam = 60;
}

void mantis_calib_sizes(int32_t* params_bytes, int32_t* result_bytes) {
  if (params_bytes) *params_bytes = (int32_t)sizeof(mantis_calib_params);
  if (result_bytes) *result_bytes = (int32_t)sizeof(mantis_calib_result);
}

mantis_status mantis_calibrate_extrinsics(void* ctx, const mantis_image* cams, int32_t n_rigs, int32_t cams_per_rig,
                                          const double* T_w_b_in, const mantis_refine_params* p,
                                          const mantis_calib_params* cp, double* T_w_b_out, mantis_calib_result* out) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  return calib_impl(c, cams, n_rigs, cams_per_rig, T_w_b_in, p, cp, T_w_b_out, out);
}

mantis_status mantis_get_calib_record(void* ctx, int32_t rig, int32_t pass, double* T_w_b, double* T_base_cam,
                                      int32_t* codes, int32_t* Sw, int32_t* Skw, double* rows, double* acc91) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  return linecal_record<lc::Ext>(c, c->cb, kCalibNames, rig, pass, T_w_b, T_base_cam, nullptr, codes, Sw, Skw, rows,
                                 acc91);
}

void mantis_default_icalib_params(mantis_icalib_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(mantis_icalib_params);
  p->free_cams = 0;
  p->param_mask = 0xFF;
  p->min_obs_cam = 60;
}

void mantis_icalib_sizes(int32_t* params_bytes, int32_t* result_bytes) {
  if (params_bytes) *params_bytes = (int32_t)sizeof(mantis_icalib_params);
  if (result_bytes) *result_bytes = (int32_t)sizeof(mantis_icalib_result);
}

mantis_status mantis_calibrate_intrinsics(void* ctx, const mantis_image* cams, int32_t n_rigs, int32_t cams_per_rig,
                                          const double* T_w_b_in, const mantis_refine_params* p,
                                          const mantis_icalib_params* ip, double* T_w_b_out, mantis_icalib_result* out) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  return icalib_impl(c, cams, n_rigs, cams_per_rig, T_w_b_in, p, ip, T_w_b_out, out);
}

mantis_status mantis_get_icalib_record(void* ctx, int32_t rig, int32_t pass, double* T_w_b, double* KD, int32_t* codes,
                                       int32_t* Sw, int32_t* Skw, double* rows, double* acc120) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  return linecal_record<lc::Int>(c, c->ib, kIcalibNames, rig, pass, T_w_b, nullptr, KD, codes, Sw, Skw, rows, acc120);
}

void mantis_default_rcalib_params(mantis_rcalib_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(mantis_rcalib_params);
  p->free_ext = 0;
  p->free_int = 0;
  p->param_mask = 0xFF;
  p->min_obs_cam = 60;
}

void mantis_rcalib_sizes(int32_t* params_bytes, int32_t* result_bytes) {
  if (params_bytes) *params_bytes = (int32_t)sizeof(mantis_rcalib_params);
  if (result_bytes) *result_bytes = (int32_t)sizeof(mantis_rcalib_result);
}

mantis_status mantis_calibrate_rig(void* ctx, const mantis_image* cams, int32_t n_rigs, int32_t cams_per_rig,
                                   const double* T_w_b_in, const mantis_refine_params* p,
                                   const mantis_rcalib_params* rp, double* T_w_b_out, mantis_rcalib_result* out) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  return rcalib_impl(c, cams, n_rigs, cams_per_rig, T_w_b_in, p, rp, T_w_b_out, out);
}

mantis_status mantis_get_rcalib_record(void* ctx, int32_t rig, int32_t pass, double* T_w_b, double* T_base_cam,
                                       double* KD, int32_t* codes, int32_t* Sw, int32_t* Skw, double* rows,
                                       double* acc231) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  return linecal_record<lc::Rig>(c, c->rb, kRcalibNames, rig, pass, T_w_b, T_base_cam, KD, codes, Sw, Skw, rows,
                                 acc231);
}

void mantis_calib_robust_sizes(int32_t* params_bytes, int32_t* stats_bytes) {
  if (params_bytes) *params_bytes = (int32_t)sizeof(mantis_refine_robust_params);
  if (stats_bytes) *stats_bytes = (int32_t)sizeof(mantis_calib_robust_stats);
}

mantis_status mantis_calib_set_robust(void* ctx, const mantis_refine_robust_params* p) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  auto fail = [c](const char* what) {
    c->err = std::string("calib robust: ") + what;
    return MANTIS_ERR_ARG;
  };
  if (!p) {
    c->calib_robust = mantis_refine_robust_params{};
    return MANTIS_OK;
  }
  if (p->struct_size != (int32_t)sizeof(mantis_refine_robust_params)) return fail("robust.struct_size mismatch");
  if (p->loss < rfn::kLossNone || p->loss > rfn::kLossTukey) return fail("robust.loss outside 0..2");
  if (p->loss == rfn::kLossNone) {
    c->calib_robust = mantis_refine_robust_params{};
    return MANTIS_OK;
  }
  if (!(p->tuning > 0) || !std::isfinite(p->tuning)) return fail("robust.tuning must be finite and > 0");
  if (!(p->scale_floor > 0) || !std::isfinite(p->scale_floor)) return fail("robust.scale_floor must be finite and > 0");
  c->calib_robust = *p;
  return MANTIS_OK;
}

mantis_status mantis_get_calib_robust(void* ctx, int32_t kind, mantis_calib_robust_stats* stats) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  if (!stats || kind < lc::kKindExt || kind > lc::kKindRig) {
    c->err = "calib robust: null argument or kind outside 0..2";
    return MANTIS_ERR_ARG;
  }
  const Ctx::Linecal& k = kind == lc::kKindExt ? c->cb : kind == lc::kKindInt ? c->ib : c->rb;
  if (!k.rigs || k.rec_loss == rfn::kLossNone) {
    c->err = "calib robust: no calibration of that kind yet, or its last call ran with the robust rows off";
    return MANTIS_ERR_STATE;
  }
  *stats = *(const mantis_calib_robust_stats*)k.h_rstats.get();
  return MANTIS_OK;
}

mantis_status mantis_get_calib_robust_record(void* ctx, int32_t kind, int32_t rig, int32_t pass, uint32_t* keys,
                                             double* weights) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  if (kind < lc::kKindExt || kind > lc::kKindRig) {
    c->err = "calib robust record: kind outside 0..2";
    return MANTIS_ERR_ARG;
  }
  const Ctx::Linecal& k = kind == lc::kKindExt ? c->cb : kind == lc::kKindInt ? c->ib : c->rb;
  if (!k.rigs || !k.record || k.rec_loss == rfn::kLossNone) {
    c->err = "calib robust record: the last calibration of that kind kept none (robust rows on and params.record = 1)";
    return MANTIS_ERR_STATE;
  }
  if (rig < 0 || rig >= k.rigs || pass < 0 || pass > k.runs) {
    c->err = "calib robust record: rig or pass out of range (0 .. iterations_run)";
    return MANTIS_ERR_ARG;
  }
  const size_t ns = (size_t)k.C * k.cands, off = ((size_t)pass * k.rigs + rig) * ns;
  if (keys && ns > 0) {
    HIP_OK(hipMemcpy(keys, k.d_rkeys + off, sizeof(uint32_t) * ns, hipMemcpyDeviceToHost));
    for (size_t q = 0; q < ns; q++)
      if (keys[q] == mk::kNoKey) keys[q] = 0;  // a rejected slot
  }
  if (weights && ns > 0) HIP_OK(hipMemcpy(weights, k.d_rweights + off, sizeof(double) * ns, hipMemcpyDeviceToHost));
  return MANTIS_OK;
}

}  // extern "C"
