// Rig calibration: one joint Gauss-Newton over the base poses of N views of
// one rig, the extrinsics of the cameras in free_ext and the eight intrinsics
// of the cameras in free_int, on the grid lines (mantis_calibrate_rig,
// include/mantis.h). Included by api.hip after icalib_impl.hip: it shares the
// frame staging, the candidate list and the line-flag cache (refine_flags) and
// Landmarks with the refinement. The rules -- one observation with J_ext and
// J_int, the views' elimination, the reduced system, the updates, the gate and
// the covariances -- are in mk_rcalib.h (shared with the host build of the
// tests).
//
// Device work of one call of I iterations, all on the context stream:
//   per pass k = 0 .. I:  k_rcalib_obs    the (view, camera, candidate) slots at
//                                         the poses, extrinsics and intrinsics
//                                         of pass k
//                         k_rcalib_rig    per view: M^T M per camera (three MFMA
//                                         tiles per wave and camera), A_r's
//                                         Cholesky, Y_r, the view's Schur term
//                         k_rcalib_solve  the gates, S and its Cholesky, eps,
//                                         every delta_r, the updates
// = 3 (I + 1) launches, then the copies of the state, the poses and the last
// pass's accumulators. As in calib_impl.hip every hand-off between blocks
// crosses a kernel boundary: no last-block counter, no flag polled inside a
// kernel, no hipGraph capture. Nothing is drawn, no image stage runs.
#include "mk_rcalib.h"

namespace mk {

namespace rc = rcalib;

struct RcalibState {  // the call between the launches, and what comes back
  mantis_rcalib_result res;  // res.T_base_cam, res.K / res.D = the current extrinsics and intrinsics
  int32_t done, pad;
};

struct RcalibArgs {
  const int32_t* cand;  // n_cand: landmark | axis << 16
  RcalibState* st;
  double* T;            // N x 16: the views' current poses
  rc::Slot* slots;      // [pass][view][C n_cand]; pass_slots = the stride between passes (record) or 0
  double* acc;          // N x C x 231 of the pass
  double* recAcc;       // [pass][N][C][231] (record) or null
  int32_t* cnt;         // N x C code-0 rows
  double* Y;            // N x 6 x kLd: A_r^-1 [E_r | a_r]
  double* Wt;           // N x kMaxS x kLd: the views' Schur terms (lower triangle and the last column)
  int32_t* pd;          // N: A_r was positive definite
  double* recT;         // [pass][N][16]: the poses each pass observed at
  double* recE;         // [pass][C][16]: the extrinsics
  double* recKD;        // [pass][C][8]: the intrinsics
  size_t pass_slots;
  int32_t C, n_cand, I, N, min_obs, min_obs_cam;
  uint32_t free_ext, free_int, param_mask;
  rc::Layout l;         // the reduced unknowns
  rfn::Window win;
  double lambda;
};

// k_icalib_obs' scheme (icalib_impl.hip) with the camera's extrinsic and its
// eight intrinsics both read from the call's state (both change per pass):
// block (candidate chunk, camera, view), two candidates per wave, one per
// 32-lane half, one distort and one pixel per lane, integer sums by
// __shfl_xor inside the half, J_ext and J_int from the half's geometry and one
// plain store of the 184-byte slot by lane 0 of the half.
__global__ __launch_bounds__(256) void k_rcalib_obs(const FrameDesc* __restrict__ frames, Landmarks lmk, RcalibArgs a,
                                                    int pass) {
  const int chunk = blockIdx.x, cam = blockIdx.y, rig = blockIdx.z;
  const RcalibState& S = *a.st;
  if (S.done) return;  // block-uniform: the call stopped in an earlier pass
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, l = lane & 31;
  const int f = rig * a.C + cam;
  const Cam cm = icalib::cam_of(S.res.K[cam], S.res.D[cam]);
  const uint8_t* bgr = frames[f].bgr;
  const int W = frames[f].w, H = frames[f].h, npx = W * H;
  GnCam gc;
  rfn::gncam_from(S.res.T_base_cam[cam], gc);
  const bool free_ext = (a.free_ext >> cam & 1u) != 0, free_int = (a.free_int >> cam & 1u) != 0;
  double Rt[9], tw[3];
  rfn::pose_parts(a.T + 16 * (size_t)rig, Rt, tw);
  const double s = 1.0 / cm.fx;
  const int R = a.win.R, k = l - R;
  const bool active = l <= 2 * R;
  rc::Slot* out = a.slots + (size_t)pass * a.pass_slots + (size_t)f * a.n_cand;
  const int c0 = chunk * kRefineCands, c1 = min(c0 + kRefineCands, a.n_cand);
  for (int base = c0 + wave * 2; base < c1; base += 8) {  // wave-uniform trips: every lane reaches the shuffles
    const int ci = base + half;
    const bool live = ci < c1;  // an odd tail: the second half repeats the first's candidate and stores nothing
    const int cv = a.cand[live ? ci : base];
    const int i = cv & 0xffff, axis = cv >> 16;
    int tg[3];
    rfn::target_bgr(i, lmk.nw, lmk.nr, tg);
    calib::Geom g;
    const int gcode = calib::geom(Rt, tw, gc, lmk.xyz + 3 * i, axis, free_ext, g);
    int x = 0, y = 0;
    int outside = 0;
    if (!gcode && active) outside = rfn::sample_px(cm, g.g, k, s, W, H, &x, &y, nullptr, nullptr) ? 0 : 1;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) outside |= __shfl_xor(outside, m, 32);
    int32_t w = 0;
    if (!gcode && active && !outside) {  // 0 <= x < W, 0 <= y < H: the pixel is inside the frame
      const uint32_t pv = load_bgr(bgr, y * W + x, npx);
      w = rfn::px_weight((int)(pv & 0xffu), (int)((pv >> 8) & 0xffu), (int)((pv >> 16) & 0xffu), tg, a.win.white_thresh);
    }
    int32_t Sw = w, Skw = k * w;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) {
      Sw += __shfl_xor(Sw, m, 32);
      Skw += __shfl_xor(Skw, m, 32);
    }
    const int32_t w_lo = __shfl(w, 0, 32), w_hi = __shfl(w, 2 * R, 32);
    if (l == 0 && live) {
      rfn::Slot o7;
      rfn::finish(gcode, outside != 0, w_lo, w_hi, Sw, Skw, a.win.min_weight, s, g.g, o7);
      double Ji[rc::kPi];
#pragma unroll
      for (int e = 0; e < rc::kPi; e++) Ji[e] = 0.0;
      if (!o7.code) icalib::jint(cm, g.g.m0, g.g.nh, free_int, a.param_mask, Ji);
      rc::Slot o;
      rc::widen(o7, g.Je, Ji, o);
      out[ci] = o;
    }
  }
}

// One block per view. Wave w builds M^T M of M = [J_pose | J_ext | J_int | r]
// over the n_cand slots of cameras w and w + 4. The 21 columns do not fit one
// v_mfma_f64_16x16x4f64 tile: a lane holds column m of the low part (columns
// 0-15) and column 16 + m of the high part (columns 16-20, zero for m >= 5),
// and each group of four rows is three MFMAs, low.low, low.high and high.high
// (the tile's entry (i, j) is in lane (i & 3) * 16 + j, register i >> 2). One
// wave owns its three tiles, so there is no cross-wave sum. After a barrier
// the block forms A_r and [E_r | a_r] from the tiles, thread 0 factors A_r,
// one thread per column solves Y_r = A_r^-1 [E_r | a_r] and one thread per
// entry forms the lower triangle and the last column of the view's Schur term
// E_r^T Y_r (what k_rcalib_solve reads). Pass I solves nothing: it writes the
// accumulators and the counts only.
__global__ __launch_bounds__(256) void k_rcalib_rig(RcalibArgs a, int pass) {
  __shared__ double s_acc[rc::kMaxCams * rc::kAcc];
  __shared__ double s_A[36], s_L[36];
  __shared__ double s_E[6 * rc::kLd], s_Y[6 * rc::kLd];
  __shared__ int32_t s_pd;
  const int rig = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  if (a.st->done) return;
  const int C = a.C, nc = a.n_cand, nS = a.l.nS;
  const int kk = lane >> 4, m = lane & 15;
  constexpr int kHi = rc::kRow - 16;  // columns of the high part
  for (int cam = wave; cam < C; cam += 4) {  // wave-uniform
    const rc::Slot* sl = a.slots + (size_t)pass * a.pass_slots + (size_t)(rig * C + cam) * nc;
    v4d ll = {0, 0, 0, 0}, lh = {0, 0, 0, 0}, hh = {0, 0, 0, 0};
    // four trips' loads in flight before their MFMAs (the accumulation order is
    // the plain loop's; trips past the end add exact zeros)
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
    int32_t n = 0;
    for (int r = lane; r < nc; r += 64) n += sl[r].code == 0;
#pragma unroll
    for (int q = 32; q >= 1; q >>= 1) n += __shfl_xor(n, q, 64);
    if (lane == 0) a.cnt[rig * C + cam] = n;
    double* sa = s_acc + rc::kAcc * cam;
#pragma unroll
    for (int r = 0; r < 4; r++) {  // entry (kk + 4 r, m) of each tile; low.low and high.high are symmetric bit for bit
      const int i = kk + 4 * r;
      if (i <= m) sa[rc::tri(i, m)] = ll[r];
      if (m < kHi) sa[rc::tri(i, 16 + m)] = lh[r];
      if (i <= m && m < kHi) sa[rc::tri(16 + i, 16 + m)] = hh[r];
    }
  }
  __syncthreads();
  for (int e = t; e < C * rc::kAcc; e += 256) {
    const double v = s_acc[e];
    a.acc[(size_t)rig * C * rc::kAcc + e] = v;
    if (a.recAcc) a.recAcc[((size_t)pass * a.N + rig) * C * rc::kAcc + e] = v;
  }
  if (pass >= a.I) return;  // block-uniform
  if (t < 36) s_A[t] = rc::view_A(s_acc, C, t / 6, t % 6, a.lambda);
  for (int e = t; e < 6 * (nS + 1); e += 256) {
    const int k = e / (nS + 1), j = e % (nS + 1);
    s_E[rc::kLd * k + j] = rc::view_rhs(s_acc, C, a.l, k, j);
  }
  __syncthreads();
  if (t == 0) {
    const int32_t ok = calib::chol6(s_A, s_L) ? 1 : 0;
    s_pd = ok;
    a.pd[rig] = ok;
  }
  __syncthreads();
  if (!s_pd) return;  // k_rcalib_solve stops the call: Y_r and the term are not read
  if (t <= nS) rc::view_solve(s_L, s_E + t, s_Y + t);
  __syncthreads();
  for (int e = t; e < 6 * (nS + 1); e += 256) {
    const int k = e / (nS + 1), j = e % (nS + 1);
    a.Y[((size_t)rig * 6 + k) * rc::kLd + j] = s_Y[rc::kLd * k + j];
  }
  for (int e = t; e < nS * (nS + 1); e += 256) {
    const int i = e / (nS + 1), j = e % (nS + 1);
    if (j <= i || j == nS) a.Wt[((size_t)rig * rc::kMaxS + i) * rc::kLd + j] = rc::schur_entry(s_E, s_Y, i, j);
  }
}

// One block. k_icalib_solve's scheme: the figures of the pass and its gates;
// one thread per entry sums the views' Schur terms in view order into [S | s];
// the left-looking Cholesky of S with one barrier per column (every entry by
// the sequential formula, the pivot recomputed by every thread; L's strict
// lower triangle overwrites S's in place, its diagonal is kept apart); eps by
// thread 0; one thread per camera of free_int forms the updated intrinsics and
// the DIVERGED test; then one thread per view forms delta_r from the stored
// Y_r and updates T_r, one per camera of free_ext updates E_c, one per camera
// of free_int stores its intrinsics. [S | s] is up to 106 x 107 doubles, past
// the static LDS limit: it is the kernel's dynamic LDS (nS rows of kLd). The
// pass record (poses, extrinsics, intrinsics) is written here.
__global__ __launch_bounds__(256) void k_rcalib_solve(RcalibArgs a, int pass) {
  extern __shared__ double rcs_S[];  // nS x kLd
  __shared__ double s_rr[rc::kMaxViews * rc::kMaxCams];
  __shared__ double s_d[rc::kMaxS], s_eps[rc::kMaxS], s_y[rc::kMaxS];
  __shared__ double s_next[rc::kMaxCams][rc::kPi];
  __shared__ int32_t s_view[rc::kMaxViews], s_vpd[rc::kMaxViews], s_camn[rc::kMaxCams], s_ok[rc::kMaxCams], s_stop;
  double* s_S = rcs_S;
  RcalibState& S = *a.st;
  if (S.done) return;
  const int t = threadIdx.x, N = a.N, C = a.C, nS = a.l.nS, Fe = a.l.Fe, Fi = a.l.Fi;
  const uint32_t free_any = a.free_ext | a.free_int;
  for (int e = t; e < N * 16; e += 256) a.recT[(size_t)pass * N * 16 + e] = a.T[e];
  for (int e = t; e < C * 16; e += 256) a.recE[(size_t)pass * C * 16 + e] = S.res.T_base_cam[e >> 4][e & 15];
  for (int e = t; e < C * rc::kPi; e += 256) {
    const int c = e >> 3, q = e & 7;
    a.recKD[(size_t)pass * C * rc::kPi + e] = q < 4 ? S.res.K[c][q] : S.res.D[c][q - 4];
  }
  for (int e = t; e < N * C; e += 256) s_rr[e] = a.acc[(size_t)rc::kAcc * e + (rc::kAcc - 1)];
  if (t < N) {  // N <= 256 = the block
    int32_t n = 0;
    for (int c = 0; c < C; c++) n += a.cnt[t * C + c];
    s_view[t] = n;
    s_vpd[t] = pass < a.I ? a.pd[t] : 1;
  }
  if (t < C) {
    int32_t n = 0;
    for (int r = 0; r < N; r++) n += a.cnt[r * C + t];
    s_camn[t] = n;
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
    int32_t stop = 0;
    if (pass >= a.I) {
      stop = 1;
    } else if (starved) {
      S.res.status = rc::kStarved;
      stop = 1;
    } else if (singular) {
      S.res.status = rc::kSingular;
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
      s_S[rc::kLd * i + j] = rc::reduced_entry(a.acc, a.Wt, N, C, a.l, i, j, a.lambda, a.param_mask);
  }
  __syncthreads();
  bool bad = false;
  for (int j = 0; j < nS; j++) {
    const double d = rc::cholS_pivot(s_S, s_S, j);
    if (!(d > 0)) {
      bad = true;
      break;
    }
    const double ljj = sqrt(d);
    const int i = j + 1 + t;
    if (t == 0) s_d[j] = ljj;
    if (i < nS) s_S[rc::kLd * i + j] = rc::cholS_below(s_S, s_S, i, j, ljj);
    __syncthreads();
  }
  if (bad) {
    if (t == 0) {
      S.res.status = rc::kSingular;
      S.done = 1;
    }
    return;
  }
  if (t == 0) rc::cholS_solve(s_S, s_d, nS, s_S + nS, rc::kLd, s_y, s_eps);
  __syncthreads();
  const double* epi = s_eps + rc::kPe * Fe;
  if (t < Fi) {
    const int cam = a.l.fi[t];
    double th[rc::kPi], x[rc::kPi], nx[rc::kPi];
    icalib::cam_to(icalib::cam_of(S.res.K[cam], S.res.D[cam]), th);
#pragma unroll
    for (int e = 0; e < rc::kPi; e++) x[e] = epi[rc::kPi * t + e];
    s_ok[t] = icalib::param_update(th, x, a.param_mask, nx) ? 1 : 0;
#pragma unroll
    for (int e = 0; e < rc::kPi; e++) s_next[t][e] = nx[e];
  }
  __syncthreads();
  bool diverged = false;
  for (int f = 0; f < Fi; f++) diverged = diverged || !s_ok[f];  // block-uniform
  if (diverged) {
    if (t == 0) {
      S.res.status = rc::kDiverged;
      S.done = 1;
    }
    return;
  }
  if (t < N) {
    double d6[6], T[16];
    rc::pose_delta(a.Y + (size_t)t * 6 * rc::kLd, s_eps, nS, d6);
#pragma unroll
    for (int e = 0; e < 16; e++) T[e] = a.T[16 * t + e];
    calib::right_update(T, d6);
#pragma unroll
    for (int e = 0; e < 16; e++) a.T[16 * t + e] = T[e];
  }
  if (t < Fe) {
    const int cam = a.l.fe[t];
    double x[6], E[16];
#pragma unroll
    for (int e = 0; e < 6; e++) x[e] = s_eps[rc::kPe * t + e];
#pragma unroll
    for (int e = 0; e < 16; e++) E[e] = S.res.T_base_cam[cam][e];
    calib::right_update(E, x);
#pragma unroll
    for (int e = 0; e < 16; e++) S.res.T_base_cam[cam][e] = E[e];
#pragma unroll
    for (int e = 0; e < 6; e++) S.res.delta_ext[pass][cam][e] = x[e];
  }
  if (t < Fi) {
    const int cam = a.l.fi[t];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      S.res.K[cam][e] = s_next[t][e];
      S.res.D[cam][e] = s_next[t][4 + e];
    }
#pragma unroll
    for (int e = 0; e < rc::kPi; e++)
      S.res.delta_int[pass][cam][e] = (a.param_mask >> e & 1u) ? epi[rc::kPi * t + e] : 0.0;
  }
  if (t == 0) S.res.iterations_run = pass + 1;
}

}  // namespace mk

namespace {

namespace rc = mk::rcalib;

mantis_status rcalib_fail(Ctx* c, const char* what) {
  c->err = std::string("rcalib: ") + what;
  return MANTIS_ERR_ARG;
}

// workspaces for a call of N views x C cameras
mantis_status rcalib_workspace(Ctx* c, int N, int C, int I, bool record) {
  Ctx::Rcalib& k = c->rb;
  const size_t slots = (record ? (size_t)I + 1 : 1) * N * C * std::max(c->rf.n_cand, 1);
  const size_t racc = record ? (size_t)(I + 1) * N * C * rc::kAcc : 0;
  if (N > k.view_cap || slots > k.slot_cap || racc > k.racc_cap) HIP_OK(hipStreamSynchronize(c->s));
  if (N > k.view_cap) {
    k.view_cap = 0;
    if (k.h_state) (void)hipHostFree(k.h_state);
    k.h_state = nullptr;
    const size_t n = (size_t)N, nc = n * rc::kMaxCams;
    // pinned: the state, the poses, the accumulators, the counts
    const size_t hb = sizeof(mk::RcalibState) + sizeof(double) * (16 * n + rc::kAcc * nc) + sizeof(int32_t) * nc;
    if (refine_grow(c, (mk::RcalibState**)&k.d_state, (size_t)1) || refine_grow(c, &k.d_T, 16 * n) ||
        refine_grow(c, &k.d_acc, rc::kAcc * nc) || refine_grow(c, &k.d_cnt, nc) ||
        refine_grow(c, &k.d_Y, n * 6 * rc::kLd) || refine_grow(c, &k.d_Wt, n * rc::kMaxS * rc::kLd) ||
        refine_grow(c, &k.d_pd, n) || refine_grow(c, &k.d_recT, (size_t)(rfn::kMaxIterations + 1) * 16 * n) ||
        refine_grow(c, &k.d_recE, (size_t)(rfn::kMaxIterations + 1) * 16 * rc::kMaxCams) ||
        refine_grow(c, &k.d_recKD, (size_t)(rfn::kMaxIterations + 1) * rc::kPi * rc::kMaxCams) ||
        halloc(c, (uint8_t**)&k.h_state, hb))
      return MANTIS_ERR_OOM;
    k.view_cap = N;
  }
  if (slots > k.slot_cap) {
    k.slot_cap = 0;
    if (refine_grow(c, (rc::Slot**)&k.d_slots, slots)) return MANTIS_ERR_OOM;
    k.slot_cap = slots;
  }
  if (racc > k.racc_cap) {
    k.racc_cap = 0;
    if (refine_grow(c, &k.d_recAcc, racc)) return MANTIS_ERR_OOM;
    k.racc_cap = racc;
  }
  return MANTIS_OK;
}

mantis_status rcalib_impl(Ctx* c, const mantis_image* cams, int32_t N, int32_t C, const double* T_in,
                          const mantis_refine_params* p, const mantis_rcalib_params* rp, double* T_out,
                          mantis_rcalib_result* out) {
  if (!cams || !T_in || !p || !rp || !T_out || !out) return rcalib_fail(c, "null argument");
  if (rp->struct_size != (int32_t)sizeof(mantis_rcalib_params))
    return rcalib_fail(c, "rcalib_params.struct_size mismatch");
  if (N > rc::kMaxViews) return rcalib_fail(c, "n_rigs exceeds 256");
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
  for (size_t i = 0; i < 16 * (size_t)N; i++)
    if (!std::isfinite(T_in[i])) return rcalib_fail(c, "T_w_b_in is not finite");
  for (int k = 0; k < C; k++) {
    for (int e = 0; e < 16; e++)
      if (!std::isfinite(cams[k].T_base_cam[e])) return rcalib_fail(c, "T_base_cam is not finite");
    for (int e = 0; e < 9; e++)
      if (!std::isfinite(cams[k].K[e])) return rcalib_fail(c, "K is not finite");
    for (int e = 0; e < 4; e++)
      if (!std::isfinite(cams[k].D[e])) return rcalib_fail(c, "D is not finite");
    const mk::Cam cm = cam_from(cams[k]);
    if (!(cm.fx > 0) || !(cm.fy > 0) || !std::isfinite(cm.fx) || !std::isfinite(cm.fy) || !std::isfinite(cm.cx) ||
        !std::isfinite(cm.cy))
      return rcalib_fail(c, "K: fx and fy must be > 0 and finite as floats");
  }
  for (int r = 1; r < N; r++)
    for (int k = 0; k < C; k++) {
      const mantis_image &v = cams[r * C + k], &v0 = cams[k];
      if (std::memcmp(v.T_base_cam, v0.T_base_cam, sizeof(v0.T_base_cam)) != 0)
        return rcalib_fail(c, "T_base_cam of a view differs from view 0's");
      if (std::memcmp(v.K, v0.K, sizeof(v0.K)) != 0) return rcalib_fail(c, "K of a view differs from view 0's");
      if (std::memcmp(v.D, v0.D, sizeof(v0.D)) != 0) return rcalib_fail(c, "D of a view differs from view 0's");
    }

  const int I = p->iterations, n = N * C;
  Ctx::Rcalib& k = c->rb;
  k.rigs = 0;  // no record until this call has finished
  if (!k.lds_asked) {  // [S | s] of the largest system as k_rcalib_solve's dynamic LDS
    k.lds_asked = true;
    k.lds_ok = hipFuncSetAttribute((const void*)mk::k_rcalib_solve, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(sizeof(double) * rc::kMaxS * rc::kLd)) == hipSuccess;
  }
  if (!k.lds_ok) {
    c->err = "rcalib: the device refused k_rcalib_solve's dynamic LDS";
    return MANTIS_ERR_STATE;
  }
  if (mantis_status e = refine_flags(c, p->landmark_pitch)) return e;
  if (mantis_status e = rcalib_workspace(c, N, C, I, p->record != 0)) return e;
  const int nc = c->rf.n_cand;

  mk::RcalibState* h_st = (mk::RcalibState*)k.h_state;
  double* h_T = (double*)(h_st + 1);
  double* h_acc = h_T + 16 * (size_t)k.view_cap;
  int32_t* h_cnt = (int32_t*)(h_acc + (size_t)rc::kAcc * k.view_cap * rc::kMaxCams);
  std::memset(h_st, 0, sizeof(*h_st));
  h_st->res.n_cand = nc;
  h_st->res.n_rigs = N;
  h_st->res.n_cams = C;
  h_st->res.free_ext = rp->free_ext;
  h_st->res.free_int = rp->free_int;
  h_st->res.param_mask = rp->param_mask;
  for (int q = 0; q < C; q++) {
    double th[rc::kPi];
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
  HIP_OK(hipMemcpyAsync(k.d_state, h_st, sizeof(mk::RcalibState), hipMemcpyHostToDevice, c->s));
  HIP_OK(hipMemcpyAsync(k.d_T, h_T, sizeof(double) * 16 * (size_t)N, hipMemcpyHostToDevice, c->s));

  mk::RcalibArgs a{};
  a.cand = c->rf.d_cand;
  a.st = (mk::RcalibState*)k.d_state;
  a.T = k.d_T;
  a.slots = (rc::Slot*)k.d_slots;
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
  a.min_obs_cam = rp->min_obs_cam;
  a.free_ext = fe;
  a.free_int = fi;
  a.param_mask = (uint32_t)rp->param_mask;
  rc::layout(fe, fi, C, a.l);
  a.win = rfn::Window{p->half_window, p->white_thresh, p->min_weight, 0};
  a.lambda = p->lambda;
  const size_t solve_lds = sizeof(double) * (size_t)a.l.nS * rc::kLd;
  const Landmarks L = lmk_of(c);
  mark(c, "start");
  const dim3 grid((nc + mk::kRefineCands - 1) / mk::kRefineCands, C, N);
  for (int pass = 0; pass <= I; pass++) {
    if (nc > 0) {
      mk::k_rcalib_obs<<<grid, 256, 0, c->s>>>(c->d_frames, L, a, pass);
      HIP_OK(hipGetLastError());
    }
    mark(c, "rcalib_obs/k_rcalib_obs");
    mk::k_rcalib_rig<<<N, 256, 0, c->s>>>(a, pass);
    HIP_OK(hipGetLastError());
    mark(c, "rcalib_rig/k_rcalib_rig");
    mk::k_rcalib_solve<<<1, 256, solve_lds, c->s>>>(a, pass);
    HIP_OK(hipGetLastError());
    mark(c, "rcalib_solve/k_rcalib_solve");
  }
  HIP_OK(hipMemcpyAsync(h_st, k.d_state, sizeof(mk::RcalibState), hipMemcpyDeviceToHost, c->s));
  HIP_OK(hipMemcpyAsync(h_T, k.d_T, sizeof(double) * 16 * (size_t)N, hipMemcpyDeviceToHost, c->s));
  HIP_OK(hipMemcpyAsync(h_acc, k.d_acc, sizeof(double) * rc::kAcc * (size_t)n, hipMemcpyDeviceToHost, c->s));
  HIP_OK(hipMemcpyAsync(h_cnt, k.d_cnt, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->s));
  HIP_OK(wait_stream(c, n));
  finish_profile(c);
  rc::conclude(h_acc, h_cnt, N, C, fe, fi, (uint32_t)rp->param_mask, p->min_obs, rp->min_obs_cam, p->max_rms,
               h_st->res);
  *out = h_st->res;
  std::memcpy(T_out, h_T, sizeof(double) * 16 * (size_t)N);
  k.rigs = N;
  k.C = C;
  k.record = p->record;
  k.cands = nc;
  k.runs = h_st->res.iterations_run;
  return MANTIS_OK;
}

}  // namespace

extern "C" {

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
  const Ctx::Rcalib& k = c->rb;
  if (!k.rigs || !k.record) {
    c->err = "rcalib record: the last rig calibration kept none (params.record = 1)";
    return MANTIS_ERR_STATE;
  }
  if (rig < 0 || rig >= k.rigs || pass < 0 || pass > k.runs)
    return rcalib_fail(c, "record: rig or pass out of range (0 .. iterations_run)");
  const size_t ns = (size_t)k.C * k.cands, pr = (size_t)pass * k.rigs + rig;
  if (T_w_b) HIP_OK(hipMemcpy(T_w_b, k.d_recT + pr * 16, sizeof(double) * 16, hipMemcpyDeviceToHost));
  if (T_base_cam)
    HIP_OK(hipMemcpy(T_base_cam, k.d_recE + (size_t)pass * k.C * 16, sizeof(double) * 16 * k.C, hipMemcpyDeviceToHost));
  if (KD)
    HIP_OK(hipMemcpy(KD, k.d_recKD + (size_t)pass * k.C * rc::kPi, sizeof(double) * rc::kPi * k.C, hipMemcpyDeviceToHost));
  if (acc231)
    HIP_OK(hipMemcpy(acc231, k.d_recAcc + pr * k.C * rc::kAcc, sizeof(double) * rc::kAcc * k.C, hipMemcpyDeviceToHost));
  if ((codes || Sw || Skw || rows) && ns > 0) {
    std::vector<rc::Slot> hs(ns);
    HIP_OK(hipMemcpy(hs.data(), (const rc::Slot*)k.d_slots + pr * ns, sizeof(rc::Slot) * ns, hipMemcpyDeviceToHost));
    for (size_t q = 0; q < ns; q++) {
      if (codes) codes[q] = hs[q].code;
      if (Sw) Sw[q] = hs[q].Sw;
      if (Skw) Skw[q] = hs[q].Skw;
      if (rows) std::memcpy(rows + rc::kRow * q, hs[q].row, sizeof(double) * rc::kRow);
    }
  }
  return MANTIS_OK;
}

}  // extern "C"
