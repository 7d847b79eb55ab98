// Intrinsic calibration: a joint Gauss-Newton over the base poses of N views
// of one rig and the eight intrinsics (fx, fy, cx, cy, k1..k4) of its free
// cameras, on the grid lines (mantis_calibrate_intrinsics, include/mantis.h).
// Included by api.hip after calib_impl.hip: it shares the frame staging, the
// candidate list and the line-flag cache (refine_flags) and Landmarks with the
// refinement. The rules -- one observation with J_int, the views' elimination,
// the reduced system, the parameter update, the gate and the covariance -- are
// in mk_icalib.h (shared with the host build of the tests).
//
// Device work of one call of I iterations, all on the context stream:
//   per pass k = 0 .. I:  k_icalib_obs    the (view, camera, candidate) slots at
//                                         the poses and intrinsics of pass k
//                         k_icalib_rig    per view: M^T M per camera (one MFMA
//                                         tile per wave and camera), A_r's
//                                         Cholesky, Y_r, the view's Schur term
//                         k_icalib_solve  the gates, S and its Cholesky, eps,
//                                         every delta_r, the updates
// = 3 (I + 1) launches, then the copies of the state, the poses and the last
// pass's accumulators. As in calib_impl.hip every hand-off between blocks
// crosses a kernel boundary: no last-block counter, no flag polled inside a
// kernel, no hipGraph capture. Nothing is drawn, no image stage runs.
#include "mk_icalib.h"

namespace mk {

namespace ic = icalib;

struct IcalibState {  // the call between the launches, and what comes back
  mantis_icalib_result res;  // res.K / res.D = the current intrinsics
  double Tbc[ic::kMaxCams][16];  // the extrinsics, held
  int32_t done, pad;
};

struct IcalibArgs {
  const int32_t* cand;  // n_cand: landmark | axis << 16
  IcalibState* st;
  double* T;            // N x 16: the views' current poses
  ic::Slot* slots;      // [pass][view][C n_cand]; pass_slots = the stride between passes (record) or 0
  double* acc;          // N x C x 120 of the pass
  double* recAcc;       // [pass][N][C][120] (record) or null
  int32_t* cnt;         // N x C code-0 rows
  double* Y;            // N x 6 x kLd: A_r^-1 [E_r | a_r]
  double* Wt;           // N x kMaxS x kLd: the views' Schur terms (lower triangle and the last column)
  int32_t* pd;          // N: A_r was positive definite
  double* recT;         // [pass][N][16]: the poses each pass observed at
  double* recKD;        // [pass][C][8]: the intrinsics
  size_t pass_slots;
  int32_t C, n_cand, I, N, min_obs, min_obs_cam, F, nS;
  uint32_t free_cams, param_mask;
  int32_t fcam[ic::kMaxCams];  // the free cameras, ascending
  rfn::Window win;
  double lambda;
};

// k_calib_obs' scheme (calib_impl.hip) with the camera's eight intrinsics read
// from the call's state (they change per pass): block (candidate chunk,
// camera, view), two candidates per wave, one per 32-lane half, one distort
// and one pixel per lane, integer sums by __shfl_xor inside the half, J_int
// from the half's geometry and one plain store of the 136-byte slot by lane 0
// of the half.
__global__ __launch_bounds__(256) void k_icalib_obs(const FrameDesc* __restrict__ frames, Landmarks lmk, IcalibArgs a,
                                                    int pass) {
  const int chunk = blockIdx.x, cam = blockIdx.y, rig = blockIdx.z;
  const IcalibState& S = *a.st;
  if (S.done) return;  // block-uniform: the call stopped in an earlier pass
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, l = lane & 31;
  const int f = rig * a.C + cam;
  const Cam cm = ic::cam_of(S.res.K[cam], S.res.D[cam]);
  const uint8_t* bgr = frames[f].bgr;
  const int W = frames[f].w, H = frames[f].h, npx = W * H;
  GnCam gc;
  rfn::gncam_from(S.Tbc[cam], gc);
  const bool free_cam = (a.free_cams >> cam & 1u) != 0;
  double Rt[9], tw[3];
  rfn::pose_parts(a.T + 16 * (size_t)rig, Rt, tw);
  const double s = 1.0 / cm.fx;
  const int R = a.win.R, k = l - R;
  const bool active = l <= 2 * R;
  ic::Slot* out = a.slots + (size_t)pass * a.pass_slots + (size_t)f * a.n_cand;
  const int c0 = chunk * kRefineCands, c1 = min(c0 + kRefineCands, a.n_cand);
  for (int base = c0 + wave * 2; base < c1; base += 8) {  // wave-uniform trips: every lane reaches the shuffles
    const int ci = base + half;
    const bool live = ci < c1;  // an odd tail: the second half repeats the first's candidate and stores nothing
    const int cv = a.cand[live ? ci : base];
    const int i = cv & 0xffff, axis = cv >> 16;
    int tg[3];
    rfn::target_bgr(i, lmk.nw, lmk.nr, tg);
    rfn::Geom g;
    const int gcode = rfn::geom(Rt, tw, gc, lmk.xyz + 3 * i, axis, g);
    int x = 0, y = 0;
    int outside = 0;
    if (!gcode && active) outside = rfn::sample_px(cm, g, k, s, W, H, &x, &y, nullptr, nullptr) ? 0 : 1;
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
      rfn::finish(gcode, outside != 0, w_lo, w_hi, Sw, Skw, a.win.min_weight, s, g, o7);
      double Ji[ic::kP];
#pragma unroll
      for (int e = 0; e < ic::kP; e++) Ji[e] = 0.0;
      if (!o7.code) ic::jint(cm, g.m0, g.nh, free_cam, a.param_mask, Ji);
      ic::Slot o;
      ic::widen(o7, Ji, o);
      out[ci] = o;
    }
  }
}

// One block per view. Wave w builds M^T M of M = [J_pose | J_int | r] over the
// n_cand slots of cameras w and w + 4 with v_mfma_f64_16x16x4f64 (columns 0-14
// of the tile, four rows per instruction): one wave owns one tile, so there is
// no cross-wave sum. After a barrier the block forms A_r and [E_r | a_r] from
// the tiles, thread 0 factors A_r, one thread per column solves Y_r = A_r^-1
// [E_r | a_r] and one thread per entry forms the lower triangle and the last
// column of the view's Schur term E_r^T Y_r (what k_icalib_solve reads).
// Pass I solves nothing: it writes the accumulators and the counts only.
__global__ __launch_bounds__(256) void k_icalib_rig(IcalibArgs a, int pass) {
  __shared__ double s_acc[ic::kMaxCams * ic::kAcc];
  __shared__ double s_A[36], s_L[36];
  __shared__ double s_E[6 * ic::kLd], s_Y[6 * ic::kLd];
  __shared__ int32_t s_pd;
  const int rig = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  if (a.st->done) return;
  const int C = a.C, nc = a.n_cand, nS = a.nS;
  const int kk = lane >> 4, m = lane & 15;
  for (int cam = wave; cam < C; cam += 4) {  // wave-uniform
    const ic::Slot* sl = a.slots + (size_t)pass * a.pass_slots + (size_t)(rig * C + cam) * nc;
    v4d acc = {0, 0, 0, 0};
    // eight trips' loads in flight before their MFMAs (the accumulation order is
    // the plain loop's; trips past the end add exact zeros)
    constexpr int kU = 8;
    for (int base = 0; base < nc; base += 4 * kU) {
      double v[kU];
#pragma unroll
      for (int u = 0; u < kU; u++) {
        const int r = base + 4 * u + kk;
        v[u] = (r < nc && m < ic::kRow) ? sl[r].row[m] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kU; u++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u], v[u], acc, 0, 0, 0);
    }
    int32_t n = 0;
    for (int r = lane; r < nc; r += 64) n += sl[r].code == 0;
#pragma unroll
    for (int q = 32; q >= 1; q >>= 1) n += __shfl_xor(n, q, 64);
    if (lane == 0) a.cnt[rig * C + cam] = n;
#pragma unroll
    for (int r = 0; r < 4; r++) {  // entry (kk + 4 r, m) of the tile; the tile is symmetric bit for bit
      const int i = kk + 4 * r;
      if (i <= m && m < ic::kRow) s_acc[ic::kAcc * cam + ic::tri(i, m)] = acc[r];
    }
  }
  __syncthreads();
  for (int e = t; e < C * ic::kAcc; e += 256) {
    const double v = s_acc[e];
    a.acc[(size_t)rig * C * ic::kAcc + e] = v;
    if (a.recAcc) a.recAcc[((size_t)pass * a.N + rig) * C * ic::kAcc + e] = v;
  }
  if (pass >= a.I) return;  // block-uniform
  if (t < 36) s_A[t] = ic::view_A(s_acc, C, t / 6, t % 6, a.lambda);
  for (int e = t; e < 6 * (nS + 1); e += 256) {
    const int k = e / (nS + 1), j = e % (nS + 1);
    s_E[ic::kLd * k + j] = ic::view_rhs(s_acc, C, a.fcam, nS, k, j);
  }
  __syncthreads();
  if (t == 0) {
    const int32_t ok = calib::chol6(s_A, s_L) ? 1 : 0;
    s_pd = ok;
    a.pd[rig] = ok;
  }
  __syncthreads();
  if (!s_pd) return;  // k_icalib_solve stops the call: Y_r and the term are not read
  if (t <= nS) ic::view_solve(s_L, s_E + t, s_Y + t);
  __syncthreads();
  for (int e = t; e < 6 * (nS + 1); e += 256) {
    const int k = e / (nS + 1), j = e % (nS + 1);
    a.Y[((size_t)rig * 6 + k) * ic::kLd + j] = s_Y[ic::kLd * k + j];
  }
  for (int e = t; e < nS * (nS + 1); e += 256) {
    const int i = e / (nS + 1), j = e % (nS + 1);
    if (j <= i || j == nS) a.Wt[((size_t)rig * ic::kMaxS + i) * ic::kLd + j] = ic::schur_entry(s_E, s_Y, i, j);
  }
}

// One block. The figures of the pass and its gates; one thread per entry sums
// the views' Schur terms in view order into [S | s]; the left-looking Cholesky
// of S with one barrier per column (every entry by the sequential formula, the
// pivot recomputed by every thread, so the values do not depend on which
// thread computes them and the exit is block-uniform; L's strict lower
// triangle overwrites S's in place, its diagonal is kept apart); eps by thread
// 0; one thread per free camera forms the updated intrinsics and the DIVERGED
// test; then one thread per view forms delta_r from the stored Y_r and updates
// T_r, one per free camera stores its intrinsics. The pass record (poses,
// intrinsics) is written here.
__global__ __launch_bounds__(256) void k_icalib_solve(IcalibArgs a, int pass) {
  __shared__ double s_S[ic::kMaxS * ic::kLd];
  __shared__ double s_rr[ic::kMaxViews * ic::kMaxCams];
  __shared__ double s_d[ic::kMaxS], s_eps[ic::kMaxS], s_y[ic::kMaxS];
  __shared__ double s_next[ic::kMaxCams][ic::kP];
  __shared__ int32_t s_view[ic::kMaxViews], s_vpd[ic::kMaxViews], s_camn[ic::kMaxCams], s_ok[ic::kMaxCams], s_stop;
  IcalibState& S = *a.st;
  if (S.done) return;
  const int t = threadIdx.x, N = a.N, C = a.C, nS = a.nS;
  for (int e = t; e < N * 16; e += 256) a.recT[(size_t)pass * N * 16 + e] = a.T[e];
  for (int e = t; e < C * ic::kP; e += 256) {
    const int c = e >> 3, q = e & 7;
    a.recKD[(size_t)pass * C * ic::kP + e] = q < 4 ? S.res.K[c][q] : S.res.D[c][q - 4];
  }
  for (int e = t; e < N * C; e += 256) s_rr[e] = a.acc[(size_t)ic::kAcc * e + (ic::kAcc - 1)];
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
      if (a.free_cams >> c & 1u) starved |= s_camn[c] < a.min_obs_cam;
    }
    S.res.n_obs[pass] = n_obs;
    S.res.rms[pass] = n_obs > 0 ? sqrt(rr / (double)n_obs) : 0.0;
    int32_t stop = 0;
    if (pass >= a.I) {
      stop = 1;
    } else if (starved) {
      S.res.status = ic::kStarved;
      stop = 1;
    } else if (singular) {
      S.res.status = ic::kSingular;
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
      s_S[ic::kLd * i + j] = ic::reduced_entry(a.acc, a.Wt, N, C, a.fcam, nS, i, j, a.lambda, a.param_mask);
  }
  __syncthreads();
  bool bad = false;
  for (int j = 0; j < nS; j++) {
    const double d = ic::cholS_pivot(s_S, s_S, j);
    if (!(d > 0)) {
      bad = true;
      break;
    }
    const double ljj = sqrt(d);
    const int i = j + 1 + t;
    if (t == 0) s_d[j] = ljj;
    if (i < nS) s_S[ic::kLd * i + j] = ic::cholS_below(s_S, s_S, i, j, ljj);
    __syncthreads();
  }
  if (bad) {
    if (t == 0) {
      S.res.status = ic::kSingular;
      S.done = 1;
    }
    return;
  }
  if (t == 0) ic::cholS_solve(s_S, s_d, nS, s_S + nS, ic::kLd, s_y, s_eps);
  __syncthreads();
  if (t < a.F) {
    const int cam = a.fcam[t];
    double th[ic::kP], x[ic::kP], nx[ic::kP];
    ic::cam_to(ic::cam_of(S.res.K[cam], S.res.D[cam]), th);
#pragma unroll
    for (int e = 0; e < ic::kP; e++) x[e] = s_eps[ic::kP * t + e];
    s_ok[t] = ic::param_update(th, x, a.param_mask, nx) ? 1 : 0;
#pragma unroll
    for (int e = 0; e < ic::kP; e++) s_next[t][e] = nx[e];
  }
  __syncthreads();
  bool diverged = false;
  for (int f = 0; f < a.F; f++) diverged = diverged || !s_ok[f];  // block-uniform
  if (diverged) {
    if (t == 0) {
      S.res.status = ic::kDiverged;
      S.done = 1;
    }
    return;
  }
  if (t < N) {
    double d6[6], T[16];
    ic::pose_delta(a.Y + (size_t)t * 6 * ic::kLd, s_eps, nS, d6);
#pragma unroll
    for (int e = 0; e < 16; e++) T[e] = a.T[16 * t + e];
    calib::right_update(T, d6);
#pragma unroll
    for (int e = 0; e < 16; e++) a.T[16 * t + e] = T[e];
  }
  if (t < a.F) {
    const int cam = a.fcam[t];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      S.res.K[cam][e] = s_next[t][e];
      S.res.D[cam][e] = s_next[t][4 + e];
    }
#pragma unroll
    for (int e = 0; e < ic::kP; e++)
      S.res.delta_cam[pass][cam][e] = (a.param_mask >> e & 1u) ? s_eps[ic::kP * t + e] : 0.0;
  }
  if (t == 0) S.res.iterations_run = pass + 1;
}

}  // namespace mk

namespace {

namespace ic = mk::icalib;

mantis_status icalib_fail(Ctx* c, const char* what) {
  c->err = std::string("icalib: ") + what;
  return MANTIS_ERR_ARG;
}

// workspaces for a call of N views x C cameras
mantis_status icalib_workspace(Ctx* c, int N, int C, int I, bool record) {
  Ctx::Icalib& k = c->ib;
  const size_t slots = (record ? (size_t)I + 1 : 1) * N * C * std::max(c->rf.n_cand, 1);
  const size_t racc = record ? (size_t)(I + 1) * N * C * ic::kAcc : 0;
  if (N > k.view_cap || slots > k.slot_cap || racc > k.racc_cap) HIP_OK(hipStreamSynchronize(c->s));
  if (N > k.view_cap) {
    k.view_cap = 0;
    if (k.h_state) (void)hipHostFree(k.h_state);
    k.h_state = nullptr;
    const size_t n = (size_t)N, nc = n * ic::kMaxCams;
    // pinned: the state, the poses, the accumulators, the counts
    const size_t hb = sizeof(mk::IcalibState) + sizeof(double) * (16 * n + ic::kAcc * nc) + sizeof(int32_t) * nc;
    if (refine_grow(c, (mk::IcalibState**)&k.d_state, (size_t)1) || refine_grow(c, &k.d_T, 16 * n) ||
        refine_grow(c, &k.d_acc, ic::kAcc * nc) || refine_grow(c, &k.d_cnt, nc) ||
        refine_grow(c, &k.d_Y, n * 6 * ic::kLd) || refine_grow(c, &k.d_Wt, n * ic::kMaxS * ic::kLd) ||
        refine_grow(c, &k.d_pd, n) || refine_grow(c, &k.d_recT, (size_t)(rfn::kMaxIterations + 1) * 16 * n) ||
        refine_grow(c, &k.d_recKD, (size_t)(rfn::kMaxIterations + 1) * ic::kP * ic::kMaxCams) ||
        halloc(c, (uint8_t**)&k.h_state, hb))
      return MANTIS_ERR_OOM;
    k.view_cap = N;
  }
  if (slots > k.slot_cap) {
    k.slot_cap = 0;
    if (refine_grow(c, (ic::Slot**)&k.d_slots, slots)) return MANTIS_ERR_OOM;
    k.slot_cap = slots;
  }
  if (racc > k.racc_cap) {
    k.racc_cap = 0;
    if (refine_grow(c, &k.d_recAcc, racc)) return MANTIS_ERR_OOM;
    k.racc_cap = racc;
  }
  return MANTIS_OK;
}

mantis_status icalib_impl(Ctx* c, const mantis_image* cams, int32_t N, int32_t C, const double* T_in,
                          const mantis_refine_params* p, const mantis_icalib_params* ip, double* T_out,
                          mantis_icalib_result* out) {
  if (!cams || !T_in || !p || !ip || !T_out || !out) return icalib_fail(c, "null argument");
  if (ip->struct_size != (int32_t)sizeof(mantis_icalib_params))
    return icalib_fail(c, "icalib_params.struct_size mismatch");
  if (N > ic::kMaxViews) return icalib_fail(c, "n_rigs exceeds 256");
  if (mantis_status e = refine_check(c, cams, N, C, p)) return e;
  const uint32_t fm = (uint32_t)ip->free_cams, all = (1u << C) - 1u;
  if (fm & ~all) return icalib_fail(c, "free_cams has a bit at or above cams_per_rig");
  if (fm == 0) return icalib_fail(c, "free_cams names no camera");
  if (ip->param_mask < 1 || ip->param_mask > 0xFF) return icalib_fail(c, "param_mask outside 1..0xFF");
  if (ip->min_obs_cam < 8) return icalib_fail(c, "min_obs_cam must be >= 8");
  for (size_t i = 0; i < 16 * (size_t)N; i++)
    if (!std::isfinite(T_in[i])) return icalib_fail(c, "T_w_b_in is not finite");
  for (int k = 0; k < C; k++) {
    for (int e = 0; e < 16; e++)
      if (!std::isfinite(cams[k].T_base_cam[e])) return icalib_fail(c, "T_base_cam is not finite");
    for (int e = 0; e < 9; e++)
      if (!std::isfinite(cams[k].K[e])) return icalib_fail(c, "K is not finite");
    for (int e = 0; e < 4; e++)
      if (!std::isfinite(cams[k].D[e])) return icalib_fail(c, "D is not finite");
    const mk::Cam cm = cam_from(cams[k]);
    if (!(cm.fx > 0) || !(cm.fy > 0) || !std::isfinite(cm.fx) || !std::isfinite(cm.fy) || !std::isfinite(cm.cx) ||
        !std::isfinite(cm.cy))
      return icalib_fail(c, "K: fx and fy must be > 0 and finite as floats");
  }
  for (int r = 1; r < N; r++)
    for (int k = 0; k < C; k++) {
      const mantis_image &v = cams[r * C + k], &v0 = cams[k];
      if (std::memcmp(v.T_base_cam, v0.T_base_cam, sizeof(v0.T_base_cam)) != 0)
        return icalib_fail(c, "T_base_cam of a view differs from view 0's");
      if (std::memcmp(v.K, v0.K, sizeof(v0.K)) != 0) return icalib_fail(c, "K of a view differs from view 0's");
      if (std::memcmp(v.D, v0.D, sizeof(v0.D)) != 0) return icalib_fail(c, "D of a view differs from view 0's");
    }

  const int I = p->iterations, n = N * C;
  Ctx::Icalib& k = c->ib;
  k.rigs = 0;  // no record until this call has finished
  if (mantis_status e = refine_flags(c, p->landmark_pitch)) return e;
  if (mantis_status e = icalib_workspace(c, N, C, I, p->record != 0)) return e;
  const int nc = c->rf.n_cand;

  mk::IcalibState* h_st = (mk::IcalibState*)k.h_state;
  double* h_T = (double*)(h_st + 1);
  double* h_acc = h_T + 16 * (size_t)k.view_cap;
  int32_t* h_cnt = (int32_t*)(h_acc + (size_t)ic::kAcc * k.view_cap * ic::kMaxCams);
  std::memset(h_st, 0, sizeof(*h_st));
  h_st->res.n_cand = nc;
  h_st->res.n_rigs = N;
  h_st->res.n_cams = C;
  h_st->res.free_cams = ip->free_cams;
  h_st->res.param_mask = ip->param_mask;
  for (int q = 0; q < C; q++) {
    double th[ic::kP];
    ic::cam_to(cam_from(cams[q]), th);  // K rounded to float, D as given
    for (int e = 0; e < 4; e++) {
      h_st->res.K[q][e] = th[e];
      h_st->res.D[q][e] = th[4 + e];
    }
    std::memcpy(h_st->Tbc[q], cams[q].T_base_cam, sizeof(double) * 16);
  }
  std::memcpy(h_T, T_in, sizeof(double) * 16 * (size_t)N);

  int W, H;
  mantis_status st = stage_frames(c, cams, n, W, H);
  if (st != MANTIS_OK) return st;
  HIP_OK(hipMemcpyAsync(k.d_state, h_st, sizeof(mk::IcalibState), hipMemcpyHostToDevice, c->s));
  HIP_OK(hipMemcpyAsync(k.d_T, h_T, sizeof(double) * 16 * (size_t)N, hipMemcpyHostToDevice, c->s));

  mk::IcalibArgs a{};
  a.cand = c->rf.d_cand;
  a.st = (mk::IcalibState*)k.d_state;
  a.T = k.d_T;
  a.slots = (ic::Slot*)k.d_slots;
  a.acc = k.d_acc;
  a.recAcc = p->record ? k.d_recAcc : nullptr;
  a.cnt = k.d_cnt;
  a.Y = k.d_Y;
  a.Wt = k.d_Wt;
  a.pd = k.d_pd;
  a.recT = k.d_recT;
  a.recKD = k.d_recKD;
  a.pass_slots = p->record ? (size_t)n * nc : 0;
  a.C = C;
  a.n_cand = nc;
  a.I = I;
  a.N = N;
  a.min_obs = p->min_obs;
  a.min_obs_cam = ip->min_obs_cam;
  a.free_cams = fm;
  a.param_mask = (uint32_t)ip->param_mask;
  int fcam[ic::kMaxCams] = {0};
  a.F = cal::free_list(fm, C, fcam);
  for (int q = 0; q < ic::kMaxCams; q++) a.fcam[q] = fcam[q];
  a.nS = ic::kP * a.F;
  a.win = rfn::Window{p->half_window, p->white_thresh, p->min_weight, 0};
  a.lambda = p->lambda;
  const Landmarks L = lmk_of(c);
  mark(c, "start");
  const dim3 grid((nc + mk::kRefineCands - 1) / mk::kRefineCands, C, N);
  for (int pass = 0; pass <= I; pass++) {
    if (nc > 0) {
      mk::k_icalib_obs<<<grid, 256, 0, c->s>>>(c->d_frames, L, a, pass);
      HIP_OK(hipGetLastError());
    }
    mark(c, "icalib_obs/k_icalib_obs");
    mk::k_icalib_rig<<<N, 256, 0, c->s>>>(a, pass);
    HIP_OK(hipGetLastError());
    mark(c, "icalib_rig/k_icalib_rig");
    mk::k_icalib_solve<<<1, 256, 0, c->s>>>(a, pass);
    HIP_OK(hipGetLastError());
    mark(c, "icalib_solve/k_icalib_solve");
  }
  HIP_OK(hipMemcpyAsync(h_st, k.d_state, sizeof(mk::IcalibState), hipMemcpyDeviceToHost, c->s));
  HIP_OK(hipMemcpyAsync(h_T, k.d_T, sizeof(double) * 16 * (size_t)N, hipMemcpyDeviceToHost, c->s));
  HIP_OK(hipMemcpyAsync(h_acc, k.d_acc, sizeof(double) * ic::kAcc * (size_t)n, hipMemcpyDeviceToHost, c->s));
  HIP_OK(hipMemcpyAsync(h_cnt, k.d_cnt, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->s));
  HIP_OK(wait_stream(c, n));
  finish_profile(c);
  ic::conclude(h_acc, h_cnt, N, C, fm, (uint32_t)ip->param_mask, p->min_obs, ip->min_obs_cam, p->max_rms, h_st->res);
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
  const Ctx::Icalib& k = c->ib;
  if (!k.rigs || !k.record) {
    c->err = "icalib record: the last intrinsic calibration kept none (params.record = 1)";
    return MANTIS_ERR_STATE;
  }
  if (rig < 0 || rig >= k.rigs || pass < 0 || pass > k.runs)
    return icalib_fail(c, "record: rig or pass out of range (0 .. iterations_run)");
  const size_t ns = (size_t)k.C * k.cands, pr = (size_t)pass * k.rigs + rig;
  if (T_w_b) HIP_OK(hipMemcpy(T_w_b, k.d_recT + pr * 16, sizeof(double) * 16, hipMemcpyDeviceToHost));
  if (KD)
    HIP_OK(hipMemcpy(KD, k.d_recKD + (size_t)pass * k.C * ic::kP, sizeof(double) * ic::kP * k.C, hipMemcpyDeviceToHost));
  if (acc120)
    HIP_OK(hipMemcpy(acc120, k.d_recAcc + pr * k.C * ic::kAcc, sizeof(double) * ic::kAcc * k.C, hipMemcpyDeviceToHost));
  if ((codes || Sw || Skw || rows) && ns > 0) {
    std::vector<ic::Slot> hs(ns);
    HIP_OK(hipMemcpy(hs.data(), (const ic::Slot*)k.d_slots + pr * ns, sizeof(ic::Slot) * ns, hipMemcpyDeviceToHost));
    for (size_t q = 0; q < ns; q++) {
      if (codes) codes[q] = hs[q].code;
      if (Sw) Sw[q] = hs[q].Sw;
      if (Skw) Skw[q] = hs[q].Skw;
      if (rows) std::memcpy(rows + ic::kRow * q, hs[q].row, sizeof(double) * ic::kRow);
    }
  }
  return MANTIS_OK;
}

}  // extern "C"
