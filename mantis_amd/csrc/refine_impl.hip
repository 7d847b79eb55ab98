// Line refinement: Gauss-Newton on the grid lines from a pose prior
// (mantis_refine / mantis_refine_batch, include/mantis.h). Included by api.hip
// after mcl_color_impl.hip (shares its Ctx and frame staging). The rules --
// line flags, one observation, the end of a pass, the gate and the covariance
// -- are in mk_refine.h (shared with the host build of the tests).
//
// Device work of one call of I iterations, all on the context stream:
//   per pass k = 0 .. I:  k_refine_obs   the (camera, candidate) slots at T_k
//                         k_refine_step  M^T M over the rig's slots, the gates,
//                                        the solve, T_k+1 (pass I: no solve)
//                         (k_refine_step_robust, refine_robust_impl.hip, in its
//                         place when mantis_refine_set_robust switched it on)
// = 2 (I + 1) launches, then one D2H copy of the rigs' states (and one of the
// robust stats). Every hand-off
// between blocks -- the slots the observation blocks write for the rig's step
// block, the pose that block writes for the next observation blocks -- crosses
// a kernel boundary: no last-block counter, no flag polled inside a kernel, no
// hipGraph capture (as track_impl.hip). No image stage runs: the samples are
// read from the raw staged frames. Nothing is drawn.
#include "mk_refine.h"

namespace mk {

namespace rfn = refine;

struct RefineRig {  // one rig between the launches, and what comes back
  mantis_refine_result res;  // res.T_w_b = the current pose
  double acc28[28];          // of the last pass taken
  int32_t done, pad;
};

struct RefineArgs {
  const GnCam* gncam;   // per frame: inverse(T_base_cam)
  const int32_t* cand;  // n_cand: landmark | axis << 16
  RefineRig* st;        // rigs
  rfn::Slot* slots;     // [pass][rig][C n_cand]; pass_slots = the stride between passes (record) or 0
  double* recT;         // [pass][rig][16]: the pose each pass observed at
  double* recAcc;       // [pass][rig][28]
  size_t pass_slots;
  int32_t C, n_cand, I, n_rigs, min_obs;
  int32_t rig_stride;   // frame of (rig, cam) = rig * rig_stride + cam: C, or 0 when the rigs share C frames
  rfn::Window win;
  double lambda;
};

constexpr int kRefineCands = 32;  // candidates of a k_refine_obs block: 4 trips of 4 waves x 2

// One candidate's window in one 32-lane half, at the geometry g (gcode: what
// rfn::geom returned; tg: the landmark's target colour; npx = W H). Lane
// l <= 2 R of the half (active) is sample k = l - R, with one distort and one
// pixel load; the caller forms k and active once, before its candidate loop.
// The outside vote, Sw and Skw are integer sums by __shfl_xor inside the half,
// w_lo and w_hi the weights of the window's two ends; all five come back in
// every lane of the half. Every lane of the wave executes the shuffles: call
// it outside any lane-divergent branch.
__device__ __forceinline__ void refine_window(const Cam& cm, const uint8_t* bgr, int W, int H, int npx, const int* tg,
                                              const rfn::Geom& g, int gcode, double s, int k, bool active,
                                              const rfn::Window& win, int& outside, int32_t& Sw, int32_t& Skw,
                                              int32_t& w_lo, int32_t& w_hi) {
  int x = 0, y = 0;
  outside = 0;
  if (!gcode && active) outside = rfn::sample_px(cm, g, k, s, W, H, &x, &y, nullptr, nullptr) ? 0 : 1;
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) outside |= __shfl_xor(outside, m, 32);
  int32_t w = 0;
  if (!gcode && active && !outside) {  // 0 <= x < W, 0 <= y < H: the pixel is inside the frame
    const uint32_t pv = load_bgr(bgr, y * W + x, npx);
    w = rfn::px_weight((int)(pv & 0xffu), (int)((pv >> 8) & 0xffu), (int)((pv >> 16) & 0xffu), tg, win.white_thresh);
  }
  Sw = w;
  Skw = k * w;
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) {
    Sw += __shfl_xor(Sw, m, 32);
    Skw += __shfl_xor(Skw, m, 32);
  }
  w_lo = __shfl(w, 0, 32);
  w_hi = __shfl(w, 2 * win.R, 32);
}

// Block (candidate chunk, camera, rig): each wave takes two candidates at a
// time, one per 32-lane half; lane l <= 2 R of a half is sample k = l - R. The
// pose and the camera come from the grid and the kernel arguments (rig_stride:
// the mode path of mcl_refine_impl.hip reads the same C frames for every rig),
// so they are wave-uniform (scalar) loads; the candidate's geometry (a few
// dozen FP64 operations) is redone by every lane of the half rather than
// broadcast. One distort and one pixel load per lane, integer sums by
// __shfl_xor inside the half, one plain store of the slot by lane 0 of the
// half: every slot has exactly one writer.
__global__ __launch_bounds__(256) void k_refine_obs(const FrameDesc* __restrict__ frames, Landmarks lmk, RefineArgs a,
                                                    int pass) {
  const int chunk = blockIdx.x, cam = blockIdx.y, rig = blockIdx.z;
  const RefineRig& S = a.st[rig];
  if (S.done) return;  // block-uniform: the rig stopped in an earlier pass
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, l = lane & 31;
  const int f = rig * a.rig_stride + cam;
  const Cam cm = frames[f].cam;
  const uint8_t* bgr = frames[f].bgr;
  const int W = frames[f].w, H = frames[f].h, npx = W * H;
  const GnCam gc = a.gncam[f];
  double Rt[9], tw[3];
  rfn::pose_parts(S.res.T_w_b, Rt, tw);
  const double s = 1.0 / cm.fx;
  const int k = l - a.win.R;
  const bool active = l <= 2 * a.win.R;
  rfn::Slot* out = a.slots + (size_t)pass * a.pass_slots + (size_t)(rig * a.C + cam) * a.n_cand;
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
    int outside;
    int32_t Sw, Skw, w_lo, w_hi;
    refine_window(cm, bgr, W, H, npx, tg, g, gcode, s, k, active, a.win, outside, Sw, Skw, w_lo, w_hi);
    if (l == 0 && live) {
      rfn::Slot o;
      rfn::finish(gcode, outside != 0, w_lo, w_hi, Sw, Skw, a.win.min_weight, s, g, o);
      out[ci] = o;
    }
  }
}

// The 7-column accumulation of the step kernels (k_refine_step,
// k_refine_step_robust, k_smooth_acc): one block of four waves per rig builds
// M^T M of M = [J | r] over the rig's slots with v_mfma_f64_16x16x4f64, four
// rows per instruction (the tile's entry (i, j) is in lane (i & 3) * 16 + j,
// register i >> 2), and sums the waves' tiles in wave order (as gn_acc_block).
//
// One wave's trips over the n rows of the slots sl, kk = lane >> 4 and
// m = lane & 15: eight trips' loads in flight before their MFMAs (a loop of one
// trip waited for one 72-byte-strided load per MFMA); trips past the end add
// exact zeros. kW: row r times sqw[r], its sqrt(w), from LDS.
template <bool kW>
__device__ __forceinline__ void refine_trips(const rfn::Slot* sl, const double* sqw, int n, int wave, int kk, int m,
                                             v4d& acc) {
  constexpr int kU = 8;
  for (int base = wave * 4; base < n; base += 16 * kU) {
    double v[kU];
#pragma unroll
    for (int u = 0; u < kU; u++) {
      const int r = base + 16 * u + kk;
      if constexpr (kW) v[u] = (r < n && m < 7) ? sl[r].row[m] * sqw[r] : 0.0;
      else v[u] = (r < n && m < 7) ? sl[r].row[m] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kU; u++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u], v[u], acc, 0, 0, 0);
  }
}
// the code-0 rows the block's threads count among `rows` slots, summed over the wave (in every lane)
__device__ __forceinline__ int32_t refine_count(const rfn::Slot* sl, int rows, int t) {
  int32_t n = 0;
  for (int r = t; r < rows; r += 256) n += sl[r].code == 0;
#pragma unroll
  for (int q = 32; q >= 1; q >>= 1) n += __shfl_xor(n, q, 64);
  return n;
}
// a wave's tile into red; after the block's barrier one thread sums the four tiles into acc28
__device__ __forceinline__ void refine_tile(double (*red)[16][16], int wave, int kk, int m, const v4d& acc) {
  for (int r = 0; r < 4; r++) red[wave][kk + 4 * r][m] = acc[r];
}
__device__ __forceinline__ void refine_sum28(const double (*red)[16][16], double* acc28) {
  int e = 0;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++) acc28[e++] = red[0][i][j] + red[1][i][j] + red[2][i][j] + red[3][i][j];
  for (int i = 0; i < 6; i++) acc28[21 + i] = red[0][i][6] + red[1][i][6] + red[2][i][6] + red[3][i][6];
  acc28[27] = red[0][6][6] + red[1][6][6] + red[2][6][6] + red[3][6][6];
}
// the pass record of a rig: the pose the pass observed at and its acc28, also kept in the rig's state
__device__ __forceinline__ void refine_record(const RefineArgs& a, RefineRig& S, int rig, int pass,
                                              const double* acc28) {
  double* rT = a.recT + ((size_t)pass * a.n_rigs + rig) * 16;
  double* rA = a.recAcc + ((size_t)pass * a.n_rigs + rig) * 28;
  for (int i = 0; i < 16; i++) rT[i] = S.res.T_w_b[i];
  for (int i = 0; i < 28; i++) rA[i] = S.acc28[i] = acc28[i];
}

// One block per rig: the accumulation above over the rig's C n_cand slots;
// n_obs is a block count; thread 0 ends the pass (rfn::end_pass: gates,
// gn_solve6, T_k+1) and writes the pass record. Pass I solves nothing.
__global__ __launch_bounds__(256) void k_refine_step(RefineArgs a, int pass) {
  __shared__ double red[4][16][16];
  __shared__ int32_t cnt[4];
  const int rig = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  RefineRig& S = a.st[rig];
  if (S.done) return;
  const int rows = a.C * a.n_cand;
  const rfn::Slot* sl = a.slots + (size_t)pass * a.pass_slots + (size_t)rig * rows;
  v4d acc = {0, 0, 0, 0};
  const int kk = lane >> 4, m = lane & 15;
  refine_trips<false>(sl, nullptr, rows, wave, kk, m, acc);
  const int32_t n = refine_count(sl, rows, t);
  if (lane == 0) cnt[wave] = n;
  refine_tile(red, wave, kk, m, acc);
  __syncthreads();
  if (t == 0) {
    double acc28[28];
    refine_sum28(red, acc28);
    const int32_t n_obs = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    refine_record(a, S, rig, pass, acc28);
    S.done = rfn::end_pass(acc28, n_obs, pass, a.I, a.min_obs, a.lambda, S.res) ? 1 : 0;
  }
}

}  // namespace mk

#include "refine_robust_impl.hip"

namespace {

namespace rfn = mk::refine;

// an argument error of the entry point that calls itself `prefix`
mantis_status line_fail(Ctx* c, const char* prefix, const char* what) {
  c->err = std::string(prefix) + ": " + what;
  return MANTIS_ERR_ARG;
}
mantis_status refine_fail(Ctx* c, const char* what) { return line_fail(c, "refine", what); }

// ns slots (S: rfn::Slot or a calibration's, rows of kRow doubles) from the device into the caller's arrays
template <class S, int kRow>
mantis_status slots_scatter(Ctx* c, const S* d_slots, size_t ns, int32_t* codes, int32_t* Sw, int32_t* Skw,
                            double* rows) {
  if (!(codes || Sw || Skw || rows) || ns == 0) return MANTIS_OK;
  std::vector<S> hs(ns);
  HIP_OK(hipMemcpy(hs.data(), d_slots, sizeof(S) * ns, hipMemcpyDeviceToHost));
  for (size_t k = 0; k < ns; k++) {
    if (codes) codes[k] = hs[k].code;
    if (Sw) Sw[k] = hs[k].Sw;
    if (Skw) Skw[k] = hs[k].Skw;
    if (rows) std::memcpy(rows + kRow * k, hs[k].row, sizeof(double) * kRow);
  }
  return MANTIS_OK;
}

// the line flags of the current map at `pitch`, and the candidate list on the device
mantis_status refine_flags(Ctx* c, double pitch) {
  Ctx::Refine& r = c->rf;
  const int n = c->nw + c->nr + c->ng;
  if (r.pitch == pitch && (int)r.flags.size() == n) return MANTIS_OK;
  r.pitch = 0;
  r.flags.assign(n, 0);
  rfn::line_flags(c->h_lm.data(), n, pitch, r.flags.data());
  std::vector<int32_t> cand(n > 0 ? n : 1);
  r.n_cand = rfn::candidates(r.flags.data(), n, cand.data());
  HIP_OK(hipStreamSynchronize(c->s));  // nothing of an earlier call still reads the list
  if (r.d_cand.grow(c, (size_t)r.n_cand)) return MANTIS_ERR_OOM;
  if (r.n_cand > 0) HIP_OK(hipMemcpy(r.d_cand, cand.data(), sizeof(int32_t) * r.n_cand, hipMemcpyHostToDevice));
  r.pitch = pitch;
  return MANTIS_OK;
}

// workspaces for a call of R rigs x C cameras on F frames, I iterations; robust: the switch is on
mantis_status refine_workspace(Ctx* c, int R, int C, int F, int I, bool record, bool robust) {
  Ctx::Refine& r = c->rf;
  const size_t slots = (record ? (size_t)I + 1 : 1) * R * C * std::max(r.n_cand, 1);
  const size_t rslots = robust && record ? slots : 0;  // keys and weights: only as a record
  const size_t rstats = robust ? (size_t)R : 0;
  if (R > r.rig_cap || F > r.cam_cap || slots > r.d_slots.capacity() || rslots > r.d_rkeys.capacity() ||
      rstats > r.d_rstats.capacity())
    HIP_OK(hipStreamSynchronize(c->s));
  if (R > r.rig_cap || F > r.cam_cap) {
    const int rc = std::max(R, r.rig_cap), cc = std::max(F, r.cam_cap);
    r.rig_cap = r.cam_cap = 0;
    const size_t hb = sizeof(mk::RefineRig) * rc + sizeof(mk::GnCam) * cc;
    if (r.d_state.alloc(c, (size_t)rc) || r.d_gncam.alloc(c, (size_t)cc) ||
        r.d_recT.alloc(c, (size_t)(rfn::kMaxIterations + 1) * rc * 16) ||
        r.d_recAcc.alloc(c, (size_t)(rfn::kMaxIterations + 1) * rc * 28) || r.h_state.alloc(c, hb))
      return MANTIS_ERR_OOM;
    r.rig_cap = rc;
    r.cam_cap = cc;
  }
  if (r.d_slots.grow(c, slots) || r.d_rstats.grow(c, rstats) || r.h_rstats.grow(c, rstats) ||
      r.d_rkeys.grow(c, rslots) || r.d_rweights.grow(c, rslots))
    return MANTIS_ERR_OOM;
  return MANTIS_OK;
}

// The checks every solver on the grid lines shares, in the order its errors
// fire: the window and solve fields (Pm: mantis_refine_params or
// mantis_smooth_params, which name them alike), then, behind the caller's own
// fields, the record flag and the n frames (cams: not null).
template <class Pm>
mantis_status line_check_fields(Ctx* c, const char* prefix, const Pm* p) {
  if (p->iterations < 0 || p->iterations > rfn::kMaxIterations) return line_fail(c, prefix, "iterations outside 0..10");
  if (p->half_window < 1 || p->half_window > rfn::kMaxHalfWindow)
    return line_fail(c, prefix, "half_window outside 1..15");
  if (p->white_thresh < 1 || p->white_thresh > 195075) return line_fail(c, prefix, "white_thresh outside 1..195075");
  if (p->min_weight < 1) return line_fail(c, prefix, "min_weight must be >= 1");
  if (p->min_obs < 6) return line_fail(c, prefix, "min_obs must be >= 6");
  if (!(p->lambda >= 0) || !std::isfinite(p->lambda)) return line_fail(c, prefix, "lambda must be finite and >= 0");
  if (!(p->landmark_pitch > 0) || !std::isfinite(p->landmark_pitch))
    return line_fail(c, prefix, "landmark_pitch must be finite and > 0");
  if (std::isnan(p->max_rms)) return line_fail(c, prefix, "max_rms is NaN");
  return MANTIS_OK;
}
mantis_status line_check_frames(Ctx* c, const char* prefix, int32_t record, const mantis_image* cams, int n) {
  if (record != 0 && record != 1) return line_fail(c, prefix, "record must be 0 or 1");
  for (int i = 0; i < n; i++) {
    if (cams[i].width != cams[0].width || cams[i].height != cams[0].height)
      return line_fail(c, prefix, "all frames of a call must share one size");
    if (!cams[i].bgr || cams[i].step_bytes < 3 * cams[i].width)
      return line_fail(c, prefix, "bgr8 image with step >= 3*width required");
  }
  if (cams[0].width <= 2 || cams[0].height <= 2 || cams[0].width > c->Wmax || cams[0].height > c->Hmax)
    return line_fail(c, prefix, "image size outside [3, max]");
  return MANTIS_OK;
}

// the parameter and frame checks of a call of n_rigs x C frames (cams, p: not null)
mantis_status refine_check(Ctx* c, const mantis_image* cams, int32_t n_rigs, int32_t C, const mantis_refine_params* p) {
  if (p->struct_size != (int32_t)sizeof(mantis_refine_params)) return refine_fail(c, "params.struct_size mismatch");
  if (!c->d_lm || c->nw + c->nr + c->ng <= 0) return refine_fail(c, "map not set (mantis_set_map)");
  if (n_rigs <= 0 || C <= 0) return refine_fail(c, "n_rigs and cams_per_rig must be positive");
  if (C > rfn::kMaxCams) return refine_fail(c, "cams_per_rig exceeds 8");
  if ((int64_t)n_rigs * C > c->F) return refine_fail(c, "n_rigs x cams_per_rig exceeds max_cams");
  if (mantis_status e = line_check_fields(c, "refine", p)) return e;
  return line_check_frames(c, "refine", p->record, cams, n_rigs * C);
}

// The device work of a checked call: n_rigs rigs of C cameras from T_in. Rig r
// reads frames r * C .. r * C + C - 1 of n_rigs x C (shared = false), or every
// rig the same C frames, staged once (shared = true: the modes of
// mantis_mcl_refine_modes).
mantis_status refine_run(Ctx* c, const mantis_image* cams, int32_t n_rigs, int32_t C, bool shared, const double* T_in,
                         const mantis_refine_params* p, mantis_refine_result* out) {
  const int I = p->iterations, n = shared ? C : n_rigs * C;
  Ctx::Refine& r = c->rf;
  r.rigs = 0;  // no record until this call has finished
  const bool robust = r.robust.loss != rfn::kLossNone;  // as mantis_refine_set_robust left it
  if (mantis_status e = refine_flags(c, p->landmark_pitch)) return e;
  if (mantis_status e = refine_workspace(c, n_rigs, C, n, I, p->record != 0, robust)) return e;

  mk::RefineRig* h_st = (mk::RefineRig*)r.h_state.get();
  mk::GnCam* h_gc = (mk::GnCam*)(h_st + r.rig_cap);
  for (int k = 0; k < n_rigs; k++) {
    std::memset(&h_st[k], 0, sizeof(h_st[k]));
    std::memcpy(h_st[k].res.T_w_b, T_in + 16 * (size_t)k, sizeof(double) * 16);
    h_st[k].res.n_cand = r.n_cand;
  }
  for (int i = 0; i < n; i++) rfn::gncam_from(cams[i].T_base_cam, h_gc[i]);

  int W, H;
  mantis_status st = stage_frames(c, cams, n, W, H);
  if (st != MANTIS_OK) return st;
  HIP_OK(hipMemcpyAsync(r.d_state, h_st, sizeof(mk::RefineRig) * n_rigs, hipMemcpyHostToDevice, c->s));
  HIP_OK(hipMemcpyAsync(r.d_gncam, h_gc, sizeof(mk::GnCam) * n, hipMemcpyHostToDevice, c->s));

  mk::RefineArgs a;
  a.gncam = (const mk::GnCam*)r.d_gncam;
  a.cand = r.d_cand;
  a.st = (mk::RefineRig*)r.d_state;
  a.slots = (rfn::Slot*)r.d_slots;
  a.recT = r.d_recT;
  a.recAcc = r.d_recAcc;
  a.pass_slots = p->record ? (size_t)n_rigs * C * r.n_cand : 0;
  a.C = C;
  a.n_cand = r.n_cand;
  a.I = I;
  a.n_rigs = n_rigs;
  a.min_obs = p->min_obs;
  a.rig_stride = shared ? 0 : C;
  a.win = rfn::Window{p->half_window, p->white_thresh, p->min_weight, 0};
  a.lambda = p->lambda;
  mk::RobustArgs rb{};
  if (robust) {
    rb.stats = r.d_rstats;
    rb.keys = p->record ? r.d_rkeys : nullptr;
    rb.weights = p->record ? r.d_rweights : nullptr;
    rb.rb = rfn::Robust{r.robust.loss, 0, r.robust.tuning, r.robust.scale_floor};
    HIP_OK(hipMemsetAsync(r.d_rstats, 0, sizeof(mantis_refine_robust_stats) * n_rigs, c->s));
  }
  const Landmarks L = lmk_of(c);
  mark(c, "start");
  const dim3 grid((r.n_cand + mk::kRefineCands - 1) / mk::kRefineCands, C, n_rigs);
  for (int pass = 0; pass <= I; pass++) {
    if (r.n_cand > 0) {  // a map without candidates: the step sees no rows
      mk::k_refine_obs<<<grid, 256, 0, c->s>>>(c->d_frames, L, a, pass);
      HIP_OK(hipGetLastError());
    }
    mark(c, "refine_obs/k_refine_obs");
    if (robust) {
      mk::k_refine_step_robust<<<n_rigs, 256, 0, c->s>>>(a, rb, pass);
      HIP_OK(hipGetLastError());
      mark(c, "refine_step/k_refine_step_robust");
    } else {
      mk::k_refine_step<<<n_rigs, 256, 0, c->s>>>(a, pass);
      HIP_OK(hipGetLastError());
      mark(c, "refine_step/k_refine_step");
    }
  }
  HIP_OK(hipMemcpyAsync(h_st, r.d_state, sizeof(mk::RefineRig) * n_rigs, hipMemcpyDeviceToHost, c->s));
  if (robust)
    HIP_OK(hipMemcpyAsync(r.h_rstats, r.d_rstats, sizeof(mantis_refine_robust_stats) * n_rigs, hipMemcpyDeviceToHost,
                          c->s));
  HIP_OK(wait_stream(c, n));
  finish_profile(c);
  r.runs.assign(n_rigs, 0);
  for (int k = 0; k < n_rigs; k++) {
    rfn::conclude(h_st[k].acc28, p->min_obs, p->max_rms, h_st[k].res);
    out[k] = h_st[k].res;
    r.runs[k] = h_st[k].res.iterations_run;
  }
  r.rigs = n_rigs;
  r.C = C;
  r.I = I;
  r.record = p->record;
  r.cands = r.n_cand;
  r.rec_loss = r.robust.loss;
  for (int k = 0; robust && k < n_rigs; k++) r.h_rstats[k].loss = r.robust.loss;
  return MANTIS_OK;
}

// the setting's checks (p: not null, loss != 0)
mantis_status robust_check(Ctx* c, const mantis_refine_robust_params* p) {
  if (!(p->tuning > 0) || !std::isfinite(p->tuning)) return refine_fail(c, "robust.tuning must be finite and > 0");
  if (!(p->scale_floor > 0) || !std::isfinite(p->scale_floor))
    return refine_fail(c, "robust.scale_floor must be finite and > 0");
  return MANTIS_OK;
}

mantis_status refine_impl(Ctx* c, const mantis_image* cams, int32_t n_rigs, int32_t C, const double* T_in,
                          const mantis_refine_params* p, mantis_refine_result* out) {
  if (!cams || !T_in || !p || !out) return refine_fail(c, "null argument");
  if (mantis_status e = refine_check(c, cams, n_rigs, C, p)) return e;
  for (int i = 0; i < 16 * n_rigs; i++)
    if (!std::isfinite(T_in[i])) return refine_fail(c, "T_w_b_in is not finite");
  return refine_run(c, cams, n_rigs, C, false, T_in, p, out);
}

}  // namespace

extern "C" {

void mantis_default_refine_params(mantis_refine_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(mantis_refine_params);
  p->iterations = 4;
  p->half_window = 12;
  p->white_thresh = 3 * 64 * 64;
  p->min_weight = 24576;
  p->min_obs = 12;
  p->lambda = 0;
  p->landmark_pitch = 0.08;
  p->max_rms = 0;
  p->record = 0;
}

void mantis_refine_sizes(int32_t* params_bytes, int32_t* result_bytes) {
  if (params_bytes) *params_bytes = (int32_t)sizeof(mantis_refine_params);
  if (result_bytes) *result_bytes = (int32_t)sizeof(mantis_refine_result);
}

mantis_status mantis_refine_line_flags(void* ctx, double pitch, uint8_t* flags_out, int32_t n) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  if (!flags_out) return refine_fail(c, "null argument");
  if (!c->d_lm || c->nw + c->nr + c->ng <= 0) return refine_fail(c, "map not set (mantis_set_map)");
  if (!(pitch > 0) || !std::isfinite(pitch)) return refine_fail(c, "landmark_pitch must be finite and > 0");
  if (n != c->nw + c->nr + c->ng) return refine_fail(c, "line flags: n must be nw + nr + ng");
  c->rf.rigs = 0;  // a record's slot count follows the cached candidates
  if (mantis_status e = refine_flags(c, pitch)) return e;
  std::memcpy(flags_out, c->rf.flags.data(), (size_t)n);
  return MANTIS_OK;
}

mantis_status mantis_refine_batch(void* ctx, const mantis_image* cams, int32_t n_rigs, int32_t cams_per_rig,
                                  const double* T_w_b_in, const mantis_refine_params* p, mantis_refine_result* out) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  return refine_impl(c, cams, n_rigs, cams_per_rig, T_w_b_in, p, out);
}

mantis_status mantis_refine(void* ctx, const mantis_image* cams, int32_t n_cams, const mantis_motion* motion,
                            const mantis_refine_params* p, mantis_result* out, mantis_refine_result* rout) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  if (!out) return refine_fail(c, "null argument");
  if (!c->has_prior) {
    c->err = "refine: no prior pose (mantis_set_prior_pose, or a published mantis_process call)";
    return MANTIS_ERR_STATE;
  }
  double start[16];
  const double* pq = motion ? motion->delta_quat_xyzw : nullptr;
  if (motion && pq[0] * pq[0] + pq[1] * pq[1] + pq[2] * pq[2] + pq[3] * pq[3] >= 0.5) {  // as mantis_track
    double D[16];
    quat_to_mat4(motion->delta_quat_xyzw, motion->delta_pos, D);
    mat4_mul(c->prior_Twb, D, start);
  } else {
    std::memcpy(start, c->prior_Twb, sizeof(start));
  }
  mantis_refine_result tmp;
  mantis_refine_result* rr = rout ? rout : &tmp;
  const mantis_status st = refine_impl(c, cams, 1, n_cams, start, p, rr);
  if (st != MANTIS_OK) return st;
  std::memset(out, 0, sizeof(*out));
  out->status = MANTIS_OK;
  out->num_particles = rr->n_obs[rr->iterations_run];
  out->rng_state_after = c->rng_state;
  if (!rr->refined) return MANTIS_OK;  // publish = 0, the prior stays: the caller falls back to mantis_process
  std::memcpy(c->prior_Twb, rr->T_w_b, sizeof(c->prior_Twb));
  out->publish = 1;
  const Xf T = mk::track::xf_from_mat4(rr->T_w_b);
  const Quat q = basis_to_quat(T.R);  // Matrix3x3::getRotation, as the published poses of the pipeline
  out->orientation_xyzw[0] = q.x; out->orientation_xyzw[1] = q.y;
  out->orientation_xyzw[2] = q.z; out->orientation_xyzw[3] = q.w;
  for (int i = 0; i < 3; i++) out->position[i] = T.t[i];
  std::memcpy(out->covariance, rr->covariance, sizeof(out->covariance));
  out->weight = rr->rms[rr->iterations_run];
  return MANTIS_OK;
}

mantis_status mantis_get_refine_record(void* ctx, int32_t rig, int32_t pass, double* T_w_b, int32_t* codes,
                                       int32_t* Sw, int32_t* Skw, double* rows, double* acc28) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  const Ctx::Refine& r = c->rf;
  if (!r.rigs || !r.record) {
    c->err = "refine record: the last refine call kept none (params.record = 1)";
    return MANTIS_ERR_STATE;
  }
  if (rig < 0 || rig >= r.rigs || pass < 0 || pass > r.runs[rig])
    return refine_fail(c, "record: rig or pass out of range (0 .. the rig's iterations_run)");
  const size_t ns = (size_t)r.C * r.cands;
  if (T_w_b)
    HIP_OK(hipMemcpy(T_w_b, r.d_recT + ((size_t)pass * r.rigs + rig) * 16, sizeof(double) * 16, hipMemcpyDeviceToHost));
  if (acc28)
    HIP_OK(hipMemcpy(acc28, r.d_recAcc + ((size_t)pass * r.rigs + rig) * 28, sizeof(double) * 28, hipMemcpyDeviceToHost));
  return slots_scatter<rfn::Slot, 7>(c, (const rfn::Slot*)r.d_slots + ((size_t)pass * r.rigs + rig) * ns, ns, codes, Sw,
                                     Skw, rows);
}

void mantis_default_refine_robust_params(int32_t loss, mantis_refine_robust_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(mantis_refine_robust_params);
  p->loss = loss;
  p->tuning = loss == rfn::kLossTukey ? 4.685 : 1.345;
  p->scale_floor = 0.25;
}

void mantis_refine_robust_sizes(int32_t* params_bytes, int32_t* stats_bytes) {
  if (params_bytes) *params_bytes = (int32_t)sizeof(mantis_refine_robust_params);
  if (stats_bytes) *stats_bytes = (int32_t)sizeof(mantis_refine_robust_stats);
}

mantis_status mantis_refine_set_robust(void* ctx, const mantis_refine_robust_params* p) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  if (!p) {
    c->rf.robust = mantis_refine_robust_params{};
    return MANTIS_OK;
  }
  if (p->struct_size != (int32_t)sizeof(mantis_refine_robust_params))
    return refine_fail(c, "robust.struct_size mismatch");
  if (p->loss < rfn::kLossNone || p->loss > rfn::kLossTukey) return refine_fail(c, "robust.loss outside 0..2");
  if (p->loss == rfn::kLossNone) {
    c->rf.robust = mantis_refine_robust_params{};
    return MANTIS_OK;
  }
  if (mantis_status e = robust_check(c, p)) return e;
  c->rf.robust = *p;
  return MANTIS_OK;
}

mantis_status mantis_get_refine_robust(void* ctx, int32_t rig, mantis_refine_robust_stats* stats) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  const Ctx::Refine& r = c->rf;
  if (!stats) return refine_fail(c, "null argument");
  if (!r.rigs || r.rec_loss == rfn::kLossNone) {
    c->err = "refine robust: no refine call yet, or the last one ran with the robust rows off";
    return MANTIS_ERR_STATE;
  }
  if (rig < 0 || rig >= r.rigs) return refine_fail(c, "robust stats: rig out of range");
  *stats = r.h_rstats[rig];
  return MANTIS_OK;
}

mantis_status mantis_get_refine_robust_record(void* ctx, int32_t rig, int32_t pass, uint32_t* keys, double* weights) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  const Ctx::Refine& r = c->rf;
  if (!r.rigs || !r.record || r.rec_loss == rfn::kLossNone) {
    c->err = "refine robust record: the last refine call kept none (robust rows on and params.record = 1)";
    return MANTIS_ERR_STATE;
  }
  if (rig < 0 || rig >= r.rigs || pass < 0 || pass > r.runs[rig])
    return refine_fail(c, "robust record: rig or pass out of range (0 .. the rig's iterations_run)");
  const size_t ns = (size_t)r.C * r.cands, off = ((size_t)pass * r.rigs + rig) * ns;
  if (keys && ns > 0) HIP_OK(hipMemcpy(keys, r.d_rkeys + off, sizeof(uint32_t) * ns, hipMemcpyDeviceToHost));
  if (weights && ns > 0) HIP_OK(hipMemcpy(weights, r.d_rweights + off, sizeof(double) * ns, hipMemcpyDeviceToHost));
  return MANTIS_OK;
}

}  // extern "C"
