// Fixed-lag smoothing: a context-held window that marginalises (mantis_lag_*,
// include/mantis.h). Included by api.hip after smooth_impl.hip: the passes are
// its kernels, launched as they are, on a window whose views, motions, prior,
// descriptors and frames stay in HBM between the pushes (Ctx::Lag). The rules
// of the slide -- the marginal of the leaving view, the whitener of its prior,
// the predicted start -- are in mk_smooth.h (shared with the host build of the
// tests).
//
// Device work of one push of I iterations, all on the context stream:
//   the C frame copies into the ring slot the slide frees, one small upload
//   k_lag_slide      one block: the marginal and its whitener (window full),
//                    the shift, the new view's row, the clean window
//   per pass p = 0 .. I:  k_refine_obs, k_smooth_acc, k_smooth_solve
// = 1 + 3 (I + 1) launches, then one D2H copy (the head with T_p / Cov_p, the
// views' states, the final blocks). Every hand-off crosses a kernel boundary:
// no polled flag, no last-block counter, no hipGraph.
#include "mk_smooth.h"

namespace mk {

struct LagHead {  // the window between the pushes, and what comes back first
  SmoothWin win;
  double Tp[16], Wp[36], Cov[36];  // the prior of the solve: pose, sigma_row L_c^-1, covariance
  int32_t has_prior, drop_reason, n, pad;
};

struct LagIn {  // what a push uploads
  double D[16];        // Transform of the motion into the new view (has_motion)
  double T_start[16];  // (has_start)
  double Tp[16], Wp[36], Cov[36];  // the reset's prior (load_prior, first push only)
  int32_t has_motion, has_start, first, load_prior;
  int32_t slide;  // the window is full: the oldest view leaves
  int32_t why;    // what the host knows against a prior (smo::kLagNoFactor / kLagNotOk), or kLagKept
  int32_t n_old, n_cand;
  FrameDesc fd[refine::kMaxCams];  // the new view's cameras, pointing into the ring
  GnCam gc[refine::kMaxCams];
};

struct LagArgs {
  LagHead *head, *peek;  // peek: only the marginal, into *peek (mantis_lag_get_prior); nothing else is touched
  const LagIn* in;
  RefineRig* st;   // capacity views, time order
  double* D;       // capacity x 16; the row of the newest view is zeros
  int32_t* has;    // capacity; likewise
  GnCam* gncam;    // capacity x C
  FrameDesc* fd;   // capacity x C
  const double *Hd0, *g0, *fe0, *fJ0;  // view 0's blocks and factor 0 of the last push's final pass
  double sigma_row;
  int32_t C;
};

// rows 0 .. keep - 1 of `stride` 32-bit words take the row above them. Thread t
// owns the words t, t + 64, .. of every row and walks the rows upwards, so no
// word is read by one thread and written by another.
__device__ __forceinline__ void lag_shift(uint32_t* p, int stride, int keep, int t) {
  for (int w = t; w < stride; w += 64)
    for (int k = 0; k < keep; k++) p[(size_t)k * stride + w] = p[(size_t)(k + 1) * stride + w];
}

// One block of one wave, once per push before the passes. Lane 0 runs the
// marginal (a 6 x 6 Schur complement and three Cholesky factors: about 2000
// dependent FP64 operations, once per push) and forms the new view's start; the
// wave then shifts the surviving rows down, appends the new view and leaves
// every view and the window result as a batch call's upload leaves them.
__global__ __launch_bounds__(64) void k_lag_slide(LagArgs a) {
  __shared__ double sT[16];
  const int t = threadIdx.x;
  const LagIn& in = *a.in;
  if (a.peek) {
    if (t == 0) {
      LagHead& P = *a.peek;
      P.drop_reason = smooth::marginal_prior(a.Hd0, a.g0, a.fJ0, a.fJ0 + 36, a.fe0, a.st[1].res.T_w_b, a.sigma_row, P.Tp,
                                             P.Cov, P.Wp);
      P.has_prior = P.drop_reason == smooth::kLagKept;
    }
    return;
  }
  LagHead& Hh = *a.head;
  const int n_old = in.n_old, sh = in.slide ? 1 : 0, n = n_old - sh + 1, C = a.C, v = n - 1;
  if (t == 0) {
    if (in.first) {
      Hh.has_prior = in.load_prior;
      for (int q = 0; q < 16; q++) Hh.Tp[q] = in.Tp[q];
      for (int q = 0; q < 36; q++) {
        Hh.Wp[q] = in.Wp[q];
        Hh.Cov[q] = in.Cov[q];
      }
    }
    Hh.drop_reason = smooth::kLagKept;
    if (sh) {
      int why = in.why;
      if (why == smooth::kLagKept) {
        why = smooth::marginal_prior(a.Hd0, a.g0, a.fJ0, a.fJ0 + 36, a.fe0, a.st[1].res.T_w_b, a.sigma_row, Hh.Tp, Hh.Cov,
                                     Hh.Wp);
      } else {
        for (int q = 0; q < 16; q++) Hh.Tp[q] = q % 5 == 0 ? 1.0 : 0.0;
        for (int q = 0; q < 36; q++) Hh.Cov[q] = Hh.Wp[q] = 0.0;
      }
      Hh.has_prior = why == smooth::kLagKept;
      Hh.drop_reason = why;
    }
    if (in.has_start) {
      for (int q = 0; q < 16; q++) sT[q] = in.T_start[q];
    } else {
      double T[16];
      smooth::predict_start(a.st[n_old - 1].res.T_w_b, in.D, T);  // the host asked for it only with n_old >= 1
      for (int q = 0; q < 16; q++) sT[q] = T[q];
    }
  }
  __syncthreads();
  if (sh) {  // n_old = n = the capacity: rows 1 .. n - 1 move to 0 .. n - 2
    lag_shift((uint32_t*)a.st, (int)(sizeof(RefineRig) / 4), n - 1, t);
    lag_shift((uint32_t*)a.D, 32, n - 1, t);
    lag_shift((uint32_t*)a.has, 1, n - 1, t);
    lag_shift((uint32_t*)a.gncam, C * (int)(sizeof(GnCam) / 4), n - 1, t);
    lag_shift((uint32_t*)a.fd, C * (int)(sizeof(FrameDesc) / 4), n - 1, t);
  }
  __syncthreads();
  if (t < 16) {
    a.st[v].res.T_w_b[t] = sT[t];
    if (v > 0) a.D[16 * (size_t)(v - 1) + t] = in.has_motion ? in.D[t] : 0.0;
    a.D[16 * (size_t)v + t] = 0.0;
  }
  if (t == 16) {
    if (v > 0) a.has[v - 1] = in.has_motion ? 1 : 0;
    a.has[v] = 0;
  }
  for (int w = t; w < C * (int)(sizeof(GnCam) / 4); w += 64)
    ((uint32_t*)(a.gncam + (size_t)v * C))[w] = ((const uint32_t*)in.gc)[w];
  for (int w = t; w < C * (int)(sizeof(FrameDesc) / 4); w += 64)
    ((uint32_t*)(a.fd + (size_t)v * C))[w] = ((const uint32_t*)in.fd)[w];
  __syncthreads();
  // every view keeps its pose and starts clean otherwise, as the upload of a batch call leaves it
  constexpr int kW = sizeof(RefineRig) / 4;
  constexpr int kT0 = (offsetof(RefineRig, res) + offsetof(mantis_refine_result, T_w_b)) / 4;
  constexpr int kNc = (offsetof(RefineRig, res) + offsetof(mantis_refine_result, n_cand)) / 4;
  for (int idx = t; idx < n * kW; idx += 64) {
    const int w = idx % kW;
    if (w >= kT0 && w < kT0 + 32) continue;
    ((uint32_t*)a.st)[idx] = w == kNc ? (uint32_t)in.n_cand : 0u;
  }
  for (int w = t; w < (int)(sizeof(SmoothWin) / 4); w += 64) ((uint32_t*)&Hh.win)[w] = 0u;
  __syncthreads();
  if (t == 0) {
    Hh.win.res.n_cand = in.n_cand;
    Hh.win.res.n_views = n;
    Hh.win.res.has_prior = Hh.has_prior;
    Hh.n = n;
  }
}

}  // namespace mk

namespace {

mantis_status lag_fail(Ctx* c, const char* what) { return line_fail(c, "lag", what); }

// bytes into the out buffer of a window of `cap` views
struct LagLayout {
  size_t o_st, o_Hd, o_Ho, o_peek, bytes;
};
LagLayout lag_layout(size_t cap) {
  LagLayout L;
  L.o_st = (sizeof(mk::LagHead) + 7) / 8 * 8;
  L.o_Hd = L.o_st + sizeof(mk::RefineRig) * cap;
  L.o_Ho = L.o_Hd + sizeof(double) * 36 * cap;
  L.o_peek = L.o_Ho + sizeof(double) * 36 * cap;
  L.bytes = L.o_peek + sizeof(mk::LagHead);
  return L;
}

void lag_release(Ctx::Lag& g) {
  g.ws.d_out.release();
  g.ws.h_out.release();
  g.ws.d_in.release();
  g.ws.h_in.release();
  g.ws.d_work.release();
  g.ws.d_slots.release();
  g.d_D.release();
  g.d_has.release();
  g.d_gncam.release();
  g.d_fd.release();
  g.d_ring.release();
  g.cap = 0;
}

// the window's buffers for its shape and W x H frames (the first push since a reset that changed them)
mantis_status lag_alloc(Ctx* c, int W, int H) {
  Ctx::Lag& g = c->lag;
  const int N = g.p.capacity, C = g.p.cams_per_rig, I = g.p.smooth.iterations;
  if (g.cap == N && g.C == C && g.I == I && g.W == W && g.H == H) return MANTIS_OK;
  HIP_OK(hipStreamSynchronize(c->s));
  lag_release(g);
  const LagLayout L = lag_layout(N);
  const SmoothLayout S = smooth_layout(N, 1, (size_t)N * C, (size_t)I + 1);
  if (g.ws.d_out.alloc(c, L.bytes) || g.ws.h_out.alloc(c, L.bytes) || g.ws.d_in.alloc(c, sizeof(mk::LagIn)) ||
      g.ws.h_in.alloc(c, sizeof(mk::LagIn)) || g.ws.d_work.alloc(c, S.work_doubles) || g.d_D.alloc(c, 16 * (size_t)N) ||
      g.d_has.alloc(c, (size_t)N) || g.d_gncam.alloc(c, (size_t)N * C) || g.d_fd.alloc(c, (size_t)N * C) ||
      g.d_ring.alloc(c, (size_t)N * C * W * H * 3)) {
    lag_release(g);
    return MANTIS_ERR_OOM;
  }
  g.cap = N;
  g.C = C;
  g.I = I;
  g.W = W;
  g.H = H;
  return MANTIS_OK;
}

// the arguments of k_lag_slide on the window as the last push left it
mk::LagArgs lag_args(Ctx* c) {
  Ctx::Lag& g = c->lag;
  const LagLayout L = lag_layout(g.cap);
  // the last push's workspace: a window of g.n views (the marginal is only taken of a full one)
  const SmoothLayout S = smooth_layout(g.n, 1, (size_t)g.n * g.C, (size_t)g.I + 1);
  const size_t pv = (size_t)g.I * g.n;  // pass I, view 0: where a window that ended OK keeps its final factors
  mk::LagArgs a;
  a.head = (mk::LagHead*)g.ws.d_out.get();
  a.peek = nullptr;
  a.in = (const mk::LagIn*)g.ws.d_in.get();
  a.st = (mk::RefineRig*)(g.ws.d_out + L.o_st);
  a.D = g.d_D;
  a.has = g.d_has;
  a.gncam = g.d_gncam;
  a.fd = g.d_fd;
  a.Hd0 = (const double*)(g.ws.d_out + L.o_Hd);
  a.g0 = g.ws.d_work;
  a.fe0 = g.ws.d_work + S.w_recE + 6 * pv;
  a.fJ0 = g.ws.d_work + S.w_recJ + 72 * pv;
  a.sigma_row = g.p.smooth.sigma_row;
  a.C = g.C;
  return a;
}

// what the host knows against carrying a prior out of the full window
int lag_why(const Ctx::Lag& g) {
  if (!g.has[0]) return smo::kLagNoFactor;
  if (!g.last_ok) return smo::kLagNotOk;
  return smo::kLagKept;
}

mantis_status lag_push_impl(Ctx* c, const mantis_image* cams, const mantis_motion* motion, const double* T_start,
                            mantis_smooth_result* out, mantis_smooth_view* views, mantis_lag_info* info) {
  Ctx::Lag& g = c->lag;
  if (!g.live) return lag_fail(c, "push before reset (mantis_lag_reset)");
  if (!cams || !out || !views) return lag_fail(c, "null argument");
  if (!c->d_lm || c->nw + c->nr + c->ng <= 0) return lag_fail(c, "map not set (mantis_set_map)");
  const mantis_smooth_params* p = &g.p.smooth;
  const int N = g.p.capacity, C = g.p.cams_per_rig, I = p->iterations;
  if (C > c->F) return lag_fail(c, "cams_per_rig exceeds max_cams");
  if (mantis_status e = line_check_frames(c, "lag", p->record, cams, C)) return e;
  const int W = cams[0].width, H = cams[0].height;
  const bool first = g.n == 0;
  if (!first && (W != g.W || H != g.H)) return lag_fail(c, "frame size differs from the first push since the reset");
  if (!first && !motion) return lag_fail(c, "null argument (motion, after the first push)");
  bool has_motion = false;
  if (!first) {
    const double* q = motion->delta_quat_xyzw;
    for (int i = 0; i < 4; i++)
      if (!std::isfinite(q[i])) return lag_fail(c, "motion: delta_quat is not finite");
    for (int i = 0; i < 3; i++)
      if (!std::isfinite(motion->delta_pos[i])) return lag_fail(c, "motion: delta_pos is not finite");
    has_motion = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] >= 0.5;  // as mantis_track
  }
  if (T_start) {
    for (int i = 0; i < 16; i++)
      if (!std::isfinite(T_start[i])) return lag_fail(c, "T_start is not finite");
  } else if (first || !has_motion) {
    return lag_fail(c, "T_start is required on the first push and after an unset motion");
  }

  g.ws.windows = 0;  // no record until this push has finished
  c->sm_rec = &g.ws;
  if (mantis_status e = refine_flags(c, p->landmark_pitch)) return e;
  const int n_cand = c->rf.n_cand;
  if (mantis_status e = lag_alloc(c, W, H)) return e;
  const bool slide = g.n == N;
  const int n = slide ? N : g.n + 1;
  const size_t pass_slots = (size_t)n * C * n_cand;
  {
    const size_t slots = (p->record ? (size_t)I + 1 : 1) * std::max<size_t>((size_t)N * C * n_cand, 1);
    if (slots > g.ws.d_slots.capacity()) HIP_OK(hipStreamSynchronize(c->s));
    if (g.ws.d_slots.grow(c, slots)) return MANTIS_ERR_OOM;
  }
  const LagLayout L = lag_layout(N);
  mk::LagArgs la = lag_args(c);  // on the last push's window, before anything below changes it

  mk::LagIn* in = (mk::LagIn*)g.ws.h_in.get();
  std::memset(in, 0, sizeof(*in));
  if (has_motion) quat_to_mat4(motion->delta_quat_xyzw, motion->delta_pos, in->D);
  in->has_motion = has_motion ? 1 : 0;
  if (T_start) std::memcpy(in->T_start, T_start, sizeof(in->T_start));
  in->has_start = T_start ? 1 : 0;
  in->first = first ? 1 : 0;
  if (first && g.reset_prior) {
    in->load_prior = 1;
    std::memcpy(in->Tp, g.Tp, sizeof(in->Tp));
    std::memcpy(in->Wp, g.Wp, sizeof(in->Wp));
    std::memcpy(in->Cov, g.Cov, sizeof(in->Cov));
  }
  in->slide = slide ? 1 : 0;
  in->why = slide ? lag_why(g) : smo::kLagKept;
  in->n_old = g.n;
  in->n_cand = n_cand;
  // the ring slot the new view takes: the one the oldest view leaves (views enter in ring order)
  const size_t fb = (size_t)W * H * 3, slot = (size_t)(g.pushes % N);
  for (int k = 0; k < C; k++) {
    const mantis_image& im = cams[k];
    mk::FrameDesc& fd = in->fd[k];
    fd.w = W;
    fd.h = H;
    fd.cam = cam_from(im);
    fd.scam = screen_cam_cached(c, fd.cam);
    fd.bgr = g.d_ring + (slot * C + k) * fb;
    rfn::gncam_from(im.T_base_cam, in->gc[k]);
  }

  mark(c, "start");
  for (int k = 0; k < C; k++)
    HIP_OK(hipMemcpy2DAsync(g.d_ring + (slot * C + k) * fb, 3 * (size_t)W, cams[k].bgr, cams[k].step_bytes, 3 * (size_t)W,
                            H, cams[k].mem_kind == 1 ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->s));
  HIP_OK(hipMemcpyAsync(g.ws.d_in, g.ws.h_in, sizeof(mk::LagIn), hipMemcpyHostToDevice, c->s));
  mark(c, "lag_frames");
  mk::k_lag_slide<<<1, 64, 0, c->s>>>(la);
  HIP_OK(hipGetLastError());
  mark(c, "lag_slide/k_lag_slide");

  // from here on the window on the device is the new one, whatever follows: keep the host's account in step
  if (slide) {
    g.has.erase(g.has.begin());
    g.stamps.erase(g.stamps.begin());
  }
  if (!first) g.has[n - 2] = has_motion ? 1 : 0;
  g.has.resize(N, 0);
  g.has[n - 1] = 0;
  g.stamps.push_back(cams[0].stamp_ns);
  const int solve_prior = slide ? (in->why == smo::kLagKept ? 1 : 0) : (first ? in->load_prior : g.has_prior);
  g.n = n;
  g.pushes++;
  g.last_ok = false;
  g.reset_prior = false;

  const SmoothLayout S = smooth_layout(n, 1, (size_t)n * C, (size_t)I + 1);
  mk::RefineArgs a;
  a.gncam = g.d_gncam;
  a.cand = c->rf.d_cand;
  a.st = la.st;
  a.slots = (rfn::Slot*)g.ws.d_slots;
  a.recT = g.ws.d_work + S.w_recT;
  a.recAcc = g.ws.d_work + S.w_recAcc;
  a.pass_slots = p->record ? pass_slots : 0;
  a.C = C;
  a.n_cand = n_cand;
  a.I = I;
  a.n_rigs = n;
  a.min_obs = p->min_obs;
  a.rig_stride = C;
  a.win = rfn::Window{p->half_window, p->white_thresh, p->min_weight, 0};
  a.lambda = p->lambda;
  mk::SmoothArgs s;
  s.win = &la.head->win;
  s.D = g.d_D;
  s.has = g.d_has;
  s.Tp = la.head->Tp;
  s.Wp = la.head->Wp;
  s.Hd = (double*)(g.ws.d_out + L.o_Hd);
  s.Ho = (double*)(g.ws.d_out + L.o_Ho);
  s.g = g.ws.d_work;
  s.Ld = g.ws.d_work + S.w_Ld;
  s.Lo = g.ws.d_work + S.w_Lo;
  s.y = g.ws.d_work + S.w_y;
  s.x = g.ws.d_work + S.w_x;
  s.recE = g.ws.d_work + S.w_recE;
  s.recJ = g.ws.d_work + S.w_recJ;
  s.recPe = g.ws.d_work + S.w_recPe;
  s.recPJ = g.ws.d_work + S.w_recPJ;
  s.recDelta = g.ws.d_work + S.w_recDelta;
  s.N = n;
  s.V = n;
  s.Wn = 1;
  // a marginal the device finds not positive definite leaves a zero whitener (exact zeros in H_00, g_0 and
  // the cost) and has_prior = 0 in the result
  s.has_prior = solve_prior;
  s.w = smo::Weights{p->sigma_row / p->sigma_t, p->sigma_row / p->sigma_rot, p->sigma_row, p->lambda};

  const Landmarks lm = lmk_of(c);
  const dim3 grid((n_cand + mk::kRefineCands - 1) / mk::kRefineCands, C, n);
  for (int pass = 0; pass <= I; pass++) {
    if (n_cand > 0) {
      mk::k_refine_obs<<<grid, 256, 0, c->s>>>(g.d_fd, lm, a, pass);
      HIP_OK(hipGetLastError());
    }
    mark(c, "smooth_obs/k_refine_obs");
    mk::k_smooth_acc<<<n, 256, 0, c->s>>>(a, pass);
    HIP_OK(hipGetLastError());
    mark(c, "smooth_acc/k_smooth_acc");
    mk::k_smooth_solve<<<1, 256, 0, c->s>>>(a, s, pass);
    HIP_OK(hipGetLastError());
    mark(c, "smooth_solve/k_smooth_solve");
  }
  HIP_OK(hipMemcpyAsync(g.ws.h_out, g.ws.d_out, L.o_peek, hipMemcpyDeviceToHost, c->s));
  HIP_OK(wait_stream(c, n * C));
  finish_profile(c);

  mk::LagHead* hd = (mk::LagHead*)g.ws.h_out.get();
  const mk::RefineRig* h_st = (const mk::RefineRig*)(g.ws.h_out + L.o_st);
  g.views.assign(n, mantis_smooth_view{});
  for (int k = 0; k < n; k++) {
    const mantis_refine_result& rr = h_st[k].res;
    g.views[k].n_obs = rr.n_obs[rr.iterations_run];
    g.views[k].rms = rr.rms[rr.iterations_run];
    std::memcpy(g.views[k].T_w_b, rr.T_w_b, sizeof(double) * 16);
  }
  smo::conclude(n, (const double*)(g.ws.h_out + L.o_Hd), (const double*)(g.ws.h_out + L.o_Ho), g.has.data(), p->min_obs,
                p->max_rms, hd->win.res, g.views.data());
  *out = hd->win.res;
  for (int k = 0; k < n; k++) views[k] = g.views[k];
  g.last_ok = hd->win.res.status == smo::kOk;
  g.has_prior = hd->has_prior;
  g.drop_reason = hd->drop_reason;
  std::memcpy(g.Tp, hd->Tp, sizeof(g.Tp));
  std::memcpy(g.Wp, hd->Wp, sizeof(g.Wp));
  std::memcpy(g.Cov, hd->Cov, sizeof(g.Cov));
  if (info) {
    info->pushes = g.pushes;
    info->oldest_stamp_ns = g.stamps.front();
    info->n_views = n;
    info->has_prior = g.has_prior;
    info->drop_reason = g.drop_reason;
    info->slid = slide ? 1 : 0;
  }
  g.ws.runs.assign(1, hd->win.res.iterations_run);
  g.ws.windows = 1;
  g.ws.N = n;
  g.ws.C = C;
  g.ws.P = I + 1;
  g.ws.record = p->record;
  g.ws.cands = n_cand;
  g.ws.lay_F = n * C;
  return MANTIS_OK;
}

}  // namespace

extern "C" {

void mantis_default_lag_params(mantis_lag_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(mantis_lag_params);
  p->capacity = 8;
  p->cams_per_rig = 1;
  mantis_default_smooth_params(&p->smooth);
}

void mantis_lag_sizes(int32_t* params_bytes, int32_t* info_bytes) {
  if (params_bytes) *params_bytes = (int32_t)sizeof(mantis_lag_params);
  if (info_bytes) *info_bytes = (int32_t)sizeof(mantis_lag_info);
}

mantis_status mantis_lag_reset(void* ctx, const mantis_lag_params* lp, const double* prior_T, const double* prior_cov) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  if (!lp) return lag_fail(c, "null argument");
  if (lp->struct_size != (int32_t)sizeof(mantis_lag_params)) return lag_fail(c, "params.struct_size mismatch");
  const mantis_smooth_params* p = &lp->smooth;
  if (p->struct_size != (int32_t)sizeof(mantis_smooth_params)) return lag_fail(c, "params.smooth.struct_size mismatch");
  if (lp->capacity < 2 || lp->capacity > smo::kMaxViews) return lag_fail(c, "capacity outside 2..256");
  if (lp->cams_per_rig < 1 || lp->cams_per_rig > rfn::kMaxCams) return lag_fail(c, "cams_per_rig outside 1..8");
  if (lp->cams_per_rig > c->F) return lag_fail(c, "cams_per_rig exceeds max_cams");
  if (mantis_status e = line_check_fields(c, "lag", p)) return e;
  if (!(p->sigma_row > 0) || !std::isfinite(p->sigma_row)) return lag_fail(c, "sigma_row must be finite and > 0");
  if (!(p->sigma_t > 0) || !std::isfinite(p->sigma_t)) return lag_fail(c, "sigma_t must be finite and > 0");
  if (!(p->sigma_rot > 0) || !std::isfinite(p->sigma_rot)) return lag_fail(c, "sigma_rot must be finite and > 0");
  if (p->record != 0 && p->record != 1) return lag_fail(c, "record must be 0 or 1");
  if (prior_T && !prior_cov) return lag_fail(c, "null argument (prior_cov with prior_T)");
  double Wp[36];
  if (prior_T) {
    for (int q = 0; q < 16; q++)
      if (!std::isfinite(prior_T[q])) return lag_fail(c, "prior_T is not finite");
    if (!smo::prior_whitener(prior_cov, p->sigma_row, Wp))
      return lag_fail(c, "prior_cov must be finite and positive definite");
  }
  Ctx::Lag& g = c->lag;
  if (g.cap && (g.cap != lp->capacity || g.C != lp->cams_per_rig || g.I != p->iterations)) {
    HIP_OK(hipStreamSynchronize(c->s));
    lag_release(g);
  }
  if (c->sm_rec == &g.ws) g.ws.windows = 0;  // the record of the emptied window is gone
  g.p = *lp;
  g.live = true;
  g.n = 0;
  g.pushes = 0;
  g.last_ok = false;
  g.drop_reason = 0;
  g.has.assign(lp->capacity, 0);
  g.stamps.clear();
  g.views.clear();
  g.reset_prior = prior_T != nullptr;
  g.has_prior = prior_T ? 1 : 0;
  if (prior_T) {
    std::memcpy(g.Tp, prior_T, sizeof(g.Tp));
    std::memcpy(g.Wp, Wp, sizeof(g.Wp));
    std::memcpy(g.Cov, prior_cov, sizeof(g.Cov));
  }
  return MANTIS_OK;
}

mantis_status mantis_lag_push(void* ctx, const mantis_image* cams, const mantis_motion* motion, const double* T_start,
                              mantis_smooth_result* out_result, mantis_smooth_view* out_views, mantis_lag_info* out_info) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  return lag_push_impl(c, cams, motion, T_start, out_result, out_views, out_info);
}

mantis_status mantis_lag_get_prior(void* ctx, double* T, double* cov, int32_t* has, int32_t* reason) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  Ctx::Lag& g = c->lag;
  if (!g.live) return lag_fail(c, "get_prior before reset (mantis_lag_reset)");
  int hp = g.has_prior, why = smo::kLagKept;
  const double *pT = g.Tp, *pC = g.Cov;
  if (g.n == g.p.capacity) {  // full: the next push slides first
    why = lag_why(g);
    hp = 0;
    if (why == smo::kLagKept) {
      const LagLayout L = lag_layout(g.cap);
      mk::LagArgs la = lag_args(c);
      la.peek = (mk::LagHead*)(g.ws.d_out + L.o_peek);
      mk::k_lag_slide<<<1, 64, 0, c->s>>>(la);
      HIP_OK(hipGetLastError());
      mk::LagHead* hp_out = (mk::LagHead*)(g.ws.h_out + L.o_peek);
      HIP_OK(hipMemcpyAsync(hp_out, la.peek, sizeof(mk::LagHead), hipMemcpyDeviceToHost, c->s));
      HIP_OK(hipStreamSynchronize(c->s));
      hp = hp_out->has_prior;
      why = hp_out->drop_reason;
      pT = hp_out->Tp;
      pC = hp_out->Cov;
    }
  }
  if (has) *has = hp;
  if (reason) *reason = why;
  if (T) {
    if (hp) std::memcpy(T, pT, sizeof(double) * 16);
    else std::memset(T, 0, sizeof(double) * 16);
  }
  if (cov) {
    if (hp) std::memcpy(cov, pC, sizeof(double) * 36);
    else std::memset(cov, 0, sizeof(double) * 36);
  }
  return MANTIS_OK;
}

mantis_status mantis_lag_get_views(void* ctx, mantis_smooth_view* views, int32_t* n) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  Ctx::Lag& g = c->lag;
  if (!g.live) return lag_fail(c, "get_views before reset (mantis_lag_reset)");
  if (!views || !n) return lag_fail(c, "null argument");
  if (*n < (int32_t)g.views.size()) return lag_fail(c, "get_views: too little room for the views held");
  for (size_t k = 0; k < g.views.size(); k++) views[k] = g.views[k];
  *n = (int32_t)g.views.size();
  return MANTIS_OK;
}

}  // extern "C"
