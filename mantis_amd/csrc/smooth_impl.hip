// Window smoothing: line rows plus odometry factors over N views
// (mantis_smooth_batch, include/mantis.h). Included by api.hip after
// refine_impl.hip (shares its candidates, RefineRig / RefineArgs and
// k_refine_obs). The rules -- log_so3, the between and prior factors, the
// assembly, the block Cholesky's operation order, the window's figures, the
// gate and the marginals -- are in mk_smooth.h (shared with the host build of
// the tests).
//
// Device work of one call of I iterations, all on the context stream:
//   per pass p = 0 .. I:  k_refine_obs    as it is, the views as its rigs
//                         k_smooth_acc    M^T M over each view's slots
//                         k_smooth_solve  per window: the factors, the blocks,
//                                         the figures and gates, the chain,
//                                         T_p+1 (pass I: the lambda = 0 blocks)
// = 3 (I + 1) launches, then one D2H copy (the views' states, the windows'
// results and the final blocks, one buffer). Every hand-off crosses a kernel
// boundary: no last-block counter, no polled flag, no hipGraph. The blocks of
// a window live in a context workspace (162 doubles per view as stored; a
// 256-view window is 332 KB, written and read once per pass by one block, so
// it stays in L2).
#include "mk_smooth.h"

namespace mk {

namespace smo = smooth;

struct SmoothWin {  // one window between the launches, and what comes back
  mantis_smooth_result res;
  int32_t done, pad;
};

struct SmoothArgs {
  SmoothWin* win;      // windows
  const double* D;     // per view slot k of a window: Transform of motion k (k < N - 1)
  const int32_t* has;  // per view slot: motion k is set
  const double *Tp, *Wp;  // per window: the prior's pose, sigma_row L_c^-1
  double *Hd, *Ho;     // per view: H_kk, H_{k+1,k} (come back with the results)
  double *g, *Ld, *Lo, *y, *x;  // per view: the rest of the chain's workspace
  // the pass record, [pass][view] or [pass][window]: e (6), Ja | Jb (72), the prior's e (6) and J (36), x (6)
  double *recE, *recJ, *recPe, *recPJ, *recDelta;
  int32_t N, V, Wn, has_prior;  // views per window, views and windows of the call
  smo::Weights w;
};

// One block per view: k_refine_step's accumulation (refine_trips, the block
// count of code-0 rows, the wave-order sum) without its solve. Thread 0 writes
// acc28, n_obs and rms of the view and the pass record.
__global__ __launch_bounds__(256) void k_smooth_acc(RefineArgs a, int pass) {
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
    S.res.n_obs[pass] = n_obs;
    S.res.rms[pass] = n_obs > 0 ? sqrt(acc28[27] / (double)n_obs) : 0.0;
    S.res.iterations_run = pass;  // the last pass taken: where the view's final figures are
  }
}

// The block-Cholesky chain of one window, run by wave 0: lane e < 36 holds
// element (e / 6, e % 6) of the current 6 x 6 block, lanes 0..5 the current
// 6-vector; operands travel by __shfl and every lane commits only its own
// element, so each dot product runs in smo::chain_step's / back_step's order.
// Every lane of the wave executes every shuffle (the idle lanes mirror element
// 0 and store nothing). Returns false when a diagonal block is not positive
// definite (wave-uniform).
__device__ bool smooth_chain(const SmoothArgs& s, int v0, int N, int lane) {
  const int e = lane < 36 ? lane : 0, i = e / 6, j = e - 6 * i, i6 = lane < 6 ? lane : 0;
  const int32_t* has = s.has + v0;
  double *Ld = s.Ld + 36 * (size_t)v0, *Lo = s.Lo + 36 * (size_t)v0, *yy = s.y + 6 * (size_t)v0;
  double Lp = 0, yp = 0;
  // the next step's blocks are loaded while this one computes (a chain step is a few microseconds
  // of dependent shuffles: a load issued at its top would add its whole latency to every step)
  double nH = s.Hd[36 * (size_t)v0 + e], nO = s.Ho[36 * (size_t)v0 + e], ng = s.g[6 * (size_t)v0 + i6];
  for (int k = 0; k < N; k++) {
    const bool coupled = k > 0 && has[k - 1], next = k < N - 1 && has[k];
    const size_t v = (size_t)(v0 + k);
    double mm = nH;
    const double h = nO, gk = ng;
    if (k + 1 < N) {
      nH = s.Hd[36 * (v + 1) + e];
      nO = s.Ho[36 * (v + 1) + e];
      ng = s.g[6 * (v + 1) + i6];
    }
    if (coupled) {
#pragma unroll
      for (int q = 0; q < 6; q++) mm -= __shfl(Lp, 6 * i + q) * __shfl(Lp, 6 * j + q);
    }
    double L = 0;
#pragma unroll
    for (int c = 0; c < 6; c++) {
      double sa = mm;
#pragma unroll
      for (int q = 0; q < c; q++) sa -= __shfl(L, 6 * i + q) * __shfl(L, 6 * j + q);
      const double sd = __shfl(sa, 7 * c);
      if (!(sd > 0)) return false;
      const double d = sqrt(sd);
      if (j == c && i == c) L = d;
      else if (j == c && i > c) L = sa / d;
    }
    double X = 0;
    if (next) {
#pragma unroll
      for (int c = 0; c < 6; c++) {
        double sa = h;
#pragma unroll
        for (int q = 0; q < c; q++) sa -= __shfl(X, 6 * i + q) * __shfl(L, 6 * j + q);
        const double d = __shfl(L, 7 * c);
        if (j == c) X = sa / d;
      }
    }
    double ta = -gk, yv = 0;
    if (coupled) {
#pragma unroll
      for (int q = 0; q < 6; q++) ta -= __shfl(Lp, 6 * i6 + q) * __shfl(yp, q);
    }
#pragma unroll
    for (int c = 0; c < 6; c++) {
#pragma unroll
      for (int q = 0; q < c; q++) {
        const double pr = __shfl(L, 6 * i6 + q) * __shfl(yv, q);
        if (lane == c) ta -= pr;
      }
      const double d = __shfl(L, 7 * c);
      if (lane == c) yv = ta / d;
    }
    if (lane < 36) {
      Ld[36 * (size_t)k + lane] = L;
      Lo[36 * (size_t)k + lane] = X;
    }
    if (lane < 6) yy[6 * (size_t)k + lane] = yv;
    Lp = X;
    yp = yv;
  }
  double xn = 0;
  // each lane reads back its own elements, one view ahead of the substitution
  double nL = Ld[36 * (size_t)(N - 1) + e], nX = Lo[36 * (size_t)(N - 1) + e], ny = yy[6 * (size_t)(N - 1) + i6];
  for (int k = N - 1; k >= 0; k--) {
    const bool next = k < N - 1 && has[k];
    const size_t v = (size_t)(v0 + k);
    const double L = nL, X = nX;
    double ta = ny, xv = 0;
    if (k > 0) {
      nL = Ld[36 * (size_t)(k - 1) + e];
      nX = Lo[36 * (size_t)(k - 1) + e];
      ny = yy[6 * (size_t)(k - 1) + i6];
    }
    if (next) {
#pragma unroll
      for (int q = 0; q < 6; q++) ta -= __shfl(X, 6 * q + i6) * __shfl(xn, q);
    }
#pragma unroll
    for (int c = 5; c >= 0; c--) {
#pragma unroll
      for (int q = c + 1; q < 6; q++) {
        const double pr = __shfl(L, 6 * q + i6) * __shfl(xv, q);
        if (lane == c) ta -= pr;
      }
      const double d = __shfl(L, 7 * c);
      if (lane == c) xv = ta / d;
    }
    if (lane < 6) s.x[6 * v + lane] = xv;
    xn = xv;
  }
  return true;
}

// One block of 256 threads per window. Thread t < N - 1 forms the factor of
// step t, thread 255 the prior's (N <= 256 leaves it free of a step); thread
// t < N assembles the blocks of view t; thread 0 forms the window's figures
// and applies the gates; wave 0 runs the chain; thread t < N applies the step
// to view t. Pass I stops after the figures: its blocks carry lambda = 0 for
// the host's conclude.
__global__ __launch_bounds__(256) void k_smooth_solve(RefineArgs a, SmoothArgs s, int pass) {
  __shared__ int sh_end, sh_sing;
  const int w = blockIdx.x, t = threadIdx.x, N = s.N, v0 = w * N;
  SmoothWin& Wd = s.win[w];
  if (Wd.done) return;
  const size_t pv = (size_t)pass * s.V + v0, pw = (size_t)pass * s.Wn + w;
  double *fe = s.recE + 6 * pv, *fJ = s.recJ + 72 * pv, *pe = s.recPe + 6 * pw, *pJ = s.recPJ + 36 * pw;
  const int32_t* has = s.has + v0;
  if (t == 0) sh_sing = 0;
  if (t < N - 1) {
    if (has[t]) {
      smo::between(a.st[v0 + t].res.T_w_b, a.st[v0 + t + 1].res.T_w_b, s.D + 16 * (size_t)(v0 + t), s.w.wt, s.w.wr,
                   fe + 6 * t, fJ + 72 * t, fJ + 72 * t + 36);
    } else {
      for (int q = 0; q < 6; q++) fe[6 * t + q] = 0.0;
      for (int q = 0; q < 72; q++) fJ[72 * t + q] = 0.0;
    }
  }
  if (t == 255) {
    if (s.has_prior) {
      smo::prior(a.st[v0].res.T_w_b, s.Tp + 16 * (size_t)w, s.Wp + 36 * (size_t)w, pe, pJ);
    } else {
      for (int q = 0; q < 6; q++) pe[q] = 0.0;
      for (int q = 0; q < 36; q++) pJ[q] = 0.0;
    }
  }
  __syncthreads();
  const double lam = pass < a.I ? s.w.lambda : 0.0;
  if (t < N)
    smo::assemble(t, N, a.st[v0 + t].acc28, has, fe, fJ, s.has_prior, pe, pJ, lam, s.Hd + 36 * (size_t)(v0 + t),
                  s.Ho + 36 * (size_t)(v0 + t), s.g + 6 * (size_t)(v0 + t));
  if (t == 0) {
    int32_t n_sum = 0;
    double rtr = 0;
    for (int k = 0; k < N; k++) {
      n_sum += a.st[v0 + k].res.n_obs[pass];
      rtr += a.st[v0 + k].acc28[27];
    }
    smo::Sums S;
    smo::window_sums(N, n_sum, rtr, has, fe, s.has_prior, pe, s.w.sigma_row, S);
    sh_end = smo::end_sums(S, pass, a.I, a.min_obs, Wd.res) ? 1 : 0;
  }
  __syncthreads();
  if (!sh_end && t < 64) {
    const bool ok = smooth_chain(s, v0, N, t);
    if (t == 0 && !ok) sh_sing = 1;
  }
  __syncthreads();
  if (sh_end || sh_sing) {  // the window stops here: its views observe nothing more
    if (t < N) {
      a.st[v0 + t].done = 1;
      for (int q = 0; q < 6; q++) s.recDelta[6 * (pv + t) + q] = 0.0;
    }
    if (t == 0) {
      if (sh_sing) Wd.res.status = smo::kSingular;
      Wd.done = 1;
    }
    return;
  }
  if (t < N) {
    double x[6], T[16];
    for (int q = 0; q < 6; q++) x[q] = s.recDelta[6 * (pv + t) + q] = s.x[6 * (size_t)(v0 + t) + q];
    for (int q = 0; q < 16; q++) T[q] = a.st[v0 + t].res.T_w_b[q];
    calib::right_update(T, x);
    for (int q = 0; q < 16; q++) a.st[v0 + t].res.T_w_b[q] = T[q];
  }
  if (t == 0) Wd.res.iterations_run = pass + 1;
}

}  // namespace mk

namespace {

namespace smo = mk::smooth;

mantis_status smooth_fail(Ctx* c, const char* what) { return line_fail(c, "smooth", what); }

// the device buffers of a call of Wn windows x N views, F frames, P = I + 1 passes
struct SmoothLayout {
  size_t out_bytes, in_bytes, work_doubles;
  size_t o_win, o_Hd, o_Ho;                                   // bytes into the out buffer (the views' RefineRig first)
  size_t i_Tp, i_Wp, i_has, i_gncam;                          // bytes into the in buffer (D first)
  size_t w_Ld, w_Lo, w_y, w_x, w_recT, w_recAcc, w_recE, w_recJ, w_recPe, w_recPJ, w_recDelta;  // doubles (g first)
};
SmoothLayout smooth_layout(size_t V, size_t Wn, size_t F, size_t P) {
  SmoothLayout L;
  L.o_win = sizeof(mk::RefineRig) * V;
  L.o_Hd = L.o_win + sizeof(mk::SmoothWin) * Wn;
  L.o_Ho = L.o_Hd + sizeof(double) * 36 * V;
  L.out_bytes = L.o_Ho + sizeof(double) * 36 * V;
  L.i_Tp = sizeof(double) * 16 * V;
  L.i_Wp = L.i_Tp + sizeof(double) * 16 * Wn;
  L.i_gncam = L.i_Wp + sizeof(double) * 36 * Wn;
  L.i_has = L.i_gncam + sizeof(mk::GnCam) * F;
  L.in_bytes = L.i_has + sizeof(int32_t) * V;
  size_t o = 6 * V;
  L.w_Ld = o; o += 36 * V;
  L.w_Lo = o; o += 36 * V;
  L.w_y = o; o += 6 * V;
  L.w_x = o; o += 6 * V;
  L.w_recT = o; o += P * 16 * V;
  L.w_recAcc = o; o += P * 28 * V;
  L.w_recE = o; o += P * 6 * V;
  L.w_recJ = o; o += P * 72 * V;
  L.w_recPe = o; o += P * 6 * Wn;
  L.w_recPJ = o; o += P * 36 * Wn;
  L.w_recDelta = o; o += P * 6 * V;
  L.work_doubles = o;
  return L;
}

mantis_status smooth_workspace(Ctx* c, const SmoothLayout& L, size_t slots) {
  Ctx::Smooth& r = c->sm;
  if (L.out_bytes > r.d_out.capacity() || L.in_bytes > r.d_in.capacity() || L.work_doubles > r.d_work.capacity() ||
      slots > r.d_slots.capacity())
    HIP_OK(hipStreamSynchronize(c->s));
  if (r.d_out.grow(c, L.out_bytes) || r.h_out.grow(c, L.out_bytes) || r.d_in.grow(c, L.in_bytes) ||
      r.h_in.grow(c, L.in_bytes) || r.d_work.grow(c, L.work_doubles) || r.d_slots.grow(c, slots))
    return MANTIS_ERR_OOM;
  return MANTIS_OK;
}

mantis_status smooth_check(Ctx* c, const mantis_image* cams, int32_t Wn, int32_t N, int32_t C,
                           const mantis_smooth_params* p) {
  if (p->struct_size != (int32_t)sizeof(mantis_smooth_params)) return smooth_fail(c, "params.struct_size mismatch");
  if (!c->d_lm || c->nw + c->nr + c->ng <= 0) return smooth_fail(c, "map not set (mantis_set_map)");
  if (Wn <= 0 || N <= 0 || C <= 0) return smooth_fail(c, "n_windows, n_views and cams_per_rig must be positive");
  if (N > smo::kMaxViews) return smooth_fail(c, "n_views exceeds 256");
  if (C > rfn::kMaxCams) return smooth_fail(c, "cams_per_rig exceeds 8");
  if ((int64_t)Wn * N * C > c->F) return smooth_fail(c, "n_windows x n_views x cams_per_rig exceeds max_cams");
  if (mantis_status e = line_check_fields(c, "smooth", p)) return e;
  if (!(p->sigma_row > 0) || !std::isfinite(p->sigma_row)) return smooth_fail(c, "sigma_row must be finite and > 0");
  if (!(p->sigma_t > 0) || !std::isfinite(p->sigma_t)) return smooth_fail(c, "sigma_t must be finite and > 0");
  if (!(p->sigma_rot > 0) || !std::isfinite(p->sigma_rot)) return smooth_fail(c, "sigma_rot must be finite and > 0");
  return line_check_frames(c, "smooth", p->record, cams, Wn * N * C);
}

mantis_status smooth_impl(Ctx* c, const mantis_image* cams, int32_t Wn, int32_t N, int32_t C, const double* T_in,
                          const mantis_motion* motions, const double* prior_T, const double* prior_cov,
                          const mantis_smooth_params* p, mantis_smooth_result* out, mantis_smooth_view* views) {
  if (!cams || !T_in || !p || !out || !views) return smooth_fail(c, "null argument");
  if (mantis_status e = smooth_check(c, cams, Wn, N, C, p)) return e;
  if (N > 1 && !motions) return smooth_fail(c, "null argument (motions, n_views > 1)");
  if (prior_T && !prior_cov) return smooth_fail(c, "null argument (prior_cov with prior_T)");
  const int V = Wn * N, F = V * C, I = p->iterations;
  for (size_t i = 0; i < 16 * (size_t)V; i++)
    if (!std::isfinite(T_in[i])) return smooth_fail(c, "T_w_b_in is not finite");
  for (int i = 0; i < Wn * (N - 1); i++) {
    for (int q = 0; q < 4; q++)
      if (!std::isfinite(motions[i].delta_quat_xyzw[q])) return smooth_fail(c, "motions: delta_quat is not finite");
    for (int q = 0; q < 3; q++)
      if (!std::isfinite(motions[i].delta_pos[q])) return smooth_fail(c, "motions: delta_pos is not finite");
  }
  std::vector<double> Wp(prior_T ? 36 * (size_t)Wn : 0);
  for (int w = 0; prior_T && w < Wn; w++) {
    for (int q = 0; q < 16; q++)
      if (!std::isfinite(prior_T[16 * (size_t)w + q])) return smooth_fail(c, "prior_T is not finite");
    if (!smo::prior_whitener(prior_cov + 36 * (size_t)w, p->sigma_row, &Wp[36 * (size_t)w]))
      return smooth_fail(c, "prior_cov must be finite and positive definite");
  }

  Ctx::Smooth& r = c->sm;
  Ctx::Refine& rf = c->rf;
  r.windows = 0;  // no record until this call has finished
  c->sm_rec = &r;
  if (mantis_status e = refine_flags(c, p->landmark_pitch)) return e;
  const int n_cand = rf.n_cand;
  const SmoothLayout L = smooth_layout(V, Wn, F, (size_t)I + 1);
  const size_t pass_slots = (size_t)V * C * n_cand;
  if (mantis_status e = smooth_workspace(c, L, (p->record ? (size_t)I + 1 : 1) * std::max<size_t>(pass_slots, 1)))
    return e;

  std::memset(r.h_out, 0, L.o_Hd);
  mk::RefineRig* h_st = (mk::RefineRig*)r.h_out.get();
  mk::SmoothWin* h_win = (mk::SmoothWin*)(r.h_out + L.o_win);
  for (int k = 0; k < V; k++) {
    std::memcpy(h_st[k].res.T_w_b, T_in + 16 * (size_t)k, sizeof(double) * 16);
    h_st[k].res.n_cand = n_cand;
  }
  for (int w = 0; w < Wn; w++) {
    h_win[w].res.n_cand = n_cand;
    h_win[w].res.n_views = N;
    h_win[w].res.has_prior = prior_T ? 1 : 0;
  }
  std::memset(r.h_in, 0, L.in_bytes);
  double* h_D = (double*)r.h_in.get();
  int32_t* h_has = (int32_t*)(r.h_in + L.i_has);
  for (int w = 0; w < Wn; w++)
    for (int k = 0; k < N - 1; k++) {
      const mantis_motion& mo = motions[(size_t)w * (N - 1) + k];
      const double* q = mo.delta_quat_xyzw;
      if (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] >= 0.5) {  // as mantis_track
        quat_to_mat4(mo.delta_quat_xyzw, mo.delta_pos, h_D + 16 * ((size_t)w * N + k));
        h_has[(size_t)w * N + k] = 1;
      }
    }
  if (prior_T) {
    std::memcpy(r.h_in + L.i_Tp, prior_T, sizeof(double) * 16 * Wn);
    std::memcpy(r.h_in + L.i_Wp, Wp.data(), sizeof(double) * 36 * Wn);
  }
  mk::GnCam* h_gc = (mk::GnCam*)(r.h_in + L.i_gncam);
  for (int i = 0; i < F; i++) rfn::gncam_from(cams[i].T_base_cam, h_gc[i]);

  int W, H;
  mantis_status st = stage_frames(c, cams, F, W, H);
  if (st != MANTIS_OK) return st;
  HIP_OK(hipMemcpyAsync(r.d_out, r.h_out, L.o_Hd, hipMemcpyHostToDevice, c->s));
  HIP_OK(hipMemcpyAsync(r.d_in, r.h_in, L.in_bytes, hipMemcpyHostToDevice, c->s));

  mk::RefineArgs a;
  a.gncam = (const mk::GnCam*)(r.d_in + L.i_gncam);
  a.cand = rf.d_cand;
  a.st = (mk::RefineRig*)r.d_out.get();
  a.slots = (rfn::Slot*)r.d_slots;
  a.recT = r.d_work + L.w_recT;
  a.recAcc = r.d_work + L.w_recAcc;
  a.pass_slots = p->record ? pass_slots : 0;
  a.C = C;
  a.n_cand = n_cand;
  a.I = I;
  a.n_rigs = V;
  a.min_obs = p->min_obs;
  a.rig_stride = C;
  a.win = rfn::Window{p->half_window, p->white_thresh, p->min_weight, 0};
  a.lambda = p->lambda;
  mk::SmoothArgs s;
  s.win = (mk::SmoothWin*)(r.d_out + L.o_win);
  s.D = (const double*)r.d_in.get();
  s.has = (const int32_t*)(r.d_in + L.i_has);
  s.Tp = (const double*)(r.d_in + L.i_Tp);
  s.Wp = (const double*)(r.d_in + L.i_Wp);
  s.Hd = (double*)(r.d_out + L.o_Hd);
  s.Ho = (double*)(r.d_out + L.o_Ho);
  s.g = r.d_work;
  s.Ld = r.d_work + L.w_Ld;
  s.Lo = r.d_work + L.w_Lo;
  s.y = r.d_work + L.w_y;
  s.x = r.d_work + L.w_x;
  s.recE = r.d_work + L.w_recE;
  s.recJ = r.d_work + L.w_recJ;
  s.recPe = r.d_work + L.w_recPe;
  s.recPJ = r.d_work + L.w_recPJ;
  s.recDelta = r.d_work + L.w_recDelta;
  s.N = N;
  s.V = V;
  s.Wn = Wn;
  s.has_prior = prior_T ? 1 : 0;
  s.w = smo::Weights{p->sigma_row / p->sigma_t, p->sigma_row / p->sigma_rot, p->sigma_row, p->lambda};

  const Landmarks lm = lmk_of(c);
  mark(c, "start");
  const dim3 grid((n_cand + mk::kRefineCands - 1) / mk::kRefineCands, C, V);
  for (int pass = 0; pass <= I; pass++) {
    if (n_cand > 0) {
      mk::k_refine_obs<<<grid, 256, 0, c->s>>>(c->d_frames, lm, a, pass);
      HIP_OK(hipGetLastError());
    }
    mark(c, "smooth_obs/k_refine_obs");
    mk::k_smooth_acc<<<V, 256, 0, c->s>>>(a, pass);
    HIP_OK(hipGetLastError());
    mark(c, "smooth_acc/k_smooth_acc");
    mk::k_smooth_solve<<<Wn, 256, 0, c->s>>>(a, s, pass);
    HIP_OK(hipGetLastError());
    mark(c, "smooth_solve/k_smooth_solve");
  }
  HIP_OK(hipMemcpyAsync(r.h_out, r.d_out, L.out_bytes, hipMemcpyDeviceToHost, c->s));
  HIP_OK(wait_stream(c, F));
  finish_profile(c);

  const double* h_Hd = (const double*)(r.h_out + L.o_Hd);
  const double* h_Ho = (const double*)(r.h_out + L.o_Ho);
  r.runs.assign(Wn, 0);
  for (int w = 0; w < Wn; w++) {
    mantis_smooth_view* vw = views + (size_t)w * N;
    for (int k = 0; k < N; k++) {
      const mantis_refine_result& rr = h_st[(size_t)w * N + k].res;
      vw[k] = mantis_smooth_view{};
      vw[k].n_obs = rr.n_obs[rr.iterations_run];
      vw[k].rms = rr.rms[rr.iterations_run];
      std::memcpy(vw[k].T_w_b, rr.T_w_b, sizeof(double) * 16);
    }
    smo::conclude(N, h_Hd + 36 * (size_t)w * N, h_Ho + 36 * (size_t)w * N, h_has + (size_t)w * N, p->min_obs, p->max_rms,
                  h_win[w].res, vw);
    out[w] = h_win[w].res;
    r.runs[w] = h_win[w].res.iterations_run;
  }
  r.windows = Wn;
  r.N = N;
  r.C = C;
  r.P = I + 1;
  r.record = p->record;
  r.cands = n_cand;
  r.lay_F = F;
  return MANTIS_OK;
}

}  // namespace

extern "C" {

void mantis_default_smooth_params(mantis_smooth_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(mantis_smooth_params);
  p->iterations = 4;
  p->half_window = 12;
  p->white_thresh = 3 * 64 * 64;
  p->min_weight = 24576;
  p->min_obs = 12;
  p->lambda = 0;
  p->landmark_pitch = 0.08;
  p->max_rms = 0;
  p->sigma_row = 0.00127;
  p->sigma_t = 0.01;
  p->sigma_rot = 0.03;
  p->record = 0;
}

void mantis_smooth_sizes(int32_t* params_bytes, int32_t* result_bytes, int32_t* view_bytes) {
  if (params_bytes) *params_bytes = (int32_t)sizeof(mantis_smooth_params);
  if (result_bytes) *result_bytes = (int32_t)sizeof(mantis_smooth_result);
  if (view_bytes) *view_bytes = (int32_t)sizeof(mantis_smooth_view);
}

mantis_status mantis_smooth_batch(void* ctx, const mantis_image* cams, int32_t n_windows, int32_t n_views,
                                  int32_t cams_per_rig, const double* T_w_b_in, const mantis_motion* motions,
                                  const double* prior_T, const double* prior_cov, const mantis_smooth_params* p,
                                  mantis_smooth_result* out, mantis_smooth_view* views) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  return smooth_impl(c, cams, n_windows, n_views, cams_per_rig, T_w_b_in, motions, prior_T, prior_cov, p, out, views);
}

mantis_status mantis_get_smooth_record(void* ctx, int32_t window, int32_t view, int32_t pass, double* T_w_b,
                                       int32_t* codes, int32_t* Sw, int32_t* Skw, double* rows, double* acc28) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  const Ctx::Smooth& r = c->sm_rec ? *c->sm_rec : c->sm;  // the last smooth call: a batch call, or a push (lag_impl.hip)
  if (!r.windows || !r.record) {
    c->err = "smooth record: the last smooth call kept none (params.record = 1)";
    return MANTIS_ERR_STATE;
  }
  if (window < 0 || window >= r.windows || view < 0 || view >= r.N || pass < 0 || pass > r.runs[window])
    return smooth_fail(c, "record: window, view or pass out of range (0 .. the window's iterations_run)");
  const size_t V = (size_t)r.windows * r.N, v = (size_t)window * r.N + view, ns = (size_t)r.C * r.cands;
  const SmoothLayout L = smooth_layout(V, r.windows, r.lay_F, r.P);
  if (T_w_b)
    HIP_OK(hipMemcpy(T_w_b, r.d_work + L.w_recT + ((size_t)pass * V + v) * 16, sizeof(double) * 16, hipMemcpyDeviceToHost));
  if (acc28)
    HIP_OK(hipMemcpy(acc28, r.d_work + L.w_recAcc + ((size_t)pass * V + v) * 28, sizeof(double) * 28,
                     hipMemcpyDeviceToHost));
  return slots_scatter<rfn::Slot, 7>(c, (const rfn::Slot*)r.d_slots + ((size_t)pass * V + v) * ns, ns, codes, Sw, Skw,
                                     rows);
}

mantis_status mantis_get_smooth_pass(void* ctx, int32_t window, int32_t pass, double* e, double* J, double* prior_e,
                                     double* prior_J, double* delta) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  const Ctx::Smooth& r = c->sm_rec ? *c->sm_rec : c->sm;  // the last smooth call: a batch call, or a push (lag_impl.hip)
  if (!r.windows || !r.record) {
    c->err = "smooth pass: the last smooth call kept none (params.record = 1)";
    return MANTIS_ERR_STATE;
  }
  if (window < 0 || window >= r.windows || pass < 0 || pass > r.runs[window])
    return smooth_fail(c, "pass record: window or pass out of range (0 .. the window's iterations_run)");
  const size_t V = (size_t)r.windows * r.N, Wn = r.windows, v0 = (size_t)window * r.N, nf = (size_t)r.N - 1;
  const SmoothLayout L = smooth_layout(V, Wn, r.lay_F, r.P);
  const size_t pv = (size_t)pass * V + v0, pw = (size_t)pass * Wn + window;
  if (e && nf) HIP_OK(hipMemcpy(e, r.d_work + L.w_recE + 6 * pv, sizeof(double) * 6 * nf, hipMemcpyDeviceToHost));
  if (J && nf) HIP_OK(hipMemcpy(J, r.d_work + L.w_recJ + 72 * pv, sizeof(double) * 72 * nf, hipMemcpyDeviceToHost));
  if (prior_e) HIP_OK(hipMemcpy(prior_e, r.d_work + L.w_recPe + 6 * pw, sizeof(double) * 6, hipMemcpyDeviceToHost));
  if (prior_J) HIP_OK(hipMemcpy(prior_J, r.d_work + L.w_recPJ + 36 * pw, sizeof(double) * 36, hipMemcpyDeviceToHost));
  if (delta)
    HIP_OK(hipMemcpy(delta, r.d_work + L.w_recDelta + 6 * pv, sizeof(double) * 6 * r.N, hipMemcpyDeviceToHost));
  return MANTIS_OK;
}

}  // extern "C"
