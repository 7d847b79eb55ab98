// Monte Carlo localization: the persistent rig particle filter
// (mantis_mcl_*, include/mantis.h). Included by api.hip (shares its Ctx, frame
// staging and image stages). The weight / scan / ancestor / estimate rules are in mk_mcl.h
// (shared with the host build of the tests).
//
// Device work of one step, all on the context stream: the image stages up to
// the cleanImageByEdge bit plane (run_image_stages), then 4 launches (5 with
// the colour evidence on: k_mcl_color, mcl_color_impl.hip, after k_mcl_score):
//   k_mcl_predict    one lane per particle: T_j <- T_j * Delta * rand_j, and per
//                    camera the FP64 c2w and its FP32 screen pose
//   k_mcl_score      grid (particle chunk, camera): pose_score_block (kernels.hip),
//                    the body of k_track_score too; each (particle,
//                    camera) owned by one block, (sum, n) written with one store
//   k_mcl_weight     one block of 1024: pool, validity, L (less the colour charge
//                    in the instantiation that folds it), Lmax, q, the integer
//                    scan (c_j, S), best, ess, the estimate, the covariance,
//                    the ancestors when resampling, the result record
//   k_mcl_resample   gathers the poses by ancestor into the other buffer of the
//                    ping-pong pair and zeroes L (returns at once when the
//                    step did not resample)
// Every hand-off between blocks is a kernel boundary: no last-block counter,
// no polled flag, no hipGraph capture.
#include "mk_mcl.h"
#include "mk_mcl_color.h"

namespace mk {

struct MclArgs {
  Xf* T;               // the set: predicted in place
  Xf* Tdst;            // resampling target (the other buffer)
  const Xf* ext;       // C: T_base_cam
  const Xf* delta;     // the motion (read when has_motion)
  const float* gauss;  // N x 6
  double* L;
  double* Lprev;       // L as the step found it (record)
  unsigned long long* q;
  unsigned long long* cum;
  int32_t* anc;
  Xf* c2w;             // N x C
  PoseF* pf;
  long long* sums;     // N x C
  int32_t* cnt;
  mantis_mcl_result* res;
  const double* charge;  // N: the colour charge k_mcl_weight<true> folds into L (null otherwise)
  int32_t N, C, min_projections, has_motion;
  uint32_t U;
  double sigma_rot, sigma_t, tau, resample_frac;
};

__global__ __launch_bounds__(256) void k_mcl_predict(MclArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.N) return;
  Xf T = a.T[j];
  if (a.has_motion) T = xf_mul(T, *a.delta);
  T = track::particle(T, a.gauss + (size_t)j * 6, a.sigma_rot, a.sigma_t);
  a.T[j] = T;
  for (int c = 0; c < a.C; c++) {
    const Xf v = track::cam_c2w(T, a.ext[c]);
    a.c2w[(size_t)j * a.C + c] = v;
    a.pf[(size_t)j * a.C + c] = posef_from(v);
  }
}

template <int NT, int SPLIT>
__global__ __launch_bounds__(NT) void k_mcl_score(const FrameDesc* __restrict__ frames,
                                                  const uint32_t* __restrict__ mbits, size_t bstride, Landmarks lmk,
                                                  MclArgs a) {
  pose_score_block<NT, SPLIT>(frames, mbits, bstride, lmk, a.c2w, a.pf, a.sums, a.cnt, 0, a.C, blockIdx.y, blockIdx.y,
                               blockIdx.x, a.N);
}

constexpr int kMclWT = 1024;  // k_mcl_weight's block
constexpr int kMclRounds = mcl::kMaxParticles / kMclWT;

// K sums over the block, every thread gets them (wave shuffles, then the 16
// wave totals added in wave order by every thread)
template <int K>
__device__ inline void mcl_block_sum(double* v, double (*sh)[kMclWT / 64]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; k++)
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
  __syncthreads();
  if (lane == 0)
    for (int k = 0; k < K; k++) sh[k][wave] = v[k];
  __syncthreads();
  for (int k = 0; k < K; k++) {
    double t = 0;
    for (int w = 0; w < kMclWT / 64; w++) t += sh[k][w];
    v[k] = t;
  }
}
__device__ inline double mcl_block_max(double v, double (*sh)[kMclWT / 64]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  __syncthreads();
  if (lane == 0) sh[0][wave] = v;
  __syncthreads();
  double t = sh[0][0];
  for (int w = 1; w < kMclWT / 64; w++) t = fmax(t, sh[0][w]);
  return t;
}

// One block. Particle j = round * 1024 + tid, at most 4 rounds. COLOR: L also
// pays a.charge (mk_mcl_color.h); the step without colour runs the other
// instantiation, whose arithmetic and registers are those it always had.
template <bool COLOR>
__global__ __launch_bounds__(kMclWT) void k_mcl_weight(MclArgs a) {
  constexpr int NT = kMclWT, kW = NT / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, C = a.C;
  const int rounds = (N + NT - 1) / NT;  // <= kMclRounds (N <= 4096, checked by the host)
  __shared__ uint64_t s_cum[mcl::kMaxParticles];
  __shared__ double s_red[21][kW];
  __shared__ unsigned long long s_wt[kW], s_bq[kW];
  __shared__ int s_bj[kW];
  mantis_mcl_result& R = *a.res;

  double Ln[kMclRounds], E[kMclRounds];
  double lmax = -INFINITY;
#pragma unroll
  for (int r = 0; r < kMclRounds; r++) {
    const int j = r * NT + tid;
    Ln[r] = -INFINITY;
    E[r] = DBL_MAX;
    if (r < rounds && j < N) {
      int32_t n;
      E[r] = track::pool(a.sums + (size_t)j * C, a.cnt + (size_t)j * C, C, &n);
      const double Lp = a.L[j];
      a.Lprev[j] = Lp;
      if (COLOR && a.charge) Ln[r] = mcl::log_weight_color(Lp, E[r], n, a.min_projections, a.tau, a.charge[j]);
      else Ln[r] = mcl::log_weight(Lp, E[r], n, a.min_projections, a.tau);
      lmax = fmax(lmax, Ln[r]);
      a.anc[j] = -1;
    }
  }
  const double Lmax = mcl_block_max(lmax, s_red);
  if (!(Lmax > -INFINITY)) {  // lost (block-uniform): poses and L stay
#pragma unroll
    for (int r = 0; r < kMclRounds; r++) {
      const int j = r * NT + tid;
      if (r < rounds && j < N) a.q[j] = a.cum[j] = 0;
    }
    if (tid == 0) {
      R.lost = 1;
      R.resampled = 0;
      R.n_particles = N;
      R.n_valid = 0;
      R.best = -1;
      R.ess = 0;
      R.best_error = DBL_MAX;
      R.weight_sum = 0;
      for (int k = 0; k < 16; k++) R.T_w_b[k] = 0;
      for (int k = 0; k < 36; k++) R.covariance[k] = 0;
    }
    return;
  }

  // q, the inclusive integer scan, and the per-thread parts of sum q^2, n_valid, last, best
  unsigned long long q[kMclRounds], carry = 0, bq = 0;
  int bj = 0x7fffffff;
  double acc[3] = {0, 0, 0};  // sum q^2, n_valid
  double lastd = -1;
#pragma unroll
  for (int r = 0; r < kMclRounds; r++) {
    q[r] = 0;
    if (r >= rounds) continue;  // block-uniform
    const int j = r * NT + tid;
    if (j < N) q[r] = mcl::weight_q(Ln[r], Lmax);
    unsigned long long incl = q[r];
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    if (lane == 63) s_wt[wave] = incl;
    __syncthreads();
    unsigned long long pre = carry, tot = carry;
    for (int w = 0; w < kW; w++) {
      const unsigned long long t = s_wt[w];
      if (w < wave) pre += t;
      tot += t;
    }
    carry = tot;
    if (j < N) {
      const unsigned long long c = pre + incl;
      s_cum[j] = c;
      a.cum[j] = c;
      a.q[j] = q[r];
      acc[0] += (double)q[r] * (double)q[r];
      if (q[r] > 0) {
        acc[1] += 1.0;
        lastd = (double)j;
      }
      if (mcl::heavier(q[r], j, bq, bj)) { bq = q[r]; bj = j; }
    }
    __syncthreads();  // s_wt is rewritten by the next round
  }
  const unsigned long long S = carry;
  mcl_block_sum<2>(acc, s_red);
  const int last = (int)mcl_block_max(lastd, s_red);
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long oq = __shfl_xor(bq, o);
    const int oj = __shfl_xor(bj, o);
    if (mcl::heavier(oq, oj, bq, bj)) { bq = oq; bj = oj; }
  }
  __syncthreads();
  if (lane == 0) { s_bq[wave] = bq; s_bj[wave] = bj; }
  __syncthreads();
  bq = s_bq[0];
  bj = s_bj[0];
  for (int w = 1; w < kW; w++)
    if (mcl::heavier(s_bq[w], s_bj[w], bq, bj)) { bq = s_bq[w]; bj = s_bj[w]; }
  const int best = bj, n_valid = (int)acc[1];
  const double ess = (double)S * (double)S / acc[0];
  // resampling depends on the weights alone: decide it now, write the
  // ancestors or the carried log-weights, and let L and E go before the
  // estimate's passes need the registers
  const bool resample = ess < a.resample_frac * (double)N;
#pragma unroll
  for (int r = 0; r < kMclRounds; r++) {
    const int j = r * NT + tid;
    if (r >= rounds || j >= N) continue;
    if (resample) a.anc[j] = mcl::ancestor(s_cum, N, a.U, j, last);  // s_cum: complete since the scan's last barrier
    else a.L[j] = Ln[r];
    if (j == best) R.best_error = E[r];  // the thread that pooled particle best
  }

  // the estimate: first moments about particle best, then the covariance about the mean
  const Xf Tb = a.T[best];
  const Quat qb = basis_to_quat(Tb.R);
  double m7[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < kMclRounds; r++) {
    const int j = r * NT + tid;
    if (!q[r]) continue;
    double t7[7];
    mcl::mean_terms(a.T[j], Tb, qb, (double)q[r] / (double)S, t7);
    for (int k = 0; k < 7; k++) m7[k] += t7[k];
  }
  mcl_block_sum<7>(m7, s_red);
  Quat qs;
  const Xf Tm = mcl::mean_pose(Tb, qb, m7, n_valid == 1, &qs);
  double c21[21];
  for (int k = 0; k < 21; k++) c21[k] = 0;
#pragma unroll
  for (int r = 0; r < kMclRounds; r++) {
    const int j = r * NT + tid;
    if (!q[r]) continue;
    double xi[6], t21[21];
    mcl::xi_of(a.T[j], Tm, qs, xi);
    mcl::cov_terms(xi, (double)q[r] / (double)S, t21);
    for (int k = 0; k < 21; k++) c21[k] += t21[k];
  }
  mcl_block_sum<21>(c21, s_red);

  if (tid == 0) {
    R.lost = 0;
    R.resampled = resample ? 1 : 0;
    R.n_particles = N;
    R.n_valid = n_valid;
    R.best = best;
    R.ess = ess;
    R.weight_sum = S;
    track::xf_to_mat4(Tm, R.T_w_b);
    mcl::cov_expand(c21, R.covariance);
  }
}

__global__ __launch_bounds__(256) void k_mcl_resample(MclArgs a) {
  if (!a.res->resampled) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  const int s = a.anc[i];
  a.Tdst[i] = a.T[s >= 0 && s < a.N ? s : i];
  a.L[i] = 0.0;
}

}  // namespace mk

namespace {

namespace mc = mk::mcl;

mantis_status mcl_fail(Ctx* c, const char* what) {
  c->err = std::string("mcl: ") + what;
  return MANTIS_ERR_ARG;
}

mantis_status mcl_check_params(Ctx* c, const mantis_mcl_params* p) {
  if (!p) return mcl_fail(c, "null argument");
  if (p->struct_size != (int32_t)sizeof(mantis_mcl_params)) return mcl_fail(c, "params.struct_size mismatch");
  if (p->n_particles < 1 || p->n_particles > mc::kMaxParticles) return mcl_fail(c, "n_particles outside 1..4096");
  if (!(p->sigma_rot >= 0 && p->sigma_rot <= 1e6) || !(p->sigma_t >= 0) || !std::isfinite(p->sigma_t))
    return mcl_fail(c, "sigma_rot / sigma_t must be finite and >= 0 (sigma_rot <= 1e6)");
  if (!(p->tau > 0) || !std::isfinite(p->tau)) return mcl_fail(c, "tau must be finite and > 0");
  if (!(p->resample_frac >= 0 && p->resample_frac <= 2)) return mcl_fail(c, "resample_frac outside 0..2");
  if (p->record != 0 && p->record != 1) return mcl_fail(c, "record must be 0 or 1");
  return MANTIS_OK;
}

// buffers for N particles (x 8 cameras); an init with more particles than any before reallocates
mantis_status mcl_workspace(Ctx* c, int N) {
  Ctx::Mcl& m = c->mcl;
  if (N <= m.cap) return MANTIS_OK;
  HIP_OK(hipStreamSynchronize(c->s));  // nothing of an earlier step still reads what is freed
  m.cap = 0;
  m.live = false;
  m.has_record = m.has_modes = false;
  const size_t n = (size_t)N, tasks = n * mk::track::kMaxCams;
  const size_t in_bytes = sizeof(Xf) * (mk::track::kMaxCams + 1) + sizeof(float) * n * 6;
  if (m.d_T[0].alloc(c, n) || m.d_T[1].alloc(c, n) || m.d_L.alloc(c, n) || m.d_Lprev.alloc(c, n) ||
      m.d_q.alloc(c, n) || m.d_cum.alloc(c, n) || m.d_anc.alloc(c, n) || m.d_in.alloc(c, in_bytes) ||
      m.h_in.alloc(c, in_bytes) || m.d_c2w.alloc(c, tasks) || m.d_pf.alloc(c, tasks) || m.d_sums.alloc(c, tasks) ||
      m.d_cnt.alloc(c, tasks) || m.d_res.alloc(c, 1) || m.h_res.alloc(c, 1))
    return MANTIS_ERR_OOM;
  m.cap = N;
  return MANTIS_OK;
}

// the set from host poses, every L = 0
mantis_status mcl_upload(Ctx* c, const std::vector<Xf>& T, const mantis_mcl_params* p) {
  Ctx::Mcl& m = c->mcl;
  const int N = (int)T.size();
  if (mantis_status e = mcl_workspace(c, N)) return e;
  HIP_OK(hipStreamSynchronize(c->s));
  m.live = false;
  HIP_OK(hipMemcpy(m.d_T[0], T.data(), sizeof(Xf) * N, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(m.d_L, 0, sizeof(double) * N));
  m.p = *p;
  m.N = N;
  m.cur = 0;
  m.has_record = false;
  m.has_modes = false;
  m.recentred = false;
  m.live = true;
  return MANTIS_OK;
}

// the colour evidence of a step (mcl_color_impl.hip)
mantis_status mcl_color_workspace(Ctx* c);
mantis_status mcl_color_stage(Ctx* c, const mk::MclArgs& s);

}  // namespace

extern "C" {

void mantis_default_mcl_params(mantis_mcl_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(mantis_mcl_params);
  p->n_particles = 256;
  p->sigma_rot = 0.03;
  p->sigma_t = 0.01;
  p->tau = MANTIS_MCL_TAU_DEFAULT;
  p->resample_frac = 0.5;
  p->min_projections = 10;
  p->record = 0;
}

void mantis_mcl_sizes(int32_t* params_bytes, int32_t* result_bytes) {
  if (params_bytes) *params_bytes = (int32_t)sizeof(mantis_mcl_params);
  if (result_bytes) *result_bytes = (int32_t)sizeof(mantis_mcl_result);
}

mantis_status mantis_mcl_init(void* ctx, const double* T_w_b_mean, double sigma_rot0, double sigma_t0,
                              const mantis_mcl_params* p) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  if (!T_w_b_mean) return mcl_fail(c, "null argument");
  if (mantis_status e = mcl_check_params(c, p)) return e;
  if (!(sigma_rot0 >= 0 && sigma_rot0 <= 1e6) || !(sigma_t0 >= 0) || !std::isfinite(sigma_t0))
    return mcl_fail(c, "sigma_rot0 / sigma_t0 must be finite and >= 0 (sigma_rot0 <= 1e6)");
  for (int i = 0; i < 16; i++)
    if (!std::isfinite(T_w_b_mean[i])) return mcl_fail(c, "T_w_b_mean is not finite");
  const Xf mean = mk::track::xf_from_mat4(T_w_b_mean);
  std::vector<Xf> T(p->n_particles);
  uint64_t s = c->rng_state;
  for (Xf& t : T) {
    float g[6];
    for (float& v : g) v = rng_gauss(s);
    t = mk::track::particle(mean, g, sigma_rot0, sigma_t0);
  }
  if (mantis_status e = mcl_upload(c, T, p)) return e;
  c->rng_state = s;
  return MANTIS_OK;
}

mantis_status mantis_mcl_init_particles(void* ctx, const double* T_w_b, const mantis_mcl_params* p) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  if (!T_w_b) return mcl_fail(c, "null argument");
  if (mantis_status e = mcl_check_params(c, p)) return e;
  for (size_t i = 0; i < (size_t)16 * p->n_particles; i++)
    if (!std::isfinite(T_w_b[i])) return mcl_fail(c, "T_w_b is not finite");
  std::vector<Xf> T(p->n_particles);
  for (int j = 0; j < p->n_particles; j++) T[j] = mk::track::xf_from_mat4(T_w_b + 16 * (size_t)j);
  return mcl_upload(c, T, p);
}

mantis_status mantis_mcl_reset(void* ctx) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  c->mcl.live = false;
  c->mcl.has_record = false;
  c->mcl.has_modes = false;
  return MANTIS_OK;
}

mantis_status mantis_mcl_step(void* ctx, const mantis_image* cams, int32_t n_cams, const mantis_motion* motion,
                              mantis_result* out, mantis_mcl_result* mout) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  Ctx::Mcl& m = c->mcl;
  if (!m.live) {
    c->err = "mcl: no particle set (mantis_mcl_init or mantis_mcl_init_particles)";
    return MANTIS_ERR_STATE;
  }
  if (!cams || !out) return mcl_fail(c, "null argument");
  if (!c->d_lm || c->nw + c->nr + c->ng <= 0) return mcl_fail(c, "map not set (mantis_set_map)");
  const int C = n_cams, N = m.N;
  if (C <= 0) return mcl_fail(c, "n_cams must be positive");
  if (C > mk::track::kMaxCams) return mcl_fail(c, "n_cams exceeds 8");
  if (C > c->F) return mcl_fail(c, "n_cams exceeds max_cams");
  for (int i = 0; i < C; i++) {
    if (cams[i].width != cams[0].width || cams[i].height != cams[0].height)
      return mcl_fail(c, "all frames of a step must share one size");
    if (!cams[i].bgr || cams[i].step_bytes < 3 * cams[i].width) return mcl_fail(c, "bgr8 image with step >= 3*width required");
    for (int k = 0; k < 16; k++)
      if (!std::isfinite(cams[i].T_base_cam[k])) return mcl_fail(c, "T_base_cam is not finite");
  }
  if (cams[0].width <= 2 || cams[0].height <= 2 || cams[0].width > c->Wmax || cams[0].height > c->Hmax)
    return mcl_fail(c, "image size outside [3, max]");
  bool has_motion = false;
  if (motion) {
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(motion->delta_pos[k])) return mcl_fail(c, "motion is not finite");
    double n2 = 0;
    for (int k = 0; k < 4; k++) {
      if (!std::isfinite(motion->delta_quat_xyzw[k])) return mcl_fail(c, "motion is not finite");
      n2 += motion->delta_quat_xyzw[k] * motion->delta_quat_xyzw[k];
    }
    has_motion = n2 >= 0.5;
  }

  // inputs in one pinned block: extrinsics (8 slots), the motion, the gaussians in draw order
  Xf* h_ext = (Xf*)m.h_in.get();
  Xf* h_delta = h_ext + mk::track::kMaxCams;
  float* h_g = (float*)(h_delta + 1);
  for (int i = 0; i < C; i++) h_ext[i] = mk::track::xf_from_mat4(cams[i].T_base_cam);
  std::memset(h_delta, 0, sizeof(Xf));
  if (has_motion) {
    double D[16];
    quat_to_mat4(motion->delta_quat_xyzw, motion->delta_pos, D);
    *h_delta = mk::track::xf_from_mat4(D);
  }
  uint64_t s = c->rng_state;
  for (size_t k = 0; k < (size_t)N * 6; k++) h_g[k] = rng_gauss(s);
  s = mc::rng_next(s);
  const uint32_t U = (uint32_t)s;
  const size_t in_bytes = sizeof(Xf) * (mk::track::kMaxCams + 1) + sizeof(float) * (size_t)N * 6;

  const int color = m.color.enable;  // as mantis_mcl_set_color left it: 0 = the step without colour
  if (color)
    if (mantis_status e = mcl_color_workspace(c)) return e;
  m.has_record = false;
  m.has_modes = false;  // the modes are the last step's
  m.recentred = false;  // and so is a correction of them (mantis_mcl_refine_modes)
  int W, H;
  mantis_status st = stage_frames(c, cams, C, W, H);
  if (st != MANTIS_OK) return st;
  if ((st = run_image_stages(c, C, W, H)) != MANTIS_OK) return st;
  HIP_OK(hipMemcpyAsync(m.d_in, m.h_in, in_bytes, hipMemcpyHostToDevice, c->s));

  mk::MclArgs a;
  a.T = (Xf*)m.d_T[m.cur];
  a.Tdst = (Xf*)m.d_T[m.cur ^ 1];
  a.ext = (const Xf*)m.d_in.get();
  a.delta = a.ext + mk::track::kMaxCams;
  a.gauss = (const float*)(a.delta + 1);
  a.L = m.d_L;
  a.Lprev = m.d_Lprev;
  a.q = m.d_q;
  a.cum = m.d_cum;
  a.anc = m.d_anc;
  a.c2w = (Xf*)m.d_c2w;
  a.pf = (PoseF*)m.d_pf;
  a.sums = m.d_sums;
  a.cnt = m.d_cnt;
  a.res = (mantis_mcl_result*)m.d_res;
  a.charge = color == 2 ? m.d_charge : nullptr;
  a.N = N;
  a.C = C;
  a.min_projections = m.p.min_projections;
  a.has_motion = has_motion ? 1 : 0;
  a.U = U;
  a.sigma_rot = m.p.sigma_rot;
  a.sigma_t = m.p.sigma_t;
  a.tau = m.p.tau;
  a.resample_frac = m.p.resample_frac;
  const int nb = (N + 255) / 256;
  mk::k_mcl_predict<<<nb, 256, 0, c->s>>>(a);
  HIP_OK(hipGetLastError());
  mark(c, "mcl_predict/k_mcl_predict");
  const dim3 grid((N + mk::kTrackPP - 1) / mk::kTrackPP, C);
  mk::k_mcl_score<kPfThreads, kPfSplit><<<grid, kPfThreads, 0, c->s>>>(c->d_frames, c->d_mbits, c->bstride, lmk_of(c), a);
  HIP_OK(hipGetLastError());
  mark(c, "mcl_score/k_mcl_score");
  if (color)
    if (mantis_status e = mcl_color_stage(c, a)) return e;
  if (color == 2) mk::k_mcl_weight<true><<<1, mk::kMclWT, 0, c->s>>>(a);
  else mk::k_mcl_weight<false><<<1, mk::kMclWT, 0, c->s>>>(a);
  HIP_OK(hipGetLastError());
  mark(c, "mcl_weight/k_mcl_weight");
  mk::k_mcl_resample<<<nb, 256, 0, c->s>>>(a);
  HIP_OK(hipGetLastError());
  mark(c, "mcl_resample/k_mcl_resample");
  HIP_OK(hipMemcpyAsync(m.h_res, m.d_res, sizeof(mantis_mcl_result), hipMemcpyDeviceToHost, c->s));
  HIP_OK(wait_stream(c, C));
  finish_profile(c);

  mantis_mcl_result r = *(const mantis_mcl_result*)m.h_res;
  r.status = MANTIS_OK;
  r.U = U;
  r.pad = 0;
  r.rng_state_after = s;
  c->rng_state = s;
  m.rec_pred = m.cur;  // the predicted poses stay in the buffer the step found the set in
  m.rec_C = C;
  m.rec_color = color;
  m.rec_color_min = m.color.min_color_projections;
  m.has_record = true;
  if (r.resampled) m.cur ^= 1;
  if (mout) *mout = r;
  std::memset(out, 0, sizeof(*out));
  out->status = MANTIS_OK;
  out->num_particles = N;
  out->rng_state_after = s;
  if (r.lost) return MANTIS_OK;  // publish = 0, the prior stays
  std::memcpy(c->prior_Twb, r.T_w_b, sizeof(c->prior_Twb));
  c->has_prior = true;
  out->publish = 1;
  const Xf T = mk::track::xf_from_mat4(r.T_w_b);
  const Quat q = basis_to_quat(T.R);
  out->orientation_xyzw[0] = q.x; out->orientation_xyzw[1] = q.y;
  out->orientation_xyzw[2] = q.z; out->orientation_xyzw[3] = q.w;
  for (int i = 0; i < 3; i++) out->position[i] = T.t[i];
  std::memcpy(out->covariance, r.covariance, sizeof(out->covariance));
  out->weight = r.best_error;
  return MANTIS_OK;
}

mantis_status mantis_mcl_get(void* ctx, double* T_w_b, double* log_w, int32_t* n) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  const Ctx::Mcl& m = c->mcl;
  if (!m.live) {
    c->err = "mcl: no particle set (mantis_mcl_init or mantis_mcl_init_particles)";
    return MANTIS_ERR_STATE;
  }
  if (n) *n = m.N;
  if (T_w_b) {
    std::vector<Xf> h(m.N);
    HIP_OK(hipMemcpy(h.data(), m.d_T[m.cur], sizeof(Xf) * m.N, hipMemcpyDeviceToHost));
    for (int j = 0; j < m.N; j++) mk::track::xf_to_mat4(h[j], T_w_b + 16 * (size_t)j);
  }
  if (log_w) HIP_OK(hipMemcpy(log_w, m.d_L, sizeof(double) * m.N, hipMemcpyDeviceToHost));
  return MANTIS_OK;
}

mantis_status mantis_mcl_get_record(void* ctx, double* T_w_b_pred, double* c2w, int64_t* sums, int32_t* counts,
                                    double* L_before, double* L_after, uint64_t* q, uint64_t* cum,
                                    int32_t* ancestors, int32_t* n_particles, int32_t* n_cams) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  const Ctx::Mcl& m = c->mcl;
  if (!m.live || !m.has_record || !m.p.record) {
    c->err = "mcl record: no step since the init, or the filter keeps none (params.record = 1)";
    return MANTIS_ERR_STATE;
  }
  const int N = m.N, C = m.rec_C;
  const size_t tasks = (size_t)N * C;
  if (n_particles) *n_particles = N;
  if (n_cams) *n_cams = C;
  static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(unsigned long long) == sizeof(uint64_t), "copied as is");
  if (T_w_b_pred) {
    std::vector<Xf> h(N);
    HIP_OK(hipMemcpy(h.data(), m.d_T[m.rec_pred], sizeof(Xf) * N, hipMemcpyDeviceToHost));
    for (int j = 0; j < N; j++) mk::track::xf_to_mat4(h[j], T_w_b_pred + 16 * (size_t)j);
  }
  if (c2w) {
    std::vector<Xf> h(tasks);
    HIP_OK(hipMemcpy(h.data(), m.d_c2w, sizeof(Xf) * tasks, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < tasks; k++) {
      std::memcpy(c2w + 12 * k, h[k].R, sizeof(double) * 9);
      std::memcpy(c2w + 12 * k + 9, h[k].t, sizeof(double) * 3);
    }
  }
  if (sums) HIP_OK(hipMemcpy(sums, m.d_sums, sizeof(int64_t) * tasks, hipMemcpyDeviceToHost));
  if (counts) HIP_OK(hipMemcpy(counts, m.d_cnt, sizeof(int32_t) * tasks, hipMemcpyDeviceToHost));
  if (L_before) HIP_OK(hipMemcpy(L_before, m.d_Lprev, sizeof(double) * N, hipMemcpyDeviceToHost));
  if (L_after) HIP_OK(hipMemcpy(L_after, m.d_L, sizeof(double) * N, hipMemcpyDeviceToHost));
  if (q) HIP_OK(hipMemcpy(q, m.d_q, sizeof(uint64_t) * N, hipMemcpyDeviceToHost));
  if (cum) HIP_OK(hipMemcpy(cum, m.d_cum, sizeof(uint64_t) * N, hipMemcpyDeviceToHost));
  if (ancestors) HIP_OK(hipMemcpy(ancestors, m.d_anc, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
  return MANTIS_OK;
}

}  // extern "C"
