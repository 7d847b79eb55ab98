// Monte Carlo localization, the modes of the set: mantis_mcl_init_lattice,
// mantis_mcl_modes and mantis_mcl_select_mode (include/mantis.h). Included by
// api.hip after mcl_impl.hip, whose context state, workspace and upload it
// uses. The key, bin, order and lattice rules are in mk_mcl_modes.h (shared
// with the host build of the tests).
//
// Device work, on the context stream:
//   k_mcl_modes   grid = max_modes blocks of 256. Every block rebuilds the
//                 901-bin table (W, n, packed heaviest) in LDS from the last
//                 step's predicted poses and q, block b takes the first b + 1
//                 bins of the mode order by repeated block maximum and writes
//                 mode b's record (moments about the bin's heaviest particle,
//                 then the covariance about the mean); block 0 also the header.
//                 The blocks share nothing but their inputs.
//   k_mcl_keep    one block of 1024: the keys of the current set, the count of
//                 the particles in the chosen bin, and -inf into the others' L
//                 when that count is positive.
// No counter, no polled flag, no hipGraph capture: each call is one launch and
// one D2H copy of its result.
#include "mk_mcl_modes.h"

// the struct shares its name with the call: an elaborated name everywhere but here
using mcl_modes_rec = struct mantis_mcl_modes;

namespace mk {

static_assert(sizeof(mcl::Mode) == sizeof(mantis_mcl_mode) && sizeof(mcl::Modes) == sizeof(mcl_modes_rec),
              "mk_mcl_modes.h restates the layout of include/mantis.h");
static_assert(offsetof(mcl::Mode, weight) == offsetof(mantis_mcl_mode, weight) &&
                  offsetof(mcl::Mode, covariance) == offsetof(mantis_mcl_mode, covariance) &&
                  offsetof(mcl::Modes, anchor_T_w_b) == offsetof(mcl_modes_rec, anchor_T_w_b) &&
                  offsetof(mcl::Modes, mode) == offsetof(mcl_modes_rec, mode),
              "mk_mcl_modes.h restates the layout of include/mantis.h");

constexpr int kMclMT = 256;  // k_mcl_modes' block: a lane may use up to 512 VGPRs
constexpr int kMclNoBin = 0xffff;  // s_bin of a particle with q = 0

struct MclModesArgs {
  const Xf* T;  // the last step's predicted poses
  const unsigned long long* q;
  const long long* sums;  // N x C
  const int32_t* cnt;
  mcl::Modes* out;
  int32_t N, C, best, max_modes;
  double g;
};

// K sums over a block of 256, every thread gets them: wave shuffles, then the
// 4 wave totals added in wave order by every thread
template <int K>
__device__ inline void mcl_modes_sum(double* v, double (*sh)[kMclMT / 64]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; k++)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; k++) sh[k][wave] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; k++) {
    double t = 0;
#pragma unroll
    for (int w = 0; w < kMclMT / 64; w++) t += sh[k][w];
    v[k] = t;
  }
}

__global__ __launch_bounds__(kMclMT) void k_mcl_modes(MclModesArgs a) {
  constexpr int NT = kMclMT, kW = NT / 64, kBins = mcl::kModeBins;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, b = blockIdx.x;
  const int rounds = (N + NT - 1) / NT;  // <= kMclMRounds (N <= 4096, checked by the host)
  __shared__ unsigned long long s_W[kBins + 1], s_pk[kBins + 1];
  __shared__ int s_n[kBins + 1];
  __shared__ unsigned short s_bin[mcl::kMaxParticles];
  __shared__ double s_red[21][kW];
  __shared__ unsigned long long s_u[2][kW];
  __shared__ int s_i[kW];
  mcl::Modes& O = *a.out;

  for (int k = tid; k <= kBins; k += NT) {
    s_W[k] = 0;
    s_pk[k] = 0;
    s_n[k] = 0;
  }
  __syncthreads();
  const Xf A = a.T[a.best];  // 0 <= best < N: checked by the host
  for (int r = 0; r < rounds; r++) {
    const int j = r * NT + tid;
    if (j >= N) continue;
    const unsigned long long q = a.q[j];
    int bin = kMclNoBin;
    if (q) {
      Xf T;  // the key reads the translation's x, y and the base x-axis' x, y alone
      T.R[0] = a.T[j].R[0];
      T.R[3] = a.T[j].R[3];
      T.t[0] = a.T[j].t[0];
      T.t[1] = a.T[j].t[1];
      int32_t ix, iy, k;
      bin = mcl::cell_key(T, A, a.g, &ix, &iy, &k);  // <= kBins
      atomicAdd(&s_W[bin], q);
      atomicAdd(&s_n[bin], 1);
      atomicMax(&s_pk[bin], (unsigned long long)mcl::heaviest_pack(q, j));
    }
    s_bin[j] = (unsigned short)bin;
  }
  __syncthreads();

  // S and the non-empty in-range bins (integers: exact in any order)
  unsigned long long wsum = 0;
  int cells = 0;
  for (int k = tid; k <= kBins; k += NT) {
    wsum += s_W[k];
    cells += k < kBins && s_n[k] > 0;
  }
  for (int o = 32; o > 0; o >>= 1) {
    wsum += __shfl_xor(wsum, o);
    cells += __shfl_xor(cells, o);
  }
  if (lane == 0) {
    s_u[0][wave] = wsum;
    s_i[wave] = cells;
  }
  __syncthreads();
  wsum = 0;
  cells = 0;
  for (int w = 0; w < kW; w++) {
    wsum += s_u[0][w];
    cells += s_i[w];
  }
  const unsigned long long S = wsum;
  const int n_modes = cells < a.max_modes ? cells : a.max_modes;

  if (b == 0 && tid == 0) {
    O.status = 0;
    O.n_modes = n_modes;
    O.n_cells = cells;
    O.n_outside = s_n[kBins];
    O.weight_sum = S;
    O.outside_weight = s_W[kBins];
    track::xf_to_mat4(A, O.anchor_T_w_b);
  }
  mcl::Mode& M = O.mode[b];
  if (b >= n_modes) {  // block-uniform
    if (tid == 0) mcl::mode_clear(M);
    return;
  }

  // the first b + 1 bins of the mode order: the block maximum of (W, bin), taken out, again
  int bin = 0;
  unsigned long long Wb = 0;
  for (int m = 0; m <= b; m++) {
    unsigned long long top = 0;
    for (int k = tid; k < kBins; k += NT) {
      const unsigned long long key = mcl::mode_order_key(s_W[k], k);
      top = key > top ? key : top;
    }
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long t = __shfl_xor(top, o);
      top = t > top ? t : top;
    }
    if (lane == 0) s_u[1][wave] = top;  // s_u[0] may still be read for S; a pass ends with a barrier
    __syncthreads();
    top = s_u[1][0];
    for (int w = 1; w < kW; w++) top = s_u[1][w] > top ? s_u[1][w] : top;
    if (!top) return;  // cannot be (m < n_modes <= the non-empty bins); block-uniform
    bin = mcl::mode_order_bin(top);
    Wb = top >> 10;
    __syncthreads();  // every thread has read s_W[bin]'s key before it goes
    if (tid == 0) s_W[bin] = 0;
    __syncthreads();
  }
  const int nb = s_n[bin], jb = mcl::heaviest_index(s_pk[bin]);

  // the estimate of the bin: first moments about its heaviest particle, then the covariance about the mean
  const Xf Tb = a.T[jb];
  const Quat qb = basis_to_quat(Tb.R);
  double m7[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int r = 0; r < rounds; r++) {
    const int j = r * NT + tid;
    if (j >= N || s_bin[j] != bin) continue;
    double t7[7];
    mcl::mean_terms(a.T[j], Tb, qb, (double)a.q[j] / (double)Wb, t7);
#pragma unroll
    for (int k = 0; k < 7; k++) m7[k] += t7[k];
  }
  mcl_modes_sum<7>(m7, s_red);
  Quat qs;
  const Xf Tm = mcl::mean_pose(Tb, qb, m7, nb == 1, &qs);
  double c21[21];
#pragma unroll
  for (int k = 0; k < 21; k++) c21[k] = 0;
  for (int r = 0; r < rounds; r++) {
    const int j = r * NT + tid;
    if (j >= N || s_bin[j] != bin) continue;
    double xi[6], t21[21];
    mcl::xi_of(a.T[j], Tm, qs, xi);
    mcl::cov_terms(xi, (double)a.q[j] / (double)Wb, t21);
#pragma unroll
    for (int k = 0; k < 21; k++) c21[k] += t21[k];
  }
  mcl_modes_sum<21>(c21, s_red);

  if (tid == 0) {
    mcl::bin_cell(bin, &M.ix, &M.iy, &M.yaw_quadrant);
    M.n = nb;
    M.best = jb;
    M.pad = 0;
    M.weight = Wb;
    M.share = (double)Wb / (double)S;
    int32_t np;
    M.best_error = track::pool(a.sums + (size_t)jb * a.C, a.cnt + (size_t)jb * a.C, a.C, &np);
    track::xf_to_mat4(Tm, M.T_w_b);
    mcl::cov_expand(c21, M.covariance);
  }
}

struct MclKeepArgs {
  const Xf* T;  // the current set
  double* L;
  int32_t* kept;  // the result: particles of the set in the chosen bin
  Xf A;           // the anchor of the modes call
  double g;
  int32_t N, bin;
};

// One block. Particle j = round * 1024 + tid, at most 4 rounds.
__global__ __launch_bounds__(kMclWT) void k_mcl_keep(MclKeepArgs a) {
  constexpr int NT = kMclWT, kW = NT / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ int s_c[kW];
  bool in[kMclRounds];
  int c = 0;
#pragma unroll
  for (int r = 0; r < kMclRounds; r++) {
    const int j = r * NT + tid;
    in[r] = false;
    if (j < a.N) {
      int32_t ix, iy, k;
      in[r] = mcl::cell_key(a.T[j], a.A, a.g, &ix, &iy, &k) == a.bin;
      c += in[r];
    }
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) s_c[wave] = c;
  __syncthreads();
  c = 0;
  for (int w = 0; w < kW; w++) c += s_c[w];
  if (tid == 0) *a.kept = c;
  if (c <= 0) return;  // block-uniform: nothing changes
#pragma unroll
  for (int r = 0; r < kMclRounds; r++) {
    const int j = r * NT + tid;
    if (j < a.N && !in[r]) a.L[j] = -INFINITY;
  }
}

}  // namespace mk

namespace {

mantis_status mcl_state(Ctx* c, const char* what) {
  c->err = std::string("mcl: ") + what;
  return MANTIS_ERR_STATE;
}

// the result buffers of the two calls: the modes record and the kept count behind it
mantis_status mcl_modes_buffers(Ctx* c) {
  Ctx::Mcl& m = c->mcl;
  const size_t bytes = sizeof(mcl_modes_rec) + 16;
  if (m.d_modes.grow(c, bytes) || m.h_modes.grow(c, bytes)) return MANTIS_ERR_OOM;
  return MANTIS_OK;
}

}  // namespace

extern "C" {

void mantis_mcl_modes_sizes(int32_t* mode_bytes, int32_t* modes_bytes) {
  if (mode_bytes) *mode_bytes = (int32_t)sizeof(mantis_mcl_mode);
  if (modes_bytes) *modes_bytes = (int32_t)sizeof(mcl_modes_rec);
}

mantis_status mantis_mcl_init_lattice(void* ctx, const double* T_w_b_mean, double sigma_rot0, double sigma_t0,
                                      int32_t cells_x, int32_t cells_y, const mantis_mcl_params* p) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  if (!T_w_b_mean) return mcl_fail(c, "null argument");
  if (mantis_status e = mcl_check_params(c, p)) return e;
  if (!(sigma_rot0 >= 0 && sigma_rot0 <= 1e6) || !(sigma_t0 >= 0) || !std::isfinite(sigma_t0))
    return mcl_fail(c, "sigma_rot0 / sigma_t0 must be finite and >= 0 (sigma_rot0 <= 1e6)");
  if (cells_x < 0 || cells_x > mc::kCellHalf || cells_y < 0 || cells_y > mc::kCellHalf)
    return mcl_fail(c, "cells_x / cells_y outside 0..7");
  const int n_sites = (2 * cells_x + 1) * (2 * cells_y + 1);
  if (p->n_particles < n_sites) return mcl_fail(c, "n_particles below the lattice's sites");
  const double g = c->cfg.grid_spacing;
  if (!(g > 0) || !std::isfinite(g)) return mcl_fail(c, "grid_spacing must be finite and > 0");
  for (int i = 0; i < 16; i++)
    if (!std::isfinite(T_w_b_mean[i])) return mcl_fail(c, "T_w_b_mean is not finite");
  const Xf mean = mk::track::xf_from_mat4(T_w_b_mean);
  std::vector<Xf> T(p->n_particles);
  uint64_t s = c->rng_state;
  for (int j = 0; j < p->n_particles; j++) {
    float gs[6];
    for (float& v : gs) v = rng_gauss(s);
    T[j] = mk::track::particle(mean, gs, sigma_rot0, sigma_t0);
    int32_t ix, iy;
    mc::lattice_site(j % n_sites, cells_x, cells_y, &ix, &iy);
    T[j].t[0] = T[j].t[0] + (double)ix * g;
    T[j].t[1] = T[j].t[1] + (double)iy * g;
  }
  if (mantis_status e = mcl_upload(c, T, p)) return e;
  c->rng_state = s;
  return MANTIS_OK;
}

mantis_status mantis_mcl_modes(void* ctx, int32_t max_modes, struct mantis_mcl_modes* out) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  Ctx::Mcl& m = c->mcl;
  if (!out) return mcl_fail(c, "null argument");
  if (max_modes < 1 || max_modes > mc::kMaxModes) return mcl_fail(c, "max_modes outside 1..8");
  if (!m.live || !m.has_record) return mcl_state(c, "modes: no step since the init");
  const double g = c->cfg.grid_spacing;
  if (!(g > 0) || !std::isfinite(g)) return mcl_fail(c, "grid_spacing must be finite and > 0");
  const mantis_mcl_result& last = *(const mantis_mcl_result*)m.h_res;  // the last step's, as it was copied back
  m.has_modes = false;
  if (last.lost || last.best < 0 || last.best >= m.N) {  // a lost step has no modes; nothing to launch
    std::memset(&m.modes, 0, sizeof(m.modes));
    for (int k = 0; k < mc::kMaxModes; k++) mc::mode_clear(((mc::Modes*)&m.modes)->mode[k]);
  } else {
    if (mantis_status e = mcl_modes_buffers(c)) return e;
    mk::MclModesArgs a;
    a.T = (const Xf*)m.d_T[m.rec_pred];
    a.q = m.d_q;
    a.sums = m.d_sums;
    a.cnt = m.d_cnt;
    a.out = (mc::Modes*)m.d_modes.get();
    a.N = m.N;
    a.C = m.rec_C;
    a.best = last.best;
    a.max_modes = max_modes;
    a.g = g;
    // blocks past max_modes are not launched: their records are cleared here, once the copy is back
    mk::k_mcl_modes<<<max_modes, mk::kMclMT, 0, c->s>>>(a);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(m.h_modes, m.d_modes, sizeof(mcl_modes_rec), hipMemcpyDeviceToHost, c->s));
    HIP_OK(hipStreamSynchronize(c->s));
    std::memcpy(&m.modes, m.h_modes, sizeof(m.modes));
    mc::Modes* r = (mc::Modes*)&m.modes;
    for (int k = max_modes; k < mc::kMaxModes; k++) mc::mode_clear(r->mode[k]);
  }
  m.modes.status = MANTIS_OK;
  m.modes_g = g;
  m.has_modes = true;
  *out = m.modes;
  return MANTIS_OK;
}

mantis_status mantis_mcl_select_mode(void* ctx, int32_t mode_index) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  Ctx::Mcl& m = c->mcl;
  if (!m.live || !m.has_record || !m.has_modes) return mcl_state(c, "select_mode: no mantis_mcl_modes call since the last step");
  if (mode_index < 0 || mode_index >= m.modes.n_modes) return mcl_fail(c, "mode_index is not below n_modes");
  if (mantis_status e = mcl_modes_buffers(c)) return e;
  const mantis_mcl_mode& k = m.modes.mode[mode_index];
  int32_t* d_kept = (int32_t*)((uint8_t*)m.d_modes + sizeof(mcl_modes_rec));
  const int32_t* h_kept = (const int32_t*)((const uint8_t*)m.h_modes + sizeof(mcl_modes_rec));
  mk::MclKeepArgs a;
  a.T = (const Xf*)m.d_T[m.cur];
  a.L = m.d_L;
  a.kept = d_kept;
  a.A = mk::track::xf_from_mat4(m.modes.anchor_T_w_b);
  a.g = m.modes_g;
  a.N = m.N;
  a.bin = mc::cell_bin(k.ix, k.iy, k.yaw_quadrant);
  mk::k_mcl_keep<<<1, mk::kMclWT, 0, c->s>>>(a);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync((void*)h_kept, d_kept, sizeof(int32_t), hipMemcpyDeviceToHost, c->s));
  HIP_OK(hipStreamSynchronize(c->s));
  if (*h_kept <= 0) return mcl_state(c, "select_mode: no particle of the current set lies in the mode");
  std::memcpy(c->prior_Twb, k.T_w_b, sizeof(c->prior_Twb));
  c->has_prior = true;
  return MANTIS_OK;
}

}  // extern "C"
