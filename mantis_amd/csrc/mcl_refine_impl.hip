// Monte Carlo localization, the modes refined on the grid lines and the set
// recentred on them: mantis_mcl_refine_modes (include/mantis.h). Included by
// api.hip after refine_impl.hip, whose kernels, workspaces and checks it uses,
// and after mcl_modes_impl.hip, whose modes call it makes. The plan and the
// move of a particle are in mk_mcl_refine.h (shared with the host build of the
// tests).
//
// Device work of one call of I iterations, all on the context stream:
//   k_mcl_modes                    as mantis_mcl_modes, one copy back
//   k_refine_obs / k_refine_step   per pass 0 .. I, the modes as rigs over the
//                                  one staged set of frames (rig_stride = 0);
//                                  one copy back of the modes' states
//   k_mcl_recentre                 only when a mode is applied: one particle
//                                  per thread, then one copy back of the counters
// The plan needs the refined poses and their gate (refine::conclude, a Cholesky
// on the host), so it is formed on the host between the states' copy and the
// recentre launch and travels as kernel arguments. No counter is waited on, no
// flag is polled, no hipGraph capture. Nothing is drawn.
#include "mk_mcl_refine.h"

using mcl_refined_rec = struct mantis_mcl_refined;

namespace mk {

static_assert(sizeof(mcl::Recentre) <= 1024, "the plan travels as kernel arguments");

struct MclRecentreArgs {
  const Xf* src;   // the current set
  Xf* dst;         // the same buffer, or the other one (the step's record lies in src)
  int32_t* moved;  // kMaxModes counters, cleared on the stream before the launch
  int32_t N, pad;
  mcl::Recentre P;
};

// grid ceil(N / 256) x 256, one particle per thread: its key against the
// anchor, the compare with the applied bins, the product with that mode's
// correction, one plain store. The plan is kernel arguments read by a uniform
// index: scalar operands. Per mode the movers of a wave are a ballot's
// popcount, added by lane 0 with one integer atomicAdd (exact in any order).
// Every lane reaches the ballots: no return before them.
__global__ __launch_bounds__(256) void k_mcl_recentre(MclRecentreArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  int32_t hit = -1;
  if (j < a.N) {
    Xf T = a.src[j];
    hit = mcl::recentre_pose(a.P, T);
    a.dst[j] = T;  // moved, or the same bits (in place or into the other buffer)
  }
  for (int k = 0; k < mcl::kMaxModes; k++) {
    if (k >= a.P.n_modes || a.P.bin[k] < 0) continue;  // uniform
    const unsigned long long b = __ballot(hit == k);
    if (lane == 0 && b) atomicAdd(&a.moved[k], (int32_t)__popcll(b));
  }
}

}  // namespace mk

namespace {

mantis_status mcl_refine_buffers(Ctx* c) {
  Ctx::Mcl& m = c->mcl;
  if (m.d_moved.grow(c, (size_t)mc::kMaxModes) || m.h_moved.grow(c, (size_t)mc::kMaxModes)) return MANTIS_ERR_OOM;
  return MANTIS_OK;
}

}  // namespace

extern "C" {

void mantis_mcl_refine_sizes(int32_t* mode_bytes, int32_t* refined_bytes) {
  if (mode_bytes) *mode_bytes = (int32_t)sizeof(mantis_mcl_mode_refined);
  if (refined_bytes) *refined_bytes = (int32_t)sizeof(mcl_refined_rec);
}

mantis_status mantis_mcl_refine_modes(void* ctx, const mantis_image* cams, int32_t n_cams, int32_t max_modes,
                                      const mantis_refine_params* p, int32_t apply, struct mantis_mcl_refined* out) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  Ctx::Mcl& m = c->mcl;
  if (!cams || !p || !out) return mcl_fail(c, "null argument");
  if (max_modes < 1 || max_modes > mc::kMaxModes) return mcl_fail(c, "max_modes outside 1..8");
  if (apply != 0 && apply != 1) return mcl_fail(c, "apply must be 0 or 1");
  if (!m.live || !m.has_record) return mcl_state(c, "refine_modes: no step since the init");
  const double g = c->cfg.grid_spacing;
  if (!(g > 0) || !std::isfinite(g)) return mcl_fail(c, "grid_spacing must be finite and > 0");
  // mantis_refine_batch's checks with one rig of n_cams frames: the modes never count against max_cams
  if (mantis_status e = refine_check(c, cams, 1, n_cams, p)) return e;
  if (apply && m.recentred)
    return mcl_state(c, "refine_modes: the set was already recentred since the last step (apply = 1 once per step)");
  if (mantis_status e = mcl_refine_buffers(c)) return e;

  mcl_modes_rec modes;
  if (mantis_status e = mantis_mcl_modes(ctx, max_modes, &modes)) return e;  // caches: mantis_mcl_select_mode may follow
  std::memset(out, 0, sizeof(*out));
  out->status = MANTIS_OK;
  out->n_modes = modes.n_modes;
  out->apply = apply;
  out->modes = modes;
  const int K = modes.n_modes;
  if (K <= 0) return MANTIS_OK;  // a lost step, or no in-range cell: nothing to refine

  double T_in[mc::kMaxModes * 16];
  mantis_refine_result res[mc::kMaxModes];
  for (int k = 0; k < K; k++) std::memcpy(T_in + 16 * k, modes.mode[k].T_w_b, sizeof(double) * 16);
  if (mantis_status e = refine_run(c, cams, K, n_cams, true, T_in, p, res)) return e;

  double T_ref[mc::kMaxModes * 16] = {0};
  int32_t refined[mc::kMaxModes] = {0}, key_kept[mc::kMaxModes], applied[mc::kMaxModes];
  for (int k = 0; k < K; k++) {
    out->mode[k].refine = res[k];
    std::memcpy(T_ref + 16 * k, res[k].T_w_b, sizeof(double) * 16);
    refined[k] = res[k].refined;
  }
  mk::MclRecentreArgs a;
  mc::refine_plan(*(const mc::Modes*)&modes, m.modes_g, T_ref, refined, apply, key_kept, applied, &a.P);
  bool any = false;
  for (int k = 0; k < K; k++) {
    out->mode[k].key_kept = key_kept[k];
    out->mode[k].applied = applied[k];
    any = any || applied[k];
  }
  if (!any) return MANTIS_OK;

  // the last step's record must survive: its predicted poses stay where they are
  const bool flip = m.cur == m.rec_pred;
  a.src = (const Xf*)m.d_T[m.cur];
  a.dst = (Xf*)m.d_T[flip ? m.cur ^ 1 : m.cur];
  a.moved = m.d_moved;
  a.N = m.N;
  a.pad = 0;
  HIP_OK(hipMemsetAsync(m.d_moved, 0, sizeof(int32_t) * mc::kMaxModes, c->s));
  mark(c, "start");
  mk::k_mcl_recentre<<<(m.N + 255) / 256, 256, 0, c->s>>>(a);
  HIP_OK(hipGetLastError());
  mark(c, "mcl_recentre/k_mcl_recentre");
  HIP_OK(hipMemcpyAsync(m.h_moved, m.d_moved, sizeof(int32_t) * mc::kMaxModes, hipMemcpyDeviceToHost, c->s));
  HIP_OK(hipStreamSynchronize(c->s));
  finish_profile(c, true);
  if (flip) m.cur ^= 1;
  for (int k = 0; k < K; k++) {
    out->mode[k].n_moved = applied[k] ? m.h_moved[k] : 0;
    out->n_moved += out->mode[k].n_moved;
  }
  if (out->n_moved > 0) m.recentred = true;
  return MANTIS_OK;
}

}  // extern "C"
