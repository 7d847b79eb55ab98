// Rig tracking: the joint multi-camera particle filter from a pose prior
// (mantis_track / mantis_track_batch, include/mantis.h). Included by api.hip
// (shares its Ctx, frame staging and image stages). The pool / pick / gate /
// particle rules are in mk_track.h (shared with the host build of the tests).
//
// Device work of one call, all on the context stream: the image stages up to
// the cleanImageByEdge bit plane (run_image_stages), then
//   k_track_particles (seed)            the prediction as the one "particle"
//   k_track_score                       its (sum, n) per camera
//   per iteration: k_track_particles    pool + pick the previous pass, draw the next particles
//                  k_track_score        their (sum, n) per camera
//   k_track_particles (last)            pool + pick the last pass, gate, result
// = 2 x iterations + 3 launches. Every hand-off between blocks -- the poses
// one wave per rig writes for the scoring blocks, the integer sums those
// blocks write for that wave -- crosses a kernel boundary: no last-block
// counter, no flag polled inside a kernel, so no agent-scope release / acquire
// is needed for a block to see another block's stores. No hipGraph capture.
#include "mk_track.h"

namespace mk {

struct TrackState {  // one rig between the launches
  Xf cur;            // current base pose T_w_b
  double err;        // its pooled error
  int32_t n, pad;    // its pooled landmark count
};

struct TrackArgs {
  const Xf* pred;            // rigs: predicted T_w_b
  const Xf* ext;             // rigs x C: T_base_cam
  const float* gauss;        // rigs x iterations x P x 6
  TrackState* st;            // rigs
  mantis_track_result* res;  // rigs
  // one pass = rigs x P particles (x C cameras); pass_poses / pass_tasks = the
  // stride between passes (record: every pass kept) or 0 (each pass overwrites the last)
  Xf* Twb;                   // [pass][rig][P]
  Xf* c2w;                   // [pass][rig][P][C]
  PoseF* pf;                 // the same poses as the FP32 screen reads them
  long long* sums;           // [pass][rig][P][C]
  int32_t* cnt;
  size_t pass_poses, pass_tasks;
  int32_t C, P, iterations, min_projections;
  double sigma_rot, sigma_t, max_error;
};

// One wave per rig. call = 0: the seed; 1 .. iterations: pool the previous
// pass, pick, draw iteration `call`'s particles; iterations + 1: pool the
// last pass, pick, gate, result. Pass k (0 = seed, k = iteration k) was
// written by call k and scored by the k_track_score launch after it.
__global__ __launch_bounds__(64) void k_track_particles(TrackArgs a, int call) {
  const int rig = blockIdx.x, lane = threadIdx.x;
  const int C = a.C, P = a.P;
  TrackState& S = a.st[rig];
  mantis_track_result& R = a.res[rig];
  Xf cur;
  double cur_err = DBL_MAX;
  int32_t cur_n = 0;
  if (call == 0) {
    cur = a.pred[rig];
  } else {
    // pool pass call - 1 over the cameras, per particle, and take the argmin
    // by (error, index); every lane ends with the same (be, bj, bn)
    const int pass = call - 1, np = pass == 0 ? 1 : P;
    const size_t t0 = (size_t)pass * a.pass_tasks + (size_t)rig * P * C;
    double be;
    int bj;
    int32_t bn;
    wave_argmin(np, [&](int j, int32_t& n) {
      return track::pool(a.sums + t0 + (size_t)j * C, a.cnt + t0 + (size_t)j * C, C, &n);
    }, be, bj, bn);
    if (pass == 0) {  // the seed's own error
      cur = S.cur;
      cur_err = be;
      cur_n = bn;
      if (lane == 0) R.seed_error = R.iter_err[0] = be;
    } else {
      cur_err = S.err;
      cur_n = S.n;
      const bool take = bj < np && be < cur_err;  // first strict minimum, strictly below the current error
      // the winner's pose as call `pass` wrote it (a uniform load: every lane holds it)
      cur = take ? a.Twb[(size_t)pass * a.pass_poses + (size_t)rig * P + bj] : S.cur;
      if (take) { cur_err = be; cur_n = bn; }
      if (lane == 0) {
        R.iter_pick[pass - 1] = take ? bj : -1;
        R.iter_err[pass] = cur_err;
      }
    }
  }
  if (call <= a.iterations) {
    // pass `call`: its particles' base poses, and per camera the world -> camera pose in FP64 and FP32
    const int np = call == 0 ? 1 : P;
    const float* g = a.gauss + ((size_t)rig * a.iterations + (call > 0 ? call - 1 : 0)) * P * 6;
    const size_t p0 = (size_t)call * a.pass_poses + (size_t)rig * P;
    const size_t t0 = (size_t)call * a.pass_tasks + (size_t)rig * P * C;
    for (int j = lane; j < np; j += 64) {
      const Xf T = call == 0 ? cur : track::particle(cur, g + (size_t)j * 6, a.sigma_rot, a.sigma_t);
      a.Twb[p0 + j] = T;
      for (int c = 0; c < C; c++) {
        const Xf v = track::cam_c2w(T, a.ext[(size_t)rig * C + c]);
        a.c2w[t0 + (size_t)j * C + c] = v;
        a.pf[t0 + (size_t)j * C + c] = posef_from(v);
      }
    }
  }
  if (lane == 0) {
    S.cur = cur;
    S.err = cur_err;
    S.n = cur_n;
    if (call == a.iterations + 1) {
      R.status = MANTIS_OK;
      R.n_proj = cur_n;
      R.n_scored = 1 + P * a.iterations;
      R.error = cur_err;
      R.tracked = track::gate(cur_err, cur_n, a.min_projections, a.max_error);
      track::xf_to_mat4(cur, R.T_w_b);
    }
  }
}

// Pass `pass` of every rig on every camera: block (chunk, camera, rig) scores
// particles [chunk * kTrackPP, ...) of the pass (np of them: 1 for the seed)
// with pose_score_block (kernels.hip; shared with k_mcl_score, whose particle
// set is one "rig" of up to 4096).
template <int NT, int SPLIT>
__global__ __launch_bounds__(NT) void k_track_score(const FrameDesc* __restrict__ frames,
                                                    const uint32_t* __restrict__ mbits, size_t bstride, Landmarks lmk,
                                                    TrackArgs a, int pass, int np) {
  const int chunk = blockIdx.x, cam = blockIdx.y, rig = blockIdx.z;
  pose_score_block<NT, SPLIT>(frames, mbits, bstride, lmk, a.c2w, a.pf, a.sums, a.cnt,
                               (size_t)pass * a.pass_tasks + (size_t)rig * a.P * a.C, a.C, rig * a.C + cam, cam, chunk,
                               np);
}
constexpr int kTrackPP = (kPfThreads / 64) / kPfSplit;  // k_track_score's particles per block

}  // namespace mk

namespace {

namespace trk = mk::track;

// workspaces for a call of R rigs x C cameras x P particles x I iterations
mantis_status track_workspace(Ctx* c, int R, int C, int P, int I, bool record) {
  Ctx::Track& t = c->trk;
  const size_t in_bytes = sizeof(Xf) * ((size_t)R + (size_t)R * C) + sizeof(float) * (size_t)R * I * P * 6;
  const size_t passes = record ? (size_t)I + 1 : 1;
  const size_t poses = passes * R * P, tasks = poses * C;
  if (in_bytes > t.d_in.capacity() || (size_t)R > t.d_state.capacity() || poses > t.d_Twb.capacity() ||
      tasks > t.d_c2w.capacity())
    HIP_OK(hipStreamSynchronize(c->s));  // nothing of an earlier call still reads what is freed
  if (t.d_in.grow(c, in_bytes) || t.h_in.grow(c, in_bytes) || t.d_state.grow(c, (size_t)R) ||
      t.d_res.grow(c, (size_t)R) || t.h_res.grow(c, (size_t)R) || t.d_Twb.grow(c, poses) || t.d_c2w.grow(c, tasks) ||
      t.d_pf.grow(c, tasks) || t.d_sums.grow(c, tasks) || t.d_cnt.grow(c, tasks))
    return MANTIS_ERR_OOM;
  return MANTIS_OK;
}

mantis_status track_fail(Ctx* c, const char* what) {
  c->err = std::string("track: ") + what;
  return MANTIS_ERR_ARG;
}

mantis_status track_impl(Ctx* c, const mantis_image* cams, int32_t n_rigs, int32_t C, const double* pred,
                         const mantis_track_params* p, mantis_track_result* out) {
  if (!cams || !pred || !p || !out) return track_fail(c, "null argument");
  if (p->struct_size != (int32_t)sizeof(mantis_track_params)) return track_fail(c, "params.struct_size mismatch");
  if (!c->d_lm || c->nw + c->nr + c->ng <= 0) return track_fail(c, "map not set (mantis_set_map)");
  if (n_rigs <= 0 || C <= 0) return track_fail(c, "n_rigs and cams_per_rig must be positive");
  if (C > trk::kMaxCams) return track_fail(c, "cams_per_rig exceeds 8");
  if ((int64_t)n_rigs * C > c->F) return track_fail(c, "n_rigs x cams_per_rig exceeds max_cams");
  const int P = p->particles, I = p->iterations;
  if (P < 1 || P > trk::kMaxParticles) return track_fail(c, "particles outside 1..96");
  if (I < 0 || I > trk::kMaxIterations) return track_fail(c, "iterations outside 0..10");
  if (P * C > trk::kMaxTasks) return track_fail(c, "particles x cams_per_rig exceeds 512");
  if (!(p->sigma_rot >= 0 && p->sigma_rot <= 1e6) || !(p->sigma_t >= 0) || !std::isfinite(p->sigma_t))
    return track_fail(c, "sigma_rot / sigma_t must be finite and >= 0 (sigma_rot <= 1e6)");
  if (std::isnan(p->max_error)) return track_fail(c, "max_error is NaN");
  if (p->record != 0 && p->record != 1) return track_fail(c, "record must be 0 or 1");
  const int n = n_rigs * C;
  for (int i = 0; i < n; i++) {
    if (cams[i].width != cams[0].width || cams[i].height != cams[0].height)
      return track_fail(c, "all frames of a call must share one size");
    if (!cams[i].bgr || cams[i].step_bytes < 3 * cams[i].width) return track_fail(c, "bgr8 image with step >= 3*width required");
  }
  if (cams[0].width <= 2 || cams[0].height <= 2 || cams[0].width > c->Wmax || cams[0].height > c->Hmax)
    return track_fail(c, "image size outside [3, max]");
  for (int i = 0; i < 16 * n_rigs; i++)
    if (!std::isfinite(pred[i])) return track_fail(c, "T_w_b_pred is not finite");

  Ctx::Track& t = c->trk;
  t.rigs = 0;  // no record until this call has finished
  if (mantis_status e = track_workspace(c, n_rigs, C, P, I, p->record != 0)) return e;

  // inputs in one pinned block: predictions, extrinsics, then every rig's
  // gaussians in draw order (rig-major; a rig draws whether or not it ends up tracked)
  Xf* h_pred = (Xf*)t.h_in.get();
  Xf* h_ext = h_pred + n_rigs;
  float* h_g = (float*)(h_ext + (size_t)n);
  for (int r = 0; r < n_rigs; r++) h_pred[r] = trk::xf_from_mat4(pred + 16 * (size_t)r);
  for (int i = 0; i < n; i++) h_ext[i] = trk::xf_from_mat4(cams[i].T_base_cam);
  const size_t per = (size_t)P * I * 6;
  std::vector<uint64_t> states(n_rigs);
  uint64_t s = c->rng_state;
  for (int r = 0; r < n_rigs; r++) {
    for (size_t k = 0; k < per; k++) h_g[(size_t)r * per + k] = rng_gauss(s);
    states[r] = s;
  }
  const size_t in_bytes = sizeof(Xf) * ((size_t)n_rigs + n) + sizeof(float) * per * n_rigs;

  int W, H;
  mantis_status st = stage_frames(c, cams, n, W, H);
  if (st != MANTIS_OK) return st;
  if ((st = run_image_stages(c, n, W, H)) != MANTIS_OK) return st;
  HIP_OK(hipMemcpyAsync(t.d_in, t.h_in, in_bytes, hipMemcpyHostToDevice, c->s));

  TrackArgs a;
  a.pred = (const Xf*)t.d_in.get();
  a.ext = a.pred + n_rigs;
  a.gauss = (const float*)(a.ext + (size_t)n);
  a.st = (TrackState*)t.d_state;
  a.res = (mantis_track_result*)t.d_res;
  a.Twb = (Xf*)t.d_Twb;
  a.c2w = (Xf*)t.d_c2w;
  a.pf = (PoseF*)t.d_pf;
  a.sums = t.d_sums;
  a.cnt = t.d_cnt;
  a.pass_poses = p->record ? (size_t)n_rigs * P : 0;
  a.pass_tasks = a.pass_poses * C;
  a.C = C;
  a.P = P;
  a.iterations = I;
  a.min_projections = p->min_projections;
  a.sigma_rot = p->sigma_rot;
  a.sigma_t = p->sigma_t;
  a.max_error = p->max_error;
  const Landmarks L = lmk_of(c);
  for (int call = 0; call <= I + 1; call++) {
    k_track_particles<<<n_rigs, 64, 0, c->s>>>(a, call);
    HIP_OK(hipGetLastError());
    mark(c, "track_particles/k_track_particles");
    if (call > I) break;
    const int np = call == 0 ? 1 : P;
    const dim3 grid((np + kTrackPP - 1) / kTrackPP, C, n_rigs);
    k_track_score<kPfThreads, kPfSplit><<<grid, kPfThreads, 0, c->s>>>(c->d_frames, c->d_mbits, c->bstride, L, a, call, np);
    HIP_OK(hipGetLastError());
    mark(c, "track_score/k_track_score");
  }
  HIP_OK(hipMemcpyAsync(t.h_res, t.d_res, sizeof(mantis_track_result) * n_rigs, hipMemcpyDeviceToHost, c->s));
  HIP_OK(wait_stream(c, n));
  finish_profile(c);
  const mantis_track_result* hr = (const mantis_track_result*)t.h_res;
  for (int r = 0; r < n_rigs; r++) {
    out[r] = hr[r];
    // passes that did not run (iterations < 10) read as "no particle", the error staying where it was
    for (int k = I; k < trk::kMaxIterations; k++) {
      out[r].iter_pick[k] = -1;
      out[r].iter_err[k + 1] = out[r].error;
    }
    out[r].rng_state_after = states[r];
  }
  c->rng_state = s;
  t.rigs = n_rigs;
  t.C = C;
  t.P = P;
  t.I = I;
  t.record = p->record;
  return MANTIS_OK;
}

}  // namespace

extern "C" {

void mantis_default_track_params(void* ctx, mantis_track_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(mantis_track_params);
  p->particles = 50;
  p->iterations = 10;
  if (const Ctx* c = (const Ctx*)ctx) {
    if (c->cfg.particles >= 1 && c->cfg.particles <= trk::kMaxParticles) p->particles = c->cfg.particles;
    if (c->cfg.iterations >= 0 && c->cfg.iterations <= trk::kMaxIterations) p->iterations = c->cfg.iterations;
  }
  p->sigma_rot = 0.03;
  p->sigma_t = 0.01;
  p->min_projections = 10;
  p->record = 0;
  p->max_error = 0;
}

void mantis_track_sizes(int32_t* params_bytes, int32_t* result_bytes) {
  if (params_bytes) *params_bytes = (int32_t)sizeof(mantis_track_params);
  if (result_bytes) *result_bytes = (int32_t)sizeof(mantis_track_result);
}

mantis_status mantis_track_batch(void* ctx, const mantis_image* cams, int32_t n_rigs, int32_t cams_per_rig,
                                 const double* T_w_b_pred, const mantis_track_params* p, mantis_track_result* out) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  return track_impl(c, cams, n_rigs, cams_per_rig, T_w_b_pred, p, out);
}

mantis_status mantis_track(void* ctx, const mantis_image* cams, int32_t n_cams, const mantis_motion* motion,
                           const mantis_track_params* p, mantis_result* out, mantis_track_result* tout) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  if (!out) return track_fail(c, "null argument");
  if (!c->has_prior) {
    c->err = "track: no prior pose (mantis_set_prior_pose, or a published mantis_process call)";
    return MANTIS_ERR_STATE;
  }
  double pred[16];
  const double* pq = motion ? motion->delta_quat_xyzw : nullptr;
  if (motion && pq[0] * pq[0] + pq[1] * pq[1] + pq[2] * pq[2] + pq[3] * pq[3] >= 0.5) {
    double D[16];
    quat_to_mat4(motion->delta_quat_xyzw, motion->delta_pos, D);
    mat4_mul(c->prior_Twb, D, pred);
  } else {
    std::memcpy(pred, c->prior_Twb, sizeof(pred));
  }
  mantis_track_result tmp;
  mantis_track_result* tr = tout ? tout : &tmp;
  const mantis_status st = track_impl(c, cams, 1, n_cams, pred, p, tr);
  if (st != MANTIS_OK) return st;
  std::memset(out, 0, sizeof(*out));
  out->status = MANTIS_OK;
  out->num_particles = tr->n_scored;
  out->rng_state_after = tr->rng_state_after;
  if (!tr->tracked) return MANTIS_OK;  // publish = 0, the prior stays: the caller falls back to mantis_process
  std::memcpy(c->prior_Twb, tr->T_w_b, sizeof(c->prior_Twb));
  out->publish = 1;
  const Xf T = trk::xf_from_mat4(tr->T_w_b);
  const Quat q = basis_to_quat(T.R);  // Matrix3x3::getRotation, as the published poses of the pipeline
  out->orientation_xyzw[0] = q.x; out->orientation_xyzw[1] = q.y;
  out->orientation_xyzw[2] = q.z; out->orientation_xyzw[3] = q.w;
  for (int i = 0; i < 3; i++) out->position[i] = T.t[i];
  for (int i = 0; i < 6; i++) out->covariance[i * 6 + i] = tr->error * (1.0 / 600.0);  // PosePub.h:47-56
  out->weight = tr->error;
  return MANTIS_OK;
}

mantis_status mantis_get_track_record(void* ctx, int32_t rig, int32_t iteration, double* T_w_b, double* c2w,
                                      int64_t* sums, int32_t* counts, int32_t* n_particles) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  const Ctx::Track& t = c->trk;
  if (!t.rigs || !t.record) {
    c->err = "track record: the last track call kept none (params.record = 1)";
    return MANTIS_ERR_STATE;
  }
  const int pass = iteration < 0 ? 0 : iteration;
  if (rig < 0 || rig >= t.rigs || iteration == 0 || iteration < -1 || iteration > t.I)
    return track_fail(c, "record: rig or iteration out of range (-1 = seed, 1 .. iterations)");
  const int np = pass == 0 ? 1 : t.P, C = t.C;
  if (n_particles) *n_particles = np;
  const size_t p0 = ((size_t)pass * t.rigs + rig) * t.P, t0 = p0 * C;
  std::vector<Xf> hp(np), hc((size_t)np * C);
  static_assert(sizeof(long long) == sizeof(int64_t), "sums are copied as int64");
  HIP_OK(hipMemcpy(hp.data(), (const Xf*)t.d_Twb + p0, sizeof(Xf) * np, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(hc.data(), (const Xf*)t.d_c2w + t0, sizeof(Xf) * np * C, hipMemcpyDeviceToHost));
  if (sums) HIP_OK(hipMemcpy(sums, t.d_sums + t0, sizeof(int64_t) * np * C, hipMemcpyDeviceToHost));
  if (counts) HIP_OK(hipMemcpy(counts, t.d_cnt + t0, sizeof(int32_t) * np * C, hipMemcpyDeviceToHost));
  for (int j = 0; j < np && T_w_b; j++) trk::xf_to_mat4(hp[j], T_w_b + 16 * (size_t)j);
  for (size_t k = 0; k < (size_t)np * C && c2w; k++) {
    std::memcpy(c2w + 12 * k, hc[k].R, sizeof(double) * 9);
    std::memcpy(c2w + 12 * k + 9, hc[k].t, sizeof(double) * 3);
  }
  return MANTIS_OK;
}

}  // extern "C"
