// Monte Carlo localization, the colour evidence (mantis_mcl_set_color /
// mantis_mcl_get_color_record / mantis_mcl_modes_color, include/mantis.h).
// Included by api.hip after mcl_modes_impl.hip. The rules are in
// mk_mcl_color.h (shared with the host build of the tests).
//
// k_mcl_color runs between k_mcl_score and k_mcl_weight when colour is on:
// one block owns kMclColorP particles over all the step's cameras, makes one
// plain store of (csum, cn) per (particle, camera) and writes the pooled Ec
// and the charge of its particles itself -- no cross-block pooling, every
// hand-off a kernel boundary. The cameras are the inner index of the block's
// pair space, pair g = ((particle p) C + camera c) ng + landmark l, so that
// the projections and the row loads of all the cameras are in flight together
// (a serial loop over the cameras, each with its own three barriers, measured
// 0.056 ms at N = 1024 x 4 cameras).
//   phase 1  one thread per pair: the exact FP64 projection, the validity
//            decision, x0 = cvRound(u - 5), y0, the "columns / rows are a run"
//            tests, into an LDS pair table
//   phase 2  (pair, window row) items over the whole block, four row loads in
//            flight per thread: color_row_run for the common row, the exact
//            per-pixel forms for the rest (kernels.hip, as block_score_color);
//            integer row sums added to the pair's LDS accumulator
//   phase 3  thread t = p C + c adds the window sums of its (particle,
//            camera); thread p then pools its particle (integers: order-free)
// The table holds kMclColorPairs = 640 pairs: 2 particles x 8 cameras x 37
// landmarks fit; anything larger (mantis_set_map takes up to 64 green
// landmarks) goes through it in chunks of 640 pairs.
// A map with no green landmark: the kernel still runs, every cn is 0, every Ec
// is DBL_MAX and every charge the miss charge.
#include "mk_mcl_color.h"

namespace mk {

constexpr int kMclColorT = 256;      // k_mcl_color's block
constexpr int kMclColorP = 2;        // particles per block
constexpr int kMclColorPairs = 640;  // the pair table (7.5 KB)

struct MclColorArgs {
  const Xf* c2w;     // N x C, as k_mcl_predict wrote them
  long long* csums;  // N x C
  int32_t* ccnt;     // N x C
  double* Ec;        // N
  double* charge;    // N
  int32_t N, C, min_color_projections, pad;
  double color_miss, color_tau;
};

struct MclColorPairs {
  int32_t x0[kMclColorPairs];   // cvRound(u - 5)
  int32_t yf[kMclColorPairs];   // cvRound(v - 5) << 6 | camera << 3 | yrun << 2 | xrun << 1 | ok
  int32_t acc[kMclColorPairs];  // window sum
};
struct MclColorCam {  // what a pair needs of its camera's frame
  const uint8_t* bgr;
  int32_t W, H;
  Cam cm;
};

__global__ __launch_bounds__(kMclColorT) void k_mcl_color(const FrameDesc* __restrict__ frames, Landmarks lmk,
                                                          MclColorArgs a) {
  constexpr int NT = kMclColorT, P = kMclColorP, kMaxC = track::kMaxCams;
  static_assert(P * kMaxC <= NT && kMaxC <= 8, "one thread per (particle, camera); the camera takes 3 bits of yf");
  __shared__ MclColorPairs cp;
  __shared__ Xf s_T[P * kMaxC];
  __shared__ MclColorCam s_cam[kMaxC];
  __shared__ long long s_cs[P * kMaxC];
  __shared__ int32_t s_cn[P * kMaxC];
  const int tid = threadIdx.x;
  const int j0 = blockIdx.x * P, nj = min(P, a.N - j0);
  if (nj <= 0) return;  // block-uniform (the grid covers N exactly)
  const double* green = lmk.xyz + 3 * (lmk.nw + lmk.nr);
  const int ng = lmk.ng, C = a.C;
  const int nt = nj * C;  // the block's (particle, camera) tasks, t = p C + c: a.c2w / csums / ccnt entry j0 C + t
  if (tid < nt) s_T[tid] = a.c2w[(size_t)j0 * C + tid];
  if (tid < C) {
    s_cam[tid].bgr = frames[tid].bgr;
    s_cam[tid].W = frames[tid].w;
    s_cam[tid].H = frames[tid].h;
    s_cam[tid].cm = frames[tid].cam;
  }
  long long cs = 0;  // thread t < nt: its task's sums
  int32_t cn = 0;
  const int npairs = nt * ng;  // pair g = t ng + l
  for (int base = 0; base < npairs; base += kMclColorPairs) {
    const int np = min(kMclColorPairs, npairs - base);
    __syncthreads();  // s_T, s_cam written; the last chunk's sums read
    for (int i = tid; i < np; i += NT) {
      const int g = base + i, t = g / ng, l = g - t * ng, c = t % C;
      const int W = s_cam[c].W, H = s_cam[c].H;
      double rp[3], u, v;
      xf_apply(s_T[t], green + 3 * l, rp);
      distort(s_cam[c].cm, rp[0], rp[1], rp[2], &u, &v);
      const int ok = rp[2] > 0 && in_frame(u, v, H, W);
      const int x0 = cv_round(u + (-5.0 + 0.0)), y0 = cv_round(v + (-5.0 + 0.0));
      int xrun = 1, yrun = 1;
#pragma unroll
      for (int k = 1; k < 10; k++) {
        xrun &= cv_round(u + (-5.0 + (double)k)) == x0 + k;
        yrun &= cv_round(v + (-5.0 + (double)k)) == y0 + k;
      }
      cp.x0[i] = x0;
      cp.yf[i] = (int32_t)((uint32_t)y0 << 6) | (c << 3) | (yrun << 2) | (xrun << 1) | ok;
      cp.acc[i] = 0;
    }
    __syncthreads();
    // (pair, row) items, row-major over the pairs so a wave's lanes add into different pairs
    const int ni = 10 * np;
    constexpr int kU = 4;
    for (int q0 = tid; q0 < ni; q0 += kU * NT) {
      int rsum[kU], slot[kU];
#pragma unroll
      for (int k = 0; k < kU; k++) {
        const int q = q0 + k * NT;
        slot[k] = -1;
        rsum[k] = 0;
        if (q >= ni) continue;
        const int r = q / np, i = q - r * np;
        const int yf = cp.yf[i];
        if (!(yf & 1)) continue;
        slot[k] = i;
        const int c = (yf >> 3) & 7;
        const uint8_t* bgr = s_cam[c].bgr;
        const int W = s_cam[c].W, H = s_cam[c].H;
        const long npx = (long)W * H;
        const int x0 = cp.x0[i], y = (yf >> 6) + r;
        const long lin0 = (long)y * W + x0;
        if ((yf & 6) == 6 && lin0 >= 0 && lin0 + 12 <= npx) {
          rsum[k] = color_row_run(bgr, lin0);
        } else if ((yf & 6) == 6) {  // a row reaching past the buffer: pixel by pixel, out-of-buffer reads 0 (Q10)
          int rs = 0;
          for (int ox = 0; ox < 10; ox++) {
            const long lin = lin0 + ox;
            int b = 0, gg = 0, rr = 0;
            if (lin >= 0 && lin < npx) {
              const uint32_t pv = load_bgr(bgr, lin, npx);
              b = (int)(pv & 0xffu);
              gg = (int)((pv >> 8) & 0xffu);
              rr = (int)((pv >> 16) & 0xffu);
            }
            rs += mcl::color_px_err(b, gg, rr);
          }
          rsum[k] = rs;
        } else {
          const int g = base + i, t = g / ng;
          rsum[k] = color_row_exact(s_T[t], green + 3 * (g - t * ng), s_cam[c].cm, bgr, W, H, r);
        }
      }
#pragma unroll
      for (int k = 0; k < kU; k++)
        if (slot[k] >= 0) atomicAdd(&cp.acc[slot[k]], rsum[k]);
    }
    __syncthreads();
    if (tid < nt) {  // the part of task tid's pairs that lies in this chunk
      const int lo = max(tid * ng, base), hi = min((tid + 1) * ng, base + np);
      for (int g = lo; g < hi; g++)
        if (cp.yf[g - base] & 1) {
          cs += cp.acc[g - base];
          cn++;
        }
    }
  }
  if (tid < nt) {
    a.csums[(size_t)j0 * C + tid] = cs;
    a.ccnt[(size_t)j0 * C + tid] = cn;
    s_cs[tid] = cs;
    s_cn[tid] = cn;
  }
  __syncthreads();
  if (tid < nj) {
    // color_pool's rule on the block's own sums
    long long tot = 0;
    int32_t totn = 0;
    for (int c = 0; c < C; c++) {
      tot += s_cs[tid * C + c];
      totn += s_cn[tid * C + c];
    }
    const double Ec = totn >= a.min_color_projections && totn > 0
                          ? (double)tot / ((double)totn * 100.0 * mcl::kColorBias) : DBL_MAX;
    a.Ec[j0 + tid] = Ec;
    a.charge[j0 + tid] = mcl::color_charge(Ec, a.color_miss, a.color_tau);
  }
}

}  // namespace mk

namespace {

mantis_status mcl_check_color(Ctx* c, const mantis_mcl_color_params* p) {
  if (!p) return mcl_fail(c, "null argument");
  if (p->struct_size != (int32_t)sizeof(mantis_mcl_color_params)) return mcl_fail(c, "color params.struct_size mismatch");
  if (p->enable < 0 || p->enable > 2) return mcl_fail(c, "color enable must be 0, 1 or 2");
  if (!(p->color_tau > 0) || !std::isfinite(p->color_tau)) return mcl_fail(c, "color_tau must be finite and > 0");
  if (!(p->color_miss >= 0) || !std::isfinite(p->color_miss)) return mcl_fail(c, "color_miss must be finite and >= 0");
  if (p->min_color_projections < 1) return mcl_fail(c, "min_color_projections must be >= 1");
  return MANTIS_OK;
}

// the colour buffers for the set's capacity (cap x 8 cameras); called by a step with colour on, before it queues anything
mantis_status mcl_color_workspace(Ctx* c) {
  Ctx::Mcl& m = c->mcl;
  if (m.color_cap >= m.cap && m.d_csums) return MANTIS_OK;
  HIP_OK(hipStreamSynchronize(c->s));  // nothing of an earlier step still reads what is freed
  m.color_cap = 0;
  const size_t n = (size_t)m.cap, tasks = n * mk::track::kMaxCams;
  if (m.d_csums.alloc(c, tasks) || m.d_ccnt.alloc(c, tasks) || m.d_Ec.alloc(c, n) || m.d_charge.alloc(c, n))
    return MANTIS_ERR_OOM;
  m.color_cap = m.cap;
  return MANTIS_OK;
}

// the step's fifth launch (between k_mcl_score and k_mcl_weight)
mantis_status mcl_color_stage(Ctx* c, const mk::MclArgs& s) {
  Ctx::Mcl& m = c->mcl;
  mk::MclColorArgs a;
  a.c2w = s.c2w;
  a.csums = m.d_csums;
  a.ccnt = m.d_ccnt;
  a.Ec = m.d_Ec;
  a.charge = m.d_charge;
  a.N = s.N;
  a.C = s.C;
  a.min_color_projections = m.color.min_color_projections;
  a.pad = 0;
  a.color_miss = m.color.color_miss;
  a.color_tau = m.color.color_tau;
  const int nb = (s.N + mk::kMclColorP - 1) / mk::kMclColorP;
  mk::k_mcl_color<<<nb, mk::kMclColorT, 0, c->s>>>(c->d_frames, lmk_of(c), a);
  HIP_OK(hipGetLastError());
  mark(c, "mcl_color/k_mcl_color");
  return MANTIS_OK;
}

}  // namespace

extern "C" {

void mantis_default_mcl_color_params(mantis_mcl_color_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(mantis_mcl_color_params);
  p->enable = 0;
  p->color_tau = MANTIS_MCL_COLOR_TAU_DEFAULT;
  p->color_miss = MANTIS_MCL_COLOR_MISS_DEFAULT;
  p->min_color_projections = 10;
}

void mantis_mcl_color_sizes(int32_t* params_bytes) {
  if (params_bytes) *params_bytes = (int32_t)sizeof(mantis_mcl_color_params);
}

mantis_status mantis_mcl_set_color(void* ctx, const mantis_mcl_color_params* p) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  if (mantis_status e = mcl_check_color(c, p)) return e;
  c->mcl.color = *p;
  c->mcl.color.pad = 0;
  return MANTIS_OK;
}

mantis_status mantis_mcl_get_color_record(void* ctx, int64_t* csums, int32_t* ccounts, double* Ec, double* charge,
                                          int32_t* n_particles, int32_t* n_cams) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  const Ctx::Mcl& m = c->mcl;
  if (!m.live || !m.has_record || m.rec_color < 1)
    return mcl_state(c, "color record: no step since the init, or the last step ran with colour off");
  const int N = m.N, C = m.rec_C;
  const size_t tasks = (size_t)N * C;
  if (n_particles) *n_particles = N;
  if (n_cams) *n_cams = C;
  if (csums) HIP_OK(hipMemcpy(csums, m.d_csums, sizeof(int64_t) * tasks, hipMemcpyDeviceToHost));
  if (ccounts) HIP_OK(hipMemcpy(ccounts, m.d_ccnt, sizeof(int32_t) * tasks, hipMemcpyDeviceToHost));
  if (Ec) HIP_OK(hipMemcpy(Ec, m.d_Ec, sizeof(double) * N, hipMemcpyDeviceToHost));
  if (charge) HIP_OK(hipMemcpy(charge, m.d_charge, sizeof(double) * N, hipMemcpyDeviceToHost));
  return MANTIS_OK;
}

mantis_status mantis_mcl_modes_color(void* ctx, double* color_error, int32_t* color_n) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return MANTIS_ERR_ARG;
  bind_device(c);
  const Ctx::Mcl& m = c->mcl;
  if (!color_error || !color_n) return mcl_fail(c, "null argument");
  if (!m.live || !m.has_record || !m.has_modes)
    return mcl_state(c, "modes_color: no mantis_mcl_modes call since the last step");
  if (m.rec_color < 1) return mcl_state(c, "modes_color: the last step ran with colour off");
  const int C = m.rec_C;
  for (int k = 0; k < mc::kMaxModes; k++) {
    color_error[k] = DBL_MAX;
    color_n[k] = 0;
    const int best = m.modes.mode[k].best;
    if (k >= m.modes.n_modes || best < 0 || best >= m.N) continue;
    long long s[mk::track::kMaxCams];
    int32_t n[mk::track::kMaxCams];
    HIP_OK(hipMemcpy(s, m.d_csums + (size_t)best * C, sizeof(long long) * C, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(n, m.d_ccnt + (size_t)best * C, sizeof(int32_t) * C, hipMemcpyDeviceToHost));
    color_error[k] = mc::color_pool(s, n, C, m.rec_color_min, &color_n[k]);
  }
  return MANTIS_OK;
}

}  // extern "C"
