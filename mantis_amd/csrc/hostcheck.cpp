// Host build of the device-logic headers (mk_*.h) for CPU unit tests only:
// lets tests/ check the per-work-item algorithms (RPP, Jenkins–Traub, the
// libstdc++ sort port, border following + approxPolyDP, and the parallel
// contour formulation) against the oracle without a GPU. The product path is
// the HIP build in libmantis_amd.so; nothing here is loaded by it.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

// runtime switch for the Jacobi noise-phase fast-forward (mk_rpp.h), so the
// tests can compare it bit for bit against the full sweep sequence
static int g_jacobi_ff = 1;
#define MK_JACOBI_FF g_jacobi_ff
#include "mk_bits.h"
#include "mk_linecal.h"
#include "mk_contour.h"
#include "mk_gn.h"
#include "mk_math.h"
#include "mk_mcl.h"
#include "mk_mcl_color.h"
#include "mk_mcl_modes.h"
#include "mk_mcl_refine.h"
#include "mk_refine.h"
#include "mk_rpp.h"
#include "mk_screen.h"
#include "mk_shard.h"
#include "mk_smooth.h"
#include "mk_sort.h"
#include "mk_track.h"

extern "C" {

void hc_set_jacobi_ff(int on) { g_jacobi_ff = on; }

int hc_rpp(const double* model, const double* iprts, double* R, double* t, double* errs, int* err_code) {
  mk::rpp::Result r = mk::rpp::solve(model, iprts);
  std::memcpy(R, r.R, sizeof(r.R));
  std::memcpy(t, r.t, sizeof(r.t));
  errs[0] = r.obj_err;
  errs[1] = r.img_err;
  errs[2] = r.iterations;
  *err_code = r.error;
  return r.status;
}

// RPP::Rpp on n points (4..12) through the per-count instances mantis_rpp_solve runs
int hc_rpp_n(const double* model, const double* iprts, int n, double* R, double* t, double* errs, int* err_code) {
  mk::rpp::Result r;
  switch (n) {
    case 4: r = mk::rpp::solve(model, iprts); break;
#define MK_HC_RPP(k) \
    case k: r = mk::rpp::n##k::solve(model, iprts); break;
    MK_RPP_INSTANCES(MK_HC_RPP)
#undef MK_HC_RPP
    default: return -100;
  }
  std::memcpy(R, r.R, sizeof(r.R));
  std::memcpy(t, r.t, sizeof(r.t));
  errs[0] = r.obj_err;
  errs[1] = r.img_err;
  errs[2] = r.iterations;
  *err_code = r.error;
  return r.status;
}

// first ObjPose (stage1a): R[9], t[3], obj_err, img_err, iterations, Q after (12)
void hc_first_objpose(const double* model, const double* iprts, double* R, double* t, double* errs, int32_t* it,
                      double* Qout) {
  mk::rpp::Stage1 s;
  mk::rpp::stage1a(model, iprts, s);
  std::memcpy(R, s.R, sizeof(s.R));
  std::memcpy(t, s.t, sizeof(s.t));
  errs[0] = s.obj_err;
  errs[1] = s.img_err;
  *it = s.iterations;
  std::memcpy(Qout, s.Q, sizeof(s.Q));
}

// stage1 (first ObjPose + Get2ndPose setup): candidate initial rotations sR (kCand x 9), keep mask, error;
// refine each kept candidate: R (kCand x 9), t (kCand x 3), errs (kCand x 2), iterations (kCand)
int hc_stage1_cands(const double* model, const double* iprts, double* sR, double* R, double* t, double* errs,
                    int32_t* its, int32_t* error) {
  mk::rpp::Stage1 s;
  mk::rpp::stage1(model, iprts, s);
  *error = s.error;
  std::memcpy(sR, s.sR, sizeof(s.sR));
  for (int j = 0; j < mk::rpp::kCand; j++) {
    its[j] = -1;
    if (s.error != 1 && ((s.keep_mask >> j) & 1)) {
      mk::rpp::Refine r;
      mk::rpp::refine(model, s.Q, s.sR[j], r);
      std::memcpy(R + 9 * j, r.R, sizeof(r.R));
      std::memcpy(t + 3 * j, r.t, sizeof(r.t));
      errs[2 * j] = r.obj_err;
      errs[2 * j + 1] = r.img_err;
      its[j] = r.iterations;
    }
  }
  return s.keep_mask;
}

// iteration counts of the phases: it[0] first ObjPose, it[1..5] candidate ObjPoses (-1 if absent)
void hc_rpp_iters(const double* model, const double* iprts, int32_t* it) {
  mk::rpp::Stage1 s;
  mk::rpp::stage1(model, iprts, s);
  it[0] = s.iterations;
  for (int j = 0; j < mk::rpp::kCand; j++) {
    it[1 + j] = -1;
    if (s.error != 1 && ((s.keep_mask >> j) & 1)) {
      mk::rpp::Refine r;
      mk::rpp::refine(model, s.Q, s.sR[j], r);
      it[1 + j] = r.iterations;
    }
  }
}

// longest-first scheduling predictor (mk_rpp.h op_predict) for the first
// ObjPose (sR == nullptr) or a candidate ObjPose from initial rotation sR
float hc_objpose_predict(const double* model, const double* iprts, const double* sR, int kprobe) {
  mk::rpp::M34 P, Q;
  for (int i = 0; i < 12; i++) { P.a[i] = model[i]; Q.a[i] = iprts[i]; }
  mk::rpp::OpState s;
  mk::rpp::M33 R0;
  if (sR)
    for (int k = 0; k < 9; k++) R0.a[k] = sR[k];
  mk::rpp::op_setup(P, Q, sR ? &R0 : nullptr, s);
  return mk::rpp::op_predict(s, kprobe);
}

// the ObjPose error sequence (new_err after each AbsKernel, first n) and its
// total AbsKernel count (predictor studies, tools/)
int hc_objpose_trace(const double* model, const double* iprts, const double* sR, int n, double* errs) {
  mk::rpp::M34 P, Q;
  for (int i = 0; i < 12; i++) { P.a[i] = model[i]; Q.a[i] = iprts[i]; }
  mk::rpp::OpState s;
  mk::rpp::M33 R0;
  if (sR)
    for (int k = 0; k < 9; k++) R0.a[k] = sR[k];
  mk::rpp::op_setup(P, Q, sR ? &R0 : nullptr, s);
  int k = 0;
  while (!mk::rpp::op_step(s)) {
    if (k < n) errs[k] = s.new_err;
    k++;
  }
  return s.it;
}

int hc_rpoly(const double* op, int deg, double* zr, double* zi) { return mk::rpp::rpoly(op, deg, zr, zi); }

void hc_sort_desc(const double* err, int n, int* perm) {
  std::vector<mk::ErrIdx> v(n);
  for (int i = 0; i < n; i++) v[i] = {err[i], i};
  mk::std_sort_desc(v.data(), v.data() + n);
  for (int i = 0; i < n; i++) perm[i] = v[i].i;
}

int hc_approx(const int32_t* pts, int n, double eps, int closed, int32_t* out, int max_dp) {
  std::vector<int32_t> dst(2 * n + 2), stack(2 * n + 2);
  int m = mk::approx_poly(pts, n, eps, closed != 0, dst.data(), stack.data(), max_dp);
  if (m > n) return m;
  std::memcpy(out, dst.data(), sizeof(int32_t) * 2 * m);
  return m;
}

// Parallel contour formulation (what the GPU kernels compute), sequential here:
// fg 8-connected / bg 4-connected labels with root = minimum padded index,
// one border per fg component (outer, start = root) and per enclosed bg
// component (hole, start = root - 1), CCOMP/LIST output order from the keys.
int hc_find_contours(const uint8_t* bin, int w, int h, int mode, int32_t* pts, int max_pts, int32_t* meta,
                     int max_c) {
  const int Wp = w + 2, Hp = h + 2;
  std::vector<uint8_t> img((size_t)Wp * Hp, 0);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) img[(size_t)(y + 1) * Wp + x + 1] = bin[(size_t)y * w + x] ? 1 : 0;
  std::vector<int> lab((size_t)Wp * Hp);
  for (size_t i = 0; i < lab.size(); i++) lab[i] = (int)i;
  auto find = [&](int x) {
    while (lab[x] != x) x = lab[x] = lab[lab[x]];
    return x;
  };
  auto unite = [&](int a, int b) {
    a = find(a); b = find(b);
    if (a == b) return;
    if (a < b) lab[b] = a; else lab[a] = b;
  };
  for (int y = 0; y < Hp; y++)
    for (int x = 0; x < Wp; x++) {
      int p = y * Wp + x;
      if (img[p]) {
        const int dx[4] = {-1, -1, 0, 1}, dy[4] = {0, -1, -1, -1};
        for (int k = 0; k < 4; k++) {
          int xx = x + dx[k], yy = y + dy[k];
          if (xx < 0 || yy < 0 || xx >= Wp) continue;
          int q = yy * Wp + xx;
          if (img[q]) unite(p, q);
        }
      } else {
        if (x > 0 && !img[p - 1]) unite(p, p - 1);
        if (y > 0 && !img[p - Wp]) unite(p, p - Wp);
      }
    }
  for (size_t i = 0; i < lab.size(); i++) lab[i] = find((int)i);
  struct B { long long key; int start; int hole; int parent; };
  std::vector<B> bs;
  for (int p = 0; p < Wp * Hp; p++) {
    if (lab[p] != p) continue;
    if (img[p]) bs.push_back({p, p, 0, p});
    else if (p != 0) bs.push_back({p, p - 1, 1, lab[p - 1]});
  }
  // CCOMP: outers by key desc, each followed by its holes by key desc; LIST: all by key desc
  std::sort(bs.begin(), bs.end(), [&](const B& a, const B& b) {
    if (mode == 2) {
      if (a.parent != b.parent) return a.parent > b.parent;
      if (a.hole != b.hole) return a.hole < b.hole;
    }
    return a.key > b.key;
  });
  if ((int)bs.size() > max_c) return -1;
  // the device tracer: packed 8-neighbourhood per step
  auto nb = [&](int x, int y) {
    auto row = [&](int yy) {
      const uint8_t* r = img.data() + (size_t)yy * Wp;
      return (uint32_t)(r[x - 1] != 0) | ((uint32_t)(r[x] != 0) << 1) | ((uint32_t)(r[x + 1] != 0) << 2);
    };
    return mk::nb8_from_rows(row(y - 1), row(y), row(y + 1));
  };
  int off = 0;
  for (size_t i = 0; i < bs.size(); i++) {
    int sx = bs[i].start % Wp, sy = bs[i].start / Wp;
    int n = mk::trace_border_nb(nb, sx, sy, bs[i].hole != 0, nullptr, 0);
    if (off + n > max_pts) return -1;
    mk::trace_border_nb(nb, sx, sy, bs[i].hole != 0, pts + 2 * off, n);
    meta[3 * i] = off;
    meta[3 * i + 1] = n;
    meta[3 * i + 2] = bs[i].hole;
    off += n;
  }
  return (int)bs.size();
}

// The bit-packed detector/mask chains (what the GPU passes compute), word by word.
void hc_masks_bits(const uint8_t* edge, int W, int H, uint8_t* det, uint8_t* mask) {
  namespace B = mk::bits;
  const int WW = B::words(W);
  std::vector<uint32_t> E((size_t)WW * H, 0), a((size_t)WW * H), b((size_t)WW * H);
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++)
      if (edge[(size_t)y * W + x]) E[(size_t)y * WW + (x >> 5)] |= 1u << (x & 31);
  auto hpass = [&](const std::vector<uint32_t>& src, std::vector<uint32_t>& dst, int r, bool dil) {
    for (int y = 0; y < H; y++)
      for (int w = 0; w < WW; w++) dst[(size_t)y * WW + w] = B::hword(src.data() + (size_t)y * WW, w, W, r, dil);
  };
  auto vpass = [&](const std::vector<uint32_t>& src, std::vector<uint32_t>& dst, int r, bool dil) {
    for (int y = 0; y < H; y++)
      for (int w = 0; w < WW; w++) dst[(size_t)y * WW + w] = B::vword(src.data(), w, y, W, H, r, dil);
  };
  auto unpack = [&](const std::vector<uint32_t>& src, uint8_t* out) {
    for (int y = 0; y < H; y++)
      for (int x = 0; x < W; x++) out[(size_t)y * W + x] = (src[(size_t)y * WW + (x >> 5)] >> (x & 31)) & 1u;
  };
  hpass(E, a, 2, true);
  vpass(a, b, 2, true);
  hpass(b, a, 1, false);
  vpass(a, b, 1, false);
  unpack(b, det);
  for (int y = 0; y < H; y++)
    for (int w = 0; w < WW; w++) a[(size_t)y * WW + w] = B::m0word(E.data(), w, y, W, H);
  for (int i = 0; i < 3; i++) {
    hpass(a, b, 3 + i, true);
    vpass(b, a, 3 + i, true);
    hpass(a, b, 3 + i, false);
    vpass(b, a, 3 + i, false);
  }
  hpass(a, b, 3, false);
  vpass(b, a, 3, false);
  unpack(a, mask);
}

void hc_distort(const double* xyz, int n, const double* K, const double* D, double* px) {
  mk::Cam cm{(double)(float)K[0], (double)(float)K[4], (double)(float)K[2], (double)(float)K[5], {D[0], D[1], D[2], D[3]}};
  for (int i = 0; i < n; i++) mk::distort(cm, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], px + 2 * i, px + 2 * i + 1);
}
void hc_undistort(const double* px, int n, const double* K, const double* D, double* out) {
  mk::Cam cm{(double)(float)K[0], (double)(float)K[4], (double)(float)K[2], (double)(float)K[5], {D[0], D[1], D[2], D[3]}};
  for (int i = 0; i < n; i++) mk::undistort(cm, px[2 * i], px[2 * i + 1], out + 2 * i, out + 2 * i + 1);
}

// screen constants (mk_screen.h screen_cam_from / screen_bounds): out = sens,
// crel, S (per unit focal length), M; returns the bound's admissibility
int hc_screen_consts(const double* K, const double* D, int pieces, double* out) {
  mk::Cam cm;
  cm.fx = (double)(float)K[0];
  cm.fy = (double)(float)K[4];
  cm.cx = (double)(float)K[2];
  cm.cy = (double)(float)K[5];
  for (int k = 0; k < 4; k++) cm.k[k] = D[k];
  const mk::ScreenCam sc = mk::screen_cam_from(cm);
  const mk::ScreenBounds b = mk::screen_bounds(cm.k, pieces);
  out[0] = sc.sens;
  out[1] = sc.crel;
  out[2] = b.S;
  out[3] = b.M;
  return b.ok ? 1 : 0;
}

// FP32 projection screen (mk_screen.h) against the exact projection on n
// (c2w, landmark) pairs: res[4 i] = screen state (0 out, 1 in, 2 unsure),
// res[4 i + 1] = exact in-frame (z > 0 and inFrame), res[4 i + 2 / + 3] = the
// screened pixel when in (else the exact pixel). Returns the number of
// screened decisions that differ from the exact ones.
int hc_screen_check(const double* c2w, const double* X, int n, const double* K, const double* D, int W, int H,
                    int32_t* res) {
  mk::Cam cm{(double)(float)K[0], (double)(float)K[4], (double)(float)K[2], (double)(float)K[5], {D[0], D[1], D[2], D[3]}};
  const mk::ScreenCam sc = mk::screen_cam_from(cm);
  int bad = 0;
  for (int i = 0; i < n; i++) {
    mk::Xf T;
    for (int k = 0; k < 12; k++) (k < 9 ? T.R[k] : T.t[k - 9]) = c2w[12 * i + k];
    double rp[3], u, v;
    mk::xf_apply(T, X + 3 * i, rp);
    mk::distort(cm, rp[0], rp[1], rp[2], &u, &v);
    const bool in = rp[2] > 0 && mk::in_frame(u, v, H, W);
    float xl[4];
    mk::screen_landmark(X + 3 * i, xl);
    int px = 0, py = 0;
    const int st = mk::screen_project(mk::posef_from(T), xl[0], xl[1], xl[2], xl[3], sc, W, H, &px, &py);
    res[4 * i] = st;
    res[4 * i + 1] = in;
    res[4 * i + 2] = st == mk::SCR_IN ? px : (in ? mk::cv_round(u) : 0);
    res[4 * i + 3] = st == mk::SCR_IN ? py : (in ? mk::cv_round(v) : 0);
    if ((st == mk::SCR_IN && (!in || px != mk::cv_round(u) || py != mk::cv_round(v))) || (st == mk::SCR_OUT && in))
      bad++;
  }
  return bad;
}

// cross-rank bookkeeping of mantis_process_rig_sharded (mk_shard.h): the
// library's own rules, for the gloo tests
int hc_sizeof_cam_result(void) { return (int)sizeof(mantis_cam_result); }
int hc_sizeof_result(void) { return (int)sizeof(mantis_result); }
int hc_sizeof_shard_rec(void) { return (int)sizeof(mk::shard::Rec); }
void hc_shard_global_indices(int n_rigs, int n_local, const int32_t* cam_index, int cams_per_rig, int32_t* gidx) {
  mk::shard::global_indices(n_rigs, n_local, cam_index, cams_per_rig, gidx);
}
void hc_shard_pack_pairs(const int32_t* gidx, const int32_t* pf, int n_local, int slots, int32_t* pairs) {
  mk::shard::pack_pairs(gidx, pf, n_local, slots, pairs);
}
int64_t hc_shard_offsets(const int32_t* pairs, int npairs, int ng, int64_t per, int32_t* flags, int64_t* offset) {
  return mk::shard::offsets_from_pairs(pairs, npairs, ng, per, flags, offset);
}
// records of n local frames padded to slots (gidx -1)
void hc_shard_make_recs(const mantis_cam_result* res, const double* Tbc, const int32_t* gidx, int n, int slots,
                        mk::shard::Rec* out) {
  for (int s = 0; s < slots; s++) {
    std::memset(&out[s], 0, sizeof(out[s]));
    out[s].gidx = -1;
    if (s < n) {
      out[s].res = res[s];
      std::memcpy(out[s].Tbc, Tbc + 16 * (size_t)s, sizeof(double) * 16);
      out[s].gidx = gidx[s];
    }
  }
}
int hc_shard_merge(const mk::shard::Rec* recv, int nrec, int ng, mantis_cam_result* all, double* Tall) {
  std::vector<int32_t> seen(ng > 0 ? ng : 1);
  return mk::shard::merge_records(recv, nrec, ng, all, Tall, seen.data());
}
void hc_rig_results(int n_rigs, int cams_per_rig, const mantis_cam_result* all, const double* Tall, const int32_t* pf,
                    const uint64_t* states, mantis_result* out) {
  mk::shard::rig_results(n_rigs, cams_per_rig, all, Tall, pf, states, out);
}

// rig GN accumulators of n_obs observations [cam, u, v, X, Y, Z] about T_w_b
// (camera c has extrinsic T_base_cam[16 c]): the same residual rows as the
// device's MFMA accumulation (mk_gn.h gn_entry), summed in row order
void hc_gn_accumulate(const double* Twb, const double* Tbc, int n_cams, const double* obs, int n_obs, double* acc28) {
  std::vector<mk::GnCam> cams(n_cams);
  for (int i = 0; i < n_cams; i++) {
    const double* a = Tbc + 16 * i;
    for (int r = 0; r < 3; r++) {
      for (int k = 0; k < 3; k++) cams[i].R_cb[3 * r + k] = a[4 * k + r];
      cams[i].t_cb[r] = -(a[r] * a[3] + a[4 + r] * a[7] + a[8 + r] * a[11]);
    }
  }
  mk::gn_accumulate_seq(Twb, cams.data(), obs, n_obs, acc28);
}

// per-quad GN after RPP (mk_gn.h quad_gn_refine) on n problems
void hc_quad_gn(int n, double* R, double* t, const double* img, const double* obj, int iters, int32_t* steps,
                double* cost0, double* cost) {
  for (int i = 0; i < n; i++)
    steps[i] = mk::quad_gn_refine(R + 9 * i, t + 3 * i, img + 8 * i, obj + 12 * i, iters, cost0 + i, cost + i);
}

// rig tracking (mk_track.h): the rules k_track_particles runs, one call each.
// sums / counts: n_particles x n_cams; err / n_proj: one entry per particle
void hc_track_pool(const int64_t* sums, const int32_t* counts, int n_particles, int n_cams, double* err,
                   int32_t* n_proj) {
  for (int j = 0; j < n_particles; j++) {
    long long s[mk::track::kMaxCams];
    for (int c = 0; c < n_cams && c < mk::track::kMaxCams; c++) s[c] = sums[(size_t)j * n_cams + c];
    err[j] = mk::track::pool(s, counts + (size_t)j * n_cams, n_cams < mk::track::kMaxCams ? n_cams : mk::track::kMaxCams,
                             &n_proj[j]);
  }
}
double hc_track_error_of(int64_t sum, int32_t n) { return mk::track::error_of((long long)sum, n); }
int hc_track_pick(const double* err, int n, double cur_err) { return mk::track::pick(err, n, cur_err); }
int hc_track_gate(double error, int32_t n_proj, int32_t min_projections, double max_error) {
  return mk::track::gate(error, n_proj, min_projections, max_error);
}
// particle = T_w_b * rand(g6) and its world -> camera pose through T_base_cam (row-major 4x4 in, 4x4 / 12 out)
void hc_track_particle(const double* T_w_b, const float* g6, double sigma_rot, double sigma_t, const double* T_base_cam,
                       double* T_out, double* c2w12) {
  const mk::Xf T = mk::track::particle(mk::track::xf_from_mat4(T_w_b), g6, sigma_rot, sigma_t);
  mk::track::xf_to_mat4(T, T_out);
  const mk::Xf v = mk::track::cam_c2w(T, mk::track::xf_from_mat4(T_base_cam));
  std::memcpy(c2w12, v.R, sizeof(double) * 9);
  std::memcpy(c2w12 + 9, v.t, sizeof(double) * 3);
}

// Monte Carlo localization (mk_mcl.h): the rules k_mcl_weight / k_mcl_resample run.
// L <- L - E / tau or -inf, then q = floor(exp(L - Lmax) 2^40); returns 1 when lost (no finite L: q = 0)
int hc_mcl_weights(const double* L, const double* E, const int32_t* n_proj, int N, double tau, int32_t min_projections,
                   double* L_out, uint64_t* q) {
  double Lmax = -INFINITY;
  for (int j = 0; j < N; j++) {
    L_out[j] = mk::mcl::log_weight(L[j], E[j], n_proj[j], min_projections, tau);
    if (L_out[j] > Lmax) Lmax = L_out[j];
  }
  for (int j = 0; j < N; j++) q[j] = Lmax > -INFINITY ? mk::mcl::weight_q(L_out[j], Lmax) : 0;
  return Lmax > -INFINITY ? 0 : 1;
}
// the inclusive integer scan, added the way the device block does: lanes of a
// wave, then waves of a round of 1024, then rounds
void hc_mcl_scan(const uint64_t* q, int N, uint64_t* cum) {
  uint64_t carry = 0;
  for (int r0 = 0; r0 < N; r0 += 1024) {
    uint64_t wt[16] = {0};
    for (int w = 0; w < 16; w++) {
      uint64_t incl = 0;
      for (int l = 0; l < 64; l++) {
        const int j = r0 + w * 64 + l;
        if (j >= N) break;
        incl += q[j];
        cum[j] = incl;  // within the wave
      }
      wt[w] = incl;
    }
    uint64_t pre = carry;
    for (int w = 0; w < 16; w++) {
      for (int l = 0; l < 64; l++) {
        const int j = r0 + w * 64 + l;
        if (j < N) cum[j] += pre;
      }
      pre += wt[w];
    }
    carry = pre;
  }
}
// ancestors of systematic resampling from the inclusive sums and the draw U
void hc_mcl_ancestors(const uint64_t* cum, const uint64_t* q, int N, uint32_t U, int32_t* anc) {
  int last = 0;
  for (int j = 0; j < N; j++)
    if (q[j] > 0) last = j;
  for (int i = 0; i < N; i++) anc[i] = mk::mcl::ancestor(cum, N, U, i, last);
}
// the exact comparison c N 2^32 > (U + i 2^32) S on its own
int hc_mcl_past(uint64_t c, int N, uint32_t U, int i, uint64_t S) { return mk::mcl::past(c, N, U, i, S) ? 1 : 0; }
uint64_t hc_mcl_rng_next(uint64_t s) { return mk::mcl::rng_next(s); }

// One step's bookkeeping on given (sum, n) inputs (mk_mcl.h step_seq): T (N x
// 16 row-major) and L in / out; flags4 = lost, resampled, n_valid, best;
// ess_err2 = ess, best_error; the estimate as T_mean16 and cov36 (zeros when
// lost); E, Lnew (the log-weights before any reset) nullable
void hc_mcl_step(const int64_t* sums, const int32_t* counts, int N, int C, double* T, double* L, double tau,
                 double resample_frac, int32_t min_projections, uint32_t U, uint64_t* q, uint64_t* cum, int32_t* anc,
                 int32_t* flags4, uint64_t* S, double* ess_err2, double* T_mean16, double* cov36, double* E,
                 double* Lnew) {
  std::vector<mk::Xf> X(N);
  std::vector<long long> s((size_t)N * C);
  for (size_t k = 0; k < s.size(); k++) s[k] = sums[k];
  for (int j = 0; j < N; j++) X[j] = mk::track::xf_from_mat4(T + 16 * (size_t)j);
  const mk::mcl::Outcome o = mk::mcl::step_seq(s.data(), counts, N, C, X.data(), L, tau, resample_frac, min_projections,
                                               U, q, cum, anc, E, Lnew);
  for (int j = 0; j < N; j++) mk::track::xf_to_mat4(X[j], T + 16 * (size_t)j);
  flags4[0] = o.lost; flags4[1] = o.resampled; flags4[2] = o.n_valid; flags4[3] = o.best;
  *S = o.S;
  ess_err2[0] = o.ess;
  ess_err2[1] = o.best_error;
  if (o.lost) {
    std::memset(T_mean16, 0, sizeof(double) * 16);
    std::memset(cov36, 0, sizeof(double) * 36);
  } else {
    mk::track::xf_to_mat4(o.mean, T_mean16);
    std::memcpy(cov36, o.cov, sizeof(double) * 36);
  }
}

// The modes of the set (mk_mcl_modes.h): the rules k_mcl_modes / k_mcl_keep run.
// key4 = ix, iy, k, bin of pose T against the anchor A (row-major 4x4 each)
void hc_mcl_cell_key(const double* T, const double* A, double g, int32_t* key4) {
  key4[3] = mk::mcl::cell_key(mk::track::xf_from_mat4(T), mk::track::xf_from_mat4(A), g, key4, key4 + 1, key4 + 2);
}
void hc_mcl_lattice_site(int s, int cx, int cy, int32_t* ixy2) { mk::mcl::lattice_site(s, cx, cy, ixy2, ixy2 + 1); }
// modes_seq on T (N x 16 row-major), q, sums / counts (N x C); out: a struct mantis_mcl_modes
void hc_mcl_modes(const double* T, const uint64_t* q, const int64_t* sums, const int32_t* counts, int N, int C, int best,
                  double g, int max_modes, void* out) {
  std::vector<mk::Xf> X(N);
  std::vector<long long> s((size_t)N * C);
  for (size_t k = 0; k < s.size(); k++) s[k] = sums[k];
  for (int j = 0; j < N; j++) X[j] = mk::track::xf_from_mat4(T + 16 * (size_t)j);
  mk::mcl::modes_seq(X.data(), q, s.data(), counts, N, C, best, g, max_modes, (mk::mcl::Modes*)out);
}

// The colour evidence (mk_mcl_color.h): the rules k_mcl_color / k_mcl_weight run.
// the window sum of a landmark at (u, v) on the raw BGR frame (W x H, stride 3 W)
int32_t hc_mcl_color_window(const uint8_t* bgr, int W, int H, double u, double v) {
  return mk::mcl::color_window_sum(bgr, W, H, u, v);
}
// (csum, cn) of n poses c2w (12 each: R row-major | t) over the ng green landmarks
void hc_mcl_color_sums(const double* c2w, int n, const double* green, int ng, const double* K, const double* D,
                       const uint8_t* bgr, int W, int H, int64_t* csum, int32_t* cn) {
  mk::Cam cm{(double)(float)K[0], (double)(float)K[4], (double)(float)K[2], (double)(float)K[5], {D[0], D[1], D[2], D[3]}};
  for (int i = 0; i < n; i++) {
    mk::Xf T;
    for (int k = 0; k < 12; k++) (k < 9 ? T.R[k] : T.t[k - 9]) = c2w[12 * i + k];
    long long s;
    mk::mcl::color_sums(T, green, ng, cm, bgr, W, H, &s, &cn[i]);
    csum[i] = s;
  }
}
// pooled Ec (DBL_MAX where undefined), the pooled count and the charge of N particles from csums / cns (N x C)
void hc_mcl_color_charge(const int64_t* csums, const int32_t* cns, int N, int C, int32_t min_color_projections,
                         double color_miss, double color_tau, double* Ec, int32_t* n_out, double* charge) {
  std::vector<long long> s(C > 0 ? C : 1);
  for (int j = 0; j < N; j++) {
    for (int c = 0; c < C; c++) s[c] = csums[(size_t)j * C + c];
    Ec[j] = mk::mcl::color_pool(s.data(), cns + (size_t)j * C, C, min_color_projections, &n_out[j]);
    charge[j] = mk::mcl::color_charge(Ec[j], color_miss, color_tau);
  }
}
// L <- (L - E / tau) - charge or -inf
void hc_mcl_color_fold(const double* L, const double* E, const int32_t* n_proj, const double* charge, int N, double tau,
                       int32_t min_projections, double* L_out) {
  for (int j = 0; j < N; j++)
    L_out[j] = mk::mcl::log_weight_color(L[j], E[j], n_proj[j], min_projections, tau, charge[j]);
}

// Line refinement (mk_refine.h): the rules k_refine_obs / k_refine_step run.
void hc_refine_flags(const double* X, int n, double pitch, uint8_t* flags) { mk::refine::line_flags(X, n, pitch, flags); }
static mk::Cam hc_cam(const double* K, const double* D) {
  return mk::Cam{(double)(float)K[0], (double)(float)K[4], (double)(float)K[2], (double)(float)K[5], {D[0], D[1], D[2], D[3]}};
}
// one pass for one camera (extrinsic T_base_cam) at base pose Twb over the
// candidates of `flags`: per candidate the code, Sw, Skw, the 7 row doubles and
// the tie-near flag (nullable); bgr: W x H, stride 3 W. Returns n_cand.
int hc_refine_obs(const double* Twb, const double* Tbc, const double* K, const double* D, const uint8_t* bgr, int W,
                  int H, const double* X, int nw, int nr, int ng, const uint8_t* flags, int R, int white_thresh,
                  int min_weight, int32_t* codes, int32_t* Sw, int32_t* Skw, double* rows, int32_t* tie) {
  namespace rf = mk::refine;
  const int n = nw + nr + ng;
  std::vector<int32_t> cand(n > 0 ? n : 1);
  const int nc = rf::candidates(flags, n, cand.data());
  mk::GnCam gc;
  rf::gncam_from(Tbc, gc);
  const mk::Cam cm = hc_cam(K, D);
  double Rt[9], t[3];
  rf::pose_parts(Twb, Rt, t);
  const rf::Window win{R, white_thresh, min_weight, 0};
  for (int k = 0; k < nc; k++) {
    const int i = cand[k] & 0xffff, axis = cand[k] >> 16;
    int tg[3], near = 0;
    rf::target_bgr(i, nw, nr, tg);
    rf::Slot o;
    rf::observe(Rt, t, gc, cm, bgr, W, H, X + 3 * i, axis, tg, win, o, &near);
    codes[k] = o.code;
    Sw[k] = o.Sw;
    Skw[k] = o.Skw;
    std::memcpy(rows + 7 * k, o.row, sizeof(o.row));
    if (tie) tie[k] = near;
  }
  return nc;
}
// acc28 of n rows of 7 doubles, summed in row order
void hc_refine_accumulate(const double* rows, int n, double* acc28) {
  for (int e = 0; e < 28; e++) acc28[e] = 0.0;
  for (int k = 0; k < n; k++) mk::refine::accumulate_row(rows + 7 * k, acc28);
}
// the whole iteration of one rig of C cameras (Tbc C x 16, K C x 9, D C x 4,
// frames: C pointers to W x H frames of stride 3 W), rows summed in slot order
void hc_refine_seq(const double* T_in, const double* Tbc, const double* K, const double* D, const uint8_t* const* frames,
                   int C, int W, int H, const double* X, int nw, int nr, int ng, const mantis_refine_params* p,
                   mantis_refine_result* out) {
  namespace rf = mk::refine;
  const int n = nw + nr + ng;
  std::vector<uint8_t> flags(n > 0 ? n : 1);
  rf::line_flags(X, n, p->landmark_pitch, flags.data());
  std::vector<int32_t> cand(n > 0 ? n : 1);
  const int nc = rf::candidates(flags.data(), n, cand.data());
  std::vector<mk::GnCam> gc(C);
  std::vector<mk::Cam> cm(C);
  for (int c = 0; c < C; c++) {
    rf::gncam_from(Tbc + 16 * c, gc[c]);
    cm[c] = hc_cam(K + 9 * c, D + 4 * c);
  }
  rf::refine_seq(T_in, gc.data(), cm.data(), frames, C, W, H, X, nw, nr, cand.data(), nc, *p, *out, nullptr);
}
// gn_solve6 on its own (the step of a pass): returns 1 when solved
int hc_gn_solve6(const double* acc28, double lambda, double* T, double* d6) { return mk::gn_solve6(acc28, lambda, T, d6) ? 1 : 0; }
// the gate and the covariance (refine::conclude) of a result record with the last pass's acc28
void hc_refine_conclude(const double* acc28, int min_obs, double max_rms, mantis_refine_result* R) {
  mk::refine::conclude(acc28, min_obs, max_rms, *R);
}
int hc_sizeof_refine_params(void) { return (int)sizeof(mantis_refine_params); }
int hc_sizeof_refine_result(void) { return (int)sizeof(mantis_refine_result); }

// The robust rows (mk_refine.h robust_*): the rules k_refine_step_robust runs.
uint32_t hc_refine_robust_key(int32_t Sw, int32_t Skw) { return mk::refine::robust_key(Sw, Skw); }
// keys (n; codes nullable = every slot is a row) to the lower median, the scale, the weights (n, 0
// in rejected slots) and counts (4: n_obs, n_down, n_zero, n with w > 0); sum_w in slot order
void hc_refine_robust_weights(const uint32_t* keys, const int32_t* codes, int n, int loss, double tuning,
                              double scale_floor, double* weights, uint32_t* median_key, double* scale, int32_t* counts,
                              double* sum_w) {
  mk::refine::RobustPass P;
  mk::refine::robust_weights(keys, codes, n, mk::refine::Robust{loss, 0, tuning, scale_floor}, weights, P);
  *median_key = P.median_key;
  *scale = P.scale;
  counts[0] = P.n_obs;
  counts[1] = P.n_down;
  counts[2] = P.n_zero;
  counts[3] = P.n_obs - P.n_zero;
  *sum_w = P.sum_w;
}
// hc_refine_seq with the robust rows of rb (null or loss 0: hc_refine_seq's bytes); stats nullable
void hc_refine_seq_robust(const double* T_in, const double* Tbc, const double* K, const double* D,
                          const uint8_t* const* frames, int C, int W, int H, const double* X, int nw, int nr, int ng,
                          const mantis_refine_params* p, const mantis_refine_robust_params* rb,
                          mantis_refine_result* out, mantis_refine_robust_stats* stats) {
  namespace rf = mk::refine;
  const int n = nw + nr + ng;
  std::vector<uint8_t> flags(n > 0 ? n : 1);
  rf::line_flags(X, n, p->landmark_pitch, flags.data());
  std::vector<int32_t> cand(n > 0 ? n : 1);
  const int nc = rf::candidates(flags.data(), n, cand.data());
  std::vector<mk::GnCam> gc(C);
  std::vector<mk::Cam> cm(C);
  for (int c = 0; c < C; c++) {
    rf::gncam_from(Tbc + 16 * c, gc[c]);
    cm[c] = hc_cam(K + 9 * c, D + 4 * c);
  }
  const rf::Robust r = rb ? rf::Robust{rb->loss, 0, rb->tuning, rb->scale_floor} : rf::Robust{0, 0, 1.0, 1.0};
  rf::refine_seq_robust(T_in, gc.data(), cm.data(), frames, C, W, H, X, nw, nr, cand.data(), nc, *p, r, *out, stats);
}
// one step of a pass with the starved gate of the robust rows: returns 1 when the rig is finished
int hc_refine_end_pass_robust(const double* acc28, int n_obs, int n_pos, int pass, int I, int min_obs, double lambda,
                              mantis_refine_result* R) {
  return mk::refine::end_pass_robust(acc28, n_obs, n_pos, pass, I, min_obs, lambda, *R) ? 1 : 0;
}
int hc_sizeof_refine_robust_params(void) { return (int)sizeof(mantis_refine_robust_params); }
int hc_sizeof_refine_robust_stats(void) { return (int)sizeof(mantis_refine_robust_stats); }

// The three calibrations (mk_linecal.h): the rules k_linecal_obs / k_linecal_rig / k_linecal_solve run,
// at the problem P (linecal::Ext / Int / Rig). The hc_calib_* and hc_icalib_* entries take the public
// structs of the single calibrations and widen / narrow them around the shared rules.
extern "C++" {
namespace {
namespace lc = mk::linecal;

// hc_refine_obs at the intrinsics cm with rows of P::kRow ([J_pose | J_ext | J_int | r]; J_ext zeros unless
// free_ext, J_int zeros unless free_int, a zero for a parameter outside param_mask)
template <class P>
int lc_obs(const double* Twb, const double* Tbc, const mk::Cam& cm, const uint8_t* bgr, int W, int H, const double* X,
           int nw, int nr, int ng, const uint8_t* flags, int R, int white_thresh, int min_weight, int free_ext,
           int free_int, int param_mask, int32_t* codes, int32_t* Sw, int32_t* Skw, double* rows, int32_t* tie) {
  namespace rf = mk::refine;
  const int n = nw + nr + ng;
  std::vector<int32_t> cand(n > 0 ? n : 1);
  const int nc = rf::candidates(flags, n, cand.data());
  mk::GnCam gc;
  rf::gncam_from(Tbc, gc);
  double Rt[9], t[3];
  rf::pose_parts(Twb, Rt, t);
  const rf::Window win{R, white_thresh, min_weight, 0};
  for (int k = 0; k < nc; k++) {
    const int i = cand[k] & 0xffff, axis = cand[k] >> 16;
    int tg[3], near = 0;
    rf::target_bgr(i, nw, nr, tg);
    typename P::Slot o;
    P::observe(Rt, t, gc, cm, bgr, W, H, X + 3 * i, axis, tg, win, free_ext != 0, free_int != 0, (uint32_t)param_mask, o,
               &near);
    codes[k] = o.code;
    Sw[k] = o.Sw;
    Skw[k] = o.Skw;
    std::memcpy(rows + P::kRow * k, o.row, sizeof(o.row));
    if (tie) tie[k] = near;
  }
  return nc;
}
// the accumulator of n rows of P::kRow doubles, summed in row order
template <class P>
void lc_accumulate(const double* rows, int n, double* acc) {
  for (int e = 0; e < P::kAcc; e++) acc[e] = 0.0;
  for (int k = 0; k < n; k++) P::accumulate_row(rows + P::kRow * k, acc);
}
// the whole call on the host: N views of C cameras (Tbc C x 16, K C x 9 rounded to float as the
// library does, D C x 4, frames: N x C pointers to W x H frames of stride 3 W), rows summed in slot order
template <class P>
void lc_seq(const double* T_in, const double* Tbc, const double* K, const double* D, const uint8_t* const* frames, int N,
            int C, int W, int H, const double* X, int nw, int nr, int ng, const mantis_refine_params* p, uint32_t fe,
            uint32_t fi, uint32_t pm, int32_t min_obs_cam, double* T_out, mantis_rcalib_result* out,
            const mantis_refine_robust_params* rb = nullptr, mantis_calib_robust_stats* stats = nullptr) {
  namespace rf = mk::refine;
  const int n = nw + nr + ng;
  std::vector<uint8_t> flags(n > 0 ? n : 1);
  rf::line_flags(X, n, p->landmark_pitch, flags.data());
  std::vector<int32_t> cand(n > 0 ? n : 1);
  const int nc = rf::candidates(flags.data(), n, cand.data());
  std::vector<mk::Cam> cm(C);
  for (int c = 0; c < C; c++) cm[c] = hc_cam(K + 9 * c, D + 4 * c);
  const rf::Robust r = rb ? rf::Robust{rb->loss, 0, rb->tuning, rb->scale_floor} : rf::Robust{0, 0, 1.0, 1.0};
  P::seq(T_in, Tbc, cm.data(), frames, N, C, W, H, X, nw, nr, cand.data(), nc, *p, fe, fi, pm, min_obs_cam, T_out, *out,
         nullptr, &r, stats);
}
}  // namespace
}  // extern "C++"

// Extrinsic calibration: rows of 13, acc91; K, D as hc_refine_obs takes them
int hc_calib_obs(const double* Twb, const double* Tbc, const double* K, const double* D, const uint8_t* bgr, int W,
                 int H, const double* X, int nw, int nr, int ng, const uint8_t* flags, int R, int white_thresh,
                 int min_weight, int free_cam, int32_t* codes, int32_t* Sw, int32_t* Skw, double* rows, int32_t* tie) {
  return lc_obs<lc::Ext>(Twb, Tbc, hc_cam(K, D), bgr, W, H, X, nw, nr, ng, flags, R, white_thresh, min_weight, free_cam,
                         0, 0, codes, Sw, Skw, rows, tie);
}
void hc_calib_accumulate(const double* rows, int n, double* acc91) { lc_accumulate<lc::Ext>(rows, n, acc91); }
// the end of a pass from given accumulators (N x C x 91) and counts (N x C): T (N x 16, in / out),
// R->T_base_cam (in / out), delta (N x 6, nullable). Returns 1 when the call is finished.
int hc_calib_end_pass(const double* acc91, const int32_t* cnt, int N, int C, int free_cams, int pass, int I, int min_obs,
                      int min_obs_cam, double lambda, double* T, mantis_calib_result* R, double* delta) {
  return lc::with_state(*R, [&](mantis_rcalib_result& w) {
    return lc::Ext::end_pass(acc91, cnt, N, C, (uint32_t)free_cams, 0u, 0u, pass, I, min_obs, min_obs_cam, lambda, T, w,
                             delta) ? 1 : 0;
  });
}
void hc_calib_seq(const double* T_in, const double* Tbc, const double* K, const double* D, const uint8_t* const* frames,
                  int N, int C, int W, int H, const double* X, int nw, int nr, int ng, const mantis_refine_params* p,
                  const mantis_calib_params* cp, double* T_out, mantis_calib_result* out) {
  mantis_rcalib_result w;
  lc_seq<lc::Ext>(T_in, Tbc, K, D, frames, N, C, W, H, X, nw, nr, ng, p, (uint32_t)cp->free_cams, 0u, 0u,
                  cp->min_obs_cam, T_out, &w);
  lc::narrow(w, *out);
}
// the gate, rms_cam and the covariances (conclude) of a result record with the last pass's acc91 / counts
void hc_calib_conclude(const double* acc91, const int32_t* cnt, int N, int C, int free_cams, int min_obs,
                       int min_obs_cam, double max_rms, mantis_calib_result* R) {
  lc::with_state(*R, [&](mantis_rcalib_result& w) {
    lc::Ext::conclude(acc91, cnt, N, C, (uint32_t)free_cams, 0u, 0u, min_obs, min_obs_cam, max_rms, w);
  });
}
int hc_sizeof_calib_params(void) { return (int)sizeof(mantis_calib_params); }
int hc_sizeof_calib_result(void) { return (int)sizeof(mantis_calib_result); }

// Intrinsic calibration: rows of 15, acc120, at the FP64 intrinsics KD (fx, fy, cx, cy, k1..k4, taken as given)
int hc_icalib_obs(const double* Twb, const double* Tbc, const double* KD, const uint8_t* bgr, int W, int H,
                  const double* X, int nw, int nr, int ng, const uint8_t* flags, int R, int white_thresh, int min_weight,
                  int free_cam, int param_mask, int32_t* codes, int32_t* Sw, int32_t* Skw, double* rows, int32_t* tie) {
  return lc_obs<lc::Int>(Twb, Tbc, mk::icalib::cam_of(KD, KD + 4), bgr, W, H, X, nw, nr, ng, flags, R, white_thresh,
                         min_weight, 0, free_cam, param_mask, codes, Sw, Skw, rows, tie);
}
void hc_icalib_accumulate(const double* rows, int n, double* acc120) { lc_accumulate<lc::Int>(rows, n, acc120); }
// as hc_calib_end_pass, with R->K / R->D (in / out)
int hc_icalib_end_pass(const double* acc120, const int32_t* cnt, int N, int C, int free_cams, int param_mask, int pass,
                       int I, int min_obs, int min_obs_cam, double lambda, double* T, mantis_icalib_result* R,
                       double* delta) {
  return lc::with_state(*R, [&](mantis_rcalib_result& w) {
    return lc::Int::end_pass(acc120, cnt, N, C, 0u, (uint32_t)free_cams, (uint32_t)param_mask, pass, I, min_obs,
                             min_obs_cam, lambda, T, w, delta) ? 1 : 0;
  });
}
void hc_icalib_seq(const double* T_in, const double* Tbc, const double* K, const double* D, const uint8_t* const* frames,
                   int N, int C, int W, int H, const double* X, int nw, int nr, int ng, const mantis_refine_params* p,
                   const mantis_icalib_params* ip, double* T_out, mantis_icalib_result* out) {
  mantis_rcalib_result w;
  lc_seq<lc::Int>(T_in, Tbc, K, D, frames, N, C, W, H, X, nw, nr, ng, p, 0u, (uint32_t)ip->free_cams,
                  (uint32_t)ip->param_mask, ip->min_obs_cam, T_out, &w);
  lc::narrow(w, *out);
}
void hc_icalib_conclude(const double* acc120, const int32_t* cnt, int N, int C, int free_cams, int param_mask,
                        int min_obs, int min_obs_cam, double max_rms, mantis_icalib_result* R) {
  lc::with_state(*R, [&](mantis_rcalib_result& w) {
    lc::Int::conclude(acc120, cnt, N, C, 0u, (uint32_t)free_cams, (uint32_t)param_mask, min_obs, min_obs_cam, max_rms, w);
  });
}
int hc_sizeof_icalib_params(void) { return (int)sizeof(mantis_icalib_params); }
int hc_sizeof_icalib_result(void) { return (int)sizeof(mantis_icalib_result); }

// Rig calibration: rows of 21, acc231; R->T_base_cam, R->K / R->D (in / out)
int hc_rcalib_obs(const double* Twb, const double* Tbc, const double* KD, const uint8_t* bgr, int W, int H,
                  const double* X, int nw, int nr, int ng, const uint8_t* flags, int R, int white_thresh, int min_weight,
                  int free_ext, int free_int, int param_mask, int32_t* codes, int32_t* Sw, int32_t* Skw, double* rows,
                  int32_t* tie) {
  return lc_obs<lc::Rig>(Twb, Tbc, mk::icalib::cam_of(KD, KD + 4), bgr, W, H, X, nw, nr, ng, flags, R, white_thresh,
                         min_weight, free_ext, free_int, param_mask, codes, Sw, Skw, rows, tie);
}
void hc_rcalib_accumulate(const double* rows, int n, double* acc231) { lc_accumulate<lc::Rig>(rows, n, acc231); }
int hc_rcalib_end_pass(const double* acc231, const int32_t* cnt, int N, int C, int free_ext, int free_int,
                       int param_mask, int pass, int I, int min_obs, int min_obs_cam, double lambda, double* T,
                       mantis_rcalib_result* R, double* delta) {
  return lc::Rig::end_pass(acc231, cnt, N, C, (uint32_t)free_ext, (uint32_t)free_int, (uint32_t)param_mask, pass, I,
                           min_obs, min_obs_cam, lambda, T, *R, delta)
             ? 1 : 0;
}
void hc_rcalib_seq(const double* T_in, const double* Tbc, const double* K, const double* D, const uint8_t* const* frames,
                   int N, int C, int W, int H, const double* X, int nw, int nr, int ng, const mantis_refine_params* p,
                   const mantis_rcalib_params* rp, double* T_out, mantis_rcalib_result* out) {
  lc_seq<lc::Rig>(T_in, Tbc, K, D, frames, N, C, W, H, X, nw, nr, ng, p, (uint32_t)rp->free_ext, (uint32_t)rp->free_int,
                  (uint32_t)rp->param_mask, rp->min_obs_cam, T_out, out);
}
void hc_rcalib_conclude(const double* acc231, const int32_t* cnt, int N, int C, int free_ext, int free_int,
                        int param_mask, int min_obs, int min_obs_cam, double max_rms, mantis_rcalib_result* R) {
  lc::Rig::conclude(acc231, cnt, N, C, (uint32_t)free_ext, (uint32_t)free_int, (uint32_t)param_mask, min_obs,
                    min_obs_cam, max_rms, *R);
}
int hc_sizeof_rcalib_params(void) { return (int)sizeof(mantis_rcalib_params); }
int hc_sizeof_rcalib_result(void) { return (int)sizeof(mantis_rcalib_result); }

// The calibrations' robust rows (mk_linecal.h robust_*): the rules k_linecal_hist and the robust
// instantiations of k_linecal_rig / k_linecal_solve run. One pass over all N x C x n_cand slots
// (view-major): keys and weights (0 in rejected slots), the call-wide lower median and scale,
// counts (4: n_obs, n_down, n_zero, n with w > 0), sum_w in slot order, and per (view, camera)
// cell_counts (N x C x 2: n_down, n_zero) and cell_sum_w (N x C)
void hc_linecal_robust_weights(const int32_t* codes, const int32_t* Sw, const int32_t* Skw, int N, int C, int n_cand,
                               int loss, double tuning, double scale_floor, uint32_t* keys, double* weights,
                               uint32_t* median_key, double* scale, int32_t* counts, double* sum_w,
                               int32_t* cell_counts, double* cell_sum_w) {
  mk::refine::RobustPass P;
  std::vector<lc::RobustCell> cells((size_t)N * C);
  lc::robust_pass(codes, Sw, Skw, N, C, n_cand, mk::refine::Robust{loss, 0, tuning, scale_floor}, keys, weights,
                  cells.data(), P);
  *median_key = P.median_key;
  *scale = P.scale;
  counts[0] = P.n_obs;
  counts[1] = P.n_down;
  counts[2] = P.n_zero;
  counts[3] = P.n_obs - P.n_zero;
  *sum_w = P.sum_w;
  for (int f = 0; f < N * C; f++) {
    cell_counts[2 * f] = cells[f].n_down;
    cell_counts[2 * f + 1] = cells[f].n_zero;
    cell_sum_w[f] = cells[f].sum_w;
  }
}
// the stats of a pass from its cells (as hc_linecal_robust_weights lays them out) and counts
void hc_linecal_robust_tally(const int32_t* cell_counts, const double* cell_sum_w, const int32_t* cnt, int N, int C,
                             int pass, uint32_t median_key, double sigma, mantis_calib_robust_stats* stats) {
  std::vector<lc::RobustCell> cells((size_t)N * C);
  for (int f = 0; f < N * C; f++) cells[f] = lc::RobustCell{cell_counts[2 * f], cell_counts[2 * f + 1], cell_sum_w[f]};
  lc::robust_tally(cells.data(), cnt, N, C, pass, median_key, sigma, *stats);
}
// hc_*_seq with the robust rows of rb (null or loss 0: hc_*_seq's bytes); stats nullable
void hc_calib_seq_robust(const double* T_in, const double* Tbc, const double* K, const double* D,
                         const uint8_t* const* frames, int N, int C, int W, int H, const double* X, int nw, int nr,
                         int ng, const mantis_refine_params* p, const mantis_calib_params* cp,
                         const mantis_refine_robust_params* rb, double* T_out, mantis_calib_result* out,
                         mantis_calib_robust_stats* stats) {
  mantis_rcalib_result w;
  lc_seq<lc::Ext>(T_in, Tbc, K, D, frames, N, C, W, H, X, nw, nr, ng, p, (uint32_t)cp->free_cams, 0u, 0u,
                  cp->min_obs_cam, T_out, &w, rb, stats);
  lc::narrow(w, *out);
}
void hc_icalib_seq_robust(const double* T_in, const double* Tbc, const double* K, const double* D,
                          const uint8_t* const* frames, int N, int C, int W, int H, const double* X, int nw, int nr,
                          int ng, const mantis_refine_params* p, const mantis_icalib_params* ip,
                          const mantis_refine_robust_params* rb, double* T_out, mantis_icalib_result* out,
                          mantis_calib_robust_stats* stats) {
  mantis_rcalib_result w;
  lc_seq<lc::Int>(T_in, Tbc, K, D, frames, N, C, W, H, X, nw, nr, ng, p, 0u, (uint32_t)ip->free_cams,
                  (uint32_t)ip->param_mask, ip->min_obs_cam, T_out, &w, rb, stats);
  lc::narrow(w, *out);
}
void hc_rcalib_seq_robust(const double* T_in, const double* Tbc, const double* K, const double* D,
                          const uint8_t* const* frames, int N, int C, int W, int H, const double* X, int nw, int nr,
                          int ng, const mantis_refine_params* p, const mantis_rcalib_params* rp,
                          const mantis_refine_robust_params* rb, double* T_out, mantis_rcalib_result* out,
                          mantis_calib_robust_stats* stats) {
  lc_seq<lc::Rig>(T_in, Tbc, K, D, frames, N, C, W, H, X, nw, nr, ng, p, (uint32_t)rp->free_ext, (uint32_t)rp->free_int,
                  (uint32_t)rp->param_mask, rp->min_obs_cam, T_out, out, rb, stats);
}
// hc_*_end_pass with the robust rows' two starved gates: pos (N x C) = the rows with w > 0
int hc_calib_end_pass_robust(const double* acc91, const int32_t* cnt, const int32_t* pos, int N, int C, int free_cams,
                             int pass, int I, int min_obs, int min_obs_cam, double lambda, double* T,
                             mantis_calib_result* R, double* delta) {
  return lc::with_state(*R, [&](mantis_rcalib_result& w) {
    return lc::Ext::end_pass(acc91, cnt, N, C, (uint32_t)free_cams, 0u, 0u, pass, I, min_obs, min_obs_cam, lambda, T, w,
                             delta, pos) ? 1 : 0;
  });
}
int hc_icalib_end_pass_robust(const double* acc120, const int32_t* cnt, const int32_t* pos, int N, int C, int free_cams,
                              int param_mask, int pass, int I, int min_obs, int min_obs_cam, double lambda, double* T,
                              mantis_icalib_result* R, double* delta) {
  return lc::with_state(*R, [&](mantis_rcalib_result& w) {
    return lc::Int::end_pass(acc120, cnt, N, C, 0u, (uint32_t)free_cams, (uint32_t)param_mask, pass, I, min_obs,
                             min_obs_cam, lambda, T, w, delta, pos) ? 1 : 0;
  });
}
int hc_rcalib_end_pass_robust(const double* acc231, const int32_t* cnt, const int32_t* pos, int N, int C, int free_ext,
                              int free_int, int param_mask, int pass, int I, int min_obs, int min_obs_cam,
                              double lambda, double* T, mantis_rcalib_result* R, double* delta) {
  return lc::Rig::end_pass(acc231, cnt, N, C, (uint32_t)free_ext, (uint32_t)free_int, (uint32_t)param_mask, pass, I,
                           min_obs, min_obs_cam, lambda, T, *R, delta, pos)
             ? 1 : 0;
}
int hc_sizeof_calib_robust_stats(void) { return (int)sizeof(mantis_calib_robust_stats); }

// The modes refined (mk_mcl_refine.h): the rules mantis_mcl_refine_modes and k_mcl_recentre run.
// modes: a struct mantis_mcl_modes; T_ref 8 x 16 (row-major), refined 8; out: key_kept / applied (8
// each), X 8 x 16 (the corrections; the identity past n_modes), bins 8 (-1: not applied)
void hc_mcl_refine_plan(const void* modes, double g, const double* T_ref, const int32_t* refined, int apply,
                        int32_t* key_kept, int32_t* applied, double* X, int32_t* bins) {
  mk::mcl::Recentre P;
  mk::mcl::refine_plan(*(const mk::mcl::Modes*)modes, g, T_ref, refined, apply, key_kept, applied, &P);
  for (int k = 0; k < mk::mcl::kMaxModes; k++) {
    mk::track::xf_to_mat4(P.X[k], X + 16 * k);
    bins[k] = P.bin[k];
  }
}
// the plan of (modes, T_ref, refined, apply) applied to the set T (N x 16 row-major, in / out); n_moved 8
void hc_mcl_recentre(const void* modes, double g, const double* T_ref, const int32_t* refined, int apply, double* T,
                     int N, int32_t* n_moved) {
  mk::mcl::Recentre P;
  int32_t kept[mk::mcl::kMaxModes], applied[mk::mcl::kMaxModes];
  mk::mcl::refine_plan(*(const mk::mcl::Modes*)modes, g, T_ref, refined, apply, kept, applied, &P);
  for (int k = 0; k < mk::mcl::kMaxModes; k++) n_moved[k] = 0;
  for (int j = 0; j < N; j++) {
    mk::Xf X = mk::track::xf_from_mat4(T + 16 * (size_t)j);
    const int32_t hit = mk::mcl::recentre_pose(P, X);
    if (hit < 0) continue;  // keeps its bits
    n_moved[hit]++;
    mk::track::xf_to_mat4(X, T + 16 * (size_t)j);
  }
}

// Window smoothing (mk_smooth.h): the rules k_smooth_solve and the host's conclude run.
// the motion's Transform as mantis_track forms it; returns 0 (and leaves D) when the motion is unset
int hc_smooth_motion(const double* pos3, const double* quat4, double* D) {
  if (!(quat4[0] * quat4[0] + quat4[1] * quat4[1] + quat4[2] * quat4[2] + quat4[3] * quat4[3] >= 0.5)) return 0;
  mk::shard::quat_to_mat4(quat4, pos3, D);
  return 1;
}
void hc_smooth_log(const double* R9, double* phi) { mk::smooth::log_so3(R9, phi); }
void hc_smooth_jr_inv(const double* phi, double* J9) { mk::smooth::jr_inv(phi, J9); }
void hc_smooth_between(const double* Tk, const double* Tk1, const double* D, double wt, double wr, double* e, double* Ja,
                       double* Jb) {
  mk::smooth::between(Tk, Tk1, D, wt, wr, e, Ja, Jb);
}
// the prior factor whitened by sigma_row L_c^-1 of cov (36); returns 0 when cov is not finite or not PD
int hc_smooth_prior(const double* T0, const double* Tp, const double* cov, double sigma_row, double* e, double* J) {
  double Wp[36];
  if (!mk::smooth::prior_whitener(cov, sigma_row, Wp)) return 0;
  mk::smooth::prior(T0, Tp, Wp, e, J);
  return 1;
}
// the blocks of every view of a window from its accumulators (N x 28) and whitened factors
void hc_smooth_assemble(int N, const double* acc28, const int32_t* has, const double* fe, const double* fJ, int has_prior,
                        const double* pe, const double* pJ, double lambda, double* Hd, double* Ho, double* g) {
  for (int k = 0; k < N; k++)
    mk::smooth::assemble(k, N, acc28 + 28 * (size_t)k, has, fe, fJ, has_prior, pe, pJ, lambda, Hd + 36 * (size_t)k,
                         Ho + 36 * (size_t)k, g + 6 * (size_t)k);
}
// blocks -> x = -H^-1 g (N x 6), with the factor (Ld, Lo: N x 36); -1, or the first view whose block is not PD
int hc_smooth_solve(int N, const double* Hd, const double* Ho, const double* g, const int32_t* has, double* x, double* Ld,
                    double* Lo) {
  return mk::smooth::solve(N, Hd, Ho, g, has, Ld, Lo, x);
}
// the diagonal blocks of H^-1 (N x 36); -1, or the first view whose block is not PD
int hc_smooth_marginals(int N, const double* Hd, const double* Ho, const int32_t* has, double* S) {
  std::vector<double> Ld(36 * (size_t)N), Lo(36 * (size_t)N), x(6 * (size_t)N), g(6 * (size_t)N, 0.0);
  const int bad = mk::smooth::solve(N, Hd, Ho, g.data(), has, Ld.data(), Lo.data(), x.data());
  if (bad >= 0) return bad;
  mk::smooth::marginals(N, Ld.data(), Lo.data(), has, S);
  return -1;
}
// the figures of a pass: out = [rms, motion_rms, cost], counts = [n_obs, n_factors]
void hc_smooth_sums(int N, const int32_t* n_obs, const double* acc28, const int32_t* has, const double* fe, int has_prior,
                    const double* pe, double sigma_row, double* out3, int32_t* counts2) {
  int32_t n = 0;
  double rtr = 0;
  for (int k = 0; k < N; k++) {
    n += n_obs[k];
    rtr += acc28[28 * (size_t)k + 27];
  }
  mk::smooth::Sums S;
  mk::smooth::window_sums(N, n, rtr, has, fe, has_prior, pe, sigma_row, S);
  out3[0] = S.rms;
  out3[1] = S.motion_rms;
  out3[2] = S.cost;
  counts2[0] = S.n_obs;
  counts2[1] = S.n_factors;
}
void hc_smooth_conclude(int N, const double* Hd, const double* Ho, const int32_t* has, int min_obs, double max_rms,
                        mantis_smooth_result* R, mantis_smooth_view* V) {
  mk::smooth::conclude(N, Hd, Ho, has, min_obs, max_rms, *R, V);
}
// The whole call of one window on host frames (frames: N x C pointers to W x H frames of stride
// 3 W; motions: (N - 1) x 7 = delta_pos | delta_quat; prior_T / prior_cov nullable). The record
// pointers (each nullable) get every pass taken: recT [pass][N][16], recAcc [pass][N][28], recN
// [pass][N], recE [pass][N - 1][6], recJ [pass][N - 1][72], recPe [pass][6], recPJ [pass][36],
// recDelta [pass][N][6]. Returns 0 when the prior covariance is refused.
int hc_smooth_seq(int N, const double* T_in, const double* motions, const double* prior_T, const double* prior_cov,
                  const double* Tbc, const double* K, const double* D, const uint8_t* const* frames, int C, int W, int H,
                  const double* X, int nw, int nr, int ng, const mantis_smooth_params* p, mantis_smooth_result* out,
                  mantis_smooth_view* views, double* recT, double* recAcc, int32_t* recN, double* recE, double* recJ,
                  double* recPe, double* recPJ, double* recDelta) {
  namespace rf = mk::refine;
  namespace sm = mk::smooth;
  const int n = nw + nr + ng;
  std::vector<uint8_t> flags(n > 0 ? n : 1);
  rf::line_flags(X, n, p->landmark_pitch, flags.data());
  std::vector<int32_t> cand(n > 0 ? n : 1);
  const int nc = rf::candidates(flags.data(), n, cand.data());
  std::vector<mk::GnCam> gc(C);
  std::vector<mk::Cam> cm(C);
  for (int c = 0; c < C; c++) {
    rf::gncam_from(Tbc + 16 * c, gc[c]);
    cm[c] = hc_cam(K + 9 * c, D + 4 * c);
  }
  const int NF = N > 1 ? N - 1 : 1;
  std::vector<double> Dm(16 * (size_t)NF, 0.0);
  std::vector<int32_t> has(NF, 0);
  for (int k = 0; k < N - 1; k++) has[k] = hc_smooth_motion(motions + 7 * k, motions + 7 * k + 3, &Dm[16 * (size_t)k]);
  double Wp[36] = {0};
  if (prior_T && !sm::prior_whitener(prior_cov, p->sigma_row, Wp)) return 0;
  std::vector<sm::PassRecord> rec;
  sm::smooth_seq(N, T_in, Dm.data(), has.data(), prior_T ? 1 : 0, prior_T, Wp, gc.data(), cm.data(), frames, C, W, H, X,
                 nw, nr, cand.data(), nc, *p, *out, views, &rec);
  for (size_t q = 0; q < rec.size(); q++) {
    const sm::PassRecord& P = rec[q];
    if (recT) std::memcpy(recT + q * 16 * N, P.T.data(), sizeof(double) * 16 * N);
    if (recAcc) std::memcpy(recAcc + q * 28 * N, P.acc28.data(), sizeof(double) * 28 * N);
    if (recN) std::memcpy(recN + q * N, P.n_obs.data(), sizeof(int32_t) * N);
    if (recE && N > 1) std::memcpy(recE + q * 6 * (N - 1), P.e.data(), sizeof(double) * 6 * (N - 1));
    if (recJ && N > 1) std::memcpy(recJ + q * 72 * (N - 1), P.J.data(), sizeof(double) * 72 * (N - 1));
    if (recPe) std::memcpy(recPe + q * 6, P.pe.data(), sizeof(double) * 6);
    if (recPJ) std::memcpy(recPJ + q * 36, P.pJ.data(), sizeof(double) * 36);
    if (recDelta) std::memcpy(recDelta + q * 6 * N, P.delta.data(), sizeof(double) * 6 * N);
  }
  return 1;
}
// The fixed-lag window (mk_smooth.h, lag_impl.hip): the rules k_lag_slide runs.
// the marginal of view 0 on view 1 and its whitener; returns the drop reason (0: a prior is carried)
int hc_lag_marginalize(const double* H00, const double* g0, const double* Ja, const double* Jb, const double* e,
                       const double* T1, double sigma_row, double* Tp, double* Cov, double* Wp) {
  return mk::smooth::marginal_prior(H00, g0, Ja, Jb, e, T1, sigma_row, Tp, Cov, Wp);
}
// marginalize alone: Lambda's inverse scaled and turned, without the whitener's verdict
int hc_lag_marginal(const double* H00, const double* g0, const double* Ja, const double* Jb, const double* e,
                    const double* T1, double sigma_row, double* Tp, double* Cov) {
  return mk::smooth::marginalize(H00, g0, Ja, Jb, e, T1, sigma_row, Tp, Cov);
}
int hc_lag_schur(const double* H00, const double* g0, const double* Ja, const double* Jb, const double* e, double* Lam,
                 double* eta) {
  return mk::smooth::schur0(H00, g0, Ja, Jb, e, Lam, eta);
}
int hc_lag_whitener(const double* cov, double sigma_row, double* Wp) {
  return mk::smooth::prior_whitener(cov, sigma_row, Wp) ? 1 : 0;
}
void hc_lag_predict(const double* T_newest, const double* D, double* T) { mk::smooth::predict_start(T_newest, D, T); }
// A push sequence on host frames, as mantis_lag_reset + n_push x mantis_lag_push run it: frames
// [push][C], T_start [push][16] with has_start [push], motions [push][7] (row 0 unused), the reset's
// prior (nullable). Per push: out [push], views [push][cap], info [push][4] = views held, has_prior,
// drop_reason, slid, and prior [push][52] = T_p | Cov_p of the push's solve. Returns 0 when the
// reset's prior is refused or a start is missing where it is required.
int hc_lag_seq(int n_push, int cap, const double* T_start, const int32_t* has_start, const double* motions,
               const double* prior_T, const double* prior_cov, const double* Tbc, const double* K, const double* D,
               const uint8_t* const* frames, int C, int W, int H, const double* X, int nw, int nr, int ng,
               const mantis_smooth_params* p, mantis_smooth_result* out, mantis_smooth_view* views, int32_t* info,
               double* prior) {
  namespace rf = mk::refine;
  namespace sm = mk::smooth;
  const int nl = nw + nr + ng;
  std::vector<uint8_t> flags(nl > 0 ? nl : 1);
  rf::line_flags(X, nl, p->landmark_pitch, flags.data());
  std::vector<int32_t> cand(nl > 0 ? nl : 1);
  const int nc = rf::candidates(flags.data(), nl, cand.data());
  std::vector<mk::GnCam> gc(C);
  std::vector<mk::Cam> cm(C);
  for (int c = 0; c < C; c++) {
    rf::gncam_from(Tbc + 16 * c, gc[c]);
    cm[c] = hc_cam(K + 9 * c, D + 4 * c);
  }
  double Tp[16] = {0}, Wp[36] = {0}, Cov[36] = {0};
  int hp = 0;
  if (prior_T) {
    if (!sm::prior_whitener(prior_cov, p->sigma_row, Wp)) return 0;
    std::memcpy(Tp, prior_T, sizeof(Tp));
    std::memcpy(Cov, prior_cov, sizeof(Cov));
    hp = 1;
  }
  std::vector<double> T, Dm;  // the poses held (n x 16), the steps' Transforms (cap x 16)
  std::vector<int32_t> has(cap, 0);
  std::vector<const uint8_t*> fr;
  Dm.assign(16 * (size_t)cap, 0.0);
  std::vector<sm::PassRecord> rec;
  bool last_ok = false;
  for (int q = 0; q < n_push; q++) {
    int n = (int)(T.size() / 16), why = sm::kLagKept, slid = 0;
    double Dn[16] = {0};
    const int hm = q > 0 ? hc_smooth_motion(motions + 7 * q, motions + 7 * q + 3, Dn) : 0;
    if (!has_start[q] && (n == 0 || !hm)) return 0;
    double Ts[16];
    if (has_start[q]) std::memcpy(Ts, T_start + 16 * (size_t)q, sizeof(Ts));
    else sm::predict_start(&T[16 * (size_t)(n - 1)], Dn, Ts);
    if (n == cap) {
      slid = 1;
      why = !has[0] ? sm::kLagNoFactor : !last_ok ? sm::kLagNotOk : sm::kLagKept;
      if (why == sm::kLagKept) {
        const sm::PassRecord& P = rec.back();
        double Hd[36], Ho[36], g[6];
        sm::assemble(0, n, P.acc28.data(), has.data(), P.e.data(), P.J.data(), hp, P.pe.data(), P.pJ.data(), 0.0, Hd, Ho, g);
        why = sm::marginal_prior(Hd, g, P.J.data(), P.J.data() + 36, P.e.data(), &T[16], p->sigma_row, Tp, Cov, Wp);
      } else {
        for (int e = 0; e < 16; e++) Tp[e] = e % 5 == 0 ? 1.0 : 0.0;
        for (int e = 0; e < 36; e++) Cov[e] = Wp[e] = 0.0;
      }
      hp = why == sm::kLagKept;
      T.erase(T.begin(), T.begin() + 16);
      Dm.erase(Dm.begin(), Dm.begin() + 16);
      Dm.resize(16 * (size_t)cap, 0.0);
      has.erase(has.begin());
      has.push_back(0);
      fr.erase(fr.begin(), fr.begin() + C);
      n--;
    }
    T.insert(T.end(), Ts, Ts + 16);
    if (n > 0) {
      std::memcpy(&Dm[16 * (size_t)(n - 1)], Dn, sizeof(Dn));
      has[n - 1] = hm;
    }
    for (int c = 0; c < C; c++) fr.push_back(frames[(size_t)q * C + c]);
    n++;
    mantis_smooth_view* V = views + (size_t)q * cap;
    sm::smooth_seq(n, T.data(), Dm.data(), has.data(), hp, Tp, Wp, gc.data(), cm.data(), fr.data(), C, W, H, X, nw, nr,
                   cand.data(), nc, *p, out[q], V, &rec);
    for (int k = 0; k < n; k++) std::memcpy(&T[16 * (size_t)k], V[k].T_w_b, sizeof(double) * 16);
    last_ok = out[q].status == sm::kOk;
    info[4 * q] = n;
    info[4 * q + 1] = hp;
    info[4 * q + 2] = why;
    info[4 * q + 3] = slid;
    std::memcpy(prior + 52 * (size_t)q, Tp, sizeof(Tp));
    std::memcpy(prior + 52 * (size_t)q + 16, Cov, sizeof(Cov));
  }
  return 1;
}
int hc_sizeof_lag_params(void) { return (int)sizeof(mantis_lag_params); }
int hc_sizeof_lag_info(void) { return (int)sizeof(mantis_lag_info); }

int hc_sizeof_smooth_params(void) { return (int)sizeof(mantis_smooth_params); }
int hc_sizeof_smooth_result(void) { return (int)sizeof(mantis_smooth_result); }
int hc_sizeof_smooth_view(void) { return (int)sizeof(mantis_smooth_view); }

}  // extern "C"
