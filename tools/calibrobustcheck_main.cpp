// Stand-alone check of the calibrations' robust rows (mantis_amd/csrc/
// mk_linecal.h robust_*: the call-wide median, scale and weights at their edge
// cases -- n = 0, 1, 2, equal keys, rejected slots, t exactly 1 --, the stats'
// orders, both extra starved gates of the end of a pass at each problem, and
// one whole robust call per problem -- Ext, Int, Rig -- on painted grids with
// one frame of one view painted from a knocked camera, beside the plain call
// and the switch-off call) on small synthetic frames that are allocated at
// exactly their size, as a program of its own so that it can be built with
// sanitizers and run directly:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o build/calibrobustcheck tools/calibrobustcheck_main.cpp && \
//       build/calibrobustcheck
// Exit status 0 and "calibrobustcheck ok" when every case holds.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../mantis_amd/csrc/mk_linecal.h"

namespace rf = mk::refine;
namespace cal = mk::calib;
namespace ic = mk::icalib;
namespace lc = mk::linecal;

static int g_fail = 0;
static bool g_verbose = false;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      g_fail++;                                                      \
    }                                                                \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd64() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}
static double unif() { return (double)(rnd64() >> 11) / 9007199254740992.0; }

// a camera looking straight down from (x, y, h), yawed by a: T_w_b (the camera is the base)
static void nadir_pose(double x, double y, double h, double a, double* T) {
  const double c = std::cos(a), s = std::sin(a);
  const double R[9] = {c, s, 0, s, -c, 0, 0, 0, -1};  // rot_z(a) * diag(1, -1, -1)
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) T[4 * i + j] = R[3 * i + j];
  T[3] = x; T[7] = y; T[11] = h;
  T[12] = T[13] = T[14] = 0; T[15] = 1;
}
// an extrinsic: yaw a about the base's z, then a tilt b about the camera's x, at the offset (x, y, z)
static void ext_pose(double x, double y, double z, double a, double* E, double b = 0.0) {
  const double c = std::cos(a), s = std::sin(a), cb = std::cos(b), sb = std::sin(b);
  const double M[16] = {c, -s * cb, s * sb, x, s, c * cb, -c * sb, y, 0, sb, cb, z, 0, 0, 0, 1};
  std::memcpy(E, M, sizeof(M));
}
static void mul4(const double* A, const double* B, double* C) {
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      double s = 0;
      for (int k = 0; k < 4; k++) s += A[4 * i + k] * B[4 * k + j];
      C[4 * i + j] = s;
    }
}
// paint the lines y = j pitch and x = j pitch (|j| <= m, each from -len to len) of the floor into a W x H frame of a
// camera at T (camera in the world)
static void paint_grid(std::vector<uint8_t>& img, int W, int H, const double* T, const mk::Cam& cam, double pitch, int m,
                       double len) {
  double Rt[9], t[3];
  rf::pose_parts(T, Rt, t);
  for (int fam = 0; fam < 2; fam++)
    for (int j = -m; j <= m; j++)
      for (int i = -4000; i <= 4000; i++) {
        const double a = i * (len / 4000.0), b = j * pitch;
        const double X[3] = {fam == 0 ? a : b, fam == 0 ? b : a, 0.0};
        const double d[3] = {X[0] - t[0], X[1] - t[1], X[2] - t[2]};
        double p[3];
        for (int r = 0; r < 3; r++) p[r] = Rt[3 * r] * d[0] + Rt[3 * r + 1] * d[1] + Rt[3 * r + 2] * d[2];
        if (!(p[2] > 0)) continue;
        double u, v;
        mk::distort(cam, p[0], p[1], p[2], &u, &v);
        if (!(u > -0.5 && u < W - 0.5 && v > -0.5 && v < H - 0.5)) continue;
        const size_t o = 3 * ((size_t)mk::cv_round(v) * W + mk::cv_round(u));
        img.at(o) = img.at(o + 1) = img.at(o + 2) = 255;
      }
}

// slots whose key is `key` exactly: Sw = 2^20, Skw = key (keys up to 15 x 2^20)
struct Slots {
  std::vector<int32_t> codes, Sw, Skw;
  void add(uint32_t key, int32_t code = 0) {
    codes.push_back(code);
    Sw.push_back(1 << 20);
    Skw.push_back((int32_t)key);
  }
};
struct Pass {
  std::vector<uint32_t> keys;
  std::vector<double> w;
  std::vector<lc::RobustCell> cells;
  rf::RobustPass P;
};
static Pass run_pass(const Slots& s, int N, int C, int nc, const rf::Robust& rb) {
  Pass o;
  const size_t n = (size_t)N * C * nc;
  o.keys.assign(n + 1, 0xdeadbeefu);  // one past the end: must stay
  o.w.assign(n + 1, -7.0);
  o.cells.assign((size_t)N * C, lc::RobustCell{-1, -1, -1.0});
  CHECK(s.codes.size() == n);
  lc::robust_pass(s.codes.data(), s.Sw.data(), s.Skw.data(), N, C, nc, rb, o.keys.data(), o.w.data(), o.cells.data(), o.P);
  CHECK(o.keys[n] == 0xdeadbeefu && o.w[n] == -7.0);
  return o;
}

static void check_rule() {
  const rf::Robust huber{rf::kLossHuber, 0, 1.345, 0.25}, tukey{rf::kLossTukey, 0, 4.685, 0.25};
  const uint32_t one = 1u << 20;
  {  // n = 0: no slot at all, and slots that are all rejected
    Slots s;
    Pass o = run_pass(s, 1, 1, 0, huber);
    CHECK(o.P.n_obs == 0 && o.P.median_key == 0 && o.P.scale == 0.25 && o.P.sum_w == 0.0);
    CHECK(o.cells[0].n_down == 0 && o.cells[0].n_zero == 0 && o.cells[0].sum_w == 0.0);
    for (int k = 0; k < 4; k++) s.add(5 * one, 3);
    o = run_pass(s, 2, 1, 2, tukey);
    CHECK(o.P.n_obs == 0 && o.P.median_key == 0 && o.P.scale == 0.25);
    for (int k = 0; k < 4; k++) CHECK(o.keys[k] == 0 && o.w[k] == 0.0);
  }
  {  // n = 1: the median is the key; n = 2: the lower one, wherever it stands
    Slots s;
    s.add(3 * one);
    Pass o = run_pass(s, 1, 1, 1, tukey);
    CHECK(o.P.n_obs == 1 && o.P.median_key == 3 * one && o.P.scale == 1.4826 * 3.0);
    for (int flip = 0; flip < 2; flip++) {
      Slots t;
      t.add(flip ? 7 * one : 2 * one);
      t.add(9 * one, 4);  // rejected: does not count, whatever its sums
      t.add(flip ? 2 * one : 7 * one);
      o = run_pass(t, 1, 3, 1, huber);
      CHECK(o.P.n_obs == 2 && o.P.median_key == 2 * one && o.keys[1] == 0 && o.w[1] == 0.0);
      CHECK(o.cells[1].n_down == 0 && o.cells[1].n_zero == 0 && o.cells[1].sum_w == 0.0);
    }
  }
  {  // equal keys: the median is that key, every weight the same
    Slots s;
    for (int k = 0; k < 24; k++) s.add(123456);
    Pass o = run_pass(s, 2, 3, 4, tukey);
    CHECK(o.P.median_key == 123456 && o.P.n_obs == 24);
    for (int k = 1; k < 24; k++) CHECK(o.w[k] == o.w[0]);
    CHECK(o.w[0] > 0.0 && o.w[0] < 1.0 && o.P.n_down == 24 && o.P.n_zero == 0);
  }
  {  // t exactly 1: tuning 2 on a scale at its floor of 0.5, key 2^20. Huber 1, Tukey 0
    for (int loss = 1; loss <= 2; loss++) {
      Slots s;
      const uint32_t keys[12] = {0, 1, one - 1, one, one + 1, 2 * one, 0, 0, 0, 0, 0, 0};
      for (uint32_t k : keys) s.add(k);
      Pass o = run_pass(s, 2, 2, 3, rf::Robust{loss, 0, 2.0, 0.5});
      CHECK(o.P.median_key == 0 && o.P.scale == 0.5 && o.w[0] == 1.0);
      CHECK(o.w[3] == (loss == rf::kLossHuber ? 1.0 : 0.0));
      CHECK(o.w[5] == (loss == rf::kLossHuber ? 0.5 : 0.0));
      CHECK(loss == rf::kLossHuber ? o.w[4] < 1.0 && o.w[4] > 0.999 : o.w[4] == 0.0);
      // the cells against a plain recount, and the stats' orders
      std::vector<int32_t> cnt(4, 3);
      mantis_calib_robust_stats st;
      std::memset(&st, 0xff, sizeof(st));
      lc::robust_tally(o.cells.data(), cnt.data(), 2, 2, 5, o.P.median_key, o.P.scale, st);
      int32_t down = 0, zero = 0;
      for (int k = 0; k < 12; k++) {
        down += o.w[k] < 1.0;
        zero += o.w[k] == 0.0;
      }
      CHECK(st.n_down[5] == down && st.n_zero[5] == zero && st.median_key[5] == 0 && st.scale[5] == 0.5);
      CHECK(st.sum_w_view[0] == o.cells[0].sum_w + o.cells[1].sum_w && st.sum_w_view[1] == o.cells[2].sum_w + o.cells[3].sum_w);
      CHECK(st.sum_w_cam[0] == o.cells[0].sum_w + o.cells[2].sum_w && st.sum_w[5] == st.sum_w_view[0] + st.sum_w_view[1]);
      CHECK(st.n_obs_view[0] == 6 && st.n_obs_view[1] == 6 && st.n_obs_view[2] == 0 && st.n_obs_view[255] == 0);
      CHECK(st.n_zero_cam[2] == 0 && st.sum_w_cam[7] == 0.0 && st.sum_w_view[255] == 0.0);
      std::vector<int32_t> pos(4);
      lc::robust_pos(o.cells.data(), cnt.data(), 4, pos.data());
      for (int f = 0; f < 4; f++) CHECK(pos[f] == 3 - o.cells[f].n_zero);
    }
  }
  {  // many random keys against a sort, at a size past one view's slots
    for (int n : {3, 540, 4321}) {
      Slots s;
      std::vector<uint32_t> live;
      for (int k = 0; k < 2 * n; k++) {
        const uint32_t key = (uint32_t)(rnd64() % (15u * one));
        const int32_t code = (rnd64() & 3) == 0 ? 2 : 0;
        s.add(key, code);
        if (!code) live.push_back(key);
      }
      Pass o = run_pass(s, 2, 1, n, tukey);
      std::sort(live.begin(), live.end());
      CHECK(o.P.n_obs == (int32_t)live.size() && o.P.median_key == live[(live.size() - 1) / 2]);
    }
  }
}

// the two extra starved gates at problem P: rows of random numbers, every count above the gates, then a view and
// a free camera with too few rows of positive weight
template <class P>
static void check_gates() {
  const int N = 3, C = 3;
  const uint32_t fe = P::kExt ? 0b110u : 0u, fi = P::kInt ? 0b011u : 0u, pm = P::kInt ? 0xFFu : 0u;  // camera 0 / 2 held
  std::vector<double> acc((size_t)N * C * P::kAcc, 0.0);
  std::vector<int32_t> cnt((size_t)N * C, 80);
  for (int f = 0; f < N * C; f++)
    for (int k = 0; k < 80; k++) {
      double row[P::kRow];
      for (int e = 0; e < P::kRow; e++) row[e] = (unif() - 0.5) * (e == P::kColR ? 0.01 : 1.0);
      const int c = f % C;
      if (P::kExt && !(fe >> c & 1))
        for (int e = 0; e < lc::kPe; e++) row[P::kColE + e] = 0.0;
      if (P::kInt && !(fi >> c & 1))
        for (int e = 0; e < lc::kPi; e++) row[P::kColI + e] = 0.0;
      P::accumulate_row(row, acc.data() + (size_t)P::kAcc * f);
    }
  const mk::Cam cam{150.0, 150.0, 159.5, 119.5, {0.003, -0.01, 0.005, -0.002}};
  auto run = [&](const int32_t* pos, int pass, int I, mantis_rcalib_result& R, double* T) {
    std::memset(&R, 0, sizeof(R));
    for (int c = 0; c < C; c++) {
      ext_pose(0.01 * c, 0, 0, 0.5 * c, R.T_base_cam[c]);
      double th[8];
      ic::cam_to(cam, th);
      for (int e = 0; e < 4; e++) {
        R.K[c][e] = th[e];
        R.D[c][e] = th[4 + e];
      }
    }
    for (int r = 0; r < N; r++) nadir_pose(0.1 * r, 0, 1.0, 0.2 * r, T + 16 * r);
    return P::end_pass(acc.data(), cnt.data(), N, C, fe, fi, pm, pass, I, 12, 60, 1e-6, T, R, nullptr, pos);
  };
  mantis_rcalib_result R;
  double T[16 * N], T0[16 * N];
  for (int r = 0; r < N; r++) nadir_pose(0.1 * r, 0, 1.0, 0.2 * r, T0 + 16 * r);
  CHECK(!run(nullptr, 0, 4, R, T) && R.status == lc::kOk && R.iterations_run == 1);
  std::vector<int32_t> pos = cnt;
  CHECK(!run(pos.data(), 0, 4, R, T) && R.status == lc::kOk);
  pos = cnt;  // view 1 keeps 11 rows of positive weight: one below min_obs
  pos[1 * C + 0] = 4, pos[1 * C + 1] = 4, pos[1 * C + 2] = 3;
  CHECK(run(pos.data(), 0, 4, R, T) && R.status == lc::kStarved && R.iterations_run == 0);
  CHECK(std::memcmp(T, T0, sizeof(T)) == 0 && R.n_obs[0] == 80 * N * C && R.rms[0] > 0);
  pos[1 * C + 2] = 4;
  CHECK(!run(pos.data(), 0, 4, R, T) || R.status != lc::kStarved);
  pos = cnt;  // camera 1 (free in every problem) keeps 59 rows over the views: one below min_obs_cam
  pos[0 * C + 1] = 20, pos[1 * C + 1] = 20, pos[2 * C + 1] = 19;
  CHECK(run(pos.data(), 0, 4, R, T) && R.status == lc::kStarved);
  pos[2 * C + 1] = 20;
  CHECK(!run(pos.data(), 0, 4, R, T));
  pos = cnt;  // a camera held in every mask has no gate of its own
  const int held = P::kExt && P::kInt ? -1 : P::kExt ? 0 : 2;
  if (held >= 0) {
    pos[0 * C + held] = pos[1 * C + held] = pos[2 * C + held] = 4;
    CHECK(!run(pos.data(), 0, 4, R, T));
  }
  pos.assign(pos.size(), 0);  // the final pass solves nothing and starves nothing
  CHECK(run(pos.data(), 4, 4, R, T) && R.status == lc::kOk && R.n_obs[4] == 80 * N * C);
  // conclude: the same gates clear `calibrated`
  pos = cnt;
  R.iterations_run = 0;
  R.status = lc::kOk;
  (void)run(pos.data(), 4, 4, R, T);
  R.iterations_run = 4;
  P::conclude(acc.data(), cnt.data(), N, C, fe, fi, pm, 12, 60, 0.0, R, pos.data());
  CHECK(R.calibrated == 1);
  pos[1 * C + 0] = 4, pos[1 * C + 1] = 4, pos[1 * C + 2] = 3;
  P::conclude(acc.data(), cnt.data(), N, C, fe, fi, pm, 12, 60, 0.0, R, pos.data());
  CHECK(R.calibrated == 0);
}

static double ext_gap(const double* A, const double* B) {
  double s = 0;
  for (int i = 0; i < 3; i++) s += (A[4 * i + 3] - B[4 * i + 3]) * (A[4 * i + 3] - B[4 * i + 3]);
  return std::sqrt(s);
}

// One whole call per problem on painted grids: N views of C cameras at the nominal model, the frame of view 1's
// last camera painted from a camera knocked by 6 mm and 0.6 degrees. Plain, switched off (the plain call's bytes),
// Huber and Tukey.
template <class P>
static void check_seq(const char* name) {
  const int W = 320, H = 240, N = 3, C = 3;
  const mk::Cam nominal{150.0, 150.0, 159.5, 119.5, {0.003, -0.01, 0.005, -0.002}};
  const double pitch = 0.08;
  std::vector<double> X;
  for (int j = -4; j <= 4; j += 2)
    for (int i = -8; i <= 8; i++) {
      X.insert(X.end(), {i * pitch * 0.5, j * pitch, 0.0});
      if (i % 4) X.insert(X.end(), {j * pitch, i * pitch * 0.5, 0.0});
    }
  const int n = (int)X.size() / 3;
  std::vector<uint8_t> flags(n);
  rf::line_flags(X.data(), n, pitch * 0.5, flags.data());
  std::vector<int32_t> cand(n);
  const int nc = rf::candidates(flags.data(), n, cand.data());
  CHECK(nc > 40);
  const uint32_t all = (1u << C) - 1u, fe = P::kExt ? all & ~1u : 0u, fi = P::kInt ? all : 0u, pm = P::kInt ? 0x0Fu : 0u;
  std::vector<double> E((size_t)16 * C), T_true((size_t)16 * N), T0((size_t)16 * N);
  std::vector<mk::Cam> cams(C, nominal);
  for (int c = 0; c < C; c++) ext_pose(0.012 * c - 0.03, 0.01 * (c % 3) - 0.01, 0.0, 0.7 * c, E.data() + 16 * c, 0.45);
  std::vector<std::vector<uint8_t>> imgs((size_t)N * C, std::vector<uint8_t>((size_t)W * H * 3, 0));
  std::vector<const uint8_t*> frames((size_t)N * C);
  for (int r = 0; r < N; r++) {
    double Tn[16], Tt[16];
    nadir_pose(0.03 - 0.02 * r, -0.02 + 0.015 * r, 0.5 + 0.08 * r, 0.3 + 0.4 * r, Tn);
    ext_pose(0, 0, 0, 0.0, Tt, -0.3 + 0.2 * r);
    mul4(Tn, Tt, T_true.data() + 16 * r);
    const double d0[6] = {0.003, -0.003, 0.001, 0.002, -0.001, 0.003};
    std::memcpy(T0.data() + 16 * r, T_true.data() + 16 * r, 16 * sizeof(double));
    cal::right_update(T0.data() + 16 * r, d0);
    for (int c = 0; c < C; c++) {
      double Ec[16], Twc[16];
      std::memcpy(Ec, E.data() + 16 * c, sizeof(Ec));
      if (r == 1 && c == C - 1) {
        const double knock[6] = {0.0, 0.006, 0.0, 0.0, 0.0, 0.0105};
        cal::right_update(Ec, knock);
      }
      mul4(T_true.data() + 16 * r, Ec, Twc);
      paint_grid(imgs[r * C + c], W, H, Twc, nominal, 2 * pitch, 2, 4 * pitch);
      frames[r * C + c] = imgs[r * C + c].data();
    }
  }
  mantis_refine_params p{};
  p.struct_size = sizeof(p);
  p.iterations = 6;
  p.half_window = 6;
  p.white_thresh = 3 * 64 * 64;
  p.min_weight = 12288;
  p.min_obs = 12;
  p.lambda = 1e-6;
  p.landmark_pitch = pitch * 0.5;
  const int32_t moc = 14;
  auto run = [&](const rf::Robust* rb, std::vector<double>& T_out, mantis_rcalib_result& R, mantis_calib_robust_stats* st,
                 std::vector<typename P::Slot>* slots) {
    T_out.assign((size_t)16 * N, 0.0);
    P::seq(T0.data(), E.data(), cams.data(), frames.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p, fe, fi, pm, moc,
           T_out.data(), R, slots ? slots->data() : nullptr, rb, st);
  };
  std::vector<double> T_plain, T_off, T_rob;
  mantis_rcalib_result plain, off, rob;
  mantis_calib_robust_stats st;
  std::vector<typename P::Slot> s_plain((size_t)N * C * nc), s_rob((size_t)N * C * nc);
  run(nullptr, T_plain, plain, nullptr, &s_plain);
  CHECK(plain.status == lc::kOk && plain.iterations_run == 6);
  const rf::Robust none{rf::kLossNone, 0, 0.0, 0.0};
  run(&none, T_off, off, &st, nullptr);
  CHECK(std::memcmp(&off, &plain, sizeof(off)) == 0 && T_off == T_plain);
  for (size_t b = 0; b < sizeof(st); b++) CHECK(((const uint8_t*)&st)[b] == 0);
  for (int loss = 1; loss <= 2; loss++) {
    const rf::Robust rb{loss, 0, loss == rf::kLossTukey ? 4.685 : 1.345, 0.25};
    run(&rb, T_rob, rob, &st, &s_rob);
    const int fp = rob.iterations_run;
    CHECK(rob.status == lc::kOk && fp == 6 && rob.calibrated == 1 && st.loss == loss && st.n_rigs == N && st.n_cams == C);
    CHECK(st.kind == (P::kExt && P::kInt ? lc::kKindRig : P::kInt ? lc::kKindInt : lc::kKindExt));
    CHECK(rob.n_obs[0] == plain.n_obs[0] && rob.rms[0] < plain.rms[0]);  // pass 0 observes the inputs; weights <= 1
    int32_t nv = 0;
    double wv = 0;
    for (int r = 0; r < N; r++) {
      nv += st.n_obs_view[r];
      wv += st.sum_w_view[r];
    }
    CHECK(nv == rob.n_obs[fp] && wv == st.sum_w[fp] && st.sum_w[fp] > 0 && st.sum_w[fp] <= rob.n_obs[fp]);
    for (int k = 0; k <= fp; k++) CHECK(st.scale[k] >= 0.25 && st.n_zero[k] <= st.n_down[k] && st.n_down[k] <= rob.n_obs[k]);
    for (int k = fp + 1; k < 11; k++) CHECK(st.scale[k] == 0.0 && st.median_key[k] == 0 && st.sum_w[k] == 0.0);
    // the knocked frame's view and camera have the lowest mean weight
    int worst_view = 0, worst_cam = 0;
    for (int r = 1; r < N; r++)
      if (st.sum_w_view[r] / st.n_obs_view[r] < st.sum_w_view[worst_view] / st.n_obs_view[worst_view]) worst_view = r;
    for (int c = 1; c < C; c++)
      if (st.sum_w_cam[c] / rob.n_obs_cam[fp][c] < st.sum_w_cam[worst_cam] / rob.n_obs_cam[fp][worst_cam]) worst_cam = c;
    CHECK(worst_view == 1 && worst_cam == C - 1);
    double ep = 0, er = 0;
    for (int r = 0; r < N; r++) {
      ep = std::fmax(ep, ext_gap(T_plain.data() + 16 * r, T_true.data() + 16 * r));
      er = std::fmax(er, ext_gap(T_rob.data() + 16 * r, T_true.data() + 16 * r));
    }
    if (g_verbose)
      std::printf("%s loss %d: worst pose %.3f -> %.3f mm, rms %.3g -> %.3g, scale %.3f, down %d zero %d of %d, mean weight "
                  "view 1 %.3f camera %d %.3f\n",
                  name, loss, 1e3 * ep, 1e3 * er, plain.rms[6], rob.rms[6], st.scale[fp], st.n_down[fp], st.n_zero[fp],
                  rob.n_obs[fp], st.sum_w_view[1] / st.n_obs_view[1], C - 1, st.sum_w_cam[C - 1] / rob.n_obs_cam[fp][C - 1]);
    // with both blocks free these small frames leave focal length, height and the extrinsics' offsets nearly
    // tied (the rig check program's note), so the pose distance is reported but asserted for Ext and Int only
    if (!(P::kExt && P::kInt)) CHECK(er < ep);
    // the recorded rows are unweighted: a rejected slot is zeros
    for (size_t k = 0; k < s_rob.size(); k++)
      if (s_rob[k].code)
        for (int e = 0; e < P::kRow; e++) CHECK(s_rob[k].row[e] == 0.0);
    // I = 0: the inputs bit for bit, the stats of pass 0 filled
    mantis_refine_params p0 = p;
    p0.iterations = 0;
    std::vector<double> T_z((size_t)16 * N);
    mantis_rcalib_result z;
    mantis_calib_robust_stats sz;
    P::seq(T0.data(), E.data(), cams.data(), frames.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p0, fe, fi, pm,
           moc, T_z.data(), z, nullptr, &rb, &sz);
    CHECK(T_z == T0 && z.iterations_run == 0 && z.status == lc::kOk && sz.sum_w[0] == st.sum_w[0]);
    CHECK(sz.median_key[0] == st.median_key[0] && sz.median_key[0] > 0);
    for (int c = 0; c < C; c++) CHECK(std::memcmp(z.T_base_cam[c], E.data() + 16 * c, 16 * sizeof(double)) == 0);
    // no candidates at all: n = 0 through the whole call
    P::seq(T0.data(), E.data(), cams.data(), frames.data(), N, C, W, H, X.data(), n, 0, cand.data(), 0, p, fe, fi, pm, moc,
           T_z.data(), z, nullptr, &rb, &sz);
    CHECK(z.status == lc::kStarved && z.rms[0] == 0.0 && sz.median_key[0] == 0 && sz.scale[0] == 0.25);
  }
  // a tuning so small that only rows of key 0 keep a positive weight: with the views' gate at the smallest
  // view's code-0 count the plain call passes it and the robust gates alone starve pass 0
  mantis_refine_params p0 = p;
  p0.iterations = 0;
  std::vector<double> T_z((size_t)16 * N);
  P::seq(T0.data(), E.data(), cams.data(), frames.data(), N, C, W, H, X.data(), n, 0, cand.data(), nc, p0, fe, fi, pm, moc,
         T_z.data(), rob, s_rob.data());
  int32_t least = 1 << 30, least_pos = 1 << 30;
  for (int r = 0; r < N; r++) {
    int32_t cnt = 0, pos = 0;
    for (int k = 0; k < C * nc; k++) {
      const typename P::Slot& o = s_rob[(size_t)r * C * nc + k];
      cnt += o.code == 0;
      pos += o.code == 0 && rf::robust_key(o.Sw, o.Skw) == 0;
    }
    least = std::min(least, cnt);
    least_pos = std::min(least_pos, pos);
  }
  CHECK(least_pos < least && least >= 12);
  p.min_obs = least;
  const rf::Robust tiny{rf::kLossTukey, 0, 1e-6, 0.25};
  run(&tiny, T_rob, rob, &st, nullptr);
  CHECK(rob.status == lc::kStarved && rob.iterations_run == 0 && rob.n_obs[0] == plain.n_obs[0] && T_rob == T0);
  CHECK(st.n_zero[0] > 0 && st.n_obs_view[0] >= least);
  run(nullptr, T_rob, rob, nullptr, nullptr);
  CHECK(rob.status != lc::kStarved || rob.iterations_run > 0);
}

int main(int argc, char** argv) {
  g_verbose = argc > 1 && std::strcmp(argv[1], "-v") == 0;
  check_rule();
  check_gates<lc::Ext>();
  check_gates<lc::Int>();
  check_gates<lc::Rig>();
  check_seq<lc::Ext>("ext");
  check_seq<lc::Int>("int");
  check_seq<lc::Rig>("rig");
  if (g_fail) {
    std::printf("calibrobustcheck: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("calibrobustcheck ok\n");
  return 0;
}
