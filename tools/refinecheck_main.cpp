// Stand-alone check of the line refinement's rules (mantis_amd/csrc/
// mk_refine.h: line flags, one observation with its window over the frame
// edges, the end of a pass, the gate and the covariance, the whole iteration,
// the robust rows: key, median, scale, weight, the starved gate)
// on small synthetic frames that are allocated at exactly their size, as a
// program of its own so that it can be built with sanitizers and run directly:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o build/refinecheck tools/refinecheck_main.cpp && build/refinecheck
// Exit status 0 and "refinecheck ok" when every case holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../mantis_amd/csrc/mk_refine.h"

namespace rf = mk::refine;

static int g_fail = 0;
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

static mk::GnCam identity_cam() {
  mk::GnCam g;
  const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  rf::gncam_from(I, g);
  return g;
}

// the observation restated with bounds-checked reads: code, Sw, Skw
static int observe_ref(const double* T, const mk::Cam& cam, const std::vector<uint8_t>& img, int W, int H,
                       const double* X, int axis, const int* tg, const rf::Window& win, long long* Sw, long long* Skw) {
  double Rt[9], t[3];
  rf::pose_parts(T, Rt, t);
  rf::Geom g;
  *Sw = *Skw = 0;
  const int gc = rf::geom(Rt, t, identity_cam(), X, axis, g);
  if (gc) return gc;
  const double s = 1.0 / cam.fx;
  std::vector<long long> w;
  for (int k = -win.R; k <= win.R; k++) {
    double u, v;
    mk::distort(cam, g.m0[0] + (double)k * s * g.nh[0], g.m0[1] + (double)k * s * g.nh[1], 1.0, &u, &v);
    if (!std::isfinite(u) || !std::isfinite(v)) return rf::kOutside;
    if (std::fabs(u) > 1e9 || std::fabs(v) > 1e9) return rf::kOutside;
    const long long x = (long long)std::nearbyint(u), y = (long long)std::nearbyint(v);
    if (x < 0 || x >= W || y < 0 || y >= H) return rf::kOutside;
    long long d2 = 0;
    for (int ch = 0; ch < 3; ch++) {
      const long long e = (long long)img.at((size_t)(3 * (y * W + x) + ch)) - tg[ch];
      d2 += e * e;
    }
    w.push_back(win.white_thresh - d2 > 0 ? win.white_thresh - d2 : 0);
  }
  for (int k = -win.R; k <= win.R; k++) {
    *Sw += w[k + win.R];
    *Skw += k * w[k + win.R];
  }
  if (w.front() > 0 || w.back() > 0) return rf::kWindowEnd;
  if (*Sw < win.min_weight) return rf::kWeak;
  return 0;
}

// paint the lines y = j pitch and x = j pitch (|j| <= m, each from -len to len) of the floor into a W x H frame seen from T
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

static void check_flags() {
  const double X[] = {0, 0, 0, 0.08, 0, 0, -0.08, 0, 0, 0, 0.08, 0, 0, -0.08, 0, 0.5, 0.5, 0, 0.5, 0.5, 0};
  uint8_t f[7];
  rf::line_flags(X, 7, 0.08, f);
  const uint8_t want[7] = {3, 1, 1, 2, 2, 0, 0};  // a duplicate at the same place is no neighbour
  CHECK(std::memcmp(f, want, 7) == 0);
  int32_t cand[7];
  CHECK(rf::candidates(f, 7, cand) == 4);
  CHECK(cand[0] == 1 && cand[1] == 2 && cand[2] == (3 | 1 << 16) && cand[3] == (4 | 1 << 16));
  rf::line_flags(X, 0, 0.08, f);
  CHECK(rf::candidates(f, 0, cand) == 0);
}

// windows against frames of exactly W x H x 3 bytes, the candidate pushed over every edge and corner
static void check_windows() {
  const int tg[3] = {255, 255, 255};
  int codes_seen[6] = {0};
  for (int R : {1, 15, 12}) {
    for (int size = 0; size < 3; size++) {
      const int W = size == 0 ? 40 : size == 1 ? 97 : 33, H = size == 0 ? 32 : size == 1 ? 61 : 33;
      const mk::Cam cam{60.0, 60.0, W / 2.0 - 0.25, H / 2.0 + 0.125, {0.003, -0.01, 0.005, -0.002}};
      std::vector<uint8_t> img((size_t)W * H * 3);
      for (int trial = 0; trial < 4000; trial++) {
        if (trial % 50 == 0)
          for (auto& b : img) b = (rnd64() & 3) ? (uint8_t)(rnd64() & 0xff) : 255;
        // the landmark at the origin; the camera placed so that it projects around an edge or a corner
        const double h = 0.5 + unif();
        const int edge = trial % 9;
        const double ex = (edge % 3 - 1) * (W / 2.0) / cam.fx, ey = (edge / 3 - 1) * (H / 2.0) / cam.fy;
        const double jx = (unif() - 0.5) * 40.0 / cam.fx, jy = (unif() - 0.5) * 40.0 / cam.fy;
        double T[16];
        nadir_pose(-(ex + jx) * h, (ey + jy) * h, h, (trial % 7) * 0.9, T);
        if (trial % 11 == 0) T[11] = -T[11];  // under the floor: behind the camera
        const double X[3] = {0, 0, 0};
        const rf::Window win{R, 3 * 64 * 64, trial % 3 ? 24576 : 1, 0};
        double Rt[9], t[3];
        rf::pose_parts(T, Rt, t);
        rf::Slot o;
        int tie;
        rf::observe(Rt, t, identity_cam(), cam, img.data(), W, H, X, trial & 1, tg, win, o, &tie);
        long long Sw, Skw;
        const int code = observe_ref(T, cam, img, W, H, X, trial & 1, tg, win, &Sw, &Skw);
        CHECK(o.code == code);
        if (code == 0 || code == rf::kWindowEnd || code == rf::kWeak) CHECK(o.Sw == Sw && o.Skw == Skw);
        else CHECK(o.Sw == 0 && o.Skw == 0);
        if (code == 0) {
          CHECK(o.row[6] == -(((double)Skw / (double)Sw) * (1.0 / cam.fx)));
          for (int e = 0; e < 7; e++) CHECK(std::isfinite(o.row[e]));
        } else {
          for (int e = 0; e < 7; e++) CHECK(o.row[e] == 0.0);
        }
        codes_seen[code]++;
      }
    }
  }
  for (int c : {0, 1, 3, 4, 5}) CHECK(codes_seen[c] > 0);
  std::printf("windows: codes 0..5 seen %d %d %d %d %d %d\n", codes_seen[0], codes_seen[1], codes_seen[2], codes_seen[3],
              codes_seen[4], codes_seen[5]);
  // no tangent: a line through the camera's axis seen end-on cannot happen on the floor; a degenerate pose can
  double T[16] = {0};  // R_wb = 0: every direction maps to 0
  T[11] = 1; T[15] = 1;
  T[2] = 0; T[6] = 0; T[10] = -1;  // only z survives: p_z > 0, the tangent is 0
  double Rt[9], t[3];
  rf::pose_parts(T, Rt, t);
  rf::Geom g;
  const double X[3] = {0, 0, 0};
  CHECK(rf::geom(Rt, t, identity_cam(), X, 0, g) == rf::kNoTangent);
}

// starved and singular systems, the gate and the covariance
static void check_passes() {
  mantis_refine_result R{};
  for (int e = 0; e < 16; e++) R.T_w_b[e] = (e % 5 == 0) ? 1.0 : 0.0;
  double acc[28] = {0};
  // starved: fewer rows than min_obs, the pose stays
  CHECK(rf::end_pass(acc, 11, 0, 4, 12, 0.0, R) && R.status == rf::kStarved && R.iterations_run == 0);
  CHECK(R.n_obs[0] == 11 && R.rms[0] == 0.0);
  // no row at all: rms is 0, not 0 / 0
  R = mantis_refine_result{};
  CHECK(rf::end_pass(acc, 0, 0, 4, 12, 0.0, R) && R.status == rf::kStarved && R.rms[0] == 0.0);
  // singular: rows that see one direction only
  R = mantis_refine_result{};
  for (int e = 0; e < 16; e++) R.T_w_b[e] = (e % 5 == 0) ? 1.0 : 0.0;
  for (int k = 0; k < 20; k++) {
    const double row[7] = {1, 0, 0, 0, 0, 0, 0.01};
    rf::accumulate_row(row, acc);
  }
  CHECK(rf::end_pass(acc, 20, 0, 4, 12, 0.0, R) && R.status == rf::kSingular && R.iterations_run == 0);
  CHECK(R.T_w_b[0] == 1.0 && R.T_w_b[3] == 0.0);
  rf::conclude(acc, 12, 0.0, R);
  CHECK(R.refined == 0);
  for (int e = 0; e < 36; e++) CHECK(R.covariance[e] == 0.0);
  // the final pass solves nothing, whatever the system
  R = mantis_refine_result{};
  CHECK(rf::end_pass(acc, 20, 4, 4, 12, 0.0, R) && R.status == rf::kOk && R.n_obs[4] == 20);
  // a well-posed system: identity normal matrix, n_obs = 106 -> sigma^2 = r^T r / 100
  double a2[28] = {0};
  for (int d = 0; d < 6; d++) {
    double row[7] = {0};
    row[d] = 1.0;
    rf::accumulate_row(row, a2);
  }
  a2[27] = 4.0;
  R = mantis_refine_result{};
  for (int e = 0; e < 16; e++) R.T_w_b[e] = (e % 5 == 0) ? 1.0 : 0.0;
  CHECK(!rf::end_pass(a2, 106, 0, 1, 12, 0.0, R) && R.iterations_run == 1);
  CHECK(rf::end_pass(a2, 106, 1, 1, 12, 0.0, R));
  rf::conclude(a2, 12, 0.0, R);
  CHECK(R.refined == 1);
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) CHECK(std::fabs(R.covariance[6 * i + j] - (i == j ? 0.04 : 0.0)) < 1e-15);
  R.n_obs[1] = 6;  // n_obs <= 6: no covariance
  rf::conclude(a2, 6, 0.0, R);
  CHECK(R.refined == 0 && R.covariance[0] == 0.0);
}

// the whole iteration on a painted grid, one camera and three, R = 1 and R = 15 included
static void check_seq() {
  const int W = 320, H = 240;
  const mk::Cam cam{150.0, 150.0, 159.5, 119.5, {0.003, -0.01, 0.005, -0.002}};
  const double pitch = 0.08;
  std::vector<double> X;  // landmarks every pitch / 2 along the lines every 2 pitch: candidates and intersections
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
  double T[16];
  nadir_pose(0.03, -0.02, 0.6, 0.3, T);
  std::vector<uint8_t> img((size_t)W * H * 3, 0);
  paint_grid(img, W, H, T, cam, 2 * pitch, 2, 4 * pitch);
  const uint8_t* frames[3] = {img.data(), img.data(), img.data()};
  const mk::GnCam gcs[3] = {identity_cam(), identity_cam(), identity_cam()};
  const mk::Cam cams[3] = {cam, cam, cam};
  for (int R : {1, 6, 15})
    for (int C : {1, 3}) {
      mantis_refine_params p{};
      p.struct_size = sizeof(p);
      p.iterations = 5;
      p.half_window = R;
      p.white_thresh = 3 * 64 * 64;
      p.min_weight = 12288;
      p.min_obs = 12;
      p.landmark_pitch = pitch * 0.5;
      double T0[16];
      const double off = R == 1 ? 0.0004 : 0.004;  // the start must leave the lines inside the window
      nadir_pose(0.03 + off, -0.02 - off, 0.6, 0.3 + (R == 1 ? 0.0005 : 0.004), T0);
      mantis_refine_result res;
      std::vector<rf::Slot> slots((size_t)C * nc);
      rf::refine_seq(T0, gcs, cams, frames, C, W, H, X.data(), n, 0, cand.data(), nc, p, res, slots.data());
      const double d0 = std::hypot(T0[3] - T[3], T0[7] - T[7]), d1 = std::hypot(res.T_w_b[3] - T[3], res.T_w_b[7] - T[7]);
      std::printf("seq R=%d C=%d: status %d refined %d runs %d n_obs %d..%d  %.5f -> %.5f m\n", R, C, res.status,
                  res.refined, res.iterations_run, res.n_obs[0], res.n_obs[res.iterations_run], d0, d1);
      CHECK(res.status == rf::kOk && res.iterations_run == 5 && res.n_cand == nc);
      CHECK(res.n_obs[5] >= 12 && res.n_obs[5] % C == 0);
      if (R > 1) CHECK(res.refined == 1 && d1 < d0);
      // I = 0: the pose comes back bit for bit
      p.iterations = 0;
      rf::refine_seq(T0, gcs, cams, frames, C, W, H, X.data(), n, 0, cand.data(), nc, p, res, nullptr);
      CHECK(std::memcmp(res.T_w_b, T0, sizeof(T0)) == 0 && res.iterations_run == 0);
    }
  // starved: a black frame; the pose stays
  std::vector<uint8_t> black((size_t)W * H * 3, 0);
  const uint8_t* bf[1] = {black.data()};
  mantis_refine_params p{};
  p.iterations = 4; p.half_window = 12; p.white_thresh = 12288; p.min_weight = 24576; p.min_obs = 12;
  p.landmark_pitch = pitch * 0.5;
  mantis_refine_result res;
  rf::refine_seq(T, gcs, cams, bf, 1, W, H, X.data(), n, 0, cand.data(), nc, p, res, nullptr);
  CHECK(res.status == rf::kStarved && res.refined == 0 && std::memcmp(res.T_w_b, T, sizeof(T)) == 0);
  // singular: one family of lines only constrains no motion along them
  std::vector<double> X1;
  for (int i = -8; i <= 8; i++) X1.insert(X1.end(), {i * pitch * 0.5, 0.0, 0.0});
  std::vector<uint8_t> f1(17);
  rf::line_flags(X1.data(), 17, pitch * 0.5, f1.data());
  std::vector<int32_t> c1(17);
  const int nc1 = rf::candidates(f1.data(), 17, c1.data());
  CHECK(nc1 == 17);
  double Ts[16];
  nadir_pose(0.0, 0.0, 0.6, 0.0, Ts);
  std::fill(img.begin(), img.end(), 0);
  paint_grid(img, W, H, Ts, cam, 2 * pitch, 0, 4 * pitch);  // the lines x = 0 and y = 0
  rf::refine_seq(Ts, gcs, cams, frames, 1, W, H, X1.data(), 17, 0, c1.data(), nc1, p, res, nullptr);
  std::printf("one line: status %d runs %d n_obs %d\n", res.status, res.iterations_run, res.n_obs[0]);
  CHECK(res.n_obs[0] >= 12 || res.status == rf::kStarved);
  for (int e = 0; e < 16; e++) CHECK(std::isfinite(res.T_w_b[e]));
}

// the robust rows: keys at their limits, the lower median of 0, 1, 2 and many keys (buffers of
// exactly n entries), both losses, t exactly 1, the starved gate, the whole iteration
static void check_robust() {
  const int32_t big = 31 * 195075;
  CHECK(rf::robust_key(1, 0) == 0 && rf::robust_key(1, 15) == (15u << 20) && rf::robust_key(1, -15) == (15u << 20));
  CHECK(rf::robust_key(big, 15 * big) == (15u << 20) && rf::robust_key(big, -15 * big) == (15u << 20));
  CHECK(rf::robust_key(big, big) == (1u << 20) && rf::robust_key(big, -1) == 0 && rf::robust_key(3, -2) == 699050);
  for (int loss : {rf::kLossHuber, rf::kLossTukey}) {
    const rf::Robust rb{loss, 0, loss == rf::kLossHuber ? 1.345 : 4.685, 0.25};
    for (int n : {0, 1, 2, 3, 8, 9, 4321}) {
      std::vector<uint32_t> keys(n);
      std::vector<int32_t> codes(n);
      std::vector<double> w(n);
      for (int k = 0; k < n; k++) {
        keys[k] = (uint32_t)(rnd64() % (15u << 20));
        codes[k] = (rnd64() % 4) ? 0 : 4;
      }
      for (int masked = 0; masked < 2; masked++) {
        rf::RobustPass P;
        rf::robust_weights(keys.data(), masked ? codes.data() : nullptr, n, rb, w.data(), P);
        std::vector<uint32_t> live;
        for (int k = 0; k < n; k++)
          if (!masked || codes[k] == 0) live.push_back(keys[k]);
        std::sort(live.begin(), live.end());
        CHECK(P.n_obs == (int)live.size());
        CHECK(P.median_key == (live.empty() ? 0u : live[(live.size() - 1) / 2]));
        CHECK(P.scale == rf::robust_scale(P.median_key, 0.25) && P.scale >= 0.25);
        int down = 0, zero = 0;
        double sum = 0;
        for (int k = 0; k < n; k++) {
          if (masked && codes[k]) {
            CHECK(w[k] == 0.0);
            continue;
          }
          CHECK(w[k] >= 0.0 && w[k] <= 1.0);
          down += w[k] < 1.0;
          zero += w[k] == 0.0;
          sum += w[k];
        }
        CHECK(down == P.n_down && zero == P.n_zero && sum == P.sum_w);
        if (loss == rf::kLossHuber) CHECK(P.n_zero == 0);
      }
      // all keys equal: the median is that key and every row weighs the same
      std::fill(keys.begin(), keys.end(), 5u << 20);
      rf::RobustPass P;
      rf::robust_weights(keys.data(), nullptr, n, rb, w.data(), P);
      CHECK(P.median_key == (n ? 5u << 20 : 0u));
      for (int k = 1; k < n; k++) CHECK(w[k] == w[0]);
      if (n) CHECK(w[0] == (loss == rf::kLossHuber ? 1.0 : rf::robust_weight(5u << 20, rb, 1.4826 * 5.0)) && w[0] > 0);
    }
    // t exactly 1: tuning 2 on a scale of 0.5
    const rf::Robust one{loss, 0, 2.0, 0.5};
    CHECK(rf::robust_weight(1u << 20, one, 0.5) == (loss == rf::kLossHuber ? 1.0 : 0.0));
    CHECK(rf::robust_weight((1u << 20) - 1, one, 0.5) > 0.0 && rf::robust_weight((1u << 20) + 1, one, 0.5) < 1.0);
    CHECK(rf::robust_weight(0, one, 0.5) == 1.0);
  }
  // the starved gate: rows enough, positive weights too few
  double acc[28] = {0};
  for (int k = 0; k < 20; k++) {
    double row[7] = {0, 0, 0, 0, 0, 0, 0.01};
    row[k % 6] = 1.0;
    rf::accumulate_row(row, acc);
  }
  mantis_refine_result R{};
  for (int e = 0; e < 16; e++) R.T_w_b[e] = (e % 5 == 0) ? 1.0 : 0.0;
  CHECK(rf::end_pass_robust(acc, 20, 11, 0, 4, 12, 0.0, R) && R.status == rf::kStarved && R.n_obs[0] == 20);
  CHECK(R.rms[0] == std::sqrt(acc[27] / 20.0) && R.iterations_run == 0 && R.T_w_b[3] == 0.0);
  R.status = rf::kOk;
  CHECK(!rf::end_pass_robust(acc, 20, 12, 0, 4, 12, 0.0, R) && R.status == rf::kOk && R.iterations_run == 1);
  CHECK(rf::end_pass_robust(acc, 20, 0, 4, 4, 12, 0.0, R) && R.status == rf::kOk);  // the final pass starves nothing

  // the whole iteration on check_seq's painted grid, three cameras of which one sees a grid painted from another pose
  const int W = 320, H = 240;
  const mk::Cam cam{150.0, 150.0, 159.5, 119.5, {0.003, -0.01, 0.005, -0.002}};
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
  double T[16], Tbad[16], T0[16];
  nadir_pose(0.03, -0.02, 0.6, 0.3, T);
  nadir_pose(0.03, -0.02 + 0.006, 0.6, 0.3 + 0.004, Tbad);
  nadir_pose(0.034, -0.024, 0.6, 0.304, T0);
  std::vector<uint8_t> img((size_t)W * H * 3, 0), bad((size_t)W * H * 3, 0);
  paint_grid(img, W, H, T, cam, 2 * pitch, 2, 4 * pitch);
  paint_grid(bad, W, H, Tbad, cam, 2 * pitch, 2, 4 * pitch);
  const uint8_t* frames[3] = {img.data(), img.data(), bad.data()};
  const mk::GnCam gcs[3] = {identity_cam(), identity_cam(), identity_cam()};
  const mk::Cam cams[3] = {cam, cam, cam};
  mantis_refine_params p{};
  p.struct_size = sizeof(p);
  p.iterations = 5;
  p.half_window = 6;
  p.white_thresh = 3 * 64 * 64;
  p.min_weight = 12288;
  p.min_obs = 12;
  p.landmark_pitch = pitch * 0.5;
  mantis_refine_result plain, off;
  rf::refine_seq(T0, gcs, cams, frames, 3, W, H, X.data(), n, 0, cand.data(), nc, p, plain, nullptr);
  mantis_refine_robust_stats st;
  rf::refine_seq_robust(T0, gcs, cams, frames, 3, W, H, X.data(), n, 0, cand.data(), nc, p, rf::Robust{0, 0, 1.0, 1.0}, off,
                        &st);
  CHECK(std::memcmp(&plain, &off, sizeof(plain)) == 0 && st.loss == 0 && st.n_down[0] == 0);
  const double d0 = std::hypot(plain.T_w_b[3] - T[3], plain.T_w_b[7] - T[7]);
  for (int loss : {rf::kLossHuber, rf::kLossTukey}) {
    mantis_refine_result res;
    rf::refine_seq_robust(T0, gcs, cams, frames, 3, W, H, X.data(), n, 0, cand.data(), nc, p,
                          rf::Robust{loss, 0, loss == rf::kLossHuber ? 1.345 : 4.685, 0.25}, res, &st);
    const double d1 = std::hypot(res.T_w_b[3] - T[3], res.T_w_b[7] - T[7]);
    const int fp = res.iterations_run;
    std::printf("robust loss %d: status %d runs %d n_obs %d down %d zero %d scale %.3f  plain %.5f -> %.5f m\n", loss,
                res.status, fp, res.n_obs[fp], st.n_down[fp], st.n_zero[fp], st.scale[fp], d0, d1);
    CHECK(res.status == rf::kOk && fp == 5 && st.loss == loss && st.n_down[fp] > 0 && st.sum_w[fp] < res.n_obs[fp]);
    CHECK(d1 < d0);
    for (int k = fp + 1; k < 11; k++) CHECK(st.median_key[k] == 0 && st.scale[k] == 0.0 && st.sum_w[k] == 0.0);
  }
  // no candidates at all: every pass is empty, the stats are defined
  mantis_refine_result res;
  rf::refine_seq_robust(T0, gcs, cams, frames, 3, W, H, X.data(), n, 0, cand.data(), 0, p, rf::Robust{2, 0, 4.685, 0.25},
                        res, &st);
  CHECK(res.status == rf::kStarved && st.median_key[0] == 0 && st.scale[0] == 0.25 && st.sum_w[0] == 0.0);
}

int main() {
  check_flags();
  check_windows();
  check_passes();
  check_seq();
  check_robust();
  if (g_fail) {
    std::printf("refinecheck: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("refinecheck ok\n");
  return 0;
}
