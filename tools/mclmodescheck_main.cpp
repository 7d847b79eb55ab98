// Stand-alone check of the rules of the Monte Carlo localization modes
// (mantis_amd/csrc/mk_mcl_modes.h: the cell key, the bins and their order, the
// lattice site, modes_seq) on constructed and random sets up to N = 4096, as
// a program of its own so that it can be built with sanitizers and run directly:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o build/mclmodescheck tools/mclmodescheck_main.cpp && build/mclmodescheck
// Exit status 0 and "mclmodescheck ok" when every case holds.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "../mantis_amd/csrc/mk_mcl_modes.h"

namespace mc = mk::mcl;

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

static const double kG = 0.32;

// a pose with heading `yaw` about z at (x, y, 1.2), tilted a little
static mk::Xf pose(double yaw, double x, double y, double tilt = 0.0) {
  mk::Xf T;
  mk::basis_from_rpy(0.0, tilt, yaw, T.R);
  T.t[0] = x; T.t[1] = y; T.t[2] = 1.2;
  return T;
}

int main() {
  // the key at exactly +-0.5 cell, at the edge of the range and far outside
  const mk::Xf A0 = pose(0.0, 0.0, 0.0);
  int32_t ix, iy, k;
  CHECK(0.5 * kG / kG == 0.5);
  CHECK(mc::cell_key(pose(0, 0.5 * kG, 0), A0, kG, &ix, &iy, &k) == mc::cell_bin(1, 0, 0) && ix == 1 && iy == 0);
  CHECK(mc::cell_key(pose(0, -0.5 * kG, 0), A0, kG, &ix, &iy, &k) == mc::cell_bin(0, 0, 0) && ix == 0);
  CHECK(mc::cell_key(pose(0, std::nextafter(-0.5 * kG, -1.0), 0), A0, kG, &ix, &iy, &k) == mc::cell_bin(-1, 0, 0) && ix == -1);
  CHECK(mc::cell_key(pose(0, 0, std::nextafter(0.5 * kG, 0.0)), A0, kG, &ix, &iy, &k) == mc::cell_bin(0, 0, 0) && iy == 0);
  for (int n : {-8, -7, 7, 8}) {
    const int32_t b = mc::cell_key(pose(0, n * kG, -n * kG), A0, kG, &ix, &iy, &k);
    CHECK(ix == n && iy == -n && (b < mc::kModeBins) == (n == 7 || n == -7));
  }
  CHECK(mc::cell_key(pose(0, 1e300, -1e300), A0, kG, &ix, &iy, &k) == mc::kModeBins && ix > 0 && iy < 0);
  CHECK(mc::cell_key(pose(0, NAN, 0), A0, kG, &ix, &iy, &k) == mc::kModeBins);
  CHECK(mc::cell_bin(-7, -7, 0) == 0 && mc::cell_bin(7, 7, 3) == mc::kModeBins - 1 && mc::cell_bin(8, 0, 0) == mc::kModeBins);
  for (int b = 0; b < mc::kModeBins; b++) {
    mc::bin_cell(b, &ix, &iy, &k);
    CHECK(mc::cell_in_range(ix, iy) && k >= 0 && k < 4 && mc::cell_bin(ix, iy, k) == b);
  }
  // yaw quadrants: the axis headings, ties on the diagonals, a vertical x-axis
  const double kHalfPi = 1.5707963267948966;
  for (int q4 = 0; q4 < 4; q4++)
    for (double jit : {-0.4, 0.0, 0.4}) CHECK(mc::yaw_quadrant(pose(0.7 + q4 * kHalfPi + jit, 0, 0, 0.1), pose(0.7, 0, 0)) == q4);
  {
    mk::Xf I = pose(0, 0, 0), D = I;
    const double v = std::sqrt(0.5);
    const double h[4][2] = {{v, v}, {-v, v}, {-v, -v}, {v, -v}};
    const int want[4] = {0, 2, 2, 0};
    for (int i = 0; i < 4; i++) {
      D.R[0] = h[i][0]; D.R[3] = h[i][1];
      CHECK(mc::yaw_quadrant(D, I) == want[i]);
    }
    D.R[0] = 0; D.R[3] = 0;
    CHECK(mc::yaw_quadrant(D, I) == 0 && mc::yaw_quadrant(I, D) == 0);
  }
  // the packed orders
  CHECK(mc::heaviest_pack(5, 3) > mc::heaviest_pack(5, 4) && mc::heaviest_pack(6, 4095) > mc::heaviest_pack(5, 0));
  CHECK(mc::heaviest_index(mc::heaviest_pack(1ULL << 40, 4095)) == 4095 && mc::heaviest_index(mc::heaviest_pack(1, 0)) == 0);
  CHECK(mc::mode_order_key(7, 10) > mc::mode_order_key(7, 11) && mc::mode_order_key(8, 899) > mc::mode_order_key(7, 0));
  CHECK(mc::mode_order_key(0, 5) == 0 && mc::mode_order_bin(mc::mode_order_key(4096ULL << 40, 899)) == 899);
  CHECK((mc::mode_order_key(4096ULL << 40, 0) >> 10) == (4096ULL << 40));
  // lattice sites: x runs fastest, from (-cx, -cy) to (cx, cy)
  for (int cx = 0; cx <= 7; cx++)
    for (int cy = 0; cy <= 7; cy++) {
      const int w = 2 * cx + 1, n = w * (2 * cy + 1);
      for (int s = 0; s < n; s++) {
        mc::lattice_site(s, cx, cy, &ix, &iy);
        CHECK(ix == s % w - cx && iy == s / w - cy && ix >= -cx && ix <= cx && iy >= -cy && iy <= cy);
      }
    }

  // modes_seq on random sets: bins against a map, order, sums, the estimate's shape
  const int sizes[] = {1, 2, 7, 64, 257, 1025, 4096};
  for (int N : sizes) {
    for (int shape = 0; shape < 5; shape++) {  // 0 spread, 1 one cell, 2 all outside but the anchor, 3 equal weights, 4 lost
      const int C = 1 + (int)(rnd64() % 3);
      std::vector<mk::Xf> T(N);
      std::vector<uint64_t> q(N);
      std::vector<long long> sums((size_t)N * C);
      std::vector<int32_t> counts((size_t)N * C);
      const double x0 = unif() - 0.5, y0 = unif() - 0.5, yaw0 = 6.0 * (unif() - 0.5);
      for (int j = 0; j < N; j++) {
        const int span = shape == 1 ? 0 : 9;
        int cx = span ? (int)(rnd64() % (2 * span + 1)) - span : 0, cy = span ? (int)(rnd64() % (2 * span + 1)) - span : 0;
        if (shape == 2) {  // the anchor-to-be at the centre, everybody else 8 cells and more away
          cx = j == N / 2 ? 0 : 8 + (int)(rnd64() % 4);
          cy = j == N / 2 ? 0 : cy;
        }
        const int quad = shape == 1 ? 0 : (int)(rnd64() % 4);
        T[j] = pose(yaw0 + quad * kHalfPi + 0.1 * (unif() - 0.5), x0 + cx * kG + 0.05 * (unif() - 0.5),
                    y0 + cy * kG + 0.05 * (unif() - 0.5), 0.05 * (unif() - 0.5));
        q[j] = shape == 3 ? 1000 : (rnd64() % 4 ? 1 + rnd64() % (1ULL << 40) : 0);
        if (shape == 4) q[j] = 0;
        for (int c = 0; c < C; c++) {
          counts[(size_t)j * C + c] = (int32_t)(rnd64() % 700);
          sums[(size_t)j * C + c] = (long long)counts[(size_t)j * C + c] * (long long)(20000 + rnd64() % 70000);
        }
      }
      int best = -1;
      if (shape != 4) {
        q[N / 2] = 1ULL << 40;
        uint64_t bq = 0;
        int bj = 0x7fffffff;
        for (int j = 0; j < N; j++)
          if (mc::heavier(q[j], j, bq, bj)) { bq = q[j]; bj = j; }
        best = bj;
      }
      for (int max_modes : {8, 3, 1}) {
        mc::Modes o;
        mc::modes_seq(T.data(), q.data(), sums.data(), counts.data(), N, C, best, kG, max_modes, &o);
        if (shape == 4) {
          CHECK(o.n_modes == 0 && o.n_cells == 0 && o.weight_sum == 0 && o.mode[0].best == -1);
          continue;
        }
        std::map<int32_t, uint64_t> W;
        std::map<int32_t, int> cnt;
        uint64_t S = 0;
        for (int j = 0; j < N; j++) {
          if (!q[j]) continue;
          const int32_t b = mc::cell_key(T[j], T[best], kG, &ix, &iy, &k);
          W[b] += q[j];
          cnt[b]++;
          S += q[j];
        }
        const uint64_t Wout = W.count(mc::kModeBins) ? W[mc::kModeBins] : 0;
        const int nout = cnt.count(mc::kModeBins) ? cnt[mc::kModeBins] : 0;
        W.erase(mc::kModeBins);
        std::vector<std::pair<uint64_t, int32_t>> order;
        for (auto& e : W) order.push_back({e.second, e.first});
        std::sort(order.begin(), order.end(), [](auto& a, auto& b) { return a.first > b.first || (a.first == b.first && a.second < b.second); });
        CHECK(o.weight_sum == S && o.outside_weight == Wout && o.n_outside == nout && o.n_cells == (int)order.size());
        CHECK(o.n_modes == std::min<int>(max_modes, (int)order.size()));
        if (shape == 1) CHECK(o.n_modes == 1 && o.mode[0].weight == S && o.mode[0].share == 1.0);
        if (shape == 2) CHECK(o.n_modes == 1 && o.n_outside + o.mode[0].n == (int)std::count_if(q.begin(), q.end(), [](uint64_t v) { return v > 0; }));
        for (int m = 0; m < mc::kMaxModes; m++) {
          const mc::Mode& r = o.mode[m];
          if (m >= o.n_modes) {
            CHECK(r.best == -1 && r.n == 0 && r.weight == 0);
            continue;
          }
          CHECK(mc::cell_bin(r.ix, r.iy, r.yaw_quadrant) == order[m].second && r.weight == order[m].first);
          CHECK(r.n == cnt[order[m].second] && r.best >= 0 && r.best < N && q[r.best] > 0);
          CHECK(mc::cell_key(T[r.best], T[best], kG, &ix, &iy, &k) == order[m].second);
          for (int j = 0; j < N; j++)
            if (q[j] && mc::cell_key(T[j], T[best], kG, &ix, &iy, &k) == order[m].second)
              CHECK(!mc::heavier(q[j], j, q[r.best], r.best));
          CHECK(r.share > 0 && r.share <= 1.0);
          for (int i = 0; i < 36; i++) CHECK(std::isfinite(r.covariance[i]) && r.covariance[i] == r.covariance[(i % 6) * 6 + i / 6]);
          for (int i = 0; i < 6; i++) CHECK(r.covariance[i * 7] >= 0.0);
          // the mean lies in the cell's neighbourhood of its heaviest particle
          CHECK(std::fabs(r.T_w_b[3] - T[r.best].t[0]) < kG && std::fabs(r.T_w_b[7] - T[r.best].t[1]) < kG);
          if (r.n == 1) {
            for (int i = 0; i < 3; i++) CHECK(r.T_w_b[4 * i + 3] == T[r.best].t[i]);
            for (int i = 0; i < 36; i++) CHECK(r.covariance[i] == 0.0);
          }
        }
      }
    }
  }
  if (g_fail) {
    std::printf("mclmodescheck: %d case(s) failed\n", g_fail);
    return 1;
  }
  std::printf("mclmodescheck ok\n");
  return 0;
}
