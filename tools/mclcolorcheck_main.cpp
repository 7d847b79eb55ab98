// Stand-alone check of the rules of the Monte Carlo localization colour
// evidence (mantis_amd/csrc/mk_mcl_color.h: the window sum with its
// out-of-buffer rows, the (csum, cn) of a pose, the pooled colour error, the
// charge and the fold into the log-weight) on small synthetic buffers that are
// allocated at exactly their size, as a program of its own so that it can be
// built with sanitizers and run directly:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o build/mclcolorcheck tools/mclcolorcheck_main.cpp && build/mclcolorcheck
// Exit status 0 and "mclcolorcheck ok" when every case holds.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../mantis_amd/csrc/mk_mcl_color.h"

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

// the window sum restated pixel by pixel over (x, y) pairs with the row wrap made explicit
static long long window_ref(const std::vector<uint8_t>& img, int W, int H, double u, double v) {
  long long s = 0;
  for (int oy = -5; oy < 5; oy++)
    for (int ox = -5; ox < 5; ox++) {
      const long long x = (long long)std::nearbyint(u + (double)ox), y = (long long)std::nearbyint(v + (double)oy);
      const long long lin = y * W + x;
      int b = 0, g = 0, r = 0;
      if (lin >= 0 && lin < (long long)W * H) {
        b = img[(size_t)(3 * lin)];
        g = img[(size_t)(3 * lin + 1)];
        r = img[(size_t)(3 * lin + 2)];
      }
      s += (b - 50) * (b - 50) + (g - 255) * (g - 255) + (r - 85) * (r - 85);
    }
  return s;
}

int main() {
  // window sums on buffers of exactly W x H x 3 bytes: inside, over every edge, over the start and the end
  const int sizes[][2] = {{23, 17}, {10, 10}, {7, 31}, {3, 3}, {64, 2}, {1, 40}};
  for (const auto& wh : sizes) {
    const int W = wh[0], H = wh[1];
    std::vector<uint8_t> img((size_t)W * H * 3);
    for (auto& p : img) p = (uint8_t)rnd64();
    int over_start = 0, over_end = 0;
    for (int k = 0; k < 400; k++) {
      double u = unif() * (W + 16) - 8, v = unif() * (H + 16) - 8;
      if (k % 7 == 0) u = std::floor(u) + 0.5;  // ties round to even
      if (k % 11 == 0) v = std::floor(v) + 0.5;
      if (k == 1) { u = W - 0.01; v = H - 0.01; }  // in frame, the window runs past the last pixel
      if (k == 2) { u = 0.0; v = 0.01; }            // in frame, the window starts before the first pixel
      const long long ref = window_ref(img, W, H, u, v);
      CHECK((long long)mc::color_window_sum(img.data(), W, H, u, v) == ref);
      const long long lo = (long long)std::nearbyint(v - 5) * W + (long long)std::nearbyint(u - 5);
      const long long hi = (long long)std::nearbyint(v + 4) * W + (long long)std::nearbyint(u + 4);
      over_start += lo < 0 && hi >= 0;
      over_end += lo < (long long)W * H && hi >= (long long)W * H;
    }
    CHECK(over_start > 0 && over_end > 0);
  }
  {  // extremes: all GREEN costs 0, all outside costs 100 |GREEN|^2, the largest pixel error fits
    std::vector<uint8_t> g(20 * 20 * 3), w(12 * 12 * 3);
    for (size_t i = 0; i < g.size(); i += 3) { g[i] = 50; g[i + 1] = 255; g[i + 2] = 85; }
    for (size_t i = 0; i < w.size(); i += 3) { w[i] = 255; w[i + 1] = 0; w[i + 2] = 255; }
    CHECK(mc::color_window_sum(g.data(), 20, 20, 10.0, 10.0) == 0);
    CHECK(mc::color_window_sum(g.data(), 20, 20, 10.0, -40.0) == 100 * (50 * 50 + 255 * 255 + 85 * 85));
    CHECK(mc::color_window_sum(w.data(), 12, 12, 6.0, 6.0) == 100 * 135950);
  }

  // (csum, cn) of poses above a green row: the sum of the scored landmarks' windows, in any order
  {
    const int W = 96, H = 64, ng = 41;
    std::vector<uint8_t> img((size_t)W * H * 3);
    for (auto& p : img) p = (uint8_t)rnd64();
    std::vector<double> green(3 * ng);
    for (int l = 0; l < ng; l++) { green[3 * l] = -1.2 + 0.06 * l; green[3 * l + 1] = 0.6; green[3 * l + 2] = 0.0; }
    const mk::Cam cm{60.0, 60.0, 48.0, 32.0, {0.003, -0.01, 0.0056, -0.002}};
    int seen_none = 0, seen_some = 0, seen_all = 0;
    for (int k = 0; k < 200; k++) {
      // a camera looking down (x right, y down, z = -Z_world) from (cx, cy, h), yawed; every fifth one under the floor
      const double yaw = unif() * 6.283, cx = unif() * 2 - 1, cy = unif() * 2 - 1, h = k % 5 == 4 ? -1.0 : 0.3 + unif() * 2;
      const double c = std::cos(yaw), s = std::sin(yaw);
      mk::Xf T;  // world -> camera: R = (Rz(yaw) * diag(1, -1, -1))^T, t = -R * pos
      const double Rwc[9] = {c, s, 0, s, -c, 0, 0, 0, -1};
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) T.R[3 * i + j] = Rwc[3 * j + i];
      const double pos[3] = {cx, cy, h};
      for (int i = 0; i < 3; i++) T.t[i] = -(T.R[3 * i] * pos[0] + T.R[3 * i + 1] * pos[1] + T.R[3 * i + 2] * pos[2]);
      long long cs;
      int32_t cn;
      mc::color_sums(T, green.data(), ng, cm, img.data(), W, H, &cs, &cn);
      long long ref = 0;
      int32_t nref = 0;
      for (int l = ng - 1; l >= 0; l--) {  // the other order
        double rp[3], u, v;
        mk::xf_apply(T, &green[3 * l], rp);
        if (!(rp[2] > 0)) continue;
        mk::distort(cm, rp[0], rp[1], rp[2], &u, &v);
        if (!mk::in_frame(u, v, H, W)) continue;
        ref += window_ref(img, W, H, u, v);
        nref++;
      }
      CHECK(cs == ref && cn == nref);
      seen_none += cn == 0;
      seen_some += cn > 0 && cn < ng;
      seen_all += cn == ng;
    }
    CHECK(seen_none > 0 && seen_some > 0);
    long long cs = -1;
    int32_t cn = -1;
    mk::Xf I{};
    I.R[0] = I.R[4] = I.R[8] = 1.0;
    mc::color_sums(I, green.data(), 0, cm, img.data(), W, H, &cs, &cn);  // a map without green landmarks
    CHECK(cs == 0 && cn == 0);
  }

  // pooling and the two charges
  {
    const long long big = 37LL * 100 * 195075;
    for (int C = 1; C <= 8; C++)
      for (int k = 0; k < 200; k++) {
        long long s[8];
        int32_t n[8];
        long long S = 0;
        int32_t Nn = 0;
        for (int c = 0; c < C; c++) {
          n[c] = rnd64() % 3 ? (int32_t)(rnd64() % 38) : 0;
          s[c] = k == 0 ? (n[c] = 37, big) : (long long)(unif() * 100 * 195075) * n[c];
          S += s[c];
          Nn += n[c];
        }
        for (int minc : {1, 10, 60}) {
          int32_t got_n = -1;
          const double Ec = mc::color_pool(s, n, C, minc, &got_n);
          CHECK(got_n == Nn);
          if (Nn >= minc && Nn > 0) CHECK(Ec == (double)S / ((double)Nn * 100.0 * 1.1));
          else CHECK(Ec == DBL_MAX);
          const double ch = mc::color_charge(Ec, 9000.0, 2500.0);
          CHECK(ch == (Ec == DBL_MAX ? 9000.0 / 2500.0 : Ec / 2500.0) && std::isfinite(ch) && ch >= 0);
        }
      }
    CHECK(mc::color_charge(DBL_MAX, 0.0, 7.0) == 0.0);
  }

  // the fold: (L - E / tau) - charge in that order; validity by the WHITE counts alone; a zero charge changes nothing
  {
    int order_seen = 0;
    for (int k = 0; k < 4096; k++) {
      const double L = -unif() * 50, E = k % 17 == 0 ? DBL_MAX : 5000 + unif() * 145000, ch = unif() * 9, tau = 63478.0;
      const int32_t n = (int32_t)(rnd64() % 40);
      const double got = mc::log_weight_color(L, E, n, 10, tau, ch);
      if (E == DBL_MAX || n < 10) {
        CHECK(got == -INFINITY);
        continue;
      }
      const double a = L - E / tau;
      CHECK(got == a - ch);
      order_seen += got != L - (E / tau + ch);
      CHECK(mc::log_weight_color(L, E, n, 10, tau, 0.0) == mc::log_weight(L, E, n, 10, tau));
    }
    CHECK(order_seen > 0);
  }

  if (g_fail) {
    std::printf("mclcolorcheck: %d case(s) failed\n", g_fail);
    return 1;
  }
  std::printf("mclcolorcheck ok\n");
  return 0;
}
