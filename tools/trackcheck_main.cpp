// Stand-alone check of the rig-tracking rules (mantis_amd/csrc/mk_track.h:
// pool / error_of, pick, gate, particle) on the cases tests/test_track_host.py runs
// through the host helper library, as a program of its own so that it can be
// built with sanitizers and run directly:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o build/trackcheck tools/trackcheck_main.cpp && build/trackcheck
// Exit status 0 and "trackcheck ok" when every case holds.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../mantis_amd/csrc/mk_track.h"

namespace t = mk::track;

static int g_fail = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      g_fail++;                                                      \
    }                                                                \
  } while (0)

// the rules restated as plainly as the definition reads
static double ref_pool(const std::vector<long long>& s, const std::vector<int32_t>& n, int32_t* nout) {
  long long ss = 0, nn = 0;
  for (size_t c = 0; c < s.size(); c++) { ss += s[c]; nn += n[c]; }
  *nout = (int32_t)nn;
  return nn == 0 ? DBL_MAX : (double)ss / ((double)nn * 1.1);
}
static int ref_pick(const std::vector<double>& e, double cur) {
  size_t b = 0;
  for (size_t j = 1; j < e.size(); j++)
    if (e[j] < e[b]) b = j;
  return e[b] < cur ? (int)b : -1;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
static uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 16);
}

int main() {
  // pool: random sums over the shapes of the GPU tests, with blind cameras
  const int shapes[][2] = {{1, 1}, {7, 3}, {96, 1}, {64, 8}};
  for (const auto& sh : shapes) {
    for (int j = 0; j < sh[0]; j++) {
      std::vector<long long> s(sh[1]);
      std::vector<int32_t> n(sh[1]);
      for (int c = 0; c < sh[1]; c++) {
        n[c] = rnd() % 10 < 3 ? 0 : (int32_t)(rnd() % 769);
        s[c] = (long long)n[c] * (long long)(rnd() % (3 * 255 * 255 + 1));
      }
      int32_t a, b;
      const double e = t::pool(s.data(), n.data(), sh[1], &a), r = ref_pool(s, n, &b);
      CHECK(e == r && a == b);
      CHECK(sh[1] != 1 || t::error_of(s[0], n[0]) == e);  // one camera: the single scorers' error
    }
  }
  CHECK(t::error_of(0, 0) == DBL_MAX && t::error_of(5, 0) == DBL_MAX && t::error_of(0, 1) == 0.0);
  {  // all-blind cameras: DBL_MAX, no pick, not tracked
    std::vector<long long> s(4, 0);
    std::vector<int32_t> n(4, 0);
    int32_t np;
    const double e = t::pool(s.data(), n.data(), 4, &np);
    CHECK(e == DBL_MAX && np == 0);
    const double errs[3] = {DBL_MAX, DBL_MAX, DBL_MAX};
    CHECK(t::pick(errs, 3, DBL_MAX) == -1);
    CHECK(t::gate(DBL_MAX, 0, 0, 0.0) == 0);
    CHECK(t::gate(DBL_MAX, 100, 10, 0.0) == 0);
    s[1] = 123456;  // one seeing camera: its error alone
    n[1] = 40;
    CHECK(t::pool(s.data(), n.data(), 4, &np) == 123456.0 / (40.0 * 1.1) && np == 40);
  }
  {  // equal errors: the lowest index; equal to the current error: not accepted
    const double a[4] = {5.0, 3.0, 3.0, 4.0};
    CHECK(t::pick(a, 4, 10.0) == 1);
    std::vector<double> same(96, 3.0);
    CHECK(t::pick(same.data(), 96, 10.0) == 0);
    const double b[3] = {7.0, 3.0, 9.0};
    CHECK(t::pick(b, 3, 3.0) == -1);
    CHECK(t::pick(b, 3, std::nextafter(3.0, 4.0)) == 1);
    const double m[2] = {DBL_MAX, 2.0};
    CHECK(t::pick(m, 2, DBL_MAX) == 1);
    const int sizes[] = {1, 2, 63, 64, 65, 96};
    for (int n : sizes)
      for (int rep = 0; rep < 20; rep++) {
        std::vector<double> e(n);
        for (double& v : e) v = (double)(rnd() % 6);
        const double cur = (double)(rnd() % 6);
        CHECK(t::pick(e.data(), n, cur) == ref_pick(e, cur));
      }
  }
  // gate: n_proj one below / exactly at min_projections, max_error <= 0
  CHECK(t::gate(100.0, 9, 10, 0.0) == 0);
  CHECK(t::gate(100.0, 10, 10, 0.0) == 1);
  CHECK(t::gate(100.0, 10, 10, -1.0) == 1);
  CHECK(t::gate(100.0, 10, 10, 100.0) == 1);
  CHECK(t::gate(100.0, 10, 10, std::nextafter(100.0, 0.0)) == 0);
  CHECK(t::gate(0.0, 0, 0, 0.0) == 1);
  {  // particle: sigma 0 leaves the pose bit for bit; c2w inverts T * T_base_cam
    double T[16] = {0.36, -0.48, 0.8, 0.1, 0.8, 0.6, 0.0, -0.2, -0.48, 0.64, 0.6, 1.5, 0, 0, 0, 1};
    const float g[6] = {0.5f, -1.25f, 2.0f, -0.75f, 0.25f, 1.5f};
    const mk::Xf X = t::xf_from_mat4(T);
    const mk::Xf P0 = t::particle(X, g, 0.0, 0.0);
    for (int k = 0; k < 9; k++) CHECK(P0.R[k] == X.R[k]);
    for (int k = 0; k < 3; k++) CHECK(P0.t[k] == X.t[k]);
    const mk::Xf P = t::particle(X, g, 0.03, 0.01);
    const mk::Xf inv = t::cam_c2w(P, X), back = mk::xf_mul(inv, mk::xf_mul(P, X));
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) CHECK(std::fabs(back.R[i * 3 + j] - (i == j ? 1.0 : 0.0)) < 1e-12);
      CHECK(std::fabs(back.t[i]) < 1e-12);
    }
    double M[16];
    t::xf_to_mat4(P, M);
    const mk::Xf again = t::xf_from_mat4(M);
    for (int k = 0; k < 9; k++) CHECK(again.R[k] == P.R[k]);
    CHECK(M[12] == 0 && M[13] == 0 && M[14] == 0 && M[15] == 1);
  }
  if (g_fail) {
    std::printf("trackcheck: %d case(s) failed\n", g_fail);
    return 1;
  }
  std::printf("trackcheck ok\n");
  return 0;
}
