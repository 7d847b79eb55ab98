// Stand-alone check of the Monte Carlo localization rules
// (mantis_amd/csrc/mk_mcl.h: weights, integer scan, ancestors, estimate, the
// full step's bookkeeping) over random and degenerate inputs, as a program of
// its own so that it can be built with sanitizers and run directly:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o build/mclcheck tools/mclcheck_main.cpp && build/mclcheck
// Exit status 0 and "mclcheck ok" when every case holds.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../mantis_amd/csrc/mk_mcl.h"

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

// the ancestor rule as the definition reads, with the compiler's 128-bit integers
static int ref_ancestor(const std::vector<uint64_t>& cum, const std::vector<uint64_t>& q, uint32_t U, int i) {
  const int N = (int)cum.size();
  const unsigned __int128 S = cum[N - 1];
  int last = 0;
  for (int j = 0; j < N; j++)
    if (q[j] > 0) last = j;
  for (int j = 0; j < N; j++)
    if ((unsigned __int128)cum[j] * (unsigned)N * ((unsigned __int128)1 << 32) >
        ((unsigned __int128)U + ((unsigned __int128)i << 32)) * S)
      return j < last ? j : last;
  return last;
}

static mk::Xf pose(double spread) {
  const float g[6] = {(float)(unif() - 0.5), (float)(unif() - 0.5), (float)(unif() - 0.5),
                      (float)(unif() - 0.5), (float)(unif() - 0.5), (float)(unif() - 0.5)};
  const double T[16] = {0.36, -0.48, 0.8, 0.1, 0.8, 0.6, 0.0, -0.2, -0.48, 0.64, 0.6, 1.5, 0, 0, 0, 1};
  return mk::track::particle(mk::track::xf_from_mat4(T), g, spread, spread);
}

int main() {
  // the 128-bit product against the compiler's
  for (int k = 0; k < 20000; k++) {
    const uint64_t a = rnd64() >> (rnd64() % 64), b = rnd64() >> (rnd64() % 64);
    const mc::U128 p = mc::mul64(a, b);
    const unsigned __int128 r = (unsigned __int128)a * b;
    CHECK(p.lo == (uint64_t)r && p.hi == (uint64_t)(r >> 64));
  }
  CHECK(mc::past(4096ULL << 40, 4096, 0xffffffffu, 4095, 4096ULL << 40));  // c N = 2^64 exactly
  CHECK(mc::rng_next(0x0123456789ABCDEFULL) == 0x89ABCDEFULL * 4164903690ULL + 0x01234567ULL);

  // weights: the heaviest is 2^40 exactly, dropped particles are 0, no NaN at the extremes
  CHECK(mc::weight_q(-3.5, -3.5) == (1ULL << 40));
  CHECK(mc::weight_q(-INFINITY, 0.0) == 0 && mc::weight_q(-1e308, 0.0) == 0);
  CHECK(mc::log_weight(0.0, DBL_MAX, 100, 10, 1.0) == -INFINITY);
  CHECK(mc::log_weight(0.0, 5.0, 9, 10, 1.0) == -INFINITY && mc::log_weight(1.0, 5.0, 10, 10, 2.0) == -1.5);
  CHECK(mc::log_weight(0.0, 1e5, 10, 10, 1e-305) == -INFINITY);  // E / tau overflows: dropped, not NaN

  const int sizes[] = {1, 2, 7, 64, 65, 1025, 4096};
  const uint32_t draws[] = {0u, 1u, 0x80000000u, 0xffffffffu};
  for (int N : sizes) {
    for (int shape = 0; shape < 6; shape++) {
      std::vector<uint64_t> q(N), cum(N);
      for (int j = 0; j < N; j++) q[j] = 1 + rnd64() % (1ULL << 40);
      if (shape == 1) for (int j = 0; j < N / 3; j++) q[j] = 0;               // zeros first
      if (shape == 2) for (int j = N - N / 3; j < N; j++) q[j] = 0;           // zeros last
      if (shape == 3) for (int j = N / 3; j < 2 * N / 3; j++) q[j] = 0;       // zeros in the middle
      if (shape == 4) { for (auto& v : q) v = 0; q[N / 2] = 1ULL << 40; }    // one heavy particle
      if (shape == 5) for (auto& v : q) v = 1ULL << 40;                       // the largest sum
      uint64_t s = 0;
      int last = 0;
      for (int j = 0; j < N; j++) { s += q[j]; cum[j] = s; if (q[j]) last = j; }
      for (uint32_t U : draws)
        for (int i = 0; i < N; i += (N > 128 ? 37 : 1)) {
          const int a = mc::ancestor(cum.data(), N, U, i, last);
          CHECK(a == ref_ancestor(cum, q, U, i) && q[a] > 0);
          if (shape == 4) CHECK(a == N / 2);
        }
    }
  }

  // the full step on random and degenerate inputs
  for (int N : sizes) {
    for (int mode = 0; mode < 4; mode++) {  // 0 random, 1 one survivor, 2 nobody (lost), 3 identical poses
      const int C = 1 + (int)(rnd64() % 3);
      std::vector<long long> sums((size_t)N * C, 0);
      std::vector<int32_t> counts((size_t)N * C, 0);
      std::vector<mk::Xf> T(N), T0;
      std::vector<double> L(N), L0, E(N), Ln(N);
      std::vector<uint64_t> q(N), cum(N);
      std::vector<int32_t> anc(N);
      const mk::Xf same = pose(0.1);
      for (int j = 0; j < N; j++) {
        T[j] = mode == 3 ? same : pose(mode == 1 ? 3.0 : 0.05);
        L[j] = -5.0 * unif();
        const bool sees = mode == 0 || mode == 3 ? rnd64() % 4 != 0 : (mode == 1 && j == N / 2);
        for (int c = 0; c < C && sees; c++) {
          counts[(size_t)j * C + c] = 10 + (int32_t)(rnd64() % 700);
          sums[(size_t)j * C + c] = (long long)counts[(size_t)j * C + c] * (long long)(20000 + rnd64() % 70000);
        }
      }
      if (mode == 0 || mode == 3) { counts[0] = 500; sums[0] = 500LL * 30000; }
      T0 = T;
      L0 = L;
      const uint32_t U = (uint32_t)rnd64();
      const double frac = (rnd64() & 1) ? 2.0 : 0.0;
      const mc::Outcome o = mc::step_seq(sums.data(), counts.data(), N, C, T.data(), L.data(), 3000.0, frac, 10, U,
                                         q.data(), cum.data(), anc.data(), E.data(), Ln.data());
      if (mode == 2) {
        CHECK(o.lost == 1 && o.resampled == 0 && o.best == -1 && o.n_valid == 0);
        for (int j = 0; j < N; j++) CHECK(L[j] == L0[j] && q[j] == 0 && cum[j] == 0 && anc[j] == -1 && T[j].t[0] == T0[j].t[0]);
        continue;
      }
      CHECK(o.lost == 0 && o.best >= 0 && o.best < N && q[o.best] == (1ULL << 40));
      uint64_t s = 0;
      int nv = 0;
      for (int j = 0; j < N; j++) { s += q[j]; CHECK(cum[j] == s); nv += q[j] > 0; CHECK(q[j] <= q[o.best]); }
      CHECK(o.S == s && o.n_valid == nv && o.ess >= 1.0 - 1e-12 && o.ess <= nv + 1e-9);
      for (int k = 0; k < 36; k++) CHECK(std::isfinite(o.cov[k]) && o.cov[k] == o.cov[(k % 6) * 6 + k / 6]);
      for (int k = 0; k < 6; k++) CHECK(o.cov[k * 7] >= 0.0);
      if (mode == 1) {
        CHECK(o.n_valid == 1 && o.best == N / 2 && o.ess == 1.0);
        for (int k = 0; k < 9; k++) CHECK(o.mean.R[k] == T0[N / 2].R[k]);
        for (int k = 0; k < 3; k++) CHECK(o.mean.t[k] == T0[N / 2].t[k]);
        for (int k = 0; k < 36; k++) CHECK(o.cov[k] == 0.0);
      }
      if (mode == 3) {
        for (int k = 0; k < 36; k++) CHECK(o.cov[k] == 0.0);
        for (int k = 0; k < 3; k++) CHECK(o.mean.t[k] == same.t[k]);
      }
      CHECK(o.resampled == (frac == 2.0 ? 1 : 0));
      for (int i = 0; i < N; i++) {
        if (o.resampled) {
          CHECK(anc[i] >= 0 && anc[i] < N && q[anc[i]] > 0 && L[i] == 0.0 && (i == 0 || anc[i] >= anc[i - 1]));
          for (int k = 0; k < 3; k++) CHECK(T[i].t[k] == T0[anc[i]].t[k]);
        } else {
          CHECK(anc[i] == -1 && L[i] == Ln[i] && T[i].t[0] == T0[i].t[0]);
        }
      }
    }
  }
  if (g_fail) {
    std::printf("mclcheck: %d case(s) failed\n", g_fail);
    return 1;
  }
  std::printf("mclcheck ok\n");
  return 0;
}
