// Stand-alone check of the fixed-lag window's rule (mantis_amd/csrc/mk_smooth.h:
// schur0, marginalize, marginal_prior, prior_whitener, predict_start) on
// buffers allocated at exactly their size: the Schur complement against the
// elimination of view 0 from a whole two-view system, the symmetry of Lambda
// and Cov_p, the whitener, the prior factor at T_p, every numeric drop reason
// and the predicted start. A program of its own, so that it can be built with
// sanitizers and run directly on the CPU:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o build/lagcheck tools/lagcheck_main.cpp && build/lagcheck
// (make lagcheck). Exit status 0 and "lagcheck ok" when every case holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../mantis_amd/csrc/mk_smooth.h"

namespace sm = mk::smooth;

static int g_fail = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      g_fail++;                                                      \
    }                                                                \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
static double unif() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (double)(g_rng >> 11) / 9007199254740992.0 - 0.5;
}
// a heap array of exactly n doubles (the sanitizer sees every step past it)
static std::unique_ptr<double[]> arr(size_t n) { return std::unique_ptr<double[]>(new double[n]()); }

static void pose_of(const double* t, const double* phi, double* T) {
  for (int e = 0; e < 16; e++) T[e] = e % 5 == 0 ? 1.0 : 0.0;
  const double x[6] = {t[0], t[1], t[2], phi[0], phi[1], phi[2]};
  mk::calib::right_update(T, x);
}

// a random two-view system: acc (2 x 28), one factor, optionally a prior term
struct Sys {
  std::unique_ptr<double[]> acc = arr(56), fe = arr(6), fJ = arr(72), pe = arr(6), pJ = arr(36);
  int32_t has[1] = {1};
  int has_prior = 0;
};
static void fill(Sys& S, int has_prior) {
  S.has_prior = has_prior;
  for (int k = 0; k < 2; k++) {
    double M[12][6];
    for (auto& r : M)
      for (double& v : r) v = 2 * unif();
    int m = 0;
    for (int i = 0; i < 6; i++)
      for (int j = i; j < 6; j++) {
        double s = 0;
        for (int r = 0; r < 12; r++) s += M[r][i] * M[r][j];
        S.acc[28 * k + m++] = s;
      }
    for (int i = 0; i < 6; i++) S.acc[28 * k + 21 + i] = unif();
  }
  for (int i = 0; i < 6; i++) S.fe[i] = 0.2 * unif();
  for (int i = 0; i < 72; i++) S.fJ[i] = 2 * unif();
  for (int i = 0; i < 6; i++) S.pe[i] = has_prior ? unif() : 0.0;
  for (int i = 0; i < 36; i++) S.pJ[i] = has_prior ? 2 * unif() : 0.0;
}

static void check_schur_and_prior() {
  for (int rep = 0; rep < 16; rep++) {
    Sys S;
    fill(S, rep & 1);
    auto Hd = arr(72), Ho = arr(72), g = arr(12), Ld = arr(72), Lo = arr(72), x = arr(12);
    for (int k = 0; k < 2; k++)
      sm::assemble(k, 2, &S.acc[28 * k], S.has, S.fe.get(), S.fJ.get(), S.has_prior, S.pe.get(), S.pJ.get(), 0.0, &Hd[36 * k],
                   &Ho[36 * k], &g[6 * k]);
    CHECK(sm::solve(2, Hd.get(), Ho.get(), g.get(), S.has, Ld.get(), Lo.get(), x.get()) == -1);
    auto Lam = arr(36), eta = arr(6);
    CHECK(sm::schur0(Hd.get(), g.get(), S.fJ.get(), &S.fJ[36], S.fe.get(), Lam.get(), eta.get()) == sm::kLagKept);
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) CHECK(Lam[6 * i + j] == Lam[6 * j + i]);
    // view 1 alone: A_1 + Lambda, b_1 + eta, against x_1 of the whole system
    auto H1 = arr(36), g1 = arr(6), L1 = arr(36), x1 = arr(6);
    int32_t none[1] = {0};
    auto Ho1 = arr(36);
    sm::assemble(0, 1, &S.acc[28], none, nullptr, nullptr, 0, nullptr, nullptr, 0.0, H1.get(), Ho1.get(), g1.get());
    for (int e = 0; e < 36; e++) H1[e] += Lam[e];
    for (int i = 0; i < 6; i++) g1[i] = -(g1[i] + eta[i]);
    CHECK(mk::calib::chol6(H1.get(), L1.get()));
    mk::calib::chol6_solve(L1.get(), g1.get(), 1, x1.get(), 1);
    for (int i = 0; i < 6; i++) CHECK(std::fabs(x1[i] - x[6 + i]) <= 1e-9 * (1 + std::fabs(x[6 + i])));

    const double t[3] = {unif(), unif(), 1 + unif()}, phi[3] = {unif(), unif(), 2 * unif()};
    auto T1 = arr(16), Tp = arr(16), Cov = arr(36), Wp = arr(36);
    pose_of(t, phi, T1.get());
    const double sr = 0.00127;
    CHECK(sm::marginal_prior(Hd.get(), g.get(), S.fJ.get(), &S.fJ[36], S.fe.get(), T1.get(), sr, Tp.get(), Cov.get(),
                             Wp.get()) == sm::kLagKept);
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) CHECK(Cov[6 * i + j] == Cov[6 * j + i]);
    // W^T W Cov = sigma_row^2 I
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) {
        double s = 0;
        for (int a = 0; a < 6; a++)
          for (int b = 0; b < 6; b++) s += Wp[6 * a + i] * Wp[6 * a + b] * Cov[6 * b + j];
        CHECK(std::fabs(s / (sr * sr) - (i == j ? 1.0 : 0.0)) <= 1e-8);
      }
    // the prior factor at T_p itself is zero and its Jacobian is the whitener times diag(R_p, I)
    auto e = arr(6), J = arr(36);
    sm::prior(Tp.get(), Tp.get(), Wp.get(), e.get(), J.get());
    for (int i = 0; i < 6; i++) CHECK(std::fabs(e[i]) <= 1e-9);
  }
}

static void check_drops() {
  auto I6 = arr(36), z = arr(6), H = arr(36), Jb = arr(36), T1 = arr(16), Tp = arr(16), Cov = arr(36), Wp = arr(36);
  for (int i = 0; i < 6; i++) I6[7 * i] = 1.0;
  for (int e = 0; e < 16; e++) T1[e] = e % 5 == 0 ? 1.0 : 0.0;
  const double sr = 0.00127;
  for (int e = 0; e < 36; e++) H[e] = -I6[e];
  CHECK(sm::marginal_prior(H.get(), z.get(), I6.get(), I6.get(), z.get(), T1.get(), sr, Tp.get(), Cov.get(), Wp.get()) ==
        sm::kLagH00);
  for (int e = 0; e < 36; e++) H[e] = NAN;
  CHECK(sm::marginal_prior(H.get(), z.get(), I6.get(), I6.get(), z.get(), T1.get(), sr, Tp.get(), Cov.get(), Wp.get()) ==
        sm::kLagH00);
  for (int e = 0; e < 36; e++) H[e] = 0.5 * I6[e];
  CHECK(sm::marginal_prior(H.get(), z.get(), I6.get(), I6.get(), z.get(), T1.get(), sr, Tp.get(), Cov.get(), Wp.get()) ==
        sm::kLagLambda);
  for (int e = 0; e < 36; e++) {
    H[e] = 2.0 * I6[e];
    Jb[e] = 1e-160 * I6[e];
  }
  CHECK(sm::marginal_prior(H.get(), z.get(), I6.get(), Jb.get(), z.get(), T1.get(), sr, Tp.get(), Cov.get(), Wp.get()) ==
        sm::kLagCov);
  for (int e = 0; e < 36; e++) CHECK(Cov[e] == 0.0 && Wp[e] == 0.0);
  for (int e = 0; e < 16; e++) CHECK(Tp[e] == (e % 5 == 0 ? 1.0 : 0.0));
  CHECK(sm::marginal_prior(H.get(), z.get(), I6.get(), I6.get(), z.get(), T1.get(), sr, Tp.get(), Cov.get(), Wp.get()) ==
        sm::kLagKept);
  for (int i = 0; i < 6; i++) CHECK(std::fabs(Cov[7 * i] / (2 * sr * sr) - 1.0) < 1e-14);
  auto bad = arr(36);
  bad[0] = INFINITY;
  CHECK(!sm::prior_whitener(bad.get(), sr, Wp.get()));
}

static void check_predict() {
  const double t[3] = {0.3, -0.2, 1.4}, phi[3] = {0.02, -0.03, 0.4}, dt[3] = {0.08, 0, 0}, dphi[3] = {0, 0, 0.05};
  auto T = arr(16), D = arr(16), P = arr(16);
  pose_of(t, phi, T.get());
  pose_of(dt, dphi, D.get());
  sm::predict_start(T.get(), D.get(), P.get());
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      double s = 0;
      for (int k = 0; k < 4; k++) s += T[4 * i + k] * D[4 * k + j];
      CHECK(std::fabs(P[4 * i + j] - s) <= 1e-15);
    }
}

int main() {
  check_schur_and_prior();
  check_drops();
  check_predict();
  if (g_fail) {
    std::printf("lagcheck: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("lagcheck ok\n");
  return 0;
}
