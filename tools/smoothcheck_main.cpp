// Stand-alone check of the window smoother's rules (mantis_amd/csrc/
// mk_smooth.h: log_so3 and J_r^-1 at and around their small-angle switch, the
// between and prior factors, the block Cholesky with buffers of exactly N
// blocks for N = 1, 2, 3 and a broken chain, the marginals, a blind view, a
// starved window, a singular block, and one whole call on frames allocated at
// exactly their size) as a program of its own so that it can be built with
// sanitizers and run directly on the CPU:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o build/smoothcheck tools/smoothcheck_main.cpp && build/smoothcheck
// Exit status 0 and "smoothcheck ok" when every case holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../mantis_amd/csrc/mk_smooth.h"

namespace rf = mk::refine;
namespace sm = mk::smooth;

static int g_fail = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      g_fail++;                                                      \
    }                                                                \
  } while (0)

static uint64_t g_rng = 0x2545F4914F6CDD1DULL;
static double unif() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (double)(g_rng >> 11) / 9007199254740992.0;
}

// T = [Exp(phi) | t] through the library's own update of the identity
static void pose_of(const double* t, const double* phi, double* T) {
  for (int e = 0; e < 16; e++) T[e] = e % 5 == 0 ? 1.0 : 0.0;
  const double x[6] = {t[0], t[1], t[2], phi[0], phi[1], phi[2]};
  mk::calib::right_update(T, x);
}
static void mul4(const double* A, const double* B, double* o) {
  double r[16];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      double s = 0;
      for (int k = 0; k < 4; k++) s += A[4 * i + k] * B[4 * k + j];
      r[4 * i + j] = s;
    }
  std::memcpy(o, r, sizeof(r));
}
// a camera looking straight down from (x, y, h), yawed by a (the camera is the base)
static void nadir_pose(double x, double y, double h, double a, double* T) {
  const double c = std::cos(a), s = std::sin(a);
  const double R[9] = {c, s, 0, s, -c, 0, 0, 0, -1};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) T[4 * i + j] = R[3 * i + j];
  T[3] = x; T[7] = y; T[11] = h;
  T[12] = T[13] = T[14] = 0; T[15] = 1;
}

static void check_small_angles() {
  const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  double phi[3], J[9];
  sm::log_so3(I3, phi);
  CHECK(phi[0] == 0 && phi[1] == 0 && phi[2] == 0);
  sm::jr_inv(phi, J);
  for (int e = 0; e < 9; e++) CHECK(J[e] == I3[e]);
  const double ax[3] = {0.6, -0.64, 0.48};
  for (double th : {0.0, 0.9999e-8, 1.0001e-8, 1e-6, 0.5, 3.0}) {
    const double p[3] = {th * ax[0], th * ax[1], th * ax[2]}, z[3] = {0, 0, 0};
    double T[16], R[9], tt[3], back[3];
    pose_of(z, p, T);
    sm::rt_of(T, R, tt);
    sm::log_so3(R, back);
    for (int i = 0; i < 3; i++) CHECK(std::fabs(back[i] - p[i]) <= 1e-15 + 1e-14 * th);
    sm::jr_inv(p, J);
    for (int e = 0; e < 9; e++) CHECK(std::isfinite(J[e]) && std::fabs(J[e] - I3[e]) <= 0.6 * th + 0.1 * th * th);
  }
  // a half turn: the axis from R + I
  const double Rz[9] = {-1, 0, 0, 0, -1, 0, 0, 0, 1};
  sm::log_so3(Rz, phi);
  CHECK(std::fabs(std::fabs(phi[2]) - M_PI) < 1e-12 && phi[0] == 0 && phi[1] == 0);
}

static void check_factors() {
  for (int trial = 0; trial < 20; trial++) {
    const double t0[3] = {unif() - 0.5, unif() - 0.5, 1 + unif()}, p0[3] = {0.1 * unif(), 0.1 * unif(), 6 * unif()};
    const double td[3] = {0.08, 0.01 * unif(), 0}, pd[3] = {0, 0, 0.05}, z[3] = {0, 0, 0};
    double Tk[16], D[16], Tn[16], e[6], Ja[36], Jb[36];
    pose_of(t0, p0, Tk);
    pose_of(td, pd, D);
    mul4(Tk, D, Tn);
    sm::between(Tk, Tn, D, 1.0, 1.0, e, Ja, Jb);
    for (int i = 0; i < 6; i++) CHECK(std::fabs(e[i]) < 1e-14);
    // a step dx on view k + 1 moves e by Jb dx to first order
    double dx[6], Tn2[16], e2[6];
    for (int i = 0; i < 6; i++) dx[i] = 1e-6 * (unif() - 0.5);
    std::memcpy(Tn2, Tn, sizeof(Tn));
    mk::calib::right_update(Tn2, dx);
    sm::between(Tk, Tn2, D, 1.0, 1.0, e2, Ja, Jb);
    for (int i = 0; i < 6; i++) {
      double s = 0;
      for (int j = 0; j < 6; j++) s += Jb[6 * i + j] * dx[j];
      CHECK(std::fabs(e2[i] - s) < 1e-11);
    }
    double cov[36] = {0}, Wp[36], pe[6], pJ[36];
    for (int i = 0; i < 6; i++) cov[7 * i] = 1e-4 * (1 + i);
    cov[1] = cov[6] = 2e-5;
    CHECK(sm::prior_whitener(cov, 0.5, Wp));
    sm::prior(Tn2, Tn, Wp, pe, pJ);
    for (int i = 0; i < 6; i++) CHECK(std::isfinite(pe[i]));
    (void)z;
  }
  double bad[36] = {0}, Wp[36];
  CHECK(!sm::prior_whitener(bad, 1.0, Wp));
  for (int i = 0; i < 6; i++) bad[7 * i] = 1.0;
  bad[35] = NAN;
  CHECK(!sm::prior_whitener(bad, 1.0, Wp));
}

// random PD blocks with factors, buffers of exactly N blocks; the solution checked by H x + g = 0
static void check_solve(int N, int broken) {
  std::vector<double> acc(28 * (size_t)N), fe(6 * (size_t)(N - 1)), fJ(72 * (size_t)(N - 1));
  std::vector<int32_t> has(N - 1);
  for (int k = 0; k < N; k++) {
    double a[28] = {0};
    for (int r = 0; r < 30; r++) {
      double v[7];
      for (int c = 0; c < 7; c++) v[c] = (unif() - 0.5) * (c == 6 ? 0.01 : 2.0);
      rf::accumulate_row(v, a);
    }
    std::memcpy(&acc[28 * (size_t)k], a, sizeof(a));
  }
  for (int k = 0; k < N - 1; k++) {
    has[k] = k != broken;
    for (int q = 0; q < 6; q++) fe[6 * (size_t)k + q] = has[k] ? 0.01 * (unif() - 0.5) : 0.0;
    for (int q = 0; q < 72; q++) fJ[72 * (size_t)k + q] = has[k] ? unif() - 0.5 : 0.0;
  }
  std::vector<double> Hd(36 * (size_t)N), Ho(36 * (size_t)N), g(6 * (size_t)N), Ld(36 * (size_t)N), Lo(36 * (size_t)N),
      x(6 * (size_t)N), S(36 * (size_t)N);
  double pe[6] = {0}, pJ[36] = {0};
  for (int k = 0; k < N; k++)
    sm::assemble(k, N, &acc[28 * (size_t)k], has.data(), fe.data(), fJ.data(), 0, pe, pJ, 1e-6, &Hd[36 * (size_t)k],
                 &Ho[36 * (size_t)k], &g[6 * (size_t)k]);
  CHECK(sm::solve(N, Hd.data(), Ho.data(), g.data(), has.data(), Ld.data(), Lo.data(), x.data()) == -1);
  double worst = 0;
  for (int k = 0; k < N; k++)
    for (int i = 0; i < 6; i++) {
      double s = g[6 * (size_t)k + i];
      for (int j = 0; j < 6; j++) {
        s += Hd[36 * (size_t)k + 6 * i + j] * x[6 * (size_t)k + j];
        if (k > 0) s += Ho[36 * (size_t)(k - 1) + 6 * i + j] * x[6 * (size_t)(k - 1) + j];
        if (k < N - 1) s += Ho[36 * (size_t)k + 6 * j + i] * x[6 * (size_t)(k + 1) + j];
      }
      worst = std::fmax(worst, std::fabs(s));
    }
  std::printf("solve N=%d broken=%d: |H x + g| %.3g\n", N, broken, worst);
  CHECK(worst < 1e-12);
  sm::marginals(N, Ld.data(), Lo.data(), has.data(), S.data());
  for (int k = 0; k < N; k++)
    for (int i = 0; i < 6; i++) CHECK(S[36 * (size_t)k + 7 * i] > 0);
  // a diagonal block that is not PD is named
  for (int i = 0; i < 36; i++) Hd[36 * (size_t)(N - 1) + i] = 0.0;
  CHECK(sm::solve(N, Hd.data(), Ho.data(), g.data(), has.data(), Ld.data(), Lo.data(), x.data()) == N - 1);
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

// whole calls on painted grids: N = 1, 2, 3, a blind view, a broken chain, I = 0, starved, singular
static void check_seq() {
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
  CHECK(nc > 40);
  mk::GnCam gc;
  const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  rf::gncam_from(I4, gc);
  const int NV = 3;
  const double td[3] = {0.02, 0.005, 0.0}, pd[3] = {0, 0, 0.04};
  double D[2 * 16], Tt[NV][16], T0[NV * 16];
  pose_of(td, pd, D);
  std::memcpy(D + 16, D, sizeof(double) * 16);
  nadir_pose(0.0, -0.01, 0.6, 0.2, Tt[0]);
  for (int k = 1; k < NV; k++) mul4(Tt[k - 1], D, Tt[k]);
  std::vector<std::vector<uint8_t>> img(NV, std::vector<uint8_t>((size_t)W * H * 3, 0));  // exactly their size
  for (int k = 0; k < NV; k++) paint_grid(img[k], W, H, Tt[k], cam, 2 * pitch, 2, 4 * pitch);
  const double off[3] = {0.004, -0.003, 0.0}, offr[3] = {0, 0, 0.004};
  double Off[16];
  pose_of(off, offr, Off);
  for (int k = 0; k < NV; k++) mul4(Tt[k], Off, T0 + 16 * k);
  std::vector<uint8_t> black((size_t)W * H * 3, 0);
  mantis_smooth_params p{};
  p.struct_size = sizeof(p);
  p.iterations = 4; p.half_window = 12; p.white_thresh = 12288; p.min_weight = 12288; p.min_obs = 12;
  p.landmark_pitch = pitch * 0.5;
  p.sigma_row = 0.00127; p.sigma_t = 0.01; p.sigma_rot = 0.03;
  mantis_smooth_result R;
  std::vector<mantis_smooth_view> V(NV);
  std::vector<sm::PassRecord> rec;
  const int32_t both[2] = {1, 1}, none[2] = {0, 0}, first[2] = {1, 0};
  for (int N = 1; N <= NV; N++) {
    const uint8_t* fr[NV] = {img[0].data(), img[1].data(), img[2].data()};
    sm::smooth_seq(N, T0, D, both, 0, nullptr, nullptr, &gc, &cam, fr, 1, W, H, X.data(), n, 0, cand.data(), nc, p, R,
                   V.data(), &rec);
    std::printf("seq N=%d: status %d smoothed %d runs %d n_obs %d factors %d dof %d motion_rms %.4f\n", N, R.status,
                R.smoothed, R.iterations_run, R.n_obs[R.iterations_run], R.n_factors, R.dof, R.motion_rms[R.iterations_run]);
    CHECK(R.status == sm::kOk && R.iterations_run == 4 && R.n_factors == N - 1 && R.smoothed == 1);
    CHECK((int)rec.size() == 5);
    for (int k = 0; k < N; k++) {
      const double d0 = std::hypot(T0[16 * k + 3] - Tt[k][3], T0[16 * k + 7] - Tt[k][7]);
      const double d1 = std::hypot(V[k].T_w_b[3] - Tt[k][3], V[k].T_w_b[7] - Tt[k][7]);
      CHECK(d1 < d0);
      for (int i = 0; i < 6; i++) CHECK(V[k].covariance[7 * i] > 0);
    }
  }
  {  // a blind middle view: held by its factors
    const uint8_t* fr[NV] = {img[0].data(), black.data(), img[2].data()};
    sm::smooth_seq(3, T0, D, both, 0, nullptr, nullptr, &gc, &cam, fr, 1, W, H, X.data(), n, 0, cand.data(), nc, p, R,
                   V.data(), nullptr);
    const double d0 = std::hypot(T0[16 + 3] - Tt[1][3], T0[16 + 7] - Tt[1][7]);
    const double d1 = std::hypot(V[1].T_w_b[3] - Tt[1][3], V[1].T_w_b[7] - Tt[1][7]);
    std::printf("blind view: %.5f -> %.5f m, n_obs %d\n", d0, d1, V[1].n_obs);
    CHECK(R.status == sm::kOk && R.smoothed == 1 && V[1].n_obs == 0 && d1 < 0.25 * d0);
  }
  {  // a broken chain: step 1 unset, and a prior on view 0
    const uint8_t* fr[NV] = {img[0].data(), img[1].data(), img[2].data()};
    double cov[36] = {0}, Wp[36];
    for (int i = 0; i < 6; i++) cov[7 * i] = 1e-4;
    CHECK(sm::prior_whitener(cov, p.sigma_row, Wp));
    sm::smooth_seq(3, T0, D, first, 1, Tt[0], Wp, &gc, &cam, fr, 1, W, H, X.data(), n, 0, cand.data(), nc, p, R, V.data(),
                   &rec);
    CHECK(R.status == sm::kOk && R.n_factors == 1 && R.has_prior == 1 && R.smoothed == 1);
    CHECK(R.dof == R.n_obs[4] + 6 + 6 - 18);
    for (int q = 0; q < 72; q++) CHECK(rec[0].J[72 + q] == 0.0);
    // I = 0: the poses come back bit for bit
    mantis_smooth_params p0 = p;
    p0.iterations = 0;
    sm::smooth_seq(3, T0, D, both, 0, nullptr, nullptr, &gc, &cam, fr, 1, W, H, X.data(), n, 0, cand.data(), nc, p0, R,
                   V.data(), nullptr);
    for (int k = 0; k < 3; k++) CHECK(std::memcmp(V[k].T_w_b, T0 + 16 * k, sizeof(double) * 16) == 0);
    CHECK(R.iterations_run == 0 && R.status == sm::kOk);
  }
  {  // starved: every view black; singular: an all-blind segment at lambda = 0
    const uint8_t* fb[NV] = {black.data(), black.data(), black.data()};
    sm::smooth_seq(3, T0, D, both, 0, nullptr, nullptr, &gc, &cam, fb, 1, W, H, X.data(), n, 0, cand.data(), nc, p, R,
                   V.data(), nullptr);
    CHECK(R.status == sm::kStarved && R.smoothed == 0 && R.iterations_run == 0);
    for (int k = 0; k < 3; k++) CHECK(std::memcmp(V[k].T_w_b, T0 + 16 * k, sizeof(double) * 16) == 0);
    const uint8_t* fs[NV] = {img[0].data(), black.data(), black.data()};
    sm::smooth_seq(3, T0, D, none, 0, nullptr, nullptr, &gc, &cam, fs, 1, W, H, X.data(), n, 0, cand.data(), nc, p, R,
                   V.data(), nullptr);
    CHECK(R.status == sm::kSingular && R.smoothed == 0 && R.iterations_run == 0);
    for (int e = 0; e < 36; e++) CHECK(V[1].covariance[e] == 0.0);
  }
}

int main() {
  check_small_angles();
  check_factors();
  for (int N : {1, 2, 3}) check_solve(N, -1);
  check_solve(7, 3);
  check_seq();
  if (g_fail) {
    std::printf("smoothcheck: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("smoothcheck ok\n");
  return 0;
}
