// Line refinement, robust rows (mantis_refine_set_robust, include/mantis.h):
// the step kernel of a pass when the context's switch is on. Included by
// refine_impl.hip after k_refine_step, which it replaces launch for launch:
// still 2 (I + 1) launches, every hand-off between blocks a kernel boundary.
// The rules -- key, scale, weight, the starved gate -- are in mk_refine.h
// (shared with the host build of the tests).
namespace mk {

struct RobustArgs {
  mantis_refine_robust_stats* stats;  // rigs
  uint32_t* keys;                     // [pass][rig][C n_cand], record only (else null)
  double* weights;                    // the same
  rfn::Robust rb;
};

constexpr int kRobustBins = 4096;   // two 12-bit digits of a 24-bit key
constexpr int kRobustChunk = 2048;  // rows whose sqrt(w) wait in LDS at a time: 16 trips of the MFMA loop
constexpr int kRobustKeys = 4096;   // slots whose key stays in LDS between the passes; later slots are read again
constexpr uint32_t kNoKey = 0xffffffffu;  // a rejected slot (keys are below 2^24)

// the key of slot r after the first pass: kept in LDS, or formed again from a slot past the kept ones
__device__ uint32_t robust_key_of(const rfn::Slot* sl, const uint32_t* kept, int r) {
  if (r < kRobustKeys) return kept[r];
  return sl[r].code == 0 ? rfn::robust_key(sl[r].Sw, sl[r].Skw) : kNoKey;
}

// The rank-`rank` entry of the block's histogram (rank < the sum of the bins):
// every thread sums its 16 consecutive bins, the sums are scanned over the
// block (shuffles inside a wave, the four wave totals through `wsum`), and the
// one thread whose bins hold the rank walks them. Every thread gets the bin
// and, in *rest, the rank inside that bin. wsum (4) and sel (2) are LDS words.
// Ends with the block in step behind a barrier, so the histogram may be
// cleared right after.
__device__ uint32_t robust_select(const uint32_t* hist, uint32_t rank, uint32_t* wsum, uint32_t* sel, uint32_t* rest) {
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  uint32_t own = 0;
#pragma unroll
  for (int b = 0; b < kRobustBins / 256; b++) own += hist[t * (kRobustBins / 256) + b];
  uint32_t inc = own;  // inclusive scan over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(inc, d, 64);
    if (lane >= d) inc += up;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t before = inc - own;
  for (int w = 0; w < wave; w++) before += wsum[w];
  if (rank >= before && rank < before + own) {  // exactly one thread: the bins partition the ranks
    uint32_t left = rank - before;
    int b = t * (kRobustBins / 256);
    while (left >= hist[b]) left -= hist[b++];  // stops inside the thread's 16 bins: left < own
    sel[0] = (uint32_t)b;
    sel[1] = left;
  }
  __syncthreads();
  *rest = sel[1];
  return sel[0];
}

// One block per rig, in k_refine_step's place when the robust rows are on.
//  1. Selection: n = the code-0 count; the key of rank (n - 1) / 2 by two
//     4096-bin LDS histograms (integer atomics: the counts do not depend on
//     the order), the top 12 bits, then the low 12 bits of the keys inside the
//     selected top bin; two passes over the keys, whatever their number. The
//     first pass reads the slots, eight strided loads in flight per thread,
//     and leaves the keys of the first 4096 slots in LDS for the later passes
//     (one 64-bit division and one trip to memory per slot instead of three);
//     slots past them -- an eight-camera rig on the full map has 4320 -- are
//     read again.
//  2. Accumulation: refine_trips on row[m] * sqrt(w). The weights of
//     2048 rows at a time are formed by the whole block (one row per thread
//     and trip, so the 64-bit division, the FP64 division and the root are
//     paid once per row, not once per MFMA lane) and wait in LDS for the 16
//     MFMA trips that read them; a chunk is a whole number of trips, so every
//     wave adds its rows in k_refine_step's order. n_down, n_zero and sum_w
//     are per-thread sums in row order, then shuffles, then wave order.
//  3. k_refine_step's tail with end_pass_robust, and the pass's stats.
__global__ __launch_bounds__(256) void k_refine_step_robust(RefineArgs a, RobustArgs b, int pass) {
  __shared__ double red[4][16][16];
  __shared__ double sqw[kRobustChunk];
  __shared__ uint32_t hist[kRobustBins];
  __shared__ uint32_t kept[kRobustKeys];
  __shared__ double wred[4];
  __shared__ int32_t cnt[4][3];
  __shared__ uint32_t wsum[4], sel[2];
  const int rig = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  RefineRig& S = a.st[rig];
  if (S.done) return;
  const int rows = a.C * a.n_cand;
  const rfn::Slot* sl = a.slots + (size_t)pass * a.pass_slots + (size_t)rig * rows;

  // 1. the count and the top digit
  for (int i = t; i < kRobustBins; i += 256) hist[i] = 0;
  __syncthreads();
  int32_t n = 0;
  constexpr int kL = 8;
  for (int r0 = t; r0 < rows; r0 += 256 * kL) {
    int32_t code[kL], Sw[kL], Skw[kL];
#pragma unroll
    for (int u = 0; u < kL; u++) {
      const int r = r0 + 256 * u;
      code[u] = r < rows ? sl[r].code : -1;
      Sw[u] = r < rows ? sl[r].Sw : 0;
      Skw[u] = r < rows ? sl[r].Skw : 0;
    }
#pragma unroll
    for (int u = 0; u < kL; u++) {
      const int r = r0 + 256 * u;
      if (r >= rows) continue;
      const uint32_t key = code[u] == 0 ? rfn::robust_key(Sw[u], Skw[u]) : kNoKey;
      if (r < kRobustKeys) kept[r] = key;
      if (key != kNoKey) {
        n++;
        atomicAdd(&hist[key >> 12], 1u);
      }
    }
  }
#pragma unroll
  for (int q = 32; q >= 1; q >>= 1) n += __shfl_xor(n, q, 64);
  if (lane == 0) cnt[wave][0] = n;
  __syncthreads();
  const int32_t n_obs = cnt[0][0] + cnt[1][0] + cnt[2][0] + cnt[3][0];
  uint32_t median = 0;
  if (n_obs > 0) {  // block-uniform
    uint32_t rest;
    const uint32_t hi = robust_select(hist, (uint32_t)(n_obs - 1) / 2, wsum, sel, &rest);
    for (int i = t; i < kRobustBins; i += 256) hist[i] = 0;
    __syncthreads();
    for (int r = t; r < rows; r += 256) {
      const uint32_t key = robust_key_of(sl, kept, r);  // kNoKey >> 12 is no top digit of a key
      if ((key >> 12) == hi) atomicAdd(&hist[key & (kRobustBins - 1)], 1u);
    }
    __syncthreads();
    median = (hi << 12) | robust_select(hist, rest, wsum, sel, &rest);
  }
  const double sigma = rfn::robust_scale(median, b.rb.scale_floor);

  // 2. the weighted accumulation
  uint32_t* rk = b.keys ? b.keys + ((size_t)pass * a.n_rigs + rig) * rows : nullptr;
  double* rw = b.weights ? b.weights + ((size_t)pass * a.n_rigs + rig) * rows : nullptr;
  v4d acc = {0, 0, 0, 0};
  const int kk = lane >> 4, m = lane & 15;
  int32_t n_down = 0, n_zero = 0;
  double sum_w = 0.0;
  for (int c0 = 0; c0 < rows; c0 += kRobustChunk) {
    const int c1 = min(c0 + kRobustChunk, rows);
    for (int r = c0 + t; r < c1; r += 256) {
      uint32_t key = robust_key_of(sl, kept, r);
      double w = 0.0;
      if (key == kNoKey) {
        key = 0;
      } else {
        w = rfn::robust_weight(key, b.rb, sigma);
        n_down += w < 1.0;
        n_zero += w == 0.0;
        sum_w += w;
      }
      sqw[r - c0] = sqrt(w);
      if (rk) {  // the record: every slot of the pass has one writer
        rk[r] = key;
        rw[r] = w;
      }
    }
    __syncthreads();
    refine_trips<true>(sl + c0, sqw, c1 - c0, wave, kk, m, acc);  // c1 - c0 <= 2048: inside sqw
    __syncthreads();  // the next chunk overwrites sqw
  }
#pragma unroll
  for (int q = 32; q >= 1; q >>= 1) {
    n_down += __shfl_xor(n_down, q, 64);
    n_zero += __shfl_xor(n_zero, q, 64);
    sum_w += __shfl_xor(sum_w, q, 64);
  }
  if (lane == 0) {
    cnt[wave][1] = n_down;
    cnt[wave][2] = n_zero;
    wred[wave] = sum_w;
  }
  refine_tile(red, wave, kk, m, acc);
  __syncthreads();

  // 3. the tail
  if (t == 0) {
    double acc28[28];
    refine_sum28(red, acc28);
    const int32_t down = cnt[0][1] + cnt[1][1] + cnt[2][1] + cnt[3][1];
    const int32_t zero = cnt[0][2] + cnt[1][2] + cnt[2][2] + cnt[3][2];
    mantis_refine_robust_stats& st = b.stats[rig];
    st.median_key[pass] = median;
    st.n_down[pass] = down;
    st.n_zero[pass] = zero;
    st.scale[pass] = sigma;
    st.sum_w[pass] = wred[0] + wred[1] + wred[2] + wred[3];
    refine_record(a, S, rig, pass, acc28);
    S.done = rfn::end_pass_robust(acc28, n_obs, n_obs - zero, pass, a.I, a.min_obs, a.lambda, S.res) ? 1 : 0;
  }
}

}  // namespace mk
