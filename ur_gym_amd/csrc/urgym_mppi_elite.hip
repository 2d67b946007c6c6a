// urgym_mppi_elite.hip — the two kernels of elite selection and the adaptive std (include/urgym.h, "elite samples and an adaptive std";
// DESIGN.md section 29).  urgym_mppi_elite.h and urgym_mppi.h state every index and every float operation; the kernels below only
// decide who runs which of them.
//
// This unit is built with -ffp-contract=off.  There are no atomics: every output has ONE writer, and the sums of the update are formed
// in the order ordered_partial / ordered_fold state (urgym_sac_terms.h), exactly as mppi_update_kernel (urgym_mppi.hip) forms them:
// with M == K every output the two kernels share is the same bits.  exp, sqrt, logf, sqrtf, cospif and sinpif are the device library's;
// division and the float64 square root are the correctly rounded ones.
//
// Launches.  mppi_sample_adaptive_kernel: mppi_sample_kernel's geometry (256 lanes a workgroup, one lane per (h, planner env)) and its
// lines up to eps, restated here so that the text of urgym_mppi.hip stays what it was; the action line reads std[h][p][c] where that
// kernel reads sigma.  mppi_elite_update_kernel: ONE workgroup of 1024 lanes per parent, lane j < K holds sample j.  The K keys go to
// LDS once (8 KB); lane j then counts the keys that stand before its own, reading key[i] for i = 0 .. K - 1.  Every lane of a wave
// reads the same address in the same trip, which the LDS serves as a broadcast without a bank conflict, so the count costs K reads per
// lane and no barrier, and only the waves that hold a sample run it.  The six sums of a horizon step are folded side by side through
// LDS (48 KB) as in mppi_update_kernel, twice per step: once for the mean, once -- around the unrounded mean -- for the variance.
#include "urgym_mppi_elite.h"

#include "urgym_philox.h"
#include "urgym_policy_noise.h"

namespace urgym {

namespace {

constexpr int T = 256;  // lanes of a workgroup of the sample kernel

__global__ void __launch_bounds__(T) mppi_sample_adaptive_kernel(const urgym_mppi M, const MppiElite A, const uint64_t draw, const int iteration) {
  const size_t E = (size_t)M.num_parents, NK = E * (size_t)M.samples;
  const size_t at = (size_t)blockIdx.x * T + threadIdx.x;
  if (at >= NK * (size_t)M.horizon) return;
  const int h = (int)(at / NK), n = (int)(at % NK);
  const int p = mppi_parent(n, M.samples), j = mppi_sample(n, M.samples);
  float eps[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (j != 0) {  // mppi_sample_kernel's lines
    const uint32_t k0 = (uint32_t)M.seed, k1 = (uint32_t)(M.seed >> 32);
    const MppiCounter c0 = mppi_counter(p, iteration, h, j, draw, 0u), c1 = mppi_counter(p, iteration, h, j, draw, 1u);
    uint32_t a[4], b[4];
    philox4x32_10(k0, k1, c0.c0, c0.c1, c0.c2, c0.c3, a);
    philox4x32_10(k0, k1, c1.c0, c1.c1, c1.c2, c1.c3, b);
    const float m[6] = {(float)(a[0] >> 8), (float)(a[1] >> 8), (float)(a[2] >> 8), (float)(a[3] >> 8), (float)(b[0] >> 8), (float)(b[1] >> 8)};
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const float r = sqrtf(-2.0f * logf((m[2 * q] + 1.0f) * TWO_M24));
      const float turn = 2.0f * (m[2 * q + 1] * TWO_M24);
      eps[2 * q] = r * cospif(turn);
      eps[2 * q + 1] = r * sinpif(turn);
    }
  }
  const size_t row = ((size_t)h * E + (size_t)p) * 6;
  const float *mean = M.mean + row, *sd = A.std + row;
#pragma unroll
  for (int c = 0; c < 6; c++) {
    M.eps[at * 6 + c] = eps[c];
    M.actions[at * 6 + c] = mppi_action(mean[c], eps[c], sd[c]);
  }
}

// part[c][t] += part[c][t + s] for s = 512, ..., 1 and c < C: ordered_fold with a barrier per level; a barrier before the first level
template <int C>
__device__ __forceinline__ void fold(double (*part)[MPPI_LANES], int t) {
  __syncthreads();
  for (int s = MPPI_LANES / 2; s >= 1; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int c = 0; c < C; c++) part[c][t] += part[c][t + s];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(MPPI_LANES) mppi_elite_update_kernel(const urgym_mppi M, const MppiElite A) {
  __shared__ double part[6][MPPI_LANES];
  __shared__ double key[MPPI_LANES];
  __shared__ double center[6];
  const int t = threadIdx.x, p = blockIdx.x, K = M.samples, H = M.horizon;
  const size_t E = (size_t)M.num_parents, NK = E * (size_t)K;
  const bool in = t < K;
  const size_t n = (size_t)p * K + (in ? t : 0);  // lanes past K read sample 0 and weigh nothing
  const double r = M.ret[n];
  const double k = in ? mppi_elite_key(r) : -INFINITY;
  key[t] = k;
  // rmax: the fold of mppi_update_kernel over the same terms
  part[0][t] = k;
  __syncthreads();
  // the rank: a count over the K keys, each read a broadcast
  int rank = 0, finite = 0;
  if (in) {
    for (int i = 0; i < K; i++) {
      const double ki = key[i];
      rank += mppi_elite_before(ki, i, k, t) ? 1 : 0;
      finite += ki != -INFINITY ? 1 : 0;
    }
  }
  for (int s = MPPI_LANES / 2; s >= 1; s >>= 1) {
    if (t < s) part[0][t] = fmax(part[0][t], part[0][t + s]);
    __syncthreads();
  }
  const double rmax = part[0][0];
  __syncthreads();  // every lane has rmax before a lane overwrites part[0]
  const bool elite = in && mppi_elite_is(rank, A.M, r);
  if (in) {
    if (A.rank) A.rank[n] = rank;
    if (A.elite) A.elite[n] = elite ? 1 : 0;
    const int count = mppi_elite_count(finite, A.M);
    if (rank == mppi_elite_last_rank(count)) {
      A.elite_count[p] = count;
      A.threshold[p] = mppi_elite_threshold(count, r);
    }
  }
  double w = 0.0;
  if (in && !mppi_elite_weight_fixed(rmax, t, elite, w)) w = exp(mppi_exponent(r, rmax, M.lam));
  if (in && M.w) M.w[n] = w;
  // Z and Q side by side
  part[0][t] = ordered_partial(t, K, [w](int) { return w; });
  part[1][t] = ordered_partial(t, K, [w](int) { return mppi_square_term(w); });
  fold<2>(part, t);
  const double Z = part[0][0], Q = part[1][0];
  if (t == 0) {
    M.best_return[p] = rmax;
    M.nominal_return[p] = r;
    M.ess[p] = mppi_ess(Z, Q);
  }
  for (int h = 0; h < H; h++) {
    __syncthreads();  // part[..][0] of the step before (and Z, Q) have been read
    const float* a = M.actions + ((size_t)h * NK + n) * 6;
    float ac[6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
      ac[c] = a[c];
      const float x = ac[c];
      part[c][t] = ordered_partial(t, K, [w, x](int) { return mppi_mean_term(w, x); });
    }
    fold<6>(part, t);
    const size_t out = ((size_t)h * E + p) * 6 + t;
    if (t < 6) {
      const double S = part[t][0];
      const float v = mppi_mean(S, Z);
      center[t] = mppi_elite_center(S, Z);
      M.new_mean[out] = v;
      if (h == 0) M.action_out[(size_t)p * 6 + t] = v;
      int first, second;
      mppi_shift_rows(h, H, M.shift, first, second);
      if (first >= 0) M.mean[((size_t)first * E + p) * 6 + t] = v;
      if (second >= 0) M.mean[((size_t)second * E + p) * 6 + t] = v;
    }
    __syncthreads();  // center is written, and part[..][0] read, before the second pass overwrites part
#pragma unroll
    for (int c = 0; c < 6; c++) {
      const float x = ac[c];
      const double m = center[c];
      part[c][t] = ordered_partial(t, K, [w, x, m](int) { return mppi_elite_var_term(w, x, m); });
    }
    fold<6>(part, t);
    if (t < 6) A.new_std[out] = mppi_elite_std(part[t][0], Z, A.std_min, A.std_max);
  }
}

unsigned blocks(size_t lanes) { return (unsigned)((lanes + T - 1) / T); }

}  // namespace

void mppi_sample_adaptive_launch(const urgym_mppi& m, const MppiElite& a, uint64_t draw, int iteration, hipStream_t s) {
  hipLaunchKernelGGL(mppi_sample_adaptive_kernel, dim3(blocks((size_t)m.num_parents * m.samples * m.horizon)), dim3(T), 0, s, m, a, draw, iteration);
}

void mppi_elite_update_launch(const urgym_mppi& m, const MppiElite& a, hipStream_t s) {
  hipLaunchKernelGGL(mppi_elite_update_kernel, dim3((unsigned)m.num_parents), dim3(MPPI_LANES), 0, s, m, a);
}

}  // namespace urgym
