// urgym_mppi_temper.hip — the tempered update: the update of the MPPI planner with its temperature solved per parent from a target
// effective sample size (include/urgym.h, "the temperature from a target effective sample size").
// urgym_mppi_temper.h, urgym_mppi_elite.h and urgym_mppi.h state every index and every float operation; the kernel below only decides
// who runs which of them.
//
// This unit is built with -ffp-contract=off.  There are no atomics: every output has ONE writer, and every sum is formed in the order
// ordered_partial / ordered_fold state (urgym_sac_terms.h).  The exponential is urgym_mppi_temper.h's own, so that the host restates it;
// rint, division and the float64 square root are the correctly rounded ones.
//
// mppi_tempered_update_kernel: ONE workgroup of 1024 lanes per parent, lane j < K holds sample j.  Up to the weight it is
// mppi_elite_update_kernel (keys in LDS, the rank by broadcast reads, the fmax fold), restated here so that the text of
// urgym_mppi_elite.hip and urgym_mppi.hip stays what it was; without elites the rank is not formed and a sample counts where its return
// is finite.  After the weight it is that kernel's lines, or mppi_update_kernel's without elites, on the weights at the solved lambda.
//
// THE SEARCH between them is the kernel's cost: 2 + S evaluations, each one exponential per lane and one fold of Z and Q side by side.
// Every lane reads the same Z and Q from LDS, so every lane takes the same branch of the search and reaches the same barriers.
//   - The fold of an evaluation starts at the largest power of two below K: a level s >= K would add part[t + s] of lanes >= K, which
//     is the +0.0 an empty ordered_partial returns, to a weight, which is +0.0 or positive -- x + (+0.0) is x, bit for bit, for every x
//     that is not -0.0.  K = 256 folds 8 levels, not 10.  All 16 waves still take part in every barrier: waves without a sample do NOT
//     sit the search out (a wave that skips a barrier others wait at would have to leave the workgroup, and the sums after the search
//     need it).
//   - Evaluations alternate between two pairs of LDS rows (part[0..1], part[2..3]): the lanes that still read Z and Q of evaluation e
//     from row 0 of its pair are separated from the writes of evaluation e + 2 into that pair by the barriers of evaluation e + 1, so an
//     evaluation costs 1 + log2 barriers and none to protect the reads of the one before.
#include "urgym_mppi_temper.h"

namespace urgym {

namespace {

// part[c][t] += part[c][t + s] for s = first, ..., 1 and c < C: the levels of ordered_fold from `first` down with a barrier per level; a
// barrier before the first level.  first == MPPI_LANES / 2 is the whole fold.
template <int C>
__device__ __forceinline__ void fold(double (*part)[MPPI_LANES], int t, int first = MPPI_LANES / 2) {
  __syncthreads();
  for (int s = first; s >= 1; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int c = 0; c < C; c++) part[c][t] += part[c][t + s];
    }
    __syncthreads();
  }
}

template <bool ELITE>
__global__ void __launch_bounds__(MPPI_LANES) mppi_tempered_update_kernel(const urgym_mppi M, const MppiTemper P, const MppiElite A) {
  __shared__ double part[6][MPPI_LANES];
  __shared__ double key[MPPI_LANES];
  __shared__ double center[6];
  const int t = threadIdx.x, p = blockIdx.x, K = M.samples, H = M.horizon;
  const size_t E = (size_t)M.num_parents, NK = E * (size_t)K;
  const bool in = t < K;
  const size_t n = (size_t)p * K + (in ? t : 0);  // lanes past K read sample 0 and weigh nothing
  const double r = M.ret[n];
  const double k = in ? mppi_elite_key(r) : -INFINITY;
  if (ELITE) key[t] = k;
  // rmax: the fold of mppi_update_kernel over the same terms
  part[0][t] = k;
  __syncthreads();
  int rank = 0, finite = 0;
  if (ELITE && in) {  // the rank: a count over the K keys, each read a broadcast
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
  const bool counted = in && (ELITE ? mppi_elite_is(rank, A.M, r) : mppi_finite(r));
  if (ELITE && in) {
    if (A.rank) A.rank[n] = rank;
    if (A.elite) A.elite[n] = counted ? 1 : 0;
    const int count = mppi_elite_count(finite, A.M);
    if (rank == mppi_elite_last_rank(count)) {
      A.elite_count[p] = count;
      A.threshold[p] = mppi_elite_threshold(count, r);
    }
  }
  // THE SEARCH
  double lam = M.lam, w = 0.0;
  uint8_t saturated = MPPI_TEMPER_NO_RETURN;
  if (rmax == -INFINITY) {  // no finite return: the nominal alone, as the untempered updates put it
    w = in && t == 0 ? 1.0 : 0.0;
  } else {
    int first = MPPI_LANES / 2;
    while (first >= K) first >>= 1;  // the levels s >= K add only the +0.0 of lanes past K
    double(*const rows0)[MPPI_LANES] = part;
    auto ess = [=, pair = 0](double at) mutable {
      double(*rows)[MPPI_LANES] = rows0 + 2 * pair;
      pair ^= 1;
      const double wt = mppi_temper_weight(r, rmax, at, counted);
      rows[0][t] = ordered_partial(t, K, [wt](int) { return wt; });
      rows[1][t] = ordered_partial(t, K, [wt](int) { return mppi_square_term(wt); });
      fold<2>(rows, t, first);
      return mppi_ess(rows[0][0], rows[1][0]);
    };
    lam = mppi_temper_search(P.target, P.lam_min, P.lam_max, P.steps, ess, saturated);
    w = mppi_temper_weight(r, rmax, lam, counted);
    __syncthreads();  // Z and Q of the last evaluations have been read before the sums below overwrite part
  }
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
    P.lam_out[p] = lam;
    if (P.saturated) P.saturated[p] = saturated;
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
      if (ELITE) center[t] = mppi_elite_center(S, Z);
      M.new_mean[out] = v;
      if (h == 0) M.action_out[(size_t)p * 6 + t] = v;
      int first, second;
      mppi_shift_rows(h, H, M.shift, first, second);
      if (first >= 0) M.mean[((size_t)first * E + p) * 6 + t] = v;
      if (second >= 0) M.mean[((size_t)second * E + p) * 6 + t] = v;
    }
    if (!ELITE) continue;
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

}  // namespace

void mppi_tempered_update_launch(const urgym_mppi& m, const MppiTemper& t, const MppiElite* a, hipStream_t s) {
  if (a) hipLaunchKernelGGL(mppi_tempered_update_kernel<true>, dim3((unsigned)m.num_parents), dim3(MPPI_LANES), 0, s, m, t, *a);
  else hipLaunchKernelGGL(mppi_tempered_update_kernel<false>, dim3((unsigned)m.num_parents), dim3(MPPI_LANES), 0, s, m, t, MppiElite{});
}

}  // namespace urgym
