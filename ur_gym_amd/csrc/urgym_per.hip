// urgym_per.hip — proportional prioritized replay on the device (include/urgym.h, "prioritized replay"): the sum
// levels over the leaves, the draw through them with the one-step gather behind it, the importance weights and the write-back of the
// new priorities.  urgym_per.h states every index and every float operation; the kernels below only decide who runs which of them.
//
// This unit is built with -ffp-contract=off.  There are no floating-point atomics: a sum entry is formed by ONE lane, in the order
// per_ordered_sum states, from values that are final when it reads them (the launch before wrote them), so every lane that forms the
// same entry stores the same bits.  powf is the device library's; division is the correctly rounded one; subnormals are kept.
//
// Launches.  per_level1_kernel: one workgroup of 256 lanes per level-1 entry (the lanes load the 256 leaves side by side into LDS,
// lane 0 adds them in order).  per_upper_kernel: ONE workgroup that forms every level above level 1 and the total, a barrier between
// levels.  urgym_per_rebuild and urgym_per_fill are these two; urgym_per_terms is per_terms_kernel and then these two;
// urgym_replay_sample_prioritized is per_gather_kernel alone.
#include "urgym_per.h"

#include "urgym_philox.h"
#include "urgym_replay_gather.h"

namespace urgym {

namespace {

constexpr int F = PER_FANOUT;

struct PerLevel1 {
  PerFill f;
  const int64_t* index;  // non-null: workgroup g forms the entry that holds leaf index[g] (urgym_per_terms); an index outside the leaves forms none
};

__global__ void __launch_bounds__(F) per_level1_kernel(const PerLevel1 P) {
  __shared__ float v[F];
  const PerFill& f = P.f;
  const int t = threadIdx.x;
  const int64_t g = blockIdx.x;
  int64_t b;
  if (P.index) {
    const int64_t at = P.index[g];
    if (at < 0 || at >= f.tree.leaves) return;  // the same for every lane
    b = at / F;
  } else {
    b = g < f.blocks0 ? f.block0 + g : f.block1 + (g - f.blocks0);
  }
  const int64_t i = b * F + t;
  float x = 0.0f;
  if (i < f.tree.leaves) {
    if ((i >= f.lo0 && i < f.hi0) || (i >= f.lo1 && i < f.hi1)) {
      x = f.tree.max_leaf[0];
      f.tree.leaf[i] = x;
    } else {
      x = f.tree.leaf[i];
    }
  }
  v[t] = x;
  __syncthreads();
  if (t == 0) f.tree.sums[b] = per_ordered_sum(v, 0, per_block_span<F>(f.tree.leaves, b));  // level 1 starts the array
}

__global__ void __launch_bounds__(F) per_upper_kernel(const PerTree T, const PerShape S) {
  const int t = threadIdx.x;
  for (int k = 2; k <= S.levels; k++) {
    for (int64_t b = t; b < S.count[k]; b += F) T.sums[S.offset[k] + b] = per_block_sum<F>(T.sums + S.offset[k - 1], S.count[k - 1], b);
    __syncthreads();  // the level is complete, and visible to the workgroup, before the next reads it
  }
  if (t == 0) T.sums[S.doubles - 1] = per_ordered_sum(T.sums + S.offset[S.levels], 0, (int)S.count[S.levels]);
}

// replay_gather_kernel with the descent in place of the uniform draw: the same geometry, the same body (urgym_replay_gather.h)
__global__ void __launch_bounds__(GATHER_THREADS) per_gather_kernel(const PerGather P, const PerShape S) {
  const int lane = threadIdx.x;
  const int base = blockIdx.x * GATHER_THREADS;
  const ReplayGather& G = P.g;
  int64_t entry = 0;
  if (base + lane < G.count) {
    const int i = base + lane;
    uint32_t w[4];
    philox4x32_10((uint32_t)G.seed, (uint32_t)(G.seed >> 32), (uint32_t)i, (uint32_t)G.draw, (uint32_t)(G.draw >> 32), PER_TAG, w);
    const double total = P.tree.sums[S.doubles - 1];
    entry = per_descend<F>(S, P.tree.leaf, P.tree.sums, total, ((uint64_t)w[0] << 32) | w[1]);  // in [0, leaves) whatever the values
    P.leaf_out[i] = P.tree.leaf[entry];
    if (i == 0) P.total_out[0] = total;
    gather_scalars(G.ring, G.batch, i, entry);
  }
  gather_rows(G, base, lane, entry);
}

// red[0] = the maximum (fmaxf: a NaN is passed over) of the 1024 lanes' values; a barrier before, one per level, and one after the read
__device__ __forceinline__ float fold_max(float* red, int t, float x) {
  red[t] = x;
  __syncthreads();
  for (int s = PER_TERMS_LANES / 2; s >= 1; s >>= 1) {
    if (t < s) red[t] = fmaxf(red[t], red[t + s]);
    __syncthreads();
  }
  const float m = red[0];
  __syncthreads();
  return m;
}

__global__ void __launch_bounds__(PER_TERMS_LANES) per_terms_kernel(const PerTermsCall P) {
  __shared__ float red[PER_TERMS_LANES];
  const int t = threadIdx.x;
  const bool back = P.index != nullptr;
  // read by every lane before the first barrier; lane 0 writes max_leaf after the last
  const double total = P.total[0];
  const float old_max = back ? P.tree.max_leaf[0] : 0.0f;
  float wm = 0.0f;
  for (int r = t; r < P.count; r += PER_TERMS_LANES) {
    const float wr = per_raw_weight(P.leaf_in[r], total, P.size, P.beta);
    P.w_raw[r] = wr;
    wm = fmaxf(wm, wr);
  }
  const float wmax = fold_max(red, t, wm);
  float lm = 0.0f;
  for (int r = t; r < P.count; r += PER_TERMS_LANES) {
    const float w = P.w_raw[r] / wmax;  // this lane's own store
    P.w[r] = w;
    const PerRow row = per_row(P.q[r], P.q[(size_t)P.count + r], P.y[r], w, P.scale, P.eps, P.alpha, old_max);
    P.dq[r] = row.dq0;
    P.dq[(size_t)P.count + r] = row.dq1;
    if (!back) continue;
    P.new_leaf[r] = row.new_leaf;
    lm = fmaxf(lm, row.new_leaf);
    const int64_t at = P.index[r];
    if (at >= 0 && at < P.tree.leaves) P.tree.leaf[at] = 0.0f;  // every row of an entry stores the same +0: the start of its maximum
  }
  if (!back) return;  // the same for every lane
  const float new_max = fold_max(red, t, lm);  // its barriers also put every +0 before the first maximum
  for (int r = t; r < P.count; r += PER_TERMS_LANES) {
    const int64_t at = P.index[r];
    // new_leaf is non-negative and finite: the order of the bit patterns is the order of the values, and an integer maximum does not
    // depend on the order of its operands
    if (at >= 0 && at < P.tree.leaves) atomicMax((unsigned int*)(P.tree.leaf + at), __float_as_uint(P.new_leaf[r]));
  }
  if (t == 0) P.tree.max_leaf[0] = fmaxf(old_max, new_max);
}

void upper_launch(const PerTree& tree, const PerShape& shape, hipStream_t s) {
  hipLaunchKernelGGL(per_upper_kernel, dim3(1), dim3(F), 0, s, tree, shape);
}

}  // namespace

void per_fill_launch(const PerFill& p, hipStream_t s) {
  hipLaunchKernelGGL(per_level1_kernel, dim3((unsigned)(p.blocks0 + p.blocks1)), dim3(F), 0, s, PerLevel1{p, nullptr});
  upper_launch(p.tree, per_shape<F>(p.tree.leaves), s);
}

void per_gather_launch(const PerGather& p, hipStream_t s) {
  hipLaunchKernelGGL(per_gather_kernel, dim3((p.g.count + GATHER_THREADS - 1) / GATHER_THREADS), dim3(GATHER_THREADS), 0, s, p,
                     per_shape<F>(p.tree.leaves));
}

void per_terms_launch(const PerTermsCall& p, hipStream_t s) {
  hipLaunchKernelGGL(per_terms_kernel, dim3(1), dim3(PER_TERMS_LANES), 0, s, p);
  if (!p.index) return;
  const PerShape shape = per_shape<F>(p.tree.leaves);
  PerLevel1 l;
  l.f = PerFill{p.tree, 0, 0, 0, 0, 0, 0, 0, 0};
  l.index = p.index;
  // at least as many rows as level-1 entries: every entry once instead of one per row (the same bits either way)
  if ((int64_t)p.count >= shape.count[1]) l.f.blocks0 = shape.count[1], l.index = nullptr;
  hipLaunchKernelGGL(per_level1_kernel, dim3((unsigned)(l.index ? (int64_t)p.count : l.f.blocks0)), dim3(F), 0, s, l);
  upper_launch(p.tree, shape, s);
}

}  // namespace urgym
