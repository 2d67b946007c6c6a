// urgym_per.h — proportional prioritized replay on the device (include/urgym.h, "prioritized replay"): the shape
// of the sum levels over the leaves, the ordered sum of one block, the descent that turns a uniform word into a ring entry, the per-row
// arithmetic of urgym_per_terms and the beta schedule, stated once as functions the kernels of urgym_per.hip and tests/per_harness.cpp
// (a host program, built without HIP) both compile; and, for HIP units only, the seam between urgym_per.hip and urgym_policy_abi.hip.
// Nothing here is exported.
//
// Leaves.  leaf[n], n = C * N, float32, indexed by the flat ring entry slot * N + env (the index urgym_replay_batch.index holds).  A leaf
// is the priority ALREADY raised to alpha; 0 = never drawn.  Leaves are non-negative and finite (urgym_per_terms writes no other).
//
// Sum levels, float64, fan-out F (PER_FANOUT = 256 on the device; the harness also runs 4).  Level 0 is the leaves.  Entry b of level
// k + 1 is the sum of entries F b .. F b + F - 1 of level k, those below the level's count: ONE float64 addition per entry in ascending
// order starting from +0.0 (per_block_sum).  Levels are added until one holds at most F entries (at least one: a ring of up to F
// entries has one level of one entry); the TOTAL is the ascending sum of that top level.  The levels lie one after the other, level 1
// first, and the total after the last: per_shape gives the counts and the offsets.  The order depends on n alone, and there are no
// floating-point atomics: whoever forms an entry from the same children stores the same bits, so an incremental repair (the touched
// entries of level 1, then everything above) leaves bitwise what a full rebuild leaves.
//
// The draw of row i.  w = (w0 << 32) | w1 of Philox4x32-10 with key = (seed lo, seed hi) and counter = (i, draw lo, draw hi, PER_TAG):
// urgym_replay_sample's word with another last counter word.  PER_TAG = 0x50455200 meets none of the existing ones: the policy noise's
// 0x504F4C00 | block (block 0, 1), the uniform replay draw's 0x52504C00, the reset sampler's blocks 0..4.
//   u = (double)(w >> 11) * 2^-53      in [0, 1), exact
//   t = u * total                      one float64 product
// then from the top level down (per_descend): the children of the chosen node (at the top: every entry of the level) are walked in
// ascending order with s = +0.0 (per_pick):
//   s2 = s + v[k];   if t < s2: take k, t = t - s, stop;   else s = s2
// where v[k] is the child's float64 sum, or (double)leaf at level 0.  If no child is taken -- t reached the sum of the children by
// rounding -- the LAST child with v > 0 is taken, and the FIRST child if there is none; t is left as it is (it stays at or above the
// sum of that child's own children, so every level below falls back the same way).  An all-zero structure therefore yields entry 0.
// A child of 0 is never taken by the rule (t < s + 0 would have held one child earlier) nor by the fallback while a sibling is positive:
// a leaf of 0 is never drawn while any leaf is positive.
//
// Every float operation of the row arithmetic below is float32 with ONE operation per line, rounded on its own, unless it says float64:
// the units that compile this are built with -ffp-contract=off.  ur_gym_amd.evaluation.per_sums / per_descent / per_terms / per_beta
// restate it.
#pragma once
#include <math.h>
#include <stdint.h>

#include "urgym_pack_map.h"  // URGYM_HD

namespace urgym {

constexpr int PER_FANOUT = 256;             // URGYM_PER_FANOUT
constexpr uint32_t PER_TAG = 0x50455200u;   // the last counter word of the prioritized draw
constexpr int PER_MAX_LEVELS = 32;          // fan-out 4 over 2^62 leaves; fan-out 256 needs at most 8
constexpr int PER_CHUNK = 16;               // children whose values are loaded together before they are scanned
constexpr int PER_TERMS_LANES = 1024;       // ONE workgroup of this many lanes runs the per-row kernel of urgym_per_terms
constexpr int PER_TERMS_MAX_COUNT = 65536;  // URGYM_PER_TERMS_MAX_COUNT: 64 rows per lane at the most

// count[k] entries at level k (count[0] = the leaves), level k >= 1 at sums[offset[k]], the total at sums[doubles - 1]
struct PerShape {
  int levels;  // the top level's number, >= 1
  int64_t count[PER_MAX_LEVELS], offset[PER_MAX_LEVELS];
  int64_t doubles;  // every level and the total
};

template <int F>
URGYM_HD inline PerShape per_shape(int64_t leaves) {
  PerShape s;
  s.count[0] = leaves, s.offset[0] = 0;
  int64_t at = 0;
  int k = 0;
  do {
    k++;
    s.count[k] = (s.count[k - 1] + F - 1) / F;
    s.offset[k] = at;
    at += s.count[k];
  } while (s.count[k] > F && k + 1 < PER_MAX_LEVELS);
  s.levels = k;
  s.doubles = at + 1;
  return s;
}

// the ascending float64 sum of v[first .. first + span), starting from +0.0: one addition per entry
template <class T>
URGYM_HD inline double per_ordered_sum(const T* v, int64_t first, int span) {
  double s = 0.0;
  for (int k0 = 0; k0 < span; k0 += PER_CHUNK) {
    double c[PER_CHUNK];
    for (int j = 0; j < PER_CHUNK; j++) c[j] = k0 + j < span ? (double)v[first + k0 + j] : 0.0;  // the loads do not wait for the sums
    for (int j = 0; j < PER_CHUNK; j++)
      if (k0 + j < span) s = s + c[j];
  }
  return s;
}

// the entries of block b of a level that holds `count`: F, or fewer in the last block
template <int F>
URGYM_HD inline int per_block_span(int64_t count, int64_t b) {
  const int64_t rest = count - b * F;
  return (int)(rest < F ? rest : F);
}

template <int F, class T>
URGYM_HD inline double per_block_sum(const T* v, int64_t count, int64_t b) {
  return per_ordered_sum(v, b * F, per_block_span<F>(count, b));
}

// one level of the descent: `span` children from v[first] on; returns the child taken and moves t into it
template <class T>
URGYM_HD inline int per_pick(const T* v, int64_t first, int span, double& t) {
  double s = 0.0;
  int last_positive = -1;
  for (int k0 = 0; k0 < span; k0 += PER_CHUNK) {
    double c[PER_CHUNK];
    for (int j = 0; j < PER_CHUNK; j++) c[j] = k0 + j < span ? (double)v[first + k0 + j] : 0.0;  // the loads do not wait for the chain
    for (int j = 0; j < PER_CHUNK; j++) {
      if (k0 + j >= span) break;
      const double s2 = s + c[j];
      if (t < s2) {
        t = t - s;
        return k0 + j;
      }
      if (c[j] > 0.0) last_positive = k0 + j;
      s = s2;
    }
  }
  return last_positive >= 0 ? last_positive : 0;
}

// u of a Philox word
URGYM_HD inline double per_uniform(uint64_t w) { return (double)(w >> 11) * 0x1p-53; }

// the leaf a word draws; total = sums[shape.doubles - 1] as the caller read it
template <int F>
URGYM_HD inline int64_t per_descend(const PerShape& shape, const float* leaf, const double* sums, double total, uint64_t w) {
  const double u = per_uniform(w);
  double t = u * total;
  int64_t node = 0;
  int span = (int)shape.count[shape.levels];  // the top level: every entry is a child
  for (int k = shape.levels; k >= 1; k--) {
    node = node * F + per_pick(sums + shape.offset[k], node * F, span, t);
    span = per_block_span<F>(shape.count[k - 1], node);
  }
  return node * F + per_pick(leaf, node * F, span, t);
}

// ---- urgym_per_terms, per row

// the importance weight before it is normalised: prob in float64 rounded once, then two float32 operations
URGYM_HD inline float per_raw_weight(float leaf, double total, float size, float beta) {
  const float prob = (float)((double)leaf / total);
  const float x = size * prob;
  return powf(x, -beta);
}

struct PerRow {
  float dq0, dq1, new_leaf;
};

// q0, q1: the two critics' values; y: the target; w: the normalised weight; fallback: max_leaf as it stood before the call
URGYM_HD inline PerRow per_row(float q0, float q1, float y, float w, float scale, float eps, float alpha, float fallback) {
  const float e0 = q0 - y;
  const float e1 = q1 - y;
  const float g0 = e0 * scale;
  const float g1 = e1 * scale;
  PerRow r;
  r.dq0 = g0 * w;
  r.dq1 = g1 * w;
  const float td = fmaxf(fabsf(e0), fabsf(e1));
  const float p = td + eps;
  const float l = powf(p, alpha);
  r.new_leaf = fabsf(l) < INFINITY ? l : fallback;  // a NaN or infinite leaf (a NaN q or y) becomes max_leaf
  return r;
}

// beta of the update at Adam step `step` (1, 2, ...): beta0 + (1 - beta0) min(1, step / beta_steps), in float64, rounded to float32 once
inline float per_beta(double beta0, int64_t step, int64_t beta_steps) {
  const double f = (double)step / (double)beta_steps;
  const double c = f < 1.0 ? f : 1.0;
  return (float)(beta0 + (1.0 - beta0) * c);
}

}  // namespace urgym

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "urgym_replay.h"

namespace urgym {

// include/urgym.h, urgym_per_priorities, validated
struct PerTree {
  int64_t leaves;  // C * N
  int N, capacity;
  float* leaf;
  double* sums;
  float* max_leaf;
};

// urgym_per_rebuild (fill = false: the leaves as they lie) and urgym_per_fill: the leaves in [lo0, hi0) and [lo1, hi1) become
// max_leaf[0], and the level-1 entries [block0, block0 + blocks0) and [block1, block1 + blocks1) are formed again
struct PerFill {
  PerTree tree;
  int64_t lo0, hi0, lo1, hi1;
  int64_t block0, blocks0, block1, blocks1;
};

// TWO launches on `s`: level 1 (one workgroup per entry), then every level above and the total (one workgroup)
void per_fill_launch(const PerFill& p, hipStream_t s);

// urgym_replay_sample_prioritized, validated: the gather's arguments (oldest_slot and size are not used) and the structure
struct PerGather {
  ReplayGather g;
  PerTree tree;
  float* leaf_out;
  double* total_out;
};

// ONE launch on `s`
void per_gather_launch(const PerGather& p, hipStream_t s);

// include/urgym.h, urgym_per_terms_args, validated
struct PerTermsCall {
  int count;
  float size, beta, alpha, eps, scale;
  const float* leaf_in;
  const double* total;
  const float *q, *y;
  float *w_raw, *w, *dq;
  const int64_t* index;  // null = no write-back group
  float* new_leaf;
  PerTree tree;  // with the write-back group
};

// ONE launch of one workgroup of PER_TERMS_LANES lanes; with the write-back group TWO more (level 1, the levels above)
void per_terms_launch(const PerTermsCall& p, hipStream_t s);

}  // namespace urgym
#endif
