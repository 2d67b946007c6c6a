// urgym_demo.hip — the mixed gather of urgym_replay_sample_mixed (include/urgym.h, "the demonstration ring"):
// rows 0 .. D - 1 of a minibatch drawn from a demonstration ring, rows D .. count - 1 from the learner's own, in ONE launch.  It only
// moves bytes; float32 rows travel as 32-bit words, so a copy is bitwise whatever the value.  A unit of its own, so that the text of
// urgym_replay.hip's and urgym_per.hip's kernels does not depend on it; built with urgym_replay.hip's flags.
//
// The geometry is urgym_replay_gather.h's: one wave takes 64 samples, lane l draws the entry of sample l and moves its scalars, then the
// wave copies its samples' rows four at a time, 16 lanes per row.  What is new is that a wave whose samples straddle D reads TWO rings
// with two env counts: the sample's own lane picks its side (urgym_demo.h) for the draw and the scalars, and in the row rounds each
// group of 16 lanes picks the ring of ITS sample from the sample number alone -- the side is a function of the sample number, so
// nothing but the entry travels through the shuffles, and every lane of the wave takes part in every shuffle before any lane leaves
// the round.
#include "urgym_demo.h"

#include "urgym_replay_gather.h"
#include "urgym_philox.h"

namespace urgym {

namespace {

__global__ void __launch_bounds__(GATHER_THREADS) replay_gather_mixed_kernel(const ReplayGatherMixed Q) {
  const ReplayGather& P = Q.g;
  const urgym_replay_batch& B = P.batch;
  const int lane = threadIdx.x;
  const int base = blockIdx.x * GATHER_THREADS;  // count is an int: so is every sample number
  int64_t entry = 0;
  if (base + lane < P.count) {
    const int i = base + lane;
    const bool demo = demo_row(i, Q.demo_count);
    uint32_t w[4];
    philox4x32_10((uint32_t)P.seed, (uint32_t)(P.seed >> 32), (uint32_t)i, (uint32_t)P.draw, (uint32_t)(P.draw >> 32), demo_tag(demo), w);
    const DemoSide own{P.size, P.N, P.capacity, P.oldest_slot};
    entry = demo_entry(demo ? Q.demo_side : own, w[0], w[1]);
    gather_scalars(demo ? Q.demo : P.ring, B, i, entry);
    if (Q.source_out) Q.source_out[i] = demo ? 1 : 0;
  }
  const int group = lane / GATHER_GROUP, l = lane % GATHER_GROUP;
  const int lo = (int)(uint32_t)entry, hi = (int)(uint32_t)((uint64_t)entry >> 32);
  for (int r = 0; r < GATHER_ROUNDS; r++) {
    const int from = r * (GATHER_THREADS / GATHER_GROUP) + group;  // the lane that holds this group's sample
    const uint32_t e_lo = (uint32_t)__shfl(lo, from), e_hi = (uint32_t)__shfl(hi, from);  // every lane takes part
    const int sample = base + from;
    if (sample >= P.count) continue;
    const urgym_replay_ring& R = demo_row(sample, Q.demo_count) ? Q.demo : P.ring;  // the ring of THIS group's sample
    const size_t e = (size_t)(((uint64_t)e_hi << 32) | e_lo), s = (size_t)sample;
    gather_row(B.observation, R.observation, P.obs_dim, s, e, l);
    gather_row(B.achieved_goal, R.achieved_goal, P.goal_dim, s, e, l);
    gather_row(B.desired_goal, R.desired_goal, P.goal_dim, s, e, l);
    gather_row(B.action, R.action, 6, s, e, l);
    gather_row(B.next_observation, R.next_observation, P.obs_dim, s, e, l);
    gather_row(B.next_achieved_goal, R.next_achieved_goal, P.goal_dim, s, e, l);
    gather_row(B.next_desired_goal, R.next_desired_goal, P.goal_dim, s, e, l);
  }
}

}  // namespace

void replay_gather_mixed_launch(const ReplayGatherMixed& p, hipStream_t s) {
  hipLaunchKernelGGL(replay_gather_mixed_kernel, dim3((p.g.count + GATHER_THREADS - 1) / GATHER_THREADS), dim3(GATHER_THREADS), 0, s, p);
}

}  // namespace urgym
