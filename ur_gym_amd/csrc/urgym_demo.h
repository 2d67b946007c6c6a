// urgym_demo.h — the demonstration ring: which ring a row of a mixed minibatch reads and the entry a draw maps
// to, stated once as plain C++ functions that the kernel of urgym_demo.hip and tests/demo_harness.cpp (a host program, built without
// HIP) both compile; and, for HIP units only, the seam between urgym_demo.hip and urgym_policy_abi.hip.  Integer code only.  Nothing
// here is exported.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // __umul64hi
#endif

#include "urgym_pack_map.h"  // URGYM_HD

namespace urgym {

// the last counter word of a draw from the learner's own ring: urgym_replay_sample's
constexpr uint32_t REPLAY_TAG = 0x52504C00u;
// the last counter word of a draw from the demonstrations, "DEM\0" (URGYM_DEMO_TAG): it meets none of 0x504F4C00 | block (policy noise),
// 0x52504C00 (replay), 0x50455200 (prioritized replay), 0x4D505000 | block (the planner) or the reset sampler's blocks 0 .. 4
constexpr uint32_t DEMO_TAG = 0x44454D00u;

// THE SPLIT: rows 0 .. D - 1 of a mixed minibatch come from the demonstrations, rows D .. count - 1 from the learner's own ring
URGYM_HD inline bool demo_row(int i, int D) { return i < D; }

// the last counter word of row i's Philox call: counter = (i, draw lo, draw hi, tag)
URGYM_HD inline uint32_t demo_tag(bool demo) { return demo ? DEMO_TAG : REPLAY_TAG; }

// One side of a mixed draw: the slots (oldest_slot + j) % capacity, j < filled_steps, of a ring with N envs; size = filled_steps * N
struct DemoSide {
  uint64_t size;
  int32_t N, capacity, oldest_slot;
};

// the high half of the 128-bit product: uniform on [0, size) for a uniform 64-bit w
URGYM_HD inline uint64_t demo_mulhi(uint64_t w, uint64_t size) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(w, size);
#else
  return (uint64_t)(((unsigned __int128)w * (unsigned __int128)size) >> 64);
#endif
}

// THE ENTRY MAP of a draw, urgym_replay_sample's line by line on the side's own numbers: w = (w0 << 32) | w1 of the Philox call,
// e = (w * size) >> 64, slot = (oldest_slot + e / N) % capacity, env = e % N, index = slot * N + env
URGYM_HD inline int64_t demo_entry(const DemoSide& side, uint32_t w0, uint32_t w1) {
  const uint64_t e = demo_mulhi(((uint64_t)w0 << 32) | w1, side.size);
  const uint64_t step = e / (uint64_t)side.N, env = e - step * (uint64_t)side.N;
  uint64_t slot = (uint64_t)side.oldest_slot + step;  // < 2 capacity
  if (slot >= (uint64_t)side.capacity) slot -= (uint64_t)side.capacity;
  return (int64_t)(slot * (uint64_t)side.N + env);
}

}  // namespace urgym

#if defined(__HIPCC__)
#include "urgym_replay.h"

namespace urgym {

// One mixed minibatch (urgym_replay_sample_mixed), validated: `g` is urgym_replay_sample's own call on the learner's ring (its N,
// capacity, oldest_slot and size are the learner side's), `demo` the demonstration ring with its side's numbers
struct ReplayGatherMixed {
  ReplayGather g;
  urgym_replay_ring demo;
  DemoSide demo_side;
  int demo_count;       // D in [0, g.count]
  uint8_t* source_out;  // [count] or null
};

// ONE launch on `s`
void replay_gather_mixed_launch(const ReplayGatherMixed& p, hipStream_t s);

}  // namespace urgym
#endif
