// urgym_launch_plan.h — the launch geometry of a handle, decided once in urgym_create: envs per workgroup of every kernel, the grid
// of the step launch, which auto-reset path runs, and the scheduling knobs of the URGYM_* environment variables.  Plain C++ without
// HIP, so that tests compile it with g++ (tests/plan_harness.cpp).
#pragma once
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "../../include/urgym.h"

namespace urgym {

constexpr int GROUP = 64;                  // env slots per wave-wide pass
constexpr int PREFETCH_MAX_ENVS = 32;      // envs per PREFETCH workgroup at most
constexpr int MAX_ENVS = 64;               // most envs one RESET / REFRESH workgroup serves (one wave of per-env lanes)
// A STEP workgroup may serve up to two waves' worth of envs: with its link distances parked in a global scratch array instead
// of LDS the per-env LDS footprint is 12 bytes, so the 53.7 KB that three resident workgroups allow are not exceeded, and
// N = 65536 fits ONE round of resident workgroups (E = 90) instead of two rounds of 46 with a ragged second one.
constexpr int STEP_MAX_ENVS = 128;

// The URGYM_* environment variables of urgym_create (tuning / tests; include/urgym.h).  Numbers: 0 = not set or out of range.
struct Tuning {
  int step_envs, reset_envs, refill_blocks;  // URGYM_STEP_ENVS (1 .. STEP_MAX_ENVS), URGYM_RESET_ENVS (1 .. MAX_ENVS), URGYM_REFILL_BLOCKS
  int tiers = -1, tier_envs = 0, tier_blocks = 0, tier_tail = 0;  // URGYM_STEP_TIERS: -1 not set, 0 "0" (uniform), 1 "E1,B,E2"
  bool prefetch;     // URGYM_PREFETCH (0: the auto-reset kernel after each step)
  bool verbose;      // URGYM_VERBOSE (set: print the plan to stderr)
};

// read at every urgym_create (not once per process: tests change them between handles)
inline Tuning read_tuning() {
  auto number = [](const char* name, int lo, int hi) {
    const char* v = getenv(name);
    const int x = v ? atoi(v) : 0;
    return x < lo || x > hi ? 0 : x;
  };
  Tuning t;
  t.step_envs = number("URGYM_STEP_ENVS", 1, STEP_MAX_ENVS);
  t.reset_envs = number("URGYM_RESET_ENVS", 1, MAX_ENVS);
  t.refill_blocks = number("URGYM_REFILL_BLOCKS", 1, INT_MAX);
  const char* pf = getenv("URGYM_PREFETCH");
  t.prefetch = !pf || atoi(pf) != 0;
  t.verbose = getenv("URGYM_VERBOSE") != nullptr;
  if (const char* v = getenv("URGYM_STEP_TIERS")) {
    int e1 = 0, b = 0, e2 = 0;
    if (sscanf(v, "%d,%d,%d", &e1, &b, &e2) == 3 && e1 >= 1 && e1 <= STEP_MAX_ENVS && e2 >= 1 && e2 <= STEP_MAX_ENVS && b >= 1)
      t.tiers = 1, t.tier_envs = e1, t.tier_blocks = b, t.tier_tail = e2;
    else if (atoi(v) == 0)
      t.tiers = 0;
  }
  return t;
}

struct LaunchPlan {
  int num_envs = 0;
  // STEP grid: step_blocks workgroups; the first big_blocks serve step_envs envs each, the rest tail_envs (0, 0: uniform)
  int step_envs = GROUP, big_blocks = 0, tail_envs = 0, step_blocks = 0;
  int reset_envs = 4;        // envs per workgroup of the auto-reset kernel (latency-bound: few envs, spread wide)
  bool prefetch = false;     // obstacle envs: prefetched episode records (DESIGN.md "auto-reset off the critical path")
  bool fused = false;        // ... and the steady-state step is the fused STEP + PREFETCH launch (prefetch with auto-reset)
  bool inline_ori = false;   // UR5OriReach-v1: finished envs are reset inside the step kernel (no RESET launch per step)
  // the set-up cache of the step kernel has one form, level 1 of the former three: sin / cos of the joints + the advanced obstacle
  // pose (level 2 added the link frames: +1 % for +61 MB of traffic per launch; profiles/r2/exp_setup_cache_levels.txt)
  static constexpr int setup_cache = 1;
  int rl_cap[4] = {0, 0, 0, 0};  // refill lists: three rotating asynchronous ones, one synchronous (index 3)
  int refill_blocks = 0;     // URGYM_REFILL_BLOCKS: refill workgroups per fused launch, 0 = the policy of refill_blocks()
};

// Which paths a handle takes.  Decided before the grids, which depend on the residency of the kernel the steady-state step launches.
inline LaunchPlan plan_paths(int env_kind, int num_envs, bool auto_reset, const Tuning& t) {
  LaunchPlan p;
  p.num_envs = num_envs;
  // prefetched episode records: on unless URGYM_PREFETCH=0 (then finished envs are reset by a kernel after each step).  Ori's
  // reset is a goal draw, no distance query: there the extra launches cost more than the reset kernel they replace, so Ori resets
  // inline in the step kernel instead (the same switch: URGYM_PREFETCH=0 asks for the reset kernel)
  p.prefetch = env_kind != URGYM_ENV_ORI && t.prefetch;
  p.fused = p.prefetch && auto_reset;
  p.inline_ori = env_kind == URGYM_ENV_ORI && t.prefetch;
  p.refill_blocks = t.refill_blocks;
  if (p.prefetch) {
    p.rl_cap[0] = p.rl_cap[1] = p.rl_cap[2] = num_envs;  // at most one entry per env and step: no entry is ever dropped
    p.rl_cap[3] = 2 * num_envs;
  }
  return p;
}

// Envs per step workgroup (E <= STEP_MAX_ENVS = 128).  Measured on MI355X (DESIGN.md "launch geometry"): the kernel is bound
// by the latency of the GJK iteration chains; a workgroup's lifetime grows slowly with E (145 us at 46 envs, 177 us at 64),
// while every additional ROUND of workgroups costs a whole lifetime plus a ragged tail.  So the fewest rounds win:
//   * N fits one round of <= 128-env workgroups: E = ceil(N / slots), but at least 8, rounded up to a multiple of 8 below
//     64 (64-byte runs of the float64 state arrays) -- 65536 envs -> 91 per workgroup, all 721 resident at once; 16384 -> 24;
//   * otherwise R = ceil(N / (128 slots)) rounds of equal workgroups: E = ceil(N / (R slots)).
// cus: compute units of the device; per_cu: resident workgroups per CU of the kernel the steady-state step launches.
inline void plan_grids(LaunchPlan& p, int cus, int per_cu, const Tuning& t) {
  const long n = p.num_envs;
  long slots = (long)cus * per_cu;
  if (p.fused) {  // the refill of ~2 % of the envs runs beside the step workgroups, 32 envs per workgroup
    const long refill = n / 1600;
    slots -= refill < slots / 8 ? refill : slots / 8;
  }
  const long rounds = (n + slots * STEP_MAX_ENVS - 1) / (slots * STEP_MAX_ENVS);
  long envs = (n + slots * rounds - 1) / (slots * rounds);
  if (envs < 8) envs = 8;
  if (envs < GROUP) envs = (envs + 7) / 8 * 8;
  if (envs > STEP_MAX_ENVS) envs = STEP_MAX_ENVS;
  p.step_envs = (int)envs;
  // One round, three workgroups per CU: the first 2 x CUs workgroups (two per CU, dispatched first) serve E1 envs each, the third
  // one of a CU 0.7 E1.  A CU with three resident workgroups advances each of them more slowly than one with two, and the third
  // starts last; giving it less work evens the finishing times out (N = 65536: 512 x 100 + 205 x 70 instead of 721 x 91, +5 %,
  // profiles/r2/exp_two_tier_one_round.jsonl).  URGYM_STEP_TIERS=0 keeps the uniform geometry.
  if (rounds == 1 && per_cu == 3 && slots > 2L * cus) {
    const long big = 2L * cus, rest = slots - big;
    const long e1 = (10 * n + (10 * big + 7 * rest) - 1) / (10 * big + 7 * rest);
    if (e1 >= 64 && e1 <= STEP_MAX_ENVS && n > big * e1) {  // (below ~40 000 envs the uniform geometry is as fast or faster)
      const long e2 = (n - big * e1 + rest - 1) / rest;
      p.step_envs = (int)e1; p.big_blocks = (int)big; p.tail_envs = (int)(e2 < 1 ? 1 : e2);
    }
  }
  // auto-reset kernel: ~1 % of the envs finish per step; keep that to about one workgroup per CU (4 envs at N = 65536,
  // 8 at 262144): it is pure latency, smaller workgroups shorten the wave-wide maxima, more than one per CU queue up
  while (p.reset_envs < GROUP && n / 100 > (long)p.reset_envs * (cus + cus / 4)) p.reset_envs *= 2;
  if (t.step_envs) { p.step_envs = t.step_envs; p.big_blocks = p.tail_envs = 0; }
  if (t.tiers == 1) { p.step_envs = t.tier_envs; p.big_blocks = t.tier_blocks; p.tail_envs = t.tier_tail; }
  if (t.tiers == 0) { p.step_envs = (int)envs; p.big_blocks = p.tail_envs = 0; }
  if (t.reset_envs) p.reset_envs = t.reset_envs;
  // the grid: tiers only where the big workgroups leave envs over for the tail ones
  if (p.big_blocks > 0 && (long)p.big_blocks * p.step_envs >= n) p.big_blocks = p.tail_envs = 0;
  if (p.big_blocks > 0)
    p.step_blocks = (int)(p.big_blocks + (n - (long)p.big_blocks * p.step_envs + p.tail_envs - 1) / p.tail_envs);
  else
    p.step_blocks = (int)((n + p.step_envs - 1) / p.step_envs);
}

// A STEP grid must cover env 0 .. n-1 exactly once with workgroups of at most STEP_MAX_ENVS envs: the kernel derives every per-env
// index (LDS slots, rows of the scratch arrays, observation rows) from (workgroup index, envs, big_blocks, envs_tail).
inline bool step_geometry_ok(const LaunchPlan& p) {
  const long n = p.num_envs, blocks = p.step_blocks;
  if (p.step_envs < 1 || p.step_envs > STEP_MAX_ENVS || blocks < 1) return false;
  if (p.tail_envs == 0) return (blocks - 1) * p.step_envs < n && blocks * p.step_envs >= n;
  if (p.tail_envs < 1 || p.tail_envs > STEP_MAX_ENVS || p.big_blocks < 1 || p.big_blocks >= blocks) return false;
  const long covered_before_last = (long)p.big_blocks * p.step_envs + (blocks - p.big_blocks - 1) * p.tail_envs;
  return covered_before_last < n && covered_before_last + p.tail_envs >= n;
}

// Refill workgroups of a fused launch: they stride over the list, so their number only decides how parallel the refill is.  About
// 1.6 % of the envs finish per step under a random policy (N / 1920 chunks of 32); the grid carries four times that, at least 64 --
// and the whole list's worth (one workgroup per possible chunk) in the steps where a burst is due: every env that survives from a
// full reset is truncated max_episode_steps later, all in the same step (and their successors again a period later).  The refill of
// a step's finished envs rides in the NEXT launch: a burst that happens in step k * max_episode_steps (counted from 1) is served
// one launch later; allow a step of slack on either side.  steps_since_full_reset: step launches since the last urgym_reset of
// every env, -1 if unknown.
inline long refill_blocks(const LaunchPlan& p, long steps_since_full_reset, int max_episode_steps) {
  const long full = ((long)p.rl_cap[0] + PREFETCH_MAX_ENVS - 1) / PREFETCH_MAX_ENVS;
  if (p.refill_blocks > 0) return std::min<long>(p.refill_blocks, full);
  const long s = steps_since_full_reset, m = max_episode_steps;
  const bool burst = s < 0 || m < 4 || (s >= m - 1 && (s % m <= 2 || s % m == m - 1));
  return burst ? full : std::min(std::max(64L, 4 * ((long)p.num_envs / 1920 + 1)), full);
}

}  // namespace urgym
