// Host harness: the launch planner (ur_gym_amd/csrc/urgym_launch_plan.h) compiled with g++, so that tests can check the geometry
// urgym_create picks without a GPU.  The URGYM_* tuning variables are read from the process environment, as urgym_create does.
// Test infrastructure only.
#include "../ur_gym_amd/csrc/urgym_launch_plan.h"

using namespace urgym;

static LaunchPlan plan(int kind, int n, int auto_reset, int cus, int per_cu) {
  const Tuning t = read_tuning();
  LaunchPlan p = plan_paths(kind, n, auto_reset != 0, t);
  plan_grids(p, cus, per_cu, t);
  return p;
}

// out: step_envs, big_blocks, tail_envs, step_blocks, reset_envs, prefetch, fused, inline_ori, setup_cache, rl_cap[0..3],
// refill_blocks (the URGYM_REFILL_BLOCKS override), step_geometry_ok
extern "C" int harness_plan(int kind, int n, int auto_reset, int cus, int per_cu, int* out) {
  const LaunchPlan p = plan(kind, n, auto_reset, cus, per_cu);
  const int v[] = {p.step_envs, p.big_blocks, p.tail_envs, p.step_blocks, p.reset_envs, p.prefetch, p.fused, p.inline_ori,
                   p.setup_cache, p.rl_cap[0], p.rl_cap[1], p.rl_cap[2], p.rl_cap[3], p.refill_blocks, step_geometry_ok(p)};
  for (int i = 0; i < 15; i++) out[i] = v[i];
  return 0;
}

extern "C" long harness_refill_blocks(int kind, int n, int cus, int per_cu, long steps_since_full_reset, int max_episode_steps) {
  return refill_blocks(plan(kind, n, 1, cus, per_cu), steps_since_full_reset, max_episode_steps);
}

// Every N in 1 .. n_max: walk the plan's STEP grid workgroup by workgroup the way the kernel maps workgroups to envs (the first
// big_blocks serve step_envs envs, the rest tail_envs, contiguous ranges) and check that the envs 0 .. N-1 are covered exactly once
// by non-empty workgroups of at most STEP_MAX_ENVS envs.  out[0] = plans that fail, out[1] = the first N that fails (0: none),
// out[2] = plans that step_geometry_ok refuses.
extern "C" int harness_cover_sweep(int kind, int auto_reset, int cus, int per_cu, int n_max, long* out) {
  out[0] = out[1] = out[2] = 0;
  for (int n = 1; n <= n_max; n++) {
    const LaunchPlan p = plan(kind, n, auto_reset, cus, per_cu);
    long covered = 0;
    bool ok = p.step_blocks >= 1;
    for (long b = 0; b < p.step_blocks && ok; b++) {
      const bool tail = p.tail_envs > 0 && b >= p.big_blocks;
      const long envs = tail ? p.tail_envs : p.step_envs;
      const long first = tail ? (long)p.big_blocks * p.step_envs + (b - p.big_blocks) * p.tail_envs : b * p.step_envs;
      ok = envs >= 1 && envs <= STEP_MAX_ENVS && first == covered && first < n;
      covered = std::min<long>(first + envs, n);
    }
    ok = ok && covered == n;
    if (!ok && out[0]++ == 0) out[1] = n;
    if (!step_geometry_ok(p)) out[2]++;
  }
  return 0;
}
