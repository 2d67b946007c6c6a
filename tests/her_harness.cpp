// Stand-alone host program (tests/test_her_host.py builds and runs it, once plainly and once with -fsanitize=address,undefined): the
// draw, the relabel decision, the episode window, the goal entry and the re-scoring of ur_gym_amd/csrc/urgym_her.h, with the pose
// distances of urgym_device.h -- the very functions the kernel of urgym_her.hip compiles -- run on the host the way the kernel's
// sample lane runs them, for a comparison with evaluation.hindsight_pick (word for word) and evaluation.hindsight_batch (bit for
// bit, given this program's own pose terms: the host's sincos and acos are not the device's).
//
//   her_harness rows IN OUT
//     IN:  int32 N, C, oldest_slot, filled_steps, horizon, strategy, count, env_kind, goal_dim, reserved; uint64 threshold, seed, draw;
//          double distance_threshold, ori_threshold, w_collision, w_success, w_distance, w_orientation;
//          float next_achieved_goal[C][N][goal_dim], next_desired_goal[C][N][goal_dim], reward[C][N];
//          uint8 terminated[C][N], truncated[C][N], is_success[C][N]
//     OUT: per row: int64 index, g, goal_index; int32 relabel, F, j; float reward; double d, th, d0, th0; uint8 terminated,
//          is_success, pad[6]; float goal[6]  (F, j and g for every row; the re-scored values only where relabel)
//   her_harness layout          sizeof and offsets of the two structs of include/urgym.h, as JSON
#define URGYM_HOST_HARNESS 1
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/urgym.h"
#include "../ur_gym_amd/csrc/urgym_device.h"
#include "../ur_gym_amd/csrc/urgym_her.h"

using namespace urgym;

static_assert(URGYM_HER_HORIZON_MAX == HER_HORIZON_MAX && URGYM_HER_GOAL_FUTURE == HER_GOAL_FUTURE && URGYM_HER_GOAL_FINAL == HER_GOAL_FINAL &&
                  URGYM_HER_GOAL_OWN == HER_GOAL_OWN,
              "include/urgym.h");

template <class T>
static bool read_all(FILE* f, std::vector<T>& v) {
  return fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

struct Row {
  int64_t index, g, goal_index;
  int32_t relabel, F, j;
  float reward;
  double terms[4];
  uint8_t terminated, is_success, pad[6];
  float goal[6];
};
static_assert(sizeof(Row) == 104, "the layout tests/test_her_host.py reads");

static int rows(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  if (!f) return printf("cannot open %s\n", in), 2;
  int32_t head[10];
  uint64_t big[3];
  double cfg[6];
  bool ok = fread(head, sizeof(int32_t), 10, f) == 10 && fread(big, sizeof(uint64_t), 3, f) == 3 && fread(cfg, sizeof(double), 6, f) == 6;
  const int N = head[0], C = head[1], oldest = head[2], filled = head[3], horizon = head[4], strategy = head[5], count = head[6], kind = head[7], GD = head[8];
  const uint64_t threshold = big[0], seed = big[1], draw = big[2];
  ok = ok && N >= 1 && C >= 1 && oldest >= 0 && oldest < C && filled >= 1 && filled <= C && horizon >= 1 && horizon <= HER_HORIZON_MAX && strategy >= 0 &&
       strategy <= 2 && count >= 1 && count <= (1 << 20) && kind >= 0 && kind <= 3 && (GD == 3 || GD == 6) && threshold <= (uint64_t)1 << 32;
  std::vector<float> ach, des, reward;
  std::vector<uint8_t> terminated, truncated, is_success;
  if (ok) {
    const size_t cells = (size_t)C * N;
    ach.resize(cells * GD), des.resize(cells * GD), reward.resize(cells), terminated.resize(cells), truncated.resize(cells), is_success.resize(cells);
    ok = read_all(f, ach) && read_all(f, des) && read_all(f, reward) && read_all(f, terminated) && read_all(f, truncated) && read_all(f, is_success);
  }
  fclose(f);
  if (!ok) return printf("short or malformed input %s\n", in), 2;
  const HerRule rule{cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], cfg[5], kind == URGYM_ENV_ORI || kind == URGYM_ENV_OBS, GD};
  const uint64_t size = (uint64_t)filled * (uint64_t)N;
  f = fopen(out, "wb");
  if (!f) return printf("cannot open %s\n", out), 2;
  for (int i = 0; i < count; i++) {
    // what the sample's lane of replay_gather_hindsight_kernel does
    uint32_t w[4];
    philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)i, (uint32_t)draw, (uint32_t)(draw >> 32), 0x52504C00u, w);
    const uint64_t e = (uint64_t)(((unsigned __int128)(((uint64_t)w[0] << 32) | w[1]) * size) >> 64);
    const uint64_t step = e / (uint64_t)N, env = e - step * (uint64_t)N;
    const int p = (int)step;
    Row r;
    memset(&r, 0, sizeof(r));
    r.index = (int64_t)((uint64_t)her_slot(oldest, p, 0, C) * (uint64_t)N + env);
    r.relabel = her_relabels(w[2], threshold);
    const int H = her_window(horizon, filled, p);
    HerWalk walk = her_begin();
    for (int k0 = 0; k0 < H && walk.open; k0 += HER_CHUNK) {
      uint32_t ends[HER_CHUNK];
      for (int j = 0; j < HER_CHUNK; j++) {
        const int k = k0 + j < H - 1 ? k0 + j : H - 1;  // a step at or past H reads step H - 1 again
        const size_t at = (size_t)her_slot(oldest, p, k, C) * (size_t)N + (size_t)env;
        ends[j] = (uint32_t)terminated.at(at) | (uint32_t)truncated.at(at);
      }
      her_chunk(walk, k0, H, ends);
    }
    r.F = walk.F;
    r.j = her_pick(strategy, w[3], walk.F);
    r.g = (int64_t)((uint64_t)her_slot(oldest, p, r.j, C) * (uint64_t)N + env);
    r.goal_index = r.relabel && strategy != HER_GOAL_OWN ? r.g : -1;
    r.reward = reward.at((size_t)r.index), r.terminated = terminated.at((size_t)r.index), r.is_success = is_success.at((size_t)r.index);
    if (r.relabel) {
      const float* g1 = strategy == HER_GOAL_OWN ? &des.at((size_t)r.index * GD) : &ach.at((size_t)r.g * GD);
      const float* a = &ach.at((size_t)r.index * GD);
      const float* g0 = &des.at((size_t)r.index * GD);
      double a6[6] = {0, 0, 0, 0, 0, 0}, n6[6] = {0, 0, 0, 0, 0, 0}, o6[6] = {0, 0, 0, 0, 0, 0};
      for (int k = 0; k < GD; k++) a6[k] = (double)a[k], n6[k] = (double)g1[k], o6[k] = (double)g0[k], r.goal[k] = g1[k];
      double d = pos_distance(a6, n6), d0 = pos_distance(a6, o6), th = 0.0, th0 = 0.0;
      if (GD == 6) th = angular_distance(a6 + 3, n6 + 3), th0 = angular_distance(a6 + 3, o6 + 3);
      const HerScore s = her_rescore(rule, r.reward, r.terminated != 0, r.is_success != 0, d, th, d0, th0);
      r.reward = s.reward, r.terminated = s.terminated, r.is_success = s.is_success;
      r.terms[0] = d, r.terms[1] = th, r.terms[2] = d0, r.terms[3] = th0;
    }
    ok = ok && fwrite(&r, sizeof(r), 1, f) == 1;
  }
  ok = fclose(f) == 0 && ok;
  if (!ok) return printf("cannot write %s\n", out), 2;
  printf("rows %d\n", count);
  return 0;
}

#define FIELD(s, m) printf(", \"%s\": %zu", #m, offsetof(s, m))

static int layout() {
  printf("{\"urgym_replay_hindsight\": {\"sizeof\": %zu", sizeof(urgym_replay_hindsight));
  FIELD(urgym_replay_hindsight, relabel_threshold), FIELD(urgym_replay_hindsight, strategy), FIELD(urgym_replay_hindsight, horizon);
  FIELD(urgym_replay_hindsight, goal_index), FIELD(urgym_replay_hindsight, pose_terms), FIELD(urgym_replay_hindsight, reserved0);
  printf("}, \"urgym_sac_hindsight\": {\"sizeof\": %zu", sizeof(urgym_sac_hindsight));
  FIELD(urgym_sac_hindsight, relabel_threshold), FIELD(urgym_sac_hindsight, strategy), FIELD(urgym_sac_hindsight, horizon), FIELD(urgym_sac_hindsight, reserved0);
  printf("}}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "rows")) return rows(argv[2], argv[3]);
  if (argc == 2 && !strcmp(argv[1], "layout")) return layout();
  return printf("usage: her_harness rows IN OUT | layout\n"), 2;
}
