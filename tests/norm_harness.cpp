// norm_harness.cpp — a stand-alone host program (g++, no HIP) around ur_gym_amd/csrc/urgym_norm.h, the header the kernels of
// urgym_norm.hip compile: tests/test_norm_host.py compares what it writes with evaluation.norm_sums, evaluation.norm_fold,
// evaluation.normalize_rows and evaluation.normalize_reward, and runs it a second time built with -fsanitize=address,undefined.
//
//   norm_harness fold STATE_IN RING STATE_OUT N OBS_DIM GOAL_DIM C GAMMA NORM_OBS NORM_REWARD FIRST:K...
//       STATE_IN holds the thirteen float64 arrays of urgym_norm_state back to back in the struct's order; RING the ring's observation
//       [C][N][OBS_DIM], achieved_goal and desired_goal [C][N][GOAL_DIM], reward [C][N] (float32), terminated and truncated [C][N]
//       (uint8); every FIRST:K folds K slots from FIRST on, one merge per slot and group; STATE_OUT receives the state
//   norm_harness sums FILE N        FILE holds N float64 terms; prints the 64-bit word of norm_sum_host
//   norm_harness apply IN OUT COUNT D EPS CLIP REWARD
//       IN holds COUNT * D float32 values, then D float64 means, then D float64 variances; OUT receives COUNT * D float32 values:
//       norm_value per element with inv = norm_inv(var, EPS) once per feature, or norm_reward_value where REWARD is 1 (D = 1)
//   norm_harness layout             sizeof and every offsetof of the three new structs as the C compiler lays them out, one JSON object
//   norm_harness refusal GAMMA EPS CLIP_OBS CLIP_REWARD RESERVED0     what norm_options_refusal says, or "null"
#include <inttypes.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../ur_gym_amd/csrc/urgym_norm.h"

using namespace urgym;

template <class T>
static bool io(FILE* f, std::vector<T>& v, bool write) {
  return (write ? fwrite(v.data(), sizeof(T), v.size(), f) : fread(v.data(), sizeof(T), v.size(), f)) == v.size();
}

static int fold(int argc, char** v) {
  const int n = atoi(v[3]), od = atoi(v[4]), gd = atoi(v[5]), cap = atoi(v[6]);
  const double gamma = strtod(v[7], nullptr);
  const int norm_obs = atoi(v[8]), norm_reward = atoi(v[9]);
  if (n < 1 || od < 1 || gd < 1 || cap < 1) return 3;
  const int dim[3] = {od, gd, gd};
  std::vector<double> mean[4], var[4], count[4], running((size_t)n);
  for (int g = 0; g < 4; g++) mean[g].resize(g < 3 ? dim[g] : 1), var[g].resize(g < 3 ? dim[g] : 1), count[g].resize(1);
  auto state = [&](const char* path, bool write) {
    FILE* f = fopen(path, write ? "wb" : "rb");
    if (!f) return false;
    bool ok = true;
    for (int g = 0; g < 4; g++) ok = ok && io(f, mean[g], write) && io(f, var[g], write) && io(f, count[g], write);
    ok = ok && io(f, running, write);
    fclose(f);
    return ok;
  };
  if (!state(v[0], false)) return 4;
  const size_t entries = (size_t)n * (size_t)cap;
  std::vector<float> rows[3], reward(entries);
  std::vector<uint8_t> terminated(entries), truncated(entries);
  for (int g = 0; g < 3; g++) rows[g].resize(entries * (size_t)dim[g]);
  FILE* f = fopen(v[1], "rb");
  if (!f) return 5;
  const bool ok = io(f, rows[0], false) && io(f, rows[1], false) && io(f, rows[2], false) && io(f, reward, false) && io(f, terminated, false) && io(f, truncated, false);
  fclose(f);
  if (!ok) return 6;
  std::vector<double> term((size_t)n), sq((size_t)n);
  for (int i = 10; i < argc; i++) {
    char* end;
    const int first = (int)strtol(v[i], &end, 10);
    const int steps = (int)strtol(end + 1, nullptr, 10);
    if (first < 0 || first >= cap || steps < 1 || steps > cap) return 7;  // what the entry point refuses
    for (int k = 0; k < steps; k++) {
      const size_t at = norm_slot(first, k, cap) * (size_t)n;
      if (norm_obs)
        for (int g = 0; g < 3; g++) norm_fold_group_host(mean[g].data(), var[g].data(), count[g].data(), rows[g].data() + at * (size_t)dim[g], n, dim[g], term.data(), sq.data());
      if (norm_reward)
        norm_fold_ret_host(mean[3].data(), var[3].data(), count[3].data(), running.data(), reward.data() + at, terminated.data() + at, truncated.data() + at, n, gamma, sq.data());
    }
  }
  return state(v[2], true) ? 0 : 9;
}

static int sums(char** v) {
  const int n = atoi(v[1]);
  if (n < 1) return 3;
  std::vector<double> t((size_t)n);
  FILE* f = fopen(v[0], "rb");
  if (!f) return 4;
  const bool ok = io(f, t, false);
  fclose(f);
  if (!ok) return 5;
  const double s = norm_sum_host(t.data(), n);
  uint64_t w;
  memcpy(&w, &s, sizeof(w));
  printf("%" PRIu64 "\n", w);
  return 0;
}

static int apply(char** v) {
  const int count = atoi(v[2]), d = atoi(v[3]);
  const double eps = strtod(v[4], nullptr), clip = strtod(v[5], nullptr);
  const int reward = atoi(v[6]);
  if (count < 1 || d < 1 || (reward && d != 1)) return 3;
  std::vector<float> x((size_t)count * (size_t)d);
  std::vector<double> mean((size_t)d), var((size_t)d), inv((size_t)d);
  FILE* f = fopen(v[0], "rb");
  if (!f) return 4;
  const bool ok = io(f, x, false) && io(f, mean, false) && io(f, var, false);
  fclose(f);
  if (!ok) return 5;
  for (int j = 0; j < d; j++) inv[j] = norm_inv(var[j], eps);
  for (size_t e = 0; e < x.size(); e++) {
    const size_t j = e % (size_t)d;
    x[e] = reward ? norm_reward_value(x[e], inv[j], clip) : norm_value(x[e], mean[j], inv[j], clip);
  }
  f = fopen(v[1], "wb");
  if (!f) return 6;
  const bool wrote = io(f, x, true);
  fclose(f);
  return wrote ? 0 : 7;
}

#define BEGIN(T) printf("%s\"%s\": {\"sizeof\": %zu", sep, #T, sizeof(T)), sep = ", "
#define FIELD(T, f) printf(", \"%s\": %zu", #f, offsetof(T, f))
#define END() printf("}")

static int layout() {
  const char* sep = "";
  printf("{");
  BEGIN(urgym_norm_state);
  FIELD(urgym_norm_state, observation_mean), FIELD(urgym_norm_state, observation_var), FIELD(urgym_norm_state, observation_count);
  FIELD(urgym_norm_state, achieved_goal_mean), FIELD(urgym_norm_state, achieved_goal_var), FIELD(urgym_norm_state, achieved_goal_count);
  FIELD(urgym_norm_state, desired_goal_mean), FIELD(urgym_norm_state, desired_goal_var), FIELD(urgym_norm_state, desired_goal_count);
  FIELD(urgym_norm_state, ret_mean), FIELD(urgym_norm_state, ret_var), FIELD(urgym_norm_state, ret_count), FIELD(urgym_norm_state, running_ret);
  END();
  BEGIN(urgym_normalization);
  FIELD(urgym_normalization, state), FIELD(urgym_normalization, gamma), FIELD(urgym_normalization, eps), FIELD(urgym_normalization, clip_obs);
  FIELD(urgym_normalization, clip_reward), FIELD(urgym_normalization, norm_obs), FIELD(urgym_normalization, norm_reward), FIELD(urgym_normalization, training);
  FIELD(urgym_normalization, scratch), FIELD(urgym_normalization, workspace), FIELD(urgym_normalization, workspace_bytes), FIELD(urgym_normalization, eval_scratch);
  FIELD(urgym_normalization, best_state), FIELD(urgym_normalization, reserved0);
  END();
  BEGIN(urgym_norm_rows_args);
  FIELD(urgym_norm_rows_args, observation), FIELD(urgym_norm_rows_args, achieved_goal), FIELD(urgym_norm_rows_args, desired_goal);
  FIELD(urgym_norm_rows_args, observation_out), FIELD(urgym_norm_rows_args, achieved_goal_out), FIELD(urgym_norm_rows_args, desired_goal_out);
  END();
  printf("}\n");
  return 0;
}

static int refusal(char** v) {
  urgym_normalization o;
  memset(&o, 0, sizeof(o));
  o.gamma = strtod(v[0], nullptr), o.eps = strtod(v[1], nullptr), o.clip_obs = strtod(v[2], nullptr), o.clip_reward = strtod(v[3], nullptr);
  o.reserved0 = strtoll(v[4], nullptr, 10);
  const char* what = norm_options_refusal(o);
  if (what)
    printf("\"%s\"\n", what);
  else
    printf("null\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "layout")) return layout();
  if (argc >= 13 && !strcmp(argv[1], "fold")) return fold(argc - 2, argv + 2);
  if (argc == 4 && !strcmp(argv[1], "sums")) return sums(argv + 2);
  if (argc == 9 && !strcmp(argv[1], "apply")) return apply(argv + 2);
  if (argc == 7 && !strcmp(argv[1], "refusal")) return refusal(argv + 2);
  fprintf(stderr, "usage: %s layout | fold ... | sums FILE N | apply IN OUT COUNT D EPS CLIP REWARD | refusal GAMMA EPS CLIP_OBS CLIP_REWARD RESERVED0\n", argv[0]);
  return 2;
}
