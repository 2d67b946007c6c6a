// Stand-alone host program (tests/test_nstep_host.py builds and runs it, once plainly and once with -fsanitize=address,undefined): the
// window, the walk and the accumulation of ur_gym_amd/csrc/urgym_nstep.h and the target row of urgym_sac_terms.h -- the very functions
// the kernels of urgym_replay.hip and urgym_sac_terms.hip compile -- run on the host the way the kernels run them, for a bitwise
// comparison with evaluation.nstep_batch / entropy_step_nstep.
//
//   nstep_harness walk IN OUT
//     IN:  int32 N, C, oldest_slot, filled_steps, n_steps, count; float gamma; int64 e[count] (the drawn entries);
//          float reward[C][N]; uint8 terminated[C][N], truncated[C][N], is_success[C][N]
//     OUT: per row: float R, g; int32 m; uint32 flag word; int64 entry_0, entry_{m-1}
//   nstep_harness target IN OUT
//     IN:  int32 count; float alpha; float reward[count], q_min_next[count], discount[count], next_log_prob[count]; uint8 terminated[count]
//     OUT: float y[count]
//   nstep_harness layout          sizeof and offsets of the three structs of include/urgym.h, as JSON
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/urgym.h"
#include "../ur_gym_amd/csrc/urgym_nstep.h"
#include "../ur_gym_amd/csrc/urgym_sac_terms.h"

using namespace urgym;

static_assert(URGYM_REPLAY_NSTEP_MAX == NSTEP_MAX, "include/urgym.h");

template <class T>
static bool read_all(FILE* f, std::vector<T>& v) {
  return fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

static int walk(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  if (!f) return printf("cannot open %s\n", in), 2;
  int32_t head[6];
  float gamma = 0.0f;
  bool ok = fread(head, sizeof(int32_t), 6, f) == 6 && fread(&gamma, sizeof(float), 1, f) == 1;
  const int N = head[0], C = head[1], oldest = head[2], filled = head[3], n_steps = head[4], count = head[5];
  ok = ok && N >= 1 && C >= 1 && oldest >= 0 && oldest < C && filled >= 1 && filled <= C && n_steps >= 1 && n_steps <= NSTEP_MAX && count >= 1 && count <= (1 << 20);
  std::vector<int64_t> e;
  std::vector<float> reward;
  std::vector<uint8_t> terminated, truncated, is_success;
  if (ok) {
    const size_t cells = (size_t)C * N;
    e.resize(count), reward.resize(cells), terminated.resize(cells), truncated.resize(cells), is_success.resize(cells);
    ok = read_all(f, e) && read_all(f, reward) && read_all(f, terminated) && read_all(f, truncated) && read_all(f, is_success);
    for (int64_t x : e) ok = ok && x >= 0 && x < (int64_t)filled * N;
  }
  fclose(f);
  if (!ok) return printf("short or malformed input %s\n", in), 2;
  f = fopen(out, "wb");
  if (!f) return printf("cannot open %s\n", out), 2;
  for (int i = 0; i < count; i++) {
    // what the sample's lane of replay_gather_nstep_kernel does after the draw
    const int p = (int)(e[i] / N), env = (int)(e[i] % N);
    const int L = nstep_window(n_steps, filled, p);
    NstepWalk w = nstep_begin(gamma);
    for (int k0 = 0; k0 < L && w.open; k0 += NSTEP_CHUNK) {
      uint32_t flag[NSTEP_CHUNK];
      float r[NSTEP_CHUNK];
      for (int j = 0; j < NSTEP_CHUNK; j++) {
        flag[j] = 0u, r[j] = 0.0f;
        if (k0 + j >= n_steps) continue;
        const int k = k0 + j < L - 1 ? k0 + j : L - 1;  // a step at or past L reads step L - 1 again
        const size_t at = (size_t)nstep_slot(oldest, p, k, C) * (size_t)N + (size_t)env;
        r[j] = reward.at(at);
        flag[j] = (uint32_t)terminated.at(at) | (uint32_t)truncated.at(at) << NSTEP_TRUNCATED_SHIFT | (uint32_t)is_success.at(at) << NSTEP_SUCCESS_SHIFT;
      }
      nstep_chunk(w, k0, L, flag, r, gamma);
    }
    const int64_t first = (int64_t)nstep_slot(oldest, p, 0, C) * N + env, last = (int64_t)nstep_slot(oldest, p, w.m - 1, C) * N + env;
    const int32_t m = w.m;
    ok = ok && fwrite(&w.R, 4, 1, f) == 1 && fwrite(&w.g, 4, 1, f) == 1 && fwrite(&m, 4, 1, f) == 1 && fwrite(&w.last, 4, 1, f) == 1 &&
         fwrite(&first, 8, 1, f) == 1 && fwrite(&last, 8, 1, f) == 1;
  }
  ok = fclose(f) == 0 && ok;
  if (!ok) return printf("cannot write %s\n", out), 2;
  printf("rows %d\n", count);
  return 0;
}

static int target(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  if (!f) return printf("cannot open %s\n", in), 2;
  int32_t count = 0;
  float alpha = 0.0f;
  bool ok = fread(&count, sizeof(count), 1, f) == 1 && fread(&alpha, sizeof(alpha), 1, f) == 1 && count >= 1 && count <= SAC_TERMS_MAX_COUNT;
  std::vector<float> reward, q_min_next, discount, next_log_prob, y;
  std::vector<uint8_t> terminated;
  if (ok) {
    reward.resize(count), q_min_next.resize(count), discount.resize(count), next_log_prob.resize(count), terminated.resize(count), y.resize(count);
    ok = read_all(f, reward) && read_all(f, q_min_next) && read_all(f, discount) && read_all(f, next_log_prob) && read_all(f, terminated);
  }
  fclose(f);
  if (!ok) return printf("short or malformed input %s\n", in), 2;
  for (int r = 0; r < count; r++) y[r] = sac_target_row_nstep(reward[r], q_min_next[r], discount[r], next_log_prob[r], terminated[r] != 0, alpha);
  f = fopen(out, "wb");
  if (!f) return printf("cannot open %s\n", out), 2;
  ok = fwrite(y.data(), sizeof(float), y.size(), f) == y.size();
  ok = fclose(f) == 0 && ok;
  if (!ok) return printf("cannot write %s\n", out), 2;
  printf("rows %d\n", (int)count);
  return 0;
}

#define FIELD(s, m) printf(", \"%s\": %zu", #m, offsetof(s, m))

static int layout() {
  printf("{\"urgym_replay_nstep\": {\"sizeof\": %zu", sizeof(urgym_replay_nstep));
  FIELD(urgym_replay_nstep, n_steps), FIELD(urgym_replay_nstep, reserved0), FIELD(urgym_replay_nstep, gamma), FIELD(urgym_replay_nstep, reserved1);
  FIELD(urgym_replay_nstep, discount), FIELD(urgym_replay_nstep, steps), FIELD(urgym_replay_nstep, last_index);
  printf("}, \"urgym_sac_entropy_nstep_args\": {\"sizeof\": %zu", sizeof(urgym_sac_entropy_nstep_args));
  FIELD(urgym_sac_entropy_nstep_args, count), FIELD(urgym_sac_entropy_nstep_args, reserved0), FIELD(urgym_sac_entropy_nstep_args, target_entropy);
  FIELD(urgym_sac_entropy_nstep_args, scale), FIELD(urgym_sac_entropy_nstep_args, log_prob), FIELD(urgym_sac_entropy_nstep_args, log_ent_coef);
  FIELD(urgym_sac_entropy_nstep_args, exp_avg), FIELD(urgym_sac_entropy_nstep_args, exp_avg_sq), FIELD(urgym_sac_entropy_nstep_args, ent_coef_out);
  FIELD(urgym_sac_entropy_nstep_args, loss_out), FIELD(urgym_sac_entropy_nstep_args, reward), FIELD(urgym_sac_entropy_nstep_args, q_min_next);
  FIELD(urgym_sac_entropy_nstep_args, discount), FIELD(urgym_sac_entropy_nstep_args, next_log_prob), FIELD(urgym_sac_entropy_nstep_args, terminated);
  FIELD(urgym_sac_entropy_nstep_args, y_out), FIELD(urgym_sac_entropy_nstep_args, d_log_prob_out);
  printf("}, \"urgym_sac_nstep\": {\"sizeof\": %zu", sizeof(urgym_sac_nstep));
  FIELD(urgym_sac_nstep, n_steps), FIELD(urgym_sac_nstep, reserved0), FIELD(urgym_sac_nstep, discount), FIELD(urgym_sac_nstep, q_min_next);
  printf("}}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "walk")) return walk(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "target")) return target(argv[2], argv[3]);
  if (argc == 2 && !strcmp(argv[1], "layout")) return layout();
  return printf("usage: nstep_harness walk|target IN OUT | layout\n"), 2;
}
