// Stand-alone host program (tests/test_demo_host.py builds and runs it, once plainly and once with -fsanitize=address,undefined): the
// split, the tag and the entry map of ur_gym_amd/csrc/urgym_demo.h and the masked verdict of urgym_sac_bc.h -- the very functions the
// kernels of urgym_demo.hip and urgym_sac_bc_masked.hip compile -- run on the host the way the kernels run them, for a bitwise comparison
// with evaluation.mixed_entries and evaluation.policy_terms_cloned(row_mask=).
//
//   demo_harness layout         sizeof and every offsetof of urgym_replay_demonstrations and urgym_sac_demonstrating, as JSON
//   demo_harness entries IN OUT
//     IN:  uint64 seed, draw; int64 count, D; then twice (the learner's side, the demonstrations'): uint64 size; int32 N, capacity,
//          oldest_slot, pad
//     OUT: int64 index[count]; uint8 source[count]
//   demo_harness masked IN OUT
//     IN:  int64 count; int32 scale_by_q, q_filter; float alpha, scale, weight, bc_scale;
//          float log_prob[count], q[2][count], y[count], q_min[count], dqmin_da[count][6], action_pi[count][6], action_data[count][6];
//          uint8 row_mask[count]
//     OUT: double S_q0, S_q1, S_actor, S_absq, S_h; float critic_loss, actor_loss, bc_loss, w, mean_abs; int32 rows;
//          uint8 cloned[count]; float d_action[count][6]
#define URGYM_HOST_HARNESS 1
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/urgym.h"
#include "../ur_gym_amd/csrc/urgym_device.h"
#include "../ur_gym_amd/csrc/urgym_demo.h"
#include "../ur_gym_amd/csrc/urgym_sac_bc.h"

using namespace urgym;

static_assert(URGYM_DEMO_TAG == DEMO_TAG, "include/urgym.h");

#define FIELD(s, m) printf(", \"%s\": %zu", #m, offsetof(s, m))

static int layout() {
  printf("{\"urgym_replay_demonstrations\": {\"sizeof\": %zu", sizeof(urgym_replay_demonstrations));
  FIELD(urgym_replay_demonstrations, ring), FIELD(urgym_replay_demonstrations, num_envs), FIELD(urgym_replay_demonstrations, oldest_slot);
  FIELD(urgym_replay_demonstrations, filled_steps), FIELD(urgym_replay_demonstrations, count);
  printf("}, \"urgym_sac_demonstrating\": {\"sizeof\": %zu", sizeof(urgym_sac_demonstrating));
  FIELD(urgym_sac_demonstrating, demonstrations), FIELD(urgym_sac_demonstrating, source), FIELD(urgym_sac_demonstrating, clone_demonstrations_only);
  FIELD(urgym_sac_demonstrating, reserved0);
  printf("}}\n");
  return 0;
}

struct SideIn {
  uint64_t size;
  int32_t N, capacity, oldest_slot, pad;
};

static int entries(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  if (!f) return printf("cannot open %s\n", in), 2;
  uint64_t key[2];
  int64_t n[2];
  SideIn sides[2];
  bool ok = fread(key, sizeof(uint64_t), 2, f) == 2 && fread(n, sizeof(int64_t), 2, f) == 2 && fread(sides, sizeof(SideIn), 2, f) == 2;
  fclose(f);
  ok = ok && n[0] >= 1 && n[0] <= (1 << 24) && n[1] >= 0 && n[1] <= n[0];
  for (const SideIn& s : sides) ok = ok && s.N >= 1 && s.capacity >= 1 && s.oldest_slot >= 0 && s.oldest_slot < s.capacity && s.size >= 1 && s.size < (uint64_t)1 << 63;
  if (!ok) return printf("short or malformed input %s\n", in), 2;
  const uint64_t seed = key[0], draw = key[1];
  const int count = (int)n[0], D = (int)n[1];
  const DemoSide own{sides[0].size, sides[0].N, sides[0].capacity, sides[0].oldest_slot}, demo{sides[1].size, sides[1].N, sides[1].capacity, sides[1].oldest_slot};
  std::vector<int64_t> index(count);
  std::vector<uint8_t> source(count);
  for (int i = 0; i < count; i++) {  // the sample lane of replay_gather_mixed_kernel
    const bool from_demo = demo_row(i, D);
    uint32_t w[4];
    philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)i, (uint32_t)draw, (uint32_t)(draw >> 32), demo_tag(from_demo), w);
    index[i] = demo_entry(from_demo ? demo : own, w[0], w[1]);
    source[i] = from_demo ? 1 : 0;
  }
  f = fopen(out, "wb");
  if (!f) return printf("cannot open %s\n", out), 2;
  ok = fwrite(index.data(), sizeof(int64_t), index.size(), f) == index.size() && fwrite(source.data(), 1, source.size(), f) == source.size();
  ok = fclose(f) == 0 && ok;
  if (!ok) return printf("cannot write %s\n", out), 2;
  printf("rows %d demonstrations %d\n", count, D);
  return 0;
}

static int masked(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  if (!f) return printf("cannot open %s\n", in), 2;
  int64_t n = 0;
  int32_t flags[2];
  float sc[4];
  bool ok = fread(&n, sizeof(n), 1, f) == 1 && fread(flags, sizeof(int32_t), 2, f) == 2 && fread(sc, sizeof(float), 4, f) == 4 && n >= 1 && n <= SAC_TERMS_MAX_COUNT;
  std::vector<float> log_prob, q, y, q_min, dqmin_da, action_pi, action_data;
  std::vector<uint8_t> mask;
  if (ok) {
    const size_t c = (size_t)n;
    log_prob.resize(c), q.resize(2 * c), y.resize(c), q_min.resize(c), dqmin_da.resize(6 * c), action_pi.resize(6 * c), action_data.resize(6 * c), mask.resize(c);
    for (std::vector<float>* x : {&log_prob, &q, &y, &q_min, &dqmin_da, &action_pi, &action_data}) ok = ok && fread(x->data(), sizeof(float), x->size(), f) == x->size();
    ok = ok && fread(mask.data(), 1, mask.size(), f) == mask.size();
  }
  fclose(f);
  if (!ok) return printf("short or malformed input %s\n", in), 2;
  const int count = (int)n;
  const bool scale_by_q = flags[0] != 0, q_filter = flags[1] != 0;
  const float alpha = sc[0], scale = sc[1], weight = sc[2], bc_scale = sc[3];

  // phase 1: the row's verdict and its five terms, then the sums (over ALL rows)
  auto cloned_row = [&](int r) { return sac_bc_cloned_masked(mask[r], q_filter, sac_bc_q_data(q[r], q[(size_t)count + r]), q_min[r]); };
  std::vector<uint8_t> cloned(count);
  int32_t rows = 0;
  for (int r = 0; r < count; r++) cloned[r] = cloned_row(r), rows += cloned[r];
  double S[5];
  S[0] = ordered_sum(count, [&](int r) { return sac_critic_term(q[r], y[r]); });
  S[1] = ordered_sum(count, [&](int r) { return sac_critic_term(q[(size_t)count + r], y[r]); });
  S[2] = ordered_sum(count, [&](int r) { return sac_actor_term(alpha, log_prob[r], q_min[r]); });
  S[3] = ordered_sum(count, [&](int r) { return fabsf(q_min[r]); });
  S[4] = ordered_sum(count, [&](int r) { return cloned_row(r) ? sac_bc_term(&action_pi[(size_t)r * 6], &action_data[(size_t)r * 6]) : 0.0f; });
  const float mean_abs = ordered_mean(S[3], count);
  const float w = sac_bc_weight(scale_by_q, weight, mean_abs);

  // phase 2: the elements, the mask and the actions read again
  std::vector<float> d_action(6 * (size_t)count);
  for (size_t i = 0; i < d_action.size(); i++) {
    const float g = dqmin_da[i] * scale;
    d_action[i] = cloned_row((int)(i / 6)) ? sac_bc_upstream(g, sac_bc_difference(action_pi[i], action_data[i]), w, bc_scale) : g;
  }

  f = fopen(out, "wb");
  if (!f) return printf("cannot open %s\n", out), 2;
  const float scalars[5] = {sac_critic_loss(ordered_mean(S[0], count), ordered_mean(S[1], count)), ordered_mean(S[2], count), ordered_mean(S[4], count), w, mean_abs};
  ok = fwrite(S, sizeof(double), 5, f) == 5 && fwrite(scalars, sizeof(float), 5, f) == 5 && fwrite(&rows, sizeof(rows), 1, f) == 1 &&
       fwrite(cloned.data(), 1, cloned.size(), f) == cloned.size() && fwrite(d_action.data(), sizeof(float), d_action.size(), f) == d_action.size();
  ok = fclose(f) == 0 && ok;
  if (!ok) return printf("cannot write %s\n", out), 2;
  printf("rows %d cloned %d\n", count, rows);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "layout")) return layout();
  if (argc == 4 && !strcmp(argv[1], "entries")) return entries(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "masked")) return masked(argv[2], argv[3]);
  return printf("usage: demo_harness layout | entries IN OUT | masked IN OUT\n"), 2;
}
