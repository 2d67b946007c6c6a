// Stand-alone host program (tests/test_sac_bc_host.py builds and runs it, once plainly and once with -fsanitize=address,undefined): the
// per-row arithmetic and the scalar weight of ur_gym_amd/csrc/urgym_sac_bc.h -- the very functions the kernel of urgym_sac_bc.hip compiles
// -- with the ordered sums of urgym_sac_terms.h as host loops in the stated order, in the kernel's two phases, for a bitwise comparison
// with evaluation.policy_terms_cloned.
//
//   sac_bc_harness layout      sizeof and every offsetof of urgym_sac_clone_args and urgym_sac_cloning as the C compiler lays them out, JSON
//   sac_bc_harness IN OUT
//     IN:  int64 count; int32 scale_by_q, q_filter; float alpha, scale, weight, bc_scale;
//          float log_prob[count], q[2][count], y[count], q_min[count], dqmin_da[count][6], action_pi[count][6], action_data[count][6]
//     OUT: double S_q0, S_q1, S_actor, S_absq, S_h (the five ordered sums);
//          float critic_loss, actor_loss, bc_loss, w, mean_abs; int32 rows; uint8 cloned[count]; float d_action[count][6]
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../include/urgym.h"
#include "../ur_gym_amd/csrc/urgym_sac_bc.h"

using namespace urgym;

#define FIELD(s, m) printf(", \"%s\": %zu", #m, offsetof(s, m))

static int layout() {
  printf("{\"urgym_sac_clone_args\": {\"sizeof\": %zu", sizeof(urgym_sac_clone_args));
  FIELD(urgym_sac_clone_args, action_pi), FIELD(urgym_sac_clone_args, action_data), FIELD(urgym_sac_clone_args, weight), FIELD(urgym_sac_clone_args, bc_scale);
  FIELD(urgym_sac_clone_args, scale_by_q), FIELD(urgym_sac_clone_args, q_filter), FIELD(urgym_sac_clone_args, bc_loss_out);
  FIELD(urgym_sac_clone_args, bc_weight_out), FIELD(urgym_sac_clone_args, bc_rows_out), FIELD(urgym_sac_clone_args, reserved0);
  printf("}, \"urgym_sac_cloning\": {\"sizeof\": %zu", sizeof(urgym_sac_cloning));
  FIELD(urgym_sac_cloning, weight), FIELD(urgym_sac_cloning, scale_by_q), FIELD(urgym_sac_cloning, q_filter), FIELD(urgym_sac_cloning, reserved0);
  FIELD(urgym_sac_cloning, bc_loss), FIELD(urgym_sac_cloning, bc_weight), FIELD(urgym_sac_cloning, bc_rows);
  printf("}}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "layout")) return layout();
  if (argc != 3) return printf("usage: sac_bc_harness layout | IN OUT\n"), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return printf("cannot open %s\n", argv[1]), 2;
  int64_t n = 0;
  int32_t flags[2];
  float sc[4];
  bool ok = fread(&n, sizeof(n), 1, f) == 1 && fread(flags, sizeof(int32_t), 2, f) == 2 && fread(sc, sizeof(float), 4, f) == 4 && n >= 1 && n <= SAC_TERMS_MAX_COUNT;
  std::vector<float> log_prob, q, y, q_min, dqmin_da, action_pi, action_data;
  if (ok) {
    const size_t c = (size_t)n;
    log_prob.resize(c), q.resize(2 * c), y.resize(c), q_min.resize(c), dqmin_da.resize(6 * c), action_pi.resize(6 * c), action_data.resize(6 * c);
    for (std::vector<float>* x : {&log_prob, &q, &y, &q_min, &dqmin_da, &action_pi, &action_data}) ok = ok && fread(x->data(), sizeof(float), x->size(), f) == x->size();
  }
  fclose(f);
  if (!ok) return printf("short or malformed input %s\n", argv[1]), 2;
  const int count = (int)n;
  const bool scale_by_q = flags[0] != 0, q_filter = flags[1] != 0;
  const float alpha = sc[0], scale = sc[1], weight = sc[2], bc_scale = sc[3];

  // phase 1: the row's verdict and its five terms, then the sums
  auto cloned_row = [&](int r) { return sac_bc_cloned(q_filter, sac_bc_q_data(q[r], q[(size_t)count + r]), q_min[r]); };
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

  // phase 2: the elements, the actions read again
  std::vector<float> d_action(6 * (size_t)count);
  for (size_t i = 0; i < d_action.size(); i++) {
    const float g = dqmin_da[i] * scale;
    d_action[i] = cloned_row((int)(i / 6)) ? sac_bc_upstream(g, sac_bc_difference(action_pi[i], action_data[i]), w, bc_scale) : g;
  }

  f = fopen(argv[2], "wb");
  if (!f) return printf("cannot open %s\n", argv[2]), 2;
  const float scalars[5] = {sac_critic_loss(ordered_mean(S[0], count), ordered_mean(S[1], count)), ordered_mean(S[2], count), ordered_mean(S[4], count), w, mean_abs};
  ok = fwrite(S, sizeof(double), 5, f) == 5 && fwrite(scalars, sizeof(float), 5, f) == 5 && fwrite(&rows, sizeof(rows), 1, f) == 1 &&
       fwrite(cloned.data(), 1, cloned.size(), f) == cloned.size() && fwrite(d_action.data(), sizeof(float), d_action.size(), f) == d_action.size();
  ok = fclose(f) == 0 && ok;
  if (!ok) return printf("cannot write %s\n", argv[2]), 2;
  printf("rows %d cloned %d\n", count, rows);
  return 0;
}
