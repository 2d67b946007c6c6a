// Stand-alone host program (tests/test_sac_bc_weighted_host.py builds and runs it, once plainly and once with
// -fsanitize=address,undefined): the advantage weight of ur_gym_amd/csrc/urgym_sac_bc.h -- the very functions the kernel of
// urgym_sac_bc_weighted.hip compiles, the float64 exponential of urgym_mppi_temper.h among them -- with the ordered sums of
// urgym_sac_terms.h as host loops in the stated order, in the kernel's three sweeps, for a bitwise comparison with
// evaluation.policy_terms_weighted.
//
//   sac_bc_weighted_harness layout      sizeof and every offsetof of urgym_sac_advantage_args and urgym_sac_weighting as the C compiler lays
//                                       them out, JSON
//   sac_bc_weighted_harness IN OUT
//     IN:  int64 count; int32 scale_by_q, masked; float alpha, scale, weight, bc_scale, temperature, max_weight;
//          float log_prob[count], q[2][count], y[count], q_min[count], dqmin_da[count][6], action_pi[count][6], action_data[count][6];
//          uint8 row_mask[count] (read always, used with masked)
//     OUT: double S_q0, S_q1, S_actor, S_absq, Z, Q, S_ah (the seven ordered sums);
//          float critic_loss, actor_loss, bc_loss, w, mean_abs, adv_ess, adv_max; int32 n, clipped; uint8 eligible[count]; float a[count];
//          float d_action[count][6]
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
  printf("{\"urgym_sac_advantage_args\": {\"sizeof\": %zu", sizeof(urgym_sac_advantage_args));
  FIELD(urgym_sac_advantage_args, temperature), FIELD(urgym_sac_advantage_args, max_weight), FIELD(urgym_sac_advantage_args, row_mask);
  FIELD(urgym_sac_advantage_args, adv_ess_out), FIELD(urgym_sac_advantage_args, adv_max_out), FIELD(urgym_sac_advantage_args, adv_clipped_out);
  FIELD(urgym_sac_advantage_args, reserved0);
  printf("}, \"urgym_sac_weighting\": {\"sizeof\": %zu", sizeof(urgym_sac_weighting));
  FIELD(urgym_sac_weighting, temperature), FIELD(urgym_sac_weighting, max_weight), FIELD(urgym_sac_weighting, reserved0);
  FIELD(urgym_sac_weighting, adv_ess), FIELD(urgym_sac_weighting, adv_max), FIELD(urgym_sac_weighting, adv_clipped);
  printf("}}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "layout")) return layout();
  if (argc != 3) return printf("usage: sac_bc_weighted_harness layout | IN OUT\n"), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return printf("cannot open %s\n", argv[1]), 2;
  int64_t n64 = 0;
  int32_t flags[2];
  float sc[6];
  bool ok = fread(&n64, sizeof(n64), 1, f) == 1 && fread(flags, sizeof(int32_t), 2, f) == 2 && fread(sc, sizeof(float), 6, f) == 6 && n64 >= 1 && n64 <= SAC_TERMS_MAX_COUNT;
  std::vector<float> log_prob, q, y, q_min, dqmin_da, action_pi, action_data;
  std::vector<uint8_t> row_mask;
  if (ok) {
    const size_t c = (size_t)n64;
    log_prob.resize(c), q.resize(2 * c), y.resize(c), q_min.resize(c), dqmin_da.resize(6 * c), action_pi.resize(6 * c), action_data.resize(6 * c), row_mask.resize(c);
    for (std::vector<float>* x : {&log_prob, &q, &y, &q_min, &dqmin_da, &action_pi, &action_data}) ok = ok && fread(x->data(), sizeof(float), x->size(), f) == x->size();
    ok = ok && fread(row_mask.data(), 1, c, f) == c;
  }
  fclose(f);
  if (!ok) return printf("short or malformed input %s\n", argv[1]), 2;
  const int count = (int)n64;
  const bool scale_by_q = flags[0] != 0, masked = flags[1] != 0;
  const float alpha = sc[0], scale = sc[1], weight = sc[2], bc_scale = sc[3], temperature = sc[4], max_weight = sc[5];

  auto advantage = [&](int r) { return sac_adv_advantage(sac_bc_q_data(q[r], q[(size_t)count + r]), q_min[r]); };
  auto eligible_row = [&](int r) { return sac_adv_eligible(masked, masked ? row_mask[r] : (uint8_t)1, advantage(r)); };

  // sweep 1: A_max and n
  float a_max = -INFINITY;
  int32_t n = 0;
  std::vector<uint8_t> eligible(count);
  for (int r = 0; r < count; r++) {
    eligible[r] = eligible_row(r);
    a_max = sac_adv_max(a_max, sac_adv_max_term(eligible[r] != 0, advantage(r)));
    n += eligible[r];
  }

  // sweep 2: the four sums of the cloned call, Z and Q
  auto e_row = [&](int r) { return sac_adv_e(advantage(r), a_max, temperature, eligible_row(r)); };
  double S[7];
  S[0] = ordered_sum(count, [&](int r) { return sac_critic_term(q[r], y[r]); });
  S[1] = ordered_sum(count, [&](int r) { return sac_critic_term(q[(size_t)count + r], y[r]); });
  S[2] = ordered_sum(count, [&](int r) { return sac_actor_term(alpha, log_prob[r], q_min[r]); });
  S[3] = ordered_sum(count, [&](int r) { return fabsf(q_min[r]); });
  S[4] = ordered_sum(count, [&](int r) { return e_row(r); });
  S[5] = ordered_sum(count, [&](int r) { return mppi_square_term(e_row(r)); });
  const float mean_abs = ordered_mean(S[3], count);
  const float w = sac_bc_weight(scale_by_q, weight, mean_abs);
  const double mean_e = n > 0 ? sac_adv_mean_e(S[4], n) : 1.0;

  // sweep 3: the weights, the weighted loss, the rows the cap held, and the elements
  std::vector<float> a(count), d_action(6 * (size_t)count);
  int32_t clipped = 0;
  for (int r = 0; r < count; r++) {
    a[r] = 0.0f;
    if (!eligible_row(r)) continue;
    bool over;
    a[r] = sac_adv_row_weight(e_row(r), mean_e, max_weight, over);
    clipped += over ? 1 : 0;
  }
  S[6] = ordered_sum(count, [&](int r) { return eligible_row(r) ? sac_adv_term(a[r], sac_bc_term(&action_pi[(size_t)r * 6], &action_data[(size_t)r * 6])) : 0.0f; });
  for (size_t i = 0; i < d_action.size(); i++) {
    const int r = (int)(i / 6);
    const float g = dqmin_da[i] * scale;
    d_action[i] = eligible_row(r) ? sac_bc_upstream(g, sac_bc_difference(action_pi[i], action_data[i]), sac_adv_element_weight(w, a[r]), bc_scale) : g;
  }
  bool over = false;
  const float adv_ess = n > 0 ? sac_adv_ess(S[4], S[5]) : 0.0f;
  const float adv_max = n > 0 ? sac_adv_row_weight(1.0, mean_e, max_weight, over) : 0.0f;

  f = fopen(argv[2], "wb");
  if (!f) return printf("cannot open %s\n", argv[2]), 2;
  const float scalars[7] = {sac_critic_loss(ordered_mean(S[0], count), ordered_mean(S[1], count)), ordered_mean(S[2], count), ordered_mean(S[6], count), w, mean_abs, adv_ess, adv_max};
  const int32_t counts[2] = {n, clipped};
  ok = fwrite(S, sizeof(double), 7, f) == 7 && fwrite(scalars, sizeof(float), 7, f) == 7 && fwrite(counts, sizeof(int32_t), 2, f) == 2 &&
       fwrite(eligible.data(), 1, eligible.size(), f) == eligible.size() && fwrite(a.data(), sizeof(float), a.size(), f) == a.size() &&
       fwrite(d_action.data(), sizeof(float), d_action.size(), f) == d_action.size();
  ok = fclose(f) == 0 && ok;
  if (!ok) return printf("cannot write %s\n", argv[2]), 2;
  printf("rows %d eligible %d clipped %d\n", count, n, clipped);
  return 0;
}
