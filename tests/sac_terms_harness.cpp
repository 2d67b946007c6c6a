// Stand-alone host program (tests/test_sac_terms_host.py builds and runs it, once plainly and once with -fsanitize=address,undefined):
// the per-row arithmetic, the ordered sum and the scalar tails of ur_gym_amd/csrc/urgym_sac_terms.h -- the very functions the kernels of
// urgym_sac_terms.hip compile -- run on the host, the ordered sum as a host loop in the stated order (ordered_sum: 1024 "lanes", each
// adding its rows in ascending order, then the fold), for a bitwise comparison with evaluation.entropy_step / policy_terms.
//
//   sac_terms_harness IN OUT
//     IN:  double lr, beta1, beta2, eps; int64 step; int64 count;
//          float alpha, target_entropy, gamma, scale_log_prob, scale_action, l, m, v;
//          uint8 terminated[count]; float log_prob[count], target[count], next_log_prob[count], dqmin_da[count][6], q[2][count],
//          y[count], q_min[count]
//     OUT: double S_entropy, S_q0, S_q1, S_actor (the four ordered sums);
//          float l', m', v', entropy_loss, entropy_mean, critic_loss, actor_loss;
//          float y_out[count], d_log_prob[count], d_action[count][6]
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../ur_gym_amd/csrc/urgym_sac_terms.h"

using namespace urgym;

int main(int argc, char** argv) {
  if (argc != 3) return printf("usage: sac_terms_harness IN OUT\n"), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return printf("cannot open %s\n", argv[1]), 2;
  double hyper[4];
  int64_t step = 0, n = 0;
  float sc[8];
  bool ok = fread(hyper, sizeof(double), 4, f) == 4 && fread(&step, sizeof(step), 1, f) == 1 && fread(&n, sizeof(n), 1, f) == 1 &&
            fread(sc, sizeof(float), 8, f) == 8 && n >= 1 && n <= SAC_TERMS_MAX_COUNT;
  std::vector<uint8_t> terminated;
  std::vector<float> log_prob, target, next_log_prob, dqmin_da, q, y, q_min;
  if (ok) {
    const size_t c = (size_t)n;
    terminated.resize(c), log_prob.resize(c), target.resize(c), next_log_prob.resize(c), dqmin_da.resize(6 * c), q.resize(2 * c), y.resize(c), q_min.resize(c);
    ok = fread(terminated.data(), 1, c, f) == c;
    for (std::vector<float>* x : {&log_prob, &target, &next_log_prob, &dqmin_da, &q, &y, &q_min}) ok = ok && fread(x->data(), sizeof(float), x->size(), f) == x->size();
  }
  fclose(f);
  if (!ok) return printf("short or malformed input %s\n", argv[1]), 2;
  const int count = (int)n;
  const float alpha = sc[0], target_entropy = sc[1], gamma = sc[2], scale_log_prob = sc[3], scale_action = sc[4];
  float l = sc[5], m = sc[6], v = sc[7];

  // urgym_sac_entropy_step: the rows as a lane handles them, then the sum, then the tail
  std::vector<float> y_out(count), d_log_prob(count), d_action(6 * (size_t)count);
  const float up = alpha * scale_log_prob;
  for (int r = 0; r < count; r++) {
    y_out[r] = sac_target_row(target[r], next_log_prob[r], terminated[r] != 0, gamma, alpha);
    d_log_prob[r] = up;
  }
  double S[4];
  S[0] = ordered_sum(count, [&](int r) { return sac_entropy_term(log_prob[r], target_entropy); });
  const float mean = ordered_mean(S[0], count);
  float loss;
  sac_entropy_tail(adam_coefficients(hyper[0], hyper[1], hyper[2], hyper[3], step), mean, l, m, v, loss);

  // urgym_sac_policy_terms
  for (size_t i = 0; i < d_action.size(); i++) d_action[i] = dqmin_da[i] * scale_action;
  S[1] = ordered_sum(count, [&](int r) { return sac_critic_term(q[r], y[r]); });
  S[2] = ordered_sum(count, [&](int r) { return sac_critic_term(q[(size_t)count + r], y[r]); });
  S[3] = ordered_sum(count, [&](int r) { return sac_actor_term(alpha, log_prob[r], q_min[r]); });
  const float critic_loss = sac_critic_loss(ordered_mean(S[1], count), ordered_mean(S[2], count));
  const float actor_loss = ordered_mean(S[3], count);

  f = fopen(argv[2], "wb");
  if (!f) return printf("cannot open %s\n", argv[2]), 2;
  const float scalars[7] = {l, m, v, loss, mean, critic_loss, actor_loss};
  ok = fwrite(S, sizeof(double), 4, f) == 4 && fwrite(scalars, sizeof(float), 7, f) == 7;
  for (std::vector<float>* x : {&y_out, &d_log_prob, &d_action}) ok = ok && fwrite(x->data(), sizeof(float), x->size(), f) == x->size();
  ok = fclose(f) == 0 && ok;
  if (!ok) return printf("cannot write %s\n", argv[2]), 2;
  printf("rows %d\n", count);
  return 0;
}
