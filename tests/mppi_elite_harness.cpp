// mppi_elite_harness.cpp — a stand-alone host program (g++, no HIP) around ur_gym_amd/csrc/urgym_mppi_elite.h, the header the kernels of
// urgym_mppi_elite.hip compile: tests/test_mppi_elite_host.py compares what it writes with evaluation.mppi_elite_rank,
// mppi_elite_weights, mppi_elite_update and mppi_actions, and runs it a second time built with -fsanitize=address,undefined.  Arrays
// travel as raw bytes: FILE in, FILE.out out.
//
//   mppi_elite_harness layout                        sizeof and every offsetof of urgym_mppi_adapt as the C compiler lays it out, JSON
//   mppi_elite_harness rank FILE E K M               in: ret f64 [E][K]; out: rank i32 [E][K], elite u8 [E][K], elite_count i32 [E],
//                                                    threshold f64 [E]
//   mppi_elite_harness weights FILE E K M lam_bits   in: ret f64 [E][K]; out: rmax f64 [E], x f64 [E][K] (the argument of exp; NaN where
//                                                    the weight is fixed), fixed w f64 [E][K] (-1 where exp decides)
//   mppi_elite_harness update FILE H E K shift min_bits max_bits
//                                                    in: w f64 [E][K], actions f32 [H][E K][6]; out: new_mean, mean f32 [H][E][6], ess f64
//                                                    [E], new_std f32 [H][E][6] of mppi_elite_update_host, then new_mean, mean, ess of
//                                                    mppi_update_host on the same input
//   mppi_elite_harness actions FILE COUNT            in: mean, eps, std f32 [COUNT] each; out: action f32 [COUNT]
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../ur_gym_amd/csrc/urgym_mppi_elite.h"

using namespace urgym;

template <class X>
static X from_bits(const char* text) {
  const uint64_t bits = strtoull(text, nullptr, 10);
  X x;
  memcpy(&x, &bits, sizeof(x));
  return x;
}

static std::vector<char> slurp(const char* path, size_t bytes) {
  std::vector<char> data(bytes);
  FILE* f = fopen(path, "rb");
  const bool ok = f && fread(data.data(), 1, bytes, f) == bytes && fgetc(f) == EOF;
  if (f) fclose(f);
  if (!ok) fprintf(stderr, "%s: expected exactly %zu bytes\n", path, bytes), exit(4);
  return data;
}

struct Out {
  FILE* f;
  explicit Out(const char* path) : f(fopen((std::string(path) + ".out").c_str(), "wb")) {
    if (!f) exit(5);
  }
  template <class X>
  void put(const std::vector<X>& v) {
    if (fwrite(v.data(), sizeof(X), v.size(), f) != v.size()) exit(5);
  }
  ~Out() { fclose(f); }
};

#define FIELD(f) printf(", \"%s\": %zu", #f, offsetof(urgym_mppi_adapt, f))

static int layout() {
  printf("{\"sizeof\": %zu, \"alignof\": %zu", sizeof(urgym_mppi_adapt), alignof(urgym_mppi_adapt));
  FIELD(elites), FIELD(adapt_std), FIELD(std_min), FIELD(std_max), FIELD(std), FIELD(new_std), FIELD(rank), FIELD(elite), FIELD(elite_count);
  FIELD(threshold);
  printf("}\n");
  return 0;
}

static int rank(char** v) {
  const int E = atoi(v[1]), K = atoi(v[2]), M = atoi(v[3]);
  const std::vector<char> in = slurp(v[0], (size_t)E * K * 8);
  const double* r = (const double*)in.data();
  std::vector<int32_t> rk((size_t)E * K, -7), count(E, -7);  // every element must be written
  std::vector<uint8_t> elite((size_t)E * K, 0xAB);
  std::vector<double> threshold(E, 7.0);
  for (int p = 0; p < E; p++) {
    const size_t n0 = (size_t)p * K;
    mppi_elite_rank_host(r + n0, K, M, rk.data() + n0, elite.data() + n0, &count[p], &threshold[p]);
  }
  Out o(v[0]);
  o.put(rk), o.put(elite), o.put(count), o.put(threshold);
  return 0;
}

static int weights(char** v) {
  const int E = atoi(v[1]), K = atoi(v[2]), M = atoi(v[3]);
  const double lam = from_bits<double>(v[4]);
  const std::vector<char> in = slurp(v[0], (size_t)E * K * 8);
  const double* r = (const double*)in.data();
  std::vector<double> rmax(E), x((size_t)E * K), fixed((size_t)E * K);
  std::vector<int32_t> rk(K);
  std::vector<uint8_t> elite(K);
  for (int p = 0; p < E; p++) {
    const size_t n0 = (size_t)p * K;
    int32_t count;
    double threshold;
    mppi_elite_rank_host(r + n0, K, M, rk.data(), elite.data(), &count, &threshold);
    double m = -INFINITY;
    for (int j = 0; j < K; j++) m = fmax(m, mppi_max_term(r[n0 + j]));
    rmax[p] = m;
    for (int j = 0; j < K; j++) {
      double w = -1.0;
      const bool is_fixed = mppi_elite_weight_fixed(m, j, elite[j] != 0, w);
      fixed[n0 + j] = is_fixed ? w : -1.0;
      x[n0 + j] = is_fixed ? NAN : mppi_exponent(r[n0 + j], m, lam);
    }
  }
  Out o(v[0]);
  o.put(rmax), o.put(x), o.put(fixed);
  return 0;
}

static int update(char** v) {
  const int H = atoi(v[1]), E = atoi(v[2]), K = atoi(v[3]), shift = atoi(v[4]);
  const float std_min = from_bits<float>(v[5]), std_max = from_bits<float>(v[6]);
  const size_t NK = (size_t)E * K, rows = (size_t)H * E * 6;
  const std::vector<char> in = slurp(v[0], NK * 8 + (size_t)H * NK * 6 * 4);
  const double* w = (const double*)in.data();
  const float* act = (const float*)(w + NK);
  std::vector<float> new_mean(rows, -7.0f), mean(rows, -7.0f), new_std(rows, -7.0f), plain_new_mean(rows, -7.0f), plain_mean(rows, -7.0f);
  std::vector<double> ess(E), plain_ess(E);
  for (int p = 0; p < E; p++) {
    mppi_elite_update_host(w + (size_t)p * K, act, H, K, NK, (size_t)p * K, E, p, shift, std_min, std_max, new_mean.data(), mean.data(), &ess[p], new_std.data());
    mppi_update_host(w + (size_t)p * K, act, H, K, NK, (size_t)p * K, E, p, shift, plain_new_mean.data(), plain_mean.data(), &plain_ess[p]);
  }
  Out o(v[0]);
  o.put(new_mean), o.put(mean), o.put(ess), o.put(new_std), o.put(plain_new_mean), o.put(plain_mean), o.put(plain_ess);
  return 0;
}

static int actions(char** v) {
  const size_t count = strtoull(v[1], nullptr, 10);
  const std::vector<char> in = slurp(v[0], count * 12);
  const float* mean = (const float*)in.data();
  const float *eps = mean + count, *sd = eps + count;
  std::vector<float> a(count);
  for (size_t k = 0; k < count; k++) a[k] = mppi_action(mean[k], eps[k], sd[k]);
  Out(v[0]).put(a);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "layout")) return layout();
  if (argc == 6 && !strcmp(argv[1], "rank")) return rank(argv + 2);
  if (argc == 7 && !strcmp(argv[1], "weights")) return weights(argv + 2);
  if (argc == 9 && !strcmp(argv[1], "update")) return update(argv + 2);
  if (argc == 4 && !strcmp(argv[1], "actions")) return actions(argv + 2);
  fprintf(stderr, "usage: %s layout | rank FILE E K M | weights FILE E K M lam_bits | update FILE H E K shift min_bits max_bits | actions FILE COUNT\n", argv[0]);
  return 2;
}
