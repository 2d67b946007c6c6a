// mppi_temper_harness.cpp — a stand-alone host program (g++, no HIP) around ur_gym_amd/csrc/urgym_mppi_temper.h, the header the kernel of
// urgym_mppi_temper.hip compiles: tests/test_mppi_temper_host.py compares what it writes with evaluation.mppi_temper_exp and
// mppi_temper_solve, and runs it a second time built with -fsanitize=address,undefined.  Arrays travel as raw bytes: FILE in, FILE.out
// out.
//
//   mppi_temper_harness layout             sizeof and every offsetof of urgym_mppi_temper as the C compiler lays it out, JSON
//   mppi_temper_harness exp FILE COUNT     in: x f64 [COUNT]; out: mppi_temper_exp(x) f64 [COUNT]
//   mppi_temper_harness solve FILE E K M target_bits min_bits max_bits STEPS lam_bits
//                                          in: ret f64 [E][K]; M = 0: every finite sample counts, else the M elites of the rank;
//                                          out: lam f64 [E], saturated u8 [E], w f64 [E][K], ess f64 [E] (mppi_update_host's, of w)
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../ur_gym_amd/csrc/urgym_mppi_temper.h"

using namespace urgym;

static double from_bits(const char* text) {
  const uint64_t bits = strtoull(text, nullptr, 10);
  double x;
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

#define FIELD(f) printf(", \"%s\": %zu", #f, offsetof(urgym_mppi_temper, f))

static int layout() {
  printf("{\"sizeof\": %zu, \"alignof\": %zu", sizeof(urgym_mppi_temper), alignof(urgym_mppi_temper));
  FIELD(ess_target), FIELD(lam_min), FIELD(lam_max), FIELD(steps), FIELD(reserved0), FIELD(lam_out), FIELD(saturated);
  printf("}\n");
  return 0;
}

static int exponential(char** v) {
  const size_t count = strtoull(v[1], nullptr, 10);
  const std::vector<char> in = slurp(v[0], count * 8);
  const double* x = (const double*)in.data();
  std::vector<double> y(count, -7.0);
  for (size_t k = 0; k < count; k++) y[k] = mppi_temper_exp(x[k]);
  Out(v[0]).put(y);
  return 0;
}

static int solve(char** v) {
  const int E = atoi(v[1]), K = atoi(v[2]), M = atoi(v[3]), steps = atoi(v[7]);
  const double target = from_bits(v[4]), lam_min = from_bits(v[5]), lam_max = from_bits(v[6]), lam_fixed = from_bits(v[8]);
  const std::vector<char> in = slurp(v[0], (size_t)E * K * 8);
  const double* r = (const double*)in.data();
  std::vector<double> lam(E, -7.0), w((size_t)E * K, -7.0), ess(E, -7.0);  // every element must be written
  std::vector<uint8_t> saturated(E, 0xAB), counted(K);
  std::vector<int32_t> rank(K);
  for (int p = 0; p < E; p++) {
    const size_t n0 = (size_t)p * K;
    if (M > 0) {
      int32_t count;
      double threshold;
      mppi_elite_rank_host(r + n0, K, M, rank.data(), counted.data(), &count, &threshold);
    } else {
      for (int j = 0; j < K; j++) counted[j] = mppi_finite(r[n0 + j]) ? 1 : 0;
    }
    mppi_temper_solve_host(r + n0, counted.data(), K, target, lam_min, lam_max, steps, lam_fixed, &lam[p], &saturated[p], w.data() + n0);
    const double Z = ordered_sum(K, [&](int j) { return w[n0 + j]; });
    const double Q = ordered_sum(K, [&](int j) { return mppi_square_term(w[n0 + j]); });
    ess[p] = mppi_ess(Z, Q);
  }
  Out o(v[0]);
  o.put(lam), o.put(saturated), o.put(w), o.put(ess);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "layout")) return layout();
  if (argc == 4 && !strcmp(argv[1], "exp")) return exponential(argv + 2);
  if (argc == 11 && !strcmp(argv[1], "solve")) return solve(argv + 2);
  fprintf(stderr, "usage: %s layout | exp FILE COUNT | solve FILE E K M target_bits min_bits max_bits STEPS lam_bits\n", argv[0]);
  return 2;
}
