// mppi_guide_harness.cpp — a stand-alone host program (g++, no HIP) around ur_gym_amd/csrc/urgym_mppi_guide.h, the header the kernels
// of urgym_mppi_guide.hip compile: tests/test_mppi_guide_host.py compares what it writes with evaluation.mppi_guided_actions and
// mppi_terminal, and runs it a second time built with -fsanitize=address,undefined.  Arrays travel as raw bytes: FILE in, FILE.out out.
//
//   mppi_guide_harness layout                              sizeof and every offsetof of urgym_mppi_guide as the C compiler lays it out, JSON
//   mppi_guide_harness guide FILE H NK K P sigma_bits      in: actions, policy_action, eps f32 [H][NK][6] each; out: actions f32 [H][NK][6]
//   mppi_guide_harness terminal FILE N terminal_value fail_cost_bits
//                                                          in: ret f64 [N], g f64 [N], alive u8 [N], success u8 [N], value f32 [N];
//                                                          out: terminal f64 [N], ret f64 [N], read u8 [N] (1 where value[n] was read)
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../ur_gym_amd/csrc/urgym_mppi_guide.h"

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

#define FIELD(f) printf(", \"%s\": %zu", #f, offsetof(urgym_mppi_guide, f))

static int layout() {
  printf("{\"sizeof\": %zu", sizeof(urgym_mppi_guide));
  FIELD(actor), FIELD(critic), FIELD(policy_samples), FIELD(terminal_value), FIELD(policy_sigma), FIELD(reserved0), FIELD(fail_cost);
  FIELD(policy_action), FIELD(value), FIELD(terminal);
  printf("}\n");
  return 0;
}

// the guide launch of every horizon step, in the kernel's indexing: lane (n, c) of step h
static int guide(char** v) {
  const int H = atoi(v[1]), NK = atoi(v[2]), K = atoi(v[3]), P = atoi(v[4]);
  const float sigma = from_bits<float>(v[5]);
  const size_t count = (size_t)H * NK * 6;
  const std::vector<char> in = slurp(v[0], count * 12);
  const float* actions = (const float*)in.data();
  const float *policy = actions + count, *eps = policy + count;
  std::vector<float> out(actions, actions + count);
  for (int h = 0; h < H; h++)
    for (size_t at = 0; at < (size_t)NK * 6; at++) {
      const int n = (int)(at / 6);
      if (!mppi_guided(mppi_sample(n, K), P)) continue;
      const size_t row = (size_t)h * NK * 6 + at;
      out[row] = mppi_guided_action(policy[row], eps[row], sigma);
    }
  Out(v[0]).put(out);
  return 0;
}

static int terminal(char** v) {
  const size_t N = strtoull(v[1], nullptr, 10);
  const int terminal_value = atoi(v[2]);
  const double fail_cost = from_bits<double>(v[3]);
  const std::vector<char> in = slurp(v[0], N * 22);
  const double* ret = (const double*)in.data();
  const double* g = ret + N;
  const uint8_t *alive = (const uint8_t*)(g + N), *success = alive + N;
  std::vector<float> value(N);  // the bytes after 2 N flags need not be aligned for a float
  memcpy(value.data(), success + N, N * 4);
  std::vector<double> term(N), out(N);
  std::vector<uint8_t> read(N);
  for (size_t n = 0; n < N; n++) {
    const bool reads = mppi_terminal_reads_value(alive[n], terminal_value);
    const double t = mppi_terminal_credit(alive[n], success[n], reads, reads ? value[n] : 0.0f, fail_cost);
    term[n] = t, read[n] = reads;
    out[n] = mppi_terminal_return(ret[n], g[n], t);
  }
  Out o(v[0]);
  o.put(term), o.put(out), o.put(read);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "layout")) return layout();
  if (argc == 8 && !strcmp(argv[1], "guide")) return guide(argv + 2);
  if (argc == 6 && !strcmp(argv[1], "terminal")) return terminal(argv + 2);
  fprintf(stderr, "usage: %s layout | guide FILE H NK K P sigma_bits | terminal FILE N terminal_value fail_cost_bits\n", argv[0]);
  return 2;
}
