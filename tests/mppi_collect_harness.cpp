// mppi_collect_harness.cpp — a stand-alone host program (g++, no HIP) around ur_gym_amd/csrc/urgym_mppi_collect.h, the header the kernel
// of urgym_mppi_collect.hip compiles: tests/test_mppi_collect_host.py compares what it writes with evaluation.mppi_explore_counters and
// mppi_execute, and runs it a second time built with -fsanitize=address,undefined.  Arrays travel as raw bytes: FILE in, FILE.out out.
//
//   mppi_collect_harness layout                     sizeof and every offsetof of urgym_mppi_explore as the C compiler lays it out, JSON
//   mppi_collect_harness counter P DRAW             the two exploration counters of (P, DRAW), and for every component c the block and the
//                                                   first word its pair reads, JSON
//   mppi_collect_harness meet P DRAW                how many of the planner's sample counters (i < 8, h < 64, j < 1024, block 0, 1, parent P,
//                                                   draw DRAW) equal one of the two exploration counters of (P, DRAW): JSON {"compared", "met"}
//   mppi_collect_harness execute FILE E sigma_bits  in: action_out, eps f32 [E][6] each; out: executed f32 [E][6], explore_eps f32 [E][6],
//                                                   drew u8 [E][6] (1 where the lane would draw a Philox word)
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../ur_gym_amd/csrc/urgym_mppi_collect.h"

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

#define FIELD(f) printf(", \"%s\": %zu", #f, offsetof(urgym_mppi_explore, f))

static int layout() {
  printf("{\"sizeof\": %zu", sizeof(urgym_mppi_explore));
  FIELD(explore_sigma), FIELD(reserved0), FIELD(explore_eps);
  printf("}\n");
  return 0;
}

static bool same(const MppiCounter& a, const MppiCounter& b) { return a.c0 == b.c0 && a.c1 == b.c1 && a.c2 == b.c2 && a.c3 == b.c3; }

static int counter(char** v) {
  const int p = atoi(v[0]);
  const uint64_t draw = strtoull(v[1], nullptr, 10);
  printf("{\"counters\": [");
  for (uint32_t b = 0; b < 2; b++) {
    const MppiCounter k = mppi_explore_counter(p, draw, MPPI_EXPLORE_BLOCK + b);
    printf("%s[%u, %u, %u, %u]", b ? ", " : "", k.c0, k.c1, k.c2, k.c3);
  }
  printf("], \"block_of\": [");
  for (int c = 0; c < 6; c++) printf("%s%u", c ? ", " : "", mppi_explore_block_of(c));
  printf("], \"first_word\": [");
  for (int c = 0; c < 6; c++) printf("%s%d", c ? ", " : "", mppi_explore_first_word(c));
  printf("]}\n");
  return 0;
}

static int meet(char** v) {
  const int p = atoi(v[0]);
  const uint64_t draw = strtoull(v[1], nullptr, 10);
  const MppiCounter x2 = mppi_explore_counter(p, draw, MPPI_EXPLORE_BLOCK), x3 = mppi_explore_counter(p, draw, MPPI_EXPLORE_BLOCK + 1);
  long compared = 0, met = 0;
  for (int i = 0; i < URGYM_MPPI_ITERATIONS_MAX; i++)
    for (int h = 0; h < URGYM_MPPI_HORIZON_MAX; h++)
      for (int j = 0; j < URGYM_MPPI_SAMPLES_MAX; j++)
        for (uint32_t b = 0; b < 2; b++) {
          const MppiCounter k = mppi_counter(p, i, h, j, draw, b);
          compared += 2;
          met += same(k, x2) + same(k, x3);
        }
  printf("{\"compared\": %ld, \"met\": %ld}\n", compared, met);
  return 0;
}

// the execute launch in the kernel's indexing: lane at = p * 6 + c
static int execute(char** v) {
  const size_t E = strtoull(v[1], nullptr, 10);
  const float sigma = from_bits<float>(v[2]);
  const size_t count = E * 6;
  const std::vector<char> in = slurp(v[0], count * 8);
  const float* action_out = (const float*)in.data();
  const float* eps = action_out + count;
  std::vector<float> executed(count), explore_eps(count);
  std::vector<uint8_t> drew(count);
  for (size_t at = 0; at < count; at++) {
    if (mppi_execute_copies(sigma)) {
      memcpy(&executed[at], &action_out[at], 4);  // 32 bits, whatever they mean
      explore_eps[at] = 0.0f, drew[at] = 0;
      continue;
    }
    executed[at] = mppi_executed(action_out[at], eps[at], sigma);
    explore_eps[at] = eps[at], drew[at] = 1;
  }
  Out o(v[0]);
  o.put(executed), o.put(explore_eps), o.put(drew);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "layout")) return layout();
  if (argc == 4 && !strcmp(argv[1], "counter")) return counter(argv + 2);
  if (argc == 4 && !strcmp(argv[1], "meet")) return meet(argv + 2);
  if (argc == 5 && !strcmp(argv[1], "execute")) return execute(argv + 2);
  fprintf(stderr, "usage: %s layout | counter P DRAW | meet P DRAW | execute FILE E sigma_bits\n", argv[0]);
  return 2;
}
