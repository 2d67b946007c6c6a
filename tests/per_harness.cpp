// Stand-alone host program (tests/test_per_host.py builds and runs it, once plainly and once with -fsanitize=address,undefined): the
// shape of the sum levels, the ordered block sum, the descent and the beta schedule of ur_gym_amd/csrc/urgym_per.h -- the very
// functions the kernels of urgym_per.hip compile -- run on the host the way the kernels run them, for a bitwise comparison with
// evaluation.per_sums / per_descent / per_beta.  F is the fan-out, 4 or 256.
//
//   per_harness sums F IN OUT
//     IN:  int64 n; float leaf[n]
//     OUT: double sums[doubles]: level 1, level 2, ..., the total
//   per_harness descend F IN OUT
//     IN:  int64 n, count, given; float leaf[n]; if given: double sums[doubles] (a hand-built tree), else they are formed; uint64 w[count]
//     OUT: int64 entry[count]
//   per_harness beta IN OUT
//     IN:  int64 count; per row: double beta0; int64 step, beta_steps
//     OUT: float beta[count]
//   per_harness layout            sizeof and offsets of the three structs of include/urgym.h, as JSON
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/urgym.h"
#include "../ur_gym_amd/csrc/urgym_per.h"

using namespace urgym;

static_assert(URGYM_PER_FANOUT == PER_FANOUT && URGYM_PER_TERMS_MAX_COUNT == PER_TERMS_MAX_COUNT, "include/urgym.h");

template <class T>
static bool read_all(FILE* f, std::vector<T>& v) {
  return fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

template <class T>
static int write_all(const char* out, const std::vector<T>& v) {
  FILE* f = fopen(out, "wb");
  if (!f) return printf("cannot open %s\n", out), 2;
  bool ok = fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
  ok = fclose(f) == 0 && ok;
  if (!ok) return printf("cannot write %s\n", out), 2;
  printf("rows %zu\n", v.size());
  return 0;
}

// what urgym_per_rebuild's two launches do: level 1 from the leaves, every level above from the one below, the total
template <int F>
static std::vector<double> build(const std::vector<float>& leaf) {
  const PerShape s = per_shape<F>((int64_t)leaf.size());
  std::vector<double> sums((size_t)s.doubles);
  for (int64_t b = 0; b < s.count[1]; b++) sums.at((size_t)b) = per_block_sum<F>(leaf.data(), s.count[0], b);
  for (int k = 2; k <= s.levels; k++)
    for (int64_t b = 0; b < s.count[k]; b++) sums.at((size_t)(s.offset[k] + b)) = per_block_sum<F>(sums.data() + s.offset[k - 1], s.count[k - 1], b);
  sums.at((size_t)s.doubles - 1) = per_ordered_sum(sums.data() + s.offset[s.levels], 0, (int)s.count[s.levels]);
  return sums;
}

template <int F>
static int sums(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  if (!f) return printf("cannot open %s\n", in), 2;
  int64_t n = 0;
  bool ok = fread(&n, sizeof(n), 1, f) == 1 && n >= 1 && n <= (1 << 24);
  std::vector<float> leaf;
  if (ok) leaf.resize((size_t)n), ok = read_all(f, leaf);
  fclose(f);
  if (!ok) return printf("short or malformed input %s\n", in), 2;
  return write_all(out, build<F>(leaf));
}

template <int F>
static int descend(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  if (!f) return printf("cannot open %s\n", in), 2;
  int64_t head[3] = {0, 0, 0};
  bool ok = fread(head, sizeof(int64_t), 3, f) == 3 && head[0] >= 1 && head[0] <= (1 << 24) && head[1] >= 1 && head[1] <= (1 << 20);
  std::vector<float> leaf;
  std::vector<double> tree;
  std::vector<uint64_t> w;
  PerShape s = per_shape<F>(ok ? head[0] : 1);
  if (ok) {
    leaf.resize((size_t)head[0]), w.resize((size_t)head[1]);
    ok = read_all(f, leaf);
    if (ok && head[2]) tree.resize((size_t)s.doubles), ok = read_all(f, tree);
    ok = ok && read_all(f, w);
  }
  fclose(f);
  if (!ok) return printf("short or malformed input %s\n", in), 2;
  if (!head[2]) tree = build<F>(leaf);
  std::vector<int64_t> entry(w.size());
  for (size_t i = 0; i < w.size(); i++) {
    // what the sample's lane of per_gather_kernel does with its word
    entry[i] = per_descend<F>(s, leaf.data(), tree.data(), tree.at((size_t)s.doubles - 1), w[i]);
    if (entry[i] < 0 || entry[i] >= head[0]) return printf("entry %lld outside the leaves\n", (long long)entry[i]), 3;
  }
  return write_all(out, entry);
}

static int beta(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  if (!f) return printf("cannot open %s\n", in), 2;
  int64_t count = 0;
  bool ok = fread(&count, sizeof(count), 1, f) == 1 && count >= 1 && count <= (1 << 20);
  std::vector<float> b(ok ? (size_t)count : 0);
  for (size_t i = 0; ok && i < b.size(); i++) {
    double beta0 = 0.0;
    int64_t at[2] = {0, 0};
    ok = fread(&beta0, sizeof(beta0), 1, f) == 1 && fread(at, sizeof(int64_t), 2, f) == 2 && at[1] >= 1;
    if (ok) b[i] = per_beta(beta0, at[0], at[1]);
  }
  fclose(f);
  if (!ok) return printf("short or malformed input %s\n", in), 2;
  return write_all(out, b);
}

#define FIELD(s, m) printf(", \"%s\": %zu", #m, offsetof(s, m))

static int layout() {
  printf("{\"urgym_per_priorities\": {\"sizeof\": %zu", sizeof(urgym_per_priorities));
  FIELD(urgym_per_priorities, capacity_steps), FIELD(urgym_per_priorities, reserved0), FIELD(urgym_per_priorities, leaf);
  FIELD(urgym_per_priorities, sums), FIELD(urgym_per_priorities, max_leaf);
  printf("}, \"urgym_per_terms_args\": {\"sizeof\": %zu", sizeof(urgym_per_terms_args));
  FIELD(urgym_per_terms_args, count), FIELD(urgym_per_terms_args, reserved0), FIELD(urgym_per_terms_args, size), FIELD(urgym_per_terms_args, beta);
  FIELD(urgym_per_terms_args, alpha), FIELD(urgym_per_terms_args, eps), FIELD(urgym_per_terms_args, scale), FIELD(urgym_per_terms_args, reserved1);
  FIELD(urgym_per_terms_args, leaf_in), FIELD(urgym_per_terms_args, total), FIELD(urgym_per_terms_args, q), FIELD(urgym_per_terms_args, y);
  FIELD(urgym_per_terms_args, w_raw), FIELD(urgym_per_terms_args, w), FIELD(urgym_per_terms_args, dq), FIELD(urgym_per_terms_args, index);
  FIELD(urgym_per_terms_args, new_leaf), FIELD(urgym_per_terms_args, priorities);
  printf("}, \"urgym_sac_prioritized\": {\"sizeof\": %zu", sizeof(urgym_sac_prioritized));
  FIELD(urgym_sac_prioritized, priorities), FIELD(urgym_sac_prioritized, beta0), FIELD(urgym_sac_prioritized, beta_steps), FIELD(urgym_sac_prioritized, alpha);
  FIELD(urgym_sac_prioritized, eps), FIELD(urgym_sac_prioritized, leaf), FIELD(urgym_sac_prioritized, total), FIELD(urgym_sac_prioritized, q);
  FIELD(urgym_sac_prioritized, w_raw), FIELD(urgym_sac_prioritized, w), FIELD(urgym_sac_prioritized, dq), FIELD(urgym_sac_prioritized, new_leaf);
  FIELD(urgym_sac_prioritized, reserved0);
  printf("}}\n");
  return 0;
}

int main(int argc, char** argv) {
  const int F = argc == 5 ? atoi(argv[2]) : 0;
  if (argc == 5 && !strcmp(argv[1], "sums") && F == 4) return sums<4>(argv[3], argv[4]);
  if (argc == 5 && !strcmp(argv[1], "sums") && F == 256) return sums<256>(argv[3], argv[4]);
  if (argc == 5 && !strcmp(argv[1], "descend") && F == 4) return descend<4>(argv[3], argv[4]);
  if (argc == 5 && !strcmp(argv[1], "descend") && F == 256) return descend<256>(argv[3], argv[4]);
  if (argc == 4 && !strcmp(argv[1], "beta")) return beta(argv[2], argv[3]);
  if (argc == 2 && !strcmp(argv[1], "layout")) return layout();
  return printf("usage: per_harness sums|descend F IN OUT | beta IN OUT | layout\n"), 2;
}
