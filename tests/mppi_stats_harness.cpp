// mppi_stats_harness.cpp — a stand-alone host program (g++, no HIP) around ur_gym_amd/csrc/urgym_mppi_stats.h, the header the kernel of
// urgym_mppi_stats.hip compiles: tests/test_mppi_train_host.py compares the record it writes with evaluation.mppi_plan_stats, and runs it
// a second time built with -fsanitize=address,undefined.
//
//   mppi_stats_harness stats IN OUT E ADAPTIVE ITERATION
//       IN holds best_return, nominal_return and ess, float64 [E] each, back to back, and with ADAPTIVE != 0 elite_count int32 [E] and
//       threshold float64 [E] after them; OUT receives the bytes of the one urgym_mppi_stats_record mppi_stats_host writes
//   mppi_stats_harness layout
//       sizeof and every offsetof of the two new structs as the C compiler lays them out, one JSON object
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../ur_gym_amd/csrc/urgym_mppi_stats.h"

using namespace urgym;

template <class T>
static bool load(FILE* f, std::vector<T>& v) {
  return fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

static int stats(char** v) {
  const int E = atoi(v[2]), adaptive = atoi(v[3]);
  const int64_t iteration = strtoll(v[4], nullptr, 10);
  if (E < 1 || E > SAC_TERMS_MAX_COUNT) return 3;  // what the entry point refuses
  const size_t n = (size_t)E;
  std::vector<double> best(n), nominal(n), ess(n), threshold(n);
  std::vector<int32_t> elite_count(n);
  FILE* f = fopen(v[0], "rb");
  if (!f) return 4;
  bool ok = load(f, best) && load(f, nominal) && load(f, ess);
  if (ok && adaptive) ok = load(f, elite_count) && load(f, threshold);
  fclose(f);
  if (!ok) return 5;
  urgym_mppi_stats_record rec;
  memset(&rec, 0xA5, sizeof(rec));  // the host loop writes every field
  mppi_stats_host(E, best.data(), nominal.data(), ess.data(), adaptive ? elite_count.data() : nullptr, adaptive ? threshold.data() : nullptr, iteration, rec);
  f = fopen(v[1], "wb");
  if (!f) return 6;
  ok = fwrite(&rec, sizeof(rec), 1, f) == 1;
  fclose(f);
  return ok ? 0 : 7;
}

#define BEGIN(T) printf("%s\"%s\": {\"sizeof\": %zu", sep, #T, sizeof(T)), sep = ", "
#define FIELD(T, f) printf(", \"%s\": %zu", #f, offsetof(T, f))
#define END() printf("}")

static int layout() {
  const char* sep = "";
  printf("{");
  BEGIN(urgym_mppi_stats_record);
  FIELD(urgym_mppi_stats_record, mean_best_return), FIELD(urgym_mppi_stats_record, mean_nominal_return), FIELD(urgym_mppi_stats_record, mean_gain);
  FIELD(urgym_mppi_stats_record, mean_ess), FIELD(urgym_mppi_stats_record, min_ess), FIELD(urgym_mppi_stats_record, mean_elite_count);
  FIELD(urgym_mppi_stats_record, mean_threshold), FIELD(urgym_mppi_stats_record, iteration), FIELD(urgym_mppi_stats_record, num_parents);
  FIELD(urgym_mppi_stats_record, planned), FIELD(urgym_mppi_stats_record, nominal_finite), FIELD(urgym_mppi_stats_record, gain_count);
  FIELD(urgym_mppi_stats_record, threshold_count), FIELD(urgym_mppi_stats_record, reserved0);
  END();
  BEGIN(urgym_sac_planning);
  FIELD(urgym_sac_planning, planner_handle), FIELD(urgym_sac_planning, mppi), FIELD(urgym_sac_planning, adapt_or_NULL);
  FIELD(urgym_sac_planning, guide_or_NULL), FIELD(urgym_sac_planning, explore), FIELD(urgym_sac_planning, sync);
  FIELD(urgym_sac_planning, record_capacity), FIELD(urgym_sac_planning, records), FIELD(urgym_sac_planning, reserved0);
  END();
  printf("}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "layout")) return layout();
  if (argc == 7 && !strcmp(argv[1], "stats")) return stats(argv + 2);
  fprintf(stderr, "usage: %s layout | stats IN OUT E ADAPTIVE ITERATION\n", argv[0]);
  return 2;
}
