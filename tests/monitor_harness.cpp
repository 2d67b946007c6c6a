// monitor_harness.cpp — a stand-alone host program (g++, no HIP) around ur_gym_amd/csrc/urgym_monitor.h, the header the kernels of
// urgym_monitor.hip and urgym_sac_train_monitored compile: tests/test_monitor_host.py compares what it prints with
// evaluation.monitor_fold, evaluation.monitor_stats and evaluation.monitor_points, and runs it a second time built with
// -fsanitize=address,undefined.
//
//   monitor_harness run STATE_IN STATE_OUT N C op...
//       STATE_IN holds the six state arrays of N envs back to back, in urgym_monitor_state's order; STATE_OUT receives them afterwards.
//       The ops run in order:  ring:FILE   loads a ring of C slots: reward float32 [C][N], then terminated, truncated, is_success
//                                          uint8 [C][N]
//                              fold:FIRST:K    monitor_fold_host
//                              stats:ITERATION:CLEAR   monitor_stats_host; prints the record
//       One JSON list of the records, floats as the 64-bit words they are
//   monitor_harness points first_iteration num_iterations steps_per_iteration capacity_steps log_every first_record record_capacity
//       one JSON object: the iterations followed by a record (walked with monitor_record_follows), monitor_record_count, and what
//       monitor_schedule_refusal says
//   monitor_harness layout
//       sizeof and every offsetof of the three new structs as the C compiler lays them out, one JSON object
#include <inttypes.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../ur_gym_amd/csrc/urgym_monitor.h"

using namespace urgym;

static uint64_t word(double x) {
  uint64_t w;
  memcpy(&w, &x, sizeof(w));
  return w;
}

template <class T>
static bool io(FILE* f, std::vector<T>& v, bool write) {
  return (write ? fwrite(v.data(), sizeof(T), v.size(), f) : fread(v.data(), sizeof(T), v.size(), f)) == v.size();
}

struct HostState {
  std::vector<double> running_return, sum_return;
  std::vector<int32_t> running_length, episodes, successes;
  std::vector<int64_t> sum_length;
  explicit HostState(size_t n) : running_return(n), sum_return(n), running_length(n), episodes(n), successes(n), sum_length(n) {}
  bool file(const char* path, bool write) {
    FILE* f = fopen(path, write ? "wb" : "rb");
    if (!f) return false;
    const bool ok = io(f, running_return, write) && io(f, running_length, write) && io(f, sum_return, write) && io(f, sum_length, write) &&
                    io(f, episodes, write) && io(f, successes, write);
    fclose(f);
    return ok;
  }
  urgym_monitor_state pointers() { return urgym_monitor_state{running_return.data(), running_length.data(), sum_return.data(), sum_length.data(), episodes.data(), successes.data()}; }
};

static int run(int argc, char** v) {
  const int n = atoi(v[2]), cap = atoi(v[3]);
  if (n < 1 || cap < 1) return 3;
  const size_t entries = (size_t)n * (size_t)cap;
  HostState st((size_t)n);
  if (!st.file(v[0], false)) return 4;
  std::vector<float> reward(entries);
  std::vector<uint8_t> terminated(entries), truncated(entries), is_success(entries);
  bool have_ring = false;
  const char* sep = "";
  printf("[");
  for (int i = 4; i < argc; i++) {
    char* op = v[i];
    if (!strncmp(op, "ring:", 5)) {
      FILE* f = fopen(op + 5, "rb");
      if (!f) return 5;
      have_ring = io(f, reward, false) && io(f, terminated, false) && io(f, truncated, false) && io(f, is_success, false);
      fclose(f);
      if (!have_ring) return 6;
    } else if (!strncmp(op, "fold:", 5)) {
      char* end;
      const int first = (int)strtol(op + 5, &end, 10);
      const int steps = (int)strtol(end + 1, nullptr, 10);
      if (!have_ring || first < 0 || first >= cap || steps < 1 || steps > cap) return 7;  // what the entry point refuses
      monitor_fold_host(st.pointers(), reward.data(), terminated.data(), truncated.data(), is_success.data(), n, cap, first, steps);
    } else if (!strncmp(op, "stats:", 6)) {
      char* end;
      const int64_t iteration = strtoll(op + 6, &end, 10);
      const int clear = (int)strtol(end + 1, nullptr, 10);
      urgym_monitor_record rec;
      monitor_stats_host(st.pointers(), n, iteration, clear, rec);
      printf("%s{\"mean_return\": %" PRIu64 ", \"mean_length\": %" PRIu64 ", \"success_rate\": %" PRIu64 ", \"sum_return\": %" PRIu64 ", \"episodes\": %" PRId64
             ", \"length_sum\": %" PRId64 ", \"successes\": %" PRId64 ", \"iteration\": %" PRId64 ", \"reserved0\": %" PRId64 "}",
             sep, word(rec.mean_return), word(rec.mean_length), word(rec.success_rate), word(rec.sum_return), rec.episodes, rec.length_sum, rec.successes,
             rec.iteration, rec.reserved0);
      sep = ", ";
    } else {
      return 8;
    }
  }
  printf("]\n");
  return st.file(v[1], true) ? 0 : 9;
}

static int points(char** v) {
  urgym_sac_schedule s;
  memset(&s, 0, sizeof(s));
  const int64_t first_iteration = strtoll(v[0], nullptr, 10);
  s.num_iterations = (int32_t)strtoll(v[1], nullptr, 10);
  s.steps_per_iteration = (int32_t)strtoll(v[2], nullptr, 10);
  s.capacity_steps = (int32_t)strtoll(v[3], nullptr, 10);
  const int32_t every = (int32_t)strtoll(v[4], nullptr, 10), first_record = (int32_t)strtoll(v[5], nullptr, 10), capacity = (int32_t)strtoll(v[6], nullptr, 10);
  const char* refusal = monitor_schedule_refusal(s, every, first_iteration, first_record, capacity);
  printf("{\"refused\": ");
  if (refusal)
    printf("\"%s\"", refusal);
  else
    printf("null");
  printf(", \"points\": [");
  const bool sound = every >= 1 && first_iteration >= 0 && first_iteration <= INT64_MAX - s.num_iterations;
  if (sound) {
    bool first = true;
    for (int32_t i = 0; i < s.num_iterations; i++)
      if (monitor_record_follows(first_iteration, every, i)) printf("%s%d", first ? "" : ", ", i), first = false;
  }
  printf("], \"count\": %" PRId64 "}\n", sound ? monitor_record_count(first_iteration, every, s.num_iterations) : (int64_t)-1);
  return 0;
}

#define BEGIN(T) printf("%s\"%s\": {\"sizeof\": %zu", sep, #T, sizeof(T)), sep = ", "
#define FIELD(T, f) printf(", \"%s\": %zu", #f, offsetof(T, f))
#define END() printf("}")

static int layout() {
  const char* sep = "";
  printf("{");
  BEGIN(urgym_monitor_state);
  FIELD(urgym_monitor_state, running_return), FIELD(urgym_monitor_state, running_length), FIELD(urgym_monitor_state, sum_return);
  FIELD(urgym_monitor_state, sum_length), FIELD(urgym_monitor_state, episodes), FIELD(urgym_monitor_state, successes);
  END();
  BEGIN(urgym_monitor_record);
  FIELD(urgym_monitor_record, mean_return), FIELD(urgym_monitor_record, mean_length), FIELD(urgym_monitor_record, success_rate);
  FIELD(urgym_monitor_record, sum_return), FIELD(urgym_monitor_record, episodes), FIELD(urgym_monitor_record, length_sum);
  FIELD(urgym_monitor_record, successes), FIELD(urgym_monitor_record, iteration), FIELD(urgym_monitor_record, reserved0);
  END();
  BEGIN(urgym_sac_monitoring);
  FIELD(urgym_sac_monitoring, state), FIELD(urgym_sac_monitoring, records), FIELD(urgym_sac_monitoring, record_capacity);
  FIELD(urgym_sac_monitoring, first_record), FIELD(urgym_sac_monitoring, log_every), FIELD(urgym_sac_monitoring, clear);
  FIELD(urgym_sac_monitoring, first_iteration), FIELD(urgym_sac_monitoring, reserved0);
  END();
  printf("}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "layout")) return layout();
  if (argc >= 6 && !strcmp(argv[1], "run")) return run(argc - 2, argv + 2);
  if (argc == 9 && !strcmp(argv[1], "points")) return points(argv + 2);
  fprintf(stderr, "usage: %s layout | run STATE_IN STATE_OUT N C op... | points first_iteration n K C log_every first_record capacity\n", argv[0]);
  return 2;
}
