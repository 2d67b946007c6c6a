// urgym_monitor.hip — training-episode statistics on the device (include/urgym.h, urgym_monitor_fold / urgym_monitor_stats; DESIGN.md
// section 19): the return, the length and the success of the episodes the collecting policy itself finishes, followed across steps and
// calls from the replay ring the collection has just written, so that a training call reports its own curve without a copy of the
// [K][N] flags to the host.
//
// monitor_fold_kernel is one lane per env, 256 lanes per workgroup: the six state words of env n are read once, the K steps run in a
// loop whose loads are contiguous over n within a slot, the state is written once.  A lane touches nothing of another env.
//
// monitor_stats_kernel is ONE launch of ONE workgroup of 1024 lanes, in the structure of eval_stats_kernel (urgym_eval.hip): lane t
// handles envs t, t + 1024, ..., the float64 partial and the three int64 partials are folded through LDS with a barrier per level, the
// scalar tail runs on lane 0.  With `clear` each lane zeroes the interval entries it has read itself: an entry belongs to one lane.
// No atomics: the order of every sum depends on nothing but N.
//
// This unit is built with -ffp-contract=off: every line of urgym_monitor.h is one operation rounded on its own.  Division is the
// correctly rounded one.
#include <hip/hip_runtime.h>

#include "urgym_monitor.h"

namespace urgym {

namespace {

constexpr int FOLD_LANES = 256;

__global__ void __launch_bounds__(FOLD_LANES) monitor_fold_kernel(const MonitorFoldCall P) {
  const int n = blockIdx.x * FOLD_LANES + threadIdx.x;
  if (n >= P.num_envs) return;
  const urgym_monitor_state& st = P.state;
  MonitorLane m{st.running_return[n], st.running_length[n], st.sum_return[n], st.sum_length[n], st.episodes[n], st.successes[n]};
  for (int k = 0; k < P.num_steps; k++) {
    const size_t at = monitor_entry(P.first_slot, k, P.capacity, P.num_envs, n);
    monitor_step(m, P.reward[at], P.terminated[at], P.truncated[at], P.is_success[at]);
  }
  st.running_return[n] = m.running_return, st.running_length[n] = m.running_length, st.sum_return[n] = m.sum_return;
  st.sum_length[n] = m.sum_length, st.episodes[n] = m.episodes, st.successes[n] = m.successes;
}

__global__ void __launch_bounds__(SAC_TERMS_LANES) monitor_stats_kernel(const MonitorStatsCall P) {
  __shared__ double partial[SAC_TERMS_LANES];
  __shared__ int64_t episodes[SAC_TERMS_LANES];
  __shared__ int64_t lengths[SAC_TERMS_LANES];
  __shared__ int64_t successes[SAC_TERMS_LANES];
  const int t = threadIdx.x;
  const urgym_monitor_state& st = P.state;
  const double* const sum_return = st.sum_return;
  int64_t ep = 0, len = 0, ok = 0;
  for (int n = t; n < P.num_envs; n += SAC_TERMS_LANES) {
    ep += (int64_t)st.episodes[n];
    len += st.sum_length[n];
    ok += (int64_t)st.successes[n];
  }
  partial[t] = ordered_partial(t, P.num_envs, [sum_return](int n) { return sum_return[n]; });
  episodes[t] = ep, lengths[t] = len, successes[t] = ok;
  if (P.clear != 0)  // the entries this lane has just read, and no other lane reads
    for (int n = t; n < P.num_envs; n += SAC_TERMS_LANES) st.sum_return[n] = 0.0, st.sum_length[n] = 0, st.episodes[n] = 0, st.successes[n] = 0;
  __syncthreads();
  for (int s = SAC_TERMS_LANES / 2; s >= 1; s >>= 1) {
    if (t < s) {
      partial[t] += partial[t + s];
      episodes[t] += episodes[t + s];
      lengths[t] += lengths[t + s];
      successes[t] += successes[t + s];
    }
    __syncthreads();
  }
  if (t != 0) return;
  urgym_monitor_record rec;
  monitor_tail(partial[0], episodes[0], lengths[0], successes[0], P.iteration, rec);
  P.record[0] = rec;
}

}  // namespace

void monitor_fold_launch(const MonitorFoldCall& call, hipStream_t s) {
  hipLaunchKernelGGL(monitor_fold_kernel, dim3((call.num_envs + FOLD_LANES - 1) / FOLD_LANES), dim3(FOLD_LANES), 0, s, call);
}

void monitor_stats_launch(const MonitorStatsCall& call, hipStream_t s) {
  hipLaunchKernelGGL(monitor_stats_kernel, dim3(1), dim3(SAC_TERMS_LANES), 0, s, call);
}

}  // namespace urgym
