// urgym_handle.h — what the two host units of liburgym_hip.so share: the handle behind every void* of include/urgym.h, how a call
// fails, and the two functions that cross between urgym_hip.hip (step kernels, their launches, the environment's entry points) and
// urgym_policy_abi.hip (the learner's entry points).  No device code, and none of urgym_device.h or the robot model: a change to the
// learner's host side does not recompile the step kernels.  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/urgym.h"
#include "urgym_launch_plan.h"

namespace urgym {

struct CandRec;  // urgym_device.h
struct Actor;    // urgym_actor.h
struct Critic;   // urgym_critic.h

// The kernel instances a handle launches, chosen once by urgym_hip.hip.  The struct they take as their first parameter(s), KParams,
// is a type of that unit's anonymous namespace and part of every kernel's symbol name, so no declaration of it can be shared: the
// table holds the pointers untyped, and the unit that filled it casts them back where it launches (ModeKernel, FusedKernel there).
struct Kernels {
  void (*mode[4])();  // by MODE_*
  void (*fused)();    // env_step_fused (none for Ori)
};

struct Handle {
  urgym_config cfg;
  urgym_buffers buf;
  bool bound = false;
  int device = 0;
  int obs_dim = 0, goal_dim = 0;
  LaunchPlan plan;                 // launch geometry and paths (urgym_launch_plan.h), fixed at urgym_create
  Kernels k;
  double* d_ld_scratch = nullptr;  // [5][N] link distances of the running step
  double* d_sc_scratch = nullptr;  // [SC_ROWS][N] set-up cache of the running step
  double* d_lf_scratch = nullptr;  // [3][12][N] frames of links 4, 5, 6 of the running step (sized by this handle's N)
  CandRec* d_recs = nullptr;          // support map: candidate records ...
  unsigned short* d_cell = nullptr;   // ... and the cube map of directions that points into them
  uint64_t seed = 0;
  int pp = 0;
  char err[512] = {0};
  // timing
  bool timing = false;
  int timing_every = 1;   // time every k-th step (an event pair costs the stream ~6 us: sampling keeps the measurement out of the measured)
  long timing_tick = 0;
  std::vector<hipEvent_t> ev;  // pairs: [2i] start, [2i+1] stop ; kind in ev_kind
  std::vector<int> ev_kind;    // 0 = step kernel, 1 = reset kernel(s) on the caller's stream
  size_t ev_used = 0;
  // prefetched episode records (DESIGN.md "auto-reset off the critical path")
  float neutral_ach[6] = {0, 0, 0, 0, 0, 0};
  double* d_rec = nullptr;      // [2][REC_FIELDS][N]
  int32_t* d_reci = nullptr;    // [2][2][N]
  int2* d_rl[4] = {nullptr, nullptr, nullptr, nullptr};  // refill lists (capacities: plan.rl_cap)
  int* d_rcount = nullptr;      // their counters
  int parity = 0;
  uint64_t rec_seed = 0;
  bool rec_seed_valid = false;
  // Steps left in which a finished env may still meet a record that is not valid for its episode (after create / bind /
  // urgym_invalidate_records / a reset that did not cover every env): only then does a step carry the fallback launches.
  // An env that falls back gets fresh records for its next two episodes, and every env finishes within max_episode_steps.
  int dirty_steps = 0;
  long steps_since_full_reset = -1; // step launches since the last urgym_reset of every env (-1: none yet)
  // policies (urgym_policy_abi.hip)
  std::vector<Actor*> actors;  // alive, released by urgym_destroy at the latest
  std::vector<Critic*> critics;  // the same for the twin Q-networks (urgym_critic.hip)
  bool observed = false;       // a reset / refresh has filled the bound observation buffers: an actor has something to read
};

// the message of a failure that has no handle to keep it (urgym_last_error(NULL))
inline thread_local char g_err[512] = {0};

inline int fail(Handle* h, int code, const char* what, hipError_t e = hipSuccess) {
  char* dst = h ? h->err : g_err;
  if (e != hipSuccess)
    snprintf(dst, 512, "%s: %s", what, hipGetErrorString(e));
  else
    snprintf(dst, 512, "%s", what);
  return code;
}
// fail() with a formatted message of up to 199 characters
inline int failf(Handle* h, int code, const char* format, ...) {
  char msg[200];
  va_list args;
  va_start(args, format);
  vsnprintf(msg, sizeof(msg), format, args);
  va_end(args);
  return fail(h, code, msg);
}
// fail() with the message "<who>: <what>", who being the entry point
inline int fail_in(Handle* h, int code, const char* who, const char* what) { return failf(h, code, "%s: %s", who, what); }
#define HIP_TRY(h, call)                                              \
  do {                                                                \
    hipError_t _e = (call);                                           \
    if (_e != hipSuccess) return fail(h, URGYM_ERR_HIP, #call, _e);   \
  } while (0)

// the end of an entry point that has launched: what the launches left behind
inline int launched(Handle* h) {
  HIP_TRY(h, hipGetLastError());
  return URGYM_OK;
}

// the checks of a call that needs bound buffers, and its device made current
inline int enter_bound(Handle* h) {
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!h->bound) return fail(h, URGYM_ERR_STATE, "urgym_bind() has not been called");
  HIP_TRY(h, hipSetDevice(h->device));
  return URGYM_OK;
}

// urgym_hip.hip: one environment step on `s` (every launch of it, the timing events), for the rollouts of urgym_policy_abi.hip
int do_step(Handle* h, const float* actions, hipStream_t s);
// urgym_policy_abi.hip: destroys the actors and critics still alive, for the release() of urgym_hip.hip
void release_policies(Handle* h);

}  // namespace urgym
