// urgym_policy_abi.hip -- the learner's half of the C-ABI of include/urgym.h.  Host code only: no kernel lives in this unit, so a check
// added here leaves every kernel's object file alone.  Every check is made here, before the first launch; every launch goes through the
// kernel units' headers (urgym_actor.h ... urgym_norm.h) or through do_step of urgym_hip.hip (urgym_handle.h).  In file order:
//   - actors: create / forward / sample, the rollouts, urgym_rollout_collect; the replay ring and its gathers (urgym_replay.h,
//     urgym_nstep.h, urgym_her.h, urgym_demo.h)
//   - the twin critic, its action gradient and parameter gradients; the actor's parameter gradients
//   - the Adam steps (urgym_adam.h) and gradient-norm clipping (urgym_grad_clip.h)
//   - SAC's entropy step and loss terms (urgym_sac_terms.h)
//   - the weight reloads and their inverse, urgym_actor_unpack / urgym_critic_unpack (urgym_weights.h)
//   - prioritized replay (urgym_per.h)
//   - running normalization (urgym_norm.h), evaluation (urgym_eval.h, urgym_eval_schedule.h) and training-episode statistics
//     (urgym_monitor.h): the checking halves, then their entry points
//   - the training loop in one call: TrainOptions, TrainExtras, sac_train_body, and the nine urgym_sac_train* entry points
//     (urgym_sac_schedule.h has the index arithmetic).  With a planner the collection and the plan statistics
//     are urgym_mppi_abi.hip's, reached through urgym_mppi_train.h
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/urgym.h"
#include "urgym_handle.h"
#include "urgym_actor.h"
#include "urgym_critic.h"
#include "urgym_pack_map.h"
#include "urgym_weights.h"
#include "urgym_replay.h"
#include "urgym_demo.h"
#include "urgym_nstep.h"
#include "urgym_her.h"
#include "urgym_adam.h"
#include "urgym_sac_bc.h"
#include "urgym_sac_terms.h"
#include "urgym_sac_schedule.h"
#include "urgym_eval.h"
#include "urgym_eval_schedule.h"
#include "urgym_monitor.h"
#include "urgym_per.h"
#include "urgym_grad_clip.h"
#include "urgym_norm.h"
#include "urgym_mppi_train.h"

using namespace urgym;

// every failure path of urgym_create and urgym_destroy (release() of urgym_hip.hip)
void urgym::release_policies(Handle* h) {
  for (Actor* a : h->actors) actor_destroy(a);
  for (Critic* c : h->critics) critic_destroy(c);
}

namespace {

const char* const NOT_OBSERVED = "no observations yet: call urgym_reset (or urgym_refresh) first";

// p as a T* if it is an element of v -- an actor or a critic of THIS handle, still alive -- else null
template <class T>
T* member(const std::vector<T*>& v, const void* p) {
  return std::find(v.begin(), v.end(), p) != v.end() ? (T*)p : nullptr;
}

// urgym_actor_destroy / urgym_critic_destroy
template <class T>
int destroy_member(Handle* h, std::vector<T*>& v, void* p, void (*destroy)(T*), const char* refusal) {
  if (!p) return URGYM_OK;
  T* x = member(v, p);
  if (!x) return fail(h, URGYM_ERR_ARG, refusal);
  hipSetDevice(h->device);
  hipDeviceSynchronize();  // launches that read its weights may still be in flight
  destroy(x);
  v.erase(std::find(v.begin(), v.end(), x));
  return URGYM_OK;
}

// ---- policies: the checks and the per-pass arguments of the entry points that run an actor

int actor_features(const Handle* h) { return h->obs_dim + 2 * h->goal_dim; }

ActorEnv actor_env(const Handle* h) {
  const urgym_buffers& b = h->buf;
  return ActorEnv{h->cfg.num_envs, h->obs_dim, h->goal_dim, h->cfg.auto_reset, b.observation, b.achieved_goal, b.desired_goal,
                  b.reward, b.final_observation, b.terminated, b.truncated, b.is_success, b.collision};
}

// the records of pass k (ActorPass): rows k of what the actor sees, rows k - 1 of what the step before returned
ActorPass actor_pass(const Handle* h, Actor* a, const urgym_trajectory& t, int k, int num_steps) {
  const size_t n = (size_t)h->cfg.num_envs, od = (size_t)h->obs_dim, gd = (size_t)h->goal_dim;
  const size_t pre = (size_t)k * n, post = (size_t)(k > 0 ? k - 1 : 0) * n;
  auto at = [](auto* p, size_t off) { return p ? p + off : p; };
  ActorPass r;
  r.obs = at(t.observation, pre * od), r.ach = at(t.achieved_goal, pre * gd), r.des = at(t.desired_goal, pre * gd);
  r.reward = at(t.reward, post);
  r.terminated = at(t.terminated, post), r.truncated = at(t.truncated, post), r.is_success = at(t.is_success, post);
  r.collision = at(t.collision, post);
  r.final_obs = at(t.final_observation, post * od);
  r.ep_return = t.episode_return, r.ep_last = t.episode_last_step, r.ep_success = t.episode_success;
  const bool summary = t.episode_return || t.episode_last_step || t.episode_success || t.episode_done;
  r.ep_done = t.episode_done ? t.episode_done : (summary ? actor_done_scratch(a) : nullptr);
  r.k = k, r.num_steps = num_steps;
  return r;
}

// The checks of every entry point that runs an actor; *out = the actor.  One that reads the bound buffers (own_rows null) is refused
// with both feature counts, and before anything has been observed.  One that takes the caller's rows words the feature refusal itself
// (own_rows) and leaves the observations to resolve_rows.
int enter_actor(Handle* h, void* actor, const char* who, Actor** out, const char* own_rows = nullptr) {
  if (int rc = enter_bound(h)) return rc;
  Actor* a = member(h->actors, actor);
  if (!a) return fail_in(h, URGYM_ERR_ARG, who, "not an actor of this handle (actors belong to the handle they were created with)");
  if (actor_in_features(a) != actor_features(h)) {
    if (own_rows) return fail_in(h, URGYM_ERR_ARG, who, own_rows);
    return failf(h, URGYM_ERR_ARG, "%s: the actor takes %d features, this env kind offers %d", who, actor_in_features(a), actor_features(h));
  }
  if (!own_rows && !h->observed) return fail_in(h, URGYM_ERR_STATE, who, NOT_OBSERVED);
  *out = a;
  return URGYM_OK;
}

// the checks of every entry point that samples; wants_density: a log-probability or a sample record is asked for
int check_sampling(Handle* h, const Actor* a, const urgym_sampling* how, bool wants_density, const char* who) {
  const char* what = nullptr;
  if (!how) what = "null sampling description";
  else if (how->reserved0 != 0) what = "urgym_sampling.reserved0 must be 0";
  else if (how->mode != URGYM_SAMPLE_MEAN && how->mode != URGYM_SAMPLE_GAUSSIAN && how->mode != URGYM_SAMPLE_UNIFORM)
    what = "unknown sampling mode (URGYM_SAMPLE_MEAN, _GAUSSIAN or _UNIFORM)";
  else if (!actor_has_log_std(a) && (how->mode == URGYM_SAMPLE_GAUSSIAN || (how->mode == URGYM_SAMPLE_MEAN && wants_density)))
    what = "the actor has no log_std head (urgym_actor_set_log_std)";
  return what ? fail_in(h, URGYM_ERR_ARG, who, what) : URGYM_OK;
}

// The one launch of a policy pass.  MEAN with no density asked for (no log-probability, no sample record) is the deterministic kernel.
void policy_launch(Actor* a, const ActorEnv& env, float* actions, const ActorPass* pass, const ActorSample& smp, hipStream_t s) {
  if (smp.mode == URGYM_SAMPLE_MEAN && !smp.log_prob && !smp.noise && !smp.mean_action && !smp.log_std)
    actor_launch(a, env, actions, pass, s);
  else
    actor_launch_sampled(a, env, actions, pass, smp, s);
}

// ---- explicit rows (the critic's entry points, urgym_actor_sample_rows): the checks that concern rows and count; on success obs / ach /
// des are the pointers to read (the bound buffers where rows->observation is null)
int resolve_rows(Handle* h, const urgym_critic_rows* rows, int count, const char* who, const float** obs, const float** ach, const float** des) {
  const char* what = nullptr;
  if (!rows) what = "null rows";
  else if (count <= 0) what = "count must be positive";
  else if (!rows->observation && count != h->cfg.num_envs) what = "rows->observation is null (the bound buffers): count must be num_envs";
  else if (rows->observation && (!rows->achieved_goal || !rows->desired_goal)) what = "rows->achieved_goal or rows->desired_goal is null";
  if (what) return fail_in(h, URGYM_ERR_ARG, who, what);
  const bool bound = !rows->observation;
  if (bound && !h->observed) return fail_in(h, URGYM_ERR_STATE, who, NOT_OBSERVED);
  *obs = bound ? h->buf.observation : rows->observation;
  *ach = bound ? h->buf.achieved_goal : rows->achieved_goal;
  *des = bound ? h->buf.desired_goal : rows->desired_goal;
  return URGYM_OK;
}

// ---- the replay ring (urgym_rollout_collect, urgym_replay_sample): the checks that concern the ring itself
int check_ring(Handle* h, const urgym_replay_ring* r, const char* who) {
  const char* what = nullptr;
  if (!r) what = "null ring";
  else if (r->capacity_steps <= 0) what = "ring->capacity_steps must be positive";
  else if (r->reserved0 != 0) what = "urgym_replay_ring.reserved0 must be 0";
  else if (!r->observation || !r->achieved_goal || !r->desired_goal || !r->action || !r->reward || !r->next_observation ||
           !r->next_achieved_goal || !r->next_desired_goal || !r->terminated)
    what = "a required ring pointer is null (all but truncated and is_success)";
  return what ? fail_in(h, URGYM_ERR_ARG, who, what) : URGYM_OK;
}

// the store pass before step k of a collection that started at first_slot: the s of slot k (k < num_steps), the outcome of slot k - 1
ReplayStore replay_store(const Handle* h, const urgym_replay_ring& r, int first_slot, int k, int num_steps) {
  const urgym_buffers& b = h->buf;
  const size_t n = (size_t)h->cfg.num_envs, od = (size_t)h->obs_dim, gd = (size_t)h->goal_dim, C = (size_t)r.capacity_steps;
  ReplayStore p;
  memset(&p, 0, sizeof(p));
  p.N = h->cfg.num_envs, p.obs_dim = h->obs_dim, p.goal_dim = h->goal_dim, p.auto_reset = h->cfg.auto_reset;
  p.observation = b.observation, p.achieved_goal = b.achieved_goal, p.desired_goal = b.desired_goal, p.reward = b.reward;
  p.final_observation = b.final_observation, p.final_achieved_goal = b.final_achieved_goal, p.final_desired_goal = b.final_desired_goal;
  p.terminated = b.terminated, p.truncated = b.truncated, p.is_success = b.is_success;
  if (k < num_steps) {
    const size_t at = (((size_t)first_slot + (size_t)k) % C) * n;
    p.obs = r.observation + at * od, p.ach = r.achieved_goal + at * gd, p.des = r.desired_goal + at * gd;
  }
  if (k > 0) {
    const size_t at = (((size_t)first_slot + (size_t)k - 1) % C) * n;
    p.reward_out = r.reward + at, p.terminated_out = r.terminated + at;
    p.truncated_out = r.truncated ? r.truncated + at : nullptr, p.is_success_out = r.is_success ? r.is_success + at : nullptr;
    p.next_obs = r.next_observation + at * od, p.next_ach = r.next_achieved_goal + at * gd, p.next_des = r.next_desired_goal + at * gd;
  }
  return p;
}

// ---- the rollout loop of urgym_rollout_actor, urgym_rollout_sampled and urgym_rollout_collect

// What a rollout keeps besides stepping; every pointer may be null.  A ring excludes the two kinds of records.
struct RolloutSinks {
  const urgym_trajectory* traj;
  const urgym_sample_records* extra;
  const urgym_replay_ring* ring;  // its slots (first_slot + k) % capacity_steps
  int first_slot;
};

// num_steps policy passes, each followed by its step, and a closing pass for the outcome of the last step; the callers have checked
// everything.  how: null = the deterministic actor.
// Every launch below goes to `s`, and so does everything do_step launches (the step or fused launch, the RESET / PREFETCH fallbacks of
// a dirty step, the timing events): stream order alone puts step k - 1 before the passes that read its outputs (the store pass files
// its outcome, the actor's pass records it) and those before the step that reads their actions.
// `norm`: given (urgym_rollout_collect_normalized) = one more launch before every policy pass, which maps the bound rows into the
// scratch its destinations name, and the actor reads the scratch; the store pass and the step see the bound buffers as before.
int rollout(Handle* h, Actor* a, const urgym_sampling* how, int num_steps, const RolloutSinks& to, hipStream_t s, const NormApplyCall* norm = nullptr) {
  if (num_steps == 0) return URGYM_OK;
  ActorEnv env = actor_env(h);
  if (norm) env.observation = norm->seg[0].dst, env.achieved_goal = norm->seg[1].dst, env.desired_goal = norm->seg[2].dst;
  const size_t n = (size_t)h->cfg.num_envs, row = n * 6;
  auto at = [](float* p, size_t off) { return p ? p + off : p; };
  for (int k = 0; k <= num_steps; k++) {
    if (to.ring) replay_store_launch(replay_store(h, *to.ring, to.first_slot, k, num_steps), s);
    ActorPass pass;
    if (to.traj) pass = actor_pass(h, a, *to.traj, k, num_steps);
    if (k == num_steps) {
      if (to.traj) actor_launch(a, env, nullptr, &pass, s);  // the result of the last step; no forward pass
      break;
    }
    float* actions = actor_action_scratch(a);
    if (to.ring)  // the actor writes the slot, the step reads it
      actions = to.ring->action + (size_t)((to.first_slot + (int64_t)k) % to.ring->capacity_steps) * row;
    else if (to.traj && to.traj->action)
      actions = to.traj->action + (size_t)k * row;
    ActorSample smp{how ? how->mode : URGYM_SAMPLE_MEAN, how ? how->seed : 0, how ? how->first_draw + (uint64_t)k : 0, nullptr, nullptr, nullptr, nullptr};
    if (to.extra) {
      smp.log_prob = at(to.extra->log_prob, (size_t)k * n), smp.noise = at(to.extra->noise, (size_t)k * row);
      smp.mean_action = at(to.extra->mean_action, (size_t)k * row), smp.log_std = at(to.extra->log_std, (size_t)k * row);
    }
    if (norm) norm_apply_launch(*norm, s);
    policy_launch(a, env, actions, to.traj ? &pass : nullptr, smp, s);
    if (int rc = do_step(h, actions, s)) return rc;
  }
  return launched(h);
}

// ---- the twin critic

// The checks of every entry point that runs a critic: one of this handle's, taking this env kind's features and, where the kernels of
// the call are built for some widths only (supported), one of those; *out = the critic
int enter_critic(Handle* h, void* critic, const char* who, Critic** out, bool (*supported)(Critic*) = nullptr, const char* unsupported = nullptr) {
  Critic* c = member(h->critics, critic);
  if (!c) return fail_in(h, URGYM_ERR_ARG, who, "not a critic of this handle (critics belong to the handle they were created with)");
  if (critic_in_features(c) != actor_features(h) + 6) return fail_in(h, URGYM_ERR_ARG, who, "the critic does not take this env kind's features");
  if (supported && !supported(c)) return fail_in(h, URGYM_ERR_ARG, who, unsupported);
  *out = c;
  return URGYM_OK;
}

// the rows of a critic call (its first fields are CriticCall's in all three kinds): resolve_rows, then the action and the sizes
template <class Call>
int critic_rows(Handle* h, const urgym_critic_rows* rows, int count, const char* who, Call* call) {
  memset(call, 0, sizeof(*call));
  if (int rc = resolve_rows(h, rows, count, who, &call->observation, &call->achieved_goal, &call->desired_goal)) return rc;
  if (!rows->action) return fail_in(h, URGYM_ERR_ARG, who, "rows->action is null");
  call->M = count, call->obs_dim = h->obs_dim, call->goal_dim = h->goal_dim;
  call->action = rows->action;
  return URGYM_OK;
}

// the checks urgym_critic_parameter_gradients and its workspace query share: enter_critic with the widths the kernels are built for,
// and count within [1, URGYM_CRITIC_GRADIENTS_MAX_COUNT]
int backward_critic(Handle* h, void* critic, int count, const char* who, Critic** out) {
  static_assert(URGYM_CRITIC_GRADIENTS_MAX_COUNT == CRITIC_BACKWARD_MAX_COUNT, "include/urgym.h");
  if (int rc = enter_critic(h, critic, who, out, critic_backward_supported, "the gradient kernels are built for hidden widths up to 256")) return rc;
  if (count <= 0) return fail_in(h, URGYM_ERR_ARG, who, "count must be positive");
  if (count > CRITIC_BACKWARD_MAX_COUNT) return fail_in(h, URGYM_ERR_ARG, who, "count is above URGYM_CRITIC_GRADIENTS_MAX_COUNT (65536)");
  return URGYM_OK;
}

// the checks urgym_actor_parameter_gradients and its workspace query share: an actor of this handle that takes this env kind's features,
// has a log_std head and a width the kernels are built for, and count within [1, URGYM_ACTOR_GRADIENTS_MAX_COUNT]
int backward_actor(Handle* h, void* actor, int count, const char* who, Actor** out) {
  static_assert(URGYM_ACTOR_GRADIENTS_MAX_COUNT == ACTOR_BACKWARD_MAX_COUNT, "include/urgym.h");
  if (int rc = enter_actor(h, actor, who, out, "the actor does not take this env kind's features")) return rc;
  if (!actor_has_log_std(*out)) return fail_in(h, URGYM_ERR_ARG, who, "the actor has no log_std head (urgym_actor_set_log_std)");
  if (!actor_backward_supported(*out)) return fail_in(h, URGYM_ERR_ARG, who, "the gradient kernels are built for hidden widths up to 256");
  if (count <= 0) return fail_in(h, URGYM_ERR_ARG, who, "count must be positive");
  if (count > ACTOR_BACKWARD_MAX_COUNT) return fail_in(h, URGYM_ERR_ARG, who, "count is above URGYM_ACTOR_GRADIENTS_MAX_COUNT (65536)");
  return URGYM_OK;
}

// urgym_actor_read_packed / urgym_critic_read_packed
int read_packed(Handle* h, const char* who, const float* dev, size_t floats, float* host_out, uint64_t capacity, uint64_t* count) {
  if (!count) return fail_in(h, URGYM_ERR_ARG, who, "null count");
  *count = floats;
  if (!host_out) return URGYM_OK;
  if (capacity < floats)
    return failf(h, URGYM_ERR_ARG, "%s: capacity is %llu floats, the packed buffer has %llu", who, (unsigned long long)capacity, (unsigned long long)floats);
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipDeviceSynchronize());
  HIP_TRY(h, hipMemcpy(host_out, dev, floats * sizeof(float), hipMemcpyDeviceToHost));
  return URGYM_OK;
}

// ---- Adam (urgym_adam.h): what urgym_adam_coefficients and both step calls refuse about the hyperparameters; null = accepted
const char* adam_hyper_refusal(const urgym_adam_hyper* hp) {
  if (!hp) return "null hyperparameters";
  if (hp->reserved0 != 0) return "urgym_adam_hyper.reserved0 must be 0";
  if (!(hp->lr >= 0.0 && hp->lr < (double)INFINITY)) return "lr must be finite and not negative";  // refuses NaN too
  if (!(hp->beta1 >= 0.0 && hp->beta1 < 1.0) || !(hp->beta2 >= 0.0 && hp->beta2 < 1.0)) return "beta1 and beta2 must be in [0, 1)";
  if (!(hp->eps > 0.0 && hp->eps < (double)INFINITY)) return "eps must be finite and positive";
  if (hp->step < 1) return "step is the 1-based index of this step: it must be at least 1";
  return nullptr;
}

AdamCoef adam_coef(const urgym_adam_hyper& hp) { return adam_coefficients(hp.lr, hp.beta1, hp.beta2, hp.eps, hp.step); }

// ---- the checking half of every entry point urgym_sac_train composes.  Each makes ALL the checks of its entry point, in its order and
// with its refusal texts (`who` names the entry point), launches nothing, and leaves what the launching half needs: the launch struct of
// the kernel unit's seam header, filled.  The entry points below are check + launch; urgym_sac_train runs every check first.

// what urgym_actor_sample_rows launches
struct SampleRows {
  Actor* a;
  ActorEnv env;
  float* actions;
  ActorSample smp;
};
// what the two Adam steps launch, but for the coefficients
struct ActorAdamStep {
  Actor* a;
  ActorPacked buf;
  AdamTensors<PACK_ACTOR_TENSORS> T;
};
struct CriticAdamStep {
  CriticPacked buf, target_buf;
  bool has_target;
  float tau;
  AdamTensors<2 * PACK_CRITIC_TENSORS> T;
};

int check_actor_adam(Handle* h, void* actor, const urgym_actor_adam* t, const urgym_adam_hyper* hp, const char* who, ActorAdamStep* out) {
  Actor* a = member(h->actors, actor);
  if (!a) return fail_in(h, URGYM_ERR_ARG, who, "not an actor of this handle (actors belong to the handle they were created with)");
  if (!t) return fail_in(h, URGYM_ERR_ARG, who, "null tensors");
  if (t->reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_actor_adam.reserved0 must be 0");
  const ActorPacked buf = actor_packed(a);
  if (t->in_features != buf.in_features || t->hidden_width != buf.hidden)
    return failf(h, URGYM_ERR_ARG, "%s: tensors are %d -> %d, the actor is %d -> %d", who, t->in_features, t->hidden_width, buf.in_features, buf.hidden);
  AdamTensors<PACK_ACTOR_TENSORS>& T = out->T;
  {
    const urgym_actor_tensors &p = t->param, &m = t->exp_avg, &v = t->exp_avg_sq;
    const urgym_actor_tensors_const& g = t->grad;
    float* const ps[PACK_ACTOR_TENSORS] = {p.w0, p.b0, p.w1, p.b1, p.w_mu, p.b_mu, p.w_log_std, p.b_log_std};
    const float* const gs[PACK_ACTOR_TENSORS] = {g.w0, g.b0, g.w1, g.b1, g.w_mu, g.b_mu, g.w_log_std, g.b_log_std};
    float* const ms[PACK_ACTOR_TENSORS] = {m.w0, m.b0, m.w1, m.b1, m.w_mu, m.b_mu, m.w_log_std, m.b_log_std};
    float* const vs[PACK_ACTOR_TENSORS] = {v.w0, v.b0, v.w1, v.b1, v.w_mu, v.b_mu, v.w_log_std, v.b_log_std};
    for (int i = 0; i < PACK_ACTOR_TENSORS; i++) {
      if (!ps[i] || !gs[i] || !ms[i] || !vs[i]) return fail_in(h, URGYM_ERR_ARG, who, "a tensor pointer is null (all 32 are required)");
      T.param[i] = ps[i], T.grad[i] = gs[i], T.exp_avg[i] = ms[i], T.exp_avg_sq[i] = vs[i];
    }
  }
  if (const char* what = adam_hyper_refusal(hp)) return fail_in(h, URGYM_ERR_ARG, who, what);
  out->a = a, out->buf = buf;
  return URGYM_OK;
}

int check_critic_adam(Handle* h, void* online, void* target_or_NULL, const urgym_critic_adam* t, const urgym_adam_hyper* hp, float tau, const char* who,
                      CriticAdamStep* out) {
  Critic* c = member(h->critics, online);
  if (!c) return fail_in(h, URGYM_ERR_ARG, who, "not a critic of this handle (critics belong to the handle they were created with)");
  const CriticPacked buf = critic_packed(c);
  CriticPacked& target_buf = out->target_buf;
  if (target_or_NULL) {
    if (target_or_NULL == online) return fail_in(h, URGYM_ERR_ARG, who, "the target is the online critic itself");
    Critic* tc = member(h->critics, target_or_NULL);
    if (!tc) return fail_in(h, URGYM_ERR_ARG, who, "the target is not a critic of this handle");
    target_buf = critic_packed(tc);
    if (target_buf.in_features != buf.in_features || target_buf.hidden != buf.hidden || target_buf.floats != buf.floats)
      return failf(h, URGYM_ERR_ARG, "%s: the target is %d -> %d, the online critic is %d -> %d", who, target_buf.in_features, target_buf.hidden, buf.in_features, buf.hidden);
    if (!(tau > 0.0f && tau <= 1.0f)) return fail_in(h, URGYM_ERR_ARG, who, "tau must be in (0, 1]");  // refuses NaN too
  }
  if (!t) return fail_in(h, URGYM_ERR_ARG, who, "null tensors");
  if (t->reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_critic_adam.reserved0 must be 0");
  if (t->in_features != buf.in_features || t->hidden_width != buf.hidden)
    return failf(h, URGYM_ERR_ARG, "%s: tensors are %d -> %d, the critic is %d -> %d", who, t->in_features, t->hidden_width, buf.in_features, buf.hidden);
  AdamTensors<2 * PACK_CRITIC_TENSORS>& T = out->T;
  for (int net = 0; net < 2; net++) {
    const urgym_q_network_grad &p = t->param[net], &m = t->exp_avg[net], &v = t->exp_avg_sq[net];
    const urgym_q_network_dev& g = t->grad[net];
    float* const ps[PACK_CRITIC_TENSORS] = {p.w0, p.b0, p.w1, p.b1, p.w_q, p.b_q};
    const float* const gs[PACK_CRITIC_TENSORS] = {g.w0, g.b0, g.w1, g.b1, g.w_q, g.b_q};
    float* const ms[PACK_CRITIC_TENSORS] = {m.w0, m.b0, m.w1, m.b1, m.w_q, m.b_q};
    float* const vs[PACK_CRITIC_TENSORS] = {v.w0, v.b0, v.w1, v.b1, v.w_q, v.b_q};
    for (int i = 0; i < PACK_CRITIC_TENSORS; i++) {
      if (!ps[i] || !gs[i] || !ms[i] || !vs[i]) return fail_in(h, URGYM_ERR_ARG, who, "a tensor pointer is null (all 48 are required)");
      const int k = PACK_CRITIC_TENSORS * net + i;
      T.param[k] = ps[i], T.grad[k] = gs[i], T.exp_avg[k] = ms[i], T.exp_avg_sq[k] = vs[i];
    }
  }
  if (const char* what = adam_hyper_refusal(hp)) return fail_in(h, URGYM_ERR_ARG, who, what);
  out->buf = buf, out->has_target = target_or_NULL != nullptr, out->tau = tau;
  return URGYM_OK;
}

// ---- gradient-norm clipping (include/urgym.h, urgym_actor_grad_norm ... urgym_sac_train_clipped)

// what both norm calls refuse about their args
int check_grad_norm_args(Handle* h, const urgym_grad_norm* args, const char* who, GradNormCall* out) {
  if (!args) return fail_in(h, URGYM_ERR_ARG, who, "null args");
  if (args->reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_grad_norm.reserved0 must be 0");
  if (!(args->max_norm > 0.0f && args->max_norm < INFINITY)) return fail_in(h, URGYM_ERR_ARG, who, "max_norm must be finite and positive");  // refuses NaN too
  if (!args->norm_out || !args->scale_out) return fail_in(h, URGYM_ERR_ARG, who, "norm_out or scale_out is null");
  if ((uintptr_t)args->tensor_sums_out % 8 != 0) return fail_in(h, URGYM_ERR_ARG, who, "tensor_sums_out must be 8-byte aligned");
  out->max_norm = args->max_norm, out->norm_out = args->norm_out, out->scale_out = args->scale_out, out->tensor_sums_out = args->tensor_sums_out;
  return URGYM_OK;
}

int check_actor_grad_norm(Handle* h, void* actor, const urgym_actor_tensors_const* grad, const urgym_grad_norm* args, const char* who, GradNormCall* out) {
  static_assert(GRAD_NORM_ACTOR_TENSORS == 8 && GRAD_NORM_CRITIC_TENSORS == 12, "include/urgym.h");
  Actor* a = member(h->actors, actor);
  if (!a) return fail_in(h, URGYM_ERR_ARG, who, "not an actor of this handle (actors belong to the handle they were created with)");
  if (!grad) return fail_in(h, URGYM_ERR_ARG, who, "null grad");
  const ActorPacked buf = actor_packed(a);
  const int n = buf.in_features, H = buf.hidden;
  const float* const gs[GRAD_NORM_ACTOR_TENSORS] = {grad->w0, grad->b0, grad->w1, grad->b1, grad->w_mu, grad->b_mu, grad->w_log_std, grad->b_log_std};
  const int counts[GRAD_NORM_ACTOR_TENSORS] = {H * n, H, H * H, H, 6 * H, 6, 6 * H, 6};
  memset(out, 0, sizeof(*out));
  out->tensors = GRAD_NORM_ACTOR_TENSORS;
  for (int i = 0; i < GRAD_NORM_ACTOR_TENSORS; i++) {
    if (!gs[i]) return fail_in(h, URGYM_ERR_ARG, who, "a tensor pointer is null (all 8 are required)");
    out->grad[i] = gs[i], out->count[i] = counts[i];
  }
  return check_grad_norm_args(h, args, who, out);
}

int check_critic_grad_norm(Handle* h, void* critic, const urgym_q_network_dev* grad, const urgym_grad_norm* args, const char* who, GradNormCall* out) {
  Critic* c = member(h->critics, critic);
  if (!c) return fail_in(h, URGYM_ERR_ARG, who, "not a critic of this handle (critics belong to the handle they were created with)");
  if (!grad) return fail_in(h, URGYM_ERR_ARG, who, "null grad");
  const CriticPacked buf = critic_packed(c);
  const int n = buf.in_features, H = buf.hidden;
  const int counts[PACK_CRITIC_TENSORS] = {H * n, H, H * H, H, H, 1};
  memset(out, 0, sizeof(*out));
  out->tensors = GRAD_NORM_CRITIC_TENSORS;
  for (int net = 0; net < 2; net++) {
    const urgym_q_network_dev& g = grad[net];
    const float* const gs[PACK_CRITIC_TENSORS] = {g.w0, g.b0, g.w1, g.b1, g.w_q, g.b_q};
    for (int i = 0; i < PACK_CRITIC_TENSORS; i++) {
      if (!gs[i]) return fail_in(h, URGYM_ERR_ARG, who, "a tensor pointer is null (all 12 are required)");
      out->grad[PACK_CRITIC_TENSORS * net + i] = gs[i], out->count[PACK_CRITIC_TENSORS * net + i] = counts[i];
    }
  }
  return check_grad_norm_args(h, args, who, out);
}

int check_entropy_step(Handle* h, const urgym_sac_entropy_args* args, const urgym_adam_hyper* hp, const char* who, SacEntropyCall* out) {
  static_assert(URGYM_SAC_TERMS_MAX_COUNT == SAC_TERMS_MAX_COUNT, "include/urgym.h");
  if (!args) return fail_in(h, URGYM_ERR_ARG, who, "null args");
  const urgym_sac_entropy_args& a = *args;
  if (a.reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_entropy_args.reserved0 must be 0");
  if (a.count < 1 || a.count > SAC_TERMS_MAX_COUNT) return fail_in(h, URGYM_ERR_ARG, who, "count must be in [1, URGYM_SAC_TERMS_MAX_COUNT] (65536)");
  if (!a.log_prob || !a.log_ent_coef || !a.exp_avg || !a.exp_avg_sq || !a.ent_coef_out)
    return fail_in(h, URGYM_ERR_ARG, who, "a required pointer is null (log_prob, log_ent_coef, exp_avg, exp_avg_sq, ent_coef_out)");
  if (!(fabsf(a.target_entropy) < INFINITY)) return fail_in(h, URGYM_ERR_ARG, who, "target_entropy must be finite");  // refuses NaN too
  if (!(fabsf(a.gamma) < INFINITY)) return fail_in(h, URGYM_ERR_ARG, who, "gamma must be finite");
  if (!(fabsf(a.scale) < INFINITY)) return fail_in(h, URGYM_ERR_ARG, who, "scale must be finite");
  const int given = (a.target_in != nullptr) + (a.next_log_prob != nullptr) + (a.y_out != nullptr);
  if ((given != 0 && given != 3) || (given == 0 && a.terminated))
    return fail_in(h, URGYM_ERR_ARG, who, "the target group is half given: target_in, next_log_prob and y_out go together (terminated only with them)");
  if (const char* what = adam_hyper_refusal(hp)) return fail_in(h, URGYM_ERR_ARG, who, what);
  SacEntropyCall& c = *out;
  c.count = a.count, c.target_entropy = a.target_entropy, c.gamma = a.gamma, c.scale = a.scale;
  c.log_prob = a.log_prob, c.log_ent_coef = a.log_ent_coef, c.exp_avg = a.exp_avg, c.exp_avg_sq = a.exp_avg_sq;
  c.ent_coef_out = a.ent_coef_out, c.loss_out = a.loss_out;
  c.target_in = a.target_in, c.next_log_prob = a.next_log_prob, c.terminated = a.terminated, c.y_out = a.y_out;
  c.d_log_prob_out = a.d_log_prob_out;
  c.c = adam_coef(*hp);
  return URGYM_OK;
}

int check_policy_terms(Handle* h, const urgym_sac_policy_args* args, const char* who, SacPolicyCall* out) {
  if (!args) return fail_in(h, URGYM_ERR_ARG, who, "null args");
  const urgym_sac_policy_args& a = *args;
  if (a.reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_policy_args.reserved0 must be 0");
  if (a.count < 1 || a.count > SAC_TERMS_MAX_COUNT) return fail_in(h, URGYM_ERR_ARG, who, "count must be in [1, URGYM_SAC_TERMS_MAX_COUNT] (65536)");
  if (!a.ent_coef) return fail_in(h, URGYM_ERR_ARG, who, "null ent_coef");
  if (!(fabsf(a.scale) < INFINITY)) return fail_in(h, URGYM_ERR_ARG, who, "scale must be finite");  // refuses NaN too
  const int upstream = (a.dqmin_da != nullptr) + (a.d_action_out != nullptr);
  const int critic = (a.q != nullptr) + (a.y != nullptr) + (a.critic_loss_out != nullptr);
  const int actor = (a.log_prob != nullptr) + (a.q_min != nullptr) + (a.actor_loss_out != nullptr);
  if (upstream == 1) return fail_in(h, URGYM_ERR_ARG, who, "the upstream group is half given: dqmin_da and d_action_out go together");
  if (critic != 0 && critic != 3) return fail_in(h, URGYM_ERR_ARG, who, "the critic-loss group is half given: q, y and critic_loss_out go together");
  if (actor != 0 && actor != 3) return fail_in(h, URGYM_ERR_ARG, who, "the actor-loss group is half given: log_prob, q_min and actor_loss_out go together");
  if (!upstream && !critic && !actor) return fail_in(h, URGYM_ERR_ARG, who, "no group is given (upstream, critic loss, actor loss)");
  SacPolicyCall& c = *out;
  c.count = a.count, c.scale = a.scale, c.ent_coef = a.ent_coef;
  c.dqmin_da = a.dqmin_da, c.d_action_out = a.d_action_out;
  c.q = a.q, c.y = a.y, c.critic_loss_out = a.critic_loss_out;
  c.log_prob = a.log_prob, c.q_min = a.q_min, c.actor_loss_out = a.actor_loss_out;
  return URGYM_OK;
}

// what urgym_sac_policy_terms_cloned and urgym_sac_train_cloned refuse about the option's numbers, or null
const char* clone_option_refusal(float weight, int32_t scale_by_q, int32_t q_filter, int32_t reserved0) {
  if (reserved0 != 0) return "reserved0 of the cloning struct must be 0";
  if (!(weight >= 0.0f && weight < INFINITY)) return "the cloning weight must be finite and >= 0";  // refuses NaN too
  if ((scale_by_q != 0 && scale_by_q != 1) || (q_filter != 0 && q_filter != 1)) return "scale_by_q and q_filter must be 0 or 1";
  return nullptr;
}

// urgym_sac_policy_terms_cloned: `call` is check_policy_terms' result for the same args
int check_policy_terms_cloned(Handle* h, const SacPolicyCall& call, const urgym_sac_clone_args* clone, const char* who, SacCloneCall* out) {
  if (!call.d_action_out || !call.critic_loss_out || !call.actor_loss_out)
    return fail_in(h, URGYM_ERR_ARG, who, "the cloned call needs all three groups (upstream, critic loss, actor loss)");
  if (!clone) return fail_in(h, URGYM_ERR_ARG, who, "null clone args");
  const urgym_sac_clone_args& b = *clone;
  if (!b.action_pi || !b.action_data || !b.bc_loss_out || !b.bc_weight_out || !b.bc_rows_out)
    return fail_in(h, URGYM_ERR_ARG, who, "a pointer of urgym_sac_clone_args is null (action_pi, action_data, bc_loss_out, bc_weight_out, bc_rows_out)");
  if (const char* what = clone_option_refusal(b.weight, b.scale_by_q, b.q_filter, b.reserved0)) return fail_in(h, URGYM_ERR_ARG, who, what);
  if (!(fabsf(b.bc_scale) < INFINITY)) return fail_in(h, URGYM_ERR_ARG, who, "bc_scale must be finite");
  if (call.d_action_out == b.action_pi || call.d_action_out == b.action_data)
    return fail_in(h, URGYM_ERR_ARG, who, "d_action_out is action_pi or action_data (the actions are read again after d_action_out is written)");
  *out = SacCloneCall{b.action_pi, b.action_data, b.weight, b.bc_scale, b.scale_by_q, b.q_filter, b.bc_loss_out, b.bc_weight_out, b.bc_rows_out};
  return URGYM_OK;
}

// what urgym_sac_policy_terms_weighted and urgym_sac_train_weighted refuse about the option's numbers, or null
const char* weight_option_refusal(float temperature, float max_weight, int32_t reserved0, int32_t q_filter) {
  if (reserved0 != 0) return "reserved0 of the advantage-weight struct must be 0";
  if (q_filter != 0) return "q_filter must be 0 with the advantage weight (the two gates are alternatives)";
  if (!(temperature > 0.0f && temperature < INFINITY)) return "the advantage temperature must be finite and > 0";  // refuses NaN too
  if (!(max_weight > 0.0f)) return "max_weight must be > 0 (finite or +infinity)";                               // refuses NaN too
  return nullptr;
}

// urgym_sac_policy_terms_weighted: after check_policy_terms and check_policy_terms_cloned of the same call
int check_policy_terms_weighted(Handle* h, const SacCloneCall& clone, const urgym_sac_advantage_args* advantage, const char* who, SacAdvantageCall* out) {
  if (!advantage) return fail_in(h, URGYM_ERR_ARG, who, "null advantage args");
  const urgym_sac_advantage_args& a = *advantage;
  if (!a.adv_ess_out || !a.adv_max_out || !a.adv_clipped_out)
    return fail_in(h, URGYM_ERR_ARG, who, "an output pointer of urgym_sac_advantage_args is null (adv_ess_out, adv_max_out, adv_clipped_out)");
  if (const char* what = weight_option_refusal(a.temperature, a.max_weight, a.reserved0, clone.q_filter)) return fail_in(h, URGYM_ERR_ARG, who, what);
  *out = SacAdvantageCall{a.temperature, a.max_weight, a.row_mask, a.adv_ess_out, a.adv_max_out, a.adv_clipped_out};
  return URGYM_OK;
}

int check_sample_rows(Handle* h, void* actor, const urgym_sampling* how, const urgym_critic_rows* rows, int count, float* actions_dev, float* log_prob_dev,
                      const char* who, SampleRows* out) {
  Actor* a = nullptr;
  if (int rc = enter_actor(h, actor, who, &a, "the actor does not take this env kind's features")) return rc;
  if (int rc = check_sampling(h, a, how, log_prob_dev != nullptr, who)) return rc;
  if (!actions_dev) return fail_in(h, URGYM_ERR_ARG, who, "null actions");
  ActorEnv& env = out->env;
  memset(&env, 0, sizeof(env));  // no records ride in this launch: the step outputs are not read
  if (int rc = resolve_rows(h, rows, count, who, &env.observation, &env.achieved_goal, &env.desired_goal)) return rc;
  env.N = count, env.obs_dim = h->obs_dim, env.goal_dim = h->goal_dim;
  out->a = a, out->actions = actions_dev;
  out->smp = ActorSample{how->mode, how->seed, how->first_draw, log_prob_dev, nullptr, nullptr, nullptr};
  return URGYM_OK;
}

int check_collect(Handle* h, void* actor, const urgym_sampling* how, int num_steps, const urgym_replay_ring* ring, int first_slot, const char* who, Actor** out) {
  Actor* a = nullptr;
  if (int rc = enter_actor(h, actor, who, &a)) return rc;
  if (int rc = check_sampling(h, a, how, false, who)) return rc;
  if (int rc = check_ring(h, ring, who)) return rc;
  if (first_slot < 0 || first_slot >= ring->capacity_steps) return fail_in(h, URGYM_ERR_ARG, who, "first_slot outside [0, capacity_steps)");
  if (num_steps <= 0) return fail_in(h, URGYM_ERR_ARG, who, "num_steps must be positive");
  *out = a;
  return URGYM_OK;
}

int check_replay_sample(Handle* h, const urgym_replay_ring* ring, int oldest_slot, int filled_steps, uint64_t seed, uint64_t draw, int count,
                        const urgym_replay_batch* batch, const char* who, ReplayGather* out) {
  if (int rc = check_ring(h, ring, who)) return rc;
  if (filled_steps < 1 || filled_steps > ring->capacity_steps) return fail_in(h, URGYM_ERR_ARG, who, "filled_steps outside [1, capacity_steps]");
  if (oldest_slot < 0 || oldest_slot >= ring->capacity_steps) return fail_in(h, URGYM_ERR_ARG, who, "oldest_slot outside [0, capacity_steps)");
  if (count <= 0) return fail_in(h, URGYM_ERR_ARG, who, "count must be positive");
  if (!batch) return fail_in(h, URGYM_ERR_ARG, who, "null batch");
  const urgym_replay_batch& b = *batch;
  if (!b.observation && !b.achieved_goal && !b.desired_goal && !b.action && !b.reward && !b.next_observation && !b.next_achieved_goal &&
      !b.next_desired_goal && !b.terminated && !b.truncated && !b.is_success && !b.index)
    return fail_in(h, URGYM_ERR_ARG, who, "no output requested (every batch pointer is null)");
  if ((b.truncated && !ring->truncated) || (b.is_success && !ring->is_success))
    return fail_in(h, URGYM_ERR_ARG, who, "truncated / is_success asked from a ring that does not keep it");
  ReplayGather& g = *out;
  g.N = h->cfg.num_envs, g.obs_dim = h->obs_dim, g.goal_dim = h->goal_dim, g.capacity = ring->capacity_steps;
  g.oldest_slot = oldest_slot, g.count = count;
  g.size = (uint64_t)filled_steps * (uint64_t)h->cfg.num_envs;
  g.seed = seed, g.draw = draw;
  g.ring = *ring, g.batch = b;
  return URGYM_OK;
}

// urgym_replay_sample_mixed: check_replay_sample's refusals first, then the demonstrations'
int check_replay_sample_mixed(Handle* h, const urgym_replay_ring* ring, int oldest_slot, int filled_steps, uint64_t seed, uint64_t draw, int count,
                              const urgym_replay_batch* batch, const urgym_replay_demonstrations* demo, uint8_t* source_out, const char* who, ReplayGatherMixed* out) {
  static_assert(URGYM_DEMO_TAG == DEMO_TAG, "include/urgym.h");
  if (int rc = check_replay_sample(h, ring, oldest_slot, filled_steps, seed, draw, count, batch, who, &out->g)) return rc;
  if (!demo) return fail_in(h, URGYM_ERR_ARG, who, "null demonstrations");
  const urgym_replay_demonstrations& d = *demo;
  const urgym_replay_ring& r = d.ring;
  if (r.capacity_steps <= 0) return fail_in(h, URGYM_ERR_ARG, who, "demonstrations: ring.capacity_steps must be positive");
  if (r.reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "demonstrations: urgym_replay_ring.reserved0 must be 0");
  if (!r.observation || !r.achieved_goal || !r.desired_goal || !r.action || !r.reward || !r.next_observation || !r.next_achieved_goal ||
      !r.next_desired_goal || !r.terminated)
    return fail_in(h, URGYM_ERR_ARG, who, "demonstrations: a required ring pointer is null (all but truncated and is_success)");
  if (d.num_envs < 1) return fail_in(h, URGYM_ERR_ARG, who, "demonstrations: num_envs must be at least 1");
  if (d.oldest_slot < 0 || d.oldest_slot >= r.capacity_steps) return fail_in(h, URGYM_ERR_ARG, who, "demonstrations: oldest_slot outside [0, capacity_steps)");
  if (d.filled_steps < 1 || d.filled_steps > r.capacity_steps) return fail_in(h, URGYM_ERR_ARG, who, "demonstrations: filled_steps outside [1, capacity_steps]");
  if (d.count < 0 || d.count > count) return fail_in(h, URGYM_ERR_ARG, who, "demonstrations: count outside [0, count]");
  // two positive int32: the product is below 2^62, stated as a check so that the entry arithmetic never depends on the types
  const uint64_t size_d = (uint64_t)d.filled_steps * (uint64_t)d.num_envs;
  if (size_d >= (uint64_t)1 << 63) return fail_in(h, URGYM_ERR_ARG, who, "demonstrations: filled_steps * num_envs must be below 2^63");
  if ((batch->truncated && !r.truncated) || (batch->is_success && !r.is_success))
    return fail_in(h, URGYM_ERR_ARG, who, "truncated / is_success asked while the demonstration ring does not keep it");
  out->demo = r;
  out->demo_side = DemoSide{size_d, d.num_envs, r.capacity_steps, d.oldest_slot};
  out->demo_count = d.count, out->source_out = source_out;
  return URGYM_OK;
}

// urgym_replay_sample_nstep: check_replay_sample's refusals first, then the window's
int check_replay_sample_nstep(Handle* h, const urgym_replay_ring* ring, int oldest_slot, int filled_steps, uint64_t seed, uint64_t draw, int count,
                              const urgym_replay_batch* batch, const urgym_replay_nstep* nstep, const char* who, ReplayGatherNstep* out) {
  static_assert(URGYM_REPLAY_NSTEP_MAX == NSTEP_MAX, "include/urgym.h");
  if (int rc = check_replay_sample(h, ring, oldest_slot, filled_steps, seed, draw, count, batch, who, &out->g)) return rc;
  if (!nstep) return fail_in(h, URGYM_ERR_ARG, who, "null nstep");
  const urgym_replay_nstep& n = *nstep;
  if (n.n_steps < 1 || n.n_steps > NSTEP_MAX) return fail_in(h, URGYM_ERR_ARG, who, "n_steps must be in [1, URGYM_REPLAY_NSTEP_MAX] (32)");
  if (n.reserved0 != 0 || n.reserved1 != 0.0f) return fail_in(h, URGYM_ERR_ARG, who, "urgym_replay_nstep.reserved0 and reserved1 must be 0");
  if (!(fabsf(n.gamma) < INFINITY)) return fail_in(h, URGYM_ERR_ARG, who, "gamma must be finite");  // refuses NaN too
  if (!n.discount) return fail_in(h, URGYM_ERR_ARG, who, "null discount");
  if (n.n_steps > 1 && !ring->truncated)
    return fail_in(h, URGYM_ERR_ARG, who, "n_steps > 1 on a ring that keeps no truncated (an episode's end at the time limit could not be seen)");
  out->n_steps = n.n_steps, out->filled_steps = filled_steps, out->gamma = n.gamma;
  out->discount = n.discount, out->steps = n.steps, out->last_index = n.last_index;
  return URGYM_OK;
}

// urgym_replay_sample_hindsight: check_replay_sample's refusals first, then the rule's
int check_replay_sample_hindsight(Handle* h, const urgym_replay_ring* ring, int oldest_slot, int filled_steps, uint64_t seed, uint64_t draw, int count,
                                  const urgym_replay_batch* batch, const urgym_replay_hindsight* hindsight, const char* who, ReplayGatherHindsight* out) {
  static_assert(URGYM_HER_HORIZON_MAX == HER_HORIZON_MAX && URGYM_HER_GOAL_FUTURE == HER_GOAL_FUTURE && URGYM_HER_GOAL_FINAL == HER_GOAL_FINAL &&
                    URGYM_HER_GOAL_OWN == HER_GOAL_OWN,
                "include/urgym.h");
  if (int rc = check_replay_sample(h, ring, oldest_slot, filled_steps, seed, draw, count, batch, who, &out->g)) return rc;
  if (!hindsight) return fail_in(h, URGYM_ERR_ARG, who, "null hindsight");
  const urgym_replay_hindsight& q = *hindsight;
  if (q.relabel_threshold > (uint64_t)1 << 32) return fail_in(h, URGYM_ERR_ARG, who, "relabel_threshold must be in [0, 2^32]");
  if (q.strategy < HER_GOAL_FUTURE || q.strategy > HER_GOAL_OWN) return fail_in(h, URGYM_ERR_ARG, who, "strategy must be URGYM_HER_GOAL_FUTURE, _FINAL or _OWN");
  if (q.horizon < 1 || q.horizon > HER_HORIZON_MAX) return fail_in(h, URGYM_ERR_ARG, who, "horizon must be in [1, URGYM_HER_HORIZON_MAX] (256)");
  if (q.reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_replay_hindsight.reserved0 must be 0");
  if (!ring->truncated || !ring->is_success)
    return fail_in(h, URGYM_ERR_ARG, who, "the ring keeps no truncated or no is_success (an episode's end and a collision could not be seen)");
  if (h->obs_dim < HER_GOAL_OFFSET + h->goal_dim || (h->goal_dim != 3 && h->goal_dim != 6))
    return fail_in(h, URGYM_ERR_ARG, who, "the observation row holds no goal at floats [12, 12 + goal_dim)");
  const urgym_config& c = h->cfg;
  out->filled_steps = filled_steps, out->strategy = q.strategy, out->horizon = q.horizon, out->relabel_threshold = q.relabel_threshold;
  out->distance_threshold = c.distance_threshold, out->ori_threshold = c.ori_threshold, out->w_collision = c.w_collision;
  out->w_success = c.w_success, out->w_distance = c.w_distance, out->w_orientation = c.w_orientation;
  out->additive = c.env_kind == URGYM_ENV_ORI || c.env_kind == URGYM_ENV_OBS;
  out->goal_index = q.goal_index, out->pose_terms = q.pose_terms;
  return URGYM_OK;
}

// urgym_sac_entropy_step_nstep: check_entropy_step's refusals on the other target group
int check_entropy_step_nstep(Handle* h, const urgym_sac_entropy_nstep_args* args, const urgym_adam_hyper* hp, const char* who, SacEntropyNstepCall* out) {
  if (!args) return fail_in(h, URGYM_ERR_ARG, who, "null args");
  const urgym_sac_entropy_nstep_args& a = *args;
  if (a.reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_entropy_nstep_args.reserved0 must be 0");
  if (a.count < 1 || a.count > SAC_TERMS_MAX_COUNT) return fail_in(h, URGYM_ERR_ARG, who, "count must be in [1, URGYM_SAC_TERMS_MAX_COUNT] (65536)");
  if (!a.log_prob || !a.log_ent_coef || !a.exp_avg || !a.exp_avg_sq || !a.ent_coef_out)
    return fail_in(h, URGYM_ERR_ARG, who, "a required pointer is null (log_prob, log_ent_coef, exp_avg, exp_avg_sq, ent_coef_out)");
  if (!(fabsf(a.target_entropy) < INFINITY)) return fail_in(h, URGYM_ERR_ARG, who, "target_entropy must be finite");  // refuses NaN too
  if (!(fabsf(a.scale) < INFINITY)) return fail_in(h, URGYM_ERR_ARG, who, "scale must be finite");
  const int given = (a.reward != nullptr) + (a.q_min_next != nullptr) + (a.discount != nullptr) + (a.next_log_prob != nullptr) + (a.y_out != nullptr);
  if ((given != 0 && given != 5) || (given == 0 && a.terminated))
    return fail_in(h, URGYM_ERR_ARG, who,
                   "the target group is half given: reward, q_min_next, discount, next_log_prob and y_out go together (terminated only with them)");
  if (const char* what = adam_hyper_refusal(hp)) return fail_in(h, URGYM_ERR_ARG, who, what);
  SacEntropyNstepCall& c = *out;
  c.count = a.count, c.target_entropy = a.target_entropy, c.scale = a.scale;
  c.log_prob = a.log_prob, c.log_ent_coef = a.log_ent_coef, c.exp_avg = a.exp_avg, c.exp_avg_sq = a.exp_avg_sq;
  c.ent_coef_out = a.ent_coef_out, c.loss_out = a.loss_out;
  c.reward = a.reward, c.q_min_next = a.q_min_next, c.discount = a.discount, c.next_log_prob = a.next_log_prob;
  c.terminated = a.terminated, c.y_out = a.y_out, c.d_log_prob_out = a.d_log_prob_out;
  c.c = adam_coef(*hp);
  return URGYM_OK;
}

int check_critic_evaluate(Handle* h, void* critic, const urgym_critic_rows* rows, int count, const urgym_critic_terms* terms, const urgym_critic_out* out,
                          const char* who, Critic** critic_out, CriticCall* call_out) {
  if (int rc = enter_bound(h)) return rc;
  Critic* c = nullptr;
  if (int rc = enter_critic(h, critic, who, &c)) return rc;
  CriticCall& call = *call_out;
  if (int rc = critic_rows(h, rows, count, who, &call)) return rc;
  if (!out) return fail_in(h, URGYM_ERR_ARG, who, "null out");
  if (!out->q && !out->q_min && !out->target) return fail_in(h, URGYM_ERR_ARG, who, "no output requested (q, q_min and target are all null)");
  if (out->target && (!terms || !terms->reward)) return fail_in(h, URGYM_ERR_ARG, who, "target requested without terms->reward");
  if (terms && out->target) {
    call.reward = terms->reward, call.terminated = terms->terminated, call.log_prob = terms->log_prob;
    call.gamma = terms->gamma, call.ent_coef = terms->ent_coef;
  }
  call.q = out->q, call.q_min = out->q_min, call.target = out->target;
  *critic_out = c;
  return URGYM_OK;
}

int check_critic_action_gradient(Handle* h, void* critic, const urgym_critic_rows* rows, int count, const urgym_critic_grad_out* out, const char* who,
                                 Critic** critic_out, CriticGradCall* call_out) {
  if (int rc = enter_bound(h)) return rc;
  Critic* c = nullptr;
  if (int rc = enter_critic(h, critic, who, &c, critic_grad_supported, "the gradient kernel is built for hidden widths up to 256")) return rc;
  CriticGradCall& call = *call_out;
  if (int rc = critic_rows(h, rows, count, who, &call)) return rc;
  if (!out) return fail_in(h, URGYM_ERR_ARG, who, "null out");
  if (!out->dq_da && !out->dqmin_da) return fail_in(h, URGYM_ERR_ARG, who, "no gradient requested (dq_da and dqmin_da are both null)");
  call.dq_da = out->dq_da, call.dqmin_da = out->dqmin_da, call.q = out->q, call.q_min = out->q_min;
  *critic_out = c;
  return URGYM_OK;
}

int check_critic_parameter_gradients(Handle* h, void* critic, const urgym_critic_rows* rows, int count, const float* dq, const float* target, float scale,
                                     const urgym_critic_param_grads* out, void* workspace, uint64_t workspace_bytes, const char* who, Critic** critic_out,
                                     CriticBackwardCall* call_out) {
  if (int rc = enter_bound(h)) return rc;
  Critic* c = nullptr;
  CriticBackwardCall& call = *call_out;
  if (int rc = backward_critic(h, critic, count, who, &c)) return rc;
  if (int rc = critic_rows(h, rows, count, who, &call)) return rc;
  if ((dq != nullptr) == (target != nullptr)) return fail_in(h, URGYM_ERR_ARG, who, "exactly one of dq and target must be given");
  if (target && !(fabsf(scale) < INFINITY)) return fail_in(h, URGYM_ERR_ARG, who, "scale must be finite");
  if (!out) return fail_in(h, URGYM_ERR_ARG, who, "null out");
  for (int net = 0; net < 2; net++) {
    const urgym_q_network_grad& g = out->qf[net];
    float* one[6] = {g.w0, g.b0, g.w1, g.b1, g.w_q, g.b_q};
    for (int i = 0; i < 6; i++) {
      if (!one[i]) return fail_in(h, URGYM_ERR_ARG, who, "a gradient pointer is null (all twelve are required)");
      call.grad[net][i] = one[i];
    }
  }
  if (!workspace) return fail_in(h, URGYM_ERR_ARG, who, "null workspace");
  if ((uintptr_t)workspace % 16 != 0) return fail_in(h, URGYM_ERR_ARG, who, "the workspace must be 16-byte aligned");
  if (workspace_bytes < critic_backward_workspace_bytes(c, count))
    return fail_in(h, URGYM_ERR_ARG, who, "the workspace is smaller than urgym_critic_parameter_gradients_workspace reports");
  call.dq = dq, call.target = target, call.scale = target ? scale : 0.0f;
  call.q = out->q, call.workspace = (float*)workspace;
  *critic_out = c;
  return URGYM_OK;
}

int check_actor_parameter_gradients(Handle* h, void* actor, const urgym_sampling* how, const urgym_critic_rows* rows, int count, const urgym_actor_upstream* upstream,
                                    const urgym_actor_param_grads* out, void* workspace, uint64_t workspace_bytes, const char* who, Actor** actor_out,
                                    ActorBackwardCall* call_out) {
  Actor* a = nullptr;
  if (int rc = backward_actor(h, actor, count, who, &a)) return rc;
  if (int rc = check_sampling(h, a, how, true, who)) return rc;
  if (how->mode == URGYM_SAMPLE_UNIFORM) return fail_in(h, URGYM_ERR_ARG, who, "mode must be URGYM_SAMPLE_GAUSSIAN or URGYM_SAMPLE_MEAN (UNIFORM runs no network)");
  ActorBackwardCall& call = *call_out;
  memset(&call, 0, sizeof(call));
  if (int rc = resolve_rows(h, rows, count, who, &call.observation, &call.achieved_goal, &call.desired_goal)) return rc;
  if (!upstream) return fail_in(h, URGYM_ERR_ARG, who, "null upstream");
  const bool sample = upstream->d_action || upstream->d_log_prob, heads = upstream->d_mu || upstream->d_log_std;
  if (sample == heads) return fail_in(h, URGYM_ERR_ARG, who, "exactly one upstream form must be given: d_action (with d_log_prob or NULL), or d_mu and d_log_std");
  if (sample && !upstream->d_action) return fail_in(h, URGYM_ERR_ARG, who, "d_log_prob is given without d_action");
  if (heads && (!upstream->d_mu || !upstream->d_log_std)) return fail_in(h, URGYM_ERR_ARG, who, "the HEADS form needs both d_mu and d_log_std");
  if (!out) return fail_in(h, URGYM_ERR_ARG, who, "null out");
  float* const tensors[8] = {out->w0, out->b0, out->w1, out->b1, out->w_mu, out->b_mu, out->w_log_std, out->b_log_std};
  for (int i = 0; i < 8; i++) {
    if (!tensors[i]) return fail_in(h, URGYM_ERR_ARG, who, "a gradient pointer is null (all eight are required)");
    call.grad[i] = tensors[i];
  }
  if (!workspace) return fail_in(h, URGYM_ERR_ARG, who, "null workspace");
  if ((uintptr_t)workspace % 16 != 0) return fail_in(h, URGYM_ERR_ARG, who, "the workspace must be 16-byte aligned");
  if (workspace_bytes < actor_backward_workspace_bytes(a, count))
    return fail_in(h, URGYM_ERR_ARG, who, "the workspace is smaller than urgym_actor_parameter_gradients_workspace reports");
  call.M = count, call.obs_dim = h->obs_dim, call.goal_dim = h->goal_dim;
  call.mode = how->mode, call.seed = how->seed, call.draw = how->first_draw;
  call.d_action = upstream->d_action, call.d_log_prob = upstream->d_log_prob, call.d_mu = upstream->d_mu, call.d_log_std = upstream->d_log_std;
  call.action = out->action, call.log_prob = out->log_prob, call.noise = out->noise, call.log_std = out->log_std;
  call.out_d_mu = out->d_mu, call.out_d_log_std = out->d_log_std, call.std = out->std;
  call.workspace = (float*)workspace;
  *actor_out = a;
  return URGYM_OK;
}

}  // namespace

extern "C" {

// ---- Adam on the device (urgym_adam.hip): everything is checked here, before the launch
int urgym_adam_coefficients(const urgym_adam_hyper* hp, float out[7]) {
  if (const char* what = adam_hyper_refusal(hp)) return fail_in(nullptr, URGYM_ERR_ARG, "urgym_adam_coefficients", what);
  if (!out) return fail(nullptr, URGYM_ERR_ARG, "urgym_adam_coefficients: null out");
  const AdamCoef c = adam_coef(*hp);
  out[0] = c.b1, out[1] = c.omb1, out[2] = c.b2, out[3] = c.omb2, out[4] = c.step_size, out[5] = c.bc2_sqrt, out[6] = c.eps;
  return URGYM_OK;
}

int urgym_actor_adam_step(void* handle, void* actor, const urgym_actor_adam* t, const urgym_adam_hyper* hp, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  ActorAdamStep step;
  if (int rc = check_actor_adam(h, actor, t, hp, "urgym_actor_adam_step", &step)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  actor_adam_launch(step.buf, step.T, adam_coef(*hp), (hipStream_t)stream);
  HIP_TRY(h, hipGetLastError());
  actor_mark_log_std(step.a);  // as urgym_actor_load with both head pointers
  return URGYM_OK;
}

int urgym_critic_adam_step(void* handle, void* online, void* target_or_NULL, const urgym_critic_adam* t, const urgym_adam_hyper* hp, float tau, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  CriticAdamStep step;
  if (int rc = check_critic_adam(h, online, target_or_NULL, t, hp, tau, "urgym_critic_adam_step", &step)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  critic_adam_launch(step.buf, step.has_target ? &step.target_buf : nullptr, step.T, adam_coef(*hp), tau, (hipStream_t)stream);
  return launched(h);
}

// ---- gradient-norm clipping (urgym_grad_clip.hip, the scaled kernels of urgym_adam.hip): everything is checked here, before the launch
int urgym_actor_grad_norm(void* handle, void* actor, const urgym_actor_tensors_const* grad, const urgym_grad_norm* args, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  GradNormCall c;
  if (int rc = check_actor_grad_norm(h, actor, grad, args, "urgym_actor_grad_norm", &c)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  grad_norm_launch(c, (hipStream_t)stream);
  return launched(h);
}

int urgym_critic_grad_norm(void* handle, void* critic, const urgym_q_network_dev grad[2], const urgym_grad_norm* args, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  GradNormCall c;
  if (int rc = check_critic_grad_norm(h, critic, grad, args, "urgym_critic_grad_norm", &c)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  grad_norm_launch(c, (hipStream_t)stream);
  return launched(h);
}

int urgym_actor_adam_step_scaled(void* handle, void* actor, const urgym_actor_adam* t, const urgym_adam_hyper* hp, const float* scale_dev, void* stream) {
  const char* who = "urgym_actor_adam_step_scaled";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  ActorAdamStep step;
  if (int rc = check_actor_adam(h, actor, t, hp, who, &step)) return rc;
  if (!scale_dev) return fail_in(h, URGYM_ERR_ARG, who, "null scale_dev");
  HIP_TRY(h, hipSetDevice(h->device));
  actor_adam_scaled_launch(step.buf, step.T, adam_coef(*hp), scale_dev, (hipStream_t)stream);
  HIP_TRY(h, hipGetLastError());
  actor_mark_log_std(step.a);  // as urgym_actor_adam_step
  return URGYM_OK;
}

int urgym_critic_adam_step_scaled(void* handle, void* online, void* target_or_NULL, const urgym_critic_adam* t, const urgym_adam_hyper* hp, float tau, const float* scale_dev, void* stream) {
  const char* who = "urgym_critic_adam_step_scaled";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  CriticAdamStep step;
  if (int rc = check_critic_adam(h, online, target_or_NULL, t, hp, tau, who, &step)) return rc;
  if (!scale_dev) return fail_in(h, URGYM_ERR_ARG, who, "null scale_dev");
  HIP_TRY(h, hipSetDevice(h->device));
  critic_adam_scaled_launch(step.buf, step.has_target ? &step.target_buf : nullptr, step.T, adam_coef(*hp), tau, scale_dev, (hipStream_t)stream);
  return launched(h);
}

// ---- SAC's entropy coefficient on the device (urgym_sac_terms.hip): everything is checked here, before the launch
int urgym_sac_entropy_step(void* handle, const urgym_sac_entropy_args* args, const urgym_adam_hyper* hp, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  SacEntropyCall c;
  if (int rc = check_entropy_step(h, args, hp, "urgym_sac_entropy_step", &c)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  sac_entropy_launch(c, (hipStream_t)stream);
  return launched(h);
}

int urgym_sac_entropy_step_nstep(void* handle, const urgym_sac_entropy_nstep_args* args, const urgym_adam_hyper* hp, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  SacEntropyNstepCall c;
  if (int rc = check_entropy_step_nstep(h, args, hp, "urgym_sac_entropy_step_nstep", &c)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  sac_entropy_nstep_launch(c, (hipStream_t)stream);
  return launched(h);
}

int urgym_sac_policy_terms(void* handle, const urgym_sac_policy_args* args, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  SacPolicyCall c;
  if (int rc = check_policy_terms(h, args, "urgym_sac_policy_terms", &c)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  sac_policy_launch(c, (hipStream_t)stream);
  return launched(h);
}

// the policy terms with behaviour cloning (urgym_sac_bc.hip)
int urgym_sac_policy_terms_cloned(void* handle, const urgym_sac_policy_args* args, const urgym_sac_clone_args* clone, void* stream) {
  const char* who = "urgym_sac_policy_terms_cloned";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  SacPolicyCall c;
  SacCloneCall b;
  if (int rc = check_policy_terms(h, args, who, &c)) return rc;
  if (int rc = check_policy_terms_cloned(h, c, clone, who, &b)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  sac_policy_bc_launch(c, b, (hipStream_t)stream);
  return launched(h);
}

// the cloned policy terms on marked rows only (urgym_sac_bc_masked.hip)
int urgym_sac_policy_terms_cloned_masked(void* handle, const urgym_sac_policy_args* args, const urgym_sac_clone_args* clone, const uint8_t* row_mask, void* stream) {
  const char* who = "urgym_sac_policy_terms_cloned_masked";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  SacPolicyCall c;
  SacCloneCall b;
  if (int rc = check_policy_terms(h, args, who, &c)) return rc;
  if (int rc = check_policy_terms_cloned(h, c, clone, who, &b)) return rc;
  if (!row_mask) return fail_in(h, URGYM_ERR_ARG, who, "null row_mask");
  HIP_TRY(h, hipSetDevice(h->device));
  sac_policy_bc_masked_launch(c, b, row_mask, (hipStream_t)stream);
  return launched(h);
}

// the cloned policy terms with the advantage weight in the place of the verdict (urgym_sac_bc_weighted.hip)
int urgym_sac_policy_terms_weighted(void* handle, const urgym_sac_policy_args* args, const urgym_sac_clone_args* clone, const urgym_sac_advantage_args* advantage, void* stream) {
  const char* who = "urgym_sac_policy_terms_weighted";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  SacPolicyCall c;
  SacCloneCall b;
  SacAdvantageCall w;
  if (int rc = check_policy_terms(h, args, who, &c)) return rc;
  if (int rc = check_policy_terms_cloned(h, c, clone, who, &b)) return rc;
  if (int rc = check_policy_terms_weighted(h, b, advantage, who, &w)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  sac_policy_bc_weighted_launch(c, b, w, (hipStream_t)stream);
  return launched(h);
}

// ---- weights from the device (urgym_weights.hip): everything is checked here, before the launch
int urgym_actor_load(void* handle, void* actor, const urgym_actor_params_dev* p, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  Actor* a = member(h->actors, actor);
  if (!a) return fail(h, URGYM_ERR_ARG, "urgym_actor_load: not an actor of this handle (actors belong to the handle they were created with)");
  if (!p) return fail(h, URGYM_ERR_ARG, "urgym_actor_load: null params");
  if (p->reserved0 != 0) return fail(h, URGYM_ERR_ARG, "urgym_actor_load: reserved0 must be 0");
  const ActorPacked buf = actor_packed(a);
  if (p->in_features != buf.in_features || p->hidden_width != buf.hidden)
    return failf(h, URGYM_ERR_ARG, "urgym_actor_load: params are %d -> %d, the actor is %d -> %d", p->in_features, p->hidden_width, buf.in_features, buf.hidden);
  if (!p->w0 || !p->b0 || !p->w1 || !p->b1 || !p->w_mu || !p->b_mu) return fail(h, URGYM_ERR_ARG, "urgym_actor_load: a weight or bias pointer is null");
  if (!p->w_log_std != !p->b_log_std) return fail(h, URGYM_ERR_ARG, "urgym_actor_load: the log_std head needs both w_log_std and b_log_std, or neither");
  HIP_TRY(h, hipSetDevice(h->device));
  const float* src[PACK_ACTOR_TENSORS] = {p->w0, p->b0, p->w1, p->b1, p->w_mu, p->b_mu, p->w_log_std, p->b_log_std};
  actor_pack_launch(buf, src, (hipStream_t)stream);
  HIP_TRY(h, hipGetLastError());
  if (p->w_log_std) actor_mark_log_std(a);  // the checks of later calls are made in program order, which is stream order for this stream
  return URGYM_OK;
}

int urgym_critic_load(void* handle, void* critic, const urgym_critic_params_dev* p, float tau, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  Critic* c = member(h->critics, critic);
  if (!c) return fail(h, URGYM_ERR_ARG, "urgym_critic_load: not a critic of this handle (critics belong to the handle they were created with)");
  if (!p) return fail(h, URGYM_ERR_ARG, "urgym_critic_load: null params");
  if (p->reserved0 != 0) return fail(h, URGYM_ERR_ARG, "urgym_critic_load: reserved0 must be 0");
  if (!(tau > 0.0f && tau <= 1.0f)) return fail(h, URGYM_ERR_ARG, "urgym_critic_load: tau must be in (0, 1]");  // refuses NaN too
  const CriticPacked buf = critic_packed(c);
  if (p->in_features != buf.in_features || p->hidden_width != buf.hidden)
    return failf(h, URGYM_ERR_ARG, "urgym_critic_load: params are %d -> %d, the critic is %d -> %d", p->in_features, p->hidden_width, buf.in_features, buf.hidden);
  const float* src[2 * PACK_CRITIC_TENSORS];
  for (int net = 0; net < 2; net++) {
    const urgym_q_network_dev& q = p->qf[net];
    if (!q.w0 || !q.b0 || !q.w1 || !q.b1 || !q.w_q || !q.b_q) return fail(h, URGYM_ERR_ARG, "urgym_critic_load: a weight or bias pointer is null");
    const float* one[PACK_CRITIC_TENSORS] = {q.w0, q.b0, q.w1, q.b1, q.w_q, q.b_q};
    for (int i = 0; i < PACK_CRITIC_TENSORS; i++) src[PACK_CRITIC_TENSORS * net + i] = one[i];
  }
  HIP_TRY(h, hipSetDevice(h->device));
  critic_pack_launch(buf, src, tau, (hipStream_t)stream);
  return launched(h);
}

// ---- weights back to device tensors (the unpack kernels of urgym_weights.hip): a checking half that launches nothing and leaves what
// the launching half needs, like the entry points urgym_sac_train composes
namespace {

struct ActorUnpack {
  ActorPacked buf;
  float* dst[PACK_ACTOR_TENSORS];
};
struct CriticUnpack {
  CriticPacked buf;
  float* dst[2 * PACK_CRITIC_TENSORS];
};

int check_actor_unpack(Handle* h, void* actor, const urgym_actor_params_out* p, const char* who, ActorUnpack* call) {
  Actor* a = member(h->actors, actor);
  if (!a) return fail_in(h, URGYM_ERR_ARG, who, "not an actor of this handle (actors belong to the handle they were created with)");
  if (!p) return fail_in(h, URGYM_ERR_ARG, who, "null out");
  if (p->reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "reserved0 must be 0");
  call->buf = actor_packed(a);
  if (p->in_features != call->buf.in_features || p->hidden_width != call->buf.hidden)
    return failf(h, URGYM_ERR_ARG, "%s: out is %d -> %d, the actor is %d -> %d", who, p->in_features, p->hidden_width, call->buf.in_features, call->buf.hidden);
  float* const dst[PACK_ACTOR_TENSORS] = {p->w0, p->b0, p->w1, p->b1, p->w_mu, p->b_mu, p->w_log_std, p->b_log_std};
  static const char* const names[PACK_ACTOR_TENSORS] = {"w0", "b0", "w1", "b1", "w_mu", "b_mu", "w_log_std", "b_log_std"};
  for (int i = 0; i <= PACK_B_OUT; i++)
    if (!dst[i]) return failf(h, URGYM_ERR_ARG, "%s: out->%s is null", who, names[i]);
  if (!p->w_log_std != !p->b_log_std) return fail_in(h, URGYM_ERR_ARG, who, "the log_std head needs both w_log_std and b_log_std, or neither");
  if (p->w_log_std && !actor_has_log_std(a)) return fail_in(h, URGYM_ERR_ARG, who, "the actor has no log_std head (urgym_actor_set_log_std): w_log_std and b_log_std must be null");
  for (int i = 0; i < PACK_ACTOR_TENSORS; i++) call->dst[i] = dst[i];
  return URGYM_OK;
}

int check_critic_unpack(Handle* h, void* critic, const urgym_critic_params_out* p, const char* who, CriticUnpack* call) {
  Critic* c = member(h->critics, critic);
  if (!c) return fail_in(h, URGYM_ERR_ARG, who, "not a critic of this handle (critics belong to the handle they were created with)");
  if (!p) return fail_in(h, URGYM_ERR_ARG, who, "null out");
  if (p->reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "reserved0 must be 0");
  call->buf = critic_packed(c);
  if (p->in_features != call->buf.in_features || p->hidden_width != call->buf.hidden)
    return failf(h, URGYM_ERR_ARG, "%s: out is %d -> %d, the critic is %d -> %d", who, p->in_features, p->hidden_width, call->buf.in_features, call->buf.hidden);
  static const char* const names[PACK_CRITIC_TENSORS] = {"w0", "b0", "w1", "b1", "w_q", "b_q"};
  for (int net = 0; net < 2; net++) {
    const urgym_q_network_out& q = p->qf[net];
    float* const one[PACK_CRITIC_TENSORS] = {q.w0, q.b0, q.w1, q.b1, q.w_q, q.b_q};
    for (int i = 0; i < PACK_CRITIC_TENSORS; i++) {
      if (!one[i]) return failf(h, URGYM_ERR_ARG, "%s: out->qf[%d].%s is null", who, net, names[i]);
      call->dst[PACK_CRITIC_TENSORS * net + i] = one[i];
    }
  }
  return URGYM_OK;
}

}  // namespace

int urgym_actor_unpack(void* handle, void* actor, const urgym_actor_params_out* out, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  ActorUnpack call;
  if (int rc = check_actor_unpack(h, actor, out, "urgym_actor_unpack", &call)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  actor_unpack_launch(call.buf, call.dst, (hipStream_t)stream);
  return launched(h);
}

int urgym_critic_unpack(void* handle, void* critic, const urgym_critic_params_out* out, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  CriticUnpack call;
  if (int rc = check_critic_unpack(h, critic, out, "urgym_critic_unpack", &call)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  critic_unpack_launch(call.buf, call.dst, (hipStream_t)stream);
  return launched(h);
}

int urgym_actor_read_packed(void* handle, void* actor, float* host_out, uint64_t capacity, uint64_t* count) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  Actor* a = member(h->actors, actor);
  if (!a) return fail(h, URGYM_ERR_ARG, "urgym_actor_read_packed: not an actor of this handle");
  const ActorPacked buf = actor_packed(a);
  return read_packed(h, "urgym_actor_read_packed", buf.weights, buf.floats, host_out, capacity, count);
}

int urgym_critic_read_packed(void* handle, void* critic, float* host_out, uint64_t capacity, uint64_t* count) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  Critic* c = member(h->critics, critic);
  if (!c) return fail(h, URGYM_ERR_ARG, "urgym_critic_read_packed: not a critic of this handle");
  const CriticPacked buf = critic_packed(c);
  return read_packed(h, "urgym_critic_read_packed", buf.weights, buf.floats, host_out, capacity, count);
}

int urgym_actor_create(void* handle, const urgym_actor_desc* desc, void** actor) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!actor) return fail(h, URGYM_ERR_ARG, "urgym_actor_create: null argument");
  HIP_TRY(h, hipSetDevice(h->device));
  Actor* a = nullptr;
  if (int rc = actor_create(desc, actor_features(h), h->cfg.num_envs, &a, h->err, sizeof(h->err))) return rc;
  h->actors.push_back(a);
  *actor = a;
  return URGYM_OK;
}

int urgym_actor_destroy(void* handle, void* actor) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  return destroy_member(h, h->actors, actor, actor_destroy, "urgym_actor_destroy: not an actor of this handle");
}

int urgym_actor_forward(void* handle, void* actor, float* actions_dev, void* stream) {
  Handle* h = (Handle*)handle;
  Actor* a = nullptr;
  if (int rc = enter_actor(h, actor, "urgym_actor_forward", &a)) return rc;
  if (!actions_dev) return fail(h, URGYM_ERR_ARG, "urgym_actor_forward: null actions");
  actor_launch(a, actor_env(h), actions_dev, nullptr, (hipStream_t)stream);
  return launched(h);
}

int urgym_rollout_actor(void* handle, void* actor, int num_steps, const urgym_trajectory* traj, void* stream) {
  Handle* h = (Handle*)handle;
  Actor* a = nullptr;
  if (int rc = enter_actor(h, actor, "urgym_rollout_actor", &a)) return rc;
  if (num_steps < 0) return fail(h, URGYM_ERR_ARG, "urgym_rollout_actor: num_steps < 0");
  return rollout(h, a, nullptr, num_steps, RolloutSinks{traj, nullptr, nullptr, 0}, (hipStream_t)stream);
}

int urgym_actor_set_log_std(void* handle, void* actor, const float* w_log_std, const float* b_log_std) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  Actor* a = member(h->actors, actor);
  if (!a) return fail(h, URGYM_ERR_ARG, "urgym_actor_set_log_std: not an actor of this handle");
  if (!w_log_std || !b_log_std) return fail(h, URGYM_ERR_ARG, "urgym_actor_set_log_std: a weight or bias pointer is null");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipDeviceSynchronize());  // launches that read the head may still be in flight
  return actor_set_log_std(a, w_log_std, b_log_std, h->err, sizeof(h->err));
}

int urgym_actor_sample(void* handle, void* actor, const urgym_sampling* how, float* actions_dev, float* log_prob_dev, void* stream) {
  Handle* h = (Handle*)handle;
  Actor* a = nullptr;
  if (int rc = enter_actor(h, actor, "urgym_actor_sample", &a)) return rc;
  if (int rc = check_sampling(h, a, how, log_prob_dev != nullptr, "urgym_actor_sample")) return rc;
  if (!actions_dev) return fail(h, URGYM_ERR_ARG, "urgym_actor_sample: null actions");
  policy_launch(a, actor_env(h), actions_dev, nullptr, ActorSample{how->mode, how->seed, how->first_draw, log_prob_dev, nullptr, nullptr, nullptr},
                (hipStream_t)stream);
  return launched(h);
}

// With mode MEAN and no sample record asked for, every policy pass is the deterministic kernel: the launches of urgym_rollout_actor.
int urgym_rollout_sampled(void* handle, void* actor, const urgym_sampling* how, int num_steps, const urgym_trajectory* traj,
                          const urgym_sample_records* extra, void* stream) {
  Handle* h = (Handle*)handle;
  Actor* a = nullptr;
  if (int rc = enter_actor(h, actor, "urgym_rollout_sampled", &a)) return rc;
  const bool wants = extra && (extra->log_prob || extra->noise || extra->mean_action || extra->log_std);
  if (int rc = check_sampling(h, a, how, wants, "urgym_rollout_sampled")) return rc;
  if (num_steps < 0) return fail(h, URGYM_ERR_ARG, "urgym_rollout_sampled: num_steps < 0");
  return rollout(h, a, how, num_steps, RolloutSinks{traj, extra, nullptr, 0}, (hipStream_t)stream);
}

int urgym_actor_sample_rows(void* handle, void* actor, const urgym_sampling* how, const urgym_critic_rows* rows, int count, float* actions_dev, float* log_prob_dev, void* stream) {
  Handle* h = (Handle*)handle;
  SampleRows r;
  if (int rc = check_sample_rows(h, actor, how, rows, count, actions_dev, log_prob_dev, "urgym_actor_sample_rows", &r)) return rc;
  policy_launch(r.a, r.env, r.actions, nullptr, r.smp, (hipStream_t)stream);
  return launched(h);
}

// The launches of urgym_rollout_sampled without records, a store pass before each actor and one after the last step.
int urgym_rollout_collect(void* handle, void* actor, const urgym_sampling* how, int num_steps, const urgym_replay_ring* ring, int first_slot, void* stream) {
  Handle* h = (Handle*)handle;
  Actor* a = nullptr;
  if (int rc = check_collect(h, actor, how, num_steps, ring, first_slot, "urgym_rollout_collect", &a)) return rc;
  return rollout(h, a, how, num_steps, RolloutSinks{nullptr, nullptr, ring, first_slot}, (hipStream_t)stream);
}

int urgym_replay_sample(void* handle, const urgym_replay_ring* ring, int oldest_slot, int filled_steps, uint64_t seed, uint64_t draw, int count, const urgym_replay_batch* batch, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  ReplayGather g;
  if (int rc = check_replay_sample(h, ring, oldest_slot, filled_steps, seed, draw, count, batch, "urgym_replay_sample", &g)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  replay_gather_launch(g, (hipStream_t)stream);
  return launched(h);
}

// the mixed gather of the demonstration ring (urgym_demo.hip)
int urgym_replay_sample_mixed(void* handle, const urgym_replay_ring* ring, int oldest_slot, int filled_steps, uint64_t seed, uint64_t draw, int count, const urgym_replay_batch* batch, const urgym_replay_demonstrations* demo, uint8_t* source_out, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  ReplayGatherMixed g;
  if (int rc = check_replay_sample_mixed(h, ring, oldest_slot, filled_steps, seed, draw, count, batch, demo, source_out, "urgym_replay_sample_mixed", &g)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  replay_gather_mixed_launch(g, (hipStream_t)stream);
  return launched(h);
}

int urgym_replay_sample_nstep(void* handle, const urgym_replay_ring* ring, int oldest_slot, int filled_steps, uint64_t seed, uint64_t draw, int count, const urgym_replay_batch* batch, const urgym_replay_nstep* nstep, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  ReplayGatherNstep g;
  if (int rc = check_replay_sample_nstep(h, ring, oldest_slot, filled_steps, seed, draw, count, batch, nstep, "urgym_replay_sample_nstep", &g)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  replay_gather_nstep_launch(g, (hipStream_t)stream);
  return launched(h);
}

int urgym_replay_sample_hindsight(void* handle, const urgym_replay_ring* ring, int oldest_slot, int filled_steps, uint64_t seed, uint64_t draw, int count, const urgym_replay_batch* batch, const urgym_replay_hindsight* hindsight, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  ReplayGatherHindsight g;
  if (int rc = check_replay_sample_hindsight(h, ring, oldest_slot, filled_steps, seed, draw, count, batch, hindsight, "urgym_replay_sample_hindsight", &g)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  replay_gather_hindsight_launch(g, (hipStream_t)stream);
  return launched(h);
}

}  // extern "C"

// ---- prioritized replay (urgym_per.hip; urgym_per.h states the arithmetic): everything is checked here, before the first launch
namespace {

int check_priorities(Handle* h, const urgym_per_priorities* pri, const char* who, PerTree* out) {
  static_assert(URGYM_PER_FANOUT == PER_FANOUT && URGYM_PER_TERMS_MAX_COUNT == PER_TERMS_MAX_COUNT, "include/urgym.h");
  if (!pri) return fail_in(h, URGYM_ERR_ARG, who, "null priorities");
  if (pri->capacity_steps <= 0) return fail_in(h, URGYM_ERR_ARG, who, "priorities: capacity_steps must be positive");
  if (pri->reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_per_priorities.reserved0 must be 0");
  if (!pri->leaf || !pri->sums || !pri->max_leaf) return fail_in(h, URGYM_ERR_ARG, who, "a priorities pointer is null (leaf, sums, max_leaf)");
  const int64_t leaves = (int64_t)pri->capacity_steps * (int64_t)h->cfg.num_envs;
  if ((leaves + PER_FANOUT - 1) / PER_FANOUT > (int64_t)INT32_MAX) return fail_in(h, URGYM_ERR_ARG, who, "more than 2^31 - 1 level-1 entries");
  *out = PerTree{leaves, h->cfg.num_envs, pri->capacity_steps, pri->leaf, pri->sums, pri->max_leaf};
  return URGYM_OK;
}

// the leaves of `num_steps` slots from first_slot on as at most two runs, and the level-1 entries that overlap each
void per_fill_ranges(PerFill& f, int first_slot, int64_t num_steps) {
  const int64_t N = f.tree.N, C = f.tree.capacity;
  f.lo0 = f.hi0 = f.lo1 = f.hi1 = 0;
  if (num_steps >= C) {
    f.hi0 = f.tree.leaves;
  } else if (first_slot + num_steps <= C) {
    f.lo0 = first_slot * N, f.hi0 = (first_slot + num_steps) * N;
  } else {
    f.lo0 = first_slot * N, f.hi0 = f.tree.leaves;
    f.hi1 = (first_slot + num_steps - C) * N;
  }
  f.block0 = f.lo0 / PER_FANOUT, f.blocks0 = f.hi0 > f.lo0 ? (f.hi0 - 1) / PER_FANOUT - f.block0 + 1 : 0;
  f.block1 = f.lo1 / PER_FANOUT, f.blocks1 = f.hi1 > f.lo1 ? (f.hi1 - 1) / PER_FANOUT - f.block1 + 1 : 0;
}

int check_per_terms(Handle* h, const urgym_per_terms_args* args, const char* who, PerTermsCall* out) {
  if (!args) return fail_in(h, URGYM_ERR_ARG, who, "null args");
  const urgym_per_terms_args& a = *args;
  if (a.reserved0 != 0 || a.reserved1 != 0.0f) return fail_in(h, URGYM_ERR_ARG, who, "urgym_per_terms_args.reserved0 and reserved1 must be 0");
  if (a.count < 1 || a.count > PER_TERMS_MAX_COUNT) return fail_in(h, URGYM_ERR_ARG, who, "count must be in [1, URGYM_PER_TERMS_MAX_COUNT] (65536)");
  if (!a.leaf_in || !a.total || !a.q || !a.y || !a.w_raw || !a.w || !a.dq)
    return fail_in(h, URGYM_ERR_ARG, who, "a required pointer is null (leaf_in, total, q, y, w_raw, w, dq)");
  if (!(a.alpha >= 0.0f && a.alpha <= 1.0f)) return fail_in(h, URGYM_ERR_ARG, who, "alpha must be in [0, 1]");  // refuses NaN too
  if (!(a.beta >= 0.0f && a.beta <= 1.0f)) return fail_in(h, URGYM_ERR_ARG, who, "beta must be in [0, 1]");
  if (!(a.eps > 0.0f && a.eps < INFINITY)) return fail_in(h, URGYM_ERR_ARG, who, "eps must be positive and finite");
  if (!(a.size > 0.0f && a.size < INFINITY)) return fail_in(h, URGYM_ERR_ARG, who, "size must be positive and finite");
  if (!(fabsf(a.scale) < INFINITY)) return fail_in(h, URGYM_ERR_ARG, who, "scale must be finite");
  const urgym_per_priorities& p = a.priorities;
  const int given = (a.index != nullptr) + (a.new_leaf != nullptr) + (p.leaf != nullptr) + (p.sums != nullptr) + (p.max_leaf != nullptr);
  if (given != 0 && given != 5)
    return fail_in(h, URGYM_ERR_ARG, who, "the write-back group is half given: index, new_leaf and the three pointers of priorities go together");
  PerTermsCall& c = *out;
  memset(&c, 0, sizeof(c));
  if (given)
    if (int rc = check_priorities(h, &p, who, &c.tree)) return rc;
  c.count = a.count, c.size = a.size, c.beta = a.beta, c.alpha = a.alpha, c.eps = a.eps, c.scale = a.scale;
  c.leaf_in = a.leaf_in, c.total = a.total, c.q = a.q, c.y = a.y, c.w_raw = a.w_raw, c.w = a.w, c.dq = a.dq;
  c.index = a.index, c.new_leaf = a.new_leaf;
  return URGYM_OK;
}

}  // namespace

extern "C" {

int urgym_per_sums_count(void* handle, int capacity_steps, uint64_t* doubles) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  const char* who = "urgym_per_sums_count";
  if (!doubles) return fail_in(h, URGYM_ERR_ARG, who, "null doubles");
  if (capacity_steps <= 0) return fail_in(h, URGYM_ERR_ARG, who, "capacity_steps must be positive");
  const int64_t leaves = (int64_t)capacity_steps * (int64_t)h->cfg.num_envs;
  if ((leaves + PER_FANOUT - 1) / PER_FANOUT > (int64_t)INT32_MAX) return fail_in(h, URGYM_ERR_ARG, who, "more than 2^31 - 1 level-1 entries");
  *doubles = (uint64_t)per_shape<PER_FANOUT>(leaves).doubles;
  return URGYM_OK;
}

int urgym_per_rebuild(void* handle, const urgym_per_priorities* pri, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  PerFill f;
  memset(&f, 0, sizeof(f));
  if (int rc = check_priorities(h, pri, "urgym_per_rebuild", &f.tree)) return rc;
  f.blocks0 = per_shape<PER_FANOUT>(f.tree.leaves).count[1];  // every level-1 entry, no leaf written
  HIP_TRY(h, hipSetDevice(h->device));
  per_fill_launch(f, (hipStream_t)stream);
  return launched(h);
}

int urgym_per_fill(void* handle, const urgym_per_priorities* pri, int first_slot, int num_steps, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  const char* who = "urgym_per_fill";
  PerFill f;
  memset(&f, 0, sizeof(f));
  if (int rc = check_priorities(h, pri, who, &f.tree)) return rc;
  if (first_slot < 0 || first_slot >= pri->capacity_steps) return fail_in(h, URGYM_ERR_ARG, who, "first_slot outside [0, capacity_steps)");
  if (num_steps <= 0) return fail_in(h, URGYM_ERR_ARG, who, "num_steps must be positive");
  per_fill_ranges(f, first_slot, num_steps);
  HIP_TRY(h, hipSetDevice(h->device));
  per_fill_launch(f, (hipStream_t)stream);
  return launched(h);
}

int urgym_replay_sample_prioritized(void* handle, const urgym_replay_ring* ring, const urgym_per_priorities* pri, uint64_t seed, uint64_t draw, int count, const urgym_replay_batch* batch, float* leaf_out, double* total_out, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  const char* who = "urgym_replay_sample_prioritized";
  PerGather g;
  memset(&g, 0, sizeof(g));
  // filled_steps = C and oldest_slot = 0: the leaves, not a window of slots, say which entries can be drawn
  if (int rc = check_ring(h, ring, who)) return rc;
  if (int rc = check_replay_sample(h, ring, 0, ring->capacity_steps, seed, draw, count, batch, who, &g.g)) return rc;
  if (!batch->index) return fail_in(h, URGYM_ERR_ARG, who, "batch->index is required");
  if (int rc = check_priorities(h, pri, who, &g.tree)) return rc;
  if (pri->capacity_steps != ring->capacity_steps) return fail_in(h, URGYM_ERR_ARG, who, "priorities->capacity_steps is not the ring's");
  if (!leaf_out || !total_out) return fail_in(h, URGYM_ERR_ARG, who, "leaf_out or total_out is null");
  g.leaf_out = leaf_out, g.total_out = total_out;
  HIP_TRY(h, hipSetDevice(h->device));
  per_gather_launch(g, (hipStream_t)stream);
  return launched(h);
}

int urgym_per_terms(void* handle, const urgym_per_terms_args* args, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  PerTermsCall c;
  if (int rc = check_per_terms(h, args, "urgym_per_terms", &c)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  per_terms_launch(c, (hipStream_t)stream);
  return launched(h);
}

int urgym_critic_create(void* handle, const urgym_critic_desc* desc, void** critic) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!critic) return fail(h, URGYM_ERR_ARG, "urgym_critic_create: null argument");
  HIP_TRY(h, hipSetDevice(h->device));
  Critic* c = nullptr;
  if (int rc = critic_create(desc, actor_features(h) + 6, &c, h->err, sizeof(h->err))) return rc;
  h->critics.push_back(c);
  *critic = c;
  return URGYM_OK;
}

int urgym_critic_destroy(void* handle, void* critic) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  return destroy_member(h, h->critics, critic, critic_destroy, "urgym_critic_destroy: not a critic of this handle");
}

int urgym_critic_evaluate(void* handle, void* critic, const urgym_critic_rows* rows, int count, const urgym_critic_terms* terms, const urgym_critic_out* out, void* stream) {
  Handle* h = (Handle*)handle;
  Critic* c = nullptr;
  CriticCall call;
  if (int rc = check_critic_evaluate(h, critic, rows, count, terms, out, "urgym_critic_evaluate", &c, &call)) return rc;
  critic_launch(c, call, (hipStream_t)stream);
  return launched(h);
}

int urgym_critic_action_gradient(void* handle, void* critic, const urgym_critic_rows* rows, int count, const urgym_critic_grad_out* out, void* stream) {
  Handle* h = (Handle*)handle;
  Critic* c = nullptr;
  CriticGradCall call;
  if (int rc = check_critic_action_gradient(h, critic, rows, count, out, "urgym_critic_action_gradient", &c, &call)) return rc;
  critic_grad_launch(c, call, (hipStream_t)stream);
  return launched(h);
}

int urgym_critic_parameter_gradients_workspace(void* handle, void* critic, int count, uint64_t* bytes) {
  const char* who = "urgym_critic_parameter_gradients_workspace";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!bytes) return fail(h, URGYM_ERR_ARG, "urgym_critic_parameter_gradients_workspace: null bytes");
  Critic* c = nullptr;
  if (int rc = backward_critic(h, critic, count, who, &c)) return rc;
  *bytes = critic_backward_workspace_bytes(c, count);
  return URGYM_OK;
}

int urgym_critic_parameter_gradients(void* handle, void* critic, const urgym_critic_rows* rows, int count, const float* dq, const float* target, float scale, const urgym_critic_param_grads* out, void* workspace, uint64_t workspace_bytes, void* stream) {
  Handle* h = (Handle*)handle;
  Critic* c = nullptr;
  CriticBackwardCall call;
  if (int rc = check_critic_parameter_gradients(h, critic, rows, count, dq, target, scale, out, workspace, workspace_bytes, "urgym_critic_parameter_gradients", &c, &call)) return rc;
  critic_backward_launch(c, call, (hipStream_t)stream);
  return launched(h);
}

int urgym_actor_parameter_gradients_workspace(void* handle, void* actor, int count, uint64_t* bytes) {
  const char* who = "urgym_actor_parameter_gradients_workspace";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!bytes) return fail(h, URGYM_ERR_ARG, "urgym_actor_parameter_gradients_workspace: null bytes");
  Actor* a = nullptr;
  if (int rc = backward_actor(h, actor, count, who, &a)) return rc;
  *bytes = actor_backward_workspace_bytes(a, count);
  return URGYM_OK;
}

int urgym_actor_parameter_gradients(void* handle, void* actor, const urgym_sampling* how, const urgym_critic_rows* rows, int count, const urgym_actor_upstream* upstream, const urgym_actor_param_grads* out, void* workspace, uint64_t workspace_bytes, void* stream) {
  Handle* h = (Handle*)handle;
  Actor* a = nullptr;
  ActorBackwardCall call;
  if (int rc = check_actor_parameter_gradients(h, actor, how, rows, count, upstream, out, workspace, workspace_bytes, "urgym_actor_parameter_gradients", &a, &call)) return rc;
  actor_backward_launch(a, call, (hipStream_t)stream);
  return launched(h);
}

}  // extern "C"

// ---- normalization, evaluation and training-episode statistics: the checking halves first, in the order in which they build on each
// other (the training loop below composes all of them), then the features' own entry points

namespace {

// a required pointer and the name a NULL refusal gives it: urgym_sac_learner's, and those of the structs below
struct LearnerPointer {
  const char* name;
  const void* p;
};

// what a fold of num_steps slots from first_slot on refuses about the ring and the handle: urgym_monitor_fold's and urgym_norm_fold's
int check_fold_ring(Handle* h, const urgym_replay_ring* ring, int first_slot, int num_steps, const char* who) {
  if (int rc = check_ring(h, ring, who)) return rc;
  if (first_slot < 0 || first_slot >= ring->capacity_steps) return fail_in(h, URGYM_ERR_ARG, who, "first_slot outside [0, capacity_steps)");
  if (!ring->truncated || !ring->is_success) return fail_in(h, URGYM_ERR_ARG, who, "the ring keeps no truncated or no is_success (an episode's end and its success are read from them)");
  if (num_steps <= 0) return fail_in(h, URGYM_ERR_ARG, who, "num_steps must be positive");
  if (num_steps > ring->capacity_steps) return fail_in(h, URGYM_ERR_ARG, who, "num_steps is above capacity_steps (the ring no longer holds the earlier steps)");
  if (!h->cfg.auto_reset) return fail_in(h, URGYM_ERR_ARG, who, "the handle has auto_reset off (its episodes do not restart)");
  return URGYM_OK;
}

// ---- running observation and reward normalization (include/urgym.h, urgym_norm_workspace ... urgym_rollout_collect_normalized;
// DESIGN.md section 25).  As above each entry point is a checking half, which launches nothing and fills the launch struct of
// urgym_norm.h, and a launching half, which refuses nothing.

// the state's thirteen pointers, all given and 8-byte aligned, and the options
int check_normalization(Handle* h, const urgym_normalization* norm, const char* who) {
  static_assert(sizeof(urgym_norm_state) == 13 * sizeof(void*) && sizeof(urgym_normalization) == sizeof(urgym_norm_state) + 96, "include/urgym.h");
  if (!norm) return fail_in(h, URGYM_ERR_ARG, who, "null normalization");
  const urgym_norm_state& m = norm->state;
  const LearnerPointer required[] = {{"observation_mean", m.observation_mean},       {"observation_var", m.observation_var},     {"observation_count", m.observation_count},
                                     {"achieved_goal_mean", m.achieved_goal_mean},   {"achieved_goal_var", m.achieved_goal_var}, {"achieved_goal_count", m.achieved_goal_count},
                                     {"desired_goal_mean", m.desired_goal_mean},     {"desired_goal_var", m.desired_goal_var},   {"desired_goal_count", m.desired_goal_count},
                                     {"ret_mean", m.ret_mean},                       {"ret_var", m.ret_var},                     {"ret_count", m.ret_count},
                                     {"running_ret", m.running_ret}};
  for (const LearnerPointer& r : required) {
    if (!r.p) return failf(h, URGYM_ERR_ARG, "%s: urgym_norm_state.%s is null", who, r.name);
    if ((uintptr_t)r.p % 8 != 0) return failf(h, URGYM_ERR_ARG, "%s: urgym_norm_state.%s must be 8-byte aligned", who, r.name);
  }
  if (const char* what = norm_options_refusal(*norm)) return fail_in(h, URGYM_ERR_ARG, who, what);
  if (actor_features(h) + 1 > NORM_FEATURE_LANES || h->obs_dim > 48 || h->goal_dim > 48)
    return fail_in(h, URGYM_ERR_ARG, who, "the kernels are built for at most 63 features in all and 48 in a group");
  return URGYM_OK;
}

int check_norm_fold(Handle* h, const urgym_normalization* norm, const urgym_replay_ring* ring, int first_slot, int num_steps, const char* who, NormFoldCall* out) {
  if (int rc = check_normalization(h, norm, who)) return rc;
  if (int rc = check_fold_ring(h, ring, first_slot, num_steps, who)) return rc;  // urgym_monitor_fold's ring refusals
  if (num_steps >= 65535) return fail_in(h, URGYM_ERR_ARG, who, "num_steps must be below 65535 (one grid row per slot)");
  if (!norm->workspace) return fail_in(h, URGYM_ERR_ARG, who, "urgym_normalization.workspace is null");
  if ((uintptr_t)norm->workspace % 8 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_normalization.workspace must be 8-byte aligned");
  const uint64_t need = norm_workspace_doubles(h->cfg.num_envs, actor_features(h), num_steps) * sizeof(double);
  if (norm->workspace_bytes < need)
    return failf(h, URGYM_ERR_ARG, "%s: workspace_bytes is %llu, %d steps need %llu (urgym_norm_workspace)", who, (unsigned long long)norm->workspace_bytes, num_steps, (unsigned long long)need);
  NormFoldCall& c = *out;
  memset(&c, 0, sizeof(c));
  c.num_envs = h->cfg.num_envs, c.capacity = ring->capacity_steps, c.first_slot = first_slot, c.num_steps = num_steps;
  c.dim[0] = h->obs_dim, c.dim[1] = h->goal_dim, c.dim[2] = h->goal_dim;
  c.norm_obs = norm->norm_obs != 0, c.norm_reward = norm->norm_reward != 0, c.gamma = norm->gamma, c.state = norm->state;
  c.rows[0] = ring->observation, c.rows[1] = ring->achieved_goal, c.rows[2] = ring->desired_goal;
  c.reward = ring->reward, c.terminated = ring->terminated, c.truncated = ring->truncated, c.workspace = (double*)norm->workspace;
  return URGYM_OK;
}

// the three observation groups of `count` rows, src -> dst (each pair whole or absent), appended to the call's segments
const char* norm_row_segments(const Handle* h, const urgym_normalization& norm, const float* const src[3], float* const dst[3], NormApplyCall* c) {
  const urgym_norm_state& m = norm.state;
  const double* const mean[3] = {m.observation_mean, m.achieved_goal_mean, m.desired_goal_mean};
  const double* const var[3] = {m.observation_var, m.achieved_goal_var, m.desired_goal_var};
  const int dim[3] = {h->obs_dim, h->goal_dim, h->goal_dim};
  for (int g = 0; g < 3; g++) {
    if ((src[g] == nullptr) != (dst[g] == nullptr)) return "a source without its destination, or a destination without its source";
    if (!src[g]) continue;
    c->seg[c->segments++] = NormSegment{src[g], dst[g], mean[g], var[g], dim[g], norm.clip_obs};
  }
  return nullptr;
}

int check_norm_rows(Handle* h, const urgym_normalization* norm, const urgym_norm_rows_args* rows, int count, const char* who, NormApplyCall* out) {
  if (int rc = check_normalization(h, norm, who)) return rc;
  if (!rows) return fail_in(h, URGYM_ERR_ARG, who, "null rows");
  if (count <= 0) return fail_in(h, URGYM_ERR_ARG, who, "count must be positive");
  memset(out, 0, sizeof(*out));
  out->count = count, out->eps = norm->eps, out->identity = norm->norm_obs == 0;
  const float* const src[3] = {rows->observation, rows->achieved_goal, rows->desired_goal};
  float* const dst[3] = {rows->observation_out, rows->achieved_goal_out, rows->desired_goal_out};
  if (const char* what = norm_row_segments(h, *norm, src, dst, out)) return fail_in(h, URGYM_ERR_ARG, who, what);
  if (out->segments == 0) return fail_in(h, URGYM_ERR_ARG, who, "no group is given");
  return URGYM_OK;
}

// segments == 0 afterwards: nothing to launch
int check_norm_batch(Handle* h, const urgym_normalization* norm, const urgym_replay_batch* batch, int count, const char* who, NormApplyCall* out) {
  if (int rc = check_normalization(h, norm, who)) return rc;
  if (!batch) return fail_in(h, URGYM_ERR_ARG, who, "null batch");
  if (count <= 0) return fail_in(h, URGYM_ERR_ARG, who, "count must be positive");
  memset(out, 0, sizeof(*out));
  out->count = count, out->eps = norm->eps;
  if (norm->norm_obs != 0) {
    float* const now[3] = {batch->observation, batch->achieved_goal, batch->desired_goal};
    float* const next[3] = {batch->next_observation, batch->next_achieved_goal, batch->next_desired_goal};
    norm_row_segments(h, *norm, now, now, out);
    norm_row_segments(h, *norm, next, next, out);
  }
  if (norm->norm_reward != 0 && batch->reward)
    out->seg[out->segments++] = NormSegment{batch->reward, batch->reward, nullptr, norm->state.ret_var, 1, norm->clip_reward};
  return URGYM_OK;
}

// the twelve pointers of a state that is read or written without its running_ret
int check_norm_state12(Handle* h, const urgym_norm_state* st, const char* who, const char* what) {
  if (!st) return failf(h, URGYM_ERR_ARG, "%s: null %s", who, what);
  const void* const p[12] = {st->observation_mean,   st->observation_var,  st->observation_count,  st->achieved_goal_mean, st->achieved_goal_var, st->achieved_goal_count,
                             st->desired_goal_mean,  st->desired_goal_var, st->desired_goal_count, st->ret_mean,           st->ret_var,           st->ret_count};
  for (const void* q : p)
    if (!q || (uintptr_t)q % 8 != 0) return failf(h, URGYM_ERR_ARG, "%s: a pointer of %s is null or not 8-byte aligned (mean, var and count of the four groups)", who, what);
  return URGYM_OK;
}

int check_norm_snapshot(Handle* h, const urgym_norm_state* source, const urgym_norm_state* destination, const int32_t* when, const char* who, NormSnapshotCall* out) {
  if (int rc = check_norm_state12(h, source, who, "source state")) return rc;
  if (int rc = check_norm_state12(h, destination, who, "destination state")) return rc;
  if (actor_features(h) + 1 > NORM_FEATURE_LANES) return fail_in(h, URGYM_ERR_ARG, who, "the kernels are built for at most 63 features in all");
  memset(out, 0, sizeof(*out));
  out->dim[0] = h->obs_dim, out->dim[1] = h->goal_dim, out->dim[2] = h->goal_dim;
  out->src = *source, out->dst = *destination, out->when = when;
  return URGYM_OK;
}

// ---- evaluation inside the training call (include/urgym.h, urgym_eval_stats ... urgym_sac_train_evaluated).
// As above each entry point is a checking half, which launches nothing and fills the launch struct of urgym_eval.h, and a launching
// half, which refuses nothing.

int check_eval_stats(Handle* h, const urgym_eval_stats_args* args, const char* who, EvalStatsCall* out) {
  static_assert(sizeof(urgym_eval_record) == 72 && alignof(urgym_eval_record) == 8, "include/urgym.h");
  if (!args) return fail_in(h, URGYM_ERR_ARG, who, "null args");
  const urgym_eval_stats_args& a = *args;
  if (a.reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_eval_stats_args.reserved0 must be 0");
  if (a.count < 1 || a.count > SAC_TERMS_MAX_COUNT) return fail_in(h, URGYM_ERR_ARG, who, "count must be in [1, URGYM_SAC_TERMS_MAX_COUNT] (65536)");
  if (a.eval_index < 0) return fail_in(h, URGYM_ERR_ARG, who, "eval_index is negative");
  const LearnerPointer required[] = {{"episode_return", a.episode_return}, {"episode_last_step", a.episode_last_step}, {"episode_success", a.episode_success},
                                     {"best_mean", a.best_mean},           {"best_index", a.best_index},               {"record", a.record}};
  for (const LearnerPointer& r : required)
    if (!r.p) return failf(h, URGYM_ERR_ARG, "%s: urgym_eval_stats_args.%s is null", who, r.name);
  if ((uintptr_t)a.record % 8 != 0 || (uintptr_t)a.best_mean % 8 != 0 || (uintptr_t)a.best_index % 8 != 0 || (uintptr_t)a.episode_return % 8 != 0)
    return fail_in(h, URGYM_ERR_ARG, who, "record, best_mean, best_index and episode_return must be 8-byte aligned");
  *out = EvalStatsCall{a.count, a.eval_index, a.episode_return, a.episode_last_step, a.episode_success, a.best_mean, a.best_index, a.record};
  return URGYM_OK;
}

int check_actor_snapshot(Handle* h, const urgym_actor_snapshot_args* args, const char* who, ActorSnapshotCall* out) {
  if (!args) return fail_in(h, URGYM_ERR_ARG, who, "null args");
  const urgym_actor_snapshot_args& a = *args;
  if (a.reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_actor_snapshot_args.reserved0 must be 0");
  if (a.in_features < 1) return fail_in(h, URGYM_ERR_ARG, who, "in_features must be positive");
  if (a.hidden_width < 1 || a.hidden_width > 512) return fail_in(h, URGYM_ERR_ARG, who, "hidden_width must be in [1, 512]");
  const urgym_actor_tensors_const& f = a.source;
  const urgym_actor_tensors& t = a.destination;
  const float* const src[ACTOR_SNAPSHOT_TENSORS] = {f.w0, f.b0, f.w1, f.b1, f.w_mu, f.b_mu, f.w_log_std, f.b_log_std};
  float* const dst[ACTOR_SNAPSHOT_TENSORS] = {t.w0, t.b0, t.w1, t.b1, t.w_mu, t.b_mu, t.w_log_std, t.b_log_std};
  for (int i = 0; i < ACTOR_SNAPSHOT_TENSORS; i++) {
    if (!src[i] || !dst[i]) return fail_in(h, URGYM_ERR_ARG, who, "a tensor pointer is null (all sixteen are required)");
    out->src[i] = src[i], out->dst[i] = dst[i];
  }
  actor_snapshot_offsets(a.in_features, a.hidden_width, out->first);
  out->when = a.when;
  return URGYM_OK;
}

// what urgym_policy_evaluate launches: the five calls of its sequence, checked
struct PolicyEvaluation {
  Handle* eh;
  Actor* actor;
  ActorPacked buf;
  const float* src[PACK_ACTOR_TENSORS];
  urgym_trajectory traj;
  int num_steps;
  uint64_t reset_seed;
  urgym_eval_record* records;
  EvalStatsCall stats;       // record and eval_index move per evaluation
  ActorSnapshotCall snapshot;  // when moves per evaluation
  bool normalized, normalized_rows;  // urgym_policy_evaluate_normalized; ... with norm_obs on
  NormApplyCall norm;                // the evaluation handle's bound rows into eval_scratch
  NormSnapshotCall norm_snapshot;    // when moves per evaluation
};

// What urgym_policy_evaluate_normalized checks beyond urgym_policy_evaluate, after check_policy_evaluation has filled `out`.  The
// dimensions are the evaluation handle's; messages go to `report`.
int check_evaluation_normalization(Handle* report, Handle* eh, const urgym_normalization* norm, const char* who, PolicyEvaluation* out) {
  auto relay = [&](int rc) { return report == eh ? rc : failf(report, rc, "%.200s", eh->err); };
  if (int rc = check_normalization(eh, norm, who)) return relay(rc);
  if (!norm->eval_scratch) return fail_in(report, URGYM_ERR_ARG, who, "urgym_normalization.eval_scratch is null");
  if (int rc = check_norm_snapshot(eh, &norm->state, norm->best_state, nullptr, who, &out->norm_snapshot)) return relay(rc);
  out->normalized = true, out->normalized_rows = norm->norm_obs != 0;
  if (out->normalized_rows) {
    const size_t n = (size_t)eh->cfg.num_envs;
    float* const ach = norm->eval_scratch + n * (size_t)eh->obs_dim;
    const urgym_norm_rows_args rows{eh->buf.observation, eh->buf.achieved_goal, eh->buf.desired_goal, norm->eval_scratch, ach, ach + n * (size_t)eh->goal_dim};
    if (int rc = check_norm_rows(eh, norm, &rows, eh->cfg.num_envs, who, &out->norm)) return relay(rc);
  }
  return URGYM_OK;
}

// Every check of urgym_policy_evaluate but those of eval_index and record_slot (check_evaluation_slot).  Messages go to `report` -- the
// evaluation handle itself, or the training handle of urgym_sac_train_evaluated.
int check_policy_evaluation(Handle* report, Handle* eh, const urgym_policy_evaluation* evaluation, const char* who, PolicyEvaluation* out) {
  static_assert(PACK_ACTOR_TENSORS == ACTOR_SNAPSHOT_TENSORS, "urgym_actor_tensors' eight");
  if (!eh) return fail_in(report, URGYM_ERR_ARG, who, "null evaluation handle");
  if (!eh->bound) return fail_in(report, URGYM_ERR_STATE, who, "urgym_bind() has not been called on the evaluation handle");
  if (!evaluation) return fail_in(report, URGYM_ERR_ARG, who, "null evaluation");
  const urgym_policy_evaluation& e = *evaluation;
  if (e.reserved0 != 0) return fail_in(report, URGYM_ERR_ARG, who, "urgym_policy_evaluation.reserved0 must be 0");
  if (eh->cfg.auto_reset) return fail_in(report, URGYM_ERR_ARG, who, "the evaluation handle has auto_reset on (the episode summary is that of whole first episodes)");
  if (eh->cfg.num_envs > SAC_TERMS_MAX_COUNT) return fail_in(report, URGYM_ERR_ARG, who, "the evaluation handle has more than 65536 envs (URGYM_SAC_TERMS_MAX_COUNT)");
  if (e.num_steps < 1) return fail_in(report, URGYM_ERR_ARG, who, "num_steps must be at least 1");
  if (e.record_capacity < 1) return fail_in(report, URGYM_ERR_ARG, who, "record_capacity must be at least 1");
  if (!e.eval_actor) return fail_in(report, URGYM_ERR_ARG, who, "urgym_policy_evaluation.eval_actor is null");
  Actor* a = member(eh->actors, e.eval_actor);
  if (!a) return fail_in(report, URGYM_ERR_ARG, who, "eval_actor is not an actor of the evaluation handle (actors belong to the handle they were created with)");
  if (actor_in_features(a) != actor_features(eh))
    return failf(report, URGYM_ERR_ARG, "%s: the eval actor takes %d features, the evaluation env kind offers %d", who, actor_in_features(a), actor_features(eh));
  const ActorPacked buf = actor_packed(a);
  if (e.in_features != buf.in_features || e.hidden_width != buf.hidden)
    return failf(report, URGYM_ERR_ARG, "%s: the source is %d -> %d, the eval actor is %d -> %d", who, e.in_features, e.hidden_width, buf.in_features, buf.hidden);
  const LearnerPointer required[] = {{"episode_return", e.episode_return}, {"episode_last_step", e.episode_last_step}, {"episode_success", e.episode_success},
                                     {"episode_done", e.episode_done},     {"records", e.records},                     {"best_mean", e.best_mean},
                                     {"best_index", e.best_index}};
  for (const LearnerPointer& r : required)
    if (!r.p) return failf(report, URGYM_ERR_ARG, "%s: urgym_policy_evaluation.%s is null", who, r.name);
  PolicyEvaluation& c = *out;
  memset(&c, 0, sizeof(c));
  // the snapshot's checks: all sixteen tensors, the shape
  urgym_actor_snapshot_args sa;
  memset(&sa, 0, sizeof(sa));
  sa.in_features = e.in_features, sa.hidden_width = e.hidden_width, sa.source = e.source, sa.destination = e.best;
  if (int rc = check_actor_snapshot(report, &sa, who, &c.snapshot)) return rc;
  // the statistics' checks, on slot 0 (every slot has its alignment: the record is a multiple of 8 bytes)
  urgym_eval_stats_args ea;
  memset(&ea, 0, sizeof(ea));
  ea.count = eh->cfg.num_envs, ea.episode_return = e.episode_return, ea.episode_last_step = e.episode_last_step, ea.episode_success = e.episode_success;
  ea.best_mean = e.best_mean, ea.best_index = e.best_index, ea.record = e.records;
  if (int rc = check_eval_stats(report, &ea, who, &c.stats)) return rc;
  c.eh = eh, c.actor = a, c.buf = buf;
  for (int i = 0; i < PACK_ACTOR_TENSORS; i++) c.src[i] = c.snapshot.src[i];  // urgym_actor_load's order is urgym_actor_tensors'
  c.traj.episode_return = e.episode_return, c.traj.episode_last_step = e.episode_last_step;
  c.traj.episode_success = e.episode_success, c.traj.episode_done = e.episode_done;
  c.num_steps = e.num_steps, c.reset_seed = e.reset_seed, c.records = e.records;
  return URGYM_OK;
}

int check_evaluation_slot(Handle* report, const urgym_policy_evaluation& e, int64_t eval_index, int32_t record_slot, const char* who) {
  if (eval_index < 0) return fail_in(report, URGYM_ERR_ARG, who, "eval_index is negative");
  if (record_slot < 0 || record_slot >= e.record_capacity) return fail_in(report, URGYM_ERR_ARG, who, "record_slot outside [0, record_capacity)");
  return URGYM_OK;
}

// the launching half: the five calls on `s`.  A failure leaves its message in the evaluation handle.
int launch_policy_evaluation(PolicyEvaluation& c, int64_t eval_index, int32_t record_slot, hipStream_t s) {
  Handle* eh = c.eh;
  HIP_TRY(eh, hipSetDevice(eh->device));
  actor_pack_launch(c.buf, c.src, s);  // urgym_actor_load with both head pointers
  HIP_TRY(eh, hipGetLastError());
  actor_mark_log_std(c.actor);
  // env.reset(seed=): a seeded reset of every env rewinds the episode counters, so that it starts the same episodes every time
  HIP_TRY(eh, hipMemsetAsync(eh->buf.episode_id, 0, sizeof(int32_t) * (size_t)eh->cfg.num_envs, s));
  // ... and on an environment that looks fresh: RESET leaves the velocity slot of the UR5DynReach-v1 observation as it finds it (the
  // reference's stale ReachDyn.velocity, reach.py:657), so without this the first evaluation of a handle would see zeros there and every
  // later one the twist of the previous evaluation's last step -- other first observations, other returns, no fair comparison
  HIP_TRY(eh, hipMemsetAsync(eh->buf.observation, 0, sizeof(float) * (size_t)eh->cfg.num_envs * (size_t)eh->obs_dim, s));
  if (int rc = urgym_reset(eh, nullptr, c.reset_seed, s)) return rc;
  if (int rc = rollout(eh, c.actor, nullptr, c.num_steps, RolloutSinks{&c.traj, nullptr, nullptr, 0}, s, c.normalized_rows ? &c.norm : nullptr)) return rc;
  urgym_eval_record* record = c.records + record_slot;
  c.stats.eval_index = eval_index, c.stats.record = record;
  eval_stats_launch(c.stats, s);
  HIP_TRY(eh, hipGetLastError());
  c.snapshot.when = &record->improved;
  actor_snapshot_launch(c.snapshot, s);
  if (c.normalized) {  // the statistics the actor was selected under, beside it
    HIP_TRY(eh, hipGetLastError());
    c.norm_snapshot.when = &record->improved;
    norm_snapshot_launch(c.norm_snapshot, s);
  }
  return launched(eh);
}

// ---- training-episode statistics (include/urgym.h, urgym_monitor_fold ... urgym_sac_train_monitored).  As above
// each entry point is a checking half, which launches nothing and fills the launch struct of urgym_monitor.h, and a launching half,
// which refuses nothing.

// the six state pointers: all given, the 8-byte ones aligned
int check_monitor_state(Handle* h, const urgym_monitor_state* state, const char* who) {
  if (!state) return fail_in(h, URGYM_ERR_ARG, who, "null monitor state");
  const urgym_monitor_state& m = *state;
  const LearnerPointer required[] = {{"running_return", m.running_return}, {"running_length", m.running_length}, {"sum_return", m.sum_return},
                                     {"sum_length", m.sum_length},         {"episodes", m.episodes},             {"successes", m.successes}};
  for (const LearnerPointer& r : required)
    if (!r.p) return failf(h, URGYM_ERR_ARG, "%s: urgym_monitor_state.%s is null", who, r.name);
  if ((uintptr_t)m.running_return % 8 != 0 || (uintptr_t)m.sum_return % 8 != 0 || (uintptr_t)m.sum_length % 8 != 0)
    return fail_in(h, URGYM_ERR_ARG, who, "running_return, sum_return and sum_length must be 8-byte aligned");
  return URGYM_OK;
}

int check_monitor_fold(Handle* h, const urgym_monitor_state* state, const urgym_replay_ring* ring, int first_slot, int num_steps, const char* who, MonitorFoldCall* out) {
  if (int rc = check_monitor_state(h, state, who)) return rc;
  if (int rc = check_fold_ring(h, ring, first_slot, num_steps, who)) return rc;
  *out = MonitorFoldCall{h->cfg.num_envs, ring->capacity_steps, first_slot, num_steps, *state, ring->reward, ring->terminated, ring->truncated, ring->is_success};
  return URGYM_OK;
}

int check_monitor_stats(Handle* h, const urgym_monitor_state* state, urgym_monitor_record* record, int64_t iteration, int clear, const char* who, MonitorStatsCall* out) {
  static_assert(sizeof(urgym_monitor_record) == 72 && alignof(urgym_monitor_record) == 8, "include/urgym.h");
  if (int rc = check_monitor_state(h, state, who)) return rc;
  if (!record) return fail_in(h, URGYM_ERR_ARG, who, "null record");
  if ((uintptr_t)record % 8 != 0) return fail_in(h, URGYM_ERR_ARG, who, "record must be 8-byte aligned");
  *out = MonitorStatsCall{h->cfg.num_envs, clear, iteration, *state, record};
  return URGYM_OK;
}

}  // namespace

extern "C" {

int urgym_eval_stats(void* handle, const urgym_eval_stats_args* args, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  EvalStatsCall c;
  if (int rc = check_eval_stats(h, args, "urgym_eval_stats", &c)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  eval_stats_launch(c, (hipStream_t)stream);
  return launched(h);
}

int urgym_actor_snapshot(void* handle, const urgym_actor_snapshot_args* args, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  ActorSnapshotCall c;
  if (int rc = check_actor_snapshot(h, args, "urgym_actor_snapshot", &c)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  actor_snapshot_launch(c, (hipStream_t)stream);
  return launched(h);
}

int urgym_policy_evaluate(void* eval_handle, const urgym_policy_evaluation* evaluation, int64_t eval_index, int32_t record_slot, void* stream) {
  const char* who = "urgym_policy_evaluate";
  Handle* eh = (Handle*)eval_handle;
  if (!eh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  PolicyEvaluation c;
  if (int rc = check_policy_evaluation(eh, eh, evaluation, who, &c)) return rc;
  if (int rc = check_evaluation_slot(eh, *evaluation, eval_index, record_slot, who)) return rc;
  return launch_policy_evaluation(c, eval_index, record_slot, (hipStream_t)stream);
}

int urgym_monitor_fold(void* handle, const urgym_monitor_state* state, const urgym_replay_ring* ring, int first_slot, int num_steps, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  MonitorFoldCall c;
  if (int rc = check_monitor_fold(h, state, ring, first_slot, num_steps, "urgym_monitor_fold", &c)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  monitor_fold_launch(c, (hipStream_t)stream);
  return launched(h);
}

int urgym_monitor_stats(void* handle, const urgym_monitor_state* state, urgym_monitor_record* record, int64_t iteration, int clear, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  MonitorStatsCall c;
  if (int rc = check_monitor_stats(h, state, record, iteration, clear, "urgym_monitor_stats", &c)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  monitor_stats_launch(c, (hipStream_t)stream);
  return launched(h);
}

int urgym_norm_snapshot(void* handle, const urgym_norm_state* source, const urgym_norm_state* destination, const int32_t* when, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  NormSnapshotCall c;
  if (int rc = check_norm_snapshot(h, source, destination, when, "urgym_norm_snapshot", &c)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  norm_snapshot_launch(c, (hipStream_t)stream);
  return launched(h);
}

int urgym_policy_evaluate_normalized(void* eval_handle, const urgym_policy_evaluation* evaluation, const urgym_normalization* normalization, int64_t eval_index, int32_t record_slot, void* stream) {
  const char* who = "urgym_policy_evaluate_normalized";
  Handle* eh = (Handle*)eval_handle;
  if (!eh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  PolicyEvaluation c;
  if (int rc = check_policy_evaluation(eh, eh, evaluation, who, &c)) return rc;
  if (int rc = check_evaluation_slot(eh, *evaluation, eval_index, record_slot, who)) return rc;
  if (int rc = check_evaluation_normalization(eh, eh, normalization, who, &c)) return rc;
  return launch_policy_evaluation(c, eval_index, record_slot, (hipStream_t)stream);
}

int urgym_norm_workspace(void* handle, int num_steps, uint64_t* bytes) {
  const char* who = "urgym_norm_workspace";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!bytes) return fail_in(h, URGYM_ERR_ARG, who, "null bytes");
  if (num_steps <= 0) return fail_in(h, URGYM_ERR_ARG, who, "num_steps must be positive");
  *bytes = norm_workspace_doubles(h->cfg.num_envs, actor_features(h), num_steps) * sizeof(double);
  return URGYM_OK;
}

int urgym_norm_fold(void* handle, const urgym_normalization* norm, const urgym_replay_ring* ring, int first_slot, int num_steps, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  NormFoldCall c;
  if (int rc = check_norm_fold(h, norm, ring, first_slot, num_steps, "urgym_norm_fold", &c)) return rc;
  if (norm->training == 0) return URGYM_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  norm_fold_launch(c, (hipStream_t)stream);
  return launched(h);
}

int urgym_norm_rows(void* handle, const urgym_normalization* norm, const urgym_norm_rows_args* rows, int count, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  NormApplyCall c;
  if (int rc = check_norm_rows(h, norm, rows, count, "urgym_norm_rows", &c)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  norm_apply_launch(c, (hipStream_t)stream);
  return launched(h);
}

int urgym_norm_batch(void* handle, const urgym_normalization* norm, const urgym_replay_batch* batch, int count, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  NormApplyCall c;
  if (int rc = check_norm_batch(h, norm, batch, count, "urgym_norm_batch", &c)) return rc;
  if (c.segments == 0) return URGYM_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  norm_apply_launch(c, (hipStream_t)stream);
  return launched(h);
}

int urgym_rollout_collect_normalized(void* handle, void* actor, const urgym_sampling* how, int num_steps, const urgym_replay_ring* ring, int first_slot, const urgym_normalization* norm, void* stream) {
  const char* who = "urgym_rollout_collect_normalized";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  Actor* a = nullptr;
  if (int rc = check_collect(h, actor, how, num_steps, ring, first_slot, who, &a)) return rc;
  if (int rc = check_normalization(h, norm, who)) return rc;
  if (norm->norm_obs == 0) return rollout(h, a, how, num_steps, RolloutSinks{nullptr, nullptr, ring, first_slot}, (hipStream_t)stream);
  if (!norm->scratch) return fail_in(h, URGYM_ERR_ARG, who, "urgym_normalization.scratch is null");
  const size_t n = (size_t)h->cfg.num_envs;
  float* const obs = norm->scratch;
  float* const ach = obs + n * (size_t)h->obs_dim;
  float* const des = ach + n * (size_t)h->goal_dim;
  const urgym_norm_rows_args rows{h->buf.observation, h->buf.achieved_goal, h->buf.desired_goal, obs, ach, des};
  NormApplyCall c;
  if (int rc = check_norm_rows(h, norm, &rows, h->cfg.num_envs, who, &c)) return rc;
  return rollout(h, a, how, num_steps, RolloutSinks{nullptr, nullptr, ring, first_slot}, (hipStream_t)stream, &c);
}

}  // extern "C"

// ---- the training loop in one call (include/urgym.h, urgym_sac_train): every check above first, then nothing
// but launches.  The launch structs are filled once; an update rewrites the few numbers that move (draws, the ring view, Adam's
// coefficients, the loss slots).

namespace {

// after the launches of one stage: urgym_last_error names the iteration and the stage
int train_stage(Handle* h, const char* who, int iteration, const char* stage) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return URGYM_OK;
  return failf(h, URGYM_ERR_HIP, "%s: iteration %d, %s: %s", who, iteration, stage, hipGetErrorString(e));
}

// What one training call takes beyond the learner and the schedule: the option structs of the entry points, null = absent.
struct TrainOptions {
  const urgym_sac_nstep* nstep;            // the update whose gather, third call and entropy step are the multi-step ones
  const urgym_sac_prioritized* per;        // urgym_per_fill after every collection, the gather through the priorities, urgym_per_terms
  const urgym_sac_hindsight* her;          // the update whose gather is urgym_replay_sample_hindsight
  const urgym_sac_clipping* clip;          // the update with the two norm launches and the scaled steps
  const urgym_normalization* norm;         // the actor reads normalized rows, one fold after every collection, one urgym_norm_batch after every gather
  const urgym_sac_evaluation* evaluation;  // TrainExtras
  const urgym_sac_monitoring* monitoring;  // TrainExtras
  const urgym_sac_planning* planning;      // the collection is the planner's (urgym_mppi_train.h), planner_sync after the updates, TrainExtras
  const urgym_mppi_temper* temper;         // with planning: the planner's update is the tempered one (urgym_sac_train_tempered)
  const urgym_mppi_noise* noise;           // with planning: the planner's sample is the coloured one (urgym_sac_train_colored)
  const urgym_sac_cloning* cloning;        // the update whose policy terms are urgym_sac_policy_terms_cloned's (urgym_sac_train_cloned)
  const urgym_sac_demonstrating* demonstrating;  // the update whose gather is urgym_replay_sample_mixed's; with cloning and
                                                 // clone_demonstrations_only its policy terms are the masked ones (urgym_sac_train_demonstrated)
  const urgym_sac_weighting* weighting;    // with cloning: the policy terms are urgym_sac_policy_terms_weighted's (urgym_sac_train_weighted)
};

// The evaluations and the training-episode statistics of one training call: what the body runs beside its own checks and launches.
// check() runs after every check of the body (so the learner and the schedule are sound) and before its first launch: a refusal leaves
// nothing launched.  after(i) runs after the launches of iteration i.  The monitor's half goes first in both; with neither option given
// both do nothing.
struct TrainExtras {
  const char* who;  // the entry point that runs them
  Handle* h;
  const urgym_sac_learner* learner;
  const urgym_sac_schedule* schedule;
  hipStream_t s;
  const urgym_sac_evaluation* evaluation;
  const urgym_sac_monitoring* monitoring;
  const urgym_normalization* norm;  // given: the evaluations are urgym_policy_evaluate_normalized's
  const PlannedCall* planned;       // given: the collection is the planner's; with records, a plan-statistics record beside every monitor record
  PolicyEvaluation eval_call;
  int64_t evals_done;      // evaluations launched so far
  MonitorFoldCall fold;    // first_slot moves per iteration
  MonitorStatsCall stats;  // record and iteration move per record
  int64_t records_done;    // records launched so far

  int check_monitoring() {
    const urgym_sac_monitoring& M = *monitoring;
    const urgym_sac_schedule& S = *schedule;
    if (M.reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_monitoring.reserved0 must be 0");
    if (const char* what = monitor_schedule_refusal(S, M.log_every, M.first_iteration, M.first_record, M.record_capacity)) return fail_in(h, URGYM_ERR_ARG, who, what);
    // the fold's checks with the first iteration's slots (a call that collects nothing folds nothing: its state is still checked below)
    if (S.steps_per_iteration > 0)
      if (int rc = check_monitor_fold(h, &M.state, &learner->ring, S.first_slot, S.steps_per_iteration, who, &fold)) return rc;
    // the statistics' checks, on the first record (every record has its alignment: it is a multiple of 8 bytes); without a record point
    // the pointer may be anything
    const bool records = monitor_record_count(M.first_iteration, M.log_every, S.num_iterations) > 0;
    urgym_monitor_record unused;
    return check_monitor_stats(h, &M.state, records ? M.records : &unused, 0, M.clear, who, &stats);
  }

  int check_evaluation() {
    const urgym_sac_evaluation& E = *evaluation;
    Handle* eh = (Handle*)E.eval_handle;
    if (!eh) return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_evaluation.eval_handle is null");
    if (eh == h) return fail_in(h, URGYM_ERR_ARG, who, "eval_handle is the training handle (an evaluation would reset the training env; evaluation on it is not supported)");
    if (eh->device != h->device) return fail_in(h, URGYM_ERR_ARG, who, "the training handle and the evaluation handle are on different devices");
    if (int rc = check_policy_evaluation(h, eh, &E.evaluation, who, &eval_call)) return rc;
    if (norm)
      if (int rc = check_evaluation_normalization(h, eh, norm, who, &eval_call)) return rc;
    const urgym_actor_tensors& p = learner->actor_adam.param;
    const float* const params[PACK_ACTOR_TENSORS] = {p.w0, p.b0, p.w1, p.b1, p.w_mu, p.b_mu, p.w_log_std, p.b_log_std};
    for (int i = 0; i < PACK_ACTOR_TENSORS; i++)
      if (eval_call.src[i] != params[i]) return fail_in(h, URGYM_ERR_ARG, who, "the evaluation's source tensors are not learner->actor_adam.param");
    if (learner->actor_adam.in_features != E.evaluation.in_features || learner->actor_adam.hidden_width != E.evaluation.hidden_width)
      return fail_in(h, URGYM_ERR_ARG, who, "the evaluation's shape is not learner->actor_adam's");
    if (const char* what = eval_schedule_refusal(*schedule, E.every, E.first_eval_index, E.first_record_slot, E.evaluation.record_capacity))
      return fail_in(h, URGYM_ERR_ARG, who, what);
    return URGYM_OK;
  }

  // what urgym_sac_train_planned refuses about the planning beside the two options
  int check_planning() {
    if (evaluation && evaluation->eval_handle == (void*)planned->planner) return fail_in(h, URGYM_ERR_ARG, who, "planner_handle is the evaluation's eval_handle");
    if (!planned->records) return URGYM_OK;
    if (!monitoring) return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_planning.records is given without monitoring (a plan-statistics record goes beside a monitor record)");
    const urgym_sac_monitoring& M = *monitoring;
    if (M.log_every < 1 || M.first_iteration < 0 || M.first_record < 0) return URGYM_OK;  // check_monitoring refuses it
    if (monitor_record_count(M.first_iteration, M.log_every, schedule->num_iterations) > (int64_t)planned->record_capacity - M.first_record)
      return fail_in(h, URGYM_ERR_ARG, who, "first_record + the records of the call is beyond urgym_sac_planning.record_capacity");
    return URGYM_OK;
  }

  int check() {
    if (planned)
      if (int rc = check_planning()) return rc;
    if (monitoring)
      if (int rc = check_monitoring()) return rc;
    return evaluation ? check_evaluation() : URGYM_OK;
  }

  int after(int i) {
    if (monitoring) {
      const urgym_sac_monitoring& M = *monitoring;
      if (schedule->steps_per_iteration > 0) {
        fold.first_slot = sac_schedule_iteration(*schedule, i).collect_first_slot;
        monitor_fold_launch(fold, s);
        if (int rc = train_stage(h, who, i, "monitor_fold")) return rc;
      }
      if (monitor_record_follows(M.first_iteration, M.log_every, i)) {
        stats.record = M.records + M.first_record + records_done;
        stats.iteration = M.first_iteration + i + 1;
        records_done++;
        monitor_stats_launch(stats, s);
        if (int rc = train_stage(h, who, i, "monitor_stats")) return rc;
        if (planned && planned->records) {  // planner record r beside monitor record r
          planned_stats(*planned, planned->records + M.first_record + (records_done - 1), stats.iteration, s);
          if (int rc = train_stage(h, who, i, "mppi_stats")) return rc;
        }
      }
    }
    if (!evaluation || !eval_follows(*schedule, evaluation->every, i)) return URGYM_OK;
    const int rc = launch_policy_evaluation(eval_call, evaluation->first_eval_index + evals_done, (int32_t)(evaluation->first_record_slot + evals_done), s);
    evals_done++;
    if (rc) return failf(h, rc, "%s: iteration %d, evaluation: %.150s", who, i, eval_call.eh->err);
    HIP_TRY(h, hipSetDevice(h->device));  // the same device: what the launches of the next iteration expect to be current
    return URGYM_OK;
  }
};

// The one driver of the fourteen urgym_sac_train* entry points: `who` is the entry point's own name in every refusal, `opt` what it was given.
int sac_train_body(const char* who, Handle* h, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, hipStream_t s, const TrainOptions& opt) {
  if (!learner) return fail_in(h, URGYM_ERR_ARG, who, "null learner");
  if (!schedule) return fail_in(h, URGYM_ERR_ARG, who, "null schedule");
  const urgym_sac_nstep* const nstep = opt.nstep;
  const urgym_sac_prioritized* const per = opt.per;
  const urgym_sac_hindsight* const her = opt.her;
  const urgym_sac_clipping* const clip = opt.clip;
  const urgym_normalization* const norm = opt.norm;
  const urgym_sac_planning* const planning = opt.planning;
  const urgym_sac_cloning* const cloning = opt.cloning;
  const urgym_sac_demonstrating* const demonstrating = opt.demonstrating;
  const urgym_sac_weighting* const weighting = opt.weighting;
  PlannedCall planned;
  TrainExtras extras{who, h, learner, schedule, s, opt.evaluation, opt.monitoring, norm, planning ? &planned : nullptr};
  const urgym_sac_learner& L = *learner;
  const urgym_sac_schedule& S = *schedule;
  if (L.reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_learner.reserved0 must be 0");
  const LearnerPointer required[] = {
      {"actor", L.actor}, {"online", L.online}, {"target", L.target}, {"actor_workspace", L.actor_workspace},
      {"critic_workspace", L.critic_workspace}, {"log_ent_coef", L.log_ent_coef}, {"exp_avg", L.exp_avg}, {"exp_avg_sq", L.exp_avg_sq},
      {"batch.observation", L.batch.observation}, {"batch.achieved_goal", L.batch.achieved_goal}, {"batch.desired_goal", L.batch.desired_goal},
      {"batch.action", L.batch.action}, {"batch.reward", L.batch.reward}, {"batch.next_observation", L.batch.next_observation},
      {"batch.next_achieved_goal", L.batch.next_achieved_goal}, {"batch.next_desired_goal", L.batch.next_desired_goal},
      {"batch.terminated", L.batch.terminated}, {"next_actions", L.next_actions}, {"next_log_prob", L.next_log_prob},
      {"target_value", L.target_value}, {"y", L.y}, {"action_pi", L.action_pi}, {"log_prob", L.log_prob}, {"q", L.q}, {"q_min", L.q_min},
      {"dqmin_da", L.dqmin_da}, {"d_action", L.d_action}, {"d_log_prob", L.d_log_prob}, {"ent_coef", L.ent_coef}};
  const LearnerPointer losses[] = {{"critic_loss", L.critic_loss}, {"actor_loss", L.actor_loss}, {"ent_coef_loss", L.ent_coef_loss}};
  for (const LearnerPointer& r : required)
    if (!r.p) return failf(h, URGYM_ERR_ARG, "%s: urgym_sac_learner.%s is null", who, r.name);
  if (L.online == L.target) return fail_in(h, URGYM_ERR_ARG, who, "the target is the online critic itself");
  if (const char* what = sac_schedule_refusal(S)) return fail_in(h, URGYM_ERR_ARG, who, what);
  if (S.capacity_steps != L.ring.capacity_steps) return fail_in(h, URGYM_ERR_ARG, who, "schedule->capacity_steps is not ring.capacity_steps");
  for (const LearnerPointer& r : losses)  // zero slots need no array
    if (!r.p && sac_schedule_updates(S) > 0) return failf(h, URGYM_ERR_ARG, "%s: urgym_sac_learner.%s is null", who, r.name);
  if (nstep) {  // the window's own refusals, whether or not the call holds an update
    if (nstep->n_steps < 2 || nstep->n_steps > NSTEP_MAX)
      return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_nstep.n_steps must be in [2, URGYM_REPLAY_NSTEP_MAX] (n_steps == 1 is urgym_sac_train and its kin)");
    if (nstep->reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_nstep.reserved0 must be 0");
    if (!nstep->discount || !nstep->q_min_next) return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_nstep.discount or q_min_next is null");
    if (!L.ring.truncated) return fail_in(h, URGYM_ERR_ARG, who, "the ring keeps no truncated (an episode's end at the time limit could not be seen)");
  }
  ReplayGatherHindsight gather_her;
  urgym_replay_hindsight her_rule;
  memset(&her_rule, 0, sizeof(her_rule));
  if (her) {  // the rule's own refusals, whether or not the call holds an update: the gather's checks on the ring as it stands
    if (her->strategy == HER_GOAL_OWN) return fail_in(h, URGYM_ERR_ARG, who, "URGYM_HER_GOAL_OWN is a diagnostic of the gather, not a way to train");
    if (her->reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_hindsight.reserved0 must be 0");
    her_rule.relabel_threshold = her->relabel_threshold, her_rule.strategy = her->strategy, her_rule.horizon = her->horizon;
    if (L.count <= 0) return fail_in(h, URGYM_ERR_ARG, who, "count must be positive");
    if (int rc = check_replay_sample_hindsight(h, &L.ring, 0, 1, L.update_seed, 0, L.count, &L.batch, &her_rule, who, &gather_her)) return rc;
  }
  PerFill per_fill;
  memset(&per_fill, 0, sizeof(per_fill));
  if (per) {  // the structure's own refusals, whether or not the call holds an update
    if (per->reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_prioritized.reserved0 must be 0");
    if (int rc = check_priorities(h, &per->priorities, who, &per_fill.tree)) return rc;
    if (per->priorities.capacity_steps != L.ring.capacity_steps) return fail_in(h, URGYM_ERR_ARG, who, "priorities.capacity_steps is not ring.capacity_steps");
    if (!(per->beta0 >= 0.0 && per->beta0 <= 1.0)) return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_prioritized.beta0 must be in [0, 1]");
    if (per->beta_steps < 1) return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_prioritized.beta_steps must be positive");
    if (!(per->alpha >= 0.0f && per->alpha <= 1.0f)) return fail_in(h, URGYM_ERR_ARG, who, "alpha must be in [0, 1]");
    if (!(per->eps > 0.0f && per->eps < INFINITY)) return fail_in(h, URGYM_ERR_ARG, who, "eps must be positive and finite");
    if (!per->leaf || !per->total || !per->q || !per->w_raw || !per->w || !per->dq || !per->new_leaf)
      return fail_in(h, URGYM_ERR_ARG, who, "a scratch pointer of urgym_sac_prioritized is null (leaf, total, q, w_raw, w, dq, new_leaf)");
  }
  if (clip) {  // the option's own refusals, whether or not the call holds an update
    if (clip->reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_clipping.reserved0 must be 0");
    if (!(clip->max_grad_norm > 0.0f && clip->max_grad_norm < INFINITY)) return fail_in(h, URGYM_ERR_ARG, who, "max_grad_norm must be finite and positive");
    if (!clip->scale) return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_clipping.scale is null");
    if ((!clip->critic_grad_norm || !clip->actor_grad_norm) && sac_schedule_updates(S) > 0)  // zero slots need no array
      return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_clipping.critic_grad_norm or actor_grad_norm is null");
  }
  if (cloning) {  // the option's own refusals, whether or not the call holds an update
    if (const char* what = clone_option_refusal(cloning->weight, cloning->scale_by_q, cloning->q_filter, cloning->reserved0)) return fail_in(h, URGYM_ERR_ARG, who, what);
    if ((!cloning->bc_loss || !cloning->bc_weight || !cloning->bc_rows) && sac_schedule_updates(S) > 0)  // zero slots need no array
      return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_cloning.bc_loss, bc_weight or bc_rows is null");
  }
  if (weighting) {  // the option's own refusals, whether or not the call holds an update
    if (!cloning) return fail_in(h, URGYM_ERR_ARG, who, "weighting needs cloning");
    if (const char* what = weight_option_refusal(weighting->temperature, weighting->max_weight, weighting->reserved0, cloning->q_filter)) return fail_in(h, URGYM_ERR_ARG, who, what);
    if ((!weighting->adv_ess || !weighting->adv_max || !weighting->adv_clipped) && sac_schedule_updates(S) > 0)  // zero slots need no array
      return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_weighting.adv_ess, adv_max or adv_clipped is null");
  }
  ReplayGatherMixed gather_mixed;
  if (demonstrating) {  // the option's own refusals, whether or not the call holds an update: the gather's checks on the ring as it stands
    const urgym_sac_demonstrating& dm = *demonstrating;
    if (dm.reserved0 != 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_demonstrating.reserved0 must be 0");
    if (dm.clone_demonstrations_only != 0 && dm.clone_demonstrations_only != 1) return fail_in(h, URGYM_ERR_ARG, who, "clone_demonstrations_only must be 0 or 1");
    if (dm.clone_demonstrations_only != 0 && !cloning) return fail_in(h, URGYM_ERR_ARG, who, "clone_demonstrations_only needs cloning");
    if (L.count <= 0) return fail_in(h, URGYM_ERR_ARG, who, "count must be positive");
    if (dm.demonstrations.count > L.count) return fail_in(h, URGYM_ERR_ARG, who, "demonstrations.count is above the learner's count (D > M)");
    if (int rc = check_replay_sample_mixed(h, &L.ring, 0, 1, L.update_seed, 0, L.count, &L.batch, &dm.demonstrations, dm.source, who, &gather_mixed)) return rc;
    if (!dm.source && sac_schedule_updates(S) > 0) return fail_in(h, URGYM_ERR_ARG, who, "urgym_sac_demonstrating.source is null");
  }
  if (planning) {  // the planner's own refusals and the collection's, whether or not the call holds an update
    if (int rc = planned_check(who, h, planning, &L.ring, S, &planned, opt.temper, opt.noise)) return rc;
    if (planning->sync != 0) {  // planner_sync reloads the guide's actor and critic from the learner's tensors
      if (planned.sync_actor) {
        const ActorPacked buf = actor_packed(planned.sync_actor);
        if (buf.in_features != L.actor_adam.in_features || buf.hidden != L.actor_adam.hidden_width)
          return failf(h, URGYM_ERR_ARG, "%s: sync: learner->actor_adam is %d -> %d, the guide's actor is %d -> %d", who, L.actor_adam.in_features,
                       L.actor_adam.hidden_width, buf.in_features, buf.hidden);
      }
      if (planned.sync_critic) {
        const CriticPacked buf = critic_packed(planned.sync_critic);
        if (buf.in_features != L.critic_adam.in_features || buf.hidden != L.critic_adam.hidden_width)
          return failf(h, URGYM_ERR_ARG, "%s: sync: learner->critic_adam is %d -> %d, the guide's critic is %d -> %d", who, L.critic_adam.in_features,
                       L.critic_adam.hidden_width, buf.in_features, buf.hidden);
      }
    }
  }

  // ---- the checking halves, with the numbers of the first collection and the first update
  const int M = L.count, K = S.steps_per_iteration, G = S.updates_per_iteration;
  NormFoldCall norm_fold;
  NormApplyCall norm_collect, norm_batch;
  memset(&norm_batch, 0, sizeof(norm_batch));
  if (norm) {  // the option's own refusals, whether or not the call holds an update
    if (int rc = check_normalization(h, norm, who)) return rc;
    if (K > 0) {
      if (int rc = check_norm_fold(h, norm, &L.ring, S.first_slot, K, who, &norm_fold)) return rc;
      if (norm->norm_obs != 0) {
        if (!norm->scratch) return fail_in(h, URGYM_ERR_ARG, who, "urgym_normalization.scratch is null");
        const size_t n = (size_t)h->cfg.num_envs;
        float* const ach = norm->scratch + n * (size_t)h->obs_dim;
        const urgym_norm_rows_args rows{h->buf.observation, h->buf.achieved_goal, h->buf.desired_goal, norm->scratch, ach, ach + n * (size_t)h->goal_dim};
        if (int rc = check_norm_rows(h, norm, &rows, h->cfg.num_envs, who, &norm_collect)) return rc;
      }
    }
    if (M <= 0) return fail_in(h, URGYM_ERR_ARG, who, "count must be positive");
    if (int rc = check_norm_batch(h, norm, &L.batch, M, who, &norm_batch)) return rc;
  }
  const bool normalized_rows = norm && K > 0 && norm->norm_obs != 0, folds = norm && K > 0 && norm->training != 0;
  const int64_t updates = sac_schedule_updates(S);
  const float scale = (float)(1.0 / (double)M), neg_scale = (float)(-1.0 / (double)M);  // as SACLearner._update_on_device hands them over
  Actor* collector = nullptr;
  if (K > 0 && !planning) {
    for (int mode : {URGYM_SAMPLE_UNIFORM, URGYM_SAMPLE_GAUSSIAN}) {  // each mode the call collects with
      if (mode == URGYM_SAMPLE_UNIFORM ? S.uniform_iterations == 0 : S.uniform_iterations >= S.num_iterations) continue;
      const urgym_sampling how{mode, 0, L.seed, S.collect_first_draw};
      if (int rc = check_collect(h, L.actor, &how, K, &L.ring, S.first_slot, who, &collector)) return rc;
    }
  }
  // the collection of iteration i: the launches of urgym_rollout_collect, or with a planner those of urgym_mppi_collect(_adaptive)
  auto collect = [&](int i, const SacIteration& it) {
    const urgym_sampling how{it.collect_mode, 0, L.seed, it.collect_first_draw};
    const int rc = planning ? planned_collect(planned, it.collect_first_draw, K, it.collect_first_slot, s)
                            : rollout(h, collector, &how, K, RolloutSinks{nullptr, nullptr, &L.ring, it.collect_first_slot}, s, normalized_rows ? &norm_collect : nullptr);
    if (!rc && folds) {  // urgym_norm_fold on the slots just written
      norm_fold.first_slot = it.collect_first_slot;
      norm_fold_launch(norm_fold, s);
      if (int stage = train_stage(h, who, i, "norm_fold")) return stage;
    }
    if (!rc && per) {  // urgym_per_fill on the slots just written
      per_fill_ranges(per_fill, it.collect_first_slot, K);
      per_fill_launch(per_fill, s);
      return train_stage(h, who, i, "per_fill");
    }
    if (!rc) return rc;
    char was[160];
    snprintf(was, sizeof(was), "%s", h->err);
    return failf(h, rc, "%s: iteration %d, collect: %s", who, i, was);
  };
  if (updates == 0) {  // the sequence holds no update call: nothing more to check
    if (int rc = extras.check()) return rc;
    for (int i = 0; i < S.num_iterations; i++) {
      if (int rc = collect(i, sac_schedule_iteration(S, i))) return rc;
      if (int rc = extras.after(i)) return rc;
    }
    return URGYM_OK;
  }
  const SacIteration view = sac_schedule_iteration(S, S.idle_iterations);  // what the first update sees
  const SacUpdate first = sac_schedule_update(S, 0);
  urgym_adam_hyper hp{L.lr, L.beta1, L.beta2, L.eps, first.adam_step, 0};

  ReplayGatherNstep gather_nstep;
  ReplayGather& gather = gather_nstep.g;
  if (nstep) {
    const urgym_replay_nstep window{nstep->n_steps, 0, L.gamma, 0.0f, nstep->discount, nullptr, nullptr};
    if (int rc = check_replay_sample_nstep(h, &L.ring, view.oldest_slot, view.filled_steps, L.update_seed, first.gather_draw, M, &L.batch, &window, who, &gather_nstep))
      return rc;
  } else if (int rc = check_replay_sample(h, &L.ring, view.oldest_slot, view.filled_steps, L.update_seed, first.gather_draw, M, &L.batch, who, &gather)) {
    return rc;
  }
  if (her)
    if (int rc = check_replay_sample_hindsight(h, &L.ring, view.oldest_slot, view.filled_steps, L.update_seed, first.gather_draw, M, &L.batch, &her_rule, who, &gather_her))
      return rc;
  if (demonstrating)
    if (int rc = check_replay_sample_mixed(h, &L.ring, view.oldest_slot, view.filled_steps, L.update_seed, first.gather_draw, M, &L.batch,
                                           &demonstrating->demonstrations, demonstrating->source, who, &gather_mixed))
      return rc;
  PerGather per_gather;
  memset(&per_gather, 0, sizeof(per_gather));
  if (per) {  // urgym_replay_sample_prioritized
    if (int rc = check_replay_sample(h, &L.ring, 0, L.ring.capacity_steps, L.update_seed, first.gather_draw, M, &L.batch, who, &per_gather.g)) return rc;
    if (!L.batch.index) return fail_in(h, URGYM_ERR_ARG, who, "batch.index is required with priorities");
    per_gather.tree = per_fill.tree, per_gather.leaf_out = per->leaf, per_gather.total_out = per->total;
  }
  const urgym_critic_rows next_rows{L.batch.next_observation, L.batch.next_achieved_goal, L.batch.next_desired_goal, L.next_actions};
  const urgym_critic_rows batch_rows{L.batch.observation, L.batch.achieved_goal, L.batch.desired_goal, L.batch.action};
  const urgym_critic_rows policy_rows{L.batch.observation, L.batch.achieved_goal, L.batch.desired_goal, L.action_pi};
  urgym_sampling how{URGYM_SAMPLE_GAUSSIAN, 0, L.update_seed, first.gather_draw};
  SampleRows next_sample, policy_sample;
  if (int rc = check_sample_rows(h, L.actor, &how, &next_rows, M, L.next_actions, L.next_log_prob, who, &next_sample)) return rc;
  const urgym_critic_terms terms{L.batch.reward, L.batch.terminated, L.next_log_prob, L.gamma, 0.0f};
  const urgym_critic_out target_out{nullptr, nstep ? nstep->q_min_next : nullptr, nstep ? nullptr : L.target_value};
  Critic *target = nullptr, *online = nullptr, *online_grad = nullptr;
  CriticCall bootstrap;
  if (int rc = check_critic_evaluate(h, L.target, &next_rows, M, nstep ? nullptr : &terms, &target_out, who, &target, &bootstrap)) return rc;
  how.first_draw = first.policy_draw;
  if (int rc = check_sample_rows(h, L.actor, &how, &batch_rows, M, L.action_pi, L.log_prob, who, &policy_sample)) return rc;
  urgym_sac_entropy_args ea;
  memset(&ea, 0, sizeof(ea));
  ea.count = M, ea.target_entropy = L.target_entropy, ea.gamma = L.gamma, ea.scale = scale;
  ea.log_prob = L.log_prob, ea.log_ent_coef = L.log_ent_coef, ea.exp_avg = L.exp_avg, ea.exp_avg_sq = L.exp_avg_sq;
  ea.ent_coef_out = L.ent_coef, ea.loss_out = L.ent_coef_loss;
  ea.target_in = L.target_value, ea.next_log_prob = L.next_log_prob, ea.terminated = L.batch.terminated, ea.y_out = L.y;
  ea.d_log_prob_out = L.d_log_prob;
  SacEntropyCall entropy;
  SacEntropyNstepCall entropy_nstep;
  if (nstep) {
    urgym_sac_entropy_nstep_args na;
    memset(&na, 0, sizeof(na));
    na.count = M, na.target_entropy = L.target_entropy, na.scale = scale;
    na.log_prob = L.log_prob, na.log_ent_coef = L.log_ent_coef, na.exp_avg = L.exp_avg, na.exp_avg_sq = L.exp_avg_sq;
    na.ent_coef_out = L.ent_coef, na.loss_out = L.ent_coef_loss;
    na.reward = L.batch.reward, na.q_min_next = nstep->q_min_next, na.discount = nstep->discount, na.next_log_prob = L.next_log_prob;
    na.terminated = L.batch.terminated, na.y_out = L.y, na.d_log_prob_out = L.d_log_prob;
    if (int rc = check_entropy_step_nstep(h, &na, &hp, who, &entropy_nstep)) return rc;
  } else if (int rc = check_entropy_step(h, &ea, &hp, who, &entropy)) {
    return rc;
  }
  urgym_critic_param_grads cg;
  for (int net = 0; net < 2; net++) {
    const urgym_q_network_dev& g = L.critic_adam.grad[net];  // the tensors the step reads are the ones the gradient call writes
    cg.qf[net] = urgym_q_network_grad{(float*)g.w0, (float*)g.b0, (float*)g.w1, (float*)g.b1, (float*)g.w_q, (float*)g.b_q};
  }
  cg.q = L.q;
  // with priorities: the online critics' q on the batch rows, then urgym_per_terms, and the gradients take its dq
  Critic* online_q = nullptr;
  CriticCall evaluate_q;
  PerTermsCall per_terms;
  if (per) {
    const urgym_critic_out q_out{per->q, nullptr, nullptr};
    if (int rc = check_critic_evaluate(h, L.online, &batch_rows, M, nullptr, &q_out, who, &online_q, &evaluate_q)) return rc;
    urgym_per_terms_args ta;
    memset(&ta, 0, sizeof(ta));
    ta.count = M, ta.size = (float)((uint64_t)view.filled_steps * (uint64_t)h->cfg.num_envs), ta.beta = per_beta(per->beta0, first.adam_step, per->beta_steps);
    ta.alpha = per->alpha, ta.eps = per->eps, ta.scale = scale;
    ta.leaf_in = per->leaf, ta.total = per->total, ta.q = per->q, ta.y = L.y, ta.w_raw = per->w_raw, ta.w = per->w, ta.dq = per->dq;
    ta.index = L.batch.index, ta.new_leaf = per->new_leaf, ta.priorities = per->priorities;
    if (int rc = check_per_terms(h, &ta, who, &per_terms)) return rc;
  }
  CriticBackwardCall critic_backward;
  if (int rc = check_critic_parameter_gradients(h, L.online, &batch_rows, M, per ? per->dq : nullptr, per ? nullptr : L.y, scale, &cg, L.critic_workspace,
                                                L.critic_workspace_bytes, who, &online, &critic_backward))
    return rc;
  CriticAdamStep critic_step;
  if (int rc = check_critic_adam(h, L.online, L.target, &L.critic_adam, &hp, L.tau, who, &critic_step)) return rc;
  GradNormCall critic_norm, actor_norm;
  if (clip) {
    const urgym_grad_norm na{clip->max_grad_norm, 0, clip->critic_grad_norm, clip->scale, nullptr};
    if (int rc = check_critic_grad_norm(h, L.online, L.critic_adam.grad, &na, who, &critic_norm)) return rc;
  }
  const urgym_critic_grad_out go{nullptr, L.dqmin_da, nullptr, L.q_min};
  CriticGradCall action_gradient;
  if (int rc = check_critic_action_gradient(h, L.online, &policy_rows, M, &go, who, &online_grad, &action_gradient)) return rc;
  urgym_sac_policy_args pa;
  memset(&pa, 0, sizeof(pa));
  pa.count = M, pa.scale = neg_scale, pa.ent_coef = L.ent_coef;
  pa.dqmin_da = L.dqmin_da, pa.d_action_out = L.d_action;
  pa.q = L.q, pa.y = L.y, pa.critic_loss_out = L.critic_loss;
  pa.log_prob = L.log_prob, pa.q_min = L.q_min, pa.actor_loss_out = L.actor_loss;
  SacPolicyCall terms_call;
  if (int rc = check_policy_terms(h, &pa, who, &terms_call)) return rc;
  SacCloneCall clone_call;
  if (cloning) {
    urgym_sac_clone_args ca;
    memset(&ca, 0, sizeof(ca));
    ca.action_pi = L.action_pi, ca.action_data = L.batch.action, ca.weight = cloning->weight, ca.bc_scale = scale;
    ca.scale_by_q = cloning->scale_by_q, ca.q_filter = cloning->q_filter;
    ca.bc_loss_out = cloning->bc_loss, ca.bc_weight_out = cloning->bc_weight, ca.bc_rows_out = cloning->bc_rows;
    if (int rc = check_policy_terms_cloned(h, terms_call, &ca, who, &clone_call)) return rc;
  }
  const bool clone_masked = cloning && demonstrating && demonstrating->clone_demonstrations_only != 0;  // row_mask = source
  SacAdvantageCall weight_call;
  if (weighting) {
    urgym_sac_advantage_args wa;
    memset(&wa, 0, sizeof(wa));
    wa.temperature = weighting->temperature, wa.max_weight = weighting->max_weight, wa.row_mask = clone_masked ? demonstrating->source : nullptr;
    wa.adv_ess_out = weighting->adv_ess, wa.adv_max_out = weighting->adv_max, wa.adv_clipped_out = weighting->adv_clipped;
    if (int rc = check_policy_terms_weighted(h, clone_call, &wa, who, &weight_call)) return rc;
  }
  const urgym_actor_upstream upstream{L.d_action, L.d_log_prob, nullptr, nullptr};
  urgym_actor_param_grads ag;
  memset(&ag, 0, sizeof(ag));
  {
    const urgym_actor_tensors_const& g = L.actor_adam.grad;
    ag.w0 = (float*)g.w0, ag.b0 = (float*)g.b0, ag.w1 = (float*)g.w1, ag.b1 = (float*)g.b1;
    ag.w_mu = (float*)g.w_mu, ag.b_mu = (float*)g.b_mu, ag.w_log_std = (float*)g.w_log_std, ag.b_log_std = (float*)g.b_log_std;
  }
  Actor* actor = nullptr;
  ActorBackwardCall actor_backward;
  if (int rc = check_actor_parameter_gradients(h, L.actor, &how, &batch_rows, M, &upstream, &ag, L.actor_workspace, L.actor_workspace_bytes, who, &actor,
                                               &actor_backward))
    return rc;
  ActorAdamStep actor_step;
  if (int rc = check_actor_adam(h, L.actor, &L.actor_adam, &hp, who, &actor_step)) return rc;
  if (clip) {
    const urgym_grad_norm na{clip->max_grad_norm, 0, clip->actor_grad_norm, clip->scale + 1, nullptr};
    if (int rc = check_actor_grad_norm(h, L.actor, &L.actor_adam.grad, &na, who, &actor_norm)) return rc;
  }

  if (int rc = extras.check()) return rc;

  // ---- the launching halves: nothing below refuses
  int64_t u = 0;
  for (int i = 0; i < S.num_iterations; i++) {
    const SacIteration it = sac_schedule_iteration(S, i);
    if (K > 0)
      if (int rc = collect(i, it)) return rc;
    if (it.idle) {
      if (int rc = extras.after(i)) return rc;
      continue;
    }
    gather.oldest_slot = it.oldest_slot, gather.size = (uint64_t)it.filled_steps * (uint64_t)h->cfg.num_envs;
    gather_nstep.filled_steps = it.filled_steps;
    if (her) gather_her.g.oldest_slot = gather.oldest_slot, gather_her.g.size = gather.size, gather_her.filled_steps = it.filled_steps;
    if (demonstrating) gather_mixed.g.oldest_slot = gather.oldest_slot, gather_mixed.g.size = gather.size;
    for (int g = 0; g < G; g++, u++) {
      const SacUpdate up = sac_schedule_update(S, u);
      const AdamCoef coef = adam_coefficients(L.lr, L.beta1, L.beta2, L.eps, up.adam_step);  // urgym_adam_coefficients' own function
      gather.draw = up.gather_draw;
      per_gather.g.draw = up.gather_draw;
      gather_her.g.draw = up.gather_draw;
      gather_mixed.g.draw = up.gather_draw;
      if (demonstrating)
        replay_gather_mixed_launch(gather_mixed, s);
      else if (her)
        replay_gather_hindsight_launch(gather_her, s);
      else if (per)
        per_gather_launch(per_gather, s);
      else if (nstep)
        replay_gather_nstep_launch(gather_nstep, s);
      else
        replay_gather_launch(gather, s);
      if (int rc = train_stage(h, who, i, "replay_sample")) return rc;
      if (norm_batch.segments > 0) {
        norm_apply_launch(norm_batch, s);
        if (int rc = train_stage(h, who, i, "norm_batch")) return rc;
      }
      next_sample.smp.draw = up.gather_draw;
      policy_launch(next_sample.a, next_sample.env, next_sample.actions, nullptr, next_sample.smp, s);
      if (int rc = train_stage(h, who, i, "actor_sample_rows (next rows)")) return rc;
      critic_launch(target, bootstrap, s);
      if (int rc = train_stage(h, who, i, "critic_evaluate")) return rc;
      policy_sample.smp.draw = up.policy_draw;
      policy_launch(policy_sample.a, policy_sample.env, policy_sample.actions, nullptr, policy_sample.smp, s);
      if (int rc = train_stage(h, who, i, "actor_sample_rows (batch rows)")) return rc;
      if (nstep) {
        entropy_nstep.c = coef, entropy_nstep.loss_out = L.ent_coef_loss + up.loss_slot;
        sac_entropy_nstep_launch(entropy_nstep, s);
      } else {
        entropy.c = coef, entropy.loss_out = L.ent_coef_loss + up.loss_slot;
        sac_entropy_launch(entropy, s);
      }
      if (int rc = train_stage(h, who, i, "sac_entropy_step")) return rc;
      if (per) {
        critic_launch(online_q, evaluate_q, s);
        if (int rc = train_stage(h, who, i, "critic_evaluate (batch rows)")) return rc;
        per_terms.size = (float)((uint64_t)it.filled_steps * (uint64_t)h->cfg.num_envs);
        per_terms.beta = per_beta(per->beta0, up.adam_step, per->beta_steps);
        per_terms_launch(per_terms, s);
        if (int rc = train_stage(h, who, i, "per_terms")) return rc;
      }
      critic_backward_launch(online, critic_backward, s);
      if (int rc = train_stage(h, who, i, "critic_parameter_gradients")) return rc;
      if (clip) {
        critic_norm.norm_out = clip->critic_grad_norm + up.loss_slot;
        grad_norm_launch(critic_norm, s);
        if (int rc = train_stage(h, who, i, "critic_grad_norm")) return rc;
        critic_adam_scaled_launch(critic_step.buf, &critic_step.target_buf, critic_step.T, coef, critic_step.tau, clip->scale, s);
      } else {
        critic_adam_launch(critic_step.buf, &critic_step.target_buf, critic_step.T, coef, critic_step.tau, s);
      }
      if (int rc = train_stage(h, who, i, "critic_adam_step")) return rc;
      critic_grad_launch(online_grad, action_gradient, s);
      if (int rc = train_stage(h, who, i, "critic_action_gradient")) return rc;
      terms_call.critic_loss_out = L.critic_loss + up.loss_slot, terms_call.actor_loss_out = L.actor_loss + up.loss_slot;
      if (cloning) {
        clone_call.bc_loss_out = cloning->bc_loss + up.loss_slot, clone_call.bc_weight_out = cloning->bc_weight + up.loss_slot;
        clone_call.bc_rows_out = cloning->bc_rows + up.loss_slot;
        if (weighting) {
          weight_call.adv_ess_out = weighting->adv_ess + up.loss_slot, weight_call.adv_max_out = weighting->adv_max + up.loss_slot;
          weight_call.adv_clipped_out = weighting->adv_clipped + up.loss_slot;
          sac_policy_bc_weighted_launch(terms_call, clone_call, weight_call, s);
        } else if (clone_masked)
          sac_policy_bc_masked_launch(terms_call, clone_call, demonstrating->source, s);
        else
          sac_policy_bc_launch(terms_call, clone_call, s);
      } else {
        sac_policy_launch(terms_call, s);
      }
      if (int rc = train_stage(h, who, i, "sac_policy_terms")) return rc;
      actor_backward.draw = up.policy_draw;
      actor_backward_launch(actor, actor_backward, s);
      if (int rc = train_stage(h, who, i, "actor_parameter_gradients")) return rc;
      if (clip) {
        actor_norm.norm_out = clip->actor_grad_norm + up.loss_slot;
        grad_norm_launch(actor_norm, s);
        if (int rc = train_stage(h, who, i, "actor_grad_norm")) return rc;
        actor_adam_scaled_launch(actor_step.buf, actor_step.T, coef, clip->scale + 1, s);
      } else {
        actor_adam_launch(actor_step.buf, actor_step.T, coef, s);
      }
      if (int rc = train_stage(h, who, i, "actor_adam_step")) return rc;
      actor_mark_log_std(actor_step.a);  // as urgym_actor_adam_step; the checks above have required the head already
    }
    if (planning && planning->sync != 0 && G > 0) {  // planner_sync: the launches of urgym_actor_load and urgym_critic_load (tau = 1) on the planner handle
      if (planned.sync_actor) {
        const urgym_actor_tensors& p = L.actor_adam.param;
        const float* src[PACK_ACTOR_TENSORS] = {p.w0, p.b0, p.w1, p.b1, p.w_mu, p.b_mu, p.w_log_std, p.b_log_std};
        actor_pack_launch(actor_packed(planned.sync_actor), src, s);
        if (int rc = train_stage(h, who, i, "planner_sync (actor)")) return rc;
        if (p.w_log_std) actor_mark_log_std(planned.sync_actor);
      }
      if (planned.sync_critic) {
        const float* src[2 * PACK_CRITIC_TENSORS];
        for (int net = 0; net < 2; net++) {
          const auto& q = L.critic_adam.param[net];
          const float* one[PACK_CRITIC_TENSORS] = {q.w0, q.b0, q.w1, q.b1, q.w_q, q.b_q};
          for (int k = 0; k < PACK_CRITIC_TENSORS; k++) src[PACK_CRITIC_TENSORS * net + k] = one[k];
        }
        critic_pack_launch(critic_packed(planned.sync_critic), src, 1.0f, s);
        if (int rc = train_stage(h, who, i, "planner_sync (critic)")) return rc;
      }
    }
    if (int rc = extras.after(i)) return rc;
  }
  return URGYM_OK;
}

// what urgym_sac_train_clipped and urgym_sac_train_normalized refuse before the driver: the body takes the three gathers' options as given
const char* const ONE_GATHER = "at most one of nstep, prioritized and hindsight may be given (each has a gather of its own)";

}  // namespace

extern "C" {

// Each entry point: the null handle, its own required option, then the driver with what it was given.  TrainOptions' order is
// {nstep, per, her, clip, norm, evaluation, monitoring, planning, temper, noise, cloning, demonstrating, weighting}.

int urgym_sac_train(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  return sac_train_body("urgym_sac_train", h, learner, schedule, (hipStream_t)stream, TrainOptions{});
}

int urgym_sac_train_evaluated(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_evaluation* evaluation, void* stream) {
  const char* who = "urgym_sac_train_evaluated";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!evaluation) return fail_in(h, URGYM_ERR_ARG, who, "null evaluation");
  return sac_train_body(who, h, learner, schedule, (hipStream_t)stream, TrainOptions{nullptr, nullptr, nullptr, nullptr, nullptr, evaluation, nullptr});
}

int urgym_sac_train_monitored(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring, void* stream) {
  const char* who = "urgym_sac_train_monitored";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!monitoring) return fail_in(h, URGYM_ERR_ARG, who, "null monitoring");
  return sac_train_body(who, h, learner, schedule, (hipStream_t)stream, TrainOptions{nullptr, nullptr, nullptr, nullptr, nullptr, evaluation_or_NULL, monitoring});
}

int urgym_sac_train_nstep(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_nstep* nstep, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream) {
  const char* who = "urgym_sac_train_nstep";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!nstep) return fail_in(h, URGYM_ERR_ARG, who, "null nstep");
  return sac_train_body(who, h, learner, schedule, (hipStream_t)stream, TrainOptions{nstep, nullptr, nullptr, nullptr, nullptr, evaluation_or_NULL, monitoring_or_NULL});
}

int urgym_sac_train_prioritized(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_prioritized* prioritized, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream) {
  const char* who = "urgym_sac_train_prioritized";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!prioritized) return fail_in(h, URGYM_ERR_ARG, who, "null prioritized");
  return sac_train_body(who, h, learner, schedule, (hipStream_t)stream, TrainOptions{nullptr, prioritized, nullptr, nullptr, nullptr, evaluation_or_NULL, monitoring_or_NULL});
}

int urgym_sac_train_hindsight(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_hindsight* hindsight, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream) {
  const char* who = "urgym_sac_train_hindsight";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!hindsight) return fail_in(h, URGYM_ERR_ARG, who, "null hindsight");
  return sac_train_body(who, h, learner, schedule, (hipStream_t)stream, TrainOptions{nullptr, nullptr, hindsight, nullptr, nullptr, evaluation_or_NULL, monitoring_or_NULL});
}

int urgym_sac_train_clipped(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_clipping* clipping, const urgym_sac_nstep* nstep_or_NULL, const urgym_sac_prioritized* prioritized_or_NULL, const urgym_sac_hindsight* hindsight_or_NULL, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream) {
  const char* who = "urgym_sac_train_clipped";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!clipping) return fail_in(h, URGYM_ERR_ARG, who, "null clipping");
  if ((nstep_or_NULL != nullptr) + (prioritized_or_NULL != nullptr) + (hindsight_or_NULL != nullptr) > 1) return fail_in(h, URGYM_ERR_ARG, who, ONE_GATHER);
  return sac_train_body(who, h, learner, schedule, (hipStream_t)stream, TrainOptions{nstep_or_NULL, prioritized_or_NULL, hindsight_or_NULL, clipping, nullptr, evaluation_or_NULL, monitoring_or_NULL});
}

int urgym_sac_train_normalized(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_normalization* normalization, const urgym_sac_clipping* clipping_or_NULL, const urgym_sac_nstep* nstep_or_NULL, const urgym_sac_prioritized* prioritized_or_NULL, const urgym_sac_hindsight* hindsight_or_NULL, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream) {
  const char* who = "urgym_sac_train_normalized";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!normalization) return fail_in(h, URGYM_ERR_ARG, who, "null normalization");
  if ((nstep_or_NULL != nullptr) + (prioritized_or_NULL != nullptr) + (hindsight_or_NULL != nullptr) > 1) return fail_in(h, URGYM_ERR_ARG, who, ONE_GATHER);
  return sac_train_body(who, h, learner, schedule, (hipStream_t)stream, TrainOptions{nstep_or_NULL, prioritized_or_NULL, hindsight_or_NULL, clipping_or_NULL, normalization, evaluation_or_NULL, monitoring_or_NULL});
}

int urgym_sac_train_planned(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_planning* planning, const urgym_sac_clipping* clipping_or_NULL, const urgym_sac_nstep* nstep_or_NULL, const urgym_sac_prioritized* prioritized_or_NULL, const urgym_sac_hindsight* hindsight_or_NULL, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream) {
  const char* who = "urgym_sac_train_planned";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!planning) return fail_in(h, URGYM_ERR_ARG, who, "null planning");
  if ((nstep_or_NULL != nullptr) + (prioritized_or_NULL != nullptr) + (hindsight_or_NULL != nullptr) > 1) return fail_in(h, URGYM_ERR_ARG, who, ONE_GATHER);
  return sac_train_body(who, h, learner, schedule, (hipStream_t)stream, TrainOptions{nstep_or_NULL, prioritized_or_NULL, hindsight_or_NULL, clipping_or_NULL, nullptr, evaluation_or_NULL, monitoring_or_NULL, planning});
}

int urgym_sac_train_tempered(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_planning* planning, const urgym_mppi_temper* temper, const urgym_sac_clipping* clipping_or_NULL, const urgym_sac_nstep* nstep_or_NULL, const urgym_sac_prioritized* prioritized_or_NULL, const urgym_sac_hindsight* hindsight_or_NULL, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream) {
  const char* who = "urgym_sac_train_tempered";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!planning) return fail_in(h, URGYM_ERR_ARG, who, "null planning");
  if (!temper) return fail_in(h, URGYM_ERR_ARG, who, "null urgym_mppi_temper");
  if ((nstep_or_NULL != nullptr) + (prioritized_or_NULL != nullptr) + (hindsight_or_NULL != nullptr) > 1) return fail_in(h, URGYM_ERR_ARG, who, ONE_GATHER);
  return sac_train_body(who, h, learner, schedule, (hipStream_t)stream, TrainOptions{nstep_or_NULL, prioritized_or_NULL, hindsight_or_NULL, clipping_or_NULL, nullptr, evaluation_or_NULL, monitoring_or_NULL, planning, temper});
}

int urgym_sac_train_colored(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_planning* planning, const urgym_mppi_noise* noise, const urgym_mppi_temper* temper_or_NULL, const urgym_sac_clipping* clipping_or_NULL, const urgym_sac_nstep* nstep_or_NULL, const urgym_sac_prioritized* prioritized_or_NULL, const urgym_sac_hindsight* hindsight_or_NULL, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream) {
  const char* who = "urgym_sac_train_colored";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!planning) return fail_in(h, URGYM_ERR_ARG, who, "null planning");
  if (!noise) return fail_in(h, URGYM_ERR_ARG, who, "null urgym_mppi_noise");
  if ((nstep_or_NULL != nullptr) + (prioritized_or_NULL != nullptr) + (hindsight_or_NULL != nullptr) > 1) return fail_in(h, URGYM_ERR_ARG, who, ONE_GATHER);
  return sac_train_body(who, h, learner, schedule, (hipStream_t)stream, TrainOptions{nstep_or_NULL, prioritized_or_NULL, hindsight_or_NULL, clipping_or_NULL, nullptr, evaluation_or_NULL, monitoring_or_NULL, planning, temper_or_NULL, noise});
}

int urgym_sac_train_cloned(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_cloning* cloning, const urgym_sac_planning* planning_or_NULL, const urgym_mppi_temper* temper_or_NULL, const urgym_mppi_noise* noise_or_NULL, const urgym_normalization* normalization_or_NULL, const urgym_sac_clipping* clipping_or_NULL, const urgym_sac_nstep* nstep_or_NULL, const urgym_sac_prioritized* prioritized_or_NULL, const urgym_sac_hindsight* hindsight_or_NULL, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream) {
  const char* who = "urgym_sac_train_cloned";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!cloning) return fail_in(h, URGYM_ERR_ARG, who, "null cloning");
  if (!planning_or_NULL && (temper_or_NULL || noise_or_NULL)) return fail_in(h, URGYM_ERR_ARG, who, "temper and noise are the planner's and need planning");
  if (planning_or_NULL && normalization_or_NULL) return fail_in(h, URGYM_ERR_ARG, who, "normalization together with planning is out of scope (the planner's actor and critic read raw rows)");
  if ((nstep_or_NULL != nullptr) + (prioritized_or_NULL != nullptr) + (hindsight_or_NULL != nullptr) > 1) return fail_in(h, URGYM_ERR_ARG, who, ONE_GATHER);
  return sac_train_body(who, h, learner, schedule, (hipStream_t)stream, TrainOptions{nstep_or_NULL, prioritized_or_NULL, hindsight_or_NULL, clipping_or_NULL, normalization_or_NULL, evaluation_or_NULL, monitoring_or_NULL, planning_or_NULL, temper_or_NULL, noise_or_NULL, cloning});
}

int urgym_sac_train_demonstrated(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_demonstrating* demonstrating, const urgym_sac_cloning* cloning_or_NULL, const urgym_sac_planning* planning_or_NULL, const urgym_mppi_temper* temper_or_NULL, const urgym_mppi_noise* noise_or_NULL, const urgym_normalization* normalization_or_NULL, const urgym_sac_clipping* clipping_or_NULL, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream) {
  const char* who = "urgym_sac_train_demonstrated";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!demonstrating) return fail_in(h, URGYM_ERR_ARG, who, "null demonstrating");
  if (!planning_or_NULL && (temper_or_NULL || noise_or_NULL)) return fail_in(h, URGYM_ERR_ARG, who, "temper and noise are the planner's and need planning");
  if (planning_or_NULL && normalization_or_NULL) return fail_in(h, URGYM_ERR_ARG, who, "normalization together with planning is out of scope (the planner's actor and critic read raw rows)");
  return sac_train_body(who, h, learner, schedule, (hipStream_t)stream, TrainOptions{nullptr, nullptr, nullptr, clipping_or_NULL, normalization_or_NULL, evaluation_or_NULL, monitoring_or_NULL, planning_or_NULL, temper_or_NULL, noise_or_NULL, cloning_or_NULL, demonstrating});
}

int urgym_sac_train_weighted(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_weighting* weighting, const urgym_sac_cloning* cloning, const urgym_sac_demonstrating* demonstrating_or_NULL, const urgym_sac_planning* planning_or_NULL, const urgym_mppi_temper* temper_or_NULL, const urgym_mppi_noise* noise_or_NULL, const urgym_normalization* normalization_or_NULL, const urgym_sac_clipping* clipping_or_NULL, const urgym_sac_nstep* nstep_or_NULL, const urgym_sac_prioritized* prioritized_or_NULL, const urgym_sac_hindsight* hindsight_or_NULL, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream) {
  const char* who = "urgym_sac_train_weighted";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (!weighting) return fail_in(h, URGYM_ERR_ARG, who, "null weighting");
  if (!cloning) return fail_in(h, URGYM_ERR_ARG, who, "null cloning");
  if (!planning_or_NULL && (temper_or_NULL || noise_or_NULL)) return fail_in(h, URGYM_ERR_ARG, who, "temper and noise are the planner's and need planning");
  if (planning_or_NULL && normalization_or_NULL) return fail_in(h, URGYM_ERR_ARG, who, "normalization together with planning is out of scope (the planner's actor and critic read raw rows)");
  if ((nstep_or_NULL != nullptr) + (prioritized_or_NULL != nullptr) + (hindsight_or_NULL != nullptr) > 1) return fail_in(h, URGYM_ERR_ARG, who, ONE_GATHER);
  if (demonstrating_or_NULL && (nstep_or_NULL || prioritized_or_NULL || hindsight_or_NULL))
    return fail_in(h, URGYM_ERR_ARG, who, "demonstrations together with nstep, prioritized or hindsight is out of scope (each of those has a gather of its own)");
  return sac_train_body(who, h, learner, schedule, (hipStream_t)stream, TrainOptions{nstep_or_NULL, prioritized_or_NULL, hindsight_or_NULL, clipping_or_NULL, normalization_or_NULL, evaluation_or_NULL, monitoring_or_NULL, planning_or_NULL, temper_or_NULL, noise_or_NULL, cloning, demonstrating_or_NULL, weighting});
}

}  // extern "C"
