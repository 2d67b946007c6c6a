// urgym_mppi_abi.hip -- the planner's entry points of include/urgym.h ("sampling-based MPC on the device", "MPPI with the learner in the
// loop", "planner-collected experience", "elite samples and an adaptive std", "the planner inside the training call", "the temperature from a
// target effective sample size", "temporally correlated sampling noise"; DESIGN.md sections 26 to 32), and those of the scripted reach
// controller ("a scripted reach controller on the device"; its launch: urgym_ik.h), which share the planner's record
// pass and the checks of its collection.  Host code only, beside
// urgym_policy_abi.hip: every check is made here, before the first launch; every launch goes through urgym_mppi.h, urgym_mppi_guide.h,
// urgym_mppi_collect.h, urgym_mppi_elite.h, urgym_mppi_temper.h, urgym_mppi_noise.h, the actor's and the critic's own launches (urgym_actor.h, urgym_critic.h), the ring's store
// pass (urgym_replay.h) or through do_step of urgym_hip.hip (urgym_handle.h); the one exception is the device-to-device copy of new_std
// into std between two iterations of an adaptive plan.  As there, each entry point is a checking half, which launches nothing, and a
// launching half, which refuses nothing.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/urgym.h"
#include <algorithm>

#include "urgym_actor.h"
#include "urgym_critic.h"
#include "urgym_handle.h"
#include "urgym_ik.h"
#include "urgym_mppi.h"
#include "urgym_mppi_collect.h"
#include "urgym_mppi_elite.h"
#include "urgym_mppi_guide.h"
#include "urgym_mppi_noise.h"
#include "urgym_mppi_stats.h"
#include "urgym_mppi_temper.h"
#include "urgym_mppi_train.h"
#include "urgym_replay.h"

using namespace urgym;

namespace {

constexpr uint64_t DRAW_END = (uint64_t)1 << 32;  // the counter holds 32 bits of the draw

struct NamedPointer {
  const char* name;
  const void* p;
};

// the checks that concern the struct alone; `report` keeps the message
int check_mppi(Handle* report, const urgym_mppi* m, const char* who) {
  static_assert(sizeof(urgym_mppi) == 176 && alignof(urgym_mppi) == 8, "include/urgym.h");
  if (!m) return fail_in(report, URGYM_ERR_ARG, who, "null urgym_mppi");
  const char* what = nullptr;
  if (m->reserved0 != 0 || m->reserved1 != 0) what = "urgym_mppi.reserved0 and reserved1 must be 0";
  else if (m->num_parents < 1) what = "urgym_mppi.num_parents must be positive";
  else if (m->samples < 2 || m->samples > URGYM_MPPI_SAMPLES_MAX) what = "urgym_mppi.samples must be in [2, URGYM_MPPI_SAMPLES_MAX] (1024)";
  else if (m->horizon < 1 || m->horizon > URGYM_MPPI_HORIZON_MAX) what = "urgym_mppi.horizon must be in [1, URGYM_MPPI_HORIZON_MAX] (64)";
  else if (m->iterations < 1 || m->iterations > URGYM_MPPI_ITERATIONS_MAX) what = "urgym_mppi.iterations must be in [1, URGYM_MPPI_ITERATIONS_MAX] (8)";
  else if ((int64_t)m->num_parents * m->samples > INT32_MAX) what = "num_parents * samples does not fit an env count";
  else if (!isfinite(m->sigma) || m->sigma < 0.0f) what = "urgym_mppi.sigma must be finite and not negative";
  else if (!isfinite(m->lam) || m->lam <= 0.0) what = "urgym_mppi.lam must be finite and positive";
  else if (!isfinite(m->gamma)) what = "urgym_mppi.gamma must be finite";
  if (what) return fail_in(report, URGYM_ERR_ARG, who, what);
  const NamedPointer required[] = {{"mean", m->mean},       {"new_mean", m->new_mean},       {"actions", m->actions},
                                   {"eps", m->eps},         {"ret", m->ret},                 {"g", m->g},
                                   {"alive", m->alive},     {"end_step", m->end_step},       {"success", m->success},
                                   {"collided", m->collided}, {"action_out", m->action_out}, {"best_return", m->best_return},
                                   {"nominal_return", m->nominal_return}, {"ess", m->ess}};
  for (const NamedPointer& r : required)
    if (!r.p) return failf(report, URGYM_ERR_ARG, "%s: urgym_mppi.%s is null", who, r.name);
  return URGYM_OK;
}

int check_bound(Handle* report, const Handle* h, const char* who, const char* which) {
  if (!h->bound) return failf(report, URGYM_ERR_STATE, "%s: urgym_bind() has not been called on the %s handle", who, which);
  return URGYM_OK;
}

int check_planner(Handle* report, const Handle* ph, const urgym_mppi* m, const char* who) {
  if (int rc = check_bound(report, ph, who, "planner")) return rc;
  if ((int64_t)ph->cfg.num_envs != (int64_t)m->num_parents * m->samples)
    return failf(report, URGYM_ERR_ARG, "%s: the planner has %d envs, num_parents * samples is %lld", who, ph->cfg.num_envs,
                 (long long)m->num_parents * m->samples);
  return URGYM_OK;
}

int check_source(Handle* report, const Handle* sh, const urgym_mppi* m, const char* who) {
  if (int rc = check_bound(report, sh, who, "source")) return rc;
  if (sh->cfg.num_envs != m->num_parents) return failf(report, URGYM_ERR_ARG, "%s: the source has %d envs, num_parents is %d", who, sh->cfg.num_envs, m->num_parents);
  return URGYM_OK;
}

// the checks of a call that moves a source's state into a planner (urgym_mppi_fanout, _plan, _control); the source keeps the message
int check_pair(Handle* sh, Handle* ph, const urgym_mppi* m, const char* who) {
  if (!ph) return fail_in(sh, URGYM_ERR_ARG, who, "null planner handle");
  if (int rc = check_mppi(sh, m, who)) return rc;
  if (int rc = check_source(sh, sh, m, who)) return rc;
  if (int rc = check_planner(sh, ph, m, who)) return rc;
  if (sh == ph) return fail_in(sh, URGYM_ERR_ARG, who, "source and planner are the same handle");
  if (sh->device != ph->device) return failf(sh, URGYM_ERR_ARG, "%s: the source is on device %d, the planner on device %d", who, sh->device, ph->device);
  if (ph->cfg.auto_reset != 0) return fail_in(sh, URGYM_ERR_ARG, who, "the planner must have auto_reset == 0 (its episodes must not restart)");
  urgym_config a = sh->cfg, b = ph->cfg;
  a.num_envs = b.num_envs = 0, a.auto_reset = b.auto_reset = 0;
  if (memcmp(&a, &b, sizeof(a)) != 0)
    return fail_in(sh, URGYM_ERR_ARG, who, "source and planner differ in a urgym_config field other than num_envs and auto_reset");
  return URGYM_OK;
}

int check_draw(Handle* report, uint64_t first_draw, int count, const char* who) {
  if (first_draw >= DRAW_END || first_draw + (uint64_t)count > DRAW_END) return fail_in(report, URGYM_ERR_ARG, who, "draw must stay below 2^32");
  return URGYM_OK;
}

MppiFanout fanout_of(const Handle* sh, const Handle* ph, const urgym_mppi& m) {
  return MppiFanout{sh->buf, ph->buf, m.num_parents, m.samples, sh->obs_dim, sh->goal_dim};
}

MppiOutcome outcome_of(const Handle* ph) {
  const urgym_buffers& b = ph->buf;
  return MppiOutcome{b.reward, b.terminated, b.truncated, b.is_success, b.collision};
}

int check_record(Handle* sh, int k, int num_steps, const urgym_trajectory* t, const char* who) {
  if (num_steps < 1) return fail_in(sh, URGYM_ERR_ARG, who, "num_steps must be positive");
  if (k < 0 || k > num_steps) return fail_in(sh, URGYM_ERR_ARG, who, "k must be in [0, num_steps]");
  if (t && (t->episode_return || t->episode_last_step || t->episode_success) && !t->episode_done)
    return fail_in(sh, URGYM_ERR_ARG, who, "traj->episode_done is null with an episode summary asked for");
  return URGYM_OK;
}

// pass k of the records: rows k of what the planner sees, rows k - 1 of what the step before returned (actor_pass of urgym_policy_abi.hip)
MppiRecord record_of(const Handle* sh, const urgym_mppi& m, const urgym_trajectory* traj, int k, int num_steps) {
  const urgym_buffers& b = sh->buf;
  const size_t n = (size_t)sh->cfg.num_envs, od = (size_t)sh->obs_dim, gd = (size_t)sh->goal_dim;
  const size_t pre = (size_t)k * n, post = (size_t)(k > 0 ? k - 1 : 0) * n;
  auto at = [](auto* p, size_t off) { return p ? p + off : p; };
  MppiRecord r;
  memset(&r, 0, sizeof(r));
  r.E = sh->cfg.num_envs, r.H = m.horizon, r.obs_dim = sh->obs_dim, r.goal_dim = sh->goal_dim, r.auto_reset = sh->cfg.auto_reset;
  r.k = k, r.num_steps = num_steps;
  r.observation = b.observation, r.achieved_goal = b.achieved_goal, r.desired_goal = b.desired_goal, r.reward = b.reward;
  r.final_observation = b.final_observation;
  r.terminated = b.terminated, r.truncated = b.truncated, r.is_success = b.is_success, r.collision = b.collision;
  r.action_in = m.action_out;
  r.mean = m.mean;
  if (!traj) return r;
  const urgym_trajectory& t = *traj;
  r.obs = at(t.observation, pre * od), r.ach = at(t.achieved_goal, pre * gd), r.des = at(t.desired_goal, pre * gd);
  r.action_row = at(t.action, post * 6);
  r.reward_row = at(t.reward, post);
  r.terminated_row = at(t.terminated, post), r.truncated_row = at(t.truncated, post), r.is_success_row = at(t.is_success, post);
  r.collision_row = at(t.collision, post);
  r.final_obs_row = at(t.final_observation, post * od);
  r.ep_return = t.episode_return, r.ep_last = t.episode_last_step, r.ep_success = t.episode_success, r.ep_done = t.episode_done;
  return r;
}

// ---- the guide (urgym_mppi_guide): what a guided plan launches besides the plain one's, resolved by check_guide
struct Guide {
  Actor* actor = nullptr;    // launched where P > 0 or terminal_value
  Critic* critic = nullptr;  // launched with terminal_value
  bool terminal = false;     // the terminal launch is made: terminal_value or fail_cost > 0
  float* policy_action = nullptr;  // what the actor writes
  float* value = nullptr;          // what the critic writes
  MppiGuideCall call;
};

// the checks that concern urgym_mppi_guide; m and the planner have been checked.  `report` keeps the message.
int check_guide(Handle* report, Handle* ph, const urgym_mppi* m, const urgym_mppi_guide* g, const char* who, Guide* out) {
  static_assert(sizeof(urgym_mppi_guide) == 64 && alignof(urgym_mppi_guide) == 8, "include/urgym.h");
  if (!g) return fail_in(report, URGYM_ERR_ARG, who, "null urgym_mppi_guide");
  const bool wants_value = g->terminal_value != 0;
  const char* what = nullptr;
  if (g->reserved0 != 0) what = "urgym_mppi_guide.reserved0 must be 0";
  else if (g->policy_samples < 0 || g->policy_samples > m->samples - 1) what = "urgym_mppi_guide.policy_samples must be in [0, samples - 1]";
  else if (!isfinite(g->policy_sigma) || g->policy_sigma < 0.0f) what = "urgym_mppi_guide.policy_sigma must be finite and not negative";
  else if (!isfinite(g->fail_cost) || g->fail_cost < 0.0) what = "urgym_mppi_guide.fail_cost must be finite and not negative";
  else if (g->policy_samples > 0 && !g->actor) what = "urgym_mppi_guide.actor is null with policy_samples > 0";
  else if (wants_value && !g->actor) what = "urgym_mppi_guide.actor is null with terminal_value";
  else if (wants_value && !g->critic) what = "urgym_mppi_guide.critic is null with terminal_value";
  if (what) return fail_in(report, URGYM_ERR_ARG, who, what);
  const int features = ph->obs_dim + 2 * ph->goal_dim;
  Guide r;
  if (g->actor) {
    if (std::find(ph->actors.begin(), ph->actors.end(), (Actor*)g->actor) == ph->actors.end())
      return fail_in(report, URGYM_ERR_ARG, who, "urgym_mppi_guide.actor is not an actor of the planner handle (actors belong to the handle they were created with)");
    r.actor = (Actor*)g->actor;
    if (actor_in_features(r.actor) != features)
      return failf(report, URGYM_ERR_ARG, "%s: urgym_mppi_guide.actor takes %d features, this env kind offers %d", who, actor_in_features(r.actor), features);
  }
  if (g->critic) {
    if (std::find(ph->critics.begin(), ph->critics.end(), (Critic*)g->critic) == ph->critics.end())
      return fail_in(report, URGYM_ERR_ARG, who, "urgym_mppi_guide.critic is not a critic of the planner handle (critics belong to the handle they were created with)");
    r.critic = (Critic*)g->critic;
    if (critic_in_features(r.critic) != features + 6) return fail_in(report, URGYM_ERR_ARG, who, "urgym_mppi_guide.critic does not take this env kind's features");
  }
  r.terminal = wants_value || g->fail_cost > 0.0;
  if ((g->policy_samples > 0 || wants_value) && !g->policy_action) what = "urgym_mppi_guide.policy_action is null";
  else if (wants_value && !g->value) what = "urgym_mppi_guide.value is null with terminal_value";
  else if (r.terminal && !g->terminal) what = "urgym_mppi_guide.terminal is null";
  if (what) return fail_in(report, URGYM_ERR_ARG, who, what);
  if (g->policy_samples == 0 && !wants_value) r.actor = nullptr;  // given, not used
  if (!wants_value) r.critic = nullptr;
  r.policy_action = g->policy_action, r.value = g->value;
  r.call = MppiGuideCall{g->policy_samples, wants_value ? 1 : 0, g->policy_sigma, g->fail_cost, g->policy_action, g->value, g->terminal};
  *out = r;
  return URGYM_OK;
}

// urgym_actor_forward's launch on the planner's bound rows (actor_env of urgym_policy_abi.hip)
void policy_launch(const Handle* ph, const Guide& gd, hipStream_t s) {
  const urgym_buffers& b = ph->buf;
  const ActorEnv env{ph->cfg.num_envs, ph->obs_dim, ph->goal_dim, ph->cfg.auto_reset, b.observation, b.achieved_goal, b.desired_goal,
                     b.reward, b.final_observation, b.terminated, b.truncated, b.is_success, b.collision};
  actor_launch(gd.actor, env, gd.policy_action, nullptr, s);
}

// urgym_critic_evaluate's launch on the planner's bound rows with action = policy_action, out.q_min = value and nothing else asked for
void value_launch(const Handle* ph, const Guide& gd, hipStream_t s) {
  CriticCall call;
  memset(&call, 0, sizeof(call));
  call.M = ph->cfg.num_envs, call.obs_dim = ph->obs_dim, call.goal_dim = ph->goal_dim;
  call.observation = ph->buf.observation, call.achieved_goal = ph->buf.achieved_goal, call.desired_goal = ph->buf.desired_goal;
  call.action = gd.policy_action;
  call.q_min = gd.value;
  critic_launch(gd.critic, call, s);
}

// ---- elite samples and the adaptive std (urgym_mppi_adapt), resolved by check_adapt
struct Adapt {
  bool adapt_std = false;
  float* std = nullptr;  // what the copy between two iterations writes
  MppiElite call;
};

// the checks that concern urgym_mppi_adapt; m has been checked.  `report` keeps the message.
int check_adapt(Handle* report, const urgym_mppi* m, const urgym_mppi_adapt* a, const char* who, Adapt* out) {
  static_assert(sizeof(urgym_mppi_adapt) == 64 && alignof(urgym_mppi_adapt) == 8, "include/urgym.h");
  if (!a) return fail_in(report, URGYM_ERR_ARG, who, "null urgym_mppi_adapt");
  const char* what = nullptr;
  if (a->elites < 1 || a->elites > m->samples) what = "urgym_mppi_adapt.elites must be in [1, samples]";
  else if (!isfinite(a->std_min) || a->std_min < 0.0f) what = "urgym_mppi_adapt.std_min must be finite and not negative";
  else if (!isfinite(a->std_max) || a->std_max < 0.0f) what = "urgym_mppi_adapt.std_max must be finite and not negative";
  else if (a->std_min > a->std_max) what = "urgym_mppi_adapt.std_min must not exceed std_max";
  if (what) return fail_in(report, URGYM_ERR_ARG, who, what);
  const NamedPointer required[] = {{"std", a->std}, {"new_std", a->new_std}, {"elite_count", a->elite_count}, {"threshold", a->threshold}};
  for (const NamedPointer& r : required)
    if (!r.p) return failf(report, URGYM_ERR_ARG, "%s: urgym_mppi_adapt.%s is null", who, r.name);
  Adapt r;
  r.adapt_std = a->adapt_std != 0;
  r.std = a->std;
  r.call = MppiElite{a->elites, a->std_min, a->std_max, a->std, a->new_std, a->rank, a->elite, a->elite_count, a->threshold};
  *out = r;
  return URGYM_OK;
}

// ---- the temperature from a target effective sample size (urgym_mppi_temper), resolved by check_temper

// the checks that concern urgym_mppi_temper; m and, where given, the adapt struct have been checked.  `report` keeps the message.
int check_temper(Handle* report, const urgym_mppi* m, const urgym_mppi_temper* t, const urgym_mppi_adapt* a, const char* who, MppiTemper* out) {
  static_assert(sizeof(urgym_mppi_temper) == 48 && alignof(urgym_mppi_temper) == 8, "include/urgym.h");
  if (!t) return fail_in(report, URGYM_ERR_ARG, who, "null urgym_mppi_temper");
  const double most = (double)(a ? a->elites : m->samples);
  const char* what = nullptr;
  if (t->reserved0 != 0) what = "urgym_mppi_temper.reserved0 must be 0";
  else if (!isfinite(t->ess_target) || t->ess_target < 1.0 || t->ess_target > most) what = "urgym_mppi_temper.ess_target must be finite and in [1, M] (M = elites; samples without adapt)";
  else if (!isfinite(t->lam_min) || !isfinite(t->lam_max)) what = "urgym_mppi_temper.lam_min and lam_max must be finite";
  else if (t->lam_min < 1e-100 || t->lam_max > 1e100) what = "urgym_mppi_temper.lam_min and lam_max must lie in [1e-100, 1e100]";
  else if (t->lam_min > t->lam_max) what = "urgym_mppi_temper.lam_min must not exceed lam_max";
  else if (t->steps < 1 || t->steps > URGYM_MPPI_TEMPER_STEPS_MAX) what = "urgym_mppi_temper.steps must be in [1, URGYM_MPPI_TEMPER_STEPS_MAX] (64)";
  else if (!t->lam_out) what = "urgym_mppi_temper.lam_out is null";
  if (what) return fail_in(report, URGYM_ERR_ARG, who, what);
  *out = MppiTemper{t->ess_target, t->lam_min, t->lam_max, t->steps, t->lam_out, t->saturated};
  return URGYM_OK;
}

// ---- temporally correlated sampling noise (urgym_mppi_noise), resolved by check_noise

// the checks that concern urgym_mppi_noise.  `report` keeps the message.  The scale is formed here, on the host, once per call; std is
// left null: plan() and the single launch put the adapt struct's there where the width is per element.
int check_noise(Handle* report, const urgym_mppi_noise* z, const char* who, MppiNoise* out) {
  static_assert(sizeof(urgym_mppi_noise) == 8 && alignof(urgym_mppi_noise) == 4, "include/urgym.h");
  if (!z) return fail_in(report, URGYM_ERR_ARG, who, "null urgym_mppi_noise");
  if (z->reserved0 != 0) return fail_in(report, URGYM_ERR_ARG, who, "urgym_mppi_noise.reserved0 must be 0");
  if (!isfinite(z->beta) || z->beta < 0.0f || z->beta > 1.0f) return fail_in(report, URGYM_ERR_ARG, who, "urgym_mppi_noise.beta must be finite and in [0, 1]");
  *out = MppiNoise{z->beta, mppi_noise_scale(z->beta), nullptr};
  return URGYM_OK;
}

// the launches of one plan; everything has been checked.  gd == nullptr: the plain plan.  ad == nullptr: the plain update and sample;
// else the elite update stands in place of the update and, with adapt_std, iterations >= 1 sample with new_std of the iteration before.
// tp != nullptr: the tempered update stands in place of either update.  nz != nullptr: the coloured sample stands in place of either
// sample, after the same copy and with the std where the adaptive sample would have read it.
int plan(Handle* sh, Handle* ph, const urgym_mppi& m, uint64_t draw, hipStream_t s, const Guide* gd = nullptr, const Adapt* ad = nullptr, const MppiTemper* tp = nullptr,
         const MppiNoise* nz = nullptr) {
  const size_t row = (size_t)ph->cfg.num_envs * 6;
  const MppiFanout f = fanout_of(sh, ph, m);
  const MppiOutcome o = outcome_of(ph);
  const bool proposes = gd && gd->call.policy_samples > 0;
  for (int i = 0; i < m.iterations; i++) {
    mppi_fanout_launch(f, s);
    if (ad && ad->adapt_std && i >= 1) {
      const size_t bytes = (size_t)m.horizon * (size_t)m.num_parents * 6 * sizeof(float);
      HIP_TRY(sh, hipMemcpyAsync(ad->std, ad->call.new_std, bytes, hipMemcpyDeviceToDevice, s));
      if (nz) mppi_sample_colored_launch(m, MppiNoise{nz->beta, nz->scale, ad->call.std}, draw, i, s);
      else mppi_sample_adaptive_launch(m, ad->call, draw, i, s);
    } else if (nz) {
      mppi_sample_colored_launch(m, *nz, draw, i, s);
    } else {
      mppi_sample_launch(m, draw, i, s);
    }
    for (int h = 0; h < m.horizon; h++) {
      if (proposes) {
        policy_launch(ph, *gd, s);
        mppi_guide_launch(m, gd->call, h, s);
      }
      if (int rc = do_step(ph, m.actions + (size_t)h * row, s)) {
        if (ph != sh) memcpy(sh->err, ph->err, sizeof(sh->err));  // the caller asks the source
        return rc;
      }
      mppi_score_launch(m, o, h, s);
    }
    if (gd && gd->critic) {
      policy_launch(ph, *gd, s);
      value_launch(ph, *gd, s);
    }
    if (gd && gd->terminal) mppi_terminal_launch(m, gd->call, s);
    urgym_mppi last = m;
    if (i + 1 < m.iterations) last.shift = 0;  // the sequence advances once, after the last refinement
    if (tp) mppi_tempered_update_launch(last, *tp, ad ? &ad->call : nullptr, s);
    else if (ad) mppi_elite_update_launch(last, ad->call, s);
    else mppi_update_launch(last, s);
  }
  return URGYM_OK;
}

// the launches of the closed loop; everything has been checked.  Every launch goes to `s`: stream order alone puts a plan's update
// before the source step that reads action_out, and that step before the record pass that files its outcome and the fan-out that
// clones its state.
int control(Handle* sh, Handle* ph, const urgym_mppi& m, uint64_t first_draw, int num_steps, const urgym_trajectory* traj, hipStream_t s, const Guide* gd = nullptr,
            const Adapt* ad = nullptr, const MppiTemper* tp = nullptr, const MppiNoise* nz = nullptr) {
  mppi_record_launch(record_of(sh, m, traj, 0, num_steps), s);
  for (int t = 0; t < num_steps; t++) {
    if (int rc = plan(sh, ph, m, first_draw + (uint64_t)t, s, gd, ad, tp, nz)) return rc;
    if (int rc = do_step(sh, m.action_out, s)) return rc;
    mppi_record_launch(record_of(sh, m, traj, t + 1, num_steps), s);
  }
  return URGYM_OK;
}

// the checks of the two composed guided calls after check_pair
int check_guided_pair(Handle* sh, Handle* ph, const urgym_mppi* m, const urgym_mppi_guide* g, const char* who, Guide* out) {
  if (int rc = check_pair(sh, ph, m, who)) return rc;
  return check_guide(sh, ph, m, g, who, out);
}

// what the three composed coloured calls resolve before their own checks: the pair, then the optional structs in the order of their
// tempered kin, then the noise.  gd, ad and tp point into the struct where the option was given, else they are null.
struct Colored {
  Guide guide;
  Adapt adapt;
  MppiTemper temper;
  MppiNoise nz;
  const Guide* gd = nullptr;
  const Adapt* ad = nullptr;
  const MppiTemper* tp = nullptr;
};

int check_colored(Handle* sh, Handle* ph, const urgym_mppi* m, const urgym_mppi_noise* noise, const urgym_mppi_temper* temper, const urgym_mppi_adapt* adapt,
                  const urgym_mppi_guide* guide, const char* who, Colored* c) {
  if (int rc = guide ? check_guided_pair(sh, ph, m, guide, who, &c->guide) : check_pair(sh, ph, m, who)) return rc;
  if (adapt)
    if (int rc = check_adapt(sh, m, adapt, who, &c->adapt)) return rc;
  if (temper)
    if (int rc = check_temper(sh, m, temper, adapt, who, &c->temper)) return rc;
  if (int rc = check_noise(sh, noise, who, &c->nz)) return rc;
  c->gd = guide ? &c->guide : nullptr, c->ad = adapt ? &c->adapt : nullptr, c->tp = temper ? &c->temper : nullptr;
  return URGYM_OK;
}

// the checks of the two single guided launches: the planner keeps the message
int check_guided_planner(Handle* ph, const urgym_mppi* m, const urgym_mppi_guide* g, const char* who, Guide* out) {
  if (int rc = check_mppi(ph, m, who)) return rc;
  if (int rc = check_planner(ph, ph, m, who)) return rc;
  return check_guide(ph, ph, m, g, who, out);
}

// ---- planner-collected experience (urgym_mppi_execute, urgym_mppi_collect)

// the checks that concern urgym_mppi_explore; `report` keeps the message
int check_explore(Handle* report, const urgym_mppi_explore* x, const char* who) {
  static_assert(sizeof(urgym_mppi_explore) == 16 && alignof(urgym_mppi_explore) == 8, "include/urgym.h");
  const char* what = nullptr;
  if (!x) what = "null urgym_mppi_explore";
  else if (x->reserved0 != 0) what = "urgym_mppi_explore.reserved0 must be 0";
  else if (!isfinite(x->explore_sigma) || x->explore_sigma < 0.0f) what = "urgym_mppi_explore.explore_sigma must be finite and not negative";
  return what ? fail_in(report, URGYM_ERR_ARG, who, what) : URGYM_OK;
}

MppiExecute execute_of(const urgym_mppi& m, const urgym_mppi_explore& x, uint64_t draw, float* executed) {
  return MppiExecute{m.num_parents, x.explore_sigma, m.seed, draw, m.action_out, executed, x.explore_eps};
}

// what urgym_rollout_collect refuses about the ring and the slots (check_ring and check_collect of urgym_policy_abi.hip, restated)
int check_ring(Handle* h, const urgym_replay_ring* r, int first_slot, int num_steps, const char* who) {
  const char* what = nullptr;
  if (!r) what = "null ring";
  else if (r->capacity_steps <= 0) what = "ring->capacity_steps must be positive";
  else if (r->reserved0 != 0) what = "urgym_replay_ring.reserved0 must be 0";
  else if (!r->observation || !r->achieved_goal || !r->desired_goal || !r->action || !r->reward || !r->next_observation ||
           !r->next_achieved_goal || !r->next_desired_goal || !r->terminated)
    what = "a required ring pointer is null (all but truncated and is_success)";
  else if (first_slot < 0 || first_slot >= r->capacity_steps) what = "first_slot outside [0, capacity_steps)";
  else if (num_steps <= 0) what = "num_steps must be positive";
  return what ? fail_in(h, URGYM_ERR_ARG, who, what) : URGYM_OK;
}

// the store pass before step k of a collection that started at first_slot (replay_store of urgym_policy_abi.hip, restated): the s of
// slot k (k < num_steps), the outcome of slot k - 1
ReplayStore store_of(const Handle* h, const urgym_replay_ring& r, int first_slot, int k, int num_steps) {
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

// The launches of a collection; everything has been checked.  Every launch goes to `s`: stream order alone puts source step t - 1
// before the store pass that files its outcome and the record pass that zeroes the finished envs' mean, those before the plan that
// clones the source's state and reads mean, the plan's update before the execute launch that reads action_out, and that before the
// source step that reads the slot's action rows.
int collect(Handle* sh, Handle* ph, const urgym_mppi& m, const Guide* gd, const urgym_mppi_explore& x, uint64_t first_draw, int num_steps,
            const urgym_replay_ring& ring, int first_slot, hipStream_t s, const Adapt* ad = nullptr, const MppiTemper* tp = nullptr,
            const MppiNoise* nz = nullptr) {
  const size_t row = (size_t)sh->cfg.num_envs * 6, C = (size_t)ring.capacity_steps;
  for (int t = 0; t < num_steps; t++) {
    replay_store_launch(store_of(sh, ring, first_slot, t, num_steps), s);
    if (t > 0) mppi_record_launch(record_of(sh, m, nullptr, t, num_steps), s);
    const uint64_t draw = first_draw + (uint64_t)t;
    if (int rc = plan(sh, ph, m, draw, s, gd, ad, tp, nz)) return rc;
    float* actions = ring.action + (((size_t)first_slot + (size_t)t) % C) * row;  // the execute launch writes the slot, the step reads it
    mppi_execute_launch(execute_of(m, x, draw, actions), s);
    if (int rc = do_step(sh, actions, s)) return rc;
  }
  replay_store_launch(store_of(sh, ring, first_slot, num_steps, num_steps), s);
  mppi_record_launch(record_of(sh, m, nullptr, num_steps, num_steps), s);
  return URGYM_OK;
}

// ---- the scripted reach controller (urgym_controller_actions, _control, _collect)

// the checks of the three calls but the null handle; the handle keeps the message.  An unbound handle is an argument error here.
int check_controller(Handle* h, const urgym_reach_controller* c, const char* who) {
  static_assert(sizeof(urgym_reach_controller) == 40 && alignof(urgym_reach_controller) == 8, "include/urgym.h");
  const char* what = nullptr;
  if (!c) what = "null urgym_reach_controller";
  else if (!h->bound) what = "urgym_bind() has not been called on the handle";
  else if (c->reserved0 != 0) what = "urgym_reach_controller.reserved0 must be 0";
  else if (!isfinite(c->damping) || c->damping < 1e-2 || c->damping > 10.0) what = "urgym_reach_controller.damping must be finite and in [1e-2, 10]";
  else if (!isfinite(c->gain) || c->gain <= 0.0 || c->gain > 10.0) what = "urgym_reach_controller.gain must be finite and in (0, 10]";
  else if (!isfinite(c->explore_sigma) || c->explore_sigma < 0.0f) what = "urgym_reach_controller.explore_sigma must be finite and not negative";
  return what ? fail_in(h, URGYM_ERR_ARG, who, what) : URGYM_OK;
}

IkLaunch ik_of(const Handle* h, const urgym_reach_controller& c, uint64_t draw, float* actions) {
  IkLaunch x;
  x.N = h->cfg.num_envs, x.rotational = h->goal_dim == 6;
  x.damping = c.damping, x.gain = c.gain, x.action_scale = h->cfg.action_scale;
  x.explore_sigma = c.explore_sigma, x.seed = c.seed, x.draw = draw;
  x.q = h->buf.q, x.goal = h->buf.goal;
  x.actions = actions, x.explore_eps = c.explore_eps;
  ik_model_fill(x.model);
  return x;
}

// pass k of the closed loop's records: THE RECORD with the controller's action rows and no mean to zero (a horizon of 0 steps)
MppiRecord controller_record_of(const Handle* h, const urgym_trajectory& traj, int k, int num_steps) {
  urgym_mppi none;
  memset(&none, 0, sizeof(none));
  MppiRecord r = record_of(h, none, &traj, k, num_steps);
  r.action_row = nullptr;  // nothing to copy: the action launch wrote the row where it belongs
  return r;
}

// The launches of the closed loop; everything has been checked.  Every launch goes to `s`: stream order alone puts the action launch
// behind the step that wrote q, and the step that reads the row behind the launch that wrote it.
int controller_control(Handle* h, const urgym_reach_controller& c, uint64_t first_draw, int num_steps, const urgym_trajectory& traj, hipStream_t s) {
  const size_t row = (size_t)h->cfg.num_envs * 6;
  mppi_record_launch(controller_record_of(h, traj, 0, num_steps), s);
  for (int t = 0; t < num_steps; t++) {
    float* actions = traj.action + (size_t)t * row;
    ik_actions_launch(ik_of(h, c, first_draw + (uint64_t)t, actions), s);
    if (int rc = do_step(h, actions, s)) return rc;
    mppi_record_launch(controller_record_of(h, traj, t + 1, num_steps), s);
  }
  return URGYM_OK;
}

// The launches of a collection; everything has been checked.  collect() above with the plan, the record pass and the execute launch
// replaced by the action launch.
int controller_collect(Handle* h, const urgym_reach_controller& c, uint64_t first_draw, int num_steps, const urgym_replay_ring& ring, int first_slot,
                       hipStream_t s) {
  const size_t row = (size_t)h->cfg.num_envs * 6, C = (size_t)ring.capacity_steps;
  for (int t = 0; t < num_steps; t++) {
    replay_store_launch(store_of(h, ring, first_slot, t, num_steps), s);
    float* actions = ring.action + (((size_t)first_slot + (size_t)t) % C) * row;  // the action launch writes the slot, the step reads it
    ik_actions_launch(ik_of(h, c, first_draw + (uint64_t)t, actions), s);
    if (int rc = do_step(h, actions, s)) return rc;
  }
  replay_store_launch(store_of(h, ring, first_slot, num_steps, num_steps), s);
  return URGYM_OK;
}

// ---- plan statistics (urgym_mppi_stats)

// the checks of urgym_mppi_stats but the null handle; `report` keeps the message
int check_stats(Handle* report, const urgym_mppi* m, const urgym_mppi_adapt* a, urgym_mppi_stats_record* record, int64_t iteration, const char* who, MppiStatsCall* out) {
  static_assert(sizeof(urgym_mppi_stats_record) == 88 && alignof(urgym_mppi_stats_record) == 8, "include/urgym.h");
  const char* what = nullptr;
  if (!m) what = "null urgym_mppi";
  else if (!record) what = "null record_dev";
  else if (m->num_parents < 1 || m->num_parents > SAC_TERMS_MAX_COUNT) what = "urgym_mppi.num_parents must be in [1, 65536]";
  else if (!m->best_return || !m->nominal_return || !m->ess) what = "urgym_mppi.best_return, nominal_return or ess is null";
  else if (a && (!a->elite_count || !a->threshold)) what = "urgym_mppi_adapt.elite_count or threshold is null";
  else if ((uintptr_t)record % 8 != 0) what = "record_dev must be 8-byte aligned";
  if (what) return fail_in(report, URGYM_ERR_ARG, who, what);
  *out = MppiStatsCall{m->num_parents, iteration, m->best_return, m->nominal_return, m->ess, a ? a->elite_count : nullptr, a ? a->threshold : nullptr, record};
  return URGYM_OK;
}

}  // namespace

// ---- the planner inside the training call (urgym_mppi_train.h)
namespace urgym {

int planned_check(const char* who, Handle* h, const urgym_sac_planning* planning, const urgym_replay_ring* ring, const urgym_sac_schedule& S, PlannedCall* out,
                  const urgym_mppi_temper* temper_or_NULL, const urgym_mppi_noise* noise_or_NULL) {
  static_assert(sizeof(urgym_sac_planning) == 72 && alignof(urgym_sac_planning) == 8, "include/urgym.h");
  if (!planning) return fail_in(h, URGYM_ERR_ARG, who, "null planning");
  const urgym_sac_planning& P = *planning;
  const char* what = nullptr;
  if (!P.planner_handle) what = "urgym_sac_planning.planner_handle is null";
  else if (!P.mppi) what = "urgym_sac_planning.mppi is null";
  else if (P.reserved0 != 0) what = "urgym_sac_planning.reserved0 must be 0";
  else if (P.record_capacity < 0) what = "urgym_sac_planning.record_capacity is negative";
  else if (S.steps_per_iteration == 0) what = "steps_per_iteration is 0: there is nothing to plan";
  else if (S.uniform_iterations != 0) what = "schedule->uniform_iterations must be 0 (the planner plans from the first step)";
  if (what) return fail_in(h, URGYM_ERR_ARG, who, what);
  Handle* ph = (Handle*)P.planner_handle;
  if (ph == h) return fail_in(h, URGYM_ERR_ARG, who, "planner_handle is the training handle (source and planner are the same handle)");
  const int K = S.steps_per_iteration;
  PlannedCall c;
  memset(&c, 0, sizeof(c));
  Guide gd;
  Adapt ad;
  if (int rc = P.guide_or_NULL ? check_guided_pair(h, ph, P.mppi, P.guide_or_NULL, who, &gd) : check_pair(h, ph, P.mppi, who)) return rc;
  if (P.adapt_or_NULL)
    if (int rc = check_adapt(h, P.mppi, P.adapt_or_NULL, who, &ad)) return rc;
  MppiTemper tp;
  if (temper_or_NULL)
    if (int rc = check_temper(h, P.mppi, temper_or_NULL, P.adapt_or_NULL, who, &tp)) return rc;
  MppiNoise nz;
  if (noise_or_NULL)
    if (int rc = check_noise(h, noise_or_NULL, who, &nz)) return rc;
  if (!h->observed) return fail_in(h, URGYM_ERR_STATE, who, "nothing has been observed yet: urgym_reset() or urgym_refresh() the source first");
  if (int rc = check_explore(h, &P.explore, who)) return rc;
  if (int rc = check_ring(h, ring, S.first_slot, K, who)) return rc;
  if (S.collect_first_draw >= DRAW_END || S.collect_first_draw + (uint64_t)S.num_iterations * (uint64_t)K > DRAW_END)
    return fail_in(h, URGYM_ERR_ARG, who, "draw must stay below 2^32 (collect_first_draw + num_iterations * steps_per_iteration)");
  if (P.records)
    if (int rc = check_stats(h, P.mppi, P.adapt_or_NULL, P.records, 0, who, &c.stats)) return rc;
  c.source = h, c.planner = ph, c.m = *P.mppi, c.explore = P.explore, c.ring = *ring, c.records = P.records, c.record_capacity = P.record_capacity;
  c.guided = P.guide_or_NULL != nullptr, c.adaptive = P.adapt_or_NULL != nullptr;
  if (c.guided) c.guide = *P.guide_or_NULL, c.sync_actor = gd.actor, c.sync_critic = gd.critic;
  if (c.adaptive) c.adapt = *P.adapt_or_NULL;
  c.tempered = temper_or_NULL != nullptr;
  if (c.tempered) c.temper = *temper_or_NULL;
  c.colored = noise_or_NULL != nullptr;
  if (c.colored) c.noise = *noise_or_NULL;
  *out = c;
  return URGYM_OK;
}

// planned_check has accepted the guide, the adapt, the temper and the noise struct: resolving them again refuses nothing
int planned_collect(const PlannedCall& c, uint64_t first_draw, int num_steps, int first_slot, hipStream_t s) {
  const char* who = "planned_collect";
  Guide gd;
  Adapt ad;
  if (c.guided)
    if (int rc = check_guide(c.source, c.planner, &c.m, &c.guide, who, &gd)) return rc;
  if (c.adaptive)
    if (int rc = check_adapt(c.source, &c.m, &c.adapt, who, &ad)) return rc;
  MppiTemper tp;
  if (c.tempered)
    if (int rc = check_temper(c.source, &c.m, &c.temper, c.adaptive ? &c.adapt : nullptr, who, &tp)) return rc;
  MppiNoise nz;
  if (c.colored)
    if (int rc = check_noise(c.source, &c.noise, who, &nz)) return rc;
  return collect(c.source, c.planner, c.m, c.guided ? &gd : nullptr, c.explore, first_draw, num_steps, c.ring, first_slot, s, c.adaptive ? &ad : nullptr,
                 c.tempered ? &tp : nullptr, c.colored ? &nz : nullptr);
}

void planned_stats(const PlannedCall& c, urgym_mppi_stats_record* record, int64_t iteration, hipStream_t s) {
  MppiStatsCall call = c.stats;
  call.record = record, call.iteration = iteration;
  mppi_stats_launch(call, s);
}

}  // namespace urgym

extern "C" {

int urgym_mppi_fanout(void* source_handle, void* planner_handle, const urgym_mppi* m, void* stream) {
  const char* who = "urgym_mppi_fanout";
  Handle *sh = (Handle*)source_handle, *ph = (Handle*)planner_handle;
  if (!sh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_pair(sh, ph, m, who)) return rc;
  HIP_TRY(sh, hipSetDevice(sh->device));
  mppi_fanout_launch(fanout_of(sh, ph, *m), (hipStream_t)stream);
  return launched(sh);
}

int urgym_mppi_sample(void* handle, const urgym_mppi* m, uint64_t draw, int iteration, void* stream) {
  const char* who = "urgym_mppi_sample";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_mppi(h, m, who)) return rc;
  if (int rc = check_draw(h, draw, 1, who)) return rc;
  if (iteration < 0 || iteration >= URGYM_MPPI_ITERATIONS_MAX) return fail_in(h, URGYM_ERR_ARG, who, "iteration must be in [0, URGYM_MPPI_ITERATIONS_MAX)");
  HIP_TRY(h, hipSetDevice(h->device));
  mppi_sample_launch(*m, draw, iteration, (hipStream_t)stream);
  return launched(h);
}

int urgym_mppi_score(void* planner_handle, const urgym_mppi* m, int h, void* stream) {
  const char* who = "urgym_mppi_score";
  Handle* ph = (Handle*)planner_handle;
  if (!ph) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_mppi(ph, m, who)) return rc;
  if (int rc = check_planner(ph, ph, m, who)) return rc;
  if (h < 0 || h >= m->horizon) return fail_in(ph, URGYM_ERR_ARG, who, "h must be in [0, horizon)");
  HIP_TRY(ph, hipSetDevice(ph->device));
  mppi_score_launch(*m, outcome_of(ph), h, (hipStream_t)stream);
  return launched(ph);
}

int urgym_mppi_update(void* handle, const urgym_mppi* m, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_mppi(h, m, "urgym_mppi_update")) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  mppi_update_launch(*m, (hipStream_t)stream);
  return launched(h);
}

int urgym_mppi_record(void* source_handle, const urgym_mppi* m, int k, int num_steps, const urgym_trajectory* traj_or_NULL, void* stream) {
  const char* who = "urgym_mppi_record";
  Handle* sh = (Handle*)source_handle;
  if (!sh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_mppi(sh, m, who)) return rc;
  if (int rc = check_source(sh, sh, m, who)) return rc;
  if (int rc = check_record(sh, k, num_steps, traj_or_NULL, who)) return rc;
  HIP_TRY(sh, hipSetDevice(sh->device));
  mppi_record_launch(record_of(sh, *m, traj_or_NULL, k, num_steps), (hipStream_t)stream);
  return launched(sh);
}

int urgym_mppi_plan(void* source_handle, void* planner_handle, const urgym_mppi* m, uint64_t draw, void* stream) {
  const char* who = "urgym_mppi_plan";
  Handle *sh = (Handle*)source_handle, *ph = (Handle*)planner_handle;
  if (!sh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_pair(sh, ph, m, who)) return rc;
  if (int rc = check_draw(sh, draw, 1, who)) return rc;
  HIP_TRY(sh, hipSetDevice(sh->device));
  if (int rc = plan(sh, ph, *m, draw, (hipStream_t)stream)) return rc;
  return launched(sh);
}

int urgym_mppi_control(void* source_handle, void* planner_handle, const urgym_mppi* m, uint64_t first_draw, int num_steps, const urgym_trajectory* traj_or_NULL, void* stream) {
  const char* who = "urgym_mppi_control";
  Handle *sh = (Handle*)source_handle, *ph = (Handle*)planner_handle;
  hipStream_t s = (hipStream_t)stream;
  if (!sh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_pair(sh, ph, m, who)) return rc;
  if (int rc = check_record(sh, 0, num_steps, traj_or_NULL, who)) return rc;
  if (int rc = check_draw(sh, first_draw, num_steps, who)) return rc;
  HIP_TRY(sh, hipSetDevice(sh->device));
  if (int rc = control(sh, ph, *m, first_draw, num_steps, traj_or_NULL, s)) return rc;
  return launched(sh);
}

int urgym_mppi_guide_actions(void* planner_handle, const urgym_mppi* m, const urgym_mppi_guide* g, int h, void* stream) {
  const char* who = "urgym_mppi_guide_actions";
  Handle* ph = (Handle*)planner_handle;
  Guide gd;
  if (!ph) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_guided_planner(ph, m, g, who, &gd)) return rc;
  if (h < 0 || h >= m->horizon) return fail_in(ph, URGYM_ERR_ARG, who, "h must be in [0, horizon)");
  HIP_TRY(ph, hipSetDevice(ph->device));
  if (gd.call.policy_samples > 0) mppi_guide_launch(*m, gd.call, h, (hipStream_t)stream);  // P == 0: no sample follows the actor
  return launched(ph);
}

int urgym_mppi_terminal(void* planner_handle, const urgym_mppi* m, const urgym_mppi_guide* g, void* stream) {
  const char* who = "urgym_mppi_terminal";
  Handle* ph = (Handle*)planner_handle;
  Guide gd;
  if (!ph) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_guided_planner(ph, m, g, who, &gd)) return rc;
  if (!gd.terminal) return fail_in(ph, URGYM_ERR_ARG, who, "neither urgym_mppi_guide.terminal_value nor fail_cost > 0: there is no terminal launch");
  HIP_TRY(ph, hipSetDevice(ph->device));
  mppi_terminal_launch(*m, gd.call, (hipStream_t)stream);
  return launched(ph);
}

int urgym_mppi_plan_guided(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_guide* g, uint64_t draw, void* stream) {
  const char* who = "urgym_mppi_plan_guided";
  Handle *sh = (Handle*)source_handle, *ph = (Handle*)planner_handle;
  Guide gd;
  if (!sh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_guided_pair(sh, ph, m, g, who, &gd)) return rc;
  if (int rc = check_draw(sh, draw, 1, who)) return rc;
  HIP_TRY(sh, hipSetDevice(sh->device));
  if (int rc = plan(sh, ph, *m, draw, (hipStream_t)stream, &gd)) return rc;
  return launched(sh);
}

int urgym_mppi_control_guided(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_guide* g, uint64_t first_draw, int num_steps, const urgym_trajectory* traj_or_NULL, void* stream) {
  const char* who = "urgym_mppi_control_guided";
  Handle *sh = (Handle*)source_handle, *ph = (Handle*)planner_handle;
  Guide gd;
  if (!sh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_guided_pair(sh, ph, m, g, who, &gd)) return rc;
  if (int rc = check_record(sh, 0, num_steps, traj_or_NULL, who)) return rc;
  if (int rc = check_draw(sh, first_draw, num_steps, who)) return rc;
  HIP_TRY(sh, hipSetDevice(sh->device));
  if (int rc = control(sh, ph, *m, first_draw, num_steps, traj_or_NULL, (hipStream_t)stream, &gd)) return rc;
  return launched(sh);
}

int urgym_mppi_execute(void* source_handle, const urgym_mppi* m, const urgym_mppi_explore* x, uint64_t draw, float* executed, void* stream) {
  const char* who = "urgym_mppi_execute";
  Handle* sh = (Handle*)source_handle;
  if (!sh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_mppi(sh, m, who)) return rc;
  if (int rc = check_source(sh, sh, m, who)) return rc;
  if (int rc = check_explore(sh, x, who)) return rc;
  if (!executed) return fail_in(sh, URGYM_ERR_ARG, who, "executed is null");
  if (int rc = check_draw(sh, draw, 1, who)) return rc;
  HIP_TRY(sh, hipSetDevice(sh->device));
  mppi_execute_launch(execute_of(*m, *x, draw, executed), (hipStream_t)stream);
  return launched(sh);
}

int urgym_mppi_collect(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_guide* guide_or_NULL, const urgym_mppi_explore* x, uint64_t first_draw, int num_steps, const urgym_replay_ring* ring, int first_slot, void* stream) {
  const char* who = "urgym_mppi_collect";
  Handle *sh = (Handle*)source_handle, *ph = (Handle*)planner_handle;
  Guide gd;
  if (!sh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = guide_or_NULL ? check_guided_pair(sh, ph, m, guide_or_NULL, who, &gd) : check_pair(sh, ph, m, who)) return rc;
  if (!sh->observed) return fail_in(sh, URGYM_ERR_STATE, who, "nothing has been observed yet: urgym_reset() or urgym_refresh() the source first");
  if (int rc = check_explore(sh, x, who)) return rc;
  if (int rc = check_ring(sh, ring, first_slot, num_steps, who)) return rc;
  if (int rc = check_draw(sh, first_draw, num_steps, who)) return rc;
  HIP_TRY(sh, hipSetDevice(sh->device));
  if (int rc = collect(sh, ph, *m, guide_or_NULL ? &gd : nullptr, *x, first_draw, num_steps, *ring, first_slot, (hipStream_t)stream)) return rc;
  return launched(sh);
}

int urgym_mppi_sample_adaptive(void* handle, const urgym_mppi* m, const urgym_mppi_adapt* a, uint64_t draw, int iteration, void* stream) {
  const char* who = "urgym_mppi_sample_adaptive";
  Handle* h = (Handle*)handle;
  Adapt ad;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_mppi(h, m, who)) return rc;
  if (int rc = check_adapt(h, m, a, who, &ad)) return rc;
  if (int rc = check_draw(h, draw, 1, who)) return rc;
  if (iteration < 0 || iteration >= URGYM_MPPI_ITERATIONS_MAX) return fail_in(h, URGYM_ERR_ARG, who, "iteration must be in [0, URGYM_MPPI_ITERATIONS_MAX)");
  HIP_TRY(h, hipSetDevice(h->device));
  mppi_sample_adaptive_launch(*m, ad.call, draw, iteration, (hipStream_t)stream);
  return launched(h);
}

int urgym_mppi_update_elite(void* handle, const urgym_mppi* m, const urgym_mppi_adapt* a, void* stream) {
  const char* who = "urgym_mppi_update_elite";
  Handle* h = (Handle*)handle;
  Adapt ad;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_mppi(h, m, who)) return rc;
  if (int rc = check_adapt(h, m, a, who, &ad)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  mppi_elite_update_launch(*m, ad.call, (hipStream_t)stream);
  return launched(h);
}

int urgym_mppi_plan_adaptive(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_adapt* a, const urgym_mppi_guide* guide_or_NULL, uint64_t draw, void* stream) {
  const char* who = "urgym_mppi_plan_adaptive";
  Handle *sh = (Handle*)source_handle, *ph = (Handle*)planner_handle;
  Guide gd;
  Adapt ad;
  if (!sh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = guide_or_NULL ? check_guided_pair(sh, ph, m, guide_or_NULL, who, &gd) : check_pair(sh, ph, m, who)) return rc;
  if (int rc = check_adapt(sh, m, a, who, &ad)) return rc;
  if (int rc = check_draw(sh, draw, 1, who)) return rc;
  HIP_TRY(sh, hipSetDevice(sh->device));
  if (int rc = plan(sh, ph, *m, draw, (hipStream_t)stream, guide_or_NULL ? &gd : nullptr, &ad)) return rc;
  return launched(sh);
}

int urgym_mppi_control_adaptive(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_adapt* a, const urgym_mppi_guide* guide_or_NULL, uint64_t first_draw, int num_steps, const urgym_trajectory* traj_or_NULL, void* stream) {
  const char* who = "urgym_mppi_control_adaptive";
  Handle *sh = (Handle*)source_handle, *ph = (Handle*)planner_handle;
  Guide gd;
  Adapt ad;
  if (!sh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = guide_or_NULL ? check_guided_pair(sh, ph, m, guide_or_NULL, who, &gd) : check_pair(sh, ph, m, who)) return rc;
  if (int rc = check_adapt(sh, m, a, who, &ad)) return rc;
  if (int rc = check_record(sh, 0, num_steps, traj_or_NULL, who)) return rc;
  if (int rc = check_draw(sh, first_draw, num_steps, who)) return rc;
  HIP_TRY(sh, hipSetDevice(sh->device));
  if (int rc = control(sh, ph, *m, first_draw, num_steps, traj_or_NULL, (hipStream_t)stream, guide_or_NULL ? &gd : nullptr, &ad)) return rc;
  return launched(sh);
}

int urgym_mppi_collect_adaptive(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_adapt* a, const urgym_mppi_guide* guide_or_NULL, const urgym_mppi_explore* x, uint64_t first_draw, int num_steps, const urgym_replay_ring* ring, int first_slot, void* stream) {
  const char* who = "urgym_mppi_collect_adaptive";
  Handle *sh = (Handle*)source_handle, *ph = (Handle*)planner_handle;
  Guide gd;
  Adapt ad;
  if (!sh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = guide_or_NULL ? check_guided_pair(sh, ph, m, guide_or_NULL, who, &gd) : check_pair(sh, ph, m, who)) return rc;
  if (int rc = check_adapt(sh, m, a, who, &ad)) return rc;
  if (!sh->observed) return fail_in(sh, URGYM_ERR_STATE, who, "nothing has been observed yet: urgym_reset() or urgym_refresh() the source first");
  if (int rc = check_explore(sh, x, who)) return rc;
  if (int rc = check_ring(sh, ring, first_slot, num_steps, who)) return rc;
  if (int rc = check_draw(sh, first_draw, num_steps, who)) return rc;
  HIP_TRY(sh, hipSetDevice(sh->device));
  if (int rc = collect(sh, ph, *m, guide_or_NULL ? &gd : nullptr, *x, first_draw, num_steps, *ring, first_slot, (hipStream_t)stream, &ad)) return rc;
  return launched(sh);
}

int urgym_mppi_update_tempered(void* handle, const urgym_mppi* m, const urgym_mppi_temper* temper, const urgym_mppi_adapt* adapt_or_NULL, void* stream) {
  const char* who = "urgym_mppi_update_tempered";
  Handle* h = (Handle*)handle;
  Adapt ad;
  MppiTemper tp;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_mppi(h, m, who)) return rc;
  if (adapt_or_NULL)
    if (int rc = check_adapt(h, m, adapt_or_NULL, who, &ad)) return rc;
  if (int rc = check_temper(h, m, temper, adapt_or_NULL, who, &tp)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  mppi_tempered_update_launch(*m, tp, adapt_or_NULL ? &ad.call : nullptr, (hipStream_t)stream);
  return launched(h);
}

int urgym_mppi_plan_tempered(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_temper* temper, const urgym_mppi_adapt* adapt_or_NULL, const urgym_mppi_guide* guide_or_NULL, uint64_t draw, void* stream) {
  const char* who = "urgym_mppi_plan_tempered";
  Handle *sh = (Handle*)source_handle, *ph = (Handle*)planner_handle;
  Guide gd;
  Adapt ad;
  MppiTemper tp;
  if (!sh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = guide_or_NULL ? check_guided_pair(sh, ph, m, guide_or_NULL, who, &gd) : check_pair(sh, ph, m, who)) return rc;
  if (adapt_or_NULL)
    if (int rc = check_adapt(sh, m, adapt_or_NULL, who, &ad)) return rc;
  if (int rc = check_temper(sh, m, temper, adapt_or_NULL, who, &tp)) return rc;
  if (int rc = check_draw(sh, draw, 1, who)) return rc;
  HIP_TRY(sh, hipSetDevice(sh->device));
  if (int rc = plan(sh, ph, *m, draw, (hipStream_t)stream, guide_or_NULL ? &gd : nullptr, adapt_or_NULL ? &ad : nullptr, &tp)) return rc;
  return launched(sh);
}

int urgym_mppi_control_tempered(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_temper* temper, const urgym_mppi_adapt* adapt_or_NULL, const urgym_mppi_guide* guide_or_NULL, uint64_t first_draw, int num_steps, const urgym_trajectory* traj_or_NULL, void* stream) {
  const char* who = "urgym_mppi_control_tempered";
  Handle *sh = (Handle*)source_handle, *ph = (Handle*)planner_handle;
  Guide gd;
  Adapt ad;
  MppiTemper tp;
  if (!sh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = guide_or_NULL ? check_guided_pair(sh, ph, m, guide_or_NULL, who, &gd) : check_pair(sh, ph, m, who)) return rc;
  if (adapt_or_NULL)
    if (int rc = check_adapt(sh, m, adapt_or_NULL, who, &ad)) return rc;
  if (int rc = check_temper(sh, m, temper, adapt_or_NULL, who, &tp)) return rc;
  if (int rc = check_record(sh, 0, num_steps, traj_or_NULL, who)) return rc;
  if (int rc = check_draw(sh, first_draw, num_steps, who)) return rc;
  HIP_TRY(sh, hipSetDevice(sh->device));
  if (int rc = control(sh, ph, *m, first_draw, num_steps, traj_or_NULL, (hipStream_t)stream, guide_or_NULL ? &gd : nullptr, adapt_or_NULL ? &ad : nullptr, &tp)) return rc;
  return launched(sh);
}

int urgym_mppi_collect_tempered(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_temper* temper, const urgym_mppi_adapt* adapt_or_NULL, const urgym_mppi_guide* guide_or_NULL, const urgym_mppi_explore* x, uint64_t first_draw, int num_steps, const urgym_replay_ring* ring, int first_slot, void* stream) {
  const char* who = "urgym_mppi_collect_tempered";
  Handle *sh = (Handle*)source_handle, *ph = (Handle*)planner_handle;
  Guide gd;
  Adapt ad;
  MppiTemper tp;
  if (!sh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = guide_or_NULL ? check_guided_pair(sh, ph, m, guide_or_NULL, who, &gd) : check_pair(sh, ph, m, who)) return rc;
  if (adapt_or_NULL)
    if (int rc = check_adapt(sh, m, adapt_or_NULL, who, &ad)) return rc;
  if (int rc = check_temper(sh, m, temper, adapt_or_NULL, who, &tp)) return rc;
  if (!sh->observed) return fail_in(sh, URGYM_ERR_STATE, who, "nothing has been observed yet: urgym_reset() or urgym_refresh() the source first");
  if (int rc = check_explore(sh, x, who)) return rc;
  if (int rc = check_ring(sh, ring, first_slot, num_steps, who)) return rc;
  if (int rc = check_draw(sh, first_draw, num_steps, who)) return rc;
  HIP_TRY(sh, hipSetDevice(sh->device));
  if (int rc = collect(sh, ph, *m, guide_or_NULL ? &gd : nullptr, *x, first_draw, num_steps, *ring, first_slot, (hipStream_t)stream, adapt_or_NULL ? &ad : nullptr, &tp)) return rc;
  return launched(sh);
}

int urgym_mppi_sample_colored(void* handle, const urgym_mppi* m, const urgym_mppi_noise* noise, const urgym_mppi_adapt* adapt_or_NULL, uint64_t draw, int iteration, void* stream) {
  const char* who = "urgym_mppi_sample_colored";
  Handle* h = (Handle*)handle;
  Adapt ad;
  MppiNoise nz;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_mppi(h, m, who)) return rc;
  if (adapt_or_NULL)
    if (int rc = check_adapt(h, m, adapt_or_NULL, who, &ad)) return rc;
  if (int rc = check_noise(h, noise, who, &nz)) return rc;
  if (int rc = check_draw(h, draw, 1, who)) return rc;
  if (iteration < 0 || iteration >= URGYM_MPPI_ITERATIONS_MAX) return fail_in(h, URGYM_ERR_ARG, who, "iteration must be in [0, URGYM_MPPI_ITERATIONS_MAX)");
  if (adapt_or_NULL) nz.std = ad.call.std;
  HIP_TRY(h, hipSetDevice(h->device));
  mppi_sample_colored_launch(*m, nz, draw, iteration, (hipStream_t)stream);
  return launched(h);
}

int urgym_mppi_plan_colored(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_noise* noise, const urgym_mppi_temper* temper_or_NULL, const urgym_mppi_adapt* adapt_or_NULL, const urgym_mppi_guide* guide_or_NULL, uint64_t draw, void* stream) {
  const char* who = "urgym_mppi_plan_colored";
  Handle *sh = (Handle*)source_handle, *ph = (Handle*)planner_handle;
  Colored c;
  if (!sh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_colored(sh, ph, m, noise, temper_or_NULL, adapt_or_NULL, guide_or_NULL, who, &c)) return rc;
  if (int rc = check_draw(sh, draw, 1, who)) return rc;
  HIP_TRY(sh, hipSetDevice(sh->device));
  if (int rc = plan(sh, ph, *m, draw, (hipStream_t)stream, c.gd, c.ad, c.tp, &c.nz)) return rc;
  return launched(sh);
}

int urgym_mppi_control_colored(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_noise* noise, const urgym_mppi_temper* temper_or_NULL, const urgym_mppi_adapt* adapt_or_NULL, const urgym_mppi_guide* guide_or_NULL, uint64_t first_draw, int num_steps, const urgym_trajectory* traj_or_NULL, void* stream) {
  const char* who = "urgym_mppi_control_colored";
  Handle *sh = (Handle*)source_handle, *ph = (Handle*)planner_handle;
  Colored c;
  if (!sh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_colored(sh, ph, m, noise, temper_or_NULL, adapt_or_NULL, guide_or_NULL, who, &c)) return rc;
  if (int rc = check_record(sh, 0, num_steps, traj_or_NULL, who)) return rc;
  if (int rc = check_draw(sh, first_draw, num_steps, who)) return rc;
  HIP_TRY(sh, hipSetDevice(sh->device));
  if (int rc = control(sh, ph, *m, first_draw, num_steps, traj_or_NULL, (hipStream_t)stream, c.gd, c.ad, c.tp, &c.nz)) return rc;
  return launched(sh);
}

int urgym_mppi_collect_colored(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_noise* noise, const urgym_mppi_temper* temper_or_NULL, const urgym_mppi_adapt* adapt_or_NULL, const urgym_mppi_guide* guide_or_NULL, const urgym_mppi_explore* x, uint64_t first_draw, int num_steps, const urgym_replay_ring* ring, int first_slot, void* stream) {
  const char* who = "urgym_mppi_collect_colored";
  Handle *sh = (Handle*)source_handle, *ph = (Handle*)planner_handle;
  Colored c;
  if (!sh) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_colored(sh, ph, m, noise, temper_or_NULL, adapt_or_NULL, guide_or_NULL, who, &c)) return rc;
  if (!sh->observed) return fail_in(sh, URGYM_ERR_STATE, who, "nothing has been observed yet: urgym_reset() or urgym_refresh() the source first");
  if (int rc = check_explore(sh, x, who)) return rc;
  if (int rc = check_ring(sh, ring, first_slot, num_steps, who)) return rc;
  if (int rc = check_draw(sh, first_draw, num_steps, who)) return rc;
  HIP_TRY(sh, hipSetDevice(sh->device));
  if (int rc = collect(sh, ph, *m, c.gd, *x, first_draw, num_steps, *ring, first_slot, (hipStream_t)stream, c.ad, c.tp, &c.nz)) return rc;
  return launched(sh);
}

int urgym_mppi_stats(void* handle, const urgym_mppi* m, const urgym_mppi_adapt* a_or_NULL, urgym_mppi_stats_record* record_dev, int64_t iteration, void* stream) {
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  MppiStatsCall c;
  if (int rc = check_stats(h, m, a_or_NULL, record_dev, iteration, "urgym_mppi_stats", &c)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  mppi_stats_launch(c, (hipStream_t)stream);
  return launched(h);
}

int urgym_controller_actions(void* handle, const urgym_reach_controller* c, uint64_t draw, float* actions, void* stream) {
  const char* who = "urgym_controller_actions";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_controller(h, c, who)) return rc;
  if (!actions) return fail_in(h, URGYM_ERR_ARG, who, "actions is null");
  if (int rc = check_draw(h, draw, 1, who)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  ik_actions_launch(ik_of(h, *c, draw, actions), (hipStream_t)stream);
  return launched(h);
}

int urgym_controller_control(void* handle, const urgym_reach_controller* c, uint64_t first_draw, int num_steps, const urgym_trajectory* traj_or_NULL, void* stream) {
  const char* who = "urgym_controller_control";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_controller(h, c, who)) return rc;
  if (!h->observed) return fail_in(h, URGYM_ERR_STATE, who, "nothing has been observed yet: urgym_reset() or urgym_refresh() first");
  if (int rc = check_record(h, 0, num_steps, traj_or_NULL, who)) return rc;
  if (!traj_or_NULL || !traj_or_NULL->action)
    return fail_in(h, URGYM_ERR_ARG, who, "traj->action is null: the library allocates nothing, the action rows are the trajectory's");
  if (int rc = check_draw(h, first_draw, num_steps, who)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = controller_control(h, *c, first_draw, num_steps, *traj_or_NULL, (hipStream_t)stream)) return rc;
  return launched(h);
}

int urgym_controller_collect(void* handle, const urgym_reach_controller* c, uint64_t first_draw, int num_steps, const urgym_replay_ring* ring, int first_slot, void* stream) {
  const char* who = "urgym_controller_collect";
  Handle* h = (Handle*)handle;
  if (!h) return fail(nullptr, URGYM_ERR_ARG, "null handle");
  if (int rc = check_controller(h, c, who)) return rc;
  if (!h->observed) return fail_in(h, URGYM_ERR_STATE, who, "nothing has been observed yet: urgym_reset() or urgym_refresh() first");
  if (int rc = check_ring(h, ring, first_slot, num_steps, who)) return rc;
  if (int rc = check_draw(h, first_draw, num_steps, who)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = controller_collect(h, *c, first_draw, num_steps, *ring, first_slot, (hipStream_t)stream)) return rc;
  return launched(h);
}

}  // extern "C"
