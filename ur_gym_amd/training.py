"""A small SAC learner on the device pieces: the call pattern of the reference's ``train.py:40-60`` (stable-baselines3
``SAC("MultiInputPolicy", env, gamma=0.95, batch_size=256).learn``) with collection, a' ~ pi(.|s'), the bootstrapped target and the
minibatch gather on the HIP kernels, and gradients and optimisers in torch autograd unless the options below move them to the device too.

    collect   replay.collect with the DeviceActor: uniform actions before ``learning_starts`` env steps, the sampled policy after.
    update    1. replay.sample_targets with the DeviceActor and the TARGET DeviceCritic: the batch, a', log pi(a'|s') and the
                 bootstrapped part of the target, r + gamma (1 - terminated) min_i Q_i'(s', a'), from three launches.  The entropy
                 coefficient is a torch parameter; handing it to the kernel as a number would need a host synchronisation, so the
                 kernel is given ent_coef = 0 and the entropy term, -gamma (1 - terminated) alpha log pi(a'|s'), is added in torch.
              2. critic, actor and entropy-coefficient losses as SB3's SAC.train states them; one Adam step each.
              3. DeviceActor.load_parameters(the torch actor's parameters): one launch.
              4. target.load_parameters(the torch critic's parameters, tau): one launch, the Polyak update while it packs.
    With ``device_action_gradient=True`` the actor loss does not run the torch critic a second time: an ONLINE DeviceCritic is reloaded
    after the critic's Adam step (tau = 1) and one launch of the gradient kernel gives g = d min_i Q_i / d a and q_min at the policy's
    action; ``(ent_coef * log_prob - (action_pi * g).sum(1)).mean()`` has the actor loss's gradient with respect to the actor.
    With ``device_critic_gradient=True`` the critic loss does not run the torch critic either: the online DeviceCritic (shared with the
    option above) holds the torch critic's parameters when ``update`` starts, ``env.critic_parameter_gradients(target=y, scale=1/M)``
    writes d loss / d parameters into preallocated tensors that ARE the parameters' ``.grad``, the loss value is formed from the
    returned q, Adam steps, and the online critic is reloaded.
    With ``device_actor_gradient=True`` (it needs ``device_action_gradient=True``) the torch actor does not run at all: the DeviceActor
    draws action_pi and log_prob on the batch rows (``policy_actions(sample=, rows=)`` with draw | 2^63, apart from the draw
    ``sample_targets`` takes for a' on the same row indices), and after the critic step ONE ``env.actor_parameter_gradients`` call in
    the SAMPLE form, d_action = -g / M and d_log_prob = ent_coef / M, writes d loss / d parameters into preallocated tensors that ARE
    the actor parameters' ``.grad``.  No ``torch.Generator`` is drawn from, and nothing of ``update`` goes through torch autograd but
    the entropy coefficient's scalar loss.
    With ``device_optimizer=True`` (it needs ``device_critic_gradient=True`` and ``device_actor_gradient=True``, so that every
    ``.grad`` is a tensor the kernels wrote) the two Adam steps and the three reloads are two launches: ``critic_opt.step()``,
    ``online.load_parameters`` and the final ``target.load_parameters`` become one ``env.critic_adam_step(target=self.target, tau=)``,
    ``actor_opt.step()`` and ``device_actor.load_parameters`` one ``env.actor_adam_step``.  ``exp_avg`` and ``exp_avg_sq`` are zero
    tensors of the learner's, a Python int counts the steps, and the torch optimisers of the actor and the critic are not stepped (the
    entropy coefficient's stays in torch).  The Polyak blend of the target thereby moves from the end of ``update`` to the critic's
    step; in stream order that is equivalent, because nothing between the two places reads the target: it is read only by the NEXT
    update's ``sample_targets``.
    With ``device_entropy=True`` (it needs ``device_optimizer=True``) no torch operation is left in ``update`` but allocations and
    views: ``env.entropy_step`` (one launch) forms alpha = exp(log_ent_coef), y = target - gamma (1 - terminated) alpha log pi(a'|s')
    into a preallocated tensor, d_log_prob = alpha / M, the temperature loss, and steps ``log_ent_coef`` -- the same (1,) tensor,
    written by the kernel -- with Adam moments of the learner's; ``env.policy_terms`` (one launch, after the action gradient) forms
    d_action = -g / M and the critic's and the actor's loss values.  ``update`` is then thirteen launches: ``sample_targets`` (3),
    ``policy_actions``, ``entropy_step``, ``critic_parameter_gradients(target=y)`` (2), ``critic_adam_step``,
    ``critic_action_gradient``, ``policy_terms``, ``actor_parameter_gradients`` (2), ``actor_adam_step``.  ``ent_opt`` is not stepped,
    nothing goes through autograd, the losses are 0-dim views of preallocated tensors, and ``self.last_update`` keeps references
    (no copies) to the ``log_prob``, ``y``, ``q``, ``q_min`` and ``dqmin_da`` the update used.  Every float of it is stated in
    include/urgym.h.
    With ``n_steps`` > 1 (it needs ``device_entropy=True``; SB3's ``n_steps=``) the target is a multi-step return: the gather walks up
    to ``n_steps`` consecutive steps of the drawn env and stops at an episode's end (``DeviceReplay.sample_targets(n_steps=)``,
    urgym_replay_sample_nstep), the third launch writes min_i Q_i'(s', a') alone, and ``env.entropy_step_nstep`` forms
    y = R + gamma^m (1 - terminated) (min Q' - alpha log pi(a'|s')) from the row's own discount: still thirteen launches.
    ``n_steps`` = 1, the default, makes exactly the calls above.
    With ``max_grad_norm=X`` (it needs ``device_entropy=True``) each of the two Adam steps is preceded by ONE launch that reduces the
    global norm of its gradients on the device and leaves the clip coefficient there (``env.critic_gradient_norm``,
    ``env.actor_gradient_norm``), and the step multiplies each gradient element by it as it reads it (``scale=``): fifteen launches.
    The ``.grad`` tensors are not written, the temperature's scalar step is not clipped.  ``None``, the default, makes exactly the
    calls above.
    With ``normalize=True`` (it needs ``device_entropy=True``; SB3's ``VecNormalize``) the learner owns an
    ``evaluation.DeviceNormalizer`` (``self.normalizer``): ``collect`` runs the actor on rows normalized with the running statistics
    (one more launch per step; the ring keeps the raw rows) and folds the collected slots into them afterwards (two launches), and
    ``update`` normalizes the gathered minibatch in place right after the gather (``env.norm_batch``: fourteen launches, sixteen with
    clipping).  ``self.normalizer.training = False`` freezes the statistics.  ``False``, the default, makes exactly the calls above.
    With ``collect(planner=)`` (an ``evaluation.DeviceMPPI`` on the learner's env) the collecting policy is the MPPI
    planner instead of the sampled actor: every step is planned (urgym_mppi_collect), the executed action is the plan's first action plus
    ``explore_sigma`` times exploration noise, and the transitions land in the same ring slots, so ``update`` trains on them as they stand
    (SAC is off-policy); ``sync_planner`` puts the planner's actor and critic on the learner's current parameters.  Not with ``normalize``.
    ``train(planner=)`` runs that loop -- the planned collection, the updates, ``sync_planner`` -- inside the one native call
    (urgym_sac_train_planned, urgym_sac_train_tempered for a planner made with ``ess_target=``, urgym_sac_train_colored for one made with
    ``noise_beta=``; DESIGN.md sections 30 to 32), and with
    ``plan_stats=True`` keeps a record of how the plans went beside every
    record of the monitor.
    With ``bc_weight=X`` (it needs ``device_entropy=True``) the policy loss also imitates the action the ring holds:
    ``env.policy_terms`` becomes ``env.policy_terms_cloned`` on ``batch["actions"]`` -- ONE launch in its place, so the counts above
    stand -- which adds ``X' (action_pi - action) / M`` to d_action on the rows it clones, X' = X or, with ``bc_scale_by_q``, X times the
    mean |min Q| (TD3+BC's normalisation), the rows being all of them or, with ``bc_q_filter``, those where the critics rate the ring's
    action above the policy's own.  ``None``, the default, makes exactly the calls above.
    With ``bc_advantage_temperature=T`` (it needs ``bc_weight``, and not ``bc_q_filter``) that launch is
    ``env.policy_terms_weighted``: every row is cloned with the weight exp(A / T) normalised to mean 1 over the batch, A the critics'
    advantage of the ring's action over the policy's own, capped at ``bc_advantage_max_weight``; ``last_update`` and ``train``'s result
    gain ``adv_ess``, ``adv_max`` and ``adv_clipped``.  ``None``, the default, makes exactly the calls above.
    None of them synchronises with the host.  ``train`` runs the whole loop in one native call and, given an
    ``evaluation.DeviceEvaluation``, the reference's EvalCallback inside it: evaluations of the deterministic policy at a fixed interval of
    updates, their statistics as records on the device, and the best actor's tensors, which ``DeviceEvaluation.save_best`` writes as an
    ``.npz`` ``DeviceActor.load`` reads.  Given an ``evaluation.DeviceMonitor``, ``collect`` and ``train`` also keep the reference's
    ``Monitor`` (train.py:52) on the device: the return, the length and the success of the episodes the collecting policy finishes, as
    records of the training curve (SB3's rollout/ep_rew_mean, ep_len_mean and success_rate); nothing else is logged.
    ``save`` / ``load`` write and read the WHOLE run -- the parameters, the target critic (through the unpack kernel: it exists only
    packed), every Adam moment, the entropy coefficient, the counters and, handed in, the replay ring, the environment, the monitor and
    the evaluation -- so that a run rebuilt in fresh objects continues bit for bit; ``load_parameters`` is the
    reference's ``SAC.load`` then ``learn`` (train.py:31-36) from plain parameter files.  ``DeviceEvaluation.save_best`` still writes the
    best actor alone; tools/train_sac.py runs all of it.
"""
import numpy as np
import torch
from torch import nn

from .evaluation import ACTOR_ARRAYS, CRITIC_ARRAYS, LOG_STD_ARRAYS, LOG_STD_MAX, LOG_STD_MIN, DeviceActor, DeviceCritic

# SB3's SAC defaults where train.py does not set them (tests/golden/critics/sac_hyperparameters.json has the checkpoints' gamma, tau)
SAC_DEFAULTS = dict(gamma=0.95, tau=0.005, learning_rate=1e-4, batch_size=256, learning_starts=100, hidden_width=256, target_entropy=-6.0,
                    ent_coef_init=1.0, device_action_gradient=False, device_critic_gradient=False,
                    device_actor_gradient=False, device_optimizer=False, device_entropy=False, n_steps=1)
# Prioritized replay: the options of SACLearner(prioritized=True).  Kept apart from SAC_DEFAULTS: a run without
# priorities holds none of them in its checkpoint.  beta of the update at Adam step t is evaluation.per_beta(per_beta, t, per_beta_steps).
PER_DEFAULTS = dict(prioritized=False, per_beta=0.4, per_beta_steps=100000)
# Hindsight experience replay: the options of SACLearner(hindsight=True), SB3's HerReplayBuffer arguments.  Kept
# apart like PER_DEFAULTS: a run without hindsight saves none of them, so its checkpoint is what it was before the option existed.
HER_DEFAULTS = dict(hindsight=False, her_n_sampled_goal=4, her_strategy="future")
# Gradient-norm clipping: SACLearner(max_grad_norm=X) clips the critics' and the actor's gradients by their global
# norm, torch.nn.utils.clip_grad_norm_'s idiom on the device.  SB3's SAC does not clip; None, the default, is the learner as it was.  Kept
# apart like the two above: a run without it saves no new key.
CLIP_DEFAULTS = dict(max_grad_norm=None)
# Running observation and reward normalization: SACLearner(normalize=True) is SB3's VecNormalize on the device, with
# its defaults.  Kept apart like the three above: a run without it saves none of these, and no statistics.
NORM_DEFAULTS = dict(normalize=False, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, norm_epsilon=1e-8)
# Behaviour cloning in the policy loss: SACLearner(bc_weight=X) pulls the policy's action towards the ring's, with
# TD3+BC's normalisation by the mean |Q| (bc_scale_by_q) and the Q-filter (bc_q_filter).  None, the default, is the learner as it was.
# Kept apart like the four above: a run without it saves none of the three.
BC_DEFAULTS = dict(bc_weight=None, bc_scale_by_q=False, bc_q_filter=False)
# The demonstration ring: SACLearner(demonstrations=replay_d, demo_batch_size=D) draws the first D rows of every
# minibatch from a second ring that collection never overwrites; with bc_demo_only the cloning term applies to those rows only.  None,
# the default, is the learner as it was; demo_batch_size=0 takes the new calls and leaves the same bits.  Kept apart like the five above:
# a run without it saves neither key.
DEMO_DEFAULTS = dict(demo_batch_size=None, bc_demo_only=False)
# Advantage-weighted cloning: SACLearner(bc_weight=X, bc_advantage_temperature=T) weights every cloned row by
# exp(advantage / T), normalised over the batch and capped at bc_advantage_max_weight (None: no cap) -- AWAC's weight, the soft
# alternative to bc_q_filter.  None, the default, is the learner as it was.  Kept apart like the six above: a run without it saves neither.
ADV_DEFAULTS = dict(bc_advantage_temperature=None, bc_advantage_max_weight=None)


def _mlp(n_in, hidden, n_out=None):
    layers = [nn.Linear(n_in, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU()]
    if n_out is not None:
        layers.append(nn.Linear(hidden, n_out))
    return nn.Sequential(*layers)


class TorchActor(nn.Module):
    """SB3's SAC actor: latent_pi = Linear-ReLU-Linear-ReLU, mu and log_std heads, squashed diagonal Gaussian."""

    def __init__(self, in_features, hidden):
        super().__init__()
        self.latent_pi, self.mu, self.log_std = _mlp(in_features, hidden), nn.Linear(hidden, 6), nn.Linear(hidden, 6)

    def tensors(self):
        """The parameters under the names DeviceActor takes (ACTOR_ARRAYS + LOG_STD_ARRAYS), as they lie."""
        p = (self.latent_pi[0].weight, self.latent_pi[0].bias, self.latent_pi[2].weight, self.latent_pi[2].bias, self.mu.weight, self.mu.bias,
             self.log_std.weight, self.log_std.bias)
        return dict(zip(ACTOR_ARRAYS + LOG_STD_ARRAYS, p))

    def sample(self, x, eps):
        """(action, log_prob) of tanh(mu + exp(log_std) eps), reparameterised; the density as include/urgym.h states it."""
        h = self.latent_pi(x)
        mu, log_std = self.mu(h), self.log_std(h).clamp(LOG_STD_MIN, LOG_STD_MAX)
        action = torch.tanh(mu + log_std.exp() * eps)
        log_prob = (-0.5 * eps * eps - log_std - 0.5 * np.log(2 * np.pi)).sum(1) - torch.log(1.0 - action * action + 1e-6).sum(1)
        return action, log_prob


class TorchTwinCritic(nn.Module):
    """SB3's ContinuousCritic with two Q-networks on cat([features, action])."""

    def __init__(self, in_features, hidden):
        super().__init__()
        self.qf = nn.ModuleList([_mlp(in_features, hidden, 1) for _ in range(2)])

    def tensors(self):
        """The parameters of both networks under CRITIC_ARRAYS, as they lie."""
        return [dict(zip(CRITIC_ARRAYS, (q[0].weight, q[0].bias, q[2].weight, q[2].bias, q[4].weight, q[4].bias))) for q in self.qf]

    def forward(self, x, action):
        xa = torch.cat([x, action], dim=1)
        return self.qf[0](xa)[:, 0], self.qf[1](xa)[:, 0]


def _features(rows):
    return torch.cat([rows["achieved_goal"], rows["desired_goal"], rows["observation"]], dim=1)


def host_arrays(tensors):
    """A dict (or a list of dicts) of tensors as numpy arrays: what DeviceActor / DeviceCritic are created from.  Synchronises."""
    if isinstance(tensors, dict):
        return {k: v.detach().cpu().numpy().copy() for k, v in tensors.items()}
    return [host_arrays(t) for t in tensors]


def _optimizer_to_host(sd):
    """A ``torch.optim`` state dict as a checkpoint tree: tensors as numpy arrays, the parameter indices as strings."""
    state = {str(i): {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in s.items()} for i, s in sd["state"].items()}
    return dict(state=state, param_groups=[{k: (list(v) if isinstance(v, tuple) else v) for k, v in g.items()} for g in sd["param_groups"]])


def _optimizer_from_host(tree, opt, device):
    """The inverse of ``_optimizer_to_host`` for ``opt.load_state_dict``: every tensor goes where `opt` keeps its like (the step
    count on the host, the moments on `device`).  The hyperparameters of the parameter groups stay `opt`'s own, learning rate included."""
    here = opt.state_dict()
    if [len(g["params"]) for g in tree["param_groups"]] != [len(g["params"]) for g in here["param_groups"]]:
        raise ValueError("load_state_dict: the optimiser state is of other parameter groups")
    state = {}
    for i, s in tree["state"].items():
        state[int(i)] = {k: (torch.from_numpy(np.array(v)).to("cpu" if k == "step" else device) if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    return dict(state=state, param_groups=here["param_groups"])


class SACLearner:
    """Torch modules for the actor and the twin critic with Adam on each and on ``log_ent_coef``; a DeviceActor that follows the
    torch actor and a target DeviceCritic that follows the torch critic by Polyak averaging.  `env`: a UR5ReachVectorEnv with
    auto_reset.  Keyword arguments override SAC_DEFAULTS and PER_DEFAULTS: ``prioritized=True`` (with ``per_beta``, ``per_beta_steps``; needs
    all five ``device_*`` options and a ``DevicePrioritizedReplay``) draws each minibatch in proportion to the transitions' priorities and
    weights the critics' gradient by the importance weights; not together with ``n_steps`` > 1.  ``hindsight=True``
    (HER_DEFAULTS: ``her_n_sampled_goal``, ``her_strategy`` "future" or "final"; needs ``device_entropy=True``) relabels the goals of each
    minibatch in the gather (``DeviceReplay.sample_hindsight``); not together with ``n_steps`` > 1 or ``prioritized``.
    ``max_grad_norm=X`` (CLIP_DEFAULTS; needs ``device_entropy=True``) clips the critics' and the actor's gradients by their global norm on
    the device, inside the Adam steps; with any of the options above.

    ``demonstrations=replay_d, demo_batch_size=D`` (DEMO_DEFAULTS; needs ``device_entropy=True``): `replay_d` is a
    ``DeviceReplay`` of ANOTHER env of the same kind, with any env count, filled beforehand (by a planner, say) and never written by this
    learner; rows 0 .. D - 1 of every minibatch come from it (``DeviceReplay.sample_targets(demonstrations=)``, one mixed gather launch),
    the rest from the learner's own ring, in ``update`` and ``train`` alike.  With ``bc_demo_only=True`` (it needs ``bc_weight``) only those
    rows can be cloned (``env.policy_terms_cloned_masked``).  The learner keeps passing ``bc_scale = 1 / M``, not 1 / D, so a weight means
    the same at every demonstration share.  ``demo_batch_size=0`` goes through the new calls and leaves the bits of a learner without the
    option.  Not together with ``n_steps`` > 1, ``prioritized`` or ``hindsight``."""

    def __init__(self, env, seed=0, demonstrations=None, **overrides):
        unknown = [k for k in overrides if k not in SAC_DEFAULTS and k not in PER_DEFAULTS and k not in HER_DEFAULTS and k not in CLIP_DEFAULTS and k not in NORM_DEFAULTS
                   and k not in BC_DEFAULTS and k not in DEMO_DEFAULTS and k not in ADV_DEFAULTS]
        if unknown:
            raise TypeError(f"unknown hyperparameters {unknown}; available: "
                            f"{sorted(SAC_DEFAULTS) + sorted(PER_DEFAULTS) + sorted(HER_DEFAULTS) + sorted(CLIP_DEFAULTS) + sorted(NORM_DEFAULTS) + sorted(BC_DEFAULTS) + sorted(DEMO_DEFAULTS) + sorted(ADV_DEFAULTS)}")
        hp = dict(SAC_DEFAULTS, **PER_DEFAULTS, **HER_DEFAULTS, **CLIP_DEFAULTS, **NORM_DEFAULTS, **BC_DEFAULTS, **DEMO_DEFAULTS, **ADV_DEFAULTS)
        hp.update(overrides)
        if hp["bc_advantage_temperature"] is None:
            if hp["bc_advantage_max_weight"] is not None:
                raise ValueError("bc_advantage_max_weight qualifies bc_advantage_temperature and needs it")
        else:
            with np.errstate(over="ignore"):
                T, cap = hp["bc_advantage_temperature"], hp["bc_advantage_max_weight"]
                ok = not isinstance(T, bool) and isinstance(T, (int, float, np.integer, np.floating)) and bool(np.isfinite(np.float32(T))) and float(np.float32(T)) > 0.0
                if not ok:
                    raise ValueError(f"bc_advantage_temperature must be None or a number that is finite and > 0 in float32, got {T!r}")
                ok = cap is None or (not isinstance(cap, bool) and isinstance(cap, (int, float, np.integer, np.floating)) and float(np.float32(cap)) > 0.0)
                if not ok:
                    raise ValueError(f"bc_advantage_max_weight must be None or a number > 0 in float32, got {cap!r}")
            if hp["bc_weight"] is None:
                raise ValueError("bc_advantage_temperature needs bc_weight (it weights the cloning term)")
            if hp["bc_q_filter"] is True:
                raise ValueError("bc_advantage_temperature together with bc_q_filter is refused: the two gates are alternatives")
            hp["bc_advantage_temperature"], hp["bc_advantage_max_weight"] = float(T), None if cap is None else float(cap)
        if not isinstance(hp["bc_demo_only"], bool):
            raise ValueError(f"bc_demo_only must be True or False, got {hp['bc_demo_only']!r}")
        if hp["demo_batch_size"] is None:
            if demonstrations is not None:
                raise ValueError("demonstrations= needs demo_batch_size (the number of rows of every minibatch drawn from it; 0 is allowed)")
            if hp["bc_demo_only"]:
                raise ValueError("bc_demo_only qualifies demo_batch_size and needs it")
        else:
            D = hp["demo_batch_size"]
            if isinstance(D, bool) or not isinstance(D, (int, np.integer)) or not 0 <= int(D) <= int(hp["batch_size"]):
                raise ValueError(f"demo_batch_size must be None or an integer in [0, batch_size = {hp['batch_size']}], got {D!r}")
            hp["demo_batch_size"] = int(D)
            if not hp["device_entropy"]:
                raise ValueError("demo_batch_size needs device_entropy=True (the mixed minibatch is gathered and used by the device's launches)")
            if hp["bc_demo_only"] and hp["bc_weight"] is None:
                raise ValueError("bc_demo_only needs bc_weight (it restricts the cloning term to the demonstration rows)")
            if hp["prioritized"] is True or hp["hindsight"] is True or (not isinstance(hp["n_steps"], bool) and hp["n_steps"] != 1):
                raise ValueError("demo_batch_size with n_steps > 1, prioritized=True or hindsight=True is out of scope: each of the three has a gather of its own")
            if demonstrations is None:
                raise ValueError("demo_batch_size needs demonstrations= (a DeviceReplay of another env of the same kind)")
        for k in ("bc_scale_by_q", "bc_q_filter"):
            if not isinstance(hp[k], bool):
                raise ValueError(f"{k} must be True or False, got {hp[k]!r}")
        if hp["bc_weight"] is None:
            if hp["bc_scale_by_q"] or hp["bc_q_filter"]:
                raise ValueError("bc_scale_by_q and bc_q_filter qualify bc_weight and need it")
        else:
            with np.errstate(over="ignore"):
                weight = hp["bc_weight"]
                ok = not isinstance(weight, bool) and isinstance(weight, (int, float, np.integer, np.floating)) and bool(np.isfinite(np.float32(weight))) and float(np.float32(weight)) >= 0.0
            if not ok:
                raise ValueError(f"bc_weight must be None or a number that is finite in float32 and >= 0, got {hp['bc_weight']!r}")
            if not hp["device_entropy"]:
                raise ValueError("bc_weight needs device_entropy=True (the cloning term is added to the policy's upstream gradient by the device's policy terms)")
            hp["bc_weight"] = float(weight)
        if not isinstance(hp["normalize"], bool):
            raise ValueError(f"normalize must be True or False, got {hp['normalize']!r}")
        if hp["normalize"]:
            from .evaluation import DeviceNormalizer

            if not hp["device_entropy"]:
                raise ValueError("normalize=True needs device_entropy=True (the collecting actor and the update read the normalized rows between the device's launches)")
            DeviceNormalizer.check_options(gamma=hp["gamma"], norm_obs=hp["norm_obs"], norm_reward=hp["norm_reward"], clip_obs=hp["clip_obs"],
                                           clip_reward=hp["clip_reward"], epsilon=hp["norm_epsilon"])
        if hp["max_grad_norm"] is not None:
            with np.errstate(over="ignore"):
                bound = hp["max_grad_norm"]
                ok = not isinstance(bound, bool) and isinstance(bound, (int, float, np.integer, np.floating)) and bool(np.isfinite(np.float32(bound))) and float(np.float32(bound)) > 0.0
            if not ok:
                raise ValueError(f"max_grad_norm must be None or a positive number that is finite in float32, got {hp['max_grad_norm']!r}")
            if not hp["device_entropy"]:
                raise ValueError("max_grad_norm needs device_entropy=True (the norm is reduced and the clip coefficient applied between the device's launches; "
                                 "clipping the .grad tensors from torch would bring host-visible norms back into the update)")
            hp["max_grad_norm"] = float(bound)
        if not isinstance(hp["hindsight"], bool):
            raise ValueError(f"hindsight must be True or False, got {hp['hindsight']!r}")
        if hp["hindsight"]:
            from .evaluation import relabel_threshold

            if not hp["device_entropy"]:
                raise ValueError("hindsight=True needs device_entropy=True (the relabelled minibatch is gathered and used by the device's launches)")
            if hp["prioritized"] is True or (not isinstance(hp["n_steps"], bool) and hp["n_steps"] != 1):
                raise ValueError("hindsight=True with n_steps > 1 or prioritized=True is out of scope: each of the three has a gather of its own")
            if hp["her_strategy"] not in ("future", "final"):
                raise ValueError(f"her_strategy must be 'future' or 'final', got {hp['her_strategy']!r} ('own' is a diagnostic of the gather, SB3's 'episode' is out of scope)")
            if relabel_threshold(hp["her_n_sampled_goal"]) == 0:
                raise ValueError("her_n_sampled_goal must be a positive integer")
            if env is not None and int(env.cfg.max_episode_steps) > 256:
                raise ValueError(f"hindsight=True needs max_episode_steps <= 256 (the episode window's horizon), got {int(env.cfg.max_episode_steps)}")
        if not isinstance(hp["prioritized"], bool):
            raise ValueError(f"prioritized must be True or False, got {hp['prioritized']!r}")
        if hp["prioritized"]:
            if not hp["device_entropy"]:
                raise ValueError("prioritized=True needs all five device_* options (the weights and the new priorities are formed between the device's launches)")
            if int(hp["n_steps"]) != 1:
                raise ValueError("prioritized=True with n_steps > 1 is out of scope: the multi-step gather draws its own indices")
            if not 0.0 <= float(hp["per_beta"]) <= 1.0:
                raise ValueError(f"per_beta must be in [0, 1], got {hp['per_beta']!r}")
            steps = hp["per_beta_steps"]
            if isinstance(steps, bool) or int(steps) != steps or int(steps) < 1:
                raise ValueError(f"per_beta_steps must be a positive integer, got {steps!r}")
        n_steps = hp["n_steps"]
        if isinstance(n_steps, bool) or int(n_steps) != n_steps or not 1 <= int(n_steps) <= 32:
            raise ValueError(f"n_steps must be an integer in [1, 32], got {n_steps!r}")
        if int(n_steps) > 1 and not hp["device_entropy"]:
            raise ValueError("n_steps > 1 needs device_entropy=True (the multi-step target is formed by the device's entropy step)")
        self.env, self.hp, self.seed = env, hp, int(seed)
        n_in, H, dev = env.obs_dim + 2 * env.goal_dim, int(hp["hidden_width"]), env.device
        torch.manual_seed(self.seed)
        self.actor = TorchActor(n_in, H).to(dev)
        self.critic = TorchTwinCritic(n_in + 6, H).to(dev)
        self.log_ent_coef = torch.full((1,), float(np.log(hp["ent_coef_init"])), device=dev, requires_grad=True)
        lr = hp["learning_rate"]
        self.actor_opt = torch.optim.Adam(self.actor.parameters(), lr=lr)
        self.critic_opt = torch.optim.Adam(self.critic.parameters(), lr=lr)
        self.ent_opt = torch.optim.Adam([self.log_ent_coef], lr=lr)
        self.noise = torch.Generator(device=dev)
        self.noise.manual_seed(self.seed)
        self.device_actor = DeviceActor(host_arrays(self.actor.tensors()), env)
        self.target = DeviceCritic(host_arrays(self.critic.tensors()), env)  # starts as a copy of the online critic
        # the online critic on the device, only where the actor loss takes its action gradient from the kernel
        self.online = DeviceCritic(host_arrays(self.critic.tensors()), env) if hp["device_action_gradient"] or hp["device_critic_gradient"] else None
        # with device_critic_gradient the critic parameters' .grad are tensors of the learner's, written by the gradient kernels
        self.critic_grads = self.critic_workspace = None
        if hp["device_critic_gradient"]:
            self.critic_grads = [{k: torch.zeros_like(p) for k, p in w.items()} for w in self.critic.tensors()]
            for w, g in zip(self.critic.tensors(), self.critic_grads):
                for k, p in w.items():
                    p.grad = g[k]
            self.critic_workspace = env.critic_gradient_workspace(self.online, int(hp["batch_size"]))
        # with device_actor_gradient the actor parameters' .grad are tensors of the learner's as well, and so are the upstream gradients
        self.actor_grads = self.actor_workspace = self.actor_d_action = self.actor_d_log_prob = None
        if hp["device_actor_gradient"]:
            if not hp["device_action_gradient"]:
                raise ValueError("device_actor_gradient needs device_action_gradient=True (the upstream gradient is the critics' d min Q / da)")
            M = int(hp["batch_size"])
            self.actor_grads = {k: torch.zeros_like(p) for k, p in self.actor.tensors().items()}
            for k, p in self.actor.tensors().items():
                p.grad = self.actor_grads[k]
            self.actor_workspace = env.actor_gradient_workspace(self.device_actor, M)
            self.actor_d_action = torch.zeros((M, 6), dtype=torch.float32, device=dev)
            self.actor_d_log_prob = torch.zeros((M,), dtype=torch.float32, device=dev)
        # with device_optimizer Adam's moments are tensors of the learner's too, and the step kernels take the place of the torch optimisers
        self.adam_state = None
        if hp["device_optimizer"]:
            if not (hp["device_critic_gradient"] and hp["device_actor_gradient"]):
                raise ValueError("device_optimizer needs device_critic_gradient=True and device_actor_gradient=True (the step kernels read the .grad tensors the gradient kernels write)")
            zeros = lambda w: {k: torch.zeros_like(p) for k, p in w.items()}  # noqa: E731
            self.adam_state = dict(step=0, betas=(0.9, 0.999), eps=1e-8,  # torch.optim.Adam's defaults, as the optimisers above
                                   actor=(zeros(self.actor.tensors()), zeros(self.actor.tensors())),
                                   critic=([zeros(w) for w in self.critic.tensors()], [zeros(w) for w in self.critic.tensors()]))
        # with device_entropy the entropy coefficient's step, its uses and the loss values are two launches: the moments of log_ent_coef,
        # alpha, y and the three losses are tensors of the learner's
        self.entropy_state = self.last_update = None
        if hp["device_entropy"]:
            if not hp["device_optimizer"]:
                raise ValueError("device_entropy needs device_optimizer=True (the entropy step shares its step count, and nothing else of update is left in torch)")
            scalar = lambda: torch.zeros((1,), dtype=torch.float32, device=dev)  # noqa: E731
            es = dict(exp_avg=scalar(), exp_avg_sq=scalar(), ent_coef=scalar(), y=torch.zeros((int(hp["batch_size"]),), dtype=torch.float32, device=dev),
                      critic_loss=scalar(), actor_loss=scalar(), ent_coef_loss=scalar())
            es["losses"] = {k: es[k][0] for k in ("critic_loss", "actor_loss", "ent_coef_loss")}  # 0-dim views, made once
            self.entropy_state = es
        # with max_grad_norm the two norms and the two clip coefficients of the running update are tensors of the learner's; never saved
        self.clip_state = None
        if hp["max_grad_norm"] is not None:
            scale = torch.zeros((2,), dtype=torch.float32, device=dev)  # the critics' coefficient, then the actor's
            self.clip_state = dict(scale=scale, critic_scale=scale[0:1], actor_scale=scale[1:2], critic_grad_norm=torch.zeros((1,), dtype=torch.float32, device=dev),
                                   actor_grad_norm=torch.zeros((1,), dtype=torch.float32, device=dev))
        # with bc_weight the cloning loss, the weight used and the number of cloned rows of the running update are tensors of the learner's; never saved
        self.bc_state = None
        if hp["bc_weight"] is not None:
            self.bc_state = dict(bc_loss=torch.zeros((1,), dtype=torch.float32, device=dev), bc_weight=torch.zeros((1,), dtype=torch.float32, device=dev),
                                 bc_rows=torch.zeros((1,), dtype=torch.int32, device=dev))
        # with bc_advantage_temperature the weights' effective sample size, the largest weight and the capped rows of the running update; never saved
        self.adv_state = None
        if hp["bc_advantage_temperature"] is not None:
            self.adv_state = dict(adv_ess=torch.zeros((1,), dtype=torch.float32, device=dev), adv_max=torch.zeros((1,), dtype=torch.float32, device=dev),
                                  adv_clipped=torch.zeros((1,), dtype=torch.int32, device=dev))
        # with normalize the running statistics, the actor's scratch rows and the fold's workspace are the normalizer's
        self.normalizer = None
        if hp["normalize"]:
            from .evaluation import DeviceNormalizer

            self.normalizer = DeviceNormalizer(env, gamma=hp["gamma"], norm_obs=hp["norm_obs"], norm_reward=hp["norm_reward"], clip_obs=hp["clip_obs"],
                                               clip_reward=hp["clip_reward"], epsilon=hp["norm_epsilon"])
        # with demo_batch_size the demonstration ring is the caller's; the gather's source bytes are a tensor of the learner's; never saved
        self.demonstrations = self.demo_source = None
        if hp["demo_batch_size"] is not None:
            env._demonstrations("SACLearner", demonstrations, hp["demo_batch_size"])  # another env of this kind and device, and not empty
            self.demonstrations = demonstrations
            self.demo_source = torch.zeros((int(hp["batch_size"]),), dtype=torch.uint8, device=dev)
        self._train = None  # the scratch and the checked struct of train(), per replay
        self.env_steps = 0  # per env; decides between the warm-up and the policy
        self.draw = 0       # draw index of the next collection pass

    def collect(self, replay, num_steps, monitor=None, planner=None, explore_sigma=0.0, controller=None):
        """`num_steps` env steps of all N envs into `replay`, with uniform actions before ``learning_starts`` env steps and the sampled
        policy afterwards (a call is one or the other: the mode is decided when it starts).  With `monitor` (an
        ``evaluation.DeviceMonitor``) the steps just collected are folded into its state: one more launch.  With ``normalize`` the actor
        reads normalized rows and the steps are folded into the statistics first (at most ``normalizer.fold_steps`` steps a call).

        With `planner` (an ``evaluation.DeviceMPPI`` on this learner's env) every step is planned instead
        (``replay.collect_planned``): ``learning_starts`` is not consulted, the planner's draw is ``self.draw``, and
        the executed action is the plan's plus `explore_sigma` times the exploration noise.  SAC is off-policy and trains on these
        transitions as they stand; ``sync_planner`` keeps the planner's actor and critic on this learner's parameters.  Not together
        with ``normalize``: the planner's actor and critic read raw rows.  Without `planner` the calls are those above.

        With `controller` (an ``evaluation.DeviceReachController`` on this learner's env) every step is the scripted reach controller's
        instead (``replay.collect_scripted``): as with a planner, ``learning_starts`` is not consulted, the draw is
        ``self.draw`` and `explore_sigma` scales the exploration noise; the ring holds raw rows, and with ``normalize`` the steps are folded
        into the statistics like any others.  Not together with `planner`."""
        if controller is not None:
            if planner is not None:
                raise ValueError("collect: controller= and planner= are alternatives")
            if getattr(controller, "env", None) is not self.env:
                raise ValueError("collect: the controller's env is not this learner's env (DeviceReachController(learner.env, ...))")
            if self.normalizer is not None and int(num_steps) > self.normalizer.fold_steps:
                raise ValueError(f"collect: with normalize at most fold_steps = {self.normalizer.fold_steps} steps a call, got {num_steps}")
            first = replay.cursor
            replay.collect_scripted(controller, num_steps, first_draw=self.draw, explore_sigma=explore_sigma)
            if self.normalizer is not None:
                self.normalizer.fold(replay, first, num_steps)
            if monitor is not None:
                monitor.fold(replay, first, num_steps)
            self.env_steps += int(num_steps)
            self.draw += int(num_steps)
            return
        if planner is not None:
            if self.normalizer is not None:
                raise ValueError("collect: planner= together with normalize=True is out of scope (the planner's actor and critic read raw rows, not normalized ones)")
            if getattr(planner, "env", None) is not self.env:
                raise ValueError("collect: the planner's source env is not this learner's env (DeviceMPPI(learner.env, ...))")
            first = replay.cursor
            replay.collect_planned(planner, num_steps, first_draw=self.draw, explore_sigma=explore_sigma)
            if monitor is not None:
                monitor.fold(replay, first, num_steps)
            self.env_steps += int(num_steps)
            self.draw += int(num_steps)
            return
        if explore_sigma:
            raise ValueError("collect: explore_sigma is the planner's (or the controller's) exploration noise and needs planner= or controller=")
        mode = "uniform" if self.env_steps * self.env.num_envs < self.hp["learning_starts"] else "gaussian"
        first = replay.cursor
        if self.normalizer is not None:
            if int(num_steps) > self.normalizer.fold_steps:
                raise ValueError(f"collect: with normalize at most fold_steps = {self.normalizer.fold_steps} steps a call, got {num_steps}")
            replay.collect(self.device_actor, num_steps, sample=dict(mode=mode, seed=self.seed, first_draw=self.draw), normalizer=self.normalizer)
            self.normalizer.fold(replay, first, num_steps)
        else:
            replay.collect(self.device_actor, num_steps, sample=dict(mode=mode, seed=self.seed, first_draw=self.draw))
        if monitor is not None:
            monitor.fold(replay, first, num_steps)
        self.env_steps += int(num_steps)
        self.draw += int(num_steps)

    def sync_planner(self, planner):
        """Puts `planner`'s actor and critic (an ``evaluation.DeviceMPPI`` made with ``actor=`` / ``critic=``) on this learner's current
        parameters: the actor from the torch actor's tensors (urgym_actor_load), the critic from the ONLINE critics with tau = 1
        (urgym_critic_load), one launch each on the planner's handle, nothing synchronised.  A part the planner does not have is skipped."""
        if planner.actor is not None:
            planner.actor.load_parameters(self.actor.tensors())
        if planner.critic is not None:
            planner.critic.load_parameters(self.critic.tensors(), tau=1.0)

    def update(self, replay, seed, draw):
        """One gradient step on a minibatch drawn with (seed, draw), then the two reloads.  Returns the three losses as device
        tensors (not synchronised)."""
        if self.entropy_state is not None:
            return self._update_on_device(replay, seed, draw)
        hp = self.hp
        gamma = float(hp["gamma"])
        if self.actor_grads is not None and not 0 <= int(draw) < 2 ** 63:
            raise ValueError("with device_actor_gradient the draw must be below 2**63 (its top bit marks the policy's own draw)")
        batch = replay.sample_targets(self.device_actor, self.target, hp["batch_size"], seed, draw, gamma, 0.0)
        x = _features(batch["observations"])
        with torch.no_grad():
            ent_coef = self.log_ent_coef.exp()
            discount = gamma * (~batch["terminated"]).to(torch.float32)
            y = batch["target"] - discount * ent_coef * batch["next_log_prob"]

        if self.actor_grads is None:
            eps = torch.randn((x.shape[0], 6), device=x.device, generator=self.noise)
            action_pi, log_prob = self.actor.sample(x, eps)
        else:
            # the DeviceActor holds the torch actor's parameters here (loaded at construction and at the end of every update)
            how = dict(mode="gaussian", seed=seed, first_draw=int(draw) | 1 << 63)
            action_pi, log_prob = self.env.policy_actions(self.device_actor, sample=how, rows=batch["observations"])

        ent_loss = -(self.log_ent_coef * (log_prob.detach() + hp["target_entropy"])).mean()
        self.ent_opt.zero_grad(set_to_none=True)
        ent_loss.backward()
        self.ent_opt.step()

        if self.critic_grads is None:
            q0, q1 = self.critic(x, batch["actions"])
            critic_loss = 0.5 * (((q0 - y) ** 2).mean() + ((q1 - y) ** 2).mean())
            self.critic_opt.zero_grad(set_to_none=True)
            critic_loss.backward()
            self.critic_opt.step()
        else:
            # the online DeviceCritic holds the torch critic's parameters here (loaded at construction and after every Adam step)
            got = self.env.critic_parameter_gradients(self.online, batch["actions"], target=y, scale=1.0 / x.shape[0], rows=batch["observations"],
                                                      out=self.critic_grads, workspace=self.critic_workspace)
            critic_loss = 0.5 * (((got["q"][0] - y) ** 2).mean() + ((got["q"][1] - y) ** 2).mean())
            if self.adam_state is None:
                self.critic_opt.step()  # on the .grad tensors the launches wrote
                self.online.load_parameters(self.critic.tensors(), tau=1.0)
            else:  # the step, the reload of the online critic and the target's Polyak update (read next by the next update) in one launch
                st = self.adam_state
                st["step"] += 1
                self.env.critic_adam_step(self.online, self.critic.tensors(), self.critic_grads, *st["critic"], lr=hp["learning_rate"],
                                          betas=st["betas"], eps=st["eps"], step=st["step"], target=self.target, tau=hp["tau"])

        if self.actor_grads is not None:
            M = x.shape[0]
            if self.critic_grads is None:
                self.online.load_parameters(self.critic.tensors(), tau=1.0)
            grad = self.env.critic_action_gradient(self.online, action_pi, rows=batch["observations"])
            torch.mul(grad["dqmin_da"], -1.0 / M, out=self.actor_d_action)
            self.actor_d_log_prob.copy_((ent_coef / M).expand(M))
            self.env.actor_parameter_gradients(self.device_actor, sample=how, rows=batch["observations"], d_action=self.actor_d_action,
                                               d_log_prob=self.actor_d_log_prob, out=self.actor_grads, workspace=self.actor_workspace)
            actor_loss = (ent_coef * log_prob - grad["q_min"]).mean()
            if self.adam_state is not None:
                st = self.adam_state
                self.env.actor_adam_step(self.device_actor, self.actor.tensors(), self.actor_grads, *st["actor"], lr=hp["learning_rate"],
                                         betas=st["betas"], eps=st["eps"], step=st["step"])
                return {"critic_loss": critic_loss.detach(), "actor_loss": actor_loss.detach(), "ent_coef_loss": ent_loss.detach()}
            self.actor_opt.step()  # on the .grad tensors the launches wrote
            self.device_actor.load_parameters(self.actor.tensors())
            self.target.load_parameters(self.critic.tensors(), tau=hp["tau"])
            return {"critic_loss": critic_loss.detach(), "actor_loss": actor_loss.detach(), "ent_coef_loss": ent_loss.detach()}

        self.actor_opt.zero_grad(set_to_none=True)
        if not hp["device_action_gradient"]:
            q_pi = torch.min(*self.critic(x, action_pi))
            actor_loss = (ent_coef * log_prob - q_pi).mean()
            actor_loss.backward()  # also fills the critic's gradients, which its next zero_grad discards
        else:
            if self.critic_grads is None:
                self.online.load_parameters(self.critic.tensors(), tau=1.0)
            grad = self.env.critic_action_gradient(self.online, action_pi.detach(), rows=batch["observations"])
            (ent_coef * log_prob - (action_pi * grad["dqmin_da"]).sum(1)).mean().backward()  # through the torch actor only
            actor_loss = (ent_coef * log_prob.detach() - grad["q_min"]).mean()
        self.actor_opt.step()

        self.device_actor.load_parameters(self.actor.tensors())
        self.target.load_parameters(self.critic.tensors(), tau=hp["tau"])
        return {"critic_loss": critic_loss.detach(), "actor_loss": actor_loss.detach(), "ent_coef_loss": ent_loss.detach()}

    def _update_on_device(self, replay, seed, draw):
        """``update`` with ``device_entropy``: thirteen launches of the library's and no torch operation but allocations and views."""
        hp, env, st, es = self.hp, self.env, self.adam_state, self.entropy_state
        if not 0 <= int(draw) < 2 ** 63:
            raise ValueError("with device_actor_gradient the draw must be below 2**63 (its top bit marks the policy's own draw)")
        M, gamma, n_steps = int(hp["batch_size"]), float(hp["gamma"]), int(hp["n_steps"])
        if hp.get("prioritized"):
            return self._update_prioritized(replay, seed, draw)
        her = dict(hindsight=dict(n_sampled_goal=hp["her_n_sampled_goal"], strategy=hp["her_strategy"])) if hp.get("hindsight") else {}
        norm = {} if self.normalizer is None else dict(normalizer=self.normalizer)
        demo = {} if self.demonstrations is None else dict(demonstrations=(self.demonstrations, hp["demo_batch_size"]))
        batch = replay.sample_targets(self.device_actor, self.target, M, seed, draw, gamma, 0.0, **({} if n_steps == 1 else dict(n_steps=n_steps)), **her, **norm, **demo)
        rows = batch["observations"]
        how = dict(mode="gaussian", seed=seed, first_draw=int(draw) | 1 << 63)
        action_pi, log_prob = env.policy_actions(self.device_actor, sample=how, rows=rows)
        st["step"] += 1
        adam = dict(lr=hp["learning_rate"], betas=st["betas"], eps=st["eps"], step=st["step"])
        # alpha of the old log_ent_coef, y, d_log_prob = alpha / M, the temperature loss and its Adam step
        if n_steps == 1:
            env.entropy_step((self.log_ent_coef, es["exp_avg"], es["exp_avg_sq"]), log_prob, hp["target_entropy"], ent_coef_out=es["ent_coef"],
                             loss_out=es["ent_coef_loss"], target=batch["target"], next_log_prob=batch["next_log_prob"], terminated=batch["terminated"],
                             gamma=gamma, y_out=es["y"], d_log_prob_out=self.actor_d_log_prob, scale=1.0 / M, **adam)
        else:
            env.entropy_step_nstep((self.log_ent_coef, es["exp_avg"], es["exp_avg_sq"]), log_prob, hp["target_entropy"], ent_coef_out=es["ent_coef"],
                                   loss_out=es["ent_coef_loss"], reward=batch["rewards"], q_min_next=batch["q_min_next"], discount=batch["discount"],
                                   next_log_prob=batch["next_log_prob"], terminated=batch["terminated"], y_out=es["y"],
                                   d_log_prob_out=self.actor_d_log_prob, scale=1.0 / M, **adam)
        got = env.critic_parameter_gradients(self.online, batch["actions"], target=es["y"], scale=1.0 / M, rows=rows, out=self.critic_grads,
                                             workspace=self.critic_workspace)
        env.critic_adam_step(self.online, self.critic.tensors(), self.critic_grads, *st["critic"], target=self.target, tau=hp["tau"], **adam,
                             **self._clip("critic"))
        grad = env.critic_action_gradient(self.online, action_pi, rows=rows)
        # d_action = -g / M and the critic's and the actor's loss values
        self._policy_terms(M, grad, got, log_prob, action_pi, batch["actions"], source=batch.get("source"))
        env.actor_parameter_gradients(self.device_actor, sample=how, rows=rows, d_action=self.actor_d_action, d_log_prob=self.actor_d_log_prob,
                                      out=self.actor_grads, workspace=self.actor_workspace)
        env.actor_adam_step(self.device_actor, self.actor.tensors(), self.actor_grads, *st["actor"], **adam, **self._clip("actor"))
        self.last_update = dict(log_prob=log_prob, y=es["y"], q=got["q"], q_min=grad["q_min"], dqmin_da=grad["dqmin_da"], **self._clip_record(), **self._bc_record(action_pi, batch["actions"]),
                                **({} if self.demonstrations is None else dict(source=batch["source"])))
        return dict(es["losses"])

    def _policy_terms(self, M, grad, got, log_prob, action_pi, actions, source=None):
        """d_action = -g / M and the critic's and the actor's loss values: ``env.policy_terms``, or with ``bc_weight`` the ONE launch of
        ``env.policy_terms_cloned`` in its place, which adds the cloning term on the rows it clones (`actions`: the ring's); with
        ``bc_demo_only`` that launch is ``env.policy_terms_cloned_masked``'s with the gather's `source` as the mask.  ``bc_scale`` stays
        1 / M whatever the demonstration share."""
        hp, es, bc = self.hp, self.entropy_state, self.bc_state
        common = dict(dqmin_da=grad["dqmin_da"], scale=-1.0 / M, d_action_out=self.actor_d_action, q=got["q"], y=es["y"], critic_loss_out=es["critic_loss"],
                      log_prob=log_prob, q_min=grad["q_min"], actor_loss_out=es["actor_loss"])
        if bc is None:
            self.env.policy_terms(es["ent_coef"], M, **common)
        elif self.adv_state is not None:  # the advantage weight in the place of the verdict: still ONE launch
            adv = self.adv_state
            self.env.policy_terms_weighted(
                es["ent_coef"], M, **common, **(dict(row_mask=source) if hp["bc_demo_only"] else {}), action_pi=action_pi, action_data=actions, weight=hp["bc_weight"],
                bc_scale=1.0 / M, scale_by_q=hp["bc_scale_by_q"], bc_loss_out=bc["bc_loss"], bc_weight_out=bc["bc_weight"], bc_rows_out=bc["bc_rows"],
                temperature=hp["bc_advantage_temperature"], max_weight=hp["bc_advantage_max_weight"], adv_ess_out=adv["adv_ess"], adv_max_out=adv["adv_max"],
                adv_clipped_out=adv["adv_clipped"])
        else:
            masked = dict(row_mask=source) if hp["bc_demo_only"] else {}
            (self.env.policy_terms_cloned_masked if masked else self.env.policy_terms_cloned)(
                es["ent_coef"], M, **common, **masked, action_pi=action_pi, action_data=actions, weight=hp["bc_weight"], bc_scale=1.0 / M, scale_by_q=hp["bc_scale_by_q"],
                q_filter=hp["bc_q_filter"], bc_loss_out=bc["bc_loss"], bc_weight_out=bc["bc_weight"], bc_rows_out=bc["bc_rows"])

    def _bc_record(self, action_pi, actions):
        """What ``last_update`` gains with ``bc_weight``: references to the cloning loss, the weight used and the number of cloned rows, and
        to the two actions the cloning term was formed from."""
        return {} if self.bc_state is None else dict(self.bc_state, **(self.adv_state or {}), action_pi=action_pi, action_data=actions)

    def _clip(self, which):
        """With ``max_grad_norm``: ONE launch reduces the global norm of the critics' (or the actor's) gradients into the learner's
        tensors; returns the ``scale=`` keyword of the step that follows.  Without it: nothing is launched, no keyword."""
        cs = self.clip_state
        if cs is None:
            return {}
        if which == "critic":
            self.env.critic_gradient_norm(self.online, self.critic_grads, self.hp["max_grad_norm"], norm_out=cs["critic_grad_norm"], scale_out=cs["critic_scale"],
                                          tensor_sums_out=False)
        else:
            self.env.actor_gradient_norm(self.device_actor, self.actor_grads, self.hp["max_grad_norm"], norm_out=cs["actor_grad_norm"], scale_out=cs["actor_scale"],
                                         tensor_sums_out=False)
        return dict(scale=cs[which + "_scale"])

    def _clip_record(self):
        """What ``last_update`` gains with ``max_grad_norm``: references to the two norms and the two coefficients of the update."""
        cs = self.clip_state
        return {} if cs is None else {k: cs[k] for k in ("critic_grad_norm", "actor_grad_norm", "critic_scale", "actor_scale")}

    def _update_prioritized(self, replay, seed, draw):
        """``_update_on_device`` on a ``DevicePrioritizedReplay``: the draw goes through the priority sums, and between the entropy step
        and the critics' gradients come the online critics' q on the batch rows (urgym_critic_evaluate) and urgym_per_terms -- the
        importance weights at ``per_beta`` of this Adam step, the weighted upstream gradient dq, the new priorities written back and
        the sums repaired.  Seventeen launches (nineteen above 1024 rows).  The critic loss reported stays the unweighted one."""
        from .evaluation import DevicePrioritizedReplay, per_beta

        if not isinstance(replay, DevicePrioritizedReplay):
            raise ValueError("prioritized=True needs a DevicePrioritizedReplay")
        hp, env, st, es = self.hp, self.env, self.adam_state, self.entropy_state
        M, gamma = int(hp["batch_size"]), float(hp["gamma"])
        batch = replay.sample_prioritized(M, seed, draw)
        if self.normalizer is not None:
            self.normalizer.normalize_batch(batch)
        rows, nxt = batch["observations"], batch["next_observations"]
        next_actions, next_log_prob = env.policy_actions(self.device_actor, sample=dict(mode="gaussian", seed=seed, first_draw=draw), rows=nxt)
        target = env.critic_values(self.target, next_actions, rows=nxt, reward=batch["rewards"], terminated=batch["terminated"], log_prob=next_log_prob,
                                   gamma=gamma, ent_coef=0.0)["target"]
        how = dict(mode="gaussian", seed=seed, first_draw=int(draw) | 1 << 63)
        action_pi, log_prob = env.policy_actions(self.device_actor, sample=how, rows=rows)
        st["step"] += 1
        adam = dict(lr=hp["learning_rate"], betas=st["betas"], eps=st["eps"], step=st["step"])
        env.entropy_step((self.log_ent_coef, es["exp_avg"], es["exp_avg_sq"]), log_prob, hp["target_entropy"], ent_coef_out=es["ent_coef"],
                         loss_out=es["ent_coef_loss"], target=target, next_log_prob=next_log_prob, terminated=batch["terminated"],
                         gamma=gamma, y_out=es["y"], d_log_prob_out=self.actor_d_log_prob, scale=1.0 / M, **adam)
        q = env.critic_values(self.online, batch["actions"], rows=rows)["q"]
        per = replay.terms(batch, q, es["y"], per_beta(hp["per_beta"], st["step"], hp["per_beta_steps"]), 1.0 / M)
        got = env.critic_parameter_gradients(self.online, batch["actions"], dq=per["dq"], rows=rows, out=self.critic_grads, workspace=self.critic_workspace)
        env.critic_adam_step(self.online, self.critic.tensors(), self.critic_grads, *st["critic"], target=self.target, tau=hp["tau"], **adam,
                             **self._clip("critic"))
        grad = env.critic_action_gradient(self.online, action_pi, rows=rows)
        self._policy_terms(M, grad, got, log_prob, action_pi, batch["actions"])
        env.actor_parameter_gradients(self.device_actor, sample=how, rows=rows, d_action=self.actor_d_action, d_log_prob=self.actor_d_log_prob,
                                      out=self.actor_grads, workspace=self.actor_workspace)
        env.actor_adam_step(self.device_actor, self.actor.tensors(), self.actor_grads, *st["actor"], **adam, **self._clip("actor"))
        self.last_update = dict(log_prob=log_prob, y=es["y"], q=got["q"], q_min=grad["q_min"], dqmin_da=grad["dqmin_da"], q_evaluated=q, index=batch["index"],
                                leaf=batch["leaf"], total=batch["total"], **per, **self._clip_record(), **self._bc_record(action_pi, batch["actions"]))
        return dict(es["losses"])

    def _train_binding(self, replay):
        """The scratch of ``train`` and the checked struct of the native call, made once per (learner, replay) pair."""
        if self._train is not None and self._train["replay"] is replay:
            return self._train
        from . import _abi
        from .vector_env import _TORCH_DTYPE

        hp, env, st, es = self.hp, self.env, self.adam_state, self.entropy_state
        M, dev = int(hp["batch_size"]), env.device
        batch = {name: torch.empty((M,) + tuple(shape(1, 1, env.obs_dim, env.goal_dim)[2:]), dtype=_TORCH_DTYPE[ct], device=dev)
                 for name, ct, shape, _ in _abi.REPLAY_RING_FIELDS}
        batch["index"] = torch.empty((M,), dtype=torch.int64, device=dev)
        scratch = {name: torch.zeros(shape(M), dtype=torch.float32, device=dev) for name, shape in _abi.SAC_LEARNER_SCRATCH}
        # the tensors update() already owns stay the ones both routes write
        scratch.update(y=es["y"], ent_coef=es["ent_coef"], d_action=self.actor_d_action, d_log_prob=self.actor_d_log_prob)
        binding = env.sac_learner(
            actor=self.device_actor, online=self.online, target=self.target, actor_params=self.actor.tensors(), actor_grads=self.actor_grads,
            actor_exp_avg=st["actor"][0], actor_exp_avg_sq=st["actor"][1], critic_params=self.critic.tensors(), critic_grads=self.critic_grads,
            critic_exp_avg=st["critic"][0], critic_exp_avg_sq=st["critic"][1], actor_workspace=self.actor_workspace,
            critic_workspace=self.critic_workspace, log_ent_coef=self.log_ent_coef, exp_avg=es["exp_avg"], exp_avg_sq=es["exp_avg_sq"], replay=replay,
            batch=batch, scratch=scratch, count=M, seed=self.seed, update_seed=0, gamma=hp["gamma"], tau=hp["tau"],
            target_entropy=hp["target_entropy"], lr=hp["learning_rate"], betas=st["betas"], eps=st["eps"])
        self._train = dict(replay=replay, binding=binding, scratch=scratch, batch=batch, nstep=None, prioritized=None, hindsight=None)
        if hp.get("hindsight"):  # the rule of urgym_sac_train_hindsight's gathers: numbers only, no scratch
            self._train["hindsight"] = dict(n_sampled_goal=hp["her_n_sampled_goal"], strategy=hp["her_strategy"], horizon=int(env.cfg.max_episode_steps))
        if hp.get("prioritized"):  # the scratch of urgym_sac_train_prioritized; like the batch scratch, never saved
            per = {name: torch.zeros(shape(M), dtype=torch.float32, device=dev) for name, shape in _abi.SAC_PRIORITIZED_SCRATCH}
            per.update(total=torch.zeros((1,), dtype=torch.float64, device=dev), replay=replay, beta0=float(hp["per_beta"]), beta_steps=int(hp["per_beta_steps"]))
            self._train["prioritized"] = per
        if int(hp["n_steps"]) > 1:  # the two scratch tensors of urgym_sac_train_nstep; like the batch scratch, never saved
            self._train["nstep"] = dict(n_steps=int(hp["n_steps"]), discount=torch.zeros((M,), dtype=torch.float32, device=dev),
                                        q_min_next=torch.zeros((M,), dtype=torch.float32, device=dev))
        return self._train

    def train(self, replay, iterations, steps_per_iteration=1, updates_per_iteration=1, *, seed, first_draw, evaluation=None, eval_every=None,
              monitor=None, log_every=None, planner=None, explore_sigma=0.0, sync_planner=True, plan_stats=False):
        """`iterations` x (``collect(replay, steps_per_iteration)``, `updates_per_iteration` x ``update(replay, seed, draw)`` with draw =
        `first_draw`, `first_draw` + 1, ...) in ONE native call (``env.sac_train``, urgym_sac_train), bit for bit: the loop of
        tools/train_sac.py without Python between the launches.  Needs ``device_entropy``.  The warm-up is the loop's: an iteration
        collects with uniform actions while ``env_steps * N < learning_starts`` when it starts, and runs no update while that still
        holds after its collection (``evaluation.warmup_iterations``).  Advances ``env_steps``, ``draw``, ``adam_state["step"]``,
        ``replay.cursor`` and ``replay.filled``; ``last_update`` refers to the scratch the last update used.  Returns the three
        losses as device tensors of one entry per update (not synchronised).  ``steps_per_iteration=0, iterations=1`` is
        `updates_per_iteration` updates in one call.  Whatever is given below, it stays ONE native call (``env.sac_train`` picks the
        entry point).

        With `evaluation` (an ``evaluation.DeviceEvaluation`` on a second environment) and `eval_every`: after every iteration in which
        the update count (``adam_state["step"]``) passes a multiple of `eval_every`, the actor as it then stands is evaluated
        (``evaluation.evaluate`` of ``self.actor.tensors()``, bit for bit) without leaving the call; `evaluation`'s counters advance.
        Both or neither: one alone raises ValueError.

        With `monitor` (an ``evaluation.DeviceMonitor`` of the training environment) and `log_every`: every iteration's collection is
        folded into the monitor (``collect(..., monitor=)``, bit for bit, warm-up iterations included), and after every iteration at
        which ``monitor.iterations`` reaches a multiple of `log_every` the finished episodes go to the monitor's next record
        (``monitor.record(monitor.iterations)``).  ``monitor.iterations`` and ``monitor.count`` advance, so that split calls place
        records where one call would.  Both or neither: one alone raises ValueError.

        With ``n_steps`` > 1 every update is the multi-step one.  With ``prioritized``, on a ``DevicePrioritizedReplay``, every
        collection is followed by the fill of its slots and every update is ``update``'s seventeen launches.  With ``hindsight`` an
        update is the thirteen launches with the gather of ``DeviceReplay.sample_hindsight``.  With ``max_grad_norm``: two more
        launches per update, and the result also holds ``critic_grad_norm`` and ``actor_grad_norm``, one entry per update like the
        losses.  With ``normalize``: the normalized collection, one fold of the statistics per iteration and one ``norm_batch`` per
        update; not together with `evaluation` unless ``norm_obs`` is off.

        With `planner` (an ``evaluation.DeviceMPPI`` on this learner's env) every iteration is
        ``collect(replay, steps_per_iteration, monitor=, planner=, explore_sigma=)``, then -- unless the warm-up still holds after it --
        the updates and, with `sync_planner`, ``sync_planner(planner)``, bit for bit and still ONE native call
        (urgym_sac_train_planned).  Every step is planned: ``learning_starts`` only decides which iterations run no update.  With
        ``plan_stats=True`` (it needs `monitor`) every record of the monitor has a ``planner.stats`` record of the iteration's last plan
        beside it, in ``planner.records`` at the monitor's index, and the result holds the records of this call (rows of
        ``planner.records``, not synchronised) under ``"plan_stats"``.  Raises ValueError, before anything runs, for ``normalize=True``,
        for a planner on another env, for `explore_sigma` without `planner` and for `plan_stats` without `monitor` (or without
        `planner`).  Without `planner` the call is exactly the one above."""
        from .evaluation import warmup_iterations

        if (evaluation is None) != (eval_every is None):
            raise ValueError("train: evaluation and eval_every go together (an interval needs something to evaluate with, and the reverse)")
        if (monitor is None) != (log_every is None):
            raise ValueError("train: monitor and log_every go together (an interval needs something to record with, and the reverse)")
        if self.entropy_state is None:
            raise ValueError("train needs device_entropy=True (the native loop is the thirteen launches of the update on the device)")
        if self.hp.get("prioritized") and not hasattr(replay, "priorities_struct"):
            raise ValueError("prioritized=True needs a DevicePrioritizedReplay")
        planning = {}
        if planner is None:
            if explore_sigma:
                raise ValueError("train: explore_sigma is the planner's exploration noise and needs planner=")
            if plan_stats:
                raise ValueError("train: plan_stats needs planner= (the statistics are the planner's)")
        else:
            if self.normalizer is not None:
                raise ValueError("train: planner= together with normalize=True is out of scope (the planner's actor and critic read raw rows, not normalized ones)")
            if getattr(planner, "env", None) is not self.env:
                raise ValueError("train: the planner's source env is not this learner's env (DeviceMPPI(learner.env, ...))")
            if plan_stats and monitor is None:
                raise ValueError("train: plan_stats=True needs monitor= and log_every= (a plan-statistics record goes beside a monitor record)")
            planner.check_explore(explore_sigma)
            planning = dict(planner=dict(planner=planner, explore_sigma=explore_sigma, sync=bool(sync_planner), records=bool(plan_stats)))
        hp, env, st = self.hp, self.env, self.adam_state
        n, K, G = int(iterations), int(steps_per_iteration), int(updates_per_iteration)
        tr = self._train_binding(replay)
        uniform, idle = warmup_iterations(self.env_steps, env.num_envs, hp["learning_starts"], n, K)
        if planner is not None:
            uniform = 0  # every step is planned; the warm-up only keeps the idle iterations without updates
        first_record = None if monitor is None else monitor.count
        updates = max(0, n - idle) * max(0, G)
        losses = torch.empty((3, updates), dtype=torch.float32, device=env.device)
        cs, clipping = self.clip_state, {}
        if cs is not None:
            norms = torch.empty((2, updates), dtype=torch.float32, device=env.device)
            clipping = dict(clipping=dict(max_grad_norm=hp["max_grad_norm"], scale=cs["scale"], critic_grad_norm=norms[0], actor_grad_norm=norms[1]))
        cloning, bc_out = {}, {}
        if self.bc_state is not None:
            bc_out = dict(bc_loss=torch.empty((updates,), dtype=torch.float32, device=env.device), bc_weight=torch.empty((updates,), dtype=torch.float32, device=env.device),
                          bc_rows=torch.empty((updates,), dtype=torch.int32, device=env.device))
            cloning = dict(cloning=dict(weight=hp["bc_weight"], scale_by_q=hp["bc_scale_by_q"], q_filter=hp["bc_q_filter"], **bc_out))
        if self.adv_state is not None:
            adv_out = dict(adv_ess=torch.empty((updates,), dtype=torch.float32, device=env.device), adv_max=torch.empty((updates,), dtype=torch.float32, device=env.device),
                           adv_clipped=torch.empty((updates,), dtype=torch.int32, device=env.device))
            cloning["weighting"] = dict(temperature=hp["bc_advantage_temperature"], max_weight=hp["bc_advantage_max_weight"], **adv_out)
            bc_out.update(adv_out)
        if self.demonstrations is not None:  # read at its own oldest_slot and filled as they stand now
            cloning["demonstrating"] = dict(replay=self.demonstrations, count=hp["demo_batch_size"], source=self.demo_source, clone_only=hp["bc_demo_only"])
        tr["binding"].struct.update_seed = int(seed)
        env.sac_train(tr["binding"], losses[0], losses[1], losses[2], first_slot=replay.cursor, filled_steps=replay.filled, num_iterations=n,
                      steps_per_iteration=K, updates_per_iteration=G, uniform_iterations=uniform, idle_iterations=idle,
                      collect_first_draw=self.draw, update_first_draw=int(first_draw), first_step=st["step"] + 1,
                      **({} if evaluation is None else dict(evaluation=evaluation, eval_every=eval_every)),
                      **({} if monitor is None else dict(monitor=monitor, log_every=log_every)),
                      **({} if tr["nstep"] is None else dict(nstep=tr["nstep"])),
                      **({} if tr["prioritized"] is None else dict(prioritized=tr["prioritized"])),
                      **({} if tr["hindsight"] is None else dict(hindsight=tr["hindsight"])), **clipping,
                      **({} if self.normalizer is None else dict(normalizer=self.normalizer)), **planning, **cloning)
        self.env_steps += n * K
        self.draw += n * K
        st["step"] += updates
        replay.cursor = (replay.cursor + n * K) % replay.capacity
        replay.filled = min(replay.capacity, replay.filled + n * K)
        if updates:
            sc = tr["scratch"]
            self.last_update = dict(log_prob=sc["log_prob"], y=sc["y"], q=sc["q"], q_min=sc["q_min"], dqmin_da=sc["dqmin_da"])
            if tr["prioritized"] is not None:
                per = tr["prioritized"]
                self.last_update.update(q_evaluated=per["q"], index=tr["batch"]["index"], leaf=per["leaf"], total=per["total"],
                                        **{k: per[k] for k in ("w_raw", "w", "dq", "new_leaf")})
            if cs is not None:  # the last update's norms, as views of the call's slots; the coefficients are the scratch's
                self.last_update.update(critic_grad_norm=norms[0, updates - 1:], actor_grad_norm=norms[1, updates - 1:], critic_scale=cs["critic_scale"],
                                        actor_scale=cs["actor_scale"])
            if self.demonstrations is not None:
                self.last_update.update(source=self.demo_source)
            if bc_out:  # the last update's three (six with the advantage weight), as views of the call's slots
                self.last_update.update({k: v[updates - 1:] for k, v in bc_out.items()}, action_pi=sc["action_pi"], action_data=tr["batch"]["action"])
        extra = {"plan_stats": planner.records[first_record:monitor.count]} if plan_stats else {}
        extra.update(bc_out)
        if cs is not None:
            return {"critic_loss": losses[0], "actor_loss": losses[1], "ent_coef_loss": losses[2], "critic_grad_norm": norms[0], "actor_grad_norm": norms[1], **extra}
        return {"critic_loss": losses[0], "actor_loss": losses[1], "ent_coef_loss": losses[2], **extra}

    # ------------------------------------------------------------------------------------------------ checkpoints
    OVERRIDABLE = ("learning_rate", "learning_starts")  # what a resumed run may set anew; everything else must be the checkpoint's

    def _optimizers(self):
        return dict(actor_opt=self.actor_opt, critic_opt=self.critic_opt, ent_opt=self.ent_opt)

    def _saved_hp(self):
        """The hyperparameters as a checkpoint holds them: ``n_steps`` only where it is not 1, so that the file of a one-step run is
        what it was before the option existed (``check_state_dict`` reads an absent ``n_steps`` as 1)."""
        return {k: v for k, v in self.hp.items() if (k != "n_steps" or int(v) != 1) and (k not in PER_DEFAULTS or self.hp.get("prioritized"))
                and (k not in HER_DEFAULTS or self.hp.get("hindsight")) and (k not in CLIP_DEFAULTS or v is not None)
                and (k not in NORM_DEFAULTS or self.hp.get("normalize")) and (k not in BC_DEFAULTS or self.hp.get("bc_weight") is not None)
                and (k not in DEMO_DEFAULTS or self.hp.get("demo_batch_size") is not None)
                and (k not in ADV_DEFAULTS or self.hp.get("bc_advantage_temperature") is not None)}

    def state_dict(self):
        """Everything the learner is, as host arrays and scalars: the actor's eight and the critics' twelve parameter tensors, the
        TARGET critic's twelve in the same layout (``DeviceCritic.parameters``: the unpack kernel; the Polyak average lives nowhere
        else), ``log_ent_coef``, ``adam_state`` and ``entropy_state``'s two moments where the learner has them, the three
        ``torch.optim`` state dicts and the ``torch.Generator`` state (empty and unused on the device routes), ``env_steps``, ``draw``,
        ``seed``, the hyperparameters, the env id and env count.  One launch, then ONE synchronisation, then copies."""
        target = self.target.parameters()
        torch.cuda.synchronize(self.env.device)
        host = lambda w: {k: v.detach().cpu().numpy() for k, v in w.items()}  # noqa: E731
        out = dict(env_id=self.env.env_id, num_envs=self.env.num_envs, hp=self._saved_hp(), seed=self.seed, env_steps=self.env_steps, draw=self.draw,
                   actor=host(self.actor.tensors()), critic=[host(w) for w in self.critic.tensors()], target=[host(w) for w in target],
                   log_ent_coef=self.log_ent_coef.detach().cpu().numpy(), adam_state=None, entropy_state=None)
        st, es = self.adam_state, self.entropy_state
        if st is not None:
            out["adam_state"] = dict(step=st["step"], betas=list(st["betas"]), eps=st["eps"], actor=[host(w) for w in st["actor"]],
                                     critic=[[host(w) for w in pair] for pair in st["critic"]])
        if es is not None:
            out["entropy_state"] = dict(exp_avg=es["exp_avg"].cpu().numpy(), exp_avg_sq=es["exp_avg_sq"].cpu().numpy())
        if self.normalizer is not None:  # a run without the option gains no key
            out["normalizer"] = self.normalizer.state_dict()
        out["torch"] = dict({name: _optimizer_to_host(opt.state_dict()) for name, opt in self._optimizers().items()},
                            generator=self.noise.get_state().cpu().numpy())
        return out

    def _tensor_plan(self, state):
        """[(destination tensor, source array, name)] for every tensor ``load_state_dict`` writes in place, shapes and dtypes checked."""
        plan = []

        def add(dst, src, name):
            a = np.asarray(src)
            if a.dtype != np.float32 or a.shape != tuple(dst.shape):
                raise ValueError(f"load_state_dict: {name} must be float32 {tuple(dst.shape)}, got {a.dtype} {a.shape}")
            plan.append((dst, a, name))

        def add_set(dst, src, name):
            if sorted(dst) != sorted(src):
                raise ValueError(f"load_state_dict: {name} holds {sorted(src)}, expected {sorted(dst)}")
            for k in dst:
                add(dst[k], src[k], f"{name}.{k}")

        add_set(self.actor.tensors(), state["actor"], "actor")
        for i, w in enumerate(self.critic.tensors()):
            add_set(w, state["critic"][i], f"critic.qf{i}")
        add(self.log_ent_coef, state["log_ent_coef"], "log_ent_coef")
        st, es = self.adam_state, self.entropy_state
        if st is not None:
            for j, moment in enumerate(("exp_avg", "exp_avg_sq")):
                add_set(st["actor"][j], state["adam_state"]["actor"][j], f"adam_state.actor.{moment}")
                for i in range(2):
                    add_set(st["critic"][j][i], state["adam_state"]["critic"][j][i], f"adam_state.critic.{moment}.qf{i}")
        if es is not None:
            for k in ("exp_avg", "exp_avg_sq"):
                add(es[k], state["entropy_state"][k], f"entropy_state.{k}")
        return plan

    def check_state_dict(self, state, override=()):
        """Raises ValueError naming the first difference unless `state` is a ``state_dict`` of a learner like this one: the same env id
        and env count, the same hyperparameters -- widths and the ``device_*`` option set among them -- but those named in `override`
        (of ``OVERRIDABLE``), and tensors of this learner's shapes.  Writes nothing.  Returns what ``load_state_dict`` needs."""
        unknown = [k for k in override if k not in self.OVERRIDABLE]
        if unknown:
            raise ValueError(f"load_state_dict: only {self.OVERRIDABLE} may be overridden, got {unknown}")
        if state["env_id"] != self.env.env_id:
            raise ValueError(f"load_state_dict: env_id is {state['env_id']!r} in the checkpoint, {self.env.env_id!r} here")
        if int(state["num_envs"]) != self.env.num_envs:
            raise ValueError(f"load_state_dict: num_envs is {state['num_envs']} in the checkpoint, {self.env.num_envs} here")
        for k in SAC_DEFAULTS:
            if k in override:
                continue
            saved = dict(n_steps=1, **state["hp"]) if "n_steps" not in state["hp"] else state["hp"]  # a one-step run's file holds no n_steps
            if k not in saved or saved[k] != self.hp[k]:
                raise ValueError(f"load_state_dict: {k} is {saved.get(k)!r} in the checkpoint, {self.hp[k]!r} here")
        for k, default in PER_DEFAULTS.items():  # a file without priorities holds none of the three
            if k != "prioritized" and not self.hp.get("prioritized") and not state["hp"].get("prioritized"):
                continue
            if state["hp"].get(k, default) != self.hp.get(k, default):
                raise ValueError(f"load_state_dict: {k} is {state['hp'].get(k, default)!r} in the checkpoint, {self.hp.get(k, default)!r} here")
        for k, default in HER_DEFAULTS.items():  # a file without hindsight holds none of the three
            if k != "hindsight" and not self.hp.get("hindsight") and not state["hp"].get("hindsight"):
                continue
            if state["hp"].get(k, default) != self.hp.get(k, default):
                raise ValueError(f"load_state_dict: {k} is {state['hp'].get(k, default)!r} in the checkpoint, {self.hp.get(k, default)!r} here")
        for k, default in CLIP_DEFAULTS.items():  # a file without clipping holds no max_grad_norm
            if state["hp"].get(k, default) != self.hp.get(k, default):
                raise ValueError(f"load_state_dict: {k} is {state['hp'].get(k, default)!r} in the checkpoint, {self.hp.get(k, default)!r} here")
        for k, default in BC_DEFAULTS.items():  # a file without cloning holds none of the three
            if state["hp"].get(k, default) != self.hp.get(k, default):
                raise ValueError(f"load_state_dict: {k} is {state['hp'].get(k, default)!r} in the checkpoint, {self.hp.get(k, default)!r} here")
        for k, default in DEMO_DEFAULTS.items():  # a file without demonstrations holds neither
            if state["hp"].get(k, default) != self.hp.get(k, default):
                raise ValueError(f"load_state_dict: {k} is {state['hp'].get(k, default)!r} in the checkpoint, {self.hp.get(k, default)!r} here")
        for k, default in ADV_DEFAULTS.items():  # a file without the advantage weight holds neither
            if state["hp"].get(k, default) != self.hp.get(k, default):
                raise ValueError(f"load_state_dict: {k} is {state['hp'].get(k, default)!r} in the checkpoint, {self.hp.get(k, default)!r} here")
        for k, default in NORM_DEFAULTS.items():  # a file without normalization holds none of the six, and no statistics
            if k != "normalize" and not self.hp.get("normalize") and not state["hp"].get("normalize"):
                continue
            if state["hp"].get(k, default) != self.hp.get(k, default):
                raise ValueError(f"load_state_dict: {k} is {state['hp'].get(k, default)!r} in the checkpoint, {self.hp.get(k, default)!r} here")
        normalizer = getattr(self, "normalizer", None)
        if (state.get("normalizer") is None) != (normalizer is None):
            raise ValueError(f"load_state_dict: the statistics of normalize are {'absent from' if state.get('normalizer') is None else 'present in'} the checkpoint and the reverse here")
        if normalizer is not None:
            normalizer.check_state_dict(state["normalizer"])
        for name, mine in (("adam_state", self.adam_state), ("entropy_state", self.entropy_state)):
            if (state[name] is None) != (mine is None):
                raise ValueError(f"load_state_dict: {name} is {'absent' if state[name] is None else 'present'} in the checkpoint and the reverse here")
        if self.adam_state is not None:
            st, saved = self.adam_state, state["adam_state"]
            if list(saved["betas"]) != list(st["betas"]) or saved["eps"] != st["eps"]:
                raise ValueError(f"load_state_dict: adam_state has betas {saved['betas']} and eps {saved['eps']} in the checkpoint, {list(st['betas'])} and {st['eps']} here")
        plan = self._tensor_plan(state)
        n, H = self.target.in_features, self.target.hidden_width
        shapes = dict(zip(CRITIC_ARRAYS, ((H, n), (H,), (H, H), (H,), (1, H), (1,))))
        target = []
        for i in range(2):
            w = {k: np.asarray(state["target"][i][k]) for k in CRITIC_ARRAYS}
            for k, a in w.items():
                if a.dtype != np.float32 or a.shape != shapes[k]:
                    raise ValueError(f"load_state_dict: target.qf{i}.{k} must be float32 {shapes[k]}, got {a.dtype} {a.shape}")
            target.append(w)
        return plan, target

    def load_state_dict(self, state, override=()):
        """Puts a ``state_dict`` back.  Refuses (ValueError, nothing written) what ``check_state_dict`` refuses; `override` names the
        hyperparameters of ``OVERRIDABLE`` for which this learner's own value stays.  Every tensor is written IN PLACE, so the
        ``.grad`` aliases, the workspaces and a ``train`` binding made earlier stay valid; then the three packed buffers are rebuilt by
        the launches that always build them: ``device_actor.load_parameters``, ``online.load_parameters(tau=1)`` and
        ``target.load_parameters(the saved target tensors, tau=1)``.  Not synchronised beyond the host-to-device copies."""
        plan, target = self.check_state_dict(state, override)
        dev = self.env.device
        with torch.no_grad():
            for dst, a, _ in plan:
                dst.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        if self.adam_state is not None:
            self.adam_state["step"] = int(state["adam_state"]["step"])
        for name, opt in self._optimizers().items():
            opt.load_state_dict(_optimizer_from_host(state["torch"][name], opt, dev))
        self.noise.set_state(torch.from_numpy(np.ascontiguousarray(state["torch"]["generator"])))
        self.seed, self.env_steps, self.draw = int(state["seed"]), int(state["env_steps"]), int(state["draw"])
        if self.normalizer is not None:
            self.normalizer.load_state_dict(state["normalizer"])
        if self._train is not None:
            self._train["binding"].struct.seed = self.seed  # the collection's seed of a binding made before the load
        self._repack([{k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in w.items()} for w in target])

    def _repack(self, target_tensors):
        """The three packed buffers from the torch parameters as they stand, and the target from `target_tensors`."""
        self.device_actor.load_parameters(self.actor.tensors())
        if self.online is not None:
            self.online.load_parameters(self.critic.tensors(), tau=1.0)
        self.target.load_parameters(target_tensors, tau=1.0)

    def load_parameters(self, actor, critics, target=None, log_ent_coef=None):
        """A warm start from plain parameter files, the reference's ``SAC.load(...)`` followed by ``learn`` (train.py:31-36): `actor` a
        dict of arrays under ACTOR_ARRAYS + LOG_STD_ARRAYS, `critics` (and `target`, default `critics`) two dicts under
        CRITIC_ARRAYS, as tests/golden/actors and tests/golden/critics hold them.  Sets the parameters in place, zeroes every Adam
        moment and the step count, and rebuilds the packed buffers; `log_ent_coef` (a float) is set where given.  ``env_steps`` and
        ``draw`` stay.  ValueError for shapes that are not this learner's, before anything is written."""
        def host(w, keys):
            w = dict(w)
            return {k: np.asarray(w[k], dtype=np.float32) for k in keys if k in w}

        actor = host(actor, ACTOR_ARRAYS + LOG_STD_ARRAYS)
        missing = [k for k in ACTOR_ARRAYS + LOG_STD_ARRAYS if k not in actor]
        if missing:
            raise ValueError(f"load_parameters: actor arrays missing: {missing}")
        critics = [host(w, CRITIC_ARRAYS) for w in critics]
        target = critics if target is None else [host(w, CRITIC_ARRAYS) for w in target]
        if len(critics) != 2 or len(target) != 2:
            raise ValueError("load_parameters: a twin critic has two Q-networks")
        mine = self.critic.tensors()
        checked = [("actor", self.actor.tensors(), actor)] + [(f"critics[{i}]", mine[i], critics[i]) for i in range(2)] + \
                  [(f"target[{i}]", mine[i], target[i]) for i in range(2)]  # the target has the critics' shapes and no tensor of its own
        for name, dst, src in checked:
            for k, t in dst.items():
                if k not in src or src[k].shape != tuple(t.shape):
                    raise ValueError(f"load_parameters: {name}.{k} must have shape {tuple(t.shape)}, got {src[k].shape if k in src else 'nothing'}")
        plan = [(t, src[k]) for _, dst, src in checked[:3] for k, t in dst.items()]
        if log_ent_coef is not None and not np.isfinite(float(log_ent_coef)):
            raise ValueError(f"load_parameters: log_ent_coef must be finite, got {log_ent_coef}")
        dev = self.env.device
        with torch.no_grad():
            for t, a in plan:
                t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
            if log_ent_coef is not None:
                self.log_ent_coef.fill_(float(log_ent_coef))
            if self.adam_state is not None:
                st = self.adam_state
                st["step"] = 0
                for w in list(st["actor"]) + [w for pair in st["critic"] for w in pair]:
                    for t in w.values():
                        t.zero_()
            if self.entropy_state is not None:
                self.entropy_state["exp_avg"].zero_()
                self.entropy_state["exp_avg_sq"].zero_()
        for opt in self._optimizers().values():
            opt.state.clear()  # torch's Adam starts again: zero moments, step 0
        self._repack([{k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in w.items()} for w in target])

    def save(self, path, replay=None, monitor=None, evaluation=None, env_state=True, extra=None, demonstrations=None):
        """One ``.npz`` (``ur_gym_amd.checkpoint``: plain arrays and one JSON string, readable with ``allow_pickle=False``) holding
        ``state_dict()`` and, where given, the ``state_dict`` of `replay`, `monitor` and `evaluation`, the training environment's
        ``checkpoint_state`` (`env_state`) and `extra`, the caller's own counters as JSON scalars (tools/train_sac.py keeps its update
        draw there).  Written to a temporary name and renamed: a job killed mid-save leaves the previous file whole.  With
        `demonstrations` (the learner's demonstration ring) its ``state_dict`` goes under ``demonstrations``, a key a file without it does
        not hold."""
        from . import checkpoint

        state = dict(learner=self.state_dict(), extra=extra,
                     replay=None if replay is None else replay.state_dict(), monitor=None if monitor is None else monitor.state_dict(),
                     evaluation=None if evaluation is None else evaluation.state_dict(), env=self.env.checkpoint_state() if env_state else None)
        if demonstrations is not None:
            state["demonstrations"] = demonstrations.state_dict()
        checkpoint.write(path, state)

    def load(self, path, replay=None, monitor=None, evaluation=None, env_state=True, override=(), demonstrations=None):
        """Reads what ``save`` wrote into this learner and the same objects; returns `extra`.  A part that was saved but has no object
        handed in, or the reverse, raises ValueError, and so does everything ``load_state_dict`` and the parts' own loads refuse -- the
        learner's, the ring's and the environment's checks are all made before anything is written."""
        from . import checkpoint

        state = checkpoint.read(path)
        given = dict(replay=replay, monitor=monitor, evaluation=evaluation, env=self.env if env_state else None)
        for name, obj in given.items():
            if (state[name] is None) != (obj is None):
                raise ValueError(f"load: {name} is {'absent from' if state[name] is None else 'present in'} the checkpoint, "
                                 f"and the call has {'no' if obj is None else 'an'} object for it")
        if ("demonstrations" in state) != (demonstrations is not None):
            raise ValueError(f"load: demonstrations is {'present in' if 'demonstrations' in state else 'absent from'} the checkpoint, "
                             f"and the call has {'no' if demonstrations is None else 'an'} object for it")
        self.check_state_dict(state["learner"], override)
        if replay is not None:
            replay.check_state_dict(state["replay"])
        if demonstrations is not None:
            demonstrations.check_state_dict(state["demonstrations"])
        if env_state:
            self.env.check_checkpoint(state["env"])
        self.load_state_dict(state["learner"], override)
        if env_state:
            self.env.restore_checkpoint(state["env"])
        for name in ("replay", "monitor", "evaluation"):
            if given[name] is not None:
                given[name].load_state_dict(state[name])
        if demonstrations is not None:
            demonstrations.load_state_dict(state["demonstrations"])
        return state["extra"]

    def close(self):
        self._train = None
        self.device_actor.close()
        self.target.close()
        if self.online is not None:
            self.online.close()
