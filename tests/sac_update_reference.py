"""One SAC update as scalar losses in torch on the CPU, every gradient from ``torch.autograd``.

A second derivation of what ``SACLearner._update_on_device`` and the native training call compute, written from the equations of
DESIGN.md sections 9 to 16, 21, 22, 24, 25 and 33 to 35 and from SAC as published (Haarnoja et al. 2018; stable-baselines3's
``SAC.train`` for the order of the three steps): no kernel, no restatement and no hand-derived gradient is used.  ``dtype`` is
``torch.float64`` (the reference) or ``torch.float32`` (the yardstick the GPU test measures the device against).  Taken as given: the
gathered minibatch (the gathers are tested bit for bit elsewhere) and the noise words (``evaluation.policy_noise``, a data-free helper,
like ``per_beta``).

``run(inputs, dtype, variant=None)`` returns a dict of float64 numpy arrays (and ``decisions``).  `inputs`:

    actor, critics[2], target[2]      dicts of float32 arrays under the learner's parameter names; log_ent_coef a float32
    moments                           dict(actor=(m, v), critics=([m0, m1], [v0, v1]), ent=(m, v)) and ``step`` (the count BEFORE the update)
    batch                             the raw gathered rows: observations / next_observations (dicts of the three groups), actions,
                                      rewards, terminated and, where they apply, discount (n-step), leaf + total + size (PER), source
    seed, draw, hp                    hp: gamma, tau, learning_rate, target_entropy, betas, eps and the options' keys
    norm                              None or the normalizer's statistics and options

`variant` names ONE deliberate mis-wiring (``VARIANTS``): switches for tests/test_sac_update_reference_host.py only, which shows that
each moves a compared quantity far above the GPU test's bound.  Every discrete decision of the run (ReLU masks, the log_std clamp, the
``q_1 < q_0`` selector, the filter verdict, the weight cap, the clip verdicts, the normalizer's clips) is recorded in ``decisions`` as
(name, quantity - threshold, sum of |terms| that formed it, verdict).
"""
import numpy as np
import torch

from ur_gym_amd.evaluation import per_beta, policy_noise

LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
ACTOR_KEYS = ("latent_pi_0_weight", "latent_pi_0_bias", "latent_pi_2_weight", "latent_pi_2_bias", "mu_weight", "mu_bias", "log_std_weight", "log_std_bias")
CRITIC_KEYS = ("q_0_weight", "q_0_bias", "q_2_weight", "q_2_bias", "q_4_weight", "q_4_bias")
GROUPS = ("achieved_goal", "desired_goal", "observation")  # the order of the networks' input features
MARGIN = 2.0 ** -16

# stage -> the mis-wired variants of it (``variant_applies`` says under which options a variant changes anything)
VARIANTS = {
    "target and noise": ("actor_pre_step_critic", "alpha_after_step_in_y", "alpha_after_step_in_actor", "y_online", "y_target_after_blend", "next_policy_stream"),
    "entropy term": ("entropy_on_terminated", "entropy_gamma"),
    "critic selection": ("q0_for_min",),
    "cloning": ("meanabs_attached", "bc_mean_over_cloned", "filter_from_target", "clone_tanh_mu"),
    "advantage weights": ("adv_attached", "adv_norm_all"),
    "PER": ("per_no_max", "per_beta_previous"),
    "clipping": ("clip_joint_norm", "clip_on_moments"),
    "normalization": ("norm_next_raw",),
}


def variant_applies(variant, hp):
    """Whether `variant` changes anything under the options `hp`."""
    bc, adv = hp.get("bc_weight") is not None, hp.get("bc_advantage_temperature") is not None
    return {
        "entropy_gamma": int(hp.get("n_steps", 1)) > 1,
        "meanabs_attached": bc and bool(hp.get("bc_scale_by_q")),
        "bc_mean_over_cloned": bc and not adv and (bool(hp.get("bc_q_filter")) or bool(hp.get("bc_demo_only"))),
        "filter_from_target": bc and bool(hp.get("bc_q_filter")),
        "clone_tanh_mu": bc,
        "adv_attached": adv, "adv_norm_all": adv and bool(hp.get("bc_demo_only")),
        "per_no_max": bool(hp.get("prioritized")), "per_beta_previous": bool(hp.get("prioritized")),
        "clip_joint_norm": hp.get("max_grad_norm") is not None, "clip_on_moments": hp.get("max_grad_norm") is not None,
        "norm_next_raw": bool(hp.get("normalize")),
    }.get(variant, True)


class Decisions(list):
    def add(self, name, quantity, magnitude, verdict=None):
        q = np.asarray(quantity.detach().double().numpy() if isinstance(quantity, torch.Tensor) else quantity, dtype=np.float64)
        m = np.asarray(magnitude.detach().double().numpy() if isinstance(magnitude, torch.Tensor) else magnitude, dtype=np.float64)
        self.append((name, q, np.broadcast_to(m, q.shape), (q > 0) if verdict is None else np.asarray(verdict, dtype=bool)))


def margins_hold(decisions):
    """The condition of the cases: every decision's distance from its threshold is at least 2^-16 of the sum of |terms|.  Returns the
    list of (name, worst ratio, count of elements below) that break it: empty where it holds."""
    bad = []
    for name, q, m, _ in decisions:
        short = np.abs(q) < MARGIN * m
        if short.any():
            with np.errstate(all="ignore"):
                bad.append((name, float(np.min(np.abs(q)[short] / m[short])), int(short.sum())))
    return bad


def _t(a, dtype, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype, requires_grad=grad)


def _params(w, keys, dtype, grad):
    return {k: _t(w[k], dtype, grad) for k in keys}


def _hidden(dec, name, x, w, prefix):
    h = x
    for i in (0, 2):
        W, b = w[f"{prefix}_{i}_weight"], w[f"{prefix}_{i}_bias"]
        z = h @ W.T + b
        dec.add(f"{name}.relu{i}", z, h.abs() @ W.abs().T + b.abs())
        h = torch.relu(z)
    return h


def _sample(dec, name, x, w, eps):
    """The squashed Gaussian of SAC: a = tanh(mu + exp(log_std) eps), log pi(a|s) with the tanh correction log(1 - a^2 + 1e-6)."""
    h = _hidden(dec, name, x, w, "latent_pi")
    mu = h @ w["mu_weight"].T + w["mu_bias"]
    raw = h @ w["log_std_weight"].T + w["log_std_bias"]
    mag = h.abs() @ w["log_std_weight"].abs().T + w["log_std_bias"].abs()
    dec.add(f"{name}.log_std_above_max", raw - LOG_STD_MAX, mag + abs(LOG_STD_MAX))
    dec.add(f"{name}.log_std_below_min", LOG_STD_MIN - raw, mag + abs(LOG_STD_MIN))
    log_std = raw.clamp(LOG_STD_MIN, LOG_STD_MAX)
    action = torch.tanh(mu + log_std.exp() * eps)
    log_prob = (-0.5 * eps * eps - log_std - 0.5 * np.log(2.0 * np.pi)).sum(1) - torch.log(1.0 - action * action + 1e-6).sum(1)
    return action, log_prob, mu, log_std


def _q(dec, name, x, a, w):
    h = _hidden(dec, name, torch.cat([x, a], dim=1), w, "q")
    W, b = w["q_4_weight"], w["q_4_bias"]
    return (h @ W.T + b)[:, 0], (h.abs() @ W.abs().T + b.abs())[:, 0]


def _min(dec, name, q0, m0, q1, m1):
    dec.add(f"{name}.q1_below_q0", q1 - q0, m0 + m1)
    pick = q1 < q0
    return torch.where(pick, q1, q0), torch.where(pick, m1, m0)


def _features(rows, dtype):
    return torch.cat([_t(rows[g], dtype) for g in GROUPS], dim=1)


def _normalize(dec, name, x, mean, var, eps, clip, dtype, centre=True):
    """VecNormalize: clip((x - mean) / sqrt(var + eps), -clip, clip); a reward is not centred."""
    x, mean, var = _t(x, dtype), _t(mean, dtype), _t(var, dtype)
    z = ((x - mean) if centre else x) / torch.sqrt(var + eps)
    mag = (x.abs() + (mean.abs() if centre else 0.0)) / torch.sqrt(var + eps) + clip
    dec.add(f"{name}.above_clip", z - clip, mag)
    dec.add(f"{name}.below_clip", -clip - z, mag)
    return z.clamp(-clip, clip)


def _adam(p, g, m, v, lr, b1, b2, eps, t, clip_moments=None):
    """torch.optim.Adam's step (Kingma & Ba with the bias corrections, eps outside the corrected root)."""
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * g * g
    top = m2 if clip_moments is None else m2 * clip_moments
    return p - (lr / (1.0 - b1 ** t)) * top / (v2.sqrt() / np.sqrt(1.0 - b2 ** t) + eps), m2, v2


def _norm(grads):
    return torch.sqrt(sum((g.double() ** 2).sum() for g in grads)).to(grads[0].dtype)


def _clip(dec, name, norm, max_norm):
    """torch.nn.utils.clip_grad_norm_: the coefficient max / (norm + 1e-6) where that is below 1, else 1."""
    if max_norm is None:
        return None
    dec.add(f"{name}.clips", norm + 1e-6 - max_norm, norm.abs() + 1e-6 + max_norm)
    c = max_norm / (norm + 1e-6)
    return c if float(c) < 1.0 else torch.ones_like(c)


def run(inputs, dtype=torch.float64, variant=None):
    V = variant
    hp, batch, norm = inputs["hp"], inputs["batch"], inputs.get("norm")
    dec, out = Decisions(), {}
    n64 = lambda x: x.detach().double().numpy().copy()  # noqa: E731
    correct = run(inputs, dtype) if V in ("y_target_after_blend", "clip_joint_norm") else None  # what a later stage of the right update leaves
    lr, (b1, b2), aeps = float(hp["learning_rate"]), hp["betas"], float(hp["eps"])
    gamma, tau, M = float(hp["gamma"]), float(hp["tau"]), len(batch["rewards"])
    t = int(inputs["moments"]["step"]) + 1
    terminated = torch.tensor(np.asarray(batch["terminated"]).astype(bool))
    alive = (~terminated).to(dtype)
    source = None if batch.get("source") is None else torch.tensor(np.asarray(batch["source"]) != 0)

    # 1. the rows and the reward, normalized with the statistics as they stand
    if hp.get("normalize"):
        o = norm["options"]
        rows = {}
        for which, src in (("s", batch["observations"]), ("n", batch["next_observations"])):
            if which == "n" and V == "norm_next_raw":
                rows[which] = _features(src, dtype)
                continue
            rows[which] = torch.cat([_normalize(dec, f"norm.{which}.{g}", src[g], norm[f"{g}_mean"], norm[f"{g}_var"], o["epsilon"], o["clip_obs"], dtype) for g in GROUPS], dim=1)
        x, xn = rows["s"], rows["n"]
        reward = _normalize(dec, "norm.reward", batch["rewards"], 0.0, norm["ret_var"], o["epsilon"], o["clip_reward"], dtype, centre=False)
    else:
        x, xn, reward = _features(batch["observations"], dtype), _features(batch["next_observations"], dtype), _t(batch["rewards"], dtype)
    actions = _t(batch["actions"], dtype)
    discount = _t(batch["discount"], dtype) if int(hp.get("n_steps", 1)) > 1 else torch.full((M,), gamma, dtype=dtype)

    # the two noise streams: a' at `draw`, the policy's own action at draw | 2^63, the row index as the env word
    ids = np.arange(M)
    eps_pi = _t(policy_noise(inputs["seed"], int(inputs["draw"]) | 1 << 63, ids, "gaussian", dtype=np.float64), dtype)
    eps_next = eps_pi if V == "next_policy_stream" else _t(policy_noise(inputs["seed"], int(inputs["draw"]), ids, "gaussian", dtype=np.float64), dtype)

    actor = _params(inputs["actor"], ACTOR_KEYS, dtype, True)
    online = [_params(w, CRITIC_KEYS, dtype, True) for w in inputs["critics"]]
    target = [_params(w, CRITIC_KEYS, dtype, False) for w in inputs["target"]]
    l = _t(inputs["log_ent_coef"], dtype, True).reshape(())
    alpha = l.detach().exp()

    # 3. the policy's action on the batch rows, from the snapshot actor
    a_pi, log_prob, mu, log_std = _sample(dec, "actor.s", x, actor, eps_pi)
    # the action as the critics and the cloning term read it, apart from the action inside log pi: the gradient with respect to a_q is
    # the partial derivative the learner calls d_action (the path through log pi is d_log_prob's)
    a_q = a_pi.clone()

    # 4. the temperature loss, its gradient and its Adam step
    mom = inputs["moments"]
    ent_loss = -(l * (log_prob.detach() + float(hp["target_entropy"]))).mean()
    (g_l,) = torch.autograd.grad(ent_loss, l)
    l_new, lm, lv = _adam(l.detach(), g_l, _t(mom["ent"][0], dtype).reshape(()), _t(mom["ent"][1], dtype).reshape(()), lr, b1, b2, aeps, t)
    alpha_after = l_new.exp()
    out.update(ent_coef=n64(alpha), ent_coef_loss=n64(ent_loss), ent_coef_loss_scale=n64((l * (log_prob.detach() + float(hp["target_entropy"]))).abs().mean()),
               ent_grad=n64(g_l), log_ent_coef_after=n64(l_new), ent_m_after=n64(lm), ent_v_after=n64(lv))

    # 2. the next action and the target, all of it a constant of the step
    with torch.no_grad():
        a_next, log_prob_next, _, _ = _sample(dec, "actor.s'", xn, {k: v.detach() for k, v in actor.items()}, eps_next)
        nets = target
        if V == "y_online":
            nets = [{k: v.detach() for k, v in w.items()} for w in online]
        elif V == "y_target_after_blend":
            nets = [{k: _t(a, dtype) for k, a in w.items()} for w in correct["target_after"]]
        qn = [_q(dec, f"target{i}.s'", xn, a_next, nets[i]) for i in range(2)]
        q_min_next, _ = _min(dec, "target.s'", qn[0][0], qn[0][1], qn[1][0], qn[1][1])
        alpha_y = alpha_after if V == "alpha_after_step_in_y" else alpha
        ent_discount = (torch.full((M,), gamma, dtype=dtype) if V == "entropy_gamma" else discount) * (1.0 if V == "entropy_on_terminated" else alive)
        y = reward + discount * alive * q_min_next - ent_discount * alpha_y * log_prob_next
    out.update(next_actions=n64(a_next), next_log_prob=n64(log_prob_next), q_min_next=n64(q_min_next), y=n64(y), log_prob=n64(log_prob), action_pi=n64(a_pi))

    # 5. the critic loss on the replayed action, its gradients, the clip, the Adam step and the Polyak blend
    qs = [_q(dec, f"online{i}.s", x, actions, online[i]) for i in range(2)]
    q = torch.stack([qs[0][0], qs[1][0]])
    q.retain_grad()
    e = q - y[None, :]
    unweighted = 0.5 * ((e[0] ** 2).mean() + (e[1] ** 2).mean())
    critic_loss = unweighted
    if hp.get("prioritized"):
        beta = float(per_beta(hp["per_beta"], t - 1 if V == "per_beta_previous" else t, hp["per_beta_steps"]))
        prob = _t(batch["leaf"], dtype) / float(np.asarray(batch["total"]).reshape(-1)[0])
        w_raw = (float(batch["size"]) * prob) ** -beta
        w = w_raw if V == "per_no_max" else w_raw / w_raw.max()
        critic_loss = 0.5 * ((w * e[0] ** 2).mean() + (w * e[1] ** 2).mean())
        new_leaf = (e.detach().abs().max(0).values + float(hp["per_eps"])) ** float(hp["per_alpha"])
        out.update(w=n64(w), new_leaf=n64(new_leaf), per_beta=np.float64(beta))
    flat_c = [online[i][k] for i in range(2) for k in CRITIC_KEYS]
    grads_c = torch.autograd.grad(critic_loss, flat_c + [q])
    dq, grads_c = grads_c[-1], grads_c[:-1]
    out.update(q=n64(q), dq=n64(dq), critic_loss=n64(unweighted), critic_loss_scale=n64(0.5 * ((e[0] ** 2).mean() + (e[1] ** 2).mean())),
               critic_loss_weighted=n64(critic_loss), critic_grads=[{k: n64(grads_c[i * 6 + j]) for j, k in enumerate(CRITIC_KEYS)} for i in range(2)])
    c_norm = _norm(grads_c)
    if V == "clip_joint_norm":
        c_norm = torch.sqrt(c_norm ** 2 + _t(correct["actor_grad_norm"], dtype) ** 2)
    c_scale = _clip(dec, "critic", c_norm, hp.get("max_grad_norm"))
    out.update(critic_grad_norm=n64(c_norm), critic_scale=None if c_scale is None else n64(c_scale))
    stepped, cm, cv = [{}, {}], [{}, {}], [{}, {}]
    for i in range(2):
        for j, k in enumerate(CRITIC_KEYS):
            g = grads_c[i * 6 + j]
            on_m = c_scale if (V == "clip_on_moments" and c_scale is not None) else None
            g = g if (c_scale is None or on_m is not None) else g * c_scale
            stepped[i][k], cm[i][k], cv[i][k] = _adam(online[i][k].detach(), g, _t(mom["critics"][0][i][k], dtype), _t(mom["critics"][1][i][k], dtype), lr, b1, b2, aeps, t, on_m)
    blended = [{k: (1.0 - tau) * target[i][k] + tau * stepped[i][k] for k in CRITIC_KEYS} for i in range(2)]
    out.update(critics_after=[{k: n64(v) for k, v in w.items()} for w in stepped], target_after=[{k: n64(v) for k, v in w.items()} for w in blended],
               critic_m_after=[{k: n64(v) for k, v in w.items()} for w in cm], critic_v_after=[{k: n64(v) for k, v in w.items()} for w in cv])

    # 6. the actor loss through the stepped online critics, the cloning term of whichever option is on, the clip, the Adam step
    nets = [{k: v.detach() for k, v in w.items()} for w in online] if V == "actor_pre_step_critic" else stepped
    qp = [_q(dec, f"stepped{i}.pi", x, a_q, nets[i]) for i in range(2)]
    if V == "q0_for_min":
        q_min, q_min_mag = qp[0]
    else:
        q_min, q_min_mag = _min(dec, "stepped.pi", qp[0][0], qp[0][1], qp[1][0], qp[1][1])
    (dqmin_da,) = torch.autograd.grad(q_min.sum(), a_q, retain_graph=True)
    alpha_pi = alpha_after if V == "alpha_after_step_in_actor" else alpha
    rows_a = alpha_pi * log_prob - q_min
    actor_loss = rows_a.mean()
    total = actor_loss
    out.update(q_min=n64(q_min), dqmin_da=n64(dqmin_da), actor_loss=n64(actor_loss), actor_loss_scale=n64(rows_a.abs().mean()))
    if hp.get("bc_weight") is not None:
        d = (torch.tanh(mu) if V == "clone_tanh_mu" else a_q) - actions
        h = 0.5 * (d * d).sum(1)
        mean_abs = q_min.abs().mean()
        w_bc = torch.as_tensor(float(hp["bc_weight"]), dtype=dtype)
        if hp.get("bc_scale_by_q"):
            w_bc = w_bc * (mean_abs if V == "meanabs_attached" else mean_abs.detach())
        # the critics at the replayed action are the ones the critic's backward pass ran: the online critics before their step
        if V == "filter_from_target":
            with torch.no_grad():
                td_ = [_q(dec, f"target{i}.s", x, actions, target[i]) for i in range(2)]
                tp_ = [_q(dec, f"target{i}.pi", x, a_pi.detach(), target[i]) for i in range(2)]
                q_data, q_data_mag = _min(dec, "target.s", td_[0][0], td_[0][1], td_[1][0], td_[1][1])
                q_ref, q_ref_mag = _min(dec, "target.pi", tp_[0][0], tp_[0][1], tp_[1][0], tp_[1][1])
        else:
            q_data, q_data_mag = _min(dec, "online.s", qs[0][0].detach(), qs[0][1], qs[1][0].detach(), qs[1][1])
            q_ref, q_ref_mag = (q_min if V == "adv_attached" else q_min.detach()), q_min_mag
        mask = torch.ones(M, dtype=torch.bool) if not hp.get("bc_demo_only") else source
        if hp.get("bc_advantage_temperature") is not None:
            T, cap = float(hp["bc_advantage_temperature"]), hp.get("bc_advantage_max_weight")
            A = q_data - q_ref
            n = int(mask.sum())
            ex = torch.where(mask, torch.exp((A - A[mask].max()) / T), torch.zeros_like(A))
            u = ex / (ex.sum() / (M if V == "adv_norm_all" else n))
            if cap is not None:
                dec.add("advantage.above_cap", (u - float(cap))[mask], (u.abs() + float(cap))[mask])
                over = mask & (u > float(cap))
                a_w = u.clamp(max=float(cap))
            else:
                over, a_w = torch.zeros(M, dtype=torch.bool), u
            if V != "adv_attached":
                a_w = a_w.detach()
            per_row = a_w * h
            out.update(adv_ess=n64(ex.sum() ** 2 / (ex * ex).sum()), adv_max=n64(a_w[mask].max()), adv_clipped=np.int64(over.sum()), bc_rows=np.int64(n), adv_weights=n64(a_w))
            cloned = mask
        else:
            cloned = mask
            if hp.get("bc_q_filter"):
                dec.add("filter.data_above_policy", q_data - q_ref.detach(), q_data_mag + q_ref_mag)
                cloned = mask & (q_data > q_ref.detach())
            per_row = cloned.to(dtype) * h
            out.update(bc_rows=np.int64(cloned.sum()))
        denominator = max(int(cloned.sum()), 1) if V == "bc_mean_over_cloned" else M
        bc_loss = per_row.sum() / denominator
        total = total + w_bc * bc_loss
        out.update(bc_loss=n64(bc_loss), bc_loss_scale=n64(per_row.abs().sum() / M), bc_weight=n64(w_bc), cloned=cloned.numpy().copy(), mean_abs=n64(mean_abs))
    flat_a = [actor[k] for k in ACTOR_KEYS]
    grads_a = torch.autograd.grad(total, flat_a + [a_q, log_prob, mu, log_std], allow_unused=True)
    d_action, d_log_prob, d_mu, d_log_std = grads_a[-4:]
    grads_a = grads_a[:-4]
    out.update(actor_grads={k: n64(g) for k, g in zip(ACTOR_KEYS, grads_a)}, d_action=n64(d_action), d_log_prob=n64(d_log_prob), d_mu=n64(d_mu), d_log_std=n64(d_log_std),
               log_std=n64(log_std), eps_pi=n64(eps_pi))
    a_norm = _norm(grads_a)
    if V == "clip_joint_norm":
        a_norm = torch.sqrt(a_norm ** 2 + _t(correct["critic_grad_norm"], dtype) ** 2)
    a_scale = _clip(dec, "actor", a_norm, hp.get("max_grad_norm"))
    out.update(actor_grad_norm=n64(a_norm), actor_scale=None if a_scale is None else n64(a_scale))
    after, am, av = {}, {}, {}
    for k, g in zip(ACTOR_KEYS, grads_a):
        on_m = a_scale if (V == "clip_on_moments" and a_scale is not None) else None
        g = g if (a_scale is None or on_m is not None) else g * a_scale
        after[k], am[k], av[k] = _adam(actor[k].detach(), g, _t(mom["actor"][0][k], dtype), _t(mom["actor"][1][k], dtype), lr, b1, b2, aeps, t, on_m)
    out.update(actor_after={k: n64(v) for k, v in after.items()}, actor_m_after={k: n64(v) for k, v in am.items()}, actor_v_after={k: n64(v) for k, v in av.items()})
    out["decisions"] = dec
    return out


def adam64(p, g, m, v, lr, betas, eps, t, scale=None):
    """Float64 Adam on float32 inputs (numpy): the parameters the device must hold after its step, given ITS gradients and clip coefficient."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    if scale is not None:
        g = g * np.float64(scale)
    m2 = betas[0] * m + (1.0 - betas[0]) * g
    v2 = betas[1] * v + (1.0 - betas[1]) * g * g
    return p - (lr / (1.0 - betas[0] ** t)) * m2 / (np.sqrt(v2) / np.sqrt(1.0 - betas[1] ** t) + eps)
