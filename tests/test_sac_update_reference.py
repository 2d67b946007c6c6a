"""GPU tests (-m gpu): whole SAC updates of the device learner against the float64 autograd reference.

Per case of tests/sac_update_cases.py a learner with all five ``device_*`` options and the case's option is loaded with the case's
parameters and a synthetic ring, and runs three updates with consecutive draws.  Before each update the parameters, moments, step and
leaves are read from the device and the raw batch is fetched with the gather the update will use (a pure function of seed, draw and
ring), so errors do not compound; after it tests/sac_update_reference.py runs on that snapshot in float64 and in float32.

For every quantity X the device exposes -- ``last_update``, the three losses, alpha, both sets of parameter gradients per tensor, the
gradient implied for ``log_ent_coef``, ``actor_d_action``, ``actor_d_log_prob``, norms and clip coefficients, the cloning and advantage
records, PER's ``w``, ``dq`` and ``new_leaf`` -- with e(X) = max|X - X64| / max|X64| (for a loss the denominator is the float64 mean of
the absolute per-row terms) the requirement is

    e(device) <= 8 * max(e(float32 reference), 2^-24).

The yardstick is the reference's own float32 run on the same inputs; nothing of the code under test enters it.  The factor 8 covers
the device's own summation order and its own tanhf, expf and logf.  One quantity carries a derived bound beside it, the gradient of a
critic's head bias (``head_bias_bound``): measured at 10.08 times the yardstick once, for a reason its docstring states.  ``bc_rows``
and ``adv_clipped`` are equal exactly, which is fair because every discrete decision of the float64 run keeps the margin of the cases
(asserted here on the device's snapshots too).

The parameters after the update must be float64 Adam on the snapshot with the DEVICE's gradients and clip coefficient of this update
(``adam_cases.p_bound`` for one step), the target the Polyak blend of those stepped critics (three float32 roundings, DESIGN.md section
11: 3 * 2^-24 max|.|), ``log_ent_coef`` likewise from the device's ``log_prob``: the step count, the gradients consumed, the scale and
the order of step and blend, without comparing Adam's sign-like first step across two gradient computations.

Every line printed is ``case update quantity e(device) e(float32) ratio``; profiles/policy_rollout/gpu_tests_update_reference.txt is a run.
"""
import numpy as np
import pytest
import torch

import sac_update_cases as cases
import sac_update_reference as ref
from adam_cases import p_bound
from sac_update_cases import CAP, CAP_DEMO, CURSOR, CURSOR_DEMO, D, FILLED_DEMO, H, HYPER, N, N_DEMO, PER, UPDATES
from ur_gym_amd import make_vec
from ur_gym_amd.evaluation import DevicePrioritizedReplay, DeviceReplay
from ur_gym_amd.training import SACLearner

pytestmark = pytest.mark.gpu

ALL = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)
FACTOR, FLOOR = 8.0, 2.0 ** -24


def write_ring(replay, ring, cursor, filled):
    for name, a in ring.items():
        replay.ring[name].copy_(torch.from_numpy(a).to(replay.ring[name].device))
    replay.cursor, replay.filled = cursor, filled


def host(w):
    if isinstance(w, dict):
        return {k: host(v) for k, v in w.items()}
    if isinstance(w, (list, tuple)):
        return [host(v) for v in w]
    return w.detach().cpu().numpy().copy()


class Rig:
    """The env, the learner and the ring(s) of one case, loaded from the case's numpy seeds."""

    def __init__(self, name):
        self.name, self.case = name, cases.CASES[name]
        case, o = self.case, dict(self.case["options"])
        own, demo = cases.rings(case)
        self.env = make_vec(case["kind"], num_envs=N, seed=5, auto_reset=True)
        self.env.reset(seed=5)
        self.env_d = self.replay_d = None
        more = {}
        if demo is not None:
            self.env_d = make_vec(case["kind"], num_envs=N_DEMO, seed=6, auto_reset=True)
            self.env_d.reset(seed=6)
            self.replay_d = DeviceReplay(self.env_d, CAP_DEMO)
            write_ring(self.replay_d, demo, CURSOR_DEMO, FILLED_DEMO)
            more = dict(demonstrations=self.replay_d)
        self.learner = SACLearner(self.env, seed=5, hidden_width=H, batch_size=case["M"], learning_starts=0, **ALL, **HYPER, **o, **more)
        if o.get("prioritized"):
            self.replay = DevicePrioritizedReplay(self.env, CAP, alpha=PER["per_alpha"], eps=PER["per_eps"])
        else:
            self.replay = DeviceReplay(self.env, CAP)
        write_ring(self.replay, own, CURSOR, CAP)
        p = cases.parameters(case)
        self.learner.load_parameters(p["actor"], p["critics"], log_ent_coef=float(p["log_ent_coef"]))
        if o.get("prioritized"):
            leaf, max_leaf = cases.leaves(case)
            self.replay.leaf.copy_(torch.from_numpy(leaf).to(self.env.device))
            self.replay.max_leaf.copy_(torch.from_numpy(max_leaf).to(self.env.device))
            self.replay.rebuild()
        self.norm = None
        if o.get("normalize"):
            self.norm = cases.statistics(case, own)
            obs_dim, goal_dim = cases.KINDS[case["kind"]]
            self.learner.normalizer.load_state_dict(dict(num_envs=N, obs_dim=obs_dim, goal_dim=goal_dim, options=self.norm["options"], training=False,
                                                         state=self.norm["state"]))

    def snapshot(self):
        lr = self.learner
        st, es = lr.adam_state, lr.entropy_state
        return dict(actor=host(lr.actor.tensors()), critics=host(lr.critic.tensors()), target=host(lr.target.parameters()), log_ent_coef=host(lr.log_ent_coef)[0],
                    moments=dict(actor=(host(st["actor"][0]), host(st["actor"][1])), critics=(host(st["critic"][0]), host(st["critic"][1])),
                                 ent=(host(es["exp_avg"]), host(es["exp_avg_sq"])), step=int(st["step"])))

    def batch(self, draw):
        """The raw minibatch of `draw`, by the gather call and the arguments the update uses, in the reference's input form."""
        o, M, seed, hp = self.case["options"], self.case["M"], self.case["seed"], self.learner.hp
        more = {}
        if o.get("prioritized"):
            b = self.replay.sample_prioritized(M, seed, draw)
            more = dict(leaf=host(b["leaf"]), total=host(b["total"]), size=float(np.float32(self.replay.filled * N)))
        elif o.get("hindsight"):
            b = self.replay.sample_hindsight(M, seed, draw, n_sampled_goal=hp["her_n_sampled_goal"], strategy=hp["her_strategy"])
        elif int(o.get("n_steps", 1)) > 1:
            b = self.replay.sample(M, seed, draw, n_steps=o["n_steps"], gamma=HYPER["gamma"])
            more = dict(discount=host(b["discount"]))
        elif self.replay_d is not None:
            b = self.replay.sample(M, seed, draw, demonstrations=(self.replay_d, D))
            more = dict(source=host(b["source"]))
        else:
            b = self.replay.sample(M, seed, draw)
        return dict(observations=host(b["observations"]), next_observations=host(b["next_observations"]), actions=host(b["actions"]), rewards=host(b["rewards"]),
                    terminated=host(b["terminated"]).astype(np.uint8), index=host(b["index"]), **more)

    def state(self):
        """Everything an update may leave, for the comparison of the two routes bit for bit."""
        lr, out = self.learner, {}
        snap = self.snapshot()
        for k in ("actor", "critics", "target"):
            out[k] = snap[k]
        out.update(log_ent_coef=snap["log_ent_coef"], moments=[snap["moments"][k] for k in ("actor", "critics", "ent")], step=snap["moments"]["step"],
                   actor_grads=host(lr.actor_grads), critic_grads=host(lr.critic_grads), last={k: host(v) for k, v in lr.last_update.items()})
        if hasattr(self.replay, "leaf"):
            out.update(leaf=host(self.replay.leaf), max_leaf=host(self.replay.max_leaf))
        return out

    def close(self):
        self.learner.close()
        self.env.close()
        if self.env_d is not None:
            self.env_d.close()


def err(x, x64, scale=None):
    x, x64 = np.asarray(x, dtype=np.float64), np.asarray(x64, dtype=np.float64)
    assert x.shape == x64.shape, (x.shape, x64.shape)
    denominator = float(np.max(np.abs(x64))) if scale is None else float(scale)
    diff = float(np.max(np.abs(x - x64)))
    return diff / denominator if denominator > 0 else (0.0 if diff == 0 else np.inf)


def device_quantities(lr, losses, snap):
    """name -> (device value, reference key, loss-scale key or None)."""
    last, es, te = lr.last_update, lr.entropy_state, float(lr.hp["target_entropy"])
    q = {k: (host(last[k]), k, None) for k in ("log_prob", "y", "q", "q_min", "dqmin_da")}
    for k in ("critic_loss", "actor_loss", "ent_coef_loss"):
        q[k] = (host(losses[k]), k, k + "_scale")
    q["ent_coef"] = (host(es["ent_coef"])[0], "ent_coef", None)
    q["d_action"] = (host(lr.actor_d_action), "d_action", None)
    q["d_log_prob"] = (host(lr.actor_d_log_prob), "d_log_prob", None)
    # the gradient the temperature's step consumed is -mean(log pi + target entropy) of the device's own log_prob
    q["ent_grad"] = (-np.mean(host(last["log_prob"]).astype(np.float64) + te), "ent_grad", None)
    for i, w in enumerate(host(lr.critic_grads)):
        for k, g in w.items():
            q[f"critic_grads[{i}].{k}"] = (g, ("critic_grads", i, k), None)
    for k, g in host(lr.actor_grads).items():
        q[f"actor_grads.{k}"] = (g, ("actor_grads", k), None)
    for k in ("critic_grad_norm", "actor_grad_norm", "critic_scale", "actor_scale", "bc_weight", "adv_ess", "adv_max", "w", "dq", "new_leaf"):
        if k in last:
            q[k] = (host(last[k]), k, None)
    if "action_pi" in last:
        q["action_pi"] = (host(last["action_pi"]), "action_pi", None)
    if "q_evaluated" in last:  # PER: the online critics before their step on the batch rows, what the critic loss reads
        q["q_evaluated"] = (host(last["q_evaluated"]), "q", None)
    if "bc_loss" in last:
        q["bc_loss"] = (host(last["bc_loss"])[0], "bc_loss", "bc_loss_scale")
    return q


def pick(out, key):
    if isinstance(key, tuple):
        for k in key:
            out = out[k]
        return out
    return out[key]


def head_bias_bound(r64, r32, net):
    """The bound of the one quantity whose measured ratio exceeded 8 (10.08: the combined case, update 1, net 0): the gradient of a
    critic's head bias, g = sum_m dq_m with dq_m = (q_m - y_m) w_m / M, the one compared quantity that is a single sum of terms of both
    signs -- its own magnitude |g| can be far below sum |dq_m| (normalized rewards centre the TD errors), and e(X) divides by |g|.
    The device adds the dq_m in float64 (urgym_mlp_grad.h, ``lane_sum``), so its error is the terms' own: q_m and y_m are float32 results
    that this test holds within E_q = 8 max(e32(q), 2^-24) max|q64| and E_y likewise of the reference, w_m <= 1, and forming dq_m is two
    more roundings.  Hence |g - g64| <= E_q + E_y + 2 * 2^-24 sum_m |dq64_m|, and e(g) is that over |g64|.  Every number in it is the
    reference's or the yardstick's; nothing is read off the device."""
    E = sum(FACTOR * max(err(r32[k] if k == "y" else r32[k][net], r64[k] if k == "y" else r64[k][net], None), FLOOR) *
            float(np.max(np.abs(r64[k] if k == "y" else r64[k][net]))) for k in ("q", "y"))
    g64 = abs(float(r64["critic_grads"][net]["q_4_bias"].reshape(-1)[0]))
    return (E + 2 * FLOOR * float(np.abs(r64["dq"][net]).sum())) / g64


def check_update(rig, u, lines):
    lr, case = rig.learner, rig.case
    draw = case["draw"] + u
    snap = rig.snapshot()
    batch = rig.batch(draw)
    losses = lr.update(rig.replay, case["seed"], draw)
    torch.cuda.synchronize(rig.env.device)
    inputs = cases.inputs_of(case, snap, batch, draw, rig.norm)
    r64, r32 = ref.run(inputs, torch.float64), ref.run(inputs, torch.float32)
    assert ref.margins_hold(r64["decisions"]) == [], (rig.name, u)
    failures = []
    for name, (value, key, scale_key) in device_quantities(lr, losses, snap).items():
        x64 = pick(r64, key)
        scale = None if scale_key is None else r64[scale_key]
        e_dev, e_32 = err(np.reshape(value, np.shape(x64)), x64, scale), err(pick(r32, key), x64, scale)
        bound = FACTOR * max(e_32, FLOOR)
        if name.endswith(".q_4_bias"):
            bound = max(bound, head_bias_bound(r64, r32, int(key[1])))
        lines.append(f"{rig.name} {u} {name} {e_dev:.3e} {e_32:.3e} {e_dev / max(e_32, FLOOR):.2f}" + (f" bound {bound:.3e}" if bound > FACTOR * max(e_32, FLOOR) else ""))
        if not e_dev <= bound:
            failures.append((name, e_dev, e_32))
    last = lr.last_update
    for k in ("bc_rows", "adv_clipped"):
        if k in last:
            lines.append(f"{rig.name} {u} {k} device {int(host(last[k])[0])} reference {int(r64[k])}")
            if int(host(last[k])[0]) != int(r64[k]):
                failures.append((k, int(host(last[k])[0]), int(r64[k])))
    # the parameters after the update: float64 Adam on the snapshot with the device's own gradients and clip coefficient
    hp, t, after = lr.hp, snap["moments"]["step"] + 1, rig.snapshot()
    lrate, betas, eps = hp["learning_rate"], cases.ADAM["betas"], cases.ADAM["eps"]
    assert after["moments"]["step"] == t
    scales = {k: (host(last[k + "_scale"])[0] if k + "_scale" in last else None) for k in ("critic", "actor")}
    g_actor, g_critic = host(lr.actor_grads), host(lr.critic_grads)
    stepped = []
    for k, p in snap["actor"].items():
        want = ref.adam64(p, g_actor[k], snap["moments"]["actor"][0][k], snap["moments"]["actor"][1][k], lrate, betas, eps, t, scales["actor"])
        stepped.append((f"actor.{k}", after["actor"][k], want, p_bound(1, np.abs(p).max(), lrate)))
    for i in range(2):
        for k, p in snap["critics"][i].items():
            m, v = snap["moments"]["critics"][0][i][k], snap["moments"]["critics"][1][i][k]
            want = ref.adam64(p, g_critic[i][k], m, v, lrate, betas, eps, t, scales["critic"])
            stepped.append((f"critics[{i}].{k}", after["critics"][i][k], want, p_bound(1, np.abs(p).max(), lrate)))
            old, src = snap["target"][i][k].astype(np.float64), after["critics"][i][k].astype(np.float64)
            blend = (1.0 - hp["tau"]) * old + hp["tau"] * src
            stepped.append((f"target[{i}].{k}", after["target"][i][k], blend, 3 * 2.0 ** -24 * max(np.abs(old).max(), np.abs(src).max())))
    g_l = -np.mean(host(last["log_prob"]).astype(np.float64) + float(hp["target_entropy"]))
    want = ref.adam64(snap["log_ent_coef"], g_l, snap["moments"]["ent"][0], snap["moments"]["ent"][1], lrate, betas, eps, t)
    stepped.append(("log_ent_coef", after["log_ent_coef"], want.reshape(()), p_bound(1, abs(float(snap["log_ent_coef"])), lrate)))
    worst = 0.0
    for name, got, want, bound in stepped:
        d = float(np.max(np.abs(got.astype(np.float64) - want)))
        worst = max(worst, d / bound)
        if not d <= bound:
            failures.append((name + " after the step", d, bound))
    lines.append(f"{rig.name} {u} parameters_after worst |p - p64| / bound {worst:.3f}")
    return failures


@pytest.mark.parametrize("name", list(cases.CASES))
def test_three_updates_against_the_float64_reference(name):
    rig, lines, failures = Rig(name), [], []
    try:
        for u in range(UPDATES):
            failures += [(u,) + f for f in check_update(rig, u, lines)]
    finally:
        print("\n".join(lines))
        rig.close()
    assert not failures, failures


def same(a, b, path=""):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), path
        for k in a:
            same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{path}[{i}]")
    elif isinstance(a, np.ndarray):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)), path
    else:
        assert a == b, path


@pytest.mark.parametrize("name", list(cases.CASES))
def test_train_leaves_what_the_three_updates_left(name):
    """The native driver on the same case: ONE ``train`` call of three updates against three ``update`` calls, bit for bit in every
    parameter, moment, gradient, the target, the leaves, the losses and ``last_update`` -- so the reference's result extends to it."""
    a, b = Rig(name), Rig(name)
    case = a.case
    try:
        want = [host(a.learner.update(a.replay, case["seed"], case["draw"] + u)) for u in range(UPDATES)]
        got = host(b.learner.train(b.replay, 1, 0, UPDATES, seed=case["seed"], first_draw=case["draw"]))
        torch.cuda.synchronize(a.env.device)
        for u in range(UPDATES):
            for k in ("critic_loss", "actor_loss", "ent_coef_loss"):
                same(np.asarray(want[u][k]).reshape(()), np.asarray(got[k][u]).reshape(()), f"{name} {u} {k}")
        sa, sb = a.state(), b.state()
        keys = sorted(set(sa["last"]) & set(sb["last"]))  # the two routes name the same records; references to the inputs are update()'s alone
        assert {"log_prob", "y", "q", "q_min", "dqmin_da"} <= set(keys)
        sa["last"], sb["last"] = {k: sa["last"][k].reshape(-1) for k in keys}, {k: sb["last"][k].reshape(-1) for k in keys}
        same(sa, sb, name)
    finally:
        a.close(), b.close()
