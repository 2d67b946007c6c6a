"""GPU tests (-m gpu) of the running observation and reward normalization: urgym_norm_fold, urgym_norm_rows,
urgym_norm_batch, urgym_rollout_collect_normalized, urgym_sac_train_normalized, DeviceNormalizer and SACLearner(normalize=True).

The kernels are compared BIT FOR BIT with evaluation.norm_fold / normalize_rows / normalize_reward, the restatements
tests/test_norm_host.py holds against the header and against exact arithmetic: on synthetic rings the test fills and on the ring a real
collection has written.  The collection is compared with a Python loop of normalize_rows on the bound buffers, policy_actions(rows=) and
step; the learner with the restatement applied to the batch an update gathered, with the Python loop of collect and update on a twin of
the same seeds, and with a twin without the option.  Small shapes: N = 64 envs, H = 32, M = 32 rows, a ring of 4 slots.

The evaluation (urgym_policy_evaluate_normalized) is compared with a closed loop on a twin whose rows the host restatement normalizes,
its best statistics with the record's flag, and inside the training call with the Python sequence of collect, update and evaluate.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from norm_cases import CAP, DEVICE_COUNTS, GAMMA, SPLIT, WHOLE, ring
from test_norm_host import clip_cases
from test_sac_train import ALL, H, N, SEED, STARTS, UPDATE_SEED, Side, assert_same_last_update, assert_same_losses, assert_same_state, bits, guarded, guards_intact
from ur_gym_amd import _abi, make_vec
from test_evaluation import EVAL_SEED, EVAL_STEPS, assert_record, eval_env
from ur_gym_amd.evaluation import DeviceActor, DeviceEvaluation, evaluation_stats, load_best_normalization
from ur_gym_amd.training import host_arrays
from ur_gym_amd.evaluation import NORM_ROW_GROUPS, DeviceMonitor, DevicePrioritizedReplay, DeviceNormalizer, DeviceReplay, norm_fold, norm_initial_state, normalize_reward, normalize_rows
from ur_gym_amd.training import SACLearner

pytestmark = pytest.mark.gpu

STATE = [name for name, _ in _abi.NORM_STATE_FIELDS]
M = 32
NORMALIZED = dict(normalize=True)


def host_state(nz):
    return {k: v.cpu().numpy() for k, v in nz.state.items()}


def assert_state(nz, want, what):
    got = host_state(nz)
    for k in STATE:
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k, got[k][:3], want[k][:3])


def guard(nz):
    """Moves the state and the workspace of `nz` into guarded allocations; returns the guards."""
    dev, g = nz.env.device, {}
    for name in STATE:
        g[name] = guarded(tuple(nz.state[name].shape), torch.float64, dev)
        g[name][1].copy_(nz.state[name])
        nz.state[name] = g[name][1]
        setattr(nz._struct.state, name, C.cast(g[name][1].data_ptr(), C.POINTER(C.c_double)))
    g["workspace"] = guarded(tuple(nz.workspace.shape), torch.float64, dev, 0.0)
    nz.workspace = g["workspace"][1]
    nz._struct.workspace = nz.workspace.data_ptr()
    return g


def reset(nz):
    env = nz.env
    for k, a in norm_initial_state(env.num_envs, env.obs_dim, env.goal_dim).items():
        nz.state[k].copy_(torch.from_numpy(a))


class Synthetic:
    """An environment of n envs that is never stepped, a ring of CAP slots holding norm_cases.ring, and a guarded normalizer."""

    def __init__(self, n, env_id="UR5OriReach-v1", **options):
        self.env = make_vec(env_id, num_envs=n, seed=SEED, auto_reset=True)
        self.replay = DeviceReplay(self.env, CAP)
        self.host = ring(n, 1, self.env.obs_dim, self.env.goal_dim)
        for k, a in self.host.items():
            self.replay.ring[k].copy_(torch.from_numpy(a).to(self.env.device))
        self.nz = DeviceNormalizer(self.env, gamma=GAMMA, fold_steps=CAP, **options)
        self.g = guard(self.nz)

    def run(self, script):
        for first, K in script:
            self.nz.fold(self.replay, first, K)

    def want(self, script, **switches):
        env, st = self.env, norm_initial_state(self.env.num_envs, self.env.obs_dim, self.env.goal_dim)
        for first, K in script:
            st = norm_fold(st, self.host, first, K, GAMMA, **switches)
        return st

    def close(self):
        self.env.close()


def check_fold(n, env_id="UR5OriReach-v1"):
    s = Synthetic(n, env_id)
    dev = s.env.device
    s.run(WHOLE)  # K = 3 from slot 3 (wraps the ring), K = 1, K = C; no synchronise in between
    torch.cuda.synchronize(dev)
    want = s.want(WHOLE)
    assert_state(s.nz, want, (n, "whole"))
    first = host_state(s.nz)
    reset(s.nz)
    s.run(SPLIT)  # the same steps in pieces
    torch.cuda.synchronize(dev)
    assert_state(s.nz, want, (n, "split"))
    # training = 0 launches nothing: every word stays, the workspace's too
    ws = s.nz.workspace.clone()
    s.nz.training = False
    s.run(WHOLE)
    torch.cuda.synchronize(dev)
    assert_state(s.nz, first, (n, "frozen"))
    assert torch.equal(ws, s.nz.workspace)
    assert guards_intact(s.g) is None, guards_intact(s.g)
    print(f"N = {n} {env_id}: observation mean[:3] {want['observation_mean'][:3]}, ret var {want['ret_var'][0]!r}, count {want['ret_count'][0]!r}")
    s.close()


@pytest.mark.parametrize("n", DEVICE_COUNTS)
def test_fold_equals_the_restatement_bitwise(n):
    check_fold(n)


def test_fold_at_65536_envs():
    """512 slabs: 32 per part in the combine kernel, 512 x (K + 1) workgroups in the partial kernel."""
    check_fold(65536)


@pytest.mark.parametrize("env_id", ["UR5ObsReach-v1", "UR5DynReach-v1", "UR5StaReach-v1"])
def test_fold_on_every_env_kind(env_id):
    check_fold(65, env_id)


@pytest.mark.parametrize("switches", [dict(norm_obs=False), dict(norm_reward=False)], ids=["obs-off", "reward-off"])
def test_fold_with_a_group_switched_off(switches):
    s = Synthetic(129, **switches)
    s.run(WHOLE)
    torch.cuda.synchronize(s.env.device)
    want, start = s.want(WHOLE, **switches), norm_initial_state(129, s.env.obs_dim, s.env.goal_dim)
    assert_state(s.nz, want, switches)
    off = [k for k in STATE if (k.startswith("ret") or k == "running_ret") == ("norm_reward" in switches)]
    assert all(want[k].tobytes() == start[k].tobytes() for k in off) and guards_intact(s.g) is None
    s.close()


def test_fold_on_a_ring_a_real_collection_filled():
    side = Side(M=M)
    nz = DeviceNormalizer(side.env, gamma=GAMMA, fold_steps=CAP)
    side.replay.collect(side.learner.device_actor, 6, sample=dict(mode="gaussian", seed=3, first_draw=0))  # wraps: slots 0..3, 0, 1
    nz.fold(side.replay, 2, CAP)  # the four live slots, oldest first
    torch.cuda.synchronize(side.env.device)
    host = {k: side.replay.ring[k].cpu().numpy() for k in ("observation", "achieved_goal", "desired_goal", "reward", "terminated", "truncated")}
    assert_state(nz, norm_fold(norm_initial_state(N, side.env.obs_dim, side.env.goal_dim), host, 2, CAP, GAMMA), "collected ring")
    side.close()


# ------------------------------------------------------------------------------------------------ rows and batch
def folded(n=129):
    s = Synthetic(n)
    s.run(WHOLE)
    return s


@pytest.mark.parametrize("count", (1, 64, 65, 256))
def test_rows_equal_the_restatement_bitwise(count):
    s = folded()
    dev, st = s.env.device, None
    rng = np.random.default_rng(count)
    dims = dict(observation=s.env.obs_dim, achieved_goal=s.env.goal_dim, desired_goal=s.env.goal_dim)
    x = {g: (rng.normal(size=(count, d)) * 10.0 ** rng.integers(-2, 3, d)).astype(np.float32) for g, d in dims.items()}
    x["observation"][0, :3] = (1e30, -1e30, np.float32(1e-41))  # both clip bounds, a subnormal
    rows = {g: torch.from_numpy(a).to(dev) for g, a in x.items()}
    out = s.nz.normalize(rows)                                        # out of place, fresh tensors
    views = {g: guarded((count, d), torch.float32, dev) for g, d in dims.items()}
    for g in dims:
        views[g][1].copy_(rows[g])
    s.nz.normalize({g: v[1] for g, v in views.items()}, out={g: v[1] for g, v in views.items()})  # in place, on views 4 bytes off a 16-byte boundary
    single = {g: s.nz.normalize({g: rows[g]}) for g in dims}          # each group alone: the two others absent
    torch.cuda.synchronize(dev)
    st = host_state(s.nz)
    o = s.nz.options
    for g in dims:
        want = normalize_rows(x[g], st[g + "_mean"], st[g + "_var"], o["epsilon"], o["clip_obs"])
        assert out[g].cpu().numpy().tobytes() == want.tobytes() == views[g][1].cpu().numpy().tobytes() == single[g][g].cpu().numpy().tobytes(), (count, g)
        assert rows[g].cpu().numpy().tobytes() == x[g].tobytes()      # the source of an out-of-place call is not written
    assert out["observation"][0, 0] == 10.0 and out["observation"][0, 1] == -10.0 and guards_intact(views) is None and guards_intact(s.g) is None
    s.close()


def test_rows_hit_both_clip_bounds_exactly():
    env = make_vec("UR5OriReach-v1", num_envs=8, seed=SEED, auto_reset=True)
    x, mean, var, eps, clip = clip_cases()  # [7, 3] for the first three features
    nz = DeviceNormalizer(env, clip_obs=clip, epsilon=eps)
    nz.state["observation_mean"][:3] = torch.from_numpy(mean)
    nz.state["observation_var"][:3] = torch.from_numpy(var)
    rows = np.zeros((7, env.obs_dim), np.float32)
    rows[:, :3] = x
    got = nz.normalize(dict(observation=torch.from_numpy(rows).to(env.device)))["observation"].cpu().numpy()
    st = host_state(nz)
    assert got.tobytes() == normalize_rows(rows, st["observation_mean"], st["observation_var"], eps, clip).tobytes()
    assert np.array_equal(got[0, :3], [10.0] * 3) and np.array_equal(got[1, :3], [-10.0] * 3) and np.array_equal(got[4, :3], [9.5] * 3)
    env.close()


@pytest.mark.parametrize("switches", [{}, dict(norm_obs=False), dict(norm_reward=False), dict(clip_obs=0.5, clip_reward=0.01), dict(clip_obs=np.inf, clip_reward=np.inf, epsilon=0.0)],
                         ids=["defaults", "obs-off", "reward-off", "tight-clips", "no-clips"])
def test_batch_equals_the_restatement_bitwise(switches):
    s = Synthetic(129, **switches)
    s.run(WHOLE)
    s.replay.filled = CAP
    for count in (1, 64, 65, 256):
        batch = s.replay.sample(count, 3, count)
        raw = {k: ({g: v.clone() for g, v in batch[k].items()} if isinstance(batch[k], dict) else batch[k].clone()) for k in batch}
        s.nz.normalize_batch(batch)
        torch.cuda.synchronize(s.env.device)
        st, o = host_state(s.nz), s.nz.options
        for key in ("observations", "next_observations"):
            for g in NORM_ROW_GROUPS:
                x = raw[key][g].cpu().numpy()
                want = normalize_rows(x, st[g + "_mean"], st[g + "_var"], o["epsilon"], o["clip_obs"]) if o["norm_obs"] else x
                assert batch[key][g].cpu().numpy().tobytes() == want.tobytes(), (switches, count, key, g)
        r = raw["rewards"].cpu().numpy()
        want = normalize_reward(r, st["ret_var"], o["epsilon"], o["clip_reward"]) if o["norm_reward"] else r
        assert batch["rewards"].cpu().numpy().tobytes() == want.tobytes(), (switches, count)
        for k in ("actions", "terminated", "truncated", "is_success", "index"):
            assert torch.equal(batch[k], raw[k]), k
    if "clip_reward" in switches and switches["clip_reward"] == 0.01:
        assert (batch["rewards"] == 0.01).any() and (batch["rewards"] == -0.01).any() and (batch["observations"]["observation"] == 0.5).any()
    assert guards_intact(s.g) is None
    s.close()


def test_a_later_fold_changes_the_next_launch_and_not_the_one_before():
    """Stream order: rows, fold, rows without a synchronise; the first result is of the statistics before the fold, the second after."""
    s = Synthetic(65)
    rows = dict(observation=s.replay.ring["observation"][0])
    before = s.nz.normalize(rows)["observation"]
    s.nz.fold(s.replay, 0, 2)
    after = s.nz.normalize(rows)["observation"]
    torch.cuda.synchronize(s.env.device)
    x, o = s.host["observation"][0], s.nz.options
    st0, st1 = norm_initial_state(65, s.env.obs_dim, s.env.goal_dim), s.want([(0, 2)])
    assert before.cpu().numpy().tobytes() == normalize_rows(x, st0["observation_mean"], st0["observation_var"], o["epsilon"], o["clip_obs"]).tobytes()
    assert after.cpu().numpy().tobytes() == normalize_rows(x, st1["observation_mean"], st1["observation_var"], o["epsilon"], o["clip_obs"]).tobytes()
    assert not torch.equal(before, after)
    s.close()


# ------------------------------------------------------------------------------------------------ collection
def test_collect_equals_a_python_loop_of_normalize_rows_policy_actions_and_step():
    K, how = 6, dict(mode="gaussian", seed=29, first_draw=100)
    a, b = Side(M=M), Side(M=M)
    nz = DeviceNormalizer(a.env, gamma=GAMMA, fold_steps=CAP)
    a.replay.collect(a.learner.device_actor, 3, sample=dict(mode="uniform", seed=1, first_draw=0))  # statistics that are not the initial ones
    b.replay.collect(b.learner.device_actor, 3, sample=dict(mode="uniform", seed=1, first_draw=0))
    nz.fold(a.replay, 0, 3)
    torch.cuda.synchronize(a.env.device)
    st, o = host_state(nz), nz.options
    a.replay.collect(a.learner.device_actor, K, sample=how, normalizer=nz)  # from slot 3 on: wraps, the last four steps stay
    torch.cuda.synchronize(a.env.device)
    assert_state(nz, st, "collect folds nothing")
    rows, steps, env = NORM_ROW_GROUPS, [], b.env
    for k in range(K):
        t = {g: env.buf[g].clone() for g in rows}
        seen = {g: torch.from_numpy(normalize_rows(t[g].cpu().numpy(), st[g + "_mean"], st[g + "_var"], o["epsilon"], o["clip_obs"])).to(env.device) for g in rows}
        act, _ = env.policy_actions(b.learner.device_actor, sample=dict(how, first_draw=how["first_draw"] + k), rows=seen)
        obs, rew, term, trunc, info = env.step(act)
        done = (term | trunc)[:, None]
        t["action"], t["reward"] = act.clone(), rew.clone()
        for g in rows:
            t["next_" + g] = torch.where(done, info["final_observation"][g], obs[g])
        t["terminated"], t["truncated"], t["is_success"] = term.view(torch.uint8).clone(), trunc.view(torch.uint8).clone(), info["is_success"].view(torch.uint8).clone()
        steps.append(t)
    torch.cuda.synchronize(a.env.device)
    for k in range(K - CAP, K):
        for key, _, _, _ in _abi.REPLAY_RING_FIELDS:
            assert np.array_equal(bits(a.replay.ring[key][(3 + k) % CAP]), bits(steps[k][key])), (k, key)  # every ring tensor, raw
    for key in ("observation", "achieved_goal", "desired_goal", "reward"):
        assert np.array_equal(bits(a.env.buf[key]), bits(b.env.buf[key])), key
    # and the normalized rows steered the actor: a twin collecting on raw rows answers otherwise
    c = Side(M=M)
    c.replay.collect(c.learner.device_actor, 3, sample=dict(mode="uniform", seed=1, first_draw=0))
    c.replay.collect(c.learner.device_actor, K, sample=how)
    torch.cuda.synchronize(a.env.device)
    assert not torch.equal(c.replay.ring["action"], a.replay.ring["action"])
    for s in (a, b, c):
        s.close()


# ------------------------------------------------------------------------------------------------ the learner
class NormSide(Side):
    """test_sac_train's Side at batch 32 with episodes of at most 3 steps and normalize=True; a monitor on request."""

    def __init__(self, env_id="UR5OriReach-v1", monitored=False, evaluated=False, prioritized=False, **over):
        self.env = make_vec(env_id, num_envs=N, seed=SEED, auto_reset=True, max_episode_steps=3)
        self.env.reset(seed=SEED)
        self.learner = SACLearner(self.env, seed=SEED, hidden_width=H, batch_size=M, learning_starts=STARTS, **dict(ALL, **dict(NORMALIZED, prioritized=prioritized, **over)))
        self.replay = DevicePrioritizedReplay(self.env, 40, alpha=0.6, eps=1e-6) if prioritized else DeviceReplay(self.env, CAP)
        self.mon = None
        self.ev = self.test_env = None
        if monitored:
            self.mon = DeviceMonitor(self.env, capacity=4)
            self.mon.records.fill_(-1)
        if evaluated:
            self.test_env = eval_env(env_id, N)
            self.ev = DeviceEvaluation(self.test_env, self.learner.actor.tensors(), num_steps=EVAL_STEPS, seed=EVAL_SEED, capacity=4, normalizer=self.learner.normalizer)
            self.ev.records.fill_(-1)

    def close(self):
        if self.ev is not None:
            self.ev.close(), self.test_env.close()
        super().close()

    def state(self):
        out = super().state()
        if hasattr(self.replay, "leaf"):
            out.update(leaf=self.replay.leaf, sums=self.replay.sums, max_leaf=self.replay.max_leaf)
        if self.learner.normalizer is not None:
            out.update({f"norm.{k}": v for k, v in self.learner.normalizer.state.items()})
        if self.mon is not None:
            out.update({f"monitor.{k}": v for k, v in self.mon.state.items()}, monitor_records=self.mon.records)
        if self.ev is not None:
            out.update({f"eval.buf.{k}": v for k, v in self.test_env.buf.items()})
            out.update({f"best.{k}": v for k, v in self.ev.best.items()})
            out.update({f"best_norm.{k}": v for k, v in self.ev.best_norm.items()})
            out.update(eval_records=self.ev.records, best_mean=self.ev.best_mean, best_index=self.ev.best_index, eval_packed=self.ev.actor.packed())
        return out


def norm_loop(side, iterations, K, G, first_draw):
    """Side.loop with the monitor's fold and records and the evaluations placed as train places them."""
    lr, losses, draw = side.learner, [], first_draw
    for _ in range(iterations):
        if K:
            lr.collect(side.replay, K, monitor=side.mon)
        before = lr.adam_state["step"]
        if lr.env_steps * N >= lr.hp["learning_starts"]:
            for _ in range(G):
                got = lr.update(side.replay, UPDATE_SEED, draw)
                losses.append({k: v.clone() for k, v in got.items()})
                draw += 1
        if side.mon is not None:
            side.mon.iterations += 1
            if side.mon.iterations % 2 == 0:
                side.mon.record(side.mon.iterations)
        if side.ev is not None and lr.adam_state["step"] // 4 > before // 4:
            side.ev.evaluate(lr.actor.tensors())
    return losses


def same_last_update(a, b, what):
    la, lb = a.learner.last_update, b.learner.last_update
    assert sorted(la) == sorted(lb), (what, sorted(la), sorted(lb))
    for k in la:
        assert la[k].shape == lb[k].shape and np.array_equal(bits(la[k]), bits(lb[k])), (what, k)


def test_update_equals_the_restatement_applied_to_the_gathered_batch():
    """The launches after the gather are the learner's own, so a twin WITHOUT the option whose gathered batch is overwritten with the
    restated normalization (numpy, on the host) must leave the same words.  Both collect CAP warm-up steps first: uniform actions do not
    depend on the rows the actor reads, so the two rings hold the same transitions."""
    a, b = NormSide(), NormSide(normalize=False)
    a.learner.collect(a.replay, CAP)
    b.learner.collect(b.replay, CAP)
    torch.cuda.synchronize(a.env.device)
    for k in a.replay.ring:
        assert np.array_equal(bits(a.replay.ring[k]), bits(b.replay.ring[k])), k
    st, o = host_state(a.learner.normalizer), a.learner.normalizer.options
    assert st["observation_count"][0] == _abi.NORM_INITIAL_COUNT + CAP * N  # collect folded the four slots
    gather = b.replay.sample

    def restated(*args, **kw):
        batch = gather(*args, **kw)
        torch.cuda.synchronize(b.env.device)
        for key in ("observations", "next_observations"):
            for g in NORM_ROW_GROUPS:
                batch[key][g].copy_(torch.from_numpy(normalize_rows(batch[key][g].cpu().numpy(), st[g + "_mean"], st[g + "_var"], o["epsilon"], o["clip_obs"])))
        batch["rewards"].copy_(torch.from_numpy(normalize_reward(batch["rewards"].cpu().numpy(), st["ret_var"], o["epsilon"], o["clip_reward"])))
        return batch

    b.replay.sample = restated
    for draw in (5, 6):
        la, lb = a.learner.update(a.replay, UPDATE_SEED, draw), b.learner.update(b.replay, UPDATE_SEED, draw)
        torch.cuda.synchronize(a.env.device)
        for k in la:
            assert np.array_equal(bits(la[k]), bits(lb[k])), (draw, k)
        assert_same_last_update(a, b, draw)
    assert_state(a.learner.normalizer, st, "update folds nothing")
    nz, a.learner.normalizer = a.learner.normalizer, None  # compare the states both sides have
    assert_same_state(a, b, "two updates")
    a.learner.normalizer = nz
    a.close(), b.close()


def test_train_equals_the_python_loop_and_a_split_call():
    a, b, c = NormSide(), NormSide(), NormSide()
    want = norm_loop(a, 6, 1, 2, first_draw=7)                                            # a: collect / update in Python
    got = b.learner.train(b.replay, 6, 1, 2, seed=UPDATE_SEED, first_draw=7)             # b: ONE native call
    first = c.learner.train(c.replay, 2, 1, 2, seed=UPDATE_SEED, first_draw=7)           # c: the call split in two
    second = c.learner.train(c.replay, 4, 1, 2, seed=UPDATE_SEED, first_draw=7 + 2)
    torch.cuda.synchronize(a.env.device)
    assert len(want) == 10
    assert_same_losses(want, got, "one call")
    assert_same_state(a, b, "one call"), assert_same_last_update(a, b, "one call")
    for k in got:
        assert np.array_equal(bits(got[k]), bits(torch.cat([first[k], second[k]]))), k
    assert_same_state(a, c, "2 + 4 iterations"), assert_same_last_update(a, c, "2 + 4 iterations")
    st = host_state(b.learner.normalizer)
    assert st["observation_count"][0] == _abi.NORM_INITIAL_COUNT + 6 * N and st["ret_count"][0] == st["observation_count"][0]  # idle iterations are folded too
    # normalization is another computation than the learner without it
    d = NormSide(normalize=False)
    other = d.learner.train(d.replay, 6, 1, 2, seed=UPDATE_SEED, first_draw=7)
    torch.cuda.synchronize(a.env.device)
    assert not np.array_equal(bits(other["critic_loss"]), bits(got["critic_loss"])) and d.learner.normalizer is None
    for s in (a, b, c, d):
        s.close()


@pytest.mark.parametrize("option", [dict(n_steps=3), dict(prioritized=True, per_beta=0.4, per_beta_steps=7), dict(hindsight=True), dict(max_grad_norm=0.01), dict(monitored=True, evaluated=True),
                                    dict(evaluated=True, norm_obs=False)],
                         ids=["n_steps", "prioritized", "hindsight", "max_grad_norm", "monitor-and-evaluation", "evaluation-rewards-only"])
def test_train_with_each_other_option(option):
    env_id = "UR5DynReach-v1" if option.get("hindsight") or option.get("prioritized") else "UR5OriReach-v1"
    a, b = NormSide(env_id, **option), NormSide(env_id, **option)
    want = norm_loop(a, 6, 1, 2, first_draw=7)
    extra = {} if b.mon is None else dict(monitor=b.mon, log_every=2)
    extra.update({} if b.ev is None else dict(evaluation=b.ev, eval_every=4))
    got = b.learner.train(b.replay, 6, 1, 2, seed=UPDATE_SEED, first_draw=7, **extra)  # ONE call: urgym_sac_train_normalized with the option
    torch.cuda.synchronize(a.env.device)
    assert len(want) == 10
    assert_same_losses(want, {k: got[k] for k in ("critic_loss", "actor_loss", "ent_coef_loss")}, str(option))
    assert_same_state(a, b, str(option))  # the statistics state among it, and the monitor's
    if "max_grad_norm" not in option:
        same_last_update(a, b, str(option))
    if b.mon is not None:
        assert a.mon.count == b.mon.count == 3
    if b.ev is not None:
        assert a.ev.count == b.ev.count == 2 and a.ev.best_state() == b.ev.best_state() and b.ev.best_state()[1] >= 0
    a.close(), b.close()


def test_identity_statistics_are_the_learner_without_the_option():
    """eps = 0, infinite clips, training off and the initial state forced to mean 0, var 1: (x - 0) * 1 and r * 1 are x and r, so every
    tensor is bit for bit that of a twin without the option."""
    a, b = NormSide(normalize=False), NormSide(norm_epsilon=0.0, clip_obs=float("inf"), clip_reward=float("inf"))
    b.learner.normalizer.training = False
    la = a.loop(4, 1, 2, first_draw=7)
    lb = b.learner.train(b.replay, 4, 1, 2, seed=UPDATE_SEED, first_draw=7)
    torch.cuda.synchronize(a.env.device)
    start = norm_initial_state(N, b.env.obs_dim, b.env.goal_dim)
    assert_state(b.learner.normalizer, start, "frozen")
    nz = b.learner.normalizer
    b.learner.normalizer = None  # compare the states both sides have
    assert_same_losses(la, lb, "identity")
    assert_same_state(a, b, "identity"), assert_same_last_update(a, b, "identity")
    b.learner.normalizer = nz
    assert not set(a.learner._saved_hp()) & {"normalize", "norm_obs", "clip_obs"} and b.learner._saved_hp()["normalize"] is True
    a.close(), b.close()


def test_save_and_load_continue_bit_for_bit(tmp_path):
    a, b = NormSide(), NormSide()
    a.learner.train(a.replay, 6, 1, 2, seed=UPDATE_SEED, first_draw=7)
    b.learner.train(b.replay, 3, 1, 2, seed=UPDATE_SEED, first_draw=7)
    path = tmp_path / "run.npz"
    b.learner.save(path, replay=b.replay, extra=dict(update_draw=7 + b.learner.adam_state["step"]))
    b.close()
    one = NormSide(normalize=False)  # a learner without the option refuses the file, and nothing of it is written
    with pytest.raises(ValueError, match="normalize is True in the checkpoint, False here"):
        one.learner.load(path, replay=one.replay)
    plain = tmp_path / "plain.npz"  # ... and its own checkpoint holds no new key
    one.learner.collect(one.replay, 2)
    one.learner.save(plain, replay=one.replay)
    assert "normalizer" not in one.learner.state_dict() and not any("normaliz" in k or "norm_obs" in k for k in np.load(plain, allow_pickle=False).files)
    with pytest.raises(ValueError, match="normalize is False in the checkpoint, True here"):
        a.learner.check_state_dict(one.learner.state_dict())
    one.close()
    c = NormSide()
    extra = c.learner.load(path, replay=c.replay)
    c.learner.train(c.replay, 3, 1, 2, seed=UPDATE_SEED, first_draw=extra["update_draw"])
    torch.cuda.synchronize(a.env.device)
    assert_same_state(a, c, "3 + 3"), assert_same_last_update(a, c, "3 + 3")
    a.close(), c.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing_and_write_nothing():
    s = Synthetic(65)
    env, nz, lib = s.env, s.nz, s.env.lib
    s.run([(0, 2)])
    torch.cuda.synchronize(env.device)
    before = host_state(nz)
    ws = nz.workspace.clone()
    Z = nz.struct()

    def refused(what, rc, expect):
        assert rc == _abi.ERR_ARG, (what, rc)
        msg = lib.urgym_last_error(env._h).decode()
        assert expect in msg, (what, msg)

    def fold(z=Z, ring=s.replay._ring, first=0, K=1):
        return lib.urgym_norm_fold(env._h, C.byref(z) if z is not None else None, C.byref(ring) if ring is not None else None, first, K, None)

    def edited(**fields):
        z = _abi.Normalization.from_buffer_copy(bytes(Z))
        for k, v in fields.items():
            if k in STATE:
                setattr(z.state, k, v)
            else:
                setattr(z, k, v)
        return z

    refused("null norm", fold(z=None), "null normalization")
    refused("null ring", fold(ring=None), "null ring")
    for name in STATE:
        refused(name, fold(edited(**{name: None})), f"urgym_norm_state.{name} is null")
    odd = C.cast(nz.state["ret_mean"].data_ptr() + 4, C.POINTER(C.c_double))
    refused("misaligned", fold(edited(ret_mean=odd)), "ret_mean must be 8-byte aligned")
    for fields, expect in ((dict(gamma=1.5), "gamma"), (dict(eps=-1.0), "eps"), (dict(clip_obs=0.0), "clip_obs"), (dict(clip_reward=float("nan")), "clip_reward"),
                           (dict(reserved0=1), "reserved0"), (dict(workspace=None), "workspace is null"), (dict(workspace=nz.workspace.data_ptr() + 4), "8-byte aligned"),
                           (dict(workspace_bytes=Z.workspace_bytes // CAP - 8), "workspace_bytes")):
        refused(str(fields), fold(edited(**fields)), expect)
    refused("first_slot", fold(first=CAP), "first_slot outside")
    refused("K = 0", fold(K=0), "num_steps must be positive")
    refused("K > C", fold(K=CAP + 1), "above capacity_steps")
    refused("workspace for fewer steps", fold(edited(workspace_bytes=Z.workspace_bytes // CAP), K=2), "workspace_bytes")
    no_trunc = _abi.ReplayRing.from_buffer_copy(bytes(s.replay._ring))
    no_trunc.truncated = None
    refused("no truncated", fold(ring=no_trunc), "truncated")
    rows = _abi.NormRowsArgs()
    refused("no group", lib.urgym_norm_rows(env._h, C.byref(Z), C.byref(rows), 4, None), "no group")
    rows.observation = C.cast(s.replay.ring["observation"].data_ptr(), C.POINTER(C.c_float))
    refused("no destination", lib.urgym_norm_rows(env._h, C.byref(Z), C.byref(rows), 4, None), "destination")
    rows.observation_out = rows.observation
    refused("count", lib.urgym_norm_rows(env._h, C.byref(Z), C.byref(rows), 0, None), "count must be positive")
    refused("null rows", lib.urgym_norm_rows(env._h, C.byref(Z), None, 1, None), "null rows")
    refused("null batch", lib.urgym_norm_batch(env._h, C.byref(Z), None, 1, None), "null batch")
    refused("batch count", lib.urgym_norm_batch(env._h, C.byref(Z), C.byref(_abi.ReplayBatch()), 0, None), "count must be positive")
    n = C.c_uint64(0)
    refused("workspace steps", lib.urgym_norm_workspace(env._h, 0, C.byref(n)), "num_steps must be positive")
    assert lib.urgym_norm_workspace(env._h, CAP, C.byref(n)) == 0 and n.value == Z.workspace_bytes == 8 * CAP * 1 * 2 * (env.obs_dim + 2 * env.goal_dim + 1)
    for bad in (dict(first_slot=CAP, num_steps=1), dict(first_slot=0, num_steps=CAP + 1)):
        with pytest.raises(ValueError):
            nz.fold(s.replay, **bad)
    with pytest.raises(ValueError, match="DeviceNormalizer of this environment"):
        env.norm_fold(object(), s.replay, 0, 1)
    torch.cuda.synchronize(env.device)
    assert_state(nz, before, "after the refusals")
    assert torch.equal(ws, nz.workspace) and guards_intact(s.g) is None
    # an env without auto_reset has no normalizer, and the entry point refuses it too
    plain = make_vec("UR5OriReach-v1", num_envs=8, seed=SEED, auto_reset=False)
    with pytest.raises(ValueError, match="auto_reset"):
        DeviceNormalizer(plain)
    plain.close()
    s.close()


def test_training_call_refusals():
    a = NormSide()
    lr, env = a.learner, a.env
    with pytest.raises(ValueError, match="fold_steps"):
        lr.collect(a.replay, lr.normalizer.fold_steps + 1)
    before = {k: bits(v).copy() for k, v in a.state().items()}
    small = DeviceNormalizer(env, fold_steps=1)
    lr.normalizer, keep = small, lr.normalizer
    with pytest.raises(ValueError, match="fold_steps"):
        lr.train(a.replay, 2, 2, 1, seed=UPDATE_SEED, first_draw=0)
    lr.normalizer = keep
    tr = lr._train_binding(a.replay)
    L, S = tr["binding"].struct, _abi.SacSchedule()
    assert env.lib.urgym_sac_train_normalized(env._h, C.byref(L), C.byref(S), None, None, None, None, None, None, None, None) == _abi.ERR_ARG
    assert b"null normalization" in env.lib.urgym_last_error(env._h)
    test_env = eval_env("UR5OriReach-v1", N)
    plain = DeviceEvaluation(test_env, lr.actor.tensors(), num_steps=EVAL_STEPS, seed=EVAL_SEED, capacity=4)  # made without the normalizer
    with pytest.raises(ValueError, match="share one normalizer"):
        lr.train(a.replay, 2, 1, 1, seed=UPDATE_SEED, first_draw=0, evaluation=plain, eval_every=1)
    plain.close(), test_env.close()
    torch.cuda.synchronize(env.device)
    after = a.state()
    assert all(np.array_equal(before[k], bits(after[k])) for k in before)
    a.close()


# ------------------------------------------------------------------------------------------------ evaluation with the training statistics
def restated_closed_loop(env, actor, st, o, steps):
    """The episode of every env of `env` under `actor` on rows the HOST restatement normalizes, summed as the rollout's summary sums it
    (rewards while it runs, closed at `terminated` or at the last step): what run_closed_loop_device returns."""
    n = env.num_envs
    ret, alive, ok, last = np.zeros(n), np.ones(n, bool), np.zeros(n, bool), np.full(n, steps - 1.0)
    for k in range(steps):
        rows = {g: torch.from_numpy(normalize_rows(env.buf[g].cpu().numpy(), st[g + "_mean"], st[g + "_var"], o["epsilon"], o["clip_obs"])).to(env.device)
                for g in NORM_ROW_GROUPS}
        _, rew, term, trunc, info = env.step(env.policy_actions(actor, rows=rows))
        done = alive & (term.cpu().numpy() | (k == steps - 1))
        ret += np.where(alive, rew.cpu().numpy().astype(np.float64), 0.0)
        ok |= done & info["is_success"].cpu().numpy()
        last[done] = k
        alive &= ~done
    return dict(reward=ret, success=ok, last_step=last)


def test_evaluate_normalized_equals_a_restated_closed_loop_and_the_best_state_follows_the_flag(tmp_path):
    """urgym_policy_evaluate_normalized on a second environment with the TRAINING environment's statistics (sync_envs_normalization):
    every record against a closed loop on a twin whose rows the host restatement normalizes; the best statistics are those of the
    evaluation whose record says `improved`, and stay where it does not; save_best writes them and the loader reads them back."""
    from ur_gym_amd.evaluation import run_closed_loop_device

    side, n, steps = Side(M=M), 48, 12
    nz = DeviceNormalizer(side.env, gamma=GAMMA, fold_steps=CAP)
    actor = side.learner.device_actor
    side.replay.collect(actor, CAP, sample=dict(mode="uniform", seed=1, first_draw=0))
    nz.fold(side.replay, 0, 2)
    torch.cuda.synchronize(side.env.device)
    make = lambda: make_vec("UR5OriReach-v1", num_envs=n, seed=EVAL_SEED, auto_reset=False)  # noqa: E731
    test_env, twin = make(), make()
    w = host_arrays(side.learner.actor.tensors())
    source = {k: v.detach().clone() for k, v in side.learner.actor.tensors().items()}
    ev = DeviceEvaluation(test_env, {k: np.zeros_like(v) for k, v in w.items()}, num_steps=steps, seed=EVAL_SEED, capacity=3, normalizer=nz)
    twin_actor = DeviceActor(w, twin)
    stats, o, best_mean, best_index, best_stats = [], nz.options, -np.inf, -1, None
    for i in range(3):
        if i == 1:
            nz.fold(side.replay, 2, 2)  # other statistics for the second evaluation; the third repeats the second
        assert ev.evaluate(source) == i  # not synchronised: the statistics are read when the launches run
        torch.cuda.synchronize(side.env.device)
        st = host_state(nz)
        stats.append(st)
        twin.buf["observation"].zero_()
        twin.reset(seed=EVAL_SEED)
        res = restated_closed_loop(twin, twin_actor, st, o, steps)
        want = evaluation_stats(res["reward"], res["last_step"].astype(np.int32), res["success"], best_mean, best_index, i)
        got = ev.results()[i]
        assert_record(got, want, i)
        if got["improved"]:
            best_stats = st
        best_mean, best_index = want["best_mean"], want["best_index"]
        for k, v in ev.best_norm.items():  # the best state follows the flag
            assert v.cpu().numpy().tobytes() == best_stats[k].tobytes(), (i, k, got["improved"])
        for k in test_env.buf:
            assert np.array_equal(bits(test_env.buf[k]), bits(twin.buf[k])), (i, k)
        # the Python route an evaluation environment has as well
        twin.buf["observation"].zero_()
        twin.reset(seed=EVAL_SEED)
        loop = run_closed_loop_device(twin, twin_actor, max_steps=steps, normalizer=nz)
        assert loop["reward"].tobytes() == res["reward"].tobytes() and np.array_equal(loop["success"], res["success"]) and np.array_equal(loop["last_step"], res["last_step"])
    flags = [r["improved"] for r in ev.results()]
    assert flags[0] == 1 and flags[2] == 0, flags  # from -inf; a repeat of the second evaluation is never strictly above
    assert stats[0]["observation_mean"].tobytes() != stats[1]["observation_mean"].tobytes() and stats[1]["ret_var"].tobytes() == stats[2]["ret_var"].tobytes()
    assert_state(nz, stats[2], "an evaluation folds nothing")
    for k in source:
        assert np.array_equal(bits(ev.best[k]), bits(source[k])), k
    # save_best, the loader, and the reader of the actor that exists
    path = str(tmp_path / "best_model.npz")
    ev.save_best(path)
    state, options = load_best_normalization(path)
    assert options == o and sorted(state) == sorted(ev.best_norm) and all(state[k].tobytes() == best_stats[k].tobytes() and state[k].dtype == np.float64 for k in state)
    back = DeviceActor.load(path, twin)
    assert np.array_equal(back.packed().view(np.uint8), twin_actor.packed().view(np.uint8))
    # the state_dict carries the best statistics; an evaluation without a normalizer writes none and refuses such a state
    other_env = make()
    other = DeviceEvaluation(other_env, w, num_steps=steps, seed=EVAL_SEED, capacity=3, normalizer=nz)
    other.load_state_dict(ev.state_dict())
    assert all(other.best_norm[k].cpu().numpy().tobytes() == best_stats[k].tobytes() for k in other.best_norm) and other.count == 3
    bare = DeviceEvaluation(other_env, w, num_steps=steps, seed=EVAL_SEED, capacity=3)
    with pytest.raises(ValueError, match="no normalizer"):
        bare.load_state_dict(ev.state_dict())
    bare.evaluate(source)
    bare.save_best(path)
    assert load_best_normalization(path) is None and "best_norm" not in bare.state_dict() and sorted(np.load(path).files) == sorted(w)
    # refusals: nothing launched, nothing written
    before = bits(ev.records).copy()
    ev.count = 2  # a free record
    Z = ev.norm_struct()
    for fields, expect in ((dict(eval_scratch=None), "eval_scratch is null"), (dict(best_state=None), "null destination state"), (dict(clip_obs=0.0), "clip_obs")):
        z = _abi.Normalization.from_buffer_copy(bytes(Z))
        for k, v in fields.items():
            setattr(z, k, v)
        assert test_env.lib.urgym_policy_evaluate_normalized(test_env._h, C.byref(ev.struct(source)), C.byref(z), 2, 2, None) == _abi.ERR_ARG, fields
        assert expect in test_env.lib.urgym_last_error(test_env._h).decode(), (fields, test_env.lib.urgym_last_error(test_env._h))
    assert test_env.lib.urgym_policy_evaluate_normalized(test_env._h, C.byref(ev.struct(source)), None, 2, 2, None) == _abi.ERR_ARG
    torch.cuda.synchronize(side.env.device)
    assert np.array_equal(before, bits(ev.records))
    with pytest.raises(ValueError, match="DeviceNormalizer of this environment"):
        test_env.collect(ev.actor, 1, DeviceReplay(test_env, 2), normalizer=nz)  # only rows and evaluations take another environment's statistics
    dyn = make_vec("UR5DynReach-v1", num_envs=8, seed=SEED, auto_reset=False)
    with pytest.raises(ValueError, match="DeviceNormalizer of this environment"):
        dyn.norm_rows(nz, dict(observation=dyn.buf["observation"]))
    with pytest.raises(ValueError, match="kind and device"):
        DeviceEvaluation(dyn, random_like(dyn), normalizer=nz)
    for x in (back, twin_actor, ev, other, bare):
        x.close()
    for e in (dyn, other_env, test_env, twin):
        e.close()
    side.close()


def random_like(env):
    from test_evaluation import random_actor
    return random_actor(env.env_id, H, 3)


def test_snapshot_copies_under_the_flag_and_only_then():
    s = Synthetic(65)
    s.run([(0, 2)])
    env, dev = s.env, s.env.device
    dst = {k: guarded(tuple(v.shape), torch.float64, dev, -7.0) for k, v in s.nz.state.items() if k != "running_ret"}
    D = _abi.NormState()
    for k, (_, view) in dst.items():
        setattr(D, k, C.cast(view.data_ptr(), C.POINTER(C.c_double)))
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    call = lambda when: env.lib.urgym_norm_snapshot(env._h, C.byref(s.nz._struct.state), C.byref(D), when, None)  # noqa: E731
    assert call(C.c_void_p(flag.data_ptr())) == 0
    torch.cuda.synchronize(dev)
    assert all(bool((view == -7.0).all()) for _, view in dst.values())  # the flag holds 0: nothing is written
    flag.fill_(1)
    assert call(C.c_void_p(flag.data_ptr())) == 0
    torch.cuda.synchronize(dev)
    st = host_state(s.nz)
    assert all(view.cpu().numpy().tobytes() == st[k].tobytes() for k, (_, view) in dst.items())
    for _, view in dst.values():
        view.fill_(-7.0)
    assert call(None) == 0  # no flag: always
    torch.cuda.synchronize(dev)
    assert all(view.cpu().numpy().tobytes() == st[k].tobytes() for k, (_, view) in dst.items()) and guards_intact(dst) is None and guards_intact(s.g) is None
    assert env.lib.urgym_norm_snapshot(env._h, None, C.byref(D), None, None) == _abi.ERR_ARG and env.lib.urgym_norm_snapshot(env._h, C.byref(D), None, None, None) == _abi.ERR_ARG
    D.ret_var = None
    assert call(None) == _abi.ERR_ARG and b"destination state" in env.lib.urgym_last_error(env._h)
    s.close()
