"""GPU tests (-m gpu) of the multi-step returns: urgym_replay_sample_nstep, urgym_sac_entropy_step_nstep,
urgym_sac_train_nstep and SACLearner(n_steps=).

Everything is compared BIT FOR BIT: the gather with evaluation.nstep_batch on synthetic rings (tests/nstep_cases.py: every ring state,
every kind of window, payloads of NaNs, -0.0f and denormals, one NaN reward) and on rings a real collection filled; the entropy step
with evaluation.entropy_step_nstep and, with discount = gamma, with today's two calls; the training call with the Python loop of
``collect`` / ``update``.  Small shapes throughout; the one large count is the entropy step's cap of 65,536 rows.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from nstep_cases import CAPACITY, COUNTS, DRAW, GAMMA, N_STEPS, NUM_ENVS, RING_STATES, SEED as DRAW_SEED, entropy_inputs, same_bits, synthetic_ring
from test_evaluation import EVAL_SEED, EVAL_STEPS, eval_env, random_actor
from test_monitor import MonitoredEvaluated, assert_same_monitor
from test_sac_train import ALL, CAP, H, N, SEED, STARTS, UPDATE_SEED, Side, assert_same_last_update, assert_same_losses, assert_same_state, bits, guarded, guards_intact
from ur_gym_amd import _abi, make_vec
from ur_gym_amd._native import NativeError
from ur_gym_amd.evaluation import (DeviceActor, DeviceCritic, DeviceEvaluation, DeviceMonitor, DeviceReplay, adam_coefficients, entropy_step_nstep,
                                   nstep_batch)
from ur_gym_amd.training import SACLearner, TorchTwinCritic, host_arrays

pytestmark = pytest.mark.gpu

EXTRA = {"discount": torch.float32, "steps": torch.int32, "last_index": torch.int64}
ADAM = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, step=3)
TARGET_ENTROPY = -6.0


def batch_kinds(env):
    from ur_gym_amd.vector_env import _TORCH_DTYPE

    kinds = {name: (_TORCH_DTYPE[ct], tuple(shape(1, 1, env.obs_dim, env.goal_dim)[2:])) for name, ct, shape, _ in _abi.REPLAY_RING_FIELDS}
    kinds["index"] = (torch.int64, ())
    kinds.update({k: (dt, ()) for k, dt in EXTRA.items()})
    return kinds


def guarded_batch(env, count, names=None):
    """name -> (flat, view) of guarded outputs, filled with a pattern no ring holds."""
    return {name: guarded((count,) + tail, dt, env.device, 85) for name, (dt, tail) in batch_kinds(env).items() if names is None or name in names}


def views(g, nstep=True):
    return {k: v[1] for k, v in g.items() if nstep or k not in EXTRA}


def upload(replay, ring, filled, oldest):
    for k, a in ring.items():
        replay.ring[k].copy_(torch.from_numpy(a))
    replay.filled, replay.cursor = filled, (oldest + filled) % replay.capacity
    assert replay.oldest_slot == oldest


def ring_arrays(replay):
    return {k: v.cpu().numpy() for k, v in replay.ring.items()}


def assert_batch(g, want, where):
    for name, (_, view) in g.items():
        assert same_bits(view.cpu().numpy(), want[name]), (where, name)
    assert guards_intact(g) is None, (where, guards_intact(g))


# ------------------------------------------------------------------------------------------------ 1. the gather on synthetic rings
@pytest.mark.parametrize("num_envs", NUM_ENVS)
def test_gather_equals_the_restatement_bitwise(num_envs):
    env = make_vec("UR5OriReach-v1", num_envs=num_envs, seed=SEED, auto_reset=True)
    env.reset(seed=SEED)
    replay = DeviceReplay(env, CAPACITY)
    ring = synthetic_ring(num_envs, env.obs_dim, env.goal_dim)
    assert np.isnan(ring["reward"]).sum() == 1
    outs = {count: guarded_batch(env, count) for count in COUNTS}
    for filled, oldest in RING_STATES:
        upload(replay, ring, filled, oldest)
        for n in N_STEPS:
            for count in COUNTS:
                where, g = (num_envs, filled, oldest, n, count), outs[count]
                replay.sample_into(views(g), DRAW_SEED, DRAW, n_steps=n, gamma=GAMMA)
                want = nstep_batch(ring, oldest, filled, DRAW_SEED, DRAW, count, n, GAMMA)
                assert_batch(g, want, where)
                if n == 1:  # every batch output is urgym_replay_sample's, and the discount is gamma itself
                    one = guarded_batch(env, count, names=[k for k in g if k not in EXTRA])
                    replay.sample_into(views(one), DRAW_SEED, DRAW)
                    for name, (_, view) in one.items():
                        assert np.array_equal(bits(view), bits(g[name][1])), (where, name)
                    assert same_bits(g["discount"][1].cpu().numpy(), np.full(count, np.float32(GAMMA)))
        # a second call gives the same bits, and outputs that are not asked for are not written
        first = {k: v[1].clone() for k, v in g.items()}
        replay.sample_into(views(g), DRAW_SEED, DRAW, n_steps=n, gamma=GAMMA)
        assert all(np.array_equal(bits(first[k]), bits(g[k][1])) for k in g), (filled, oldest)
        few = guarded_batch(env, COUNTS[-1])
        asked = ("reward", "discount", "next_desired_goal")
        replay.sample_into({k: few[k][1] for k in asked}, DRAW_SEED, DRAW, n_steps=3, gamma=GAMMA)
        want = nstep_batch(ring, oldest, filled, DRAW_SEED, DRAW, COUNTS[-1], 3, GAMMA)
        for k, (flat, view) in few.items():
            if k in asked:
                assert same_bits(view.cpu().numpy(), want[k]), k
            else:
                assert (view == 85).all(), k
        assert guards_intact(few) is None
    # the ring is unchanged
    for k, a in ring.items():
        assert same_bits(replay.ring[k].cpu().numpy(), a), k
    # a row depends on (seed, draw, i) and the ring only: the first rows of a longer batch are the shorter batch
    short, long = guarded_batch(env, COUNTS[1]), guarded_batch(env, COUNTS[3])
    replay.sample_into(views(short), DRAW_SEED, DRAW, n_steps=5, gamma=GAMMA)
    replay.sample_into(views(long), DRAW_SEED, DRAW, n_steps=5, gamma=GAMMA)
    assert all(np.array_equal(bits(short[k][1]), bits(long[k][1][:COUNTS[1]])) for k in short)
    env.close()


# ------------------------------------------------------------------------------------------------ 2. rings a real collection filled
@pytest.mark.parametrize("env_id,num_envs", [("UR5DynReach-v1", 65), ("UR5OriReach-v1", 33)])
def test_gather_on_a_collected_ring(env_id, num_envs):
    env = make_vec(env_id, num_envs=num_envs, seed=SEED, auto_reset=True, max_episode_steps=8)
    env.reset(seed=SEED)
    actor = DeviceActor(random_actor(env_id, H, SEED), env)
    replay = DeviceReplay(env, 12)
    replay.collect(actor, 20, sample=dict(mode="uniform", seed=SEED, first_draw=0))
    assert replay.filled == 12 and replay.cursor == 8 and replay.oldest_slot == 8  # wrapped
    ring = ring_arrays(replay)
    assert ring["truncated"].any()  # episodes are cut at 8 steps: a window must stop there
    stopped = 0
    for n in (1, 3, 5):
        g = guarded_batch(env, 130)
        replay.sample_into(views(g), DRAW_SEED, DRAW + n, n_steps=n, gamma=GAMMA)
        want = nstep_batch(ring, replay.oldest_slot, replay.filled, DRAW_SEED, DRAW + n, 130, n, GAMMA)
        assert_batch(g, want, (env_id, n))
        stopped += int(((want["steps"] < n) & (want["truncated"] != 0)).sum())
    assert stopped > 0  # some window did stop at a truncation before its n steps
    for k, a in ring.items():
        assert same_bits(replay.ring[k].cpu().numpy(), a), k
    # DeviceReplay.sample returns the three new tensors beside the batch
    got = replay.sample(64, DRAW_SEED, DRAW, n_steps=3, gamma=GAMMA)
    want = nstep_batch(ring, replay.oldest_slot, replay.filled, DRAW_SEED, DRAW, 64, 3, GAMMA)
    assert all(same_bits(got[k].cpu().numpy(), want[k]) for k in EXTRA) and same_bits(got["rewards"].cpu().numpy(), want["reward"])
    assert same_bits(got["next_observations"]["observation"].cpu().numpy(), want["next_observation"])
    actor.close(), env.close()


# ------------------------------------------------------------------------------------------------ 3. the entropy step
@pytest.fixture(scope="module")
def small_env():
    env = make_vec("UR5OriReach-v1", num_envs=4, seed=SEED, auto_reset=True)
    env.reset(seed=SEED)
    yield env
    env.close()


def entropy_call(env, x, count, discount=None, y_is_reward=False):
    """One urgym_sac_entropy_step_nstep on guarded tensors.  Returns (the guarded pairs, the restatement's dict)."""
    dev = env.device
    g = {k: guarded((count,), torch.float32, dev, 0.0) for k in ("log_prob", "reward", "q_min_next", "discount", "next_log_prob", "y", "d_log_prob")}
    g["terminated"] = guarded((count,), torch.uint8, dev, 0)
    for k in ("l", "m", "v", "ent_coef", "loss"):
        g[k] = guarded((1,), torch.float32, dev, 0.0)
    x = dict(x, discount=x["discount"] if discount is None else discount)
    for k in ("log_prob", "reward", "q_min_next", "discount", "next_log_prob", "terminated", "l", "m", "v"):
        g[k][1].copy_(torch.from_numpy(np.asarray(x[k]).reshape(g[k][1].shape)))
    y_out = g["reward"][1] if y_is_reward else g["y"][1]
    env.entropy_step_nstep((g["l"][1], g["m"][1], g["v"][1]), g["log_prob"][1], TARGET_ENTROPY, ent_coef_out=g["ent_coef"][1], loss_out=g["loss"][1],
                           reward=g["reward"][1], q_min_next=g["q_min_next"][1], discount=g["discount"][1], next_log_prob=g["next_log_prob"][1],
                           terminated=g["terminated"][1], y_out=y_out, d_log_prob_out=g["d_log_prob"][1], scale=1.0 / count, **ADAM)
    alpha = g["ent_coef"][1].cpu().numpy()[0]  # the device's expf: an input of the restatement
    want = entropy_step_nstep(alpha, x["log_prob"], TARGET_ENTROPY, x["l"], x["m"], x["v"], adam_coefficients(env, **ADAM), reward=x["reward"],
                              q_min_next=x["q_min_next"], discount=x["discount"], next_log_prob=x["next_log_prob"], terminated=x["terminated"], scale=1.0 / count)
    return g, want, alpha


@pytest.mark.parametrize("count", [1, 1023, 1025, 65536])
def test_entropy_step_equals_the_restatement_bitwise(small_env, count):
    x = entropy_inputs(count)
    g, want, alpha = entropy_call(small_env, x, count)
    assert abs(float(alpha) - float(np.exp(np.float64(x["l"])))) <= 2 * float(np.spacing(alpha))  # expf within its ulp
    got = {k: g[k][1].cpu().numpy() for k in g}
    assert same_bits(got["y"], want["y"]) and same_bits(got["d_log_prob"], want["d_log_prob"])
    assert same_bits(got["l"], want["l"]) and same_bits(got["m"], want["m"]) and same_bits(got["v"], want["v"])
    assert same_bits(got["loss"], np.asarray(want["loss"], np.float32).reshape(1))
    assert np.isfinite(got["y"]).all() and guards_intact(g) is None, guards_intact(g)
    for k in ("log_prob", "reward", "q_min_next", "discount", "next_log_prob"):  # the inputs are read only
        assert same_bits(got[k], x[k]), k
    # y_out may be reward itself; and one NaN next_log_prob row reaches that y row and no other (which NaN it is -- the sign a negated
    # operand leaves -- is the one thing the two sides need not share, so that row is compared as a NaN and every other row bitwise)
    x["next_log_prob"][count // 2] = np.nan
    g2, want2, _ = entropy_call(small_env, x, count, y_is_reward=True)
    y2, others = g2["reward"][1].cpu().numpy(), np.arange(count) != count // 2
    assert np.isnan(y2).tolist() == [i == count // 2 for i in range(count)] and np.isnan(want2["y"][count // 2])
    assert same_bits(y2[others], want2["y"][others]) and same_bits(y2[others], want["y"][others])
    assert not g2["y"][1].any() and guards_intact(g2) is None
    for k in ("l", "m", "v", "loss"):  # the step itself does not see the target group
        assert same_bits(g2[k][1].cpu().numpy(), got[k]), k


def test_entropy_step_with_gamma_as_discount_is_todays_two_calls(small_env):
    env, count, dev = small_env, 1025, small_env.device
    torch.manual_seed(3)
    critic = DeviceCritic(host_arrays(TorchTwinCritic(env.obs_dim + 2 * env.goal_dim + 6, H).tensors()), env)
    rows = {"observation": torch.randn((count, env.obs_dim), device=dev), "achieved_goal": torch.randn((count, env.goal_dim), device=dev),
            "desired_goal": torch.randn((count, env.goal_dim), device=dev)}
    actions = torch.rand((count, 6), device=dev) * 2 - 1
    x = entropy_inputs(count)
    t = {k: torch.from_numpy(x[k]).to(dev) for k in ("log_prob", "reward", "next_log_prob", "terminated")}
    state = lambda: tuple(torch.from_numpy(np.asarray(x[k], np.float32).reshape(1)).to(dev) for k in ("l", "m", "v"))  # noqa: E731
    scalar = lambda: torch.zeros((1,), dtype=torch.float32, device=dev)  # noqa: E731
    # today: urgym_critic_evaluate(target, ent_coef = 0), then urgym_sac_entropy_step
    old = env.critic_values(critic, actions, rows=rows, reward=t["reward"], terminated=t["terminated"], log_prob=t["next_log_prob"], gamma=GAMMA, ent_coef=0.0)
    y_old, s_old, a_old = torch.zeros(count, device=dev), state(), scalar()
    env.entropy_step(s_old, t["log_prob"], TARGET_ENTROPY, ent_coef_out=a_old, target=old["target"], next_log_prob=t["next_log_prob"],
                     terminated=t["terminated"], gamma=GAMMA, y_out=y_old, **ADAM)
    # the new pair: q_min alone, then the step with a discount that is gamma on every row
    q_min = env.critic_values(critic, actions, rows=rows)["q_min"]
    y_new, s_new, a_new = torch.zeros(count, device=dev), state(), scalar()
    env.entropy_step_nstep(s_new, t["log_prob"], TARGET_ENTROPY, ent_coef_out=a_new, reward=t["reward"], q_min_next=q_min,
                           discount=torch.full((count,), GAMMA, dtype=torch.float32, device=dev), next_log_prob=t["next_log_prob"],
                           terminated=t["terminated"], y_out=y_new, **ADAM)
    assert np.array_equal(bits(q_min), bits(old["q_min"])) and np.array_equal(bits(y_new), bits(y_old)) and np.array_equal(bits(a_new), bits(a_old))
    assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(s_new, s_old)) and torch.isfinite(y_new).all()
    critic.close()


# ------------------------------------------------------------------------------------------------ 4. the learner
class NSide(Side):
    """test_sac_train's Side on UR5DynReach-v1 with batch 96 and three-step returns."""

    def __init__(self, **over):
        super().__init__("UR5DynReach-v1", M=96, **dict(dict(n_steps=3), **over))


def test_train_equals_the_python_loop_bit_for_bit():
    a, b, c = NSide(), NSide(), NSide()
    want = a.loop(6, 1, 2, first_draw=7)                                                 # a: collect / update in Python
    got = b.learner.train(b.replay, 6, 1, 2, seed=UPDATE_SEED, first_draw=7)             # b: ONE native call
    first = c.learner.train(c.replay, 2, 1, 2, seed=UPDATE_SEED, first_draw=7)           # c: the call split in two
    second = c.learner.train(c.replay, 4, 1, 2, seed=UPDATE_SEED, first_draw=7 + 2)
    torch.cuda.synchronize(a.env.device)
    assert len(want) == 10 and b.replay.filled == CAP and b.replay.cursor == 2  # the ring wrapped under the updates
    assert_same_losses(want, got, "one call")
    assert_same_state(a, b, "one call"), assert_same_last_update(a, b, "one call")
    for k in got:
        assert np.array_equal(bits(got[k]), bits(torch.cat([first[k], second[k]]))), k
    assert_same_state(a, c, "2 + 4 iterations"), assert_same_last_update(a, c, "2 + 4 iterations")
    assert np.isfinite(bits(got["critic_loss"]).view(np.float32)).all()
    # three-step returns are another computation than one-step ones
    d = NSide(n_steps=1)
    other = d.learner.train(d.replay, 6, 1, 2, seed=UPDATE_SEED, first_draw=7)
    torch.cuda.synchronize(a.env.device)
    assert not np.array_equal(bits(other["critic_loss"]), bits(got["critic_loss"]))
    for s in (a, b, c, d):
        s.close()


class NMonitoredEvaluated(MonitoredEvaluated):
    """test_monitor's MonitoredEvaluated on UR5DynReach-v1 with batch 96 and three-step returns (episodes of at most 3 steps)."""

    def __init__(self, capacity=4):
        self.env = make_vec("UR5DynReach-v1", num_envs=N, seed=SEED, auto_reset=True, max_episode_steps=3)
        self.env.reset(seed=SEED)
        self.learner = SACLearner(self.env, seed=SEED, hidden_width=H, batch_size=96, learning_starts=STARTS, **dict(ALL, n_steps=3))
        self.replay = DeviceReplay(self.env, CAP)
        self.mon = DeviceMonitor(self.env, capacity=capacity)
        self.mon.records.fill_(-1)
        self.test_env = eval_env("UR5DynReach-v1", N)
        self.ev = DeviceEvaluation(self.test_env, self.learner.actor.tensors(), num_steps=EVAL_STEPS, seed=EVAL_SEED, capacity=4)
        self.ev.records.fill_(-1)


def test_train_with_a_monitor_and_an_evaluation_attached():
    a, b = NMonitoredEvaluated(), NMonitoredEvaluated()
    got = a.train(6, first_draw=7, evaluation=a.ev, eval_every=4)  # ONE call: urgym_sac_train_nstep with both
    want, draw = [], 7                                             # the Python loop with the fold, the records and the evaluations
    for _ in range(6):
        b.learner.collect(b.replay, 1, monitor=b.mon)
        before = b.learner.adam_state["step"]
        if b.learner.env_steps * N >= STARTS:
            for _ in range(2):
                want.append({k: v.clone() for k, v in b.learner.update(b.replay, UPDATE_SEED, draw).items()})
                draw += 1
        b.mon.iterations += 1
        if b.mon.iterations % 2 == 0:
            b.mon.record(b.mon.iterations)
        if b.learner.adam_state["step"] // 4 > before // 4:
            b.ev.evaluate(b.learner.actor.tensors())
    torch.cuda.synchronize(a.env.device)
    assert_same_losses(want, got, "monitor and evaluation")
    assert_same_state(a, b, "monitor and evaluation"), assert_same_monitor(a, b, "monitor and evaluation")
    sa, sb = a.evaluation_state(), b.evaluation_state()
    for k in sa:
        assert np.array_equal(bits(sa[k]), bits(sb[k])), k
    assert a.ev.count == b.ev.count == 2 and a.mon.count == b.mon.count == 3
    a.close(), b.close()


def test_n_steps_1_is_the_learner_without_the_argument():
    a, b = Side("UR5DynReach-v1", M=96), Side("UR5DynReach-v1", M=96, n_steps=1)
    assert "n_steps" not in a.learner._saved_hp() and "n_steps" not in b.learner._saved_hp()
    la, lb = a.loop(4, 1, 2, first_draw=7), b.learner.train(b.replay, 4, 1, 2, seed=UPDATE_SEED, first_draw=7)
    torch.cuda.synchronize(a.env.device)
    assert b.learner._train["nstep"] is None  # urgym_sac_train itself: no scratch of the multi-step call exists
    assert_same_losses(la, lb, "n_steps = 1"), assert_same_state(a, b, "n_steps = 1"), assert_same_last_update(a, b, "n_steps = 1")
    a.close(), b.close()
    with pytest.raises(ValueError, match="device_entropy"):
        SACLearner(None, **dict(ALL, device_entropy=False, n_steps=3))


def test_save_and_load_continue_bit_for_bit(tmp_path):
    from test_checkpoint import Fresh, assert_same_side

    a, b = NSide(), NSide()
    a.learner.train(a.replay, 6, 1, 2, seed=UPDATE_SEED, first_draw=7)
    b.learner.train(b.replay, 3, 1, 2, seed=UPDATE_SEED, first_draw=7)
    path = tmp_path / "run.npz"
    b.learner.save(path, replay=b.replay, extra=dict(update_draw=7 + b.learner.adam_state["step"]))
    b.close()
    one = Fresh("UR5DynReach-v1", M=96)  # a one-step learner refuses the file, and nothing of it is written
    with pytest.raises(ValueError, match="n_steps is 3 in the checkpoint, 1 here"):
        one.learner.load(path, replay=one.replay)
    one.close()
    c = Fresh("UR5DynReach-v1", M=96, n_steps=3)
    extra = c.learner.load(path, replay=c.replay)
    c.learner.train(c.replay, 3, 1, 2, seed=UPDATE_SEED, first_draw=extra["update_draw"])
    torch.cuda.synchronize(a.env.device)
    assert_same_side(a, c, "3 + 3"), assert_same_last_update(a, c, "3 + 3")
    a.close(), c.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_launch_nothing_and_write_nothing(small_env):
    env, lib, count = small_env, small_env.lib, 8
    replay = DeviceReplay(env, CAPACITY)
    upload(replay, synthetic_ring(env.num_envs, env.obs_dim, env.goal_dim), 4, 0)
    g = guarded_batch(env, count)
    snapshot = lambda pairs: torch.cat([flat.view(torch.uint8).reshape(-1) for flat, _ in pairs.values()]).clone()  # noqa: E731
    before = snapshot(g)
    ptr = lambda name, ct: C.cast(g[name][1].data_ptr(), C.POINTER(ct))  # noqa: E731

    def batch():
        b = _abi.ReplayBatch()
        for name, ct, _, _ in _abi.REPLAY_RING_FIELDS:
            setattr(b, name, ptr(name, ct))
        b.index = ptr("index", C.c_int64)
        return b

    def nstep(**over):
        n = _abi.ReplayNstep(3, 0, GAMMA, 0.0, ptr("discount", C.c_float), ptr("steps", C.c_int32), ptr("last_index", C.c_int64))
        for k, v in over.items():
            setattr(n, k, v)
        return n

    def sample(ring=None, oldest=0, filled=4, count_=count, b=True, n=True):
        ring = replay._ring if ring is None else ring
        return lib.urgym_replay_sample_nstep(env._h, C.byref(ring), oldest, filled, 1, 2, count_, C.byref(batch()) if b is True else b,
                                             C.byref(nstep()) if n is True else n, env._stream())

    no_truncated = _abi.ReplayRing.from_buffer_copy(replay._ring)
    no_truncated.truncated = None
    bad_ring = _abi.ReplayRing.from_buffer_copy(replay._ring)
    bad_ring.reserved0 = 1
    null = C.POINTER(C.c_float)()
    refused = {
        "nstep NULL": lambda: sample(n=None), "n_steps 0": lambda: sample(n=C.byref(nstep(n_steps=0))), "n_steps 33": lambda: sample(n=C.byref(nstep(n_steps=33))),
        "reserved0": lambda: sample(n=C.byref(nstep(reserved0=1))), "reserved1": lambda: sample(n=C.byref(nstep(reserved1=1.0))),
        "gamma inf": lambda: sample(n=C.byref(nstep(gamma=float("inf")))), "gamma nan": lambda: sample(n=C.byref(nstep(gamma=float("nan")))),
        "discount NULL": lambda: sample(n=C.byref(nstep(discount=null))), "no truncated at n_steps 3": lambda: sample(ring=no_truncated),
        # urgym_replay_sample's own
        "filled 0": lambda: sample(filled=0), "filled above C": lambda: sample(filled=CAPACITY + 1), "oldest C": lambda: sample(oldest=CAPACITY),
        "count 0": lambda: sample(count_=0), "batch NULL": lambda: sample(b=None), "no output": lambda: sample(b=C.byref(_abi.ReplayBatch())),
        "ring reserved0": lambda: sample(ring=bad_ring),
    }
    for name, call in refused.items():
        assert call() == _abi.ERR_ARG, name
        assert b"urgym_replay_sample_nstep" in lib.urgym_last_error(env._h), name
    torch.cuda.synchronize(env.device)
    # the Python layer refuses the same before the library is asked
    for kw in (dict(n_steps=0, gamma=GAMMA), dict(n_steps=33, gamma=GAMMA), dict(n_steps=2.5, gamma=GAMMA), dict(n_steps=3, gamma=float("inf")), dict(n_steps=3),
               dict(gamma=GAMMA)):
        with pytest.raises(ValueError):
            replay.sample_into(views(g), 1, 2, **kw)
    with pytest.raises(ValueError, match="discount"):
        replay.sample_into(views(g, nstep=False), 1, 2, n_steps=3, gamma=GAMMA)

    # ---- the entropy step: urgym_sac_entropy_step's refusals on the new group
    e = {k: guarded((count,), torch.float32, env.device, 1.0) for k in ("log_prob", "reward", "q_min_next", "discount", "next_log_prob", "y", "d_log_prob")}
    e.update({k: guarded((1,), torch.float32, env.device, 0.5) for k in ("l", "m", "v", "ent_coef", "loss")})
    e["terminated"] = guarded((count,), torch.uint8, env.device, 0)
    e_before = snapshot(e)
    fp = lambda name: C.cast(e[name][1].data_ptr(), C.POINTER(C.c_float))  # noqa: E731

    def args(**over):
        a = _abi.SacEntropyNstepArgs(count, 0, TARGET_ENTROPY, 1.0 / count, fp("log_prob"), fp("l"), fp("m"), fp("v"), fp("ent_coef"), fp("loss"), fp("reward"),
                                     fp("q_min_next"), fp("discount"), fp("next_log_prob"), C.cast(e["terminated"][1].data_ptr(), C.POINTER(C.c_uint8)), fp("y"),
                                     fp("d_log_prob"))
        for k, v in over.items():
            setattr(a, k, v)
        return a

    hp = _abi.AdamHyper(1e-4, 0.9, 0.999, 1e-8, 3, 0)
    step = lambda a, h=hp: lib.urgym_sac_entropy_step_nstep(env._h, C.byref(a) if a is not None else None, C.byref(h) if h is not None else None, env._stream())  # noqa: E731
    bad = {"args NULL": (None, hp), "hp NULL": (args(), None), "count 0": (args(count=0), hp), "count above the cap": (args(count=65537), hp),
           "reserved0": (args(reserved0=1), hp), "target_entropy nan": (args(target_entropy=float("nan")), hp), "scale inf": (args(scale=float("inf")), hp),
           "step 0": (args(), _abi.AdamHyper(1e-4, 0.9, 0.999, 1e-8, 0, 0))}
    bad.update({f"{k} NULL": (args(**{k: null}), hp) for k in ("log_prob", "log_ent_coef", "exp_avg", "exp_avg_sq", "ent_coef_out")})
    bad.update({f"the group without {k}": (args(**{k: null}), hp) for k in ("reward", "q_min_next", "discount", "next_log_prob", "y_out")})
    bad["terminated alone"] = (args(reward=null, q_min_next=null, discount=null, next_log_prob=null, y_out=null), hp)
    for name, (a, h) in bad.items():
        assert step(a, h) == _abi.ERR_ARG, name
    torch.cuda.synchronize(env.device)
    assert torch.equal(snapshot(g), before) and torch.equal(snapshot(e), e_before)
    # one step needs no truncated: the same ring is accepted at n_steps = 1
    only_reward = _abi.ReplayBatch()
    only_reward.reward = ptr("reward", C.c_float)
    assert lib.urgym_replay_sample_nstep(env._h, C.byref(no_truncated), 0, 4, 1, 2, count, C.byref(only_reward), C.byref(nstep(n_steps=1)), env._stream()) == 0
    torch.cuda.synchronize(env.device)
    assert same_bits(g["discount"][1].cpu().numpy(), np.full(count, np.float32(GAMMA))) and (g["steps"][1] == 1).all() and guards_intact(g) is None
    with pytest.raises(ValueError, match="half given"):
        env.entropy_step_nstep((e["l"][1], e["m"][1], e["v"][1]), e["log_prob"][1], TARGET_ENTROPY, ent_coef_out=e["ent_coef"][1], reward=e["reward"][1], **ADAM)


def test_training_call_refusals():
    s = NSide()
    s.learner.collect(s.replay, 2)
    env, lib, lr = s.env, s.env.lib, s.learner
    tr = lr._train_binding(s.replay)
    L, M = tr["binding"].struct, 96
    losses = torch.full((3, 2), float("nan"), device=env.device)
    for name, row in zip(_abi.SAC_LEARNER_LOSSES, losses):
        setattr(L, name, C.cast(row.data_ptr(), C.POINTER(C.c_float)))
    S = _abi.SacSchedule(2, 2, CAP, 1, 0, 2, 0, 0, 0, 5, 1)  # two updates on the ring as it stands
    scratch = {k: torch.full((M,), 7.0, device=env.device) for k in ("discount", "q_min_next")}
    fp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float))  # noqa: E731
    state_before = {k: (v.clone() if isinstance(v, torch.Tensor) else np.array(v)) for k, v in s.state().items()}
    null = C.POINTER(C.c_float)()
    cases = {"nstep NULL": None, "n_steps 1": _abi.SacNstep(1, 0, fp(scratch["discount"]), fp(scratch["q_min_next"])),
             "n_steps 33": _abi.SacNstep(33, 0, fp(scratch["discount"]), fp(scratch["q_min_next"])),
             "reserved0": _abi.SacNstep(3, 1, fp(scratch["discount"]), fp(scratch["q_min_next"])),
             "discount NULL": _abi.SacNstep(3, 0, null, fp(scratch["q_min_next"])), "q_min_next NULL": _abi.SacNstep(3, 0, fp(scratch["discount"]), null)}
    for name, n in cases.items():
        assert lib.urgym_sac_train_nstep(env._h, C.byref(L), C.byref(S), C.byref(n) if n is not None else None, None, None, env._stream()) == _abi.ERR_ARG, name
        assert b"urgym_sac_train_nstep" in lib.urgym_last_error(env._h), name
    collects_only = _abi.SacSchedule(2, 2, CAP, 1, 1, 0, 0, 0, 0, 5, 1)  # one step, no update: the window is checked all the same
    assert lib.urgym_sac_train_nstep(env._h, C.byref(L), C.byref(collects_only), C.byref(cases["n_steps 1"]), None, None, env._stream()) == _abi.ERR_ARG
    torch.cuda.synchronize(env.device)
    assert torch.isnan(losses).all() and all((t == 7.0).all() for t in scratch.values())
    after = s.state()
    assert all(np.array_equal(bits(state_before[k]), bits(after[k])) for k in after)
    for name in _abi.SAC_LEARNER_LOSSES:
        setattr(L, name, None)
    with pytest.raises(ValueError, match="n_steps"):
        env.sac_train(tr["binding"], losses[0], losses[1], losses[2], first_slot=2, filled_steps=2, num_iterations=1, steps_per_iteration=0,
                      updates_per_iteration=2, nstep=dict(n_steps=1, **scratch))
    with pytest.raises(NativeError):  # what the call without the window refuses is refused here too: an update on an empty ring
        env.sac_train(tr["binding"], losses[0], losses[1], losses[2], first_slot=0, filled_steps=0, num_iterations=1, steps_per_iteration=0,
                      updates_per_iteration=2, nstep=dict(n_steps=3, **scratch))
    s.close()
