"""GPU tests (-m gpu) of the checkpoint: the unpack kernels (urgym_actor_unpack / urgym_critic_unpack through
``DeviceActor.parameters`` / ``DeviceCritic.parameters``), the environment's ``checkpoint_state`` / ``restore_checkpoint``, and
``SACLearner.save`` / ``load`` / ``load_parameters``.

Nothing here has a tolerance: the unpack kernels copy, and a run that is saved, torn down, rebuilt in fresh objects made from OTHER seeds
and loaded must continue with the same words as the run that was never interrupted.  The shapes are test_sac_train's: N = 64 envs,
H = 32 (padded to 128, so the padding paths run), M = 64 rows, a ring of 4 slots, learning_starts = 128.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_evaluation import EVAL_SEED, EVAL_STEPS
from test_sac_train import ALL, CAP, H, N, SEED, STARTS, UPDATE_SEED, Side, assert_same_last_update, assert_same_state, bits, guarded, guards_intact
from ur_gym_amd import _abi, checkpoint, make_vec
from ur_gym_amd.evaluation import (ACTOR_ARRAYS, CRITIC_ARRAYS, LOG_STD_ARRAYS, DeviceActor, DeviceCritic, DeviceEvaluation, DeviceMonitor, DeviceReplay,
                                   evaluation_points, polyak)
from ur_gym_amd.training import SACLearner

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WIDTHS = (32, 160, 256, 288, 512)
CANARY = 0x7FC0C0DE  # a NaN no source holds
OTHER = 1000         # what the fresh objects' seeds differ by


def weird(a):
    """`a` with the bit patterns a copy must keep planted in it: -0.0f, a NaN with a payload, a denormal."""
    w = np.ascontiguousarray(a, dtype=np.float32).copy()
    flat = w.reshape(-1).view(np.uint32)
    flat[0::13], flat[1::17], flat[2::19] = 0x80000000, 0x7FC00ABC, 0x00000003
    return w


def actor_arrays(rng, n, Hh, head=True):
    shapes = dict(zip(ACTOR_ARRAYS + LOG_STD_ARRAYS, ((Hh, n), (Hh,), (Hh, Hh), (Hh,), (6, Hh), (6,), (6, Hh), (6,))))
    return {k: weird(rng.standard_normal(shapes[k])) for k in ACTOR_ARRAYS + (LOG_STD_ARRAYS if head else ())}


def critic_arrays(rng, n, Hh, plain=False):
    shapes = dict(zip(CRITIC_ARRAYS, ((Hh, n), (Hh,), (Hh, Hh), (Hh,), (1, Hh), (1,))))
    make = (lambda a: a.astype(np.float32)) if plain else weird
    return [{k: make(rng.standard_normal(s)) for k, s in shapes.items()} for _ in range(2)]


def guarded_like(arrays, device):
    """name -> (flat, view): destinations one element into allocations between guard words, filled with the canary."""
    out = {}
    for k, a in arrays.items():
        flat, view = guarded(a.shape, torch.float32, device)
        view.view(torch.int32).fill_(CANARY)
        out[k] = (flat, view)
    return out


def assert_written(pairs, want, what):
    assert guards_intact(pairs) is None, (what, guards_intact(pairs))
    for k, (_, view) in pairs.items():
        got = view.cpu().numpy()
        assert not (got.view(np.uint32) == CANARY).any(), (what, k, "the canary survives inside the tensor")
        assert np.array_equal(bits(got), bits(want[k])), (what, k)


def on_device(arrays, device):
    if isinstance(arrays, dict):
        return {k: torch.from_numpy(v).to(device) for k, v in arrays.items()}
    return [on_device(w, device) for w in arrays]


# ------------------------------------------------------------------------------------------------ 1. unpack, every instance
@pytest.mark.parametrize("env_id", sorted(_abi.ENV_IDS))
def test_unpack_every_instance(env_id):
    env = make_vec(env_id, num_envs=4, seed=SEED, auto_reset=True)
    dev, n = env.device, env.obs_dim + 2 * env.goal_dim
    rng = np.random.default_rng(_abi.ENV_IDS[env_id])
    for Hh in WIDTHS:
        what = f"{env_id} H={Hh}"
        # the actor with the head: eight tensors, bitwise the arrays it was created from
        w = actor_arrays(rng, n, Hh)
        actor = DeviceActor(w, env)
        pairs = guarded_like(w, dev)
        got = actor.parameters(out={k: v for k, (_, v) in pairs.items()})
        torch.cuda.synchronize(dev)
        assert sorted(got) == sorted(ACTOR_ARRAYS + LOG_STD_ARRAYS)
        assert_written(pairs, w, what + " actor")
        fresh = actor.parameters()  # tensors of its own
        assert sorted(fresh) == sorted(w) and all(np.array_equal(bits(fresh[k]), bits(w[k])) for k in w), what
        # parameters() then load_parameters() leaves the packed buffer as it was; an unpack between two loads sees the first
        before = actor.packed()
        actor.load_parameters(fresh)
        assert np.array_equal(bits(actor.packed()), bits(before)), what
        w2 = actor_arrays(rng, n, Hh)
        actor.load_parameters(on_device(w, dev))
        between = actor.parameters()
        actor.load_parameters(on_device(w2, dev))
        after = actor.parameters()
        torch.cuda.synchronize(dev)
        assert all(np.array_equal(bits(between[k]), bits(w[k])) and np.array_equal(bits(after[k]), bits(w2[k])) for k in w), what
        actor.close()
        # the actor without the head: six tensors; the head's destinations are refused, and skipped when they are not given
        bare = DeviceActor({k: w[k] for k in ACTOR_ARRAYS}, env)
        six = bare.parameters()
        assert sorted(six) == sorted(ACTOR_ARRAYS) and all(np.array_equal(bits(six[k]), bits(w[k])) for k in six), what
        pairs = guarded_like(w, dev)
        with pytest.raises(ValueError, match="no log_std head"):
            bare.parameters(out={k: v for k, (_, v) in pairs.items()})
        p = _abi.ActorParamsOut(n, Hh, 0, *[C.cast(pairs[k][1].data_ptr(), C.POINTER(C.c_float)) for k in ACTOR_ARRAYS + LOG_STD_ARRAYS])
        assert env.lib.urgym_actor_unpack(env._h, bare._a, C.byref(p), env._stream()) == _abi.ERR_ARG
        assert b"no log_std head" in env.lib.urgym_last_error(env._h)
        torch.cuda.synchronize(dev)
        assert guards_intact(pairs) is None and all((v.view(torch.int32) == CANARY).all() for _, v in pairs.values()), what
        bare.close()
        # the critic: twelve tensors
        cw = critic_arrays(rng, n + 6, Hh)
        critic = DeviceCritic(cw, env)
        cpairs = [guarded_like(net, dev) for net in cw]
        critic.parameters(out=[{k: v for k, (_, v) in pr.items()} for pr in cpairs])
        torch.cuda.synchronize(dev)
        for i in range(2):
            assert_written(cpairs[i], cw[i], f"{what} qf{i}")
        # round trip with NaN in real weights (cw holds some): the packed buffer does not move
        before = critic.packed()
        assert np.isnan(before).any()
        critic.load_parameters(critic.parameters(), tau=1.0)
        assert np.array_equal(bits(critic.packed()), bits(before)), what
        # stream order: an unpack enqueued between two loads, without a synchronisation, sees the first
        c1, c2 = critic_arrays(rng, n + 6, Hh), critic_arrays(rng, n + 6, Hh)
        critic.load_parameters(on_device(c1, dev), tau=1.0)
        between = critic.parameters()
        critic.load_parameters(on_device(c2, dev), tau=1.0)
        torch.cuda.synchronize(dev)
        assert all(np.array_equal(bits(between[i][k]), bits(c1[i][k])) for i in range(2) for k in CRITIC_ARRAYS), what
        critic.close()
        # three Polyak blends: the target a learner keeps equals the recursion applied per tensor in torch's layout
        start, srcs = critic_arrays(rng, n + 6, Hh, plain=True), [critic_arrays(rng, n + 6, Hh, plain=True) for _ in range(3)]
        target = DeviceCritic(start, env)
        want = [dict(net) for net in start]
        for src in srcs:
            target.load_parameters(on_device(src, dev), tau=0.005)
            want = [{k: polyak(want[i][k], src[i][k], 0.005) for k in CRITIC_ARRAYS} for i in range(2)]
        got = target.parameters()
        torch.cuda.synchronize(dev)
        assert all(np.array_equal(bits(got[i][k]), bits(want[i][k])) for i in range(2) for k in CRITIC_ARRAYS), what
        assert any(not np.array_equal(bits(want[0][k]), bits(start[0][k])) for k in CRITIC_ARRAYS)  # the blends moved it
        target.close()
    env.close()


def test_unpack_refusals():
    env = make_vec("UR5DynReach-v1", num_envs=4, seed=SEED, auto_reset=True)
    other = make_vec("UR5DynReach-v1", num_envs=4, seed=SEED, auto_reset=True)
    dev, n, lib = env.device, env.obs_dim + 2 * env.goal_dim, env.lib
    rng = np.random.default_rng(9)
    w, cw = actor_arrays(rng, n, H), critic_arrays(rng, n + 6, H)
    actor, critic = DeviceActor(w, env), DeviceCritic(cw, env)
    stranger_a, stranger_c = DeviceActor(w, other), DeviceCritic(cw, other)
    pairs, cpairs = guarded_like(w, dev), [guarded_like(net, dev) for net in cw]
    fp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float))  # noqa: E731

    def actor_out(**over):
        p = _abi.ActorParamsOut(n, H, 0, *[fp(pairs[k][1]) for k in ACTOR_ARRAYS + LOG_STD_ARRAYS])
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def critic_out(**over):
        p = _abi.CriticParamsOut(n + 6, H, 0)
        for i in range(2):
            p.qf[i] = _abi.QNetworkOut(*[fp(cpairs[i][k][1]) for k in CRITIC_ARRAYS])
        for k, v in over.items():
            setattr(p, k, v)
        return p

    null = C.POINTER(C.c_float)()
    call_a = lambda h, a, p: lib.urgym_actor_unpack(h, a, C.byref(p) if p is not None else None, env._stream())   # noqa: E731
    call_c = lambda h, c, p: lib.urgym_critic_unpack(h, c, C.byref(p) if p is not None else None, env._stream())  # noqa: E731
    def without(i, field):
        p = critic_out()
        setattr(p.qf[i], field, null)
        return p

    refusals = [  # (the call, the handle that keeps its message, the message)
        (lambda: call_a(None, actor._a, actor_out()), None, b"null handle"),
        (lambda: call_a(env._h, None, actor_out()), env._h, b"urgym_actor_unpack: not an actor of this handle"),
        (lambda: call_a(env._h, actor._a, None), env._h, b"null out"),
        (lambda: call_a(env._h, stranger_a._a, actor_out()), env._h, b"not an actor of this handle"),
        (lambda: call_a(env._h, critic._c, actor_out()), env._h, b"not an actor of this handle"),
        (lambda: call_a(env._h, actor._a, actor_out(w0=null)), env._h, b"urgym_actor_unpack: out->w0 is null"),
        (lambda: call_a(env._h, actor._a, actor_out(w1=null)), env._h, b"out->w1 is null"),
        (lambda: call_a(env._h, actor._a, actor_out(b_mu=null)), env._h, b"out->b_mu is null"),
        (lambda: call_a(env._h, actor._a, actor_out(w_log_std=null)), env._h, b"needs both w_log_std and b_log_std"),
        (lambda: call_a(env._h, actor._a, actor_out(b_log_std=null)), env._h, b"needs both w_log_std and b_log_std"),
        (lambda: call_a(env._h, actor._a, actor_out(in_features=n + 1)), env._h, b"out is 48 -> 32, the actor is 47 -> 32"),
        (lambda: call_a(env._h, actor._a, actor_out(hidden_width=2 * H)), env._h, b"out is 47 -> 64, the actor is 47 -> 32"),
        (lambda: call_a(env._h, actor._a, actor_out(reserved0=1)), env._h, b"reserved0 must be 0"),
        (lambda: call_c(None, critic._c, critic_out()), None, b"null handle"),
        (lambda: call_c(env._h, None, critic_out()), env._h, b"urgym_critic_unpack: not a critic of this handle"),
        (lambda: call_c(env._h, critic._c, None), env._h, b"null out"),
        (lambda: call_c(env._h, stranger_c._c, critic_out()), env._h, b"not a critic of this handle"),
        (lambda: call_c(env._h, actor._a, critic_out()), env._h, b"not a critic of this handle"),
        (lambda: call_c(env._h, critic._c, critic_out(in_features=n)), env._h, b"out is 47 -> 32, the critic is 53 -> 32"),
        (lambda: call_c(env._h, critic._c, critic_out(hidden_width=2 * H)), env._h, b"out is 53 -> 64, the critic is 53 -> 32"),
        (lambda: call_c(env._h, critic._c, critic_out(reserved0=-1)), env._h, b"reserved0 must be 0"),
        (lambda: call_c(env._h, critic._c, without(0, "w0")), env._h, b"urgym_critic_unpack: out->qf[0].w0 is null"),
        (lambda: call_c(env._h, critic._c, without(1, "w_q")), env._h, b"out->qf[1].w_q is null"),
        (lambda: call_c(env._h, critic._c, without(1, "b_q")), env._h, b"out->qf[1].b_q is null"),
    ]
    for call, handle, message in refusals:
        assert call() == _abi.ERR_ARG, message
        assert message in lib.urgym_last_error(handle), (message, lib.urgym_last_error(handle))
    # nothing was launched: every destination still holds the canary, every guard its word
    torch.cuda.synchronize(dev)
    for pr in [pairs] + cpairs:
        assert guards_intact(pr) is None and all((v.view(torch.int32) == CANARY).all() for _, v in pr.values())
    # and the objects are usable afterwards
    assert call_a(env._h, actor._a, actor_out()) == _abi.OK and call_c(env._h, critic._c, critic_out()) == _abi.OK
    torch.cuda.synchronize(dev)
    assert_written(pairs, w, "after the refusals")
    for i in range(2):
        assert_written(cpairs[i], cw[i], "after the refusals")
    # the Python layer checks `out` like the sources of load_parameters
    with pytest.raises(ValueError, match="shape"):
        actor.parameters(out=dict(actor.parameters(), mu_bias=torch.zeros(5, device=dev)))
    with pytest.raises(ValueError, match="is on cpu"):
        critic.parameters(out=[{k: torch.zeros(v.shape) for k, v in net.items()} for net in cw])
    for x in (actor, critic, stranger_a, stranger_c):
        x.close()
    env.close(), other.close()


# ------------------------------------------------------------------------------------------------ 2. the environment's round trip
@pytest.mark.parametrize("env_id", ["UR5DynReach-v1", "UR5ObsReach-v1"])
def test_environment_round_trip(env_id, tmp_path):
    make = lambda seed: make_vec(env_id, num_envs=N, seed=seed, auto_reset=True, max_episode_steps=12)  # noqa: E731
    a, b = make(SEED), make(SEED)
    a.reset(seed=SEED), b.reset(seed=SEED)
    gen = torch.Generator(device="cpu").manual_seed(3)
    actions = (torch.rand((15 + 29, N, 6), generator=gen) * 2 - 1).to(a.device)
    for k in range(15):
        a.step(actions[k]), b.step(actions[k])
    checkpoint.write(tmp_path / "env.npz", dict(env=a.checkpoint_state()))
    assert sorted(a.checkpoint_state()["buffers"]) == sorted(name for name, _, _ in _abi.BUFFER_FIELDS)
    a.close()
    c = make(SEED + OTHER)
    c.reset(seed=SEED + OTHER)
    for k in range(3):
        c.step(actions[k])
    assert any(not np.array_equal(bits(b.buf[k]), bits(c.buf[k])) for k in b.buf)  # a restore that does nothing is noticed
    c.restore_checkpoint(checkpoint.read(tmp_path / "env.npz")["env"])
    assert (c._seed, c._needs_reset) == (SEED, False)
    torch.cuda.synchronize(b.device)
    for name in b.buf:
        assert np.array_equal(bits(b.buf[name]), bits(c.buf[name])), ("after the restore", name)
    resets = np.zeros(N, np.int64)
    for k in range(15, 15 + 2 * 12 + 5):
        b.step(actions[k]), c.step(actions[k])
        torch.cuda.synchronize(b.device)
        for name in b.buf:
            assert np.array_equal(bits(b.buf[name]), bits(c.buf[name])), (k, name)
        resets += (b.buf["terminated"] | b.buf["truncated"]).cpu().numpy().astype(np.int64)
    assert resets.min() >= 2  # every env passed through at least two auto-resets on the way
    for e in (b, c):
        assert not (e.buf["status"].cpu().numpy() & _abi.STATUS_STALE_RECORD).any()
    # another id, env count or configuration is refused before anything is written
    state = checkpoint.read(tmp_path / "env.npz")["env"]
    kept = {k: v.clone() for k, v in c.buf.items()}
    d = make_vec(env_id, num_envs=N, seed=SEED, auto_reset=True, max_episode_steps=13)
    with pytest.raises(ValueError, match="config.max_episode_steps is 12"):
        d.restore_checkpoint(state)
    with pytest.raises(ValueError, match="num_envs|x 32"):
        c.restore_checkpoint(dict(state, num_envs=32))
    with pytest.raises(ValueError, match="UR5OriReach-v1"):
        c.restore_checkpoint(dict(state, env_id="UR5OriReach-v1"))
    with pytest.raises(ValueError, match="buffers\\['q'\\]"):
        c.restore_checkpoint(dict(state, buffers=dict(state["buffers"], q=state["buffers"]["q"][:, :8])))
    assert all(np.array_equal(bits(kept[k]), bits(c.buf[k])) for k in kept)
    b.close(), c.close(), d.close()


# ------------------------------------------------------------------------------------------------ 3. resume equals the uninterrupted run
class Run:
    """A training environment (episodes of at most 3 steps, so that they finish), a learner with all five device options, a ring, a
    monitor, and an evaluation on a second environment: the whole of what ``save`` holds.  `shift` moves every seed a fresh object
    may be made from; the evaluation's seed is part of what it is and stays."""

    def __init__(self, shift=0, env_id="UR5OriReach-v1"):
        self.env = make_vec(env_id, num_envs=N, seed=SEED + shift, auto_reset=True, max_episode_steps=3)
        self.env.reset(seed=SEED + shift)
        self.learner = SACLearner(self.env, seed=SEED + shift, hidden_width=H, batch_size=64, learning_starts=STARTS, **ALL)
        self.replay = DeviceReplay(self.env, CAP)
        self.mon = DeviceMonitor(self.env, capacity=4)
        self.test_env = make_vec(env_id, num_envs=N, seed=EVAL_SEED + shift, auto_reset=False)
        self.ev = DeviceEvaluation(self.test_env, self.learner.actor.tensors(), num_steps=EVAL_STEPS, seed=EVAL_SEED, capacity=8)
        if shift:  # garbage where a load must write: a load that does nothing fails
            for t in self.replay.ring.values():
                t.fill_(1)
            self.replay.cursor, self.replay.filled = 1, 3
            self.mon.records.fill_(-1), self.ev.records.fill_(-1)
            for t in self.mon.state.values():
                t.fill_(7)

    def parts(self):
        return dict(replay=self.replay, monitor=self.mon, evaluation=self.ev)

    def train(self, iterations, first_draw):
        return self.learner.train(self.replay, iterations, 1, 2, seed=UPDATE_SEED, first_draw=first_draw, evaluation=self.ev, eval_every=2,
                                  monitor=self.mon, log_every=2)

    def python_loop(self, iterations, first_draw):
        """tools/train_sac.py's loop with the monitor and the evaluation: what ``train`` is bit for bit."""
        lr, losses, draw = self.learner, [], first_draw
        for _ in range(iterations):
            before = lr.adam_state["step"]
            lr.collect(self.replay, 1, monitor=self.mon)
            if lr.env_steps * N >= lr.hp["learning_starts"]:
                for _ in range(2):
                    losses.append({k: v.clone() for k, v in lr.update(self.replay, UPDATE_SEED, draw).items()})
                    draw += 1
            self.mon.iterations += 1
            if self.mon.iterations % 2 == 0:
                self.mon.record(self.mon.iterations)
            if lr.adam_state["step"] // 2 > before // 2:
                self.ev.evaluate(lr.actor.tensors())
        return {k: torch.stack([l[k] for l in losses]) for k in ("critic_loss", "actor_loss", "ent_coef_loss")}

    def state(self):
        """name -> tensor or array of everything the checkpoint promises."""
        lr, out = self.learner, {}
        valid = [(self.replay.oldest_slot + i) % CAP for i in range(self.replay.filled)]
        out.update({f"ring.{k}": v[valid] for k, v in self.replay.ring.items()})
        out.update({f"buf.{k}": v for k, v in self.env.buf.items()})
        out.update({f"eval.buf.{k}": v for k, v in self.test_env.buf.items()})
        st, es = lr.adam_state, lr.entropy_state
        for kind, w in (("param", lr.actor.tensors()), ("moment:m", st["actor"][0]), ("moment:v", st["actor"][1])):
            out.update({f"{kind}:actor.{k}": v for k, v in w.items()})
        for kind, nets in (("param", lr.critic.tensors()), ("moment:m", st["critic"][0]), ("moment:v", st["critic"][1]), ("target", lr.target.parameters())):
            for i, w in enumerate(nets):
                out.update({f"{kind}:qf{i}.{k}": v for k, v in w.items()})
        out.update(log_ent_coef=lr.log_ent_coef, ent_m=es["exp_avg"], ent_v=es["exp_avg_sq"])
        out.update({"packed.actor": lr.device_actor.packed(), "packed.online": lr.online.packed(), "packed.target": lr.target.packed()})
        out.update({f"best.{k}": v for k, v in self.ev.best.items()})
        out.update({"eval.records": self.ev.records[:self.ev.count], "best_mean": self.ev.best_mean, "best_index": self.ev.best_index})
        out.update({f"monitor.{k}": v for k, v in self.mon.state.items()})
        out["monitor.records"] = self.mon.records[:self.mon.count]
        return out

    def counters(self):
        lr = self.learner
        return dict(env_steps=lr.env_steps, draw=lr.draw, seed=lr.seed, step=lr.adam_state["step"], cursor=self.replay.cursor, filled=self.replay.filled,
                    mon_count=self.mon.count, mon_iterations=self.mon.iterations, ev_count=self.ev.count, env_seed=self.env._seed,
                    eval_env_seed=self.test_env._seed, needs_reset=(self.env._needs_reset, self.test_env._needs_reset))

    def close(self):
        self.learner.close(), self.ev.close(), self.test_env.close(), self.env.close()


def assert_same_run(a, b, what):
    sa, sb = a.state(), b.state()
    assert sa.keys() == sb.keys()
    count = lambda prefix: sum(k.startswith(prefix) for k in sa)  # noqa: E731
    assert (count("param:"), count("target:"), count("moment:"), count("buf."), count("eval.buf."), count("ring.")) == (8 + 12, 12, 40, 24, 24, 11)
    for k in sa:
        assert sa[k].shape == sb[k].shape and np.array_equal(bits(sa[k]), bits(sb[k])), (what, k)
    assert a.counters() == b.counters(), (what, a.counters(), b.counters())


@pytest.fixture(scope="module")
def uninterrupted():
    """Run A: one object lifetime, 6 x (1 step, 2 updates) in one call.  Shared, read only."""
    a = Run()
    losses = a.train(6, first_draw=7)
    torch.cuda.synchronize(a.env.device)
    assert a.learner.adam_state["step"] == 10 and a.ev.count == 5 and a.mon.count == 3
    yield a, {k: v.clone() for k, v in losses.items()}
    a.close()


def interrupted(tmp_path):
    """Run B up to the load: 3 iterations, save, everything closed; fresh objects from other seeds with garbage in them; load."""
    b = Run()
    first = b.train(3, first_draw=7)
    path = tmp_path / "run.npz"
    b.learner.save(path, **b.parts(), extra=dict(update_draw=7 + b.learner.adam_state["step"]))
    b.close()
    del b
    c = Run(shift=OTHER)
    extra = c.learner.load(path, **c.parts())
    assert extra == dict(update_draw=11) and first["critic_loss"].shape == (4,)
    return c, extra


@pytest.mark.parametrize("route", ["train", "python-loop"])
def test_resume_equals_the_uninterrupted_run(uninterrupted, tmp_path, route):
    a, losses = uninterrupted
    assert evaluation_points(1, 6, 2, 1, 2) == [1, 2, 3, 4, 5]
    c, extra = interrupted(tmp_path)
    second = c.train(3, first_draw=extra["update_draw"]) if route == "train" else c.python_loop(3, first_draw=extra["update_draw"])
    torch.cuda.synchronize(c.env.device)
    for k in losses:  # the loss slots of the last three iterations
        assert second[k].shape == (6,) and np.array_equal(bits(second[k]), bits(losses[k][4:])), (route, k)
    assert_same_run(a, c, route)
    assert_same_last_update(a, c, route)
    assert [r["eval_index"] for r in c.ev.results()] == [0, 1, 2, 3, 4] and [r["iteration"] for r in c.mon.results()] == [2, 4, 6]
    assert c.ev.best_state() == a.ev.best_state()
    c.close()


# ------------------------------------------------------------------------------------------------ 4. smaller cases
class Fresh(Side):
    """test_sac_train's Side made from other seeds, with garbage in its ring."""

    def __init__(self, env_id="UR5OriReach-v1", M=64, hidden=H, **over):
        self.env = make_vec(env_id, num_envs=N, seed=SEED + OTHER, auto_reset=True)
        self.env.reset(seed=SEED + OTHER)
        self.learner = SACLearner(self.env, seed=SEED + OTHER, hidden_width=hidden, batch_size=M, learning_starts=STARTS, **dict(ALL, **over))
        self.replay = DeviceReplay(self.env, CAP)
        for t in self.replay.ring.values():
            t.fill_(1)


def ring_view(side):
    r = side.replay
    return [(r.oldest_slot + i) % CAP for i in range(r.filled)]


def assert_same_side(a, b, what):
    """assert_same_state, but the gradients (scratch a save does not hold: every update rewrites them before it reads them) and the ring
    slots that hold nothing yet."""
    sa, sb = a.state(), b.state()
    assert ring_view(a) == ring_view(b)
    for k in sa:
        if k.startswith("grad:"):
            continue
        x, y = (sa[k][ring_view(a)], sb[k][ring_view(a)]) if k.startswith("ring.") else (sa[k], sb[k])
        assert np.array_equal(bits(x), bits(y)), (what, k)
    assert a.counters() == b.counters() and a.learner.seed == b.learner.seed, (what, a.counters(), b.counters())


@pytest.mark.parametrize("before,after,warm", [(1, 5, False), (6, 2, False), (3, 3, True)], ids=["mid-warm-up", "wrapped-ring", "live-binding"])
def test_saved_at_other_points(tmp_path, before, after, warm):
    """mid-warm-up: env_steps * N < learning_starts at the save, so the resumed call's warm-up counts must come out as the uninterrupted
    one's.  wrapped-ring: filled == capacity and cursor != 0.  live-binding: the loading learner has trained before (its ``train``
    binding exists and points at its tensors), then loads, then trains."""
    a, b = Side(), Side()
    a.learner.train(a.replay, before + after, 1, 2, seed=UPDATE_SEED, first_draw=7)
    b.learner.train(b.replay, before, 1, 2, seed=UPDATE_SEED, first_draw=7)
    if before == 1:
        assert b.learner.env_steps * N < STARTS and b.learner.adam_state["step"] == 0
    if before == 6:
        assert b.replay.filled == CAP and b.replay.cursor == 2
    path = tmp_path / "run.npz"
    b.learner.save(path, replay=b.replay, extra=dict(update_draw=7 + b.learner.adam_state["step"]))
    b.close()
    c = Fresh()
    if warm:
        c.learner.train(c.replay, 2, 1, 2, seed=UPDATE_SEED + 1, first_draw=0)
        binding = c.learner._train
    extra = c.learner.load(path, replay=c.replay)
    if warm:
        assert c.learner._train is binding  # not rebuilt: the tensors were written in place
    c.learner.train(c.replay, after, 1, 2, seed=UPDATE_SEED, first_draw=extra["update_draw"])
    torch.cuda.synchronize(a.env.device)
    assert_same_side(a, c, f"{before} + {after}")
    assert_same_last_update(a, c, f"{before} + {after}")
    a.close(), c.close()


def test_saved_without_the_ring_data(tmp_path):
    a = Side()
    a.learner.train(a.replay, 3, 1, 2, seed=UPDATE_SEED, first_draw=7)
    state = a.replay.state_dict(include_data=False)
    assert "ring" not in state
    c = Fresh()
    c.replay.load_state_dict(state)
    assert (c.replay.cursor, c.replay.filled, len(c.replay)) == (3, 0, 0)
    c.learner.load_state_dict(a.learner.state_dict())
    with pytest.raises(ValueError, match="filled_steps"):  # as today: nothing to draw from
        c.learner.update(c.replay, UPDATE_SEED, 0)
    c.learner.collect(c.replay, 1)
    c.learner.update(c.replay, UPDATE_SEED, 0)
    torch.cuda.synchronize(c.env.device)
    assert c.replay.filled == 1 and np.isfinite(c.learner.log_ent_coef.detach().cpu().numpy()).all()
    a.close(), c.close()


def test_torch_route_restores_every_tensor(tmp_path):
    """No device_* option: parameters, the three torch.optim states and the torch.Generator state come back bitwise.  Compared after the
    load; continuation on this route runs torch's kernels and is not asserted bitwise."""
    none = {k: False for k in ALL}
    a = Side(**none)
    for draw in range(3):
        a.learner.collect(a.replay, 1)
        a.learner.update(a.replay, UPDATE_SEED, draw)
    path = tmp_path / "run.npz"
    a.learner.save(path, replay=a.replay)
    c = Fresh(**none)
    c.learner.collect(c.replay, 2)
    c.learner.update(c.replay, UPDATE_SEED, 0)  # its optimisers and its generator have moved
    assert c.learner.load(path, replay=c.replay) is None
    torch.cuda.synchronize(a.env.device)
    la, lc = a.learner, c.learner
    assert la.adam_state is None and lc.online is None
    for k, v in la.actor.tensors().items():
        assert np.array_equal(bits(v), bits(lc.actor.tensors()[k])), k
    for i in range(2):
        for k, v in la.critic.tensors()[i].items():
            assert np.array_equal(bits(v), bits(lc.critic.tensors()[i][k])), (i, k)
    assert np.array_equal(bits(la.log_ent_coef), bits(lc.log_ent_coef))
    for name in ("actor_opt", "critic_opt", "ent_opt"):
        sa, sc = getattr(la, name).state_dict(), getattr(lc, name).state_dict()
        assert sa["param_groups"] == sc["param_groups"] and sorted(sa["state"]) == sorted(sc["state"]) and len(sa["state"]) > 0, name
        for i, s in sa["state"].items():
            assert sorted(s) == sorted(sc["state"][i]) == ["exp_avg", "exp_avg_sq", "step"]
            for k, v in s.items():
                assert v.dtype == sc["state"][i][k].dtype and v.device == sc["state"][i][k].device and np.array_equal(bits(v), bits(sc["state"][i][k])), (name, i, k)
    assert torch.equal(la.noise.get_state(), lc.noise.get_state())
    assert np.array_equal(bits(la.target.packed()), bits(lc.target.packed())) and np.array_equal(bits(la.device_actor.packed()), bits(lc.device_actor.packed()))
    assert (la.env_steps, la.draw, la.seed) == (lc.env_steps, lc.draw, lc.seed)
    for k, v in a.env.buf.items():
        assert np.array_equal(bits(v), bits(c.env.buf[k])), k
    lc.collect(c.replay, 1)
    lc.update(c.replay, UPDATE_SEED, 3)  # and it goes on
    torch.cuda.synchronize(a.env.device)
    a.close(), c.close()


def test_load_parameters_from_the_golden_files():
    """The reference's SAC.load(...) then learn (train.py:31-36) from plain parameter files: UR5DynReach-v1, H = 256."""
    actor = dict(np.load(os.path.join(GOLDEN, "actors", "actor_dyn.npz")))
    actor.update(np.load(os.path.join(GOLDEN, "actors", "log_std_dyn.npz")))
    critics = [dict(np.load(os.path.join(GOLDEN, "critics", f"critic_dyn_qf{i}.npz"))) for i in range(2)]
    env = make_vec("UR5DynReach-v1", num_envs=N, seed=SEED, auto_reset=True)
    env.reset(seed=SEED)
    lr = SACLearner(env, seed=SEED, hidden_width=256, batch_size=64, learning_starts=0, **ALL)
    replay = DeviceReplay(env, CAP)
    lr.collect(replay, 2)
    lr.update(replay, UPDATE_SEED, 0)  # moments and a step count to zero
    lr.load_parameters(actor=actor, critics=critics, log_ent_coef=-1.5)
    reference = DeviceActor(actor, env)
    torch.cuda.synchronize(env.device)
    assert np.array_equal(bits(lr.device_actor.packed()), bits(reference.packed()))
    mine, theirs = env.policy_actions(lr.device_actor), env.policy_actions(reference)
    torch.cuda.synchronize(env.device)
    assert np.array_equal(bits(mine), bits(theirs))  # evaluates bitwise like DeviceActor.load of the same files
    assert np.array_equal(bits(lr.target.packed()), bits(lr.online.packed()))
    assert np.array_equal(bits(lr.online.packed()), bits(DeviceCritic(critics, env).packed()))
    st, es = lr.adam_state, lr.entropy_state
    assert st["step"] == 0 and float(lr.log_ent_coef.detach()) == -1.5
    moments = [t for w in st["actor"] for t in w.values()] + [t for pair in st["critic"] for w in pair for t in w.values()] + [es["exp_avg"], es["exp_avg_sq"]]
    assert len(moments) == 42 and not any(bool(t.any()) for t in moments)
    for k, v in lr.actor.tensors().items():
        assert np.array_equal(bits(v), bits(actor[k])), k
    lr.update(replay, UPDATE_SEED, 1)  # one update then runs
    torch.cuda.synchronize(env.device)
    assert st["step"] == 1 and any(bool(t.any()) for t in moments) and np.isfinite(lr.device_actor.packed()).all()
    # a target of its own, and shapes that are not the learner's
    lr.load_parameters(actor=actor, critics=critics, target=[{k: v + 1 for k, v in w.items()} for w in critics])
    assert not np.array_equal(bits(lr.target.packed()), bits(lr.online.packed()))
    kept = lr.device_actor.packed()
    with pytest.raises(ValueError, match="mu_bias"):
        lr.load_parameters(actor=dict(actor, mu_bias=np.zeros(5, np.float32)), critics=critics)
    with pytest.raises(ValueError, match="missing"):
        lr.load_parameters(actor={k: actor[k] for k in ACTOR_ARRAYS}, critics=critics)
    assert np.array_equal(bits(lr.device_actor.packed()), bits(kept))
    reference.close(), lr.close(), env.close()


def test_mismatches_are_refused_and_write_nothing(tmp_path):
    a = Side()
    a.learner.train(a.replay, 3, 1, 2, seed=UPDATE_SEED, first_draw=7)
    path = tmp_path / "run.npz"
    a.learner.save(path, replay=a.replay)
    good = a.learner.state_dict()

    def refused(side, match, **kw):
        before = {k: np.array(bits(v)) for k, v in side.state().items()}
        counters = side.counters()
        with pytest.raises(ValueError, match=match):
            side.learner.load(path, **kw)
        torch.cuda.synchronize(side.env.device)
        after = side.state()
        assert all(np.array_equal(before[k], bits(after[k])) for k in before) and side.counters() == counters, match

    c = Fresh(hidden=64)
    refused(c, "hidden_width is 32", replay=c.replay)
    c.close()
    c = Fresh(M=80)
    refused(c, "batch_size is 64", replay=c.replay)
    c.close()
    c = Fresh("UR5DynReach-v1")
    refused(c, "env_id is 'UR5OriReach-v1'", replay=c.replay)
    c.close()
    c = Fresh()
    refused(c, "replay is present in the checkpoint", replay=None)
    refused(c, "monitor is absent from the checkpoint", replay=c.replay, monitor=DeviceMonitor(c.env))
    refused(c, "env is present in the checkpoint", replay=c.replay, env_state=False)
    small = DeviceReplay(c.env, CAP + 1)
    refused(c, "capacity", replay=small)
    before = {k: np.array(bits(v)) for k, v in c.state().items()}
    for bad, match in ((dict(good, hp=dict(good["hp"], gamma=0.5)), "gamma is 0.5"), (dict(good, num_envs=32), "num_envs is 32"),
                       (dict(good, entropy_state=None), "entropy_state is absent"),
                       (dict(good, target=[good["target"][0], dict(good["target"][1], q_0_bias=np.zeros(H + 1, np.float32))]), "target.qf1.q_0_bias")):
        with pytest.raises(ValueError, match=match):
            c.learner.load_state_dict(bad)
    after = c.state()
    assert all(np.array_equal(before[k], bits(after[k])) for k in before)
    # learning_rate and learning_starts may be set anew, explicitly
    d = Fresh(learning_rate=3e-4)
    refused(d, "learning_rate is 0.0001", replay=d.replay)
    assert d.learner.load(path, replay=d.replay, override=("learning_rate",)) is None and d.learner.hp["learning_rate"] == 3e-4
    torch.cuda.synchronize(d.env.device)
    assert np.array_equal(bits(d.learner.target.packed()), bits(a.learner.target.packed())) and d.learner._train is None
    a.close(), c.close(), d.close()


def test_a_killed_save_leaves_the_previous_file_loadable(tmp_path):
    from test_checkpoint_host import DyingStream

    a = Side()
    a.learner.train(a.replay, 3, 1, 2, seed=UPDATE_SEED, first_draw=7)
    path = tmp_path / "run.npz"
    a.learner.save(path, replay=a.replay, extra=dict(update_draw=11))
    a.learner.train(a.replay, 1, 1, 2, seed=UPDATE_SEED, first_draw=11)
    later = dict(learner=a.learner.state_dict(), extra=None, replay=a.replay.state_dict(), monitor=None, evaluation=None, env=a.env.checkpoint_state())
    with pytest.raises(OSError, match="died"):
        checkpoint.write(path, later, opener=lambda name, mode: DyingStream(name, mode, 20000))
    assert os.path.exists(checkpoint.temporary_name(path))  # the unfinished file lies beside the whole one
    c = Fresh()
    assert c.learner.load(path, replay=c.replay) == dict(update_draw=11)
    assert c.learner.adam_state["step"] == 4 and c.replay.filled == 3
    a.close(), c.close()
