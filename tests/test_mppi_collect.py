"""GPU tests (-m gpu) of the planner-driven collection (include/urgym.h, "planner-collected experience"): the execute
launch against its numpy restatement (ur_gym_amd.evaluation.mppi_execute on mppi_explore_noise), urgym_mppi_collect against the
Python-stepped loop it promises to be (read the live rows, plan, execute, step, file the outcome), against urgym_mppi_control(_guided)
at explore_sigma = 0, as two calls against one, the slots it must not write, every refusal, and the learner's side: SACLearner.collect
with a planner, the monitor, the prioritized ring, sync_planner.

Shapes: E = 3 source envs, K = 5, H = 2, so planner handles of 15 envs; E = 171 (1026 lanes: four workgroups and a tail of 2) for the
execute launch alone.  Every array -- those of urgym_mppi, of the guide, of the ring -- lies between guard words.
"""
import ctypes as C

import numpy as np
import pytest

from mppi_collect_cases import DRAW, E, E_WIDE, SEED, SIGMAS, action_rows, noise_bound, poisoned
from test_mppi_guide import (GUARD, OUTPUTS, STATE, Guarded, actor_path, assert_same_planner, check, critic_paths, guard, guards_intact, make_vec, np_, refused,
                             same_bits)
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import DeviceMonitor, DeviceMPPI, DevicePrioritizedReplay, DeviceReplay, mppi_execute, mppi_explore_noise

pytestmark = pytest.mark.gpu

K, HC = 5, 2
CONFIGS = {"plain": dict(), "value_policy": dict(terminal_value=True, policy_samples=2, policy_sigma=0.2), "fail_cost": dict(fail_cost=1e4)}
ROWS = ("observation", "achieved_goal", "desired_goal")
SHORT = dict(auto_reset=True, max_episode_steps=3)  # every env finishes inside a call of 4 steps


def pair(env_id, mode, **env_options):
    """A source that has been reset and a DeviceMPPI on it (plain, or guided by the golden actor and critics), every array guarded."""
    src = make_vec(env_id, E, 21, **env_options)
    src.reset(seed=21)
    options = CONFIGS[mode]
    learner = dict(actor=actor_path(env_id), critic=critic_paths(env_id)) if options.get("terminal_value") else {}
    mppi = DeviceMPPI(src, samples=K, horizon=HC, sigma=0.3, lam=20.0, gamma=0.95, seed=8, keep_weights=True, **learner, **options)
    return src, mppi, guard(mppi)


def pattern_like(t):
    """(the guarded tensor, the view of `t`'s shape inside it), every byte 0xA5."""
    import torch

    raw = torch.full(((t.numel() + 2 * GUARD) * t.element_size(),), 0xA5, dtype=torch.uint8, device="cuda:0")
    full = raw.view(t.dtype)
    return full, full[GUARD:GUARD + t.numel()].view(t.shape)


def guarded_replay(env, capacity, cls=DeviceReplay):
    """A ring whose tensors lie between guard words and hold the byte 0xA5 throughout, so that a slot nobody wrote shows."""
    replay, full = cls(env, capacity), {}
    for name, ct, _, _ in _abi.REPLAY_RING_FIELDS:
        full[name], replay.ring[name] = pattern_like(replay.ring[name])
        setattr(replay._ring, name, C.cast(replay.ring[name].data_ptr(), C.POINTER(ct)))
    return replay, full


def pattern_slots(ring, slots):
    import torch

    return all((np_(t[slots].contiguous().view(-1).view(torch.uint8)) == 0xA5).all() for t in ring.values())


def stepped_loop(mppi, capacity, first_slot, first_draw, num_steps, explore_sigma, ring=None):
    """What urgym_mppi_collect promises to be, stepped from Python: per step read the live rows into the slot, plan, execute into the
    slot's action rows, step the source, file the outcome (the final_* rows for an env that finished under auto_reset) and zero the mean
    of the envs that finished.  Returns (the ring as a dict of tensors that were 0xA5 throughout, the per-step masks of finished envs)."""
    import torch

    src = mppi.env
    if ring is None:
        ring = {name: pattern_like(torch.zeros(shape(capacity, E, src.obs_dim, src.goal_dim), dtype=torch.uint8 if ct is C.c_uint8 else torch.float32))[1]
                for name, ct, shape, _ in _abi.REPLAY_RING_FIELDS}
    finished = []
    for t in range(num_steps):
        slot, b = (first_slot + t) % capacity, src.buf
        for key in ROWS:
            ring[key][slot] = b[key]
        mppi.plan(first_draw + t)
        executed, _ = mppi.execute(first_draw + t, explore_sigma)
        ring["action"][slot] = executed
        src.step(executed)
        done = (b["terminated"] | b["truncated"]).bool()
        for key in ROWS:
            final = b["final_observation" if key == "observation" else "final_" + key]
            ring["next_" + key][slot] = torch.where(done[:, None], final, b[key]) if src.cfg.auto_reset else b[key]
        for key in ("reward", "terminated", "truncated", "is_success"):
            ring[key][slot] = b[key]
        mppi.buf["mean"][:, done] = 0.0
        finished.append(np_(done))
    return ring, np.stack(finished)


def assert_same_ring(got, want, where):
    for name, _, _, _ in _abi.REPLAY_RING_FIELDS:
        assert same_bits(np_(got[name]), np_(want[name])), (where, name)


def assert_same_everything(a, b, where):
    """Every buffer of urgym_mppi and of the guide, the planner's state and outputs, and every bound buffer of the source."""
    assert_same_planner(a, b, where)
    for key in a.env.buf:
        assert same_bits(np_(a.env.buf[key]), np_(b.env.buf[key])), (where, "source", key)


def close(*things):
    for x in things:
        x.close()


# ------------------------------------------------------------------------------------------------ 1. the execute launch
def test_execute_launch_is_the_restatement():
    """urgym_mppi_execute at E = 3 and E = 171 with explore_sigma 0, 0.3 and 25, on rows with a -0.0 and, a second time, with NaNs: executed
    is bitwise mppi_execute on the eps the launch reports, that eps is within the planner's bound of the float64 restatement, sigma 0 is a
    byte copy that reports eps = 0, and nothing but executed and explore_eps is written.  The noise of parent 0 alone equals its row at E = 3."""
    import torch

    lib = _native.lib()
    bound, got = noise_bound(), {}
    for e in (E, E_WIDE, 1):
        env = make_vec("UR5OriReach-v1", e, 0)  # names the device and E; needs no reset
        clean = action_rows(max(e, E))[:e]
        f64 = mppi_explore_noise(SEED, DRAW, np.arange(e), dtype=np.float64)
        for rows, nan in ((clean, np.zeros(clean.shape, bool)),) + ((poisoned(clean),) if e > 1 else ()):
            for sigma in SIGMAS:
                g = Guarded(e, 2, 1, seed=SEED)
                g.put("action_out", rows)
                full = {}
                full["executed"], executed = pattern_like(g.a["action_out"])
                full["explore_eps"], eps_out = pattern_like(g.a["action_out"])
                x = _abi.MppiExplore(sigma, 0, C.cast(eps_out.data_ptr(), C.POINTER(C.c_float)))
                check(lib.urgym_mppi_execute(env._h, C.byref(g.M), C.byref(x), DRAW, C.c_void_p(executed.data_ptr()), env._stream()), env)
                torch.cuda.synchronize()
                out, eps = np_(executed), np_(eps_out)
                where = (e, sigma, bool(nan.any()))
                assert g.guards_intact() and guards_intact(full) and g.untouched([n for n in g.a if n != "action_out"]) and same_bits(np_(g.a["action_out"]), rows), where
                assert same_bits(out, mppi_execute(rows, eps, sigma)), where
                if sigma == 0.0:
                    assert same_bits(out, rows) and np.signbit(out[0, 0]) and not eps.any() and not np.signbit(eps).any(), where
                    continue
                dev = float(np.abs(eps.astype(np.float64) - f64).max())
                print(f"exploration noise E={e} sigma={sigma}: device vs float64 {dev:.3e}, bound {bound:.3e}")
                assert dev <= bound, (where, dev, bound)
                assert same_bits(out[~nan], mppi_execute(clean, eps, sigma)[~nan]) and not np.isnan(out[~nan]).any(), where  # a NaN reaches its own element only
                if sigma == 25.0 and e == E_WIDE:
                    assert (out == 1).mean() > 0.3 and (out == -1).mean() > 0.3, where
                if not nan.any():
                    got[e, sigma] = (out, eps)
                    # without explore_eps the launch writes executed alone, and the same bits
                    full["executed"], again = pattern_like(g.a["action_out"])
                    check(lib.urgym_mppi_execute(env._h, C.byref(g.M), C.byref(_abi.MppiExplore(sigma, 0, None)), DRAW, C.c_void_p(again.data_ptr()), env._stream()), env)
                    torch.cuda.synchronize()
                    assert same_bits(np_(again), out) and guards_intact(full), where
        env.close()
    for sigma in (0.3, 25.0):  # not a function of E: parent 0 alone, and the first three parents of 171
        assert same_bits(got[1, sigma][1], got[E, sigma][1][:1]) and same_bits(got[1, sigma][0], got[E, sigma][0][:1])
        assert same_bits(got[E_WIDE, sigma][1][:E], got[E, sigma][1])


# ------------------------------------------------------------------------------------------------ 2, 4. the collection
@pytest.mark.parametrize("mode", list(CONFIGS))
@pytest.mark.parametrize("env_id", ["UR5DynReach-v1", "UR5OriReach-v1"])
def test_collect_is_the_python_stepped_loop(env_id, mode):
    """4 steps with explore_sigma = 0.3 into a ring of 3 slots (the call wraps) on a source that auto-resets with a time limit of 3 steps
    (every env finishes inside the call): ONE urgym_mppi_collect against the Python-stepped loop, and against two calls of 2 + 2 steps --
    every ring tensor, every bound buffer of the source, every buffer of urgym_mppi and of the planner, bit for bit."""
    import torch

    capacity, steps, draw, sigma = 3, 4, 10, 0.3
    (sa, a, fa), (sb, b, fb), (sc, c, fc) = (pair(env_id, mode, **SHORT) for _ in range(3))
    ra, ga = guarded_replay(sa, capacity)
    rc, gc = guarded_replay(sc, capacity)
    ra.collect_planned(a, steps, first_draw=draw, explore_sigma=sigma)
    want, finished = stepped_loop(b, capacity, 0, draw, steps, sigma)
    rc.collect_planned(c, 2, first_draw=draw, explore_sigma=sigma)
    rc.collect_planned(c, 2, first_draw=draw + 2, explore_sigma=sigma)
    torch.cuda.synchronize()
    assert (ra.cursor, ra.filled) == (rc.cursor, rc.filled) == (1, 3)
    assert_same_ring(ra.ring, want, (env_id, mode, "loop"))
    assert_same_everything(a, b, (env_id, mode, "loop"))
    assert_same_ring(ra.ring, rc.ring, (env_id, mode, "2 + 2"))
    assert_same_everything(a, c, (env_id, mode, "2 + 2"))
    assert all(guards_intact(f) for f in (fa, fb, fc, ga, gc))
    # the time limit: every env finished by step 2 at the latest, so slot 2 holds final_* rows, which differ from the next episode's first
    assert finished[:3].any(axis=0).all(), finished
    done2 = finished[2]
    ring = {k: np_(v) for k, v in ra.ring.items()}
    assert done2.any() and same_bits((ring["terminated"][2] | ring["truncated"][2]) != 0, done2)
    assert not (ring["next_observation"][2][done2] == ring["observation"][0][done2]).all(axis=1).any()  # slot 0 now holds the s of step 3
    live = ~done2
    assert same_bits(ring["next_observation"][2][live], ring["observation"][0][live])
    assert np.abs(ring["action"]).max() <= 1.0
    # mean is zeroed for the envs that finished at the last step, and carried for the others
    mean = np_(a.buf["mean"])
    assert not mean[:, finished[3]].any() and (finished[3].all() or mean[:, ~finished[3]].any())
    close(a, b, c, sa, sb, sc)


# ------------------------------------------------------------------------------------------------ 3. agreement with the closed loop
@pytest.mark.parametrize("mode", ["plain", "value_policy"])
def test_collect_without_noise_is_the_closed_loop(mode):
    """explore_sigma = 0: the ring's action, reward and flags are urgym_mppi_control(_guided)'s trajectory of the same seeds and draws, and
    both calls leave the same planner and source."""
    import torch

    env_id, steps, draw = "UR5DynReach-v1", 4, 10
    (sa, a, fa), (sb, b, fb) = (pair(env_id, mode, **SHORT) for _ in range(2))
    rb, gb = guarded_replay(sb, 5)
    traj = a.run(steps, first_draw=draw, record=("action", "reward", "terminated", "truncated", "is_success"))
    rb.collect_planned(b, steps, first_draw=draw)
    torch.cuda.synchronize()
    for key, t in traj.items():
        got = np_(rb.ring[key][:steps])
        assert same_bits(got, np_(t).view(np.uint8) if t.dtype == torch.bool else np_(t)), (mode, key)
    assert_same_everything(a, b, (mode, "control"))
    assert guards_intact(fa) and guards_intact(fb) and guards_intact(gb) and pattern_slots(rb.ring, [4])
    close(a, b, sa, sb)


# ------------------------------------------------------------------------------------------------ 5. no stray writes
def test_collect_writes_its_own_slots_only():
    """3 steps from slot 1 of a ring of 5: slots 0 and 4 keep every byte, slots 1 .. 3 are complete; the envs that met the time limit at the
    last step have their mean zeroed."""
    import torch

    src, mppi, full = pair("UR5OriReach-v1", "value_policy", **SHORT)
    replay, guards = guarded_replay(src, 5)
    replay.cursor = 1
    replay.collect_planned(mppi, 3, first_draw=0, explore_sigma=0.3)
    torch.cuda.synchronize()
    assert (replay.cursor, replay.filled) == (4, 3)
    assert pattern_slots(replay.ring, [0, 4]) and guards_intact(guards) and guards_intact(full)
    for name, t in replay.ring.items():
        raw = np_(t[1:4].contiguous().view(-1).view(torch.uint8)).reshape(3, -1)
        assert not (raw == 0xA5).all(axis=1).any(), name  # every slot of the call was written
    done = (np_(replay.ring["terminated"][3]) | np_(replay.ring["truncated"][3])) != 0
    mean = np_(mppi.buf["mean"])
    assert done.any() and not mean[:, done].any()
    close(mppi, src)


# ------------------------------------------------------------------------------------------------ 6. the refusals
def test_every_refusal_launches_nothing():
    import torch

    lib = _native.lib()
    env_id, who = "UR5DynReach-v1", "urgym_mppi_collect"
    src = make_vec(env_id, E, 1, auto_reset=True)
    src.reset(seed=1)
    fresh = make_vec(env_id, E, 1, auto_reset=True)  # has observed nothing
    planner = make_vec(env_id, E * K, 1, auto_reset=False)
    resetting = make_vec(env_id, E * K, 1, auto_reset=True)
    short = make_vec(env_id, E * K - 1, 1, auto_reset=False)
    ori = make_vec("UR5OriReach-v1", E * K, 1, auto_reset=False)
    from ur_gym_amd.evaluation import DeviceActor, DeviceCritic

    actor, critic = DeviceActor.load(actor_path(env_id), planner), DeviceCritic.load(critic_paths(env_id), planner)
    source_actor = DeviceActor.load(actor_path(env_id), src)
    replay, ring_guards = guarded_replay(src, 4)
    torch.cuda.synchronize()
    before = {key: np_(planner.buf[key]).copy() for key in STATE + OUTPUTS}
    source_before = {key: np_(t).copy() for key, t in src.buf.items()}
    g = Guarded(E, K, HC, policy_samples=2, policy_sigma=0.1, terminal_value=1, fail_cost=10.0, actor=actor, critic=critic)
    full = {}
    full["executed"], executed = pattern_like(g.a["action_out"])
    full["explore_eps"], eps_out = pattern_like(g.a["action_out"])
    x = _abi.MppiExplore(0.3, 0, C.cast(eps_out.data_ptr(), C.POINTER(C.c_float)))
    s = src._stream()

    def edited(struct, **fields):
        new = type(struct).from_buffer_copy(struct)
        for name, value in fields.items():
            setattr(new, name, value)
        return new

    def ref(p):
        return C.byref(p) if p is not None else None

    def collect(M=g.M, G=g.G, X=x, source=src, plan=planner, draw=0, steps=2, ring=replay._ring, slot=0):
        return lib.urgym_mppi_collect(getattr(source, "_h", None), getattr(plan, "_h", None), ref(M), ref(G), ref(X), draw, steps, ref(ring), slot, s)

    def execute(M=g.M, X=x, source=src, draw=0, out=executed):
        return lib.urgym_mppi_execute(getattr(source, "_h", None), ref(M), ref(X), draw, C.c_void_p(out.data_ptr()) if out is not None else None, s)

    def both(*words, **fields):
        """Both entry points refuse the same edit of their shared arguments, each naming itself."""
        refused(collect(**fields), fields.get("source", src), who, *words)
        refused(execute(**{k: v for k, v in fields.items() if k in ("M", "X", "source", "draw")}), fields.get("source", src), "urgym_mppi_execute", *words)

    # the handles and urgym_mppi: what urgym_mppi_control refuses
    refused(collect(source=None), None, "null handle")
    refused(execute(source=None), None, "null handle")
    refused(collect(plan=None), src, who, "null planner handle")
    both("null urgym_mppi", M=None)
    for name, _, _ in _abi.MPPI_FIELDS[:-1]:
        both(f"urgym_mppi.{name} is null", M=edited(g.M, **{name: None}))
    for fields, word in ((dict(samples=1), "samples"), (dict(samples=1025), "samples"), (dict(horizon=0), "horizon"), (dict(horizon=65), "horizon"),
                         (dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"), (dict(num_parents=0), "num_parents"),
                         (dict(sigma=float("nan")), "sigma"), (dict(sigma=-0.5), "sigma"), (dict(lam=0.0), "lam"), (dict(lam=float("nan")), "lam"),
                         (dict(gamma=float("inf")), "gamma"), (dict(reserved0=1), "reserved"), (dict(reserved1=1), "reserved")):
        both(word, M=edited(g.M, **fields))
    both("the source has", M=edited(g.M, num_parents=E + 1))
    refused(collect(plan=resetting), src, who, "auto_reset")
    refused(collect(plan=short), src, who, "num_parents * samples")
    refused(collect(plan=ori), src, who, "urgym_config")
    refused(collect(plan=src), src, who, "the planner has")
    for draw in (1 << 32, (1 << 64) - 1):
        both("2^32", draw=draw)
    refused(collect(draw=(1 << 32) - 1, steps=2), src, who, "2^32")
    for steps in (0, -1):
        refused(collect(steps=steps), src, who, "num_steps")
    # the guide: what urgym_mppi_control_guided refuses
    refused(collect(G=edited(g.G, reserved0=1)), src, who, "reserved0")
    for p in (-1, K):
        refused(collect(G=edited(g.G, policy_samples=p)), src, who, "policy_samples")
    refused(collect(G=edited(g.G, actor=None)), src, who, "actor is null")
    refused(collect(G=edited(g.G, critic=None)), src, who, "critic is null")
    refused(collect(G=edited(g.G, actor=source_actor._a)), src, who, "actor is not an actor of the planner handle")
    for value in (float("nan"), float("inf"), -0.5):
        refused(collect(G=edited(g.G, policy_sigma=value)), src, who, "policy_sigma")
        refused(collect(G=edited(g.G, fail_cost=value)), src, who, "fail_cost")
    for name in ("policy_action", "value", "terminal"):
        refused(collect(G=edited(g.G, **{name: None})), src, who, f"{name} is null")
    # the exploration
    both("null urgym_mppi_explore", X=None)
    both("reserved0", X=edited(x, reserved0=1))
    for value in (float("nan"), float("inf"), -float("inf"), -0.5):
        both("explore_sigma", X=edited(x, explore_sigma=value))
    refused(execute(out=None), src, "urgym_mppi_execute", "executed is null")
    # the ring and the source's state: what urgym_rollout_collect refuses
    refused(collect(ring=None), src, who, "null ring")
    refused(collect(ring=edited(replay._ring, capacity_steps=0)), src, who, "capacity_steps")
    refused(collect(ring=edited(replay._ring, reserved0=1)), src, who, "reserved0")
    for name, _, _, required in _abi.REPLAY_RING_FIELDS:
        if required:
            refused(collect(ring=edited(replay._ring, **{name: None})), src, who, "ring pointer is null")
    for slot in (-1, 4):
        refused(collect(slot=slot), src, who, "first_slot")
    refused(collect(source=fresh), fresh, who, "observed")
    torch.cuda.synchronize()
    assert g.untouched() and g.guards_intact() and guards_intact(full) and guards_intact(ring_guards)
    assert pattern_slots(replay.ring, slice(None)) and pattern_slots({"executed": executed, "explore_eps": eps_out}, slice(None))
    for key in STATE + OUTPUTS:
        assert same_bits(np_(planner.buf[key]), before[key]), key
    for key, want in source_before.items():
        assert same_bits(np_(src.buf[key]), want), key
    # the Python layers say the same before they call
    mppi = DeviceMPPI(src, samples=K, horizon=HC)
    other = DeviceReplay(fresh, 4)
    for call in (lambda: mppi.execute(0, -1.0), lambda: mppi.execute(0, float("nan")), lambda: replay.collect_planned(mppi, 2, explore_sigma=float("inf")),
                 lambda: replay.collect_planned(mppi, 0), lambda: other.collect_planned(mppi, 2)):
        with pytest.raises(ValueError):
            call()
    assert (replay.cursor, replay.filled, other.cursor, other.filled) == (0, 0, 0, 0)
    close(mppi, actor, critic, source_actor, src, fresh, planner, resetting, short, ori)


# ------------------------------------------------------------------------------------------------ 7. the learner
ALL = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)


class Side:
    """An env, a SACLearner on it and a planner guided by the learner's own initial parameters; the same bits whichever side it is."""

    def __init__(self, replay=DeviceReplay, capacity=6, **hp):
        from ur_gym_amd.training import SACLearner, host_arrays

        self.env = make_vec("UR5OriReach-v1", E, 21, **SHORT)
        self.env.reset(seed=21)
        self.learner = SACLearner(self.env, seed=5, hidden_width=32, batch_size=64, **ALL, **hp)
        self.mppi = DeviceMPPI(self.env, samples=K, horizon=HC, sigma=0.3, lam=20.0, gamma=0.95, seed=8, keep_weights=True,
                               actor=host_arrays(self.learner.actor.tensors()), critic=host_arrays(self.learner.critic.tensors()), **CONFIGS["value_policy"])
        self.mppi_guards = guard(self.mppi)
        self.replay, self.ring_guards = guarded_replay(self.env, capacity, replay)

    def close(self):
        close(self.mppi, self.learner, self.env)


def test_learner_collects_with_a_planner():
    import torch

    from ur_gym_amd.training import SACLearner

    steps, sigma = 4, 0.3
    a, b = Side(), Side()
    mon, after = DeviceMonitor(a.env), DeviceMonitor(a.env)
    a.learner.draw = b.learner.draw = 7
    a.learner.collect(a.replay, steps, monitor=mon, planner=a.mppi, explore_sigma=sigma)
    want, _ = stepped_loop(b.mppi, 6, 0, 7, steps, sigma)
    after.fold(a.replay, 0, steps)
    torch.cuda.synchronize()
    assert (a.learner.env_steps, a.learner.draw, a.replay.cursor, a.replay.filled) == (steps, 7 + steps, steps, steps)
    assert_same_ring(a.replay.ring, want, "learner")
    assert_same_everything(a.mppi, b.mppi, "learner")
    assert pattern_slots(a.replay.ring, [4, 5]) and guards_intact(a.ring_guards) and guards_intact(a.mppi_guards)
    for key in mon.state:  # monitor= is a fold of those slots
        assert same_bits(np_(mon.state[key]), np_(after.state[key])), key
    assert np_(mon.state["episodes"]).sum() >= E  # the time limit of 3 steps closed an episode per env
    # update runs on what the planner collected, and sync_planner puts the planner on the stepped parameters
    losses = a.learner.update(a.replay, 3, 0)
    torch.cuda.synchronize()
    assert all(np.isfinite(np_(v)).all() for v in losses.values())
    assert not same_bits(a.mppi.actor.packed(), a.learner.device_actor.packed()) and not same_bits(a.mppi.critic.packed(), a.learner.online.packed())
    a.learner.sync_planner(a.mppi)
    torch.cuda.synchronize()
    assert same_bits(a.mppi.actor.packed(), a.learner.device_actor.packed()) and same_bits(a.mppi.critic.packed(), a.learner.online.packed())
    plain = DeviceMPPI(a.env, samples=K, horizon=HC)  # neither an actor nor a critic: nothing to reload
    a.learner.sync_planner(plain)
    plain.close()
    # what is refused: a planner of another env, exploration noise without a planner
    for call in (lambda: b.learner.collect(b.replay, 1, planner=a.mppi), lambda: b.learner.collect(b.replay, 1, explore_sigma=0.3)):
        with pytest.raises(ValueError):
            call()
    # a learner without a planner makes the calls it made: planner=None against the call without the keyword, bit for bit
    c, d = Side(), Side()
    c.learner.collect(c.replay, 2)
    d.learner.collect(d.replay, 2, monitor=None, planner=None, explore_sigma=0.0)
    torch.cuda.synchronize()
    assert_same_ring(c.replay.ring, d.replay.ring, "no planner")
    assert (c.learner.env_steps, c.learner.draw) == (d.learner.env_steps, d.learner.draw) == (2, 2)
    # normalize=True with a planner is refused, with a message, before anything runs
    e = Side(normalize=True)
    with pytest.raises(ValueError, match="normalize"):
        e.learner.collect(e.replay, 1, planner=e.mppi)
    torch.cuda.synchronize()
    assert pattern_slots(e.replay.ring, slice(None)) and (e.learner.env_steps, e.replay.filled) == (0, 0)
    assert isinstance(e.learner, SACLearner)
    close(a, b, c, d, e)


def test_a_prioritized_ring_fills_the_new_leaves():
    import torch

    side = Side(replay=DevicePrioritizedReplay, prioritized=True)
    side.replay.cursor = 1
    side.learner.collect(side.replay, 3, planner=side.mppi, explore_sigma=0.3)
    torch.cuda.synchronize()
    leaf = np_(side.replay.leaf)
    assert (leaf[1:4] == np_(side.replay.max_leaf)[0]).all() and leaf[1:4].all() and not leaf[[0, 4, 5]].any()
    assert pattern_slots(side.replay.ring, [0, 4, 5]) and guards_intact(side.ring_guards)
    losses = side.learner.update(side.replay, 3, 0)
    torch.cuda.synchronize()
    assert all(np.isfinite(np_(v)).all() for v in losses.values())
    side.close()
