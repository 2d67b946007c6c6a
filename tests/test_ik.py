"""GPU tests (-m gpu) of the scripted reach controller (include/urgym.h, "a scripted reach controller on the device"; DESIGN.md section
37): the action launch against its float64 restatement (ur_gym_amd.evaluation.ik_actions) within 2^-22, row by row independence, the
exploration noise bit for bit, urgym_controller_control and urgym_controller_collect against the Python-stepped loops they promise to
be, the success floor on UR5OriReach-v1, stream order, every refusal, and the learner's side.

Shapes: N = 1, 63, 64, 65, 257 for the single launch (a wave's tail, a whole wave, one lane past it, a workgroup and one lane); N = 64
for the loops (40 steps with auto-reset: episodes last about 12 steps, so resets are crossed); N = 256 for the floor.  Every output
array lies between guard words.
"""
import ctypes as C

import numpy as np
import pytest

import ik_cases as K
from test_mppi_guide import GUARD, check, guards_intact, make_vec, np_, refused, same_bits
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import (DevicePrioritizedReplay, DeviceReachController, DeviceReplay, ik_actions, ik_explore_noise, mppi_execute,
                                   run_closed_loop_controller)

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)
ROWS = ("observation", "achieved_goal", "desired_goal")


def pattern(shape, dtype=None):
    """(the guarded tensor, the view of `shape` inside it), every byte 0xA5."""
    import torch

    dtype = dtype or torch.float32
    count = int(np.prod(shape))
    raw = torch.full(((count + 2 * GUARD) * torch.empty((), dtype=dtype).element_size(),), 0xA5, dtype=torch.uint8, device="cuda:0")
    full = raw.view(dtype)
    return full, full[GUARD:GUARD + count].view(shape)


def is_pattern(t):
    import torch

    return bool((np_(t.contiguous().view(-1).view(torch.uint8)) == 0xA5).all())


def guarded_replay(env, capacity, cls=DeviceReplay):
    replay, full = cls(env, capacity), {}
    for name, ct, _, _ in _abi.REPLAY_RING_FIELDS:
        full[name], replay.ring[name] = pattern(replay.ring[name].shape, replay.ring[name].dtype)
        setattr(replay._ring, name, C.cast(replay.ring[name].data_ptr(), C.POINTER(ct)))
    return replay, full


def state_of(env):
    """(q [N, 6], goal [N, 6]) the env holds, on the host."""
    return np_(env.buf["q"]).T.copy(), np_(env.buf["goal"]).T.copy()


def reference(env, damping=K.DAMPING, gain=K.GAIN):
    q, goal = state_of(env)
    return ik_actions(q, goal, env.env_kind, damping, gain, env.cfg.action_scale)


def plant_cases(env, oracle):
    """Overwrites the first envs' q and goal with the shared cases of tests/ik_cases.py (as many as fit): the launch reads the bound state
    and nothing derived from it."""
    import torch

    q, goal, names = K.cases(oracle, env.env_kind)
    keep = ~K.dropped(q, goal, env.env_kind)
    assert keep.all()
    order = np.r_[np.arange(K.RANDOM, len(q)), np.arange(K.RANDOM)][:env.num_envs]  # the special rows first
    n = len(order)
    env.buf["q"][:, :n] = torch.from_numpy(q[order].T.copy()).to(env.device)
    env.buf["goal"][:, :n] = torch.from_numpy(goal[order].T.copy()).to(env.device)
    return [names[i] for i in order]


# ------------------------------------------------------------------------------------------------ 1. the single launch
@pytest.mark.parametrize("kind", K.KINDS)
def test_single_launch_against_the_reference(kind, oracle):
    """urgym_controller_actions against ik_actions on the state the env holds -- after a reset and two random steps, then with the shared
    cases planted -- for every kind at N = 1, 63, 64, 65, 257 and three dampings: within 2^-22, finite, |a| <= 1, guards intact."""
    import torch

    rng = np.random.default_rng(3)
    for n in SIZES:
        env = make_vec(K.KIND_IDS[kind], n, 5, auto_reset=True)
        env.reset(seed=5)
        for _ in range(2):
            env.step(torch.from_numpy(rng.uniform(-1, 1, (n, 6)).astype(np.float32)).to(env.device))
        for planted in (False, True):
            names = plant_cases(env, oracle) if planted else []
            for damping in K.DAMPINGS:
                full, out = pattern((n, 6))
                env.controller_actions(out=out, damping=damping, gain=K.GAIN)
                torch.cuda.synchronize()
                got, want = np_(out), reference(env, damping)
                err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
                print(f"kind {kind} N {n} planted {planted} damping {damping}: max |device - ik_actions| = {err:.3e} (bound {K.BOUND:.3e})")
                assert guards_intact({"actions": full}) and np.isfinite(got).all() and np.abs(got).max() <= 1.0
                assert err <= K.BOUND, (kind, n, planted, damping, err)
            if planted and "far_goal" in names and "own_goal" in names:
                got = np_(env.controller_actions())
                assert np.abs(got[names.index("far_goal")]).max() == 1.0 and np.abs(got[names.index("own_goal")]).max() < 1e-6
        env.close()


# ------------------------------------------------------------------------------------------------ 2. row independence
@pytest.mark.parametrize("kind", (_abi.ENV_ORI, _abi.ENV_OBS))
def test_rows_are_independent(kind):
    """Env n's six floats are bitwise the same at N = 257 and in a one-env handle given the same state; a NaN planted in one env's q or in
    its goal zeroes that row only."""
    import torch

    wide, one = make_vec(K.KIND_IDS[kind], 257, 9), make_vec(K.KIND_IDS[kind], 1, 9)
    wide.reset(seed=9), one.reset(seed=2)
    base = np_(wide.controller_actions())
    for n in (0, 63, 64, 200, 256):
        one.buf["q"][:, 0], one.buf["goal"][:, 0] = wide.buf["q"][:, n], wide.buf["goal"][:, n]
        assert same_bits(np_(one.controller_actions())[0], base[n]), (kind, n)
    wide.buf["q"][3, 70], wide.buf["goal"][1, 130], wide.buf["q"][0, 256] = float("nan"), float("inf"), -float("inf")
    wide.buf["goal"][4, 5] = float("nan")  # a column UR5ObsReach-v1 does not read
    got = np_(wide.controller_actions())
    zero = np.zeros(257, bool)
    zero[[70, 130, 256]] = True
    zero[5] = wide.goal_dim == 6
    assert (got[zero].view(np.uint32) == 0).all() and same_bits(got[~zero], base[~zero]), kind
    assert np.abs(got.astype(np.float64) - reference(wide)).max() <= K.BOUND
    wide.close(), one.close()


# ------------------------------------------------------------------------------------------------ 3. the noise
def noise_runs():
    """For N = 65 and 257 on UR5DynReach-v1: (plain action, {sigma: (executed, explore_eps)}), guards checked, from one env each."""
    import torch

    runs = {}
    for n in (65, 257):
        env = make_vec("UR5DynReach-v1", n, 4)
        env.reset(seed=4)
        plain = np_(env.controller_actions())
        fe, eps = pattern((n, 6))
        fa, out = pattern((n, 6))
        by_sigma = {}
        for sigma in (0.0, 0.3, 25.0):
            env.controller_actions(out=out, draw=NOISE_DRAW, seed=NOISE_SEED, explore_sigma=sigma, explore_eps=eps)
            torch.cuda.synchronize()
            by_sigma[sigma] = (np_(out).copy(), np_(eps).copy())
        assert guards_intact({"eps": fe, "out": fa})
        runs[n] = (env, plain, by_sigma)
    return runs


NOISE_SEED, NOISE_DRAW = 0xFEEDFACE12345678, 41


def test_exploration_noise():
    """The executed row is bitwise the execute line on (the sigma = 0 action, the eps the launch reports); with sigma = 0 the bits equal the
    plain call's and explore_eps is zeros; the same draw gives the same bits, another draw or key gives others; the noise is no function
    of N; and eps is within the bound the planner's own eps is held to (mppi_collect_cases.noise_bound) of the float64 restatement."""
    from mppi_collect_cases import noise_bound

    runs, bound = noise_runs(), noise_bound()
    for n, (env, plain, by_sigma) in runs.items():
        out0, eps0 = by_sigma[0.0]
        assert same_bits(out0, plain) and not eps0.any() and not np.signbit(eps0).any()
        f64 = ik_explore_noise(NOISE_SEED, NOISE_DRAW, n, dtype=np.float64)
        for sigma in (0.3, 25.0):
            out, e = by_sigma[sigma]
            dev = float(np.abs(e.astype(np.float64) - f64).max())
            print(f"exploration noise N={n} sigma={sigma}: device vs float64 restatement {dev:.3e}, bound {bound:.3e}")
            assert dev <= bound, (n, sigma, dev, bound)
            assert same_bits(out, mppi_execute(plain, e, sigma)), (n, sigma)
            again = np_(env.controller_actions(draw=NOISE_DRAW, seed=NOISE_SEED, explore_sigma=sigma))  # the same draw, no explore_eps
            assert same_bits(again, out)
            other = np_(env.controller_actions(draw=NOISE_DRAW + 1, seed=NOISE_SEED, explore_sigma=sigma))
            keyed = np_(env.controller_actions(draw=NOISE_DRAW, seed=NOISE_SEED + 1, explore_sigma=sigma))
            assert not same_bits(other, again) and not same_bits(keyed, again)
            if sigma == 25.0:
                assert (again == 1).mean() > 0.3 and (again == -1).mean() > 0.3
        assert same_bits(by_sigma[0.3][1], by_sigma[25.0][1])
    assert same_bits(runs[257][2][0.3][1][:65], runs[65][2][0.3][1])
    for env, _, _ in runs.values():
        env.close()


def test_exploration_noise_is_bitwise_the_restatement():
    """explore_eps is bitwise ik_explore_noise.  The kernel's Box-Muller states ln, cos and sin as float64 lines of its own
    (urgym_ik.h), which numpy restates exactly; with the device library's logf, cospif and sinpif in their place 236 of 390 elements
    (N = 65) and 977 of 1,542 (N = 257) differed from numpy's float32 evaluation, by up to 8.9e-7."""
    runs = noise_runs()
    bad = []
    for n, (env, plain, by_sigma) in runs.items():
        e, want = by_sigma[0.3][1], ik_explore_noise(NOISE_SEED, NOISE_DRAW, n)
        differ = e.view(np.uint32) != want.view(np.uint32)
        ulps = np.abs(e.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        print(f"exploration noise N={n}: {int(differ.sum())} of {differ.size} elements differ from ik_explore_noise, "
              f"max |difference| {float(np.abs(e.astype(np.float64) - want.astype(np.float64)).max()):.3e}, max distance {int(ulps.max())} float32 steps")
        bad.append((n, int(differ.sum())))
        env.close()
    assert all(count == 0 for _, count in bad), bad


# ------------------------------------------------------------------------------------------------ 4. closed loop and collection
def stepped(env, steps, first_draw, sigma, seed, capacity=None, first_slot=0):
    """The Python loop of controller_actions + env.step: (the trajectory as a dict of [steps, N, ...] arrays, the ring it would leave as a
    dict of tensors that were 0xA5 throughout, or None without a capacity)."""
    import torch

    traj = {k: [] for k in ROWS + ("action", "reward", "terminated", "truncated", "is_success", "collision")}
    ring = None
    if capacity is not None:
        ring = {name: pattern(shape(capacity, env.num_envs, env.obs_dim, env.goal_dim), torch.uint8 if ct is C.c_uint8 else torch.float32)[1]
                for name, ct, shape, _ in _abi.REPLAY_RING_FIELDS}
    b = env.buf
    for t in range(steps):
        for k in ROWS:
            traj[k].append(np_(b[k]).copy())
        a = env.controller_actions(draw=first_draw + t, seed=seed, explore_sigma=sigma)
        if ring is not None:
            slot = (first_slot + t) % capacity
            for k in ROWS:
                ring[k][slot] = b[k]
            ring["action"][slot] = a
        env.step(a)
        traj["action"].append(np_(a).copy())
        for k in ("reward", "terminated", "truncated", "is_success", "collision"):
            traj[k].append(np_(b[k]).copy())
        if ring is not None:
            done = (b["terminated"] | b["truncated"]).bool()
            for k in ROWS:
                final = b["final_observation" if k == "observation" else "final_" + k]
                ring["next_" + k][slot] = torch.where(done[:, None], final, b[k]) if env.cfg.auto_reset else b[k]
            for k in ("reward", "terminated", "truncated", "is_success"):
                ring[k][slot] = b[k]
    return {k: np.stack(v) for k, v in traj.items()}, ring


def same_state(a, b, where):
    for key in a.buf:
        assert same_bits(np_(a.buf[key]), np_(b.buf[key])), (where, key)


@pytest.mark.parametrize("env_id", ["UR5OriReach-v1", "UR5DynReach-v1"])
def test_control_and_collect_are_the_python_loop(env_id):
    """N = 64, 40 steps with auto-reset and explore_sigma = 0.1: ONE urgym_controller_control and ONE urgym_controller_collect against the
    Python loop, bit for bit -- trajectory, ring (capacity 16 < 40: it wraps), bound buffers; two collect calls of 15 + 25 steps against
    one; and at sigma = 0 the ring's action, reward and flags against the trajectory's."""
    import torch

    n, steps, draw, sigma, seed, cap = 64, 40, 6, 0.1, 77, 16
    envs = [make_vec(env_id, n, 13, auto_reset=True) for _ in range(6)]
    for e in envs:
        e.reset(seed=13)
    a, b, c, d, e0, f0 = envs
    want_traj, want_ring = stepped(a, steps, draw, sigma, seed, capacity=cap)
    got = DeviceReachController(b, seed=seed).run(steps, first_draw=draw, record="all", explore_sigma=sigma)
    rc, gc = guarded_replay(c, cap)
    rc.collect_scripted(DeviceReachController(c, seed=seed), steps, first_draw=draw, explore_sigma=sigma)
    rd, gd = guarded_replay(d, cap)
    ctl = DeviceReachController(d, seed=seed)
    rd.collect_scripted(ctl, 15, first_draw=draw, explore_sigma=sigma)
    rd.collect_scripted(ctl, 25, first_draw=draw + 15, explore_sigma=sigma)
    torch.cuda.synchronize()
    done = (want_traj["terminated"] | want_traj["truncated"]).astype(bool)
    assert done.any(axis=0).mean() > 0.9 and done[:-1].any(), "episodes end inside the call, so auto-resets are crossed"
    for key, want in want_traj.items():
        t = got[key]
        assert same_bits(np_(t).view(np.uint8) if t.dtype == torch.bool else np_(t), want), (env_id, "control", key)
    final = np_(got["final_observation"])
    assert final[done].any() and not final[~done].any()
    assert (rc.cursor, rc.filled) == (rd.cursor, rd.filled) == (steps % cap, cap)
    for name in want_ring:
        assert same_bits(np_(rc.ring[name]), np_(want_ring[name])), (env_id, "collect", name)
        assert same_bits(np_(rd.ring[name]), np_(rc.ring[name])), (env_id, "15 + 25", name)
    for other, where in ((b, "control"), (c, "collect"), (d, "15 + 25")):
        same_state(a, other, (env_id, where))
    assert guards_intact(gc) and guards_intact(gd)
    # sigma = 0: the ring's action, reward and flags are the trajectory's
    traj = DeviceReachController(e0).run(12, record=("action", "reward", "terminated", "truncated", "is_success"))
    rf, gf = guarded_replay(f0, cap)
    rf.collect_scripted(DeviceReachController(f0), 12)
    torch.cuda.synchronize()
    for key, t in traj.items():
        assert same_bits(np_(rf.ring[key][:12]), np_(t).view(np.uint8) if t.dtype == torch.bool else np_(t)), (env_id, "sigma 0", key)
    assert all(is_pattern(t[12:]) for t in rf.ring.values()) and guards_intact(gf)
    same_state(e0, f0, (env_id, "sigma 0"))
    for x in envs:
        x.close()


def test_collect_writes_its_own_slots_only():
    """3 steps from slot 1 of a ring of 5: slots 0 and 4 keep every byte, slots 1 .. 3 are complete."""
    import torch

    env = make_vec("UR5StaReach-v1", 65, 2, auto_reset=True)
    env.reset(seed=2)
    replay, guards = guarded_replay(env, 5, DevicePrioritizedReplay)
    replay.cursor = 1
    replay.collect_scripted(DeviceReachController(env), 3, explore_sigma=0.2)
    torch.cuda.synchronize()
    assert (replay.cursor, replay.filled) == (4, 3) and guards_intact(guards)
    assert all(is_pattern(t[[0, 4]]) for t in replay.ring.values())
    for name, t in replay.ring.items():
        raw = np_(t[1:4].contiguous().view(-1).view(torch.uint8)).reshape(3, -1)
        assert not (raw == 0xA5).all(axis=1).any(), name
    leaf = np_(replay.leaf)
    assert leaf[1:4].all() and not leaf[[0, 4]].any()  # the prioritized ring's override filled the new leaves
    env.close()


# ------------------------------------------------------------------------------------------------ 5. it reaches
def test_it_actually_reaches():
    """UR5OriReach-v1, N = 256, reset(seed=1), 100 steps, the default parameters: success >= 0.80, the floor of the CPU measurement
    (0.906 and 0.879 on two seeds with the numpy controller on the oracle; one standard error at 256 envs is 0.019)."""
    env = make_vec("UR5OriReach-v1", 256, 1, auto_reset=False)
    env.reset(seed=1)
    res = run_closed_loop_controller(env, max_steps=100)
    print(f"UR5OriReach-v1 N=256 seed 1: success {res['success_rate_percent']:.2f} %, mean last step {res['mean_last_step_index']:.2f}, "
          f"mean episode reward {res['mean_episode_reward']:.1f}")
    assert res["success"].mean() >= 0.80
    env.close()


# ------------------------------------------------------------------------------------------------ 6. stream order
def test_stream_order():
    """The launch is enqueued on a side stream behind a delayed writer of q: it reads what that writer wrote, not what was there when the
    call was made."""
    import torch

    env = make_vec("UR5OriReach-v1", 257, 6)
    env.reset(seed=6)
    before = reference(env)
    new_q = env.buf["q"].clone() + 0.3
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    big = torch.randn((2048, 2048), device=env.device)
    with torch.cuda.stream(side):
        for _ in range(20):  # the delay: work the writer has to wait behind
            big = big @ big * 1e-3
        env.buf["q"].copy_(new_q)
        out = env.controller_actions()
    side.synchronize()
    torch.cuda.synchronize()
    want = reference(env)
    assert np.abs(np_(out).astype(np.float64) - want).max() <= K.BOUND and np.abs(want.astype(np.float64) - before).max() > 1e-3
    env.close()


# ------------------------------------------------------------------------------------------------ 7. the refusals
def test_every_refusal_launches_nothing():
    import torch

    lib = _native.lib()
    env = make_vec("UR5DynReach-v1", 65, 1, auto_reset=True)
    env.reset(seed=1)
    fresh = make_vec("UR5DynReach-v1", 65, 1, auto_reset=True)  # has observed nothing
    unbound = C.c_void_p()
    cfg = _abi.Config()
    assert lib.urgym_config_default(_abi.ENV_DYN, 65, C.byref(cfg)) == 0 and lib.urgym_create(C.byref(cfg), 0, C.byref(unbound)) == 0
    replay, ring_guards = guarded_replay(env, 4)
    fa, out = pattern((65, 6))
    fe, eps = pattern((65, 6))
    ft, rows = pattern((2, 65, 6))
    fr, done_rows = pattern((65,), torch.float64)
    torch.cuda.synchronize()
    before = {key: np_(t).copy() for key, t in env.buf.items()}
    good = _abi.ReachController(0.2, 0.5, 3, 0.3, 0, C.cast(eps.data_ptr(), C.POINTER(C.c_float)))
    traj = _abi.Trajectory()
    traj.action = C.cast(rows.data_ptr(), C.POINTER(C.c_float))
    s = env._stream()

    def edited(struct, **fields):
        new = type(struct).from_buffer_copy(struct)
        for name, value in fields.items():
            setattr(new, name, value)
        return new

    def ref(p):
        return C.byref(p) if p is not None else None

    def handle(x):
        return x if isinstance(x, C.c_void_p) or x is None else x._h

    def actions(c=good, h=env, draw=0, o=out):
        return lib.urgym_controller_actions(handle(h), ref(c), draw, C.c_void_p(o.data_ptr()) if o is not None else None, s)

    def control(c=good, h=env, draw=0, steps=2, t=traj):
        return lib.urgym_controller_control(handle(h), ref(c), draw, steps, ref(t), s)

    def collect(c=good, h=env, draw=0, steps=2, ring=replay._ring, slot=0):
        return lib.urgym_controller_collect(handle(h), ref(c), draw, steps, ref(ring), slot, s)

    calls = (("urgym_controller_actions", actions), ("urgym_controller_control", control), ("urgym_controller_collect", collect))

    def all_three(*words, **fields):
        for who, call in calls:
            rc = call(**fields)
            assert rc == _abi.ERR_ARG, (who, fields, rc)
            refused(rc, handle(fields.get("h", env)), who, *words)

    for who, call in calls:
        rc = call(h=None)
        assert rc == _abi.ERR_ARG
        refused(rc, None, "null handle")
    all_three("null urgym_reach_controller", c=None)
    all_three("urgym_bind", h=unbound)
    all_three("reserved0", c=edited(good, reserved0=1))
    for value in (float("nan"), float("inf"), 0.0, 9.9e-3, 10.001, -0.2):
        all_three("damping", c=edited(good, damping=value))
    for value in (float("nan"), float("inf"), 0.0, -0.5, 10.001):
        all_three("gain", c=edited(good, gain=value))
    for value in (float("nan"), float("inf"), -float("inf"), -0.5):
        all_three("explore_sigma", c=edited(good, explore_sigma=value))
    for draw in (1 << 32, (1 << 64) - 1):
        all_three("2^32", draw=draw)
    assert actions(o=None) == _abi.ERR_ARG
    refused(-1, env, "urgym_controller_actions", "actions is null")
    for who, call in calls[1:]:
        assert call(draw=(1 << 32) - 1, steps=2) == _abi.ERR_ARG
        refused(-1, env, who, "2^32")
        for steps in (0, -1):
            assert call(steps=steps) == _abi.ERR_ARG
            refused(-1, env, who, "num_steps")
        rc = call(h=fresh)
        refused(rc, fresh, who, "observed")
    # the trajectory of the closed loop
    assert control(t=None) == _abi.ERR_ARG and control(t=_abi.Trajectory()) == _abi.ERR_ARG
    refused(-1, env, "urgym_controller_control", "traj->action")
    summary = edited(traj, episode_return=C.cast(done_rows.data_ptr(), C.POINTER(C.c_double)))
    assert control(t=summary) == _abi.ERR_ARG
    refused(-1, env, "urgym_controller_control", "episode_done")
    # the ring: what urgym_rollout_collect refuses
    who = "urgym_controller_collect"
    for fields, word in ((dict(ring=None), "null ring"), (dict(ring=edited(replay._ring, capacity_steps=0)), "capacity_steps"),
                         (dict(ring=edited(replay._ring, reserved0=1)), "reserved0"), (dict(slot=-1), "first_slot"), (dict(slot=4), "first_slot")):
        assert collect(**fields) == _abi.ERR_ARG
        refused(-1, env, who, word)
    for name, _, _, required in _abi.REPLAY_RING_FIELDS:
        if required:
            assert collect(ring=edited(replay._ring, **{name: None})) == _abi.ERR_ARG
            refused(-1, env, who, "ring pointer is null")
    torch.cuda.synchronize()
    assert guards_intact(ring_guards) and guards_intact({"a": fa, "e": fe, "t": ft, "r": fr})
    assert all(is_pattern(t) for t in replay.ring.values()) and all(is_pattern(t) for t in (out, eps, rows, done_rows))
    for key, want in before.items():
        assert same_bits(np_(env.buf[key]), want), key
    # the good arguments are accepted
    check(actions(), env), check(control(), env), check(collect(), env)
    torch.cuda.synchronize()
    assert not is_pattern(out) and not is_pattern(rows) and not is_pattern(replay.ring["action"][:2])
    # the Python layers say the same before they call
    other = DeviceReplay(fresh, 4)
    ctl = DeviceReachController(env)
    for call in (lambda: DeviceReachController(env, damping=0.0), lambda: DeviceReachController(env, gain=11.0), lambda: ctl.actions(explore_sigma=-1.0),
                 lambda: ctl.actions(draw=1 << 32), lambda: replay.collect_scripted(ctl, 0), lambda: other.collect_scripted(ctl, 2), lambda: ctl.run(0),
                 lambda: ctl.actions(out=torch.zeros((64, 6), device=env.device))):
        with pytest.raises(ValueError):
            call()
    assert (other.cursor, other.filled) == (0, 0)
    assert lib.urgym_destroy(unbound) == 0
    env.close(), fresh.close()


# ------------------------------------------------------------------------------------------------ 8. the learner
def test_the_learner_collects_with_the_controller():
    """SACLearner.collect(controller=) fills the slots DeviceReplay.collect_scripted fills, bit for bit, and advances the learner's
    counters; controller= and planner= are alternatives; a demonstration ring filled this way feeds urgym_replay_sample_mixed unchanged."""
    import torch

    from ur_gym_amd.training import SACLearner

    ALL = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)
    n, steps, sigma = 8, 5, 0.2
    a, b, demo_env = (make_vec("UR5OriReach-v1", m, 21, auto_reset=True) for m in (n, n, 3))
    for e in (a, b, demo_env):
        e.reset(seed=21)
    learner = SACLearner(a, seed=5, hidden_width=32, batch_size=16, **ALL)
    ra, ga = guarded_replay(a, 6)
    rb, gb = guarded_replay(b, 6)
    learner.draw = 7
    learner.collect(ra, steps, controller=DeviceReachController(a, seed=9), explore_sigma=sigma)
    rb.collect_scripted(DeviceReachController(b, seed=9), steps, first_draw=7, explore_sigma=sigma)
    torch.cuda.synchronize()
    assert (learner.env_steps, learner.draw, ra.cursor, ra.filled) == (steps, 7 + steps, steps, steps)
    for name in ra.ring:
        assert same_bits(np_(ra.ring[name]), np_(rb.ring[name])), name
    assert all(is_pattern(t[5:]) for t in ra.ring.values()) and guards_intact(ga) and guards_intact(gb)
    same_state(a, b, "learner")
    for call in (lambda: learner.collect(ra, 1, controller=DeviceReachController(b)), lambda: learner.collect(ra, 1, controller=DeviceReachController(a), planner=object())):
        with pytest.raises(ValueError):
            call()
    losses = learner.update(ra, 3, 0)  # the update runs on what the controller collected
    torch.cuda.synchronize()
    assert all(np.isfinite(np_(v)).all() for v in losses.values())
    # a demonstration ring filled by the controller, read by the mixed gather
    demo = DeviceReplay(demo_env, 4)
    demo.collect_scripted(DeviceReachController(demo_env), 4)
    D, count = 6, 16
    batch = ra.sample(count, 11, 2, demonstrations=(demo, D))
    torch.cuda.synchronize()
    source, index = np_(batch["source"]), np_(batch["index"])
    assert source.tolist() == [1] * D + [0] * (count - D)
    flat_demo, flat_own = np_(demo.ring["action"]).reshape(-1, 6), np_(ra.ring["action"]).reshape(-1, 6)
    assert same_bits(np_(batch["actions"])[:D], flat_demo[index[:D]]) and same_bits(np_(batch["actions"])[D:], flat_own[index[D:]])
    assert (index[:D] < 4 * 3).all() and np.abs(np_(batch["actions"])).max() <= 1.0
    learner.close()
    for e in (a, b, demo_env):
        e.close()
