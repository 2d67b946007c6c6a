"""The device replay ring: urgym_rollout_collect / urgym_replay_sample through ``DeviceReplay``, ``env.collect`` and the numpy
restatement ``replay_indices``.

Everything on the device is compared BITWISE: both kernels only move 32-bit words and bytes, and the index draw is integer
arithmetic, so there is no tolerance anywhere in this file.  The one statistical bound (the bucket check) is 5 standard deviations
of a binomial count: 65536 draws, 16 buckets -> sd = sqrt(65536 * (1 / 16) * (15 / 16)) = 61.97, 5 sd = 310.  size = 5 * 417 = 2085
is no multiple of 16, so the buckets floor(16 e / size) hold 130 or 131 entries of 2085 and their expected counts lie between 4086
and 4118 -- within 22 of 4096, small against 310; the bound is applied about 4096 as stated.

The collection case (seed 3, max_episode_steps 6, noise seed 29 from draw 100) was chosen with the CPU oracle and the numpy
``StochasticActor``: of the 5 x 417 transitions in the live slots of a 13-step collection into 5 slots, UR5DynReach-v1 has 92
terminated, 324 truncated-not-terminated and 1669 unfinished rows, UR5ObsReach-v1 48 / 369 / 1668 (dozens of each, so the device
actor's rounding cannot empty a class); the GPU test asserts all three on its own Python-stepped side.

The GPU tests below have NOT been run yet: no MI355X could be had while this file was written.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from test_critic import critic_paths, hyper
from test_policy_sampling import _make, _same_bits, _same_state
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import DeviceCritic, DeviceReplay, TwinCritic, philox4x32_10, replay_indices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("urgym_rollout_collect", "urgym_replay_sample")
RING_KEYS = tuple(name for name, _, _, _ in _abi.REPLAY_RING_FIELDS)
N, CAP, K = 417, 5, 13  # not a multiple of the wave or a workgroup; the ring wraps twice and ends mid-ring
ENV_SEED, STEP_LIMIT = 3, 6
HOW = dict(mode="gaussian", seed=29, first_draw=100)
BUCKET_SEED, BUCKET_DRAW = 5, 7  # verified once: the 16 counts lie in [3917, 4255]


# ------------------------------------------------------------------------------------------------ CPU
def test_replay_structs_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    ctype = {"float*": C.POINTER(C.c_float), "uint8_t*": C.POINTER(C.c_uint8), "int64_t*": C.POINTER(C.c_int64), "int32_t": C.c_int32}

    def fields(struct):
        body = hdr[hdr.index(f"typedef struct {struct}"):hdr.index(f"}} {struct};")]
        return [(n, ctype[t]) for t, n in re.findall(r"^\s*(float\*|uint8_t\*|int64_t\*|int32_t)\s+(\w+);", body, flags=re.M)]

    ring = fields("urgym_replay_ring")
    assert ring == list(_abi.ReplayRing._fields_) and [n for n, _ in ring] == ["capacity_steps", "reserved0"] + list(RING_KEYS)
    assert C.sizeof(_abi.ReplayRing) == 8 + 11 * C.sizeof(C.c_void_p)
    batch = fields("urgym_replay_batch")
    assert batch == list(_abi.ReplayBatch._fields_) and [n for n, _ in batch] == list(RING_KEYS) + ["index"]
    assert [n for n, _, _, req in _abi.REPLAY_RING_FIELDS if not req] == ["truncated", "is_success"]
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    assert f"0x{_abi.REPLAY_TAG:08X}" in hdr and _abi.REPLAY_TAG & ~0xFF != _abi.NOISE_TAG and _abi.REPLAY_TAG > 4
    assert "handle_timeout_termination" in hdr  # the header says what `terminated` means and cites SB3
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
        assert re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym  # one line, starting with int
    assert lib.urgym_abi_version() == 4


def _words(seed, draw, count):
    w = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (np.arange(count, dtype=np.uint64), np.uint64(draw & 0xFFFFFFFF), np.uint64(draw >> 32),
                                                        np.uint64(0x52504C00)))
    return [(int(a) << 32) | int(b) for a, b in zip(w[0], w[1])]


def test_replay_indices():
    seed, draw = 0x0123456789ABCDEF, (7 << 32) | 5
    for size in (1, 2085, 1 << 20, 3 * (1 << 31) + 11, (1 << 40) + 12345, (1 << 62) + 3):  # not powers of two; beyond 2^32
        e = replay_indices(seed, draw, 300, size)
        assert e.dtype == np.int64 and e.shape == (300,) and e.min() >= 0 and e.max() < size
        # e = floor(w size / 2^64) in exact integers: e 2^64 <= w size < (e + 1) 2^64
        assert all((int(x) << 64) <= w * size < ((int(x) + 1) << 64) for x, w in zip(e, _words(seed, draw, 300))), size
        assert np.array_equal(replay_indices(seed, draw, 37, size), e[:37])  # independent of count
        if size > 1 << 32:
            assert e.max() > 1 << 32  # the high word takes part
    assert replay_indices(seed, draw, 0, 10).shape == (0,)
    # known answers, computed once with Python integers from Random123-checked Philox words (tests/test_policy_sampling.py)
    assert [int(v) for v in replay_indices(BUCKET_SEED, BUCKET_DRAW, 5, 2085)] == [1220, 1601, 1426, 450, 1489]
    base = replay_indices(seed, draw, 256, 1 << 40)
    assert len(set(base.tolist())) == 256  # changes with i
    for other in (replay_indices(seed ^ 1, draw, 256, 1 << 40), replay_indices(seed ^ (1 << 32), draw, 256, 1 << 40),
                  replay_indices(seed, draw + 1, 256, 1 << 40), replay_indices(seed, draw + (1 << 32), 256, 1 << 40)):
        assert (other != base).mean() > 0.99  # ... with either half of seed and of draw
    for bad in (dict(count=-1, size=5), dict(count=3, size=0), dict(count=3, size=1 << 63)):
        with pytest.raises(ValueError):
            replay_indices(1, 1, **bad)


def test_replay_indices_are_uniform():
    size = CAP * N
    e = replay_indices(BUCKET_SEED, BUCKET_DRAW, 65536, size)
    counts = np.bincount(e * 16 // size, minlength=16)
    print("bucket counts", counts.tolist())
    assert counts.shape == (16,) and counts.sum() == 65536
    assert np.all(np.abs(counts - 4096) <= 310), counts  # 5 standard deviations (module docstring)
    assert len(np.unique(e)) == size  # every entry of the ring is reachable


def test_check_args_needs_no_gpu():
    ok = DeviceReplay.check_args
    assert ok(5) == 5 and ok(5, num_steps=13, first_slot=4, filled_steps=5, oldest_slot=0, batch_size=1) == 5
    assert ok(1, num_steps=1, first_slot=0, filled_steps=1, oldest_slot=0, batch_size=256) == 1
    for bad in (dict(capacity_steps=0), dict(capacity_steps=-3), dict(capacity_steps=2.5), dict(capacity_steps=1 << 31),
                dict(capacity_steps=5, num_steps=0), dict(capacity_steps=5, num_steps=-1),
                dict(capacity_steps=5, first_slot=5), dict(capacity_steps=5, first_slot=-1),
                dict(capacity_steps=5, oldest_slot=5), dict(capacity_steps=5, oldest_slot=-1),
                dict(capacity_steps=5, filled_steps=0), dict(capacity_steps=5, filled_steps=6),
                dict(capacity_steps=5, batch_size=0), dict(capacity_steps=5, batch_size=-256)):
        with pytest.raises(ValueError):
            ok(**bad)


# ------------------------------------------------------------------------------------------------ GPU
def _ring_copy(replay):
    return {k: v.clone() for k, v in replay.ring.items()}


def _collected(name, splits=(K,), cap=CAP):
    """A fresh env and ring after collecting sum(splits) steps in len(splits) calls (first_draw advanced between them)."""
    env, actor = _make(name, N, ENV_SEED, max_episode_steps=STEP_LIMIT)
    replay = DeviceReplay(env, cap)
    done = 0
    for part in splits:
        replay.collect(actor, part, sample=dict(HOW, first_draw=HOW["first_draw"] + done))
        done += part
    return env, actor, replay


@functools.lru_cache(maxsize=None)
def python_stepped(name, n=N, num_steps=K, mode=HOW["mode"], step_limit=STEP_LIMIT):
    """The reference: a second env with the same seed stepped from Python, every transition assembled in torch from what step()
    returns (info['final_observation'], all three keys).  Returns (transitions of all steps, the env's final buffers)."""
    import torch

    env, actor = _make(name, n, ENV_SEED, max_episode_steps=step_limit)
    rows = ("observation", "achieved_goal", "desired_goal")
    steps = []
    for k in range(num_steps):
        t = {key: env.buf[key].clone() for key in rows}
        if mode == "mean":
            a = env.policy_actions(actor)  # urgym_actor_forward
        else:
            a, _ = env.policy_actions(actor, sample=dict(HOW, mode=mode, first_draw=HOW["first_draw"] + k))
        obs, rew, term, trunc, info = env.step(a)
        done = (term | trunc)[:, None]
        t["action"], t["reward"] = a.clone(), rew.clone()
        for key in rows:
            t["next_" + key] = torch.where(done, info["final_observation"][key], obs[key])
        t["terminated"], t["truncated"], t["is_success"] = term.view(torch.uint8).clone(), trunc.view(torch.uint8).clone(), info["is_success"].view(torch.uint8).clone()
        steps.append(t)
    torch.cuda.synchronize()
    final = {key: v.clone() for key, v in env.buf.items()}
    actor.close()
    env.close()
    return steps, final


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dyn", "obs"])
def test_collect_is_bitwise_a_python_stepped_loop(name):
    import torch

    steps, final = python_stepped(name)
    live = steps[K - CAP:]
    term = torch.stack([t["terminated"] for t in live]).bool()
    trunc = torch.stack([t["truncated"] for t in live]).bool()
    cases = (int(term.sum()), int((trunc & ~term).sum()), int((~term & ~trunc).sum()))
    print(f"{name}: live slots hold {cases[0]} terminated, {cases[1]} truncated-not-terminated, {cases[2]} unfinished rows")
    assert min(cases) > 0, cases  # on the Python-stepped side alone
    done = (term | trunc)
    moved = torch.stack([(t["next_desired_goal"] != steps[K - CAP + i + 1]["desired_goal"]).any(dim=1) for i, t in enumerate(live[:-1])])
    assert bool(moved[done[:-1]].any())  # a finished row's s' is NOT the next step's s: the terminal goals count
    env, actor, replay = _collected(name)
    torch.cuda.synchronize()
    assert replay.cursor == K % CAP and replay.filled == CAP and replay.oldest_slot == K % CAP and len(replay) == CAP * N
    for k in range(K - CAP, K):
        for key in RING_KEYS:
            assert _same_bits(replay.ring[key][k % CAP], steps[k][key]), (name, k, key)
    for key, want in final.items():  # and the environment is where the Python loop left its own
        if key not in ("done_list", "done_count"):
            assert _same_bits(env.buf[key], want), key
    actor.close()
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["mean", "gaussian", "uniform"])
def test_collect_in_every_mode_wraps_a_small_ring(mode):
    """65 envs (one more than a wave), 3 steps from slot 1 of a 2-slot ring: slots 1, 0, 1, so the first, a middle and the closing
    store pass all occur and the last step overwrites the first.  max_episode_steps = 2: every env is auto-reset at the second step.
    "mean" is the deterministic kernel (the reference takes its actions from urgym_actor_forward), "uniform" runs no forward pass."""
    import torch

    n, steps_k, cap = 65, 3, 2
    steps, final = python_stepped("dyn", n, steps_k, mode, 2)
    assert bool(torch.stack([t["truncated"] for t in steps]).any())  # on the Python-stepped side alone
    env, actor = _make("dyn", n, ENV_SEED, max_episode_steps=2)
    replay = DeviceReplay(env, cap)
    env.collect(actor, steps_k, replay, sample=None if mode == "mean" else dict(HOW, mode=mode), first_slot=1)
    torch.cuda.synchronize()
    for k, slot in ((1, 0), (2, 1)):
        for key in RING_KEYS:
            assert _same_bits(replay.ring[key][slot], steps[k][key]), (mode, k, key)
    for key, want in final.items():
        if key not in ("done_list", "done_count"):
            assert _same_bits(env.buf[key], want), key
    actor.close()
    env.close()


@pytest.mark.gpu
def test_collect_leaves_the_environment_where_the_recorded_rollout_does():
    env, actor, _ = _collected("dyn")
    other, other_actor = _make("dyn", N, ENV_SEED, max_episode_steps=STEP_LIMIT)
    other.rollout_policy(other_actor, K, record=("reward",), sample=HOW)
    _same_state(env, other)  # the bound buffers, q, step_count and episode_id included
    assert int(env.buf["episode_id"].max()) > 0  # envs were reset on the way
    for obj in (actor, other_actor, env, other):
        obj.close()


@pytest.mark.gpu
def test_split_calls_fill_the_same_ring():
    env, actor, whole = _collected("dyn")
    env2, actor2, parts = _collected("dyn", splits=(8, 5))
    assert (parts.cursor, parts.filled) == (whole.cursor, whole.filled)
    for key in RING_KEYS:
        assert _same_bits(parts.ring[key], whole.ring[key]), key
    _same_state(env, env2)
    for obj in (actor, actor2, env, env2):
        obj.close()


def _nan_ring(name, cap=8, first=6, steps=3):
    """A ring pre-filled with a NaN bit pattern (flags: 0xA5) that then collects `steps` steps from slot `first`."""
    import torch

    env, actor = _make(name, N, ENV_SEED, max_episode_steps=STEP_LIMIT)
    replay = DeviceReplay(env, cap)
    for t in replay.ring.values():
        if t.dtype == torch.float32:
            t.view(torch.int32).fill_(0x7FC00123)
        else:
            t.fill_(0xA5)
    before = _ring_copy(replay)
    replay.cursor = first
    replay.collect(actor, steps, sample=HOW)
    torch.cuda.synchronize()
    return env, actor, replay, before


@pytest.mark.gpu
def test_no_stray_writes():
    import torch

    env, actor, replay, before = _nan_ring("dyn")
    assert (replay.cursor, replay.filled, replay.oldest_slot) == (1, 3, 6)
    for key in RING_KEYS:
        t = replay.ring[key]
        for slot in (6, 7, 0):
            if t.dtype == torch.float32:
                assert bool(torch.isfinite(t[slot]).all()), (key, slot)
            else:
                assert bool((t[slot] <= 1).all()), (key, slot)
        assert _same_bits(t[1:6], before[key][1:6]), key  # untouched, bit for bit
    actor.close()
    env.close()


def _check_sample(replay, batch_size, seed, draw):
    import torch

    n, cap = replay.env.num_envs, replay.capacity
    got = replay.sample(batch_size, seed, draw)
    torch.cuda.synchronize()
    e = replay_indices(seed, draw, batch_size, replay.filled * n)
    want = ((replay.oldest_slot + e // n) % cap) * n + e % n
    index = got["index"].cpu().numpy()
    assert index.dtype == np.int64 and np.array_equal(index, want)
    idx = got["index"]
    flat = {"action": got["actions"], "reward": got["rewards"], "terminated": got["terminated"], "truncated": got["truncated"], "is_success": got["is_success"]}
    for key in ("observation", "achieved_goal", "desired_goal"):
        flat[key], flat["next_" + key] = got["observations"][key], got["next_observations"][key]
    assert set(flat) == set(RING_KEYS)
    for key in RING_KEYS:
        src = replay.ring[key]
        rows = src.reshape((cap * n,) + tuple(src.shape[2:]))[idx]
        assert _same_bits(flat[key].view(src.dtype), rows), key
    return got, flat


@pytest.mark.gpu
@pytest.mark.parametrize("state", ["partly_filled", "wrapped"])
def test_sample(state):
    import torch

    if state == "partly_filled":  # 3 of 8 slots, slots 6, 7, 0: the other five hold NaN patterns and must never be drawn
        env, actor, replay, _ = _nan_ring("dyn")
        valid = {6, 7, 0}
    else:  # full, oldest_slot = 3
        env, actor, replay = _collected("dyn")
        assert replay.oldest_slot == 3
        valid = set(range(CAP))
    for batch_size in (1, 256, 417):
        got, flat = _check_sample(replay, batch_size, seed=77, draw=(1 << 32) + batch_size)
        assert set((got["index"] // N).cpu().tolist()) <= valid
        assert all(bool(torch.isfinite(v).all()) for v in flat.values() if v.dtype == torch.float32)
    # only some outputs requested: those are written, and equal the full batch's
    some = {"reward": torch.full((417,), float("nan"), device=env.device), "next_desired_goal": torch.full((417, env.goal_dim), float("nan"), device=env.device),
            "index": torch.full((417,), -1, dtype=torch.int64, device=env.device)}
    replay.sample_into(some, 77, (1 << 32) + 417)
    torch.cuda.synchronize()
    assert _same_bits(some["reward"], flat["reward"]) and _same_bits(some["next_desired_goal"], flat["next_desired_goal"]) and _same_bits(some["index"], got["index"])
    only = {"index": torch.full((5,), -1, dtype=torch.int64, device=env.device)}
    replay.sample_into(only, 77, (1 << 32) + 417)
    assert _same_bits(only["index"], got["index"][:5])  # and a prefix of a longer draw is the shorter draw
    actor.close()
    env.close()


@pytest.mark.gpu
def test_sample_targets():
    import torch

    name = "dyn"
    env, actor, replay = _collected(name)
    critic = DeviceCritic.load(critic_paths(name), env)
    gamma, alpha = hyper(name)
    seed, draw, B = 11, 5, 256
    got = replay.sample_targets(actor, critic, B, seed, draw, gamma, alpha)
    batch = replay.sample(B, seed, draw)
    nxt = batch["next_observations"]
    a2, lp2 = env.policy_actions(actor, sample=dict(mode="gaussian", seed=seed, first_draw=draw), rows=nxt)
    by_hand = env.critic_values(critic, a2, rows=nxt, reward=batch["rewards"], terminated=batch["terminated"], log_prob=lp2, gamma=gamma, ent_coef=alpha)
    torch.cuda.synchronize()
    assert _same_bits(got["index"], batch["index"]) and _same_bits(got["next_actions"], a2) and _same_bits(got["next_log_prob"], lp2)
    assert got["target"].shape == (B,) and _same_bits(got["target"], by_hand["target"])
    q = by_hand["q"].cpu().numpy()
    term = batch["terminated"].cpu().numpy()
    _, t32 = TwinCritic.target(q[0], q[1], batch["rewards"].cpu().numpy(), gamma, term, lp2.cpu().numpy(), alpha)
    assert np.array_equal(t32.view(np.uint32), got["target"].cpu().numpy().view(np.uint32))
    # the ring's `terminated` is the env's own flag: a truncated-not-terminated row is bootstrapped through
    rows = batch["truncated"].cpu().numpy() & ~term
    assert rows.any() and term.any()
    assert np.all(t32[term] == batch["rewards"].cpu().numpy()[term]) and np.any(t32[rows] != batch["rewards"].cpu().numpy()[rows])
    for obj in (critic, actor, env):
        obj.close()


@pytest.mark.gpu
def test_refusals_leave_the_handle_usable():
    import torch

    env, actor, replay = _collected("dyn")
    first = replay.sample(256, 9, 1)
    lib, h, s = env.lib, env._h, env._stream()
    how = _abi.Sampling(_abi.SAMPLE_GAUSSIAN, 0, 29, 500)

    def ring(**kw):
        r = _abi.ReplayRing.from_buffer_copy(replay._ring)
        for key, v in kw.items():
            setattr(r, key, v)
        return r

    def refused(rc, call):
        msg = lib.urgym_last_error(h).decode()
        assert rc == _abi.ERR_ARG and call in msg, (rc, msg)

    col, who = lib.urgym_rollout_collect, "urgym_rollout_collect"
    good = ring()
    refused(col(h, actor._a, C.byref(how), 3, None, 0, s), who)
    for key in RING_KEYS[:9]:  # every required pointer
        refused(col(h, actor._a, C.byref(how), 3, C.byref(ring(**{key: None})), 0, s), who)
    refused(col(h, actor._a, C.byref(how), 3, C.byref(ring(capacity_steps=0)), 0, s), who)
    refused(col(h, actor._a, C.byref(how), 3, C.byref(ring(capacity_steps=-5)), 0, s), who)
    refused(col(h, actor._a, C.byref(how), 3, C.byref(ring(reserved0=1)), 0, s), who)
    refused(col(h, actor._a, C.byref(how), 3, C.byref(good), CAP, s), who)
    refused(col(h, actor._a, C.byref(how), 3, C.byref(good), -1, s), who)
    refused(col(h, actor._a, C.byref(how), 0, C.byref(good), 0, s), who)
    refused(col(h, actor._a, C.byref(how), -2, C.byref(good), 0, s), who)
    # urgym_rollout_sampled's own refusals
    refused(col(h, None, C.byref(how), 3, C.byref(good), 0, s), who)
    refused(col(h, actor._a, None, 3, C.byref(good), 0, s), who)
    refused(col(h, actor._a, C.byref(_abi.Sampling(7, 0, 0, 0)), 3, C.byref(good), 0, s), who)
    refused(col(h, actor._a, C.byref(_abi.Sampling(_abi.SAMPLE_GAUSSIAN, 1, 0, 0)), 3, C.byref(good), 0, s), who)

    smp, who = lib.urgym_replay_sample, "urgym_replay_sample"
    index = torch.empty((256,), dtype=torch.int64, device=env.device)
    flag = torch.empty((256,), dtype=torch.uint8, device=env.device)
    out = _abi.ReplayBatch(index=C.cast(index.data_ptr(), C.POINTER(C.c_int64)))
    refused(smp(h, None, 0, CAP, 9, 1, 256, C.byref(out), s), who)
    refused(smp(h, C.byref(ring(reward=None)), 0, CAP, 9, 1, 256, C.byref(out), s), who)
    refused(smp(h, C.byref(ring(capacity_steps=0)), 0, 1, 9, 1, 256, C.byref(out), s), who)
    refused(smp(h, C.byref(ring(reserved0=2)), 0, CAP, 9, 1, 256, C.byref(out), s), who)
    refused(smp(h, C.byref(good), 0, 0, 9, 1, 256, C.byref(out), s), who)
    refused(smp(h, C.byref(good), 0, CAP + 1, 9, 1, 256, C.byref(out), s), who)
    refused(smp(h, C.byref(good), CAP, CAP, 9, 1, 256, C.byref(out), s), who)
    refused(smp(h, C.byref(good), -1, CAP, 9, 1, 256, C.byref(out), s), who)
    refused(smp(h, C.byref(good), 0, CAP, 9, 1, 0, C.byref(out), s), who)
    refused(smp(h, C.byref(good), 0, CAP, 9, 1, -4, C.byref(out), s), who)
    refused(smp(h, C.byref(good), 0, CAP, 9, 1, 256, None, s), who)
    refused(smp(h, C.byref(good), 0, CAP, 9, 1, 256, C.byref(_abi.ReplayBatch()), s), who)
    flags = _abi.ReplayBatch(truncated=C.cast(flag.data_ptr(), C.POINTER(C.c_uint8)))
    refused(smp(h, C.byref(ring(truncated=None)), 0, CAP, 9, 1, 256, C.byref(flags), s), who)
    with pytest.raises(ValueError):
        env.collect(actor, 0, replay)
    with pytest.raises(ValueError):
        env.collect(actor, 3, object())
    with pytest.raises(ValueError):
        DeviceReplay(env, 2).sample(4, 0, 0)  # nothing collected yet
    # the handle is as usable as before: nothing above touched the ring or the env
    again = replay.sample(256, 9, 1)
    for key in ("actions", "rewards", "index"):
        assert _same_bits(again[key], first[key]), key
    assert smp(h, C.byref(ring(truncated=None, is_success=None)), replay.oldest_slot, CAP, 9, 1, 256, C.byref(out), s) == 0  # the optional two
    torch.cuda.synchronize()
    assert _same_bits(index, first["index"])
    env2, actor2, more = _collected("dyn", splits=(K, 3))
    replay.collect(actor, 3, sample=dict(HOW, first_draw=HOW["first_draw"] + K))
    for key in RING_KEYS:
        assert _same_bits(replay.ring[key], more.ring[key]), key
    for obj in (actor, actor2, env, env2):
        obj.close()
