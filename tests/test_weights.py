"""GPU tests (-m gpu) of the weight reload from device tensors: urgym_actor_load / urgym_critic_load through
DeviceActor.load_parameters / DeviceCritic.load_parameters, read back with packed().

The yardstick is the host route that existed before: an object CREATED from the same weights (the host packing loops, then a copy).
A load must leave the whole packed buffer, padding included, word for word what such an object holds; everything that follows from
the buffer (forward passes, samples, Q-values, targets) is then bitwise equal too, which the behaviour tests check on their own.
The blend is checked against evaluation.polyak, the numpy float32 restatement with three separately rounded operations.

N = 161 envs: one full workgroup of the forward kernels and one ragged one.  The packing itself does not depend on N.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from ur_gym_amd import _abi, _native, make_vec
from ur_gym_amd.evaluation import ACTOR_ARRAYS, CRITIC_ARRAYS, LOG_STD_ARRAYS, DeviceActor, DeviceCritic, DeviceReplay, polyak

pytestmark = pytest.mark.gpu

N = 161
KINDS = {"ori": "UR5OriReach-v1", "obs": "UR5ObsReach-v1", "sta": "UR5StaReach-v1", "dyn": "UR5DynReach-v1"}
ACTOR_IN = {"ori": 30, "obs": 32, "sta": 41, "dyn": 47}
WIDTHS = (32, 160, 256, 288, 512)
GRID = [(k, H) for k in KINDS for H in WIDTHS]


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(words(a), words(b))


def actor_weights(kind, H, seed, head=True):
    rng = np.random.default_rng(seed)
    n = ACTOR_IN[kind]
    shapes = dict(zip(ACTOR_ARRAYS + LOG_STD_ARRAYS, ((H, n), (H,), (H, H), (H,), (6, H), (6,), (6, H), (6,))))
    scale = dict(zip(ACTOR_ARRAYS + LOG_STD_ARRAYS, (n ** -0.5, 0.1, H ** -0.5, 0.1, H ** -0.5, 0.1, 0.1 * H ** -0.5, 0.1)))
    keys = ACTOR_ARRAYS + (LOG_STD_ARRAYS if head else ())
    return {k: (rng.standard_normal(shapes[k]) * scale[k]).astype(np.float32) for k in keys}


def critic_weights(kind, H, seed):
    rng = np.random.default_rng(1000 + seed)
    n = ACTOR_IN[kind] + 6
    shapes = dict(zip(CRITIC_ARRAYS, ((H, n), (H,), (H, H), (H,), (1, H), (1,))))
    scale = dict(zip(CRITIC_ARRAYS, (n ** -0.5, 0.1, H ** -0.5, 0.1, H ** -0.5, 0.1)))
    return [{k: (rng.standard_normal(sh) * scale[k]).astype(np.float32) for k, sh in shapes.items()} for _ in range(2)]


def on_device(w, env, offset=0):
    """Device tensors of a weight dict (or list of dicts).  offset = 1: every tensor is a view that starts one float into a larger
    allocation, so its address is 4 bytes past a 16-byte boundary."""
    if isinstance(w, list):
        return [on_device(x, env, offset) for x in w]
    out = {}
    for k, v in w.items():
        flat = torch.empty(v.size + offset, dtype=torch.float32, device=env.device)
        flat[offset:] = torch.from_numpy(v.reshape(-1)).to(env.device)
        out[k] = flat[offset:].view(v.shape)
        assert out[k].is_contiguous() and (offset == 0 or out[k].data_ptr() % 16 == 4)
    return out


@pytest.fixture(scope="module")
def envs():
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = make_vec(KINDS[kind], num_envs=N, seed=3, auto_reset=True)
            made[kind].reset(seed=3)
        return made[kind]

    yield get
    for e in made.values():
        e.close()


# ------------------------------------------------------------------------------------------------ bitwise pack
@pytest.mark.parametrize("kind,H", GRID)
def test_actor_load_equals_a_fresh_actor(envs, kind, H):
    env = envs(kind)
    a, b = actor_weights(kind, H, 1), actor_weights(kind, H, 2)
    A, fresh_b = DeviceActor(a, env), DeviceActor(b, env)
    first, want = A.packed(), fresh_b.packed()
    assert first.size == (H + 127) // 128 * 128 // 32 * (6 * 256 + (H + 127) // 128 * 128 // 32 * 4 * 256) + 14 * ((H + 127) // 128 * 128) + 16
    A.load_parameters(on_device(b, env, offset=1))
    assert same(A.packed(), want)  # the whole buffer, padding included
    A.load_parameters(on_device(a, env))
    assert same(A.packed(), first)
    A.close(), fresh_b.close()


@pytest.mark.parametrize("kind,H", GRID)
def test_critic_load_equals_a_fresh_critic(envs, kind, H):
    env = envs(kind)
    a, b = critic_weights(kind, H, 1), critic_weights(kind, H, 2)
    A, fresh_b = DeviceCritic(a, env), DeviceCritic(b, env)
    first, want = A.packed(), fresh_b.packed()
    A.load_parameters(on_device(b, env, offset=1))
    assert same(A.packed(), want)
    A.load_parameters(on_device(a, env), tau=1.0)
    assert same(A.packed(), first)
    A.close(), fresh_b.close()


# ------------------------------------------------------------------------------------------------ the log_std head
def test_log_std_head_semantics(envs):
    env, kind, H = envs("dyn"), "dyn", 160
    a, b = actor_weights(kind, H, 1), actor_weights(kind, H, 2)
    body_b = {k: b[k] for k in ACTOR_ARRAYS}
    how = dict(mode="gaussian", seed=1, first_draw=0)

    # an actor without head refuses GAUSSIAN; a load without head changes nothing about that; a load with head makes it sample
    bare = DeviceActor({k: a[k] for k in ACTOR_ARRAYS}, env)
    assert not bare.has_log_std
    with pytest.raises(_native.NativeError, match="log_std"):
        env.policy_actions(bare, sample=how)
    bare.load_parameters(on_device(body_b, env))
    assert not bare.has_log_std
    with pytest.raises(_native.NativeError, match="log_std"):
        env.policy_actions(bare, sample=how)
    bare.load_parameters(on_device(b, env))
    assert bare.has_log_std
    got = env.policy_actions(bare, sample=how)
    fresh_b = DeviceActor(b, env)  # create + set_log_std on the host
    want = env.policy_actions(fresh_b, sample=how)
    assert same(bare.packed(), fresh_b.packed())
    assert same(got[0].cpu().numpy(), want[0].cpu().numpy()) and same(got[1].cpu().numpy(), want[1].cpu().numpy())

    # loading without the head leaves a previously set head's words as they were: body of b, head of a
    A = DeviceActor(a, env)
    A.load_parameters(on_device(body_b, env, offset=1))
    mixed = DeviceActor(dict(body_b, **{k: a[k] for k in LOG_STD_ARRAYS}), env)
    assert A.has_log_std and same(A.packed(), mixed.packed())
    for x in (bare, fresh_b, A, mixed):
        x.close()


# ------------------------------------------------------------------------------------------------ behaviour
@pytest.mark.parametrize("H", (32, 256))
def test_reloaded_objects_behave_like_fresh_ones(envs, H):
    env, kind = envs("dyn"), "dyn"
    a, b = actor_weights(kind, H, 1), actor_weights(kind, H, 2)
    ca, cb = critic_weights(kind, H, 1), critic_weights(kind, H, 2)
    actor, fresh = DeviceActor(a, env), DeviceActor(b, env)
    critic, fresh_c = DeviceCritic(ca, env), DeviceCritic(cb, env)
    actor.load_parameters(on_device(b, env, offset=1))
    critic.load_parameters(on_device(cb, env, offset=1))
    how = dict(mode="gaussian", seed=7, first_draw=3)
    np_ = lambda t: t.cpu().numpy()  # noqa: E731
    assert same(np_(env.policy_actions(actor)), np_(env.policy_actions(fresh)))
    (act, lp), (act_f, lp_f) = env.policy_actions(actor, sample=how), env.policy_actions(fresh, sample=how)
    assert same(np_(act), np_(act_f)) and same(np_(lp), np_(lp_f))
    kw = dict(reward=env.buf["reward"], terminated=env.buf["terminated"], log_prob=lp, gamma=0.95, ent_coef=0.3)
    got, want = env.critic_values(critic, act, **kw), env.critic_values(fresh_c, act, **kw)
    for k in ("q", "q_min", "target"):
        assert same(np_(got[k]), np_(want[k])), k
    assert np.isfinite(np_(got["q"])).all() and np.ptp(np_(got["q"])) > 0
    for x in (actor, fresh, critic, fresh_c):
        x.close()


def test_stream_order(envs):
    """forward -> load -> forward without a host synchronisation: the first sees the old weights, the second the new."""
    env, kind, H = envs("dyn"), "dyn", 256
    a, b = actor_weights(kind, H, 1), actor_weights(kind, H, 2)
    A, B, live = DeviceActor(a, env), DeviceActor(b, env), DeviceActor(a, env)
    tb = on_device(b, env)
    X = torch.zeros((N, 6), dtype=torch.float32, device=env.device)
    Y = torch.zeros_like(X)
    torch.cuda.synchronize(env.device)
    env.policy_actions(live, out=X)
    live.load_parameters(tb)
    env.policy_actions(live, out=Y)
    want_x, want_y = env.policy_actions(A), env.policy_actions(B)
    torch.cuda.synchronize(env.device)
    assert same(X.cpu().numpy(), want_x.cpu().numpy()) and same(Y.cpu().numpy(), want_y.cpu().numpy())
    assert not same(X.cpu().numpy(), Y.cpu().numpy())
    for x in (A, B, live):
        x.close()


# ------------------------------------------------------------------------------------------------ Polyak
@pytest.mark.parametrize("H", (32, 256))
def test_polyak_recursion_is_bitwise(envs, H):
    env, kind, tau = envs("dyn"), "dyn", 0.005
    start = critic_weights(kind, H, 0)
    target = DeviceCritic(start, env)
    want = target.packed()
    zero_words = words(want) == 0
    for i in (1, 2, 3):
        src = critic_weights(kind, H, i)
        fresh = DeviceCritic(src, env)
        want = polyak(want, fresh.packed(), tau)
        fresh.close()
        target.load_parameters(on_device(src, env, offset=i % 2), tau=tau)
    got = target.packed()
    assert same(got, want)
    # padding stays +0 (where the start is +0 and is no weight: a weight is +0 with probability 0)
    assert np.all(words(got)[zero_words] == 0) and zero_words.sum() >= 4 * 3

    # tau = 1 repairs a buffer that holds NaN (NaN-filled tensors are legitimate input)
    nan = [{k: np.full_like(v, np.nan) for k, v in net.items()} for net in start]
    target.load_parameters(on_device(nan, env), tau=1.0)
    held = target.packed()
    assert np.isnan(held).sum() == sum(v.size for net in start for v in net.values())
    target.load_parameters(on_device(start, env), tau=tau)  # blending cannot repair it ...
    assert np.isnan(target.packed()).sum() == np.isnan(held).sum()
    target.load_parameters(on_device(start, env), tau=1.0)  # ... replacing does
    fresh = DeviceCritic(start, env)
    assert same(target.packed(), fresh.packed())
    fresh.close(), target.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_everything_as_it_was(envs):
    env, other, kind, H = envs("dyn"), envs("sta"), "dyn", 64
    lib = env.lib
    aw, cw = actor_weights(kind, H, 1), critic_weights(kind, H, 1)
    actor, critic = DeviceActor(aw, env), DeviceCritic(cw, env)
    stranger_a, stranger_c = DeviceActor(actor_weights("sta", H, 1), other), DeviceCritic(critic_weights("sta", H, 1), other)
    ta, tc = on_device(actor_weights(kind, H, 2), env), on_device(critic_weights(kind, H, 2), env)
    before_a, before_c = actor.packed(), critic.packed()
    fp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float))  # noqa: E731
    stream = env._stream()

    def actor_params(**over):
        p = _abi.ActorParamsDev(47, H, 0, *[fp(ta[k]) for k in ACTOR_ARRAYS + LOG_STD_ARRAYS])
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def critic_params(**over):
        p = _abi.CriticParamsDev(53, H, 0)
        for i in (0, 1):
            p.qf[i] = _abi.QNetworkDev(*[fp(tc[i][k]) for k in CRITIC_ARRAYS])
        for k, v in over.items():
            if k.startswith("qf1_"):
                setattr(p.qf[1], k[4:], v)
            else:
                setattr(p, k, v)
        return p

    null = C.POINTER(C.c_float)()
    refused = []
    call_a = lambda h, a, p: lib.urgym_actor_load(h, a, C.byref(p) if p is not None else None, stream)  # noqa: E731
    call_c = lambda h, c, p, tau=1.0: lib.urgym_critic_load(h, c, C.byref(p) if p is not None else None, tau, stream)  # noqa: E731
    refused.append(call_a(None, actor._a, actor_params()))
    refused.append(call_a(env._h, None, actor_params()))
    refused.append(call_a(env._h, actor._a, None))
    refused.append(call_a(env._h, stranger_a._a, actor_params()))  # an actor of another handle
    refused.append(call_a(other._h, actor._a, actor_params()))
    for name in _abi.ACTOR_DEV_ARRAYS[:6]:
        refused.append(call_a(env._h, actor._a, actor_params(**{name: null})))
    refused.append(call_a(env._h, actor._a, actor_params(w_log_std=null)))  # only one of the two
    refused.append(call_a(env._h, actor._a, actor_params(b_log_std=null)))
    refused.append(call_a(env._h, actor._a, actor_params(in_features=41)))
    refused.append(call_a(env._h, actor._a, actor_params(hidden_width=H + 32)))
    refused.append(call_a(env._h, actor._a, actor_params(reserved0=1)))
    n_actor = len(refused)
    refused.append(call_c(None, critic._c, critic_params()))
    refused.append(call_c(env._h, None, critic_params()))
    refused.append(call_c(env._h, critic._c, None))
    refused.append(call_c(env._h, stranger_c._c, critic_params()))
    refused.append(call_c(other._h, critic._c, critic_params()))
    for name in ("w0", "b0", "w1", "b1", "w_q", "b_q"):
        refused.append(call_c(env._h, critic._c, critic_params(**{"qf1_" + name: null})))
    refused.append(call_c(env._h, critic._c, critic_params(in_features=47)))
    refused.append(call_c(env._h, critic._c, critic_params(hidden_width=H + 32)))
    refused.append(call_c(env._h, critic._c, critic_params(reserved0=1)))
    for tau in (0.0, -0.005, 1.0000001, float("nan"), float("inf"), float("-inf")):
        refused.append(call_c(env._h, critic._c, critic_params(), tau))
    assert refused == [_abi.ERR_ARG] * len(refused) and n_actor == 16 and len(refused) == 16 + 20
    assert b"tau" in lib.urgym_last_error(env._h)
    # read_packed: too small a buffer, a stranger, no count
    count, small = C.c_uint64(), np.empty(8, np.float32)
    assert lib.urgym_actor_read_packed(env._h, actor._a, C.c_void_p(small.ctypes.data), 8, C.byref(count)) == _abi.ERR_ARG
    assert count.value == before_a.size
    assert lib.urgym_critic_read_packed(env._h, stranger_c._c, None, 0, C.byref(count)) == _abi.ERR_ARG
    assert lib.urgym_critic_read_packed(env._h, critic._c, None, 0, None) == _abi.ERR_ARG
    # the Python layer refuses before the library is asked
    with pytest.raises(ValueError, match="tau"):
        critic.load_parameters(tc, tau=0.0)
    with pytest.raises(ValueError, match="is on cpu"):
        actor.load_parameters({k: v.cpu() for k, v in ta.items()})

    # nothing was launched, and everything still works
    assert same(actor.packed(), before_a) and same(critic.packed(), before_c)
    fresh = DeviceActor(aw, env)
    assert same(env.policy_actions(actor).cpu().numpy(), env.policy_actions(fresh).cpu().numpy())
    actor.load_parameters(ta)
    critic.load_parameters(tc, tau=0.5)
    assert not same(actor.packed(), before_a) and same(critic.packed(), polyak(before_c, DeviceCritic(critic_weights(kind, H, 2), env).packed(), 0.5))
    for x in (actor, critic, stranger_a, stranger_c, fresh):
        x.close()


# ------------------------------------------------------------------------------------------------ the learner
def test_learner_mechanics():
    """collect(8), then three updates: after each, the device actor holds the torch actor's current parameters and the device
    target the Polyak recursion over the torch critic's parameters after each step.  No learning curve is asserted."""
    from ur_gym_amd.training import SACLearner, host_arrays

    env = make_vec("UR5OriReach-v1", num_envs=64, seed=5, auto_reset=True)
    env.reset(seed=5)
    learner = SACLearner(env, seed=5, hidden_width=64, batch_size=64)
    tau = learner.hp["tau"]
    replay = DeviceReplay(env, 8)

    def host_packed(cls, arrays):
        obj = cls(arrays, env)
        out = obj.packed()
        obj.close()
        return out

    want_target = host_packed(DeviceCritic, host_arrays(learner.critic.tensors()))
    assert same(learner.target.packed(), want_target)
    learner.collect(replay, 8)
    assert replay.filled == 8 and learner.env_steps == 8
    before = host_arrays(learner.actor.tensors())
    for i in range(3):
        losses = learner.update(replay, seed=11, draw=i)
        assert same(learner.device_actor.packed(), host_packed(DeviceActor, host_arrays(learner.actor.tensors())))
        want_target = polyak(want_target, host_packed(DeviceCritic, host_arrays(learner.critic.tensors())), tau)
        assert same(learner.target.packed(), want_target)
        assert all(np.isfinite(v.item()) for v in losses.values())
    after = host_arrays(learner.actor.tensors())
    assert any(not np.array_equal(before[k], after[k]) for k in before)  # the optimiser moved the actor, so the loads had work to do
    learner.collect(replay, 2)  # past learning_starts (8 x 64 env steps >= 100): the sampled policy, on the reloaded actor
    torch.cuda.synchronize(env.device)  # raises if any launch of update / collect left an error
    assert np.isfinite(replay.ring["action"].cpu().numpy()).all()
    learner.close()
    env.close()
