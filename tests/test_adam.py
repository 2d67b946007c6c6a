"""GPU tests (-m gpu) of the Adam step that repacks: urgym_actor_adam_step / urgym_critic_adam_step.

After every call the stepped tensors equal evaluation.adam_step with the library's coefficients on every float, and the packed buffers
equal those of fresh objects created from the stepped parameters on the host (the target: evaluation.polyak of them).  N = 161 envs,
the packing does not depend on N.  Tensors are handed over as views one float into larger allocations, with guard words around each.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from adam_cases import HYPER, STEPS, p_bound, same, wide_gradients, words
from ur_gym_amd import _abi, make_vec
from ur_gym_amd.evaluation import ACTOR_ARRAYS, CRITIC_ARRAYS, LOG_STD_ARRAYS, DeviceActor, DeviceCritic, DeviceReplay, adam_coefficients, adam_step, polyak

pytestmark = pytest.mark.gpu

N = 161
KINDS = {"ori": "UR5OriReach-v1", "sta": "UR5StaReach-v1", "dyn": "UR5DynReach-v1"}
ACTOR_IN = {"ori": 30, "sta": 41, "dyn": 47}
GRID = [(k, H) for k in ("ori", "dyn") for H in (32, 160, 256)] + [("dyn", 512)]
ACTOR_KEYS = ACTOR_ARRAYS + LOG_STD_ARRAYS
GUARD, GUARD_WORD = 4, 0x7FC0ADA0  # floats of guard on either side of a tensor (after the one-float offset), and what they hold


def actor_shapes(kind, H):
    n = ACTOR_IN[kind]
    return dict(zip(ACTOR_KEYS, ((H, n), (H,), (H, H), (H,), (6, H), (6,), (6, H), (6,))))


def critic_shapes(kind, H):
    return dict(zip(CRITIC_ARRAYS, ((H, ACTOR_IN[kind] + 6), (H,), (H, H), (H,), (1, H), (1,))))


def draw(shapes, fn):
    return {k: fn(sh) for k, sh in shapes.items()}


class Guarded:
    """Device tensors of a dict of host arrays: each a contiguous view that starts GUARD + 1 floats into its own allocation (4 bytes
    past a 16-byte boundary) and ends GUARD floats before its end; the rest holds GUARD_WORD."""

    def __init__(self, host, device):
        self.flat, self.t = {}, {}
        for k, a in host.items():
            flat = torch.full((a.size + 2 * GUARD + 1,), GUARD_WORD, dtype=torch.int32, device=device).view(torch.float32)
            view = flat[GUARD + 1:GUARD + 1 + a.size]
            view.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1)))
            self.flat[k], self.t[k] = flat, view.view(a.shape)
            assert self.t[k].is_contiguous() and self.t[k].data_ptr() % 16 == 4

    def host(self):
        return {k: t.cpu().numpy() for k, t in self.t.items()}

    def guards_intact(self):
        for k, flat in self.flat.items():
            w = flat.view(torch.int32).cpu().numpy()
            n = self.t[k].numel()
            if not (np.all(w[:GUARD + 1] == GUARD_WORD) and np.all(w[GUARD + 1 + n:] == GUARD_WORD)):
                return False
        return True


class Sets:
    """The four tensor sets of one network (the critic: a list of two) on the device, and their host mirror stepped by adam_step."""

    def __init__(self, shapes, rng, device, nets=None):
        self.nets = nets
        count = nets or 1
        normal = lambda sh: rng.standard_normal(sh).astype(np.float32)  # noqa: E731
        zeros = lambda sh: np.zeros(sh, np.float32)  # noqa: E731
        self.host = {name: [draw(shapes, fn) for _ in range(count)] for name, fn in (("param", normal), ("grad", zeros), ("exp_avg", zeros), ("exp_avg_sq", zeros))}
        self.dev = {name: [Guarded(w, device) for w in ws] for name, ws in self.host.items()}
        self.shapes, self.rng = shapes, rng

    def args(self):
        """(params, grads, exp_avg, exp_avg_sq) as the env methods take them."""
        pick = (lambda gs: [g.t for g in gs]) if self.nets else (lambda gs: gs[0].t)
        return tuple(pick(self.dev[name]) for name in _abi.ADAM_SETS)

    def params(self):
        return self.host["param"] if self.nets else self.host["param"][0]

    def new_gradients(self, make=wide_gradients):
        for i, w in enumerate(self.host["grad"]):
            for k, sh in self.shapes.items():
                w[k] = make(self.rng, sh)
                self.dev["grad"][i].t[k].copy_(torch.from_numpy(w[k]))

    def step_host(self, coef):
        h = self.host
        for i in range(len(h["param"])):
            for k in self.shapes:
                h["param"][i][k], h["exp_avg"][i][k], h["exp_avg_sq"][i][k] = adam_step(h["param"][i][k], h["grad"][i][k], h["exp_avg"][i][k], h["exp_avg_sq"][i][k], coef)

    def differences(self, nan_ok=False):
        """(set, net, key) of every tensor whose device words differ from the host mirror's, and whether all guards are intact.
        nan_ok: where both hold a NaN the words are not compared (the payload of a propagated NaN is not part of the contract)."""
        def equal(got, want):
            both = np.isnan(got) & np.isnan(want) if nan_ok else np.zeros(got.shape, bool)
            return got.shape == want.shape and np.array_equal(words(got)[~both], words(want)[~both])

        bad = [(name, i, k) for name, ws in self.host.items() for i, w in enumerate(ws) for k, got in self.dev[name][i].host().items() if not equal(got, w[k])]
        return bad, all(g.guards_intact() for gs in self.dev.values() for g in gs)


def fresh_packed(cls, weights, env):
    obj = cls(weights, env)
    out = obj.packed()
    obj.close()
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


# ------------------------------------------------------------------------------------------------ bitwise
@pytest.mark.parametrize("kind,H", GRID)
def test_actor_step_is_adam_step_and_a_fresh_pack(envs, kind, H):
    env = envs(kind)
    s = Sets(actor_shapes(kind, H), np.random.default_rng(100 + H), env.device)
    actor = DeviceActor({k: np.zeros_like(v) for k, v in s.params().items() if k in ACTOR_ARRAYS}, env)  # no head yet: the step gives it one
    assert not actor.has_log_std
    for step in STEPS:
        s.new_gradients()
        env.actor_adam_step(actor, *s.args(), step=step, **HYPER)
        s.step_host(adam_coefficients(env, step=step, **HYPER))
        bad, guards = s.differences()
        assert not bad and guards, (step, bad, guards)
        assert same(actor.packed(), fresh_packed(DeviceActor, s.params(), env)), step
    assert actor.has_log_std
    env.policy_actions(actor, sample=dict(mode="gaussian", seed=1, first_draw=0))  # accepted: the actor has a head now
    torch.cuda.synchronize(env.device)
    actor.close()


@pytest.mark.parametrize("kind,H", GRID)
def test_critic_step_is_adam_step_a_fresh_pack_and_polyak(envs, kind, H):
    env = envs(kind)
    s = Sets(critic_shapes(kind, H), np.random.default_rng(200 + H), env.device, nets=2)
    start = [{k: np.zeros_like(v) for k, v in w.items()} for w in s.params()]
    online = DeviceCritic(start, env)
    target = DeviceCritic([{k: (0.5 * v).astype(np.float32) for k, v in w.items()} for w in s.params()], env)
    want_target = target.packed()
    zero_words = words(online.packed()) == 0  # everything is +0 in an all-zero critic: padding is where fresh packs stay +0
    for step in STEPS:
        tau = 1.0 if step == STEPS[-1] else 0.005
        s.new_gradients()
        env.critic_adam_step(online, *s.args(), step=step, target=target, tau=tau, **HYPER)
        s.step_host(adam_coefficients(env, step=step, **HYPER))
        bad, guards = s.differences()
        assert not bad and guards, (step, bad, guards)
        fresh = fresh_packed(DeviceCritic, s.params(), env)
        assert same(online.packed(), fresh), step
        want_target = polyak(want_target, fresh, tau)
        assert same(target.packed(), want_target), (step, tau)
        padding = zero_words & (words(fresh) == 0)
        assert padding.sum() >= 4 * 3 and np.all(words(target.packed())[padding] == 0)  # padding stays +0
    assert same(target.packed(), online.packed())  # the last call was tau = 1
    # without a target, tau is ignored and the target keeps what it held
    s.new_gradients()
    env.critic_adam_step(online, *s.args(), step=7, **HYPER)
    s.step_host(adam_coefficients(env, step=7, **HYPER))
    bad, guards = s.differences()
    assert not bad and guards and same(online.packed(), fresh_packed(DeviceCritic, s.params(), env)) and same(target.packed(), want_target)
    online.close(), target.close()


# ------------------------------------------------------------------------------------------------ independence, determinism
def nan_like(weights):
    return {k: np.full_like(v, np.nan) for k, v in weights.items()}


def on_device(w, env):
    if isinstance(w, list):
        return [on_device(x, env) for x in w]
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(env.device) for k, v in w.items()}


def test_a_nan_gradient_touches_its_own_element_only_and_a_nan_buffer_does_not_matter(envs):
    env, kind, H = envs("dyn"), "dyn", 32
    step = 2
    coef = adam_coefficients(env, step=step, **HYPER)

    # ---- actor
    packed, states = [], []
    for poison in (False, True):
        s = Sets(actor_shapes(kind, H), np.random.default_rng(5), env.device)
        actor = DeviceActor(s.params(), env)
        actor.load_parameters(on_device(nan_like(s.params()), env))  # the buffer holds NaN before the call (but for padding)
        assert np.isnan(actor.packed()).sum() == sum(v.size for v in s.params().values())
        s.new_gradients()
        if poison:
            s.host["grad"][0]["latent_pi_2_weight"][3, 5] = np.nan
            s.dev["grad"][0].t["latent_pi_2_weight"][3, 5] = float("nan")
        env.actor_adam_step(actor, *s.args(), step=step, **HYPER)
        s.step_host(coef)
        bad, guards = s.differences(nan_ok=poison)
        assert not bad and guards, bad
        packed.append(actor.packed())
        states.append(s)
        actor.close()
    assert same(packed[0], fresh_packed(DeviceActor, states[0].params(), env)) and not np.isnan(packed[0]).any()
    for name in ("param", "exp_avg", "exp_avg_sq"):
        for k in ACTOR_KEYS:
            a, b = states[0].dev[name][0].host()[k], states[1].dev[name][0].host()[k]
            differs = words(a) != words(b)
            if k == "latent_pi_2_weight":
                assert differs.sum() == 1 and differs[3, 5] and np.isnan(b[3, 5]) and not np.isnan(a[3, 5]), (name, k)
            else:
                assert not differs.any(), (name, k)
    differs = words(packed[0]) != words(packed[1])
    assert differs.sum() == 1 and np.isnan(packed[1][differs]).all()

    # ---- critic: online NaN-filled and no target; then a NaN-filled target at tau = 1
    packed_online, packed_target, states = [], [], []
    for poison in (False, True):
        s = Sets(critic_shapes(kind, H), np.random.default_rng(6), env.device, nets=2)
        online, target = DeviceCritic(s.params(), env), DeviceCritic(s.params(), env)
        nan = on_device([nan_like(w) for w in s.params()], env)
        online.load_parameters(nan, tau=1.0)
        target.load_parameters(nan, tau=1.0)
        s.new_gradients()
        if poison:
            s.host["grad"][1]["q_0_weight"][7, 11] = np.nan
            s.dev["grad"][1].t["q_0_weight"][7, 11] = float("nan")
        env.critic_adam_step(online, *s.args(), step=step, target=target, tau=1.0, **HYPER)
        s.step_host(coef)
        bad, guards = s.differences(nan_ok=poison)
        assert not bad and guards, bad
        packed_online.append(online.packed()), packed_target.append(target.packed()), states.append(s)
        online.close(), target.close()
    fresh = fresh_packed(DeviceCritic, states[0].params(), env)
    assert same(packed_online[0], fresh) and same(packed_target[0], fresh) and not np.isnan(fresh).any()
    for name in ("param", "exp_avg", "exp_avg_sq"):
        for net in (0, 1):
            for k in CRITIC_ARRAYS:
                a, b = states[0].dev[name][net].host()[k], states[1].dev[name][net].host()[k]
                differs = words(a) != words(b)
                if (net, k) == (1, "q_0_weight"):
                    assert differs.sum() == 1 and differs[7, 11] and np.isnan(b[7, 11]), (name, net, k)
                else:
                    assert not differs.any(), (name, net, k)
    for got in (packed_online, packed_target):
        differs = words(got[0]) != words(got[1])
        assert differs.sum() == 1 and np.isnan(got[1][differs]).all()
    assert same(packed_online[1], packed_target[1])


def test_two_calls_from_the_same_state_give_the_same_bits(envs):
    env, kind, H = envs("dyn"), "dyn", 160
    results = []
    for _ in range(2):
        sa = Sets(actor_shapes(kind, H), np.random.default_rng(8), env.device)
        sc = Sets(critic_shapes(kind, H), np.random.default_rng(9), env.device, nets=2)
        actor, online, target = DeviceActor(sa.params(), env), DeviceCritic(sc.params(), env), DeviceCritic(sc.params(), env)
        for step in (1, 2):
            sa.new_gradients(), sc.new_gradients()
            env.actor_adam_step(actor, *sa.args(), step=step, **HYPER)
            env.critic_adam_step(online, *sc.args(), step=step, target=target, tau=0.005, **HYPER)
        results.append([actor.packed(), online.packed(), target.packed()] + [v for s in (sa, sc) for gs in s.dev.values() for g in gs for v in g.host().values()])
        for x in (actor, online, target):
            x.close()
    assert len(results[0]) == len(results[1]) == 3 + 4 * 8 + 4 * 2 * 6
    assert all(same(a, b) for a, b in zip(*results))


# ------------------------------------------------------------------------------------------------ stream order
def test_stream_order(envs):
    """gradients -> forward -> step -> forward without a host synchronisation: the step reads the gradients the call before it wrote,
    the first forward sees the old weights and the second the new."""
    env, kind, H = envs("dyn"), "dyn", 256
    s = Sets(actor_shapes(kind, H), np.random.default_rng(12), env.device)
    for k, v in s.params().items():  # a sensible actor, so that actions are not saturated
        v *= np.float32(0.1)
        s.dev["param"][0].t[k].copy_(torch.from_numpy(v))
    old = {k: v.copy() for k, v in s.params().items()}
    live = DeviceActor(old, env)
    X = torch.zeros((N, 6), dtype=torch.float32, device=env.device)
    Y = torch.zeros_like(X)
    d_action = torch.randn((N, 6), device=env.device) / N
    ws = env.actor_gradient_workspace(live, N)
    how = dict(mode="gaussian", seed=4, first_draw=1)
    torch.cuda.synchronize(env.device)
    env.actor_parameter_gradients(live, sample=how, d_action=d_action, out=s.dev["grad"][0].t, workspace=ws)  # writes the gradients ...
    env.policy_actions(live, out=X)
    env.actor_adam_step(live, *s.args(), step=1, lr=1e-2, betas=HYPER["betas"], eps=HYPER["eps"])  # ... the step reads them
    env.policy_actions(live, out=Y)
    torch.cuda.synchronize(env.device)
    s.host["grad"][0] = s.dev["grad"][0].host()
    assert any(np.any(g != 0) for g in s.host["grad"][0].values())
    s.step_host(adam_coefficients(env, lr=1e-2, betas=HYPER["betas"], eps=HYPER["eps"], step=1))
    bad, guards = s.differences()
    assert not bad and guards, bad
    A, B = DeviceActor(old, env), DeviceActor(s.params(), env)
    want_x, want_y = env.policy_actions(A).cpu().numpy(), env.policy_actions(B).cpu().numpy()
    assert same(X.cpu().numpy(), want_x) and same(Y.cpu().numpy(), want_y) and not same(want_x, want_y)
    for x in (A, B, live):
        x.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_everything_as_it_was(envs):
    env, other, kind, H = envs("dyn"), envs("sta"), "dyn", 64
    lib, stream = env.lib, env._stream()
    sa = Sets(actor_shapes(kind, H), np.random.default_rng(1), env.device)
    sc = Sets(critic_shapes(kind, H), np.random.default_rng(2), env.device, nets=2)
    sa.new_gradients(), sc.new_gradients()
    actor, online, target = DeviceActor(sa.params(), env), DeviceCritic(sc.params(), env), DeviceCritic(sc.params(), env)
    wide = DeviceCritic([draw(critic_shapes(kind, H + 32), lambda sh: np.zeros(sh, np.float32)) for _ in range(2)], env)
    stranger_a = DeviceActor(draw(actor_shapes("sta", H), lambda sh: np.zeros(sh, np.float32)), other)
    stranger_c = DeviceCritic([draw(critic_shapes("sta", H), lambda sh: np.zeros(sh, np.float32)) for _ in range(2)], other)
    before = actor.packed(), online.packed(), target.packed()
    fp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float))  # noqa: E731
    null = C.POINTER(C.c_float)()

    def hyper(**over):
        return _abi.AdamHyper(**dict(dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=1, reserved0=0), **over))

    def actor_tensors(null_at=None, **over):
        t = _abi.ActorAdam(47, H, 0)
        for name, w in zip(_abi.ADAM_SETS, sa.args()):
            setattr(t, name, _abi.ActorTensors(*[null if null_at == (name, f) else fp(w[k]) for f, k in zip(_abi.ACTOR_DEV_ARRAYS, ACTOR_KEYS)]))
        for k, v in over.items():
            setattr(t, k, v)
        return t

    def critic_tensors(null_at=None, **over):
        t = _abi.CriticAdam(53, H, 0)
        for name, ws in zip(_abi.ADAM_SETS, sc.args()):
            for i, w in enumerate(ws):
                getattr(t, name)[i] = _abi.QNetworkDev(*[null if null_at == (name, i, f) else fp(w[k]) for f, k in zip(("w0", "b0", "w1", "b1", "w_q", "b_q"), CRITIC_ARRAYS)])
        for k, v in over.items():
            setattr(t, k, v)
        return t

    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    call_a = lambda h, a, t, hp: lib.urgym_actor_adam_step(h, a, ref(t), ref(hp), stream)  # noqa: E731
    call_c = lambda h, c, tg, t, hp, tau=0.005: lib.urgym_critic_adam_step(h, c, tg, ref(t), ref(hp), tau, stream)  # noqa: E731
    nan, inf = float("nan"), float("inf")
    bad_hyper = [dict(lr=-1e-4), dict(lr=nan), dict(lr=inf), dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=nan), dict(beta2=1.0), dict(beta2=-0.1),
                 dict(beta2=nan), dict(eps=0.0), dict(eps=-1e-8), dict(eps=nan), dict(eps=inf), dict(step=0), dict(step=-1), dict(reserved0=1)]

    refused = [call_a(None, actor._a, actor_tensors(), hyper()), call_a(env._h, None, actor_tensors(), hyper()), call_a(env._h, actor._a, None, hyper()),
               call_a(env._h, actor._a, actor_tensors(), None), call_a(env._h, stranger_a._a, actor_tensors(), hyper()),
               call_a(other._h, actor._a, actor_tensors(), hyper()), call_a(env._h, actor._a, actor_tensors(in_features=41), hyper()),
               call_a(env._h, actor._a, actor_tensors(hidden_width=H + 32), hyper()), call_a(env._h, actor._a, actor_tensors(reserved0=1), hyper())]
    refused += [call_a(env._h, actor._a, actor_tensors(null_at=(name, f)), hyper()) for name in _abi.ADAM_SETS for f in _abi.ACTOR_DEV_ARRAYS]
    refused += [call_a(env._h, actor._a, actor_tensors(), hyper(**over)) for over in bad_hyper]
    n_actor = len(refused)
    assert n_actor == 9 + 32 + 16

    t, o = target._c, online._c
    refused += [call_c(None, o, t, critic_tensors(), hyper()), call_c(env._h, None, t, critic_tensors(), hyper()), call_c(env._h, o, t, None, hyper()),
                call_c(env._h, o, t, critic_tensors(), None), call_c(env._h, stranger_c._c, t, critic_tensors(), hyper()),
                call_c(env._h, o, stranger_c._c, critic_tensors(), hyper()), call_c(other._h, o, t, critic_tensors(), hyper()),
                call_c(env._h, o, o, critic_tensors(), hyper()),      # target == online
                call_c(env._h, o, wide._c, critic_tensors(), hyper()),  # a target of another width
                call_c(env._h, o, t, critic_tensors(in_features=47), hyper()), call_c(env._h, o, t, critic_tensors(hidden_width=H + 32), hyper()),
                call_c(env._h, o, t, critic_tensors(reserved0=1), hyper())]
    refused += [call_c(env._h, o, t, critic_tensors(null_at=(name, i, f)), hyper()) for name in _abi.ADAM_SETS for i in (0, 1) for f in ("w0", "b0", "w1", "b1", "w_q", "b_q")]
    refused += [call_c(env._h, o, t, critic_tensors(), hyper(**over)) for over in bad_hyper]
    refused += [call_c(env._h, o, t, critic_tensors(), hyper(), tau) for tau in (0.0, -0.005, 1.0000001, nan, inf, -inf)]
    assert len(refused) == n_actor + 12 + 48 + 16 + 6
    assert refused == [_abi.ERR_ARG] * len(refused)
    assert b"tau" in lib.urgym_last_error(env._h)
    # the Python layer refuses before the library is asked
    with pytest.raises(ValueError, match="tau"):
        env.critic_adam_step(online, *sc.args(), step=1, target=target, tau=0.0, **HYPER)
    with pytest.raises(ValueError, match="tau"):
        env.critic_adam_step(online, *sc.args(), step=1, target=target, **HYPER)
    with pytest.raises(ValueError, match="log_std"):
        env.actor_adam_step(actor, {k: v for k, v in sa.args()[0].items() if k in ACTOR_ARRAYS}, *sa.args()[1:], step=1, **HYPER)
    with pytest.raises(ValueError, match="is on cpu"):
        env.actor_adam_step(actor, {k: v.cpu() for k, v in sa.args()[0].items()}, *sa.args()[1:], step=1, **HYPER)
    with pytest.raises(ValueError, match="this environment"):
        env.critic_adam_step(stranger_c, *sc.args(), step=1, **HYPER)

    # nothing was launched: the read-back and all tensors are what they were, guards included
    torch.cuda.synchronize(env.device)
    assert same(actor.packed(), before[0]) and same(online.packed(), before[1]) and same(target.packed(), before[2])
    for s in (sa, sc):
        bad, guards = s.differences()
        assert not bad and guards, bad
    # tau is ignored without a target, and everything still works
    assert call_c(env._h, o, None, critic_tensors(), hyper(), nan) == _abi.OK
    assert call_a(env._h, actor._a, actor_tensors(), hyper()) == _abi.OK
    coef = adam_coefficients(env, step=1, **HYPER)
    sa.step_host(coef), sc.step_host(coef)
    for s in (sa, sc):
        bad, guards = s.differences()
        assert not bad and guards, bad
    assert same(actor.packed(), fresh_packed(DeviceActor, sa.params(), env)) and same(online.packed(), fresh_packed(DeviceCritic, sc.params(), env))
    assert same(target.packed(), before[2])
    for x in (actor, online, target, wide, stranger_a, stranger_c):
        x.close()


# ------------------------------------------------------------------------------------------------ against torch on the device
def test_three_steps_against_torch_adam_on_the_device(envs):
    """torch.optim.Adam (float32, its default implementation) on clones: both routes are within adam_cases.p_bound of float64 Adam
    (tests/test_adam_host.py checks that of adam_step), so they agree within twice the bound."""
    env, kind, H = envs("dyn"), "dyn", 160
    rng = np.random.default_rng(21)
    mild = lambda rng, sh: (rng.standard_normal(sh) * np.exp(rng.uniform(-30.0, 2.0, sh))).astype(np.float32)  # noqa: E731
    for lr in (1e-4, 1e-2):
        s = Sets(critic_shapes(kind, H), rng, env.device, nets=2)
        online = DeviceCritic(s.params(), env)
        p0_max = max(float(np.abs(v).max()) for w in s.params() for v in w.values())
        clones = [{k: t.detach().clone().requires_grad_(True) for k, t in g.t.items()} for g in s.dev["param"]]
        opt = torch.optim.Adam([t for w in clones for t in w.values()], lr=lr)
        for step in (1, 2, 3):
            s.new_gradients(mild)
            for w, g in zip(clones, s.dev["grad"]):
                for k, t in w.items():
                    t.grad = g.t[k].clone()
            opt.step()
            env.critic_adam_step(online, *s.args(), step=step, lr=lr, betas=HYPER["betas"], eps=HYPER["eps"])
            worst = max(float((t.detach() - g.t[k]).abs().max()) for w, g in zip(clones, s.dev["param"]) for k, t in w.items())
            print(f"lr={lr} step {step}: max |p - p_torch| = {worst:.3e}, bound {2 * p_bound(step, p0_max, lr):.3e}")
            assert worst <= 2 * p_bound(step, p0_max, lr), (lr, step, worst)
        online.close()


# ------------------------------------------------------------------------------------------------ the learner
def test_learner_with_the_device_optimizer():
    from ur_gym_amd.training import SAC_DEFAULTS, SACLearner, host_arrays

    assert SAC_DEFAULTS["device_optimizer"] is False
    env = make_vec("UR5OriReach-v1", num_envs=64, seed=5, auto_reset=True)
    env.reset(seed=5)
    three = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True)
    for missing in ("device_critic_gradient", "device_actor_gradient"):
        with pytest.raises(ValueError, match="device_optimizer needs"):
            SACLearner(env, seed=5, hidden_width=32, batch_size=64, device_optimizer=True, **dict(three, **{missing: False}))
    learner = SACLearner(env, seed=5, hidden_width=32, batch_size=64, device_optimizer=True, **three)
    twin = SACLearner(env, seed=5, hidden_width=32, batch_size=64, **three)  # the same seed: the same initial parameters
    assert twin.adam_state is None and learner.adam_state["step"] == 0  # with the option off nothing new is allocated
    lr, tau = learner.hp["learning_rate"], learner.hp["tau"]
    replay = DeviceReplay(env, 8)
    learner.collect(replay, 8)

    want_actor, want_critic = host_arrays(learner.actor.tensors()), host_arrays(learner.critic.tensors())
    assert all(same(want_actor[k], v) for k, v in host_arrays(twin.actor.tensors()).items())
    zeros = lambda w: {k: np.zeros_like(v) for k, v in w.items()}  # noqa: E731
    m_a, v_a = zeros(want_actor), zeros(want_actor)
    m_c, v_c = [zeros(w) for w in want_critic], [zeros(w) for w in want_critic]
    want_target = fresh_packed(DeviceCritic, want_critic, env)
    p0_max = max(float(np.abs(v).max()) for w in [want_actor] + want_critic for v in w.values())
    for i in range(3):
        losses = learner.update(replay, seed=11, draw=i)
        assert learner.adam_state["step"] == i + 1
        coef = adam_coefficients(env, lr, (0.9, 0.999), 1e-8, i + 1)
        g_a, g_c = host_arrays(learner.actor_grads), host_arrays(learner.critic_grads)  # the .grad tensors the kernels wrote
        assert all(p.grad is learner.actor_grads[k] for k, p in learner.actor.tensors().items())
        for k in want_actor:
            want_actor[k], m_a[k], v_a[k] = adam_step(want_actor[k], g_a[k], m_a[k], v_a[k], coef)
        for n in (0, 1):
            for k in want_critic[n]:
                want_critic[n][k], m_c[n][k], v_c[n][k] = adam_step(want_critic[n][k], g_c[n][k], m_c[n][k], v_c[n][k], coef)
        got_actor, got_critic = host_arrays(learner.actor.tensors()), host_arrays(learner.critic.tensors())
        assert all(same(got_actor[k], want_actor[k]) for k in want_actor), i
        assert all(same(got_critic[n][k], want_critic[n][k]) for n in (0, 1) for k in want_critic[n]), i
        assert any(np.any(g != 0) for g in g_a.values()) and any(np.any(g != 0) for w in g_c for g in w.values())
        assert same(learner.device_actor.packed(), fresh_packed(DeviceActor, got_actor, env))
        packed_critic = fresh_packed(DeviceCritic, got_critic, env)
        assert same(learner.online.packed(), packed_critic)
        want_target = polyak(want_target, packed_critic, tau)
        assert same(learner.target.packed(), want_target)
        assert all(np.isfinite(v.item()) for v in losses.values())
        if i == 0:  # the gradients of update 1 are the same kernels on the same bits: torch's Adam agrees within twice the bound
            twin.update(replay, seed=11, draw=0)
            other_actor, other_critic = host_arrays(twin.actor.tensors()), host_arrays(twin.critic.tensors())
            assert all(same(host_arrays(twin.actor_grads)[k], g_a[k]) for k in g_a)
            worst = max([float(np.abs(other_actor[k] - got_actor[k]).max()) for k in got_actor] +
                        [float(np.abs(other_critic[n][k] - got_critic[n][k]).max()) for n in (0, 1) for k in got_critic[n]])
            print(f"update 1: max |p - p_torch| = {worst:.3e}, bound {2 * p_bound(1, p0_max, lr):.3e}")
            assert worst <= 2 * p_bound(1, p0_max, lr)
    learner.collect(replay, 2)  # the sampled policy, on the actor the step kernel packed
    torch.cuda.synchronize(env.device)  # raises if any launch left an error
    assert np.isfinite(replay.ring["action"].cpu().numpy()).all()
    learner.close(), twin.close()
    env.close()
