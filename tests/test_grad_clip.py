"""GPU tests (-m gpu) of gradient-norm clipping on the device: urgym_actor_grad_norm / urgym_critic_grad_norm,
urgym_actor_adam_step_scaled / urgym_critic_adam_step_scaled, urgym_sac_train_clipped and SACLearner(max_grad_norm=X).

The two norm calls are compared BIT FOR BIT with evaluation.grad_norm on the groups of tests/grad_clip_cases.py -- the per-tensor sums,
the float32 norm and the coefficient, so the device's float64 square root is held bitwise to the host's correctly rounded one -- and
the scaled steps with evaluation.adam_step(scale=), the packed buffers with fresh packs, the target with evaluation.polyak.  The
learner is compared update by update with the restatement on ``last_update``, and the training call with the Python loop of
``collect`` / ``update``.  Small shapes: the learner runs at batch 32, H = 32.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_clip_cases as gc
from adam_cases import HYPER
from grad_clip_cases import CASES, same, same64
from test_adam import Guarded, Sets, actor_shapes, critic_shapes, fresh_packed
from test_evaluation import EVAL_SEED, EVAL_STEPS, eval_env
from test_monitor import assert_same_monitor
from test_sac_terms import ALLOCATIONS_AND_VIEWS
from test_sac_train import ALL, CAP, H, N, SEED, STARTS, UPDATE_SEED, Side, assert_same_losses, assert_same_state, bits, guarded, guards_intact
from ur_gym_amd import _abi, make_vec
from ur_gym_amd._native import NativeError
from ur_gym_amd.evaluation import (ACTOR_ARRAYS, CRITIC_ARRAYS, LOG_STD_ARRAYS, DeviceActor, DeviceCritic, DeviceEvaluation, DeviceMonitor,
                                   DevicePrioritizedReplay, DeviceReplay, adam_coefficients, adam_step, grad_norm, polyak)
from ur_gym_amd.training import SACLearner

pytestmark = pytest.mark.gpu

NUM_ENVS = 8
ACTOR_KEYS = ACTOR_ARRAYS + LOG_STD_ARRAYS
M = 32         # the learner's batch
CLIP = 1e-2    # the learner's bound: far below the gradient norms of a fresh learner on these rewards, so both groups clip
NAN = float("nan")


@pytest.fixture(scope="module")
def envs():
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = make_vec(gc.ENV_ID[kind], num_envs=NUM_ENVS, seed=3, auto_reset=True)
            made[kind].reset(seed=3)
        return made[kind]

    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def references():
    """evaluation.grad_norm's sums of every shared group, computed once (the bound does not reach them)."""
    return {(which, kind, Hh): grad_norm(gc.group(which, kind, Hh), 1.0) for kind, Hh in CASES for which in ("actor", "critic")}


def zero_object(which, kind, Hh, env):
    if which == "actor":
        return DeviceActor({k: np.zeros(sh, np.float32) for k, sh in actor_shapes(kind, Hh).items()}, env)
    return DeviceCritic([{k: np.zeros(sh, np.float32) for k, sh in critic_shapes(kind, Hh).items()} for _ in range(2)], env)


def guarded_group(which, tensors, device):
    """The group on the device as guarded, misaligned views (test_adam.Guarded), as the env methods take it."""
    if which == "actor":
        g = [Guarded(gc.as_actor_dict(tensors), device)]
        return g, g[0].t
    g = [Guarded(w, device) for w in gc.as_critic_dicts(tensors)]
    return g, [x.t for x in g]


def norm_call(env, which, obj, grads, max_norm, out):
    call = env.actor_gradient_norm if which == "actor" else env.critic_gradient_norm
    return call(obj, grads, max_norm, norm_out=out["norm"][1], scale_out=out["scale"][1], tensor_sums_out=out["tensor_sums"][1])


def outputs(device, tensors):
    return dict(norm=guarded((1,), torch.float32, device, NAN), scale=guarded((1,), torch.float32, device, NAN),
                tensor_sums=guarded((tensors,), torch.float64, device, NAN))


def assert_norm(out, want, where):
    torch.cuda.synchronize()
    assert guards_intact(out) is None, (where, guards_intact(out))
    got = {k: v[1].cpu().numpy() for k, v in out.items()}
    assert same64(got["tensor_sums"], want["tensor_sums"]), (where, got["tensor_sums"], want["tensor_sums"])
    print(f"{where}: norm64 = {float(want['norm64'])!r}, device norm {got['norm'][0]!r}, scale {got['scale'][0]!r} (restated {want['scale']!r})")
    assert same(got["norm"][0], want["norm"]) and same(got["scale"][0], want["scale"]), (where, got["norm"], want["norm"], got["scale"], want["scale"])


# ------------------------------------------------------------------------------------------------ 1. the norm calls
@pytest.mark.parametrize("kind,Hh", CASES, ids=[f"{k}-{h}" for k, h in CASES])
@pytest.mark.parametrize("which", ("actor", "critic"))
def test_norm_equals_the_restatement_bitwise(envs, references, which, kind, Hh):
    env = envs(kind)
    tensors = gc.group(which, kind, Hh)
    obj = zero_object(which, kind, Hh, env)
    holders, grads = guarded_group(which, tensors, env.device)
    before = [h.host() for h in holders]
    ref = references[(which, kind, Hh)]
    n = float(ref["norm64"])
    for max_norm in (np.float32(2.0 * n), np.float32(0.5 * n), np.float32(1e-3 * n)):
        want = grad_norm(tensors, max_norm)
        assert same64(want["tensor_sums"], ref["tensor_sums"])
        out = outputs(env.device, len(tensors))
        norm_call(env, which, obj, grads, float(max_norm), out)
        assert_norm(out, want, (which, kind, Hh, float(max_norm)))
        first = {k: v[1].clone() for k, v in out.items()}
        norm_call(env, which, obj, grads, float(max_norm), out)  # repeatable: the same words from a second launch
        torch.cuda.synchronize(env.device)
        assert all(np.array_equal(bits(first[k]), bits(out[k][1])) for k in out)
    # the gradient tensors are only read, and nothing around them is written
    assert all(h.guards_intact() for h in holders)
    for h, was in zip(holders, before):
        assert all(same(h.host()[k], was[k]) for k in was)
    # without the sums: the same norm and coefficient, and the call allocates what it is not handed
    got = (env.actor_gradient_norm if which == "actor" else env.critic_gradient_norm)(obj, grads, float(np.float32(0.5 * n)))
    torch.cuda.synchronize(env.device)
    want = grad_norm(tensors, np.float32(0.5 * n))
    assert same(got["scale"].cpu().numpy()[0], want["scale"]) and same64(got["tensor_sums"].cpu().numpy(), want["tensor_sums"])
    # the non-finite cases of the header
    big = max(range(len(tensors)), key=lambda k: tensors[k].size)
    for value in (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)):
        bad = gc.with_element(tensors, big, tensors[big].size // 2, value)
        holders_bad, grads_bad = guarded_group(which, bad, env.device)
        out = outputs(env.device, len(tensors))
        norm_call(env, which, obj, grads_bad, 1.0, out)
        torch.cuda.synchronize(env.device)
        want, got_norm, got_scale = grad_norm(bad, 1.0), out["norm"][1].cpu().numpy()[0], out["scale"][1].cpu().numpy()[0]
        assert same(got_scale, want["scale"]) and same(got_scale, np.float32(1.0 if np.isnan(value) else 0.0)), (which, kind, Hh, value)
        assert np.isnan(got_norm) if np.isnan(value) else got_norm == np.float32(np.inf)
    obj.close()


def test_norm_follows_a_preceding_writer_in_stream_order(envs):
    env, which, kind, Hh = envs("ori"), "critic", "ori", 64
    tensors = gc.moderate_group(which, kind, Hh)
    obj = zero_object(which, kind, Hh, env)
    holders, grads = guarded_group(which, tensors, env.device)
    out_a, out_b = outputs(env.device, 12), outputs(env.device, 12)
    norm_call(env, which, obj, grads, 1.0, out_a)
    for w in grads:  # a device-side writer on the same stream, no synchronisation: doubling is exact
        for t in w.values():
            t.mul_(2.0)
    norm_call(env, which, obj, grads, 1.0, out_b)
    assert_norm(out_a, grad_norm(tensors, 1.0), "before the writer")
    assert_norm(out_b, grad_norm([2.0 * g for g in tensors], 1.0), "after the writer")
    obj.close()


# ------------------------------------------------------------------------------------------------ 2. the scaled steps
def step_host_scaled(s, coef, scale):
    h = s.host
    for i in range(len(h["param"])):
        for k in s.shapes:
            h["param"][i][k], h["exp_avg"][i][k], h["exp_avg_sq"][i][k] = adam_step(h["param"][i][k], h["grad"][i][k], h["exp_avg"][i][k], h["exp_avg_sq"][i][k],
                                                                                      coef, scale=scale)


def moderate(rng, shape):
    return (rng.standard_normal(shape) * np.power(10.0, rng.uniform(-3.0, 0.0, shape))).astype(np.float32)


@pytest.mark.parametrize("kind,Hh", CASES, ids=[f"{k}-{h}" for k, h in CASES])
def test_scaled_actor_step(envs, kind, Hh):
    env = envs(kind)
    a, twin = (Sets(actor_shapes(kind, Hh), np.random.default_rng(300 + Hh), env.device) for _ in range(2))
    actor, actor_twin = zero_object("actor", kind, Hh, env), zero_object("actor", kind, Hh, env)
    for step, factor in ((1, 0.25), (2, 1e6), (3, 0.9)):
        a.new_gradients(moderate), twin.new_gradients(moderate)
        grads = [a.host["grad"][0][k] for k in ACTOR_KEYS]
        max_norm = np.float32(factor * float(grad_norm(grads, 1.0)["norm64"]))
        want = grad_norm(grads, max_norm)
        got = env.actor_gradient_norm(actor, a.args()[1], float(max_norm))
        env.actor_adam_step(actor, *a.args(), step=step, scale=got["scale"], **HYPER)
        env.actor_adam_step(actor_twin, *twin.args(), step=step, **HYPER)  # the unscaled kernels, on a twin
        coef = adam_coefficients(env, step=step, **HYPER)
        step_host_scaled(a, coef, want["scale"])
        twin.step_host(coef)
        assert same(got["scale"].cpu().numpy()[0], want["scale"]) and (want["scale"] == 1.0) == (factor > 1), (step, want["scale"])
        for s, obj, what in ((a, actor, "scaled"), (twin, actor_twin, "unscaled twin")):
            bad, guards = s.differences()
            assert not bad and guards, (what, step, bad, guards)  # p', m', v' bitwise, and the gradients (a set of the mirror) unchanged
            assert same(obj.packed(), fresh_packed(DeviceActor, s.params(), env)), (what, step)
        equal = all(same(a.host[name][0][k], twin.host[name][0][k]) for name in ("param", "exp_avg", "exp_avg_sq") for k in ACTOR_KEYS)
        if factor > 1:  # scale == 1.0f: every output is the unscaled call's
            assert equal and same(actor.packed(), actor_twin.packed())
        else:
            assert not equal and not same(actor.packed(), actor_twin.packed())
            for name in ("param", "exp_avg", "exp_avg_sq"):  # carry on from one state
                for k in ACTOR_KEYS:
                    twin.host[name][0][k] = a.host[name][0][k].copy()
                    twin.dev[name][0].t[k].copy_(a.dev[name][0].t[k])
            actor_twin.load_parameters(twin.dev["param"][0].t)
    actor.close(), actor_twin.close()


@pytest.mark.parametrize("kind,Hh", CASES, ids=[f"{k}-{h}" for k, h in CASES])
def test_scaled_critic_step_and_the_targets_blend(envs, kind, Hh):
    env = envs(kind)
    a, twin = (Sets(critic_shapes(kind, Hh), np.random.default_rng(400 + Hh), env.device, nets=2) for _ in range(2))
    online, online_twin = zero_object("critic", kind, Hh, env), zero_object("critic", kind, Hh, env)
    half = [{k: (0.5 * v).astype(np.float32) for k, v in w.items()} for w in a.params()]
    target, target_twin = DeviceCritic(half, env), DeviceCritic(half, env)
    want_target = {id(a): target.packed(), id(twin): target_twin.packed()}
    for step, factor, tau in ((1, 0.25, 0.005), (2, 1e6, 0.005), (3, 0.9, 1.0)):
        a.new_gradients(moderate), twin.new_gradients(moderate)
        grads = [a.host["grad"][net][k] for net in range(2) for k in CRITIC_ARRAYS]
        max_norm = np.float32(factor * float(grad_norm(grads, 1.0)["norm64"]))
        want = grad_norm(grads, max_norm)
        got = env.critic_gradient_norm(online, a.args()[1], float(max_norm))
        env.critic_adam_step(online, *a.args(), step=step, target=target, tau=tau, scale=got["scale"], **HYPER)
        env.critic_adam_step(online_twin, *twin.args(), step=step, target=target_twin, tau=tau, **HYPER)
        coef = adam_coefficients(env, step=step, **HYPER)
        step_host_scaled(a, coef, want["scale"])
        twin.step_host(coef)
        assert same(got["scale"].cpu().numpy()[0], want["scale"]) and (want["scale"] == 1.0) == (factor > 1), (step, want["scale"])
        for s, on, tg, what in ((a, online, target, "scaled"), (twin, online_twin, target_twin, "unscaled twin")):
            bad, guards = s.differences()
            assert not bad and guards, (what, step, bad, guards)
            fresh = fresh_packed(DeviceCritic, s.params(), env)
            assert same(on.packed(), fresh), (what, step)
            want_target[id(s)] = polyak(want_target[id(s)], fresh, tau)
            assert same(tg.packed(), want_target[id(s)]), (what, step, tau)
        equal = all(same(a.host[name][net][k], twin.host[name][net][k]) for name in ("param", "exp_avg", "exp_avg_sq") for net in range(2) for k in CRITIC_ARRAYS)
        if factor > 1:
            assert equal and same(online.packed(), online_twin.packed()) and same(target.packed(), target_twin.packed())
        else:
            assert not equal and not same(online.packed(), online_twin.packed())
            for name in ("param", "exp_avg", "exp_avg_sq"):
                for net in range(2):
                    for k in CRITIC_ARRAYS:
                        twin.host[name][net][k] = a.host[name][net][k].copy()
                        twin.dev[name][net].t[k].copy_(a.dev[name][net].t[k])
            online_twin.load_parameters([g.t for g in twin.dev["param"]], tau=1.0)
            target_twin.load_parameters([g.t for g in a.dev["param"]], tau=1.0), target.load_parameters([g.t for g in a.dev["param"]], tau=1.0)
            want_target = {id(a): target.packed(), id(twin): target_twin.packed()}
    for c in (online, online_twin, target, target_twin):
        c.close()


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_launch_nothing_and_write_nothing(envs):
    env, other = envs("ori"), envs("dyn")
    lib, dev = env.lib, env.device
    actor, critic = zero_object("actor", "ori", 32, env), zero_object("critic", "ori", 32, env)
    foreign_actor, foreign_critic = zero_object("actor", "dyn", 64, other), zero_object("critic", "dyn", 64, other)
    sa, sc = Sets(actor_shapes("ori", 32), np.random.default_rng(1), dev), Sets(critic_shapes("ori", 32), np.random.default_rng(2), dev, nets=2)
    sa.new_gradients(moderate), sc.new_gradients(moderate)
    out = outputs(dev, 12)
    scale = guarded((1,), torch.float32, dev, 0.5)
    fptr = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float))  # noqa: E731

    def actor_grads(**over):
        t = {k: fptr(v) for k, v in zip(_abi.ACTOR_DEV_ARRAYS, [sa.dev["grad"][0].t[k] for k in ACTOR_KEYS])}
        t.update(over)
        return _abi.ActorTensors(**t)

    def critic_grads(null=None):
        nets = (_abi.QNetworkDev * 2)()
        for i in range(2):
            nets[i] = _abi.QNetworkDev(*[None if null == (i, k) else fptr(sc.dev["grad"][i].t[k]) for k in CRITIC_ARRAYS])
        return nets

    def args(**over):
        a = dict(max_norm=1.0, reserved0=0, norm_out=fptr(out["norm"][1]), scale_out=fptr(out["scale"][1]),
                 tensor_sums_out=C.cast(out["tensor_sums"][1].data_ptr(), C.POINTER(C.c_double)))
        a.update(over)
        return _abi.GradNorm(**a)

    def everything():
        parts = [flat for flat, _ in out.values()] + [scale[0]] + [g for s in (sa, sc) for gs in s.dev.values() for x in gs for g in x.flat.values()]
        parts += [torch.from_numpy(o.packed()).to(dev) for o in (actor, critic)]
        return torch.cat([p.contiguous().view(torch.uint8).reshape(-1) for p in parts])

    before = everything()

    def refused(what, rc, handle=env._h, expect=None):
        assert rc == _abi.ERR_ARG, (what, rc)
        if expect:
            assert expect.encode() in lib.urgym_last_error(handle), (what, lib.urgym_last_error(handle))

    misaligned = C.cast(out["tensor_sums"][1].data_ptr() + 4, C.POINTER(C.c_double))
    for what, over, expect in (("reserved0", dict(reserved0=1), "reserved0"), ("zero bound", dict(max_norm=0.0), "max_norm"), ("negative bound", dict(max_norm=-1.0), "max_norm"),
                               ("NaN bound", dict(max_norm=NAN), "max_norm"), ("infinite bound", dict(max_norm=float("inf")), "max_norm"),
                               ("null norm_out", dict(norm_out=None), "norm_out"), ("null scale_out", dict(scale_out=None), "scale_out"),
                               ("misaligned sums", dict(tensor_sums_out=misaligned), "8-byte")):
        refused(what, lib.urgym_actor_grad_norm(env._h, actor._a, C.byref(actor_grads()), C.byref(args(**over)), None), expect=expect)
        refused(what, lib.urgym_critic_grad_norm(env._h, critic._c, critic_grads(), C.byref(args(**over)), None), expect=expect)
    refused("null handle", lib.urgym_actor_grad_norm(None, actor._a, C.byref(actor_grads()), C.byref(args()), None), handle=None, expect="null handle")
    refused("null actor", lib.urgym_actor_grad_norm(env._h, None, C.byref(actor_grads()), C.byref(args()), None), expect="not an actor")
    refused("another handle's actor", lib.urgym_actor_grad_norm(env._h, foreign_actor._a, C.byref(actor_grads()), C.byref(args()), None), expect="not an actor")
    refused("null grad", lib.urgym_actor_grad_norm(env._h, actor._a, None, C.byref(args()), None), expect="null grad")
    refused("null args", lib.urgym_actor_grad_norm(env._h, actor._a, C.byref(actor_grads()), None, None), expect="null args")
    refused("a null tensor", lib.urgym_actor_grad_norm(env._h, actor._a, C.byref(actor_grads(w_mu=None)), C.byref(args()), None), expect="tensor pointer")
    refused("null critic", lib.urgym_critic_grad_norm(env._h, None, critic_grads(), C.byref(args()), None), expect="not a critic")
    refused("another handle's critic", lib.urgym_critic_grad_norm(env._h, foreign_critic._c, critic_grads(), C.byref(args()), None), expect="not a critic")
    refused("null grad", lib.urgym_critic_grad_norm(env._h, critic._c, None, C.byref(args()), None), expect="null grad")
    refused("a null tensor", lib.urgym_critic_grad_norm(env._h, critic._c, critic_grads(null=(1, "q_4_bias")), C.byref(args()), None), expect="tensor pointer")

    # the scaled steps: a null scale_dev, and the unscaled step's own refusals
    def actor_adam(**over):
        t = _abi.ActorAdam(30, 32, 0)
        for name, tensors in zip(_abi.ADAM_SETS, sa.args()):
            setattr(t, name, _abi.ActorTensors(*[fptr(tensors[k]) for k in ACTOR_KEYS]))
        for k, v in over.items():
            setattr(t, k, v)
        return t

    def critic_adam(**over):
        t = _abi.CriticAdam(36, 32, 0)
        for name, tensors in zip(_abi.ADAM_SETS, sc.args()):
            nets = getattr(t, name)
            for i, w in enumerate(tensors):
                nets[i] = _abi.QNetworkDev(*[fptr(w[k]) for k in CRITIC_ARRAYS])
        for k, v in over.items():
            setattr(t, k, v)
        return t

    hp = lambda **over: _abi.AdamHyper(**dict(dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=1, reserved0=0), **over))  # noqa: E731
    sptr = C.c_void_p(scale[1].data_ptr())
    refused("null scale_dev", lib.urgym_actor_adam_step_scaled(env._h, actor._a, C.byref(actor_adam()), C.byref(hp()), None, None), expect="null scale_dev")
    refused("null scale_dev", lib.urgym_critic_adam_step_scaled(env._h, critic._c, None, C.byref(critic_adam()), C.byref(hp()), 1.0, None, None), expect="null scale_dev")
    for what, a_over, h_over, expect in (("reserved0", dict(reserved0=1), {}, "reserved0"), ("width", dict(hidden_width=64), {}, "tensors are"),
                                         ("step 0", {}, dict(step=0), "step"), ("negative lr", {}, dict(lr=-1.0), "lr"), ("beta1 = 1", {}, dict(beta1=1.0), "beta"),
                                         ("eps = 0", {}, dict(eps=0.0), "eps")):
        refused(what, lib.urgym_actor_adam_step_scaled(env._h, actor._a, C.byref(actor_adam(**a_over)), C.byref(hp(**h_over)), sptr, None), expect=expect)
        refused(what, lib.urgym_critic_adam_step_scaled(env._h, critic._c, None, C.byref(critic_adam(**a_over)), C.byref(hp(**h_over)), 1.0, sptr, None), expect=expect)
    refused("null handle", lib.urgym_actor_adam_step_scaled(None, actor._a, C.byref(actor_adam()), C.byref(hp()), sptr, None), handle=None, expect="null handle")
    refused("another handle's actor", lib.urgym_actor_adam_step_scaled(env._h, foreign_actor._a, C.byref(actor_adam()), C.byref(hp()), sptr, None), expect="not an actor")
    refused("null tensors", lib.urgym_actor_adam_step_scaled(env._h, actor._a, None, C.byref(hp()), sptr, None), expect="null tensors")
    refused("null hp", lib.urgym_actor_adam_step_scaled(env._h, actor._a, C.byref(actor_adam()), None, sptr, None))
    refused("another handle's critic", lib.urgym_critic_adam_step_scaled(env._h, foreign_critic._c, None, C.byref(critic_adam()), C.byref(hp()), 1.0, sptr, None), expect="not a critic")
    refused("the target is the online critic", lib.urgym_critic_adam_step_scaled(env._h, critic._c, critic._c, C.byref(critic_adam()), C.byref(hp()), 0.5, sptr, None), expect="itself")
    torch.cuda.synchronize(dev)
    assert torch.equal(before, everything())
    # the Python layer's own refusals
    with pytest.raises(ValueError, match="max_norm"):
        env.actor_gradient_norm(actor, sa.args()[1], 0.0)
    with pytest.raises(ValueError, match="scale"):
        env.actor_adam_step(actor, *sa.args(), step=1, scale=torch.ones(2, device=dev), **HYPER)
    with pytest.raises(ValueError, match="scale"):
        env.critic_adam_step(critic, *sc.args(), step=1, scale=torch.ones(1, dtype=torch.float64, device=dev), **HYPER)
    for o in (actor, critic, foreign_actor, foreign_critic):
        o.close()


# ------------------------------------------------------------------------------------------------ 4. the learner
CLIPPED = dict(max_grad_norm=CLIP)
NORM_KEYS = ("critic_grad_norm", "actor_grad_norm")


def host(w):
    return {k: v.detach().cpu().numpy().copy() for k, v in w.items()}


def snapshot(lr):
    st = lr.adam_state
    return dict(actor=[host(lr.actor.tensors()), host(st["actor"][0]), host(st["actor"][1])],
                critic=[[host(w) for w in lr.critic.tensors()], [host(w) for w in st["critic"][0]], [host(w) for w in st["critic"][1]]])


def clipped_loop(side, iterations, K, G, first_draw, monitor=None, evaluation=None):
    """Side.loop that also keeps the two norms of every update, and folds / records / evaluates as train does where asked to."""
    lr, losses, draw = side.learner, [], first_draw
    for _ in range(iterations):
        if K:
            lr.collect(side.replay, K, monitor=monitor)
        before = lr.adam_state["step"]
        if lr.env_steps * side.env.num_envs >= lr.hp["learning_starts"]:
            for _ in range(G):
                got = lr.update(side.replay, UPDATE_SEED, draw)
                losses.append(dict({k: v.clone() for k, v in got.items()}, **{k: lr.last_update[k][0].clone() for k in NORM_KEYS}))
                draw += 1
        if monitor is not None:
            monitor.iterations += 1
            if monitor.iterations % 2 == 0:
                monitor.record(monitor.iterations)
        if evaluation is not None and lr.adam_state["step"] // 4 > before // 4:
            evaluation.evaluate(lr.actor.tensors())
    return losses


def assert_same_clipped_losses(want, got, what):
    assert sorted(got) == sorted(("critic_loss", "actor_loss", "ent_coef_loss") + NORM_KEYS) and all(v.shape == (len(want),) for v in got.values()), what
    for u, w in enumerate(want):
        for k in got:
            assert np.array_equal(bits(got[k][u]), bits(w[k])), (what, u, k, float(got[k][u]), float(w[k]))


def assert_same_clipped_last_update(a, b, what):
    la, lb = a.learner.last_update, b.learner.last_update
    assert sorted(la) == sorted(lb) and set(NORM_KEYS) | {"critic_scale", "actor_scale"} <= set(la), (what, sorted(la), sorted(lb))
    for k in la:
        assert la[k].shape == lb[k].shape and np.array_equal(bits(la[k]), bits(lb[k])), (what, k)


def test_update_by_update_equals_the_restatement():
    s = Side(M=M, **CLIPPED)
    lr = s.learner
    lr.collect(s.replay, CAP)
    clipped = {"critic": 0, "actor": 0}
    for draw in range(5):
        was = snapshot(lr)
        lr.update(s.replay, UPDATE_SEED, draw)
        torch.cuda.synchronize(s.env.device)
        coef = adam_coefficients(s.env, lr=lr.hp["learning_rate"], step=lr.adam_state["step"])
        last, now = lr.last_update, snapshot(lr)
        ga, gc_ = host(lr.actor_grads), [host(w) for w in lr.critic_grads]
        for which, grads in (("critic", gc_), ("actor", ga)):
            want = grad_norm(grads, CLIP)
            norm, scale = last[f"{which}_grad_norm"].cpu().numpy(), last[f"{which}_scale"].cpu().numpy()
            print(f"update {draw}: {which} norm {norm[0]!r} scale {scale[0]!r}")
            assert norm.shape == scale.shape == (1,) and same(norm[0], want["norm"]) and same(scale[0], want["scale"]), (draw, which, norm, want)
            clipped[which] += bool(scale[0] < 1.0)
            nets = zip(*was[which], grads, *now[which]) if which == "critic" else [(*was[which], grads, *now[which])]
            for p, m, v, g, p1, m1, v1 in nets:
                for k in p:
                    wp, wm, wv = adam_step(p[k], g[k], m[k], v[k], coef, scale=want["scale"])
                    assert same(p1[k], wp) and same(m1[k], wm) and same(v1[k], wv), (draw, which, k)
    assert clipped["critic"] > 0 and clipped["actor"] > 0, clipped  # the bound is below a fresh learner's norms: both groups were scaled
    assert same(lr.device_actor.packed(), fresh_packed(DeviceActor, host(lr.actor.tensors()), s.env))
    assert same(lr.online.packed(), fresh_packed(DeviceCritic, [host(w) for w in lr.critic.tensors()], s.env))
    s.close()


def test_train_equals_the_python_loop_bit_for_bit():
    a, b, c = Side(M=M, **CLIPPED), Side(M=M, **CLIPPED), Side(M=M, **CLIPPED)
    want = clipped_loop(a, 6, 1, 2, first_draw=7)                                        # a: collect / update in Python
    got = b.learner.train(b.replay, 6, 1, 2, seed=UPDATE_SEED, first_draw=7)             # b: ONE native call
    first = c.learner.train(c.replay, 2, 1, 2, seed=UPDATE_SEED, first_draw=7)           # c: the call split in two
    second = c.learner.train(c.replay, 4, 1, 2, seed=UPDATE_SEED, first_draw=7 + 2)
    torch.cuda.synchronize(a.env.device)
    assert len(want) == 10
    assert_same_clipped_losses(want, got, "one call")
    assert_same_state(a, b, "one call"), assert_same_clipped_last_update(a, b, "one call")
    for k in got:
        assert np.array_equal(bits(got[k]), bits(torch.cat([first[k], second[k]]))), k
    assert_same_state(a, c, "2 + 4 iterations"), assert_same_clipped_last_update(a, c, "2 + 4 iterations")
    assert all(np.isfinite(bits(got[k]).view(np.float32)).all() and (got[k] > 0).all() for k in NORM_KEYS)
    # clipping is another computation than the learner without it
    d = Side(M=M)
    other = d.learner.train(d.replay, 6, 1, 2, seed=UPDATE_SEED, first_draw=7)
    torch.cuda.synchronize(a.env.device)
    assert sorted(other) == ["actor_loss", "critic_loss", "ent_coef_loss"] and not np.array_equal(bits(other["critic_loss"]), bits(got["critic_loss"]))
    for s in (a, b, c, d):
        s.close()


class ClippedSide(Side):
    """test_sac_train's Side at batch 32 with episodes of at most 3 steps and the option under test; a monitor and an evaluation on
    request."""

    def __init__(self, env_id="UR5OriReach-v1", monitored=False, prioritized=False, **over):
        self.env = make_vec(env_id, num_envs=N, seed=SEED, auto_reset=True, max_episode_steps=3)
        self.env.reset(seed=SEED)
        self.learner = SACLearner(self.env, seed=SEED, hidden_width=H, batch_size=M, learning_starts=STARTS, **dict(ALL, **dict(CLIPPED, prioritized=prioritized, **over)))
        self.replay = DevicePrioritizedReplay(self.env, 40, alpha=0.6, eps=1e-6) if prioritized else DeviceReplay(self.env, CAP)
        self.mon = self.ev = self.test_env = None
        if monitored:
            self.mon = DeviceMonitor(self.env, capacity=4)
            self.mon.records.fill_(-1)
            self.test_env = eval_env(env_id, N)
            self.ev = DeviceEvaluation(self.test_env, self.learner.actor.tensors(), num_steps=EVAL_STEPS, seed=EVAL_SEED, capacity=4)
            self.ev.records.fill_(-1)

    def state(self):
        out = super().state()
        if hasattr(self.replay, "leaf"):
            out.update(leaf=self.replay.leaf, sums=self.replay.sums, max_leaf=self.replay.max_leaf)
        return out

    def monitor_state(self):
        return dict(self.mon.state, records=self.mon.records)

    def evaluation_state(self):
        out = {f"eval.buf.{k}": v for k, v in self.test_env.buf.items()}
        out.update({f"best.{k}": v for k, v in self.ev.best.items()})
        out.update(records=self.ev.records, best_mean=self.ev.best_mean, best_index=self.ev.best_index, eval_packed=self.ev.actor.packed())
        return out

    def close(self):
        if self.ev is not None:
            self.ev.close(), self.test_env.close()
        super().close()


@pytest.mark.parametrize("option", [dict(n_steps=3), dict(prioritized=True, per_beta=0.4, per_beta_steps=7), dict(hindsight=True), dict(monitored=True)],
                         ids=["n_steps", "prioritized", "hindsight", "monitor-and-evaluation"])
def test_train_with_each_other_option(option):
    env_id = "UR5DynReach-v1" if option.get("hindsight") or option.get("prioritized") else "UR5OriReach-v1"
    a, b = ClippedSide(env_id, **option), ClippedSide(env_id, **option)
    want = clipped_loop(a, 6, 1, 2, first_draw=7, monitor=a.mon, evaluation=a.ev)
    extra = {} if b.mon is None else dict(monitor=b.mon, log_every=2, evaluation=b.ev, eval_every=4)
    got = b.learner.train(b.replay, 6, 1, 2, seed=UPDATE_SEED, first_draw=7, **extra)  # ONE call: urgym_sac_train_clipped with the option
    torch.cuda.synchronize(a.env.device)
    assert len(want) == 10
    assert_same_clipped_losses(want, got, str(option))
    assert_same_state(a, b, str(option)), assert_same_clipped_last_update(a, b, str(option))
    if b.mon is not None:
        assert_same_monitor(a, b, "monitor and evaluation")
        sa, sb = a.evaluation_state(), b.evaluation_state()
        for k in sa:
            assert np.array_equal(bits(sa[k]), bits(sb[k])), k
        assert a.ev.count == b.ev.count == 2 and a.mon.count == b.mon.count == 3
    a.close(), b.close()


def test_a_huge_bound_is_the_learner_without_the_option():
    a, b = Side(M=M), Side(M=M, max_grad_norm=1e30)
    la = a.loop(4, 1, 2, first_draw=7)
    lb = b.learner.train(b.replay, 4, 1, 2, seed=UPDATE_SEED, first_draw=7)
    torch.cuda.synchronize(a.env.device)
    assert_same_losses(la, {k: lb[k] for k in ("critic_loss", "actor_loss", "ent_coef_loss")}, "huge bound")
    assert_same_state(a, b, "huge bound")  # every tensor bit for bit the twin's without the option
    assert (b.learner.clip_state["scale"] == 1.0).all() and a.learner.clip_state is None and "critic_grad_norm" not in a.learner.last_update
    assert "max_grad_norm" not in a.learner._saved_hp() and b.learner._saved_hp()["max_grad_norm"] == 1e30
    a.close(), b.close()


def test_save_and_load_continue_bit_for_bit(tmp_path):
    from test_checkpoint import Fresh, assert_same_side

    a, b = Side(M=M, **CLIPPED), Side(M=M, **CLIPPED)
    a.learner.train(a.replay, 6, 1, 2, seed=UPDATE_SEED, first_draw=7)
    b.learner.train(b.replay, 3, 1, 2, seed=UPDATE_SEED, first_draw=7)
    path = tmp_path / "run.npz"
    b.learner.save(path, replay=b.replay, extra=dict(update_draw=7 + b.learner.adam_state["step"]))
    b.close()
    one = Fresh(M=M)  # a learner without the option refuses the file, and nothing of it is written
    with pytest.raises(ValueError, match="max_grad_norm is 0.01 in the checkpoint, None here"):
        one.learner.load(path, replay=one.replay)
    # ... and its own checkpoint holds no new key and loads into a learner of this commit
    plain = tmp_path / "plain.npz"
    one.learner.collect(one.replay, 2)
    one.learner.save(plain, replay=one.replay)
    assert "max_grad_norm" not in one.learner.state_dict()["hp"] and not any("grad_norm" in k or "clip" in k for k in np.load(plain, allow_pickle=False).files)
    two = Fresh(M=M)
    two.learner.load(plain, replay=two.replay)
    one.close(), two.close()
    c = Fresh(M=M, **CLIPPED)
    extra = c.learner.load(path, replay=c.replay)
    c.learner.train(c.replay, 3, 1, 2, seed=UPDATE_SEED, first_draw=extra["update_draw"])
    torch.cuda.synchronize(a.env.device)
    assert_same_side(a, c, "3 + 3"), assert_same_clipped_last_update(a, c, "3 + 3")
    a.close(), c.close()


def test_the_option_needs_device_entropy_and_the_call_refuses_what_it_states():
    env = make_vec("UR5OriReach-v1", num_envs=N, seed=SEED, auto_reset=True)
    env.reset(seed=SEED)
    with pytest.raises(ValueError, match="max_grad_norm needs device_entropy=True"):
        SACLearner(env, seed=SEED, hidden_width=H, batch_size=M, max_grad_norm=1.0, **dict(ALL, device_entropy=False))
    env.close()
    s = Side(M=M, **CLIPPED)
    lr = s.learner
    lr.collect(s.replay, CAP)
    tr = lr._train_binding(s.replay)
    dev = s.env.device
    losses = torch.full((3, 2), NAN, device=dev)
    norms, scale = torch.full((2, 2), NAN, device=dev), torch.full((2,), NAN, device=dev)
    sched = dict(first_slot=s.replay.cursor, filled_steps=s.replay.filled, num_iterations=1, steps_per_iteration=0, updates_per_iteration=2, update_first_draw=3,
                 first_step=1)
    before = {k: bits(v).copy() for k, v in s.state().items()}

    def refused(what, expect, **clip):
        c = dict(dict(max_grad_norm=1.0, scale=scale, critic_grad_norm=norms[0], actor_grad_norm=norms[1]), **clip)
        with pytest.raises((NativeError, ValueError), match=expect):
            s.env.sac_train(tr["binding"], losses[0], losses[1], losses[2], clipping=c, **sched)

    refused("zero bound", "max_grad_norm", max_grad_norm=0.0)
    refused("NaN bound", "max_grad_norm", max_grad_norm=NAN)
    refused("short slots", "critic_grad_norm", critic_grad_norm=norms[0, :1])
    refused("scale of one", "scale", scale=scale[:1])
    lib, L = s.env.lib, tr["binding"].struct
    S = _abi.SacSchedule(s.replay.cursor, s.replay.filled, CAP, 1, 0, 2, 0, 0, 0, 3, 1)
    fptr = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float))  # noqa: E731
    for name, t in zip(_abi.SAC_LEARNER_LOSSES, losses):
        setattr(L, name, fptr(t))
    good = dict(max_grad_norm=1.0, reserved0=0, scale=fptr(scale), critic_grad_norm=fptr(norms[0]), actor_grad_norm=fptr(norms[1]))
    nstep = _abi.SacNstep(3, 0, fptr(scale), fptr(scale))
    her = _abi.SacHindsight(1 << 31, 0, 3, 0)
    for what, clip, extra, expect in (("null clipping", None, {}, b"null clipping"), ("reserved0", dict(good, reserved0=1), {}, b"reserved0"),
                                      ("infinite bound", dict(good, max_grad_norm=float("inf")), {}, b"max_grad_norm"), ("null scale", dict(good, scale=None), {}, b"scale is null"),
                                      ("null slots", dict(good, actor_grad_norm=None), {}, b"actor_grad_norm is null"),
                                      ("two gathers", good, dict(nstep=nstep, her=her), b"at most one")):
        rc = lib.urgym_sac_train_clipped(s.env._h, C.byref(L), C.byref(S), C.byref(_abi.SacClipping(**clip)) if clip else None,
                                         C.byref(extra["nstep"]) if "nstep" in extra else None, None, C.byref(extra["her"]) if "her" in extra else None, None, None, None)
        assert rc == _abi.ERR_ARG and expect in lib.urgym_last_error(s.env._h), (what, rc, lib.urgym_last_error(s.env._h))
    for name in _abi.SAC_LEARNER_LOSSES:
        setattr(L, name, None)
    torch.cuda.synchronize(dev)
    after = s.state()
    assert all(np.array_equal(before[k], bits(after[k])) for k in before)
    assert torch.isnan(losses).all() and torch.isnan(norms).all() and torch.isnan(scale).all()  # nothing was launched
    s.close()


def test_update_runs_no_torch_operation_that_launches():
    from torch.utils._python_dispatch import TorchDispatchMode

    class Recorder(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.append(str(func))
            return func(*args, **(kwargs or {}))

    s = Side(M=M, **CLIPPED)
    s.learner.collect(s.replay, CAP)
    s.learner.update(s.replay, UPDATE_SEED, 0)  # whatever is made lazily is made here
    with Recorder() as rec:
        s.learner.update(s.replay, UPDATE_SEED, 1)
    torch.cuda.synchronize(s.env.device)
    print(f"clipped update: {len(rec.names)} torch operations: {sorted(set(rec.names))}")
    assert rec.names and "aten.empty.memory_format" in rec.names and set(rec.names) <= ALLOCATIONS_AND_VIEWS, sorted(set(rec.names) - ALLOCATIONS_AND_VIEWS)
    s.close()
