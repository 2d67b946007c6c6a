"""GPU tests (-m gpu) of the SAC training loop in one native call: urgym_sac_train / env.sac_train /
SACLearner.train.

The call adds no kernel and no arithmetic, so everything is compared BIT FOR BIT with the route that exists: a second learner with the
same seed on a second environment with the same seed runs today's loop -- ``collect`` then ``update`` per iteration, with the learner's
rule for skipping updates -- and every ring tensor, bound buffer, parameter, moment, packed buffer, loss and ``last_update`` tensor must
be the same words.  Small shapes: N = 64 envs, H = 32, M = 64 rows, a ring of 4 slots, learning_starts = 128 (U = 2 uniform iterations,
I = 1 idle one at K = 1: the uniform-but-updating iteration is covered).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from sac_train_cases import REFUSED
from ur_gym_amd import _abi, make_vec
from ur_gym_amd._native import NativeError
from ur_gym_amd.evaluation import DeviceReplay, warmup_iterations
from ur_gym_amd.training import SACLearner

pytestmark = pytest.mark.gpu

ALL = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)
N, H, CAP, STARTS, SEED, UPDATE_SEED = 64, 32, 4, 128, 5, 11
GUARD, GUARD_WORD = 4, 0x7FC05AC0


def bits(t):
    """The bytes of a tensor or array on the host: a comparison of them is bitwise, NaNs and the sign of zero included."""
    if isinstance(t, torch.Tensor):
        t = t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy()
    return np.ascontiguousarray(t).view(np.uint8).reshape(-1)


class Side:
    """An environment, a learner on it and a ring, all made from the same seeds whichever side it is."""

    def __init__(self, env_id="UR5OriReach-v1", M=64, hidden=H, **over):
        self.env = make_vec(env_id, num_envs=N, seed=SEED, auto_reset=True)
        self.env.reset(seed=SEED)
        self.learner = SACLearner(self.env, seed=SEED, hidden_width=hidden, batch_size=M, learning_starts=STARTS, **dict(ALL, **over))
        self.replay = DeviceReplay(self.env, CAP)

    def loop(self, iterations, K, G, first_draw):
        """Today's loop (tools/train_sac.py's body).  Returns the losses of every update, copied as they were produced."""
        lr, losses, draw = self.learner, [], first_draw
        for _ in range(iterations):
            if K:
                lr.collect(self.replay, K)
            if lr.env_steps * N < lr.hp["learning_starts"]:
                continue
            for _ in range(G):
                got = lr.update(self.replay, UPDATE_SEED, draw)
                losses.append({k: v.clone() for k, v in got.items()})
                draw += 1
        return losses

    def state(self):
        """name -> tensor or array of everything a call may write, but the losses and last_update."""
        lr, out = self.learner, {}
        out.update({f"ring.{k}": v for k, v in self.replay.ring.items()})
        out.update({f"buf.{k}": v for k, v in self.env.buf.items()})
        st = lr.adam_state
        for kind, w in (("param", lr.actor.tensors()), ("moment:m", st["actor"][0]), ("moment:v", st["actor"][1]), ("grad", lr.actor_grads)):
            out.update({f"{kind}:actor.{k}": v for k, v in w.items()})
        for kind, nets in (("param", lr.critic.tensors()), ("moment:m", st["critic"][0]), ("moment:v", st["critic"][1]), ("grad", lr.critic_grads)):
            for i, w in enumerate(nets):
                out.update({f"{kind}:qf{i}.{k}": v for k, v in w.items()})
        es = lr.entropy_state
        out.update(log_ent_coef=lr.log_ent_coef, ent_m=es["exp_avg"], ent_v=es["exp_avg_sq"], ent_coef=es["ent_coef"])
        out.update({"packed.actor": lr.device_actor.packed(), "packed.online": lr.online.packed(), "packed.target": lr.target.packed()})
        return out

    def counters(self):
        lr = self.learner
        return dict(env_steps=lr.env_steps, draw=lr.draw, step=lr.adam_state["step"], cursor=self.replay.cursor, filled=self.replay.filled)

    def close(self):
        self.learner.close()
        self.env.close()


def assert_same_state(a, b, what):
    sa, sb = a.state(), b.state()
    assert sa.keys() == sb.keys()
    # every parameter tensor there is (8 of the actor, 2 x 6 of the twin critic) and their two moments each are among them
    assert sum(k.startswith("param:") for k in sa) == 8 + 12 and sum(k.startswith("moment:") for k in sa) == 2 * (8 + 12)
    for k in sa:
        assert np.array_equal(bits(sa[k]), bits(sb[k])), (what, k)
    assert a.counters() == b.counters(), (what, a.counters(), b.counters())


def assert_same_losses(python_losses, native, what):
    assert all(v.shape == (len(python_losses),) for v in native.values()), what
    for u, want in enumerate(python_losses):
        for k in ("critic_loss", "actor_loss", "ent_coef_loss"):
            assert np.array_equal(bits(native[k][u]), bits(want[k])), (what, u, k, float(native[k][u]), float(want[k]))


def assert_same_last_update(a, b, what):
    la, lb = a.learner.last_update, b.learner.last_update
    assert sorted(la) == sorted(lb) == ["dqmin_da", "log_prob", "q", "q_min", "y"]
    for k in la:
        assert la[k].shape == lb[k].shape and np.array_equal(bits(la[k]), bits(lb[k])), (what, k)


def compare_with_the_python_loop(env_id, M, iterations, K, G, prefill=0, what=""):
    a, b = Side(env_id, M), Side(env_id, M)
    for s in (a, b):  # a filled ring first, by the existing route on both sides
        if prefill:
            s.learner.collect(s.replay, prefill)
    want = a.loop(iterations, K, G, first_draw=7)
    got = b.learner.train(b.replay, iterations, K, G, seed=UPDATE_SEED, first_draw=7)
    torch.cuda.synchronize(a.env.device)
    assert len(want) > 0, "the case runs no update"
    assert_same_losses(want, got, what)
    assert_same_state(a, b, what)
    assert_same_last_update(a, b, what)
    assert np.isfinite(bits(got["critic_loss"]).view(np.float32)).all()
    a.close(), b.close()
    return len(want)


def test_one_call_equals_the_python_loop_bit_for_bit():
    U, I = warmup_iterations(0, N, STARTS, 6, 1)
    assert (U, I) == (2, 1)  # iteration 1 collects with uniform actions and updates
    assert compare_with_the_python_loop("UR5OriReach-v1", 64, 6, 1, 2, what="6 x (1 step, 2 updates)") == 10


def test_split_calls_equal_the_single_call():
    a, b = Side(), Side()
    one = a.learner.train(a.replay, 6, 1, 2, seed=UPDATE_SEED, first_draw=7)
    first = b.learner.train(b.replay, 2, 1, 2, seed=UPDATE_SEED, first_draw=7)  # no synchronisation between the two
    second = b.learner.train(b.replay, 4, 1, 2, seed=UPDATE_SEED, first_draw=7 + 2)
    torch.cuda.synchronize(a.env.device)
    assert first["critic_loss"].shape == (2,) and second["critic_loss"].shape == (8,)
    for k in one:
        assert np.array_equal(bits(one[k]), bits(torch.cat([first[k], second[k]]))), k
    assert_same_state(a, b, "2 + 4 iterations")
    assert_same_last_update(a, b, "2 + 4 iterations")
    a.close(), b.close()


@pytest.mark.parametrize("env_id,M,iterations,K,G,prefill", [
    ("UR5OriReach-v1", 64, 4, 2, 1, 0),   # K = 2, G = 1: U, I = 1, 0
    ("UR5OriReach-v1", 80, 4, 1, 2, 0),   # M no power of two and no multiple of 64
    ("UR5DynReach-v1", 64, 4, 1, 2, 0),   # other row widths, a moving obstacle
    ("UR5OriReach-v1", 64, 1, 0, 3, 4),   # three updates in one call on a filled ring, against three update() calls
], ids=["K2-G1", "M80", "Dyn", "K0-G3"])
def test_shapes_equal_the_python_loop(env_id, M, iterations, K, G, prefill):
    compare_with_the_python_loop(env_id, M, iterations, K, G, prefill, what=f"{env_id} M={M} {iterations} x ({K}, {G})")


def test_train_needs_device_entropy():
    s = Side(device_entropy=False)
    with pytest.raises(ValueError, match="device_entropy"):
        s.learner.train(s.replay, 1, 1, 1, seed=UPDATE_SEED, first_draw=0)
    s.close()


# ------------------------------------------------------------------------------------------------ hand-built structs: guards and refusals
def guarded(shape, dtype, device, fill=None):
    """(flat, view): `view` is a contiguous tensor of `shape` that starts GUARD words and one element into its own allocation `flat`
    and ends at least GUARD words before its end; every other byte of `flat` holds GUARD_WORD."""
    n, size = int(np.prod(shape)), torch.empty((), dtype=dtype).element_size()
    words = (n * size + 3) // 4 + 2 * GUARD + 2
    flat = torch.full((words,), GUARD_WORD, dtype=torch.int32, device=device)
    first = GUARD * (4 // size) + 1 if size <= 4 else (GUARD * 4) // size + 1
    view = flat.view(dtype)[first:first + n].view(shape)
    if fill is not None:
        view.fill_(fill)
    assert view.is_contiguous() and view.data_ptr() == flat.data_ptr() + first * size
    return flat, view


def guards_intact(pairs):
    for name, (flat, view) in pairs.items():
        b = flat.view(torch.uint8).cpu().numpy()
        want = np.full(flat.numel(), GUARD_WORD, dtype=np.int32).view(np.uint8)
        lo = view.data_ptr() - flat.data_ptr()
        hi = lo + view.numel() * view.element_size()
        if not (np.array_equal(b[:lo], want[:lo]) and np.array_equal(b[hi:], want[hi:])):
            return name
    return None


class HandBuilt:
    """A Side whose batch, scratch, temperature state and loss slots are guarded views, bound by env.sac_learner directly."""

    def __init__(self, updates, M=64, prefill=CAP):
        from ur_gym_amd.vector_env import _TORCH_DTYPE

        self.side = s = Side(M=M)
        env, lr, dev = s.env, s.learner, s.env.device
        if prefill:
            lr.collect(s.replay, prefill)
        self.g = g = {}
        for name, ct, shape, _ in _abi.REPLAY_RING_FIELDS:
            g[f"batch.{name}"] = guarded((M,) + tuple(shape(1, 1, env.obs_dim, env.goal_dim)[2:]), _TORCH_DTYPE[ct], dev, 0)
        g["batch.index"] = guarded((M,), torch.int64, dev, 0)
        for name, shape in _abi.SAC_LEARNER_SCRATCH:
            g[name] = guarded(shape(M), torch.float32, dev, 0.0)
        for name in _abi.SAC_LEARNER_STATE:
            g[name] = guarded((1,), torch.float32, dev, 0.0)
        for name in _abi.SAC_LEARNER_LOSSES:
            g[name] = guarded((updates,), torch.float32, dev, float("nan"))
        st, hp = lr.adam_state, lr.hp
        self.fields = dict(
            actor=lr.device_actor, online=lr.online, target=lr.target, actor_params=lr.actor.tensors(), actor_grads=lr.actor_grads,
            actor_exp_avg=st["actor"][0], actor_exp_avg_sq=st["actor"][1], critic_params=lr.critic.tensors(), critic_grads=lr.critic_grads,
            critic_exp_avg=st["critic"][0], critic_exp_avg_sq=st["critic"][1], actor_workspace=lr.actor_workspace, critic_workspace=lr.critic_workspace,
            log_ent_coef=g["log_ent_coef"][1], exp_avg=g["exp_avg"][1], exp_avg_sq=g["exp_avg_sq"][1], replay=s.replay,
            batch={k[6:]: v[1] for k, v in g.items() if k.startswith("batch.")}, scratch={n: g[n][1] for n, _ in _abi.SAC_LEARNER_SCRATCH}, count=M,
            seed=SEED, update_seed=UPDATE_SEED, gamma=hp["gamma"], tau=hp["tau"], target_entropy=hp["target_entropy"], lr=hp["learning_rate"])
        self.binding = env.sac_learner(**self.fields)
        self.losses = [g[n][1] for n in _abi.SAC_LEARNER_LOSSES]

    def everything(self):
        """One uint8 device tensor of every byte a call may write: the Side's state and the guarded allocations whole."""
        parts = [v for v in self.side.state().values()] + [flat for flat, _ in self.g.values()]
        return torch.cat([(torch.from_numpy(np.ascontiguousarray(p)).to(self.side.env.device) if isinstance(p, np.ndarray) else p.detach().contiguous())
                          .view(torch.uint8).reshape(-1) for p in parts])

    def close(self):
        self.side.close()


def test_no_stray_writes_and_every_loss_slot_once():
    K, G, n = 1, 2, 2
    hb = HandBuilt(updates=n * G, prefill=2)  # cursor 2, two slots filled: the call's steps go to slots 2 and 3
    s, env = hb.side, hb.side.env
    ring_before = {k: v.clone() for k, v in s.replay.ring.items()}
    assert s.replay.cursor == 2 and torch.isnan(torch.stack(hb.losses)).all()
    done = env.sac_train(hb.binding, *hb.losses, first_slot=2, filled_steps=2, num_iterations=n, steps_per_iteration=K, updates_per_iteration=G,
                         uniform_iterations=0, idle_iterations=0, collect_first_draw=s.learner.draw, update_first_draw=3, first_step=1)
    torch.cuda.synchronize(env.device)
    assert done == 4 and guards_intact(hb.g) is None, guards_intact(hb.g)
    for k, v in s.replay.ring.items():  # slots outside the call's steps are untouched, the call's own are written
        assert torch.equal(v[:2], ring_before[k][:2]), k
    assert not torch.equal(s.replay.ring["observation"][2:], ring_before["observation"][2:])
    losses = torch.stack(hb.losses).cpu().numpy()
    assert np.isfinite(losses).all()  # every slot written ...
    # ... and by its own update: slot u holds the bits of update u of the Python loop on a second side
    ref = Side()
    ref.learner.collect(ref.replay, 2)
    ref.learner.env_steps = STARTS  # past the warm-up, as the hand-built schedule says (U = I = 0)
    want = ref.loop(n, K, G, first_draw=3)
    torch.cuda.synchronize(env.device)
    for u, w in enumerate(want):
        for row, k in zip(losses, _abi.SAC_LEARNER_LOSSES):
            assert np.array_equal(bits(row[u]), bits(w[k])), (u, k)
    ref.close(), hb.close()


def pointer_paths(struct, prefix=""):
    """Every pointer field of a ctypes struct, nested structs and arrays of structs walked: (path, owner, field name)."""
    for name, kind in struct._fields_:
        value = getattr(struct, name)
        if isinstance(value, C.Structure):
            yield from pointer_paths(value, f"{prefix}{name}.")
        elif isinstance(value, C.Array):
            for i, item in enumerate(value):
                yield from pointer_paths(item, f"{prefix}{name}[{i}].")
        elif kind is C.c_void_p or issubclass(kind, C._Pointer):
            yield f"{prefix}{name}", struct, name


def test_refusals_launch_nothing_and_write_nothing():
    hb = HandBuilt(updates=4)
    s, env, lib = hb.side, hb.side.env, hb.side.env.lib
    other = Side()  # objects of another handle
    L = hb.binding.struct
    for name, t in zip(_abi.SAC_LEARNER_LOSSES, hb.losses):
        setattr(L, name, C.cast(t.data_ptr(), C.POINTER(C.c_float)))
    ok = dict(first_slot=0, filled_steps=CAP, capacity_steps=CAP, num_iterations=2, steps_per_iteration=1, updates_per_iteration=2,
              uniform_iterations=1, idle_iterations=0, collect_first_draw=0, update_first_draw=0, first_step=1)
    before = hb.everything()
    refused = []

    def call(learner, **sched):
        S = _abi.SacSchedule(*[dict(ok, **sched)[n] for n, _ in _abi.SacSchedule._fields_])
        rc = lib.urgym_sac_train(env._h, C.byref(learner) if learner is not None else None, C.byref(S), env._stream())
        return rc, lib.urgym_last_error(env._h).decode()

    def refuse(what, learner, expect=None, **sched):
        rc, msg = call(learner, **sched)
        assert rc == _abi.ERR_ARG and msg.startswith("urgym_sac_train: "), (what, rc, msg)
        assert expect is None or expect in msg, (what, msg)
        refused.append(what)

    def edited(**fields):
        c = _abi.SacLearner.from_buffer_copy(L)
        for k, v in fields.items():
            *inner, field = k.split(".")
            owner = c
            for p in inner:
                owner = getattr(owner, p)
            setattr(owner, field, v)
        return c

    # every pointer field to NULL in turn, but the three documented optional ones
    paths = list(pointer_paths(L))
    assert len(paths) == 3 + 32 + 48 + 2 + 3 + 11 + 12 + 12 + 3, len(paths)
    for path, _, _ in paths:
        c = _abi.SacLearner.from_buffer_copy(L)
        owner = c
        *inner, field = path.replace("]", "").replace("[", ".").split(".")
        for p in inner:
            owner = owner[int(p)] if p.isdigit() else getattr(owner, p)
        setattr(owner, field, None)
        if path in _abi.SAC_LEARNER_OPTIONAL:
            continue
        refuse(f"{path} = NULL", c)
    assert lib.urgym_sac_train(env._h, None, C.byref(_abi.SacSchedule()), env._stream()) == _abi.ERR_ARG
    assert lib.urgym_sac_train(env._h, C.byref(L), None, env._stream()) == _abi.ERR_ARG
    # the schedule's refusals (sac_train_cases.REFUSED, at this ring's capacity) and a capacity that is not the ring's
    for what, sched in REFUSED.items():
        refuse(what, L, **{k: v for k, v in sched.items() if k != "capacity_steps" or v != CAP})
    refuse("capacity of another ring", L, "ring.capacity_steps", capacity_steps=CAP + 1, first_slot=0)
    # objects
    o = other.learner
    refuse("actor of another handle", edited(actor=o.device_actor._a), "not an actor of this handle")
    refuse("online of another handle", edited(online=o.online._c), "not a critic of this handle")
    refuse("target of another handle", edited(target=o.target._c))
    refuse("online == target", edited(target=L.online), "the online critic itself")
    # numbers
    for count in (0, 65537, -1):
        refuse(f"count = {count}", edited(count=count))
    refuse("critic workspace one byte short", edited(critic_workspace_bytes=L.critic_workspace_bytes - 1), "workspace is smaller")
    refuse("actor workspace one byte short", edited(actor_workspace_bytes=L.actor_workspace_bytes - 1), "workspace is smaller")
    refuse("reserved0", edited(reserved0=1), "reserved0")
    refuse("actor_adam.reserved0", edited(**{"actor_adam.reserved0": 1}), "reserved0")
    refuse("critic_adam.reserved0", edited(**{"critic_adam.reserved0": 1}), "reserved0")
    refuse("ring.reserved0", edited(**{"ring.reserved0": 1}), "reserved0")
    refuse("actor_adam.hidden_width", edited(**{"actor_adam.hidden_width": H + 32}))
    refuse("critic_adam.in_features", edited(**{"critic_adam.in_features": 1}))
    for name in ("gamma", "target_entropy"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            refuse(f"{name} = {bad}", edited(**{name: bad}), name)
    for bad in (float("nan"), float("inf"), 0.0, -0.5, 1.5):
        refuse(f"tau = {bad}", edited(tau=bad), "tau")
    for name, bads in (("lr", (float("nan"), float("inf"), -1e-4)), ("beta1", (1.0, -0.1, float("nan"))), ("beta2", (1.0, -0.1)),
                       ("eps", (0.0, -1e-8, float("inf"), float("nan")))):
        for bad in bads:
            refuse(f"{name} = {bad}", edited(**{name: bad}))
    # a ring that cannot serve an update: nothing in it and nothing collected first
    refuse("an empty ring", L, "empty ring", filled_steps=0, steps_per_iteration=0)
    # nothing was launched: every state, ring and output byte is what it was, guards and NaN-filled loss slots included
    torch.cuda.synchronize(env.device)
    assert torch.equal(hb.everything(), before) and torch.isnan(torch.stack(hb.losses)).all()
    assert len(refused) > 150, len(refused)

    # an actor without the log_std head, and a learner at H = 288, above the gradient kernels' width cap, on the same handle
    from ur_gym_amd.evaluation import ACTOR_ARRAYS, DeviceActor, DeviceCritic
    from ur_gym_amd.training import TorchActor, TorchTwinCritic, host_arrays

    bare = DeviceActor({k: v for k, v in host_arrays(s.learner.actor.tensors()).items() if k in ACTOR_ARRAYS}, env)
    assert not bare.has_log_std
    refuse("an actor without the log_std head", edited(actor=bare._a), "log_std head")
    bare.close()
    n_in = env.obs_dim + 2 * env.goal_dim
    wa, wc = TorchActor(n_in, 288).to(env.device), TorchTwinCritic(n_in + 6, 288).to(env.device)
    wide = dict(actor=DeviceActor(host_arrays(wa.tensors()), env), online=DeviceCritic(host_arrays(wc.tensors()), env),
                target=DeviceCritic(host_arrays(wc.tensors()), env))
    zeros = lambda w: {k: torch.zeros_like(v) for k, v in w.items()}  # noqa: E731
    wide.update(actor_params=wa.tensors(), critic_params=wc.tensors())
    wide.update({f"actor_{k}": zeros(wa.tensors()) for k in ("grads", "exp_avg", "exp_avg_sq")})
    wide.update({f"critic_{k}": [zeros(w) for w in wc.tensors()] for k in ("grads", "exp_avg", "exp_avg_sq")})
    wide_binding = env.sac_learner(**dict(hb.fields, **wide))
    with pytest.raises(NativeError, match="hidden widths up to 256"):
        env.sac_train(wide_binding, *hb.losses, first_slot=0, filled_steps=CAP, num_iterations=2, updates_per_iteration=2)
    for k in ("actor", "online", "target"):
        wide[k].close()
    torch.cuda.synchronize(env.device)
    assert torch.equal(hb.everything(), before)

    # the Python layer's own checks: ValueError before the library is called
    lr, good = s.learner, dict(first_slot=0, filled_steps=CAP, num_iterations=1)
    with pytest.raises(ValueError, match="critic_loss"):
        env.sac_train(hb.binding, hb.losses[0][:1], hb.losses[1], hb.losses[2], updates_per_iteration=4, **good)  # one entry per update
    with pytest.raises(ValueError, match="actor_loss"):
        env.sac_train(hb.binding, hb.losses[0], hb.losses[1].double(), hb.losses[2], updates_per_iteration=4, **good)  # nothing is converted
    with pytest.raises(ValueError, match="ent_coef_loss"):
        env.sac_train(hb.binding, hb.losses[0], hb.losses[1], torch.zeros(8, device=env.device)[::2], updates_per_iteration=4, **good)
    with pytest.raises(ValueError, match="integer"):
        env.sac_train(hb.binding, *hb.losses, updates_per_iteration=4, **dict(good, num_iterations=1.5))
    with pytest.raises(ValueError, match="sac_learner"):
        env.sac_train(other.learner._train_binding(other.replay)["binding"], *hb.losses, updates_per_iteration=4, **good)
    fields = hb.fields
    env.sac_learner(**fields)  # accepted as it stands
    no_reward = {k: v for k, v in fields["batch"].items() if k != "reward"}
    for bad, match in ((dict(target=lr.online), "online critic itself"), (dict(online=other.learner.online), "online"), (dict(replay=other.replay), "replay"),
                       (dict(count=0), "count"), (dict(count=65537), "count"), (dict(tau=0.0), "tau"), (dict(gamma=float("nan")), "gamma"),
                       (dict(batch=no_reward), "reward"), (dict(batch=dict(fields["batch"], reward=fields["batch"]["reward"].double())), "reward"),
                       (dict(scratch=dict(fields["scratch"], q=fields["scratch"]["q_min"])), "q"), (dict(exp_avg=torch.zeros(2, device=env.device)), "exp_avg"),
                       (dict(actor_workspace=lr.actor_workspace.double()), "actor_workspace"), (dict(actor=other.learner.device_actor), "actor"),
                       (dict(betas=(0.9,)), "betas")):
        with pytest.raises(ValueError, match=match):
            env.sac_learner(**dict(fields, **bad))
    torch.cuda.synchronize(env.device)
    assert torch.equal(hb.everything(), before)
    other.close(), hb.close()


def test_refusals_of_the_evaluation_and_monitoring_halves_carry_the_callers_name():
    """Each of the five entry points that take their evaluation and monitoring as options, with its own required option valid: an
    evaluation without a handle, and a monitoring with reserved0 set, are refused under that entry point's name, with nothing launched."""
    from ur_gym_amd.evaluation import DeviceMonitor, DeviceNormalizer, DevicePrioritizedReplay, _her_arguments, relabel_threshold

    hb = HandBuilt(updates=4)
    s, env, lib, dev = hb.side, hb.side.env, hb.side.env.lib, hb.side.env.device
    L, M = hb.binding.struct, 64
    fp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float))  # noqa: E731
    for name, t in zip(_abi.SAC_LEARNER_LOSSES, hb.losses):
        setattr(L, name, fp(t))
    S = _abi.SacSchedule(first_slot=0, filled_steps=CAP, capacity_steps=CAP, num_iterations=2, steps_per_iteration=1, updates_per_iteration=2,
                         uniform_iterations=1, idle_iterations=0, collect_first_draw=0, update_first_draw=0, first_step=1)
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)  # noqa: E731
    # the options' own scratch and outputs, and the learner's: NaN before every call, NaN after it
    scratch = dict(discount=nan(M), q_min_next=nan(M), scale=nan(2), critic_grad_norm=nan(4), actor_grad_norm=nan(4))
    scratch.update({f"per.{name}": nan(*shape(M)) for name, shape in _abi.SAC_PRIORITIZED_SCRATCH})
    scratch.update({name: hb.g[name][1] for name, _ in _abi.SAC_LEARNER_SCRATCH})
    scratch.update(zip(_abi.SAC_LEARNER_LOSSES, hb.losses))
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    pri = DevicePrioritizedReplay(env, CAP)  # for its priorities alone: the ring is the learner's
    normalizer, monitor = DeviceNormalizer(env), DeviceMonitor(env)
    nstep = _abi.SacNstep(3, 0, fp(scratch["discount"]), fp(scratch["q_min_next"]))
    prioritized = _abi.SacPrioritized(priorities=pri.priorities_struct(), beta0=0.4, beta_steps=7, alpha=pri.alpha, eps=pri.eps,
                                      total=C.cast(total.data_ptr(), C.POINTER(C.c_double)),
                                      **{name: fp(scratch[f"per.{name}"]) for name, _ in _abi.SAC_PRIORITIZED_SCRATCH})
    hindsight = _abi.SacHindsight(*_her_arguments(relabel_threshold(4), "future", 3), 0)
    clipping = _abi.SacClipping(1.0, 0, fp(scratch["scale"]), fp(scratch["critic_grad_norm"]), fp(scratch["actor_grad_norm"]))
    normalization = env._normalization("test", normalizer)
    b = C.byref
    calls = {  # entry point -> the call with its own option given and the evaluation and monitoring passed through
        "urgym_sac_train_nstep": lambda E, Mo: lib.urgym_sac_train_nstep(env._h, b(L), b(S), b(nstep), E, Mo, env._stream()),
        "urgym_sac_train_prioritized": lambda E, Mo: lib.urgym_sac_train_prioritized(env._h, b(L), b(S), b(prioritized), E, Mo, env._stream()),
        "urgym_sac_train_hindsight": lambda E, Mo: lib.urgym_sac_train_hindsight(env._h, b(L), b(S), b(hindsight), E, Mo, env._stream()),
        "urgym_sac_train_clipped": lambda E, Mo: lib.urgym_sac_train_clipped(env._h, b(L), b(S), b(clipping), None, None, None, E, Mo, env._stream()),
        "urgym_sac_train_normalized": lambda E, Mo: lib.urgym_sac_train_normalized(env._h, b(L), b(S), b(normalization), None, None, None, None, E, Mo, env._stream()),
    }
    no_handle = _abi.SacEvaluation()  # eval_handle is NULL
    reserved = _abi.SacMonitoring.from_buffer_copy(monitor.struct(1))
    reserved.reserved0 = 1
    for who, call in calls.items():
        for what, E, Mo, expect in (("evaluation", b(no_handle), None, "eval_handle is null"), ("monitoring", None, b(reserved), "urgym_sac_monitoring.reserved0")):
            for t in scratch.values():
                t.fill_(float("nan"))
            torch.cuda.synchronize(dev)
            before = hb.everything()
            rc = call(E, Mo)
            msg = lib.urgym_last_error(env._h).decode()
            assert rc == _abi.ERR_ARG and msg.startswith(who + ": ") and expect in msg, (who, what, rc, msg)
            torch.cuda.synchronize(dev)
            assert torch.equal(hb.everything(), before), (who, what)
            assert all(torch.isnan(t).all() for t in scratch.values()), (who, what)
    for name in _abi.SAC_LEARNER_LOSSES:
        setattr(L, name, None)
    hb.close()


# names of operations that allocate or make a view: nothing among them launches a kernel (test_sac_terms.py's list, restated)
ALLOCATIONS_AND_VIEWS = {"aten.empty.memory_format", "aten.empty_strided.default", "aten.view.default", "aten.view.dtype", "aten._unsafe_view.default",
                         "aten.select.int", "aten.slice.Tensor", "aten.squeeze.dim", "aten.unsqueeze.default", "aten.expand.default",
                         "aten.as_strided.default", "aten.alias.default", "aten.detach.default"}


def test_train_runs_no_torch_operation_that_launches():
    from torch.utils._python_dispatch import TorchDispatchMode

    class Recorder(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.append(str(func))
            return func(*args, **(kwargs or {}))

    s = Side()
    s.learner.train(s.replay, 3, 1, 2, seed=UPDATE_SEED, first_draw=0)  # warms: the scratch and the struct exist afterwards
    with Recorder() as rec:
        losses = s.learner.train(s.replay, 2, 1, 2, seed=UPDATE_SEED, first_draw=4)
    torch.cuda.synchronize(s.env.device)
    print(f"{len(rec.names)} torch operations in one train call of 2 x (1 step, 2 updates): {sorted(set(rec.names))}")
    assert losses["critic_loss"].shape == (4,) and "aten.empty.memory_format" in rec.names  # the recorder sees the allocation of the losses
    assert set(rec.names) <= ALLOCATIONS_AND_VIEWS, sorted(set(rec.names) - ALLOCATIONS_AND_VIEWS)
    assert len(rec.names) <= 8  # and their number does not grow with the updates
    s.close()
