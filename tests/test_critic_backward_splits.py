"""The parameter gradients of the twin critics past two splits of the rows, up to the row cap.

urgym_critic_parameter_gradients runs stage 2 once per split of 1024 rows above 1024 rows and adds the splits in float64 in a third
launch.  tests/test_critic_backward.py reaches one and two splits; this file reaches 3, 5 and 64, the cap of 65,536 rows, the padded
hidden widths (H = 32 in HP = 128, H = 160 in HP = 256) with old contents in the workspace and with guard words, and the learner's
two untested combinations of options.  The helpers are test_critic_backward.py's.

Where the checks come from (no number is taken from what the kernels give):
  * the exact network of test_critic_backward.py at these counts: the largest sum of absolute terms over any output element is
    computed from the float64 pass and asserted below 2^24 units for every case the device runs, so every partial sum in any order is
    a float32 number, a float64 sum of float32 partial sums rounded once is exact, and float64 and the device agree BITWISE.
  * that a mistake in the splits would show: the float64 gradients per split, and five wrong ways of putting them together, each
    shown to differ from the right one in every tensor it can touch.  The last row of every batch has dq != 0 in both networks and
    a live neuron in each hidden layer (set where the seed does not give it, asserted always), so a lost one-row split shows.
  * the checkpoint at five splits: within 4 x numpy float32's deviation from float64 per tensor, the project's rule for a second
    float32 order (test_critic_backward.py).
  * the learner: within 4 x the default route's deviation from float64 autograd plus one float32 ulp of the tensor's largest
    gradient, test_learner_critic_gradients's bound.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_critic_backward import (DQ_UNIT, GRID, SPLIT, _all_same, _dev, _env, _raw, _rows, _same, assert_exact, bits_equal, checkpoint_case,
                                  exact_critic, exact_dq, exact_inputs, exact_target, forward_f64, gradients_f64, split)
from ur_gym_amd import _abi
from ur_gym_amd.evaluation import CRITIC_ARRAYS, DeviceCritic, TwinCritic

CAP = _abi.CRITIC_GRADIENTS_MAX_COUNT
# a last split of one row; all splits full; a partial last split of 14 row groups, the last of them partial; 64 splits with a one-row
# tail; the cap
MANY_COUNTS = (2 * SPLIT + 1, 3 * SPLIT, 4 * SPLIT + 417)
CAP_COUNTS = (63 * SPLIT + 1, CAP)
COUNTS = MANY_COUNTS + CAP_COUNTS
MANY_CASES = [(kind, H) for kind in ("dyn", "ori") for H in (32, 160, 256)]  # the HT = 4 instance, HT = 8 padded, HT = 8 full
CAP_CASES = [(H, n) for H in (32, 256) for n in CAP_COUNTS]
OLD_CASES = [(H, n) for H in (32, 160) for n in (417, 2 * SPLIT + 1)]  # padded widths, one split and three
STRAY_CASES = [(160, 2 * SPLIT + 1), (160, 417)]
SCALE = 2.0 ** -3
CAP_BYTES = 592970240  # include/urgym.h: the workspace at in_features = 53, H = 256, 65,536 rows


def splits_of(n):
    return (n + SPLIT - 1) // SPLIT


def live_tail(nets, x, dq):
    """Whether the last row counts in every tensor's sum: dq != 0 in both networks, a live neuron in each hidden layer of both."""
    for i, w in enumerate(nets):
        z1, z2, _ = forward_f64(w, x[-1:])
        if dq[i][-1] == 0.0 or not (z1 > 0.0).any() or not (z2 > 0.0).any():
            return False
    return True


@functools.lru_cache(maxsize=None)
def dq_case(kind, H, n):
    """The exact network on n exact rows with dq given: built once per (kind, H, n), shared by the tests, which leave it as it is."""
    nets, x, dq = exact_critic(kind, H), exact_inputs(kind, n), exact_dq(kind, n)
    for i in (0, 1):  # a one-row tail that adds nothing would hide a lost split
        if dq[i, -1] == 0.0:
            dq[i, -1] = (1 - 2 * i) * DQ_UNIT
    assert live_tail(nets, x, dq), (kind, H, n)
    refs, worst = assert_exact(nets, x, dq, DQ_UNIT)
    q64 = np.stack([forward_f64(w, x)[2] for w in nets])
    return (dict(nets=nets, x=x, dq=dq, refs=refs, worst=worst, q64=q64))


@functools.lru_cache(maxsize=None)
def target_case(kind, H, n):
    """The same in the target form (test_critic_backward.py: exact_target), dq = (q - y) 2^-3.  The rows are the n of 16 n candidates on
    which q_0 and q_1 lie closest: of 4 n, as at the counts up to 1025, the sums pass 2^24 units at H = 160 and 4513 rows."""
    nets = exact_critic(kind, H)
    x, y, q64, dq = exact_target(nets, kind, H, n, SCALE, live_tail=True, pool=16)
    assert live_tail(nets, x, dq), (kind, H, n)
    refs, worst = assert_exact(nets, x, dq, GRID * SCALE)
    return (dict(nets=nets, x=x, y=y, dq=dq, refs=refs, worst=worst, q64=q64))


def nonzero_everywhere(refs):
    return all((refs[i][k] != 0.0).any() for i in (0, 1) for k in CRITIC_ARRAYS)


# ------------------------------------------------------------------------------------------------ CPU
def device_cases():
    """Every (kind, H, count) the device tests below run in the dq form, per (kind, H)."""
    todo = {}
    for kind, H in MANY_CASES:
        todo.setdefault((kind, H), []).extend(MANY_COUNTS)
    for H, n in CAP_CASES + OLD_CASES + STRAY_CASES:
        if n not in todo.setdefault(("dyn", H), []):
            todo[("dyn", H)].append(n)
    return todo


@pytest.mark.parametrize("kind,H", list(device_cases()), ids=[f"{k}-{H}" for k, H in device_cases()])
def test_inputs_are_exact_at_these_counts(kind, H):
    for n in device_cases()[(kind, H)]:
        case = dq_case(kind, H, n)
        print(f"{kind} H={H} count={n} splits={splits_of(n)} dq form: largest sum of absolute terms {case['worst']:.4g} units (2^24 = {2.0 ** 24:.4g})")
        assert case["worst"] < 2.0 ** 24 and nonzero_everywhere(case["refs"])
        if (kind, H) in MANY_CASES and n in MANY_COUNTS:
            case = target_case(kind, H, n)
            print(f"{kind} H={H} count={n} splits={splits_of(n)} target form: largest sum of absolute terms {case['worst']:.4g} units")
            assert case["worst"] < 2.0 ** 24 and nonzero_everywhere(case["refs"])


def _add(parts):
    return {k: sum(p[k] for p in parts) for k in CRITIC_ARRAYS}


def _differing(a, b):
    return [k for k in CRITIC_ARRAYS if not np.array_equal(a[k], b[k])]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("H", (32, 256))
def test_split_mistakes_would_show(H, n):
    """The float64 gradients per split of 1024 rows add up to the whole (exactly: every term is a multiple of one unit), and five wrong
    ways of adding them differ from it in all six tensors of both networks."""
    case = dq_case("dyn", H, n)
    nets, x, dq, S = case["nets"], case["x"], case["dq"], splits_of(n)
    bounds = [(s * SPLIT, min(n, (s + 1) * SPLIT)) for s in range(S)]
    assert S >= 3 and bounds[-1][1] == n and bounds[-1][1] - bounds[-1][0] == (n - 1) % SPLIT + 1
    # part[i][s]: the float64 gradients of network i on the rows of split s
    part = [[gradients_f64(nets[i], x[a:b], dq[i][a:b]) for a, b in bounds] for i in (0, 1)]
    last_group = (n // 32 * 32, n)  # the partial last row group; empty where the count is a multiple of 32
    for i in (0, 1):
        whole = case["refs"][i]
        assert _differing(_add(part[i]), whole) == []
        wrong = {"last split dropped": _add(part[i][:-1]),
                 "only splits 0 and 1 added": _add(part[i][:2]),
                 "split s >= 2 from the rows of split s - 1": _add(part[i][:2] + part[i][1:S - 1]),
                 "networks exchanged from split 2 on": _add(part[i][:2] + part[1 - i][2:])}
        if n % 32:
            tail = gradients_f64(nets[i], x[last_group[0]:], dq[i][last_group[0]:])
            wrong["last partial row group dropped"] = {k: whole[k] - tail[k] for k in CRITIC_ARRAYS}
        else:  # 3 SPLIT and the cap end on a full row group: this mistake has nothing to drop there and touches no tensor
            assert n in (3 * SPLIT, CAP)
        for label, bad in wrong.items():
            differs = _differing(bad, whole)
            print(f"dyn H={H} count={n} qf{i} '{label}': differs in {len(differs)} of {len(CRITIC_ARRAYS)} tensors")
            assert differs == list(CRITIC_ARRAYS), (H, n, i, label, differs)


# ------------------------------------------------------------------------------------------------ GPU
def _assert_bitwise(res, refs, q64, tag):
    assert bits_equal(res["q"].cpu().numpy(), q64), tag
    for i in (0, 1):
        for key in CRITIC_ARRAYS:
            assert bits_equal(res["grads"][i][key].cpu().numpy(), refs[i][key]), tag + (i, key)


def _filled_out(critic, fill):
    import torch

    n, H = critic.in_features, critic.hidden_width
    shapes = dict(zip(CRITIC_ARRAYS, ((H, n), (H,), (H, H), (H,), (1, H), (1,))))
    return [{k: torch.full(sh, fill, dtype=torch.float32, device="cuda:0") for k, sh in shapes.items()} for _ in range(2)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,H", MANY_CASES, ids=[f"{k}-{H}" for k, H in MANY_CASES])
def test_exact_network_many_splits_on_the_device(kind, H):
    import torch

    env = _env(kind, 8)
    critic = DeviceCritic(exact_critic(kind, H), env)
    for n in MANY_COUNTS:
        by_dq, by_target = dq_case(kind, H, n), target_case(kind, H, n)
        assert nonzero_everywhere(by_dq["refs"]) and nonzero_everywhere(by_target["refs"])
        rows, act = _rows(kind, by_dq["x"])
        got = env.critic_parameter_gradients(critic, act, dq=_dev(by_dq["dq"]), rows=rows)
        rows_t, act_t = _rows(kind, by_target["x"])
        got_t = env.critic_parameter_gradients(critic, act_t, target=_dev(by_target["y"]), scale=SCALE, rows=rows_t)
        torch.cuda.synchronize()
        _assert_bitwise(got, by_dq["refs"], by_dq["q64"], (kind, H, n, "dq"))
        _assert_bitwise(got_t, by_target["refs"], by_target["q64"], (kind, H, n, "target"))
        print(f"{kind} H={H} count={n} splits={splits_of(n)}: worst sum {by_dq['worst']:.4g} (dq form), {by_target['worst']:.4g} (target form) of 2^24 = "
              f"{2.0 ** 24:.4g} units; q and twelve tensors bitwise float64 in both forms")
    critic.close()
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,n", CAP_CASES, ids=[f"dyn-{H}-{n}" for H, n in CAP_CASES])
def test_exact_network_at_the_cap_on_the_device(H, n):
    import torch

    case = dq_case("dyn", H, n)
    assert splits_of(n) == 64 and nonzero_everywhere(case["refs"])
    env = _env("dyn", 8)
    critic = DeviceCritic(case["nets"], env)
    rows, act = _rows("dyn", case["x"])
    dq = _dev(case["dq"])
    got = env.critic_parameter_gradients(critic, act, dq=dq, rows=rows)
    torch.cuda.synchronize()
    _assert_bitwise(got, case["refs"], case["q64"], ("dyn", H, n))
    print(f"dyn H={H} count={n} splits=64: worst sum {case['worst']:.4g} of 2^24 = {2.0 ** 24:.4g} units; q and twelve tensors bitwise float64")
    if (H, n) == (256, CAP):
        size = C.c_uint64()
        assert env.lib.urgym_critic_parameter_gradients_workspace(env._h, critic._c, n, C.byref(size)) == 0 and size.value == CAP_BYTES
        assert _all_same(env.critic_parameter_gradients(critic, act, dq=dq, rows=rows), got)
        ws = env.critic_gradient_workspace(critic, n)
        assert ws.numel() * 4 == CAP_BYTES
        ws.fill_(float("nan"))
        out = _filled_out(critic, float("nan"))
        again = env.critic_parameter_gradients(critic, act, dq=dq, rows=rows, out=out, workspace=ws)
        torch.cuda.synchronize()
        assert again["grads"] is out and _all_same(again, got)
        assert bool(torch.isfinite(again["q"]).all()) and all(bool(torch.isfinite(out[i][k]).all()) for i in (0, 1) for k in CRITIC_ARRAYS)
        print(f"dyn H=256 count={n}: workspace {size.value:,} bytes; a second call and a call on NaN-filled workspace and outputs give the same bits")
    critic.close()
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,n", OLD_CASES, ids=[f"dyn-{H}-{n}" for H, n in OLD_CASES])
def test_old_contents_at_padded_widths(H, n):
    """Stage 2 reads the padded neurons H .. HP - 1 of the workspace's arrays; what lay in the workspace and the outputs before the
    call reaches no result."""
    import torch

    case = dq_case("dyn", H, n)
    env = _env("dyn", 8)
    critic = DeviceCritic(case["nets"], env)
    assert critic.hidden_width == H and H % 128 != 0
    rows, act = _rows("dyn", case["x"])
    dq = _dev(case["dq"])
    results = []
    for fill in (float("nan"), 0.0):
        ws = env.critic_gradient_workspace(critic, n)
        ws.fill_(fill)
        out = _filled_out(critic, fill)
        results.append(env.critic_parameter_gradients(critic, act, dq=dq, rows=rows, out=out, workspace=ws))
        assert results[-1]["grads"] is out
    results.append(env.critic_parameter_gradients(critic, act, dq=dq, rows=rows))  # freshly allocated
    torch.cuda.synchronize()
    assert _all_same(results[0], results[1]) and _all_same(results[0], results[2])
    for res in results:
        _assert_bitwise(res, case["refs"], case["q64"], ("dyn", H, n))
    print(f"dyn H={H} count={n} splits={splits_of(n)}: NaN-filled, zero-filled and fresh workspace and outputs agree, bitwise float64")
    critic.close()
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,m", STRAY_CASES, ids=[f"dyn-{H}-{m}" for H, m in STRAY_CASES])
def test_no_stray_writes_at_a_padded_width(H, m):
    import torch

    case = dq_case("dyn", H, m)
    env = _env("dyn", 8)
    critic = DeviceCritic(case["nets"], env)
    rows, act = _rows("dyn", case["x"])
    d = _dev(case["dq"])
    r = _raw(dict(env=env, critic=critic, rows=rows, act=act), m, with_q=False)
    pad, fill = r["pad"], r["fill"]
    assert r["need"] == 4 * _floats(critic.in_features, H, m)
    rc = env.lib.urgym_critic_parameter_gradients(env._h, critic._c, C.byref(r["cr"]), m, C.c_void_p(d.data_ptr()), None, 0.0, C.byref(r["out"]),
                                                  C.c_void_p(r["ws"][pad:].data_ptr()), r["need"], env._stream())
    assert rc == 0, env.lib.urgym_last_error(env._h)
    want = env.critic_parameter_gradients(critic, act, dq=d, rows=rows)
    torch.cuda.synchronize()
    assert bool((r["q"] == fill).all())  # q is not written when NULL
    assert bool((r["ws"][:pad] == fill).all()) and bool((r["ws"][pad + r["need"] // 4:] == fill).all())
    for i in (0, 1):
        for k, size in r["sizes"].items():
            t = r["big"][i][k]
            assert bool((t[:pad] == fill).all()) and bool((t[pad + size:] == fill).all()), (i, k)
            assert _same(t[pad:pad + size], want["grads"][i][k].reshape(-1)), (i, k)
    _assert_bitwise(want, case["refs"], case["q64"], ("dyn", H, m))
    critic.close()
    env.close()


def _floats(n_in, H, count):
    """The workspace in floats as urgym_backward_map.h lays it out: four arrays per network, x, dq, the partial sums above one split."""
    HP, RG, S = (H + 127) // 128 * 128, (count + 31) // 32, splits_of(count)
    P = H * n_in + H * H + 3 * H + 1
    return 2 * 4 * RG * HP * 32 + RG * 56 * 32 + 2 * RG * 32 + (S * 2 * P if S > 1 else 0)


@pytest.mark.gpu
def test_checkpoint_at_five_splits_on_the_device():
    import torch

    case = checkpoint_case("dyn")
    nets = case["nets"]
    x, y = np.tile(case["x"], (3, 1)), np.tile(case["y"], 3)
    M = len(x)
    assert splits_of(M) == 5
    dq = np.stack([((forward_f64(w, x)[2] - y) / M).astype(np.float32) for w in nets])
    g64 = [gradients_f64(w, x, dq[i]) for i, w in enumerate(nets)]
    g32, _ = TwinCritic(nets).parameter_gradients(*split("dyn", x), dq=dq)
    env = _env("dyn", 8)
    critic = DeviceCritic(nets, env)
    rows, act = _rows("dyn", x)
    got = env.critic_parameter_gradients(critic, act, dq=_dev(dq), rows=rows)
    scale = np.float32(1.0 / M)
    by_target = env.critic_parameter_gradients(critic, act, target=_dev(y), scale=float(scale), rows=rows)
    torch.cuda.synchronize()
    own = ((by_target["q"].cpu().numpy() - y[None, :]).astype(np.float32) * scale).astype(np.float32)
    by_dq = env.critic_parameter_gradients(critic, act, dq=_dev(own), rows=rows)
    torch.cuda.synchronize()
    assert _all_same(by_target, by_dq)
    for i in (0, 1):
        for k in CRITIC_ARRAYS:
            dev = float(np.abs(got["grads"][i][k].cpu().numpy().astype(np.float64) - g64[i][k]).max())
            dev32 = float(np.abs(g32[i][k].astype(np.float64) - g64[i][k]).max())
            print(f"dyn qf{i} {k}: kernels vs float64 {dev:.3e}, numpy float32 vs float64 {dev32:.3e} (bound {4 * dev32:.3e}) on {M} rows, 5 splits")
            assert dev <= 4.0 * dev32, (i, k, dev, dev32)
    critic.close()
    env.close()


def _learner_setup():
    from ur_gym_amd.evaluation import DeviceReplay

    env = _env("dyn", 161, seed=3, auto_reset=True)
    return env, DeviceReplay(env, 4)


def _targets(ln, batch):
    """SAC's y of a sampled batch as SACLearner.update forms it in float32, and in float64 from the same float32 terms."""
    import torch

    gamma = float(ln.hp["gamma"])
    with torch.no_grad():
        alpha = ln.log_ent_coef.detach().exp()
        y32 = batch["target"] - gamma * (~batch["terminated"]).to(torch.float32) * alpha * batch["next_log_prob"]
        y64 = batch["target"].double() - gamma * (~batch["terminated"]).double() * alpha.double() * batch["next_log_prob"].double()
    return y32, y64


def _loss_gradients(ln, batch, y, dtype):
    """torch.autograd on SAC's critic loss, the default route's expression, on a copy of the learner's critic as it stands, in `dtype`:
    (two dicts keyed by CRITIC_ARRAYS, the loss)."""
    from ur_gym_amd.training import TorchTwinCritic, _features

    copy = TorchTwinCritic(ln.critic.qf[0][0].in_features, ln.critic.qf[0][0].out_features).to("cuda:0").to(dtype)
    copy.load_state_dict({k: v.detach().clone().to(dtype) for k, v in ln.critic.state_dict().items()})
    q0, q1 = copy(_features(batch["observations"]).to(dtype), batch["actions"].to(dtype))
    loss = 0.5 * (((q0 - y) ** 2).mean() + ((q1 - y) ** 2).mean())
    loss.backward()
    return [{k: p.grad.detach().double() for k, p in w.items()} for w in copy.tensors()], loss.detach()


@pytest.mark.gpu
def test_learner_critic_gradients_under_the_torch_actor_loss():
    """device_critic_gradient with the actor loss in torch: ``actor_loss.backward()`` adds into the very tensors the kernels write,
    and nothing zeroes them.  Two updates; what the launches of the second write is captured as they return (a wrapper round
    ``env.critic_parameter_gradients`` that clones its result: SACLearner is as it is), so that the first update's leftovers would show.
    The yardstick is torch float32 autograd on the same loss, batch and parameters: the default route's arithmetic."""
    import torch

    from ur_gym_amd.training import SACLearner

    env, replay = _learner_setup()
    ln = SACLearner(env, seed=5, hidden_width=32, batch_size=64, device_critic_gradient=True, device_action_gradient=False)
    assert ln.critic_grads is not None and isinstance(ln.online, DeviceCritic)
    ln.collect(replay, 4)
    verb, captured = env.critic_parameter_gradients, []

    def recording(*args, **kw):
        got = verb(*args, **kw)
        captured.append(dict(grads=[{k: v.clone() for k, v in w.items()} for w in got["grads"]], q=got["q"].clone(), into=kw.get("out")))
        return got

    env.critic_parameter_gradients = recording

    def grads_are_the_learners():
        return all(p.grad is g[k] for w, g in zip(ln.critic.tensors(), ln.critic_grads) for k, p in w.items())

    ln.update(replay, 9, 2)
    assert len(captured) == 1 and captured[0]["into"] is ln.critic_grads and grads_are_the_learners()
    # the actor loss's backward pass has added to what the launches wrote: the tensors are dirty when the second update starts
    dirty = [[k for k in CRITIC_ARRAYS if not _same(ln.critic_grads[i][k], captured[0]["grads"][i][k])] for i in (0, 1)]
    print(f"after the first update the actor loss has changed {dirty} of the critic's gradient tensors")
    assert dirty[0] and dirty[1]

    seed, draw = 10, 3
    batch = replay.sample_targets(ln.device_actor, ln.target, 64, seed, draw, float(ln.hp["gamma"]), 0.0)
    y32, y64 = _targets(ln, batch)
    g64, _ = _loss_gradients(ln, batch, y64, torch.float64)
    g32, _ = _loss_gradients(ln, batch, y32, torch.float32)
    clean = verb(ln.online, batch["actions"], target=y32, scale=1.0 / 64, rows=batch["observations"])  # fresh outputs and workspace
    ln.update(replay, seed, draw)
    torch.cuda.synchronize()
    assert len(captured) == 2 and captured[1]["into"] is ln.critic_grads and grads_are_the_learners()
    assert _all_same(captured[1], clean)  # the launches overwrite: nothing of the first update is in the second's gradients
    for i in (0, 1):
        for k in CRITIC_ARRAYS:
            top = float(g64[i][k].abs().max())
            ulp = float(np.spacing(np.float32(top)))
            dev = float((captured[1]["grads"][i][k].double() - g64[i][k]).abs().max())
            dev32 = float((g32[i][k] - g64[i][k]).abs().max())
            left = float((ln.critic_grads[i][k].double() - g64[i][k]).abs().max())
            print(f"second update qf{i} {k}: device route {dev:.3e}, default route's arithmetic {dev32:.3e} (bound {4 * dev32 + ulp:.3e}), largest gradient "
                  f"{top:.3e}, ulp {ulp:.3e}; .grad after the actor loss's backward pass is {left:.3e} away")
            assert top > 0.0 and dev <= 4.0 * dev32 + ulp, (i, k, dev, dev32, ulp)
    del env.critic_parameter_gradients
    ln.close()
    env.close()


@pytest.mark.gpu
def test_learner_critic_gradients_above_one_split():
    """test_learner_critic_gradients at a batch of 2048: the three-launch path through SACLearner."""
    import torch

    from ur_gym_amd.training import SACLearner

    B = 2 * SPLIT
    env, replay = _learner_setup()
    kw = dict(seed=5, hidden_width=32, batch_size=B)
    learners = {"default": SACLearner(env, device_action_gradient=True, **kw),
                "device": SACLearner(env, device_action_gradient=True, device_critic_gradient=True, **kw)}
    assert learners["device"].critic_grads is not None
    assert learners["device"].critic_workspace.numel() == _floats(53, 32, B) and splits_of(B) == 2
    learners["default"].collect(replay, 4)
    dev, ref_max, losses = {}, {}, {}
    for label, ln in learners.items():
        batch = replay.sample_targets(ln.device_actor, ln.target, B, 9, 2, float(ln.hp["gamma"]), 0.0)
        _, y64 = _targets(ln, batch)
        g64, _ = _loss_gradients(ln, batch, y64, torch.float64)
        losses[label] = ln.update(replay, 9, 2)
        dev[label] = [{k: float((p.grad.detach().double() - g64[i][k]).abs().max()) for k, p in w.items()} for i, w in enumerate(ln.critic.tensors())]
        ref_max[label] = [{k: float(g64[i][k].abs().max()) for k in CRITIC_ARRAYS} for i in (0, 1)]
    ln = learners["device"]
    assert all(p.grad is g[k] for w, g in zip(ln.critic.tensors(), ln.critic_grads) for k, p in w.items())
    for i in (0, 1):
        for k in CRITIC_ARRAYS:
            top = ref_max["device"][i][k]
            ulp = float(np.spacing(np.float32(top)))
            print(f"batch {B} qf{i} {k}: device route {dev['device'][i][k]:.3e}, default route {dev['default'][i][k]:.3e} (bound "
                  f"{4 * dev['default'][i][k] + ulp:.3e}), largest gradient {top:.3e}, ulp {ulp:.3e}")
            assert top == ref_max["default"][i][k] and top > 0.0
            assert dev["device"][i][k] <= 4.0 * dev["default"][i][k] + ulp, (i, k)
    rel = abs(float(losses["device"]["critic_loss"]) - float(losses["default"]["critic_loss"])) / abs(float(losses["default"]["critic_loss"]))
    print(f"batch {B}: critic_loss {float(losses['device']['critic_loss']):.6g} on the device route, {float(losses['default']['critic_loss']):.6g} on the default "
          f"route, {rel:.3e} relative (bound 1e-05)")
    assert rel <= 1e-5, rel  # one loss, two float32 evaluation orders
    for ln in learners.values():
        ln.close()
    env.close()
