"""GPU tests (-m gpu) of the evaluation inside the training call: urgym_eval_stats, urgym_actor_snapshot,
urgym_policy_evaluate / DeviceEvaluation.evaluate and urgym_sac_train_evaluated / SACLearner.train(..., evaluation=, eval_every=).

The statistics are compared BIT FOR BIT with evaluation.evaluation_stats, the restatement tests/test_evaluation_host.py holds against
the header and against exact arithmetic.  An evaluation is compared with the route that exists -- reset(seed), run_closed_loop_device on
a twin environment -- and the training call with the Python sequence of train segments and evaluate calls on twins of the same seeds.
"""
import ctypes as C
import os
import struct
from fractions import Fraction

import numpy as np
import pytest
import torch

from evaluation_cases import DEVICE_COUNTS, episodes
from test_sac_train import (ALLOCATIONS_AND_VIEWS, H, N, SEED, UPDATE_SEED, Side, assert_same_last_update, assert_same_losses, assert_same_state, bits, guarded,
                            guards_intact)
from ur_gym_amd import _abi, make_vec
from ur_gym_amd._native import NativeError
from ur_gym_amd.evaluation import (ACTOR_ARRAYS, LOG_STD_ARRAYS, DeviceActor, DeviceEvaluation, evaluation_points, evaluation_stats, run_closed_loop_device)
from ur_gym_amd.training import TorchActor, host_arrays

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "actors")
KEYS = ACTOR_ARRAYS + LOG_STD_ARRAYS
FLOATS = ("mean_return", "var_return", "mean_length", "success_rate", "best_mean_after")
INTS = ("eval_index", "length_sum", "successes", "count", "improved", "reserved0")
U = 2.0 ** -53
EVAL_SEED, EVAL_STEPS = SEED + 1, 12


def word(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def decode(records):
    """An int64 [..., 9] tensor of urgym_eval_record -> a list of dicts."""
    raw = records.reshape(-1, _abi.EVAL_RECORD_WORDS).cpu().numpy().tobytes()
    recs = [_abi.EvalRecord.from_buffer_copy(raw, i * C.sizeof(_abi.EvalRecord)) for i in range(len(raw) // C.sizeof(_abi.EvalRecord))]
    return [{name: getattr(r, name) for name, _ in _abi.EvalRecord._fields_} for r in recs]


def assert_record(got, want, what, nan_ok=False):
    for k in FLOATS:
        same = word(got[k]) == word(want[k]) or (nan_ok and np.isnan(got[k]) and np.isnan(want[k]))  # a NaN's sign and payload are the hardware's
        assert same, (what, k, got[k], float(want[k]))
    for k in INTS:
        assert got[k] == want[k], (what, k, got[k], want[k])


@pytest.fixture(scope="module")
def env():
    e = make_vec("UR5OriReach-v1", num_envs=4, seed=SEED, auto_reset=False)  # the two raw calls need a handle, not its envs
    yield e
    e.close()


class RawStats:
    """Guarded device views for one urgym_eval_stats problem of n episodes and `slots` records."""

    def __init__(self, dev, n, slots=1):
        self.g = dict(r=guarded((n,), torch.float64, dev, 0.0), last=guarded((n,), torch.int32, dev, 0), succ=guarded((n,), torch.uint8, dev, 0),
                      best_mean=guarded((1,), torch.float64, dev, -np.inf), best_index=guarded((1,), torch.int64, dev, -1),
                      records=guarded((slots, _abi.EVAL_RECORD_WORDS), torch.int64, dev, -1))
        self.v = {k: view for k, (_, view) in self.g.items()}

    def call(self, env, slot, eval_index):
        v = self.v
        env.evaluation_stats(v["r"], v["last"], v["succ"], v["best_mean"], v["best_index"], v["records"][slot], eval_index)

    def best(self):
        return float(self.v["best_mean"].cpu()[0]), int(self.v["best_index"].cpu()[0])


@pytest.mark.parametrize("n", DEVICE_COUNTS)
def test_eval_stats_equals_the_restatement_bitwise(env, n):
    dev = env.device
    r, last, succ = episodes(n)
    raw = RawStats(dev, n, slots=2)
    src = [torch.from_numpy(x).to(dev) for x in (r, last, succ)]
    torch.cuda.synchronize(dev)
    # the inputs are written by kernels on the stream, the call follows without a synchronise: stream order
    for k, s in zip(("r", "last", "succ"), src):
        raw.v[k].copy_(s * 1)
    raw.call(env, 0, 3)
    raw.v["best_mean"].fill_(-np.inf), raw.v["best_index"].fill_(-1)
    raw.call(env, 1, 3)  # repeatable: the same problem again
    torch.cuda.synchronize(dev)
    want = evaluation_stats(r, last, succ, -np.inf, -1, 3)
    got = decode(raw.v["records"])
    assert_record(got[0], want, n)
    assert got[1] == got[0] and bits(raw.v["records"][0]).tobytes() == bits(raw.v["records"][1]).tobytes()
    assert (word(raw.best()[0]), raw.best()[1]) == (word(want["best_mean"]), 3) and want["improved"] == 1
    assert guards_intact(raw.g) is None, guards_intact(raw.g)
    print(f"N = {n}: mean {got[0]['mean_return']!r} var {got[0]['var_return']!r} length {got[0]['mean_length']!r} success {got[0]['success_rate']!r}")


def test_eval_stats_sequence_through_the_device_best_state(env):
    """rising mean, a tie, a NaN return, a lower mean: five evaluations chained through the best state on the device, no synchronise."""
    dev, n = env.device, 65
    r, last, succ = episodes(n)
    raw = RawStats(dev, n, slots=5)
    raw.v["last"].copy_(torch.from_numpy(last).to(dev)), raw.v["succ"].copy_(torch.from_numpy(succ).to(dev))
    nan = r.copy()
    nan[64] = np.nan
    series = [r, r + 1.0, r + 1.0, nan, r - 2.0]
    for i, x in enumerate(series):
        raw.v["r"].copy_(torch.from_numpy(x).to(dev))
        raw.call(env, i, i)
    torch.cuda.synchronize(dev)
    got, best = decode(raw.v["records"]), (-np.inf, -1)
    for i, x in enumerate(series):
        want = evaluation_stats(x, last, succ, best[0], best[1], i)
        assert_record(got[i], want, i, nan_ok=(i == 3))
        best = (want["best_mean"], want["best_index"])
    assert [g["improved"] for g in got] == [1, 1, 0, 0, 0] and np.isnan(got[3]["mean_return"])
    assert (word(raw.best()[0]), raw.best()[1]) == (word(got[1]["mean_return"]), 1) == (word(best[0]), best[1])
    assert all(word(g["best_mean_after"]) == word(got[1]["mean_return"]) for g in got[1:])
    assert guards_intact(raw.g) is None


def actor_tensors(dev, n_in, hidden, fill=None, seed=0):
    """(guarded pairs, dict of views) for the eight tensors of an n_in -> hidden actor."""
    shapes = dict(zip(KEYS, ((hidden, n_in), (hidden,), (hidden, hidden), (hidden,), (6, hidden), (6,), (6, hidden), (6,))))
    gen = torch.Generator(device="cpu").manual_seed(seed)
    g = {}
    for k, sh in shapes.items():
        g[k] = guarded(sh, torch.float32, dev, fill)
        if fill is None:
            g[k][1].copy_(torch.randn(sh, generator=gen).to(dev))
    return g, {k: v for k, (_, v) in g.items()}


@pytest.mark.parametrize("hidden", [32, 512])
@pytest.mark.parametrize("n_in", [30, 32, 41, 47])
def test_actor_snapshot(env, n_in, hidden):
    dev = env.device
    gs, src = actor_tensors(dev, n_in, hidden, seed=n_in + hidden)
    src["mu_bias"][0] = float("nan")  # bits, not values
    flag = torch.zeros(3, dtype=torch.int32, device=dev)
    flag[1] = 1
    flag[2] = -7  # any non-zero word copies
    for when, copies in ((flag[0:1], False), (flag[1:2], True), (flag[2:3], True), (None, True)):
        gd, dst = actor_tensors(dev, n_in, hidden, fill=float("nan"))
        before = {k: flat.clone() for k, (flat, _) in gd.items()}
        env.actor_snapshot(src, dst, n_in, hidden, when=when)
        torch.cuda.synchronize(dev)
        for k in KEYS:
            if copies:
                assert np.array_equal(bits(dst[k]), bits(src[k])), (when, k)
            else:
                assert torch.equal(gd[k][0], before[k]), (when, k)  # the NaN-filled destination, bit for bit
        assert guards_intact(gd) is None and guards_intact(gs) is None, (when, guards_intact(gd))


def eval_env(env_id, n):
    return make_vec(env_id, num_envs=n, seed=EVAL_SEED, auto_reset=False)


def random_actor(env_id, hidden, seed):
    torch.manual_seed(seed)
    obs, goal = _abi.OBS_DIMS[_abi.ENV_IDS[env_id]]
    return host_arrays(TorchActor(obs + 2 * goal, hidden).tensors())


def shipped_actor():
    w = dict(np.load(os.path.join(GOLDEN, "actor_ori.npz")))
    w.update(np.load(os.path.join(GOLDEN, "log_std_ori.npz")))
    return w


@pytest.mark.parametrize("env_id,n,steps,weights", [("UR5OriReach-v1", 256, 100, "shipped"), ("UR5DynReach-v1", 65, 12, "random")], ids=["Ori-256", "Dyn-65"])
def test_evaluate_equals_reset_and_closed_loop_on_a_twin(env_id, n, steps, weights, tmp_path):
    w = shipped_actor() if weights == "shipped" else random_actor(env_id, 32, 3)
    test_env, twin = eval_env(env_id, n), eval_env(env_id, n)
    dev = test_env.device
    source = {k: torch.from_numpy(np.ascontiguousarray(w[k], dtype=np.float32)).to(dev) for k in KEYS}
    blank = {k: np.zeros_like(v) for k, v in w.items()}  # the eval actor starts with other weights: evaluate loads the source
    ev = DeviceEvaluation(test_env, blank, num_steps=steps, seed=EVAL_SEED, capacity=1)
    assert ev.evaluate(source) == 0 and ev.count == 1
    # the route that exists, on the twin
    twin_actor = DeviceActor(w, twin)
    twin.reset(seed=EVAL_SEED)
    res = run_closed_loop_device(twin, twin_actor, steps)
    got = ev.results()
    want = evaluation_stats(res["reward"], res["last_step"].astype(np.int32), res["success"], -np.inf, -1, 0)
    assert len(got) == 1
    assert_record(got[0], want, env_id)
    assert got[0]["std_return"] == float(np.sqrt(want["var_return"])) and got[0]["count"] == n and got[0]["improved"] == 1
    assert got[0]["success_rate"] * 100.0 == res["success_rate_percent"]  # exact
    # the mean against the exact one, within the bound of tests/test_evaluation_host.py; numpy's pairwise mean meets the same bound
    exact = [Fraction(float(x)) for x in res["reward"]]
    bound = (n + 1) * Fraction(U) * sum(abs(x) for x in exact) / n
    print(f"{env_id}: mean_return {got[0]['mean_return']!r} against numpy's {res['mean_episode_reward']!r}, bound {float(bound):.3e}; "
          f"success {res['success_rate_percent']}%, mean length {got[0]['mean_length']}")
    assert abs(Fraction(got[0]["mean_return"]) - sum(exact) / n) <= bound and abs(Fraction(res["mean_episode_reward"]) - sum(exact) / n) <= bound
    for k in test_env.buf:  # all 24 bound buffers
        assert np.array_equal(bits(test_env.buf[k]), bits(twin.buf[k])), k
    assert len(test_env.buf) == 24 and np.array_equal(ev.actor.packed().view(np.uint8), twin_actor.packed().view(np.uint8))
    best = {k: v.clone() for k, v in ev.best_parameters().items()}
    for k in KEYS:
        assert np.array_equal(bits(best[k]), bits(source[k])), k
    assert ev.best_state() == (got[0]["mean_return"], 0)
    with pytest.raises(ValueError, match="records"):
        ev.evaluate(source)  # capacity = 1
    # the writer, and the reader that exists
    path = os.path.join(str(tmp_path), "best_model.npz")
    ev.save_best(path)
    back = DeviceActor.load(path, twin)
    assert back.has_log_std and np.array_equal(back.packed().view(np.uint8), twin_actor.packed().view(np.uint8))
    back.close(), twin_actor.close(), ev.close(), test_env.close(), twin.close()


@pytest.mark.parametrize("env_id,n,steps,weights", [("UR5OriReach-v1", 256, 100, "shipped"), ("UR5DynReach-v1", 65, 12, "random")], ids=["Ori-256", "Dyn-65"])
def test_a_second_evaluate_with_unchanged_parameters_gives_the_same_record(env_id, n, steps, weights):
    """The same statistics again, a tie (improved == 0), the best tensors unchanged.

    UR5DynReach-v1 is the case that can go wrong: RESET leaves the velocity slot of its observation as it finds it (the reference's
    reset returns the stale ReachDyn.velocity of the step before, reach.py:657, which urgym_reset reproduces), so a plain
    ``reset(seed=s)`` shows zeros there on a fresh environment and, later, the twist the last step of the previous rollout applied:
    the Python route, ``reset(seed)`` + ``rollout_policy`` three times on one environment, gives mean return -1566.4523972731372, then
    -1566.0327082707333 twice.  urgym_policy_evaluate zeroes the observation before its reset, so every evaluation starts as the first
    one of a fresh environment does."""
    w = shipped_actor() if weights == "shipped" else random_actor(env_id, 32, 3)
    test_env = eval_env(env_id, n)
    source = {k: torch.from_numpy(np.ascontiguousarray(w[k], dtype=np.float32)).to(test_env.device) for k in KEYS}
    ev = DeviceEvaluation(test_env, w, num_steps=steps, seed=EVAL_SEED, capacity=3)
    ev.evaluate(source)
    torch.cuda.synchronize(test_env.device)
    for v in ev.best.values():  # poisoned, to see that nothing is copied
        v.fill_(float("nan"))
    ev.evaluate(source)
    torch.cuda.synchronize(test_env.device)
    poisoned = all(torch.isnan(v).all().item() for v in ev.best.values())
    state = ev.best_state()
    ev.evaluate(source)
    first, second, third = ev.results()
    print(f"{env_id}: mean return {first['mean_return']!r}, {second['mean_return']!r}, {third['mean_return']!r}; improved "
          f"{[r['improved'] for r in (first, second, third)]}")
    assert first["improved"] == 1
    assert_record(third, dict(second, eval_index=2, improved=0), "the third against the second")
    assert_record(second, dict(first, eval_index=1, improved=0), "the second against the first")
    assert poisoned and state == (first["mean_return"], 0)
    ev.close(), test_env.close()


class Evaluated:
    """A Side with a DeviceEvaluation on an evaluation env of its own, all from the same seeds whichever side it is."""

    def __init__(self, capacity=4):
        self.side = Side()
        self.test_env = eval_env("UR5OriReach-v1", N)
        self.ev = DeviceEvaluation(self.test_env, self.side.learner.actor.tensors(), num_steps=EVAL_STEPS, seed=EVAL_SEED, capacity=capacity)
        self.ev.records.fill_(-1)  # so that an untouched record shows

    def train(self, iterations, first_draw, every=4, **kw):
        s = self.side
        return s.learner.train(s.replay, iterations, 1, 2, seed=UPDATE_SEED, first_draw=first_draw, evaluation=self.ev, eval_every=every, **kw)

    def evaluation_state(self):
        out = {f"eval.buf.{k}": v for k, v in self.test_env.buf.items()}
        out.update({f"best.{k}": v for k, v in self.ev.best.items()})
        out.update({f"scratch.{k}": v for k, v in self.ev.scratch.items()})
        out.update(records=self.ev.records, best_mean=self.ev.best_mean, best_index=self.ev.best_index, eval_packed=self.ev.actor.packed())
        return out

    def everything(self):
        """One uint8 device tensor of every byte a call may write, on either environment."""
        parts = list(self.side.state().values()) + list(self.evaluation_state().values())
        dev = self.side.env.device
        return torch.cat([(torch.from_numpy(np.ascontiguousarray(p)).to(dev) if isinstance(p, np.ndarray) else p.detach().contiguous()).view(torch.uint8).reshape(-1)
                          for p in parts])

    def close(self):
        self.ev.close(), self.test_env.close(), self.side.close()


def assert_same_evaluation(a, b, what):
    sa, sb = a.evaluation_state(), b.evaluation_state()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(bits(sa[k]), bits(sb[k])), (what, k)
    assert a.ev.count == b.ev.count, what


def test_train_with_evaluation_equals_the_python_sequence_bit_for_bit():
    points = evaluation_points(1, 6, 2, 1, 4)
    assert points == [2, 4]  # iteration 0 is idle; the update count passes 4 in iteration 2 and 8 in iteration 4
    a, b, c = Evaluated(), Evaluated(), Side()
    # a: ONE native call
    got = a.train(6, first_draw=7)
    # b: the Python sequence: train segments that end where an evaluation falls, evaluate in between
    pieces, done, at = [], 0, 0
    for stop in points + [5]:
        if stop + 1 > at:
            pieces.append(b.side.learner.train(b.side.replay, stop + 1 - at, 1, 2, seed=UPDATE_SEED, first_draw=7 + done))
            done, at = b.side.learner.adam_state["step"], stop + 1
        if stop in points:
            b.ev.evaluate(b.side.learner.actor.tensors())
    # c: the same training without any evaluation
    plain = c.learner.train(c.replay, 6, 1, 2, seed=UPDATE_SEED, first_draw=7)
    torch.cuda.synchronize(a.side.env.device)
    assert a.ev.count == b.ev.count == 2
    for k in got:
        assert got[k].shape == (10,) and np.array_equal(bits(got[k]), bits(torch.cat([p[k] for p in pieces]))), k
        assert np.array_equal(bits(got[k]), bits(plain[k])), k
    assert_same_state(a.side, b.side, "one call against the sequence")
    assert_same_last_update(a.side, b.side, "one call against the sequence")
    assert_same_evaluation(a, b, "one call against the sequence")
    assert_same_state(a.side, c, "the evaluation perturbs nothing")
    assert_same_last_update(a.side, c, "the evaluation perturbs nothing")
    recs = a.ev.results()
    assert [r["eval_index"] for r in recs] == [0, 1] and recs[0]["improved"] == 1 and all(r["count"] == N and np.isfinite(r["mean_return"]) for r in recs)
    assert bits(a.ev.records[2:]).tobytes() == b"\xff" * (2 * 72)  # the records beyond the call's two are untouched
    # the best tensors are the parameters as they stood at the best evaluation, which the sequence's side b holds the same way
    best_mean, best_index = a.ev.best_state()
    assert best_index in (0, 1) and best_mean == recs[best_index]["mean_return"] == max(r["mean_return"] for r in recs)
    print(f"records: {[(r['mean_return'], r['improved']) for r in recs]}, best {best_mean!r} at {best_index}")

    # the same as two calls, 2 + 4 iterations, without a synchronise in between
    d = Evaluated()
    first = d.train(2, first_draw=7)
    second = d.train(4, first_draw=7 + 2)
    torch.cuda.synchronize(d.side.env.device)
    assert first["critic_loss"].shape == (2,) and second["critic_loss"].shape == (8,) and d.ev.count == 2
    for k in got:
        assert np.array_equal(bits(got[k]), bits(torch.cat([first[k], second[k]]))), k
    assert_same_state(a.side, d.side, "2 + 4 iterations")
    assert_same_evaluation(a, d, "2 + 4 iterations")
    a.close(), b.close(), c.close(), d.close()


def test_an_interval_beyond_the_calls_updates_evaluates_nothing():
    a, c = Evaluated(), Side()
    before = {k: bits(v).copy() for k, v in a.evaluation_state().items()}
    got = a.train(6, first_draw=7, every=1000)
    plain = c.learner.train(c.replay, 6, 1, 2, seed=UPDATE_SEED, first_draw=7)
    torch.cuda.synchronize(a.side.env.device)
    assert a.ev.count == 0 and a.ev.results() == []
    for k, v in a.evaluation_state().items():  # the records and everything else of the evaluation are untouched
        assert np.array_equal(bits(v), before[k]), k
    for k in got:
        assert np.array_equal(bits(got[k]), bits(plain[k])), k
    assert_same_state(a.side, c, "no evaluation")
    a.close(), c.close()


def test_train_wants_both_arguments_or_neither():
    a = Evaluated()
    s = a.side
    with pytest.raises(ValueError, match="go together"):
        s.learner.train(s.replay, 1, 1, 2, seed=UPDATE_SEED, first_draw=0, evaluation=a.ev)
    with pytest.raises(ValueError, match="go together"):
        s.learner.train(s.replay, 1, 1, 2, seed=UPDATE_SEED, first_draw=0, eval_every=4)
    a.close()


def test_train_with_evaluation_runs_no_torch_operation_that_launches():
    from torch.utils._python_dispatch import TorchDispatchMode

    class Recorder(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.append(str(func))
            return func(*args, **(kwargs or {}))

    a = Evaluated(capacity=8)
    a.train(3, first_draw=0, every=2)  # warms: the scratch and both structs exist afterwards
    assert a.ev.count == 2
    with Recorder() as rec:
        losses = a.train(2, first_draw=4, every=2)
    torch.cuda.synchronize(a.side.env.device)
    print(f"{len(rec.names)} torch operations in one train call of 2 x (1 step, 2 updates) with 2 evaluations: {sorted(set(rec.names))}")
    assert a.ev.count == 4 and losses["critic_loss"].shape == (4,) and "aten.empty.memory_format" in rec.names
    assert set(rec.names) <= ALLOCATIONS_AND_VIEWS, sorted(set(rec.names) - ALLOCATIONS_AND_VIEWS)
    assert len(rec.names) <= 8
    a.close()


def test_refusals_launch_nothing_and_write_nothing():
    a = Evaluated()
    s, env, lib, ev, test_env = a.side, a.side.env, a.side.env.lib, a.ev, a.test_env
    dev = env.device
    other_env = eval_env("UR5OriReach-v1", N)
    other_actor = DeviceActor(host_arrays(s.learner.actor.tensors()), other_env)
    auto_env = make_vec("UR5OriReach-v1", num_envs=N, seed=EVAL_SEED, auto_reset=True)
    auto_actor = DeviceActor(host_arrays(s.learner.actor.tensors()), auto_env)
    wide = DeviceActor(random_actor("UR5OriReach-v1", 64, 1), test_env)  # of the evaluation handle, of another shape
    P = ev.struct(s.learner.actor.tensors())
    binding = s.learner._train_binding(s.replay)["binding"]
    L = binding.struct
    losses = torch.full((3, 4), float("nan"), dtype=torch.float32, device=dev)
    for name, t in zip(_abi.SAC_LEARNER_LOSSES, losses):
        setattr(L, name, C.cast(t.data_ptr(), C.POINTER(C.c_float)))
    s.learner.collect(s.replay, 4)  # a filled ring, so that the schedule below is sound
    torch.cuda.synchronize(dev)
    before = a.everything()
    refused = []

    def edited(struct, **fields):
        c = type(struct).from_buffer_copy(struct)
        for k, v in fields.items():
            *inner, field = k.split(".")
            owner = c
            for p in inner:
                owner = getattr(owner, p)
            setattr(owner, field, v)
        return c

    def refuse_evaluate(what, handle, struct, expect=None, eval_index=0, slot=0, code=_abi.ERR_ARG):
        rc = lib.urgym_policy_evaluate(handle, C.byref(struct) if struct is not None else None, eval_index, slot, test_env._stream())
        msg = lib.urgym_last_error(handle).decode()
        assert rc == code and msg.startswith("urgym_policy_evaluate: "), (what, rc, msg)
        assert expect is None or expect in msg, (what, msg)
        refused.append(what)

    th = test_env._h
    refuse_evaluate("NULL struct", th, None, "null evaluation")
    refuse_evaluate("reserved0", th, edited(P, reserved0=1), "reserved0")
    for k in (0, -3):
        refuse_evaluate(f"num_steps = {k}", th, edited(P, num_steps=k), "num_steps")
    refuse_evaluate("record_capacity = 0", th, edited(P, record_capacity=0), "record_capacity")
    refuse_evaluate("auto_reset on", auto_env._h, edited(P, eval_actor=auto_actor._a), "auto_reset")
    refuse_evaluate("an actor of another handle", th, edited(P, eval_actor=other_actor._a), "not an actor of the evaluation handle")
    refuse_evaluate("NULL eval_actor", th, edited(P, eval_actor=None), "eval_actor")
    refuse_evaluate("an actor of another shape", th, edited(P, eval_actor=wide._a), "the eval actor is")
    refuse_evaluate("a source of another width", th, edited(P, hidden_width=H + 32), "the source is")
    refuse_evaluate("a source of other features", th, edited(P, in_features=31), "the source is")
    for group in ("source", "best"):
        for field in _abi.ACTOR_DEV_ARRAYS:
            refuse_evaluate(f"{group}.{field} = NULL", th, edited(P, **{f"{group}.{field}": None}), "all sixteen")
    for field in ("episode_return", "episode_last_step", "episode_success", "episode_done", "records", "best_mean", "best_index"):
        refuse_evaluate(f"{field} = NULL", th, edited(P, **{field: None}), field)
    for slot in (-1, ev.capacity, ev.capacity + 5):
        refuse_evaluate(f"record_slot = {slot}", th, P, "record_slot", slot=slot)
    refuse_evaluate("eval_index = -1", th, P, "eval_index", eval_index=-1)
    assert lib.urgym_policy_evaluate(None, C.byref(P), 0, 0, None) == _abi.ERR_ARG
    # an evaluation handle that was never bound, and one with more envs than one workgroup reduces
    unbound = C.c_void_p()
    cfg = _abi.Config()
    assert lib.urgym_config_default(_abi.ENV_ORI, N, C.byref(cfg)) == 0
    cfg.auto_reset = 0
    assert lib.urgym_create(C.byref(cfg), dev.index, C.byref(unbound)) == 0
    refuse_evaluate("an unbound handle", unbound, P, "urgym_bind", code=_abi.ERR_STATE)
    assert lib.urgym_destroy(unbound) == 0
    big = eval_env("UR5OriReach-v1", _abi.EVAL_MAX_COUNT + 1)
    big_actor = DeviceActor(host_arrays(s.learner.actor.tensors()), big)
    refuse_evaluate("65537 envs", big._h, edited(P, eval_actor=big_actor._a), "more than 65536 envs")
    with pytest.raises(ValueError, match="65536"):
        DeviceEvaluation(big, s.learner.actor.tensors())
    big_actor.close(), big.close()
    with pytest.raises(ValueError, match="auto_reset"):
        DeviceEvaluation(auto_env, s.learner.actor.tensors())

    # the training call
    ok = dict(first_slot=0, filled_steps=4, capacity_steps=4, num_iterations=2, steps_per_iteration=1, updates_per_iteration=2, uniform_iterations=0,
              idle_iterations=0, collect_first_draw=0, update_first_draw=0, first_step=1)
    E = _abi.SacEvaluation(test_env._h, P, 2, 0, 0)  # two evaluations

    def refuse_train(what, learner, evaluation, expect=None, code=_abi.ERR_ARG, **sched):
        S = _abi.SacSchedule(*[dict(ok, **sched)[n] for n, _ in _abi.SacSchedule._fields_])
        rc = lib.urgym_sac_train_evaluated(env._h, C.byref(learner), C.byref(S), C.byref(evaluation) if evaluation is not None else None, env._stream())
        msg = lib.urgym_last_error(env._h).decode()
        assert rc == code and msg.startswith("urgym_sac_train_evaluated: "), (what, rc, msg)
        assert expect is None or expect in msg, (what, msg)
        refused.append(what)

    refuse_train("NULL evaluation", L, None, "null evaluation")
    refuse_train("NULL eval_handle", L, edited(E, eval_handle=None), "eval_handle is null")
    refuse_train("eval_handle == handle", L, edited(E, eval_handle=env._h), "the training handle")
    own_copy = {k: v.detach().clone() for k, v in s.learner.actor.tensors().items()}
    other_source = _abi.ActorTensors(*[C.cast(own_copy[k].data_ptr(), C.POINTER(C.c_float)) for k in KEYS])
    refuse_train("source tensors other than the learner's", L, edited(E, **{"evaluation.source": other_source}), "actor_adam.param")
    for every in (0, -1):
        refuse_train(f"every = {every}", L, edited(E, every=every), "every")
    refuse_train("first_eval_index = -1", L, edited(E, first_eval_index=-1), "first_eval_index")
    refuse_train("first_record_slot = -1", L, edited(E, first_record_slot=-1), "first_record_slot")
    refuse_train("one record too few", L, edited(E, first_record_slot=ev.capacity - 1), "record_capacity")
    refuse_train("capacity of one", L, edited(E, **{"evaluation.record_capacity": 1}), "record_capacity")
    # every refusal of the composed calls: one of the training call's, one of the schedule's, several of the evaluation's
    refuse_train("count = 0", edited(L, count=0), E)
    refuse_train("online == target", edited(L, target=L.online), E, "the online critic itself")
    refuse_train("num_iterations = 0", L, E, "num_iterations", num_iterations=0)
    refuse_train("num_steps = 0", L, edited(E, **{"evaluation.num_steps": 0}), "num_steps")
    refuse_train("evaluation.reserved0", L, edited(E, **{"evaluation.reserved0": 1}), "reserved0")
    refuse_train("an eval actor of another handle", L, edited(E, **{"evaluation.eval_actor": other_actor._a}), "not an actor of the evaluation handle")
    refuse_train("auto_reset on", L, edited(E, eval_handle=auto_env._h, **{"evaluation.eval_actor": auto_actor._a}), "auto_reset")
    refuse_train("best.w1 = NULL", L, edited(E, **{"evaluation.best.w1": None}), "all sixteen")
    refuse_train("records = NULL", L, edited(E, **{"evaluation.records": None}), "records")
    # a call without an update still validates the evaluation
    refuse_train("every = 0 without updates", L, edited(E, every=0), "every", updates_per_iteration=0)
    assert lib.urgym_sac_train_evaluated(None, C.byref(L), C.byref(_abi.SacSchedule()), C.byref(E), None) == _abi.ERR_ARG

    # the two raw calls
    raw = RawStats(dev, 5)
    v = raw.v
    SA = _abi.EvalStatsArgs(5, 0, 0)
    for name, key, ct in (("episode_return", "r", C.c_double), ("episode_last_step", "last", C.c_int32), ("episode_success", "succ", C.c_uint8),
                          ("best_mean", "best_mean", C.c_double), ("best_index", "best_index", C.c_int64)):
        setattr(SA, name, C.cast(v[key].data_ptr(), C.POINTER(ct)))
    SA.record = C.cast(v["records"].data_ptr(), C.POINTER(_abi.EvalRecord))
    raw_before = torch.cat([flat.view(torch.uint8) for flat, _ in raw.g.values()]).clone()

    def refuse_raw(call, who, what, struct, expect=None):
        rc = call(env._h, C.byref(struct) if struct is not None else None, env._stream())
        msg = lib.urgym_last_error(env._h).decode()
        assert rc == _abi.ERR_ARG and msg.startswith(who + ": "), (what, rc, msg)
        assert expect is None or expect in msg, (what, msg)
        refused.append(what)

    for count in (0, -1, 65537):
        refuse_raw(lib.urgym_eval_stats, "urgym_eval_stats", f"stats count = {count}", edited(SA, count=count), "count")
    refuse_raw(lib.urgym_eval_stats, "urgym_eval_stats", "stats NULL args", None, "null args")
    refuse_raw(lib.urgym_eval_stats, "urgym_eval_stats", "stats reserved0", edited(SA, reserved0=2), "reserved0")
    refuse_raw(lib.urgym_eval_stats, "urgym_eval_stats", "stats eval_index", edited(SA, eval_index=-1), "eval_index")
    for name, _ in _abi.EvalStatsArgs._fields_[3:]:
        refuse_raw(lib.urgym_eval_stats, "urgym_eval_stats", f"stats {name} = NULL", edited(SA, **{name: None}), name)
    SN = _abi.ActorSnapshotArgs(P.in_features, P.hidden_width, P.source, P.best)
    refuse_raw(lib.urgym_actor_snapshot, "urgym_actor_snapshot", "snapshot NULL args", None, "null args")
    refuse_raw(lib.urgym_actor_snapshot, "urgym_actor_snapshot", "snapshot reserved0", edited(SN, reserved0=1), "reserved0")
    for bad in (dict(in_features=0), dict(hidden_width=0), dict(hidden_width=513)):
        refuse_raw(lib.urgym_actor_snapshot, "urgym_actor_snapshot", f"snapshot {bad}", edited(SN, **bad))
    for group in ("source", "destination"):
        for field in _abi.ACTOR_DEV_ARRAYS:
            refuse_raw(lib.urgym_actor_snapshot, "urgym_actor_snapshot", f"snapshot {group}.{field} = NULL", edited(SN, **{f"{group}.{field}": None}), "all sixteen")

    # the Python layer's own checks: ValueError before the library is called
    with pytest.raises(ValueError, match="float64"):
        env.evaluation_stats(v["r"].float(), v["last"], v["succ"], v["best_mean"], v["best_index"], v["records"][0], 0)
    with pytest.raises(ValueError, match="record"):
        env.evaluation_stats(v["r"], v["last"], v["succ"], v["best_mean"], v["best_index"], v["records"][0][:8], 0)
    with pytest.raises(ValueError, match="eval_index"):
        env.evaluation_stats(v["r"], v["last"], v["succ"], v["best_mean"], v["best_index"], v["records"][0], -1)
    with pytest.raises(ValueError, match="when"):
        env.actor_snapshot(s.learner.actor.tensors(), ev.best, P.in_features, P.hidden_width, when=torch.zeros(1, device=dev))
    with pytest.raises(ValueError, match="log_std"):
        env.actor_snapshot({k: v_ for k, v_ in s.learner.actor.tensors().items() if k in ACTOR_ARRAYS}, ev.best, P.in_features, P.hidden_width)
    own = DeviceEvaluation.__new__(DeviceEvaluation)
    own.env = env
    with pytest.raises(ValueError, match="environment of its own"):
        env.sac_train(binding, *losses, first_slot=0, filled_steps=4, num_iterations=2, updates_per_iteration=2, evaluation=own, eval_every=2)
    with pytest.raises(ValueError, match="eval_every"):
        env.sac_train(binding, *losses, first_slot=0, filled_steps=4, num_iterations=2, updates_per_iteration=2, evaluation=ev, eval_every=0)
    with pytest.raises(ValueError, match="DeviceEvaluation"):
        env.sac_train(binding, *losses, first_slot=0, filled_steps=4, num_iterations=2, updates_per_iteration=2, evaluation=object(), eval_every=2)
    with pytest.raises(NativeError, match="record_capacity"):  # five evaluations into four records: refused by the library, nothing advanced
        env.sac_train(binding, *[torch.empty(10, device=dev)] * 3, first_slot=0, filled_steps=4, num_iterations=5, updates_per_iteration=2, evaluation=ev,
                      eval_every=2)
    assert ev.count == 0

    # nothing was launched: every byte on both environments is what it was
    torch.cuda.synchronize(dev)
    assert torch.equal(a.everything(), before) and torch.isnan(losses).all()
    assert torch.equal(torch.cat([flat.view(torch.uint8) for flat, _ in raw.g.values()]), raw_before)
    assert len(refused) > 90, len(refused)
    for name in _abi.SAC_LEARNER_LOSSES:
        setattr(L, name, None)
    wide.close(), auto_actor.close(), auto_env.close(), other_actor.close(), other_env.close(), a.close()
