"""GPU tests (-m gpu) of the training-episode statistics: urgym_monitor_fold, urgym_monitor_stats,
DeviceMonitor and urgym_sac_train_monitored / SACLearner.train(..., monitor=, log_every=).

The two kernels are compared BIT FOR BIT with evaluation.monitor_fold / monitor_stats, the restatements tests/test_monitor_host.py holds
against the header and against exact arithmetic: on synthetic rings the test fills, and on the ring a real collection has written.  The
training call is compared with the Python loop of collect(..., monitor=), update and record on a twin of the same seeds, and with the
same call without a monitor.  Small shapes: N = 64 envs, H = 32, M = 64 rows, a ring of 4 slots, episodes of at most 3 steps.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from monitor_cases import AFTER_NAN_RECORD, CAP, DEVICE_COUNTS, EMPTY_RECORD, FLOATS, INTS, NAN_RECORD, SCRIPT, restate, rings, zero_state
from test_evaluation import EVAL_SEED, EVAL_STEPS, eval_env, random_actor
from test_sac_train import (ALL, ALLOCATIONS_AND_VIEWS, H, N, SEED, STARTS, UPDATE_SEED, Side, assert_same_last_update, assert_same_state, bits, guarded, guards_intact)
from ur_gym_amd import _abi, make_vec
from ur_gym_amd._native import NativeError
from ur_gym_amd.evaluation import DeviceActor, DeviceEvaluation, DeviceMonitor, DeviceReplay, monitor_fold, monitor_points, monitor_stats
from ur_gym_amd.training import SACLearner

pytestmark = pytest.mark.gpu

STATE = [name for name, _ in _abi.MONITOR_STATE_FIELDS]
RING = ("reward", "terminated", "truncated", "is_success")
DTYPE = {C.c_double: torch.float64, C.c_int32: torch.int32, C.c_int64: torch.int64}


def decode(records):
    """An int64 [..., 9] tensor of urgym_monitor_record -> a list of dicts."""
    raw = records.reshape(-1, _abi.MONITOR_RECORD_WORDS).cpu().numpy().tobytes()
    size = C.sizeof(_abi.MonitorRecord)
    recs = [_abi.MonitorRecord.from_buffer_copy(raw, i * size) for i in range(len(raw) // size)]
    return [{name: getattr(r, name) for name, _ in _abi.MonitorRecord._fields_} for r in recs]


def same_floats(a, b):
    """Bitwise, except that a NaN equals a NaN: its sign and payload are the hardware's."""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.uint64)[~np.isnan(a)], b.view(np.uint64)[~np.isnan(b)])


def assert_record(got, want, what, nan_ok=False):
    for k in FLOATS:
        same = same_floats(got[k], want[k]) if nan_ok else bits(np.float64(got[k])).tobytes() == bits(np.float64(want[k])).tobytes()
        assert same, (what, k, got[k], float(want[k]))
    for k in INTS:
        assert got[k] == want[k], (what, k, got[k], want[k])


def assert_state(got, want, what, nan_ok=False):
    """`got`: device tensors; `want`: the restatement's arrays."""
    for name, ct in _abi.MONITOR_STATE_FIELDS:
        g = got[name].cpu().numpy()
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name)
        same = same_floats(g, want[name]) if nan_ok and g.dtype == np.float64 else g.tobytes() == want[name].tobytes()
        assert same, (what, name)


class Synthetic:
    """An environment of n envs that is never stepped, a ring of CAP slots the test fills, and a guarded state and record array."""

    def __init__(self, n, slots=8):
        self.env = make_vec("UR5OriReach-v1", num_envs=n, seed=SEED, auto_reset=True)
        self.replay = DeviceReplay(self.env, CAP)
        dev = self.env.device
        self.g = {name: guarded((n,), DTYPE[ct], dev, 0) for name, ct in _abi.MONITOR_STATE_FIELDS}
        self.g["records"] = guarded((slots, _abi.MONITOR_RECORD_WORDS), torch.int64, dev, -1)
        self.state = {name: self.g[name][1] for name in STATE}
        self.records = self.g["records"][1]
        self.rings = {name: [torch.from_numpy(x).to(dev) for x in ring] for name, ring in rings(n).items()}
        self.used = 0

    def zero(self):
        for v in self.state.values():
            v.zero_()

    def load(self, name):
        """The ring's four tensors written by kernels on the stream: what follows follows in stream order."""
        for key, src in zip(RING, self.rings[name]):
            self.replay.ring[key].copy_(src * 1)

    def run(self, script):
        """`script` on the device, without a synchronise.  Returns the indices of the records it wrote."""
        first = self.used
        for op in script:
            if op[0] == "ring":
                self.load(op[1])
            elif op[0] == "fold":
                self.env.monitor_fold(self.state, self.replay, op[1], op[2])
            else:
                self.env.monitor_stats(self.state, self.records[self.used], op[1], clear=bool(op[2]))
                self.used += 1
        return range(first, self.used)

    def close(self):
        self.env.close()


def check_script(n):
    s = Synthetic(n, slots=10)
    dev = s.env.device
    torch.cuda.synchronize(dev)
    one = s.run(SCRIPT)
    torch.cuda.synchronize(dev)
    want, want_state = restate(n, SCRIPT)
    got = decode(s.records)
    for i, w in zip(one, want):
        assert_record(got[i], w, (n, i), nan_ok=(i == NAN_RECORD))
    assert np.isnan(got[NAN_RECORD]["mean_return"]) and all(np.isfinite(got[AFTER_NAN_RECORD][k]) for k in FLOATS)
    assert all(bits(np.float64(got[EMPTY_RECORD][k])).tobytes() == bytes(8) for k in FLOATS) and got[EMPTY_RECORD]["episodes"] == 0  # +0.0
    assert_state(s.state, want_state, n)
    # the same problem again: the same bits
    first_state = {k: v.clone() for k, v in s.state.items()}
    s.zero()
    two = s.run(SCRIPT)
    torch.cuda.synchronize(dev)
    for i, j in zip(one, two):
        assert bits(s.records[i]).tobytes() == bits(s.records[j]).tobytes() or i == NAN_RECORD, (n, i)
    assert decode(s.records[NAN_RECORD])[0]["episodes"] == decode(s.records[two[NAN_RECORD]])[0]["episodes"] == n
    assert all(bits(s.state[k]).tobytes() == bits(first_state[k]).tobytes() for k in STATE)
    assert guards_intact(s.g) is None, guards_intact(s.g)
    print(f"N = {n}: " + "; ".join(f"{g['episodes']} episodes, mean return {g['mean_return']!r}, length {g['mean_length']!r}, success {g['success_rate']!r}" for g in got[:5]))
    s.close()


@pytest.mark.parametrize("n", DEVICE_COUNTS)
def test_fold_and_stats_equal_the_restatements_bitwise(n):
    check_script(n)


def test_fold_and_stats_at_65536_envs():
    """64 terms per lane in the stats kernel's ordered sum, 256 workgroups in the fold."""
    check_script(65536)


@pytest.mark.parametrize("n", DEVICE_COUNTS)
def test_slots_outside_the_folded_steps_change_nothing(n):
    s = Synthetic(n)
    dev = s.env.device
    s.load("busy")
    s.replay.ring["reward"][2].fill_(float("nan"))  # slot 2 is not among the slots 3, 0, 1 the fold reads
    for key in RING[1:]:
        s.replay.ring[key][2].fill_(0xFF)
    s.env.monitor_fold(s.state, s.replay, 3, 3)
    s.env.monitor_stats(s.state, s.records[0], 5, clear=False)
    torch.cuda.synchronize(dev)
    state = monitor_fold(zero_state(n), *rings(n)["busy"], 3, 3)
    want, state = monitor_stats(state, 5, clear=False)
    assert_record(decode(s.records)[0], want, n)
    assert_state(s.state, state, n)
    assert guards_intact(s.g) is None
    s.close()


@pytest.mark.parametrize("env_id", ["UR5OriReach-v1", "UR5DynReach-v1"])
def test_a_real_collection(env_id):
    """Two collections of 3 steps into a ring of 4 (the second wraps), each folded behind it.  With max_episode_steps = 3 the time limit ends
    an episode every third step at the latest, so the 6 steps finish at least 2 episodes per env: a condition on the test, not a
    measurement."""
    n = 65
    env = make_vec(env_id, num_envs=n, seed=SEED, auto_reset=True, max_episode_steps=3)
    env.reset(seed=SEED)
    actor = DeviceActor(random_actor(env_id, 32, 3), env)
    replay, mon = DeviceReplay(env, CAP), DeviceMonitor(env, capacity=2)
    want = zero_state(n)
    for call in range(2):
        first = replay.cursor
        replay.collect(actor, 3, sample=dict(mode="uniform", seed=SEED, first_draw=3 * call))
        mon.fold(replay, first, 3)
        torch.cuda.synchronize(env.device)
        back = [replay.ring[k].cpu().numpy() for k in RING]  # the ring as the collection left it, read back
        want = monitor_fold(want, *back, first, 3)
        assert_state(mon.state, want, (env_id, call))
    assert (first, replay.cursor) == (3, 2)  # the second fold wrapped
    lengths_ok = (want["sum_length"] <= 3 * want["episodes"].astype(np.int64)).all() and (want["running_length"] <= 3).all()
    assert mon.record(6) == 0
    (got,) = mon.results()
    rec, want = monitor_stats(want, 6, clear=True)
    assert_record(got, rec, env_id)
    assert_state(mon.state, want, (env_id, "after the record"))
    assert got["episodes"] >= 2 * n and lengths_ok and got["mean_length"] <= 3.0 and got["length_sum"] <= 6 * n
    assert np.isfinite(got["mean_return"]) and 0.0 <= got["success_rate"] <= 1.0 and got["iteration"] == 6
    assert not any(mon.state[k].any().item() for k in ("sum_return", "sum_length", "episodes", "successes"))
    print(f"{env_id}: {got['episodes']} episodes in 6 steps of {n} envs, mean return {got['mean_return']!r}, mean length {got['mean_length']!r}, "
          f"success rate {got['success_rate']!r}")
    actor.close(), env.close()


class Monitored(Side):
    """test_sac_train's Side with episodes of at most 3 steps and a DeviceMonitor, all from the same seeds whichever side it is."""

    def __init__(self, capacity=4):
        self.env = make_vec("UR5OriReach-v1", num_envs=N, seed=SEED, auto_reset=True, max_episode_steps=3)
        self.env.reset(seed=SEED)
        self.learner = SACLearner(self.env, seed=SEED, hidden_width=H, batch_size=64, learning_starts=STARTS, **ALL)
        self.replay = DeviceReplay(self.env, CAP)
        self.mon = DeviceMonitor(self.env, capacity=capacity)
        self.mon.records.fill_(-1)  # so that an untouched record shows

    def train(self, iterations, first_draw, log_every=2, **kw):
        return self.learner.train(self.replay, iterations, 1, 2, seed=UPDATE_SEED, first_draw=first_draw, monitor=self.mon, log_every=log_every, **kw)

    def python_loop(self, iterations, first_draw, log_every=2):
        """tools/train_sac.py's loop with the monitor: collect and fold, update, record at every multiple of log_every."""
        lr, losses, draw = self.learner, [], first_draw
        for _ in range(iterations):
            lr.collect(self.replay, 1, monitor=self.mon)
            if lr.env_steps * N >= lr.hp["learning_starts"]:
                for _ in range(2):
                    losses.append({k: v.clone() for k, v in lr.update(self.replay, UPDATE_SEED, draw).items()})
                    draw += 1
            self.mon.iterations += 1
            if self.mon.iterations % log_every == 0:
                self.mon.record(self.mon.iterations)
        return losses

    def monitor_state(self):
        return dict(self.mon.state, records=self.mon.records)


def assert_same_monitor(a, b, what):
    sa, sb = a.monitor_state(), b.monitor_state()
    for k in sa:
        assert np.array_equal(bits(sa[k]), bits(sb[k])), (what, k)
    assert (a.mon.count, a.mon.iterations) == (b.mon.count, b.mon.iterations), what


def test_train_with_a_monitor_equals_the_python_loop_bit_for_bit():
    assert monitor_points(0, 6, 2) == [1, 3, 5]
    a, b, c = Monitored(), Monitored(), Monitored()
    got = a.train(6, first_draw=7)                                                     # a: ONE native call
    want = b.python_loop(6, first_draw=7)                                              # b: the Python loop
    plain = c.learner.train(c.replay, 6, 1, 2, seed=UPDATE_SEED, first_draw=7)         # c: the same training without a monitor
    torch.cuda.synchronize(a.env.device)
    assert len(want) == 10 and all(v.shape == (10,) for v in got.values())
    for u, w in enumerate(want):
        for k in got:
            assert np.array_equal(bits(got[k][u]), bits(w[k])), (u, k)
    for k in got:
        assert np.array_equal(bits(got[k]), bits(plain[k])), k
    assert_same_state(a, b, "one call against the loop")
    assert_same_last_update(a, b, "one call against the loop")
    assert_same_monitor(a, b, "one call against the loop")
    assert_same_state(a, c, "monitoring perturbs nothing")
    assert_same_last_update(a, c, "monitoring perturbs nothing")
    recs = a.mon.results()
    assert [r["iteration"] for r in recs] == [2, 4, 6] and a.mon.count == 3 and a.mon.iterations == 6
    # every env is cut off at its third step at the latest: 6 steps finish at least 2 episodes per env
    assert sum(r["episodes"] for r in recs) >= 2 * N and all(r["reserved0"] == 0 and np.isfinite(r["mean_return"]) and r["mean_length"] <= 3.0 for r in recs)
    assert bits(a.mon.records[3:]).tobytes() == b"\xff" * 72  # the record beyond the call's three is untouched
    print("records: " + "; ".join(f"{r['iteration']}: {r['episodes']} episodes, return {r['mean_return']!r}, length {r['mean_length']!r}, success {r['success_rate']!r}"
                                  for r in recs))

    # the same as two calls, 2 + 4 iterations, without a synchronise in between
    d = Monitored()
    first = d.train(2, first_draw=7)
    second = d.train(4, first_draw=7 + 2)
    torch.cuda.synchronize(d.env.device)
    assert first["critic_loss"].shape == (2,) and second["critic_loss"].shape == (8,)
    for k in got:
        assert np.array_equal(bits(got[k]), bits(torch.cat([first[k], second[k]]))), k
    assert_same_state(a, d, "2 + 4 iterations")
    assert_same_monitor(a, d, "2 + 4 iterations")
    a.close(), b.close(), c.close(), d.close()


class MonitoredEvaluated(Monitored):
    """A Monitored with a DeviceEvaluation on an evaluation env of its own."""

    def __init__(self, capacity=4):
        super().__init__(capacity)
        self.test_env = eval_env("UR5OriReach-v1", N)
        self.ev = DeviceEvaluation(self.test_env, self.learner.actor.tensors(), num_steps=EVAL_STEPS, seed=EVAL_SEED, capacity=4)
        self.ev.records.fill_(-1)

    def evaluation_state(self):
        out = {f"eval.buf.{k}": v for k, v in self.test_env.buf.items()}
        out.update({f"best.{k}": v for k, v in self.ev.best.items()})
        out.update({f"scratch.{k}": v for k, v in self.ev.scratch.items()})
        out.update(records=self.ev.records, best_mean=self.ev.best_mean, best_index=self.ev.best_index, eval_packed=self.ev.actor.packed())
        return out

    def close(self):
        self.ev.close(), self.test_env.close(), super().close()


def test_train_with_a_monitor_and_an_evaluation():
    """One call with both against urgym_sac_train_evaluated in calls of one iteration (bit for bit one call: tests/test_evaluation.py), each
    followed by the Python fold of the slot it collected and, at a multiple of log_every, the Python record."""
    a, b = MonitoredEvaluated(), MonitoredEvaluated()
    got = a.train(6, first_draw=7, evaluation=a.ev, eval_every=4)
    pieces = []
    for i in range(6):
        cursor = b.replay.cursor
        pieces.append(b.learner.train(b.replay, 1, 1, 2, seed=UPDATE_SEED, first_draw=7 + b.learner.adam_state["step"], evaluation=b.ev, eval_every=4))
        b.mon.fold(b.replay, cursor, 1)
        b.mon.iterations += 1
        if b.mon.iterations % 2 == 0:
            b.mon.record(b.mon.iterations)
    torch.cuda.synchronize(a.env.device)
    for k in got:
        assert got[k].shape == (10,) and np.array_equal(bits(got[k]), bits(torch.cat([p[k] for p in pieces]))), k
    assert_same_state(a, b, "both against the pieces")
    assert_same_monitor(a, b, "both against the pieces")
    sa, sb = a.evaluation_state(), b.evaluation_state()
    for k in sa:
        assert np.array_equal(bits(sa[k]), bits(sb[k])), k
    assert a.ev.count == b.ev.count == 2 and a.mon.count == 3 and [r["eval_index"] for r in a.ev.results()] == [0, 1]
    a.close(), b.close()


def test_an_interval_beyond_the_call_records_nothing_but_still_folds():
    a, b = Monitored(), Monitored()
    a.train(6, first_draw=7, log_every=1000)
    b.python_loop(6, first_draw=7, log_every=1000)
    torch.cuda.synchronize(a.env.device)
    assert a.mon.count == 0 and a.mon.iterations == 6 and a.mon.results() == []
    assert bits(a.mon.records).tobytes() == b"\xff" * (4 * 72)
    assert_same_monitor(a, b, "no record")
    assert int(a.mon.state["episodes"].sum()) >= 2 * N  # folded all the same
    assert_same_state(a, b, "no record")
    a.close(), b.close()


def test_train_wants_both_arguments_or_neither():
    a = Monitored()
    with pytest.raises(ValueError, match="go together"):
        a.learner.train(a.replay, 1, 1, 2, seed=UPDATE_SEED, first_draw=0, monitor=a.mon)
    with pytest.raises(ValueError, match="go together"):
        a.learner.train(a.replay, 1, 1, 2, seed=UPDATE_SEED, first_draw=0, log_every=2)
    a.close()


def test_train_with_a_monitor_runs_no_torch_operation_that_launches():
    from torch.utils._python_dispatch import TorchDispatchMode

    class Recorder(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.append(str(func))
            return func(*args, **(kwargs or {}))

    a = Monitored(capacity=8)
    a.train(3, first_draw=0, log_every=1)  # warms: the scratch and both structs exist afterwards
    assert a.mon.count == 3
    with Recorder() as rec:
        losses = a.train(2, first_draw=4, log_every=1)
    torch.cuda.synchronize(a.env.device)
    print(f"{len(rec.names)} torch operations in one train call of 2 x (1 step, 2 updates) with 2 records: {sorted(set(rec.names))}")
    assert a.mon.count == 5 and losses["critic_loss"].shape == (4,) and "aten.empty.memory_format" in rec.names
    assert set(rec.names) <= ALLOCATIONS_AND_VIEWS, sorted(set(rec.names) - ALLOCATIONS_AND_VIEWS)
    assert len(rec.names) <= 8
    a.close()


def test_refusals_launch_nothing_and_write_nothing():
    a = Monitored()
    env, lib, mon, replay = a.env, a.env.lib, a.mon, a.replay
    dev = env.device
    off_env = make_vec("UR5OriReach-v1", num_envs=N, seed=SEED, auto_reset=False)
    a.learner.collect(replay, 4, monitor=mon)  # a filled ring and a state that is not all zero
    binding = a.learner._train_binding(replay)["binding"]
    L = binding.struct
    losses = torch.full((3, 4), float("nan"), dtype=torch.float32, device=dev)
    for name, t in zip(_abi.SAC_LEARNER_LOSSES, losses):
        setattr(L, name, C.cast(t.data_ptr(), C.POINTER(C.c_float)))
    torch.cuda.synchronize(dev)

    def everything():
        parts = list(a.state().values()) + list(a.monitor_state().values()) + list(off_env.buf.values())
        return torch.cat([(torch.from_numpy(np.ascontiguousarray(p)).to(dev) if isinstance(p, np.ndarray) else p.detach().contiguous()).view(torch.uint8).reshape(-1)
                          for p in parts])

    before, refused = everything(), []

    def edited(struct, **fields):
        c = type(struct).from_buffer_copy(struct)
        for k, v in fields.items():
            *inner, field = k.split(".")
            owner = c
            for p in inner:
                owner = getattr(owner, p)
            setattr(owner, field, v)
        return c

    M = mon.struct(2)  # two records for four iterations; first_record 0, first_iteration 0
    S0, R0 = edited(M.state), edited(replay._ring)
    record = C.cast(mon.records.data_ptr(), C.POINTER(_abi.MonitorRecord))

    def refuse(what, rc, who, expect=None, handle=None):
        msg = lib.urgym_last_error(handle or env._h).decode()
        assert rc == _abi.ERR_ARG and msg.startswith(who + ": "), (what, rc, msg)
        assert expect is None or expect in msg, (what, msg)
        refused.append(what)

    def refuse_fold(what, state, ring, first=0, steps=1, expect=None, handle=None):
        h = handle or env._h
        rc = lib.urgym_monitor_fold(h, C.byref(state) if state is not None else None, C.byref(ring) if ring is not None else None, first, steps, env._stream())
        refuse("fold: " + what, rc, "urgym_monitor_fold", expect, h)

    def refuse_stats(what, state, rec, expect=None):
        rc = lib.urgym_monitor_stats(env._h, C.byref(state) if state is not None else None, rec, 0, 1, env._stream())
        refuse("stats: " + what, rc, "urgym_monitor_stats", expect)

    refuse_fold("NULL state", None, R0, expect="null monitor state")
    refuse_fold("NULL ring", S0, None, expect="null ring")
    for name in STATE:
        refuse_fold(f"{name} = NULL", edited(S0, **{name: None}), R0, expect=name)
        refuse_stats(f"{name} = NULL", edited(S0, **{name: None}), record, expect=name)
    for name, _, _, required in _abi.REPLAY_RING_FIELDS:
        refuse_fold(f"ring.{name} = NULL", S0, edited(R0, **{name: None}), expect="required ring pointer" if required else "truncated or no is_success")
    refuse_fold("ring.reserved0", S0, edited(R0, reserved0=1), expect="reserved0")
    refuse_fold("capacity_steps = 0", S0, edited(R0, capacity_steps=0), expect="capacity_steps")
    for first in (-1, CAP):
        refuse_fold(f"first_slot = {first}", S0, R0, first=first, expect="first_slot")
    for steps in (0, -2):
        refuse_fold(f"num_steps = {steps}", S0, R0, steps=steps, expect="num_steps must be positive")
    refuse_fold("num_steps > C", S0, R0, steps=CAP + 1, expect="above capacity_steps")
    refuse_fold("auto_reset off", S0, R0, expect="auto_reset off", handle=off_env._h)
    refuse_fold("a misaligned sum_return", edited(S0, sum_return=C.cast(mon.state["sum_return"].data_ptr() + 4, C.POINTER(C.c_double))), R0, expect="8-byte aligned")
    refuse_stats("NULL state", None, record, expect="null monitor state")
    refuse_stats("NULL record", S0, None, expect="null record")
    refuse_stats("a misaligned record", S0, C.cast(mon.records.data_ptr() + 4, C.POINTER(_abi.MonitorRecord)), expect="8-byte aligned")

    # the training call
    ok = dict(first_slot=0, filled_steps=4, capacity_steps=4, num_iterations=4, steps_per_iteration=1, updates_per_iteration=1, uniform_iterations=0,
              idle_iterations=0, collect_first_draw=0, update_first_draw=0, first_step=1)

    def refuse_train(what, learner, monitoring, expect=None, **sched):
        S = _abi.SacSchedule(*[dict(ok, **sched)[n] for n, _ in _abi.SacSchedule._fields_])
        rc = lib.urgym_sac_train_monitored(env._h, C.byref(learner), C.byref(S), None, C.byref(monitoring) if monitoring is not None else None, env._stream())
        refuse("train: " + what, rc, "urgym_sac_train_monitored", expect)

    refuse_train("NULL monitoring", L, None, "null monitoring")
    for name in STATE:
        refuse_train(f"state.{name} = NULL", L, edited(M, **{f"state.{name}": None}), name)
    refuse_train("records = NULL", L, edited(M, records=None), "null record")
    refuse_train("K > C", L, M, "above capacity_steps", steps_per_iteration=CAP + 1)
    # (without updates, so that the gather of a batch that asks for the two flags is not what refuses)
    refuse_train("a ring without truncated", edited(L, **{"ring.truncated": None}), M, "truncated or no is_success", updates_per_iteration=0)
    refuse_train("a ring without is_success", edited(L, **{"ring.is_success": None}), M, "truncated or no is_success", updates_per_iteration=0)
    for every in (0, -1):
        refuse_train(f"log_every = {every}", L, edited(M, log_every=every), "log_every")
    refuse_train("first_iteration = -1", L, edited(M, first_iteration=-1), "first_iteration is negative")
    refuse_train("first_iteration beyond int64", L, edited(M, first_iteration=2 ** 63 - 2), "int64")
    refuse_train("first_record = -1", L, edited(M, first_record=-1), "first_record")
    refuse_train("one record too few", L, edited(M, record_capacity=1), "record_capacity")
    refuse_train("one record too few from the cursor", L, edited(M, first_record=mon.capacity - 1), "record_capacity")
    refuse_train("monitoring.reserved0", L, edited(M, reserved0=1), "reserved0")
    refuse_train("learner.reserved0", edited(L, reserved0=1), M, "reserved0")
    refuse_train("ring.reserved0", edited(L, **{"ring.reserved0": 1}), M, "reserved0")
    # every refusal of the composed call: one of the training call's, one of the schedule's
    refuse_train("online == target", edited(L, target=L.online), M, "the online critic itself")
    refuse_train("num_iterations = 0", L, M, "num_iterations", num_iterations=0)
    # a call without an update still validates the monitoring
    refuse_train("log_every = 0 without updates", L, edited(M, log_every=0), "log_every", updates_per_iteration=0)
    # with an evaluation: its refusals carry this call's name
    E = _abi.SacEvaluation()
    S = _abi.SacSchedule(*[ok[n] for n, _ in _abi.SacSchedule._fields_])
    rc = lib.urgym_sac_train_monitored(env._h, C.byref(L), C.byref(S), C.byref(E), C.byref(M), env._stream())
    refuse("train: an evaluation without a handle", rc, "urgym_sac_train_monitored", "eval_handle is null")
    assert lib.urgym_sac_train_monitored(None, C.byref(L), C.byref(S), None, C.byref(M), None) == _abi.ERR_ARG

    # the Python layer's own checks: ValueError before the library is called
    with pytest.raises(ValueError, match="float64"):
        env.monitor_fold(dict(mon.state, sum_return=mon.state["sum_return"].float()), replay, 0, 1)
    with pytest.raises(ValueError, match="state must be a dict"):
        env.monitor_fold({k: v for k, v in mon.state.items() if k != "episodes"}, replay, 0, 1)
    with pytest.raises(ValueError, match="shape"):
        env.monitor_fold(dict(mon.state, episodes=mon.state["episodes"][:5]), replay, 0, 1)
    with pytest.raises(ValueError, match="at most the ring's"):
        env.monitor_fold(mon.state, replay, 0, CAP + 1)
    with pytest.raises(ValueError, match="first_slot"):
        env.monitor_fold(mon.state, replay, CAP, 1)
    with pytest.raises(ValueError, match="DeviceReplay"):
        env.monitor_fold(mon.state, object(), 0, 1)
    with pytest.raises(ValueError, match="auto_reset"):
        off_env.monitor_fold(mon.state, DeviceReplay(off_env, CAP), 0, 1)
    with pytest.raises(ValueError, match="auto_reset"):
        DeviceMonitor(off_env)
    with pytest.raises(ValueError, match="capacity"):
        DeviceMonitor(env, capacity=0)
    with pytest.raises(ValueError, match="record"):
        env.monitor_stats(mon.state, mon.records[0][:8], 0)
    with pytest.raises(ValueError, match="iteration"):
        env.monitor_stats(mon.state, mon.records[0], 1 << 63)
    sched = dict(first_slot=0, filled_steps=4, num_iterations=4, updates_per_iteration=1)
    with pytest.raises(ValueError, match="go together"):
        env.sac_train(binding, *losses, monitor=mon, **sched)
    with pytest.raises(ValueError, match="log_every"):
        env.sac_train(binding, *losses, monitor=mon, log_every=0, **sched)
    with pytest.raises(ValueError, match="DeviceMonitor"):
        env.sac_train(binding, *losses, monitor=object(), log_every=2, **sched)
    other = object.__new__(DeviceMonitor)
    other.env = off_env
    with pytest.raises(ValueError, match="of this environment"):
        env.sac_train(binding, *losses, monitor=other, log_every=2, **sched)
    full = DeviceMonitor(env, capacity=1)
    with pytest.raises(NativeError, match="record_capacity"):  # two records into one: refused by the library, nothing advanced
        env.sac_train(binding, *losses, monitor=full, log_every=2, **sched)
    assert (full.count, full.iterations) == (0, 0)
    full.record(1)
    with pytest.raises(ValueError, match="records are used"):
        full.record(2)

    # nothing was launched: every byte is what it was
    torch.cuda.synchronize(dev)
    assert torch.equal(everything(), before) and torch.isnan(losses).all()
    assert (mon.count, mon.iterations) == (0, 0) and len(refused) > 50, len(refused)
    for name in _abi.SAC_LEARNER_LOSSES:
        setattr(L, name, None)
    off_env.close(), a.close()
