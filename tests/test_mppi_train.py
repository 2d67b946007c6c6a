"""GPU tests (-m gpu) of the planner inside the native training call and of the plan statistics (include/urgym.h, "the planner inside the
training call"): urgym_mppi_stats against its numpy restatement (ur_gym_amd.evaluation.mppi_plan_stats),
SACLearner.train(planner=) against the Python loop it promises to be (collect(planner=), update x G, sync_planner, monitor.record,
planner.stats), as two calls against one, with every learner option, against urgym_mppi_control(_guided) at explore_sigma = 0, the slots
it must not write, every refusal, and train without a planner against train as it was.

Shapes: E = 3 source envs with a time limit of 3 steps, K = 5 samples, H = 2, hidden width 32, batch 64, a ring of 6 slots (it wraps),
learning_starts = 4 x steps_per_iteration so that the first iteration runs no update.  Every array lies between guard words.
"""
import ctypes as C

import numpy as np
import pytest

from mppi_collect_cases import E
from mppi_train_cases import GPU_COUNTS, plain, plan_buffers, plan_record_slots, record_of, same_record, unplanned_buffers
from test_mppi_collect import ALL, CONFIGS, HC, K, SHORT, Side, assert_same_everything, close, guarded_replay, pattern_like, pattern_slots
from test_mppi_elite import guard
from test_mppi_guide import actor_path, check, critic_paths, guards_intact, make_vec, np_, refused, same_bits
from test_sac_train import ALLOCATIONS_AND_VIEWS, assert_same_losses
from test_sac_train import Side as SacSide
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import (DeviceEvaluation, DeviceMonitor, DeviceMPPI, DevicePrioritizedReplay, DeviceReplay, evaluation_points, monitor_points,
                                   mppi_plan_stats)

pytestmark = pytest.mark.gpu

SIGMA, UPDATE_SEED, FIRST_DRAW, CAP = 0.3, 11, 7, 6
MODES = dict(CONFIGS, adaptive=dict(elites=3, adapt_std=True, iterations=2))
WHO = "urgym_sac_train_planned"


class TrainSide(Side):
    """test_mppi_collect.Side with the env, the planner's mode and the warm-up chosen: an env that has been reset, a SACLearner on it
    whose first iteration of `steps` steps is idle, a planner guided (where the mode has a guide) by the learner's own initial
    parameters, a guarded ring, a monitor and guarded plan-statistics records; the same bits whichever side it is."""

    def __init__(self, env_id="UR5OriReach-v1", mode="value_policy", steps=1, replay=DeviceReplay, capacity=CAP, **hp):
        from ur_gym_amd.training import SACLearner, host_arrays

        self.env = make_vec(env_id, E, 21, **SHORT)
        self.env.reset(seed=21)
        self.learner = SACLearner(self.env, seed=5, hidden_width=32, batch_size=64, learning_starts=4 * steps, **ALL, **hp)
        options = MODES[mode]
        nets = dict(actor=host_arrays(self.learner.actor.tensors()), critic=host_arrays(self.learner.critic.tensors())) if options.get("terminal_value") else {}
        self.mppi = DeviceMPPI(self.env, samples=K, horizon=HC, sigma=0.3, lam=20.0, gamma=0.95, seed=8, keep_weights=True, **nets, **options)
        self.mppi_guards = guard(self.mppi)
        self.replay, self.ring_guards = guarded_replay(self.env, capacity, replay)
        self.monitor = DeviceMonitor(self.env, capacity=8)
        self.record_guards, self.mppi.records = pattern_like(self.mppi.records[:8])
        self.losses = []

    def loop(self, iterations, steps, updates, first_draw, log_every=1, sigma=SIGMA, sync=True, evaluation=None, eval_every=None):
        """The loop of tools/train_sac.py --planner, with the monitor's and the planner's records where ``train`` places them."""
        lr, mon, draw = self.learner, self.monitor, first_draw
        for _ in range(iterations):
            lr.collect(self.replay, steps, monitor=mon, planner=self.mppi, explore_sigma=sigma)
            if not lr.env_steps * E < lr.hp["learning_starts"]:
                before = lr.adam_state["step"]
                for _ in range(updates):
                    got = lr.update(self.replay, UPDATE_SEED, draw)
                    self.losses.append({k: v.clone() for k, v in got.items()})
                    draw += 1
                if sync and updates:
                    lr.sync_planner(self.mppi)
            mon.iterations += 1
            if mon.iterations % log_every == 0:
                slot = mon.record(mon.iterations)
                self.mppi.stats(iteration=mon.iterations, out=self.mppi.records[slot])
            if evaluation is not None and not lr.env_steps * E < lr.hp["learning_starts"] and lr.adam_state["step"] // eval_every > before // eval_every:
                evaluation.evaluate(lr.actor.tensors())
        return draw

    def state(self):
        """Everything a call may write but the losses: test_sac_train.Side.state (ring, bound buffers, parameters, moments, gradients,
        packed buffers, the target) and the planner's packed actor and critic, the monitor and the plan-statistics records."""
        out = SacSide.state(self)
        if self.mppi.actor is not None:
            out["planner.packed.actor"] = self.mppi.actor.packed()
        if self.mppi.critic is not None:
            out["planner.packed.critic"] = self.mppi.critic.packed()
        out.update({f"monitor.{k}": v for k, v in self.monitor.state.items()})
        out["monitor.records"] = self.monitor.records[:self.monitor.count]
        out["plan.records"] = self.mppi.records[:self.monitor.count]
        return out

    def counters(self):
        return dict(SacSide.counters(self), iterations=self.monitor.iterations, records=self.monitor.count)

    def intact(self):
        return guards_intact(self.mppi_guards) and guards_intact(self.ring_guards) and guards_intact({"records": self.record_guards})


def bits(x):
    return np_(x).tobytes() if hasattr(x, "detach") else np.ascontiguousarray(x).tobytes()


def assert_same_sides(a, b, what):
    import torch

    torch.cuda.synchronize()
    sa, sb = a.state(), b.state()
    assert sa.keys() == sb.keys(), what
    for k in sa:
        assert bits(sa[k]) == bits(sb[k]), (what, k)
    assert a.counters() == b.counters(), (what, a.counters(), b.counters())
    assert_same_everything(a.mppi, b.mppi, what)
    assert a.intact() and b.intact(), what


def train(side, iterations, steps, updates, first_draw, log_every=1, sigma=SIGMA, **options):
    return side.learner.train(side.replay, iterations, steps, updates, seed=UPDATE_SEED, first_draw=first_draw, monitor=side.monitor, log_every=log_every,
                              planner=side.mppi, explore_sigma=sigma, plan_stats=True, **options)


# ------------------------------------------------------------------------------------------------ 1. the statistics launch
def stats_call(lib, env, buffers, iteration):
    """One urgym_mppi_stats on copies of `buffers` between guard words.  Returns (the record's bytes, the guarded tensors, the views)."""
    import torch

    full, view = {}, {}
    for name, array in buffers.items():
        full[name], view[name] = pattern_like(torch.from_numpy(array))
        view[name].copy_(torch.from_numpy(array))
    full["record"], record = pattern_like(torch.zeros(_abi.MPPI_STATS_RECORD_WORDS, dtype=torch.int64))
    M, A = _abi.Mppi(), _abi.MppiAdapt()
    M.num_parents = buffers["best_return"].shape[0]
    for name in ("best_return", "nominal_return", "ess"):
        setattr(M, name, C.cast(view[name].data_ptr(), C.POINTER(C.c_double)))
    adaptive = "elite_count" in buffers
    if adaptive:
        A.elite_count, A.threshold = C.cast(view["elite_count"].data_ptr(), C.POINTER(C.c_int32)), C.cast(view["threshold"].data_ptr(), C.POINTER(C.c_double))

    def launch():
        check(lib.urgym_mppi_stats(env._h, C.byref(M), C.byref(A) if adaptive else None, C.cast(record.data_ptr(), C.POINTER(_abi.MppiStatsRecord)), iteration,
                                   env._stream()), env)
        torch.cuda.synchronize()
        return np_(record).tobytes()

    return launch, full, view, (M, A, record)


def test_stats_launch_is_the_restatement():
    """urgym_mppi_stats at E = 1, 3, 1025 and 65536 on made-up diagnostics with a -inf best_return, a NaN and a +inf nominal_return and a
    NaN ess, on diagnostics where no parent planned, with and without the adapt fields: the record is bitwise mppi_plan_stats, a second
    launch writes the same bits, and nothing but the record is written."""
    lib = _native.lib()
    env = make_vec("UR5OriReach-v1", 1, 0)  # names the device; the launch needs no bound environment
    for count in GPU_COUNTS:
        for make in (plan_buffers, unplanned_buffers):
            whole = make(count)
            for buffers in (whole, plain(whole)):
                launch, full, view, _ = stats_call(lib, env, buffers, 40 + count)
                raw = launch()
                same_record(record_of(raw), mppi_plan_stats(**buffers, iteration=40 + count))
                assert launch() == raw, count  # the order of every sum depends on E alone
                assert guards_intact(full) and all(same_bits(np_(view[k]), buffers[k]) for k in buffers), count
    # parent 0 alone: every mean is its own value
    one = dict(best_return=np.array([-12.5]), nominal_return=np.array([-20.25]), ess=np.array([3.5]), elite_count=np.array([2], np.int32), threshold=np.array([-14.0]))
    launch, full, _, _ = stats_call(lib, env, one, -1)
    rec = record_of(launch())
    assert (rec["mean_best_return"], rec["mean_nominal_return"], rec["mean_gain"], rec["mean_ess"], rec["min_ess"]) == (-12.5, -20.25, 7.75, 3.5, 3.5)
    assert (rec["mean_elite_count"], rec["mean_threshold"], rec["iteration"], rec["num_parents"]) == (2.0, -14.0, -1, 1)
    assert (rec["planned"], rec["nominal_finite"], rec["gain_count"], rec["threshold_count"], rec["reserved0"]) == (1, 1, 1, 1, 0) and guards_intact(full)
    env.close()


def test_stats_refusals_launch_nothing():
    import torch

    lib = _native.lib()
    env = make_vec("UR5OriReach-v1", 1, 0)
    launch, full, view, (M, A, record) = stats_call(lib, env, plan_buffers(3), 0)
    rec = C.cast(record.data_ptr(), C.POINTER(_abi.MppiStatsRecord))
    who, s = "urgym_mppi_stats", env._stream()

    def edited(struct, **fields):
        new = type(struct).from_buffer_copy(struct)
        for name, value in fields.items():
            setattr(new, name, value)
        return new

    refused(lib.urgym_mppi_stats(None, C.byref(M), C.byref(A), rec, 0, s), None, "null handle")
    refused(lib.urgym_mppi_stats(env._h, None, C.byref(A), rec, 0, s), env, who, "null urgym_mppi")
    refused(lib.urgym_mppi_stats(env._h, C.byref(M), C.byref(A), None, 0, s), env, who, "null record_dev")
    for n in (0, -1, 65537):
        refused(lib.urgym_mppi_stats(env._h, C.byref(edited(M, num_parents=n)), C.byref(A), rec, 0, s), env, who, "num_parents")
    for name in ("best_return", "nominal_return", "ess"):
        refused(lib.urgym_mppi_stats(env._h, C.byref(edited(M, **{name: None})), C.byref(A), rec, 0, s), env, who, "is null")
    for name in ("elite_count", "threshold"):
        refused(lib.urgym_mppi_stats(env._h, C.byref(M), C.byref(edited(A, **{name: None})), rec, 0, s), env, who, "is null")
    odd = C.cast(record.data_ptr() + 4, C.POINTER(_abi.MppiStatsRecord))
    refused(lib.urgym_mppi_stats(env._h, C.byref(M), C.byref(A), odd, 0, s), env, who, "8-byte aligned")
    torch.cuda.synchronize()
    assert guards_intact(full) and (np_(record.view(torch.uint8)) == 0xA5).all()
    env.close()


def test_stats_of_a_real_plan():
    """DeviceMPPI.stats on the buffers a plan left at E = 3, plain and adaptive: the record is mppi_plan_stats of those buffers, its views
    name its fields, and the launch writes nothing else."""
    import torch

    for mode in ("value_policy", "adaptive"):
        side = TrainSide(mode=mode)
        side.mppi.plan(3)
        torch.cuda.synchronize()
        before = {k: np_(v).copy() for k, v in side.mppi.buf.items()}
        got = side.mppi.stats(iteration=5, out=side.mppi.records[2])
        torch.cuda.synchronize()
        names = ("best_return", "nominal_return", "ess") + (("elite_count", "threshold") if mode == "adaptive" else ())
        want = mppi_plan_stats(**{k: before[k] for k in names}, iteration=5)
        same_record(record_of(np_(side.mppi.records).tobytes(), 2), want)
        same_record({k: np_(got[k]) for k in want}, want)
        assert want["planned"] == E and want["num_parents"] == E and np.isfinite(want["mean_best_return"]) and 0.999 <= want["min_ess"] <= K  # ess = Z^2 / Q lies in [1, K] up to the rounding of its three operations
        assert want["mean_gain"] >= 0.0  # the best sample is at least the nominal, which is sample 0
        assert all(same_bits(np_(side.mppi.buf[k]), before[k]) for k in before) and side.intact()
        assert (np_(side.mppi.records[[0, 1, 3, 4, 5, 6, 7]].contiguous().view(torch.uint8)) == 0xA5).all()
        fresh = side.mppi.stats()  # a record of its own
        torch.cuda.synchronize()
        assert int(fresh["iteration"]) == 0 and float(fresh["mean_ess"]) == want["mean_ess"]
        side.close()


# ------------------------------------------------------------------------------------------------ 2. the call against the Python loop
def compare_with_the_python_loop(what, iterations, steps, updates, log_every=1, sync=True, env_id="UR5OriReach-v1", mode="value_policy", replay=DeviceReplay, **hp):
    a, b = (TrainSide(env_id, mode, steps, replay, **hp) for _ in range(2))
    a.loop(iterations, steps, updates, FIRST_DRAW, log_every, sync=sync)
    got = train(b, iterations, steps, updates, FIRST_DRAW, log_every, sync_planner=sync)
    assert len(a.losses) == (iterations - 1) * updates > 0, what  # the first iteration is idle, the others update
    assert_same_losses(a.losses, {k: got[k] for k in ("critic_loss", "actor_loss", "ent_coef_loss")}, what)
    assert_same_sides(a, b, what)
    points = plan_record_slots(0, 0, iterations, log_every)
    assert b.monitor.count == len(points) > 0 and bits(got["plan_stats"]) == bits(b.mppi.records[:len(points)]), what
    stats = b.mppi.plan_stats(0, len(points))
    assert [r["iteration"] for r in stats] == [tag for _, tag in points] and all(r["num_parents"] == E and r["planned"] == E for r in stats), what
    return a, b


@pytest.mark.parametrize("shape", [(4, 1, 2), (3, 2, 1)])
@pytest.mark.parametrize("mode", list(MODES))
def test_train_with_a_planner_is_the_python_loop(mode, shape):
    """ONE urgym_sac_train_planned against collect(planner=, explore_sigma=0.3, monitor=), update x G, sync_planner, monitor.record and
    planner.stats on a twin: every ring tensor, every bound buffer of the source and of the planner env, every buffer of urgym_mppi, guide
    and adapt, every parameter, moment and packed buffer of learner and planner, the target, the losses, the monitor's records and the
    plan-statistics records, bit for bit."""
    iterations, steps, updates = shape
    a, b = compare_with_the_python_loop((mode, shape), iterations, steps, updates, mode=mode)
    if MODES[mode].get("terminal_value"):  # the planner follows the learner: its packed buffers are the learner's after the last sync
        assert same_bits(b.mppi.actor.packed(), b.learner.device_actor.packed()) and same_bits(b.mppi.critic.packed(), b.learner.online.packed())
    if mode == "adaptive":
        assert all(r["threshold_count"] == E and 1.0 <= r["mean_elite_count"] <= 3.0 for r in b.mppi.plan_stats(0, b.monitor.count))
    assert iterations * steps > CAP or pattern_slots(b.replay.ring, list(range(iterations * steps, CAP)))
    close(a, b)


def test_train_with_a_planner_on_the_dynamic_env():
    a, b = compare_with_the_python_loop("dyn", 3, 2, 1, log_every=2, env_id="UR5DynReach-v1")
    assert b.monitor.count == 1 and b.mppi.plan_stats(0, 1)[0]["iteration"] == 2
    close(a, b)


def test_split_calls_equal_the_single_call():
    """2 + 2 iterations against 4, log_every = 3: the counters are handed on, mean is carried, and the record of iteration 3 falls in the
    second call at the index one call gives it."""
    a, b = TrainSide(), TrainSide()
    whole = train(a, 4, 1, 2, FIRST_DRAW, log_every=3)
    first = train(b, 2, 1, 2, FIRST_DRAW, log_every=3)
    second = train(b, 2, 1, 2, FIRST_DRAW + first["critic_loss"].shape[0], log_every=3)
    assert first["plan_stats"].shape[0] == 0 and second["plan_stats"].shape[0] == 1 and plan_record_slots(2, 0, 2, 3) == [(0, 3)]
    for k in ("critic_loss", "actor_loss", "ent_coef_loss"):
        assert bits(whole[k]) == bits(first[k]) + bits(second[k]), k
    assert_same_sides(a, b, "2 + 2")
    assert bits(whole["plan_stats"]) == bits(second["plan_stats"]) and a.mppi.plan_stats(0, 1)[0]["iteration"] == 3
    close(a, b)


def test_without_sync_the_planner_keeps_its_parameters():
    import torch

    a, b = TrainSide(), TrainSide()
    torch.cuda.synchronize()
    before = (b.mppi.actor.packed().copy(), b.mppi.critic.packed().copy())
    a.loop(4, 1, 2, FIRST_DRAW, sync=False)
    train(b, 4, 1, 2, FIRST_DRAW, sync_planner=False)
    assert_same_sides(a, b, "no sync")
    assert same_bits(b.mppi.actor.packed(), before[0]) and same_bits(b.mppi.critic.packed(), before[1])
    assert not same_bits(b.learner.device_actor.packed(), before[0])  # the learner moved, the planner did not follow
    close(a, b)


@pytest.mark.parametrize("option", ["n_steps", "prioritized", "hindsight", "max_grad_norm"])
def test_train_with_a_planner_and_a_learner_option(option):
    hp = dict(n_steps=dict(n_steps=3), prioritized=dict(prioritized=True), hindsight=dict(hindsight=True), max_grad_norm=dict(max_grad_norm=0.5))[option]
    replay = DevicePrioritizedReplay if option == "prioritized" else DeviceReplay
    a, b = compare_with_the_python_loop(option, 4, 1, 2, replay=replay, **hp)
    if option == "prioritized":  # the leaves of exactly the new slots were filled (and those drawn re-weighted): the others stay 0
        leaf = np_(b.replay.leaf)
        assert same_bits(leaf, np_(a.replay.leaf)) and leaf[:4].all() and not leaf[4:].any()
    close(a, b)


def test_train_with_a_planner_and_an_evaluation():
    """An evaluation attached: a third handle on the same device; its records and the best actor equal the loop's."""
    import torch

    sides, evs, envs = [], [], []
    for _ in range(2):
        side = TrainSide()
        test_env = make_vec("UR5OriReach-v1", 4, 33, auto_reset=False, max_episode_steps=3)
        sides.append(side), envs.append(test_env), evs.append(DeviceEvaluation(test_env, side.learner.actor.tensors(), num_steps=3, seed=9, capacity=4))
    (a, b), (ea, eb) = sides, evs
    a.loop(4, 1, 2, FIRST_DRAW, evaluation=ea, eval_every=3)
    train(b, 4, 1, 2, FIRST_DRAW, evaluation=eb, eval_every=3)
    assert_same_sides(a, b, "evaluation")
    assert ea.count == eb.count == len(evaluation_points(1, 4, 2, 1, 3)) == 2
    assert bits(ea.records[:2]) == bits(eb.records[:2]) and all(bits(ea.best[k]) == bits(eb.best[k]) for k in ea.best)
    assert bits(ea.best_mean) == bits(eb.best_mean) and eb.env.device == b.env.device == b.mppi.planner.device
    torch.cuda.synchronize()
    for ev, env in zip(evs, envs):
        ev.close(), env.close()
    close(a, b)


def test_without_noise_the_ring_is_the_closed_loop():
    """explore_sigma = 0: the ring's action, reward and flags are urgym_mppi_control_guided's trajectory on a twin planner that was synced
    by hand, from a learner that ran the Python loop, at the points where the call reloads its own."""
    import torch

    iterations, steps, updates = 3, 2, 1
    a, b, c = (TrainSide(steps=steps) for _ in range(3))
    train(a, iterations, steps, updates, FIRST_DRAW, sigma=0.0)
    lr, draw, record = b.learner, FIRST_DRAW, ("action", "reward", "terminated", "truncated", "is_success")
    trajectory = []
    for _ in range(iterations):
        trajectory.append(c.mppi.run(steps, first_draw=lr.draw, record=record))
        lr.collect(b.replay, steps, planner=b.mppi, explore_sigma=0.0)
        if not lr.env_steps * E < lr.hp["learning_starts"]:
            lr.update(b.replay, UPDATE_SEED, draw)
            draw += 1
            lr.sync_planner(b.mppi), lr.sync_planner(c.mppi)
    torch.cuda.synchronize()
    for key in record:
        want = np.concatenate([np_(t[key]).view(np.uint8) if t[key].dtype == torch.bool else np_(t[key]) for t in trajectory])
        assert same_bits(np_(a.replay.ring[key]), want), key  # 6 steps into 6 slots
    assert_same_everything(a.mppi, c.mppi, "closed loop")
    assert a.intact() and c.intact()
    close(a, b, c)


# ------------------------------------------------------------------------------------------------ 3. no stray writes
def test_no_stray_writes_and_every_slot_once():
    """2 iterations of 1 step from slot 1 of the ring, log_every = 1: slots 0 and 3 .. 5 keep their pattern, the loss slots and the two
    records of each kind are written exactly once (a second call from the same state writes the same bits into fresh ones), the others
    keep theirs, and every guard is intact."""
    import torch

    a, b = TrainSide(), TrainSide()
    for s in (a, b):
        s.replay.cursor = 1
        s.learner.env_steps = 1  # one step per env behind it: the first iteration already updates
    got = train(a, 2, 1, 2, FIRST_DRAW)
    again = train(b, 2, 1, 2, FIRST_DRAW)
    torch.cuda.synchronize()
    assert got["critic_loss"].shape == (4,) and all(np.isfinite(np_(got[k])).all() and bits(got[k]) == bits(again[k]) for k in got)
    assert pattern_slots(a.replay.ring, [0, 3, 4, 5]) and a.intact()
    for name, t in a.replay.ring.items():
        raw = np_(t[1:3].contiguous().view(-1).view(torch.uint8)).reshape(2, -1)
        assert not (raw == 0xA5).all(axis=1).any(), name
    records = np_(a.mppi.records.contiguous().view(torch.uint8)).reshape(8, -1)
    assert not (records[:2] == 0xA5).all(axis=1).any() and (records[2:] == 0xA5).all()
    assert a.monitor.count == 2 and not np_(a.monitor.records[2:]).any() and [r["iteration"] for r in a.mppi.plan_stats(0, 2)] == [1, 2]
    assert_same_sides(a, b, "again")
    close(a, b)


# ------------------------------------------------------------------------------------------------ 4. the refusals
def test_every_refusal_launches_nothing():
    import torch

    from ur_gym_amd.training import host_arrays

    lib = _native.lib()
    side = TrainSide(mode="adaptive")
    guided = TrainSide()
    src, lr, mppi = side.env, side.learner, side.mppi
    tr = lr._train_binding(side.replay)
    L = tr["binding"].struct
    full, loss = {}, {}
    for name in _abi.SAC_LEARNER_LOSSES:
        full[name], loss[name] = pattern_like(torch.zeros(4, dtype=torch.float32))
        setattr(L, name, C.cast(loss[name].data_ptr(), C.POINTER(C.c_float)))
    L.update_seed = UPDATE_SEED
    fields = dict(first_slot=0, filled_steps=0, capacity_steps=CAP, num_iterations=3, steps_per_iteration=1, updates_per_iteration=2, uniform_iterations=0,
                  idle_iterations=1, collect_first_draw=0, update_first_draw=FIRST_DRAW, first_step=1)
    S = _abi.SacSchedule(*[fields[name] for name, _ in _abi.SacSchedule._fields_])
    P = mppi.planning(SIGMA, True, True)
    P.record_capacity = 8
    M = side.monitor.struct(1)
    small = make_vec("UR5OriReach-v1", E * K - 1, 1, auto_reset=False, max_episode_steps=3)
    torch.cuda.synchronize()
    before = dict(SacSide.state(side), **{f"mppi.{k}": v for k, v in mppi.buf.items()}, **{f"planner.{k}": v for k, v in mppi.planner.buf.items()})
    before = {k: bits(v) for k, v in before.items()}
    s = src._stream()

    def edited(struct, **changes):
        new = type(struct).from_buffer_copy(struct)
        for name, value in changes.items():
            setattr(new, name, value)
        return new

    def ref(x):
        return C.byref(x) if x is not None else None

    def call(handle=src._h, learner=L, schedule=S, planning=P, clipping=None, nstep=None, prioritized=None, hindsight=None, evaluation=None, monitoring=M):
        return lib.urgym_sac_train_planned(handle, ref(learner), ref(schedule), ref(planning), ref(clipping), ref(nstep), ref(prioritized), ref(hindsight),
                                           ref(evaluation), ref(monitoring), s)

    def no(*words, **changes):
        refused(call(**changes), src, WHO, *words)

    refused(call(handle=None), None, "null handle")
    no("null planning", planning=None)
    no("null learner", learner=None)
    no("null schedule", schedule=None)
    no("planner_handle is null", planning=edited(P, planner_handle=None))
    no("mppi is null", planning=edited(P, mppi=None))
    no("reserved0", planning=edited(P, reserved0=1))
    no("record_capacity is negative", planning=edited(P, record_capacity=-1))
    no("nothing to plan", schedule=edited(S, steps_per_iteration=0, filled_steps=1))
    no("uniform_iterations", schedule=edited(S, uniform_iterations=1))
    no("training handle", planning=edited(P, planner_handle=src._h))
    no("the planner has", planning=edited(P, planner_handle=small._h))
    no("eval_handle", evaluation=edited(_abi.SacEvaluation(), eval_handle=mppi.planner._h))
    no("without monitoring", monitoring=None)
    no("record_capacity", planning=edited(P, record_capacity=2))  # three record points
    no("record_capacity", planning=edited(P, record_capacity=4), monitoring=edited(M, first_record=2))
    no("8-byte aligned", planning=edited(P, records=C.cast(mppi.records.data_ptr() + 4, C.POINTER(_abi.MppiStatsRecord))))
    # what urgym_mppi_collect(_adaptive) refuses about mppi, adapt, guide, explore and the draws
    for changes, word in ((dict(samples=1), "samples"), (dict(horizon=0), "horizon"), (dict(iterations=9), "iterations"), (dict(lam=0.0), "lam"),
                          (dict(reserved0=1), "reserved"), (dict(num_parents=E + 1), "the source has"), (dict(best_return=None), "best_return is null")):
        no(word, planning=edited(P, mppi=C.pointer(edited(mppi.struct(), **changes))))
    for changes, word in ((dict(elites=0), "elites"), (dict(std_min=1.0, std_max=0.5), "std_min"), (dict(threshold=None), "threshold is null")):
        no(word, planning=edited(P, adapt_or_NULL=C.pointer(edited(mppi.adapt(), **changes))))
    G = guided.mppi.guide()  # of another planner handle: its actor is not this planner's
    no("not an actor of the planner handle", planning=edited(P, guide_or_NULL=C.pointer(G)))
    for value in (float("nan"), float("inf"), -0.5):
        no("explore_sigma", planning=edited(P, explore=_abi.MppiExplore(value, 0, None)))
    no("reserved0", planning=edited(P, explore=_abi.MppiExplore(0.3, 1, None)))
    no("2^32", schedule=edited(S, collect_first_draw=(1 << 32) - 2))
    no("2^32", schedule=edited(S, collect_first_draw=1 << 32))
    # what the existing options refuse, under this entry point's name
    no("capacity_steps", schedule=edited(S, capacity_steps=CAP + 1))
    no("max_grad_norm", clipping=_abi.SacClipping(float("nan"), 0, None, None, None))
    no("at most one of", nstep=_abi.SacNstep(2, 0, None, None), hindsight=_abi.SacHindsight(0, 0, 3, 0))
    no("log_every", monitoring=edited(M, log_every=0))
    no("urgym_sac_learner.actor is null", learner=edited(L, actor=None))
    # sync: the guide's actor and critic must have the learner's shapes
    for nets, word in ((dict(actor=actor_path("UR5OriReach-v1"), critic=critic_paths("UR5OriReach-v1")), "the guide's actor"),
                       (dict(actor=host_arrays(lr.actor.tensors()), critic=critic_paths("UR5OriReach-v1")), "the guide's critic")):
        wide = DeviceMPPI(src, samples=K, horizon=HC, sigma=0.3, lam=20.0, gamma=0.95, seed=8, **nets, **CONFIGS["value_policy"])
        no("sync", word, planning=wide.planning(SIGMA, True, False), monitoring=None)
        wide.close()
    torch.cuda.synchronize()
    after = dict(SacSide.state(side), **{f"mppi.{k}": v for k, v in mppi.buf.items()}, **{f"planner.{k}": v for k, v in mppi.planner.buf.items()})
    assert all(bits(v) == before[k] for k, v in after.items())
    assert guards_intact(full) and all((np_(t.view(torch.uint8)) == 0xA5).all() for t in loss.values())
    assert pattern_slots(side.replay.ring, slice(None)) and (np_(mppi.records.contiguous().view(torch.uint8)) == 0xA5).all() and side.intact()
    assert not np_(side.monitor.records).any() and not any(np_(v).any() for v in side.monitor.state.values())
    for name in _abi.SAC_LEARNER_LOSSES:
        setattr(L, name, None)
    # the ValueErrors of train, before anything runs
    other, normalized = TrainSide(), TrainSide(normalize=True)
    counters = side.counters()
    for message, run in (("normalize", lambda: train(normalized, 2, 1, 1, 0)),
                         ("planner's source env", lambda: side.learner.train(side.replay, 2, 1, 1, seed=1, first_draw=0, planner=other.mppi)),
                         ("explore_sigma", lambda: side.learner.train(side.replay, 2, 1, 1, seed=1, first_draw=0, explore_sigma=0.3)),
                         ("plan_stats", lambda: side.learner.train(side.replay, 2, 1, 1, seed=1, first_draw=0, planner=side.mppi, plan_stats=True)),
                         ("plan_stats", lambda: side.learner.train(side.replay, 2, 1, 1, seed=1, first_draw=0, plan_stats=True)),
                         ("explore_sigma", lambda: side.learner.train(side.replay, 2, 1, 1, seed=1, first_draw=0, planner=side.mppi, explore_sigma=-1.0))):
        with pytest.raises(ValueError, match=message):
            run()
    torch.cuda.synchronize()
    assert side.counters() == counters and pattern_slots(side.replay.ring, slice(None)) and pattern_slots(normalized.replay.ring, slice(None))
    assert (normalized.learner.env_steps, normalized.replay.filled, normalized.monitor.iterations) == (0, 0, 0)
    small.close()
    close(side, guided, other, normalized)


# ------------------------------------------------------------------------------------------------ 5. a learner without a planner
class Calls:
    """Records which urgym_sac_train* entry points a block calls, and passes every call on."""

    def __init__(self, env):
        self.env, self.lib, self.names = env, env.lib, []

    def __getattr__(self, name):
        if name.startswith("urgym_sac_train"):
            self.names.append(name)
        return getattr(self.lib, name)

    def __enter__(self):
        self.env.lib = self
        return self

    def __exit__(self, *exc):
        self.env.lib = self.lib


def test_train_without_a_planner_is_the_call_of_before():
    """planner=None against the call without the keyword: the same entry point, the same bits; and with a planner the one new symbol."""
    import torch

    a, b, c = TrainSide(), TrainSide(), TrainSide()
    with Calls(a.env) as ca:
        la = a.learner.train(a.replay, 4, 1, 2, seed=UPDATE_SEED, first_draw=FIRST_DRAW, monitor=a.monitor, log_every=2)
    with Calls(b.env) as cb:
        lb = b.learner.train(b.replay, 4, 1, 2, seed=UPDATE_SEED, first_draw=FIRST_DRAW, monitor=b.monitor, log_every=2, planner=None, explore_sigma=0.0,
                             sync_planner=True, plan_stats=False)
    with Calls(c.env) as cc:
        train(c, 4, 1, 2, FIRST_DRAW)
    torch.cuda.synchronize()
    assert ca.names == cb.names == ["urgym_sac_train_monitored"] and cc.names == [WHO]
    assert sorted(la) == sorted(lb) == ["actor_loss", "critic_loss", "ent_coef_loss"] and all(bits(la[k]) == bits(lb[k]) for k in la)
    assert_same_sides(a, b, "no planner")
    assert (np_(a.mppi.records.contiguous().view(torch.uint8)) == 0xA5).all() and not any(np_(v).any() for k, v in a.mppi.buf.items())  # the planner was never asked
    close(a, b, c)


def test_train_with_a_planner_runs_no_torch_operation_that_launches():
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode

    class Recorder(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.append(str(func))
            return func(*args, **(kwargs or {}))

    s = TrainSide()
    train(s, 2, 1, 2, FIRST_DRAW)  # warms: the scratch and the structs exist afterwards
    with Recorder() as rec:
        got = train(s, 2, 1, 2, FIRST_DRAW + 2)
    torch.cuda.synchronize()
    print(f"{len(rec.names)} torch operations in one train call with a planner: {sorted(set(rec.names))}")
    assert got["critic_loss"].shape == (4,) and got["plan_stats"].shape == (2, _abi.MPPI_STATS_RECORD_WORDS) and "aten.empty.memory_format" in rec.names
    assert set(rec.names) <= ALLOCATIONS_AND_VIEWS, sorted(set(rec.names) - ALLOCATIONS_AND_VIEWS)
    assert len(rec.names) <= 10  # and their number does not grow with the iterations
    assert [r["iteration"] for r in s.mppi.plan_stats(0, 4)] == [1, 2, 3, 4] and monitor_points(2, 2, 1) == [0, 1]
    s.close()
