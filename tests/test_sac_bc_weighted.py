"""GPU tests (-m gpu) of advantage-weighted cloning in SAC's policy loss on the device:
urgym_sac_policy_terms_weighted / env.policy_terms_weighted, urgym_sac_train_weighted / env.sac_train(weighting=) and
SACLearner(bc_weight=, bc_advantage_temperature=, bc_advantage_max_weight=).

The launch is compared BIT FOR BIT with evaluation.policy_terms_weighted (the header restated in numpy), with
urgym_sac_policy_terms_cloned (masked) where the weights are all one, and with urgym_sac_policy_terms on the rows that are not eligible;
the learner with the sequence of single calls and the restated terms; ``train`` with the Python loop of ``collect`` and ``update`` on a
twin made from the same seeds.  The learner's shapes: 8 envs, hidden width 32, a batch of 64 rows, a ring of 4 slots, 3 to 4 iterations.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import sac_bc_weighted_cases as wc
from sac_bc_weighted_cases import FLT_MAX, FORMS, GPU_COUNTS, MASKS, WEIGHT, same
from test_sac_bc import Calls, same_but_nan
from test_sac_terms import ALLOCATIONS_AND_VIEWS, Guarded
from test_sac_train import ALL, Side, bits, guarded, guards_intact
from ur_gym_amd import _abi, make_vec
from ur_gym_amd.evaluation import DeviceMPPI, DeviceReplay, policy_terms, policy_terms_weighted
from ur_gym_amd.training import SACLearner, host_arrays

pytestmark = pytest.mark.gpu

NAN = np.float32("nan")
INPUTS = ("log_prob", "q", "y", "q_min", "dqmin_da", "action_pi", "action_data")
FLOAT_OUTPUTS = ("d_action", "critic_loss", "actor_loss", "bc_loss", "bc_weight", "adv_ess", "adv_max")
INT_OUTPUTS = ("bc_rows", "adv_clipped")
BEFORE = -7  # what the two counts hold before a call


@pytest.fixture(scope="module")
def env():
    e = make_vec("UR5OriReach-v1", num_envs=64, seed=3, auto_reset=True)
    e.reset(seed=3)
    yield e
    e.close()


class Case:
    """Inputs and NaN-filled outputs of urgym_sac_policy_terms_weighted at one count on the device, every tensor between guard words."""

    def __init__(self, env, count, variant="plain"):
        self.env, self.count = env, count
        self.x = x = wc.inputs(count, variant)
        host = {k: x[k] for k in INPUTS}
        host.update(ent_coef=np.full(1, x["alpha"]), d_action=np.full((count, 6), NAN), other_d_action=np.full((count, 6), NAN))
        host.update({k: np.full(1, NAN) for k in FLOAT_OUTPUTS[1:] + ("other_critic_loss", "other_actor_loss", "other_bc_loss", "other_bc_weight")})
        self.g = Guarded(host, env.device)
        self.ints = {k: guarded((1,), torch.int32, env.device, fill=BEFORE) for k in INT_OUTPUTS + ("other_bc_rows",)}
        self.mask = guarded((count,), torch.uint8, env.device, fill=0)
        self.mask[1].copy_(torch.from_numpy(x["mask"]))

    def terms(self, d_action="d_action", prefix=""):
        t = self.g.t
        return dict(dqmin_da=t["dqmin_da"], scale=-1.0 / self.count, d_action_out=t[d_action], q=t["q"], y=t["y"], critic_loss_out=t[prefix + "critic_loss"],
                    log_prob=t["log_prob"], q_min=t["q_min"], actor_loss_out=t[prefix + "actor_loss"])

    def call(self, masked, max_weight, temperature, weight=WEIGHT, scale_by_q=False, d_action="d_action"):
        t = self.g.t
        self.env.policy_terms_weighted(t["ent_coef"], self.count, **self.terms(d_action), action_pi=t["action_pi"], action_data=t["action_data"], weight=weight,
                                       bc_scale=1.0 / self.count, scale_by_q=scale_by_q, bc_loss_out=t["bc_loss"], bc_weight_out=t["bc_weight"],
                                       bc_rows_out=self.ints["bc_rows"][1], temperature=temperature, max_weight=None if max_weight == float("inf") else max_weight,
                                       adv_ess_out=t["adv_ess"], adv_max_out=t["adv_max"], adv_clipped_out=self.ints["adv_clipped"][1],
                                       **(dict(row_mask=self.mask[1]) if masked else {}))

    def cloned(self, masked, scale_by_q=False):
        """urgym_sac_policy_terms_cloned (masked) without the filter on the same inputs, into outputs of its own."""
        t = self.g.t
        fn = self.env.policy_terms_cloned_masked if masked else self.env.policy_terms_cloned
        fn(t["ent_coef"], self.count, **self.terms("other_d_action", "other_"), action_pi=t["action_pi"], action_data=t["action_data"], weight=WEIGHT,
           bc_scale=1.0 / self.count, scale_by_q=scale_by_q, q_filter=False, bc_loss_out=t["other_bc_loss"], bc_weight_out=t["other_bc_weight"],
           bc_rows_out=self.ints["other_bc_rows"][1], **(dict(row_mask=self.mask[1]) if masked else {}))

    def plain(self):
        """urgym_sac_policy_terms on the same inputs, into the other outputs."""
        t = self.g.t
        self.env.policy_terms(t["ent_coef"], self.count, **self.terms("other_d_action", "other_"))

    def outputs(self, prefix=""):
        torch.cuda.synchronize(self.env.device)
        keys = FLOAT_OUTPUTS if not prefix else FLOAT_OUTPUTS[:5]
        out = {k: self.g.host(prefix + k) for k in keys}
        out.update({k: self.ints[prefix + k][1].cpu().numpy() for k in (INT_OUTPUTS if not prefix else INT_OUTPUTS[:1])})
        return out

    def assert_is(self, want, where, eq=same):
        got = self.outputs()
        for k in FLOAT_OUTPUTS:
            assert eq(got[k], np.asarray(want[k], dtype=np.float32).reshape(got[k].shape)), (where, k, got[k], want[k])
        for k in INT_OUTPUTS:
            assert got[k].dtype == np.int32 and got[k][0] == want[k], (where, k, got[k], want[k])
        self.assert_intact(where)
        return got

    def assert_intact(self, where):
        for k in INPUTS:
            assert same_but_nan(self.g.host(k), self.x[k]), (where, k)  # inputs are only read
        assert np.array_equal(self.mask[1].cpu().numpy(), self.x["mask"]), where
        assert self.g.guards_intact() and guards_intact(dict(self.ints, mask=self.mask)) is None, where


# ------------------------------------------------------------------------------------------------ 1. the launch against the restatement
@pytest.mark.parametrize("count", GPU_COUNTS)
def test_weighted_terms_are_the_restatement_bitwise(env, count):
    c = Case(env, count)
    c.plain()
    plain = c.outputs("other_")
    for masked, max_weight, temperature in FORMS:
        where = (count, masked, max_weight, temperature)
        scale_by_q = temperature == 1.0
        want = wc.restate(c.x, count, masked, max_weight, temperature, scale_by_q=scale_by_q)
        c.call(masked, max_weight, temperature, scale_by_q=scale_by_q)
        got = c.assert_is(want, where)
        assert np.isfinite(got["d_action"]).all() and np.isfinite([got[k][0] for k in FLOAT_OUTPUTS[1:]]).all(), where
        # the two losses are bitwise urgym_sac_policy_terms', and so is every row that is not eligible
        assert same(got["critic_loss"], plain["critic_loss"]) and same(got["actor_loss"], plain["actor_loss"]), where
        el = want["eligible"]
        assert same(got["d_action"][~el], plain["d_action"][~el]) and (got["d_action"][el] != plain["d_action"][el]).any(), where
        assert got["bc_rows"][0] == (np.count_nonzero(c.x["mask"]) if masked else count), where
    # the identity: the largest finite temperature, no cap -- the bits of the cloned call without the filter, masked or not
    for masked in MASKS:
        for scale_by_q in (False, True):
            c.cloned(masked, scale_by_q)
            c.call(masked, float("inf"), FLT_MAX, scale_by_q=scale_by_q)
            got, other = c.outputs(), c.outputs("other_")
            for k in FLOAT_OUTPUTS[:5]:
                assert same(got[k], other[k]), (count, masked, scale_by_q, k)
            assert got["bc_rows"][0] == other["bc_rows"][0] and got["adv_clipped"][0] == 0 and got["adv_max"][0] == 1, (count, masked)
            assert got["adv_ess"][0] == np.float32(got["bc_rows"][0]), (count, masked)


@pytest.mark.parametrize("variant", wc.VARIANTS[1:])
def test_input_variants_are_the_restatement_bitwise(env, variant):
    for count in (1, 65, 1025):
        c = Case(env, count, variant)
        c.plain()
        plain = c.outputs("other_")
        for masked, max_weight, temperature in FORMS:
            where = (variant, count, masked, max_weight, temperature)
            want = wc.restate(c.x, count, masked, max_weight, temperature)
            c.call(masked, max_weight, temperature)
            got = c.assert_is(want, where, eq=same_but_nan)
            el = want["eligible"]
            assert same(got["d_action"][~el], plain["d_action"][~el]), where  # NaN placement: a row that is not eligible is policy_terms'
            if variant == "nan_action":  # an eligible row's NaN reaches that row and bc_loss only
                rest = np.ones((count, 6), dtype=bool)
                rest[0, 3] = False
                assert el[0] and np.isnan(got["d_action"][0, 3]) and np.isnan(got["bc_loss"][0]) and np.isfinite(got["d_action"][rest]).all(), where
                assert np.isfinite([got[k][0] for k in ("critic_loss", "actor_loss", "bc_weight", "adv_ess", "adv_max")]).all(), where
            if variant == "nan_action_ineligible":  # the actions of a row that is not eligible reach nothing
                assert not el[count - 1] and np.isfinite(got["d_action"]).all() and np.isfinite(got["bc_loss"][0]), where
            if variant == "zero_mask" and masked:  # n == 0: policy_terms' bits and zeros
                assert same(got["d_action"], plain["d_action"]) and got["bc_rows"][0] == 0 and got["adv_clipped"][0] == 0, where
                assert all(same(got[k], np.zeros(1, np.float32)) for k in ("bc_loss", "adv_ess", "adv_max")), where
            if variant == "one_eligible" and masked:
                assert got["bc_rows"][0] == 1 and got["adv_ess"][0] == 1 and got["adv_max"][0] == 1, where


def test_in_place_and_two_runs_give_the_same_bits(env):
    count = 1025
    runs = []
    for _ in range(2):
        c = Case(env, count)
        c.call(True, 2.0, 1.0, scale_by_q=True, d_action="dqmin_da")  # d_action_out is dqmin_da
        torch.cuda.synchronize(env.device)
        want = wc.restate(c.x, count, True, 2.0, 1.0, scale_by_q=True)
        assert same(c.g.host("dqmin_da"), want["d_action"]) and np.isnan(c.g.host("d_action")).all()
        assert same(c.g.host("bc_loss"), np.full(1, want["bc_loss"])) and c.ints["bc_rows"][1].item() == want["bc_rows"]
        assert c.g.guards_intact() and guards_intact(dict(c.ints, mask=c.mask)) is None
        runs.append([c.g.host(k) for k in ("dqmin_da",) + FLOAT_OUTPUTS[1:]] + [c.ints[k][1].cpu().numpy() for k in INT_OUTPUTS])
    assert all(same(a, b) if a.dtype == np.float32 else np.array_equal(a, b) for a, b in zip(*runs))
    c = Case(env, 4097)  # the same launch twice from one state
    c.call(False, 2.0, 1.0)
    first = c.outputs()
    c.call(False, 2.0, 1.0)
    second = c.outputs()
    assert all(same(first[k], second[k]) for k in FLOAT_OUTPUTS) and all(first[k][0] == second[k][0] for k in INT_OUTPUTS)


def test_stream_order_without_a_synchronisation(env):
    """Two launches on one set of inputs with q_min rewritten between them by a device copy, nothing synchronised in between: the first
    reads the first q_min, the second the second, and each leaves its own outputs."""
    count = 1025
    c, other = Case(env, count), Case(env, count)  # other's outputs receive the second launch
    first, second = c.x["q_min"].copy(), -c.x["q_min"][::-1].copy()
    dev = [torch.from_numpy(a).to(env.device) for a in (first, second)]
    t, o = c.g.t, other.g.t
    torch.cuda.synchronize(env.device)
    t["q_min"].copy_(dev[0])
    c.call(False, 2.0, 1.0)
    t["q_min"].copy_(dev[1])  # in host time the first launch may not have run yet
    env.policy_terms_weighted(t["ent_coef"], count, dqmin_da=t["dqmin_da"], scale=-1.0 / count, d_action_out=o["d_action"], q=t["q"], y=t["y"],
                              critic_loss_out=o["critic_loss"], log_prob=t["log_prob"], q_min=t["q_min"], actor_loss_out=o["actor_loss"], action_pi=t["action_pi"],
                              action_data=t["action_data"], weight=WEIGHT, bc_scale=1.0 / count, bc_loss_out=o["bc_loss"], bc_weight_out=o["bc_weight"],
                              bc_rows_out=other.ints["bc_rows"][1], temperature=1.0, max_weight=2.0, adv_ess_out=o["adv_ess"], adv_max_out=o["adv_max"],
                              adv_clipped_out=other.ints["adv_clipped"][1])
    torch.cuda.synchronize(env.device)
    wants = [wc.restate(dict(c.x, q_min=q), count, False, 2.0, 1.0) for q in (first, second)]
    assert not same(wants[0]["adv_ess"], wants[1]["adv_ess"]) and not same(wants[0]["d_action"], wants[1]["d_action"])
    for case, want in zip((c, other), wants):
        got = case.outputs()
        assert all(same(got[k], np.asarray(want[k]).reshape(got[k].shape)) for k in FLOAT_OUTPUTS) and all(got[k][0] == want[k] for k in INT_OUTPUTS)


# ------------------------------------------------------------------------------------------------ 2. refusals
def test_every_refusal_leaves_state_and_outputs_unchanged(env):
    lib, count = env.lib, 65
    c = Case(env, count)
    t = c.g.t
    fptr = lambda x: C.cast(x.data_ptr(), C.POINTER(C.c_float))  # noqa: E731
    iptr = lambda x: C.cast(x.data_ptr(), C.POINTER(C.c_int32))  # noqa: E731
    good_a = dict(count=count, reserved0=0, scale=-1.0 / count, ent_coef=fptr(t["ent_coef"]), dqmin_da=fptr(t["dqmin_da"]), d_action_out=fptr(t["d_action"]),
                  q=fptr(t["q"]), y=fptr(t["y"]), critic_loss_out=fptr(t["critic_loss"]), log_prob=fptr(t["log_prob"]), q_min=fptr(t["q_min"]),
                  actor_loss_out=fptr(t["actor_loss"]))
    good_b = dict(action_pi=fptr(t["action_pi"]), action_data=fptr(t["action_data"]), weight=WEIGHT, bc_scale=1.0 / count, scale_by_q=1, q_filter=0,
                  bc_loss_out=fptr(t["bc_loss"]), bc_weight_out=fptr(t["bc_weight"]), bc_rows_out=iptr(c.ints["bc_rows"][1]), reserved0=0)
    good_w = dict(temperature=1.0, max_weight=2.0, row_mask=C.cast(c.mask[1].data_ptr(), C.POINTER(C.c_uint8)), adv_ess_out=fptr(t["adv_ess"]),
                  adv_max_out=fptr(t["adv_max"]), adv_clipped_out=iptr(c.ints["adv_clipped"][1]), reserved0=0)
    inf, nan = float("inf"), float("nan")
    cases = [("null clone args", {}, None, {}, b"null clone args"), ("null advantage args", {}, {}, None, b"null advantage args")]
    # everything urgym_sac_policy_terms_cloned refuses
    cases += [(f"args: {k}={v!r}", {k: v}, {}, {}, expect) for k, v, expect in (
        ("count", 0, b"count"), ("count", _abi.SAC_TERMS_MAX_COUNT + 1, b"count"), ("reserved0", 1, b"reserved0"), ("ent_coef", None, b"ent_coef"),
        ("scale", inf, b"scale"), ("scale", nan, b"scale"), ("dqmin_da", None, b"half given"), ("y", None, b"half given"), ("q_min", None, b"half given"))]
    for group in (("dqmin_da", "d_action_out"), ("q", "y", "critic_loss_out"), ("log_prob", "q_min", "actor_loss_out")):
        cases.append((f"no {group[-1]} group", {k: None for k in group}, {}, {}, b"all three groups"))
    cases += [(f"clone: {k}=NULL", {}, {k: None}, {}, b"is null") for k in ("action_pi", "action_data", "bc_loss_out", "bc_weight_out", "bc_rows_out")]
    cases += [(f"clone: {k}={v!r}", {}, {k: v}, {}, expect) for k, v, expect in (
        ("weight", -1.0, b"weight"), ("weight", inf, b"weight"), ("weight", nan, b"weight"), ("bc_scale", inf, b"bc_scale"), ("scale_by_q", 2, b"0 or 1"),
        ("q_filter", 2, b"0 or 1"), ("reserved0", 1, b"reserved0"))]
    cases += [("d_action_out is action_pi", dict(d_action_out=fptr(t["action_pi"])), {}, {}, b"d_action_out is action_pi or action_data")]
    # its own: the other gate, the output pointers, the two numbers, reserved0
    cases += [("clone: q_filter=1", {}, dict(q_filter=1), {}, b"alternatives")]
    cases += [(f"advantage: {k}=NULL", {}, {}, {k: None}, b"is null") for k in ("adv_ess_out", "adv_max_out", "adv_clipped_out")]
    cases += [(f"advantage: {k}={v!r}", {}, {}, {k: v}, expect) for k, v, expect in (
        ("temperature", 0.0, b"temperature"), ("temperature", -1.0, b"temperature"), ("temperature", inf, b"temperature"), ("temperature", nan, b"temperature"),
        ("max_weight", 0.0, b"max_weight"), ("max_weight", -1.0, b"max_weight"), ("max_weight", nan, b"max_weight"), ("reserved0", 1, b"reserved0"))]
    for what, a_over, b_over, w_over, expect in cases:
        a = _abi.SacPolicyArgs(**dict(good_a, **a_over))
        b = None if b_over is None else C.byref(_abi.SacCloneArgs(**dict(good_b, **b_over)))
        w = None if w_over is None else C.byref(_abi.SacAdvantageArgs(**dict(good_w, **w_over)))
        rc = lib.urgym_sac_policy_terms_weighted(env._h, C.byref(a), b, w, env._stream())
        assert rc == _abi.ERR_ARG and expect in lib.urgym_last_error(env._h), (what, rc, lib.urgym_last_error(env._h))
    assert lib.urgym_sac_policy_terms_weighted(env._h, None, C.byref(_abi.SacCloneArgs(**good_b)), C.byref(_abi.SacAdvantageArgs(**good_w)), env._stream()) == _abi.ERR_ARG
    # the binding refuses before the library is asked
    kw = dict(c.terms(), action_pi=t["action_pi"], action_data=t["action_data"], weight=WEIGHT, bc_scale=1.0 / count, scale_by_q=True, bc_loss_out=t["bc_loss"],
              bc_weight_out=t["bc_weight"], bc_rows_out=c.ints["bc_rows"][1], temperature=1.0, max_weight=2.0, adv_ess_out=t["adv_ess"], adv_max_out=t["adv_max"],
              adv_clipped_out=c.ints["adv_clipped"][1], row_mask=c.mask[1])
    for over in (dict(temperature=0.0), dict(temperature=NAN), dict(temperature=True), dict(temperature=1e39), dict(max_weight=0.0), dict(max_weight=NAN), dict(max_weight="2"),
                 dict(q_filter=False), dict(weight=-1.0), dict(row_mask=c.mask[1][:-1]), dict(row_mask=t["bc_loss"]), dict(row_mask=c.x["mask"]), dict(adv_ess_out=t["d_action"]),
                 dict(adv_clipped_out=t["adv_ess"]), dict(action_pi=t["action_pi"][:-1]), dict(d_action_out=t["action_pi"])):
        with pytest.raises(ValueError):
            env.policy_terms_weighted(t["ent_coef"], count, **dict(kw, **over))
    with pytest.raises(ValueError, match="count"):
        env.policy_terms_weighted(t["ent_coef"], 0, **dict(kw))
    got = c.outputs()
    assert all(np.isnan(got[k]).all() for k in FLOAT_OUTPUTS) and all(got[k][0] == BEFORE for k in INT_OUTPUTS)  # nothing was launched, nothing written
    c.assert_intact("refusals")
    env.policy_terms_weighted(t["ent_coef"], count, **kw)  # and the good arguments are good
    c.assert_is(wc.restate(c.x, count, True, 2.0, 1.0, scale_by_q=True), "after the refusals")


# ------------------------------------------------------------------------------------------------ 3. the learner
N, H, M, CAP, STARTS, SEED, UPDATE_SEED, FIRST_DRAW = 8, 32, 64, 4, 16, 5, 11, 7
N_DEMO, CAP_DEMO, D = 3, 3, 17
ADV = dict(bc_weight=0.5, bc_scale_by_q=True, bc_advantage_temperature=0.5, bc_advantage_max_weight=4.0)
ADV_KEYS = ("bc_loss", "bc_weight", "bc_rows", "adv_ess", "adv_max", "adv_clipped")
LOSS_KEYS = ("critic_loss", "actor_loss", "ent_coef_loss")
SIGMA = 0.3


class WeightedSide(Side):
    """test_sac_train's Side at 8 envs, batch 64, episodes of at most 3 steps, the warm-up over after two steps, with the option under
    test; an MPPI planner guided by the learner's own initial parameters, or a demonstration ring a planner filled on a second env of 3
    envs, on request.  The same bits whichever side it is; `seeds` moves every seed (the rebuilt run of the checkpoint test)."""

    def __init__(self, planner=False, demos=False, seeds=0, **over):
        env_id = "UR5OriReach-v1"
        self.env_d = self.replay_d = self.mppi = None
        if demos:
            self.env_d = make_vec(env_id, num_envs=N_DEMO, seed=41, auto_reset=True, max_episode_steps=3)
            self.env_d.reset(seed=41)
            self.replay_d = DeviceReplay(self.env_d, CAP_DEMO)
            mppi = DeviceMPPI(self.env_d, samples=5, horizon=2, sigma=0.3, lam=20.0, gamma=0.95, seed=9)
            self.replay_d.collect_planned(mppi, CAP_DEMO + 2, first_draw=0, explore_sigma=0.1)
            mppi.close()
            over = dict(over, demonstrations=self.replay_d, demo_batch_size=D)
        self.env = make_vec(env_id, num_envs=N, seed=SEED + seeds, auto_reset=True, max_episode_steps=3)
        self.env.reset(seed=SEED + seeds)
        self.learner = SACLearner(self.env, seed=SEED + seeds, hidden_width=H, batch_size=M, learning_starts=STARTS, **dict(ALL, **over))
        self.replay = DeviceReplay(self.env, CAP)
        if planner:
            self.mppi = DeviceMPPI(self.env, samples=5, horizon=2, sigma=0.3, lam=20.0, gamma=0.95, seed=8, actor=host_arrays(self.learner.actor.tensors()),
                                   critic=host_arrays(self.learner.critic.tensors()), terminal_value=True, policy_samples=2, policy_sigma=0.2)

    def loop(self, iterations, K, G, first_draw):
        """The loop of tools/train_sac.py: collect (with the planner where there is one), the updates unless the warm-up still holds, the
        planner's sync.  Returns per update the three losses and, with the option, the six cloning values, copied as they were made."""
        lr, out, draw = self.learner, [], first_draw
        for _ in range(iterations):
            if K:
                lr.collect(self.replay, K, **({} if self.mppi is None else dict(planner=self.mppi, explore_sigma=SIGMA)))
            if lr.env_steps * N < lr.hp["learning_starts"]:
                continue
            for _ in range(G):
                got = lr.update(self.replay, UPDATE_SEED, draw)
                out.append(dict({k: v.clone() for k, v in got.items()}, **{k: lr.last_update[k][0].clone() for k in ADV_KEYS if k in lr.last_update}))
                draw += 1
            if self.mppi is not None and G:
                lr.sync_planner(self.mppi)
        return out

    def train(self, iterations, K, G, first_draw):
        extra = {} if self.mppi is None else dict(planner=self.mppi, explore_sigma=SIGMA)
        return self.learner.train(self.replay, iterations, K, G, seed=UPDATE_SEED, first_draw=first_draw, **extra)

    def state(self):
        out = super().state()
        if self.learner.normalizer is not None:
            out.update({f"norm.{k}": v for k, v in self.learner.normalizer.state.items()})
        if self.mppi is not None:
            out.update({"planner.packed.actor": self.mppi.actor.packed(), "planner.packed.critic": self.mppi.critic.packed()})
            out.update({f"planner.buf.{k}": v for k, v in self.mppi.buf.items()})
        if self.replay_d is not None:
            out.update({f"demo.{k}": v for k, v in self.replay_d.ring.items()})
        return out

    def close(self):
        if self.mppi is not None:
            self.mppi.close()
        super().close()
        if self.env_d is not None:
            self.env_d.close()


def assert_same(a, b, what, skip=(), keys=ADV_KEYS):
    sa, sb = a.state(), b.state()
    assert sa.keys() == sb.keys(), what
    assert sum(k.startswith("param:") for k in sa) == 8 + 12 and sum(k.startswith("moment:") for k in sa) == 2 * (8 + 12)
    for k in sa:
        if not k.startswith(skip):
            assert np.array_equal(bits(sa[k]), bits(sb[k])), (what, k)
    assert a.counters() == b.counters(), (what, a.counters(), b.counters())
    la, lb = a.learner.last_update, b.learner.last_update
    assert sorted(la) == sorted(lb) and set(keys) <= set(la), (what, sorted(la), sorted(lb))
    for k in la:
        assert la[k].shape == lb[k].shape and np.array_equal(bits(la[k]), bits(lb[k])), (what, "last_update", k)


def assert_same_values(want, got, what, keys=LOSS_KEYS + ADV_KEYS):
    assert set(keys) <= set(got) and all(got[k].shape == (len(want),) for k in keys), what
    for u, w in enumerate(want):
        for k in keys:
            assert got[k].dtype == w[k].dtype and np.array_equal(bits(got[k][u]), bits(w[k])), (what, u, k, got[k][u].item(), w[k].item())


def restated(lr, host, **more):
    es, hp = lr.entropy_state, lr.hp
    return policy_terms_weighted(es["ent_coef"].cpu().numpy()[0], dqmin_da=host["dqmin_da"], scale=-1.0 / M, q=host["q"], y=host["y"], log_prob=host["log_prob"],
                                 q_min=host["q_min"], action_pi=host["action_pi"], action_data=host["action_data"], weight=hp["bc_weight"], bc_scale=1.0 / M,
                                 scale_by_q=hp["bc_scale_by_q"], temperature=hp["bc_advantage_temperature"],
                                 max_weight=np.inf if hp["bc_advantage_max_weight"] is None else hp["bc_advantage_max_weight"], **more)


@pytest.mark.parametrize("demos", (False, True))
def test_update_is_the_sequence_of_single_calls_with_the_restated_terms(demos):
    s = WeightedSide(demos=demos, **ADV, **(dict(bc_demo_only=True) if demos else {}))
    lr = s.learner
    lr.collect(s.replay, CAP)
    for draw in range(3):
        losses = lr.update(s.replay, UPDATE_SEED, draw)
        torch.cuda.synchronize(s.env.device)
        last = lr.last_update
        host = {k: v.cpu().numpy() for k, v in last.items()}
        assert host["action_data"].shape == host["action_pi"].shape == (M, 6) and last["bc_rows"].dtype == last["adv_clipped"].dtype == torch.int32
        want = restated(lr, host, **(dict(row_mask=host["source"]) if demos else {}))
        assert same(lr.actor_d_action.cpu().numpy(), want["d_action"]), draw
        assert same(losses["critic_loss"].cpu().numpy(), want["critic_loss"]) and same(losses["actor_loss"].cpu().numpy(), want["actor_loss"]), draw
        for k in ("bc_loss", "bc_weight", "adv_ess", "adv_max"):
            assert same(host[k], np.full(1, want[k])), (draw, k)
        assert host["bc_rows"][0] == want["bc_rows"] == (D if demos else M) and host["adv_clipped"][0] == want["adv_clipped"], draw
        plain = policy_terms(lr.entropy_state["ent_coef"].cpu().numpy()[0], dqmin_da=host["dqmin_da"], scale=-1.0 / M)["d_action"]
        assert same(want["d_action"][~want["eligible"]], plain[~want["eligible"]]) and (want["d_action"][want["eligible"]] != plain[want["eligible"]]).any()
        print(f"demos {demos} update {draw}: bc_loss {host['bc_loss'][0]!r} adv_ess {host['adv_ess'][0]!r} of {want['bc_rows']} adv_max {host['adv_max'][0]!r} "
              f"clipped {host['adv_clipped'][0]}")
    s.close()


OPTIONS = {"plain": {}, "planner": dict(planner=True), "demonstrations_demo_only": dict(demos=True, bc_demo_only=True), "max_grad_norm": dict(max_grad_norm=1e-2),
           "normalize": dict(normalize=True)}


@pytest.mark.parametrize("option", list(OPTIONS))
def test_train_equals_the_python_loop_bit_for_bit(option):
    """ONE native call (urgym_sac_train_weighted with the option's struct) against collect / update (/ sync_planner) on a twin: every
    ring tensor, bound buffer, parameter, moment, gradient, packed buffer, the planner's buffers, the statistics, the demonstrations,
    the losses, the six arrays and last_update, bit for bit."""
    iterations = 3 if option == "planner" else 4
    a, b = WeightedSide(**ADV, **OPTIONS[option]), WeightedSide(**ADV, **OPTIONS[option])
    want = a.loop(iterations, 1, 2, FIRST_DRAW)
    got = b.train(iterations, 1, 2, FIRST_DRAW)
    torch.cuda.synchronize(a.env.device)
    assert len(want) == 2 * (iterations - 1) and all(k in want[0] for k in ADV_KEYS), option
    assert_same_values(want, got, option)
    assert_same(a, b, option)
    rows, ess = got["bc_rows"].cpu().numpy(), got["adv_ess"].cpu().numpy()
    assert (rows == (D if "demo" in option else M)).all() and ((1 <= ess) & (ess <= rows)).all() and np.isfinite(got["bc_loss"].cpu().numpy()).all(), option
    assert (got["adv_max"].cpu().numpy() <= ADV["bc_advantage_max_weight"]).all() and got["adv_clipped"].dtype == torch.int32, option
    if option == "max_grad_norm":
        assert got["critic_grad_norm"].shape == (len(want),)
    if option == "planner":  # the planner follows the learner after the sync
        assert np.array_equal(b.mppi.actor.packed(), b.learner.device_actor.packed()) and np.array_equal(b.mppi.critic.packed(), b.learner.online.packed())
    a.close(), b.close()


def test_split_calls_and_the_learner_without_the_option():
    a, b = WeightedSide(**ADV), WeightedSide(**ADV)
    whole = a.train(4, 1, 2, FIRST_DRAW)
    first = b.train(1, 1, 2, FIRST_DRAW)  # the idle iteration: no update, six empty arrays
    second = b.train(3, 1, 2, FIRST_DRAW)
    torch.cuda.synchronize(a.env.device)
    assert all(first[k].shape == (0,) for k in LOSS_KEYS + ADV_KEYS) and second["adv_ess"].shape == (6,)
    for k in LOSS_KEYS + ADV_KEYS:
        assert np.array_equal(bits(whole[k]), bits(torch.cat([first[k], second[k]]))), k
    d = WeightedSide(**ADV)
    d.train(2, 1, 2, FIRST_DRAW)
    d.train(2, 1, 2, FIRST_DRAW + 2)
    torch.cuda.synchronize(a.env.device)
    assert_same(a, d, "2 + 2 iterations")
    for s in (a, b, d):
        s.close()


NEW_SYMBOLS = ("urgym_sac_policy_terms_weighted", "urgym_sac_train_weighted")


def test_update_launches_what_it_launched_and_no_torch_operation():
    """With the option an update is the thirteen calls of the learner without it, the one policy-terms call replaced; a learner without
    the option -- plain, or cloning alone -- makes the calls it made: neither new symbol, and train ends in the entry point it had."""
    from torch.utils._python_dispatch import TorchDispatchMode

    class Recorder(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.append(str(func))
            return func(*args, **(kwargs or {}))

    seen, results = {}, {}
    for label, over in (("weighted", ADV), ("cloned", dict(bc_weight=0.5, bc_scale_by_q=True)), ("plain", {})):
        s = WeightedSide(**over)
        with Calls(s.env) as calls:
            s.learner.collect(s.replay, CAP)
            s.learner.update(s.replay, UPDATE_SEED, 0)  # whatever is made lazily is made here
            del calls.names[:]
            with Recorder() as rec:
                s.learner.update(s.replay, UPDATE_SEED, 1)
            update = list(calls.names)
            results[label] = s.train(1, 0, 2, 2)
            everything = list(calls.names)
        torch.cuda.synchronize(s.env.device)
        print(f"{label} update: {len(update)} library calls {update}; {len(rec.names)} torch operations: {sorted(set(rec.names))}")
        assert rec.names and "aten.empty.memory_format" in rec.names and set(rec.names) <= ALLOCATIONS_AND_VIEWS, sorted(set(rec.names) - ALLOCATIONS_AND_VIEWS)
        seen[label] = (update, everything, sorted(s.learner.last_update), s.learner.adv_state)
        s.close()
    launches = lambda names: len(names) + sum(n.endswith("_parameter_gradients") for n in names)  # noqa: E731  (those two calls are two launches each)
    assert launches(seen["plain"][0]) == 13 and launches(seen["weighted"][0]) == 13, seen["plain"][0]
    assert seen["weighted"][0] == ["urgym_sac_policy_terms_weighted" if n == "urgym_sac_policy_terms" else n for n in seen["plain"][0]]
    assert seen["cloned"][0] == ["urgym_sac_policy_terms_cloned" if n == "urgym_sac_policy_terms" else n for n in seen["plain"][0]]
    assert seen["weighted"][1][-1] == "urgym_sac_train_weighted" and seen["cloned"][1][-1] == "urgym_sac_train_cloned" and seen["plain"][1][-1] == "urgym_sac_train"
    for label in ("plain", "cloned"):  # a learner without the option calls neither new symbol and reports no new key
        assert not set(NEW_SYMBOLS) & set(seen[label][1]) and seen[label][3] is None
        assert not {"adv_ess", "adv_max", "adv_clipped"} & (set(seen[label][2]) | set(results[label]))
    assert {"adv_ess", "adv_max", "adv_clipped"} <= set(seen["weighted"][2]) and {"adv_ess", "adv_max", "adv_clipped"} <= set(results["weighted"])


def test_learner_without_the_option_matches_a_twin_on_the_existing_calls():
    """SACLearner(bc_weight=) without a temperature: train is bit for bit the loop of collect and update, whose policy terms are the
    restated CLONED terms -- the calls and the bits the learner made before the option existed."""
    from ur_gym_amd.evaluation import policy_terms_cloned

    over = dict(bc_weight=0.5, bc_scale_by_q=True, bc_q_filter=True)
    a, b = WeightedSide(**over), WeightedSide(**over)
    want = a.loop(4, 1, 2, FIRST_DRAW)
    got = b.train(4, 1, 2, FIRST_DRAW)
    torch.cuda.synchronize(a.env.device)
    keys = ("bc_loss", "bc_weight", "bc_rows")
    assert_same_values(want, got, "cloned", keys=LOSS_KEYS + keys)
    assert_same(a, b, "cloned", keys=keys)
    assert sorted(got) == sorted(LOSS_KEYS + keys)
    host = {k: v.cpu().numpy() for k, v in a.learner.last_update.items()}
    terms = policy_terms_cloned(a.learner.entropy_state["ent_coef"].cpu().numpy()[0], dqmin_da=host["dqmin_da"], scale=-1.0 / M, q=host["q"], y=host["y"],
                                log_prob=host["log_prob"], q_min=host["q_min"], action_pi=host["action_pi"], action_data=host["action_data"], weight=0.5, bc_scale=1.0 / M,
                                scale_by_q=True, q_filter=True)
    assert same(a.learner.actor_d_action.cpu().numpy(), terms["d_action"]) and same(host["bc_loss"], np.full(1, terms["bc_loss"]))
    a.close(), b.close()


def test_save_and_load_continue_bit_for_bit(tmp_path):
    a, b = WeightedSide(**ADV), WeightedSide(**ADV)
    a.train(6, 1, 2, FIRST_DRAW)
    b.train(3, 1, 2, FIRST_DRAW)
    path = tmp_path / "run.npz"
    b.learner.save(path, replay=b.replay, extra=dict(update_draw=FIRST_DRAW + b.learner.adam_state["step"]))
    assert {k: b.learner.state_dict()["hp"][k] for k in ADV} == ADV
    b.close()
    one = WeightedSide(seeds=100, bc_weight=0.5, bc_scale_by_q=True)  # a learner without the option refuses the file, and nothing of it is written
    with pytest.raises(ValueError, match="bc_advantage_temperature is 0.5 in the checkpoint, None here"):
        one.learner.load(path, replay=one.replay)
    plain = tmp_path / "plain.npz"  # ... and its own checkpoint holds no new key
    one.learner.collect(one.replay, 2)
    one.learner.save(plain, replay=one.replay)
    assert not {"bc_advantage_temperature", "bc_advantage_max_weight"} & set(one.learner.state_dict()["hp"])
    assert not any("bc_advantage" in k or "adv_" in k for k in np.load(plain, allow_pickle=False).files)
    one.close()
    other = WeightedSide(seeds=100, **dict(ADV, bc_advantage_max_weight=None))
    with pytest.raises(ValueError, match="bc_advantage_max_weight is 4.0 in the checkpoint, None here"):
        other.learner.load(path, replay=other.replay)
    other.close()
    c = WeightedSide(seeds=100, **ADV)  # rebuilt from other seeds
    for t in c.replay.ring.values():
        t.fill_(1)
    extra = c.learner.load(path, replay=c.replay)
    c.train(3, 1, 2, extra["update_draw"])
    torch.cuda.synchronize(a.env.device)
    assert a.learner.seed == c.learner.seed
    assert_same(a, c, "3 + 3", skip=("grad:",))  # the ring has wrapped: every slot holds a collected step
    a.close(), c.close()


def test_every_refusal_of_the_training_call():
    s = WeightedSide(demos=True, **ADV)
    lr, env = s.learner, s.env
    lr.collect(s.replay, CAP)
    before = {k: bits(v).copy() for k, v in s.state().items()}
    tr = lr._train_binding(s.replay)
    tr["binding"].struct.update_seed = UPDATE_SEED
    u = 2
    f32 = lambda: torch.full((u,), NAN, dtype=torch.float32, device=env.device)  # noqa: E731
    i32 = lambda: torch.full((u,), BEFORE, dtype=torch.int32, device=env.device)  # noqa: E731
    losses = [f32() for _ in range(3)]
    cloning = dict(weight=0.5, scale_by_q=True, bc_loss=f32(), bc_weight=f32(), bc_rows=i32())
    weighting = dict(temperature=0.5, max_weight=4.0, adv_ess=f32(), adv_max=f32(), adv_clipped=i32())
    sched = dict(first_slot=s.replay.cursor, filled_steps=s.replay.filled, num_iterations=1, steps_per_iteration=0, updates_per_iteration=u, uniform_iterations=0,
                 idle_iterations=0, collect_first_draw=lr.draw, update_first_draw=0, first_step=1)
    demo = dict(replay=s.replay_d, count=D, source=lr.demo_source, clone_only=True)
    for over, match in ((dict(cloning=None), "needs cloning"), (dict(cloning=dict(cloning, q_filter=True)), "alternatives"),
                        (dict(weighting=dict(weighting, temperature=0.0)), "temperature"), (dict(weighting=dict(weighting, temperature=float("nan"))), "temperature"),
                        (dict(weighting=dict(weighting, max_weight=-1.0)), "max_weight"), (dict(weighting=dict(weighting, adv_ess=f32()[:1])), "adv_ess"),
                        (dict(weighting=dict(weighting, adv_clipped=f32())), "adv_clipped"), (dict(weighting=dict(weighting, beta=1.0)), "unknown weighting options"),
                        (dict(demonstrating=demo, nstep=dict(n_steps=3, discount=torch.zeros((M,), dtype=torch.float32, device=env.device),
                                                                q_min_next=torch.zeros((M,), dtype=torch.float32, device=env.device))), "out of scope")):
        with pytest.raises(ValueError, match=match):
            env.sac_train(tr["binding"], *losses, **sched, **dict(dict(cloning=cloning, weighting=weighting), **over))
    # the library's own refusals, through the raw symbol
    lib = env.lib
    fptr = lambda x: C.cast(x.data_ptr(), C.POINTER(C.c_float))  # noqa: E731
    iptr = lambda x: C.cast(x.data_ptr(), C.POINTER(C.c_int32))  # noqa: E731
    L, sd = tr["binding"].struct, dict(sched, capacity_steps=CAP)
    S = _abi.SacSchedule(*[int(sd[name]) for name, _ in _abi.SacSchedule._fields_])
    for name, t in zip(_abi.SAC_LEARNER_LOSSES, losses):  # a call that is good but for the option under test
        setattr(L, name, fptr(t))
    good_c = _abi.SacCloning(0.5, 1, 0, 0, fptr(cloning["bc_loss"]), fptr(cloning["bc_weight"]), iptr(cloning["bc_rows"]))
    good_w = dict(temperature=0.5, max_weight=4.0, reserved0=0, adv_ess=fptr(weighting["adv_ess"]), adv_max=fptr(weighting["adv_max"]), adv_clipped=iptr(weighting["adv_clipped"]))
    rest = [None] * 11
    call = lambda w, c, *more: lib.urgym_sac_train_weighted(env._h, C.byref(L), C.byref(S), w, c, *(more or rest), env._stream())  # noqa: E731
    assert call(None, C.byref(good_c)) == _abi.ERR_ARG and b"null weighting" in lib.urgym_last_error(env._h)
    assert call(C.byref(_abi.SacWeighting(**good_w)), None) == _abi.ERR_ARG and b"null cloning" in lib.urgym_last_error(env._h)
    for over, expect in ((dict(temperature=0.0), b"temperature"), (dict(temperature=float("inf")), b"temperature"), (dict(max_weight=0.0), b"max_weight"),
                         (dict(max_weight=float("nan")), b"max_weight"), (dict(reserved0=1), b"reserved0")):
        assert call(C.byref(_abi.SacWeighting(**dict(good_w, **over))), C.byref(good_c)) == _abi.ERR_ARG and expect in lib.urgym_last_error(env._h), over
    filtered = _abi.SacCloning(0.5, 1, 1, 0, fptr(cloning["bc_loss"]), fptr(cloning["bc_weight"]), iptr(cloning["bc_rows"]))
    assert call(C.byref(_abi.SacWeighting(**good_w)), C.byref(filtered)) == _abi.ERR_ARG and b"alternatives" in lib.urgym_last_error(env._h)
    torch.cuda.synchronize(env.device)
    after = {k: bits(v) for k, v in s.state().items()}
    assert all(np.array_equal(before[k], after[k]) for k in before)  # nothing was launched
    assert all(torch.isnan(t).all() for t in losses + [cloning["bc_loss"], weighting["adv_ess"], weighting["adv_max"]]) and (weighting["adv_clipped"] == BEFORE).all()
    for name in _abi.SAC_LEARNER_LOSSES:
        setattr(L, name, None)
    s.close()
