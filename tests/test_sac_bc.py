"""GPU tests (-m gpu) of behaviour cloning in SAC's policy loss on the device: urgym_sac_policy_terms_cloned /
env.policy_terms_cloned, urgym_sac_train_cloned / env.sac_train(cloning=) and SACLearner(bc_weight=, bc_scale_by_q=, bc_q_filter=).

The launch is compared BIT FOR BIT with evaluation.policy_terms_cloned (the header restated in numpy) and with urgym_sac_policy_terms on
the same inputs; the learner with the sequence of single calls and the restated terms; ``train`` with the Python loop of ``collect`` and
``update`` on a twin made from the same seeds.  The learner's shapes are the smallest that still cross the boundaries: 8 envs, hidden
width 32, a batch of 65 rows (a second wave with one live lane), a ring of 4 slots, 3 to 4 iterations.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import sac_bc_cases as bc
from sac_bc_cases import FLAGS, GPU_COUNTS, WEIGHT, same
from test_sac_terms import ALLOCATIONS_AND_VIEWS, Guarded
from test_sac_train import ALL, Side, bits, guarded, guards_intact
from ur_gym_amd import _abi, make_vec
from ur_gym_amd._native import NativeError
from ur_gym_amd.evaluation import DeviceMPPI, DevicePrioritizedReplay, DeviceReplay, policy_terms, policy_terms_cloned
from ur_gym_amd.training import SACLearner, host_arrays

pytestmark = pytest.mark.gpu

NAN = np.float32("nan")
INPUTS = ("log_prob", "q", "y", "q_min", "dqmin_da", "action_pi", "action_data")
FLOAT_OUTPUTS = ("d_action", "critic_loss", "actor_loss", "bc_loss", "bc_weight")
ROWS_BEFORE = -7  # what bc_rows holds before a call


def same_but_nan(a, b):
    """Bitwise equal, except that where both hold a NaN the words are not compared (the sign and payload of a propagated NaN are not part
    of the contract)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    a, b = a.reshape(-1), b.reshape(-1)
    both = np.isnan(a) & np.isnan(b)
    return np.array_equal(a[~both].view(np.uint32), b[~both].view(np.uint32))


@pytest.fixture(scope="module")
def env():
    e = make_vec("UR5OriReach-v1", num_envs=64, seed=3, auto_reset=True)
    e.reset(seed=3)
    yield e
    e.close()


class Case:
    """Inputs and NaN-filled outputs of urgym_sac_policy_terms_cloned at one count on the device, every tensor between guard words."""

    def __init__(self, env, count, variant="plain"):
        self.env, self.count = env, count
        self.x = x = bc.inputs(count, variant)
        host = {k: x[k] for k in INPUTS}
        host.update(ent_coef=np.full(1, x["alpha"]), d_action=np.full((count, 6), NAN), plain_d_action=np.full((count, 6), NAN))
        host.update({k: np.full(1, NAN) for k in FLOAT_OUTPUTS[1:] + ("plain_critic_loss", "plain_actor_loss")})
        self.g = Guarded(host, env.device)
        self.rows = guarded((1,), torch.int32, env.device, fill=ROWS_BEFORE)

    def args(self, d_action="d_action"):
        t = self.g.t
        return dict(dqmin_da=t["dqmin_da"], scale=-1.0 / self.count, d_action_out=t[d_action], q=t["q"], y=t["y"], critic_loss_out=t["critic_loss"], log_prob=t["log_prob"],
                    q_min=t["q_min"], actor_loss_out=t["actor_loss"])

    def call(self, scale_by_q, q_filter, weight=WEIGHT, d_action="d_action"):
        t = self.g.t
        self.env.policy_terms_cloned(t["ent_coef"], self.count, **self.args(d_action), action_pi=t["action_pi"], action_data=t["action_data"], weight=weight,
                                     bc_scale=1.0 / self.count, scale_by_q=scale_by_q, q_filter=q_filter, bc_loss_out=t["bc_loss"], bc_weight_out=t["bc_weight"],
                                     bc_rows_out=self.rows[1])

    def plain(self):
        """urgym_sac_policy_terms on the same inputs, into outputs of its own."""
        t = self.g.t
        self.env.policy_terms(t["ent_coef"], self.count, dqmin_da=t["dqmin_da"], scale=-1.0 / self.count, d_action_out=t["plain_d_action"], q=t["q"], y=t["y"],
                              critic_loss_out=t["plain_critic_loss"], log_prob=t["log_prob"], q_min=t["q_min"], actor_loss_out=t["plain_actor_loss"])

    def outputs(self):
        torch.cuda.synchronize(self.env.device)
        out = {k: self.g.host(k) for k in FLOAT_OUTPUTS}
        out["bc_rows"] = self.rows[1].cpu().numpy()
        return out

    def assert_is(self, want, where, eq=same):
        got = self.outputs()
        for k in FLOAT_OUTPUTS:
            assert eq(got[k], np.asarray(want[k], dtype=np.float32).reshape(got[k].shape)), (where, k, got[k], want[k])
        assert got["bc_rows"].dtype == np.int32 and got["bc_rows"][0] == want["bc_rows"], (where, got["bc_rows"], want["bc_rows"])
        self.assert_intact(where)
        return got

    def assert_intact(self, where):
        for k in INPUTS:
            assert same_but_nan(self.g.host(k), self.x[k]), (where, k)  # inputs are only read
        assert self.g.guards_intact() and guards_intact({"bc_rows": self.rows}) is None, where


# ------------------------------------------------------------------------------------------------ 1. the launch against the restatement
@pytest.mark.parametrize("count", GPU_COUNTS)
def test_cloned_terms_are_the_restatement_bitwise(env, count):
    c = Case(env, count)
    c.plain()
    torch.cuda.synchronize(env.device)
    plain = {k: c.g.host("plain_" + k) for k in ("d_action", "critic_loss", "actor_loss")}
    for scale_by_q, q_filter in FLAGS:
        where = (count, scale_by_q, q_filter)
        want = bc.restate(c.x, count, scale_by_q, q_filter)
        c.call(scale_by_q, q_filter)
        got = c.assert_is(want, where)
        assert np.isfinite(got["d_action"]).all() and np.isfinite([got[k][0] for k in FLOAT_OUTPUTS[1:]]).all(), where
        # the two losses are bitwise urgym_sac_policy_terms', and so is every row that is not cloned
        assert same(got["critic_loss"], plain["critic_loss"]) and same(got["actor_loss"], plain["actor_loss"]), where
        cloned = want["cloned"]
        assert same(got["d_action"][~cloned], plain["d_action"][~cloned]), where
        assert not cloned.any() or (got["d_action"][cloned] != plain["d_action"][cloned]).any(), where  # the cloning term is there
        assert cloned.all() if not q_filter else (count < 2 or (cloned.any() and not cloned.all())), where
        # with weight = 0 the whole d_action_out compares equal to that call's: g + (+-0) == g.  A -0.0 of g may become +0.0, so the
        # comparison is by value, not by bits.
        c.call(scale_by_q, q_filter, weight=0.0)
        zero = c.outputs()
        assert np.array_equal(zero["d_action"], plain["d_action"]) and zero["bc_weight"][0] == 0 and same(zero["bc_loss"], got["bc_loss"]), where
        assert zero["bc_rows"][0] == want["bc_rows"], where


def test_in_place_and_two_runs_give_the_same_bits(env):
    count = 1025
    runs = []
    for _ in range(2):
        c = Case(env, count)
        c.call(True, True, d_action="dqmin_da")  # d_action_out is dqmin_da
        torch.cuda.synchronize(env.device)
        want = bc.restate(c.x, count, True, True)
        assert same(c.g.host("dqmin_da"), want["d_action"]) and np.isnan(c.g.host("d_action")).all()
        assert same(c.g.host("bc_loss"), np.full(1, want["bc_loss"])) and c.rows[1].item() == want["bc_rows"]
        assert c.g.guards_intact() and guards_intact({"bc_rows": c.rows}) is None
        runs.append([c.g.host(k) for k in ("dqmin_da",) + FLOAT_OUTPUTS[1:]] + [c.rows[1].cpu().numpy()])
    assert all(same(a, b) if a.dtype == np.float32 else np.array_equal(a, b) for a, b in zip(*runs))
    c = Case(env, 4097)  # the same launch twice from one state
    c.call(True, True)
    first = c.outputs()
    c.call(True, True)
    second = c.outputs()
    assert all(same(first[k], second[k]) for k in FLOAT_OUTPUTS) and first["bc_rows"][0] == second["bc_rows"][0]


def test_non_finite_values_stay_where_the_header_says(env):
    count = 1025
    for scale_by_q, q_filter in FLAGS:
        where = (scale_by_q, q_filter)
        base = bc.restate(bc.inputs(count), count, scale_by_q, q_filter)
        # a NaN action of a cloned row reaches that row of d_action_out and bc_loss_out
        c = Case(env, count, "nan_action")
        c.call(scale_by_q, q_filter)
        got = c.assert_is(bc.restate(c.x, count, scale_by_q, q_filter), where, eq=same_but_nan)
        rest = np.ones((count, 6), dtype=bool)
        rest[0, 3] = False
        assert np.isnan(got["d_action"][0, 3]) and np.isnan(got["bc_loss"][0]) and same(got["d_action"][rest], base["d_action"][rest]), where
        assert same(got["bc_weight"], np.full(1, base["bc_weight"])) and got["bc_rows"][0] == base["bc_rows"], where
        # a NaN q_min reaches w only with scale_by_q, and through w every cloned row; a row that is not cloned is never touched
        c = Case(env, count, "nan_q_min")
        c.plain()
        c.call(scale_by_q, q_filter)
        want = bc.restate(c.x, count, scale_by_q, q_filter)
        got = c.assert_is(want, where, eq=same_but_nan)
        cloned = want["cloned"]
        assert cloned[count - 1] == (not q_filter) and np.isnan(got["bc_weight"][0]) == scale_by_q, where
        assert same(got["d_action"][~cloned], c.g.host("plain_d_action")[~cloned]), where
        assert np.isnan(got["d_action"][cloned]).all() if scale_by_q else np.isfinite(got["d_action"]).all(), where
        assert np.isfinite(got["bc_loss"][0]), where
    # +-0 differences: the restatement's bits, signs of zero included
    c = Case(env, count, "zero_differences")
    c.call(False, False)
    c.assert_is(bc.restate(c.x, count, False, False), "zero differences")


def test_stream_order_without_a_synchronisation(env):
    """Two launches on one set of inputs with q_min rewritten between them by a device copy, nothing synchronised in between: the
    first reads the first q_min, the second the second, and each leaves its own outputs."""
    count = 1025
    c = Case(env, count)
    other = Case(env, count)  # its outputs receive the second launch
    first, second = c.x["q_min"].copy(), -c.x["q_min"][::-1].copy()
    dev = [torch.from_numpy(a).to(env.device) for a in (first, second)]
    t, o = c.g.t, other.g.t
    torch.cuda.synchronize(env.device)
    t["q_min"].copy_(dev[0])
    c.call(True, True)
    t["q_min"].copy_(dev[1])  # in host time the first launch may not have run yet
    env.policy_terms_cloned(t["ent_coef"], count, dqmin_da=t["dqmin_da"], scale=-1.0 / count, d_action_out=o["d_action"], q=t["q"], y=t["y"],
                            critic_loss_out=o["critic_loss"], log_prob=t["log_prob"], q_min=t["q_min"], actor_loss_out=o["actor_loss"], action_pi=t["action_pi"],
                            action_data=t["action_data"], weight=WEIGHT, bc_scale=1.0 / count, scale_by_q=True, q_filter=True, bc_loss_out=o["bc_loss"],
                            bc_weight_out=o["bc_weight"], bc_rows_out=other.rows[1])
    torch.cuda.synchronize(env.device)
    wants = [bc.restate(dict(c.x, q_min=q), count, True, True) for q in (first, second)]
    assert wants[0]["bc_rows"] != wants[1]["bc_rows"] and not same(wants[0]["d_action"], wants[1]["d_action"])
    for case, want in zip((c, other), wants):
        got = case.outputs()
        assert all(same(got[k], np.asarray(want[k]).reshape(got[k].shape)) for k in FLOAT_OUTPUTS) and got["bc_rows"][0] == want["bc_rows"]


# ------------------------------------------------------------------------------------------------ 2. refusals
def test_every_refusal_leaves_state_and_outputs_unchanged(env):
    lib, count = env.lib, 65
    c = Case(env, count)
    t = c.g.t
    fptr = lambda x: C.cast(x.data_ptr(), C.POINTER(C.c_float))  # noqa: E731
    good_a = dict(count=count, reserved0=0, scale=-1.0 / count, ent_coef=fptr(t["ent_coef"]), dqmin_da=fptr(t["dqmin_da"]), d_action_out=fptr(t["d_action"]),
                  q=fptr(t["q"]), y=fptr(t["y"]), critic_loss_out=fptr(t["critic_loss"]), log_prob=fptr(t["log_prob"]), q_min=fptr(t["q_min"]),
                  actor_loss_out=fptr(t["actor_loss"]))
    good_b = dict(action_pi=fptr(t["action_pi"]), action_data=fptr(t["action_data"]), weight=WEIGHT, bc_scale=1.0 / count, scale_by_q=1, q_filter=1,
                  bc_loss_out=fptr(t["bc_loss"]), bc_weight_out=fptr(t["bc_weight"]), bc_rows_out=C.cast(c.rows[1].data_ptr(), C.POINTER(C.c_int32)), reserved0=0)
    inf = float("inf")
    cases = [("null clone args", {}, None, b"null clone args")]
    # everything urgym_sac_policy_terms refuses
    cases += [(f"args: {k}={v!r}", {k: v}, {}, expect) for k, v, expect in (
        ("count", 0, b"count"), ("count", _abi.SAC_TERMS_MAX_COUNT + 1, b"count"), ("reserved0", 1, b"reserved0"), ("ent_coef", None, b"ent_coef"),
        ("scale", inf, b"scale"), ("scale", float("nan"), b"scale"), ("dqmin_da", None, b"half given"), ("y", None, b"half given"), ("q_min", None, b"half given"))]
    # any of its three groups absent
    for group in (("dqmin_da", "d_action_out"), ("q", "y", "critic_loss_out"), ("log_prob", "q_min", "actor_loss_out")):
        cases.append((f"no {group[-1]} group", {k: None for k in group}, {}, b"all three groups"))
    # the clone args' own
    cases += [(f"clone: {k}=NULL", {}, {k: None}, b"is null") for k in ("action_pi", "action_data", "bc_loss_out", "bc_weight_out", "bc_rows_out")]
    cases += [(f"clone: {k}={v!r}", {}, {k: v}, expect) for k, v, expect in (
        ("weight", -1.0, b"weight"), ("weight", -1e-30, b"weight"), ("weight", inf, b"weight"), ("weight", float("nan"), b"weight"), ("bc_scale", inf, b"bc_scale"),
        ("bc_scale", float("nan"), b"bc_scale"), ("scale_by_q", 2, b"0 or 1"), ("scale_by_q", -1, b"0 or 1"), ("q_filter", 2, b"0 or 1"), ("q_filter", -1, b"0 or 1"),
        ("reserved0", 1, b"reserved0"))]
    cases += [("d_action_out is action_pi", dict(d_action_out=fptr(t["action_pi"])), {}, b"d_action_out is action_pi or action_data"),
              ("d_action_out is action_data", dict(d_action_out=fptr(t["action_data"])), {}, b"d_action_out is action_pi or action_data")]
    for what, a_over, b_over, expect in cases:
        a = _abi.SacPolicyArgs(**dict(good_a, **a_over))
        b = None if b_over is None else C.byref(_abi.SacCloneArgs(**dict(good_b, **b_over)))
        rc = lib.urgym_sac_policy_terms_cloned(env._h, C.byref(a), b, env._stream())
        assert rc == _abi.ERR_ARG and expect in lib.urgym_last_error(env._h), (what, rc, lib.urgym_last_error(env._h))
    assert lib.urgym_sac_policy_terms_cloned(env._h, None, C.byref(_abi.SacCloneArgs(**good_b)), env._stream()) == _abi.ERR_ARG
    # the binding refuses before the library is asked
    for over in (dict(weight=-1.0), dict(weight=NAN), dict(weight=True), dict(bc_scale=inf), dict(scale_by_q=1), dict(q_filter=None),
                 dict(action_pi=t["action_pi"][:-1]), dict(action_data=t["action_data"].double()), dict(bc_rows_out=t["bc_loss"]), dict(d_action_out=t["action_pi"])):
        kw = dict(c.args(), action_pi=t["action_pi"], action_data=t["action_data"], weight=WEIGHT, bc_scale=1.0 / count, scale_by_q=True, q_filter=True,
                  bc_loss_out=t["bc_loss"], bc_weight_out=t["bc_weight"], bc_rows_out=c.rows[1])
        with pytest.raises(ValueError):
            env.policy_terms_cloned(t["ent_coef"], count, **dict(kw, **over))
    with pytest.raises(ValueError, match="count"):
        env.policy_terms_cloned(t["ent_coef"], 0, **dict(kw))
    got = c.outputs()
    assert all(np.isnan(got[k]).all() for k in FLOAT_OUTPUTS) and got["bc_rows"][0] == ROWS_BEFORE  # nothing was launched, nothing written
    c.assert_intact("refusals")
    c.call(True, True)  # and the good structs are good
    c.assert_is(bc.restate(c.x, count, True, True), "after the refusals")


# ------------------------------------------------------------------------------------------------ 3. the learner
N, H, M, CAP, STARTS, SEED, UPDATE_SEED, FIRST_DRAW = 8, 32, 65, 4, 16, 5, 11, 7
BC = dict(bc_weight=0.5, bc_scale_by_q=True, bc_q_filter=True)
BC_KEYS = ("bc_loss", "bc_weight", "bc_rows")
LOSS_KEYS = ("critic_loss", "actor_loss", "ent_coef_loss")
SIGMA = 0.3


class BcSide(Side):
    """test_sac_train's Side at 8 envs, batch 65, episodes of at most 3 steps, the warm-up over after two steps, with the option under
    test; a prioritized ring or an MPPI planner guided by the learner's own initial parameters on request.  The same bits whichever
    side it is; `seeds` moves every seed (the rebuilt run of the checkpoint test)."""

    def __init__(self, env_id="UR5OriReach-v1", planner=False, prioritized=False, seeds=0, **over):
        self.env = make_vec(env_id, num_envs=N, seed=SEED + seeds, auto_reset=True, max_episode_steps=3)
        self.env.reset(seed=SEED + seeds)
        self.learner = SACLearner(self.env, seed=SEED + seeds, hidden_width=H, batch_size=M, learning_starts=STARTS, **dict(ALL, prioritized=prioritized, **over))
        self.replay = DevicePrioritizedReplay(self.env, 40, alpha=0.6, eps=1e-6) if prioritized else DeviceReplay(self.env, CAP)
        self.mppi = None
        if planner:
            self.mppi = DeviceMPPI(self.env, samples=5, horizon=2, sigma=0.3, lam=20.0, gamma=0.95, seed=8, actor=host_arrays(self.learner.actor.tensors()),
                                   critic=host_arrays(self.learner.critic.tensors()), terminal_value=True, policy_samples=2, policy_sigma=0.2)

    def loop(self, iterations, K, G, first_draw):
        """The loop of tools/train_sac.py: collect (with the planner where there is one), the updates unless the warm-up still holds, the
        planner's sync.  Returns per update the three losses and, with the option, the three cloning values, copied as they were made."""
        lr, out, draw = self.learner, [], first_draw
        for _ in range(iterations):
            if K:
                lr.collect(self.replay, K, **({} if self.mppi is None else dict(planner=self.mppi, explore_sigma=SIGMA)))
            if lr.env_steps * N < lr.hp["learning_starts"]:
                continue
            for _ in range(G):
                got = lr.update(self.replay, UPDATE_SEED, draw)
                out.append(dict({k: v.clone() for k, v in got.items()}, **{k: lr.last_update[k][0].clone() for k in BC_KEYS if k in lr.last_update}))
                draw += 1
            if self.mppi is not None and G:
                lr.sync_planner(self.mppi)
        return out

    def train(self, iterations, K, G, first_draw):
        extra = {} if self.mppi is None else dict(planner=self.mppi, explore_sigma=SIGMA)
        return self.learner.train(self.replay, iterations, K, G, seed=UPDATE_SEED, first_draw=first_draw, **extra)

    def state(self):
        out = super().state()
        if hasattr(self.replay, "leaf"):
            out.update(leaf=self.replay.leaf, sums=self.replay.sums, max_leaf=self.replay.max_leaf)
        if self.learner.normalizer is not None:
            out.update({f"norm.{k}": v for k, v in self.learner.normalizer.state.items()})
        if self.mppi is not None:
            out.update({"planner.packed.actor": self.mppi.actor.packed(), "planner.packed.critic": self.mppi.critic.packed()})
            out.update({f"planner.buf.{k}": v for k, v in self.mppi.buf.items()})
        return out

    def close(self):
        if self.mppi is not None:
            self.mppi.close()
        super().close()


def assert_same(a, b, what, skip=()):
    sa, sb = a.state(), b.state()
    assert sa.keys() == sb.keys(), what
    assert sum(k.startswith("param:") for k in sa) == 8 + 12 and sum(k.startswith("moment:") for k in sa) == 2 * (8 + 12)
    for k in sa:
        if not k.startswith(skip):
            assert np.array_equal(bits(sa[k]), bits(sb[k])), (what, k)
    assert a.counters() == b.counters(), (what, a.counters(), b.counters())
    la, lb = a.learner.last_update, b.learner.last_update
    assert sorted(la) == sorted(lb) and set(BC_KEYS) | {"action_pi", "action_data"} <= set(la), (what, sorted(la), sorted(lb))
    for k in la:
        assert la[k].shape == lb[k].shape and np.array_equal(bits(la[k]), bits(lb[k])), (what, "last_update", k)


def assert_same_values(want, got, what):
    assert set(LOSS_KEYS + BC_KEYS) <= set(got) and all(got[k].shape == (len(want),) for k in LOSS_KEYS + BC_KEYS), what
    assert got["bc_rows"].dtype == torch.int32 and got["bc_loss"].dtype == got["bc_weight"].dtype == torch.float32
    for u, w in enumerate(want):
        for k in LOSS_KEYS + BC_KEYS:
            assert np.array_equal(bits(got[k][u]), bits(w[k])), (what, u, k, got[k][u].item(), w[k].item())


def test_update_is_the_sequence_of_single_calls_with_the_restated_terms():
    s = BcSide(**BC)
    lr = s.learner
    lr.collect(s.replay, CAP)
    shares = []
    for draw in range(3):
        losses = lr.update(s.replay, UPDATE_SEED, draw)
        torch.cuda.synchronize(s.env.device)
        last, es = lr.last_update, lr.entropy_state
        host = {k: v.cpu().numpy() for k, v in last.items()}
        assert host["action_data"].shape == host["action_pi"].shape == (M, 6) and last["bc_rows"].dtype == torch.int32
        want = policy_terms_cloned(es["ent_coef"].cpu().numpy()[0], dqmin_da=host["dqmin_da"], scale=-1.0 / M, q=host["q"], y=host["y"], log_prob=host["log_prob"],
                                   q_min=host["q_min"], action_pi=host["action_pi"], action_data=host["action_data"], weight=BC["bc_weight"], bc_scale=1.0 / M,
                                   scale_by_q=True, q_filter=True)
        assert same(lr.actor_d_action.cpu().numpy(), want["d_action"]), draw
        assert same(losses["critic_loss"].cpu().numpy(), want["critic_loss"]) and same(losses["actor_loss"].cpu().numpy(), want["actor_loss"]), draw
        assert same(host["bc_loss"], np.full(1, want["bc_loss"])) and same(host["bc_weight"], np.full(1, want["bc_weight"])) and host["bc_rows"][0] == want["bc_rows"], draw
        # the rows the term was formed on are the ring's actions of the gathered rows: every one of them is an action the ring holds
        ring = s.replay.ring["action"].cpu().numpy().reshape(-1, 6)
        assert all((ring == row).all(1).any() for row in host["action_data"]), draw
        plain = policy_terms(es["ent_coef"].cpu().numpy()[0], dqmin_da=host["dqmin_da"], scale=-1.0 / M)["d_action"]
        assert same(want["d_action"][~want["cloned"]], plain[~want["cloned"]])
        shares.append(int(want["bc_rows"]))
        print(f"update {draw}: bc_loss {host['bc_loss'][0]!r} bc_weight {host['bc_weight'][0]!r} cloned {want['bc_rows']} of {M}")
    assert any(0 < n for n in shares) and any(n < M for n in shares), shares  # the filter clones some rows and leaves some
    s.close()


OPTIONS = {"plain": {}, "planner": dict(planner=True), "n_steps": dict(n_steps=3), "max_grad_norm": dict(max_grad_norm=1e-2), "hindsight": dict(hindsight=True),
           "prioritized": dict(prioritized=True, per_beta=0.4, per_beta_steps=7), "normalize": dict(normalize=True)}


@pytest.mark.parametrize("option", list(OPTIONS))
def test_train_equals_the_python_loop_bit_for_bit(option):
    """ONE native call (urgym_sac_train_cloned with the option's struct) against collect / update (/ sync_planner) on a twin: every
    ring tensor, bound buffer, parameter, moment, gradient, packed buffer, the planner's buffers, the priorities, the statistics, the
    losses, the three new arrays and last_update, bit for bit.  The planner's case is one trip that updates and syncs after the idle one."""
    env_id = "UR5DynReach-v1" if option in ("hindsight", "prioritized") else "UR5OriReach-v1"
    iterations = 3 if option == "planner" else 4
    a, b = BcSide(env_id, **BC, **OPTIONS[option]), BcSide(env_id, **BC, **OPTIONS[option])
    want = a.loop(iterations, 1, 2, FIRST_DRAW)
    got = b.train(iterations, 1, 2, FIRST_DRAW)
    torch.cuda.synchronize(a.env.device)
    assert len(want) == 2 * (iterations - 1) and all(k in want[0] for k in BC_KEYS), option
    assert_same_values(want, got, option)
    assert_same(a, b, option)
    rows = got["bc_rows"].cpu().numpy()
    assert ((0 <= rows) & (rows <= M)).all() and np.isfinite(got["bc_loss"].cpu().numpy()).all() and (got["bc_weight"].cpu().numpy() > 0).all(), option
    if option == "max_grad_norm":
        assert got["critic_grad_norm"].shape == (len(want),)
    if option == "planner":  # the planner follows the learner after the sync
        assert np.array_equal(b.mppi.actor.packed(), b.learner.device_actor.packed()) and np.array_equal(b.mppi.critic.packed(), b.learner.online.packed())
    a.close(), b.close()


def test_split_calls_and_the_learner_without_the_option():
    a, b, c = BcSide(**BC), BcSide(**BC), BcSide()
    whole = a.train(4, 1, 2, FIRST_DRAW)
    first = b.train(1, 1, 2, FIRST_DRAW)  # the idle iteration: no update, three empty arrays
    second = b.train(3, 1, 2, FIRST_DRAW)
    other = c.train(4, 1, 2, FIRST_DRAW)
    torch.cuda.synchronize(a.env.device)
    assert all(first[k].shape == (0,) for k in LOSS_KEYS + BC_KEYS) and second["bc_rows"].shape == (6,)
    for k in LOSS_KEYS + BC_KEYS:
        assert np.array_equal(bits(whole[k]), bits(torch.cat([first[k], second[k]]))), k
    d = BcSide(**BC)
    d.train(2, 1, 2, FIRST_DRAW)
    d.train(2, 1, 2, FIRST_DRAW + 2)
    torch.cuda.synchronize(a.env.device)
    assert_same(a, d, "2 + 2 iterations")
    # cloning is another computation than the learner without it, whose result and last_update hold no new key
    assert sorted(other) == sorted(LOSS_KEYS) and not set(BC_KEYS) & set(c.learner.last_update) and c.learner.bc_state is None
    assert not np.array_equal(bits(other["actor_loss"]), bits(whole["actor_loss"]))
    for s in (a, b, c, d):
        s.close()


class Calls:
    """Records every urgym_* symbol a block calls through env.lib, and passes every call on."""

    def __init__(self, env):
        self.env, self.lib, self.names = env, env.lib, []

    def __getattr__(self, name):
        if name.startswith("urgym_"):
            self.names.append(name)
        return getattr(self.lib, name)

    def __enter__(self):
        self.env.lib = self
        return self

    def __exit__(self, *exc):
        self.env.lib = self.lib


NEW_SYMBOLS = ("urgym_sac_policy_terms_cloned", "urgym_sac_train_cloned")


def test_update_launches_what_it_launched_and_no_torch_operation():
    from torch.utils._python_dispatch import TorchDispatchMode

    class Recorder(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.append(str(func))
            return func(*args, **(kwargs or {}))

    seen = {}
    for label, over in (("cloned", BC), ("plain", {})):
        s = BcSide(**over)
        with Calls(s.env) as calls:
            s.learner.collect(s.replay, CAP)
            s.learner.update(s.replay, UPDATE_SEED, 0)  # whatever is made lazily is made here
            del calls.names[:]
            with Recorder() as rec:
                s.learner.update(s.replay, UPDATE_SEED, 1)
            update = list(calls.names)
            s.train(1, 0, 2, 2)
            everything = list(calls.names)
        torch.cuda.synchronize(s.env.device)
        print(f"{label} update: {len(update)} library calls {update}; {len(rec.names)} torch operations: {sorted(set(rec.names))}")
        assert rec.names and "aten.empty.memory_format" in rec.names and set(rec.names) <= ALLOCATIONS_AND_VIEWS, sorted(set(rec.names) - ALLOCATIONS_AND_VIEWS)
        seen[label] = (update, everything)
        s.close()
    # the same calls in the same order, but for the one that is replaced: the launch count is unchanged
    assert seen["cloned"][0] == ["urgym_sac_policy_terms_cloned" if n == "urgym_sac_policy_terms" else n for n in seen["plain"][0]]
    assert seen["plain"][0].count("urgym_sac_policy_terms") == 1 and seen["cloned"][0].count("urgym_sac_policy_terms_cloned") == 1
    assert seen["cloned"][1][-1] == "urgym_sac_train_cloned" and seen["plain"][1][-1] == "urgym_sac_train"
    # a learner without the option calls neither new symbol
    assert not set(NEW_SYMBOLS) & set(seen["plain"][1]) and "urgym_sac_policy_terms" not in seen["cloned"][1]


def test_save_and_load_continue_bit_for_bit(tmp_path):
    a, b = BcSide(**BC), BcSide(**BC)
    a.train(6, 1, 2, FIRST_DRAW)
    b.train(3, 1, 2, FIRST_DRAW)
    path = tmp_path / "run.npz"
    b.learner.save(path, replay=b.replay, extra=dict(update_draw=FIRST_DRAW + b.learner.adam_state["step"]))
    assert {k: b.learner.state_dict()["hp"][k] for k in BC} == BC
    b.close()
    one = BcSide(seeds=100)  # a learner without the option refuses the file, and nothing of it is written
    with pytest.raises(ValueError, match="bc_weight is 0.5 in the checkpoint, None here"):
        one.learner.load(path, replay=one.replay)
    plain = tmp_path / "plain.npz"  # ... and its own checkpoint holds no new key
    one.learner.collect(one.replay, 2)
    one.learner.save(plain, replay=one.replay)
    assert not set(BC) & set(one.learner.state_dict()["hp"]) and not any("bc_" in k for k in np.load(plain, allow_pickle=False).files)
    one.close()
    other = BcSide(seeds=100, **dict(BC, bc_q_filter=False))
    with pytest.raises(ValueError, match="bc_q_filter is True in the checkpoint, False here"):
        other.learner.load(path, replay=other.replay)
    other.close()
    c = BcSide(seeds=100, **BC)  # rebuilt from other seeds
    for t in c.replay.ring.values():
        t.fill_(1)
    extra = c.learner.load(path, replay=c.replay)
    c.train(3, 1, 2, extra["update_draw"])
    torch.cuda.synchronize(a.env.device)
    assert a.learner.seed == c.learner.seed
    assert_same(a, c, "3 + 3", skip=("grad:",))  # the ring has wrapped: every slot holds a collected step
    a.close(), c.close()
