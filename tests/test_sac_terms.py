"""GPU tests (-m gpu) of SAC's entropy coefficient on the device: urgym_sac_entropy_step / urgym_sac_policy_terms.

Every output of either call equals evaluation.entropy_step / evaluation.policy_terms bit for bit, the restatement being fed the alpha the
launch itself wrote to ent_coef_out (the device's expf is checked on its own, against float64 exp).  Tensors are handed over as views
one float into larger allocations, with guard words around each.  One small environment (UR5OriReach-v1, 64 envs): neither call reads
anything of it but the handle.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from sac_terms_cases import COUNTS, GAMMA, HYPER, POLICY_COUNTS, TARGET_ENTROPY, inputs, p_bound, same, words
from ur_gym_amd import _abi, make_vec
from ur_gym_amd._native import NativeError
from ur_gym_amd.evaluation import CRITIC_ARRAYS, DeviceCritic, DeviceReplay, adam_coefficients, adam_step, entropy_step, policy_terms

pytestmark = pytest.mark.gpu

GUARD, GUARD_WORD = 4, 0x7FC05AC0  # floats of guard on either side of a tensor (after the one-float offset), and what they hold
STATE = ("l", "m", "v")
ENTROPY_INPUTS = ("log_prob", "target", "next_log_prob")
NAN = np.float32("nan")


@pytest.fixture(scope="module")
def env():
    e = make_vec("UR5OriReach-v1", num_envs=64, seed=3, auto_reset=True)
    e.reset(seed=3)
    yield e
    e.close()


class Guarded:
    """Device tensors of a dict of host arrays (float32 or uint8): each a contiguous view that starts GUARD + 1 words into its own
    allocation (4 bytes past a 16-byte boundary) and ends at least GUARD words before its end; the rest holds GUARD_WORD."""

    def __init__(self, host, device):
        self.flat, self.t = {}, {}
        for k, a in host.items():
            self.add(k, a, device)

    def add(self, k, a, device):
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.float32, np.uint8), a.dtype
        n_words = (a.nbytes + 3) // 4
        flat = torch.full((n_words + 2 * GUARD + 1,), GUARD_WORD, dtype=torch.int32, device=device)
        typed = flat.view(torch.float32 if a.dtype == np.float32 else torch.uint8)
        first = (GUARD + 1) * (4 // a.itemsize)
        view = typed[first:first + a.size]
        view.copy_(torch.from_numpy(a.reshape(-1)))
        self.flat[k], self.t[k] = flat, view.view(a.shape)
        assert self.t[k].is_contiguous() and self.t[k].data_ptr() % 16 == 4

    def set(self, k, a):
        self.t[k].copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(self.t[k].shape)))

    def host(self, k):
        return self.t[k].cpu().numpy()

    def guards_intact(self):
        for k, flat in self.flat.items():
            b = flat.view(torch.uint8).cpu().numpy()
            want = np.full(flat.numel(), GUARD_WORD, dtype=np.int32).view(np.uint8)
            lo, n = (GUARD + 1) * 4, self.t[k].numel() * self.t[k].element_size()
            if not (np.array_equal(b[:lo], want[:lo]) and np.array_equal(b[lo + n:], want[lo + n:])):
                return False
        return True


def same_but_nan(a, b):
    """Bitwise equal, except that where both hold a NaN the words are not compared (the sign and payload of a propagated NaN are not
    part of the contract)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(words(a)[both.reshape(-1) == 0], words(b)[both.reshape(-1) == 0])


class EntropyCase:
    """Inputs, state and NaN-filled outputs of urgym_sac_entropy_step at one count on the device, and the host mirror of the state."""

    def __init__(self, env, count, seed=16):
        self.env, self.count = env, count
        self.x = x = inputs(count, seed)
        self.state = {k: np.full(1, x[k], np.float32) for k in STATE}
        nan1, nanc = np.full(1, NAN), np.full(count, NAN)
        host = {k: x[k] for k in ENTROPY_INPUTS}
        host.update(terminated=x["terminated"], l=self.state["l"], m=self.state["m"], v=self.state["v"], ent_coef=nan1, loss=nan1, y=nanc, d_log_prob=nanc)
        self.g = Guarded(host, env.device)
        self.step = 0

    def call(self, y="out", terminated=True, target=True, upstream=True, loss=True, scale=None, same_y=same):
        """One launch and the restatement of it on the alpha it wrote; asserts every output bitwise and returns the restatement."""
        env, g, x, count = self.env, self.g, self.x, self.count
        self.step += 1
        scale = 1.0 / count if scale is None else scale
        kw, want_kw = {}, {}
        target_before = g.host("target")
        if target:
            kw.update(target=g.t["target"], next_log_prob=g.t["next_log_prob"], gamma=GAMMA, y_out=g.t["y"] if y == "out" else g.t["target"])
            want_kw.update(target=target_before, next_log_prob=g.host("next_log_prob"), gamma=GAMMA)
            if terminated:
                kw["terminated"], want_kw["terminated"] = g.t["terminated"], x["terminated"]
        if upstream:
            kw.update(d_log_prob_out=g.t["d_log_prob"], scale=scale)
            want_kw["scale"] = scale
        before = {k: g.host(k) for k in ("y", "d_log_prob", "loss")}
        env.entropy_step((g.t["l"], g.t["m"], g.t["v"]), g.t["log_prob"], TARGET_ENTROPY, step=self.step, ent_coef_out=g.t["ent_coef"],
                         loss_out=g.t["loss"] if loss else None, **kw, **HYPER)
        torch.cuda.synchronize(env.device)
        alpha = g.host("ent_coef")[0]
        want = entropy_step(alpha, g.host("log_prob"), TARGET_ENTROPY, self.state["l"], self.state["m"], self.state["v"],
                            adam_coefficients(env, step=self.step, **HYPER), **want_kw)
        for k in STATE:
            assert same(g.host(k), want[k]), (count, self.step, k, g.host(k), want[k])
            self.state[k] = want[k]
        assert same(g.host("loss"), np.full(1, want["loss"]) if loss else before["loss"]), (count, self.step, g.host("loss"), want["loss"])
        if target:
            assert same_y(g.host("y" if y == "out" else "target"), want["y"]), (count, self.step, "y")
            assert same_y(g.host("y"), want["y"] if y == "out" else before["y"]) and (y != "out" or same(g.host("target"), target_before))
        else:
            assert same(g.host("y"), before["y"]) and same(g.host("target"), target_before)
        assert same(g.host("d_log_prob"), want["d_log_prob"] if upstream else before["d_log_prob"]), (count, self.step, "d_log_prob")
        assert g.guards_intact(), (count, self.step)
        return want


# ------------------------------------------------------------------------------------------------ entropy_step, bitwise
@pytest.mark.parametrize("count", COUNTS)
def test_entropy_step_is_the_restatement_bitwise(env, count):
    c = EntropyCase(env, count)
    for _ in range(3):  # steps 1, 2, 3 on the carried state, every group given, y out of place, a quarter of the rows terminal
        want = c.call()
        assert np.isfinite(want["y"]).all() and np.isfinite([want[k][0] for k in STATE]).all() and np.isfinite(want["loss"])
    assert c.x["terminated"].sum() > 0 or count < 8
    c.call(terminated=False)                 # terminated NULL: no row is terminal
    c.call(upstream=False)                   # each optional group absent ...
    c.call(target=False)
    c.call(target=False, upstream=False, loss=False)  # ... both, and no loss either: the bare step
    c.call(y="in place")                     # y_out == target_in; last, because it overwrites the input
    c.call(y="in place", terminated=False)


def test_terminal_rows_drop_the_entropy_term_and_the_step_uses_the_old_coefficient(env):
    c = EntropyCase(env, 1025)
    l_before = c.state["l"].copy()
    want = c.call()
    term = c.x["terminated"].astype(bool)
    assert term.any() and (~term).any()
    assert same(want["y"][term], c.x["target"][term])  # d = gamma * 0 = 0, e = 0 * next_log_prob = 0 (the inputs are finite)
    assert not same(want["y"][~term], c.x["target"][~term])
    alpha = c.g.host("ent_coef")[0]
    assert abs(float(alpha) - np.exp(float(l_before[0]))) <= 2 * np.spacing(alpha) and not same(c.state["l"], l_before)  # alpha is exp of the OLD l


def test_ent_coef_out_against_float64_exp(env):
    grid = np.concatenate([np.arange(-2000, 201, dtype=np.float64) / 100.0, np.random.default_rng(2).uniform(-20.0, 2.0, 800)]).astype(np.float32)
    assert grid.min() == -20 and grid.max() == 2 and np.any(grid == 0)
    K = grid.size
    l = torch.from_numpy(grid).to(env.device)
    alpha = torch.full((K,), float("nan"), device=env.device)
    m, v = torch.zeros((K,), device=env.device), torch.zeros((K,), device=env.device)
    log_prob = torch.zeros((1,), device=env.device)
    for k in range(K):  # one launch per grid point: each steps an l, m, v of its own
        env.entropy_step((l[k:k + 1], m[k:k + 1], v[k:k + 1]), log_prob, TARGET_ENTROPY, step=1, ent_coef_out=alpha[k:k + 1], **HYPER)
    torch.cuda.synchronize(env.device)
    got = alpha.cpu().numpy()
    want = np.exp(grid.astype(np.float64))
    ulps = np.abs(got.astype(np.float64) - want) / np.spacing(want.astype(np.float32)).astype(np.float64)
    worst = int(np.argmax(ulps))
    print(f"ent_coef_out against float64 exp on {K} values of l in [-20, 2]: worst {ulps[worst]:.3f} ulp at l = {grid[worst]!r}")
    assert np.all(ulps <= 2.0), (grid[worst], got[worst], want[worst])
    assert same(got[grid == 0], np.ones(int((grid == 0).sum()), np.float32))  # l = 0 gives exactly 1.0f
    assert np.all(l.cpu().numpy() != grid)  # every l was stepped (g = 6: target_entropy = -6 on log_prob = 0)


# ------------------------------------------------------------------------------------------------ policy_terms, bitwise
POLICY_GROUPS = {"upstream": ("d_action",), "critic": ("critic_loss",), "actor": ("actor_loss",)}


@pytest.mark.parametrize("count", POLICY_COUNTS)
def test_policy_terms_is_the_restatement_bitwise(env, count):
    x = inputs(count, seed=17)
    alpha = np.float32(0.37)
    scale = -1.0 / count
    for groups in (("upstream",), ("critic",), ("actor",), ("upstream", "critic", "actor")):
        host = {k: x[k] for k in ("dqmin_da", "q", "y", "log_prob", "q_min")}
        host.update(ent_coef=np.full(1, alpha), d_action=np.full((count, 6), NAN), critic_loss=np.full(1, NAN), actor_loss=np.full(1, NAN))
        g = Guarded(host, env.device)
        kw, want_kw = {}, {}
        if "upstream" in groups:
            kw.update(dqmin_da=g.t["dqmin_da"], scale=scale, d_action_out=g.t["d_action"])
            want_kw.update(dqmin_da=x["dqmin_da"], scale=scale)
        if "critic" in groups:
            kw.update(q=g.t["q"], y=g.t["y"], critic_loss_out=g.t["critic_loss"])
            want_kw.update(q=x["q"], y=x["y"])
        if "actor" in groups:
            kw.update(log_prob=g.t["log_prob"], q_min=g.t["q_min"], actor_loss_out=g.t["actor_loss"])
            want_kw.update(log_prob=x["log_prob"], q_min=x["q_min"])
        env.policy_terms(g.t["ent_coef"], count, **kw)
        torch.cuda.synchronize(env.device)
        want = policy_terms(alpha, **want_kw)
        for name, outs in POLICY_GROUPS.items():
            for k in outs:
                got = g.host(k)
                if name in groups:
                    assert same(got, np.asarray(want[k]).reshape(got.shape)), (count, groups, k, got, want[k])
                    assert np.isfinite(got).all()
                else:
                    assert np.isnan(got).all(), (count, groups, k)  # a group that is absent writes nothing
        for k in ("dqmin_da", "q", "y", "log_prob", "q_min", "ent_coef"):
            assert same(g.host(k), host[k]), k  # inputs are only read
        assert g.guards_intact(), (count, groups)


def test_policy_terms_upstream_in_place(env):
    count = 65
    x = inputs(count, seed=18)
    g = Guarded(dict(dqmin_da=x["dqmin_da"], ent_coef=np.ones(1, np.float32)), env.device)
    env.policy_terms(g.t["ent_coef"], count, dqmin_da=g.t["dqmin_da"], scale=-0.3, d_action_out=g.t["dqmin_da"])
    assert same(g.host("dqmin_da"), policy_terms(1.0, dqmin_da=x["dqmin_da"], scale=-0.3)["d_action"]) and g.guards_intact()


# ------------------------------------------------------------------------------------------------ NaN, repeatability, stream order
def test_a_nan_stays_in_its_row_or_in_the_scalars(env):
    count, row = 1025, 1024  # the one row of lane 0's second trip
    clean = EntropyCase(env, count)
    ref = clean.call()
    ref_state = {k: clean.g.host(k) for k in STATE}

    c = EntropyCase(env, count)
    nlp = c.x["next_log_prob"].copy()
    nlp[row] = NAN
    c.g.set("next_log_prob", nlp)
    got = c.call(same_y=same_but_nan)  # bitwise the restatement but for the NaN's own bits; the outputs were NaN-filled before the call
    assert np.isnan(got["y"][row]) and same(np.delete(got["y"], row), np.delete(ref["y"], row))
    assert all(same(c.g.host(k), ref_state[k]) for k in STATE) and same(got["d_log_prob"], ref["d_log_prob"]) and same(got["loss"], ref["loss"])

    c = EntropyCase(env, count)
    lp = c.x["log_prob"].copy()
    lp[row] = NAN
    c.g.set("log_prob", lp)
    env.entropy_step((c.g.t["l"], c.g.t["m"], c.g.t["v"]), c.g.t["log_prob"], TARGET_ENTROPY, step=1, ent_coef_out=c.g.t["ent_coef"], loss_out=c.g.t["loss"],
                     target=c.g.t["target"], next_log_prob=c.g.t["next_log_prob"], terminated=c.g.t["terminated"], gamma=GAMMA, y_out=c.g.t["y"],
                     d_log_prob_out=c.g.t["d_log_prob"], scale=1.0 / count, **HYPER)
    torch.cuda.synchronize(env.device)
    assert all(np.isnan(c.g.host(k)).all() for k in STATE + ("loss",))
    assert same(c.g.host("y"), ref["y"]) and same(c.g.host("d_log_prob"), ref["d_log_prob"]) and same(c.g.host("ent_coef"), clean.g.host("ent_coef"))
    assert c.g.guards_intact()


def test_two_runs_from_one_state_give_the_same_bits(env):
    count = 4097
    runs = []
    for _ in range(2):
        c = EntropyCase(env, count)
        c.call()
        x = inputs(count, seed=17)
        g = Guarded(dict(dqmin_da=x["dqmin_da"], q=x["q"], y=x["y"], log_prob=x["log_prob"], q_min=x["q_min"], d_action=np.full((count, 6), NAN),
                         critic_loss=np.full(1, NAN), actor_loss=np.full(1, NAN)), env.device)
        env.policy_terms(c.g.t["ent_coef"], count, dqmin_da=g.t["dqmin_da"], scale=-1.0 / count, d_action_out=g.t["d_action"], q=g.t["q"], y=g.t["y"],
                         critic_loss_out=g.t["critic_loss"], log_prob=g.t["log_prob"], q_min=g.t["q_min"], actor_loss_out=g.t["actor_loss"])
        torch.cuda.synchronize(env.device)
        runs.append([c.g.host(k) for k in STATE + ("ent_coef", "loss", "y", "d_log_prob")] + [g.host(k) for k in ("d_action", "critic_loss", "actor_loss")])
    assert all(same(a, b) for a, b in zip(*runs))


def critic_weights(rng, n_in, H):
    shapes = dict(zip(CRITIC_ARRAYS, ((H, n_in), (H,), (H, H), (H,), (1, H), (1,))))
    return [{k: (rng.standard_normal(sh) * 0.2).astype(np.float32) for k, sh in shapes.items()} for _ in range(2)]


def test_stream_order_without_a_synchronisation(env):
    """entropy_step, critic_parameter_gradients(target=y), entropy_step again into the same y, nothing synchronised in between: the
    gradients are those of the FIRST y."""
    rng = np.random.default_rng(5)
    count = env.num_envs  # the live rows
    critic = DeviceCritic(critic_weights(rng, env.obs_dim + 2 * env.goal_dim + 6, 32), env)
    actions = torch.from_numpy(rng.uniform(-1, 1, (count, 6)).astype(np.float32)).to(env.device)
    x = inputs(count, seed=19)
    dev = {k: torch.from_numpy(np.ascontiguousarray(x[k])).to(env.device) for k in ENTROPY_INPUTS + ("terminated",)}
    workspace = env.critic_gradient_workspace(critic, count)

    def state(l):
        return tuple(torch.full((1,), val, dtype=torch.float32, device=env.device) for val in (l, 0.0, 0.0))

    def step(st, y, k):
        env.entropy_step(st, dev["log_prob"], TARGET_ENTROPY, step=k, ent_coef_out=torch.empty((1,), device=env.device), target=dev["target"],
                         next_log_prob=dev["next_log_prob"], terminated=dev["terminated"], gamma=GAMMA, y_out=y, **HYPER)

    y, y_first = torch.zeros((count,), device=env.device), torch.zeros((count,), device=env.device)
    st = state(0.5)
    torch.cuda.synchronize(env.device)
    step(st, y, 1)
    got = env.critic_parameter_gradients(critic, actions, target=y, scale=1.0 / count, workspace=workspace)
    step(st, y, 2)  # overwrites y with the stepped l's alpha while (in host time) the gradient launches may not have run yet
    torch.cuda.synchronize(env.device)
    step(state(0.5), y_first, 1)
    torch.cuda.synchronize(env.device)
    assert not same(y.cpu().numpy(), y_first.cpu().numpy())  # the second call did change y
    want = env.critic_parameter_gradients(critic, actions, target=y_first, scale=1.0 / count)
    torch.cuda.synchronize(env.device)
    for n in (0, 1):
        for k in CRITIC_ARRAYS:
            assert same(got["grads"][n][k].cpu().numpy(), want["grads"][n][k].cpu().numpy()), (n, k)
    assert any(np.any(got["grads"][n][k].cpu().numpy() != 0) for n in (0, 1) for k in CRITIC_ARRAYS)
    critic.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_leaves_state_and_outputs_unchanged(env):
    lib, count = env.lib, 65
    c = EntropyCase(env, count)
    x = inputs(count, seed=17)
    p = Guarded(dict(dqmin_da=x["dqmin_da"], q=x["q"], y=x["y"], log_prob=x["log_prob"], q_min=x["q_min"], ent_coef=np.full(1, np.float32(0.5)),
                     d_action=np.full((count, 6), NAN), critic_loss=np.full(1, NAN), actor_loss=np.full(1, NAN)), env.device)
    torch.cuda.synchronize(env.device)
    before_c = {k: c.g.host(k) for k in c.g.t}
    before_p = {k: p.host(k) for k in p.t}
    stream = env._stream()
    fp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float))  # noqa: E731
    E_PTRS = dict(log_prob="log_prob", log_ent_coef="l", exp_avg="m", exp_avg_sq="v", ent_coef_out="ent_coef", loss_out="loss", target_in="target",
                  next_log_prob="next_log_prob", y_out="y", d_log_prob_out="d_log_prob")

    def e_args(null=(), **over):
        a = _abi.SacEntropyArgs(count, 0, TARGET_ENTROPY, GAMMA, 1.0 / count)
        for field, k in E_PTRS.items():
            if field not in null:
                setattr(a, field, fp(c.g.t[k]))
        if "terminated" not in null:
            a.terminated = C.cast(c.g.t["terminated"].data_ptr(), C.POINTER(C.c_uint8))
        for k, val in over.items():
            setattr(a, k, val)
        return a

    P_PTRS = dict(ent_coef="ent_coef", dqmin_da="dqmin_da", d_action_out="d_action", q="q", y="y", critic_loss_out="critic_loss", log_prob="log_prob",
                  q_min="q_min", actor_loss_out="actor_loss")

    def p_args(null=(), **over):
        a = _abi.SacPolicyArgs(count, 0, -1.0 / count)
        for field, k in P_PTRS.items():
            if field not in null:
                setattr(a, field, fp(p.t[k]))
        for k, val in over.items():
            setattr(a, k, val)
        return a

    def hyper(**over):
        return _abi.AdamHyper(**dict(dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=1, reserved0=0), **over))

    ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731
    call_e = lambda h, a, hp: lib.urgym_sac_entropy_step(h, ref(a), ref(hp), stream)  # noqa: E731
    call_p = lambda h, a: lib.urgym_sac_policy_terms(h, ref(a), stream)  # noqa: E731
    nan, inf = float("nan"), float("inf")
    bad_hyper = [dict(lr=-1e-4), dict(lr=nan), dict(lr=inf), dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=nan), dict(beta2=1.0), dict(beta2=-0.1),
                 dict(beta2=nan), dict(eps=0.0), dict(eps=-1e-8), dict(eps=nan), dict(eps=inf), dict(step=0), dict(step=-1), dict(reserved0=1)]
    target_group = ("target_in", "next_log_prob", "y_out")
    half_target = [tuple(f for f in target_group if f not in keep) for keep in (("target_in",), ("next_log_prob",), ("y_out",), ("target_in", "next_log_prob"),
                                                                                ("target_in", "y_out"), ("next_log_prob", "y_out"))]

    refused = [call_e(None, e_args(), hyper()), call_e(env._h, None, hyper()), call_e(env._h, e_args(), None)]
    refused += [call_e(env._h, e_args(null=(f,)), hyper()) for f in ("log_prob", "log_ent_coef", "exp_avg", "exp_avg_sq", "ent_coef_out")]
    refused += [call_e(env._h, e_args(count=n), hyper()) for n in (0, -1, _abi.SAC_TERMS_MAX_COUNT + 1, 2 ** 31 - 1)]
    refused += [call_e(env._h, e_args(reserved0=1), hyper())]
    refused += [call_e(env._h, e_args(**{k: val}), hyper()) for k in ("target_entropy", "gamma", "scale") for val in (nan, inf, -inf)]
    refused += [call_e(env._h, e_args(null=null), hyper()) for null in half_target]
    refused += [call_e(env._h, e_args(null=target_group), hyper())]  # terminated without its group
    refused += [call_e(env._h, e_args(), hyper(**over)) for over in bad_hyper]
    n_entropy = len(refused)
    assert n_entropy == 3 + 5 + 4 + 1 + 9 + 6 + 1 + 16

    groups = (("dqmin_da", "d_action_out"), ("q", "y", "critic_loss_out"), ("log_prob", "q_min", "actor_loss_out"))
    halves = [tuple(f for f in g if f not in keep) for g in groups for r in range(1, len(g)) for keep in _subsets(g, r)]
    refused += [call_p(None, p_args()), call_p(env._h, None), call_p(env._h, p_args(null=("ent_coef",)))]
    refused += [call_p(env._h, p_args(count=n)) for n in (0, -1, _abi.SAC_TERMS_MAX_COUNT + 1)]
    refused += [call_p(env._h, p_args(reserved0=1))]
    refused += [call_p(env._h, p_args(scale=val)) for val in (nan, inf, -inf)]
    refused += [call_p(env._h, p_args(null=null)) for null in halves]
    refused += [call_p(env._h, p_args(null=tuple(f for g in groups for f in g)))]  # no group at all
    assert len(refused) == n_entropy + 3 + 3 + 1 + 3 + (2 + 6 + 6) + 1
    assert refused == [_abi.ERR_ARG] * len(refused), refused
    assert b"no group" in lib.urgym_last_error(env._h)

    # the Python layer: half-given groups, and tensors that are not what the call reads or writes in place
    t, st = c.g.t, (c.g.t["l"], c.g.t["m"], c.g.t["v"])
    ok = dict(step=1, ent_coef_out=t["ent_coef"], **HYPER)
    with pytest.raises(ValueError, match="half given"):
        env.entropy_step(st, t["log_prob"], TARGET_ENTROPY, target=t["target"], next_log_prob=t["next_log_prob"], y_out=t["y"], **ok)  # no gamma
    with pytest.raises(ValueError, match="half given"):
        env.entropy_step(st, t["log_prob"], TARGET_ENTROPY, terminated=t["terminated"], **ok)
    with pytest.raises(ValueError, match="half given"):
        env.entropy_step(st, t["log_prob"], TARGET_ENTROPY, d_log_prob_out=t["d_log_prob"], **ok)  # no scale
    with pytest.raises(ValueError, match="finite"):
        env.entropy_step(st, t["log_prob"], nan, **ok)
    with pytest.raises(ValueError, match="finite"):
        env.entropy_step(st, t["log_prob"], TARGET_ENTROPY, d_log_prob_out=t["d_log_prob"], scale=1e39, **ok)  # infinite in float32
    with pytest.raises(ValueError, match="log_prob"):
        env.entropy_step(st, t["log_prob"].double(), TARGET_ENTROPY, **ok)
    with pytest.raises(ValueError, match="log_prob"):
        env.entropy_step(st, t["log_prob"].cpu(), TARGET_ENTROPY, **ok)
    with pytest.raises(ValueError, match="contiguous"):
        env.entropy_step(st, c.g.t["target"][::2], TARGET_ENTROPY, **ok)
    with pytest.raises(ValueError, match="ent_coef_out"):
        env.entropy_step(st, t["log_prob"], TARGET_ENTROPY, **dict(ok, ent_coef_out=t["y"]))  # [count], not [1]
    with pytest.raises(ValueError, match="y_out"):
        env.entropy_step(st, t["log_prob"], TARGET_ENTROPY, target=t["target"], next_log_prob=t["next_log_prob"], gamma=GAMMA, y_out=t["y"][:-1], **ok)
    with pytest.raises(ValueError, match="terminated"):
        env.entropy_step(st, t["log_prob"], TARGET_ENTROPY, target=t["target"], next_log_prob=t["next_log_prob"], gamma=GAMMA, y_out=t["y"],
                         terminated=t["y"], **ok)  # float32, not uint8 / bool
    with pytest.raises(ValueError, match="state"):
        env.entropy_step(st[:2], t["log_prob"], TARGET_ENTROPY, **ok)
    with pytest.raises(NativeError, match="step"):
        env.entropy_step(st, t["log_prob"], TARGET_ENTROPY, **dict(ok, step=0))
    with pytest.raises(ValueError, match="count"):
        env.policy_terms(p.t["ent_coef"], 0, log_prob=p.t["log_prob"], q_min=p.t["q_min"], actor_loss_out=p.t["actor_loss"])
    with pytest.raises(ValueError, match="no group"):
        env.policy_terms(p.t["ent_coef"], count)
    with pytest.raises(ValueError, match="half given"):
        env.policy_terms(p.t["ent_coef"], count, q=p.t["q"], y=p.t["y"])
    with pytest.raises(ValueError, match="q"):
        env.policy_terms(p.t["ent_coef"], count, q=p.t["q"][0], y=p.t["y"], critic_loss_out=p.t["critic_loss"])
    with pytest.raises(ValueError, match="finite"):
        env.policy_terms(p.t["ent_coef"], count, dqmin_da=p.t["dqmin_da"], d_action_out=p.t["d_action"], scale=inf)

    # nothing was launched: state, inputs and outputs are what they were, guards included
    torch.cuda.synchronize(env.device)
    for k, val in before_c.items():
        got = c.g.host(k)
        assert np.array_equal(got.view(np.uint8), val.view(np.uint8)), k
    for k, val in before_p.items():
        assert np.array_equal(words(p.host(k)), words(val)), k
    assert c.g.guards_intact() and p.guards_intact()
    # and everything still works
    c.call()
    assert call_p(env._h, p_args()) == _abi.OK
    torch.cuda.synchronize(env.device)
    want = policy_terms(np.float32(0.5), dqmin_da=x["dqmin_da"], scale=-1.0 / count, q=x["q"], y=x["y"], log_prob=x["log_prob"], q_min=x["q_min"])
    assert same(p.host("d_action"), want["d_action"]) and same(p.host("critic_loss")[0], want["critic_loss"]) and same(p.host("actor_loss")[0], want["actor_loss"])


def _subsets(items, r):
    import itertools

    return list(itertools.combinations(items, r))


# ------------------------------------------------------------------------------------------------ the learner
FOUR = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True)


def test_learner_with_the_device_entropy():
    from ur_gym_amd.training import SAC_DEFAULTS, SACLearner, host_arrays

    assert SAC_DEFAULTS["device_entropy"] is False
    env = make_vec("UR5OriReach-v1", num_envs=64, seed=5, auto_reset=True)
    env.reset(seed=5)
    M = 64
    with pytest.raises(ValueError, match="device_entropy needs"):
        SACLearner(env, seed=5, hidden_width=32, batch_size=M, device_entropy=True, **dict(FOUR, device_optimizer=False))
    learner = SACLearner(env, seed=5, hidden_width=32, batch_size=M, device_entropy=True, **FOUR)
    twin = SACLearner(env, seed=5, hidden_width=32, batch_size=M, **FOUR)  # the same seed: the same initial parameters
    assert twin.entropy_state is None and twin.last_update is None  # with the option off nothing new is allocated
    hp = learner.hp
    lr, gamma, te = hp["learning_rate"], float(hp["gamma"]), hp["target_entropy"]
    log_ent_coef = learner.log_ent_coef
    assert log_ent_coef.shape == (1,) and float(log_ent_coef.item()) == 0.0  # ent_coef_init = 1: alpha is exactly 1 at update 1
    replay = DeviceReplay(env, 8)
    learner.collect(replay, 8)
    f = np.float32

    # the twin's y of update 1, by the learner's torch lines on the same draw (sample_targets is a pure function of seed and draw)
    with torch.no_grad():
        batch = replay.sample_targets(twin.device_actor, twin.target, M, 11, 0, gamma, 0.0)
        discount = gamma * (~batch["terminated"]).to(torch.float32)
        y_twin = (batch["target"] - discount * twin.log_ent_coef.exp() * batch["next_log_prob"]).cpu().numpy()

    state = {k: np.zeros(1, f) for k in STATE}
    want_actor, want_critic = host_arrays(learner.actor.tensors()), host_arrays(learner.critic.tensors())
    zeros = lambda w: {k: np.zeros_like(v) for k, v in w.items()}  # noqa: E731
    m_a, v_a = zeros(want_actor), zeros(want_actor)
    m_c, v_c = [zeros(w) for w in want_critic], [zeros(w) for w in want_critic]
    for i in range(3):
        losses = learner.update(replay, seed=11, draw=i)
        torch.cuda.synchronize(env.device)
        assert learner.log_ent_coef is log_ent_coef and learner.adam_state["step"] == i + 1 and not learner.ent_opt.state  # ent_opt is not stepped
        es, last = learner.entropy_state, learner.last_update
        assert sorted(last) == ["dqmin_da", "log_prob", "q", "q_min", "y"] and last["y"] is es["y"]  # references, not copies
        assert all(v.dim() == 0 for v in losses.values()) and losses["critic_loss"].data_ptr() == es["critic_loss"].data_ptr()
        alpha = es["ent_coef"].cpu().numpy()[0]
        host = {k: v.cpu().numpy() for k, v in last.items()}
        coef = adam_coefficients(env, lr, (0.9, 0.999), 1e-8, i + 1)

        # log_ent_coef and its moments: bitwise the restatement on last_update
        want = entropy_step(alpha, host["log_prob"], te, state["l"], state["m"], state["v"], coef, scale=1.0 / M)
        l_old = state["l"].copy()
        got_state = dict(l=log_ent_coef.detach().cpu().numpy(), m=es["exp_avg"].cpu().numpy(), v=es["exp_avg_sq"].cpu().numpy())
        for k in STATE:
            assert same(got_state[k], want[k]), (i, k, got_state[k], want[k])
            state[k] = want[k]
        assert same(losses["ent_coef_loss"].cpu().numpy(), want["loss"]) and same(learner.actor_d_log_prob.cpu().numpy(), want["d_log_prob"])
        terms = policy_terms(alpha, dqmin_da=host["dqmin_da"], scale=-1.0 / M, q=host["q"], y=host["y"], log_prob=host["log_prob"], q_min=host["q_min"])
        assert same(learner.actor_d_action.cpu().numpy(), terms["d_action"])
        assert same(losses["critic_loss"].cpu().numpy(), terms["critic_loss"]) and same(losses["actor_loss"].cpu().numpy(), terms["actor_loss"])

        # each loss against the float64 mean of its own per-row terms: one rounding of a float64 sum (and of what is formed from it)
        s64 = host["log_prob"].astype(np.float64) + np.float64(f(te))
        per_row = {"ent_coef_loss": -(float(l_old[0]) * (host["log_prob"] + f(te)).astype(np.float64)),
                   "critic_loss": 0.5 * (terms["critic_terms"][0].astype(np.float64) + terms["critic_terms"][1].astype(np.float64)),
                   "actor_loss": terms["actor_terms"].astype(np.float64)}
        assert s64.shape == (M,)
        for k, t64 in per_row.items():
            err, bound = abs(float(losses[k].item()) - t64.mean()), 2.0 ** -23 * np.abs(t64).mean()
            print(f"update {i + 1} {k}: {float(losses[k].item()):.6e}, |loss - mean64| = {err:.3e} of bound {bound:.3e}")
            assert err <= bound, (i, k, err, bound)

        # the parameters: bitwise adam_step of the .grad tensors the kernels wrote
        g_a, g_c = host_arrays(learner.actor_grads), host_arrays(learner.critic_grads)
        for k in want_actor:
            want_actor[k], m_a[k], v_a[k] = adam_step(want_actor[k], g_a[k], m_a[k], v_a[k], coef)
        for n in (0, 1):
            for k in want_critic[n]:
                want_critic[n][k], m_c[n][k], v_c[n][k] = adam_step(want_critic[n][k], g_c[n][k], m_c[n][k], v_c[n][k], coef)
        got_actor, got_critic = host_arrays(learner.actor.tensors()), host_arrays(learner.critic.tensors())
        assert all(same(got_actor[k], want_actor[k]) for k in want_actor), i
        assert all(same(got_critic[n][k], want_critic[n][k]) for n in (0, 1) for k in want_critic[n]), i
        assert any(np.any(g != 0) for g in g_a.values()) and any(np.any(g != 0) for w in g_c for g in w.values())

        if i == 0:  # against the twin with the option off
            assert same(alpha, f(1))
            assert same(host["y"], y_twin)
            twin.update(replay, seed=11, draw=0)
            torch.cuda.synchronize(env.device)
            t_a, t_c = host_arrays(twin.actor_grads), host_arrays(twin.critic_grads)
            assert all(same(t_a[k], g_a[k]) for k in g_a) and all(same(t_c[n][k], g_c[n][k]) for n in (0, 1) for k in g_c[n])
            err, bound = abs(float(twin.log_ent_coef.item()) - float(log_ent_coef.item())), 2 * p_bound(1, lr, lr)
            print(f"update 1: |log_ent_coef - torch Adam's| = {err:.3e}, bound {bound:.3e}; log_ent_coef = {float(log_ent_coef.item()):.6e}")
            assert err <= bound and float(log_ent_coef.item()) != 0.0
    learner.collect(replay, 2)  # the sampled policy, on the actor the step kernel packed
    torch.cuda.synchronize(env.device)  # raises if any launch left an error
    assert np.isfinite(replay.ring["action"].cpu().numpy()).all()
    learner.close(), twin.close()
    env.close()


# names of operations that allocate or make a view: nothing among them launches a kernel
ALLOCATIONS_AND_VIEWS = {"aten.empty.memory_format", "aten.empty_strided.default", "aten.view.default", "aten.view.dtype", "aten._unsafe_view.default",
                         "aten.select.int", "aten.slice.Tensor", "aten.squeeze.dim", "aten.unsqueeze.default", "aten.expand.default",
                         "aten.as_strided.default", "aten.alias.default", "aten.detach.default"}


def test_update_runs_no_torch_operation_that_launches():
    from torch.utils._python_dispatch import TorchDispatchMode

    from ur_gym_amd.training import SACLearner

    class Recorder(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.append(str(func))
            return func(*args, **(kwargs or {}))

    env = make_vec("UR5OriReach-v1", num_envs=64, seed=5, auto_reset=True)
    env.reset(seed=5)
    seen = {}
    for label, options in (("device_entropy", dict(FOUR, device_entropy=True)), ("device_optimizer", FOUR)):
        learner = SACLearner(env, seed=5, hidden_width=32, batch_size=64, **options)
        replay = DeviceReplay(env, 4)
        learner.collect(replay, 4)
        learner.update(replay, seed=11, draw=0)  # whatever is made lazily is made here
        with Recorder() as rec:
            learner.update(replay, seed=11, draw=1)
        torch.cuda.synchronize(env.device)
        seen[label] = rec.names
        print(f"{label}: {len(rec.names)} torch operations in one update: {sorted(set(rec.names))}")
        learner.close()
    env.close()
    assert seen["device_entropy"] and "aten.empty.memory_format" in seen["device_entropy"]  # the recorder sees the allocations
    assert set(seen["device_entropy"]) <= ALLOCATIONS_AND_VIEWS, sorted(set(seen["device_entropy"]) - ALLOCATIONS_AND_VIEWS)
    # the same recorder on the route before does see what the option removes
    for prefix in ("aten.exp.", "aten.mul.", "aten.sub.", "aten.mean.", "aten.copy_."):
        assert any(n.startswith(prefix) for n in seen["device_optimizer"]), prefix
        assert not any(n.startswith(prefix) for n in seen["device_entropy"]), prefix
    assert not set(seen["device_optimizer"]) <= ALLOCATIONS_AND_VIEWS
