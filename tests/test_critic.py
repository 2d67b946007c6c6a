"""The twin Q critics on the device: urgym_critic_create / urgym_critic_evaluate / urgym_actor_sample_rows through ``DeviceCritic``,
``env.critic_values`` and ``env.policy_actions(rows=)``, and the numpy restatement ``TwinCritic``.

Where the bounds come from (no number is taken from what the kernel gives):
  * ``TwinCritic`` (float32) against float64: the running error bound of tests/test_policy_sampling.py::_f64, restated for a one-output
    head (``critic_f64``): a float32 sum of K products errs by at most (K + 1) 2^-24 sum |w_i x_i|, errors pass through the next layer
    multiplied by |W|, relu is 1-Lipschitz.
  * device against float64 on the checkpoints: 4 x the deviation of ``TwinCritic`` from float64, measured in the test on the same
    inputs (the project's rule for a second float32 evaluation order).  min is 1-Lipschitz in the maximum norm -- |min(a, b) -
    min(a', b')| <= max(|a - a'|, |b - b'|) -- so q_min has the bound of q and NO row is dropped.  target = r + (gamma nd) (q_min -
    alpha lp): the bound of q_min times gamma, plus four float32 roundings, 4 * 2^-24 (|r| + gamma |q_min| + gamma alpha |lp|) per row.
  * the exact network (construction of tests/test_actor_widths.py part 1): W0 / W1 dense +-1, inputs and hidden biases in {-1, 0, 1},
    head +-2^-S with a bias on that grid.  Every partial sum in any order is a multiple of the layer's grid and bounded by the sum of
    the magnitudes; below 2^24 grid units it is a float32 number, so float32 is exact and the device must equal float64 BITWISE.  The
    three epilogue operations have a fixed order (include/urgym.h); each exact result is shown to be a float32 number.

The GPU tests below have NOT been run yet: no MI355X was available when this file was written.  The CPU
figures are in DESIGN.md section 9; the GPU tests print theirs (run with -s) for profiles/policy_rollout/gpu_tests_critic.txt.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from test_actor_widths import CASES, COUNTS, GRID, OTHER_KIND_WIDTHS, WIDTHS, instance
from test_policy_sampling import ENVS, KINDS, U24, _same_bits, weights as actor_weights
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import CRITIC_ARRAYS, DeviceActor, DeviceCritic, TwinCritic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CRITICS = os.path.join(ROOT, "tests", "golden", "critics")
NEW_SYMBOLS = ("urgym_critic_create", "urgym_critic_destroy", "urgym_critic_evaluate", "urgym_actor_sample_rows")
NAMES = ("ori", "obs", "sta", "dyn")
IN_FEATURES = {"ori": 36, "obs": 38, "sta": 47, "dyn": 53}
# the exact network's target terms: powers of two, so that every product stays on a grid
EXACT_GAMMA, EXACT_ENT = 0.5, 0.25


def critic_paths(name):
    return [os.path.join(CRITICS, f"critic_{name}_qf{i}.npz") for i in (0, 1)]


def critic_weights(name):
    return [dict(np.load(p)) for p in critic_paths(name)]


def hyper(name):
    with open(os.path.join(CRITICS, "sac_hyperparameters.json")) as f:
        h = json.load(f)[name]
    return h["gamma"], float(np.exp(h["log_ent_coef"]))


def critic_f64(w, x):
    """One Q-network in float64 on float32 inputs, and the bound of what a float32 evaluation may deviate (module docstring)."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    x = x.astype(np.float64)

    def layer(W, b, v, ev):
        K = W.shape[1] + 1
        mag = np.abs(v) @ np.abs(W).T + np.abs(b)
        return v @ W.T + b, ev @ np.abs(W).T + (K + 1) * U24 * (mag + ev @ np.abs(W).T)

    z, e = layer(w["q_0_weight"], w["q_0_bias"], x, np.zeros_like(x))
    z, e = layer(w["q_2_weight"], w["q_2_bias"], np.maximum(z, 0.0), e)
    q, e = layer(w["q_4_weight"], w["q_4_bias"], np.maximum(z, 0.0), e)
    return q[:, 0], e[:, 0]


def target_f64(q0, q1, reward, gamma, terminated=None, log_prob=None, ent_coef=0.0):
    q_min = np.minimum(q0, q1)
    v = q_min if log_prob is None else q_min - float(np.float32(ent_coef)) * log_prob.astype(np.float64)
    nd = 1.0 if terminated is None else 1.0 - terminated.astype(bool).astype(np.float64)
    return q_min, reward.astype(np.float64) + float(np.float32(gamma)) * nd * v


def split(name, x):
    od, gd = _abi.OBS_DIMS[KINDS[name]]
    return x[:, :gd], x[:, gd:2 * gd], x[:, 2 * gd:2 * gd + od], x[:, 2 * gd + od:]


def trace_rows(name):
    """Real rows: the observations of the recorded steps with the recorded actions that followed them."""
    z = np.load(os.path.join(ROOT, "tests", "golden", f"step_trace_{name}.npz"))
    parts = [z["step_achieved_goal"][:-1], z["step_desired_goal"][:-1], z["step_observation"][:-1], z["actions"][1:]]
    return np.concatenate([p.reshape(-1, p.shape[-1]) for p in parts], axis=1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the exact network
def exact_inputs(kind, n):
    rng = np.random.default_rng([n, IN_FEATURES[kind], 11])
    return rng.integers(-1, 2, (n, IN_FEATURES[kind])).astype(np.float32)


def exact_critic(kind, H):
    """Two different networks of the construction of tests/test_actor_widths.py::exact_network, with a one-output head."""
    n_in = IN_FEATURES[kind]
    nets = []
    # the head: as many + as - weights, so that q spreads about the bias both networks share and either can be the minimum
    bias = (np.random.default_rng([H, n_in, 12]).integers(-1024, 1025, 1) * GRID).astype(np.float32)  # one head bias: either can be the minimum
    for i in (1, 2):
        rng = np.random.default_rng([H, n_in, 12 + i])
        sign = lambda shape: (rng.integers(0, 2, shape) * 2 - 1).astype(np.float32)  # noqa: E731
        plus = H // 2 + int(np.ceil(0.45 * np.sqrt(H)))  # every layer-2 neuron fires on most rows (see exact_network there)
        w1 = rng.permuted(np.where(np.arange(H) < plus, 1.0, -1.0)[None, :].repeat(H, axis=0), axis=1).astype(np.float32)
        nets.append({"q_0_weight": sign((H, n_in)), "q_0_bias": rng.integers(-1, 2, H).astype(np.float32),
                     "q_2_weight": w1, "q_2_bias": rng.integers(-1, 2, H).astype(np.float32),
                     "q_4_weight": rng.permutation(np.where(np.arange(H) < H // 2, 1.0, -1.0))[None, :].astype(np.float32) * np.float32(GRID), "q_4_bias": bias})
    return nets


def exact_terms(n):
    """Integer rewards, log-probabilities on the grid 4 * 2^-S (ent_coef = 1 / 4 brings them to 2^-S), some rows terminated."""
    rng = np.random.default_rng([n, 13])
    reward = rng.integers(-500, 201, n).astype(np.float32)
    log_prob = (rng.integers(-8192, 8193, n) * (4.0 * GRID)).astype(np.float32)
    terminated = (rng.random(n) < 0.25).astype(np.uint8)
    return reward, terminated, log_prob


def hidden2_f64(w, x):
    h = np.maximum(x.astype(np.float64) @ np.float64(w["q_0_weight"]).T + np.float64(w["q_0_bias"]), 0.0)
    return np.maximum(h @ np.float64(w["q_2_weight"]).T + np.float64(w["q_2_bias"]), 0.0)


def exact_reference(nets, x, terms):
    """float64: q [2, n], q_min, target with (EXACT_GAMMA, EXACT_ENT), and the intermediate results of the epilogue."""
    reward, terminated, log_prob = terms
    q = np.stack([critic_f64(w, x)[0] for w in nets])
    q_min = np.minimum(q[0], q[1])
    e = EXACT_ENT * log_prob.astype(np.float64)
    v = q_min - e
    g = EXACT_GAMMA * (1.0 - terminated.astype(np.float64))
    d = g * v
    return q, q_min, reward.astype(np.float64) + d, (e, v, g, d)


def is_float32(a):
    return np.array_equal(a.astype(np.float32).astype(np.float64), a)


# ------------------------------------------------------------------------------------------------ CPU
def test_critic_structs_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    ctype = {"const float*": C.POINTER(C.c_float), "float*": C.POINTER(C.c_float), "const uint8_t*": C.POINTER(C.c_uint8),
             "float": C.c_float, "int32_t": C.c_int32}

    def fields(struct):
        body = hdr[hdr.index(f"typedef struct {struct}"):hdr.index(f"}} {struct};")]
        return re.findall(r"^\s*(const float\*|const uint8_t\*|float\*|float|int32_t|urgym_q_network)\s+(\w+)(\[2\])?;", body, flags=re.M)

    got = fields("urgym_q_network")
    assert [(n, ctype[t]) for t, n, _ in got] == list(_abi.QNetwork._fields_) and [n for _, n, _ in got] == ["w0", "b0", "w1", "b1", "w_q", "b_q"]
    got = fields("urgym_critic_desc")
    assert [n for _, n, _ in got] == [f[0] for f in _abi.CriticDesc._fields_] == ["in_features", "hidden_width", "n_critics", "reserved0", "qf"]
    assert [ctype[t] for t, _, _ in got[:4]] == [f[1] for f in _abi.CriticDesc._fields_[:4]]
    assert got[4] == ("urgym_q_network", "qf", "[2]") and _abi.CriticDesc._fields_[4][1] is _abi.QNetwork * 2
    assert C.sizeof(_abi.CriticDesc) == 16 + 12 * C.sizeof(C.c_void_p)
    for struct, mirror, n in (("urgym_critic_rows", _abi.CriticRows, 4), ("urgym_critic_terms", _abi.CriticTerms, 5), ("urgym_critic_out", _abi.CriticOut, 3)):
        got = fields(struct)
        assert [(name, ctype[t]) for t, name, _ in got] == list(mirror._fields_) and len(got) == n, struct
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
        assert re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym  # one line, starting with int
    assert lib.urgym_abi_version() == 4


def test_critic_shape_checks_need_no_gpu():
    for name in NAMES:
        w = critic_weights(name)
        assert DeviceCritic.check_shapes(w, KINDS[name]) == (IN_FEATURES[name], 256)
        other = "obs" if name != "obs" else "dyn"
        with pytest.raises(ValueError, match="features"):  # wrong in_features for the env kind
            DeviceCritic.check_shapes(w, KINDS[other])
    w = critic_weights("dyn")
    cut = dict(w[1], q_2_weight=w[1]["q_2_weight"][:128], q_2_bias=w[1]["q_2_bias"][:128], q_4_weight=w[1]["q_4_weight"][:, :128])
    with pytest.raises(ValueError, match="one width"):  # unequal hidden widths within a network
        DeviceCritic.check_shapes([w[0], cut], _abi.ENV_DYN)

    def narrow(net, H):
        return {"q_0_weight": net["q_0_weight"][:1].repeat(H, 0), "q_0_bias": np.zeros(H, np.float32), "q_2_weight": np.zeros((H, H), np.float32),
                "q_2_bias": np.zeros(H, np.float32), "q_4_weight": np.zeros((1, H), np.float32), "q_4_bias": np.zeros(1, np.float32)}

    with pytest.raises(ValueError, match="one hidden width"):  # unequal between the twins
        DeviceCritic.check_shapes([w[0], narrow(w[0], 128)], _abi.ENV_DYN)
    for H in (48, 544):
        with pytest.raises(ValueError, match="multiple of 32"):
            DeviceCritic.check_shapes([narrow(w[0], H), narrow(w[0], H)], _abi.ENV_DYN)
    assert DeviceCritic.check_shapes([narrow(w[0], 512), narrow(w[0], 512)], _abi.ENV_DYN) == (53, 512)
    two = dict(w[0], q_4_weight=np.zeros((2, 256), np.float32), q_4_bias=np.zeros(2, np.float32))
    with pytest.raises(ValueError, match="1 output"):
        DeviceCritic.check_shapes([two, w[1]], _abi.ENV_DYN)
    with pytest.raises(ValueError, match="two Q-networks"):  # a missing twin
        DeviceCritic.check_shapes([w[0]], _abi.ENV_DYN)
    with pytest.raises(ValueError, match="missing"):
        DeviceCritic.check_shapes([w[0], {k: v for k, v in w[1].items() if k != "q_4_bias"}], _abi.ENV_DYN)


def test_fixtures_and_hyperparameters():
    for name in NAMES:
        for w in critic_weights(name):
            assert set(w) == set(CRITIC_ARRAYS) and all(v.dtype == np.float32 for v in w.values())
        gamma, alpha = hyper(name)
        assert gamma == 0.95 and 1.0 < alpha < 2.5
    for p in sum((critic_paths(n) for n in NAMES), []):
        assert os.path.getsize(p) < 1 << 20


@pytest.mark.parametrize("name", NAMES)
def test_twin_critic_against_float64(name):
    nets = critic_weights(name)
    x = trace_rows(name)
    assert x.shape == (35 * 48, IN_FEATURES[name]) and x.dtype == np.float32
    host = TwinCritic(nets)
    got = host(*split(name, x))
    assert all(g.dtype == np.float32 and g.shape == (len(x),) for g in got)
    ref = []
    for i, w in enumerate(nets):
        q64, err = critic_f64(w, x)
        dev = np.abs(got[i].astype(np.float64) - q64)
        print(f"{name} qf{i}: float32 vs float64 {dev.max():.3e} on |q| up to {np.abs(q64).max():.4g}, largest bound {err.max():.3e}, "
              f"largest deviation / bound {float((dev / err).max()):.3e}")
        assert np.all(dev <= err), (name, i, float((dev - err).max()))
        ref.append(q64)
    # the target: float32 operation by operation from the float32 q, against float64 from the same float32 q
    gamma, alpha = hyper(name)
    rng = np.random.default_rng(4)
    reward = rng.uniform(-60.0, 5.0, len(x)).astype(np.float32)
    log_prob = rng.uniform(-12.0, 6.0, len(x)).astype(np.float32)
    term = (rng.random(len(x)) < 0.2).astype(np.uint8)
    q_min, tgt = TwinCritic.target(got[0], got[1], reward, gamma, term, log_prob, alpha)
    assert q_min.dtype == tgt.dtype == np.float32 and np.array_equal(q_min, np.minimum(got[0], got[1]))
    qm64, t64 = target_f64(got[0].astype(np.float64), got[1].astype(np.float64), reward, gamma, term, log_prob, alpha)
    slack = 4 * U24 * (np.abs(reward) + gamma * np.abs(qm64) + gamma * alpha * np.abs(log_prob))
    assert np.all(np.abs(tgt.astype(np.float64) - t64) <= slack)
    assert np.array_equal(tgt[term == 1], reward[term == 1])  # a terminal row's target is its reward
    no_ent = TwinCritic.target(got[0], got[1], reward, gamma, term)[1]
    assert np.array_equal(no_ent, TwinCritic.target(got[0], got[1], reward, gamma, term, np.zeros_like(log_prob), alpha)[1])


def test_cases_reach_every_critic_instance():
    assert {instance(H) for H in WIDTHS} == {instance(H) for H in OTHER_KIND_WIDTHS} == {4, 8, 12, 16}
    assert [IN_FEATURES[k] for k in NAMES] == [sum(_abi.OBS_DIMS[KINDS[k]]) + _abi.OBS_DIMS[KINDS[k]][1] + 6 for k in NAMES]
    assert max(IN_FEATURES.values()) == 53  # more than the actor's 48 padded inputs: the kernel pads layer 1 to 56
    for kind, H in CASES:
        assert DeviceCritic.check_shapes(exact_critic(kind, H), KINDS[kind]) == (IN_FEATURES[kind], H)


@pytest.mark.parametrize("kind,H", CASES, ids=[f"{k}-{H}" for k, H in CASES])
def test_exact_critic_is_exact_in_float32(kind, H):
    nets = exact_critic(kind, H)
    host = TwinCritic(nets)
    assert not np.array_equal(nets[0]["q_2_weight"], nets[1]["q_2_weight"])
    for w in nets:
        assert np.all(np.abs(w["q_0_weight"]) == 1.0) and np.all(np.abs(w["q_2_weight"]) == 1.0)  # dense: every slot of the packing counts
        assert np.all(np.abs(w["q_4_weight"]) == np.float32(GRID))
    for n in COUNTS + (2048,):
        x = exact_inputs(kind, n)
        assert set(np.unique(x)) <= {-1.0, 0.0, 1.0}
        terms = exact_terms(n)
        worst = 0.0
        for w in nets:  # the proof: sums of magnitudes in grid units, what no partial sum in any order can exceed
            a = {k: np.abs(np.asarray(v, dtype=np.float64)) for k, v in w.items()}
            m1 = np.abs(x.astype(np.float64)) @ a["q_0_weight"].T + a["q_0_bias"]
            m2 = m1 @ a["q_2_weight"].T + a["q_2_bias"]
            m3 = (m2 @ a["q_4_weight"].T + a["q_4_bias"]) / GRID
            worst = max(worst, m1.max(), m2.max(), m3.max())
        assert worst < 2.0 ** 24, (kind, H, n, worst)
        q, q_min, target, (e, v, g, d) = exact_reference(nets, x, terms)
        # the epilogue has ONE order: each exact intermediate result is a float32 number, so each rounded operation is exact
        for step in (e, v, g, d, target):
            assert is_float32(step), (kind, H, n)
        assert max(np.abs(v).max() / GRID, np.abs(d).max() / (GRID / 2), np.abs(target).max() / (GRID / 2)) < 2.0 ** 24  # each on its grid
        got = host(*split(kind, x))
        assert got[0].dtype == np.float32 and np.array_equal(got[0].astype(np.float64), q[0]) and np.array_equal(got[1].astype(np.float64), q[1])
        qm32, t32 = TwinCritic.target(got[0], got[1], terms[0], EXACT_GAMMA, terms[1], terms[2], EXACT_ENT)
        assert qm32.dtype == t32.dtype == np.float32
        assert np.array_equal(qm32.astype(np.float64), q_min) and np.array_equal(t32.astype(np.float64), target)
        # another float32 summation order: the neurons of both hidden layers backwards
        back = [{"q_0_weight": np.ascontiguousarray(w["q_0_weight"][::-1]), "q_0_bias": np.ascontiguousarray(w["q_0_bias"][::-1]),
                 "q_2_weight": np.ascontiguousarray(w["q_2_weight"][::-1, ::-1]), "q_2_bias": np.ascontiguousarray(w["q_2_bias"][::-1]),
                 "q_4_weight": np.ascontiguousarray(w["q_4_weight"][:, ::-1]), "q_4_bias": w["q_4_bias"]} for w in nets]
        again = TwinCritic(back)(*split(kind, x))
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
        assert (q != 0.0).any(axis=1).all() and np.all(target[terms[1] == 1] == terms[0][terms[1] == 1])  # all-zero output cannot pass
        if n >= 128:  # both networks are the minimum somewhere; terminal and other rows
            assert (q[0] < q[1]).any() and (q[1] < q[0]).any() and terms[1].any() and not terms[1].all()
    # sensitivity (n = 2048): ONE misplaced weight changes q, bitwise, wherever its input neuron fires
    shares, shares2 = [], []
    for w in nets:
        h1 = np.maximum(x.astype(np.float64) @ np.float64(w["q_0_weight"]).T + np.float64(w["q_0_bias"]), 0.0)
        h2 = hidden2_f64(w, x)
        shares.append((h2 > 0.0).mean(axis=0).min())  # a flipped head weight j moves q by -2 w_j h2[:, j]: non-zero where h2[:, j] > 0
        # two head weights exchanged (a misplacement within the packing): q moves by (w_i - w_j)(h2_j - h2_i)
        j = np.arange(H - 1)
        differ = np.float64(w["q_4_weight"])[0, j] != np.float64(w["q_4_weight"])[0, j + 1]
        moved = (h2[:, j] != h2[:, j + 1])[:, differ].mean(axis=0)
        shares.append(moved.min() if differ.any() else 1.0)
        # a flipped layer-2 weight (i, j) moves the pre-activation of neuron i by -2 w h1[:, j]: seen where h1_j > 0 (about half the
        # rows) and neuron i fires before or after (about 70 %); sampled pairs.  Any share above 0 fails a bitwise comparison.
        rng = np.random.default_rng([H, 14])
        z2 = h1 @ np.float64(w["q_2_weight"]).T + np.float64(w["q_2_bias"])
        for i, jj in zip(rng.integers(0, H, 64), rng.integers(0, H, 64)):
            z_new = z2[:, i] - 2.0 * float(w["q_2_weight"][i, jj]) * h1[:, jj]
            shares2.append(float((np.maximum(z_new, 0.0) != np.maximum(z2[:, i], 0.0)).mean()))
    print(f"{kind} H={H}: largest magnitude bound {worst:.4g} of {2.0 ** 24:.4g}; a misplaced head weight changes q on at least {min(shares):.3f} "
          f"of the rows, a flipped layer-2 weight its neuron on at least {min(shares2):.3f}")
    assert min(shares) > 0.5 and min(shares2) > 0.1, (kind, H, min(shares), min(shares2))


def test_generator_reproduces_the_fixtures():
    reference = "/root/reference"
    if not os.path.isdir(os.path.join(reference, "Trained_Models")):
        pytest.skip("the reference checkpoints are not on this machine")
    import importlib.util

    spec = importlib.util.spec_from_file_location("gen_critic_fixtures", os.path.join(ROOT, "tests", "golden", "gen_critic_fixtures.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    arrays, hyp = gen.export(reference)
    assert sorted(arrays) == sorted(os.path.basename(p) for n in NAMES for p in critic_paths(n))
    for fname, arrs in arrays.items():
        have = dict(np.load(os.path.join(CRITICS, fname)))
        assert set(have) == set(arrs) == set(CRITIC_ARRAYS)
        for k in arrs:
            assert have[k].dtype == arrs[k].dtype == np.float32 and have[k].tobytes() == arrs[k].tobytes(), (fname, k)
    with open(os.path.join(CRITICS, "sac_hyperparameters.json")) as f:
        assert json.load(f) == hyp


# ------------------------------------------------------------------------------------------------ GPU
def _env(kind, n, seed=1, **kw):
    from ur_gym_amd import make_vec

    env = make_vec(ENVS[kind], num_envs=n, device="cuda:0", seed=seed, **kw)
    env.reset(seed=seed)
    return env


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _np_bits_equal(got, want64):
    """float32 device result == the float64 reference, bit for bit (the reference is a float32 number: CPU test)."""
    got = got.cpu().numpy()
    return got.dtype == np.float32 and got.shape == want64.shape and np.array_equal(got.view(np.uint32), want64.astype(np.float32).view(np.uint32))


def _bound_rows(env):
    return {k: env.buf[k].clone() for k in ("observation", "achieved_goal", "desired_goal")}


def checkpoint_values(name, n=4096):
    """Test 6's body; returns what the refusal test compares with.  After 20 random steps: actions (a) uniform random, without
    entropy term; (b) drawn by the policy (GAUSSIAN), with its log-probabilities.  Reward and terminated are the last step's."""
    import torch

    env = _env(name, n, seed=31)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(6)
    for _ in range(20):
        env.step(torch.rand((n, 6), device="cuda:0", generator=g) * 2.0 - 1.0)
    nets = critic_weights(name)
    gamma, alpha = hyper(name)
    critic = DeviceCritic.load(critic_paths(name), env)
    actor = DeviceActor(actor_weights(name), env)
    uniform = torch.rand((n, 6), device="cuda:0", generator=g) * 2.0 - 1.0
    sampled, log_prob = env.policy_actions(actor, sample=dict(mode="gaussian", seed=17, first_draw=3))
    reward, term = env.buf["reward"].clone(), env.buf["terminated"].clone()
    x_obs = np.concatenate([env.buf[k].cpu().numpy() for k in ("achieved_goal", "desired_goal", "observation")], axis=1)
    host = TwinCritic(nets)
    results = {}
    for label, act, lp in (("uniform", uniform, None), ("gaussian", sampled, log_prob)):
        got = env.critic_values(critic, act, reward=reward, terminated=term, log_prob=lp, gamma=gamma, ent_coef=alpha)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in got.items()}
        assert got["q"].shape == (2, n) and got["q_min"].shape == got["target"].shape == (n,)
        assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
        x = np.concatenate([x_obs, act.cpu().numpy()], axis=1).astype(np.float32)
        r, t, lp_np = reward.cpu().numpy(), term.cpu().numpy(), (lp.cpu().numpy() if lp is not None else None)
        q64 = np.stack([critic_f64(w, x)[0] for w in nets])
        q32 = np.stack(host(*split(name, x)))
        dev_numpy = float(np.abs(q32.astype(np.float64) - q64).max())
        bound_q = 4.0 * dev_numpy
        qm64, t64 = target_f64(q64[0], q64[1], r, gamma, t, lp_np, alpha)
        g32, a32 = float(np.float32(gamma)), float(np.float32(alpha))
        bound_t = g32 * bound_q + 4 * U24 * (np.abs(r) + g32 * np.abs(qm64) + (g32 * a32 * np.abs(lp_np) if lp_np is not None else 0.0))
        dev = {"q": float(np.abs(got["q"] - q64).max()), "q_min": float(np.abs(got["q_min"] - qm64).max())}
        worst_t = float((np.abs(got["target"] - t64) / bound_t).max())
        line = (f"critic {name} {label} N={n}: |q| up to {np.abs(q64).max():.4g}; numpy float32 vs float64 {dev_numpy:.3e}, kernel vs float64 "
                f"q {dev['q']:.3e} q_min {dev['q_min']:.3e} (bound {bound_q:.3e}, no row dropped); target {np.abs(got['target'] - t64).max():.3e}, "
                f"largest deviation / bound {worst_t:.3f}; terminated rows {int(t.sum())}")
        print(line)
        assert dev["q"] <= bound_q and dev["q_min"] <= bound_q, (name, label, dev, bound_q)
        assert worst_t <= 1.0, (name, label, worst_t)
        # the float32 restatement of the epilogue is bitwise, given the kernel's own q
        qm32, t32 = TwinCritic.target(got["q"][0], got["q"][1], r, gamma, t, lp_np, alpha)
        assert np.array_equal(qm32.view(np.uint32), got["q_min"].view(np.uint32)) and np.array_equal(t32.view(np.uint32), got["target"].view(np.uint32))
        results[label] = got
    return env, critic, actor, (uniform, sampled, log_prob, reward, term, gamma, alpha), results


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_checkpoints_against_float64(name):
    env, critic, actor, _, _ = checkpoint_values(name)
    critic.close()
    actor.close()
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,H", CASES, ids=[f"{k}-{H}" for k, H in CASES])
def test_exact_critic_on_the_device(kind, H):
    """critic_kernel<HT> at the width's instance: explicit rows at every count of COUNTS, and the bound buffers (M = N = 417), bitwise
    float64 for q, q_min and target.  Neither reference q is all zero (CPU test), so an output nobody wrote cannot pass."""
    import torch

    nets = exact_critic(kind, H)
    n_env = max(COUNTS)
    env = _env(kind, n_env)
    critic = DeviceCritic(nets, env)
    for n in COUNTS:
        x = exact_inputs(kind, n)
        reward, term, lp = exact_terms(n)
        q, q_min, target, _ = exact_reference(nets, x, (reward, term, lp))
        ach, des, obs, act = (_dev(p) for p in split(kind, x))
        got = env.critic_values(critic, act, rows=dict(observation=obs, achieved_goal=ach, desired_goal=des), reward=_dev(reward),
                                terminated=_dev(term), log_prob=_dev(lp), gamma=EXACT_GAMMA, ent_coef=EXACT_ENT)
        torch.cuda.synchronize()
        assert _np_bits_equal(got["q"], q) and _np_bits_equal(got["q_min"], q_min) and _np_bits_equal(got["target"], target), (kind, H, n)
        if n == n_env:  # the bound buffers
            for key, part in (("achieved_goal", ach), ("desired_goal", des), ("observation", obs)):
                env.buf[key].copy_(part)
            bound = env.critic_values(critic, act, reward=_dev(reward), terminated=_dev(term), log_prob=_dev(lp), gamma=EXACT_GAMMA, ent_coef=EXACT_ENT)
            torch.cuda.synchronize()
            assert all(_same_bits(bound[k], got[k]) for k in ("q", "q_min", "target")), (kind, H)
            no_ent = env.critic_values(critic, act, reward=_dev(reward), gamma=EXACT_GAMMA)  # no log_prob, nowhere terminated
            assert _np_bits_equal(no_ent["target"], reward.astype(np.float64) + EXACT_GAMMA * q_min)
    critic.close()
    env.close()
    print(f"exact critic {kind} H={H} HT={instance(H)} (M = {COUNTS} explicit rows, N = {n_env} bound): q, q_min, target bitwise float64")


@pytest.mark.gpu
def test_rows_are_independent():
    import torch

    name, n, K = "dyn", 300, 5
    env = _env(name, n, seed=9)
    critic = DeviceCritic.load(critic_paths(name), env)
    actor = DeviceActor(actor_weights(name), env)
    rec = env.rollout_policy(actor, K, record=("observation", "achieved_goal", "desired_goal", "action", "reward", "terminated"))
    gamma, alpha = hyper(name)
    whole = env.critic_values(critic, rec["action"], rows=rec, reward=rec["reward"], terminated=rec["terminated"], gamma=gamma, ent_coef=alpha)
    assert whole["q"].shape == (2, K, n) and whole["q_min"].shape == whole["target"].shape == (K, n)
    for k in range(K):  # K N rows in one launch == K launches of N rows
        step = env.critic_values(critic, rec["action"][k], rows={key: rec[key][k] for key in env.ROW_KEYS}, reward=rec["reward"][k],
                                 terminated=rec["terminated"][k], gamma=gamma, ent_coef=alpha)
        assert _same_bits(step["q"], whole["q"][:, k].contiguous()) and _same_bits(step["q_min"], whole["q_min"][k]) and _same_bits(step["target"], whole["target"][k])
    flat = env.critic_values(critic, rec["action"].reshape(K * n, 6), rows=tuple(rec[key].reshape(K * n, -1) for key in env.ROW_KEYS))
    assert _same_bits(flat["q"], whole["q"].reshape(2, K * n)) and "target" not in flat
    odd = env.critic_values(critic, rec["action"].reshape(K * n, 6)[7:138], rows=tuple(rec[key].reshape(K * n, -1)[7:138] for key in env.ROW_KEYS))
    assert _same_bits(odd["q"], whole["q"].reshape(2, K * n)[:, 7:138].contiguous())  # another position, another geometry
    # the bound buffers == explicit rows on copies of them
    act = rec["action"][0]
    assert _same_bits(env.critic_values(critic, act)["q"], env.critic_values(critic, act, rows=_bound_rows(env))["q"])
    # the twins exchanged
    nets = critic_weights(name)
    swapped = DeviceCritic([nets[1], nets[0]], env)
    other = env.critic_values(swapped, rec["action"], rows=rec)
    torch.cuda.synchronize()
    assert _same_bits(other["q"][0], whole["q"][1]) and _same_bits(other["q"][1], whole["q"][0]) and _same_bits(other["q_min"], whole["q_min"])
    assert not _same_bits(whole["q"][0], whole["q"][1])
    for obj in (swapped, critic, actor):
        obj.close()
    env.close()


@pytest.mark.gpu
def test_actor_sample_rows():
    import torch

    name, n, K, seed, first = "dyn", 417, 4, 23, (1 << 32) - 2
    env = _env(name, n, seed=4)
    actor = DeviceActor(actor_weights(name), env)
    how = dict(mode="gaussian", seed=seed, first_draw=first)
    a0, lp0 = env.policy_actions(actor, sample=how)
    a1, lp1 = env.policy_actions(actor, sample=how, rows=_bound_rows(env))  # copies of the bound buffers
    assert _same_bits(a0, a1) and _same_bits(lp0, lp1)
    assert _same_bits(env.policy_actions(actor), env.policy_actions(actor, rows=_bound_rows(env)))  # without sample: the mean action
    m0, mlp0 = env.policy_actions(actor, sample=dict(mode="mean"))
    m1, mlp1 = env.policy_actions(actor, sample=dict(mode="mean"), rows=_bound_rows(env))
    assert _same_bits(m0, m1) and _same_bits(mlp0, mlp1)
    rec = env.rollout_policy(actor, K, record=("observation", "achieved_goal", "desired_goal", "action", "log_prob"), sample=how)
    for k in range(K):  # the step-k slice with draw first + k
        a, lp = env.policy_actions(actor, sample=dict(how, first_draw=first + k), rows={key: rec[key][k] for key in env.ROW_KEYS})
        assert _same_bits(a, rec["action"][k]) and _same_bits(lp, rec["log_prob"][k]), k
    allk, _ = env.policy_actions(actor, sample=how, rows=rec)  # [K, N] rows in one launch: the env word is the row index
    torch.cuda.synchronize()
    assert allk.shape == (K, n, 6) and _same_bits(allk[0], rec["action"][0]) and not _same_bits(allk[1], rec["action"][1])
    actor.close()
    env.close()


@pytest.mark.gpu
def test_refusals_leave_the_handle_usable():
    import torch

    name = "dyn"
    env, critic, actor, (uniform, sampled, log_prob, reward, term, gamma, alpha), results = checkpoint_values(name, n=512)
    lib, h, n = env.lib, env._h, env.num_envs
    fp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float))  # noqa: E731
    rows_b = _bound_rows(env)
    rows = _abi.CriticRows(fp(rows_b["observation"]), fp(rows_b["achieved_goal"]), fp(rows_b["desired_goal"]), fp(uniform))
    bound = _abi.CriticRows(None, None, None, fp(uniform))
    q = torch.empty((2, n), dtype=torch.float32, device="cuda:0")
    tgt = torch.empty((n,), dtype=torch.float32, device="cuda:0")
    out_q, out_t, out_none = _abi.CriticOut(fp(q), None, None), _abi.CriticOut(None, None, fp(tgt)), _abi.CriticOut()
    no_reward = _abi.CriticTerms(None, None, None, gamma, alpha)
    s = env._stream()

    def refused(rc, call):
        msg = lib.urgym_last_error(h).decode()
        assert rc == _abi.ERR_ARG and call in msg, (rc, msg)

    ev = lib.urgym_critic_evaluate
    refused(ev(h, None, C.byref(rows), n, None, C.byref(out_q), s), "urgym_critic_evaluate")
    refused(ev(h, actor._a, C.byref(rows), n, None, C.byref(out_q), s), "urgym_critic_evaluate")  # not a critic
    refused(ev(h, critic._c, None, n, None, C.byref(out_q), s), "urgym_critic_evaluate")
    refused(ev(h, critic._c, C.byref(rows), n, None, None, s), "urgym_critic_evaluate")
    refused(ev(h, critic._c, C.byref(rows), 0, None, C.byref(out_q), s), "urgym_critic_evaluate")
    refused(ev(h, critic._c, C.byref(rows), -5, None, C.byref(out_q), s), "urgym_critic_evaluate")
    refused(ev(h, critic._c, C.byref(bound), n - 1, None, C.byref(out_q), s), "urgym_critic_evaluate")  # bound buffers: count == N
    refused(ev(h, critic._c, C.byref(_abi.CriticRows(rows.observation, None, rows.desired_goal, rows.action)), n, None, C.byref(out_q), s), "urgym_critic_evaluate")
    refused(ev(h, critic._c, C.byref(_abi.CriticRows(rows.observation, rows.achieved_goal, rows.desired_goal, None)), n, None, C.byref(out_q), s), "urgym_critic_evaluate")
    refused(ev(h, critic._c, C.byref(rows), n, None, C.byref(out_t), s), "urgym_critic_evaluate")  # target without terms
    refused(ev(h, critic._c, C.byref(rows), n, C.byref(no_reward), C.byref(out_t), s), "urgym_critic_evaluate")  # ... without reward
    refused(ev(h, critic._c, C.byref(rows), n, None, C.byref(out_none), s), "urgym_critic_evaluate")  # no output at all
    # urgym_critic_create
    nets = [[np.ascontiguousarray(w[k], dtype=np.float32) for k in CRITIC_ARRAYS] for w in critic_weights(name)]

    def desc(in_features=53, hidden=256, n_critics=2, reserved0=0, drop=False):
        d = _abi.CriticDesc(in_features, hidden, n_critics, reserved0)
        for i in (0, 1):
            d.qf[i] = _abi.QNetwork(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in nets[i]])
        if drop:
            d.qf[1].w_q = None
        return d

    made = C.c_void_p()
    for bad in (desc(n_critics=1), desc(n_critics=3), desc(reserved0=1), desc(in_features=47), desc(hidden=48), desc(hidden=544), desc(drop=True)):
        refused(lib.urgym_critic_create(h, C.byref(bad), C.byref(made)), "urgym_critic_create")
    refused(lib.urgym_critic_create(h, None, C.byref(made)), "urgym_critic_create")
    refused(lib.urgym_critic_create(h, C.byref(desc()), None), "urgym_critic_create")
    refused(lib.urgym_critic_destroy(h, actor._a), "urgym_critic_destroy")
    # urgym_actor_sample_rows
    how = _abi.Sampling(_abi.SAMPLE_GAUSSIAN, 0, 17, 3)
    acts = torch.empty((n, 6), dtype=torch.float32, device="cuda:0")
    sr = lib.urgym_actor_sample_rows
    refused(sr(h, critic._c, C.byref(how), C.byref(rows), n, acts.data_ptr(), None, s), "urgym_actor_sample_rows")  # not an actor
    refused(sr(h, actor._a, None, C.byref(rows), n, acts.data_ptr(), None, s), "urgym_actor_sample_rows")
    refused(sr(h, actor._a, C.byref(how), None, n, acts.data_ptr(), None, s), "urgym_actor_sample_rows")
    refused(sr(h, actor._a, C.byref(how), C.byref(rows), 0, acts.data_ptr(), None, s), "urgym_actor_sample_rows")
    refused(sr(h, actor._a, C.byref(how), C.byref(bound), n + 1, acts.data_ptr(), None, s), "urgym_actor_sample_rows")
    refused(sr(h, actor._a, C.byref(how), C.byref(rows), n, None, None, s), "urgym_actor_sample_rows")
    refused(sr(h, actor._a, C.byref(_abi.Sampling(7, 0, 0, 0)), C.byref(rows), n, acts.data_ptr(), None, s), "urgym_actor_sample_rows")
    with pytest.raises(ValueError):
        env.critic_values(critic, uniform, reward=reward)  # the Python verb asks for gamma
    with pytest.raises(ValueError):
        env.critic_values(actor, uniform)
    # the handle is as usable as before: the valid evaluations of test 6 again, bitwise
    for label, act, lp in (("uniform", uniform, None), ("gaussian", sampled, log_prob)):
        again = env.critic_values(critic, act, reward=reward, terminated=term, log_prob=lp, gamma=gamma, ent_coef=alpha)
        torch.cuda.synchronize()
        for k, v in again.items():
            assert np.array_equal(v.cpu().numpy().view(np.uint32), results[label][k].view(np.uint32)), (label, k)
    a2, lp2 = env.policy_actions(actor, sample=dict(mode="gaussian", seed=17, first_draw=3))
    assert _same_bits(a2, sampled) and _same_bits(lp2, log_prob)
    critic.close()
    actor.close()
    env.close()
