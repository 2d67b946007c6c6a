"""The stochastic half of the SAC policy on the device: urgym_actor_set_log_std / urgym_actor_sample / urgym_rollout_sampled through
``DeviceActor``, ``policy_actions(sample=)`` and ``rollout_policy(sample=)``, and its numpy restatement (``policy_noise``,
``StochasticActor``).

Where the bounds come from:
  * noise statistics: 1.95 / sqrt(M) is the 0.1 % point of the Kolmogorov-Smirnov statistic, 3.3 / sqrt(M) the 0.1 % two-sided
    point of a sample correlation of M independent pairs; the seeds are fixed, so the tests are deterministic;
  * ``StochasticActor`` (float32) against float64: a running error bound of the float32 evaluation, computed in float64 from the
    weights and inputs themselves (``_f64`` below): a float32 sum of K products errs by at most K 2^-24 sum |w_i x_i|, errors
    pass through the next layer multiplied by |W|, relu and tanh are 1-Lipschitz;
  * device against float64: 4 x the deviation of the float32 numpy evaluation from float64 on the same inputs, the factor
    tests/test_policy_rollout.py::test_actor_kernel_against_float64 uses for a second float32 evaluation order; for log_prob plus
    sum_j 4 * 2^-24 / (1 - a_j^2 + 1e-6), the float32 rounding of 1 - a^2 + 1e-6 carried through the logarithm.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import DeviceActor, StochasticActor, philox4x32_10, policy_noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTORS = os.path.join(ROOT, "tests", "golden", "actors")
ENVS = {"ori": "UR5OriReach-v1", "obs": "UR5ObsReach-v1", "sta": "UR5StaReach-v1", "dyn": "UR5DynReach-v1"}
KINDS = {"ori": _abi.ENV_ORI, "obs": _abi.ENV_OBS, "sta": _abi.ENV_STA, "dyn": _abi.ENV_DYN}
NEW_SYMBOLS = ("urgym_actor_set_log_std", "urgym_actor_sample", "urgym_rollout_sampled")
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
U24 = 2.0 ** -24


def weights(name):
    w = dict(np.load(os.path.join(ACTORS, f"actor_{name}.npz")))
    w.update(np.load(os.path.join(ACTORS, f"log_std_{name}.npz")))
    return w


def _f64(w, x, eps):
    """float64 closed form on float32 inputs.  Returns dict(mean_action, log_std, action, gauss = the Gaussian part of log_prob,
    log_prob) and `err`, bounds of what a float32 evaluation of the same quantities may deviate (see the module docstring)."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    x, eps = x.astype(np.float64), eps.astype(np.float64)

    def layer(W, b, v, ev):  # value, error bound of a float32 evaluation given the input's error bound ev
        K = W.shape[1] + 1
        mag = np.abs(v) @ np.abs(W).T + np.abs(b)
        return v @ W.T + b, ev @ np.abs(W).T + (K + 1) * U24 * (mag + ev @ np.abs(W).T)

    z, e = layer(w["latent_pi_0_weight"], w["latent_pi_0_bias"], x, np.zeros_like(x))
    h, e = np.maximum(z, 0.0), e
    z, e = layer(w["latent_pi_2_weight"], w["latent_pi_2_bias"], h, e)
    h = np.maximum(z, 0.0)
    mu, e_mu = layer(w["mu_weight"], w["mu_bias"], h, e)
    ls, e_ls = layer(w["log_std_weight"], w["log_std_bias"], h, e)
    ls = np.clip(ls, -20.0, 2.0)
    std = np.exp(ls)
    pre = mu + std * eps
    action = np.tanh(pre)
    gauss = (-0.5 * eps * eps - ls - HALF_LOG_2PI).sum(axis=1)
    log_prob = gauss - np.log(1.0 - action ** 2 + 1e-6).sum(axis=1)
    e_pre = e_mu + np.abs(eps) * std * (np.expm1(e_ls) + 4 * U24) + 4 * U24 * (np.abs(mu) + np.abs(std * eps))
    err = {"mean_action": e_mu + 4 * U24, "log_std": e_ls + 4 * U24 * np.abs(ls), "action": e_pre + 4 * U24,
           "gauss": e_ls.sum(axis=1) + 16 * U24 * (0.5 * eps * eps + np.abs(ls) + HALF_LOG_2PI).sum(axis=1)}
    return {"mu": mu, "mean_action": np.tanh(mu), "log_std": ls, "action": action, "gauss": gauss, "log_prob": log_prob}, err


def _ks(x, cdf):
    x = np.sort(np.asarray(x, dtype=np.float64).ravel())
    M, F, i = len(x), cdf(x), np.arange(len(x))
    return max(np.max(F - i / M), np.max((i + 1) / M - F)), M


# ------------------------------------------------------------------------------------------------ CPU
def test_sampling_structs_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    ctype = {"float": C.c_float, "int32_t": C.c_int32, "uint64_t": C.c_uint64}
    body = hdr[hdr.index("typedef struct urgym_sampling"):hdr.index("} urgym_sampling;")]
    fields = re.findall(r"^\s*(int32_t|uint64_t)\s+(\w+);", body, flags=re.M)
    assert [(n, ctype[t]) for t, n in fields] == list(_abi.Sampling._fields_) and len(fields) == 4
    body = hdr[hdr.index("typedef struct urgym_sample_records"):hdr.index("} urgym_sample_records;")]
    fields = re.findall(r"^\s*(float)\*\s*(\w+);", body, flags=re.M)
    assert [n for _, n in fields] == [f[0] for f in _abi.SampleRecords._fields_] == [n for n, _, _ in _abi.SAMPLE_RECORD_FIELDS]
    assert len(fields) == 4 and all(ct is C.c_float for _, ct, _ in _abi.SAMPLE_RECORD_FIELDS)
    modes = dict(re.findall(r"(URGYM_SAMPLE_\w+) = (\d)", hdr))
    assert modes == {"URGYM_SAMPLE_MEAN": "0", "URGYM_SAMPLE_GAUSSIAN": "1", "URGYM_SAMPLE_UNIFORM": "2"}
    assert (_abi.SAMPLE_MEAN, _abi.SAMPLE_GAUSSIAN, _abi.SAMPLE_UNIFORM) == (0, 1, 2)
    assert f"0x{_abi.NOISE_TAG:08X}" in hdr
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym), sym


def test_philox_known_answers_and_counter_layout():
    """Random123's kat_vectors for philox4x32-10 (counter / key all zero and all ones), then the counter of the policy noise."""
    z = philox4x32_10((0, 0), (0, 0, 0, 0))
    assert [int(v) for v in z] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    o = philox4x32_10((0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF,) * 4)
    assert [int(v) for v in o] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    seed, draw, env = 0x0123456789ABCDEF, (7 << 32) | 5, np.array([0, 3, 70000])
    a = philox4x32_10((0x89ABCDEF, 0x01234567), (env, 5, 7, _abi.NOISE_TAG | 0))
    b = philox4x32_10((0x89ABCDEF, 0x01234567), (env, 5, 7, _abi.NOISE_TAG | 1))
    words = np.stack([a[0], a[1], a[2], a[3], b[0], b[1]], axis=1)
    u = policy_noise(seed, draw, env, "uniform")
    assert u.dtype == np.float32 and u.shape == (3, 6)
    assert np.array_equal(u, ((words >> 8).astype(np.float64) * U24).astype(np.float32)) and u.min() >= 0.0 and u.max() < 1.0
    g = policy_noise(seed, draw, env, "gaussian", dtype=np.float64)
    u1, u2 = ((words[:, 0::2] >> 8) + 1.0) * U24, (words[:, 1::2] >> 8) * U24
    r = np.sqrt(-2.0 * np.log(u1))
    assert np.allclose(g[:, 0::2], r * np.cos(2 * np.pi * u2), atol=1e-12) and np.allclose(g[:, 1::2], r * np.sin(2 * np.pi * u2), atol=1e-12)
    assert not policy_noise(seed, draw, env, "mean").any()
    assert (_abi.NOISE_TAG | 1) > 4  # the reset sampler's counters end in a block number 0..4
    # a pure function of (seed, draw, env): no dependence on what else is asked for
    assert np.array_equal(policy_noise(seed, draw, 70000, "uniform"), u[2])
    assert not np.array_equal(policy_noise(seed + 1, draw, env, "uniform"), u)
    assert not np.array_equal(policy_noise(seed, draw + 1, env, "uniform"), u)


@pytest.mark.parametrize("seed", [1, 2])
def test_noise_statistics(seed):
    from scipy.special import ndtr

    env, draw = np.arange(4096)[None, :], np.arange(256)[:, None]  # 2^20 (draw, env) pairs x 6 components
    for mode, cdf in (("gaussian", ndtr), ("uniform", lambda v: v)):
        x = policy_noise(seed, draw, env, mode).astype(np.float64)
        d, M = _ks(x, cdf)
        print(f"seed {seed} {mode}: KS distance {d:.3e} (bound {1.95 / np.sqrt(M):.3e}, M = {M})")
        assert M >= 10 ** 6 and d <= 1.95 / np.sqrt(M)

        def corr(a, b, what):
            a, b = a.ravel(), b.ravel()
            c = abs(float(np.corrcoef(a, b)[0, 1]))
            assert len(a) >= 10 ** 6 and c <= 3.3 / np.sqrt(len(a)), (seed, mode, what, c, 3.3 / np.sqrt(len(a)))

        for i in range(6):
            for j in range(i + 1, 6):
                corr(x[..., i], x[..., j], ("components", i, j))
        corr(x[:, :-1], x[:, 1:], "neighbouring envs")
        corr(x[:-1], x[1:], "consecutive draws")


@pytest.mark.parametrize("name", ["ori", "obs", "sta", "dyn"])
def test_stochastic_actor_against_float64(name):
    import torch

    w = weights(name)
    assert DeviceActor.check_shapes(w, KINDS[name])[1] == 256
    n_in = w["latent_pi_0_weight"].shape[1]
    rng = np.random.default_rng(3)
    n = 4096
    x = rng.uniform(-1.0, 1.0, (n, n_in)).astype(np.float32)
    od, gd = _abi.OBS_DIMS[KINDS[name]]
    ach, des, obs = x[:, :gd], x[:, gd:2 * gd], x[:, 2 * gd:]
    eps = policy_noise(11, 4, np.arange(n), "gaussian")
    host = StochasticActor(w)
    action, log_prob = host(ach, des, obs, eps)
    mu, log_std = host.heads(ach, des, obs)
    ref, err = _f64(w, x, eps)
    assert action.dtype == np.float32 and log_prob.dtype == np.float32 and action.shape == (n, 6) and log_prob.shape == (n,)
    for key, got in (("action", action), ("mean_action", np.tanh(mu)), ("log_std", log_std)):
        dev = np.abs(got.astype(np.float64) - ref[key])
        print(f"{name} {key}: float32 vs float64 {dev.max():.3e}, largest bound {err[key].max():.3e}, "
              f"largest deviation / bound {float((dev / err[key]).max()):.3e}")
        assert np.all(dev <= err[key]), (name, key, float((dev - err[key]).max()))
    # log_prob: the Gaussian part by the bound; the squash part is compared where float32 computed it, from the float32 action
    gauss = StochasticActor.gaussian_log_prob(eps, log_std)
    assert np.all(np.abs(gauss.astype(np.float64) - ref["gauss"]) <= err["gauss"])
    a64 = action.astype(np.float64)
    terms = np.log(1.0 - a64 ** 2 + 1e-6)
    want = gauss.astype(np.float64) - terms.sum(axis=1)
    slack = (4 * U24 / (1.0 - a64 ** 2 + 1e-6)).sum(axis=1) + 16 * U24 * (np.abs(gauss) + np.abs(terms).sum(axis=1))
    assert np.all(np.abs(log_prob.astype(np.float64) - want) <= slack)
    # second opinion for the Gaussian term: torch.distributions.Normal in float64 on the CPU
    mu64, ls64 = (torch.from_numpy(np.asarray(v, dtype=np.float64)) for v in (ref["mu"], ref["log_std"]))
    pre = mu64 + ls64.exp() * torch.from_numpy(eps.astype(np.float64))
    second = torch.distributions.Normal(mu64, ls64.exp()).log_prob(pre).sum(dim=1).numpy()
    assert np.allclose(second, ref["gauss"], rtol=0, atol=1e-6)
    # eps = 0 is the deterministic actor
    a0, _ = host(ach, des, obs, np.zeros_like(eps))
    assert np.array_equal(a0, np.tanh(mu).astype(np.float32))


def test_log_std_shape_checks_need_no_gpu():
    w = weights("dyn")
    assert DeviceActor.check_shapes(w, _abi.ENV_DYN) == (47, 256)
    with pytest.raises(ValueError, match="both"):
        DeviceActor.check_shapes({k: v for k, v in w.items() if k != "log_std_bias"}, _abi.ENV_DYN)
    with pytest.raises(ValueError, match="log_std head"):
        DeviceActor.check_shapes(dict(w, log_std_weight=w["log_std_weight"][:, :128]), _abi.ENV_DYN)
    with pytest.raises(ValueError, match="log_std head"):
        DeviceActor.check_shapes(dict(w, log_std_bias=np.zeros(5, np.float32)), _abi.ENV_DYN)


# ------------------------------------------------------------------------------------------------ GPU
def _bits(t):
    import torch

    return t.contiguous().view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    import torch

    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _make(name, n, seed, **kw):
    from ur_gym_amd import make_vec

    env = make_vec(ENVS[name], num_envs=n, device="cuda:0", seed=seed, **kw)
    env.reset(seed=seed)
    return env, DeviceActor(weights(name), env)


def _same_state(env_a, env_b):
    for key in env_a.buf:
        if key in ("done_list", "done_count"):  # scratch of the reset path, not state
            continue
        assert _same_bits(env_a.buf[key], env_b.buf[key]), key


@pytest.mark.gpu
def test_noise_record_is_policy_noise():
    import torch

    seed, first, K = 0xC0FFEE1234, (1 << 32) - 1, 3  # the draws cross 2^32: draw_hi takes part
    got, bound = {}, None
    for n in (65536, 4097, 1):
        env, actor = _make("ori", n, 5)
        for mode in ("gaussian", "uniform"):
            rec = env.rollout_policy(actor, K, record=("noise",), sample=dict(mode=mode, seed=seed, first_draw=first))
            torch.cuda.synchronize()
            got[mode, n] = rec["noise"].cpu().numpy()
        actor.close()
        env.close()
        draws, envs = (first + np.arange(K, dtype=np.uint64))[:, None], np.arange(n)[None, :]
        assert np.array_equal(got["uniform", n], policy_noise(seed, draws, envs, "uniform")), n  # integer Philox + exact conversion
        f32, f64 = policy_noise(seed, draws, envs, "gaussian"), policy_noise(seed, draws, envs, "gaussian", dtype=np.float64)
        if bound is None:
            host_dev = float(np.abs(f32.astype(np.float64) - f64).max())
            bound = 4.0 * host_dev
        dev = float(np.abs(got["gaussian", n].astype(np.float64) - f64).max())
        print(f"noise N={n}: numpy float32 vs float64 {host_dev:.3e}, device vs float64 {dev:.3e}, bound {bound:.3e}")
        assert dev <= bound, (n, dev, bound)
    for mode in ("gaussian", "uniform"):  # the same (seed, draw, env) gives the same words at every N
        assert np.array_equal(got[mode, 65536][:, :4097], got[mode, 4097]) and np.array_equal(got[mode, 4097][:, :1], got[mode, 1])


def sampled_steps_against_float64(name, w, n, K, label=None, warm_steps=0):
    """The body of the step-by-step test (tests/test_actor_widths.py runs it at the other hidden widths, after `warm_steps` random
    steps): every recorded step of a GAUSSIAN rollout with the arrays `w` on its own (closed loops diverge): recorded observations
    and noise in, action / mean_action / log_std / log_prob out, against float64.  No row is excluded.  Returns, per quantity,
    [numpy float32 vs float64, device vs float64], and the records as numpy arrays."""
    import torch

    from ur_gym_amd import make_vec

    label = label or name
    env = make_vec(ENVS[name], num_envs=n, device="cuda:0", seed=23)
    env.reset(seed=23)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(5)
    for _ in range(warm_steps):  # leave the neutral pose
        env.step(torch.rand((n, 6), device="cuda:0", generator=g) * 2.0 - 1.0)
    actor = DeviceActor(w, env)
    host = StochasticActor(w)
    rec = env.rollout_policy(actor, K, record=("observation", "achieved_goal", "desired_goal", "action") + env.SAMPLE_RECORD_KEYS,
                             sample=dict(mode="gaussian", seed=99, first_draw=1000))
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in rec.items()}
    actor.close()
    env.close()
    worst = {k: [0.0, 0.0] for k in ("action", "mean_action", "log_std", "gauss")}
    rows = []
    for k in range(K):
        ach, des, obs, eps = r["achieved_goal"][k], r["desired_goal"][k], r["observation"][k], r["noise"][k]
        assert np.abs(r["action"][k]).max() <= 1.0
        n32, n64 = (policy_noise(99, 1000 + k, np.arange(n), "gaussian", dtype=t) for t in (np.float32, np.float64))
        assert np.abs(eps - n64).max() <= 4.0 * np.abs(n32 - n64).max(), k  # the draw schedule: pass k draws first_draw + k
        ref, _ = _f64(w, np.concatenate([ach, des, obs], axis=1), eps)
        h_action, _ = host(ach, des, obs, eps)
        h_mu, h_ls = host.heads(ach, des, obs)
        hostv = {"action": h_action, "mean_action": np.tanh(h_mu), "log_std": h_ls, "gauss": StochasticActor.gaussian_log_prob(eps, h_ls)}
        a64 = r["action"][k].astype(np.float64)
        squash = np.log(1.0 - a64 ** 2 + 1e-6).sum(axis=1)  # from the recorded float32 action
        devv = {"action": r["action"][k], "mean_action": r["mean_action"][k], "log_std": r["log_std"][k]}
        for key in ("action", "mean_action", "log_std", "gauss"):
            worst[key][0] = max(worst[key][0], float(np.abs(hostv[key].astype(np.float64) - ref[key]).max()))
            if key != "gauss":
                worst[key][1] = max(worst[key][1], float(np.abs(devv[key].astype(np.float64) - ref[key]).max()))
        rows.append((np.abs(r["log_prob"][k].astype(np.float64) - (ref["gauss"] - squash)), (4 * U24 / (1.0 - a64 ** 2 + 1e-6)).sum(axis=1)))
    for key in ("action", "mean_action", "log_std"):
        print(f"{label} {key}: numpy float32 vs float64 {worst[key][0]:.3e}, device vs float64 {worst[key][1]:.3e}, bound {4 * worst[key][0]:.3e}")
        assert worst[key][1] <= 4.0 * worst[key][0], (label, key, worst[key])
    dev = np.concatenate([d for d, _ in rows])
    bound = 4.0 * worst["gauss"][0] + np.concatenate([s for _, s in rows])
    print(f"{label} log_prob: Gaussian part numpy float32 vs float64 {worst['gauss'][0]:.3e}; device vs float64 worst {dev.max():.3e}, "
          f"worst excess over its row's bound {float((dev - bound).max()):.3e}, largest row bound {bound.max():.3e}")
    assert np.all(dev <= bound), (label, float((dev - bound).max()))
    return worst, r


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ori", "obs", "sta", "dyn"])
def test_sampled_actions_and_log_prob_step_by_step(name):
    sampled_steps_against_float64(name, weights(name), 2048, 12)


def mean_mode_is_bitwise_the_deterministic_path(name, n, K, w):
    """The body of the MEAN-mode test (tests/test_actor_widths.py runs it at the other hidden widths): with the arrays `w`, MEAN
    through the sampling instance, through the C ABI, and in a rollout with and without sample records is bitwise the deterministic
    path, records and final state included."""
    import torch

    from ur_gym_amd import make_vec

    def make():
        env = make_vec(ENVS[name], num_envs=n, device="cuda:0", seed=31)
        env.reset(seed=31)
        return env, DeviceActor(w, env)

    env_a, actor_a = make()
    env_b, actor_b = make()
    env_c, actor_c = make()
    a0 = env_a.policy_actions(actor_a)
    a1, lp = env_b.policy_actions(actor_b, sample=dict(mode="mean"))  # log_prob asked for: the sampling instance
    assert _same_bits(a0, a1) and lp.shape == (n,) and bool(torch.isfinite(lp).all())
    lib = _native.lib()
    how = _abi.Sampling(_abi.SAMPLE_MEAN, 0, 0, 0)
    a2 = torch.empty_like(a0)
    assert lib.urgym_actor_sample(env_b._h, actor_b._a, C.byref(how), C.c_void_p(a2.data_ptr()), None, env_b._stream()) == _abi.OK
    assert _same_bits(a0, a2)
    rec_a = env_a.rollout_policy(actor_a, K, record="all")
    rec_b = env_b.rollout_policy(actor_b, K, record=env_b.RECORD_KEYS, sample=dict(mode="mean"))
    rec_c = env_c.rollout_policy(actor_c, K, record="all", sample=dict(mode="mean", seed=5))
    torch.cuda.synchronize()
    assert set(rec_a) == set(rec_b) == set(env_a.RECORD_KEYS) and set(rec_c) == set(env_a.RECORD_KEYS + env_a.SAMPLE_RECORD_KEYS)
    for key in rec_a:
        assert _same_bits(rec_a[key], rec_b[key]) and _same_bits(rec_a[key], rec_c[key]), key
    _same_state(env_a, env_b)
    _same_state(env_a, env_c)
    assert not bool(rec_c["noise"].any()) and _same_bits(rec_c["mean_action"], rec_c["action"])
    if K > 100:
        assert bool(rec_a["truncated"].any())  # K passes the common truncation at step 100
    for actor, env in ((actor_a, env_a), (actor_b, env_b), (actor_c, env_c)):
        actor.close()
        env.close()


@pytest.mark.gpu
def test_mean_mode_is_bitwise_the_deterministic_path():
    import torch

    mean_mode_is_bitwise_the_deterministic_path("dyn", 3000, 110, weights("dyn"))
    # the clamp of log_std: a synthetic head driven past both ends
    w = weights("dyn")
    w["log_std_weight"] = np.zeros_like(w["log_std_weight"])
    w["log_std_bias"] = np.array([5.0, -30.0, 0.0, 2.5, -20.5, 1.0], np.float32)
    from ur_gym_amd import make_vec

    env = make_vec(ENVS["dyn"], num_envs=300, device="cuda:0", seed=1)
    env.reset(seed=1)
    actor = DeviceActor(w, env)
    rec = env.rollout_policy(actor, 2, record=("log_std",), sample=dict(mode="gaussian", seed=1))
    torch.cuda.synchronize()
    want = torch.tensor([2.0, -20.0, 0.0, 2.0, -20.0, 1.0], device="cuda:0").expand(2, 300, 6)
    assert torch.equal(rec["log_std"], want)
    actor.close()
    env.close()


@pytest.mark.gpu
def test_teacher_forced_replay_of_a_sampled_rollout_is_bitwise():
    from test_policy_rollout import replay_teacher_forced

    rec = replay_teacher_forced("dyn", 4096, 130, weights("dyn"), sample=dict(mode="gaussian", seed=7, first_draw=0))
    assert bool((rec["action"] != rec["mean_action"]).any())


@pytest.mark.gpu
def test_split_invariance_and_seed():
    import torch

    n, K = 2500, 9
    per_step = ("observation", "achieved_goal", "desired_goal", "action", "reward", "terminated", "truncated", "is_success", "collision")
    names = per_step + ("log_prob", "noise", "mean_action", "log_std")
    env_a, actor_a = _make("dyn", n, 41)
    env_b, actor_b = _make("dyn", n, 41)
    env_c, actor_c = _make("dyn", n, 41)
    one = env_a.rollout_policy(actor_a, K, record=names, sample=dict(mode="gaussian", seed=77, first_draw=20))
    first = env_b.rollout_policy(actor_b, (K + 1) // 2, record=names, sample=dict(mode="gaussian", seed=77, first_draw=20))
    second = env_b.rollout_policy(actor_b, K // 2, record=names, sample=dict(mode="gaussian", seed=77, first_draw=20 + (K + 1) // 2))
    other = env_c.rollout_policy(actor_c, K, record=("action",), sample=dict(mode="gaussian", seed=78, first_draw=20))
    torch.cuda.synchronize()
    for key in names:
        assert _same_bits(one[key], torch.cat([first[key], second[key]])), key
    _same_state(env_a, env_b)
    assert not _same_bits(one["action"], other["action"])
    for actor, env in ((actor_a, env_a), (actor_b, env_b), (actor_c, env_c)):
        actor.close()
        env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["mean", "gaussian", "uniform"])
def test_rollout_branches_are_bitwise_single_calls(mode):
    """What a rollout may leave out, each against the same steps made one call at a time (urgym_actor_sample, urgym_actor_forward for
    the actions of "mean", urgym_step): no steps at all, no trajectory and no records, sample records without a trajectory (for
    "mean" this is the sampling kernel, without them the deterministic one), a trajectory without its actions (they pass through the
    actor's scratch) and one with them.  65 envs: one more than a wave.  3 steps: a first, a middle and a closing pass.
    max_episode_steps = 2: every env is truncated and auto-reset at the second step, so the third acts on a reset observation."""
    import torch

    n, K = 65, 3
    sample = dict(mode=mode, seed=19, first_draw=(1 << 32) - 2)  # the draws cross 2^32
    ref, ref_actor = _make("dyn", n, 7, max_episode_steps=2)
    actions, log_prob, reward = [], [], []
    for k in range(K):
        a, lp = ref.policy_actions(ref_actor, sample=dict(sample, first_draw=sample["first_draw"] + k))
        if mode == "mean":
            a = ref.policy_actions(ref_actor)
        rew = ref.step(a)[1]
        actions.append(a.clone()), log_prob.append(lp.clone()), reward.append(rew.clone())
    actions, log_prob, reward = torch.stack(actions), torch.stack(log_prob), torch.stack(reward)
    assert int(ref.buf["episode_id"].min()) >= 1  # on the single-call side alone

    lib = _native.lib()
    made = [_make("dyn", n, 7, max_episode_steps=2) for _ in range(4)]
    (env_a, actor_a), (env_b, actor_b), (env_c, actor_c), (env_d, actor_d) = made
    how = env_a._sampling(sample)
    assert lib.urgym_rollout_sampled(env_a._h, actor_a._a, C.byref(how), 0, None, None, env_a._stream()) == _abi.OK  # launches nothing
    assert lib.urgym_rollout_sampled(env_a._h, actor_a._a, C.byref(how), K, None, None, env_a._stream()) == _abi.OK
    _same_state(env_a, ref)
    lp_b = torch.zeros((K, n), dtype=torch.float32, device="cuda:0")
    extra = _abi.SampleRecords(log_prob=C.cast(lp_b.data_ptr(), C.POINTER(C.c_float)))
    assert lib.urgym_rollout_sampled(env_b._h, actor_b._a, C.byref(how), K, None, C.byref(extra), env_b._stream()) == _abi.OK
    assert _same_bits(lp_b, log_prob)
    _same_state(env_b, ref)
    rec_c = env_c.rollout_policy(actor_c, K, record=("reward", "log_prob"), sample=sample)
    assert _same_bits(rec_c["reward"], reward) and _same_bits(rec_c["log_prob"], log_prob)
    _same_state(env_c, ref)
    rec_d = env_d.rollout_policy(actor_d, K, record=("action",), sample=sample)
    assert _same_bits(rec_d["action"], actions)
    _same_state(env_d, ref)
    for env, actor in made + [(ref, ref_actor)]:
        actor.close()
        env.close()


@pytest.mark.gpu
def test_warm_up_then_policy():
    """SAC's collection schedule: learning_starts = 100 uniform steps, then the policy."""
    import torch

    n, warm, K = 4096, 100, 20
    env, actor = _make("dyn", n, 3)
    names = ("action", "log_prob", "noise")
    u = env.rollout_policy(actor, warm, record=names, sample=dict(mode="uniform", seed=123, first_draw=0))
    g = env.rollout_policy(actor, K, record=names, sample=dict(mode="gaussian", seed=123, first_draw=warm))
    torch.cuda.synchronize()
    a, ag = u["action"].cpu().numpy().astype(np.float64), g["action"].cpu().numpy()
    assert a.min() >= -1.0 and a.max() <= 1.0 and ag.min() >= -1.0 and ag.max() <= 1.0
    assert np.array_equal(u["log_prob"].cpu().numpy(), np.full((warm, n), np.float32(-6.0 * np.log(2.0))))
    assert np.array_equal(u["action"].cpu().numpy(), 2.0 * u["noise"].cpu().numpy() - 1.0)
    assert bool(torch.isfinite(g["log_prob"]).all())
    M = warm * n
    mean, var = a.reshape(M, 6).mean(axis=0), a.reshape(M, 6).var(axis=0)
    se_mean, se_var = np.sqrt(1.0 / 3.0 / M), np.sqrt(4.0 / 45.0 / M)  # Var x = 1/3; Var x^2 = 1/5 - 1/9
    print("uniform actions: mean / se", mean / se_mean, "(var - 1/3) / se", (var - 1.0 / 3.0) / se_var)
    assert np.all(np.abs(mean) <= 3.3 * se_mean) and np.all(np.abs(var - 1.0 / 3.0) <= 3.3 * se_var)
    actor.close()
    env.close()


@pytest.mark.gpu
def test_sampling_refusals_leave_the_handle_usable():
    import torch

    from ur_gym_amd import make_vec

    lib = _native.lib()
    n = 300
    env = make_vec("UR5DynReach-v1", num_envs=n, device="cuda:0", seed=2)
    other = make_vec("UR5DynReach-v1", num_envs=n, device="cuda:0", seed=2)
    full = weights("dyn")
    actor = DeviceActor(full, env)
    bare = DeviceActor({k: v for k, v in full.items() if not k.startswith("log_std")}, env)
    foreign = DeviceActor(full, other)
    stream = env._stream()
    out = torch.empty((n, 6), device="cuda:0")
    lp = torch.empty((n,), device="cuda:0")
    act, lpp = C.c_void_p(out.data_ptr()), C.c_void_p(lp.data_ptr())
    gauss = _abi.Sampling(_abi.SAMPLE_GAUSSIAN, 0, 1, 0)

    def refused(rc, code, text):
        assert rc == code, (rc, text)
        assert text in lib.urgym_last_error(env._h), lib.urgym_last_error(env._h)

    # before reset: no observations to act on
    refused(lib.urgym_rollout_sampled(env._h, actor._a, C.byref(gauss), 3, None, None, stream), _abi.ERR_STATE, b"urgym_reset")
    refused(lib.urgym_actor_sample(env._h, actor._a, C.byref(gauss), act, lpp, stream), _abi.ERR_STATE, b"urgym_reset")
    env.reset(seed=2)
    other.reset(seed=2)
    for call in (lambda how: lib.urgym_actor_sample(env._h, actor._a, how, act, lpp, stream),
                 lambda how: lib.urgym_rollout_sampled(env._h, actor._a, how, 2, None, None, stream)):
        refused(call(None), _abi.ERR_ARG, b"null sampling")
        refused(call(C.byref(_abi.Sampling(7, 0, 1, 0))), _abi.ERR_ARG, b"unknown sampling mode")
        refused(call(C.byref(_abi.Sampling(-1, 0, 1, 0))), _abi.ERR_ARG, b"unknown sampling mode")
        refused(call(C.byref(_abi.Sampling(_abi.SAMPLE_GAUSSIAN, 1, 1, 0))), _abi.ERR_ARG, b"reserved0")
    # GAUSSIAN (and a density in MEAN mode) without a log_std head
    refused(lib.urgym_actor_sample(env._h, bare._a, C.byref(gauss), act, None, stream), _abi.ERR_ARG, b"log_std head")
    refused(lib.urgym_rollout_sampled(env._h, bare._a, C.byref(gauss), 2, None, None, stream), _abi.ERR_ARG, b"log_std head")
    mean = _abi.Sampling(_abi.SAMPLE_MEAN, 0, 0, 0)
    refused(lib.urgym_actor_sample(env._h, bare._a, C.byref(mean), act, lpp, stream), _abi.ERR_ARG, b"log_std head")
    assert lib.urgym_actor_sample(env._h, bare._a, C.byref(mean), act, None, stream) == _abi.OK
    assert lib.urgym_actor_sample(env._h, bare._a, C.byref(_abi.Sampling(_abi.SAMPLE_UNIFORM, 0, 1, 0)), act, lpp, stream) == _abi.OK
    with pytest.raises(_native.NativeError):
        env.rollout_policy(bare, 2, sample=dict(mode="gaussian"))
    with pytest.raises(ValueError):
        env.rollout_policy(actor, 2, sample=dict(mode="normal"))
    with pytest.raises(ValueError):
        env.rollout_policy(actor, 2, record=("log_prob",))  # a sample record without sample
    # an actor of another handle; null actions; negative K; a null head
    refused(lib.urgym_rollout_sampled(env._h, foreign._a, C.byref(gauss), 2, None, None, stream), _abi.ERR_ARG, b"not an actor of this handle")
    refused(lib.urgym_actor_sample(env._h, foreign._a, C.byref(gauss), act, lpp, stream), _abi.ERR_ARG, b"not an actor of this handle")
    refused(lib.urgym_actor_set_log_std(env._h, foreign._a, None, None), _abi.ERR_ARG, b"not an actor of this handle")
    refused(lib.urgym_actor_set_log_std(env._h, actor._a, None, None), _abi.ERR_ARG, b"null")
    refused(lib.urgym_actor_sample(env._h, actor._a, C.byref(gauss), None, lpp, stream), _abi.ERR_ARG, b"null actions")
    refused(lib.urgym_rollout_sampled(env._h, actor._a, C.byref(gauss), -1, None, None, stream), _abi.ERR_ARG, b"num_steps")
    # the handle still works: with and without records, null record structs, K = 0
    env.step(torch.zeros((n, 6), device="cuda:0"))
    assert lib.urgym_rollout_sampled(env._h, actor._a, C.byref(gauss), 2, None, None, stream) == _abi.OK
    assert lib.urgym_rollout_sampled(env._h, actor._a, C.byref(gauss), 2, C.byref(_abi.Trajectory()), C.byref(_abi.SampleRecords()), stream) == _abi.OK
    assert lib.urgym_rollout_sampled(env._h, actor._a, C.byref(gauss), 0, None, None, stream) == _abi.OK
    rec = env.rollout_policy(actor, 2, record=("episode_return", "log_prob"), sample=dict(mode="gaussian", seed=4))
    a, logp = env.policy_actions(actor, sample=dict(mode="gaussian", seed=4, first_draw=9))
    torch.cuda.synchronize()
    assert torch.isfinite(rec["episode_return"]).all() and torch.isfinite(rec["log_prob"]).all() and torch.isfinite(logp).all()
    assert float(a.abs().max()) <= 1.0
    # a destroyed actor is refused, not used
    gone = actor._a
    actor.close()
    refused(lib.urgym_rollout_sampled(env._h, gone, C.byref(gauss), 1, None, None, stream), _abi.ERR_ARG, b"not an actor of this handle")
    refused(lib.urgym_actor_sample(env._h, gone, C.byref(gauss), act, lpp, stream), _abi.ERR_ARG, b"not an actor of this handle")
    env.step(torch.zeros((n, 6), device="cuda:0"))
    torch.cuda.synchronize()
    bare.close()
    foreign.close()
    other.close()
    env.close()
