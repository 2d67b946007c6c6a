"""Every instance of the actor kernel (ur_gym_amd/csrc/urgym_actor.hip): ``actor_kernel<HT, SAMPLE>`` for HT = 4, 8, 12, 16 tiles of
32 neurons, deterministic and sampling, each at its full hidden width and at a width that ``urgym_actor_create`` pads with zero
rows and columns, on all four env kinds (30 / 32 / 41 / 47 inputs) and on env counts with ragged ends.  The shipped checkpoints all
have width 256, so the other test files run HT = 8 only.  Everything goes through ``DeviceActor``, ``policy_actions`` and
``rollout_policy``; the one exception is the second ``urgym_actor_set_log_std`` on a live actor, which has no Python verb.

1. An exact-arithmetic network.  Inputs in {-1, 0, 1}, W0 / W1 dense +-1, b0 / b1 in {-1, 0, 1}, both heads dense +-2^-S, head biases
   multiples of 2^-S.  Every term of every sum is then an integer multiple of the layer's grid (1 in the hidden layers, 2^-S in the
   heads), and so is every partial sum in ANY order, fused or not; a partial sum is bounded by the sum of the terms' magnitudes.  If
   that bound, in units of the grid, stays below 2^24, every partial sum is a float32 number and float32 evaluation is exact.  The
   CPU test proves the bound from the construction (|x| through |W|) and sees numpy float32 reproduce float64 bit for bit.  On the
   device ``log_std`` = clamp(W_ls h + b_ls) must then equal float64 BITWISE on every row; ``mu`` is as exact, so the three
   tanh(mu) outputs are bitwise one another and differ from float64 tanh by ``tanhf``'s own error only.
   That error: the ROCm installation's documents give no figure for ``tanhf``, so the bound is the 5 ulp the OpenCL specification
   requires of single-precision tanh, counted in float32 ulps of the rounded float64 result.  A single misplaced weight of the mu
   head moves tanh(mu) by more than 100 x that bound on most rows (more than half, for every one of the 6 H weights; ReLU zeroes
   the weight's neuron on the others; CPU test), so the tolerance hides no misplacement.
2. Random float weights (He: variance GAIN^2 * 2 / fan_in; heads 1 / H) on real observations after 20 random steps, deterministic
   and GAUSSIAN, against float64 on the same float32 inputs.  The bound is the project's rule, no new number: 4 x the deviation of
   the float32 numpy actor from float64, measured in the test on the same inputs; per-row log_prob bound as in
   tests/test_policy_sampling.py.  Condition on the float64 reference alone: at most 10 % of its actions beyond 0.999, no layer-2
   neuron dead on all rows (``random_weights`` draws the rows of W1 that are, on these observations, again).
3. MEAN mode bitwise the deterministic path, and teacher-forced replay (deterministic and GAUSSIAN), at one width of each of
   HT = 4, 12, 16: the bodies of the tests in tests/test_policy_sampling.py / tests/test_policy_rollout.py.

Measured on MI355X (profiles/policy_rollout/gpu_tests_actor_widths.txt).
"""
import ctypes as C

import numpy as np
import pytest

from test_policy_rollout import _actor_f64, replay_teacher_forced
from test_policy_sampling import ENVS, KINDS, _f64, _same_bits, mean_mode_is_bitwise_the_deterministic_path, sampled_steps_against_float64
from ur_gym_amd import _abi
from ur_gym_amd.evaluation import DeterministicActor, DeviceActor, StochasticActor

WIDTHS = (32, 96, 128, 160, 256, 288, 384, 416, 512)  # HT 4: 32, 96, 128; HT 8: 160, 256; HT 12: 288, 384; HT 16: 416, 512
OTHER_KIND_WIDTHS = (96, 160, 384, 512)  # Ori / Obs / Sta: one width of each instance
CASES = [("dyn", H) for H in WIDTHS] + [(kind, H) for kind in ("ori", "obs", "sta") for H in OTHER_KIND_WIDTHS]
COUNTS = (1, 128, 417)  # one env; a full workgroup; 3 workgroups + a full wave + a wave with one live env + two dead waves
CROSS_PATH_WIDTHS = (96, 384, 416)  # HT 4, 12, 16 (tests/test_policy_sampling.py has HT 8)
S = 13  # the heads' grid is 2^-S
GRID = 2.0 ** -S
TANHF_ULPS = 5.0  # OpenCL C specification, relative error of single-precision tanh
GAIN = 1.0  # of W0 / W1 in part 2


def instance(H):
    return (H + 127) // 128 * 4


def features(kind):
    od, gd = _abi.OBS_DIMS[KINDS[kind]]
    return od + 2 * gd, od, gd


def exact_inputs(kind, n):
    rng = np.random.default_rng([n, features(kind)[0], 1])
    return rng.integers(-1, 2, (n, features(kind)[0])).astype(np.float32)


def exact_network(kind, H):
    """The network of part 1, and a second log_std head (other weights) for the clamp-edge and head-replacement checks; that head's
    bias depends on the inputs (``edge_bias``)."""
    n_in = features(kind)[0]
    rng = np.random.default_rng([H, n_in, 2])

    def sign(shape):
        return (rng.integers(0, 2, shape) * 2 - 1).astype(np.float32)

    # W1: every row has H / 2 + 0.45 sqrt(H) entries +1, at random places.  The layer-1 activations are all >= 0 with about one mean,
    # so a row's surplus of signs shifts its neuron on all rows at once; with independent signs the surplus has standard deviation
    # sqrt(H) and some neurons fire on 1 % of the rows, where a misplaced head weight would show on 1 % of the rows only.  A fixed
    # surplus of about half a standard deviation of the pre-activation lets every neuron fire on about 70 % of the rows.
    plus = H // 2 + int(np.ceil(0.45 * np.sqrt(H)))
    w1 = rng.permuted(np.where(np.arange(H) < plus, 1.0, -1.0)[None, :].repeat(H, axis=0), axis=1).astype(np.float32)
    w = {"latent_pi_0_weight": sign((H, n_in)), "latent_pi_0_bias": rng.integers(-1, 2, H).astype(np.float32),
         "latent_pi_2_weight": w1, "latent_pi_2_bias": rng.integers(-1, 2, H).astype(np.float32),
         "mu_weight": sign((6, H)) * np.float32(GRID), "mu_bias": (rng.integers(-1024, 1025, 6) * GRID).astype(np.float32),
         "log_std_weight": sign((6, H)) * np.float32(GRID), "log_std_bias": (-1.0 + rng.integers(-1024, 1025, 6) * GRID).astype(np.float32)}
    return w, sign((6, H)) * np.float32(GRID)


def hidden_f64(w, x):
    h = np.maximum(x.astype(np.float64) @ np.float64(w["latent_pi_0_weight"]).T + np.float64(w["latent_pi_0_bias"]), 0.0)
    return np.maximum(h @ np.float64(w["latent_pi_2_weight"]).T + np.float64(w["latent_pi_2_bias"]), 0.0)


def edge_bias(w, w_ls2, x):
    """Biases (multiples of 2^-S) that put W_ls2 h + b exactly on the clamp's edges on some rows and beyond them on others: column 0
    meets 2 on the row of its median and passes it on the rows above, column 1 the same at -20, columns 2 / 3 at the lower and upper
    quartile, column 4 lies beyond 2 and column 5 beyond -20 on every row."""
    lin = hidden_f64(w, x) @ np.float64(w_ls2).T
    at = [np.sort(lin[:, o])[int(q * (len(lin) - 1))] for o, q in ((0, 0.5), (1, 0.5), (2, 0.25), (3, 0.75))]
    b = np.array([2.0 - at[0], -20.0 - at[1], 2.0 - at[2], -20.0 - at[3], 2.0 - lin[:, 4].min() + GRID, -20.0 - lin[:, 5].max() - GRID])
    assert np.array_equal(b, np.round(b / GRID) * GRID)
    return b.astype(np.float32)


def magnitude_bounds(w, x):
    """Sum of the terms' magnitudes, in units of the layer's grid: what no partial sum of the layer can exceed, in any order."""
    a = {k: np.abs(np.float64(v)) for k, v in w.items()}
    m1 = np.abs(x.astype(np.float64)) @ a["latent_pi_0_weight"].T + a["latent_pi_0_bias"]
    m2 = m1 @ a["latent_pi_2_weight"].T + a["latent_pi_2_bias"]
    heads = [(m2 @ a[f"{h}_weight"].T + a[f"{h}_bias"]) / GRID for h in ("mu", "log_std")]
    return float(m1.max()), float(m2.max()), float(max(h.max() for h in heads))


def ulps_from_f64(got32, ref64):
    """|got - ref| in float32 ulps of the float64 result rounded to float32."""
    return np.abs(got32.astype(np.float64) - ref64) / np.spacing(np.abs(ref64.astype(np.float32))).astype(np.float64)


def random_weights(kind, H, gain=GAIN, alive_on=None):
    """He weights, heads of variance 1 / H, small biases, b_log_std near -1; a fixed seed per (width, inputs).  With `alive_on`
    (sets of float32 inputs [rows, in]) the draw is conditioned on part 2's requirement that every layer-2 neuron fires on at least
    one row of each set: real observations share a large common part, so on them an unconditioned draw leaves about 1 % of the layer-2 neurons
    below zero on every row (5 of 256 on 2049 Dyn observations of the CPU oracle), and what their head weights do would go
    unseen.  Such a neuron's row of W1 and its bias are drawn again from the same distributions, in float64 on the reference alone."""
    n_in = features(kind)[0]
    rng = np.random.default_rng([H, n_in, 3])
    f = np.float32
    w = {"latent_pi_0_weight": f(rng.normal(0.0, gain * np.sqrt(2.0 / n_in), (H, n_in))), "latent_pi_0_bias": f(rng.normal(0.0, 0.05, H)),
         "latent_pi_2_weight": f(rng.normal(0.0, gain * np.sqrt(2.0 / H), (H, H))), "latent_pi_2_bias": f(rng.normal(0.0, 0.05, H)),
         "mu_weight": f(rng.normal(0.0, np.sqrt(1.0 / H), (6, H))), "mu_bias": f(rng.normal(0.0, 0.05, 6)),
         "log_std_weight": f(rng.normal(0.0, np.sqrt(1.0 / H), (6, H))), "log_std_bias": f(-1.0 + rng.normal(0.0, 0.05, 6))}
    for _ in range(64 if alive_on is not None else 0):
        dead = np.flatnonzero(np.any([(hidden_f64(w, x) <= 0.0).all(axis=0) for x in alive_on], axis=0))
        if not len(dead):
            break
        w["latent_pi_2_weight"][dead] = f(rng.normal(0.0, gain * np.sqrt(2.0 / H), (len(dead), H)))
        w["latent_pi_2_bias"][dead] = f(rng.normal(0.0, 0.05, len(dead)))
    return w


def reference_condition(w, x, actions64, label):
    """The condition of part 2 on the float64 reference alone.  Returns the saturated share."""
    saturated = float((np.abs(actions64) > 0.999).mean())
    dead = int((hidden_f64(w, x) <= 0.0).all(axis=0).sum())
    assert saturated <= 0.10, (label, saturated)
    assert dead == 0, (label, dead)
    return saturated


# ------------------------------------------------------------------------------------------------ CPU
def test_cases_reach_every_instance():
    assert {instance(H) for H in WIDTHS} == {instance(H) for H in OTHER_KIND_WIDTHS} == {4, 8, 12, 16}
    assert {instance(H) for H in CROSS_PATH_WIDTHS} == {4, 12, 16}
    for ht in (4, 8, 12, 16):  # at its full width and at a padded one; the smallest legal width
        assert 32 * ht in WIDTHS and any(instance(H) == ht and H % 128 for H in WIDTHS)
    assert min(WIDTHS) == 32 and [features(k)[0] for k in ("ori", "obs", "sta", "dyn")] == [30, 32, 41, 47]
    for kind, H in CASES:
        assert DeviceActor.check_shapes(exact_network(kind, H)[0], KINDS[kind]) == (features(kind)[0], H)
        assert DeviceActor.check_shapes(random_weights(kind, H), KINDS[kind]) == (features(kind)[0], H)


@pytest.mark.parametrize("kind,H", CASES, ids=[f"{k}-{H}" for k, H in CASES])
def test_exact_network_is_exact_in_float32(kind, H):
    w, w_ls2 = exact_network(kind, H)
    n_in, od, gd = features(kind)
    for k in ("latent_pi_0_weight", "latent_pi_2_weight"):
        assert np.all(np.abs(w[k]) == 1.0)  # dense: every (neuron, k) slot of the packing carries information
    for k in ("mu_weight", "log_std_weight"):
        assert np.all(np.abs(w[k]) == np.float32(GRID)) and np.all(np.abs(w_ls2) == np.float32(GRID))
    host = StochasticActor(w)
    for n in COUNTS + (2048,):
        x = exact_inputs(kind, n)
        assert set(np.unique(x)) <= {-1.0, 0.0, 1.0}
        edge = dict(w, log_std_weight=w_ls2, log_std_bias=edge_bias(w, w_ls2, x))
        for net in (w, edge):
            m1, m2, m3 = magnitude_bounds(net, x)
            assert max(m1, m2, m3) < 2.0 ** 24, (kind, H, n, m1, m2, m3)
            ref, _ = _f64(net, x, np.zeros((n, 6), np.float32))
            mu32, ls32 = StochasticActor(net).heads(x[:, :gd], x[:, gd:2 * gd], x[:, 2 * gd:])
            assert mu32.dtype == np.float32 and np.array_equal(mu32.astype(np.float64), ref["mu"])
            assert ls32.dtype == np.float32 and np.array_equal(ls32.astype(np.float64), ref["log_std"])
            # another float32 summation order: the neurons of both hidden layers backwards
            back = {k: v[::-1] if k.startswith("latent") else v[..., ::-1] for k, v in net.items() if k.endswith("weight")}
            back["latent_pi_2_weight"] = back["latent_pi_2_weight"][:, ::-1]
            back.update({k: v[::-1] if k.startswith("latent") else v for k, v in net.items() if k.endswith("bias")})
            mu_b, ls_b = StochasticActor({k: np.ascontiguousarray(v) for k, v in back.items()}).heads(x[:, :gd], x[:, gd:2 * gd], x[:, 2 * gd:])
            assert np.array_equal(mu_b, mu32) and np.array_equal(ls_b, ls32)
        ref, _ = _f64(w, x, np.zeros((n, 6), np.float32))
        lin = hidden_f64(w, x) @ np.float64(w["log_std_weight"]).T + np.float64(w["log_std_bias"])
        assert -20.0 < lin.min() and lin.max() < 2.0 and np.array_equal(lin, ref["log_std"])  # the clamp does not take part
        assert np.abs(ref["mean_action"]).max() <= 0.999 and np.all(ref["log_std"] != 0.0)  # (a stale zeroed record would differ)
        ls = _f64(edge, x, np.zeros((n, 6), np.float32))[0]["log_std"]
        lin = hidden_f64(w, x) @ np.float64(w_ls2).T + np.float64(edge["log_std_bias"])
        assert (lin[:, 0] == 2.0).any() and (lin[:, 1] == -20.0).any() and (lin[:, 2] == 2.0).any() and (lin[:, 3] == -20.0).any()
        assert (lin[:, 4] > 2.0).all() and (lin[:, 5] < -20.0).all() and ls.min() == -20.0 and ls.max() == 2.0
        if n >= 128:
            for o in range(4):
                edge_value = (2.0, -20.0)[o & 1]
                assert (lin[:, o] > edge_value).any() and (lin[:, o] < edge_value).any(), (n, o)
    # sensitivity (n = 2048 rows): flipping the sign of the one weight (o, j) moves mu[:, o] by -2 w[o, j] h[:, j]
    h = hidden_f64(w, x)
    tol = TANHF_ULPS * np.spacing(np.abs(ref["mean_action"].astype(np.float32))).astype(np.float64)  # [n, 6]
    share = np.empty((6, H))
    for o in range(6):
        moved = np.abs(np.tanh(ref["mu"][:, o, None] - 2.0 * np.float64(w["mu_weight"])[o] * h) - ref["mean_action"][:, o, None])
        share[o] = (moved > 100.0 * tol[:, o, None]).mean(axis=0)
    print(f"{kind} H={H}: magnitude bounds {m1:.0f} / {m2:.0f} / {m3:.4g} of {2.0 ** 24:.4g}; a flipped mu weight moves tanh(mu) by > "
          f"{100 * TANHF_ULPS:.0f} ulp on {share.min():.3f} .. {share.max():.3f} of the rows")
    assert share.min() > 0.5, (kind, H, float(share.min()))


# ------------------------------------------------------------------------------------------------ GPU
def _env(kind, n, seed=1):
    from ur_gym_amd import make_vec

    env = make_vec(ENVS[kind], num_envs=n, device="cuda:0", seed=seed)
    env.reset(seed=seed)
    return env


def _write_inputs(env, x):
    """The actor reads the bound observation tensors, which env.buf owns."""
    import torch

    gd = env.goal_dim
    for key, part in (("achieved_goal", x[:, :gd]), ("desired_goal", x[:, gd:2 * gd]), ("observation", x[:, 2 * gd:])):
        assert env.buf[key].shape == part.shape and env.buf[key].dtype == torch.float32
        env.buf[key].copy_(torch.from_numpy(np.ascontiguousarray(part)))


def _nan_out(n):
    import torch

    return torch.full((n, 6), float("nan"), dtype=torch.float32, device="cuda:0")


def _same_array_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,H", CASES, ids=[f"{k}-{H}" for k, H in CASES])
def test_exact_network_on_the_device(kind, H):
    """Both instances of the width's HT.  The records of rollout_policy are allocated (zeroed) inside the call, so NaN cannot be
    put there first; a launch that did not happen would leave zeros, which the bitwise comparison refuses (the reference log_std is
    nowhere 0: CPU test).  The tensors policy_actions fills are pre-filled with NaN."""
    import torch

    from ur_gym_amd import _native

    w, w_ls2 = exact_network(kind, H)
    records = ("action", "mean_action", "log_std", "noise")
    worst = 0.0
    for n in COUNTS:
        x = exact_inputs(kind, n)
        ref, _ = _f64(w, x, np.zeros((n, 6), np.float32))
        env = _env(kind, n)
        actor = DeviceActor(w, env)
        _write_inputs(env, x)
        det = env.policy_actions(actor, out=_nan_out(n))  # actor_kernel<HT, false>
        smp, lp = env.policy_actions(actor, out=_nan_out(n), sample=dict(mode="mean"))  # actor_kernel<HT, true>
        rec = env.rollout_policy(actor, 1, record=records, sample=dict(mode="mean"))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(det).all()) and bool(torch.isfinite(smp).all()) and bool(torch.isfinite(lp).all())
        got = {k: v.cpu().numpy() for k, v in rec.items()}
        assert all(got[k].shape == (1, n, 6) and np.isfinite(got[k]).all() for k in records) and not got["noise"].any()
        assert _same_array_bits(got["log_std"][0], ref["log_std"].astype(np.float32)), (kind, H, n)  # no tolerance, every row
        assert _same_bits(det, smp) and _same_bits(det, rec["action"][0]) and _same_bits(det, rec["mean_action"][0]), (kind, H, n)
        ulps = ulps_from_f64(det.cpu().numpy(), ref["mean_action"])
        worst = max(worst, float(ulps.max()))
        assert ulps.max() <= TANHF_ULPS, (kind, H, n, float(ulps.max()))
        # a second head on the same actor: other weights, biases on the clamp's edges.  The step above overwrote the inputs.
        b_ls2 = edge_bias(w, w_ls2, x)
        edge, _ = _f64(dict(w, log_std_weight=w_ls2, log_std_bias=b_ls2), x, np.zeros((n, 6), np.float32))
        head = [np.ascontiguousarray(a, dtype=np.float32) for a in (w_ls2, b_ls2)]
        _native.check(env.lib.urgym_actor_set_log_std(env._h, actor._a, *[a.ctypes.data_as(C.POINTER(C.c_float)) for a in head]), env._h)
        _write_inputs(env, x)
        rec = env.rollout_policy(actor, 1, record=records, sample=dict(mode="mean"))
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in rec.items()}
        assert _same_array_bits(got["log_std"][0], edge["log_std"].astype(np.float32)), (kind, H, n)
        assert (got["log_std"] == 2.0).any() and (got["log_std"] == -20.0).any() and got["log_std"].min() == -20.0 and got["log_std"].max() == 2.0
        assert _same_bits(det, rec["action"][0]) and _same_bits(det, rec["mean_action"][0]), (kind, H, n)  # mu is the first call's
        actor.close()
        env.close()
    print(f"exact {kind} H={H} HT={instance(H)} (deterministic and sampling instance, N = {COUNTS}): log_std bitwise float64, "
          f"tanh(mu) worst {worst:.2f} ulp from float64 (bound {TANHF_ULPS:.0f})")


def _warm(kind, n, seed):
    """An env after reset and 20 random steps (it has left the neutral pose), and the float32 inputs the actor will read."""
    import torch

    env = _env(kind, n, seed=seed)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(5)
    for _ in range(20):
        env.step(torch.rand((n, 6), device="cuda:0", generator=g) * 2.0 - 1.0)
    return env, np.concatenate([env.buf[k].cpu().numpy() for k in ("achieved_goal", "desired_goal", "observation")], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("H", WIDTHS)
def test_random_weights_against_float64(H):
    kind, n, n_smp, K = "dyn", 4097, 2049, 4
    label = f"float H={H} HT={instance(H)}"
    env, x = _warm(kind, n, 21)
    other, x_smp = _warm(kind, n_smp, 23)  # where sampled_steps_against_float64 starts
    other.close()
    w = random_weights(kind, H, alive_on=(x, x_smp))
    host = DeterministicActor(w)
    actor = DeviceActor(w, env)
    got = env.policy_actions(actor, out=_nan_out(n)).cpu().numpy()  # actor_kernel<HT, false>
    actor.close()
    env.close()
    gd = features(kind)[2]
    ref = _actor_f64(w, x)
    saturated = reference_condition(w, x, ref, label)
    dev_numpy = float(np.abs(host(x[:, :gd], x[:, gd:2 * gd], x[:, 2 * gd:]).astype(np.float64) - ref).max())
    dev_kernel = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{label} deterministic N={n}: numpy float32 vs float64 {dev_numpy:.3e}, kernel vs float64 {dev_kernel:.3e}, "
          f"bound {4.0 * dev_numpy:.3e}, saturated {saturated:.4f}")
    assert got.shape == (n, 6) and got.dtype == np.float32 and np.isfinite(got).all()
    assert dev_kernel <= 4.0 * dev_numpy, (label, dev_kernel, 4.0 * dev_numpy)
    # GAUSSIAN, every recorded step on its own: actor_kernel<HT, true>
    worst, r = sampled_steps_against_float64(kind, w, n_smp, K, label=label + " gaussian", warm_steps=20)
    xs = np.concatenate([np.concatenate([r[k][s] for k in ("achieved_goal", "desired_goal", "observation")], axis=1) for s in range(K)])
    assert np.array_equal(xs[:n_smp], x_smp)
    saturated = reference_condition(w, xs, _f64(w, xs, np.concatenate(list(r["noise"])))[0]["action"], label)
    print(f"{label} gaussian N={n_smp} K={K}: saturated {saturated:.4f}")


@pytest.mark.gpu
@pytest.mark.parametrize("H", CROSS_PATH_WIDTHS)
def test_cross_path_identities(H):
    w = random_weights("dyn", H)
    mean_mode_is_bitwise_the_deterministic_path("dyn", 1000, 12, w)
    replay_teacher_forced("dyn", 1000, 12, w, min_finished=-1)
    rec = replay_teacher_forced("dyn", 1000, 12, w, sample=dict(mode="gaussian", seed=7, first_draw=0), min_finished=-1)
    assert bool((rec["action"] != rec["mean_action"]).any())
