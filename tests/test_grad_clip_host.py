"""CPU tests (-m "not gpu") of gradient-norm clipping on the device.

  * tests/grad_clip_harness.cpp, a stand-alone host program around ur_gym_amd/csrc/urgym_grad_clip.h -- the functions the kernels
    compile -- equals evaluation.grad_norm bit for bit (tensor_sums, total, norm64, norm, scale) on the shared cases, and its scaled
    element equals evaluation.adam_step(scale=); built a second time with -fsanitize=address,undefined and run as that program.
  * evaluation.grad_norm against exact rational arithmetic: total within the float64 bound of a 1024-lane sum, norm64 against the
    correctly rounded square root of the float64 total.
  * scale is 1.0f exactly when max_norm >= norm64 + 1e-6 (but for the one rounding the docstring below names), and the non-finite
    cases the header states.
  * the ctypes mirrors of the two new structs against the header's text and the C compiler's own layout, the new symbols, the
    refusals that need no device, and the learner's option and its checkpoint rule on CPU tensors.
"""
import ctypes as C
import json
import math
import os
import re
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import grad_clip_cases as gc
from adam_cases import HYPER
from grad_clip_cases import CASES, same, same64
from test_checkpoint_host import assembled_learner, learner_state
from ur_gym_amd import _abi, _native, checkpoint
from ur_gym_amd.evaluation import ACTOR_ARRAYS, CRITIC_ARRAYS, LOG_STD_ARRAYS, adam_coefficients, adam_step, grad_norm
from ur_gym_amd.training import CLIP_DEFAULTS, HER_DEFAULTS, PER_DEFAULTS, SAC_DEFAULTS, SACLearner

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
NEW_SYMBOLS = ("urgym_actor_grad_norm", "urgym_critic_grad_norm", "urgym_actor_adam_step_scaled", "urgym_critic_adam_step_scaled", "urgym_sac_train_clipped")
GROUPS = [(which, kind, H) for kind, H in CASES for which in ("actor", "critic")]
DEVICE = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "grad_clip_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h")] + [os.path.join(CSRC, h) for h in ("urgym_grad_clip.h", "urgym_sac_terms.h", "urgym_adam.h", "urgym_pack_map.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("grad_clip_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("grad_clip_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


@pytest.fixture(scope="module")
def references():
    """evaluation.grad_norm of every shared group at a bound that does not clip and does not matter here: computed once."""
    return {key: grad_norm(gc.group(*key), 1.0) for key in GROUPS}


def run(exe, *args):
    got = subprocess.run([exe, *args], capture_output=True, text=True)
    assert got.returncode == 0 and not got.stderr, (args, got.returncode, got.stdout[-500:], got.stderr[-2000:])
    return got.stdout


def harness_norm(exe, tmp_path, tensors, max_norm):
    src, dst = str(tmp_path / "norm_in.bin"), str(tmp_path / "norm_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack(f"<if{len(tensors)}i", len(tensors), max_norm, *[g.size for g in tensors]))
        for g in tensors:
            f.write(np.ascontiguousarray(g, dtype=np.float32).tobytes())
    run(exe, "norm", src, dst)
    raw, k = open(dst, "rb").read(), len(tensors)
    assert len(raw) == 8 * (k + 2) + 8
    d = np.frombuffer(raw[:8 * (k + 2)], dtype=np.float64)
    f = np.frombuffer(raw[8 * (k + 2):], dtype=np.float32)
    return dict(tensor_sums=d[:k], total=d[k], norm64=d[k + 1], norm=f[0], scale=f[1])


def same_result(got, want):
    return (same64(got["tensor_sums"], want["tensor_sums"]) and same64(got["total"], want["total"]) and same64(got["norm64"], want["norm64"])
            and same(got["norm"], want["norm"]) and same(got["scale"], want["scale"]))


def bounds_for(want):
    """Three bounds per group, from the norm itself: one that leaves the gradients alone, two that clip."""
    n = float(want["norm64"])
    return (np.float32(2.0 * n), np.float32(0.5 * n), np.float32(1e-3 * n))


def compare_with_harness(exe, tmp_path, references, groups):
    for key in groups:
        tensors = gc.group(*key)
        for max_norm in bounds_for(references[key]):
            got, want = harness_norm(exe, tmp_path, tensors, float(max_norm)), grad_norm(tensors, max_norm)
            assert same_result(got, want), (key, max_norm, got, want)
            assert same64(want["tensor_sums"], references[key]["tensor_sums"])  # the bound does not reach the sums
        # the non-finite cases: NaN compares as NaN, the rest bitwise
        big = max(range(len(tensors)), key=lambda k: tensors[k].size)
        for value in (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)):
            bad = gc.with_element(tensors, big, tensors[big].size // 2, value)
            got, want = harness_norm(exe, tmp_path, bad, 1.0), grad_norm(bad, 1.0)
            if np.isnan(value):
                assert np.isnan(got["total"]) and np.isnan(got["norm64"]) and np.isnan(got["norm"]) and np.isnan(want["norm64"]), key
            else:
                assert same64(got["total"], want["total"]) and same64(got["norm64"], want["norm64"]) and same(got["norm"], want["norm"]), key
            assert same(got["scale"], want["scale"]), (key, value)


def test_shared_header_equals_grad_norm_bitwise(harness, tmp_path, references):
    compare_with_harness(harness, tmp_path, references, GROUPS)


def harness_step(exe, tmp_path, step, scale, p, g, m, v):
    src, dst = str(tmp_path / "step_in.bin"), str(tmp_path / "step_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<4dqqf", HYPER["lr"], HYPER["betas"][0], HYPER["betas"][1], HYPER["eps"], step, p.size, scale))
        for x in (p, g, m, v):
            f.write(np.ascontiguousarray(x, dtype=np.float32).tobytes())
    run(exe, "step", src, dst)
    out = np.fromfile(dst, dtype=np.float32)
    assert out.size == 3 * p.size
    return out[:p.size], out[p.size:2 * p.size], out[2 * p.size:]


def scaled_steps(exe, tmp_path, n):
    rng = np.random.default_rng(24)
    p, m, v = rng.standard_normal(n).astype(np.float32), (1e-3 * rng.standard_normal(n)).astype(np.float32), (1e-6 * rng.random(n)).astype(np.float32)
    g = np.concatenate([gc.group("actor", "ori", 32)[2].reshape(-1), gc.moderate_group("actor", "ori", 32)[2].reshape(-1)])[:n]
    g[:4] = (np.nan, np.inf, -np.inf, 0.0)
    for step, scale in ((1, np.float32(1.0)), (2, np.float32(0.37)), (3, np.float32(1e-30)), (1000, np.float32(0.0)), (5, np.float32(0.99999994))):
        coef = adam_coefficients(None, step=step, **HYPER)
        got = harness_step(exe, tmp_path, step, float(scale), p, g, m, v)
        want = adam_step(p, g, m, v, coef, scale=scale)
        for a, b in zip(got, want):
            both = np.isnan(a) & np.isnan(b)
            assert same(np.where(both, np.float32(0), a), np.where(both, np.float32(0), b)), (step, scale)
        if scale == np.float32(1.0):  # the scaled element at 1.0f is the unscaled one
            for a, b in zip(want, adam_step(p, g, m, v, coef)):
                both = np.isnan(a) & np.isnan(b)
                assert same(np.where(both, np.float32(0), a), np.where(both, np.float32(0), b))
        else:
            assert not same(want[1][4:], adam_step(p, g, m, v, coef)[1][4:])  # the first moment sees the coefficient
    # infinity times a zero coefficient is NaN; a finite element times it is a signed zero: m' = b1 * m exactly
    zero = adam_step(p, g, m, v, adam_coefficients(None, step=1, **HYPER), scale=np.float32(0.0))
    assert np.isnan(zero[1][1]) and np.isnan(zero[1][2]) and same(zero[1][4:], (adam_coefficients(None, step=1, **HYPER)[0] * m[4:]).astype(np.float32))


def test_scaled_element_equals_adam_step_with_scale(harness, tmp_path):
    scaled_steps(harness, tmp_path, 2048)


def test_harness_is_clean_under_address_and_undefined_sanitizers(sanitized_harness, tmp_path, references):
    compare_with_harness(sanitized_harness, tmp_path, references, [g for g in GROUPS if g[2] <= 64])
    scaled_steps(sanitized_harness, tmp_path, 1031)
    run(sanitized_harness, "layout")


@pytest.mark.parametrize("key", GROUPS, ids=lambda k: f"{k[0]}-{k[1]}-{k[2]}")
def test_grad_norm_against_exact_rational_arithmetic(key, references):
    """total against the exact sum of the exact squares.  A lane adds at most ceil(n / 1024) terms and the fold adds ten levels, so a
    tensor's sum carries at most m = ceil(n / 1024) - 1 + 10 roundings on any path; the K - 1 additions of the tensors' sums follow.
    Every term is >= 0, so the error is at most gamma(m + K - 1) x the exact total, gamma(k) = k u / (1 - k u), u = 2^-53 (Higham,
    Accuracy and Stability of Numerical Algorithms, section 4.2).  norm64 is the correctly rounded square root of the float64 total."""
    tensors, want = gc.group(*key), references[key]
    u = Fraction(1, 2 ** 53)
    exact_total = Fraction(0)
    for g, s in zip(tensors, want["tensor_sums"]):
        exact = sum((Fraction(float(x)) ** 2 for x in g.reshape(-1)), Fraction(0))
        k = -(-g.size // 1024) - 1 + 10
        assert abs(Fraction(float(s)) - exact) <= k * u / (1 - k * u) * exact, (key, g.shape)
        if not g.any():
            assert s == 0.0 and not np.signbit(s)
        exact_total += exact
    k = max(-(-g.size // 1024) for g in tensors) - 1 + 10 + len(tensors) - 1
    assert abs(Fraction(float(want["total"])) - exact_total) <= k * u / (1 - k * u) * exact_total, key
    assert float(want["norm64"]) == math.sqrt(float(want["total"]))  # math.sqrt is the C library's, correctly rounded
    # ... and that is within half an ulp of the real root of the float64 total: r^2 brackets it
    r, t = Fraction(float(want["norm64"])), Fraction(float(want["total"]))
    half = Fraction(math.ulp(float(want["norm64"]))) / 2
    assert (r - half) ** 2 <= t <= (r + half) ** 2
    assert same(want["norm"], np.float32(want["norm64"]))


def test_the_cases_can_tell_one_order_from_another(references):
    """On these values a float64 accumulation in plain element order is not THE ORDERED SUM in the last bits (in most groups: one
    that happened to agree would not make the definition wrong), and a float32 accumulation is nowhere near it."""
    plain = []
    for key in GROUPS:
        flat = np.concatenate([g.reshape(-1) for g in gc.group(*key)]).astype(np.float64)
        plain.append(float(np.cumsum(flat * flat)[-1]) != float(references[key]["total"]))
        with np.errstate(over="ignore"):
            flat32 = np.concatenate([g.reshape(-1) for g in gc.group(*key)])
            assert float(np.cumsum(flat32 * flat32, dtype=np.float32)[-1]) != float(references[key]["total"]), key
    assert sum(plain) > len(GROUPS) // 2, plain


@pytest.mark.parametrize("key", GROUPS, ids=lambda k: f"{k[0]}-{k[1]}-{k[2]}")
def test_scale_is_one_exactly_when_the_bound_is_not_reached(key, references):
    """scale == 1.0f exactly when max_norm >= norm64 + 1e-6.  The one exception the arithmetic has: c64 below 1 by less than 2^-25
    rounds to 1.0f, so a bound within 3e-8 (relative) under norm64 + 1e-6 gives 1.0f too; no bound below is that close."""
    tensors = gc.group(*key)
    n = float(references[key]["norm64"])
    for factor in (4.0, 1.5, 1.0 + 1e-6, 1.0 - 1e-6, 0.75, 0.01):
        max_norm = np.float32(factor * n)
        got = grad_norm(tensors, max_norm)
        assert (got["scale"] == np.float32(1.0)) == (float(max_norm) >= n + 1e-6), (key, factor)
        if got["scale"] != np.float32(1.0):
            assert same(got["scale"], np.float32(np.float64(max_norm) / (np.float64(n) + np.float64(1e-6)))) and 0.0 < got["scale"] < 1.0
    # all zeros: norm 0, and the bound is compared with 1e-6 alone
    zeros = [np.zeros_like(g) for g in tensors]
    assert grad_norm(zeros, 1.0)["norm64"] == 0.0 and grad_norm(zeros, 1.0)["scale"] == np.float32(1.0)
    assert same(grad_norm(zeros, 2.5e-7)["scale"], np.float32(0.25))


def test_non_finite_elements():
    tensors = gc.group("critic", "ori", 32)
    nan = grad_norm(gc.with_element(tensors, 2, 17, np.float32(np.nan)), 1.0)
    assert np.isnan(nan["norm64"]) and np.isnan(nan["norm"]) and same(nan["scale"], np.float32(1.0))  # the step is what it is without clipping
    for value in (np.inf, -np.inf):
        inf = grad_norm(gc.with_element(tensors, 8, 5, np.float32(value)), 1.0)
        assert inf["norm64"] == np.inf and inf["norm"] == np.float32(np.inf) and same(inf["scale"], np.float32(0.0))
    both = grad_norm(gc.with_element(gc.with_element(tensors, 8, 5, np.float32(np.inf)), 0, 0, np.float32(np.nan)), 1.0)
    assert same(both["scale"], np.float32(1.0))
    # finite float32 elements cannot overflow the float64 sum
    top = [np.full_like(g, np.finfo(np.float32).max) for g in tensors]
    assert np.isfinite(grad_norm(top, 1.0)["norm64"]) and grad_norm(top, 1.0)["norm"] == np.float32(np.inf)
    for bad in (0.0, -1.0, np.nan, np.inf, 1e39):
        with pytest.raises(ValueError, match="max_norm"):
            grad_norm(tensors, bad)


def test_groups_have_a_fixed_order():
    a, c = gc.group("actor", "dyn", 64), gc.group("critic", "dyn", 64)
    assert same64(grad_norm(gc.as_actor_dict(a), 1.0)["tensor_sums"], grad_norm(a, 1.0)["tensor_sums"])
    assert same64(grad_norm(gc.as_critic_dicts(c), 1.0)["tensor_sums"], grad_norm(c, 1.0)["tensor_sums"])
    assert grad_norm(a, 1.0)["tensor_sums"].shape == (_abi.GRAD_NORM_ACTOR_TENSORS,) and grad_norm(c, 1.0)["tensor_sums"].shape == (_abi.GRAD_NORM_CRITIC_TENSORS,)
    assert tuple(gc.ACTOR_KEYS) == tuple(ACTOR_ARRAYS + LOG_STD_ARRAYS) and tuple(gc.CRITIC_KEYS) == tuple(CRITIC_ARRAYS)
    with pytest.raises(ValueError, match="two networks"):
        grad_norm(gc.as_critic_dicts(c)[:1], 1.0)
    with pytest.raises(ValueError, match="float32"):
        grad_norm([g.astype(np.float64) for g in a], 1.0)


def test_structs_mirror_the_header(harness):
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    layout = json.loads(run(harness, "layout"))
    for name, mirror in (("urgym_grad_norm", _abi.GradNorm), ("urgym_sac_clipping", _abi.SacClipping)):
        body = hdr[hdr.index(f"typedef struct {name} {{"):hdr.index(f"}} {name};")]
        declared = re.findall(r"^\s*(?:const\s+)?\w+\*?\s+(\w+);", body, flags=re.M)
        assert declared == [f for f, _ in mirror._fields_], name  # the header's order is the mirror's
        want = layout[name]
        assert C.sizeof(mirror) == want.pop("sizeof"), name
        assert {f: getattr(mirror, f).offset for f, _ in mirror._fields_} == want, name  # the C compiler's own offsets
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    assert lib.urgym_abi_version() == 4
    # the header states the arithmetic, what is not written, and the sequence of the composed call
    for text in ("total  = ((s_0 + s_1) + s_2) + ...", "c64    = (double)max_norm / (norm64 + 1e-6)", "scale  = c64 < 1.0 ? (float)c64 : 1.0f",
                 "the gradient tensors are NOT written", "gs = g * scale", "SB3's SAC does NOT clip",
                 "urgym_critic_adam_step_scaled(online, target, critic_adam, hp, tau, scale + 0)", "urgym_actor_adam_step_scaled(actor, actor_adam, hp, scale + 1)",
                 "15 launches per update", "The temperature's scalar step is not clipped"):
        assert text in hdr, text
    clip = open(os.path.join(CSRC, "urgym_grad_clip.h")).read()
    assert "GRAD_NORM_EPS = 1e-6" in clip and _abi.GRAD_NORM_EPS == 1e-6 and "NOT written" in clip and "ordered_sum(" in clip


def test_refusals_that_need_no_device():
    lib = _native.lib()
    assert lib.urgym_actor_grad_norm(None, None, C.byref(_abi.ActorTensors()), C.byref(_abi.GradNorm()), None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert lib.urgym_critic_grad_norm(None, None, (_abi.QNetworkDev * 2)(), C.byref(_abi.GradNorm()), None) == _abi.ERR_ARG
    assert lib.urgym_actor_adam_step_scaled(None, None, C.byref(_abi.ActorAdam()), C.byref(_abi.AdamHyper()), None, None) == _abi.ERR_ARG
    assert lib.urgym_critic_adam_step_scaled(None, None, None, C.byref(_abi.CriticAdam()), C.byref(_abi.AdamHyper()), 1.0, None, None) == _abi.ERR_ARG
    assert lib.urgym_sac_train_clipped(None, C.byref(_abi.SacLearner()), C.byref(_abi.SacSchedule()), C.byref(_abi.SacClipping()), None, None, None, None, None,
                                       None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    p, g, m, v = (np.zeros(4, np.float32) for _ in range(4))
    coef = adam_coefficients(None, step=1, **HYPER)
    for bad in (np.float64(1.0), np.ones(2, np.float32), 1.0):
        with pytest.raises(ValueError, match="scale"):
            adam_step(p, g, m, v, coef, scale=bad)


def test_learner_option_and_the_checkpoint_rule_for_clipping():
    assert CLIP_DEFAULTS == dict(max_grad_norm=None)
    assert not set(CLIP_DEFAULTS) & (set(SAC_DEFAULTS) | set(PER_DEFAULTS) | set(HER_DEFAULTS))
    plain = assembled_learner()
    clipped = assembled_learner(**DEVICE, max_grad_norm=0.5)
    assert "max_grad_norm" not in plain._saved_hp() and "max_grad_norm" not in assembled_learner(max_grad_norm=None)._saved_hp()
    assert clipped._saved_hp()["max_grad_norm"] == 0.5
    # a clipped state round-trips through the checkpoint's own flattening, and a mismatch either way is refused
    state = dict(learner_state(clipped), hp=clipped._saved_hp())
    arrays, tree = checkpoint.flatten(state)
    back = checkpoint.unflatten(arrays, json.loads(json.dumps(tree)))
    assert back["hp"] == state["hp"]
    clipped.check_state_dict(back)
    plain_state = dict(learner_state(plain), hp=plain._saved_hp())
    plain.check_state_dict(plain_state)  # a file without the option holds no new key and loads
    with pytest.raises(ValueError, match="max_grad_norm is 0.5 in the checkpoint, None here"):
        assembled_learner(**DEVICE).check_state_dict(back)
    with pytest.raises(ValueError, match="max_grad_norm is None in the checkpoint, 0.5 here"):
        clipped.check_state_dict(dict(learner_state(clipped), hp={k: v for k, v in clipped._saved_hp().items() if k != "max_grad_norm"}))
    with pytest.raises(ValueError, match="max_grad_norm is 0.5 in the checkpoint, 2.0 here"):
        assembled_learner(**DEVICE, max_grad_norm=2.0).check_state_dict(back)
    with pytest.raises(ValueError, match="only"):
        clipped.check_state_dict(back, override=("max_grad_norm",))
    # the constructor's refusals, before it touches the environment
    with pytest.raises(ValueError, match="max_grad_norm needs device_entropy=True"):
        SACLearner(None, max_grad_norm=1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e39, True, "1"):
        with pytest.raises(ValueError, match="max_grad_norm must be"):
            SACLearner(None, **DEVICE, max_grad_norm=bad)
