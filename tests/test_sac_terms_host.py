"""CPU tests (-m "not gpu") of SAC's entropy coefficient on the device.

  * tests/sac_terms_harness.cpp, a stand-alone host program: the per-row arithmetic, the ordered sum (as a host loop in the stated
    order) and the scalar tails of urgym_sac_terms.h, the functions the kernels compile, equal evaluation.entropy_step and
    evaluation.policy_terms bit for bit at every count of sac_terms_cases.COUNTS, the four float64 sums included; a plain ascending
    float64 sum of the same terms gives other bits at one count or more, so the order is being tested.  Built a second time with
    -fsanitize=address,undefined and run as that program.
  * the ctypes mirrors of the new structs, the new symbols, and the refusals that need no device.
  * five carried steps of evaluation.entropy_step against SAC's temperature update in float64 (float64 Adam on log_ent_coef), within
    adam_cases.p_bound.
"""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from sac_terms_cases import COUNTS, GAMMA, HYPER, TARGET_ENTROPY, inputs, p_bound, plain_ascending_sum, same
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import adam_coefficients, entropy_step, ordered_sum, policy_terms

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
NEW_SYMBOLS = ("urgym_sac_entropy_step", "urgym_sac_policy_terms")


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "sac_terms_harness.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("urgym_sac_terms.h", "urgym_adam.h", "urgym_pack_map.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("sac_terms_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("sac_terms_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run_harness(exe, tmp_path, step, alpha, scale_log_prob, scale_action, x):
    n = x["log_prob"].size
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<4dqq", HYPER["lr"], HYPER["betas"][0], HYPER["betas"][1], HYPER["eps"], step, n))
        f.write(np.array([alpha, TARGET_ENTROPY, GAMMA, scale_log_prob, scale_action, x["l"], x["m"], x["v"]], dtype=np.float32).tobytes())
        f.write(np.ascontiguousarray(x["terminated"], dtype=np.uint8).tobytes())
        for k in ("log_prob", "target", "next_log_prob", "dqmin_da", "q", "y", "q_min"):
            f.write(np.ascontiguousarray(x[k], dtype=np.float32).tobytes())
    run = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (run.stdout, run.stderr[-2000:])
    raw = open(dst, "rb").read()
    sums, rest = np.frombuffer(raw[:32], dtype=np.float64), np.frombuffer(raw[32:], dtype=np.float32)
    assert rest.size == 7 + 8 * n
    names = ("l", "m", "v", "loss", "mean", "critic_loss", "actor_loss")
    out = dict(zip(names, rest[:7]))
    out.update(sums=sums, y=rest[7:7 + n], d_log_prob=rest[7 + n:7 + 2 * n], d_action=rest[7 + 2 * n:].reshape(n, 6))
    return out


def same64(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).reshape(-1).view(np.uint64), np.asarray(b, dtype=np.float64).reshape(-1).view(np.uint64))


def compare_all_counts(exe, tmp_path, counts):
    """Returns the counts at which a plain ascending float64 sum of the entropy step's terms has other bits than the ordered sum."""
    order_matters = []
    for i, count in enumerate(counts):
        x = inputs(count)
        step = 1 + i
        alpha = np.float32(np.exp(x["l"]))  # an input of both sides: whose exp it is does not matter here
        scale_e, scale_p = 1.0 / count, -1.0 / count
        got = run_harness(exe, tmp_path, step, alpha, scale_e, scale_p, x)
        coef = adam_coefficients(None, step=step, **HYPER)
        e = entropy_step(alpha, x["log_prob"], TARGET_ENTROPY, x["l"], x["m"], x["v"], coef, target=x["target"], next_log_prob=x["next_log_prob"],
                         terminated=x["terminated"], gamma=GAMMA, scale=scale_e)
        p = policy_terms(alpha, dqmin_da=x["dqmin_da"], scale=scale_p, q=x["q"], y=x["y"], log_prob=x["log_prob"], q_min=x["q_min"])
        for k in ("l", "m", "v", "loss", "mean", "y", "d_log_prob"):
            assert same(got[k], np.asarray(e[k]).reshape(np.shape(got[k]))), (count, k, got[k], e[k])
        assert same(got["d_action"], p["d_action"]) and same(got["critic_loss"], p["critic_loss"]) and same(got["actor_loss"], p["actor_loss"]), count
        terms = [x["log_prob"] + np.float32(TARGET_ENTROPY), p["critic_terms"][0], p["critic_terms"][1], p["actor_terms"]]
        want = [ordered_sum(t) for t in terms]
        assert same64(got["sums"], want), (count, got["sums"], want)
        assert np.isfinite(got["sums"]).all() and np.isfinite([got[k] for k in ("l", "m", "v", "loss")]).all()
        if any(not same64(plain_ascending_sum(t), w) for t, w in zip(terms, want)):
            order_matters.append(count)
    return order_matters


def test_shared_arithmetic_and_ordered_sum_equal_the_restatements_bitwise(harness, tmp_path):
    order_matters = compare_all_counts(harness, tmp_path, COUNTS)
    print("a plain ascending float64 sum differs from the ordered sum at counts", order_matters)
    assert order_matters, "the inputs do not tell the ordered sum from a plain ascending one: the order is not being tested"


def test_harness_is_clean_under_address_and_undefined_sanitizers(sanitized_harness, tmp_path):
    compare_all_counts(sanitized_harness, tmp_path, COUNTS)


def test_ordered_sum_is_the_stated_order():
    # integers sum exactly in any order
    assert ordered_sum(np.arange(5000, dtype=np.float32)) == 5000 * 4999 / 2
    # 2^53 in lane 0, ones everywhere else, two rows: lane 0 holds 2^53 + 1 = 2^53 (a tie, rounded to even), every other lane 2.0, and
    # the fold adds 2, 4, ..., 1024 to it, all exact; added one at a time behind 2^53, every 1.0 is lost
    t = np.ones(2048, np.float32)
    t[0] = 2.0 ** 53
    assert ordered_sum(t) == 2.0 ** 53 + 2046.0 and plain_ascending_sum(t) == 2.0 ** 53
    assert ordered_sum(np.zeros(1, np.float32)) == 0 and not np.signbit(ordered_sum(np.full(3, -0.0, np.float32)))  # lanes start at +0.0
    with pytest.raises(ValueError):
        ordered_sum(np.zeros(4, np.float64))
    with pytest.raises(ValueError):
        ordered_sum(np.zeros((2, 2), np.float32))


def test_structs_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    ctype = {"int32_t": C.c_int32, "float": C.c_float, "const float*": C.POINTER(C.c_float), "float*": C.POINTER(C.c_float),
             "const uint8_t*": C.POINTER(C.c_uint8)}

    def fields(struct_name):
        body = hdr[hdr.index(f"typedef struct {struct_name} {{"):hdr.index(f"}} {struct_name};")]
        return re.findall(r"^\s*(int32_t|float|const float\*|float\*|const uint8_t\*)\s+(\w+);", body, flags=re.M)

    for name, mirror, n in (("urgym_sac_entropy_args", _abi.SacEntropyArgs, 16), ("urgym_sac_policy_args", _abi.SacPolicyArgs, 12)):
        got = fields(name)
        assert len(got) == n and [(f, ctype[t]) for t, f in got] == list(mirror._fields_), name
    # five 4-byte fields, padded to 8, then eleven pointers; three 4-byte fields, padded, then nine pointers
    assert _abi.SacEntropyArgs.log_prob.offset == 24 and C.sizeof(_abi.SacEntropyArgs) == 24 + 11 * 8
    assert _abi.SacPolicyArgs.ent_coef.offset == 16 and C.sizeof(_abi.SacPolicyArgs) == 16 + 9 * 8
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    assert f"#define URGYM_SAC_TERMS_MAX_COUNT {_abi.SAC_TERMS_MAX_COUNT}" in hdr and _abi.SAC_TERMS_MAX_COUNT == 64 * _abi.SAC_TERMS_LANES
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
        assert re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    assert lib.urgym_abi_version() == 4
    # the arithmetic is stated in the header
    assert "y_out[m] = target_in[m] - e" in hdr and "loss   = -(l * mean)" in hdr and "partial[t] += partial[t + s]" in hdr


def test_refusals_that_need_no_device():
    lib = _native.lib()
    hp = _abi.AdamHyper(1e-4, 0.9, 0.999, 1e-8, 1, 0)
    # a NULL handle is refused before anything else is looked at
    assert lib.urgym_sac_entropy_step(None, C.byref(_abi.SacEntropyArgs()), C.byref(hp), None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert lib.urgym_sac_policy_terms(None, C.byref(_abi.SacPolicyArgs()), None) == _abi.ERR_ARG
    assert lib.urgym_sac_entropy_step(None, None, None, None) == _abi.ERR_ARG and lib.urgym_sac_policy_terms(None, None, None) == _abi.ERR_ARG
    # the restatements refuse half-given groups and what is not float32
    x = inputs(8)
    coef = adam_coefficients(None, step=1, **HYPER)
    ok = dict(target=x["target"], next_log_prob=x["next_log_prob"], gamma=GAMMA)
    for missing in ok:
        with pytest.raises(ValueError, match="half given"):
            entropy_step(1.0, x["log_prob"], TARGET_ENTROPY, 0.0, 0.0, 0.0, coef, **{k: v for k, v in ok.items() if k != missing})
    with pytest.raises(ValueError, match="half given"):
        entropy_step(1.0, x["log_prob"], TARGET_ENTROPY, 0.0, 0.0, 0.0, coef, terminated=x["terminated"])
    with pytest.raises(ValueError):
        entropy_step(1.0, x["log_prob"].astype(np.float64), TARGET_ENTROPY, 0.0, 0.0, 0.0, coef)
    with pytest.raises(ValueError, match="no group"):
        policy_terms(1.0)
    for half in (dict(dqmin_da=x["dqmin_da"]), dict(scale=1.0), dict(q=x["q"]), dict(y=x["y"]), dict(log_prob=x["log_prob"]), dict(q_min=x["q_min"])):
        with pytest.raises(ValueError, match="half given"):
            policy_terms(1.0, **half)
    with pytest.raises(ValueError):
        policy_terms(1.0, q=x["q"][:, :4], y=x["y"])


@pytest.mark.parametrize("lr", (1e-4, 1e-2))
@pytest.mark.parametrize("ent_coef_init", (1.0, 0.2))
def test_entropy_step_against_the_float64_temperature_update(lr, ent_coef_init):
    """SB3's update of log_ent_coef in float64: loss = -(l * (log_prob + target_entropy)).mean(), so g = -mean(log_prob + target_entropy);
    Adam with betas (0.9, 0.999), eps 1e-8 on the one element."""
    rng = np.random.default_rng(3)
    b1, b2, eps, M = 0.9, 0.999, 1e-8, 256
    l0 = np.float32(np.log(ent_coef_init))
    l, m, v = l0, np.float32(0), np.float32(0)
    l64, m64, v64 = float(l0), 0.0, 0.0
    for t in range(1, 6):
        log_prob = (rng.standard_normal(M) * 2.0 + rng.uniform(-8.0, 4.0)).astype(np.float32)  # a batch mean on either side of 6
        got = entropy_step(np.float32(np.exp(l)), log_prob, TARGET_ENTROPY, l, m, v, adam_coefficients(None, lr, (b1, b2), eps, t))
        l, m, v = got["l"][0], got["m"][0], got["v"][0]
        mean64 = float(np.mean(log_prob.astype(np.float64) + TARGET_ENTROPY))
        loss64, g64 = -(l64 * mean64), -mean64
        m64, v64 = b1 * m64 + (1 - b1) * g64, b2 * v64 + (1 - b2) * g64 * g64
        l_before = l64
        l64 -= lr / (1 - b1 ** t) * m64 / (np.sqrt(v64) / np.sqrt(1 - b2 ** t) + eps)
        bound = p_bound(t, max(abs(float(l0)), lr), lr)
        err = abs(float(l) - l64)
        print(f"lr={lr} l0={float(l0):.4f} step {t}: |l - l64| = {err:.3e} of bound {bound:.3e} ({err / bound:.2f})")
        assert err <= bound, (t, err, bound)
        # the loss is that of the OLD l, to float32 rounding of l * mean (l itself carries the error bounded above)
        assert abs(float(got["loss"]) - loss64) <= 2.0 ** -22 * abs(loss64) + abs(mean64) * p_bound(t, max(abs(float(l0)), lr), lr), (t, got["loss"], loss64, l_before)
