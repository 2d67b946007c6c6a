"""CPU tests (-m "not gpu") of behaviour cloning in SAC's policy loss.

  * tests/sac_bc_harness.cpp, a stand-alone host program around urgym_sac_bc.h -- the functions the kernel compiles -- equals
    evaluation.policy_terms_cloned bit for bit in every output (the five float64 sums, the three losses, w, mean_abs, the row count, the
    verdict of every row and d_action) at counts 1, 2, 1023, 1024, 1025, 2049 and 65536 under all four flag combinations, and in the
    cases of a NaN q_min row, a NaN action row and +-0 differences.  Built a second time with -fsanitize=address,undefined and run as
    that program.
  * the restatement against float64: d_action within five roundings of g64 + u64, bc_loss within the bound of the ordered sum.
  * the ctypes mirrors of the two new structs against the header's text and the C compiler's layout, the new symbols, the refusals
    that need no device, and the learner's option with its checkpoint rule.
"""
import ctypes as C
import json
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import sac_bc_cases as bc
from sac_bc_cases import FLAGS, HOST_COUNTS, WEIGHT, same
from test_checkpoint_host import assembled_learner, learner_state
from ur_gym_amd import _abi, _native, checkpoint
from ur_gym_amd.evaluation import ordered_sum, policy_terms, policy_terms_cloned
from ur_gym_amd.training import BC_DEFAULTS, CLIP_DEFAULTS, HER_DEFAULTS, NORM_DEFAULTS, PER_DEFAULTS, SAC_DEFAULTS, SACLearner
from ur_gym_amd.vector_env import _SAC_TRAIN_ENTRIES, _sac_train_entry

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
NEW_SYMBOLS = ("urgym_sac_policy_terms_cloned", "urgym_sac_train_cloned")
DEVICE = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "sac_bc_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h")] + [os.path.join(CSRC, h) for h in ("urgym_sac_bc.h", "urgym_sac_terms.h", "urgym_adam.h", "urgym_pack_map.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("sac_bc_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("sac_bc_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run_harness(exe, tmp_path, x, count, scale_by_q, q_filter, weight=WEIGHT):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<qii", count, int(scale_by_q), int(q_filter)))
        f.write(np.array([x["alpha"], -1.0 / count, weight, 1.0 / count], dtype=np.float32).tobytes())
        for k in ("log_prob", "q", "y", "q_min", "dqmin_da", "action_pi", "action_data"):
            f.write(np.ascontiguousarray(x[k], dtype=np.float32).tobytes())
    run = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (run.stdout, run.stderr[-2000:])
    raw = open(dst, "rb").read()
    assert len(raw) == 40 + 20 + 4 + count + 24 * count
    out = dict(sums=np.frombuffer(raw[:40], dtype=np.float64))
    out.update(zip(("critic_loss", "actor_loss", "bc_loss", "bc_weight", "mean_abs"), np.frombuffer(raw[40:60], dtype=np.float32)))
    out["bc_rows"] = np.frombuffer(raw[60:64], dtype=np.int32)[0]
    out["cloned"] = np.frombuffer(raw[64:64 + count], dtype=np.uint8).astype(bool)
    out["d_action"] = np.frombuffer(raw[64 + count:], dtype=np.float32).reshape(count, 6)
    return out


def same64(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).reshape(-1).view(np.uint64), np.asarray(b, dtype=np.float64).reshape(-1).view(np.uint64))


def compare(exe, tmp_path, count, variant, scale_by_q, q_filter):
    x = bc.inputs(count, variant)
    got = run_harness(exe, tmp_path, x, count, scale_by_q, q_filter)
    want = bc.restate(x, count, scale_by_q, q_filter)
    where = (count, variant, scale_by_q, q_filter)
    for k in ("critic_loss", "actor_loss", "bc_loss", "bc_weight", "mean_abs", "d_action"):
        assert same(got[k], want[k]), (where, k, got[k], want[k])
    assert got["bc_rows"] == want["bc_rows"] and got["bc_rows"].dtype == np.int32 and want["bc_rows"].dtype == np.int32, where
    assert np.array_equal(got["cloned"], want["cloned"]), where
    with np.errstate(invalid="ignore"):
        sums = [ordered_sum(t) for t in (want["critic_terms"][0], want["critic_terms"][1], want["actor_terms"], np.abs(x["q_min"]), want["bc_terms"])]
    assert same64(got["sums"], sums), (where, got["sums"], sums)
    return x, want


def compare_everything(exe, tmp_path):
    for count in HOST_COUNTS:
        for scale_by_q, q_filter in FLAGS:
            x, want = compare(exe, tmp_path, count, "plain", scale_by_q, q_filter)
            if not q_filter:
                assert want["cloned"].all() and want["bc_rows"] == count
            elif count >= 2:
                assert 0 < want["bc_rows"] < count and want["cloned"][0] and not want["cloned"][1]
            assert np.isfinite(want["d_action"]).all() and np.isfinite(want["bc_loss"]) and np.isfinite(want["bc_weight"])
    for variant in bc.VARIANTS[1:]:
        for count in (1, 2, 1025):
            for scale_by_q, q_filter in FLAGS:
                compare(exe, tmp_path, count, variant, scale_by_q, q_filter)


def test_shared_inputs_hold_what_the_cases_need():
    for count in set(HOST_COUNTS + bc.GPU_COUNTS):
        x = bc.inputs(count)
        assert all(np.isfinite(v).all() for v in x.values())
        if count >= 2:
            bc.check_inputs(x, count)
        assert np.isnan(bc.inputs(count, "nan_q_min")["q_min"]).sum() == 1 and np.isnan(bc.inputs(count, "nan_action")["action_pi"]).sum() == 1
        z = bc.inputs(count, "zero_differences")
        d = z["action_pi"] - z["action_data"]
        assert ((d == 0) & np.signbit(d)).any() and ((d == 0) & ~np.signbit(d)).any()


def test_shared_arithmetic_equals_the_restatement_bitwise(harness, tmp_path):
    compare_everything(harness, tmp_path)


def test_harness_is_clean_under_address_and_undefined_sanitizers(sanitized_harness, tmp_path):
    compare_everything(sanitized_harness, tmp_path)


def test_non_finite_values_stay_where_the_header_says():
    count = 1025
    plain = {flags: bc.restate(bc.inputs(count), count, *flags) for flags in FLAGS}
    for (scale_by_q, q_filter), base in plain.items():
        # a NaN action of a cloned row reaches that row and the cloning loss, nothing else
        got = bc.restate(bc.inputs(count, "nan_action"), count, scale_by_q, q_filter)
        assert got["cloned"][0] and np.isnan(got["d_action"][0, 3]) and np.isnan(got["bc_loss"])
        rest = np.ones((count, 6), dtype=bool)
        rest[0, 3] = False
        assert same(got["d_action"][rest], base["d_action"][rest]) and same(got["bc_weight"], base["bc_weight"])
        assert same(got["critic_loss"], base["critic_loss"]) and same(got["actor_loss"], base["actor_loss"])
        # a NaN q_min reaches w only with scale_by_q, and through w every cloned row; rows that are not cloned are never touched
        x = bc.inputs(count, "nan_q_min")
        got = bc.restate(x, count, scale_by_q, q_filter)
        g = policy_terms(x["alpha"], dqmin_da=x["dqmin_da"], scale=-1.0 / count)["d_action"]
        assert np.isnan(got["mean_abs"]) and np.isnan(got["bc_weight"]) == scale_by_q
        assert got["cloned"][count - 1] == (not q_filter)  # a NaN on either side of the filter: not cloned
        assert same(got["d_action"][~got["cloned"]], g[~got["cloned"]])
        if scale_by_q:
            assert np.isnan(got["d_action"][got["cloned"]]).all()
        else:
            assert np.isfinite(got["d_action"]).all() and np.isfinite(got["bc_loss"])


def test_weight_zero_and_unfiltered_rows_against_policy_terms():
    count = 1025
    x = bc.inputs(count, "zero_differences")
    plain = policy_terms(x["alpha"], dqmin_da=x["dqmin_da"], scale=-1.0 / count, q=x["q"], y=x["y"], log_prob=x["log_prob"], q_min=x["q_min"])
    for scale_by_q, q_filter in FLAGS:
        got = bc.restate(x, count, scale_by_q, q_filter)
        assert same(got["critic_loss"], plain["critic_loss"]) and same(got["actor_loss"], plain["actor_loss"])
        assert same(got["d_action"][~got["cloned"]], plain["d_action"][~got["cloned"]])
        zero = bc.restate(x, count, scale_by_q, q_filter, weight=0.0)
        # g + (+-0) compares equal to g; a -0.0 g may become +0.0, so the comparison is by value
        assert np.array_equal(zero["d_action"], plain["d_action"]) and zero["bc_weight"] == 0
        assert same(zero["bc_loss"], got["bc_loss"])
    # w_mean_abs replaces the mean in the weight and nothing else
    other = bc.restate(x, count, True, False, w_mean_abs=np.float32(2.0))
    assert same(other["bc_weight"], np.float32(WEIGHT) * np.float32(2.0)) and same(other["mean_abs"], bc.restate(x, count, True, False)["mean_abs"])


def moderate_inputs(count, seed=7):
    """Inputs of ordinary magnitude, far from the subnormal range: every product below is at least 2^-24 * 2^-17 * 2^-16 in magnitude or
    exactly zero, so float32 rounds each operation to relative 2^-24."""
    rng = np.random.default_rng([seed, count])
    x = dict(log_prob=rng.normal(-3.0, 2.0, count), y=rng.normal(-5.0, 3.0, count), q=rng.normal(-5.0, 3.0, (2, count)), q_min=rng.normal(-5.0, 3.0, count),
             dqmin_da=rng.normal(0.0, 2.0, (count, 6)), action_pi=np.tanh(rng.standard_normal((count, 6))), action_data=rng.uniform(-1.0, 1.0, (count, 6)))
    x = {k: v.astype(np.float32) for k, v in x.items()}
    x["alpha"] = np.float32(0.2)
    return x


@pytest.mark.parametrize("count", (2, 1025, 65536))
@pytest.mark.parametrize("scale_by_q,q_filter", FLAGS)
def test_restatement_against_float64(count, scale_by_q, q_filter):
    """d_action of a cloned row is five float32 roundings away from g64 + u64 = dqmin_da * scale + (a - b) * w * bc_scale, with w the
    float32 the restatement reports: dqmin_da * scale (g, relative 2^-24 of |g|), a - b, * w, * bc_scale (u, three roundings: relative
    3 * 2^-24 of |u| to first order) and the sum (2^-24 of |g + u| <= |g| + |u|): 2^-24 (2 |g64| + 4 |u64|), times 1.01 for the second
    order.  bc_loss is the ordered sum of EXACT float32 terms h in float64: a term passes through at most ceil(count / 1024) - 1 + 10
    additions, each relative 2^-53, then the division (2^-53) and one rounding to float32 (2^-24)."""
    x = moderate_inputs(count)
    got = bc.restate(x, count, scale_by_q, q_filter)
    f8 = lambda v: np.asarray(v, dtype=np.float64)  # noqa: E731
    scale, bc_scale, w = f8(np.float32(-1.0 / count)), f8(np.float32(1.0 / count)), f8(got["bc_weight"])
    g64 = f8(x["dqmin_da"]) * scale
    u64 = (f8(x["action_pi"]) - f8(x["action_data"])) * w * bc_scale
    u64 = np.where(got["cloned"][:, None], u64, 0.0)
    err = np.abs(f8(got["d_action"]) - (g64 + u64))
    bound = 1.01 * 2.0 ** -24 * (2 * np.abs(g64) + 4 * np.abs(u64))
    print(f"count {count} flags {scale_by_q, q_filter}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}, cloned {got['bc_rows']}")
    assert (err <= bound).all()
    assert (err[~got["cloned"]] <= 1.01 * 2.0 ** -24 * np.abs(g64[~got["cloned"]])).all()  # one rounding where nothing is cloned
    h = f8(got["bc_terms"])
    exact = math.fsum(h) / count
    depth = -(-count // 1024) - 1 + 10
    bound = 1.01 * (2.0 ** -24 * abs(exact) + (depth + 1) * 2.0 ** -53 * math.fsum(np.abs(h)) / count)
    print(f"  bc_loss {got['bc_loss']!r}: |err| = {abs(float(got['bc_loss']) - exact):.3e} of bound {bound:.3e}")
    assert abs(float(got["bc_loss"]) - exact) <= bound
    # the term itself: half the squared distance in float64, within the roundings of six differences, squares and sums
    d64 = f8(x["action_pi"]) - f8(x["action_data"])
    h64 = np.where(got["cloned"], 0.5 * (d64 * d64).sum(1), 0.0)
    assert (np.abs(h - h64) <= 1.01 * 9 * 2.0 ** -24 * h64).all()


def test_structs_mirror_the_header(harness):
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    layout = json.loads(subprocess.run([harness, "layout"], capture_output=True, text=True, check=True).stdout)
    for name, mirror in (("urgym_sac_clone_args", _abi.SacCloneArgs), ("urgym_sac_cloning", _abi.SacCloning)):
        body = hdr[hdr.index(f"typedef struct {name} {{"):hdr.index(f"}} {name};")]
        declared = re.findall(r"^\s*(const float\*|float\*|int32_t\*|float|int32_t)\s+(\w+);", body, flags=re.M)
        ctype = {"const float*": C.POINTER(C.c_float), "float*": C.POINTER(C.c_float), "int32_t*": C.POINTER(C.c_int32), "float": C.c_float, "int32_t": C.c_int32}
        assert [(f, ctype[t]) for t, f in declared] == list(mirror._fields_), name  # the header's order and types are the mirror's
        want = layout[name]
        assert C.sizeof(mirror) == want.pop("sizeof"), name
        assert {f: getattr(mirror, f).offset for f, _ in mirror._fields_} == want, name  # the C compiler's own offsets
    assert C.sizeof(_abi.SacCloneArgs) == 64 and C.sizeof(_abi.SacCloning) == 40
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    assert lib.urgym_abi_version() == 4
    # the header states the arithmetic
    for text in ("qd        = q[1][m] < q[0][m] ? q[1][m] : q[0][m]", "cloned[m] = q_filter ? (qd > q_min[m]) : true", "h[m]      = 0.5f * s",
                 "w = scale_by_q ? weight * mean_abs : weight", "t = d_k * w;  u = t * bc_scale;  d_action_out[m][k] = g + u", "a -0.0 g may become +0.0"):
        assert text in hdr, text
    # the training entry: ahead of the table, which stays what it was, with every other option after cloning
    assert len(_SAC_TRAIN_ENTRIES) == 10 and all("cloning" not in opts for _, _, opts in _SAC_TRAIN_ENTRIES)
    for present in (set(), {"planner", "noise"}, {"normalizer", "clipping"}, {"monitor"}):
        symbol, options = _sac_train_entry(present | {"cloning"})
        assert symbol == "urgym_sac_train_cloned" and options[0] == "cloning" and present <= set(options)
        assert _sac_train_entry(present)[0] != "urgym_sac_train_cloned"
    symbol, options = _sac_train_entry({"cloning"})
    argtypes = lib.urgym_sac_train_cloned.argtypes
    mirrors = dict(cloning=_abi.SacCloning, planner=_abi.SacPlanning, temper=_abi.MppiTemper, noise=_abi.MppiNoise, normalizer=_abi.Normalization, clipping=_abi.SacClipping,
                   nstep=_abi.SacNstep, prioritized=_abi.SacPrioritized, hindsight=_abi.SacHindsight, evaluation=_abi.SacEvaluation, monitor=_abi.SacMonitoring)
    assert len(argtypes) == len(options) + 4 and [argtypes[3 + i] for i in range(len(options))] == [C.POINTER(mirrors[o]) for o in options]


def test_refusals_that_need_no_device():
    lib = _native.lib()
    # a NULL handle is refused before anything else is looked at
    assert lib.urgym_sac_policy_terms_cloned(None, C.byref(_abi.SacPolicyArgs()), C.byref(_abi.SacCloneArgs()), None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert lib.urgym_sac_policy_terms_cloned(None, None, None, None) == _abi.ERR_ARG
    fn = lib.urgym_sac_train_cloned
    assert fn(None, C.byref(_abi.SacLearner()), C.byref(_abi.SacSchedule()), C.byref(_abi.SacCloning()), *[None] * 11) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert fn(*[None] * len(fn.argtypes)) == _abi.ERR_ARG
    # the restatement refuses what the call refuses about the numbers, and shapes that are not the rows'
    x = bc.inputs(8)
    for bad in (-1.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="weight"):
            bc.restate(x, 8, False, False, weight=bad)
    with pytest.raises(ValueError):
        policy_terms_cloned(x["alpha"], dqmin_da=x["dqmin_da"], scale=-0.125, q=x["q"], y=x["y"], log_prob=x["log_prob"], q_min=x["q_min"], action_pi=x["action_pi"][:4],
                            action_data=x["action_data"], weight=1.0, bc_scale=0.125)
    with pytest.raises(ValueError):
        policy_terms_cloned(x["alpha"], dqmin_da=x["dqmin_da"], scale=-0.125, q=x["q"], y=x["y"], log_prob=x["log_prob"], q_min=x["q_min"], action_pi=x["action_pi"],
                            action_data=x["action_data"].astype(np.float64), weight=1.0, bc_scale=0.125)


def test_learner_option_and_the_checkpoint_rule_for_cloning():
    assert BC_DEFAULTS == dict(bc_weight=None, bc_scale_by_q=False, bc_q_filter=False)
    assert not set(BC_DEFAULTS) & (set(SAC_DEFAULTS) | set(PER_DEFAULTS) | set(HER_DEFAULTS) | set(CLIP_DEFAULTS) | set(NORM_DEFAULTS))
    plain = assembled_learner()
    cloned = assembled_learner(**DEVICE, bc_weight=0.5, bc_scale_by_q=True, bc_q_filter=False)
    for L in (plain, assembled_learner(**BC_DEFAULTS)):  # without the option: no new key
        assert not set(BC_DEFAULTS) & set(L._saved_hp())
    assert {k: cloned._saved_hp()[k] for k in BC_DEFAULTS} == dict(bc_weight=0.5, bc_scale_by_q=True, bc_q_filter=False)
    # a state with the option round-trips through the checkpoint's own flattening, and a mismatch either way is refused
    state = dict(learner_state(cloned), hp=cloned._saved_hp())
    arrays, tree = checkpoint.flatten(state)
    back = checkpoint.unflatten(arrays, json.loads(json.dumps(tree)))
    assert back["hp"] == state["hp"]
    cloned.check_state_dict(back)
    plain.check_state_dict(dict(learner_state(plain), hp=plain._saved_hp()))  # a file without the option holds no new key and loads
    with pytest.raises(ValueError, match="bc_weight is 0.5 in the checkpoint, None here"):
        assembled_learner(**DEVICE).check_state_dict(back)
    with pytest.raises(ValueError, match="bc_weight is None in the checkpoint, 0.5 here"):
        cloned.check_state_dict(dict(learner_state(cloned), hp={k: v for k, v in cloned._saved_hp().items() if k not in BC_DEFAULTS}))
    with pytest.raises(ValueError, match="bc_weight is 0.5 in the checkpoint, 2.0 here"):
        assembled_learner(**DEVICE, bc_weight=2.0, bc_scale_by_q=True, bc_q_filter=False).check_state_dict(back)
    with pytest.raises(ValueError, match="bc_scale_by_q is True in the checkpoint, False here"):
        assembled_learner(**DEVICE, bc_weight=0.5, bc_scale_by_q=False, bc_q_filter=False).check_state_dict(back)
    with pytest.raises(ValueError, match="bc_q_filter is False in the checkpoint, True here"):
        assembled_learner(**DEVICE, bc_weight=0.5, bc_scale_by_q=True, bc_q_filter=True).check_state_dict(back)
    with pytest.raises(ValueError, match="only"):
        cloned.check_state_dict(back, override=("bc_weight",))
    # the constructor's refusals, before it touches the environment
    with pytest.raises(ValueError, match="bc_weight needs device_entropy=True"):
        SACLearner(None, bc_weight=1.0)
    for bad in (-1.0, -1e-30, float("nan"), float("inf"), 1e39, True, "1"):
        with pytest.raises(ValueError, match="bc_weight must be"):
            SACLearner(None, **DEVICE, bc_weight=bad)
    for k in ("bc_scale_by_q", "bc_q_filter"):
        with pytest.raises(ValueError, match=f"{k} must be True or False"):
            SACLearner(None, **DEVICE, bc_weight=1.0, **{k: 1})
        with pytest.raises(ValueError, match="need it"):
            SACLearner(None, **DEVICE, **{k: True})
    with pytest.raises(TypeError, match="bc_weight"):  # the list of what is available names the new options
        SACLearner(None, bc_wieght=1.0)
