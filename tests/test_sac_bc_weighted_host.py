"""CPU tests (-m "not gpu") of advantage-weighted cloning in SAC's policy loss.

  * tests/sac_bc_weighted_harness.cpp, a stand-alone host program around urgym_sac_bc.h and urgym_mppi_temper.h -- the functions the kernel
    compiles -- equals evaluation.policy_terms_weighted bit for bit in every output (the seven float64 sums, the three losses, w, mean_abs,
    adv_ess, adv_max, both counts, every row's eligibility and weight, and d_action) at counts 1, 2, 1023, 1024, 1025, 2049 and 65536, with
    and without a mask, with and without a finite cap, at three temperatures (most e cut to +0.0, order one, the largest finite float32),
    and in the cases of a NaN q, an infinite advantage, an all-zero mask, one eligible row and a tie for A_max.  Built a second time with
    -fsanitize=address,undefined and run as that program.
  * the identities, bitwise: at the largest finite temperature without a cap every weight is exactly 1.0f and every shared output is
    policy_terms_cloned(q_filter=False)'s (with a mask: row_mask='s); rows that are not eligible are policy_terms'; the two losses always.
  * the weights against a float64 numpy softmax times n, within one float32 ulp.
  * the ctypes mirrors of the two new structs against the header's text and the C compiler's layout, the new symbols, the refusals that
    need no device, and the learner's option with its checkpoint rule.
"""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import sac_bc_weighted_cases as wc
from sac_bc_weighted_cases import CAPS, FLT_MAX, FORMS, HOST_COUNTS, MASKS, TEMPERATURES, same
from test_checkpoint_host import assembled_learner, learner_state
from ur_gym_amd import _abi, _native, checkpoint
from ur_gym_amd.evaluation import ordered_sum, policy_terms, policy_terms_weighted
from ur_gym_amd.training import ADV_DEFAULTS, BC_DEFAULTS, CLIP_DEFAULTS, DEMO_DEFAULTS, HER_DEFAULTS, NORM_DEFAULTS, PER_DEFAULTS, SAC_DEFAULTS, SACLearner
from ur_gym_amd.vector_env import _SAC_TRAIN_ENTRIES, _sac_train_entry

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
NEW_SYMBOLS = ("urgym_sac_policy_terms_weighted", "urgym_sac_train_weighted")
DEVICE = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)
HEADERS = ("urgym_sac_bc.h", "urgym_sac_terms.h", "urgym_adam.h", "urgym_pack_map.h", "urgym_mppi_temper.h", "urgym_mppi.h", "urgym_mppi_elite.h")


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "sac_bc_weighted_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h")] + [os.path.join(CSRC, h) for h in HEADERS]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("sac_bc_weighted_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("sac_bc_weighted_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run_harness(exe, tmp_path, x, count, masked, max_weight, temperature, scale_by_q=False, weight=wc.WEIGHT):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<qii", count, int(scale_by_q), int(masked)))
        with np.errstate(over="ignore"):
            f.write(np.array([x["alpha"], -1.0 / count, weight, 1.0 / count, temperature, max_weight], dtype=np.float32).tobytes())
        for k in ("log_prob", "q", "y", "q_min", "dqmin_da", "action_pi", "action_data"):
            f.write(np.ascontiguousarray(x[k], dtype=np.float32).tobytes())
        f.write(np.ascontiguousarray(x["mask"], dtype=np.uint8).tobytes())
    run = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (run.stdout, run.stderr[-2000:])
    raw = open(dst, "rb").read()
    assert len(raw) == 56 + 28 + 8 + count + 4 * count + 24 * count
    out = dict(sums=np.frombuffer(raw[:56], dtype=np.float64))
    out.update(zip(("critic_loss", "actor_loss", "bc_loss", "bc_weight", "mean_abs", "adv_ess", "adv_max"), np.frombuffer(raw[56:84], dtype=np.float32)))
    out["bc_rows"], out["adv_clipped"] = np.frombuffer(raw[84:92], dtype=np.int32)
    out["eligible"] = np.frombuffer(raw[92:92 + count], dtype=np.uint8).astype(bool)
    out["a"] = np.frombuffer(raw[92 + count:92 + 5 * count], dtype=np.float32)
    out["d_action"] = np.frombuffer(raw[92 + 5 * count:], dtype=np.float32).reshape(count, 6)
    return out


def same64(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).reshape(-1).view(np.uint64), np.asarray(b, dtype=np.float64).reshape(-1).view(np.uint64))


FLOATS = ("critic_loss", "actor_loss", "bc_loss", "bc_weight", "mean_abs", "adv_ess", "adv_max", "a", "d_action")


def compare(exe, tmp_path, count, variant, masked, max_weight, temperature, scale_by_q=False):
    x = wc.inputs(count, variant)
    got = run_harness(exe, tmp_path, x, count, masked, max_weight, temperature, scale_by_q)
    want = wc.restate(x, count, masked, max_weight, temperature, scale_by_q=scale_by_q)
    where = (count, variant, masked, max_weight, temperature, scale_by_q)
    for k in FLOATS:
        assert same(got[k], want[k]), (where, k, got[k], want[k])
    for k in ("bc_rows", "adv_clipped"):
        assert got[k] == want[k] and got[k].dtype == np.int32 and want[k].dtype == np.int32, (where, k, got[k], want[k])
    assert np.array_equal(got["eligible"], want["eligible"]), where
    with np.errstate(invalid="ignore"):
        sums = [ordered_sum(t) for t in (want["critic_terms"][0], want["critic_terms"][1], want["actor_terms"], np.abs(x["q_min"]))]
        sums += [want["Z"], want["Q"], ordered_sum(want["weighted_terms"])]
    assert same64(got["sums"], sums), (where, got["sums"], sums)
    return x, want


def compare_everything(exe, tmp_path):
    seen = dict(cut=0, clipped=0)
    for count in HOST_COUNTS:
        for masked, max_weight, temperature in FORMS:
            x, want = compare(exe, tmp_path, count, "plain", masked, max_weight, temperature, scale_by_q=count % 2 == 1)
            n = int(want["bc_rows"])
            assert n == (int(np.count_nonzero(x["mask"])) if masked else count) and np.isfinite(want["d_action"]).all()
            assert 1.0 <= want["adv_ess"] <= n and np.isfinite(want["bc_loss"]) and want["adv_max"] == want["a"].max()
            seen["cut"] += int(np.count_nonzero(want["eligible"] & (want["e"] == 0)))
            seen["clipped"] += int(want["adv_clipped"])
            if count >= 1023 and temperature == TEMPERATURES[0]:
                assert np.count_nonzero(want["e"][want["eligible"]] == 0) > n // 2  # most e fall below the cut
    assert seen["cut"] and seen["clipped"]
    for variant in wc.VARIANTS[1:]:
        for count in (1, 2, 1025):
            for masked, max_weight, temperature in FORMS:
                compare(exe, tmp_path, count, variant, masked, max_weight, temperature)


def test_shared_inputs_hold_what_the_cases_need():
    for count in sorted(set(HOST_COUNTS + wc.GPU_COUNTS)):
        x = wc.inputs(count)
        assert all(np.isfinite(v).all() for v in x.values()) and x["mask"][0] == 1 and x["mask"].dtype == np.uint8
        if count >= 65:
            assert 0 < np.count_nonzero(x["mask"]) < count
        want = wc.restate(wc.inputs(count, "nan_q"), count, False, np.inf, 1.0)
        assert not want["eligible"][count - 1] and want["bc_rows"] == count - 1 and np.isnan(want["critic_loss"])
        want = wc.restate(wc.inputs(count, "inf_advantage"), count, False, np.inf, 1.0)
        assert np.isposinf(want["advantage"][0]) and not want["eligible"][0] and want["bc_rows"] == count - 1
        want = wc.restate(wc.inputs(count, "zero_mask"), count, True, np.inf, 1.0)
        assert want["bc_rows"] == 0
        want = wc.restate(wc.inputs(count, "one_eligible"), count, True, np.inf, 1.0)
        assert want["bc_rows"] == 1 and want["a"][0] == 1 and want["adv_ess"] == 1 and want["adv_max"] == 1
        if count >= 2:
            want = wc.restate(wc.inputs(count, "tie"), count, False, np.inf, 1.0)
            assert want["e"][0] == 1.0 and want["e"][count - 1] == 1.0 and np.count_nonzero(want["e"] == 1.0) == 2


def test_shared_arithmetic_equals_the_restatement_bitwise(harness, tmp_path):
    compare_everything(harness, tmp_path)


def test_harness_is_clean_under_address_and_undefined_sanitizers(sanitized_harness, tmp_path):
    compare_everything(sanitized_harness, tmp_path)


@pytest.mark.parametrize("count", HOST_COUNTS)
def test_identities_hold_bitwise(count):
    x = wc.inputs(count)
    plain = policy_terms(x["alpha"], dqmin_da=x["dqmin_da"], scale=-1.0 / count, q=x["q"], y=x["y"], log_prob=x["log_prob"], q_min=x["q_min"])
    assert np.isfinite(wc.restate(x, count, False, np.inf, 1.0)["advantage"]).all()  # the identities are stated for finite A
    for masked in MASKS:
        for scale_by_q in (False, True):
            # the largest finite temperature, no cap: every weight is exactly 1.0f, and the call is the cloned one without the filter
            got = wc.restate(x, count, masked, np.inf, FLT_MAX, scale_by_q=scale_by_q)
            cloned = wc.restate_cloned(x, count, masked, scale_by_q=scale_by_q)
            assert same(got["a"][got["eligible"]], np.ones(int(got["bc_rows"]), np.float32)) and not got["a"][~got["eligible"]].any(), (count, masked)
            for k in ("d_action", "critic_loss", "actor_loss", "bc_loss", "bc_weight", "mean_abs", "bc_terms"):
                assert same(got[k], cloned[k]), (count, masked, scale_by_q, k)
            assert got["bc_rows"] == cloned["bc_rows"] and np.array_equal(got["eligible"], cloned["cloned"])
            assert got["adv_clipped"] == 0 and got["adv_max"] == 1 and got["adv_ess"] == np.float32(int(got["bc_rows"]))
        for max_weight, temperature in ((c, t) for c in CAPS for t in TEMPERATURES):
            got = wc.restate(x, count, masked, max_weight, temperature)
            # rows that are not eligible are policy_terms' rows, and the two losses are policy_terms' always
            assert same(got["d_action"][~got["eligible"]], plain["d_action"][~got["eligible"]]), (count, masked, max_weight, temperature)
            assert same(got["critic_loss"], plain["critic_loss"]) and same(got["actor_loss"], plain["actor_loss"])
            assert got["a"].max() <= np.float32(max_weight) and (got["adv_clipped"] == 0 or (got["a"] == np.float32(max_weight)).any())
    for variant in ("zero_mask", "nan_q", "inf_advantage", "nan_action_ineligible"):
        v = wc.inputs(count, variant)
        got = wc.restate(v, count, True, 2.0, 1.0)
        g = policy_terms(v["alpha"], dqmin_da=v["dqmin_da"], scale=-1.0 / count)["d_action"]
        assert same(got["d_action"][~got["eligible"]], g[~got["eligible"]]), (count, variant)
    zero = wc.restate(wc.inputs(count, "zero_mask"), count, True, 2.0, 1.0)  # n == 0: nothing is divided
    assert zero["bc_rows"] == 0 and zero["adv_clipped"] == 0 and not zero["a"].any() and same(zero["d_action"], plain["d_action"])
    for k in ("bc_loss", "adv_ess", "adv_max"):
        assert same(zero[k], np.float32(0.0)), k


def test_non_finite_actions_stay_where_the_header_says():
    count = 1025
    for masked, max_weight, temperature in FORMS:
        base = wc.restate(wc.inputs(count), count, masked, max_weight, temperature)
        got = wc.restate(wc.inputs(count, "nan_action"), count, masked, max_weight, temperature)  # row 0 is eligible
        rest = np.ones((count, 6), dtype=bool)
        rest[0, 3] = False
        # (where the row's weight underflowed to +0.0 the product a * h is still a NaN: 0 * NaN)
        assert got["eligible"][0] and np.isnan(got["bc_loss"]) and np.isnan(got["d_action"][0, 3]) and same(got["d_action"][rest], base["d_action"][rest])
        for k in ("critic_loss", "actor_loss", "bc_weight", "adv_ess", "adv_max", "a"):
            assert same(got[k], base[k]), k
        # the actions of a row that is not eligible reach nothing
        x = wc.inputs(count, "nan_action_ineligible")
        got = wc.restate(x, count, masked, max_weight, temperature)
        clean = dict(x, action_pi=np.where(np.isnan(x["action_pi"]), np.float32(0), x["action_pi"]), action_data=np.where(np.isnan(x["action_data"]), np.float32(0), x["action_data"]))
        want = wc.restate(clean, count, masked, max_weight, temperature)
        assert not got["eligible"][count - 1] and np.isfinite(got["d_action"]).all() and np.isfinite(got["bc_loss"])
        for k in ("d_action", "bc_loss", "a", "adv_ess", "adv_max"):
            assert same(got[k], want[k]), k


@pytest.mark.parametrize("count", (2, 1025, 65536))
@pytest.mark.parametrize("masked", MASKS)
@pytest.mark.parametrize("temperature", (0.5, 1.0, 8.0))
def test_weights_against_a_float64_softmax(count, masked, temperature):
    """a[m] = softmax(A / T)[m] * n.  The restatement's float64 value u = e / (Z / n) differs from the exact one by the exponential's 2 ulp
    (2^-52 relative), at most 65536 float64 additions in Z (each 2^-53 relative of a sum of positive terms), and three more float64
    roundings (the argument's division, Z / n, e / mean_e): far below 2^-24.  The float64 numpy softmax carries an error of the same
    order.  So after the one rounding to float32 the two agree within one float32 ulp (half an ulp each way of a common real number,
    which the two float64 values bracket to within 2^-35).  Rows on the cap are left out."""
    x = wc.inputs(count)
    for max_weight in CAPS:
        got = wc.restate(x, count, masked, max_weight, temperature)
        el = got["eligible"]
        A = got["advantage"].astype(np.float64)[el]
        z = (A - A.max()) / np.float64(np.float32(temperature))
        p = np.exp(z)
        want = p / p.sum() * el.sum()
        a = got["a"][el]
        free = want <= np.float64(np.float32(max_weight)) * (1 - 2.0 ** -30)  # off the cap, with room for the float64 errors
        free &= a != np.float32(max_weight)
        want32 = want.astype(np.float32)
        ulp = np.spacing(np.maximum(np.abs(want32), np.float32(np.finfo(np.float32).tiny)))
        err = np.abs(a.astype(np.float64) - want32.astype(np.float64))
        print(f"count {count} masked {masked} T {temperature} cap {max_weight}: max err / ulp = {np.max(err[free] / ulp[free]):.3f} over {free.sum()} rows")
        assert free.sum() >= el.sum() // 2 and (err[free] <= ulp[free]).all()
        assert abs(float(a.astype(np.float64).mean()) - 1.0) < 1e-6 or max_weight != np.inf  # without a cap the weights average to 1


def test_structs_mirror_the_header(harness):
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    layout = json.loads(subprocess.run([harness, "layout"], capture_output=True, text=True, check=True).stdout)
    for name, mirror in (("urgym_sac_advantage_args", _abi.SacAdvantageArgs), ("urgym_sac_weighting", _abi.SacWeighting)):
        body = hdr[hdr.index(f"typedef struct {name} {{"):hdr.index(f"}} {name};")]
        declared = re.findall(r"^\s*(const uint8_t\*|const float\*|float\*|int32_t\*|float|int32_t)\s+(\w+);", body, flags=re.M)
        ctype = {"const uint8_t*": C.POINTER(C.c_uint8), "const float*": C.POINTER(C.c_float), "float*": C.POINTER(C.c_float), "int32_t*": C.POINTER(C.c_int32),
                 "float": C.c_float, "int32_t": C.c_int32}
        assert [(f, ctype[t]) for t, f in declared] == list(mirror._fields_), name  # the header's order and types are the mirror's
        want = layout[name]
        assert C.sizeof(mirror) == want.pop("sizeof"), name
        assert {f: getattr(mirror, f).offset for f, _ in mirror._fields_} == want, name  # the C compiler's own offsets
    assert C.sizeof(_abi.SacAdvantageArgs) == 48 and C.sizeof(_abi.SacWeighting) == 40
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    assert lib.urgym_abi_version() == 4
    # the header states the arithmetic
    for text in ("A[m]    = qd - q_min[m]", "elig[m] = (row_mask == NULL || row_mask[m] != 0) && isfinite(A[m])", "mean_e = Z / (double)n",
                 "u = e[m] / mean_e;  v = u > (double)max_weight ? (double)max_weight : u;  a[m] = (float)v", "wr = w * a[m];  t = d_k * wr;  u = t * bc_scale",
                 "adv_ess_out[0] = (float)((Z * Z) / Q)", "With n == 0 nothing is divided"):
        assert text in hdr, text
    # the training entry: ahead of the table, which stays what it was, with weighting then cloning first and every other option after
    assert len(_SAC_TRAIN_ENTRIES) == 10 and all("weighting" not in opts for _, _, opts in _SAC_TRAIN_ENTRIES)
    for present in (set(), {"planner", "noise"}, {"normalizer", "clipping"}, {"monitor"}, {"demonstrating"}, {"nstep"}):
        symbol, options = _sac_train_entry(present | {"cloning", "weighting"})
        assert symbol == "urgym_sac_train_weighted" and options[:2] == ("weighting", "cloning") and present <= set(options)
        assert _sac_train_entry(present | {"cloning"})[0] != "urgym_sac_train_weighted"
    symbol, options = _sac_train_entry({"weighting", "cloning"})
    argtypes = lib.urgym_sac_train_weighted.argtypes
    mirrors = dict(weighting=_abi.SacWeighting, cloning=_abi.SacCloning, demonstrating=_abi.SacDemonstrating, planner=_abi.SacPlanning, temper=_abi.MppiTemper,
                   noise=_abi.MppiNoise, normalizer=_abi.Normalization, clipping=_abi.SacClipping, nstep=_abi.SacNstep, prioritized=_abi.SacPrioritized,
                   hindsight=_abi.SacHindsight, evaluation=_abi.SacEvaluation, monitor=_abi.SacMonitoring)
    assert len(argtypes) == len(options) + 4 and [argtypes[3 + i] for i in range(len(options))] == [C.POINTER(mirrors[o]) for o in options]
    # the header's parameter order is the table's
    decl = re.search(r"^int urgym_sac_train_weighted\((.*)\);$", hdr, flags=re.M).group(1)
    names = [p.split()[-1].replace("_or_NULL", "") for p in decl.split(",")]
    rename = dict(planning="planner", normalization="normalizer", monitoring="monitor")
    assert [rename.get(n, n) for n in names[3:-1]] == list(options)


def test_refusals_that_need_no_device():
    lib = _native.lib()
    # a NULL handle is refused before anything else is looked at
    assert lib.urgym_sac_policy_terms_weighted(None, C.byref(_abi.SacPolicyArgs()), C.byref(_abi.SacCloneArgs()), C.byref(_abi.SacAdvantageArgs()), None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert lib.urgym_sac_policy_terms_weighted(None, None, None, None, None) == _abi.ERR_ARG
    fn = lib.urgym_sac_train_weighted
    assert fn(None, C.byref(_abi.SacLearner()), C.byref(_abi.SacSchedule()), C.byref(_abi.SacWeighting()), C.byref(_abi.SacCloning()), *[None] * 12) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert fn(*[None] * len(fn.argtypes)) == _abi.ERR_ARG
    # the restatement refuses what the call refuses about the numbers, and shapes that are not the rows'
    x = wc.inputs(8)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="temperature"):
            wc.restate(x, 8, False, np.inf, bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_weight"):
            wc.restate(x, 8, False, bad, 1.0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="weight"):
            wc.restate(x, 8, False, np.inf, 1.0, weight=bad)
    kw = dict(dqmin_da=x["dqmin_da"], scale=-0.125, q=x["q"], y=x["y"], log_prob=x["log_prob"], q_min=x["q_min"], action_pi=x["action_pi"], action_data=x["action_data"],
              weight=1.0, bc_scale=0.125, temperature=1.0)
    for over in (dict(action_pi=x["action_pi"][:4]), dict(action_data=x["action_data"].astype(np.float64)), dict(row_mask=x["mask"][:4]), dict(row_mask=x["mask"].astype(np.int32))):
        with pytest.raises(ValueError):
            policy_terms_weighted(x["alpha"], **dict(kw, **over))


def test_learner_option_and_the_checkpoint_rule_for_the_advantage_weight():
    assert ADV_DEFAULTS == dict(bc_advantage_temperature=None, bc_advantage_max_weight=None)
    others = set(SAC_DEFAULTS) | set(PER_DEFAULTS) | set(HER_DEFAULTS) | set(CLIP_DEFAULTS) | set(NORM_DEFAULTS) | set(BC_DEFAULTS) | set(DEMO_DEFAULTS)
    assert not set(ADV_DEFAULTS) & others
    ADV = dict(bc_weight=0.5, bc_scale_by_q=True, bc_advantage_temperature=2.0, bc_advantage_max_weight=20.0)
    plain = assembled_learner()
    cloned = assembled_learner(**DEVICE, bc_weight=0.5)
    weighted = assembled_learner(**DEVICE, **ADV)
    for L in (plain, cloned, assembled_learner(**ADV_DEFAULTS)):  # without the option: no new key
        assert not set(ADV_DEFAULTS) & set(L._saved_hp())
    assert {k: weighted._saved_hp()[k] for k in ADV} == ADV
    # a state with the option round-trips through the checkpoint's own flattening, and a mismatch either way is refused
    state = dict(learner_state(weighted), hp=weighted._saved_hp())
    arrays, tree = checkpoint.flatten(state)
    back = checkpoint.unflatten(arrays, json.loads(json.dumps(tree)))
    assert back["hp"] == state["hp"]
    weighted.check_state_dict(back)
    plain.check_state_dict(dict(learner_state(plain), hp=plain._saved_hp()))  # a file without the option holds no new key and loads
    cloned.check_state_dict(dict(learner_state(cloned), hp=cloned._saved_hp()))
    with pytest.raises(ValueError, match="bc_advantage_temperature is 2.0 in the checkpoint, None here"):
        assembled_learner(**DEVICE, bc_weight=0.5, bc_scale_by_q=True).check_state_dict(back)
    with pytest.raises(ValueError, match="bc_advantage_temperature is None in the checkpoint, 2.0 here"):
        weighted.check_state_dict(dict(learner_state(weighted), hp={k: v for k, v in weighted._saved_hp().items() if k not in ADV_DEFAULTS}))
    with pytest.raises(ValueError, match="bc_advantage_temperature is 2.0 in the checkpoint, 3.0 here"):
        assembled_learner(**DEVICE, **dict(ADV, bc_advantage_temperature=3.0)).check_state_dict(back)
    with pytest.raises(ValueError, match="bc_advantage_max_weight is 20.0 in the checkpoint, None here"):
        assembled_learner(**DEVICE, **dict(ADV, bc_advantage_max_weight=None)).check_state_dict(back)
    with pytest.raises(ValueError, match="only"):
        weighted.check_state_dict(back, override=("bc_advantage_temperature",))
    # the constructor's refusals, before it touches the environment
    with pytest.raises(ValueError, match="bc_advantage_temperature needs bc_weight"):
        SACLearner(None, **DEVICE, bc_advantage_temperature=1.0)
    with pytest.raises(ValueError, match="bc_weight needs device_entropy=True"):
        SACLearner(None, bc_weight=1.0, bc_advantage_temperature=1.0)
    with pytest.raises(ValueError, match="alternatives"):
        SACLearner(None, **DEVICE, bc_weight=1.0, bc_q_filter=True, bc_advantage_temperature=1.0)
    with pytest.raises(ValueError, match="needs it"):
        SACLearner(None, **DEVICE, bc_weight=1.0, bc_advantage_max_weight=2.0)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e39, True, "1"):
        with pytest.raises(ValueError, match="bc_advantage_temperature must be"):
            SACLearner(None, **DEVICE, bc_weight=1.0, bc_advantage_temperature=bad)
    for bad in (0.0, -1.0, float("nan"), True, "1"):
        with pytest.raises(ValueError, match="bc_advantage_max_weight must be"):
            SACLearner(None, **DEVICE, bc_weight=1.0, bc_advantage_temperature=1.0, bc_advantage_max_weight=bad)
    with pytest.raises(TypeError, match="bc_advantage_temperature"):  # the list of what is available names the new options
        SACLearner(None, bc_advantage_temprature=1.0)
