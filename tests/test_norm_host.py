"""CPU tests (-m "not gpu") of the running observation and reward normalization.

  * tests/norm_harness.cpp, a stand-alone host program around ur_gym_amd/csrc/urgym_norm.h -- the header the kernels compile -- equals
    evaluation.norm_sums, norm_fold, normalize_rows and normalize_reward bitwise: sums, merges over several slots, split folds, inv,
    normalized values, clip edges hit exactly; built a second time with -fsanitize=address,undefined and run as that program.
  * evaluation.norm_fold against exact rational arithmetic, within the forward-error bound tests/norm_cases.py derives from the stated
    order; and against a literal float64 RunningMeanStd (np.mean, np.var, the merge) within twice that bound.
  * the ctypes mirrors of the three new structs against the C compiler's own layout, the new symbols, the refusals that need no device,
    and the learner option's refusals and checkpoint key rule.
"""
import ctypes as C
import json
import os
import re
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from norm_cases import (CAP, GAMMA, GOAL_DIM, HOST_COUNTS, OBS_DIM, SPLIT, WHOLE, bounded_merge, bounded_sum, literal_running_mean_std, restate, ring,
                        sum_depth)
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import (NORM_ROW_GROUPS, DeviceNormalizer, norm_fold, norm_initial_state, norm_merge, norm_sums, normalize_reward, normalize_rows)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
STATE = [name for name, _ in _abi.NORM_STATE_FIELDS]
RING = ("observation", "achieved_goal", "desired_goal", "reward", "terminated", "truncated")


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "norm_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h")] + [os.path.join(CSRC, h) for h in ("urgym_norm.h", "urgym_pack_map.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("norm_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("norm_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run_harness(exe, *args):
    run = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (args, run.returncode, run.stdout[-500:], run.stderr[-2000:])
    return run.stdout


def harness_fold(exe, tmp_path, n, script, norm_obs=True, norm_reward=True, seed=1):
    tmp = str(tmp_path)
    state, r = norm_initial_state(n, OBS_DIM, GOAL_DIM), ring(n, seed)
    with open(os.path.join(tmp, "state.bin"), "wb") as f:
        f.write(b"".join(state[k].tobytes() for k in STATE))
    with open(os.path.join(tmp, "ring.bin"), "wb") as f:
        f.write(b"".join(np.ascontiguousarray(r[k]).tobytes() for k in RING))
    run_harness(exe, "fold", os.path.join(tmp, "state.bin"), os.path.join(tmp, "ring.bin"), os.path.join(tmp, "out.bin"), n, OBS_DIM, GOAL_DIM, CAP, repr(GAMMA),
                int(norm_obs), int(norm_reward), *[f"{a}:{b}" for a, b in script])
    raw, out, at = open(os.path.join(tmp, "out.bin"), "rb").read(), {}, 0
    for name in STATE:
        out[name] = np.frombuffer(raw, np.float64, state[name].size, at)
        at += 8 * state[name].size
    assert at == len(raw)
    return out


def harness_apply(exe, tmp_path, x, mean, var, eps, clip, reward=False):
    tmp = str(tmp_path)
    with open(os.path.join(tmp, "apply.bin"), "wb") as f:
        f.write(np.ascontiguousarray(x, np.float32).tobytes() + np.asarray(mean, np.float64).tobytes() + np.asarray(var, np.float64).tobytes())
    run_harness(exe, "apply", os.path.join(tmp, "apply.bin"), os.path.join(tmp, "applied.bin"), x.shape[0], x.shape[1], repr(float(eps)), repr(float(clip)), int(reward))
    return np.fromfile(os.path.join(tmp, "applied.bin"), np.float32).reshape(x.shape)


def clip_cases():
    """[count, d] values with mean and var chosen so that both clip bounds are hit EXACTLY and exceeded: with mean 1, var 0.25 - eps
    (inv = 2 exactly) and clip 10, x = 6 gives +10, x = -4 gives -10, x = 6.5 and -4.5 are clipped, x = 5.75 gives 9.5."""
    eps, clip = 2.0 ** -10, 10.0
    mean = np.array([1.0, 0.0, -3.0])
    var = np.array([0.25 - eps, 1.0 - eps, 4.0 - eps])
    x = np.array([[6.0, 10.0, 17.0], [-4.0, -10.0, -23.0], [6.5, 10.5, 18.0], [-4.5, -11.0, -24.0], [5.75, 9.5, 16.0], [1.0, -0.0, -3.0],
                  [np.float32(1e-40), np.float32(-1e-40), 3.0e38]], np.float32)
    return x, mean, var, eps, clip


def compare(exe, tmp_path):
    rng = np.random.default_rng(5)
    for n in HOST_COUNTS:
        terms = rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, n)
        path = os.path.join(str(tmp_path), "terms.bin")
        terms.tofile(path)
        assert int(run_harness(exe, "sums", path, n)) == struct.unpack("<Q", struct.pack("<d", norm_sums(terms)))[0], n
    for n in (1, 65, 129, 2049):
        want = restate(n, WHOLE)
        got = harness_fold(exe, tmp_path, n, WHOLE)
        split = harness_fold(exe, tmp_path, n, SPLIT)
        for k in STATE:
            assert got[k].tobytes() == want[k].tobytes(), (n, k)
            assert split[k].tobytes() == want[k].tobytes() == restate(n, SPLIT)[k].tobytes(), (n, k)  # K steps in one call or in pieces
        assert want["observation_count"][0] == _abi.NORM_INITIAL_COUNT + 8 * n and want["ret_count"][0] == want["observation_count"][0]
    for switches in ((True, False), (False, True)):
        want = restate(65, WHOLE, norm_obs=switches[0], norm_reward=switches[1])
        got = harness_fold(exe, tmp_path, 65, WHOLE, *switches)
        start = norm_initial_state(65, OBS_DIM, GOAL_DIM)
        for k in STATE:
            assert got[k].tobytes() == want[k].tobytes(), (switches, k)
            off = not switches[1] if k.startswith("ret") or k == "running_ret" else not switches[0]  # a switched-off group is left alone
            assert (got[k].tobytes() == start[k].tobytes()) == off, (switches, k)
    # normalize: the folded statistics on the ring's own rows, infinite clips and eps = 0; then the clip edges
    st, r = restate(129, WHOLE), ring(129)
    for g in NORM_ROW_GROUPS:
        x = r[g].reshape(-1, r[g].shape[-1])
        for eps, clip in ((1e-8, 10.0), (0.0, np.inf), (1e-8, 0.5)):
            got = harness_apply(exe, tmp_path, x, st[g + "_mean"], st[g + "_var"], eps, clip)
            assert got.tobytes() == normalize_rows(x, st[g + "_mean"], st[g + "_var"], eps, clip).tobytes(), (g, eps, clip)
    for eps, clip in ((1e-8, 10.0), (0.0, np.inf), (1e-8, 0.01)):
        rew = r["reward"].reshape(-1, 1)
        got = harness_apply(exe, tmp_path, rew, [0.0], st["ret_var"], eps, clip, reward=True)
        assert got.tobytes() == normalize_reward(rew, st["ret_var"], eps, clip).tobytes(), (eps, clip)
    x, mean, var, eps, clip = clip_cases()
    got = harness_apply(exe, tmp_path, x, mean, var, eps, clip)
    assert got.tobytes() == normalize_rows(x, mean, var, eps, clip).tobytes()
    assert np.array_equal(got[0], [10.0] * 3) and np.array_equal(got[1], [-10.0] * 3) and np.array_equal(got[2], [10.0] * 3) and np.array_equal(got[3], [-10.0] * 3)
    assert np.array_equal(got[4], [9.5, 9.5, 9.5]) and np.array_equal(got[5], [0.0, 0.0, 0.0]) and got[6, 2] == 10.0
    assert got[6, 0] == -2.0 and got[6, 1] == np.float32(-1e-40)  # a subnormal: (x - 1) * 2, and x * 1 back to the same subnormal


def test_harness_equals_the_restatements_bitwise(harness, tmp_path):
    compare(harness, tmp_path)


def test_harness_is_clean_under_address_and_undefined_sanitizers(sanitized_harness, tmp_path):
    compare(sanitized_harness, tmp_path)


def test_inv_is_one_division_of_one_square_root():
    x, mean, var, eps, clip = clip_cases()
    inv = 1.0 / np.sqrt(var + eps)
    assert np.array_equal(inv, [2.0, 1.0, 0.5])  # exact: the clip cases rest on it
    assert np.array_equal(normalize_rows(x[:1], mean, var, eps, np.inf), ((x[:1].astype(np.float64) - mean) * inv).astype(np.float32))


@pytest.mark.parametrize("n", (1, 63, 129, 1025, 2049))
def test_restatement_against_exact_arithmetic(n):
    """One slot folded from the initial state and a second one from what the first left, each against exact rational arithmetic on the
    same float64 inputs, within the bound norm_cases derives (gamma_D over the chain length and the fold levels for S1 and S2, then
    the merge's operations one by one).  Nothing in the bound is measured."""
    r = ring(n)
    state, worst = norm_initial_state(n, OBS_DIM, GOAL_DIM), {}
    for slot in (0, 1):
        after = norm_fold(state, r, slot, 1, GAMMA)
        groups = [(g, r[g][slot].astype(np.float64)) for g in NORM_ROW_GROUPS]
        running = state["running_ret"] * np.float64(GAMMA) + r["reward"][slot].astype(np.float64)  # two operations on given inputs, taken as given
        groups.append(("ret", running.reshape(n, 1)))
        for g, x in groups:
            for j in range(x.shape[1]):
                terms = [Fraction(float(v)) for v in x[:, j]]
                s1, s2 = bounded_sum(terms, n), bounded_sum([t * t for t in terms], n, extra=int(g == "ret"))  # float64 squares round once
                got1, got2 = norm_sums(x[:, j]), norm_sums(x[:, j] * x[:, j])
                assert abs(Fraction(float(got1)) - s1.v) <= s1.e and abs(Fraction(float(got2)) - s2.v) <= s2.e, (n, g, j)
                mean, var = bounded_merge(state[g + "_mean"][j], state[g + "_var"][j], state[g + "_count"][0], s1, s2, n)
                for name, b, got in (("mean", mean, after[g + "_mean"][j]), ("var", var, after[g + "_var"][j])):
                    err = abs(Fraction(float(got)) - b.v)
                    assert err <= b.e, (n, slot, g, j, name, float(err), float(b.e))
                    if b.e:
                        worst[name] = max(worst.get(name, 0.0), float(err / b.e))
            assert after[g + "_count"][0] == state[g + "_count"][0] + n  # exact here: 1e-4 + n rounds once, 2 n is then added exactly or rounds once
        state = after
    print(f"n = {n}: D = {sum_depth(n)}, largest error / bound: {worst}")


@pytest.mark.parametrize("n", (1, 63, 129, 1025, 2049))
def test_restatement_against_a_literal_running_mean_std(n):
    """SB3's RunningMeanStd.update written out in float64 (np.mean, np.var, the merge) against the restatement, slot after slot, each
    merge of both sides from the SAME state (the restatement's): the bound is twice the exact-arithmetic bound of that merge, since
    both sides round."""
    r = ring(n)
    state = norm_initial_state(n, OBS_DIM, GOAL_DIM)
    worst = 0.0
    for slot in (2, 3, 0):
        after = norm_fold(state, r, slot, 1, GAMMA)
        for g in NORM_ROW_GROUPS:
            x = r[g][slot].astype(np.float64)
            lit = literal_running_mean_std(state[g + "_mean"], state[g + "_var"], state[g + "_count"][0], x)
            for j in range(x.shape[1]):
                terms = [Fraction(float(v)) for v in x[:, j]]
                mean, var = bounded_merge(state[g + "_mean"][j], state[g + "_var"][j], state[g + "_count"][0], bounded_sum(terms, n),
                                          bounded_sum([t * t for t in terms], n), n)
                for name, b, got, want in (("mean", mean, after[g + "_mean"][j], lit[0][j]), ("var", var, after[g + "_var"][j], lit[1][j])):
                    dev = abs(Fraction(float(got)) - Fraction(float(want)))
                    assert dev <= 2 * b.e, (n, slot, g, j, name, float(dev), float(b.e))
                    worst = max(worst, float(dev))
        state = after
    print(f"n = {n}: largest deviation from the literal RunningMeanStd {worst:.3e}")


def test_cases_say_what_their_comments_say():
    r = ring(129)
    obs = r["observation"].astype(np.float64)
    assert np.all(obs[:, :, 0] == 0.25) and abs(obs[:, :, 1].mean() - 1.0) < 1e-4 and 0.3e-8 < obs[:, :, 1].var() < 3e-8
    sub = r["observation"][:, :, 2]
    assert np.all(np.abs(sub) < np.finfo(np.float32).tiny) and (sub > 0).any() and (sub < 0).any()
    assert np.signbit(r["observation"][:, :, 4]).any() and not np.signbit(r["observation"][:, :, 4]).all() and np.all(r["observation"][:, :, 4] == 0)
    assert (r["reward"] == -500).any() and (r["reward"] == 200).any() and r["terminated"][0, 0] and r["truncated"][0, 0]
    st = restate(129, WHOLE)
    assert 0.0 <= st["observation_var"][0] < 1e-3 and st["observation_var"][4] < 1e-3  # zero-variance features: var shrinks from 1 towards 0, never negative
    assert np.all(st["observation_var"] >= 0) and st["ret_var"][0] > 100.0
    assert np.all(st["running_ret"][(r["terminated"][3] | r["truncated"][3]) != 0] == 0.0)


def test_restatements_refuse_what_they_cannot_state():
    n = 5
    st, r = norm_initial_state(n, OBS_DIM, GOAL_DIM), ring(n)
    for bad in ((dict(st, ret_mean=st["ret_mean"].astype(np.float32)), r, 0, 1), ({k: v for k, v in st.items() if k != "ret_var"}, r, 0, 1),
                (st, dict(r, reward=r["reward"].astype(np.float64)), 0, 1), (st, dict(r, terminated=r["terminated"].astype(np.int32)), 0, 1),
                (st, dict(r, observation=r["observation"][:, :, :5]), 0, 1), (st, r, CAP, 1), (st, r, -1, 1), (st, r, 0, 0), (st, r, 0, CAP + 1),
                (dict(st, running_ret=st["running_ret"][:4]), r, 0, 1)):
        with pytest.raises(ValueError):
            norm_fold(*bad, GAMMA)
    before = {k: v.copy() for k, v in st.items()}
    norm_fold(st, r, 0, 4, GAMMA)
    assert all(np.array_equal(st[k], before[k]) for k in st)  # the arguments are not written
    with pytest.raises(ValueError):
        normalize_rows(np.zeros((2, 3)), np.zeros(3), np.ones(3), 0.0, 1.0)
    with pytest.raises(ValueError):
        norm_sums(np.zeros(3, np.float32))
    m, v, c = norm_merge(np.zeros(2), np.ones(2), 1e-4, np.array([3.0, 6.0]), np.array([3.0, 12.0]), 3)
    assert c == 1e-4 + 3 and np.allclose(m, [1.0, 2.0], atol=1e-4) and np.allclose(v, [0.0, 0.0], atol=1e-3)


def test_structs_mirror_the_header(harness):
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    layout = json.loads(run_harness(harness, "layout"))
    mirrors = (("urgym_norm_state", _abi.NormState), ("urgym_normalization", _abi.Normalization), ("urgym_norm_rows_args", _abi.NormRowsArgs))
    assert set(layout) == {name for name, _ in mirrors}
    for name, mirror in mirrors:
        body = hdr[hdr.index(f"typedef struct {name} {{"):hdr.index(f"}} {name};")]
        declared = re.findall(r"^\s*(?:const\s+)?\w+\*?\s+(\w+);", body, flags=re.M)
        assert declared == [f for f, _ in mirror._fields_], name  # the header's order is the mirror's
        want = layout[name]
        assert C.sizeof(mirror) == want.pop("sizeof"), name
        assert {f: getattr(mirror, f).offset for f, _ in mirror._fields_} == want, name  # the C compiler's own offsets
    assert [name for name, _ in _abi.NormState._fields_] == STATE and dict(_abi.Normalization._fields_)["state"] is _abi.NormState
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    lib = _native.lib()
    for sym in ("urgym_norm_workspace", "urgym_norm_fold", "urgym_norm_rows", "urgym_norm_batch", "urgym_norm_snapshot", "urgym_rollout_collect_normalized",
                "urgym_policy_evaluate_normalized", "urgym_sac_train_normalized"):
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    assert lib.urgym_abi_version() == 4
    # the header states the order of the sums, every line of the merge and of the normalization
    for text in ("chain q = 0..3 starts at +0.0 and adds rows 128 b + q", "slab = (chain0 + chain1) + (chain2 + chain3)", "part c = 0..15 starts at +0.0 and adds slabs c, c + 16",
                 "part[c] += part[c + s] for s = 8, 4, 2, 1", "bm = S1 / n;  bv = max(S2 / n - bm * bm, 0.0)", "delta = bm - mean", "tot   = count + n",
                 "mean' = mean + (delta * n) / tot", "M2    = (var * count + bv * n) + ((delta * delta) * count) * n / tot", "var'  = M2 / tot",
                 "running_ret = running_ret * gamma + (double)reward", "running_ret = +0.0 where terminated | truncated", "inv_j = 1.0 / sqrt(var_j + eps)",
                 "(float)min(max(((double)x - mean_j) * inv_j, -clip_obs), clip_obs)", "(float)min(max((double)r * inv_ret, -clip_reward), clip_reward)",
                 "Non-finite inputs are out of scope"):
        assert text in hdr, text
    src = open(os.path.join(CSRC, "urgym_norm.h")).read()
    assert (_abi.NORM_SLAB_ROWS, _abi.NORM_CHAINS, _abi.NORM_PARTS) == tuple(int(re.search(rf"constexpr int {k} = (\d+);", src).group(1))
                                                                              for k in ("NORM_SLAB_ROWS", "NORM_CHAINS", "NORM_PARTS"))


def test_option_refusals(harness):
    refusal = lambda *a: json.loads(run_harness(harness, "refusal", *a))  # noqa: E731
    assert refusal(0.95, 1e-8, 10, 10, 0) is None and refusal(0, 0, "inf", "inf", 0) is None and refusal(1, 0, 1e-300, 1, 0) is None
    for args, word in (((1.5, 0, 1, 1, 0), "gamma"), ((-0.1, 0, 1, 1, 0), "gamma"), (("nan", 0, 1, 1, 0), "gamma"), ((0.9, -1e-9, 1, 1, 0), "eps"), ((0.9, "inf", 1, 1, 0), "eps"),
                       ((0.9, 0, 0, 1, 0), "clip_obs"), ((0.9, 0, -1, 1, 0), "clip_obs"), ((0.9, 0, "nan", 1, 0), "clip_obs"), ((0.9, 0, 1, 0, 0), "clip_reward"),
                       ((0.9, 0, 1, 1, 7), "reserved0")):
        assert word in refusal(*args), (args, word)
    ok = dict(gamma=0.95, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, epsilon=1e-8)
    assert DeviceNormalizer.check_options(**ok) == ok and DeviceNormalizer.check_options(**dict(ok, clip_obs=np.inf, epsilon=0))["clip_obs"] == np.inf
    for bad in (dict(gamma=1.5), dict(gamma=True), dict(norm_obs=1), dict(norm_reward="yes"), dict(clip_obs=0.0), dict(clip_reward=-1.0), dict(clip_obs=np.nan),
                dict(epsilon=-1e-9), dict(epsilon=np.inf), dict(epsilon=None)):
        with pytest.raises(ValueError):
            DeviceNormalizer.check_options(**dict(ok, **bad))


def test_refusals_that_need_no_device():
    lib = _native.lib()
    n = C.c_uint64(0)
    assert lib.urgym_norm_workspace(None, 1, C.byref(n)) == _abi.ERR_ARG
    assert lib.urgym_norm_fold(None, C.byref(_abi.Normalization()), C.byref(_abi.ReplayRing()), 0, 1, None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert lib.urgym_norm_fold(None, None, None, 0, 0, None) == _abi.ERR_ARG
    assert lib.urgym_norm_rows(None, C.byref(_abi.Normalization()), C.byref(_abi.NormRowsArgs()), 1, None) == _abi.ERR_ARG
    assert lib.urgym_norm_batch(None, C.byref(_abi.Normalization()), C.byref(_abi.ReplayBatch()), 1, None) == _abi.ERR_ARG
    assert lib.urgym_rollout_collect_normalized(None, None, None, 1, None, 0, None, None) == _abi.ERR_ARG
    assert lib.urgym_norm_snapshot(None, C.byref(_abi.NormState()), C.byref(_abi.NormState()), None, None) == _abi.ERR_ARG
    assert lib.urgym_policy_evaluate_normalized(None, C.byref(_abi.PolicyEvaluation()), C.byref(_abi.Normalization()), 0, 0, None) == _abi.ERR_ARG
    assert lib.urgym_sac_train_normalized(None, C.byref(_abi.SacLearner()), C.byref(_abi.SacSchedule()), C.byref(_abi.Normalization()), None, None, None, None, None, None,
                                          None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)


def test_learner_option_is_kept_apart_and_refused_without_the_device_route():
    from ur_gym_amd import training

    assert training.NORM_DEFAULTS == dict(normalize=False, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, norm_epsilon=1e-8)
    assert not set(training.NORM_DEFAULTS) & (set(training.SAC_DEFAULTS) | set(training.PER_DEFAULTS) | set(training.HER_DEFAULTS) | set(training.CLIP_DEFAULTS))
    with pytest.raises(ValueError, match="device_entropy"):
        training.SACLearner(None, normalize=True)
    for bad in (dict(normalize=1), dict(normalize=True, device_entropy=True, clip_obs=0.0), dict(normalize=True, device_entropy=True, norm_epsilon=-1.0),
                dict(normalize=True, device_entropy=True, norm_obs="no")):
        with pytest.raises(ValueError):
            training.SACLearner(None, **bad)
    # the checkpoint key rule: the options are saved only where normalize=True
    plain = type("L", (), dict(hp=dict(training.SAC_DEFAULTS, **training.PER_DEFAULTS, **training.HER_DEFAULTS, **training.CLIP_DEFAULTS, **training.NORM_DEFAULTS)))()
    saved = training.SACLearner._saved_hp(plain)
    assert not set(training.NORM_DEFAULTS) & set(saved)
    plain.hp["normalize"] = True
    assert set(training.NORM_DEFAULTS) <= set(training.SACLearner._saved_hp(plain))
