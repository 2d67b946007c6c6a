"""CPU tests (-m "not gpu") of the evaluation inside the training call.

  * tests/eval_harness.cpp, a stand-alone host program around ur_gym_amd/csrc/urgym_eval.h and urgym_eval_schedule.h -- the headers the
    kernel and urgym_sac_train_evaluated compile -- equals evaluation.evaluation_stats bitwise and evaluation.evaluation_points exactly;
    built a second time with -fsanitize=address,undefined and run as that program.
  * evaluation.evaluation_stats against exact rational arithmetic, within bounds derived below from the number of rounded operations.
  * evaluation.evaluation_points against a plain simulation of the Python loop's rule.
  * the ctypes mirrors of the five new structs against the C compiler's own layout, the new symbols, the refusals that need no device,
    and the checkpoint round trip on the host.
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

from evaluation_cases import HOST_COUNTS, SCHEDULES, episodes, flag_cases, simulate_loop_rule
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import (ACTOR_ARRAYS, LOG_STD_ARRAYS, DeterministicActor, DeviceEvaluation, evaluation_points, evaluation_stats, ordered_sum,
                                   save_actor)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
FLOATS = ("mean_return", "var_return", "mean_length", "success_rate", "best_mean_after", "best_mean")
INTS = ("eval_index", "length_sum", "successes", "count", "improved", "reserved0", "best_index")
U = 2.0 ** -53


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "eval_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h")] + [os.path.join(CSRC, h) for h in ("urgym_eval.h", "urgym_eval_schedule.h", "urgym_sac_terms.h",
                                                                                            "urgym_sac_schedule.h", "urgym_adam.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("eval_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("eval_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run_harness(exe, *args):
    run = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (args, run.returncode, run.stdout[-500:], run.stderr[-2000:])
    return json.loads(run.stdout)


def word(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def harness_stats(exe, tmp_path, r, last, succ, best_mean, best_index, eval_index):
    path = os.path.join(str(tmp_path), "episodes.bin")
    with open(path, "wb") as f:
        f.write(r.tobytes() + last.tobytes() + succ.tobytes())
    return run_harness(exe, "stats", path, r.size, eval_index, word(best_mean), best_index)


def assert_bitwise(got, want, what):
    for k in FLOATS:
        assert got[k] == word(want[k]), (what, k, got[k], float(want[k]))
    for k in INTS:
        assert got[k] == want[k], (what, k, got[k], want[k])


def compare_stats(exe, tmp_path):
    for n in HOST_COUNTS:
        r, last, succ = episodes(n)
        assert n < 3 or (r.min() < -400 and r.max() > 1e3 and 0 < np.abs(r).min() < 1e-6), n  # signs and magnitudes are mixed
        want = evaluation_stats(r, last, succ, -np.inf, -1, 3)
        assert want["improved"] == 1 and want["best_index"] == 3 and want["length_sum"] == int(last.astype(np.int64).sum()) + n
        assert_bitwise(harness_stats(exe, tmp_path, r, last, succ, -np.inf, -1, 3), want, n)
        # against a best mean that is not beaten: the state stays
        want = evaluation_stats(r, last, succ, 1e300, 7, 4)
        assert want["improved"] == 0 and (want["best_mean"], want["best_index"]) == (1e300, 7)
        assert_bitwise(harness_stats(exe, tmp_path, r, last, succ, 1e300, 7, 4), want, n)
    for name, (r, best, improved) in flag_cases().items():
        r = np.ascontiguousarray(r, dtype=np.float64)
        last, succ = np.zeros(r.size, np.int32), np.ones(r.size, np.uint8)
        want = evaluation_stats(r, last, succ, best, 5, 9)
        got = harness_stats(exe, tmp_path, r, last, succ, best, 5, 9)
        assert want["improved"] == improved == got["improved"], name
        if not improved:  # the best state is unchanged, bit for bit
            assert (got["best_mean"], got["best_index"]) == (word(best), 5) and got["best_mean_after"] == word(best), name
        else:
            assert (got["best_mean"], got["best_index"]) == (got["mean_return"], 9), name
        assert_bitwise(got, want, name)
        if "NaN" in name:
            assert np.isnan(want["mean_return"]), name
        if "-inf" in name.split("against")[0]:
            assert want["mean_return"] == -np.inf, name


def compare_points(exe):
    for case in SCHEDULES:
        first, n, G, idle, E = case
        want = evaluation_points(first, n, G, idle, E)
        got = run_harness(exe, "points", first, n, G, idle, E, 0, max(1, len(want)))
        assert got["points"] == want and got["count"] == len(want) and got["refused"] is None, (case, got, want)
        if want:  # one record too few is refused, and so is a start slot that leaves one too few
            assert "record_capacity" in run_harness(exe, "points", first, n, G, idle, E, 0, len(want) - 1)["refused"], case
            assert "record_capacity" in run_harness(exe, "points", first, n, G, idle, E, 3, len(want) + 2)["refused"], case
        assert run_harness(exe, "points", first, n, G, idle, E, 3, len(want) + 3)["refused"] is None, case
    assert "every" in run_harness(exe, "points", 1, 4, 1, 0, 0, 0, 8)["refused"]
    assert "every" in run_harness(exe, "points", 1, 4, 1, 0, -2, 0, 8)["refused"]
    assert "first_record_slot" in run_harness(exe, "points", 1, 4, 1, 0, 1, -1, 8)["refused"]


def test_harness_equals_the_restatement_bitwise(harness, tmp_path):
    compare_stats(harness, tmp_path)
    compare_points(harness)


def test_harness_is_clean_under_address_and_undefined_sanitizers(sanitized_harness, tmp_path):
    compare_stats(sanitized_harness, tmp_path)
    compare_points(sanitized_harness)


def test_schedule_cases_say_what_their_names_say():
    assert evaluation_points(1, 6, 2, 1, 4) == [2, 4]
    assert evaluation_points(1, 6, 3, 0, 1) == list(range(6))
    assert evaluation_points(1, 6, 3, 2, 3) == [2, 3, 4, 5]
    assert evaluation_points(1, 5, 3, 0, 100) == evaluation_points(1, 5, 0, 0, 1) == evaluation_points(1, 5, 1, 5, 1) == []
    assert evaluation_points(8, 4, 1, 0, 4) == [0] and evaluation_points(9, 4, 1, 0, 4) == [3]
    assert evaluation_points(4, 3, 3, 1, 4) == [1, 2]
    for bad in ((0, 1, 1, 0, 1), (1, 0, 1, 0, 1), (1, 1, -1, 0, 1), (1, 1, 1, -1, 1), (1, 1, 1, 0, 0)):
        with pytest.raises(ValueError):
            evaluation_points(*bad)


@pytest.mark.parametrize("case", SCHEDULES)
def test_points_equal_a_simulation_of_the_python_loop_rule(case):
    assert evaluation_points(*case) == simulate_loop_rule(*case), case


@pytest.mark.parametrize("n", HOST_COUNTS)
def test_restatement_against_exact_arithmetic(n):
    """Both bounds are derived, not measured, with u = 2^-53 (n^2 u << 1 up to 65536, so the first-order bounds hold with the slack
    they carry).  The mean: a sum of n terms in ANY order is within (n - 1) u sum|r| of the exact one, the division adds a relative u:
    (n + 1) u sum|r| / n covers both.  The variance about the COMPUTED mean: each term d * d carries three roundings (the difference,
    which enters squared, and the product), the sum of n non-negative terms (n - 1) more, relative, and the division one:
    (n + 3) u, below the (n + 8) u asserted."""
    r, last, succ = episodes(n, seed=1)
    got = evaluation_stats(r, last, succ, -np.inf, -1, 0)
    exact = [Fraction(float(x)) for x in r]
    exact_mean = sum(exact) / n
    mean = Fraction(float(got["mean_return"]))
    assert abs(mean - exact_mean) <= (n + 1) * Fraction(U) * sum(abs(x) for x in exact) / n
    exact_var = sum((x - mean) ** 2 for x in exact) / n  # about the computed mean
    assert abs(Fraction(float(got["var_return"])) - exact_var) <= (n + 8) * Fraction(U) * exact_var
    assert got["mean_length"] == (int(last.astype(np.int64).sum()) + n) / n and got["success_rate"] == int(succ.sum()) / n  # one rounding each
    assert got["std_return"] == np.sqrt(got["var_return"])


def test_restatement_refuses_what_it_cannot_state():
    r, last, succ = episodes(5)
    for bad in ((r.astype(np.float32), last, succ), (r, last.astype(np.int64), succ), (r, last, succ.astype(np.int32)), (r[:0], last[:0], succ[:0]),
                (r, last[:4], succ), (r.reshape(1, 5), last, succ)):
        with pytest.raises(ValueError):
            evaluation_stats(*bad, -np.inf, -1, 0)
    evaluation_stats(r, last, succ.astype(bool), -np.inf, -1, 0)  # the rollout's bool views are taken
    assert ordered_sum(r, np.float64) == ordered_sum(r, dtype=np.float64)
    with pytest.raises(ValueError):
        ordered_sum(r)  # float32 unless asked
    with pytest.raises(ValueError):
        ordered_sum(r.astype(np.float32), np.float64)


def test_structs_mirror_the_header(harness):
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    layout = run_harness(harness, "layout")
    mirrors = (("urgym_eval_record", _abi.EvalRecord), ("urgym_eval_stats_args", _abi.EvalStatsArgs), ("urgym_actor_snapshot_args", _abi.ActorSnapshotArgs),
               ("urgym_policy_evaluation", _abi.PolicyEvaluation), ("urgym_sac_evaluation", _abi.SacEvaluation))
    assert set(layout) == {name for name, _ in mirrors}
    for name, mirror in mirrors:
        body = hdr[hdr.index(f"typedef struct {name} {{"):hdr.index(f"}} {name};")]
        declared = re.findall(r"^\s*(?:const\s+)?\w+\*?\s+(\w+);", body, flags=re.M)
        assert declared == [f for f, _ in mirror._fields_], name  # the header's order is the mirror's
        want = layout[name]
        assert C.sizeof(mirror) == want.pop("sizeof"), name
        assert {f: getattr(mirror, f).offset for f, _ in mirror._fields_} == want, name  # the C compiler's own offsets
    assert C.sizeof(_abi.EvalRecord) == 8 * _abi.EVAL_RECORD_WORDS and C.alignment(_abi.EvalRecord) == 8
    assert dict(_abi.SacEvaluation._fields_)["evaluation"] is _abi.PolicyEvaluation
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    lib = _native.lib()
    for sym in ("urgym_eval_stats", "urgym_actor_snapshot", "urgym_policy_evaluate", "urgym_sac_train_evaluated"):
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    assert lib.urgym_abi_version() == 4
    # the header states every float of the statistics, the sequence and the quirk that is not reproduced
    for text in ("mean         = sum_r / (double)N", "d            = r[n] - mean;  term = d * d", "var          = sum_d2 / (double)N",
                 "mean_length  = (double)len_sum / (double)N", "success_rate = (double)successes / (double)N", "improved     = mean > best_mean",
                 "NOT E[r^2] - mean^2", "sqrt(var_return) on the host", "when = &records[record_slot].improved", "eval_handle == handle is refused",
                 "floor(s_i / E) > floor(s_{i-1} / E)"):
        assert text in hdr, text


def test_refusals_that_need_no_device():
    lib = _native.lib()
    # a NULL handle is refused before anything else is looked at
    assert lib.urgym_eval_stats(None, C.byref(_abi.EvalStatsArgs()), None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert lib.urgym_eval_stats(None, None, None) == _abi.ERR_ARG
    assert lib.urgym_actor_snapshot(None, C.byref(_abi.ActorSnapshotArgs()), None) == _abi.ERR_ARG
    assert lib.urgym_actor_snapshot(None, None, None) == _abi.ERR_ARG
    assert lib.urgym_policy_evaluate(None, C.byref(_abi.PolicyEvaluation()), 0, 0, None) == _abi.ERR_ARG
    assert lib.urgym_policy_evaluate(None, None, 0, 0, None) == _abi.ERR_ARG
    assert lib.urgym_sac_train_evaluated(None, C.byref(_abi.SacLearner()), C.byref(_abi.SacSchedule()), C.byref(_abi.SacEvaluation()), None) == _abi.ERR_ARG
    assert lib.urgym_sac_train_evaluated(None, None, None, None, None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)


def test_save_best_round_trip_on_the_host(tmp_path):
    import torch

    rng = np.random.default_rng(3)
    n, H = 30, 32
    shapes = dict(zip(ACTOR_ARRAYS + LOG_STD_ARRAYS, ((H, n), (H,), (H, H), (H,), (6, H), (6,), (6, H), (6,))))
    arrays = {k: rng.standard_normal(sh).astype(np.float32) for k, sh in shapes.items()}
    arrays["mu_bias"][0], arrays["mu_bias"][1], arrays["mu_bias"][2] = np.float32(np.nan), np.float32(-0.0), np.float32(1e-45)  # bits, not values
    ev = object.__new__(DeviceEvaluation)  # the writer alone: no device, no environment
    ev.best = {k: torch.from_numpy(v.copy()) for k, v in arrays.items()}
    path = os.path.join(str(tmp_path), "best_model.npz")
    ev.save_best(path)
    assert os.path.exists(path)  # under the name given, no suffix appended
    back = DeterministicActor.load(path)
    assert sorted(back.w) == sorted(arrays) and back.in_features == n
    for k, v in arrays.items():
        assert back.w[k].dtype == np.float32 and back.w[k].shape == v.shape and back.w[k].tobytes() == v.tobytes(), k
    x = rng.standard_normal((4, n)).astype(np.float32)
    assert back(x[:, :6], x[:, 6:12], x[:, 12:]).shape == (4, 6)
    save_actor(path, arrays)  # arrays are taken as well as tensors
    assert all(np.load(path)[k].tobytes() == v.tobytes() for k, v in arrays.items())
