"""CPU tests (-m "not gpu") of the plan statistics and of the planner inside the training call.

  * tests/mppi_stats_harness.cpp, a stand-alone host program around ur_gym_amd/csrc/urgym_mppi_stats.h -- the header the kernel of
    urgym_mppi_stats.hip compiles -- equals evaluation.mppi_plan_stats bitwise; built a second time with -fsanitize=address,undefined
    and run as that program.
  * evaluation.mppi_plan_stats against exact rational arithmetic on integer-valued inputs: every sum is exact there, so every mean is
    the correctly rounded quotient and nothing else.
  * the ctypes mirrors of the two new structs against the C compiler's own layout, the two new symbols, the row of the dispatch table,
    and the refusals that need no device.
  * where the plan-statistics records of split calls fall.
"""
import ctypes as C
import json
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from mppi_train_cases import (FLOATS, HOST_COUNTS, plain, plan_buffers, plan_record_slots, poisoned, record_of, same_record, small_integers,
                              unplanned_buffers)
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import monitor_points, mppi_plan_stats, mppi_stats_record_bytes
from ur_gym_amd.vector_env import _sac_train_entry

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "mppi_stats_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h")] + [os.path.join(CSRC, h) for h in ("urgym_mppi_stats.h", "urgym_mppi.h", "urgym_sac_terms.h",
                                                                                            "urgym_adam.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("mppi_stats_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("mppi_stats_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def harness_record(exe, tmp_path, buffers, iteration):
    E, adaptive = buffers["best_return"].shape[0], "elite_count" in buffers
    order = ("best_return", "nominal_return", "ess") + (("elite_count", "threshold") if adaptive else ())
    src, dst = os.path.join(str(tmp_path), "in.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as f:
        f.write(b"".join(np.ascontiguousarray(buffers[k]).tobytes() for k in order))
    run = subprocess.run([exe, "stats", src, dst, str(E), str(int(adaptive)), str(iteration)], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (E, adaptive, run.returncode, run.stderr[-2000:])
    raw = open(dst, "rb").read()
    assert len(raw) == C.sizeof(_abi.MppiStatsRecord)
    return record_of(raw)


def compare_all(exe, tmp_path):
    for E in HOST_COUNTS:
        for make in (plan_buffers, unplanned_buffers, small_integers):
            full = make(E)
            for buffers in (full, plain(full)):
                want = mppi_plan_stats(**buffers, iteration=-3 - E)
                got = harness_record(exe, tmp_path, buffers, -3 - E)
                same_record(got, want)
                assert got["iteration"] == -3 - E and got["num_parents"] == E and got["reserved0"] == 0


def test_harness_equals_the_restatement_bitwise(harness, tmp_path):
    compare_all(harness, tmp_path)


def test_harness_is_clean_under_address_and_undefined_sanitizers(sanitized_harness, tmp_path):
    compare_all(sanitized_harness, tmp_path)


@pytest.mark.parametrize("E", HOST_COUNTS)
def test_cases_say_what_their_names_say(E):
    b, at = plan_buffers(E), poisoned(E)
    rec = mppi_plan_stats(**b)
    fin = lambda x: np.isfinite(x)  # noqa: E731
    assert b["best_return"][at["best_ninf"]] == -np.inf and np.isnan(b["nominal_return"][at["nominal_nan"]]) and np.isnan(b["ess"][at["ess_nan"]])
    assert rec["planned"] == int(fin(b["best_return"]).sum()) == E - 1
    assert rec["nominal_finite"] == int(fin(b["nominal_return"]).sum()) < E
    assert rec["gain_count"] == int((fin(b["best_return"]) & fin(b["nominal_return"])).sum())
    assert rec["threshold_count"] == int(fin(b["threshold"]).sum()) == E - 1
    # the NaN ess reaches the mean and nothing else; the minimum passes it over (with one parent there is no other operand)
    assert np.isnan(rec["mean_ess"])
    assert all(np.isfinite(rec[k]) for k in FLOATS if k not in ("mean_ess", "min_ess"))
    others = np.delete(b["ess"], at["ess_nan"])
    assert (np.isnan(rec["min_ess"]) and E == 1) or rec["min_ess"] == others.min()
    # every parent unplanned: the means of the returns, of the gain and of the threshold are +0.0, their counts 0; ess is the nominal's
    un = mppi_plan_stats(**unplanned_buffers(E))
    for k in ("mean_best_return", "mean_nominal_return", "mean_gain", "mean_elite_count", "mean_threshold"):
        assert np.float64(un[k]).tobytes() == np.float64(0.0).tobytes(), k
    assert un["planned"] == un["nominal_finite"] == un["gain_count"] == un["threshold_count"] == 0 and un["mean_ess"] == un["min_ess"] == 1.0
    # without the adapt fields the three are zero and the rest is unchanged
    without = mppi_plan_stats(**plain(b))
    assert without["mean_elite_count"] == without["mean_threshold"] == 0.0 and without["threshold_count"] == 0
    same_record({**without, **{k: rec[k] for k in ("mean_elite_count", "mean_threshold", "threshold_count")}}, rec)


@pytest.mark.parametrize("E", HOST_COUNTS)
def test_restatement_against_exact_arithmetic(E):
    """Integer-valued inputs below 2^10 in magnitude: every partial sum of at most 65,536 of them is an integer below 2^53, hence exact
    in float64 whatever the order, and a mean is then the one correctly rounded division -- which int / int is in Python."""
    b = small_integers(E)
    rec = mppi_plan_stats(**b)
    fb, fn, ft = np.isfinite(b["best_return"]), np.isfinite(b["nominal_return"]), np.isfinite(b["threshold"])

    def exact(values, mask):
        total, count = sum(Fraction(float(v)) for v in values[mask]), int(mask.sum())
        assert total.denominator == 1
        return (int(total) / count if count else 0.0), count

    both = fb & fn
    for name, count_name, (want, count) in (("mean_best_return", "planned", exact(b["best_return"], fb)),
                                            ("mean_nominal_return", "nominal_finite", exact(b["nominal_return"], fn)),
                                            ("mean_gain", "gain_count", exact(np.where(both, b["best_return"] - b["nominal_return"], 0.0), both)),
                                            ("mean_threshold", "threshold_count", exact(b["threshold"], ft)),
                                            ("mean_ess", "num_parents", exact(b["ess"], np.ones(E, bool))),
                                            ("mean_elite_count", "num_parents", exact(b["elite_count"].astype(np.float64), np.ones(E, bool)))):
        assert rec[name] == want and rec[count_name] == count, (name, rec[name], want)
    assert rec["min_ess"] == b["ess"].min()


def test_restatement_refuses_what_it_cannot_state():
    b = plan_buffers(5)
    for bad in (dict(b, ess=b["ess"].astype(np.float32)), dict(b, best_return=b["best_return"][:4]), dict(plain(b), elite_count=b["elite_count"]),
                dict(b, elite_count=b["elite_count"].astype(np.int64)), dict(b, threshold=b["threshold"][:3]),
                {k: v[:0] for k, v in b.items()}):
        with pytest.raises(ValueError):
            mppi_plan_stats(**bad)
    rec = mppi_plan_stats(**b, iteration=9)
    assert record_of(mppi_stats_record_bytes(rec))["iteration"] == 9


def test_structs_mirror_the_header(harness):
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    layout = json.loads(subprocess.run([harness, "layout"], capture_output=True, text=True, check=True).stdout)
    mirrors = (("urgym_mppi_stats_record", _abi.MppiStatsRecord), ("urgym_sac_planning", _abi.SacPlanning))
    assert set(layout) == {name for name, _ in mirrors}
    for name, mirror in mirrors:
        body = hdr[hdr.index(f"typedef struct {name} {{"):hdr.index(f"}} {name};")]
        declared = re.findall(r"^\s*(?:const\s+)?\w+\*?\s+(\w+);", body, flags=re.M)
        assert declared == [f for f, _ in mirror._fields_], name  # the header's order is the mirror's
        want = layout[name]
        assert C.sizeof(mirror) == want.pop("sizeof"), name
        assert {f: getattr(mirror, f).offset for f, _ in mirror._fields_} == want, name  # the C compiler's own offsets
    assert C.sizeof(_abi.MppiStatsRecord) == 8 * _abi.MPPI_STATS_RECORD_WORDS == 88 and C.alignment(_abi.MppiStatsRecord) == 8
    assert C.sizeof(_abi.SacPlanning) % 8 == 0 and dict(_abi.SacPlanning._fields_)["explore"] is _abi.MppiExplore
    assert _abi.MPPI_STATS_MAX_PARENTS == _abi.SAC_TRAIN_MAX_COUNT == 65536
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4


def test_symbols_and_the_dispatch_row():
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    lib = _native.lib()
    for sym in ("urgym_mppi_stats", "urgym_sac_train_planned"):
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    assert lib.urgym_abi_version() == _abi.ABI_VERSION == 4  # found by lookup, within the version
    # a planner picks urgym_sac_train_planned whatever else is given, and its option tuple lines up with the declared signature
    structs = {"planner": _abi.SacPlanning, "clipping": _abi.SacClipping, "nstep": _abi.SacNstep, "prioritized": _abi.SacPrioritized,
               "hindsight": _abi.SacHindsight, "evaluation": _abi.SacEvaluation, "monitor": _abi.SacMonitoring}
    for present in ({"planner"}, {"planner", "clipping", "monitor"}, {"planner", "evaluation", "hindsight"}, {"planner", "nstep"}, {"planner", "prioritized"}):
        symbol, options = _sac_train_entry(present)
        assert symbol == "urgym_sac_train_planned" and present <= set(options)
    argtypes = lib.urgym_sac_train_planned.argtypes
    assert len(options) + 4 == len(argtypes) and "normalizer" not in options  # there is no normalization argument
    assert argtypes[1] is C.POINTER(_abi.SacLearner) and argtypes[2] is C.POINTER(_abi.SacSchedule)
    for position, option in enumerate(options):
        assert argtypes[3 + position] is C.POINTER(structs[option]), (position, option)
    # without a planner the table names what it named before
    assert _sac_train_entry({"clipping", "monitor"})[0] == "urgym_sac_train_clipped" and _sac_train_entry(set())[0] == "urgym_sac_train"


def test_refusals_that_need_no_device():
    lib = _native.lib()
    # a NULL handle is refused before anything else is looked at
    assert lib.urgym_mppi_stats(None, C.byref(_abi.Mppi()), None, C.byref(_abi.MppiStatsRecord()), 0, None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert lib.urgym_mppi_stats(None, None, None, None, 0, None) == _abi.ERR_ARG
    fn = lib.urgym_sac_train_planned
    assert fn(None, *[C.byref(t._type_()) for t in fn.argtypes[1:-1]], None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert fn(*[None] * len(fn.argtypes)) == _abi.ERR_ARG


@pytest.mark.parametrize("log_every", (1, 2, 3))
def test_plan_records_of_split_calls_fall_where_one_call_puts_them(log_every):
    """Planner record r sits where evaluation.monitor_points puts monitor record r: the slot is the monitor's own index and the tag the
    monitor's iteration count, so calls of a and b iterations that hand both counters on place the records of one call of a + b."""
    for a, b in ((2, 2), (1, 4), (3, 3), (5, 0)):
        whole = plan_record_slots(0, 0, a + b, log_every)
        first = plan_record_slots(0, 0, a, log_every)
        second = plan_record_slots(a, len(first), b, log_every)
        assert first + second == whole
        assert [slot for slot, _ in whole] == list(range(len(monitor_points(0, a + b, log_every))))
        assert [tag for _, tag in whole] == [i + 1 for i in monitor_points(0, a + b, log_every)]
        assert all(tag % log_every == 0 for _, tag in whole)
