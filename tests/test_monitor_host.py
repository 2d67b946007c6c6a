"""CPU tests (-m "not gpu") of the training-episode statistics.

  * tests/monitor_harness.cpp, a stand-alone host program around ur_gym_amd/csrc/urgym_monitor.h -- the header the two kernels and
    urgym_sac_train_monitored compile -- equals evaluation.monitor_fold and evaluation.monitor_stats bitwise and evaluation.monitor_points
    exactly; built a second time with -fsanitize=address,undefined and run as that program.
  * evaluation.monitor_stats against exact rational arithmetic, within a bound derived below from the two summation stages.
  * evaluation.monitor_points against a plain simulation of a loop that counts its iterations.
  * the ctypes mirrors of the three new structs against the C compiler's own layout, the new symbols, and the refusals that need no
    device.
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

from monitor_cases import (AFTER_NAN_RECORD, CAP, EMPTY_RECORD, FLOATS, HOST_COUNTS, INTS, NAN_RECORD, PLACEMENTS, SCRIPT, SPLIT, WHOLE, restate, rings,
                           simulate_logging, zero_state)
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import monitor_fold, monitor_points, monitor_stats

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
U = 2.0 ** -53
STATE = [name for name, _ in _abi.MONITOR_STATE_FIELDS]


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "monitor_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h")] + [os.path.join(CSRC, h) for h in ("urgym_monitor.h", "urgym_sac_terms.h", "urgym_sac_schedule.h",
                                                                                            "urgym_adam.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("monitor_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("monitor_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run_harness(exe, *args):
    run = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (args, run.returncode, run.stdout[-500:], run.stderr[-2000:])
    return json.loads(run.stdout)


def word(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def harness_script(exe, tmp_path, n, script, state=None):
    """The harness over `script`: (records with floats as words, final state as arrays)."""
    tmp = str(tmp_path)
    state = zero_state(n) if state is None else state
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        f.write(b"".join(state[k].tobytes() for k in STATE))
    ops = []
    for op in script:
        if op[0] == "ring":
            path = os.path.join(tmp, f"ring_{op[1]}.bin")
            with open(path, "wb") as f:
                f.write(b"".join(np.ascontiguousarray(x).tobytes() for x in rings(n)[op[1]]))
            ops.append(f"ring:{path}")
        else:
            ops.append(f"{op[0]}:{op[1]}:{op[2]}")
    records = run_harness(exe, "run", os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin"), n, CAP, *ops)
    raw, out, at = open(os.path.join(tmp, "out.bin"), "rb").read(), {}, 0
    for name, ct in _abi.MONITOR_STATE_FIELDS:
        out[name] = np.frombuffer(raw, np.dtype(ct), n, at)
        at += n * C.sizeof(ct)
    assert at == len(raw)
    return records, out


def same_floats(a, b):
    """Bitwise, except that a NaN equals a NaN: its sign and payload are the adder's."""
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    return np.array_equal(a.view(np.uint64)[~np.isnan(a)], b.view(np.uint64)[~np.isnan(b)]) and np.array_equal(np.isnan(a), np.isnan(b))


def assert_same_state(got, want, what):
    for k in STATE:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        same = same_floats(got[k], want[k]) if got[k].dtype == np.float64 else np.array_equal(got[k], want[k])
        assert same, (what, k)


def compare_script(exe, tmp_path):
    for n in HOST_COUNTS:
        want, want_state = restate(n, SCRIPT)
        got, got_state = harness_script(exe, tmp_path, n, SCRIPT)
        assert len(got) == len(want) == 5
        for i, (g, w) in enumerate(zip(got, want)):
            for k in FLOATS:
                if i == NAN_RECORD and np.isnan(w[k]):
                    assert np.isnan(struct.unpack("<d", struct.pack("<Q", g[k]))[0]), (n, i, k)
                else:
                    assert g[k] == word(w[k]), (n, i, k, g[k], float(w[k]))
            for k in INTS:
                assert g[k] == w[k], (n, i, k, g[k], w[k])  # every integer field is exact, the NaN interval's too
        assert_same_state(got_state, want_state, n)
        # the fold in pieces leaves identical bits
        whole, split = harness_script(exe, tmp_path, n, WHOLE)[1], harness_script(exe, tmp_path, n, SPLIT)[1]
        for k in STATE:
            assert whole[k].tobytes() == split[k].tobytes() == restate(n, SPLIT)[1][k].tobytes(), (n, k)


def compare_points(exe):
    for first, n, E in PLACEMENTS:
        want = monitor_points(first, n, E)
        for K in (0, 1, CAP):  # iterations that collect nothing are counted like the others
            got = run_harness(exe, "points", first, n, K, CAP, E, 0, max(1, len(want)))
            assert got["points"] == want and got["count"] == len(want) and got["refused"] is None, (first, n, E, K, got, want)
        if want:  # one record too few is refused, and so is a first record that leaves one too few
            assert "record_capacity" in run_harness(exe, "points", first, n, 1, CAP, E, 0, len(want) - 1)["refused"]
            assert "record_capacity" in run_harness(exe, "points", first, n, 1, CAP, E, 3, len(want) + 2)["refused"]
        assert run_harness(exe, "points", first, n, 1, CAP, E, 3, len(want) + 3)["refused"] is None
    assert run_harness(exe, "points", 0, 5, 1, CAP, 100, 0, 0)["refused"] is None  # no record point needs no record
    assert "log_every" in run_harness(exe, "points", 0, 4, 1, CAP, 0, 0, 8)["refused"]
    assert "log_every" in run_harness(exe, "points", 0, 4, 1, CAP, -2, 0, 8)["refused"]
    assert "first_iteration is negative" in run_harness(exe, "points", -1, 4, 1, CAP, 1, 0, 8)["refused"]
    assert "int64" in run_harness(exe, "points", 2 ** 63 - 3, 4, 1, CAP, 1, 0, 8)["refused"]
    assert "first_record" in run_harness(exe, "points", 0, 4, 1, CAP, 1, -1, 8)["refused"]
    assert "steps_per_iteration is above capacity_steps" in run_harness(exe, "points", 0, 4, CAP + 1, CAP, 1, 0, 8)["refused"]


def test_harness_equals_the_restatements_bitwise(harness, tmp_path):
    compare_script(harness, tmp_path)
    compare_points(harness)


def test_harness_is_clean_under_address_and_undefined_sanitizers(sanitized_harness, tmp_path):
    compare_script(sanitized_harness, tmp_path)
    compare_points(sanitized_harness)


@pytest.mark.parametrize("n", HOST_COUNTS)
def test_script_says_what_its_comments_say(n):
    """The NaN reward: the mean return (and the sum it is the quotient of) of that interval is NaN -- the two other means are quotients of
    integers and stay exact --, every integer field is exact, and after the episode has ended and a clear the next record is finite."""
    records, state = restate(n, SCRIPT)
    empty, nan, after = records[EMPTY_RECORD], records[NAN_RECORD], records[AFTER_NAN_RECORD]
    assert empty["episodes"] == empty["length_sum"] == empty["successes"] == 0
    for k in FLOATS:  # +0.0, not -0.0 and not NaN
        assert word(empty[k]) == 0, k
    r = rings(n)
    # clear = 0 then clear = 1: the second record counts the first's episodes again
    assert records[2]["episodes"] >= records[1]["episodes"] > 0 and records[2]["length_sum"] >= records[1]["length_sum"]
    ended = lambda ring, slots: int(sum(((ring[1][s] | ring[2][s]) != 0).sum() for s in slots))  # noqa: E731
    assert records[1]["episodes"] == ended(r["busy"], (3, 0, 1)) and records[2]["episodes"] == ended(r["busy"], (3, 0, 1, 2))
    assert r["busy"][1][0, 0] and r["busy"][2][0, 0]  # both flags on one step: one episode, not two
    assert np.isnan(nan["mean_return"]) and np.isnan(nan["sum_return"])
    assert nan["episodes"] == n and nan["successes"] == int((np.arange(n) % 5 == 0).sum()) and nan["iteration"] == -4
    assert nan["mean_length"] == nan["length_sum"] / n and nan["success_rate"] == nan["successes"] / n
    assert all(np.isfinite(after[k]) for k in FLOATS) and after["episodes"] > 0 and after["iteration"] == 1 << 40
    assert all(np.isfinite(state[k]).all() for k in ("running_return", "sum_return"))
    # the lengths are those of the episodes: every step folded belongs to a finished episode or to the one in progress
    steps = 4 + 3 + 1 + 3 + 4
    total = sum(rec["length_sum"] for rec in (records[0], records[2], records[3], records[4]))
    assert total + int(state["running_length"].astype(np.int64).sum()) == steps * n


@pytest.mark.parametrize("n", HOST_COUNTS)
def test_restatement_against_exact_arithmetic(n):
    """The bound is derived, not measured, with u = 2^-53.  sum_r is ONE sum of the T step rewards of the finished episodes (each exact
    in float64), taken in two stages.  Stage one, per env, sequential: a reward passes through at most L additions into running_return
    (L = the steps folded: no episode is longer) and then at most e additions into sum_return (e <= L: the episodes of its env from its
    own on).  Stage two, the ordered sum: at most ceil(n / 1024) additions in its lane, then the 10 levels of the fold.  Every reward
    is therefore multiplied by at most d = 2 L + ceil(n / 1024) + 10 factors (1 + delta), |delta| <= u, whatever the order, so
    |sum_r - exact| <= ((1 + u)^d - 1) sum|r|; the division adds one more factor.  (1 + u)^(d + 1) - 1 <= (d + 2) u while (d + 1)^2 u
    << 1, and d is below 50 here."""
    L = 4 + 3 + 1 + 4
    script = [("ring", "quiet"), ("fold", 0, 4), ("ring", "busy"), ("fold", 3, 3), ("fold", 2, 1), ("fold", 0, 4), ("stats", 9, 1)]
    (got,), _ = restate(n, script)
    # the same episodes in rationals
    all_rings = rings(n)
    order = [("quiet", s) for s in range(4)] + [("busy", s) for s in (3, 0, 1, 2, 0, 1, 2, 3)]
    assert len(order) == L
    exact, magnitude, episodes, lengths = Fraction(0), Fraction(0), 0, 0
    for env in range(n):
        running, mag, steps = Fraction(0), Fraction(0), 0
        for name, s in order:
            reward, term, trunc, _ = all_rings[name]
            x = Fraction(float(reward[s, env]))
            running, mag, steps = running + x, mag + abs(x), steps + 1
            if term[s, env] or trunc[s, env]:
                exact, magnitude, episodes, lengths = exact + running, magnitude + mag, episodes + 1, lengths + steps
                running, mag, steps = Fraction(0), Fraction(0), 0
    assert got["episodes"] == episodes > 0 and got["length_sum"] == lengths
    d = 2 * L + -(-n // 1024) + 10
    bound = (d + 2) * Fraction(U) * magnitude / episodes
    error = abs(Fraction(float(got["mean_return"])) - exact / episodes)
    print(f"n = {n}: mean_return {got['mean_return']!r}, |error| {float(error):.3e}, bound {float(bound):.3e}")
    assert error <= bound
    assert got["mean_length"] == lengths / episodes and got["success_rate"] == got["successes"] / episodes  # one rounding each


@pytest.mark.parametrize("case", PLACEMENTS)
def test_points_equal_a_simulation_of_a_counting_loop(case):
    assert monitor_points(*case) == simulate_logging(*case), case


def test_placement_cases_say_what_their_names_say():
    assert monitor_points(0, 6, 2) == [1, 3, 5] and monitor_points(0, 6, 1) == list(range(6))
    assert monitor_points(0, 7, 3) == [2, 5] and monitor_points(0, 5, 100) == []
    assert monitor_points(3, 4, 2) == [0, 2] and monitor_points(4, 4, 2) == [1, 3]  # just below a multiple, and on one
    # 2 + 4 iterations in two calls place the records of one call of 6
    assert [i for i in monitor_points(0, 2, 2)] + [2 + i for i in monitor_points(2, 4, 2)] == monitor_points(0, 6, 2)
    for bad in ((-1, 1, 1), (0, -1, 1), (0, 1, 0)):
        with pytest.raises(ValueError):
            monitor_points(*bad)


def test_restatements_refuse_what_they_cannot_state():
    n = 5
    st, (r, term, trunc, succ) = zero_state(n), rings(n)["busy"]
    monitor_fold(st, r, term.astype(bool), trunc, succ, 0, 1)  # the ring's bool views are taken
    for bad in ((dict(st, episodes=st["episodes"].astype(np.int64)), r, term, trunc, succ, 0, 1), ({k: v for k, v in st.items() if k != "episodes"}, r, term, trunc, succ, 0, 1),
                (st, r.astype(np.float64), term, trunc, succ, 0, 1), (st, r, term.astype(np.int32), trunc, succ, 0, 1), (st, r, term, trunc[:3], succ, 0, 1),
                (st, r, term, trunc, succ, CAP, 1), (st, r, term, trunc, succ, -1, 1), (st, r, term, trunc, succ, 0, 0), (st, r, term, trunc, succ, 0, CAP + 1),
                (dict(st, sum_return=st["sum_return"][:4]), r, term, trunc, succ, 0, 1)):
        with pytest.raises(ValueError):
            monitor_fold(*bad)
    with pytest.raises(ValueError):
        monitor_stats(dict(st, sum_length=st["sum_length"].astype(np.int32)), 0)
    before = {k: v.copy() for k, v in st.items()}
    monitor_stats(monitor_fold(st, r, term, trunc, succ, 0, 4), 0)
    assert all(np.array_equal(st[k], before[k]) for k in st)  # the arguments are not written


def test_structs_mirror_the_header(harness):
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    layout = run_harness(harness, "layout")
    mirrors = (("urgym_monitor_state", _abi.MonitorState), ("urgym_monitor_record", _abi.MonitorRecord), ("urgym_sac_monitoring", _abi.SacMonitoring))
    assert set(layout) == {name for name, _ in mirrors}
    for name, mirror in mirrors:
        body = hdr[hdr.index(f"typedef struct {name} {{"):hdr.index(f"}} {name};")]
        declared = re.findall(r"^\s*(?:const\s+)?\w+\*?\s+(\w+);", body, flags=re.M)
        assert declared == [f for f, _ in mirror._fields_], name  # the header's order is the mirror's
        want = layout[name]
        assert C.sizeof(mirror) == want.pop("sizeof"), name
        assert {f: getattr(mirror, f).offset for f, _ in mirror._fields_} == want, name  # the C compiler's own offsets
    assert C.sizeof(_abi.MonitorRecord) == 8 * _abi.MONITOR_RECORD_WORDS and C.alignment(_abi.MonitorRecord) == 8
    assert [name for name, _ in _abi.MonitorState._fields_] == STATE and dict(_abi.SacMonitoring._fields_)["state"] is _abi.MonitorState
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    lib = _native.lib()
    for sym in ("urgym_monitor_fold", "urgym_monitor_stats", "urgym_sac_train_monitored"):
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    assert lib.urgym_abi_version() == 4
    # the header states every line of the fold and of the record
    for text in ("running_return += (double)reward", "running_length += 1", "sum_return += running_return;  sum_length += running_length;  episodes += 1;",
                 "successes += (is_success != 0)", "running_return = +0.0;  running_length = 0", "mean_return  = sum_r / (double)episodes",
                 "mean_length  = (double)length_sum / (double)episodes", "success_rate = (double)successes / (double)episodes",
                 "ceil(N / 1024) terms per lane", "the three quotients are +0.0", "(first_iteration + i + 1) % log_every == 0"):
        assert text in hdr, text


def test_refusals_that_need_no_device():
    lib = _native.lib()
    # a NULL handle is refused before anything else is looked at
    assert lib.urgym_monitor_fold(None, C.byref(_abi.MonitorState()), C.byref(_abi.ReplayRing()), 0, 1, None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert lib.urgym_monitor_fold(None, None, None, 0, 0, None) == _abi.ERR_ARG
    assert lib.urgym_monitor_stats(None, C.byref(_abi.MonitorState()), C.byref(_abi.MonitorRecord()), 0, 1, None) == _abi.ERR_ARG
    assert lib.urgym_monitor_stats(None, None, None, 0, 0, None) == _abi.ERR_ARG
    assert lib.urgym_sac_train_monitored(None, C.byref(_abi.SacLearner()), C.byref(_abi.SacSchedule()), None, C.byref(_abi.SacMonitoring()), None) == _abi.ERR_ARG
    assert lib.urgym_sac_train_monitored(None, None, None, None, None, None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
