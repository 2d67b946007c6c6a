"""CPU tests (-m "not gpu") of the SAC training loop in one native call.

  * tests/sac_schedule_harness.cpp, a stand-alone host program around ur_gym_amd/csrc/urgym_sac_schedule.h -- the header
    urgym_sac_train compiles -- equals evaluation.training_schedule field by field on every schedule of sac_train_cases.SCHEDULES;
    built a second time with -fsanitize=address,undefined and run as that program.
  * evaluation.training_schedule, with U and I from evaluation.warmup_iterations (the function SACLearner.train uses), equals a
    plain-Python simulation of today's loop: the same slots, modes, draws, step numbers and ring views for every update.
  * every schedule refusal, through the harness and through the restatement.
  * the ctypes mirrors of the two new structs against the C compiler's own layout, the new symbol, the refusals that need no device.
"""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

from sac_train_cases import REFUSED, SCHEDULES, TOP, simulate_loop
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import training_schedule, warmup_iterations

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
ORDER = [name for name, _ in _abi.SacSchedule._fields_]


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "sac_schedule_harness.cpp")
    deps = [src, os.path.join(CSRC, "urgym_sac_schedule.h"), os.path.join(ROOT, "include", "urgym.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("sac_schedule_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("sac_schedule_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run_harness(exe, *args):
    run = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (args, run.returncode, run.stdout[-500:], run.stderr[-2000:])
    return json.loads(run.stdout)


def compare_all(exe):
    for name, sched in SCHEDULES.items():
        got = run_harness(exe, "schedule", *[sched[k] for k in ORDER])
        want = training_schedule(**sched)
        assert "refused" not in got, (name, got)
        assert got["num_updates"] == want["num_updates"] == len(want["updates"]) and len(got["iterations"]) == sched["num_iterations"], name
        assert (got["cursor"], got["filled"]) == (want["cursor"], want["filled"]), name
        for i, (g, w) in enumerate(zip(got["iterations"], want["iterations"])):
            assert g == w, (name, i, g, w)  # field by field: the dicts hold the same names
        for u, (g, w) in enumerate(zip(got["updates"], want["updates"])):
            assert g == w, (name, u, g, w)
    for name, sched in REFUSED.items():
        got = run_harness(exe, "schedule", *[sched[k] for k in ORDER])
        assert set(got) == {"refused"} and got["refused"], (name, got)
        with pytest.raises(ValueError):
            training_schedule(**sched)


def test_harness_equals_the_restatement_field_by_field(harness):
    compare_all(harness)


def test_harness_is_clean_under_address_and_undefined_sanitizers(sanitized_harness):
    compare_all(sanitized_harness)


def test_schedule_cases_say_what_their_names_say():
    s = training_schedule(**SCHEDULES["wraps at K = 1"])
    assert [it["collect_first_slot"] for it in s["iterations"]] == [0, 1, 2, 3, 0, 1] and (s["cursor"], s["filled"]) == (2, 4)
    assert [(it["oldest_slot"], it["filled_steps"]) for it in s["iterations"]] == [(0, 1), (0, 2), (0, 3), (0, 4), (1, 4), (2, 4)]
    assert [it["collect_first_draw"] for it in s["iterations"]] == [5, 6, 7, 8, 9, 10]
    assert [u["gather_draw"] for u in s["updates"]] == list(range(100, 112)) and s["updates"][3]["policy_draw"] == 103 | TOP
    assert [u["adam_step"] for u in s["updates"]] == list(range(1, 13)) and [u["loss_slot"] for u in s["updates"]] == list(range(12))
    s = training_schedule(**SCHEDULES["K = 5 > C"])
    assert all(it["filled_steps"] == 4 and it["oldest_slot"] == (it["collect_first_slot"] + 5) % 4 for it in s["iterations"])  # oldest = cursor
    s = training_schedule(**SCHEDULES["U, I = 2, 1"])
    assert [it["collect_mode"] for it in s["iterations"]] == [_abi.SAMPLE_UNIFORM] * 2 + [_abi.SAMPLE_GAUSSIAN] * 4
    assert [it["idle"] for it in s["iterations"]] == [1, 0, 0, 0, 0, 0] and s["updates"][0]["iteration"] == 1 and s["num_updates"] == 10
    s = training_schedule(**SCHEDULES["U, I = 7, 7 with 6 iterations"])
    assert s["num_updates"] == 0 and all(it["collect_mode"] == _abi.SAMPLE_UNIFORM and it["idle"] for it in s["iterations"])
    s = training_schedule(**SCHEDULES["K = 0 on a filled ring"])
    assert (s["cursor"], s["filled"], s["num_updates"]) == (1, 4, 6) and all((it["oldest_slot"], it["filled_steps"]) == (1, 4) for it in s["iterations"])
    s = training_schedule(**SCHEDULES["the last admissible update_first_draw"])
    assert s["updates"][-1]["gather_draw"] == TOP - 1 and s["updates"][-1]["policy_draw"] == (1 << 64) - 1
    s = training_schedule(**SCHEDULES["collect draws wrap at 2^64"])
    assert [it["collect_first_draw"] for it in s["iterations"]] == [(1 << 64) - 2, (1 << 64) - 1, 0, 1]


LOOPS = [  # (N, learning_starts, env_steps before, K, G, iterations, capacity, first_slot, filled)
    (64, 128, 0, 1, 2, 6, 4, 0, 0),     # the GPU tests' configuration: U, I = 2, 1
    (64, 128, 0, 2, 1, 4, 4, 0, 0),     # U, I = 1, 0
    (64, 128, 1, 1, 2, 4, 4, 1, 1),     # a second call: U, I = 1, 0
    (64, 129, 0, 1, 1, 6, 4, 0, 0),     # learning_starts no multiple of N: U, I = 3, 2
    (64, 100, 0, 0, 3, 1, 4, 2, 3),     # K = 0 before learning_starts: every iteration idle
    (64, 100, 2, 0, 3, 2, 4, 2, 2),     # K = 0 after it
    (64, 10 ** 6, 0, 3, 2, 5, 4, 0, 0),  # all warm-up
    (1024, 100, 0, 1, 4, 5, 3, 0, 0),   # tools/train_sac.py's defaults: N above learning_starts, U, I = 1, 0
    (7, 100, 3, 5, 1, 6, 4, 3, 3),
]


@pytest.mark.parametrize("case", LOOPS)
def test_restatement_equals_a_simulation_of_todays_loop(case):
    N, starts, env_steps, K, G, n, cap, slot, filled = case
    U, I = warmup_iterations(env_steps, N, starts, n, K)
    assert 0 <= I <= n and 0 <= U <= n and (K == 0 or I <= U)
    if G > 0 and I < n and K == 0 and filled == 0:
        pytest.fail("the case would be refused")
    s = training_schedule(first_slot=slot, filled_steps=filled, capacity_steps=cap, num_iterations=n, steps_per_iteration=K, updates_per_iteration=G,
                          uniform_iterations=U, idle_iterations=I, collect_first_draw=40, update_first_draw=9, first_step=3 + 1)
    collections, updates, end = simulate_loop(capacity_steps=cap, first_slot=slot, filled_steps=filled, num_envs=N, learning_starts=starts,
                                              env_steps=env_steps, draw=40, adam_step=3, iterations=n, steps_per_iteration=K, updates_per_iteration=G,
                                              update_first_draw=9)
    assert len(collections) == (n if K else 0)
    for c in collections:
        it = s["iterations"][c["iteration"]]
        assert {k: it[k] for k in ("collect_first_slot", "collect_first_draw", "collect_mode")} == {k: c[k] for k in c if k != "iteration"}, c
    assert len(updates) == s["num_updates"] == len(s["updates"])
    for got, want in zip(s["updates"], updates):
        it = s["iterations"][got["iteration"]]
        assert not it["idle"]
        merged = dict(got, oldest_slot=it["oldest_slot"], filled_steps=it["filled_steps"])
        assert merged == want, (merged, want)
    assert all(it["idle"] == (not any(u["iteration"] == i for u in updates)) or G == 0 for i, it in enumerate(s["iterations"]))
    assert (s["cursor"], s["filled"]) == (end["cursor"], end["filled"])
    # what SACLearner.train adds to its counters
    assert end["env_steps"] == env_steps + n * K and end["draw"] == 40 + n * K and end["adam_step"] == 3 + s["num_updates"]


def test_structs_mirror_the_header(harness):
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    layout = run_harness(harness, "layout")
    for name, mirror in (("urgym_sac_schedule", _abi.SacSchedule), ("urgym_sac_learner", _abi.SacLearner)):
        body = hdr[hdr.index(f"typedef struct {name} {{"):hdr.index(f"}} {name};")]
        declared = re.findall(r"^\s*(?:const\s+)?\w+\*?\s+(\w+);", body, flags=re.M)
        assert declared == [f for f, _ in mirror._fields_], name  # the header's order is the mirror's
        want = layout[name]
        assert C.sizeof(mirror) == want.pop("sizeof"), name
        assert {f: getattr(mirror, f).offset for f, _ in mirror._fields_} == want, name  # the C compiler's own offsets
    # members that are structs of the header are the existing mirrors
    kinds = dict(_abi.SacLearner._fields_)
    assert kinds["actor_adam"] is _abi.ActorAdam and kinds["critic_adam"] is _abi.CriticAdam and kinds["ring"] is _abi.ReplayRing and kinds["batch"] is _abi.ReplayBatch
    assert [n for n, _ in _abi.SAC_LEARNER_SCRATCH] == [f for f, _ in _abi.SacLearner._fields_][14:26]
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    lib = _native.lib()
    sym = "urgym_sac_train"
    assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M)
    assert lib.urgym_abi_version() == 4
    # the header states the sequence and lists the schedule's refusals
    for text in ("urgym_critic_adam_step(online, target, critic_adam, hp, tau)", "an update that\n * would see an empty ring", "K and G both 0",
                 "update_first_draw + the number of updates > 2^63", "first_step < 1", "names the iteration and the stage"):
        assert text in hdr, text


def test_refusals_that_need_no_device():
    lib = _native.lib()
    # a NULL handle is refused before anything else is looked at
    assert lib.urgym_sac_train(None, C.byref(_abi.SacLearner()), C.byref(_abi.SacSchedule()), None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert lib.urgym_sac_train(None, None, None, None) == _abi.ERR_ARG
    assert lib.urgym_sac_train(None, None, C.byref(_abi.SacSchedule()), None) == _abi.ERR_ARG
    # the restatement refuses what is no integer or does not fit its field
    ok = SCHEDULES["wraps at K = 1"]
    for bad in (dict(num_iterations=1.5), dict(first_slot=True), dict(capacity_steps=1 << 31), dict(collect_first_draw=1 << 64), dict(first_step=1 << 63)):
        with pytest.raises(ValueError):
            training_schedule(**dict(ok, **bad))


def test_warmup_iterations_is_the_learning_starts_rule():
    for N, starts, e, K, n in ((64, 128, 0, 1, 6), (64, 128, 5, 1, 3), (64, 129, 0, 2, 6), (3, 1000, 7, 4, 200), (64, 128, 0, 0, 4), (64, 128, 2, 0, 4),
                               (64, 0, 0, 1, 3), (5, 99.5, 0, 3, 10)):
        U = next((i for i in range(n) if not (e + i * K) * N < starts), n)
        I = next((i for i in range(n) if not (e + (i + 1) * K) * N < starts), n)
        assert warmup_iterations(e, N, starts, n, K) == (U, I), (N, starts, e, K, n)
