"""CPU tests (-m "not gpu") of the multi-step returns.

  * tests/nstep_harness.cpp, a stand-alone host program around ur_gym_amd/csrc/urgym_nstep.h and sac_target_row_nstep of
    urgym_sac_terms.h -- the functions the kernels compile -- equals evaluation.nstep_batch and evaluation.entropy_step_nstep word for
    word on the shared cases; built a second time with -fsanitize=address,undefined and run as that program.
  * evaluation.nstep_batch against nstep_cases.reference_rows, a per-row Python loop written from the rule alone: m, entry_0 and
    entry_{m-1} exactly, R within m 2^-23 sum |gamma^k r_k| of the float64 sum, discount within m ulp of gamma^m, and at n_steps = 1
    plain indexing by replay_indices, bitwise.
  * the census: in every (N, ring state, n_steps > 1) case the drawn rows hold every kind of window (nstep_cases.census).
  * the ctypes mirrors of the three new structs against the header's text and the C compiler's own layout, the new symbols, the
    refusals that need no device, and the checkpoint rule for n_steps on CPU tensors.
"""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from nstep_cases import (CAPACITY, COUNTS, DRAW, GAMMA, N_STEPS, NUM_ENVS, RING_STATES, SEED, census, entropy_inputs, reference_rows, same_bits,
                         synthetic_ring)
from test_checkpoint_host import assembled_learner, learner_state
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import adam_coefficients, entropy_step, entropy_step_nstep, nstep_batch, replay_indices
from ur_gym_amd.training import SAC_DEFAULTS, SACLearner

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
OBS_DIM, GOAL_DIM = 5, 3  # the walk reads no row: any widths do on the host
NEW_SYMBOLS = ("urgym_replay_sample_nstep", "urgym_sac_entropy_step_nstep", "urgym_sac_train_nstep")
CASES = [(N, filled, oldest, n) for N in NUM_ENVS for filled, oldest in RING_STATES for n in N_STEPS]


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "nstep_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h")] + [os.path.join(CSRC, h) for h in ("urgym_nstep.h", "urgym_sac_terms.h", "urgym_adam.h", "urgym_pack_map.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("nstep_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("nstep_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


@pytest.fixture(scope="module")
def rings():
    return {N: synthetic_ring(N, OBS_DIM, GOAL_DIM) for N in NUM_ENVS}


def run(exe, *args):
    got = subprocess.run([exe, *args], capture_output=True, text=True)
    assert got.returncode == 0 and not got.stderr, (args, got.returncode, got.stdout[-500:], got.stderr[-2000:])
    return got.stdout


def harness_walk(exe, tmp_path, ring, oldest, filled, n_steps, count, gamma=GAMMA):
    Cs, N = ring["reward"].shape
    src, dst = str(tmp_path / "walk_in.bin"), str(tmp_path / "walk_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<6if", N, Cs, oldest, filled, n_steps, count, gamma))
        f.write(replay_indices(SEED, DRAW, count, filled * N).astype("<i8").tobytes())
        f.write(ring["reward"].tobytes())
        for k in ("terminated", "truncated", "is_success"):
            f.write(ring[k].tobytes())
    run(exe, "walk", src, dst)
    rows = np.frombuffer(open(dst, "rb").read(), dtype=np.dtype([("R", "<f4"), ("g", "<f4"), ("m", "<i4"), ("flags", "<u4"), ("first", "<i8"), ("last", "<i8")]))
    assert rows.size == count
    return rows


def compare_walks(exe, tmp_path, rings):
    for N, filled, oldest, n in CASES:
        for count in (COUNTS[0], COUNTS[-1]):
            got = harness_walk(exe, tmp_path, rings[N], oldest, filled, n, count)
            want = nstep_batch(rings[N], oldest, filled, SEED, DRAW, count, n, GAMMA)
            where = (N, filled, oldest, n, count)
            assert same_bits(got["R"], want["reward"]) and same_bits(got["g"], want["discount"]), where
            assert same_bits(got["m"], want["steps"]) and same_bits(got["first"], want["index"]) and same_bits(got["last"], want["last_index"]), where
            flags = want["terminated"].astype(np.uint32) | want["truncated"].astype(np.uint32) << 8 | want["is_success"].astype(np.uint32) << 16
            assert same_bits(got["flags"], flags), where


def compare_targets(exe, tmp_path):
    for count in (1, 1023, 1025):
        x = entropy_inputs(count)
        alpha = np.float32(np.exp(x["l"]))
        src, dst = str(tmp_path / "target_in.bin"), str(tmp_path / "target_out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<if", count, alpha))
            for k in ("reward", "q_min_next", "discount", "next_log_prob", "terminated"):
                f.write(x[k].tobytes())
        run(exe, "target", src, dst)
        y = np.frombuffer(open(dst, "rb").read(), dtype=np.float32)
        want = entropy_step_nstep(alpha, x["log_prob"], -6.0, x["l"], x["m"], x["v"], host_coef(), reward=x["reward"], q_min_next=x["q_min_next"],
                                  discount=x["discount"], next_log_prob=x["next_log_prob"], terminated=x["terminated"])
        assert same_bits(y, want["y"]), count


def host_coef():
    """Adam's seven coefficients as the library forms them; any valid set does here: the comparisons are of y."""
    return adam_coefficients(None, 1e-4, step=3)


def test_harness_equals_the_restatements_word_for_word(harness, tmp_path, rings):
    compare_walks(harness, tmp_path, rings)
    compare_targets(harness, tmp_path)


def test_harness_is_clean_under_address_and_undefined_sanitizers(sanitized_harness, tmp_path, rings):
    compare_walks(sanitized_harness, tmp_path, rings)
    compare_targets(sanitized_harness, tmp_path)


@pytest.mark.parametrize("N", NUM_ENVS)
def test_restatement_equals_a_per_row_loop_written_from_the_rule(N, rings):
    ring, count, g32 = rings[N], COUNTS[-1], np.float32(GAMMA)
    flat = lambda a: a.reshape(CAPACITY * N, *a.shape[2:])  # noqa: E731
    for filled, oldest in RING_STATES:
        e = replay_indices(SEED, DRAW, count, filled * N)
        for n in N_STEPS:
            got = nstep_batch(ring, oldest, filled, SEED, DRAW, count, n, GAMMA)
            rows = reference_rows(ring, oldest, filled, e, n, GAMMA)
            where = (N, filled, oldest, n)
            assert got["steps"].tolist() == [r["m"] for r in rows] and got["index"].tolist() == [r["first"] for r in rows], where
            assert got["last_index"].tolist() == [r["last"] for r in rows], where
            for i, r in enumerate(rows):
                R = float(got["reward"][i])
                if np.isnan(r["total"]):
                    assert np.isnan(R), (where, i)
                else:  # m - 1 products and m - 1 sums, each within half an ulp of a partial sum no larger than the sum of magnitudes
                    assert abs(R - r["total"]) <= r["m"] * 2.0 ** -23 * r["magnitude"], (where, i, R, r["total"])
                assert abs(float(got["discount"][i]) - r["discount"]) <= r["m"] * float(np.spacing(np.float32(r["discount"]))), (where, i)
            assert got["discount"].dtype == np.float32 and got["reward"].dtype == np.float32 and got["steps"].dtype == np.int32
            # the rows come from entry_0, the next rows and the flags from entry_{m-1}
            for name in ("observation", "achieved_goal", "desired_goal", "action"):
                assert same_bits(got[name], flat(ring[name])[got["index"]]), (where, name)
            for name in ("next_observation", "next_achieved_goal", "next_desired_goal", "terminated", "truncated", "is_success"):
                assert same_bits(got[name], flat(ring[name])[got["last_index"]]), (where, name)
            if n == 1:  # plain indexing by replay_indices, and the discount is gamma itself
                entry = ((oldest + e // N) % CAPACITY) * N + e % N
                assert same_bits(got["index"], entry) and same_bits(got["last_index"], entry) and same_bits(got["discount"], np.full(count, g32))
                assert same_bits(got["reward"], flat(ring["reward"])[entry]) and (got["steps"] == 1).all(), where
    # one NaN reward reaches the rows whose window holds it, and no other row
    got = nstep_batch(ring, 0, CAPACITY, SEED, DRAW, count, 3, GAMMA)
    rows = reference_rows(ring, 0, CAPACITY, replay_indices(SEED, DRAW, count, CAPACITY * N), 3, GAMMA)
    assert np.isnan(got["reward"]).tolist() == [bool(np.isnan(r["total"])) for r in rows] and 0 < np.isnan(got["reward"]).sum() < count


@pytest.mark.parametrize("N", NUM_ENVS)
def test_every_case_holds_every_kind_of_window(N, rings):
    for filled, oldest in RING_STATES:
        e = replay_indices(SEED, DRAW, COUNTS[-1], filled * N)
        for n in N_STEPS:
            if n == 1:
                continue
            have, missing = census(reference_rows(rings[N], oldest, filled, e, n, GAMMA), n, filled)
            assert not missing, (N, filled, oldest, n, missing, have)
    # and the synthetic ring has entries with both flags set where it has random envs
    assert N == 3 or (rings[N]["terminated"] & rings[N]["truncated"]).any()


def test_entropy_step_nstep_with_gamma_as_discount_is_the_two_step_route():
    f = np.float32
    for count in (1, 1025):
        x = entropy_inputs(count)
        alpha, gamma = f(np.exp(x["l"])), f(GAMMA)
        nd = np.where(x["terminated"].astype(bool), f(0), f(1))
        target = x["reward"] + (gamma * nd) * x["q_min_next"]  # urgym_critic_evaluate's target at ent_coef = 0, one rounding per operation
        assert target.dtype == f
        old = entropy_step(alpha, x["log_prob"], -6.0, x["l"], x["m"], x["v"], host_coef(), target=target, next_log_prob=x["next_log_prob"],
                           terminated=x["terminated"], gamma=GAMMA, scale=1.0 / count)
        new = entropy_step_nstep(alpha, x["log_prob"], -6.0, x["l"], x["m"], x["v"], host_coef(), reward=x["reward"], q_min_next=x["q_min_next"],
                                 discount=np.full(count, gamma), next_log_prob=x["next_log_prob"], terminated=x["terminated"], scale=1.0 / count)
        assert set(old) == set(new) and all(same_bits(np.asarray(old[k]), np.asarray(new[k])) for k in old), count
    with pytest.raises(ValueError, match="half given"):
        entropy_step_nstep(alpha, x["log_prob"], -6.0, x["l"], x["m"], x["v"], host_coef(), reward=x["reward"])


def test_structs_mirror_the_header(harness):
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    layout = json.loads(run(harness, "layout"))
    for name, mirror in (("urgym_replay_nstep", _abi.ReplayNstep), ("urgym_sac_entropy_nstep_args", _abi.SacEntropyNstepArgs), ("urgym_sac_nstep", _abi.SacNstep)):
        body = hdr[hdr.index(f"typedef struct {name} {{"):hdr.index(f"}} {name};")]
        declared = re.findall(r"^\s*(?:const\s+)?\w+\*?\s+(\w+);", body, flags=re.M)
        assert declared == [f for f, _ in mirror._fields_], name  # the header's order is the mirror's
        want = layout[name]
        assert C.sizeof(mirror) == want.pop("sizeof"), name
        assert {f: getattr(mirror, f).offset for f, _ in mirror._fields_} == want, name  # the C compiler's own offsets
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    assert f"#define URGYM_REPLAY_NSTEP_MAX {_abi.REPLAY_NSTEP_MAX}" in hdr
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    assert lib.urgym_abi_version() == 4


def test_refusals_that_need_no_device(rings):
    lib = _native.lib()
    assert lib.urgym_replay_sample_nstep(None, None, 0, 1, 0, 0, 1, None, None, None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert lib.urgym_sac_entropy_step_nstep(None, C.byref(_abi.SacEntropyNstepArgs()), C.byref(_abi.AdamHyper()), None) == _abi.ERR_ARG
    assert lib.urgym_sac_train_nstep(None, C.byref(_abi.SacLearner()), C.byref(_abi.SacSchedule()), C.byref(_abi.SacNstep()), None, None, None) == _abi.ERR_ARG
    ring = rings[3]
    for bad in (dict(n_steps=0), dict(n_steps=33), dict(gamma=np.inf), dict(gamma=np.nan), dict(filled=0), dict(filled=CAPACITY + 1), dict(oldest_slot=CAPACITY)):
        args = dict(dict(oldest_slot=0, filled=4, n_steps=3, gamma=GAMMA), **bad)
        with pytest.raises(ValueError):
            nstep_batch(ring, args["oldest_slot"], args["filled"], SEED, DRAW, 4, args["n_steps"], args["gamma"])
    with pytest.raises(ValueError, match="truncated"):
        nstep_batch({k: v for k, v in ring.items() if k != "truncated"}, 0, 4, SEED, DRAW, 4, 2, GAMMA)
    nstep_batch({k: v for k, v in ring.items() if k != "truncated"}, 0, 4, SEED, DRAW, 4, 1, GAMMA)  # one step needs no truncated


def test_learner_arguments_and_the_checkpoint_rule_for_n_steps():
    assert SAC_DEFAULTS["n_steps"] == 1
    # the key is absent from a one-step run's hyperparameters and present otherwise
    one, three = assembled_learner(), assembled_learner(n_steps=3)
    assert "n_steps" not in one._saved_hp() and three._saved_hp()["n_steps"] == 3
    assert {k: v for k, v in one._saved_hp().items()} == {k: v for k, v in SAC_DEFAULTS.items() if k != "n_steps"} | dict(hidden_width=32, batch_size=64)
    # a state without the key is a one-step run's; a mismatch either way is refused with the other mismatch errors
    state = dict(learner_state(one), hp=one._saved_hp())
    one.check_state_dict(state)
    with pytest.raises(ValueError, match="n_steps is 1 in the checkpoint, 3 here"):
        three.check_state_dict(state)
    state3 = dict(learner_state(three), hp=three._saved_hp())
    three.check_state_dict(state3)
    with pytest.raises(ValueError, match="n_steps is 3 in the checkpoint, 1 here"):
        one.check_state_dict(state3)
    with pytest.raises(ValueError, match="only"):
        three.check_state_dict(state3, override=("n_steps",))
    # the constructor refuses n_steps > 1 without device_entropy, and values outside [1, 32], before it touches the environment
    for bad in (dict(n_steps=3), dict(n_steps=0), dict(n_steps=33), dict(n_steps=2.5), dict(n_steps=True)):
        with pytest.raises((ValueError, TypeError)):
            SACLearner(None, **bad)
