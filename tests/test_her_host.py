"""CPU tests (-m "not gpu") of hindsight experience replay.

  * tests/her_harness.cpp, a stand-alone host program around ur_gym_amd/csrc/urgym_her.h and the pose distances of urgym_device.h --
    the functions the kernel compiles -- equals evaluation.hindsight_pick word for word and, given its own pose terms,
    evaluation.hindsight_batch bit for bit on the shared cases; built a second time with -fsanitize=address,undefined and run as
    that program.
  * evaluation.hindsight_pick and hindsight_batch against her_cases.reference_rows, a per-row Python loop written from the rule alone.
  * the census: in every count-1000 case the drawn rows hold every kind of window and every re-scoring branch the case can hold
    (her_cases.census_wanted), the largest cases hold all of them, and the relabelled share is the threshold's.
  * the properties that involve no restatement: threshold 0, OWN, FINAL on a finished episode, the ages of FUTURE.
  * the ctypes mirrors of the two new structs against the header's text and the C compiler's own layout, the new symbols, the
    refusals that need no device, and the checkpoint rule for the hindsight options on CPU tensors.

A NaN reward is compared as a NaN, not by its sign and payload bits: which NaN an operation returns is the processor's choice.
"""
import ctypes as C
import json
import os
import re
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import her_cases as hc
from her_cases import CAPACITY, COUNTS, DRAW, KINDS, NUM_ENVS, SEED, same_bits
from test_checkpoint_host import assembled_learner, learner_state
from ur_gym_amd import _abi, _native, checkpoint
from ur_gym_amd.evaluation import hindsight_batch, hindsight_pick, relabel_threshold, replay_indices
from ur_gym_amd.training import HER_DEFAULTS, PER_DEFAULTS, SAC_DEFAULTS, SACLearner

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
NEW_SYMBOLS = ("urgym_replay_sample_hindsight", "urgym_sac_train_hindsight")
CASES = hc.cases()
ROW = np.dtype([("index", "<i8"), ("g", "<i8"), ("goal_index", "<i8"), ("relabel", "<i4"), ("F", "<i4"), ("j", "<i4"), ("reward", "<f4"),
                ("terms", "<f8", (4,)), ("terminated", "u1"), ("is_success", "u1"), ("pad", "u1", (6,)), ("goal", "<f4", (6,))])


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "her_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h")] + [os.path.join(CSRC, h) for h in ("urgym_her.h", "urgym_device.h", "urgym_philox.h", "urgym_pack_map.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("her_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("her_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


@pytest.fixture(scope="module")
def rings():
    return {(N, kind): hc.synthetic_ring(N, kind) for N in NUM_ENVS for kind in KINDS}


def run(exe, *args):
    got = subprocess.run([exe, *args], capture_output=True, text=True)
    assert got.returncode == 0 and not got.stderr, (args, got.returncode, got.stdout[-500:], got.stderr[-2000:])
    return got.stdout


def harness_rows(exe, tmp_path, ring, kind, oldest, filled, horizon, strategy, threshold, count):
    Cs, N, goal_dim = ring["next_desired_goal"].shape
    cfg = hc.config(kind)
    src, dst = str(tmp_path / "her_in.bin"), str(tmp_path / "her_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<10i3Q6d", N, Cs, oldest, filled, horizon, strategy, count, kind, goal_dim, 0, threshold, SEED, DRAW,
                            *[cfg[k] for k in ("distance_threshold", "ori_threshold", "w_collision", "w_success", "w_distance", "w_orientation")]))
        for k in ("next_achieved_goal", "next_desired_goal", "reward", "terminated", "truncated", "is_success"):
            f.write(np.ascontiguousarray(ring[k]).tobytes())
    run(exe, "rows", src, dst)
    rows = np.frombuffer(open(dst, "rb").read(), dtype=ROW)
    assert rows.size == count
    return rows


def same_reward(a, b):
    """bitwise, but for rows where both are NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and same_bits(np.where(both, np.float32(0), a), np.where(both, np.float32(0), b))


def compare_with_harness(exe, tmp_path, rings, cases):
    for N, filled, oldest, horizon, strategy, kind, threshold, count in cases:
        ring = rings[(N, kind)][0]
        got = harness_rows(exe, tmp_path, ring, kind, oldest, filled, horizon, strategy, threshold, count)
        where = (N, filled, oldest, horizon, strategy, kind, threshold, count)
        pick = hindsight_pick(ring, oldest, filled, SEED, DRAW, count, threshold, strategy, horizon, N)
        for k in ("index", "g", "goal_index", "F", "j"):
            assert same_bits(got[k], pick[k]), (where, k)
        assert same_bits(got["relabel"] != 0, pick["relabel"]), where
        want = hindsight_batch(ring, oldest, filled, SEED, DRAW, count, threshold, strategy, horizon, hc.config(kind), np.ascontiguousarray(got["terms"]))
        assert same_reward(got["reward"], want["reward"]), where
        assert same_bits(got["terminated"], want["terminated"]) and same_bits(got["is_success"], want["is_success"]), where
        rel, gd = pick["relabel"], ring["desired_goal"].shape[2]
        assert same_bits(got["goal"][rel][:, :gd], want["desired_goal"][rel]) and same_bits(want["desired_goal"][rel], want["next_desired_goal"][rel]), where


def counted(cases, counts):
    return [c + (n,) for c in cases for n in counts]


def test_harness_equals_the_restatements_word_for_word(harness, tmp_path, rings):
    compare_with_harness(harness, tmp_path, rings, counted(CASES, COUNTS[-1:]) + counted(CASES[::7], COUNTS[:-1]))


def test_harness_is_clean_under_address_and_undefined_sanitizers(sanitized_harness, tmp_path, rings):
    # every ring state, horizon, strategy, env kind, threshold and count, on a third of the case list
    compare_with_harness(sanitized_harness, tmp_path, rings, counted(CASES[::3], COUNTS[-1:]) + counted(CASES[::21], COUNTS[:-1]))


def reference(ring, kind, oldest, filled, count, threshold, strategy, horizon):
    return hc.reference_rows(ring, kind, oldest, filled, hc.words(SEED, DRAW, count), threshold, strategy, horizon)


@pytest.mark.parametrize("N", NUM_ENVS)
def test_restatement_equals_a_per_row_loop_written_from_the_rule(N, rings):
    count, nan_rows, nan_reached = COUNTS[-1], 0, 0
    for n, filled, oldest, horizon, strategy, kind, threshold in CASES:
        if n != N:
            continue
        ring = rings[(N, kind)][0]
        flat = lambda a: a.reshape(CAPACITY * N, *a.shape[2:])  # noqa: E731
        rows = reference(ring, kind, oldest, filled, count, threshold, strategy, horizon)
        where = (N, filled, oldest, horizon, strategy, kind, threshold)
        pick = hindsight_pick(ring, oldest, filled, SEED, DRAW, count, threshold, strategy, horizon, N)
        for k in ("index", "relabel", "F", "j", "g", "goal_index"):
            assert pick[k].tolist() == [r[k] for r in rows], (where, k)
        assert pick["index"].dtype == np.int64 and pick["goal_index"].dtype == np.int64 and pick["F"].dtype == np.int32
        terms = np.zeros((count, 4))
        for i, r in enumerate(rows):
            if r["relabel"]:
                terms[i] = r["terms"]
        got = hindsight_batch(ring, oldest, filled, SEED, DRAW, count, threshold, strategy, horizon, hc.config(kind), terms)
        rel = pick["relabel"]
        # rows that are not relabelled are plain indexing, in every output
        for name, _, _, _ in _abi.REPLAY_RING_FIELDS:
            assert same_bits(got[name][~rel], flat(ring[name])[pick["index"]][~rel]), (where, name)
        for name in ("achieved_goal", "next_achieved_goal", "action", "truncated"):  # and these in every row
            assert same_bits(got[name], flat(ring[name])[pick["index"]]), (where, name)
        gd, lo = ring["desired_goal"].shape[2], _abi.HER_GOAL_OFFSET
        for i, r in enumerate(rows):
            if not r["relabel"]:
                continue
            assert same_reward(got["reward"][i], r["reward"]) and got["terminated"][i] == r["terminated"] and got["is_success"][i] == r["is_success"], (where, i)
            for name in ("desired_goal", "next_desired_goal"):
                assert same_bits(got[name][i], r["goal"]), (where, i, name)
            for name in ("observation", "next_observation"):
                stored = flat(ring[name])[r["index"]]
                assert same_bits(got[name][i][lo:lo + gd], r["goal"]) and same_bits(got[name][i][:lo], stored[:lo]) and same_bits(got[name][i][lo + gd:], stored[lo + gd:])
            # the NaN goal reaches the reward of a row that reads it, at most, and nothing else of any row
            reads_nan = np.isnan(r["goal"]).any() or np.isnan(flat(ring["next_achieved_goal"])[r["index"]]).any()
            assert reads_nan or not np.isnan(got["reward"][i]), (where, i)
            nan_rows, nan_reached = nan_rows + reads_nan, nan_reached + bool(np.isnan(got["reward"][i]))
    assert 0 < nan_reached <= nan_rows


@pytest.mark.parametrize("N", NUM_ENVS)
def test_every_case_holds_every_kind_of_window_and_branch(N, rings):
    everything = 0
    for n, filled, oldest, horizon, strategy, kind, threshold in CASES:
        if n != N:
            continue
        ring = rings[(N, kind)][0]
        rows = reference(ring, kind, oldest, filled, COUNTS[-1], threshold, strategy, horizon)
        relabelled = [r for r in rows if r["relabel"]]
        where = (N, filled, oldest, horizon, strategy, kind, threshold)
        # the relabelled share: within four binomial standard deviations of the threshold's ratio
        ratio = threshold / 2.0 ** 32
        assert abs(len(relabelled) - ratio * len(rows)) <= 4.0 * (len(rows) * ratio * (1.0 - ratio)) ** 0.5, (where, len(relabelled))
        have = set().union(*[hc.kinds_of(r) for r in relabelled]) if relabelled else set()
        wanted = hc.census_wanted(ring, kind, oldest, filled, threshold, strategy, horizon)
        assert wanted <= have, (where, sorted(wanted - have))
        # a full ring that wraps, with a horizon inside it and goals from other steps, holds every kind there is
        if N > 1 and (filled, oldest) == (12, 5) and horizon == 4 and strategy == _abi.HER_GOAL_FUTURE and threshold:
            branches = {"collision", "new_success"} | ({"additive"} if kind in (_abi.ENV_ORI, _abi.ENV_OBS) else {"shaping"})
            assert set(hc.WINDOW_KINDS) | branches <= have, (where, have)
            everything += 1
    assert N == 1 or everything >= 1


def near_threshold(kind, terms):
    cfg = hc.config(kind)
    return abs(terms[2] - cfg["distance_threshold"]) < 1e-6 or abs(terms[3] - cfg["ori_threshold"]) < 1e-6


@pytest.mark.parametrize("kind", KINDS)
def test_properties_that_involve_no_restatement(kind, rings):
    N, count, cfg = 257, COUNTS[-1], hc.config(kind)
    ring, shaping = rings[(N, kind)]
    flat = lambda a: a.reshape(CAPACITY * N, *a.shape[2:])  # noqa: E731
    zeros = np.zeros((count, 4))
    for filled, oldest in hc.RING_STATES:
        # threshold 0 is replay_indices plus plain indexing, bitwise
        e = replay_indices(SEED, DRAW, count, filled * N)
        entry = ((oldest + e // N) % CAPACITY) * N + e % N
        got = hindsight_batch(ring, oldest, filled, SEED, DRAW, count, 0, "future", 4, cfg, zeros)
        assert same_bits(got["index"], entry) and (got["goal_index"] == -1).all() and not got["relabel"].any()
        for name, _, _, _ in _abi.REPLAY_RING_FIELDS:
            assert same_bits(got[name], flat(ring[name])[entry]), (filled, oldest, name)
        # OWN: every reward and every flag is the stored one (rows within 1e-6 of a threshold may differ in their flags: none here)
        rows = reference(ring, kind, oldest, filled, count, 1 << 32, _abi.HER_GOAL_OWN, 4)
        terms = np.array([r["terms"] for r in rows])
        got = hindsight_batch(ring, oldest, filled, SEED, DRAW, count, 1 << 32, "own", 4, cfg, terms)
        excluded = np.array([near_threshold(kind, r["terms"]) for r in rows])
        assert excluded.mean() <= 0.01
        stored = {k: flat(ring[k])[entry] for k in ("reward", "terminated", "is_success", "next_desired_goal")}
        assert got["relabel"].all() and (got["goal_index"] == -1).all()
        clean = ~np.isnan(terms).any(axis=1)  # the row whose own achieved pose holds the NaN has no distance to anything
        assert same_bits(got["reward"][clean], stored["reward"][clean]), (filled, oldest)
        for k in ("terminated", "is_success"):
            assert same_bits(got[k][~excluded & clean], stored[k][~excluded & clean]), (filled, oldest, k)
        assert same_bits(got["desired_goal"], stored["next_desired_goal"])
        # FINAL on a finished, collision-free episode: its last row gets w_success and terminated' = 1
        rows = reference(ring, kind, oldest, filled, count, 1 << 32, _abi.HER_GOAL_FINAL, 256)
        got = hindsight_batch(ring, oldest, filled, SEED, DRAW, count, 1 << 32, "final", 256, cfg, np.array([r["terms"] for r in rows]))
        last = 0
        for i, r in enumerate(rows):
            s, n = r["slot"], r["env"]
            coll = ring["terminated"][s, n] and not ring["is_success"][s, n]
            if r["why"] not in ("terminated", "truncated") or r["F"] != 1 or coll or np.isnan(r["terms"]).any():
                continue
            last += 1
            assert r["g"] == r["index"] and got["terminated"][i] == 1 and got["is_success"][i] == 1, (filled, oldest, i)
            if kind in (_abi.ENV_DYN, _abi.ENV_STA):
                assert got["reward"][i] == np.float32(cfg["w_success"])
            else:  # the additive rewards keep what does not depend on the goal: the shaping the row was made with, and no success twice
                keep = shaping[s, n]
                r0, r1 = float(ring["reward"][s, n]), float(got["reward"][i])
                assert abs(r1 - (cfg["w_success"] + keep)) <= 2.0 ** -22 * (abs(r0) + abs(r1) + 700.0), (filled, oldest, i, r1, keep)
        assert last > 0
        # FUTURE: e's age <= g's age < e's age + F, same env
        for horizon in hc.HORIZONS:
            pick = hindsight_pick(ring, oldest, filled, SEED, DRAW, count, 1 << 32, "future", horizon, N)
            age = lambda x: (x // N - oldest) % CAPACITY  # noqa: E731
            a_e, a_g = age(pick["index"]), age(pick["goal_index"])
            assert (pick["goal_index"] % N == pick["index"] % N).all() and (a_e <= a_g).all() and (a_g < a_e + pick["F"]).all() and (a_g < filled).all()
            assert (pick["F"] >= 1).all() and (pick["F"] <= min(horizon, filled)).all()


@pytest.mark.parametrize("kind", KINDS)
def test_a_collision_with_a_success_in_one_step_is_the_rules_blind_spot(kind):
    """What the rule returns, by its own text, for an entry the step kernel stores with terminated = 1, is_success = 0 and -- in the
    additive kinds -- w_success inside the reward: succ0 is the stored flag, so G(succ0, d0, th0) holds no w_success while G(succ, d,
    th) does, and OWN returns the stored reward plus w_success.  The branching kinds return w_collision, the stored reward."""
    ring, (d, th) = hc.blind_spot_entry(kind)
    cfg = hc.config(kind)
    got = hindsight_batch(ring, 0, 1, SEED, DRAW, 4, 1 << 32, "own", 4, cfg, np.tile(np.array([[d, th, d, th]]), (4, 1)))
    stored = float(ring["reward"][0, 0])
    extra = cfg["w_success"] if kind in (_abi.ENV_ORI, _abi.ENV_OBS) else 0.0
    assert np.allclose(got["reward"], stored + extra, rtol=0, atol=1e-4) and (got["terminated"] == 1).all() and (got["is_success"] == 0).all()


def test_structs_mirror_the_header(harness):
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    layout = json.loads(run(harness, "layout"))
    for name, mirror in (("urgym_replay_hindsight", _abi.ReplayHindsight), ("urgym_sac_hindsight", _abi.SacHindsight)):
        body = hdr[hdr.index(f"typedef struct {name} {{"):hdr.index(f"}} {name};")]
        declared = re.findall(r"^\s*(?:const\s+)?\w+\*?\s+(\w+);", body, flags=re.M)
        assert declared == [f for f, _ in mirror._fields_], name  # the header's order is the mirror's
        want = layout[name]
        assert C.sizeof(mirror) == want.pop("sizeof"), name
        assert {f: getattr(mirror, f).offset for f, _ in mirror._fields_} == want, name  # the C compiler's own offsets
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    assert f"#define URGYM_HER_HORIZON_MAX {_abi.HER_HORIZON_MAX}" in hdr
    for name, value in _abi.HER_STRATEGIES.items():
        assert f"#define URGYM_HER_GOAL_{name.upper()} {value}" in hdr
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    assert lib.urgym_abi_version() == 4
    # the rule's text is in the header, and the shared header states the same constants
    her = open(os.path.join(CSRC, "urgym_her.h")).read()
    assert "HER_HORIZON_MAX = 256" in her and "HER_GOAL_OFFSET = 12" in her and "0x52504C00" in hdr[hdr.index("hindsight experience replay"):]


def test_refusals_that_need_no_device(rings):
    lib = _native.lib()
    assert lib.urgym_replay_sample_hindsight(None, None, 0, 1, 0, 0, 1, None, None, None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert lib.urgym_sac_train_hindsight(None, C.byref(_abi.SacLearner()), C.byref(_abi.SacSchedule()), C.byref(_abi.SacHindsight()), None, None, None) == _abi.ERR_ARG
    ring = rings[(5, _abi.ENV_DYN)][0]
    good = dict(oldest_slot=0, filled=4, threshold=1 << 31, strategy="future", horizon=4)
    for bad in (dict(threshold=-1), dict(threshold=(1 << 32) + 1), dict(threshold=0.5), dict(strategy="episode"), dict(strategy=3), dict(horizon=0),
                dict(horizon=257), dict(filled=0), dict(filled=CAPACITY + 1), dict(oldest_slot=CAPACITY)):
        a = dict(good, **bad)
        with pytest.raises(ValueError):
            hindsight_pick(ring, a["oldest_slot"], a["filled"], SEED, DRAW, 4, a["threshold"], a["strategy"], a["horizon"], 5)
    for k in ("truncated", "is_success"):
        with pytest.raises(ValueError, match=k):
            hindsight_batch({n: v for n, v in ring.items() if n != k}, 0, 4, SEED, DRAW, 4, 1 << 31, "future", 4, hc.config(_abi.ENV_DYN), np.zeros((4, 4)))
    with pytest.raises(ValueError, match="pose_terms"):
        hindsight_batch(ring, 0, 4, SEED, DRAW, 4, 1 << 31, "future", 4, hc.config(_abi.ENV_DYN), np.zeros((4, 4), np.float32))
    # the threshold is formed with integers
    assert relabel_threshold(4) == (4 << 32) // 5 == 3435973836 and relabel_threshold(0) == 0 and relabel_threshold(1) == 1 << 31
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError):
            relabel_threshold(bad)


def test_learner_arguments_and_the_checkpoint_rule_for_hindsight():
    assert HER_DEFAULTS == dict(hindsight=False, her_n_sampled_goal=4, her_strategy="future")
    assert not set(HER_DEFAULTS) & (set(SAC_DEFAULTS) | set(PER_DEFAULTS))
    # no her_* key in a plain run's hyperparameters; all three in a hindsight run's
    device = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)
    plain = assembled_learner()
    her = assembled_learner(**device, **dict(HER_DEFAULTS, hindsight=True, her_strategy="final"))
    assert not [k for k in plain._saved_hp() if k.startswith("her_") or k == "hindsight"]
    assert {k: her._saved_hp()[k] for k in HER_DEFAULTS} == dict(hindsight=True, her_n_sampled_goal=4, her_strategy="final")
    # a hindsight state round-trips through the checkpoint's own flattening, and a mismatch either way is refused
    state = dict(learner_state(her), hp=her._saved_hp())
    arrays, tree = checkpoint.flatten(state)
    back = checkpoint.unflatten(arrays, json.loads(json.dumps(tree)))
    assert back["hp"] == state["hp"]
    her.check_state_dict(back)
    plain_state = dict(learner_state(plain), hp=plain._saved_hp())
    plain.check_state_dict(plain_state)
    with pytest.raises(ValueError, match="hindsight is True in the checkpoint, False here"):
        assembled_learner(**device).check_state_dict(back)
    with pytest.raises(ValueError, match="hindsight is False in the checkpoint, True here"):
        her.check_state_dict(dict(learner_state(her), hp={k: v for k, v in her._saved_hp().items() if k not in HER_DEFAULTS}))
    other = assembled_learner(**device, **dict(HER_DEFAULTS, hindsight=True))
    with pytest.raises(ValueError, match="her_strategy is 'final' in the checkpoint, 'future' here"):
        other.check_state_dict(back)
    with pytest.raises(ValueError, match="only"):
        her.check_state_dict(back, override=("her_strategy",))
    # the constructor's refusals, before it touches the environment
    for bad, match in ((dict(hindsight=True), "device_entropy"), (dict(device, hindsight=True, n_steps=3), "out of scope"),
                       (dict(device, hindsight=True, prioritized=True), "out of scope"), (dict(device, hindsight=True, her_strategy="own"), "her_strategy"),
                       (dict(device, hindsight=True, her_strategy="episode"), "her_strategy"), (dict(device, hindsight=True, her_n_sampled_goal=0), "her_n_sampled_goal"),
                       (dict(device, hindsight=1), "hindsight must be")):
        with pytest.raises(ValueError, match=match):
            SACLearner(None, **bad)
    with pytest.raises(ValueError, match="max_episode_steps"):
        SACLearner(SimpleNamespace(cfg=SimpleNamespace(max_episode_steps=300)), **device, hindsight=True)
    with pytest.raises(TypeError, match="unknown"):
        SACLearner(None, her_horizon=5)
