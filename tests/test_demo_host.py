"""CPU tests (-m "not gpu") of the demonstration ring.

  * tests/demo_harness.cpp, a stand-alone host program around urgym_demo.h and urgym_sac_bc.h -- the functions the kernels compile --
    equals evaluation.mixed_entries in every index and source byte (N_d = 1, size_d = 1, wrapping oldest slots, a size above 2^32), and
    evaluation.policy_terms_cloned(row_mask=) bit for bit in every output.  Built a second time with -fsanitize=address,undefined and run
    as that program.
  * mixed_indices with D = 0 is replay_indices; rows from D on are replay_indices' at every D; a row does not depend on count.
  * the ctypes mirrors of the two new structs against the header's text and the C compiler's layout, the new symbols, the refusals that
    need no device, the dispatch of the training entry, the file round trip of a ring, the learner's argument errors and checkpoint rule.
"""
import ctypes as C
import json
import os
import re
import struct
import subprocess
import types

import numpy as np
import pytest

import sac_bc_cases as bc
from sac_bc_cases import FLAGS, WEIGHT, same
from test_checkpoint_host import assembled_learner, learner_state
from ur_gym_amd import _abi, _native, checkpoint
from ur_gym_amd.evaluation import DeviceReplay, mixed_entries, mixed_indices, policy_terms, policy_terms_cloned, replay_indices
from ur_gym_amd.training import BC_DEFAULTS, CLIP_DEFAULTS, DEMO_DEFAULTS, HER_DEFAULTS, NORM_DEFAULTS, PER_DEFAULTS, SAC_DEFAULTS, SACLearner
from ur_gym_amd.vector_env import _SAC_TRAIN_ENTRIES, _sac_train_entry

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
NEW_SYMBOLS = ("urgym_replay_sample_mixed", "urgym_sac_policy_terms_cloned_masked", "urgym_sac_train_demonstrated")
DEVICE = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)

# (count, D, own = (oldest, filled, N, C), demo = (oldest, filled, N, C)): one env in the demonstrations; ONE entry in them; both oldest
# slots wrapping; the straddled wave; sizes above 2^32 on either side (filled * N in int32 each: 2^21 x 2^12 = 2^33)
ENTRY_CASES = (
    (65, 17, (3, 4, 8, 4), (2, 3, 1, 3)),
    (65, 64, (1, 2, 8, 4), (0, 1, 1, 1)),
    (130, 65, (3, 4, 8, 4), (2, 3, 3, 3)),
    (130, 129, (0, 1, 1, 1), (1, 2, 3, 3)),
    (1, 1, (0, 4, 8, 4), (1, 3, 3, 3)),
    (1, 0, (0, 4, 8, 4), (1, 3, 3, 3)),
    (257, 100, (1 << 20, 1 << 21, 1 << 12, 1 << 21), (5, 7, 3, 9)),
    (257, 200, (2, 3, 5, 4), ((1 << 21) - 1, 1 << 21, 1 << 12, 1 << 21)),
)


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "demo_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h")] + [os.path.join(CSRC, h) for h in ("urgym_demo.h", "urgym_sac_bc.h", "urgym_sac_terms.h", "urgym_adam.h",
                                                                                                "urgym_pack_map.h", "urgym_device.h", "urgym_philox.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("demo_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("demo_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run(exe, mode, src, dst):
    got = subprocess.run([exe, mode, src, dst], capture_output=True, text=True)
    assert got.returncode == 0 and not got.stderr, (got.stdout, got.stderr[-2000:])
    return open(dst, "rb").read()


def harness_entries(exe, tmp_path, seed, draw, count, D, own, demo):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<QQqq", seed, draw, count, D))
        for oldest, filled, n, cap in (own, demo):
            f.write(struct.pack("<Qiiii", filled * n, n, cap, oldest, 0))
    raw = run(exe, "entries", src, dst)
    assert len(raw) == 9 * count
    return np.frombuffer(raw[:8 * count], dtype=np.int64), np.frombuffer(raw[8 * count:], dtype=np.uint8)


def compare_entries(exe, tmp_path):
    for count, D, own, demo in ENTRY_CASES:
        for seed, draw in ((7, 0), (0xDEADBEEFCAFEF00D, (1 << 63) + 12345)):
            index, source = harness_entries(exe, tmp_path, seed, draw, count, D, own, demo)
            want_index, want_source = mixed_entries(seed, draw, count, own, D, demo)
            where = (count, D, own, demo, seed, draw)
            assert np.array_equal(index, want_index), where
            assert np.array_equal(source, want_source.astype(np.uint8)) and source.sum() == D, where
            for mask, (oldest, filled, n, cap) in ((want_source, demo), (~want_source, own)):  # an entry of a filled slot of the row's own ring
                slot, env = index[mask] // n, index[mask] % n
                assert ((slot - oldest) % cap < filled).all() and (0 <= env).all() and (index[mask] < cap * n).all(), where


def test_entry_map_equals_the_restatement(harness, tmp_path):
    compare_entries(harness, tmp_path)


def test_entry_map_is_clean_under_address_and_undefined_sanitizers(sanitized_harness, tmp_path):
    compare_entries(sanitized_harness, tmp_path)


def test_cases_reach_what_they_are_meant_to():
    big = [c for c in ENTRY_CASES if c[2][1] * c[2][2] > 1 << 32 or c[3][1] * c[3][2] > 1 << 32]
    assert len(big) == 2
    for count, D, own, demo in big:  # the draws really go above 2^32 on the big side, and e / N is not e >> 32 of anything
        e = mixed_indices(7, 0, count, own[1] * own[2], D, demo[1] * demo[2])
        assert (e >= 1 << 32).any() and (e < 1 << 32).any()
    assert any(c[3][2] == 1 for c in ENTRY_CASES) and any(c[3][1] * c[3][2] == 1 for c in ENTRY_CASES)
    assert any((c[3][0] + c[3][1]) > c[3][3] for c in ENTRY_CASES) and any((c[2][0] + c[2][1]) > c[2][3] for c in ENTRY_CASES)  # both wrap


def test_mixed_indices_against_replay_indices():
    for seed, draw, count, size, size_d in ((3, 9, 130, 32, 9), (1 << 40, (1 << 64) - 1, 65, (1 << 33) + 5, 1), (0, 0, 1, 1, 1 << 62)):
        plain = replay_indices(seed, draw, count, size)
        assert np.array_equal(mixed_indices(seed, draw, count, size, 0, size_d), plain)  # D = 0: the plain draw
        for D in sorted({1, count // 2, count - 1, count} & set(range(count + 1))):
            got = mixed_indices(seed, draw, count, size, D, size_d)
            assert np.array_equal(got[D:], plain[D:]) and (got[:D] < size_d).all() and (got[:D] >= 0).all()
            # a row is a function of (seed, draw, i, size, size_d) alone: not of count, and of D only through its side
            longer = mixed_indices(seed, draw, count + 65, size, D, size_d)
            assert np.array_equal(longer[:count], got)
            assert np.array_equal(mixed_indices(seed, draw, count, size, count, size_d)[:D], got[:D])
        if count > 1 and size_d > 1 and size > 1:  # the two tags give different words
            assert not np.array_equal(mixed_indices(seed, draw, count, size, count, size), plain)
    for bad in (dict(demo_count=-1), dict(demo_count=11), dict(demo_size=0), dict(demo_size=1 << 63)):
        with pytest.raises(ValueError):
            mixed_indices(1, 2, 10, 5, **dict(dict(demo_count=3, demo_size=4), **bad))
    tags = {_abi.REPLAY_TAG, 0x50455200, _abi.DEMO_TAG} | {0x504F4C00 | b for b in range(256)} | {0x4D505000 | b for b in range(256)} | set(range(5))
    assert _abi.DEMO_TAG == 0x44454D00 and len(tags) == 3 + 256 + 256 + 5  # it meets none of the tags in use


MASKS = ("ones", "zeros", "prefix1", "prefix64", "scattered")


def mask_of(kind, count):
    m = np.zeros(count, dtype=np.uint8)
    if kind == "ones":
        m[:] = 1
    elif kind.startswith("prefix"):
        m[:min(count, int(kind[6:]))] = 1
    elif kind == "scattered":
        m[:] = np.random.default_rng([count, 5]).integers(0, 2, count)
        m[m != 0] = np.random.default_rng([count, 6]).integers(1, 256, int((m != 0).sum()))  # any nonzero byte marks a row
    return m


def harness_masked(exe, tmp_path, x, count, mask, scale_by_q, q_filter):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<qii", count, int(scale_by_q), int(q_filter)))
        f.write(np.array([x["alpha"], -1.0 / count, WEIGHT, 1.0 / count], dtype=np.float32).tobytes())
        for k in ("log_prob", "q", "y", "q_min", "dqmin_da", "action_pi", "action_data"):
            f.write(np.ascontiguousarray(x[k], dtype=np.float32).tobytes())
        f.write(mask.tobytes())
    raw = run(exe, "masked", src, dst)
    assert len(raw) == 40 + 20 + 4 + count + 24 * count
    out = dict(zip(("critic_loss", "actor_loss", "bc_loss", "bc_weight", "mean_abs"), np.frombuffer(raw[40:60], dtype=np.float32)))
    out["bc_rows"] = np.frombuffer(raw[60:64], dtype=np.int32)[0]
    out["cloned"] = np.frombuffer(raw[64:64 + count], dtype=np.uint8).astype(bool)
    out["d_action"] = np.frombuffer(raw[64 + count:], dtype=np.float32).reshape(count, 6)
    return out


def compare_masked(exe, tmp_path):
    for count in (1, 65, 1025):
        x = bc.inputs(count)
        for kind in MASKS:
            mask = mask_of(kind, count)
            for scale_by_q, q_filter in FLAGS:
                got = harness_masked(exe, tmp_path, x, count, mask, scale_by_q, q_filter)
                want = bc.restate(x, count, scale_by_q, q_filter, row_mask=mask)
                where = (count, kind, scale_by_q, q_filter)
                for k in ("critic_loss", "actor_loss", "bc_loss", "bc_weight", "mean_abs", "d_action"):
                    assert same(got[k], want[k]), (where, k)
                assert got["bc_rows"] == want["bc_rows"] and np.array_equal(got["cloned"], want["cloned"]), where
                assert not want["cloned"][mask == 0].any(), where


def test_masked_verdict_equals_the_restatement_bitwise(harness, tmp_path):
    compare_masked(harness, tmp_path)


def test_masked_verdict_is_clean_under_address_and_undefined_sanitizers(sanitized_harness, tmp_path):
    compare_masked(sanitized_harness, tmp_path)


def test_masked_restatement_at_its_two_ends_and_with_excluded_nans():
    count = 1025
    x = bc.inputs(count)
    plain = policy_terms(x["alpha"], dqmin_da=x["dqmin_da"], scale=-1.0 / count, q=x["q"], y=x["y"], log_prob=x["log_prob"], q_min=x["q_min"])
    for scale_by_q, q_filter in FLAGS:
        full = bc.restate(x, count, scale_by_q, q_filter)
        ones = bc.restate(x, count, scale_by_q, q_filter, row_mask=np.ones(count, dtype=np.uint8))
        for k in ("d_action", "critic_loss", "actor_loss", "bc_loss", "bc_weight", "bc_rows", "cloned"):
            assert same(ones[k], full[k]) if ones[k].dtype == np.float32 else np.array_equal(ones[k], full[k]), k  # all ones: the cloned call
        zeros = bc.restate(x, count, scale_by_q, q_filter, row_mask=np.zeros(count, dtype=bool))
        assert same(zeros["d_action"], plain["d_action"]) and same(zeros["critic_loss"], plain["critic_loss"]) and same(zeros["actor_loss"], plain["actor_loss"])
        assert zeros["bc_rows"] == 0 and same(zeros["bc_loss"], np.float32(0.0)) and not np.signbit(zeros["bc_loss"])
        assert same(zeros["bc_weight"], full["bc_weight"])  # still written, and over ALL rows
        # a NaN in action_data of a row the mask excludes reaches no output
        mask = mask_of("prefix64", count)
        y = {k: np.array(v, copy=True) for k, v in x.items()}
        y["action_data"][64:] = np.nan
        a, b = bc.restate(x, count, scale_by_q, q_filter, row_mask=mask), bc.restate(y, count, scale_by_q, q_filter, row_mask=mask)
        for k in ("d_action", "bc_loss", "bc_weight", "critic_loss", "actor_loss"):
            assert same(a[k], b[k]) and np.isfinite(b[k]).all(), k
    for bad in (np.ones(count - 1, dtype=np.uint8), np.ones(count, dtype=np.int32), np.ones((count, 1), dtype=np.uint8)):
        with pytest.raises(ValueError, match="row_mask"):
            bc.restate(x, count, False, False, row_mask=bad)


def test_structs_mirror_the_header(harness):
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    layout = json.loads(subprocess.run([harness, "layout"], capture_output=True, text=True, check=True).stdout)
    ctype = {"urgym_replay_ring": _abi.ReplayRing, "urgym_replay_demonstrations": _abi.ReplayDemonstrations, "int32_t": C.c_int32, "uint8_t*": C.POINTER(C.c_uint8)}
    for name, mirror in (("urgym_replay_demonstrations", _abi.ReplayDemonstrations), ("urgym_sac_demonstrating", _abi.SacDemonstrating)):
        body = hdr[hdr.index(f"typedef struct {name} {{"):hdr.index(f"}} {name};")]
        declared = re.findall(r"^\s*(urgym_replay_ring|urgym_replay_demonstrations|uint8_t\*|int32_t)\s+(\w+);", body, flags=re.M)
        assert [(f, ctype[t]) for t, f in declared] == list(mirror._fields_), name  # the header's order and types are the mirror's
        want = layout[name]
        assert C.sizeof(mirror) == want.pop("sizeof"), name
        assert {f: getattr(mirror, f).offset for f, _ in mirror._fields_} == want, name  # the C compiler's own offsets
    assert C.sizeof(_abi.ReplayDemonstrations) == C.sizeof(_abi.ReplayRing) + 16 and C.sizeof(_abi.SacDemonstrating) == C.sizeof(_abi.ReplayDemonstrations) + 16
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    assert re.search(r"^#define URGYM_DEMO_TAG 0x44454D00u", hdr, flags=re.M)
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    assert lib.urgym_abi_version() == 4
    for text in ("counter (i, draw lo, draw hi, URGYM_DEMO_TAG)", "slot = (oldest_d + e / N_d) % C_d", "cloned[m] = row_mask[m] != 0 && (q_filter ? qd > q_min[m] : true)",
                 "the running\n * statistics still come from the learner's own collection only"):
        assert text in hdr, text


def test_training_entry_dispatch():
    # the table stays what it was; the new entry is tried ahead of it and only where the option is given
    assert len(_SAC_TRAIN_ENTRIES) == 10 and all("demonstrating" not in opts for _, _, opts in _SAC_TRAIN_ENTRIES)
    for present in (set(), {"cloning"}, {"planner", "noise", "cloning"}, {"normalizer", "clipping"}, {"monitor", "evaluation"}):
        symbol, options = _sac_train_entry(present | {"demonstrating"})
        assert symbol == "urgym_sac_train_demonstrated" and options[0] == "demonstrating" and present <= set(options)
        assert not {"nstep", "prioritized", "hindsight"} & set(options)
        assert _sac_train_entry(present)[0] != "urgym_sac_train_demonstrated"
    symbol, options = _sac_train_entry({"demonstrating"})
    argtypes = _native.lib().urgym_sac_train_demonstrated.argtypes
    mirrors = dict(demonstrating=_abi.SacDemonstrating, cloning=_abi.SacCloning, planner=_abi.SacPlanning, temper=_abi.MppiTemper, noise=_abi.MppiNoise,
                   normalizer=_abi.Normalization, clipping=_abi.SacClipping, evaluation=_abi.SacEvaluation, monitor=_abi.SacMonitoring)
    assert len(argtypes) == len(options) + 4 and [argtypes[3 + i] for i in range(len(options))] == [C.POINTER(mirrors[o]) for o in options]


def test_refusals_that_need_no_device():
    lib = _native.lib()
    fn = lib.urgym_replay_sample_mixed
    assert fn(None, C.byref(_abi.ReplayRing()), 0, 1, 0, 0, 1, C.byref(_abi.ReplayBatch()), C.byref(_abi.ReplayDemonstrations()), None, None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert fn(None, None, 0, 0, 0, 0, 0, None, None, None, None) == _abi.ERR_ARG
    fn = lib.urgym_sac_policy_terms_cloned_masked
    assert fn(None, C.byref(_abi.SacPolicyArgs()), C.byref(_abi.SacCloneArgs()), None, None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    fn = lib.urgym_sac_train_demonstrated
    assert fn(None, C.byref(_abi.SacLearner()), C.byref(_abi.SacSchedule()), C.byref(_abi.SacDemonstrating()), *[None] * 9) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert fn(*[None] * len(fn.argtypes)) == _abi.ERR_ARG


def host_env(num_envs):
    return types.SimpleNamespace(num_envs=num_envs, obs_dim=5, goal_dim=3, device="cpu")


def test_ring_file_round_trip(tmp_path):
    import torch

    ring = DeviceReplay(host_env(3), 4)
    rng = np.random.default_rng(4)
    for name, t in ring.ring.items():
        t.copy_(torch.from_numpy(rng.integers(0, 2, tuple(t.shape)).astype(np.uint8) if t.dtype == torch.uint8 else rng.standard_normal(tuple(t.shape)).astype(np.float32)))
    ring.cursor, ring.filled = 1, 3  # oldest_slot 2: the valid slots wrap
    path = str(tmp_path / "demos.npz")
    ring.save(path)
    assert not os.path.exists(checkpoint.temporary_name(path))
    with np.load(path, allow_pickle=False) as z:
        assert checkpoint.META_KEY in z.files
    back = DeviceReplay(host_env(3), 4)
    back.load_file(path)
    assert (back.cursor, back.filled, back.oldest_slot) == (1, 3, 2)
    for name, t in ring.ring.items():
        for slot in (2, 3, 0):
            assert torch.equal(back.ring[name][slot].view(torch.uint8), t[slot].view(torch.uint8)), (name, slot)
        assert not back.ring[name][1].any()  # the slot that is not valid stays as it was
    with pytest.raises(ValueError, match="num_envs is 3 in the state, 2 here"):
        DeviceReplay(host_env(2), 4).load_file(path)
    with pytest.raises(ValueError, match="capacity is 4 in the state, 5 here"):
        DeviceReplay(host_env(3), 5).load_file(path)
    other = str(tmp_path / "other.npz")
    checkpoint.write(other, dict(learner=None))
    with pytest.raises(ValueError, match="not a file of DeviceReplay.save"):
        back.load_file(other)
    with pytest.raises(ValueError):  # an empty ring holds no demonstration
        DeviceReplay(host_env(3), 4).demonstrations_struct(1)
    d = ring.demonstrations_struct(2)
    assert (d.num_envs, d.oldest_slot, d.filled_steps, d.count, d.ring.capacity_steps) == (3, 2, 3, 2, 4)


def test_learner_option_and_the_checkpoint_rule_for_demonstrations():
    assert DEMO_DEFAULTS == dict(demo_batch_size=None, bc_demo_only=False)
    assert not set(DEMO_DEFAULTS) & (set(SAC_DEFAULTS) | set(PER_DEFAULTS) | set(HER_DEFAULTS) | set(CLIP_DEFAULTS) | set(NORM_DEFAULTS) | set(BC_DEFAULTS))
    plain = assembled_learner()
    demo = assembled_learner(**DEVICE, bc_weight=0.5, demo_batch_size=17, bc_demo_only=True)
    for L in (plain, assembled_learner(**DEMO_DEFAULTS), assembled_learner(**DEVICE, bc_weight=0.5)):  # without the option: no new key
        assert not set(DEMO_DEFAULTS) & set(L._saved_hp())
    assert {k: demo._saved_hp()[k] for k in DEMO_DEFAULTS} == dict(demo_batch_size=17, bc_demo_only=True)
    assert assembled_learner(**DEVICE, demo_batch_size=0)._saved_hp()["demo_batch_size"] == 0  # D = 0 is the option, set
    state = dict(learner_state(demo), hp=demo._saved_hp())
    arrays, tree = checkpoint.flatten(state)
    back = checkpoint.unflatten(arrays, json.loads(json.dumps(tree)))
    demo.check_state_dict(back)
    plain.check_state_dict(dict(learner_state(plain), hp=plain._saved_hp()))
    with pytest.raises(ValueError, match="demo_batch_size is 17 in the checkpoint, None here"):
        assembled_learner(**DEVICE, bc_weight=0.5).check_state_dict(back)
    with pytest.raises(ValueError, match="demo_batch_size is None in the checkpoint, 17 here"):
        demo.check_state_dict(dict(learner_state(demo), hp={k: v for k, v in demo._saved_hp().items() if k not in DEMO_DEFAULTS}))
    with pytest.raises(ValueError, match="demo_batch_size is 17 in the checkpoint, 65 here"):
        assembled_learner(**DEVICE, bc_weight=0.5, demo_batch_size=65, bc_demo_only=True).check_state_dict(back)
    with pytest.raises(ValueError, match="bc_demo_only is True in the checkpoint, False here"):
        assembled_learner(**DEVICE, bc_weight=0.5, demo_batch_size=17).check_state_dict(back)
    with pytest.raises(ValueError, match="only"):
        demo.check_state_dict(back, override=("demo_batch_size",))
    # the constructor's refusals, before it touches the environment
    ring = object()
    with pytest.raises(ValueError, match="demo_batch_size needs device_entropy=True"):
        SACLearner(None, demonstrations=ring, demo_batch_size=4)
    with pytest.raises(ValueError, match="demonstrations= needs demo_batch_size"):
        SACLearner(None, **DEVICE, demonstrations=ring)
    with pytest.raises(ValueError, match="demo_batch_size needs demonstrations="):
        SACLearner(None, **DEVICE, demo_batch_size=4)
    for bad in (-1, 257, 1.0, True, "4"):
        with pytest.raises(ValueError, match="demo_batch_size must be"):
            SACLearner(None, **DEVICE, demonstrations=ring, demo_batch_size=bad)
    with pytest.raises(ValueError, match="bc_demo_only needs bc_weight"):
        SACLearner(None, **DEVICE, demonstrations=ring, demo_batch_size=4, bc_demo_only=True)
    with pytest.raises(ValueError, match="bc_demo_only qualifies demo_batch_size and needs it"):
        SACLearner(None, **DEVICE, bc_weight=1.0, bc_demo_only=True)
    with pytest.raises(ValueError, match="bc_demo_only must be True or False"):
        SACLearner(None, **DEVICE, demonstrations=ring, demo_batch_size=4, bc_weight=1.0, bc_demo_only=1)
    for pair in (dict(n_steps=3), dict(prioritized=True), dict(hindsight=True)):
        with pytest.raises(ValueError, match="out of scope: each of the three has a gather of its own"):
            SACLearner(None, **DEVICE, demonstrations=ring, demo_batch_size=4, **pair)
    with pytest.raises(TypeError, match="demo_batch_size"):  # the list of what is available names the new options
        SACLearner(None, demo_batch_sise=4)
