"""CPU tests (-m "not gpu") of the prioritized replay.

  * tests/per_harness.cpp, a stand-alone host program around ur_gym_amd/csrc/urgym_per.h -- the functions the kernels compile -- equals
    evaluation.per_sums / per_descent / per_beta bit for bit, with fan-out 4 (four and five levels, ragged last blocks) and 256; built a
    second time with -fsanitize=address,undefined and run as that program.
  * the share of u-space each leaf takes is leaf / total, in exact rational arithmetic from the level boundaries, on a tree whose every
    sum is exact.
  * the two fallbacks of the descent, each forced by a hand-built tree; the empty structure yields entry 0; a zero leaf is never taken.
  * the ctypes mirrors of the three new structs against the header's text and the C compiler's own layout, the new symbols, the
    refusals that need no device.
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

from per_cases import DRAW, SEED, TREES, leaves, levels_of, same_bits
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import DevicePrioritizedReplay, per_beta, per_descent, per_sums, per_terms, per_words, replay_indices

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
NEW_SYMBOLS = ("urgym_per_sums_count", "urgym_per_rebuild", "urgym_per_fill", "urgym_replay_sample_prioritized", "urgym_per_terms",
               "urgym_sac_train_prioritized")
COUNT = 2000


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "per_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h")] + [os.path.join(CSRC, h) for h in ("urgym_per.h", "urgym_pack_map.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("per_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("per_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run(exe, *args):
    got = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert got.returncode == 0 and not got.stderr, (args, got.returncode, got.stdout[-500:], got.stderr[-2000:])
    return got.stdout


def harness_sums(exe, tmp_path, leaf, fanout):
    src, dst = str(tmp_path / "sums_in.bin"), str(tmp_path / "sums_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<q", leaf.size) + leaf.tobytes())
    run(exe, "sums", fanout, src, dst)
    return np.frombuffer(open(dst, "rb").read(), dtype=np.float64)


def harness_descend(exe, tmp_path, leaf, words, fanout, tree=None):
    src, dst = str(tmp_path / "descend_in.bin"), str(tmp_path / "descend_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<3q", leaf.size, len(words), tree is not None) + leaf.tobytes())
        if tree is not None:
            f.write(np.asarray(tree, np.float64).tobytes())
        f.write(np.asarray(words, np.uint64).tobytes())
    run(exe, "descend", fanout, src, dst)
    return np.frombuffer(open(dst, "rb").read(), dtype=np.int64)


def words_at(u_numerators):
    """Words whose u = (w >> 11) 2^-53 is numerator 2^-53."""
    return np.array([int(a) << 11 for a in u_numerators], dtype=np.uint64)


def compare_with_restatements(exe, tmp_path):
    words = per_words(SEED, DRAW, COUNT)
    edge = words_at([0, 1, (1 << 53) - 1, 1 << 52])  # u = 0, the smallest, the largest, one half
    for name, n, fanout in TREES:
        leaf = leaves(n)
        want = per_sums(leaf, fanout)
        assert [v.size for v in want["levels"]] == levels_of(n, fanout), name
        assert same_bits(harness_sums(exe, tmp_path, leaf, fanout), want["flat"]), name
        w = np.concatenate([words, edge])
        got = harness_descend(exe, tmp_path, leaf, w, fanout)
        assert same_bits(got, per_descent(leaf, w, fanout, sums=want)), name
        assert (leaf[got] > 0).all(), name  # a zero leaf is never taken
    assert len(levels_of(TREES[0][1], 4)) >= 4 and len(levels_of(70000, 256)) == 2 and levels_of(600, 256) == [3]
    # beta
    rows = [(0.4, 1, 100000), (0.4, 50000, 100000), (0.4, 100000, 100000), (0.4, 10 ** 9, 100000), (0.0, 7, 9), (1.0, 3, 1000), (0.25, 1, 1),
            (0.4, 33333, 99999)]
    src, dst = str(tmp_path / "beta_in.bin"), str(tmp_path / "beta_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<q", len(rows)) + b"".join(struct.pack("<dqq", *r) for r in rows))
    run(exe, "beta", src, dst)
    got = np.frombuffer(open(dst, "rb").read(), dtype=np.float32)
    assert same_bits(got, np.array([per_beta(*r) for r in rows], np.float32))
    assert per_beta(0.4, 100000, 100000) == 1 and per_beta(0.4, 10 ** 9, 100000) == 1 and per_beta(0.4, 0, 10) == np.float32(0.4)


def test_harness_equals_the_restatements_bit_for_bit(harness, tmp_path):
    compare_with_restatements(harness, tmp_path)


def test_harness_is_clean_under_address_and_undefined_sanitizers(sanitized_harness, tmp_path):
    compare_with_restatements(sanitized_harness, tmp_path)
    check_fallbacks(sanitized_harness, tmp_path)


def test_sums_are_the_ascending_float64_sums():
    """per_sums against a plain Python loop: float64 additions one at a time, from +0.0."""
    for name, n, fanout in TREES[:5]:
        leaf = leaves(n, seed=1)
        v, got = [float(x) for x in leaf], per_sums(leaf, fanout)
        for level in got["levels"]:
            up = []
            for b in range(0, len(v), fanout):
                s = 0.0
                for x in v[b:b + fanout]:
                    s = s + x
                up.append(s)
            assert same_bits(level, np.array(up, np.float64)), name
            v = up
        s = 0.0
        for x in v:
            s = s + x
        assert got["total"].tobytes() == np.float64(s).tobytes(), name


def test_each_leaf_takes_its_share_of_u_space_exactly(harness, tmp_path):
    """Small integers that sum to 2^10: every sum and t = u total are exact, so leaf j owns exactly the u in [lo_j, hi_j) / total with
    lo_j the leaves before it -- formed here as rationals from the level boundaries -- and hi_j - lo_j = leaf_j."""
    rng = np.random.default_rng(5)
    n, fanout = 37, 4
    leaf = rng.integers(0, 40, n).astype(np.float32)
    leaf[[3, 4, 5, 6, 7, 20]] = 0
    leaf[-1] += 1024 - leaf.sum()
    assert leaf.sum() == 1024 and leaf[-1] > 0
    sums = per_sums(leaf, fanout)
    total = Fraction(float(sums["total"]))
    below = [leaf.astype(np.float64)] + sums["levels"]
    for j in np.nonzero(leaf)[0]:
        lo, node = Fraction(0), int(j)
        for v in below:  # the siblings before the node, at every level
            first = node - node % fanout
            lo += sum(Fraction(float(x)) for x in v[first:node])
            node //= fanout
        hi = lo + Fraction(float(leaf[j]))
        assert (hi - lo) / total == Fraction(float(leaf[j])) / total
        # u = lo / total and the last u below hi / total draw j; the u before lo / total and u = hi / total do not
        scale = Fraction(1 << 53) / total
        inside = [lo * scale, hi * scale - 1]
        outside = [a for a in (lo * scale - 1, hi * scale) if 0 <= a < 1 << 53]
        assert all(a.denominator == 1 for a in inside + outside)
        for draw in (per_descent(leaf, words_at(inside + outside), fanout, sums=sums), harness_descend(harness, tmp_path, leaf, words_at(inside + outside), fanout)):
            assert (draw[:2] == j).all() and (draw[2:] != j).all(), (j, draw)


def check_fallbacks(exe, tmp_path):
    fanout = 4
    leaf = np.array([1, 0, 2, 0, 0, 0, 0, 0, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0], np.float32)  # 5 level-1 entries, 2 level-2 entries
    honest = per_sums(leaf, fanout)
    assert [v.size for v in honest["levels"]] == [5, 2]
    # the last positive child: a total larger than its children's sum puts t past every child at the top, and t stays past every sum
    # below: level 2 -> entry 0 (entry 1 is zero), level 1 -> entry 2 (3 is zero), leaves -> entry 9 (10, 11 are zero)
    tree = honest["flat"].copy()
    tree[-1] = 100.0
    sums = dict(levels=honest["levels"], total=np.float64(100.0), flat=tree)
    w = words_at([(1 << 53) - 1, 1 << 52])
    for got in (harness_descend(exe, tmp_path, leaf, w, fanout, tree=tree), per_descent(leaf, w, fanout, sums=sums)):
        assert got.tolist() == [9, 9]
    # the fallback one level down only: level-1 entry 0 claims 10 where its leaves sum to 3; t in [3, 10) finds no leaf: leaf 2
    tree = honest["flat"].copy()
    tree[0], tree[5], tree[-1] = 10.0, 15.0, 15.0
    levels = [np.array([10.0, 0, 5, 0, 0]), np.array([15.0, 0.0])]
    sums = dict(levels=levels, total=np.float64(15.0), flat=tree)
    assert same_bits(np.concatenate(levels + [[15.0]]), tree)
    w = words_at([(1 << 53) // 15 * 4, (1 << 53) // 15 * 9, 0, (1 << 53) // 15 * 11])  # t about 4, 9, 0, 11
    for got in (harness_descend(exe, tmp_path, leaf, w, fanout, tree=tree), per_descent(leaf, w, fanout, sums=sums)):
        assert got.tolist() == [2, 2, 0, 8]
    # every child zero: the first child at every level, entry 0, whatever the word
    empty = np.zeros(70, np.float32)
    w = np.concatenate([per_words(SEED, DRAW, 50), words_at([0, (1 << 53) - 1])])
    for got in (harness_descend(exe, tmp_path, empty, w, fanout), per_descent(empty, w, fanout)):
        assert not got.any()
    assert not per_sums(empty, fanout)["flat"].any()
    # one positive leaf takes every row
    one = np.zeros(600, np.float32)
    one[517] = 3e-7
    for f in (4, 256):
        for got in (harness_descend(exe, tmp_path, one, w, f), per_descent(one, w, f)):
            assert (got == 517).all()


def test_fallbacks_of_the_descent(harness, tmp_path):
    check_fallbacks(harness, tmp_path)


def test_the_draw_word_is_its_own_stream():
    assert _abi.PER_TAG == 0x50455200 and _abi.PER_TAG not in (_abi.REPLAY_TAG, _abi.NOISE_TAG, _abi.NOISE_TAG | 1, 0, 1, 2, 3, 4)
    w = per_words(SEED, DRAW, 64)
    assert w.dtype == np.uint64 and len(set(w.tolist())) == 64
    assert same_bits(per_words(SEED, DRAW, 1025)[:64], w)  # row i does not depend on count
    # not the uniform draw's words: e = (w size) >> 64 of these would differ from replay_indices
    assert (np.array([(int(x) << 10) >> 64 for x in w]) != replay_indices(SEED, DRAW, 64, 1 << 10)).any()


def test_terms_restatement_properties():
    from per_cases import terms_inputs

    count = 300
    x = terms_inputs(count)
    total, size = np.float64(x["leaf"].astype(np.float64).sum() * 7), 4000
    ones = np.ones(count, np.float32)
    out = per_terms(x["leaf"], total, size, 0.0, x["q"], x["y"], 1.0 / count, 1e-6, 0.6, w_raw=ones)
    # w == 1: dq is the target route's (q - y) * scale, bitwise
    assert same_bits(out["w"], ones) and same_bits(out["dq"], (x["q"] - x["y"][None, :]) * np.float32(1.0 / count))
    # the write-back: duplicates end at the largest value, max_leaf is monotone
    index = np.arange(count, dtype=np.int64) % 7
    new_leaf = np.abs(x["y"]) + np.float32(0.5)
    leaf = np.full((5, 4), 9.0, np.float32)
    out = per_terms(x["leaf"], total, size, 0.4, x["q"], x["y"], 1.0 / count, 1e-6, 0.6, w_raw=ones, new_leaf=new_leaf, index=index, leaf=leaf, max_leaf=2.0)
    for k in range(7):
        assert out["leaf"].reshape(-1)[k] == new_leaf[k::7].max()
    assert (out["leaf"].reshape(-1)[7:] == 9).all() and out["max_leaf"] == max(np.float32(2.0), new_leaf.max())
    assert per_terms(x["leaf"], total, size, 0.4, x["q"], x["y"], 1.0, 1e-6, 0.6, w_raw=ones, new_leaf=ones * np.float32(0.1), index=index, leaf=leaf,
                     max_leaf=2.0)["max_leaf"] == 2
    q = x["q"].copy()
    q[:, 5] = np.nan
    out = per_terms(x["leaf"], total, size, 0.4, q, x["y"], 1.0, 1e-6, 0.6, w_raw=ones)
    assert out["replaced"].nonzero()[0].tolist() == [5] and np.isnan(out["dq"][:, 5]).all() and np.isfinite(np.delete(out["dq"], 5, axis=1)).all()


def test_structs_mirror_the_header(harness):
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    layout = json.loads(run(harness, "layout"))
    for name, mirror in (("urgym_per_priorities", _abi.PerPriorities), ("urgym_per_terms_args", _abi.PerTermsArgs), ("urgym_sac_prioritized", _abi.SacPrioritized)):
        body = hdr[hdr.index(f"typedef struct {name} {{"):hdr.index(f"}} {name};")]
        declared = re.findall(r"^\s*(?:const\s+)?\w+\*?\s+(\w+);", body, flags=re.M)
        assert declared == [f for f, _ in mirror._fields_], name  # the header's order is the mirror's
        want = layout[name]
        assert C.sizeof(mirror) == want.pop("sizeof"), name
        assert {f: getattr(mirror, f).offset for f, _ in mirror._fields_} == want, name  # the C compiler's own offsets
    assert _abi.ABI_VERSION == 4 and "#define URGYM_ABI_VERSION 4" in hdr  # added within version 4
    assert f"#define URGYM_PER_FANOUT {_abi.PER_FANOUT}" in hdr and f"#define URGYM_PER_TERMS_MAX_COUNT {_abi.PER_TERMS_MAX_COUNT}" in hdr
    assert "0x%08X" % _abi.PER_TAG in hdr
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    assert lib.urgym_abi_version() == 4


def test_refusals_that_need_no_device():
    lib = _native.lib()
    n = C.c_uint64(0)
    assert lib.urgym_per_sums_count(None, 4, C.byref(n)) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert lib.urgym_per_rebuild(None, C.byref(_abi.PerPriorities()), None) == _abi.ERR_ARG
    assert lib.urgym_per_fill(None, C.byref(_abi.PerPriorities()), 0, 1, None) == _abi.ERR_ARG
    assert lib.urgym_replay_sample_prioritized(None, None, None, 0, 0, 1, None, None, None, None) == _abi.ERR_ARG
    assert lib.urgym_per_terms(None, C.byref(_abi.PerTermsArgs()), None) == _abi.ERR_ARG
    assert lib.urgym_sac_train_prioritized(None, C.byref(_abi.SacLearner()), C.byref(_abi.SacSchedule()), C.byref(_abi.SacPrioritized()), None, None, None) == _abi.ERR_ARG
    for bad in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=np.nan), dict(eps=0.0), dict(eps=-1e-6), dict(eps=np.inf), dict(eps=np.nan)):
        with pytest.raises(ValueError):
            DevicePrioritizedReplay.check_per_args(**dict(dict(alpha=0.6, eps=1e-6), **bad))
    assert DevicePrioritizedReplay.check_per_args(0.0, 1e-6) == (0.0, 1e-6) and DevicePrioritizedReplay.check_per_args(1, 1.0) == (1.0, 1.0)
    with pytest.raises(ValueError):
        per_sums(np.zeros(4, np.float64))


def test_checkpoint_keys_round_trip_and_are_absent_without_priorities(tmp_path, monkeypatch):
    import torch

    from test_checkpoint_host import assembled_learner, fill_ring, learner_state, stand_in_env
    from ur_gym_amd import checkpoint
    from ur_gym_amd.evaluation import DeviceReplay
    from ur_gym_amd.training import PER_DEFAULTS, SAC_DEFAULTS, SACLearner

    # ---- the learner: the three options are saved only where prioritized is on, and a mismatch either way is named
    assert PER_DEFAULTS == dict(prioritized=False, per_beta=0.4, per_beta_steps=100000) and not set(PER_DEFAULTS) & set(SAC_DEFAULTS)
    off, on = assembled_learner(), assembled_learner(prioritized=True, per_beta=0.5, per_beta_steps=1000)
    assert not set(PER_DEFAULTS) & set(off._saved_hp()) and {k: on._saved_hp()[k] for k in PER_DEFAULTS} == dict(prioritized=True, per_beta=0.5, per_beta_steps=1000)
    assert not set(PER_DEFAULTS) & set(assembled_learner(prioritized=False, per_beta=0.9)._saved_hp())
    state_off, state_on = dict(learner_state(off), hp=off._saved_hp()), dict(learner_state(on), hp=on._saved_hp())
    off.check_state_dict(state_off), on.check_state_dict(state_on)
    with pytest.raises(ValueError, match="prioritized is False in the checkpoint, True here"):
        on.check_state_dict(state_off)
    with pytest.raises(ValueError, match="prioritized is True in the checkpoint, False here"):
        off.check_state_dict(state_on)
    with pytest.raises(ValueError, match="per_beta_steps is 1000 in the checkpoint, 7 here"):
        assembled_learner(prioritized=True, per_beta=0.5, per_beta_steps=7).check_state_dict(state_on)
    with pytest.raises(ValueError, match="only"):
        on.check_state_dict(state_on, override=("per_beta",))
    for bad in (dict(prioritized=True), dict(prioritized=True, n_steps=3), dict(prioritized="yes")):  # before the environment is touched
        with pytest.raises(ValueError):
            SACLearner(None, **bad)
    with pytest.raises(TypeError, match="unknown"):
        SACLearner(None, per_gamma=1)

    # ---- the ring: leaves, max_leaf, alpha and eps are saved, the sums are rebuilt; a uniform ring's state holds no such key
    def rebuild(self):  # the device's rebuild, restated: what load_state_dict must leave
        self.sums.copy_(torch.from_numpy(per_sums(self.leaf.numpy())["flat"]))

    monkeypatch.setattr(DevicePrioritizedReplay, "rebuild", rebuild)

    def ring(alpha=0.6, eps=1e-6):
        r = object.__new__(DevicePrioritizedReplay)
        DeviceReplay.__init__(r, stand_in_env(), 4)
        r.alpha, r.eps = DevicePrioritizedReplay.check_per_args(alpha, eps)
        r.leaf, r.max_leaf = torch.zeros((4, 8)), torch.ones(1)
        r.sums = torch.zeros(per_sums(np.zeros(32, np.float32))["flat"].size, dtype=torch.float64)
        return r

    rng = np.random.default_rng(8)
    a, b = ring(), ring()
    fill_ring(a, rng, 2, 4), fill_ring(b, rng, 1, 1)
    a.leaf.copy_(torch.from_numpy(leaves(32, seed=4).reshape(4, 8))), a.max_leaf.fill_(17.5), a.rebuild()
    b.leaf.fill_(3), b.max_leaf.fill_(2), b.sums.fill_(9)
    path = tmp_path / "ring.npz"
    checkpoint.write(path, dict(replay=a.state_dict()))
    state = checkpoint.read(path)["replay"]
    assert sorted(state["priorities"]) == ["alpha", "eps", "leaf", "max_leaf"]  # no sums
    b.load_state_dict(state)
    for name in ("leaf", "max_leaf", "sums"):
        assert same_bits(getattr(a, name).numpy(), getattr(b, name).numpy()), name
    assert (b.cursor, b.filled) == (2, 4) and all(same_bits(a.ring[k].numpy(), b.ring[k].numpy()) for k in a.ring)
    assert "priorities" not in DeviceReplay(stand_in_env(), 4).state_dict()
    for other in (ring(alpha=0.5), ring(eps=1e-3)):
        with pytest.raises(ValueError, match="in the state"):
            other.check_state_dict(state)
    with pytest.raises(ValueError, match="holds no priorities"):
        b.check_state_dict(DeviceReplay(stand_in_env(), 4).state_dict())
    empty = a.state_dict(include_data=False)
    b.load_state_dict(empty)
    assert b.filled == 0 and not b.leaf.any() and not b.sums.any() and b.max_leaf.item() == 17.5
