"""CPU tests (-m "not gpu") of the planner-driven collection.

  * tests/mppi_collect_harness.cpp, a stand-alone host program around ur_gym_amd/csrc/urgym_mppi_collect.h -- the header the kernel
    compiles -- equals the numpy restatements of ur_gym_amd.evaluation: the words of the two exploration counters
    (mppi_explore_counters), which block and word a component's pair reads, and the execute line (mppi_execute) bitwise with a clamp
    that acts on both sides, sigma 0 with action_out = -0.0 (a byte copy, nothing drawn), and a NaN in action_out that reaches its own
    element only.  Built a second time with -fsanitize=address,undefined and run as that program.
  * the exploration counters (blocks 2, 3) meet none of the planner's sample counters over i < 8, h < 64, j < 1024.
  * the ctypes mirror of urgym_mppi_explore against the C compiler's own layout, the two new symbols, the refusals that need no device.
"""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from mppi_collect_cases import COUNTER_POINTS, DRAW, E, E_WIDE, SEED, SIGMAS, action_rows, noise_bound, poisoned
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import (DeviceMPPI, _box_muller, _noise_integers, mppi_actions, mppi_execute, mppi_explore_counters, mppi_explore_noise,
                                   philox4x32_10)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
SYMBOLS = ("urgym_mppi_execute", "urgym_mppi_collect")


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "mppi_collect_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h")] + [os.path.join(CSRC, h) for h in ("urgym_mppi_collect.h", "urgym_mppi.h", "urgym_sac_terms.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("mppi_collect_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("mppi_collect_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run_harness(exe, *args):
    run = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (args, run.returncode, run.stdout[-500:], run.stderr[-2000:])
    return json.loads(run.stdout) if run.stdout else None


def bits32(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def through(exe, tmp_path, mode, arrays, args, out):
    """Runs `mode` on the bytes of `arrays`; returns the arrays of FILE.out, `out` being (dtype, shape) in file order."""
    path = os.path.join(str(tmp_path), mode + ".bin")
    with open(path, "wb") as f:
        f.write(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays))
    run_harness(exe, mode, path, *args)
    data, got, at = open(path + ".out", "rb").read(), [], 0
    for dtype, shape in out:
        size = int(np.prod(shape)) * np.dtype(dtype).itemsize
        got.append(np.frombuffer(data[at:at + size], dtype).reshape(shape))
        at += size
    assert at == len(data), (mode, at, len(data))
    return got


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def compare_counters(exe):
    for p, draw in COUNTER_POINTS:
        got = run_harness(exe, "counter", p, draw)
        want = [[int(np.asarray(w)) for w in c] for c in mppi_explore_counters(draw, p)]
        assert got["counters"] == want, (p, draw, got, want)
        assert want == [[p, 0, draw, _abi.MPPI_TAG | 2], [p, 0, draw, _abi.MPPI_TAG | 3]]
        # component c is the cosine (c even) or the sine of pair c // 2, whose words are 2 (c // 2) and the next of w0 .. w5:
        # w0 .. w3 are block 2's, w4 and w5 block 3's -- the order _noise_integers and _box_muller take them in
        assert got["block_of"] == [2, 2, 2, 2, 3, 3] and got["first_word"] == [0, 0, 2, 2, 0, 0]
    with pytest.raises(ValueError):
        mppi_explore_counters(1 << 32, 0)
    # the restated noise is Box-Muller on exactly those words
    key = (SEED & 0xFFFFFFFF, SEED >> 32)
    c2, c3 = mppi_explore_counters(DRAW, np.arange(E_WIDE))
    want = _box_muller(_noise_integers(philox4x32_10(key, c2), philox4x32_10(key, c3), np.float32), np.float32)
    assert same_bits(mppi_explore_noise(SEED, DRAW, np.arange(E_WIDE)), want) and want.shape == (E_WIDE, 6)


def compare_execute(exe, tmp_path):
    for e in (E, E_WIDE):
        action = action_rows(e)
        eps = mppi_explore_noise(SEED, DRAW, np.arange(e))
        for rows, nan in ((action, np.zeros(action.shape, bool)), poisoned(action)):
            for sigma in SIGMAS:
                want = mppi_execute(rows, eps, sigma)
                got, out_eps, drew = through(exe, tmp_path, "execute", [rows, eps], [e, bits32(sigma)], [(np.float32, (e, 6)), (np.float32, (e, 6)), (np.uint8, (e, 6))])
                where = (e, sigma, bool(nan.any()))
                assert same_bits(got, want), where
                if sigma == 0.0:  # a byte copy: -0.0 stays -0.0, a NaN keeps its payload, no word is drawn, explore_eps is 0
                    assert same_bits(got, rows) and np.signbit(got[0, 0]) and np.signbit(got[e - 1, 5]) and not drew.any() and same_bits(out_eps, np.zeros((e, 6), np.float32)), where
                    assert same_bits(mppi_execute(rows, None, 0.0), rows)
                    continue
                assert drew.all() and same_bits(out_eps, eps), where
                assert np.abs(got[~nan]).max() <= 1.0 and not np.isnan(got[~nan]).any(), where
                # a NaN reaches its own element only: every other element is what the clean rows give
                assert same_bits(got[~nan], mppi_execute(action, eps, sigma)[~nan]), where
                # the line is the sample launch's with action_out in place of the mean
                assert same_bits(want, mppi_actions(rows[None], eps[None], sigma)[0]), where
                if sigma == 25.0:  # the clamp acts on both sides
                    assert (got == 1).any() and (got == -1).any() and (e < E_WIDE or ((got == 1).mean() > 0.3 and (got == -1).mean() > 0.3)), where
    for bad in (dict(action_out=np.zeros((3, 6), np.float64)), dict(action_out=np.zeros((3, 5), np.float32)), dict(eps=np.zeros((2, 6), np.float32)),
                dict(explore_sigma=-0.1), dict(explore_sigma=float("nan")), dict(explore_sigma=float("inf"))):
        args = dict(action_out=np.zeros((3, 6), np.float32), eps=np.zeros((3, 6), np.float32), explore_sigma=0.3)
        args.update(bad)
        with pytest.raises(ValueError):
            mppi_execute(**args)


def test_harness_equals_numpy(harness, tmp_path):
    compare_counters(harness)
    compare_execute(harness, tmp_path)


def test_sanitized_harness(sanitized_harness, tmp_path):
    """The same comparisons on the program built with -fsanitize=address,undefined: any finding ends it with a non-zero status."""
    compare_counters(sanitized_harness)
    compare_execute(sanitized_harness, tmp_path)
    assert run_harness(sanitized_harness, "meet", 2, 7)["met"] == 0


def test_exploration_counters_meet_no_sample_counter(harness):
    """Blocks 2 and 3 against the planner's blocks 0 and 1 over every (i, h, j) the planner can name, for a few (p, draw) -- among them
    p = 0, draw = 0, where the sample counter of (i, h, j) = (0, 0, 0) differs from the exploration counter in word 3 alone."""
    for p, draw in COUNTER_POINTS:
        got = run_harness(harness, "meet", p, draw)
        assert got == {"compared": 8 * 64 * 1024 * 2 * 2, "met": 0}, (p, draw, got)
    # and in the restatement: word 3 of every exploration counter is the tag with block 2 or 3, that of the sample noise block 0 or 1
    assert [int(c[3]) for c in mppi_explore_counters(0, 0)] == [_abi.MPPI_TAG | 2, _abi.MPPI_TAG | 3] and _abi.MPPI_TAG & 0xFF == 0
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    assert re.search(r"^#define URGYM_MPPI_EXPLORE_BLOCK 2$", hdr, flags=re.M) and _abi.MPPI_EXPLORE_BLOCK == 2


def test_noise_restatement_is_within_the_planners_bound():
    """numpy's float32 evaluation of the exploration noise against its float64 one, within the bound the planner's eps is held to."""
    f32, f64 = (mppi_explore_noise(SEED, DRAW, np.arange(E_WIDE), dtype=t) for t in (np.float32, np.float64))
    assert f32.dtype == np.float32 and f64.dtype == np.float64
    assert float(np.abs(f32.astype(np.float64) - f64).max()) <= noise_bound()
    assert abs(float(f64.mean())) < 0.15 and 0.85 < float(f64.std()) < 1.15  # 1026 standard normals
    assert same_bits(mppi_explore_noise(SEED, DRAW, 0), f32[0]) and same_bits(mppi_explore_noise(SEED, DRAW, np.arange(E)), f32[:E])  # not a function of E
    assert not same_bits(mppi_explore_noise(SEED, DRAW - 1, np.arange(E)), f32[:E]) and not same_bits(mppi_explore_noise(SEED + 1, DRAW, np.arange(E)), f32[:E])


def test_struct_mirror_and_symbols(harness):
    lay = run_harness(harness, "layout")
    assert lay.pop("sizeof") == C.sizeof(_abi.MppiExplore) == 16
    assert lay == {name: getattr(_abi.MppiExplore, name).offset for name, _ in _abi.MppiExplore._fields_}
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    body = hdr[hdr.index("typedef struct urgym_mppi_explore {"):hdr.index("} urgym_mppi_explore;")]
    assert re.findall(r"^\s*(?:int32_t|float)\*?\s+(\w+);", body, flags=re.M) == [name for name, _ in _abi.MppiExplore._fields_]
    lib = _native.lib()
    for sym in SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    assert lib.urgym_abi_version() == _abi.ABI_VERSION == 4  # found by lookup, within the version


def test_refusals_without_a_device():
    """A NULL handle is refused by both entry points before anything else is looked at; the Python layers refuse a bad explore_sigma and a
    planner with normalize before they touch a device."""
    lib = _native.lib()
    m, x, ring = _abi.Mppi(), _abi.MppiExplore(), _abi.ReplayRing()
    out = (C.c_float * 6)()
    for call, args in ((lib.urgym_mppi_execute, (None, C.byref(m), C.byref(x), 0, C.cast(out, C.c_void_p), None)),
                       (lib.urgym_mppi_collect, (None, None, C.byref(m), None, C.byref(x), 0, 1, C.byref(ring), 0, None))):
        assert call(*args) == _abi.ERR_ARG and b"null handle" in lib.urgym_last_error(None)
    assert not any(out)
    for bad in (-0.5, float("nan"), float("inf"), 1e39, True):
        with pytest.raises(ValueError):
            DeviceMPPI.check_explore(bad)
    assert DeviceMPPI.check_explore(0) == 0.0 and DeviceMPPI.check_explore(0.25) == 0.25
