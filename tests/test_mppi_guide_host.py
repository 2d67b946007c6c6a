"""CPU tests (-m "not gpu") of the guided MPPI planner.

  * tests/mppi_guide_harness.cpp, a stand-alone host program around ur_gym_amd/csrc/urgym_mppi_guide.h -- the header the kernels compile
    -- equals the numpy restatements of ur_gym_amd.evaluation bitwise: the guided action line (mppi_guided_actions) with P = 0, 1 and
    K - 1, and the terminal step (mppi_terminal) on a live future, an ended success, an ended failure, v = 0 with ret = -0.0, and a NaN
    value in a dead and in a live future.  Built a second time with -fsanitize=address,undefined and run as that program.
  * the ctypes mirror of urgym_mppi_guide against the C compiler's own layout, the four new symbols, the refusals that need no device.
"""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from mppi_guide_cases import E, FAIL_COSTS, GAMMAS, H, STEP_SAMPLES, guide_rows, policy_samples, terminal_lanes
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import mppi_actions, mppi_guided_actions, mppi_terminal

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
SYMBOLS = ("urgym_mppi_guide_actions", "urgym_mppi_terminal", "urgym_mppi_plan_guided", "urgym_mppi_control_guided")


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "mppi_guide_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h")] + [os.path.join(CSRC, h) for h in ("urgym_mppi_guide.h", "urgym_mppi.h", "urgym_sac_terms.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("mppi_guide_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("mppi_guide_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run_harness(exe, *args):
    run = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (args, run.returncode, run.stdout[-500:], run.stderr[-2000:])
    return json.loads(run.stdout) if run.stdout else None


def bits64(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


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


def compare_guide(exe, tmp_path):
    for k in STEP_SAMPLES:
        n = E * k
        actions, policy, eps = guide_rows(H, n, k)
        j = np.arange(n) % k
        for p in policy_samples(k):
            for sigma in (0.0, 0.3, 25.0):
                want = mppi_guided_actions(actions, policy, eps, sigma, k, p)
                (got,) = through(exe, tmp_path, "guide", [actions, policy, eps], [H, n, k, p, bits32(sigma)], [(np.float32, actions.shape)])
                assert same_bits(got, want), (k, p, sigma)
                guided = (j >= 1) & (j <= p)
                assert guided.sum() == E * p and same_bits(want[:, ~guided], actions[:, ~guided]), (k, p)  # sample 0 and j > P are not written
                if p:
                    assert np.abs(want[:, guided]).max() <= 1.0
                    # the line is the sample launch's with the actor's output in place of the mean
                    line = mppi_actions(policy[:, guided].reshape(H, -1, 6), eps[:, guided].reshape(H, -1, 6), sigma)
                    assert same_bits(want[:, guided], line), (k, p, sigma)
                    if sigma == 0.0:
                        assert same_bits(want[:, guided], policy[:, guided])
                    if sigma == 25.0:  # the clamp acts on both sides
                        assert (want[:, guided] == 1).mean() > 0.3 and (want[:, guided] == -1).mean() > 0.3
                else:
                    assert same_bits(want, actions)
        # one policy_action row for every horizon step is the same as that row repeated
        assert same_bits(mppi_guided_actions(actions, policy[0], eps, 0.3, k, 1), mppi_guided_actions(actions, np.repeat(policy[:1], H, axis=0), eps, 0.3, k, 1))
    for bad in (dict(policy_samples=5), dict(policy_samples=-1), dict(samples=4), dict(policy_action=np.zeros((2, 15, 6), np.float32)),
                dict(eps=np.zeros((H, 15, 6), np.float64))):
        actions, policy, eps = guide_rows(H, 15, 0)
        args = dict(actions=actions, policy_action=policy, eps=eps, policy_sigma=0.1, samples=5, policy_samples=2)
        args.update(bad)
        with pytest.raises(ValueError):
            mppi_guided_actions(**args)


def compare_terminal(exe, tmp_path):
    for gamma in GAMMAS:
        score, value, nan_alive = terminal_lanes(gamma)
        n = value.size
        alive, success, ret, g = score["alive"] != 0, score["success"] != 0, score["ret"], score["g"]
        for terminal_value in (0, 1):
            for fail_cost in FAIL_COSTS:
                want = mppi_terminal(score, value if terminal_value else None, terminal_value, fail_cost)
                term, new, read = through(exe, tmp_path, "terminal", [ret, g, score["alive"], score["success"], value], [n, terminal_value, bits64(fail_cost)],
                                          [(np.float64, (n,)), (np.float64, (n,)), (np.uint8, (n,))])
                where = (gamma, terminal_value, fail_cost)
                assert same_bits(term, want["terminal"]) and same_bits(new, want["ret"]), (where, term, want)
                assert same_bits(read.astype(bool), alive & bool(terminal_value)), where  # the value of an ended future is not read
                t = want["terminal"]
                assert same_bits(t[~alive & success], np.zeros((~alive & success).sum())), where           # an ended success: +0
                assert same_bits(t[~alive & ~success], np.full((~alive & ~success).sum(), -np.float64(fail_cost))), where  # an ended failure
                assert same_bits(t[alive], value[alive].astype(np.float64) if terminal_value else np.zeros(alive.sum())), where  # a live future
                untouched = ~(t != 0)
                assert same_bits(new[untouched], ret[untouched]) and np.signbit(new[[4, 8]]).all(), where  # v == 0 leaves ret = -0.0 as it is
                assert np.signbit(new[3]) == (not terminal_value), where
                assert np.isnan(new).sum() == (nan_alive.size if terminal_value else 0) and np.isnan(new[nan_alive]).all() == bool(terminal_value), where
                dead_nan = ~alive & np.isnan(value)
                assert dead_nan.sum() == 2 and np.isfinite(new[dead_nan]).all() and np.isfinite(t[dead_nan]).all(), where  # reaches nothing
                # lane 2 ended at step 1: its cost is discounted by gamma^2; lane 0 is alive: its value by gamma^H
                g2 = np.float64(gamma) * np.float64(gamma)
                assert new[2] == (ret[2] + g2 * -np.float64(fail_cost) if fail_cost else ret[2]), where
                gh = np.float64(1.0)
                for _ in range(H):
                    gh = gh * np.float64(gamma)
                assert new[0] == (ret[0] + gh * np.float64(value[0]) if terminal_value else ret[0]), where
    with pytest.raises(ValueError):
        mppi_terminal(score, value[:-1], 1, 0.0)


def test_harness_equals_numpy(harness, tmp_path):
    compare_guide(harness, tmp_path)
    compare_terminal(harness, tmp_path)


def test_sanitized_harness(sanitized_harness, tmp_path):
    """The same comparisons on the program built with -fsanitize=address,undefined: any finding ends it with a non-zero status."""
    compare_guide(sanitized_harness, tmp_path)
    compare_terminal(sanitized_harness, tmp_path)


def test_struct_mirror_and_symbols(harness):
    lay = run_harness(harness, "layout")
    assert lay.pop("sizeof") == C.sizeof(_abi.MppiGuide) == 64
    assert lay == {name: getattr(_abi.MppiGuide, name).offset for name, _ in _abi.MppiGuide._fields_}
    assert [name for name, _, _ in _abi.MPPI_GUIDE_FIELDS] == [name for name, _ in _abi.MppiGuide._fields_[7:]]
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    body = hdr[hdr.index("typedef struct urgym_mppi_guide {"):hdr.index("} urgym_mppi_guide;")]
    assert re.findall(r"^\s*(?:void|int32_t|float|double)\*?\s+(\w+);", body, flags=re.M) == [name for name, _ in _abi.MppiGuide._fields_]
    lib = _native.lib()
    for sym in SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    assert lib.urgym_abi_version() == _abi.ABI_VERSION == 4  # found by lookup, within the version


def test_refusals_without_a_device():
    """A NULL handle is refused by every new entry point before anything else is looked at."""
    lib = _native.lib()
    m, g = _abi.Mppi(), _abi.MppiGuide()
    calls = ((lib.urgym_mppi_guide_actions, (None, C.byref(m), C.byref(g), 0, None)), (lib.urgym_mppi_terminal, (None, C.byref(m), C.byref(g), None)),
             (lib.urgym_mppi_plan_guided, (None, None, C.byref(m), C.byref(g), 0, None)),
             (lib.urgym_mppi_control_guided, (None, None, C.byref(m), C.byref(g), 0, 1, None, None)))
    for call, args in calls:
        assert call(*args) == _abi.ERR_ARG and b"null handle" in lib.urgym_last_error(None)
