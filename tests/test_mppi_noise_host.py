"""CPU tests (-m "not gpu") of the temporally correlated sampling noise of the MPPI planner.

  * tests/mppi_noise_harness.cpp, a stand-alone host program around ur_gym_amd/csrc/urgym_mppi_noise.h -- the header the kernel compiles
    -- equals the numpy restatement ur_gym_amd.evaluation.mppi_colored_noise bitwise on random xi at H = 1, 2, 3 and 64 with beta = 0,
    0.5, 0.9, the largest float32 below 1, and 1.  Built a second time with -fsanitize=address,undefined and run as that program.
  * what the recurrence promises: beta = 0 returns xi by value, beta = 1 repeats row 0, the nominal sample stays zero.
  * the distribution of the restatement over mppi_noise: unit variance at every step, lag-1 correlation beta.
  * the ctypes mirror of urgym_mppi_noise against the C compiler's own layout, the five symbols, the refusals that need no device,
    DeviceMPPI.check_noise, and the selection of the training entry point.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mppi_noise_cases import (BELOW_ONE, BETAS, HORIZONS, STAT_BETAS, STAT_BOUND, STAT_COUNT, STAT_DRAW, STAT_E, STAT_H, STAT_ITERATION, STAT_K, STAT_SEED, WIDTH,
                              env_grid, random_xi)
from test_mppi_host import bits32, run_harness, same_bits, through
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import DeviceMPPI, mppi_colored_noise, mppi_noise
from ur_gym_amd.vector_env import _SAC_TRAIN_ENTRIES, _sac_train_entry

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
SYMBOLS = ("urgym_mppi_sample_colored", "urgym_mppi_plan_colored", "urgym_mppi_control_colored", "urgym_mppi_collect_colored", "urgym_sac_train_colored")


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "mppi_noise_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h")] + [os.path.join(CSRC, h) for h in ("urgym_mppi_noise.h", "urgym_mppi.h", "urgym_sac_terms.h", "urgym_adam.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("mppi_noise_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("mppi_noise_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def host_scale(beta):
    """scale as include/urgym.h states it, restated apart from mppi_colored_noise: float64 up to the correctly rounded square root."""
    b = np.float64(np.float32(beta))
    return np.float32(np.sqrt(np.float64(1.0) - b * b))


def compare(exe, tmp_path):
    for beta in BETAS:
        assert run_harness(exe, "scale", bits32(beta))["scale"] == bits32(host_scale(beta)), beta
        for h in HORIZONS:
            xi = random_xi(h)
            (got,) = through(exe, tmp_path, "color", [xi], [h, WIDTH, bits32(beta)], [(np.float32, xi.shape)])
            assert same_bits(got, mppi_colored_noise(xi, beta)), (beta, h)


def test_harness_equals_numpy(harness, tmp_path):
    compare(harness, tmp_path)


def test_sanitized_harness(sanitized_harness, tmp_path):
    """The same comparisons on the program built with -fsanitize=address,undefined: any finding ends it with a non-zero status."""
    compare(sanitized_harness, tmp_path)


def test_the_scale_at_its_ends():
    assert host_scale(0.0) == 1 and host_scale(1.0) == 0 and np.float32(BELOW_ONE) < 1
    small = host_scale(BELOW_ONE)
    assert 0 < small < 1e-3 and abs(float(small) ** 2 + BELOW_ONE ** 2 - 1) < 1e-10  # formed in float64: 1 - beta^2 does not cancel to 0
    assert abs(float(host_scale(0.5)) - np.sqrt(0.75)) < 1e-7 and abs(float(host_scale(0.9)) - np.sqrt(1 - np.float64(np.float32(0.9)) ** 2)) < 1e-7


def test_the_recurrence_keeps_its_promises():
    for h in HORIZONS:
        xi = random_xi(h)
        white = mppi_colored_noise(xi, 0.0)
        assert np.array_equal(white, xi) and white.dtype == np.float32  # by value: a -0.0 of xi becomes +0.0 from step 1 on
        assert same_bits(white[0], xi[0])
        frozen = mppi_colored_noise(xi, 1.0)
        assert all(np.array_equal(frozen[k], xi[0]) for k in range(h))  # by value too: -0.0 + 0 * xi is +0.0
        for beta in BETAS:
            eps = mppi_colored_noise(xi, beta)
            assert same_bits(eps[:, :6], np.zeros((h, 6), np.float32)), (beta, h)  # the nominal sample: +0.0, never -0.0
            assert same_bits(eps[0], xi[0]) and np.isfinite(eps).all()
        if h >= 2:  # one step by hand
            beta = np.float32(0.9)
            eps = mppi_colored_noise(xi, beta)
            assert same_bits(eps[1], beta * xi[0] + host_scale(0.9) * xi[1])
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            mppi_colored_noise(random_xi(2), bad)
    with pytest.raises(ValueError):
        mppi_colored_noise(random_xi(2).astype(np.float64), 0.5)


def test_every_step_has_unit_variance_and_lag_one_correlation_beta():
    """The restatement over mppi_noise at seed 0xC0FFEE1234, draw 7, iteration 0, E = 8, K = 256, H = 32: 12,240 non-nominal values per
    step.  The variance of every step within 0.06 of 1 and the mean lag-1 product of every adjacent pair of steps within 0.06 of beta:
    about 4.7 standard errors of a variance at that count (sqrt(2 / 12240) = 0.0128).  A wrong scale or a reversed recurrence does not
    pass; this is not a measurement of the kernel."""
    xi = mppi_noise(STAT_SEED, STAT_DRAW, STAT_ITERATION, *env_grid(STAT_E, STAT_K, STAT_H))
    assert xi.shape == (STAT_H, STAT_E * STAT_K, 6) and xi.dtype == np.float32
    live = (np.arange(STAT_E * STAT_K) % STAT_K) != 0
    for beta in STAT_BETAS:
        eps = mppi_colored_noise(xi, beta)
        assert not eps[:, ~live].any()
        x = eps[:, live].reshape(STAT_H, -1).astype(np.float64)
        assert x.shape[1] == STAT_COUNT == 12240
        variance = (x * x).mean(axis=1) - x.mean(axis=1) ** 2
        lag = (x[1:] * x[:-1]).mean(axis=1)
        worst = (np.abs(variance - 1).max(), np.abs(lag - beta).max())
        print(f"beta = {beta}: worst deviation of a step's variance {worst[0]:.4f}, of a lag-1 product {worst[1]:.4f}")
        assert worst[0] <= STAT_BOUND and worst[1] <= STAT_BOUND, (beta, worst)


def test_struct_mirror_and_symbols(harness):
    lay = run_harness(harness, "layout")
    assert lay.pop("sizeof") == C.sizeof(_abi.MppiNoise) == 8 and lay.pop("alignof") == C.alignment(_abi.MppiNoise) == 4
    assert lay == {name: getattr(_abi.MppiNoise, name).offset for name, _ in _abi.MppiNoise._fields_} == {"beta": 0, "reserved0": 4}
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    body = hdr[hdr.index("typedef struct urgym_mppi_noise {"):hdr.index("} urgym_mppi_noise;")]
    names = re.findall(r"^\s*(?:int32_t|float)\s+(\w+);", body, flags=re.M)
    assert names == [name for name, _ in _abi.MppiNoise._fields_]
    assert "#define URGYM_ABI_VERSION 4\n" in hdr and C.sizeof(_abi.MppiTemper) == 48 and C.sizeof(_abi.SacPlanning) == 72  # nothing else moved
    lib = _native.lib()
    for sym in SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym


def test_refusals_without_a_device():
    """A NULL handle is refused by every entry point before anything else is looked at."""
    lib = _native.lib()
    m, z, x, ring, learner, schedule, planning = _abi.Mppi(), _abi.MppiNoise(), _abi.MppiExplore(), _abi.ReplayRing(), _abi.SacLearner(), _abi.SacSchedule(), _abi.SacPlanning()
    calls = ((lib.urgym_mppi_sample_colored, (None, C.byref(m), C.byref(z), None, 0, 0, None)),
             (lib.urgym_mppi_plan_colored, (None, None, C.byref(m), C.byref(z), None, None, None, 0, None)),
             (lib.urgym_mppi_control_colored, (None, None, C.byref(m), C.byref(z), None, None, None, 0, 1, None, None)),
             (lib.urgym_mppi_collect_colored, (None, None, C.byref(m), C.byref(z), None, None, None, C.byref(x), 0, 1, C.byref(ring), 0, None)),
             (lib.urgym_sac_train_colored, (None, C.byref(learner), C.byref(schedule), C.byref(planning), C.byref(z), None, None, None, None, None, None, None, None)))
    for call, args in calls:
        assert call(*args) == _abi.ERR_ARG and b"null handle" in lib.urgym_last_error(None)


def test_planner_option_is_checked_without_a_device():
    check = DeviceMPPI.check_noise
    assert check() is None and check(None) is None
    assert check(0.0) == 0.0 and check(0) == 0.0 and check(1) == 1.0 and check(0.5) == 0.5 and check(np.float32(0.9)) == float(np.float32(0.9))
    assert check(BELOW_ONE) == BELOW_ONE
    for bad in (-0.1, -1e-30, 1.0000001, 2, float("nan"), float("inf"), -float("inf"), True, False, 1e300):
        with pytest.raises(ValueError):
            check(bad)


def test_the_training_entry_is_selected_ahead_of_the_table():
    """Every set of the options of before names the symbol, and takes the arguments, it did; any set with "noise" names
    urgym_sac_train_colored, whose arguments are the tempered call's with the noise struct after the planner."""
    table = _SAC_TRAIN_ENTRIES
    assert all(symbol != "urgym_sac_train_colored" and "noise" not in opts for symbol, _, opts in table) and len(table) == 10
    options = [selects for _, selects, _ in table if selects]
    assert "temper" in options and "planner" in options and "noise" not in options
    for mask in range(1 << len(options)):
        present = {o for i, o in enumerate(options) if mask >> i & 1}
        want = next((symbol, opts) for symbol, selects, opts in table if selects is None or selects in present)
        assert _sac_train_entry(present) == want, present
        symbol, opts = _sac_train_entry(present | {"noise"})
        assert symbol == "urgym_sac_train_colored", present
        assert opts == ("planner", "noise") + table[0][2][1:] and table[0][0] == "urgym_sac_train_tempered"
