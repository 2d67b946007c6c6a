"""CPU tests (-m "not gpu") of the MPPI temperature from a target effective sample size.

  * tests/mppi_temper_harness.cpp, a stand-alone host program around ur_gym_amd/csrc/urgym_mppi_temper.h -- the header the kernel compiles
    -- equals the numpy restatements of ur_gym_amd.evaluation bitwise: the exponential (mppi_temper_exp) on a grid over [-708, 0], at its
    breakpoints and at the half-way points of x * LOG2E; the search and its weights (mppi_temper_solve) at K = 2, 5, 64, 65 and 1024,
    with and without elites, on returns that take every branch.  Built a second time with -fsanitize=address,undefined and run as that
    program.
  * the exponential against the correctly rounded exp (50-digit decimal arithmetic) within 2 ulp.
  * what the search promises where it is solved, and that the effective sample size does not fall as the temperature rises.
  * the ctypes mirror of urgym_mppi_temper against the C compiler's own layout, the five symbols, the refusals that need no device,
    DeviceMPPI.check_temper, and the table of training entry points.
"""
import ctypes as C
import decimal
import os
import re
import subprocess

import numpy as np
import pytest

from mppi_temper_cases import (KINDS, LAM_FIXED, LAM_MAX, LAM_MIN, SAMPLES, STEPS, exp_breakpoints, exp_grid, exp_halfway, lam_grid, solve_cases, temper_actions,
                               temper_returns)
from test_mppi_host import bits64, run_harness, same_bits, through
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import DeviceMPPI, mppi_elite_rank, mppi_elite_update, mppi_temper_exp, mppi_temper_solve, mppi_update, ordered_sum
from ur_gym_amd.vector_env import _SAC_TRAIN_ENTRIES, _sac_train_entry

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
SYMBOLS = ("urgym_mppi_update_tempered", "urgym_mppi_plan_tempered", "urgym_mppi_control_tempered", "urgym_mppi_collect_tempered", "urgym_sac_train_tempered")
E = len(KINDS)


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "mppi_temper_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h")] + [os.path.join(CSRC, h) for h in ("urgym_mppi_temper.h", "urgym_mppi_elite.h", "urgym_mppi.h",
                                                                                                 "urgym_sac_terms.h", "urgym_adam.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("mppi_temper_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("mppi_temper_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


@pytest.fixture(scope="module")
def solved():
    """mppi_temper_solve of every case, computed once: (K, M, T) -> its dict."""
    return {(k, m, t): mppi_temper_solve(temper_returns(k), k, t, LAM_MIN, LAM_MAX, STEPS, lam=LAM_FIXED, elites=m) for k, m, t in solve_cases()}


def exp_arguments():
    return np.concatenate([exp_grid(), exp_breakpoints(), exp_halfway()])


def compare_exp(exe, tmp_path):
    x = exp_arguments()
    (got,) = through(exe, tmp_path, "exp", [x], [x.size], [(np.float64, x.shape)])
    assert same_bits(got, mppi_temper_exp(x))


def compare_solve(exe, tmp_path, solved):
    for (k, m, t), want in solved.items():
        ret = temper_returns(k)
        lam, saturated, w, ess = through(exe, tmp_path, "solve", [ret], [E, k, m or 0, bits64(t), bits64(LAM_MIN), bits64(LAM_MAX), STEPS, bits64(LAM_FIXED)],
                                         [(np.float64, (E,)), (np.uint8, (E,)), (np.float64, (E, k)), (np.float64, (E,))])
        case = (k, m, t)
        assert same_bits(lam, want["lam"]) and same_bits(saturated, want["saturated"]), (case, lam, want["lam"], saturated, want["saturated"])
        assert same_bits(w, want["w"]) and same_bits(ess, want["ess"]), case


def test_harness_equals_numpy(harness, tmp_path, solved):
    compare_exp(harness, tmp_path)
    compare_solve(harness, tmp_path, solved)


def test_sanitized_harness(sanitized_harness, tmp_path, solved):
    """The same comparisons on the program built with -fsanitize=address,undefined: any finding ends it with a non-zero status."""
    compare_exp(sanitized_harness, tmp_path)
    compare_solve(sanitized_harness, tmp_path, solved)


def test_exponential_at_its_breakpoints():
    one = np.float64(1.0)
    got = mppi_temper_exp(np.array([0.0, -0.0, -708.0, np.nextafter(-708.0, -np.inf), -np.inf]))
    assert same_bits(got[:2], np.array([one, one]))  # the best sample of a parent weighs exactly 1
    assert got[2] >= np.finfo(np.float64).tiny and same_bits(got[3:], np.zeros(2))  # normal at the last accepted argument, +0.0 below it
    x = exp_arguments()
    y = mppi_temper_exp(x)
    accepted = x >= -708.0
    assert (y[accepted] >= np.finfo(np.float64).tiny).all() and (y[accepted] <= 1.0).all() and not y[~accepted].any() and not np.signbit(y).any()
    order = np.argsort(x)
    assert (np.diff(y[order]) >= -2 * np.spacing(y[order][1:])).all()  # monotone up to its own error
    half = exp_halfway()
    frac = np.abs(half * np.float64(1.4426950408889634) - np.floor(half * np.float64(1.4426950408889634)) - 0.5)
    assert half.size > 4000 and (frac < 1e-12).all()  # they are where they claim to be
    for bad in (np.array([0.5]), np.array([np.nan])):
        with pytest.raises(ValueError):
            mppi_temper_exp(bad)


def test_exponential_against_the_correctly_rounded_one():
    """Within 2 ulp of exp on the grid, the breakpoints and the half-way points.  The exact value comes from 50-digit decimal arithmetic
    on the float64 argument itself; its own error, 1e-49 relative, is far below any ulp.  Where the 2 comes from, with u = 2^-53 and
    |r| <= 0.35: the reduction leaves r within 2 u |r| + 2^-60 of x - kf ln 2 (kf * LN2_HI is exact, LN2_HI + LN2_LO is ln 2 to
    2^-100, and the two subtractions and the second product round once each), which moves exp(r) by less than 0.8 u; the polynomial
    drops less than 2^-58; of the Horner steps only the last two, which end near 1, add an error of the size of u each (u / 2 at the
    most), the earlier ones are scaled down by |r| per step; the product with the power of two is exact.  In all below 2.2 u relative,
    and a relative error of u is between half an ulp and one ulp of the result: 2 ulp holds the sum with a margin.  The largest
    error seen is printed (1.07 ulp)."""
    x = exp_arguments()
    x = x[x >= -708.0]
    y = mppi_temper_exp(x)
    worst = 0.0
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        for xi, yi in zip(x.tolist(), y.tolist()):
            exact = decimal.Decimal(xi).exp()
            ulp = decimal.Decimal(float(np.spacing(np.float64(yi))))
            worst = max(worst, float(abs(decimal.Decimal(yi) - exact) / ulp))
    print(f"mppi_temper_exp against the correctly rounded exp on {x.size} arguments: largest error {worst:.3f} ulp")
    assert worst <= 2.0, worst


def counted_of(ret, k, m):
    r = ret.reshape(-1, k)
    return np.isfinite(r) if m is None else mppi_elite_rank(ret, k, m)["elite"] != 0


def ess_at(r, counted, rmax, lam):
    with np.errstate(all="ignore"):
        w = np.where(counted, mppi_temper_exp(np.where(counted, r - rmax, 0.0) / np.float64(lam)), 0.0)
    Z, Q = ordered_sum(w, np.float64), ordered_sum(w * w, np.float64)
    return (Z * Z) / Q


def test_search_takes_every_branch_and_keeps_its_promises(solved):
    seen = set()
    for (k, m, t), got in solved.items():
        ret = temper_returns(k)
        r, counted = ret.reshape(E, k), counted_of(ret, k, m)
        case = (k, m, t)
        for p, kind in enumerate(KINDS):
            how, lam = int(got["saturated"][p]), got["lam"][p]
            seen.add((kind, how))
            w = got["w"][p]
            assert not w[~(counted[p] if kind != "none" else np.arange(k) == 0)].any() and (w >= 0).all(), (case, kind)  # a counted weight may underflow to +0.0
            if kind == "none":
                assert how == _abi.MPPI_TEMPER_NO_RETURN and lam == LAM_FIXED and w[0] == 1 and got["ess"][p] == 1, (case, kind)
                continue
            assert w.max() == 1.0 and same_bits(got["ess"][p], ess_at(r[p], counted[p], got["rmax"][p], lam)), (case, kind)
            count = int(counted[p].sum())
            if kind == "one":  # ess is 1 whatever the temperature
                assert (how, lam) == ((_abi.MPPI_TEMPER_AT_MIN, LAM_MIN) if t == 1 else (_abi.MPPI_TEMPER_AT_MAX, LAM_MAX)) and got["ess"][p] == 1, (case, kind)
            elif kind == "equal":  # ess is the count whatever the temperature
                assert got["ess"][p] == count and (how, lam) == (_abi.MPPI_TEMPER_AT_MIN, LAM_MIN), (case, kind)
            elif kind == "spread" and 1 < t < count:  # one weight at lam_min, nearly equal ones at lam_max (T = count itself is not quite met there)
                assert how == _abi.MPPI_TEMPER_SOLVED and ess_at(r[p], counted[p], got["rmax"][p], LAM_MIN) == 1, (case, kind)
            if how == _abi.MPPI_TEMPER_SOLVED:
                below = got["lam_below"][p]
                assert LAM_MIN <= below < lam <= LAM_MAX and got["ess"][p] >= t > ess_at(r[p], counted[p], got["rmax"][p], below), (case, kind)
                assert lam / below - 1 < 1e-8 and got["ess"][p] - t < 1e-5 * t, (case, kind, lam, below, got["ess"][p])  # 32 halvings of nine decades
            elif how == _abi.MPPI_TEMPER_AT_MAX:
                assert lam == LAM_MAX == got["lam_below"][p] and got["ess"][p] < t, (case, kind)
            else:
                assert how == _abi.MPPI_TEMPER_AT_MIN and lam == LAM_MIN and got["ess"][p] >= t, (case, kind)
    assert {how for _, how in seen} == {0, 1, 2, 3}
    for kind in ("special", "spread", "plain"):
        assert (kind, _abi.MPPI_TEMPER_SOLVED) in seen, kind
    assert {("one", 1), ("one", 2), ("equal", 2), ("none", 3)} <= seen
    # the cases are what they claim: K at the wave and power-of-two edges, NaN and both infinities among finite returns
    assert SAMPLES == (2, 5, 64, 65, 1024)
    special = temper_returns(64).reshape(E, 64)[KINDS.index("special")]
    assert np.isnan(special).any() and np.isposinf(special).any() and np.isneginf(special).any() and np.isfinite(special).sum() == 61


def test_the_weights_feed_the_existing_updates():
    """mppi_temper_solve's w is what mppi_update and mppi_elite_update take: their ess is the search's, bit for bit."""
    for k, m in ((5, None), (64, 8)):
        ret = temper_returns(k)
        got = mppi_temper_solve(ret, k, 2.0, LAM_MIN, LAM_MAX, STEPS, lam=LAM_FIXED, elites=m)
        act = temper_actions(E, k, k)
        out = mppi_update(ret, got["w"], act, 1) if m is None else mppi_elite_update(ret, got["w"], act, 1, 0.05, 0.6)
        assert same_bits(out["ess"], got["ess"]) and np.array_equal(out["best_return"], got["rmax"]) and np.isfinite(out["new_mean"]).all(), (k, m)


def test_ess_does_not_fall_as_the_temperature_rises():
    """Over the committed grid of 91 temperatures, for every parent with a finite return at K = 5, 64 and 65, with and without elites."""
    grid = lam_grid()
    assert grid[0] == 1e-3 and abs(grid[-1] / 1e6 - 1) < 1e-12 and grid.size == 91
    for k in (5, 64, 65):
        ret = temper_returns(k)
        r = ret.reshape(E, k)
        rmax = np.where(np.isfinite(r), r, -np.inf).max(axis=1)
        for m in (None, max(2, k // 8)):
            counted = counted_of(ret, k, m)
            for p, kind in enumerate(KINDS):
                if kind == "none":
                    continue
                ess = np.array([ess_at(r[p], counted[p], rmax[p], lam) for lam in grid])
                assert (np.diff(ess) >= 0).all() and ess[0] >= 1 and ess[-1] <= counted[p].sum() * (1 + 1e-12), (k, m, kind)


def test_struct_mirror_and_symbols(harness):
    lay = run_harness(harness, "layout")
    assert lay.pop("sizeof") == C.sizeof(_abi.MppiTemper) == 48 and lay.pop("alignof") == C.alignment(_abi.MppiTemper) == 8
    assert lay == {name: getattr(_abi.MppiTemper, name).offset for name, _ in _abi.MppiTemper._fields_}
    at = 0  # no hidden padding: every field starts where the one before ends
    for name, ct in _abi.MppiTemper._fields_:
        assert getattr(_abi.MppiTemper, name).offset == at, name
        at += C.sizeof(ct)
    assert at == 48
    assert [name for name, _, _ in _abi.MPPI_TEMPER_FIELDS] == [name for name, _ in _abi.MppiTemper._fields_[5:]]
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    body = hdr[hdr.index("typedef struct urgym_mppi_temper {"):hdr.index("} urgym_mppi_temper;")]
    names = [n for line in re.findall(r"^\s*(?:int32_t|float|double|uint8_t)\*?\s+([\w, ]+);", body, flags=re.M) for n in line.split(", ")]
    assert names == [name for name, _ in _abi.MppiTemper._fields_]
    for name, value in (("SOLVED", 0), ("AT_MAX", 1), ("AT_MIN", 2), ("NO_RETURN", 3), ("STEPS_MAX", 64)):
        assert getattr(_abi, "MPPI_TEMPER_" + name) == value and re.search(rf"^#define URGYM_MPPI_TEMPER_{name} {value}$", hdr, flags=re.M), name
    assert "#define URGYM_ABI_VERSION 4\n" in hdr and C.sizeof(_abi.MppiStatsRecord) == 88 and C.sizeof(_abi.SacPlanning) == 72  # nothing else moved
    lib = _native.lib()
    for sym in SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym


def test_refusals_without_a_device():
    """A NULL handle is refused by every entry point before anything else is looked at."""
    lib = _native.lib()
    m, t, x, ring, learner, schedule, planning = _abi.Mppi(), _abi.MppiTemper(), _abi.MppiExplore(), _abi.ReplayRing(), _abi.SacLearner(), _abi.SacSchedule(), _abi.SacPlanning()
    calls = ((lib.urgym_mppi_update_tempered, (None, C.byref(m), C.byref(t), None, None)),
             (lib.urgym_mppi_plan_tempered, (None, None, C.byref(m), C.byref(t), None, None, 0, None)),
             (lib.urgym_mppi_control_tempered, (None, None, C.byref(m), C.byref(t), None, None, 0, 1, None, None)),
             (lib.urgym_mppi_collect_tempered, (None, None, C.byref(m), C.byref(t), None, None, C.byref(x), 0, 1, C.byref(ring), 0, None)),
             (lib.urgym_sac_train_tempered, (None, C.byref(learner), C.byref(schedule), C.byref(planning), C.byref(t), None, None, None, None, None, None, None)))
    for call, args in calls:
        assert call(*args) == _abi.ERR_ARG and b"null handle" in lib.urgym_last_error(None)


def test_planner_options_are_checked_without_a_device():
    check = DeviceMPPI.check_temper
    assert check(8) is None and check(8, None, -1.0, float("nan"), 0) is None  # no target: nothing is looked at
    assert check(8, 2) == (2.0, 1e-3, 1e6, 32) and check(8, 8.0, 1e-100, 1e100, 64) == (8.0, 1e-100, 1e100, 64) and check(3, 1, 5.0, 5.0, 1) == (1.0, 5.0, 5.0, 1)
    for bad in (dict(ess_target=0.5), dict(ess_target=8.5), dict(ess_target=float("nan")), dict(ess_target=float("inf")), dict(ess_target=True),
                dict(ess_target=2, lam_min=0.0), dict(ess_target=2, lam_min=1e-101), dict(ess_target=2, lam_max=1e101), dict(ess_target=2, lam_max=float("inf")),
                dict(ess_target=2, lam_min=float("nan")), dict(ess_target=2, lam_min=2.0, lam_max=1.0), dict(ess_target=2, temper_steps=0),
                dict(ess_target=2, temper_steps=65), dict(ess_target=2, temper_steps=2.5), dict(ess_target=2, temper_steps=True)):
        with pytest.raises(ValueError):
            check(8, **bad)
    with pytest.raises(ValueError):
        check(3, 4)  # the elites bound the target


def test_the_train_entry_table_keeps_its_rows():
    """The new row stands first and is selected by the planner's temper struct alone: every combination of the options of before names
    the symbol, and takes the arguments, it did."""
    before = (
        ("urgym_sac_train_planned", "planner", ("planner", "clipping", "nstep", "prioritized", "hindsight", "evaluation", "monitor")),
        ("urgym_sac_train_normalized", "normalizer", ("normalizer", "clipping", "nstep", "prioritized", "hindsight", "evaluation", "monitor")),
        ("urgym_sac_train_clipped", "clipping", ("clipping", "nstep", "prioritized", "hindsight", "evaluation", "monitor")),
        ("urgym_sac_train_hindsight", "hindsight", ("hindsight", "evaluation", "monitor")),
        ("urgym_sac_train_prioritized", "prioritized", ("prioritized", "evaluation", "monitor")),
        ("urgym_sac_train_nstep", "nstep", ("nstep", "evaluation", "monitor")),
        ("urgym_sac_train_monitored", "monitor", ("evaluation", "monitor")),
        ("urgym_sac_train_evaluated", "evaluation", ("evaluation",)),
        ("urgym_sac_train", None, ()),
    )
    assert _SAC_TRAIN_ENTRIES[1:] == before
    assert _SAC_TRAIN_ENTRIES[0] == ("urgym_sac_train_tempered", "temper", ("planner", "temper") + before[0][2][1:])
    options = [selects for _, selects, _ in before if selects]
    for mask in range(1 << len(options)):
        present = {o for i, o in enumerate(options) if mask >> i & 1}
        want = next((symbol, opts) for symbol, selects, opts in before if selects is None or selects in present)
        assert _sac_train_entry(present) == want, present
        if "planner" in present:
            assert _sac_train_entry(present | {"temper"})[0] == "urgym_sac_train_tempered", present
