"""CPU tests (-m "not gpu") of elite samples and the adaptive std of the MPPI planner.

  * tests/mppi_elite_harness.cpp, a stand-alone host program around ur_gym_amd/csrc/urgym_mppi_elite.h -- the header the kernels compile
    -- equals the numpy restatements of ur_gym_amd.evaluation bitwise: the rank, the elites, their count and the threshold
    (mppi_elite_rank), the fixed weights and the argument of exp (mppi_elite_weights), the elite update with its std (mppi_elite_update),
    the adaptive action line (mppi_actions with an array sigma).  With M == K the header's update is mppi_update_host's, bit for bit.
    Built a second time with -fsanitize=address,undefined and run as that program.
  * the std against exact rational arithmetic given w, within a bound derived below from the rounded operations.
  * the ctypes mirror of urgym_mppi_adapt against the C compiler's own layout, the five symbols, and the refusals that need no device.
"""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from mppi_elite_cases import H, LAM, RANK_SAMPLES, elite_counts, random_std, rank_cases, rank_returns, update_cases
from test_mppi_host import bits32, bits64, run_harness, same_bits, through
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import (DeviceMPPI, mppi_actions, mppi_elite_rank, mppi_elite_update, mppi_elite_weights, mppi_noise, mppi_update,
                                   mppi_weights)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
SYMBOLS = ("urgym_mppi_sample_adaptive", "urgym_mppi_update_elite", "urgym_mppi_plan_adaptive", "urgym_mppi_control_adaptive", "urgym_mppi_collect_adaptive")


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "mppi_elite_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h")] + [os.path.join(CSRC, h) for h in ("urgym_mppi_elite.h", "urgym_mppi.h", "urgym_sac_terms.h", "urgym_adam.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("mppi_elite_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("mppi_elite_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def same_values(a, b):
    """Equal as float64 compares, NaN with NaN: what is asked of rmax and of the argument of exp where a maximum of -0.0 and 0.0 may be
    either zero (fmax and numpy's max need not pick the same one; exp gives 1 for both)."""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def compare_rank(exe, tmp_path, cases):
    for k, layout, m in cases:
        ret = rank_returns(k, layout)
        want = mppi_elite_rank(ret, k, m)
        rank, elite, count, threshold = through(exe, tmp_path, "rank", [ret], [3, k, m], [(np.int32, (3, k)), (np.uint8, (3, k)), (np.int32, (3,)), (np.float64, (3,))])
        case = (k, layout, m)
        assert same_bits(rank, want["rank"]) and same_bits(elite, want["elite"]), case
        assert same_bits(count, want["elite_count"]) and same_bits(threshold, want["threshold"]), case
        # what the rank is, stated without the restatement: a permutation; sorted by it the keys descend and equal keys keep their order
        r = ret.reshape(3, k)
        key = np.where(np.isfinite(r), r, -np.inf)
        for p in range(3):
            assert sorted(rank[p].tolist()) == list(range(k)), case
            order = np.argsort(rank[p])
            ks = key[p, order]
            assert (ks[:-1] >= ks[1:]).all() and (order[:-1][ks[:-1] == ks[1:]] < order[1:][ks[:-1] == ks[1:]]).all(), case
            finite = int(np.isfinite(r[p]).sum())
            assert count[p] == min(m, finite) == elite[p].sum() and not elite[p][~np.isfinite(r[p])].any(), case
            if count[p]:
                assert threshold[p] == r[p][elite[p] != 0].min() and (r[p][(elite[p] == 0) & np.isfinite(r[p])] <= threshold[p]).all(), case
            else:
                assert threshold[p] == -np.inf, case


def compare_weights(exe, tmp_path, cases):
    for k, layout, m in cases:
        ret = rank_returns(k, layout)
        w, rmax = mppi_elite_weights(ret, LAM, k, m)
        got_rmax, x, fixed = through(exe, tmp_path, "weights", [ret], [3, k, m, bits64(LAM)], [(np.float64, (3,)), (np.float64, (3, k)), (np.float64, (3, k))])
        case = (k, layout, m)
        assert same_values(got_rmax, rmax), case
        decided = fixed >= 0
        assert same_bits(fixed[decided], w[decided]), case  # a weight that needs no exp
        elite = mppi_elite_rank(ret, k, m)["elite"] != 0
        none = ~np.isfinite(ret.reshape(3, k)).any(axis=1)
        assert np.array_equal(~decided, elite & ~none[:, None]), case  # exp decides the weight of an elite, and of nothing else
        with np.errstate(all="ignore"):
            want_x = (ret.reshape(3, k) - rmax[:, None]) / np.float64(LAM)
        assert same_values(x[~decided], want_x[~decided]) and np.isnan(x[decided]).all(), case
        if m == k:  # the plain update's weight
            assert same_bits(w, mppi_weights(ret, LAM, k)[0]), case
        assert (w[none, 0] == 1).all() and (w[none, 1:] == 0).all() and ((w > 0).sum(axis=1)[~none] == np.minimum(m, np.isfinite(ret.reshape(3, k)).sum(axis=1))[~none]).all(), case


def compare_update(exe, tmp_path):
    for name, c in update_cases().items():
        e, k, h, m = c["E"], c["K"], c["H"], c["M"]
        w, _ = mppi_elite_weights(c["ret"], c["lam"], k, m)
        want = mppi_elite_update(c["ret"], w, c["actions"], c["shift"], c["std_min"], c["std_max"])
        rows = (np.float32, (h, e, 6))
        new_mean, mean, ess, new_std, plain_new_mean, plain_mean, plain_ess = through(
            exe, tmp_path, "update", [w, c["actions"]], [h, e, k, c["shift"], bits32(c["std_min"]), bits32(c["std_max"])],
            [rows, rows, (np.float64, (e,)), rows, rows, rows, (np.float64, (e,))])
        assert same_bits(new_mean, want["new_mean"]) and same_bits(mean, want["mean"]) and same_bits(ess, want["ess"]), name
        assert same_bits(new_std, want["new_std"]), (name, new_std, want["new_std"])
        # the shared outputs are the plain update's on the same weights: with M == K those are the plain weights
        assert same_bits(new_mean, plain_new_mean) and same_bits(mean, plain_mean) and same_bits(ess, plain_ess), name
        plain = mppi_update(c["ret"], w, c["actions"], c["shift"])
        assert all(same_bits(want[key], plain[key]) for key in plain), name
        lo, hi = np.float32(c["std_min"]), np.float32(c["std_max"])
        assert (new_std >= lo).all() and (new_std <= hi).all(), name  # never a NaN, whatever the actions are
        if c["expect"] == "both clamps":
            assert (new_std == lo).any() and (new_std == hi).any() and ((new_std > lo) & (new_std < hi)).any(), (name, new_std)
        if c["expect"] == "floor everywhere":  # one elite: a variance of exactly 0 wherever a return is finite
            assert (new_std == lo).all(), (name, new_std)
        if c["expect"] == "floor":
            assert np.isnan(new_mean[1, 2, 3]) and new_std[1, 2, 3] == lo and np.isnan(new_mean).sum() == 1 and (new_std == lo).sum() == 1, (name, new_std)


def compare_actions(exe, tmp_path):
    e = 3
    for k in (2, 5):
        rng = np.random.default_rng(k)
        mean = rng.uniform(-0.9, 0.9, (H, e, 6)).astype(np.float32)
        eps = mppi_noise(77, 3, 1, np.arange(e * k)[None, :] // k, np.arange(e * k)[None, :] % k, np.arange(H)[:, None])
        std = random_std(H, e, k)
        want = mppi_actions(mean, eps, std)
        (got,) = through(exe, tmp_path, "actions", [np.repeat(mean, k, axis=1), eps, np.repeat(std, k, axis=1)], [want.size], [(np.float32, want.shape)])
        assert same_bits(got, want), k
        assert same_bits(want[:, ::k], mean), k  # sample 0 is the nominal whatever its width
        for sigma in (0.0, 0.3, 25.0):  # one width everywhere is the scalar line
            assert same_bits(mppi_actions(mean, eps, np.full(mean.shape, sigma, np.float32)), mppi_actions(mean, eps, sigma)), (k, sigma)
    with pytest.raises(ValueError):
        mppi_actions(mean, eps, std.astype(np.float64))
    with pytest.raises(ValueError):
        mppi_actions(mean, eps, std[:, :2])


def test_harness_equals_numpy(harness, tmp_path):
    compare_rank(harness, tmp_path, rank_cases())
    compare_weights(harness, tmp_path, rank_cases())
    compare_update(harness, tmp_path)
    compare_actions(harness, tmp_path)


def test_sanitized_harness(sanitized_harness, tmp_path):
    """The same comparisons on the program built with -fsanitize=address,undefined: any finding ends it with a non-zero status."""
    compare_rank(sanitized_harness, tmp_path, rank_cases())
    compare_weights(sanitized_harness, tmp_path, rank_cases())
    compare_update(sanitized_harness, tmp_path)
    compare_actions(sanitized_harness, tmp_path)


def test_rank_cases_cover_what_they_claim():
    assert RANK_SAMPLES == (2, 3, 64, 65, 1000, 1024)
    assert elite_counts(2) == (1, 2) and elite_counts(3) == (1, 2, 3) and elite_counts(64) == (1, 2, 8, 63, 64) and elite_counts(1000) == (1, 2, 125, 999, 1000)
    for k in RANK_SAMPLES:
        a, b = rank_returns(k, 0).reshape(3, k), rank_returns(k, 1).reshape(3, k)
        assert len(set(a[0].tolist())) < k  # exact ties
        if k >= 64:
            assert (np.signbit(a[0]) & (a[0] == 0)).any() and (~np.signbit(a[0]) & (a[0] == 0)).any()  # -0.0 against 0.0
        assert np.isposinf(a[1]).any() and np.isfinite(a[1]).any()
        if k >= 3:
            assert np.isneginf(a[1]).any()
        if k >= 64:
            assert np.isnan(a[1]).any()
        assert (b[0] == b[0, 0]).all() and not np.isfinite(b[1]).any() and (b[2] == 0).all() and np.signbit(b[2]).any() and not np.signbit(b[2]).all()
        assert np.isnan(b[1]).any() and np.isneginf(b[1]).any() and (k < 3 or np.isposinf(b[1]).any())
    # all K equal: the rank is the index; signed zeros tie
    for layout, p in ((1, 0), (1, 2), (1, 1)):
        assert mppi_elite_rank(rank_returns(65, layout), 65, 8)["rank"][p].tolist() == list(range(65))


def test_std_against_exact_arithmetic():
    """new_std given w against exact rational arithmetic where no clamp acts.  With u = 2^-53 and |a| <= 1, |m| <= 1 (1 + 13 u): m carries
    at most 13 roundings (mppi_update's count: a product, eleven additions, a quotient), so d = a - m is off by at most 14 u |d| + 13 u
    <= 42 u, dd by 2 (42 u) |d| + u dd + O(u^2) <= 170 u, a term w dd one rounding more, the ordered sum of K <= 1024 terms at most 11
    more on any path, the quotient one.  In all |v - exact| <= (170 + 14) u sum(w) / Z + 14 u v <= 200 u.  The root of v has the
    derivative 1 / (2 sqrt(v)), so for sqrt(v) >= 2^-10: |sd - exact| <= 200 u 2^9 + u, and the conversion to float32 adds half a float32
    ulp: 2^-24 sd."""
    u = 2.0 ** -53
    checked = 0
    for name, c in update_cases().items():
        e, k, h, m = c["E"], c["K"], c["H"], c["M"]
        if k > 65 or c["expect"] is not None:
            continue  # the bound is the same; the rationals of 1024 terms are slow
        w, _ = mppi_elite_weights(c["ret"], c["lam"], k, m)
        got = mppi_elite_update(c["ret"], w, c["actions"], c["shift"], c["std_min"], c["std_max"])["new_std"]
        a = c["actions"].reshape(h, e, k, 6)
        for p in range(e):
            ws = [Fraction(float(x)) for x in w[p]]
            Z = sum(ws)
            for t in range(h):
                for j in range(6):
                    if not np.float32(c["std_min"]) < got[t, p, j] < np.float32(c["std_max"]):
                        continue  # a clamp acted
                    xs = [Fraction(float(y)) for y in a[t, p, :, j]]
                    mean = sum(x * y for x, y in zip(ws, xs)) / Z
                    var = sum(x * (y - mean) ** 2 for x, y in zip(ws, xs)) / Z
                    sd = float(got[t, p, j])
                    assert sd >= 2.0 ** -10, (name, sd)
                    # |sd^2 - var| <= |sd - exact| (sd + exact) <= 2.1 sd |sd - exact|
                    bound = 2.1 * sd * (200 * u * 2 ** 9 + u + 2.0 ** -24 * sd)
                    assert abs(Fraction(sd) ** 2 - var) <= bound, (name, p, t, j, sd, float(var))
                    checked += 1
    assert checked > 100


def test_struct_mirror_and_symbols(harness):
    lay = run_harness(harness, "layout")
    assert lay.pop("sizeof") == C.sizeof(_abi.MppiAdapt) == 64 and lay.pop("alignof") == C.alignment(_abi.MppiAdapt) == 8
    assert lay == {name: getattr(_abi.MppiAdapt, name).offset for name, _ in _abi.MppiAdapt._fields_}
    # no hidden padding: every field starts where the one before ends
    at = 0
    for name, ct in _abi.MppiAdapt._fields_:
        assert getattr(_abi.MppiAdapt, name).offset == at, name
        at += C.sizeof(ct)
    assert at == 64
    assert [name for name, _, _ in _abi.MPPI_ADAPT_FIELDS] == [name for name, _ in _abi.MppiAdapt._fields_[4:]]
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    body = hdr[hdr.index("typedef struct urgym_mppi_adapt {"):hdr.index("} urgym_mppi_adapt;")]
    names = [n for line in re.findall(r"^\s*(?:int32_t|float|double|uint8_t)\*?\s+([\w, ]+);", body, flags=re.M) for n in line.split(", ")]
    assert names == [name for name, _ in _abi.MppiAdapt._fields_]
    lib = _native.lib()
    for sym in SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym


def test_refusals_without_a_device():
    """A NULL handle is refused by every entry point before anything else is looked at."""
    lib = _native.lib()
    m, a, x, ring = _abi.Mppi(), _abi.MppiAdapt(), _abi.MppiExplore(), _abi.ReplayRing()
    calls = ((lib.urgym_mppi_sample_adaptive, (None, C.byref(m), C.byref(a), 0, 0, None)), (lib.urgym_mppi_update_elite, (None, C.byref(m), C.byref(a), None)),
             (lib.urgym_mppi_plan_adaptive, (None, None, C.byref(m), C.byref(a), None, 0, None)),
             (lib.urgym_mppi_control_adaptive, (None, None, C.byref(m), C.byref(a), None, 0, 1, None, None)),
             (lib.urgym_mppi_collect_adaptive, (None, None, C.byref(m), C.byref(a), None, C.byref(x), 0, 1, C.byref(ring), 0, None)))
    for call, args in calls:
        assert call(*args) == _abi.ERR_ARG and b"null handle" in lib.urgym_last_error(None)


def test_planner_options_are_checked_without_a_device():
    check = DeviceMPPI.check_adapt
    assert check(8, 0.6) is None and check(8, 0.6, None, False, 0.3, 0.2) is None  # neither option: nothing is looked at
    assert check(8, 0.6, elites=3) == (3, 0, 0.05, 0.6) and check(8, 0.6, adapt_std=True) == (8, 1, 0.05, 0.6)
    assert check(8, 0.01, adapt_std=True, std_min=0.0) == (8, 1, 0.0, 0.01)  # std_max defaults to sigma
    assert check(8, 0.6, 8, True, 0.1, 0.9) == (8, 1, 0.1, 0.9)
    with pytest.raises(ValueError):
        check(8, 0.01, adapt_std=True)  # ... which the default std_min then exceeds
    for bad in (dict(elites=0), dict(elites=9), dict(elites=True), dict(adapt_std=True, std_min=-0.1), dict(adapt_std=True, std_min=0.7, std_max=0.6),
                dict(adapt_std=True, std_max=float("inf")), dict(adapt_std=True, std_min=float("nan")), dict(elites=2, std_max=1e39)):
        with pytest.raises(ValueError):
            check(8, 0.6, **bad)
