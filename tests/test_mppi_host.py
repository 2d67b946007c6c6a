"""CPU tests (-m "not gpu") of the MPPI planner.

  * tests/mppi_harness.cpp, a stand-alone host program around ur_gym_amd/csrc/urgym_mppi.h -- the header the kernels compile -- equals the
    numpy restatements of ur_gym_amd.evaluation bitwise: the env map, the counter words and the Philox integers behind mppi_noise, the
    action line (mppi_actions), the score step (mppi_score), the fixed weights and the argument of exp (mppi_weights), the mean, the
    effective sample size and the shift (mppi_update).  Built a second time with -fsanitize=address,undefined and run as that program.
  * mppi_update against exact rational arithmetic for the mean given w, within a bound derived below from the rounded operations.
  * the ctypes mirror of urgym_mppi against the C compiler's own layout, the new symbols, and the refusals that need no device.
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

from mppi_cases import E, H, STEP_SAMPLES, outcomes, sample_means, update_cases
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import (_noise_integers, mppi_actions, mppi_noise, mppi_score, mppi_update, mppi_weights, ordered_sum, philox4x32_10,
                                   policy_noise)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
SYMBOLS = ("urgym_mppi_fanout", "urgym_mppi_sample", "urgym_mppi_score", "urgym_mppi_update", "urgym_mppi_record", "urgym_mppi_plan", "urgym_mppi_control")


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "mppi_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h")] + [os.path.join(CSRC, h) for h in ("urgym_mppi.h", "urgym_sac_terms.h", "urgym_adam.h", "urgym_philox.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("mppi_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("mppi_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


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


def compare_map_and_words(exe):
    for k in STEP_SAMPLES + (1024,):
        got = run_harness(exe, "map", k, 3 * k + 1)
        n = np.arange(3 * k + 1)
        assert got["parent"] == (n // k).tolist() and got["sample"] == (n % k).tolist(), k
    tags = {_abi.NOISE_TAG | 0, _abi.NOISE_TAG | 1, _abi.REPLAY_TAG, _abi.PER_TAG, 0, 1, 2, 3, 4}
    assert _abi.MPPI_TAG == 0x4D505000 and not tags & {_abi.MPPI_TAG | 0, _abi.MPPI_TAG | 1}
    for seed, draw, i, p, j, h in ((0, 0, 0, 0, 1, 0), (0xC0FFEE1234567, (1 << 32) - 1, 7, 65535, 1023, 63), (9, 12345, 2, 2, 4, 1)):
        got = run_harness(exe, "words", seed, draw, i, p, j, h)
        mid = (i << 24) | (h << 16) | j
        assert got["counter"] == [[p, mid, draw, _abi.MPPI_TAG | b] for b in (0, 1)], (got, mid)
        key = (seed & 0xFFFFFFFF, seed >> 32)
        a, b = (philox4x32_10(key, (np.uint64(p), np.uint64(mid), np.uint64(draw), np.uint64(_abi.MPPI_TAG | blk))) for blk in (0, 1))
        m = _noise_integers(a, b, np.float64)
        assert got["m"] == [int(x) for x in m], (got, m)
        # mppi_noise is Box-Muller on exactly these integers: the policy noise's expressions on other words
        eps = mppi_noise(seed, draw, i, p, j, h, dtype=np.float64)
        u1, u2 = (m[0::2] + 1) * 2.0 ** -24, m[1::2] * 2.0 ** -24
        r = np.sqrt(-2 * np.log(u1))
        assert np.allclose(eps[0::2], r * np.cos(2 * np.pi * u2), atol=1e-12) and np.allclose(eps[1::2], r * np.sin(2 * np.pi * u2), atol=1e-12)


def compare_actions(exe, tmp_path):
    for k in STEP_SAMPLES:
        mean = sample_means()
        eps = mppi_noise(77, 3, 1, np.arange(E * k)[None, :] // k, np.arange(E * k)[None, :] % k, np.arange(H)[:, None])
        assert eps.shape == (H, E * k, 6) and not eps[:, ::k].any() and eps[:, 1::k].all()  # sample 0 is the nominal
        for sigma in (0.0, 0.3, 25.0):
            want = mppi_actions(mean, eps, sigma)
            assert want.dtype == np.float32 and np.abs(want).max() <= 1.0
            (got,) = through(exe, tmp_path, "actions", [np.repeat(mean, k, axis=1), eps], [want.size, bits32(sigma)], [(np.float32, want.shape)])
            assert same_bits(got, want), (k, sigma)
            assert same_bits(want[:, ::k], np.clip(mean, -1, 1)), (k, sigma)  # sample 0 is clip(mean)
            if sigma == 25.0:  # the clamp acts on most components, on both sides
                assert (want == 1).mean() > 0.3 and (want == -1).mean() > 0.3
    special = np.array([-0.0, 0.0, 1.0, -1.0, 3e38, -3e38, np.inf, -np.inf, 1e-45], np.float32)
    mean, eps = np.meshgrid(special, special)
    mean, eps = mean.reshape(1, -1, 1).repeat(6, 2).copy(), eps.reshape(1, -1, 1).repeat(6, 2).copy()
    with np.errstate(all="ignore"):  # signed zeros, overflow to an infinity, inf - inf (fmax passes the NaN over: -1)
        want = mppi_actions(mean, eps, 2.5)
    (got,) = through(exe, tmp_path, "actions", [mean, eps], [want.size, bits32(2.5)], [(np.float32, want.shape)])
    assert same_bits(got, want)


def compare_score(exe, tmp_path):
    for n in (1, 7, 40):
        for gamma in (1.0, 0.95):
            arrays = outcomes(H, n, n)
            want = mppi_score(*arrays, gamma)
            got = through(exe, tmp_path, "score", arrays, [H, n, bits64(gamma)],
                          [(np.float64, (n,)), (np.float64, (n,)), (np.int32, (n,)), (np.uint8, (n,)), (np.uint8, (n,)), (np.uint8, (n,))])
            for name, g in zip(("ret", "g", "end_step", "alive", "success", "collided"), got):
                assert same_bits(g, want[name]), (n, gamma, name, g, want[name])
            if n == 40:
                reward, term, trunc = arrays[:3]
                assert np.isnan(want["ret"][H + 2]) and np.isnan(want["ret"]).sum() == 1  # the NaN reward reaches that env only
                assert want["end_step"][:H].tolist() == list(range(H)) and not want["alive"][:H].any()  # terminated at every step index
                assert want["end_step"][H] == min(1, H - 1) and want["end_step"][H + 1] == H - 1 and not want["alive"][H + 1]
                assert want["alive"][H + 3:].all() and (want["end_step"][H + 3:] == H - 1).all() and not want["success"][H + 3:].any()
                assert want["ret"][0] == np.float64(reward[0, 0])  # the sum stops with the episode
                if gamma == 1.0:
                    assert want["ret"][-1] == np.float64(reward[0, -1]) + np.float64(reward[1, -1]) + np.float64(reward[2, -1])


def compare_update(exe, tmp_path):
    for name, c in update_cases().items():
        e, k, h = c["E"], c["K"], c["H"]
        w, rmax = mppi_weights(c["ret"], c["lam"], k)
        got_rmax, x, fixed = through(exe, tmp_path, "weights", [c["ret"]], [e, k, bits64(c["lam"])], [(np.float64, (e,)), (np.float64, (e, k)), (np.float64, (e, k))])
        assert same_bits(got_rmax, rmax), name
        decided = fixed >= 0
        assert same_bits(fixed[decided], w[decided]), name  # a weight that needs no exp
        with np.errstate(all="ignore"):
            want_x = (c["ret"].reshape(e, k) - rmax[:, None]) / np.float64(c["lam"])
        assert same_bits(x[~decided], want_x[~decided]) and np.isnan(x[decided]).all(), name
        want = mppi_update(c["ret"], w, c["actions"], c["shift"])
        new_mean, mean, ess = through(exe, tmp_path, "update", [w, c["actions"]], [h, e, k, c["shift"]],
                                      [(np.float32, (h, e, 6)), (np.float32, (h, e, 6)), (np.float64, (e,))])
        assert same_bits(new_mean, want["new_mean"]) and same_bits(mean, want["mean"]) and same_bits(ess, want["ess"]), name
        assert same_bits(want["action_out"], want["new_mean"][0]) and same_bits(want["nominal_return"], c["ret"].reshape(e, k)[:, 0]), name
        if c["shift"]:
            assert same_bits(want["mean"][:-1], want["new_mean"][1:]) and same_bits(want["mean"][-1], want["new_mean"][-1]), name
        else:
            assert same_bits(want["mean"], want["new_mean"]), name
        a = c["actions"].reshape(h, e, k, 6)
        if c["expect"] == "uniform":  # w = 1 for every sample: the plain ordered mean, and every sample counts
            assert (w == 1).all() and (want["ess"] == k).all(), name
            plain = np.array([[[np.float32(ordered_sum(a[t, p, :, j].astype(np.float64), np.float64) / np.float64(k)) for j in range(6)] for p in range(e)] for t in range(h)])
            assert same_bits(want["new_mean"], plain), name
        if c["expect"] == "best":  # one weight is 1, the others 0: the best sample's actions, bit for bit
            best = c["ret"].reshape(e, k).argmax(axis=1)
            assert ((w == 1).sum(axis=1) == 1).all() and ((w == 0).sum(axis=1) == k - 1).all() and (want["ess"] == 1).all(), name
            assert same_bits(want["new_mean"], np.ascontiguousarray(a[:, np.arange(e), best])), name
        if c["expect"] == "zero weight":
            r = c["ret"].reshape(e, k)
            assert (w[~np.isfinite(r)] == 0).all() and (~np.isfinite(r)).sum() == 3 and (w[np.isfinite(r)] > 0).all(), name
            assert np.isfinite(want["new_mean"]).all() and np.isfinite(rmax).all() and want["nominal_return"][2] == np.inf, name
        if c["expect"] == "nominal":  # parents 0 and 1: sample 0 alone
            assert (rmax[:2] == -np.inf).all() and (w[:2, 0] == 1).all() and (w[:2, 1:] == 0).all() and np.isfinite(rmax[2]), name
            assert same_bits(want["new_mean"][:, :2], np.ascontiguousarray(a[:, :2, 0])), name


def test_harness_equals_numpy(harness, tmp_path):
    compare_map_and_words(harness)
    compare_actions(harness, tmp_path)
    compare_score(harness, tmp_path)
    compare_update(harness, tmp_path)


def test_sanitized_harness(sanitized_harness, tmp_path):
    """The same comparisons on the program built with -fsanitize=address,undefined: any finding ends it with a non-zero status."""
    compare_map_and_words(sanitized_harness)
    compare_actions(sanitized_harness, tmp_path)
    compare_score(sanitized_harness, tmp_path)
    compare_update(sanitized_harness, tmp_path)


def test_update_against_exact_arithmetic():
    """new_mean given w against exact rational arithmetic.  With u = 2^-53: a term w a is one rounding, the ordered sum of K terms adds
    at most 10 + ceil(K / 1024) = 11 roundings on any path to the root (K <= 1024: one term a lane, ten fold levels), Z the same without
    the product, the quotient one more, the conversion to float32 half a float32 ulp.  So |m - exact| <= 25 u sum|w a| / Z + 2^-24 |m|,
    and sum|w a| / Z <= 1 since |a| <= 1."""
    u = 2.0 ** -53
    for name, c in update_cases().items():
        e, k, h = c["E"], c["K"], c["H"]
        if k > 64:
            continue  # the bound is the same; the rationals of 1024 terms are slow
        w, _ = mppi_weights(c["ret"], c["lam"], k)
        got = mppi_update(c["ret"], w, c["actions"], c["shift"])["new_mean"]
        a = c["actions"].reshape(h, e, k, 6)
        for p in range(e):
            Z = sum(Fraction(float(x)) for x in w[p])
            for t in range(h):
                for j in range(6):
                    exact = sum(Fraction(float(x)) * Fraction(float(y)) for x, y in zip(w[p], a[t, p, :, j])) / Z
                    err = abs(Fraction(float(got[t, p, j])) - exact)
                    assert err <= 25 * u + 2.0 ** -24 * abs(exact) + Fraction(2.0 ** -149), (name, p, t, j, float(err))


def test_noise_is_a_function_of_its_counter():
    """mppi_noise depends on (seed, draw, iteration, p, j, h) and on nothing else -- not on how many parents or samples are asked for --
    and differs from the policy noise of the same seed and draw."""
    full = mppi_noise(5, 9, 0, np.arange(3)[:, None, None], np.arange(8)[None, :, None], np.arange(H)[None, None, :])
    assert full.shape == (3, 8, H, 6)
    assert np.array_equal(mppi_noise(5, 9, 0, 1, np.arange(5)[:, None], np.arange(H)[None, :]), full[1, :5])
    for other in (mppi_noise(6, 9, 0, 1, 3, 2), mppi_noise(5, 10, 0, 1, 3, 2), mppi_noise(5, 9, 1, 1, 3, 2), policy_noise(5, 9, 1, "gaussian")):
        assert not np.array_equal(other, full[1, 3, 2])
    assert not full[:, 0].any() and np.abs(full[:, 1:]).min() > 0
    x = mppi_noise(1, 2, 3, np.arange(64)[:, None, None], np.arange(1, 256)[None, :, None], np.arange(4)[None, None, :], dtype=np.float64).ravel()
    assert abs(x.mean()) < 3.3 / np.sqrt(x.size) and abs(x.std() - 1) < 3.3 / np.sqrt(2 * x.size)  # the bounds test_policy_sampling.py uses
    for bad in (dict(draw=1 << 32), dict(iteration=8), dict(samples=1024), dict(steps=64)):
        args = dict(seed=0, draw=0, iteration=0, parents=0, samples=1, steps=0)
        args.update(bad)
        with pytest.raises(ValueError):
            mppi_noise(**args)


def test_struct_mirror_and_symbols(harness):
    lay = run_harness(harness, "layout")
    assert lay.pop("sizeof") == C.sizeof(_abi.Mppi) == 176
    assert lay == {name: getattr(_abi.Mppi, name).offset for name, _ in _abi.Mppi._fields_}
    assert [name for name, _, _ in _abi.MPPI_FIELDS] == [name for name, _ in _abi.Mppi._fields_[11:]]
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    body = hdr[hdr.index("typedef struct urgym_mppi {"):hdr.index("} urgym_mppi;")]
    assert re.findall(r"^\s*(?:int32_t|float|double|uint64_t|uint8_t)\*?\s+(\w+);", body, flags=re.M) == [name for name, _ in _abi.Mppi._fields_]
    lib = _native.lib()
    for sym in SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    for name, value in (("URGYM_MPPI_TAG", "0x4D505000u"), ("URGYM_MPPI_SAMPLES_MAX", _abi.MPPI_SAMPLES_MAX), ("URGYM_MPPI_HORIZON_MAX", _abi.MPPI_HORIZON_MAX),
                        ("URGYM_MPPI_ITERATIONS_MAX", _abi.MPPI_ITERATIONS_MAX)):
        assert re.search(rf"^#define {name} {value}$", hdr, flags=re.M), name
    assert _abi.MPPI_SAMPLES_MAX == _abi.SAC_TERMS_LANES  # one lane per sample: the ordered sum takes one term a lane


def test_refusals_without_a_device():
    """A NULL handle is refused by every entry point before anything else is looked at."""
    lib = _native.lib()
    m = _abi.Mppi()
    calls = ((lib.urgym_mppi_fanout, (None, None, C.byref(m), None)), (lib.urgym_mppi_sample, (None, C.byref(m), 0, 0, None)),
             (lib.urgym_mppi_score, (None, C.byref(m), 0, None)), (lib.urgym_mppi_update, (None, C.byref(m), None)),
             (lib.urgym_mppi_record, (None, C.byref(m), 0, 1, None, None)), (lib.urgym_mppi_plan, (None, None, C.byref(m), 0, None)),
             (lib.urgym_mppi_control, (None, None, C.byref(m), 0, 1, None, None)))
    for call, args in calls:
        assert call(*args) == _abi.ERR_ARG and b"null handle" in lib.urgym_last_error(None)
