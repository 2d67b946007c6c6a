"""The culling predicate of the step kernel's per-env phase without its square roots (ur_gym_amd/csrc/urgym_device.h cull_bound2,
seg_box_lower_bound2, segseg_dist2), compiled with g++ through tests/p1_cull_harness.cpp and run on the
CPU beside the root form it replaces in the step kernels without the penetration-depth phase, on a seeded census of poses:

  random joints within their limits; joints at their limits, at zero and at multiples of pi / 2; and poses in which one joint has been
  bisected to the two neighbouring float64 values between which the root form of one pair changes its verdict -- there the bound equals
  the margin sum to within the last bits -- judged under the margin sum itself and under it moved by -2 .. +2 ulp.

Two conditions, per mode and margin: NO pair is kept by the root form and culled by the squared form (a culled pair is never queried:
that would be a missed collision), and every pair kept by the squared form alone lies within its slack band (its capsule distance
exceeds the bound by no more than 1e-12, relative; such a pair costs one exact query and changes no output).  The counts are
printed.  Test infrastructure; nothing here ships."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libp1_cull_harness.so")
MODES = {"random": 0, "limits": 1, "bisected": 2}
COUNTS = {"random": 200000, "limits": 50000, "bisected": 4000}
MARGINS = (0.01, 0.0, 0.05)  # check_collision's contact margin (pyb_setup.py:402-422), none, a wide one


@pytest.fixture(scope="module")
def harness():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "p1_cull_harness.cpp")
    deps = [src, os.path.join(HERE, "p1_chain.h"), os.path.join(ROOT, "ur_gym_amd", "csrc", "urgym_device.h"), os.path.join(ROOT, "data", "ur5e_model.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", SO, src])
    lib = C.CDLL(SO)
    lib.harness_cull_census.argtypes = [C.c_int, C.c_int, C.c_ulonglong, C.c_double, C.POINTER(C.c_long)]
    return lib


def census(lib, mode, count, seed, margin):
    out = (C.c_long * 8)()
    assert lib.harness_cull_census(MODES[mode], count, seed, margin, out) == 0
    keys = ("pairs", "kept_root", "kept_squared", "lost", "added", "added_outside_band", "poses", "bisected")
    return dict(zip(keys, out))


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("mode", list(MODES))
def test_the_squared_form_keeps_what_the_root_form_keeps(harness, mode, margin):
    got = census(harness, mode, COUNTS[mode], 20260 + MODES[mode], margin)
    print(mode, "margin", margin, got)
    assert got["pairs"] == 19 * got["poses"] and got["poses"] > 0
    assert got["lost"] == 0                 # kept by the root form, culled by the squared form: never
    assert got["added_outside_band"] == 0   # kept by the squared form alone: only within the slack band
    assert got["kept_squared"] == got["kept_root"] + got["added"]
    if mode == "bisected":
        # the census does reach the boundary: a drawn (joint, pair) often cannot change the pair's verdict at all (a joint behind the
        # link, a pair far from its bound at every angle), but hundreds of bisections do end between two neighbouring angles
        assert got["bisected"] >= COUNTS[mode] // 10 and got["poses"] == 10 * got["bisected"]
    else:
        assert got["poses"] == COUNTS[mode]
        # culling does cull, and does keep: neither form is trivially true or false on this census
        assert 0 < got["kept_root"] < got["pairs"]
