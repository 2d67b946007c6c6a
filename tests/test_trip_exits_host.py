"""One GJK iteration of the step kernel after its exits were flattened (ur_gym_amd/csrc/urgym_device.h gjk_advance; DESIGN.md
section 4, round 7), compiled with g++ through tests/trip_exits_harness.cpp and run on the CPU on constructed pairs that take EVERY
exit of the iteration:

  the separating-axis early-out, a duplicate vertex, f0 <= f1, touching cores (nsq < 1e-12), the verdict stop (GJK_CLOSE), no
  progress, the origin inside the tetrahedron, a sliver tetrahedron (four near-coplanar points), the iteration cap.

Two references.  (1) The oracle's GJK (oracle.closest): what it reports of a search -- the iteration count, whether the cores overlap,
the distance -- must be the device code's.  It reports no exit code, no simplex and no separating axis, it has no verdict queries,
and it iterates in another frame (relative to the mid point of the two shapes, the device code in shape B's frame), so its distance
differs from the device's in the last bits on either side of this change: the distances are held to 1e-9 m, the bar of
tests/test_device_header_on_host.py.  (2) For everything the oracle does not report, the iteration AS IT WAS BRANCHED before the
change, restated in the harness (ref_advance) and run in lockstep: after EVERY trip the exit code, GJK_* flags, r.n, r.iter and
the bits of r.v, r.sq and of the simplex vertices must be equal, after the last also gjk_finish's core distance and flags, and
gjk_core_distance (gjk_iterate = gjk_advance + gjk_finish) must return the same bits.  The earlier form also says which exit it
took, so a case cannot quietly stop exercising its exit.

The iteration cap is a constant of the shipped code (r.iter++ > 1000); the harness reaches it by presetting the run's iteration
counter to 1001, and the no-progress exit by presetting the run's squared distance -- 46 000 random pairs of the shapes below did
not end on it once (Bullet's f0 <= f1 and duplicate-vertex tests come first).  The arm `n == 4 after a step that moved` (exit code
3 without GJK_ITERCAP) cannot be reached at all: a closest point rests on at most three vertices and the reduction then leaves at
most three, and an origin inside the tetrahedron gives nv = 0, which the touching-cores test takes first -- the lockstep runs would
still show a difference there.  Test infrastructure; nothing here ships."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libtrip_exits_harness.so")
DP = C.POINTER(C.c_double)

HULL, CYL, BOX, POINT = 0, 1, 2, 3
ARMS = ("none", "separating_axis", "duplicate", "f0_f1", "sliver", "touching", "verdict", "no_progress", "cap", "inside")
GJK_PENETRATING, GJK_ITERCAP, GJK_SEPARATED, GJK_CLOSE = 1, 2, 4, 8
IDENT = [0.0, 0.0, 0.0, 1.0]
OBSTACLE, TRACK = [0.05, 0.4, 0.0], [0.1, 0.55, 0.06]   # cylinder radius / height, box half extents (the scene's)
EXACT = 5.0                                               # getClosestPoints(distance = 5.0)
CONTACT = 0.01                                            # check_collision's margin: a boolean query's two bounds


@pytest.fixture(scope="module")
def harness():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "trip_exits_harness.cpp")
    deps = [src, os.path.join(HERE, "device_harness.cpp"), os.path.join(ROOT, "ur_gym_amd", "csrc", "urgym_device.h"),
            os.path.join(ROOT, "ur_gym_amd", "csrc", "urgym_tables_host.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", SO, src])
    lib = C.CDLL(SO)
    lib.harness_trip_exits.argtypes = [C.c_int, DP, DP, C.c_int, DP, DP, C.c_double, C.c_double, C.c_int, C.c_double, DP]
    return lib


def run(lib, a, b, threshold=EXACT, boolean=False, iter0=0, sq0=0.0):
    """a, b = (type, parameters, pose xyz + quaternion xyzw).  An exact query hands in Bullet's early-out distance margins + 0.02 +
    threshold; a boolean one the margins + the contact margin as both of its bounds (urgym_hip.hip)."""
    (ta, pa, xa), (tb, pb, xb) = a, b
    pa, xa, pb, xb = [np.ascontiguousarray(v, dtype=np.float64) for v in (pa, xa, pb, xb)]
    margins = sum(0.001 if t != POINT else p[0] for t, p in ((ta, pa), (tb, pb)))
    max_d = margins + CONTACT if boolean else margins + 0.02 + threshold
    out = np.zeros(12)
    assert lib.harness_trip_exits(ta, pa.ctypes.data_as(DP), xa.ctypes.data_as(DP), tb, pb.ctypes.data_as(DP), xb.ctypes.data_as(DP),
                                  max_d, max_d if boolean else 0.0, iter0, sq0, out.ctypes.data_as(DP)) == 0
    assert out[11] == margins
    return dict(mismatches=int(out[0]), fin=int(out[1]), info=int(out[2]), n=int(out[3]), iter=int(out[4]), core=out[5], v=out[6:9].copy(),
                arm=ARMS[int(out[9])], trips=int(out[10]), margins=margins)


def against_the_oracle(oracle, got, a, b, threshold=EXACT):
    """What the oracle reports of the same (exact) query."""
    (ta, pa, xa), (tb, pb, xb) = a, b
    ref = oracle.closest(ta, np.asarray(pa, dtype=np.float64), np.asarray(xa, dtype=np.float64), tb, np.asarray(pb, dtype=np.float64),
                         np.asarray(xb, dtype=np.float64), threshold)
    assert bool(got["info"] & GJK_PENETRATING) == ref["penetrating"]
    if not ref["penetrating"]:
        assert got["iter"] == ref["iterations"]
        print("distance", got["core"] - got["margins"], "oracle", ref["distance"], "difference", got["core"] - got["margins"] - ref["distance"])
        assert abs(got["core"] - got["margins"] - ref["distance"]) <= 1e-9
    return ref


def link(k, xyz, quat=IDENT):
    return (HULL, [k, 0.0, 0.0], list(xyz) + list(quat))


def test_separating_axis_early_out(harness):
    # link 3 half a metre from the obstacle, "closer than the contact margin?": the first support point already proves it is not
    got = run(harness, link(3, [0.5, 0.0, 0.3]), (CYL, OBSTACLE, [0, 0, 0] + IDENT), boolean=True)
    assert got["mismatches"] == 0 and got["arm"] == "separating_axis"
    assert got["fin"] == 5 and got["info"] == GJK_SEPARATED and got["core"] > 0.4


def test_duplicate_vertex(harness, oracle):
    # two polytopes: the search ends when the support map returns a vertex the simplex holds already
    a, b = link(3, [0.5, 0.1, 0.3]), (BOX, TRACK, [0, 0, 0] + IDENT)
    got = run(harness, a, b)
    assert got["mismatches"] == 0 and got["arm"] == "duplicate"
    assert got["fin"] == 1 and got["info"] == 0 and got["n"] == 3 and got["iter"] == 12
    against_the_oracle(oracle, got, a, b)


F0_F1 = [  # converged to 1e-12 of the squared distance along v: a smooth shape among the two
    (link(4, [-0.003, 0.005, 0.295]), (CYL, OBSTACLE, [0, 0, 0] + IDENT)),
    ((CYL, [0.03, 0.2, 0.0], [-0.113, -0.046, 0.314] + IDENT), (BOX, TRACK, [0, 0, 0] + IDENT)),
    ((POINT, [0.01, 0.0, 0.0], [-0.009, -0.017, 0.336] + IDENT), (CYL, OBSTACLE, [0, 0, 0] + IDENT)),
    ((CYL, OBSTACLE, [-0.085, -0.046, 0.4] + IDENT), (CYL, OBSTACLE, [0, 0, 0] + IDENT)),
]


@pytest.mark.parametrize("case", range(len(F0_F1)))
def test_f0_f1(harness, oracle, case):
    a, b = F0_F1[case]
    got = run(harness, a, b)
    assert got["mismatches"] == 0 and got["arm"] == "f0_f1"
    assert got["fin"] == 1 and got["info"] == 0 and got["n"] == 3
    against_the_oracle(oracle, got, a, b)


def test_touching_cores(harness, oracle):
    # a point on the corner of the track's core: the first Minkowski-difference point is the origin itself
    a, b = (POINT, [0.01, 0.0, 0.0], [0.099, 0.549, 0.059] + IDENT), (BOX, TRACK, [0, 0, 0] + IDENT)
    got = run(harness, a, b)
    assert got["mismatches"] == 0 and got["arm"] == "touching"
    assert got["fin"] == 1 and got["info"] == GJK_PENETRATING and got["n"] == 1 and got["iter"] == 0 and got["core"] == 0.0
    assert not got["v"].any()
    against_the_oracle(oracle, got, a, b)


def test_verdict_stop(harness):
    # a point 5 mm above the track's core, "closer than margins + contact margin = 21 mm?": yes, as soon as |v| says so
    got = run(harness, (POINT, [0.01, 0.0, 0.0], [0.01, 0.02, 0.064] + IDENT), (BOX, TRACK, [0, 0, 0] + IDENT), boolean=True)
    assert got["mismatches"] == 0 and got["arm"] == "verdict"
    assert got["fin"] == 1 and got["info"] == GJK_CLOSE and 0.0 < got["core"] <= 0.021


def test_no_progress(harness):
    # the run believes it is 1 mm away (sq0) and its first closest point is farther: the previous v stands, r.sq is updated, r.iter not
    got = run(harness, link(3, [0.5, 0.1, 0.3]), (CYL, OBSTACLE, [0, 0, 0] + IDENT), sq0=1.0e-6)
    assert got["mismatches"] == 0 and got["arm"] == "no_progress"
    assert got["fin"] == 1 and got["info"] == 0 and got["n"] == 1 and got["iter"] == 0 and got["trips"] == 1
    assert got["core"] == 1.0  # |v0|: Bullet's start axis stands


def test_origin_inside_the_tetrahedron(harness, oracle):
    # a point well inside the track: the simplex grows to a tetrahedron around the origin
    a, b = (POINT, [0.001, 0.0, 0.0], [0.01, 0.02, 0.01] + IDENT), (BOX, TRACK, [0, 0, 0] + IDENT)
    got = run(harness, a, b)
    assert got["mismatches"] == 0 and got["arm"] == "touching"  # (nv = 0: see the module's docstring)
    assert got["fin"] == 1 and got["info"] == GJK_PENETRATING and got["n"] == 4 and got["core"] == 0.0
    against_the_oracle(oracle, got, a, b)


SLIVER = [  # four near-coplanar Minkowski-difference points: Bullet's closest() fails, the previous v stands
    (link(5, [0.007, 0.27, -0.028]), (CYL, OBSTACLE, [0, 0, 0] + IDENT)),
    ((CYL, [0.03, 0.2, 0.0], [-0.22, -0.058, 0.002] + IDENT), (BOX, TRACK, [0, 0, 0] + IDENT)),
    ((CYL, OBSTACLE, [0.152, 0.023, 0.065] + IDENT), (CYL, OBSTACLE, [0, 0, 0] + IDENT)),
]
# A sliver at which the oracle's search, in its own frame, takes one trip more (13 against 12) -- with the earlier form of the iteration
# exactly as with this one: a plane test within rounding of its 1e-16 threshold (DESIGN.md section 3 on such queries).  Lockstep only.
SLIVER_LOCKSTEP_ONLY = ((POINT, [0.01, 0.0, 0.0], [-0.054, 0.03, -0.086] + IDENT), (CYL, OBSTACLE, [0, 0, 0] + IDENT))


@pytest.mark.parametrize("case", range(len(SLIVER)))
def test_sliver_tetrahedron(harness, oracle, case):
    a, b = SLIVER[case]
    got = run(harness, a, b)
    assert got["mismatches"] == 0 and got["arm"] == "sliver"
    assert got["fin"] == 1 and got["info"] == 0 and got["n"] == 4 and got["core"] > 0.0
    against_the_oracle(oracle, got, a, b)


def test_sliver_tetrahedron_where_the_oracles_path_splits(harness):
    got = run(harness, *SLIVER_LOCKSTEP_ONLY)
    assert got["mismatches"] == 0 and got["arm"] == "sliver"
    assert got["fin"] == 1 and got["info"] == 0 and got["n"] == 4 and got["iter"] == 12


def test_iteration_cap(harness):
    # the counter preset to 1001: the first step that moves ends the search without the simplex check
    got = run(harness, link(3, [0.5, 0.1, 0.3]), (CYL, OBSTACLE, [0, 0, 0] + IDENT), iter0=1001)
    assert got["mismatches"] == 0 and got["arm"] == "cap"
    assert got["fin"] == 3 and got["info"] == GJK_ITERCAP and got["iter"] == 1002 and got["trips"] == 1 and got["core"] == 0.0
    # one below the cap the search goes on to its ordinary end
    got = run(harness, link(3, [0.5, 0.1, 0.3]), (CYL, OBSTACLE, [0, 0, 0] + IDENT), iter0=900)
    assert got["mismatches"] == 0 and got["arm"] in ("duplicate", "f0_f1") and not got["info"] & GJK_ITERCAP


@pytest.mark.parametrize("boolean", [False, True])
def test_random_pairs_in_lockstep(harness, boolean):
    """Links against the obstacle, the track, each other and a small box, boxes against the same, exact and boolean: every trip of
    every search is the earlier form's, and between them the searches end on every exit that random pairs reach."""
    rng = np.random.default_rng(7 + boolean)
    arms = set()
    for k in range(3000):
        quat = Rot.random(random_state=int(rng.integers(1 << 30))).as_quat()
        xyz = rng.uniform([-0.3, -0.3, -0.1], [0.3, 0.3, 0.4])
        a = link(int(rng.integers(1, 7)), xyz, quat) if k % 8 < 6 else (BOX, [0.08, 0.12, 0.05], list(xyz) + list(quat))
        other = [(CYL, OBSTACLE), (BOX, TRACK), (HULL, [int(rng.integers(1, 7)), 0.0, 0.0]), (BOX, [0.1, 0.1, 0.1])][k % 4]
        b = other + (list(rng.uniform(-0.2, 0.2, 3)) + list(Rot.random(random_state=int(rng.integers(1 << 30))).as_quat()),)
        got = run(harness, a, b, boolean=boolean)
        assert got["mismatches"] == 0, (k, got)
        arms.add(got["arm"])
    assert arms >= ({"separating_axis", "verdict", "touching"} if boolean else {"duplicate", "f0_f1", "touching", "sliver"}), arms
