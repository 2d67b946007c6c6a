"""Host tests (-m "not gpu") of the separated side of the closest-distance code: the CPU oracle and the device header compiled for
the host (tests/device_harness.cpp), both against the self-certifying reference of tests/separation_cases.py -- a bracket (lo, up)
of the true distance that shares nothing with Bullet's Voronoi simplex, which the oracle and urgym_device.h both restate.

  1  the reference checks itself: the committed brackets are reproduced, closed forms lie inside them, rigid motions and swapping
     A and B leave them alone, and the numpy forward kinematics the GPU tests pose links with agrees with the oracle's
  2  oracle and device header on every committed query: never below the truth, within LD_TOL above it on the stable set, within
     SLIVER_CAP elsewhere; the census of what that covered is asserted on the oracle's side
  3  the per-cell brackets of the step / refresh tests (separation_cases.link_brackets) on the ORACLE's own environments
Run with -s for the tables (DESIGN.md section 3 quotes them).
"""
import ctypes as C

import numpy as np
import pytest

import separation_cases as sc
from test_device_header_on_host import harness  # noqa: F401  (the fixture that builds tests/_build/libdevice_harness.so)
from ur_gym_amd import _abi

AT = lambda x, y, z: np.r_[x, y, z, 0.0, 0.0, 0.0, 1.0]


@pytest.fixture(scope="module")
def fixture():
    return sc.load_fixture()


@pytest.fixture(scope="module")
def rows(oracle, fixture):
    return sc.oracle_rows(oracle, fixture[0])


def harness_distance(lib, q):
    dp = C.POINTER(C.c_double)
    arr = [np.ascontiguousarray(np.r_[np.asarray(x, np.float64), np.zeros(3)][:n]) for x, n in ((q[1], 3), (q[2], 7), (q[4], 3), (q[5], 7))]
    out = np.zeros(2)
    lib.harness_closest(q[0], arr[0].ctypes.data_as(dp), arr[1].ctypes.data_as(dp), q[3], arr[2].ctypes.data_as(dp), arr[3].ctypes.data_as(dp), 5.0,
                        out.ctypes.data_as(dp))
    return out[0], int(out[1])


# ------------------------------------------------------------------------------------------------ 1: the reference itself
def test_fixture_is_reproduced(fixture):
    cases, lo, up = fixture
    assert len(cases) == 7 * sc.FAR_COUNT + sum(sc.NEAR.values())
    again = np.array([sc.exact_separation(q) for _, q in cases])
    assert np.abs(again[:, 0] - lo).max() <= 1e-13 and np.abs(again[:, 1] - up).max() <= 1e-13
    # the far families are drawn afresh as well (cheap); the near ones are placed by a bisection of half a second each
    k = 0
    for fam in sc.FAR:
        for q in sc.far_queries(fam, sc.SEEDS[fam]):
            got = cases[k][1]
            assert cases[k][0] == fam and got[0] == q[0] and got[3] == q[3] and list(got[1]) == list(q[1]) and list(got[4]) == list(q[4])
            assert np.abs(got[2] - q[2]).max() <= 1e-15 and np.abs(got[5] - q[5]).max() <= 1e-15  # (a quaternion's norm may round differently)
            k += 1
    # every near query sits at a gap inside the range it was drawn from
    near = np.array([f in sc.NEAR for f, _ in cases])
    assert (up[near] >= sc.GAP_LO - 1e-12).all() and (up[near] <= sc.GAP_HI + 1e-12).all()


def closed_forms():
    box, core = [0.1, 0.1, 0.1], 0.099
    r, h = sc.CYL[0] - sc.MARGIN, 0.5 * sc.CYL[1] - sc.MARGIN
    sph = (sc.SPHERE, [sc.SPHERE_R, 0, 0])
    gap = 0.3 - 2 * core
    out = [
        ("box<->box face", (sc.BOX, box, AT(0, 0, 0), sc.BOX, box, AT(0.3, 0.02, 0.01)), gap - 0.002),
        ("box<->box edge", (sc.BOX, box, AT(0, 0, 0), sc.BOX, box, AT(0.3, 0.3, 0.01)), np.sqrt(2.0) * gap - 0.002),
        ("box<->box corner", (sc.BOX, box, AT(0, 0, 0), sc.BOX, box, AT(0.3, -0.3, 0.3)), np.sqrt(3.0) * gap - 0.002),
        ("cube above the table", (sc.BOX, [0.05] * 3, AT(0.5, 0.1, 0.03), sc.BOX, sc.TABLE_HALF, sc.TABLE_POSE), (0.03 - 0.049) - (-0.58 + 0.459) - 0.002),
        ("sphere<->cylinder side", sph + (AT(0.2, 0.1, 0.05), sc.CYLZ, sc.CYL, AT(0, 0, 0)), np.hypot(0.2, 0.1) - r - 0.021),
        ("sphere<->cylinder cap", sph + (AT(0.01, -0.02, 0.5), sc.CYLZ, sc.CYL, AT(0, 0, 0)), 0.5 - h - 0.021),
        ("sphere<->cylinder rim", sph + (AT(0.12, 0.09, -0.3), sc.CYLZ, sc.CYL, AT(0, 0, 0)), np.hypot(0.15 - r, 0.3 - h) - 0.021),
        ("sphere<->box face", sph + (AT(0.05, 0.3, -0.02), sc.BOX, box, AT(0, 0, 0)), (0.3 - core) - 0.021),
        ("sphere<->box edge", sph + (AT(0.05, 0.3, -0.4), sc.BOX, box, AT(0, 0, 0)), np.hypot(0.3 - core, 0.4 - core) - 0.021),
        ("sphere<->box corner", sph + (AT(-0.2, 0.3, -0.4), sc.BOX, box, AT(0, 0, 0)), np.sqrt((0.2 - core) ** 2 + (0.3 - core) ** 2 + (0.4 - core) ** 2) - 0.021),
    ]
    return out


def test_closed_forms_lie_inside_the_bracket(oracle, harness):
    print()
    for name, q, want in closed_forms():
        lo, up = sc.exact_separation(q)
        d, dh = oracle.closest(*q)["distance"], harness_distance(harness, q)[0]
        print(f"  {name:24s} expected {want:.12f}: bracket [{lo - want:+.1e}, {up - want:+.1e}], oracle {d - want:+.1e}, device header {dh - want:+.1e}")
        assert up - lo <= sc.BRACKET_CAP and lo - 1e-13 <= want <= up + 1e-13, (name, lo, up, want)
        assert abs(d - want) <= sc.LD_TOL and abs(dh - want) <= sc.LD_TOL, (name, d, dh, want)


def _moved(q, R, t):
    mv = lambda p: np.r_[R @ p[:3] + t, sc.matrix_to_quat(R @ sc.quat_to_matrix(p[3:]))]
    return (q[0], q[1], mv(q[2]), q[3], q[4], mv(q[5]))


def test_bracket_is_invariant_under_rigid_motion_and_swap(fixture):
    cases, lo, up = fixture
    rng = np.random.default_rng(5)
    pick = np.arange(0, len(cases), 9)
    worst = [0.0, 0.0]
    for k in pick:
        q = cases[k][1]
        if not sc.kept(lo[k], up[k]) or up[k] < -2 * sc.MARGIN + 1e-9:
            continue
        R = sc.quat_to_matrix(rng.normal(size=4))
        a = sc.exact_separation(_moved(q, R, rng.uniform(-1, 1, 3)))
        b = sc.exact_separation((q[3], q[4], q[5], q[0], q[1], q[2]))
        worst = [max(worst[0], abs(a[0] - lo[k]), abs(a[1] - up[k])), max(worst[1], abs(b[0] - lo[k]), abs(b[1] - up[k]))]
    print(f"\n  {len(pick)} queries: bracket moves by {worst[0]:.1e} under a rigid motion, {worst[1]:.1e} under swapping A and B")
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12


def test_numpy_fk_agrees_with_the_oracle(oracle):
    rng = np.random.default_rng(1)
    worst = 0.0
    for k in range(200):
        q = rng.uniform(-2 * np.pi, 2 * np.pi, 6) if k else np.zeros(6)
        R, t = sc.numpy_fk(q)
        Ro, to = oracle.fk(q)
        worst = max(worst, np.abs(R - Ro).max(), np.abs(t - to).max())
        Rq = sc.quat_to_matrix(sc.matrix_to_quat(R[6]))
        worst = max(worst, np.abs(Rq - R[6]).max())
    assert worst <= 1e-12, worst


# ------------------------------------------------------------------------------------------------ 2: oracle and device header
def test_census_of_the_committed_queries(fixture, rows):
    cases, lo, up = fixture
    print("\n" + "\n".join(sc.census_table(rows, lo, up)))
    sep = [k for k, r in enumerate(rows) if not r["penetrating"] and sc.kept(lo[k], up[k])]
    print(f"  {len(rows)} queries, {len(sep)} separated with a kept bracket (widest kept {max(up[k] - lo[k] for k in sep):.1e}), "
          f"{sum(rows[k]['stable'] for k in sep)} stable, {sum(rows[k]['exit'] == sc.SLIVER_EXIT for k in sep)} sliver exits")
    sc.assert_census_conditions(rows, lo, up)


def test_oracle_against_the_bracket(fixture, rows):
    cases, lo, up = fixture
    d = np.array([r["distance"] for r in rows])
    worst = sc.assert_against_bracket(d, rows, lo, up, "oracle")
    print(f"\n  oracle: largest d - up {worst[0]:+.2e} on the stable set, {worst[1]:+.2e} off it (SLIVER_CAP {sc.SLIVER_CAP:.3e})")
    # SLIVER_CAP is twice what the oracle shows on these very queries: the recorded measurement must still be the oracle's
    assert abs(worst[1] - sc.ORACLE_MAX_EXCESS) <= 1e-3 * sc.ORACLE_MAX_EXCESS, worst


def test_device_header_against_the_bracket(harness, fixture, rows):
    cases, lo, up = fixture
    got = [harness_distance(harness, q) for _, q in cases]
    d = np.array([g[0] for g in got])
    for (fam, _), g, r in zip(cases, got, rows):
        assert bool(g[1] & 1) == r["penetrating"], (fam, g, r)  # GJK_PENETRATING
    print("\n" + "\n".join(sc.census_table(rows, lo, up, values=d, title="device header on the host")))
    worst = sc.assert_against_bracket(d, rows, lo, up, "device header")
    print(f"  device header: largest d - up {worst[0]:+.2e} on the stable set, {worst[1]:+.2e} off it")


# ------------------------------------------------------------------------------------------------ 3: per-cell brackets
@pytest.mark.parametrize("kind,workbench", [(_abi.ENV_OBS, False), (_abi.ENV_DYN, False), (_abi.ENV_OBS, True)])
def test_link_brackets_on_the_oracles_own_steps(oracle, kind, workbench):
    """What tests/test_separation.py asserts of the step kernel, asserted of the oracle first: the cells of link_dist after steps 1
    and 25 of 100 auto-resetting envs lie in the brackets that numpy FK and the reference give for the state's own q and obstacle
    pose.  (It also shows that the state of an env that was auto-reset in the step is consistent: the cells belong to the new q.)"""
    n, seed = 100, 61
    scope = _abi.LINK_DIST_WORKBENCH if workbench else 0
    orc = oracle.OracleEnv(kind, n, threads=8, link_dist_scope=scope)
    orc.reset(seed=seed)
    rng = np.random.default_rng(seed)
    cells = negative = dropped = 0
    worst = 0.0
    for t in range(1, 26):
        orc.step(rng.uniform(-1, 1, (n, 6)).astype(np.float32))
        if t not in (1, 25):
            continue
        st = {k: orc.buf[k].copy() for k in ("q", "obst_pos", "obst_quat", "link_dist")}
        c = sc.assert_cells_against_brackets(st, workbench, f"oracle kind {kind} step {t}")
        cells, negative, dropped, worst = cells + c["cells"], negative + c["negative"], dropped + c["dropped"], max(worst, c["excess"])
    print(f"\n  kind {kind} workbench {workbench}: {cells} cells, {negative} negative, {dropped} dropped, largest d - up {worst:+.2e}")
    assert dropped <= sc.DROP_SHARE * cells
    orc.close()


def test_link_brackets_on_the_oracles_own_refresh(oracle):
    """What tests/test_separation.py asserts of the refresh kernel, asserted of the oracle first: 48 envs with the obstacle placed by
    the reference 0.1 .. 20 mm from one link of each.  The targeted cell's bracket, formed from the state the refresh left (the
    project's own conversion of obst_start's angles), must hold the gap that was asked for."""
    n = 48
    state, links, gaps = sc.refresh_near_state(n)
    orc = oracle.OracleEnv(_abi.ENV_OBS, n, auto_reset=0)
    orc.reset(seed=9)
    orc.load_state(state)
    orc.refresh()
    st = {k: orc.buf[k].copy() for k in ("q", "obst_pos", "obst_quat", "link_dist")}
    sc.assert_refresh_coverage(st, links, gaps)
    c = sc.assert_cells_against_brackets(st, False, "oracle refresh")
    print(f"\n  refresh: {c['cells']} cells, {c['negative']} negative, {c['dropped']} dropped, largest d - up {c['excess']:+.2e}")
    assert c["dropped"] <= sc.DROP_SHARE * c["cells"]
    orc.close()
