"""GPU tests (-m gpu) of the device penetration depth: the wave-cooperative EPA (urgym_device.h epa_wave), the one part of the
device's float64 geometry that the host harness cannot compile, in the three kernels that call it.

  B  probe kernel against an EXACT reference for polytope pairs (tests/penetration_cases.py: minimum of the support function over
     the finite set of facet-normal candidates of A - B; shares nothing with the expanding polytope)      -> EPA_TOL + 1e-12
  C  probe kernel on the analytic cases of test_oracle.py and a shallow ladder (core overlaps 1e-3, 1e-5, 1e-7 m)   -> 1e-8
  D  probe kernel against the oracle over seven families, with the ORACLE's census asserting that the run held searches that
     stop at the 48-point cap, flagged ones and trivially short ones                                     -> LD_TOL, flags equal
  E  one wave serves its penetrating lanes one after the other from one LDS workspace: (dist, info) bitwise independent of what
     else is in the call
  F  step kernel: the service wave's table / track marks, kept in link_dist by check_collision=False + WORKBENCH + no auto-reset
  G  refresh kernel under WORKBENCH
Every minimum count below is asserted on the oracle's side, never on the kernel's output.  Run with -s for the census tables
(profiles/r4/gpu_tests_penetration_depth.txt).
"""
import numpy as np
import pytest
import torch

import penetration_cases as pc
from test_gpu_parity import LD_TOL, OBS_TOL, make_vec, np_, obs_diff, step_both
from ur_gym_amd import _abi

pytestmark = pytest.mark.gpu

PENETRATING, ITERCAP = 1, 2  # urgym_device.h: GJK_PENETRATING, GJK_ITERCAP


@pytest.fixture(scope="module")
def env():
    e = make_vec("UR5DynReach-v1", num_envs=64, seed=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def families(oracle):
    """Part D's queries and the oracle's census of them, computed once (E draws its penetrating set from the same rows)."""
    queries = pc.family_queries()
    return queries, pc.oracle_census(oracle, queries)


def probe(env, queries):
    if not queries:
        return np.zeros(0), np.zeros(0, np.int32)
    return env.probe_closest(*[[q[k] for q in queries] for k in range(6)])


def test_probe_against_the_exact_polytope_reference(oracle, env):
    """B.  Hull <-> track / table / cube, rotated box <-> box, hull <-> the 70-vertex link 6: the device within EPA_TOL + 1e-12 of
    the exact depth, on queries whose oracle search converged below the cap (then depth - d_best <= gain <= EPA_TOL by
    construction of an expanding polytope: the best face is inside A - B, its support plane outside)."""
    cases = pc.polytope_queries()
    queries = [q for _, q in cases]
    ref = np.array([pc.exact_polytope_distance(q) for q in queries])
    orc = []
    for (label, q), r in zip(cases, ref):
        got = oracle.closest(*q)
        assert got["penetrating"] and oracle.last_epa_iterations() < pc.EPA_CAP, (label, got)
        assert abs(got["distance"] - r) <= pc.EPA_TOL + 1e-12, (label, got, r)
        orc.append(got["distance"])
    d, info = probe(env, queries)
    print()
    for label in dict.fromkeys(l for l, _ in cases):
        m = np.array([l == label for l, _ in cases])
        print(f"  B {label:14s} {int(m.sum()):3d} pairs: device vs exact {np.abs(d[m] - ref[m]).max():.2e}, oracle vs exact "
              f"{np.abs(np.array(orc)[m] - ref[m]).max():.2e}, depth {-ref[m].max():.4f} .. {-ref[m].min():.4f}")
    assert (info & PENETRATING).all() and not (info & ITERCAP).any()
    err = np.abs(d - ref)
    assert err.max() <= pc.EPA_TOL + 1e-12, (cases[int(err.argmax())], d[int(err.argmax())], ref[int(err.argmax())])


def test_probe_on_the_analytic_cases(oracle, env):
    """C.  test_oracle.py::test_penetration_depth_analytic_cases through the device, and the shallow ladder (all three rungs: the
    oracle holds each to 1e-8 on the CPU, asserted here as well)."""
    cases = pc.analytic_cases()
    d, info = probe(env, [q for _, q, _, _ in cases])
    print()
    for (name, q, want, tol), dk, ik in zip(cases, d, info):
        got = oracle.closest(*q)
        assert got["penetrating"] and abs(got["distance"] - want) < tol, (name, got)
        print(f"  C {name:30s} expected {want:.9f}: device {dk - want:+.2e}, oracle {got['distance'] - want:+.2e}")
        assert ik & PENETRATING and abs(dk - want) < tol, (name, dk, want)
    a, b = pc.rigid_motion_pair()
    (d0, d1), info = probe(env, [a, b])
    assert (info & PENETRATING).all() and d0 < -0.002 and abs(d1 - d0) < 1e-7, (d0, d1)
    assert abs(d0 - oracle.closest(*a)["distance"]) < LD_TOL


def test_probe_against_the_oracle_by_family(oracle, env, families):
    """D.  Same flag, same distance, same `capped` verdict (bit GJK_ITERCAP of info == the oracle's iterations == 1001) on every
    query of seven families; the oracle's census guarantees what the comparison covered.  Every penetration depth must agree to
    LD_TOL.  The few queries of these families whose cores do NOT overlap are GJK distances, and LD_TOL is test_gpu_parity's
    bound with its exception: at an ill-conditioned GJK query the oracle's own answer jumps between values 1e-8 .. 1e-5 apart under
    a 1e-14 perturbation of the pose.  So every separated query is compared with the range the ORACLE produces under that
    perturbation, widened by LD_TOL -- a single value wherever the query is well-conditioned.  (Spheres a millimetre outside the
    cylinder's core are ill-conditioned more often than not: a point against a curved surface; the device has always landed on
    one of the oracle's own two or three answers to the last digit.)"""
    queries, rows = families
    print("\n" + "\n".join(pc.census_table(rows, pc.FAMILIES)))
    pc.assert_census_conditions(rows)
    d, info = probe(env, [q for _, q in queries])
    worst, unstable, separated = {}, 0, 0
    rng = np.random.default_rng(0)
    for k, ((fam, q), r) in enumerate(zip(queries, rows)):
        assert bool(info[k] & PENETRATING) == r["penetrating"], (fam, k, info[k], r)
        assert bool(info[k] & ITERCAP) == r["capped"], (fam, k, info[k], r)
        diff = abs(d[k] - r["distance"])
        if not r["penetrating"]:
            # the oracle's own range at this query, from the oracle alone; a well-conditioned query has lo == hi: LD_TOL as it stands
            vals = [oracle.closest(q[0], q[1], np.r_[q[2][:3] + rng.normal(0, 1e-14, 3), q[2][3:]], q[3], q[4], q[5])["distance"] for _ in range(200)]
            lo, hi = min(vals + [r["distance"]]), max(vals + [r["distance"]])
            separated += 1
            if hi - lo > LD_TOL:
                unstable += 1
                print(f"  D {fam} query {k}: separated and ill-conditioned, the oracle's own answers span {hi - lo:.2e}; device {d[k]!r} in [{lo!r}, {hi!r}]")
            assert lo - LD_TOL <= d[k] <= hi + LD_TOL, (fam, k, d[k], lo, hi)
            continue
        worst[fam] = max(worst.get(fam, 0.0), diff)
        assert diff <= LD_TOL, (fam, k, q, d[k], r)
    print(f"  D {separated} separated queries, {unstable} of them ill-conditioned by the oracle's own spread")
    for fam in pc.FAMILIES:
        print(f"  D {fam:20s} device vs oracle {worst[fam]:.2e}")
    # the coaxial family has a closed form (test_oracle.py::test_coplanar_points_do_not_derail_the_expanding_polytope): the device
    # against it directly -- EPA_TOL where the oracle's search converged, EPA_CAP_RESIDUAL where it stopped at the cap unflagged
    err = [0.0, 0.0]
    for k, ((fam, q), r) in enumerate(zip(queries, rows)):
        if fam == "box<->cyl coaxial":
            e = abs(d[k] - pc.coaxial_closed_form(q))
            assert e <= (pc.EPA_CAP_RESIDUAL if r["at_cap"] else pc.EPA_TOL + 1e-12), (k, q, d[k], e)
            err[r["at_cap"]] = max(err[r["at_cap"]], e)
    print(f"  D box<->cyl coaxial    device vs closed form: converged {err[0]:.2e}, at the cap {err[1]:.2e}")


def test_probe_results_do_not_depend_on_the_rest_of_the_call(env, families):
    """E.  About 200 penetrating queries in order (three blocks whose 64 lanes all penetrate), permuted, interleaved with separated
    ones, one per call, and as the last query of calls of 1, 63, 64, 65 and 129 (the idle lanes of the last block shadow it):
    (dist, info) of every query bitwise the same."""
    queries, rows = families
    pen = [q for (_, q), r in zip(queries, rows) if r["penetrating"]]
    pen = pen[::max(1, len(pen) // 200)][:200]
    assert len(pen) >= 192  # three full blocks
    sep = [(q[0], q[1], q[2], q[3], q[4], np.r_[q[5][:3] + [2.0, 0.0, 0.0], q[5][3:]]) for q in pen]  # the same pairs, 2 m apart
    bits = lambda d, i: (np.asarray(d).view(np.int64), np.asarray(i))
    base_d, base_i = bits(*probe(env, pen))
    assert (base_i & PENETRATING).all()
    sep_d, sep_i = bits(*probe(env, sep))
    assert not (sep_i & PENETRATING).any()

    def same(got, idx, what):
        d, i = bits(*got)
        assert np.array_equal(d, base_d[idx]) and np.array_equal(i, base_i[idx]), what

    perm = np.random.default_rng(3).permutation(len(pen))
    same(probe(env, [pen[k] for k in perm]), perm, "permuted")
    mixed = [x for pair in zip(sep, pen) for x in pair]
    d, i = probe(env, mixed)
    same((d[1::2], i[1::2]), np.arange(len(pen)), "interleaved with separated queries")
    assert np.array_equal(bits(d[0::2], i[0::2])[0], sep_d) and np.array_equal(i[0::2], sep_i)
    for k in range(0, len(pen), len(pen) // 10):
        same(probe(env, [pen[k]]), [k], f"query {k} alone")
    for count in (1, 63, 64, 65, 129):
        last = (7 * count) % len(pen)
        d, i = probe(env, mixed[:count - 1] + [pen[last]])
        same((d[-1:], i[-1:]), [last], f"last of {count}")
        same((d[1:count - 1:2], i[1:count - 1:2]), np.arange((count - 1) // 2), f"the others of {count}")


@pytest.mark.parametrize("env_id,kind,step_envs", [("UR5ObsReach-v1", _abi.ENV_OBS, None), ("UR5ObsReach-v1", _abi.ENV_OBS, 100),
                                                   ("UR5DynReach-v1", _abi.ENV_DYN, None), ("UR5DynReach-v1", _abi.ENV_DYN, 100)])
def test_step_keeps_table_and_track_depths(oracle, monkeypatch, env_id, kind, step_envs):
    """F.  check_collision=False + WORKBENCH + no auto-reset is the one configuration in which the depths of the service wave's
    table and track marks (merged with atomicMin) stay in link_dist: every step against the oracle, and the oracle's per-body
    recomputation shows that table and track did supply minima, that two EPA results met in one cell, and that one env had
    several marks."""
    if step_envs:
        monkeypatch.setenv("URGYM_STEP_ENVS", str(step_envs))  # two waves' worth of envs per workgroup
    n, steps, seed = 512, 25, 43
    cfg = dict(check_collision=False, link_dist_scope=_abi.LINK_DIST_WORKBENCH, auto_reset=False)
    env = make_vec(env_id, num_envs=n, seed=seed, **cfg)
    orc = oracle.OracleEnv(kind, n, threads=8, check_collision=0, link_dist_scope=_abi.LINK_DIST_WORKBENCH, auto_reset=0)
    env.reset(seed=seed)
    orc.reset(seed=seed)
    rng = np.random.default_rng(seed)
    deep, by_body, two, multi, err = 0, np.zeros(3, int), 0, 0, 0.0
    for t in range(steps):
        a = rng.uniform(-1, 1, (n, 6)).astype(np.float32)
        step_both(oracle, kind, env, orc, a, where=f"{env_id} workbench depths step {t}")
        assert np.array_equal(np_(env.buf["status"]), orc.buf["status"]), t
        c = pc.workbench_census(oracle, orc.buf, cap=60)
        deep, by_body, two, multi = deep + c["deep"], by_body + c["by_body"], two + c["two_bodies_deep"], multi + c["envs_multi_deep"]
        err = max(err, c["recompute_err"])
    print(f"\n  F {env_id} step_envs={step_envs}: {deep} deep cells; minimum by obstacle/table/track (first 60 per step) "
          f"{by_body.tolist()}; cells with two bodies deep {two}; env-steps with >= 2 deep links {multi}; recomputation within {err:.1e}")
    assert err < 1e-5  # (the bookkeeping above, not the kernel: searches that stop at the cap differ by up to ~2e-6 between routes)
    assert by_body[1] >= 100 and by_body[2] >= 10 and two >= 5 and multi >= 50
    env.close()


def test_refresh_under_workbench_reports_table_track_and_obstacle_depths(oracle):
    """G.  set_state + refresh with the arm bent down over the base -- upper arm in the track, forearm through the table top -- and
    the obstacle inside a link of every third env: the REFRESH kernel's EPA under WORKBENCH against the oracle, then one step."""
    n = 48
    cfg = dict(auto_reset=False, link_dist_scope=_abi.LINK_DIST_WORKBENCH)
    env = make_vec("UR5ObsReach-v1", num_envs=n, seed=7, **cfg)
    orc = oracle.OracleEnv(_abi.ENV_OBS, n, auto_reset=0, link_dist_scope=_abi.LINK_DIST_WORKBENCH)
    env.reset(seed=7)
    orc.reset(seed=7)
    state = pc.refresh_workbench_state(oracle, n)
    orc.load_state(state)
    orc.refresh()
    env.set_state(state, refresh=True)
    torch.cuda.synchronize()
    c = pc.workbench_census(oracle, orc.buf, cap=10 ** 6)
    envs = [len(s) for s in c["envs_by_body"]]
    print(f"\n  G {c['deep']} deep cells; minimum by obstacle/table/track in {envs} envs ({c['by_body']} cells); cells with two bodies "
          f"deep {c['two_bodies_deep']}; envs with >= 2 deep links {c['envs_multi_deep']}")
    assert min(envs) >= 3 and c["recompute_err"] < 1e-5
    st = env.get_state()
    assert np.abs(st["obst_pos"] - orc.buf["obst_pos"]).max() < 1e-12 and np.abs(st["obst_quat"] - orc.buf["obst_quat"]).max() < 1e-12
    assert np.abs(st["link_dist"] - orc.buf["link_dist"]).max() < 1e-8
    assert np.array_equal(np_(env.buf["collision"]), orc.buf["collision"]) and orc.buf["collision"].sum() >= n // 2
    assert np.array_equal(np_(env.buf["status"]), orc.buf["status"])
    assert obs_diff(_abi.ENV_OBS, np_(env.buf["observation"]), orc.buf["observation"]) < OBS_TOL
    a = np.random.default_rng(7).uniform(-0.2, 0.2, (n, 6)).astype(np.float32)
    step_both(oracle, _abi.ENV_OBS, env, orc, a, where="after the workbench refresh")
    assert np.array_equal(np_(env.buf["status"]), orc.buf["status"])
    env.close()
