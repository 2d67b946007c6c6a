"""GPU tests (-m gpu) of the SEPARATED side of the device GJK -- the distances of the probe, step and refresh kernels -- against the
self-certifying reference of tests/separation_cases.py: a bracket (lo, up) of the true distance from a search that shares nothing
with Bullet's Voronoi simplex, which the oracle and urgym_device.h both restate (a defect the two shared would pass every parity test).

  a  probe kernel on all committed queries (tests/golden/separation_queries.npz: seven far and four near-contact families):
     never below the truth, within LD_TOL above it on the stable set, within SLIVER_CAP elsewhere and there on one of the
     oracle's own branches; bitwise the same when the call is permuted
  b  calls of 1, 63, 64, 65 and 129 near-contact queries: every value bitwise that of the full call
  c  step kernel: link_dist of 100 auto-resetting envs after steps 1 and 25 against brackets formed from get_state() with a numpy
     forward kinematics of its own, under OBSTACLE (Obs, Dyn) and WORKBENCH (Obs)
  d  refresh kernel: 48 envs with the obstacle placed by the reference 0.1 .. 20 mm from a link of each; the same bounds, and
     every cell on one of the oracle's branches
Which queries are stable, which searches end in the sliver exit and what a run must cover is decided on the oracle's side
(separation_cases.oracle_rows / assert_census_conditions), never on a kernel's output.  Run with -s for the tables
(profiles/r10/gpu_tests_separation.txt).
"""
import numpy as np
import pytest
import torch

import separation_cases as sc
from test_gpu_parity import link_dist_slack, make_vec
from ur_gym_amd import _abi

pytestmark = pytest.mark.gpu

PENETRATING, ITERCAP = 1, 2  # urgym_device.h: GJK_PENETRATING, GJK_ITERCAP


@pytest.fixture(scope="module")
def env():
    e = make_vec("UR5DynReach-v1", num_envs=64, seed=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def data(oracle):
    """The committed queries, their brackets and the oracle's rows (distance, exit, stable set), computed once and left unchanged."""
    cases, lo, up = sc.load_fixture()
    return cases, lo, up, sc.oracle_rows(oracle, cases)


def probe(env, queries):
    return env.probe_closest(*[[q[k] for q in queries] for k in range(6)])


@pytest.fixture(scope="module")
def full_call(env, data):
    """ONE probe call with every committed query: (dist, info)."""
    return probe(env, [q for _, q in data[0]])


bits = lambda d, i: (np.asarray(d, np.float64).view(np.int64), np.asarray(i))


def test_probe_against_the_brackets(oracle, env, data, full_call):
    """a."""
    cases, lo, up, rows = data
    sc.assert_census_conditions(rows, lo, up)
    d, info = full_call
    assert len(d) == len(cases) >= 1700
    perm = np.random.default_rng(4).permutation(len(cases))
    dp, ip = probe(env, [cases[k][1] for k in perm])
    assert np.array_equal(bits(dp, ip)[0], bits(d, info)[0][perm]) and np.array_equal(ip, info[perm]), "permuted call"
    pen = np.array([r["penetrating"] for r in rows])
    assert np.array_equal((info & PENETRATING) != 0, pen), "GJK_PENETRATING where, and only where, the oracle's cores overlap"
    assert not (info[~pen] & (PENETRATING | ITERCAP)).any()
    print("\n" + "\n".join(sc.census_table(rows, lo, up, values=d, title="MI355X probe kernel")))
    worst = sc.assert_against_bracket(d, rows, lo, up, "probe kernel")
    print(f"  probe kernel: largest d - up {worst[0]:+.2e} on the stable set, {worst[1]:+.2e} off it (SLIVER_CAP {sc.SLIVER_CAP:.3e}); "
          f"lowest d - lo {min(d[k] - lo[k] for k in range(len(d)) if not pen[k]):+.2e}")
    # off the stable set the device must be on one of the ORACLE's branches: within LD_TOL of its answer, or inside the range of its
    # answers under the 1e-14 perturbation (the rule of test_probe_against_the_oracle_by_family: 200 further moves where needed)
    rng = np.random.default_rng(0)
    off = by_range = 0
    for k, ((fam, q), r) in enumerate(zip(cases, rows)):
        if pen[k] or r["stable"]:
            continue
        off += 1
        if abs(d[k] - r["distance"]) <= sc.LD_TOL:
            continue
        by_range += 1
        a, b = r["d_min"], r["d_max"]
        if not a - sc.LD_TOL <= d[k] <= b + sc.LD_TOL:
            vals = [oracle.closest(q[0], q[1], np.r_[q[2][:3] + rng.normal(0, sc.PERTURB, 3), q[2][3:]], q[3], q[4], q[5])["distance"] for _ in range(200)]
            a, b = min(vals + [a]), max(vals + [b])
        assert a - sc.LD_TOL <= d[k] <= b + sc.LD_TOL, (fam, k, d[k], r["distance"], a, b)
    print(f"  {off} separated queries off the stable set: {off - by_range} within LD_TOL of the oracle, {by_range} inside the oracle's own range only")
    st = np.array([r["stable"] for r in rows])
    print(f"  on the stable set: device vs oracle {np.abs(d - np.array([r['distance'] for r in rows]))[st].max():.2e}")


def test_probe_call_sizes(env, data, full_call):
    """b.  Near-contact queries in calls of 1, 63, 64, 65 and 129 (a lone lane, one short of a wave, a full wave, one lane of a
    second block, one lane of a third): the last query of each call, and every other, bitwise as in the full call."""
    cases = data[0]
    near = [k for k, (fam, _) in enumerate(cases) if fam in sc.NEAR]
    base_d, base_i = bits(*full_call)
    for j, count in enumerate((1, 63, 64, 65, 129)):
        idx = np.array(near[11 * j::5][:count])
        assert len(idx) == count
        d, i = bits(*probe(env, [cases[k][1] for k in idx]))
        assert d[-1] == base_d[idx[-1]] and i[-1] == base_i[idx[-1]], f"last of {count}"
        assert np.array_equal(d, base_d[idx]) and np.array_equal(i, base_i[idx]), f"the others of {count}"


@pytest.mark.parametrize("env_id,kind,workbench", [("UR5ObsReach-v1", _abi.ENV_OBS, False), ("UR5DynReach-v1", _abi.ENV_DYN, False),
                                                   ("UR5ObsReach-v1", _abi.ENV_OBS, True)])
def test_step_kernel_against_the_brackets(oracle, env_id, kind, workbench):
    """c.  100 envs (ragged: a wave and 36 lanes), auto-reset on, random actions.  After steps 1 and 25 every link_dist cell is held to
    the bracket formed from get_state()'s q and obstacle pose through separation_cases.numpy_fk: never below, at most SLIVER_CAP
    above.  Negative cells (penetration depths) are counted and held to the oracle's own share + 2 %.
    The link queries run with Bullet's early-out distance of getClosestPoints(distance = 5.0): urgym_hip.hip hands gjk_advance
    margin sum + 0.02 + 5.0, so the separating-axis exit (the oracle's exit 10, |v| unconverged) needs a link more than 5 m from the
    body.  The arm reaches 1 m and the obstacle stays within the workspace: exit 10 is not reachable here, and no cell is exempt
    from the upper bound."""
    n, seed = 100, 61
    scope = _abi.LINK_DIST_WORKBENCH if workbench else _abi.LINK_DIST_OBSTACLE
    env = make_vec(env_id, num_envs=n, seed=seed, link_dist_scope=scope)
    orc = oracle.OracleEnv(kind, n, threads=8, link_dist_scope=scope)
    env.reset(seed=seed)
    orc.reset(seed=seed)
    rng = np.random.default_rng(seed)
    tot = dict(cells=0, negative=0, dropped=0, excess=-np.inf)
    orc_negative = 0
    for t in range(1, 26):
        a = rng.uniform(-1, 1, (n, 6)).astype(np.float32)
        env.step(torch.from_numpy(a).cuda())
        orc.step(a)
        if t in (1, 25):
            torch.cuda.synchronize()
            c = sc.assert_cells_against_brackets(env.get_state(), workbench, f"{env_id} workbench={workbench} step {t}")
            tot = {k: max(tot[k], c[k]) if k == "excess" else tot[k] + c[k] for k in tot}
            orc_negative += int((orc.buf["link_dist"] < 0.0).sum())
    print(f"\n  c {env_id} workbench={workbench}: {tot['cells']} cells, {tot['negative']} negative (oracle {orc_negative}), {tot['dropped']} dropped, "
          f"largest d - up {tot['excess']:+.2e}")
    assert tot["cells"] == 2 * 5 * n and tot["dropped"] <= sc.DROP_SHARE * tot["cells"]
    assert tot["negative"] <= orc_negative + 0.02 * tot["cells"]
    env.close()
    orc.close()


def test_refresh_kernel_against_the_brackets(oracle):
    """d.  set_state(..., refresh=True) with the obstacle 0.1 .. 20 mm from one link of every env (placed by the reference, the gap
    confirmed from the state the refresh left); the assertions of c."""
    n = 48
    state, links, gaps = sc.refresh_near_state(n)
    env = make_vec("UR5ObsReach-v1", num_envs=n, seed=9, auto_reset=False)
    orc = oracle.OracleEnv(_abi.ENV_OBS, n, auto_reset=0)
    env.reset(seed=9)
    orc.reset(seed=9)
    orc.load_state(state)
    orc.refresh()
    env.set_state(state, refresh=True)
    torch.cuda.synchronize()
    st = env.get_state()
    sc.assert_refresh_coverage(st, links, gaps)
    c = sc.assert_cells_against_brackets(st, False, "refresh")
    orc_negative = int((orc.buf["link_dist"] < 0.0).sum())
    print(f"\n  d refresh: {c['cells']} cells, {c['negative']} negative (oracle {orc_negative}), {c['dropped']} dropped, largest d - up {c['excess']:+.2e}")
    assert c["cells"] == 5 * n and c["dropped"] <= sc.DROP_SHARE * c["cells"]
    assert c["negative"] <= orc_negative + 0.02 * c["cells"]
    # and, this close to the obstacle, on the oracle's branches (test_gpu_parity's rule: within LD_TOL, or inside the range of the
    # oracle's own answers under a 1e-14 move of the obstacle at a query the oracle itself is unstable at)
    diff = np.abs(st["link_dist"] - orc.buf["link_dist"])
    print(f"  d refresh: {int((diff > sc.LD_TOL).sum())} cells differ from the oracle by more than LD_TOL, at most {diff.max():.2e}")
    link_dist_slack(oracle, st["link_dist"], orc.buf["link_dist"], orc.buf["q"], orc.buf["obst_pos"], orc.buf["obst_quat"])
    env.close()
    orc.close()
