"""GPU tests (-m gpu) of the step kernel's collision verdict at the contact margin against the certified rule of
tests/verdict_cases.py: the committed poses of tests/golden/verdict_poses.npz (one check_collision pair at a signed gap of 1e-6 .. 3e-3
from the 0.01 m margin, the other 23 certified free; a family in which the culling pass's capsule bound is least conservative) are
loaded with set_state and stepped once with a zero action, auto-reset off and the obstacle at rest, as test_collision_verdict_census
does.

  collision   certainly free, certainly colliding, or -- in the band between -- the oracle's verdict (test_gpu_parity's 2e-5 rule)
  link_dist   of obstacle poses: separation_cases.assert_cells_against_brackets, as in tests/test_separation.py
  terminated, reward   take the collision branch exactly where collision is set: the oracle's step on the same state
  bitwise     the same verdicts when the call is permuted, and in calls of 1, 63, 64, 65 and 129 poses
Every kind runs in the default launch geometry and once more as one workgroup of 99 envs (URGYM_STEP_ENVS=99) on a slice that holds
every pair.  Run with -s for the tables (profiles/r11/gpu_tests_verdicts.txt).
"""
import numpy as np
import pytest
import torch

import separation_cases as sc
import verdict_cases as vc
from test_gpu_parity import KINDS, REWARD_TOL, make_vec, np_
from ur_gym_amd import _abi

pytestmark = pytest.mark.gpu

OUT = ("collision", "terminated", "is_success", "reward")


@pytest.fixture(scope="module")
def fx():
    return vc.load_fixture()


def slice_of_99(fx):
    """99 poses that hold every pair of the fixture on both sides of the margin: per pair the first pose at -3e-4, -1e-6, +1e-6 and
    +1e-3, then the tight family, then further band poses."""
    idx = []
    for p in sorted(set(fx["pair"])):
        for g in (-3e-4, -1e-6, 1e-6, 1e-3):
            idx.append(int(np.nonzero((fx["pair"] == p) & (fx["gap"] == g) & (fx["family"] == vc.FAMILY_DIRECTED))[0][0]))
    rest = [int(i) for i in np.nonzero(fx["family"] == vc.FAMILY_TIGHT)[0]] + [int(i) for i in np.nonzero(np.abs(fx["gap"]) == 1e-5)[0]]
    idx += [i for i in rest if i not in idx][: 99 - len(idx)]
    assert len(idx) == 99 and set(fx["pair"][idx]) == set(fx["pair"])
    return np.array(idx)


def step_once(env, fx, idx, has_obstacle):
    """set_state + one zero-action step: the outputs on the host, and the state after the step."""
    env.set_state(vc.state_of(fx, idx, has_obstacle))
    env.step(torch.zeros((len(idx), 6), dtype=torch.float32, device="cuda:0"))
    torch.cuda.synchronize()
    return {k: np_(env.buf[k]).copy() for k in OUT}, env.get_state()


def oracle_step(oracle, kind, fx, idx, has_obstacle, seed):
    orc = oracle.OracleEnv(kind, len(idx), threads=8, auto_reset=0)
    orc.reset(seed=seed)
    orc.load_state(vc.state_of(fx, idx, has_obstacle))
    orc.step(np.zeros((len(idx), 6), np.float32))
    out = {k: orc.buf[k].copy() for k in OUT + ("link_dist", "q", "obst_pos", "obst_quat")}
    cfg = orc.cfg
    out["w_collision"], out["w_link"] = float(cfg.w_collision), float(max(cfg.w_link))
    orc.close()
    return out


def check_call(oracle, kind, fx, idx, got, state, ref, what):
    """The assertions of one call; returns the table of vc.assert_verdicts."""
    has_obstacle = kind != _abi.ENV_ORI
    coll, want = got["collision"].astype(bool), ref["collision"].astype(bool)
    table = vc.assert_verdicts(oracle, coll, want, fx, idx, has_obstacle, what)
    # terminated and the reward follow the verdict: the oracle's step on the same state
    assert np.array_equal(got["terminated"].astype(bool), coll | got["is_success"].astype(bool)), what
    assert np.array_equal(got["is_success"][coll == want], ref["is_success"][coll == want]), what
    slack = np.zeros(len(idx))
    if has_obstacle:
        # the reward carries w_link * (link distance - last) per near link: what the two sides' link distances differ by is allowed on
        # top (the distances themselves are held to the certified brackets below and in tests/test_separation.py).  On a collision
        # ReachDyn.compute_reward returns before the link distances: where the verdicts differ the cells are not comparable.
        diff = np.abs(state["link_dist"] - ref["link_dist"])
        diff[:, coll != want] = 0.0
        slack = ref["w_link"] * diff.sum(0)
    rd = np.abs(got["reward"].astype(np.float64) - ref["reward"])
    same = coll == want
    assert (rd[same] < REWARD_TOL + slack[same]).all(), (what, "reward", int(np.argmax(np.where(same, rd - slack, -1))), rd.max())
    for j in np.nonzero(~same)[0]:  # (a band pose on which the 2e-5 rule let the verdicts differ: the reward differs by the collision branch)
        if kind in (_abi.ENV_ORI, _abi.ENV_OBS):
            assert abs(rd[j] - abs(ref["w_collision"])) < REWARD_TOL + slack[j], (what, "reward without the collision term", j)
        elif coll[j]:
            assert got["reward"][j] == np.float32(ref["w_collision"]), (what, "reward of the collision branch", j)
    if kind in (_abi.ENV_DYN, _abi.ENV_STA):
        assert (got["reward"][coll] == np.float32(ref["w_collision"])).all(), what  # ReachDyn.compute_reward returns at the collision
    return table, float(np.abs(state["link_dist"] - ref["link_dist"])[:, coll == want].max()) if has_obstacle else 0.0


def cells_of_obstacle_poses(kind, fx, idx, got, state, what):
    """link_dist of every third obstacle pose against the brackets of separation_cases.link_brackets.  (ReachDyn.compute_reward
    returns before the link distances on a collision: those cells keep what set_state put there and are left out.)"""
    pick = [j for j, i in enumerate(idx) if fx["pair"][i] < vc.N_OBST][::3]
    if kind in (_abi.ENV_DYN, _abi.ENV_STA):
        pick = [j for j in pick if not got["collision"][j]]
    sub = {k: state[k][:, pick] for k in ("q", "obst_pos", "obst_quat", "link_dist")}
    c = sc.assert_cells_against_brackets(sub, False, what)
    assert c["dropped"] <= sc.DROP_SHARE * c["cells"] and c["negative"] == 0, (what, c)
    return c


@pytest.mark.parametrize("step_envs", [None, 99])
@pytest.mark.parametrize("env_id,kind", KINDS)
def test_verdicts_at_the_margin(oracle, monkeypatch, fx, env_id, kind, step_envs):
    has_obstacle = kind != _abi.ENV_ORI
    if step_envs:
        monkeypatch.setenv("URGYM_STEP_ENVS", str(step_envs))  # one workgroup: the frames path is on, the pair bits are drawn after the tickets
    idx = slice_of_99(fx) if step_envs else np.arange(len(fx["pair"]))
    what = f"{env_id} step_envs={step_envs}"
    env = make_vec(env_id, num_envs=len(idx), seed=11, auto_reset=False)
    env.reset(seed=11)
    got, state = step_once(env, fx, idx, has_obstacle)
    assert np.abs(state["q"] - fx["q"][idx].T).max() == 0.0, "a zero action leaves the joints where set_state put them"
    ref = oracle_step(oracle, kind, fx, idx, has_obstacle, 11)
    table, ld_diff = check_call(oracle, kind, fx, idx, got, state, ref, what)
    exp = vc.expected(fx, has_obstacle)[idx]
    print("\n" + "\n".join(vc.table_lines(table, what)))
    band = exp == "band"
    print(f"  {what}: {len(idx)} poses, {int((exp == 'free').sum())} certainly free, {int((exp == 'colliding').sum())} certainly colliding, {int(band.sum())} in the band: "
          f"{int((got['collision'][band] == ref['collision'][band]).sum())} the oracle's verdict, {int((got['collision'][band] != ref['collision'][band]).sum())} excused by the 2e-5 rule; "
          f"{int(got['collision'].sum())} reported colliding (oracle {int(ref['collision'].sum())})")
    if has_obstacle:
        c = cells_of_obstacle_poses(kind, fx, idx, got, state, what)
        print(f"  {what}: link_dist of obstacle poses: {c['cells']} cells, {c['dropped']} dropped, largest d - up {c['excess']:+.2e}; "
              f"largest |link_dist - oracle| over all poses {ld_diff:.2e}")
    # the same call permuted: every output of every pose bitwise the same
    perm = np.random.default_rng(12).permutation(len(idx))
    again, _ = step_once(env, fx, idx[perm], has_obstacle)
    for k in OUT:
        assert np.array_equal(again[k].view(np.uint8), got[k][perm].view(np.uint8)), (what, "permuted call", k)
    env.close()


@pytest.mark.parametrize("env_id,kind", [KINDS[0], KINDS[2]])
def test_verdicts_do_not_depend_on_the_call_size(oracle, fx, env_id, kind):
    """Calls of 1, 63, 64, 65 and 129 poses (a lone lane, one short of a wave, a full wave, one lane more, two waves and one): the
    last pose of each call, and every other, has the outputs of the call that held them all."""
    has_obstacle = kind != _abi.ENV_ORI
    near = np.nonzero(np.abs(fx["gap"]) <= 1e-4)[0]  # the poses on which a verdict could move
    env = make_vec(env_id, num_envs=len(near), seed=13, auto_reset=False)
    env.reset(seed=13)
    base, _ = step_once(env, fx, near, has_obstacle)
    env.close()
    at = {int(i): j for j, i in enumerate(near)}
    for j, count in enumerate((1, 63, 64, 65, 129)):
        idx = near[7 * j::3][:count]
        assert len(idx) == count
        env = make_vec(env_id, num_envs=count, seed=13, auto_reset=False)
        env.reset(seed=13)
        got, _ = step_once(env, fx, idx, has_obstacle)
        env.close()
        rows = [at[int(i)] for i in idx]
        for k in OUT:
            assert np.array_equal(got[k].view(np.uint8), base[k][rows].view(np.uint8)), (env_id, "call of", count, k)
