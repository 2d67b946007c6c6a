"""GPU tests (-m gpu) of the deferred filing of finished GJK searches in the step kernel: a lane whose
search ends only notes how it ended; gjk_finish, the distance / verdict, the status bits and EPA marks are filed when the lane next
draws, or behind the drain loop.  Filing later may not change one bit of anything, so every case compares EVERY output and state
array after EVERY step with what the parent commit's library computed on the GPU: tests/golden/parent_outputs_filing.npz, recorded
by tests/golden/gen_parent_outputs_filing.py, which also holds the cases and says what of a run the fixture keeps (the link distances,
rewards, flags and counters in full, a row subset of the observations, and a digest of every array).

The cases are the smallest shapes at which filing can go wrong (one workgroup of 256 lanes each, 5 tickets per env):
  * no lane ever draws (8 and 51 envs): everything is filed behind the drain loop;
  * a few tickets are drawn late (52, 53 envs) by waves that stay below the 16 idle lanes a draw waits for until the pool is dry:
    finished lanes wait unfiled for many trips;
  * lanes file, draw and file again (64 and 128 envs, 40 steps with auto-reset: finished envs, refill workgroups);
  * boolean pair queries file the collision bit (UR5OriReach-v1: nothing but pair bits; UR5DynReach-v1: pair bits behind tickets);
  * the WORKBENCH link-distance scope files with atomicMin;
  * UR5ObsReach-v1 without collision checks consumes penetration depths: the EPA mark of an overlapping query is raised, served,
    and the depth is the parent's;
  * the RESET kernel after each step (URGYM_PREFETCH=0) against the prefetched records, bitwise, at 64 envs: both share the loop.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("gen_parent_outputs_filing", os.path.join(HERE, "golden", "gen_parent_outputs_filing.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def parent():
    return np.load(gen.FIXTURE)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_is_the_parents(parent, name, steps):
    got = gen.pack(steps)
    for k in gen.FULL + ("observation_rows",):
        want = parent[f"{name}/{k}"]
        assert got[k].shape == want.shape and got[k].dtype == want.dtype, (name, k)
        for t in range(len(steps)):
            assert np.array_equal(bits(got[k][t]), bits(want[t])), (name, k, "step", t)
    want = parent[f"{name}/digest"]
    for t in range(len(steps)):
        for i, k in enumerate(gen.KEYS):
            assert np.array_equal(got["digest"][t, i], want[t, i]), (name, k, "step", t)


@pytest.mark.parametrize("name", list(gen.CASES))
def test_every_array_every_step_is_bitwise_the_parents(parent, name):
    case = gen.CASES[name]
    steps = gen.run_case(case)
    assert len(steps) == case["steps"]
    assert_is_the_parents(parent, name, steps)


def test_the_recorded_cases_hold_what_they_are_there_for(parent):
    """Read from the parent's recording, so that a case cannot quietly stop exercising its path: envs finish in the 40-step cases,
    pair queries decide collisions (UR5OriReach-v1 has no other source of one; UR5DynReach-v1: a collision with every link farther
    from the obstacle than the margin), and the collision-free Obs case holds depths beyond the margin sum (the criterion of
    test_obs_terminal_collision_reward_uses_penetration_depth) with the penetration status bit."""
    from ur_gym_amd import _abi

    for name in ("dyn_n64", "dyn_n128"):
        done = parent[f"{name}/terminated"].astype(bool) | parent[f"{name}/truncated"].astype(bool)
        assert done.any(axis=1).sum() >= 3, name  # envs finish in several steps: refill workgroups ride in later launches
    assert parent["ori_pairs/collision"].astype(bool).sum() >= 3
    # (dyn_pairs runs without auto-reset, so the link distances of a step that ended in a collision are still those of that step)
    by_pair = parent["dyn_pairs/collision"].astype(bool) & (parent["dyn_pairs/link_dist"].min(axis=1) > 0.01)
    assert by_pair.sum() >= 3
    ld, status = parent["obs_free_n32/link_dist"], parent["obs_free_n32/status"]
    deep = (ld < -0.002 - 1e-9).any(axis=1)  # [steps, N]
    assert deep.sum() >= 5
    assert (status[deep] & _abi.STATUS_PENETRATION).all()
    assert not parent["obs_free_n32/collision"].any()


def test_reset_kernel_and_prefetched_records_file_alike(parent):
    """64 envs, 40 steps: URGYM_PREFETCH=0 (a RESET kernel after each step) leaves the bits of the default path (PREFETCH workgroups in
    the step's launch, inline reset), which are the parent's."""
    case = gen.CASES["dyn_n64"]
    steps = gen.run_case(case, URGYM_PREFETCH="0")
    assert_is_the_parents(parent, "dyn_n64", steps)
