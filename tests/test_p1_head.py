"""GPU tests (-m gpu) of the head of the P1 waves of the step kernel.  With two P1 waves the one that
finishes first waits (bounded) for its sister's publication and sets its own first tickets up from the set-up cache and the link
frames; the culling pass compares squared distances with squared bounds (tests/test_p1_cull_host.py holds that predicate to the
earlier one on the CPU).  The cached values are what the lane would have re-derived, a pair kept in addition is decided by its exact
query, and the distance cells are indexed by (link, env): not one bit of anything may change.  Every case compares EVERY output and
state array after EVERY step with what the parent commit's library computed on the GPU (tests/golden/parent_outputs_p1_head.npz,
recorded by tests/golden/gen_parent_outputs_p1_head.py, which holds the cases):
  * 64 envs in one workgroup (one P1 wave: nothing waits), 65 (one env on the second P1 wave), 128 (two full P1 waves);
  * 51 and 52 envs: either side of the size from which P1 stores link frames;
  * a forced two-tier launch of one workgroup of 100 envs and one of 70;
  * an env with non-finite joints on each P1 wave (set_state): P1's verdict refuses its tickets on every path;
  * arms driven into the table, the track and themselves, so that pair bits are set by the culling pass and claimed;
  * the WORKBENCH scope;
  * 40 steps with auto-reset.
"""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("gen_parent_outputs_p1_head", os.path.join(HERE, "golden", "gen_parent_outputs_p1_head.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def parent():
    return np.load(gen.FIXTURE)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_is_the_parents(parent, name, i, steps, digest_only=False):
    got = gen.pack(steps, digest_only)
    for k in (() if digest_only else gen.FULL + ("observation_rows",)):
        want = parent[f"{name}/{i}/{k}"]
        assert got[k].shape == want.shape and got[k].dtype == want.dtype, (name, i, k)
        for t in range(len(steps)):
            assert np.array_equal(bits(got[k][t]), bits(want[t])), (name, i, k, "step", t)
    want = parent[f"{name}/{i}/digest"]
    assert got["digest"].shape == want.shape, (name, i)
    for t in range(len(steps)):
        for j, k in enumerate(gen.KEYS):
            assert np.array_equal(got["digest"][t, j], want[t, j]), (name, i, k, "step", t)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(gen.CASES))
def test_every_array_every_step_is_bitwise_the_parents(parent, name):
    case = gen.CASES[name]
    runs = gen.run_case(case)
    assert len(runs) == len(case["envs"])
    for i, steps in enumerate(runs):
        assert len(steps) == case["steps"]
        assert_is_the_parents(parent, name, i, steps, case.get("digest_only", False))


def test_the_recorded_cases_hold_what_they_are_there_for(parent):
    """Read from the parent's recording, so that a case cannot quietly stop exercising its path."""
    # the refused envs, one per P1 wave: NaN distances from the first step on, while every neighbour has finite ones
    ld = parent["dyn_nan_n128/0/link_dist"]  # [steps, 5, N]
    assert min(gen.NAN_ENVS) < 64 <= max(gen.NAN_ENVS)
    assert np.isnan(ld[0][:, list(gen.NAN_ENVS)]).all()
    assert np.isfinite(np.delete(ld[0], list(gen.NAN_ENVS), axis=1)).all()
    # contacts: collisions in many steps, on envs of both P1 waves (a pair bit was set by the culling pass, claimed and decided)
    coll = parent["dyn_contacts_n128/0/collision"].astype(bool)  # [steps, N]
    assert coll.sum() >= 40 and coll.any(axis=1).sum() >= 8
    assert coll[:, :64].any() and coll[:, 64:].any()
    # auto-reset: episodes end and start anew within the 40 steps
    sc = parent["dyn_autoreset_n100/0/step_count"]
    ep = parent["dyn_autoreset_n100/0/episode_id"]
    assert sc.shape[0] == 40 and (ep[-1] > ep[0]).sum() >= 10
    # the shapes: one digest per step and array
    for name, case in gen.CASES.items():
        assert parent[f"{name}/0/digest"].shape == (case["steps"], len(gen.KEYS), 8), name
