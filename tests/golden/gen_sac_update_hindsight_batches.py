"""Writes tests/golden/sac_update_hindsight_batches.npz: the three minibatches ``DeviceReplay.sample_hindsight`` gathers for the
hindsight case of tests/sac_update_cases.py (its synthetic ring, its seed and draws), as the GPU test fetches them.  Needs an MI355X:

    python tests/golden/gen_sac_update_hindsight_batches.py

The relabelled rewards come from the device's pose terms, which no host restates; the CPU tests read the batches from this file."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import sac_update_cases as cases  # noqa: E402
from test_sac_update_reference import Rig  # noqa: E402

rig, out = Rig("hindsight"), {}
for u in range(cases.UPDATES):
    b = rig.batch(rig.case["draw"] + u)
    for g in cases.GROUPS:
        out[f"{u}.{g}"], out[f"{u}.next_{g}"] = b["observations"][g], b["next_observations"][g]
    out[f"{u}.action"], out[f"{u}.reward"], out[f"{u}.terminated"], out[f"{u}.index"] = b["actions"], b["rewards"], b["terminated"], b["index"]
np.savez_compressed(cases.HINDSIGHT_FIXTURE, **out)
rig.close()
