"""Inputs the two behaviour-cloning test files share (tests/test_sac_bc_host.py on the CPU, tests/test_sac_bc.py on the GPU)."""
import itertools

import numpy as np

from sac_terms_cases import inputs as terms_inputs
from sac_terms_cases import same, wide  # noqa: F401  (re-exported: the bitwise comparison and the wide-exponent normals)

# 1 row; 2 rows (the smallest count that holds a cloned and a not cloned row); one short of, exactly and one past the workgroup's 1024
# lanes; a second term in some lanes and a third in one (2049); the cap (64 rows per lane)
HOST_COUNTS = (1, 2, 1023, 1024, 1025, 2049, 65536)
# 65: a second wave with one live lane; 1025: a second term in one lane; 65536: the cap
GPU_COUNTS = (1, 65, 1024, 1025, 65536)
FLAGS = tuple(itertools.product((False, True), repeat=2))  # (scale_by_q, q_filter), all four
VARIANTS = ("plain", "nan_q_min", "nan_action", "zero_differences")
WEIGHT = 0.75


def inputs(count, variant="plain", seed=33):
    """Everything urgym_sac_policy_terms_cloned reads at `count` rows, a pure function of (count, variant, seed): the per-row arrays of
    sac_terms_cases.inputs (normals times 2^U(-30, 30), so that the float64 sums are inexact and the verdict of the Q-filter falls either
    way), actions in (-1, 1), and from 2 rows on two rows set by hand:
      row 0   q = (1, 2), q_min = 0.5     q[0] < q[1], cloned under the filter
      row 1   q = (3, 1), q_min = 1       q[1] < q[0], a tie min(q) == q_min: NOT cloned under the filter
    The variants put, in cases of their own, a NaN into q_min of one row (the last), a NaN into action_pi of one row that the filter
    clones (row 0), or differences of +0.0 (equal actions) and -0.0 (action_pi = -0.0, action_data = +0.0) into rows 0 and the last."""
    assert variant in VARIANTS, variant
    x = terms_inputs(count, seed)
    rng = np.random.default_rng([seed, count, 1])
    x = {k: x[k] for k in ("log_prob", "y", "q", "q_min", "dqmin_da")}
    x["action_pi"] = np.tanh(rng.standard_normal((count, 6)) * 1.5).astype(np.float32)
    x["action_data"] = rng.uniform(-1.0, 1.0, (count, 6)).astype(np.float32)
    x["alpha"] = np.float32(rng.uniform(0.05, 1.0))
    if count >= 2:
        x["q"][:, 0], x["q_min"][0] = (1.0, 2.0), 0.5
        x["q"][:, 1], x["q_min"][1] = (3.0, 1.0), 1.0
    if variant == "nan_q_min":
        x["q_min"][count - 1] = np.nan
    elif variant == "nan_action":
        x["action_pi"][0, 3] = np.nan
        if count < 2:
            x["q"][:, 0], x["q_min"][0] = (1.0, 2.0), 0.5  # cloned under the filter at one row too
    elif variant == "zero_differences":
        x["action_pi"][0] = x["action_data"][0]
        x["action_pi"][count - 1, :3], x["action_data"][count - 1, :3] = -0.0, 0.0
    return x


def check_inputs(x, count):
    """What the issue asks of the shared inputs at every count >= 2."""
    qd = np.minimum(x["q"][0], x["q"][1])
    with np.errstate(invalid="ignore"):
        cloned = qd > x["q_min"]
    assert cloned.any() and not cloned.all(), count
    assert (qd == x["q_min"]).any(), count
    assert (x["q"][1] < x["q"][0]).any() and (x["q"][0] < x["q"][1]).any(), count


def restate(x, count, scale_by_q, q_filter, weight=WEIGHT, **more):
    from ur_gym_amd.evaluation import policy_terms_cloned

    return policy_terms_cloned(x["alpha"], dqmin_da=x["dqmin_da"], scale=-1.0 / count, q=x["q"], y=x["y"], log_prob=x["log_prob"], q_min=x["q_min"],
                               action_pi=x["action_pi"], action_data=x["action_data"], weight=weight, bc_scale=1.0 / count, scale_by_q=scale_by_q,
                               q_filter=q_filter, **more)
