"""Inputs the two advantage-weighted cloning test files share (tests/test_sac_bc_weighted_host.py on the CPU, tests/test_sac_bc_weighted.py on
the GPU)."""
import itertools

import numpy as np

from sac_terms_cases import same, wide  # noqa: F401  (re-exported: the bitwise comparison)

# 1 row; 2 rows; one short of, exactly and one past the workgroup's 1024 lanes; a second term in some lanes and a third in one (2049);
# the cap (64 rows per lane)
HOST_COUNTS = (1, 2, 1023, 1024, 1025, 2049, 65536)
# one row, a ragged wave, exactly one trip per lane, the first wrap, the cap
GPU_COUNTS = (1, 65, 1024, 1025, 65536)
FLT_MAX = float(np.finfo(np.float32).max)
# the three regimes of e = exp((A - A_max) / T) on advantages spread over a few units: most arguments below the -708 cut (e = +0.0),
# order one, and every e equal to 1
TEMPERATURES = (2e-3, 1.0, FLT_MAX)
CAPS = (float("inf"), 2.0)
MASKS = (False, True)
VARIANTS = ("plain", "nan_q", "inf_advantage", "zero_mask", "one_eligible", "tie", "nan_action", "nan_action_ineligible")
WEIGHT = 0.75
FORMS = tuple(itertools.product(MASKS, CAPS, TEMPERATURES))


def inputs(count, variant="plain", seed=35):
    """Everything urgym_sac_policy_terms_weighted reads at `count` rows, a pure function of (count, variant, seed): critics and targets of
    ordinary magnitude (so that the advantages spread over a few units and all three temperature regimes occur), log_prob and dqmin_da
    by ``wide`` (normals times 2^U(-30, 30): inexact float64 sums), actions in (-1, 1), and a mask that marks about half of the rows,
    row 0 among them.  The variants, in cases of their own:
      nan_q                  q[0] of the last row is a NaN: the row is not eligible (and the critic loss is a NaN, as in every call)
      inf_advantage          q_min of row 0 is -inf: A = +inf, the row is not eligible
      zero_mask              the mask marks no row: n == 0 with the mask
      one_eligible           the mask marks row 0 alone: n == 1 with the mask
      tie                    the last row holds row 0's q and q_min, and they are the largest advantage: two rows with e = 1
      nan_action             a NaN in action_pi of row 0, which is eligible
      nan_action_ineligible  a NaN in action_pi and action_data of the last row, whose q_min is a NaN: not eligible"""
    assert variant in VARIANTS, variant
    rng = np.random.default_rng([seed, count])
    f = np.float32
    x = dict(log_prob=wide(rng, count), dqmin_da=wide(rng, (count, 6)), y=rng.normal(-5.0, 3.0, count).astype(f), q=rng.normal(-5.0, 3.0, (2, count)).astype(f),
             q_min=rng.normal(-5.0, 3.0, count).astype(f))
    x["action_pi"] = np.tanh(rng.standard_normal((count, 6)) * 1.5).astype(f)
    x["action_data"] = rng.uniform(-1.0, 1.0, (count, 6)).astype(f)
    x["alpha"] = f(rng.uniform(0.05, 1.0))
    mask = (rng.random(count) < 0.5).astype(np.uint8)
    mask[0] = 1
    last = count - 1
    if variant == "nan_q":
        x["q"][0, last] = np.nan
    elif variant == "inf_advantage":
        x["q_min"][0] = -np.inf
    elif variant == "zero_mask":
        mask[:] = 0
    elif variant == "one_eligible":
        mask[:] = 0
        mask[0] = 1
    elif variant == "tie":
        x["q"][:, 0], x["q_min"][0] = (40.0, 41.0), -2.0
        x["q"][:, last], x["q_min"][last] = x["q"][:, 0], x["q_min"][0]
        mask[last] = 1
    elif variant == "nan_action":
        x["action_pi"][0, 3] = np.nan
    elif variant == "nan_action_ineligible":
        x["q_min"][last] = np.nan
        x["action_pi"][last, 2] = x["action_data"][last, 4] = np.nan
    x["mask"] = mask
    return x


def restate(x, count, masked, max_weight, temperature, weight=WEIGHT, scale_by_q=False):
    from ur_gym_amd.evaluation import policy_terms_weighted

    return policy_terms_weighted(x["alpha"], dqmin_da=x["dqmin_da"], scale=-1.0 / count, q=x["q"], y=x["y"], log_prob=x["log_prob"], q_min=x["q_min"],
                                 action_pi=x["action_pi"], action_data=x["action_data"], weight=weight, bc_scale=1.0 / count, temperature=temperature,
                                 max_weight=max_weight, scale_by_q=scale_by_q, row_mask=x["mask"] if masked else None)


def restate_cloned(x, count, masked, weight=WEIGHT, scale_by_q=False):
    from ur_gym_amd.evaluation import policy_terms_cloned

    return policy_terms_cloned(x["alpha"], dqmin_da=x["dqmin_da"], scale=-1.0 / count, q=x["q"], y=x["y"], log_prob=x["log_prob"], q_min=x["q_min"],
                               action_pi=x["action_pi"], action_data=x["action_data"], weight=weight, bc_scale=1.0 / count, scale_by_q=scale_by_q, q_filter=False,
                               **(dict(row_mask=x["mask"]) if masked else {}))
