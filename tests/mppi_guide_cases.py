"""Cases shared by tests/test_mppi_guide.py (GPU) and tests/test_mppi_guide_host.py (CPU): synthetic planner lanes for the terminal step
and action rows for the guide launch of the guided MPPI planner.  Pure numpy; everything is a function of a seed."""
import numpy as np

from mppi_cases import E, H, STEP_SAMPLES, actions, sample_means  # noqa: F401  (re-exported: the shapes of everything that steps)

GAMMAS = (1.0, 0.95)
FAIL_COSTS = (0.0, 1e4, 37.5)


def policy_samples(k):
    """P of the guide launch: none, the smallest, and every sample but the nominal."""
    return (0, 1, k - 1)


def guide_rows(h, n, seed):
    """(actions, policy_action, eps), float32 [h, n, 6] each: what a sample launch could have left, and an actor's output per horizon
    step with components at and beyond the bounds, so that the clamp acts on both sides."""
    rng = np.random.default_rng(5000 + seed)
    eps = rng.normal(0.0, 1.0, (h, n, 6)).astype(np.float32)
    policy_action = np.tanh(rng.normal(0.0, 1.5, (h, n, 6))).astype(np.float32)
    policy_action[:, ::3, 0], policy_action[:, 1::3, 1] = 1.0, -1.0
    return actions(h, n, seed), policy_action, eps


def terminal_lanes(gamma, horizon=H, repeat=1):
    """A score as mppi_score leaves it, and a value row, holding by lane: 0 a live future, 1 an ended success, 2 an ended failure, 3 a
    live future with ret = -0.0, 4 an ended success with ret = -0.0, 5 an ended failure with a NaN value, 6 an ended success with a NaN
    value, 7 a live future with a NaN value, 8 a live future whose value is exactly 0, 9 a failure at the last step, 10 a live future
    with a negative value.  `repeat` tiles the lanes.  Returns (score dict, value float32 [N], the lanes that hold a NaN value alive)."""
    g_live = np.float64(1.0)
    for _ in range(horizon):
        g_live = g_live * np.float64(gamma)

    def ended(step):
        g = np.float64(1.0)
        for _ in range(step + 1):
            g = g * np.float64(gamma)
        return g

    #        ret      g            alive success end_step          value
    rows = [(-41.25, g_live,       1,    0,      horizon - 1,       12.5),
            (163.5,  ended(0),     0,    1,      0,                 -3.0),
            (-512.0, ended(1),     0,    0,      1,                 55.0),
            (-0.0,   g_live,       1,    0,      horizon - 1,       7.0),
            (-0.0,   ended(0),     0,    1,      0,                 7.0),
            (-505.5, ended(0),     0,    0,      0,                 np.nan),
            (190.0,  ended(1),     0,    1,      1,                 np.nan),
            (-20.0,  g_live,       1,    0,      horizon - 1,       np.nan),
            (-0.0,   g_live,       1,    0,      horizon - 1,       0.0),
            (-530.0, ended(horizon - 1), 0, 0,   horizon - 1,       1.0),
            (-77.0,  g_live,       1,    0,      horizon - 1,       -250.125)]
    cols = [np.tile(np.array(c), repeat) for c in zip(*rows)]
    score = dict(ret=cols[0].astype(np.float64), g=cols[1].astype(np.float64), alive=cols[2].astype(np.uint8), success=cols[3].astype(np.uint8),
                 end_step=cols[4].astype(np.int32), collided=(1 - cols[2] - cols[3]).clip(0, 1).astype(np.uint8))
    value = cols[5].astype(np.float32)
    return score, value, np.flatnonzero(np.isnan(value) & (score["alive"] != 0))
