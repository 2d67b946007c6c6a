"""Cases shared by tests/test_mppi_collect.py (GPU) and tests/test_mppi_collect_host.py (CPU): action rows for the execute launch of the
planner-driven collection, and the bound the exploration noise is held to.  Pure numpy; everything is a function
of a seed."""
import numpy as np

from mppi_cases import E, H  # noqa: F401  (re-exported: the shapes of everything that steps)

E_WIDE = 171                      # 1026 lanes of the execute launch: four full workgroups of 256 and a tail of 2
SIGMAS = (0.0, 0.3, 25.0)         # none (a byte copy), ordinary, and one at which the clamp acts on both sides
SEED, DRAW = 0xC0FFEE1234, (1 << 32) - 1   # a key with both halves set, and the last draw the counter holds
COUNTER_POINTS = ((0, 0), (2, 7), (170, DRAW), ((1 << 31) - 1, 1 << 31))   # (p, draw) whose counters are compared word for word


def action_rows(e, seed=0):
    """action_out, float32 [e, 6]: what an update could have left -- values inside [-1, 1], components at both bounds, and a -0.0 at
    [0, 0] and [e - 1, 5]."""
    rng = np.random.default_rng(7000 + seed)
    a = np.tanh(rng.normal(0.0, 1.0, (e, 6))).astype(np.float32)
    a[::3, 1], a[1::3, 2] = 1.0, -1.0
    a[0, 0] = a[e - 1, 5] = -0.0
    return a


def poisoned(a):
    """`a` with a NaN (of a payload of its own) at [1, 3] and at the last row's first component; returns (rows, the mask of the NaNs)."""
    out = a.copy()
    nan = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    out[1, 3] = out[-1, 0] = nan
    return out, np.isnan(out)


def noise_bound():
    """The bound tests/test_mppi.py::test_sample_is_the_action_line_on_the_stated_noise holds the planner's eps to, formed as there: four
    times the largest difference between the float32 and the float64 evaluation of the restatement on that test's first case
    (seed 0xC0FFEE1234, draw 2^32 - 1, iteration 3, E = 3 parents, K = 8, H steps).  The expressions are the same Box-Muller lines."""
    from ur_gym_amd.evaluation import mppi_noise

    n = np.arange(E * 8)
    f32, f64 = (mppi_noise(0xC0FFEE1234, (1 << 32) - 1, 3, n[None, :] // 8, n[None, :] % 8, np.arange(H)[:, None], dtype=t) for t in (np.float32, np.float64))
    return 4.0 * float(np.abs(f32.astype(np.float64) - f64).max())
