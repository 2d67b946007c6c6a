"""Inputs the two SAC-terms test files share (tests/test_sac_terms_host.py on the CPU, tests/test_sac_terms.py on the GPU)."""
import numpy as np

from adam_cases import p_bound, same, words  # noqa: F401  (re-exported: the bound and the bitwise comparison of the Adam tests)

# 1 row; one short of, exactly and one past a wave; the same around the workgroup's 1024 lanes (one and two rows per lane); a count that
# is no multiple of anything; the cap (64 rows per lane)
COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 4097, 65536)
POLICY_COUNTS = (1, 65, 1024, 1025, 65536)
HYPER = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8)  # SB3's SAC, which train.py does not change
TARGET_ENTROPY, GAMMA = -6.0, 0.95


def wide(rng, shape):
    """Seeded normals times 2^U(-30, 30): float64 sums of such terms are inexact, so their bits depend on the order of the additions."""
    return (rng.standard_normal(shape) * np.exp2(rng.uniform(-30.0, 30.0, shape))).astype(np.float32)


def inputs(count, seed=16):
    """Everything both calls read at `count` rows: per-row arrays by ``wide``, a quarter of the rows terminal, and a scalar state
    (log_ent_coef in [-2, 1], small moments) -- a pure function of (count, seed)."""
    rng = np.random.default_rng([seed, count])
    x = {k: wide(rng, count) for k in ("log_prob", "target", "next_log_prob", "y", "q_min")}
    x["q"], x["dqmin_da"] = wide(rng, (2, count)), wide(rng, (count, 6))
    x["terminated"] = (rng.integers(0, 4, count) == 0).astype(np.uint8)
    x["l"] = np.float32(rng.uniform(-2.0, 1.0))
    x["m"], x["v"] = np.float32(rng.standard_normal() * 1e-3), np.float32(rng.uniform(0.0, 1e-4))
    return x


def plain_ascending_sum(terms):
    """A float64 sum in plain ascending order (numpy's cumsum adds one element after another): what the ordered sum is NOT."""
    return np.cumsum(np.asarray(terms, dtype=np.float64))[-1]
