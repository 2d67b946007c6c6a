"""The cases the CPU and the GPU tests of the temporally correlated sampling noise share: nothing here needs a
device, and nothing here is random beyond a seeded generator."""
import numpy as np

BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))  # the largest float32 below 1: scale is small and not zero
BETAS = (0.0, 0.5, 0.9, BELOW_ONE, 1.0)  # the host harness against numpy
HORIZONS = (1, 2, 3, 64)
WIDTH = 7 * 6  # seven samples of six joints; sample 0 is the nominal one

DEVICE_BETAS = (0.0, 0.5, 0.9, 1.0)  # the single launch
DEVICE_SIGMAS = (0.3, 25.0, 0.0)  # 25: the clamp of the action line acts on nearly every element

# the distribution check: the restatement over mppi_noise
STAT_SEED, STAT_DRAW, STAT_ITERATION = 0xC0FFEE1234, 7, 0
STAT_E, STAT_K, STAT_H = 8, 256, 32
STAT_BETAS = (0.0, 0.5, 0.9)
STAT_BOUND = 0.06
STAT_COUNT = STAT_E * (STAT_K - 1) * 6  # the non-nominal values of a step


def random_xi(h, seed=0):
    """float32 [h, WIDTH]: standard normals, a few exact zeros of either sign and large values among them, sample 0 all +0.0."""
    rng = np.random.default_rng(1000 + 17 * h + seed)
    xi = rng.standard_normal((h, WIDTH)).astype(np.float32)
    xi[:, 6:12:5] *= np.float32(40.0)
    xi[h // 2, 13] = np.float32(-0.0)
    xi[0, 14] = np.float32(-0.0)
    xi[:, :6] = 0
    return xi


def env_grid(e, k, h):
    """(parents, samples, steps) index arrays that broadcast to [h, e * k] for ``mppi_noise``."""
    n = np.arange(e * k)
    return (n // k)[None, :], (n % k)[None, :], np.arange(h)[:, None]


def pattern_mean(h, e, seed=3):
    """float32 [h, e, 6] in (-0.9, 0.9): a nominal sequence that is not zero."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.9, 0.9, size=(h, e, 6)).astype(np.float32)


def pattern_std(h, e, seed=4):
    """float32 [h, e, 6] in (0.05, 0.6): one width per element, none equal to another."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.05, 0.6, size=(h, e, 6)).astype(np.float32)
