"""Inputs and bounds the two Adam test files share (tests/test_adam_host.py on the CPU, tests/test_adam.py on the GPU)."""
import numpy as np

STEPS = (1, 2, 3, 1000, 10 ** 6)  # 1-based step indices of the bitwise input set: three in a row, then two jumps on the carried state
HYPER = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8)  # SB3's SAC, which train.py does not change


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(words(a), words(b))


def wide_gradients(rng, shape):
    """The bitwise input set's gradients: seeded normal times a per-element scale of 2^U(-70, 10), so that g * g is subnormal or
    underflows to zero on part of them (|g| below 2^-63 squares to a subnormal, below 2^-75 to zero); a seventh are exactly 0."""
    g = (rng.standard_normal(shape) * np.exp2(rng.uniform(-70.0, 10.0, shape))).astype(np.float32)
    g.reshape(-1)[rng.integers(0, 7, g.size) == 0] = 0.0
    return g


def p_bound(t, p0_abs_max, lr):
    """|p - p64| after step t against float64 Adam on the same float32 inputs: t (1.1 * 2^-24 max|p0| + 2^-19 lr).  The first term is
    half an ulp of p per step (the one rounding of p' = p - w, |p| within 10 % of max|p0|); the second the at most 8 roundings (2^-24
    relative each, and the coefficients') on an update of at most 3.17 lr = lr (1 - b1) / sqrt(1 - b2): 8 * 3.17 * 2^-24 < 2^-19."""
    return t * (1.1 * 2.0 ** -24 * p0_abs_max + 2.0 ** -19 * lr)
