"""Cases shared by tests/test_per_host.py (CPU) and tests/test_per.py (GPU): leaves, words and hand-built trees for the prioritized
replay."""
import numpy as np

SEED, DRAW = 0x1234_5678_9ABC_DEF0, 0x1_0000_0007

# (name, leaves, fan-out): fan-out 4 with ragged last blocks at several levels and at least four levels; fan-out 256 with one, two and
# three levels
TREES = [("f4_ragged", 1 + 4 + 16 + 64 + 256 + 3, 4), ("f4_one_block", 3, 4), ("f4_exact", 256, 4), ("f4_five", 1031, 4),
         ("f256_one", 200, 256), ("f256_two", 600, 256), ("f256_three", 70000, 256)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def leaves(n, seed=0, zeros=0.3):
    """float32 [n]: priorities over eight orders of magnitude, a share of them 0 (never drawn), whole runs of zeros included."""
    rng = np.random.default_rng(1000 + seed)
    v = np.exp(rng.uniform(-9.0, 9.0, n)).astype(np.float32)
    v[rng.random(n) < zeros] = 0
    if n > 40:
        v[n // 3:n // 3 + 17] = 0  # more than a fan-out-4 block of zeros
    if not v.any():
        v[0] = 1
    return v


def levels_of(n, fanout):
    """The entry counts of the sum levels, level 1 first, from the rule alone."""
    out = []
    while True:
        n = -(-n // fanout)
        out.append(n)
        if n <= fanout:
            return out


def terms_inputs(count, seed=0):
    """q [2, count], y [count] float32 with errors from 1e-4 to 1e2, and leaves in (0, 30]."""
    rng = np.random.default_rng(2000 + seed)
    y = rng.normal(0, 50, count).astype(np.float32)
    e = (np.exp(rng.uniform(-9, 5, (2, count))) * rng.choice([-1.0, 1.0], (2, count))).astype(np.float32)
    return dict(q=(y[None, :] + e).astype(np.float32), y=y, leaf=np.exp(rng.uniform(-6, 3.4, count)).astype(np.float32))


def ulp_error(got, exact):
    """|got - exact| in units of the float32 spacing at `exact` (float64), per element."""
    exact = np.asarray(exact, np.float64)
    spacing = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - exact) / spacing
