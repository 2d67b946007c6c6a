"""Cases of the normalization tests, shared by tests/test_norm_host.py (CPU) and tests/test_norm.py (GPU):
synthetic rings of C = 4 slots whose features meet the awkward cases, fold scripts, the forward-error bound of the fold with its
derivation, and the literal float64 RunningMeanStd.  No GPU, no torch."""
from fractions import Fraction

import numpy as np

from ur_gym_amd import _abi
from ur_gym_amd.evaluation import norm_fold, norm_initial_state

CAP = 4
OBS_DIM, GOAL_DIM = _abi.OBS_DIMS[_abi.ENV_ORI]  # the synthetic rings have UR5OriReach-v1's shape
# around a wave of 64, around a slab of 128 rows, around the 16 parts (2048 rows fill them once), three slabs a part
HOST_COUNTS = (1, 63, 64, 65, 127, 129, 1023, 1024, 1025, 2049, 4097)
DEVICE_COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
GAMMA = 0.95
U = Fraction(1, 2 ** 53)       # the unit roundoff of float64
ETA = Fraction(1, 2 ** 1075)   # half the smallest subnormal: the absolute error of a product or quotient that underflows


def rows(n, d, seed):
    """float32 [CAP, n, d] with, where d allows: column 0 constant (zero variance), column 1 a mean of order 1 with variance 1e-8,
    column 2 float32 subnormals of both signs, column 3 values of order 100 of both signs, column 4 all zero with some -0.0; the others
    normal with scales 0.01 .. 10."""
    rng = np.random.default_rng(9000 * seed + 17 * n + d)
    x = rng.normal(size=(CAP, n, d)) * (10.0 ** rng.integers(-2, 2, d))
    special = [np.full((CAP, n), 0.25), 1.0 + 1e-4 * rng.normal(size=(CAP, n)), rng.integers(-3000, 3000, (CAP, n)) * 1.4e-45,
               100.0 * rng.normal(size=(CAP, n)), np.where(rng.random((CAP, n)) < 0.5, -0.0, 0.0)]
    for j, col in enumerate(special[:d]):
        x[:, :, j] = col
    return np.ascontiguousarray(x, dtype=np.float32)


def rewards(n, seed):
    """float32 [CAP, n] as the tasks' rewards look: shaping values of order 1 of both signs, the -500 and +200 terminal rewards."""
    rng = np.random.default_rng(7000 * seed + n)
    r = rng.uniform(-1.0, 3.0, (CAP, n))
    kind = rng.integers(0, 8, (CAP, n))
    r = np.where(kind == 0, -500.0, r)
    r = np.where(kind == 1, 200.0, r)
    return np.ascontiguousarray(r, dtype=np.float32)


def ring(n, seed=1, obs_dim=OBS_DIM, goal_dim=GOAL_DIM):
    """The six ring arrays the fold reads, as a dict.  terminated where (env + slot) % 3 == 0, truncated where (env + 2 slot) % 4 == 0
    (any non-zero byte counts): env 0 has both on slot 0, some envs end an episode on every slot, some on none."""
    env, slot = np.meshgrid(np.arange(n), np.arange(CAP))
    u8 = lambda x: np.ascontiguousarray(x, dtype=np.uint8)  # noqa: E731
    return dict(observation=rows(n, obs_dim, seed), achieved_goal=rows(n, goal_dim, seed + 100), desired_goal=rows(n, goal_dim, seed + 200),
                reward=rewards(n, seed), terminated=u8((env + slot) % 3 == 0), truncated=u8((env + 2 * slot) % 4 == 0) * 255)


# folds as (first_slot, K): K = 1, K = 3 that wraps the ring, K = C
WHOLE = [(3, 3), (2, 1), (0, 4)]
# the same steps in pieces
SPLIT = [(3, 1), (0, 2), (2, 1), (0, 1), (1, 3)]


def restate(n, script, state=None, seed=1, gamma=GAMMA, norm_obs=True, norm_reward=True):
    r = ring(n, seed)
    state = norm_initial_state(n, OBS_DIM, GOAL_DIM) if state is None else state
    for first, K in script:
        state = norm_fold(state, r, first, K, gamma, norm_obs=norm_obs, norm_reward=norm_reward)
    return state


# ---- THE BOUND.  With u = 2^-53, every float64 operation returns its exact result times (1 + delta), |delta| <= u (plus at most ETA
# where a product or a quotient underflows; sums and differences are then exact).
#
# The sums.  A term of S1 or S2 of an observation group (each exact in float64: a float32, or the product of two) passes through at most
#     32        additions of its chain (a slab of 128 rows has four chains of 32 terms),
#     2         of the join (c0 + c1) + (c2 + c3),
#     ceil(B / 16)  of its part, B = ceil(N / 128) slabs,
#     4         levels of the fold of the 16 parts,
# so it is multiplied by at most D = 38 + ceil(ceil(N / 128) / 16) factors (1 + delta) whatever the order, and
#     |S - exact| <= gamma_D * sum |term|,   gamma_D = D u / (1 - D u)          (Higham, Accuracy and Stability, Lemma 3.1).
# The terms of the return group's S1 are the values of running_ret, which the restatement and the exact computation both take as GIVEN
# float64 inputs (they are part of the state the merge starts from).  The terms of its S2 are running_ret * running_ret IN FLOAT64, which
# is not exact: each rounds once before it is added, in the kernel, the header and the restatement alike, so against the exact squares
# that sum carries one factor more, D + 1 (bounded_sum(..., extra=1)).
#
# The merge.  Each later line is one operation on values that already carry an error; the class below carries, for every intermediate,
# its exact value v and a bound e on |computed - v|, by the standard rules
#     z = x + y :  e_z = (e_x + e_y) + u (|v_z| + e_x + e_y)
#     z = x * y :  p = |v_x| e_y + |v_y| e_x + e_x e_y;          e_z = p + u (|v_z| + p) + ETA
#     z = x / y :  p = (e_x + |v_z| e_y) / (|v_y| - e_y);        e_z = p + u (|v_z| + p) + ETA      (|v_y| > e_y)
#     z = max(x, 0) :  e_z = e_x                                  (1-Lipschitz, exact)
# in exact rational arithmetic, so the bound is a theorem about the stated order and formulas and owes nothing to what any
# implementation returns.  The state before the merge (mean, var, count) is exact input.
class Bounded:
    def __init__(self, v, e=Fraction(0)):
        self.v, self.e = Fraction(v), Fraction(e)

    @staticmethod
    def lift(x):
        return x if isinstance(x, Bounded) else Bounded(Fraction(x))

    def __add__(self, o):
        o = Bounded.lift(o)
        v, p = self.v + o.v, self.e + o.e
        return Bounded(v, p + U * (abs(v) + p))

    def __sub__(self, o):
        o = Bounded.lift(o)
        v, p = self.v - o.v, self.e + o.e
        return Bounded(v, p + U * (abs(v) + p))

    def __mul__(self, o):
        o = Bounded.lift(o)
        v = self.v * o.v
        p = abs(self.v) * o.e + abs(o.v) * self.e + self.e * o.e
        return Bounded(v, p + U * (abs(v) + p) + ETA)

    def __truediv__(self, o):
        o = Bounded.lift(o)
        assert abs(o.v) > o.e
        v = self.v / o.v
        p = (self.e + abs(v) * o.e) / (abs(o.v) - o.e)
        return Bounded(v, p + U * (abs(v) + p) + ETA)

    def relu(self):
        return Bounded(max(self.v, Fraction(0)), self.e)


def sum_depth(n):
    return 38 + -(-(-(-n // _abi.NORM_SLAB_ROWS)) // _abi.NORM_PARTS)


def bounded_sum(terms, n, extra=0):
    """The exact sum of the exact `terms` (Fractions) with the bound gamma_D sum |term| of the stated order; `extra`: roundings a term
    has been through before it is added (1 for the return group's squares)."""
    D = sum_depth(n) + extra
    gamma = D * U / (1 - D * U)
    return Bounded(sum(terms, Fraction(0)), gamma * sum((abs(t) for t in terms), Fraction(0)))


def bounded_merge(mean, var, count, s1, s2, n):
    """include/urgym.h's merge on Bounded values; mean, var, count exact floats.  Returns (mean', var') as Bounded."""
    nn = Fraction(n)
    mean, var, count = (Fraction(float(x)) for x in (mean, var, count))
    bm = s1 / nn
    bv = (s2 / nn - bm * bm).relu()
    delta = bm - mean
    tot = Bounded(count) + nn
    new_mean = Bounded(mean) + (delta * nn) / tot
    m2 = (Bounded(var) * count + bv * nn) + ((delta * delta) * count) * nn / tot
    return new_mean, m2 / tot


def literal_running_mean_std(mean, var, count, x):
    """SB3's RunningMeanStd.update in float64 as its source writes it: np.mean, np.var, update_from_moments."""
    batch_mean, batch_var, batch_count = np.mean(x, axis=0), np.var(x, axis=0), x.shape[0]
    delta = batch_mean - mean
    tot_count = count + batch_count
    new_mean = mean + delta * batch_count / tot_count
    m_a = var * count
    m_b = batch_var * batch_count
    m_2 = m_a + m_b + np.square(delta) * count * batch_count / (count + batch_count)
    new_var = m_2 / (count + batch_count)
    return new_mean, new_var, batch_count + count
