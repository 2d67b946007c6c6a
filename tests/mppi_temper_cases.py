"""Cases shared by tests/test_mppi_temper.py (GPU) and tests/test_mppi_temper_host.py (CPU): arguments for the tempered update's own
exponential, returns that take every branch of the search, and a temperature grid.  Pure numpy; everything is a
function of a seed."""
import numpy as np

from mppi_cases import actions, returns
from mppi_elite_cases import parent_returns

H = 3
SAMPLES = (2, 5, 64, 65, 1024)  # the smallest, an odd one, one wave, one wave and a lane, every lane
LAM_MIN, LAM_MAX, STEPS = 1e-3, 1e6, 32  # DeviceMPPI's defaults
LAM_FIXED = 20.0  # urgym_mppi.lam: what a parent without a finite return keeps
LOG2E = 1.4426950408889634
KINDS = ("none", "one", "equal", "special", "spread", "plain")  # the kinds of parents 0 .. 5 of every case


def exp_grid():
    """The committed grid over [-708, 0]: 2001 evenly spaced points, 2000 drawn ones (half of them within [-40, 0], where the weights
    that matter lie), float64."""
    rng = np.random.default_rng(7100)
    return np.concatenate([-np.linspace(0.0, 708.0, 2001), -rng.uniform(0.0, 708.0, 1000), -rng.uniform(0.0, 40.0, 1000)])


def exp_breakpoints():
    """0, -0.0, the last accepted argument, the first refused one, -inf, and the neighbours of both bounds."""
    low = np.float64(-708.0)
    return np.array([0.0, -0.0, low, np.nextafter(low, -np.inf), np.nextafter(low, 0.0), -np.inf, -5e-324, -2.0 ** -1022, -1e-17, -745.2, -1e300])


def exp_halfway():
    """Arguments whose product with LOG2E lies at or next to k + 1/2 for k = -1021 .. -1: rint decides between two kf there, and |r| is
    largest.  For each k the float64 nearest (k + 1/2) / LOG2E and its two neighbours on either side."""
    k = np.arange(-1021, 0, dtype=np.float64)
    x = (k + 0.5) / np.float64(LOG2E)
    out = [x]
    lo = hi = x
    for _ in range(2):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, 0.0)
        out += [lo, hi]
    x = np.concatenate(out)
    return x[x >= -708.0]


def temper_parent(kind, k, seed):
    """The K returns of one parent.
    none     no finite return: the search does not run
    one      one finite return (sample K - 1) among NaN, -inf and +inf: ess is 1 at every temperature -- T = 1 ends at lam_min, T = 2 at
             lam_max
    equal    all K the same: ess is the count at every temperature, the search ends at lam_min
    special  distinct returns with a NaN, a -inf and a +inf among them
    spread   returns 3 apart or more: at lam_min = 1e-3 every weight but the best underflows to +0.0 (x <= -3000), at lam_max = 1e6 all
             weigh nearly the same -- an interior solution for every T in (1, count)
    plain    distinct returns of an episode prefix's size: an interior solution"""
    if kind == "one":
        r = parent_returns("none", k, seed)
        r[k - 1] = -12.5
        return r
    if kind == "spread":
        rng = np.random.default_rng(7200 + 31 * k + seed)
        return -3.0 * rng.permutation(k).astype(np.float64) - rng.uniform(0.0, 1.0, k)
    return parent_returns(kind, k, seed)


def temper_returns(k):
    """float64 [6 * k]: the returns of six parents, one kind each (KINDS)."""
    return np.concatenate([temper_parent(kind, k, p) for p, kind in enumerate(KINDS)])


def temper_elites(k):
    """The M of the cases at K = k: None (every finite sample counts), and K / 8 elites (at least 2)."""
    return (None, max(2, k // 8))


def temper_targets(k, m):
    """The targets of the cases with `most` = M counted samples at the most: 1, 2, M / 2 and M -- those of them in [1, M], each once."""
    most = k if m is None else m
    return tuple(sorted({float(t) for t in (1, 2, most / 2, most) if 1 <= t <= most}))


def solve_cases():
    """(K, M or None, T) of every search case; each runs on temper_returns(K)."""
    return [(k, m, t) for k in SAMPLES for m in temper_elites(k) for t in temper_targets(k, m)]


def lam_grid():
    """The committed temperature grid: 91 temperatures over [1e-3, 1e6], ten to a decade."""
    return np.float64(10.0) ** (np.arange(-30, 61, dtype=np.float64) / 10.0)


def temper_actions(e, k, seed, h=H):
    return actions(h, e * k, 70 + seed)


def plain_returns(e, k, seed):
    return returns(e, k, 70 + seed)
