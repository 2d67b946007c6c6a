"""Cases shared by tests/test_mppi_elite.py (GPU) and tests/test_mppi_elite_host.py (CPU): returns for the rank (exact ties, signed
zeros, returns that are not finite), weights and actions for the elite update and its std.  Pure numpy; everything
is a function of a seed."""
import numpy as np

from mppi_cases import actions, returns

H = 3
RANK_SAMPLES = (2, 3, 64, 65, 1000, 1024)  # the smallest, an odd one, one wave, one wave and a lane, a ragged last wave, every lane
LAM = 40.0


def elite_counts(k):
    """The M of the rank cases for K = k: 1, 2, K / 8 (at least 1), K - 1, K -- those of them that lie in [1, K], each once."""
    return tuple(sorted({m for m in (1, 2, max(1, k // 8), k - 1, k) if 1 <= m <= k}))


def parent_returns(kind, k, seed):
    """The K returns of one parent.
    ties     seven levels, so almost every return has an exact twin; the zeros among them alternate -0.0 and 0.0
    special  distinct returns with a NaN, a -inf and a +inf among them (positions 1, K / 2 and K - 1; a later one replaces an earlier)
    equal    all K the same
    zeros    all K zero, alternating -0.0 and 0.0: equal keys with different bits
    none     no finite return: NaN, -inf, +inf in turn
    plain    distinct returns"""
    rng = np.random.default_rng(5000 + 31 * k + seed)
    if kind == "ties":
        r = rng.integers(-3, 4, k).astype(np.float64) * 12.5
        r[-1] = r[0]  # a tie at every K
        zero = np.nonzero(r == 0)[0]
        r[zero[0::2]] = -0.0
        return r
    if kind == "special":
        r = returns(1, k, seed)
        r[1 % k], r[k // 2], r[k - 1] = np.nan, -np.inf, np.inf
        return r
    if kind == "equal":
        return np.full(k, -37.25)
    if kind == "zeros":
        r = np.zeros(k)
        r[0::2] = -0.0
        return r
    if kind == "none":
        return np.resize(np.array([np.nan, -np.inf, np.inf]), k).astype(np.float64)
    assert kind == "plain", kind
    return returns(1, k, seed)


LAYOUTS = (("ties", "special", "plain"), ("equal", "none", "zeros"))  # the kinds of parents 0, 1, 2


def rank_returns(k, layout):
    """float64 [3 * k]: the returns of three parents, one kind each."""
    return np.concatenate([parent_returns(kind, k, p) for p, kind in enumerate(LAYOUTS[layout])])


def rank_cases():
    """(K, layout, M) of every rank case."""
    return [(k, layout, m) for k in RANK_SAMPLES for layout in range(len(LAYOUTS)) for m in elite_counts(k)]


def elite_actions(h, e, k, seed, nan_at=None):
    """Actions [h, e * k, 6] float32 in [-1, 1]; `nan_at` = (step, env, component) makes that one a NaN."""
    a = actions(h, e * k, seed)
    if nan_at is not None:
        a[nan_at] = np.nan
    return a


def update_cases():
    """name -> dict(ret, actions, lam, E, K, M, H, shift, std_min, std_max, expect).  `expect` names what the CPU test asserts about the
    case beyond the bits: "both clamps" (some element of new_std at std_min, some at std_max), "floor" (a NaN variance ends at std_min)."""
    out = {}
    e = 3
    for k in (2, 5, 64, 65, 1024):
        for shift in (0, 1):
            for m in sorted({max(1, k // 8), k}):
                out[f"K={k} M={m} shift={shift}"] = dict(ret=rank_returns(k, 0), actions=elite_actions(H, e, k, k + m), lam=LAM, E=e, K=k, M=m, H=H, shift=shift,
                                                         std_min=0.05, std_max=0.6, expect=None)
    k = 64
    # three elites: the spread of three actions drawn over [-1, 1] falls below 0.25, above 0.5 and between them, each for some (h, p, c)
    out["both clamps"] = dict(ret=rank_returns(k, 0), actions=elite_actions(H, e, k, 21), lam=LAM, E=e, K=k, M=3, H=H, shift=1, std_min=0.25, std_max=0.5,
                              expect="both clamps")
    out["one elite"] = dict(ret=rank_returns(k, 0), actions=elite_actions(H, e, k, 22), lam=LAM, E=e, K=k, M=1, H=H, shift=0, std_min=0.125, std_max=0.5,
                            expect="floor everywhere")
    # a NaN action of the worst sample of parent 2 (rank K - 1, no elite at M = 8): 0 * NaN reaches the mean and the variance of (1, 2, 3)
    r = rank_returns(k, 0)
    worst = 2 * k + int(np.argmin(r[2 * k:]))
    out["NaN action"] = dict(ret=r, actions=elite_actions(H, e, k, 23, nan_at=(1, worst, 3)), lam=LAM, E=e, K=k, M=8, H=H, shift=0, std_min=0.0625, std_max=0.75,
                             expect="floor")
    out["no finite return"] = dict(ret=rank_returns(k, 1), actions=elite_actions(H, e, k, 24), lam=LAM, E=e, K=k, M=8, H=H, shift=1, std_min=0.0, std_max=1.0,
                                   expect=None)
    out["H=1"] = dict(ret=rank_returns(5, 0), actions=elite_actions(1, e, 5, 25), lam=LAM, E=e, K=5, M=2, H=1, shift=1, std_min=0.05, std_max=0.6, expect=None)
    return out


def random_std(h, e, seed, lo=0.0, hi=1.5):
    """A per-(step, parent, joint) width [h, e, 6] float32 with a zero and a value that drives the clamp among them."""
    rng = np.random.default_rng(6000 + seed)
    s = rng.uniform(lo, hi, (h, e, 6)).astype(np.float32)
    s[0, 0, 0], s[-1, -1, -1] = 0.0, 25.0
    return s
