"""Cases shared by tests/test_mppi.py (GPU) and tests/test_mppi_host.py (CPU): synthetic returns, weights, actions and step outcomes
for the MPPI planner's update, score and sample arithmetic.  Pure numpy; everything is a function of a seed."""
import numpy as np

E, H = 3, 3          # ragged parent count, the shortest horizon with a first, a middle and a last step
STEP_SAMPLES = (5, 8)            # K of everything that steps
UPDATE_SAMPLES = (2, 5, 64, 1024)  # K of the update alone: the smallest, an odd one, one wave, every lane


def sample_means(h=H, e=E, seed=0):
    """A nominal sequence [h, e, 6] float32 inside (-1, 1), with parent 1 pinned at the bounds (the clamp must act there)."""
    rng = np.random.default_rng(1000 + seed)
    mean = rng.uniform(-0.9, 0.9, (h, e, 6)).astype(np.float32)
    if e > 1:
        mean[:, 1, 0::2], mean[:, 1, 1::2] = 1.0, -1.0
    return mean


def returns(e, k, seed):
    """Returns of the magnitude an episode prefix has: mixed signs, a few hundred in size, distinct."""
    rng = np.random.default_rng(2000 + 7 * e + k + seed)
    return (rng.normal(-150.0, 120.0, e * k)).astype(np.float64)


def actions(h, n, seed):
    rng = np.random.default_rng(3000 + seed)
    return np.clip(rng.normal(0.0, 0.7, (h, n, 6)), -1, 1).astype(np.float32)


def update_cases():
    """name -> dict(ret, actions, lam, E, K, H, shift, and what the case expects under `expect`)."""
    out = {}
    for k in UPDATE_SAMPLES:
        for shift in (0, 1):
            out[f"plain K={k} shift={shift}"] = dict(ret=returns(E, k, shift), actions=actions(H, E * k, k), lam=40.0, E=E, K=k, H=H, shift=shift, expect=None)
    k = 5
    out["all returns equal"] = dict(ret=np.full(E * k, -37.25), actions=actions(H, E * k, 11), lam=3.0, E=E, K=k, H=H, shift=0, expect="uniform")
    r = returns(E, 64, 5)
    out["lambda so small that every other weight underflows"] = dict(ret=r, actions=actions(H, E * 64, 12), lam=1e-6, E=E, K=64, H=H, shift=1, expect="best")
    r = returns(E, k, 6)
    r[1], r[k + 2], r[2 * k] = np.nan, -np.inf, np.inf  # sample 1 of parent 0, sample 2 of parent 1, the NOMINAL of parent 2
    out["one NaN, one -inf, one +inf"] = dict(ret=r, actions=actions(H, E * k, 13), lam=25.0, E=E, K=k, H=H, shift=0, expect="zero weight")
    r = returns(E, k, 7)
    r[:k], r[k:2 * k] = np.nan, -np.inf  # parents 0 and 1 have no finite return; parent 2 is ordinary
    out["all non-finite"] = dict(ret=r, actions=actions(H, E * k, 14), lam=25.0, E=E, K=k, H=H, shift=1, expect="nominal")
    for shift in (0, 1):
        out[f"H=1 shift={shift}"] = dict(ret=returns(E, k, 8), actions=actions(1, E * k, 15), lam=60.0, E=E, K=k, H=1, shift=shift, expect=None)
    return out


def outcomes(h, n, seed):
    """What h planner steps of n envs returned, synthetic: rewards of mixed sign and size, an env that terminates at every step index,
    one that is truncated, one with both flags, one with a NaN reward, most that run through."""
    rng = np.random.default_rng(4000 + seed)
    reward = rng.normal(-30.0, 40.0, (h, n)).astype(np.float32)
    term, trunc = np.zeros((h, n), np.uint8), np.zeros((h, n), np.uint8)
    for step in range(h):
        term[step:, step % n] = 1  # stays set afterwards, as a finished env that is not reset reports it
    if n > h:
        trunc[min(1, h - 1), h] = 1
    if n > h + 1:
        term[h - 1, h + 1] = trunc[h - 1, h + 1] = 1
    if n > h + 2:
        reward[0, h + 2] = np.nan
    succ = (rng.random((h, n)) < 0.5).astype(np.uint8)
    coll = (rng.random((h, n)) < 0.5).astype(np.uint8)
    return reward, term, trunc, succ, coll
