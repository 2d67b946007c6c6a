"""Shared cases of the hindsight experience replay tests (test_her_host.py on the CPU, test_her.py on the GPU): synthetic rings, the
ring states, the case list, the independent per-row reference and the census of what the drawn rows cover.  No GPU, no native library.

A synthetic ring is [C = 12][N][...] with N = 1, 5 or 257 and the row widths of one of the four env kinds.  Every entry is made by a
forward model of the step kernel's reward, so that what the ring stores is consistent with the re-scoring rule: a goal, an achieved
pose that lies within the success thresholds of it with probability 0.15 and far from it otherwise, a collision with probability
0.08, `terminated = success | collision`, `is_success = terminated & !collision`, the env kind's reward with a random shaping term
(none for Ori), `truncated` with probability 0.12, independent of the rest (so entries with both flags occur).  The remaining row
payloads are distinct bit patterns with NaN payloads, -0.0f and denormals among them.  ONE next_achieved_goal holds a NaN.

No synthetic entry is a collision and a success at once.  The step kernel adds w_success for the geometric success even in a step
that collides, while is_success of such a step is 0; the rule takes the stored is_success as succ0, so for such an entry of the
additive kinds it cannot tell that the stored reward holds w_success (``blind_spot_entry`` and its test state what it then returns).
"""
import math

import numpy as np

from nstep_cases import FLOAT_FIELDS, RING_STATES as NSTEP_RING_STATES, SPECIAL_BITS, same_bits  # noqa: F401
from ur_gym_amd import _abi
from ur_gym_amd.evaluation import philox4x32_10

CAPACITY = 12
NUM_ENVS = (1, 5, 257)
# (filled, oldest_slot): the states of nstep_cases (none of which wraps in a ring of 12 slots) and two whose windows cross the ring's
# seam, one full and one not
RING_STATES = tuple(NSTEP_RING_STATES) + ((12, 5), (7, 8))
HORIZONS = (1, 4, 256)
COUNTS = (1, 63, 64, 65, 1000)  # a lone lane, the wave boundary from both sides, sixteen waves with a tail
THRESHOLDS = (0, 1 << 31, (4 << 32) // 5, 1 << 32)
STRATEGIES = (_abi.HER_GOAL_FUTURE, _abi.HER_GOAL_FINAL, _abi.HER_GOAL_OWN)
KINDS = (_abi.ENV_ORI, _abi.ENV_OBS, _abi.ENV_DYN, _abi.ENV_STA)
SEED, DRAW = 0x48455221, 23  # chosen so that the census holds in every count-1000 case (test_her_host.py checks it)
NAN_GOAL_AT = (2, 0)  # (slot, env) of the next_achieved_goal that holds a NaN
# the reference's constants per env kind (reach.py; urgym_config_default states the same, test_abi_and_host.py compares them)
WEIGHTS = {_abi.ENV_ORI: (-70.0, -30.0), _abi.ENV_OBS: (-100.0, 0.0), _abi.ENV_DYN: (-70.0, -30.0), _abi.ENV_STA: (-70.0, -30.0)}


def config(kind):
    wd, wo = WEIGHTS[kind]
    return dict(env_kind=kind, distance_threshold=0.05, ori_threshold=0.0873, w_collision=-500.0, w_success=200.0, w_distance=wd, w_orientation=wo)


def cases():
    """The (N, filled, oldest, horizon, strategy, kind, threshold) list at count 1000: every N x ring state x horizon x strategy, with
    the env kind and the threshold rotating so that every (kind, threshold), (kind, strategy) and (threshold, strategy) pair occurs."""
    out, i = [], 0
    for N in NUM_ENVS:
        for filled, oldest in RING_STATES:
            for horizon in HORIZONS:
                for strategy in STRATEGIES:
                    out.append((N, filled, oldest, horizon, strategy, KINDS[i % 4], THRESHOLDS[(i // 4 + i) % 4]))
                    i += 1
    return out


def _quat_zyx(a0, a1, a2):
    """qz(a0) qy(a1) qx(a2) as (x, y, z, w), Hamilton products"""
    def mul(a, b):
        ax, ay, az, aw = a
        bx, by, bz, bw = b
        return (aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                aw * bw - ax * bx - ay * by - az * bz)
    qz = (0.0, 0.0, math.sin(0.5 * a0), math.cos(0.5 * a0))
    qy = (0.0, math.sin(0.5 * a1), 0.0, math.cos(0.5 * a1))
    qx = (math.sin(0.5 * a2), 0.0, 0.0, math.cos(0.5 * a2))
    return mul(mul(qz, qy), qx)


def pose_terms(a, g):
    """(distance, angular distance) of two poses xyz (+ rpy) given as float32 rows, in Python float64 from the definitions: the L2 norm
    of the position difference, and twice the arc cosine of |<qa, qb>| of the ZYX quaternions (0 for a position alone)."""
    a, g = [float(x) for x in a], [float(x) for x in g]
    d = math.sqrt(sum((a[k] - g[k]) ** 2 for k in range(3)))
    if len(a) == 3:
        return d, 0.0
    if any(math.isnan(x) or math.isinf(x) for x in a[3:] + g[3:]):
        return d, math.nan
    dot = sum(x * y for x, y in zip(_quat_zyx(*a[3:]), _quat_zyx(*g[3:])))
    return d, 2.0 * math.acos(min(1.0, abs(dot)))


def synthetic_ring(num_envs, kind, seed=11):
    """The ring's eleven fields as host arrays [C, N, ...] for env kind `kind`, and the shaping term [C, N] its rewards were made with."""
    rng = np.random.default_rng(seed + 1000 * kind + num_envs)
    C, N = CAPACITY, num_envs
    obs_dim, goal_dim = _abi.OBS_DIMS[kind]
    cfg = config(kind)
    dims = dict(observation=obs_dim, achieved_goal=goal_dim, desired_goal=goal_dim, action=6, next_observation=obs_dim,
                next_achieved_goal=goal_dim, next_desired_goal=goal_dim)
    ring, tag = {}, 0
    for name in FLOAT_FIELDS:
        size = C * N * dims[name]
        bits = (np.arange(size, dtype=np.uint64) * 2654435761 + (tag << 28) + 54321).astype(np.uint32)  # distinct within the field
        bits[::11] = np.resize(np.array(SPECIAL_BITS, dtype=np.uint32), bits[::11].size)
        ring[name] = bits.view(np.float32).reshape(C, N, dims[name]).copy()
        tag += 1
    goal = np.concatenate([rng.uniform(-0.5, 0.5, (C, N, 3)), rng.uniform(-1.0, 1.0, (C, N, 3))], axis=2)[..., :goal_dim]
    near = rng.random((C, N)) < 0.15
    delta = np.where(near[..., None], rng.uniform(-0.01, 0.01, (C, N, 6)), rng.normal(0.0, 0.3, (C, N, 6)))[..., :goal_dim]
    ring["next_desired_goal"] = goal.astype(np.float32)
    ring["next_achieved_goal"] = (goal + delta).astype(np.float32)
    coll = rng.random((C, N)) < 0.08
    shaping = np.zeros((C, N)) if kind == _abi.ENV_ORI else rng.normal(0.0, 2.0, (C, N))
    reward, term, succ = np.zeros((C, N), np.float32), np.zeros((C, N), np.uint8), np.zeros((C, N), np.uint8)
    for s in range(C):
        for n in range(N):
            d, th = pose_terms(ring["next_achieved_goal"][s, n], ring["next_desired_goal"][s, n])
            ok = d < cfg["distance_threshold"] and (goal_dim == 3 or th < cfg["ori_threshold"])
            c = bool(coll[s, n]) and not ok  # a collision and a success in one step are kept apart (see the module's text)
            if kind in (_abi.ENV_ORI, _abi.ENV_OBS):
                r = (cfg["w_success"] if ok else 0.0) + (cfg["w_collision"] if c else 0.0) + cfg["w_distance"] * d + cfg["w_orientation"] * th + shaping[s, n]
            else:
                r = cfg["w_collision"] if c else cfg["w_success"] if ok else cfg["w_distance"] * d + cfg["w_orientation"] * th + shaping[s, n]
            reward[s, n], term[s, n], succ[s, n] = r, ok or c, (ok or c) and not c
    ring["next_achieved_goal"][NAN_GOAL_AT][0] = np.nan  # after the forward model: the stored row is an ordinary one
    ring.update(reward=reward, terminated=term, truncated=(rng.random((C, N)) < 0.12).astype(np.uint8), is_success=succ)
    return ring, shaping


def words(seed, draw, count):
    """The four Philox words of urgym_replay_sample's draw for rows 0 .. count - 1, as Python integers."""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    w = philox4x32_10(key, (np.arange(count, dtype=np.uint64), np.uint64(draw & 0xFFFFFFFF), np.uint64(draw >> 32), np.uint64(_abi.REPLAY_TAG)))
    return [[int(w[k][i]) for k in range(4)] for i in range(count)]


def rescore(cfg, goal_dim, r, terminated, succ0, d, th, d0, th0):
    """The re-scoring rule of the issue on Python floats (IEEE double, one rounding per operation): (r', terminated', is_success',
    the branch taken)."""
    wd, wo, ws, wc = cfg["w_distance"], cfg["w_orientation"], cfg["w_success"], cfg["w_collision"]
    coll = bool(terminated) and not succ0
    succ = d < cfg["distance_threshold"] and (goal_dim == 3 or th < cfg["ori_threshold"])
    r = float(r)
    if cfg["env_kind"] in (_abi.ENV_ORI, _abi.ENV_OBS):
        G = lambda s, dist, ang: (((ws if s else 0.0) + (wc if coll else 0.0)) + wd * dist) + wo * ang  # noqa: E731
        out, branch = (r - G(succ0, d0, th0)) + G(succ, d, th), "additive"
    elif coll:
        out, branch = wc, "collision"
    elif succ:
        out, branch = ws, "success"
    else:
        S = ((r - wd * d0) - wo * th0) if not succ0 else 0.0
        out, branch = (wd * d + wo * th) + S, "shaping"
    term = succ or coll
    return np.float32(out), int(term), int(term and not coll), branch, coll, succ


def reference_rows(ring, kind, oldest, filled, w4, threshold, strategy, horizon, terms=pose_terms):
    """The rule of include/urgym.h as a per-row Python loop, written from the rule alone.  `w4`: the Philox words per row (``words``);
    `terms(a, g)`: the pose distances.  Per row a dict: index, relabel, F, j, g, goal_index, why the window ended, and -- for a
    relabelled row -- the new goal, the pose terms, the new reward and flags and the branch taken."""
    C, N = ring["reward"].shape
    goal_dim = ring["desired_goal"].shape[2]
    cfg = config(kind)
    rows = []
    for w in w4:
        e = (((w[0] << 32) | w[1]) * (filled * N)) >> 64
        p, env = e // N, e % N
        slot = (oldest + p) % C
        H = min(horizon, filled - p)
        F, why = H, ("horizon" if H == horizon else "newest")
        for k in range(H):
            s = (oldest + p + k) % C
            if ring["terminated"][s, env] or ring["truncated"][s, env]:
                F, why = k + 1, ("terminated" if ring["terminated"][s, env] else "truncated")
                break
        j = (w[3] * F) >> 32 if strategy == _abi.HER_GOAL_FUTURE else F - 1
        gslot = (oldest + p + j) % C
        row = dict(index=slot * N + env, relabel=w[2] < threshold, F=F, j=j, g=gslot * N + env, why=why, seam=gslot < slot, age=p, slot=slot, env=env)
        row["goal_index"] = row["g"] if row["relabel"] and strategy != _abi.HER_GOAL_OWN else -1
        if row["relabel"]:
            a, g0 = ring["next_achieved_goal"][slot, env], ring["next_desired_goal"][slot, env]
            g1 = g0 if strategy == _abi.HER_GOAL_OWN else ring["next_achieved_goal"][gslot, env]
            d, th = terms(a, g1)
            d0, th0 = terms(a, g0)
            r, term, succ, branch, coll, new = rescore(cfg, goal_dim, ring["reward"][slot, env], ring["terminated"][slot, env], bool(ring["is_success"][slot, env]), d, th, d0, th0)
            row.update(goal=g1, terms=(d, th, d0, th0), reward=r, terminated=term, is_success=succ, branch=branch,
                       new_success=new and not coll and not ring["is_success"][slot, env])
        rows.append(row)
    return rows


WINDOW_KINDS = ("terminated", "truncated", "newest", "horizon", "F=1", "seam")
BRANCHES = ("collision", "new_success", "shaping", "additive")


def kinds_of(row):
    """the census categories a relabelled row of ``reference_rows`` belongs to"""
    out = {row["why"]}
    if row["F"] == 1:
        out.add("F=1")
    if row["seam"]:
        out.add("seam")
    if row["branch"] in ("collision", "shaping", "additive"):
        out.add(row["branch"])
    if row["new_success"]:
        out.add("new_success")
    return out


def census_wanted(ring, kind, oldest, filled, threshold, strategy, horizon, floor=0.02, envs=64):
    """What a case can hold: the categories whose probability under the draw (the entry uniform over the filled ring, j uniform over
    the window for FUTURE) is at least `floor`, by enumeration of every entry (of the first `envs` envs: the envs of a synthetic ring
    are made alike) and every j.  A ring of one slot holds no window longer than one step, a horizon of 256 ends no window in a ring
    of 12 slots, and the branching rewards have no additive row: what a case cannot hold is not asked of it.  At floor 0.02 a category
    is missed by 400 relabelled rows with probability 0.98^400 < 4e-4."""
    C, N = ring["reward"].shape
    if threshold == 0 or strategy == _abi.HER_GOAL_OWN:
        return set()
    mass, total, memo = {}, 0.0, {}

    def terms(a, g):
        key = (a.tobytes(), g.tobytes())
        if key not in memo:
            memo[key] = pose_terms(a, g)
        return memo[key]

    for p in range(filled):
        for env in range(min(N, envs)):
            e = p * N + env
            hi = (e << 64) // (filled * N) + 1  # a 64-bit word that draws e
            w01 = [hi >> 32, hi & 0xFFFFFFFF]
            F = reference_rows(ring, kind, oldest, filled, [w01 + [0, 0]], 1, _abi.HER_GOAL_FINAL, horizon, terms)[0]["F"]
            js = range(F) if strategy == _abi.HER_GOAL_FUTURE else [F - 1]
            for j in js:
                w3 = ((j << 32) + F - 1) // F if strategy == _abi.HER_GOAL_FUTURE else 0  # the smallest word with (w3 F) >> 32 == j
                row = reference_rows(ring, kind, oldest, filled, [w01 + [0, w3]], 1, strategy, horizon, terms)[0]
                assert row["index"] == ((oldest + p) % C) * N + env and row["j"] == j
                for k in kinds_of(row):
                    mass[k] = mass.get(k, 0.0) + 1.0 / len(js)
            total += 1.0
    return {k for k, m in mass.items() if m / total >= floor}


def blind_spot_entry(kind):
    """A ring of one slot and one env whose only step collides while its pose lies within the thresholds of its goal, as the step
    kernel stores it: terminated = 1, is_success = 0, and for the additive kinds a reward that holds w_success AND w_collision."""
    obs_dim, goal_dim = _abi.OBS_DIMS[kind]
    cfg = config(kind)
    goal = np.array([0.3, -0.2, 0.4, 0.5, -0.25, 0.75], np.float32)[:goal_dim]
    ach = goal + np.float32(0.0078125)
    d, th = pose_terms(ach, goal)
    assert d < cfg["distance_threshold"] and th < cfg["ori_threshold"]
    r = cfg["w_success"] + cfg["w_collision"] + cfg["w_distance"] * d + cfg["w_orientation"] * th if kind in (_abi.ENV_ORI, _abi.ENV_OBS) else cfg["w_collision"]
    zeros = lambda *shape: np.zeros(shape, np.float32)  # noqa: E731
    ring = dict(observation=zeros(1, 1, obs_dim), achieved_goal=zeros(1, 1, goal_dim), desired_goal=goal.reshape(1, 1, -1).copy(), action=zeros(1, 1, 6),
                reward=np.full((1, 1), r, np.float32), next_observation=zeros(1, 1, obs_dim), next_achieved_goal=ach.reshape(1, 1, -1).copy(),
                next_desired_goal=goal.reshape(1, 1, -1).copy(), terminated=np.ones((1, 1), np.uint8), truncated=np.zeros((1, 1), np.uint8),
                is_success=np.zeros((1, 1), np.uint8))
    return ring, (d, th)
