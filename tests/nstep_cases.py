"""Shared cases of the multi-step return tests (test_nstep_host.py on the CPU, test_nstep.py on the GPU): synthetic rings, the ring
states, the independent per-row reference and the census of what the drawn rows cover.  No GPU, no native library.

A synthetic ring is [C = 7][N][...] with N = 3 or 5.  Its flags are laid out so that EVERY ring state below holds every kind of window:
env 0 never ends an episode (its windows stop at the newest slot or run full, and take every length the state allows), env 1 has
`terminated` set in slots 0, 3 and 4, env 2 has `truncated` set in slots 0, 2 and 5; further envs (N = 5) draw both flags at random
with rate 0.3, so that entries with both flags set occur as well.  Slot 0 carries flags because the state `filled = 1` holds nothing else.
The row payloads are distinct bit patterns with NaN payloads, -0.0f and denormals among them; rewards are ordinary numbers except ONE NaN.
"""
import numpy as np

CAPACITY = 7
NUM_ENVS = (3, 5)
# (filled, oldest_slot): growing rings start at slot 0; full rings with the oldest slot at 0 and at 3 (wrapped)
RING_STATES = ((1, 0), (2, 0), (4, 0), (7, 0), (7, 3))
N_STEPS = (1, 2, 3, 5, 32)
COUNTS = (1, 64, 65, 130)  # a lone lane, a full wave, the wave boundary, two waves and a tail
GAMMA = 0.95
SEED, DRAW = 0x5EED5AC, 41  # chosen so that the census below holds in every (N, ring state, n_steps > 1) case at count = 130
NAN_REWARD_AT = (2, 0)      # (slot, env): in env 0's clean run, so that it is reached as a first and as a later step
SPECIAL_BITS = (0x80000000, 0x00000001, 0x807FFFFF, 0x7FC01234, 0xFFC00001, 0x7FFFFFFF, 0x00000000, 0x7F800000)  # -0, denormals, NaNs, 0, inf
FLOAT_FIELDS = ("observation", "achieved_goal", "desired_goal", "action", "next_observation", "next_achieved_goal", "next_desired_goal")


def synthetic_ring(num_envs, obs_dim, goal_dim, seed=7):
    """The ring's eleven fields as host arrays [C, N, ...]."""
    rng = np.random.default_rng(seed + num_envs)
    C, N = CAPACITY, num_envs
    dims = dict(observation=obs_dim, achieved_goal=goal_dim, desired_goal=goal_dim, action=6, next_observation=obs_dim,
                next_achieved_goal=goal_dim, next_desired_goal=goal_dim)
    ring, tag = {}, 0
    for name in FLOAT_FIELDS:
        size = C * N * dims[name]
        bits = (np.arange(size, dtype=np.uint64) * 2654435761 + (tag << 28) + 12345).astype(np.uint32)  # distinct within the field
        bits[::11] = np.resize(np.array(SPECIAL_BITS, dtype=np.uint32), bits[::11].size)
        ring[name] = bits.view(np.float32).reshape(C, N, dims[name]).copy()
        tag += 1
    reward = rng.uniform(-3.0, 1.0, (C, N)).astype(np.float32)
    reward[NAN_REWARD_AT] = np.nan
    term, trunc = np.zeros((C, N), np.uint8), np.zeros((C, N), np.uint8)
    term[[0, 3, 4], 1] = 1
    trunc[[0, 2, 5], 2] = 1
    if N > 3:
        term[:, 3:] = rng.random((C, N - 3)) < 0.3
        trunc[:, 3:] = rng.random((C, N - 3)) < 0.3
    ring.update(reward=reward, terminated=term, truncated=trunc, is_success=(rng.random((C, N)) < 0.5).astype(np.uint8))
    return ring


def reference_rows(ring, oldest_slot, filled, entries, n_steps, gamma):
    """The rule of include/urgym.h as a per-row Python loop, written from the rule alone: for each drawn e a dict with m, entry_0,
    entry_last, why the walk stopped, the float64 return sum gamma^k r_k, the sum of |gamma^k r_k|, and gamma^m in float64 (gamma
    being the float32 number)."""
    C, N = ring["reward"].shape
    g32 = float(np.float32(gamma))
    rows = []
    for e in entries:
        p, env = int(e) // N, int(e) % N
        L = min(n_steps, filled - p)
        window = [((oldest_slot + p + k) % C) * N + env for k in range(L)]
        m, why = L, ("full" if L == n_steps else "newest")
        for k, entry in enumerate(window):
            slot = entry // N
            if ring["terminated"][slot, env] or ring["truncated"][slot, env]:
                m, why = k + 1, ("terminated" if ring["terminated"][slot, env] else "truncated")
                break
        terms = [g32 ** k * float(ring["reward"][window[k] // N, env]) for k in range(m)]
        rows.append(dict(m=m, first=window[0], last=window[m - 1], why=why, L=L, total=sum(terms), magnitude=sum(abs(t) for t in terms), discount=g32 ** m))
    return rows


def census(rows, n_steps, filled):
    """What the drawn rows cover, and what they must cover in a (ring state, n_steps > 1) case: a row stopped by terminated, one by
    truncated, one at the newest slot, one full window, and every m from 1 to min(n_steps, 5).  A ring of `filled` slots holds no
    window longer than `filled`, so the last two are asked up to what it can hold: a full window where filled >= n_steps, and every m
    from 1 to min(n_steps, 5, filled)."""
    have = dict(terminated=any(r["why"] == "terminated" for r in rows), truncated=any(r["why"] == "truncated" for r in rows),
                newest=any(r["why"] == "newest" for r in rows), full=any(r["why"] == "full" for r in rows), lengths={r["m"] for r in rows})
    want_lengths = set(range(1, min(n_steps, 5, filled) + 1))
    missing = [k for k in ("terminated", "truncated", "newest") if not have[k]]
    if filled >= n_steps and not have["full"]:
        missing.append("full")
    if not want_lengths <= have["lengths"]:
        missing.append(f"lengths {sorted(want_lengths - have['lengths'])}")
    return have, missing


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def entropy_inputs(count, seed=3):
    """Rows for urgym_sac_entropy_step_nstep: returns, bootstrap values, discounts gamma^m with m in 1..5, log-probabilities, flags."""
    rng = np.random.default_rng(seed + count)
    f = np.float32
    steps = rng.integers(1, 6, count)
    discount = np.ones(count, f)
    for k in range(5):
        discount = np.where(steps > k, discount * f(GAMMA), discount).astype(f)
    return dict(log_prob=rng.normal(-4.0, 2.0, count).astype(f), reward=rng.uniform(-9.0, 3.0, count).astype(f),
                q_min_next=rng.normal(-20.0, 10.0, count).astype(f), discount=discount, next_log_prob=rng.normal(-4.0, 2.0, count).astype(f),
                terminated=(rng.random(count) < 0.2).astype(np.uint8), l=f(rng.normal(-0.5, 0.2)), m=f(rng.normal(0, 1e-2)), v=f(abs(rng.normal(0, 1e-3))))
