"""Cases of the evaluation tests, shared by tests/test_evaluation_host.py (CPU) and tests/test_evaluation.py (GPU):
episode arrays with mixed signs and magnitudes, the improvement-flag cases, and evaluation schedules."""
import numpy as np

HOST_COUNTS = (1, 2, 1023, 1024, 1025, 2049, 65536)   # around the 1024 lanes of the ordered sum, and the cap
DEVICE_COUNTS = (1, 63, 65, 1024, 1025, 65536)        # around a wave of 64, around the lanes, and the cap


def episodes(n, seed=0):
    """(returns float64 [n], last_step int32 [n], success uint8 [n]) as the reference's rewards look: small positive rewards summed over
    up to 100 steps, the -500 collision penalty on some episodes, a few tiny and a few large values, both signs."""
    rng = np.random.default_rng(1000 * seed + n)
    r = rng.uniform(0.0, 3.0, n)
    kind = rng.integers(0, 10, n)
    r = np.where(kind == 0, r - 500.0, r)                      # a collision
    r = np.where(kind == 1, -r * 40.0, r)                      # a long episode far from the goal
    r = np.where(kind == 2, r * 1e-9, r)                       # nearly nothing
    r = np.where(kind == 3, r * 1e6, r)                        # large
    last = rng.integers(0, 100, n).astype(np.int32)
    succ = (rng.integers(0, 3, n) == 0).astype(np.uint8)
    return np.ascontiguousarray(r, dtype=np.float64), last, succ


def flag_cases():
    """name -> (returns, best_mean before, improved expected, best state expected to change)."""
    inf = np.inf
    three = np.array([1.0, 2.0, 3.0])
    return {
        "first evaluation against -inf": (three, -inf, 1),
        "a tie": (three, 2.0, 0),                               # strict: equal is not improved
        "just above": (three, np.nextafter(2.0, 0.0), 1),
        "below": (three, 2.5, 0),
        "a NaN return": (np.array([1.0, np.nan, 3.0]), -inf, 0),  # the mean is NaN: never improved, the best state stays
        "a NaN return against a finite best": (np.array([np.nan]), -1e300, 0),
        "a mean of -inf": (np.array([1.0, -inf]), -inf, 0),     # -inf > -inf is false
        "a mean of -inf against a finite best": (np.array([-inf, -inf]), -5.0, 0),
        "a mean of +inf": (np.array([1.0, inf]), 1e300, 1),
    }


# (first_step, iterations, G, idle, E): idle iterations, G in {0, 1, 3}, E in {1, G, a non-multiple of G, larger than the call's updates},
# a first_step that sits just below a multiple of E
SCHEDULES = [
    (1, 6, 2, 1, 4),      # the GPU test's: evaluations after iterations 2 and 4
    (1, 6, 1, 0, 1),      # E = 1 = G: after every iteration
    (1, 6, 3, 0, 1),      # E = 1 < G: after every iteration, once
    (1, 6, 3, 2, 3),      # E = G with idle iterations
    (1, 7, 3, 0, 2),      # E a non-multiple of G, below it
    (1, 9, 3, 1, 7),      # E a non-multiple of G, above it
    (1, 5, 3, 0, 100),    # E larger than the call's updates: none
    (1, 5, 0, 0, 1),      # G = 0: no update, none
    (1, 5, 1, 5, 1),      # every iteration idle: none
    (1, 4, 1, 9, 2),      # more idle iterations than iterations
    (8, 4, 1, 0, 4),      # first_step - 1 = 7, just below a multiple of E: the first iteration passes it
    (9, 4, 1, 0, 4),      # first_step - 1 = 8, ON a multiple: the next is four updates away
    (4, 3, 3, 1, 4),      # 3 done; idle, then 6 and 9: both pass a multiple
    (2 ** 40, 3, 2, 0, 3),
]


def simulate_loop_rule(first_step, iterations, G, idle, E):
    """tools/train_sac.py's Python loop, update by update: an evaluation whenever ``updates % eval_every == 0`` after an update.  Returns
    the iterations (loop trips) in which at least one evaluation fell: the trips a native call evaluates after."""
    updates, trips = first_step - 1, []
    for i in range(iterations):
        if i < idle:        # the trip's `continue` before learning_starts
            continue
        hit = False
        for _ in range(G):
            updates += 1
            if updates % E == 0:
                hit = True
        if hit:
            trips.append(i)
    return trips
