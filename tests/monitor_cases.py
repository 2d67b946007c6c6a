"""Cases of the monitor tests, shared by tests/test_monitor_host.py (CPU) and tests/test_monitor.py (GPU): synthetic
rings of C = 4 slots, a script of folds and records over them that meets every path of the two kernels, the restatement run over that
script, and placement cases.  No GPU, no torch."""
import numpy as np

from ur_gym_amd import _abi
from ur_gym_amd.evaluation import monitor_fold, monitor_stats

CAP = 4
HOST_COUNTS = (1, 63, 65, 1023, 1024, 1025, 2049)  # around a wave of 64, around the 1024 lanes of the ordered sum, three terms a lane
DEVICE_COUNTS = (1, 65, 1025)                      # one lane, a second wave, a fifth workgroup of the fold and a second term in the sum
FLOATS = ("mean_return", "mean_length", "success_rate", "sum_return")
INTS = ("episodes", "length_sum", "successes", "iteration", "reserved0")


def zero_state(n):
    return {name: np.zeros(n, np.dtype(ct)) for name, ct in _abi.MONITOR_STATE_FIELDS}


def rewards(n, seed):
    """float32 [CAP, n] as the reference's rewards look: small values of both signs, the -500 collision penalty, values near 1e-9 and near
    1e6."""
    rng = np.random.default_rng(7000 * seed + n)
    r = rng.uniform(-1.0, 3.0, (CAP, n))
    kind = rng.integers(0, 8, (CAP, n))
    r = np.where(kind == 0, -500.0, r)
    r = np.where(kind == 1, r * 1e-9, r)
    r = np.where(kind == 2, r * 1e6, r)
    r = np.ascontiguousarray(r, dtype=np.float32)
    # whatever the draw, every kind is there when there is room for it
    for j, v in enumerate((-500.0, 2.5e-9, 1.25e6)):
        if n > j:
            r[j % CAP, j] = v
    return r


def rings(n):
    """name -> (reward float32, terminated, truncated, is_success uint8), each [CAP, n].
      quiet   no flag anywhere: no episode ends
      busy    terminated where (env + slot) % 3 == 0, truncated where (env + 2 slot) % 4 == 0: env 0 has BOTH on slot 0, some envs end an
              episode on every slot, some on none; is_success on a pattern of its own, also where no episode ends
      last    a NaN reward for env n // 2 in slot 1; every env ends an episode in slot 2, the last step of fold(0, 3), and nowhere else"""
    env, slot = np.meshgrid(np.arange(n), np.arange(CAP))
    u8 = lambda x: np.ascontiguousarray(x, dtype=np.uint8)  # noqa: E731
    zeros = np.zeros((CAP, n), np.uint8)
    busy = (rewards(n, 1), u8((env + slot) % 3 == 0), u8((env + 2 * slot) % 4 == 0) * 255, u8((env + slot) % 2 == 0) * 3)  # any non-zero byte counts
    nan = rewards(n, 2)
    nan[1, n // 2] = np.nan
    last = (nan, u8(slot == 2), zeros.copy(), u8((env % 5 == 0) & (slot == 2)))
    return {"quiet": (rewards(n, 0), zeros.copy(), zeros.copy(), u8(env % 2 == 0)), "busy": busy, "last": last}


# ("ring", name) puts that ring's content in place; ("fold", first_slot, K); ("stats", iteration tag, clear)
SCRIPT = [
    ("ring", "quiet"), ("fold", 0, 4),                 # K = C: an episode that ends on none of the folded steps
    ("stats", 1, 1),                                   # an interval with no finished episode: the quotients are +0.0
    ("ring", "busy"), ("fold", 3, 3),                  # a wrapping first_slot: slots 3, 0, 1; both flags on one step (env 0, slot 0)
    ("stats", 2, 0),                                   # clear = 0: the sums stay
    ("fold", 2, 1),                                    # K = 1
    ("stats", 3, 1),                                   # ... and are counted again, then cleared
    ("ring", "last"), ("fold", 0, 3),                  # the NaN reward; every episode ends on the LAST folded step
    ("stats", -4, 1),                                  # the interval with the NaN; the tag is the caller's, any int64
    ("ring", "busy"), ("fold", 0, 4),
    ("stats", 1 << 40, 1),                             # finite again
]
NAN_RECORD, AFTER_NAN_RECORD, EMPTY_RECORD = 3, 4, 0
# the fold of slots 3, 0, 1 in pieces
SPLIT = [("ring", "quiet"), ("fold", 0, 4), ("ring", "busy"), ("fold", 3, 1), ("fold", 0, 2)]
WHOLE = [("ring", "quiet"), ("fold", 0, 4), ("ring", "busy"), ("fold", 3, 3)]


def restate(n, script, state=None):
    """The restatement over `script` from `state` (default: all zero).  Returns (records, state)."""
    all_rings, ring, records = rings(n), None, []
    state = zero_state(n) if state is None else state
    for op in script:
        if op[0] == "ring":
            ring = all_rings[op[1]]
        elif op[0] == "fold":
            state = monitor_fold(state, *ring, op[1], op[2])
        else:
            rec, state = monitor_stats(state, op[1], clear=bool(op[2]))
            records.append(rec)
    return records, state


# (first_iteration, iterations, log_every): log_every in {1, 2, a non-divisor, larger than the call}, a first_iteration just below a
# multiple and on one
PLACEMENTS = [
    (0, 6, 1), (0, 6, 2), (0, 7, 3), (0, 5, 100), (3, 4, 2), (4, 4, 2), (9, 5, 10), (10, 5, 10), (2, 4, 4), (2 ** 40 + 1, 5, 3), (0, 1, 1),
]


def simulate_logging(first_iteration, iterations, log_every):
    """A training loop that counts its iterations and logs at every multiple of log_every: the trips followed by a record."""
    count, trips = first_iteration, []
    for i in range(iterations):
        count += 1
        if count % log_every == 0:
            trips.append(i)
    return trips
