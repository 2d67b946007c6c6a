"""Shared cases of tests/test_mppi_train_host.py and tests/test_mppi_train.py: the diagnostics a plan leaves,
made up, with the entries that must be passed over; and where the plan-statistics records of a training call fall."""
import numpy as np

from ur_gym_amd import _abi
from ur_gym_amd.evaluation import monitor_points

HOST_COUNTS = (1, 2, 3, 1023, 1024, 1025, 65536)
GPU_COUNTS = (1, 3, 1025, 65536)
FLOATS = tuple(name for name, ct in _abi.MppiStatsRecord._fields_ if ct is _abi.C.c_double)
INTS = tuple(name for name, ct in _abi.MppiStatsRecord._fields_ if ct is not _abi.C.c_double)


def poisoned(E):
    """Where the made-up diagnostics of E parents are poisoned: parent -> what.  With few parents several fall on one parent."""
    return {"best_ninf": E // 2, "nominal_pinf": E // 3, "ess_nan": (2 * E) // 3, "nominal_nan": E - 1}


def plan_buffers(E, seed=0):
    """best_return, nominal_return, ess (float64 [E]), elite_count (int32 [E]) and threshold (float64 [E]) as a plan could leave them:
    one parent without a finite sample (best_return and threshold -inf, no elite), a NaN and a +inf nominal_return, a NaN ess, and from
    1025 parents on zeros of both signs in ess, two of them in one lane of the reduction."""
    rng = np.random.default_rng(1000 * seed + E)
    best = rng.normal(-50.0, 30.0, E)
    nominal = best - np.abs(rng.normal(0.0, 5.0, E))
    ess = rng.uniform(1.0, 64.0, E)
    elite_count = rng.integers(1, 6, E).astype(np.int32)
    threshold = best - rng.uniform(0.0, 9.0, E)
    at = poisoned(E)
    best[at["best_ninf"]], threshold[at["best_ninf"]], elite_count[at["best_ninf"]] = -np.inf, -np.inf, 0
    nominal[at["nominal_pinf"]] = np.inf
    nominal[at["nominal_nan"]] = np.nan
    ess[at["ess_nan"]] = np.nan
    if E >= 1025:
        ess[0], ess[1024], ess[7], ess[8] = 0.0, -0.0, -0.0, 0.0
    return dict(best_return=best, nominal_return=nominal, ess=ess, elite_count=elite_count, threshold=threshold)


def unplanned_buffers(E):
    """What the update leaves where no parent had a finite return: best_return, nominal_return and threshold -inf, no elite, and the
    nominal alone weighing in (ess = 1)."""
    ninf = np.full(E, -np.inf)
    return dict(best_return=ninf.copy(), nominal_return=ninf.copy(), ess=np.ones(E), elite_count=np.zeros(E, np.int32), threshold=ninf.copy())


def small_integers(E, seed=0):
    """Integer-valued diagnostics small enough for every float64 sum to be exact, a few parents passed over."""
    rng = np.random.default_rng(77 + 1000 * seed + E)
    best = rng.integers(-900, 100, E).astype(np.float64)
    nominal = best - rng.integers(0, 50, E).astype(np.float64)
    ess = rng.integers(1, 64, E).astype(np.float64)
    elite_count = rng.integers(0, 6, E).astype(np.int32)
    threshold = best - rng.integers(0, 9, E).astype(np.float64)
    best[::7], threshold[::7] = -np.inf, -np.inf
    nominal[3::11] = np.nan
    return dict(best_return=best, nominal_return=nominal, ess=ess, elite_count=elite_count, threshold=threshold)


def plain(buffers):
    """The three arrays a planner without urgym_mppi_adapt has."""
    return {k: buffers[k] for k in ("best_return", "nominal_return", "ess")}


def same_record(got, want):
    """Bitwise, except that a NaN equals a NaN: its sign and payload are the adder's."""
    for k in FLOATS:
        g, w = np.float64(got[k]), np.float64(want[k])
        if np.isnan(w):
            assert np.isnan(g), (k, g, w)
        else:
            assert g.tobytes() == w.tobytes(), (k, g, w)
    for k in INTS:
        assert int(got[k]) == int(want[k]), (k, got[k], want[k])


def record_of(raw, index=0):
    """Record `index` of `raw` (bytes of an array of urgym_mppi_stats_record) as a dict."""
    r = _abi.MppiStatsRecord.from_buffer_copy(raw, index * _abi.C.sizeof(_abi.MppiStatsRecord))
    return {name: getattr(r, name) for name, _ in _abi.MppiStatsRecord._fields_}


def plan_record_slots(first_iteration, first_record, iterations, log_every):
    """(slot, iteration tag) of the plan-statistics records of one call, as include/urgym.h states them: beside monitor record r, at the
    monitor's own index first_record + (records of the call so far), tagged first_iteration + i + 1."""
    return [(first_record + r, first_iteration + i + 1) for r, i in enumerate(monitor_points(first_iteration, iterations, log_every))]
