"""CPU tests (-m "not gpu") of how ``VectorEnv.sac_train`` picks one of the eight urgym_sac_train* entry points.

  * ``vector_env._sac_train_entry`` names, for all 128 presence combinations of the seven options, the symbol the priority list
    gives; the list is written out here, not read from the table.
  * each symbol's option tuple lines up with the signature ``_native`` declares for it: the count, and at every option's position the
    pointer to that option's ``_abi`` struct.
  * all eight symbols refuse a NULL handle, and every pointer NULL, with URGYM_ERR_ARG.
"""
import ctypes as C
import itertools

import pytest

from ur_gym_amd import _abi, _native
from ur_gym_amd.vector_env import _sac_train_entry

OPTIONS = ("evaluation", "monitor", "nstep", "prioritized", "hindsight", "clipping", "normalizer")
STRUCT = {"evaluation": _abi.SacEvaluation, "monitor": _abi.SacMonitoring, "nstep": _abi.SacNstep, "prioritized": _abi.SacPrioritized,
          "hindsight": _abi.SacHindsight, "clipping": _abi.SacClipping, "normalizer": _abi.Normalization}
SYMBOLS = ("urgym_sac_train", "urgym_sac_train_evaluated", "urgym_sac_train_monitored", "urgym_sac_train_nstep", "urgym_sac_train_prioritized",
           "urgym_sac_train_hindsight", "urgym_sac_train_clipped", "urgym_sac_train_normalized")


def expected_symbol(present):
    if "normalizer" in present:
        return "urgym_sac_train_normalized"
    if "clipping" in present:
        return "urgym_sac_train_clipped"
    if "hindsight" in present:
        return "urgym_sac_train_hindsight"
    if "prioritized" in present:
        return "urgym_sac_train_prioritized"
    if "nstep" in present:
        return "urgym_sac_train_nstep"
    if "monitor" in present:
        return "urgym_sac_train_monitored"
    if "evaluation" in present:
        return "urgym_sac_train_evaluated"
    return "urgym_sac_train"


def test_every_presence_combination_names_the_symbol_of_the_priority_list():
    seen = set()
    combinations = [set(c) for r in range(len(OPTIONS) + 1) for c in itertools.combinations(OPTIONS, r)]
    assert len(combinations) == 128
    for present in combinations:
        symbol, options = _sac_train_entry(present)
        assert symbol == expected_symbol(present), present
        if len(present & {"nstep", "prioritized", "hindsight"}) <= 1:  # (two gathers: sac_train raises before it gets here)
            assert present <= set(options), (present, symbol)  # whatever is given has a place in the signature that was picked
        assert _sac_train_entry({o: object() for o in present}) == (symbol, options)  # a dict of structs, as sac_train passes it
        seen.add(symbol)
    assert seen == set(SYMBOLS)


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_option_tuple_lines_up_with_the_declared_signature(symbol):
    rows = {_sac_train_entry(set(c)) for r in range(len(OPTIONS) + 1) for c in itertools.combinations(OPTIONS, r)}
    (options,) = [o for s, o in rows if s == symbol]  # one row per symbol
    argtypes = getattr(_native.lib(), symbol).argtypes
    assert len(options) + 4 == len(argtypes)
    assert argtypes[0] is C.c_void_p and argtypes[-1] is C.c_void_p
    assert argtypes[1] is C.POINTER(_abi.SacLearner) and argtypes[2] is C.POINTER(_abi.SacSchedule)
    assert len(set(options)) == len(options)
    for position, option in enumerate(options):
        assert argtypes[3 + position] is C.POINTER(STRUCT[option]), (symbol, position, option)


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_null_handle_and_all_null_are_refused(symbol):
    lib = _native.lib()
    fn = getattr(lib, symbol)
    structs = [C.byref(t._type_()) for t in fn.argtypes[1:-1]]
    assert fn(None, *structs, None) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
    assert fn(*[None] * len(fn.argtypes)) == _abi.ERR_ARG
    assert b"null handle" in lib.urgym_last_error(None)
