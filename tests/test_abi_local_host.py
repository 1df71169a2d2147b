"""cetkmc_run_supersteps_local's part of the C ABI without a device: the symbol is declared, exported and prototyped, the
argument struct has one size (72 bytes) and one layout in the library, the header and the ctypes mirror, local.hpp is among
the hashed sources, and the call refuses a null handle without touching a device."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

FIELDS = {"step0": 0, "n_steps": 8, "box": 16, "defect_fraction": 24, "seed": 32, "thermal_mode": 40, "thermal_dt": 48,
          "max_events": 56, "horizon_events": 64}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cetkmc.h")).read(), flags=re.S)


def test_symbol_and_struct():
    from cetkmc import _lib
    lib = _lib.load()
    assert re.search(r"\bint\s+cetkmc_run_supersteps_local\s*\(", _header())
    assert hasattr(lib, "cetkmc_run_supersteps_local") and "cetkmc_run_supersteps_local" in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES["cetkmc_run_supersteps_local"][1]) == 9
    assert lib.cetkmc_struct_size(b"local_args") == 72 == C.sizeof(_lib.LocalArgs)
    assert _lib.STRUCT_MIRRORS["local_args"] is _lib.LocalArgs
    assert '"local_args"' in open(os.path.join(ROOT, "include", "cetkmc.h")).read()
    assert {k: getattr(_lib.LocalArgs, k).offset for k in FIELDS} == FIELDS
    body = re.search(r"typedef struct cetkmc_local_args \{(.*?)\} cetkmc_local_args;", _header(), flags=re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == list(FIELDS)
    assert lib.cetkmc_abi_version() == 1                       # purely additive
    assert os.path.join(_lib.CSRC, "local.hpp") in _lib.sources()


def test_null_arguments_are_refused():
    from cetkmc import _lib
    lib = _lib.load()
    a, res = _lib.LocalArgs(), _lib.RunResult()
    a.box, a.max_events, a.horizon_events = 8, 4, 1.0
    buf = np.zeros(8)
    assert lib.cetkmc_run_supersteps_local(None, C.byref(a), C.byref(res), buf.ctypes.data, None, None, None, None, None) != 0
    assert b"null" in lib.cetkmc_last_error()
    assert not buf.any() and res.steps_done == 0


def test_engine_method():
    import inspect

    import cetkmc
    sig = inspect.signature(cetkmc.Engine.run_supersteps_local)
    assert list(sig.parameters)[1:] == ["step0", "n", "defect_fraction", "seed", "max_events", "horizon_events", "thermal_mode",
                                        "thermal_dt", "want_events"]
    assert sig.parameters["thermal_mode"].default == 1 and sig.parameters["want_events"].default is False
