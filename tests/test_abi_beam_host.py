"""The beam tables' part of the C ABI without a device: the four symbols and cetkmc_struct_size are
declared, exported and prototyped, cetkmc_beam (48 bytes) and cetkmc_beam_info (32 bytes) have one size in the library, in the
ctypes mirrors and in the header's list of names, the calls refuse a null handle by name without touching a device, and nothing
that existed changed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("cetkmc_set_beam", "cetkmc_ensemble_set_beam", "cetkmc_get_beam_info", "cetkmc_thermal_beam", "cetkmc_struct_size")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cetkmc.h")).read(), flags=re.S)


def test_symbols_and_struct_sizes():
    from cetkmc import _lib
    lib = _lib.load()
    code = _code()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert lib.cetkmc_struct_size(b"beam") == 48 == C.sizeof(_lib.Beam)
    assert lib.cetkmc_struct_size(b"beam_info") == 32 == C.sizeof(_lib.BeamInfo)
    assert _lib.STRUCT_MIRRORS["beam"] is _lib.Beam and _lib.STRUCT_MIRRORS["beam_info"] is _lib.BeamInfo
    header = open(os.path.join(ROOT, "include", "cetkmc.h")).read()
    assert '"beam"' in header and '"beam_info"' in header
    body = re.search(r"struct cetkmc_beam \{(.*?)\};", code, flags=re.S).group(1)
    assert re.findall(r"\*?(\w+)\s*[,;]", body) == [n for n, _ in _lib.Beam._fields_] == ["u0", "n_u", "depth", "amp", "gj", "gk", "fi"]
    body = re.search(r"struct cetkmc_beam_info \{(.*?)\};", code, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)\b[,;]", body) == [n for n, _ in _lib.BeamInfo._fields_] == ["updates", "steps", "launches", "table_uploads"]
    assert lib.cetkmc_abi_version() == 1                       # purely additive
    for name, size in (("implicit_info", 32), ("boundary_info", 32), ("thermal_boundary", 144)):        # existing structs, untouched
        assert lib.cetkmc_struct_size(name.encode()) == size


def test_null_handles():
    from cetkmc import _lib
    lib = _lib.load()
    info = _lib.BeamInfo()
    for name, call in (("cetkmc_set_beam", lambda: lib.cetkmc_set_beam(None, None)),
                       ("cetkmc_ensemble_set_beam", lambda: lib.cetkmc_ensemble_set_beam(None, 0, None, None)),
                       ("cetkmc_get_beam_info", lambda: lib.cetkmc_get_beam_info(None, C.byref(info))),
                       ("cetkmc_thermal_beam", lambda: lib.cetkmc_thermal_beam(None, 1e-6, 0, 1, 1))):
        assert call() != 0
        err = lib.cetkmc_last_error()
        assert b"null" in err and name.encode() in err, err
    assert (info.updates, info.steps, info.launches, info.table_uploads) == (0, 0, 0, 0)


def test_python_table_argument_is_checked_before_the_library():
    """a malformed table is a ValueError that names the wrapper (no handle needed to find out)"""
    from cetkmc import engine
    good = dict(u0=3, amp=np.ones(2), gj=np.ones((2, 5)), gk=np.ones((2, 5)), fi=[0.5, 0.5])
    for bad in (7, {"amp": [1.0]}, dict(good, gj=np.ones((2, 4))), dict(good, gk=np.ones((3, 5)))):
        with pytest.raises(ValueError, match="Engine.set_beam"):
            engine._beam_struct(bad, 5, "Engine.set_beam", [])
    keep = []
    b = engine._beam_struct(good, 5, "Engine.set_beam", keep)
    assert (b.u0, b.n_u, b.depth, len(keep)) == (3, 2, 2, 4) and b.gk[9] == 1.0 and b.fi[1] == 0.5
