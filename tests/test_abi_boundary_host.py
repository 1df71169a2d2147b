"""The thermal boundary's part of the C ABI without a device: the four symbols are declared, exported and prototyped, the enum
names the six faces in order, cetkmc_thermal_boundary (144 bytes) and cetkmc_boundary_info (32 bytes) have one size in the
library, in the ctypes mirrors and in the header's list of names, the handle calls refuse a null handle and the host routine
null tables without touching a device, and nothing that existed changed."""
import ctypes as C
import os
import re

from conftest import ROOT

SYMBOLS = ("cetkmc_set_thermal_boundary", "cetkmc_ensemble_set_thermal_boundary", "cetkmc_get_thermal_boundary", "cetkmc_implicit_coeffs_bc")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cetkmc.h")).read(), flags=re.S)


def test_symbols_enum_and_struct_sizes():
    import cetkmc
    from cetkmc import _lib
    lib = _lib.load()
    code = _code()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert lib.cetkmc_struct_size(b"thermal_boundary") == 144 == C.sizeof(_lib.ThermalBoundary)
    assert lib.cetkmc_struct_size(b"boundary_info") == 32 == C.sizeof(_lib.BoundaryInfo)
    assert _lib.STRUCT_MIRRORS["thermal_boundary"] is _lib.ThermalBoundary and _lib.STRUCT_MIRRORS["boundary_info"] is _lib.BoundaryInfo
    header = open(os.path.join(ROOT, "include", "cetkmc.h")).read()
    assert '"thermal_boundary"' in header and '"boundary_info"' in header
    body = re.search(r"struct cetkmc_thermal_boundary \{(.*?)\};", code, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)\[6\]", body) == [n for n, _ in _lib.ThermalBoundary._fields_] == ["beta", "T_ext", "ramp"]
    body = re.search(r"struct cetkmc_boundary_info \{(.*?)\};", code, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)\b[,;]", body) == [n for n, _ in _lib.BoundaryInfo._fields_] == ["updates", "steps", "launches", "coeff_uploads"]
    enum = re.search(r"enum \{ (CETKMC_FACE_I_LO = 0,[^}]*) \};", code).group(1)
    assert [w.split(" = ")[0] for w in enum.split(", ")] == ["CETKMC_FACE_" + f.upper() for f in cetkmc.engine.FACES]
    assert cetkmc.engine.FACES == ("i_lo", "i_hi", "j_lo", "j_hi", "k_lo", "k_hi")
    assert lib.cetkmc_abi_version() == 1                       # purely additive
    assert lib.cetkmc_struct_size(b"implicit_info") == 32       # (an existing struct, untouched)


def test_null_handles_and_tables():
    from cetkmc import _lib
    lib = _lib.load()
    b, info = _lib.ThermalBoundary(), _lib.BoundaryInfo()
    for name, call in (("cetkmc_set_thermal_boundary", lambda: lib.cetkmc_set_thermal_boundary(None, C.byref(b))),
                       ("cetkmc_ensemble_set_thermal_boundary", lambda: lib.cetkmc_ensemble_set_thermal_boundary(None, None)),
                       ("cetkmc_get_thermal_boundary", lambda: lib.cetkmc_get_thermal_boundary(None, C.byref(b), C.byref(info))),
                       ("cetkmc_implicit_coeffs_bc", lambda: lib.cetkmc_implicit_coeffs_bc(4, 1.0, 0.5, 0.5, None, None))):
        assert call() != 0
        err = lib.cetkmc_last_error()
        assert b"null" in err and name.encode() in err, err
    assert (info.updates, info.steps, info.launches, info.coeff_uploads) == (0, 0, 0, 0)


def test_python_boundary_argument_is_checked_before_the_library():
    """a malformed mapping is a ValueError that names the wrapper (no handle needed to find out)"""
    import pytest
    from cetkmc import engine
    for bad in ({"T_ext": [0] * 6}, {"beta": [0] * 5}, 7, {"beta": "x"}):
        with pytest.raises(ValueError, match="Engine.set_thermal_boundary"):
            engine._boundary_struct(bad, "Engine.set_thermal_boundary")
    assert engine._boundary_struct(None, "x") is None
