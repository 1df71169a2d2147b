"""The implicit scheme's part of the C ABI without a device: the four symbols are declared, exported and prototyped, the enum
holds its two values, cetkmc_implicit_info has one size (32 bytes) in the library, in the ctypes mirror and in the header's list
of names, thermal_imp.hpp is among the hashed sources, and the handle calls refuse a null handle without touching a device."""
import ctypes as C
import os
import re

from conftest import ROOT

SYMBOLS = ("cetkmc_set_thermal_scheme", "cetkmc_ensemble_set_thermal_scheme", "cetkmc_get_implicit_info", "cetkmc_implicit_coeffs")


def _header():
    return open(os.path.join(ROOT, "include", "cetkmc.h")).read()


def test_symbols_and_struct_size():
    from cetkmc import _lib
    lib = _lib.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert lib.cetkmc_struct_size(b"implicit_info") == 32 == C.sizeof(_lib.ImplicitInfo)
    assert _lib.STRUCT_MIRRORS["implicit_info"] is _lib.ImplicitInfo
    assert '"implicit_info"' in _header()
    body = re.search(r"struct cetkmc_implicit_info \{(.*?)\};", code, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)\b[,;]", body) == [n for n, _ in _lib.ImplicitInfo._fields_] == ["updates", "steps", "launches", "coeff_uploads"]
    assert re.search(r"enum \{ CETKMC_THERMAL_EXPLICIT = 0, CETKMC_THERMAL_IMPLICIT = 1 \};", code)
    assert lib.cetkmc_abi_version() == 1                       # purely additive


def test_sources_null_handles_and_the_marker_comment():
    import cetkmc
    from cetkmc import _lib
    assert os.path.join(_lib.CSRC, "thermal_imp.hpp") in _lib.sources()
    assert cetkmc.engine.THERMAL_SCHEMES == {"explicit": 0, "implicit": 1}
    lib = _lib.load()
    info = _lib.ImplicitInfo()
    for call in (lambda: lib.cetkmc_set_thermal_scheme(None, 1), lambda: lib.cetkmc_ensemble_set_thermal_scheme(None, 1),
                 lambda: lib.cetkmc_get_implicit_info(None, C.byref(info)), lambda: lib.cetkmc_implicit_coeffs(4, 1.0, None, None)):
        assert call() != 0 and b"null" in lib.cetkmc_last_error()
    assert (info.updates, info.steps, info.launches, info.coeff_uploads) == (0, 0, 0, 0)
    # the q_planes comment lists the calls that leave the applied-update marker alone
    assert re.search(r"cetkmc_set_thermal_substeps, cetkmc_set_thermal_scheme,", _header())
