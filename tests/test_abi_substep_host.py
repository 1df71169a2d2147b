"""Sub-stepping's part of the C ABI without a device: the four symbols are declared, exported and prototyped, the struct has
one size in the library and in the ctypes mirror with the fields in the header's order, thermal_sub.hpp is among the hashed
sources, the invalidation table has no new row, and the calls refuse a null handle without touching a device."""
import ctypes as C
import os
import re

from conftest import ROOT

SYMBOLS = ("cetkmc_set_thermal_substeps", "cetkmc_ensemble_set_thermal_substeps", "cetkmc_get_substep_info", "cetkmc_time_thermal")
FIELDS = ("updates", "substeps", "launches", "blocked_launches")


def _header():
    return open(os.path.join(ROOT, "include", "cetkmc.h")).read()


def test_symbols_and_struct():
    from cetkmc import _lib
    lib = _lib.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert lib.cetkmc_struct_size(b"substep_info") == 32 == C.sizeof(_lib.SubstepInfo)
    assert _lib.STRUCT_MIRRORS["substep_info"] is _lib.SubstepInfo
    assert '"substep_info"' in _header()                       # the list of names cetkmc_struct_size documents
    assert [getattr(_lib.SubstepInfo, f).offset for f in FIELDS] == [0, 8, 16, 24]
    body = re.search(r"struct cetkmc_substep_info \{(.*?)\};", code, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)\b[,;]", body) == list(FIELDS) and "int64_t" in body
    assert int(re.search(r"#define CETKMC_MAX_THERMAL_SUBSTEPS (\d+)", code).group(1)) == 65536
    assert lib.cetkmc_abi_version() == 1                       # purely additive


def test_sources_table_and_null_handles():
    from cetkmc import _lib
    assert os.path.join(_lib.CSRC, "thermal_sub.hpp") in _lib.sources()
    lib = _lib.load()
    # the last blocked launch raises the existing cause: row sums and rate table stale
    assert lib.cetkmc_invalidates(b"thermal_update") & 3 == 3 and lib.cetkmc_invalidates(b"thermal_substeps") == -1
    info = _lib.SubstepInfo()
    calls = (lambda: lib.cetkmc_set_thermal_substeps(None, 2), lambda: lib.cetkmc_ensemble_set_thermal_substeps(None, 2),
             lambda: lib.cetkmc_get_substep_info(None, C.byref(info)),
             lambda: lib.cetkmc_time_thermal(None, 0, 1, C.byref(C.c_double(0.0))))
    assert len(calls) == len(SYMBOLS)
    for call in calls:
        assert call() != 0 and b"null" in lib.cetkmc_last_error()
    assert [getattr(info, f) for f in FIELDS] == [0, 0, 0, 0]
