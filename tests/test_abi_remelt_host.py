"""Remelting's part of the C ABI without a device: the five symbols (and the timing entry point) are declared, exported and prototyped, the struct has one
size in the library and in the ctypes mirror with the fields in the header's order, melt.hpp is among the hashed sources, the
invalidation table has no new row, and the calls refuse a null handle without touching a device."""
import ctypes as C
import os
import re

from conftest import ROOT

SYMBOLS = ("cetkmc_set_remelt", "cetkmc_remelt", "cetkmc_get_remelt_info", "cetkmc_ensemble_set_remelt", "cetkmc_ensemble_remelt_info",
           "cetkmc_time_remelt")      # the issue's five, and the hipEvent-timed pass tools/remelt_timing.py measures with
FIELDS = ("passes", "n_melted", "n_melted_last", "n_appended")


def _header():
    return open(os.path.join(ROOT, "include", "cetkmc.h")).read()


def test_symbols_and_struct():
    from cetkmc import _lib
    lib = _lib.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert lib.cetkmc_struct_size(b"remelt_info") == 32 == C.sizeof(_lib.RemeltInfo)
    assert _lib.STRUCT_MIRRORS["remelt_info"] is _lib.RemeltInfo
    assert '"remelt_info"' in _header()                        # the list of names cetkmc_struct_size documents
    assert [getattr(_lib.RemeltInfo, f).offset for f in FIELDS] == [0, 8, 16, 24]
    body = re.search(r"struct cetkmc_remelt_info \{(.*?)\};", code, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)\b[,;]", body) == list(FIELDS) and "int64_t" in body
    assert lib.cetkmc_abi_version() == 1                       # purely additive


def test_sources_table_and_null_handles():
    from cetkmc import _lib
    assert os.path.join(_lib.CSRC, "melt.hpp") in _lib.sources()
    lib = _lib.load()
    # the direct pass raises the existing cause: row sums and interface sums stale, the rate table valid
    assert lib.cetkmc_invalidates(b"apply") == 1 | 4 and lib.cetkmc_invalidates(b"remelt") == -1
    info = _lib.RemeltInfo()
    calls = (lambda: lib.cetkmc_set_remelt(None, 1, 3695.0), lambda: lib.cetkmc_remelt(None, 3695.0, C.byref(info)),
             lambda: lib.cetkmc_get_remelt_info(None, C.byref(info)), lambda: lib.cetkmc_ensemble_set_remelt(None, 1, 3695.0),
             lambda: lib.cetkmc_ensemble_remelt_info(None, C.addressof(info)),
             lambda: lib.cetkmc_time_remelt(None, 3695.0, 1, C.byref(C.c_double(0.0))))
    assert len(calls) == len(SYMBOLS)
    for call in calls:
        assert call() != 0 and b"null" in lib.cetkmc_last_error()
    assert [getattr(info, f) for f in FIELDS] == [0, 0, 0, 0]
