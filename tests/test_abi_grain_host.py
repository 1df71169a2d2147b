"""The per-grain table's part of the C ABI without a device: the two symbols are declared, exported and prototyped, the
record is 160 bytes in the library, in the ctypes mirror and in the NumPy dtype with the fields at the header's offsets, the
new header is among the hashed sources, and the calls refuse a null handle without touching a device."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "cetkmc.h")).read()


def test_symbols_and_record_size():
    from cetkmc import _lib
    lib = _lib.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("cetkmc_grain_table", "cetkmc_ensemble_grain_table"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert lib.cetkmc_struct_size(b"grain_rec") == 160 == C.sizeof(_lib.GrainRec)
    assert _lib.STRUCT_MIRRORS["grain_rec"] is _lib.GrainRec
    assert '"grain_rec"' in _header()                          # the list of names cetkmc_struct_size documents
    assert lib.cetkmc_abi_version() == 1                       # purely additive


def test_record_layout():
    import cetkmc
    from cetkmc import _lib
    dt = cetkmc.engine.GRAIN_DTYPE
    assert dt.itemsize == 160
    want = {"n": 0, "sum": 8, "sq": 32, "n_state": 80, "nb": 112, "first_theta": 144, "first_phi": 152}
    assert {k: dt.fields[k][1] for k in dt.names} == want
    assert {k: getattr(_lib.GrainRec, k).offset for k in want} == want
    body = re.search(r"struct cetkmc_grain_rec \{(.*?)\};", _header(), flags=re.S).group(1)
    names = re.findall(r"\b(n|sum|sq|n_state|nb_same|nb_other|nb_empty|nb_out|first_theta|first_phi)\b(?:\[\d\])?[,;]", body)
    assert names == ["n", "sum", "sq", "n_state", "nb_same", "nb_other", "nb_empty", "nb_out", "first_theta", "first_phi"]


def test_sources_and_null_handles():
    from cetkmc import _lib
    assert os.path.join(_lib.CSRC, "grain.hpp") in _lib.sources()
    lib = _lib.load()
    buf = np.zeros(2, dtype=np.dtype([("w", "<i8", 20)]))
    assert lib.cetkmc_grain_table(None, 2, buf.ctypes.data) != 0 and b"null" in lib.cetkmc_last_error()
    assert lib.cetkmc_ensemble_grain_table(None, buf.ctypes.data) != 0 and b"null" in lib.cetkmc_last_error()
    assert not buf["w"].any()
