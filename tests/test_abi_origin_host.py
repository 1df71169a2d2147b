"""The origin map's part of the C ABI without a device: the eleven symbols are declared, exported and prototyped, the record
has one size (96 bytes) in the library, in the ctypes mirror and in the NumPy dtype with the fields at the header's offsets,
origin.hpp and keyed.hpp are among the hashed sources, and the calls refuse a null handle without touching a device."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

SYMBOLS = ("cetkmc_origin_begin", "cetkmc_origin_end", "cetkmc_origin_absorb_events", "cetkmc_origin_read", "cetkmc_origin_census",
           "cetkmc_origin_seq", "cetkmc_origin_profile", "cetkmc_ensemble_origin_begin", "cetkmc_ensemble_origin_end",
           "cetkmc_ensemble_origin_census", "cetkmc_ensemble_origin_profile")


def _header():
    return open(os.path.join(ROOT, "include", "cetkmc.h")).read()


def test_symbols_and_struct_size():
    from cetkmc import _lib
    lib = _lib.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert len(SYMBOLS) == 11
    for name in SYMBOLS:
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert lib.cetkmc_struct_size(b"origin_rec") == 96 == C.sizeof(_lib.OriginRec)
    assert _lib.STRUCT_MIRRORS["origin_rec"] is _lib.OriginRec
    assert '"origin_rec"' in _header()                         # the list of names cetkmc_struct_size documents
    assert lib.cetkmc_abi_version() == 1                       # purely additive


def test_layout():
    import cetkmc
    import origin_ref as OR
    from cetkmc import _lib
    dt = cetkmc.engine.ORIGIN_DTYPE
    want = {"n_occ": 0, "n_by": 8, "n_unrec": 40, "n_left": 48, "ord_sum": 56, "ord_min": 64, "ord_max": 72, "birth": 80, "pad": 88}
    assert dt.itemsize == 96 == OR.REC.itemsize
    assert {k: dt.fields[k][1] for k in dt.names} == want == {k: OR.REC.fields[k][1] for k in OR.REC.names}
    assert {k: getattr(_lib.OriginRec, k).offset for k in want} == want
    body = re.search(r"struct cetkmc_origin_rec \{(.*?)\};", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S), flags=re.S).group(1)
    assert re.findall(r"\b(n_occ|n_by|n_unrec|n_left|ord_sum|ord_min|ord_max|birth|pad)\b(?:\[\d\])?[,;]", body) == list(want)
    assert cetkmc.engine.EVENT_DTYPE == OR.EVENT
    o, c = cetkmc.engine.origin_decode(np.array([0, (8 << 3) | 1, (1 << 3) | 5], np.uint64))
    assert o.tolist() == [-1, 7, 0] and c.tolist() == [0, 1, 5]


def test_sources_and_null_handles():
    from cetkmc import _lib
    for f in ("origin.hpp", "keyed.hpp"):
        assert os.path.join(_lib.CSRC, f) in _lib.sources()
    lib = _lib.load()
    buf = np.zeros(4, dtype=np.dtype([("w", "<i8", 12)]))
    calls = (lambda: lib.cetkmc_origin_begin(None), lambda: lib.cetkmc_origin_end(None),
             lambda: lib.cetkmc_origin_absorb_events(None, buf.ctypes.data, 1, 1),
             lambda: lib.cetkmc_origin_read(None, buf.ctypes.data), lambda: lib.cetkmc_origin_census(None, buf.ctypes.data),
             lambda: lib.cetkmc_origin_profile(None, buf.ctypes.data, 0, None),
             lambda: lib.cetkmc_ensemble_origin_begin(None), lambda: lib.cetkmc_ensemble_origin_end(None),
             lambda: lib.cetkmc_ensemble_origin_census(None, buf.ctypes.data),
             lambda: lib.cetkmc_ensemble_origin_profile(None, buf.ctypes.data, None))
    for call in calls:
        assert call() != 0 and b"null" in lib.cetkmc_last_error()
    assert lib.cetkmc_origin_seq(None) == -1
    assert not buf["w"].any()
