"""The solidification map's part of the C ABI without a device: the nine symbols are declared, exported and prototyped, the
three structs have one size in the library, in the ctypes mirrors and in the NumPy dtypes with the fields at the header's
offsets, solid.hpp is among the hashed sources, and the calls refuse a null handle without touching a device."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

SYMBOLS = ("cetkmc_solid_begin", "cetkmc_solid_end", "cetkmc_solid_update", "cetkmc_solid_read", "cetkmc_solid_profile",
           "cetkmc_ensemble_solid_begin", "cetkmc_ensemble_solid_end", "cetkmc_ensemble_solid_update", "cetkmc_ensemble_solid_profile")


def _header():
    return open(os.path.join(ROOT, "include", "cetkmc.h")).read()


def test_symbols_and_struct_sizes():
    from cetkmc import _lib
    lib = _lib.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    for name, mirror, size in (("solid_info", _lib.SolidInfo, 24), ("solid_args", _lib.SolidArgs, 32), ("solid_rec", _lib.SolidRec, 80)):
        assert lib.cetkmc_struct_size(name.encode()) == size == C.sizeof(mirror)
        assert _lib.STRUCT_MIRRORS[name] is mirror
        assert '"%s"' % name in _header()                      # the list of names cetkmc_struct_size documents
    assert lib.cetkmc_abi_version() == 1                       # purely additive


def test_layouts():
    import cetkmc
    from cetkmc import _lib
    dt = cetkmc.engine.SOLID_DTYPE
    assert dt.itemsize == 80
    want = {"n_rec": 0, "n_bad": 8, "n_cooling": 16, "stamp_sum": 24, "stamp_min": 32, "stamp_max": 40, "q": 48}
    assert {k: dt.fields[k][1] for k in dt.names} == want
    assert {k: getattr(_lib.SolidRec, k).offset for k in want} == want
    body = re.search(r"struct cetkmc_solid_rec \{(.*?)\};", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S), flags=re.S).group(1)
    assert re.findall(r"\b(n_rec|n_bad|n_cooling|stamp_sum|stamp_min|stamp_max|q)\b(?:\[\d\])?[,;]", body) == list(want)
    di = cetkmc.engine.SOLID_INFO_DTYPE
    want_i = {"n_new": 0, "n_cleared": 8, "n_recorded": 16}
    assert {k: di.fields[k][1] for k in di.names} == want_i == {k: getattr(_lib.SolidInfo, k).offset for k in want_i}
    body = re.search(r"struct cetkmc_solid_info \{(.*?)\};", _header(), flags=re.S).group(1)
    assert re.findall(r"\b(n_new|n_cleared|n_recorded)\b[,;]", body) == list(want_i)
    assert _lib.SolidArgs.qscale.offset == 0 and C.sizeof(_lib.SolidArgs) == 32
    assert re.search(r"struct cetkmc_solid_args \{\s*double qscale\[4\];\s*\};", _header())
    scales = cetkmc.engine.default_solid_scales()
    assert len(scales) == 4 and all(np.isfinite(s) and s > 0 for s in scales)


def test_sources_and_null_handles():
    from cetkmc import _lib
    assert os.path.join(_lib.CSRC, "solid.hpp") in _lib.sources()
    lib = _lib.load()
    buf = np.zeros(4, dtype=np.dtype([("w", "<i8", 10)]))
    args = _lib.SolidArgs()
    args.qscale[:] = [1.0] * 4
    info = _lib.SolidInfo()
    calls = (lambda: lib.cetkmc_solid_begin(None), lambda: lib.cetkmc_solid_end(None),
             lambda: lib.cetkmc_solid_update(None, 0, 1.0, 1.0, C.addressof(info)),
             lambda: lib.cetkmc_solid_read(None, buf.ctypes.data, None, None, None),
             lambda: lib.cetkmc_solid_profile(None, C.byref(args), buf.ctypes.data, 0, None),
             lambda: lib.cetkmc_ensemble_solid_begin(None), lambda: lib.cetkmc_ensemble_solid_end(None),
             lambda: lib.cetkmc_ensemble_solid_update(None, 0, 1.0, 1.0, C.addressof(info)),
             lambda: lib.cetkmc_ensemble_solid_profile(None, C.byref(args), buf.ctypes.data, None))
    assert len(calls) == len(SYMBOLS)
    for call in calls:
        assert call() != 0 and b"null" in lib.cetkmc_last_error()
    assert not buf["w"].any() and (info.n_new, info.n_cleared, info.n_recorded) == (0, 0, 0)
