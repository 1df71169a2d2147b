"""cetkmc_shift's part of the C ABI without a device: the two symbols are declared, exported and
prototyped, cetkmc_shift (48 bytes) and cetkmc_shift_info (72 bytes) have one size in the library, in the ctypes mirrors and in
the header's list of names, the calls refuse null arguments by name without touching a device, the Python records are built as
the header lays them out, no row was added to the invalidation table, and nothing that existed changed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("cetkmc_shift", "cetkmc_ensemble_shift")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cetkmc.h")).read(), flags=re.S)


def test_symbols_and_struct_sizes():
    from cetkmc import _lib
    lib = _lib.load()
    code = _code()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert lib.cetkmc_struct_size(b"shift") == 48 == C.sizeof(_lib.Shift)
    assert lib.cetkmc_struct_size(b"shift_info") == 72 == C.sizeof(_lib.ShiftInfo)
    assert _lib.STRUCT_MIRRORS["shift"] is _lib.Shift and _lib.STRUCT_MIRRORS["shift_info"] is _lib.ShiftInfo
    header = open(os.path.join(ROOT, "include", "cetkmc.h")).read()
    names = re.search(r"sizeof of an ABI struct by name \((.*?)\)", header, flags=re.S).group(1)
    assert '"shift"' in names and '"shift_info"' in names
    body = re.search(r"struct cetkmc_shift \{(.*?)\};", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\d\])?\s*[,;]", body) == [n for n, _ in _lib.Shift._fields_] == \
        ["d", "fill_state", "T_mode", "pad", "fill_T", "fill_theta", "fill_phi"]
    body = re.search(r"struct cetkmc_shift_info \{(.*?)\};", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\d\])?\s*[,;]", body) == [n for n, _ in _lib.ShiftInfo._fields_] == ["calls", "kept", "exposed", "dropped"]
    assert re.search(r"enum\s*\{\s*CETKMC_SHIFT_T_VALUE\s*=\s*0\s*,\s*CETKMC_SHIFT_T_EDGE\s*=\s*1\s*\}", code)
    assert _lib.Shift.fill_T.offset == 24 and _lib.ShiftInfo.dropped.offset == 24
    assert lib.cetkmc_abi_version() == 1                       # purely additive
    for name, size in (("beam", 48), ("beam_info", 32), ("counters", C.sizeof(_lib.Counters))):        # existing structs, untouched
        assert lib.cetkmc_struct_size(name.encode()) == size


def test_null_arguments():
    from cetkmc import _lib
    lib = _lib.load()
    s, info = _lib.Shift(), _lib.ShiftInfo()
    for name in SYMBOLS:
        assert getattr(lib, name)(None, C.byref(s), C.byref(info)) != 0
        err = lib.cetkmc_last_error()
        assert b"null" in err and err.startswith(name.encode() + b":"), err
    assert (info.calls, info.kept, info.exposed, list(info.dropped)) == (0, 0, 0, [0] * 6)


def test_the_shift_is_an_upload_in_the_invalidation_table():
    """no cause of its own: the table keeps its rows, and the cause a shift raises is the upload's"""
    from cetkmc import _lib
    lib = _lib.load()
    assert lib.cetkmc_invalidates(b"shift") == -1
    assert lib.cetkmc_invalidates(b"upload_T_or_state") == 1 | 2 | 4 | 8       # SWEEP | TABLE | IFC | APPLIED, not STAGED


def test_python_records():
    from cetkmc import engine
    import constants as K
    s = engine._shift_struct((-3, 0, 7))
    assert (list(s.d), s.fill_state, s.T_mode, s.pad, s.fill_T, s.fill_theta, s.fill_phi) == ([-3, 0, 7], 0, 0, 0, float(K.T_SUB), 0.0, 0.0)
    s = engine._shift_struct((1, 2, 3), fill_state=4, fill_T=np.inf, T_mode="edge", fill_theta=-0.0, fill_phi=np.nan)
    assert (s.fill_state, s.T_mode, s.fill_T) == (4, 1, np.inf) and np.signbit(s.fill_theta) and np.isnan(s.fill_phi)
    assert engine._shift_struct((0, 0, 0), T_mode=7).T_mode == 7          # a number is the library's to judge
    with pytest.raises(KeyError):
        engine._shift_struct((0, 0, 0), T_mode="clamp")
    assert hasattr(engine.Engine, "shift") and hasattr(engine.Ensemble, "shift") and engine._Replica.shift is engine.Engine.shift
