"""The host layer's cache state: which cause makes which cache stale, on the CPU.

Between calls a handle keeps the row and block sums of the last sweep (SWEEP), the rate table (TABLE), the listed voxels'
sums (IFC), the marker of a temperature update that a stopped batch already applied (APPLIED) and a staged batch (STAGED).
csrc/cetkmc_hip.hip holds one table of what every cause makes stale, read by the one function that clears the flags and
exported as cetkmc_invalidates().  ``TABLE`` below restates it by hand, from the behaviour of the library before that table
existed; tests/test_gpu_invalidation_counts.py checks the same rows against what a live handle does."""
import re

import pytest

import live_ops as lo

SWEEP, TABLE_, IFC, APPLIED, STAGED = 1, 2, 4, 8, 16
BITS = dict(SWEEP=SWEEP, TABLE=TABLE_, IFC=IFC, APPLIED=APPLIED, STAGED=STAGED)

# cause -> caches made stale
TABLE = {
    "upload": SWEEP | IFC | APPLIED,                           # any field: theta / phi only and defects only as well
    "upload_T_or_state": SWEEP | TABLE_ | IFC | APPLIED,
    "set_params": SWEEP | TABLE_ | IFC,
    "option_sweep_variant": SWEEP | TABLE_ | IFC,
    "option_interface_every_step": IFC,
    "option_reserve_batch": STAGED,                            # the batch buffers may move
    "set_defects": SWEEP | IFC,                                # dense, sparse, an ensemble replica with counts[r] >= 0
    "set_prev_state_null": IFC,                                # the list is re-ordered
    "set_prev_state_array": 0,
    "apply": SWEEP | IFC,
    "thermal_update": SWEEP | TABLE_ | APPLIED,                # the update did not write the table
    "thermal_update_wrote_table": SWEEP | IFC | APPLIED,
    "lookahead_adopted": SWEEP | IFC,                          # the adopted field came with its table
    "step": SWEEP,
    "step_no_upkeep": SWEEP | IFC,                             # a batched step without touched-voxel upkeep
    "batch_stopped": SWEEP | TABLE_ | IFC,                     # status != 0, Mode A and Mode B
    "ensemble_stepped": SWEEP | TABLE_ | IFC | APPLIED,
    "batch_begin": STAGED,                                     # run_steps, run_supersteps, stage_inputs
    "table_written": IFC,                                      # the table launch overwrites the listed voxels' entries
    "marker_taken": APPLIED,                                   # run_steps hands the marker to its batch
}


def cause_of(mutator):
    """The cause a mutator of tests/live_ops.py raises, by its class; an option that no cache depends on raises none."""
    cls = lo.MUTATORS.get(mutator) or lo.MUTATORS2[mutator]
    if cls == "setting":         # cetkmc_set_remelt, cetkmc_set_thermal_substeps: later stepping calls change, no cache does
        return None
    if cls in ("remelt", "remelt_noop"):       # a direct pass, also one that melts nothing (threshold +inf) and the timed ones
        return "apply"
    if cls == "timed_thermal":   # cetkmc_time_thermal applies real updates
        return "thermal_update"
    if cls == "upload":
        return "upload" if mutator in ("upload_orient", "upload_defects") else "upload_T_or_state"
    if cls == "options":
        key = re.fullmatch(r"opt_(\w+)=-?\d+", mutator).group(1)
        return "option_" + key if key in ("sweep_variant", "interface_every_step", "reserve_batch") else None
    if cls == "prev":
        return "set_prev_state_null" if mutator == "set_prev_state_none" else "set_prev_state_array"
    return dict(defects="set_defects", thermal="thermal_update", apply="apply", staged="batch_begin", params="set_params")[cls]


def _lib():
    from cetkmc import _lib
    _lib.build_library()
    return _lib.load()


def test_bits_are_the_headers():
    from conftest import ROOT
    src = open(f"{ROOT}/include/cetkmc.h").read()
    for name, bit in BITS.items():
        m = re.search(rf"\bCETKMC_CACHE_{name}\s*=\s*(\d+)", src)
        assert m and int(m.group(1)) == bit, name


@pytest.mark.parametrize("cause", sorted(TABLE))
def test_cause_invalidates_what_the_table_says(cause):
    got = _lib().cetkmc_invalidates(cause.encode())
    names = lambda m: sorted(n for n, b in BITS.items() if m & b)
    assert got == TABLE[cause], (cause, "library", names(got) if got >= 0 else got, "table", names(TABLE[cause]))


def test_unknown_cause():
    lib = _lib()
    for name in (b"", b"no_such_cause", b"Upload", b"upload ", b"step_"):
        assert lib.cetkmc_invalidates(name) == -1, name
    assert lib.cetkmc_invalidates(None) == -1


def test_library_has_no_cause_the_table_lacks():
    """every cause of the library's table is one of the rows above: its names are read from the source, beside the table"""
    from conftest import PKG
    src = open(f"{PKG}/csrc/cetkmc_hip.hip").read()
    body = re.search(r"constexpr\s+CauseRow\s+INVALIDATES\[\]\s*=\s*\{(.*?)\n\};", src, re.S)
    assert body, "INVALIDATES[] not found in csrc/cetkmc_hip.hip"
    names = re.findall(r'\{\s*Cause::\w+\s*,\s*"(\w+)"', body.group(1))
    assert sorted(names) == sorted(TABLE), set(names) ^ set(TABLE)


def test_every_mutator_has_a_cause():
    """a mutator of a class this test does not know raises KeyError in cause_of(): no new mutator without a row"""
    lib = _lib()
    seen = set()
    classes = dict(lo.MUTATORS, **lo.MUTATORS2)
    for m in classes:
        c = cause_of(m)
        if c is None:
            assert classes[m] in ("options", "setting"), m
            continue
        assert c in TABLE and lib.cetkmc_invalidates(c.encode()) >= 0, (m, c)
        seen.add(classes[m])
    assert seen == set(classes.values()) - {"setting"}, set(classes.values()) - seen
