"""The stale-row rule (dirty_offset() in csrc/kernels.hpp, exported as cetkmc_dirty_offset) against the oracle, on the CPU.

The apply block of a sweep launch re-evaluates exactly the rows the rule names around each changed voxel while the
launch's tiles read the lattice beside it; the incremental mode's dirty list is built from the same rule.  A row the rule
missed would hold sums from before OR after the event depending on timing, so a GPU on/off comparison can pass by luck.
Here every single-voxel change is made on the oracle and the rows whose sums changed are compared with the rule."""
import os
import re

import numpy as np
import pytest

from conftest import PKG
from helpers import random_lattice


def _rule():
    from cetkmc import _lib
    _lib.build_library()
    lib = _lib.load()
    return lambda di, dj: bool(lib.cetkmc_dirty_offset(int(di), int(dj)))


def _patch_max():
    src = open(os.path.join(PKG, "csrc", "kernels.hpp")).read()
    m = re.search(r"constexpr\s+int\s+PATCH_MAX\s*=\s*(\d+)\s*;", src)
    assert m, "PATCH_MAX not found in csrc/kernels.hpp"
    return int(m.group(1))


def _sites(L, rs):
    corners = [(i, j, k) for i in (0, L - 1) for j in (0, L - 1) for k in (0, L - 1)]
    edges = [(0, 0, L // 2), (L - 1, L // 2, 0), (L // 2, L - 1, L - 1), (L // 2, 0, L // 2), (0, L // 2, L // 2),
             (L // 2, L // 2, L - 1)]
    rnd = [tuple(int(x) for x in rs.randint(0, L, 3)) for _ in range(30)]
    return corners + edges + rnd


def _changed_rows(before, after):
    """(plane, row) of every (plane, category, row) whose sum or count differs (a NaN that stays a NaN is no change)"""
    (s0, c0), (s1, c1) = before, after
    ch = (c0 != c1) | ~((s0 == s1) | (np.isnan(s0) & np.isnan(s1)))
    return {(int(i), int(j)) for i, _, j in np.argwhere(ch)}


@pytest.mark.parametrize("L,seed", [(7, 3), (10, 4)])
def test_changed_rows_lie_in_the_rules_footprint(oracle_mod, L, seed):
    """Change one voxel to each other state (new orientation, defect flag flipped): every row whose sums change sits at an
    offset the exported rule accepts; over all changes the offsets that did change are exactly the rule's set in
    [-2, 2]^2, and that set fits PATCH_MAX / 2 rows per changed site."""
    rule = _rule()
    accepted = {(di, dj) for di in range(-2, 3) for dj in range(-2, 3) if rule(di, dj)}
    # nothing outside [-2, 2]^2 (the apply block and the dirty list scan only that window)
    assert not any(rule(di, dj) for di in range(-4, 5) for dj in range(-4, 5) if max(abs(di), abs(dj)) > 2)
    patch_max = _patch_max()
    assert patch_max % 2 == 0 and len(accepted) <= patch_max // 2, (sorted(accepted), patch_max)

    rs = np.random.RandomState(100 + seed)
    state, theta, phi, T, defects = random_lattice(L, seed, fill=0.4)
    lat = oracle_mod.Lattice(state, theta, phi, T, defects, impurity_c=0.2)
    seen, n_changes = set(), 0
    for (i, j, k) in _sites(L, rs):
        old = (lat.state[i, j, k], lat.theta[i, j, k], lat.phi[i, j, k], lat.defects[i, j, k])
        base = tuple(a.copy() for a in lat.row_sums())
        for new_state in range(5):
            if new_state == old[0]:
                continue
            lat.state[i, j, k] = new_state
            oriented = new_state in (1, 2, 3)
            lat.theta[i, j, k] = rs.uniform(0, np.pi) if oriented else 0.0
            lat.phi[i, j, k] = rs.uniform(0, 2 * np.pi) if oriented else 0.0
            lat.defects[i, j, k] = 1 - old[3]
            rows = _changed_rows(base, lat.row_sums())
            n_changes += 1
            for (pi, pj) in rows:
                off = (pi - i, pj - j)
                assert max(abs(off[0]), abs(off[1])) <= 2 and rule(*off), \
                    f"voxel {(i, j, k)} {old[0]} -> {new_state}: row (plane {pi}, row {pj}) changed, offset {off} is not in the rule"
                seen.add(off)
        lat.state[i, j, k], lat.theta[i, j, k], lat.phi[i, j, k], lat.defects[i, j, k] = old
        again = lat.row_sums()
        assert not _changed_rows(base, again)          # restored: the next site starts from the same lattice
    assert n_changes >= 4 * 40
    assert seen == accepted, f"accepted but never changed: {sorted(accepted - seen)}; changed but not accepted: {sorted(seen - accepted)}"


def test_rule_is_symmetric_and_names_11_offsets():
    """The apply block de-duplicates the second site's rows with dirty_offset(gi - i0, j - j0): that is only the same
    set as 'a row of the first site' if the rule is symmetric under (di, dj) -> (-di, -dj)."""
    rule = _rule()
    acc = {(di, dj) for di in range(-2, 3) for dj in range(-2, 3) if rule(di, dj)}
    assert acc == {(-di, -dj) for di, dj in acc}
    assert (0, 0) in acc and len(acc) == 11
