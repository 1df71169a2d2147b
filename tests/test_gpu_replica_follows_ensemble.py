"""A direct temperature update on a replica handle follows the ensemble's settings: the ensemble walks through sub-steps, the
implicit scheme, a thermal boundary and back; after every setting one ``thermal_laser`` on replicas 0 and 2 and on two single
handles that hold the same lattices and were set the same directly.  L = 9 (odd, below every tile width; 81 rows: one full and
one partial block of k_imp_rows), R = 3, lattices with a NaN, a +inf and blocks outside the clip range.  The replicas' fields and
replica 2's three info records equal the twins'; the ensemble handle's own records stay zero (no ``run`` is made)."""
import numpy as np
import pytest

import boundary_cases as bc
import implicit_cases as ic
from oracle import oracle

pytestmark = pytest.mark.gpu

L, R = 9, 3
IMPURITY_C = 0.1
CASE = dict(ic.ENSEMBLE["ens_L33_n3"], L=L)
# (setter, value) in order; the state after each: (substeps, scheme, boundary)
SETTINGS = (
    (("set_thermal_substeps", 3),),                                             # substeps 3, explicit
    (("set_thermal_scheme", "implicit"),),                                      # substeps 3, implicit
    (("set_thermal_boundary", bc.ENS_BC),),                                     # implicit with a boundary
    (("set_thermal_boundary", None),),                                          # boundary cleared
    (("set_thermal_scheme", "explicit"), ("set_thermal_substeps", 1)),          # explicit, substeps 1
)
INFOS = ("substep_info", "implicit_info", "boundary_info")


def test_direct_update_on_a_replica_follows_the_ensemble():
    import cetkmc
    q = oracle.laser_source_plane(L, (L - 1, 0), ic.POWER)
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(IMPURITY_C) for _ in range(R)])
    twins = {r: cetkmc.Engine(L, impurity_c=IMPURITY_C) for r in (0, 2)}
    try:
        for r in range(R):
            lat = ic.lattice_of(CASE, r)
            assert np.isnan(lat[3]).any() and np.isinf(lat[3]).any()
            ens.replica(r).upload(*lat)
            if r in twins:
                twins[r].upload(*lat)
        for k, calls in enumerate(SETTINGS):
            for name, value in calls:
                for h in (ens, *twins.values()):
                    getattr(h, name)(value)
            for r, twin in twins.items():
                rep = ens.replica(r)
                for h in (rep, twin):
                    h.thermal_laser(1e-6, q, use_latent=True, scrub_nan=True)
                a, b = rep.download(defects=True), twin.download(defects=True)
                for f in ("T", "state", "defects"):
                    assert a[f].tobytes() == b[f].tobytes(), (k, r, f)
            for info in INFOS:
                assert getattr(ens.replica(2), info)() == getattr(twins[2], info)(), (k, info)
        # every kind of update was counted on the twin: the equalities above compared live counters
        assert twins[2].substep_info()["updates"] == 1 and twins[2].implicit_info()["updates"] == 3
        assert twins[2].boundary_info()["updates"] == 1
        for info in INFOS:
            rec = getattr(ens, info)()
            assert rec and not any(rec.values()), (info, rec)
    finally:
        for e in twins.values():
            e.close()
        ens.close()
