"""cetkmc_run_supersteps_local with one event per box and an infinite horizon IS cetkmc_run_supersteps without null events:
two engines, the logs compared slot by slot as bytes, totals, time increments, every field."""
import math

import numpy as np
import pytest

from helpers import random_lattice

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("L,fill,df", [(16, 0.2, 0.05), (32, 0.3, 0.1)])
def test_one_event_per_box_is_mode_b(L, fill, df):
    import cetkmc
    fields = random_lattice(L, 100 + L, fill=fill)
    a, b = cetkmc.Engine(L, impurity_c=0.2), cetkmc.Engine(L, impurity_c=0.2)
    a.upload(*fields)
    b.upload(*fields)
    step = 5
    for n in (19, 26):
        ra = a.run_supersteps_local(step, n, df, 4242, 1, math.inf, thermal_mode=1, want_events=True)
        rb = b.run_supersteps(step, n, 8, df, seed=4242, thermal_mode=1, want_events=True, null_events=False)
        assert ra["done"] == rb["done"] == n and ra["status"] == rb["status"] == 0
        assert ra["events"].shape == (n, (L // 8) ** 3, 1) and ra["domains"] == rb["domains"]
        assert np.ascontiguousarray(ra["events"][:, :, 0]).tobytes() == rb["events"].tobytes()
        for f in ("totals", "n_exec", "dt_event"):
            assert np.array_equal(ra[f], rb[f]), f
        assert np.array_equal(ra["n_capped"], rb["n_exec"]) and np.all(np.isinf(ra["horizon"]))
        assert ra["nucleation_count"] == rb["nucleation_count"]
        da, db = a.download(), b.download()
        for f in ("state", "theta", "phi", "T"):
            assert np.array_equal(da[f], db[f]), f
        step += n
    assert a.counters()["supersteps"] == b.counters()["supersteps"] == 45
    a.close()
    b.close()
