"""thermal_solver.laser_scan_planes on the host: which global steps get a source plane, where the beam stands at each, and
that a plane depends on the global step alone (adjacent ranges concatenate).  No GPU."""
import numpy as np
import pytest

import thermal_solver as ts

LASER = dict(power=180.0, start=2.5, speed=0.75)


def _updates(first, n):
    return [g // 20 for g in range(first, first + n) if g % 20 == 0]


@pytest.mark.parametrize("first,n", [(0, 1), (0, 20), (0, 21), (1, 19), (1, 20), (7, 58), (20, 41), (39, 2), (40, 0), (137, 450)])
def test_one_plane_per_update_at_the_scan_position(first, n):
    L = 9
    q = ts.laser_scan_planes(L, LASER, first, n)
    us = _updates(first, n)
    assert q.shape == (len(us), L, L) and q.dtype == np.float64
    for x, u in enumerate(us):
        c = LASER["start"] + LASER["speed"] * u
        assert np.array_equal(q[x], ts.laser_source_plane(L, (c, c), LASER["power"])), (first, n, u)


def test_range_without_update_is_empty():
    for first, n in [(1, 19), (21, 5), (5, 0), (0, 0)]:
        q = ts.laser_scan_planes(6, LASER, first, n)
        assert q.shape == (0, 6, 6), (first, n)


@pytest.mark.parametrize("first,n1,n2", [(0, 20, 20), (0, 7, 53), (13, 7, 1), (19, 1, 1), (20, 1, 39), (3, 10, 5)])
def test_adjacent_ranges_concatenate(first, n1, n2):
    L = 7
    a, b = ts.laser_scan_planes(L, LASER, first, n1), ts.laser_scan_planes(L, LASER, first + n1, n2)
    assert np.array_equal(np.concatenate([a, b]), ts.laser_scan_planes(L, LASER, first, n1 + n2))


def test_optional_keys_and_defaults():
    L = 8
    z = dict(LASER, beam_radius=30e-6, absorptivity=0.5, latent=False)
    q = ts.laser_scan_planes(L, z, 20, 1)
    c = z["start"] + z["speed"]
    assert np.array_equal(q[0], ts.laser_source_plane(L, (c, c), z["power"], 30e-6, 0.5))
    d = ts.laser_scan_planes(L, LASER, 20, 1)
    assert np.array_equal(d[0], ts.laser_source_plane(L, (c, c), LASER["power"], ts.DEFAULT_BEAM_RADIUS, ts.DEFAULT_ABSORPTIVITY))
    assert not np.array_equal(q, d)
