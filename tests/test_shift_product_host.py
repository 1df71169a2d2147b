"""run_kmc's ``build`` option (layer-by-layer builds): everything that is refused is refused with a
ValueError before an engine exists -- no GPU here, so a call that got as far as creating one would raise RuntimeError -- and the
per-layer beam tables and the rows of build_layers.csv are what the docstring says.  No GPU."""
import numpy as np
import pytest


def _run(**kw):
    import kmc_simulation
    base = dict(L=16, n_steps=40, output_prefix="shift_product_host", build=dict(layers=3, thickness=4))
    base.update(kw)
    return kmc_simulation.run_kmc(**base)


@pytest.mark.parametrize("kw,match", [
    (dict(mode="B"), "build needs mode 'A'"),
    (dict(checkpoint_every=20), "checkpoint does not carry the layer state"),
    (dict(resume_from="no_such_checkpoint.npz"), "checkpoint does not carry the layer state"),
    (dict(build=dict(layers=3, thickness=0)), r"thickness must lie in 1 \.\. L - 1"),
    (dict(build=dict(layers=3, thickness=16)), r"thickness must lie in 1 \.\. L - 1"),
    (dict(build=dict(layers=0, thickness=4)), "layers must be >= 1"),
    (dict(build=dict(layers=-2, thickness=4)), "layers must be >= 1"),
    (dict(n_steps=30), "positive multiple of 20"),
    (dict(n_steps=0), "positive multiple of 20"),
    (dict(n_steps=-20), "positive multiple of 20"),
    (dict(build=dict(layers=3)), "keys layers, thickness"),
    (dict(build=dict(layers=3, thickness=4, height=1)), "keys layers, thickness"),
    (dict(build=(3, 4)), "keys layers, thickness"),
    (dict(build=dict(layers=3, thickness=4, state=5)), r"state must lie in 0 \.\. 4"),
])
def test_refused_before_an_engine_exists(kw, match, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match=match):
        _run(**kw)
    assert not (tmp_path / "outputs").exists()            # ... and before anything is written


def test_checked_copy_and_defaults():
    import constants
    import kmc_simulation as ks
    assert ks._check_build(None, 16, 7, "B", True) is None          # no build: nothing of it is looked at
    b = ks._check_build(dict(layers=2, thickness=15), 16, 20, "A", False)
    assert b == dict(layers=2, thickness=15, T=float(constants.T_SUB), state=0)
    b = ks._check_build(dict(layers=1, thickness=1, T=3000, state=1), 16, 400, "A", False)
    assert b == dict(layers=1, thickness=1, T=3000.0, state=1)


def test_beam_table_of_a_layer_scans_the_path_from_its_beginning():
    import kmc_simulation as ks
    L, per = 24, 60                                         # U = 3 updates per layer
    laser = ks.beam_laser(80.0, "serpentine", 4.0, hatch=5.0, depth=2)
    t0 = ks._beam_table_of_layer(laser, L, 0, per)
    t2 = ks._beam_table_of_layer(laser, L, 2, per)
    assert (t0["u0"], t2["u0"]) == (0, 6) and t0["amp"].shape == t2["amp"].shape == (3,)
    for k in ("amp", "gj", "gk", "fi"):
        assert np.array_equal(t0[k], t2[k]), k
    whole = ks._beam_table_of(laser, L, per)                # without a build: the table of a run of that many steps
    for k in ("amp", "gj", "gk", "fi"):
        assert np.array_equal(t0[k], whole[k]), k
    assert whole["u0"] == 0


def test_retired_plane_rows():
    import kmc_simulation as ks
    L = 5
    tables = dict(layer={"plane": np.arange(L), "n_occ": np.arange(L) * 10}, origin={"Step": np.full(L, 39), "plane": np.arange(L), "n_occ": np.arange(L) + 100})
    rows = ks._retired_planes(tables, 2, 1, 2)
    assert rows == [dict(Layer=1, BuildHeight=2, Plane=0, layer_n_occ=0, origin_Step=39, origin_n_occ=100),
                    dict(Layer=1, BuildHeight=3, Plane=1, layer_n_occ=10, origin_Step=39, origin_n_occ=101)]
    rows = ks._retired_planes(tables, L, 2, 4)
    assert [r["BuildHeight"] for r in rows] == [4, 5, 6, 7, 8] and rows[-1]["layer_n_occ"] == 40
