"""Every refusal of the 24 diagnostic entry points (front stats, layer / texture profile, grain table, solidification map,
origin map; single lattice and ensemble) that can be provoked without launching a diagnostic kernel, each against the exact
cetkmc_last_error text.  All of them return on the host before any launch."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L, R = 8, 2
NULL = "null argument"
NULL_HANDLE = "null handle"
NOT_ENS = "not an ensemble handle (cetkmc_create_ensemble)"


def one_lattice(fn):
    return f"cetkmc_{fn} takes one lattice: an ensemble handle goes to cetkmc_ensemble_{fn}"


def single_handle(fn, family):
    return f"cetkmc_{fn} takes a single-lattice handle: an ensemble's maps are kept by cetkmc_ensemble_{family}_*"


def one_slab(fn):
    return f"cetkmc_{fn} needs the whole lattice in one slab"


def no_cluster(fn):
    return f"cetkmc_{fn} needs a preceding cetkmc_cluster"


def no_analysis(fn):
    return f"cetkmc_ensemble_{fn} needs a preceding cetkmc_ensemble_analyze"


def no_map(fn, family):
    return f"cetkmc_{fn} needs a map (cetkmc_{family}_begin)"


def no_maps(fn, family):
    return f"cetkmc_ensemble_{fn} needs the maps (cetkmc_ensemble_{family}_begin)"


@pytest.fixture(scope="module")
def handles():
    import cetkmc
    eng = cetkmc.Engine(L, impurity_c=0.2)
    two = cetkmc.Engine(L, impurity_c=0.2, n_slabs=2)
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.2)] * R)
    yield dict(lib=eng.lib, E=eng.h, S=two.h, X=ens.h, P=ens.replica(1).h, N=None)
    ens.close()
    two.close()
    eng.close()


def _buf(n=4096):
    return np.zeros(n, np.int64).ctypes.data_as(C.c_void_p)


def _refused(hs, name, want, who, *args):
    lib = hs["lib"]
    rc = getattr(lib, "cetkmc_" + name)(hs[who], *args)
    got = lib.cetkmc_last_error().decode()
    assert rc != 0 and got == want, (name, who, rc, got, want)


def test_front_stats(handles):
    out = _buf()
    _refused(handles, "front_stats", NULL, "N", 1.0, out)
    _refused(handles, "front_stats", NULL, "E", 1.0, None)
    _refused(handles, "front_stats", one_slab("front_stats"), "S", 1.0, out)
    _refused(handles, "ensemble_front_stats", NULL, "N", 1.0, out)
    _refused(handles, "ensemble_front_stats", NULL, "X", 1.0, None)
    _refused(handles, "ensemble_front_stats", NOT_ENS, "E", 1.0, out)
    _refused(handles, "ensemble_front_stats", NOT_ENS, "P", 1.0, out)


def test_layer_profile(handles):
    out = _buf()
    _refused(handles, "layer_profile", NULL, "N", 2.0, out)
    _refused(handles, "layer_profile", NULL, "E", 2.0, None)
    _refused(handles, "layer_profile", one_lattice("layer_profile"), "X", 2.0, out)
    _refused(handles, "layer_profile", one_slab("layer_profile"), "S", 2.0, out)
    _refused(handles, "layer_profile", no_cluster("layer_profile"), "E", 2.0, out)
    _refused(handles, "layer_profile", no_cluster("layer_profile"), "P", 2.0, out)      # a replica is one lattice
    _refused(handles, "ensemble_layer_profile", NULL, "N", 2.0, out)
    _refused(handles, "ensemble_layer_profile", NULL, "X", 2.0, None)
    _refused(handles, "ensemble_layer_profile", NOT_ENS, "E", 2.0, out)
    _refused(handles, "ensemble_layer_profile", NOT_ENS, "P", 2.0, out)
    _refused(handles, "ensemble_layer_profile", no_analysis("layer_profile"), "X", 2.0, out)


def test_texture_profile(handles):
    from cetkmc import _lib
    a = _lib.TextureArgs()          # n_bins 0: refused only behind the clustering check
    gb, pole, bad = _buf(), _buf(), _buf()
    _refused(handles, "texture_profile", NULL, "N", C.byref(a), gb, pole, bad)
    _refused(handles, "texture_profile", NULL, "E", None, gb, pole, bad)
    _refused(handles, "texture_profile", one_lattice("texture_profile"), "X", C.byref(a), gb, pole, bad)
    _refused(handles, "texture_profile", one_slab("texture_profile"), "S", C.byref(a), gb, pole, bad)
    _refused(handles, "texture_profile", no_cluster("texture_profile"), "E", C.byref(a), gb, pole, bad)
    _refused(handles, "texture_profile", no_cluster("texture_profile"), "P", C.byref(a), gb, pole, bad)
    _refused(handles, "ensemble_texture_profile", NULL, "N", C.byref(a), gb, pole, bad)
    _refused(handles, "ensemble_texture_profile", NULL, "X", None, gb, pole, bad)
    _refused(handles, "ensemble_texture_profile", NOT_ENS, "E", C.byref(a), gb, pole, bad)
    _refused(handles, "ensemble_texture_profile", NOT_ENS, "P", C.byref(a), gb, pole, bad)
    _refused(handles, "ensemble_texture_profile", no_analysis("texture_profile"), "X", C.byref(a), gb, pole, bad)


def test_grain_table(handles):
    out = _buf()
    _refused(handles, "grain_table", NULL_HANDLE, "N", 4, out)
    _refused(handles, "grain_table", one_lattice("grain_table"), "X", 4, out)
    _refused(handles, "grain_table", one_slab("grain_table"), "S", 4, out)
    _refused(handles, "grain_table", no_cluster("grain_table"), "E", 4, out)
    _refused(handles, "grain_table", no_cluster("grain_table"), "E", 4, None)       # the clustering is asked for first
    _refused(handles, "grain_table", no_cluster("grain_table"), "P", 4, out)
    _refused(handles, "ensemble_grain_table", NULL, "N", out)
    _refused(handles, "ensemble_grain_table", NOT_ENS, "E", out)
    _refused(handles, "ensemble_grain_table", NOT_ENS, "P", out)
    _refused(handles, "ensemble_grain_table", no_analysis("grain_table"), "X", out)
    _refused(handles, "ensemble_grain_table", no_analysis("grain_table"), "X", None)


def test_solid_map(handles):
    from cetkmc import _lib
    a = _lib.SolidArgs()
    a.qscale[:] = [1.0] * 4
    info, lay, gr = _buf(), _buf(), _buf()
    for fn in ("solid_begin", "solid_end"):
        _refused(handles, fn, NULL_HANDLE, "N")
        _refused(handles, fn, single_handle(fn, "solid"), "X")
        _refused(handles, fn, single_handle(fn, "solid"), "P")
        _refused(handles, fn, one_slab(fn), "S")
    _refused(handles, "solid_end", no_map("solid_end", "solid"), "E")
    _refused(handles, "solid_update", NULL_HANDLE, "N", 0, 1.0, 1e-6, info)
    _refused(handles, "solid_update", single_handle("solid_update", "solid"), "X", 0, 1.0, 1e-6, info)
    _refused(handles, "solid_update", single_handle("solid_update", "solid"), "P", 0, 1.0, 1e-6, info)
    _refused(handles, "solid_update", one_slab("solid_update"), "S", 0, 1.0, 1e-6, info)
    _refused(handles, "solid_update", no_map("solid_update", "solid"), "E", 0, 1.0, 1e-6, info)
    _refused(handles, "solid_update", no_map("solid_update", "solid"), "E", -1, 1.0, 0.0, info)    # the map is asked for first
    _refused(handles, "solid_profile", NULL, "N", C.byref(a), lay, 0, None)
    _refused(handles, "solid_profile", NULL, "E", None, lay, 0, None)
    _refused(handles, "solid_profile", NULL, "E", C.byref(a), None, 0, None)
    _refused(handles, "solid_profile", one_lattice("solid_profile"), "X", C.byref(a), lay, 0, None)
    _refused(handles, "solid_profile", one_slab("solid_profile"), "S", C.byref(a), lay, 0, None)
    _refused(handles, "solid_profile", no_map("solid_profile", "solid"), "E", C.byref(a), lay, 4, gr)
    _refused(handles, "solid_profile", no_map("solid_profile", "solid"), "P", C.byref(a), lay, 0, None)
    for fn, args in (("solid_begin", ()), ("solid_end", ()), ("solid_update", (0, 1.0, 1e-6, info)),
                     ("solid_profile", (C.byref(a), lay, gr))):
        _refused(handles, "ensemble_" + fn, NULL, "N", *args)
        _refused(handles, "ensemble_" + fn, NOT_ENS, "E", *args)
        _refused(handles, "ensemble_" + fn, NOT_ENS, "P", *args)
        if fn != "solid_begin":
            _refused(handles, "ensemble_" + fn, no_maps(fn, "solid"), "X", *args)
    _refused(handles, "ensemble_solid_profile", no_maps("solid_profile", "solid"), "X", None, None, None)    # the maps first
    _refused(handles, "ensemble_solid_update", no_maps("solid_update", "solid"), "X", -1, 1.0, 0.0, info)


def test_origin_map_without_a_map(handles):
    out, lay, gr = _buf(), _buf(), _buf()
    for fn in ("origin_begin", "origin_end"):
        _refused(handles, fn, NULL_HANDLE, "N")
        _refused(handles, fn, single_handle(fn, "origin"), "X")
        _refused(handles, fn, single_handle(fn, "origin"), "P")
        _refused(handles, fn, one_slab(fn), "S")
    _refused(handles, "origin_end", no_map("origin_end", "origin"), "E")
    _refused(handles, "origin_census", NULL, "N", out)
    _refused(handles, "origin_census", NULL, "E", None)
    _refused(handles, "origin_census", one_slab("origin_census"), "S", out)
    for who in ("E", "X", "P"):       # any lattice handle may be asked; none has a map
        _refused(handles, "origin_census", no_map("origin_census", "origin"), who, out)
    _refused(handles, "origin_profile", NULL, "N", lay, 0, None)
    _refused(handles, "origin_profile", NULL, "E", None, 0, None)
    _refused(handles, "origin_profile", one_lattice("origin_profile"), "X", lay, 0, None)
    _refused(handles, "origin_profile", one_slab("origin_profile"), "S", lay, 0, None)
    _refused(handles, "origin_profile", no_map("origin_profile", "origin"), "E", lay, 4, gr)
    _refused(handles, "origin_profile", no_map("origin_profile", "origin"), "P", lay, 0, None)
    for fn, args in (("origin_begin", ()), ("origin_end", ()), ("origin_census", (out,)), ("origin_profile", (lay, gr))):
        _refused(handles, "ensemble_" + fn, NULL, "N", *args)
        _refused(handles, "ensemble_" + fn, NOT_ENS, "E", *args)
        _refused(handles, "ensemble_" + fn, NOT_ENS, "P", *args)
        if fn != "origin_begin":
            _refused(handles, "ensemble_" + fn, no_maps(fn, "origin"), "X", *args)
    _refused(handles, "ensemble_origin_census", no_maps("origin_census", "origin"), "X", None)              # the maps first
    _refused(handles, "ensemble_origin_profile", no_maps("origin_profile", "origin"), "X", None, None)


def test_origin_map_with_a_map(handles):
    """cetkmc_origin_begin issues a memset and a copy, no kernel: with a map in place the calls get as far as their outputs
    and the grain records' clustering."""
    lib, lay, gr = handles["lib"], _buf(), _buf()
    assert lib.cetkmc_origin_begin(handles["E"]) == 0, lib.cetkmc_last_error()
    assert lib.cetkmc_ensemble_origin_begin(handles["X"]) == 0, lib.cetkmc_last_error()
    try:
        _refused(handles, "origin_census", NULL, "E", None)
        _refused(handles, "origin_profile", NULL, "E", None, 0, None)
        _refused(handles, "origin_profile", no_cluster("origin_profile") + " for its grain records", "E", lay, 4, gr)
        _refused(handles, "origin_profile", no_cluster("origin_profile") + " for its grain records", "P", lay, 4, gr)
        _refused(handles, "origin_profile", one_lattice("origin_profile"), "X", lay, 4, gr)
        _refused(handles, "ensemble_origin_census", NULL, "X", None)
        _refused(handles, "ensemble_origin_profile", NULL, "X", None, gr)
        _refused(handles, "ensemble_origin_profile", no_analysis("origin_profile") + " for its grain records", "X", lay, gr)
        _refused(handles, "origin_begin", single_handle("origin_begin", "origin"), "P")
    finally:
        assert lib.cetkmc_origin_end(handles["E"]) == 0, lib.cetkmc_last_error()
        assert lib.cetkmc_ensemble_origin_end(handles["X"]) == 0, lib.cetkmc_last_error()
    _refused(handles, "origin_end", no_map("origin_end", "origin"), "E")
    _refused(handles, "ensemble_origin_end", no_maps("origin_end", "origin"), "X")
