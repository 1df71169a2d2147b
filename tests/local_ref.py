"""Comparator of Mode B's local event loop (include/cetkmc.h, cetkmc_run_supersteps_local).

Built on oracle.Lattice primitives only (window_pick, apply, sweep, thermal_cet, counter_uniform) and tests/helpers.dep_species;
it never touches the engine.  Per super-step g: temperature update and sweep as Lattice.run_supersteps; every box's first
pick on the frozen lattice; R_max over the non-idle boxes, horizon tau = horizon_events / R_max; then box after box (their
windows are independent) the local loop: waiting time w = -ln(u) / R, stop when t + w > tau or after max_events events,
apply, pick again on the lattice as the box's own events left it.

    run(lat, step0, n, defect_fraction, seed, max_events, horizon_events, thermal_mode=1, thermal_dt=1e-6)

returns the logs of the call plus what the run exercised (``stats``)."""
import math

import numpy as np

from helpers import dep_species

EVENT = np.dtype([("type", "<i4"), ("pos", "<i4", 3), ("target", "<i4", 3), ("atom", "<i4"), ("rate", "<f8"),
                  ("dep_rank", "<i8"), ("theta", "<f8"), ("phi", "<f8")], align=True)
assert EVENT.itemsize == 64
KEY_PICK, KEY_THETA, KEY_PHI, KEY_DEFECT, KEY_ACCEPT, KEY_DT, KEY_WAIT = (q << 40 for q in range(1, 8))
BOX, H = 8, 4
STOPS = ("idle", "horizon", "capped", "emptied")


# The inputs of the GPU comparison (tests/test_gpu_local_vs_ref.py), whose coverage tests/test_local_ref_host.py asserts on
# the comparator alone: name -> (L, random_lattice seed, random_lattice keywords, horizon_events, max_events, parameter
# tweak, thermal_mode, defect_fraction).  The first five are the table of the definition's coverage conditions.
INPUTS = {
    "L16": (16, 116, dict(fill=0.2), 1.0, 4, None, 1, 0.05),
    "L16_four_kinds": (16, 118, dict(fill=0.2), 4.0, 8, "FOUR_KIND_PARAMS", 1, 0.1),
    "L24_sparse": (24, 124, dict(fill=0.02), 4.0, 4, "FOUR_KIND_PARAMS", 0, 0.02),
    "L16_top": (16, 216, dict(fill=0.3, hot_frac=0.0), 8.0, 8, "FOUR_KIND_PARAMS", 1, 0.0),
    "L32_top": (32, 132, dict(fill=0.3, hot_frac=0.0), 4.0, 8, "FOUR_KIND_PARAMS", 0, 0.05),
    "L8": (8, 101, dict(fill=0.1), 4.0, 6, "FOUR_KIND_PARAMS", 1, 0.05),
    "L40": (40, 140, dict(fill=0.1), 2.0, 4, None, 1, 0.02),
    # no horizon: every box runs to the cap or empties its window.  With the cap at the window's 64 voxels the lattice is
    # full after 12 super-steps (the batch ends with status 1 and the second batch is empty: that stop is what the input
    # compares); with the cap at 8 the run lasts through both batches, the second starting mid-cadence and mid-octant.
    "L16_to_the_cap": (16, 116, dict(fill=0.2), float("inf"), 64, "FOUR_KIND_PARAMS", 1, 0.05),
    "L16_no_horizon": (16, 116, dict(fill=0.2), float("inf"), 8, "FOUR_KIND_PARAMS", 1, 0.05),
}
TABLE = ("L16", "L16_four_kinds", "L24_sparse", "L16_top", "L32_top")
NO_HORIZON = ("L16_to_the_cap", "L16_no_horizon")      # the horizon stop cannot occur there
BATCHES = (19, 26)          # from super-step 5: the second batch starts mid-cadence and mid-octant
STEP0 = 5
SEED = 4242
IMPURITY_C = 0.2


def make_input_fields(name):
    """(fields, L, tweak dict) of an input."""
    import helpers
    L, seed, kw, _, _, tweak, _, _ = INPUTS[name]
    return helpers.random_lattice(L, seed, **kw), L, (dict(getattr(helpers, tweak)) if tweak else {})


def make_input(oracle_mod, name):
    """(fields, oracle lattice, tweak dict) of an input."""
    fields, _, tw = make_input_fields(name)
    lat = oracle_mod.Lattice(*fields, impurity_c=IMPURITY_C)
    for k, v in tw.items():
        setattr(lat.params, k, v)
    return fields, lat, tw


_RUNS = {}


def reference_run(oracle_mod, name):
    """The comparator's two batches on an input, computed once per process and shared (callers must not change it): a list
    of (result, state, theta, phi, T, nuc_count) after each batch."""
    if name not in _RUNS:
        _, _, _, hor, K, _, tm, df = INPUTS[name]
        _, lat, _ = make_input(oracle_mod, name)
        out, step = [], STEP0
        for n in BATCHES:
            r = run(oracle_mod, lat, step, n, df, SEED, K, hor, thermal_mode=tm)
            out.append((r, lat.state.copy(), lat.theta.copy(), lat.phi.copy(), lat.T.copy(), lat.nuc_count))
            step += n
        _RUNS[name] = out
    return _RUNS[name]


def window_origin(L, g, d):
    nb = L // BOX
    sec = g % 8
    di, dj, dk = d // (nb * nb), (d // nb) % nb, d % nb
    return di * BOX + ((sec >> 2) & 1) * H, dj * BOX + ((sec >> 1) & 1) * H, dk * BOX + (sec & 1) * H


def keys(m, d, j, k, L):
    """The uniform keys of event m of box d (deposition at column (j, k)): for m = 0 they are Mode B's."""
    md = (m << 24) | d
    return dict(wait=KEY_WAIT | md, pick=KEY_PICK | md, theta=KEY_THETA | md, phi=KEY_PHI | md, defect=KEY_DEFECT | md,
                species=(m << 44) | (j * L + k))


def _empty_log(shape):
    ev = np.zeros(shape, EVENT)
    ev["type"] = -1
    ev["target"] = -1
    ev["dep_rank"] = -1
    return ev


def run(oracle_mod, lat, step0, n, defect_fraction, seed, max_events, horizon_events, thermal_mode=1, thermal_dt=1e-6):
    assert lat.L % BOX == 0 and lat.L >= BOX and 1 <= max_events <= 64 and horizon_events > 0 and thermal_mode in (0, 1)
    L, K = lat.L, max_events
    D = (L // BOX) ** 3
    u_of = oracle_mod.counter_uniform
    c, re = lat.params.impurity_c, lat.params.impurity_re
    totals, dt_event, horizon = [], [], []
    n_exec, n_capped = [], []
    events = _empty_log((n, D, K))
    stats = dict(per_box=[], stops={s: 0 for s in STOPS}, kinds_later=[0, 0, 0, 0], targets_outside=0, min_margin=math.inf,
                 max_per_box=0)
    status, done = 0, 0
    for s in range(n):
        g = step0 + s
        if thermal_mode and g % 20 == 0:
            lat.thermal_cet(dt=thermal_dt, scrub_nan=True)
        sw = lat.sweep()
        total = sw["total"]
        totals.append(total)
        if sw["n_events"] == 0 or total < 1e-25 or not np.isfinite(total):
            status = 1
            break
        dt_event.append(max(-math.log(max(1e-12, u_of(seed, g, KEY_DT))) / total, 1e-12))
        org = [window_origin(L, g, d) for d in range(D)]
        first = [lat.window_pick(*org[d], H, u_of(seed, g, KEY_PICK | d), with_total=True) for d in range(D)]
        Rmax = max([R for ev, R in first if ev is not None], default=0.0)
        tau = (horizon_events / Rmax) if Rmax > 0.0 else 0.0
        ex = cap = 0
        counts = np.zeros(D, np.int64)
        for d in range(D):
            ev, R = first[d]
            i0, j0, k0 = org[d]
            t, m = 0.0, 0
            stop = "idle" if ev is None else "emptied"
            while ev is not None:
                if m == K:
                    stop = "capped"
                    break
                u = u_of(seed, g, KEY_WAIT | (m << 24) | d)
                w = (-math.log(u) / R) if u > 0.0 else math.inf
                if math.isfinite(tau) and math.isfinite(w):
                    stats["min_margin"] = min(stats["min_margin"], abs(t + w - tau) / tau)
                if t + w > tau:
                    stop = "horizon"
                    break
                t += w
                pos = tuple(ev.pos)
                kk = keys(m, d, pos[1], pos[2], L)
                if ev.type == 0:
                    ev.atom = dep_species(u_of(seed, g, kk["species"]), c, re)
                th = ph = 0.0
                if ev.type in (0, 2):
                    th = 0.0 + (3.141592653589793 - 0.0) * u_of(seed, g, kk["theta"])
                    ph = 0.0 + (6.283185307179586 - 0.0) * u_of(seed, g, kk["phi"])
                else:      # diffusion carries the atom's orientation, attachment copies the neighbour's
                    src = pos if ev.type == 1 else tuple(ev.target)
                    th, ph = float(lat.theta[src]), float(lat.phi[src])
                mk = bool(defect_fraction > 0.0 and u_of(seed, g, kk["defect"]) < defect_fraction)
                rec = events[s, d, m]
                rec["type"], rec["pos"], rec["target"], rec["atom"], rec["rate"] = ev.type, pos, tuple(ev.target), ev.atom, ev.rate
                rec["theta"], rec["phi"] = th, ph
                if m >= 1:
                    stats["kinds_later"][ev.type] += 1
                if ev.type == 1:
                    tg = tuple(ev.target)
                    stats["targets_outside"] += int(not all(o <= x < o + H for x, o in zip(tg, (i0, j0, k0))))
                lat.apply(ev, th, ph, mk)
                m += 1
                ex += 1
                if m < K:
                    ev, R = lat.window_pick(i0, j0, k0, H, u_of(seed, g, kk["pick"] + (1 << 24)), with_total=True)
            stats["stops"][stop] += 1
            cap += stop == "capped"
            counts[d] = m
        stats["per_box"].append(counts)
        stats["max_per_box"] = max(stats["max_per_box"], int(counts.max()))
        n_exec.append(ex)
        n_capped.append(cap)
        horizon.append(tau)
        done += 1
    return dict(done=done, status=status, totals=np.array(totals), dt_event=np.array(dt_event), horizon=np.array(horizon),
                n_exec=np.array(n_exec, np.int64), n_capped=np.array(n_capped, np.int64), events=events[:done], stats=stats)
