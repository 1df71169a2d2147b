"""A third vocabulary for the live-handle scripts of live_ops.py (test-only; nothing here needs a GPU to import): the implicit
scheme, thermal boundaries, beam tables, direct beam updates, the shifts, and the lane and tile options.

It sits BESIDE the first two: nothing here feeds the scripts that tests/test_live_ops_host.py pins by hash.  ``Runner3`` extends
live_ops.Runner: the settings change what LATER updates do and leave every cache and the applied-update marker alone; a non-zero
shift leaves the handle as an upload of the five new fields would and drops the marker; the options are documented no-ops.
While the scheme is implicit the oracle side of a run_steps call is ONE persistent beam_ref.Stepper (boundary_ref and
implicit_ref beneath it) whose n, threshold, boundary and table follow the settings; under the explicit scheme it is the
substep_ref.Stepper of the second vocabulary; the marker (applied_g) is carried from one to the other.  The Runner predicts the
running totals of cetkmc_get_implicit_info, the boundary and beam records (both coeff_uploads from the sequence of (r, six beta)
keys the script produced), the shift calls and, on shapes with a lane table, cetkmc_lane_table's ``fresh``.
"""
import functools

import numpy as np

import beam_ref
import boundary_ref
import live_ops as lo
import substep_ref
from live_ops import (COUNTER_SEED, DEFECT_FRACTION, LASER_POWER, REFUSED_LOOKAHEAD, REFUSED_MELT_ON, REFUSED_SLABS, REFUSED_SUBSTEPS,
                      T_MELT, THERMAL_DT, TIMED_DT, _is_mode_b, _mut, _opt, _set, _step)

# ---- the vocabulary --------------------------------------------------------------------------------------------------------------
SETTINGS3 = ("set_scheme_implicit", "set_scheme_explicit", "set_boundary_sink", "set_boundary_mixed", "set_boundary_none",
             "set_beam_d1", "set_beam_d3", "set_beam_short", "set_beam_none")
OPTION_DEFAULTS3 = dict(lane_sums=1, lane_sweep=1, lane_build=1, table_lane_skip=1, fused_tiles=1, early_tiles=-1)
OPTION_MUTATORS3 = [("lane_sums", 0), ("lane_sweep", 0), ("lane_build", 0), ("table_lane_skip", 0), ("fused_tiles", 0), ("fused_tiles", 2),
                    ("early_tiles", 0)]
MUTATORS3 = {s: "setting3" for s in SETTINGS3}
MUTATORS3.update(shift_layer="shift", shift_frame="shift", time_shift="shift", shift_zero="shift_noop", thermal_beam="beam_update")
MUTATORS3.update({f"opt_{k}={v}": "options" for k, v in OPTION_MUTATORS3})
NOOP_CLASSES3 = lo.NOOP_CLASSES2 + ("setting3", "shift_noop")
READ_ONLY3 = ("implicit_info", "thermal_boundary", "beam_info", "lane_table", "lane_table_arrays")
# the mutators of the earlier vocabularies that pairs3 also meets while the scheme is implicit
IMPLICIT_TOO = ("thermal_cet", "thermal_laser", "time_thermal_cet", "time_thermal_laser")

# the fragments of the documented refusals (include/cetkmc.h)
REFUSED_IMPLICIT = "refused while the thermal scheme is implicit"
REFUSED_BOUNDARY_SET = "refused while a thermal boundary is set"
REFUSED_BEAM_SET = "refused while a beam is set"
REFUSED_BOUNDARY_EXPLICIT = "a thermal boundary needs the implicit scheme"
REFUSED_BEAM_EXPLICIT = "a beam needs the implicit scheme"
REFUSED_LASER_BEAM = "cetkmc_thermal_laser: a beam is set"
REFUSED_PLANES_BEAM = "q_planes must be NULL"
REFUSED_STEP_ROWS = "leave the beam table's rows"
REFUSED_BEAM_ROW = "is outside the beam table's rows"
REFUSED_NO_BEAM = "no beam is set"

# Face i_lo is the substrate side.  The sink's face temperature rises with the update ordinal (ramp != 0), so an update that
# took the ordinal of another step would show.  Small beta: plane i = 0 cools by a few kelvin per update and the event mix
# stays what the comment at live_ops.LASER_POWER asks for.  The deposition plane (face i_hi) stays adiabatic in both.
BOUNDARIES = dict(
    sink=dict(beta=[0.05, 0.0, 0.0, 0.0, 0.0, 0.0], T_ext=[3300.0, 0.0, 0.0, 0.0, 0.0, 0.0], ramp=[2.0, 0.0, 0.0, 0.0, 0.0, 0.0]),
    mixed=dict(beta=[0.04, 0.0, 0.02, 0.03, 0.05, 1.0], T_ext=[3300.0, 0.0, 3400.0, 3400.0, 3100.0, T_MELT + 0.2],
               ramp=[1.0, 0.0, 0.5, -0.5, 2.0, 0.01]))
BEAMS = dict(d1=(4, 1), d3=(4, 3), short=(2, 1))         # name -> (n_u, depth); u0 = 0: ordinal 0 is an update of the paths
BEAM_U0 = 0
SHIFTS = dict(
    shift_layer=dict(d=(-2, 0, 0), fill_state=0, fill_T=T_MELT + 0.3, T_mode="value", fill_theta=0.0, fill_phi=0.0),     # a recoated layer
    shift_frame=dict(d=(0, 3, -2), fill_state=1, fill_T=0.0, T_mode="edge", fill_theta=0.3, fill_phi=1.1),               # a frame that moves
    shift_zero=dict(d=(0, 0, 0), fill_state=2, fill_T=3000.0, T_mode="value", fill_theta=0.5, fill_phi=0.5),             # the documented no-op
    time_shift=dict(d=(-1, 0, 1), fill_state=0, fill_T=T_MELT + 0.2, T_mode="value", fill_theta=0.2, fill_phi=0.0))


def boundary_of(name):
    """the boundary as tests/boundary_ref.py takes it, or None"""
    if name is None:
        return None
    return {k: np.array(v, np.float64) for k, v in BOUNDARIES[name].items()}


@functools.lru_cache(maxsize=None)
def beam_table(L, name):
    """A beam table (tests/beam_ref.py): a Gaussian spot of 1.5 voxels that moves from row to row, cut to exact zeros outside its
    footprint; the amplitude is the peak of the plane that live_ops.LASER_POWER gives, so one update heats the spot as much."""
    from cetkmc import synthetic
    n_u, D = BEAMS[name]
    A = float(synthetic.laser_planes(L, 0, 1, power=LASER_POWER)[0].max())
    x = np.arange(L, dtype=np.float64)
    gj, gk = np.zeros((n_u, L)), np.zeros((n_u, L))
    for u in range(n_u):
        for g, c in ((gj, L / 3.0 + 1.5 * u), (gk, L / 2.0 - u + 0.3)):
            row = np.exp(-0.5 * ((x - c) / 1.5) ** 2)
            row[row < 1e-4] = 0.0
            g[u] = row
    fi = np.array([1.0, 0.6, 0.3][:D])
    amp = A * np.array([1.1, 0.7] if name == "short" else [1.0, 0.8, 1.2, 0.9])
    return dict(u0=BEAM_U0, amp=amp, gj=gj, gk=gk, fi=fi)


def update_ordinals(step0, n):
    """the ordinals g / 20 of the update steps of a call (from step0 and n alone, as the library computes them)"""
    return [g // 20 for g in range(step0, step0 + n) if g % 20 == 0]


def leaves_table(spec, beam):
    return (beam is not None and spec["kind"] == "run" and spec.get("thermal_mode") == 2 and
            any(not 0 <= u - BEAM_U0 < BEAMS[beam][0] for u in update_ordinals(spec["step0"], spec["n"])))


def beam_u(seed):
    """the ordinal of a direct thermal_beam update: inside the tables d1 and d3, outside ``short`` two times in three"""
    return 1 + seed % 3


def shift_oracle(lat, d, **kw):
    """tests/shift_ref.shift_fields into the oracle lattice with prev_state := state, as an upload of all five leaves them"""
    import shift_ref
    out, info = shift_ref.shift_fields(dict(state=lat.state, defects=lat.defects, theta=lat.theta, phi=lat.phi, T=lat.T), d, **kw)
    lat.state = np.ascontiguousarray(out["state"], dtype=np.int8)
    lat.defects = np.ascontiguousarray(out["defects"], dtype=np.int8)
    lat.theta, lat.phi, lat.T = (np.ascontiguousarray(out[k], dtype=np.float64) for k in ("theta", "phi", "T"))
    lat.prev_state = lat.state.copy()
    return info


# ---- the comparator of the implicit scheme -------------------------------------------------------------------------------------
class Stepper3(beam_ref.Stepper):
    """beam_ref.Stepper whose table may be None: its laser updates then read planes, as boundary_ref.Stepper's do"""

    def _update(self, lat, n, dt, thermal_mode, q, **kw):
        if thermal_mode != 2 or self.table is None:
            return boundary_ref.Stepper._update(self, lat, n, dt, thermal_mode, q, **kw)
        return super()._update(lat, n, dt, thermal_mode, q, **kw)

    def run_steps(self, step0, n, *args, **kw):
        if self.table is None:
            return boundary_ref.Stepper.run_steps(self, step0, n, *args, **kw)
        return super().run_steps(step0, n, *args, **kw)


def _hooked(base):
    """``base`` with the Runner's look at every melt pass (runner: set on the instance)"""
    class Hooked(base):
        def melt(self, g):
            r = self.runner
            r._note_gap(self.threshold)
            occ = self.lat.state != 0
            k = super().melt(g)
            r.ever_melted |= occ & (self.lat.state == 0)
            r.last["melted"] = r.last.get("melted", 0) + k
            return k
    return Hooked


HOOKED = {True: _hooked(Stepper3), False: _hooked(substep_ref.Stepper)}


def make_stepper(lat, implicit, n, threshold, bc, table, cls=None):
    """Stepper3 under the implicit scheme, substep_ref.Stepper under the explicit one"""
    if implicit:
        return (cls or Stepper3)(lat, table, n, threshold, bc=bc)
    return (cls or substep_ref.Stepper)(lat, n, threshold)


class Runner3(lo.Runner):
    def __init__(self, o, L, **kw):
        self.implicit, self.bc_name, self.beam_name = False, None, None
        self.imp = dict(updates=0, steps=0, launches=0, coeff_uploads=0)          # cetkmc_get_implicit_info as it must read
        self.bci = dict(updates=0, steps=0, launches=0, coeff_uploads=0)          # the boundary's record
        self.beami = dict(updates=0, steps=0, launches=0, table_uploads=0)        # cetkmc_get_beam_info
        self.shift_calls = 0
        self.coef_key = dict(imp=None, bc=None)        # (r, six beta, n, dt) of the device tables coef and coef_bc
        self.coef_log = []                             # (tag, table, cause): first | beta | n | dt | several
        self.steppers = {}                             # scheme -> the persistent comparator
        self.marker = -1                               # applied_g, carried from one comparator to the other
        self.lflag = None                              # the handle's lanes_fresh as predicted (None: not predicted)
        self.lane_checks = self.lane_builds = self.lane_call_checks = 0
        self.has_lanes = False
        super().__init__(o, L, **kw)
        self.opt.update(OPTION_DEFAULTS3)
        self.opt_defaults.update(OPTION_DEFAULTS3)
        if self.e is not None and self.n_slabs == 1 and 128 < self.L <= 256:
            lt = self.e.lane_table()
            self.has_lanes = lt["chunks"] > 0
            assert self.has_lanes, "this shape has a lane table"
            self.lane_builds0 = lt["builds"] + lt["builds_thermal"]       # (the comparison at creation ran before has_lanes was known)

    # -- what the settings amount to ------------------------------------------------------------
    def bc(self):
        return boundary_of(self.bc_name)

    def table(self):
        return None if self.beam_name is None else beam_table(self.L, self.beam_name)

    def _lane_on(self):
        o = self.opt
        return bool(o["lane_sums"] and o["table_lane_skip"] and o["fused_tiles"] >= 1 and not o["thermal_lookahead"] and o["sweep_variant"] == 1)

    def _count_update(self, dt, source, u=None):
        """one implicit update joins the records; the table it reads is rebuilt where its (r, six beta) key changed"""
        n = self.substeps
        P = self.lat.params
        dt_s = dt / n if n > 1 else dt
        r = (P.alpha * dt_s) * P.inv_dx2
        on = self.bc_name is not None
        for rec, counts in ((self.imp, True), (self.bci, on), (self.beami, bool(source and self.beam_name))):
            if counts:
                rec["updates"] += 1
                rec["steps"] += n
                rec["launches"] += 3 * n
        which, rec = ("bc", self.bci) if on else ("imp", self.imp)
        key = (r, tuple(BOUNDARIES[self.bc_name]["beta"]) if on else (0.0,) * 6, n, dt)
        old = self.coef_key[which]
        if old is None or old[:2] != key[:2]:
            rec["coeff_uploads"] += 1
            why = [w for w, a, b in (("beta", old and old[1], key[1]), ("n", old and old[2], n), ("dt", old and old[3], dt)) if a != b]
            self.coef_log.append((self.tag, which, "first" if old is None else why[0] if len(why) == 1 else "several"))
        self.coef_key[which] = key

    def _verify_info(self):
        super()._verify_info()
        if self.e is not None:
            for name, got, want in (("implicit_info", self.e.implicit_info(), self.imp), ("boundary_info", self.e.boundary_info(), self.bci),
                                    ("beam_info", self.e.beam_info(), self.beami)):
                assert got == want, (self.tag, name, got, want)

    def _verify(self):
        lanes = self.e is not None and self.has_lanes
        if lanes:
            lt = self.e.lane_table()
            pred = self.lflag if self._lane_on() else 0
            if pred is not None:
                assert lt["fresh"] == int(pred), (self.tag, "lane_table fresh before the next plain launch", lt, pred)
                self.lane_checks += 1
        super()._verify()
        if lanes:
            lt2, on = self.e.lane_table(), self._lane_on()
            assert lt2["fresh"] == int(on), (self.tag, "lane_table fresh behind a plain launch", lt2, on)
            built = lt2["builds"] + lt2["builds_thermal"] - lt["builds"] - lt["builds_thermal"]
            assert built == int(on and not lt["fresh"]), (self.tag, "lane table builds of one plain launch", lt, lt2)
            self.lane_builds += built
            if on:
                self.lflag = True

    def _drop_marker(self):
        self.marker = -1

    # -- settings, options ----------------------------------------------------------------------------
    def setting(self, name):
        e = self.e
        if name not in SETTINGS3:
            return super().setting(name)
        if name == "set_scheme_implicit":
            call = lambda: e.set_thermal_scheme("implicit")
            if self.n_slabs > 1:
                return self._refused(call, REFUSED_SLABS)
            if self.opt["thermal_lookahead"]:
                return self._refused(call, REFUSED_LOOKAHEAD)
            self.implicit = True
        elif name == "set_scheme_explicit":
            call = lambda: e.set_thermal_scheme("explicit")
            if self.bc_name is not None:
                return self._refused(call, REFUSED_BOUNDARY_SET)
            if self.beam_name is not None:
                return self._refused(call, REFUSED_BEAM_SET)
            self.implicit = False
        elif name.startswith("set_boundary_"):
            which = None if name.endswith("_none") else name[13:]
            call = lambda: e.set_thermal_boundary(None if which is None else BOUNDARIES[which])
            if which is not None and not self.implicit:
                return self._refused(call, REFUSED_BOUNDARY_EXPLICIT)
            self.bc_name = which
        else:
            which = None if name.endswith("_none") else name[9:]
            call = lambda: e.set_beam(None if which is None else beam_table(self.L, which))
            if which is not None and not self.implicit:
                return self._refused(call, REFUSED_BEAM_EXPLICIT)
            self.beam_name = which
            self.beami["table_uploads"] += which is not None
        if e is not None:
            call()

    def set_option(self, key, value):
        if key == "thermal_lookahead" and value and self.implicit and not (self.remelt_on or self.substeps > 1):
            return self._refused(lambda: self.e.set_option(key, value), REFUSED_IMPLICIT)
        refusals = len(self.refusals)
        super().set_option(key, value)
        if len(self.refusals) == refusals:
            if key in ("lane_sums", "thermal_lookahead", "sweep_variant", "interface_every_step"):
                self.lflag = False
            elif key not in ("lane_sweep", "lane_build", "table_lane_skip", "fused_tiles", "early_tiles", "apply_in_sweep", "reserve_batch",
                             "substep_block", "substep_planes", "thermal_planes_per_block", "thermal_planes_per_block16", "thermal_table",
                             "thermal_variant"):
                self.lflag = None

    # -- one operation ---------------------------------------------------------------------------------
    # what a mutator of the earlier vocabularies does to the lane table's freshness: False = stale (its cause carries TABLE or
    # IFC); absent = not predicted
    LANE_STALE = ("upload_", "set_defects", "set_prev_state_none", "apply_event", "staged", "param_", "remelt", "time_remelt", "freeze")

    def _do(self, op):
        kind, name = op["kind"], op["name"]
        if kind == "ro" and name not in READ_ONLY3:
            self.lflag = None
        elif kind == "mut" and name not in MUTATORS3 and not name.startswith("opt_"):
            if name.startswith(self.LANE_STALE):
                self.lflag = False
            elif name != "set_prev_state":
                self.lflag = False if self.implicit and name.startswith(("thermal_", "time_thermal")) else None
        return super()._do(op)

    def _lane_builds_of_call(self, op, stale):
        """Plain launches of a run_steps call that build the lane table, from the rules of the host layer; None: not predicted.
        Every temperature update of a shape whose rows the fused 16-row tiles do not cover raises cause thermal_update (TABLE): the
        table goes stale, and the sweep of an update step is a plain launch (the step before it is never deferred), which
        builds.  So is the call's first sweep.  Every other launch applies a pending event or reads a table that the batched
        apply has kept fresh."""
        spec = self.paths[op["name"]]
        if spec["kind"] != "run" or spec["incremental"] or self.L % 16 == 0 or self.remelt_on or stale is None:
            return None
        if not self._lane_on():
            return 0
        ups = [g for g in range(spec["step0"], spec["step0"] + spec["n"]) if spec["thermal_mode"] and g % 20 == 0 and g != self.marker]
        return len(ups) + int(bool(stale) and spec["step0"] not in ups)

    def step(self, op):
        lanes = self.e is not None and self.has_lanes
        if lanes:
            lt = self.e.lane_table()
            stale = None if self.lflag is None else not (self.lflag and self._lane_on())
            want = self._lane_builds_of_call(op, stale)
        ro = super().step(op)
        if lanes and ro is not None:
            lt2, on = self.e.lane_table(), self._lane_on()
            built = lt2["builds"] + lt2["builds_thermal"] - lt["builds"] - lt["builds_thermal"]
            assert lt2["fresh"] == int(on), (self.tag, "lane_table fresh behind a stepping call and its comparison", lt2, on)
            if want is not None:         # (the comparison's own plain launch builds nothing: the call left the table fresh)
                assert built == want, (self.tag, "lane table builds of a stepping call", lt, lt2, want)
                self.lane_call_checks += 1
            self.lane_builds += built
            if on:
                self.lflag = True
        return ro

    # -- direct updates ------------------------------------------------------------------------------------
    def _update(self, laser, dt, q=None, latent=True, scrub=True, u=0):
        if not self.implicit:
            self.lflag = None            # an explicit update may write the rate table and the lane table with it: not predicted
            return super()._update(laser, dt, q, latent=latent, scrub=scrub)
        self.lflag = False               # cause thermal_update: TABLE
        self._drop_marker()
        self._count_update(dt, laser)
        if laser and self.beam_name is not None:
            beam_ref.update(self.lat, self.substeps, dt, self.table(), u, use_latent=latent, scrub=scrub, bc=self.bc())
        else:
            boundary_ref.update(self.lat, self.substeps, dt, 2 if laser else 1, q, use_latent=latent, scrub=scrub, bc=self.bc(), u=u)

    def m_thermal_laser(self, op, latent=True):
        if self.beam_name is not None:
            from cetkmc import synthetic
            q = synthetic.laser_planes(self.L, 0, 1, power=LASER_POWER)[0]
            return self._refused(lambda: self.e.thermal_laser(THERMAL_DT, q, use_latent=latent, scrub_nan=True), REFUSED_LASER_BEAM)
        super().m_thermal_laser(op, latent)
        if self.e is not None:
            self._verify_info()              # the records behind every direct update

    def m_thermal_cet(self, op, dt=THERMAL_DT, scrub=True):
        super().m_thermal_cet(op, dt=dt, scrub=scrub)
        if self.e is not None:
            self._verify_info()

    def m_time_thermal(self, laser):
        if not (self.implicit and laser and self.beam_name is not None):
            return super().m_time_thermal(laser)
        for _ in range(lo.TIMED_UPDATES):           # a beam: row 0 of its table, update ordinal u0
            self._update(True, TIMED_DT, None, latent=True, scrub=True, u=BEAM_U0)
        if self.e is not None:
            self.e.time_thermal(lo.TIMED_UPDATES, laser=True)
            self._verify_info()

    def m_thermal_beam(self, op):
        u = beam_u(op["seed"])
        call = lambda: self.e.thermal_beam(THERMAL_DT, u, use_latent=True, scrub_nan=True)
        if self.beam_name is None:
            return self._refused(call, REFUSED_NO_BEAM)
        if not 0 <= u - BEAM_U0 < BEAMS[self.beam_name][0]:
            return self._refused(call, REFUSED_BEAM_ROW)
        self.last = dict(u=u)
        self._update(True, THERMAL_DT, None, latent=True, scrub=True, u=u)
        if self.e is not None:
            call()
            self._verify_info()

    # -- shifts ----------------------------------------------------------------------------------------------
    def m_shift(self, op, timed=False):
        sh = SHIFTS[op["name"]]
        call = (lambda: self.e.time_shift(**sh)[0]) if timed else (lambda: self.e.shift(**sh))
        if self.n_slabs > 1:
            return self._refused(call, REFUSED_SLABS)
        moved = any(sh["d"])
        info = shift_oracle(self.lat, **sh) if moved else dict(kept=self.L ** 3, exposed=0, dropped=[0] * 6)
        if moved:
            self.shift_calls += 1
            self._drop_marker()                  # a new field: the update a stopped batch applied is no longer remembered
            self.lflag = False                   # cause upload_T_or_state
        self.last = dict(shift=sh, info=info)
        if self.e is not None:
            got = call()
            assert got == dict(info, calls=self.shift_calls), (self.tag, "shift info", got, info, self.shift_calls)

    m_shift_layer = m_shift_frame = m_shift_zero = m_shift

    def m_time_shift(self, op):
        self.m_shift(op, timed=True)

    # -- read-only calls -----------------------------------------------------------------------------------------
    def read_only(self, name, seed):
        if name not in READ_ONLY3:
            return super().read_only(name, seed)
        e = self.e
        if e is None:
            return
        if name in ("implicit_info", "beam_info"):
            return self._verify_info()
        if name == "thermal_boundary":
            want = BOUNDARIES[self.bc_name] if self.bc_name else dict(beta=[0.0] * 6, T_ext=[0.0] * 6, ramp=[0.0] * 6)
            got = e.thermal_boundary()
            assert got == {k: [float(x) for x in v] for k, v in want.items()}, (self.tag, "thermal_boundary", got, want)
            return self._verify_info()
        lt = e.lane_table()
        assert (lt["chunks"] > 0) == self.has_lanes and lt["usable"] + lt["poisoned"] <= lt["chunks"], (self.tag, lt)
        if name == "lane_table_arrays" and self.has_lanes:
            sums, counts = e.lane_table_arrays()
            assert sums.shape == counts.shape and sums.shape[:2] == (self.L, self.L), (self.tag, sums.shape, counts.shape)
            assert int((counts == 0xFF).sum()) == lt["poisoned"], (self.tag, "poisoned chunks", lt)

    # -- stepping ------------------------------------------------------------------------------------------------
    def _inputs(self, spec, op):
        self._op = op
        inp = lo.step_inputs(self.L, spec, op["seed"])
        if self.beam_name is not None and spec["kind"] == "run" and not op.get("with_planes"):
            inp["q"] = None                      # a beam: the updates' sources are rows of its table
        return inp

    def _step_refusal(self, spec):
        if _is_mode_b(spec) and self.implicit and not (self.remelt_on or self.substeps > 1):
            return REFUSED_IMPLICIT
        frag = super()._step_refusal(spec)
        if frag is None and spec["kind"] == "run" and spec["thermal_mode"] == 2 and self.beam_name is not None:
            if self._op.get("with_planes"):
                return REFUSED_PLANES_BEAM
            if leaves_table(spec, self.beam_name):
                return REFUSED_STEP_ROWS
        if frag is None:
            self.lflag = None            # the call runs: what its launches leave of the lane table is not predicted
        return frag

    def _needs_stepper(self, op):
        return self.implicit or self.remelt_on or self.substeps > 1 or "cut" in op or "resume" in op or self.marker >= 0

    def _stepper(self, lat=None, probe=False):
        thr = self.remelt_threshold if self.remelt_on else None
        if probe:
            return make_stepper(lat, self.implicit, self.substeps, thr, self.bc(), self.table())
        st = self.steppers.get(self.implicit)
        if st is None:
            st = self.steppers[self.implicit] = make_stepper(self.lat, self.implicit, 1, None, None, None, cls=HOOKED[self.implicit])
            st.runner = self
            st.info = self.info                       # one set of counters for direct passes and the loop's
        st.lat, st.n, st.threshold = self.lat, self.substeps, thr
        if self.implicit:
            st.bc, st.table = self.bc(), self.table()
        st.applied_g = self.marker
        return st

    def _stepper_run(self, op, spec, inp):
        st = self._stepper()
        step0, n = spec["step0"], spec["n"]
        kw = dict(rng_mode=spec["rng_mode"], seed=COUNTER_SEED, thermal_mode=spec["thermal_mode"], thermal_dt=THERMAL_DT)
        if "cut" in op:          # the stream ends where step op["cut"] would begin to read it: a probe on a clone finds the place
            x = op["cut"] - step0

            def probe(m, u_np):
                p = self._stepper(lo.clone(self.o, self.lat), probe=True)
                return p.run_steps(step0, m, DEFECT_FRACTION, inp["u_pick"][:m], inp["u_def"][:m], u_np, q_planes=inp["q"], **kw)

            lo_ = probe(x, inp["u_np"])["np_used"]
            hi_ = min(lo_ + self.L * self.L + 2, len(inp["u_np"]))
            while lo_ < hi_:
                mid = (lo_ + hi_) // 2
                lo_, hi_ = (lo_, mid) if probe(x, inp["u_np"][:mid])["done"] >= x else (mid + 1, hi_)
            self.cut = lo_
            inp = dict(inp, u_np=inp["u_np"][:self.cut])
        elif "resume" in op:
            x = op["resume"] - step0
            q = inp["q"]
            inp = dict(u_pick=inp["u_pick"][x:], u_def=inp["u_def"][x:], u_np=inp["u_np"][self.cut:],
                       q=None if q is None else q[lo.updates_before(step0, x):])
            step0, n = step0 + x, n - x
        self.last.update(substeps=st.n, threshold=st.threshold, marker=self.marker, melted=0, inp=inp, args=(step0, n),
                         implicit=self.implicit, bc=self.bc_name, beam=self.beam_name)
        if self.implicit and spec["thermal_mode"]:
            issued = [g for g in range(step0, step0 + n) if g % 20 == 0 and g != self.marker]
            for g in issued:         # what the host issues, a stop or not: every update step of the call but the one it skips
                self._count_update(THERMAL_DT, spec["thermal_mode"] == 2)
        before = dict(st.stats)
        ro = st.run_steps(step0, n, DEFECT_FRACTION, inp["u_pick"], inp["u_def"], inp["u_np"], q_planes=inp["q"], **kw)
        self.marker = st.applied_g
        if st.n > 1 and not self.implicit:
            for k in self.sub:
                self.sub[k] += st.stats[k] - before[k]
        return ro, inp


# ---- scripts -----------------------------------------------------------------------------------------------------------------------
def paths3(L):
    """the stepping paths of the walk: every path of the first two vocabularies and the Mode A call from step 39"""
    return dict(lo.paths2(L), a_rng1_full_laser_39=lo.extra_paths()["a_rng1_full_laser_39"])


def mode_a_paths(L):
    return [p for p, s in lo.stepping_paths(L).items() if s["kind"] in ("run", "loop")]


def _restore3(name):
    key = name[4:].split("=")[0]
    return _opt(f"opt_{key}={OPTION_DEFAULTS3[key]}")


IMP, EXP = "set_scheme_implicit", "set_scheme_explicit"


def _block3(name, seed, pname, spec):
    """New setting, mutator or option M = ``name`` directly ahead of a call of path S = ``pname``, with what M needs in front
    and what puts the handle back behind.  Where S leaves the rows of set_beam_short: the refused S, the restore, S."""
    s1, s2 = _step(pname, seed + 1), _step(pname, seed + 2)
    if name == IMP:
        return [_set(IMP), s1, _set(EXP)]
    if name == EXP:
        return [_set(IMP), _set(EXP), s1]
    if name in ("set_boundary_sink", "set_boundary_mixed"):
        return [_set(IMP), _set(name), s1, _set("set_boundary_none"), _set(EXP)]
    if name == "set_boundary_none":
        return [_set(IMP), _set("set_boundary_sink"), _set(name), s1, _set(EXP)]
    if name in ("set_beam_d1", "set_beam_d3", "set_beam_short"):
        return [_set(IMP), _set(name), s1, _set("set_beam_none"), _set(EXP)] + [s2] * leaves_table(spec, name[9:])
    if name == "set_beam_none":
        return [_set(IMP), _set("set_beam_d1"), _set(name), s1, _set(EXP)]
    if name == "thermal_beam":
        return [_set(IMP), _set("set_beam_d3"), _mut(name, seed), s1, _set("set_beam_none"), _set(EXP)]
    if name in ("shift_layer", "shift_frame", "time_shift", "shift_zero"):
        return [_mut(name, seed), s1]
    if name.startswith("opt_"):
        return [_opt(name), s1, _restore3(name)]
    if name.startswith("imp:"):          # a mutator of the earlier vocabularies while the scheme is implicit
        m = name[4:]
        if m.startswith("time_thermal"):
            return [_set(IMP), _set("set_boundary_sink"), _mut(m, seed), s1, _mut("upload_T", seed + 3), _set("set_boundary_none"), _set(EXP)]
        return [_set(IMP), _mut(m, seed), s1, _set(EXP)]
    raise KeyError(name)


def _balance(seed):
    """With the base parameters three events in a hundred are nucleations, and a script without parameter mutators keeps them:
    the alternative I0 and nu_dep (live_ops.ALT_PARAMS) give about 45 : 25 : 15 : 15, so that the first call behind a mutator
    that occurs a few times only still meets all four kinds."""
    return [_mut("param_I0", seed + 19990), _mut("param_nu_dep", seed + 19991)]


def pairs3_names():
    """shift_frame last: it fills five sixteenths of the lattice with atoms, and a fresh lattice in its place (upload_full) would
    nucleate next to nothing for the calls that follow"""
    return [m for m in MUTATORS3 if m != "shift_frame"] + ["imp:" + m for m in IMPLICIT_TOO] + ["shift_frame"]


def pairs3_script(L, pname, seed=0):
    spec = lo.stepping_paths(L)[pname]
    ops = _balance(seed) + [_step(pname, seed + 20000)]
    for q, name in enumerate(pairs3_names()):
        ops += _block3(name, seed + 20000 + 10 * (q + 1), pname, spec)
    return ops


def deferred_pairs3_script(seed=0):
    """L > 128: every new setting, mutator and option once, the path alternating between the deferring default and apply_in_sweep
    off; two mutators whose cause carries IFC without TABLE; then the Mode chain, Mode B and the local loop alternating with
    the deferring call on the same handle."""
    paths = lo.deferred_paths()
    names = list(paths)
    ops = _balance(seed) + [_step(names[0], seed + 20000), _step(names[1], seed + 20001)]
    ops += [dict(kind="ro", name=x, seed=seed + 20002) for x in READ_ONLY3]          # behind a warm deferring call
    for q, name in enumerate([m for m in MUTATORS3 if m != "shift_frame"] + ["imp:thermal_cet", "imp:time_thermal_laser", "shift_frame"]):
        pname = names[q % 2]
        ops += _block3(name, seed + 20000 + 10 * (q + 1), pname, paths[pname])
    s = seed + 21000
    # (the read-only calls behind a mutator that made the lane table stale, and whose interface kernel poisons chunks)
    ops += [_mut("set_defects", s), dict(kind="ro", name="lane_table_arrays", seed=s), dict(kind="ro", name="lane_table", seed=s),
            _step("a_deferred", s + 1), _mut("upload_orient", s + 2), _step("a_deferred", s + 3)]
    chain = ["a_deferred", "b_box8", "a_deferred", "local_k4", "a_deferred", "shift_layer", "a_deferred"]
    return ops + [_mut(x, s + 10 + q) if x in MUTATORS3 else _step(x, s + 10 + q) for q, x in enumerate(chain)]


class _State:
    """the switches as a script sets them, for _legalize3 (Runner3 decides what is refused; this only plans)"""

    def __init__(self):
        self.implicit, self.bc, self.beam, self.ahead, self.melt, self.n, self.nan = False, None, None, 0, False, 1, False

    def apply(self, op):
        name = op["name"]
        busy = self.melt or self.n > 1
        if name == IMP:
            self.implicit = self.implicit or not self.ahead
        elif name == EXP:
            self.implicit = self.implicit and (self.bc is not None or self.beam is not None)
        elif name.startswith("set_boundary_"):
            which = None if name.endswith("_none") else name[13:]
            if which is None or self.implicit:
                self.bc = which
        elif name.startswith("set_beam_"):
            which = None if name.endswith("_none") else name[9:]
            if which is None or self.implicit:
                self.beam = which
        elif name == "opt_thermal_lookahead=1":
            self.ahead = int(self.ahead or not (busy or self.implicit))
        elif name == "opt_thermal_lookahead=0":
            self.ahead = 0
        elif name == "set_remelt_on":
            self.melt = self.melt or not self.ahead
        elif name == "set_remelt_off":
            self.melt = False
        elif name.startswith("set_substeps="):
            k = int(name.split("=")[1])
            self.n = k if (k == 1 or not self.ahead) else self.n
        elif name == "upload_T_nan":
            self.nan = True
        elif name in ("upload_T", "upload_full", "staged", "freeze", "thermal_cet", "time_thermal_cet", "time_thermal_laser"):
            self.nan = False

    def to_explicit(self):
        return [_set("set_beam_none")] * (self.beam is not None) + [_set("set_boundary_none")] * (self.bc is not None) + [_set(EXP)]

    def to_implicit(self):
        return [] if self.implicit else [_opt("opt_thermal_lookahead=0")] * self.ahead + [_set(IMP)]

    def conflict(self, op, spaths):
        """(kind, what to insert ahead, whether a refusal may be left to be met) or None"""
        name, s = op["name"], self
        if op["kind"] == "step" and _is_mode_b(spaths[name]) and s.implicit:
            return "mode_b", s.to_explicit(), True
        if name == "opt_thermal_lookahead=1" and s.implicit:
            return "lookahead", s.to_explicit(), True
        if name == IMP and s.ahead:
            return "implicit_ahead", [_opt("opt_thermal_lookahead=0")], True
        if name == EXP and (s.bc is not None or s.beam is not None):
            return "explicit", s.to_explicit()[:-1], True
        if name in ("set_boundary_sink", "set_boundary_mixed", "set_beam_d1", "set_beam_d3", "set_beam_short") and not s.implicit:
            return "needs_implicit", s.to_implicit(), True
        if name in ("thermal_laser", "thermal_laser_nolatent") and s.beam is not None:
            return "laser_beam", [_set("set_beam_none")], True
        if name == "thermal_beam" and s.beam is None:
            return "no_beam", s.to_implicit() + [_set("set_beam_d3")], True
        if name == "staged" and s.beam is not None:          # the staging call of a laser batch would carry planes
            return "staged", [_set("set_beam_none")], False
        if name == "thermal_cet_noscrub_1e6" and s.implicit and s.nan:
            # an unscrubbed NaN travels along whole lines of an implicit solve: the lattice would hold nothing finite
            return "nan", [_mut("upload_T", op.get("seed", 0) + 4)], False
        return None


def _legalize3(ops, spaths):
    """Behind live_ops._legalize: inserts what a call of the third vocabulary needs ahead of it, and, as there, leaves the first,
    fifth, ... conflict of each kind to meet its documented refusal on a warm handle."""
    out, st, met = [], _State(), {}
    for op in ops:
        c = st.conflict(op, spaths)
        if c is not None:
            kind, fixes, may_leave = c
            leave = may_leave and met.get(kind, 0) % 4 == 0
            met[kind] = met.get(kind, 0) + 1
            if not leave:
                for f in fixes:
                    st.apply(f)
                    out.append(f)
        st.apply(op)
        out.append(op)
        if op["name"] in lo.COOLERS and not st.implicit:
            # an explicit update at 1e-6 s leaves a field near its clip values, where the deposition parameters stop mattering
            # (live_ops.py): a new field behind it.  The implicit update at 1e-6 s is stable and is stepped on as it stands.
            out.append(_mut("upload_T", op.get("seed", 0) + 5))
            st.apply(out[-1])
    return out


def walk3_script(L, n_ops=250, seed=0):
    """live_ops.walk2_script over all three vocabularies: two shuffled rounds of everything first, a stepping call at least every
    third drawn operation, then both legalizing passes.  ``stepq`` is a laser call that carries planes: refused under a beam."""
    rs = np.random.RandomState(26000 + seed)
    spaths = paths3(L)
    paths = list(spaths)
    old = lo.stepping_paths(L)
    pool = ([("mut", m) for m in lo.MUTATORS] + [("set" if c == "setting" else "mut", m) for m, c in lo.MUTATORS2.items()] +
            [("set" if c == "setting3" else "mut", m) for m, c in MUTATORS3.items()] +
            [("ro", r) for r in lo.READ_ONLY + lo.READ_ONLY2 + READ_ONLY3] + [("step", p) for p in paths] + [("stepq", "a_rng0_incr_laser_inside")])
    pool += [("set", s) for s in ("set_scheme_implicit", "set_beam_d1", "set_boundary_sink")] * 2      # more of the walk under the new scheme
    pool += [("mut", "thermal_beam"), ("mut", "shift_zero"), ("mut", "shift_layer"), ("mut", "time_shift")] * 2      # (few mutators: more first calls)
    pool += [("opt", f"opt_{k}={v}") for k, v in OPTION_DEFAULTS3.items()]                               # the options find their defaults again
    order = [pool[q] for q in rs.permutation(len(pool))] + [pool[q] for q in rs.permutation(len(pool))]
    while len(order) < n_ops:
        order.append(pool[rs.randint(len(pool))])
    ops, since = [], 0
    for q, (kind, name) in enumerate(order):
        s = seed + 25000 + 7 * q
        if kind not in ("step", "stepq") and since >= 2:
            ops.append(_step(paths[rs.randint(len(paths))], s + 3))
            since = 0
        if kind in ("step", "stepq"):
            ops.append(dict(_step(name, s + 1), **(dict(with_planes=True) if kind == "stepq" else {})))
            since = 0
            continue
        if name == "staged":
            pname = [p for p in old if old[p]["kind"] == "run" and old[p]["rng_mode"] != 2][rs.randint(4)]
            ops += lo._mutator_block(name, s, old[pname], pname, s + 1) + [_step(pname, s + 1, staged=True)]
            since = 0
            continue
        ops += (lo._mutator_block(name, s, dict(kind="run")) if name in lo.MUTATORS else [dict(kind=kind, name=name, seed=s)])
        since += 1
    ops.append(_step(paths[0], seed + 5))
    # Latent heat parks many occupied voxels ON the upper clip value, more so in a walk this long: no threshold then separates
    # three of them from the rest (live_ops.melt_threshold).  A direct pass of this walk gets a new field in front; the pass behind
    # a warm rate table is walk2's and pairs2's business.
    # Behind a shift: a call of seven steps that deposits (the exposed plane i = L - 1 holds the candidates), so that the call
    # behind every shift executes an event at the seam.
    out = []
    for op in _legalize3(lo._legalize(ops, spaths), spaths):
        out += [_mut("upload_T", op.get("seed", 0) + 4)] * (op["name"] in ("remelt", "time_remelt")) + [op]
        out += [_step("a_rng1_full_laser_none", op.get("seed", 0) + 6)] * (MUTATORS3.get(op["name"]) == "shift")
    return out


def toggles3_script(L, seed=0):
    """The switches of the implicit scheme on and off on one handle, a Mode A call that crosses an update (step0 19, 20 or 39)
    behind every change; the coefficient tables are rebuilt for a changed beta alone (the mixed boundary), a changed n alone
    (substeps 1) and a changed dt alone (cetkmc_time_thermal's 1e-6 s, and back)."""
    a19c, a20c, a39l, a19l = "a_rng1_full_cet_last", "a_rng1_incr_cet_first20", "a_rng1_full_laser_39", "a_rng0_incr_laser_inside"
    ahead = "opt_thermal_lookahead="
    # (the refused calls between them change nothing: each documented refusal of the vocabulary is met here on a warm handle)
    chain = [a19c, "set_boundary_sink", "set_beam_d1", ahead + "1", IMP, ahead + "0",
             IMP, ahead + "1", "b_box8", "local_k4", a20c, "set_boundary_sink", EXP, a39l, "set_beam_d1", "thermal_laser", "q:" + a19l, a19l,
             "set_substeps=3", a39l, "set_remelt_on", a19l,
             "shift_layer", a20c, "set_boundary_mixed", a39l, "set_substeps=1", a19l, "time_thermal_cet", a19c, "set_beam_d3", a39l,
             "shift_frame", a19l, "set_beam_none", a39l, "set_boundary_none", a20c, "set_remelt_off", a19c, EXP, a19l, "b_box8", "local_k4",
             IMP, a20c, "set_beam_short", EXP, "a_rng2_incr_laser_first", "thermal_beam", "thermal_beam", a19l, "set_beam_none", EXP]
    ops = []
    for q, x in enumerate(chain):
        s = seed + 27000 + q
        ops.append(_set(x) if x.startswith("set_") else dict(_step(x[2:], s), with_planes=True) if x.startswith("q:") else
                   _opt(x) if x.startswith("opt_") else _mut(x, s) if x in MUTATORS3 or x in lo.MUTATORS2 or x in lo.MUTATORS else _step(x, s))
    return ops


# one operation between a batch that ran out of its stream ON update step 20 and its continuation.  (before, X, behind):
STOPPED3_KEEP = ((), IMP, (EXP,)), ((IMP,), "set_boundary_sink", ("set_boundary_none", EXP)), ((IMP,), "set_beam_d1", ("set_beam_none", EXP)), \
                ((IMP, "set_beam_d1"), "set_beam_none", (EXP,)), ((), "shift_zero", ()), ((), "beam_info", ())
STOPPED3_DROP = ((), "shift_layer", ("upload_full",)), ((), "time_shift", ("upload_full",)), \
                ((IMP, "set_beam_d3"), "thermal_beam", ("set_beam_none", EXP))


def _op3(x, s):
    return _set(x) if x.startswith("set_") else dict(kind="ro", name=x, seed=s) if x in READ_ONLY3 else _mut(x, s)


def stopped3_script(L, seed=0):
    ops = []
    for q, (before, x, behind) in enumerate(STOPPED3_KEEP + STOPPED3_DROP):
        s = seed + 28000 + 20 * q
        ops += [_op3(b, s + 3) for b in before]
        ops += [dict(_step("a_stop", s), cut=20), _op3(x, s + 1), dict(_step("a_stop", s), resume=20, keeps=q < len(STOPPED3_KEEP))]
        ops += [_op3(b, s + 4) for b in behind]
    return ops


REFUSED_ON_SLABS = ("set_scheme_implicit", "set_boundary_sink", "set_boundary_mixed", "set_beam_d1", "set_beam_d3", "set_beam_short",
                    "shift_layer", "shift_frame", "shift_zero", "time_shift", "thermal_beam")


def refusals3_script(L, seed=0):
    """Three slabs: every setting and shift the handle refuses, and the ones it takes as no-ops, between stepping calls of all
    kinds.  Nothing changes."""
    paths = list(lo.paths2(L))
    names = list(REFUSED_ON_SLABS) + ["set_scheme_explicit", "set_boundary_none", "set_beam_none", "implicit_info", "thermal_boundary", "beam_info",
                                      "lane_table"]
    ops = [_step(paths[0], seed + 29000)]
    for q, x in enumerate(names + list(REFUSED_ON_SLABS)):
        s = seed + 29000 + 10 * (q + 1)
        ops += [_op3(x, s), _step(paths[(q + 1) % len(paths)], s + 1)]
    return ops


def script_names3(L):
    return [f"pairs3:{p}" for p in mode_a_paths(L)] + ["walk3", "toggles3", "stopped3"]


# Seeds where seed 0 does not meet the conditions of tests/test_live_ops3_host.py on the oracle: (script, L) -> seed.
SCRIPT_SEEDS3 = {("walk3", 24): 200}


def make_script3(L, name):
    seed = SCRIPT_SEEDS3.get((name, L), 0)
    if name.startswith("pairs3:"):
        return lo._with_prep(pairs3_script(L, name[7:], seed=seed))
    if name == "pairs3_deferred":
        return lo._with_prep(deferred_pairs3_script(seed=seed))
    return dict(walk3=walk3_script, toggles3=toggles3_script, stopped3=stopped3_script, refusals3=refusals3_script)[name](L, seed=seed)
