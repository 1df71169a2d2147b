"""Remelting: the definition in executable form.  NumPy on oracle.Lattice arrays; never touches the
engine.

``remelt(lat, threshold)`` is one pass.  ``Stepper`` is the stepping loop with remelting switched on, composed from existing
oracle calls: before a step with g % 20 == 0 the temperature update, then ``remelt``, then the steps up to the next update
with thermal_mode 0, the uniform streams carried from chunk to chunk.
"""
import numpy as np


def remelt(lat, threshold):
    """m = (state != 0) & (T >= threshold): NaN never melts, +inf does, equality melts, state 4 melts like an atom.  On m:
    state = prev_state = 0, theta = phi = 0.0.  Nothing else changes.  Returns the number of melted voxels."""
    with np.errstate(invalid="ignore"):
        m = (lat.state != 0) & (lat.T >= threshold)
    lat.state[m] = 0
    lat.prev_state[m] = 0
    lat.theta[m] = 0.0
    lat.phi[m] = 0.0
    return int(m.sum())


NB14 = ((1, 1, 0), (1, -1, 0), (-1, 1, 0), (-1, -1, 0), (0, 1, 1), (0, 1, -1), (0, -1, 1), (0, -1, -1),
        (2, 0, 0), (-2, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 2), (0, 0, -2))      # kmc_event_rates.py:29-30


def empty_neighbour(state):
    """mask: the voxel has an empty voxel among its (in-lattice) 14 neighbours"""
    L = state.shape[0]
    pad = np.ones((L + 4,) * 3, bool)
    pad[2:-2, 2:-2, 2:-2] = state != 0
    out = np.zeros(state.shape, bool)
    for di, dj, dk in NB14:
        out |= ~pad[2 + di:2 + di + L, 2 + dj:2 + dj + L, 2 + dk:2 + dk + L]
    return out


def updates_in(step0, n):
    """temperature-update steps (g % 20 == 0) among the n global steps from step0"""
    return sum(1 for g in range(step0, step0 + n) if g % 20 == 0)


class Stepper:
    """The stepping loop of one lattice with remelting on (threshold) -- ``run_steps`` takes what oracle.Lattice.run_steps
    takes and returns what it returns, for consecutive calls on the same lattice.  ``info`` mirrors cetkmc_remelt_info
    (n_appended is the engine's own business and is not modelled).  ``stats`` says what the run exercised, for the tests
    that check their own inputs: the updates at which something melted, melted voxels found occupied again (in front of an
    update or at the end of a call, ``refilled``, the largest count seen; in front of a latent-heat update with prev_state
    still 0, so that they release heat, ``latent_refills``) and
    the kinds of melted voxels (atoms with an empty neighbour = listed, atoms without = interior, state 4)."""

    def __init__(self, lat, threshold):
        self.lat, self.threshold = lat, threshold
        self.applied_g = -1         # a call that stopped with status 2 ON an update step has applied that step's update and melt
        self.info = dict(passes=0, n_melted=0, n_melted_last=0)
        self.ever = np.zeros(lat.state.shape, bool)      # melted at some pass
        self.stats = dict(melting=[], refilled=0, latent_refills=0, listed=0, interior=0, state4=0)
        self.min_gap = np.inf       # smallest |T - threshold| / |threshold| over the occupied voxels at a decision

    def melt(self, g=-1):
        lat = self.lat
        occ = lat.state != 0
        if occ.any() and np.isfinite(self.threshold):
            with np.errstate(invalid="ignore"):
                gap = np.abs(lat.T[occ] - self.threshold) / abs(self.threshold)
            gap = gap[np.isfinite(gap)]
            if len(gap):
                self.min_gap = min(self.min_gap, float(gap.min()))
        with np.errstate(invalid="ignore"):
            m = occ & (lat.T >= self.threshold)
        if m.any():
            self.stats["melting"].append(g)
            self.stats["state4"] += int((m & (lat.state == 4)).sum())
            atoms = m & (lat.state != 4)
            nb = empty_neighbour(lat.state)
            self.stats["listed"] += int((atoms & nb).sum())
            self.stats["interior"] += int((atoms & ~nb).sum())
            self.ever |= m
        k = remelt(lat, self.threshold)
        self.info["passes"] += 1
        self.info["n_melted"] += k
        self.info["n_melted_last"] = k
        return k

    def _seen_refilled(self):
        self.stats["refilled"] = max(self.stats["refilled"], int((self.ever & (self.lat.state != 0)).sum()))

    def run_steps(self, step0, n, defect_fraction, u_pick, u_defect, u_np, rng_mode=0, seed=0, thermal_mode=1, thermal_dt=1e-6,
                  q_planes=None, use_latent=True):
        lat = self.lat
        skip_g, self.applied_g = self.applied_g, -1
        u_np = np.zeros(0) if u_np is None else np.asarray(u_np, np.float64)
        s, np_pos, q_idx, status = 0, 0, 0, 0
        totals, events, nev, dts = [], [], [], []
        while s < n and status == 0:
            g = step0 + s
            if thermal_mode and g % 20 == 0:
                if s == 0 and g == skip_g:
                    q_idx += thermal_mode == 2          # its plane was consumed by the stopped call; no update, no melt
                else:
                    self._seen_refilled()
                    if thermal_mode == 1:
                        lat.thermal_cet(thermal_dt, scrub_nan=True)
                    else:
                        if use_latent:
                            self.stats["latent_refills"] += int((self.ever & (lat.prev_state == 0) & (lat.state != 0)).sum())
                        lat.thermal_laser(thermal_dt, q_planes[q_idx], prev_state=None if use_latent else lat.state,
                                          scrub_nan=True, update_prev=True)
                        q_idx += 1
                    self.melt(g)
            nxt = min(n, s + 20 - g % 20) if thermal_mode else n
            m = nxt - s
            if rng_mode == 2:       # every uniform counter based: the oracle's single-domain super-steps
                r = lat.run_supersteps(g, m, lat.L, defect_fraction, seed, thermal_mode=0, want_events=True)
                events.append(r["events"].reshape(-1))
                dts.append(r["dt_event"])
            else:
                r = lat.run_steps(g, m, defect_fraction, u_pick[s:nxt], None if u_defect is None else u_defect[s:nxt],
                                  u_np[np_pos:], rng_mode=rng_mode, seed=seed, thermal_mode=0)
                events.append(r["events"])
                nev.append(r["n_events"])
                np_pos += r["np_used"]
            totals.append(r["totals"])
            s += r["done"]
            status = r["status"]
        self._seen_refilled()
        if status == 2 and thermal_mode and s < n and (step0 + s) % 20 == 0:
            self.applied_g = step0 + s
        out = dict(done=s, status=status,
                   q_used=0 if thermal_mode != 2 else updates_in(step0, n if status == 0 else min(s + 1, n)),
                   totals=np.concatenate(totals) if totals else np.zeros(0),
                   events=np.concatenate(events) if events else np.zeros(0, dtype=[("type", "<i4")]))
        if rng_mode == 2:
            out["dt_event"] = np.concatenate(dts) if dts else np.zeros(0)
        else:
            out["np_used"] = np_pos
            out["n_events"] = np.concatenate(nev) if nev else np.zeros(0, np.int64)
        return out
