"""Sub-stepped temperature updates: the definition in executable form.  Oracle calls only; never
touches the engine.

``update(lat, n, dt, ...)`` is one update with thermal_substeps = n: n oracle updates with dt / n from the same source plane,
the first with the NaN scrub and the latent-heat term, the others with neither.  ``Stepper`` is the stepping loop composed
from it, modelled on tests/remelt_ref.Stepper (whose melt rule it uses when a threshold is given): before a step with
g % 20 == 0 the update (then the melt), then the steps up to the next update with thermal_mode 0, the uniform streams
carried from chunk to chunk.
"""
import numpy as np

from remelt_ref import remelt, updates_in


def new_stats():
    """what the updates of a run exercised, for the tests that check their own inputs"""
    return dict(updates=0, substeps=0, nan_before=0, inf_before=0, on_clip_lo=0, on_clip_hi=0, latent=0, source=0)


def update(lat, n, dt, thermal_mode=1, q=None, use_latent=True, scrub=True, stats=None):
    """One temperature update of ``lat`` (oracle.Lattice) in n sub-steps of dt / n.  thermal_mode 1: thermal_cet; 2:
    thermal_laser with source plane q.  stats (new_stats()) is added to: NaN / inf voxels present before sub-step 1, the
    largest number of voxels on either clip value after a sub-step, latent releases, updates with a non-zero source."""
    dt_s = dt / n                                   # one IEEE division, as the host does
    lo, hi = lat.params.T_clip_lo, lat.params.T_clip_hi
    if stats is not None:
        stats["updates"] += 1
        stats["substeps"] += n
        stats["nan_before"] += int(np.isnan(lat.T).sum())
        stats["inf_before"] += int(np.isinf(lat.T).sum())
        if thermal_mode == 2:
            stats["source"] += int(np.any(np.asarray(q) != 0.0))
            if use_latent:
                stats["latent"] += int(((lat.prev_state == 0) & (lat.state != 0)).sum())
    for s in range(n):
        first = s == 0
        if thermal_mode == 1:
            lat.thermal_cet(dt_s, scrub_nan=bool(scrub and first))
        else:
            lat.thermal_laser(dt_s, q, prev_state=None if (use_latent and first) else lat.state,
                              scrub_nan=bool(scrub and first), update_prev=True)
        if stats is not None:
            stats["on_clip_lo"] = max(stats["on_clip_lo"], int((lat.T == lo).sum()))
            stats["on_clip_hi"] = max(stats["on_clip_hi"], int((lat.T == hi).sum()))


def on_clip(lat):
    """share of voxels on a clip value"""
    return float(((lat.T == lat.params.T_clip_lo) | (lat.T == lat.params.T_clip_hi)).mean())


def max_inplane_difference(T):
    """largest difference between neighbours within a plane (axes 1 and 2: across the planes a field may carry a gradient)"""
    return max(float(np.abs(np.diff(T, axis=a)).max()) for a in (1, 2) if T.shape[a] > 1)


class Stepper:
    """The stepping loop of one lattice with thermal_substeps = n (and, with a threshold, remelting on).  ``run_steps``
    takes what oracle.Lattice.run_steps takes and returns what it returns, for consecutive calls on the same lattice."""

    def __init__(self, lat, n, threshold=None):
        self.lat, self.n, self.threshold = lat, int(n), threshold
        self.applied_g = -1         # a call that stopped with status 2 ON an update step has applied that step's whole update
        self.stats = new_stats()
        self.melted = 0
        self.info = dict(passes=0, n_melted=0, n_melted_last=0)      # mirrors cetkmc_remelt_info for the passes of this loop

    def melt(self, g):
        """the melt pass behind the update of global step g (a subclass may look at the lattice first)"""
        k = remelt(self.lat, self.threshold)
        self.melted += k
        self.info["passes"] += 1
        self.info["n_melted"] += k
        self.info["n_melted_last"] = k
        return k

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
                    q_idx += thermal_mode == 2          # its plane was consumed by the stopped call; no update
                else:
                    update(lat, self.n, thermal_dt, thermal_mode, None if thermal_mode == 1 else q_planes[q_idx],
                           use_latent=use_latent, scrub=True, stats=self.stats)
                    q_idx += thermal_mode == 2
                    if self.threshold is not None:
                        self.melt(g)
            nxt = min(n, s + 20 - g % 20) if thermal_mode else n
            m = nxt - s
            if rng_mode == 2:
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
