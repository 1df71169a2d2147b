"""Temperature-field updates on the GPU (drop-in for the reference ``thermal_solver.py``).

Same pure-function interface (arrays in, new array out); the 7-point explicit-Euler stencil
runs in the ``k_thermal`` HIP kernel, bit-identical to ``scipy.ndimage.laplace`` + NumPy
(thermal_solver.py:36-117).  The Gaussian source plane is built on the host with NumPy, like
the reference, so its ``exp`` rounds as the reference's does.
"""
import numpy as np

from constants import LATTICE_SIZE, T_MELT, T_SUB, VOXEL_SIZE

K = 173.0        # [W/m-K]      thermal_solver.py:6
RHO = 19300.0    # [kg/m^3]     :7
CP = 132.0       # [J/kg-K]     :8
ALPHA = K / (RHO * CP)
DEFAULT_BEAM_RADIUS = 50e-6
DEFAULT_ABSORPTIVITY = 0.35

class _EngineCache:
    """Device lattices kept between calls of the pure-function drop-ins, least recently used first out: at most
    ``max_engines`` handles (a 256^3 handle owns ~1.3 GB of HBM); ``close_engines()`` releases them all."""

    def __init__(self, max_engines=2):
        from collections import OrderedDict
        self.max_engines = max_engines
        self._d = OrderedDict()

    def get(self, L, make):
        eng = self._d.pop(L, None)
        if eng is None:
            while len(self._d) >= self.max_engines:
                self._d.popitem(last=False)[1].close()
            eng = make()
        self._d[L] = eng
        return eng

    def close(self):
        while self._d:
            self._d.popitem()[1].close()

    def __len__(self):
        return len(self._d)


_engines = _EngineCache()


def close_engines():
    """Release the cached device lattices of this module."""
    _engines.close()


def _engine(L):
    import cetkmc
    return _engines.get(L, lambda: cetkmc.Engine(L))


def build_temperature_field(L=None):
    """Steady ramp along axis 0: T(i) = T_SUB + (T_MELT-T_SUB)/(L-1) * i (thermal_solver.py:15-34)."""
    if L is None:
        L = LATTICE_SIZE
    slope = (T_MELT - T_SUB) / (L - 1) if L > 1 else 0.0
    column = T_SUB + slope * np.arange(L, dtype=np.float64)
    return np.repeat(np.repeat(column[:, None, None], L, axis=1), L, axis=2)


def laser_source_plane(L, laser_pos, laser_power, beam_radius=DEFAULT_BEAM_RADIUS, absorptivity=DEFAULT_ABSORPTIVITY):
    """Volumetric source [W/m^3] of plane i=L-1 (thermal_solver.py:82-95).  As in the reference,
    ``j0`` centres the beam on BOTH in-plane axes and ``i0`` is ignored (:86)."""
    _i0, j0 = laser_pos
    axis = np.arange(L, dtype=np.float64)
    JJ, KK = np.meshgrid(axis, axis, indexing="ij")
    r_m = np.sqrt((JJ - j0) ** 2 + (KK - j0) ** 2) * VOXEL_SIZE
    peak = laser_power * absorptivity / (np.pi * beam_radius * beam_radius)
    surface = peak * np.exp(-(r_m ** 2) / (beam_radius ** 2))
    return surface / VOXEL_SIZE


SCAN_EVERY = 20      # run_kmc's temperature update cadence (kmc_simulation.py:248)


def stable_substeps(dt, alpha=ALPHA, dx=VOXEL_SIZE):
    """Smallest n >= 1 for which the explicit 7-point update with dt / n is stable: alpha * (dt / n) / dx**2 <= 1/6, the
    quotient evaluated as written (17 for the reference's dt = 1e-6 s, where alpha dt / dx^2 = 2.716).  For the
    ``substeps`` / ``thermal_substeps`` options."""
    dt, alpha, dx = float(dt), float(alpha), float(dx)
    if not (dt > 0.0 and alpha > 0.0 and dx > 0.0) or not np.isfinite(alpha * dt / (dx * dx)):
        raise ValueError("stable_substeps needs positive finite dt, alpha and dx")
    n = max(1, int(np.floor(6.0 * alpha * dt / (dx * dx))))
    while n > 1 and alpha * (dt / (n - 1)) / (dx * dx) <= 1.0 / 6.0:
        n -= 1
    while alpha * (dt / n) / (dx * dx) > 1.0 / 6.0:
        n += 1
    return n


def _check_substeps(substeps):
    if isinstance(substeps, bool) or not isinstance(substeps, (int, np.integer)) or substeps < 1:
        raise ValueError("substeps must be an integer >= 1")
    return int(substeps)


THERMAL_SCHEMES = ("explicit", "implicit")


def _check_scheme(scheme, where="scheme"):
    if scheme not in THERMAL_SCHEMES:
        raise ValueError(f"{where} must be 'explicit' or 'implicit' (got {scheme!r})")
    return scheme


FACES = ("i_lo", "i_hi", "j_lo", "j_hi", "k_lo", "k_hi")        # cetkmc's face order: i_lo the substrate side, i_hi the top


def _face_group(spec, where):
    """(beta, T, fixed) of "adiabatic", ("fixed", T) or ("convective", h [W/m^2-K], T_ambient)"""
    if spec is None or spec == "adiabatic":
        return 0.0, 0.0, False
    try:
        kind = spec[0]
        if kind == "fixed" and len(spec) == 2:
            return 1.0, float(spec[1]), True
        if kind == "convective" and len(spec) == 3:
            return float(spec[1]) * VOXEL_SIZE / K, float(spec[2]), False
    except (TypeError, IndexError, ValueError):
        pass
    raise ValueError(f"thermal_boundary: {where} must be 'adiabatic', ('fixed', T) or ('convective', h, T_ambient) (got {spec!r})")


def thermal_boundary(bottom="adiabatic", top="adiabatic", sides="adiabatic", cooling_rate=0.0, dt=1e-6):
    """The boundary of the implicit temperature updates (not in the reference) as
    dict(beta=, T_ext=, ramp=), six values each in the order FACES.  ``bottom`` is face i_lo, ``top`` face i_hi, ``sides`` the
    four j and k faces; each "adiabatic", ("fixed", T [K]) or ("convective", h [W/m^2-K], T_ambient [K]) with
    beta = h * VOXEL_SIZE / K.  ``cooling_rate`` [K/s] lowers the fixed faces by cooling_rate * dt per temperature update."""
    groups = [_face_group(bottom, "bottom"), _face_group(top, "top")] + [_face_group(sides, "sides")] * 4
    return dict(beta=[g[0] for g in groups], T_ext=[g[1] for g in groups],
                ramp=[-float(cooling_rate) * float(dt) if g[2] else 0.0 for g in groups])


def gradient_boundary(L, T_bottom=T_SUB, T_top=T_MELT, cooling_rate=0.0, dt=1e-6):
    """The two fixed i faces whose ghost temperatures extend ``build_temperature_field``'s ramp by one voxel, so that the ramp
    is a fixed point of the implicit update; every other face adiabatic."""
    slope = (T_top - T_bottom) / (L - 1) if L > 1 else 0.0
    return thermal_boundary(bottom=("fixed", T_bottom - slope), top=("fixed", T_top + slope), cooling_rate=cooling_rate, dt=dt)


def _check_boundary(boundary, scheme, where):
    if boundary is not None and scheme != "implicit":
        raise ValueError(f"{where}: boundary= needs scheme='implicit' (the explicit update is adiabatic)")
    return boundary


def laser_scan_planes(L, laser, first_step, n_steps):
    """Source planes (n, L, L) of the temperature updates that fall in the global steps [first_step, first_step + n_steps):
    one per step g with g % 20 == 0, in step order.  ``laser`` is a dict: ``power`` [W], ``start`` (beam centre at update
    0, in voxels), ``speed`` (voxels per update), optional ``beam_radius`` / ``absorptivity`` (this module's defaults) and
    ``latent`` (read by the stepping loops, not here).  The beam centre of update u = g // 20 is start + speed * u, so a
    plane depends on the global step alone: adjacent ranges concatenate, and a batch that starts again at the same step
    gets the same plane again."""
    first_step, n_steps = int(first_step), int(n_steps)
    u0 = -(-first_step // SCAN_EVERY)                               # first update at or after first_step
    u1 = -(-(first_step + max(n_steps, 0)) // SCAN_EVERY)           # first update at or after the end
    out = np.zeros((max(u1 - u0, 0), L, L), dtype=np.float64)
    start, speed = float(laser["start"]), float(laser["speed"])
    for x, u in enumerate(range(u0, u1)):
        c = start + speed * u
        out[x] = laser_source_plane(L, (c, c), laser["power"], laser.get("beam_radius", DEFAULT_BEAM_RADIUS),
                                    laser.get("absorptivity", DEFAULT_ABSORPTIVITY))
    return out


SCAN_PATTERNS = ("diagonal", "line", "raster", "serpentine")


def scan_path(L, pattern, speed, hatch=None, start=None, margin=0.0):
    """A scan strategy (not in the reference): a function u -> (cj, ck, on) of the update ordinal
    u = g // 20 -- the beam centre in voxels along j and k, and whether the beam is on.  Pure in u, so adjacent ranges of
    updates concatenate and a resumed range gets the same rows (as ``laser_scan_planes``' planes do).
      "diagonal"    cj = ck = start + speed * u (``laser_scan_planes``' path; start defaults to 0); always on
      "line"        one track along +k at j = start (default: the middle, (L - 1) / 2); off behind its end
      "raster"      tracks along +k at j = start + hatch * t (start defaults to margin), each from k = margin; the beam
                    jumps back between tracks
      "serpentine"  as "raster", every odd track along -k from k = L - 1 - margin
    A track of length len = L - 1 - 2 * margin voxels takes n_t = floor(len / speed) + 1 updates; track t = u // n_t,
    position s = u % n_t, ck = margin + speed * s (or L - 1 - margin - speed * s); off once cj passes L - 1 - margin."""
    L, speed, margin = int(L), float(speed), float(margin)
    if pattern not in SCAN_PATTERNS:
        raise ValueError(f"scan_path: pattern must be one of {SCAN_PATTERNS} (got {pattern!r})")
    if not (np.isfinite(speed) and speed > 0.0):
        raise ValueError("scan_path: speed must be positive and finite (voxels per update)")
    if pattern == "diagonal":
        s0 = 0.0 if start is None else float(start)
        return lambda u: (s0 + speed * int(u), s0 + speed * int(u), True)
    length = L - 1 - 2.0 * margin
    if not (margin >= 0.0 and length >= 0.0):
        raise ValueError("scan_path: margin must be >= 0 and leave a track (L - 1 - 2 * margin >= 0)")
    if pattern == "line":
        hatch_v, j0 = 0.0, ((L - 1) / 2.0 if start is None else float(start))
    else:
        if hatch is None or not (np.isfinite(float(hatch)) and float(hatch) > 0.0):
            raise ValueError(f"scan_path: pattern {pattern!r} needs a positive hatch spacing (voxels)")
        hatch_v, j0 = float(hatch), (margin if start is None else float(start))
    n_t = int(np.floor(length / speed)) + 1
    k_lo, k_hi = margin, L - 1 - margin

    def path(u):
        u = int(u)
        if u < 0:
            return j0, k_lo, False
        t, s = divmod(u, n_t)
        cj = j0 + hatch_v * t
        back = pattern == "serpentine" and t % 2 == 1
        ck = k_hi - speed * s if back else k_lo + speed * s
        on = cj <= k_hi and (pattern != "line" or t == 0)
        return cj, ck, bool(on)
    return path


def beam_table(L, path, u0, n_u, power, beam_radius=DEFAULT_BEAM_RADIUS, absorptivity=DEFAULT_ABSORPTIVITY, depth=1,
               penetration=None, cutoff=3.0):
    """The beam table of update ordinals u0 .. u0 + n_u - 1 of ``path`` (``scan_path``) for cetkmc's set_beam (DESIGN.md
    section 28): dict(u0, amp (n_u), gj (n_u, L), gk (n_u, L), fi (depth)).  The Gaussian beam is separable,
    exp(-(dj^2 + dk^2) / r_b^2) = gj[j] * gk[k]: the host's exp runs over 2 L values per update and the device multiplies.
      gj[x][j] = exp(-((j - cj) dx)^2 / r_b^2), exactly 0 where |j - cj| dx > cutoff * r_b; gk likewise
      amp[x]   = power * absorptivity / (pi r_b^2) / dx, 0 where the path is off
      fi       = w / w.sum(), w[d] = exp(-d dx / penetration) over the ``depth`` planes from the top down (uniform for
                 penetration=None, [1.0] for depth 1): the absorbed power is spread over the planes, not multiplied."""
    L, u0, n_u, depth = int(L), int(u0), int(n_u), int(depth)
    if n_u < 1 or not 1 <= depth <= L:
        raise ValueError("beam_table: n_u >= 1 and 1 <= depth <= L")
    r_b, cutoff = float(beam_radius), float(cutoff)
    if not (r_b > 0.0 and np.isfinite(r_b) and cutoff > 0.0):
        raise ValueError("beam_table: a positive finite beam_radius and a positive cutoff")
    axis = np.arange(L, dtype=np.float64)
    amp, gj, gk = np.zeros(n_u), np.zeros((n_u, L)), np.zeros((n_u, L))
    peak = float(power) * float(absorptivity) / (np.pi * r_b * r_b) / VOXEL_SIZE
    for x in range(n_u):
        cj, ck, on = path(u0 + x)
        for g, c in ((gj, cj), (gk, ck)):
            r_m = (axis - c) * VOXEL_SIZE
            g[x] = np.where(np.abs(r_m) > cutoff * r_b, 0.0, np.exp(-(r_m ** 2) / (r_b ** 2)))
        amp[x] = peak if on else 0.0
    if depth == 1:
        fi = np.ones(1)
    else:
        if penetration is not None and not (float(penetration) > 0.0 and np.isfinite(float(penetration))):
            raise ValueError("beam_table: penetration must be positive and finite (metres), or None")
        w = np.ones(depth) if penetration is None else np.exp(-np.arange(depth, dtype=np.float64) * VOXEL_SIZE / float(penetration))
        fi = w / w.sum()
    return dict(u0=u0, amp=amp, gj=gj, gk=gk, fi=fi)


def update_temperature(T, state, prev_state, dt, laser_pos, laser_power,
                       beam_radius=DEFAULT_BEAM_RADIUS, absorptivity=DEFAULT_ABSORPTIVITY, substeps=1, scheme="explicit", boundary=None):
    """Explicit Euler step with Laplacian + Gaussian surface source on i=L-1 + latent heat where
    ``prev_state==0 & state!=0``; clipped to [T_SUB, 1.1*T_MELT] (thermal_solver.py:36-105).  ``substeps=n`` (not in the
    reference): n such steps of dt / n from the same source, the latent heat in the first (``stable_substeps``).
    ``scheme="implicit"`` (not in the reference): the steps are locally one-dimensional backward-Euler steps, stable at any dt
    (DESIGN.md section 26); ``boundary`` (``thermal_boundary``; implicit only): its faces, at update 0 (section 27)."""
    L = T.shape[0]
    assert T.shape == (L, L, L)
    assert state.shape == T.shape and prev_state.shape == T.shape
    substeps = _check_substeps(substeps)
    _check_boundary(boundary, _check_scheme(scheme), "update_temperature")
    eng = _engine(L)
    eng.upload(state=state, T=T)
    eng.set_prev_state(prev_state)
    eng.set_thermal_substeps(substeps)
    try:
        eng.set_thermal_scheme(scheme)
        if boundary is not None:
            eng.set_thermal_boundary(boundary)
        eng.thermal_laser(dt, laser_source_plane(L, laser_pos, laser_power, beam_radius, absorptivity),
                          use_latent=True, scrub_nan=False)
    finally:
        eng.set_thermal_substeps(1)        # the handle is cached
        eng.set_thermal_boundary(None)
        eng.set_thermal_scheme("explicit")
    return eng.download(state=False, theta=False, phi=False, T=True)["T"]


def update_temperature_cet(T, state, dt=1e-6, substeps=1, scheme="explicit", boundary=None):
    """Diffusion-only step used by run_kmc; ``state`` is unused, as in the reference
    (thermal_solver.py:107-117).  ``substeps=n`` (not in the reference): n such steps of dt / n; ``scheme="implicit"`` (not in
    the reference): implicit steps; ``boundary``: as in ``update_temperature``."""
    L = T.shape[0]
    substeps = _check_substeps(substeps)
    _check_boundary(boundary, _check_scheme(scheme), "update_temperature_cet")
    eng = _engine(L)
    eng.upload(T=T)
    eng.set_thermal_substeps(substeps)
    try:
        eng.set_thermal_scheme(scheme)
        if boundary is not None:
            eng.set_thermal_boundary(boundary)
        eng.thermal_cet(dt, scrub_nan=False)
    finally:
        eng.set_thermal_substeps(1)
        eng.set_thermal_boundary(None)
        eng.set_thermal_scheme("explicit")
    return eng.download(state=False, theta=False, phi=False, T=True)["T"]
