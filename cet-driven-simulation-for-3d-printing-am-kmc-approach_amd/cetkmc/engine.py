"""Engine: one lattice resident on the GPU, driven through the C ABI (include/cetkmc.h)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Counters, EnsAnalysis, EnsArgs, Event, LaneTableInfo, LocalArgs, Params, RunArgs, RunResult, SuperArgs, SweepInfo, build_library  # noqa: F401

EVENT_DTYPE = np.dtype([("type", "<i4"), ("pos", "<i4", 3), ("target", "<i4", 3), ("atom", "<i4"),
                        ("rate", "<f8"), ("dep_rank", "<i8"), ("theta", "<f8"), ("phi", "<f8")], align=True)
assert EVENT_DTYPE.itemsize == C.sizeof(Event) == 64
FRONT_DTYPE = np.dtype([("n_front", "<i8"), ("n_skipped", "<i8"), ("pos_sum", "<i8", 3), ("G_sum", "<f8"), ("G_min", "<f8"),
                        ("G_max", "<f8"), ("Gi_sum", "<f8"), ("T_sum", "<f8"), ("n_melt", "<i8"), ("melt_bbox", "<i4", 6)],
                       align=True)
assert FRONT_DTYPE.itemsize == C.sizeof(_lib.FrontStats) == 112
LAYER_DTYPE = np.dtype([("n_occ", "<i8"), ("n_start", "<i8"), ("n_eq", "<i8"), ("seg", "<i8", 3), ("cut", "<i8", 3),
                        ("occ_state", "<i8", 4), ("gb_state", "<i8", 4), ("pad", "<i8")])
assert LAYER_DTYPE.itemsize == C.sizeof(_lib.LayerRec) == 144
GRAIN_DTYPE = np.dtype([("n", "<i8"), ("sum", "<i8", 3), ("sq", "<i8", 6), ("n_state", "<i8", 4), ("nb", "<i8", 4),
                        ("first_theta", "<f8"), ("first_phi", "<f8")])
assert GRAIN_DTYPE.itemsize == C.sizeof(_lib.GrainRec) == 160
SOLID_DTYPE = np.dtype([("n_rec", "<i8"), ("n_bad", "<i8"), ("n_cooling", "<i8"), ("stamp_sum", "<i8"), ("stamp_min", "<i8"),
                        ("stamp_max", "<i8"), ("q", "<i8", 4)])
assert SOLID_DTYPE.itemsize == C.sizeof(_lib.SolidRec) == 80
SOLID_INFO_DTYPE = np.dtype([("n_new", "<i8"), ("n_cleared", "<i8"), ("n_recorded", "<i8")])
assert SOLID_INFO_DTYPE.itemsize == C.sizeof(_lib.SolidInfo) == 24
ORIGIN_DTYPE = np.dtype([("n_occ", "<i8"), ("n_by", "<i8", 4), ("n_unrec", "<i8"), ("n_left", "<i8"), ("ord_sum", "<i8"),
                         ("ord_min", "<i8"), ("ord_max", "<i8"), ("birth", "<i8"), ("pad", "<i8")])
assert ORIGIN_DTYPE.itemsize == C.sizeof(_lib.OriginRec) == 96
ORIGIN_CODES = ("none", "dep", "nuc", "att", "hop", "left")      # code of an origin word (word & 7)

TYPE_BYTES = (b"dep", b"diff", b"nuc", b"att")   # kmc_event_rates.py:72,109,132,158


def library_path():
    return _lib.SO_PATH


def default_params(impurity_c=0.0):
    """cetkmc_params filled from constants.py / thermal_solver.py of this package (same
    expressions as the reference so derived values round identically)."""
    import constants as K
    p = Params()
    p.nu, p.nu_dep = K.NU, K.NU_DEP
    p.E_b[:] = (K.E_B_W, K.E_B_RE, K.E_B_C)
    p.E_diff[:] = (K.E_DIFF_W, K.E_DIFF_RE, K.E_DIFF_C)
    p.kT, p.T_melt, p.I0, p.delta_T_c = K.K_T, float(K.T_MELT), K.I0, float(K.DELTA_T_C)
    p.K_nuc, p.beta_imp_nuc, p.max_imp_frac = float(K.K_NUC), K.BETA_IMP_NUC, K.MAX_IMP_FRACTION
    p.rate_threshold, p.anisotropy, p.impurity_re = K.RATE_THRESHOLD, K.ANISOTROPY_FACTOR, K.IMPURITY_RE
    p.impurity_c = float(impurity_c)
    k_cond, rho, cp = 173.0, 19300.0, 132.0            # thermal_solver.py:6-8
    p.alpha = k_cond / (rho * cp)
    p.inv_dx2 = 1.0 / (K.VOXEL_SIZE * K.VOXEL_SIZE)
    p.T_clip_lo, p.T_clip_hi, p.T_nan = float(K.T_SUB), K.T_MELT * 1.1, float(K.T_SUB)
    p.rho_cp = rho * cp
    p.latent_coef = 200e3 / cp
    return p


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def texture_edges_deg(n_bins, span_deg):
    """The n_bins - 1 interior edges of n_bins equal steps over 0..span_deg, in degrees (ascending)."""
    return np.arange(1, int(n_bins), dtype=np.float64) * (float(span_deg) / int(n_bins))


def _texture_args(n_bins, gb_edges_deg, pole_edges_deg, axis):
    """(TextureArgs, the arrays it points into, gb edge angles, pole edge angles): the edges go to the library as
    np.cos(np.deg2rad(angles)), cosines of ascending angles = strictly decreasing values; it does the checking."""
    gb_deg = texture_edges_deg(n_bins, 180.0) if gb_edges_deg is None else np.asarray(gb_edges_deg, np.float64).ravel()
    pole_deg = texture_edges_deg(n_bins, 90.0) if pole_edges_deg is None else np.asarray(pole_edges_deg, np.float64).ravel()
    n_edges = max(int(n_bins) - 1, 0)
    if len(gb_deg) != n_edges or len(pole_deg) != n_edges:
        raise ValueError(f"n_bins = {n_bins} takes {n_edges} interior edges, got {len(gb_deg)} and {len(pole_deg)}")
    keep = (np.ascontiguousarray(np.cos(np.deg2rad(gb_deg))), np.ascontiguousarray(np.cos(np.deg2rad(pole_deg))))
    a = _lib.TextureArgs()
    a.n_bins = int(n_bins)
    a.gb_edges, a.pole_edges = (_dptr(keep[0]), _dptr(keep[1])) if n_edges else (None, None)
    a.axis[:] = [float(x) for x in axis]
    return a, keep, gb_deg, pole_deg


def _default_ar_threshold():
    import constants as K
    return K.CET_AR_THRESHOLD


def _default_inv_dx():
    import constants as K
    return 1.0 / K.VOXEL_SIZE


def default_solid_scales():
    """The quantisation scales (G, gi, cool, T_s) of the solidification profile (cetkmc_solid_args.qscale) when the caller
    gives none: the quantities are counted in steps of 2^-24 of a natural unit -- T_MELT per voxel edge for the two
    gradients (K/m), T_MELT per microsecond for the cooling rate (K/s), T_MELT for the temperature (K).  A value saturates
    (the voxel counts as bad) at 2^14 of these units, far outside the clip range of the temperature update."""
    import constants as K
    u = 2.0 ** 24 / float(K.T_MELT)
    return (u * K.VOXEL_SIZE, u * K.VOXEL_SIZE, u * 1e-6, u)


def _solid_args(scales):
    a = _lib.SolidArgs()
    a.qscale[:] = [float(x) for x in (default_solid_scales() if scales is None else scales)]
    return a


def _solid_fields(buf):
    return {f: buf[f].copy() for f in SOLID_DTYPE.names}


def _origin_fields(buf):
    return {f: buf[f].copy() for f in ORIGIN_DTYPE.names if f != "pad"}


def origin_decode(words):
    """(ordinal int64, -1 for none; code uint8) of origin words ((ordinal + 1) << 3 | code)."""
    w = np.asarray(words, np.uint64)
    return (w >> np.uint64(3)).astype(np.int64) - 1, (w & np.uint64(7)).astype(np.uint8)


def device_count():
    """Number of HIP devices this process can see (0 when there is none)."""
    n = C.c_int(0)
    if _lib.load().cetkmc_device_count(C.byref(n)):
        return 0
    return n.value


THERMAL_SCHEMES = {"explicit": 0, "implicit": 1}        # CETKMC_THERMAL_EXPLICIT / _IMPLICIT


def _scheme_value(scheme, where="set_thermal_scheme"):
    """a scheme by name ("explicit", "implicit") or by the library's integer value (which the library checks); anything else
    is a ValueError naming the wrapper"""
    if isinstance(scheme, str) and scheme in THERMAL_SCHEMES:
        return THERMAL_SCHEMES[scheme]
    if isinstance(scheme, (int, np.integer)) and not isinstance(scheme, bool):
        return int(scheme)
    raise ValueError(f"{where}: the scheme must be 'explicit', 'implicit' or a CETKMC_THERMAL_* value (got {scheme!r})")


def implicit_coeffs(L, r):
    """cetkmc_implicit_coeffs: (inv, p), the Thomas coefficients of (I - r D) along a line of L voxels (DESIGN.md section
    26), computed on the host in double.  Needs no GPU."""
    lib = _lib.load()
    inv, p = np.zeros(max(int(L), 0)), np.zeros(max(int(L), 0))
    if lib.cetkmc_implicit_coeffs(int(L), float(r), _dptr(inv), _dptr(p)):
        raise ValueError("cetkmc: " + lib.cetkmc_last_error().decode(errors="replace"))
    return inv, p


FACES = ("i_lo", "i_hi", "j_lo", "j_hi", "k_lo", "k_hi")        # CETKMC_FACE_*: i_lo the substrate side, i_hi the top


def implicit_coeffs_bc(L, r, beta_lo, beta_hi):
    """cetkmc_implicit_coeffs_bc: (inv, p) of one axis whose two faces carry beta_lo, beta_hi; both 0:
    the bits of ``implicit_coeffs``.  Needs no GPU."""
    lib = _lib.load()
    inv, p = np.zeros(max(int(L), 0)), np.zeros(max(int(L), 0))
    if lib.cetkmc_implicit_coeffs_bc(int(L), float(r), float(beta_lo), float(beta_hi), _dptr(inv), _dptr(p)):
        raise ValueError("cetkmc: " + lib.cetkmc_last_error().decode(errors="replace"))
    return inv, p


def _boundary_struct(boundary, where):
    """None (adiabatic), a _lib.ThermalBoundary, or a mapping with ``beta`` and optionally ``T_ext``, ``ramp`` (six values each,
    in the order of FACES) -> a pointer argument for the setters; the library checks the values"""
    if boundary is None:
        return None
    if isinstance(boundary, _lib.ThermalBoundary):
        return C.byref(boundary)
    try:
        cols = [np.asarray(boundary.get(n, np.zeros(6)) if n != "beta" else boundary["beta"], np.float64).reshape(6)
                for n in ("beta", "T_ext", "ramp")]
    except (AttributeError, KeyError, TypeError, ValueError):
        raise ValueError(f"{where}: the boundary must be None or a mapping with six 'beta' (and 'T_ext', 'ramp') values in the "
                         f"order {FACES} (got {boundary!r})") from None
    b = _lib.ThermalBoundary()
    for n, col in zip(("beta", "T_ext", "ramp"), cols):
        getattr(b, n)[:] = [float(x) for x in col]
    return C.byref(b)


def _beam_struct(table, L, where, keep):
    """a beam table -- a mapping with ``u0``, ``amp`` (n_u), ``gj`` and ``gk`` (n_u, L), ``fi`` (depth),
    as thermal_solver.beam_table returns it -- as a _lib.Beam; the arrays it points to are appended to ``keep``.  Shapes are
    checked here, values by the library."""
    try:
        amp = np.ascontiguousarray(table["amp"], np.float64).reshape(-1)
        gj, gk = (np.ascontiguousarray(table[n], np.float64) for n in ("gj", "gk"))
        fi = np.ascontiguousarray(table["fi"], np.float64).reshape(-1)
        u0 = int(table.get("u0", 0))
    except (AttributeError, KeyError, TypeError, ValueError):
        raise ValueError(f"{where}: a beam table is a mapping with 'u0', 'amp', 'gj', 'gk' and 'fi' (got {table!r})") from None
    if gj.shape != (amp.size, L) or gk.shape != (amp.size, L):
        raise ValueError(f"{where}: gj and gk must have the shape (n_u, L) = ({amp.size}, {L}) (got {gj.shape}, {gk.shape})")
    keep += [amp, gj, gk, fi]
    b = _lib.Beam()
    b.u0, b.n_u, b.depth = u0, amp.size, fi.size
    b.amp, b.gj, b.gk, b.fi = _dptr(amp), _dptr(gj), _dptr(gk), _dptr(fi)
    return b


SHIFT_T_MODES = {"value": 0, "edge": 1}      # CETKMC_SHIFT_T_VALUE, _EDGE


def _shift_struct(d, fill_state=0, fill_T=None, T_mode="value", fill_theta=0.0, fill_phi=0.0):
    """a cetkmc_shift record; T_mode by name, or a number passed through for the library to judge"""
    if fill_T is None:
        import constants as K
        fill_T = float(K.T_SUB)
    s = _lib.Shift()
    s.d[:] = [int(x) for x in d]
    s.fill_state = int(fill_state)
    s.T_mode = SHIFT_T_MODES[T_mode] if isinstance(T_mode, str) else int(T_mode)
    s.pad = 0
    s.fill_T, s.fill_theta, s.fill_phi = float(fill_T), float(fill_theta), float(fill_phi)
    return s


def _shift_info(info):
    return dict(calls=int(info.calls), kept=int(info.kept), exposed=int(info.exposed), dropped=[int(x) for x in info.dropped])


def _info_dict(info):
    """an info record of the library (a ctypes structure of integers) as a dict"""
    return {n: int(getattr(info, n)) for n, _ in info._fields_}


class _ThermalSettings:
    """How a temperature update is made (DESIGN.md sections 25-28): the setters and info records that :class:`Engine` and
    :class:`Ensemble` share.  The class names the symbol prefix of its setters (``_SET``) and itself (``_WHO``, which the
    ValueErrors of a wrapper carry); the getters are the same symbols for both."""

    def _set(self, name, value):
        self._ck(getattr(self.lib, self._SET + name)(self.h, value))

    def _get_info(self, name, record):
        info = record()
        self._ck(getattr(self.lib, name)(self.h, C.byref(info)))
        return _info_dict(info)

    def _boundary_get(self):
        b, info = _lib.ThermalBoundary(), _lib.BoundaryInfo()
        self._ck(self.lib.cetkmc_get_thermal_boundary(self.h, C.byref(b), C.byref(info)))
        return {n: [float(x) for x in getattr(b, n)] for n, _ in b._fields_}, _info_dict(info)

    # -- sub-stepped temperature updates ------------------------------------------
    def set_thermal_substeps(self, n):
        """cetkmc_set_thermal_substeps: every temperature update of the handle becomes ``n`` applications of the explicit
        step with ``dt / n`` (1: as before).  Ensemble (cetkmc_ensemble_set_thermal_substeps): one sub-step count for every
        replica's temperature updates in ``run``."""
        self._set("set_thermal_substeps", int(n))

    def substep_info(self):
        """cetkmc_get_substep_info: dict(updates, substeps, launches, blocked_launches), running totals of the updates made
        while thermal_substeps > 1.  Ensemble: of the ensemble handle, the totals of its calls."""
        return self._get_info("cetkmc_get_substep_info", _lib.SubstepInfo)

    # -- implicit temperature updates ---------------------------------------------
    def set_thermal_scheme(self, scheme):
        """cetkmc_set_thermal_scheme: "explicit" (the default) or "implicit" -- every temperature update becomes
        ``thermal_substeps`` locally one-dimensional backward-Euler steps.  Ensemble (cetkmc_ensemble_set_thermal_scheme):
        every replica's temperature update in ``run``."""
        self._set("set_thermal_scheme", _scheme_value(scheme, self._WHO + ".set_thermal_scheme"))

    def implicit_info(self):
        """cetkmc_get_implicit_info: dict(updates, steps, launches, coeff_uploads), running totals of the implicit updates."""
        return self._get_info("cetkmc_get_implicit_info", _lib.ImplicitInfo)

    # -- thermal boundary conditions ----------------------------------------------
    def set_thermal_boundary(self, boundary):
        """cetkmc_set_thermal_boundary: None (adiabatic) or dict(beta=, T_ext=, ramp=), six values each in the order of
        ``cetkmc.engine.FACES``; needs the implicit scheme unless every beta is 0.  Ensemble
        (cetkmc_ensemble_set_thermal_boundary): one boundary for all replicas."""
        self._set("set_thermal_boundary", _boundary_struct(boundary, self._WHO + ".set_thermal_boundary"))

    def thermal_boundary(self):
        """the boundary as set: dict(beta, T_ext, ramp) of six floats each (all zero: adiabatic)"""
        return self._boundary_get()[0]

    def boundary_info(self):
        """dict(updates, steps, launches, coeff_uploads): running totals of the updates made with a non-adiabatic boundary"""
        return self._boundary_get()[1]

    # -- beam tables ----------------------------------------------------------------
    def beam_info(self):
        """cetkmc_get_beam_info: dict(updates, steps, launches, table_uploads), running totals of the updates whose source was
        a row of a beam table.  Ensemble: the totals of its calls."""
        return self._get_info("cetkmc_get_beam_info", _lib.BeamInfo)


class Engine(_ThermalSettings):
    """Owns a cetkmc handle.  ``n_slabs>1`` splits the lattice into axis-0 slabs on the same
    GPU (decomposition check); ``rank/nranks/unique_id`` selects the one-process-per-GPU
    RCCL mode."""

    _SET, _WHO = "cetkmc_", "Engine"

    def __init__(self, L, impurity_c=0.0, params=None, n_slabs=1, device=0, rank=None, nranks=None, unique_id=None,
                 host_comm=None):
        self.lib = _lib.load()
        self.L = int(L)
        self.params = params if params is not None else default_params(impurity_c)
        self.h = C.c_void_p()
        n = C.c_int(0)
        if self.lib.cetkmc_device_count(C.byref(n)) or n.value <= 0:
            raise RuntimeError("cetkmc: no usable HIP device (there is no CPU fallback): " + self.error())
        if rank is None:
            devs = (C.c_int * n_slabs)(*([device] * n_slabs))
            rc = self.lib.cetkmc_create(C.byref(self.params), self.L, n_slabs, devs, C.byref(self.h))
        elif host_comm is not None:
            # bring-up / test transport: collectives relayed through Python callables (see host_transport.py)
            allgather, exchange = host_comm
            self._hc = _lib.HostComm(_lib.ALLGATHER_FN(allgather), _lib.EXCHANGE_FN(exchange), None)     # keep alive
            rc = self.lib.cetkmc_create_rank_host(C.byref(self.params), self.L, int(rank), int(nranks), int(device),
                                                  C.byref(self._hc), C.byref(self.h))
        else:
            rc = self.lib.cetkmc_create_rank(C.byref(self.params), self.L, int(rank), int(nranks), int(device),
                                             unique_id, C.byref(self.h))
        if rc:
            raise RuntimeError("cetkmc_create: " + self.error())
        i0, i1 = C.c_int(0), C.c_int(0)
        self._ck(self.lib.cetkmc_owned_planes(self.h, C.byref(i0), C.byref(i1)))
        self.i0, self.i1 = i0.value, i1.value

    # -- plumbing ---------------------------------------------------------------------
    def error(self):
        return self.lib.cetkmc_last_error().decode(errors="replace")

    def _ck(self, rc):
        if rc:
            raise RuntimeError("cetkmc: " + self.error())

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.cetkmc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        lib = _lib.load()
        if lib.cetkmc_get_unique_id(buf):
            raise RuntimeError("cetkmc_get_unique_id: " + lib.cetkmc_last_error().decode())
        return buf.raw

    def set_impurity_c(self, c):
        self.params.impurity_c = float(c)
        self._ck(self.lib.cetkmc_set_params(self.h, C.byref(self.params)))

    def set_params(self, params=None):
        """cetkmc_set_params: ``params`` (a cetkmc_params; None: ``self.params`` as the caller has edited it) replaces the
        handle's model constants; the next sweep evaluates every rate with them."""
        if params is not None:
            self.params = params
        self._ck(self.lib.cetkmc_set_params(self.h, C.byref(self.params)))

    # -- transfers --------------------------------------------------------------------
    def upload(self, state=None, theta=None, phi=None, T=None, defects=None):
        L = self.L

        def i64(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.int64)
            assert a.shape == (L, L, L)
            return a

        def f64(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64)
            assert a.shape == (L, L, L)
            return a

        s, th, ph, t, d = i64(state), f64(theta), f64(phi), f64(T), i64(defects)
        self._ck(self.lib.cetkmc_upload(self.h, _ptr(s), _ptr(th), _ptr(ph), _ptr(t), _ptr(d)))

    def download(self, state=True, theta=True, phi=True, T=True, defects=False):
        L = self.L
        out = {}
        if state:
            out["state"] = np.zeros((L, L, L), np.int64)
        if theta:
            out["theta"] = np.zeros((L, L, L), np.float64)
        if phi:
            out["phi"] = np.zeros((L, L, L), np.float64)
        if T:
            out["T"] = np.zeros((L, L, L), np.float64)
        if defects:
            out["defects"] = np.zeros((L, L, L), np.int64)
        self._ck(self.lib.cetkmc_download(self.h, _ptr(out.get("state")), _ptr(out.get("theta")), _ptr(out.get("phi")),
                                          _ptr(out.get("T")), _ptr(out.get("defects"))))
        return out

    def upload_planes(self, i_begin, i_end, state=None, theta=None, phi=None, T=None, defects=None):
        n, L = i_end - i_begin, self.L

        def u8(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.uint8)
            assert a.shape == (n, L, L)
            return a

        def f64(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64)
            assert a.shape == (n, L, L)
            return a

        s, th, ph, t, d = u8(state), f64(theta), f64(phi), f64(T), u8(defects)
        self._ck(self.lib.cetkmc_upload_planes(self.h, i_begin, i_end, _ptr(s), _ptr(th), _ptr(ph), _ptr(t), _ptr(d)))

    def download_planes(self, i_begin, i_end, state=True, theta=False, phi=False, T=False, defects=False):
        n, L = i_end - i_begin, self.L
        out = {}
        if state:
            out["state"] = np.zeros((n, L, L), np.uint8)
        if theta:
            out["theta"] = np.zeros((n, L, L), np.float64)
        if phi:
            out["phi"] = np.zeros((n, L, L), np.float64)
        if T:
            out["T"] = np.zeros((n, L, L), np.float64)
        if defects:
            out["defects"] = np.zeros((n, L, L), np.uint8)
        self._ck(self.lib.cetkmc_download_planes(self.h, i_begin, i_end, _ptr(out.get("state")), _ptr(out.get("theta")),
                                                 _ptr(out.get("phi")), _ptr(out.get("T")), _ptr(out.get("defects"))))
        return out

    def set_defects(self, mask):
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        assert m.shape == (self.L,) * 3
        self._ck(self.lib.cetkmc_set_defects(self.h, _ptr(m)))

    def set_prev_state(self, prev=None):
        p = None if prev is None else np.ascontiguousarray(prev, dtype=np.int64)
        self._ck(self.lib.cetkmc_set_prev_state(self.h, _ptr(p)))

    # -- thermal ------------------------------------------------------------------------
    def thermal_cet(self, dt=1e-6, scrub_nan=True):
        self._ck(self.lib.cetkmc_thermal_cet(self.h, float(dt), int(bool(scrub_nan))))

    def thermal_laser(self, dt, q_top, use_latent=True, scrub_nan=False):
        q = np.ascontiguousarray(q_top, dtype=np.float64)
        assert q.shape == (self.L, self.L)
        self._ck(self.lib.cetkmc_thermal_laser(self.h, float(dt), _ptr(q), int(bool(use_latent)), int(bool(scrub_nan))))

    def set_beam(self, table):
        """cetkmc_set_beam: the source of every laser-mode update becomes a row of ``table`` (thermal_solver.beam_table: u0,
        amp, gj, gk, fi); None removes the beam.  Needs the implicit scheme.  The table is copied to the device."""
        if table is None:
            self._ck(self.lib.cetkmc_set_beam(self.h, None))
            return
        keep = []
        b = _beam_struct(table, self.L, "Engine.set_beam", keep)
        self._ck(self.lib.cetkmc_set_beam(self.h, C.byref(b)))

    def thermal_beam(self, dt, u, use_latent=True, scrub_nan=False):
        """cetkmc_thermal_beam: one update now from the beam table's row of update ordinal ``u``"""
        self._ck(self.lib.cetkmc_thermal_beam(self.h, float(dt), int(u), int(bool(use_latent)), int(bool(scrub_nan))))

    # -- single-step primitives -----------------------------------------------------------
    def rate_sweep(self):
        info = SweepInfo()
        self._ck(self.lib.cetkmc_rate_sweep(self.h, C.byref(info)))
        return info.total, info.n_events, info.n_dep

    def select(self, r):
        ev = Event()
        self._ck(self.lib.cetkmc_select(self.h, float(r), C.byref(ev)))
        return ev

    def apply(self, ev, theta_new=0.0, phi_new=0.0, make_defect=False):
        self._ck(self.lib.cetkmc_apply(self.h, C.byref(ev), float(theta_new), float(phi_new), int(bool(make_defect))))

    def enumerate_events(self, cap=None):
        n = C.c_int64(0)
        self._ck(self.lib.cetkmc_enumerate_events(self.h, None, 0, C.byref(n)))
        cap = n.value if cap is None else min(cap, n.value)
        buf = np.zeros(max(cap, 1), dtype=EVENT_DTYPE)
        if cap:
            self._ck(self.lib.cetkmc_enumerate_events(self.h, _ptr(buf), cap, C.byref(n)))
        return buf[:cap], n.value

    def row_sums(self):
        L = self.L
        rs = np.zeros((L, 3, L), np.float64)
        rc = np.zeros((L, 3, L), np.int32)
        self._ck(self.lib.cetkmc_row_sums(self.h, _ptr(rs), _ptr(rc)))
        return rs, rc

    # -- batched loop ------------------------------------------------------------------------
    def _run_args(self, step0, n, defect_fraction, u_pick, u_defect, u_np, rng_mode, seed, thermal_mode, thermal_dt, q_planes,
                  use_latent, profile, incremental):
        a = RunArgs()
        u_pick = None if u_pick is None else np.ascontiguousarray(u_pick, dtype=np.float64)     # rng_mode 2: no host streams
        u_defect = None if u_defect is None else np.ascontiguousarray(u_defect, dtype=np.float64)
        u_np = np.zeros(0) if u_np is None else np.ascontiguousarray(u_np, dtype=np.float64)
        q = None if q_planes is None else np.ascontiguousarray(q_planes, dtype=np.float64)
        a.step0, a.n_steps, a.defect_fraction = int(step0), int(n), float(defect_fraction)
        a.u_pick, a.u_defect, a.u_np = _dptr(u_pick), _dptr(u_defect), _dptr(u_np)
        a.np_cap, a.rng_mode, a.seed = len(u_np), int(rng_mode), int(seed)
        a.thermal_mode, a.thermal_dt = int(thermal_mode), float(thermal_dt)
        a.q_planes, a.n_q = _dptr(q), (0 if q is None else q.shape[0])
        a.use_latent, a.profile = int(bool(use_latent)), int(profile)       # profile: False/True/2 (per-phase, see counters())
        a.incremental = int(bool(incremental))
        return a, (u_pick, u_defect, u_np, q)       # (the arrays stay referenced while the pointers are in use)

    def stage_inputs(self, step0, n, defect_fraction, u_pick, u_defect, u_np, rng_mode=0, seed=0, thermal_mode=1,
                     thermal_dt=1e-6, q_planes=None, use_latent=True, profile=False, incremental=False):
        """cetkmc_stage_inputs: the batch's random streams and laser source planes go to the device NOW; the matching
        run_steps(..., staged=True) call copies nothing."""
        a, keep = self._run_args(step0, n, defect_fraction, u_pick, u_defect, u_np, rng_mode, seed, thermal_mode, thermal_dt,
                                 q_planes, use_latent, profile, incremental)
        self._ck(self.lib.cetkmc_stage_inputs(self.h, C.byref(a)))

    def run_steps(self, step0, n, defect_fraction, u_pick, u_defect, u_np, rng_mode=0, seed=0, thermal_mode=1,
                  thermal_dt=1e-6, q_planes=None, use_latent=True, profile=False, want_logs=True, incremental=False, staged=False):
        a, keep = self._run_args(step0, n, defect_fraction, u_pick, u_defect, u_np, rng_mode, seed, thermal_mode, thermal_dt,
                                 q_planes, use_latent, profile, incremental)
        if staged:       # same arguments as the stage_inputs call; the library checks the batch shape and copies nothing
            a.u_pick = a.u_defect = a.u_np = a.q_planes = None
        res = RunResult()
        totals = np.zeros(n + 1, np.float64) if want_logs else None
        events = np.zeros(max(n, 1), dtype=EVENT_DTYPE) if want_logs else None
        nev = np.zeros(max(n, 1), np.int64) if want_logs else None
        self._ck(self.lib.cetkmc_run_steps(self.h, C.byref(a), C.byref(res), _ptr(totals), _ptr(events), _ptr(nev)))
        done = res.steps_done
        out = dict(done=int(done), status=int(res.status), np_used=int(res.np_used), q_used=int(res.q_used),
                   nucleation_count=int(res.nucleation_count), sweep_ms_total=res.sweep_ms_total,
                   sweep_launches=int(res.sweep_launches), wall_ms=res.wall_ms, full_sweeps=int(res.full_sweeps),
                   min_margin=float(res.min_margin))
        if want_logs:
            out.update(totals=totals[:done + (1 if res.status == 1 else 0)], events=events[:done], n_events=nev[:done])
        return out

    def counters(self, reset=False):
        """cetkmc_get_counters as a dict: work issued (deferred_steps: steps whose event the next sweep launch applied),
        bytes moved, per-phase device ms of the profile=2 runs."""
        c = Counters()
        self._ck(self.lib.cetkmc_get_counters(self.h, C.byref(c), int(bool(reset))))
        return {n: getattr(c, n) for n, _ in Counters._fields_}

    def lane_table(self):
        """cetkmc_lane_table as a dict (tests): fresh, chunks, usable, poisoned, builds, builds_thermal."""
        info = LaneTableInfo()
        self._ck(self.lib.cetkmc_lane_table(self.h, C.byref(info)))
        return {n: int(getattr(info, n)) for n, _ in LaneTableInfo._fields_}

    def lane_table_arrays(self):
        """cetkmc_lane_table_copy (tests): the owned chunks' sums (f64) and count bytes (u8), each (planes, L, chunks per row)."""
        n = self.lane_table()["chunks"]
        sums, counts = np.empty(n, np.float64), np.empty(n, np.uint8)
        self._ck(self.lib.cetkmc_lane_table_copy(self.h, sums.ctypes.data, counts.ctypes.data, n))
        shape = (self.i1 - self.i0, self.L, n // ((self.i1 - self.i0) * self.L))
        return sums.reshape(shape), counts.reshape(shape)

    # -- Mode B: synchronous super-steps over (L/box)^3 boxes (not in the reference; include/cetkmc.h) --------
    def run_supersteps(self, step0, n, box, defect_fraction, seed, thermal_mode=1, thermal_dt=1e-6, q_planes=None,
                       use_latent=True, want_events=False, null_events=False):
        """box == L: the single-domain case (one Mode A step per super-step, counter uniforms of box 0).
        Returns also ``dt_event`` (time increment per executed event of every super-step, kmc_simulation.py:331-332
        restated; identical on every rank) -- simulated time advances by ``n_exec[g] * dt_event[g]`` with n_exec summed
        over ranks."""
        a = SuperArgs()
        q = None if q_planes is None else np.ascontiguousarray(q_planes, dtype=np.float64)
        a.step0, a.n_steps, a.box, a.defect_fraction, a.seed = int(step0), int(n), int(box), float(defect_fraction), int(seed)
        a.thermal_mode, a.thermal_dt = int(thermal_mode), float(thermal_dt)
        a.q_planes, a.n_q, a.use_latent = _dptr(q), (0 if q is None else q.shape[0]), int(bool(use_latent))
        a.null_events = int(bool(null_events))
        # boxes of this handle: the box layers of its owned planes (across ranks every rank runs its own boxes and logs
        # their events / executed counts; global box order = rank order)
        nbx = self.L // int(box) if box and self.L % int(box) == 0 else 1
        D = max(1, (self.i1 - self.i0) // int(box)) * nbx * nbx if box and self.L % int(box) == 0 else 1
        return self._supersteps(self.lib.cetkmc_run_supersteps, a, n, D, (D,) if want_events else None)

    def _supersteps(self, call, a, n, D, event_shape, more=()):
        """A cetkmc_run_supersteps* ``call`` of n super-steps over D boxes: its output arrays (events of shape (n,) +
        event_shape, or none; ``more``: (name, dtype) of the (n,) logs it takes behind dt_event) and its result dict."""
        res = RunResult()
        totals = np.zeros(n + 1, np.float64)
        n_exec = np.zeros(max(n, 1), np.int64)
        dt_event = np.zeros(max(n, 1), np.float64)
        events = None if event_shape is None else np.zeros((max(n, 1),) + event_shape, dtype=EVENT_DTYPE)
        logs = {name: np.zeros(max(n, 1), dtype) for name, dtype in more}
        self._ck(call(self.h, C.byref(a), C.byref(res), _ptr(totals), _ptr(events), _ptr(n_exec), _ptr(dt_event),
                      *[_ptr(v) for v in logs.values()]))
        done = int(res.steps_done)
        return dict(done=done, status=int(res.status), q_used=int(res.q_used), nucleation_count=int(res.nucleation_count),
                    wall_ms=res.wall_ms, totals=totals[:done + (1 if res.status == 1 else 0)], n_exec=n_exec[:done],
                    events=None if events is None else events[:done], domains=D, dt_event=dt_event[:done],
                    **{name: v[:done] for name, v in logs.items()})

    def run_supersteps_local(self, step0, n, defect_fraction, seed, max_events, horizon_events, thermal_mode=1, thermal_dt=1e-6,
                             want_events=False):
        """Mode B with a local event loop (cetkmc_run_supersteps_local; box 8): every box executes up to ``max_events``
        events per super-step, until its waiting times pass the horizon ``horizon_events / R_max``.  Returns the keys of
        run_supersteps plus ``horizon`` (tau of every super-step) and ``n_capped`` (boxes stopped by max_events); events are
        shaped (n, D, max_events), unused slots of type -1."""
        a = LocalArgs()
        a.step0, a.n_steps, a.box, a.defect_fraction, a.seed = int(step0), int(n), 8, float(defect_fraction), int(seed)
        a.thermal_mode, a.thermal_dt = int(thermal_mode), float(thermal_dt)
        a.max_events, a.horizon_events = int(max_events), float(horizon_events)
        D = max(1, self.L // 8) ** 3
        K = min(max(int(max_events), 1), 64)
        return self._supersteps(self.lib.cetkmc_run_supersteps_local, a, n, D, (D, K) if want_events else None,
                                more=(("horizon", np.float64), ("n_capped", np.int64)))

    # -- grain clustering (utils.get_clusters on the device) --------------------------------------
    def clusters(self, threshold=0.5, labels=False):
        """dict(first (n,3) int32, size (n,) int64, bbox (n,6) int32[, labels (L,L,L) int32]); clusters are
        numbered in the reference's order (first voxel, row-major)."""
        out = self._cluster_table(self._recluster(threshold, True))
        if labels:
            lab = np.zeros((self.L,) * 3, np.int32)
            self._ck(self.lib.cetkmc_cluster_labels(self.h, _ptr(lab)))
            out["labels"] = lab
        return out

    def import_clusters(self, labels):
        """cetkmc_cluster_import: install ``labels`` (L, L, L) -- 0 = empty, ids 1..n numbered by first occurrence in
        row-major order; anything else is refused with the offending voxel named -- as the handle's last clustering, for
        ``layer_profile(recluster=False)`` and the table calls.  Labels are not checked against the state.  Returns the
        table as ``clusters(labels=False)`` does: dict(first, size, bbox)."""
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        assert lab.shape == (self.L,) * 3, lab.shape
        n = C.c_int64(0)
        self._ck(self.lib.cetkmc_cluster_import(self.h, _ptr(lab), C.byref(n)))
        self._cc_n = n.value
        return self._cluster_table(n.value)

    _cc_n = None        # grains of the handle's last clustering, when it was made through this object

    def _recluster(self, threshold, recluster):
        """cetkmc_cluster with ``threshold`` unless ``recluster`` is False; returns ``_cc_n``."""
        if recluster:
            n = C.c_int64(0)
            self._ck(self.lib.cetkmc_cluster(self.h, float(threshold), C.byref(n)))
            self._cc_n = n.value
        return self._cc_n

    def _cluster_table(self, k):
        """dict(first, size, bbox) of the k grains of the handle's clustering (cetkmc_cluster_stats)."""
        first = np.zeros((max(k, 1), 3), np.int32)
        size = np.zeros(max(k, 1), np.int64)
        bbox = np.zeros((max(k, 1), 6), np.int32)
        if k:
            self._ck(self.lib.cetkmc_cluster_stats(self.h, k, _ptr(first), _ptr(size), _ptr(bbox)))
        return dict(first=first[:k], size=size[:k], bbox=bbox[:k])

    # -- sparse site queries (defect model / species counts without full-lattice transfers) -------
    def species_counts(self):
        c = np.zeros(6, np.int64)
        self._ck(self.lib.cetkmc_species_counts(self.h, _ptr(c)))
        return c

    def gather_species(self, species):
        """(linear indices ascending, T at those voxels) of the owned voxels in state ``species``."""
        n = C.c_int64(0)
        self._ck(self.lib.cetkmc_gather_species(self.h, int(species), None, None, 0, C.byref(n)))
        k = n.value
        idx = np.zeros(max(k, 1), np.int64)
        Tv = np.zeros(max(k, 1), np.float64)
        if k:
            self._ck(self.lib.cetkmc_gather_species(self.h, int(species), _ptr(idx), _ptr(Tv), k, C.byref(n)))
        order = np.argsort(idx[:k], kind="stable")
        return idx[:k][order], Tv[:k][order]

    def set_defects_sparse(self, lin_idx):
        a = np.ascontiguousarray(lin_idx, dtype=np.int64)
        self._ck(self.lib.cetkmc_set_defects_sparse(self.h, _ptr(a) if len(a) else None, len(a)))

    def front_stats(self, inv_dx=None):
        """cetkmc_front_stats (solidification-front diagnostics) of the resident lattice as a dict:
        n_front, n_skipped, n_melt (int), pos_sum (3,) int64, G_sum, G_min, G_max, Gi_sum, T_sum (float), melt_bbox (6,)
        int32.  ``inv_dx`` defaults to 1 / constants.VOXEL_SIZE.  metrics.front_metrics turns it into the row's columns."""
        buf = np.zeros(1, dtype=FRONT_DTYPE)
        self._ck(self.lib.cetkmc_front_stats(self.h, float(_default_inv_dx() if inv_dx is None else inv_dx), _ptr(buf)))
        rec = buf[0]
        return {n: (rec[n].copy() if rec[n].ndim else rec[n].item()) for n in FRONT_DTYPE.names}

    def layer_profile(self, threshold=0.5, ar_threshold=None, recluster=True):
        """cetkmc_layer_profile (layer-resolved grain structure) of the resident lattice: a dict of
        int64 arrays with leading dimension L (plane i of the build direction) -- n_occ, n_start, n_eq (L,), seg, cut (L, 3),
        occ_state, gb_state (L, 4).  Clusters first with ``threshold`` unless ``recluster`` is False, which reuses the
        handle's last clustering (Engine.clusters; the lattice must not have changed since).  ``ar_threshold`` defaults to
        constants.CET_AR_THRESHOLD.  metrics.layer_metrics turns it into the row's columns.  The ensemble's own handle
        (replica 0) is refused: Ensemble.layer_profile covers every replica."""
        self._recluster(threshold, recluster)
        buf = np.zeros(max(self.L, 1), dtype=LAYER_DTYPE)
        self._ck(self.lib.cetkmc_layer_profile(self.h, float(_default_ar_threshold() if ar_threshold is None else ar_threshold),
                                               _ptr(buf)))
        return {n: buf[n].copy() for n in LAYER_DTYPE.names if n != "pad"}

    def texture_profile(self, n_bins=36, gb_edges_deg=None, pole_edges_deg=None, axis=(1.0, 0.0, 0.0), threshold=0.5,
                        recluster=True):
        """cetkmc_texture_profile (grain-boundary misorientation and pole histograms) of the resident
        lattice: a dict of int64 arrays with leading dimension L (plane i of the build direction) -- gb_hist (L, 3, n_bins):
        the grain-grain faces of the plane across each lattice axis by misorientation bin; pole_hist (L, n_bins): its
        occupied voxels by the angle between their orientation vector (or its opposite) and ``axis``; bad (L, 4): faces per
        axis / voxels whose value is not finite -- plus the interior edge angles used, ``gb_edges_deg`` and
        ``pole_edges_deg`` (n_bins - 1 ascending degrees each; bin b lies between edge b - 1 and edge b, a value exactly on
        an edge belongs to the bin above it).  The defaults are equal steps over 0..180 degrees (boundaries) and 0..90
        degrees (pole).  ``axis`` is used as given, not normalised.  The model attaches no crystal frame to the lattice:
        reading component 0 of the orientation vectors against lattice axis 0, the build direction, is this project's
        convention for the default axis.  Clusters first with ``threshold`` unless ``recluster`` is False, which reuses the
        handle's last clustering or import (the lattice must not have changed since).  metrics.texture_metrics turns the
        profile into columns.  The ensemble's own handle is refused: Ensemble.texture_profile covers every replica."""
        self._recluster(threshold, recluster)
        a, _keep, gb_deg, pole_deg = _texture_args(n_bins, gb_edges_deg, pole_edges_deg, axis)
        nb, L = max(int(n_bins), 1), max(self.L, 1)
        gb, pole, bad = np.zeros((L, 3, nb), np.int64), np.zeros((L, nb), np.int64), np.zeros((L, 4), np.int64)
        self._ck(self.lib.cetkmc_texture_profile(self.h, C.byref(a), _ptr(gb), _ptr(pole), _ptr(bad)))
        return dict(gb_hist=gb, pole_hist=pole, bad=bad, gb_edges_deg=gb_deg, pole_edges_deg=pole_deg)

    def grain_table(self, threshold=0.5, recluster=True):
        """cetkmc_grain_table (per-grain table) of the resident lattice: a dict of arrays with leading
        dimension n, entry id - 1 for grain id -- n (n,), sum (n, 3), sq (n, 6: ii, jj, kk, ij, ik, jk), n_state (n, 4), nb
        (n, 4: same, other, empty, outside over the clustering's 14-offset stencil), all int64, and first_theta, first_phi
        (n,) float64, the stored angles of the grain's first voxel bit for bit.  Clusters first with ``threshold`` unless
        ``recluster`` is False, which reuses the handle's last clustering or import (the lattice must not have changed
        since).  metrics.grain_metrics turns it into columns.  The ensemble's own handle is refused: Ensemble.grain_table
        covers every replica."""
        k = self._recluster(threshold, recluster)
        if k is None:
            # a clustering this object did not make (or none: then the call fails in the library's words): every grain
            # has n >= 1, so the first record left at zero ends the table
            cap = 1024
            while True:
                buf = np.zeros(cap, dtype=GRAIN_DTYPE)
                self._ck(self.lib.cetkmc_grain_table(self.h, cap, _ptr(buf)))
                k = int(np.count_nonzero(buf["n"]))
                if k < cap or cap >= self.L ** 3:
                    break
                cap *= 4
        else:
            buf = np.zeros(max(k, 1), dtype=GRAIN_DTYPE)
            self._ck(self.lib.cetkmc_grain_table(self.h, k, _ptr(buf)))
        return {f: buf[f][:k].copy() for f in GRAIN_DTYPE.names}

    # -- solidification map ----------------------------------------------------
    def solid_begin(self):
        """cetkmc_solid_begin: start (or reset) the handle's solidification map -- no voxel has a record, the voxels
        occupied now are substrate, the snapshots hold the current state and T."""
        self._ck(self.lib.cetkmc_solid_begin(self.h))

    def solid_end(self):
        """cetkmc_solid_end: free the map."""
        self._ck(self.lib.cetkmc_solid_end(self.h))

    def solid_update(self, stamp, dt, inv_dx=None):
        """cetkmc_solid_update: record every voxel that solidified since the last update (stamp, its T, the gradient of
        front_stats, cool = (T - T at the last update) / dt), clear those that emptied, refresh the snapshots.  Returns
        dict(n_new, n_cleared, n_recorded).  ``inv_dx`` defaults to 1 / constants.VOXEL_SIZE."""
        info = np.zeros(1, SOLID_INFO_DTYPE)
        self._ck(self.lib.cetkmc_solid_update(self.h, int(stamp), float(_default_inv_dx() if inv_dx is None else inv_dx), float(dt),
                                              _ptr(info)))
        return {f: int(info[f][0]) for f in SOLID_INFO_DTYPE.names}

    def solid_read(self):
        """cetkmc_solid_read: the map as dict(stamp (L,L,L) int64, T_s (L,L,L), g (L,L,L,3), cool (L,L,L) float64)."""
        L = self.L
        out = dict(stamp=np.zeros((L,) * 3, np.int64), T_s=np.zeros((L,) * 3), g=np.zeros((L, L, L, 3)), cool=np.zeros((L,) * 3))
        self._ck(self.lib.cetkmc_solid_read(self.h, _ptr(out["stamp"]), _ptr(out["T_s"]), _ptr(out["g"]), _ptr(out["cool"])))
        return out

    def solid_profile(self, scales=None, grains=False, threshold=0.5, recluster=True):
        """cetkmc_solid_profile: dict(layers=..., grains=...) of int64 field arrays (n_rec, n_bad, n_cooling, stamp_sum,
        stamp_min, stamp_max, q (.., 4): the quantised sums of G, gi, cool, T_s) with leading dimension L (plane i of the
        build direction) and, with ``grains``, n (grain id - 1 of the handle's last clustering; None otherwise).
        ``scales`` defaults to :func:`default_solid_scales`; a mean is q / (n_rec * scale).  With ``grains`` the call
        clusters first with ``threshold`` unless ``recluster`` is False, which reuses the last clustering or import."""
        a = _solid_args(scales)
        lay = np.zeros(max(self.L, 1), SOLID_DTYPE)
        if not grains:
            self._ck(self.lib.cetkmc_solid_profile(self.h, C.byref(a), _ptr(lay), 0, None))
            return dict(layers=_solid_fields(lay), grains=None)
        k = self._recluster(threshold, recluster)
        if k is None:       # a clustering this object did not make: its size from the stats call (fails without one)
            k = len(self.grain_table(recluster=False)["n"])
        gr = np.zeros(max(k, 1), SOLID_DTYPE)
        self._ck(self.lib.cetkmc_solid_profile(self.h, C.byref(a), _ptr(lay), k, _ptr(gr)))
        return dict(layers=_solid_fields(lay), grains=_solid_fields(gr[:k]))

    # -- origin map --------------------------------------------------------------
    def origin_begin(self):
        """cetkmc_origin_begin: start (or reset) the handle's origin map -- no voxel has a record, the census is zero, the
        map's clock is 0.  From now on every stepping call and ``apply`` folds its executed events into the map."""
        self._ck(self.lib.cetkmc_origin_begin(self.h))

    def origin_end(self):
        """cetkmc_origin_end: free the map."""
        self._ck(self.lib.cetkmc_origin_end(self.h))

    def origin_absorb(self, events, group=1):
        """cetkmc_origin_absorb_events: host records (EVENT_DTYPE), ``group`` consecutive records per ordinal."""
        ev = np.ascontiguousarray(events, dtype=EVENT_DTYPE).ravel()
        self._ck(self.lib.cetkmc_origin_absorb_events(self.h, _ptr(ev) if len(ev) else None, len(ev), int(group)))

    def origin_words(self):
        """cetkmc_origin_read: the raw (L, L, L) uint64 words, ((ordinal + 1) << 3) | code, 0 = no record."""
        w = np.zeros((self.L,) * 3, np.uint64)
        self._ck(self.lib.cetkmc_origin_read(self.h, _ptr(w)))
        return w

    def origin_read(self):
        """The map as dict(ordinal (L,L,L) int64, -1 = no record; code (L,L,L) uint8: 0 none, 1 dep, 2 nuc, 3 att, 4 hop,
        5 left)."""
        o, c = origin_decode(self.origin_words())
        return dict(ordinal=o, code=c)

    def origin_census(self):
        """cetkmc_origin_census: (L, 5) int64 events absorbed per build plane -- dep, diff (left), nuc, att, diff (arrived)."""
        c = np.zeros((max(self.L, 1), 5), np.int64)
        self._ck(self.lib.cetkmc_origin_census(self.h, _ptr(c)))
        return c

    def origin_seq(self):
        """cetkmc_origin_seq: the map's clock (ordinal of the next absorbed step); -1 without a map."""
        return int(self.lib.cetkmc_origin_seq(self.h))

    def origin_profile(self, grains=False, threshold=0.5, recluster=True):
        """cetkmc_origin_profile: dict(layers=..., grains=...) of int64 field arrays (n_occ, n_by (.., 4: dep, nuc, att,
        hop), n_unrec, n_left, ord_sum, ord_min, ord_max, birth) with leading dimension L (plane i of the build direction)
        and, with ``grains``, n (grain id - 1 of the handle's last clustering; None otherwise).  With ``grains`` the call
        clusters first with ``threshold`` unless ``recluster`` is False, which reuses the last clustering or import."""
        lay = np.zeros(max(self.L, 1), ORIGIN_DTYPE)
        if not grains:
            self._ck(self.lib.cetkmc_origin_profile(self.h, _ptr(lay), 0, None))
            return dict(layers=_origin_fields(lay), grains=None)
        k = self._recluster(threshold, recluster)
        if k is None:       # a clustering this object did not make: its size from the table call (fails without one)
            k = len(self.grain_table(recluster=False)["n"])
        gr = np.zeros(max(k, 1), ORIGIN_DTYPE)
        self._ck(self.lib.cetkmc_origin_profile(self.h, _ptr(lay), k, _ptr(gr)))
        return dict(layers=_origin_fields(lay), grains=_origin_fields(gr[:k]))

    # -- remelting ---------------------------------------------------------------
    def set_remelt(self, on, threshold=None):
        """cetkmc_set_remelt: with ``on`` every temperature-update step of ``run_steps`` turns the occupied voxels with
        T >= ``threshold`` (default: the handle's T_melt) into empty ones, behind the update and before the step's rates."""
        self._ck(self.lib.cetkmc_set_remelt(self.h, int(bool(on)), float(self.params.T_melt if threshold is None else threshold)))

    def remelt(self, threshold=None):
        """cetkmc_remelt: one pass now.  Returns the counters as ``remelt_info`` does."""
        info = _lib.RemeltInfo()
        self._ck(self.lib.cetkmc_remelt(self.h, float(self.params.T_melt if threshold is None else threshold), C.byref(info)))
        return _info_dict(info)

    def time_remelt(self, n, threshold=None):
        """cetkmc_time_remelt: device ms of n passes (one hipEvent pair), measurement only."""
        ms = C.c_double(0.0)
        self._ck(self.lib.cetkmc_time_remelt(self.h, float(self.params.T_melt if threshold is None else threshold), int(n), C.byref(ms)))
        return ms.value

    def remelt_info(self):
        """cetkmc_get_remelt_info: dict(passes, n_melted, n_melted_last, n_appended), running totals of the handle as read
        at the end of the last stepping call or direct pass."""
        info = _lib.RemeltInfo()
        self._ck(self.lib.cetkmc_get_remelt_info(self.h, C.byref(info)))
        return _info_dict(info)

    def time_thermal(self, n_updates, laser=False):
        """cetkmc_time_thermal: device ms of n_updates temperature updates (dt = 1e-6 s, one hipEvent pair).  The updates are
        real: afterwards the handle's field has advanced by ``n_updates`` updates (``laser``: with the plane of the last
        ``thermal_laser``, zeros before the first, and the latent-heat term)."""
        ms = C.c_double(0.0)
        self._ck(self.lib.cetkmc_time_thermal(self.h, int(bool(laser)), int(n_updates), C.byref(ms)))
        return ms.value

    # -- the lattice shifted on the device ----------------------------------------
    def shift(self, d, fill_state=0, fill_T=None, T_mode="value", fill_theta=0.0, fill_phi=0.0):
        """cetkmc_shift: voxel v of the lattice moves to v + d on the device; the exposed voxels take ``fill_state``, mask 0,
        ``fill_theta`` / ``fill_phi`` and, as T, ``fill_T`` (None: constants.T_SUB) under ``T_mode`` "value" or the old field
        continued outward under "edge".  The maps move along.  Afterwards the handle stands as after an upload of the five new
        fields.  Returns dict(calls, kept, exposed, dropped[6])."""
        info = _lib.ShiftInfo()
        self._ck(self.lib.cetkmc_shift(self.h, C.byref(_shift_struct(d, fill_state, fill_T, T_mode, fill_theta, fill_phi)), C.byref(info)))
        return _shift_info(info)

    def time_shift(self, d, **kw):
        """cetkmc_time_shift: :meth:`shift` between two hipEvents; returns (info, device ms).  Measurement only."""
        if isinstance(self, _Replica):
            raise ValueError("Engine.time_shift: a replica is timed through Ensemble.time_shift (replica 0's handle is the ensemble's)")
        info, ms = _lib.ShiftInfo(), C.c_double(0.0)
        self._ck(self.lib.cetkmc_time_shift(self.h, C.byref(_shift_struct(d, **kw)), C.byref(info), C.byref(ms)))
        return _shift_info(info), ms.value

    def nucleation_count(self):
        return int(self.lib.cetkmc_nucleation_count(self.h))

    def reset_counters(self):
        self._ck(self.lib.cetkmc_reset_counters(self.h))

    def time_sweeps(self, n):
        ms = C.c_double(0.0)
        self._ck(self.lib.cetkmc_time_sweeps(self.h, int(n), C.byref(ms)))
        return ms.value

    def event_overhead(self, n=50):
        """ms between two back-to-back hipEvents around an EMPTY kernel: the part of a hipEvent-bracketed kernel time that is
        not the kernel's."""
        ms = C.c_double(0.0)
        self._ck(self.lib.cetkmc_event_overhead(self.h, int(n), C.byref(ms)))
        return ms.value

    def comm_selftest(self, nbytes=4096, timed=True):
        """Collective transport check of a multi-rank engine (every rank calls it): patterned all-gather and neighbour
        exchange verified on the host; raises with the library's message when the data is wrong.  Returns
        {"allgather_us", "exchange_us"} (averages of 20 further calls, stream synchronisation included) or None."""
        t = (C.c_double * 2)(0.0, 0.0)
        self._ck(self.lib.cetkmc_comm_selftest(self.h, int(nbytes), t if timed else None))
        return {"bytes": int(nbytes), "allgather_us": t[0], "exchange_us": t[1]} if timed else None

    def set_option(self, key, value):
        self._ck(self.lib.cetkmc_set_option(self.h, key.encode(), int(value)))

    def sync(self):
        self._ck(self.lib.cetkmc_sync(self.h))


class _Replica(Engine):
    """Replica r of an :class:`Ensemble`: every per-lattice call of :class:`Engine` on that lattice.  The handle belongs to
    the ensemble (closing the replica does not release it)."""

    def __init__(self, ens, r, handle):       # noqa: D107 -- no Engine.__init__: the lattice exists already
        self.lib, self.L, self.params = ens.lib, ens.L, ens.params[r]
        self.h = handle
        self.i0, self.i1 = 0, ens.L
        self._ens = ens                        # keeps the ensemble alive while the replica is in use

    def close(self):
        self.h = None


class Ensemble(_ThermalSettings):
    """R independent lattices of edge L (1 <= L <= 128) on one GPU, stepped together (cetkmc_create_ensemble /
    cetkmc_run_ensemble).  ``params`` is one cetkmc_params per replica (they may differ in
    impurity_c and nu_dep only); ``replica(r)`` is an :class:`Engine` view of lattice r for uploads, downloads and the
    analysis calls."""

    _SET, _WHO = "cetkmc_ensemble_", "Ensemble"

    def __init__(self, L, params, device=0):
        self.lib = _lib.load()
        self.L, self.R = int(L), len(params)
        self.params = list(params)
        self.h = C.c_void_p()
        n = C.c_int(0)
        if self.lib.cetkmc_device_count(C.byref(n)) or n.value <= 0:
            raise RuntimeError("cetkmc: no usable HIP device (there is no CPU fallback): " + self.error())
        arr = (Params * max(self.R, 1))(*self.params)
        if self.lib.cetkmc_create_ensemble(arr, self.L, self.R, int(device), C.byref(self.h)):
            self.h = None
            raise RuntimeError("cetkmc_create_ensemble: " + self.error())
        self._reps = []
        for r in range(self.R):
            hr = C.c_void_p()
            self._ck(self.lib.cetkmc_ensemble_replica(self.h, r, C.byref(hr)))
            self._reps.append(_Replica(self, r, hr))

    def error(self):
        return self.lib.cetkmc_last_error().decode(errors="replace")

    def _ck(self, rc):
        if rc:
            raise RuntimeError("cetkmc: " + self.error())

    def replica(self, r):
        return self._reps[r]

    def close(self):
        if getattr(self, "h", None):
            for e in self._reps:
                e.h = None
            self.lib.cetkmc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_beam(self, tables, set_of=None):
        """cetkmc_ensemble_set_beam: ``tables`` is a sequence of beam tables (thermal_solver.beam_table) that share u0, n_u and
        depth; replica r reads table ``set_of[r]`` (None: table r, one per replica).  None removes the beam."""
        if tables is None:
            self._ck(self.lib.cetkmc_ensemble_set_beam(self.h, 0, None, None))
            return
        keep = []
        arr = (_lib.Beam * max(len(tables), 1))(*[_beam_struct(t, self.L, "Ensemble.set_beam", keep) for t in tables])
        so = None if set_of is None else np.ascontiguousarray(np.asarray(set_of, dtype=np.int32).reshape(-1))
        if so is not None and so.size != self.R:
            raise ValueError(f"Ensemble.set_beam: set_of needs one entry per replica ({self.R}), got {so.size}")
        self._ck(self.lib.cetkmc_ensemble_set_beam(self.h, len(tables), arr, None if so is None else so.ctypes.data_as(C.POINTER(C.c_int32))))

    def run(self, step0, n, defect_fraction, u_pick=None, u_defect=None, u_np=None, rng_mode=0, seeds=None, thermal_mode=1,
            thermal_dt=1e-6, q_planes=None, q_set=None, use_latent=True):
        """n lockstep steps of every live replica from global step step0.  rng_mode 0: u_pick / u_defect (R, n) and
        u_np (R, np_stride >= n * (L*L + 2)) from each replica's own generators; rng_mode 2: ``seeds`` (R,).
        thermal_mode 2 (laser source + latent heat): ``q_planes`` (n_sets, n_q, L, L), plane u of a set feeding the u-th
        temperature update of the call (None when the call holds no update); ``q_set`` (R,) names the set of each replica
        (None: set r for replica r, n_sets == R).  Returns dict(done, status, np_used, q_used, nucleation_count,
        min_margin (R,), totals (R, n + 1), dt (R, n) (rng_mode 2), wall_ms)."""
        R, n = self.R, int(n)
        df = np.ascontiguousarray(np.broadcast_to(np.asarray(defect_fraction, dtype=np.float64), (R,)))
        a = EnsArgs()
        a.step0, a.n_steps, a.defect_fraction = int(step0), n, _dptr(df)
        keep = [df]
        if rng_mode == 0:
            u_pick = np.ascontiguousarray(u_pick, dtype=np.float64).reshape(R, n)
            u_np = np.ascontiguousarray(u_np, dtype=np.float64).reshape(R, -1)
            u_defect = None if u_defect is None else np.ascontiguousarray(u_defect, dtype=np.float64).reshape(R, n)
            a.u_pick, a.u_defect, a.u_np, a.np_stride = _dptr(u_pick), _dptr(u_defect), _dptr(u_np), u_np.shape[1]
            keep += [u_pick, u_np, u_defect]
        else:
            sd = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(R))
            a.seed = sd.ctypes.data_as(C.POINTER(C.c_uint64))
            keep.append(sd)
        a.rng_mode, a.thermal_mode, a.thermal_dt = int(rng_mode), int(thermal_mode), float(thermal_dt)
        if int(thermal_mode) == 2:
            qs = None if q_set is None else np.ascontiguousarray(np.asarray(q_set, dtype=np.int32).reshape(R))
            if q_planes is None:
                q, a.n_q, a.n_sets = None, 0, (R if qs is None else int(qs.max()) + 1)
            else:
                q = np.ascontiguousarray(q_planes, dtype=np.float64)
                assert q.ndim == 4 and q.shape[2:] == (self.L, self.L), q.shape
                a.n_sets, a.n_q = q.shape[0], q.shape[1]
            a.q_planes, a.use_latent = _dptr(q), int(bool(use_latent))
            a.q_set = None if qs is None else qs.ctypes.data_as(C.POINTER(C.c_int32))
            keep += [q, qs]
        res = (RunResult * R)()
        totals = np.zeros((R, n + 1), np.float64)
        dt = np.zeros((R, max(n, 1)), np.float64)
        self._ck(self.lib.cetkmc_run_ensemble(self.h, C.byref(a), res, _ptr(totals), _ptr(dt) if rng_mode == 2 else None))
        return dict(done=np.array([x.steps_done for x in res], np.int64), status=np.array([x.status for x in res], np.int32),
                    np_used=np.array([x.np_used for x in res], np.int64), q_used=np.array([x.q_used for x in res], np.int64),
                    nucleation_count=np.array([x.nucleation_count for x in res], np.int64),
                    min_margin=np.array([x.min_margin for x in res], np.float64), totals=totals, dt=dt[:, :n],
                    wall_ms=float(res[0].wall_ms) if R else 0.0)

    def shift(self, records):
        """cetkmc_ensemble_shift: one record per replica, each a dict of :meth:`Engine.shift`'s arguments (``d`` and the
        fills) or None, which leaves the replica untouched like d = (0, 0, 0).  Returns one info dict per replica."""
        records = list(records)
        if len(records) != self.R:
            raise ValueError(f"Ensemble.shift: {len(records)} records for {self.R} replicas")
        buf = (_lib.Shift * max(self.R, 1))()
        for r, rec in enumerate(records):
            buf[r] = _shift_struct(**rec) if rec is not None else _shift_struct((0, 0, 0))
        info = (_lib.ShiftInfo * max(self.R, 1))()
        self._ck(self.lib.cetkmc_ensemble_shift(self.h, buf, info))
        return [_shift_info(info[r]) for r in range(self.R)]

    def time_shift(self, records):
        """cetkmc_time_shift on the ensemble's handle: :meth:`shift` between two hipEvents; returns (infos, device ms)."""
        records = list(records)
        if len(records) != self.R:
            raise ValueError(f"Ensemble.time_shift: {len(records)} records for {self.R} replicas")
        buf = (_lib.Shift * max(self.R, 1))(*[_shift_struct(**rec) if rec is not None else _shift_struct((0, 0, 0)) for rec in records])
        info, ms = (_lib.ShiftInfo * max(self.R, 1))(), C.c_double(0.0)
        self._ck(self.lib.cetkmc_time_shift(self.h, buf, info, C.byref(ms)))
        return [_shift_info(info[r]) for r in range(self.R)], ms.value

    def set_remelt(self, on, threshold=None):
        """cetkmc_ensemble_set_remelt: remelting in ``run`` for every replica, one threshold (default: T_melt, which the
        replicas share)."""
        thr = float(self.params[0].T_melt if threshold is None else threshold)
        self._ck(self.lib.cetkmc_ensemble_set_remelt(self.h, int(bool(on)), thr))

    def remelt_info(self):
        """cetkmc_ensemble_remelt_info: one dict(passes, n_melted, n_melted_last, n_appended) per replica."""
        buf = (_lib.RemeltInfo * max(self.R, 1))()
        self._ck(self.lib.cetkmc_ensemble_remelt_info(self.h, buf))
        return [_info_dict(buf[r]) for r in range(self.R)]

    def analyze(self, threshold=0.5, species=-1, labels=True):
        """Clustering, species counts, nucleation counts and (species >= 0) the sorted (index, T) gather of every replica,
        in launches that do not depend on R.  Returns one dict per replica: clusters (as Engine.clusters), counts (as
        Engine.species_counts), nucleation_count and, for species >= 0, gather (as Engine.gather_species)."""
        R, n = self.R, self.L ** 3
        nc, cnt, nuc, ng = (np.zeros(R, np.int64), np.zeros((R, 6), np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64))
        a = EnsAnalysis()
        a.threshold, a.species = float(threshold), int(species)
        a.n_clusters, a.species_counts = nc.ctypes.data_as(C.POINTER(C.c_int64)), cnt.ctypes.data_as(C.POINTER(C.c_int64))
        a.nucleation_count, a.n_gathered = nuc.ctypes.data_as(C.POINTER(C.c_int64)), ng.ctypes.data_as(C.POINTER(C.c_int64))
        self._ck(self.lib.cetkmc_ensemble_analyze(self.h, C.byref(a)))
        self._an_nc = nc.copy()
        gt = int(ng.sum())
        lab = np.zeros((R,) + (self.L,) * 3, np.int32) if labels else None
        gi, gT = np.zeros(max(gt, 1), np.int64), np.zeros(max(gt, 1), np.float64)
        tables = self._cluster_tables(nc, lab, gi if species >= 0 else None, gT if species >= 0 else None)
        out, g0 = [], 0
        for r, cl in enumerate(tables):
            if labels:
                cl["labels"] = lab[r]
            d = dict(clusters=cl, counts=cnt[r], nucleation_count=int(nuc[r]))
            if species >= 0:
                m = int(ng[r])
                idx, Tv = gi[g0:g0 + m], gT[g0:g0 + m]
                order = np.argsort(idx, kind="stable")
                d["gather"] = (idx[order], Tv[order])
                g0 += m
            out.append(d)
        return out

    _an_nc = None       # grains per replica of the last analysis or import

    def _cluster_tables(self, nc, labels=None, lin_idx=None, T_vals=None):
        """One dict(first, size, bbox) per replica of the analysis in force, ``nc`` grains per replica
        (cetkmc_ensemble_analysis_data, which also fills the arrays given for its labels and gather)."""
        at = np.concatenate(([0], np.cumsum(nc[:self.R]))).astype(np.int64)
        tot = int(at[-1])
        first = np.zeros((max(tot, 1), 3), np.int32)
        size = np.zeros(max(tot, 1), np.int64)
        bbox = np.zeros((max(tot, 1), 6), np.int32)
        self._ck(self.lib.cetkmc_ensemble_analysis_data(self.h, _ptr(first), _ptr(size), _ptr(bbox), _ptr(labels), _ptr(lin_idx),
                                                        _ptr(T_vals)))
        return [dict(first=first[at[r]:at[r + 1]], size=size[at[r]:at[r + 1]], bbox=bbox[at[r]:at[r + 1]]) for r in range(self.R)]

    def _reanalyze(self, threshold, recluster, what=None):
        """:meth:`analyze` (without downloading labels) unless ``recluster`` is False; returns the offsets of every
        replica's grains in the concatenated tables ((R + 1,) int64).  Without an analysis made through this object:
        raises in the name of Ensemble.``what``, or (``what`` None) returns None and leaves the refusal to the library."""
        if recluster:
            self.analyze(threshold, labels=False)
        if self._an_nc is None:
            if what is None:
                return None
            raise RuntimeError(f"cetkmc: Ensemble.{what} needs a preceding Ensemble.analyze")
        return np.concatenate(([0], np.cumsum(self._an_nc))).astype(np.int64)

    def import_clusters(self, labels):
        """cetkmc_ensemble_cluster_import: Engine.import_clusters for every replica at once, ``labels`` (R, L, L, L), in
        place of the clustering of the last :meth:`analyze` (required; its counts and gather stay).  One bad replica
        refuses the call and leaves the analysis as it was.  Returns one dict(first, size, bbox) per replica."""
        R = self.R
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        assert lab.shape == (R,) + (self.L,) * 3, lab.shape
        nc = np.zeros(max(R, 1), np.int64)
        self._ck(self.lib.cetkmc_ensemble_cluster_import(self.h, _ptr(lab), _ptr(nc)))
        self._an_nc = nc[:R].copy()
        return self._cluster_tables(nc)

    def front_stats(self, inv_dx=None):
        """cetkmc_ensemble_front_stats: Engine.front_stats of every replica (frozen ones included) in launches that do not
        depend on R.  A dict of arrays with leading dimension R; entry r has the bits of replica(r).front_stats()."""
        buf = np.zeros(max(self.R, 1), dtype=FRONT_DTYPE)
        self._ck(self.lib.cetkmc_ensemble_front_stats(self.h, float(_default_inv_dx() if inv_dx is None else inv_dx), _ptr(buf)))
        return {n: buf[n][:self.R].copy() for n in FRONT_DTYPE.names}

    def layer_profile(self, threshold=0.5, ar_threshold=None, recluster=True):
        """cetkmc_ensemble_layer_profile: Engine.layer_profile of every replica (frozen ones included) in launches that do
        not depend on R.  A dict of int64 arrays with leading dimensions (R, L).  Runs :meth:`analyze` first (without
        downloading labels) unless ``recluster`` is False, which reuses the last analysis."""
        self._reanalyze(threshold, recluster)
        buf = np.zeros((max(self.R, 1), self.L), dtype=LAYER_DTYPE)
        self._ck(self.lib.cetkmc_ensemble_layer_profile(
            self.h, float(_default_ar_threshold() if ar_threshold is None else ar_threshold), _ptr(buf)))
        return {n: buf[n][:self.R].copy() for n in LAYER_DTYPE.names if n != "pad"}

    def texture_profile(self, n_bins=36, gb_edges_deg=None, pole_edges_deg=None, axis=(1.0, 0.0, 0.0), threshold=0.5,
                        recluster=True):
        """cetkmc_ensemble_texture_profile: Engine.texture_profile of every replica (frozen ones included) in one launch
        whatever R.  The int64 arrays gain the leading dimension R: gb_hist (R, L, 3, n_bins), pole_hist (R, L, n_bins), bad
        (R, L, 4).  Runs :meth:`analyze` first (without downloading labels) unless ``recluster`` is False, which reuses the
        last analysis or import."""
        self._reanalyze(threshold, recluster)
        a, _keep, gb_deg, pole_deg = _texture_args(n_bins, gb_edges_deg, pole_edges_deg, axis)
        nb, L, R = max(int(n_bins), 1), self.L, max(self.R, 1)
        gb, pole, bad = np.zeros((R, L, 3, nb), np.int64), np.zeros((R, L, nb), np.int64), np.zeros((R, L, 4), np.int64)
        self._ck(self.lib.cetkmc_ensemble_texture_profile(self.h, C.byref(a), _ptr(gb), _ptr(pole), _ptr(bad)))
        return dict(gb_hist=gb[:self.R], pole_hist=pole[:self.R], bad=bad[:self.R], gb_edges_deg=gb_deg, pole_edges_deg=pole_deg)

    def grain_table(self, threshold=0.5, recluster=True):
        """cetkmc_ensemble_grain_table: Engine.grain_table of every replica (frozen ones included) in launches that do not
        depend on R.  Returns one dict per replica, as :meth:`analyze` lays out its per-cluster data; entry r has the bits
        of replica(r).grain_table().  Runs :meth:`analyze` first (without downloading labels) unless ``recluster`` is
        False, which reuses the last analysis or import."""
        if not recluster and self._an_nc is None:            # no analysis yet: fails in the library's words
            self._ck(self.lib.cetkmc_ensemble_grain_table(self.h, None))
        at = self._reanalyze(threshold, recluster, "grain_table")
        buf = np.zeros(max(int(at[-1]), 1), dtype=GRAIN_DTYPE)
        self._ck(self.lib.cetkmc_ensemble_grain_table(self.h, _ptr(buf)))
        return [{f: buf[f][at[r]:at[r + 1]].copy() for f in GRAIN_DTYPE.names} for r in range(self.R)]

    # -- solidification maps of every replica ----------------------------------
    def solid_begin(self):
        """cetkmc_ensemble_solid_begin: Engine.solid_begin for every replica."""
        self._ck(self.lib.cetkmc_ensemble_solid_begin(self.h))

    def solid_end(self):
        self._ck(self.lib.cetkmc_ensemble_solid_end(self.h))

    def solid_update(self, stamp, dt, inv_dx=None):
        """cetkmc_ensemble_solid_update: Engine.solid_update of every replica (frozen ones included) in one launch whatever
        R; stamp, dt and inv_dx are shared.  dict(n_new, n_cleared, n_recorded) of (R,) int64 arrays."""
        info = np.zeros(max(self.R, 1), SOLID_INFO_DTYPE)
        self._ck(self.lib.cetkmc_ensemble_solid_update(self.h, int(stamp), float(_default_inv_dx() if inv_dx is None else inv_dx),
                                                       float(dt), _ptr(info)))
        return {f: info[f][:self.R].copy() for f in SOLID_INFO_DTYPE.names}

    def solid_read(self, r):
        """The map of replica r (Engine.solid_read on its handle)."""
        return self._reps[r].solid_read()

    def solid_profile(self, scales=None, grains=False, threshold=0.5, recluster=True):
        """cetkmc_ensemble_solid_profile: Engine.solid_profile of every replica in launches that do not depend on R.
        dict(layers=field arrays with leading dimensions (R, L), grains=one dict per replica or None).  With ``grains``
        runs :meth:`analyze` first (without downloading labels) unless ``recluster`` is False."""
        a = _solid_args(scales)
        lay = np.zeros((max(self.R, 1), self.L), SOLID_DTYPE)
        if not grains:
            self._ck(self.lib.cetkmc_ensemble_solid_profile(self.h, C.byref(a), _ptr(lay), None))
            return dict(layers=_solid_fields(lay[:self.R]), grains=None)
        at = self._reanalyze(threshold, recluster, "solid_profile(grains=True)")
        gr = np.zeros(max(int(at[-1]), 1), SOLID_DTYPE)
        self._ck(self.lib.cetkmc_ensemble_solid_profile(self.h, C.byref(a), _ptr(lay), _ptr(gr)))
        return dict(layers=_solid_fields(lay[:self.R]), grains=[_solid_fields(gr[at[r]:at[r + 1]]) for r in range(self.R)])

    # -- origin maps of every replica -------------------------------------------
    def origin_begin(self):
        """cetkmc_ensemble_origin_begin: Engine.origin_begin for every replica."""
        self._ck(self.lib.cetkmc_ensemble_origin_begin(self.h))

    def origin_end(self):
        self._ck(self.lib.cetkmc_ensemble_origin_end(self.h))

    def origin_absorb(self, r, events, group=1):
        """Host records into the map of replica r (Engine.origin_absorb on its handle)."""
        self._reps[r].origin_absorb(events, group)

    def origin_read(self, r=None):
        """The map of replica r (Engine.origin_read on its handle); r None: every replica's, arrays (R, L, L, L)."""
        if r is not None:
            return self._reps[r].origin_read()
        maps = [e.origin_read() for e in self._reps]
        return dict(ordinal=np.stack([m["ordinal"] for m in maps]), code=np.stack([m["code"] for m in maps]))

    def origin_seq(self):
        """(R,) int64: every replica's map clock."""
        return np.array([e.origin_seq() for e in self._reps], np.int64)

    def origin_census(self):
        """cetkmc_ensemble_origin_census: (R, L, 5) int64."""
        c = np.zeros((max(self.R, 1), max(self.L, 1), 5), np.int64)
        self._ck(self.lib.cetkmc_ensemble_origin_census(self.h, _ptr(c)))
        return c[:self.R]

    def origin_profile(self, grains=False, threshold=0.5, recluster=True):
        """cetkmc_ensemble_origin_profile: Engine.origin_profile of every replica in launches that do not depend on R.
        dict(layers=field arrays with leading dimensions (R, L), grains=one dict per replica or None).  With ``grains``
        runs :meth:`analyze` first (without downloading labels) unless ``recluster`` is False."""
        lay = np.zeros((max(self.R, 1), self.L), ORIGIN_DTYPE)
        if not grains:
            self._ck(self.lib.cetkmc_ensemble_origin_profile(self.h, _ptr(lay), None))
            return dict(layers=_origin_fields(lay[:self.R]), grains=None)
        at = self._reanalyze(threshold, recluster, "origin_profile(grains=True)")
        gr = np.zeros(max(int(at[-1]), 1), ORIGIN_DTYPE)
        self._ck(self.lib.cetkmc_ensemble_origin_profile(self.h, _ptr(lay), _ptr(gr)))
        return dict(layers=_origin_fields(lay[:self.R]), grains=[_origin_fields(gr[at[r]:at[r + 1]]) for r in range(self.R)])

    def set_defects_sparse(self, lists):
        """Engine.set_defects_sparse for every replica r with lists[r] not None, in launches that do not depend on R."""
        counts = np.array([-1 if x is None else len(x) for x in lists], np.int64)
        idx = [np.asarray(x, np.int64) for x in lists if x is not None and len(x)]
        flat = np.ascontiguousarray(np.concatenate(idx) if idx else np.zeros(1, np.int64))
        self._ck(self.lib.cetkmc_ensemble_set_defects_sparse(self.h, _ptr(counts), _ptr(flat)))
