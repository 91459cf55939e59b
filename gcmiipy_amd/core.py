"""`Core`: one resident model state on one MI355X behind the C ABI.

This is the fast path: state stays in HBM, `step(n)` launches n fused Matsuno
steps, `get_state()` copies back once.  The reference-shaped drop-in functions
(matsuno_c_grid.py, matsumo_temp.py, dynamics.py ... in this package) are thin
wrappers that move arrays through a cached Core per call.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib


class GcmError(RuntimeError):
    pass


def _check(rc, h=None):
    if rc == _lib.OK:
        return
    msg = lib.gcm_last_error(h).decode() if (h or rc) else ""
    if rc == _lib.ERR_ARG:
        raise ValueError(msg or "gcmcore: bad argument")
    raise GcmError("gcmcore error %d: %s" % (rc, msg))


def _count(n, h):
    """a non-negative int an entry point returned (a count, a flag, a constant), or the error a negative one stands for"""
    if n < 0:
        _check(n, h)
    return n


def as_f64(x, shape=None, name="array"):
    """float64 C-contiguous ndarray of `shape`; mirrors the reference's shape asserts
    (temperature.py:9,17; dynamics.py:203) with ValueError."""
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    if shape is not None and a.shape != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (name, a.shape, tuple(shape)))
    return a


def tracer_array(c, L, H, W):
    """the passive tracers of a GCM_PE25D handle as gcm_set_tracers takes them: float64 C-contiguous
    (n, L, H, W) with 0 <= n <= MAX_TRACERS (None: no tracers); ValueError otherwise"""
    if c is None:
        return np.empty((0, L, H, W))
    a = as_f64(c, name="tracers")
    if a.ndim != 4 or a.shape[1:] != (L, H, W):
        raise ValueError("tracers have shape %s, expected (n, %d, %d, %d)" % (a.shape, L, H, W))
    if a.shape[0] > _lib.MAX_TRACERS:
        raise ValueError("%d tracers: at most %d" % (a.shape[0], _lib.MAX_TRACERS))
    return a


class TracerStats(collections.namedtuple("TracerStats", "min max mass air negative nan")):
    """the device monitor of a GCM_PE25D handle's passive tracers (Core.tracer_stats): one entry per tracer, q last
    where asked for.  min, max: NaN where the field holds a NaN; mass = sum c p dsig_k, the quantity every
    transport scheme conserves; air = sum p dsig_k, the same number in every entry; negative, nan: int64 counts
    of the cells < 0 and of the NaN cells"""
    __slots__ = ()

    @property
    def mean(self):
        """mass / air: the mass-weighted mean mixing ratio"""
        return self.mass / self.air


CLIMATE_WORDS3 = ("u", "v", "theta", "T", "uu", "vv", "TT", "uv", "vT", "vtheta")    # the moments of gcm_get_climate's m3
CLIMATE_WORDS2 = ("p", "pp")                                                           # ... and of its m2


class Climate(collections.namedtuple("Climate", ("n",) + CLIMATE_WORDS3 + CLIMATE_WORDS2)):
    """the zonal-mean climatology of a GCM_PE25D handle (Core.climate): n, the number of samples, and the time and
    zonal means of the moments -- the device's float64 sums divided by W n (NaN where n = 0).  (L, H) arrays: u, v (at
    their own C-grid points), theta, T = theta Pi, uu, vv, TT, uv = uc vc, vT = vc T, vtheta = vc theta, where uc, vc
    are the winds averaged to the cell centre; (H,) arrays: p, pp.  A band: its own rows (bands.merge_climate)"""
    __slots__ = ()

    @property
    def eddy_momentum_flux(self):
        """[u'v'] = uv - [u][v].  uv is the mean of the product at the cell centre, [u] and [v] are the means at the
        winds' own staggered points: the zonal mean of uc IS that of u, the mean of vc is 0.5 ([v][j] + [v][j - 1]),
        approximated here by [v][j] -- exact where [v] does not vary from one row to the next"""
        return self.uv - self.u * self.v

    @property
    def eddy_heat_flux(self):
        """[v'T'] = vT - [v][T], with [v] at its own point (see eddy_momentum_flux)"""
        return self.vT - self.v * self.T

    @property
    def T_variance(self):
        """[T'T'] = TT - [T]^2: the eddy temperature variance"""
        return self.TT - self.T * self.T

    @property
    def eke(self):
        """0.5 (uu - [u]^2 + vv - [v]^2): the eddy kinetic energy per unit mass, winds at their own points"""
        return 0.5 * (self.uu - self.u * self.u + self.vv - self.v * self.v)

    @classmethod
    def from_sums(cls, n, m3, m2, width):
        """the record of the raw sums m3 (10, L, H), m2 (2, H) of n samples of rows of `width` columns"""
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.float64(width) * np.float64(n)
            return cls(int(n), *[m3[w] / d for w in range(len(CLIMATE_WORDS3))], *[m2[w] / d for w in range(len(CLIMATE_WORDS2))])


# the conditional means of gcm_get_plev_climate's words 1 .. 12 (word 0 is the count)
PLEV_WORDS = ("u", "v", "theta", "T", "q", "uu", "vv", "TT", "uv", "vT", "vtheta", "vq")


def plev_array(plev):
    """pressure targets as the C ABI takes them: float64 (N,), 1 <= N <= PLEV_MAX, in Pa, finite, positive and strictly
    decreasing; ValueError otherwise, before any device use"""
    P = as_f64(np.asarray(plev, dtype=np.float64).reshape(-1), name="plev")
    if not 1 <= P.size <= _lib.PLEV_MAX:
        raise ValueError("%d pressure targets: 1 .. %d" % (P.size, _lib.PLEV_MAX))
    if not (np.all(np.isfinite(P)) and np.all(P > 0.0) and np.all(np.diff(P) < 0.0)):
        raise ValueError("pressure targets must be finite, positive and strictly decreasing (Pa)")
    return P


class PlevClimate(collections.namedtuple("PlevClimate", ("n", "plev", "coverage") + PLEV_WORDS)):
    """the zonal-mean climatology of a GCM_PE25D handle on pressure levels (Core.plev_climate): n, the number of
    samples; plev (N,), the targets in Pa; coverage (N, H) = count / (W n), the fraction of columns and samples in
    which the target was valid; and the twelve conditional means over the valid columns, each (N, H) and NaN where the
    count is 0 -- the device's float64 sums divided by the count: u = uc, v = vc (the winds at the cell centre), theta,
    T = theta Pi, q, uu, vv, TT, uv, vT, vtheta, vq, products of the interpolated values.  A band: its own rows
    (bands.merge_plev_climate)"""
    __slots__ = ()

    @property
    def eddy_momentum_flux(self):
        """[u'v'] = uv - [u][v]: all three are means over the same valid cell centres"""
        return self.uv - self.u * self.v

    @property
    def eddy_heat_flux(self):
        """[v'T'] = vT - [v][T]"""
        return self.vT - self.v * self.T

    @property
    def eddy_theta_flux(self):
        """[v'theta'] = vtheta - [v][theta]"""
        return self.vtheta - self.v * self.theta

    @property
    def eddy_moisture_flux(self):
        """[v'q'] = vq - [v][q]: the eddies' share of the meridional moisture transport vq"""
        return self.vq - self.v * self.q

    @property
    def T_variance(self):
        """[T'T'] = TT - [T]^2: the eddy temperature variance"""
        return self.TT - self.T * self.T

    @property
    def eke(self):
        """0.5 (uu - [u]^2 + vv - [v]^2): the eddy kinetic energy per unit mass of the centred winds"""
        return 0.5 * (self.uu - self.u * self.u + self.vv - self.v * self.v)

    @classmethod
    def from_sums(cls, n, plev, s, width):
        """the record of the raw sums s (13, N, H) of n samples of rows of `width` columns at the targets plev"""
        s = np.asarray(s, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            count = np.where(s[0] > 0.0, s[0], np.nan)
            cover = s[0] / (np.float64(width) * np.float64(n))
            return cls(int(n), np.array(plev, dtype=np.float64), cover, *[s[w + 1] / count for w in range(len(PLEV_WORDS))])


def plev_columns(pl, x, plev):
    """the sigma -> p column rule on the host (gcm_plev_columns; the host build of the routines the kernels call, no
    handle, no device) over columns pl, x of shape (..., L), level 0 the bottom, at the targets plev (N,)
    -> (out (..., N), valid (..., N) bool); out holds NaN where a target is invalid.  ValueError for a refused argument"""
    pl = np.asarray(pl, dtype=np.float64)
    L = pl.shape[-1] if pl.ndim else 0
    pp = as_f64(pl.reshape(-1, L) if L else pl, name="pl")
    xx = as_f64(x, pl.shape, "x").reshape(pp.shape)
    P = plev_array(plev)
    out = np.full((pp.shape[0], P.size), np.nan)
    valid = np.zeros((pp.shape[0], P.size), dtype=np.intc)
    _check(lib.gcm_plev_columns(pp.shape[0], L, P.size, _tab(pp), _tab(xx), _tab(P), _tab(out), valid.ctypes.data_as(C.POINTER(C.c_int))))
    return out.reshape(pl.shape[:-1] + (P.size,)), valid.reshape(pl.shape[:-1] + (P.size,)).astype(bool)


# the conditional means of gcm_get_plev_maps' words 1 .. 12 (word 0 is the count), then the means of its s2
PLEV_MAP_WORDS = ("Z", "ZZ", "T", "TT", "u", "v", "uu", "vv", "uv", "vT", "q", "vq")
PLEV_MAP_WORDS2 = ("p", "pp")


class PlevMaps(collections.namedtuple("PlevMaps", ("n", "plev", "coverage") + PLEV_MAP_WORDS + PLEV_MAP_WORDS2)):
    """the time-mean maps of a GCM_PE25D handle on pressure levels (Core.plev_maps): n, the number of samples; plev
    (N,), the targets in Pa; coverage (N, H, W) = count / n, the fraction of samples in which the target was valid in
    the column; the twelve conditional means over the valid samples, each (N, H, W) and NaN where the count is 0 -- the
    device's float64 sums divided by the count: Z (the geopotential height in m), ZZ, T = theta Pi, TT, u = uc, v = vc
    (the winds at the cell centre), uu, vv, uv, vT, q, vq, products of the interpolated values; and p, pp (H, W), the
    means of the handle's p field and of its square over all n samples.  A band: its own rows (bands.merge_plev_maps).
    The variances and eddy fluxes below are differences of large numbers -- ZZ - Z^2 at 500 hPa is a few 1e3 m^2 out of
    3e7 m^2 --: float64 sums leave them about nine digits, and a cell in which the field hardly varied may come out
    slightly negative."""
    __slots__ = ()

    @property
    def Z_variance(self):
        """<Z'Z'> = ZZ - <Z>^2: the variance of the height in time, the storm track where it is large"""
        return self.ZZ - self.Z * self.Z

    @property
    def T_variance(self):
        """<T'T'> = TT - <T>^2"""
        return self.TT - self.T * self.T

    @property
    def eke(self):
        """0.5 (uu - <u>^2 + vv - <v>^2): the transient eddy kinetic energy per unit mass of the centred winds"""
        return 0.5 * (self.uu - self.u * self.u + self.vv - self.v * self.v)

    @property
    def eddy_heat_flux(self):
        """<v'T'> = vT - <v><T>: the transient eddies' meridional heat flux"""
        return self.vT - self.v * self.T

    @property
    def eddy_moisture_flux(self):
        """<v'q'> = vq - <v><q>"""
        return self.vq - self.v * self.q

    @property
    def p_variance(self):
        """<p'p'> = pp - <p>^2 of the handle's p field (surface pressure minus ptop)"""
        return self.pp - self.p * self.p

    def zonal_mean(self, word):
        """the mean along longitude of the field named `word` (one of the record's fields, or a derived one such as
        "Z_variance") over the cells that hold a value: (N, H), or (H,) for p and pp; NaN where a row holds none"""
        x = np.asarray(getattr(self, word), dtype=np.float64)
        ok = np.isfinite(x)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(ok, x, 0.0).sum(axis=-1) / ok.sum(axis=-1)

    def stationary(self, word):
        """the field named `word` minus its zonal mean: the stationary waves of a time mean (Z over topography)"""
        return np.asarray(getattr(self, word), dtype=np.float64) - self.zonal_mean(word)[..., None]

    @classmethod
    def from_sums(cls, n, plev, s, s2):
        """the record of the raw sums s (13, N, H, W), s2 (2, H, W) of n samples at the targets plev"""
        s, s2 = np.asarray(s, dtype=np.float64), np.asarray(s2, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            count = np.where(s[0] > 0.0, s[0], np.nan)
            cover = s[0] / np.float64(n)
            return cls(int(n), np.array(plev, dtype=np.float64), cover, *[s[w + 1] / count for w in range(len(PLEV_MAP_WORDS))],
                       *[s2[w] / np.float64(n) for w in range(len(PLEV_MAP_WORDS2))])


def plev_height_columns(p, theta, plev, sig, dsig, sigt, ptop=0.0, hmG=None):
    """the geopotential height of columns on the pressures plev (N,) on the host (gcm_plev_height_columns; the host
    build of the march the kernel runs, no handle, no device): p (...), theta (..., L) with level 0 the bottom, sig, dsig,
    sigt (L,), hmG (...) the heightmap times G per column (None: 0) -> (Z (..., N) in m, valid (..., N) bool); Z holds NaN
    where a target is invalid.  ValueError for a refused argument"""
    theta = np.asarray(theta, dtype=np.float64)
    L = theta.shape[-1] if theta.ndim else 0
    tt = as_f64(theta.reshape(-1, L) if L else theta, name="theta")
    pp = as_f64(p, theta.shape[:-1], "p").reshape(-1)
    hh = None if hmG is None else as_f64(hmG, theta.shape[:-1], "hmG").reshape(-1)
    lev = [as_f64(np.asarray(x, dtype=np.float64).reshape(-1), (L,), name) for x, name in ((sig, "sig"), (dsig, "dsig"), (sigt, "sigt"))]
    P = plev_array(plev)
    out = np.full((pp.size, P.size), np.nan)
    valid = np.zeros((pp.size, P.size), dtype=np.intc)
    _check(lib.gcm_plev_height_columns(pp.size, L, P.size, _tab(pp), _tab(tt), _tab(hh), _tab(lev[0]), _tab(lev[1]), _tab(lev[2]),
                                       float(ptop), _tab(P), _tab(out), valid.ctypes.data_as(C.POINTER(C.c_int))))
    return out.reshape(theta.shape[:-1] + (P.size,)), valid.reshape(theta.shape[:-1] + (P.size,)).astype(bool)


SPECTRA_WORDS = ("uu", "vv", "TT", "uv", "vT", "vtheta")    # the products of gcm_get_spectra's s


def spectra_weights(M, width):
    """the one-sided weights w_m of the wavenumbers m = 0 .. M - 1 of rows of `width` columns: 1 for m = 0 and for the
    Nyquist wavenumber m = width / 2 of an even width, 2 otherwise (the wavenumbers m and width - m together)"""
    w = np.full(M, 2.0)
    w[0] = 1.0
    if width % 2 == 0 and width // 2 < M:
        w[width // 2] = 1.0
    return w


class Spectra(collections.namedtuple("Spectra", ("n",) + SPECTRA_WORDS)):
    """the zonal wavenumber spectra of a GCM_PE25D handle (Core.spectra): n, the number of samples, and per product an
    (L, H, M) array, the one-sided spectrum by zonal wavenumber m = 0 .. M - 1 averaged over the samples -- the
    device's float64 sums times w_m / (W^2 n) (NaN where n = 0), w_m as in spectra_weights.  uu = |Uc|^2, vv = |Vc|^2,
    TT = |That|^2, uv = Re(Uc conj Vc), vT = Re(Vc conj That), vtheta = Re(Vc conj Thetahat) of the winds at the cell
    centre, T = theta Pi and theta.  With M = W / 2 + 1 a row's entries sum to the zonal mean of the product: uv, vT,
    vtheta and TT then sum to the climatology's.  A band: its own rows (bands.merge_spectra)"""
    __slots__ = ()

    @property
    def kinetic_energy(self):
        """0.5 (uu + vv): the kinetic-energy spectrum per unit mass of the centred winds (m = 0: the zonal mean flow)"""
        return 0.5 * (self.uu + self.vv)

    @classmethod
    def from_sums(cls, n, s, width):
        """the record of the raw sums s (6, L, H, M) of n samples of rows of `width` columns"""
        s = np.asarray(s, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            scale = spectra_weights(s.shape[-1], width) / (np.float64(width) * np.float64(width) * np.float64(n))
            return cls(int(n), *[s[w] * scale for w in range(len(SPECTRA_WORDS))])


DTYPES = {"f64": _lib.F64, "f32": _lib.F32}
# the transport scheme of a GCM_PE25D handle's passive tracers (gcm_set_tracer_scheme)
TRACER_SCHEMES = {"centred": _lib.TRACER_NONE, "upwind": _lib.TRACER_UPWIND, "van_leer": _lib.TRACER_VANLEER}


PHASES = {"held_suarez": _lib.PHASE_HELD_SUAREZ, "moist": _lib.PHASE_MOIST, "climate": _lib.PHASE_CLIMATE,
          "tracer_forcing": _lib.PHASE_TRACER_FORCING}


def phase_id(phase):
    """a GCM_PE25D phase as gcm_pe25d_phase_geometry takes it: a name of PHASES or a _lib.PHASE_* constant"""
    if isinstance(phase, str) and phase in PHASES:
        return PHASES[phase]
    if not isinstance(phase, (str, bool)) and phase in PHASES.values():
        return int(phase)
    raise ValueError("phase must be one of %s or a PHASE_* constant, got %r" % (sorted(PHASES), phase))


def _phase_dict(phase, out):
    if phase in (_lib.PHASE_HELD_SUAREZ, _lib.PHASE_MOIST):
        return dict(grid_x=out[0], grid_y=out[1], grid_z=out[2], levels_min=out[3], levels_max=out[4])
    if phase == _lib.PHASE_CLIMATE:
        return dict(grid_x=out[0], nseg=out[1], levels_min=out[2], levels_max=out[3], chunks=out[4])
    return dict(groups=out[0], passes=out[1])


def phase_geometry(phase, W, rows, L, cus, elem_bytes=8, accumulate=True):
    """the launch geometry of a GCM_PE25D phase over `rows` rows of W columns and L levels on a chip of `cus` compute
    units, from the helpers the launchers use themselves (gcm_pe25d_phase_geometry; no handle, no device):
    held_suarez, moist -- grid_x (256-column blocks), grid_y (rows), grid_z (level segments), levels_min / levels_max
    of a segment; climate -- grid_x (rows), nseg, levels_min / levels_max a workgroup walks, chunks (iterations of a
    level's loop over 3 x 256 columns); tracer_forcing -- groups (workgroups per forced tracer), passes"""
    out = (C.c_int * _lib.PHASE_PLAN_WORDS)()
    rc = lib.gcm_pe25d_phase_geometry(phase_id(phase), int(W), int(rows), int(L), int(cus), int(elem_bytes),
                                      int(bool(accumulate)), out, _lib.PHASE_PLAN_WORDS)
    if rc != _lib.OK:
        raise ValueError("phase_geometry: sizes must be 1 or more and elem_bytes 4 or 8")
    return _phase_dict(phase_id(phase), out)


def _stage_dict(out, band):
    n = _lib.STAGE_PLAN_WORDS if band else _lib.STAGE_BAND_WORD
    return {name: int(out[i]) for i, name in enumerate(_lib.STAGE_WORDS[:n])}


def stage_geometry(W, rows, L, cus, elem_bytes=8, plan=None):
    """the launch geometry of a whole-domain GCM_PE25D dynamics stage over `rows` rows of W columns and L levels on a
    chip of `cus` compute units at the default switches, from the helpers the launchers use themselves
    (gcm_pe25d_stage_geometry; no handle, no device).  plan: the words of gcm_filter_plan for W (None: the library's
    own plan).  K1, the looping filter kernel -- k1_loop, the instantiation k1_maxr / k1_mask (0, 1440, 2880, 4096) /
    k1_nin / k1_nw, k1_passes of the row's plan, k1_workgroups_per_row x k1_pairs_per_wg level pairs (the last
    workgroup k1_pairs_last_wg), k1_pit_rides; K4, the update kernel -- k4_rows per workgroup, k4_groups (the last of
    k4_rows_last_group rows), k4_col_tiles of 62 columns (the last of k4_cols_last_tile), k4_nseg, k4_oddtop, k4_grid"""
    out = (C.c_int * _lib.STAGE_PLAN_WORDS)()
    words, n = None, 0
    if plan is not None:
        n = len(plan)
        words = (C.c_uint * n)(*[int(x) for x in plan])
    rc = lib.gcm_pe25d_stage_geometry(int(W), int(rows), int(L), int(cus), int(elem_bytes), words, n, out,
                                      _lib.STAGE_PLAN_WORDS)
    if rc != _lib.OK:
        raise ValueError("stage_geometry: sizes must be 1 or more, elem_bytes 4 or 8, plan the words of gcm_filter_plan")
    return _stage_dict(out, False)


def tracer_scheme_id(scheme):
    """a tracer scheme as the C ABI takes it: one of the _lib.TRACER_* constants or "centred", "upwind", "van_leer"
    (None: centred); ValueError otherwise, before any device use"""
    if scheme is None:
        return _lib.TRACER_NONE
    if isinstance(scheme, str):
        if scheme in TRACER_SCHEMES:
            return TRACER_SCHEMES[scheme]
    elif not isinstance(scheme, bool):
        try:
            if int(scheme) == scheme and int(scheme) in TRACER_SCHEMES.values():
                return int(scheme)
        except (TypeError, ValueError):
            pass
    raise ValueError("tracer_scheme must be 'centred', 'upwind', 'van_leer' or a TRACER_* constant, got %r" % (scheme,))


def check_dtype(dtype):
    """the real type of a handle: "f64" (default) or "f32" (GCM_SW2D, GCM_SW2D_TEMP, GCM_PE25D); ValueError
    otherwise, before any device use"""
    if not isinstance(dtype, str) or dtype not in DTYPES:
        raise ValueError("dtype must be 'f64' or 'f32', got %r" % (dtype,))
    return dtype


# the parameters of the Held-Suarez forcing (gcm_held_suarez) with Held & Suarez (1994)'s values, in the struct's order
HELD_SUAREZ_DEFAULTS = collections.OrderedDict(
    k_f=1.0 / 86400.0, k_a=1.0 / (40.0 * 86400.0), k_s=1.0 / (4.0 * 86400.0), sigma_b=0.7, dT_y=60.0, dtheta_z=10.0,
    T_0=315.0, T_min=200.0)


def held_suarez_params(params):
    """the eight parameters of the Held-Suarez forcing as a dict of floats: Held & Suarez (1994)'s values with `params`
    laid over them; ValueError for a name that is not a parameter"""
    unknown = sorted(set(params) - set(HELD_SUAREZ_DEFAULTS))
    if unknown:
        raise ValueError("held_suarez: unknown parameter(s) %s; the parameters are %s"
                         % (", ".join(unknown), ", ".join(HELD_SUAREZ_DEFAULTS)))
    out = collections.OrderedDict(HELD_SUAREZ_DEFAULTS)
    out.update({k: float(v) for k, v in params.items()})
    return out


def _held_suarez_record(lat, params):
    """-> (gcm_held_suarez, the arrays it points to, the parameters as a dict)"""
    par = held_suarez_params(params)
    rec = _lib.HeldSuarez(*par.values())
    rec.lat = _tab(lat)
    return rec, lat, par


# the parameters of the horizontal diffusion (gcm_hdiff), in the order the checkpoint stores them.  nu: m^4/s at order 2,
# m^2/s at order 1; fields: a string of the letters u v t q, or the mask of HDIFF_FIELD_BITS
HDIFF_DEFAULTS = collections.OrderedDict(order=2, fields="uvt", nu=1.0e15, cmax=0.125)
HDIFF_FIELD_BITS = collections.OrderedDict(u=1, v=2, t=4, q=8)       # GCM_HDIFF_U, _V, _T, _Q


def hdiff_params(params):
    """the four parameters of the horizontal diffusion as a dict (order int, fields the int mask, nu, cmax floats):
    HDIFF_DEFAULTS with `params` laid over them; ValueError for a name that is not a parameter and for a `fields` that
    is neither a string of the letters u v t q nor an int"""
    unknown = sorted(set(params) - set(HDIFF_DEFAULTS))
    if unknown:
        raise ValueError("horizontal_diffusion: unknown parameter(s) %s; the parameters are %s"
                         % (", ".join(unknown), ", ".join(HDIFF_DEFAULTS)))
    out = collections.OrderedDict(HDIFF_DEFAULTS)
    out.update(params)
    fields = out["fields"]
    if isinstance(fields, str):
        bad = sorted(set(fields) - set(HDIFF_FIELD_BITS))
        if bad or not fields:
            raise ValueError("horizontal_diffusion: fields must be a non-empty string of the letters u v t q, got %r" % (fields,))
        mask = 0
        for c in fields:
            mask |= HDIFF_FIELD_BITS[c]
        fields = mask
    elif isinstance(fields, (bool, float)) or not isinstance(fields, (int, np.integer)):
        raise ValueError("horizontal_diffusion: fields must be a string of the letters u v t q or the int mask, got %r" % (fields,))
    if int(out["order"]) != out["order"]:
        raise ValueError("horizontal_diffusion: order must be 1 or 2, got %r" % (out["order"],))
    return collections.OrderedDict(order=int(out["order"]), fields=int(fields), nu=float(out["nu"]), cmax=float(out["cmax"]))


def _hdiff_record(params):
    """-> (gcm_hdiff, the parameters as a dict)"""
    par = hdiff_params(params)
    return _lib.Hdiff(par["order"], par["fields"], par["nu"], par["cmax"]), par


HDIFF_TABLES = ("ax", "bn", "bs", "area", "axv", "bnv", "bsv", "areav")      # the rows of gcm_hdiff_tables' out


def hdiff_tables(geom, dt, **params):
    """the host tables of the horizontal diffusion (gcm_hdiff_tables; no handle, no device) for the geometry's dx_j,
    dx_h (H,) and dy and the step dt -> dict of the (H,) arrays ax, bn, bs, area (centre rows: theta, q, u) and axv,
    bnv, bsv, areav (v rows): the routine the launches of Core.set_horizontal_diffusion / Core.horizontal_diffusion_step
    take their tables from.  ValueError for a refused parameter"""
    dx_j = as_f64(np.asarray(geom.dx_j, dtype=np.float64).reshape(-1), name="dx_j")
    dx_h = as_f64(np.asarray(geom.dx_h, dtype=np.float64).reshape(-1), (dx_j.size,), "dx_h")
    rec, _ = _hdiff_record(params)
    out = np.empty((len(HDIFF_TABLES), dx_j.size))
    _check(lib.gcm_hdiff_tables(dx_j.size, _tab(dx_j), _tab(dx_h), float(geom.dy), C.byref(rec), float(dt), _tab(out)))
    return dict(zip(HDIFF_TABLES, out))


def hdiff_apply(X, ax, bn, bs, order):
    """one application of the horizontal diffusion to X (nlev, H, W) or (H, W) on the host in float64, periodic both
    ways, with the rows' coefficients ax, bn, bs (H,) (gcm_hdiff_apply: the host build of the cell routine the kernel
    calls; no handle, no device) -> the array of X's shape.  order 1: X + D(X); order 2: X - D(D(X)).  ValueError for
    a refused argument"""
    X = as_f64(X, name="X")
    if X.ndim not in (2, 3):
        raise ValueError("X has shape %s, expected (nlev, H, W) or (H, W)" % (X.shape,))
    H, W = X.shape[-2:]
    nlev = X.shape[0] if X.ndim == 3 else 1
    tab = np.zeros((4, H))
    for n, (a, name) in enumerate(zip((ax, bn, bs), ("ax", "bn", "bs"))):
        tab[n] = as_f64(np.asarray(a, dtype=np.float64).reshape(-1), (H,), name)
    out = np.empty_like(X)
    _check(lib.gcm_hdiff_apply(H, W, nlev, _tab(tab), int(order), _tab(X), _tab(out)))
    return out


def hdiff_apply_band(X, ax, bn, bs, order):
    """one application of the horizontal diffusion to the own rows of a latitude band on the host in float64
    (gcm_hdiff_apply_band: the host build of the band walk, periodic in i only; no handle, no device).  X is
    (nlev, Hb + 4, W) or (Hb + 4, W): the band's Hb own rows with two ghost rows a side, rows -2 .. Hb + 1; ax, bn, bs
    (Hb + 4,) are the coefficients of those rows, taken from the tables over the global height at row (row0 + j) mod
    global_height -> the own rows, (nlev, Hb, W) or (Hb, W).  They are rows [row0, row0 + Hb) of hdiff_apply over the
    periodic whole, bit for bit.  ValueError for a refused argument"""
    X = as_f64(X, name="X")
    if X.ndim not in (2, 3):
        raise ValueError("X has shape %s, expected (nlev, Hb + 4, W) or (Hb + 4, W)" % (X.shape,))
    HT, W = X.shape[-2:]
    if HT < 5:
        raise ValueError("X has %d rows: a band is 1 own row or more and two ghost rows a side" % HT)
    nlev = X.shape[0] if X.ndim == 3 else 1
    tab = np.zeros((4, HT))
    for n, (a, name) in enumerate(zip((ax, bn, bs), ("ax", "bn", "bs"))):
        tab[n] = as_f64(np.asarray(a, dtype=np.float64).reshape(-1), (HT,), name)
    out = np.empty(X.shape[:-2] + (HT - 4, W))
    _check(lib.gcm_hdiff_apply_band(HT - 4, W, nlev, _tab(tab), int(order), _tab(X), _tab(out)))
    return out


def held_suarez_tables(sig, lat, dt, **params):
    """the host tables of the Held-Suarez forcing (gcm_held_suarez_tables; no handle, no device) for the mid-level
    sigmas `sig` (L,), the latitudes `lat` (n,) in radians and the step dt -> dict(fu (L,), kt (L, n), s2 (n,), c2 (n,)):
    the routine the launches of Core.set_held_suarez / Core.held_suarez_step take their tables from.  ValueError for a
    refused parameter"""
    sig = as_f64(np.asarray(sig, dtype=np.float64).reshape(-1), name="sig")
    lat = as_f64(np.asarray(lat, dtype=np.float64).reshape(-1), name="lat")
    rec, _, _ = _held_suarez_record(lat, params)
    L, n = sig.size, lat.size
    fu, kt, s2, c2 = np.empty(L), np.empty((L, n)), np.empty(n), np.empty(n)
    _check(lib.gcm_held_suarez_tables(L, _tab(sig), n, _tab(lat), C.byref(rec), float(dt), _tab(fu), _tab(kt), _tab(s2),
                                      _tab(c2)))
    return dict(fu=fu, kt=kt, s2=s2, c2=c2)


def grey_params(t_lw=0.1, t_sw=0.9, albedo=0.3, **clock):
    """the three parameters of the grey radiation as floats, and the clock values `clock` (utc, dt) checked with them:
    t_lw and t_sw in (0, 1], albedo in [0, 1], the clock finite -- what gcm_grey_radiation, gcm_solar_step and
    gcm_set_physics accept, said without a handle.  ValueError otherwise (NaN included).  What depends on the levels
    (a transmissivity so small that a level's share rounds to 0) is left to the library"""
    t_lw, t_sw, albedo = float(t_lw), float(t_sw), float(albedo)
    for name, x in (("t_lw", t_lw), ("t_sw", t_sw)):
        if not (0.0 < x <= 1.0):
            raise ValueError("grey radiation: %s must lie in (0, 1], got %r" % (name, x))
    if not (0.0 <= albedo <= 1.0):
        raise ValueError("grey radiation: albedo must lie in [0, 1], got %r" % albedo)
    for name, x in clock.items():
        if not np.isfinite(float(x)):
            raise ValueError("grey radiation: %s must be finite, got %r" % (name, x))
    return t_lw, t_sw, albedo


def grey_radiation_tables(dsig, sig, t_lw=0.1, t_sw=0.9):
    """the level tables of the radiation kernel (gcm_grey_radiation_tables; no handle, no device) for the levels dsig, sig
    (L,) -> dict(tlw, tsw, csw_top, clw_b_div, swfac, sigk), each (L,): the routine the launches of Core.grey_radiation,
    Core.solar_step and Core.set_physics take their tables from.  ValueError for a refused parameter"""
    dsig = as_f64(np.asarray(dsig, dtype=np.float64).reshape(-1), name="dsig")
    sig = as_f64(np.asarray(sig, dtype=np.float64).reshape(-1), (dsig.size,), "sig")
    out = np.empty((6, dsig.size))
    _check(lib.gcm_grey_radiation_tables(dsig.size, _tab(dsig), _tab(sig), float(t_lw), float(t_sw), _tab(out), out.size))
    return dict(zip(("tlw", "tsw", "csw_top", "clw_b_div", "swfac", "sigk"), out))


# the parameters of the moist physics (gcm_moist), in the struct's order: the latent heat (J / kg), the evaporation time
# scale (s; 0: no evaporation) and the target relative humidity of the lowest level
MOIST_DEFAULTS = collections.OrderedDict(Lv=2.5e6, tau_e=0.0, rh_s=0.8)


def moist_params(params):
    """the three parameters of the moist physics as a dict of floats: MOIST_DEFAULTS with `params` laid over them;
    ValueError for a name that is not a parameter"""
    unknown = sorted(set(params) - set(MOIST_DEFAULTS))
    if unknown:
        raise ValueError("moist: unknown parameter(s) %s; the parameters are %s"
                         % (", ".join(unknown), ", ".join(MOIST_DEFAULTS)))
    out = collections.OrderedDict(MOIST_DEFAULTS)
    out.update({k: float(v) for k, v in params.items()})
    return out


class Moist(collections.namedtuple("Moist", "nsteps seconds precip evap")):
    """the sums of a GCM_PE25D handle's moist physics (Core.moist_sums): the applications counted, the sum of their dt
    in seconds, and per column (H, W) the precipitation and the evaporation accumulated over them, kg / m^2, float64.
    A band: its own rows (bands.merge_moist)"""
    __slots__ = ()

    def _rate(self, a):
        if self.seconds == 0:
            raise ValueError("Moist: no time accumulated (seconds == 0)")
        return a / self.seconds

    def precip_rate(self):
        """kg / m^2 / s: precip / seconds; ValueError where seconds == 0"""
        return self._rate(self.precip)

    def evap_rate(self):
        """kg / m^2 / s: evap / seconds; ValueError where seconds == 0"""
        return self._rate(self.evap)


def moist_saturation(T, p_lev):
    """the saturation routine of the moist physics (gcm_moist_saturation; the host build of the one routine the kernel
    calls, no handle, no device) for true temperatures T (K) and level pressures p_lev (Pa) of one shape
    -> (q_s, dq_s, can): the saturation specific humidity, its derivative in T at constant pressure, and whether the cell
    can saturate (e_s < p_lev; where it cannot, q_s and dq_s are 0)"""
    T = np.asarray(T, dtype=np.float64)
    p_lev = np.asarray(p_lev, dtype=np.float64)
    if T.shape != p_lev.shape:
        raise ValueError("moist_saturation: T has shape %s, p_lev %s" % (T.shape, p_lev.shape))
    t, pl = as_f64(T.reshape(-1)), as_f64(p_lev.reshape(-1))
    qs, dqs, can = np.empty(t.size), np.empty(t.size), np.empty(t.size, dtype=np.intc)
    _check(lib.gcm_moist_saturation(t.size, _tab(t), _tab(pl), _tab(qs), _tab(dqs), can.ctypes.data_as(C.POINTER(C.c_int))))
    return qs.reshape(T.shape), dqs.reshape(T.shape), can.reshape(T.shape).astype(bool)


# the parameters of the surface fluxes and the boundary-layer mixing (gcm_boundary_layer), in the struct's order: the drag
# cd = cd0 + cd1 min(S, v_cap), the exchange coefficients of heat and moisture, the pressure at and below which the mixing
# is full (Pa) and the e-folding scale of its decay above (Pa): Reed & Jablonowski (2012)'s values
BOUNDARY_LAYER_DEFAULTS = collections.OrderedDict(cd0=7.0e-4, cd1=6.5e-5, v_cap=20.0, ch=0.0044, ce=0.0044, p_pbl=85000.0,
                                                  p_strat=10000.0)


def boundary_layer_params(params):
    """the seven parameters of the boundary layer as a dict of floats: BOUNDARY_LAYER_DEFAULTS with `params` laid over
    them; ValueError for a name that is not a parameter"""
    unknown = sorted(set(params) - set(BOUNDARY_LAYER_DEFAULTS))
    if unknown:
        raise ValueError("boundary_layer: unknown parameter(s) %s; the parameters are %s"
                         % (", ".join(unknown), ", ".join(BOUNDARY_LAYER_DEFAULTS)))
    out = collections.OrderedDict(BOUNDARY_LAYER_DEFAULTS)
    out.update({k: float(v) for k, v in params.items()})
    return out


class BoundaryLayer(collections.namedtuple("BoundaryLayer", "nsteps seconds shf evap")):
    """the sums of a GCM_PE25D handle's boundary layer (Core.boundary_layer_sums): the applications counted, the sum of
    their dt in seconds, and per column (H, W), float64, the sensible heat the surface gave the air, J / m^2, and the
    water, kg / m^2 (negative: dew)"""
    __slots__ = ()


def boundary_layer_surface(uc, vc, theta0, q0, p, sig0, ptop=0.0, **params):
    """the level-0 centre quantities of the boundary layer (gcm_boundary_layer_surface; the host build of the routine the
    kernel calls, no handle, no device) for centre winds uc, vc (m / s), theta and q of the lowest level and p (Pa, surface
    pressure minus ptop) of one shape, sig0 the lowest level's sigma -> (S, z_a, cd): the wind speed, the height of the
    lowest level (m) and the drag coefficient.  ValueError for a refused parameter"""
    uc = np.asarray(uc, dtype=np.float64)
    arrs = [as_f64(np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), uc.shape)).reshape(-1), name=n)
            for a, n in ((uc, "uc"), (vc, "vc"), (theta0, "theta0"), (q0, "q0"), (p, "p"))]
    rec = _lib.BoundaryLayer(*boundary_layer_params(params).values())
    out = [np.empty(uc.size) for _ in range(3)]
    _check(lib.gcm_boundary_layer_surface(uc.size, C.byref(rec), float(ptop), float(sig0), *[_tab(a) for a in arrs + out]))
    return tuple(a.reshape(uc.shape) for a in out)


def boundary_layer_column(dsig, a, x, target, X):
    """one column solve of the boundary layer, "surface step on level 0, then diffusion" (gcm_boundary_layer_column; the
    host build of the routines the kernels call, no handle, no device) over columns X (..., L), level 0 the bottom, with
    dsig (L,), the interface coefficients a (..., L - 1) and per column the surface weight x and the target (...)
    -> (X_out (..., L), X0_surface (...))"""
    X = np.asarray(X, dtype=np.float64)
    L = X.shape[-1] if X.ndim else 0
    XX = as_f64(X.reshape(-1, L) if L else X, name="X")
    n = XX.shape[0] if L else 0
    aa = as_f64(np.asarray(a, dtype=np.float64).reshape(n, max(L - 1, 0)), name="a")
    xx, tt = (as_f64(np.asarray(v, dtype=np.float64).reshape(n), name=nm) for v, nm in ((x, "x"), (target, "target")))
    dd = as_f64(dsig, (L,), "dsig")
    out, x0 = np.empty_like(XX), np.empty(n)
    _check(lib.gcm_boundary_layer_column(n, L, _tab(dd), _tab(aa), _tab(xx), _tab(tt), _tab(XX), _tab(out), _tab(x0)))
    return out.reshape(X.shape), x0.reshape(X.shape[:-1])


# the parameters of the slab mixed-layer ocean (gcm_slab_ocean), in the struct's order: the heat capacity of the slab,
# J m^-2 K^-1 (1.0e7: Frierson's 2.4 m of water; inf: a prescribed temperature), and the latent heat, J / kg
SLAB_OCEAN_DEFAULTS = collections.OrderedDict(heat_capacity=1.0e7, Lv=2.5e6)
# the flux words of a cell (GCM_SLAB_*) and the sums (the order of gcm_get_slab_ocean)
SLAB_OCEAN_WORDS = ("SC", "SW_SFC", "LW_DOWN", "LW_UP", "OLR", "SH_J", "EVAP_KG")
SLAB_OCEAN_SUMS = ("dt_SC", "dt_S", "dt_B", "dt_Us", "dt_OLR", "SH_J", "Lv_EVAP_KG", "dt_Q", "dt_gt", "dt_gt2")


def slab_ocean_params(params):
    """the two parameters of the slab ocean as a dict of floats: SLAB_OCEAN_DEFAULTS with `params` laid over them;
    ValueError for a name that is not a parameter"""
    unknown = sorted(set(params) - set(SLAB_OCEAN_DEFAULTS))
    if unknown:
        raise ValueError("slab_ocean: unknown parameter(s) %s; the parameters are %s"
                         % (", ".join(unknown), ", ".join(SLAB_OCEAN_DEFAULTS)))
    out = collections.OrderedDict(SLAB_OCEAN_DEFAULTS)
    out.update({k: float(v) for k, v in params.items()})
    return out


class SlabOcean(collections.namedtuple("SlabOcean", "nsteps seconds sums reflect")):
    """the sums of a GCM_PE25D handle's slab ocean (Core.slab_ocean_sums): the applications counted, the sum of their dt
    in seconds, the raw float64 sums (10, H, W) in the order of SLAB_OCEAN_SUMS, and `reflect` = albedo csw_top[0] of the
    registered physics, the share of the insolation the surface sends back to space (0 without physics).  The properties
    are time means over `seconds`, W / m^2 and positive in the direction their name says; ValueError where seconds == 0.
    A band: its own rows (bands.merge_slab_ocean)"""
    __slots__ = ()

    def _mean(self, n):
        if self.seconds == 0:
            raise ValueError("SlabOcean: no time accumulated (seconds == 0)")
        return self.sums[n] / self.seconds

    insolation = property(lambda self: self._mean(0), doc="the sun at the top of the atmosphere, SC")
    sw_surface = property(lambda self: self._mean(1), doc="short wave absorbed by the surface, S")
    lw_down = property(lambda self: self._mean(2), doc="long wave reaching the surface, B")
    lw_up = property(lambda self: self._mean(3), doc="long wave leaving the surface, U_s")
    olr = property(lambda self: self._mean(4), doc="outgoing long wave at the top")
    shf = property(lambda self: self._mean(5), doc="sensible heat the surface gave the air")
    lhf = property(lambda self: self._mean(6), doc="latent heat the surface gave the air, Lv times the evaporation")
    qflux = property(lambda self: self._mean(7), doc="the prescribed ocean heat flux into the slab")

    @property
    def asr(self):
        """short wave absorbed by the column: SC - albedo SC csw_top[0]"""
        return self.insolation - self.reflect * self.insolation

    @property
    def surface_net(self):
        """what the slab gains: ((S + B) - U_s) - shf - lhf + qflux"""
        return ((self.sw_surface + self.lw_down) - self.lw_up) - self.shf - self.lhf + self.qflux

    @property
    def toa_net(self):
        """what the column gains at the top: asr - olr"""
        return self.asr - self.olr

    @property
    def sst_mean(self):
        """the time mean of the slab's temperature, K"""
        return self._mean(8)

    @property
    def sst_variance(self):
        """the time variance of the slab's temperature, K^2: mean(gt^2) - mean(gt)^2"""
        m = self._mean(8)
        return self._mean(9) - m * m


def slab_ocean_cells(gt, words, dt, capacity=None, qflux=None, **params):
    """the cell rule of the slab ocean (gcm_slab_ocean_cells; the host build of the routine the kernel calls, no handle,
    no device) for cells gt of any shape with the flux words `words` (7, ...) in the order of SLAB_OCEAN_WORDS, the step
    dt, and per cell the heat capacity (None: the scalar heat_capacity) and the ocean heat flux (None: 0)
    -> (gt_out, E4): the new temperature and the energy the step gave the cell, J / m^2.  ValueError for a refused
    parameter"""
    gt = np.asarray(gt, dtype=np.float64)
    g = as_f64(gt.reshape(-1), name="gt")
    w = as_f64(np.asarray(words, dtype=np.float64).reshape(_lib.SLAB_WORDS, -1), (_lib.SLAB_WORDS, g.size), "words")
    opt = [None if a is None else as_f64(np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), gt.shape)).reshape(-1), name=n)
           for a, n in ((capacity, "capacity"), (qflux, "qflux"))]
    rec = _lib.SlabOcean(*slab_ocean_params(params).values())
    out, e4 = np.empty(g.size), np.empty(g.size)
    _check(lib.gcm_slab_ocean_cells(g.size, C.byref(rec), float(dt), _tab(g), None if opt[0] is None else _tab(opt[0]), _tab(w),
                                    None if opt[1] is None else _tab(opt[1]), _tab(out), _tab(e4)))
    return out.reshape(gt.shape), e4.reshape(gt.shape)


# the parameters of the grey radiation by water vapour and CO2 (gcm_gas_radiation_par), in the struct's order: the long-
# and short-wave weights of water vapour and CO2, m^2 / kg, the CO2 volume mixing ratio, the ground's albedo, the solar
# constant, W / m^2, the declination, radians, and the insolation ("uniform" | "zenith" | "daily").  The values are the
# reference's (grey_solar.py:29,76-80,208,290), as its unit bookkeeping evaluates them
GAS_RADIATION_DEFAULTS = collections.OrderedDict(k_h2o_lw=0.125, k_co2_lw=1.0, k_h2o_sw=0.125, k_co2_sw=1.0, co2_vmr=300 / 1e6,
                                                 ground_albedo=0.1, solar_constant=2 * 41840 * 60.0 ** -1, declination=0.0,
                                                 insolation="uniform")


def gas_radiation_params(params, **clock):
    """the parameters of the gas radiation as a dict: GAS_RADIATION_DEFAULTS with `params` laid over them, floats but for
    the insolation's name, and the clock values `clock` (utc, dt) checked with them -- what the library accepts, said
    without a handle.  ValueError for a name that is not a parameter and for a refused value (NaN included)"""
    unknown = sorted(set(params) - set(GAS_RADIATION_DEFAULTS))
    if unknown:
        raise ValueError("gas_radiation: unknown parameter(s) %s; the parameters are %s"
                         % (", ".join(unknown), ", ".join(GAS_RADIATION_DEFAULTS)))
    out = collections.OrderedDict(GAS_RADIATION_DEFAULTS)
    out.update({k: (v if k == "insolation" else float(v)) for k, v in params.items()})
    for k in ("k_h2o_lw", "k_co2_lw", "k_h2o_sw", "k_co2_sw", "co2_vmr", "solar_constant"):
        if not (np.isfinite(out[k]) and out[k] >= 0.0):
            raise ValueError("gas_radiation: %s must be finite and >= 0, got %r" % (k, out[k]))
    if not (0.0 <= out["ground_albedo"] < 1.0):
        raise ValueError("gas_radiation: ground_albedo must lie in [0, 1), got %r" % out["ground_albedo"])
    if not (abs(out["declination"]) <= np.pi / 2):
        raise ValueError("gas_radiation: declination must lie in [-pi/2, pi/2], got %r" % out["declination"])
    if out["insolation"] not in _lib.INSOLATION:
        raise ValueError("gas_radiation: unknown insolation %r; one of %s" % (out["insolation"], ", ".join(_lib.INSOLATION)))
    for name, x in clock.items():
        if not np.isfinite(float(x)):
            raise ValueError("gas_radiation: %s must be finite, got %r" % (name, x))
    return out


def _gas_record(par):
    return _lib.GasRadiation(*[_lib.INSOLATION[v] if k == "insolation" else v for k, v in par.items()])


def gas_insolation(lat, insolation="uniform", declination=0.0, solar_constant=GAS_RADIATION_DEFAULTS["solar_constant"]):
    """the insolation of the rows at the latitudes `lat` (radians), W / m^2 (gcm_gas_insolation; no handle, no device):
    "uniform", the reference's solar_constant 0.5 0.5, or "daily", its daily_average_irradiance(lat, declination) with the
    arccos argument kept inside [-1, 1] (finite in polar night and polar day).  ValueError for "zenith", which has no row
    table, and for a refused parameter"""
    par = gas_radiation_params(dict(insolation=insolation, declination=declination, solar_constant=solar_constant))
    lat = np.asarray(lat, dtype=np.float64)
    la = as_f64(lat.reshape(-1), name="lat")
    out = np.empty(la.size)
    _check(lib.gcm_gas_insolation(_lib.INSOLATION[par["insolation"]], la.size, _tab(la), par["declination"], par["solar_constant"], _tab(out)))
    return out.reshape(lat.shape)


def gas_radiation_columns(SC, p, tt, q, gt, sig, dsig, ptop=0.0, words=False, **params):
    """the column routine of the gas radiation (gcm_gas_radiation_columns; the host build of the routine the kernel calls,
    no handle, no device): the insolation SC, the surface pressure p and the ground temperature gt of any one shape S, the
    true temperature tt and q of shape (L,) + S, the levels sig and dsig (L,) -> (dt_ground S, dt_air (L,) + S, olr S),
    and with words=True a fourth, (5,) + S: SC, SW_SFC, LW_DOWN, LW_UP, OLR.  ValueError for a refused parameter"""
    par = gas_radiation_params(params)
    p = np.asarray(p, dtype=np.float64)
    pf = as_f64(p.reshape(-1), name="p")
    n = pf.size
    flat = [as_f64(np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), p.shape)).reshape(-1), (n,), nm)
            for a, nm in ((SC, "SC"), (gt, "gt"))]
    sig = as_f64(np.asarray(sig, dtype=np.float64).reshape(-1), name="sig")
    L = sig.size
    dsig = as_f64(np.asarray(dsig, dtype=np.float64).reshape(-1), (L,), "dsig")
    lev = [as_f64(np.asarray(a, dtype=np.float64).reshape(L, -1), (L, n), nm) for a, nm in ((tt, "tt"), (q, "q"))]
    dg, da, olr, w = np.empty(n), np.empty((L, n)), np.empty(n), np.empty((5, n))
    rec = _gas_record(par)
    _check(lib.gcm_gas_radiation_columns(n, L, C.byref(rec), _tab(flat[0]), _tab(pf), float(ptop), _tab(sig), _tab(dsig),
                                         _tab(lev[0]), _tab(lev[1]), _tab(flat[1]), _tab(dg), _tab(da), _tab(olr), _tab(w)))
    out = (dg.reshape(p.shape), da.reshape((L,) + p.shape), olr.reshape(p.shape))
    return out + (w.reshape((5,) + p.shape),) if words else out


def aquaplanet_sst(lat, dT=29.0, T_min=271.0, width=np.deg2rad(26.0)):
    """the prescribed sea-surface temperature of the moist Held-Suarez test (Thatcher & Jablonowski 2016) at the
    latitudes `lat` (radians), K: dT exp(-lat^2 / (2 width^2)) + T_min, width in radians (26 degrees).  What set_ground
    takes on an aquaplanet, broadcast over the longitudes"""
    lat = np.asarray(lat, dtype=np.float64)
    return dT * np.exp(-(lat * lat) / (2.0 * width * width)) + T_min


# the parameters of the convective adjustment (gcm_convect), in the struct's order: kappa_c = Rd gamma / g of the neutral
# profile (0: dry adjustment, neutral where theta is constant) and whether q of a merged block is mixed
CONVECT_DEFAULTS = collections.OrderedDict(kappa_c=0.0, mix_q=1)
CONVECT_RD, CONVECT_G = 287.0, 9.8              # constants.py: what turns a lapse rate gamma (K / m) into kappa_c


def convect_params(params):
    """the two parameters of the convective adjustment as a dict (kappa_c float, mix_q 0 or 1): CONVECT_DEFAULTS with
    `params` laid over them.  params: at most one of gamma (the critical lapse rate, K / m: kappa_c = Rd gamma / g) and
    kappa_c, neither means the dry adjustment; mix_q.  ValueError for a name that is not a parameter, and for gamma
    given together with kappa_c"""
    unknown = sorted(set(params) - {"gamma", "kappa_c", "mix_q"})
    if unknown:
        raise ValueError("convect: unknown parameter(s) %s; the parameters are gamma or kappa_c, and mix_q" % ", ".join(unknown))
    gamma, kappa_c = params.get("gamma"), params.get("kappa_c")
    if gamma is not None and kappa_c is not None:
        raise ValueError("convect: give gamma or kappa_c, not both")
    out = collections.OrderedDict(CONVECT_DEFAULTS)
    if gamma is not None:
        out["kappa_c"] = CONVECT_RD * float(gamma) / CONVECT_G
    elif kappa_c is not None:
        out["kappa_c"] = float(kappa_c)
    if "mix_q" in params:
        if params["mix_q"] not in (0, 1, False, True):
            raise ValueError("convect: mix_q must be 0 or 1")
        out["mix_q"] = int(params["mix_q"])
    return out


class Convect(collections.namedtuple("Convect", "nsteps seconds count levels")):
    """the sums of a GCM_PE25D handle's convective adjustment (Core.convect_sums): the applications counted, the sum of
    the registered steps' dt in seconds, and per column (H, W), float64, in how many applications the column was adjusted
    (count) and the levels its merged blocks held, summed over them (levels).  A band: its own rows
    (bands.merge_convect)"""
    __slots__ = ()

    @property
    def frequency(self):
        """count / nsteps: the share of the applications in which a column was adjusted; ValueError where nsteps == 0"""
        if self.nsteps == 0:
            raise ValueError("Convect: no application counted (nsteps == 0)")
        return self.count / self.nsteps

    @property
    def mean_depth(self):
        """levels / max(count, 1): the mean number of levels adjusted when the column was adjusted, 0 where never"""
        return self.levels / np.maximum(self.count, 1.0)


def convect_columns(y, w, q, dsig, mix_q=True):
    """the pooling of the convective adjustment (gcm_convect_columns; the host build of the one routine the kernel
    calls, no handle, no device) over columns y, w, q of shape (..., L), level 0 the bottom, with dsig (L,)
    -> (y_out, q_out, nblock): the adjusted y and q and, per level, the size of its block (int32)"""
    y = np.asarray(y, dtype=np.float64)
    L = y.shape[-1] if y.ndim else 0
    yy = as_f64(y.reshape(-1, L) if L else y, name="y")
    ww, qq = (as_f64(a, y.shape, n).reshape(yy.shape) for a, n in ((w, "w"), (q, "q")))
    dd = as_f64(dsig, (L,), "dsig")
    yo, qo, nb = np.empty_like(yy), np.empty_like(yy), np.empty(yy.shape, dtype=np.int32)
    _check(lib.gcm_convect_columns(yy.shape[0], L, _tab(yy), _tab(ww), _tab(qq), _tab(dd), int(bool(mix_q)), _tab(yo), _tab(qo),
                                   nb.ctypes.data_as(C.POINTER(C.c_int32))))
    return yo.reshape(y.shape), qo.reshape(y.shape), nb.reshape(y.shape)


def convect_tracer_columns(y, w, dsig, c, nblock=False):
    """the convective mixing of a tracer (gcm_convect_tracer_columns; the host build of the routines the kernel calls,
    no handle, no device) over columns y, w, c of shape (..., L), level 0 the bottom, with dsig (L,): the blocks are
    those convect_columns pools from y and w, and c of every merged block becomes sum c dsig / sum dsig, both sums
    sequential from the block's lowest level -> c_out; with nblock=True -> (c_out, nblock (int32))"""
    y = np.asarray(y, dtype=np.float64)
    L = y.shape[-1] if y.ndim else 0
    yy = as_f64(y.reshape(-1, L) if L else y, name="y")
    ww, cc = (as_f64(a, y.shape, n).reshape(yy.shape) for a, n in ((w, "w"), (c, "c")))
    dd = as_f64(dsig, (L,), "dsig")
    co, nb = np.empty_like(yy), np.empty(yy.shape, dtype=np.intc)
    _check(lib.gcm_convect_tracer_columns(yy.shape[0], L, _tab(yy), _tab(ww), _tab(dd), _tab(cc), _tab(co),
                                          nb.ctypes.data_as(C.POINTER(C.c_int))))
    co = co.reshape(y.shape)
    return (co, nb.astype(np.int32).reshape(y.shape)) if nblock else co


# the parameters of the Betts-Miller convection (gcm_betts_miller), in the struct's order: the latent heat (J / kg), the
# relaxation time (s), the relative humidity of the reference profile and the midpoint steps per level of the parcel's
# pseudoadiabat
BETTS_MILLER_DEFAULTS = collections.OrderedDict(Lv=2.5e6, tau=7200.0, rh_bm=0.7, nsub=2)


def betts_miller_params(params):
    """the four parameters of the Betts-Miller convection as a dict (Lv, tau, rh_bm floats, nsub an int):
    BETTS_MILLER_DEFAULTS with `params` laid over them; ValueError for a name that is not a parameter and for an nsub
    that is no whole number"""
    unknown = sorted(set(params) - set(BETTS_MILLER_DEFAULTS))
    if unknown:
        raise ValueError("betts_miller: unknown parameter(s) %s; the parameters are %s"
                         % (", ".join(unknown), ", ".join(BETTS_MILLER_DEFAULTS)))
    out = collections.OrderedDict(BETTS_MILLER_DEFAULTS)
    for k, v in params.items():
        if k == "nsub":
            if isinstance(v, bool) or int(v) != v:
                raise ValueError("betts_miller: nsub must be a whole number")
            out[k] = int(v)
        else:
            out[k] = float(v)
    return out


class BettsMiller(collections.namedtuple("BettsMiller", "nsteps seconds precip count")):
    """the sums of a GCM_PE25D handle's Betts-Miller convection (Core.betts_miller_sums): the applications counted, the
    sum of their dt in seconds, and per column (H, W), float64, the convective precipitation accumulated over them,
    kg / m^2, and in how many applications the column convected.  A band: its own rows (bands.merge_betts_miller)"""
    __slots__ = ()

    def precip_rate(self):
        """kg / m^2 / s: precip / seconds; ValueError where seconds == 0"""
        if self.seconds == 0:
            raise ValueError("BettsMiller: no time accumulated (seconds == 0)")
        return self.precip / self.seconds

    def frequency(self):
        """count / nsteps: the share of the applications in which a column convected; ValueError where nsteps == 0"""
        if self.nsteps == 0:
            raise ValueError("BettsMiller: no application counted (nsteps == 0)")
        return self.count / self.nsteps


def betts_miller_columns(p, theta, q, sig, dsig, ptop=0.0, dt=0.0, **params):
    """the column rule of the Betts-Miller convection (gcm_betts_miller_columns; the host build of the routines the
    kernel calls, no handle, no device) over columns theta, q of shape (..., L), level 0 the bottom, with p (...) (Pa,
    surface pressure minus ptop), sig and dsig (L,) and the step dt -> dict(theta, q (..., L): the columns as the phase
    leaves them; precip (...): P_q, 0 where the column did not convect; kt (...): the cloud top, -1 where it did not;
    k_lcl (...): the LCL's level, -1 where there is none; margin (...): the smallest relative distance of a comparison
    the column consulted).  ValueError for a refused parameter"""
    theta = np.asarray(theta, dtype=np.float64)
    L = theta.shape[-1] if theta.ndim else 0
    tt = as_f64(theta.reshape(-1, L) if L else theta, name="theta")
    qq = as_f64(q, theta.shape, "q").reshape(tt.shape)
    n = tt.shape[0] if L else 0
    pp = as_f64(np.asarray(p, dtype=np.float64).reshape(n), name="p")
    ss, dd = as_f64(np.asarray(sig, dtype=np.float64).reshape(-1), (L,), "sig"), as_f64(np.asarray(dsig, dtype=np.float64).reshape(-1), (L,), "dsig")
    rec = _lib.BettsMiller(*betts_miller_params(params).values())
    to, qo, pr, mg = np.empty_like(tt), np.empty_like(tt), np.empty(n), np.empty(n)
    kt, kl = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    i32 = C.POINTER(C.c_int32)
    _check(lib.gcm_betts_miller_columns(n, L, _tab(pp), _tab(tt), _tab(qq), _tab(ss), _tab(dd), float(ptop), float(dt), C.byref(rec),
                                        _tab(to), _tab(qo), _tab(pr), kt.ctypes.data_as(i32), kl.ctypes.data_as(i32), _tab(mg)))
    lead = theta.shape[:-1]
    return dict(theta=to.reshape(theta.shape), q=qo.reshape(theta.shape), precip=pr.reshape(lead), kt=kt.reshape(lead),
                k_lcl=kl.reshape(lead), margin=mg.reshape(lead))


class _ColumnPhase:
    """what tells the phases with per-column sums apart -- the boundary layer, the convective adjustment, the Betts-Miller
    convection and the moist physics, in the model's order in STEP_COLUMN_PHASES (COLUMN_PHASES: the three of them that
    came first) -- for Core's seven operations on each and for checkpoint.py: the name in the entry
    points and keys, the words of the messages, the ctypes record, the *_params function with its defaults (the record's
    order), the result namedtuple (its last two fields name the sums) and whether *_step takes dt"""

    def __init__(self, name, what, record, params, defaults, result, step_takes_dt):
        self.name, self.what, self.record, self.params, self.defaults = name, what, record, params, defaults
        self.result, self.fields, self.step_takes_dt = result, result._fields[2:], step_takes_dt
        self.set, self.on, self.step, self.get, self.put, self.reset = (
            getattr(lib, "gcm_" + f % name) for f in ("set_%s", "%s_on", "%s_step", "get_%s", "put_%s", "%s_reset"))


_CONVECT = _ColumnPhase("convect", "convective adjustment", _lib.Convect, convect_params, CONVECT_DEFAULTS, Convect, False)
_MOIST = _ColumnPhase("moist", "moist physics", _lib.Moist, moist_params, MOIST_DEFAULTS, Moist, True)
_BOUNDARY = _ColumnPhase("boundary_layer", "boundary layer", _lib.BoundaryLayer, boundary_layer_params,
                         BOUNDARY_LAYER_DEFAULTS, BoundaryLayer, True)
_BETTS_MILLER = _ColumnPhase("betts_miller", "Betts-Miller convection", _lib.BettsMiller, betts_miller_params,
                             BETTS_MILLER_DEFAULTS, BettsMiller, True)
COLUMN_PHASES = (_BOUNDARY, _CONVECT, _MOIST)
# every column phase in the order a step applies them: what checkpoint.py walks
STEP_COLUMN_PHASES = (_BOUNDARY, _CONVECT, _BETTS_MILLER, _MOIST)


class _Sampler:
    """what tells the sampled diagnostics apart -- the zonal-mean climatology, the pressure-level climatology, the
    spectra and the pressure-level maps, in the order a step samples them in SAMPLERS -- for Core's operations on each
    and for checkpoint.py: the name in the entry points and keys; the names of gcm_put_<name>'s sum arrays, their keys in
    a checkpoint file and their shapes as a function of the core; what the registration takes besides `every` (the file
    key and the Core property that returns it: the targets, mmax; None: nothing); the words of gcm_<name>_plan (None: no
    such query); and record(core, n, *sums), the result's from_sums"""

    def __init__(self, name, args, keys, shapes, extra, plan, record):
        self.name, self.args, self.keys, self.shapes, self.extra, self.plan, self.record = name, args, keys, shapes, extra, plan, record
        self.set, self.every, self.sample, self.reset, self.get, self.put = (
            getattr(lib, "gcm_" + f % name) for f in ("set_%s", "%s_every", "%s_sample", "%s_reset", "get_%s", "put_%s"))
        self.plan_of = getattr(lib, "gcm_%s_plan" % name) if plan else None


_CLIMATE = _Sampler("climate", ("m3", "m2"), ("m3", "m2"),
                    lambda c: ((_lib.CLIM_WORDS3, c.L, c.H), (_lib.CLIM_WORDS2, c.H)), None, None,
                    lambda c, n, m3, m2: Climate.from_sums(n, m3, m2, c.W))
_PLEV_CLIMATE = _Sampler("plev_climate", ("s",), ("sums",),
                         lambda c: ((_lib.PLEV_WORDS, c.plev_climate_levels.size, c.H),), ("plev", "plev_climate_levels"),
                         ("grid_x", "nseg", "targets", "threads", "lds_bytes", "chunks"),
                         lambda c, n, s: PlevClimate.from_sums(n, c.plev_climate_levels, s, c.W))
_SPECTRA = _Sampler("spectra", ("s",), ("s",),
                    lambda c: ((_lib.SPEC_WORDS, c.L, c.H, c.spectra_mmax + 1),), ("mmax", "spectra_mmax"),
                    ("grid_x", "nseg", "threads", "lds_bytes", "passes", "per_thread"),
                    lambda c, n, s: Spectra.from_sums(n, s, c.W))
_PLEV_MAPS = _Sampler("plev_maps", ("s", "s2"), ("sums", "sums2"),
                      lambda c: ((_lib.PLEV_MAP_WORDS, c.plev_maps_levels.size, c.H, c.W), (_lib.PLEV_MAP_WORDS2, c.H, c.W)),
                      ("plev", "plev_maps_levels"), ("chunks", "rows", "threads", "lds_bytes", "targets"),
                      lambda c, n, s, s2: PlevMaps.from_sums(n, c.plev_maps_levels, s, s2))
SAMPLERS = (_CLIMATE, _PLEV_CLIMATE, _SPECTRA, _PLEV_MAPS)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _tab(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


class Core:
    """Owns a gcm_handle.  Field order of set/get is (p, u, v, t, q)."""

    def __init__(self, model, width, height, layers=1, dx=0.0, tracer=_lib.TRACER_NONE,
                 variant=_lib.VARIANT_AUTO, geom=None, filter=True, nranks=1, rank=0,
                 global_height=None, row0=0, device=-1, stream=None, halo_steps=1, coriolis=False, dtype="f64",
                 members=1, band_tracers=0, tracer_scheme=None, band_tracer_rows=1, band_boundary_layer=False,
                 band_horizontal_diffusion=False):
        """band_tracers: a GCM_PE25D latitude band (nranks > 1) that carries that many passive tracers
        (gcm_set_band_tracers, right after gcm_create: the ghost-row message and halo_bytes() include them);
        band_tracer_rows: the ghost rows per side those tracers carry, 1 (default) or 2 (what "van_leer" reads on a
        band; gcm_set_band_tracer_rows, right after gcm_create and ahead of the scheme: the message carries that
        many rows of every tracer, and every band of a run must declare the same);
        tracer_scheme: the passive tracers' transport scheme (set_tracer_scheme), GCM_PE25D only;
        band_boundary_layer: a GCM_PE25D latitude band that takes the boundary layer over its own rows
        (gcm_set_band_boundary_layer, right after gcm_create): set_boundary_layer is then accepted, and every step takes
        a third exchange of the edge rows behind the phase -- band_run does it itself, a host-driven step goes
        end_step_begin, exchange, end_step_finish.  Every band of a run must declare the same;
        band_horizontal_diffusion: a GCM_PE25D latitude band that takes the horizontal diffusion over its own rows
        (gcm_set_band_hdiff, right after gcm_create): set_horizontal_diffusion is then accepted, and every step takes one
        more exchange of the edge rows behind the phase -- band_run does it itself, a host-driven step goes
        end_step_diffuse, exchange, end_step_begin.  Every band of a run must declare the same"""
        check_dtype(dtype)
        scheme = tracer_scheme_id(tracer_scheme)
        if scheme != _lib.TRACER_NONE and model != _lib.PE25D:
            raise ValueError("tracer_scheme needs GCM_PE25D (the 2-D models take tracer=)")
        band_tracers = int(band_tracers)
        if not 0 <= band_tracers <= _lib.MAX_TRACERS:
            raise ValueError("band_tracers=%d: 0 .. %d" % (band_tracers, _lib.MAX_TRACERS))
        if band_tracers > 0 and (model != _lib.PE25D or nranks <= 1):
            raise ValueError("band_tracers needs a GCM_PE25D latitude band (nranks > 1); a single domain takes "
                             "set_tracers directly")
        is_pe_band = model == _lib.PE25D and nranks > 1
        # (0: what the band_tracer_rows property of anything but a GCM_PE25D band reports, and its checkpoints carry)
        if isinstance(band_tracer_rows, bool) or band_tracer_rows not in ((1, 2) if is_pe_band else (0, 1, 2)):
            raise ValueError("band_tracer_rows must be 1 or 2, got %r" % (band_tracer_rows,))
        if band_tracer_rows == 2 and not is_pe_band:
            raise ValueError("band_tracer_rows needs a GCM_PE25D latitude band (nranks > 1); a single domain's rows "
                             "wrap and carry no ghost rows")
        band_tracer_rows = int(band_tracer_rows) if is_pe_band else 0
        if band_boundary_layer not in (0, 1, False, True):
            raise ValueError("band_boundary_layer must be True or False, got %r" % (band_boundary_layer,))
        band_boundary_layer = bool(band_boundary_layer)
        if band_boundary_layer and not is_pe_band:
            raise ValueError("band_boundary_layer needs a GCM_PE25D latitude band (nranks > 1); a single domain takes "
                             "set_boundary_layer directly")
        if band_horizontal_diffusion not in (0, 1, False, True):
            raise ValueError("band_horizontal_diffusion must be True or False, got %r" % (band_horizontal_diffusion,))
        band_horizontal_diffusion = bool(band_horizontal_diffusion)
        if band_horizontal_diffusion and not is_pe_band:
            raise ValueError("band_horizontal_diffusion needs a GCM_PE25D latitude band (nranks > 1); a single domain takes "
                             "set_horizontal_diffusion directly")
        self.model, self.W, self.H, self.L = model, int(width), int(height), int(layers)
        # ensemble members (2-D models, single band): every field is (M, H, W) when M > 1
        self.members = max(int(members), 1)
        self.nranks, self.rank = nranks, rank
        # what a checkpoint needs to rebuild this handle (checkpoint.save / restore)
        self.options = dict(dx=float(dx), tracer=int(tracer), variant=int(variant), filter=bool(filter),
                            nranks=int(nranks), rank=int(rank), row0=int(row0), halo_steps=int(halo_steps),
                            coriolis=bool(coriolis), dtype=dtype, members=int(members), band_tracers=band_tracers,
                            tracer_scheme=_lib.TRACER_NONE, band_tracer_rows=band_tracer_rows,
                            band_boundary_layer=band_boundary_layer,
                            band_horizontal_diffusion=band_horizontal_diffusion,
                            global_height=int(height if global_height is None else global_height))
        self.has_ground = False
        self._forcing = {}                      # tracer -> the forcing record registered (set_tracer_forcing)
        self._mixing = {}                       # tracer -> the profile K registered (set_tracer_mixing)
        self._held_suarez = None                # the parameters and latitudes registered (set_held_suarez)
        self._hdiff = None                      # the parameters registered (set_horizontal_diffusion)
        self._column = {}                       # the parameters registered (set_boundary_layer, set_convect, set_moist), by the phase's name
        self._slab = None                       # the parameters and fields registered (set_slab_ocean)
        self._gas = None                        # the parameters registered (set_gas_radiation)
        self._phys = None                       # t_lw, t_sw, albedo registered (set_physics): the slab ocean's ASR
        self._sigma_levels = None                     # GCM_PE25D: (sig, dsig) of the geometry
        cfg = _lib.Config()
        cfg.abi_version = _lib.ABI_VERSION
        cfg.model = model
        cfg.width, cfg.height, cfg.layers = self.W, self.H, self.L
        cfg.tracer, cfg.variant, cfg.filter = tracer, variant, 1 if filter else 0
        cfg.nranks, cfg.rank = nranks, rank
        cfg.global_height = self.H if global_height is None else int(global_height)
        self.global_height = cfg.global_height
        cfg.row0 = row0
        cfg.device = device
        cfg.halo_steps = halo_steps
        cfg.members = int(members)
        cfg.dtype = DTYPES[dtype]
        self.dtype = dtype
        self.halo_steps = halo_steps
        cfg.dx = float(dx)
        cfg.stream = stream
        self._keep = []
        if model == _lib.PE25D:
            if geom is None:
                raise ValueError("GCM_PE25D needs a geometry (gcmiipy_amd.geometry.gen_geometry)")
            gh = cfg.global_height

            def tab(x, n):
                a = as_f64(np.asarray(x, dtype=np.float64).reshape(-1), (n,), "geometry table")
                self._keep.append(a)
                return _tab(a)

            cfg.dy = float(geom.dy)
            cfg.ptop = float(geom.ptop)
            cfg.dx_j, cfg.dx_h = tab(geom.dx_j, gh), tab(geom.dx_h, gh)
            cfg.sig, cfg.dsig = tab(geom.sig, self.L), tab(geom.dsig, self.L)
            cfg.sigb, cfg.sigt = tab(geom.sigb, self.L), tab(geom.sigt, self.L)
            self._sigma_levels = (self._keep[-4], self._keep[-3])
            cfg.heightmap = tab(geom.heightmap, gh * self.W)
            if coriolis:
                from .geometry import coriolis_tables
                cu, cv = coriolis_tables(geom)
                cfg.cor_u, cfg.cor_v = tab(cu, gh), tab(cv, gh)
        self._h = _lib._H()
        rc = lib.gcm_create(C.byref(cfg), C.byref(self._h))
        if rc != _lib.OK:
            msg = lib.gcm_last_error(None).decode()
            self._h = None
            if rc == _lib.ERR_ARG:
                raise ValueError(msg)
            raise GcmError("gcm_create failed (%d): %s" % (rc, msg))
        try:
            if band_tracers > 0:
                _check(lib.gcm_set_band_tracers(self._h, band_tracers), self._h)
            if band_tracer_rows == 2:
                _check(lib.gcm_set_band_tracer_rows(self._h, band_tracer_rows), self._h)
            if scheme != _lib.TRACER_NONE:
                self.set_tracer_scheme(scheme)
            if band_boundary_layer:
                _check(lib.gcm_set_band_boundary_layer(self._h, 1), self._h)
            if band_horizontal_diffusion:
                _check(lib.gcm_set_band_hdiff(self._h, 1), self._h)
        except Exception:
            self.close()
            raise
        self.is3d = model == _lib.PE25D
        self.fields = {_lib.SW2D: (_lib.P, _lib.U, _lib.V),
                       _lib.SW2D_TEMP: (_lib.P, _lib.U, _lib.V, _lib.T) +
                       ((_lib.Q,) if tracer != _lib.TRACER_NONE else ()),
                       }.get(model, (_lib.P, _lib.U, _lib.V, _lib.T, _lib.Q))

    # -- shapes ----------------------------------------------------------------
    def shape_of(self, field):
        if self.is3d and field != _lib.P:
            return (self.L, self.H, self.W)
        if self.members > 1:
            return (self.members, self.H, self.W)
        return (self.H, self.W)

    def _prep_in(self, arrs):
        out = []
        for f, a in enumerate(arrs):
            out.append(None if a is None else as_f64(a, self.shape_of(f), "puvtq"[f]))
        return out

    # -- state -------------------------------------------------------------------
    def set_state(self, p=None, u=None, v=None, t=None, q=None):
        a = self._prep_in((p, u, v, t, q))
        _check(lib.gcm_set_state(self._h, *[_ptr(x) for x in a]), self._h)

    def set_star(self, p=None, u=None, v=None, t=None, q=None):
        a = self._prep_in((p, u, v, t, q))
        _check(lib.gcm_set_star(self._h, *[_ptr(x) for x in a]), self._h)

    def _get(self, fn, fields):
        out = [np.empty(self.shape_of(f)) if f in fields else None for f in range(5)]
        _check(fn(self._h, *[_ptr(x) for x in out]), self._h)
        return out

    def get_state(self, fields=None):
        """-> [p, u, v, t, q] (None for fields not requested / not in the model)"""
        return self._get(lib.gcm_get_state, self.fields if fields is None else fields)

    def get_star(self, fields=(_lib.P, _lib.U, _lib.V, _lib.T)):
        return self._get(lib.gcm_get_star, fields)

    # -- ensemble members ------------------------------------------------------------------
    def set_member(self, m, p=None, u=None, v=None, t=None, q=None):
        """member m's (H, W) fields alone (gcm_set_member)"""
        a = [None if x is None else as_f64(x, (self.H, self.W), "puvtq"[f]) for f, x in enumerate((p, u, v, t, q))]
        _check(lib.gcm_set_member(self._h, int(m), *[_ptr(x) for x in a]), self._h)

    def get_member(self, m, fields=None):
        """-> [p, u, v, t, q] of member m, each (H, W) (None for fields not requested / not in the model)"""
        fields = self.fields if fields is None else fields
        out = [np.empty((self.H, self.W)) if f in fields else None for f in range(5)]
        _check(lib.gcm_get_member(self._h, int(m), *[_ptr(x) for x in out]), self._h)
        return out

    def diag_members(self, kind):
        """-> (M,) array: diag(kind) of every member, by one launch and one synchronisation"""
        out = np.empty(self.members)
        _check(lib.gcm_diag_members(self._h, int(kind), _tab(out), self.members), self._h)
        return out

    # -- passive tracers (GCM_PE25D; a latitude band: Core(..., band_tracers=n)) ----------
    def set_tracers(self, c):
        """carry the tracers c (n, L, H, W) from now on (n = 0 or None: none); every stage advances them
        with the update of q (gcm_set_tracers).  A band: its own rows, n = the declared band_tracers"""
        a = tracer_array(c, self.L, self.H, self.W)
        n_before = lib.gcm_tracer_count(self._h)
        _check(lib.gcm_set_tracers(self._h, a.shape[0], _ptr(a) if a.shape[0] else None), self._h)
        if a.shape[0] != n_before:
            self._forcing.clear()               # (another count drops the forcing: gcm_set_tracer_forcing)
            self._mixing.clear()                # (and the mixing: gcm_set_tracer_mixing)

    def get_tracers(self, star=False):
        """-> (n, L, H, W): the current tracers, or with star=True those of the last predictor"""
        out = np.empty((self.tracer_count, self.L, self.H, self.W))
        _check(lib.gcm_get_tracers(self._h, 1 if star else 0, _ptr(out) if out.size else None), self._h)
        return out

    def tracer_stats(self, star=False, with_q=False):
        """-> TracerStats of the current tracers (star=True: those of the last predictor), reduced on the device
        over the handle's own rows -- a band's ghost rows are never read, bands.merge_tracer_stats gives the global
        figure; with_q adds q of the same state as the last entry.  48 bytes per entry come back
        (gcm_tracer_stats)"""
        n = self.tracer_count + (1 if with_q else 0)
        out = np.empty((max(n, 1), _lib.TRACER_STATS_WORDS))
        _check(lib.gcm_tracer_stats(self._h, 1 if star else 0, 1 if with_q else 0, _ptr(out), n * _lib.TRACER_STATS_WORDS),
               self._h)
        r = out[:n]
        return TracerStats(r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy(), r[:, 3].copy(),
                           r[:, 4].astype(np.int64), r[:, 5].astype(np.int64))

    # -- forcing of the passive tracers (gcm_set_tracer_forcing) ---------------------------
    def set_tracer_forcing(self, i, source=0.0, decay=0.0, emission=None, pin_mask=None, pin_value=0.0):
        """force tracer i from the next step on, on the device, once per Matsuno step right behind the corrector:
            c1 = c + dt * (source + emission);  c2 = c1 * exp(-decay * dt);  c = pin_value where pin_mask else c2
        in the handle's real type, every operation rounded on its own.  source: c per second (an age-of-air clock:
        1.0); decay >= 0 in 1 / s; emission (L, H, W) in c per second or None; pin_mask (L, H, W) bool or uint8 or
        None: the cells held at pin_value.  A band: its own rows.  Replaces an earlier forcing of tracer i; it
        survives set_tracers with the same count, set_tracer_scheme and set_state, and goes with set_tracers of
        another count.  The predictor's tracers (get_tracers(star=True)) and q are never forced.  ValueError for a
        wrong shape or value (a refused call changes nothing)"""
        shape = (self.L, self.H, self.W)
        e = None if emission is None else as_f64(emission, shape, "emission")
        m = None
        if pin_mask is not None:
            m = np.asarray(pin_mask)
            if m.dtype != np.bool_ and m.dtype != np.uint8:
                raise ValueError("pin_mask must be bool or uint8, got %s" % (m.dtype,))
            if m.shape != shape:
                raise ValueError("pin_mask has shape %s, expected %s" % (m.shape, shape))
            m = np.ascontiguousarray(m != 0, dtype=np.uint8)
        rec = _lib.TracerForcing()
        rec.source, rec.decay, rec.pin_value = float(source), float(decay), float(pin_value)
        rec.emission = _tab(e)
        rec.pin_mask = None if m is None else m.ctypes.data_as(C.POINTER(C.c_ubyte))
        _check(lib.gcm_set_tracer_forcing(self._h, int(i), C.byref(rec)), self._h)
        self._forcing[int(i)] = dict(source=rec.source, decay=rec.decay, emission=None if e is None else e.copy(),
                                     pin_mask=None if m is None else m.astype(np.bool_), pin_value=rec.pin_value)

    def clear_tracer_forcing(self, i=None):
        """tracer i is no longer forced (None: no tracer is)"""
        _check(lib.gcm_set_tracer_forcing(self._h, -1 if i is None else int(i), None), self._h)
        if i is None:
            self._forcing.clear()
        else:
            self._forcing.pop(int(i), None)

    def tracer_forcing(self, i):
        """-> the forcing this object registered for tracer i, dict(source, decay, emission, pin_mask, pin_value) (a
        host copy), or None where the handle carries none (gcm_tracer_forced) -- and also None for a forcing that was
        registered through the C call directly, of which this object holds no copy"""
        on = _count(lib.gcm_tracer_forced(self._h, int(i)), self._h)
        return self._forcing.get(int(i)) if on else None

    def tracer_forcings(self):
        """-> {i: record} of every forced tracer (see tracer_forcing)"""
        out = {}
        for i in range(self.tracer_count if self.model == _lib.PE25D else 0):
            r = self.tracer_forcing(i)
            if r is not None:
                out[i] = r
        return out

    # -- implicit vertical mixing of the passive tracers (gcm_set_tracer_mixing) --------------
    def set_tracer_mixing(self, i, k):
        """mix tracer i in the column from the next step on, on the device, once per Matsuno step behind the corrector
        and in front of the forcing: backward-Euler diffusion of the mixing ratio in sigma with zero flux at the top
        and the bottom.  k (L - 1,): the diffusivity at the interface between levels m and m + 1 in sigma^2 / s,
        finite and >= 0, the same in every column (all zeros: the identity).  Replaces an earlier profile of tracer i;
        the life cycle is the forcing's.  The predictor's tracers (get_tracers(star=True)) and q are never mixed.
        ValueError for a wrong shape or value (a refused call changes nothing)"""
        a = as_f64(k, (self.L - 1,), "k")
        _check(lib.gcm_set_tracer_mixing(self._h, int(i), _tab(a), a.shape[0]), self._h)
        self._mixing[int(i)] = a.copy()

    def clear_tracer_mixing(self, i=None):
        """tracer i is no longer mixed (None: no tracer is)"""
        _check(lib.gcm_set_tracer_mixing(self._h, -1 if i is None else int(i), None, 0), self._h)
        if i is None:
            self._mixing.clear()
        else:
            self._mixing.pop(int(i), None)

    def tracer_mixing(self, i):
        """-> the profile K (L - 1,) this object registered for tracer i (a host copy), or None where the handle
        carries none (gcm_tracer_mixed) -- and also None for a profile that was registered through the C call
        directly, of which this object holds no copy"""
        on = _count(lib.gcm_tracer_mixed(self._h, int(i)), self._h)
        return self._mixing.get(int(i)) if on else None

    def tracer_mixings(self):
        """-> {i: K} of every mixed tracer (see tracer_mixing)"""
        out = {}
        for i in range(self.tracer_count if self.model == _lib.PE25D else 0):
            k = self.tracer_mixing(i)
            if k is not None:
                out[i] = k
        return out

    # -- convective mixing of the passive tracers (gcm_set_tracer_convect) --------------------
    def set_tracer_convection(self, i, on=True):
        """tracer i is mixed in the blocks of the convective adjustment from its next application on (on=False: no
        longer), on the device, by a launch immediately ahead of the adjustment's -- at the end of a step with
        set_convect registered, and in convect_step: in every block the adjustment merges, the tracer becomes its mean
        weighted with dsig.  mix_q plays no part.  Single domains only: a latitude band raises the library's refusal.
        The life cycle is the forcing's.  A refused call changes nothing"""
        _check(lib.gcm_set_tracer_convect(self._h, int(i), 1 if on else 0), self._h)

    def tracer_convected(self, i):
        """-> whether tracer i has opted in (gcm_tracer_convected)"""
        return bool(_count(lib.gcm_tracer_convected(self._h, int(i)), self._h))

    def tracer_convections(self):
        """-> the indices of the tracers that have opted in, ascending"""
        return [i for i in range(self.tracer_count if self.model == _lib.PE25D else 0) if self.tracer_convected(i)]

    def set_tracer_scheme(self, scheme):
        """the transport scheme of the passive tracers from the next stage on: "centred" (the update of q, the
        default), "upwind" (donor-cell face values) or "van_leer" (donor-cell + the van Leer limited correction; on a
        latitude band only with band_tracer_rows=2: it reads rows j -+ 2), or the _lib.TRACER_* constants
        (gcm_set_tracer_scheme).  q is not affected; a refused call changes nothing"""
        scheme = tracer_scheme_id(scheme)
        _check(lib.gcm_set_tracer_scheme(self._h, scheme), self._h)
        self.options["tracer_scheme"] = scheme

    @property
    def tracer_scheme(self):
        """the scheme in force, as a _lib.TRACER_* constant"""
        return _count(lib.gcm_tracer_scheme(self._h), self._h)

    @property
    def band_tracer_rows(self):
        """the ghost rows per side a band's tracers carry (gcm_band_tracer_rows); 0: not a GCM_PE25D band"""
        return _count(lib.gcm_band_tracer_rows(self._h), self._h)

    @property
    def tracer_count(self):
        return _count(lib.gcm_tracer_count(self._h), self._h)

    # -- stepping ------------------------------------------------------------------
    def step(self, nsteps, dt):
        _check(lib.gcm_step(self._h, int(nsteps), float(dt)), self._h)

    def sw2d_fused_depth(self):
        """rows of requests a wave of the next step's fused launch keeps in flight (gcm_sw2d_fused_depth): 1, or 3 for
        the deep march (float64 GCM_SW2D_TEMP on a streaming grid, or GCM_SW2D_DEPTH=3 when the handle was created);
        0 for the staged variant"""
        d = lib.gcm_sw2d_fused_depth(self._h)
        _check(min(d, 0), self._h)
        return d

    def sw2d_plan(self, nsteps):
        """what step(nsteps, .) of a 2-D handle would launch, without launching anything (gcm_sw2d_plan): a dict of
        variant ("fused" / "staged"), rows_per_band, cols (columns per lane), strip and strip2 (the strip width in
        columns of the single-step and of the two-step kernel), two_step_launches, single_step_launches, preload and
        stream (the single-step kernel's form).  GCM_SW2D_TWO_STEP is read by this call as step reads it"""
        out = (C.c_int * _lib.SW2D_PLAN_WORDS)()
        _check(lib.gcm_sw2d_plan(self._h, int(nsteps), out, _lib.SW2D_PLAN_WORDS), self._h)
        return dict(variant={_lib.VARIANT_FUSED: "fused", _lib.VARIANT_STAGED: "staged"}[out[0]],
                    rows_per_band=out[1], cols=out[2], strip=out[3], strip2=out[4], two_step_launches=out[5],
                    single_step_launches=out[6], preload=bool(out[7]), stream=bool(out[8]))

    def sw2d_pair(self):
        """the wave pair of float64 GCM_SW2D_TEMP, two steps per launch (gcm_sw2d_pair_info): a dict of active (a
        step(n >= 2, .) goes through it: GCM_SW2D_PAIR=0|1 when the handle was created, else the library's default)
        and rows_per_band (its own band length, GCM_SW2D_PAIR_ROWS pins it; 0: a handle the pair never serves)"""
        out = (C.c_int * _lib.SW2D_PAIR_WORDS)()
        _check(lib.gcm_sw2d_pair_info(self._h, out, _lib.SW2D_PAIR_WORDS), self._h)
        return dict(active=bool(out[0]), rows_per_band=out[1])

    def phase_plan(self, phase, rows=None, accumulate=True):
        """the launch geometry of a GCM_PE25D phase over `rows` rows (None: the handle's own; the explicit phase calls
        of a band launch its four ghost rows too), without launching anything (gcm_pe25d_phase_plan).  phase:
        "held_suarez", "moist" (accumulate: the launch adds to the registered sums), "climate" or "tracer_forcing";
        the dict is that of phase_geometry below, at the handle's own width, levels, element size and compute units"""
        out = (C.c_int * _lib.PHASE_PLAN_WORDS)()
        _check(lib.gcm_pe25d_phase_plan(self._h, phase_id(phase), -1 if rows is None else int(rows), int(bool(accumulate)),
                                        out, _lib.PHASE_PLAN_WORDS), self._h)
        return _phase_dict(phase_id(phase), out)

    def stage_plan(self):
        """what a GCM_PE25D dynamics stage of this handle launches, without launching anything (gcm_pe25d_stage_plan):
        the dict of stage_geometry below at the handle's own sizes, compute units and GCM_PE_* switches, for a stage over
        all its rows.  A band that splits its stage into edge and interior rows adds band = 1, k1_split and the own
        rows' K1 launch of gcm_band_run (k1_own_workgroups_per_row, k1_own_pairs_per_wg, k1_own_pairs_last_wg), K4 of
        the edge rows (k4_edge_groups, k4_edge_rows_last_group, k4_edge_oddtop, k4_edge_grid, in nseg_edge level
        segments) and of the interior rows (k4_int_*)"""
        out = (C.c_int * _lib.STAGE_PLAN_WORDS)()
        _check(lib.gcm_pe25d_stage_plan(self._h, out, _lib.STAGE_PLAN_WORDS), self._h)
        return _stage_dict(out, bool(out[_lib.STAGE_BAND_WORD]))

    def half_step(self, stage, dt):
        _check(lib.gcm_half_step(self._h, int(stage), float(dt)), self._h)

    def end_step(self, dt):
        """the end of a GCM_PE25D step whose dynamics the caller took itself (gcm_end_step): every registered phase in
        the order of step() / band_run() -- the solar step at the handle's clock, which advances, Held-Suarez, the
        boundary layer, the convective adjustment, the Betts-Miller convection, the moist physics, the climatology's sample where one is due.  half_step(0),
        half_step(1), end_step(dt) is step(1, dt).  A band: own rows and ghost rows, the ghost rows must be current; a band
        with the boundary layer registered is refused (GcmError): end_step_begin, exchange, end_step_finish"""
        _check(lib.gcm_end_step(self._h, float(dt)), self._h)

    def end_step_diffuse(self, dt):
        """the part of a host-driven step ahead of end_step_begin (gcm_end_step_diffuse): the registered horizontal
        diffusion over the own rows of a band that carries it (band_horizontal_diffusion=True), behind the unpack of the
        post-corrector exchange.  The caller then exchanges the current state (halo_pack2, the transfer, halo_unpack2)
        and calls end_step_begin, which such a band refuses without this call.  Every other handle: nothing happens"""
        _check(lib.gcm_end_step_diffuse(self._h, float(dt)), self._h)

    def end_step_begin(self, dt):
        """the first part of end_step (gcm_end_step_begin): the solar step, the clock, Held-Suarez, the boundary layer (a
        band: over its own rows).  A band with the boundary layer registered then exchanges the ghost rows of the current
        state (halo_pack2, the transfer, halo_unpack2) ahead of end_step_finish; on every other handle nothing needs to
        happen between the two, and begin + finish is end_step"""
        _check(lib.gcm_end_step_begin(self._h, float(dt)), self._h)

    def end_step_finish(self, dt):
        """the second part of end_step (gcm_end_step_finish): the convective adjustment and the moist physics over own rows
        and ghost rows, the climatology's sample where one is due"""
        _check(lib.gcm_end_step_finish(self._h, float(dt)), self._h)

    def get_intermediate(self, kind):
        """parity tap (GCM_PE25D): spu, pit, p_n, phi or pgfu of the last half step, as the stage kernels
        left them in the handle (gcm_get_intermediate; _lib.INT_*)"""
        two_d = kind in (_lib.INT_PIT, _lib.INT_PN)
        out = np.empty((self.H, self.W) if two_d else (self.L, self.H, self.W))
        _check(lib.gcm_get_intermediate(self._h, int(kind), _ptr(out)), self._h)
        return out

    def snapshot(self):
        """device-side copy of the current state (2-D models)"""
        _check(lib.gcm_snapshot(self._h), self._h)

    def restore(self):
        """current state <- snapshot, asynchronously on the handle's stream"""
        _check(lib.gcm_restore(self._h), self._h)

    def sync(self):
        _check(lib.gcm_sync(self._h), self._h)

    def diag(self, kind):
        out = C.c_double()
        _check(lib.gcm_diag(self._h, kind, C.byref(out)), self._h)
        return out.value

    def energy(self, area):
        """(ke, ate, geo, total), no_limits_2_5d.calc_energy"""
        a = as_f64(np.asarray(area, dtype=np.float64).reshape(-1), name="area")
        out = (C.c_double * 4)()
        _check(lib.gcm_energy(self._h, _tab(a), a.size, out), self._h)
        return tuple(out)

    def stats(self, area):
        """the STATS record of full_timestep (no_limits_2_5d.py:85-91) by one launch and one
        synchronisation -> dict(u_max, u_min, v_max, v_min, ke=(ke, ate, geo, total), nans)"""
        a = as_f64(np.asarray(area, dtype=np.float64).reshape(-1), name="area")
        out = (C.c_double * 9)()
        _check(lib.gcm_stats(self._h, _tab(a), a.size, out), self._h)
        return {"u_max": out[0], "u_min": out[1], "v_max": out[2], "v_min": out[3],
                "ke": (out[4], out[5], out[6], out[7]), "nans": out[8]}

    def total_variation(self, field):
        """constants.get_total_variation of one field of the resident state (constants.py:105-108):
        sum |q - roll(q, -1, 0)| over axis 0 of the reference layout, by a device reduction"""
        return self.diag(_lib.DIAG_TV_P + int(field))

    def polar_filter(self, q):
        """low_pass.arakawa_1977 on a (H, W) or (n, H, W) field of this handle's grid (any n: the
        levels go through the handle `layers` at a time)"""
        a = as_f64(q, name="q")
        if a.ndim not in (2, 3) or a.shape[-2:] != (self.H, self.W):
            raise ValueError("q has shape %s, expected (..., %d, %d)" % (a.shape, self.H, self.W))
        a3 = a.reshape(-1, self.H, self.W)
        out = np.empty_like(a3)
        for k0 in range(0, a3.shape[0], self.L):
            k1 = min(k0 + self.L, a3.shape[0])
            _check(lib.gcm_polar_filter(self._h, k1 - k0, _ptr(a3[k0:k1]), _ptr(out[k0:k1])), self._h)
        return out.reshape(a.shape)

    # -- column physics (GCM_PE25D) ----------------------------------------------------
    def set_ground(self, gt):
        _check(lib.gcm_set_ground(self._h, _ptr(as_f64(gt, (self.H, self.W), "gt"))), self._h)
        self.has_ground = True

    def get_ground(self):
        out = np.empty((self.H, self.W))
        _check(lib.gcm_get_ground(self._h, _ptr(out)), self._h)
        return out

    def _latlon(self, geom):
        lat = as_f64(np.asarray(geom.lat, dtype=np.float64).reshape(-1), (self.global_height,), "lat")
        lon = as_f64(np.asarray(geom.long, dtype=np.float64).reshape(-1), (self.W,), "long")
        return lat, lon

    def grey_radiation(self, geom, utc, t_lw=0.1, t_sw=0.9, albedo=0.3):
        """-> (dTdt [L,H,W], dt_ground [H,W]), grey_solar.basic_grey_radiation.  ValueError for a refused parameter
        (grey_params; the call then changes nothing)"""
        t_lw, t_sw, albedo = grey_params(t_lw, t_sw, albedo, utc=utc)
        lat, lon = self._latlon(geom)
        dT, dg = np.empty((self.L, self.H, self.W)), np.empty((self.H, self.W))
        _check(lib.gcm_grey_radiation(self._h, float(utc), t_lw, t_sw, albedo, _tab(lat), _tab(lon),
                                      _ptr(dT), _ptr(dg)), self._h)
        return dT, dg

    def solar_step(self, geom, dt, utc, t_lw=0.1, t_sw=0.9, albedo=0.3):
        """no_limits_2_5d.solar_timestep in place.  ValueError for a refused parameter (grey_params; the call then
        changes nothing)"""
        t_lw, t_sw, albedo = grey_params(t_lw, t_sw, albedo, utc=utc, dt=dt)
        lat, lon = self._latlon(geom)
        _check(lib.gcm_solar_step(self._h, float(dt), float(utc), t_lw, t_sw, albedo, _tab(lat),
                                  _tab(lon)), self._h)

    def set_physics(self, geom, utc=0.0, t_lw=0.1, t_sw=0.9, albedo=0.3):
        """every step of step() / band_run() / end_step() from now on = the dynamics step followed by
        no_limits_2_5d.solar_timestep at the handle's clock, which then advances by dt (run_model's loop,
        no_limits_2_5d.py:229-234).  That clock, utc(), is the only one: whoever drives the steps, it starts at `utc`
        and counts every one of them.  geom=None switches the physics off (gcm_set_physics).  ValueError for a refused
        parameter (grey_params; the registration in place, if any, then stays as it is)"""
        if geom is None:
            _check(lib.gcm_set_physics(self._h, None), self._h)
            self._phys = None
            return
        t_lw, t_sw, albedo = grey_params(t_lw, t_sw, albedo, utc=utc)
        lat, lon = self._latlon(geom)
        ph = _lib.Physics(float(utc), t_lw, t_sw, albedo, _tab(lat), _tab(lon))
        _check(lib.gcm_set_physics(self._h, C.byref(ph)), self._h)
        self._phys = dict(t_lw=t_lw, t_sw=t_sw, albedo=albedo)

    # -- grey radiation by water vapour and CO2 (GCM_PE25D) ----------------------------------
    def set_gas_radiation(self, *off, **params):
        """while set_physics is on, every step of step() / band_run() / end_step() from now on takes its solar step from
        the grey radiation that absorbs by water vapour and CO2 (gcm_set_gas_radiation; set_ground first) instead of the
        grey scheme: a level's optical depth comes from its own q and the CO2 mixing ratio.  The clock, lat and lon are the
        physics registration's; its t_lw, t_sw and albedo are then unused.  Registering without physics is allowed and
        takes effect when physics comes on.  params: GAS_RADIATION_DEFAULTS.  set_gas_radiation(None) switches it off:
        the grey scheme again.  ValueError for a refused parameter, GcmError for a handle without a ground temperature
        (the call then changes nothing)"""
        if off:
            if off != (None,) or params:
                raise ValueError("set_gas_radiation takes keyword parameters, or None alone to switch the phase off")
            _check(lib.gcm_set_gas_radiation(self._h, None), self._h)
            self._gas = None
            return
        par = gas_radiation_params(params)
        rec = _gas_record(par)
        _check(lib.gcm_set_gas_radiation(self._h, C.byref(rec)), self._h)
        self._gas = par

    @property
    def gas_radiation_params(self):
        """the registered gas radiation's parameters as a dict in the order of GAS_RADIATION_DEFAULTS, or None where the
        handle carries none -- and also None for one registered through the C call directly"""
        gas = getattr(self, "_gas", None)
        return dict(gas) if self.gas_radiation_registered and gas else None

    @property
    def gas_radiation_registered(self):
        """whether the handle carries the phase at all (gcm_gas_radiation_on), whoever registered it"""
        return bool(_count(lib.gcm_gas_radiation_on(self._h), self._h))

    def gas_radiation(self, geom, utc, **params):
        """-> (dt_ground [H,W], dt_air [L,H,W], olr [H,W]), grey_solar.grey_radiation with clouds off on the current state
        (gcm_gas_radiation).  ValueError for a refused parameter (the call then changes nothing)"""
        par = gas_radiation_params(params, utc=utc)
        lat, lon = self._latlon(geom)
        dg, da, olr = np.empty((self.H, self.W)), np.empty((self.L, self.H, self.W)), np.empty((self.H, self.W))
        rec = _gas_record(par)
        _check(lib.gcm_gas_radiation(self._h, float(utc), C.byref(rec), _tab(lat), _tab(lon), _tab(dg), _tab(da), _tab(olr)), self._h)
        return dg, da, olr

    def gas_radiation_step(self, geom, dt, utc, **params):
        """no_limits_2_5d.solar_timestep's statements with grey_radiation's tendencies, once in place
        (gcm_gas_radiation_step); a band: own rows and ghost rows.  ValueError for a refused parameter"""
        par = gas_radiation_params(params, utc=utc, dt=dt)
        lat, lon = self._latlon(geom)
        rec = _gas_record(par)
        _check(lib.gcm_gas_radiation_step(self._h, float(dt), float(utc), C.byref(rec), _tab(lat), _tab(lon)), self._h)

    # -- Held-Suarez forcing (GCM_PE25D) ---------------------------------------------------
    def _hs_lat(self, geom):
        lat = getattr(geom, "lat", geom)        # a geometry, or the latitudes themselves
        return as_f64(np.asarray(lat, dtype=np.float64).reshape(-1), (self.global_height,), "lat")

    def set_held_suarez(self, geom, **params):
        """every step of step() / band_run() from now on ends with the Held & Suarez (1994) forcing on the device:
        Newtonian relaxation of theta towards the prescribed equilibrium and Rayleigh friction of the winds below
        sigma_b, backward Euler (gcm_set_held_suarez) -- the Matsuno step, then solar_timestep where set_physics is on,
        then this.  half_step never applies it.  geom: the geometry (its .lat, radians, over the global height) or the
        latitudes themselves; params: k_f, k_a, k_s (1 / s), sigma_b, dT_y, dtheta_z, T_0, T_min (K), Held-Suarez's
        values by default (HELD_SUAREZ_DEFAULTS).  geom=None switches the forcing off.  ValueError for a refused
        parameter (the call then changes nothing)"""
        if geom is None:
            _check(lib.gcm_set_held_suarez(self._h, None), self._h)
            self._held_suarez = None
            return
        rec, lat, par = _held_suarez_record(self._hs_lat(geom), params)
        _check(lib.gcm_set_held_suarez(self._h, C.byref(rec)), self._h)
        self._held_suarez = (dict(par), lat.copy())

    def held_suarez_step(self, geom, dt, **params):
        """the Held-Suarez forcing once, in place on the current state, with the step dt (gcm_held_suarez_step): what
        solar_step is to set_physics.  A band: own rows and ghost rows, the ghost rows must be current"""
        rec, _, _ = _held_suarez_record(self._hs_lat(geom), params)
        _check(lib.gcm_held_suarez_step(self._h, float(dt), C.byref(rec)), self._h)

    @property
    def held_suarez(self):
        """the parameters of the registered Held-Suarez forcing as a dict, or None where the handle carries none
        (gcm_held_suarez_on) -- and also None for one registered through the C call directly"""
        on = _count(lib.gcm_held_suarez_on(self._h), self._h)
        return dict(self._held_suarez[0]) if on and self._held_suarez else None

    @property
    def held_suarez_lat(self):
        """the latitudes (global_height,) the registered Held-Suarez forcing was given, or None"""
        return self._held_suarez[1].copy() if self.held_suarez is not None else None

    # -- horizontal diffusion (GCM_PE25D; a latitude band: Core(..., band_horizontal_diffusion=True)) ----
    @property
    def band_horizontal_diffusion(self):
        """True: a GCM_PE25D latitude band that takes the horizontal diffusion over its own rows and one more exchange
        per step behind it (gcm_band_hdiff); False: not a GCM_PE25D band, or one that has not opted in"""
        return bool(_count(lib.gcm_band_hdiff(self._h), self._h))

    def set_horizontal_diffusion(self, *off, **params):
        """every step of step() / end_step() from now on applies a del-2 (order=1) or del-4 (order=2) horizontal diffusion
        of the selected fields on the device (gcm_set_hdiff), once per step, directly behind the Matsuno step and ahead
        of solar_timestep, on sigma surfaces, level by level, u and v component-wise.  half_step never applies it.
        params: order, fields (a string of the letters u v t q, or the mask), nu (m^2/s at order 1, m^4/s at order 2),
        cmax (the cap of the diffusion numbers, in (0, 1/8]); HDIFF_DEFAULTS.  set_horizontal_diffusion(None) switches
        the phase off.  ValueError for an unknown keyword or a refused value, GcmError for a latitude band that has not
        opted in and for a grid with W or H below 4 (the call then changes nothing).
        A latitude band takes the phase over its own rows where it was created with band_horizontal_diffusion=True:
        band_run then exchanges the edge rows once more per step behind it (one more message of halo_bytes() per
        neighbour), a host-driven step goes end_step_diffuse, exchange, end_step_begin"""
        if off:
            if off != (None,) or params:
                raise ValueError("set_horizontal_diffusion takes keyword parameters, or None alone to switch the phase off")
            _check(lib.gcm_set_hdiff(self._h, None), self._h)
            self._hdiff = None
            return
        rec, par = _hdiff_record(params)
        _check(lib.gcm_set_hdiff(self._h, C.byref(rec)), self._h)
        self._hdiff = dict(par)

    def horizontal_diffusion_step(self, dt, **params):
        """the horizontal diffusion once, in place on the current state, with the step dt (gcm_hdiff_step), without a
        registration: what held_suarez_step is to set_held_suarez.  A band that has opted in
        (band_horizontal_diffusion=True): its own rows, from current ghost rows; the ghost rows of the selected fields
        are stale behind the call until the caller's next exchange"""
        rec, _ = _hdiff_record(params)
        _check(lib.gcm_hdiff_step(self._h, float(dt), C.byref(rec)), self._h)

    @property
    def horizontal_diffusion(self):
        """the parameters of the registered horizontal diffusion as a dict (order, fields as the mask, nu, cmax), or
        None where the handle carries none (gcm_hdiff_on) -- and also None for one registered through the C call directly"""
        on = _count(lib.gcm_hdiff_on(self._h), self._h)
        return dict(self._hdiff) if on and self._hdiff else None

    @property
    def horizontal_diffusion_registered(self):
        """whether the handle carries the phase at all (gcm_hdiff_on), whoever registered it"""
        return bool(_count(lib.gcm_hdiff_on(self._h), self._h))

    def horizontal_diffusion_plan(self):
        """the launch geometry of the horizontal diffusion of this handle, without launching (gcm_hdiff_plan), at the
        registered order and fields, else at order 2 and "uvt": tile_rows, tile_cols, tiles_i, tiles_j, grid_z (selected
        fields x levels), lds_bytes, launches (kernel launches per application)"""
        out = (C.c_int * _lib.HDIFF_PLAN_WORDS)()
        _check(lib.gcm_hdiff_plan(self._h, out, _lib.HDIFF_PLAN_WORDS), self._h)
        return dict(zip(("tile_rows", "tile_cols", "tiles_i", "tiles_j", "grid_z", "lds_bytes", "launches"), (int(x) for x in out)))

    # -- the phases with per-column sums (GCM_PE25D): one implementation for both, by their _ColumnPhase --------------
    def _set_column(self, ph, off, params):
        if off:
            if off != (None,) or params:
                raise ValueError("set_%s takes keyword parameters, or None alone to switch the phase off" % ph.name)
            _check(ph.set(self._h, None), self._h)
            self._column.pop(ph.name, None)
            return
        par = ph.params(params)
        rec = ph.record(*par.values())
        _check(ph.set(self._h, C.byref(rec)), self._h)
        self._column[ph.name] = dict(par)

    def _column_registered(self, ph):
        return bool(_count(ph.on(self._h), self._h))

    def _column_params(self, ph):
        par = self._column.get(ph.name)
        return dict(par) if self._column_registered(ph) and par else None

    def _column_step(self, ph, dt, params):
        rec = ph.record(*ph.params(params).values())
        _check(ph.step(self._h, float(dt), C.byref(rec)) if ph.step_takes_dt else ph.step(self._h, C.byref(rec)), self._h)

    def _column_sums(self, ph):
        a, b = np.empty((self.H, self.W)), np.empty((self.H, self.W))
        sec, n = C.c_double(), C.c_int64()
        _check(ph.get(self._h, _tab(a), _tab(b), C.byref(sec), C.byref(n)), self._h)
        return ph.result(int(n.value), float(sec.value), a, b)

    def _put_column(self, ph, nsteps, seconds, a, b):
        a, b = (as_f64(x, (self.H, self.W), name) for x, name in zip((a, b), ph.fields))
        _check(ph.put(self._h, _tab(a), _tab(b), float(seconds), int(nsteps)), self._h)

    def _column_reset(self, ph):
        _check(ph.reset(self._h), self._h)

    # -- surface fluxes and boundary-layer mixing (GCM_PE25D; a latitude band: Core(..., band_boundary_layer=True)) ----
    @property
    def band_boundary_layer(self):
        """whether this is a band that takes the boundary layer over its own rows, with a third exchange per step
        (gcm_band_boundary_layer); False: not a GCM_PE25D band, or one that has not opted in"""
        return bool(_count(lib.gcm_band_boundary_layer(self._h), self._h))

    def set_boundary_layer(self, *off, **params):
        """every step of step() / end_step() from now on exchanges momentum, heat and moisture with the surface and mixes
        them upwards on the device (gcm_set_boundary_layer): bulk fluxes against the ground temperature (set_ground first:
        a prescribed sea-surface temperature, e.g. aquaplanet_sst; it is never changed) and an implicit diffusion of u, v,
        theta and q in the column -- behind the Held-Suarez forcing and ahead of the convective adjustment and the moist
        physics, whose tau_e should then be 0.  half_step never applies it.  params: cd0, cd1, v_cap, ch, ce, p_pbl,
        p_strat (BOUNDARY_LAYER_DEFAULTS).  The sensible heat and the water the surface gave are accumulated per column
        (boundary_layer_sums); registering again resets the sums.  set_boundary_layer(None) switches the phase off.
        A latitude band takes the phase over its own rows where it was created with band_boundary_layer=True: band_run
        then exchanges the edge rows a third time per step, a host-driven step goes end_step_begin, exchange,
        end_step_finish (bands.merge_boundary_layer puts the bands' sums together).
        ValueError for a refused parameter, GcmError for a latitude band that has not opted in and for a handle without a
        ground temperature (the call then changes nothing)"""
        self._set_column(_BOUNDARY, off, params)

    @property
    def boundary_layer(self):
        """the parameters of the registered boundary layer as a dict, or None where the handle carries none
        (gcm_boundary_layer_on) -- and also None for one registered through the C call directly"""
        return self._column_params(_BOUNDARY)

    @property
    def boundary_layer_registered(self):
        """whether the handle carries the phase at all (gcm_boundary_layer_on), whoever registered it"""
        return self._column_registered(_BOUNDARY)

    def boundary_layer_step(self, dt, **params):
        """the boundary layer once, in place on the current state, with the step dt (gcm_boundary_layer_step).  With a
        registration the call adds to its sums, without one the sums of the call are dropped.  A band
        (band_boundary_layer=True): its own rows, from current ghost rows; the ghost rows of u, v, theta and q are stale
        behind the call until the next exchange of the current state"""
        self._column_step(_BOUNDARY, dt, params)

    def boundary_layer_sums(self):
        """-> BoundaryLayer(nsteps, seconds, shf (H, W), evap (H, W)): the float64 sums as the device holds them
        (gcm_get_boundary_layer); one synchronisation.  GcmError where no boundary layer is registered"""
        return self._column_sums(_BOUNDARY)

    def put_boundary_layer(self, nsteps, seconds, shf, evap):
        """upload sums taken by boundary_layer_sums() (gcm_put_boundary_layer): a restart goes on where the run stopped"""
        self._put_column(_BOUNDARY, nsteps, seconds, shf, evap)

    def boundary_layer_reset(self):
        """zero the sums, the seconds and the count (gcm_boundary_layer_reset)"""
        self._column_reset(_BOUNDARY)

    # -- slab mixed-layer ocean (GCM_PE25D) --------------------------------------------------
    def _slab_field(self, a, name):
        return None if a is None else as_f64(np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (self.H, self.W))),
                                             (self.H, self.W), name)

    def set_slab_ocean(self, *off, heat_capacity=1.0e7, Lv=2.5e6, capacity=None, qflux=None):
        """every step of step() / band_run() / end_step() from now on advances the ground temperature as a slab mixed-layer
        ocean on the device (gcm_set_slab_ocean; set_ground first), directly behind the boundary layer: the slab of heat
        capacity heat_capacity (J m^-2 K^-1; inf: a prescribed temperature) gains the net radiation at the surface, pays
        for the sensible heat and the evaporation the boundary layer takes from it (Lv, J / kg) and receives the ocean heat
        flux qflux (W / m^2).  capacity, qflux: fields (H, W) or None.  While it is registered the solar step leaves the
        ground temperature to it and records the surface and top-of-atmosphere fluxes (slab_ocean_fluxes, slab_ocean_sums);
        registering again resets the sums.  set_slab_ocean(None) switches the phase off, and the solar step advances the
        ground temperature by the reference's rule again.  The scheme is explicit: keep dt (4 sigma T^3 + bulk
        coefficients) / heat_capacity << 1.  ValueError for a refused parameter, GcmError for a handle without a ground
        temperature (the call then changes nothing)"""
        if off:
            if off != (None,):
                raise ValueError("set_slab_ocean takes keyword parameters, or None alone to switch the phase off")
            _check(lib.gcm_set_slab_ocean(self._h, None, None, None), self._h)
            self._slab = None
            return
        par = slab_ocean_params(dict(heat_capacity=heat_capacity, Lv=Lv))
        cap, qf = self._slab_field(capacity, "capacity"), self._slab_field(qflux, "qflux")
        rec = _lib.SlabOcean(*par.values())
        _check(lib.gcm_set_slab_ocean(self._h, C.byref(rec), None if cap is None else _tab(cap), None if qf is None else _tab(qf)),
               self._h)
        self._slab = dict(par, capacity=None if cap is None else cap.copy(), qflux=None if qf is None else qf.copy())

    @property
    def slab_ocean(self):
        """the registered slab ocean as a dict (heat_capacity, Lv, capacity, qflux: the fields or None), or None where the
        handle carries none (gcm_slab_ocean_on) -- and also None for one registered through the C call directly"""
        slab = getattr(self, "_slab", None)
        return dict(slab) if self.slab_ocean_registered and slab else None

    @property
    def slab_ocean_registered(self):
        """whether the handle carries the phase at all (gcm_slab_ocean_on), whoever registered it"""
        return bool(_count(lib.gcm_slab_ocean_on(self._h), self._h))

    def slab_ocean_apply(self, dt, words, heat_capacity=1.0e7, Lv=2.5e6):
        """the slab's cell rule once on the own rows, in place on the ground temperature, with the step dt and the flux
        words `words` (7, H, W) in the order of SLAB_OCEAN_WORDS (gcm_slab_ocean_apply); the registered capacity and
        heat-flux fields apply.  With a registration the call adds to its sums, without one nothing is summed"""
        w = as_f64(words, (_lib.SLAB_WORDS, self.H, self.W), "words")
        rec = _lib.SlabOcean(*slab_ocean_params(dict(heat_capacity=heat_capacity, Lv=Lv)).values())
        _check(lib.gcm_slab_ocean_apply(self._h, float(dt), C.byref(rec), _tab(w)), self._h)

    def slab_ocean_fluxes(self):
        """-> the flux words of the last step (or slab_ocean_apply), (7, H, W) float64 in the order of SLAB_OCEAN_WORDS:
        W / m^2, SH_J in J / m^2 and EVAP_KG in kg / m^2 over the step (gcm_get_slab_ocean_fluxes); one synchronisation"""
        out = np.empty((_lib.SLAB_WORDS, self.H, self.W))
        _check(lib.gcm_get_slab_ocean_fluxes(self._h, _tab(out)), self._h)
        return out

    def _slab_reflect(self, sums=None):
        """albedo csw_top[0] of the physics registered through set_physics, 0 without.  While the gas radiation is
        registered (with physics): the field a_g (sums[SW_SFC] / (1 - a_g)) / sums[SC], the share of the insolation the
        ground sent back, and 0 where sums[SC] == 0"""
        phys = getattr(self, "_phys", None)
        gas = self.gas_radiation_params if phys else None
        if gas is not None and sums is not None:
            a_g, sc = gas["ground_albedo"], sums[0]
            with np.errstate(divide="ignore", invalid="ignore"):
                return np.where(sc == 0, 0.0, a_g * (sums[1] / (1 - a_g)) / sc)
        if not phys or getattr(self, "_sigma_levels", None) is None:
            return 0.0
        sig, dsig = self._sigma_levels
        return phys["albedo"] * float(grey_radiation_tables(dsig, sig, phys["t_lw"], phys["t_sw"])["csw_top"][0])

    def slab_ocean_sums(self):
        """-> SlabOcean(nsteps, seconds, sums (10, H, W), reflect): the float64 sums as the device holds them
        (gcm_get_slab_ocean) and the time means they give; one synchronisation.  GcmError where no slab ocean is registered"""
        sums = np.empty((_lib.SLAB_SUMS, self.H, self.W))
        sec, n = C.c_double(), C.c_int64()
        _check(lib.gcm_get_slab_ocean(self._h, _tab(sums), C.byref(sec), C.byref(n)), self._h)
        return SlabOcean(int(n.value), float(sec.value), sums, self._slab_reflect(sums))

    def put_slab_ocean(self, nsteps, seconds, sums):
        """upload sums taken by slab_ocean_sums() (gcm_put_slab_ocean): a restart goes on where the run stopped"""
        s = as_f64(sums, (_lib.SLAB_SUMS, self.H, self.W), "sums")
        _check(lib.gcm_put_slab_ocean(self._h, _tab(s), float(seconds), int(nsteps)), self._h)

    def slab_ocean_reset(self):
        """zero the sums, the seconds and the count (gcm_slab_ocean_reset)"""
        _check(lib.gcm_slab_ocean_reset(self._h), self._h)

    # -- convective adjustment (GCM_PE25D) -------------------------------------------------
    def set_convect(self, *off, **params):
        """every step of step() / band_run() from now on adjusts statically unstable columns on the device
        (gcm_set_convect): theta, and with mix_q also q, of every unstable stretch of a column is mixed to the neutral
        profile at constant column enthalpy and water -- behind the Held-Suarez forcing and the boundary layer and ahead of
        the moist physics.
        half_step never applies it.  params: gamma, the critical lapse rate in K / m (6.5e-3: Manabe-Strickler), or
        kappa_c = Rd gamma / g, at most one of the two, neither: the dry adjustment; mix_q (True).  How often and how
        deep each column was adjusted is accumulated (convect_sums); registering again resets the sums.
        set_convect(None) switches the phase off.  ValueError for a refused parameter (the call then changes nothing)"""
        self._set_column(_CONVECT, off, params)

    @property
    def convect(self):
        """the parameters of the registered convective adjustment as a dict (kappa_c, mix_q), or None where the handle
        carries none (gcm_convect_on) -- and also None for one registered through the C call directly"""
        return self._column_params(_CONVECT)

    @property
    def convect_registered(self):
        """whether the handle carries the phase at all (gcm_convect_on), whoever registered it"""
        return self._column_registered(_CONVECT)

    def convect_step(self, **params):
        """the convective adjustment once, in place on the current state (gcm_convect_step); no dt: the adjustment is
        instantaneous.  With a registration the call adds to its counts (and no seconds), without one the counts of the
        call are dropped.  A band: own rows and ghost rows, the ghost rows must be current (a host that drives the
        exchange itself ends its steps with end_step, which applies the registered phase and counts its seconds)"""
        self._column_step(_CONVECT, None, params)

    def convect_sums(self):
        """-> Convect(nsteps, seconds, count (H, W), levels (H, W)): the float64 sums as the device holds them
        (gcm_get_convect); one synchronisation.  GcmError where no convective adjustment is registered"""
        return self._column_sums(_CONVECT)

    def put_convect(self, nsteps, seconds, count, levels):
        """upload sums taken by convect_sums() (gcm_put_convect): a restart goes on where the run stopped"""
        self._put_column(_CONVECT, nsteps, seconds, count, levels)

    def convect_reset(self):
        """zero the sums, the seconds and the count (gcm_convect_reset)"""
        self._column_reset(_CONVECT)

    # -- moist physics (GCM_PE25D) ---------------------------------------------------------
    def set_moist(self, *off, **params):
        """every step of step() / band_run() from now on ends with the moist physics on the device: q in excess of
        saturation condenses, the latent heat warms theta, the condensate leaves the column as precipitation, and with
        tau_e > 0 the lowest level is moistened towards the relative humidity rh_s (gcm_set_moist) -- the Matsuno step,
        solar_timestep where set_physics is on, the Held-Suarez forcing, the boundary layer and the convective adjustment
        where registered,
        then this, then the climatology's sample.  half_step never applies it.  params: Lv (J / kg), tau_e (s, 0: no evaporation), rh_s
        (MOIST_DEFAULTS).  Precipitation and evaporation are accumulated per column (moist_sums); registering again
        resets the sums.  set_moist(None) switches the phase off.  ValueError for a refused parameter (the call then
        changes nothing)"""
        self._set_column(_MOIST, off, params)

    @property
    def moist(self):
        """the parameters of the registered moist physics as a dict, or None where the handle carries none
        (gcm_moist_on) -- and also None for one registered through the C call directly"""
        return self._column_params(_MOIST)

    @property
    def moist_registered(self):
        """whether the handle carries the phase at all (gcm_moist_on), whoever registered it"""
        return self._column_registered(_MOIST)

    def moist_step(self, dt, **params):
        """the moist physics once, in place on the current state, with the step dt (gcm_moist_step): what
        held_suarez_step is to set_held_suarez.  With a registration the call adds to its sums, without one the sums
        of the call are dropped.  A band: own rows and ghost rows, the ghost rows must be current (a host that drives
        the exchange itself ends its steps with end_step, which applies the registered phase)"""
        self._column_step(_MOIST, dt, params)

    def moist_sums(self):
        """-> Moist(nsteps, seconds, precip (H, W), evap (H, W)): the float64 sums as the device holds them
        (gcm_get_moist); one synchronisation.  GcmError where no moist physics is registered"""
        return self._column_sums(_MOIST)

    def put_moist(self, nsteps, seconds, precip, evap):
        """upload sums taken by moist_sums() (gcm_put_moist): a restart goes on where the run stopped"""
        self._put_column(_MOIST, nsteps, seconds, precip, evap)

    def moist_reset(self):
        """zero the sums, the seconds and the count (gcm_moist_reset)"""
        self._column_reset(_MOIST)

    # -- Betts-Miller convection (GCM_PE25D) ---------------------------------------------------
    def set_betts_miller(self, *off, **params):
        """every step of step() / band_run() from now on relaxes every deep-convecting column towards the moist adiabat
        of a parcel lifted from its lowest level and towards the relative humidity rh_bm on it, over the time tau, with
        the column's enthalpy conserved and the water taken out falling as convective precipitation
        (gcm_set_betts_miller: the simplified Betts-Miller scheme) -- behind the convective adjustment and ahead of the
        moist physics.  params: any of Lv, tau, rh_bm, nsub (BETTS_MILLER_DEFAULTS).  Precipitation and the count of
        convecting applications are accumulated per column (betts_miller_sums); registering again resets the sums.
        set_betts_miller(None) switches the phase off.  ValueError for a refused parameter (the call then changes
        nothing); GcmError where the handle's levels are not supported (L < 2, sig not decreasing, L beyond the
        kernel's LDS: _lib.BETTS_MILLER_MAX_LEVELS)"""
        self._set_column(_BETTS_MILLER, off, params)

    @property
    def betts_miller(self):
        """the parameters of the registered Betts-Miller convection as a dict, or None where the handle carries none
        (gcm_betts_miller_on) -- and also None for one registered through the C call directly"""
        return self._column_params(_BETTS_MILLER)

    @property
    def betts_miller_registered(self):
        """whether the handle carries the phase at all (gcm_betts_miller_on), whoever registered it"""
        return self._column_registered(_BETTS_MILLER)

    def betts_miller_step(self, dt, **params):
        """the Betts-Miller convection once, in place on the current state, with the step dt (gcm_betts_miller_step).
        With a registration the call adds to its sums; without one they are dropped.  A band: own rows and ghost rows"""
        self._column_step(_BETTS_MILLER, dt, params)

    def betts_miller_sums(self):
        """-> BettsMiller(nsteps, seconds, precip (H, W), count (H, W)): the float64 sums as the device holds them
        (gcm_get_betts_miller); one synchronisation.  GcmError where no Betts-Miller convection is registered"""
        return self._column_sums(_BETTS_MILLER)

    def put_betts_miller(self, nsteps, seconds, precip, count):
        """upload sums taken by betts_miller_sums() (gcm_put_betts_miller): a restart goes on where the run stopped"""
        self._put_column(_BETTS_MILLER, nsteps, seconds, precip, count)

    def betts_miller_reset(self):
        """zero the sums, the seconds and the count (gcm_betts_miller_reset)"""
        self._column_reset(_BETTS_MILLER)

    # -- the sampled diagnostics (GCM_PE25D): one implementation for the four, by their _Sampler ----------------------
    def _sampler_every(self, sm):
        return _count(sm.every(self._h), self._h)

    def _sampler_sample(self, sm):
        _check(sm.sample(self._h), self._h)

    def _sampler_reset(self, sm):
        _check(sm.reset(self._h), self._h)

    def _sampler_sums(self, sm):
        sums = [np.empty(shape) for shape in sm.shapes(self)]
        n = C.c_int64(0)
        _check(sm.get(self._h, *[_tab(a) for a in sums], C.byref(n)), self._h)
        return (int(n.value), *sums)

    def _sampler_put(self, sm, n, *sums):
        sums = [as_f64(a, shape, name) for a, shape, name in zip(sums, sm.shapes(self), sm.args)]
        _check(sm.put(self._h, *[_tab(a) for a in sums], int(n)), self._h)

    def _sampler_record(self, sm):
        return sm.record(self, *self._sampler_sums(sm))

    def _sampler_plan(self, sm):
        out = (C.c_int * len(sm.plan))()
        _check(sm.plan_of(self._h, out, len(sm.plan)), self._h)
        return dict(zip(sm.plan, (int(x) for x in out)))

    def _set_plev(self, sm, every, plev):
        if int(every) == 0:
            _check(sm.set(self._h, 0, 0, None), self._h)
            return
        if int(every) < 0:
            raise ValueError("every must be >= 0")
        P = plev_array(plev)
        _check(sm.set(self._h, int(every), P.size, _tab(P)), self._h)

    def _levels(self, sm):
        P = np.empty(_lib.PLEV_MAX)
        n = _count(getattr(lib, "gcm_%s_levels" % sm.name)(self._h, _tab(P), _lib.PLEV_MAX), self._h)
        return P[:n].copy()

    # -- zonal-mean climatology (GCM_PE25D) ------------------------------------------------
    def set_climate(self, every=1):
        """accumulate the zonal-mean climatology on the device (gcm_set_climate): from now on every `every`-th step of
        step() / band_run() ends with one launch that adds the zonal sums of the moments of `Climate` to float64 sums in
        the handle, behind the solar step and the Held-Suarez forcing.  The step counter runs across calls; half_step
        never samples.  Registering again resets the sums; every=0 unregisters.  ValueError for every < 0"""
        _check(lib.gcm_set_climate(self._h, int(every)), self._h)

    @property
    def climate_every(self):
        """the registered sampling interval in steps, 0 where none is registered (gcm_climate_every)"""
        return self._sampler_every(_CLIMATE)

    def climate_sample(self):
        """one sample of the current state now (gcm_climate_sample); the step counter is untouched.  A band: the ghost
        rows of the current state must be current, as for solar_step"""
        self._sampler_sample(_CLIMATE)

    def climate_reset(self):
        """zero the sums and the sample count (gcm_climate_reset)"""
        self._sampler_reset(_CLIMATE)

    def climate_sums(self):
        """-> (n, m3 (10, L, H), m2 (2, H)): the raw float64 sums as the device holds them (gcm_get_climate); one
        synchronisation, a few hundred KB"""
        return self._sampler_sums(_CLIMATE)

    def put_climate(self, n, m3, m2):
        """upload sums taken by climate_sums() (gcm_put_climate): a restart goes on where the run stopped"""
        self._sampler_put(_CLIMATE, n, m3, m2)

    def climate(self):
        """-> Climate: the sample count and the means, the sums divided by W n (gcm_get_climate).  GcmError where no
        climatology is registered"""
        return self._sampler_record(_CLIMATE)

    # -- pressure levels (GCM_PE25D) -------------------------------------------------------
    def plev_fields(self, plev, fill=np.nan):
        """-> (out (5, N, H, W), valid (N, H, W) bool): uc, vc, theta, T and q of the current state interpolated to the
        pressures plev (Pa, strictly decreasing), linearly in pressure, by one launch (gcm_plev_fields); `fill` where the
        pressure lies under the ground or above the top mid-level.  The call holds 8 * 5 * N * H * W bytes of device
        memory (and the mask's 4 N H W) while it runs: meant for a handful of levels now and then, not for all of them
        every step.  A band: the ghost rows of the current state must be current, as for climate_sample"""
        P = plev_array(plev)
        out = np.empty((5, P.size, self.H, self.W))
        valid = np.empty((P.size, self.H, self.W), dtype=np.int32)
        _check(lib.gcm_plev_fields(self._h, P.size, _tab(P), float(fill), _tab(out), valid.ctypes.data_as(C.POINTER(C.c_int32))),
               self._h)
        return out, valid.astype(bool)

    def set_plev_climate(self, every=1, plev=None):
        """accumulate the zonal-mean climatology on pressure levels on the device (gcm_set_plev_climate): from now on
        every `every`-th step of step() / band_run() / end_step() ends with one launch that interpolates every column to
        the pressures plev (Pa, strictly decreasing) and adds the zonal sums of the words of `PlevClimate` over the
        valid columns to float64 sums in the handle, directly behind the sigma climatology's sample.  The step counter
        is the registration's own.  Registering again resets; every=0 unregisters"""
        self._set_plev(_PLEV_CLIMATE, every, plev)

    @property
    def plev_climate_every(self):
        """the registered sampling interval in steps, 0 where none is registered (gcm_plev_climate_every)"""
        return self._sampler_every(_PLEV_CLIMATE)

    @property
    def plev_climate_levels(self):
        """the registered targets (N,) in Pa (gcm_plev_climate_levels); GcmError where none are registered"""
        return self._levels(_PLEV_CLIMATE)

    def plev_climate_plan(self):
        """the launch geometry of a sample of this handle, without launching (gcm_plev_climate_plan): grid_x (rows),
        nseg (target segments; 0 without a registration), targets (per segment), threads, lds_bytes, chunks (256-column
        chunks of a row)"""
        return self._sampler_plan(_PLEV_CLIMATE)

    def plev_climate_sample(self):
        """one sample of the current state now (gcm_plev_climate_sample); the step counter is untouched.  A band: the
        ghost rows of the current state must be current, as for climate_sample"""
        self._sampler_sample(_PLEV_CLIMATE)

    def plev_climate_reset(self):
        """zero the sums and the sample count (gcm_plev_climate_reset)"""
        self._sampler_reset(_PLEV_CLIMATE)

    def plev_climate_sums(self):
        """-> (n, s (13, N, H)): the raw float64 sums as the device holds them (gcm_get_plev_climate), word 0 the count
        of valid columns; one synchronisation"""
        return self._sampler_sums(_PLEV_CLIMATE)

    def put_plev_climate(self, n, s):
        """upload sums taken by plev_climate_sums() (gcm_put_plev_climate): a restart goes on where the run stopped"""
        self._sampler_put(_PLEV_CLIMATE, n, s)

    def plev_climate(self):
        """-> PlevClimate: the sample count, the targets, the coverage and the conditional means, the sums divided by
        the count (gcm_get_plev_climate).  GcmError where none is registered"""
        return self._sampler_record(_PLEV_CLIMATE)

    # -- geopotential height on pressure levels, time-mean maps (GCM_PE25D) ----------------
    def plev_height(self, plev, fill=np.nan):
        """-> (Z (N, H, W) in m, valid (N, H, W) bool): the geopotential height of the current state on the pressures
        plev (Pa, strictly decreasing) by one launch (gcm_plev_height): the model's own mid-level geopotential, continued
        inside the bracketing layer linearly in the Exner function; `fill` where the pressure lies under the ground or
        above the top mid-level.  The call holds 8 N H W bytes of device memory (and the mask's 4 N H W) while it runs"""
        P = plev_array(plev)
        out = np.empty((P.size, self.H, self.W))
        valid = np.empty((P.size, self.H, self.W), dtype=np.int32)
        _check(lib.gcm_plev_height(self._h, P.size, _tab(P), float(fill), _tab(out), valid.ctypes.data_as(C.POINTER(C.c_int32))),
               self._h)
        return out, valid.astype(bool)

    def set_plev_maps(self, every=1, plev=None):
        """accumulate time-mean maps on pressure levels on the device (gcm_set_plev_maps): from now on every `every`-th
        step of step() / band_run() / end_step() ends -- behind the spectra's sample -- with one launch that adds Z, T,
        uc, vc, q and the products of `PlevMaps` at the pressures plev (Pa, strictly decreasing) to float64 sums per
        (target, cell) in the handle; longitude is kept.  The sums take 8 (13 N + 2) H W bytes of device memory: meant
        for a handful of levels (500 hPa, 850 hPa ...), not for all of them.  The step counter is the registration's own.
        Registering again resets; every=0 unregisters and frees"""
        self._set_plev(_PLEV_MAPS, every, plev)

    @property
    def plev_maps_every(self):
        """the registered sampling interval in steps, 0 where none is registered (gcm_plev_maps_every)"""
        return self._sampler_every(_PLEV_MAPS)

    @property
    def plev_maps_levels(self):
        """the registered targets (N,) in Pa (gcm_plev_maps_levels); GcmError where none are registered"""
        return self._levels(_PLEV_MAPS)

    def plev_maps_plan(self):
        """the launch geometry of a sample of this handle, without launching (gcm_plev_maps_plan): chunks (256-column
        chunks of a row, grid x), rows (grid y; 0 without a registration: no work), threads, lds_bytes, targets (0
        without a registration)"""
        return self._sampler_plan(_PLEV_MAPS)

    def plev_maps_sample(self):
        """one sample of the current state now (gcm_plev_maps_sample); the step counter is untouched.  A band: the
        ghost rows of the current state must be current, as for climate_sample"""
        self._sampler_sample(_PLEV_MAPS)

    def plev_maps_reset(self):
        """zero the sums and the sample count (gcm_plev_maps_reset)"""
        self._sampler_reset(_PLEV_MAPS)

    def plev_maps_sums(self):
        """-> (n, s (13, N, H, W), s2 (2, H, W)): the raw float64 sums as the device holds them (gcm_get_plev_maps), word
        0 of s the count of valid samples; one synchronisation"""
        return self._sampler_sums(_PLEV_MAPS)

    def put_plev_maps(self, n, s, s2):
        """upload sums taken by plev_maps_sums() (gcm_put_plev_maps): a restart goes on where the run stopped"""
        self._sampler_put(_PLEV_MAPS, n, s, s2)

    def plev_maps(self):
        """-> PlevMaps: the sample count, the targets, the coverage, the conditional means and the means of p and p p
        (gcm_get_plev_maps).  GcmError where none are registered"""
        return self._sampler_record(_PLEV_MAPS)

    # -- zonal wavenumber spectra (GCM_PE25D) ----------------------------------------------
    def set_spectra(self, every=1, mmax=None):
        """accumulate the zonal wavenumber spectra on the device (gcm_set_spectra): from now on every `every`-th step of
        step() / band_run() ends -- behind the climatology's sample -- with one launch that transforms uc, vc, T and
        theta of every (level, row) along i in float64 and adds the six products of `Spectra` at the wavenumbers
        0 .. mmax to float64 sums in the handle.  mmax=None: min(W / 2, 63).  The step counter is the spectra's own and
        runs across calls; half_step never samples.  Registering again resets the sums; every=0 unregisters.
        ValueError for every < 0 and for mmax outside 0 .. W / 2"""
        _check(lib.gcm_set_spectra(self._h, int(every), -1 if mmax is None else int(mmax)), self._h)

    @property
    def spectra_every(self):
        """the registered sampling interval in steps, 0 where none is registered (gcm_spectra_every)"""
        return self._sampler_every(_SPECTRA)

    @property
    def spectra_mmax(self):
        """the highest wavenumber in the sums (gcm_spectra_mmax); GcmError where no spectra are registered"""
        return _count(lib.gcm_spectra_mmax(self._h), self._h)

    def spectra_plan(self):
        """the launch geometry of a sample of this handle, without launching (gcm_spectra_plan): grid_x (rows), nseg
        (level segments), threads, lds_bytes, passes of a transform, per_thread (wavenumbers a thread holds)"""
        return self._sampler_plan(_SPECTRA)

    def spectra_sample(self):
        """one sample of the current state now (gcm_spectra_sample); the step counter is untouched.  A band: the ghost
        rows of the current state must be current, as for climate_sample"""
        self._sampler_sample(_SPECTRA)

    def spectra_reset(self):
        """zero the sums and the sample count (gcm_spectra_reset)"""
        self._sampler_reset(_SPECTRA)

    def spectra_sums(self):
        """-> (n, s (6, L, H, M)): the raw float64 sums as the device holds them (gcm_get_spectra), M = spectra_mmax + 1;
        one synchronisation"""
        return self._sampler_sums(_SPECTRA)

    def put_spectra(self, n, s):
        """upload sums taken by spectra_sums() (gcm_put_spectra): a restart goes on where the run stopped"""
        self._sampler_put(_SPECTRA, n, s)

    def spectra(self):
        """-> Spectra: the sample count and the one-sided spectra, the sums times w_m / (W^2 n) (gcm_get_spectra).
        GcmError where no spectra are registered"""
        return self._sampler_record(_SPECTRA)

    def utc(self):
        out = C.c_double()
        _check(lib.gcm_get_utc(self._h, C.byref(out)), self._h)
        return out.value

    def time_steps(self, nsteps, dt, per_kernel=True):
        ms, kms = C.c_double(), C.c_double()
        _check(lib.gcm_time_steps(self._h, int(nsteps), float(dt), C.byref(ms),
                                  C.byref(kms) if per_kernel else None), self._h)
        return ms.value, (kms.value if per_kernel else None)

    # -- latitude-band plumbing ------------------------------------------------------
    def halo_bytes(self):
        return lib.gcm_halo_bytes(self._h)

    def halo_pack(self, side, dev_ptr, stream=None):
        _check(lib.gcm_halo_pack(self._h, side, dev_ptr, stream), self._h)

    def halo_unpack(self, side, dev_ptr, stream=None):
        _check(lib.gcm_halo_unpack(self._h, side, dev_ptr, stream), self._h)

    def halo_pack2(self, north_ptr, south_ptr, stream=None):
        _check(lib.gcm_halo_pack2(self._h, north_ptr, south_ptr, stream), self._h)

    def halo_unpack2(self, north_ptr, south_ptr, stream=None):
        _check(lib.gcm_halo_unpack2(self._h, north_ptr, south_ptr, stream), self._h)

    def set_halo_buffers(self, north_ptr, south_ptr):
        _check(lib.gcm_set_halo_buffers(self._h, north_ptr, south_ptr), self._h)

    def wait_edges(self, stream):
        _check(lib.gcm_wait_edges(self._h, stream), self._h)

    def comm_stream(self):
        """hipStream_t (int) of a handle-owned stream measured to run beside the compute stream"""
        out = C.c_void_p()
        _check(lib.gcm_comm_stream(self._h, C.byref(out)), self._h)
        return out.value

    def set_exchange(self, send_north, send_south, recv_north, recv_south, rccl=None, north=0, south=0):
        """register the ghost-row exchange the library posts itself (gcm_set_exchange).  `rccl`: a
        gcmiipy_amd.rccl.RcclP2P (its communicator and the addresses of its librccl entry points);
        None: loopback, the band is its own neighbour (device-local copies)"""
        x = _lib.Exchange()
        x.north, x.south = north, south
        x.send_north, x.send_south, x.recv_north, x.recv_south = send_north, send_south, recv_north, recv_south
        if rccl is not None:
            x.comm = rccl.comm
            x.send, x.recv, x.group_start, x.group_end = rccl.entry_points()
        _check(lib.gcm_set_exchange(self._h, C.byref(x)), self._h)

    def set_band_overlap(self, on):
        """deep-halo 2-D bands: hide the exchange behind interior rows (gcm_set_band_overlap)"""
        _check(lib.gcm_set_band_overlap(self._h, 1 if on else 0), self._h)

    def band_run(self, nsteps, dt):
        """`nsteps` full band steps, exchanges included, one library call (gcm_band_run)"""
        _check(lib.gcm_band_run(self._h, int(nsteps), float(dt)), self._h)

    def step_interior(self, dt, stream=None):
        _check(lib.gcm_step_interior(self._h, float(dt), stream), self._h)

    def step_boundary(self, dt, stream=None):
        _check(lib.gcm_step_boundary(self._h, float(dt), stream), self._h)

    def step_phase(self, phase, dt, stream=None):
        _check(lib.gcm_step_phase(self._h, int(phase), float(dt), stream), self._h)

    def close(self):
        if getattr(self, "_h", None):
            lib.gcm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_count():
    return lib.gcm_device_count()
