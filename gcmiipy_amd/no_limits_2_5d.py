"""Drop-in for the caller side of the 2.5-D path (reference no_limits_2_5d.py): initial
conditions, `full_timestep` with its STATS record, `calc_energy`, `run_model`.  The time step
and the diagnostics run on the GPU; initial conditions are host NumPy (they are evaluated once)."""
from collections import defaultdict, namedtuple

import numpy as np

from . import _lib, geometry
from .core import Core
from .dynamics import _prep, _wrap_out, core_for
from .units import scalar
from .grey_solar import solar_timestep  # noqa: F401  (no_limits_2_5d.py:66-75 lives beside full_timestep in the reference)
from .humidity import manabe_rh, saturation_vapor_pressure, rh_to_mmr, w_s_at, vmr_from_mmr, mmr_to_rh  # noqa: F401  (no_limits_2_5d.py:28: `from humidity import *`)

Rd, Rv, P0, KAPPA = 287.0, 461.0, 100000.0, 287.0 / 1004.0     # constants.py:16,78,31,28

GroundVars = namedtuple("GroundVars", ("gt", "gw", "snow", "ice"))   # no_limits_2_5d.py:143
STATS = defaultdict(list)                                            # no_limits_2_5d.py:63


def gen_initial_conditions(geom):
    """no_limits_2_5d.py:146-168 -> (p, u, v, t, q, GroundVars)."""
    full = (geom.layers, geom.height, geom.width)
    surface = (geom.height, geom.width)
    p = np.full(surface, 1) * 100000 * 1.0 - geom.ptop
    u = np.full(full, 1) * 1.0
    v = np.full(full, 1) * .0
    tt = np.full(full, 1) * 360 * 1.0
    tp = p * geom.sig + geom.ptop
    t = tt * ((P0 / tp) ** KAPPA)                                    # to_potential_temp
    q = np.maximum(np.full(full, 1) * 0.000003, rh_to_mmr(manabe_rh(geom), tp, tt))
    g = GroundVars(np.full(surface, 1) * 360 * 1.0, np.zeros(surface), np.zeros(surface), np.zeros(surface))
    return p, u, v, t, q, g


def calc_energy(p, u, v, t, q, g, geom):
    """no_limits_2_5d.py:35-60 -> (ke, ate, geo, total), by a device reduction."""
    base, _ = _prep(p, u, v, t, q, geom)
    c = core_for(geom)
    c.set_state(*base)
    return c.energy(geom.area)


def _record(c, geom, stats):
    """no_limits_2_5d.py:85-91: max/min of u and v and calc_energy, one fused device reduction"""
    r = c.stats(geom.area)
    for k in ("u_max", "u_min", "v_max", "v_min", "ke"):
        stats[k].append(r[k])


def full_timestep(p, u, v, t, q, g, dt, utc, geom, stats=STATS):
    """no_limits_2_5d.py:79-94: one Matsuno step + the STATS record; `g` passes through (the
    physics below the reference's early return never runs)."""
    base, units = _prep(p, u, v, t, q, geom)
    c = core_for(geom)
    c.set_state(*base)
    c.step(1, scalar(dt))
    _record(c, geom, stats)
    return (*_wrap_out(c.get_state(), units), g)


def run_model(height, width, layers, dt, timesteps, callback, stats=STATS, bump=None, physics=False, tracers=None,
              tracer_scheme=None, tracer_forcing=None, held_suarez=False, climate=0, spectra=0, plev_climate=None,
              plev_maps=None):
    """no_limits_2_5d.py:220-236 (and test_geography.py:6-23 with `bump=(j, i, metres)`): the
    state stays in HBM for all `timesteps`; STATS come from device reductions every step.
    physics=True: every step is followed by solar_timestep(t, p, g, dt, utc, geom) with utc = 0, dt, 2 dt, ...
    -- the lines the reference keeps below full_timestep's early return (:93-96) and run_model's clock (:222, :231);
    on the device both phases are one gcm_step (gcm_set_physics), and the returned g carries the new ground temperature.
    tracers (n, layers, height, width): passive tracers carried through every step (Core.set_tracers); their final
    values are then appended to the result.  tracer_scheme: their transport scheme, "centred" (default), "upwind" or
    "van_leer" (Core.set_tracer_scheme); q keeps the reference's update.  tracer_forcing {i: dict(source=, decay=,
    emission=, pin_mask=, pin_value=)}: tracer i's forcing, applied on the device once per step
    (Core.set_tracer_forcing).  held_suarez=True (Held & Suarez (1994)'s values) or a dict of parameters: every step
    ends with the Held-Suarez forcing on the device -- relaxation of theta, friction of the low-level winds -- behind
    the solar step where physics is on too (Core.set_held_suarez).  climate=every (> 0): every `every`-th step ends
    with a sample of the zonal-mean climatology on the device, and its record (Core.climate) is appended to the
    result (Core.set_climate).  spectra=every (> 0): every `every`-th step ends with a sample of the zonal wavenumber
    spectra on the device, at the default mmax, and their record (Core.spectra) is appended to the result behind the
    climatology's (Core.set_spectra).  plev_climate=(every, plev): every `every`-th step ends with a sample of the
    zonal-mean climatology on the pressure levels plev (Pa, strictly decreasing) on the device, and its record
    (Core.plev_climate) is appended to the result behind the spectra's (Core.set_plev_climate).  plev_maps=(every, plev):
    every `every`-th step ends with a sample of the time-mean maps -- the geopotential height Z, T, the centred winds, q
    and their products, longitude kept -- on the pressure levels plev on the device, and their record (Core.plev_maps) is
    appended to the result last (Core.set_plev_maps)."""
    if tracer_forcing and tracers is None:
        raise ValueError("tracer_forcing needs tracers")
    geom = geometry.gen_geometry(height, width, layers, sig_func=geometry.manabe_sig)
    if bump is not None:
        geom.heightmap[bump[0], bump[1]] = bump[2]
    p, u, v, t, q, g = gen_initial_conditions(geom)
    v[0, 0, 0] = 0.1
    u *= 0
    c = Core(_lib.PE25D, width, height, layers, geom=geom, tracer_scheme=tracer_scheme)
    try:
        c.set_state(p, u, v, t, q)
        if tracers is not None:
            c.set_tracers(tracers)
            for i, rec in (tracer_forcing or {}).items():
                c.set_tracer_forcing(i, **rec)
        if physics:
            c.set_ground(g.gt)
            c.set_physics(geom, 0.0)
        if held_suarez:
            c.set_held_suarez(geom, **(held_suarez if isinstance(held_suarez, dict) else {}))
        if climate:
            c.set_climate(int(climate))
        if spectra:
            c.set_spectra(int(spectra))
        if plev_climate:
            c.set_plev_climate(int(plev_climate[0]), plev_climate[1])
        if plev_maps:
            c.set_plev_maps(int(plev_maps[0]), plev_maps[1])
        for _ in range(timesteps):
            c.step(1, scalar(dt))
            _record(c, geom, stats)
            if callback:
                callback(*c.get_state())
        p, u, v, t, q = c.get_state()
        if physics:
            g = GroundVars(c.get_ground(), g.gw, g.snow, g.ice)
        if tracers is not None:
            tracers = c.get_tracers()
        clim = c.climate() if climate else None
        spec = c.spectra() if spectra else None
        plev = c.plev_climate() if plev_climate else None
        maps = c.plev_maps() if plev_maps else None
    finally:
        c.close()
    out = (p, u, v, t, q, g, geom) + ((tracers,) if tracers is not None else ())
    return out + ((clim,) if climate else ()) + ((spec,) if spectra else ()) + ((plev,) if plev_climate else ()) + ((maps,) if plev_maps else ())
