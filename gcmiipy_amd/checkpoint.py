"""State I/O: the reference keeps its state in RAM only; long device-resident
runs want a restart file.  One `.npz` per handle holds the prognostic tuple, the ground
temperature of the column physics (when set), the model tag, every option the handle was created
with (dx, tracer, kernel variant, filter, Coriolis, dtype, band placement, ensemble members: an ensemble's
state arrays are (M, H, W), and files without "opt_members" restore as one member), the passive tracers of a GCM_PE25D
handle (key "tracers", only when it carries some; a band also stores its declared "band_tracers", files without it
restore with 0, and its ghost-row depth "band_tracer_rows", files without it restore as 1, and whether it takes the
boundary layer over its own rows, the option "band_boundary_layer", taken from the handle as it is when saved, files
without it restore as off and restore() opts in ahead of the registration; the tracers' transport scheme
is the option "tracer_scheme", files without it restore as centred; the tracers' forcing, Core.set_tracer_forcing, is
stored per forced tracer i as "forcing_<i>_scalars" (source, decay, pin_value) with "forcing_<i>_emission" and
"forcing_<i>_pin_mask" where registered, and files without these keys restore with none; their vertical mixing,
Core.set_tracer_mixing, is stored per mixed tracer i as "mixing_<i>", the float64 profile K of L - 1 values, and files
without the key restore with none; their convective mixing, Core.set_tracer_convection, is stored as "tracer_convect",
the indices of the tracers that have opted in, only when there are some, and files without the key restore with none
opted in; the Held-Suarez forcing, Core.set_held_suarez, is stored as "held_suarez", its eight
parameters in the order of core.HELD_SUAREZ_DEFAULTS, with "held_suarez_lat", the latitudes it was given, and
re-registered on restore; files without the key restore with none; the zonal-mean climatology, Core.set_climate, is
stored as "climate_every", "climate_n", "climate_m3" and "climate_m2", the interval, the sample count and the raw
float64 sums, registered and uploaded again on restore; files without these keys restore without a climatology; the
zonal wavenumber spectra, Core.set_spectra, are stored as "spectra_every", "spectra_mmax", "spectra_n" and "spectra_s",
saved and restored the same way, and files without these keys restore with none; the climatology on pressure levels,
Core.set_plev_climate, is stored as "plev_climate_every", "plev_climate_plev", "plev_climate_n" and "plev_climate_sums",
the interval, the targets in Pa, the sample count and the raw float64 sums, saved and restored the same way, and files
without these keys restore with none; the time-mean maps on pressure levels, Core.set_plev_maps, are stored as
"plev_maps_every", "plev_maps_plev", "plev_maps_n", "plev_maps_sums" and "plev_maps_sums2", the interval, the targets in
Pa, the sample count and the raw float64 sums, written only with a registration, saved and restored the same way, and
files without these keys restore with none; the horizontal diffusion,
Core.set_horizontal_diffusion, is stored as "hdiff" = [order, fields, nu, cmax] and registered again on restore, ahead of
the first step, and files without the key restore with none; whether a band takes that phase over its own rows is
the option "band_horizontal_diffusion", taken from the handle as it is when saved, files without it restore as off and
restore() opts in ahead of the registration; the
moist physics, Core.set_moist, is stored as "moist", its three parameters in the order of core.MOIST_DEFAULTS, with
"moist_n", "moist_seconds", "moist_precip" and "moist_evap", the count, the seconds and the raw float64 sums, registered
and uploaded again on restore; files without these keys restore with none; the convective adjustment, Core.set_convect,
is stored as "convect", its two parameters in the order of core.CONVECT_DEFAULTS, with "convect_n", "convect_seconds",
"convect_count" and "convect_levels", saved and restored the same way; the boundary layer, Core.set_boundary_layer, is
stored as "boundary_layer", its seven parameters in the order of core.BOUNDARY_LAYER_DEFAULTS, with "boundary_layer_n",
"boundary_layer_seconds", "boundary_layer_shf" and "boundary_layer_evap", saved the same way and restored ahead of the
convective adjustment, in the model's order (behind the ground temperature, which its registration needs); the
Betts-Miller convection, Core.set_betts_miller, is stored as "betts_miller", its four parameters in the order of
core.BETTS_MILLER_DEFAULTS, with "betts_miller_n", "betts_miller_seconds", "betts_miller_precip" and "betts_miller_count",
saved the same way and restored between the convective adjustment and the moist physics; files without these keys
restore with none; the slab ocean, Core.set_slab_ocean, is stored as "slab_ocean", its two parameters in the order of
core.SLAB_OCEAN_DEFAULTS, with "slab_ocean_n", "slab_ocean_seconds", "slab_ocean_sums", the raw float64 sums, and, where
registered, the fields "slab_ocean_capacity" and "slab_ocean_qflux", registered and uploaded again directly behind the
boundary layer; files without the key restore with none; the gas radiation, Core.set_gas_radiation, is stored as
"gas_radiation", its parameters in the order of core.GAS_RADIATION_DEFAULTS with the insolation as its GCM_INSOLATION_*
code, and registered again behind the ground temperature -- as the other column physics it acts while set_physics is
on, which the caller registers again with the saved clock; files without the key restore with none)
and the geometry tables:
`restore()` rebuilds an equivalent handle and the run resumes bit for bit.  A latitude band writes
ITS rows (one file per rank; `row0` / `global_height` are in the file)."""
import numpy as np

from . import _lib
from .core import Core, GAS_RADIATION_DEFAULTS, GcmError, HDIFF_DEFAULTS, HELD_SUAREZ_DEFAULTS, SAMPLERS, SLAB_OCEAN_DEFAULTS, STEP_COLUMN_PHASES
from .geometry import Geom

_GEOM_KEYS = ("sige", "sigt", "sigb", "dsig", "sig", "dsigv", "dx_j", "dx_h", "dy", "ptop",
              "heightmap", "area", "lat", "long")
_MODEL_NAMES = {_lib.SW2D: "SW2D", _lib.SW2D_TEMP: "SW2D_TEMP", _lib.PE2D: "PE2D", _lib.PE25D: "PE25D"}


def save(path, core, step=0, time=0.0, geom=None, **extra):
    """write the core's current state (gathered from HBM) to `path` (.npz)"""
    p, u, v, t, q = core.get_state()
    out = {"model": _MODEL_NAMES[core.model], "step": step, "time": time,
           "shape": np.asarray([core.L, core.H, core.W])}
    for name, val in core.options.items():
        out["opt_" + name] = np.asarray(val)
    if "band_boundary_layer" in core.options:    # (what the handle says now: the opt-in may have been changed since)
        out["opt_band_boundary_layer"] = np.asarray(bool(core.band_boundary_layer))
    if "band_horizontal_diffusion" in core.options:    # (the same for the diffusion's opt-in, stored beside "hdiff")
        out["opt_band_horizontal_diffusion"] = np.asarray(bool(core.band_horizontal_diffusion))
    if core.has_ground:
        out["ground"] = core.get_ground()
    if core.tracer_count > 0:
        out["tracers"] = core.get_tracers()
        for i, rec in core.tracer_forcings().items():
            out["forcing_%d_scalars" % i] = np.asarray([rec["source"], rec["decay"], rec["pin_value"]])
            if rec["emission"] is not None:
                out["forcing_%d_emission" % i] = rec["emission"]
            if rec["pin_mask"] is not None:
                out["forcing_%d_pin_mask" % i] = np.asarray(rec["pin_mask"], dtype=np.uint8)
        for i, k in core.tracer_mixings().items():
            out["mixing_%d" % i] = np.asarray(k, dtype=np.float64)
        opted = getattr(core, "tracer_convections", list)()     # (getattr: a stand-in without the convective mixing will do)
        if opted:
            out["tracer_convect"] = np.asarray(opted, dtype=np.int64)
    hs = core.held_suarez if core.model == _lib.PE25D else None
    if hs is not None:
        out["held_suarez"] = np.asarray([hs[k] for k in HELD_SUAREZ_DEFAULTS], dtype=np.float64)
        out["held_suarez_lat"] = core.held_suarez_lat
    # (the sampled diagnostics by their core._Sampler; getattr: a stand-in without one of them will do)
    for sm in SAMPLERS if core.model == _lib.PE25D else ():
        every = getattr(core, sm.name + "_every", 0)
        if every > 0:
            n, *sums = getattr(core, sm.name + "_sums")()
            out[sm.name + "_every"], out[sm.name + "_n"] = np.int64(every), np.int64(n)
            if sm.extra:                         # (the targets, mmax)
                out["%s_%s" % (sm.name, sm.extra[0])] = np.asarray(getattr(core, sm.extra[1]))
            out.update({"%s_%s" % (sm.name, k): x for k, x in zip(sm.keys, sums)})
    hd = getattr(core, "horizontal_diffusion", None) if core.model == _lib.PE25D else None   # (getattr: as above)
    if hd is not None:
        out["hdiff"] = np.asarray([hd[k] for k in HDIFF_DEFAULTS], dtype=np.float64)
    # (a core is asked only for the phases it knows: getattr, so that a stand-in without one of them will do; reversed:
    # the files have always held the moist physics' keys ahead of the convective adjustment's; the boundary layer's follow)
    for ph in reversed(STEP_COLUMN_PHASES if core.model == _lib.PE25D else ()):
        par = getattr(core, ph.name, None)
        if par is None and getattr(core, ph.name + "_registered", False):
            raise GcmError("checkpoint.save: the handle's %s was registered through gcm_set_%s directly; its parameters are "
                           "unknown here and the phase and its sums would be lost (register with Core.set_%s)"
                           % (ph.what, ph.name, ph.name))
        if par is not None:
            sums = getattr(core, ph.name + "_sums")()
            out[ph.name] = np.asarray([par[k] for k in ph.defaults], dtype=np.float64)
            out[ph.name + "_n"], out[ph.name + "_seconds"] = np.int64(sums.nsteps), np.float64(sums.seconds)
            out.update({"%s_%s" % (ph.name, f): getattr(sums, f) for f in ph.fields})
    # (getattr: a stand-in without the slab ocean will do)
    slab = getattr(core, "slab_ocean", None) if core.model == _lib.PE25D else None
    if slab is None and getattr(core, "slab_ocean_registered", False):
        raise GcmError("checkpoint.save: the handle's slab ocean was registered through gcm_set_slab_ocean directly; its "
                       "parameters are unknown here and the phase and its sums would be lost (register with Core.set_slab_ocean)")
    if slab is not None:
        sums = core.slab_ocean_sums()
        out["slab_ocean"] = np.asarray([slab[k] for k in SLAB_OCEAN_DEFAULTS], dtype=np.float64)
        out["slab_ocean_n"], out["slab_ocean_seconds"] = np.int64(sums.nsteps), np.float64(sums.seconds)
        out["slab_ocean_sums"] = sums.sums
        for k in ("capacity", "qflux"):
            if slab[k] is not None:
                out["slab_ocean_" + k] = slab[k]
    gas = getattr(core, "gas_radiation_params", None) if core.model == _lib.PE25D else None
    if gas is None and getattr(core, "gas_radiation_registered", False):
        raise GcmError("checkpoint.save: the handle's gas radiation was registered through gcm_set_gas_radiation directly; its "
                       "parameters are unknown here and the phase would be lost (register with Core.set_gas_radiation)")
    if gas is not None:
        out["gas_radiation"] = np.asarray([_lib.INSOLATION[gas[k]] if k == "insolation" else gas[k] for k in GAS_RADIATION_DEFAULTS],
                                          dtype=np.float64)
    for k, a in zip("puvtq", (p, u, v, t, q)):
        if a is not None:
            out["state_" + k] = a
    if geom is not None:
        for k in _GEOM_KEYS:
            if hasattr(geom, k):
                out["geom_" + k] = np.asarray(getattr(geom, k))
    out.update({"extra_" + k: np.asarray(v) for k, v in extra.items()})
    np.savez(path, **out)


def load(path):
    """-> dict(model, step, time, state={p,u,v,t,q}, geom or None, extra, ground, tracers, tracer_forcing,
    tracer_mixing, tracer_convect, held_suarez, hdiff, climate, plev_climate, plev_maps, spectra, moist, convect, betts_miller, boundary_layer, band_boundary_layer,
    band_horizontal_diffusion); ground and
    tracers are
    None where the file has none, tracer_forcing
    {i: dict(...)} and tracer_mixing {i: K} are then empty, and so is tracer_convect, the list of the tracers that have
    opted in to the convective mixing (files without the key: none); held_suarez is (parameters dict, lat) or None; hdiff is
    dict(order, fields, nu, cmax) or None (files without the key: None); climate is
    dict(every, n, m3, m2) or None; plev_climate is dict(every, plev, n, sums) or None (files without the keys: None); plev_maps is dict(every, plev, n, sums, sums2) or None (files without the keys: None); spectra is dict(every, mmax, n, s) or None; moist is dict(params, n, seconds, precip, evap) or None; convect is
    dict(params, n, seconds, count, levels) or None; betts_miller is dict(params, n, seconds, precip, count) or None (files
    without the keys: None); boundary_layer is dict(params, n, seconds, shf, evap) or None;
    band_boundary_layer is whether a band takes that phase (False for files without the option), and
    band_horizontal_diffusion the same for the horizontal diffusion"""
    d = np.load(path, allow_pickle=False)
    L, H, W = (int(x) for x in d["shape"])
    state = {k: d["state_" + k] for k in "puvtq" if "state_" + k in d.files}
    geom = None
    if any(f.startswith("geom_") for f in d.files):
        geom = Geom(H, W, L)
        for k in _GEOM_KEYS:
            if "geom_" + k in d.files:
                a = d["geom_" + k]
                setattr(geom, k, float(a) if a.ndim == 0 else a)
    extra = {f[6:]: d[f] for f in d.files if f.startswith("extra_")}
    opts = {}
    for f in d.files:
        if f.startswith("opt_"):
            a = d[f]
            opts[f[4:]] = str(a) if a.dtype.kind in "US" else (bool(a) if a.dtype.kind == "b" else
                                                               (float(a) if a.dtype.kind == "f" else int(a)))
    forcing = {}
    for f in d.files:
        if f.startswith("forcing_") and f.endswith("_scalars"):
            i = int(f.split("_")[1])
            source, decay, pin_value = (float(x) for x in d[f])
            key_e, key_m = "forcing_%d_emission" % i, "forcing_%d_pin_mask" % i
            forcing[i] = dict(source=source, decay=decay, pin_value=pin_value,
                              emission=d[key_e] if key_e in d.files else None,
                              pin_mask=d[key_m] if key_m in d.files else None)
    mixing = {int(f.split("_")[1]): d[f] for f in d.files if f.startswith("mixing_")}
    hs = None
    if "held_suarez" in d.files:
        hs = (dict(zip(HELD_SUAREZ_DEFAULTS, (float(x) for x in d["held_suarez"]))), d["held_suarez_lat"])
    hd = None
    if "hdiff" in d.files:
        order, fields, nu, cmax = d["hdiff"]
        hd = dict(order=int(order), fields=int(fields), nu=float(nu), cmax=float(cmax))
    sampled = {sm.name: None for sm in SAMPLERS}
    for sm in SAMPLERS:
        if sm.name + "_every" in d.files:
            rec = dict(every=int(d[sm.name + "_every"]), n=int(d[sm.name + "_n"]), **{k: d["%s_%s" % (sm.name, k)] for k in sm.keys})
            if sm.extra:                         # (the targets as they are, mmax as an int)
                x = d["%s_%s" % (sm.name, sm.extra[0])]
                rec[sm.extra[0]] = x if x.ndim else int(x)
            sampled[sm.name] = rec
    # (the parameters in the types of the phase's defaults: mix_q and nsub are ints)
    column = {ph.name: None for ph in STEP_COLUMN_PHASES}
    for ph in STEP_COLUMN_PHASES:
        if ph.name in d.files:
            par = {k: type(v)(x) for (k, v), x in zip(ph.defaults.items(), d[ph.name])}
            column[ph.name] = dict(params=par, n=int(d[ph.name + "_n"]), seconds=float(d[ph.name + "_seconds"]),
                                   **{f: d["%s_%s" % (ph.name, f)] for f in ph.fields})
    slab = None
    if "slab_ocean" in d.files:
        slab = dict(params=dict(zip(SLAB_OCEAN_DEFAULTS, (float(x) for x in d["slab_ocean"]))), n=int(d["slab_ocean_n"]),
                    seconds=float(d["slab_ocean_seconds"]), sums=d["slab_ocean_sums"],
                    capacity=d["slab_ocean_capacity"] if "slab_ocean_capacity" in d.files else None,
                    qflux=d["slab_ocean_qflux"] if "slab_ocean_qflux" in d.files else None)
    gas = None
    if "gas_radiation" in d.files:
        names = {v: k for k, v in _lib.INSOLATION.items()}
        gas = {k: names[int(x)] if k == "insolation" else float(x) for k, x in zip(GAS_RADIATION_DEFAULTS, d["gas_radiation"])}
    return dict(model=str(d["model"]), step=int(d["step"]), time=float(d["time"]), state=state, held_suarez=hs, hdiff=hd, **sampled,
                slab_ocean=slab, gas_radiation=gas,
                geom=geom, extra=extra, shape=(L, H, W), options=opts,
                ground=d["ground"] if "ground" in d.files else None,
                tracers=d["tracers"] if "tracers" in d.files else None, tracer_forcing=forcing,
                tracer_mixing=mixing,
                tracer_convect=[int(i) for i in d["tracer_convect"]] if "tracer_convect" in d.files else [],
                band_boundary_layer=bool(opts.get("band_boundary_layer", False)),
                band_horizontal_diffusion=bool(opts.get("band_horizontal_diffusion", False)), **column)


def restore(path, **core_kwargs):
    """-> (Core with the saved state resident, checkpoint dict)"""
    ck = load(path)
    L, H, W = ck["shape"]
    model = {v: k for k, v in _MODEL_NAMES.items()}[ck["model"]]
    kw = dict(ck["options"])            # the saved handle's options; keyword arguments override them
    kw.update(core_kwargs)
    if model == _lib.SW2D_TEMP and "q" in ck["state"] and not kw.get("tracer"):
        kw["tracer"] = _lib.TRACER_VANLEER      # files written before the options were stored
    core = Core(model, W, H, L, geom=ck["geom"], **kw)
    core.set_state(**ck["state"])
    if ck["ground"] is not None:
        core.set_ground(ck["ground"])
    if ck["gas_radiation"] is not None:
        core.set_gas_radiation(**ck["gas_radiation"])
    if ck["tracers"] is not None:
        core.set_tracers(ck["tracers"])
        for i, rec in sorted(ck["tracer_forcing"].items()):
            core.set_tracer_forcing(i, **rec)
        for i, k in sorted(ck["tracer_mixing"].items()):
            core.set_tracer_mixing(i, k)
        for i in ck["tracer_convect"]:
            core.set_tracer_convection(i)
    if ck["held_suarez"] is not None:
        core.set_held_suarez(ck["held_suarez"][1], **ck["held_suarez"][0])
    if ck["hdiff"] is not None:
        core.set_horizontal_diffusion(**ck["hdiff"])
    for sm in SAMPLERS:                      # (the order a step samples)
        rec = ck[sm.name]
        if rec is not None:
            getattr(core, "set_" + sm.name)(rec["every"], *([rec[sm.extra[0]]] if sm.extra else []))
            getattr(core, "put_" + sm.name)(rec["n"], *[rec[k] for k in sm.keys])
    for ph in STEP_COLUMN_PHASES:            # (the model's order: the boundary layer, the convective adjustment, the Betts-Miller convection, the moist physics)
        rec = ck[ph.name]
        if rec is not None:
            getattr(core, "set_" + ph.name)(**rec["params"])
            getattr(core, "put_" + ph.name)(rec["n"], rec["seconds"], *[rec[f] for f in ph.fields])
        if ph.name == "boundary_layer" and ck["slab_ocean"] is not None:      # (the model's order: behind the boundary layer)
            rec = ck["slab_ocean"]
            core.set_slab_ocean(capacity=rec["capacity"], qflux=rec["qflux"], **rec["params"])
            core.put_slab_ocean(rec["n"], rec["seconds"], rec["sums"])
    return core, ck
