"""gcmiipy_amd -- MI355X-native Matsuno C-grid dynamical core for gcmiipy.

Host side is Python (as the reference is); the compute path is hand-written HIP
for gfx950 in libgcmcore.so behind the C ABI of include/gcmcore.h.  Modules named
after the reference's files expose the reference's call surface:

    gcmiipy_amd.matsuno_c_grid.matsumo_scheme(u, v, p, dx, dt) -> (u, v, p)
    gcmiipy_amd.matsumo_temp.matsumo_scheme(u, v, p, t, dx, dt) -> (u, v, p, t)
    gcmiipy_amd.dynamics.matsuno_timestep(p, u, v, t, q, dt, geom) -> (p, u, v, t, q)
    gcmiipy_amd.two_d.run_2d_with_ft(state, ft, steps) ...

Importing the package loads the library and raises ImportError if it is not
built: nothing here computes on the CPU.
"""
from . import _lib  # noqa: F401  (fails loudly when the HIP library is missing)
from .core import (BettsMiller, BoundaryLayer, Climate, Convect, Core, GcmError, Moist, PlevClimate, PlevMaps, Spectra, TracerStats, aquaplanet_sst,  # noqa: F401
                   betts_miller_columns, boundary_layer_column, boundary_layer_surface, convect_columns, convect_tracer_columns, device_count,
                   hdiff_apply, hdiff_apply_band, hdiff_tables, held_suarez_tables, moist_saturation, plev_columns, plev_height_columns,
                   SlabOcean, slab_ocean_cells, GAS_RADIATION_DEFAULTS, gas_insolation, gas_radiation_columns)



def clear_cache():
    """free the device state the per-call drop-ins keep between calls"""
    from . import matsuno_c_grid, dynamics, ensemble
    for cache in (matsuno_c_grid._cache, dynamics._cache, ensemble._cache):
        while cache:
            cache.popitem()[1].close()
    _lib.lib.gcm_ops_release_scratch()      # the operator entry points' device scratch of this thread


__all__ = ["BettsMiller", "BoundaryLayer", "Climate", "Convect", "Core", "GcmError", "Moist", "PlevClimate", "PlevMaps", "Spectra", "TracerStats", "aquaplanet_sst",
           "boundary_layer_column", "boundary_layer_surface", "convect_columns", "convect_tracer_columns", "device_count",
           "betts_miller_columns", "clear_cache", "hdiff_apply", "hdiff_apply_band", "hdiff_tables", "held_suarez_tables", "moist_saturation", "plev_columns", "plev_height_columns",
           "SlabOcean", "slab_ocean_cells", "GAS_RADIATION_DEFAULTS", "gas_insolation", "gas_radiation_columns"]
