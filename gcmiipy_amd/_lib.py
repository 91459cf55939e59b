"""ctypes binding of libgcmcore.so (include/gcmcore.h).

The library is the product: if it is missing or exports fewer symbols than the
header declares, importing this module raises -- there is no NumPy fallback.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GCMCORE_LIB", os.path.join(_HERE, "lib", "libgcmcore.so"))

ABI_VERSION = 1

# enums of include/gcmcore.h
SW2D, SW2D_TEMP, PE2D, PE25D = 1, 2, 3, 4
P, U, V, T, Q = 0, 1, 2, 3, 4
TRACER_NONE, TRACER_UPWIND, TRACER_VANLEER = 0, 1, 2
VARIANT_AUTO, VARIANT_STAGED, VARIANT_FUSED = 0, 1, 2
F64, F32 = 0, 1
MAX_TRACERS = 16                     # GCM_MAX_TRACERS
TRACER_STATS_WORDS = 6               # GCM_TRACER_STATS_WORDS
CLIM_WORDS3, CLIM_WORDS2 = 10, 2     # GCM_CLIM_WORDS3, GCM_CLIM_WORDS2
PLEV_MAX, PLEV_WORDS, PLEV_PLAN_WORDS = 64, 13, 6    # GCM_PLEV_MAX, GCM_PLEV_WORDS, GCM_PLEV_PLAN_WORDS
PLEV_MAP_WORDS, PLEV_MAP_WORDS2, PLEV_MAP_PLAN_WORDS = 13, 2, 5     # GCM_PLEV_MAP_WORDS, _WORDS2, _PLAN_WORDS
SPEC_WORDS = 6                       # GCM_SPEC_WORDS
SPEC_PLAN_WORDS = 6                  # GCM_SPEC_PLAN_WORDS
HDIFF_U, HDIFF_V, HDIFF_T, HDIFF_Q = 1, 2, 4, 8     # GCM_HDIFF_*
HDIFF_PLAN_WORDS = 7                 # GCM_HDIFF_PLAN_WORDS
SW2D_PLAN_WORDS = 9                  # GCM_SW2D_PLAN_WORDS
SW2D_PAIR_WORDS = 2                  # GCM_SW2D_PAIR_WORDS
PHASE_HELD_SUAREZ, PHASE_MOIST, PHASE_CLIMATE, PHASE_TRACER_FORCING = range(4)   # gcm_pe25d_phase
PHASE_PLAN_WORDS = 5                 # GCM_PHASE_PLAN_WORDS
# GCM_STAGE_*: the words of gcm_pe25d_stage_geometry / gcm_pe25d_stage_plan in order, as Core.stage_plan() names them
STAGE_WORDS = ("k1_loop", "k1_maxr", "k1_mask", "k1_nin", "k1_nw", "k1_passes", "k1_workgroups_per_row", "k1_pairs_per_wg",
               "k1_pairs_last_wg", "k1_pit_rides", "k4_rows", "k4_groups", "k4_rows_last_group", "k4_col_tiles",
               "k4_cols_last_tile", "k4_nseg", "k4_oddtop", "k4_grid", "band", "k1_split", "k1_own_workgroups_per_row",
               "k1_own_pairs_per_wg", "k1_own_pairs_last_wg", "k4_edge_groups", "k4_edge_rows_last_group", "k4_edge_oddtop",
               "k4_edge_grid", "nseg_edge", "k4_int_groups", "k4_int_rows_last_group", "k4_int_oddtop", "k4_int_grid")
STAGE_PLAN_WORDS = 32                # GCM_STAGE_PLAN_WORDS
STAGE_BAND_WORD = 18                 # GCM_STAGE_BAND: the words from here on describe a band's split stage
ADV_UPWIND, ADV_FV_UPWIND, ADV_FV_PLAIN, ADV_VANLEER, ADV_MOMENTUM = range(5)
DIAG_ANY_NAN, DIAG_MAX_U, DIAG_MEAN_P, DIAG_SUM_P, DIAG_MIN_U, DIAG_MAX_V, DIAG_MIN_V = range(7)
DIAG_TV_P, DIAG_TV_U, DIAG_TV_V, DIAG_TV_T, DIAG_TV_Q = range(7, 12)
INT_SPU, INT_PIT, INT_PN, INT_PHI, INT_PGFU = range(5)
FL_VAN_LEER, FL_CALC_R, FL_DONOR_FLUX, FL_DONOR_ADVECTION = range(4)
OP1D_ADVEC_Q, OP1D_CALC_PU, OP1D_UN_PU, OP1D_ADVEC_P, OP1D_ADVEC_PU, OP1D_ADVEC_T, OP1D_PGF = range(7)
(PEOP_CALC_PU, PEOP_CALC_PV, PEOP_UN_PU, PEOP_UN_PV, PEOP_AFLUX, PEOP_ADVEC_SIG, PEOP_ADVEC_M_PU, PEOP_GEOPOTENTIAL,
 PEOP_PGF, PEOP_ADVEC_T) = range(10)


class PeGeom(C.Structure):
    """gcm_pe_geom"""
    _fields_ = [("dx_j", C.c_void_p), ("dx_h", C.c_void_p), ("dsig", C.c_void_p), ("sig", C.c_void_p),
                ("sigb", C.c_void_p), ("sigt", C.c_void_p), ("heightmap", C.c_void_p), ("dy", C.c_double),
                ("ptop", C.c_double)]


(OP_ADV_U, OP_ADV_V, OP_GEO_GRAD_U, OP_GEO_GRAD_V, OP_ADV_GEO, OP_LAPLACIAN, OP_VISCOSITY, OP_DENSITY_FROM,
 OP_GEOPOTENTIAL_FROM, OP_TO_TRUE_TEMP, OP_TO_POTENTIAL_TEMP, OP_TO_DENSITY, OP_SCALING, OP_UNSCALING,
 OP_PE2D_ADVEC_P, OP_PE2D_DUT, OP_PE2D_DVT, OP_PE2D_PGF_U, OP_PE2D_PGF_V) = range(19)
OK, ERR_ARG, ERR_HIP, ERR_NODEVICE, ERR_STATE, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5

_dp = C.POINTER(C.c_double)


class Config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("model", C.c_int32), ("width", C.c_int32),
        ("height", C.c_int32), ("layers", C.c_int32), ("tracer", C.c_int32),
        ("variant", C.c_int32), ("filter", C.c_int32), ("nranks", C.c_int32),
        ("rank", C.c_int32), ("global_height", C.c_int32), ("row0", C.c_int32),
        ("device", C.c_int32), ("dtype", C.c_int32), ("halo_steps", C.c_int32),
        ("members", C.c_int32),
        ("dx", C.c_double), ("dy", C.c_double), ("ptop", C.c_double),
        ("dx_j", _dp), ("dx_h", _dp), ("sig", _dp), ("dsig", _dp), ("sigb", _dp),
        ("sigt", _dp), ("heightmap", _dp), ("cor_u", _dp), ("cor_v", _dp), ("stream", C.c_void_p),
    ]


class Exchange(C.Structure):
    """gcm_exchange of include/gcmcore.h"""
    _fields_ = [("comm", C.c_void_p), ("north", C.c_int32), ("south", C.c_int32),
                ("send", C.c_void_p), ("recv", C.c_void_p), ("group_start", C.c_void_p), ("group_end", C.c_void_p),
                ("send_north", C.c_void_p), ("send_south", C.c_void_p), ("recv_north", C.c_void_p),
                ("recv_south", C.c_void_p)]


class Physics(C.Structure):
    """gcm_physics of include/gcmcore.h"""
    _fields_ = [("utc", C.c_double), ("t_lw", C.c_double), ("t_sw", C.c_double), ("albedo", C.c_double),
                ("lat", _dp), ("lon", _dp)]


class HeldSuarez(C.Structure):
    """gcm_held_suarez of include/gcmcore.h"""
    _fields_ = [("k_f", C.c_double), ("k_a", C.c_double), ("k_s", C.c_double), ("sigma_b", C.c_double),
                ("dT_y", C.c_double), ("dtheta_z", C.c_double), ("T_0", C.c_double), ("T_min", C.c_double),
                ("lat", _dp)]


class Hdiff(C.Structure):
    """gcm_hdiff of include/gcmcore.h"""
    _fields_ = [("order", C.c_int32), ("fields", C.c_int32), ("nu", C.c_double), ("cmax", C.c_double)]


class Moist(C.Structure):
    """gcm_moist of include/gcmcore.h"""
    _fields_ = [("Lv", C.c_double), ("tau_e", C.c_double), ("rh_s", C.c_double)]


class BoundaryLayer(C.Structure):
    """gcm_boundary_layer of include/gcmcore.h"""
    _fields_ = [("cd0", C.c_double), ("cd1", C.c_double), ("v_cap", C.c_double), ("ch", C.c_double), ("ce", C.c_double),
                ("p_pbl", C.c_double), ("p_strat", C.c_double)]


class SlabOcean(C.Structure):
    """gcm_slab_ocean of include/gcmcore.h"""
    _fields_ = [("heat_capacity", C.c_double), ("Lv", C.c_double)]


SLAB_WORDS, SLAB_SUMS = 7, 10                # GCM_SLAB_WORDS, GCM_SLAB_SUMS


class GasRadiation(C.Structure):
    """gcm_gas_radiation_par of include/gcmcore.h"""
    _fields_ = [("k_h2o_lw", C.c_double), ("k_co2_lw", C.c_double), ("k_h2o_sw", C.c_double), ("k_co2_sw", C.c_double),
                ("co2_vmr", C.c_double), ("ground_albedo", C.c_double), ("solar_constant", C.c_double),
                ("declination", C.c_double), ("insolation", C.c_int32)]


INSOLATION = {"uniform": 0, "zenith": 1, "daily": 2}      # GCM_INSOLATION_*


class Convect(C.Structure):
    """gcm_convect of include/gcmcore.h"""
    _fields_ = [("kappa_c", C.c_double), ("mix_q", C.c_int32)]


class BettsMiller(C.Structure):
    """gcm_betts_miller of include/gcmcore.h"""
    _fields_ = [("Lv", C.c_double), ("tau", C.c_double), ("rh_bm", C.c_double), ("nsub", C.c_int)]


BETTS_MILLER_MAX_LEVELS = 158                # GCM_BETTS_MILLER_MAX_LEVELS


class TracerForcing(C.Structure):
    """gcm_tracer_forcing of include/gcmcore.h"""
    _fields_ = [("source", C.c_double), ("decay", C.c_double), ("pin_value", C.c_double),
                ("emission", _dp), ("pin_mask", C.POINTER(C.c_ubyte))]


_H = C.c_void_p
# name -> (restype, argtypes); every symbol include/gcmcore.h declares
SYMBOLS = {
    "gcm_abi_version": (C.c_int, []),
    "gcm_device_count": (C.c_int, []),
    "gcm_build_info": (C.c_char_p, []),
    "gcm_exner_table": (C.c_int, [_dp]),
    "gcm_filter_plan": (C.c_int, [C.c_int, C.POINTER(C.c_uint), C.c_int]),
    "gcm_create": (C.c_int, [C.POINTER(Config), C.POINTER(_H)]),
    "gcm_destroy": (C.c_int, [_H]),
    "gcm_last_error": (C.c_char_p, [_H]),
    "gcm_set_state": (C.c_int, [_H] + [C.c_void_p] * 5),
    "gcm_get_state": (C.c_int, [_H] + [C.c_void_p] * 5),
    "gcm_members": (C.c_int, [_H]),
    "gcm_set_member": (C.c_int, [_H, C.c_int] + [C.c_void_p] * 5),
    "gcm_get_member": (C.c_int, [_H, C.c_int] + [C.c_void_p] * 5),
    "gcm_diag_members": (C.c_int, [_H, C.c_int, _dp, C.c_int]),
    "gcm_step": (C.c_int, [_H, C.c_int, C.c_double]),
    "gcm_sw2d_plan": (C.c_int, [_H, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "gcm_sw2d_fused_depth": (C.c_int, [_H]),
    "gcm_sw2d_pair_info": (C.c_int, [_H, C.POINTER(C.c_int), C.c_int]),
    "gcm_pe25d_phase_geometry": (C.c_int, [C.c_int] * 7 + [C.POINTER(C.c_int), C.c_int]),
    "gcm_pe25d_phase_plan": (C.c_int, [_H, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "gcm_pe25d_stage_geometry": (C.c_int, [C.c_int] * 5 + [C.POINTER(C.c_uint), C.c_int, C.POINTER(C.c_int), C.c_int]),
    "gcm_pe25d_stage_plan": (C.c_int, [_H, C.POINTER(C.c_int), C.c_int]),
    "gcm_half_step": (C.c_int, [_H, C.c_int, C.c_double]),
    "gcm_end_step": (C.c_int, [_H, C.c_double]),
    "gcm_end_step_diffuse": (C.c_int, [_H, C.c_double]),
    "gcm_end_step_begin": (C.c_int, [_H, C.c_double]),
    "gcm_end_step_finish": (C.c_int, [_H, C.c_double]),
    "gcm_get_star": (C.c_int, [_H] + [C.c_void_p] * 5),
    "gcm_set_star": (C.c_int, [_H] + [C.c_void_p] * 5),
    "gcm_diag": (C.c_int, [_H, C.c_int, _dp]),
    "gcm_energy": (C.c_int, [_H, _dp, C.c_int, _dp]),
    "gcm_stats": (C.c_int, [_H, _dp, C.c_int, _dp]),
    "gcm_flux_limiter": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p]),
    "gcm_polar_filter": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p]),
    "gcm_get_intermediate": (C.c_int, [_H, C.c_int, C.c_void_p]),
    "gcm_set_ground": (C.c_int, [_H, C.c_void_p]),
    "gcm_get_ground": (C.c_int, [_H, C.c_void_p]),
    "gcm_grey_radiation": (C.c_int, [_H] + [C.c_double] * 4 + [_dp, _dp, C.c_void_p, C.c_void_p]),
    "gcm_solar_step": (C.c_int, [_H] + [C.c_double] * 5 + [_dp, _dp]),
    "gcm_grey_radiation_tables": (C.c_int, [C.c_int, _dp, _dp, C.c_double, C.c_double, _dp, C.c_int]),
    "gcm_set_physics": (C.c_int, [_H, C.c_void_p]),
    "gcm_get_utc": (C.c_int, [_H, _dp]),
    "gcm_set_held_suarez": (C.c_int, [_H, C.POINTER(HeldSuarez)]),
    "gcm_held_suarez_on": (C.c_int, [_H]),
    "gcm_held_suarez_step": (C.c_int, [_H, C.c_double, C.POINTER(HeldSuarez)]),
    "gcm_held_suarez_tables": (C.c_int, [C.c_int, _dp, C.c_int, _dp, C.POINTER(HeldSuarez), C.c_double, _dp, _dp, _dp, _dp]),
    "gcm_set_hdiff": (C.c_int, [_H, C.POINTER(Hdiff)]),
    "gcm_hdiff_on": (C.c_int, [_H]),
    "gcm_hdiff_step": (C.c_int, [_H, C.c_double, C.POINTER(Hdiff)]),
    "gcm_hdiff_tables": (C.c_int, [C.c_int, _dp, _dp, C.c_double, C.POINTER(Hdiff), C.c_double, _dp]),
    "gcm_hdiff_apply": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp]),
    "gcm_hdiff_apply_band": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp]),
    "gcm_hdiff_plan": (C.c_int, [_H, C.POINTER(C.c_int), C.c_int]),
    "gcm_set_band_hdiff": (C.c_int, [_H, C.c_int]),
    "gcm_band_hdiff": (C.c_int, [_H]),
    "gcm_set_moist": (C.c_int, [_H, C.POINTER(Moist)]),
    "gcm_moist_on": (C.c_int, [_H]),
    "gcm_moist_step": (C.c_int, [_H, C.c_double, C.POINTER(Moist)]),
    "gcm_get_moist": (C.c_int, [_H, _dp, _dp, _dp, C.POINTER(C.c_int64)]),
    "gcm_put_moist": (C.c_int, [_H, _dp, _dp, C.c_double, C.c_int64]),
    "gcm_moist_reset": (C.c_int, [_H]),
    "gcm_moist_saturation": (C.c_int, [C.c_int, _dp, _dp, _dp, _dp, C.POINTER(C.c_int)]),
    "gcm_set_boundary_layer": (C.c_int, [_H, C.POINTER(BoundaryLayer)]),
    "gcm_set_band_boundary_layer": (C.c_int, [_H, C.c_int]),
    "gcm_band_boundary_layer": (C.c_int, [_H]),
    "gcm_boundary_layer_on": (C.c_int, [_H]),
    "gcm_boundary_layer_step": (C.c_int, [_H, C.c_double, C.POINTER(BoundaryLayer)]),
    "gcm_get_boundary_layer": (C.c_int, [_H, _dp, _dp, _dp, C.POINTER(C.c_int64)]),
    "gcm_put_boundary_layer": (C.c_int, [_H, _dp, _dp, C.c_double, C.c_int64]),
    "gcm_boundary_layer_reset": (C.c_int, [_H]),
    "gcm_boundary_layer_surface": (C.c_int, [C.c_int, C.POINTER(BoundaryLayer), C.c_double, C.c_double] + [_dp] * 8),
    "gcm_boundary_layer_column": (C.c_int, [C.c_int, C.c_int] + [_dp] * 7),
    "gcm_set_slab_ocean": (C.c_int, [_H, C.POINTER(SlabOcean), _dp, _dp]),
    "gcm_slab_ocean_on": (C.c_int, [_H]),
    "gcm_slab_ocean_apply": (C.c_int, [_H, C.c_double, C.POINTER(SlabOcean), _dp]),
    "gcm_get_slab_ocean_fluxes": (C.c_int, [_H, _dp]),
    "gcm_get_slab_ocean": (C.c_int, [_H, _dp, _dp, C.POINTER(C.c_int64)]),
    "gcm_put_slab_ocean": (C.c_int, [_H, _dp, C.c_double, C.c_int64]),
    "gcm_slab_ocean_reset": (C.c_int, [_H]),
    "gcm_slab_ocean_cells": (C.c_int, [C.c_int, C.POINTER(SlabOcean), C.c_double] + [_dp] * 6),
    "gcm_set_gas_radiation": (C.c_int, [_H, C.POINTER(GasRadiation)]),
    "gcm_gas_radiation_on": (C.c_int, [_H]),
    "gcm_gas_radiation": (C.c_int, [_H, C.c_double, C.POINTER(GasRadiation), _dp, _dp, _dp, _dp, _dp]),
    "gcm_gas_radiation_step": (C.c_int, [_H, C.c_double, C.c_double, C.POINTER(GasRadiation), _dp, _dp]),
    "gcm_gas_radiation_columns": (C.c_int, [C.c_int, C.c_int, C.POINTER(GasRadiation), _dp, _dp, C.c_double] + [_dp] * 9),
    "gcm_gas_insolation": (C.c_int, [C.c_int, C.c_int, _dp, C.c_double, C.c_double, _dp]),
    "gcm_set_convect": (C.c_int, [_H, C.POINTER(Convect)]),
    "gcm_convect_on": (C.c_int, [_H]),
    "gcm_convect_step": (C.c_int, [_H, C.POINTER(Convect)]),
    "gcm_get_convect": (C.c_int, [_H, _dp, _dp, _dp, C.POINTER(C.c_int64)]),
    "gcm_put_convect": (C.c_int, [_H, _dp, _dp, C.c_double, C.c_int64]),
    "gcm_convect_reset": (C.c_int, [_H]),
    "gcm_convect_columns": (C.c_int, [C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp, C.POINTER(C.c_int32)]),
    "gcm_set_betts_miller": (C.c_int, [_H, C.POINTER(BettsMiller)]),
    "gcm_betts_miller_on": (C.c_int, [_H]),
    "gcm_betts_miller_step": (C.c_int, [_H, C.c_double, C.POINTER(BettsMiller)]),
    "gcm_get_betts_miller": (C.c_int, [_H, _dp, _dp, _dp, C.POINTER(C.c_int64)]),
    "gcm_put_betts_miller": (C.c_int, [_H, _dp, _dp, C.c_double, C.c_int64]),
    "gcm_betts_miller_reset": (C.c_int, [_H]),
    "gcm_betts_miller_columns": (C.c_int, [C.c_int, C.c_int] + [_dp] * 5 + [C.c_double, C.c_double, C.POINTER(BettsMiller), _dp, _dp, _dp,
                                            C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp]),
    "gcm_set_climate": (C.c_int, [_H, C.c_int]),
    "gcm_climate_every": (C.c_int, [_H]),
    "gcm_climate_sample": (C.c_int, [_H]),
    "gcm_climate_reset": (C.c_int, [_H]),
    "gcm_get_climate": (C.c_int, [_H, _dp, _dp, C.POINTER(C.c_int64)]),
    "gcm_put_climate": (C.c_int, [_H, _dp, _dp, C.c_int64]),
    "gcm_plev_columns": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.POINTER(C.c_int)]),
    "gcm_plev_fields": (C.c_int, [_H, C.c_int, _dp, C.c_double, _dp, C.POINTER(C.c_int32)]),
    "gcm_set_plev_climate": (C.c_int, [_H, C.c_int, C.c_int, _dp]),
    "gcm_plev_climate_every": (C.c_int, [_H]),
    "gcm_plev_climate_levels": (C.c_int, [_H, _dp, C.c_int]),
    "gcm_plev_climate_sample": (C.c_int, [_H]),
    "gcm_plev_climate_reset": (C.c_int, [_H]),
    "gcm_get_plev_climate": (C.c_int, [_H, _dp, C.POINTER(C.c_int64)]),
    "gcm_put_plev_climate": (C.c_int, [_H, _dp, C.c_int64]),
    "gcm_plev_climate_plan": (C.c_int, [_H, C.POINTER(C.c_int), C.c_int]),
    "gcm_plev_height_columns": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, C.c_double, _dp, _dp, C.POINTER(C.c_int)]),
    "gcm_plev_height": (C.c_int, [_H, C.c_int, _dp, C.c_double, _dp, C.POINTER(C.c_int32)]),
    "gcm_set_plev_maps": (C.c_int, [_H, C.c_int, C.c_int, _dp]),
    "gcm_plev_maps_every": (C.c_int, [_H]),
    "gcm_plev_maps_levels": (C.c_int, [_H, _dp, C.c_int]),
    "gcm_plev_maps_sample": (C.c_int, [_H]),
    "gcm_plev_maps_reset": (C.c_int, [_H]),
    "gcm_get_plev_maps": (C.c_int, [_H, _dp, _dp, C.POINTER(C.c_int64)]),
    "gcm_put_plev_maps": (C.c_int, [_H, _dp, _dp, C.c_int64]),
    "gcm_plev_maps_plan": (C.c_int, [_H, C.POINTER(C.c_int), C.c_int]),
    "gcm_set_spectra": (C.c_int, [_H, C.c_int, C.c_int]),
    "gcm_spectra_every": (C.c_int, [_H]),
    "gcm_spectra_mmax": (C.c_int, [_H]),
    "gcm_spectra_plan": (C.c_int, [_H, C.POINTER(C.c_int), C.c_int]),
    "gcm_spectra_sample": (C.c_int, [_H]),
    "gcm_spectra_reset": (C.c_int, [_H]),
    "gcm_get_spectra": (C.c_int, [_H, _dp, C.POINTER(C.c_int64)]),
    "gcm_put_spectra": (C.c_int, [_H, _dp, C.c_int64]),
    "gcm_snapshot": (C.c_int, [_H]),
    "gcm_restore": (C.c_int, [_H]),
    "gcm_halo_bytes": (C.c_size_t, [_H]),
    "gcm_halo_pack": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p]),
    "gcm_halo_unpack": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p]),
    "gcm_halo_pack2": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gcm_set_halo_buffers": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "gcm_wait_edges": (C.c_int, [_H, C.c_void_p]),
    "gcm_comm_stream": (C.c_int, [_H, C.POINTER(C.c_void_p)]),
    "gcm_halo_unpack2": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gcm_step_interior": (C.c_int, [_H, C.c_double, C.c_void_p]),
    "gcm_step_boundary": (C.c_int, [_H, C.c_double, C.c_void_p]),
    "gcm_step_phase": (C.c_int, [_H, C.c_int, C.c_double, C.c_void_p]),
    "gcm_set_exchange": (C.c_int, [_H, C.POINTER(Exchange)]),
    "gcm_band_run": (C.c_int, [_H, C.c_int, C.c_double]),
    "gcm_set_band_overlap": (C.c_int, [_H, C.c_int]),
    "gcm_sync": (C.c_int, [_H]),
    "gcm_advect2d": (C.c_int, [C.c_int] * 6 + [C.c_double] * 3 + [C.c_void_p] * 3),
    "gcm_pgf2d": (C.c_int, [C.c_int] * 3 + [C.c_double] * 3 + [C.c_void_p] * 3),
    "gcm_pe1d": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_void_p * 4),
                           C.POINTER(C.c_void_p * 4), C.POINTER(C.c_void_p * 4)]),
    "gcm_sw2d_op": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p]),
    "gcm_pe25d_op": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p * 5),
                               C.POINTER(C.c_void_p * 4)]),
    "gcm_pe25d_op_last_error": (C.c_char_p, []),
    "gcm_pe1d_op": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gcm_array_stats": (C.c_int, [C.c_void_p, C.c_long, C.c_long, C.c_void_p]),
    "gcm_ops_last_error": (C.c_char_p, []),
    "gcm_ops_release_scratch": (C.c_int, []),
    "gcm_time_steps": (C.c_int, [_H, C.c_int, C.c_double, _dp, _dp]),
    "gcm_set_tracers": (C.c_int, [_H, C.c_int, C.c_void_p]),
    "gcm_get_tracers": (C.c_int, [_H, C.c_int, C.c_void_p]),
    "gcm_tracer_count": (C.c_int, [_H]),
    "gcm_tracer_stats": (C.c_int, [_H, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "gcm_set_band_tracers": (C.c_int, [_H, C.c_int]),
    "gcm_set_band_tracer_rows": (C.c_int, [_H, C.c_int]),
    "gcm_band_tracer_rows": (C.c_int, [_H]),
    "gcm_set_tracer_scheme": (C.c_int, [_H, C.c_int]),
    "gcm_tracer_scheme": (C.c_int, [_H]),
    "gcm_set_tracer_forcing": (C.c_int, [_H, C.c_int, C.POINTER(TracerForcing)]),
    "gcm_tracer_forced": (C.c_int, [_H, C.c_int]),
    "gcm_set_tracer_mixing": (C.c_int, [_H, C.c_int, _dp, C.c_int]),
    "gcm_tracer_mixed": (C.c_int, [_H, C.c_int]),
    "gcm_tracer_mixing_coeffs": (C.c_int, [C.c_int, _dp, _dp, C.c_double, _dp, _dp, _dp]),
    "gcm_set_tracer_convect": (C.c_int, [_H, C.c_int, C.c_int]),
    "gcm_tracer_convected": (C.c_int, [_H, C.c_int]),
    "gcm_convect_tracer_columns": (C.c_int, [C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_int)]),
}


def _preload_torch_hip_runtime():
    """PyTorch wheels bundle their own libamdhip64.so (SONAME libamdhip64.so.7, but requested by
    file name).  If the system runtime is loaded first and torch later, the process ends up with
    TWO HIP runtimes and torch.cuda fails with "No HIP GPUs are available".  Loading torch's copy
    first (without importing torch) makes libgcmcore.so and torch share one runtime in either
    import order.  GCMCORE_SYSTEM_HIP=1 skips this."""
    if os.environ.get("GCMCORE_SYSTEM_HIP"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
        for name in ("libhsa-runtime64.so", "libamdhip64.so"):
            path = os.path.join(libdir, name)
            if os.path.exists(path):
                C.CDLL(path, mode=C.RTLD_GLOBAL)
    except OSError:
        pass


def _load():
    _preload_torch_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "gcmiipy_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C gcmiipy_amd/csrc`; there is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise ImportError("gcmiipy_amd: %s does not export %s" % (LIB_PATH, name))
        fn.restype = res
        fn.argtypes = args
    if lib.gcm_abi_version() != ABI_VERSION:
        raise ImportError("gcmiipy_amd: ABI version mismatch")
    return lib


lib = _load()
