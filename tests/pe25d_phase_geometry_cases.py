"""The shapes of tests/test_pe25d_phase_geometry_gpu.py, each with the launch geometry it is there for -- TEST
INFRASTRUCTURE, a plain helper module.  The Held-Suarez forcing, the moist physics, the climatology's sample and the
tracers' forcing choose their grid from the rows of the launch, the row length and the chip's compute units; at the
suite's (24, 36, 9) and (6, 10, 3) every one of them marches one level per workgroup in one 256-column block and one
pass, which is not what the product grid 720 x 1440 x 24 takes.  The cases below are the smallest shapes that reach the
product grid's paths on a chip of CUS compute units.  `plan` is what gcm_pe25d_phase_geometry / Core.phase_plan must
report for the case: tests/test_pe25d_phase_geometry_cpu.py asserts it from the pure function at CUS, the GPU tests from
the handle they are about to use.  The inputs are those of tests/pe25d_inputs.py and of the phases' own restatements."""
from collections import namedtuple

import numpy as np

import pe25d_inputs as inp
import pe25d_moist_ref as moist_ref

CUS = 256                       # the compute units the cases' arithmetic is worked out for (an MI355X)
PTOPS = (0.0, 1000.0)
GHOST = 2                       # ghost rows a side of a latitude band
PRODUCT = (720, 1440, 24)       # (H, W, L) of the product grid


def segments(L, nseg):
    """[(k0, k1)] of the level segments of a launch: segment s marches [s L / nseg, (s + 1) L / nseg)"""
    return [(s * L // nseg, (s + 1) * L // nseg) for s in range(nseg)]


def batches(k0, k1, n=4):
    """the sizes of the level batches a lane takes over [k0, k1): n at a time, the last one short"""
    return [min(n, k1 - k) for k in range(k0, k1, n)]


# ---------------------------------------------------------------- Held-Suarez
# segs: the levels per segment; batches: the level batches of each segment (kHsBatch = 4)
HsCase = namedtuple("HsCase", "shape plan segs batches what")
HELD_SUAREZ = [
    HsCase((512, 40, 9), dict(grid_x=1, grid_y=512, grid_z=1, levels_min=9, levels_max=9), [9], [[4, 4, 1]],
           "512 blocks: whole columns in batches of 4, 4, 1"),
    HsCase((256, 300, 6), dict(grid_x=2, grid_y=256, grid_z=1, levels_min=6, levels_max=6), [6], [[4, 2]],
           "a second column block, 44 of its 256 lanes in use; whole columns in batches of 4, 2"),
    HsCase((200, 36, 25), dict(grid_x=1, grid_y=200, grid_z=3, levels_min=8, levels_max=9), [8, 8, 9],
           [[4, 4], [4, 4], [4, 4, 1]], "three level segments of 8, 8, 9 levels"),
]
HS_BANDS = 8                    # the (200, 36, 25) case once more on so many bands: 25 + 4 rows a launch, 18 segments
HS_BAND_PLAN = dict(grid_x=1, grid_y=29, grid_z=18, levels_min=1, levels_max=2)

# ---------------------------------------------------------------- climatology
ClCase = namedtuple("ClCase", "shape plan what")
CLIMATE = [
    ClCase((512, 70, 24), dict(grid_x=512, nseg=4, levels_min=6, levels_max=6, chunks=1), "four segments of 6 levels"),
    ClCase((700, 130, 7), dict(grid_x=700, nseg=3, levels_min=2, levels_max=3, chunks=1), "segments of 2, 2, 3 levels"),
    ClCase((2048, 10, 5), dict(grid_x=2048, nseg=1, levels_min=5, levels_max=5, chunks=1),
           "p, p p and all five levels in one workgroup"),
    ClCase((6, 1440, 3), dict(grid_x=6, nseg=3, levels_min=1, levels_max=1, chunks=2),
           "two iterations of the 3 x 256 chunk loop, the last chunk 160 of 256 lanes"),
]
CL_BAND_ROWS = 24               # rows 0 .. 23 of the (512, 70, 24) case on a band handle: one level per workgroup
CL_BAND_PLAN = dict(grid_x=24, nseg=24, levels_min=1, levels_max=1, chunks=1)

# ---------------------------------------------------------------- tracer forcing
TfCase = namedtuple("TfCase", "shape dtype plan what")
TF_PASS_VECTORS = 2048 * 256    # the 16-byte vectors one pass of the capped grid takes
TRACER_FORCING = [
    TfCase((64, 720, 24), "f64", dict(groups=2048, passes=2), "the capped grid, a second pass of 28 672 vectors"),
    TfCase((128, 720, 24), "f32", dict(groups=2048, passes=2), "the same in fp32"),
]
TF_NTR = 4


def tf_records(shape, seed=33):
    """the forcing of tracers 1, 2, 3 of TF_NTR (0 is unforced): emission + mask (a third of the cells pinned), emission
    only, a source only.  The emission is positive in every cell: in whichever cells a pass covers"""
    H, W, L = shape
    rng = np.random.default_rng(seed)
    e1, e2 = 1e-3 * (0.5 + rng.random((L, H, W))), 2e-3 * (0.5 + rng.random((L, H, W)))
    mask = rng.random((L, H, W)) < 1.0 / 3.0
    return {1: dict(emission=e1, pin_mask=mask, pin_value=0.75, decay=2.1e-6),
            2: dict(emission=e2, decay=1.0e-4),
            3: dict(source=0.25)}


def device_order(a):
    """an (L, H, W) field as the device holds it, [j][k][i], flat: the order in which the forcing's passes take it"""
    return np.ascontiguousarray(np.moveaxis(np.asarray(a), 0, 1)).reshape(-1)


# ---------------------------------------------------------------- moist physics, the launch that accumulates nothing
# A global grid of MOIST_SHAPE on MOIST_BANDS bands of 4 rows: the explicit call of a band without a registration
# launches own rows and ghost rows, 8 rows, and accumulates nothing -- the launch of a band's ghost rows.  The levels
# run from the top down (top_first), so that the level the surface moistens is the last one
MOIST_SHAPE, MOIST_BANDS = (12, 1800, 42), 3
MOIST_BAND_PLAN = dict(grid_x=8, grid_y=8, grid_z=8, levels_min=5, levels_max=6)
MOIST_GHOST_PLAN = dict(grid_x=8, grid_y=2 * GHOST, grid_z=16, levels_min=2, levels_max=3)    # the ghost rows alone
MOIST_SINGLE_PLAN = dict(grid_x=8, grid_y=12, grid_z=6, levels_min=7, levels_max=7)           # the single domain, no registration
MOIST_PAR = dict(tau_e=86400.0)
MOIST_DT = 600.0


def top_first(geom):
    """the geometry with its levels in the other order: level 0 at the top, the largest sig last.  For the column-local
    phases only (nothing here steps the dynamics)"""
    for name in ("sig", "dsig", "sigb", "sigt"):
        setattr(geom, name, np.ascontiguousarray(np.asarray(getattr(geom, name))[::-1]))
    return geom


def moist_geom(ptop=0.0):
    import gpu_setups as su
    return top_first(su.geom_of(*MOIST_SHAPE, ptop))


def moist_state(geom, dtype):
    return moist_ref.humid_state(geom, dtype)


# ---------------------------------------------------------------- states
def second_state(st):
    """another state of the same values: every field moved one column east and scaled winds (float32 values stay
    float32 values: a roll and a factor of 0.5)"""
    p, u, v, t, q = (np.roll(a, 1, axis=-1) for a in st)
    return [p, 0.5 * u, 0.5 * v, t, q]


def state(geom, dtype):
    return inp.state_of(geom, dtype)
