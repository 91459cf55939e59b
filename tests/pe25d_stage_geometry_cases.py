"""The shapes of tests/test_pe25d_stage_geometry_gpu.py, each with the launch geometry of the dynamics stage it is there
for -- TEST INFRASTRUCTURE, a plain helper module.  K1 (the looping filter kernel) chooses its workgroups per row from
the rows, the level pairs and the chip's compute units, K4 (the row-group update kernel) its rows per workgroup from the
rows and the real type; at the suite's small shapes every K1 workgroup runs its loop body once and fp64 K4 takes 3-row
workgroups, which is not what the product grids 720 x 1440 x 24 and 1440 x 2880 x 40 take.  The cases below are tall,
narrow grids that reach the product grids' paths on a chip of CUS compute units at a hundredth of their cost.  `plan` is
what gcm_pe25d_stage_geometry / Core.stage_plan() must report: tests/test_pe25d_stage_geometry_cpu.py asserts it from the
pure function at CUS, the GPU tests from the handle they are about to use.  The oracle runs of a case are made once
(refs) and shared by the tests that need them; nobody changes them."""
from collections import namedtuple

import numpy as np

import pe25d_inputs as inp

CUS = 256                       # the compute units the cases' arithmetic is worked out for (an MI355X)
DT = 1.0                        # seconds: the step of test_full_size_gpu.py from 720 rows up
TILE = 62                       # columns of a K4 column tile (kUpdCols)
PTOP = 5000.0

# K1: (maxr, mask, nin, nw, passes, workgroups per row, pairs per workgroup, pairs of the last workgroup)
# K4 per real type: (rows per workgroup, groups, rows of the last group); tiles: (column tiles, columns of the last)
Case = namedtuple("Case", "shape k1 k4_f64 k4_f32 tiles oddtop setup full what")
CASES = [
    Case((768, 30, 5), (12, 0, 12, 5, 2, 1, 3, 3), (7, 110, 5), (3, 256, 3), (1, 30), 0, dict(ptop=PTOP), True,
         "(12, none) in two passes, one workgroup loops 3 pairs, the last a single level; R = 7, last group of 5 rows"),
    Case((401, 30, 5), (12, 0, 12, 5, 2, 2, 2, 1), (7, 58, 2), (3, 134, 2), (1, 30), 0, {}, True,
         "workgroups of 2 pairs and of 1 single-level pair; R = 7 just above the rule's boundary, last group of 2"),
    Case((400, 360, 7), (12, 0, 12, 5, 3, 2, 2, 2), (3, 134, 1), (3, 134, 1), (6, 50), 0, {}, True,
         "(12, none) in three passes, 2 workgroups x 2 pairs, last pair single; R = 3 at the boundary; 6 column tiles"),
    Case((420, 30, 12), (12, 0, 12, 5, 2, 2, 3, 3), (7, 60, 7), (3, 140, 3), (1, 30), 1, {}, True,
         "2 workgroups x 3 pairs, even L; R = 7 in 60 whole groups; oddtop (the band case too)"),
    Case((768, 60, 6), (16, 0, 16, 5, 2, 1, 3, 3), (7, 110, 5), (3, 256, 3), (1, 60), 1, {}, True,
         "(16, none), 5.3 4.1, 3 pairs per workgroup; oddtop"),
    Case((420, 80, 9), (25, 0, 25, 5, 2, 2, 3, 2), (7, 60, 7), (3, 140, 3), (2, 18), 0, dict(coriolis=True), True,
         "(25, none), 5.4 4.1, workgroups of 3 and 2 pairs, the last pair single; 2 column tiles (62 + 18)"),
    Case((512, 120, 13), (12, 1440, 10, 3, 2, 2, 4, 3), (7, 74, 1), (3, 171, 2), (2, 58), 0, dict(bump=True), True,
         "(12, 1440, NIN 10, NW 3) in two passes, workgroups of 4 and 3 pairs, last single; last group of 1 row"),
    Case((768, 256, 4), (16, 4096, 16, 5, 2, 1, 2, 2), (7, 110, 5), (3, 256, 3), (5, 8), 1, {}, True,
         "(16, 4096, NW 5) in two passes, 2 pairs per workgroup; 5 tiles, the last 8 columns; oddtop"),
    Case((768, 600, 3), (16, 0, 16, 5, 3, 1, 2, 2), (7, 110, 5), (3, 256, 3), (10, 42), 0, {}, True,
         "(16, none) in three passes (5.2, 5.3, 4.1), 2 pairs, last single; 10 tiles"),
    Case((768, 1000, 3), (25, 0, 25, 5, 3, 1, 2, 2), (7, 110, 5), (3, 256, 3), (17, 8), 0, {}, True,
         "(25, none) in three passes (5.2, 5.4, 5.1); 17 tiles"),
    Case((768, 1458, 3), (12, 0, 12, 5, 4, 1, 2, 2), (7, 110, 5), (3, 256, 3), (24, 32), 0, {}, True,
         "the four-pass plan with two pairs in the loop; 24 tiles"),
    Case((768, 1440, 3), (12, 1440, 10, 3, 3, 1, 2, 2), (7, 110, 5), (3, 256, 3), (24, 14), 0, {}, True,
         "(12, 1440, NIN 10, NW 3) in three passes"),
    Case((768, 2880, 3), (16, 2880, 15, 3, 3, 1, 2, 2), (7, 110, 5), (3, 256, 3), (47, 28), 0, {}, False,
         "(16, 2880, NIN 15, NW 3) in three passes; the predictor's taps only"),
    Case((768, 4096, 3), (16, 4096, 16, 5, 3, 1, 2, 2), (7, 110, 5), (3, 256, 3), (67, 4), 0, {}, False,
         "(16, 4096, NW 5) in three passes; the predictor's taps only"),
]
DTYPES = ("f64", "f32")
BAND_CASE = (420, 30, 12)       # the loopback band of gcm_band_run
TWO_BANDS = (842, 30, 5)        # two in-process bands of 421 rows: 60 groups of 7 and the last row alone
PIT3D_CASE = (768, 30, 5)       # GCM_PE_PIT2D=0


def case_id(case):
    return "%dx%dx%d" % case.shape


def case_of(shape):
    return next(c for c in CASES if c.shape == tuple(shape))


def k4_grid(groups, tiles, nseg=1):
    """workgroups of a K4 launch: (row group, segment) pairs padded to the 8 XCDs, times the column tiles"""
    return 8 * -(-groups * nseg // 8) * tiles


def plan(case, dtype):
    """the whole dict Core.stage_plan() reports for the case on a single domain"""
    maxr, mask, nin, nw, passes, wgs, ppw, last = case.k1
    rows, groups, rows_last = case.k4_f64 if dtype == "f64" else case.k4_f32
    tiles, cols_last = case.tiles
    return dict(k1_loop=1, k1_maxr=maxr, k1_mask=mask, k1_nin=nin, k1_nw=nw, k1_passes=passes, k1_workgroups_per_row=wgs,
                k1_pairs_per_wg=ppw, k1_pairs_last_wg=last, k1_pit_rides=1, k4_rows=rows, k4_groups=groups,
                k4_rows_last_group=rows_last, k4_col_tiles=tiles, k4_cols_last_tile=cols_last, k4_nseg=1,
                k4_oddtop=case.oddtop, k4_grid=k4_grid(groups, tiles))


# ---------------------------------------------------------------- the regions a geometry bug would sit in
def last_pair_levels(L, pl):
    """the levels of the last pair of each K1 workgroup, as a mask over the levels"""
    pairs, m = (L + 1) // 2, np.zeros(L, dtype=bool)
    for first in range(0, pairs, pl["k1_pairs_per_wg"]):
        p = min(first + pl["k1_pairs_per_wg"], pairs) - 1
        m[2 * p:2 * p + 2] = True
    return m


def regions(shape, pl):
    """{name: boolean mask over (L, H, W)}: the cells of the last pair of each K1 workgroup, the rows of K4's last,
    short group, the columns of K4's last tile.  A region the case does not have -- no short group, one tile, every
    level a last pair's -- is left out"""
    H, W, L = shape
    out = {}
    lv = last_pair_levels(L, pl)
    if lv.any() and not lv.all():
        out["k1_last_pair"] = np.broadcast_to(lv[:, None, None], (L, H, W))
    if pl["k4_rows_last_group"] < pl["k4_rows"] and pl["k4_groups"] > 1:
        rows = np.arange(H) >= (pl["k4_groups"] - 1) * pl["k4_rows"]
        out["k4_last_group"] = np.broadcast_to(rows[None, :, None], (L, H, W))
    if pl["k4_col_tiles"] > 1:
        cols = np.arange(W) >= (pl["k4_col_tiles"] - 1) * TILE
        out["k4_last_tile"] = np.broadcast_to(cols[None, None, :], (L, H, W))
    return out


def region_ratio(err, mask):
    """(worst |err| in the region) / (worst |err| outside it); err and mask (L, H, W), or (H, W) with the mask's level 0"""
    if err.ndim == 2:
        mask = mask[0]
    return float(np.max(err[mask])), float(np.max(err[~mask]))


# ---------------------------------------------------------------- inputs and the oracle's side
def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def geoms(case):
    import gpu_setups as su
    H, W, L = case.shape
    return su.geoms_of(H, W, L, case.setup.get("ptop", 0.0), case.setup.get("bump", False))


def state(case, og, dtype):
    """pe25d_inputs.state at the case's own seed; f32: rounded to float32 first (what the handle holds)"""
    H, W, L = case.shape
    st = inp.state(og, H + W + L)
    return tuple(f32(x) for x in st) if dtype == "f32" else st


Ref = namedtuple("Ref", "st tap unfiltered step1 step2")
_refs = {}


def refs(case, dtype):
    """the oracle's side of a case, made once: the state, the predictor's intermediates (spu, pit, p_n, phi, pgfu), spu
    without the filter, the state after one and after two steps (None where the case holds the taps only)"""
    key = (case.shape, dtype)
    if key not in _refs:
        from oracle import dynamics as od
        _, og = geoms(case)
        cor = case.setup.get("coriolis", False)
        st = state(case, og, dtype)
        tap = {}
        star = od.half_timestep(*st, *st, DT, og, _tap=tap, coriolis=cor)
        tap = {k: tap[k] for k in ("spu", "pit", "pgfu")}
        tap["phi"] = od.compute_geopotential(st[0], st[3], og)
        tap["p_n"] = star[0]
        step1 = step2 = None
        if case.full:
            step1 = od.half_timestep(*st, *star, DT, og, coriolis=cor)
            step2 = od.matsuno_timestep(*step1, DT, og, coriolis=cor)
        _refs[key] = Ref(st, tap, od.calc_pu(st[0], st[1]), step1, step2)
    return _refs[key]


def oracle_locality(case, field, mask):
    """how uneven the reference's own sensitivity is over a region: (in / out, out / in) of the worst difference
    between the oracle from float32-rounded inputs and the oracle from the float64 inputs.  field: "spu" (the tap) or
    one of "puvtq" (the state after one step)"""
    a, b = refs(case, "f32"), refs(case, "f64")
    x, y = (a.tap["spu"], b.tap["spu"]) if field == "spu" else (a.step1["puvtq".index(field)], b.step1["puvtq".index(field)])
    inside, outside = region_ratio(np.abs(x - y), mask)
    return inside / outside, outside / inside


LOCALITY = 4.0


def locality_factors(case, field, mask):
    """the factors the device's error may be uneven by, region over rest and rest over region: LOCALITY, or twice what
    the oracle's own sensitivity shows where that is more"""
    up, down = oracle_locality(case, field, mask)
    return max(LOCALITY, 2.0 * up), max(LOCALITY, 2.0 * down)
