"""The cases of the radiation tests: the smallest shapes at which each form of pe_radiation_kernel can still go wrong,
the parameter sets, the clocks, the seeded inputs and the float64 reference of every combination, computed once per
process and shared.  TEST INFRASTRUCTURE, NumPy only, no test in here."""
import functools

import numpy as np

import pe25d_radiation_ref as ref

# (H, W, L): a workgroup has 128 lanes; <T, 24> holds up to 24 levels in registers, <T, 40> up to 40, <T, 0> parks in LDS
SHAPES = [
    (2, 20, 2),        # the fewest levels the scans make sense for
    (3, 128, 9),       # one exactly full block, an equator row
    (2, 130, 5),       # a second block with two lanes
    (2, 257, 24),      # three blocks, L = LMAX of <24>
    (2, 36, 25),       # first L of <40>, 15 padded register levels
    (2, 36, 40),       # LMAX of <40>
    (2, 36, 41),       # first LDS-parked L
    (2, 20, 156),      # the largest handle
]
PTOPS = [0.0, 5000.0]              # FACT, and the forms without it
DTYPES = ["f64", "f32"]
# (t_lw, t_sw, albedo): the reference's; a plain other set; a short-wave transmissivity of exactly 1 (swfac = 0) under a
# white ground; a transparent long wave (no emission); one more
SETS = [(0.1, 0.9, 0.3), (0.5, 0.6, 0.0), (0.02, 1.0, 1.0), (1.0, 0.9, 0.3), (0.9, 0.5, 0.5)]
CLOCKS = [0.0, 4 * 3600.0, 13.5 * 3600.0, 40 * 3600.0, 30 * 86400.0 + 7 * 3600.0]
DT = 300.0
ADMIT = 1e-11                      # float64 against long double, of the level's maximum: a tenth of the fp64 bound
GENERIC_SHAPES = [(2, 130, 5), (2, 36, 25), (2, 36, 41)]
GENERIC_SETS = [SETS[1], SETS[3]]
GENERIC_CLOCKS = [CLOCKS[1], CLOCKS[3]]


def combos():
    """(set, clock) in the order a handle takes them: the set changes between consecutive calls, and every set comes
    back under the next clock, so the level tables are rebuilt and uploaded again every time"""
    return [(s, utc) for utc in CLOCKS for s in SETS]


def geoms(H, W, L, ptop):
    """the product's geometry and the oracle's (gpu_setups.geoms_of without the device imports)"""
    from gcmiipy_amd import geometry
    from oracle import geometry as ogeo
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    og = ogeo.gen_geometry(H, W, L, sig_func=ogeo.manabe_sig)
    geom.ptop = og.ptop = ptop
    return geom, og


def seed_of(shape, ptop):
    H, W, L = shape
    return 7 * H * W + 3 * L + (1 if ptop else 0)


def inputs(shape, ptop, dtype, og):
    """(p, u, v, t, q), gt: the state recipe of test_pe25d_variants_gpu._state / _radiation (p about 1e5 - ptop, T about
    300 K, the ground between 270 and 300 K); f32: the state rounded to float32, what the handle holds.  The ground
    temperature is float64 on either handle"""
    from oracle import temperature as otemp
    H, W, L = shape
    rng = np.random.default_rng(seed_of(shape, ptop))
    p = 1e5 - og.ptop + 10 * rng.standard_normal((H, W))
    u = rng.standard_normal((L, H, W))
    v = rng.standard_normal((L, H, W))
    v[:, -1, :] = 0
    t = otemp.to_potential_temp(300 + rng.standard_normal((L, H, W)), p * og.sig + og.ptop)
    q = 3e-6 * (1 + 0.1 * rng.random((L, H, W)))
    gt = 270 + 30 * rng.random((H, W))
    st = (p, u, v, t, q)
    if dtype == "f32":
        st = tuple(np.asarray(x, dtype=np.float32).astype(np.float64) for x in st)
    return st, gt


@functools.lru_cache(maxsize=None)
def case(shape, ptop, dtype):
    """geom, og, st, gt of a case (read-only arrays)"""
    geom, og = geoms(*shape, ptop)
    st, gt = inputs(shape, ptop, dtype, og)
    for a in st + (gt,):
        a.setflags(write=False)
    return geom, og, st, gt


@functools.lru_cache(maxsize=2 * len(SETS) * len(CLOCKS))      # (two cases' worth: a case is judged by one test)
def reference(shape, ptop, dtype, pset, utc):
    """the float64 restatement of one combination -> (rec, theta_n, gt_n, bounds): computed once, read-only"""
    _, og, st, gt = case(shape, ptop, dtype)
    rec = ref.radiation(st[0], st[3], gt, og, utc, *pset)
    theta_n, gt_n = ref.advance(st[0], st[3], gt, rec, DT)
    bnds = ref.bounds(rec, theta_n, gt_n, DT, dtype == "f32")
    for a in tuple(rec) + (theta_n, gt_n) + tuple(bnds):
        a.setflags(write=False)
    return rec, theta_n, gt_n, bnds


def dark_mask(rec, pset):
    """the columns whose dTdt is exactly 0 by construction: the dark ones under a transparent long wave"""
    return (rec.sza == 0) if pset[0] == 1.0 else None


def sensitivity(shape, ptop, dtype, pset, utc):
    """the float64 restatement against the long-double one, of the level's maximum of |dTdt| (the admission figure)"""
    _, og, st, gt = case(shape, ptop, dtype)
    rec = reference(shape, ptop, dtype, pset, utc)[0]
    hi = ref.radiation(st[0], st[3], gt, og, utc, *pset, real=np.longdouble)
    scale = np.max(np.abs(hi.dTdt), axis=(1, 2), keepdims=True)
    return float(np.max(np.abs(rec.dTdt - hi.dTdt) / scale))
