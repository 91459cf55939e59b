"""The slab mixed-layer ocean of GCM_PE25D on the device (gcm_set_slab_ocean), single domain, fp64 and fp32, against the
NumPy restatement tests/pe25d_slab_ocean_ref.py: the slab launch's bits, the cell budget of a step, the flux words the
radiation's BUDGET launch and the boundary layer store, the closure of the radiation's budget, the tie to the
reference's ground rule, "off means off", the refusals and the restart.  Latitude bands:
tests/test_pe25d_band_slab_ocean_gpu.py.

Shapes (H, W, L) x ptop in (0, 1000) reach the five instantiations of the radiation kernel -- L <= 24, L <= 40 and
L > 40, with the factored Exner term (ptop = 0) and without -- a ragged 64-lane tile of the slab launch (W = 10, 36, 70,
300), a ragged 128-thread radiation tile and rows of several tiles.  W = 300 takes no filter plan.

Bounds.  The slab launch, the cell rule applied to fetched words, LW_UP and everything "off" or restarted: bit for bit.
The radiation words but LW_UP go through the Exner routine: 1e-10 of the column's largest word, the project's bound.
A sum recovered as a difference of running sums is right to the rounding of the larger running sum (one unit in its
last place).  The budgets are sums of at most L + 8 terms, each rounded to 1.1e-16: 1e-12 of the sum of the terms'
magnitudes; the terms of the cell budget are those of C gt' - C gt = sum of the energy terms, both sides, and the test
also holds the difference to the tighter C ulp(gt') + 1e-12 sum |energy terms| that the rounding of gt' alone explains.
The ground temperature of the thin slab against the reference's rule: 2 units in the last place (two association orders
of an increment far below gt)."""
import numpy as np
import pytest

import gpu_setups as su
import pe25d_boundary_layer_ref as bref
import pe25d_inputs as inp
import pe25d_slab_ocean_ref as ref
from column_phase_cases import assert_same, final, shape_id
from gpu_setups import g  # noqa: F401  (the fixture)
from oracle.physics import sb_constant

pytestmark = pytest.mark.gpu

DTS = 120.0
UTC0 = inp.UTC0
ALBEDO, T_LW, T_SW = 0.3, 0.1, 0.9                      # set_physics' defaults
CASES = [(shape, ptop) for shape in ref.SHAPES for ptop in ref.PTOPS]
IDS = ["%s-%g" % (shape_id(s), p) for s, p in CASES]
THIN = 1.13e6 * 0.1                                       # the reference's ground: Cg times 10 cm

_cache = {}


def case(shape, ptop, dtype):
    """(geometry, state, ground temperature) of a case, computed once and left unchanged: the windy, humid state of the
    boundary layer's tests and a ground warmer and colder than the air above it"""
    key = (shape, ptop, dtype)
    if key not in _cache:
        H, W, L = shape
        geom = su.geom_of(H, W, L, ptop)
        st = bref.windy_state(geom, dtype)
        gt = bref.ground(geom, st)
        for a in st + [gt]:
            a.setflags(write=False)
        _cache[key] = (geom, st, gt)
    return _cache[key]


def handle(g, geom, st, gt, dtype, phys=True, bl=True, slab=None):
    """a single-domain handle with the phases registered in the model's order; slab: set_slab_ocean's arguments, None: not
    registered"""
    c = su.single(g, geom, st, dtype=dtype, gt=gt, filter=geom.width != 300)
    if phys:
        c.set_physics(geom, UTC0)
    if bl:
        c.set_boundary_layer()
    if slab is not None:
        c.set_slab_ocean(**slab)
    return c


def fields_of(shape2, seed=3):
    """a capacity field with cells held at their temperature (inf) and a heat-flux field"""
    rng = np.random.default_rng(seed)
    cap = 10.0 ** rng.uniform(5.0, 7.5, shape2)
    cap[rng.random(shape2) < 0.2] = np.inf
    cap[0, 0], cap[-1, -1] = np.inf, 2.0e5
    return cap, 40.0 * rng.standard_normal(shape2)


def random_words(shape2, seed):
    rng = np.random.default_rng(seed)
    w = np.empty((ref.NWORDS,) + shape2)
    w[ref.SC] = 1360.0 * rng.random(shape2)
    w[ref.SW_SFC] = 0.6 * w[ref.SC]
    w[ref.LW_DOWN] = 250.0 + 150.0 * rng.random(shape2)
    w[ref.LW_UP] = 300.0 + 400.0 * rng.random(shape2)
    w[ref.OLR] = 150.0 + 150.0 * rng.random(shape2)
    w[ref.SH_J] = 6.0e4 * rng.standard_normal(shape2)
    w[ref.EVAP_KG] = 0.05 * rng.standard_normal(shape2)
    return w


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---------------------------------------------------------------- 1: the slab launch's bits
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=shape_id)
def test_apply_equals_the_restatement_bit_for_bit(g, shape, dtype):
    """slab_ocean_apply on random words: gt' and the ten sums over two applications with different dt, the words read
    back; then again with a capacity field whose inf cells keep their bits and a heat-flux field"""
    geom, st, gt = case(shape, 0.0, dtype)
    H, W, _ = shape
    cap, Q = fields_of((H, W))
    for what, reg, C_, Q_ in (("scalar", dict(heat_capacity=3.0e6, Lv=2.4e6), 3.0e6, 0.0),
                              ("fields", dict(Lv=2.4e6, capacity=cap, qflux=Q), cap, Q)):
        c = handle(g, geom, st, gt, dtype, phys=False, bl=False, slab=reg)
        want_gt, want_sums, sec = gt, None, 0.0
        for n, dt in enumerate((600.0, 150.0)):
            w = random_words((H, W), 10 * n + H)
            c.slab_ocean_apply(dt, w, heat_capacity=reg.get("heat_capacity", 1.0e7), Lv=2.4e6)
            want_gt, want_sums = ref.apply(want_gt, w, dt, want_sums, C_, 2.4e6, Q_)
            sec += dt
            assert np.array_equal(c.slab_ocean_fluxes(), w), (what, n)
            assert np.array_equal(bits(c.get_ground()), bits(want_gt)), (what, n)
            rec = c.slab_ocean_sums()
            assert (rec.nsteps, rec.seconds) == (n + 1, sec)
            for k in range(ref.NSUMS):
                assert np.array_equal(rec.sums[k], want_sums[k]), (what, n, "sum", k)
        if what == "fields":
            held = np.isinf(cap)
            assert np.array_equal(bits(c.get_ground())[held], bits(gt)[held]) and (c.get_ground()[~held] != gt[~held]).all()
        assert_same(c.get_state(), st, "the launch writes no state field")
        c.close()


def test_apply_without_a_registration_sums_nothing(g):
    geom, st, gt = case(ref.SHAPES[0], 0.0, "f64")
    H, W, _ = ref.SHAPES[0]
    c = handle(g, geom, st, gt, "f64", phys=False, bl=False)
    with pytest.raises(g.GcmError):
        c.slab_ocean_fluxes()                                # no words in place yet
    w = random_words((H, W), 2)
    c.slab_ocean_apply(300.0, w, heat_capacity=THIN)
    assert np.array_equal(bits(c.get_ground()), bits(ref.cells(gt, w, 300.0, THIN)[0]))
    assert np.array_equal(c.slab_ocean_fluxes(), w)
    assert not c.slab_ocean_registered and c.slab_ocean is None
    with pytest.raises(g.GcmError):
        c.slab_ocean_sums()
    c.close()


# ---------------------------------------------------------------- 2: the cell budget of a step
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,ptop", CASES, ids=IDS)
def test_cell_budget_of_a_step(g, shape, ptop, dtype):
    """step(1) with physics, boundary layer and slab: gt' is the restatement's cell rule applied to the fetched words, bit
    for bit, the sums are the restatement's terms of those words, and C (gt' - gt) is the step's increment of the sums"""
    geom, st, gt = case(shape, ptop, dtype)
    H, W, _ = shape
    cap, Q = fields_of((H, W))
    cap = np.where(np.isinf(cap), 4.0e5, cap)                # (finite: every cell has a budget)
    c = handle(g, geom, st, gt, dtype, slab=dict(capacity=cap, qflux=Q))
    c.step(1, DTS)
    w, gt1, rec = c.slab_ocean_fluxes(), c.get_ground(), c.slab_ocean_sums()
    c.close()
    assert np.isfinite(w).all() and (w[ref.SC] > 0).any() and w[ref.SH_J].any() and w[ref.EVAP_KG].any()
    want_gt, want_sums = ref.apply(gt, w, DTS, None, cap, 2.5e6, Q)
    assert np.array_equal(bits(gt1), bits(want_gt))
    assert (rec.nsteps, rec.seconds) == (1, DTS)
    for k in range(ref.NSUMS):
        assert np.array_equal(rec.sums[k], want_sums[k]), ("sum", k)
    s = rec.sums
    energy = [s[1], s[2], -s[3], -s[5], -s[6], s[7]]
    lhs = cap * (gt1 - gt)
    err = np.abs(lhs - sum(energy))
    mag = sum(np.abs(e) for e in energy)
    both_sides = mag + cap * np.abs(gt1) + cap * np.abs(gt)
    tight = cap * np.spacing(np.abs(gt1)) + 1e-12 * mag
    print("cell budget", shape, ptop, dtype, "err / (1e-12 sum|terms|) %.3g, err / tight %.3g"
          % (float(np.max(err / (1e-12 * both_sides))), float(np.max(err / tight))))
    assert np.all(err <= 1e-12 * both_sides)
    assert np.all(err <= tight)


# ---------------------------------------------------------------- 3: the flux words
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,ptop", CASES, ids=IDS)
def test_flux_words_against_the_restatement(g, shape, ptop, dtype):
    """the walk of the phases on the state as set (end_step: no dynamics ahead of them).  LW_UP bit for bit; SC, SW_SFC,
    LW_DOWN and OLR within 1e-10 of the column's largest word; SH_J and EVAP_KG are the step's increments of
    boundary_layer_sums(): the first step's exactly (0 + x), the second's to the rounding of the running sum.  (That
    theta of the BUDGET launch is the other instantiations' bit for bit: test_thin_slab_is_the_references_ground.)"""
    geom, st, gt = case(shape, ptop, dtype)
    c = handle(g, geom, st, gt, dtype, slab={})
    c.end_step(DTS)
    w, bl1 = c.slab_ocean_fluxes(), c.boundary_layer_sums()
    want = ref.radiation_words(st[0], st[3], gt, geom, UTC0, T_LW, T_SW, ALBEDO)
    assert np.array_equal(bits(w[ref.LW_UP]), bits(want[ref.LW_UP]))
    scale = np.max(np.abs(want), axis=0)
    share = np.abs(w[:5] - want) / (1e-10 * scale)
    print("flux words", shape, ptop, dtype, " ".join("%s %.3g" % (n, float(np.max(x))) for n, x in zip(ref.WORDS, share)))
    assert (want[ref.SC] > 0).any() and (want[ref.SC] == 0).any(), "day and night"
    assert np.all(share <= 1.0)
    assert np.array_equal(w[ref.SC][want[ref.SC] == 0], want[ref.SC][want[ref.SC] == 0])
    assert np.array_equal(w[ref.SH_J], bl1.shf) and np.array_equal(w[ref.EVAP_KG], bl1.evap)
    assert bl1.shf.any() and bl1.evap.any()
    gt1 = c.get_ground()
    assert np.array_equal(bits(gt1), bits(ref.cells(gt, w, DTS)[0]))
    c.end_step(DTS)
    w2, bl2 = c.slab_ocean_fluxes(), c.boundary_layer_sums()
    c.close()
    for word, a, b in ((ref.SH_J, bl1.shf, bl2.shf), (ref.EVAP_KG, bl1.evap, bl2.evap)):
        ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
        assert np.all(np.abs(w2[word] - (b - a)) <= ulp), ref.WORDS[word]
    assert np.array_equal(bits(w2[ref.LW_UP]), bits(1 * sb_constant * ((gt1 * gt1) * (gt1 * gt1))))


def test_words_of_a_phase_that_is_not_registered_read_as_zero(g):
    shape = ref.SHAPES[1]
    geom, st, gt = case(shape, 0.0, "f64")
    c = handle(g, geom, st, gt, "f64", slab={})
    c.end_step(DTS)
    assert all(x.any() for x in c.slab_ocean_fluxes())
    c.set_boundary_layer(None)
    c.end_step(DTS)
    w = c.slab_ocean_fluxes()
    assert not w[ref.SH_J].any() and not w[ref.EVAP_KG].any() and w[ref.LW_UP].all()
    gt1 = c.get_ground()
    c.set_physics(None)
    c.end_step(DTS)
    assert not c.slab_ocean_fluxes().any()
    assert np.array_equal(bits(c.get_ground()), bits(gt1)), "no flux, no heat flux: the slab keeps its bits"
    rec = c.slab_ocean_sums()
    assert (rec.nsteps, rec.seconds) == (3, 3 * DTS)
    c.close()


# ---------------------------------------------------------------- 4: the radiation's closure
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,ptop", CASES, ids=IDS)
def test_radiation_closure(g, shape, ptop, dtype):
    """(SC - albedo SC csw_top[0]) - OLR - (S + B - U_s) = sum_k dTdt_k Cp p dsig_k / G, dTdt from the diagnostic
    grey_radiation at the same clock and state -- of a float64 handle that holds the same values, because an fp32
    handle hands dTdt out rounded to float32, which is no part of what is tested here (its arithmetic is float64 on
    either)"""
    geom, st, gt = case(shape, ptop, dtype)
    c = handle(g, geom, st, gt, dtype, bl=False, slab={})
    c.end_step(DTS)
    w = c.slab_ocean_fluxes()
    c.close()
    d = handle(g, geom, st, gt, "f64", phys=False, bl=False)
    dTdt, _ = d.grey_radiation(geom, UTC0, T_LW, T_SW, ALBEDO)
    d.close()
    csw0 = float(g.core.grey_radiation_tables(geom.dsig, geom.sig, T_LW, T_SW)["csw_top"][0])
    heat, mag = ref.column_heating(dTdt, st[0], geom)
    lhs = (w[ref.SC] - ALBEDO * w[ref.SC] * csw0) - w[ref.OLR] - ((w[ref.SW_SFC] + w[ref.LW_DOWN]) - w[ref.LW_UP])
    scale = mag + np.abs(w[:5]).sum(axis=0)
    err = float(np.max(np.abs(lhs - heat) / scale))
    print("radiation closure", shape, ptop, dtype, "%.3g" % err)
    assert err <= 1e-12, err


# ---------------------------------------------------------------- 5: the tie to the reference's rule
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,ptop", CASES, ids=IDS)
def test_thin_slab_is_the_references_ground(g, shape, ptop, dtype):
    """radiation only, C = Cg x 10 cm, no boundary layer, no heat flux: theta after step(1) is the unregistered run's bit
    for bit, the ground temperature within 2 units in the last place"""
    geom, st, gt = case(shape, ptop, dtype)
    want = handle(g, geom, st, gt, dtype, bl=False)
    want.step(1, DTS)
    c = handle(g, geom, st, gt, dtype, bl=False, slab=dict(heat_capacity=THIN))
    c.step(1, DTS)
    got, ws = final(c), final(want)
    assert_same(got[:5], ws[:5], "state")
    assert (ws[5] != gt).all(), "the ground moves"
    n = ref.ulps(got[5], ws[5])
    print("thin slab", shape, ptop, dtype, "ulps %.3g" % n)
    assert n <= 2.0


# ---------------------------------------------------------------- 6: off means off
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_unregistered_is_as_never_registered(g, dtype):
    geom, st, gt = case(ref.SHAPES[1], 0.0, dtype)
    H, W, _ = ref.SHAPES[1]
    cap, Q = fields_of((H, W))
    never = handle(g, geom, st, gt, dtype)
    never.step(3, DTS)
    c = handle(g, geom, st, gt, dtype, slab=dict(capacity=cap, qflux=Q))
    assert c.slab_ocean_registered and c.slab_ocean["heat_capacity"] == 1.0e7
    c.set_slab_ocean(None)
    assert not c.slab_ocean_registered and c.slab_ocean is None
    c.set_slab_ocean(None)                                   # (nothing to do)
    c.step(3, DTS)
    with pytest.raises(g.GcmError):
        c.slab_ocean_fluxes()
    assert_same(final(c), final(never), "registered, then unregistered")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_dt_zero_keeps_every_bit(g, dtype):
    """the boundary layer and the slab with dt = 0: no bit of the state or the ground temperature changes (the solar
    step's theta goes to T and back, which is the radiation's own affair: not registered here)"""
    geom, st, gt = case(ref.SHAPES[1], 0.0, dtype)
    H, W, _ = ref.SHAPES[1]
    _, Q = fields_of((H, W))
    c = handle(g, geom, st, gt, dtype, phys=False, slab=dict(heat_capacity=THIN, qflux=Q))
    c.end_step(0.0)
    assert np.array_equal(bits(c.get_ground()), bits(gt))
    assert_same(c.get_state(), st, "dt = 0")
    rec = c.slab_ocean_sums()
    assert (rec.nsteps, rec.seconds) == (1, 0.0) and not rec.sums.any() and not c.slab_ocean_fluxes().any()
    c.close()


def test_refused_calls_change_nothing(g):
    lib, L_ = g._lib.lib, g._lib
    geom, st, gt = case(ref.SHAPES[0], 0.0, "f64")
    H, W, _ = ref.SHAPES[0]
    # no ground temperature: GCM_ERR_STATE, in the call itself
    bare = su.single(g, geom, st)
    with pytest.raises(g.GcmError, match="gcm_set_ground"):
        bare.set_slab_ocean()
    with pytest.raises(g.GcmError, match="gcm_set_ground"):
        bare.slab_ocean_apply(DTS, random_words((H, W), 1))
    assert not bare.slab_ocean_registered
    bare.close()
    c = handle(g, geom, st, gt, "f64", slab=dict(heat_capacity=2.0e6))
    # get, put, reset without a registration are GCM_ERR_STATE: on a second handle
    d = handle(g, geom, st, gt, "f64")
    z = np.zeros((ref.NSUMS, H, W))
    assert lib.gcm_get_slab_ocean(d._h, None, None, None) == L_.ERR_STATE
    assert lib.gcm_put_slab_ocean(d._h, z.ctypes.data_as(L_._dp), 0.0, 0) == L_.ERR_STATE
    assert lib.gcm_slab_ocean_reset(d._h) == L_.ERR_STATE and lib.gcm_slab_ocean_on(d._h) == 0
    d.close()
    c.step(1, DTS)
    was, was_state, was_w = c.slab_ocean_sums(), final(c, close=False), c.slab_ocean_fluxes()
    assert was.sums[:5].any() and was.nsteps == 1
    bad_cap = np.full((H, W), 1.0e6)
    bad_cap[2, 3] = 0.0
    for kw in (dict(heat_capacity=0.0), dict(heat_capacity=-1.0), dict(heat_capacity=np.nan), dict(Lv=0.0), dict(Lv=np.nan),
               dict(capacity=bad_cap), dict(capacity=np.where(bad_cap == 0, np.nan, bad_cap)),
               dict(qflux=np.full((H, W), np.inf))):
        with pytest.raises(ValueError, match="gcm_set_slab_ocean"):
            c.set_slab_ocean(**kw)
    with pytest.raises(ValueError):
        c.set_slab_ocean(capacity=np.ones((H + 1, W)))
    with pytest.raises(ValueError):
        c.slab_ocean_apply(np.nan, was_w)
    with pytest.raises(ValueError):
        c.slab_ocean_apply(DTS, was_w, heat_capacity=0.0)
    with pytest.raises(ValueError):
        c.put_slab_ocean(-1, 0.0, was.sums)
    with pytest.raises(ValueError):
        c.put_slab_ocean(1, float("nan"), was.sums)
    assert lib.gcm_put_slab_ocean(c._h, None, 0.0, 0) == L_.ERR_ARG
    assert lib.gcm_get_slab_ocean_fluxes(c._h, None) == L_.ERR_ARG
    assert lib.gcm_slab_ocean_apply(c._h, DTS, None, was_w.ctypes.data_as(L_._dp)) == L_.ERR_ARG
    assert c.slab_ocean == dict(heat_capacity=2.0e6, Lv=2.5e6, capacity=None, qflux=None) and lib.gcm_slab_ocean_on(c._h) == 1
    now = c.slab_ocean_sums()
    assert (now.nsteps, now.seconds) == (was.nsteps, was.seconds) and np.array_equal(now.sums, was.sums)
    assert np.array_equal(c.slab_ocean_fluxes(), was_w)
    assert_same(final(c, close=False), was_state, "after refused calls")
    # put / get / reset
    rng = np.random.default_rng(0)
    sums = rng.standard_normal(was.sums.shape)
    c.put_slab_ocean(5, 600.0, sums)
    got = c.slab_ocean_sums()
    assert (got.nsteps, got.seconds) == (5, 600.0) and np.array_equal(got.sums, sums)
    c.slab_ocean_reset()
    got = c.slab_ocean_sums()
    assert (got.nsteps, got.seconds) == (0, 0.0) and not got.sums.any()
    c.close()
    # other models
    s = g.Core(g._lib.SW2D, 32, 16, dx=1e5)
    rec = L_.SlabOcean(1.0e7, 2.5e6)
    assert lib.gcm_set_slab_ocean(s._h, rec, None, None) == L_.ERR_UNSUPPORTED
    assert lib.gcm_get_slab_ocean(s._h, None, None, None) == L_.ERR_UNSUPPORTED
    assert lib.gcm_slab_ocean_reset(s._h) == L_.ERR_UNSUPPORTED and lib.gcm_slab_ocean_on(s._h) == 0
    s.close()


# ---------------------------------------------------------------- 7: the restart
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_checkpoint_resumes_bit_exactly(g, dtype, tmp_path):
    from gcmiipy_amd import checkpoint
    geom, st, gt = case(ref.SHAPES[1], 0.0, dtype)
    H, W, _ = ref.SHAPES[1]
    cap, Q = fields_of((H, W))
    reg = dict(heat_capacity=5.0e6, Lv=2.45e6, capacity=cap, qflux=Q)
    before, after = 2, 2
    whole = handle(g, geom, st, gt, dtype, slab=reg)
    whole.step(before + after, DTS)
    want, want_rec, want_bl = final(whole, close=False), whole.slab_ocean_sums(), whole.boundary_layer_sums()
    whole.close()
    a = handle(g, geom, st, gt, dtype, slab=reg)
    a.step(before, DTS)
    path = str(tmp_path / "slab.npz")
    checkpoint.save(path, a, step=before, geom=geom)
    utc = a.utc()
    a.close()
    b, ck = checkpoint.restore(path)
    assert ck["slab_ocean"]["n"] == before and ck["slab_ocean"]["seconds"] == before * DTS
    assert ck["slab_ocean"]["params"] == dict(heat_capacity=5.0e6, Lv=2.45e6)
    now = b.slab_ocean
    assert now["heat_capacity"] == 5.0e6 and np.array_equal(now["capacity"], cap) and np.array_equal(now["qflux"], Q)
    assert b.boundary_layer_registered
    b.set_physics(geom, utc)                                 # (the clock is the caller's to restore)
    b.step(after, DTS)
    assert_same(final(b, close=False), want, "restored")
    rec = b.slab_ocean_sums()
    assert (rec.nsteps, rec.seconds, rec.reflect) == (want_rec.nsteps, want_rec.seconds, want_rec.reflect)
    assert np.array_equal(rec.sums, want_rec.sums) and rec.sums[7].any()
    assert np.array_equal(b.boundary_layer_sums().shf, want_bl.shf)
    assert np.isfinite(rec.toa_net).all() and np.isfinite(rec.surface_net).all() and (rec.sst_mean > 200).all()
    b.close()
    # a file without the keys restores with none; a slab registered through C alone is refused
    plain = handle(g, geom, st, gt, dtype)
    checkpoint.save(path, plain, geom=geom)
    rec_c = g._lib.SlabOcean(1.0e7, 2.5e6)
    assert g._lib.lib.gcm_set_slab_ocean(plain._h, rec_c, None, None) == g._lib.OK
    with pytest.raises(g.GcmError, match="gcm_set_slab_ocean"):
        checkpoint.save(str(tmp_path / "c.npz"), plain, geom=geom)
    plain.close()
    c, ck = checkpoint.restore(path)
    assert ck["slab_ocean"] is None and c.slab_ocean is None and not c.slab_ocean_registered
    c.close()
