"""The Betts-Miller convection of GCM_PE25D on the device (gcm_set_betts_miller, gcm_betts_miller_step) against the NumPy
restatement tests/pe25d_betts_miller_ref.py, its budgets on the device, its place in the step, and the cases every
column phase takes alike (tests/column_phase_cases.py, driven by this phase's descriptor): latitude bands against the
single domain, the explicit step without a registration, the refusals, the checkpoint.

Bounds, those of tests/test_pe25d_moist_gpu.py: theta and q go through the device's Exner routine and exp: 1e-10 relative
to the field's maximum (the project's parity bound) in fp64, one rounding of float32 (2^-23) in fp32; the float64
precipitation 1e-10 for either.  A column's outcome is a chain of comparisons: the columns whose decision margin on the
restatement is under 1e-8 are kept out of the comparisons of which cells changed and of the counts (at most 1 % of a
case; tests/test_pe25d_betts_miller_cpu.py asserts that the seeded inputs keep it).  Everything else is bit for bit."""
import functools

import numpy as np
import pytest

import column_phase_cases as cc
import gpu_setups as su
import pe25d_betts_miller_ref as ref
import pe25d_inputs as inp
from column_phase_cases import DT, DTS, assert_same, assert_same_sums, final, linf

pytestmark = pytest.mark.gpu

SHAPES = ref.SHAPES
BAND = (12, 36, 9)                                       # (H, W, L); H = 12: 2 and 3 bands
STEPPED = (SHAPES[0], SHAPES[1], BAND, (48, 1440, 24))   # the shapes that take dynamics steps: they take a filter plan


def _geom(shape, ptop=0.0):
    return su.geom_of(*shape, ptop)


def _inputs(geom, dtype="f64"):
    return ref.convective_state(geom, dtype), None


PH = cc.Phase(
    name="betts_miller", record="BettsMiller", ref=ref, geom_of=_geom,
    filtered=lambda geom: (geom.height, geom.width, geom.layers) in STEPPED,
    inputs=_inputs, kernel_inputs=_inputs,
    step_takes_dt=True,
    moved=lambda sums: sums.precip.max() > 0 and sums.count.any(),
    par=dict(tau=3600.0),
    band_cases=((BAND, 2), (BAND, 3)),
    loopback_shapes=(BAND,),
    chain=dict(shape=(48, 1440, 24), dt=1.0, steps=2,
               par=dict(tau=60.0),                       # (a relaxation that moves bits in a step of one second)
               moved=lambda sums, steps: sums.precip.max() > 0 and 0.0 < sums.count.mean() / steps < 1.0),
    explicit=dict(shape=SHAPES[0], par={}),
    refusal=dict(shape=SHAPES[1], par=dict(tau=3600.0), rec=ref.params(tau=3600.0)),
    checkpoint=dict(shape=SHAPES[0], par=dict(tau=3600.0, nsub=3), rec=ref.params(tau=3600.0, nsub=3),
                    beside=dict(moist={}), steps=(2, 1)))
handle = functools.partial(cc.handle, PH)


_want = {}


def _reference(shape, ptop, dtype):
    """the state and the restatement's result of a case, computed once and left unchanged"""
    key = (shape, ptop, dtype)
    if key not in _want:
        geom = _geom(shape, ptop)
        st = ref.convective_state(geom, dtype)
        res = ref.betts_miller_step(st[0], st[3], st[4], geom.sig, geom.dsig, ptop, DT, ref.params(), dtype)
        for a in list(st) + list(res.values()):
            a.setflags(write=False)
        _want[key] = (geom, st, res)
    return _want[key]


# ---------------------------------------------------------------- 1: the kernel against the restatement
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ptop", ref.PTOPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_step_equals_the_restatement(shape, ptop, dtype):
    import gcmiipy_amd as g
    H, W, L = shape
    geom, st, res = _reference(shape, ptop, dtype)
    trs, gt = inp.tracers(H, W, L, 2), inp.ground(H, W)
    tol = 1e-10 if dtype == "f64" else 2.0 ** -23
    c = handle(g, geom, st, dtype, gt=gt)
    c.set_tracers(trs)
    trs0 = c.get_tracers()
    c.set_betts_miller()
    assert c.betts_miller == ref.params() and c.betts_miller_registered
    c.betts_miller_step(DT)
    p, u, v, t, q = c.get_state()
    sums = c.betts_miller_sums()
    keep = res["margin"] >= ref.MARGIN
    errs = dict(t=linf(t, res["t"]), q=linf(q, res["q"]), precip=linf(sums.precip, res["precip"]))
    print("betts_miller step", shape, ptop, dtype, errs, "columns kept out", int((~keep).sum()), "deep", int(res["deep"].sum()))
    assert errs["t"] <= tol and errs["q"] <= tol, errs
    assert errs["precip"] <= 1e-10, errs
    assert np.array_equal(sums.count[keep], res["deep"][keep].astype(np.float64)) and sums.count.any() and not sums.count.all()
    assert np.array_equal(sums.precip > 0, sums.count > 0)
    # the same cells changed, nothing else was touched
    for got_f, want_f, was in ((t, res["t"], st[3]), (q, res["q"], st[4])):
        a, b = got_f != was, want_f != was
        assert np.array_equal(a[:, keep], b[:, keep]) and a.any()
    still = sums.count == 0
    assert np.array_equal(t[:, still], st[3][:, still]) and np.array_equal(q[:, still], st[4][:, still])
    assert np.array_equal(p, st[0]) and np.array_equal(u, st[1]) and np.array_equal(v, st[2])
    assert np.array_equal(c.get_tracers(), trs0) and np.array_equal(c.get_ground(), gt)
    assert (sums.nsteps, sums.seconds) == (1, DT)
    c.close()


# ---------------------------------------------------------------- 2: properties on the device
@pytest.mark.parametrize("ptop", ref.PTOPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_budgets_close_on_the_device(shape, ptop):
    import gcmiipy_amd as g
    geom, st, res = _reference(shape, ptop, "f64")
    c = handle(g, geom, st)
    c.set_betts_miller()
    c.betts_miller_step(DT)
    p, u, v, t, q = c.get_state()
    sums = c.betts_miller_sums()
    c.close()
    before, after = ref.column_water(st[0], st[4], geom.dsig), ref.column_water(p, q, geom.dsig)
    water = float(np.max(np.abs((before - after) - sums.precip) / before))
    Lv = ref.DEFAULTS["Lv"]
    h0 = ref.column_enthalpy(st[0], st[3], st[4], geom.sig, geom.dsig, ptop, Lv)
    h1 = ref.column_enthalpy(p, t, q, geom.sig, geom.dsig, ptop, Lv)
    heat = float(np.max(np.abs(h1 - h0) / h0))
    print("budgets", shape, ptop, water, heat)
    assert water <= 1e-12 and heat <= 1e-12, (water, heat)
    assert (q >= 0).all() and sums.count.any()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_state_without_a_convecting_column_comes_back_bit_for_bit(shape, dtype):
    import gcmiipy_amd as g
    geom = _geom(shape)
    for st in (ref.quiet_state(geom, dtype), inp.state_of(geom, dtype)):   # no parcel saturates; q = 3e-6: no parcel is buoyant
        c = handle(g, geom, st, dtype)
        c.set_betts_miller()
        c.betts_miller_step(DT)
        sums = c.betts_miller_sums()
        assert not sums.precip.any() and not sums.count.any() and (sums.nsteps, sums.seconds) == (1, DT)
        assert_same(final(c), st, "no convecting column")


# ---------------------------------------------------------------- 3: the order of the step
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_step_applies_convect_betts_miller_moist_in_that_order(dtype):
    """convect, betts_miller and moist registered on one handle and two steps, against the same dynamics steps each
    followed by convect_step, betts_miller_step, moist_step on a handle that carries no registration while it steps: it
    registers around each explicit call alone, to read that application's sums, and adds them up on the host in the same
    order.  State and all three sums are bit for bit equal; the other order gives other bits"""
    import gcmiipy_amd as g
    shape = SHAPES[0]
    H, W, L = shape
    geom = _geom(shape)
    st = ref.convective_state(geom, dtype)
    pars = dict(convect=dict(gamma=cc.GAMMA), betts_miller=dict(tau=3600.0), moist=dict(tau_e=cc.TAU))
    order = ("convect", "betts_miller", "moist")
    a = handle(g, geom, st, dtype)
    for name in order:
        getattr(a, "set_" + name)(**pars[name])
    a.step(2, DTS)
    want = final(a, close=False)
    want_sums = {name: getattr(a, name + "_sums")() for name in order}
    a.close()
    assert want_sums["betts_miller"].count.any() and want_sums["moist"].precip.max() > 0

    def explicit(sequence):
        b = handle(g, geom, st, dtype)
        tot = {name: [np.zeros((H, W)), np.zeros((H, W))] for name in order}
        for n in range(2):
            b.step(1, DTS)
            for name in sequence:
                getattr(b, "set_" + name)(**pars[name])
                step = getattr(b, name + "_step")
                step(**pars[name]) if name == "convect" else step(DTS, **pars[name])
                one = getattr(b, name + "_sums")()
                assert one.nsteps == 1
                tot[name] = [tot[name][0] + one[2], tot[name][1] + one[3]]
                getattr(b, "set_" + name)(None)
        return final(b), tot
    got, tot = explicit(order)
    assert_same(got, want, "explicit calls in the step's order")
    for name in order:
        s = want_sums[name]
        assert (s.nsteps, s.seconds) == (2, 2 * DTS), name
        assert np.array_equal(s[2], tot[name][0]) and np.array_equal(s[3], tot[name][1]), name
    other, _ = explicit(("betts_miller", "convect", "moist"))
    assert not np.array_equal(other[3], want[3])
    other, _ = explicit(("convect", "moist", "betts_miller"))
    assert not np.array_equal(other[3], want[3]) or not np.array_equal(other[4], want[4])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_without_a_registration_nothing_is_applied(dtype):
    """a handle that registered the phase and switched it off again steps as one that never did, half steps never apply
    it, and the registered phase is not the identity"""
    import gcmiipy_amd as g
    geom = _geom(SHAPES[0])
    st = ref.convective_state(geom, dtype)
    plain = handle(g, geom, st, dtype)
    plain.step(2, DTS)
    want = final(plain)
    off = handle(g, geom, st, dtype)
    off.set_betts_miller(tau=3600.0)
    off.set_betts_miller(None)
    assert off.betts_miller is None and not off.betts_miller_registered
    off.step(2, DTS)
    assert_same(final(off), want, "switched off")
    on = handle(g, geom, st, dtype)
    on.set_betts_miller(tau=3600.0)
    on.step(2, DTS)
    assert on.betts_miller_sums().nsteps == 2
    assert not np.array_equal(final(on)[3], want[3])
    r, u = handle(g, geom, st, dtype), handle(g, geom, st, dtype)
    r.set_betts_miller()
    for c in (r, u):
        c.half_step(0, DTS)
        c.half_step(1, DTS)
    assert r.betts_miller_sums().nsteps == 0
    assert_same(final(r), final(u), "half steps")


# ---------------------------------------------------------------- 4: the cases every column phase takes
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nb", [2, 3])
def test_in_process_bands_equal_single_domain(nb, dtype):
    import gcmiipy_amd as g
    cc.in_process_bands_equal_single_domain(PH, g, BAND, nb, dtype)


@pytest.mark.parametrize("host_loop", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_loopback_band_run_equals_single_domain(dtype, host_loop, monkeypatch):
    import gcmiipy_amd as g
    cc.loopback_band_run_equals_single_domain(PH, g, BAND, dtype, host_loop, monkeypatch)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_band_run_chains_with_the_phase(dtype, monkeypatch):
    """48 x 1440 x 24, tau = 60 s, 2 steps of one second"""
    import gcmiipy_amd as g
    cc.band_run_chains_with_the_phase(PH, g, dtype, monkeypatch)


def test_explicit_step_without_a_registration_keeps_no_sums():
    import gcmiipy_amd as g
    cc.explicit_step_without_a_registration_keeps_no_sums(PH, g)


def test_refused_calls_change_nothing():
    """the phase's own parameters, between the two halves of the refusals every phase shares"""
    import gcmiipy_amd as g
    geom, st, _ = cc.refusal_inputs(PH)
    c = handle(g, geom, st)
    was, was_state = cc.refused_without_a_registration(PH, g, c)
    nan, inf = float("nan"), float("inf")
    for over in (dict(Lv=0.0), dict(Lv=-1.0), dict(Lv=nan), dict(tau=0.0), dict(tau=-1.0), dict(tau=inf), dict(rh_bm=0.0),
                 dict(rh_bm=1.5), dict(rh_bm=nan), dict(nsub=0), dict(nsub=9)):
        with pytest.raises(ValueError):
            c.set_betts_miller(**over)
        with pytest.raises(ValueError):
            c.betts_miller_step(DT, **over)
    for dt in (nan, inf):
        with pytest.raises(ValueError):
            c.betts_miller_step(dt)
    with pytest.raises(ValueError):
        c.set_betts_miller(tau_e=3.0)
    cc.refused_calls_changed_nothing(PH, g, c, was, was_state)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_checkpoint_carries_the_phase_and_its_sums(dtype, tmp_path):
    """the moist physics registered beside it, 2 + 1 steps"""
    import gcmiipy_amd as g
    cc.checkpoint_carries_the_phase_and_its_sums(PH, g, dtype, tmp_path)


# ---------------------------------------------------------------- 5: the levels the handle and the kernel's LDS hold
def test_levels_that_do_not_suit_the_scheme_are_unsupported():
    """16 bytes per level and lane and the 2 KB Exner table: 160 KB hold L = 158, more than a GCM_PE25D handle can have
    (156), so the refusal of a larger L cannot be reached through a handle; the largest handle registers and steps.  A
    sig table that does not strictly decrease is refused by set and by step, and the handle goes on as before"""
    import gcmiipy_amd as g
    L_ = g._lib
    assert L_.BETTS_MILLER_MAX_LEVELS == 158
    geom = _geom((2, 64, 156), 1000.0)
    st = ref.convective_state(geom)
    c = handle(g, geom, st)
    c.set_betts_miller()
    c.betts_miller_step(DT)
    t, q = c.get_state()[3:]
    sums = c.betts_miller_sums()
    c.close()
    res = ref.betts_miller_step(st[0], st[3], st[4], geom.sig, geom.dsig, 1000.0, DT, ref.params())
    keep = res["margin"] >= ref.MARGIN
    assert linf(t, res["t"]) <= 1e-10 and linf(q, res["q"]) <= 1e-10 and linf(sums.precip, res["precip"]) <= 1e-10
    assert np.array_equal(sums.count[keep], res["deep"][keep].astype(np.float64)) and res["deep"].any()
    # sig that does not strictly decrease: two equal levels
    geom = _geom(SHAPES[1])
    st = ref.convective_state(geom)
    sig = np.asarray(geom.sig, dtype=np.float64).copy()
    sig.reshape(-1)[1] = sig.reshape(-1)[0]
    geom.sig = sig
    c = handle(g, geom, st)
    rec = L_.BettsMiller(*ref.DEFAULTS.values())
    assert L_.lib.gcm_set_betts_miller(c._h, rec) == L_.ERR_UNSUPPORTED
    assert L_.lib.gcm_betts_miller_step(c._h, DT, rec) == L_.ERR_UNSUPPORTED
    assert L_.lib.gcm_betts_miller_on(c._h) == 0
    with pytest.raises(g.GcmError):
        c.set_betts_miller()
    assert_same(c.get_state(), st, "refused")
    c.close()
