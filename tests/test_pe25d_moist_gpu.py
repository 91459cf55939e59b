"""The moist physics of GCM_PE25D on the device (gcm_set_moist, gcm_moist_step) against the NumPy restatement
tests/pe25d_moist_ref.py, its conservation properties on the device, the registered phase against the explicit call and
the refusals of its own parameters.  What it shares with the other column phases -- latitude bands against the single
domain, the explicit step without a registration, the common refusals, the checkpoint -- is
tests/test_pe25d_column_phases_gpu.py's.  theta and q go through the device's Exner routine and exp: 1e-10 relative to
the field's maximum (the project's parity bound) in fp64, one rounding of float32 (2^-23) in fp32; the float64 sums
1e-10 for either."""
import functools

import numpy as np
import pytest

import column_phase_cases as cc
import pe25d_inputs as inp
import pe25d_moist_ref as ref
from column_phase_cases import DT, DTS, TAU, assert_same, assert_same_sums, final, linf

pytestmark = pytest.mark.gpu

PH = cc.MOIST
SHAPES = ref.SHAPES
UTC0 = inp.UTC0
geom_of = PH.geom_of                                     # (H, W, L)
handle = functools.partial(cc.handle, PH)                # (the 300-column shape is never stepped and takes no filter plan)


# ---------------------------------------------------------------- 1: the kernel against the restatement
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ptop", ref.PTOPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_step_equals_the_restatement(shape, ptop, dtype):
    import gcmiipy_amd as g
    H, W, L = shape
    geom = geom_of(shape, ptop)
    trs, gt = inp.tracers(H, W, L, 2), inp.ground(H, W)
    tol = 1e-10 if dtype == "f64" else 2.0 ** -23
    for iso in (False, True):
        st = ref.humid_state(geom, dtype, iso)
        for tau_e in (0.0, TAU):
            par = ref.params(tau_e=tau_e)
            c = handle(g, geom, st, dtype, gt=gt)
            c.set_tracers(trs)
            trs0 = c.get_tracers()
            c.set_moist(tau_e=tau_e)
            assert c.moist == par
            c.moist_step(DT, tau_e=tau_e)
            p, u, v, t, q = c.get_state()
            sums = c.moist_sums()
            tn, qn, P, E = ref.moist_step(st[0], st[3], st[4], geom.sig, geom.dsig, ptop, DT, par, dtype)
            errs = dict(t=linf(t, tn), q=linf(q, qn), precip=linf(sums.precip, P))
            if tau_e > 0:
                errs["evap"] = linf(sums.evap, E)
            print("moist step", shape, ptop, dtype, iso, tau_e, errs)
            assert errs["t"] <= tol and errs["q"] <= tol, errs
            assert errs["precip"] <= 1e-10 and errs.get("evap", 0.0) <= 1e-10, errs
            if tau_e == 0:
                assert not sums.evap.any() and not E.any()
            else:
                assert E.max() > 0
            # the same cells changed, nothing else was touched
            assert np.array_equal(q != st[4], qn != st[4]) and (q != st[4]).any()
            if dtype == "f64":                          # (a small latent heating need not move a float32 theta)
                assert np.array_equal(t != st[3], tn != st[3])
            assert np.array_equal(p, st[0]) and np.array_equal(u, st[1]) and np.array_equal(v, st[2])
            assert np.array_equal(c.get_tracers(), trs0) and np.array_equal(c.get_ground(), gt)
            assert (sums.nsteps, sums.seconds) == (1, DT)
            c.close()


# ---------------------------------------------------------------- 2: properties on the device
@pytest.mark.parametrize("ptop", ref.PTOPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_budgets_close_on_the_device(shape, ptop):
    import gcmiipy_amd as g
    geom = geom_of(shape, ptop)
    for iso in (False, True):
        st = ref.humid_state(geom, "f64", iso)
        for tau_e in (0.0, TAU):
            par = ref.params(tau_e=tau_e)
            c = handle(g, geom, st)
            c.set_moist(tau_e=tau_e)
            c.moist_step(DT, tau_e=tau_e)
            p, u, v, t, q = c.get_state()
            sums = c.moist_sums()
            before = ref.column_water(st[0], st[4], geom.dsig)
            after = ref.column_water(p, q, geom.dsig)
            water = float(np.max(np.abs((before - after) - (sums.precip - sums.evap)) / before))
            print("water budget", shape, ptop, iso, tau_e, water)
            assert water <= 1e-12, water
            if tau_e == 0:
                h0 = ref.column_enthalpy(st[0], st[3], st[4], geom.sig, geom.dsig, ptop, par["Lv"])
                h1 = ref.column_enthalpy(p, t, q, geom.sig, geom.dsig, ptop, par["Lv"])
                heat = float(np.max(np.abs(h1 - h0) / h0))
                print("enthalpy", shape, ptop, iso, heat)
                assert heat <= 1e-12, heat
            p_lev, pi = ref.levels(p, geom.sig, ptop)
            _, qs0, _, can = ref.saturation(st[3] * pi, p_lev)
            cond = can & (st[4] > qs0)
            qs1 = ref.saturation(t * pi, p_lev)[1]
            assert (q[cond] <= qs1[cond] * (1 + 1e-10)).all()
            # a second application at fp64 changes nothing, the sums included
            c.moist_step(DT, tau_e=0.0)
            again = c.moist_sums()
            assert_same(c.get_state(), [p, u, v, t, q], "second application")
            assert np.array_equal(again.precip, sums.precip) and np.array_equal(again.evap, sums.evap)
            assert (again.nsteps, again.seconds) == (2, 2 * DT)
            c.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_dry_state_comes_back_bit_for_bit(shape, dtype):
    import gcmiipy_amd as g
    geom = geom_of(shape)
    st = inp.state_of(geom, dtype)                        # q = 3e-6 (1 + noise): far below saturation everywhere
    c = handle(g, geom, st, dtype)
    c.set_moist()
    c.moist_step(DT)
    sums = c.moist_sums()
    assert not sums.precip.any() and not sums.evap.any()
    assert_same(final(c), st, "dry")


# ---------------------------------------------------------------- 3: registered against explicit
@pytest.mark.parametrize("phys,hs", [(False, False), (True, True)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_registered_equals_explicit(dtype, phys, hs):
    """set_moist + step(3) against three rounds of step(1) [+ solar_step + held_suarez_step] + moist_step on a handle
    that carries no registration while it steps: the order of the phases is Matsuno step, solar step, Held-Suarez, moist
    physics, sample.  The explicit side registers around each moist_step alone, to read that application's sums, and
    adds them up on the host in the same order"""
    import gcmiipy_amd as g
    geom = geom_of(SHAPES[0])
    H, W, L = SHAPES[0]
    st, gt = ref.humid_state(geom, dtype), inp.ground(H, W)
    par = dict(tau_e=TAU)
    a = handle(g, geom, st, dtype, gt=gt, every=1000)     # (never due within this test: sampled by hand below)
    tot_p, tot_e = np.zeros((H, W)), np.zeros((H, W))
    for n in range(3):
        assert a.moist is None
        a.step(1, DTS)
        if phys:
            a.solar_step(geom, DTS, UTC0 + n * DTS)
        if hs:
            a.held_suarez_step(geom, DTS)
        a.set_moist(**par)
        a.moist_step(DTS, **par)
        one = a.moist_sums()
        assert (one.nsteps, one.seconds) == (1, DTS)
        tot_p, tot_e = tot_p + one.precip, tot_e + one.evap
        a.set_moist(None)
        if n == 0:
            a.climate_sample()
            first = a.climate_sums()
    want = final(a)
    b = handle(g, geom, st, dtype, gt=gt, phys=phys, hs={} if hs else None, every=1)
    b.set_moist(**par)
    b.step(1, DTS)
    n1, m3, m2 = b.climate_sums()
    assert n1 == 1 and np.array_equal(m3, first[1]) and np.array_equal(m2, first[2]), "the sample sees the moist state"
    b.step(2, DTS)
    assert_same(final(b, close=False), want, "registered")
    sums = b.moist_sums()
    assert sums.precip.max() > 0 and sums.evap.max() > 0
    assert_same_sums(sums, g.Moist(3, 3 * DTS, tot_p, tot_e), "registered")
    # the phase is not the identity, and the other order gives other bits
    plain = handle(g, geom, st, dtype, gt=gt, phys=phys, hs={} if hs else None)
    plain.step(3, DTS)
    assert not np.array_equal(final(plain)[3], want[3])
    if hs:
        o = handle(g, geom, st, dtype, gt=gt)
        for n in range(3):
            o.step(1, DTS)
            o.solar_step(geom, DTS, UTC0 + n * DTS)
            o.moist_step(DTS, **par)
            o.held_suarez_step(geom, DTS)
        assert not np.array_equal(final(o)[3], want[3])
    # reset, then registered and unregistered: the next steps are an unregistered handle's
    b.moist_reset()
    z = b.moist_sums()
    assert (z.nsteps, z.seconds) == (0, 0.0) and not z.precip.any() and not z.evap.any()
    b.set_moist(None)
    assert b.moist is None
    with pytest.raises(g.GcmError):
        b.moist_sums()
    b.set_climate(0)
    b.step(2, DTS)
    u = handle(g, geom, want[:5], dtype, gt=want[5], hs={} if hs else None)
    if phys:
        u.set_physics(geom, UTC0 + 3 * DTS)
    u.step(2, DTS)
    assert_same(final(b), final(u), "switched off")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_half_step_is_never_forced(dtype):
    import gcmiipy_amd as g
    geom = geom_of(SHAPES[0])
    st = ref.humid_state(geom, dtype)
    r, u = handle(g, geom, st, dtype), handle(g, geom, st, dtype)
    r.set_moist(tau_e=TAU)
    for c in (r, u):
        c.half_step(0, DTS)
    star_r, star_u = r.get_star(), u.get_star()
    for k in range(5):
        assert np.array_equal(star_r[k], star_u[k]), k
    for c in (r, u):
        c.half_step(1, DTS)
    assert r.moist_sums().nsteps == 0
    assert_same(final(r), final(u), "half steps")


# ---------------------------------------------------------------- 4: refused calls
def test_refused_calls_change_nothing():
    """the moist physics' own parameters, between the two halves of the refusals every phase shares"""
    import gcmiipy_amd as g
    geom, st, _ = cc.refusal_inputs(PH)
    c = handle(g, geom, st)
    was, was_state = cc.refused_without_a_registration(PH, g, c)
    nan, inf = float("nan"), float("inf")
    for over in (dict(Lv=0.0), dict(Lv=-1.0), dict(Lv=nan), dict(tau_e=-1.0), dict(tau_e=inf), dict(rh_s=0.0),
                 dict(rh_s=1.5), dict(rh_s=nan)):
        with pytest.raises(ValueError):
            c.set_moist(**over)
        with pytest.raises(ValueError):
            c.moist_step(DT, **over)
    for dt in (nan, inf):
        with pytest.raises(ValueError):
            c.moist_step(dt)
    with pytest.raises(ValueError):
        c.set_moist(tau=3.0)
    cc.refused_calls_changed_nothing(PH, g, c, was, was_state)
