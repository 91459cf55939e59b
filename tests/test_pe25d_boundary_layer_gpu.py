"""The surface fluxes and the boundary-layer mixing of GCM_PE25D on the device (gcm_set_boundary_layer,
gcm_boundary_layer_step) against the NumPy restatement tests/pe25d_boundary_layer_ref.py, its budgets and its maximum
principle on the device, the registered phase against the explicit calls and gcm_end_step, registration and sums, and
the refusals that are its own.  What it shares with the other column phases -- the explicit step without a registration,
the common refusals, the checkpoint -- is tests/test_pe25d_column_phases_gpu.py's.  The fields go through the device's
Exner routine, sqrt, log and exp: 1e-10 relative to the field's maximum (the project's parity bound) in fp64, one
rounding of float32 (2^-23) in fp32; the float64 sums 1e-10 for either.  The budgets and the maximum principle take the bounds of tests/test_pe25d_boundary_layer_cpu.py."""
import copy
import functools

import numpy as np
import pytest

import column_phase_cases as cc
import gpu_setups as su
import pe25d_boundary_layer_ref as ref
import pe25d_inputs as inp
from column_phase_cases import DT, DTS, GAMMA, assert_same, assert_same_sums, final, linf

pytestmark = pytest.mark.gpu

PH = cc.BOUNDARY_LAYER
SHAPES = ref.SHAPES
handle = functools.partial(cc.handle, PH)                # (the 300-column shape is never stepped and takes no filter plan)


def case(shape, ptop, dtype="f64"):
    geom = su.geom_of(*shape, ptop)
    st = ref.windy_state(geom, dtype)
    return geom, st, ref.ground(geom, st)


# ---------------------------------------------------------------- 1: the kernels against the restatement
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ptop", ref.PTOPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_step_equals_the_restatement(shape, ptop, dtype):
    import gcmiipy_amd as g
    H, W, L = shape
    geom, st, gt = case(shape, ptop, dtype)
    trs = inp.tracers(H, W, L, 2)
    tol = 1e-10 if dtype == "f64" else 2.0 ** -23
    for over in ({}, dict(cd0=1e-3, v_cap=7.5, ch=0.002, p_pbl=70000.0, p_strat=20000.0)):
        par = ref.params(**over)
        c = handle(g, geom, st, dtype, gt=gt)
        c.set_tracers(trs)
        trs0 = c.get_tracers()
        c.set_boundary_layer(**over)
        assert c.boundary_layer == par
        c.boundary_layer_step(DT, **over)
        p, u, v, t, q = c.get_state()
        sums = c.boundary_layer_sums()
        un, vn, tn, qn, shf, evap = ref.boundary_layer_step(*st, gt, geom.sig, geom.dsig, ptop, DT, par, dtype)
        errs = dict(u=linf(u, un), v=linf(v, vn), t=linf(t, tn), q=linf(q, qn), shf=linf(sums.shf, shf),
                    evap=linf(sums.evap, evap))
        print("boundary layer step", shape, ptop, dtype, over, errs)
        assert max(errs[k] for k in "uvtq") <= tol, errs
        assert errs["shf"] <= 1e-10 and errs["evap"] <= 1e-10, errs
        assert (u != st[1]).any() and (v != st[2]).any() and (t != st[3]).any() and (q != st[4]).any()
        assert np.array_equal(p, st[0])
        assert np.array_equal(c.get_tracers(), trs0) and np.array_equal(c.get_ground(), gt)
        assert (sums.nsteps, sums.seconds) == (1, DT)
        c.close()


def test_the_largest_lds_request_launches():
    """L = 40, the most levels parked in LDS (60 KB beside the 2 KB Exner table), on a row of two tiles"""
    import gcmiipy_amd as g
    geom, st, gt = case((3, 70, 40), 1000.0)
    c = su.single(g, geom, st, filter=False, gt=gt)
    c.boundary_layer_step(DT)
    got = c.get_state()
    c.close()
    want = ref.boundary_layer_step(*st, gt, geom.sig, geom.dsig, 1000.0, DT, ref.params())
    errs = {k: linf(a, b) for k, a, b in zip("uvtq", got[1:], want[:4])}
    print("boundary layer step, L = 40", errs)
    assert max(errs.values()) <= 1e-10, errs
    assert (got[1] != st[1]).any() and (got[3] != st[3]).any()


# ---------------------------------------------------------------- 2: properties on the device
@pytest.mark.parametrize("ptop", ref.PTOPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_budgets_and_maximum_principle_on_the_device(shape, ptop):
    import gcmiipy_amd as g
    geom, st, gt = case(shape, ptop)
    c = handle(g, geom, st, gt=gt)
    c.set_boundary_layer()
    c.boundary_layer_step(DT)
    p, u, v, t, q = c.get_state()
    sums = c.boundary_layer_sums()
    c.close()
    water = ref.column_sum(st[4], geom.dsig) * p / ref.G
    dwater = (ref.column_sum(q, geom.dsig) - ref.column_sum(st[4], geom.dsig)) * p / ref.G
    err_w = float(np.max(np.abs(dwater - sums.evap) / water))
    sig0 = float(np.asarray(geom.sig).reshape(-1)[0])
    cpm = ref.CP * ((sig0 * p + ptop) / ref.P0) ** ref.KAPPA * p / ref.G
    heat = cpm * ref.column_sum(st[3], geom.dsig)
    dheat = cpm * (ref.column_sum(t, geom.dsig) - ref.column_sum(st[3], geom.dsig))
    err_h = float(np.max(np.abs(dheat - sums.shf) / heat))
    print("budgets on the device", shape, ptop, err_w, err_h)
    assert err_w <= 1e-12 and err_h <= 1e-12, (err_w, err_h)
    ref.assert_maximum_principle(st, gt, geom, [u, v, t, q])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_rest_and_dt_zero_keep_every_bit(shape, dtype):
    import gcmiipy_amd as g
    geom = su.geom_of(*shape, 1000.0)
    st, gt = ref.resting_state(geom, dtype)
    c = handle(g, geom, st, dtype, gt=gt)
    c.set_boundary_layer()
    c.boundary_layer_step(DT)
    sums = c.boundary_layer_sums()
    assert not sums.shf.any() and not sums.evap.any() and sums.nsteps == 1
    assert_same(final(c), st + [gt], "rest")
    st = ref.windy_state(geom, dtype)
    gt = ref.ground(geom, st)
    c = handle(g, geom, st, dtype, gt=gt)
    c.boundary_layer_step(0.0)
    assert_same(final(c), st + [gt], "dt = 0")


# ---------------------------------------------------------------- 3: registered against explicit
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_registered_equals_explicit_and_end_step(dtype):
    """step(3) with Held-Suarez, boundary layer, convective adjustment and moist physics registered, against three rounds
    of half_step x 2 and the explicit calls in the model's order on a handle that carries no registration, and against
    half_step x 2 + end_step on one that carries them all"""
    import gcmiipy_amd as g
    geom, st, gt = case(SHAPES[0], 0.0, dtype)
    bl = dict(cd0=1e-3)

    def registered():
        c = handle(g, geom, st, dtype, gt=gt, hs={})
        c.set_boundary_layer(**bl)
        c.set_convect(gamma=GAMMA)
        c.set_moist()
        return c
    a = handle(g, geom, st, dtype, gt=gt)
    for n in range(3):
        a.half_step(0, DTS)
        a.half_step(1, DTS)
        a.held_suarez_step(geom, DTS)
        a.boundary_layer_step(DTS, **bl)
        a.convect_step(gamma=GAMMA)
        a.moist_step(DTS)
    assert a.boundary_layer is None
    with pytest.raises(g.GcmError):
        a.boundary_layer_sums()
    want = final(a)
    b = registered()
    b.step(3, DTS)
    sums = b.boundary_layer_sums()
    assert (sums.nsteps, sums.seconds) == (3, 3 * DTS) and sums.shf.any() and sums.evap.any()
    assert_same(final(b), want, "registered")
    e = registered()
    for n in range(3):
        e.half_step(0, DTS)
        e.half_step(1, DTS)
        assert e.boundary_layer_sums().nsteps == n, "half_step never applies the phase"
        e.end_step(DTS)
    assert_same_sums(e.boundary_layer_sums(), sums, "end_step")
    assert_same(final(e), want, "end_step")
    # the phase is not the identity, and the other order gives other bits
    plain = handle(g, geom, st, dtype, gt=gt, hs={})
    plain.set_convect(gamma=GAMMA)
    plain.set_moist()
    plain.step(3, DTS)
    got = final(plain)
    assert not np.array_equal(got[1], want[1]) and not np.array_equal(got[3], want[3])
    o = handle(g, geom, st, dtype, gt=gt)
    for n in range(3):
        o.step(1, DTS)
        o.held_suarez_step(geom, DTS)
        o.convect_step(gamma=GAMMA)
        o.boundary_layer_step(DTS, **bl)
        o.moist_step(DTS)
    assert not np.array_equal(final(o)[3], want[3])


# ---------------------------------------------------------------- 4: registration and sums
def test_registration_sums_and_unregistration():
    import gcmiipy_amd as g
    geom, st, gt = case(SHAPES[0], 0.0)
    c = handle(g, geom, st, gt=gt)
    c.set_boundary_layer()
    c.step(1, DTS)
    one = c.boundary_layer_sums()
    assert (one.nsteps, one.seconds) == (1, DTS) and one.shf.any() and one.evap.any()
    # put and get round-trip
    rng = np.random.default_rng(3)
    shf, evap = rng.standard_normal(one.shf.shape), rng.standard_normal(one.shf.shape)
    c.put_boundary_layer(5, 600.0, shf, evap)
    assert_same_sums(c.boundary_layer_sums(), g.BoundaryLayer(5, 600.0, shf, evap), "put / get")
    c.boundary_layer_reset()
    z = c.boundary_layer_sums()
    assert (z.nsteps, z.seconds) == (0, 0.0) and not z.shf.any() and not z.evap.any()
    c.put_boundary_layer(one.nsteps, one.seconds, one.shf, one.evap)
    # registering again resets the sums and takes the new parameters
    c.set_boundary_layer(cd0=1e-3)
    z = c.boundary_layer_sums()
    assert c.boundary_layer == ref.params(cd0=1e-3)
    assert (z.nsteps, z.seconds) == (0, 0.0) and not z.shf.any() and not z.evap.any()
    # NULL unregisters: the next steps are a handle's that never registered
    mid = final(c, close=False)
    c.set_boundary_layer(None)
    assert c.boundary_layer is None and not c.boundary_layer_registered
    with pytest.raises(g.GcmError):
        c.boundary_layer_sums()
    c.step(2, DTS)
    u = handle(g, geom, mid[:5], gt=mid[5])
    u.step(2, DTS)
    assert_same(final(c), final(u), "switched off")


# ---------------------------------------------------------------- 5: refused calls
def test_refused_calls_change_nothing():
    """the boundary layer's own refusals -- a null handle, no ground temperature, its parameters, a latitude band, one
    level, reversed levels -- around the two halves of the refusals every phase shares"""
    import gcmiipy_amd as g
    lib, L_ = g._lib.lib, g._lib
    geom, st, gt = cc.refusal_inputs(PH)
    H, W, L = PH.refusal["shape"]
    rec = L_.BoundaryLayer(*ref.DEFAULTS.values())
    # a null handle
    assert lib.gcm_set_boundary_layer(None, rec) == L_.ERR_ARG and lib.gcm_boundary_layer_on(None) == L_.ERR_ARG
    assert lib.gcm_boundary_layer_step(None, 60.0, rec) == L_.ERR_ARG
    # no ground temperature: GCM_ERR_STATE from the registration itself, and from the explicit step
    c = handle(g, geom, st)
    assert lib.gcm_set_boundary_layer(c._h, rec) == L_.ERR_STATE and lib.gcm_boundary_layer_on(c._h) == 0
    assert lib.gcm_boundary_layer_step(c._h, 60.0, rec) == L_.ERR_STATE
    assert_same(c.get_state(), st, "no ground")
    c.set_ground(gt)
    was, was_state = cc.refused_without_a_registration(PH, g, c)
    nan, inf = float("nan"), float("inf")
    for over in (dict(cd0=-1e-3), dict(cd1=-1.0), dict(ch=-1.0), dict(ce=-1.0), dict(v_cap=0.0), dict(v_cap=-1.0),
                 dict(p_strat=0.0), dict(p_strat=-5.0), dict(cd0=nan), dict(cd1=inf), dict(v_cap=nan), dict(ch=inf),
                 dict(ce=nan), dict(p_pbl=inf), dict(p_strat=nan)):
        with pytest.raises(ValueError):
            c.set_boundary_layer(**over)
        with pytest.raises(ValueError):
            c.boundary_layer_step(DT, **over)
    for dt in (nan, inf):
        with pytest.raises(ValueError):
            c.boundary_layer_step(dt)
    with pytest.raises(ValueError):
        c.set_boundary_layer(drag=3.0)
    assert lib.gcm_boundary_layer_step(c._h, DT, None) == L_.ERR_ARG
    cc.refused_calls_changed_nothing(PH, g, c, was, was_state)
    # a latitude band
    band, other = su.bands(g, geom, 2, st, gt=gt)
    other.close()
    was_state = band.get_state()
    assert lib.gcm_set_boundary_layer(band._h, rec) == L_.ERR_UNSUPPORTED and lib.gcm_boundary_layer_on(band._h) == 0
    assert lib.gcm_boundary_layer_step(band._h, 60.0, rec) == L_.ERR_UNSUPPORTED
    assert_same(band.get_state(), was_state, "band")
    band.close()
    # one level: no interface to mix across
    geom1 = su.geom_of(H, W, 1)
    st1 = inp.state_of(geom1)
    one = su.single(g, geom1, st1, filter=False, gt=gt)
    assert lib.gcm_set_boundary_layer(one._h, rec) == L_.ERR_UNSUPPORTED and lib.gcm_boundary_layer_on(one._h) == 0
    assert lib.gcm_boundary_layer_step(one._h, 60.0, rec) == L_.ERR_UNSUPPORTED
    assert lib.gcm_boundary_layer_on(one._h) == 0
    assert_same(one.get_state(), st1, "one level")
    one.close()
    # levels that do not start at the bottom
    up = copy.copy(geom)
    up.sig = np.ascontiguousarray(np.asarray(geom.sig)[::-1])
    s = g.Core(g._lib.PE25D, W, H, L, geom=up, filter=False)
    s.set_ground(gt)
    assert lib.gcm_set_boundary_layer(s._h, rec) == L_.ERR_UNSUPPORTED and lib.gcm_boundary_layer_on(s._h) == 0
    assert lib.gcm_boundary_layer_step(s._h, 60.0, rec) == L_.ERR_UNSUPPORTED
    s.close()
