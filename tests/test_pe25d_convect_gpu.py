"""The convective adjustment of GCM_PE25D on the device (gcm_set_convect, gcm_convect_step) against the NumPy restatement
tests/pe25d_convect_ref.py, its conservation properties on the device, the registered phase against the explicit call
(alone and between the Held-Suarez forcing and the moist physics), the refusals of its own parameters and records, and
the stack that does not fit the LDS.  What it shares with the other column phases -- latitude bands against the single
domain, the explicit step without a registration, the common refusals, the checkpoint -- is
tests/test_pe25d_column_phases_gpu.py's; the end of a step with every phase registered is
tests/test_pe25d_end_step_gpu.py's.  theta goes through the device's Exner routine, exp and log:
1e-10 relative to the field's maximum (the project's parity bound) for either storage type; the decisions do not depend
on those last bits (tests/test_pe25d_convect_cpu.py holds the inputs 1e-9 clear of a tie), so the set of changed cells
and the counts are the restatement's exactly."""
import functools

import numpy as np
import pytest

import column_phase_cases as cc
import gpu_setups as su
import pe25d_inputs as inp
import pe25d_convect_ref as ref
from column_phase_cases import DTS, GAMMA, KC, STEP, assert_same, assert_same_sums, final, linf, wet_state

pytestmark = pytest.mark.gpu

PH = cc.CONVECT
UTC0 = inp.UTC0
TOL = 1e-10
geom_of = PH.geom_of                                     # (L, H, W)
handle = functools.partial(cc.handle, PH)                # (the kernel tests' shapes are never stepped and take no filter plan)


# ---------------------------------------------------------------- 1: the kernel against the restatement
_ref_cache = {}


def _restated(shape, ptop, kc, mix_q, dtype):
    """the restatement's result on the case's input, computed once and left unchanged"""
    key = (shape, ptop, kc, mix_q, dtype)
    if key not in _ref_cache:
        geom = geom_of(shape, ptop)
        st = ref.unstable_state(geom, kc, dtype)
        out = ref.convect_step(st[0], st[3], st[4], geom.sig, geom.dsig, ptop, ref.params(kappa_c=kc, mix_q=mix_q), dtype)
        for a in list(st) + list(out):
            a.setflags(write=False)
        _ref_cache[key] = (geom, st, out)
    return _ref_cache[key]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ptop", ref.PTOPS)
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_step_equals_the_restatement(shape, ptop, dtype):
    import gcmiipy_amd as g
    L, H, W = shape
    trs, gt = inp.tracers(H, W, L, 2), inp.ground(H, W)
    for gamma in (None, GAMMA):
        kc = 0.0 if gamma is None else KC
        for mix_q in (0, 1):
            geom, st, (tn, qn, count, levels) = _restated(shape, ptop, kc, mix_q, dtype)
            c = handle(g, geom, st, dtype, gt=gt)
            c.set_tracers(trs)
            trs0 = c.get_tracers()
            c.set_convect(gamma=gamma, mix_q=mix_q)
            assert c.convect == ref.params(kappa_c=kc, mix_q=mix_q)
            c.convect_step(gamma=gamma, mix_q=mix_q)
            p, u, v, t, q = c.get_state()
            sums = c.convect_sums()
            errs = dict(t=linf(t, tn), q=linf(q, qn))
            print("convect step", shape, ptop, dtype, gamma, mix_q, errs, "adjusted", float(count.mean()))
            assert errs["t"] <= TOL and errs["q"] <= TOL, errs
            # exactly the restatement's cells changed, nothing else was touched
            assert np.array_equal(t != st[3], tn != st[3]) and (t != st[3]).any()
            assert np.array_equal(q != st[4], qn != st[4]) and (q != st[4]).any() == bool(mix_q)
            assert np.array_equal(sums.count, count) and np.array_equal(sums.levels, levels)
            assert count.any() and not count.all()
            assert (sums.nsteps, sums.seconds) == (1, 0.0)
            assert np.array_equal(p, st[0]) and np.array_equal(u, st[1]) and np.array_equal(v, st[2])
            assert np.array_equal(c.get_tracers(), trs0) and np.array_equal(c.get_ground(), gt)
            c.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_stable_state_comes_back_bit_for_bit(shape, dtype):
    import gcmiipy_amd as g
    for ptop, gamma in ((0.0, None), (1000.0, GAMMA)):
        geom = geom_of(shape, ptop)
        st = ref.unstable_state(geom, 0.0 if gamma is None else KC, dtype, stable=True)
        c = handle(g, geom, st, dtype)
        c.set_convect(gamma=gamma)
        c.convect_step(gamma=gamma)
        sums = c.convect_sums()
        assert not sums.count.any() and not sums.levels.any() and sums.nsteps == 1
        assert_same(final(c), st, "stable")


@pytest.mark.parametrize("ptop", ref.PTOPS)
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_device_result_conserves_enthalpy_and_water(shape, ptop):
    """computed in NumPy from the handle's own fields, before and after"""
    import gcmiipy_amd as g
    geom = geom_of(shape, ptop)
    for gamma in (None, GAMMA):
        c = handle(g, geom, ref.unstable_state(geom, 0.0 if gamma is None else KC))
        p0, _, _, t0, q0 = c.get_state()
        c.convect_step(gamma=gamma)
        p, u, v, t, q = c.get_state()
        h0, h1 = (ref.column_enthalpy(p0, x, geom.sig, geom.dsig, ptop) for x in (t0, t))
        w0, w1 = (ref.column_water(x, geom.dsig) for x in (q0, q))
        heat, water = float(np.max(np.abs(h1 - h0) / h0)), float(np.max(np.abs(w1 - w0) / w0))
        print("conservation", shape, ptop, gamma, heat, water)
        assert heat <= 1e-12 and water <= 1e-12, (heat, water)
        assert (t != t0).any() and (q != q0).any()
        if gamma is None:
            assert (np.diff(t, axis=0) >= 0).all() and (np.diff(t0, axis=0) < 0).any()
            # a second application changes no bit
            c.convect_step()
            assert_same(c.get_state(), [p, u, v, t, q], "second application")
        c.close()


# ---------------------------------------------------------------- 2: registered against explicit
@pytest.mark.parametrize("suite", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_registered_equals_explicit(dtype, suite):
    """set_convect + step(3) against three rounds of step(1) [+ solar_step + held_suarez_step] + convect_step
    [+ moist_step] on a handle that carries no registration while it steps: the order of the phases is Matsuno step,
    solar step, Held-Suarez, convection, moist physics, sample.  The explicit side registers around each convect_step
    alone, to read that application's counts, and adds them up on the host"""
    import gcmiipy_amd as g
    geom = geom_of(STEP)
    L, H, W = STEP
    st, gt = wet_state(geom, dtype), inp.ground(H, W)
    par = dict(gamma=GAMMA)
    mo = dict(tau_e=86400.0)

    def explicit(order):
        a = handle(g, geom, st, dtype, gt=gt)
        tot_c, tot_l = np.zeros((H, W)), np.zeros((H, W))
        for n in range(3):
            assert a.convect is None
            a.step(1, DTS)
            if suite:
                a.solar_step(geom, DTS, UTC0 + n * DTS)
                a.held_suarez_step(geom, DTS)
            for phase in order:
                if phase == "convect":
                    a.set_convect(**par)
                    a.convect_step(**par)
                    one = a.convect_sums()
                    assert (one.nsteps, one.seconds) == (1, 0.0)
                    tot_c, tot_l = tot_c + one.count, tot_l + one.levels
                    a.set_convect(None)
                elif suite:
                    a.moist_step(DTS, **mo)
        return final(a), tot_c, tot_l
    want, tot_c, tot_l = explicit(("convect", "moist"))
    b = handle(g, geom, st, dtype, gt=gt, phys=suite, hs={} if suite else None)
    b.set_convect(**par)
    if suite:
        b.set_moist(**mo)
    b.step(1, DTS)
    b.step(2, DTS)
    assert_same(final(b, close=False), want, "registered")
    sums = b.convect_sums()
    assert sums.count.max() > 0 and sums.levels.max() >= 2
    assert_same_sums(sums, g.Convect(3, 3 * DTS, tot_c, tot_l), "registered")
    if suite:
        assert b.moist_sums().precip.max() > 0
        # the other order gives other bits
        assert not np.array_equal(explicit(("moist", "convect"))[0][3], want[3])
    # the phase is not the identity
    plain = handle(g, geom, st, dtype, gt=gt, phys=suite, hs={} if suite else None)
    if suite:
        plain.set_moist(**mo)
    plain.step(3, DTS)
    assert not np.array_equal(final(plain)[3], want[3])
    # reset, then switched off: the next steps are an unregistered handle's
    b.convect_reset()
    z = b.convect_sums()
    assert (z.nsteps, z.seconds) == (0, 0.0) and not z.count.any() and not z.levels.any()
    b.set_convect(None)
    assert b.convect is None
    with pytest.raises(g.GcmError):
        b.convect_sums()
    b.step(2, DTS)
    u = handle(g, geom, want[:5], dtype, gt=want[5], hs={} if suite else None)
    if suite:
        u.set_physics(geom, UTC0 + 3 * DTS)
        u.set_moist(**mo)
    u.step(2, DTS)
    assert_same(final(b), final(u), "switched off")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_half_step_is_never_adjusted(dtype):
    import gcmiipy_amd as g
    geom = geom_of(STEP)
    st = ref.unstable_state(geom, 0.0, dtype)
    r, u = handle(g, geom, st, dtype), handle(g, geom, st, dtype)
    r.set_convect()
    for c in (r, u):
        c.half_step(0, DTS)
    star_r, star_u = r.get_star(), u.get_star()
    for k in range(5):
        assert np.array_equal(star_r[k], star_u[k]), k
    for c in (r, u):
        c.half_step(1, DTS)
    sums = r.convect_sums()
    assert sums.nsteps == 0 and not sums.count.any()
    assert_same(final(r), final(u), "half steps")


# ---------------------------------------------------------------- 3: refused calls
def test_refused_calls_change_nothing():
    """the adjustment's own parameters and raw records, between the two halves of the refusals every phase shares"""
    import ctypes
    import gcmiipy_amd as g
    lib, L_ = g._lib.lib, g._lib
    geom, st, _ = cc.refusal_inputs(PH)
    c = handle(g, geom, st)
    was, was_state = cc.refused_without_a_registration(PH, g, c)
    nan, inf = float("nan"), float("inf")
    for over in (dict(kappa_c=-0.1), dict(kappa_c=1.0), dict(kappa_c=nan), dict(kappa_c=inf), dict(gamma=-1e-3), dict(gamma=0.04)):
        with pytest.raises(ValueError):
            c.set_convect(**over)
        with pytest.raises(ValueError):
            c.convect_step(**over)
    for rec in (L_.Convect(0.0, 2), L_.Convect(0.0, -1)):
        assert lib.gcm_set_convect(c._h, ctypes.byref(rec)) == L_.ERR_ARG
        assert lib.gcm_convect_step(c._h, ctypes.byref(rec)) == L_.ERR_ARG
    assert lib.gcm_convect_step(c._h, None) == L_.ERR_ARG
    with pytest.raises(ValueError):
        c.set_convect(kappa=0.2)
    with pytest.raises(ValueError):
        c.set_convect(gamma=GAMMA, kappa_c=KC)
    cc.refused_calls_changed_nothing(PH, g, c, was, was_state)


def test_a_stack_that_does_not_fit_the_lds_is_unsupported():
    """44 bytes per level and lane and the 2 KB Exner table: 160 KB hold L = 57.  L = 58 is refused by set and by step, and
    the handle goes on as before"""
    import gcmiipy_amd as g
    L_ = g._lib
    for L, fits in ((57, True), (58, False)):
        geom = su.geom_of(2, 64, L)
        st = ref.unstable_state(geom)
        c = handle(g, geom, st)
        rec = L_.Convect(0.0, 1)
        if fits:
            c.set_convect()
            c.convect_step()
            t = c.get_state()[3]
            want = ref.convect_step(st[0], st[3], st[4], geom.sig, geom.dsig, 0.0, ref.params())
            assert linf(t, want[0]) <= TOL and np.array_equal(c.convect_sums().levels, want[3]) and want[2].any()
        else:
            assert L_.lib.gcm_set_convect(c._h, rec) == L_.ERR_UNSUPPORTED
            assert L_.lib.gcm_convect_step(c._h, rec) == L_.ERR_UNSUPPORTED
            assert L_.lib.gcm_convect_on(c._h) == 0
            assert_same(c.get_state(), st, "refused")
        c.close()
