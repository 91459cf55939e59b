"""The end of a step of GCM_PE25D on its own (gcm_end_step).  What it promises: everything gcm_step and gcm_band_run queue
behind the corrector, in their order and by their code, each only if registered -- the solar step at the handle's clock
(which advances by dt), the Held-Suarez forcing, the boundary layer, the convective adjustment, the moist physics (their
sums, seconds and nsteps advance as in gcm_step), the climatology's step counter and its sample where one is due -- so
that half_step(0), half_step(1), end_step(dt) is step(1, dt) bit for bit, and a latitude band whose exchange the host
drives ends its steps as the single domain does, ghost rows with own rows; with nothing registered it queues nothing, a
non-finite dt and the other models are refused and change nothing.  Held here with the solar step, the Held-Suarez
forcing, the convective adjustment, the moist physics and the climatology registered: gcm_band_run on the loopback band
under its orchestrations and the host-driven sequence, a single domain's half steps, in-process bands, and native and
host-driven steps mixed on one runner.  (With the boundary layer too: tests/test_pe25d_boundary_layer_gpu.py; a band that
takes that phase over its own rows ends its steps in two calls around a third exchange:
tests/test_pe25d_band_boundary_layer_gpu.py.)"""
import functools

import numpy as np
import pytest

import column_phase_cases as cc
import gpu_setups as su
import pe25d_inputs as inp
from column_phase_cases import BAND, DTS, assert_same, assert_same_sums, final, wet_state

pytestmark = pytest.mark.gpu

UTC0 = inp.UTC0
PAR = cc.CONVECT.par
geom_of = cc.CONVECT.geom_of                             # (L, H, W)
handle = functools.partial(cc.handle, cc.CONVECT)


# ---------------------------------------------------------------- 1: every phase registered, on a band
_all_phases_cache = {}


def _register_all(c, geom):
    """every phase behind the dynamics, on a Core or a HipBandEngine"""
    c.set_physics(geom, UTC0)
    c.set_held_suarez(geom)
    c.set_convect(**PAR)
    c.set_moist(tau_e=86400.0)
    c.set_climate(1)


def _all_phases_reference(g, dtype, steps):
    """the single domain with every phase registered: state, convect sums, moist sums, climatology sums and the clock
    after steps[0] and after steps[0] + steps[1] steps, computed once per storage type"""
    if dtype not in _all_phases_cache:
        geom = geom_of(BAND)
        c = handle(g, geom, wet_state(geom, dtype), dtype, gt=inp.ground(BAND[1], BAND[2]))
        _register_all(c, geom)
        out = []
        for n in steps:
            c.step(n, DTS)
            out.append((final(c, close=False), c.convect_sums(), c.moist_sums(), c.climate_sums(), c.utc()))
        c.close()
        for state, cv, mo, (_, m3, m2), _ in out:
            for a in state + [cv.count, cv.levels, mo.precip, mo.evap, m3, m2]:
                a.setflags(write=False)
        _all_phases_cache[dtype] = out
    return _all_phases_cache[dtype]


def _assert_all_phases(c, want, nsteps, what):
    """the handle against one record of _all_phases_reference: state and ground temperature, both phases' sums with nsteps
    and seconds, the climatology's sums and sample count (one per step), the clock"""
    state, cv, mo, (nsamples, m3, m2), utc = want
    assert_same(final(c, close=False), state, what)
    assert_same_sums(c.convect_sums(), cv, what)
    got = c.moist_sums()
    assert (got.nsteps, got.seconds) == (mo.nsteps, mo.seconds), (what, got[:2], mo[:2])
    assert np.array_equal(got.precip, mo.precip) and np.array_equal(got.evap, mo.evap), what
    gn, g3, g2 = c.climate_sums()
    assert gn == nsamples == nsteps and np.array_equal(g3, m3) and np.array_equal(g2, m2), what
    assert c.utc() == utc == UTC0 + nsteps * DTS, (what, c.utc(), utc)


@pytest.mark.parametrize("comm_stream,host_loop", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_all_phases_on_a_band_equal_the_single_domain(dtype, comm_stream, host_loop, monkeypatch):
    """gcm_band_run with the solar step, the Held-Suarez forcing, the convective adjustment, the moist physics and the
    climatology all registered: the default orchestration forces the ghost rows apart on the second stream, behind the
    corrector's unpack (pe_ghost_row_phases); GCM_BAND_COMM_STREAM=1 takes them with the own rows on the compute stream;
    GCM_BAND_HOST_LOOP=1 drives the exchange from the host and ends every step with gcm_end_step.  Every way the band
    holds the single domain's bits: state and ground temperature, both phases' sums, the climatology, the clock"""
    import torch
    import gcmiipy_amd as g
    for k in su.ORCH_ENV:
        monkeypatch.delenv(k, raising=False)
    if comm_stream:
        monkeypatch.setenv("GCM_BAND_COMM_STREAM", "1")
    if host_loop:
        monkeypatch.setenv("GCM_BAND_HOST_LOOP", "1")
    steps = (2, 1)
    want = _all_phases_reference(g, dtype, steps)
    assert want[-1][1].count.any() and want[-1][2].precip.max() > 0
    geom = geom_of(BAND)
    c, eng, runner = su.loopback_band(g, torch, geom, dtype=dtype, gt=inp.ground(BAND[1], BAND[2]))
    assert runner.native == (not host_loop)
    _register_all(eng, geom)
    c.set_state(*wet_state(geom, dtype))
    for part, n in enumerate(steps):
        runner.run(n, DTS)
        torch.cuda.synchronize()
        _assert_all_phases(c, want[part], sum(steps[:part + 1]), (comm_stream, host_loop, part))
    c.close()


# ---------------------------------------------------------------- 2: the end of a step on its own (gcm_end_step)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_half_steps_and_end_step_are_a_step(dtype):
    """half_step(0), half_step(1), end_step(dt), three times, against step(3, dt) with every phase registered"""
    import gcmiipy_amd as g
    want = _all_phases_reference(g, dtype, (2, 1))[-1]
    geom = geom_of(BAND)
    c = handle(g, geom, wet_state(geom, dtype), dtype, gt=inp.ground(BAND[1], BAND[2]))
    _register_all(c, geom)
    for _ in range(3):
        c.half_step(0, DTS)
        c.half_step(1, DTS)
        c.end_step(DTS)
    _assert_all_phases(c, want, 3, "composed")
    # a refused dt changes nothing
    with pytest.raises(ValueError, match="gcm_end_step: dt must be finite"):
        c.end_step(float("nan"))
    assert g._lib.lib.gcm_end_step(c._h, float("inf")) == g._lib.ERR_ARG
    _assert_all_phases(c, want, 3, "refused")
    c.close()


def test_end_step_with_nothing_registered_and_on_other_models():
    import gcmiipy_amd as g
    geom = geom_of(BAND)
    c = handle(g, geom, wet_state(geom), gt=inp.ground(BAND[1], BAND[2]))
    was = final(c, close=False)
    c.end_step(DTS)
    assert_same(final(c), was, "nothing registered")
    assert g._lib.lib.gcm_end_step(None, DTS) == g._lib.ERR_ARG
    s = g.Core(g._lib.SW2D, 32, 16, dx=1e5)
    assert g._lib.lib.gcm_end_step(s._h, DTS) == g._lib.ERR_UNSUPPORTED
    with pytest.raises(g.GcmError, match="gcm_end_step: GCM_PE25D only"):
        s.end_step(DTS)
    s.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nb", [2, 3])
def test_in_process_bands_end_their_steps_as_the_single_domain(nb, dtype):
    """whole stages, two exchanges per step, then end_step on every band with every phase registered: own rows and ghost
    rows, no third exchange.  The merged state, sums (seconds included) and climatology are the single domain's"""
    import torch
    import gcmiipy_amd as g
    from gcmiipy_amd.bands import merge_climate, merge_convect, merge_moist
    steps = (2, 1)
    want = _all_phases_reference(g, dtype, steps)
    geom = geom_of(BAND)
    cores = su.bands(g, geom, nb, wet_state(geom, dtype), dtype=dtype, gt=inp.ground(BAND[1], BAND[2]))
    for c in cores:
        _register_all(c, geom)
    for part, n in enumerate(steps):
        state, cv, mo, (nsamples, m3, m2), utc = want[part]
        su.whole_steps(cores, torch, n, DTS, prime=part == 0, after=lambda k: [c.end_step(DTS) for c in cores])
        parts = [final(c, close=False) for c in cores]
        got = [np.concatenate([x[f] for x in parts], axis=1 if 0 < f < 5 else 0) for f in range(6)]
        assert_same(got, state, (nb, part))
        assert_same_sums(merge_convect([c.convect_sums() for c in cores]), cv, (nb, part))
        moist = merge_moist([c.moist_sums() for c in cores])
        assert (moist.nsteps, moist.seconds) == (mo.nsteps, mo.seconds), (nb, part)
        assert np.array_equal(moist.precip, mo.precip) and np.array_equal(moist.evap, mo.evap), (nb, part)
        merged, whole = merge_climate([c.climate() for c in cores]), g.Climate.from_sums(nsamples, m3, m2, BAND[2])
        assert merged.n == nsamples == sum(steps[:part + 1])
        for f, a, b in zip(g.Climate._fields[1:], merged[1:], whole[1:]):
            assert np.array_equal(a, b), (nb, part, f)
        assert all(c.utc() == utc for c in cores)
    for c in cores:
        c.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_native_and_host_driven_steps_share_one_clock_and_one_counter(dtype, monkeypatch):
    """the loopback band with the solar step and a climatology of every second step: run(2) (gcm_band_run), two
    host-driven step()s (each ends with gcm_end_step), run(1), against the single domain after 5 steps.  The handle's clock
    and its step counter serve both drivers: the solar step sees the right hour angle in every step and the samples fall on
    steps 2 and 4"""
    import torch
    import gcmiipy_amd as g
    for k in su.ORCH_ENV:
        monkeypatch.delenv(k, raising=False)
    geom = geom_of(BAND)
    st, gt = wet_state(geom, dtype), inp.ground(BAND[1], BAND[2])
    one = handle(g, geom, st, dtype, gt=gt, phys=True, every=2)
    one.step(5, DTS)
    want, want_clim, want_utc = final(one, close=False), one.climate_sums(), one.utc()
    one.close()
    c, eng, runner = su.loopback_band(g, torch, geom, dtype=dtype, gt=gt, phys=True, every=2)
    assert runner.native
    c.set_state(*st)
    runner.run(2, DTS)
    runner.step(DTS)
    runner.step(DTS)
    runner.run(1, DTS)
    torch.cuda.synchronize()
    assert_same(final(c, close=False), want, "mixed drivers")
    assert c.utc() == want_utc == UTC0 + 5 * DTS
    n, m3, m2 = c.climate_sums()
    assert n == want_clim[0] == 2 and np.array_equal(m3, want_clim[1]) and np.array_equal(m2, want_clim[2])
    c.close()
