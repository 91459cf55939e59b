"""The convective adjustment of GCM_PE25D on the device (gcm_set_convect, gcm_convect_step) against the NumPy restatement
tests/pe25d_convect_ref.py, its conservation properties on the device, the registered phase against the explicit call
(alone and between the Held-Suarez forcing and the moist physics), latitude bands against the single domain (in-process
bands with device-copied ghost rows, the loopback band of gcm_band_run under its orchestrations, once at a size where the
streams really overlap), the end of a step by gcm_end_step with every phase registered (a single domain's half steps, the
host-driven band, in-process bands, native and host-driven steps mixed on one runner), refused calls and the checkpoint.  theta goes through the device's Exner routine, exp and log:
1e-10 relative to the field's maximum (the project's parity bound) for either storage type; the decisions do not depend
on those last bits (tests/test_pe25d_convect_cpu.py holds the inputs 1e-9 clear of a tie), so the set of changed cells
and the counts are the restatement's exactly."""
import numpy as np
import pytest

import gpu_setups as su
import pe25d_inputs as inp
import pe25d_convect_ref as ref
import pe25d_moist_ref as mref

pytestmark = pytest.mark.gpu

DTS = 120.0                                              # the dynamics' dt
UTC0 = inp.UTC0
GAMMA = ref.GAMMA
KC = ref.kappa_of(GAMMA)
STEP = (9, 24, 36)                                       # (L, H, W) of the tests that take dynamics steps
BAND = (9, 12, 36)                                       # H = 12: 2 and 3 bands
TOL = 1e-10


def geom_of(shape, ptop=0.0):
    L, H, W = shape
    return su.geom_of(H, W, L, ptop)


def handle(g, geom, st, dtype="f64", **kw):
    """a single-domain handle; the kernel tests' shapes are never stepped and take no filter plan"""
    stepped = (geom.layers, geom.height, geom.width) in (STEP, BAND) or geom.width == 1440
    return su.single(g, geom, st, dtype=dtype, filter=stepped, **kw)


def final(c, close=True):
    out = c.get_state() + ([c.get_ground()] if c.has_ground else [])
    if close:
        c.close()
    return out


def assert_same(got, want, what=""):
    assert len(got) == len(want)
    for k, a, b in zip("puvtqg", got, want):
        assert np.array_equal(a, b), (what, k, float(np.max(np.abs(a - b))))


def assert_same_sums(got, want, what="", seconds=None):
    """seconds: what the record must hold where that is not want's (explicit calls add none)"""
    assert got.nsteps == want.nsteps and got.seconds == (want.seconds if seconds is None else seconds), (what, got[:2], want[:2])
    assert np.array_equal(got.count, want.count), (what, "count", float(np.max(np.abs(got.count - want.count))))
    assert np.array_equal(got.levels, want.levels), (what, "levels")


def linf(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def wet_state(geom, dtype="f64"):
    """the unstable state with q set around saturation (the recipe of pe25d_moist_ref.humid_state on this theta), so
    that the moist physics behind the adjustment has something to condense"""
    p, u, v, t, q = ref.unstable_state(geom)
    rh = 0.3 + 1.1 * np.random.default_rng(21).random(q.shape)
    p_lev, pi = mref.levels(p, geom.sig, geom.ptop)
    _, qs, _, can = mref.saturation(t * pi, p_lev)
    q = np.where(can, np.minimum(rh * qs, 0.5), 0.02)
    st = [p, u, v, t, q]
    if dtype == "f32":
        st = [a.astype(np.float32).astype(np.float64) for a in st]
    return st


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


def test_explicit_step_without_a_registration_keeps_no_sums():
    import gcmiipy_amd as g
    geom = geom_of(ref.SHAPES[0])
    st = ref.unstable_state(geom)
    a, b = handle(g, geom, st), handle(g, geom, st)
    a.convect_step(gamma=GAMMA)
    assert a.convect is None and not a.convect_registered
    with pytest.raises(g.GcmError):
        a.convect_sums()
    b.set_convect(gamma=GAMMA)
    b.convect_step(gamma=GAMMA)
    assert b.convect_sums().count.any()
    assert_same(final(a), final(b), "with and without sums")


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


# ---------------------------------------------------------------- 3: bands equal the single domain
_single_cache = {}
PAR = dict(gamma=GAMMA)


def _single_reference(g, shape, dtype, steps, dt=DTS, par=PAR):
    """the single domain's state and sums after steps[0] and after steps[0] + steps[1] steps, computed once per case"""
    key = (shape, dtype, steps, dt)
    if key not in _single_cache:
        geom = geom_of(shape)
        c = handle(g, geom, ref.unstable_state(geom, KC, dtype), dtype)
        c.set_convect(**par)
        out = []
        for n in steps:
            c.step(n, dt)
            out.append((final(c, close=False), c.convect_sums()))
        c.close()
        for state, sums in out:
            for a in state + [sums.count, sums.levels]:
                a.setflags(write=False)
        _single_cache[key] = out
    return _single_cache[key]


def _bands(g, geom, nb, st, dtype):
    """nb in-process bands with their own rows of the state (the way gpu_setups.bands builds them), the phase registered"""
    from gcmiipy_amd.bands import split_rows
    H, W, L = geom.height, geom.width, geom.layers
    cores = []
    for r, (row0, n) in enumerate(split_rows(H, nb)):
        c = g.Core(g._lib.PE25D, W, n, L, geom=geom, nranks=nb, rank=r, global_height=H, row0=row0, dtype=dtype)
        assert c.halo_bytes() == inp.halo_bytes(W, L, 8 if dtype == "f64" else 4, 0, 1)
        c.set_state(*[inp.rows(a, slice(row0, row0 + n)) for a in st])
        c.set_convect(**PAR)
        cores.append(c)
    return cores


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nb", [2, 3])
def test_in_process_bands_equal_single_domain(nb, dtype):
    """whole stages, two exchanges per step (the order of gcm_band_run), then the phase by the explicit call on own rows
    and ghost rows: the ghost rows are adjusted locally, no third exchange, and add to no sum.  The second part steps on
    from those ghost rows: they hold the neighbour's bits"""
    import torch
    import gcmiipy_amd as g
    from gcmiipy_amd.bands import merge_convect
    steps = (2, 1)
    want = _single_reference(g, BAND, dtype, steps)
    geom = geom_of(BAND)
    cores = _bands(g, geom, nb, ref.unstable_state(geom, KC, dtype), dtype)

    def physics(k):
        for c in cores:
            c.convect_step(**PAR)
    for part, n in enumerate(steps):
        su.whole_steps(cores, torch, n, DTS, prime=part == 0, after=physics)
        parts = [c.get_state() for c in cores]
        got = [np.concatenate([x[f] for x in parts], axis=0 if f == 0 else 1) for f in range(5)]
        assert_same(got, want[part][0], (nb, part))
        assert want[part][1].count.any()
        assert_same_sums(merge_convect([c.convect_sums() for c in cores]), want[part][1], (nb, part), seconds=0.0)
    for c in cores:
        c.close()


@pytest.mark.parametrize("host_loop", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_loopback_band_run_equals_single_domain(dtype, host_loop, monkeypatch):
    """gcm_band_run with the phase registered (and the host-driven sequence, GCM_BAND_HOST_LOOP=1, whose physics_step
    ends the step with gcm_end_step: the same sums, seconds included): several steps in one run, then a second run after
    a get_state"""
    import torch
    import gcmiipy_amd as g
    for k in su.ORCH_ENV:
        monkeypatch.delenv(k, raising=False)
    if host_loop:
        monkeypatch.setenv("GCM_BAND_HOST_LOOP", "1")
    steps = (2, 1)
    want = _single_reference(g, BAND, dtype, steps)
    geom = geom_of(BAND)
    c, eng, runner = su.loopback_band(g, torch, geom, dtype=dtype)
    assert runner.native == (not host_loop)
    eng.set_convect(**PAR)
    assert c.halo_bytes() == inp.halo_bytes(BAND[2], BAND[0], 8 if dtype == "f64" else 4, 0, 1)
    c.set_state(*ref.unstable_state(geom, KC, dtype))
    for part, n in enumerate(steps):
        runner.run(n, DTS)
        torch.cuda.synchronize()
        assert_same(final(c, close=False), want[part][0], part)
        assert_same_sums(c.convect_sums(), want[part][1], part)
    c.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_band_run_chains_with_the_phase(dtype, monkeypatch):
    """the grid of test_band_run_chains_at_overlapping_size (48 x 1440 x 24: kernels of tens of microseconds on either
    stream), 2 steps.  The launch keeps the fork at the last K4: the default orchestration, one stream
    (GCM_PE_SINGLE_STREAM=1) and the exchange on the comm stream (GCM_BAND_COMM_STREAM=1) all give the single domain's
    bits, state and sums"""
    import torch
    import gcmiipy_amd as g
    shape, dt, steps = (24, 48, 1440), 1.0, 2
    geom = geom_of(shape)
    st = ref.unstable_state(geom, KC, dtype)
    for k in su.ORCH_ENV:
        monkeypatch.delenv(k, raising=False)
    one = handle(g, geom, st, dtype)
    one.set_convect(**PAR)
    one.step(steps, dt)
    want, want_sums = final(one, close=False), one.convect_sums()
    one.close()
    assert 0.5 < want_sums.count.mean() / steps < 1.0 and want_sums.levels.max() >= 4
    for env in ({}, {"GCM_PE_SINGLE_STREAM": "1"}, {"GCM_BAND_COMM_STREAM": "1"}):
        for k in su.ORCH_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c, eng, runner = su.loopback_band(g, torch, geom, dtype=dtype)
        assert runner.native
        eng.set_convect(**PAR)
        c.set_state(*st)
        runner.run(steps, dt)
        torch.cuda.synchronize()
        assert_same(final(c, close=False), want, env)
        assert_same_sums(c.convect_sums(), want_sums, env)
        c.close()


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


# ---------------------------------------------------------------- 3b: the end of a step on its own (gcm_end_step)
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


# ---------------------------------------------------------------- 4: refused calls
def test_refused_calls_change_nothing():
    import ctypes
    import gcmiipy_amd as g
    lib, L_ = g._lib.lib, g._lib
    shape = ref.SHAPES[1]
    geom = geom_of(shape)
    st = ref.unstable_state(geom)
    c = handle(g, geom, st)
    with pytest.raises(g.GcmError):
        c.convect_sums()                                  # GCM_ERR_STATE
    assert lib.gcm_get_convect(c._h, None, None, None, None) == L_.ERR_STATE
    assert lib.gcm_convect_reset(c._h) == L_.ERR_STATE
    z = np.zeros((shape[1], shape[2]))
    assert lib.gcm_put_convect(c._h, z.ctypes.data_as(L_._dp), z.ctypes.data_as(L_._dp), 0.0, 0) == L_.ERR_STATE   # put before set
    assert lib.gcm_convect_on(c._h) == 0
    c.set_convect(gamma=GAMMA)
    c.convect_step(gamma=GAMMA)
    was, was_state = c.convect_sums(), c.get_state()
    assert was.count.any()
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
    with pytest.raises(ValueError):
        c.put_convect(-1, 0.0, was.count, was.levels)
    with pytest.raises(ValueError):
        c.put_convect(1, nan, was.count, was.levels)
    assert lib.gcm_put_convect(c._h, None, None, 0.0, 0) == L_.ERR_ARG
    assert c.convect == ref.params(kappa_c=KC) and lib.gcm_convect_on(c._h) == 1
    assert_same(c.get_state(), was_state, "state after refused calls")
    assert_same_sums(c.convect_sums(), was, "sums after refused calls")
    c.close()
    # other models
    s = g.Core(g._lib.SW2D, 32, 16, dx=1e5)
    rec = L_.Convect(0.0, 1)
    assert lib.gcm_set_convect(s._h, rec) == L_.ERR_UNSUPPORTED
    assert lib.gcm_convect_step(s._h, rec) == L_.ERR_UNSUPPORTED
    assert lib.gcm_get_convect(s._h, None, None, None, None) == L_.ERR_UNSUPPORTED
    assert lib.gcm_convect_reset(s._h) == L_.ERR_UNSUPPORTED
    assert lib.gcm_convect_on(s._h) == 0
    s.close()


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


# ---------------------------------------------------------------- 5: checkpoint
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_checkpoint_carries_the_phase_and_its_sums(dtype, tmp_path):
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    geom = geom_of(STEP)
    st = ref.unstable_state(geom, KC, dtype)
    par = dict(gamma=GAMMA, mix_q=0)
    whole = handle(g, geom, st, dtype)
    whole.set_convect(**par)
    whole.step(3, DTS)
    want, want_sums = final(whole, close=False), whole.convect_sums()
    whole.close()
    assert want_sums.count.any()
    a = handle(g, geom, st, dtype)
    a.set_convect(**par)
    a.step(2, DTS)
    path = str(tmp_path / "convect.npz")
    checkpoint.save(path, a, step=2, geom=geom)
    a.close()
    b, ck = checkpoint.restore(path)
    rec = ref.params(kappa_c=KC, mix_q=0)
    assert b.convect == rec and ck["convect"]["params"] == rec and ck["convect"]["n"] == 2
    assert ck["convect"]["seconds"] == 2 * DTS
    b.step(1, DTS)
    assert_same(final(b, close=False), want, "restored")
    assert_same_sums(b.convect_sums(), want_sums, "restored")
    b.close()
    # a file without the keys restores with none
    plain = handle(g, geom, st, dtype)
    checkpoint.save(path, plain, geom=geom)
    plain.close()
    c, ck = checkpoint.restore(path)
    assert ck["convect"] is None and c.convect is None
    c.close()
    # a phase registered through C alone is refused
    d = handle(g, geom, st, dtype)
    assert g._lib.lib.gcm_set_convect(d._h, g._lib.Convect(0.0, 1)) == g._lib.OK
    assert d.convect is None and d.convect_registered
    with pytest.raises(g.GcmError, match="gcm_set_convect"):
        checkpoint.save(path, d, geom=geom)
    d.close()
