"""The moist physics of GCM_PE25D on the device (gcm_set_moist, gcm_moist_step) against the NumPy restatement
tests/pe25d_moist_ref.py, its conservation properties on the device, the registered phase against the explicit call,
latitude bands against the single domain (in-process bands with device-copied ghost rows, the loopback band of
gcm_band_run under its orchestrations, once at a size where the streams really overlap), refused calls and the
checkpoint.  theta and q go through the device's Exner routine and exp: 1e-10 relative to the field's maximum (the
project's parity bound) in fp64, one rounding of float32 (2^-23) in fp32; the float64 sums 1e-10 for either."""
import numpy as np
import pytest

import gpu_setups as su
import pe25d_inputs as inp
import pe25d_moist_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = ref.SHAPES
DT = 600.0                                               # the explicit step's dt
DTS = 120.0                                              # the dynamics' dt
TAU = 86400.0
UTC0 = inp.UTC0


def geom_of(shape, ptop=0.0):
    return su.geom_of(*shape, ptop)


def handle(g, geom, st, dtype="f64", **kw):
    """a single-domain handle; the 300-column shape is never stepped and takes no filter plan"""
    return su.single(g, geom, st, dtype=dtype, filter=geom.width != 300, **kw)


def final(c, close=True):
    out = c.get_state() + ([c.get_ground()] if c.has_ground else [])
    if close:
        c.close()
    return out


def assert_same(got, want, what=""):
    assert len(got) == len(want)
    for k, a, b in zip("puvtqg", got, want):
        assert np.array_equal(a, b), (what, k, float(np.max(np.abs(a - b))))


def assert_same_sums(got, want, what=""):
    assert (got.nsteps, got.seconds) == (want.nsteps, want.seconds), what
    assert np.array_equal(got.precip, want.precip), (what, "precip", float(np.max(np.abs(got.precip - want.precip))))
    assert np.array_equal(got.evap, want.evap), (what, "evap")


def linf(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


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


def test_explicit_step_without_a_registration_keeps_no_sums():
    import gcmiipy_amd as g
    geom = geom_of(SHAPES[0])
    st = ref.humid_state(geom)
    a, b = handle(g, geom, st), handle(g, geom, st)
    a.moist_step(DT, tau_e=TAU)
    assert a.moist is None
    with pytest.raises(g.GcmError):
        a.moist_sums()
    b.set_moist(tau_e=TAU)
    b.moist_step(DT, tau_e=TAU)
    assert_same(final(a), final(b), "with and without sums")


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


# ---------------------------------------------------------------- 4: bands equal the single domain
_single_cache = {}
PAR = dict(tau_e=TAU)


def _single_reference(g, shape, dtype, steps, dt=DTS, par=PAR):
    """the single domain's state and sums after steps[0] and after steps[0] + steps[1] steps, computed once per case"""
    key = (shape, dtype, steps, dt)
    if key not in _single_cache:
        geom = geom_of(shape)
        c = handle(g, geom, ref.humid_state(geom, dtype), dtype)
        c.set_moist(**par)
        out = []
        for n in steps:
            c.step(n, dt)
            out.append((final(c, close=False), c.moist_sums()))
        c.close()
        for state, sums in out:
            for a in state + [sums.precip, sums.evap]:
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
        c.set_moist(**PAR)
        cores.append(c)
    return cores


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,nb", [(SHAPES[0], 2), (SHAPES[0], 3), (SHAPES[1], 2)])
def test_in_process_bands_equal_single_domain(shape, nb, dtype):
    """whole stages, two exchanges per step (the order of gcm_band_run), then the phase by the explicit call on own rows
    and ghost rows: the ghost rows are adjusted locally, no third exchange, and add to no sum"""
    import torch
    import gcmiipy_amd as g
    from gcmiipy_amd.bands import merge_moist
    steps = (2, 1)
    want = _single_reference(g, shape, dtype, steps)
    geom = geom_of(shape)
    cores = _bands(g, geom, nb, ref.humid_state(geom, dtype), dtype)

    def physics(k):
        for c in cores:
            c.moist_step(DTS, **PAR)
    for part, n in enumerate(steps):
        su.whole_steps(cores, torch, n, DTS, prime=part == 0, after=physics)
        parts = [c.get_state() for c in cores]
        got = [np.concatenate([x[f] for x in parts], axis=0 if f == 0 else 1) for f in range(5)]
        assert_same(got, want[part][0], (nb, part))
        assert_same_sums(merge_moist([c.moist_sums() for c in cores]), want[part][1], (nb, part))
    for c in cores:
        c.close()


@pytest.mark.parametrize("host_loop", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_loopback_band_run_equals_single_domain(shape, dtype, host_loop, monkeypatch):
    """gcm_band_run with the phase registered (and the host-driven sequence, GCM_BAND_HOST_LOOP=1, whose physics_step
    ends the step with gcm_end_step): several steps in one run, then a second run after a get_state"""
    import torch
    import gcmiipy_amd as g
    for k in su.ORCH_ENV:
        monkeypatch.delenv(k, raising=False)
    if host_loop:
        monkeypatch.setenv("GCM_BAND_HOST_LOOP", "1")
    steps = (2, 1)
    want = _single_reference(g, shape, dtype, steps)
    geom = geom_of(shape)
    c, eng, runner = su.loopback_band(g, torch, geom, dtype=dtype)
    assert runner.native == (not host_loop)
    eng.set_moist(**PAR)
    nbytes = c.halo_bytes()
    assert nbytes == inp.halo_bytes(shape[1], shape[2], 8 if dtype == "f64" else 4, 0, 1)
    c.set_state(*ref.humid_state(geom, dtype))
    for part, n in enumerate(steps):
        runner.run(n, DTS)
        torch.cuda.synchronize()
        assert_same(final(c, close=False), want[part][0], part)
        assert_same_sums(c.moist_sums(), want[part][1], part)
    c.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_band_run_chains_with_the_phase(dtype, monkeypatch):
    """the grid of test_band_run_chains_at_overlapping_size (48 x 1440 x 24: kernels of tens of microseconds on either
    stream), 2 steps.  The launch keeps the fork at the last K4: the default orchestration, one stream
    (GCM_PE_SINGLE_STREAM=1) and the exchange on the comm stream (GCM_BAND_COMM_STREAM=1) all give the single domain's
    bits, state and sums"""
    import torch
    import gcmiipy_amd as g
    shape, dt, steps = (48, 1440, 24), 1.0, 2
    par = dict(tau_e=600.0)                               # (a source that moves bits in a step of one second)
    geom = geom_of(shape)
    st = ref.humid_state(geom, dtype)
    for k in su.ORCH_ENV:
        monkeypatch.delenv(k, raising=False)
    one = handle(g, geom, st, dtype)
    one.set_moist(**par)
    one.step(steps, dt)
    want, want_sums = final(one, close=False), one.moist_sums()
    one.close()
    assert want_sums.precip.max() > 0 and want_sums.evap.max() > 0
    for env in ({}, {"GCM_PE_SINGLE_STREAM": "1"}, {"GCM_BAND_COMM_STREAM": "1"}):
        for k in su.ORCH_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c, eng, runner = su.loopback_band(g, torch, geom, dtype=dtype)
        assert runner.native
        eng.set_moist(**par)
        c.set_state(*st)
        runner.run(steps, dt)
        torch.cuda.synchronize()
        assert_same(final(c, close=False), want, env)
        assert_same_sums(c.moist_sums(), want_sums, env)
        c.close()


# ---------------------------------------------------------------- 5: refused calls
def test_refused_calls_change_nothing():
    import gcmiipy_amd as g
    lib, L_ = g._lib.lib, g._lib
    geom = geom_of(SHAPES[1])
    st = ref.humid_state(geom)
    c = handle(g, geom, st)
    with pytest.raises(g.GcmError):
        c.moist_sums()                                    # GCM_ERR_STATE
    assert lib.gcm_get_moist(c._h, None, None, None, None) == L_.ERR_STATE
    assert lib.gcm_moist_reset(c._h) == L_.ERR_STATE
    z = np.zeros((SHAPES[1][0], SHAPES[1][1]))
    assert lib.gcm_put_moist(c._h, z.ctypes.data_as(L_._dp), z.ctypes.data_as(L_._dp), 0.0, 0) == L_.ERR_STATE
    c.set_moist(tau_e=TAU)
    c.moist_step(DT, tau_e=TAU)
    was, was_state = c.moist_sums(), c.get_state()
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
    with pytest.raises(ValueError):
        c.put_moist(-1, 0.0, was.precip, was.evap)
    with pytest.raises(ValueError):
        c.put_moist(1, nan, was.precip, was.evap)
    assert lib.gcm_put_moist(c._h, None, None, 0.0, 0) == L_.ERR_ARG
    assert c.moist == ref.params(tau_e=TAU) and lib.gcm_moist_on(c._h) == 1
    assert_same(c.get_state(), was_state, "state after refused calls")
    assert_same_sums(c.moist_sums(), was, "sums after refused calls")
    c.close()
    # other models
    s = g.Core(g._lib.SW2D, 32, 16, dx=1e5)
    rec = L_.Moist(*ref.DEFAULTS.values())
    assert lib.gcm_set_moist(s._h, rec) == L_.ERR_UNSUPPORTED
    assert lib.gcm_moist_step(s._h, 60.0, rec) == L_.ERR_UNSUPPORTED
    assert lib.gcm_get_moist(s._h, None, None, None, None) == L_.ERR_UNSUPPORTED
    assert lib.gcm_moist_reset(s._h) == L_.ERR_UNSUPPORTED
    assert lib.gcm_moist_on(s._h) == 0
    s.close()


# ---------------------------------------------------------------- 6: checkpoint
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_checkpoint_carries_the_phase_and_its_sums(dtype, tmp_path):
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    geom = geom_of(SHAPES[0])
    st = ref.humid_state(geom, dtype)
    par = dict(tau_e=43200.0, rh_s=0.7)
    whole = handle(g, geom, st, dtype)
    whole.set_moist(**par)
    whole.step(3, DTS)
    want, want_sums = final(whole, close=False), whole.moist_sums()
    whole.close()
    a = handle(g, geom, st, dtype)
    a.set_moist(**par)
    a.step(2, DTS)
    path = str(tmp_path / "moist.npz")
    checkpoint.save(path, a, step=2, geom=geom)
    a.close()
    b, ck = checkpoint.restore(path)
    assert b.moist == ref.params(**par) and ck["moist"]["params"] == ref.params(**par) and ck["moist"]["n"] == 2
    b.step(1, DTS)
    assert_same(final(b, close=False), want, "restored")
    assert_same_sums(b.moist_sums(), want_sums, "restored")
    b.close()
    # a file without the keys restores with none
    plain = handle(g, geom, st, dtype)
    checkpoint.save(path, plain, geom=geom)
    plain.close()
    c, ck = checkpoint.restore(path)
    assert ck["moist"] is None and c.moist is None
    c.close()
