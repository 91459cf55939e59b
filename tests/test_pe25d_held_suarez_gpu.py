"""The Held-Suarez forcing of GCM_PE25D on the device (gcm_set_held_suarez, gcm_held_suarez_step) against the NumPy
restatement tests/pe25d_held_suarez_ref.py, and the registered phase against the explicit call, on single domains and on
latitude bands (in-process bands with device-copied ghost rows, the loopback band of gcm_band_run), under every
orchestration of the band loop at a size where the streams really overlap.  u and v are one float64 product with the
routine's own table, rounded once: bit for bit.  theta goes through the device's Exner routine and log: 1e-10 relative
(the project's parity bound) in fp64, one rounding of float32 (2^-23 relative) in fp32."""
import numpy as np
import pytest

import gpu_setups as su
import pe25d_held_suarez_ref as ref
import pe25d_inputs as inp
from column_phase_cases import assert_same, final

pytestmark = pytest.mark.gpu

SHAPES = ((24, 36, 9), (6, 10, 3))                       # (H, W, L) of the tracer tests
PTOP = 1000.0
UTC0 = inp.UTC0
DT = 120.0
ORCH_ENV = ("GCM_PE_SINGLE_STREAM", "GCM_BAND_COMM_STREAM", "GCM_BAND_OVERLAP", "GCM_PE_STOP_EVENTS", "GCM_PE_K1_SPLIT")


def geom_of(H, W, L, ptop=0.0):
    geom = su.geom_of(H, W, L, ptop)
    r = ref.r_of(geom.sig, ref.DEFAULTS["sigma_b"])
    assert (r > 0).any() and (r == 0).any(), "the geometry needs a friction level and a free level"
    return geom


def sig_lat(geom):
    return np.asarray(geom.sig, dtype=np.float64).reshape(-1), np.asarray(geom.lat, dtype=np.float64).reshape(-1)


# ---------------------------------------------------------------- 1: the kernel against the restatement
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ptop", [0.0, PTOP])
@pytest.mark.parametrize("shape", SHAPES)
def test_step_equals_the_restatement(shape, ptop, dtype):
    import gcmiipy_amd as g
    H, W, L = shape
    geom = geom_of(H, W, L, ptop)
    sig, lat = sig_lat(geom)
    st = inp.state_of(geom, dtype)
    trs = inp.tracers(H, W, L, 2)
    gt = inp.ground(H, W)
    for over in ({}, dict(sigma_b=0.45, k_f=4e-5, T_min=240.0)):
        c = su.single(g, geom, st, dtype=dtype, gt=gt)
        c.set_tracers(trs)
        trs0 = c.get_tracers()
        c.held_suarez_step(geom, DT, **over)
        p, u, v, t, q = c.get_state()
        un, vn, tn = ref.step(st[0], st[1], st[2], st[3], sig, ptop, lat, DT, dtype=dtype, **over)
        assert np.array_equal(u, un) and np.array_equal(v, vn)
        err = np.max(np.abs(t - tn) / np.abs(tn))
        print("theta rel err", shape, ptop, dtype, err)
        assert err <= (1e-10 if dtype == "f64" else 2.0 ** -23), err
        free = ref.r_of(sig, ref.params(**over)["sigma_b"]) == 0
        assert free.any() and not free.all()
        assert np.array_equal(u[free], st[1][free]) and np.array_equal(v[free], st[2][free])
        assert not np.array_equal(u[~free], st[1][~free]) and not np.array_equal(t, st[3])
        assert np.array_equal(p, st[0]) and np.array_equal(q, st[4])
        assert np.array_equal(c.get_tracers(), trs0) and np.array_equal(c.get_ground(), gt)
        assert c.held_suarez is None                      # (an explicit step registers nothing)
        c.close()


# ---------------------------------------------------------------- 2: registered against explicit
@pytest.mark.parametrize("phys", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_registered_equals_explicit(dtype, phys):
    """step(1) + [solar_step] + held_suarez_step, five times, against set_held_suarez + step(5): the order of the phases
    is Matsuno step, solar step, Held-Suarez"""
    import gcmiipy_amd as g
    H, W, L = SHAPES[0]
    geom = geom_of(H, W, L)
    st, gt = inp.state_of(geom, dtype), inp.ground(H, W)
    a = su.single(g, geom, st, dtype=dtype, gt=gt)
    for n in range(5):
        a.step(1, DT)
        if phys:
            a.solar_step(geom, DT, UTC0 + n * DT)
        a.held_suarez_step(geom, DT)
    want = final(a)
    b = su.single(g, geom, st, dtype=dtype, gt=gt, phys=phys, hs={})
    assert b.held_suarez == ref.DEFAULTS
    b.step(5, DT)
    assert_same(final(b, close=False), want, "registered")
    # the forcing is not the identity, and the other order of the phases gives other bits
    plain = su.single(g, geom, st, dtype=dtype, gt=gt, phys=phys)
    plain.step(5, DT)
    assert not np.array_equal(final(plain)[1], want[1])
    if phys:
        o = su.single(g, geom, st, dtype=dtype, gt=gt)
        for n in range(5):
            o.step(1, DT)
            o.held_suarez_step(geom, DT)
            o.solar_step(geom, DT, UTC0 + n * DT)
        assert not np.array_equal(final(o)[3], want[3])
    # switched off: the next steps are an unregistered handle's
    b.set_held_suarez(None)
    assert b.held_suarez is None
    b.step(2, DT)
    u = su.single(g, geom, want[:5], dtype=dtype, gt=want[5])
    if phys:
        u.set_physics(geom, UTC0 + 5 * DT)
    u.step(2, DT)
    assert_same(final(b), final(u), "switched off")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_half_step_is_never_forced(dtype):
    import gcmiipy_amd as g
    H, W, L = SHAPES[0]
    geom = geom_of(H, W, L)
    st = inp.state_of(geom, dtype)
    r, u = su.single(g, geom, st, dtype=dtype, hs={}), su.single(g, geom, st, dtype=dtype)
    for c in (r, u):
        c.half_step(0, DT)
    star_r, star_u = r.get_star(), u.get_star()
    for k in range(4):
        assert np.array_equal(star_r[k], star_u[k]), k
    for c in (r, u):
        c.half_step(1, DT)
    assert_same(final(r), final(u), "half steps")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_tables_follow_a_change_of_dt(dtype):
    import gcmiipy_amd as g
    H, W, L = SHAPES[1]
    geom = geom_of(H, W, L)
    st = inp.state_of(geom, dtype)
    a = su.single(g, geom, st, dtype=dtype)
    for dt in (DT, DT, 45.0, 45.0, DT):
        a.step(1, dt)
        a.held_suarez_step(geom, dt)
    b = su.single(g, geom, st, dtype=dtype, hs={})
    b.step(2, DT)
    b.step(2, 45.0)
    b.step(1, DT)
    assert_same(final(b), final(a), "dt")


def test_refused_calls_change_nothing():
    import gcmiipy_amd as g
    H, W, L = SHAPES[1]
    geom = geom_of(H, W, L)
    st = inp.state_of(geom)
    c = su.single(g, geom, st, hs=dict(k_f=2e-5))
    was = c.held_suarez
    nan = float("nan")
    for over in (dict(k_f=-1.0), dict(k_a=-1.0), dict(k_s=-1.0), dict(sigma_b=1.0), dict(sigma_b=-0.1), dict(T_0=nan),
                 dict(dT_y=float("inf")), dict(k_f=nan)):
        with pytest.raises(ValueError):
            c.set_held_suarez(geom, **over)
        with pytest.raises(ValueError):
            c.held_suarez_step(geom, DT, **over)
    with pytest.raises(ValueError):
        c.set_held_suarez(np.zeros(H + 1))                # (the latitudes cover the global height)
    with pytest.raises(ValueError):
        c.set_held_suarez(geom, k_x=1.0)
    assert c.held_suarez == was and g._lib.lib.gcm_held_suarez_on(c._h) == 1
    assert g._lib.lib.gcm_set_held_suarez(c._h, None) == g._lib.OK and g._lib.lib.gcm_held_suarez_on(c._h) == 0
    rec = g._lib.HeldSuarez(*ref.DEFAULTS.values())       # lat = NULL
    assert g._lib.lib.gcm_set_held_suarez(c._h, rec) == g._lib.ERR_ARG and g._lib.lib.gcm_held_suarez_on(c._h) == 0
    c.set_held_suarez(geom, k_f=2e-5)
    c.step(2, DT)
    w = su.single(g, geom, st, hs=dict(k_f=2e-5))
    w.step(2, DT)
    assert_same(final(c), final(w), "after refused calls")
    # other models
    s = g.Core(g._lib.SW2D, 32, 16, dx=1e5)
    lat = np.zeros(16)
    rec.lat = lat.ctypes.data_as(g._lib._dp)
    assert g._lib.lib.gcm_set_held_suarez(s._h, rec) == g._lib.ERR_UNSUPPORTED
    assert g._lib.lib.gcm_held_suarez_step(s._h, 60.0, rec) == g._lib.ERR_UNSUPPORTED
    assert g._lib.lib.gcm_held_suarez_on(s._h) == 0
    s.close()


# ---------------------------------------------------------------- 3: bands equal the single domain
_single_cache = {}


def _single_reference(g, shape, dtype, phys, steps):
    """the single domain's state after steps[0] and after steps[0] + steps[1] steps, computed once per case"""
    key = (shape, dtype, phys, steps)
    if key not in _single_cache:
        geom = geom_of(*shape)
        c = su.single(g, geom, inp.state_of(geom, dtype), dtype=dtype, gt=inp.ground(shape[0], shape[1]), phys=phys,
                      hs={})
        c.step(steps[0], DT)
        first = final(c, close=False)
        c.step(steps[1], DT)
        _single_cache[key] = (first, final(c))
        for part in _single_cache[key]:
            for a in part:
                a.setflags(write=False)
    return _single_cache[key]


@pytest.mark.parametrize("phys", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,nb", [(SHAPES[0], 2), (SHAPES[0], 3), (SHAPES[1], 2)])
def test_in_process_bands_equal_single_domain(shape, nb, dtype, phys):
    """whole stages, two exchanges per step (the order of gcm_band_run), then the physics phases by the explicit calls on
    own rows and ghost rows: the ghost rows are forced locally, no third exchange"""
    import torch
    import gcmiipy_amd as g
    H, W, L = shape
    steps = (3, 2)
    want = _single_reference(g, shape, dtype, phys, steps)
    geom = geom_of(H, W, L)
    cores = su.bands(g, geom, nb, inp.state_of(geom, dtype), dtype=dtype, gt=inp.ground(H, W))
    done = 0

    def physics(k):
        for c in cores:
            if phys:
                c.solar_step(geom, DT, UTC0 + (done + k) * DT)
            c.held_suarez_step(geom, DT)
    for part, n in enumerate(steps):
        su.whole_steps(cores, torch, n, DT, prime=part == 0, after=physics)
        done += n
        parts = [c.get_state() + [c.get_ground()] for c in cores]
        got = [np.concatenate([x[f] for x in parts], axis=0 if f in (0, 5) else 1) for f in range(6)]
        assert_same(got, want[part], (nb, part))
    for c in cores:
        c.close()


@pytest.mark.parametrize("phys", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_loopback_band_run_equals_single_domain(shape, dtype, phys):
    """gcm_band_run with the forcing registered: several steps in one run, then a second run after a get_state"""
    import torch
    import gcmiipy_amd as g
    H, W, L = shape
    steps = (3, 2)
    want = _single_reference(g, shape, dtype, phys, steps)
    geom = geom_of(H, W, L)
    c, eng, runner = su.loopback_band(g, torch, geom, dtype=dtype, phys=phys, hs={})
    assert runner.native
    c.set_state(*inp.state_of(geom, dtype))
    c.set_ground(inp.ground(H, W))
    for part, n in enumerate(steps):
        runner.run(n, DT)
        torch.cuda.synchronize()
        assert_same(final(c, close=False), want[part], part)
    c.close()


# ---------------------------------------------------------------- 4: the chains
@pytest.mark.parametrize("phys", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_band_run_chains_with_the_forcing(dtype, phys, monkeypatch):
    """the grid of test_band_run_chains_at_overlapping_size (48 x 1440 x 24: kernels of tens of microseconds on either
    stream).  The forcing writes u and v, which the next stage's second-stream launches read: with the fork at the last
    K4 left valid they would race it.  Every orchestration of the band loop gives the single domain's bits after 4
    steps, and the single domain's step(4) equals four rounds of step(1) + sync()"""
    import torch
    import gcmiipy_amd as g
    H, W, L, dt, steps = 48, 1440, 24, 1.0, 4
    hs = dict(k_f=0.05, k_a=0.01, k_s=0.04)                # (a forcing that moves every bit in a step of one second)
    geom = geom_of(H, W, L)
    st, gt = inp.state_of(geom, dtype), inp.ground(H, W)
    for k in ORCH_ENV:
        monkeypatch.delenv(k, raising=False)
    ref_c = su.single(g, geom, st, dtype=dtype, gt=gt, phys=phys, hs=hs)
    ref_c.step(steps, dt)
    want = final(ref_c)
    one = su.single(g, geom, st, dtype=dtype, gt=gt, phys=phys, hs=hs)
    for _ in range(steps):
        one.step(1, dt)
        one.sync()
    assert_same(final(one), want, "step(1) + sync")
    plain = su.single(g, geom, st, dtype=dtype, gt=gt, phys=phys)
    plain.step(steps, dt)
    assert not np.array_equal(final(plain)[1], want[1])
    for env in ({}, {"GCM_PE_SINGLE_STREAM": "1"}, {"GCM_BAND_COMM_STREAM": "1"}, {"GCM_BAND_OVERLAP": "1"},
                {"GCM_PE_STOP_EVENTS": "0"}, {"GCM_PE_K1_SPLIT": "0"}, {"overlap_call": "1"},
                {"GCM_PE_STOP_EVENTS": "0", "GCM_BAND_COMM_STREAM": "1"}):
        for k in ORCH_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            if k in ORCH_ENV:
                monkeypatch.setenv(k, v)
        c, eng, runner = su.loopback_band(g, torch, geom, dtype=dtype, phys=phys, hs=hs)
        assert runner.native
        if "overlap_call" in env:
            c.set_band_overlap(1)
        c.set_state(*st)
        c.set_ground(gt)
        runner.run(steps, dt)
        torch.cuda.synchronize()
        assert_same(final(c), want, env)


# ---------------------------------------------------------------- 5: physical properties
def test_physical_properties():
    import gcmiipy_amd as g
    H, W, L = SHAPES[0]
    geom = geom_of(H, W, L)
    sig, lat = sig_lat(geom)
    st = inp.state_of(geom)
    c = su.single(g, geom, st)
    ke0 = c.energy(np.ones(1))[0]
    c.held_suarez_step(geom, 3600.0)
    ke1 = c.energy(np.ones(1))[0]
    assert ke1 < ke0, (ke0, ke1)
    te = ref.theta_eq(st[0], sig, 0.0, lat)
    gap = [np.max(np.abs(st[3] - te))]
    for _ in range(6):
        c.held_suarez_step(geom, 10 * 86400.0)
        gap.append(np.max(np.abs(c.get_state((3,))[3] - te)))
    assert all(b < a for a, b in zip(gap, gap[1:])), gap
    assert gap[-1] < 0.5 * gap[0]
    c.set_state(*st)
    c.held_suarez_step(geom, 3600.0, k_f=0.0, k_a=0.0, k_s=0.0)
    assert_same(final(c), st, "identity")


def test_long_run_stays_finite():
    import gcmiipy_amd as g
    H, W, L = SHAPES[0]
    geom = geom_of(H, W, L)
    c = su.single(g, geom, inp.state_of(geom, wind=1.0), hs={})
    c.step(200, DT)
    s = c.stats(np.ones(1))
    c.close()
    assert s["nans"] == 0, s


# ---------------------------------------------------------------- 6: checkpoint
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_checkpoint_carries_the_forcing(dtype, tmp_path):
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    H, W, L = SHAPES[0]
    geom = geom_of(H, W, L)
    st = inp.state_of(geom, dtype)
    hs = dict(k_f=3e-5, sigma_b=0.6)
    whole = su.single(g, geom, st, dtype=dtype, hs=hs)
    whole.step(5, DT)
    want = final(whole)
    a = su.single(g, geom, st, dtype=dtype, hs=hs)
    a.step(3, DT)
    path = str(tmp_path / "hs.npz")
    checkpoint.save(path, a, step=3, geom=geom)
    a.close()
    b, ck = checkpoint.restore(path)
    assert b.held_suarez == ref.params(**hs) and ck["held_suarez"][0] == ref.params(**hs)
    b.step(2, DT)
    assert_same(final(b), want, "restored")
    # a file without the key restores with none
    plain = su.single(g, geom, st, dtype=dtype)
    checkpoint.save(path, plain, geom=geom)
    plain.close()
    c, ck = checkpoint.restore(path)
    assert ck["held_suarez"] is None and c.held_suarez is None
    c.close()
