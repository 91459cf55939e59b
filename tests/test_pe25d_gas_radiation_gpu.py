"""The grey radiation of GCM_PE25D that absorbs by water vapour and CO2, on the device, held to the NumPy restatement
tests/pe25d_gas_radiation_ref.py (the reference's grey_radiation bit for bit: test_pe25d_gas_radiation_cpu.py) by the
rule written there: |got - want| <= 1e-10 of the level's maximum (dt_air) or the field's (dt_ground, olr, theta, the
ground temperature, the budget words); an fp32 handle adds 2^-23 |want| for what it stores in float32 (dt_air, theta)
and is fed inputs already rounded to float32.  The CPU test shows that this rule rejects every planted fault on these
very inputs.

Shapes: W = 72 (one full wave and a ragged one), H = 6, L = 12, 24 and 30 (the kernel has one form for every L), ptop = 0
and ptop != 0, fp64 and fp32; the cases that take dynamics steps: H = 8, L = 12.
 1. the diagnostic form over the six parameter sets of ref.CASES on one handle; "zenith": night columns carry no short
    wave at all (the results there are those of solar_constant = 0, bit for bit);
 2. gas_radiation_step against the restatement's advance; the closure identity on the device's diagnostic outputs;
 3. registered: step() equals, bit for bit, a twin's step() without physics followed by gas_radiation_step at the
    twin's clock; the clock advances by dt;
 4. off: registered and unregistered again, a handle steps to the bits of one that never registered (the grey scheme);
 5. with the slab ocean: the ground temperature is the slab's, the five words are the restatement's, night columns' SC
    and SW_SFC are exactly 0, and the top's and the surface's net gains close against the column's heating;
 6. bands: nranks = 2 over H = 8 under gcm_band_run, its host-driven loop and two in-process bands, with and without
    the slab ocean: state, ground temperature and clock bit for bit the single domain's after 3 steps;
 7. a checkpoint round trip keeps the parameters and the next step's bits;
 8. the refusals, on a handle."""
import ctypes as C
import math

import numpy as np
import pytest

import gpu_setups as su
import pe25d_gas_radiation_ref as ref
from column_phase_cases import assert_same, final
from gpu_setups import g  # noqa: F401  (the fixture)
from oracle.constants import Cp, G
from oracle.physics import Cg

pytestmark = pytest.mark.gpu

UTC0 = su.UTC0
DT, DTS = 600.0, 120.0
H, W = 6, 72
STEP_SHAPE = (8, 72, 12)                                  # (H, W, L) of the cases that take dynamics steps
LEVELS = (12, 24, 30)
PTOPS = (0.0, 2000.0)
NAMES = ("dt_ground", "dt_air", "olr")
ZENITH = dict(ref.CASES["zenith_d"])

_cache = {}


def inputs(shape, ptop, dtype):
    """(geometry, state, ground temperature), computed once and left unchanged"""
    key = (shape, ptop, dtype)
    if key not in _cache:
        geom = su.geom_of(*shape, ptop=ptop)
        st, gt = ref.state(geom, dtype)
        for a in st + [gt]:
            a.setflags(write=False)
        _cache[key] = (geom, st, gt)
    return _cache[key]


def f32_fields(dtype, names):
    return tuple(n for n in names if n in ("dt_air", "theta")) if dtype == "f32" else ()


# ---------------------------------------------------------------- 1: the diagnostic form
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ptop", PTOPS)
@pytest.mark.parametrize("L", LEVELS)
def test_diagnostic_form_equals_the_restatement(g, L, ptop, dtype):
    geom, st, gt = inputs((H, W, L), ptop, dtype)
    c = su.single(g, geom, st, dtype=dtype, gt=gt)
    assert not c.gas_radiation_registered
    for name, over in ref.CASES.items():
        par = ref.params(**over)
        want = ref.radiation(st[0], st[3], st[4], gt, geom, ref.UTC, par)
        got = c.gas_radiation(geom, ref.UTC, **over)
        ref.judge(got, want[:3], NAMES, (name, L, ptop, dtype), f32_fields(dtype, NAMES))
        assert np.any(want.dt_air != 0) and np.any(want.SC > 0)
        if par["insolation"] == "zenith":
            night = want.SC == 0
            assert night.sum() >= W and (~night).sum() >= W
            dark = c.gas_radiation(geom, ref.UTC, **dict(over, solar_constant=0.0))
            for n, a, b in zip(NAMES, got, dark):
                assert np.array_equal(a[..., night], b[..., night]), (name, n, "short wave in a night column")
                # (the long wave leaving at the top does not know the sun)
                assert np.array_equal(a[..., ~night], b[..., ~night]) == (n == "olr"), (name, n)
    assert_same(final(c), list(st) + [gt], "the diagnostic form changed the state")


# ---------------------------------------------------------------- 2: the step in place, and the closure
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ptop", PTOPS)
@pytest.mark.parametrize("L", LEVELS)
def test_step_in_place_equals_the_restatements_advance(g, L, ptop, dtype):
    geom, st, gt = inputs((H, W, L), ptop, dtype)
    c = su.single(g, geom, st, dtype=dtype, gt=gt)
    for name in ("defaults", "zenith_d", "daily_d"):
        over = ref.CASES[name]
        c.set_state(*st)
        c.set_ground(gt)
        rec = ref.radiation(st[0], st[3], st[4], gt, geom, ref.UTC, ref.params(**over))
        theta_n, gt_n = ref.advance(gt, rec, DT)
        c.gas_radiation_step(geom, DT, ref.UTC, **over)
        out = final(c, close=False)
        names = ("theta", "gt")
        ref.judge((out[3], out[5]), (theta_n, gt_n), names, (name, L, ptop, dtype), f32_fields(dtype, names))
        assert np.max(np.abs(theta_n - st[3])) > 1e-4 and np.max(np.abs(gt_n - gt)) > 1e-3
        for k in (0, 1, 2, 4):
            assert np.array_equal(out[k], st[k]), (name, "puvtq"[k])
    if dtype == "f64":
        # the closure on the device's own outputs; ground_albedo = 0: the ground sends nothing back, and the identity
        # needs no word the diagnostic form does not return
        c.set_state(*st)
        c.set_ground(gt)
        for name in ("uniform_unequal", "daily_d"):
            over = dict(ref.CASES[name], ground_albedo=0.0)
            rec = ref.radiation(st[0], st[3], st[4], gt, geom, ref.UTC, ref.params(**over))
            dg, da, olr = c.gas_radiation(geom, ref.UTC, **over)
            miss = np.sum(rec.heat * da, axis=0) + dg * Cg * .1 + olr - rec.SC
            print("closure on the device", name, L, ptop, "%.3g of SC" % (np.abs(miss).max() / rec.SC.max()))
            assert np.abs(miss).max() <= ref.CLOSURE * rec.SC.max()
    c.close()


# ---------------------------------------------------------------- 3, 4: registered, and off again
def stepping(dtype, ptop=0.0):
    return inputs(STEP_SHAPE, ptop, dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["defaults", "zenith_d"])
def test_registered_step_equals_step_then_explicit_call(g, name, dtype):
    over = ref.CASES[name]
    geom, st, gt = stepping(dtype)
    a = su.single(g, geom, st, dtype=dtype, gt=gt)
    a.set_gas_radiation(**over)                              # ahead of the physics: it takes effect when physics comes on
    assert a.gas_radiation_registered and a.gas_radiation_params == dict(ref.params(**over))
    a.set_physics(geom, UTC0)
    b = su.single(g, geom, st, dtype=dtype, gt=gt)
    for k in range(2):
        a.step(1, DTS)
        b.step(1, DTS)
        b.gas_radiation_step(geom, DTS, UTC0 + k * DTS, **over)
        assert_same(final(a, close=False), final(b, close=False), (name, dtype, k))
        assert a.utc() == UTC0 + (k + 1) * DTS
    assert np.isfinite(a.get_state()[3]).all()
    a.close()
    b.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_unregistered_again_steps_as_one_that_never_registered(g, dtype):
    geom, st, gt = stepping(dtype)
    never = su.single(g, geom, st, dtype=dtype, gt=gt, phys=True)
    assert g._lib.lib.gcm_gas_radiation_on(never._h) == 0 and never.gas_radiation_params is None
    never.step(1, DTS)
    first = final(never, close=False)
    never.step(1, DTS)
    want = final(never, close=False)
    onoff = su.single(g, geom, st, dtype=dtype, gt=gt, phys=True)
    onoff.set_gas_radiation(**ZENITH)
    assert g._lib.lib.gcm_gas_radiation_on(onoff._h) == 1
    onoff.set_gas_radiation(None)
    assert g._lib.lib.gcm_gas_radiation_on(onoff._h) == 0 and not onoff.gas_radiation_registered
    onoff.step(2, DTS)
    assert_same(final(onoff, close=False), want, dtype)
    assert onoff.utc() == never.utc() == UTC0 + 2 * DTS
    # and the registration is not a no-op: with it the same step ends elsewhere
    on = su.single(g, geom, st, dtype=dtype, gt=gt, phys=True)
    on.set_gas_radiation(**ZENITH)
    on.step(1, DTS)
    got = final(on)
    assert not np.array_equal(got[3], first[3]) and not np.array_equal(got[5], first[5])
    assert all(np.array_equal(got[k], first[k]) for k in (0, 1, 2, 4))       # (the solar step writes theta and gt only)
    never.close()
    onoff.close()


# ---------------------------------------------------------------- 5: with the slab ocean
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_slab_ocean_takes_the_words_and_the_budget_closes(g, dtype):
    geom, st, gt = stepping(dtype)
    par = ref.params(**ZENITH)
    C_slab = 2.0e5                                          # (1.13e5 would be the 10 cm of soil of the radiation's own rule)
    c = su.single(g, geom, st, dtype=dtype, gt=gt, phys=True)
    c.set_gas_radiation(**ZENITH)
    c.set_slab_ocean(heat_capacity=C_slab)
    twin = su.single(g, geom, st, dtype=dtype, gt=gt)
    c.step(1, DTS)
    twin.step(1, DTS)
    s1 = twin.get_state()                                    # the state the solar step saw
    twin.close()
    want = ref.radiation(s1[0], s1[3], s1[4], gt, geom, UTC0, par)
    words = c.slab_ocean_fluxes()
    want_words = [getattr(want, n) for n in ref.WORDS]
    ref.judge(list(words[:5]), want_words, ref.WORDS, ("words", dtype))
    assert np.all(words[5:] == 0)
    night = want.SC == 0
    assert night.sum() >= W and (~night).sum() >= W
    assert np.all(words[0][night] == 0) and np.all(words[1][night] == 0)
    out = final(c, close=False)
    theta_n, _ = ref.advance(gt, want, DTS)
    gt_slab = gt + DTS * ((want.sw_sfc + want.lw_down) - want.lw_up) / C_slab
    names = ("theta", "gt")
    ref.judge((out[3], out[5]), (theta_n, gt_slab), names, ("slab", dtype), f32_fields(dtype, names))
    # the ground is the slab's, not the radiation's 10 cm of soil
    assert np.max(np.abs(gt_slab - ref.advance(gt, want, DTS)[1])) > 1e3 * ref.TOL64 * gt.max()
    # the budget: what the top gains less what the surface gains is what heats the air.  The heating comes from the
    # diagnostic form on a float64 handle holding the very state (an fp32 handle rounds dt_air to float32)
    sums = c.slab_ocean_sums()
    assert sums.nsteps == 1 and sums.seconds == DTS
    probe = su.single(g, geom, s1, dtype="f64", gt=gt)
    _, da, _ = probe.gas_radiation(geom, UTC0, **ZENITH)
    probe.close()
    heating = np.sum(Cp * (s1[0] * np.asarray(geom.dsig, dtype=np.float64).reshape(-1, 1, 1)) / G * da, axis=0)
    miss = sums.toa_net - sums.surface_net - heating
    print("slab budget", dtype, "%.3g of SC" % (np.abs(miss).max() / want.SC.max()))
    assert np.abs(miss).max() <= ref.TOL64 * want.SC.max()
    a_g = par["ground_albedo"]
    assert np.all(sums.reflect[night] == 0) and np.allclose(sums.reflect[~night] * words[0][~night], a_g * want.swd0[~night], rtol=1e-9)
    c.close()


# ---------------------------------------------------------------- 6: bands
def band_reference(g, dtype, slab):
    """the single domain after 3 steps, computed once per case"""
    key = ("band", dtype, slab)
    if key not in _cache:
        geom, st, gt = stepping(dtype)
        c = su.single(g, geom, st, dtype=dtype, gt=gt, phys=True)
        register(c, slab)
        c.step(3, DTS)
        out = final(c, close=False)
        assert c.utc() == UTC0 + 3 * DTS and all(np.isfinite(a).all() for a in out)
        sums = c.slab_ocean_sums() if slab else None
        c.close()
        _cache[key] = (out, sums)
    return _cache[key]


def register(c, slab):
    c.set_gas_radiation(**ZENITH)
    if slab:
        c.set_slab_ocean(heat_capacity=1.13e5)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("slab", [False, True], ids=["plain", "slab"])
@pytest.mark.parametrize("host_loop", [False, True], ids=["band_run", "host_loop"])
def test_loopback_band_equals_single_domain(g, host_loop, slab, dtype, monkeypatch):
    import torch
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange
    for k in su.ORCH_ENV:
        monkeypatch.delenv(k, raising=False)
    if host_loop:
        monkeypatch.setenv("GCM_BAND_HOST_LOOP", "1")
    want, want_sums = band_reference(g, dtype, slab)
    geom, st, gt = stepping(dtype)
    Hs, Ws, Ls = STEP_SHAPE
    c = g.Core(g._lib.PE25D, Ws, Hs, Ls, geom=geom, nranks=2, rank=0, global_height=Hs, row0=0, dtype=dtype,
               stream=torch.cuda.current_stream().cuda_stream)
    eng = HipBandEngine(c, torch)
    c.set_ground(gt)
    eng.set_physics(geom, UTC0)
    register(eng, slab)                                     # (the engine forwards to its handle)
    runner = BandRunner(eng, 0, 2, LoopbackExchange(), north=0, south=0)
    assert runner.native == (not host_loop)
    c.set_state(*st)
    runner.run(2, DTS)
    runner.run(1, DTS)
    torch.cuda.synchronize()
    assert_same(final(c, close=False), want, (host_loop, slab, dtype))
    assert c.utc() == UTC0 + 3 * DTS
    if slab:
        got = c.slab_ocean_sums()
        assert (got.nsteps, got.seconds) == (3, 3 * DTS) and np.array_equal(got.sums, want_sums.sums)
    c.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("slab", [False, True], ids=["plain", "slab"])
def test_two_in_process_bands_equal_single_domain(g, slab, dtype):
    """whole stages with their two exchanges, then end_step on every band: own rows and ghost rows, the latter with the
    latitude of their global row"""
    import torch
    from gcmiipy_amd.bands import merge_slab_ocean, split_rows
    want, want_sums = band_reference(g, dtype, slab)
    geom, st, gt = stepping(dtype)
    Hs, Ws, Ls = STEP_SHAPE
    cores = su.bands(g, geom, 2, st, dtype=dtype, gt=gt)
    assert [c.H for c in cores] == [n for _, n in split_rows(Hs, 2)] == [4, 4]
    for c in cores:
        c.set_physics(geom, UTC0)
        register(c, slab)

    def end(k):
        for c in cores:
            c.end_step(DTS)
    su.whole_steps(cores, torch, 3, DTS, after=end)
    parts = [final(c, close=False) for c in cores]
    state = [np.concatenate([x[f] for x in parts], axis=1 if 0 < f < 5 else 0) for f in range(6)]
    assert_same(state, want, (slab, dtype))
    assert all(c.utc() == UTC0 + 3 * DTS for c in cores)
    if slab:
        got = merge_slab_ocean([c.slab_ocean_sums() for c in cores])
        assert (got.nsteps, got.seconds) == (3, 3 * DTS) and np.array_equal(got.sums, want_sums.sums)
        assert np.array_equal(got.reflect, want_sums.reflect)
    for c in cores:
        c.close()


# ---------------------------------------------------------------- 7: checkpoint
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_checkpoint_keeps_the_parameters_and_the_next_steps_bits(g, dtype, tmp_path):
    from gcmiipy_amd import checkpoint
    geom, st, gt = stepping(dtype)
    over = ref.CASES["daily_d"]
    whole = su.single(g, geom, st, dtype=dtype, gt=gt, phys=True)
    whole.set_gas_radiation(**over)
    whole.step(2, DTS)
    want = final(whole)
    a = su.single(g, geom, st, dtype=dtype, gt=gt, phys=True)
    a.set_gas_radiation(**over)
    a.step(1, DTS)
    path = str(tmp_path / "gas.npz")
    checkpoint.save(path, a, step=1, time=a.utc(), geom=geom)
    a.close()
    b, ck = checkpoint.restore(path)
    assert ck["gas_radiation"] == dict(ref.params(**over)) == b.gas_radiation_params and b.gas_radiation_registered
    b.set_physics(geom, ck["time"])
    b.step(1, DTS)
    assert_same(final(b), want, dtype)
    plain = su.single(g, geom, st, dtype=dtype, gt=gt)
    checkpoint.save(path, plain, geom=geom)
    plain.close()
    c, ck = checkpoint.restore(path)
    assert ck["gas_radiation"] is None and not c.gas_radiation_registered
    rec = g._lib.GasRadiation(*[0 if k == "insolation" else v for k, v in ref.DEFAULTS.items()])
    assert g._lib.lib.gcm_set_gas_radiation(c._h, C.byref(rec)) == g._lib.OK
    assert c.gas_radiation_registered and c.gas_radiation_params is None
    with pytest.raises(g.GcmError, match="gcm_set_gas_radiation"):
        checkpoint.save(path, c, geom=geom)
    c.close()


# ---------------------------------------------------------------- 8: the refusals
def test_refusals_change_nothing(g):
    geom, st, gt = inputs((H, W, 12), 0.0, "f64")
    bare = su.single(g, geom, st)
    for call in (lambda: bare.set_gas_radiation(), lambda: bare.gas_radiation(geom, 0.0), lambda: bare.gas_radiation_step(geom, DT, 0.0)):
        with pytest.raises(g.GcmError, match="ground"):
            call()
    assert not bare.gas_radiation_registered
    bare.close()
    c = su.single(g, geom, st, gt=gt)
    c.set_gas_radiation(**ZENITH)
    was = c.gas_radiation_params
    lat, lon = c._latlon(geom)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    bads = [dict(k_h2o_lw=-1.0), dict(k_co2_sw=math.nan), dict(co2_vmr=-1.0), dict(solar_constant=math.inf), dict(ground_albedo=1.0),
            dict(declination=1.6), dict(insolation=5)]
    for bad in bads:
        vals = dict(ref.DEFAULTS, insolation=0)
        vals.update(bad)
        rec = g._lib.GasRadiation(*vals.values())
        assert g._lib.lib.gcm_set_gas_radiation(c._h, C.byref(rec)) == g._lib.ERR_ARG, bad
        assert g._lib.lib.gcm_gas_radiation_step(c._h, DT, 0.0, C.byref(rec), ptr(lat), ptr(lon)) == g._lib.ERR_ARG, bad
        assert g._lib.lib.gcm_gas_radiation(c._h, 0.0, C.byref(rec), ptr(lat), ptr(lon), None, None, None) == g._lib.ERR_ARG, bad
        if "insolation" not in bad:
            with pytest.raises(ValueError):
                c.set_gas_radiation(**bad)
    good = g._lib.GasRadiation(*dict(ref.DEFAULTS, insolation=0).values())
    for dt, utc in ((math.nan, 0.0), (DT, math.inf), (math.inf, math.nan)):
        assert g._lib.lib.gcm_gas_radiation_step(c._h, dt, utc, C.byref(good), ptr(lat), ptr(lon)) == g._lib.ERR_ARG
        with pytest.raises(ValueError):
            c.gas_radiation_step(geom, dt, utc)
    assert g._lib.lib.gcm_gas_radiation(c._h, math.nan, C.byref(good), ptr(lat), ptr(lon), None, None, None) == g._lib.ERR_ARG
    with pytest.raises(ValueError):
        c.gas_radiation(geom, math.nan)
    with pytest.raises(ValueError):
        c.set_gas_radiation(insolation="seasonal")
    with pytest.raises(ValueError):
        c.set_gas_radiation(None, k_h2o_lw=1.0)
    assert c.gas_radiation_params == was and c.gas_radiation_registered
    assert_same(final(c), list(st) + [gt], "a refused call changed the state")
