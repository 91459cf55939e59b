"""The surface fluxes and the boundary-layer mixing of GCM_PE25D on latitude bands (gcm_set_band_boundary_layer): a band
that has opted in takes the phase over its own rows and exchanges its edge rows a third time per step.  Everything is
held to the single domain bit for bit (np.array_equal: state, ground temperature, sums with nsteps and seconds,
climatology, clock) -- the explicit call on in-process bands, steps ended by the host with gcm_end_step_begin / exchange
/ gcm_end_step_finish (and a control without the exchange, which must NOT agree), gcm_band_run on the loopback band
under every orchestration, once at a size where the streams really overlap, the two calls on a single domain, the
refused calls and the checkpoint; and gcm_band_run once more on a band that is its own neighbour at mid-latitude rows,
where the third exchange moves bits that reach the own rows, against the host-ended steps.  The bands are built here (Core(..., band_boundary_layer=True)); the exchange and the
stepping patterns are gpu_setups'."""
import functools

import numpy as np
import pytest

import column_phase_cases as cc
import gpu_setups as su
import pe25d_boundary_layer_ref as ref
import pe25d_inputs as inp
from column_phase_cases import assert_same, assert_same_sums

pytestmark = pytest.mark.gpu

DT = 600.0                                               # the explicit step's dt
DTS = 120.0                                              # the dynamics' dt
GAMMA = 6.5e-3
UTC0 = inp.UTC0
BAND = (9, 12, 36)                                       # (L, H, W); H = 12: 2 and 3 bands
BL = dict(cd0=1e-3)
STEPS = (2, 1)


def geom_of(shape, ptop=0.0):
    L, H, W = shape
    return su.geom_of(H, W, L, ptop)


def band_core(g, geom, nb, r, row0, n, dtype, **kw):
    """one band that has opted in; the opt-in changes neither the message nor anything else a plain band reports"""
    H, W, L = geom.height, geom.width, geom.layers
    c = g.Core(g._lib.PE25D, W, n, L, geom=geom, nranks=nb, rank=r, global_height=H, row0=row0, dtype=dtype,
               band_boundary_layer=True, **kw)
    assert c.band_boundary_layer and c.options["band_boundary_layer"] is True
    assert c.halo_bytes() == inp.halo_bytes(W, L, 8 if dtype == "f64" else 4, 0, 1)
    return c


def bands(g, geom, nb, st, gt, dtype="f64", filter=True):
    """nb in-process bands (split_rows) that have opted in, with their own rows of the state and the ground temperature"""
    from gcmiipy_amd.bands import split_rows
    cores = []
    for r, (row0, n) in enumerate(split_rows(geom.height, nb)):
        c = band_core(g, geom, nb, r, row0, n, dtype, filter=filter)
        sl = slice(row0, row0 + n)
        c.set_state(*[inp.rows(a, sl) for a in st])
        c.set_ground(gt[sl])
        cores.append(c)
    return cores


def loopback_band(g, torch, geom, dtype, gt):
    """the opted-in band that is its own neighbour, driven by gcm_band_run: (handle, engine, runner)"""
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange
    c = band_core(g, geom, 2, 0, 0, geom.height, dtype, stream=torch.cuda.current_stream().cuda_stream)
    eng = HipBandEngine(c, torch)
    c.set_ground(gt)
    return c, eng, BandRunner(eng, 0, 2, LoopbackExchange(), north=0, south=0)


def register_all(c, geom, solar=True, bl=True):
    """every phase behind the dynamics, on a Core or a HipBandEngine"""
    if solar:
        c.set_physics(geom, UTC0)
    c.set_held_suarez(geom)
    if bl:
        c.set_boundary_layer(**BL)
    c.set_convect(gamma=GAMMA)
    c.set_moist(tau_e=0.0)
    c.set_climate(1)


final = functools.partial(cc.final, close=False)         # (every handle here has a ground temperature; the callers close)


def merged(cores):
    parts = [final(c) for c in cores]
    return [np.concatenate([x[f] for x in parts], axis=1 if 0 < f < 5 else 0) for f in range(6)]


def clock(c):
    """the handle's clock, None where no solar step is registered"""
    import gcmiipy_amd as g
    try:
        return c.utc()
    except g.GcmError:
        return None


def record(c):
    """everything a handle with every phase registered is compared by"""
    return dict(state=final(c), bl=c.boundary_layer_sums(), cv=c.convect_sums(), mo=c.moist_sums(), clim=c.climate_sums(),
                utc=clock(c))


def assert_record(c, want, nsteps, what):
    got = record(c)
    assert_same(got["state"], want["state"], what)
    for k in ("bl", "cv", "mo"):
        assert_same_sums(got[k], want[k], what)
        assert got[k].nsteps == nsteps and got[k].seconds == nsteps * want["dt"], (what, k)
    (gn, g3, g2), (wn, w3, w2) = got["clim"], want["clim"]
    assert gn == wn == nsteps and np.array_equal(g3, w3) and np.array_equal(g2, w2), what
    assert got["utc"] == want["utc"], (what, got["utc"], want["utc"])


def single_all(g, geom, st, gt, dtype, solar=True, bl=True):
    c = su.single(g, geom, st, dtype=dtype, gt=gt)
    register_all(c, geom, solar, bl)
    return c


_cache = {}


def inputs(shape, dtype, ptop=0.0, solar=False):
    """(geometry, state, ground temperature) of a case, computed once and left unchanged: the windy state; the ground of
    the solar step's tests is the seeded field the radiation tests use, else a field warmer and colder than the air"""
    key = ("in", shape, dtype, ptop, solar)
    if key not in _cache:
        geom = geom_of(shape, ptop)
        st = ref.windy_state(geom, dtype)
        gt = inp.ground(shape[1], shape[2]) if solar else ref.ground(geom, st)
        for a in st + [gt]:
            a.setflags(write=False)
        _cache[key] = (geom, st, gt)
    return _cache[key]


def reference(g, dtype, shape=BAND, steps=STEPS, dt=DTS, solar=True):
    """the single domain with every phase registered after steps[0] and after steps[0] + steps[1] steps, computed once
    per case; finite, and not what the same run without the boundary layer gives"""
    key = ("ref", shape, dtype, steps, dt, solar)
    if key not in _cache:
        geom, st, gt = inputs(shape, dtype, solar=solar)
        c = single_all(g, geom, st, gt, dtype, solar)
        out = []
        for n in steps:
            c.step(n, dt)
            out.append(dict(record(c), dt=dt))
        c.close()
        plain = single_all(g, geom, st, gt, dtype, solar, bl=False)
        plain.step(sum(steps), dt)
        without = final(plain)
        plain.close()
        last = out[-1]
        assert all(np.isfinite(a).all() for a in last["state"])
        assert last["bl"].shf.any() and last["bl"].evap.any()
        assert all(not np.array_equal(a, b) for a, b in zip(last["state"][1:5], without[1:5])), "the phase changes u, v, theta and q"
        for r in out:
            for a in r["state"] + list(r["bl"][2:]) + list(r["cv"][2:]) + list(r["mo"][2:]) + list(r["clim"][1:]):
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


# ---------------------------------------------------------------- 1: the explicit call on in-process bands
CASES = [((9, 12, 36), 2, 0.0), ((9, 12, 36), 3, 0.0), ((9, 12, 36), 3, 1000.0),
         ((5, 8, 130), 2, 0.0),                          # two column tiles with a tail; an even width for fp32
         ((41, 8, 66), 2, 0.0)]                          # L > 40: y and g parked in the scratch fields


def explicit_reference(g, shape, ptop, dtype):
    key = ("explicit", shape, ptop, dtype)
    if key not in _cache:
        geom, st, gt = inputs(shape, dtype, ptop)
        c = su.single(g, geom, st, dtype=dtype, filter=False, gt=gt)
        c.set_boundary_layer(**BL)
        c.boundary_layer_step(DT, **BL)
        _cache[key] = (final(c), c.boundary_layer_sums())
        c.close()
    return _cache[key]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,nb,ptop", CASES)
def test_explicit_step_on_bands_equals_single_domain(shape, nb, ptop, dtype):
    """boundary_layer_step on every band behind one exchange: own rows from the ghost rows -1 and H, the single domain's
    bits; registered, so the bands' sums put together are the single domain's too"""
    import torch
    import gcmiipy_amd as g
    from gcmiipy_amd.bands import merge_boundary_layer
    want, want_sums = explicit_reference(g, shape, ptop, dtype)
    geom, st, gt = inputs(shape, dtype, ptop)
    cores = bands(g, geom, nb, st, gt, dtype, filter=False)
    for c in cores:
        c.set_boundary_layer(**BL)
        assert c.boundary_layer == ref.params(**BL)
    su.exchange(cores, torch)
    for c in cores:
        c.boundary_layer_step(DT, **BL)
    assert_same(merged(cores), want, (shape, nb, ptop, dtype))
    assert all((a != b).any() for a, b in zip(want[1:5], st[1:5]))
    sums = merge_boundary_layer([c.boundary_layer_sums() for c in cores])
    assert_same_sums(sums, want_sums, (shape, nb, ptop, dtype))
    assert (sums.nsteps, sums.seconds) == (1, DT) and sums.shf.any() and sums.evap.any()
    for c in cores:
        c.close()


# ---------------------------------------------------------------- 2: steps ended by the host
def host_ended_steps(cores, torch, n, prime, third_exchange=True):
    def end(k):
        for c in cores:
            c.end_step_begin(DTS)
        if third_exchange:
            su.exchange(cores, torch)
        for c in cores:
            c.end_step_finish(DTS)
    su.whole_steps(cores, torch, n, DTS, prime=prime, after=end)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nb", [2, 3])
def test_host_ended_steps_equal_single_domain(nb, dtype):
    """whole stages with their two exchanges, then end_step_begin on every band, the third exchange, end_step_finish on
    every band, with the solar step, Held-Suarez, the boundary layer, the convective adjustment, the moist physics and
    the climatology registered"""
    import torch
    import gcmiipy_amd as g
    from gcmiipy_amd.bands import merge_boundary_layer, merge_convect, merge_moist
    want = reference(g, dtype)
    geom, st, gt = inputs(BAND, dtype, solar=True)
    cores = bands(g, geom, nb, st, gt, dtype)
    for c in cores:
        register_all(c, geom)
    for part, n in enumerate(STEPS):
        w, nsteps, what = want[part], sum(STEPS[:part + 1]), (nb, dtype, part)
        host_ended_steps(cores, torch, n, prime=part == 0)
        got = merged(cores)
        assert all(np.isfinite(a).all() for a in got)
        assert_same(got, w["state"], what)
        for merge, name, k in ((merge_boundary_layer, "boundary_layer", "bl"), (merge_convect, "convect", "cv"),
                               (merge_moist, "moist", "mo")):
            sums = merge([getattr(c, name + "_sums")() for c in cores])
            assert_same_sums(sums, w[k], what)
            assert sums.nsteps == nsteps and sums.seconds == nsteps * DTS
        clim = [c.climate_sums() for c in cores]
        assert all(n_ == w["clim"][0] == nsteps for n_, _, _ in clim)
        assert np.array_equal(np.concatenate([m3 for _, m3, _ in clim], axis=-1), w["clim"][1]), what
        assert np.array_equal(np.concatenate([m2 for _, _, m2 in clim], axis=-1), w["clim"][2]), what
        assert all(c.utc() == w["utc"] == UTC0 + nsteps * DTS for c in cores)
    for c in cores:
        c.close()


def test_without_the_third_exchange_the_bands_differ():
    """the control of the test above: the same sequence without the exchange between begin and finish leaves the ghost
    rows as they were ahead of the boundary layer, and the next step reads them -- the bands then do NOT hold the single
    domain's bits.  (If they did, the inputs would not reach the seams and the test above would show nothing.)"""
    import torch
    import gcmiipy_amd as g
    want = reference(g, "f64")[0]
    geom, st, gt = inputs(BAND, "f64", solar=True)
    cores = bands(g, geom, 2, st, gt, "f64")
    for c in cores:
        register_all(c, geom)
    host_ended_steps(cores, torch, STEPS[0], prime=True, third_exchange=False)
    got = merged(cores)
    for c in cores:
        c.close()
    assert any(not np.array_equal(a, b) for a, b in zip(got[1:5], want["state"][1:5]))


# ---------------------------------------------------------------- 3: gcm_band_run on the loopback band
ORCHESTRATIONS = {"default": {}, "comm_stream": {"GCM_BAND_COMM_STREAM": "1"}, "single_stream": {"GCM_PE_SINGLE_STREAM": "1"},
                  "host_loop": {"GCM_BAND_HOST_LOOP": "1"}, "overlap": {}}


def orchestrate(monkeypatch, name):
    for k in su.ORCH_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in ORCHESTRATIONS[name].items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("orch", list(ORCHESTRATIONS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_band_run_equals_single_domain(dtype, orch, monkeypatch):
    """gcm_band_run with every phase registered: the third exchange on the second stream beside the own rows' convective
    adjustment and moist physics (default), on the comm stream with its join, on the one stream, driven by the host
    (physics_begin / exchange / physics_end), and with the edge rows dispatched first.  (The loopback band is its own
    neighbour: its one seam is the single domain's pole-to-pole wrap.  The seams in mid-domain are test 2's and 3b's.)"""
    import torch
    import gcmiipy_amd as g
    orchestrate(monkeypatch, orch)
    want = reference(g, dtype)
    geom, st, gt = inputs(BAND, dtype, solar=True)
    c, eng, runner = loopback_band(g, torch, geom, dtype, gt)
    assert runner.native == (orch != "host_loop")
    if orch == "overlap":
        c.set_band_overlap(1)
    register_all(eng, geom)
    c.set_state(*st)
    for part, n in enumerate(STEPS):
        runner.run(n, DTS)
        torch.cuda.synchronize()
        assert_record(c, want[part], sum(STEPS[:part + 1]), (dtype, orch, part))
    c.close()


# ---------------------------------------------------------------- 3b: gcm_band_run at a seam in mid-domain
# The loopback band above is the whole domain: its one seam is the pole-to-pole wrap, where v is zero and scratch row H
# holds the bits of row 0, so nothing the boundary layer reads from a ghost row, and nothing the third exchange
# delivers, reaches an own row there.  The band below is its own neighbour at mid-latitude rows (the middle half of the
# grid): v at its seam is not zero, and the edge rows differ from the ghost rows they become.  It is no model state, and
# no single domain holds its bits; the yardstick is the same band stepped by the host sequence that test 2 holds to the
# single domain at mid-domain seams: whole stages, end_step_begin, the exchange, end_step_finish.
def mid_band(g, geom, st, gt, dtype, **kw):
    """the middle half of the grid as a band that is its own neighbour, opted in, every phase registered"""
    H = geom.height
    row0, n = H // 4, H // 2
    c = band_core(g, geom, 2, 1, row0, n, dtype, **kw)
    sl = slice(row0, row0 + n)
    c.set_state(*[inp.rows(a, sl) for a in st])
    c.set_ground(gt[sl])
    return c


def mid_reference(g, dtype, shape, steps, dt):
    """the mid-latitude band after steps[0] and after steps[0] + steps[1] host-ended steps, computed once per case;
    finite, its seam rows moved by the third exchange (without it other bits), v at the seam not zero"""
    import torch
    key = ("mid", shape, dtype, steps, dt)
    if key not in _cache:
        geom, st, gt = inputs(shape, dtype, solar=True)
        out = {}
        for third in (True, False):
            c = mid_band(g, geom, st, gt, dtype)
            register_all(c, geom)
            recs = []
            for part, n in enumerate(steps):
                def end(k):
                    c.end_step_begin(dt)
                    if third:
                        su.exchange([c], torch)
                    c.end_step_finish(dt)
                su.whole_steps([c], torch, n, dt, prime=part == 0, after=end)
                recs.append(dict(record(c), dt=dt))
            c.close()
            out[third] = recs
        want, without = out[True], out[False]
        last = want[-1]["state"]
        assert all(np.isfinite(a).all() for a in last)
        assert last[2][:, -1].any() and last[2][:, 0].any(), "v at the seam is not zero"
        assert any(not np.array_equal(a, b) for a, b in zip(last[1:5], without[-1]["state"][1:5])), "the third exchange matters here"
        for r in want:
            for a in r["state"] + list(r["bl"][2:]) + list(r["cv"][2:]) + list(r["mo"][2:]) + list(r["clim"][1:]):
                a.setflags(write=False)
        _cache[key] = want
    return _cache[key]


def mid_band_run(g, torch, monkeypatch, dtype, shape, steps, dt, orch):
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange
    want = mid_reference(g, dtype, shape, steps, dt)
    orchestrate(monkeypatch, orch)
    geom, st, gt = inputs(shape, dtype, solar=True)
    c = mid_band(g, geom, st, gt, dtype, stream=torch.cuda.current_stream().cuda_stream)
    eng = HipBandEngine(c, torch)
    runner = BandRunner(eng, 1, 2, LoopbackExchange(), north=1, south=1)
    assert runner.native == (orch != "host_loop")
    if orch == "overlap":
        c.set_band_overlap(1)
    register_all(eng, geom)
    for part, n in enumerate(steps):
        runner.run(n, dt)
        torch.cuda.synchronize()
        assert_record(c, want[part], sum(steps[:part + 1]), (dtype, orch, part))
    c.close()


@pytest.mark.parametrize("orch", list(ORCHESTRATIONS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_band_run_at_a_mid_domain_seam_equals_host_ended_steps(dtype, orch, monkeypatch):
    """gcm_band_run's third exchange where it matters: the band that is its own neighbour at rows [H / 4, 3 H / 4), every
    phase registered, under every orchestration, against the host-ended steps of the same band -- state, ground, the
    three sums, climatology, clock"""
    import torch
    import gcmiipy_amd as g
    mid_band_run(g, torch, monkeypatch, dtype, (9, 24, 36), STEPS, DTS, orch)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_band_run_at_a_mid_domain_seam_where_launches_overlap(dtype, monkeypatch):
    """the same at 48 x 1440 x 24 (a band of 24 rows; kernels of tens of microseconds on either stream), 2 steps: the
    default orchestration, one stream, the comm stream and the edge rows first"""
    import torch
    import gcmiipy_amd as g
    for orch in ("default", "single_stream", "comm_stream", "overlap"):
        mid_band_run(g, torch, monkeypatch, dtype, (24, 48, 1440), (2,), 1.0, orch)


# ---------------------------------------------------------------- 4: at a size where the launches overlap
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_band_run_chains_with_the_third_exchange(dtype, monkeypatch):
    """48 x 1440 x 24 (kernels of tens of microseconds on either stream), 2 steps: the default orchestration, one stream
    and the exchange on the comm stream all give the single domain's bits, state and sums"""
    import torch
    import gcmiipy_amd as g
    shape, dt, steps = (24, 48, 1440), 1.0, 2
    orchestrate(monkeypatch, "default")
    want = reference(g, dtype, shape, (steps,), dt)[0]
    geom, st, gt = inputs(shape, dtype, solar=True)
    for orch in ("default", "single_stream", "comm_stream"):
        orchestrate(monkeypatch, orch)
        c, eng, runner = loopback_band(g, torch, geom, dtype, gt)
        assert runner.native
        register_all(eng, geom)
        c.set_state(*st)
        runner.run(steps, dt)
        torch.cuda.synchronize()
        assert_record(c, want, steps, (dtype, orch))
        c.close()


# ---------------------------------------------------------------- 5: the two calls on a single domain
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_begin_and_finish_are_end_step_on_a_single_domain(dtype):
    """half_step x 2 + end_step_begin + end_step_finish, and half_step x 2 + end_step, three times each, against
    step(3, dt) with every phase registered: nothing needs to happen between the two calls"""
    import gcmiipy_amd as g
    want = reference(g, dtype)[-1]
    geom, st, gt = inputs(BAND, dtype, solar=True)
    for split in (True, False):
        c = single_all(g, geom, st, gt, dtype)
        assert not c.band_boundary_layer
        for _ in range(sum(STEPS)):
            c.half_step(0, DTS)
            c.half_step(1, DTS)
            if split:
                c.end_step_begin(DTS)
                c.end_step_finish(DTS)
            else:
                c.end_step(DTS)
        assert_record(c, want, sum(STEPS), (dtype, split))
        c.close()


# ---------------------------------------------------------------- 6: refused calls
def test_refused_calls_change_nothing():
    import gcmiipy_amd as g
    lib, L_ = g._lib.lib, g._lib
    geom, st, gt = inputs(BAND, "f64", solar=True)
    H, W, L = geom.height, geom.width, geom.layers
    rec = L_.BoundaryLayer(*ref.params(**BL).values())
    nan, inf = float("nan"), float("inf")
    # a null handle
    assert lib.gcm_set_band_boundary_layer(None, 1) == L_.ERR_ARG and lib.gcm_band_boundary_layer(None) == L_.ERR_ARG
    assert lib.gcm_end_step_begin(None, DTS) == L_.ERR_ARG and lib.gcm_end_step_finish(None, DTS) == L_.ERR_ARG
    # a single domain: the opt-in is a band's; on = 0 is nothing to do
    one = single_all(g, geom, st, gt, "f64")
    one.step(1, DTS)
    was = record(one)
    assert lib.gcm_set_band_boundary_layer(one._h, 1) == L_.ERR_UNSUPPORTED and lib.gcm_band_boundary_layer(one._h) == 0
    assert b"bands only" in lib.gcm_last_error(one._h)
    assert lib.gcm_set_band_boundary_layer(one._h, 0) == L_.OK and not one.band_boundary_layer
    with pytest.raises(ValueError, match="band_boundary_layer needs a GCM_PE25D latitude band"):
        g.Core(L_.PE25D, W, H, L, geom=geom, band_boundary_layer=True)
    # a non-finite dt for both new calls
    for dt in (nan, inf, -inf):
        assert lib.gcm_end_step_begin(one._h, dt) == L_.ERR_ARG and lib.gcm_end_step_finish(one._h, dt) == L_.ERR_ARG
    with pytest.raises(ValueError, match="gcm_end_step_begin: dt must be finite"):
        one.end_step_begin(nan)
    with pytest.raises(ValueError, match="gcm_end_step_finish: dt must be finite"):
        one.end_step_finish(inf)
    assert_record(one, dict(was, dt=DTS), 1, "single domain")
    one.close()
    # other models
    s = g.Core(L_.SW2D, 32, 16, dx=1e5)
    rng = np.random.default_rng(5)
    s.set_state(8000.0 + rng.standard_normal((16, 32)), rng.standard_normal((16, 32)), rng.standard_normal((16, 32)))
    was2d = s.get_state()[:3]
    assert lib.gcm_set_band_boundary_layer(s._h, 1) == L_.ERR_UNSUPPORTED and lib.gcm_band_boundary_layer(s._h) == 0
    assert lib.gcm_set_band_boundary_layer(s._h, 0) == L_.ERR_UNSUPPORTED
    assert lib.gcm_end_step_begin(s._h, DTS) == L_.ERR_UNSUPPORTED and lib.gcm_end_step_finish(s._h, DTS) == L_.ERR_UNSUPPORTED
    assert all(np.array_equal(a, b) for a, b in zip(s.get_state()[:3], was2d)), "SW2D"
    s.close()
    with pytest.raises(ValueError, match="band_boundary_layer needs a GCM_PE25D latitude band"):
        g.Core(L_.SW2D, 32, 16, dx=1e5, nranks=2, band_boundary_layer=True)
    # an opted-in band (its own neighbour) without a ground temperature: the registration's own GCM_ERR_STATE
    import torch
    c = band_core(g, geom, 2, 0, 0, H, "f64")
    c.set_state(*st)
    assert lib.gcm_set_boundary_layer(c._h, rec) == L_.ERR_STATE and lib.gcm_boundary_layer_on(c._h) == 0
    assert lib.gcm_boundary_layer_step(c._h, DTS, rec) == L_.ERR_STATE
    assert_same(c.get_state(), st[:5], "no ground")
    # a band that opts out again is refused as ever
    assert lib.gcm_set_band_boundary_layer(c._h, 0) == L_.OK and not c.band_boundary_layer
    c.set_ground(gt)
    assert lib.gcm_set_boundary_layer(c._h, rec) == L_.ERR_UNSUPPORTED and lib.gcm_boundary_layer_on(c._h) == 0
    assert lib.gcm_boundary_layer_step(c._h, DTS, rec) == L_.ERR_UNSUPPORTED
    assert lib.gcm_set_band_boundary_layer(c._h, 1) == L_.OK and c.band_boundary_layer
    # registered: on = 0 and gcm_end_step are GCM_ERR_STATE
    register_all(c, geom)
    su.exchange([c], torch)
    c.end_step_begin(DTS)
    c.end_step_finish(DTS)
    was = record(c)
    assert lib.gcm_set_band_boundary_layer(c._h, 0) == L_.ERR_STATE and c.band_boundary_layer
    assert b"registered" in lib.gcm_last_error(c._h)
    assert lib.gcm_end_step(c._h, DTS) == L_.ERR_STATE
    msg = lib.gcm_last_error(c._h).decode()
    assert "gcm_end_step_begin" in msg and "gcm_end_step_finish" in msg, msg
    with pytest.raises(g.GcmError, match="gcm_end_step_begin"):
        c.end_step(DTS)
    for dt in (nan, inf):
        assert lib.gcm_end_step_begin(c._h, dt) == L_.ERR_ARG and lib.gcm_end_step_finish(c._h, dt) == L_.ERR_ARG
    assert c.boundary_layer == ref.params(**BL) and c.boundary_layer_registered
    assert_record(c, dict(was, dt=DTS), 1, "band")
    # unregistered, the band may opt out
    c.set_boundary_layer(None)
    assert lib.gcm_set_band_boundary_layer(c._h, 0) == L_.OK and not c.band_boundary_layer
    c.close()


# ---------------------------------------------------------------- 7: checkpoint
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_checkpoint_carries_the_opt_in(dtype, tmp_path, monkeypatch):
    """an opted-in band with the phase registered and sums accumulated: saved after 2 steps, restored (the opt-in ahead of
    the registration) and run on through the loopback runner, against the uninterrupted run; a file without the option
    restores with the opt-in off"""
    import torch
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange
    orchestrate(monkeypatch, "default")
    geom, st, gt = inputs(BAND, dtype)
    stream = torch.cuda.current_stream().cuda_stream

    def band():
        c, eng, runner = loopback_band(g, torch, geom, dtype, gt)
        assert runner.native
        register_all(eng, geom, solar=False)
        c.set_state(*st)
        return c, runner
    whole, runner = band()
    runner.run(3, DTS)
    torch.cuda.synchronize()
    want = dict(record(whole), dt=DTS)
    whole.close()
    a, runner = band()
    runner.run(2, DTS)
    torch.cuda.synchronize()
    assert a.boundary_layer_sums().shf.any()
    path = str(tmp_path / "band_bl.npz")
    checkpoint.save(path, a, step=2, geom=geom)
    a.close()
    b, ck = checkpoint.restore(path, stream=stream)
    assert ck["band_boundary_layer"] is True and b.band_boundary_layer and b.options["band_boundary_layer"] is True
    assert b.boundary_layer == ref.params(**BL) and ck["boundary_layer"]["n"] == 2
    runner = BandRunner(HipBandEngine(b, torch), 0, 2, LoopbackExchange(), north=0, south=0)
    assert runner.native
    runner.run(1, DTS)
    torch.cuda.synchronize()
    assert_record(b, want, 3, "restored")
    b.close()
    # a file written before the option existed
    plain = band_core(g, geom, 2, 0, 0, geom.height, dtype)
    plain.set_state(*st)
    checkpoint.save(path, plain, geom=geom)
    plain.close()
    d = dict(np.load(path))
    del d["opt_band_boundary_layer"]
    np.savez(path, **d)
    c, ck = checkpoint.restore(path)
    assert ck["band_boundary_layer"] is False and not c.band_boundary_layer and ck["boundary_layer"] is None
    c.close()
