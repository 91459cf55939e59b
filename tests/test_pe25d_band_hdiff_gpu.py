"""The horizontal diffusion of GCM_PE25D on latitude bands (gcm_set_band_hdiff): a band that has opted in takes the phase
over its own rows, from the ghost rows the corrector's exchange has just filled, and exchanges its edge rows once more
per step behind it.  Everything is held to the single domain bit for bit (np.array_equal: state, ground temperature,
sums with nsteps and seconds, climatology, clock) -- the explicit call on in-process bands, steps ended by the host with
gcm_end_step_diffuse / exchange / gcm_end_step_begin / [exchange] / gcm_end_step_finish (and a control without the new
exchange, which must NOT agree), gcm_band_run on the loopback band under every orchestration, once at a size where the
streams really overlap; gcm_band_run once more on a band that is its own neighbour at mid-latitude rows, where the new
exchange moves bits that reach the own rows, against the host-ended steps; the opt-in alone, the plan, the refused calls
and the checkpoint.  No tolerance anywhere: a band's own cell sees the single domain's inputs and IEEE operations in the
same order, contraction is off and the coefficients are host-built, so one differing bit is a bug."""
import numpy as np
import pytest

import column_phase_cases as cc
import gpu_setups as su
import pe25d_boundary_layer_ref as blref
import pe25d_inputs as inp
from column_phase_cases import assert_same, assert_same_sums

pytestmark = pytest.mark.gpu

DT = 600.0                                               # the explicit step's dt
DTS = 120.0                                              # the dynamics' dt
GAMMA = 6.5e-3
UTC0 = inp.UTC0
BAND = (9, 12, 36)                                       # (L, H, W); H = 12: 2 and 3 bands
MID = (9, 24, 36)                                        # the band of rows [6, 18) that is its own neighbour
BIG = (24, 48, 1440)                                     # kernels of tens of microseconds on either stream
BL = dict(cd0=1e-3)
STEPS = (2, 1)
# the registered diffusion of the cases that step: with the boundary layer beside it del-4 of all four fields, without it
# del-2 of u, v, theta at a nu that runs most rows at the cap; at BIG, where dt is one second, a nu that caps every row
HD = {True: dict(order=2, nu=1.0e15, fields="uvtq"), False: dict(order=1, nu=1.0e9, fields="uvt")}
HD_BIG = {True: dict(order=2, nu=1.0e22, fields="uvt"), False: dict(order=1, nu=1.0e9, fields="uvtq")}


def geom_of(shape):
    L, H, W = shape
    return su.geom_of(H, W, L)


def esz(dtype):
    return 8 if dtype == "f64" else 4


def band_core(g, geom, nb, r, row0, n, dtype, bl=False, opt_in=True, **kw):
    """one band that has opted in (and to the boundary layer with bl); the opt-in changes neither the message nor
    anything else a plain band reports"""
    H, W, L = geom.height, geom.width, geom.layers
    c = g.Core(g._lib.PE25D, W, n, L, geom=geom, nranks=nb, rank=r, global_height=H, row0=row0, dtype=dtype,
               band_horizontal_diffusion=opt_in, band_boundary_layer=bl, **kw)
    assert c.band_horizontal_diffusion == opt_in and c.options["band_horizontal_diffusion"] is opt_in
    assert c.band_boundary_layer == bl and not c.horizontal_diffusion_registered
    assert c.halo_bytes() == inp.halo_bytes(W, L, esz(dtype), 0, 1)
    return c


def bands(g, geom, nb, st, gt, dtype, bl=False, filter=True):
    """nb in-process bands (split_rows) that have opted in, with their own rows of the state and the ground temperature"""
    from gcmiipy_amd.bands import split_rows
    cores = []
    for r, (row0, n) in enumerate(split_rows(geom.height, nb)):
        c = band_core(g, geom, nb, r, row0, n, dtype, bl, filter=filter)
        sl = slice(row0, row0 + n)
        c.set_state(*[inp.rows(a, sl) for a in st])
        if gt is not None:
            c.set_ground(gt[sl])
        cores.append(c)
    return cores


def register_all(c, geom, hd, bl, solar=True):
    """every phase behind the dynamics, on a Core or a HipBandEngine"""
    if solar:
        c.set_physics(geom, UTC0)
    c.set_held_suarez(geom)
    if hd is not None:
        c.set_horizontal_diffusion(**hd)
    if bl:
        c.set_boundary_layer(**BL)
    c.set_convect(gamma=GAMMA)
    c.set_moist(tau_e=0.0)
    c.set_climate(1)


def final(c):
    return cc.final(c, close=False)


def merged(cores):
    parts = [final(c) for c in cores]
    return [np.concatenate([x[f] for x in parts], axis=1 if 0 < f < 5 else 0) for f in range(6)]


def clock(c):
    import gcmiipy_amd as g
    try:
        return c.utc()
    except g.GcmError:
        return None


def record(c, bl):
    """everything a handle with every phase registered is compared by"""
    out = dict(state=final(c), cv=c.convect_sums(), mo=c.moist_sums(), clim=c.climate_sums(), utc=clock(c))
    if bl:
        out["bl"] = c.boundary_layer_sums()
    return out


def freeze(rec):
    for k in ("bl", "cv", "mo"):
        for a in rec.get(k, ())[2:]:
            a.setflags(write=False)
    for a in rec["state"] + list(rec["clim"][1:]):
        a.setflags(write=False)


def assert_record(c, want, nsteps, what):
    got = record(c, "bl" in want)
    assert_same(got["state"], want["state"], what)
    for k in ("bl", "cv", "mo"):
        if k in want:
            assert_same_sums(got[k], want[k], what)
            assert got[k].nsteps == nsteps and got[k].seconds == nsteps * want["dt"], (what, k)
    (gn, g3, g2), (wn, w3, w2) = got["clim"], want["clim"]
    assert gn == wn == nsteps and np.array_equal(g3, w3) and np.array_equal(g2, w2), what
    assert got["utc"] == want["utc"], (what, got["utc"], want["utc"])


_cache = {}


def inputs(shape, dtype, solar=True):
    """(geometry, state, ground temperature) of a case, computed once and left unchanged: the windy state of the boundary
    layer's tests; the ground of the solar step's tests is the seeded field the radiation tests use"""
    key = ("in", shape, dtype, solar)
    if key not in _cache:
        geom = geom_of(shape)
        st = blref.windy_state(geom, dtype)
        gt = inp.ground(shape[1], shape[2]) if solar else blref.ground(geom, st)
        for a in st + [gt]:
            a.setflags(write=False)
        _cache[key] = (geom, st, gt)
    return _cache[key]


def single_all(g, geom, st, gt, dtype, hd, bl, solar=True):
    c = su.single(g, geom, st, dtype=dtype, gt=gt)
    register_all(c, geom, hd, bl, solar)
    return c


def reference(g, dtype, bl, shape=BAND, steps=STEPS, dt=DTS, hd=None):
    """the single domain with every phase registered after steps[0] and after steps[0] + steps[1] steps, computed once
    per case; finite, and not what the same run without the diffusion gives"""
    hd = hd or HD[bl]
    key = ("ref", shape, dtype, bl, steps, dt)
    if key not in _cache:
        geom, st, gt = inputs(shape, dtype)
        c = single_all(g, geom, st, gt, dtype, hd, bl)
        out = []
        for n in steps:
            c.step(n, dt)
            out.append(dict(record(c, bl), dt=dt))
        c.close()
        plain = single_all(g, geom, st, gt, dtype, None, bl)
        plain.step(sum(steps), dt)
        without = final(plain)
        plain.close()
        last = out[-1]["state"]
        assert all(np.isfinite(a).all() for a in last)
        assert all(not np.array_equal(last[f], without[f]) for f in (1, 2, 3)), "the phase changes u, v and theta"
        for r in out:
            freeze(r)
        _cache[key] = out
    return _cache[key]


# ---------------------------------------------------------------- 1: the explicit call on in-process bands
CASES = [((3, 12, 36), 2), ((3, 12, 36), 3),             # the plain case
         ((2, 8, 36), 4),                                # bands of 2 rows: every own row is an edge row
         ((2, 34, 36), 2),                               # 17 rows: a row-tile seam inside the band and a last tile of one row
         ((2, 32, 130), 2)]                              # 16 rows = one full tile; two column tiles with a 2-column tail
EXPLICIT = (dict(order=1, nu=1.0e9, fields="uvtq"), dict(order=2, nu=1.0e15, fields="uvt"), dict(order=2, nu=1.0e22, fields="uvtq"),
            dict(order=1, nu=1.0e5, fields="uvt"))


def explicit_reference(g, shape, dtype):
    key = ("explicit", shape, dtype)
    if key not in _cache:
        geom = geom_of(shape)
        st = inp.state_of(geom, dtype)
        c = su.single(g, geom, st, dtype=dtype, filter=False)
        out = []
        for par in EXPLICIT:
            c.set_state(*st)
            c.horizontal_diffusion_step(DT, **par)
            out.append(c.get_state())
        c.close()
        _cache[key] = (geom, st, out)
    return _cache[key]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,nb", CASES)
def test_explicit_step_on_bands_equals_single_domain(shape, nb, dtype):
    """horizontal_diffusion_step on every band behind one exchange: own rows from the ghost rows -2, -1, H and H + 1 with
    the coefficients of the global rows, the single domain's bits; unselected fields and p untouched"""
    import torch
    import gcmiipy_amd as g
    geom, st, want = explicit_reference(g, shape, dtype)
    cores = bands(g, geom, nb, st, None, dtype, filter=False)
    for par, w in zip(EXPLICIT, want):
        for c in cores:
            row0 = c.options["row0"]
            c.set_state(*[inp.rows(a, slice(row0, row0 + c.H)) for a in st])
        su.exchange(cores, torch)
        for c in cores:
            c.horizontal_diffusion_step(DT, **par)
            assert not c.horizontal_diffusion_registered      # (an explicit step registers nothing)
        parts = [c.get_state() for c in cores]
        got = [np.concatenate([x[f] for x in parts], axis=0 if f == 0 else 1) for f in range(5)]
        for f, name in enumerate("puvtq"):
            bad = np.argwhere(got[f] != w[f])
            assert bad.size == 0, (shape, nb, dtype, par, name, bad[:4].tolist())
            if name not in par["fields"]:
                assert np.array_equal(got[f], st[f]), (par, name)
        if par["nu"] >= 1.0e9:
            assert all(not np.array_equal(w[f], st[f]) for f in (1, 2, 3)), par
    for c in cores:
        c.close()


# ---------------------------------------------------------------- 2: steps ended by the host
def host_ended_steps(cores, torch, n, dt, bl, prime, new_exchange=True):
    def end(k):
        for c in cores:
            c.end_step_diffuse(dt)
        if new_exchange:
            su.exchange(cores, torch)
        for c in cores:
            c.end_step_begin(dt)
        if bl:
            su.exchange(cores, torch)
        for c in cores:
            c.end_step_finish(dt)
    su.whole_steps(cores, torch, n, dt, prime=prime, after=end)


@pytest.mark.parametrize("bl", [False, True], ids=["plain", "with_bl"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nb", [2, 3])
def test_host_ended_steps_equal_single_domain(nb, dtype, bl):
    """whole stages with their two exchanges, then end_step_diffuse on every band, the new exchange, end_step_begin, the
    boundary layer's exchange where that is registered, end_step_finish, with the solar step, Held-Suarez, the diffusion,
    [the boundary layer,] the convective adjustment, the moist physics and the climatology registered"""
    import torch
    import gcmiipy_amd as g
    from gcmiipy_amd.bands import merge_boundary_layer, merge_convect, merge_moist
    want = reference(g, dtype, bl)
    geom, st, gt = inputs(BAND, dtype)
    cores = bands(g, geom, nb, st, gt, dtype, bl)
    for c in cores:
        register_all(c, geom, HD[bl], bl)
        assert c.horizontal_diffusion_registered and c.horizontal_diffusion["order"] == HD[bl]["order"]
    for part, n in enumerate(STEPS):
        w, nsteps, what = want[part], sum(STEPS[:part + 1]), (nb, dtype, bl, part)
        host_ended_steps(cores, torch, n, DTS, bl, prime=part == 0)
        got = merged(cores)
        assert all(np.isfinite(a).all() for a in got)
        assert_same(got, w["state"], what)
        for merge, name, k in ((merge_boundary_layer, "boundary_layer", "bl"), (merge_convect, "convect", "cv"),
                               (merge_moist, "moist", "mo")):
            if k not in w:
                continue
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


@pytest.mark.parametrize("bl", [False, True], ids=["plain", "with_bl"])
def test_without_the_new_exchange_the_bands_differ(bl):
    """the control of the test above: the same sequence without the exchange between diffuse and begin leaves the ghost
    rows as they were ahead of the diffusion, and the next stage reads them -- the bands then do NOT hold the single
    domain's bits.  (If they did, the inputs would not reach the seams and the test above would show nothing.)"""
    import torch
    import gcmiipy_amd as g
    want = reference(g, "f64", bl)[0]
    geom, st, gt = inputs(BAND, "f64")
    cores = bands(g, geom, 2, st, gt, "f64", bl)
    for c in cores:
        register_all(c, geom, HD[bl], bl)
    host_ended_steps(cores, torch, STEPS[0], DTS, bl, prime=True, new_exchange=False)
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


def loopback_band(g, torch, geom, dtype, gt, bl=False, opt_in=True):
    """the opted-in band that is its own neighbour, driven by gcm_band_run: (handle, engine, runner)"""
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange
    c = band_core(g, geom, 2, 0, 0, geom.height, dtype, bl, opt_in, stream=torch.cuda.current_stream().cuda_stream)
    eng = HipBandEngine(c, torch)
    c.set_ground(gt)
    return c, eng, BandRunner(eng, 0, 2, LoopbackExchange(), north=0, south=0)


@pytest.mark.parametrize("orch", list(ORCHESTRATIONS))
@pytest.mark.parametrize("bl", [False, True], ids=["plain", "with_bl"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_band_run_equals_single_domain(dtype, bl, orch, monkeypatch):
    """gcm_band_run with every phase registered: the diffusion of the own rows behind the corrector's unpack and one more
    exchange on the second stream (default), on the comm stream with its join, on the one stream, driven by the host
    (physics_diffuse / exchange / physics_begin ...), and with the edge rows dispatched first; with the boundary layer
    registered too a step takes four exchanges.  (The loopback band is its own neighbour: its one seam is the single
    domain's pole-to-pole wrap, where rank 0's ghost rows take the coefficients of the global rows Hg - 2 and Hg - 1.)"""
    import torch
    import gcmiipy_amd as g
    orchestrate(monkeypatch, orch)
    want = reference(g, dtype, bl)
    geom, st, gt = inputs(BAND, dtype)
    c, eng, runner = loopback_band(g, torch, geom, dtype, gt, bl)
    assert runner.native == (orch != "host_loop")
    if orch == "overlap":
        c.set_band_overlap(1)
    register_all(eng, geom, HD[bl], bl)
    c.set_state(*st)
    for part, n in enumerate(STEPS):
        runner.run(n, DTS)
        torch.cuda.synchronize()
        assert_record(c, want[part], sum(STEPS[:part + 1]), (dtype, bl, orch, part))
    assert c.halo_bytes() == inp.halo_bytes(geom.width, geom.layers, esz(dtype), 0, 1)
    c.close()


@pytest.mark.parametrize("orch", ["default", "comm_stream", "host_loop"])
def test_band_run_carries_the_tracers_through_the_new_exchange(orch, monkeypatch):
    """a band with two passive tracers: their edge rows ride in the new exchange's message as in every other; state and
    tracers are the single domain's, which the diffusion leaves the tracers of alone"""
    import torch
    import gcmiipy_amd as g
    orchestrate(monkeypatch, orch)
    geom = geom_of(BAND)
    L, H, W = BAND
    st, trs = su.initial(geom, 2)
    key = ("tracers", BAND)
    if key not in _cache:
        one = su.single(g, geom, st, trs)
        one.set_horizontal_diffusion(**HD[True])
        one.step(sum(STEPS), DTS)
        _cache[key] = (one.get_state(), one.get_tracers())
        one.close()
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0, band_tracers=2,
               band_horizontal_diffusion=True, stream=torch.cuda.current_stream().cuda_stream)
    assert c.halo_bytes() == inp.halo_bytes(W, L, 8, 2, 1)
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange
    eng = HipBandEngine(c, torch)
    runner = BandRunner(eng, 0, 2, LoopbackExchange(), north=0, south=0)
    assert runner.native == (orch != "host_loop")
    eng.set_horizontal_diffusion(**HD[True])
    c.set_state(*st)
    c.set_tracers(trs)
    for n in STEPS:
        runner.run(n, DTS)
    torch.cuda.synchronize()
    su.assert_equal((c.get_state(), c.get_tracers()), _cache[key], orch)
    c.close()


# ---------------------------------------------------------------- 3b: gcm_band_run at a seam in mid-domain
# The band below is its own neighbour at mid-latitude rows (the middle half of the grid): the edge rows differ from the
# ghost rows they become and their coefficients from one another's.  It is no model state, and no single domain holds its
# bits; the yardstick is the same band stepped by the host sequence that test 2 holds to the single domain at mid-domain
# seams.
def mid_band(g, geom, st, gt, dtype, bl, **kw):
    H = geom.height
    row0, n = H // 4, H // 2
    c = band_core(g, geom, 2, 1, row0, n, dtype, bl, **kw)
    sl = slice(row0, row0 + n)
    c.set_state(*[inp.rows(a, sl) for a in st])
    c.set_ground(gt[sl])
    return c


def mid_reference(g, dtype, bl, shape, steps, dt, hd):
    """the mid-latitude band after steps[0] and after steps[0] + steps[1] host-ended steps, computed once per case;
    finite, its seam rows moved by the new exchange (without it other bits)"""
    import torch
    key = ("mid", shape, dtype, bl, steps, dt)
    if key not in _cache:
        geom, st, gt = inputs(shape, dtype)
        out = {}
        for new_exchange in (True, False):
            c = mid_band(g, geom, st, gt, dtype, bl)
            register_all(c, geom, hd, bl)
            recs = []
            for part, n in enumerate(steps):
                host_ended_steps([c], torch, n, dt, bl, prime=part == 0, new_exchange=new_exchange)
                recs.append(dict(record(c, bl), dt=dt))
            c.close()
            out[new_exchange] = recs
        want, without = out[True], out[False]
        last = want[-1]["state"]
        assert all(np.isfinite(a).all() for a in last)
        assert any(not np.array_equal(a, b) for a, b in zip(last[1:5], without[-1]["state"][1:5])), "the new exchange matters here"
        for r in want:
            freeze(r)
        _cache[key] = want
    return _cache[key]


def mid_band_run(g, torch, monkeypatch, dtype, bl, shape, steps, dt, orch, hd):
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange
    want = mid_reference(g, dtype, bl, shape, steps, dt, hd)
    orchestrate(monkeypatch, orch)
    geom, st, gt = inputs(shape, dtype)
    c = mid_band(g, geom, st, gt, dtype, bl, stream=torch.cuda.current_stream().cuda_stream)
    eng = HipBandEngine(c, torch)
    runner = BandRunner(eng, 1, 2, LoopbackExchange(), north=1, south=1)
    assert runner.native == (orch != "host_loop")
    if orch == "overlap":
        c.set_band_overlap(1)
    register_all(eng, geom, hd, bl)
    for part, n in enumerate(steps):
        runner.run(n, dt)
        torch.cuda.synchronize()
        assert_record(c, want[part], sum(steps[:part + 1]), (dtype, bl, orch, part))
    c.close()


@pytest.mark.parametrize("orch", list(ORCHESTRATIONS))
@pytest.mark.parametrize("dtype,bl", [("f64", True), ("f32", False), ("f64", False), ("f32", True)])
def test_band_run_at_a_mid_domain_seam_equals_host_ended_steps(dtype, bl, orch, monkeypatch):
    """gcm_band_run's new exchange where it matters: the band that is its own neighbour at rows [H / 4, 3 H / 4), every
    phase registered, under every orchestration, against the host-ended steps of the same band"""
    import torch
    import gcmiipy_amd as g
    mid_band_run(g, torch, monkeypatch, dtype, bl, MID, STEPS, DTS, orch, HD[bl])


@pytest.mark.parametrize("dtype,bl", [("f64", True), ("f32", False)])
def test_band_run_at_a_mid_domain_seam_where_launches_overlap(dtype, bl, monkeypatch):
    """the same at 48 x 1440 x 24 (a band of 24 rows: a row-tile seam, twelve column tiles), 2 steps: the default
    orchestration, one stream, the comm stream and the edge rows first"""
    import torch
    import gcmiipy_amd as g
    for orch in ("default", "single_stream", "comm_stream", "overlap"):
        mid_band_run(g, torch, monkeypatch, dtype, bl, BIG, (2,), 1.0, orch, HD_BIG[bl])


# ---------------------------------------------------------------- 4: at a size where the launches overlap
@pytest.mark.parametrize("dtype,bl", [("f64", False), ("f32", True)])
def test_band_run_chains_with_the_new_exchange(dtype, bl, monkeypatch):
    """48 x 1440 x 24, 2 steps, the loopback band: the default orchestration, one stream, the exchange on the comm stream
    and the edge rows first all give the single domain's bits, state and sums"""
    import torch
    import gcmiipy_amd as g
    dt, steps = 1.0, 2
    orchestrate(monkeypatch, "default")
    want = reference(g, dtype, bl, BIG, (steps,), dt, HD_BIG[bl])[0]
    geom, st, gt = inputs(BIG, dtype)
    for orch in ("default", "single_stream", "comm_stream", "overlap"):
        orchestrate(monkeypatch, orch)
        c, eng, runner = loopback_band(g, torch, geom, dtype, gt, bl)
        assert runner.native
        if orch == "overlap":
            c.set_band_overlap(1)
        register_all(eng, geom, HD_BIG[bl], bl)
        c.set_state(*st)
        runner.run(steps, dt)
        torch.cuda.synchronize()
        assert_record(c, want, steps, (dtype, bl, orch))
        c.close()


# ---------------------------------------------------------------- 5: unchanged behaviour
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_opt_in_alone_changes_nothing(dtype, monkeypatch):
    """an opted-in band without a registration: a plain band's bits and halo_bytes under gcm_band_run and under the
    host-driven sequence, whose physics_diffuse then asks for no exchange"""
    import torch
    import gcmiipy_amd as g
    geom, st, gt = inputs(BAND, dtype)
    out = {}
    for orch in ("default", "host_loop"):
        orchestrate(monkeypatch, orch)
        for opt_in in (False, True):
            c, eng, runner = loopback_band(g, torch, geom, dtype, gt, opt_in=opt_in)
            register_all(eng, geom, None, False)
            c.set_state(*st)
            assert not eng.physics_diffuse(DTS)
            runner.run(3, DTS)
            torch.cuda.synchronize()
            out[orch, opt_in] = dict(record(c, False), dt=DTS, bytes=c.halo_bytes())
            if opt_in:
                assert_record(c, out[orch, False], 3, (dtype, orch))
                assert out[orch, True]["bytes"] == out[orch, False]["bytes"]
            c.close()


def test_plan_on_a_band_reports_the_bands_tiles():
    import gcmiipy_amd as g
    L, H, W = 2, 68, 130
    geom = su.geom_of(H, W, L)
    c = band_core(g, geom, 2, 1, 34, 34, "f64", filter=False)
    plan = c.horizontal_diffusion_plan()
    tr, tc = plan["tile_rows"], plan["tile_cols"]
    assert plan["tiles_j"] == -(-34 // tr) and plan["tiles_i"] == -(-W // tc) and plan["grid_z"] == 3 * L
    assert plan["launches"] == 1
    c.set_horizontal_diffusion(order=1, nu=1.0e5, fields="uvtq")
    plan1 = c.horizontal_diffusion_plan()
    assert plan1["grid_z"] == 4 * L and plan1["lds_bytes"] < plan["lds_bytes"] and plan1["tiles_j"] == plan["tiles_j"]
    c.close()


# ---------------------------------------------------------------- 6: refused calls
def test_refused_calls_change_nothing():
    import torch
    import gcmiipy_amd as g
    from pe25d_hdiff_ref import params
    lib, L_ = g._lib.lib, g._lib
    bl = False
    geom, st, gt = inputs(BAND, "f64")
    H, W, L = geom.height, geom.width, geom.layers
    rec = L_.Hdiff(*params(order=2, nu=1.0e15).values())
    nan, inf = float("nan"), float("inf")
    # a null handle
    assert lib.gcm_set_band_hdiff(None, 1) == L_.ERR_ARG and lib.gcm_band_hdiff(None) == L_.ERR_ARG
    assert lib.gcm_end_step_diffuse(None, DTS) == L_.ERR_ARG
    # a single domain: the opt-in is a band's; on = 0 is nothing to do; end_step_diffuse queues nothing
    one = single_all(g, geom, st, gt, "f64", HD[bl], bl)
    one.step(1, DTS)
    was = record(one, bl)
    assert lib.gcm_set_band_hdiff(one._h, 1) == L_.ERR_UNSUPPORTED and lib.gcm_band_hdiff(one._h) == 0
    assert b"bands only" in lib.gcm_last_error(one._h)
    assert lib.gcm_set_band_hdiff(one._h, 0) == L_.OK and not one.band_horizontal_diffusion
    with pytest.raises(ValueError, match="band_horizontal_diffusion needs a GCM_PE25D latitude band"):
        g.Core(L_.PE25D, W, H, L, geom=geom, band_horizontal_diffusion=True)
    for dt in (nan, inf, -inf):
        assert lib.gcm_end_step_diffuse(one._h, dt) == L_.ERR_ARG
    with pytest.raises(ValueError, match="gcm_end_step_diffuse: dt must be finite"):
        one.end_step_diffuse(nan)
    one.end_step_diffuse(DTS)
    assert_record(one, dict(was, dt=DTS), 1, "single domain")
    one.close()
    # other models
    s = g.Core(L_.SW2D, 32, 16, dx=1e5)
    rng = np.random.default_rng(5)
    s.set_state(8000.0 + rng.standard_normal((16, 32)), rng.standard_normal((16, 32)), rng.standard_normal((16, 32)))
    was2d = s.get_state()[:3]
    assert lib.gcm_set_band_hdiff(s._h, 1) == L_.ERR_UNSUPPORTED and lib.gcm_band_hdiff(s._h) == 0
    assert lib.gcm_set_band_hdiff(s._h, 0) == L_.ERR_UNSUPPORTED
    assert lib.gcm_end_step_diffuse(s._h, DTS) == L_.ERR_UNSUPPORTED
    assert all(np.array_equal(a, b) for a, b in zip(s.get_state()[:3], was2d)), "SW2D"
    s.close()
    with pytest.raises(ValueError, match="band_horizontal_diffusion needs a GCM_PE25D latitude band"):
        g.Core(L_.SW2D, 32, 16, dx=1e5, nranks=2, band_horizontal_diffusion=True)
    # a band that opts out again is refused as ever
    c = band_core(g, geom, 2, 0, 0, H, "f64")
    c.set_state(*st)
    c.set_ground(gt)
    assert lib.gcm_set_band_hdiff(c._h, 0) == L_.OK and not c.band_horizontal_diffusion
    assert lib.gcm_set_hdiff(c._h, rec) == L_.ERR_UNSUPPORTED and lib.gcm_hdiff_on(c._h) == 0
    assert b"gcm_set_band_hdiff" in lib.gcm_last_error(c._h)
    assert lib.gcm_hdiff_step(c._h, DTS, rec) == L_.ERR_UNSUPPORTED
    assert_same(c.get_state(), st[:5], "not opted in")
    assert lib.gcm_set_band_hdiff(c._h, 1) == L_.OK and c.band_horizontal_diffusion
    # registered: on = 0, gcm_end_step and a gcm_end_step_begin without gcm_end_step_diffuse are GCM_ERR_STATE
    register_all(c, geom, HD[bl], bl)
    su.exchange([c], torch)
    c.end_step_diffuse(DTS)
    su.exchange([c], torch)
    c.end_step_begin(DTS)
    c.end_step_finish(DTS)
    was = record(c, bl)
    assert not np.array_equal(was["state"][1], st[1])
    assert lib.gcm_set_band_hdiff(c._h, 0) == L_.ERR_STATE and c.band_horizontal_diffusion
    assert b"registered" in lib.gcm_last_error(c._h)
    assert lib.gcm_end_step(c._h, DTS) == L_.ERR_STATE
    msg = lib.gcm_last_error(c._h).decode()
    assert "gcm_end_step_diffuse" in msg and "gcm_end_step_begin" in msg and "gcm_end_step_finish" in msg, msg
    with pytest.raises(g.GcmError, match="gcm_end_step_diffuse"):
        c.end_step(DTS)
    assert lib.gcm_end_step_begin(c._h, DTS) == L_.ERR_STATE
    msg = lib.gcm_last_error(c._h).decode()
    assert "gcm_end_step_diffuse" in msg and "gcm_end_step_begin" in msg, msg
    with pytest.raises(g.GcmError, match="gcm_end_step_diffuse"):
        c.end_step_begin(DTS)
    for dt in (nan, inf):
        assert lib.gcm_end_step_diffuse(c._h, dt) == L_.ERR_ARG and lib.gcm_end_step_begin(c._h, dt) == L_.ERR_ARG
    assert c.horizontal_diffusion_registered and c.horizontal_diffusion["order"] == HD[bl]["order"]
    assert_record(c, dict(was, dt=DTS), 1, "band")
    # unregistered, the band may opt out
    c.set_horizontal_diffusion(None)
    assert lib.gcm_set_band_hdiff(c._h, 0) == L_.OK and not c.band_horizontal_diffusion
    c.close()


# ---------------------------------------------------------------- 7: checkpoint
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_checkpoint_carries_the_opt_in(dtype, tmp_path, monkeypatch):
    """an opted-in band with the phase registered: saved after 2 steps, restored (the opt-in ahead of the registration)
    and run on through the loopback runner, against the uninterrupted run; a file without the option restores with the
    opt-in off"""
    import torch
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange
    orchestrate(monkeypatch, "default")
    bl = dtype == "f64"
    geom, st, gt = inputs(BAND, dtype, solar=False)
    stream = torch.cuda.current_stream().cuda_stream

    def band():
        c, eng, runner = loopback_band(g, torch, geom, dtype, gt, bl)
        assert runner.native
        register_all(eng, geom, HD[bl], bl, solar=False)
        c.set_state(*st)
        return c, runner
    whole, runner = band()
    runner.run(3, DTS)
    torch.cuda.synchronize()
    want = dict(record(whole, bl), dt=DTS)
    whole.close()
    a, runner = band()
    runner.run(2, DTS)
    torch.cuda.synchronize()
    path = str(tmp_path / "band_hdiff.npz")
    checkpoint.save(path, a, step=2, geom=geom)
    a.close()
    b, ck = checkpoint.restore(path, stream=stream)
    assert ck["band_horizontal_diffusion"] is True and b.band_horizontal_diffusion
    assert b.options["band_horizontal_diffusion"] is True and ck["band_boundary_layer"] is bl
    assert b.horizontal_diffusion_registered and b.horizontal_diffusion == ck["hdiff"]
    assert ck["hdiff"]["order"] == HD[bl]["order"] and ck["hdiff"]["nu"] == HD[bl]["nu"]
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
    assert bool(d["opt_band_horizontal_diffusion"]) is True
    del d["opt_band_horizontal_diffusion"]
    np.savez(path, **d)
    c, ck = checkpoint.restore(path)
    assert ck["band_horizontal_diffusion"] is False and not c.band_horizontal_diffusion and ck["hdiff"] is None
    c.close()
