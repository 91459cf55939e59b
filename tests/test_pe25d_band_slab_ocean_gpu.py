"""The slab mixed-layer ocean of GCM_PE25D on latitude bands, held to the single domain bit for bit (np.array_equal):
state, ground temperature and the merged sums with nsteps and seconds.  Two registrations on (H, W, L) = (24, 36, 9):
  * radiation + slab: the phase is column-local, a band's ghost rows are advanced locally from the words their own
    radiation launch stored, and add to no sum;
  * radiation + boundary layer + slab on bands that have opted in (band_boundary_layer=True): own rows only, ahead of the
    third exchange, whose message carries the ground temperature; here the slab also takes a capacity field (with cells
    held at their temperature) and a heat-flux field, each band its own rows.
Each under gcm_band_run on the band that is its own neighbour (the loopback band of gpu_setups), under the host-driven
sequence of the same runner (GCM_BAND_HOST_LOOP=1: end_step_begin, the exchange where the band carries the boundary
layer, end_step_finish), and on 3 in-process bands whose steps the host ends.  The message is what it was:
halo_bytes() is asserted against the plain band's."""
import numpy as np
import pytest

import gpu_setups as su
import pe25d_boundary_layer_ref as bref
import pe25d_inputs as inp
import pe25d_slab_ocean_ref as ref
from column_phase_cases import assert_same, final
from gpu_setups import g  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

DTS = 120.0
UTC0 = inp.UTC0
SHAPE = (24, 36, 9)                                       # (H, W, L): 3 bands of 8 rows
NB = 3
STEPS = (2, 1)
REGS = ("radiation", "boundary")

_cache = {}


def inputs(dtype):
    """(geometry, state, ground temperature, capacity field, heat-flux field), computed once and left unchanged"""
    if dtype not in _cache:
        H, W, L = SHAPE
        geom = su.geom_of(H, W, L)
        st = bref.windy_state(geom, dtype)
        gt = bref.ground(geom, st)
        rng = np.random.default_rng(8)
        cap = 10.0 ** rng.uniform(5.0, 7.0, (H, W))
        cap[rng.random((H, W)) < 0.2] = np.inf
        cap[7, :4], cap[8, :4] = np.inf, 2.0e5               # (either side of a seam between two bands)
        Q = 40.0 * rng.standard_normal((H, W))
        for a in st + [gt, cap, Q]:
            a.setflags(write=False)
        _cache[dtype] = (geom, st, gt, cap, Q)
    return _cache[dtype]


def register(c, geom, reg, cap, Q):
    """the phases of a case on a Core or a HipBandEngine, in the model's order; cap, Q: the handle's own rows"""
    c.set_physics(geom, UTC0)
    if reg == "boundary":
        c.set_boundary_layer()
        c.set_slab_ocean(heat_capacity=2.0e6, capacity=cap, qflux=Q)
    else:
        c.set_slab_ocean(heat_capacity=1.13e5)


def record(c):
    return dict(state=final(c, close=False), slab=c.slab_ocean_sums(), utc=c.utc(),
                bl=c.boundary_layer_sums() if c.boundary_layer_registered else None)


def reference(g, reg, dtype):
    """the single domain after STEPS[0] and after STEPS[0] + STEPS[1] steps, computed once per case; finite, the slab's
    sums moved, and the ground is not what the run without the slab leaves"""
    key = ("ref", reg, dtype)
    if key not in _cache:
        geom, st, gt, cap, Q = inputs(dtype)
        c = su.single(g, geom, st, dtype=dtype, gt=gt)
        register(c, geom, reg, cap, Q)
        out = []
        for n in STEPS:
            c.step(n, DTS)
            out.append(record(c))
        c.close()
        last = out[-1]
        assert all(np.isfinite(a).all() for a in last["state"])
        assert all(last["slab"].sums[k].any() for k in (0, 1, 2, 3, 4, 8, 9))
        if reg == "boundary":
            assert all(last["slab"].sums[k].any() for k in (5, 6, 7))
            held = np.isinf(cap)
            assert np.array_equal(last["state"][5][held], gt[held]) and (last["state"][5][~held] != gt[~held]).all()
        for r in out:
            for a in r["state"] + [r["slab"].sums]:
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def assert_record(got_state, got_slab, got_bl, utc, want, nsteps, what):
    assert_same(got_state, want["state"], what)
    assert (got_slab.nsteps, got_slab.seconds, got_slab.reflect) == (nsteps, nsteps * DTS, want["slab"].reflect), what
    assert (want["slab"].nsteps, want["slab"].seconds) == (nsteps, nsteps * DTS), what
    for k in range(ref.NSUMS):
        assert np.array_equal(got_slab.sums[k], want["slab"].sums[k]), (what, "sum", k)
    if want["bl"] is not None:
        assert np.array_equal(got_bl.shf, want["bl"].shf) and np.array_equal(got_bl.evap, want["bl"].evap), what
    assert utc == want["utc"] == UTC0 + nsteps * DTS, what


# ---------------------------------------------------------------- 1: the loopback band, gcm_band_run and the host-driven split
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("host_loop", [False, True], ids=["band_run", "host_loop"])
@pytest.mark.parametrize("reg", REGS)
def test_loopback_band_equals_single_domain(g, reg, host_loop, dtype, monkeypatch):
    import torch
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange
    for k in su.ORCH_ENV:
        monkeypatch.delenv(k, raising=False)
    if host_loop:
        monkeypatch.setenv("GCM_BAND_HOST_LOOP", "1")
    want = reference(g, reg, dtype)
    geom, st, gt, cap, Q = inputs(dtype)
    H, W, L = SHAPE
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0, dtype=dtype,
               stream=torch.cuda.current_stream().cuda_stream, band_boundary_layer=reg == "boundary")
    assert c.halo_bytes() == inp.halo_bytes(W, L, 8 if dtype == "f64" else 4, 0, 1)
    eng = HipBandEngine(c, torch)
    c.set_ground(gt)
    register(eng.c, geom, reg, cap, Q)
    runner = BandRunner(eng, 0, 2, LoopbackExchange(), north=0, south=0)
    assert runner.native == (not host_loop)
    c.set_state(*st)
    for part, n in enumerate(STEPS):
        runner.run(n, DTS)
        torch.cuda.synchronize()
        assert_record(final(c, close=False), c.slab_ocean_sums(), c.boundary_layer_sums() if reg == "boundary" else None,
                      c.utc(), want[part], sum(STEPS[:part + 1]), (reg, host_loop, dtype, part))
    assert c.halo_bytes() == inp.halo_bytes(W, L, 8 if dtype == "f64" else 4, 0, 1)
    c.close()


# ---------------------------------------------------------------- 2: three in-process bands, steps ended by the host
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("reg", REGS)
def test_host_ended_steps_on_three_bands_equal_single_domain(g, reg, dtype):
    """whole stages with their two exchanges; then end_step on every band (radiation + slab), or end_step_begin, the
    third exchange and end_step_finish (with the boundary layer)"""
    import torch
    from gcmiipy_amd.bands import merge_boundary_layer, merge_slab_ocean, split_rows
    want = reference(g, reg, dtype)
    geom, st, gt, cap, Q = inputs(dtype)
    H, W, L = SHAPE
    cores = []
    for r, (row0, n) in enumerate(split_rows(H, NB)):
        c = g.Core(g._lib.PE25D, W, n, L, geom=geom, nranks=NB, rank=r, global_height=H, row0=row0, dtype=dtype,
                   band_boundary_layer=reg == "boundary")
        assert c.halo_bytes() == inp.halo_bytes(W, L, 8 if dtype == "f64" else 4, 0, 1)
        sl = slice(row0, row0 + n)
        c.set_state(*[inp.rows(a, sl) for a in st])
        c.set_ground(gt[sl])
        register(c, geom, reg, cap[sl], Q[sl])
        cores.append(c)

    def end(k):
        if reg == "boundary":
            for c in cores:
                c.end_step_begin(DTS)
            su.exchange(cores, torch)
            for c in cores:
                c.end_step_finish(DTS)
        else:
            for c in cores:
                c.end_step(DTS)
    for part, n in enumerate(STEPS):
        su.whole_steps(cores, torch, n, DTS, prime=part == 0, after=end)
        parts = [final(c, close=False) for c in cores]
        state = [np.concatenate([x[f] for x in parts], axis=1 if 0 < f < 5 else 0) for f in range(6)]
        slab = merge_slab_ocean([c.slab_ocean_sums() for c in cores])
        bl = merge_boundary_layer([c.boundary_layer_sums() for c in cores]) if reg == "boundary" else None
        assert all(c.utc() == cores[0].utc() for c in cores)
        assert_record(state, slab, bl, cores[0].utc(), want[part], sum(STEPS[:part + 1]), (reg, dtype, part))
    for c in cores:
        c.close()
