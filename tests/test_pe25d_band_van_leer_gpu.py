"""GPU tests of van Leer transport on GCM_PE25D latitude bands with two tracer ghost rows per side
(gcm_set_band_tracer_rows(h, 2) / Core(band_tracer_rows=2)).  The criterion throughout is np.array_equal with the
single-domain handle, for state and tracers: the arithmetic per cell is the same kernel on the same values, so every
band path -- eight in-process bands, host-driven whole stages and edge-first phases, gcm_band_run with the loopback
exchange under every orchestration, two gloo ranks, the RCCL self-ring, checkpoints -- gives the single domain's bits.
tests/test_pe25d_band_van_leer_cpu.py shows on the same seeded inputs that one ghost row could not."""
import numpy as np
import pytest

import gpu_setups as su
import pe25d_inputs as inp
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu
UTC0 = inp.UTC0


# ---------------------------------------------------------------- 1. eight in-process bands
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_van_leer_on_eight_bands_equals_single_domain(g, dtype):
    """8 in-process latitude bands of the 64 x 1440 x 24 grid, 3 tracers (random, the latitude step function, a
    constant), ghost rows moved by device copies, 3 steps: state and tracers are the single domain's bit for bit, and
    the tracers are not those of the UPWIND run (VANLEER really ran)"""
    import torch
    c = inp.EIGHT
    geom = su.geom_of(c["H"], c["W"], c["L"])
    st, trs = su.initial(geom, c["ntr"])
    want = su.single_run(g, geom, st, trs, c["steps"], c["dt"], scheme="van_leer", dtype=dtype)
    upwind = su.single_run(g, geom, st, trs, c["steps"], c["dt"], scheme="upwind", dtype=dtype)
    cores = su.bands(g, geom, c["nb"], st, trs, dtype=dtype, scheme="van_leer", rows=2)
    su.whole_steps(cores, torch, c["steps"], c["dt"])
    got = su.gather(cores)
    su.assert_equal(got, want, dtype)
    assert not np.array_equal(got[1], upwind[1])
    assert not np.array_equal(got[1][1], upwind[1][1])            # the step function itself
    assert not np.array_equal(got[1], trs)


# ---------------------------------------------------------------- 2. host-driven bands
@pytest.mark.parametrize("ntr", [2, 5])
@pytest.mark.parametrize("nb", [2, 3])
@pytest.mark.parametrize("mode", ["whole", "phase"])
def test_host_driven_bands_equal_single_domain(g, mode, nb, ntr):
    """host-driven bands in one process with real neighbours: whole stages (gcm_step_interior / gcm_step_boundary) or
    the edge-first phases (gcm_step_phase without send buffers: the split stage, the tracers' edge rows on the caller's
    stream and the interior rows on the third), ghost rows moved by gcm_halo_pack / unpack; 2 and 5 tracers (chunks of
    2; 4 + 1); 16 rows in 3 bands: bands of 6, 5 and 5 rows (one interior row between the edge rows)"""
    import torch
    H, W, L, steps, dt = 16, 20, 5, 3, 120.0
    geom = su.geom_of(H, W, L)
    geom.heightmap[H // 2, 3] = 300.0
    st, trs = su.initial(geom, ntr)
    want = su.single_run(g, geom, st, trs, steps, dt, scheme="van_leer")
    cores = su.bands(g, geom, nb, st, trs, scheme="van_leer", rows=2)
    if mode == "whole":
        su.whole_steps(cores, torch, steps, dt)
    else:
        su.phase_steps(cores, torch, steps, dt)
    su.assert_equal(su.gather(cores), want, (mode, nb, ntr))


def test_unsplittable_short_bands_equal_single_domain(g):
    """bands of 4 and 3 rows (no interior rows between the edge rows: the single tracer launch behind the unpack),
    host-driven phases"""
    import torch
    H, W, L, steps, dt = 14, 20, 5, 3, 120.0
    geom = su.geom_of(H, W, L)
    st, trs = su.initial(geom, 3)
    want = su.single_run(g, geom, st, trs, steps, dt, scheme="van_leer")
    cores = su.bands(g, geom, 4, st, trs, scheme="van_leer", rows=2)        # 4, 4, 3, 3 rows
    assert sorted(c.H for c in cores) == [3, 3, 4, 4]
    su.phase_steps(cores, torch, steps, dt)
    su.assert_equal(su.gather(cores), want)


# ---------------------------------------------------------------- 3. gcm_band_run, loopback exchange
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("phys", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_band_run_loopback_equals_single_domain(g, dtype, phys, overlap):
    """gcm_band_run with the loopback exchange, runs of 3 + 2 steps, then gcm_set_tracers and 2 more (the next run
    exchanges the new tracers' ghost rows, both of them, first); gcm_set_band_overlap on and off, with and without the
    column physics.  Loopback makes the band its own neighbour, so the only boundary crossed is the pole boundary
    (global row H - 1 | row 0, where v = 0 gives the depth-2 ghost values zero weight): this test checks the message
    format, the ordering and the hazards of the two-row exchange; the values that depth 2 carries across an interior
    boundary are checked by the eight-band, host-driven, gloo and checkpoint tests."""
    import torch
    H, W, L, dt, ntr = 23, 36, 9, 120.0, 3
    geom = su.geom_of(H, W, L)
    (st, tr0), gt = su.initial(geom, ntr), inp.ground(H, W)
    tr1 = inp.tracers(H, W, L, ntr, seed=16)[::-1].copy()

    def drive(core, run, set_physics):
        core.set_state(*st)
        core.set_tracers(tr0)
        if phys:
            core.set_ground(gt)
            set_physics()
        run(3)
        run(2)
        a = (core.get_state(), core.get_tracers())
        core.set_tracers(tr1)
        run(2)
        return a, (core.get_state(), core.get_tracers())

    ref = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype=dtype, tracer_scheme="van_leer")
    want = drive(ref, lambda n: ref.step(n, dt), lambda: ref.set_physics(geom, UTC0))
    ref.close()
    c, eng, runner = su.loopback_band(g, torch, geom, ntr, dtype, scheme="van_leer", rows=2)
    assert runner.native
    if overlap:
        c.set_band_overlap(True)

    def run(n):
        runner.run(n, dt)
        torch.cuda.synchronize()
    got = drive(c, run, lambda: eng.set_physics(geom, UTC0))
    c.close()
    for part, (a, b) in enumerate(zip(got, want)):
        su.assert_equal(a, b, part)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_band_run_van_leer_at_overlapping_size(g, dtype, monkeypatch):
    """the 48 x 1440 x 24 band (edge rows marched in level segments; kernels of tens of microseconds on every stream:
    a missing dependency between the tracer launches and the stage's chains shows here) with 4 tracers under the
    default orchestration, one stream (GCM_PE_SINGLE_STREAM=1), the exchange on the comm stream with a join per stage
    (GCM_BAND_COMM_STREAM=1), the host-driven sequence (GCM_BAND_HOST_LOOP=1) and the edge rows dispatched first
    (GCM_BAND_OVERLAP=1).  Loopback: the pole boundary only, see test_band_run_loopback_equals_single_domain."""
    import torch
    H, W, L, dt, ntr = 48, 1440, 24, 1.0, 4
    geom = su.geom_of(H, W, L)
    st, trs = su.initial(geom, ntr)
    want = su.single_run(g, geom, st, trs, 5, dt, scheme="van_leer", dtype=dtype)
    for env in ({}, {"GCM_PE_SINGLE_STREAM": "1"}, {"GCM_BAND_COMM_STREAM": "1"}, {"GCM_BAND_HOST_LOOP": "1"},
                {"GCM_BAND_OVERLAP": "1"}):
        for k in su.ORCH_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c, eng, runner = su.loopback_band(g, torch, geom, ntr, dtype, scheme="van_leer", rows=2)
        assert runner.native == ("GCM_BAND_HOST_LOOP" not in env)
        c.set_state(*st)
        c.set_tracers(trs)
        runner.run(2, dt)
        runner.run(3, dt)
        torch.cuda.synchronize()
        got = c.get_state(), c.get_tracers()
        c.close()
        su.assert_equal(got, want, env)


# ---------------------------------------------------------------- 4. separate processes
GLOO_SHAPE = (14, 20, 5)        # H, W, L
RCCL_SHAPE = (23, 36, 9)
NTR = 3


def _reference(g, shape, steps, dt):
    geom = su.geom_of(*shape)
    st, trs = su.initial(geom, NTR)
    return su.single_run(g, geom, st, trs, steps, dt, scheme="van_leer")


@pytest.mark.parametrize("overlap", [True, False])
def test_gloo_ranks_one_gpu(g, tmp_path, overlap):
    """two ranks in two processes on the one GPU, HipBandEngine + BandRunner over gloo: the default engine (edge-first
    phases, the split stage) and overlap=False (whole stages); gathered from the ranks: the single domain's bits"""
    su.spawn(su.gloo_tracer_worker, (2, overlap, str(tmp_path), GLOO_SHAPE, NTR, False, 2, "van_leer"), 2)
    su.assert_equal(su.load_ranks(str(tmp_path), 2), _reference(g, GLOO_SHAPE, 3, 120.0), overlap)


def test_rccl_self_ring_native(g, tmp_path):
    """gcm_band_run over RCCL called directly, the band its own neighbour on both sides (the periodic single domain)"""
    su.spawn(su.rccl_tracer_worker, (str(tmp_path), RCCL_SHAPE, NTR, False, 2, "van_leer"), 1)
    su.assert_equal(su.load_self(str(tmp_path)), _reference(g, RCCL_SHAPE, 5, 120.0))


# ---------------------------------------------------------------- 5. depth 2 under the other schemes
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("scheme", ["centred", "upwind"])
def test_depth_two_under_centred_and_upwind(g, scheme, dtype):
    """the centred and the donor-cell scheme read rows j -+ 1 only: with two ghost rows only the message grows
    (halo_bytes() is the header's formula with R = 2, asserted where the bands are made), the bits are the single
    domain's -- host-driven phases on 3 bands and gcm_band_run with the loopback exchange"""
    import torch
    H, W, L, steps, dt, ntr = 16, 20, 5, 3, 120.0, 3
    geom = su.geom_of(H, W, L)
    st, trs = su.initial(geom, ntr)
    want = su.single_run(g, geom, st, trs, steps, dt, scheme=scheme, dtype=dtype)
    cores = su.bands(g, geom, 3, st, trs, dtype=dtype, scheme=scheme, rows=2)
    one_row = su.bands(g, geom, 3, st, trs, dtype=dtype, scheme=scheme, rows=1)
    for a, b in zip(cores, one_row):
        assert a.halo_bytes() - b.halo_bytes() == ntr * (8 if dtype == "f64" else 4) * L * W
        b.close()
    su.phase_steps(cores, torch, steps, dt)
    su.assert_equal(su.gather(cores), want, scheme)
    c, eng, runner = su.loopback_band(g, torch, geom, ntr, dtype, scheme=scheme, rows=2)
    assert runner.native
    c.set_state(*st)
    c.set_tracers(trs)
    runner.run(steps, dt)
    torch.cuda.synchronize()
    got = c.get_state(), c.get_tracers()
    c.close()
    su.assert_equal(got, want, (scheme, "band_run"))


def test_switching_schemes_on_a_depth_two_band(g):
    """VANLEER for 2 steps, then the centred scheme for 2, on 2 depth-2 bands: the single domain doing the same"""
    import torch
    H, W, L, dt, ntr = 16, 20, 5, 120.0, 3
    geom = su.geom_of(H, W, L)
    st, trs = su.initial(geom, ntr)
    one = g.Core(g._lib.PE25D, W, H, L, geom=geom, tracer_scheme="van_leer")
    one.set_state(*st)
    one.set_tracers(trs)
    one.step(2, dt)
    mid = one.get_tracers()
    one.set_tracer_scheme("centred")
    one.step(2, dt)
    want = one.get_state(), one.get_tracers()
    one.close()
    cores = su.bands(g, geom, 2, st, trs, scheme="van_leer", rows=2)
    su.whole_steps(cores, torch, 2, dt)
    assert np.array_equal(su.gather(cores, close=False)[1], mid)
    for c in cores:
        c.set_tracer_scheme("centred")
        assert c.band_tracer_rows == 2 and c.tracer_scheme == g._lib.TRACER_NONE
    su.whole_steps(cores, torch, 2, dt, prime=False)
    su.assert_equal(su.gather(cores), want)


# ---------------------------------------------------------------- 6. the setter's refusals
def test_refusals_of_the_setter(g):
    import torch
    from gcmiipy_amd import _lib
    from gcmiipy_amd.core import GcmError
    lib = _lib.lib
    H, W, L = 12, 20, 5
    geom = su.geom_of(H, W, L)
    band = lambda dtype="f64", **kw: g.Core(_lib.PE25D, W, 6, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0,
                                            dtype=dtype, **kw)
    c = band()
    assert c.band_tracer_rows == 1 and c.options["band_tracer_rows"] == 1
    base = c.halo_bytes()
    for bad in (0, 3, -1):
        assert lib.gcm_set_band_tracer_rows(c._h, bad) == _lib.ERR_ARG
        assert c.band_tracer_rows == 1
    # before or after the count, and either repeated
    assert lib.gcm_set_band_tracer_rows(c._h, 2) == _lib.OK and c.band_tracer_rows == 2
    assert c.halo_bytes() == base                                 # no tracers yet: nothing to carry
    assert lib.gcm_set_band_tracers(c._h, 3) == _lib.OK
    assert c.halo_bytes() == base + 3 * 8 * 2 * L * W == inp.halo_bytes(W, L, 8, 3, 2)
    assert lib.gcm_set_band_tracer_rows(c._h, 1) == _lib.OK and c.halo_bytes() == base + 3 * 8 * L * W
    assert c.tracer_count == 3
    # depth 1: VANLEER is still refused, with the reason and the way out, and nothing changes
    c.set_tracer_scheme("upwind")
    assert lib.gcm_set_tracer_scheme(c._h, _lib.TRACER_VANLEER) == _lib.ERR_UNSUPPORTED
    msg = lib.gcm_last_error(c._h).decode()
    assert "ghost row" in msg and "band" in msg and "gcm_set_band_tracer_rows" in msg
    assert c.tracer_scheme == _lib.TRACER_UPWIND and c.band_tracer_rows == 1
    with pytest.raises(GcmError, match="ghost row"):
        c.set_tracer_scheme("van_leer")
    assert c.options["tracer_scheme"] == _lib.TRACER_UPWIND
    # a change of depth gives zeros, like a change of count
    q = inp.state(geom)[4]
    three = np.ascontiguousarray(np.stack([q[:, :6]] * 3))
    c.set_tracers(three)
    assert np.array_equal(c.get_tracers(), three)
    assert lib.gcm_set_band_tracer_rows(c._h, 1) == _lib.OK       # the depth in force: nothing happens
    assert np.array_equal(c.get_tracers(), three)
    assert lib.gcm_set_band_tracer_rows(c._h, 2) == _lib.OK
    assert c.tracer_count == 3 and not c.get_tracers().any()
    c.set_tracers(three)
    assert np.array_equal(c.get_tracers(), three)
    # depth 2: VANLEER is accepted through the setter
    assert lib.gcm_set_tracer_scheme(c._h, _lib.TRACER_VANLEER) == _lib.OK
    assert c.tracer_scheme == _lib.TRACER_VANLEER
    assert lib.gcm_set_band_tracer_rows(c._h, 1) == _lib.ERR_STATE     # not below the scheme in force
    assert c.band_tracer_rows == 2 and c.tracer_scheme == _lib.TRACER_VANLEER
    assert np.array_equal(c.get_tracers(), three)
    # once buffers are registered the format is fixed
    bufs = [torch.empty(c.halo_bytes(), dtype=torch.uint8, device="cuda") for _ in range(4)]
    c.set_halo_buffers(bufs[0].data_ptr(), bufs[1].data_ptr())
    assert lib.gcm_set_band_tracer_rows(c._h, 2) == _lib.ERR_STATE
    c.set_tracer_scheme("centred")
    assert lib.gcm_set_band_tracer_rows(c._h, 1) == _lib.ERR_STATE
    assert c.band_tracer_rows == 2
    c.close()
    # ... through the constructor, and after gcm_set_exchange
    c = band("f32", band_tracers=2, band_tracer_rows=2, tracer_scheme="van_leer")
    assert c.band_tracer_rows == 2 and c.tracer_scheme == _lib.TRACER_VANLEER and c.options["band_tracer_rows"] == 2
    assert c.halo_bytes() == inp.halo_bytes(W, L, 4, 2, 2)
    c.set_exchange(*[b.data_ptr() for b in bufs])
    assert lib.gcm_set_band_tracer_rows(c._h, 1) == _lib.ERR_STATE
    c.close()
    with pytest.raises(GcmError, match="ghost row"):              # a band that says nothing about depth
        band(band_tracers=1, tracer_scheme="van_leer")
    single = g.Core(_lib.PE25D, W, H, L, geom=geom)
    assert lib.gcm_set_band_tracer_rows(single._h, 2) == _lib.ERR_UNSUPPORTED
    assert single.band_tracer_rows == 0
    single.close()
    sw = g.Core(_lib.SW2D, 130, 8, dx=300e3, nranks=2, rank=0, global_height=16, row0=0)
    assert lib.gcm_set_band_tracer_rows(sw._h, 2) == _lib.ERR_UNSUPPORTED
    assert lib.gcm_band_tracer_rows(sw._h) == 0
    sw.close()


# ---------------------------------------------------------------- 7. checkpoints
def test_checkpoint_restores_depth_and_scheme(g, tmp_path):
    """both bands of a 2-band VANLEER run saved after 2 steps, restored from the files' options alone and continued
    for 2: the uninterrupted single domain bit for bit; a file without opt_band_tracer_rows restores at depth 1"""
    import torch
    from gcmiipy_amd import checkpoint
    H, W, L, dt, ntr = 16, 20, 5, 120.0, 3
    geom = su.geom_of(H, W, L)
    st, trs = su.initial(geom, ntr)
    want = su.single_run(g, geom, st, trs, 4, dt, scheme="van_leer")
    cores = su.bands(g, geom, 2, st, trs, scheme="van_leer", rows=2)
    su.whole_steps(cores, torch, 2, dt)
    for r, c in enumerate(cores):
        checkpoint.save(str(tmp_path / ("b%d.npz" % r)), c, step=2, geom=geom)
        c.close()
    cores = []
    for r in range(2):
        c, ck = checkpoint.restore(str(tmp_path / ("b%d.npz" % r)))
        assert ck["options"]["band_tracer_rows"] == 2 and c.band_tracer_rows == 2
        assert c.tracer_scheme == g._lib.TRACER_VANLEER and c.tracer_count == ntr
        cores.append(c)
    su.whole_steps(cores, torch, 2, dt)
    su.assert_equal(su.gather(cores), want)
    d = dict(np.load(str(tmp_path / "b0.npz")))
    del d["opt_band_tracer_rows"]                            # a file written before the option existed ...
    d["opt_tracer_scheme"] = np.asarray(g._lib.TRACER_UPWIND)     # ... which could not hold VANLEER on a band
    old = str(tmp_path / "old.npz")
    np.savez(old, **d)
    c, ck = checkpoint.restore(old)
    assert "band_tracer_rows" not in ck["options"] and c.band_tracer_rows == 1 and c.tracer_count == ntr
    assert c.halo_bytes() == inp.halo_bytes(W, L, 8, ntr, 1)
    c.close()
