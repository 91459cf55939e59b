"""GPU tests of the passive tracers on GCM_PE25D latitude bands (gcm_set_band_tracers): every band path -- the
host-driven exchange (whole stages and the edge-first phases), gcm_band_run with the loopback exchange at a small
and at an overlapping size, eight bands of one grid, separate processes over gloo and over RCCL -- gives the single
domain's tracers and state bit for bit (the same kernel on the same inputs, fp64 and fp32 alike)."""
import numpy as np
import pytest

import gpu_setups as su
import pe25d_inputs as inp

pytestmark = pytest.mark.gpu
UTC0 = inp.UTC0


@pytest.mark.parametrize("ntr", [2, 5])
@pytest.mark.parametrize("nb", [2, 3])
@pytest.mark.parametrize("mode", ["whole", "phase"])
def test_host_driven_bands_equal_single_domain(mode, nb, ntr):
    """host-driven bands in one process: whole stages (gcm_step_interior / gcm_step_boundary) or the edge-first phases
    (gcm_step_phase without send buffers: the tracers' edge rows on the caller's stream, the interior rows on the third
    stream), the ghost rows moved by gcm_halo_pack / unpack.  2 and 5 tracers (chunks of 2; 4 + 1), the first equal
    to q: it stays equal to q."""
    import torch
    import gcmiipy_amd as g
    H, W, L, steps, dt = 16, 20, 5, 3, 120.0
    geom = su.geom_of(H, W, L)
    geom.heightmap[H // 2, 3] = 300.0
    ic, tr = su.initial(geom, ntr, from_q=True)
    want = su.single_run(g, geom, ic, tr, steps, dt)
    cores = su.bands(g, geom, nb, ic, tr)
    for c in cores:
        assert c.tracer_count == ntr
    (su.whole_steps if mode == "whole" else su.phase_steps)(cores, torch, steps, dt)
    got, got_tr = su.gather(cores)
    su.assert_equal((got, got_tr), want, mode)
    assert np.array_equal(got_tr[0], got[4])             # the tracer that started as q is still q


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("phys", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_band_run_loopback_equals_single_domain(dtype, phys, overlap):
    """gcm_band_run with the loopback exchange (the band is its own neighbour: the periodic single domain), runs of
    3 + 2 steps (the second starts from a primed state), then gcm_set_tracers between two runs: the next run exchanges
    the new tracers' ghost rows first"""
    import torch
    import gcmiipy_amd as g
    H, W, L, dt, ntr = 23, 36, 9, 120.0, 3
    geom = su.geom_of(H, W, L)
    (ic, tr0), gt = su.initial(geom, ntr, from_q=True), inp.ground(H, W)
    tr1 = inp.tracers_from_q(ic[4], ntr, seed=15)[::-1].copy()

    def drive(core, run, set_physics):
        core.set_state(*ic)
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

    ref = su.single(g, geom, dtype=dtype)
    want = drive(ref, lambda n: ref.step(n, dt), lambda: ref.set_physics(geom, UTC0))
    ref.close()
    c, eng, runner = su.loopback_band(g, torch, geom, ntr, dtype)
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
    if dtype == "f64":
        assert np.array_equal(got[0][1][0], got[0][0][4])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_band_run_tracers_at_overlapping_size(dtype, monkeypatch):
    """the 48 x 1440 x 24 band of test_band_run_chains_at_overlapping_size (kernels of tens of microseconds on every
    stream: a missing dependency between the tracer launches and the stage's chains shows here) with 4 tracers, in
    the four orchestrations: the product's chains, one stream (GCM_PE_SINGLE_STREAM=1), the exchange on the comm
    stream with a join per stage (GCM_BAND_COMM_STREAM=1), the edge rows dispatched first (GCM_BAND_OVERLAP=1);
    and the stage's two fallback paths: events recorded behind the kernels (GCM_PE_STOP_EVENTS=0), K1 of all rows in
    one launch (GCM_PE_K1_SPLIT=0)"""
    import torch
    import gcmiipy_amd as g
    H, W, L, dt, ntr = 48, 1440, 24, 1.0, 4
    geom = su.geom_of(H, W, L)
    ic, tr = su.initial(geom, ntr, from_q=True)
    want = su.single_run(g, geom, ic, tr, 5, dt, dtype=dtype)
    for env in ({}, {"GCM_PE_SINGLE_STREAM": "1"}, {"GCM_BAND_COMM_STREAM": "1"}, {"GCM_BAND_OVERLAP": "1"},
                {"GCM_PE_STOP_EVENTS": "0"}, {"GCM_PE_K1_SPLIT": "0"}):
        for k in ("GCM_PE_SINGLE_STREAM", "GCM_BAND_COMM_STREAM", "GCM_BAND_OVERLAP", "GCM_PE_STOP_EVENTS", "GCM_PE_K1_SPLIT"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c, eng, runner = su.loopback_band(g, torch, geom, ntr, dtype)
        assert runner.native
        c.set_state(*ic)
        c.set_tracers(tr)
        runner.run(2, dt)
        runner.run(3, dt)
        torch.cuda.synchronize()
        got = c.get_state(), c.get_tracers()
        c.close()
        su.assert_equal(got, want, env)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_eight_bands_with_tracers_and_physics_equal_single_domain(dtype):
    """8 latitude bands of a (24, 64, 1440) grid with 3 tracers, dynamics + solar_timestep for 3 steps in the order of
    gcm_band_run (two exchanges per step, none after the physics), ghost rows moved by device copies"""
    import torch
    import gcmiipy_amd as g
    H, W, L, steps, nb, dt, ntr = 64, 1440, 24, 3, 8, 60.0, 3
    geom = su.geom_of(H, W, L)
    (ic, tr), gt = su.initial(geom, ntr, from_q=True), inp.ground(H, W)
    ref = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype=dtype)
    ref.set_state(*ic)
    ref.set_ground(gt)
    ref.set_tracers(tr)
    for n in range(steps):
        ref.step(1, dt)
        ref.solar_step(geom, dt, UTC0 + n * dt)
    want = ref.get_state(), ref.get_tracers()
    ref.close()
    cores = su.bands(g, geom, nb, ic, tr, dtype=dtype, gt=gt)

    def solar(n):
        for c in cores:
            c.solar_step(geom, dt, UTC0 + n * dt)
    su.whole_steps(cores, torch, steps, dt, after=solar)
    su.assert_equal(su.gather(cores), want)


# ---------------------------------------------------------------- separate processes
GLOO_SHAPE = (14, 20, 5)        # H, W, L
RCCL_SHAPE = (23, 36, 9)
NTR = 2


def _reference(g, shape, steps, dt):
    geom = su.geom_of(*shape)
    ic, tr = su.initial(geom, NTR, from_q=True)
    return su.single_run(g, geom, ic, tr, steps, dt)


@pytest.mark.parametrize("overlap", [True, False])
def test_gloo_ranks_one_gpu(tmp_path, overlap):
    """two ranks in two processes on the one GPU, HipBandEngine + BandRunner over gloo: the default engine (edge-first
    phases, the split stage) and overlap=False (whole stages); the tracers gathered from the ranks are the single
    domain's"""
    import gcmiipy_amd as g
    su.spawn(su.gloo_tracer_worker, (2, overlap, str(tmp_path), GLOO_SHAPE, NTR, True, 1, None), 2)
    su.assert_equal(su.load_ranks(str(tmp_path), 2), _reference(g, GLOO_SHAPE, 3, 120.0), overlap)


def test_rccl_self_ring_native(tmp_path):
    """gcm_band_run over RCCL called directly, the band its own neighbour on both sides (the periodic single domain)"""
    import gcmiipy_amd as g
    su.spawn(su.rccl_tracer_worker, (str(tmp_path), RCCL_SHAPE, NTR, True, 1, None), 1)
    su.assert_equal(su.load_self(str(tmp_path)), _reference(g, RCCL_SHAPE, 5, 120.0))


# ---------------------------------------------------------------- refusals, message size, checkpoints
def test_refusals_and_halo_bytes():
    import torch
    import gcmiipy_amd as g
    from gcmiipy_amd import _lib
    from gcmiipy_amd.core import GcmError
    lib = _lib.lib
    H, W, L = 12, 20, 5
    geom = su.geom_of(H, W, L)
    q = inp.state(geom)[4]
    band = lambda dtype="f64", **kw: g.Core(_lib.PE25D, W, 6, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0,
                                            dtype=dtype, **kw)
    c = band()
    base = c.halo_bytes()
    assert base == 8 * 2 * W * (1 + 4 * L) + 8 * 2 * W          # unchanged without tracers
    one = np.ascontiguousarray(q[None, :, :6])
    assert lib.gcm_set_tracers(c._h, 1, one.ctypes.data) == _lib.ERR_UNSUPPORTED      # no declaration
    assert lib.gcm_set_band_tracers(c._h, 0) == _lib.OK
    assert lib.gcm_set_tracers(c._h, 1, one.ctypes.data) == _lib.ERR_UNSUPPORTED      # a declaration of 0
    assert lib.gcm_set_band_tracers(c._h, -1) == _lib.ERR_ARG
    assert lib.gcm_set_band_tracers(c._h, _lib.MAX_TRACERS + 1) == _lib.ERR_ARG
    assert lib.gcm_set_band_tracers(c._h, 3) == _lib.OK
    assert c.tracer_count == 3 and c.halo_bytes() == base + 3 * 8 * L * W
    assert not c.get_tracers().any()                              # zeros until set
    three = np.ascontiguousarray(np.repeat(one, 3, axis=0))
    for n, arr in ((1, one), (0, None), (4, np.repeat(one, 4, axis=0).copy())):
        assert lib.gcm_set_tracers(c._h, n, None if arr is None else arr.ctypes.data) == _lib.ERR_ARG
        assert "declared 3" in lib.gcm_last_error(c._h).decode()
    assert lib.gcm_set_tracers(c._h, 3, three.ctypes.data) == _lib.OK
    assert np.array_equal(c.get_tracers(), three)
    with pytest.raises(GcmError):
        c.get_tracers(star=True)                                  # no predictor yet
    bufs = [torch.empty(c.halo_bytes(), dtype=torch.uint8, device="cuda") for _ in range(4)]
    c.set_halo_buffers(bufs[0].data_ptr(), bufs[1].data_ptr())
    assert lib.gcm_set_band_tracers(c._h, 2) == _lib.ERR_STATE
    c.close()
    c = band("f32", band_tracers=2)
    assert c.halo_bytes() == 4 * 2 * W * (1 + 4 * L) + 8 * 2 * W + 2 * 4 * L * W
    c.set_exchange(*[b.data_ptr() for b in bufs])
    assert lib.gcm_set_band_tracers(c._h, 1) == _lib.ERR_STATE
    c.close()
    single = g.Core(_lib.PE25D, W, H, L, geom=geom)
    assert lib.gcm_set_band_tracers(single._h, 1) == _lib.ERR_UNSUPPORTED
    single.close()
    sw = g.Core(_lib.SW2D, 130, 8, dx=300e3, nranks=2, rank=0, global_height=16, row0=0)
    assert lib.gcm_set_band_tracers(sw._h, 1) == _lib.ERR_UNSUPPORTED
    sw.close()


def test_checkpoint_restores_band_tracers(tmp_path):
    """save both bands of a 2-band run with tracers, restore them into new handles (band_tracers comes back from the
    file's options) and go on: bit for bit the uninterrupted single domain"""
    import torch
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    H, W, L, dt, ntr = 16, 20, 5, 120.0, 2
    geom = su.geom_of(H, W, L)
    ic, tr = su.initial(geom, ntr, from_q=True)
    want = su.single_run(g, geom, ic, tr, 4, dt)
    cores = su.bands(g, geom, 2, ic, tr)
    su.whole_steps(cores, torch, 2, dt)
    for r, c in enumerate(cores):
        checkpoint.save(str(tmp_path / ("b%d.npz" % r)), c, step=2, geom=geom)
        c.close()
    cores = []
    for r in range(2):
        c, ck = checkpoint.restore(str(tmp_path / ("b%d.npz" % r)))
        assert ck["options"]["band_tracers"] == ntr and c.tracer_count == ntr
        cores.append(c)
    su.whole_steps(cores, torch, 2, dt)
    su.assert_equal(su.gather(cores), want)
