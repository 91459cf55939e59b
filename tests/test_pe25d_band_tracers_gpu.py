"""GPU tests of the passive tracers on GCM_PE25D latitude bands (gcm_set_band_tracers): every band path -- the
host-driven exchange (whole stages and the edge-first phases), gcm_band_run with the loopback exchange at a small
and at an overlapping size, eight bands of one grid, separate processes over gloo and over RCCL -- gives the single
domain's tracers and state bit for bit (the same kernel on the same inputs, fp64 and fp32 alike)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
UTC0 = 5 * 3600.0


def _ic_pe(geom):
    rng = np.random.default_rng(12)
    L, H, W = geom.layers, geom.height, geom.width
    p = 1e5 + 10 * rng.standard_normal((H, W))
    u = rng.standard_normal((L, H, W))
    v = rng.standard_normal((L, H, W))
    v[:, -1, :] = 0
    sig = np.asarray(geom.sig)
    t = (300 + rng.standard_normal((L, H, W))) * ((1e5 / (p * sig + geom.ptop)) ** (287.0 / 1004.0))
    q = 3e-6 * (1 + 0.1 * rng.random((L, H, W)))
    return p, u, v, t, q


def _ic_gt(H, W):
    return 288.0 + np.random.default_rng(13).standard_normal((H, W))


def _tracers(q, n, seed=14):
    """n tracers: the first a copy of q, the others positive noise of other magnitudes"""
    rng = np.random.default_rng(seed)
    c = [q] + [(k + 1.0) * (1 + 0.5 * rng.random(q.shape)) for k in range(n - 1)]
    return np.ascontiguousarray(np.stack(c)[:n])


def _rows(a, sl):
    """rows `sl` of a (…, H, W) array"""
    return np.ascontiguousarray(a[..., sl, :])


def _exchange(cores, torch):
    """ring exchange by device copies on the default stream: side s of a band lands in the neighbour's opposite ghost"""
    n = len(cores)
    bufs = [[torch.empty(c.halo_bytes(), dtype=torch.uint8, device="cuda") for _ in (0, 1)] for c in cores]
    for r, c in enumerate(cores):
        c.halo_pack(0, bufs[r][0].data_ptr())
        c.halo_pack(1, bufs[r][1].data_ptr())
    torch.cuda.synchronize()
    for r, c in enumerate(cores):
        c.halo_unpack(1, bufs[(r + 1) % n][0].data_ptr())
        c.halo_unpack(0, bufs[(r - 1) % n][1].data_ptr())
    torch.cuda.synchronize()


def _bands(g, geom, H, W, L, nb, ic, tr, dtype="f64", gt=None):
    from gcmiipy_amd.bands import split_rows
    cores = []
    for r, (row0, n) in enumerate(split_rows(H, nb)):
        c = g.Core(g._lib.PE25D, W, n, L, geom=geom, nranks=nb, rank=r, global_height=H, row0=row0, dtype=dtype,
                   band_tracers=tr.shape[0])
        sl = slice(row0, row0 + n)
        c.set_state(*[_rows(a, sl) for a in ic])
        c.set_tracers(_rows(tr, sl))
        if gt is not None:
            c.set_ground(gt[sl])
        cores.append(c)
    return cores


def _gather(cores):
    parts = [c.get_state() for c in cores]
    state = [np.concatenate([x[f] for x in parts], axis=0 if f == 0 else 1) for f in range(5)]
    return state, np.concatenate([c.get_tracers() for c in cores], axis=2)


def _assert_equal(got_state, got_tr, want_state, want_tr, what=""):
    for f in range(5):
        assert np.array_equal(got_state[f], want_state[f]), (what, "puvtq"[f])
    for n in range(want_tr.shape[0]):
        assert np.array_equal(got_tr[n], want_tr[n]), (what, "tracer", n)


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
    from gcmiipy_amd import geometry
    H, W, L, steps, dt = 16, 20, 5, 3, 120.0
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    geom.heightmap[H // 2, 3] = 300.0
    ic = _ic_pe(geom)
    tr = _tracers(ic[4], ntr)
    ref = g.Core(g._lib.PE25D, W, H, L, geom=geom)
    ref.set_state(*ic)
    ref.set_tracers(tr)
    ref.step(steps, dt)
    want, want_tr = ref.get_state(), ref.get_tracers()
    ref.close()
    cores = _bands(g, geom, H, W, L, nb, ic, tr)
    for c in cores:
        assert c.tracer_count == ntr
    _exchange(cores, torch)                              # the initial state's ghost rows
    for _ in range(steps):
        if mode == "whole":
            for c in cores:
                c.step_interior(dt)                      # predictor
            _exchange(cores, torch)
            for c in cores:
                c.step_boundary(dt)                      # corrector
            _exchange(cores, torch)
        else:
            for stage in (0, 1):
                for c in cores:
                    c.step_phase(2 * stage, dt)
                for c in cores:
                    c.step_phase(2 * stage + 1, dt)
                torch.cuda.synchronize()
                _exchange(cores, torch)
    got, got_tr = _gather(cores)
    for c in cores:
        c.close()
    _assert_equal(got, got_tr, want, want_tr, mode)
    assert np.array_equal(got_tr[0], got[4])             # the tracer that started as q is still q


def _loopback_band(g, torch, geom, H, W, L, ntr, dtype, overlap=True):
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0, dtype=dtype,
               stream=torch.cuda.current_stream().cuda_stream, band_tracers=ntr)
    eng = HipBandEngine(c, torch)
    runner = BandRunner(eng, 0, 2, LoopbackExchange(), north=0, south=0)
    assert runner.native
    return c, eng, runner


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("phys", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_band_run_loopback_equals_single_domain(dtype, phys, overlap):
    """gcm_band_run with the loopback exchange (the band is its own neighbour: the periodic single domain), runs of
    3 + 2 steps (the second starts from a primed state), then gcm_set_tracers between two runs: the next run exchanges
    the new tracers' ghost rows first"""
    import torch
    import gcmiipy_amd as g
    from gcmiipy_amd import geometry
    H, W, L, dt, ntr = 23, 36, 9, 120.0, 3
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    ic, gt = _ic_pe(geom), _ic_gt(H, W)
    tr0, tr1 = _tracers(ic[4], ntr), _tracers(ic[4], ntr, seed=15)[::-1].copy()

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

    ref = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype=dtype)
    want = drive(ref, lambda n: ref.step(n, dt), lambda: ref.set_physics(geom, UTC0))
    ref.close()
    c, eng, runner = _loopback_band(g, torch, geom, H, W, L, ntr, dtype)
    if overlap:
        c.set_band_overlap(True)

    def run(n):
        runner.run(n, dt)
        torch.cuda.synchronize()
    got = drive(c, run, lambda: eng.set_physics(geom, UTC0))
    c.close()
    for part, ((gs, gtr), (ws, wtr)) in enumerate(zip(got, want)):
        _assert_equal(gs, gtr, ws, wtr, part)
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
    from gcmiipy_amd import geometry
    H, W, L, dt, ntr = 48, 1440, 24, 1.0, 4
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    ic = _ic_pe(geom)
    tr = _tracers(ic[4], ntr)
    ref = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype=dtype)
    ref.set_state(*ic)
    ref.set_tracers(tr)
    ref.step(5, dt)
    want, want_tr = ref.get_state(), ref.get_tracers()
    ref.close()
    for env in ({}, {"GCM_PE_SINGLE_STREAM": "1"}, {"GCM_BAND_COMM_STREAM": "1"}, {"GCM_BAND_OVERLAP": "1"},
                {"GCM_PE_STOP_EVENTS": "0"}, {"GCM_PE_K1_SPLIT": "0"}):
        for k in ("GCM_PE_SINGLE_STREAM", "GCM_BAND_COMM_STREAM", "GCM_BAND_OVERLAP", "GCM_PE_STOP_EVENTS", "GCM_PE_K1_SPLIT"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c, eng, runner = _loopback_band(g, torch, geom, H, W, L, ntr, dtype)
        c.set_state(*ic)
        c.set_tracers(tr)
        runner.run(2, dt)
        runner.run(3, dt)
        torch.cuda.synchronize()
        got, got_tr = c.get_state(), c.get_tracers()
        c.close()
        _assert_equal(got, got_tr, want, want_tr, env)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_eight_bands_with_tracers_and_physics_equal_single_domain(dtype):
    """8 latitude bands of a (24, 64, 1440) grid with 3 tracers, dynamics + solar_timestep for 3 steps in the order of
    gcm_band_run (two exchanges per step, none after the physics), ghost rows moved by device copies"""
    import torch
    import gcmiipy_amd as g
    from gcmiipy_amd import geometry
    H, W, L, steps, nb, dt, ntr = 64, 1440, 24, 3, 8, 60.0, 3
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    ic, gt = _ic_pe(geom), _ic_gt(H, W)
    tr = _tracers(ic[4], ntr)
    ref = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype=dtype)
    ref.set_state(*ic)
    ref.set_ground(gt)
    ref.set_tracers(tr)
    for n in range(steps):
        ref.step(1, dt)
        ref.solar_step(geom, dt, UTC0 + n * dt)
    want, want_tr = ref.get_state(), ref.get_tracers()
    ref.close()
    cores = _bands(g, geom, H, W, L, nb, ic, tr, dtype, gt)
    _exchange(cores, torch)
    for n in range(steps):
        for c in cores:
            c.step_interior(dt)
        _exchange(cores, torch)
        for c in cores:
            c.step_boundary(dt)
        _exchange(cores, torch)
        for c in cores:
            c.solar_step(geom, dt, UTC0 + n * dt)
    got, got_tr = _gather(cores)
    for c in cores:
        c.close()
    _assert_equal(got, got_tr, want, want_tr)


# ---------------------------------------------------------------- separate processes
GLOO_SHAPE = (14, 20, 5)        # H, W, L
RCCL_SHAPE = (23, 36, 9)
NTR = 2


def _reference(g, geometry, shape, steps, dt):
    H, W, L = shape
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    ic = _ic_pe(geom)
    ref = g.Core(g._lib.PE25D, W, H, L, geom=geom)
    ref.set_state(*ic)
    ref.set_tracers(_tracers(ic[4], NTR))
    ref.step(steps, dt)
    out = ref.get_state(), ref.get_tracers()
    ref.close()
    return out


def _gloo_worker(rank, world, overlap, outdir):
    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    import gcmiipy_amd as g
    from gcmiipy_amd import geometry
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, split_rows
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(outdir, "rendezvous"), rank=rank, world_size=world)
    H, W, L = GLOO_SHAPE
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    ic = _ic_pe(geom)
    row0, n = split_rows(H, world)[rank]
    sl = slice(row0, row0 + n)
    c = g.Core(g._lib.PE25D, W, n, L, geom=geom, nranks=world, rank=rank, global_height=H, row0=row0,
               stream=torch.cuda.current_stream().cuda_stream, band_tracers=NTR)
    c.set_state(*[_rows(a, sl) for a in ic])
    c.set_tracers(_rows(_tracers(ic[4], NTR), sl))
    eng = HipBandEngine(c, torch, overlap=overlap, stream_aware=False)
    assert eng.edge_first == overlap
    runner = BandRunner(eng, rank, world, dist)
    runner.run(1, 120.0)
    runner.run(2, 120.0)
    torch.cuda.synchronize()
    np.savez(os.path.join(outdir, "r%d.npz" % rank), tr=c.get_tracers(), **dict(zip("puvtq", c.get_state())))
    c.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("overlap", [True, False])
def test_gloo_ranks_one_gpu(tmp_path, overlap):
    """two ranks in two processes on the one GPU, HipBandEngine + BandRunner over gloo: the default engine (edge-first
    phases, the split stage) and overlap=False (whole stages); the tracers gathered from the ranks are the single
    domain's"""
    import torch.multiprocessing as mp
    import gcmiipy_amd as g
    from gcmiipy_amd import geometry
    mp.spawn(_gloo_worker, args=(2, overlap, str(tmp_path)), nprocs=2, join=True)
    parts = [np.load(os.path.join(str(tmp_path), "r%d.npz" % r)) for r in range(2)]
    want, want_tr = _reference(g, geometry, GLOO_SHAPE, 3, 120.0)
    got = [np.concatenate([x[k] for x in parts], axis=0 if k == "p" else 1) for k in "puvtq"]
    _assert_equal(got, np.concatenate([x["tr"] for x in parts], axis=2), want, want_tr, overlap)


def _rccl_worker(rank, outdir):
    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    import gcmiipy_amd as g
    from gcmiipy_amd import geometry
    from gcmiipy_amd.bands import BandRunner, HipBandEngine
    from gcmiipy_amd.rccl import RcclP2P
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="file://" + os.path.join(outdir, "rendezvous"), rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    ring = RcclP2P(None, 0, 1, uid_bytes=RcclP2P.new_unique_id())
    H, W, L = RCCL_SHAPE
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    ic = _ic_pe(geom)
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0,
               stream=torch.cuda.current_stream().cuda_stream, band_tracers=NTR)
    c.set_state(*ic)
    c.set_tracers(_tracers(ic[4], NTR))
    runner = BandRunner(HipBandEngine(c, torch), 0, 2, ring, north=0, south=0)
    assert runner.native
    runner.run(3, 120.0)
    runner.run(2, 120.0)
    torch.cuda.synchronize()
    np.savez(os.path.join(outdir, "self.npz"), tr=c.get_tracers(), **dict(zip("puvtq", c.get_state())))
    c.close()
    ring.close()
    dist.destroy_process_group()


def test_rccl_self_ring_native(tmp_path):
    """gcm_band_run over RCCL called directly, the band its own neighbour on both sides (the periodic single domain)"""
    import torch.multiprocessing as mp
    import gcmiipy_amd as g
    from gcmiipy_amd import geometry
    mp.spawn(_rccl_worker, args=(str(tmp_path),), nprocs=1, join=True)
    got = np.load(os.path.join(str(tmp_path), "self.npz"))
    want, want_tr = _reference(g, geometry, RCCL_SHAPE, 5, 120.0)
    _assert_equal([got[k] for k in "puvtq"], got["tr"], want, want_tr)


# ---------------------------------------------------------------- refusals, message size, checkpoints
def test_refusals_and_halo_bytes():
    import torch
    import gcmiipy_amd as g
    from gcmiipy_amd import _lib, geometry
    from gcmiipy_amd.core import GcmError
    lib = _lib.lib
    H, W, L = 12, 20, 5
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    q = _ic_pe(geom)[4]
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
    from gcmiipy_amd import checkpoint, geometry
    H, W, L, dt, ntr = 16, 20, 5, 120.0, 2
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    ic = _ic_pe(geom)
    tr = _tracers(ic[4], ntr)
    ref = g.Core(g._lib.PE25D, W, H, L, geom=geom)
    ref.set_state(*ic)
    ref.set_tracers(tr)
    ref.step(4, dt)
    want, want_tr = ref.get_state(), ref.get_tracers()
    ref.close()

    def steps(cores, n):
        _exchange(cores, torch)
        for _ in range(n):
            for c in cores:
                c.step_interior(dt)
            _exchange(cores, torch)
            for c in cores:
                c.step_boundary(dt)
            _exchange(cores, torch)
    cores = _bands(g, geom, H, W, L, 2, ic, tr)
    steps(cores, 2)
    for r, c in enumerate(cores):
        checkpoint.save(str(tmp_path / ("b%d.npz" % r)), c, step=2, geom=geom)
        c.close()
    cores = []
    for r in range(2):
        c, ck = checkpoint.restore(str(tmp_path / ("b%d.npz" % r)))
        assert ck["options"]["band_tracers"] == ntr and c.tracer_count == ntr
        cores.append(c)
    steps(cores, 2)
    got, got_tr = _gather(cores)
    for c in cores:
        c.close()
    _assert_equal(got, got_tr, want, want_tr)
