"""Device set-ups shared by the GPU tests: the `g` fixture, the product geometry, single-domain handles, in-process
latitude bands with ghost rows moved by device copies (whole stages and edge-first phases), the loopback band of
gcm_band_run, and the child processes of the band tests (started under a time limit; the gloo and the RCCL self-ring
worker of the GCM_PE25D tracer bands).  A test module imports `g` by name: pytest collects a fixture that is present in
the module's namespace.  The seeded inputs are those of tests/pe25d_inputs.py.  TEST INFRASTRUCTURE, no test in here."""
import os
import sys

import numpy as np
import pytest

import pe25d_inputs as inp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
UTC0 = inp.UTC0
ORCH_ENV = ("GCM_PE_SINGLE_STREAM", "GCM_BAND_COMM_STREAM", "GCM_BAND_HOST_LOOP", "GCM_BAND_OVERLAP")
WORKER_TIMEOUT = 240            # seconds, each child process


@pytest.fixture(scope="module")
def g():
    import gcmiipy_amd
    assert gcmiipy_amd.device_count() >= 1, "no MI355X visible"
    return gcmiipy_amd


def geom_of(H, W, L, ptop=0.0, bump=False):
    """the product's geometry on manabe's sigma levels; bump: one 1500 m peak"""
    from gcmiipy_amd import geometry
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    geom.ptop = ptop
    if bump:
        geom.heightmap[H // 2, W // 3] = 1500.0
    return geom


def geoms_of(H, W, L, ptop=0.0, bump=False):
    """the product's geometry and the oracle's, with the same top pressure and topography"""
    from oracle import geometry as ogeo
    og = ogeo.gen_geometry(H, W, L, sig_func=ogeo.manabe_sig)
    og.ptop = ptop
    if bump:
        og.heightmap[H // 2, W // 3] = 1500.0
    return geom_of(H, W, L, ptop, bump), og


def initial(geom, ntr, from_q=False):
    """the seeded state and ntr tracers: inp.tracers, or (from_q) inp.tracers_from_q, whose first tracer is q"""
    st = inp.state(geom)
    trs = inp.tracers_from_q(st[4], ntr) if from_q else inp.tracers(geom.height, geom.width, geom.layers, ntr)
    return st, trs


def single(g, geom, st=None, trs=None, *, dtype="f64", scheme=None, filter=True, gt=None, phys=False, hs=None, every=None,
           recs=None):
    """a single-domain handle: state, tracers, ground temperature, then what is registered -- the column physics at
    UTC0, Held-Suarez with the parameters hs ({}: the defaults), the climatology every `every` steps, the tracer
    forcing records {i: dict}"""
    c = g.Core(g._lib.PE25D, geom.width, geom.height, geom.layers, geom=geom, dtype=dtype, tracer_scheme=scheme,
               filter=filter)
    if st is not None:
        c.set_state(*st)
    if trs is not None:
        c.set_tracers(trs)
    if gt is not None:
        c.set_ground(gt)
    if phys:
        c.set_physics(geom, UTC0)
    if hs is not None:
        c.set_held_suarez(geom, **hs)
    if every is not None:
        c.set_climate(every)
    for i, rec in (recs or {}).items():
        c.set_tracer_forcing(i, **rec)
    return c


def single_run(g, geom, st, trs, steps, dt, **kw):
    """(state, tracers) of single(...) after `steps` steps"""
    one = single(g, geom, st, trs, **kw)
    one.step(steps, dt)
    out = one.get_state(), one.get_tracers()
    one.close()
    return out


def band_rows(rec, sl):
    """the forcing record of a band that owns rows `sl`"""
    out = dict(rec)
    for k in ("emission", "pin_mask"):
        if out.get(k) is not None:
            out[k] = np.ascontiguousarray(out[k][:, sl, :])
    return out


def bands(g, geom, nb, st, trs=None, *, dtype="f64", scheme=None, rows=1, filter=True, gt=None, recs=None):
    """nb in-process bands (split_rows) with their own rows of state, tracers, ground temperature and forcing fields;
    depth, scheme and message size are checked against what the arguments say"""
    from gcmiipy_amd.bands import split_rows
    H, W, L = geom.height, geom.width, geom.layers
    ntr = 0 if trs is None else trs.shape[0]
    cores = []
    for r, (row0, n) in enumerate(split_rows(H, nb)):
        c = g.Core(g._lib.PE25D, W, n, L, geom=geom, nranks=nb, rank=r, global_height=H, row0=row0, dtype=dtype,
                   band_tracers=ntr, band_tracer_rows=rows, tracer_scheme=scheme, filter=filter)
        assert c.band_tracer_rows == rows and c.tracer_scheme == g.core.tracer_scheme_id(scheme)
        assert c.tracer_count == ntr
        assert c.halo_bytes() == inp.halo_bytes(W, L, 8 if dtype == "f64" else 4, ntr, rows)
        sl = slice(row0, row0 + n)
        c.set_state(*[inp.rows(a, sl) for a in st])
        if trs is not None:
            c.set_tracers(inp.rows(trs, sl))
        if gt is not None:
            c.set_ground(gt[sl])
        for i, rec in (recs or {}).items():
            c.set_tracer_forcing(i, **band_rows(rec, sl))
        cores.append(c)
    return cores


def pack(cores, torch):
    """both edges of every band packed into new device buffers (bytes: they serve both real types and the 2-D models);
    not synchronised"""
    bufs = [[torch.empty(c.halo_bytes(), dtype=torch.uint8, device="cuda") for _ in (0, 1)] for c in cores]
    for r, c in enumerate(cores):
        c.halo_pack(0, bufs[r][0].data_ptr())
        c.halo_pack(1, bufs[r][1].data_ptr())
    return bufs


def unpack(cores, bufs, torch):
    """side s of a band lands in the neighbour's opposite ghost; synchronised"""
    n = len(cores)
    for r, c in enumerate(cores):
        c.halo_unpack(1, bufs[(r + 1) % n][0].data_ptr())   # south ghost <- southern band's north edge
        c.halo_unpack(0, bufs[(r - 1) % n][1].data_ptr())   # north ghost <- northern band's south edge
    torch.cuda.synchronize()


def exchange(cores, torch):
    """ring exchange by device copies on the default stream, with a synchronize() after each half"""
    bufs = pack(cores, torch)
    torch.cuda.synchronize()
    unpack(cores, bufs, torch)


def whole_steps(cores, torch, n, dt, prime=True, after=None):
    """whole stages, two exchanges per step (the order of gcm_band_run); after(k): the explicit physics calls of step
    k, on own rows and ghost rows, behind the second exchange"""
    if prime:
        exchange(cores, torch)
    for k in range(n):
        for c in cores:
            c.step_interior(dt)                      # predictor
        exchange(cores, torch)
        for c in cores:
            c.step_boundary(dt)                      # corrector
        exchange(cores, torch)
        if after is not None:
            after(k)


def phase_steps(cores, torch, n, dt):
    """the edge-first phases (the split stage), an exchange behind each stage"""
    exchange(cores, torch)                           # the initial state's ghost rows
    for _ in range(n):
        for stage in (0, 1):
            for c in cores:
                c.step_phase(2 * stage, dt)
            for c in cores:
                c.step_phase(2 * stage + 1, dt)
            torch.cuda.synchronize()
            exchange(cores, torch)


def gather(cores, close=True):
    parts = [c.get_state() for c in cores]
    state = [np.concatenate([x[f] for x in parts], axis=0 if f == 0 else 1) for f in range(5)]
    tr = np.concatenate([c.get_tracers() for c in cores], axis=2)
    if close:
        for c in cores:
            c.close()
    return state, tr


def assert_equal(got, want, what=""):
    (gs, gtr), (ws, wtr) = got, want
    for f in range(5):
        assert np.array_equal(gs[f], ws[f]), (what, "puvtq"[f])
    assert gtr.shape == wtr.shape
    for n in range(wtr.shape[0]):
        assert np.array_equal(gtr[n], wtr[n]), (what, "tracer", n)


def loopback_band(g, torch, geom, ntr=0, dtype="f64", *, scheme=None, rows=1, gt=None, phys=False, hs=None, every=None):
    """the band that is its own neighbour, driven by gcm_band_run: (handle, engine, runner).  gt, phys, hs and every are
    set on the engine ahead of the runner (which registers the exchange); whether the runner is native is the caller's
    to assert"""
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange
    H, W, L = geom.height, geom.width, geom.layers
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0, dtype=dtype,
               stream=torch.cuda.current_stream().cuda_stream, band_tracers=ntr, band_tracer_rows=rows,
               tracer_scheme=scheme)
    eng = HipBandEngine(c, torch)
    if gt is not None:
        c.set_ground(gt)
    if phys:
        eng.set_physics(geom, UTC0)
    if hs is not None:
        eng.set_held_suarez(geom, **hs)
    if every is not None:
        eng.set_climate(every)
    runner = BandRunner(eng, 0, 2, LoopbackExchange(), north=0, south=0)
    return c, eng, runner


# ---------------------------------------------------------------- child processes
def worker_paths():
    """first thing in a child process: the repository root and tests/ on sys.path"""
    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)


def spawn(fn, args, nprocs):
    """fresh child processes (spawn), each under its own time limit; no retries: a child that is late is killed and
    the test fails"""
    import torch.multiprocessing as mp
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    try:
        for p in ctx.processes:
            p.join(WORKER_TIMEOUT)
        late = [p.pid for p in ctx.processes if p.is_alive()]
        assert not late, "worker processes still running after %d s: %s" % (WORKER_TIMEOUT, late)
        while not ctx.join(timeout=5):
            pass                                             # (all have exited: this collects their exit status)
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
                p.join(10)


def _save(path, c):
    np.savez(path, tr=c.get_tracers(), **dict(zip("puvtq", c.get_state())))


def gloo_tracer_worker(rank, world, overlap, outdir, shape, ntr, from_q, rows, scheme):
    """one of `world` GCM_PE25D tracer bands on the one GPU, HipBandEngine + BandRunner over gloo, 1 + 2 steps of 120 s;
    leaves r<rank>.npz in outdir"""
    worker_paths()
    import torch
    import torch.distributed as dist
    import gcmiipy_amd as g
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, split_rows
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(outdir, "rendezvous"), rank=rank, world_size=world)
    H, W, L = shape
    geom = geom_of(H, W, L)
    st, trs = initial(geom, ntr, from_q)
    row0, n = split_rows(H, world)[rank]
    sl = slice(row0, row0 + n)
    c = g.Core(g._lib.PE25D, W, n, L, geom=geom, nranks=world, rank=rank, global_height=H, row0=row0,
               stream=torch.cuda.current_stream().cuda_stream, band_tracers=ntr, band_tracer_rows=rows,
               tracer_scheme=scheme)
    c.set_state(*[inp.rows(a, sl) for a in st])
    c.set_tracers(inp.rows(trs, sl))
    eng = HipBandEngine(c, torch, overlap=overlap, stream_aware=False)
    assert eng.edge_first == overlap
    runner = BandRunner(eng, rank, world, dist)
    runner.run(1, 120.0)
    runner.run(2, 120.0)
    torch.cuda.synchronize()
    _save(os.path.join(outdir, "r%d.npz" % rank), c)
    c.close()
    dist.barrier()
    dist.destroy_process_group()


def rccl_tracer_worker(rank, outdir, shape, ntr, from_q, rows, scheme):
    """gcm_band_run over RCCL called directly on a GCM_PE25D tracer band that is its own neighbour on both sides, 3 + 2
    steps of 120 s; leaves self.npz in outdir"""
    worker_paths()
    import torch
    import torch.distributed as dist
    import gcmiipy_amd as g
    from gcmiipy_amd.bands import BandRunner, HipBandEngine
    from gcmiipy_amd.rccl import RcclP2P
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="file://" + os.path.join(outdir, "rendezvous"), rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    ring = RcclP2P(None, 0, 1, uid_bytes=RcclP2P.new_unique_id())
    H, W, L = shape
    geom = geom_of(H, W, L)
    st, trs = initial(geom, ntr, from_q)
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0,
               stream=torch.cuda.current_stream().cuda_stream, band_tracers=ntr, band_tracer_rows=rows,
               tracer_scheme=scheme)
    c.set_state(*st)
    c.set_tracers(trs)
    runner = BandRunner(HipBandEngine(c, torch), 0, 2, ring, north=0, south=0)
    assert runner.native
    runner.run(3, 120.0)
    runner.run(2, 120.0)
    torch.cuda.synchronize()
    _save(os.path.join(outdir, "self.npz"), c)
    c.close()
    ring.close()
    dist.destroy_process_group()


def load_ranks(outdir, world):
    """(state, tracers) put together from the r<rank>.npz files of gloo_tracer_worker"""
    parts = [np.load(os.path.join(outdir, "r%d.npz" % r)) for r in range(world)]
    state = [np.concatenate([x[k] for x in parts], axis=0 if k == "p" else 1) for k in "puvtq"]
    return state, np.concatenate([x["tr"] for x in parts], axis=2)


def load_self(outdir):
    """(state, tracers) from the self.npz of rccl_tracer_worker"""
    got = np.load(os.path.join(outdir, "self.npz"))
    return [got[k] for k in "puvtq"], got["tr"]
