"""The single-domain and band set-ups of tests/test_pe25d_tracer_forcing_gpu.py: the same arrangements as
tests/test_pe25d_band_van_leer_gpu.py drives (seeded inputs from band_van_leer_inputs, in-process bands with ghost rows
moved by device copies, whole stages and edge-first phases, the loopback band of gcm_band_run), kept here as this
file's own so that neither test file depends on the other's private helpers.  Beyond those: the ghost depth, the scheme
and the zonal filter are arguments (an odd width needs filter=False).  TEST INFRASTRUCTURE, no test in here."""
import numpy as np

import band_van_leer_inputs as inp

UTC0 = 5 * 3600.0
ORCH_ENV = ("GCM_PE_SINGLE_STREAM", "GCM_BAND_COMM_STREAM", "GCM_BAND_HOST_LOOP", "GCM_BAND_OVERLAP")


def geom_of(H, W, L):
    from gcmiipy_amd import geometry
    return geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)


def initial(geom, ntr, seed=inp.TRACER_SEED):
    H, W, L = geom.height, geom.width, geom.layers
    return inp.state(H, W, L, np.asarray(geom.sig), geom.ptop), inp.tracers(H, W, L, ntr, seed)


def ground(H, W):
    return 288.0 + np.random.default_rng(13).standard_normal((H, W))


def single(g, geom, st, trs, recs=None, dtype="f64", scheme="van_leer", filter=True):
    """a single-domain handle with state, tracers and the forcing records {i: dict} registered"""
    c = g.Core(g._lib.PE25D, geom.width, geom.height, geom.layers, geom=geom, dtype=dtype, tracer_scheme=scheme,
               filter=filter)
    c.set_state(*st)
    c.set_tracers(trs)
    for i, rec in (recs or {}).items():
        c.set_tracer_forcing(i, **rec)
    return c


def band_rows(rec, sl):
    """the forcing record of a band that owns rows `sl`"""
    out = dict(rec)
    for k in ("emission", "pin_mask"):
        if out.get(k) is not None:
            out[k] = np.ascontiguousarray(out[k][:, sl, :])
    return out


def bands(g, geom, nb, st, trs, recs=None, dtype="f64", scheme="van_leer", rows=2, filter=True):
    """nb in-process bands with their own rows of state, tracers and forcing fields"""
    from gcmiipy_amd.bands import split_rows
    H, W, L = geom.height, geom.width, geom.layers
    cores = []
    for r, (row0, n) in enumerate(split_rows(H, nb)):
        c = g.Core(g._lib.PE25D, W, n, L, geom=geom, nranks=nb, rank=r, global_height=H, row0=row0, dtype=dtype,
                   band_tracers=trs.shape[0], band_tracer_rows=rows, tracer_scheme=scheme, filter=filter)
        assert c.band_tracer_rows == rows
        sl = slice(row0, row0 + n)
        c.set_state(*[inp.rows(a, sl) for a in st])
        c.set_tracers(inp.rows(trs, sl))
        for i, rec in (recs or {}).items():
            c.set_tracer_forcing(i, **band_rows(rec, sl))
        cores.append(c)
    return cores


def exchange(cores, torch):
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


def whole_steps(cores, torch, n, dt, prime=True):
    """whole stages, two exchanges per step (the order of gcm_band_run)"""
    if prime:
        exchange(cores, torch)
    for _ in range(n):
        for c in cores:
            c.step_interior(dt)                      # predictor
        exchange(cores, torch)
        for c in cores:
            c.step_boundary(dt)                      # corrector
        exchange(cores, torch)


def phase_steps(cores, torch, n, dt):
    """the edge-first phases (the split stage), an exchange behind each stage"""
    exchange(cores, torch)
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


def loopback_band(g, torch, geom, ntr, dtype, scheme="van_leer", rows=2):
    """the band that is its own neighbour, driven by gcm_band_run"""
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange
    H, W, L = geom.height, geom.width, geom.layers
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0, dtype=dtype,
               stream=torch.cuda.current_stream().cuda_stream, band_tracers=ntr, band_tracer_rows=rows,
               tracer_scheme=scheme)
    eng = HipBandEngine(c, torch)
    runner = BandRunner(eng, 0, 2, LoopbackExchange(), north=0, south=0)
    return c, eng, runner
