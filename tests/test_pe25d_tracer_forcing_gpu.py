"""GPU tests of the tracer forcing of GCM_PE25D (gcm_set_tracer_forcing / Core.set_tracer_forcing): source, decay,
emission and pinned cells, applied on the device right behind the corrector.  The kernel rounds every operation on its
own, so the criterion is np.array_equal throughout: with the NumPy restatement (tests/pe25d_tracer_forcing_ref.py)
applied on the host to an unforced handle's result, with the get / force / set round trip per step that the forcing
replaces, and -- on latitude bands, under every orchestration -- with the forced single domain."""
import numpy as np
import pytest

import gpu_setups as su
import pe25d_inputs as inp
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)
from pe25d_tracer_forcing_ref import force, records

pytestmark = pytest.mark.gpu
SCHEMES = ["centred", "upwind", "van_leer"]
NTR = 4


def _setup(H, W, L):
    geom = su.geom_of(H, W, L)
    st, trs = su.initial(geom, NTR)
    return geom, st, trs, records(L, H, W, int(np.argmax(np.asarray(geom.sig))))


def _force_all(tr, dt, recs, dtype):
    """the restatement on every forced tracer of (n, L, H, W) float64 values that the type holds exactly"""
    out = tr.copy()
    for i, rec in recs.items():
        out[i] = force(tr[i], dt, rec, dtype)
    return out


def _equal_state(a, b, what=""):
    for f in range(5):
        assert np.array_equal(a[f], b[f]), (what, "puvtq"[f])


# ---------------------------------------------------------------- 1. one step
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(24, 36, 9), (6, 10, 3)])
def test_one_step_bit_for_bit(g, shape, dtype, scheme):
    """(H, W, L) = (24, 36, 9) and (6, 10, 3): a single domain's corrector is one run of all rows from an aligned own row
    0, so these cases take the wide path only, in several workgroups and in less than one (the runs that start or end
    off a 16-byte boundary: test_runs_off_a_16_byte_boundary).  Handle A steps unforced and the restatement is
    applied to what it returns; handle B steps forced: equal bits.  The unforced tracer, the state and the predictor's
    tracers are A's"""
    H, W, L = shape
    dt = 120.0
    geom, st, trs, recs = _setup(H, W, L)
    a = su.single(g, geom, st, trs, dtype=dtype, scheme=scheme)
    b = su.single(g, geom, st, trs, recs=recs, dtype=dtype, scheme=scheme)
    assert [b.tracer_forcing(i) is not None for i in range(NTR)] == [False, True, True, True]
    assert np.array_equal(b.get_tracers(), a.get_tracers())       # registering applies nothing
    a.step(1, dt)
    b.step(1, dt)
    ta, tb = a.get_tracers(), b.get_tracers()
    want = _force_all(ta, dt, recs, dtype)
    for i in range(NTR):
        assert np.array_equal(tb[i], want[i]), (shape, dtype, scheme, "tracer", i)
    assert np.array_equal(tb[0], ta[0])
    for i in (1, 2, 3):
        assert not np.array_equal(tb[i], ta[i])
    assert not tb[3][int(np.argmax(np.asarray(geom.sig)))].any()  # the clock's source region
    _equal_state(b.get_state(), a.get_state(), (shape, dtype, scheme))
    # the two stages by hand (the predictor's tracers can be read between them only): the predictor forces nothing
    # -- the star tracers are the unforced handle's, the current ones untouched -- and the corrector does
    c = su.single(g, geom, st, trs, recs=recs, dtype=dtype, scheme=scheme)
    d = su.single(g, geom, st, trs, dtype=dtype, scheme=scheme)
    t0 = c.get_tracers()
    c.half_step(0, dt)
    d.half_step(0, dt)
    assert np.array_equal(c.get_tracers(star=True), d.get_tracers(star=True))
    assert np.array_equal(c.get_tracers(), t0)
    c.half_step(1, dt)
    d.half_step(1, dt)
    assert np.array_equal(c.get_tracers(), tb) and np.array_equal(d.get_tracers(), ta)
    for x in (a, b, c, d):
        x.close()


# ---------------------------------------------------------------- 2. n steps in one call
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_five_steps_in_one_call_equal_the_round_trips(g, dtype):
    """B runs step(5) in one call; A runs five rounds of step(1), get, force, set_tracers -- the workaround the forcing
    replaces.  Then both go on with another dt: fac follows it"""
    H, W, L = 24, 36, 9
    geom, st, trs, recs = _setup(H, W, L)
    a = su.single(g, geom, st, trs, dtype=dtype, scheme="van_leer")
    b = su.single(g, geom, st, trs, recs=recs, dtype=dtype, scheme="van_leer")

    def rounds(n, dt):
        for _ in range(n):
            a.step(1, dt)
            a.set_tracers(_force_all(a.get_tracers(), dt, recs, dtype))

    rounds(5, 120.0)
    b.step(5, 120.0)
    assert np.array_equal(b.get_tracers(), a.get_tracers())
    _equal_state(b.get_state(), a.get_state())
    rounds(2, 45.0)
    b.step(2, 45.0)
    tb = b.get_tracers()
    assert np.array_equal(tb, a.get_tracers())
    # (had fac stayed at dt = 120 the decaying tracers would differ)
    stale = {i: dict(r, decay=r.get("decay", 0.0) * 120.0 / 45.0) for i, r in recs.items()}
    assert not np.array_equal(_force_all(tb, 45.0, stale, dtype)[1], _force_all(tb, 45.0, recs, dtype)[1])
    a.close()
    b.close()


# ---------------------------------------------------------------- 3. bands
def _forced_single(g, geom, st, trs, recs, steps, dt, dtype="f64", runs=None):
    one = su.single(g, geom, st, trs, recs=recs, dtype=dtype, scheme="van_leer")
    for n in (runs or [steps]):
        one.step(n, dt)
    out = one.get_state(), one.get_tracers()
    one.close()
    return out


@pytest.mark.parametrize("nb", [2, 3])
@pytest.mark.parametrize("mode", ["whole", "phase"])
def test_host_driven_forced_bands_equal_single_domain(g, mode, nb):
    """host-driven bands with real neighbours, whole stages and edge-first phases; the fields of a band are its own
    rows.  The neighbour's ghost rows come from forced edge rows: one unforced message would show after a step"""
    import torch
    H, W, L, steps, dt = 16, 20, 5, 3, 120.0
    geom, st, trs, recs = _setup(H, W, L)
    want = _forced_single(g, geom, st, trs, recs, steps, dt)
    cores = su.bands(g, geom, nb, st, trs, recs=recs, scheme="van_leer", rows=2)
    if mode == "whole":
        su.whole_steps(cores, torch, steps, dt)
    else:
        su.phase_steps(cores, torch, steps, dt)
    su.assert_equal(su.gather(cores), want, (mode, nb))


def test_unsplittable_short_forced_bands_equal_single_domain(g):
    """bands of 4 and 3 rows: the one tracer launch of the edge rows, and the forcing behind it"""
    import torch
    H, W, L, steps, dt = 14, 20, 5, 3, 120.0
    geom, st, trs, recs = _setup(H, W, L)
    want = _forced_single(g, geom, st, trs, recs, steps, dt)
    cores = su.bands(g, geom, 4, st, trs, recs=recs, scheme="van_leer", rows=2)
    assert sorted(c.H for c in cores) == [3, 3, 4, 4]
    su.phase_steps(cores, torch, steps, dt)
    su.assert_equal(su.gather(cores), want)


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("phys", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_forced_band_run_loopback_equals_single_domain(g, dtype, phys, overlap):
    """gcm_band_run with the loopback exchange at 23 x 36 x 9, runs of 3 + 2 steps, with and without gcm_set_band_overlap
    and the column physics"""
    import torch
    H, W, L, dt = 23, 36, 9, 120.0
    geom, st, trs, recs = _setup(H, W, L)
    gt = inp.ground(H, W)

    def drive(core, run, set_physics):
        if phys:
            core.set_ground(gt)
            set_physics()
        run(3)
        run(2)
        return core.get_state(), core.get_tracers()

    ref = su.single(g, geom, st, trs, recs=recs, dtype=dtype, scheme="van_leer")
    want = drive(ref, lambda n: ref.step(n, dt), lambda: ref.set_physics(geom, su.UTC0))
    ref.close()
    c, eng, runner = su.loopback_band(g, torch, geom, NTR, dtype, scheme="van_leer", rows=2)
    assert runner.native
    if overlap:
        c.set_band_overlap(True)
    c.set_state(*st)
    c.set_tracers(trs)
    for i, rec in recs.items():
        c.set_tracer_forcing(i, **rec)

    def run(n):
        runner.run(n, dt)
        torch.cuda.synchronize()
    got = drive(c, run, lambda: eng.set_physics(geom, su.UTC0))
    c.close()
    su.assert_equal(got, want, (dtype, phys, overlap))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_forced_band_run_at_overlapping_size(g, dtype, monkeypatch):
    """the 48 x 1440 x 24 loopback band with 4 tracers (three forced) under the default orchestration, one stream, the
    comm stream, the host-driven sequence and the edge rows first: kernels of tens of microseconds on every stream, so
    a forcing launch that raced the pack or the next stage would show.  Each orchestration runs once"""
    import torch
    H, W, L, dt = 48, 1440, 24, 1.0
    geom, st, trs, recs = _setup(H, W, L)
    want = _forced_single(g, geom, st, trs, recs, 5, dt, dtype)
    plain = su.single(g, geom, st, trs, dtype=dtype, scheme="van_leer")
    plain.step(5, dt)
    assert not np.array_equal(want[1][1], plain.get_tracers()[1])
    plain.close()
    for env in ({}, {"GCM_PE_SINGLE_STREAM": "1"}, {"GCM_BAND_COMM_STREAM": "1"}, {"GCM_BAND_HOST_LOOP": "1"},
                {"GCM_BAND_OVERLAP": "1"}):
        for k in su.ORCH_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c, eng, runner = su.loopback_band(g, torch, geom, NTR, dtype, scheme="van_leer", rows=2)
        assert runner.native == ("GCM_BAND_HOST_LOOP" not in env)
        c.set_state(*st)
        c.set_tracers(trs)
        for i, rec in recs.items():
            c.set_tracer_forcing(i, **rec)
        runner.run(2, dt)
        runner.run(3, dt)
        torch.cuda.synchronize()
        got = c.get_state(), c.get_tracers()
        c.close()
        su.assert_equal(got, want, env)


# ---------------------------------------------------------------- 3b. runs off a 16-byte boundary
def _full_records(L, H, W, k0):
    """every forced tracer with an emission AND a mask (all three requests of a lane), none of them uniform in a row"""
    rng = np.random.default_rng(33)
    recs = {}
    for i in (1, 2, 3):
        mask = rng.random((L, H, W)) < 0.3
        mask[k0] = True
        recs[i] = dict(source=0.01 * i, decay=1.0e-4 * i, emission=1e-3 * rng.random((L, H, W)), pin_mask=mask,
                       pin_value=-1.5 * i)
    return recs


@pytest.mark.parametrize("case", [("f32", 12, 10, 3, 2, "upwind", True), ("f32", 16, 10, 3, 3, "centred", True),
                                  ("f64", 12, 9, 3, 2, "upwind", False), ("f64", 15, 9, 3, 3, "centred", False)],
                         ids=lambda c: "%s-H%d-W%d-nb%d-%s" % (c[0], c[1], c[2], c[4], c[5]))
def test_runs_off_a_16_byte_boundary(g, case):
    """Bands with ONE tracer ghost row and rows of L W = 30 floats (120 bytes) or 27 doubles (216 bytes; an odd width
    needs the zonal filter off): own row 0 of a field lies 8 bytes past a 16-byte boundary (in a 6-row band of every
    field, in a 5-row band of every other one: both placements in one launch), so the emission and the mask are
    placed 8 bytes (2 and 1 bytes) into their allocations, and in the edge-first phases every run -- rows [0, 2),
    [H - 2, H) and the interior rows between -- starts with a head of 2 floats (1 double) in front of the first whole
    vector; the 60-float runs end in a tail of 2, the 54-double runs in a tail of 1, and a 5-row band has an interior
    run of one row.  The fp64 single domain's run of H 27 doubles ends in a tail of 1 where H is odd.  Every forced
    tracer carries an emission and a mask.  The bands equal the forced single domain, and that equals step(1), get,
    force(), set_tracers on an unforced handle"""
    import torch
    dtype, H, W, L, nb, scheme, filt = case
    steps, dt = 2, 120.0
    geom = su.geom_of(H, W, L)
    st, trs = su.initial(geom, NTR)
    recs = _full_records(L, H, W, int(np.argmax(np.asarray(geom.sig))))
    one = su.single(g, geom, st, trs, recs=recs, dtype=dtype, scheme=scheme, filter=filt)
    ref = su.single(g, geom, st, trs, dtype=dtype, scheme=scheme, filter=filt)
    for _ in range(steps):
        one.step(1, dt)
        ref.step(1, dt)
        ref.set_tracers(_force_all(ref.get_tracers(), dt, recs, dtype))
    want = one.get_state(), one.get_tracers()
    su.assert_equal(want, (ref.get_state(), ref.get_tracers()), (case, "restatement"))
    one.close()
    ref.close()
    for mode in ("phase", "whole"):
        cores = su.bands(g, geom, nb, st, trs, recs=recs, dtype=dtype, scheme=scheme, rows=1, filter=filt)
        if mode == "phase":
            su.phase_steps(cores, torch, steps, dt)
        else:
            su.whole_steps(cores, torch, steps, dt)
        su.assert_equal(su.gather(cores), want, (case, mode))


# ---------------------------------------------------------------- 4. the mass budget, through the monitor
def test_mass_budget_of_a_uniform_source(g):
    """a source S alone adds dt S to every cell, so the monitor's mass grows by dt S air.  Bound: the stats test's
    summation bound (N + 2) 2^-53 sum |c p dsig| for each of the two masses compared, plus two product roundings and
    the one rounding of the forced value per cell: 3 (N + 2) 2^-53 sum |c p dsig| over the N cells"""
    H, W, L, dt, S = 24, 36, 9, 120.0, 0.37
    geom, st, trs, _ = _setup(H, W, L)
    a = su.single(g, geom, st, trs, scheme="van_leer")
    b = su.single(g, geom, st, trs, recs={i: dict(source=S) for i in range(NTR)}, scheme="van_leer")
    a.step(1, dt)
    b.step(1, dt)
    sa, sb = a.tracer_stats(), b.tracer_stats()
    p, c = b.get_state()[0], b.get_tracers()
    w = p[None, :, :] * np.asarray(geom.dsig, dtype=np.float64).reshape(L, 1, 1)
    N = L * H * W
    assert np.array_equal(sa.air, sb.air)
    for i in range(NTR):
        bound = 3 * (N + 2) * 2.0 ** -53 * np.sum(np.abs(c[i] * w))
        diff = abs(sb.mass[i] - (sa.mass[i] + dt * S * sa.air[i]))
        print("tracer %d: |mass_B - (mass_A + dt S air)| = %.6e, bound %.6e, mass %.6e" % (i, diff, bound, sb.mass[i]))
        assert diff <= bound
        assert abs(sb.mass[i] - sa.mass[i]) > 100 * bound         # (the source is far above the bound)
    a.close()
    b.close()


# ---------------------------------------------------------------- 5. life cycle and refusals
def test_life_cycle_and_refusals(g):
    import ctypes as C
    from gcmiipy_amd import _lib
    lib = _lib.lib
    H, W, L, dt = 12, 20, 5, 120.0
    geom, st, trs, recs = _setup(H, W, L)
    c = su.single(g, geom, st, trs, recs={1: recs[1]}, scheme="van_leer")
    rec = lambda **kw: C.byref(_lib.TracerForcing(kw.get("source", 0.0), kw.get("decay", 0.0), kw.get("pin_value", 0.0), None, None))
    assert [lib.gcm_tracer_forced(c._h, i) for i in range(NTR)] == [0, 1, 0, 0]
    for i in (-1, NTR, 99):
        assert lib.gcm_tracer_forced(c._h, i) == _lib.ERR_ARG
    # every refusal, and that it changed nothing
    for i in (-1, NTR, 99):
        assert lib.gcm_set_tracer_forcing(c._h, i, rec(source=1.0)) == _lib.ERR_ARG
    for i in (-2, NTR):
        assert lib.gcm_set_tracer_forcing(c._h, i, None) == _lib.ERR_ARG
    for bad in (dict(source=np.nan), dict(source=np.inf), dict(decay=np.nan), dict(decay=np.inf), dict(decay=-1e-9),
                dict(pin_value=np.nan), dict(pin_value=-np.inf)):
        assert lib.gcm_set_tracer_forcing(c._h, 1, rec(**bad)) == _lib.ERR_ARG, bad
        assert lib.gcm_set_tracer_forcing(c._h, 2, rec(**bad)) == _lib.ERR_ARG, bad
        with pytest.raises(ValueError):
            c.set_tracer_forcing(1, **bad)
    assert [lib.gcm_tracer_forced(c._h, i) for i in range(NTR)] == [0, 1, 0, 0]
    assert c.tracer_forcing(1)["source"] == recs[1]["source"] and c.tracer_forcing(2) is None
    ref = su.single(g, geom, st, trs, recs={1: recs[1]}, scheme="van_leer")
    ref.step(1, dt)
    c.step(1, dt)
    assert np.array_equal(c.get_tracers(), ref.get_tracers())     # tracer 1 is forced as registered, nothing else is
    # it survives set_tracers with the same count, a change of scheme and set_state
    c.set_tracers(trs)
    c.set_tracer_scheme("upwind")
    c.set_tracer_scheme("van_leer")
    c.set_state(*st)
    assert [lib.gcm_tracer_forced(c._h, i) for i in range(NTR)] == [0, 1, 0, 0]
    c.step(1, dt)
    assert np.array_equal(c.get_tracers(), ref.get_tracers())
    # clearing one, then all
    c.set_tracer_forcing(3, **recs[3])
    c.clear_tracer_forcing(1)
    assert [lib.gcm_tracer_forced(c._h, i) for i in range(NTR)] == [0, 0, 0, 1] and c.tracer_forcing(1) is None
    c.set_tracer_forcing(2, **recs[2])
    c.clear_tracer_forcing()
    assert [lib.gcm_tracer_forced(c._h, i) for i in range(NTR)] == [0] * NTR and c.tracer_forcings() == {}
    plain = su.single(g, geom, st, trs, scheme="van_leer")
    plain.step(1, dt)
    c.set_tracers(trs)
    c.set_state(*st)
    c.step(1, dt)
    assert np.array_equal(c.get_tracers(), plain.get_tracers())   # cleared: the unforced step
    # another count drops it
    c.set_tracer_forcing(0, source=1.0)
    c.set_tracers(trs[:3])
    assert [lib.gcm_tracer_forced(c._h, i) for i in range(3)] == [0, 0, 0] and c.tracer_forcing(0) is None
    c.set_tracer_forcing(0, source=1.0)
    c.set_tracers(None)
    assert lib.gcm_tracer_forced(c._h, 0) == _lib.ERR_ARG and c.tracer_count == 0
    assert lib.gcm_set_tracer_forcing(c._h, 0, rec(source=1.0)) == _lib.ERR_ARG      # no tracers: no index is valid
    assert lib.gcm_set_tracer_forcing(c._h, -1, None) == _lib.OK
    for x in (c, ref, plain):
        x.close()
    # a band's reallocation drops it; the same depth again allocates nothing and keeps it
    band = g.Core(_lib.PE25D, W, 6, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0, band_tracers=2)
    band.set_tracer_forcing(1, source=1.0, pin_mask=np.ones((L, 6, W), dtype=bool))
    assert lib.gcm_tracer_forced(band._h, 1) == 1
    assert lib.gcm_set_band_tracer_rows(band._h, 1) == _lib.OK and lib.gcm_tracer_forced(band._h, 1) == 1
    assert lib.gcm_set_band_tracer_rows(band._h, 2) == _lib.OK
    assert band.tracer_count == 2 and lib.gcm_tracer_forced(band._h, 1) == 0 and band.tracer_forcing(1) is None
    band.set_tracer_forcing(1, source=1.0)
    assert lib.gcm_set_band_tracers(band._h, 2) == _lib.OK
    assert lib.gcm_tracer_forced(band._h, 1) == 0
    with pytest.raises(ValueError, match="emission"):
        band.set_tracer_forcing(1, emission=np.zeros((L, H, W)))  # a band's fields hold its own rows
    band.close()
    # other models
    sw = g.Core(_lib.SW2D, 130, 8, dx=300e3)
    assert lib.gcm_set_tracer_forcing(sw._h, 0, rec(source=1.0)) == _lib.ERR_UNSUPPORTED
    assert lib.gcm_set_tracer_forcing(sw._h, -1, None) == _lib.ERR_UNSUPPORTED
    assert lib.gcm_tracer_forced(sw._h, 0) == _lib.ERR_UNSUPPORTED
    sw.close()


# ---------------------------------------------------------------- 6. checkpoints
def test_checkpoint_single_domain(g, tmp_path):
    """saved after 2 of 4 steps and restored from the file alone: the uninterrupted run bit for bit; a file saved
    without forcing restores with none, and so does a file from before the keys existed"""
    from gcmiipy_amd import checkpoint
    H, W, L, dt = 16, 20, 5, 120.0
    geom, st, trs, recs = _setup(H, W, L)
    want = _forced_single(g, geom, st, trs, recs, 4, dt, runs=[2, 2])
    c = su.single(g, geom, st, trs, recs=recs, scheme="van_leer")
    c.step(2, dt)
    path = str(tmp_path / "forced.npz")
    checkpoint.save(path, c, step=2, geom=geom)
    c.close()
    c, ck = checkpoint.restore(path)
    assert sorted(ck["tracer_forcing"]) == [1, 2, 3]
    for i, rec in recs.items():
        got = c.tracer_forcing(i)
        assert got["source"] == rec.get("source", 0.0) and got["decay"] == rec.get("decay", 0.0)
        for k in ("emission", "pin_mask"):
            assert (got[k] is None) == (rec.get(k) is None) and (got[k] is None or np.array_equal(got[k], rec[k]))
    assert c.tracer_forcing(0) is None
    c.step(2, dt)
    su.assert_equal((c.get_state(), c.get_tracers()), want)
    c.close()
    plain = su.single(g, geom, st, trs, scheme="van_leer")
    path = str(tmp_path / "plain.npz")
    checkpoint.save(path, plain, geom=geom)
    plain.close()
    assert not [k for k in np.load(path).files if k.startswith("forcing_")]
    c, ck = checkpoint.restore(path)
    assert ck["tracer_forcing"] == {} and c.tracer_count == NTR and c.tracer_forcings() == {}
    c.close()


def test_checkpoint_bands(g, tmp_path):
    """both bands of a forced 2-band run saved after 2 steps, restored and continued for 2: the single domain"""
    import torch
    from gcmiipy_amd import checkpoint
    H, W, L, dt = 16, 20, 5, 120.0
    geom, st, trs, recs = _setup(H, W, L)
    want = _forced_single(g, geom, st, trs, recs, 4, dt)
    cores = su.bands(g, geom, 2, st, trs, recs=recs, scheme="van_leer", rows=2)
    su.whole_steps(cores, torch, 2, dt)
    for r, c in enumerate(cores):
        checkpoint.save(str(tmp_path / ("b%d.npz" % r)), c, step=2, geom=geom)
        c.close()
    cores = [checkpoint.restore(str(tmp_path / ("b%d.npz" % r)))[0] for r in range(2)]
    for c in cores:
        assert sorted(c.tracer_forcings()) == [1, 2, 3] and c.tracer_forcing(2)["emission"].shape == (L, c.H, W)
    su.whole_steps(cores, torch, 2, dt)
    su.assert_equal(su.gather(cores), want)


# ---------------------------------------------------------------- 7. the drop-ins
def test_drop_ins_equal_the_core_path(g):
    from gcmiipy_amd import dynamics
    H, W, L, dt = 12, 20, 5, 120.0
    geom, st, trs, recs = _setup(H, W, L)
    want = _forced_single(g, geom, st, trs, recs, 3, dt, runs=[3])
    got = dynamics.run(*st, dt, geom, 3, tracers=trs, tracer_scheme="van_leer", tracer_forcing=recs)
    su.assert_equal((got[:5], got[5]), want, "run")
    one = su.single(g, geom, st, trs, recs=recs, scheme="centred")
    one.step(1, dt)
    got = dynamics.matsuno_timestep(*st, dt, geom, tracers=trs, tracer_forcing=recs)
    su.assert_equal((got[:5], got[5]), (one.get_state(), one.get_tracers()), "matsuno_timestep")
    one.close()
    # the cached handle of matsuno_timestep carries no forcing over to the next call
    plain = dynamics.matsuno_timestep(*st, dt, geom, tracers=trs)
    again = su.single(g, geom, st, trs, scheme="centred")
    again.step(1, dt)
    assert np.array_equal(plain[5], again.get_tracers())
    again.close()
    with pytest.raises(ValueError, match="tracers"):
        dynamics.run(*st, dt, geom, 1, tracer_forcing=recs)
    # no_limits_2_5d.run_model builds its own state: the same set-up through Core
    g.clear_cache()
    from gcmiipy_amd import geometry, no_limits_2_5d as nl
    H = W = 12                                                    # (run_model's statistics need a square grid)
    _, _, trs, recs = _setup(H, W, L)
    out = nl.run_model(H, W, L, dt, 3, None, tracers=trs, tracer_scheme="upwind", tracer_forcing=recs)
    geom2 = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    p, u, v, t, q, _ = nl.gen_initial_conditions(geom2)
    v[0, 0, 0] = 0.1
    u *= 0
    one = su.single(g, geom2, (p, u, v, t, q), trs, recs=recs, scheme="upwind")
    for _ in range(3):
        one.step(1, dt)
    su.assert_equal((out[:5], out[7]), (one.get_state(), one.get_tracers()), "run_model")
    one.close()
    g.clear_cache()
