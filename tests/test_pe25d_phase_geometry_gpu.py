"""The launch geometries the product grid takes in the GCM_PE25D phases whose grid depends on the rows, the row length
and the chip's compute units -- the Held-Suarez forcing, the climatology's sample, the moist physics, the tracers'
forcing -- at the smallest shapes that reach them (tests/pe25d_phase_geometry_cases.py): whole columns and level
segments marched in batches of four, a second column block, several levels per workgroup of the sample and a second
iteration of its chunk loop, a second pass of the forcing's capped grid, the level split of a launch that accumulates
nothing.  Every test first asserts its geometry through Core.phase_plan on the handle it is about to use, then calls
the phase explicitly (no dynamics step but the one the tracers' forcing rides on) and holds the result to the phase's
NumPy restatement by the criteria of the phase's own test module, and to another launch geometry of the same rows bit
for bit where the kernel promises that."""
import numpy as np
import pytest

import gpu_setups as su
import pe25d_climate_ref as cl_ref
import pe25d_held_suarez_ref as hs_ref
import pe25d_inputs as inp
import pe25d_moist_ref as mo_ref
import pe25d_phase_geometry_cases as pc
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)
from pe25d_tracer_forcing_ref import force

pytestmark = pytest.mark.gpu

DT = 120.0
HS_OVER = ({}, dict(sigma_b=0.45, k_f=4e-5, T_min=240.0))


def _id(case):
    return "%dx%dx%d" % case.shape


def _sig(geom):
    return np.asarray(geom.sig, dtype=np.float64).reshape(-1)


def _lat(geom):
    return np.asarray(geom.lat, dtype=np.float64).reshape(-1)


def _assert_same(got, want, what=""):
    for k, a, b in zip("puvtq", got, want):
        assert np.array_equal(a, b), (what, k, float(np.max(np.abs(a - b))))


# ---------------------------------------------------------------- Held-Suarez
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ptop", pc.PTOPS)
@pytest.mark.parametrize("case", pc.HELD_SUAREZ, ids=_id)
def test_held_suarez_equals_the_restatement(g, case, ptop, dtype):
    """the criteria of test_pe25d_held_suarez_gpu.test_step_equals_the_restatement: u and v bit for bit, theta within
    1e-10 relative (fp64) or one rounding of float32, untouched fields and free levels bit for bit"""
    H, W, L = case.shape
    geom = su.geom_of(H, W, L, ptop)
    sig, lat = _sig(geom), _lat(geom)
    st = pc.state(geom, dtype)
    for over in HS_OVER:
        c = su.single(g, geom, st, dtype=dtype, filter=False)
        assert c.phase_plan("held_suarez") == case.plan, case.what
        c.held_suarez_step(geom, DT, **over)
        p, u, v, t, q = c.get_state()
        c.close()
        un, vn, tn = hs_ref.step(st[0], st[1], st[2], st[3], sig, ptop, lat, DT, dtype=dtype, **over)
        assert np.array_equal(u, un) and np.array_equal(v, vn)
        err = np.max(np.abs(t - tn) / np.abs(tn))
        print("theta rel err", case.shape, ptop, dtype, err)
        assert err <= (1e-10 if dtype == "f64" else 2.0 ** -23), err
        free = hs_ref.r_of(sig, hs_ref.params(**over)["sigma_b"]) == 0
        assert free.any() and not free.all()
        assert np.array_equal(u[free], st[1][free]) and np.array_equal(v[free], st[2][free])
        assert not np.array_equal(u[~free], st[1][~free]) and not np.array_equal(t, st[3])
        assert np.array_equal(p, st[0]) and np.array_equal(q, st[4])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ptop", pc.PTOPS)
def test_held_suarez_bands_equal_single_domain(g, ptop, dtype):
    """(200, 36, 25) in three level segments of 8, 8, 9 against eight bands of 25 rows, whose launches over own rows and
    current ghost rows split the levels into 18 segments of 1 or 2: the same bits whichever launch"""
    import torch
    case = pc.HELD_SUAREZ[2]
    H, W, L = case.shape
    geom = su.geom_of(H, W, L, ptop)
    st = pc.state(geom, dtype)
    one = su.single(g, geom, st, dtype=dtype)
    assert one.phase_plan("held_suarez") == case.plan
    one.held_suarez_step(geom, DT)
    want = one.get_state()
    one.close()
    cores = su.bands(g, geom, pc.HS_BANDS, st, dtype=dtype)
    su.exchange(cores, torch)
    for c in cores:
        assert c.phase_plan("held_suarez", rows=c.H + 2 * pc.GHOST) == pc.HS_BAND_PLAN
        c.held_suarez_step(geom, DT)
    parts = [c.get_state() for c in cores]
    for c in cores:
        c.close()
    got = [np.concatenate([x[f] for x in parts], axis=0 if f == 0 else 1) for f in range(5)]
    _assert_same(got, want, "eight bands")
    assert not np.array_equal(want[3], st[3]) and not np.array_equal(want[1], st[1])


# ---------------------------------------------------------------- climatology
def _match_restatement(got, want, bnd, what):
    """test_pe25d_climate_gpu.assert_sums_match_restatement: the words without the Exner routine and p, p p bit for bit,
    words 3, 6 and 8 within 1e-10 sum |term|"""
    assert got[0] == want[0], (what, got[0], want[0])
    for w in range(10):
        if w in cl_ref.EXNER_WORDS:
            ratio = float(np.max(np.abs(got[1][w] - want[1][w]) / bnd[w]))
            assert ratio <= 1e-10, (what, "m3 word", w, ratio)
        else:
            assert np.array_equal(got[1][w], want[1][w]), (what, "m3 word", w, float(np.max(np.abs(got[1][w] - want[1][w]))))
    for w in range(2):
        assert np.array_equal(got[2][w], want[2][w]), (what, "m2 word", w)


def _two_samples(c, states):
    for st in states:
        c.set_state(*st)
        c.climate_sample()
    return c.climate_sums()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ptop", pc.PTOPS)
@pytest.mark.parametrize("case", pc.CLIMATE, ids=_id)
def test_climate_two_samples_equal_the_restatement(g, case, ptop, dtype):
    H, W, L = case.shape
    geom = su.geom_of(H, W, L, ptop)
    first = pc.state(geom, dtype)
    states = [first, pc.second_state(first)]
    c = su.single(g, geom, dtype=dtype, filter=False, every=10 ** 6)
    assert c.phase_plan("climate") == case.plan, case.what
    got = _two_samples(c, states)
    sig = _sig(geom)
    want = cl_ref.accumulate(states, sig, ptop)
    bnd = sum(cl_ref.bound(s[0], s[1], s[2], s[3], sig, ptop) for s in states)
    _match_restatement(got, want, bnd, (case.shape, ptop, dtype))
    one = cl_ref.sample(first[0], first[1], first[2], first[3], sig, ptop)
    assert not np.array_equal(one[0][2], want[1][2]) and not np.array_equal(one[1][0], want[2][0])   # (two samples are in)
    if case.shape[0] == 512:
        # rows 0 .. 23 once more on a band handle, one level per workgroup; its row -1 of v is the south edge of the band
        # that holds the last rows of the grid (the single domain's pole-to-pole roll)
        import torch
        n = pc.CL_BAND_ROWS
        kw = dict(geom=geom, nranks=2, global_height=H, dtype=dtype, filter=False)
        a = g.Core(g._lib.PE25D, W, n, L, rank=0, row0=0, **kw)
        b = g.Core(g._lib.PE25D, W, n, L, rank=1, row0=H - n, **kw)
        a.set_climate(10 ** 6)
        assert a.phase_plan("climate") == pc.CL_BAND_PLAN
        buf = torch.empty(b.halo_bytes(), dtype=torch.uint8, device="cuda")
        for st in states:
            a.set_state(*[inp.rows(x, slice(0, n)) for x in st])
            b.set_state(*[inp.rows(x, slice(H - n, H)) for x in st])
            b.halo_pack(1, buf.data_ptr())
            torch.cuda.synchronize()
            a.halo_unpack(0, buf.data_ptr())
            torch.cuda.synchronize()
            a.climate_sample()
        band = a.climate_sums()
        a.close()
        b.close()
        assert band[0] == got[0] == 2
        for w in range(10):
            assert np.array_equal(band[1][w], got[1][w][:, :n]), ("band, m3 word", w)
        for w in range(2):
            assert np.array_equal(band[2][w], got[2][w][:n]), ("band, m2 word", w)
    c.close()


# ---------------------------------------------------------------- tracer forcing
@pytest.mark.parametrize("case", pc.TRACER_FORCING, ids=lambda c: c.dtype)
def test_tracer_forcing_second_pass(g, case):
    """the A / B construction of test_pe25d_tracer_forcing_gpu.test_one_step_bit_for_bit: handle A steps unforced and the
    restatement is applied to what it returns, handle B steps forced: equal bits"""
    H, W, L = case.shape
    dtype = case.dtype
    geom = su.geom_of(H, W, L)
    st, trs = su.initial(geom, pc.TF_NTR)
    recs = pc.tf_records(case.shape)
    a = su.single(g, geom, st, trs, dtype=dtype, scheme="van_leer")
    b = su.single(g, geom, st, trs, recs=recs, dtype=dtype, scheme="van_leer")
    assert b.phase_plan("tracer_forcing") == case.plan, case.what
    assert [b.tracer_forcing(i) is not None for i in range(pc.TF_NTR)] == [False, True, True, True]
    a.step(1, DT)
    b.step(1, DT)
    ta, tb = a.get_tracers(), b.get_tracers()
    sa, sb = a.get_state(), b.get_state()
    a.close()
    b.close()
    first = pc.TF_PASS_VECTORS * (2 if dtype == "f64" else 4)
    for i in range(pc.TF_NTR):
        want = force(ta[i], DT, recs[i], dtype).astype(np.float64) if i in recs else ta[i]
        bad = pc.device_order(tb[i] != want)
        assert not bad.any(), (dtype, "tracer", i, "first pass", int(bad[:first].sum()), "second pass", int(bad[first:].sum()))
        if i in recs:
            moved = pc.device_order(tb[i] != ta[i])
            assert moved[:first].any() and moved[first:].any(), i
    _assert_same(sb, sa, "state")


# ---------------------------------------------------------------- moist physics
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ptop", pc.PTOPS)
def test_moist_level_split_equals_whole_columns(g, ptop, dtype):
    """bands of 4 rows without a registration: the explicit call launches own rows and ghost rows and accumulates
    nothing, so it splits the 42 levels into 8 segments; the single domain given the same columns splits them into 6
    without a registration and marches whole columns with one.  The criterion of
    test_pe25d_column_phases_gpu.test_in_process_bands_equal_single_domain: the same bits; and theta and q against the
    restatement as in test_step_equals_the_restatement"""
    import torch
    H, W, L = pc.MOIST_SHAPE
    geom = pc.moist_geom(ptop)
    st = pc.moist_state(geom, dtype)
    whole = su.single(g, geom, st, dtype=dtype, filter=False)
    whole.set_moist(**pc.MOIST_PAR)
    assert whole.phase_plan("moist", accumulate=True)["grid_z"] == 1
    whole.moist_step(pc.MOIST_DT, **pc.MOIST_PAR)
    want = whole.get_state()
    sums = whole.moist_sums()
    whole.close()
    tn, qn, P, E = mo_ref.moist_step(st[0], st[3], st[4], geom.sig, geom.dsig, ptop, pc.MOIST_DT,
                                     mo_ref.params(**pc.MOIST_PAR), dtype)
    tol = 1e-10 if dtype == "f64" else 2.0 ** -23
    errs = dict(t=float(np.max(np.abs(want[3] - tn)) / np.max(np.abs(tn))), q=float(np.max(np.abs(want[4] - qn)) / np.max(np.abs(qn))),
                precip=float(np.max(np.abs(sums.precip - P)) / np.max(np.abs(P))), evap=float(np.max(np.abs(sums.evap - E)) / np.max(np.abs(E))))
    print("moist step", ptop, dtype, errs)
    assert errs["t"] <= tol and errs["q"] <= tol and errs["precip"] <= 1e-10 and errs["evap"] <= 1e-10, errs
    assert np.array_equal(want[4] != st[4], qn != st[4]) and (want[4] != st[4]).any()

    split = su.single(g, geom, st, dtype=dtype, filter=False)
    assert split.moist is None and split.phase_plan("moist", accumulate=False) == pc.MOIST_SINGLE_PLAN
    split.moist_step(pc.MOIST_DT, **pc.MOIST_PAR)
    _assert_same(split.get_state(), want, "single domain, six level segments")
    split.close()

    cores = su.bands(g, geom, pc.MOIST_BANDS, st, dtype=dtype, filter=False)
    su.exchange(cores, torch)
    for c in cores:
        assert c.moist is None
        plan = c.phase_plan("moist", rows=c.H + 2 * pc.GHOST, accumulate=False)
        assert plan == pc.MOIST_BAND_PLAN and 1 < plan["grid_z"] < L
        assert c.phase_plan("moist", rows=2 * pc.GHOST, accumulate=False) == pc.MOIST_GHOST_PLAN
        c.moist_step(pc.MOIST_DT, **pc.MOIST_PAR)
    parts = [c.get_state() for c in cores]
    for c in cores:
        c.close()
    got = [np.concatenate([x[f] for x in parts], axis=0 if f == 0 else 1) for f in range(5)]
    _assert_same(got, want, "three bands, eight level segments")


# ---------------------------------------------------------------- the product grid
def test_product_grid_plan(g):
    """no launch changed its grid: the handle of the product shape reports what the launchers take there"""
    H, W, L = pc.PRODUCT
    for dtype, passes in (("f64", 24), ("f32", 12)):
        c = g.Core(g._lib.PE25D, W, H, L, geom=su.geom_of(H, W, L), dtype=dtype)
        hs, mo, cl, tf = (c.phase_plan(p) for p in ("held_suarez", "moist", "climate", "tracer_forcing"))
        with pytest.raises(ValueError):
            c.phase_plan("convect")
        with pytest.raises(ValueError):
            c.phase_plan("climate", rows=0)
        c.close()
        assert hs == mo == dict(grid_x=6, grid_y=720, grid_z=1, levels_min=24, levels_max=24)
        assert cl == dict(grid_x=720, nseg=3, levels_min=8, levels_max=8, chunks=2)
        assert tf == dict(groups=2048, passes=passes)
    s = g.Core(g._lib.SW2D, 32, 16, dx=1e5)
    with pytest.raises(g.GcmError):
        s.phase_plan("climate")
    s.close()
