"""The horizontal diffusion of GCM_PE25D on the device (gcm_set_hdiff, gcm_hdiff_step) against the NumPy restatement
tests/pe25d_hdiff_ref.py, bit for bit in both storage types: every operation of the update is an IEEE add, subtract or
multiply with host-built coefficients.  The kernel on the tracer tests' shapes and across the seams of its tiles, the
registered phase against the explicit call, the stream order at a size where the streams overlap, half steps, a change
of dt, the refused calls, the checkpoint, and a run with the whole physics suite registered beside it."""
import numpy as np
import pytest

import gpu_setups as su
import pe25d_hdiff_ref as ref
import pe25d_inputs as inp
from column_phase_cases import assert_same, final

pytestmark = pytest.mark.gpu

SHAPES = ((24, 36, 9), (6, 10, 3))                       # (H, W, L) of the tracer tests
PTOP = 1000.0
UTC0 = inp.UTC0
DT = ref.DT


def diffused(st, geom, dt, dtype="f64", **par):
    """the restatement's [p, u, v, t, q] behind one application with the parameters par"""
    par = ref.params(**par)
    return ref.apply(st, ref.tables_of(geom, dt, **par), dtype=dtype, **par)


# ---------------------------------------------------------------- 1: the kernel against the restatement
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ptop", [0.0, PTOP])
@pytest.mark.parametrize("shape", SHAPES)
def test_step_equals_the_restatement(shape, ptop, dtype):
    import gcmiipy_amd as g
    H, W, L = shape
    geom = su.geom_of(H, W, L, ptop)
    st = inp.state_of(geom, dtype)
    trs = inp.tracers(H, W, L, 2)
    gt = inp.ground(H, W)
    c = su.single(g, geom, st, trs, dtype=dtype, gt=gt)
    trs0 = c.get_tracers()
    for order, nu in ref.CASES:
        for fields in ("uvt", "t", "uvtq"):
            c.set_state(*st)
            c.horizontal_diffusion_step(DT, order=order, nu=nu, fields=fields)
            got = c.get_state()
            want = diffused(st, geom, DT, dtype, order=order, nu=nu, fields=fields)
            for n, f in enumerate("puvtq"):
                assert np.array_equal(got[n], want[n]), (order, nu, fields, f, float(np.max(np.abs(got[n] - want[n]))))
                if f in fields:
                    # the selected fields really changed.  (The small nu of either order on the 6 x 10 grid moves theta
                    # by 2e-6 K, less than half an ulp of float32 at 300 K: there the restatement itself keeps theta's
                    # bits, and the large nu is the case that shows the change)
                    if nu in (1.0e9, 1.0e22) or not np.array_equal(want[n], st[n]):
                        assert not np.array_equal(got[n], st[n]), (order, nu, fields, f)
                else:
                    assert np.array_equal(got[n], st[n]), (order, nu, fields, f)
            assert np.array_equal(c.get_tracers(), trs0) and np.array_equal(c.get_ground(), gt)
            assert c.horizontal_diffusion is None            # (an explicit step registers nothing)
    c.close()


# ---------------------------------------------------------------- 2: the seams of the tiles
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_seams_of_the_tiles(dtype):
    """a grid of more than one tile each way with a partial last tile in i and in j, sized from the plan, and a grid
    smaller than one tile: both orders equal the restatement whichever tile computes a cell"""
    import gcmiipy_amd as g
    probe = su.single(g, su.geom_of(*SHAPES[1]), filter=False)
    plan = probe.horizontal_diffusion_plan()
    probe.close()
    tr, tc = plan["tile_rows"], plan["tile_cols"]
    assert plan["launches"] == 1 and 2 * plan["lds_bytes"] <= 160 * 1024
    big = (max(2 * tr + 1, 4), max(2 * tc + 3, 4), 2)
    small = (max(min(tr - 1, 7), 4), max(min(tc - 1, 10), 4), 2)
    for (H, W, L), whole in ((big, False), (small, True)):
        geom = su.geom_of(H, W, L)
        st = inp.state_of(geom, dtype)
        c = su.single(g, geom, st, dtype=dtype, filter=False)
        plan = c.horizontal_diffusion_plan()
        if whole:
            assert plan["tiles_i"] == 1 and plan["tiles_j"] == 1 and (W < tc or tc <= 4) and (H < tr or tr <= 4)
        else:
            assert plan["tiles_i"] > 1 and plan["tiles_j"] > 1 and W % tc != 0 and H % tr != 0
        assert plan["grid_z"] == 3 * L
        for order, nu in ((1, 1.0e9), (2, 1.0e22), (2, 1.0e15)):
            c.set_state(*st)
            c.horizontal_diffusion_step(DT, order=order, nu=nu, fields="uvtq")
            got = c.get_state()
            want = diffused(st, geom, DT, dtype, order=order, nu=nu, fields="uvtq")
            for n, f in enumerate("puvtq"):
                bad = np.argwhere(got[n] != want[n])
                assert bad.size == 0, (H, W, order, nu, f, bad[:4].tolist())
        c.close()


# ---------------------------------------------------------------- 3: registered against explicit
@pytest.mark.parametrize("phys", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_registered_equals_explicit(dtype, phys):
    """step(1) + horizontal_diffusion_step + [solar_step + held_suarez_step], five times, against the registrations +
    step(5): the order of the phases is Matsuno step, diffusion, solar step, Held-Suarez"""
    import gcmiipy_amd as g
    H, W, L = SHAPES[0]
    geom = su.geom_of(H, W, L)
    st, gt = inp.state_of(geom, dtype), inp.ground(H, W)
    par = dict(order=2, nu=1.0e15)
    hs = {} if phys else None

    def explicit(diffusion_last):
        a = su.single(g, geom, st, dtype=dtype, gt=gt)
        for n in range(5):
            a.step(1, DT)
            if not diffusion_last:
                a.horizontal_diffusion_step(DT, **par)
            if phys:
                a.solar_step(geom, DT, UTC0 + n * DT)
                a.held_suarez_step(geom, DT)
            if diffusion_last:
                a.horizontal_diffusion_step(DT, **par)
        return final(a)
    want = explicit(False)
    b = su.single(g, geom, st, dtype=dtype, gt=gt, phys=phys, hs=hs)
    b.set_horizontal_diffusion(**par)
    assert b.horizontal_diffusion == ref.params(**par)
    b.step(5, DT)
    assert_same(final(b, close=False), want, "registered")
    # the diffusion is not the identity, and the other order of the phases gives other bits
    plain = su.single(g, geom, st, dtype=dtype, gt=gt, phys=phys, hs=hs)
    plain.step(5, DT)
    assert not np.array_equal(final(plain)[1], want[1])
    if phys:
        assert not np.array_equal(explicit(True)[3], want[3])
    # switched off: the next steps are an unregistered handle's
    b.set_horizontal_diffusion(None)
    assert b.horizontal_diffusion is None
    b.step(2, DT)
    u = su.single(g, geom, want[:5], dtype=dtype, gt=want[5], hs=hs)
    if phys:
        u.set_physics(geom, UTC0 + 5 * DT)
    u.step(2, DT)
    assert_same(final(b), final(u), "switched off")


# ---------------------------------------------------------------- 4: the stream order
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_stream_order_at_overlapping_size(dtype):
    """the grid of test_band_run_chains_at_overlapping_size (48 x 1440 x 24: kernels of tens of microseconds on either
    stream).  The phase writes u and v, which the next stage's second-stream launches read: step(4) equals four rounds
    of step(1) + sync(), and both equal four rounds of an unregistered step(1) + the explicit call"""
    import gcmiipy_amd as g
    H, W, L, dt, steps = 48, 1440, 24, 1.0, 4
    par = dict(order=2, nu=1.0e22)
    geom = su.geom_of(H, W, L)
    tab = ref.tables_of(geom, dt, **par)
    assert (tab["ax"] == 0.125).all() and (tab["axv"] == 0.125).all()      # (a nu that caps every row)
    st = inp.state_of(geom, dtype)
    ref_c = su.single(g, geom, st, dtype=dtype)
    ref_c.set_horizontal_diffusion(**par)
    ref_c.step(steps, dt)
    want = final(ref_c)
    one = su.single(g, geom, st, dtype=dtype)
    one.set_horizontal_diffusion(**par)
    for _ in range(steps):
        one.step(1, dt)
        one.sync()
    assert_same(final(one), want, "step(1) + sync")
    ex = su.single(g, geom, st, dtype=dtype)
    for _ in range(steps):
        ex.step(1, dt)
        ex.horizontal_diffusion_step(dt, **par)
    assert_same(final(ex), want, "step(1) + explicit")
    plain = su.single(g, geom, st, dtype=dtype)
    plain.step(steps, dt)
    assert not np.array_equal(final(plain)[1], want[1])


# ---------------------------------------------------------------- 5: half steps
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_half_step_is_never_diffused(dtype):
    """gcm_half_step never applies the phase; gcm_step_phase serves latitude bands only, which cannot register it"""
    import gcmiipy_amd as g
    H, W, L = SHAPES[0]
    geom = su.geom_of(H, W, L)
    st = inp.state_of(geom, dtype)
    r, u = su.single(g, geom, st, dtype=dtype), su.single(g, geom, st, dtype=dtype)
    r.set_horizontal_diffusion(order=1, nu=1.0e9)
    for c in (r, u):
        c.half_step(0, DT)
    star_r, star_u = r.get_star(), u.get_star()
    for k in range(4):
        assert np.array_equal(star_r[k], star_u[k]), k
    for c in (r, u):
        c.half_step(1, DT)
    assert g._lib.lib.gcm_step_phase(r._h, 0, DT, None) == g._lib.ERR_STATE     # (not a latitude band)
    assert_same(final(r), final(u), "half steps")


# ---------------------------------------------------------------- 6: a change of dt
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_tables_follow_a_change_of_dt(dtype):
    import gcmiipy_amd as g
    H, W, L = SHAPES[1]
    geom = su.geom_of(H, W, L)
    st = inp.state_of(geom, dtype)
    par = dict(order=1, nu=1.0e9)
    a = su.single(g, geom, st, dtype=dtype)
    for dt in (DT, DT, 45.0, 45.0, DT):
        a.step(1, dt)
        a.horizontal_diffusion_step(dt, **par)
    b = su.single(g, geom, st, dtype=dtype)
    b.set_horizontal_diffusion(**par)
    b.step(2, DT)
    b.step(2, 45.0)
    b.step(1, DT)
    assert_same(final(b), final(a), "dt")


# ---------------------------------------------------------------- 7: refused calls
def test_refused_calls_change_nothing():
    import gcmiipy_amd as g
    lib, L_ = g._lib.lib, g._lib
    H, W, L = SHAPES[1]
    geom = su.geom_of(H, W, L)
    st = inp.state_of(geom)
    par = dict(order=1, nu=1.0e9, fields="ut")
    c = su.single(g, geom, st)
    c.set_horizontal_diffusion(**par)
    was = c.horizontal_diffusion
    assert was == ref.params(**par)
    nan, inf = float("nan"), float("inf")
    for over in (dict(order=0), dict(order=3), dict(fields=0), dict(fields=16), dict(nu=0.0), dict(nu=-1.0), dict(nu=nan),
                 dict(nu=inf), dict(cmax=0.0), dict(cmax=0.2), dict(cmax=nan)):
        with pytest.raises(ValueError):
            c.set_horizontal_diffusion(**over)
        with pytest.raises(ValueError):
            c.horizontal_diffusion_step(DT, **over)
    for dt in (nan, inf):
        with pytest.raises(ValueError):
            c.horizontal_diffusion_step(dt, **par)
    with pytest.raises(ValueError):
        c.set_horizontal_diffusion(nux=1.0)
    with pytest.raises(ValueError):
        c.set_horizontal_diffusion(None, order=1)
    with pytest.raises(ValueError):
        c.set_horizontal_diffusion(fields="xyz")
    assert lib.gcm_hdiff_step(c._h, DT, None) == L_.ERR_ARG
    assert lib.gcm_hdiff_plan(c._h, None, L_.HDIFF_PLAN_WORDS) == L_.ERR_ARG
    assert c.horizontal_diffusion == was and lib.gcm_hdiff_on(c._h) == 1
    assert_same(c.get_state(), st, "state after refused calls")
    c.step(2, DT)
    w = su.single(g, geom, st)
    w.set_horizontal_diffusion(**par)
    w.step(2, DT)
    assert_same(final(c), final(w), "after refused calls")
    # other models
    rec = L_.Hdiff(*ref.DEFAULTS.values())
    s = g.Core(L_.SW2D, 32, 16, dx=1e5)
    assert lib.gcm_set_hdiff(s._h, rec) == L_.ERR_UNSUPPORTED and lib.gcm_hdiff_step(s._h, 60.0, rec) == L_.ERR_UNSUPPORTED
    assert lib.gcm_hdiff_on(s._h) == 0
    s.close()
    # a latitude band
    b = g.Core(L_.PE25D, W, H, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0)
    b.set_state(*st)
    with pytest.raises(g.GcmError, match="single domains only"):
        b.set_horizontal_diffusion(**par)
    assert lib.gcm_set_hdiff(b._h, rec) == L_.ERR_UNSUPPORTED and lib.gcm_hdiff_step(b._h, DT, rec) == L_.ERR_UNSUPPORTED
    assert lib.gcm_hdiff_on(b._h) == 0 and b.horizontal_diffusion is None
    assert_same(b.get_state(), st, "band after refused calls")
    b.close()
    # W or H of 3
    for h3, w3 in ((3, 10), (6, 3)):
        geom3 = su.geom_of(h3, w3, L)
        st3 = inp.state_of(geom3)
        n = su.single(g, geom3, st3, filter=False)
        assert lib.gcm_set_hdiff(n._h, rec) == L_.ERR_UNSUPPORTED and lib.gcm_hdiff_step(n._h, DT, rec) == L_.ERR_UNSUPPORTED
        assert lib.gcm_hdiff_on(n._h) == 0
        assert_same(n.get_state(), st3, "small grid after refused calls")
        n.close()


# ---------------------------------------------------------------- 8: checkpoint
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_checkpoint_carries_the_registration(dtype, tmp_path):
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    H, W, L = SHAPES[0]
    geom = su.geom_of(H, W, L)
    st = inp.state_of(geom, dtype)
    par = dict(order=2, nu=3.0e15, fields="uvtq", cmax=0.1)

    def registered():
        c = su.single(g, geom, st, dtype=dtype)
        c.set_horizontal_diffusion(**par)
        return c
    whole = registered()
    whole.step(5, DT)
    want = final(whole)
    a = registered()
    a.step(3, DT)
    path = str(tmp_path / "hdiff.npz")
    checkpoint.save(path, a, step=3, geom=geom)
    a.close()
    b, ck = checkpoint.restore(path)
    assert b.horizontal_diffusion == ref.params(**par) and ck["hdiff"] == ref.params(**par)
    b.step(2, DT)
    assert_same(final(b), want, "restored")
    # a file without the key restores with none
    plain = su.single(g, geom, st, dtype=dtype)
    checkpoint.save(path, plain, geom=geom)
    plain.close()
    c, ck = checkpoint.restore(path)
    assert ck["hdiff"] is None and c.horizontal_diffusion is None
    c.close()


# ---------------------------------------------------------------- 9: with the whole suite on
def test_with_the_whole_suite_registered():
    import gcmiipy_amd as g
    import pe25d_boundary_layer_ref as bref
    H, W, L = SHAPES[0]
    geom = su.geom_of(H, W, L)
    st = inp.state_of(geom, wind=1.0)
    c = su.single(g, geom, st, gt=bref.ground(geom, st), phys=True, hs={}, every=4)
    c.set_boundary_layer()
    c.set_convect()
    c.set_moist()
    c.set_spectra(4)
    c.set_horizontal_diffusion(order=2, nu=1.0e15)
    c.step(200, DT)
    s = c.stats(np.ones(1))
    assert s["nans"] == 0, s
    mmax = c.spectra_mmax
    assert mmax >= 2

    def tt():
        """|That|^2 of one sample of the current state, summed over levels and rows, by wavenumber"""
        c.spectra_reset()
        c.spectra_sample()
        n, sums = c.spectra_sums()
        assert n == 1
        return sums[2].sum(axis=(0, 1))
    # one explicit order-2 step damps the highest retained wavenumber by a larger factor than wavenumber 1
    before = tt()
    c.horizontal_diffusion_step(DT, order=2, nu=1.0e22, fields="t")
    after = tt()
    print("TT ratios: m = 1 %.6f, m = %d %.6f" % (after[1] / before[1], mmax, after[mmax] / before[mmax]))
    assert after[mmax] / before[mmax] < after[1] / before[1]
    # one explicit order-1 step lowers the kinetic energy
    ke0 = c.energy(np.ones(1))[0]
    c.horizontal_diffusion_step(DT, order=1, nu=1.0e9, fields="uv")
    ke1 = c.energy(np.ones(1))[0]
    print("kinetic energy %.9e -> %.9e" % (ke0, ke1))
    assert ke1 < ke0, (ke0, ke1)
    c.close()
