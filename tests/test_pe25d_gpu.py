"""GPU parity of the 2.5-D primitive-equation path (GCM_PE25D) against the golden
vectors captured from the reference's dynamics.py and against the oracle.
Tolerance 1e-10 relative (L-inf over max|field|)."""
import numpy as np
import pytest

from conftest import golden, rel_err
import gpu_setups as su
import pe25d_inputs as inp
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu
TOL = 1e-10


def _check(got, want, what, tol=TOL):
    for k, x, y in zip("puvtq", got, want):
        e = rel_err(x, y)
        assert e < tol, (what, k, e)


def test_half_step_stages_vs_golden(g):
    """G7: predictor and corrector outputs on 20x12x5 with a topography bump"""
    from gcmiipy_amd import geometry
    d = golden("g7_half_step")
    L, H, W = d["u0"].shape
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    geom.heightmap[...] = d["heightmap"]
    base = [d[k + "0"] for k in "puvtq"]
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom)
    c.set_state(*base)
    c.half_step(0, float(d["dt"]))
    _check(c.get_star((0, 1, 2, 3, 4)), [d["pred_%s_n" % k] for k in "puvtq"], "predictor")
    c.half_step(1, float(d["dt"]))
    _check(c.get_state(), [d["corr_%s_n" % k] for k in "puvtq"], "corrector")
    _check(c.get_state(), [d["step_" + k] for k in "puvtq"], "step")
    c.close()


def test_dropin_half_and_full_timestep(g):
    from gcmiipy_amd import geometry, dynamics
    d = golden("g7_half_step")
    L, H, W = d["u0"].shape
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    geom.heightmap[...] = d["heightmap"]
    base = [d[k + "0"] for k in "puvtq"]
    dt = float(d["dt"])
    keep = [b.copy() for b in base]
    star = dynamics.half_timestep(*base, *base, dt, geom)
    _check(star, [d["pred_%s_n" % k] for k in "puvtq"], "half_timestep(pred)")
    out = dynamics.half_timestep(*base, *star, dt, geom)
    _check(out, [d["corr_%s_n" % k] for k in "puvtq"], "half_timestep(corr)")
    full = dynamics.matsuno_timestep(*base, dt, geom)
    _check(full, [d["step_" + k] for k in "puvtq"], "matsuno_timestep")
    assert all(np.array_equal(a, b) for a, b in zip(base, keep))       # inputs untouched
    # the boundary_conditions hook (dynamics.py:232-236): identity hook == no hook
    calls = []

    def bc(sp, su, sv, st, sq, dt_, geom_):
        calls.append(1)
        return sp, su, sv, st, sq

    hooked = dynamics.matsuno_timestep(*base, dt, geom, boundary_conditions=bc)
    assert len(calls) == 2
    _check(hooked, full, "hook", tol=1e-15)


def test_multi_step_dense_and_harness(g):
    """G8: 1/3/10 steps at 36x24x9 from a dense random IC and from the reference harness IC"""
    from gcmiipy_amd import geometry
    d = golden("g8_pe25d")
    geom = geometry.gen_geometry(24, 36, 9, sig_func=geometry.manabe_sig)
    for prefix, ic, dt in (("dense", [d["dense_%s0" % k] for k in "puvtq"], float(d["dense_dt"])),
                           ("h36_", None, 900.0)):
        if ic is None:
            ic = [d["ic_24_36_9_" + k].copy() for k in "puvtq"]
            ic[2][0, 0, 0] = 0.1
            ic[1] *= 0
        c = g.Core(g._lib.PE25D, 36, 24, 9, geom=geom)
        c.set_state(*ic)
        done = 0
        for n in (1, 3, 10):
            c.step(n - done, dt)
            done = n
            want = [d["%s%d_%s" % (prefix, n, k)] for k in "puvtq"]
            # the harness IC has |u|,|v| ~ 1e-3 after growth from one 0.1 m/s cell: compare
            # winds on the scale of the driving field instead of their own tiny max
            got = c.get_state()
            for k, x, y in zip("puvtq", got, want):
                scale = max(np.max(np.abs(y)), 1e-2 if k in "uv" else 0)
                assert np.max(np.abs(x - y)) / scale < TOL, (prefix, n, k)
        c.close()


def test_geography_harness_h1(g):
    """test_geography.py:6-23,49: H = 1, W = 16, L = 17 with a 1000 m bump"""
    from gcmiipy_amd import geometry
    d = golden("g8_pe25d")
    geom = geometry.gen_geometry(1, 16, 17, sig_func=geometry.manabe_sig)
    geom.heightmap[0, 8] = 1000
    from oracle import driver, geometry as ogeo
    og = ogeo.gen_geometry(1, 16, 17, sig_func=ogeo.manabe_sig)
    p, u, v, t, q, _ = driver.gen_initial_conditions(og)
    v[0, 0, 0] = 0.1
    u *= 0
    c = g.Core(g._lib.PE25D, 16, 1, 17, geom=geom)
    c.set_state(p, u, v, t, q)
    c.step(3, 1800.0)
    _check(c.get_state(), [d["bump3_" + k] for k in "puvtq"], "bump3")
    c.close()


@pytest.mark.parametrize("hwl", [(8, 16, 4), (6, 10, 3), (5, 12, 1), (12, 20, 5), (7, 30, 2),
                                 (3, 1440, 2), (4, 2880, 3), (3, 14, 2), (2, 2250, 1), (3, 400, 2), (2, 1250, 1),
                                 (2, 4096, 2), (3, 1458, 3), (4, 120, 3), (3, 256, 2), (2, 4608, 1), (3, 202, 2)])
def test_shapes_vs_oracle(g, hwl):
    """ragged sizes: odd L (unpaired level in the packed FFT), radix-3/5 widths, L = 1; the row
    lengths of BASELINE configs[3] / [4] (1440, 2880: in-place FFT), a radix-7 length (generic
    butterfly, generic ping-pong path), 2250 = 10.15.15, 400 = 20.20 and 1250 = 10.25.5 (the widest
    composite radices), 4096 = 16.16.16; 1458 = 6.9.9.3 (the only four-pass plan), 120 = 10.12 and
    256 = 16.16 (the kMask1440 / kMask4096 kernels in two passes), 4608 (a {2,3}-smooth width the
    generic path serves: a pass of 1152 butterflies), 202 = 2.101 (the generic radix-r butterfly)"""
    from gcmiipy_amd import geometry
    from oracle import dynamics as odyn, geometry as ogeo
    H, W, L = hwl
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    og = ogeo.gen_geometry(H, W, L, sig_func=ogeo.manabe_sig)
    p, u, v, t, q = want = inp.state(og, H * 100 + W)
    for _ in range(2):
        want = odyn.matsuno_timestep(*want, 60.0, og)
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom)
    c.set_state(p, u, v, t, q)
    c.step(2, 60.0)
    _check(c.get_state(), want, hwl)
    c.close()


def test_filter_off_and_odd_width(g):
    from gcmiipy_amd import geometry
    geom = geometry.gen_geometry(6, 9, 2)
    with pytest.raises(ValueError, match="even width"):
        g.Core(g._lib.PE25D, 9, 6, 2, geom=geom)
    c = g.Core(g._lib.PE25D, 9, 6, 2, geom=geom, filter=False)      # runs without the filter
    c.close()


def test_harness_run_model_stats_and_energy(g):
    """no_limits_2_5d.run_model at its main() size 8x8x3, dt = 1800 s: states after 1/3/10 steps,
    STATS extrema and calc_energy vs values captured from the reference (G8)."""
    from gcmiipy_amd import no_limits_2_5d as h
    d = golden("g8_pe25d")
    stats = {k: [] for k in ("u_max", "u_min", "v_max", "v_min", "ke")}
    snaps = {}

    def cb(p, u, v, t, q, _n=[0]):
        _n[0] += 1
        if _n[0] in (1, 3, 10):
            snaps[_n[0]] = (p, u, v, t, q)

    h.run_model(8, 8, 3, 1800.0, 10, cb, stats=stats)
    for n, st in snaps.items():
        for k, x in zip("puvtq", st):
            y = d["harness%d_%s" % (n, k)]
            scale = max(np.max(np.abs(y)), 1e-2 if k in "uv" else 0)
            assert np.max(np.abs(x - y)) / scale < TOL, (n, k)
    for k in ("u_max", "u_min", "v_max", "v_min"):
        assert np.max(np.abs(np.asarray(stats[k]) - d["harness_stats_" + k])) < 1e-12, k
    assert rel_err(np.asarray(stats["ke"])[:, 1:], d["harness_stats_ke"][:, 1:]) < 1e-12
    ke, ke_ref = np.asarray(stats["ke"])[:, 0], d["harness_stats_ke"][:, 0]
    assert np.max(np.abs(ke - ke_ref)) < 1e-9 * np.max(ke_ref)
    with pytest.raises(ValueError, match="broadcast"):
        from gcmiipy_amd import geometry
        geom = geometry.gen_geometry(6, 8, 2)
        h.calc_energy(*h.gen_initial_conditions(geom)[:5], None, geom)     # W != H: reference raises too


def test_geography_energy(g):
    from gcmiipy_amd import no_limits_2_5d as h
    d = golden("g8_pe25d")
    p, u, v, t, q, gr, geom = h.run_model(1, 16, 17, 1800.0, 3, None, stats={k: [] for k in
                                          ("u_max", "u_min", "v_max", "v_min", "ke")}, bump=(0, 8, 1000))
    _check((p, u, v, t, q), [d["bump3_" + k] for k in "puvtq"], "bump3 via run_model")
    assert rel_err(np.asarray(h.calc_energy(p, u, v, t, q, gr, geom)), d["bump3_energy"]) < 1e-12


def test_checkpoint_resume_bit_exact(g, tmp_path):
    """save after 2 steps, restore into a fresh Core, 2 more steps == 4 uninterrupted steps"""
    from gcmiipy_amd import geometry, checkpoint
    d = golden("g8_pe25d")
    geom = geometry.gen_geometry(24, 36, 9, sig_func=geometry.manabe_sig)
    ic = [d["dense_%s0" % k] for k in "puvtq"]
    a = g.Core(g._lib.PE25D, 36, 24, 9, geom=geom)
    a.set_state(*ic)
    a.step(2, 300.0)
    path = str(tmp_path / "ck.npz")
    checkpoint.save(path, a, step=2, time=600.0, geom=geom, note=np.asarray([1.0]))
    a.step(2, 300.0)
    want = a.get_state()
    a.close()
    b, ck = checkpoint.restore(path)
    assert ck["step"] == 2 and ck["time"] == 600.0 and ck["model"] == "PE25D"
    assert np.array_equal(ck["geom"].dx_j, geom.dx_j)
    b.step(2, 300.0)
    for x, y in zip(b.get_state(), want):
        assert np.array_equal(x, y)
    b.close()


def test_checkpoint_is_self_contained(g, tmp_path):
    """a handle with the column physics, Coriolis terms and fp32 storage, and a 2-D handle with the
    tracer: restore() needs nothing but the file, and the resumed runs match the uninterrupted ones"""
    from gcmiipy_amd import geometry, checkpoint
    d = golden("g8_pe25d")
    geom = geometry.gen_geometry(24, 36, 9, sig_func=geometry.manabe_sig)
    ic = [d["dense_%s0" % k] for k in "puvtq"]
    gt = np.full((24, 36), 288.0)
    for dtype in ("f64", "f32"):
        a = g.Core(g._lib.PE25D, 36, 24, 9, geom=geom, coriolis=True, dtype=dtype)
        a.set_state(*ic)
        a.set_ground(gt)
        for n in range(2):
            a.step(1, 300.0)
            a.solar_step(geom, 300.0, n * 300.0)
        path = str(tmp_path / ("ck_%s.npz" % dtype))
        checkpoint.save(path, a, step=2, time=600.0, geom=geom)
        for n in range(2, 4):
            a.step(1, 300.0)
            a.solar_step(geom, 300.0, n * 300.0)
        want, want_gt = a.get_state(), a.get_ground()
        a.close()
        b, ck = checkpoint.restore(path)
        assert b.dtype == dtype and b.options["coriolis"] and b.has_ground
        for n in range(2, 4):
            b.step(1, 300.0)
            b.solar_step(ck["geom"], 300.0, n * 300.0)
        for x, y in zip(b.get_state(), want):
            assert np.array_equal(x, y), dtype
        assert np.array_equal(b.get_ground(), want_gt)
        b.close()
    rng = np.random.default_rng(4)
    f = dict(u=rng.standard_normal((16, 40)), v=rng.standard_normal((16, 40)), p=101325 + rng.standard_normal((16, 40)),
             t=273.16 + rng.standard_normal((16, 40)), q=rng.random((16, 40)))
    a = g.Core(g._lib.SW2D_TEMP, 40, 16, dx=300e3, tracer=g._lib.TRACER_UPWIND, variant=g._lib.VARIANT_STAGED)
    a.set_state(**f)
    a.step(3, 300.0)
    path = str(tmp_path / "ck2d.npz")
    checkpoint.save(path, a, step=3)
    a.step(2, 300.0)
    want = a.get_state()
    a.close()
    b, ck = checkpoint.restore(path)                       # dx, the upwind tracer and the staged variant come from the file
    assert b.options["tracer"] == g._lib.TRACER_UPWIND and b.options["dx"] == 300e3
    b.step(2, 300.0)
    for x, y in zip(b.get_state(), want):
        assert (x is None and y is None) or np.array_equal(x, y)
    b.close()


def test_coriolis_option_vs_golden(g):
    """optional Coriolis terms (dynamics.py:82-92, off in the reference) vs the reference's own
    expressions run with the switch flipped (G12)"""
    from gcmiipy_amd import geometry, dynamics
    d = golden("g12_coriolis")
    L, H, W = d["u0"].shape
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    st = [d[k + "0"] for k in "puvtq"]
    for n in (1, 2):
        st = dynamics.matsuno_timestep(*st, float(d["dt"]), geom, coriolis=True)
        _check(st, [d["step%d_%s" % (n, k)] for k in "puvtq"], "coriolis step %d" % n)
    off = dynamics.matsuno_timestep(*[d[k + "0"] for k in "puvtq"], float(d["dt"]), geom)
    assert rel_err(off[1], d["step1_u"]) > 1e-6          # the terms do change the answer


def test_grey_radiation_and_solar_timestep(g):
    """column physics vs values captured from grey_solar.basic_grey_radiation and
    no_limits_2_5d.solar_timestep (G13)"""
    from gcmiipy_amd import geometry, grey_solar
    d = golden("g13_radiation")
    L, H, W = d["t0"].shape
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    p, t, gt = d["p0"], d["t0"], d["gt0"]
    gv = grey_solar.GroundVars(gt, None, None, None)
    tp = p * geom.sig + geom.ptop
    tt = t / ((1e5 / tp) ** (287.0 / 1004.0))
    for tag in "ab":
        utc = float(d["utc_" + tag])
        dTdt, dtg = grey_solar.basic_grey_radiation(p, tp, tt, gv, 0.1, 0.9, 0.3, utc, geom)
        assert rel_err(dTdt, d["dTdt_" + tag]) < TOL
        assert rel_err(dtg, d["dtg_" + tag]) < TOL
        t_n, g_n = grey_solar.solar_timestep(t, p, gv, float(d["dt"]), utc, geom)
        assert rel_err(t_n, d["t_n_" + tag]) < TOL
        assert rel_err(g_n.gt, d["gt_n_" + tag]) < TOL


def test_grey_radiation_fp32_handle(g):
    """the column physics on a float32 handle (float64 arithmetic, float32 storage) against the
    float64 handle: tendencies and the stepped theta to float32 resolution"""
    from gcmiipy_amd import geometry
    d = golden("g13_radiation")
    L, H, W = d["t0"].shape
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    z = np.zeros((L, H, W))
    res = {}
    for dt_name in ("f64", "f32"):
        c = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype=dt_name)
        c.set_state(d["p0"], z, z, d["t0"], z)
        c.set_ground(d["gt0"])
        dTdt, dtg = c.grey_radiation(geom, float(d["utc_a"]))
        c.solar_step(geom, float(d["dt"]), float(d["utc_a"]))
        res[dt_name] = (dTdt, dtg, c.get_state()[3], c.get_ground())
        c.close()
    assert rel_err(res["f64"][0], d["dTdt_a"]) < TOL and rel_err(res["f64"][2], d["t_n_a"]) < TOL
    for a, b, tol in zip(res["f32"], res["f64"], (2e-5, 2e-5, 3e-7, 1e-7)):
        assert rel_err(a, b) < tol, (rel_err(a, b), tol)


@pytest.mark.parametrize("hwl", [(12, 20, 9), (6, 16, 24), (5, 12, 5)])
def test_level_segments_do_not_change_results(g, hwl, monkeypatch):
    """the update kernel may march a column in 2-4 level segments (GCM_PE_LEVEL_SEGMENTS; pit then
    comes from the 3-D fields, pe_pit_kernel); the partial sums it then starts from are bit-identical
    to the unsplit march on the same pit"""
    from gcmiipy_amd import geometry
    H, W, L = hwl
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    p, u, v, t, q = inp.state(geom, 11)
    res = {}
    monkeypatch.setenv("GCM_PE_PIT2D", "0")
    for nseg in (1, 2, 3, 4):
        monkeypatch.setenv("GCM_PE_LEVEL_SEGMENTS", str(nseg))
        c = g.Core(g._lib.PE25D, W, H, L, geom=geom, coriolis=(nseg > 0 and H == 12))
        c.set_state(p, u, v, t, q)
        c.step(3, 120.0)
        res[nseg] = c.get_state()
        c.close()
    for nseg in (2, 3, 4):
        for a, b in zip(res[nseg], res[1]):
            assert np.array_equal(a, b), nseg


@pytest.mark.parametrize("hwl", [(12, 20, 9), (6, 16, 24), (36, 1440, 5)])
def test_pit_from_column_sums_vs_3d_form(g, hwl, monkeypatch):
    """pit = sum_k dsig conv[k] is evaluated from the 2-D column sums of the winds (pe_pit2d_kernel: the
    filter is linear, so one filtered row per latitude; the default) or level by level from the 3-D
    fields (pe_pit_kernel, GCM_PE_PIT2D=0; the reference's order, dynamics.py:38-40).  The sum is
    reassociated, nothing else: both within 1e-13 of each other after 3 steps, and the default within
    TOL of the oracle."""
    from gcmiipy_amd import geometry
    from oracle import dynamics as od, geometry as ogeo
    H, W, L = hwl
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    p, u, v, t, q = inp.state(geom, 12)
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("GCM_PE_PIT2D", flag)
        c = g.Core(g._lib.PE25D, W, H, L, geom=geom)
        c.set_state(p, u, v, t, q)
        c.step(3, 120.0)
        res[flag] = c.get_state()
        c.close()
    for a, b in zip(res["1"], res["0"]):
        assert rel_err(a, b) < 1e-13
    if W <= 64:
        st = (p, u, v, t, q)
        og = ogeo.gen_geometry(H, W, L, sig_func=ogeo.manabe_sig)
        for _ in range(3):
            st = od.matsuno_timestep(*st, 120.0, og)
        for a, b in zip(res["1"], st):
            assert rel_err(a, b) < TOL


def test_full_size_properties_c4(g):
    """BASELINE configs[3] size (1440x720x24), 3 steps: properties that do not need the oracle --
    sum(p) is conserved (the continuity equation is in flux form: the zonal term telescopes per
    row, the meridional one over the closed pole edge), the pole-edge v row is exactly zero
    (dynamics.py:222), nothing goes non-finite.  (The oracle comparison at this size and
    "8 bands == single domain" are in test_full_size_gpu.py.)"""
    from gcmiipy_amd import geometry
    H, W, L = 720, 1440, 24
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    p, u, v, t, q = inp.state(geom, 0)
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom)
    c.set_state(p, u, v, t, q)
    c.step(3, 1.0)
    assert c.diag(g._lib.DIAG_ANY_NAN) == 0.0
    pn, un, vn, tn, qn = c.get_state()
    c.close()
    assert abs(pn.sum() - p.sum()) < 1e-12 * p.sum()
    assert np.all(vn[:, -1, :] == 0.0)
    assert all(np.isfinite(x).all() for x in (pn, un, vn, tn, qn))
    assert np.max(np.abs(un - u)) > 1e-6                    # it did move


def test_fp32_tolerance_sweep(g):
    """BASELINE configs[4] names an fp32 vs fp64 tolerance sweep: the fp32 handle (arithmetic and
    storage in float, host API float64) against the fp64 one after 1 / 10 / 100 steps.  fp32 has
    ~1.2e-7 resolution on fields of magnitude 1e5 (p) and 3e2 (theta); the winds are O(1)."""
    from gcmiipy_amd import geometry
    d = golden("g8_pe25d")
    geom = geometry.gen_geometry(24, 36, 9, sig_func=geometry.manabe_sig)
    ic = [d["dense_%s0" % k] for k in "puvtq"]
    c64 = g.Core(g._lib.PE25D, 36, 24, 9, geom=geom)
    c32 = g.Core(g._lib.PE25D, 36, 24, 9, geom=geom, dtype="f32")
    c64.set_state(*ic)
    c32.set_state(*ic)
    done, errs = 0, {}
    for n in (1, 10, 100):
        c64.step(n - done, 30.0)
        c32.step(n - done, 30.0)
        done = n
        a, b = c32.get_state(), c64.get_state()
        errs[n] = [rel_err(x, y) for x, y in zip(a, b)]
        assert all(np.isfinite(x).all() for x in a)
    c64.close()
    c32.close()
    assert max(errs[1]) < 2e-6, errs                      # one step: rounding of the state itself
    assert max(errs[1][0], errs[1][3]) < 2e-7, errs        # p and theta to fp32 resolution
    assert max(errs[100]) < 5e-2, errs                     # error growth stays bounded over 100 steps
    assert errs[100][0] < 1e-5 and errs[100][3] < 1e-5, errs
    # vs the golden (reference) fp64 values after 10 steps the fp32 run is within its own resolution
    print("fp32 vs fp64 relative error (p,u,v,t,q):", {k: ["%.1e" % e for e in v] for k, v in errs.items()})


def test_fp32_bands_in_process(g):
    import torch
    H, W, L, steps, nb = 14, 20, 5, 2, 2
    geom = su.geom_of(H, W, L)
    st = inp.state(geom, 3)
    ref = su.single(g, geom, st, dtype="f32")
    ref.step(steps, 120.0)
    want = ref.get_state()
    ref.close()
    cores = su.bands(g, geom, nb, st, dtype="f32")
    for _ in range(steps):
        su.exchange(cores, torch)
        for c in cores:
            c.step_interior(120.0)
        su.exchange(cores, torch)
        for c in cores:
            c.step_boundary(120.0)
    parts = [c.get_state() for c in cores]
    for c in cores:
        c.close()
    for f in range(5):
        got = np.concatenate([p_[f] for p_ in parts], axis=0 if f == 0 else 1)
        assert np.array_equal(got, want[f]), f             # same fp32 arithmetic per row: bit-identical


def _tap(c, g):
    L = g._lib
    return {"spu": c.get_intermediate(L.INT_SPU), "pit": c.get_intermediate(L.INT_PIT), "p_n": c.get_intermediate(L.INT_PN),
            "phi": c.get_intermediate(L.INT_PHI), "pgfu": c.get_intermediate(L.INT_PGFU)}


def test_hot_path_intermediates_vs_golden(g):
    """G7: spu, pit, p_n, phi and pgfu as the STAGE kernels K1 / K2a / K2b' / K3 leave them in the handle
    (gcm_get_intermediate: a tap, not a recomputation), predictor and corrector, against the reference's
    own intermediates (dynamics.py:35-46,111-171,186-205) -- a mistake inside the fused stage is localised
    by the intermediate that fails, not only by the stage output"""
    from gcmiipy_amd import geometry
    d = golden("g7_half_step")
    L, H, W = d["u0"].shape
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    geom.heightmap[...] = d["heightmap"]
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom)
    with pytest.raises(g.GcmError):
        c.get_intermediate(g._lib.INT_SPU)                       # no half step yet
    c.set_state(*[d[k + "0"] for k in "puvtq"])
    for stage, name in ((0, "pred"), (1, "corr")):
        c.half_step(stage, float(d["dt"]))
        got = _tap(c, g)
        for k in ("spu", "pit", "p_n", "phi", "pgfu"):
            e = rel_err(got[k], d["%s_%s" % (name, k)])
            assert e < TOL, (name, k, e)
    with pytest.raises(ValueError):
        c.get_intermediate(99)
    c.close()


def test_hot_path_intermediates_vs_oracle_1440_columns(g):
    """the same tap at the production row length (1440 columns: the composite-radix transform, the looping
    K1 with pit in its launch, K3's batched sweep), 8 rows x 24 levels, predictor and corrector vs the oracle"""
    from gcmiipy_amd import geometry
    from oracle import dynamics as od, geometry as ogeo
    H, W, L = 8, 1440, 24
    rng = np.random.default_rng(21)
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    og = ogeo.gen_geometry(H, W, L, sig_func=ogeo.manabe_sig)
    geom.heightmap[...] = og.heightmap[...] = 30 * rng.random((H, W))
    base, dt = inp.state(og, rng), 30.0
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom)
    c.set_state(*base)
    stage_state = base
    for stage in (0, 1):
        tap = {}
        out = od.half_timestep(*base, *stage_state, dt, og, _tap=tap)
        tap["phi"] = od.compute_geopotential(stage_state[0], stage_state[3], og)
        tap["p_n"] = out[0]
        c.half_step(stage, dt)
        got = _tap(c, g)
        for k in ("spu", "pit", "p_n", "phi", "pgfu"):
            e = rel_err(got[k], tap[k])
            assert e < TOL, (stage, k, e)
        stage_state = out
    for a, b, k in zip(c.get_state(), stage_state, "puvtq"):
        assert rel_err(a, b) < TOL, k
    c.close()


def test_set_physics_is_the_explicit_loop(g):
    """gcm_set_physics: every step of gcm_step = matsuno_timestep + solar_timestep at the handle's clock, clock += dt
    (the loop of no_limits_2_5d.run_model, :229-234, with the physics below full_timestep's early return) -- bit for
    bit the explicit sequence of calls, which golden g13 and the 2880x1440x40 strips pin against the reference; and
    the error paths"""
    from gcmiipy_amd import geometry
    from gcmiipy_amd.core import GcmError
    d = golden("g8_pe25d")
    geom = geometry.gen_geometry(24, 36, 9, sig_func=geometry.manabe_sig)
    ic = [d["dense_%s0" % k] for k in "puvtq"]
    gt = 288.0 + np.random.default_rng(3).standard_normal((24, 36))
    utc0, dt = 4 * 3600.0, 300.0
    for dtype in ("f64", "f32"):
        a = g.Core(g._lib.PE25D, 36, 24, 9, geom=geom, dtype=dtype)
        a.set_state(*ic)
        a.set_ground(gt)
        utc = utc0
        for n in range(3):
            a.step(1, dt)
            a.solar_step(geom, dt, utc)
            utc += dt
        want, want_gt = a.get_state(), a.get_ground()
        a.close()
        b = g.Core(g._lib.PE25D, 36, 24, 9, geom=geom, dtype=dtype)
        b.set_state(*ic)
        with pytest.raises(GcmError, match="no physics registered"):
            b.utc()
        b.set_physics(geom, utc0)
        with pytest.raises(GcmError, match="ground temperature first"):
            b.step(1, dt)                                  # the physics needs gcm_set_ground
        b.set_ground(gt)
        b.step(2, dt)
        b.step(1, dt)
        assert b.utc() == utc
        for x, y in zip(b.get_state(), want):
            assert np.array_equal(x, y), dtype
        assert np.array_equal(b.get_ground(), want_gt)
        b.set_physics(None)                                # dynamics only again
        t0 = b.get_ground()
        b.step(1, dt)
        assert np.array_equal(b.get_ground(), t0)
        b.close()
    sw = g.Core(g._lib.SW2D, 32, 16, dx=300e3)
    with pytest.raises(GcmError, match="GCM_PE25D only"):
        sw.set_physics(geometry.gen_geometry(16, 32, 2, sig_func=geometry.manabe_sig), 0.0)
    sw.close()


def test_run_model_with_physics_vs_oracle(g):
    """the whole loop of BASELINE configs[4] as a user would run it -- gen_initial_conditions, then per step
    matsuno_timestep + solar_timestep at utc = 0, dt, 2 dt ... -- through the drop-in run_model(physics=True) (one
    gcm_step per step on the device) against the oracle's functions called in the reference's order"""
    from gcmiipy_amd import no_limits_2_5d as m
    from oracle import driver, dynamics as odyn, physics, geometry as ogeo
    H, W, L, dt, steps = 16, 16, 5, 900.0, 4          # (square: the STATS record broadcasts geom.area (H,) against W)
    stats = {k: [] for k in ("u_max", "u_min", "v_max", "v_min", "ke")}
    got = m.run_model(H, W, L, dt, steps, None, stats=stats, physics=True)
    og = ogeo.gen_geometry(H, W, L, sig_func=ogeo.manabe_sig)
    p, u, v, t, q, gt = driver.gen_initial_conditions(og)
    gt = np.asarray(getattr(gt, "gt", gt), dtype=np.float64)
    v[0, 0, 0] = 0.1
    u *= 0
    st, utc = (p, u, v, t, q), 0.0
    for _ in range(steps):
        st = list(odyn.matsuno_timestep(*st, dt, og))
        st[3], gt = physics.solar_timestep(st[3], st[0], gt, dt, utc, og)
        utc += dt
    for k, x, y in zip("puvtq", got[:5], st):
        assert rel_err(x, y) < 1e-10, (k, rel_err(x, y))
    assert rel_err(got[5].gt, gt) < 1e-10
    assert not np.array_equal(got[5].gt, np.full((H, W), 360.0))          # the ground did cool / warm
