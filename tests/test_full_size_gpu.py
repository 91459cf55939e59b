"""GPU parity at the BASELINE.json sizes, against the oracle (not HIP against HIP).

  configs[1]  720x360 shallow water            10 steps (odd count: pair launches + one single)
  configs[2]  4096x2048 SW + theta + viscosity + van-Leer tracer, fused, 2 steps
  configs[3]  1440x720x24 primitive equations  1 step vs the whole-grid oracle; 360x180x24 2 steps;
              8 latitude bands == single domain, bit for bit
  configs[4]  2880x1440x40 primitive equations + grey radiation + humidity: the oracle on latitude
              strips of the full-size state (the operators reach 2 rows along j, the filter and the
              column scans stay inside a row / a column, so a strip with a few spare rows reproduces
              the whole-grid result on its inner rows), conservation properties, fp32 vs fp64 sweep

Tolerance 1e-10 relative (L-inf over max|field|), BASELINE.json's north_star figure."""
import copy

import numpy as np
import pytest

from conftest import rel_err
import gpu_setups as su
import pe25d_inputs as inp
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu
TOL = 1e-10
DX = 300e3


# ------------------------------------------------------------------ configs[1], configs[2]
def test_c2_720x360_ten_steps_vs_oracle(g):
    from oracle import sw2d
    rng = np.random.default_rng(0)
    H, W = 360, 720
    u, v = rng.standard_normal((H, W)), rng.standard_normal((H, W))
    p = 8000 + rng.standard_normal((H, W))
    want = (u, v, p)
    for _ in range(11):
        want = sw2d.matsumo_scheme(*want, DX, 300.0)
    for name, var in (("fused", g._lib.VARIANT_FUSED), ("staged", g._lib.VARIANT_STAGED)):
        c = g.Core(g._lib.SW2D, W, H, dx=DX, variant=var)
        c.set_state(p=p, u=u, v=v)
        c.step(11, 300.0)                   # fused: five two-step launches and one single step
        pn, un, vn, _, _ = c.get_state((0, 1, 2))
        c.close()
        for k, x, y in zip("uvp", (un, vn, pn), want):
            assert rel_err(x, y) < TOL, (name, k, rel_err(x, y))


def test_c3_4096x2048_fused_two_steps_vs_oracle(g):
    from oracle import sw2d_temp, tracer
    rng = np.random.default_rng(0)
    H, W = 2048, 4096
    u, v = rng.standard_normal((H, W)), rng.standard_normal((H, W))
    p = 101325 + rng.standard_normal((H, W))
    t = 273.16 + rng.standard_normal((H, W))
    q = rng.random((H, W))
    c = g.Core(g._lib.SW2D_TEMP, W, H, dx=DX, tracer=g._lib.TRACER_VANLEER, variant=g._lib.VARIANT_FUSED)
    c.set_state(p=p, u=u, v=v, t=t, q=q)
    c.step(2, 300.0)
    pn, un, vn, tn, qn = c.get_state()
    c.close()
    st, qq = (u, v, p, t), q
    for _ in range(2):
        qq = tracer.limited_advection(300.0, (DX, DX), np.stack([st[1], st[0]]), qq)   # time-n winds
        st = sw2d_temp.matsumo_scheme(*st, DX, 300.0)
    for k, x, y in zip("uvptq", (un, vn, pn, tn, qn), (*st, qq)):
        assert rel_err(x, y) < TOL, (k, rel_err(x, y))


# ------------------------------------------------------------------ configs[3]
@pytest.mark.parametrize("hwl,steps", [((180, 360, 24), 2), ((720, 1440, 24), 1)])
def test_c4_whole_grid_vs_oracle(g, hwl, steps):
    from gcmiipy_amd import geometry
    from oracle import dynamics as odyn, geometry as ogeo
    H, W, L = hwl
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    og = ogeo.gen_geometry(H, W, L, sig_func=ogeo.manabe_sig)
    ic = inp.state(og, 0)
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom)
    c.set_state(*ic)
    c.step(steps, 1.0)
    got = c.get_state()
    c.close()
    want = ic
    for _ in range(steps):
        want = odyn.matsuno_timestep(*want, 1.0, og)
    for k, x, y in zip("puvtq", got, want):
        assert rel_err(x, y) < TOL, (hwl, k, rel_err(x, y))
        # the increments too: a 1 s step moves theta by 1e-6 of its size
    for k, x, y, z in zip("puvtq", got, want, ic):
        assert rel_err(x - z, y - z) < 1e-6, (hwl, "increment", k, rel_err(x - z, y - z))


def test_c4_eight_bands_equal_single_domain(g):
    """1440x720x24 split into the 8 bands of BASELINE configs[3] (90 rows each, their own number
    of level segments), ghost rows moved by device copies: bit-identical to the single domain"""
    import torch
    H, W, L, steps, nb = 720, 1440, 24, 2, 8
    geom = su.geom_of(H, W, L)
    st = inp.state(geom, 0)
    ref = su.single(g, geom, st)
    ref.step(steps, 1.0)
    want = ref.get_state()
    ref.close()
    cores = su.bands(g, geom, nb, st)
    for _ in range(steps):
        su.exchange(cores, torch)
        for c in cores:
            c.step_interior(1.0)
        su.exchange(cores, torch)
        for c in cores:
            c.step_boundary(1.0)
    parts = [c.get_state() for c in cores]
    for c in cores:
        c.close()
    for f in range(5):
        got = np.concatenate([x[f] for x in parts], axis=0 if f == 0 else 1)
        assert np.array_equal(got, want[f]), "puvtq"[f]


# ------------------------------------------------------------------ configs[4]
def strip_geom(og, rows):
    """the oracle geometry restricted to the (wrapped) global rows `rows`"""
    sg = copy.copy(og)
    sg.height = len(rows)
    sg.dx_j = og.dx_j[:, rows, :]
    sg.dx_h = og.dx_h[:, rows, :]
    sg.lat = og.lat[rows]
    sg.heightmap = og.heightmap[rows]
    return sg


def oracle_strip_step(og, state, gt, j0, j1, dt, utc, pad=6):
    """one dynamics step (+ solar_timestep when gt is given) of global rows [j0, j1) by the oracle
    on the strip [j0 - pad, j1 + pad); rows wrap as np.roll does on the whole grid, and the
    pole-edge rule v_n[:, -1, :] *= 0 (dynamics.py:222) is applied to the GLOBAL last row through
    the reference's boundary_conditions hook."""
    from oracle import dynamics as odyn, physics
    H = og.height
    rows = np.arange(j0 - pad, j1 + pad) % H
    sg = strip_geom(og, rows)
    p, u, v, t, q = state
    sl = (p[rows], u[:, rows], v[:, rows], t[:, rows], q[:, rows])
    last = np.nonzero(rows == H - 1)[0]

    def pole(sp, su, sv, st, sq, dt_, geom_):
        sv = sv.copy()
        sv[:, last, :] *= 0
        return sp, su, sv, st, sq
    out = list(odyn.matsuno_timestep(*sl, dt, sg, boundary_conditions=pole))
    gt_n = None
    if gt is not None:
        out[3], gt_n = physics.solar_timestep(out[3], out[0], gt[rows], dt, utc, sg)
        gt_n = gt_n[pad:-pad]
    inner = slice(pad, len(rows) - pad)
    return [out[0][inner]] + [x[:, inner] for x in out[1:]], gt_n


def test_c5_2880x1440x40_strips_properties_fp32_sweep(g):
    from gcmiipy_amd import geometry
    from oracle import geometry as ogeo
    H, W, L = 1440, 2880, 40
    dt, utc = 1.0, 6 * 3600.0
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    og = ogeo.gen_geometry(H, W, L, sig_func=ogeo.manabe_sig)
    ic = inp.state(og, 0)
    rng = np.random.default_rng(5)
    gt = 288.0 + rng.standard_normal((H, W))
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom)
    c.set_state(*ic)
    c.set_ground(gt)
    c.step(1, dt)
    dyn = c.get_state()
    c.solar_step(geom, dt, utc)
    got = c.get_state()
    got_gt = c.get_ground()
    # properties that hold at any size (after the dynamics step)
    assert c.diag(g._lib.DIAG_ANY_NAN) == 0.0
    assert abs(dyn[0].sum() - ic[0].sum()) < 1e-12 * ic[0].sum()
    assert np.all(dyn[2][:, -1, :] == 0.0)
    assert all(np.isfinite(x).all() for x in got)
    for f in (0, 1, 2, 4):                                   # the radiation touches theta only
        assert np.array_equal(dyn[f], got[f])
    # the oracle on strips: both poles (strongest filter; the wrap; the global last row) and mid-latitudes
    for j0, j1 in ((0, 6), (717, 723), (H - 6, H)):
        want, want_gt = oracle_strip_step(og, ic, gt, j0, j1, dt, utc)
        sl = slice(j0, j1)
        for k, x, y in zip("puvtq", got, want):
            xs = x[sl] if x.ndim == 2 else x[:, sl]
            assert rel_err(xs, y) < TOL, ((j0, j1), k, rel_err(xs, y))
        assert rel_err(got_gt[sl], want_gt) < TOL
    # fp32 handle vs fp64 handle, dynamics + radiation, after 1 and 10 steps
    c32 = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype="f32")
    c32.set_state(*ic)
    c32.set_ground(gt)
    c.set_state(*ic)
    c.set_ground(gt)
    done, errs = 0, {}
    for n in (1, 10):
        for _ in range(n - done):
            for cc in (c, c32):
                cc.step(1, dt)
                cc.solar_step(geom, dt, utc + done * dt)
        done = n
        a, b = c32.get_state(), c.get_state()
        errs[n] = [rel_err(x, y) for x, y in zip(a, b)]
        assert all(np.isfinite(x).all() for x in a)
        del a, b
    c.close()
    c32.close()
    print("c5 fp32 vs fp64 (p,u,v,t,q):", {k: ["%.1e" % e for e in v] for k, v in errs.items()})
    # measured (profiles/r01/c5_fp32_sweep.json): 1 step p 7.8e-8, theta 3.0e-7, u 4.8e-6;
    # 10 steps p 3.8e-7, theta 1.0e-6, u 4.0e-5 -- bounds at ~3x those
    assert errs[1][0] < 3e-7 and errs[1][3] < 1e-6, errs     # p, theta: fp32 resolution
    assert max(errs[1]) < 2e-5, errs
    assert errs[10][0] < 1.5e-6 and errs[10][3] < 4e-6, errs
    assert max(errs[10]) < 2e-4, errs
