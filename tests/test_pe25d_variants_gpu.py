"""GCM_PE25D instantiations that the product grids do not reach, against the float64 oracle: the filter plans of every
class (test_pe25d_variants_cpu.py pins which instantiation each width selects), the fp32 builds of all of them, level
counts around the LMAX = 24 / 40 / 0 forms of the column kernels up to the largest L the handle accepts, and
ptop != 0 (the radiation kernels without FACT).  Errors are L-inf over max|reference|."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_err
import gpu_setups as su
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)
from test_pe25d_variants_cpu import FILTER_WIDTHS

pytestmark = pytest.mark.gpu
TOL = 1e-10
# fp32 bounds of one step (test_pe25d_gpu.test_fp32_tolerance_sweep): all fields, and p and theta.  Measured over the
# widths of test_one_step_fp32_vs_oracle: u 3.9e-7 (120), theta 2.0e-7 (4800: the roundings of the flux-form update), p 3.9e-8
F32_STEP, F32_PT = 2e-6, 2e-7
# fp32 filter alone, input rounded to float32 first: worst measured 7.5e-7 (4800; 1440 6.3e-7), relative to an output
# the filter has damped well below its input; 3x that would exceed the 1e-6 cap
F32_FILTER = 1e-6
# the column physics on a float32 handle (test_pe25d_gpu.test_grey_radiation_fp32_handle): dTdt, dt_ground, theta, gt
F32_RAD = (2e-5, 2e-5, 3e-7, 1e-7)
L_MAX = 156          # pe25d_create: the radiation kernel's LDS park, 8 L 128 bytes + 4 KB <= 160 KB (both dtypes)
PTOP = 5000.0


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _state(H, W, L, og, seed, f32=False):
    """test_shapes_vs_oracle's state, p about 1e5 - ptop; f32: rounded to float32 (what the handle holds)"""
    from oracle import temperature as otemp
    rng = np.random.default_rng(seed)
    p = 1e5 - og.ptop + 10 * rng.standard_normal((H, W))
    u = rng.standard_normal((L, H, W))
    v = rng.standard_normal((L, H, W))
    v[:, -1, :] = 0
    t = otemp.to_potential_temp(300 + rng.standard_normal((L, H, W)), p * og.sig + og.ptop)
    q = 3e-6 * (1 + 0.1 * rng.random((L, H, W)))
    st = (p, u, v, t, q)
    return tuple(_f32(x) for x in st) if f32 else st


def _oracle(st, nsteps, dt, og):
    from oracle import dynamics as odyn
    for _ in range(nsteps):
        st = odyn.matsuno_timestep(*st, dt, og)
    return st


def _run(g, geom, st, nsteps, dt, dtype="f64"):
    L, H, W = st[1].shape
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype=dtype)
    c.set_state(*st)
    c.step(nsteps, dt)
    out = c.get_state()
    c.close()
    return out


def _check(got, want, what, tol=TOL, tol_pt=None):
    errs = {k: rel_err(x, y) for k, x, y in zip("puvtq", got, want)}
    print(what, " ".join("%s %.2e" % kv for kv in errs.items()))
    for k, e in errs.items():
        assert e < (tol_pt if tol_pt is not None and k in "pt" else tol), (what, k, e)
    return errs


# ---------------------------------------------------------------- B. the filter on its own
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("W", FILTER_WIDTHS)
def test_polar_filter_vs_oracle(g, W, dtype):
    """gcm_polar_filter (the non-looping K1 of the handle's plan) on the four rows of a 4-row grid (latitudes +-22.5 and
    +-67.5: the multiplier is < 1 in all of them), three levels (one unpaired)"""
    from oracle import lowpass
    H, L = 4, 3
    geom, og = su.geoms_of(H, W, L)
    q = 1e3 * np.random.default_rng(W).standard_normal((L, H, W))
    tol = TOL
    if dtype == "f32":
        q, tol = _f32(q), F32_FILTER
    want = lowpass.arakawa_1977(q, og)
    assert rel_err(q, want) > 1e3 * tol                     # the filter changes the field: skipping it fails
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype=dtype)
    got = c.polar_filter(q)
    c.close()
    e = rel_err(got, want)
    print("filter", dtype, W, "%.2e" % e)
    assert e < tol, (W, dtype, e)


# ---------------------------------------------------------------- C. one model step per plan class
@pytest.mark.parametrize("W", FILTER_WIDTHS)
def test_one_step_fp32_vs_oracle(g, W):
    """one step of an fp32 handle (K1 looping or not, pit, K3, K4 of the width's plan in float) against the float64
    oracle from the same float32-rounded state"""
    H, L = 4, 3
    geom, og = su.geoms_of(H, W, L)
    st = _state(H, W, L, og, 1000 + W, f32=True)
    want = _oracle(st, 1, 60.0, og)
    assert rel_err(want[1], st[1]) > 1e3 * F32_STEP         # the step moves the winds
    _check(_run(g, geom, st, 1, 60.0, "f32"), want, ("fp32 step", W), F32_STEP, F32_PT)


def _tap(c, g):
    L = g._lib
    return {"spu": c.get_intermediate(L.INT_SPU), "pit": c.get_intermediate(L.INT_PIT), "p_n": c.get_intermediate(L.INT_PN),
            "phi": c.get_intermediate(L.INT_PHI), "pgfu": c.get_intermediate(L.INT_PGFU)}


# fp32 intermediates vs the oracle (float32-rounded state): 3x the worst measured of 1440 and 1458 and both stages --
# spu 5.2e-7, pit 4.2e-6 and pgfu 5.2e-5 (differences of nearly equal terms), p_n 3.9e-8, phi 2.3e-7
F32_TAP = {"spu": 1.6e-6, "pit": 1.3e-5, "p_n": 1.2e-7, "phi": 7e-7, "pgfu": 1.6e-4}


@pytest.mark.parametrize("W", [1440, 1458])
def test_hot_path_intermediates_fp32_vs_oracle(g, W):
    """test_hot_path_intermediates_vs_oracle_1440_columns on an fp32 handle: 1440 (the looping K1 with NIN = 10, the
    kMask1440 K3) and 1458 (the four-pass plan in every filter kernel); a failure points at K1, pit or K3"""
    from oracle import dynamics as od
    H, L = 8, 24
    geom, og = su.geoms_of(H, W, L)
    rng = np.random.default_rng(W)
    geom.heightmap[...] = og.heightmap[...] = _f32(30 * rng.random((H, W)))
    base, dt = _state(H, W, L, og, W + 1, f32=True), 30.0
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype="f32")
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
            print("fp32 tap", W, stage, k, "%.2e" % e)
            assert e < F32_TAP[k], (W, stage, k, e)
        stage_state = out
    c.close()


# ---------------------------------------------------------------- D. level counts
LEVELS = [24, 25, 40, 41, 64, L_MAX]
SETTINGS = {"default": {}, "pit3d": {"GCM_PE_PIT2D": "0"}, "segments3": {"GCM_PE_LEVEL_SEGMENTS": "3"}}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("L", LEVELS)
def test_level_counts_vs_oracle(g, L, dtype, monkeypatch):
    """two steps (fp32: one, the step its bounds are for; two measured up to 2.4e-6 in u at 156 levels) at L around the column kernels' forms (pe_geopot_kernel<T, 24 / 40 / 0>: registers up to 40 levels,
    the LDS park above), even L (K4 starts the march on an odd level, oddtop) and odd L, up to the largest L the handle
    accepts; default, pit from the 3-D fields (the geopot launch without column sums), K4 in three level segments"""
    H, W = 5, 30
    geom, og = su.geoms_of(H, W, L)
    f32 = dtype == "f32"
    st = _state(H, W, L, og, L, f32=f32)
    nsteps = 1 if f32 else 2
    want = _oracle(st, nsteps, 60.0, og)
    tol, tol_pt = (F32_STEP, F32_PT) if f32 else (TOL, None)
    for name, env in SETTINGS.items():
        for k in ("GCM_PE_PIT2D", "GCM_PE_LEVEL_SEGMENTS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _check(_run(g, geom, st, nsteps, 60.0, dtype), want, (L, dtype, name), tol, tol_pt)


def _radiation(g, geom, og, st, dtype, seed, utc=4 * 3600.0, dt=300.0):
    """-> (got, want): (dTdt, dt_ground, theta after solar_step, gt after it) of the handle and of oracle.physics"""
    from oracle import physics, temperature as otemp
    L, H, W = st[1].shape
    gt = 270 + 30 * np.random.default_rng(seed).random((H, W))
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype=dtype)
    c.set_state(*st)
    c.set_ground(gt)
    dT, dg = c.grey_radiation(geom, utc)
    c.solar_step(geom, dt, utc)
    got = (dT, dg, c.get_state()[3], c.get_ground())
    c.close()
    p, t = st[0], st[3]
    tp = p * og.sig + og.ptop
    wdT, wdg = physics.basic_grey_radiation(p, tp, otemp.to_true_temp(t, tp), gt, 0.1, 0.9, 0.3, utc, og)
    wt, wg = physics.solar_timestep(t, p, gt, dt, utc, og)
    return got, (wdT, wdg, wt, wg)


def _check_rad(got, want, what, tols):
    for name, x, y, tol in zip(("dTdt", "dt_ground", "t", "gt"), got, want, tols):
        e = rel_err(x, y)
        print("radiation", what, name, "%.2e" % e)
        assert e < tol, (what, name, e)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("L", LEVELS)
def test_level_counts_radiation_vs_oracle(g, L, dtype):
    """grey_radiation and solar_step at the same level counts (pe_radiation_kernel<T, 24 / 40, FACT> and the LDS-parked
    <T, 0> above 40 levels)"""
    H, W = 5, 30
    geom, og = su.geoms_of(H, W, L)
    st = _state(H, W, L, og, 2 * L, f32=dtype == "f32")
    got, want = _radiation(g, geom, og, st, dtype, L)
    _check_rad(got, want, (L, dtype), F32_RAD if dtype == "f32" else (TOL,) * 4)


_GENERIC_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import gcmiipy_amd as g
from gcmiipy_amd import geometry
d = np.load(sys.argv[2])
out = {}
for key in sorted({k.rsplit("_", 1)[0] for k in d.files}):
    L, H, W, ptop = (float(x) for x in key.split("x"))
    L, H, W = int(L), int(H), int(W)
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    geom.ptop = ptop
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom)
    z = np.zeros((L, H, W))
    c.set_state(d[key + "_p"], z, z, d[key + "_t"], z)
    c.set_ground(d[key + "_gt"])
    dT, dg = c.grey_radiation(geom, 4 * 3600.0)
    c.solar_step(geom, 300.0, 4 * 3600.0)
    out[key + "_dT"], out[key + "_dg"], out[key + "_tn"], out[key + "_gn"] = dT, dg, c.get_state()[3], c.get_ground()
    c.close()
np.savez(sys.argv[3], **out)
"""


def test_radiation_generic_form_matches_default(g, tmp_path):
    """GCM_PE_RAD_GENERIC=1 (every L through the LDS-parked pe_radiation_kernel<T, 0> without FACT) against the default
    forms: <T, 24 / 40, FACT> at ptop = 0 -- within 1e-14, the Exner factor is the product (p / P0)^kappa sig^kappa
    there and the direct evaluation here -- and <T, 24 / 40> at ptop != 0: the same arithmetic, bit for bit.  The
    switch is read once per process, so the generic form runs in a child process."""
    cases, ins = [], {}
    for L, ptop in ((9, 0.0), (24, 0.0), (33, 0.0), (9, PTOP), (33, PTOP)):
        H, W = 4, 20
        geom, og = su.geoms_of(H, W, L, ptop)
        p, _, _, t, _ = _state(H, W, L, og, L + int(ptop))
        gt = 270 + 30 * np.random.default_rng(L).random((H, W))
        key = "%dx%dx%dx%g" % (L, H, W, ptop)
        ins.update({key + "_p": p, key + "_t": t, key + "_gt": gt})
        c = g.Core(g._lib.PE25D, W, H, L, geom=geom)
        z = np.zeros((L, H, W))
        c.set_state(p, z, z, t, z)
        c.set_ground(gt)
        dT, dg = c.grey_radiation(geom, 4 * 3600.0)
        c.solar_step(geom, 300.0, 4 * 3600.0)
        cases.append((key, ptop, (dT, dg, c.get_state()[3], c.get_ground())))
        c.close()
    np.savez(tmp_path / "in.npz", **ins)
    env = dict(os.environ, GCM_PE_RAD_GENERIC="1")
    r = subprocess.run([sys.executable, "-c", _GENERIC_CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    d = np.load(tmp_path / "out.npz")
    for key, ptop, got in cases:
        for name, x in zip(("dT", "dg", "tn", "gn"), got):
            y = d[key + "_" + name]
            e = rel_err(y, x)
            print("generic vs default", key, name, "%.2e" % e, "identical" if np.array_equal(x, y) else "")
            if ptop != 0.0:
                assert np.array_equal(x, y), (key, name, e)
            else:
                assert e < 1e-14, (key, name, e)


def test_tracer_equal_to_q_stays_equal_at_64_levels(g):
    """a tracer that starts equal to q stays equal to q bit for bit (the tracer kernel and K4's q update, 64 levels)"""
    H, W, L = 6, 30, 64
    geom, og = su.geoms_of(H, W, L)
    st = _state(H, W, L, og, 64)
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom)
    c.set_state(*st)
    c.set_tracers(st[4][None])
    c.step(2, 60.0)
    q = c.get_state()[4]
    tr = c.get_tracers()
    c.close()
    assert not np.array_equal(q, st[4])
    assert np.array_equal(tr[0], q)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_one_layer_too_many_is_refused(g, dtype):
    """L_MAX + 1 levels: gcm_create refuses the handle and names the limit; nothing is launched"""
    geom, _ = su.geoms_of(4, 20, L_MAX + 1)
    with pytest.raises(ValueError, match="%d layers: the column kernels' LDS holds at most %d" % (L_MAX + 1, L_MAX)):
        g.Core(g._lib.PE25D, 20, 4, L_MAX + 1, geom=geom, dtype=dtype)


# ---------------------------------------------------------------- E. ptop != 0
PTOP_SHAPES = [(12, 20, 5), (6, 1440, 24), (5, 36, 32), (5, 30, 41)]


@pytest.mark.parametrize("hwl", PTOP_SHAPES)
def test_ptop_dynamics_and_radiation_vs_oracle(g, hwl):
    """ptop = 50 hPa enters the geopotential, K3, K4 and the radiation kernels without FACT (<T, 24> for 5 and 24 levels,
    <T, 40> for 32, the LDS-parked <T, 0> for 41): two fp64 steps, grey_radiation + solar_step, one fp32 step"""
    H, W, L = hwl
    geom, og = su.geoms_of(H, W, L, PTOP)
    st = _state(H, W, L, og, H * W + L)
    _check(_run(g, geom, st, 2, 60.0), _oracle(st, 2, 60.0, og), ("ptop", hwl))
    # the ptop terms matter: the same state with ptop = 0 in the oracle is far off
    _, og0 = su.geoms_of(H, W, L)
    assert rel_err(_oracle(st, 1, 60.0, og0)[1], _oracle(st, 1, 60.0, og)[1]) > 1e-6
    for dtype, tols in (("f64", (TOL,) * 4), ("f32", F32_RAD)):
        got, want = _radiation(g, geom, og, _state(H, W, L, og, H * W + L, f32=dtype == "f32"), dtype, H + L)
        _check_rad(got, want, ("ptop", hwl, dtype), tols)
    st32 = _state(H, W, L, og, H * W + L, f32=True)
    _check(_run(g, geom, st32, 1, 60.0, "f32"), _oracle(st32, 1, 60.0, og), ("ptop fp32", hwl), F32_STEP, F32_PT)
