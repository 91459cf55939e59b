"""GPU parity of the diagnostics and the flux_limiter.py drop-in: the total
variation monitor, courant_number, the fused STATS record, van_leer / calc_r / donor-cell pieces
against the golden vectors captured from the reference (g1, g2, g4)."""
import math

import numpy as np
import pytest

from conftest import golden, rel_err
import gpu_setups as su
import pe25d_energy_ref as er
import pe25d_inputs as inp
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu
TOL = 1e-10


def test_flux_limiter_pieces_bit_exact_vs_golden(g):
    """flux_limiter.py:10-32: bit for bit, so the masks (b != 0 in calc_r, strict u > 0 in
    donor_cell_flux) are exactly the reference's; q1[3:6] are equal and u1[7] == 0 in the fixture"""
    from gcmiipy_amd import flux_limiter as fl
    d = golden("g4_tracer")
    q1, u1 = d["q1"], d["u1"]
    r = fl.calc_r(q1)
    assert np.array_equal(r, d["r1"])
    assert np.array_equal(r == 0.0, d["r1"] == 0.0) and (r[3:5] == 0.0).all()
    assert np.array_equal(fl.van_leer(r), d["phi1"])
    pts = np.asarray([fl.van_leer(x) for x in (1, 0, -2.0, 0.5, 1e30)])
    assert np.array_equal(pts, d["phi_pts"])
    assert fl.van_leer(1) == 1 and fl.van_leer(0) == 0           # flux_limiter.py:46-48
    f = fl.donor_cell_flux(q1, u1)
    assert np.array_equal(f, d["donor_flux"])
    assert f[7] == 0.0                                            # u == 0 takes ip(q) * 0
    assert np.array_equal(fl.donor_cell_advection(q1, u1, 100.0, 1.0), d["donor_adv"])
    # 100 donor-cell steps of the reference's own test setup (flux_limiter.py:73-89): conservative, bounded
    q = np.zeros(16); q[4:8] = 1.0
    u = np.full(16, 10.0)
    for _ in range(100):
        q = fl.donor_cell_advection(q, u, 100.0, 1.0)
    assert abs(q.sum() - 4.0) < 1e-12 and q.min() >= 0.0 and q.max() <= 1.0
    with pytest.raises(ValueError):
        fl.calc_r(np.zeros((3, 3)))


def test_total_variation_and_courant_vs_golden(g):
    d1, d2 = golden("g1_shifts"), golden("g2_sw2d")
    a2 = d1["a2"]
    H, W = a2.shape
    c = g.Core(g._lib.SW2D, W, H, dx=300e3)
    c.set_state(p=8000 + a2, u=a2, v=a2)
    assert abs(c.total_variation(g._lib.U) - float(d1["tv"])) < TOL * float(d1["tv"])
    assert abs(c.total_variation(g._lib.P) - float(d1["tv"])) < 1e-9 * float(d1["tv"])
    with pytest.raises(ValueError):
        c.total_variation(g._lib.T)                               # SW2D has no theta
    c.close()
    from gcmiipy_amd.matsuno_c_grid import courant_number
    got = courant_number(8000 + a2, a2, 300e3, 300.0)             # constants.py:111-112
    assert abs(got - float(d1["courant"])) < TOL * float(d1["courant"])
    got = courant_number(d2["p0"], d2["u0"], float(d2["dx"]), float(d2["dt"]))
    assert abs(got - float(d2["courant"])) < TOL * float(d2["courant"])


def test_tv_3d_axis0_is_levels_and_resident_monitor(g):
    """get_total_variation rolls axis 0: the level axis of the reference's [k][j][i] fields"""
    from gcmiipy_amd import geometry
    d = golden("g8_pe25d")
    geom = geometry.gen_geometry(24, 36, 9, sig_func=geometry.manabe_sig)
    ic = [d["dense_%s0" % k] for k in "puvtq"]
    c = g.Core(g._lib.PE25D, 36, 24, 9, geom=geom)
    c.set_state(*ic)
    for f in range(5):
        want = np.sum(np.abs(ic[f] - np.roll(ic[f], -1, 0)))
        assert abs(c.total_variation(f) - want) < TOL * want, f
    c32 = g.Core(g._lib.PE25D, 36, 24, 9, geom=geom, dtype="f32")
    c32.set_state(*ic)
    # the fp32 handle's own state widens exactly: the reference is float64 on what it holds, the bound the summation's
    u32 = c32.get_state()[1]
    assert not np.array_equal(u32, ic[1]) and np.array_equal(u32, ic[1].astype(np.float32))
    terms = np.abs(u32 - np.roll(u32, -1, 0)).ravel()
    want = math.fsum(terms)
    assert abs(c32.total_variation(1) - want) <= er.sum_bound(terms.size, want, 1)
    c32.close()
    c.close()


def test_fused_stats_equals_separate_reductions(g):
    from gcmiipy_amd import geometry
    d = golden("g8_pe25d")
    geom = geometry.gen_geometry(24, 36, 9, sig_func=geometry.manabe_sig)
    ic = [d["dense_%s0" % k] for k in "puvtq"]
    c = g.Core(g._lib.PE25D, 36, 24, 9, geom=geom)
    c.set_state(*ic)
    c.step(2, 30.0)
    area = np.ones(1)
    s = c.stats(area)
    assert s["u_max"] == c.diag(g._lib.DIAG_MAX_U) and s["u_min"] == c.diag(g._lib.DIAG_MIN_U)
    assert s["v_max"] == c.diag(g._lib.DIAG_MAX_V) and s["v_min"] == c.diag(g._lib.DIAG_MIN_V)
    assert s["ke"] == c.energy(area) and s["nans"] == 0.0
    p, u, v, t, q = c.get_state()
    assert s["u_max"] == u.max() and s["v_min"] == v.min()
    u[3, 4, 5] = np.nan
    c.set_state(p, u, v, t, q)
    s = c.stats(area)
    assert s["nans"] >= 1.0 and np.isnan(s["u_max"])
    c.close()


def test_constants_reductions_without_a_handle():
    """constants.get_total_variation / courant_number on plain arrays (gcm_array_stats) vs G1's `tv` /
    `courant`, G2's `courant`, and NumPy on other shapes; the constants themselves vs the oracle's"""
    from gcmiipy_amd import constants as c
    from oracle import constants as oc, grid
    for k in ("Rd", "Cp", "kappa", "P0", "standard_pressure", "standard_temperature", "G", "radius", "mu_air", "Rv"):
        assert getattr(c, k) == getattr(oc, k), k
    d2 = golden("g2_sw2d")
    assert abs(c.courant_number(d2["p0"], d2["u0"], float(d2["dx"]), float(d2["dt"])) / float(d2["courant"]) - 1) < 1e-12
    rng = np.random.default_rng(5)
    for shape in ((11,), (5, 7), (3, 5, 7), (1, 9), (64, 130)):
        q = rng.standard_normal(shape)
        assert abs(c.get_total_variation(q) / grid.get_total_variation(q) - 1) < 1e-12 if q.shape[0] > 1 else c.get_total_variation(q) == 0.0
    d1 = golden("g1_shifts")
    assert abs(c.get_total_variation(d1["a2"]) / float(d1["tv"]) - 1) < 1e-12
    assert abs(c.courant_number(8000 + d1["a2"], d1["a2"], 300e3, 300.0) / float(d1["courant"]) - 1) < 1e-12


def test_courant_number_propagates_nan():
    """np.max(u) is NaN when u holds a NaN (constants.py:111-112): the stability monitor must not hide a
    blown-up field behind fmax"""
    from gcmiipy_amd import constants as c
    rng = np.random.default_rng(6)
    u = rng.standard_normal((33, 70))
    p = 8000 + rng.standard_normal((33, 70))
    assert np.isfinite(c.courant_number(p, u, 300e3, 300.0))
    u[17, 3] = np.nan
    assert np.isnan(c.courant_number(p, u, 300e3, 300.0))
    assert np.isnan(c.get_total_variation(u))


def test_band_total_variation_sums_to_global_and_needs_current_ghosts(g):
    """GCM_DIAG_TV_* on latitude bands: the last row is differenced against the south ghost row, so the
    band partials add up to the single domain's figure once the CURRENT state's ghost rows have been
    exchanged -- and the call refuses (GCM_ERR_STATE) while they are stale, i.e. right after a step"""
    import torch
    from gcmiipy_amd.bands import split_rows
    from test_bands_gpu import _ic2d
    H, W, nb = 37, 130, 3
    f = _ic2d((H, W))
    kw = dict(dx=300e3, tracer=g._lib.TRACER_VANLEER)
    ref = g.Core(g._lib.SW2D_TEMP, W, H, **kw)
    ref.set_state(**f)
    cores = []
    for r, (row0, n) in enumerate(split_rows(H, nb)):
        c = g.Core(g._lib.SW2D_TEMP, W, n, nranks=nb, rank=r, global_height=H, row0=row0, **kw)
        c.set_state(**{k: v[row0:row0 + n] for k, v in f.items()})
        cores.append(c)
    with pytest.raises(g.GcmError):
        cores[0].total_variation(g._lib.P)            # fresh state: ghost rows never filled
    for rnd in range(2):
        su.exchange(cores, torch)
        for fld in (g._lib.P, g._lib.U, g._lib.Q):
            want = ref.total_variation(fld)
            got = sum(c.total_variation(fld) for c in cores)
            assert abs(got / want - 1) < 1e-12, (rnd, fld, got, want)
        ref.step(1, 300.0)
        for c in cores:
            c.step_interior(300.0)
        for c in cores:
            c.step_boundary(300.0)
        with pytest.raises(g.GcmError):
            cores[1].total_variation(g._lib.U)        # stepped: the ghost rows belong to the old state
    ref.close()
    for c in cores:
        c.close()


# ---------------------------------------------------------------- the two reduction kernels against float64 on the handle's own state
# The reference is NumPy float64 on what get_state() returns (it widens exactly, so an fp32 handle has an exact
# reference).  Max, min and ANY_NAN: ==.  SUM_P, MEAN_P and the total variations: |device - fsum| <= (n + 1) 2^-53
# sum |terms| -- any order of n doubles stays inside (n - 1) 2^-53 sum |terms|, and |x - y| is the one rounding inside
# a term; the mean's bound is that over n plus one ulp for the division.
KINDS = ("ANY_NAN", "MAX_U", "MEAN_P", "SUM_P", "MIN_U", "MAX_V", "MIN_V", "TV_P", "TV_U", "TV_V", "TV_T", "TV_Q")
assert len(KINDS) == 12                                          # (ANY_NAN and the eleven figures)


def _diag_reference(kind, st):
    """(value, bound) of the gcm_diag kind named `kind` on the fields st = [p, u, v, t, q] (bound 0: exact)"""
    p, u, v = st[0], st[1], st[2]
    if kind == "ANY_NAN":
        return float(np.isnan(u).any()), 0.0
    if kind in ("MAX_U", "MIN_U", "MAX_V", "MIN_V"):
        return float((np.max if kind[:3] == "MAX" else np.min)(u if kind[-1] == "U" else v)), 0.0
    if kind in ("SUM_P", "MEAN_P"):
        s, bound = math.fsum(p.ravel()), er.sum_bound(p.size, math.fsum(np.abs(p).ravel()), 1)
        return (s, bound) if kind == "SUM_P" else (s / p.size, bound / p.size + np.spacing(abs(s / p.size)))
    x = st["PUVTQ".index(kind[-1])]
    terms = np.abs(x - np.roll(x, -1, 0)).ravel()
    s = math.fsum(terms)
    return s, er.sum_bound(terms.size, s, 1)


def _check_kinds(c, lib, what, skip=()):
    """every kind the model has against the reference on c.get_state(); a kind whose field the model lacks is refused.
    -> {kind: the device's figure}; prints each sum's offset over its bound"""
    st = c.get_state()
    got = {}
    for kind in KINDS:
        if kind in skip:
            continue
        k = getattr(lib, "DIAG_" + kind)
        if kind[:2] == "TV" and st["PUVTQ".index(kind[-1])] is None:
            with pytest.raises(ValueError, match="no such field"):
                c.diag(k)
            continue
        want, bound = _diag_reference(kind, st)
        got[kind] = c.diag(k)
        if bound == 0.0:
            assert np.array_equal(got[kind], want, equal_nan=True), (what, kind, got[kind], want)
        elif math.isnan(want):
            assert math.isnan(got[kind]), (what, kind)
        else:
            off = abs(got[kind] - want)
            print("%s %s: %.17g, offset %.3e, bound %.3e, offset / bound %.3e" % (what, kind, got[kind], off, bound, off / bound))
            assert off <= bound, (what, kind, got[kind], want)
    return got


def _pe_dense(shape):
    H, W, L = shape
    geom = su.geom_of(H, W, L)
    return geom, list(er.dense_state(geom))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_pe25d_second_stride_iteration_and_empty_workgroups(g, dtype):
    """(40, 130, 26): the 3-D fields have 135 200 elements, so lanes 0 .. 4 127 of the 512 x 256 grid take a second
    one; p has 5 200, so workgroups 21 .. 511 have none and write the identity.  The maximum of u is the last element
    of the device layout [j][k][i], the minimum of v the first of row 39: both lie in the second iteration"""
    lib = g._lib
    shape = H, W, L = 40, 130, 26
    geom, st = _pe_dense(shape)
    assert L * H * W == 135200 > (H - 1) * L * W >= 512 * 256 and H * W < 21 * 256
    st[1][L - 1, H - 1, W - 1] = 64.0
    st[2][0, H - 1, 0] = -72.0
    c = su.single(g, geom, st, dtype=dtype, filter=False)
    got = _check_kinds(c, lib, ("pe25d", shape, dtype))
    assert got["MAX_U"] == 64.0 and got["MIN_V"] == -72.0 and got["ANY_NAN"] == 0.0
    # a NaN in theta: its own total variation is NaN, nothing else moves, and the watch (u only) stays off
    bad = [a.copy() for a in st]
    bad[3][L // 2, H - 1, 7] = np.nan
    c.set_state(*bad)
    after = _check_kinds(c, lib, ("pe25d NaN in t", shape, dtype))
    assert math.isnan(after["TV_T"]) and after["ANY_NAN"] == 0.0
    for kind in KINDS:
        if kind != "TV_T":
            assert after[kind] == got[kind], kind
    c.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_pe25d_one_workgroup_with_elements(g, dtype):
    """(3, 10, 2): 60 and 30 elements, only workgroup 0 has any.  u is negative and v positive everywhere, so an
    identity of 0 in the 511 empty workgroups' partials would be the maximum of u and the minimum of v"""
    lib = g._lib
    shape = 3, 10, 2
    geom, st = _pe_dense(shape)
    st[1] = -1.0 - np.abs(st[1])
    st[2] = 1.0 + np.abs(st[2])
    c = su.single(g, geom, st, dtype=dtype, filter=False)
    got = _check_kinds(c, lib, ("pe25d", shape, dtype))
    assert got["MAX_U"] < -1.0 and got["MIN_V"] > 1.0
    c.close()


def _sw_fields(shape, temp):
    rng = np.random.default_rng(17)
    f = dict(p=8000 + 40 * rng.standard_normal(shape), u=5 * rng.standard_normal(shape), v=5 * rng.standard_normal(shape))
    if temp:
        f.update(t=273.16 + 3 * rng.standard_normal(shape), q=rng.random(shape))
    return f


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sw2d_second_stride_iteration(g, dtype):
    """one member of (370, 360): 133 200 elements, lanes 0 .. 2 127 take a second one, on a 2-D handle and on TV_P's
    wrap from the last row to row 0; the model has no theta and no tracer, and says so"""
    lib = g._lib
    H, W = 370, 360
    f = _sw_fields((H, W), False)
    f["u"][H - 1, W - 1] = 40.0                                  # the last element: the second iteration
    f["v"][H - 1, 0] = -41.0
    c = g.Core(lib.SW2D, W, H, dx=300e3, dtype=dtype)
    c.set_state(**f)
    got = _check_kinds(c, lib, ("sw2d", (H, W), dtype))
    assert got["MAX_U"] == 40.0 and got["MIN_V"] == -41.0 and set(got) == set(KINDS) - {"TV_T", "TV_Q"}
    c.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sw2d_temp_nan_in_theta(g, dtype):
    """GCM_SW2D_TEMP with a tracer at (370, 360): all kinds, then a NaN in theta: TV_T is NaN, every other figure keeps
    its bits, GCM_DIAG_ANY_NAN looks at u only (include/gcmcore.h)"""
    lib = g._lib
    H, W = 370, 360
    f = _sw_fields((H, W), True)
    c = g.Core(lib.SW2D_TEMP, W, H, dx=300e3, tracer=lib.TRACER_VANLEER, dtype=dtype)
    c.set_state(**f)
    got = _check_kinds(c, lib, ("sw2d_temp", (H, W), dtype))
    assert set(got) == set(KINDS)
    f["t"][H - 1, W - 2] = np.nan
    c.set_state(**f)
    after = _check_kinds(c, lib, ("sw2d_temp NaN in t", (H, W), dtype))
    assert math.isnan(after["TV_T"]) and after["ANY_NAN"] == 0.0
    for kind in KINDS:
        if kind != "TV_T":
            assert after[kind] == got[kind], kind
    c.close()


@pytest.mark.parametrize("shape", [(520, 130), (70000,), (3, 150, 160)])
def test_array_stats_second_stride_iteration(shape):
    """gcm_array_stats past its 256 x 256 lanes (67 600, 70 000 and 72 000 elements): the total variation against
    oracle.grid.get_total_variation and fsum, the maximum (planted in the last element) against np.max, the mean against
    fsum / n"""
    import ctypes as C
    from gcmiipy_amd import _lib, constants as c
    from oracle import grid
    q = 3.0 * np.random.default_rng(23).standard_normal(shape) - 1.0
    q[(-1,) * len(shape)] = 31.0
    n = q.size
    assert n > 256 * 256
    out = np.full(3, 7.0)
    assert _lib.lib.gcm_array_stats(q.ctypes.data_as(C.c_void_p), q.shape[0], n // q.shape[0], out.ctypes.data_as(C.c_void_p)) == _lib.OK
    terms = np.abs(q - np.roll(q, -1, 0)).ravel()
    tv, b_tv = math.fsum(terms), er.sum_bound(n, math.fsum(terms), 1)
    mean = math.fsum(q.ravel()) / n
    b_mean = er.sum_bound(n, math.fsum(np.abs(q).ravel()), 1) / n + np.spacing(abs(mean))
    print("array_stats %s: tv offset / bound %.3e, mean offset / bound %.3e" % (shape, abs(out[0] - tv) / b_tv, abs(out[2] - mean) / b_mean))
    assert abs(out[0] - tv) <= b_tv
    assert abs(out[0] - grid.get_total_variation(q)) <= b_tv + abs(grid.get_total_variation(q) - tv)
    assert out[1] == np.max(q) == 31.0
    assert abs(out[2] - mean) <= b_mean
    assert c.get_total_variation(q) == out[0]


def test_pe25d_bands_add_up_and_merge(g):
    """3 bands of (24, 36, 9), 2 steps: every kind that reads no ghost row, per band against the band's own state, and
    over the bands against the single domain: the sums add up within the bound of the whole field, the extrema merge
    exactly.  (TV_P of a GCM_PE25D band differences against the south ghost row and is not checked here.)"""
    import torch
    lib = g._lib
    H, W, L = 24, 36, 9
    nb, steps, dt = 3, 2, 120.0
    geom = su.geom_of(H, W, L)
    st = inp.state_of(geom)
    one = su.single(g, geom, st)
    one.step(steps, dt)
    whole = _check_kinds(one, lib, "single domain")
    ref = one.get_state()
    one.close()
    cores = su.bands(g, geom, nb, st)
    su.whole_steps(cores, torch, steps, dt)
    parts = [_check_kinds(c, lib, ("band", r), skip=("TV_P",)) for r, c in enumerate(cores)]
    for c in cores:
        c.close()
    for kind in ("TV_U", "TV_V", "TV_T", "TV_Q", "SUM_P"):
        want, bound = _diag_reference(kind, ref)
        got = sum(p[kind] for p in parts)
        print("bands %s: offset / bound %.3e (the single domain's: %.3e)" % (kind, abs(got - want) / bound, abs(whole[kind] - want) / bound))
        assert abs(got - want) <= bound, kind
    for kind, merge in (("MAX_U", max), ("MIN_U", min), ("MAX_V", max), ("MIN_V", min)):
        assert merge(p[kind] for p in parts) == whole[kind], kind
    assert all(p["ANY_NAN"] == 0.0 for p in parts)
