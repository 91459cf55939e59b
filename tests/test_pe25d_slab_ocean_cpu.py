"""The slab mixed-layer ocean of GCM_PE25D without a device: the record, the header and the library's exports, the host
probe (gcm_slab_ocean_cells -- the routine the kernel calls, compiled for the host) against the NumPy restatement
tests/pe25d_slab_ocean_ref.py bit for bit, its refusals, the SlabOcean record's means, the bands' merge and the
restatement's own radiation closure.  What needs a handle: tests/test_pe25d_slab_ocean_gpu.py.

Bounds.  The cell rule is six float64 operations that the probe and the restatement round one by one in the same order:
bit for bit.  The closure of the restatement's radiation words is a sum of L + 5 terms, each rounded to 1.1e-16, held to
1e-12 of the sum of their magnitudes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gpu_setups as su
import pe25d_inputs as inp
import pe25d_radiation_ref as rad
import pe25d_slab_ocean_ref as ref

DT = 600.0
HEADER = os.path.join(su.ROOT, "include", "gcmcore.h")
EXPORTS = ("gcm_set_slab_ocean", "gcm_slab_ocean_on", "gcm_slab_ocean_apply", "gcm_get_slab_ocean_fluxes",
           "gcm_get_slab_ocean", "gcm_put_slab_ocean", "gcm_slab_ocean_reset", "gcm_slab_ocean_cells")


def words_of(shape, seed=5):
    """random flux words of plausible size, both signs of the net flux and of the boundary layer's words"""
    rng = np.random.default_rng(seed)
    w = np.empty((ref.NWORDS,) + shape)
    w[ref.SC] = 1360.0 * rng.random(shape)
    w[ref.SW_SFC] = 0.6 * w[ref.SC]
    w[ref.LW_DOWN] = 250.0 + 150.0 * rng.random(shape)
    w[ref.LW_UP] = 300.0 + 400.0 * rng.random(shape)        # (above and below S + B: both signs of R)
    w[ref.OLR] = 150.0 + 150.0 * rng.random(shape)
    w[ref.SH_J] = 6.0e4 * rng.standard_normal(shape)
    w[ref.EVAP_KG] = 0.05 * rng.standard_normal(shape)
    return w


# ---------------------------------------------------------------- 1: the record, the header, the exports
def test_record_defaults_header_and_exports():
    import gcmiipy_amd as g
    from gcmiipy_amd.core import SLAB_OCEAN_DEFAULTS, SLAB_OCEAN_SUMS, SLAB_OCEAN_WORDS
    rec = g._lib.SlabOcean
    assert C.sizeof(rec) == 16
    assert [(n, getattr(rec, n).offset) for n, _ in rec._fields_] == [("heat_capacity", 0), ("Lv", 8)]
    assert dict(SLAB_OCEAN_DEFAULTS) == ref.DEFAULTS == dict(heat_capacity=1.0e7, Lv=2.5e6)
    assert list(SLAB_OCEAN_DEFAULTS) == ["heat_capacity", "Lv"]
    assert SLAB_OCEAN_WORDS == ref.WORDS and len(SLAB_OCEAN_WORDS) == g._lib.SLAB_WORDS == ref.NWORDS
    assert len(SLAB_OCEAN_SUMS) == g._lib.SLAB_SUMS == ref.NSUMS
    assert g.SlabOcean._fields == ("nsteps", "seconds", "sums", "reflect")
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} gcm_slab_ocean;", text).group(1)
    assert re.findall(r"double\s+(\w+);", body) == ["heat_capacity", "Lv"]
    enum = re.search(r"enum \{ GCM_SLAB_SC = 0,[^}]*\}", text).group(0)
    assert [int(x) for x in re.findall(r"= (\d+)", enum)] == list(range(8)) and "GCM_SLAB_WORDS = 7" in enum
    assert re.search(r"enum \{ GCM_SLAB_SUMS = 10 \}", text)
    for name in EXPORTS:
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in g._lib.SYMBOLS and getattr(g._lib.lib, name) is not None, name
    with pytest.raises(ValueError):
        g.core.slab_ocean_params(dict(depth=1.0))


# ---------------------------------------------------------------- 2: the probe against the restatement
@pytest.mark.parametrize("dt", [DT, 0.0, -120.0])
def test_cells_equal_the_restatement_bit_for_bit(dt):
    """scalar capacity, a capacity field with inf cells (which keep their bits), a heat-flux field; dt = 0 and a negative
    dt; both signs of the net flux"""
    import gcmiipy_amd as g
    shape = (7, 33)
    rng = np.random.default_rng(11)
    gt = 288.0 + 15.0 * rng.standard_normal(shape)
    w = words_of(shape)
    R = (w[ref.SW_SFC] + w[ref.LW_DOWN]) - w[ref.LW_UP]
    assert (R < 0).any() and (R > 0).any()
    cap = 10.0 ** rng.uniform(5.0, 8.0, shape)
    cap[rng.random(shape) < 0.25] = np.inf
    assert np.isinf(cap).any() and not np.isinf(cap).all()
    Q = 50.0 * rng.standard_normal(shape)
    for what, kw, C_, Q_, par in (("defaults", {}, 1.0e7, 0.0, {}),
                                  ("thin slab", {}, 1.13e5, 0.0, dict(heat_capacity=1.13e6 * 0.1, Lv=2.4e6)),
                                  ("fields", dict(capacity=cap, qflux=Q), cap, Q, {}),
                                  ("held", {}, np.inf, 0.0, dict(heat_capacity=np.inf))):
        got, e4 = g.slab_ocean_cells(gt, w, dt, **kw, **par)
        want, want_e4 = ref.cells(gt, w, dt, C_, par.get("Lv", 2.5e6), Q_)
        assert np.array_equal(got, want) and np.array_equal(e4, want_e4), (what, dt)
        assert np.isfinite(got).all()
    held = np.isinf(cap)
    got, _ = g.slab_ocean_cells(gt, w, dt, capacity=cap, qflux=Q)
    assert np.array_equal(got[held].view(np.int64), gt[held].view(np.int64)), "an inf cell keeps its bits"
    assert dt == 0.0 or (got[~held] != gt[~held]).any()
    got, e4 = g.slab_ocean_cells(gt, w, dt, heat_capacity=np.inf)
    assert np.array_equal(got.view(np.int64), gt.view(np.int64))
    if dt == 0.0:                                            # no boundary-layer words: every bit stays
        w0 = w.copy()
        w0[ref.SH_J:] = 0.0
        got, e4 = g.slab_ocean_cells(gt, w0, 0.0, qflux=Q)
        assert np.array_equal(got.view(np.int64), gt.view(np.int64)) and not e4.any()


def test_cells_of_no_cells_and_scalars():
    import gcmiipy_amd as g
    got, e4 = g.slab_ocean_cells(np.empty((0,)), np.empty((7, 0)), DT)
    assert got.shape == e4.shape == (0,)
    w = words_of(())
    got, e4 = g.slab_ocean_cells(300.0, w, DT)
    want, want_e4 = ref.cells(300.0, w, DT)
    assert got.shape == () and got == want and e4 == want_e4


# ---------------------------------------------------------------- 3: the refusals
def test_refusals():
    import gcmiipy_amd as g
    lib, rec_t = g._lib.lib, g._lib.SlabOcean
    gt = np.full((2, 3), 290.0)
    w = words_of((2, 3))
    for bad in (dict(heat_capacity=0.0), dict(heat_capacity=-1.0), dict(heat_capacity=np.nan), dict(Lv=0.0), dict(Lv=-2.5e6),
                dict(Lv=np.nan), dict(Lv=np.inf)):
        with pytest.raises(ValueError, match="gcm_slab_ocean_cells"):
            g.slab_ocean_cells(gt, w, DT, **bad)
    for cap in (np.zeros((2, 3)), np.full((2, 3), -5.0), np.where(np.arange(6).reshape(2, 3) == 4, np.nan, 1.0e7)):
        with pytest.raises(ValueError, match="capacity"):
            g.slab_ocean_cells(gt, w, DT, capacity=cap)
    with pytest.raises(ValueError, match="heat-flux"):
        g.slab_ocean_cells(gt, w, DT, qflux=np.full((2, 3), np.inf))
    with pytest.raises(ValueError):
        g.slab_ocean_cells(gt, w, np.nan)
    with pytest.raises(ValueError):
        g.slab_ocean_cells(gt, w[:6], DT)                   # (the wrapper's shape check)
    # the entry point itself: null arrays, n < 0, no parameters
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rec = rec_t(1.0e7, 2.5e6)
    g1, wf, out = np.full(6, 290.0), np.ascontiguousarray(w.reshape(7, 6)), np.full(6, -1.0)
    ARG = g._lib.ERR_ARG
    assert lib.gcm_slab_ocean_cells(6, C.byref(rec), DT, dp(g1), None, dp(wf), None, dp(out), None) == g._lib.OK
    assert np.array_equal(out, ref.cells(g1, wf, DT)[0])
    out[:] = -1.0
    assert lib.gcm_slab_ocean_cells(-1, C.byref(rec), DT, dp(g1), None, dp(wf), None, dp(out), None) == ARG
    assert lib.gcm_slab_ocean_cells(6, None, DT, dp(g1), None, dp(wf), None, dp(out), None) == ARG
    assert lib.gcm_slab_ocean_cells(6, C.byref(rec), DT, None, None, dp(wf), None, dp(out), None) == ARG
    assert lib.gcm_slab_ocean_cells(6, C.byref(rec), DT, dp(g1), None, None, None, dp(out), None) == ARG
    assert lib.gcm_slab_ocean_cells(6, C.byref(rec), DT, dp(g1), None, dp(wf), None, None, None) == ARG
    assert b"gcm_slab_ocean_cells" in lib.gcm_last_error(None)
    assert (out == -1.0).all(), "a refused call writes nothing"
    assert lib.gcm_slab_ocean_cells(0, C.byref(rec), DT, None, None, None, None, None, None) == g._lib.OK
    # a null handle
    assert lib.gcm_set_slab_ocean(None, C.byref(rec), None, None) == ARG
    assert lib.gcm_slab_ocean_on(None) == ARG
    assert lib.gcm_slab_ocean_apply(None, DT, C.byref(rec), dp(wf)) == ARG
    assert lib.gcm_get_slab_ocean_fluxes(None, dp(wf)) == ARG
    assert lib.gcm_get_slab_ocean(None, None, None, None) == ARG
    assert lib.gcm_put_slab_ocean(None, dp(wf), 0.0, 0) == ARG
    assert lib.gcm_slab_ocean_reset(None) == ARG


# ---------------------------------------------------------------- 4: the record's means and the bands' merge
def test_record_means_and_merge():
    import gcmiipy_amd as g
    from gcmiipy_amd.bands import merge_slab_ocean
    shape = (4, 5)
    gt = np.full(shape, 290.0)
    Q = np.full(shape, 12.5)
    sums, sec = None, 0.0
    for n, dt in enumerate((600.0, 300.0)):
        w = words_of(shape, seed=n)
        gt, sums = ref.apply(gt, w, dt, sums, Q=Q)
        sec += dt
    rec = g.SlabOcean(2, sec, sums, 0.3 * 0.9)
    assert np.array_equal(rec.insolation, sums[0] / sec) and np.array_equal(rec.olr, sums[4] / sec)
    assert np.array_equal(rec.asr, rec.insolation - 0.27 * rec.insolation)
    assert np.array_equal(rec.toa_net, rec.asr - rec.olr)
    net = ((rec.sw_surface + rec.lw_down) - rec.lw_up) - rec.shf - rec.lhf + rec.qflux
    assert np.array_equal(rec.surface_net, net) and np.allclose(rec.qflux, 12.5, rtol=1e-15)
    assert np.all(rec.sst_variance >= -1e-9) and np.allclose(rec.sst_mean, sums[8] / sec)
    with pytest.raises(ValueError):
        g.SlabOcean(0, 0.0, 0 * sums, 0.0).olr
    parts = [g.SlabOcean(2, sec, sums[:, :1], 0.27), g.SlabOcean(2, sec, sums[:, 1:], 0.27)]
    whole = merge_slab_ocean(parts)
    assert (whole.nsteps, whole.seconds, whole.reflect) == (2, sec, 0.27) and np.array_equal(whole.sums, sums)
    for other in (g.SlabOcean(3, sec, sums[:, 1:], 0.27), g.SlabOcean(2, sec + 1, sums[:, 1:], 0.27),
                  g.SlabOcean(2, sec, sums[:, 1:], 0.3)):
        with pytest.raises(ValueError):
            merge_slab_ocean([parts[0], other])
    with pytest.raises(ValueError):
        merge_slab_ocean([])


# ---------------------------------------------------------------- 5: the restatement's own closure
@pytest.mark.parametrize("ptop", ref.PTOPS)
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_the_restatements_words_close_the_radiation_budget(shape, ptop):
    """(SC - albedo SC csw_top[0]) - OLR - (S + B - U_s) = sum_k dTdt_k Cp p dsig_k / G with dTdt of the radiation's own
    restatement (oracle.physics bit for bit): what the device is held to with its own dTdt"""
    H, W, L = shape
    geom = su.geom_of(H, W, L, ptop)
    p, _, _, t, _ = inp.state(geom)
    gt = inp.ground(H, W)
    albedo, t_lw, t_sw = 0.3, 0.1, 0.9
    w = ref.radiation_words(p, t, gt, geom, inp.UTC0, t_lw, t_sw, albedo)
    rec = rad.radiation(p, t, gt, geom, inp.UTC0, t_lw, t_sw, albedo)
    csw0 = rad.tables(geom.dsig, geom.sig, t_lw, t_sw)[2].reshape(-1)[0]
    heat, mag = ref.column_heating(rec.dTdt, p, geom)
    lhs = (w[ref.SC] - albedo * w[ref.SC] * csw0) - w[ref.OLR] - ((w[ref.SW_SFC] + w[ref.LW_DOWN]) - w[ref.LW_UP])
    scale = mag + np.abs(w[:5]).sum(axis=0)
    err = float(np.max(np.abs(lhs - heat) / scale))
    print("closure", shape, ptop, err)
    assert (w[ref.SC] > 0).any() and err <= 1e-12, err
