"""GPU tests of the energy and STATS record of GCM_PE25D (pe_energy_kernel: gcm_energy / gcm_stats, Core.energy /
Core.stats) against the float64 reference of tests/pe25d_energy_ref.py on what the handle itself returns.

ke, ate and geo: |device - fsum| <= 1e-12 sum |terms| (the terms carry the kernel's table-based exner, which is no
rounding of numpy's pow, so the figure is the one the harness test holds ate and geo to, not a rounding bound); each
case prints its offsets over sum |terms|.  total: ke + ate + geo of the same call, bit for bit.  The extrema: np.max /
np.min of get_state(), gcm_diag's figures and the planted values, exactly.  tests/test_pe25d_energy_ref_cpu.py shows
on the same dense state that a wrong west neighbour, north row or area index moves the sums by 1e-3 .. 1e-6."""
import ctypes as C
import math

import numpy as np
import pytest

import gpu_setups as su
import pe25d_energy_ref as er
import pe25d_inputs as inp
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu
TOL = 1e-12
STEP_SHAPE = (24, 36, 9)        # H, W, L
# (H, W, L), ptop: what each reaches is in test_shapes' docstring
CASES = [((5, 130, 3), 0.0), ((5, 130, 3), 1000.0), ((3, 300, 2), 0.0), ((3, 300, 2), 1000.0), ((4, 64, 41), 0.0),
         ((6, 36, 1), 0.0), ((70, 70, 4), 0.0), ((70, 70, 4), 1000.0), ((1, 260, 5), 0.0)]
U_MAX, U_MIN, V_MAX, V_MIN = 91.0, -92.0, 93.0, -94.0


def _area(shape):
    """a value per column where the reference's broadcast allows one (H == W or H == 1), else one value"""
    H, W, _ = shape
    return er.column_area(W) if H in (1, W) else np.asarray([3.0e9])


def _plant(shape, u, v):
    """four unique extremes by position: the last lane of the tail, the first lane of block 1 (of wave 1, of wave 0),
    cell (0, 0, 0), the last lane of wave 0 (of the tail where W < 64)"""
    H, W, L = shape
    u[L - 1, H - 1, W - 1] = U_MAX
    u[0, 0, 256 if W > 256 else 64 if W > 64 else 0] = U_MIN
    v[0, 0, 0] = V_MAX
    v[L // 2, H - 1, 63 if W >= 64 else W - 1] = V_MIN


def _check_energy(got4, state, geom, area, what):
    """ke, ate, geo of `got4` against the reference on `state`; -> the offsets over sum |terms|"""
    want, s_abs = er.energy(*state[:4], geom, area)
    off = [abs(got4[q] - want[q]) / s_abs[q] for q in range(3)]
    print("%s: ke %.17g ate %.17g geo %.17g; offset / sum|terms|: ke %.3e ate %.3e geo %.3e (tolerance %.0e)"
          % (what, got4[0], got4[1], got4[2], off[0], off[1], off[2], TOL))
    for q, name in enumerate(("ke", "ate", "geo")):
        assert off[q] <= TOL, (what, name, got4[q], want[q])
    assert got4[3] == got4[0] + got4[1] + got4[2], (what, "total")
    return off


def _check_extrema(c, g, s, u, v, what):
    lib = g._lib
    assert s["u_max"] == np.max(u) == c.diag(lib.DIAG_MAX_U), (what, "u_max")
    assert s["u_min"] == np.min(u) == c.diag(lib.DIAG_MIN_U), (what, "u_min")
    assert s["v_max"] == np.max(v) == c.diag(lib.DIAG_MAX_V), (what, "v_max")
    assert s["v_min"] == np.min(v) == c.diag(lib.DIAG_MIN_V), (what, "v_min")


# ---------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("shape,ptop", CASES)
def test_shapes(g, shape, ptop):
    """(5, 130, 3): waves 0 - 2, the third with 2 lanes; the north wrap at j = 0 and the west wrap at i = 0 with dense
    winds.  (3, 300, 2): two workgroups a row, a tail of 44 lanes, the partials' [row][block] index.  (4, 64, 41):
    exactly one full wave, the cumsum over 41 levels.  (6, 36, 1): L = 1.  (70, 70, 4): H == W, an area per column, two
    waves.  (1, 260, 5): H = 1, the north row is the row itself, an area per column over two workgroups.  ptop 1000 on
    the first, second and fifth"""
    H, W, L = shape
    geom = su.geom_of(H, W, L, ptop)
    st = list(er.dense_state(geom))
    _plant(shape, st[1], st[2])
    area = _area(shape)
    c = su.single(g, geom, st, filter=False)
    state = c.get_state()
    for a, b in zip(state, st):
        assert np.array_equal(a, b)                              # (float64 in, float64 out: the reference is exact)
    s = c.stats(area)
    _check_energy(s["ke"], state, geom, area, (shape, ptop))
    assert s["nans"] == 0.0
    _check_extrema(c, g, s, state[1], state[2], (shape, ptop))
    assert (s["u_max"], s["u_min"], s["v_max"], s["v_min"]) == (U_MAX, U_MIN, V_MAX, V_MIN)
    assert c.energy(area) == s["ke"]
    c.close()


# ---------------------------------------------------------------- 2. the state a step leaves
def test_after_an_odd_number_of_steps(g):
    """the dense state with the filter, step(3, 60): the record is that of get_state() -- the read of the current set
    after an odd number of corrector swaps"""
    H, W, L = STEP_SHAPE
    geom = su.geom_of(H, W, L)
    st = er.dense_state(geom)
    c = su.single(g, geom, st)
    area = np.asarray([3.0e9])
    before = c.stats(area)
    c.step(3, 60.0)
    s = c.stats(area)
    state = c.get_state()
    assert not np.array_equal(state[1], st[1]) and np.isfinite(state[1]).all()
    assert s["ke"] != before["ke"] and s["u_max"] != before["u_max"]
    _check_energy(s["ke"], state, geom, area, "after 3 steps")
    assert s["nans"] == 0.0
    _check_extrema(c, g, s, state[1], state[2], "after 3 steps")
    assert c.energy(area) == s["ke"]
    c.close()


def _record(s):
    return np.asarray([s["u_max"], s["u_min"], s["v_max"], s["v_min"], *s["ke"], s["nans"]])


def test_right_behind_the_step(g):
    """3 van Leer tracers and the column physics registered, so that the handle's second stream carries K1, pit and the
    tracer launches while the caller's stream carries K4 and the physics: stats() straight behind step(3) gives the 9
    doubles of a twin that was stepped the same way and waited for the whole device first.  (A single domain's state
    is written on the caller's stream only, which the call follows in stream order: the comment at pe25d_stats.)"""
    import torch
    H, W, L = STEP_SHAPE
    geom = su.geom_of(H, W, L)
    st, trs, gt = er.dense_state(geom), inp.tracers(H, W, L, 3), inp.ground(H, W)
    area = np.asarray([3.0e9])
    c = su.single(g, geom, st, trs, scheme="van_leer", gt=gt, phys=True)
    twin = su.single(g, geom, st, trs, scheme="van_leer", gt=gt, phys=True)
    twin.step(3, 60.0)
    torch.cuda.synchronize()
    want = _record(twin.stats(area))
    c.step(3, 60.0)
    got = _record(c.stats(area))
    assert got.tobytes() == want.tobytes(), (got, want)
    assert np.isfinite(got).all() and got[8] == 0.0
    _check_energy(got[4:8], c.get_state(), geom, area, "behind the step")
    c.close()
    twin.close()


# ---------------------------------------------------------------- 3. NaNs
@pytest.mark.parametrize("field", ["v", "u"])
def test_a_nan_in_one_wind_leaves_the_other_winds_extrema(g, field):
    """the reference's STATS are np.max(u), np.min(u), np.max(v), np.min(v) (oracle/driver.py:77-80): one NaN in v
    makes v_max and v_min NaN and leaves u_max and u_min what NumPy and gcm_diag give; ke and total are NaN, ate and
    geo the clean record's bits, the count is 1.  Then the mirror image with the NaN in u"""
    lib = g._lib
    shape = (5, 130, 3)
    H, W, L = shape
    geom = su.geom_of(H, W, L)
    st = list(er.dense_state(geom))
    _plant(shape, st[1], st[2])
    area = _area(shape)
    c = su.single(g, geom, st, filter=False)
    clean = c.stats(area)
    fi = "puvtq".index(field)
    bad = [a.copy() for a in st]
    bad[fi][1, 2, 70] = np.nan                                   # (wave 1 of the row's workgroup)
    c.set_state(*bad)
    s = c.stats(area)
    hit, other = ("v", "u") if field == "v" else ("u", "v")
    print("NaN in %s: %r" % (field, s))
    assert math.isnan(s[hit + "_max"]) and math.isnan(s[hit + "_min"])
    assert s["nans"] == 1.0
    assert math.isnan(s["ke"][0]) and math.isnan(s["ke"][3])
    assert s["ke"][1] == clean["ke"][1] and s["ke"][2] == clean["ke"][2]
    w = bad[3 - fi]                                              # the other wind
    assert s[other + "_max"] == np.max(w) == clean[other + "_max"]
    assert s[other + "_min"] == np.min(w) == clean[other + "_min"]
    kinds = {"u": (lib.DIAG_MAX_U, lib.DIAG_MIN_U), "v": (lib.DIAG_MAX_V, lib.DIAG_MIN_V)}
    assert s[other + "_max"] == c.diag(kinds[other][0]) and s[other + "_min"] == c.diag(kinds[other][1])
    assert math.isnan(c.diag(kinds[hit][0])) and math.isnan(c.diag(kinds[hit][1]))
    assert c.diag(lib.DIAG_ANY_NAN) == (1.0 if field == "u" else 0.0)        # (the watch looks at u only)
    # a NaN in both winds of one cell is one cell
    bad[3 - fi][1, 2, 70] = np.nan
    c.set_state(*bad)
    s = c.stats(area)
    assert s["nans"] == 1.0 and all(math.isnan(s[k]) for k in ("u_max", "u_min", "v_max", "v_min"))
    c.close()


# ---------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_output_untouched(g):
    from gcmiipy_amd import _lib
    lib = _lib.lib
    H, W, L = 8, 36, 4
    geom = su.geom_of(H, W, L)
    st = er.dense_state(geom)
    out = np.full(9, 7.0)
    po = out.ctypes.data_as(C.POINTER(C.c_double))
    area = np.ones(W)
    pa = area.ctypes.data_as(C.POINTER(C.c_double))

    def refused(c, n, rc, fn=lib.gcm_stats):
        assert fn(c._h, pa, n, po) == rc, (n, rc)
        assert np.all(out == 7.0)

    c32 = su.single(g, geom, st, dtype="f32", filter=False)
    refused(c32, 1, _lib.ERR_UNSUPPORTED)
    refused(c32, 1, _lib.ERR_UNSUPPORTED, lib.gcm_energy)
    assert "fp64" in lib.gcm_last_error(c32._h).decode()
    c32.close()
    band = su.bands(g, geom, 2, st, filter=False)
    refused(band[0], 1, _lib.ERR_UNSUPPORTED)
    assert "single band" in lib.gcm_last_error(band[0]._h).decode()
    for b in band:
        b.close()
    c = su.single(g, geom, st, filter=False)
    for n in (2, H, W - 1, W + 1):                               # neither 1 nor W
        refused(c, n, _lib.ERR_ARG)
        refused(c, n, _lib.ERR_ARG, lib.gcm_energy)
    assert lib.gcm_stats(c._h, pa, W, po) == _lib.OK and np.all(out != 7.0)
    c.close()
    out[:] = 7.0
    sw = g.Core(_lib.SW2D, 130, 16, dx=300e3)
    refused(sw, 1, _lib.ERR_UNSUPPORTED)
    refused(sw, 1, _lib.ERR_UNSUPPORTED, lib.gcm_energy)
    sw.close()
