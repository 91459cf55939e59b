"""pe_radiation_kernel against its NumPy restatement (pe25d_radiation_ref.py) across parameters, clocks and shapes: every
instantiation (<T, 24 | 40, FACT>, <T, 24 | 40>, <T, 0>, double and float) at the smallest shapes that reach it, the
parameter sets and clocks of pe25d_radiation_cases.py, through grey_radiation, solar_step, the registered physics of
step() and a band's own and ghost rows; the rebuild of the level tables when (t_lw, t_sw) change; the refusals.  The
rule (ref.judge): per element, 1e-10 of the level's maximum in fp64, the derived rounding bound in fp32, exact zeros where
the reference is exactly 0.  test_pe25d_radiation_cpu.py admits every case and plants the faults this file would catch."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import gpu_setups as su
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)
import pe25d_radiation_cases as cs
import pe25d_radiation_ref as ref

pytestmark = pytest.mark.gpu
DT = cs.DT


def _handle(g, geom, st, gt, dtype):
    H, W, L = geom.height, geom.width, geom.layers
    # (the zonal filter, which the radiation does not use, needs an even width: the three-block shape has 257 columns)
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype=dtype, filter=W % 2 == 0)
    c.set_state(*st)
    c.set_ground(gt)
    return c


def _one(c, geom, st, gt, pset, utc):
    """grey_radiation, then set_state + set_ground + solar_step -> (dTdt, dt_ground, theta_n, gt_n) of the handle, which
    is left with the inputs again (the diagnostic form reads the state the step before it advanced)"""
    dT, dg = c.grey_radiation(geom, utc, *pset)
    c.set_state(*st)
    c.set_ground(gt)
    c.solar_step(geom, DT, utc, *pset)
    out = dT, dg, c.get_state((3,))[3], c.get_ground()
    c.set_state(*st)
    c.set_ground(gt)
    return out


def _want(shape, ptop, dtype, pset, utc):
    rec, theta_n, gt_n, bnds = cs.reference(shape, ptop, dtype, pset, utc)
    return rec, (rec.dTdt, rec.dt_ground, theta_n, gt_n), bnds


CASES = [(s, p, d) for s in cs.SHAPES for p in cs.PTOPS for d in cs.DTYPES]


@pytest.mark.parametrize("shape,ptop,dtype", CASES, ids=["%dx%dx%d-ptop%g-%s" % (s + (p, d)) for s, p, d in CASES])
def test_parameters_clocks_and_shapes_vs_restatement(g, shape, ptop, dtype):
    """one handle takes every (set, clock): the set changes between consecutive calls and comes back under the next
    clock, so the level tables are rebuilt and uploaded again each time; a kernel that ignored a parameter, a cache that
    kept stale tables, a wrong hour angle, a column read from its neighbour or a scan off by a level misses the rule.
    Over the clocks every column is lit in one call and dark in another.  A fresh handle then gives the first
    combination's bits: nothing a handle has seen before changes what it computes"""
    geom, og, st, gt = cs.case(shape, ptop, dtype)
    c = _handle(g, geom, st, gt, dtype)
    worst, lit, first = {}, [], None
    for pset, utc in cs.combos():
        rec, want, bnds = _want(shape, ptop, dtype, pset, utc)
        got = _one(c, geom, st, gt, pset, utc)
        first = first or got
        lit.append(rec.sza > 0)
        ref.judge(got, want, bnds, (shape, ptop, dtype, pset, utc), dark=cs.dark_mask(rec, pset), out=worst)
    c.close()
    print("SHARE", "%dx%dx%d" % shape, "ptop %g" % ptop, dtype, " ".join("%s %.3g" % kv for kv in worst.items()))
    assert np.all(np.any(lit, axis=0)) and not np.any(np.all(lit, axis=0))
    c = _handle(g, geom, st, gt, dtype)
    again = _one(c, geom, st, gt, *cs.combos()[0])
    c.close()
    for name, x, y in zip(ref.NAMES, again, first):
        assert np.array_equal(x, y), (shape, ptop, dtype, name)


_GENERIC_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import gcmiipy_amd as g
from gcmiipy_amd import geometry
d = np.load(sys.argv[2])
out = {}
for key in sorted({k.rsplit("_", 1)[0] for k in d.files}):
    H, W, L, ptop, dtype = key.split("x")
    H, W, L, ptop = int(H), int(W), int(L), float(ptop)
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    geom.ptop = ptop
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype=dtype)
    z = np.zeros((L, H, W))
    n = 0
    for utc in d[key + "_clocks"]:
        for pset in d[key + "_sets"]:
            c.set_state(d[key + "_p"], z, z, d[key + "_t"], z)
            c.set_ground(d[key + "_gt"])
            dT, dg = c.grey_radiation(geom, utc, *pset)
            c.solar_step(geom, float(d[key + "_dt"]), utc, *pset)
            out["%s_%d_dT" % (key, n)], out["%s_%d_dg" % (key, n)] = dT, dg
            out["%s_%d_tn" % (key, n)], out["%s_%d_gn" % (key, n)] = c.get_state((3,))[3], c.get_ground()
            n += 1
    c.close()
np.savez(sys.argv[3], **out)
"""


def test_generic_form_vs_restatement(g, tmp_path):
    """GCM_PE_RAD_GENERIC=1 (every L through the LDS-parked <T, 0> without FACT) at 5, 25 and 41 levels, both ptop, both
    dtypes, two non-default sets at two clocks, judged against the restatement by the same rule.  The switch is read
    once per process, so the form runs in a fresh child process"""
    ins, keys = {}, []
    for shape in cs.GENERIC_SHAPES:
        for ptop in cs.PTOPS:
            for dtype in cs.DTYPES:
                _, _, st, gt = cs.case(shape, ptop, dtype)
                key = "%dx%dx%dx%gx%s" % (shape + (ptop, dtype))
                keys.append((key, shape, ptop, dtype))
                ins.update({key + "_p": st[0], key + "_t": st[3], key + "_gt": gt, key + "_dt": DT,
                            key + "_sets": np.array(cs.GENERIC_SETS), key + "_clocks": np.array(cs.GENERIC_CLOCKS)})
    np.savez(tmp_path / "in.npz", **ins)
    env = dict(os.environ, GCM_PE_RAD_GENERIC="1")
    r = subprocess.run([sys.executable, "-c", _GENERIC_CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    d = np.load(tmp_path / "out.npz")
    for key, shape, ptop, dtype in keys:
        n, worst = 0, {}
        for utc in cs.GENERIC_CLOCKS:
            for pset in cs.GENERIC_SETS:
                rec, want, bnds = _want(shape, ptop, dtype, pset, utc)
                got = tuple(d["%s_%d_%s" % (key, n, x)] for x in ("dT", "dg", "tn", "gn"))
                ref.judge(got, want, bnds, ("generic", key, pset, utc), dark=cs.dark_mask(rec, pset), out=worst)
                n += 1
        print("SHARE generic", key, " ".join("%s %.3g" % kv for kv in worst.items()))


# ---------------------------------------------------------------- registered physics and bands
PHYS_SHAPE = (12, 36, 9)
SET_A, SET_B = cs.SETS[1], cs.SETS[4]
UTC0, DTS = 3 * 3600.0, 60.0


def _all(c):
    return c.get_state() + [c.get_ground()]


def _same(a, b, what):
    for k, x, y in zip("puvtqg", a, b):
        assert np.array_equal(x, y), (what, k)


def _explicit(g, geom, st, gt, dtype, plan):
    """plan: the set of each step -> step(1) + solar_step at the clock with that set, on a handle without registration"""
    c = _handle(g, geom, st, gt, dtype)
    for n, pset in enumerate(plan):
        c.step(1, DTS)
        c.solar_step(geom, DTS, UTC0 + n * DTS, *pset)
    out = _all(c)
    c.close()
    return out


@pytest.mark.parametrize("dtype", cs.DTYPES)
def test_registered_physics_takes_its_parameters(g, dtype):
    """set_physics with a non-default set, then step(3) = three rounds of step(1) + solar_step(utc0 + n dt, same set) on
    a handle without the registration, bit for bit, and not the default-parameter run; a grey_radiation call with
    another set between two step() calls (which rebuilds the level tables) does not change the registered run; a second
    set_physics with another set takes effect at the next step"""
    geom, og, st, gt = cs.case(PHYS_SHAPE, 0.0, dtype)
    want = _explicit(g, geom, st, gt, dtype, [SET_A] * 3)
    c = _handle(g, geom, st, gt, dtype)
    c.set_physics(geom, UTC0, *SET_A)
    c.step(3, DTS)
    assert c.utc() == UTC0 + 3 * DTS
    _same(_all(c), want, "step(3)")
    c.close()
    default = _explicit(g, geom, st, gt, dtype, [cs.SETS[0]] * 3)
    assert not np.array_equal(default[3], want[3]) and not np.array_equal(default[5], want[5])
    # a diagnostic call with other tables between two steps
    c = _handle(g, geom, st, gt, dtype)
    c.set_physics(geom, UTC0, *SET_A)
    c.step(1, DTS)
    dT, _ = c.grey_radiation(geom, UTC0, *SET_B)
    assert np.all(np.isfinite(dT))
    c.step(2, DTS)
    _same(_all(c), want, "grey_radiation between steps")
    # a second registration: the next step takes it, the clock is the one it states
    c.set_physics(geom, c.utc(), *SET_B)
    c.step(2, DTS)
    _same(_all(c), _explicit(g, geom, st, gt, dtype, [SET_A] * 3 + [SET_B] * 2), "second set_physics")
    c.close()


@pytest.mark.parametrize("dtype", cs.DTYPES)
@pytest.mark.parametrize("nb", [2, 3])
def test_bands_solar_step_own_and_ghost_rows(g, nb, dtype):
    """(12, 36, 9) on 2 and 3 latitude bands with a non-default set: each band's solar_step takes its own rows and its
    ghost rows at the latitude of the GLOBAL row.  The merged theta and ground temperature equal the single domain's
    bit for bit and meet the restatement by the rule; two whole steps (dynamics, exchanges, solar_step) behind it, whose
    predictor reads the ghost rows the bands radiated themselves, stay the single domain's bits"""
    import torch
    pset, utc = SET_A, cs.CLOCKS[2]
    geom, og, st, gt = cs.case(PHYS_SHAPE, 0.0, dtype)
    one = _handle(g, geom, st, gt, dtype)
    one.solar_step(geom, DT, utc, *pset)
    want = _all(one)
    cores = su.bands(g, geom, nb, st, dtype=dtype, gt=gt)
    su.exchange(cores, torch)                       # the ghost rows of the initial state and of gt
    for c in cores:
        c.solar_step(geom, DT, utc, *pset)
    theta = np.concatenate([c.get_state((3,))[3] for c in cores], axis=1)
    ground = np.concatenate([c.get_ground() for c in cores], axis=0)
    assert np.array_equal(theta, want[3]) and np.array_equal(ground, want[5])
    rec, ref_want, bnds = _want(PHYS_SHAPE, 0.0, dtype, pset, utc)
    ref.judge((theta, ground), ref_want[2:], bnds[2:], ("bands", nb, dtype), names=ref.NAMES[2:])
    assert not ref.accepts((st[3], gt), ref_want[2:], bnds[2:])           # (the step moves both)
    for n in range(2):
        one.step(1, DTS)
        one.solar_step(geom, DTS, utc + n * DTS, *pset)
    want = _all(one)
    one.close()

    def solar(n):
        for c in cores:
            c.solar_step(geom, DTS, utc + n * DTS, *pset)      # own rows and ghost rows
    su.whole_steps(cores, torch, 2, DTS, prime=False, after=solar)
    ground = np.concatenate([c.get_ground() for c in cores], axis=0)
    parts = [c.get_state() for c in cores]
    for c in cores:
        c.close()
    state = [np.concatenate([x[f] for x in parts], axis=0 if f == 0 else 1) for f in range(5)]
    _same(state + [ground], want, ("bands", nb, dtype, "two steps"))


# ---------------------------------------------------------------- refusals
BAD = {"t_lw": [0.0, -0.5, 1.5, 1e-300, float("nan"), float("inf")],
       "t_sw": [0.0, 1.0 + 2.0 ** -52, 1e-300, float("nan")],
       "albedo": [-0.1, 1.0 + 2.0 ** -52, float("nan"), float("inf")],
       "utc": [float("nan"), float("inf")],
       "dt": [float("nan"), -float("inf")]}


def test_refused_calls_change_nothing(g):
    """every bad value through grey_radiation, solar_step and set_physics: a ValueError from the Core method and
    GCM_ERR_ARG from the C entry point itself; state, ground temperature, registration and clock are as before, and
    the valid calls that follow give the bits of a handle that never saw a refused one"""
    import ctypes as C
    from gcmiipy_amd import _lib
    lib = _lib.lib
    dtype = "f64"
    geom, og, st, gt = cs.case(PHYS_SHAPE, 0.0, dtype)

    def run(refuse):
        c = _handle(g, geom, st, gt, dtype)
        c.set_physics(geom, UTC0, *SET_A)
        c.step(1, DTS)
        c.grey_radiation(geom, UTC0, *SET_B)             # (the level tables in place are SET_B's)
        before = _all(c)
        if refuse:
            lat, lon = c._latlon(geom)
            dp = C.POINTER(C.c_double)
            tabs = lat.ctypes.data_as(dp), lon.ctypes.data_as(dp)
            for name, values in BAD.items():
                for bad in values:
                    kw = dict(utc=UTC0, t_lw=SET_B[0], t_sw=SET_B[1], albedo=SET_B[2])
                    if name != "dt":
                        kw[name] = bad
                        with pytest.raises(ValueError):
                            c.grey_radiation(geom, **kw)
                        with pytest.raises(ValueError):
                            c.set_physics(geom, **kw)
                        ph = _lib.Physics(kw["utc"], kw["t_lw"], kw["t_sw"], kw["albedo"], *tabs)
                        assert lib.gcm_set_physics(c._h, C.byref(ph)) == _lib.ERR_ARG, (name, bad)
                        assert lib.gcm_grey_radiation(c._h, kw["utc"], kw["t_lw"], kw["t_sw"], kw["albedo"], *tabs,
                                                      None, None) == _lib.ERR_ARG, (name, bad)
                    dt = bad if name == "dt" else DT
                    with pytest.raises(ValueError):
                        c.solar_step(geom, dt, **kw)
                    assert lib.gcm_solar_step(c._h, dt, kw["utc"], kw["t_lw"], kw["t_sw"], kw["albedo"],
                                              *tabs) == _lib.ERR_ARG, (name, bad)
            _same(_all(c), before, "after the refused calls")
            assert c.utc() == UTC0 + DTS
        out = [c.grey_radiation(geom, UTC0, *SET_B)]
        c.step(2, DTS)                                   # (the registration is still SET_A's, the clock went on)
        assert c.utc() == UTC0 + 3 * DTS
        c.solar_step(geom, DT, UTC0, *SET_B)
        out.append(_all(c))
        c.close()
        return out

    (dT_a, dg_a), all_a = run(True)
    (dT_b, dg_b), all_b = run(False)
    assert np.array_equal(dT_a, dT_b) and np.array_equal(dg_a, dg_b)
    _same(all_a, all_b, "after the valid calls")
    # the registered run the refusals left alone is SET_A's
    want = _explicit(g, geom, st, gt, dtype, [SET_A] * 3)
    c = _handle(g, geom, want[:5], want[5], dtype)
    c.solar_step(geom, DT, UTC0, *SET_B)
    _same(all_a, _all(c), "registration kept")
    c.close()
