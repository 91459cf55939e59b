"""The grey radiation without a GPU: the NumPy restatement (pe25d_radiation_ref.py) is oracle.physics bit for bit; every
case the GPU test takes (pe25d_radiation_cases.py) is well enough conditioned to be judged at 1e-10; the comparison rule
rejects every planted fault, and the inputs the suite used before -- the reference's three parameters at one clock --
accept two of them; the host code that turns the parameters into the kernel's level tables
(gcm_grey_radiation_tables) against the restatement; the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import pe25d_radiation_cases as cs
import pe25d_radiation_ref as ref

IDS = ["%dx%dx%d" % s for s in cs.SHAPES]


@pytest.mark.parametrize("shape", cs.SHAPES, ids=IDS)
def test_restatement_is_the_oracle_and_every_case_is_admitted(shape):
    """real = float64: dTdt and dt_ground equal oracle.physics.basic_grey_radiation bit for bit, and at the reference's
    parameters theta_n and gt_n equal oracle.physics.solar_timestep.  Admission, a condition and not a measurement:
    float64 differs from long double by at most 1e-11 of the level's maximum (a tenth of the fp64 bound), for every
    (ptop, dtype, set, clock) of the shape -- none is dropped"""
    from oracle import physics, temperature as otemp
    for ptop in cs.PTOPS:
        for dtype in cs.DTYPES:
            _, og, st, gt = cs.case(shape, ptop, dtype)
            p, t = st[0], st[3]
            tp = p * og.sig + og.ptop
            tt = otemp.to_true_temp(t, tp)
            worst = (0.0, None)
            for pset, utc in cs.combos():
                rec, theta_n, gt_n, _ = cs.reference(shape, ptop, dtype, pset, utc)
                dT, dg = physics.basic_grey_radiation(p, tp, tt, gt, *pset, utc, og)
                assert np.array_equal(dT, rec.dTdt) and np.array_equal(dg, rec.dt_ground), (shape, ptop, dtype, pset, utc)
                if pset == cs.SETS[0]:
                    wt, wg = physics.solar_timestep(t, p, gt, cs.DT, utc, og)
                    assert np.array_equal(wt, theta_n) and np.array_equal(wg, gt_n), (shape, ptop, dtype, utc)
                s = cs.sensitivity(shape, ptop, dtype, pset, utc)
                worst = max(worst, (s, (pset, utc)))
                assert s <= cs.ADMIT, (shape, ptop, dtype, pset, utc, s)
            print("admitted", shape, ptop, dtype, "float64 against long double: worst %.2e at" % worst[0], worst[1])


def test_day_and_night_over_the_clocks():
    """over the clocks every column of every shape is lit in one call and dark in another (the GPU test asserts the same
    from the restatement's sza)"""
    for shape in cs.SHAPES:
        lit = [cs.reference(shape, 0.0, "f64", cs.SETS[0], utc)[0].sza > 0 for utc in cs.CLOCKS]
        assert np.all(np.any(lit, axis=0)) and not np.any(np.all(lit, axis=0)), shape


# ---------------------------------------------------------------- the planted faults
BAND = ((12, 36, 9), 4, 4)          # the band test's shape, and rows [4, 8) of it: the second of three bands
FAULT_SHAPE = (2, 130, 5)


def _fault_verdicts(name):
    """{(set, clock): accepted?} of fault `name` under the fp32 rule, the looser of the two (what it rejects, the fp64
    rule rejects).  tables_stale keeps the tables of the combination before, in the order the handle takes them"""
    out, prev = {}, cs.SETS[0][:2]
    if name == "lat_own_row":
        shape, row0, n = BAND
        _, og, st, gt = cs.case(shape, 0.0, "f64")
        p, t, gt = st[0][row0:row0 + n], st[3][:, row0:row0 + n], gt[row0:row0 + n]
    else:
        shape, row0 = FAULT_SHAPE, 0
        _, og, st, gt = cs.case(shape, 0.0, "f64")
        p, t = st[0], st[3]
    for pset, utc in cs.combos():
        rec = ref.radiation(p, t, gt, og, utc, *pset, row0=row0)
        want = (rec.dTdt, rec.dt_ground) + ref.advance(p, t, gt, rec, cs.DT)
        bnds = ref.bounds(rec, want[2], want[3], cs.DT, True)
        bad = ref.faulty(name, p, t, gt, og, utc, *pset, row0=row0, stale=prev)
        got = (bad.dTdt, bad.dt_ground) + ref.advance(p, t, gt, bad, cs.DT)
        out[(pset, utc)] = ref.accepts(got, want, bnds, cs.dark_mask(rec, pset))
        assert ref.accepts(want, want, bnds, cs.dark_mask(rec, pset))
        prev = pset[:2]
    return out


@pytest.mark.parametrize("name", ref.FAULTS)
def test_every_planted_fault_is_rejected(name):
    """the rule rejects the fault on at least one combination; for the faults the old inputs could not see, the
    combination that accepts them and the one that exposes them are named"""
    v = _fault_verdicts(name)
    rejected = [k for k, ok in v.items() if not ok]
    assert rejected, name
    print("fault", name, "rejected by %d of %d combinations, first" % (len(rejected), len(v)), rejected[0])
    old = (cs.SETS[0], cs.CLOCKS[1])                     # what every test used before: 0.1 / 0.9 / 0.3 at utc = 4 h
    if name in ("albedo_default", "tables_stale"):
        # identical results at the reference's parameters and a single clock: a kernel that ignored albedo, or a cache
        # that kept stale tables, passed
        _, og, st, gt = cs.case(FAULT_SHAPE, 0.0, "f64")
        good = ref.radiation(st[0], st[3], gt, og, old[1], *old[0])
        bad = ref.faulty(name, st[0], st[3], gt, og, old[1], *old[0], stale=old[0][:2])
        assert np.array_equal(good.dTdt, bad.dTdt) and np.array_equal(good.dt_ground, bad.dt_ground)
        assert not v[(cs.SETS[1], cs.CLOCKS[1])]
    if name == "hour_sign":
        assert v[(cs.SETS[0], 0.0)] and not v[old]        # the hour angle is 0 at utc = 0; 4 h exposes the sign
    if name == "no_clamp":
        # a white ground under a transparent short wave takes no sunlight at all: S = 0 and swfac = 0 hide the clamp;
        # the reference's set exposes it in the dark columns of any clock
        assert all(v[(cs.SETS[2], utc)] for utc in cs.CLOCKS) and not any(v[(cs.SETS[0], utc)] for utc in cs.CLOCKS)
    if name == "lon_next":
        assert not any(v[(cs.SETS[0], utc)] for utc in cs.CLOCKS)
    if name == "lat_own_row":
        assert not v[old]                                 # (a band whose row0 is not 0: the band test's case)


def test_fp32_bound_holds_for_float64_arithmetic_on_float32_storage():
    """the derived fp32 bound against what it is derived for: the float64 restatement of the float32-rounded state,
    its results rounded to float32 where the handle stores them so.  Printed beside it: the same with sig and dsig
    rounded to float32 too, which the kernel read from the handle's float32 level tables until it moved to the float64
    level table -- the bound of dt_ground, which has no term for that, is then missed wherever B + S - U_s cancels"""
    for ptop in cs.PTOPS:
        for lev in (None, np.float32):
            worst = dict.fromkeys(ref.NAMES, 0.0)
            for shape in cs.SHAPES[:4]:
                _, og, st, gt = cs.case(shape, ptop, "f32")
                for pset, utc in cs.combos():
                    rec, theta_n, gt_n, bnds = cs.reference(shape, ptop, "f32", pset, utc)
                    e = ref.radiation(st[0], st[3], gt, og, utc, *pset, lev_real=lev)
                    th, g_n = ref.advance(st[0], st[3], gt, e, cs.DT)
                    got = (e.dTdt.astype(np.float32), e.dt_ground.astype(np.float32), th.astype(np.float32), g_n)
                    for name, x, y, b in zip(ref.NAMES, got, (rec.dTdt, rec.dt_ground, theta_n, gt_n), bnds):
                        d = np.abs(x - y)
                        worst[name] = max(worst[name], float(np.max(np.where(d == 0, 0.0, d / np.where(b > 0, b, 1)))))
            print("fp32 emulated, ptop %g, levels %s:" % (ptop, "float64" if lev is None else "float32"),
                  " ".join("%s %.3g" % kv for kv in worst.items()), "(error / bound)")
            if lev is None:
                assert all(s <= 1.0 for s in worst.values()), (ptop, worst)


# ---------------------------------------------------------------- the host's level tables
def _probe(dsig, sig, t_lw, t_sw, nout=None):
    from gcmiipy_amd import _lib
    dsig, sig = np.ascontiguousarray(dsig, dtype=np.float64), np.ascontiguousarray(sig, dtype=np.float64)
    out = np.full(6 * dsig.size, np.nan)
    dp = C.POINTER(C.c_double)
    rc = _lib.lib.gcm_grey_radiation_tables(dsig.size, dsig.ctypes.data_as(dp), sig.ctypes.data_as(dp), t_lw, t_sw,
                                            out.ctypes.data_as(dp), out.size if nout is None else nout)
    return rc, out.reshape(6, -1)


def _ulps(a, b):
    """|a - b| in units of the last place of b (float64)"""
    return np.abs(a - b) / np.spacing(np.abs(b))


@pytest.mark.parametrize("L", [2, 9, 24, 40, 41, 156])
def test_level_tables_of_the_library(L):
    """gcm_grey_radiation_tables returns what pe25d_physics_tables uploads (one builder serves both): the five tables of
    (t_lw, t_sw) equal the restatement's to the last bit or one ulp of pow, the cumulative products built on the
    library's own transmissivities to the bit, and sig^kappa lies within one float64 ulp of the long-double power"""
    from oracle.constants import kappa
    _, og = cs.geoms(2, 20, L, 0.0)
    dsig, sig = og.dsig.reshape(-1), og.sig.reshape(-1)
    names = ("tlw", "tsw", "csw_top", "clw_b_div", "swfac")
    for t_lw, t_sw, _ in cs.SETS:
        rc, got = _probe(dsig, sig, t_lw, t_sw)
        assert rc == 0
        want = ref.tables(dsig, sig, t_lw, t_sw)
        hi = ref.tables(dsig, sig, t_lw, t_sw, real=np.longdouble)
        report = []
        for n, name in enumerate(names):
            u = float(np.max(_ulps(got[n], want[n])))
            report.append("%s %s" % (name, "same bits" if u == 0 else "%.3g ulp" % u))
            # pow of the C library against NumPy's: the last bit or one ulp.  The three tables built on the
            # transmissivities are held to one ulp of the restatement's where the transmissivities have its bits; where a
            # pow differs in its last bit the products carry that on (2 ulp seen in clw_b_div at L = 9, t_lw = 0.1),
            # and they are held to the bit below, on the library's own transmissivities
            if n < 2 or all(np.array_equal(got[m], want[m]) for m in (0, 1)):
                assert u <= 1.0, (L, t_lw, t_sw, name, u)
        # against the long-double tables: 1 - (1 - x) keeps x to an absolute 2^-53, a product of k factors k such
        for n, name in enumerate(names[:2]):
            assert np.max(np.abs(got[n] - hi[n])) <= 2.0 ** -52, (L, t_lw, t_sw, name)
        # the expressions behind the two transmissivities, in the library's own order, on the library's own values
        tlw, tsw = got[0], got[1]
        csw = np.cumprod(tsw[::-1])[::-1]
        assert np.array_equal(got[2], csw) and np.array_equal(got[3], np.cumprod(tlw) / tlw)
        assert np.array_equal(got[4], (1 - tsw) * csw / tsw)
        sk = sig.astype(np.longdouble) ** np.longdouble(kappa)
        us = float(np.max(np.abs(got[5].astype(np.longdouble) - sk) / np.spacing(sk.astype(np.float64))))
        print("tables L %d (%g, %g):" % (L, t_lw, t_sw), ", ".join(report), "; sigk %.3g ulp of long double" % us)
        assert us <= 1.0, (L, us)
    rc, got = _probe(dsig, sig, 1.0, 1.0)
    assert rc == 0 and np.all(got[:4] == 1.0) and np.all(got[4] == 0.0)     # transparent: exactly 1, swfac exactly 0


BAD_T = [0.0, -0.1, 1.0 + 2.0 ** -52, 1.5, 1e-300, float("nan"), float("inf"), -float("inf")]
BAD_ALBEDO = [-2.0 ** -60, 1.0 + 2.0 ** -52, 2.0, float("nan"), float("inf")]
BAD_CLOCK = [float("nan"), float("inf"), -float("inf")]


def test_refusals_without_a_device():
    """t_lw and t_sw outside (0, 1], NaN or inf -- and 1e-300, where a level's transmissivity rounds to 0 and the tables
    would hold 0 / 0 -- are GCM_ERR_ARG from the probe, which then writes nothing; albedo outside [0, 1] and a
    non-finite utc or dt are a ValueError from the check the Core methods run first"""
    from gcmiipy_amd import _lib, core
    _, og = cs.geoms(2, 20, 9, 0.0)
    dsig, sig = og.dsig.reshape(-1), og.sig.reshape(-1)
    for bad in BAD_T:
        for args in ((bad, 0.9), (0.1, bad)):
            rc, out = _probe(dsig, sig, *args)
            assert rc == _lib.ERR_ARG and np.all(np.isnan(out)), (args, rc)
            with pytest.raises(ValueError):
                core.grey_radiation_tables(dsig, sig, *args)
        if bad != 1e-300:                                  # (what depends on the levels is the library's to say)
            with pytest.raises(ValueError, match="t_lw"):
                core.grey_params(bad, 0.9, 0.3)
            with pytest.raises(ValueError, match="t_sw"):
                core.grey_params(0.1, bad, 0.3)
    assert _probe(dsig, sig, 0.1, 0.9, nout=6 * dsig.size - 1)[0] == _lib.ERR_ARG
    assert _probe(dsig, -sig, 0.1, 0.9)[0] == _lib.ERR_ARG and _probe(-dsig, sig, 0.1, 0.9)[0] == _lib.ERR_ARG
    for bad in BAD_ALBEDO:
        with pytest.raises(ValueError, match="albedo"):
            core.grey_params(0.1, 0.9, bad)
    for bad in BAD_CLOCK:
        with pytest.raises(ValueError, match="utc"):
            core.grey_params(0.1, 0.9, 0.3, utc=bad)
        with pytest.raises(ValueError, match="dt"):
            core.grey_params(0.1, 0.9, 0.3, utc=0.0, dt=bad)
    # the edges that are accepted
    assert core.grey_params(1.0, 1.0, 0.0, utc=-1e9, dt=0.0) == (1.0, 1.0, 0.0)
    assert core.grey_params(5e-324, 2.0 ** -1074, 1.0) == (5e-324, 5e-324, 1.0)
    assert _probe(dsig, sig, 1e-12, 1.0)[0] == 0


def test_probe_is_bound():
    from gcmiipy_amd import _lib
    dp = C.POINTER(C.c_double)
    assert _lib.SYMBOLS["gcm_grey_radiation_tables"] == (C.c_int, [C.c_int, dp, dp, C.c_double, C.c_double, dp, C.c_int])
    assert hasattr(_lib.lib, "gcm_grey_radiation_tables")
