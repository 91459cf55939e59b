"""The grey radiation of GCM_PE25D that absorbs by water vapour and CO2, without a device: the record, the header and
the library's exports; the NumPy restatement tests/pe25d_gas_radiation_ref.py against golden g15 (the reference's own
grey_radiation, cases A and B) bit for bit; the host probe (gcm_gas_radiation_columns -- the routine the kernel calls,
compiled for the host) against the restatement within the rule the GPU test applies; the column's closure; the
insolation tables; the refusals; and every planted fault rejected by the rule on the GPU test's own inputs.  What needs a
handle: tests/test_pe25d_gas_radiation_gpu.py.

Bounds.  The restatement repeats the reference's NumPy statements in their order: bit for bit.  The probe differs from it
in 10^x (exp10 against NumPy's power) and tt^4 (two squarings against power), an ulp or two each: it is held to the
parity rule, 1e-10 of the level's or the field's maximum.  The closure is a sum of L + 4 terms of the size of SC, each
rounded to 1.1e-16: 1e-12 SC, the project's closure bound (8e-16 measured).  The daily insolation is seven
libm calls and five operations: 1e-12 relative against long double."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import gpu_setups as su
import pe25d_gas_radiation_ref as ref

HEADER = os.path.join(su.ROOT, "include", "gcmcore.h")
GOLDEN = os.path.join(su.HERE, "golden", "g15_gas_radiation.npz")
EXPORTS = ("gcm_set_gas_radiation", "gcm_gas_radiation_on", "gcm_gas_radiation", "gcm_gas_radiation_step",
           "gcm_gas_radiation_columns", "gcm_gas_insolation")
NAMES = ("dt_ground", "dt_air", "olr")
SHAPE = (6, 72, 12)                                       # (H, W, L): the GPU test's smallest


def golden():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.files}


def golden_case(d, tag):
    par = ref.params(k_h2o_lw=float(d["h2o_weight"]), k_h2o_sw=float(d["h2o_weight"]), k_co2_lw=float(d["co2_weight"]),
                     k_co2_sw=float(d["co2_sw_weight_" + tag]), co2_vmr=float(d["co2_vmr"]),
                     ground_albedo=float(d["ground_albedo"]), solar_constant=float(d["solar_constant"]))
    return par, (d["p"], d["tt"], d["q_" + tag], d["gt"], d["sig"], d["dsig"], float(d["ptop"]))


def probe(SC, p, tt, q, gt, sig, dsig, ptop, par):
    from gcmiipy_amd.core import gas_radiation_columns
    dg, da, olr, w = gas_radiation_columns(SC, p, tt, q, gt, sig, dsig, ptop=ptop, words=True, **par)
    return ref.Gas(dg, da, olr, w[0], w[1], w[2], w[3], w[1] / (1 - par["ground_albedo"]), None, tt, None)


# ---------------------------------------------------------------- 1: the record, the header, the exports
def test_record_defaults_header_and_exports():
    import gcmiipy_amd as g
    from gcmiipy_amd.core import GAS_RADIATION_DEFAULTS
    rec = g._lib.GasRadiation
    names = [n for n, _ in rec._fields_]
    assert names == list(GAS_RADIATION_DEFAULTS) == list(ref.DEFAULTS)
    assert C.sizeof(rec) == 72 and [getattr(rec, n).offset for n in names] == [8 * k for k in range(9)]
    assert dict(GAS_RADIATION_DEFAULTS) == dict(ref.DEFAULTS)
    assert g.GAS_RADIATION_DEFAULTS is GAS_RADIATION_DEFAULTS
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} gcm_gas_radiation_par;", text).group(1)
    assert re.findall(r"(?:double|int32_t)\s+(\w+);", body) == names
    enum = re.search(r"enum \{ GCM_INSOLATION_UNIFORM = 0,[^}]*\}", text).group(0)
    assert {k: int(v) for k, v in re.findall(r"GCM_INSOLATION_(\w+) = (\d+)", enum)} == {k.upper(): v for k, v in g._lib.INSOLATION.items()}
    for name in EXPORTS:
        assert re.search(r"\bint %s\(" % name, text), name
        assert hasattr(g._lib.lib, name), name


# ---------------------------------------------------------------- 2: the restatement is the reference
@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_equals_the_reference_bit_for_bit(tag):
    d = golden()
    par, cols = golden_case(d, tag)
    assert float(d["co2_mmr"]) == par["co2_vmr"] * ref.M_CO2 / ref.Md
    SC = ref.insolation(par, np.zeros(6), np.zeros(8), 0.0, 6)
    assert np.all(SC == float(d["solar_constant"]) * 0.25)
    rec = ref.columns(*cols, SC, par)
    for name, got in zip(NAMES, rec):
        assert np.array_equal(got, d["%s_%s" % (name, tag)]), (tag, name)
    if tag == "b":                                         # short wave reaches the ground, and the two powers differ
        assert rec.swd0.min() > 100.0 and par["k_co2_sw"] != par["k_co2_lw"]


# ---------------------------------------------------------------- 3: the host build of the kernel's routine
def negative_q_state():
    d = golden()
    par, cols = golden_case(d, "b")
    q = cols[2].copy()
    q[np.random.default_rng(3).random(q.shape) < 0.1] *= -50.0
    assert (q < 0).sum() > 20
    return par, cols[:2] + (q,) + cols[3:]


@pytest.mark.parametrize("case", ["a", "b", "negative_q"])
def test_host_build_agrees_with_the_restatement_and_closes(case):
    par, cols = negative_q_state() if case == "negative_q" else golden_case(golden(), case)
    SC = ref.insolation(par, np.zeros(6), np.zeros(8), 0.0, 6)
    want = ref.columns(*cols, SC, par)
    got = probe(SC, *cols, par)
    ref.judge(got[:3] + got[3:7], want[:3] + want[3:7], NAMES + ref.WORDS[:4], case)
    hp = ref.columns(*cols, SC, par, real=np.longdouble)
    ref.judge(got[:3], hp[:3], NAMES, case + " against long double")
    for name, rec in (("restatement", want), ("host build", got._replace(heat=want.heat))):
        miss = np.abs(ref.closure(rec)).max() / SC.max()
        print("closure", case, name, "%.3g of SC" % miss)
        assert miss <= ref.CLOSURE, (case, name, miss)


def test_q_below_zero_counts_as_zero():
    par, cols = negative_q_state()
    SC = np.full(cols[0].shape, 300.0)
    clamped = cols[:2] + (np.maximum(cols[2], 0),) + cols[3:]
    for got, want in zip(probe(SC, *cols, par)[:7], probe(SC, *clamped, par)[:7]):
        assert np.array_equal(got, want)


# ---------------------------------------------------------------- 4: the insolation
def test_uniform_insolation_is_a_quarter_of_the_solar_constant():
    from gcmiipy_amd.core import GAS_RADIATION_DEFAULTS, gas_insolation
    lat = np.linspace(-math.pi / 2, math.pi / 2, 9)
    S0 = GAS_RADIATION_DEFAULTS["solar_constant"]
    assert S0 == 2 * 41840 * 60.0 ** -1
    assert np.all(gas_insolation(lat) == S0 / 4)
    assert np.all(gas_insolation(lat, "uniform", 0.3, 1000.0) == 250.0)


@pytest.mark.parametrize("decl", [0.0, 0.4, -0.4, 0.1])
def test_daily_insolation_against_long_double(decl):
    from gcmiipy_amd.core import gas_insolation
    lat = np.concatenate([np.linspace(-math.pi / 2, math.pi / 2, 37), [1.2, -1.2, 0.013]])
    got = gas_insolation(lat, "daily", decl, 1360.0)
    par = ref.params(insolation="daily", declination=decl, solar_constant=1360.0)
    want = ref.insolation(par, lat, np.zeros(1), 0.0, lat.size, real=np.longdouble)[:, 0].astype(np.float64)
    assert np.isfinite(got).all() and (got >= 0).all()
    rel = np.abs(got - want) / np.where(want == 0, 1.0, np.abs(want))
    print("daily insolation, declination", decl, "worst relative error %.3g" % rel.max())
    assert rel.max() <= 1e-12
    if decl != 0:
        night = np.sign(lat) == -np.sign(decl)
        night &= np.abs(lat) > math.pi / 2 - abs(decl) + 1e-9
        assert night.sum() >= 2 and np.all(got[night] == 0)                      # polar night: exactly 0
        day = (np.sign(lat) == np.sign(decl)) & (np.abs(lat) > math.pi / 2 - abs(decl) + 1e-9)
        assert day.sum() >= 2 and np.all(got[day] > 0)                           # polar day: finite, the sun never sets
        # (the reference's own formula, arccos unclamped, has no value there)
        with np.errstate(invalid="ignore"):
            assert np.isnan(np.arccos(-np.tan(lat[night]) * np.tan(decl))).all()


def test_zenith_has_no_row_table():
    from gcmiipy_amd.core import gas_insolation
    with pytest.raises(ValueError):
        gas_insolation(np.zeros(3), "zenith")


# ---------------------------------------------------------------- 5: the refusals
REFUSED = [dict(k_h2o_lw=-1.0), dict(k_co2_lw=math.nan), dict(k_h2o_sw=math.inf), dict(k_co2_sw=-1e-300), dict(co2_vmr=-1e-6),
           dict(co2_vmr=math.nan), dict(solar_constant=-1.0), dict(solar_constant=math.inf), dict(ground_albedo=1.0),
           dict(ground_albedo=-0.01), dict(ground_albedo=math.nan), dict(declination=math.pi / 2 + 1e-9),
           dict(declination=-2.0), dict(declination=math.nan)]


@pytest.mark.parametrize("bad", REFUSED, ids=lambda b: "%s=%r" % next(iter(b.items())))
def test_refused_parameters_change_nothing(bad):
    """by the library itself (the record goes to gcm_gas_radiation_columns as it is) and by the Python layer"""
    import gcmiipy_amd as g
    from gcmiipy_amd.core import gas_radiation_columns, gas_radiation_params
    par, (p, tt, q, gt, sig, dsig, ptop) = golden_case(golden(), "a")
    with pytest.raises(ValueError):
        gas_radiation_params(bad)
    with pytest.raises(ValueError):
        gas_radiation_columns(300.0, p, tt, q, gt, sig, dsig, **bad)
    vals = dict(par, **bad)
    rec = g._lib.GasRadiation(*[g._lib.INSOLATION[v] if k == "insolation" else v for k, v in vals.items()])
    n, L = p.size, sig.size
    flat = [np.ascontiguousarray(a.reshape(-1)) for a in (np.full(p.shape, 300.0), p, sig, dsig, tt, q, gt)]
    outs = [np.full(n, -7.0), np.full(L * n, -7.0), np.full(n, -7.0), np.full(5 * n, -7.0)]
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = g._lib.lib.gcm_gas_radiation_columns(n, L, C.byref(rec), ptr(flat[0]), ptr(flat[1]), ptop, ptr(flat[2]), ptr(flat[3]),
                                              ptr(flat[4]), ptr(flat[5]), ptr(flat[6]), *[ptr(o) for o in outs])
    assert rc == g._lib.ERR_ARG
    assert all(np.all(o == -7.0) for o in outs)


def test_unknown_insolation_and_names_are_refused():
    import gcmiipy_amd as g
    from gcmiipy_amd.core import gas_insolation, gas_radiation_params
    with pytest.raises(ValueError):
        gas_radiation_params(dict(insolation="seasonal"))
    with pytest.raises(ValueError):
        gas_radiation_params(dict(k_o3=1.0))
    with pytest.raises(ValueError):
        gas_radiation_params({}, utc=math.nan)
    with pytest.raises(ValueError):
        gas_radiation_params({}, dt=math.inf)
    lat, out = np.zeros(4), np.full(4, -7.0)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for kind, decl, S0 in ((7, 0.0, 1.0), (-1, 0.0, 1.0), (1, 0.0, 1.0), (2, 2.0, 1.0), (2, 0.0, -1.0), (0, 0.0, math.nan)):
        assert g._lib.lib.gcm_gas_insolation(kind, 4, ptr(lat), decl, S0, ptr(out)) == g._lib.ERR_ARG, (kind, decl, S0)
        assert np.all(out == -7.0)
    rec = g._lib.GasRadiation(*[7 if k == "insolation" else v for k, v in ref.DEFAULTS.items()])
    one = np.ones(1)
    assert g._lib.lib.gcm_gas_radiation_columns(1, 1, C.byref(rec), *[ptr(one)] * 2, 0.0, *[ptr(one)] * 5,
                                                ptr(out), None, None, None) == g._lib.ERR_ARG
    with pytest.raises(ValueError):
        gas_insolation(lat, "daily", declination=2.0)


def test_drop_in_refuses_clouds():
    from gcmiipy_amd import grey_solar
    with pytest.raises(ValueError):
        grey_solar.grey_radiation(None, None, None, 0.5, None, 0.0, 900.0, None)


# ---------------------------------------------------------------- 6: the rule rejects every planted fault
def band_of(st, gt, row0, n):
    return [np.ascontiguousarray(a[..., row0:row0 + n, :]) for a in st], gt[row0:row0 + n]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("fault", ref.FAULTS)
def test_the_rule_rejects_every_planted_fault(fault, dtype):
    """on the GPU test's own inputs: the smallest shape, the case the fault must show on, the second band's rows for the
    latitude's row; the fp32 handle's wider rule for dt_air and theta rejects them too.  The restatement itself passes"""
    H, W, L = SHAPE
    geom = su.geoms_of(8 if fault == "lat_own_row" else H, W, L)[1]
    st, gt = ref.state(geom, dtype)
    row0 = 0
    if fault == "lat_own_row":
        row0 = 4
        st, gt = band_of(st, gt, 4, 4)
    assert fault != "q_no_clamp" or (st[4] < 0).sum() > 100
    par = ref.params(**ref.CASES[ref.FAULT_CASE.get(fault, "defaults")])
    f32 = dtype == "f32"
    want = ref.radiation(st[0], st[3], st[4], gt, geom, ref.UTC, par, row0=row0)
    bad = ref.radiation(st[0], st[3], st[4], gt, geom, ref.UTC, par, row0=row0, fault=fault)
    hp = ref.radiation(st[0], st[3], st[4], gt, geom, ref.UTC, par, real=np.longdouble, row0=row0)
    pick = lambda r: (r.dt_ground, r.dt_air, r.olr, r.SC, r.sw_sfc, r.lw_down, r.lw_up) + ref.advance(gt, r, 600.0)
    flags = (False, f32, False, False, False, False, False, f32, False)
    assert ref.accepts(pick(hp), pick(want), flags)
    assert not ref.accepts(pick(bad), pick(want), flags), fault
    # the diagnostic form's three results alone (what the first GPU case reads) reject it too
    assert not ref.accepts(pick(bad)[:3], pick(want)[:3], flags[:3]), fault
