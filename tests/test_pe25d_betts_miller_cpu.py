"""The Betts-Miller convection of GCM_PE25D without a device: the record and its refusals, the host probe
(gcm_betts_miller_columns -- the routines the kernel calls, compiled for the host) against the NumPy restatement
tests/pe25d_betts_miller_ref.py, the conditions of the seeded inputs, the budgets of the probe's output, the checkpoint
keys and the bands' merge.  What needs a handle: tests/test_pe25d_betts_miller_gpu.py.

Bounds.  theta, q and the precipitation go through the Exner routine (5.3e-16 against pow) and some four exp per level,
whose error the ascent carries upwards: 1e-10 relative to the field's maximum, the project's parity bound.  A column's
outcome is a chain of comparisons; one whose margin is under 1e-8 (100 times that bound) may fall either way on another
exp and is kept out of the comparisons of which cells changed -- at most 1 % of the columns of a case, which the seeded
inputs keep (asserted on the restatement alone).  The budgets are sums of L <= 42 terms, each rounded to 1.1e-16,
compared with the column's content: 1e-12."""
import ctypes as C

import numpy as np
import pytest

import gpu_setups as su
import pe25d_betts_miller_ref as ref

DT = 600.0
CASES = [(shape, ptop) for shape in ref.SHAPES for ptop in ref.PTOPS]


def _cols(a):
    """(L, H, W) -> (H, W, L), the probe's layout"""
    return np.ascontiguousarray(np.moveaxis(a, 0, -1))


def _levels(a):
    return np.moveaxis(a, -1, 0)


_cache = {}


def _case(shape, ptop):
    """geometry, state, the restatement's result and the probe's, computed once per case and left unchanged"""
    key = (shape, ptop)
    if key not in _cache:
        import gcmiipy_amd as g
        geom = su.geom_of(*shape, ptop)
        st = ref.convective_state(geom)
        want = ref.betts_miller_step(st[0], st[3], st[4], geom.sig, geom.dsig, ptop, DT, ref.params())
        got = g.betts_miller_columns(st[0], _cols(st[3]), _cols(st[4]), geom.sig, geom.dsig, ptop, DT)
        for a in list(st) + list(want.values()) + list(got.values()):
            a.setflags(write=False)
        _cache[key] = (geom, st, want, got)
    return _cache[key]


def _linf(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ---------------------------------------------------------------- 1: the record, the defaults, the refusals
def test_record_and_defaults():
    import gcmiipy_amd as g
    from gcmiipy_amd.core import BETTS_MILLER_DEFAULTS
    rec = g._lib.BettsMiller
    assert C.sizeof(rec) == 32
    assert [(n, getattr(rec, n).offset) for n, _ in rec._fields_] == [("Lv", 0), ("tau", 8), ("rh_bm", 16), ("nsub", 24)]
    assert dict(BETTS_MILLER_DEFAULTS) == ref.DEFAULTS and list(BETTS_MILLER_DEFAULTS) == list(ref.DEFAULTS)
    assert ref.DEFAULTS == dict(Lv=2.5e6, tau=7200.0, rh_bm=0.7, nsub=2)
    par = g.core.betts_miller_params(dict(tau=3600, nsub=4))
    assert par == ref.params(tau=3600.0, nsub=4) and type(par["nsub"]) is int and type(par["tau"]) is float
    assert g.BettsMiller._fields == ("nsteps", "seconds", "precip", "count")
    rec = g.BettsMiller(4, 2400.0, np.full((2, 3), 1.2), np.full((2, 3), 3.0))
    assert np.array_equal(rec.precip_rate(), np.full((2, 3), 1.2 / 2400.0)) and np.array_equal(rec.frequency(), np.full((2, 3), 0.75))
    with pytest.raises(ValueError):
        g.BettsMiller(0, 0.0, np.zeros((1, 1)), np.zeros((1, 1))).precip_rate()
    with pytest.raises(ValueError):
        g.BettsMiller(0, 0.0, np.zeros((1, 1)), np.zeros((1, 1))).frequency()
    assert g._lib.BETTS_MILLER_MAX_LEVELS == 158


def test_probe_refuses_bad_calls():
    import gcmiipy_amd as g
    lib, L_ = g._lib.lib, g._lib
    nan, inf = float("nan"), float("inf")
    one, col = np.ones(1) * 1e5, np.ones((1, 2))
    sig, dsig = np.array([0.75, 0.25]), np.array([0.5, 0.5])
    for over in (dict(Lv=0.0), dict(Lv=-1.0), dict(Lv=nan), dict(tau=0.0), dict(tau=-1.0), dict(tau=inf), dict(rh_bm=0.0),
                 dict(rh_bm=1.5), dict(rh_bm=nan), dict(nsub=0), dict(nsub=9), dict(nsub=-1)):
        with pytest.raises(ValueError):
            g.betts_miller_columns(one, 300.0 * col, 0.01 * col, sig, dsig, 0.0, DT, **over)
    with pytest.raises(ValueError):
        g.betts_miller_columns(one, col, col, sig, dsig, 0.0, DT, tau_e=1.0)
    with pytest.raises(ValueError):
        g.betts_miller_columns(one, col, col, sig, dsig, 0.0, DT, nsub=1.5)
    for dt, ptop in ((nan, 0.0), (inf, 0.0), (DT, nan)):
        with pytest.raises(ValueError):
            g.betts_miller_columns(one, 300.0 * col, 0.01 * col, sig, dsig, ptop, dt)
    dp = lambda a: a.ctypes.data_as(L_._dp)                                        # noqa: E731
    rec = L_.BettsMiller(*ref.DEFAULTS.values())
    five = [dp(one), dp(col), dp(col), dp(sig), dp(dsig)]
    none = [None] * 6
    assert lib.gcm_betts_miller_columns(1, 2, *five, 0.0, DT, None, *none) == L_.ERR_ARG
    assert lib.gcm_betts_miller_columns(-1, 2, *five, 0.0, DT, rec, *none) == L_.ERR_ARG
    assert lib.gcm_betts_miller_columns(1, 0, *five, 0.0, DT, rec, *none) == L_.ERR_ARG
    assert lib.gcm_betts_miller_columns(1, 2, None, *five[1:], 0.0, DT, rec, *none) == L_.ERR_ARG
    assert lib.gcm_betts_miller_columns(1, 2, *five, 0.0, DT, rec, *none) == L_.OK    # (every output may be NULL)
    assert lib.gcm_betts_miller_columns(0, 2, *none[:5], 0.0, DT, rec, *none) == L_.OK
    # a null handle
    assert lib.gcm_set_betts_miller(None, rec) == L_.ERR_ARG and lib.gcm_betts_miller_on(None) == L_.ERR_ARG
    assert lib.gcm_betts_miller_step(None, DT, rec) == L_.ERR_ARG and lib.gcm_betts_miller_reset(None) == L_.ERR_ARG
    assert lib.gcm_get_betts_miller(None, None, None, None, None) == L_.ERR_ARG
    assert lib.gcm_put_betts_miller(None, None, None, 0.0, 0) == L_.ERR_ARG


# ---------------------------------------------------------------- 3: the inputs are what the tests need them to be
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,ptop", CASES)
def test_inputs_cover_the_five_outcomes(shape, ptop, dtype):
    geom = su.geom_of(*shape, ptop)
    share, margin, res = ref.conditions(geom, dtype, DT)
    low = float(np.mean(margin < ref.MARGIN))
    print("conditions", shape, ptop, dtype, dict(zip(ref.OUTCOMES, share)), "margin min", float(margin.min()), "under the bound", low)
    assert (np.diff(np.asarray(geom.sig).reshape(-1)) < 0).all(), "level 0 is the bottom"
    assert low <= 0.01, low
    if shape == (6, 10, 3):
        assert share[4] > 0 and sum(share[:4]) > 0
        assert set(np.unique(res["kt"][res["deep"]])) <= {1, 2}
    else:
        assert min(share) >= 0.02, share
        # the run of buoyant levels ends below the top in some columns and reaches it in others
        deep = res["deep"]
        assert (res["kt"][deep] < shape[2] - 1).any() and (res["kt"][deep] == shape[2] - 1).any()
    assert res["precip"].max() > 0 and (res["precip"] >= 0).all()


# ---------------------------------------------------------------- 2: the probe against the restatement
@pytest.mark.parametrize("shape,ptop", CASES)
def test_probe_equals_the_restatement(shape, ptop):
    geom, st, want, got = _case(shape, ptop)
    keep = want["margin"] >= ref.MARGIN
    assert np.mean(~keep) <= 0.01
    errs = dict(t=_linf(_levels(got["theta"]), want["t"]), q=_linf(_levels(got["q"]), want["q"]),
                precip=_linf(got["precip"], want["precip"]))
    print("probe", shape, ptop, errs)
    assert max(errs.values()) <= 1e-10, errs
    assert np.array_equal(got["kt"][keep], want["kt"][keep]) and np.array_equal(got["k_lcl"][keep], want["k_lcl"][keep])
    assert got["kt"].dtype == np.int32 and (got["kt"] >= 0).any() and (got["kt"] < 0).any()
    # the same cells changed
    for got_f, want_f, was in ((got["theta"], want["t"], st[3]), (got["q"], want["q"], st[4])):
        a, b = _levels(got_f) != was, want_f != was
        assert np.array_equal(a[:, keep], b[:, keep]) and a.any()
    # the margin is the restatement's, and +infinity where no comparison was consulted
    m = np.isfinite(want["margin"])
    assert np.array_equal(np.isfinite(got["margin"]), m)
    assert np.max(np.abs(got["margin"][m] - want["margin"][m]) / want["margin"][m]) <= 1e-6


def test_probe_on_other_parameters_and_dt_zero():
    import gcmiipy_amd as g
    shape, ptop = ref.SHAPES[0], 1000.0
    geom, st, _, _ = _case(shape, ptop)
    for over in (dict(nsub=1), dict(nsub=8, tau=900.0), dict(rh_bm=0.5, Lv=2.4e6)):
        par = ref.params(**over)
        want = ref.betts_miller_step(st[0], st[3], st[4], geom.sig, geom.dsig, ptop, 1800.0, par)
        got = g.betts_miller_columns(st[0], _cols(st[3]), _cols(st[4]), geom.sig, geom.dsig, ptop, 1800.0, **over)
        keep = want["margin"] >= ref.MARGIN
        assert _linf(_levels(got["theta"]), want["t"]) <= 1e-10 and _linf(_levels(got["q"]), want["q"]) <= 1e-10, over
        assert _linf(got["precip"], want["precip"]) <= 1e-10 and want["deep"].any(), over
        assert np.array_equal(got["kt"][keep], want["kt"][keep]), over
    # dt = 0: r = 0, nothing is relaxed and no column convects
    got = g.betts_miller_columns(st[0], _cols(st[3]), _cols(st[4]), geom.sig, geom.dsig, ptop, 0.0)
    assert np.array_equal(_levels(got["theta"]), st[3]) and np.array_equal(_levels(got["q"]), st[4])
    assert not got["precip"].any() and (got["kt"] == -1).all()
    # a NaN compares false: the column does not convect and keeps its bits
    t = st[3].copy()
    t[2, 0, 0] = np.nan
    got = g.betts_miller_columns(st[0], _cols(t), _cols(st[4]), geom.sig, geom.dsig, ptop, DT)
    assert got["kt"][0, 0] == -1 and got["precip"][0, 0] == 0.0
    assert np.array_equal(got["q"][0, 0], st[4][:, 0, 0])


# ---------------------------------------------------------------- 4: budgets of the probe's output
@pytest.mark.parametrize("shape,ptop", CASES)
def test_budgets_close(shape, ptop):
    geom, st, want, got = _case(shape, ptop)
    p, t, q = st[0], st[3], st[4]
    tn, qn = _levels(got["theta"]), _levels(got["q"])
    before, after = ref.column_water(p, q, geom.dsig), ref.column_water(p, qn, geom.dsig)
    water = float(np.max(np.abs((before - after) - got["precip"]) / before))
    Lv = ref.DEFAULTS["Lv"]
    h0 = ref.column_enthalpy(p, t, q, geom.sig, geom.dsig, ptop, Lv)
    h1 = ref.column_enthalpy(p, tn, qn, geom.sig, geom.dsig, ptop, Lv)
    heat = float(np.max(np.abs(h1 - h0) / h0))
    print("budgets", shape, ptop, water, heat)
    assert water <= 1e-12 and heat <= 1e-12, (water, heat)
    assert (qn >= 0).all()
    still = got["kt"] < 0
    assert still.any() and np.array_equal(tn[:, still], t[:, still]) and np.array_equal(qn[:, still], q[:, still])
    assert not got["precip"][still].any() and (got["precip"][~still] > 0).all()
    # a convecting column is written on levels 0 .. kt and nowhere else
    k = np.arange(shape[2])[:, None, None]
    assert np.array_equal(qn != q, (k <= got["kt"][None]) & ~still[None])


# ---------------------------------------------------------------- 5: the checkpoint keys
class _Recorded:
    """what checkpoint.save asks of a core, and what checkpoint.restore does to one: no library call"""
    options = {}
    tracer_count = 0
    has_ground = False
    held_suarez = None
    climate_every = 0
    moist = convect = boundary_layer = None

    def __init__(self, model, L, H, W, betts_miller=None, sums=None):
        self.model, self.L, self.H, self.W = model, L, H, W
        self.betts_miller, self.sums = betts_miller, sums
        self.state = [np.zeros((H, W))] + [np.zeros((L, H, W)) for _ in range(4)]

    def get_state(self):
        return self.state

    def betts_miller_sums(self):
        return self.sums

    def set_state(self, p=None, u=None, v=None, t=None, q=None):
        self.state = [p, u, v, t, q]

    def set_betts_miller(self, **params):
        self.betts_miller, self.sums = params, None

    def put_betts_miller(self, nsteps, seconds, precip, count):
        import gcmiipy_amd as g
        self.sums = g.BettsMiller(nsteps, seconds, precip, count)


def test_checkpoint_round_trip_of_the_five_keys(tmp_path, monkeypatch):
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    from gcmiipy_amd.core import BETTS_MILLER_DEFAULTS, COLUMN_PHASES, STEP_COLUMN_PHASES
    assert [ph.name for ph in COLUMN_PHASES] == ["boundary_layer", "convect", "moist"]
    assert [ph.name for ph in STEP_COLUMN_PHASES] == ["boundary_layer", "convect", "betts_miller", "moist"], "the model's order"
    L, H, W = 3, 4, 6
    rng = np.random.default_rng(9)
    sums = g.BettsMiller(7, 4200.0, rng.random((H, W)), np.floor(8 * rng.random((H, W))))
    par = ref.params(tau=3600.0, nsub=3)
    path = str(tmp_path / "bm.npz")
    checkpoint.save(path, _Recorded(g._lib.PE25D, L, H, W, betts_miller=par, sums=sums), step=40)
    d = np.load(path)
    keys = {"betts_miller", "betts_miller_n", "betts_miller_seconds", "betts_miller_precip", "betts_miller_count"}
    assert keys <= set(d.files)
    assert list(d["betts_miller"]) == [par[k] for k in BETTS_MILLER_DEFAULTS]
    ck = checkpoint.load(path)
    assert ck["betts_miller"]["params"] == par and type(ck["betts_miller"]["params"]["nsub"]) is int
    assert ck["betts_miller"]["n"] == 7 and ck["betts_miller"]["seconds"] == 4200.0
    assert ck["convect"] is None and ck["moist"] is None and ck["boundary_layer"] is None
    made = []

    def fake_core(model, W_, H_, L_, **kw):
        made.append(_Recorded(model, L_, H_, W_))
        return made[-1]
    monkeypatch.setattr(checkpoint, "Core", fake_core)
    core, _ = checkpoint.restore(path)
    assert core is made[-1] and core.betts_miller == par and (core.sums.nsteps, core.sums.seconds) == (7, 4200.0)
    assert np.array_equal(core.sums.precip, sums.precip) and np.array_equal(core.sums.count, sums.count)
    # a file without the keys restores with none
    checkpoint.save(path, _Recorded(g._lib.PE25D, L, H, W), step=1)
    assert not any(k.startswith("betts_miller") for k in np.load(path).files)
    assert checkpoint.load(path)["betts_miller"] is None
    core, _ = checkpoint.restore(path)
    assert core.betts_miller is None and core.sums is None


# ---------------------------------------------------------------- 6: the bands' merge
def test_merge_concatenates_rows_and_refuses_differing_counters():
    import gcmiipy_amd as g
    from gcmiipy_amd import bands
    rng = np.random.default_rng(5)
    a = g.BettsMiller(3, 360.0, rng.random((2, 5)), rng.random((2, 5)))
    b = g.BettsMiller(3, 360.0, rng.random((3, 5)), rng.random((3, 5)))
    m = bands.merge_betts_miller([a, b])
    assert type(m) is g.BettsMiller and (m.nsteps, m.seconds) == (3, 360.0)
    assert np.array_equal(m.precip, np.concatenate([a.precip, b.precip])) and np.array_equal(m.count, np.concatenate([a.count, b.count]))
    with pytest.raises(ValueError):
        bands.merge_betts_miller([a, b._replace(nsteps=4)])
    with pytest.raises(ValueError):
        bands.merge_betts_miller([a, b._replace(seconds=361.0)])
    with pytest.raises(ValueError):
        bands.merge_betts_miller([])
