"""GCM_PE25D on pressure levels without a device: the host build of the column rule (gcm_plev_columns, compiled from
the header the kernels compile from) against the NumPy restatement tests/pe25d_plev_ref.py bit for bit, its edge cases
and refusals, the C surface, the PlevClimate record, merge_plev_climate and the checkpoint's keys."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pe25d_plev_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("gcm_plev_columns", "gcm_plev_fields", "gcm_set_plev_climate", "gcm_plev_climate_every",
                "gcm_plev_climate_levels", "gcm_plev_climate_sample", "gcm_plev_climate_reset", "gcm_get_plev_climate",
                "gcm_put_plev_climate", "gcm_plev_climate_plan")


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def random_columns(L, ncol, seed, ptop):
    """columns of a sigma model: pl = sig p + ptop with p between 600 and 1030 hPa, and a value per level"""
    rng = np.random.default_rng(seed)
    sig = np.sort(rng.random(L))[::-1] * 0.9 + 0.05
    p = 1e5 * (0.6 + 0.43 * rng.random(ncol)) - ptop
    pl = sig[None, :] * p[:, None] + ptop
    x = 300.0 + 40.0 * rng.standard_normal((ncol, L))
    return sig, p, pl, x


def targets_of(pl):
    """targets below every ground, above every top, between, and exactly on levels of single columns -- pl[0] and
    pl[L - 1] among them"""
    lo, hi = pl.min(), pl.max()
    P = set(np.linspace(0.5 * lo, 1.2 * hi, 11))
    P |= {float(pl[0, 0]), float(pl[1, -1]), float(pl[2, pl.shape[1] // 2]), float(pl[3, 0]), float(pl[3, -1])}
    return np.array(sorted(P, reverse=True))


@pytest.mark.parametrize("ptop", [0.0, 1000.0])
@pytest.mark.parametrize("L", [2, 3, 9])
def test_columns_equal_the_restatement_bit_for_bit(L, ptop):
    import gcmiipy_amd as g
    sig, p, pl, x = random_columns(L, 40, 100 + L, ptop)
    P = targets_of(pl)
    want, wvalid = ref.column_rule(pl.T, x.T, P)                # (the restatement has the level first, the target first)
    got, gvalid = g.plev_columns(pl, x, P)
    assert np.array_equal(gvalid, wvalid.T)
    assert same_bits(got, want.T)
    # the targets cover every case: below the ground, above the top, exactly on a level, at pl[0] and at pl[L - 1]
    assert not gvalid[:, 0].any() and not gvalid[:, -1].any() and gvalid.any(axis=0).sum() >= 6
    n0, nt = list(P).index(pl[0, 0]), list(P).index(pl[1, -1])
    assert gvalid[0, n0] and got[0, n0] == x[0, 0]              # P = pl[0]: the bottom level's value exactly
    assert gvalid[1, nt] and got[1, nt] == x[1, -1]             # P = pl[L - 1]: the top level's value exactly
    nm = list(P).index(pl[2, L // 2])
    assert gvalid[2, nm] and got[2, nm] == x[2, L // 2]
    partly = gvalid.sum(axis=0)
    assert ((partly > 0) & (partly < 40)).any()


@pytest.mark.parametrize("L", [2, 3, 9])
def test_columns_without_a_valid_target_and_nan_values(L):
    """p <= 0 and a NaN p give no valid target, whatever the targets; a NaN value propagates and decides nothing"""
    import gcmiipy_amd as g
    ptop = 1000.0
    sig, p, pl, x = random_columns(L, 8, 7 + L, ptop)
    p[0], p[1], p[2] = 0.0, -5e4, np.nan
    pl = sig[None, :] * p[:, None] + ptop
    x[3, 0], x[4, L - 1], x[0, 0] = np.nan, np.nan, np.nan
    P = np.array(sorted(set(targets_of(pl[3:])) | {ptop, 2 * ptop}, reverse=True))
    want, wvalid = ref.column_rule(pl.T, x.T, P)
    got, gvalid = g.plev_columns(pl, x, P)
    assert np.array_equal(gvalid, wvalid.T) and same_bits(got, want.T)
    assert not gvalid[:3].any() and gvalid[3:].any()
    # the mask of columns 3 and 4 is the one the same columns have without the NaN
    x2 = np.where(np.isnan(x), 1.0, x)
    _, valid2 = g.plev_columns(pl, x2, P)
    assert np.array_equal(gvalid, valid2)
    # NaN where the bracket touches the NaN level (and the weight of the other level is not what hides it), else finite
    assert np.isnan(got[3][gvalid[3] & (P > pl[3, 1])]).all()
    assert np.isnan(got[4][gvalid[4] & (P < pl[4, L - 2])]).all()
    assert np.isfinite(got[5:][gvalid[5:]]).all()


def test_a_profile_linear_in_pressure_is_reproduced():
    """x = a + b pl: the interpolant is x(P) up to the rounding of the weight and of the two products -- a few ulps of
    the larger level value"""
    import gcmiipy_amd as g
    sig, p, pl, _ = random_columns(9, 50, 31, 1000.0)
    a, b = 210.0, 9e-4
    x = a + b * pl
    P = np.linspace(0.5 * pl.min(), 1.1 * pl.max(), 23)[::-1].copy()
    got, valid = g.plev_columns(pl, x, P)
    want = np.broadcast_to(a + b * P, got.shape)
    assert valid.any() and np.all(np.abs(got[valid] - want[valid]) <= 8 * np.spacing(np.abs(x).max()))


def test_out_is_left_alone_where_a_target_is_invalid():
    import gcmiipy_amd as g
    lib, L_ = g._lib.lib, g._lib
    sig, p, pl, x = random_columns(3, 6, 5, 0.0)
    P = targets_of(pl)
    out = np.full((6, P.size), -777.0)
    valid = np.full((6, P.size), -1, dtype=np.intc)
    ip = C.POINTER(C.c_int)
    dp = L_._dp
    rc = lib.gcm_plev_columns(6, 3, P.size, pl.ctypes.data_as(dp), x.ctypes.data_as(dp), P.ctypes.data_as(dp), out.ctypes.data_as(dp),
                              valid.ctypes.data_as(ip))
    assert rc == L_.OK
    assert set(np.unique(valid)) == {0, 1}
    assert np.all(out[valid == 0] == -777.0) and np.all(out[valid == 1] != -777.0)


def test_columns_refuse_bad_arguments():
    import gcmiipy_amd as g
    lib, L_ = g._lib.lib, g._lib
    dp, ip = L_._dp, C.POINTER(C.c_int)
    pl = np.array([[9e4, 5e4, 2e4]])
    x = np.ones((1, 3))
    out, valid = np.full((1, 70), 5.0), np.full((1, 70), 9, dtype=np.intc)

    def call(ncol=1, L=3, P=(8e4, 3e4), pl_=pl, x_=x, out_=out, valid_=valid, N=None, null_P=False):
        P = np.asarray(P, dtype=np.float64)
        ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)      # noqa: E731
        return lib.gcm_plev_columns(ncol, L, P.size if N is None else N, ptr(pl_, dp), ptr(x_, dp), None if null_P else ptr(P, dp),
                                    ptr(out_, dp), ptr(valid_, ip))
    assert call() == L_.OK and valid[0, 0] == 1 and valid[0, 1] == 1
    out[:], valid[:] = 5.0, 9
    for kw in (dict(pl_=None), dict(x_=None), dict(out_=None), dict(valid_=None), dict(null_P=True), dict(L=1), dict(N=0),
               dict(N=-1), dict(P=np.linspace(9e4, 1e4, 65)), dict(P=(3e4, 8e4)), dict(P=(8e4, 8e4)), dict(P=(8e4, 0.0)),
               dict(P=(8e4, -1.0)), dict(P=(np.inf, 8e4)), dict(P=(8e4, np.nan)), dict(P=(np.nan,))):
        assert call(**kw) == L_.ERR_ARG, kw
    assert np.all(out == 5.0) and np.all(valid == 9)             # a refused call writes nothing
    assert call(P=np.linspace(9e4, 1e4, 64)) == L_.OK            # GCM_PLEV_MAX targets are taken
    with pytest.raises(ValueError):
        g.plev_columns(pl, x, [3e4, 8e4])
    with pytest.raises(ValueError):
        g.plev_columns(pl, x[:, :2], [8e4])
    with pytest.raises(ValueError):
        g.plev_columns(pl[:, :1], x[:, :1], [8e4])


def test_header_declares_the_contract():
    text = open(os.path.join(ROOT, "include", "gcmcore.h")).read()
    assert re.search(r"#define\s+GCM_PLEV_WORDS\s+13\b", text) and re.search(r"#define\s+GCM_PLEV_MAX\s+64\b", text)
    assert re.search(r"#define\s+GCM_PLEV_PLAN_WORDS\s+6\b", text)
    assert re.search(r"#define\s+GCM_ABI_VERSION\s+1\b", text)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name


def test_symbols_exist_and_refuse_a_null_handle():
    import gcmiipy_amd as g
    lib, L_ = g._lib.lib, g._lib
    for name in ENTRY_POINTS:
        assert name in L_.SYMBOLS and hasattr(lib, name), name
    assert (L_.PLEV_WORDS, L_.PLEV_MAX, L_.PLEV_PLAN_WORDS) == (len(ref.WORDS), 64, 6)
    dp = L_._dp
    s, n, P = np.zeros(13), C.c_int64(7), np.array([8e4, 5e4])
    plan = (C.c_int * 6)()
    assert lib.gcm_set_plev_climate(None, 1, 2, P.ctypes.data_as(dp)) == L_.ERR_ARG
    assert lib.gcm_plev_climate_every(None) == L_.ERR_ARG and lib.gcm_plev_climate_levels(None, None, 0) == L_.ERR_ARG
    assert lib.gcm_plev_climate_sample(None) == L_.ERR_ARG and lib.gcm_plev_climate_reset(None) == L_.ERR_ARG
    assert lib.gcm_get_plev_climate(None, s.ctypes.data_as(dp), C.byref(n)) == L_.ERR_ARG
    assert lib.gcm_put_plev_climate(None, s.ctypes.data_as(dp), 1) == L_.ERR_ARG
    assert lib.gcm_plev_climate_plan(None, plan, 6) == L_.ERR_ARG
    assert lib.gcm_plev_fields(None, 2, P.ctypes.data_as(dp), 0.0, s.ctypes.data_as(dp), None) == L_.ERR_ARG
    assert n.value == 7 and not s.any()
    from gcmiipy_amd.core import PLEV_WORDS
    assert g.PlevClimate._fields == ("n", "plev", "coverage") + PLEV_WORDS and len(PLEV_WORDS) == 12
    assert "PlevClimate" in g.__all__ and "plev_columns" in g.__all__
    for name in ("set_plev_climate", "plev_climate_every", "plev_climate_levels", "plev_climate_sample", "plev_climate_reset",
                 "plev_climate_sums", "put_plev_climate", "plev_climate_plan", "plev_climate", "plev_fields"):
        assert hasattr(g.Core, name), name


def hand_made_sums(N, H, W, n, seed=2):
    """sums of n samples of rows of W columns with a count of 0 in places"""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((13, N, H)) * 50.0
    s[0] = rng.integers(0, W * n + 1, (N, H)).astype(np.float64)
    s[0, 0, :] = 0.0                                            # a target under every column's ground
    s[0, 1, 0] = W * n
    s[1:, s[0] == 0.0] = 0.0
    return s


def test_plev_climate_record_from_hand_made_sums():
    import gcmiipy_amd as g
    N, H, W, n = 4, 5, 12, 3
    s = hand_made_sums(N, H, W, n)
    plev = np.array([9e4, 7e4, 5e4, 2e4])
    rec = g.PlevClimate.from_sums(n, plev, s, W)
    assert rec.n == n and np.array_equal(rec.plev, plev)
    assert np.array_equal(rec.coverage, s[0] / (np.float64(W) * n)) and rec.coverage[1, 0] == 1.0
    empty = s[0] == 0.0
    assert empty.any() and not empty.all()
    with np.errstate(invalid="ignore", divide="ignore"):
        for w, name in enumerate(("u", "v", "theta", "T", "q", "uu", "vv", "TT", "uv", "vT", "vtheta", "vq")):
            a = getattr(rec, name)
            assert a.shape == (N, H) and np.isnan(a[empty]).all(), name
            assert np.array_equal(a[~empty], (s[w + 1] / s[0])[~empty]), name
    m = ~empty
    assert np.array_equal(rec.eddy_momentum_flux[m], (rec.uv - rec.u * rec.v)[m])
    assert np.array_equal(rec.eddy_heat_flux[m], (rec.vT - rec.v * rec.T)[m])
    assert np.array_equal(rec.eddy_theta_flux[m], (rec.vtheta - rec.v * rec.theta)[m])
    assert np.array_equal(rec.eddy_moisture_flux[m], (rec.vq - rec.v * rec.q)[m])
    assert np.array_equal(rec.T_variance[m], (rec.TT - rec.T * rec.T)[m])
    assert np.array_equal(rec.eke[m], (0.5 * (rec.uu - rec.u * rec.u + rec.vv - rec.v * rec.v))[m])
    assert np.isnan(rec.eke[empty]).all() and np.isnan(rec.eddy_moisture_flux[empty]).all()
    # no samples yet: nothing but NaN, no warning turned error
    zero = g.PlevClimate.from_sums(0, plev, np.zeros((13, N, H)), W)
    assert zero.n == 0 and np.isnan(zero.u).all() and np.isnan(zero.coverage).all()


def test_merge_plev_climate_on_hand_made_parts():
    import gcmiipy_amd as g
    from gcmiipy_amd.bands import merge_plev_climate
    N, H, W, n = 4, 6, 12, 3
    s = hand_made_sums(N, H, W, n, seed=4)
    plev = np.array([9e4, 7e4, 5e4, 2e4])
    whole = g.PlevClimate.from_sums(n, plev, s, W)
    parts = [g.PlevClimate.from_sums(n, plev, s[:, :, sl], W) for sl in (slice(0, 2), slice(2, 3), slice(3, 6))]
    merged = merge_plev_climate(parts)
    assert merged.n == n and np.array_equal(merged.plev, plev)
    for f, a, b in zip(g.PlevClimate._fields[2:], merged[2:], whole[2:]):
        assert a.shape == (N, H) and np.array_equal(a, b, equal_nan=True), f
    with pytest.raises(ValueError):
        merge_plev_climate([parts[0], parts[1]._replace(n=2)])
    with pytest.raises(ValueError):
        merge_plev_climate([parts[0], parts[1]._replace(plev=plev * 2)])
    with pytest.raises(ValueError):
        merge_plev_climate([])


class _Recorded:
    """what checkpoint.save asks of a core, and what checkpoint.restore does to one: no library call"""
    options = {}
    has_ground = False
    tracer_count = 0
    held_suarez = None
    climate_every = 0

    def __init__(self, model, L, H, W, every=0, plev=None, sums=None):
        self.model, self.L, self.H, self.W = model, L, H, W
        self.plev_climate_every, self.plev_climate_levels, self.sums = every, plev, sums
        self.state = [np.zeros((H, W))] + [np.zeros((L, H, W)) for _ in range(4)]

    def get_state(self):
        return self.state

    def plev_climate_sums(self):
        return self.sums

    def set_state(self, p=None, u=None, v=None, t=None, q=None):
        self.state = [p, u, v, t, q]

    def set_plev_climate(self, every, plev):
        self.plev_climate_every, self.plev_climate_levels, self.sums = every, np.asarray(plev), None

    def put_plev_climate(self, n, s):
        self.sums = (n, s)


def test_checkpoint_round_trip_of_the_keys(tmp_path, monkeypatch):
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    L, H, W = 3, 4, 6
    plev = np.array([8.5e4, 5e4, 2.5e4])
    sums = (5, np.random.default_rng(9).standard_normal((13, 3, H)))
    path = str(tmp_path / "plev.npz")
    checkpoint.save(path, _Recorded(g._lib.PE25D, L, H, W, every=8, plev=plev, sums=sums), step=40)
    assert {"plev_climate_every", "plev_climate_plev", "plev_climate_n", "plev_climate_sums"} <= set(np.load(path).files)
    ck = checkpoint.load(path)["plev_climate"]
    assert ck["every"] == 8 and ck["n"] == 5 and np.array_equal(ck["plev"], plev) and np.array_equal(ck["sums"], sums[1])
    made = []

    def fake_core(model, W_, H_, L_, **kw):
        made.append(_Recorded(model, L_, H_, W_))
        return made[-1]
    monkeypatch.setattr(checkpoint, "Core", fake_core)
    core, _ = checkpoint.restore(path)
    assert core is made[-1] and core.plev_climate_every == 8 and np.array_equal(core.plev_climate_levels, plev)
    assert core.sums[0] == 5 and np.array_equal(core.sums[1], sums[1])
    # a file without the keys restores with none
    checkpoint.save(path, _Recorded(g._lib.PE25D, L, H, W), step=1)
    assert not any(k.startswith("plev_climate") for k in np.load(path).files)
    assert checkpoint.load(path)["plev_climate"] is None
    core, _ = checkpoint.restore(path)
    assert core.plev_climate_every == 0 and core.sums is None


def test_run_model_takes_plev_climate():
    import inspect
    from gcmiipy_amd import no_limits_2_5d
    assert inspect.signature(no_limits_2_5d.run_model).parameters["plev_climate"].default is None


def test_restatement_sample_on_a_masked_state():
    """the restatement's own masking inputs do what the GPU tests need of them, and its sums are the plain masked sums
    up to the reordering of W terms"""
    import pe25d_inputs as inp
    import gpu_setups as su
    H, W, L = 6, 70, 2
    for ptop in (0.0, 1000.0):
        geom = su.geom_of(H, W, L, ptop)
        st = ref.with_topography(inp.state_of(geom))
        sig = np.asarray(geom.sig, dtype=np.float64).reshape(-1)
        P = ref.targets_for(st[0], sig, ptop, 7)
        valid = ref.assert_masking_is_exercised(st[0], sig, ptop, P)
        t = ref.terms(*st, sig, ptop, P)
        s = ref.sample(*st, sig, ptop, P)
        assert np.array_equal(s[0], valid.sum(axis=-1).astype(np.float64))
        for w in range(13):
            tol = W * 2.0 ** -52 * np.sum(np.abs(t[w]), axis=-1)
            assert np.all(np.abs(s[w] - np.sum(t[w], axis=-1)) <= tol), w
