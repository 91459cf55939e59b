"""Geopotential height on pressure levels and the time-mean maps of GCM_PE25D without a device: the NumPy restatement
tests/pe25d_plev_height_ref.py against the oracle's geopotential, the host build of the column rule
(gcm_plev_height_columns, compiled from the header the kernel compiles from) against the restatement, targets that sit
exactly on levels, the refusals, the C surface, merge_plev_maps and the PlevMaps arithmetic on hand-made sums.

Bounds: the restatement's phi against the oracle's is the same float64 arithmetic in another association (measured
2 - 3e-16 of max |phi| on these shapes); the bound 1e-10 max |phi| is the project's parity figure.  The host build's Z
against the restatement's carries the library's Exner routine against np.power, which that figure bounds."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gpu_setups as su
import pe25d_inputs as inp
import pe25d_plev_height_ref as href
import pe25d_plev_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("gcm_plev_height_columns", "gcm_plev_height", "gcm_set_plev_maps", "gcm_plev_maps_every", "gcm_plev_maps_levels",
                "gcm_plev_maps_sample", "gcm_plev_maps_reset", "gcm_get_plev_maps", "gcm_put_plev_maps", "gcm_plev_maps_plan")
CASES = (((6, 10, 3), 0.0), ((24, 36, 9), 1000.0), ((4, 12, 42), 0.0))        # ((H, W, L), ptop), each with the 1500 m bump
TOL = 1e-10


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


_cases = {}


def case(shape, ptop):
    """(product geometry, oracle geometry, state, levels, heightmap, targets, the restatement's (Z, valid)), once"""
    key = (shape, ptop)
    if key not in _cases:
        H, W, L = shape
        geom, og = su.geoms_of(H, W, L, ptop, bump=True)
        st = pref.with_topography(inp.state_of(geom))
        lev = href.level_arrays(geom)
        hm = np.asarray(geom.heightmap, dtype=np.float64)
        P = pref.targets_for(st[0], lev[0], ptop, 9)
        Z, valid = href.heights(st[0], st[3], *lev, ptop, hm, P)
        _cases[key] = (geom, og, st, lev, hm, P, Z, valid)
    return _cases[key]


def host_build(g, st, lev, ptop, hm, P):
    """gcm_plev_height_columns over the state's columns -> (Z (N, H, W), valid (N, H, W))"""
    Z, valid = g.plev_height_columns(st[0], np.moveaxis(st[3], 0, -1), P, *lev, ptop=ptop, hmG=hm * href.G)
    return np.moveaxis(Z, -1, 0), np.moveaxis(valid, -1, 0)


@pytest.fixture(scope="module")
def g():
    import gcmiipy_amd
    return gcmiipy_amd


# ---------------------------------------------------------------- (a) the restatement against the oracle
@pytest.mark.parametrize("shape,ptop", CASES)
def test_the_restatement_is_the_oracles_geopotential(shape, ptop):
    from oracle import dynamics as odyn
    geom, og, st, lev, hm, P, Z, valid = case(shape, ptop)
    assert hm.max() == 1500.0 and np.count_nonzero(hm) == 1
    want = odyn.compute_geopotential(st[0], st[3], og)
    _, _, _, phi = href.geopotential(st[0], st[3], *lev, ptop, hm)
    err = float(np.max(np.abs(phi - want)) / np.max(np.abs(want)))
    print("largest |phi restatement - phi oracle| / max |phi|", shape, ptop, err)
    assert err <= TOL
    # the inputs exercise the mask: a target valid everywhere, partly masked ones, ones valid nowhere
    pref.assert_masking_is_exercised(st[0], lev[0], ptop, P)
    count = valid.sum(axis=(1, 2))
    assert (count == valid[0].size).any() and ((count > 0) & (count < valid[0].size)).any() and (count == 0).any()
    # Z increases strictly as P falls, wherever two consecutive targets are both valid
    both = valid[:-1] & valid[1:]
    assert both.any() and np.all((Z[1:] - Z[:-1])[both] > 0.0)
    # the bump lifts its own column and no other: phi[0] there carries 1500 m G
    j, i = np.argwhere(hm > 0)[0]
    _, _, _, flat = href.geopotential(st[0], st[3], *lev, ptop, np.zeros_like(hm))
    d = phi - flat
    assert np.allclose(d[:, j, i], 1500.0 * href.G, rtol=1e-12) and np.count_nonzero(d) == phi.shape[0]


# ---------------------------------------------------------------- (b) the host build against the restatement
@pytest.mark.parametrize("shape,ptop", CASES)
def test_the_host_build_equals_the_restatement(g, shape, ptop):
    geom, og, st, lev, hm, P, want, wvalid = case(shape, ptop)
    Z, valid = host_build(g, st, lev, ptop, hm, P)
    assert np.array_equal(valid, wvalid)
    assert np.isnan(Z[~valid]).all() and np.isfinite(Z[valid]).all()
    err = float(np.max(np.abs(Z[valid] - want[valid])) / np.max(np.abs(want[valid])))
    print("largest |Z host build - Z restatement| / max |Z|", shape, ptop, err)
    assert err <= TOL
    # without a heightmap (NULL) the bump's column comes down by exactly what the restatement says, the others stay
    flat, _ = g.plev_height_columns(st[0], np.moveaxis(st[3], 0, -1), P, *lev, ptop=ptop)
    flat = np.moveaxis(flat, -1, 0)
    j, i = np.argwhere(hm > 0)[0]
    other = valid.copy()
    other[:, j, i] = False
    assert same_bits(flat[other], Z[other])
    assert valid[:, j, i].any() and np.allclose((Z - flat)[valid[:, j, i], j, i], 1500.0, rtol=1e-9)


def test_nan_theta_propagates_and_never_decides_validity(g):
    geom, og, st, lev, hm, P, want, wvalid = case(*CASES[0])
    th = st[3].copy()
    th[1, 2, 3] = np.nan
    Z, valid = host_build(g, [st[0], None, None, th], lev, CASES[0][1], hm, P)
    assert np.array_equal(valid, wvalid)
    assert wvalid[:, 2, 3].any() and np.isnan(Z[wvalid[:, 2, 3], 2, 3]).all()
    keep = wvalid.copy()
    keep[:, 2, 3] = False
    assert same_bits(Z[keep], host_build(g, st, lev, CASES[0][1], hm, P)[0][keep])
    # p <= 0 and a NaN p: no valid target
    p = st[0].copy()
    p[0, 0], p[0, 1], p[0, 2] = 0.0, -5.0, np.nan
    _, valid = host_build(g, [p, None, None, st[3]], lev, CASES[0][1], hm, P)
    assert not valid[:, 0, :3].any() and np.array_equal(valid[:, 1:], wvalid[:, 1:])


# ---------------------------------------------------------------- (c) targets exactly on levels
@pytest.mark.parametrize("shape,ptop", CASES)
def test_a_target_on_a_level_returns_that_levels_height(g, shape, ptop):
    """p is the same in every column, so the L level pressures are targets of all of them.  Level k < L - 1 is the bottom
    of bracket k (the difference of the two Pi is 0.0 and Z = phi[k] / G); the top mid-level is reached as the top of
    bracket L - 2 (Z = (phi[L - 2] + stp[L - 2]) / G, the operation that forms phi[L - 1]).  Through the C ABI a level's
    height is visible only as such a Z: it must not depend on which other targets the call carries -- alone, all
    levels at once, or with the neighbouring levels removed so that the march enters the bracket with another target
    pending --, and it must be the restatement's phi[k] / G, which in NumPy is exact on a level as well"""
    H, W, L = shape
    geom, og, st, lev, hm, _, _, _ = case(shape, ptop)
    p = np.full((H, W), 9.3e4)
    pl = lev[0] * 9.3e4 + ptop
    assert np.all(np.diff(pl) < 0)
    all_Z, all_valid = host_build(g, [p, None, None, st[3]], lev, ptop, hm, pl)
    assert all_valid.all()
    _, _, _, phi = href.geopotential(p, st[3], *lev, ptop, hm)
    want, wvalid = href.heights(p, st[3], *lev, ptop, hm, pl)
    assert wvalid.all() and same_bits(want, phi / href.G)
    err = float(np.max(np.abs(all_Z - phi / href.G)) / np.max(np.abs(phi / href.G)))
    print("largest |Z on a level - phi / G| / max", shape, ptop, err)
    assert err <= TOL
    for k in range(L):
        alone, ok = host_build(g, [p, None, None, st[3]], lev, ptop, hm, pl[k:k + 1])
        assert ok.all() and same_bits(alone[0], all_Z[k]), k
    every_other, ok = host_build(g, [p, None, None, st[3]], lev, ptop, hm, pl[::2])
    assert ok.all() and same_bits(every_other, all_Z[::2])
    top_pair, ok = host_build(g, [p, None, None, st[3]], lev, ptop, hm, pl[L - 2:])
    assert ok.all() and same_bits(top_pair, all_Z[L - 2:])
    # a hair inside the brackets next to level k the height is continuous: both sides close in on the level's own
    for k in range(1, L - 1):
        near, ok = host_build(g, [p, None, None, st[3]], lev, ptop, hm, np.array([np.nextafter(pl[k], np.inf), pl[k], np.nextafter(pl[k], 0.0)]))
        assert ok.all() and same_bits(near[1], all_Z[k])
        assert np.all(np.abs(near[0] - near[1]) <= 1e-9 * np.abs(near[1])) and np.all(np.abs(near[2] - near[1]) <= 1e-9 * np.abs(near[1]))


# ---------------------------------------------------------------- (d) refusals and the C surface
def test_refusals(g):
    lib, L_ = g._lib.lib, g._lib
    dp = L_._dp
    ptr = lambda a: a.ctypes.data_as(dp)                        # noqa: E731
    ncol, L, N = 4, 3, 2
    p, th = np.full(ncol, 9e4), np.full((ncol, L), 300.0)
    sig, dsig, sigt = np.array([0.8, 0.5, 0.2]), np.array([0.4, 0.3, 0.3]), np.array([0.6, 0.3, 0.0])
    P = np.array([6e4, 4e4])
    out, valid = np.full((ncol, N), -7.0), np.full((ncol, N), 9, dtype=np.intc)
    iv = valid.ctypes.data_as(C.POINTER(C.c_int))
    def call(**kw):
        """the good call with some arguments replaced"""
        a = dict(ncol=ncol, L=L, N=N, p=ptr(p), th=ptr(th), hm=None, sig=ptr(sig), dsig=ptr(dsig), sigt=ptr(sigt), ptop=0.0,
                 P=ptr(P), out=ptr(out), valid=iv)
        a.update(kw)
        return lib.gcm_plev_height_columns(*a.values())
    for kw in (dict(p=None), dict(th=None), dict(sig=None), dict(dsig=None), dict(sigt=None), dict(out=None), dict(valid=None),
               dict(P=None), dict(L=1), dict(ncol=-1), dict(N=0), dict(N=L_.PLEV_MAX + 1), dict(ptop=np.nan), dict(ptop=np.inf)):
        assert call(**kw) == L_.ERR_ARG, kw
    for B in (np.array([4e4, 6e4]), np.array([6e4, 6e4]), np.array([6e4, -1.0]), np.array([6e4, 0.0]), np.array([np.nan, 1.0]),
              np.array([np.inf, 5e4])):
        assert call(P=ptr(B)) == L_.ERR_ARG, B
        with pytest.raises(ValueError):
            g.plev_height_columns(p, th, B, sig, dsig, sigt)
    assert np.all(out == -7.0) and np.all(valid == 9)           # a refused call changes nothing
    assert call() == L_.OK and np.all(valid == 1) and np.isfinite(out).all()
    assert call(ncol=0) == L_.OK
    with pytest.raises(ValueError):
        g.plev_height_columns(p, th[:, :2], P, sig, dsig, sigt)
    with pytest.raises(ValueError):
        g.plev_height_columns(p[:3], th, P, sig, dsig, sigt)


def test_the_c_surface_is_declared_bound_and_documented():
    import gcmiipy_amd._lib as L_
    header = open(os.path.join(ROOT, "include", "gcmcore.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(L_.lib, name), name
    assert "#define GCM_PLEV_MAP_WORDS %d" % L_.PLEV_MAP_WORDS in header
    assert "#define GCM_PLEV_MAP_WORDS2 %d" % L_.PLEV_MAP_WORDS2 in header
    assert "#define GCM_PLEV_MAP_PLAN_WORDS %d" % L_.PLEV_MAP_PLAN_WORDS in header
    assert "the geopotential height on pressure levels are not offered" not in header
    assert "returns that level's phi / G exactly" in header
    rule = open(os.path.join(ROOT, "gcmiipy_amd", "csrc", "pe25d_plev_height.h")).read()
    assert "returns phi[k] / G exactly" in rule


# ---------------------------------------------------------------- (e) the record and the bands' merge
def hand_made_sums(n, N, H, W, seed=3):
    """sums of n samples of known per-sample values: every word is n times (or count times) a value"""
    rng = np.random.default_rng(seed)
    count = rng.integers(0, n + 1, size=(N, H, W)).astype(np.float64)
    count[0, 0, 0], count[0, 0, 1] = 0.0, float(n)
    vals = rng.random((12, N, H, W)) + 1.0
    s = np.concatenate([count[None], vals * count[None]])
    s2 = np.stack([n * (9e4 + rng.random((H, W))), n * (8.1e9 + rng.random((H, W)))])
    return count, vals, s, s2


def test_from_sums_arithmetic(g):
    n, N, H, W = 8, 2, 3, 5
    count, vals, s, s2 = hand_made_sums(n, N, H, W)
    plev = np.array([8.5e4, 5e4])
    r = g.PlevMaps.from_sums(n, plev, s, s2)
    assert r.n == n and np.array_equal(r.plev, plev) and r._fields[:3] == ("n", "plev", "coverage")
    assert r._fields[3:] == ("Z", "ZZ", "T", "TT", "u", "v", "uu", "vv", "uv", "vT", "q", "vq", "p", "pp")
    assert np.array_equal(r.coverage, count / n) and r.coverage[0, 0, 0] == 0.0 and r.coverage[0, 0, 1] == 1.0
    some = count > 0
    for w, name in enumerate(r._fields[3:15]):
        x = getattr(r, name)
        assert x.shape == (N, H, W) and np.isnan(x[~some]).all() and same_bits(x[some], (s[w + 1] / np.where(some, count, 1.0))[some]), name
    assert same_bits(r.p, s2[0] / n) and same_bits(r.pp, s2[1] / n)
    with np.errstate(invalid="ignore"):
        assert same_bits(r.Z_variance[some], (r.ZZ - r.Z * r.Z)[some]) and same_bits(r.T_variance[some], (r.TT - r.T * r.T)[some])
        assert same_bits(r.eke[some], (0.5 * (r.uu - r.u * r.u + r.vv - r.v * r.v))[some])
        assert same_bits(r.eddy_heat_flux[some], (r.vT - r.v * r.T)[some])
        assert same_bits(r.eddy_moisture_flux[some], (r.vq - r.v * r.q)[some])
    assert same_bits(r.p_variance, r.pp - r.p * r.p)
    # the zonal mean skips the cells without a value; the stationary part sums to zero over them
    zm = r.zonal_mean("Z")
    assert zm.shape == (N, H)
    assert np.isclose(zm[0, 0], np.nanmean(r.Z[0, 0])) and np.allclose(zm, np.nanmean(r.Z, axis=-1))
    st = r.stationary("Z")
    assert st.shape == (N, H, W) and np.isnan(st[~some]).all() and np.allclose(np.nansum(st, axis=-1), 0.0, atol=1e-12)
    assert r.zonal_mean("p").shape == (H,) and np.allclose(r.stationary("p").sum(axis=-1), 0.0, atol=1e-6)
    assert "difference" in g.PlevMaps.__doc__ and "large numbers" in g.PlevMaps.__doc__
    # no sample at all: nothing but NaN and a count of 0
    z = g.PlevMaps.from_sums(0, plev, np.zeros_like(s), np.zeros_like(s2))
    assert z.n == 0 and np.isnan(z.Z).all() and np.isnan(z.p).all()


def test_merge_plev_maps(g):
    from gcmiipy_amd.bands import merge_plev_maps
    n, N, H, W = 4, 2, 6, 5
    _, _, s, s2 = hand_made_sums(n, N, H, W, seed=5)
    plev = np.array([8.5e4, 5e4])
    whole = g.PlevMaps.from_sums(n, plev, s, s2)
    parts = [g.PlevMaps.from_sums(n, plev, s[:, :, a:b], s2[:, a:b]) for a, b in ((0, 2), (2, 3), (3, 6))]
    merged = merge_plev_maps(parts)
    assert merged.n == n
    for f, a, b in zip(whole._fields[1:], merged[1:], whole[1:]):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), f
    with pytest.raises(ValueError):
        merge_plev_maps([])
    with pytest.raises(ValueError):
        merge_plev_maps([parts[0], parts[1]._replace(n=n + 1)])
    with pytest.raises(ValueError):
        merge_plev_maps([parts[0], parts[1]._replace(plev=np.array([8.5e4, 4e4]))])
    with pytest.raises(ValueError):
        merge_plev_maps([parts[0], parts[1]._replace(plev=plev[:1])])


def test_checkpoint_keys_only_with_a_registration(tmp_path):
    """a stand-in core: the keys a file holds with and without the maps registered"""
    from gcmiipy_amd import _lib, checkpoint
    H, W, L, N = 3, 4, 2, 2

    class Stand:
        model, H, W, L = _lib.PE25D, 3, 4, 2
        options, has_ground, tracer_count, held_suarez, climate_every = {}, False, 0, None, 0
        plev_maps_every = 0
        plev_maps_levels = np.array([8e4, 5e4])

        def get_state(self):
            return [np.zeros((H, W))] + [np.zeros((L, H, W))] * 4

        def plev_maps_sums(self):
            return 3, np.ones((13, N, H, W)), np.full((2, H, W), 2.0)

    path = str(tmp_path / "a.npz")
    checkpoint.save(path, Stand())
    plain = set(np.load(path).files)
    assert not any(k.startswith("plev_maps") for k in plain)
    assert checkpoint.load(path)["plev_maps"] is None
    on = Stand()
    on.plev_maps_every = 4
    checkpoint.save(path, on)
    assert set(np.load(path).files) - plain == {"plev_maps_every", "plev_maps_plev", "plev_maps_n", "plev_maps_sums", "plev_maps_sums2"}
    ck = checkpoint.load(path)["plev_maps"]
    assert ck["every"] == 4 and ck["n"] == 3 and np.array_equal(ck["plev"], on.plev_maps_levels)
    assert ck["sums"].shape == (13, N, H, W) and ck["sums2"].shape == (2, H, W)
