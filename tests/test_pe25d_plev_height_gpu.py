"""Geopotential height on pressure levels and the time-mean maps of GCM_PE25D on the device (gcm_plev_height,
gcm_set_plev_maps) against the NumPy restatement tests/pe25d_plev_height_ref.py: the map call on states whose surface
pressure is scaled per column to stand in for topography, with the 1500 m bump in the heightmap; the device's own
geopotential; the registered phase against explicit samples; latitude bands (in-process bands with device-copied ghost
rows and the loopback band of gcm_band_run, on the second stream and on the comm stream); reset / put / get /
checkpoint; a handle without a registration; the refusals.

Bounds.  The mask, the count, uc, vc, q, their products and p carry no Exner routine: bit for bit the restatement's.  Z
and T carry the library's Exner routine where the restatement takes np.power: Z within 1e-10 max |Z|, the project's
parity figure for that routine, and the words that hold Z or T within 1e-10 sum |term|, the same figure carried through
a sum.  The device against itself -- the sample against the map calls, a band against the single domain, the device
against the host build -- is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import gpu_setups as su
import pe25d_inputs as inp
import pe25d_plev_height_ref as href
import pe25d_plev_ref as pref
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

# (H, W, L): the third spans two 256-column chunks; one kernel path serves every L (the plan says so), and the last two
# are the sizes at which the model's own geopotential kernel changes path
SHAPES = ((6, 10, 3), (6, 70, 2), (4, 300, 2), (24, 36, 9), (4, 12, 26), (4, 12, 42))
BAND_SHAPE = (24, 36, 9)
PTOP = 1000.0
DT = 120.0
TOL = 1e-10
NT = 9


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


_case_cache = {}


def masked_case(shape, ptop, dtype):
    """(geom, state, levels, heightmap, targets, the restatement's (Z, valid)): the state with p scaled per column, the
    bump, the targets taken from the restatement -- computed once per case, read-only"""
    key = (shape, ptop, dtype)
    if key not in _case_cache:
        H, W, L = shape
        geom = su.geom_of(H, W, L, ptop, bump=True)
        st = pref.with_topography(inp.state_of(geom, dtype), dtype)
        lev = href.level_arrays(geom)
        hm = np.asarray(geom.heightmap, dtype=np.float64)
        P = pref.targets_for(st[0], lev[0], ptop, NT)
        pref.assert_masking_is_exercised(st[0], lev[0], ptop, P)
        Z, valid = href.heights(st[0], st[3], *lev, ptop, hm, P)
        for a in st + [P, Z, valid]:
            a.setflags(write=False)
        _case_cache[key] = (geom, st, lev, hm, P, Z, valid)
    return _case_cache[key]


def assert_plan(c, shape, N):
    """the launch geometry of a sample, through the plan: one path whatever L"""
    H, W, L = shape
    plan = c.plev_maps_plan()
    assert plan == dict(chunks=-(-W // 256), rows=H, threads=256, lds_bytes=8 * (256 + 64), targets=N), plan


# ---------------------------------------------------------------- 1: the map call against the restatement
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ptop", [0.0, PTOP])
@pytest.mark.parametrize("shape", SHAPES)
def test_plev_height_equals_the_restatement(g, shape, ptop, dtype):
    H, W, L = shape
    geom, st, lev, hm, P, want, wvalid = masked_case(shape, ptop, dtype)
    trs, gt = inp.tracers(H, W, L, 2), inp.ground(H, W)
    c = su.single(g, geom, st, trs, dtype=dtype, gt=gt)
    assert c.plev_maps_plan()["rows"] == 0                      # (nothing registered: no work)
    c.set_plev_maps(10 ** 6, P)
    assert_plan(c, shape, P.size)
    trs0 = c.get_tracers()
    fill = -12345.5
    Z, valid = c.plev_height(P, fill=fill)
    assert Z.shape == (P.size, H, W) and valid.shape == (P.size, H, W)
    assert np.array_equal(valid, wvalid)
    assert np.all(Z[~valid] == fill) and np.isfinite(Z[valid]).all()
    err = float(np.max(np.abs(Z[valid] - want[valid])) / np.max(np.abs(want[valid])))
    print("largest |Z device - Z restatement| / max |Z|", shape, ptop, dtype, err)
    assert err <= TOL
    # the host build runs the same march: the same bits
    hz, hv = g.plev_height_columns(st[0], np.moveaxis(st[3], 0, -1), P, *lev, ptop=ptop, hmG=hm * href.G)
    assert np.array_equal(np.moveaxis(hv, -1, 0), valid) and same_bits(np.moveaxis(hz, -1, 0)[valid], Z[valid])
    # NaN is the default fill
    Z2, valid2 = c.plev_height(P)
    assert np.array_equal(valid2, valid) and np.isnan(Z2[~valid]).all() and same_bits(Z2[valid], Z[valid])
    # a pure reader
    for k, a, b in zip("puvtq", c.get_state(), st):
        assert np.array_equal(a, b), k
    assert np.array_equal(c.get_tracers(), trs0) and np.array_equal(c.get_ground(), gt)
    c.close()


@pytest.mark.parametrize("shape", [(6, 10, 3), (24, 36, 9), (4, 12, 42)])
def test_levels_against_the_devices_own_geopotential(g, shape):
    """fp64, the same p in every column, targets on all L levels: Z G is the level's phi, held to the device's own
    dynamics.compute_geopotential within 1e-10 max |phi|.  Not bit for bit: the model's kernel takes a reciprocal
    approximation for 1 / rho where the rule divides"""
    from gcmiipy_amd import dynamics
    H, W, L = shape
    geom = su.geom_of(H, W, L, PTOP, bump=True)
    st = inp.state_of(geom)
    p = np.full((H, W), 9.3e4)
    lev = href.level_arrays(geom)
    pl = lev[0] * 9.3e4 + PTOP
    c = su.single(g, geom, [p] + st[1:])
    Z, valid = c.plev_height(pl)
    c.close()
    assert valid.all()
    phi = np.asarray(dynamics.compute_geopotential(p, st[3], geom))
    err = float(np.max(np.abs(Z * href.G - phi)) / np.max(np.abs(phi)))
    print("largest |Z G - phi of the device's model| / max |phi|", shape, err)
    assert err <= TOL


# ---------------------------------------------------------------- 2: the registered phase
def stepping_case(dtype, ptop=0.0):
    """the band shape's geometry with the bump, its state with a smooth stand-in for topography (steps are taken from
    it) and nine targets"""
    H, W, L = BAND_SHAPE
    geom = su.geom_of(H, W, L, ptop, bump=True)
    st = pref.with_topography(inp.state_of(geom, dtype), dtype, smooth=True)
    P = pref.targets_for(st[0], href.level_arrays(geom)[0], ptop, NT)
    pref.assert_masking_is_exercised(st[0], href.level_arrays(geom)[0], ptop, P)
    return geom, st, P


def assert_sums_equal(got, want, what=""):
    assert got[0] == want[0], (what, got[0], want[0])
    for w in range(13):
        assert same_bits(got[1][w], want[1][w]), (what, "word", w)
    assert same_bits(got[2], want[2]), (what, "s2")


def device_terms(c, P):
    """the thirteen terms and [p, p p] of the handle's current state from the device's own map calls"""
    Z, valid = c.plev_height(P)
    F, v2 = c.plev_fields(P)
    assert np.array_equal(valid, v2)
    uc, vc, _, T, q = F
    raw = [np.ones(valid.shape), Z, Z * Z, T, T * T, uc, vc, uc * uc, vc * vc, uc * vc, vc * T, q, vc * q]
    p = c.get_state()[0]
    return np.stack([np.where(valid, x, 0.0) for x in raw]), np.stack([p, p * p]), valid


@pytest.mark.parametrize("ptop", [0.0, PTOP])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_registered_equals_explicit(g, dtype, ptop):
    """5 steps with every = 2: the sums are, bit for bit, a NumPy float64 accumulation of the device's own plev_height
    and plev_fields outputs taken at steps 2 and 4 with the same products; the count is the masks' sum; against the
    restatement of the states at those steps the words without an Exner routine are bit for bit, the others within
    1e-10 sum |term|"""
    geom, st, P = stepping_case(dtype, ptop)
    lev, hm = href.level_arrays(geom), np.asarray(geom.heightmap, dtype=np.float64)
    a = su.single(g, geom, st, dtype=dtype)
    a.set_plev_maps(2, P)
    assert_plan(a, BAND_SHAPE, P.size)
    assert a.plev_maps_every == 2 and np.array_equal(a.plev_maps_levels, P) and a.plev_maps().n == 0
    a.step(5, DT)
    got = a.plev_maps_sums()
    assert got[0] == 2 and np.isfinite(got[1]).all()
    b = su.single(g, geom, st, dtype=dtype)
    s, s2, masks, seen = 0.0, 0.0, 0, []
    for _ in range(2):
        b.step(2, DT)
        t, t2, valid = device_terms(b, P)
        s, s2, masks = s + t, s2 + t2, masks + valid
        seen.append(b.get_state())
    b.step(1, DT)
    assert_sums_equal(got, (2, s, s2), "explicit")
    assert np.array_equal(got[1][0], masks.astype(np.float64))
    partly = (got[1][0] > 0) & (got[1][0] < 2)
    print("cells valid in one of the two samples only", dtype, ptop, int(partly.sum()))
    for k, x, y in zip("puvtq", a.get_state(), b.get_state()):
        assert np.array_equal(x, y), k
    b.close()
    n, rs, rs2, bnd = href.accumulate(seen, *lev, ptop, hm, P)
    assert n == 2 and same_bits(got[2], rs2)
    for w in href.EXACT_WORDS:
        assert same_bits(got[1][w], rs[w]), ("word", w)
    worst = 0.0
    for w in href.EXNER_WORDS:
        d = np.abs(got[1][w] - rs[w])
        ratio = np.where(bnd[w] > 0.0, d / np.where(bnd[w] > 0.0, bnd[w], 1.0), d)
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= TOL, ("word", w, float(ratio.max()))
    print("largest |device - restatement| / sum |term| of the Exner words", dtype, ptop, worst)
    # the counter runs across calls; explicit samples leave it alone; half steps never sample
    c = su.single(g, geom, st, dtype=dtype)
    c.set_plev_maps(2, P)
    for _ in range(5):
        c.step(1, DT)
    assert_sums_equal(c.plev_maps_sums(), got, "step(1) five times")
    c.close()
    a.half_step(0, DT)
    a.half_step(1, DT)
    assert a.plev_maps_sums()[0] == 2
    # the record
    rec = a.plev_maps()
    some = got[1][0] > 0
    assert rec.n == 2 and same_bits(rec.coverage, got[1][0] / 2.0) and same_bits(rec.Z[some], (got[1][1][some] / got[1][0][some]))
    assert np.isnan(rec.Z[~some]).all() and (~some).any() and same_bits(rec.p, got[2][0] / 2.0)
    a.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_without_a_registration_nothing_changes(g, dtype):
    """the plan shows no work, and the state after three steps is, bit for bit, that of a handle that registered the
    maps (the sample is a pure reader) and of one that registered and unregistered"""
    H, W, L = BAND_SHAPE
    geom, st, P = stepping_case(dtype)
    trs, gt = inp.tracers(H, W, L, 2), inp.ground(H, W)
    never = su.single(g, geom, st, trs, dtype=dtype, gt=gt, phys=True, hs={})
    plan = never.plev_maps_plan()
    assert plan["rows"] == 0 and plan["targets"] == 0 and never.plev_maps_every == 0
    on = su.single(g, geom, st, trs, dtype=dtype, gt=gt, phys=True, hs={})
    on.set_plev_maps(1, P)
    off = su.single(g, geom, st, trs, dtype=dtype, gt=gt, phys=True, hs={})
    off.set_plev_maps(1, P)
    off.set_plev_maps(0)
    assert off.plev_maps_every == 0 and off.plev_maps_plan()["rows"] == 0
    for c in (never, on, off):
        c.step(2, DT)
        c.step(1, DT)
    assert on.plev_maps_sums()[0] == 3
    for c in (on, off):
        for k, x, y in zip("puvtq", c.get_state(), never.get_state()):
            assert np.array_equal(x, y), k
        assert np.array_equal(c.get_tracers(), never.get_tracers()) and np.array_equal(c.get_ground(), never.get_ground())
        assert c.utc() == never.utc()
    for c in (never, on, off):
        c.close()


# ---------------------------------------------------------------- 3: bands
_single_cache = {}


def single_reference(g, dtype, steps, every=1):
    """the single domain with Held-Suarez after `steps` steps: (the maps' sums, state), once per case"""
    key = (dtype, steps, every)
    if key not in _single_cache:
        geom, st, P = stepping_case(dtype)
        c = su.single(g, geom, st, dtype=dtype, hs={})
        c.set_plev_maps(every, P)
        c.step(steps, DT)
        _single_cache[key] = (c.plev_maps_sums(), c.get_state())
        c.close()
    return _single_cache[key]


def merged_sums(cores):
    """merge_plev_maps of the bands' records, and the raw sums put together the same way"""
    from gcmiipy_amd.bands import merge_plev_maps
    merged = merge_plev_maps([c.plev_maps() for c in cores])
    raw = [c.plev_maps_sums() for c in cores]
    assert all(r[0] == merged.n for r in raw)
    return merged, (merged.n, np.concatenate([r[1] for r in raw], axis=-2), np.concatenate([r[2] for r in raw], axis=-2))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_three_in_process_bands_equal_the_single_domain(g, dtype):
    """three bands of 8 rows, whole stages, two exchanges per step, the Held-Suarez forcing on own rows and ghost rows,
    then the sample: every word, vc of each band's first row (which reads the ghost row) included.  The bump lies in the
    middle band: its heightmap row is the global row"""
    import torch
    steps = 4
    want, _ = single_reference(g, dtype, steps)
    geom, st, P = stepping_case(dtype)
    j = int(np.argwhere(np.asarray(geom.heightmap) > 0)[0][0])
    assert 8 <= j < 16
    cores = su.bands(g, geom, 3, st, dtype=dtype)
    for c in cores:
        assert c.H == 8
        c.set_held_suarez(geom)
        c.set_plev_maps(1, P)

    def forcing_and_sample(k):
        for c in cores:
            c.held_suarez_step(geom, DT)
            c.plev_maps_sample()
    su.whole_steps(cores, torch, steps, DT, after=forcing_and_sample)
    merged, raw = merged_sums(cores)
    assert_sums_equal(raw, want, "three bands")
    whole = g.PlevMaps.from_sums(want[0], P, want[1], want[2])
    for f, a, b in zip(g.PlevMaps._fields[1:], merged[1:], whole[1:]):
        assert np.array_equal(a, b, equal_nan=True), f
    # the map call on a band: its rows of the single domain's
    one = su.single(g, geom, st, dtype=dtype)
    Z, valid = one.plev_height(P)
    one.close()
    fresh = su.bands(g, geom, 3, st, dtype=dtype)
    for r, c in enumerate(fresh):
        zb, vb = c.plev_height(P)
        sl = slice(8 * r, 8 * r + 8)
        assert np.array_equal(vb, valid[:, sl]) and same_bits(zb[vb], Z[:, sl][vb]), r
    for c in cores + fresh:
        c.close()


def loopback(g, torch, geom, dtype, P, every):
    """the band that is its own neighbour, driven by gcm_band_run, everything registered ahead of the runner"""
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange
    H, W, L = geom.height, geom.width, geom.layers
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0, dtype=dtype,
               stream=torch.cuda.current_stream().cuda_stream)
    eng = HipBandEngine(c, torch)
    eng.set_held_suarez(geom)
    eng.set_plev_maps(every, P)
    return c, BandRunner(eng, 0, 2, LoopbackExchange(), north=0, south=0)


@pytest.mark.parametrize("comm_stream", [False, True], ids=["second-stream", "comm-stream"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_loopback_band_run_equals_the_single_domain(g, dtype, comm_stream, monkeypatch):
    """the loopback band of gcm_band_run with Held-Suarez, the exchange on the library's second stream or
    (GCM_BAND_COMM_STREAM=1, read by gcm_set_exchange) on the comm stream; 3 + 1 steps with every = 2, so the counter
    runs across the two calls and the first ends between two samples.  State and sums are the single domain's after
    step(4), bit for bit"""
    import torch
    want, want_state = single_reference(g, dtype, 4, every=2)
    assert want[0] == 2
    geom, st, P = stepping_case(dtype)
    if comm_stream:
        monkeypatch.setenv("GCM_BAND_COMM_STREAM", "1")
    else:
        monkeypatch.delenv("GCM_BAND_COMM_STREAM", raising=False)
    c, runner = loopback(g, torch, geom, dtype, P, 2)
    assert runner.native
    c.set_state(*st)
    runner.run(3, DT)
    runner.run(1, DT)
    torch.cuda.synchronize()
    _, raw = merged_sums([c])
    assert_sums_equal(raw, want, "loopback")
    for k, x, y in zip("puvtq", c.get_state(), want_state):
        assert np.array_equal(x, y), k
    c.close()


# ---------------------------------------------------------------- 4: reset, put / get, checkpoint
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_reset_put_get_and_checkpoint(g, dtype, tmp_path):
    from gcmiipy_amd import checkpoint
    geom, st, P = stepping_case(dtype)
    H, W, L = BAND_SHAPE

    def handle(state):
        c = su.single(g, geom, state, dtype=dtype, hs={})
        c.set_plev_maps(1, P)
        return c
    whole = handle(st)
    whole.step(5, DT)
    want = whole.plev_maps_sums()
    assert want[0] == 5
    whole.plev_maps_reset()
    n, s, s2 = whole.plev_maps_sums()
    assert n == 0 and not s.any() and not s2.any()
    # registering again resets too, and takes other targets
    whole.step(1, DT)
    assert whole.plev_maps_sums()[0] == 1
    whole.set_plev_maps(3, P[:4])
    n, s, s2 = whole.plev_maps_sums()
    assert n == 0 and s.shape == (13, 4, H, W) and not s.any() and not s2.any() and whole.plev_maps_every == 3
    assert np.array_equal(whole.plev_maps_levels, P[:4])
    whole.close()
    # put then get; put then more steps equals the uninterrupted run
    a = handle(st)
    a.step(3, DT)
    mid, mid_state = a.plev_maps_sums(), a.get_state()
    path = str(tmp_path / "maps.npz")
    checkpoint.save(path, a, step=3, geom=geom)
    a.close()
    b = handle(mid_state)
    b.put_plev_maps(*mid)
    assert_sums_equal(b.plev_maps_sums(), mid, "put then get")
    b.step(2, DT)
    assert_sums_equal(b.plev_maps_sums(), want, "put then steps")
    b.close()
    # a checkpoint in the middle of the run resumes bit for bit
    r, ck = checkpoint.restore(path)
    assert r.plev_maps_every == 1 and ck["plev_maps"]["n"] == 3 and np.array_equal(r.plev_maps_levels, P)
    assert_sums_equal(r.plev_maps_sums(), mid, "restored")
    r.step(2, DT)
    assert_sums_equal(r.plev_maps_sums(), want, "restored then steps")
    r.close()
    # a handle without the registration: the file holds the keys it held before, and restores with none
    plain = su.single(g, geom, st, dtype=dtype)
    checkpoint.save(path, plain, geom=geom)
    plain.close()
    assert not any(k.startswith("plev_maps") for k in np.load(path).files)
    r, ck = checkpoint.restore(path)
    assert ck["plev_maps"] is None and r.plev_maps_every == 0
    r.close()


# ---------------------------------------------------------------- 5: refusals
def test_refusals_change_nothing(g):
    lib, L_ = g._lib.lib, g._lib
    dp = L_._dp
    geom, st, P = stepping_case("f64")
    H, W, L = BAND_SHAPE
    N = P.size
    c = su.single(g, geom, st)
    s, s2, n = np.zeros((13, N, H, W)), np.zeros((2, H, W)), C.c_int64(7)
    lev = np.full(N, -1.0)
    ptr = lambda a: a.ctypes.data_as(dp)                        # noqa: E731
    # without a registration
    assert c.plev_maps_every == 0
    assert lib.gcm_plev_maps_sample(c._h) == L_.ERR_STATE and lib.gcm_plev_maps_reset(c._h) == L_.ERR_STATE
    assert lib.gcm_get_plev_maps(c._h, ptr(s), ptr(s2), C.byref(n)) == L_.ERR_STATE
    assert lib.gcm_put_plev_maps(c._h, ptr(s), ptr(s2), 1) == L_.ERR_STATE
    assert lib.gcm_plev_maps_levels(c._h, ptr(lev), N) == L_.ERR_STATE
    assert n.value == 7 and np.all(lev == -1.0)
    with pytest.raises(g.GcmError):
        c.plev_maps()
    bad = (np.array([5e4, 8e4]), np.array([8e4, 8e4]), np.array([8e4, -1.0]), np.array([8e4, 0.0]), np.array([np.nan]),
           np.array([np.inf, 5e4]), np.linspace(9e4, 1e4, 65))
    out = np.zeros((2, H, W))
    for B in bad:
        assert lib.gcm_set_plev_maps(c._h, 1, B.size, ptr(B)) == L_.ERR_ARG and c.plev_maps_every == 0
        assert lib.gcm_plev_height(c._h, B.size, ptr(B), 0.0, ptr(out), None) == L_.ERR_ARG
        with pytest.raises(ValueError):
            c.set_plev_maps(1, B)
        with pytest.raises(ValueError):
            c.plev_height(B)
    assert lib.gcm_set_plev_maps(c._h, 1, 0, ptr(P)) == L_.ERR_ARG and lib.gcm_set_plev_maps(c._h, 1, N, None) == L_.ERR_ARG
    assert lib.gcm_set_plev_maps(c._h, -1, N, ptr(P)) == L_.ERR_ARG and c.plev_maps_every == 0
    with pytest.raises(ValueError):
        c.set_plev_maps(-3, P)
    assert lib.gcm_plev_height(c._h, 2, ptr(P), 0.0, None, None) == L_.ERR_ARG and not out.any()
    assert lib.gcm_plev_height(c._h, 2, ptr(P), 0.0, ptr(out), None) == L_.OK and out.any()       # (valid may be NULL)
    plan = (C.c_int * 5)()
    assert lib.gcm_plev_maps_plan(c._h, plan, 4) == L_.ERR_ARG and lib.gcm_plev_maps_plan(c._h, None, 5) == L_.ERR_ARG
    # registered: a refused call leaves the sums, the count and the registration alone
    c.set_plev_maps(1, P)
    c.step(2, DT)
    was = c.plev_maps_sums()
    for B in bad:
        assert lib.gcm_set_plev_maps(c._h, 1, B.size, ptr(B)) == L_.ERR_ARG
    assert lib.gcm_set_plev_maps(c._h, -1, N, ptr(P)) == L_.ERR_ARG
    assert lib.gcm_put_plev_maps(c._h, None, ptr(s2), 1) == L_.ERR_ARG and lib.gcm_put_plev_maps(c._h, ptr(s), None, 1) == L_.ERR_ARG
    assert lib.gcm_put_plev_maps(c._h, ptr(s), ptr(s2), -1) == L_.ERR_ARG
    with pytest.raises(ValueError):
        c.put_plev_maps(1, np.zeros((13, N, H + 1, W)), s2)
    assert c.plev_maps_every == 1 and np.array_equal(c.plev_maps_levels, P)
    assert_sums_equal(c.plev_maps_sums(), was, "after refused calls")
    # levels: the count comes back whatever the capacity; null pointers of get are allowed
    assert lib.gcm_plev_maps_levels(c._h, None, 0) == N and lib.gcm_plev_maps_levels(c._h, ptr(lev), 2) == N
    assert np.array_equal(lev[:2], P[:2]) and np.all(lev[2:] == -1.0)
    assert lib.gcm_get_plev_maps(c._h, None, None, C.byref(n)) == L_.OK and n.value == 2
    assert lib.gcm_get_plev_maps(c._h, None, None, None) == L_.OK
    # every = 0 unregisters
    c.set_plev_maps(0)
    assert c.plev_maps_every == 0
    with pytest.raises(g.GcmError):
        c.plev_maps()
    c.close()
    # a column of one level has no bracket
    one = su.single(g, su.geom_of(6, 10, 1))
    out1 = np.zeros((2, 6, 10))
    assert lib.gcm_set_plev_maps(one._h, 1, N, ptr(P)) == L_.ERR_UNSUPPORTED and one.plev_maps_every == 0
    assert lib.gcm_plev_height(one._h, 2, ptr(P), 0.0, ptr(out1), None) == L_.ERR_UNSUPPORTED and not out1.any()
    one.close()
    # other models
    sw = g.Core(L_.SW2D, 32, 16, dx=1e5)
    assert lib.gcm_set_plev_maps(sw._h, 1, N, ptr(P)) == L_.ERR_UNSUPPORTED
    assert lib.gcm_plev_maps_sample(sw._h) == L_.ERR_UNSUPPORTED and lib.gcm_plev_maps_reset(sw._h) == L_.ERR_UNSUPPORTED
    assert lib.gcm_plev_maps_every(sw._h) == 0 and lib.gcm_plev_maps_levels(sw._h, None, 0) == L_.ERR_UNSUPPORTED
    assert lib.gcm_get_plev_maps(sw._h, None, None, None) == L_.ERR_UNSUPPORTED
    assert lib.gcm_put_plev_maps(sw._h, ptr(s), ptr(s2), 1) == L_.ERR_UNSUPPORTED
    assert lib.gcm_plev_maps_plan(sw._h, plan, 5) == L_.ERR_UNSUPPORTED
    assert lib.gcm_plev_height(sw._h, 2, ptr(P), 0.0, ptr(out), None) == L_.ERR_UNSUPPORTED
    sw.close()
