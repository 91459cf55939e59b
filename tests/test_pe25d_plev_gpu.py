"""GCM_PE25D on pressure levels on the device (gcm_plev_fields, gcm_set_plev_climate) against the NumPy restatement
tests/pe25d_plev_ref.py: the maps and one sample on states whose surface pressure is scaled per column to stand in for
topography, planted values at the two wraps and under the ground, the registered phase against explicit samples,
latitude bands (in-process bands with device-copied ghost rows and the loopback band of gcm_band_run, on the second
stream and on the comm stream), reset / put / get / checkpoint and the refusals.  The mask, and everything without the
Exner routine, are bit for bit the restatement's; T within 1e-10 |T| and words 4, 8 and 10 within 1e-10 sum_i |term|:
the project's bound of the Exner routine against np.power, carried through a convex combination and through a sum."""
import ctypes as C

import numpy as np
import pytest

import gpu_setups as su
import pe25d_inputs as inp
import pe25d_plev_ref as ref
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

SHAPES = ((6, 10, 3), (6, 70, 2), (6, 130, 2), (4, 300, 2), (24, 36, 9))      # (H, W, L)
BAND_SHAPE = (24, 36, 9)
PTOP = 1000.0
DT = 120.0
EXNER_TOL = 1e-10


def sig_of(geom):
    return np.asarray(geom.sig, dtype=np.float64).reshape(-1)


def n_targets(shape, per_segment):
    """the number of targets of a shape's case, from the plan's targets per segment: more than one segment everywhere,
    a last segment that is not full in all but one"""
    n = {0: 2 * per_segment - 1, 1: per_segment + 2, 2: 2 * per_segment, 3: 2 * per_segment + 1, 4: 2 * per_segment - 1}
    return n[SHAPES.index(shape)]


_case_cache = {}


def masked_case(g, shape, ptop, dtype):
    """(geom, state, targets, restatement's (out, valid), its sample, its bound): the state with p scaled per column, the
    targets taken from the restatement, the masking conditions asserted on it -- computed once per case, read-only"""
    key = (shape, ptop, dtype)
    if key not in _case_cache:
        H, W, L = shape
        geom = su.geom_of(H, W, L, ptop)
        st = ref.with_topography(inp.state_of(geom, dtype), dtype)
        probe = su.single(g, geom, st, dtype=dtype)
        per = probe.plev_climate_plan()["targets"]
        probe.close()
        sig = sig_of(geom)
        P = ref.targets_for(st[0], sig, ptop, n_targets(shape, per))
        ref.assert_masking_is_exercised(st[0], sig, ptop, P)
        out, valid = ref.fields(*st, sig, ptop, P)
        s, b = ref.sample(*st, sig, ptop, P), ref.bound(*st, sig, ptop, P)
        for a in st + [P, out, valid, s, b]:
            a.setflags(write=False)
        _case_cache[key] = (geom, st, P, out, valid, s, b)
    return _case_cache[key]


def assert_plan(c, shape, N):
    """the launch geometry the case is meant to have, through the plan"""
    H, W, L = shape
    plan = c.plev_climate_plan()
    per = plan["targets"]
    assert plan["grid_x"] == H and plan["threads"] == 256 and plan["chunks"] == -(-W // 256)
    assert plan["nseg"] == -(-N // per) and plan["nseg"] > 1
    assert plan["lds_bytes"] > 0
    return plan


def assert_sums_equal(got, want, what=""):
    assert got[0] == want[0], (what, got[0], want[0])
    for w in range(13):
        assert np.array_equal(got[1][w], want[1][w]), (what, "word", w)


def assert_sums_match_restatement(got, want, bnd, what=""):
    """got, want: (n, s); bnd (13, N, H): sum over samples and i of |term|"""
    assert got[0] == want[0], (what, got[0], want[0])
    for w in ref.EXACT_WORDS:
        assert np.array_equal(got[1][w], want[1][w]), (what, "word", w, float(np.max(np.abs(got[1][w] - want[1][w]))))
    worst = 0.0
    for w in ref.EXNER_WORDS:
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(bnd[w] > 0.0, np.abs(got[1][w] - want[1][w]) / bnd[w], np.abs(got[1][w] - want[1][w]))
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= EXNER_TOL, (what, "word", w, float(ratio.max()))
    return worst


def test_the_cases_cover_the_segment_geometries(g):
    """over the shapes: more than one target segment, a full last segment and a last segment that is not full"""
    c = su.single(g, su.geom_of(*SHAPES[0]))
    per = c.plev_climate_plan()["targets"]
    assert c.plev_climate_plan()["nseg"] == 0                   # (no registration yet)
    c.close()
    ns = [n_targets(s, per) for s in SHAPES]
    assert all(n > per for n in ns) and any(n % per == 0 for n in ns) and any(n % per != 0 for n in ns)
    assert all(6 <= n <= g._lib.PLEV_MAX for n in ns)


# ---------------------------------------------------------------- 1: the maps against the restatement
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ptop", [0.0, PTOP])
@pytest.mark.parametrize("shape", SHAPES)
def test_fields_equal_the_restatement(g, shape, ptop, dtype):
    H, W, L = shape
    geom, st, P, want, wvalid, _, _ = masked_case(g, shape, ptop, dtype)
    trs, gt = inp.tracers(H, W, L, 2), inp.ground(H, W)
    c = su.single(g, geom, st, trs, dtype=dtype, gt=gt)
    trs0 = c.get_tracers()
    fill = -12345.5
    out, valid = c.plev_fields(P, fill=fill)
    assert out.shape == (5, P.size, H, W) and valid.shape == (P.size, H, W)
    assert np.array_equal(valid, wvalid)
    assert np.all(out[:, ~valid] == fill)
    for n, name in enumerate(ref.QUANTITIES):
        if name != "T":
            assert np.array_equal(out[n][valid], want[n][valid]), (name, shape, ptop, dtype)
    err = np.abs(out[3][valid] - want[3][valid]) / np.abs(want[3][valid])
    print("largest |T device - T restatement| / |T|", shape, ptop, dtype, float(err.max()))
    assert err.max() <= EXNER_TOL
    # NaN is the default fill
    out2, valid2 = c.plev_fields(P)
    assert np.array_equal(valid2, valid) and np.isnan(out2[:, ~valid]).all() and np.array_equal(out2[:, valid], out[:, valid])
    # a pure reader
    for k, a, b in zip("puvtq", c.get_state(), st):
        assert np.array_equal(a, b), k
    assert np.array_equal(c.get_tracers(), trs0) and np.array_equal(c.get_ground(), gt)
    c.close()


# ---------------------------------------------------------------- 2: one sample against the restatement
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ptop", [0.0, PTOP])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_sample_equals_the_restatement(g, shape, ptop, dtype):
    H, W, L = shape
    geom, st, P, _, wvalid, want, bnd = masked_case(g, shape, ptop, dtype)
    c = su.single(g, geom, st, dtype=dtype, gt=inp.ground(H, W))
    c.set_plev_climate(10 ** 6, P)
    assert_plan(c, shape, P.size)
    assert c.plev_climate_every == 10 ** 6 and np.array_equal(c.plev_climate_levels, P) and c.plev_climate().n == 0
    c.plev_climate_sample()
    got = c.plev_climate_sums()
    assert np.array_equal(got[1][0], wvalid.sum(axis=-1).astype(np.float64))
    worst = assert_sums_match_restatement(got, (1, want), bnd, shape)
    print("largest |device - restatement| / sum|term| of the Exner words", shape, ptop, dtype, worst)
    for k, a, b in zip("puvtq", c.get_state(), st):
        assert np.array_equal(a, b), k
    # a second read returns the same bits; the record is the sums over the count
    assert_sums_equal(c.plev_climate_sums(), got, "second read")
    rec = c.plev_climate()
    some = got[1][0] > 0
    assert rec.n == 1 and np.array_equal(rec.coverage, got[1][0] / np.float64(W))
    assert np.array_equal(rec.vq[some], got[1][12][some] / got[1][0][some]) and np.isnan(rec.vq[~some]).all() and (~some).any()
    c.close()


# ---------------------------------------------------------------- 3: planted values
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_planted_values_at_the_wraps(g, dtype):
    """p is the same in every column and the one target is the top mid-level's pressure exactly, so the weight is 1 and
    the interpolated value the top level's own.  u nonzero only at (L - 1, H - 1, W - 1), v nonzero only in row H - 1 at
    i = 0.  The i wrap: uc at i = 0 takes u[W - 1], so word 9 of row H - 1 is exactly that one product and exactly 0 in
    every other row.  The j wrap: row H - 1 is row -1 of row 0, so vc of row 0 is 0.5 v[H - 1] at i = 0 and word 11 of
    row 0 exactly that times theta"""
    H, W, L = 6, 10, 3
    geom = su.geom_of(H, W, L)
    st = inp.state_of(geom, dtype)
    p = np.full((H, W), 1e5)
    u, v = np.zeros((L, H, W)), np.zeros((L, H, W))
    u[L - 1, H - 1, W - 1] = 6.0
    v[:, H - 1, 0] = 3.0 + np.arange(L)
    st = [p, u, v, st[3], st[4]]
    sig = sig_of(geom)
    P = np.array([sig[L - 1] * 1e5 + 0.0])
    c = su.single(g, geom, st, dtype=dtype)
    c.set_plev_climate(1, P)
    c.plev_climate_sample()
    n, s = c.plev_climate_sums()
    c.close()
    assert np.array_equal(s[0], np.full((1, H), float(W)))
    want9 = np.zeros((1, H))
    want9[0, H - 1] = (0.5 * (0.0 + 6.0)) * (0.5 * (3.0 + (L - 1) + 0.0))           # uc[i = 0] vc[i = 0]
    assert np.array_equal(s[9], want9), s[9]
    th = st[3]
    want11 = np.zeros((1, H))
    want11[0, 0] = (0.5 * v[L - 1, H - 1, 0]) * th[L - 1, 0, 0]
    want11[0, H - 1] = (0.5 * v[L - 1, H - 1, 0]) * th[L - 1, H - 1, 0]
    assert np.array_equal(s[11], want11), s[11]
    assert s[1][0, H - 1] == 0.5 * 6.0 + 0.5 * 6.0 and not s[1][0, :H - 1].any()       # uc at i = W - 1 and at i = 0
    r = ref.sample(*st, sig, 0.0, P)
    for w in ref.EXACT_WORDS:
        assert np.array_equal(s[w], r[w]), w


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_column_under_the_ground_appears_in_no_word(g, dtype):
    """one column's surface pressure (10 hPa) puts every target under its ground, and its theta is huge on every level:
    no word may see it, and the count of its row is W - 1 for every target"""
    H, W, L = 6, 70, 3
    geom = su.geom_of(H, W, L)
    st = inp.state_of(geom, dtype)
    sig = sig_of(geom)
    j0, i0 = 2, 65                                              # (the second wave's tail)
    p, th = st[0].copy(), st[3].copy()
    p[j0, i0] = 1e3
    th[:, j0, i0] = 1e30
    st = [p, st[1], st[2], th, st[4]]
    lo, hi = (sig[L - 1] * p).max(), (sig[0] * np.delete(p.ravel(), j0 * W + i0)).min()
    P = np.linspace(hi, lo, 7)[1:-1].copy()
    assert P.min() > sig[0] * 1e3 and lo < hi
    c = su.single(g, geom, st, dtype=dtype)
    c.set_plev_climate(1, P)
    c.plev_climate_sample()
    n, s = c.plev_climate_sums()
    out, valid = c.plev_fields(P)
    c.close()
    count = np.full((P.size, H), float(W))
    count[:, j0] = W - 1
    assert np.array_equal(s[0], count)
    assert np.isfinite(s).all() and np.abs(s).max() < 1e20
    assert not valid[:, j0, i0].any() and valid.sum() == P.size * (H * W - 1) and np.isnan(out[:, :, j0, i0]).all()
    r = ref.sample(*st, sig, 0.0, P)
    for w in ref.EXACT_WORDS:
        assert np.array_equal(s[w], r[w]), w


# ---------------------------------------------------------------- 4, 5: the registered phase
def stepping_case(dtype, ptop=0.0):
    """the band shape's state with a smooth stand-in for topography (steps are taken from it) and nine targets"""
    H, W, L = BAND_SHAPE
    geom = su.geom_of(H, W, L, ptop)
    st = ref.with_topography(inp.state_of(geom, dtype), dtype, smooth=True)
    P = ref.targets_for(st[0], sig_of(geom), ptop, 9)
    ref.assert_masking_is_exercised(st[0], sig_of(geom), ptop, P)
    return geom, st, P


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_registered_equals_explicit_samples(g, dtype):
    geom, st, P = stepping_case(dtype)
    a = su.single(g, geom, st, dtype=dtype)
    a.set_plev_climate(2, P)
    a.step(5, DT)
    got = a.plev_climate_sums()
    assert got[0] == 2 and np.isfinite(got[1]).all()
    partly = (got[1][0] > 0) & (got[1][0] < 2 * geom.width)
    assert partly.any()
    state_a = a.get_state()
    b = su.single(g, geom, st, dtype=dtype)
    b.set_plev_climate(10 ** 6, P)
    for n, sample in ((2, True), (2, True), (1, False)):
        b.step(n, DT)
        if sample:
            b.plev_climate_sample()
    assert_sums_equal(got, b.plev_climate_sums(), "explicit")
    b.close()
    # the counter runs across calls
    c = su.single(g, geom, st, dtype=dtype)
    c.set_plev_climate(2, P)
    for _ in range(5):
        c.step(1, DT)
    assert_sums_equal(got, c.plev_climate_sums(), "step(1) five times")
    c.close()
    # half steps never sample
    a.half_step(0, DT)
    a.half_step(1, DT)
    assert a.plev_climate_sums()[0] == 2
    a.close()
    for k, x in zip("puvtq", state_a):
        assert np.isfinite(x).all(), k


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_registered_sample_sees_the_forced_state(g, dtype):
    """Held-Suarez registered as well: the sample follows it.  The states at the sampling points, taken from an identical
    run, go through the restatement"""
    geom, st, P = stepping_case(dtype)
    a = su.single(g, geom, st, dtype=dtype, hs={})
    a.set_plev_climate(2, P)
    a.step(5, DT)
    got = a.plev_climate_sums()
    a.close()
    b = su.single(g, geom, st, dtype=dtype, hs={})
    seen = []
    for n in (2, 2):
        b.step(n, DT)
        seen.append(b.get_state())
    b.close()
    sig = sig_of(geom)
    want = ref.accumulate(seen, sig, 0.0, P)
    bnd = sum(ref.bound(*s, sig, 0.0, P) for s in seen)
    worst = assert_sums_match_restatement(got, want, bnd, "forced")
    print("largest ratio of the Exner words, forced state", dtype, worst)
    plain = su.single(g, geom, st, dtype=dtype)
    plain.set_plev_climate(2, P)
    plain.step(5, DT)
    assert not np.array_equal(plain.plev_climate_sums()[1][3], got[1][3])
    plain.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_registration_leaves_the_model_alone(g, dtype):
    H, W, L = BAND_SHAPE
    geom, st, P = stepping_case(dtype)
    trs, gt = inp.tracers(H, W, L, 2), inp.ground(H, W)
    a = su.single(g, geom, st, trs, dtype=dtype, gt=gt, phys=True, hs={})
    a.set_plev_climate(1, P)
    b = su.single(g, geom, st, trs, dtype=dtype, gt=gt, phys=True, hs={})
    for c in (a, b):
        c.step(2, DT)
        c.step(1, DT)
    assert a.plev_climate_sums()[0] == 3
    for k, x, y in zip("puvtq", a.get_state(), b.get_state()):
        assert np.array_equal(x, y), k
    assert np.array_equal(a.get_tracers(), b.get_tracers()) and np.array_equal(a.get_ground(), b.get_ground())
    assert a.utc() == b.utc()
    a.close()
    b.close()


# ---------------------------------------------------------------- 6: bands
_single_cache = {}


def single_reference(g, dtype, steps, every=1, beside=False):
    """the single domain with Held-Suarez after `steps` steps: (plev sums, state, climatology's sums, spectra's sums), once
    per case; beside: the sigma climatology and the spectra are registered as well"""
    key = (dtype, steps, every, beside)
    if key not in _single_cache:
        geom, st, P = stepping_case(dtype)
        c = su.single(g, geom, st, dtype=dtype, hs={}, every=every if beside else None)
        if beside:
            c.set_spectra(every)
        c.set_plev_climate(every, P)
        c.step(steps, DT)
        out = [c.plev_climate_sums(), c.get_state(), c.climate_sums() if beside else None, c.spectra_sums() if beside else None]
        c.close()
        _single_cache[key] = out
    return _single_cache[key]


def merged_sums(cores):
    """merge_plev_climate of the bands' records, and the raw sums put together the same way"""
    from gcmiipy_amd.bands import merge_plev_climate
    merged = merge_plev_climate([c.plev_climate() for c in cores])
    raw = [c.plev_climate_sums() for c in cores]
    assert all(r[0] == merged.n for r in raw)
    return merged, (merged.n, np.concatenate([r[1] for r in raw], axis=-1))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_three_in_process_bands_equal_the_single_domain(g, dtype):
    """three bands of 8 rows, whole stages, two exchanges per step, the Held-Suarez forcing on own rows and ghost rows,
    then the sample: every word, vc of each band's first row (which reads the ghost row) included"""
    import torch
    steps = 4
    want, want_state, _, _ = single_reference(g, dtype, steps)
    geom, st, P = stepping_case(dtype)
    cores = su.bands(g, geom, 3, st, dtype=dtype)
    for c in cores:
        assert c.H == 8
        c.set_held_suarez(geom)
        c.set_plev_climate(1, P)

    def forcing_and_sample(k):
        for c in cores:
            c.held_suarez_step(geom, DT)
            c.plev_climate_sample()
    su.whole_steps(cores, torch, steps, DT, after=forcing_and_sample)
    merged, raw = merged_sums(cores)
    assert_sums_equal(raw, want, "three bands")
    whole = g.PlevClimate.from_sums(want[0], P, want[1], geom.width)
    for f, a, b in zip(g.PlevClimate._fields[1:], merged[1:], whole[1:]):
        assert np.array_equal(a, b, equal_nan=True), f
    for c in cores:
        c.close()


def loopback(g, torch, geom, dtype, P, every, beside):
    """the band that is its own neighbour, driven by gcm_band_run, everything registered ahead of the runner"""
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange
    H, W, L = geom.height, geom.width, geom.layers
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0, dtype=dtype,
               stream=torch.cuda.current_stream().cuda_stream)
    eng = HipBandEngine(c, torch)
    eng.set_held_suarez(geom)
    if beside:
        eng.set_climate(every)
        eng.set_spectra(every)
    eng.set_plev_climate(every, P)
    return c, BandRunner(eng, 0, 2, LoopbackExchange(), north=0, south=0)


@pytest.mark.parametrize("beside", [False, True], ids=["alone", "beside-climate-and-spectra"])
@pytest.mark.parametrize("comm_stream", [False, True], ids=["second-stream", "comm-stream"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_loopback_band_run_equals_the_single_domain(g, dtype, comm_stream, beside, monkeypatch):
    """the loopback band of gcm_band_run with Held-Suarez, the exchange on the library's second stream or
    (GCM_BAND_COMM_STREAM=1, read by gcm_set_exchange) on the comm stream; 3 + 1 steps with every = 2, so the first run
    ends between two samples.  beside: the sigma climatology and the spectra sample on the same steps, all three behind
    the one join.  State and sums are the single domain's after step(4), bit for bit"""
    import torch
    want, want_state, want_clim, want_spec = single_reference(g, dtype, 4, every=2, beside=beside)
    assert want[0] == 2
    geom, st, P = stepping_case(dtype)
    if comm_stream:
        monkeypatch.setenv("GCM_BAND_COMM_STREAM", "1")
    else:
        monkeypatch.delenv("GCM_BAND_COMM_STREAM", raising=False)
    c, runner = loopback(g, torch, geom, dtype, P, 2, beside)
    assert runner.native
    c.set_state(*st)
    runner.run(3, DT)
    runner.run(1, DT)
    torch.cuda.synchronize()
    merged, raw = merged_sums([c])
    assert_sums_equal(raw, want, "loopback")
    for k, x, y in zip("puvtq", c.get_state(), want_state):
        assert np.array_equal(x, y), k
    if beside:
        n, m3, m2 = c.climate_sums()
        assert n == want_clim[0] and np.array_equal(m3, want_clim[1]) and np.array_equal(m2, want_clim[2])
        n, s = c.spectra_sums()
        assert n == want_spec[0] and np.array_equal(s, want_spec[1])
    c.close()


# ---------------------------------------------------------------- 7: reset, put / get, checkpoint
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_reset_put_get_and_checkpoint(g, dtype, tmp_path):
    from gcmiipy_amd import checkpoint
    geom, st, P = stepping_case(dtype)

    def handle(state):
        c = su.single(g, geom, state, dtype=dtype, hs={})
        c.set_plev_climate(1, P)
        return c
    whole = handle(st)
    whole.step(5, DT)
    want = whole.plev_climate_sums()
    assert want[0] == 5
    whole.plev_climate_reset()
    n, s = whole.plev_climate_sums()
    assert n == 0 and not s.any()
    # registering again resets too, and takes other targets
    whole.step(1, DT)
    assert whole.plev_climate_sums()[0] == 1
    whole.set_plev_climate(3, P[:4])
    n, s = whole.plev_climate_sums()
    assert n == 0 and s.shape == (13, 4, geom.height) and not s.any() and whole.plev_climate_every == 3
    assert np.array_equal(whole.plev_climate_levels, P[:4])
    whole.close()
    # put then get; put then more steps equals the uninterrupted run
    a = handle(st)
    a.step(3, DT)
    mid, mid_state = a.plev_climate_sums(), a.get_state()
    path = str(tmp_path / "plev.npz")
    checkpoint.save(path, a, step=3, geom=geom)
    a.close()
    b = handle(mid_state)
    b.put_plev_climate(*mid)
    assert_sums_equal(b.plev_climate_sums(), mid, "put then get")
    b.step(2, DT)
    assert_sums_equal(b.plev_climate_sums(), want, "put then steps")
    b.close()
    # a checkpoint in the middle of the run
    r, ck = checkpoint.restore(path)
    assert r.plev_climate_every == 1 and ck["plev_climate"]["n"] == 3 and np.array_equal(r.plev_climate_levels, P)
    assert_sums_equal(r.plev_climate_sums(), mid, "restored")
    r.step(2, DT)
    assert_sums_equal(r.plev_climate_sums(), want, "restored then steps")
    r.close()
    # a file without the keys restores with none
    plain = su.single(g, geom, st, dtype=dtype)
    checkpoint.save(path, plain, geom=geom)
    plain.close()
    r, ck = checkpoint.restore(path)
    assert ck["plev_climate"] is None and r.plev_climate_every == 0
    r.close()


# ---------------------------------------------------------------- 8: refusals
def test_refusals_change_nothing(g):
    lib, L_ = g._lib.lib, g._lib
    dp = L_._dp
    geom, st, P = stepping_case("f64")
    H, W, L = BAND_SHAPE
    N = P.size
    c = su.single(g, geom, st)
    s, n = np.zeros((13, N, H)), C.c_int64(7)
    lev = np.full(N, -1.0)
    ptr = lambda a: a.ctypes.data_as(dp)                        # noqa: E731
    # without a registration
    assert c.plev_climate_every == 0
    assert lib.gcm_plev_climate_sample(c._h) == L_.ERR_STATE and lib.gcm_plev_climate_reset(c._h) == L_.ERR_STATE
    assert lib.gcm_get_plev_climate(c._h, ptr(s), C.byref(n)) == L_.ERR_STATE
    assert lib.gcm_put_plev_climate(c._h, ptr(s), 1) == L_.ERR_STATE
    assert lib.gcm_plev_climate_levels(c._h, ptr(lev), N) == L_.ERR_STATE
    assert n.value == 7 and np.all(lev == -1.0)
    with pytest.raises(g.GcmError):
        c.plev_climate()
    bad = (np.array([5e4, 8e4]), np.array([8e4, 8e4]), np.array([8e4, -1.0]), np.array([8e4, 0.0]), np.array([np.nan]),
           np.array([np.inf, 5e4]), np.linspace(9e4, 1e4, 65))
    for B in bad:
        assert lib.gcm_set_plev_climate(c._h, 1, B.size, ptr(B)) == L_.ERR_ARG and c.plev_climate_every == 0
        with pytest.raises(ValueError):
            c.set_plev_climate(1, B)
    assert lib.gcm_set_plev_climate(c._h, 1, 0, ptr(P)) == L_.ERR_ARG and lib.gcm_set_plev_climate(c._h, 1, N, None) == L_.ERR_ARG
    assert lib.gcm_set_plev_climate(c._h, -1, N, ptr(P)) == L_.ERR_ARG and c.plev_climate_every == 0
    with pytest.raises(ValueError):
        c.set_plev_climate(-3, P)
    out = np.zeros((5, 2, H, W))
    assert lib.gcm_plev_fields(c._h, 2, ptr(bad[0]), 0.0, ptr(out), None) == L_.ERR_ARG
    assert lib.gcm_plev_fields(c._h, 2, ptr(P), 0.0, None, None) == L_.ERR_ARG and not out.any()
    assert lib.gcm_plev_fields(c._h, 2, ptr(P), 0.0, ptr(out), None) == L_.OK and out.any()       # (valid may be NULL)
    plan = (C.c_int * 6)()
    assert lib.gcm_plev_climate_plan(c._h, plan, 5) == L_.ERR_ARG and lib.gcm_plev_climate_plan(c._h, None, 6) == L_.ERR_ARG
    # registered: a refused call leaves the sums, the count and the registration alone
    c.set_plev_climate(1, P)
    c.step(2, DT)
    was = c.plev_climate_sums()
    for B in bad:
        assert lib.gcm_set_plev_climate(c._h, 1, B.size, ptr(B)) == L_.ERR_ARG
    assert lib.gcm_set_plev_climate(c._h, -1, N, ptr(P)) == L_.ERR_ARG
    assert lib.gcm_put_plev_climate(c._h, None, 1) == L_.ERR_ARG and lib.gcm_put_plev_climate(c._h, ptr(s), -1) == L_.ERR_ARG
    with pytest.raises(ValueError):
        c.put_plev_climate(1, np.zeros((13, N, H + 1)))
    assert c.plev_climate_every == 1 and np.array_equal(c.plev_climate_levels, P)
    assert_sums_equal(c.plev_climate_sums(), was, "after refused calls")
    # levels: the count comes back whatever the capacity; null pointers of get are allowed
    assert lib.gcm_plev_climate_levels(c._h, None, 0) == N and lib.gcm_plev_climate_levels(c._h, ptr(lev), 2) == N
    assert np.array_equal(lev[:2], P[:2]) and np.all(lev[2:] == -1.0)
    assert lib.gcm_get_plev_climate(c._h, None, C.byref(n)) == L_.OK and n.value == 2
    assert lib.gcm_get_plev_climate(c._h, None, None) == L_.OK
    # every = 0 unregisters
    c.set_plev_climate(0)
    assert c.plev_climate_every == 0
    with pytest.raises(g.GcmError):
        c.plev_climate()
    c.step(1, DT)
    u = su.single(g, geom, st)
    u.step(3, DT)
    for k, x, y in zip("puvtq", c.get_state(), u.get_state()):
        assert np.array_equal(x, y), k
    c.close()
    u.close()
    # a column of one level has no bracket
    one = su.single(g, su.geom_of(6, 10, 1))
    assert lib.gcm_set_plev_climate(one._h, 1, N, ptr(P)) == L_.ERR_UNSUPPORTED and one.plev_climate_every == 0
    assert lib.gcm_plev_fields(one._h, 2, ptr(P), 0.0, ptr(out), None) == L_.ERR_UNSUPPORTED
    one.close()
    # other models
    sw = g.Core(L_.SW2D, 32, 16, dx=1e5)
    assert lib.gcm_set_plev_climate(sw._h, 1, N, ptr(P)) == L_.ERR_UNSUPPORTED
    assert lib.gcm_plev_climate_sample(sw._h) == L_.ERR_UNSUPPORTED and lib.gcm_plev_climate_reset(sw._h) == L_.ERR_UNSUPPORTED
    assert lib.gcm_plev_climate_every(sw._h) == 0 and lib.gcm_plev_climate_levels(sw._h, None, 0) == L_.ERR_UNSUPPORTED
    assert lib.gcm_get_plev_climate(sw._h, None, None) == L_.ERR_UNSUPPORTED
    assert lib.gcm_put_plev_climate(sw._h, ptr(s), 1) == L_.ERR_UNSUPPORTED
    assert lib.gcm_plev_climate_plan(sw._h, plan, 6) == L_.ERR_UNSUPPORTED
    assert lib.gcm_plev_fields(sw._h, 2, ptr(P), 0.0, ptr(out), None) == L_.ERR_UNSUPPORTED
    sw.close()
