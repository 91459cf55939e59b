"""The zonal wavenumber spectra of GCM_PE25D on the device (gcm_set_spectra) against the NumPy restatement
tests/pe25d_spectra_ref.py: one sample word by word, planted waves, Parseval against the climatology's zonal sums, the
registered phase against explicit samples, latitude bands (in-process bands with device-copied ghost rows, the loopback
band of gcm_band_run on both orchestrations, steps the host ends with gcm_end_step_begin / gcm_end_step_finish), reset /
put / get / checkpoint and the refusals.

The parity bound is derived, not measured: |device - restatement| <= (8 eps log2 W + e 1e-10) B_x B_y per sample, with
eps = 2^-53, B_x = sqrt(W sum_i x_i^2) >= |X_m|, and e the number of T factors of the word (the device's Exner routine
against pow); see pe25d_spectra_ref.bound_factor.  Everything about bands, the registered phase and restarts is bit for
bit."""
import numpy as np
import pytest

import gpu_setups as su
from gpu_setups import g  # noqa: F401  (the fixture)
import pe25d_inputs as inp
import pe25d_spectra_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = ((6, 10, 3), (24, 36, 9), (6, 70, 2), (6, 130, 2), (4, 300, 2))      # (H, W, L): radix 5, 3 and 4, 7, 13; 300 = 4 3 5 5
WIDE = (2, 1440, 2)
BEYOND_64K = (2, 1620, 2)
BAND_SHAPE = (24, 36, 9)
PTOP = 1000.0
DT = 120.0


def sig_of(geom):
    return np.asarray(geom.sig, dtype=np.float64).reshape(-1)


def assert_sums_equal(got, want, what=""):
    assert got[0] == want[0], (what, got[0], want[0])
    assert got[1].shape == want[1].shape, (what, got[1].shape, want[1].shape)
    for w in range(6):
        assert np.array_equal(got[1][w], want[1][w]), (what, "word", ref.WORDS[w])


def assert_within_bound(got, want, unit, W, what="", exner=True, at=None, words=range(6)):
    """got, want (6, L, H, M); unit (6, L, H): the samples' B_x B_y added up; at: a (level, row) index that selects what
    is compared (None: everything).  -> the worst |got - want| as a fraction of the bound, over the words"""
    fac = ref.bound_factor(W, exner)
    at = (Ellipsis,) if at is None else at
    worst = 0.0
    for w in words:
        diff = np.abs(got[w][at] - want[w][at])
        bnd = (fac[w] * unit[w][at])[..., None]
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = float(np.max(np.where(bnd > 0, diff / bnd, np.where(diff > 0, np.inf, 0.0))))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (what, "word", ref.WORDS[w], "fraction of the bound", ratio)
    return worst


# ---------------------------------------------------------------- 1: one sample against the restatement
def one_sample_case(g, shape, ptop, dtype, mmaxes):
    H, W, L = shape
    geom = su.geom_of(H, W, L, ptop)
    st = inp.state_of(geom, dtype)
    trs, gt = inp.tracers(H, W, L, 2), inp.ground(H, W)
    c = su.single(g, geom, st, dtype=dtype, gt=gt)
    c.set_tracers(trs)
    trs0 = c.get_tracers()
    r = ref.rows(st[0], st[1], st[2], st[3], sig_of(geom), ptop)
    unit = ref.unit(*r)
    for mmax in mmaxes:
        c.set_spectra(10 ** 6, mmax)
        assert c.spectra_every == 10 ** 6 and c.spectra_mmax == mmax and c.spectra().n == 0
        c.spectra_sample()
        n, s = c.spectra_sums()
        assert n == 1 and s.shape == (6, L, H, mmax + 1)
        worst = assert_within_bound(s, ref.products(*r, mmax), unit, W, (shape, ptop, dtype, mmax))
        print("largest |device - restatement| as a fraction of the bound", shape, ptop, dtype, "mmax", mmax, worst)
        # a second read returns the same bits, and the record is the documented scaling
        assert_sums_equal(c.spectra_sums(), (n, s), "second read")
        rec, wm = c.spectra(), ref.weights(mmax + 1, W)
        assert rec.n == 1 and rec._fields == ("n",) + ref.WORDS
        for w in range(6):
            assert np.array_equal(rec[1 + w], s[w] * (wm / (np.float64(W) * np.float64(W) * np.float64(1)))), ref.WORDS[w]
        assert np.array_equal(g.Spectra.from_sums(n, s, W).uv, rec.uv)
    # nothing a step reads has changed
    for k, a, b in zip("puvtq", c.get_state(), st):
        assert np.array_equal(a, b), k
    assert np.array_equal(c.get_tracers(), trs0) and np.array_equal(c.get_ground(), gt)
    c.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ptop", [0.0, PTOP])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_sample_equals_the_restatement(g, shape, ptop, dtype):
    """mmax 0, 3 and W / 2 (the Nyquist term, where W - m = m), registered one after the other on one handle"""
    one_sample_case(g, shape, ptop, dtype, (0, 3, shape[1] // 2))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", [WIDE, BEYOND_64K], ids=["1440", "1620"])
def test_one_sample_at_the_product_width_and_beyond_64_kb(g, shape, dtype):
    """W = 1440 with all 721 wavenumbers: more than 512 per row, two to a thread.  W = 1620: the launch asks for
    66848 bytes of LDS, more than the 64 KB a kernel gets without its attribute raised"""
    if shape == BEYOND_64K:
        assert 32 * shape[1] + 8 * shape[1] + 2048 > 64 * 1024
    one_sample_case(g, shape, 0.0, dtype, (shape[1] // 2,))


def test_default_mmax_and_the_plan(g):
    H, W, L = SHAPES[1]
    geom = su.geom_of(H, W, L)
    c = su.single(g, geom, inp.state_of(geom))
    c.set_spectra()
    assert c.spectra_every == 1 and c.spectra_mmax == min(W // 2, 63)
    plan = c.spectra_plan()
    assert plan["grid_x"] == H and 1 <= plan["nseg"] <= L and plan["threads"] == 512 and plan["per_thread"] == 1
    assert plan["lds_bytes"] == 32 * W + 8 * W + 2048
    c.close()
    geom = su.geom_of(*WIDE)
    c = su.single(g, geom, inp.state_of(geom))
    c.set_spectra(1, 720)
    plan = c.spectra_plan()
    assert plan["lds_bytes"] == 59648 and plan["per_thread"] == 2 and plan["passes"] == 6
    c.set_spectra(1)
    assert c.spectra_mmax == 63 and c.spectra_plan()["per_thread"] == 1
    c.close()


# ---------------------------------------------------------------- 2: planted waves
def planted(geom, ptop, mu, mv, phi, lev, row, A=3.0, B=6.0, Cc=2.0):
    """u = A cos(2 pi mu i / W), v = B cos(2 pi mv i / W + phi), theta = Cc cos(2 pi mv i / W) on (lev, row), zero
    elsewhere; p constant, so that T = theta Pi is a pure cosine too"""
    H, W, L = geom.height, geom.width, geom.layers
    i = np.arange(W)
    p = np.full((H, W), 1e5 - ptop)
    u, v, t = np.zeros((L, H, W)), np.zeros((L, H, W)), np.zeros((L, H, W))
    # (m i reduced modulo W in integers: the argument of the cosine then carries a rounding error of 1e-16, not of
    # 1e-16 m i, which at m = W / 2 would move the peak by more than the bound)
    u[lev, row] = A * np.cos(2 * np.pi * (mu * i % W) / W)
    v[lev, row] = B * np.cos(2 * np.pi * (mv * i % W) / W + phi)
    t[lev, row] = Cc * np.cos(2 * np.pi * (mv * i % W) / W)
    return [p, u, v, t, np.zeros((L, H, W))]


def coefficient(W, amp, m, phase):
    """X_m of amp cos(2 pi m i / W + phase): half the amplitude with its phase, and at the Nyquist wavenumber, where the
    wave is cos(phase) (-1)^i, all of it"""
    return W * amp * np.cos(phase) + 0j if 2 * m == W else W * 0.5 * amp * np.exp(1j * phase)


@pytest.mark.parametrize("shape,mu,mv", [((6, 36, 3), 3, 5), ((6, 70, 2), 7, 2), ((4, 300, 2), 11, 150)])
def test_planted_waves_peak_where_they_were_planted(g, shape, mu, mv):
    """float64 only: a cosine rounded to float32 is no pure wave, its rounding noise at the other wavenumbers is 1e-8
    of the peak and no leakage of the transform.  Words 0, 1, 2 and 5 peak at the planted m with the analytic value and
    are at most the bound elsewhere; uv is at most the bound everywhere.  The winds are centred: uc = 0.5 (u[i] + u[i - 1])
    multiplies the coefficient by 0.5 (1 + exp(-2 pi i mu / W)), vc = 0.5 v on the planted row and on the row south of
    it.  The amplitudes of uc and vc, and of T and theta, are of one size: the two rows of a pair are transformed
    together, and a coefficient's error is relative to the larger of the two"""
    H, W, L = shape
    A, B, Cc, phi, lev, row = 3.0, 6.0, 2.0, 0.4, L - 1, 2
    geom = su.geom_of(H, W, L, PTOP)
    st = planted(geom, PTOP, mu, mv, phi, lev, row, A, B, Cc)
    c = su.single(g, geom, st)
    c.set_spectra(1, W // 2)
    c.spectra_sample()
    n, s = c.spectra_sums()
    c.close()
    sig = sig_of(geom)
    r = ref.rows(st[0], st[1], st[2], st[3], sig, PTOP)
    unit, fac = ref.unit(*r), ref.bound_factor(W)
    worst = assert_within_bound(s, ref.products(*r, W // 2), unit, W, shape, at=(lev, row))
    Pi = np.power((sig[lev] * (1e5 - PTOP) + PTOP) / 1e5, ref.clim.KAPPA)
    Uc = coefficient(W, A, mu, 0.0) * (0.5 * (1.0 + np.exp(-2j * np.pi * mu / W)))
    Vc, Th = 0.5 * coefficient(W, B, mv, phi), coefficient(W, Cc, mv, 0.0)
    amp = {0: abs(Uc) ** 2, 1: abs(Vc) ** 2, 2: abs(Pi * Th) ** 2, 5: (Vc * np.conj(Th)).real}
    peak = {0: mu, 1: mv, 2: mv, 5: mv}
    for w in (0, 1, 2, 5):
        bnd = fac[w] * unit[w, lev, row]
        assert abs(s[w, lev, row, peak[w]] - amp[w]) <= bnd, (ref.WORDS[w], s[w, lev, row, peak[w]], amp[w], bnd)
        others = np.delete(s[w, lev, row], peak[w])
        assert np.max(np.abs(others)) <= bnd, (ref.WORDS[w], "leakage", float(np.max(np.abs(others))), bnd)
        assert abs(amp[w]) > 1e6 * bnd                                       # (the bound is eps-small against the peak)
    assert np.max(np.abs(s[3, lev, row])) <= fac[3] * unit[3, lev, row]
    # a row without any wave is exactly zero; the row south of the planted one sees v through its row -1, no T
    off = np.ones((L, H), dtype=bool)
    off[lev, row] = off[lev, row + 1] = False
    assert not s[:, off].any()
    assert abs(s[1, lev, row + 1, mv] - amp[1]) <= fac[1] * unit[1, lev, row + 1] and not s[2, lev, row + 1].any()
    print("planted waves, largest fraction of the bound", shape, worst)


@pytest.mark.parametrize("phi", [0.0, 0.4, 1.5, 2.9])
def test_planted_waves_of_one_wavenumber_follow_the_cosine_law(g, phi):
    """mu = mv = m and a phase shift phi: uc lags u by pi m / W, so uv at m is (W / 2)^2 A cos(pi m / W) (B / 2)
    cos(phi + pi m / W)"""
    H, W, L = 6, 36, 3
    A, B, m, lev, row = 3.0, 6.0, 5, 1, 3
    geom = su.geom_of(H, W, L)
    st = planted(geom, 0.0, m, m, phi, lev, row, A, B)
    c = su.single(g, geom, st)
    c.set_spectra(1, W // 2)
    c.spectra_sample()
    n, s = c.spectra_sums()
    c.close()
    r = ref.rows(st[0], st[1], st[2], st[3], sig_of(geom), 0.0)
    want = ref.products(*r, W // 2)
    bnd = ref.bound_factor(W)[3] * ref.unit(*r)[3, lev, row]
    law = (W * 0.5) ** 2 * A * np.cos(np.pi * m / W) * (0.5 * B) * np.cos(phi + np.pi * m / W)
    assert abs(want[3, lev, row, m] - law) <= bnd and abs(s[3, lev, row, m] - law) <= bnd, (s[3, lev, row, m], law, bnd)
    assert np.max(np.abs(s[3, lev, row] - want[3, lev, row])) <= bnd
    assert np.max(np.abs(np.delete(s[3, lev, row], m))) <= bnd


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_planted_v_in_the_last_row_reaches_row_0_through_the_wrap(g, dtype):
    """v only in row H - 1, theta only in row 0: row H - 1 is row -1 of row 0, so vc of row 0 is 0.5 v[H - 1], and vv
    and vtheta of row 0 are that wave's.  Values a float32 holds exactly at the four points of a wave of W / 4"""
    H, W, L = 6, 36, 3
    B, Cc, m = 3.0, 2.0, 9                                       # cos(2 pi 9 i / 36) = 1, 0, -1, 0, ...
    geom = su.geom_of(H, W, L)
    wave = np.array([1.0, 0.0, -1.0, 0.0] * (W // 4))
    p = np.full((H, W), 1e5)
    u, v, t = np.zeros((L, H, W)), np.zeros((L, H, W)), np.zeros((L, H, W))
    v[:, H - 1] = B * wave * (1.0 + np.arange(L))[:, None]
    t[:, 0] = Cc * wave
    st = [p, u, v, t, np.zeros((L, H, W))]
    c = su.single(g, geom, st, dtype=dtype)
    c.set_spectra(1, W // 2)
    c.spectra_sample()
    n, s = c.spectra_sums()
    c.close()
    r = ref.rows(p, u, v, t, sig_of(geom), 0.0)
    unit, fac = ref.unit(*r), ref.bound_factor(W)
    # (u is zero everywhere: words 1 and 5 are what the restatement is asked about)
    assert_within_bound(s, ref.products(*r, W // 2), unit, W, "wrap", words=(1, 5))
    for k in range(L):
        vv = (W * 0.5 * 0.5 * B * (1.0 + k)) ** 2
        vth = (W * 0.5) ** 2 * (0.5 * B * (1.0 + k)) * Cc
        assert abs(s[1, k, 0, m] - vv) <= fac[1] * unit[1, k, 0] and abs(s[5, k, 0, m] - vth) <= fac[5] * unit[5, k, 0]
        assert abs(s[1, k, H - 1, m] - vv) <= fac[1] * unit[1, k, H - 1]
        assert vv > 1e6 * fac[1] * unit[1, k, 0]
    assert not s[1, :, 1:H - 1].any() and not s[5, :, 1:].any()


# ---------------------------------------------------------------- 3: Parseval against the climatology
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_parseval_against_the_climatology(g, shape, dtype):
    """both registered, one sample each of the same state: sum_m w_m s / W is the climatology's zonal sum of the same
    product, within (8 eps log2 W) B_x B_y -- both sides hold the device's T, no Exner term"""
    H, W, L = shape
    geom = su.geom_of(H, W, L, PTOP)
    st = inp.state_of(geom, dtype)
    c = su.single(g, geom, st, dtype=dtype, every=10 ** 6)
    c.set_spectra(10 ** 6, W // 2)
    c.climate_sample()
    c.spectra_sample()
    n3, m3, m2 = c.climate_sums()
    n, s = c.spectra_sums()
    c.close()
    assert n3 == n == 1
    unit = ref.unit(*ref.rows(st[0], st[1], st[2], st[3], sig_of(geom), PTOP))
    fac = ref.bound_factor(W, exner=False)
    wm = ref.weights(W // 2 + 1, W)
    worst = 0.0
    for w, cw in ref.CLIMATE_WORD.items():
        total = np.sum(s[w] * wm, axis=-1) / W
        ratio = float(np.max(np.abs(total - m3[cw]) / (fac[w] * unit[w])))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (shape, dtype, ref.WORDS[w], ratio)
    print("Parseval, largest fraction of the bound", shape, dtype, worst)


# ---------------------------------------------------------------- 4: registered equals explicit
@pytest.mark.parametrize("hs", [None, {}], ids=["plain", "held-suarez"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_registered_equals_explicit_samples(g, dtype, hs):
    H, W, L = BAND_SHAPE
    geom = su.geom_of(H, W, L)
    st = inp.state_of(geom, dtype)
    a = su.single(g, geom, st, dtype=dtype, hs=hs)
    a.set_spectra(2)
    a.step(5, DT)
    got = a.spectra_sums()
    assert got[0] == 2 and got[1].any()
    state_a = a.get_state()
    b = su.single(g, geom, st, dtype=dtype, hs=hs)
    b.set_spectra(10 ** 6)
    seen = []
    for n, sample in ((2, True), (2, True), (1, False)):
        b.step(n, DT)
        if sample:
            b.spectra_sample()
            seen.append(b.get_state())
    assert_sums_equal(got, b.spectra_sums(), "explicit")
    b.close()
    # ... which are the spectra of the states at the sampling points (with Held-Suarez: the forced states)
    n, want, unit = ref.accumulate(seen, sig_of(geom), 0.0, got[1].shape[-1] - 1)
    print("registered, largest fraction of the bound", dtype, hs, assert_within_bound(got[1], want, unit, W, "registered"))
    # the counter runs across calls, and is the spectra's own: a climatology of another interval beside it
    c = su.single(g, geom, st, dtype=dtype, hs=hs, every=3)
    c.set_spectra(2)
    for _ in range(5):
        c.step(1, DT)
    assert_sums_equal(got, c.spectra_sums(), "step(1) five times")
    assert c.climate_sums()[0] == 1
    c.close()
    # the state is the unregistered run's
    u = su.single(g, geom, st, dtype=dtype, hs=hs)
    u.step(5, DT)
    for k, x, y in zip("puvtq", state_a, u.get_state()):
        assert np.array_equal(x, y), k
    u.close()
    # half steps never sample
    a.half_step(0, DT)
    a.half_step(1, DT)
    assert a.spectra_sums()[0] == 2
    a.close()


# ---------------------------------------------------------------- 5: bands
_single_cache = {}


def single_reference(g, dtype, steps, every, clim=None):
    """the single domain with Held-Suarez and the spectra every `every` steps (clim: the climatology's interval) after
    `steps` steps: (spectra sums, state, climatology sums or None), computed once per case"""
    key = (dtype, steps, every, clim)
    if key not in _single_cache:
        geom = su.geom_of(*BAND_SHAPE)
        c = su.single(g, geom, inp.state_of(geom, dtype), dtype=dtype, hs={}, every=clim)
        c.set_spectra(every)
        c.step(steps, DT)
        sums, state = c.spectra_sums(), c.get_state()
        csums = c.climate_sums() if clim else None
        c.close()
        for a in [sums[1]] + state:
            a.setflags(write=False)
        _single_cache[key] = (sums, state, csums)
    return _single_cache[key]


def merged_sums(cores):
    """merge_spectra of the bands' records, and the raw sums put together the same way"""
    from gcmiipy_amd.bands import merge_spectra
    merged = merge_spectra([c.spectra() for c in cores])
    raw = [c.spectra_sums() for c in cores]
    assert all(r[0] == merged.n for r in raw)
    return merged, (merged.n, np.concatenate([r[1] for r in raw], axis=-2))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_three_in_process_bands_equal_the_single_domain(g, dtype):
    """three bands of 8 rows, whole stages, two exchanges per step, the Held-Suarez forcing on own rows and ghost rows,
    then the sample: every word, vv of each band's first row (which reads the ghost row) included"""
    import torch
    H, W, L = BAND_SHAPE
    steps = 4
    want, want_state, _ = single_reference(g, dtype, steps, 1)
    geom = su.geom_of(H, W, L)
    cores = su.bands(g, geom, 3, inp.state_of(geom, dtype), dtype=dtype)
    for c in cores:
        assert c.H == 8
        c.set_held_suarez(geom)
        c.set_spectra(1)

    def forcing_and_sample(k):
        for c in cores:
            c.held_suarez_step(geom, DT)
            c.spectra_sample()
    su.whole_steps(cores, torch, steps, DT, after=forcing_and_sample)
    merged, raw = merged_sums(cores)
    assert_sums_equal(raw, want, "three bands")
    whole = g.Spectra.from_sums(want[0], want[1], W)
    for f, a, b in zip(g.Spectra._fields[1:], merged[1:], whole[1:]):
        assert np.array_equal(a, b), f
    for c in cores:
        c.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_host_driven_steps_sample_where_due(g, dtype):
    """the same bands, every = 2, each step ended by the host with gcm_end_step_begin / gcm_end_step_finish behind the
    post-corrector exchange: the walk forces own rows and ghost rows, counts the step and samples steps 2 and 4"""
    import torch
    H, W, L = BAND_SHAPE
    want, want_state, _ = single_reference(g, dtype, 4, 2)
    assert want[0] == 2
    geom = su.geom_of(H, W, L)
    cores = su.bands(g, geom, 3, inp.state_of(geom, dtype), dtype=dtype)
    for c in cores:
        c.set_held_suarez(geom)
        c.set_spectra(2)

    def end_of_step(k):
        for c in cores:
            c.end_step_begin(DT)
            c.end_step_finish(DT)
        assert all(c.spectra_sums()[0] == (k + 1) // 2 for c in cores)
    su.whole_steps(cores, torch, 4, DT, after=end_of_step)
    merged, raw = merged_sums(cores)
    assert_sums_equal(raw, want, "host-driven")
    for c in cores:
        c.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_loopback_band_run_equals_the_single_domain(g, dtype):
    import torch
    H, W, L = BAND_SHAPE
    want, want_state, _ = single_reference(g, dtype, 4, 1)
    geom = su.geom_of(H, W, L)
    c, eng, runner = su.loopback_band(g, torch, geom, dtype=dtype, hs={})
    eng.set_spectra(1)
    assert runner.native
    c.set_state(*inp.state_of(geom, dtype))
    runner.run(3, DT)
    runner.run(1, DT)
    torch.cuda.synchronize()
    merged, raw = merged_sums([c])
    assert_sums_equal(raw, want, "loopback")
    for k, x, y in zip("puvtq", c.get_state(), want_state):
        assert np.array_equal(x, y), k
    c.close()


@pytest.mark.parametrize("comm_stream", [False, True], ids=["second-stream", "comm-stream"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_loopback_band_run_with_the_climatology_too(g, dtype, comm_stream, monkeypatch):
    """Held-Suarez, the climatology (every 2) and the spectra (every 2) together on the loopback band, the exchange on
    the library's second stream or (GCM_BAND_COMM_STREAM=1, read by gcm_set_exchange) on the comm stream; 3 + 1 steps,
    so the first run ends between two samples: one join serves both samples, and both are the single domain's"""
    import torch
    H, W, L = BAND_SHAPE
    want, want_state, want_clim = single_reference(g, dtype, 4, 2, clim=2)
    assert want[0] == 2 and want_clim[0] == 2
    geom = su.geom_of(H, W, L)
    if comm_stream:
        monkeypatch.setenv("GCM_BAND_COMM_STREAM", "1")
    else:
        monkeypatch.delenv("GCM_BAND_COMM_STREAM", raising=False)
    c, eng, runner = su.loopback_band(g, torch, geom, dtype=dtype, hs={}, every=2)
    eng.set_spectra(2)
    assert runner.native
    c.set_state(*inp.state_of(geom, dtype))
    runner.run(3, DT)
    runner.run(1, DT)
    torch.cuda.synchronize()
    merged, raw = merged_sums([c])
    assert_sums_equal(raw, want, "loopback with the climatology")
    n3, m3, m2 = c.climate_sums()
    assert n3 == want_clim[0] and np.array_equal(m3, want_clim[1]) and np.array_equal(m2, want_clim[2])
    for k, x, y in zip("puvtq", c.get_state(), want_state):
        assert np.array_equal(x, y), k
    c.close()


# ---------------------------------------------------------------- 6: reset, put / get, checkpoint
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_reset_put_get_and_checkpoint(g, dtype, tmp_path):
    from gcmiipy_amd import checkpoint
    H, W, L = BAND_SHAPE
    geom = su.geom_of(H, W, L)
    st = inp.state_of(geom, dtype)
    whole = su.single(g, geom, st, dtype=dtype, hs={})
    whole.set_spectra(1, 7)
    whole.step(5, DT)
    want = whole.spectra_sums()
    assert want[0] == 5 and want[1].shape == (6, L, H, 8)
    # reset
    whole.spectra_reset()
    n, s = whole.spectra_sums()
    assert n == 0 and not s.any()
    # registering again resets too
    whole.step(1, DT)
    assert whole.spectra_sums()[0] == 1
    whole.set_spectra(3, 7)
    n, s = whole.spectra_sums()
    assert n == 0 and not s.any() and whole.spectra_every == 3
    whole.close()
    # put then get; put then more steps equals the uninterrupted run
    a = su.single(g, geom, st, dtype=dtype, hs={})
    a.set_spectra(1, 7)
    a.step(3, DT)
    mid, mid_state = a.spectra_sums(), a.get_state()
    path = str(tmp_path / "spec.npz")
    checkpoint.save(path, a, step=3, geom=geom)
    a.close()
    b = su.single(g, geom, mid_state, dtype=dtype, hs={})
    b.set_spectra(1, 7)
    b.put_spectra(*mid)
    assert_sums_equal(b.spectra_sums(), mid, "put then get")
    b.step(2, DT)
    assert_sums_equal(b.spectra_sums(), want, "put then steps")
    b.close()
    # a checkpoint in the middle of the run
    r, ck = checkpoint.restore(path)
    assert r.spectra_every == 1 and r.spectra_mmax == 7 and ck["spectra"]["n"] == 3 and ck["spectra"]["mmax"] == 7
    assert_sums_equal(r.spectra_sums(), mid, "restored")
    r.step(2, DT)
    assert_sums_equal(r.spectra_sums(), want, "restored then steps")
    r.close()
    # a handle without spectra writes none of the keys and restores with none
    plain = su.single(g, geom, st, dtype=dtype)
    checkpoint.save(path, plain, geom=geom)
    plain.close()
    assert not any(k.startswith("spectra_") for k in np.load(path).files)
    r, ck = checkpoint.restore(path)
    assert ck["spectra"] is None and r.spectra_every == 0
    r.close()


# ---------------------------------------------------------------- 7: refusals
def test_refusals_change_nothing(g):
    import ctypes as C
    lib, L_ = g._lib.lib, g._lib
    H, W, L = SHAPES[0]
    geom = su.geom_of(H, W, L)
    st = inp.state_of(geom)
    c = su.single(g, geom, st)
    s, n = np.zeros((6, L, H, W // 2 + 1)), C.c_int64(7)
    dp = L_._dp
    # without a registration
    assert c.spectra_every == 0 and lib.gcm_spectra_mmax(c._h) == L_.ERR_STATE
    assert lib.gcm_spectra_sample(c._h) == L_.ERR_STATE and lib.gcm_spectra_reset(c._h) == L_.ERR_STATE
    assert lib.gcm_get_spectra(c._h, s.ctypes.data_as(dp), C.byref(n)) == L_.ERR_STATE
    assert lib.gcm_put_spectra(c._h, s.ctypes.data_as(dp), 1) == L_.ERR_STATE
    assert n.value == 7 and not s.any()
    with pytest.raises(g.GcmError):
        c.spectra()
    for every, mmax in ((-1, 3), (1, W // 2 + 1), (1, -2)):
        assert lib.gcm_set_spectra(c._h, every, mmax) == L_.ERR_ARG and c.spectra_every == 0
    with pytest.raises(ValueError):
        c.set_spectra(-3)
    with pytest.raises(ValueError):
        c.set_spectra(1, W)
    # registered: a refused call leaves the registration and the sums alone
    c.set_spectra(1, 3)
    c.step(2, DT)
    was = c.spectra_sums()
    assert was[0] == 2 and was[1].any()
    for every, mmax in ((-1, 3), (1, W // 2 + 1), (1, -2), (2, W)):
        assert lib.gcm_set_spectra(c._h, every, mmax) == L_.ERR_ARG
        assert c.spectra_every == 1 and c.spectra_mmax == 3
        assert_sums_equal(c.spectra_sums(), was, "after a refused registration")
    assert lib.gcm_put_spectra(c._h, None, 1) == L_.ERR_ARG
    assert lib.gcm_put_spectra(c._h, was[1].ctypes.data_as(dp), -1) == L_.ERR_ARG
    with pytest.raises(ValueError):
        c.put_spectra(1, np.zeros((6, L, H, 5)))
    assert_sums_equal(c.spectra_sums(), was, "after refused calls")
    # null pointers of get are allowed
    assert lib.gcm_get_spectra(c._h, None, C.byref(n)) == L_.OK and n.value == 2
    assert lib.gcm_get_spectra(c._h, None, None) == L_.OK
    # every = 0 unregisters, and the run is the unregistered one's
    c.set_spectra(0)
    assert c.spectra_every == 0
    with pytest.raises(g.GcmError):
        c.spectra()
    c.step(1, DT)
    u = su.single(g, geom, st)
    u.step(3, DT)
    for k, x, y in zip("puvtq", c.get_state(), u.get_state()):
        assert np.array_equal(x, y), k
    c.close()
    u.close()
    # other models
    o = g.Core(L_.SW2D, 32, 16, dx=1e5)
    assert lib.gcm_set_spectra(o._h, 1, -1) == L_.ERR_UNSUPPORTED and lib.gcm_spectra_sample(o._h) == L_.ERR_UNSUPPORTED
    assert lib.gcm_spectra_reset(o._h) == L_.ERR_UNSUPPORTED and lib.gcm_spectra_every(o._h) == 0
    assert lib.gcm_spectra_mmax(o._h) == L_.ERR_UNSUPPORTED
    assert lib.gcm_get_spectra(o._h, None, None) == L_.ERR_UNSUPPORTED
    assert lib.gcm_put_spectra(o._h, s.ctypes.data_as(dp), 1) == L_.ERR_UNSUPPORTED
    o.close()
