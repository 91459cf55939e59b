"""The zonal-mean climatology of GCM_PE25D on the device (gcm_set_climate) against the NumPy restatement
tests/pe25d_climate_ref.py: one sample word by word, planted values at the two wraps, the registered phase against
explicit samples, latitude bands (in-process bands with device-copied ghost rows, the loopback band of gcm_band_run,
and every orchestration switch of the band loop in a child process of its own), reset / put / get / checkpoint and the
refusals.  The words without the Exner routine are bit for bit the restatement's; words 3, 6 and 8 carry the device's
Exner routine against np.power: within 1e-10 sum_i |term|, the project's parity bound applied to a sum."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_setups as su
import pe25d_climate_ref as ref
import pe25d_inputs as inp

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((6, 10, 3), (24, 36, 9), (6, 70, 2), (6, 130, 2), (4, 300, 2))      # (H, W, L)
BAND_SHAPE = (24, 36, 9)
PTOP = 1000.0
UTC0 = inp.UTC0
DT = 120.0
EXACT_WORDS = tuple(w for w in range(10) if w not in ref.EXNER_WORDS)
SWITCHES = ({"GCM_PE_SINGLE_STREAM": "1"}, {"GCM_BAND_COMM_STREAM": "1"}, {"GCM_BAND_OVERLAP": "1"},
            {"GCM_PE_STOP_EVENTS": "0"}, {"GCM_PE_K1_SPLIT": "0"})
CHILD_TIMEOUT = 120                                       # seconds: start-up of a fresh process included


def sig_of(geom):
    return np.asarray(geom.sig, dtype=np.float64).reshape(-1)


def assert_sums_equal(got, want, what=""):
    assert got[0] == want[0], (what, got[0], want[0])
    for w in range(10):
        assert np.array_equal(got[1][w], want[1][w]), (what, "m3 word", w)
    for w in range(2):
        assert np.array_equal(got[2][w], want[2][w]), (what, "m2 word", w)


def assert_sums_match_restatement(got, want, bnd, what=""):
    """got, want: (n, m3, m2); bnd (10, L, H): sum over samples and i of |term|"""
    assert got[0] == want[0], (what, got[0], want[0])
    for w in EXACT_WORDS:
        assert np.array_equal(got[1][w], want[1][w]), (what, "m3 word", w, float(np.max(np.abs(got[1][w] - want[1][w]))))
    for w in range(2):
        assert np.array_equal(got[2][w], want[2][w]), (what, "m2 word", w)
    worst = 0.0
    for w in ref.EXNER_WORDS:
        ratio = float(np.max(np.abs(got[1][w] - want[1][w]) / bnd[w]))
        worst = max(worst, ratio)
        assert ratio <= 1e-10, (what, "m3 word", w, ratio)
    return worst


# ---------------------------------------------------------------- 1: one sample against the restatement
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ptop", [0.0, PTOP])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_sample_equals_the_restatement(shape, ptop, dtype):
    import gcmiipy_amd as g
    H, W, L = shape
    geom = su.geom_of(H, W, L, ptop)
    st = inp.state_of(geom, dtype)
    trs, gt = inp.tracers(H, W, L, 2), inp.ground(H, W)
    c = su.single(g, geom, st, dtype=dtype, gt=gt, every=10 ** 6)
    c.set_tracers(trs)
    trs0 = c.get_tracers()
    assert c.climate_every == 10 ** 6 and c.climate().n == 0
    c.climate_sample()
    got = c.climate_sums()
    m3, m2 = ref.sample(st[0], st[1], st[2], st[3], sig_of(geom), ptop)
    worst = assert_sums_match_restatement(got, (1, m3, m2), ref.bound(st[0], st[1], st[2], st[3], sig_of(geom), ptop), shape)
    print("largest |device - restatement| / sum|term| of the Exner words", shape, ptop, dtype, worst)
    # nothing a step reads has changed
    for k, a, b in zip("puvtq", c.get_state(), st):
        assert np.array_equal(a, b), k
    assert np.array_equal(c.get_tracers(), trs0) and np.array_equal(c.get_ground(), gt)
    # a second read returns the same bits, and the record is the sums over W n
    assert_sums_equal(c.climate_sums(), got, "second read")
    rec = c.climate()
    assert rec.n == 1 and np.array_equal(rec.u, got[1][0] / np.float64(W)) and np.array_equal(rec.pp, got[2][1] / np.float64(W))
    c.close()


# ---------------------------------------------------------------- 2: planted values at the two wraps
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_planted_values_at_the_wraps(dtype):
    """u nonzero only at (L - 1, H - 1, W - 1), v nonzero only in row H - 1 at i = 0.  The i wrap: uc at i = 0 takes
    u[W - 1], so word 7 of (L - 1, H - 1) is exactly that one product, and exactly 0 everywhere else -- row 0 included,
    where u is zero.  The j wrap: row H - 1 is row -1 of row 0, so vc of row 0 is 0.5 v[H - 1] at i = 0 and word 9 of
    row 0 exactly that times theta"""
    import gcmiipy_amd as g
    H, W, L = 6, 10, 3
    geom = su.geom_of(H, W, L)
    st = inp.state_of(geom, dtype)
    u, v = np.zeros((L, H, W)), np.zeros((L, H, W))
    u[L - 1, H - 1, W - 1] = 6.0
    v[:, H - 1, 0] = 3.0 + np.arange(L)
    st = [st[0], u, v, st[3], st[4]]
    c = su.single(g, geom, st, dtype=dtype, every=1)
    c.climate_sample()
    n, m3, m2 = c.climate_sums()
    c.close()
    want7 = np.zeros((L, H))
    want7[L - 1, H - 1] = (0.5 * (0.0 + 6.0)) * (0.5 * (3.0 + (L - 1) + 0.0))       # uc[i = 0] vc[i = 0]
    assert np.array_equal(m3[7], want7), m3[7]
    # row 0 reads row H - 1 as its row -1: vc = 0.5 (0 + v[H - 1]) at i = 0
    th = st[3]
    want9 = np.zeros((L, H))
    want9[:, 0] = (0.5 * v[:, H - 1, 0]) * th[:, 0, 0]
    want9[:, H - 1] = (0.5 * v[:, H - 1, 0]) * th[:, H - 1, 0]
    assert np.array_equal(m3[9], want9), m3[9]
    assert np.array_equal(m3[1][:, H - 1], v[:, H - 1, 0]) and not m3[1][:, :H - 1].any()
    assert m3[0][L - 1, H - 1] == 6.0 and m3[4][L - 1, H - 1] == 36.0
    # and the restatement says the same
    r3, _ = ref.sample(st[0], u, v, st[3], sig_of(geom), 0.0)
    assert np.array_equal(m3[7], r3[7]) and np.array_equal(m3[9], r3[9])


# ---------------------------------------------------------------- 3: registered equals explicit
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_registered_equals_explicit_samples(dtype):
    import gcmiipy_amd as g
    H, W, L = BAND_SHAPE
    geom = su.geom_of(H, W, L)
    st = inp.state_of(geom, dtype)
    a = su.single(g, geom, st, dtype=dtype, every=2)
    a.step(5, DT)
    got = a.climate_sums()
    assert got[0] == 2
    state_a = a.get_state()
    b = su.single(g, geom, st, dtype=dtype, every=10 ** 6)
    for n, sample in ((2, True), (2, True), (1, False)):
        b.step(n, DT)
        if sample:
            b.climate_sample()
    assert_sums_equal(got, b.climate_sums(), "explicit")
    b.close()
    # the counter runs across calls
    c = su.single(g, geom, st, dtype=dtype, every=2)
    for _ in range(5):
        c.step(1, DT)
    assert_sums_equal(got, c.climate_sums(), "step(1) five times")
    c.close()
    # the state is the unregistered run's
    u = su.single(g, geom, st, dtype=dtype)
    u.step(5, DT)
    for k, x, y in zip("puvtq", state_a, u.get_state()):
        assert np.array_equal(x, y), k
    u.close()
    # half steps never sample
    a.half_step(0, DT)
    a.half_step(1, DT)
    assert a.climate_sums()[0] == 2
    a.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_registered_sample_sees_the_forced_state(dtype):
    """physics and Held-Suarez registered as well: the sample is the last phase.  The states at the sampling points,
    taken from an identical run, go through the restatement"""
    import gcmiipy_amd as g
    H, W, L = BAND_SHAPE
    geom = su.geom_of(H, W, L)
    st, gt = inp.state_of(geom, dtype), inp.ground(H, W)
    a = su.single(g, geom, st, dtype=dtype, gt=gt, phys=True, hs={}, every=2)
    a.step(5, DT)
    got = a.climate_sums()
    state_a = a.get_state()
    a.close()
    b = su.single(g, geom, st, dtype=dtype, gt=gt, phys=True, hs={})
    seen = []
    for n in (2, 2, 1):
        b.step(n, DT)
        seen.append(b.get_state())
    for k, x, y in zip("puvtq", state_a, seen[-1]):
        assert np.array_equal(x, y), k
    b.close()
    sig = sig_of(geom)
    want = ref.accumulate(seen[:2], sig, 0.0)
    bnd = sum(ref.bound(s[0], s[1], s[2], s[3], sig, 0.0) for s in seen[:2])
    worst = assert_sums_match_restatement(got, want, bnd, "forced")
    print("largest ratio of the Exner words, forced state", dtype, worst)
    # the unforced run's samples are other numbers
    plain = su.single(g, geom, st, dtype=dtype, every=2)
    plain.step(5, DT)
    assert not np.array_equal(plain.climate_sums()[1][2], got[1][2])
    plain.close()


# ---------------------------------------------------------------- 4: bands
_single_cache = {}


def single_reference(g, shape, dtype, steps, dt=DT):
    """the single domain with Held-Suarez and every = 1 after `steps` steps: (sums, state), computed once per case"""
    key = (shape, dtype, steps, dt)
    if key not in _single_cache:
        geom = su.geom_of(*shape)
        c = su.single(g, geom, inp.state_of(geom, dtype), dtype=dtype, hs={}, every=1)
        c.step(steps, dt)
        sums, state = c.climate_sums(), c.get_state()
        c.close()
        for a in list(sums[1:]) + state:
            a.setflags(write=False)
        _single_cache[key] = (sums, state)
    return _single_cache[key]


def merged_sums(cores):
    """merge_climate of the bands' records, and the raw sums put together the same way"""
    from gcmiipy_amd.bands import merge_climate
    merged = merge_climate([c.climate() for c in cores])
    raw = [c.climate_sums() for c in cores]
    assert all(r[0] == merged.n for r in raw)
    return merged, (merged.n, np.concatenate([r[1] for r in raw], axis=-1), np.concatenate([r[2] for r in raw], axis=-1))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_three_in_process_bands_equal_the_single_domain(dtype):
    """three bands of 8 rows, whole stages, two exchanges per step, the Held-Suarez forcing on own rows and ghost rows,
    then the sample: every word, word 7 of each band's first row (which reads the ghost row) included"""
    import torch
    import gcmiipy_amd as g
    from gcmiipy_amd import Climate
    H, W, L = BAND_SHAPE
    steps = 4
    want, want_state = single_reference(g, BAND_SHAPE, dtype, steps)
    geom = su.geom_of(H, W, L)
    cores = su.bands(g, geom, 3, inp.state_of(geom, dtype), dtype=dtype)
    for c in cores:
        assert c.H == 8
        c.set_held_suarez(geom)
        c.set_climate(1)

    def forcing_and_sample(k):
        for c in cores:
            c.held_suarez_step(geom, DT)
            c.climate_sample()
    su.whole_steps(cores, torch, steps, DT, after=forcing_and_sample)
    merged, raw = merged_sums(cores)
    assert_sums_equal(raw, want, "three bands")
    whole = Climate.from_sums(want[0], want[1], want[2], W)
    for f, a, b in zip(Climate._fields[1:], merged[1:], whole[1:]):
        assert np.array_equal(a, b), f
    for c in cores:
        c.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_loopback_band_run_equals_the_single_domain(dtype):
    import torch
    import gcmiipy_amd as g
    H, W, L = BAND_SHAPE
    want, want_state = single_reference(g, BAND_SHAPE, dtype, 4)
    geom = su.geom_of(H, W, L)
    c, eng, runner = su.loopback_band(g, torch, geom, dtype=dtype, hs={}, every=1)
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


_three_phase_cache = {}


def three_phase_reference(g, dtype):
    """the single domain with physics, Held-Suarez and every = 2 after step(4): (sums, state, ground, utc), once per type"""
    if dtype not in _three_phase_cache:
        H, W, L = BAND_SHAPE
        geom = su.geom_of(H, W, L)
        c = su.single(g, geom, inp.state_of(geom, dtype), dtype=dtype, gt=inp.ground(H, W), phys=True, hs={}, every=2)
        c.step(4, DT)
        sums, state, gt, utc = c.climate_sums(), c.get_state(), c.get_ground(), c.utc()
        c.close()
        for a in list(sums[1:]) + state + [gt]:
            a.setflags(write=False)
        _three_phase_cache[dtype] = (sums, state, gt, utc)
    return _three_phase_cache[dtype]


@pytest.mark.parametrize("comm_stream", [False, True], ids=["second-stream", "comm-stream"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_loopback_band_run_with_all_three_phases(dtype, comm_stream, monkeypatch):
    """physics, Held-Suarez and the climatology registered together on the loopback band of gcm_band_run, the exchange on
    the library's second stream or (GCM_BAND_COMM_STREAM=1, read by gcm_set_exchange) on the comm stream; 3 + 1 steps
    with every = 2, so the first run ends between two samples.  State, ground temperature, clock and sums are the single
    domain's after step(4), bit for bit"""
    import torch
    import gcmiipy_amd as g
    H, W, L = BAND_SHAPE
    want, want_state, want_gt, want_utc = three_phase_reference(g, dtype)
    assert want[0] == 2 and want_utc == UTC0 + 4 * DT
    geom = su.geom_of(H, W, L)
    if comm_stream:
        monkeypatch.setenv("GCM_BAND_COMM_STREAM", "1")
    else:
        monkeypatch.delenv("GCM_BAND_COMM_STREAM", raising=False)
    c, eng, runner = su.loopback_band(g, torch, geom, dtype=dtype, gt=inp.ground(H, W), phys=True, hs={}, every=2)
    assert runner.native
    c.set_state(*inp.state_of(geom, dtype))
    runner.run(3, DT)
    runner.run(1, DT)
    torch.cuda.synchronize()
    merged, raw = merged_sums([c])
    assert_sums_equal(raw, want, "loopback, three phases")
    for k, x, y in zip("puvtq", c.get_state(), want_state):
        assert np.array_equal(x, y), k
    assert np.array_equal(c.get_ground(), want_gt)
    assert c.utc() == want_utc
    c.close()


def test_band_run_under_every_switch_in_child_processes(tmp_path):
    """the loopback band at 48 x 1440 x 24 (kernels of tens of microseconds on either stream), Held-Suarez registered,
    every = 1, 4 steps, both real types, once per orchestration switch: each run in a fresh process under its own time
    limit (tests/pe25d_climate_child.py), compared bit for bit with the single domain's sums computed here.  A child
    that faults or runs into its limit ends the test: nothing more is started"""
    import gcmiipy_amd as g
    shape, steps, dt = (48, 1440, 24), 4, 1.0
    path = str(tmp_path / "want.npz")
    out = {}
    for dtype in ("f64", "f32"):
        (n, m3, m2), state = single_reference(g, shape, dtype, steps, dt)
        out.update({"n_" + dtype: n, "m3_" + dtype: m3, "m2_" + dtype: m2, "u_" + dtype: state[1]})
    np.savez(path, **out)
    child = os.path.join(HERE, "pe25d_climate_child.py")
    for switch in ({},) + SWITCHES:
        env = {k: v for k, v in os.environ.items() if k not in {s for sw in SWITCHES for s in sw}}
        env.update(switch)
        try:
            r = subprocess.run([sys.executable, child, path, str(steps), str(dt)], env=env, capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.fail("the child under %r did not end within %d s" % (switch, CHILD_TIMEOUT))
        print(switch, r.returncode, r.stdout.strip()[-400:])
        if r.returncode < 0 or r.returncode in (134, 139):
            pytest.fail("the child under %r faulted (status %d): %s" % (switch, r.returncode, r.stderr[-2000:]))
        assert r.returncode == 0, (switch, r.returncode, r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------- 5: reset, put / get, refusals
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_reset_put_get_and_checkpoint(dtype, tmp_path):
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    H, W, L = BAND_SHAPE
    geom = su.geom_of(H, W, L)
    st = inp.state_of(geom, dtype)
    whole = su.single(g, geom, st, dtype=dtype, hs={}, every=1)
    whole.step(5, DT)
    want = whole.climate_sums()
    assert want[0] == 5
    # reset
    whole.climate_reset()
    n, m3, m2 = whole.climate_sums()
    assert n == 0 and not m3.any() and not m2.any()
    # registering again resets too
    whole.step(1, DT)
    assert whole.climate_sums()[0] == 1
    whole.set_climate(3)
    n, m3, m2 = whole.climate_sums()
    assert n == 0 and not m3.any() and whole.climate_every == 3
    whole.close()
    # put then get; put then more steps equals the uninterrupted run
    a = su.single(g, geom, st, dtype=dtype, hs={}, every=1)
    a.step(3, DT)
    mid, mid_state = a.climate_sums(), a.get_state()
    path = str(tmp_path / "clim.npz")
    checkpoint.save(path, a, step=3, geom=geom)
    a.close()
    b = su.single(g, geom, mid_state, dtype=dtype, hs={}, every=1)
    b.put_climate(*mid)
    assert_sums_equal(b.climate_sums(), mid, "put then get")
    b.step(2, DT)
    assert_sums_equal(b.climate_sums(), want, "put then steps")
    b.close()
    # a checkpoint in the middle of the run
    r, ck = checkpoint.restore(path)
    assert r.climate_every == 1 and ck["climate"]["n"] == 3
    assert_sums_equal(r.climate_sums(), mid, "restored")
    r.step(2, DT)
    assert_sums_equal(r.climate_sums(), want, "restored then steps")
    r.close()
    # a file without the keys restores without a climatology
    plain = su.single(g, geom, st, dtype=dtype)
    checkpoint.save(path, plain, geom=geom)
    plain.close()
    r, ck = checkpoint.restore(path)
    assert ck["climate"] is None and r.climate_every == 0
    r.close()


def test_refusals_change_nothing():
    import ctypes as C
    import gcmiipy_amd as g
    lib, L_ = g._lib.lib, g._lib
    H, W, L = SHAPES[0]
    geom = su.geom_of(H, W, L)
    st = inp.state_of(geom)
    c = su.single(g, geom, st)
    m3, m2, n = np.zeros((10, L, H)), np.zeros((2, H)), C.c_int64(7)
    dp = L_._dp
    # without a registration
    assert c.climate_every == 0
    assert lib.gcm_climate_sample(c._h) == L_.ERR_STATE and lib.gcm_climate_reset(c._h) == L_.ERR_STATE
    assert lib.gcm_get_climate(c._h, m3.ctypes.data_as(dp), m2.ctypes.data_as(dp), C.byref(n)) == L_.ERR_STATE
    assert lib.gcm_put_climate(c._h, m3.ctypes.data_as(dp), m2.ctypes.data_as(dp), 1) == L_.ERR_STATE
    assert n.value == 7
    with pytest.raises(g.GcmError):
        c.climate()
    assert lib.gcm_set_climate(c._h, -1) == L_.ERR_ARG and c.climate_every == 0
    with pytest.raises(ValueError):
        c.set_climate(-3)
    # registered: a refused call leaves the sums alone
    c.set_climate(1)
    c.step(2, DT)
    was = c.climate_sums()
    assert lib.gcm_set_climate(c._h, -1) == L_.ERR_ARG and c.climate_every == 1
    assert lib.gcm_put_climate(c._h, None, m2.ctypes.data_as(dp), 1) == L_.ERR_ARG
    assert lib.gcm_put_climate(c._h, m3.ctypes.data_as(dp), m2.ctypes.data_as(dp), -1) == L_.ERR_ARG
    with pytest.raises(ValueError):
        c.put_climate(1, np.zeros((10, L, H + 1)), m2)
    assert_sums_equal(c.climate_sums(), was, "after refused calls")
    # null pointers of get are allowed
    assert lib.gcm_get_climate(c._h, None, None, C.byref(n)) == L_.OK and n.value == 2
    assert lib.gcm_get_climate(c._h, None, None, None) == L_.OK
    # every = 0 unregisters
    c.set_climate(0)
    assert c.climate_every == 0
    with pytest.raises(g.GcmError):
        c.climate()
    c.step(1, DT)
    u = su.single(g, geom, st)
    u.step(3, DT)
    for k, x, y in zip("puvtq", c.get_state(), u.get_state()):
        assert np.array_equal(x, y), k
    c.close()
    u.close()
    # other models
    s = g.Core(L_.SW2D, 32, 16, dx=1e5)
    assert lib.gcm_set_climate(s._h, 1) == L_.ERR_UNSUPPORTED and lib.gcm_climate_sample(s._h) == L_.ERR_UNSUPPORTED
    assert lib.gcm_climate_reset(s._h) == L_.ERR_UNSUPPORTED and lib.gcm_climate_every(s._h) == 0
    assert lib.gcm_get_climate(s._h, None, None, None) == L_.ERR_UNSUPPORTED
    assert lib.gcm_put_climate(s._h, m3.ctypes.data_as(dp), m2.ctypes.data_as(dp), 1) == L_.ERR_UNSUPPORTED
    s.close()
