"""The launch geometries of the GCM_PE25D dynamics stage that the product grids take and the suite's small shapes do
not, against the float64 oracle: K1's workgroups that loop over two and more level pairs (the prefetch behind the
first pass, the swapped register sets, the LDS row's reuse, an odd L's single-level pair behind a prefetch) in every
looping instantiation, fp64 and fp32, and K4 in 7-row workgroups with a second column tile, every remainder of the row
groups, the 400 / 401 rule, a band's two-range edge launch in level segments and a band's row0.  The cases and what each
is there for: tests/pe25d_stage_geometry_cases.py; tests/test_pe25d_stage_geometry_cpu.py shows that they reach what
they claim.  Every test first asserts its geometry from Core.stage_plan().  Errors are L-inf over max|reference|;
every figure is printed before it is asserted."""
import numpy as np
import pytest

from conftest import rel_err
import gpu_setups as su
import pe25d_inputs as inp
import pe25d_stage_geometry_cases as sc
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)
from test_pe25d_variants_gpu import F32_PT, F32_STEP, F32_TAP, TOL, _tap

pytestmark = pytest.mark.gpu
DT = sc.DT
TAPS = ("spu", "pit", "p_n", "phi", "pgfu")
SWITCHES = ("GCM_PE_UPDATE_ROWS", "GCM_PE_K4_ODDTOP", "GCM_PE_FILTER_NO_LOOP", "GCM_PE_EDGE_SEGMENTS", "GCM_PE_PIT2D",
            "GCM_PE_LEVEL_SEGMENTS")
# fp32 bounds of a case beside the project's F32_TAP / F32_STEP / F32_PT: {(shape, key): bound}, key a tap's name or
# "step<n>_<field>"; each is 3x the error measured against the float64 oracle (profiles/stage_geometry/README.md holds
# the measurements), and stands only where the locality check passes.  Every tap, p, u, v and q stay within the
# project's bounds at every case; theta does not: F32_PT = 2e-7 is the value measured for theta after one step at
# 4 rows, with no margin, and the bound of ONE step -- here theta after one step measures 1.9e-7 to 2.2e-7 and after
# two steps 2.6e-7 to 3.6e-7 (three to five float32 roundings of theta over max|theta|)
F32_CASE_BOUNDS = {
    ((401, 30, 5), "step1_t"): 6.5e-7, ((768, 60, 6), "step1_t"): 6.1e-7, ((768, 600, 3), "step1_t"): 6.1e-7,
    ((768, 1000, 3), "step1_t"): 6.1e-7, ((768, 1458, 3), "step1_t"): 6.0e-7, ((768, 1440, 3), "step1_t"): 6.0e-7,
    ((768, 30, 5), "step2_t"): 7.8e-7, ((401, 30, 5), "step2_t"): 1.1e-6, ((400, 360, 7), "step2_t"): 1.0e-6,
    ((420, 30, 12), "step2_t"): 8.6e-7, ((768, 60, 6), "step2_t"): 1.0e-6, ((420, 80, 9), "step2_t"): 8.4e-7,
    ((512, 120, 13), "step2_t"): 8.7e-7, ((768, 256, 4), "step2_t"): 8.5e-7, ((768, 600, 3), "step2_t"): 9.9e-7,
    ((768, 1000, 3), "step2_t"): 9.2e-7, ((768, 1458, 3), "step2_t"): 9.5e-7, ((768, 1440, 3), "step2_t"): 9.9e-7,
}


def _core(g, case, geom, dtype, **kw):
    H, W, L = case.shape
    return g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype=dtype, coriolis=case.setup.get("coriolis", False), **kw)


def _clear(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


class Findings:
    """figures printed as they come, the misses collected and asserted together at the end of the test"""

    def __init__(self, what):
        self.what, self.bad = what, []

    def hold(self, name, value, bound, above=False):
        ok = value > bound if above else value < bound
        print(self.what, name, "%.3e" % value, ">" if above else "<", "%.3e" % bound, "" if ok else "MISS")
        if not ok:
            self.bad.append((name, value, bound))

    def done(self):
        assert not self.bad, (self.what, self.bad)


def _bounds(case, dtype):
    """-> (the taps' bounds, {step: {field: bound}} of steps 1 and 2, the increments' bound or None)"""
    if dtype == "f64":
        return {k: TOL for k in TAPS}, {n: {k: TOL for k in "puvtq"} for n in (1, 2)}, 1e-6
    tap = {k: F32_CASE_BOUNDS.get((case.shape, k), F32_TAP[k]) for k in TAPS}
    step = {n: {k: F32_CASE_BOUNDS.get((case.shape, "step%d_%s" % (n, k)), F32_PT if k in "pt" else F32_STEP) for k in "puvtq"}
            for n in (1, 2)}
    return tap, step, None


def _locality(f, case, field, got, want, pl, names):
    """the worst error over each region within the factor of the worst error over all other cells, and the other way
    round: rounding is everywhere, a geometry bug sits in particular cells.  Where the worst error anywhere is the last
    bit of the largest value (fp64 p: most cells have the oracle's bits, a few differ by one ulp) every cell is right or
    off by that bit and a ratio of worst errors says nothing: the figure is printed, no ratio is held"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    ulp = float(np.spacing(np.max(np.abs(want))))
    for name, mask in sc.regions(case.shape, pl).items():
        if name not in names:
            continue
        inside, outside = sc.region_ratio(err, mask)
        if max(inside, outside) <= ulp:
            print(f.what, "locality %s %s: worst error %.3e in, %.3e out, one ulp %.3e: the last bit, no ratio" %
                  (field, name, inside, outside, ulp))
            continue
        up, down = sc.locality_factors(case, field, mask)
        f.hold("locality %s %s in/out" % (field, name), inside / outside if outside > 0 else np.inf, up)
        f.hold("locality %s %s out/in" % (field, name), outside / inside if inside > 0 else np.inf, down)


def _taps(f, c, g, case, dtype, ref, pl, tap_tol):
    got = _tap(c, g)
    # the filter matters: a pair that is skipped fails
    f.hold("filter changes spu", rel_err(ref.tap["spu"], ref.unfiltered), 1e3 * tap_tol["spu"], above=True)
    for k in TAPS:
        f.hold("tap " + k, rel_err(got[k], ref.tap[k]), tap_tol[k])
    _locality(f, case, "spu", got["spu"], ref.tap["spu"], pl, ("k1_last_pair",))


def _steps(f, c, case, dtype, ref, pl, step_tol, inc_tol):
    c.half_step(1, DT)
    for n, want in ((1, ref.step1), (2, ref.step2)):
        if n == 2:
            c.step(1, DT)
        got = c.get_state()
        for k, x, y, z in zip("puvtq", got, want, ref.st if n == 1 else ref.step1):
            f.hold("step %d %s" % (n, k), rel_err(x, y), step_tol[n][k])
            if inc_tol is not None:
                f.hold("step %d increment %s" % (n, k), rel_err(x - z, y - z), inc_tol)
        if n == 1:
            for k in "put":
                i = "puvtq".index(k)
                _locality(f, case, k, got[i], want[i], pl, ("k1_last_pair", "k4_last_group", "k4_last_tile") if k != "p" else
                          ("k4_last_group", "k4_last_tile"))


# ---------------------------------------------------------------- 1. every case, both real types
@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_case_vs_oracle(g, case, dtype, monkeypatch):
    _clear(monkeypatch)
    geom, _ = sc.geoms(case)
    ref, pl = sc.refs(case, dtype), sc.plan(case, dtype)
    tap_tol, step_tol, inc_tol = _bounds(case, dtype)
    c = _core(g, case, geom, dtype)
    assert c.stage_plan() == pl, case.what
    assert pl["k1_pairs_per_wg"] >= 2
    f = Findings((sc.case_id(case), dtype))
    c.set_state(*ref.st)
    c.half_step(0, DT)
    _taps(f, c, g, case, dtype, ref, pl, tap_tol)
    if case.full:
        _steps(f, c, case, dtype, ref, pl, step_tol, inc_tol)
    c.close()
    f.done()


# ---------------------------------------------------------------- 2. the same bits from another geometry
SETTINGS = {"noloop": {"GCM_PE_FILTER_NO_LOOP": "1"}, "rows3": {"GCM_PE_UPDATE_ROWS": "3"}, "oddtop0": {"GCM_PE_K4_ODDTOP": "0"}}
# the settings whose state must equal the default run's bit for bit at every case (see profiles/stage_geometry/README.md
# and SAME_BITS_AS_DEFAULT of test_pe25d_switches_gpu.py); the others are held to the oracle at TOL
SAME_BITS = {"rows3", "oddtop0"}


def _two_steps(g, case, geom, st, want_plan=None):
    c = _core(g, case, geom, "f64")
    pl = c.stage_plan()
    if want_plan is not None:
        assert pl == want_plan
    c.set_state(*st)
    c.step(2, DT)
    out = c.get_state()
    c.close()
    return pl, out


@pytest.mark.parametrize("case", [c for c in sc.CASES if c.full], ids=sc.case_id)
def test_switches_vs_oracle_and_default_bits(g, case, monkeypatch):
    """two fp64 steps with K1 as one workgroup per pair, with 3-row K4 and with K4's march started on an even level:
    each against the oracle at TOL, and whether it reproduces the default geometry's bits"""
    _clear(monkeypatch)
    geom, _ = sc.geoms(case)
    ref, default_plan = sc.refs(case, "f64"), sc.plan(case, "f64")
    _, default = _two_steps(g, case, geom, ref.st, default_plan)
    f = Findings((sc.case_id(case), "switches"))
    for name, env in SETTINGS.items():
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        pl, got = _two_steps(g, case, geom, ref.st)
        _clear(monkeypatch)
        want_plan = dict(default_plan)
        if name == "noloop":
            want_plan.update(k1_loop=0, k1_maxr=0, k1_mask=0, k1_nin=0, k1_nw=0, k1_workgroups_per_row=(case.shape[2] + 1) // 2,
                             k1_pairs_per_wg=1, k1_pairs_last_wg=1, k1_pit_rides=0)
        elif name == "rows3":
            want_plan.update(k4_rows=3, k4_groups=case.k4_f32[1], k4_rows_last_group=case.k4_f32[2],
                             k4_grid=sc.k4_grid(case.k4_f32[1], case.tiles[0]))
        else:
            want_plan.update(k4_oddtop=0)
        assert pl == want_plan, name
        same = all(np.array_equal(a, b) for a, b in zip(got, default))
        print(sc.case_id(case), name, "the default's bits" if same else "differs from the default",
              "(the default's own geometry)" if pl == default_plan else "")
        for k, x, y in zip("puvtq", got, ref.step2):
            f.hold("%s step 2 %s" % (name, k), rel_err(x, y), TOL)
        if name in SAME_BITS:
            for k, a, b in zip("puvtq", got, default):
                assert np.array_equal(a, b), (case.shape, name, k)
    f.done()


# ---------------------------------------------------------------- 3. pit from the 3-D fields
def test_pit_from_3d_fields_vs_oracle(g, monkeypatch):
    """GCM_PE_PIT2D=0: K1 has no pit workgroup (pit_block = -1), pit comes from pe_pit_kernel"""
    _clear(monkeypatch)
    case = sc.case_of(sc.PIT3D_CASE)
    geom, _ = sc.geoms(case)
    ref = sc.refs(case, "f64")
    pl = dict(sc.plan(case, "f64"), k1_pit_rides=0)
    monkeypatch.setenv("GCM_PE_PIT2D", "0")
    c = _core(g, case, geom, "f64")
    _clear(monkeypatch)
    assert c.stage_plan() == pl and c.stage_plan()["k1_pit_rides"] == 0
    tap_tol, step_tol, inc_tol = _bounds(case, "f64")
    f = Findings((sc.case_id(case), "pit3d"))
    c.set_state(*ref.st)
    c.half_step(0, DT)
    _taps(f, c, g, case, "f64", ref, pl, tap_tol)
    _steps(f, c, case, "f64", ref, pl, step_tol, inc_tol)
    c.close()
    f.done()


# ---------------------------------------------------------------- 4. bands
def _band_state(shape, dtype):
    H, W, L = shape
    geom = su.geom_of(H, W, L)
    st = inp.state(geom, H + W + L)
    return geom, (tuple(sc.f32(x) for x in st) if dtype == "f32" else st)


_single = {}


def _single_domain(g, shape, dtype, nsteps):
    key = (shape, dtype, nsteps)
    if key not in _single:
        geom, st = _band_state(shape, dtype)
        c = su.single(g, geom, st, dtype=dtype)
        c.step(nsteps, DT)
        _single[key] = c.get_state()
        c.close()
    return _single[key]


@pytest.mark.parametrize("edge_segments", [None, "1"])
@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_loopback_band_equals_single_domain(g, dtype, edge_segments, monkeypatch):
    """the 420 x 30 x 12 loopback band of gcm_band_run, three steps: K4 in 7-row workgroups (fp64) over the two-range
    edge launch and the interior launch, the edge rows in two level segments (and in one), the split K1's own rows at 3
    pairs per workgroup -- the single domain's bits"""
    import torch
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange
    _clear(monkeypatch)
    H, W, L = shape = sc.BAND_CASE
    nsteps = 3
    want = _single_domain(g, shape, dtype, nsteps)
    geom, st = _band_state(shape, dtype)
    if edge_segments is not None:
        monkeypatch.setenv("GCM_PE_EDGE_SEGMENTS", edge_segments)
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0, dtype=dtype,
               stream=torch.cuda.current_stream().cuda_stream)
    _clear(monkeypatch)
    pl = c.stage_plan()
    print(shape, dtype, edge_segments, pl)
    R = 7 if dtype == "f64" else 3
    nseg_edge = 2 if edge_segments is None else 1
    int_groups, int_last = ((60, 3) if R == 7 else (139, 2))                      # 416 interior rows
    assert (pl["band"], pl["k4_rows"], pl["k4_nseg"], pl["k4_oddtop"]) == (1, R, 1, 1)
    assert (pl["k1_loop"], pl["k1_pit_rides"], pl["k1_pairs_per_wg"]) == (1, 1, 3)
    assert (pl["k1_split"], pl["k1_own_workgroups_per_row"], pl["k1_own_pairs_per_wg"], pl["k1_own_pairs_last_wg"]) == (1, 2, 3, 3)
    assert (pl["k4_edge_groups"], pl["k4_edge_rows_last_group"], pl["nseg_edge"]) == (2, 2, nseg_edge)
    assert pl["k4_edge_oddtop"] == (1 if nseg_edge == 1 else 0) and pl["k4_edge_grid"] == sc.k4_grid(2, 1, nseg_edge)
    assert (pl["k4_int_groups"], pl["k4_int_rows_last_group"], pl["k4_int_oddtop"]) == (int_groups, int_last, 1)
    assert pl["k4_int_grid"] == sc.k4_grid(int_groups, 1)
    runner = BandRunner(HipBandEngine(c, torch), 0, 2, LoopbackExchange(), north=0, south=0)
    assert runner.native
    c.set_state(*st)
    runner.run(nsteps, DT)
    torch.cuda.synchronize()
    got = c.get_state()
    c.close()
    assert not np.array_equal(got[1], st[1])
    for k, a, b in zip("puvtq", got, want):
        assert np.array_equal(a, b), (dtype, edge_segments, k)


@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_two_bands_equal_single_domain(g, dtype, monkeypatch):
    """two in-process bands of 421 rows each, whole stages, two steps: 7-row K4 (fp64) at a non-zero row0, and the pole
    row alone in the second band's last row group -- the single domain's bits"""
    import torch
    _clear(monkeypatch)
    H, W, L = shape = sc.TWO_BANDS
    nsteps = 2
    want = _single_domain(g, shape, dtype, nsteps)
    geom, st = _band_state(shape, dtype)
    cores = su.bands(g, geom, 2, st, dtype=dtype)
    R = 7 if dtype == "f64" else 3
    for c in cores:
        pl = c.stage_plan()
        assert (pl["k4_rows"], pl["k4_groups"], pl["k4_rows_last_group"]) == ((7, 61, 1) if R == 7 else (3, 141, 1)), pl
        assert (pl["k1_loop"], pl["k1_workgroups_per_row"], pl["k1_pairs_per_wg"], pl["k1_pairs_last_wg"]) == (1, 2, 2, 1)
        assert pl["band"] == 1 and pl["k4_oddtop"] == 0
    su.whole_steps(cores, torch, nsteps, DT)
    parts = [c.get_state() for c in cores]
    for c in cores:
        c.close()
    for i, k in enumerate("puvtq"):
        got = np.concatenate([x[i] for x in parts], axis=0 if i == 0 else 1)
        assert np.array_equal(got, want[i]), (dtype, k)
