"""GPU checks of the fp32 2-D handles (gcm_config.dtype = GCM_F32 on GCM_SW2D / GCM_SW2D_TEMP): the state is
float32 on the device, a step stays within a measured bound of the float64 oracle run on the same float32
inputs, mass and tracer are conserved to fp32 rounding, and ensembles, latitude bands, snapshots, checkpoints
and half steps reproduce the fp32 single domain bit for bit."""
import numpy as np
import pytest

from conftest import rel_err
import gpu_setups as su
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu
DX, DT = 300e3, 300.0

# (name, model, tracer): SW2D and SW2D_TEMP with every tracer scheme
MODELS = [("sw2d", 1, 0), ("temp", 2, 0), ("temp_upwind", 2, 1), ("temp_vanleer", 2, 2)]

# fp32 against the float64 oracle on the same (float32-rounded) inputs: rel_err (L-inf over max|ref|) per field
# and per step, by model (1 = GCM_SW2D, 2 = GCM_SW2D_TEMP); a run of n steps is held to n x F32_STEP.  Measured
# worst case over the shapes, tracers and variants of test_vs_oracle, per step at 1 / 10 steps:
#   SW2D       u 1.7e-6 / 9.1e-7, v 1.3e-6 / 8.3e-7, p 3.1e-8 / 1.3e-8
#   SW2D_TEMP  u 9.0e-6 / 4.5e-6, v 9.4e-6 / 4.4e-6, p 1.0e-7 / 3.1e-7, t 2.1e-7 / 9.6e-8, q 2.1e-7 / 2.0e-7
# The bounds leave a margin of 2-3x.  u and v carry the pressure gradient, a difference of p values of order 8e3
# (SW2D) or 1e5 (SW2D_TEMP) that differ by O(1): in fp32 that difference keeps only 2-3 significant digits.
F32_STEP = {1: {"u": 4e-6, "v": 4e-6, "p": 1e-7},
            2: {"u": 2e-5, "v": 2e-5, "p": 8e-7, "t": 6e-7, "q": 6e-7}}


def _states(model, tracer, H, W, seed, M=None):
    """random float64 states {p, u, v[, t[, q]]} (the bench recipe: SURVEY section 8), (H, W) or (M, H, W)"""
    rng = np.random.default_rng(seed)
    shape = (H, W) if M is None else (M, H, W)
    s = {"u": rng.standard_normal(shape), "v": rng.standard_normal(shape)}
    if model == 1:
        s["p"] = 8000 + rng.standard_normal(shape)
    else:
        s["p"] = 101325 + rng.standard_normal(shape)
        s["t"] = 273.16 + rng.standard_normal(shape)
        if tracer:
            s["q"] = rng.random(shape)
    return s


def _r32(s):
    return {k: a.astype(np.float32).astype(np.float64) for k, a in s.items()}


def _member(s, m):
    return {k: a[m] for k, a in s.items()}


def _as_dict(got):
    return {k: a for k, a in zip("puvtq", got) if a is not None}


def _run(g, model, tracer, W, H, state, steps, dtype="f32", variant=None, **kw):
    c = g.Core(model, W, H, dx=DX, tracer=tracer, dtype=dtype,
               variant=g._lib.VARIANT_AUTO if variant is None else variant, **kw)
    c.set_state(**state)
    c.step(steps, DT)
    out = _as_dict(c.get_state())
    c.close()
    return out


def _oracle(model, tracer, s, steps):
    """the float64 oracle: `steps` steps of the reference's own scheme, the tracer on the time-n winds"""
    from oracle import sw2d, sw2d_temp, tracer as otr
    if model == 1:
        st = (s["u"], s["v"], s["p"])
        for _ in range(steps):
            st = sw2d.matsumo_scheme(*st, DX, DT)
        return {"u": st[0], "v": st[1], "p": st[2]}
    st, q = (s["u"], s["v"], s["p"], s["t"]), s.get("q")
    for _ in range(steps):
        if tracer:
            q = otr.limited_advection(DT, (DX, DX), np.stack([st[1], st[0]]), q, limiter=tracer == 2)
        st = sw2d_temp.matsumo_scheme(*st, DX, DT)
    out = {"u": st[0], "v": st[1], "p": st[2], "t": st[3]}
    if tracer:
        out["q"] = q
    return out


def _f32_representable(a):
    return np.array_equal(a, a.astype(np.float32).astype(np.float64))


def test_handle_is_fp32(g):
    """the state the handle holds is float32: set_state rounds to nearest-even, get_state widens exactly, and a
    step leaves float32 values that differ from what an fp64 handle computes"""
    model, tracer, H, W = g._lib.SW2D_TEMP, g._lib.TRACER_VANLEER, 47, 130
    s = _states(2, 2, H, W, seed=1)
    c = g.Core(model, W, H, dx=DX, tracer=tracer, dtype="f32")
    assert c.dtype == "f32" and c.options["dtype"] == "f32"
    c.set_state(**s)
    got = _as_dict(c.get_state())
    for k, a in s.items():
        assert np.array_equal(got[k], a.astype(np.float32)), k
    c.step(1, DT)
    one = _as_dict(c.get_state())
    c.close()
    f64 = _run(g, model, tracer, W, H, s, 1, dtype="f64")
    for k in s:
        assert _f32_representable(one[k]), k
        assert not np.array_equal(one[k], f64[k]), k


_ORACLE = {}


# fused1 / fused2: the fused kernel with one column per lane (60-column strips) / two (120-column strips, even
# widths only), pinned with GCM_SW2D_F32_COLS; fused: the handle's own choice
@pytest.mark.parametrize("variant", ["fused", "fused1", "fused2", "staged"])
@pytest.mark.parametrize("name,model,tracer", MODELS)
@pytest.mark.parametrize("H,W", [(16, 32), (47, 130), (33, 97), (48, 2880), (360, 720)])
def test_vs_oracle(g, monkeypatch, H, W, name, model, tracer, variant):
    """1 and 10 steps against the float64 oracle on the float32-rounded inputs, within steps x F32_STEP; the
    bound is not vacuous: the unstepped state is outside it"""
    if variant in ("fused1", "fused2"):
        monkeypatch.setenv("GCM_SW2D_F32_COLS", variant[-1])
    var = g._lib.VARIANT_STAGED if variant == "staged" else g._lib.VARIANT_FUSED
    s = _r32(_states(model, tracer, H, W, seed=H + W + model + tracer))
    key = (H, W, model, tracer)
    if key not in _ORACLE:
        one = _oracle(model, tracer, s, 1)
        _ORACLE[key] = (one, _oracle(model, tracer, one, 9))
    want1, want10 = _ORACLE[key]
    c = g.Core(model, W, H, dx=DX, tracer=tracer, variant=var, dtype="f32")
    c.set_state(**s)
    c.step(1, DT)
    got1 = _as_dict(c.get_state())
    c.step(9, DT)
    got10 = _as_dict(c.get_state())
    c.close()
    errs = {("%s@%d" % (k, n)): rel_err(got[k], b) for n, got, want in ((1, got1, want1), (10, got10, want10))
            for k, b in want.items()}
    skip = {k: rel_err(s[k], want1[k]) for k in want1}
    print("f32 vs oracle", name, variant, H, W, {k: "%.2e" % e for k, e in errs.items()},
          "skip", {k: "%.1e" % e for k, e in skip.items()})
    bound = F32_STEP[model]
    for key, e in errs.items():
        k, n = key.split("@")
        assert e < int(n) * bound[k], (key, e)
    # negative check: the unstepped state misses the oracle by more than the bound, in every field
    for k, e in skip.items():
        assert e > bound[k], (k, e)


def test_conservation(g):
    """sum p (GCM_DIAG_SUM_P) and sum q over 10 steps: the flux form conserves both up to fp32 rounding"""
    H, W = 360, 720
    s = _r32(_states(2, 2, H, W, seed=3))
    for variant in (g._lib.VARIANT_FUSED, g._lib.VARIANT_STAGED):
        c = g.Core(g._lib.SW2D_TEMP, W, H, dx=DX, tracer=g._lib.TRACER_VANLEER, variant=variant, dtype="f32")
        c.set_state(**s)
        p0 = c.diag(g._lib.DIAG_SUM_P)
        assert abs(p0 - s["p"].sum()) <= 1e-12 * abs(p0)
        c.step(10, DT)
        p1 = c.diag(g._lib.DIAG_SUM_P)
        q1 = c.get_state()[4].sum()
        c.close()
        assert abs(p1 - p0) < 1e-7 * abs(p0), (p0, p1)
        assert abs(q1 - s["q"].sum()) < 1e-6 * s["q"].sum(), (q1, s["q"].sum())


@pytest.mark.parametrize("W,cols", [(97, "1"), (98, "2")])
@pytest.mark.parametrize("variant,rows", [("fused", 3), ("fused", 16), ("staged", None)])
@pytest.mark.parametrize("name,model,tracer", [MODELS[0], MODELS[3]])
def test_ensemble_members_equal_single_handles(g, monkeypatch, name, model, tracer, variant, rows, W, cols):
    """5 members, 7 steps (GCM_SW2D with 3-row bands: three two-step launches and a single step): every member
    bit for bit what an fp32 one-member handle computes; one and two columns per lane.  Plain shallow water: the
    handle launches what the pinned rows and columns mean (Core.sw2d_plan) and member 0 is within 7 x F32_STEP of
    the float64 oracle on the float32-rounded inputs, so that a fault the ensemble and the single handle share
    shows too"""
    monkeypatch.setenv("GCM_SW2D_F32_COLS", cols)
    if rows is not None:
        monkeypatch.setenv("GCM_FUSED_ROWS", str(rows))
    monkeypatch.setenv("GCM_SW2D_TWO_STEP", "1")
    var = {"fused": g._lib.VARIANT_FUSED, "staged": g._lib.VARIANT_STAGED}[variant]
    M, H = 5, 61
    s = _states(model, tracer, H, W, seed=21 + model + tracer, M=M)
    plan = None
    if name == "sw2d":
        c = g.Core(model, W, H, dx=DX, tracer=tracer, dtype="f32", variant=var, members=M)
        plan = c.sw2d_plan(7)
        c.close()
    ens = _run(g, model, tracer, W, H, s, 7, variant=var, members=M)
    for m in range(M):
        one = _run(g, model, tracer, W, H, _member(s, m), 7, variant=var)
        for k, b in one.items():
            assert np.array_equal(ens[k][m], b), (m, k)
    if name == "sw2d":
        pairs = 3 if rows == 3 else 0
        assert (plan["variant"], plan["two_step_launches"], plan["single_step_launches"]) == (variant, pairs, 7 - 2 * pairs)
        if rows is not None:
            assert (plan["rows_per_band"], plan["cols"], plan["strip"], plan["preload"], plan["stream"]) == \
                (rows, int(cols), 60 * int(cols), rows <= 4, False), plan
        key = ("ens", W)
        if key not in _ORACLE:
            _ORACLE[key] = _oracle(model, tracer, _r32(_member(s, 0)), 7)
        for k, b in _ORACLE[key].items():
            e = rel_err(ens[k][0], b)
            assert e < 7 * F32_STEP[model][k], (k, e, plan)


def test_ensemble_streams(g, monkeypatch):
    """52 x 720x360 SW2D_TEMP + van Leer in fp32 reads over 256 MB per launch (the STREAM instantiation)"""
    monkeypatch.setenv("GCM_FUSED_ROWS", "24")
    monkeypatch.setenv("GCM_SW2D_F32_COLS", "2")     # (the ensemble's own choice; pinned for the single handles)
    W, H, M, steps = 720, 360, 52, 4
    assert W * H * 4 * 5 * M > 256 << 20
    model, tracer = g._lib.SW2D_TEMP, g._lib.TRACER_VANLEER
    s = _states(2, 2, H, W, seed=41, M=M)
    c = g.Core(model, W, H, dx=DX, tracer=tracer, members=M, dtype="f32")
    c.set_state(**s)
    c.step(steps, DT)
    picks = {m: _as_dict(c.get_member(m)) for m in (0, 29, 51)}
    c.close()
    for m, got in picks.items():
        one = _run(g, model, tracer, W, H, _member(s, m), steps)
        for k, b in one.items():
            assert np.array_equal(got[k], b), (m, k)


def test_member_entry_points_and_diag_members(g):
    model, tracer, M, H, W = g._lib.SW2D_TEMP, g._lib.TRACER_VANLEER, 4, 33, 70
    s = _states(2, 2, H, W, seed=5, M=M)
    c = g.Core(model, W, H, dx=DX, tracer=tracer, members=M, dtype="f32")
    c.set_state(**s)
    new = _states(2, 2, H, W, seed=6)
    c.set_member(2, **new)
    for m in range(M):
        got = _as_dict(c.get_member(m))
        src = new if m == 2 else _member(s, m)
        for k, a in src.items():
            assert np.array_equal(got[k], a.astype(np.float32)), (m, k)
    full = _as_dict(c.get_state())
    sums = c.diag_members(g._lib.DIAG_SUM_P)
    umax = c.diag_members(g._lib.DIAG_MAX_U)
    tv = c.diag_members(g._lib.DIAG_TV_T)
    for m in range(M):
        assert abs(sums[m] - full["p"][m].sum()) <= 1e-12 * abs(sums[m])
        assert umax[m] == full["u"][m].max()
        want_tv = np.abs(full["t"][m] - np.roll(full["t"][m], -1, axis=0)).sum()
        assert abs(tv[m] - want_tv) <= 1e-12 * want_tv
    c.step(3, DT)
    after = c.diag_members(g._lib.DIAG_SUM_P)
    c.close()
    assert np.all(np.abs(after - sums) < 1e-7 * np.abs(sums))


@pytest.mark.parametrize("variant", ["fused1", "fused2", "staged"])
@pytest.mark.parametrize("nb,halo", [(2, 1), (4, 1), (2, 2), (4, 2)])
def test_bands_host_loop_equal_single_domain(g, monkeypatch, nb, halo, variant):
    """nb fp32 bands of one grid in one process, the ghost rows moved by device copies every `halo` steps"""
    import torch
    if variant != "staged":
        monkeypatch.setenv("GCM_SW2D_F32_COLS", variant[-1])
        variant = "fused"
    from gcmiipy_amd.bands import split_rows
    H, W, steps = 40, 130, 4
    var = {"fused": g._lib.VARIANT_FUSED, "staged": g._lib.VARIANT_STAGED}[variant]
    model, tracer = g._lib.SW2D_TEMP, g._lib.TRACER_VANLEER
    s = _states(2, 2, H, W, seed=7)
    want = _run(g, model, tracer, W, H, s, steps, variant=var)
    cores = []
    for r, (row0, n) in enumerate(split_rows(H, nb)):
        c = g.Core(model, W, n, dx=DX, tracer=tracer, variant=var, dtype="f32", nranks=nb, rank=r,
                   global_height=H, row0=row0, halo_steps=halo)
        assert c.halo_bytes() == 5 * 2 * halo * W * 4
        c.set_state(**{k: a[row0:row0 + n] for k, a in s.items()})
        cores.append(c)
    for _ in range(steps // halo):
        su.exchange(cores, torch)
        for c in cores:
            if halo == 1:
                c.step_interior(DT)
                c.step_boundary(DT)
            else:
                c.step(halo, DT)
    got = [np.concatenate(x, axis=0) for x in zip(*[c.get_state() for c in cores])]
    for c in cores:
        c.close()
    for k, a in _as_dict(got).items():
        assert np.array_equal(a, want[k]), k


@pytest.mark.parametrize("cols", ["1", "2"])
@pytest.mark.parametrize("halo,overlap", [(1, False), (2, False), (2, True)])
def test_band_run_loopback_equals_single_domain(g, monkeypatch, halo, overlap, cols):
    """gcm_band_run with the loopback exchange: the fp32 band is its own neighbour, i.e. the periodic single
    domain, bit for bit; with the deep-halo exchange hidden behind the interior rows too (gcm_set_band_overlap)"""
    import torch
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange
    monkeypatch.setenv("GCM_SW2D_F32_COLS", cols)
    H, W, steps = 64, 130, 6
    model, tracer = g._lib.SW2D_TEMP, g._lib.TRACER_VANLEER
    s = _states(2, 2, H, W, seed=8)
    want = _run(g, model, tracer, W, H, s, steps)
    c = g.Core(model, W, H, dx=DX, tracer=tracer, dtype="f32", nranks=2, rank=0, global_height=H, row0=0,
               stream=torch.cuda.current_stream().cuda_stream, halo_steps=halo)
    c.set_state(**s)
    runner = BandRunner(HipBandEngine(c, torch), 0, 2, LoopbackExchange(), north=0, south=0)
    assert runner.native
    if overlap:
        c.set_band_overlap(True)
    runner.run(2, DT)
    runner.run(1, DT)
    runner.run(steps - 3, DT)
    torch.cuda.synchronize()
    got = _as_dict(c.get_state())
    c.close()
    for k, a in got.items():
        assert np.array_equal(a, want[k]), k


def test_odd_width_band_refused(g):
    with pytest.raises(g.GcmError, match="even width"):
        g.Core(g._lib.SW2D, 131, 16, dx=DX, dtype="f32", nranks=2, rank=0, global_height=32)


@pytest.mark.parametrize("members", [1, 3])
def test_snapshot_and_checkpoint_bit_exact(g, tmp_path, members):
    from gcmiipy_amd import checkpoint
    model, tracer, H, W = g._lib.SW2D_TEMP, g._lib.TRACER_VANLEER, 45, 98
    M = members if members > 1 else None
    s = _states(2, 2, H, W, seed=9, M=M)
    c = g.Core(model, W, H, dx=DX, tracer=tracer, dtype="f32", members=members)
    c.set_state(**s)
    c.step(3, DT)
    c.snapshot()
    path = str(tmp_path / "ck.npz")
    checkpoint.save(path, c, step=3)
    c.step(4, DT)
    a = _as_dict(c.get_state())
    c.restore()
    c.step(4, DT)
    b = _as_dict(c.get_state())
    c.close()
    r, ck = checkpoint.restore(path)
    assert r.dtype == "f32" and r.options["dtype"] == "f32" and ck["step"] == 3
    r.step(4, DT)
    d = _as_dict(r.get_state())
    r.close()
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], d[k]), k


def test_half_steps_equal_a_full_step(g):
    """half_step(0) / get_star / set_star / half_step(1) == one full fp32 step of the staged variant"""
    model, tracer, H, W = g._lib.SW2D_TEMP, g._lib.TRACER_VANLEER, 31, 77
    s = _states(2, 2, H, W, seed=10)
    want = _run(g, model, tracer, W, H, s, 1, variant=g._lib.VARIANT_STAGED)
    c = g.Core(model, W, H, dx=DX, tracer=tracer, dtype="f32", variant=g._lib.VARIANT_STAGED)
    c.set_state(**s)
    c.half_step(0, DT)
    star = c.get_star()
    for a in star[:4]:
        assert _f32_representable(a)
    c.set_star(*star[:4])
    c.half_step(1, DT)
    got = _as_dict(c.get_state())
    c.close()
    for k, a in got.items():
        assert np.array_equal(a, want[k]), k


def test_drop_ins(g):
    """the reference-shaped drop-ins with dtype="f32" give what an fp32 Core gives"""
    from gcmiipy_amd import ensemble
    from gcmiipy_amd.matsuno_c_grid import matsumo_scheme
    from gcmiipy_amd.matsumo_temp import matsumo_scheme_with_tracer
    H, W = 29, 66
    s = _states(1, 0, H, W, seed=12)
    u, v, p = matsumo_scheme(s["u"], s["v"], s["p"], DX, DT, dtype="f32")
    want = _run(g, g._lib.SW2D, 0, W, H, s, 1)
    assert np.array_equal(u, want["u"]) and np.array_equal(v, want["v"]) and np.array_equal(p, want["p"])
    s = _states(2, 2, H, W, seed=13)
    out = matsumo_scheme_with_tracer(s["u"], s["v"], s["p"], s["t"], s["q"], DX, DT, dtype="f32")
    want = _run(g, g._lib.SW2D_TEMP, 2, W, H, s, 1)
    for k, a in zip("uvptq", out):
        assert np.array_equal(a, want[k]), k
    se = _states(2, 2, H, W, seed=14, M=3)
    out = ensemble.matsumo_temp_scheme(se["u"], se["v"], se["p"], se["t"], DX, DT, q=se["q"], dtype="f32")
    for m in range(3):
        want = _run(g, g._lib.SW2D_TEMP, 2, W, H, _member(se, m), 1)
        for k, a in zip("uvptq", out):
            assert np.array_equal(a[m], want[k]), (m, k)
    g.clear_cache()
