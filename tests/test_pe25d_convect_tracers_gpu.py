"""GPU tests of the convective mixing of the passive tracers of GCM_PE25D (gcm_set_tracer_convect /
Core.set_tracer_convection): the launch ahead of the adjustment's against the NumPy restatement
(tests/pe25d_convect_tracers_ref.py), what it must leave alone, and its place in a step -- the launch order, the join of
the tracers' streams and the next stage's wait, across steps.  The handles come from tests/gpu_setups.py and the CONVECT
set-up of tests/column_phase_cases.py; the inputs' conditions (no near-tied comparison) are checked without a device in
tests/test_pe25d_convect_tracers_cpu.py."""
import numpy as np
import pytest

import column_phase_cases as cc
import gpu_setups as su
import pe25d_convect_ref as cref
import pe25d_convect_tracers_ref as ref
from gpu_setups import g  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

PH = cc.CONVECT
GAMMA, KC, DTS = cc.GAMMA, cc.KC, cc.DTS
ON = (0, 2)                                               # the tracers that opt in; tracer 1 does not
# fp64 on every shape, fp32 on the first and the third
KERNEL_CASES = [(s, "f64") for s in ref.SHAPES] + [(ref.SHAPES[0], "f32"), (ref.SHAPES[2], "f32")]


def case_id(case):
    return "%s-%s" % (cc.shape_id(case[0]), case[1])


def handle(g, geom, st, trs, dtype="f64", on=ON):
    c = cc.handle(PH, g, geom, st, dtype, trs=trs)
    for i in on:
        c.set_tracer_convection(i)
    assert c.tracer_convections() == sorted(on)
    return c


_want = {}


def restated(shape, kappa_c, dtype):
    """(geometry, state, tracers, the restatement's tracers, its merged cells and the cells of theta that the adjustment's
    restatement changes), computed once per case and left unchanged"""
    key = (shape, kappa_c, dtype)
    if key not in _want:
        geom = PH.geom_of(shape)
        st, trs = ref.inputs(geom, kappa_c, dtype)
        out, merged = ref.mix_step(st[0], st[3], trs, ON, geom.sig, geom.dsig, geom.ptop, kappa_c, dtype)
        theta = cref.convect_step(st[0], st[3], st[4], geom.sig, geom.dsig, geom.ptop, cref.params(kappa_c=kappa_c), dtype)[0]
        moved = theta != st[3]
        # (a merged cell keeps its bits only where the block's value rounds to what the cell held: one cell in float32)
        assert not (moved & ~merged).any() and (merged & ~moved).sum() <= 1
        for a in list(st) + [trs, out, merged, moved]:
            a.setflags(write=False)
        _want[key] = (geom, st, trs, out, merged, moved)
    return _want[key]


# ---------------------------------------------------------------- the launch against the restatement
@pytest.mark.parametrize("case", KERNEL_CASES, ids=case_id)
@pytest.mark.parametrize("gamma", [None, GAMMA], ids=["dry", "gamma"])
@pytest.mark.parametrize("mix_q", [1, 0], ids=["mix_q", "keep_q"])
def test_explicit_step_equals_the_restatement(g, case, gamma, mix_q):
    shape, dtype = case
    kappa_c = 0.0 if gamma is None else KC
    geom, st, trs, want, merged, moved = restated(shape, kappa_c, dtype)
    par = dict(gamma=gamma, mix_q=mix_q)
    plain = handle(g, geom, st, trs, dtype, on=())
    plain.convect_step(**par)
    plain_state, plain_trs = plain.get_state(), plain.get_tracers()
    plain.close()
    assert np.array_equal(plain_trs, trs)                     # without an opt-in the adjustment leaves every tracer
    c = handle(g, geom, st, trs, dtype)
    c.convect_step(**par)
    state, got = c.get_state(), c.get_tracers()
    c.close()
    # theta and q are what the same call gives without any opt-in: the adjustment is untouched
    cc.assert_same(state, plain_state, "the adjustment with and without opt-ins")
    # the device's block structure is the restatement's, from theta's changed cells: the cells the restatement of the
    # adjustment changes (its merged cells, but for one cell in float32 whose block's value rounds to what the cell held)
    assert np.array_equal(state[3] != st[3], moved), "the device merged other cells than the restatement"
    assert merged.any() and not merged.all()
    # the cells the tracer launch changed are exactly the restatement's merged cells (those it gave another value)
    changed = got != trs
    assert not changed[1].any(), "tracer 1 has not opted in"
    for f in ON:
        assert not (changed[f] & ~merged).any(), f
        assert np.array_equal(changed[f], want[f] != trs[f]), f
    assert np.array_equal(changed[ON[0]] | changed[ON[1]], merged)
    if dtype == "f64":
        rel = max(cc.linf(got[f], want[f]) for f in ON)
        print(shape, dtype, par, "rel", rel)
        assert rel <= 1e-10
        assert np.array_equal(got, want)                      # (the same blocks: the same sequential sums, bit for bit)
    else:
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        worst = float(np.max(np.abs(got - want) / ulp))
        print(shape, dtype, par, "ulp", worst)
        assert worst <= 1.0
        assert np.array_equal(got.astype(np.float32).astype(np.float64), got)


@pytest.mark.parametrize("case", [(ref.SHAPES[1], "f64"), (ref.SHAPES[2], "f32")], ids=case_id)
def test_an_all_stable_state_leaves_every_tracer(g, case):
    shape, dtype = case
    geom = PH.geom_of(shape)
    st, trs = ref.inputs(geom, KC, dtype, stable=True)
    c = handle(g, geom, st, trs, dtype, on=(0, 1, 2))
    c.convect_step(gamma=GAMMA)
    state, got = c.get_state(), c.get_tracers()
    c.close()
    assert np.array_equal(state[3], st[3]) and np.array_equal(got, trs)


def test_stable_lanes_of_an_unstable_wave_are_not_written(g):
    """one unstable column per wave of (24, 4, 130): columns 3, 70 and 129 -- the last wave has two lanes in the row, and
    a store of a lane past W would land in the next level's or row's first columns.  Every other column's tracers keep
    their bits"""
    shape = ref.SHAPES[2]
    geom = PH.geom_of(shape)
    st, trs = ref.inputs(geom, 0.0, "f64", stable=True)
    cols = [3, 70, 129]
    t = st[3].copy()
    t[2][:, cols] += 7.0                                      # (level 2 warmer than levels 3 and 4 above it: 40 K / 24 a level)
    st = st[:3] + [t] + st[4:]
    want, merged = ref.mix_step(st[0], t, trs, (0, 1, 2), geom.sig, geom.dsig, geom.ptop, 0.0)
    assert merged[:, :, cols].any(axis=0).all() and not np.delete(merged, cols, axis=2).any()
    c = handle(g, geom, st, trs, on=(0, 1, 2))
    c.convect_step()
    got = c.get_tracers()
    c.close()
    assert np.array_equal(np.delete(got, cols, axis=3), np.delete(trs, cols, axis=3))
    assert np.array_equal(got, want) and (got != trs).any()


@pytest.mark.parametrize("shape", [ref.SHAPES[0], ref.SHAPES[2]], ids=cc.shape_id)
def test_mass_is_kept_and_the_range_does_not_widen(g, shape):
    geom, st, trs, want, merged, _ = restated(shape, KC, "f64")
    c = handle(g, geom, st, trs, on=(0, 1, 2))
    before = c.tracer_stats()
    c.convect_step(gamma=GAMMA)
    after = c.tracer_stats()
    moved = (c.get_tracers() != trs).reshape(ref.NTR, -1).any(axis=1)
    c.close()
    rel = np.abs(after.mass - before.mass) / np.abs(before.mass)
    print(shape, "mass", rel, "min", before.min, after.min, "max", before.max, after.max)
    assert moved.all()
    assert (rel <= 1e-12).all()
    assert (after.min >= before.min).all() and (after.max <= before.max).all()
    assert np.array_equal(after.air, before.air) and not after.nan.any()


@pytest.mark.parametrize("shape", [ref.SHAPES[0], ref.SHAPES[2]], ids=cc.shape_id)
def test_a_tracer_equal_to_q_follows_the_mixed_q(g, shape):
    """mix_q = 1: q of a block is Qs / D in the merge tree's order, the tracer's the sequential sums: equal to 1e-13
    relative, by design not to the bit"""
    geom, st, trs, _, merged, _ = restated(shape, KC, "f64")
    trs = trs.copy()
    trs[0] = st[4]
    c = handle(g, geom, st, trs, on=(0,))
    c.convect_step(gamma=GAMMA, mix_q=1)
    q, got = c.get_state()[4], c.get_tracers()[0]
    c.close()
    assert (q != st[4]).any()
    rel = float(np.max(np.abs(got - q) / np.abs(q)))
    print(shape, "tracer against q", rel)
    assert rel <= 1e-13
    assert np.array_equal(got[~merged], q[~merged])


# ---------------------------------------------------------------- steps
STEPS = 6
STEP_ON = (0, 1)


def step_inputs():
    geom = PH.geom_of(cc.STEP)
    st, trs = ref.inputs(geom, KC)
    L, H, W = cc.STEP
    emission = np.zeros((L, H, W))
    emission[0] = 1e-4 * (1.0 + np.random.default_rng(3).random((H, W)))     # (a surface source: the bottom level)
    k = 2e-6 * (1.0 + np.arange(L - 1.0))
    return geom, st, trs, emission, k


def step_handle(g, geom, st, trs, emission, k, on=STEP_ON, convect=True):
    """convection, the forcing of tracer 0 and the mixing of tracers 0 and 1 registered; 3 tracers, `on` opted in"""
    c = cc.handle(PH, g, geom, st, trs=trs)
    c.set_tracer_forcing(0, emission=emission, decay=1e-6)
    c.set_tracer_mixing(0, k)
    c.set_tracer_mixing(1, k)
    if convect:
        c.set_convect(gamma=GAMMA)
    for i in on:
        c.set_tracer_convection(i)
    return c


_stepped = {}


def stepped(g):
    """the state and the tracers after step(STEPS), computed once"""
    if "want" not in _stepped:
        geom, st, trs, emission, k = step_inputs()
        c = step_handle(g, geom, st, trs, emission, k)
        c.step(STEPS, DTS)
        out = c.get_state(), c.get_tracers()
        sums = c.convect_sums()
        c.close()
        assert sums.count.any() and sums.nsteps == STEPS
        for a in out[0] + [out[1]]:
            a.setflags(write=False)
        _stepped["want"] = out
    return _stepped["want"]


def test_six_steps_at_once_equal_six_single_steps(g):
    want = stepped(g)
    geom, st, trs, emission, k = step_inputs()
    c = step_handle(g, geom, st, trs, emission, k)
    for _ in range(STEPS):
        c.step(1, DTS)
    got = c.get_state(), c.get_tracers()
    c.close()
    su.assert_equal(got, want, "step(1) x 6")


def test_steps_equal_the_host_driven_sequence(g):
    """a dynamics step with neither the adjustment registered nor an opt-in, the mixing applied to the downloaded
    tracers by the restatement, then convect_step: the same bits as step(6).  The launch's place ahead of the
    adjustment, its join of the tracers' streams and the next stage's wait are what makes the two agree"""
    want = stepped(g)
    geom, st, trs, emission, k = step_inputs()
    c = step_handle(g, geom, st, trs, emission, k, on=(), convect=False)
    adjusted = 0
    for _ in range(STEPS):
        c.step(1, DTS)
        state, cur = c.get_state(), c.get_tracers()
        mixed, merged = ref.mix_step(state[0], state[3], cur, STEP_ON, geom.sig, geom.dsig, geom.ptop, KC)
        adjusted += int(merged.any())
        c.set_tracers(mixed)
        c.convect_step(gamma=GAMMA)
    got = c.get_state(), c.get_tracers()
    assert c.tracer_forcing(0) is not None and c.tracer_mixing(1) is not None
    c.close()
    assert adjusted == STEPS                                  # (every step had blocks to mix in)
    su.assert_equal(got, want, "host-driven")
    # and the mixing moved the tracers: without the opt-ins they end elsewhere
    d = step_handle(g, geom, st, trs, emission, k, on=())
    d.step(STEPS, DTS)
    other = d.get_tracers()
    d.close()
    assert np.array_equal(other[2], want[1][2])
    assert (other[0] != want[1][0]).any() and (other[1] != want[1][1]).any()


def test_one_stream_gives_the_same_bits(g, monkeypatch):
    want = stepped(g)
    for key in su.ORCH_ENV:
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setenv("GCM_PE_SINGLE_STREAM", "1")
    geom, st, trs, emission, k = step_inputs()
    c = step_handle(g, geom, st, trs, emission, k)
    c.step(STEPS, DTS)
    got = c.get_state(), c.get_tracers()
    c.close()
    su.assert_equal(got, want, "GCM_PE_SINGLE_STREAM=1")


def test_either_half_alone_changes_no_tracer(g):
    """opt-ins without set_convect: nothing is launched, two steps equal the plain handle's, state and tracers; set_convect
    without an opt-in: the step's tracers are the plain step's (the adjustment then changes theta and q alone)"""
    geom, st, trs, emission, k = step_inputs()

    def run(steps, **kw):
        c = step_handle(g, geom, st, trs, emission, k, **kw)
        c.step(steps, DTS)
        out = c.get_state(), c.get_tracers()
        c.close()
        return out
    plain2 = run(2, on=(), convect=False)
    su.assert_equal(run(2, on=STEP_ON, convect=False), plain2, "opt-ins without set_convect")
    plain1 = run(1, on=(), convect=False)
    state, got = run(1, on=(), convect=True)
    assert np.array_equal(got, plain1[1])
    assert (state[3] != plain1[0][3]).any()


# ---------------------------------------------------------------- refusals
def test_refusals_change_nothing(g):
    import torch
    lib, L_ = g._lib.lib, g._lib
    geom, st, trs, _, _, _ = restated(ref.SHAPES[0], KC, "f64")
    c = handle(g, geom, st, trs, on=(2,))
    flags = lambda: [lib.gcm_tracer_convected(c._h, i) for i in range(ref.NTR)]
    assert flags() == [0, 0, 1]
    for i in (-1, ref.NTR, 99):
        assert lib.gcm_set_tracer_convect(c._h, i, 1) == L_.ERR_ARG
        assert lib.gcm_tracer_convected(c._h, i) == L_.ERR_ARG
        with pytest.raises((g.GcmError, ValueError)):
            c.set_tracer_convection(i)
    assert flags() == [0, 0, 1] and np.array_equal(c.get_tracers(), trs)
    cc.assert_same(c.get_state(), st, "state after refused calls")
    # off again, and the life cycle of the forcing: kept by set_tracers of the same count, dropped with another
    c.set_tracer_convection(2, on=False)
    assert flags() == [0, 0, 0] and not c.tracer_convected(2)
    c.set_tracer_convection(1)
    c.set_tracers(trs)
    assert flags() == [0, 1, 0]
    c.set_tracers(trs[:2])
    assert [lib.gcm_tracer_convected(c._h, i) for i in range(2)] == [0, 0] and c.tracer_convections() == []
    c.close()
    # a latitude band
    band, eng, runner = su.loopback_band(g, torch, PH.geom_of(cc.BAND), ntr=2)
    assert lib.gcm_set_tracer_convect(band._h, 0, 1) == L_.ERR_UNSUPPORTED
    assert b"bands" in lib.gcm_last_error(band._h)
    with pytest.raises(g.GcmError, match="bands"):
        eng.set_tracer_convection(0)
    assert [lib.gcm_tracer_convected(band._h, i) for i in range(2)] == [0, 0]
    band.close()
    # a 2-D handle
    sw = g.Core(L_.SW2D, 32, 16, dx=1e5)
    assert lib.gcm_set_tracer_convect(sw._h, 0, 1) == L_.ERR_UNSUPPORTED
    assert lib.gcm_tracer_convected(sw._h, 0) == L_.ERR_UNSUPPORTED
    sw.close()


# ---------------------------------------------------------------- the checkpoint
def test_checkpoint_carries_the_opt_ins(g, tmp_path):
    from gcmiipy_amd import checkpoint
    geom, st, trs, emission, k = step_inputs()
    whole = step_handle(g, geom, st, trs, emission, k)
    whole.step(4, DTS)
    want = whole.get_state(), whole.get_tracers()
    whole.close()
    a = step_handle(g, geom, st, trs, emission, k)
    a.step(2, DTS)
    path = str(tmp_path / "convect_tracers.npz")
    checkpoint.save(path, a, step=2, geom=geom)
    a.close()
    b, ck = checkpoint.restore(path)
    assert ck["tracer_convect"] == list(STEP_ON) and b.tracer_convections() == list(STEP_ON)
    b.step(2, DTS)
    got = b.get_state(), b.get_tracers()
    b.close()
    su.assert_equal(got, want, "restored")
    # a file without the field (what the code before the opt-ins wrote) loads, with none set
    plain = step_handle(g, geom, st, trs, emission, k, on=())
    checkpoint.save(path, plain, geom=geom)
    plain.close()
    assert "tracer_convect" not in np.load(path).files
    c, ck = checkpoint.restore(path)
    assert ck["tracer_convect"] == [] and c.tracer_convections() == [] and c.tracer_count == ref.NTR
    c.close()
