"""What the GPU tests of the column phases of GCM_PE25D share -- the boundary layer, the convective adjustment and the
moist physics are one mechanism in the library (PeColumnSums, one phase walk) and in the package (core.COLUMN_PHASES),
and one set of cases here: the comparison helpers, one descriptor per phase (PHASES: what the cases differ in, as
data), and the bodies of the cases that every phase takes alike.  tests/test_pe25d_column_phases_gpu.py runs the bodies;
each phase's own file keeps what is its own and takes the helpers and its descriptor from here.  The entry points follow
from the phase's name the way core._ColumnPhase derives them: set_<name>, <name>_step, <name>_sums, put_<name>,
<name>_reset, <name>_registered, bands.merge_<name>, gcm_*_<name>, the checkpoint's key.  Every comparison is bit for
bit (np.array_equal).  TEST INFRASTRUCTURE, no test in here."""
import collections

import numpy as np
import pytest

import gpu_setups as su
import pe25d_boundary_layer_ref as bref
import pe25d_convect_ref as cref
import pe25d_inputs as inp
import pe25d_moist_ref as mref

DT = 600.0                                               # the explicit step's dt
DTS = 120.0                                              # the dynamics' dt
TAU = 86400.0
GAMMA = cref.GAMMA
KC = cref.kappa_of(GAMMA)
STEP = (9, 24, 36)                                       # (L, H, W) of the convect tests that take dynamics steps
BAND = (9, 12, 36)                                       # H = 12: 2 and 3 bands


# ---------------------------------------------------------------- a: the helpers
def final(c, close=True):
    """the state, and the ground temperature where the handle has one"""
    out = c.get_state() + ([c.get_ground()] if c.has_ground else [])
    if close:
        c.close()
    return out


def assert_same(got, want, what=""):
    assert len(got) == len(want)
    for k, a, b in zip("puvtqg", got, want):
        assert np.array_equal(a, b), (what, k, float(np.max(np.abs(a - b))))


def assert_same_sums(got, want, what="", seconds=None):
    """two records of one column phase: nsteps, seconds and both sums (type(want)._fields[2:]).  seconds: what the record
    must hold where that is not want's (explicit calls of a step without dt add none)"""
    assert type(got) is type(want), (what, type(got), type(want))
    assert got.nsteps == want.nsteps and got.seconds == (want.seconds if seconds is None else seconds), (what, got[:2], want[:2])
    for f in type(want)._fields[2:]:
        a, b = getattr(got, f), getattr(want, f)
        assert np.array_equal(a, b), (what, "%s.%s" % (type(want).__name__, f), float(np.max(np.abs(a - b))))


def linf(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def wet_state(geom, dtype="f64"):
    """the unstable state with q set around saturation (the recipe of pe25d_moist_ref.humid_state on this theta), so
    that the moist physics behind the adjustment has something to condense"""
    p, u, v, t, q = cref.unstable_state(geom)
    rh = 0.3 + 1.1 * np.random.default_rng(21).random(q.shape)
    p_lev, pi = mref.levels(p, geom.sig, geom.ptop)
    _, qs, _, can = mref.saturation(t * pi, p_lev)
    q = np.where(can, np.minimum(rh * qs, 0.5), 0.02)
    st = [p, u, v, t, q]
    if dtype == "f32":
        st = [a.astype(np.float32).astype(np.float64) for a in st]
    return st


# ---------------------------------------------------------------- b: one descriptor per phase
# name, record: the phase's name and the name of its records (g._lib.<record>: the parameters; g.<record>: the sums).
# ref: its restatement (params, DEFAULTS).  geom_of(shape, ptop): the shape convention of that restatement.
# filtered(geom): whether a single-domain handle takes a filter plan (the shapes that are never stepped take none).
# inputs(geom, dtype) -> (state, ground temperature or None) of the cases that take dynamics steps, kernel_inputs: of
# those that do not.  step_takes_dt: whether <name>_step takes dt; a step without dt adds no seconds to the sums.
# moved(sums): "the phase moved bits", on a record of sums.  par: the parameters of the band cases;
# band_cases, loopback_shapes: the (shape, nb) of the in-process bands and the shapes of the loopback band;
# chain: the case at a size where the launches overlap (moved takes the step count too).  explicit, refusal,
# checkpoint: shape and parameters of those cases, rec: the parameters the handle then reports; checkpoint's beside:
# the phases registered beside it, steps: the steps ahead of the file and behind it.
Phase = collections.namedtuple("Phase", "name record ref geom_of filtered inputs kernel_inputs step_takes_dt moved par "
                               "band_cases loopback_shapes chain explicit refusal checkpoint")


def _hwl(shape, ptop=0.0):
    return su.geom_of(*shape, ptop)


def _lhw(shape, ptop=0.0):
    L, H, W = shape
    return su.geom_of(H, W, L, ptop)


def _humid(geom, dtype="f64"):
    return mref.humid_state(geom, dtype), None


def _windy(geom, dtype="f64"):
    st = bref.windy_state(geom, dtype)
    return st, bref.ground(geom, st)


MOIST = Phase(
    name="moist", record="Moist", ref=mref, geom_of=_hwl,
    filtered=lambda geom: geom.width != 300,
    inputs=_humid, kernel_inputs=_humid,
    step_takes_dt=True,
    moved=lambda sums: sums.precip.max() > 0 and sums.evap.max() > 0,
    par=dict(tau_e=TAU),
    band_cases=((mref.SHAPES[0], 2), (mref.SHAPES[0], 3), (mref.SHAPES[1], 2)),
    loopback_shapes=mref.SHAPES[:2],
    chain=dict(shape=(48, 1440, 24), dt=1.0, steps=2,
               par=dict(tau_e=600.0),                    # (a source that moves bits in a step of one second)
               moved=lambda sums, steps: sums.precip.max() > 0 and sums.evap.max() > 0),
    explicit=dict(shape=mref.SHAPES[0], par=dict(tau_e=TAU)),
    refusal=dict(shape=mref.SHAPES[1], par=dict(tau_e=TAU), rec=mref.params(tau_e=TAU)),
    checkpoint=dict(shape=mref.SHAPES[0], par=dict(tau_e=43200.0, rh_s=0.7), rec=mref.params(tau_e=43200.0, rh_s=0.7),
                    beside={}, steps=(2, 1)))

CONVECT = Phase(
    name="convect", record="Convect", ref=cref, geom_of=_lhw,
    filtered=lambda geom: (geom.layers, geom.height, geom.width) in (STEP, BAND) or geom.width == 1440,
    inputs=lambda geom, dtype="f64": (cref.unstable_state(geom, KC, dtype), None),
    kernel_inputs=lambda geom, dtype="f64": (cref.unstable_state(geom, 0.0, dtype), None),
    step_takes_dt=False,
    moved=lambda sums: sums.count.any(),
    par=dict(gamma=GAMMA),
    band_cases=((BAND, 2), (BAND, 3)),
    loopback_shapes=(BAND,),
    chain=dict(shape=(24, 48, 1440), dt=1.0, steps=2, par=dict(gamma=GAMMA),
               moved=lambda sums, steps: 0.5 < sums.count.mean() / steps < 1.0 and sums.levels.max() >= 4),
    explicit=dict(shape=cref.SHAPES[0], par=dict(gamma=GAMMA)),
    refusal=dict(shape=cref.SHAPES[1], par=dict(gamma=GAMMA), rec=cref.params(kappa_c=KC)),
    checkpoint=dict(shape=STEP, par=dict(gamma=GAMMA, mix_q=0), rec=cref.params(kappa_c=KC, mix_q=0), beside={},
                    steps=(2, 1)))

# (on latitude bands the boundary layer is another protocol -- opt-in, a third exchange: tests/test_pe25d_band_boundary_layer_gpu.py)
BOUNDARY_LAYER = Phase(
    name="boundary_layer", record="BoundaryLayer", ref=bref, geom_of=_hwl,
    filtered=lambda geom: geom.width != 300,
    inputs=_windy, kernel_inputs=_windy,
    step_takes_dt=True,
    moved=lambda sums: sums.shf.any() and sums.evap.any(),
    par=None, band_cases=(), loopback_shapes=(), chain=None,
    explicit=dict(shape=bref.SHAPES[0], par={}),
    refusal=dict(shape=bref.SHAPES[1], par=dict(cd0=1e-3), rec=bref.params(cd0=1e-3)),
    checkpoint=dict(shape=bref.SHAPES[0], par=dict(cd0=1e-3, p_pbl=80000.0), rec=bref.params(cd0=1e-3, p_pbl=80000.0),
                    beside=dict(convect=dict(gamma=GAMMA), moist={}), steps=(2, 2)))

PHASES = (MOIST, CONVECT, BOUNDARY_LAYER)


def shape_id(shape):
    return "x".join(str(n) for n in shape)


# ---------------------------------------------------------------- c: the shared bodies
def handle(ph, g, geom, st, dtype="f64", **kw):
    """a single-domain handle; the shapes that are never stepped take no filter plan"""
    return su.single(g, geom, st, dtype=dtype, filter=ph.filtered(geom), **kw)


def explicit_step(ph, c, dt, **par):
    """<name>_step, with dt where the phase's step takes one"""
    step = getattr(c, ph.name + "_step")
    return step(dt, **par) if ph.step_takes_dt else step(**par)


def sums_of(ph, c):
    return getattr(c, ph.name + "_sums")()


_single_cache = {}


def single_reference(ph, g, shape, dtype, steps, dt=DTS):
    """the single domain's state and sums after steps[0] and after steps[0] + steps[1] steps, computed once per case"""
    key = (ph.name, shape, dtype, steps, dt)
    if key not in _single_cache:
        geom = ph.geom_of(shape)
        c = handle(ph, g, geom, ph.inputs(geom, dtype)[0], dtype)
        getattr(c, "set_" + ph.name)(**ph.par)
        out = []
        for n in steps:
            c.step(n, dt)
            out.append((final(c, close=False), sums_of(ph, c)))
        c.close()
        for state, sums in out:
            for a in state + list(sums[2:]):
                a.setflags(write=False)
        _single_cache[key] = out
    return _single_cache[key]


def bands(ph, g, geom, nb, st, dtype):
    """nb in-process bands with their own rows of the state (the way gpu_setups.bands builds them), the phase registered"""
    from gcmiipy_amd.bands import split_rows
    H, W, L = geom.height, geom.width, geom.layers
    cores = []
    for r, (row0, n) in enumerate(split_rows(H, nb)):
        c = g.Core(g._lib.PE25D, W, n, L, geom=geom, nranks=nb, rank=r, global_height=H, row0=row0, dtype=dtype)
        assert c.halo_bytes() == inp.halo_bytes(W, L, 8 if dtype == "f64" else 4, 0, 1)
        c.set_state(*[inp.rows(a, slice(row0, row0 + n)) for a in st])
        getattr(c, "set_" + ph.name)(**ph.par)
        cores.append(c)
    return cores


def in_process_bands_equal_single_domain(ph, g, shape, nb, dtype):
    """whole stages, two exchanges per step (the order of gcm_band_run), then the phase by the explicit call on own rows
    and ghost rows: the ghost rows are adjusted locally, no third exchange, and add to no sum.  The second part steps on
    from those ghost rows: they hold the neighbour's bits"""
    import torch
    from gcmiipy_amd import bands as gb
    steps = (2, 1)
    want = single_reference(ph, g, shape, dtype, steps)
    geom = ph.geom_of(shape)
    cores = bands(ph, g, geom, nb, ph.inputs(geom, dtype)[0], dtype)

    def physics(k):
        for c in cores:
            explicit_step(ph, c, DTS, **ph.par)
    for part, n in enumerate(steps):
        su.whole_steps(cores, torch, n, DTS, prime=part == 0, after=physics)
        parts = [c.get_state() for c in cores]
        got = [np.concatenate([x[f] for x in parts], axis=0 if f == 0 else 1) for f in range(5)]
        assert_same(got, want[part][0], (nb, part))
        assert ph.moved(want[part][1])
        merged = getattr(gb, "merge_" + ph.name)([sums_of(ph, c) for c in cores])
        assert_same_sums(merged, want[part][1], (nb, part), seconds=None if ph.step_takes_dt else 0.0)
    for c in cores:
        c.close()


def loopback_band_run_equals_single_domain(ph, g, shape, dtype, host_loop, monkeypatch):
    """gcm_band_run with the phase registered (and the host-driven sequence, GCM_BAND_HOST_LOOP=1, whose physics_step
    ends the step with gcm_end_step: the same sums, seconds included): several steps in one run, then a second run after
    a get_state"""
    import torch
    for k in su.ORCH_ENV:
        monkeypatch.delenv(k, raising=False)
    if host_loop:
        monkeypatch.setenv("GCM_BAND_HOST_LOOP", "1")
    steps = (2, 1)
    want = single_reference(ph, g, shape, dtype, steps)
    geom = ph.geom_of(shape)
    c, eng, runner = su.loopback_band(g, torch, geom, dtype=dtype)
    assert runner.native == (not host_loop)
    getattr(eng, "set_" + ph.name)(**ph.par)
    assert c.halo_bytes() == inp.halo_bytes(geom.width, geom.layers, 8 if dtype == "f64" else 4, 0, 1)
    c.set_state(*ph.inputs(geom, dtype)[0])
    for part, n in enumerate(steps):
        runner.run(n, DTS)
        torch.cuda.synchronize()
        assert ph.moved(want[part][1])
        assert_same(final(c, close=False), want[part][0], part)
        assert_same_sums(sums_of(ph, c), want[part][1], part)
    c.close()


def band_run_chains_with_the_phase(ph, g, dtype, monkeypatch):
    """the grid of test_band_run_chains_at_overlapping_size (48 x 1440 x 24: kernels of tens of microseconds on either
    stream), 2 steps.  The launch keeps the fork at the last K4: the default orchestration, one stream
    (GCM_PE_SINGLE_STREAM=1) and the exchange on the comm stream (GCM_BAND_COMM_STREAM=1) all give the single domain's
    bits, state and sums"""
    import torch
    shape, dt, steps, par = (ph.chain[k] for k in ("shape", "dt", "steps", "par"))
    geom = ph.geom_of(shape)
    st = ph.inputs(geom, dtype)[0]
    for k in su.ORCH_ENV:
        monkeypatch.delenv(k, raising=False)
    one = handle(ph, g, geom, st, dtype)
    getattr(one, "set_" + ph.name)(**par)
    one.step(steps, dt)
    want, want_sums = final(one, close=False), sums_of(ph, one)
    one.close()
    assert ph.chain["moved"](want_sums, steps)
    for env in ({}, {"GCM_PE_SINGLE_STREAM": "1"}, {"GCM_BAND_COMM_STREAM": "1"}):
        for k in su.ORCH_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c, eng, runner = su.loopback_band(g, torch, geom, dtype=dtype)
        assert runner.native
        getattr(eng, "set_" + ph.name)(**par)
        c.set_state(*st)
        runner.run(steps, dt)
        torch.cuda.synchronize()
        assert_same(final(c, close=False), want, env)
        assert_same_sums(sums_of(ph, c), want_sums, env)
        c.close()


def explicit_step_without_a_registration_keeps_no_sums(ph, g):
    geom = ph.geom_of(ph.explicit["shape"])
    st, gt = ph.kernel_inputs(geom)
    par = ph.explicit["par"]
    a, b = handle(ph, g, geom, st, gt=gt), handle(ph, g, geom, st, gt=gt)
    explicit_step(ph, a, DT, **par)
    assert getattr(a, ph.name) is None and not getattr(a, ph.name + "_registered")
    with pytest.raises(g.GcmError):
        sums_of(ph, a)
    getattr(b, "set_" + ph.name)(**par)
    explicit_step(ph, b, DT, **par)
    assert ph.moved(sums_of(ph, b))
    assert_same(final(a), final(b), "with and without sums")


# the refusals every phase shares, in two halves: a phase's own file refuses its own calls on the handle between them
def refusal_inputs(ph):
    """(geometry, state, ground temperature or None) of the refusal case"""
    geom = ph.geom_of(ph.refusal["shape"])
    return (geom,) + tuple(ph.kernel_inputs(geom))


def refused_without_a_registration(ph, g, c):
    """sums, get, put and reset ahead of the registration are GCM_ERR_STATE; then the phase registered and applied once
    -> (sums, state) as they then are"""
    lib, L_ = g._lib.lib, g._lib
    with pytest.raises(g.GcmError):
        sums_of(ph, c)                                    # GCM_ERR_STATE
    assert getattr(lib, "gcm_get_" + ph.name)(c._h, None, None, None, None) == L_.ERR_STATE
    assert getattr(lib, "gcm_%s_reset" % ph.name)(c._h) == L_.ERR_STATE
    z = np.zeros((c.H, c.W))
    assert getattr(lib, "gcm_put_" + ph.name)(c._h, z.ctypes.data_as(L_._dp), z.ctypes.data_as(L_._dp), 0.0, 0) == L_.ERR_STATE
    assert getattr(lib, "gcm_%s_on" % ph.name)(c._h) == 0
    getattr(c, "set_" + ph.name)(**ph.refusal["par"])
    explicit_step(ph, c, DT, **ph.refusal["par"])
    was, was_state = sums_of(ph, c), c.get_state()
    assert ph.moved(was)
    return was, was_state


def refused_calls_changed_nothing(ph, g, c, was, was_state):
    """refused put_* arguments, then: the registration, the state and the sums are what they were ahead of every refused
    call (the handle is closed); other models give GCM_ERR_UNSUPPORTED"""
    lib, L_ = g._lib.lib, g._lib
    put = getattr(c, "put_" + ph.name)
    with pytest.raises(ValueError):
        put(-1, 0.0, *was[2:])
    with pytest.raises(ValueError):
        put(1, float("nan"), *was[2:])
    assert getattr(lib, "gcm_put_" + ph.name)(c._h, None, None, 0.0, 0) == L_.ERR_ARG
    assert getattr(c, ph.name) == ph.refusal["rec"] and getattr(lib, "gcm_%s_on" % ph.name)(c._h) == 1
    assert_same(c.get_state(), was_state, "state after refused calls")
    assert_same_sums(sums_of(ph, c), was, "sums after refused calls")
    c.close()
    # other models
    s = g.Core(g._lib.SW2D, 32, 16, dx=1e5)
    rec = getattr(L_, ph.record)(*ph.ref.DEFAULTS.values())
    step = getattr(lib, "gcm_%s_step" % ph.name)
    assert getattr(lib, "gcm_set_" + ph.name)(s._h, rec) == L_.ERR_UNSUPPORTED
    assert (step(s._h, 60.0, rec) if ph.step_takes_dt else step(s._h, rec)) == L_.ERR_UNSUPPORTED
    assert getattr(lib, "gcm_get_" + ph.name)(s._h, None, None, None, None) == L_.ERR_UNSUPPORTED
    assert getattr(lib, "gcm_%s_reset" % ph.name)(s._h) == L_.ERR_UNSUPPORTED
    assert getattr(lib, "gcm_%s_on" % ph.name)(s._h) == 0
    s.close()


def checkpoint_carries_the_phase_and_its_sums(ph, g, dtype, tmp_path):
    from gcmiipy_amd import checkpoint
    ck_ = ph.checkpoint
    geom = ph.geom_of(ck_["shape"])
    st, gt = ph.inputs(geom, dtype)
    before, after = ck_["steps"]

    def registered():
        c = handle(ph, g, geom, st, dtype, gt=gt)
        getattr(c, "set_" + ph.name)(**ck_["par"])
        for other, par in ck_["beside"].items():
            getattr(c, "set_" + other)(**par)
        return c
    whole = registered()
    whole.step(before + after, DTS)
    want, want_sums = final(whole, close=False), sums_of(ph, whole)
    whole.close()
    assert ph.moved(want_sums)
    a = registered()
    a.step(before, DTS)
    path = str(tmp_path / (ph.name + ".npz"))
    checkpoint.save(path, a, step=before, geom=geom)
    a.close()
    b, ck = checkpoint.restore(path)
    assert getattr(b, ph.name) == ck_["rec"] and ck[ph.name]["params"] == ck_["rec"] and ck[ph.name]["n"] == before
    assert ck[ph.name]["seconds"] == before * DTS
    assert all(getattr(b, other) is not None for other in ck_["beside"])
    b.step(after, DTS)
    assert_same(final(b, close=False), want, "restored")
    assert_same_sums(sums_of(ph, b), want_sums, "restored")
    b.close()
    # a file without the keys restores with none
    plain = handle(ph, g, geom, st, dtype, gt=gt)
    checkpoint.save(path, plain, geom=geom)
    plain.close()
    c, ck = checkpoint.restore(path)
    assert ck[ph.name] is None and getattr(c, ph.name) is None
    c.close()
    # a phase registered through C alone is refused
    d = handle(ph, g, geom, st, dtype, gt=gt)
    rec = getattr(g._lib, ph.record)(*ph.ref.DEFAULTS.values())
    assert getattr(g._lib.lib, "gcm_set_" + ph.name)(d._h, rec) == g._lib.OK
    assert getattr(d, ph.name) is None and getattr(d, ph.name + "_registered")
    with pytest.raises(g.GcmError, match="gcm_set_" + ph.name):
        checkpoint.save(path, d, geom=geom)
    d.close()
