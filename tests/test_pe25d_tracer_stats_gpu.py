"""GPU tests of the passive tracers' device monitor of GCM_PE25D (gcm_tracer_stats / Core.tracer_stats).

The reference for every figure is NumPy float64 on what the handle itself returns: get_tracers() and get_state() widen
exactly, so an fp32 handle has an exact reference too; geom's float64 dsig is the sigma table; sums are math.fsum.
min, max and both counts must match exactly.  mass and air: |device - fsum| <= (N + 2) 2^-53 sum |c p dsig_k| over the N
cells summed -- any summation order of N doubles stays inside (N - 1) 2^-53 sum |terms|, and the terms carry two
product roundings each."""
import ctypes as C
import math

import numpy as np
import pytest

import gpu_setups as su
import pe25d_inputs as inp
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
BAND_SHAPE = (24, 36, 9)        # H, W, L
DT = 120.0


def _reference(fields, p, geom):
    """per field of `fields` (n, L, H, W) on p (H, W): (min, max, mass, air, negative, nan, sum |c p dsig|, sum |p dsig|)"""
    dsig = np.asarray(geom.dsig, dtype=np.float64).reshape(-1, 1, 1)
    w = (p[None] * dsig).ravel()
    air, air_abs = math.fsum(w), math.fsum(np.abs(w))
    out = []
    for c in fields:
        terms = (c * p * dsig).ravel()
        has_nan = bool(np.isnan(c).any())
        out.append((np.min(c), np.max(c), math.nan if has_nan else math.fsum(terms), air, int(np.sum(c < 0)),
                    int(np.sum(np.isnan(c))), math.nan if has_nan else math.fsum(np.abs(terms)), air_abs))
    return out


def _check(got, fields, p, geom, what=""):
    """every word of the TracerStats `got` against the NumPy reference on `fields` (the tracers, then q where asked)"""
    ref = _reference(fields, p, geom)
    assert len(got.min) == len(ref), what
    assert got.negative.dtype == np.int64 and got.nan.dtype == np.int64
    n_cells = fields[0].size
    for f, (mn, mx, mass, air, neg, nan, s_abs, air_abs) in enumerate(ref):
        d_mass = abs(got.mass[f] - mass)
        d_air = abs(got.air[f] - air)
        print("%s field %d: min %r max %r mass %.17g (off %.3e, bound %.3e) air %.17g (off %.3e, bound %.3e) neg %d nan %d"
              % (what, f, got.min[f], got.max[f], got.mass[f], d_mass, (n_cells + 2) * U * s_abs, got.air[f], d_air,
                 (n_cells + 2) * U * air_abs, got.negative[f], got.nan[f]))
        assert np.array_equal(got.min[f], mn, equal_nan=True), (what, f, "min")
        assert np.array_equal(got.max[f], mx, equal_nan=True), (what, f, "max")
        assert got.negative[f] == neg and got.nan[f] == nan, (what, f, "counts")
        if math.isnan(mass):
            assert math.isnan(got.mass[f]), (what, f, "mass")
        else:
            assert d_mass <= (n_cells + 2) * U * s_abs, (what, f, "mass")
        assert d_air <= (n_cells + 2) * U * air_abs, (what, f, "air")
        assert got.air[f] == got.air[0], (what, f, "air is one number")
    assert np.array_equal(got.mean, got.mass / got.air, equal_nan=True)


def _signed_tracers(H, W, L, n, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.standard_normal((n, L, H, W)) * (1.0 + np.arange(n)).reshape(n, 1, 1, 1))


# ---------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("n", [1, 3, 16])
@pytest.mark.parametrize("shape", [(6, 36, 1), (24, 36, 9), (5, 70, 4), (7, 130, 3)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_shape_sweep(g, dtype, shape, n):
    """W below one wave, W = 70 and 130 either side of one and two waves inside one 256-column chunk, L = 1, one unit
    per workgroup; 1, 3 and 16 tracers of both signs; with and without q: all six words of every record.  (The paths
    beyond one chunk and one unit per workgroup: test_chunks_and_strided_units.)"""
    H, W, L = shape
    geom = su.geom_of(H, W, L)
    st = inp.state(geom)
    c = su.single(g, geom, st, _signed_tracers(H, W, L, n, seed=H + W + n), dtype=dtype)
    trs, (p, _, _, _, q) = c.get_tracers(), c.get_state()
    assert (trs < 0).any() and (trs > 0).any()
    got = c.tracer_stats()
    _check(got, trs, p, geom, (dtype, shape, n))
    got_q = c.tracer_stats(with_q=True)
    _check(got_q, np.concatenate([trs, q[None]]), p, geom, (dtype, shape, n, "q"))
    for a, b in zip(got, got_q):
        assert np.array_equal(a, b[:n])                          # q changes nothing about the tracers' records
    c.close()


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", [(600, 300, 1), (5, 540, 3)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_chunks_and_strided_units(g, dtype, shape, n):
    """the paths the sizes the project runs take, at the smallest shapes that reach them.  (600, 300, 1): two 256-column
    chunks a row with a 44-column tail, 1200 (row, chunk) units on the 1024 workgroups a field is capped at -- workgroups
    0 .. 175 take a second unit, the partials are [field][1024][6], and the fold's threads each take four of them.
    (5, 540, 3): three chunks a row with a 28-column tail, 15 units and as many workgroups.  The same exact checks and
    the same derived bound as the sweep; a planted minimum and maximum sit in the last unit and in the tail"""
    H, W, L = shape
    geom = su.geom_of(H, W, L)
    trs = _signed_tracers(H, W, L, n, seed=H + W + n)
    trs[0, L - 1, H - 1, W - 1] = -1e3                         # the last column of the last unit (its tail)
    trs[n - 1, 0, H - 1, 256] = 1e3                            # the first column of the last row's second chunk
    c = su.single(g, geom, inp.state(geom), trs, dtype=dtype)
    trs, (p, _, _, _, q) = c.get_tracers(), c.get_state()
    got = c.tracer_stats(with_q=True)
    _check(got, np.concatenate([trs, q[None]]), p, geom, (dtype, shape, n, "q"))
    assert got.min[0] == -1e3 and got.max[n - 1] == 1e3
    again = c.tracer_stats(with_q=True)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    _check(c.tracer_stats(), trs, p, geom, (dtype, shape, n))
    c.close()


# ---------------------------------------------------------------- 2. planted values
def test_planted_corner_values(g):
    """tracer 0: its unique minimum at the last column of the last row of the top level; tracer 1: its unique maximum
    at cell (0, 0, 0); tracer 2: exactly one negative cell and exactly one NaN, in two other corners.  Tracer 2
    reports 1 and 1, NaN for min, max and mass; the NaN leaves the records of tracers 0 and 1 alone"""
    H, W, L = BAND_SHAPE
    geom = su.geom_of(H, W, L)
    rng = np.random.default_rng(5)
    trs = 1.0 + rng.random((3, L, H, W))
    trs[0, L - 1, H - 1, W - 1] = 0.25
    trs[1, 0, 0, 0] = 7.5
    trs[2, 0, H - 1, 0] = -1.0
    trs[2, L - 1, 0, W - 1] = np.nan
    c = su.single(g, geom, inp.state(geom), trs)
    got = c.tracer_stats()
    p = c.get_state()[0]
    _check(got, c.get_tracers(), p, geom, "planted")
    assert got.min[0] == 0.25 and got.max[1] == 7.5
    assert got.negative[2] == 1 and got.nan[2] == 1
    assert np.isnan(got.min[2]) and np.isnan(got.max[2]) and np.isnan(got.mass[2])
    assert list(got.negative[:2]) == [0, 0] and list(got.nan[:2]) == [0, 0]
    clean = trs.copy()
    clean[2, L - 1, 0, W - 1] = 1.5
    c.set_tracers(clean)
    want = c.tracer_stats()
    for a, b in zip(got, want):
        assert np.array_equal(a[:2], b[:2])                      # bit for bit the records without the NaN next door
    assert want.nan[2] == 0 and want.negative[2] == 1 and want.min[2] == -1.0
    # -0.0 is not negative
    clean[2, 0, H - 1, 0] = -0.0
    c.set_tracers(clean)
    assert c.tracer_stats().negative[2] == 0
    c.close()


# ---------------------------------------------------------------- 3. the predictor's tracers
def test_star_set(g):
    from gcmiipy_amd import _lib
    H, W, L = BAND_SHAPE
    geom = su.geom_of(H, W, L)
    st, trs = inp.state(geom), inp.tracers(H, W, L, 3)
    c = su.single(g, geom, st, trs, scheme="upwind")
    out = np.full(4 * 6, 7.0)
    ptr = out.ctypes.data_as(C.c_void_p)
    assert _lib.lib.gcm_tracer_stats(c._h, 1, 0, ptr, out.size) == _lib.ERR_STATE       # before a predictor
    assert "predicted" in _lib.lib.gcm_last_error(c._h).decode() and np.all(out == 7.0)
    c.half_step(0, DT)
    star, p_star = c.get_tracers(star=True), c.get_star()[0]
    assert not np.array_equal(star, trs)
    _check(c.tracer_stats(star=True), star, p_star, geom, "star")
    q_star = c.get_star(fields=(_lib.Q,))[_lib.Q]
    _check(c.tracer_stats(star=True, with_q=True), np.concatenate([star, q_star[None]]), p_star, geom, "star q")
    _check(c.tracer_stats(), c.get_tracers(), c.get_state()[0], geom, "current beside star")
    c.set_tracer_scheme("van_leer")                              # drops the predicted tracers
    assert _lib.lib.gcm_tracer_stats(c._h, 1, 0, ptr, out.size) == _lib.ERR_STATE
    assert np.all(out == 7.0)
    with pytest.raises(g.GcmError, match="predicted"):
        c.tracer_stats(star=True)
    c.close()


# ---------------------------------------------------------------- 4. the tracer stream
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_call_joins_the_tracer_stream(g, dtype):
    """step(3) and tracer_stats() right behind it: the last tracer launch runs on the handle's second stream, and the
    call includes it itself -- the reference is taken from get_tracers() afterwards.  A second call: the same bits"""
    H, W, L = BAND_SHAPE
    geom = su.geom_of(H, W, L)
    c = su.single(g, geom, inp.state(geom), inp.tracers(H, W, L, 5), dtype=dtype, scheme="van_leer")
    c.step(3, DT)
    got = c.tracer_stats(with_q=True)
    again = c.tracer_stats(with_q=True)
    trs, (p, _, _, _, q) = c.get_tracers(), c.get_state()
    _check(got, np.concatenate([trs, q[None]]), p, geom, ("stream", dtype))
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    # the call changes nothing a later step reads
    c.step(1, DT)
    other = su.single(g, geom, inp.state(geom), inp.tracers(H, W, L, 5), dtype=dtype, scheme="van_leer")
    other.step(4, DT)
    assert np.array_equal(c.get_tracers(), other.get_tracers())
    assert all(np.array_equal(a, b) for a, b in zip(c.get_state(), other.get_state()))
    c.close()
    other.close()


# ---------------------------------------------------------------- 5. conservation
@pytest.mark.parametrize("scheme", ["centred", "upwind", "van_leer"])
def test_mass_is_conserved_on_the_device(g, scheme):
    """the latitude step function, 20 steps: mass stays within (N + 2) 2^-53 sum |c p dsig_k| of its value before (the
    update is in flux form; tests/test_pe25d_tracer_stats_cpu.py shows the restatement conserving the same sum), and
    the donor-cell scheme leaves no negative cell"""
    H, W, L = BAND_SHAPE
    geom = su.geom_of(H, W, L)
    step = np.zeros((1, L, H, W))
    step[0, :, H // 3: 2 * H // 3, :] = 1.0
    c = su.single(g, geom, inp.state(geom), step, scheme=scheme)
    before = c.tracer_stats()
    dsig = np.asarray(geom.dsig, dtype=np.float64).reshape(-1, 1, 1)
    s_abs = math.fsum(np.abs(step[0] * c.get_state()[0] * dsig).ravel())
    c.step(20, DT)
    after = c.tracer_stats()
    bound = (L * H * W + 2) * U * s_abs
    print("%s: mass %.17g -> %.17g (off %.3e, bound %.3e), min %r max %r negative %d"
          % (scheme, before.mass[0], after.mass[0], abs(after.mass[0] - before.mass[0]), bound, after.min[0], after.max[0],
             after.negative[0]))
    assert not np.array_equal(c.get_tracers(), step)
    assert abs(after.mass[0] - before.mass[0]) <= bound
    assert after.nan[0] == 0
    if scheme == "upwind":
        assert after.negative[0] == 0
    c.close()


# ---------------------------------------------------------------- 6. latitude bands
@pytest.mark.parametrize("rows", [1, 2])
def test_bands_merge_to_the_single_domain(g, rows):
    """3 bands of 8 rows stepped in one process, 2 tracers, 1 or 2 tracer ghost rows a side, 2 steps (the ghost rows
    then hold the neighbours' values; the last exchange follows the last corrector).  The global minimum of tracer 0
    lies in band 1's first row, which is band 0's south ghost row: band 0's own min is not the global one, and the
    three records merge into the single domain's"""
    import torch
    from gcmiipy_amd.bands import merge_tracer_stats, split_rows
    H, W, L = BAND_SHAPE
    nb, ntr, steps = 3, 2, 2
    geom = su.geom_of(H, W, L)
    st = inp.state(geom)
    trs = inp.tracers(H, W, L, ntr)
    trs[0, L // 2, H // nb, W // 2] = -40.0                      # band 1's first row
    trs[1] = np.random.default_rng(9).standard_normal((L, H, W))
    one = su.single(g, geom, st, trs, scheme="upwind")
    one.step(steps, DT)
    single = one.tracer_stats(with_q=True)
    tr1, (p1, _, _, _, q1) = one.get_tracers(), one.get_state()
    one.close()
    assert np.unravel_index(np.argmin(tr1[0]), tr1[0].shape)[1] == H // nb      # the premise: still that row
    cores = su.bands(g, geom, nb, st, trs, scheme="upwind", rows=rows)
    su.whole_steps(cores, torch, steps, DT)
    parts = [c.tracer_stats(with_q=True) for c in cores]
    for r, (c, (row0, n)) in enumerate(zip(cores, split_rows(H, nb))):
        own = c.get_tracers()
        assert np.array_equal(own, tr1[:, :, row0:row0 + n])     # (the bands computed the single domain's bits)
        st_r = c.get_state()
        _check(parts[r], np.concatenate([own, st_r[4][None]]), st_r[0], geom, ("band", r, rows))
        c.close()
    assert parts[0].min[0] > single.min[0] == parts[1].min[0]    # band 0 did not read its ghost rows
    merged = merge_tracer_stats(parts)
    _check(merged, np.concatenate([tr1, q1[None]]), p1, geom, ("merged", rows))
    ref = _reference(np.concatenate([tr1, q1[None]]), p1, geom)
    for f in range(ntr + 1):
        assert merged.min[f] == single.min[f] and merged.max[f] == single.max[f]
        assert merged.negative[f] == single.negative[f] and merged.nan[f] == single.nan[f]
        assert abs(merged.mass[f] - single.mass[f]) <= (L * H * W + 2) * U * ref[f][6]
        assert abs(merged.air[f] - single.air[f]) <= (L * H * W + 2) * U * ref[f][7]


# ---------------------------------------------------------------- 7. refusals
def test_refusals(g):
    from gcmiipy_amd import _lib
    lib = _lib.lib
    H, W, L = 6, 36, 4
    geom = su.geom_of(H, W, L)
    c = su.single(g, geom, inp.state(geom), _signed_tracers(H, W, L, 2, seed=1))
    out = np.full(3 * 6, 7.0)
    ptr = out.ctypes.data_as(C.c_void_p)
    assert lib.gcm_tracer_stats(c._h, 0, 0, ptr, 11) == _lib.ERR_ARG              # 12 needed
    assert lib.gcm_tracer_stats(c._h, 0, 1, ptr, 17) == _lib.ERR_ARG              # 18 needed
    assert np.all(out == 7.0)
    assert lib.gcm_tracer_stats(c._h, 0, 0, None, 18) == _lib.ERR_ARG
    assert lib.gcm_tracer_stats(c._h, 2, 0, ptr, 18) == _lib.ERR_ARG              # which
    assert np.all(out == 7.0)
    assert lib.gcm_tracer_stats(c._h, 0, 0, ptr, 12) == _lib.OK
    assert np.all(out[:12] != 7.0) and np.all(out[12:] == 7.0)                    # nothing past the records
    # n = 0: nothing without q, q's record with it
    c.set_tracers(None)
    out[:] = 7.0
    assert lib.gcm_tracer_stats(c._h, 0, 0, ptr, 0) == _lib.OK and np.all(out == 7.0)
    e = c.tracer_stats()
    assert all(len(x) == 0 for x in e) and e.negative.dtype == np.int64
    assert lib.gcm_tracer_stats(c._h, 0, 1, ptr, 5) == _lib.ERR_ARG and np.all(out == 7.0)
    p, _, _, _, q = c.get_state()
    _check(c.tracer_stats(with_q=True), q[None], p, geom, "q alone")
    c.close()
    sw = g.Core(_lib.SW2D, 130, 16, dx=300e3)
    assert lib.gcm_tracer_stats(sw._h, 0, 0, ptr, 18) == _lib.ERR_UNSUPPORTED
    assert lib.gcm_last_error(sw._h).decode() == "gcm_tracer_stats: GCM_PE25D only"
    assert np.all(out == 7.0)
    with pytest.raises(g.GcmError, match="GCM_PE25D only"):
        sw.tracer_stats()
    sw.close()
