"""GPU parity of the stand-alone operator drop-ins (csrc/ops2d_kernels.hip behind gcm_advect2d, gcm_pgf2d,
gcm_sw2d_op, gcm_pe1d_op and gcm_flux_limiter) against the oracle at the shapes of operator_dropin_cases.py:
beyond the first workgroup, on ragged last blocks, and on extents 1, 2 and 3 where the neighbours are the cell
itself.  Also the device exner() across its stated domain, the grow-only scratch arena of these calls, and the
refusals.  test_operator_dropin_cases_cpu.py shows that the cases can tell a wrong kernel from a right one."""
import ctypes as C
import functools

import numpy as np
import pytest

import operator_dropin_cases as oc
from exner_ref import EDGE_ERR_BOUND, ERR_BOUND, exner_emulated, exner_extended, max_rel_err, table

pytestmark = pytest.mark.gpu
TOL = oc.TOL


def _frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def case_2d(shape):
    """inputs and oracle results of one 2-D shape, computed once and read-only"""
    d = _frozen(oc.inputs_2d(shape))
    return d, _frozen({op.name: np.asarray(op.ref(d)) for op in oc.ops_2d()})


@functools.lru_cache(maxsize=None)
def case_1d(n):
    d = _frozen(oc.inputs_1d(n))
    return d, _frozen({op.name: np.asarray(op.ref(d)) for op in oc.ops_1d()})


def hold(ops, d, refs, label):
    """every operator of the table against its reference: print each error, then assert them all"""
    missed = []
    for op in ops:
        got = op.run(d)
        e = oc.err(got, refs[op.name], op.floor(d))
        print("%-12s %-48s %.2e" % (label, op.name, e))
        if not e < TOL:
            missed.append((op.name, e))
    assert not missed, (label, missed)


@pytest.mark.parametrize("shape", oc.SHAPES_2D, ids=str)
def test_two_d_and_no_limits_2d_vs_oracle(shape):
    d, refs = case_2d(shape)
    hold(oc.ops_2d(), d, refs, str(shape))


@pytest.mark.parametrize("n", oc.LENGTHS_1D)
def test_no_limits_and_the_1d_call_form_vs_oracle(n):
    d, refs = case_1d(n)
    hold(oc.ops_1d(), d, refs, "n=%d" % n)


@pytest.mark.parametrize("shape", oc.ELEMENTWISE_SHAPES, ids=str)
def test_elementwise_vs_oracle(shape):
    d = oc.inputs_elementwise(shape)
    ops = oc.ops_elementwise()
    refs = {op.name: np.asarray(op.ref(d)) for op in ops}
    if shape == ():
        assert all(isinstance(op.run(d), float) for op in ops)       # a scalar in, a scalar out
    hold(ops, d, refs, str(shape))


@pytest.mark.parametrize("n", oc.LENGTHS_1D)
def test_flux_limiter_bit_for_bit(n):
    """np.array_equal against oracle.tracer (NaN equal to NaN), the signs of the zeros included: with u == 0 between
    a positive and a negative q, the sign of the zero flux is all that the strict `u > 0` decides"""
    d = oc.inputs_flux_limiter(n)
    differ = []
    for name, ref, run in oc.ops_flux_limiter():
        with np.errstate(invalid="ignore"):              # inf - inf in the oracle is meant
            got, want = run(d), ref(d)
        same = oc.same_bits(got, want)
        print("n=%-5d %-36s %s" % (n, name, "bit-identical" if same else
                                   "DIFFERS in %d cells" % np.count_nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))))
        if not same:
            differ.append(name)
    assert not differ, (n, differ)


def test_device_exner_across_its_domain():
    """to_true_temp(1.0, p) is exner(p) with no further rounding.  Element by element against extended precision,
    under the bounds test_math_cpu.py asserts of the emulation; NaN outside 2^-64 <= p < 2^64."""
    from gcmiipy_amd import temperature as tm
    tab = table()
    wide, edges = oc.exner_pressures()
    for label, p, bound in (("log-uniform 2^-60..2^60", wide, ERR_BOUND), ("interval edges +-1 ulp", edges, EDGE_ERR_BOUND)):
        got = tm.to_true_temp(np.ones_like(p), p)
        assert got.shape == p.shape and np.all(np.isfinite(got))
        e = max_rel_err(got, exner_extended(p))
        emu = exner_emulated(p, tab)
        print("device exner, %-24s %d points: max rel err %.2e (bound %.0e); emulation %.2e; numpy pow %.2e; "
              "device == emulation bit for bit: %s (%d cells differ)"
              % (label, p.size, e, bound, max_rel_err(emu, exner_extended(p)),
                 max_rel_err(np.power(p / 1e5, 287.0 / 1004.0), exner_extended(p)),
                 np.array_equal(got, emu), np.count_nonzero(got != emu)))
        assert e < bound, (label, e)
    out = oc.exner_outside()
    got = tm.to_true_temp(np.ones_like(out), out)
    print("device exner outside its domain:", dict(zip(out.tolist(), got.tolist())))
    assert np.all(np.isnan(got)), got


# ---- the scratch arena of these calls (csrc/dev_arena.h) ---------------------------------------------
def _release_scratch():
    from gcmiipy_amd import _lib
    assert _lib.lib.gcm_ops_release_scratch() == _lib.OK


def test_scratch_arena_outgrown_mid_call():
    """after a release the arena starts at 1 MiB; advect_with_momentum at 130 x 260 needs six operands of 270 KB,
    so the fourth lands in a second block while the first three are in use, and the end of the call merges the
    blocks.  A tiny call and the same call again then run in the merged block."""
    from gcmiipy_amd import two_d
    from oracle import tracer
    big, tiny = oc.inputs_2d((130, 260)), oc.inputs_2d((1, 2))
    assert 6 * big["p"].nbytes > (1 << 20) > 3 * big["p"].nbytes
    want_big = tracer.advect_with_momentum(oc.DT, oc.SC, big["V"], big["p"])
    want_tiny = tracer.advect_with_momentum(oc.DT, oc.SC, tiny["V"], tiny["p"])
    _release_scratch()
    first = two_d.advect_with_momentum(oc.DT, oc.SC, big["V"], big["p"])
    small = two_d.advect_with_momentum(oc.DT, oc.SC, tiny["V"], tiny["p"])
    again = two_d.advect_with_momentum(oc.DT, oc.SC, big["V"], big["p"])
    _release_scratch()
    small_fresh = two_d.advect_with_momentum(oc.DT, oc.SC, tiny["V"], tiny["p"])
    e_big, e_tiny = oc.err(first, want_big), oc.err(small, want_tiny)
    print("arena: 130x260 advect_with_momentum %.2e, 1x2 %.2e; second call bit-identical: %s; tiny call after a "
          "release bit-identical: %s" % (e_big, e_tiny, np.array_equal(first, again), np.array_equal(small, small_fresh)))
    assert e_big < TOL and e_tiny < TOL
    assert np.array_equal(first, again) and np.array_equal(small, small_fresh)


def test_results_do_not_depend_on_earlier_calls():
    """the whole 2-D list in ascending size (the arena grows step by step) and in descending size (it starts at
    its largest): each call gives the same bits either way, and the oracle's result"""
    ops = oc.ops_2d()
    runs = []
    for descending in (False, True):
        _release_scratch()
        runs.append({(shape, op.name): np.array(op.run(case_2d(shape)[0]))
                     for shape in oc.by_size(oc.SHAPES_2D, descending) for op in ops})
    up, down = runs
    assert list(up) != list(down) and set(up) == set(down) and len(up) == len(ops) * len(oc.SHAPES_2D)
    differ = [k for k in up if not np.array_equal(up[k], down[k], equal_nan=True)]
    errs = [(oc.err(up[(shape, op.name)], case_2d(shape)[1][op.name], op.floor(case_2d(shape)[0])), str(shape), op.name)
            for shape in oc.SHAPES_2D for op in ops]
    missed = [x for x in errs if not x[0] < TOL]
    print("ascending vs descending: %d calls, %d differ; %d miss the oracle; worst error %.2e (%s %s)"
          % ((len(up), len(differ), len(missed)) + max(errs, key=lambda x: (x[0] != x[0], x[0]))))
    assert not differ, differ
    assert not missed, missed


# ---- refusals change nothing ---------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched():
    from gcmiipy_amd import _lib, two_d
    lib = _lib.lib
    H, W = 3, 5
    d = oc.inputs_2d((H, W))
    V, q, p, t = (np.ascontiguousarray(d[k]) for k in ("V", "q", "p", "t"))
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def advect(scheme, axes, finite, nsteps, dx0=10.0, dx1=12.5):
        out = np.full((H, W), 7.25)
        with pytest.raises(ValueError):
            two_d._ops_check(lib.gcm_advect2d(scheme, axes, finite, W, H, nsteps, 1.0, dx0, dx1, ptr(V), ptr(q), ptr(out)))
        assert np.all(out == 7.25), (scheme, axes, finite, nsteps, dx0, dx1)

    advect(_lib.ADV_UPWIND, 1, 1, 2)              # finite (increment) output with nsteps != 1
    advect(_lib.ADV_UPWIND, 2, 1, 0)
    advect(_lib.ADV_FV_PLAIN, 3, 1, 1)            # finite output with both axes
    advect(-1, 1, 0, 1)                           # a bad scheme
    advect(_lib.ADV_MOMENTUM + 1, 1, 0, 1)
    advect(_lib.ADV_UPWIND, 0, 0, 1)              # no axis / an axis that is not there
    advect(_lib.ADV_UPWIND, 4, 0, 1)
    for bad in (0.0, -10.0, float("nan")):        # dx <= 0
        advect(_lib.ADV_FV_UPWIND, 3, 0, 1, dx0=bad)
        advect(_lib.ADV_FV_UPWIND, 3, 0, 1, dx1=bad)

    for kind in (1, 5):                           # pgf_c_grid and pressure_gradient without t
        out = np.full((2, H, W), 7.25)
        with pytest.raises(ValueError):
            two_d._ops_check(lib.gcm_pgf2d(kind, W, H, 1.0, 10.0, 12.5, ptr(p), None, ptr(out)))
        assert np.all(out == 7.25), kind
    # and the same calls go through once they are well formed
    out = np.full((H, W), 7.25)
    two_d._ops_check(lib.gcm_advect2d(_lib.ADV_UPWIND, 1, 1, W, H, 1, 1.0, 10.0, 12.5, ptr(V), ptr(q), ptr(out)))
    assert not np.any(out == 7.25)
    out = np.full((2, H, W), 7.25)
    two_d._ops_check(lib.gcm_pgf2d(1, W, H, 1.0, 10.0, 12.5, ptr(p), ptr(t), ptr(out)))
    assert not np.any(out == 7.25)
