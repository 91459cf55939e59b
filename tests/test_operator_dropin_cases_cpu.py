"""The cases of operator_dropin_cases.py are not vacuous (no GPU needed): the oracle is well conditioned on
them, deliberately wrong variants miss the oracle on them, and a reference is identically zero only where
every neighbour along the operator's axis is the cell itself."""
import numpy as np
import pytest

import operator_dropin_cases as oc
from exner_ref import EDGE_ERR_BOUND, ERR_BOUND, exner_emulated, exner_extended, max_rel_err, table
from oracle import tracer

FAMILIES = (
    [(op, s, oc.inputs_2d) for s in oc.SHAPES_2D for op in oc.ops_2d()]
    + [(op, (n,), lambda s: oc.inputs_1d(s[0])) for n in oc.LENGTHS_1D for op in oc.ops_1d()]
    + [(op, s, oc.inputs_elementwise) for s in oc.ELEMENTWISE_SHAPES for op in oc.ops_elementwise()]
)


def test_case_lists_are_the_ones_the_kernels_need():
    assert set(oc.SHAPES_2D) == {(1, 1), (1, 2), (2, 1), (2, 3), (3, 2), (4, 64), (5, 65), (9, 130), (67, 9)}
    assert oc.LENGTHS_1D == (1, 2, 3, 255, 256, 257, 1000)
    assert oc.ELEMENTWISE_SHAPES == ((), (1,), (63,), (64,), (65,), (300,), (3, 130))
    assert max(h * w for h, w in oc.SHAPES_2D) < 33800          # the arena test's field is the largest
    for shape in oc.SHAPES_2D:                                  # the planted plateau and zero velocity are there
        d = oc.inputs_2d(shape)
        W = shape[1]
        if W >= 6:
            assert np.all(d["q"][:, W - 3] == d["q"][:, W - 2]) and np.all(d["q"][:, W - 2] == d["q"][:, W - 1])
        if W >= 2:
            assert np.all(d["V"][:, :, oc.zero_velocity_column(W)] == 0.0) and np.count_nonzero(d["V"] == 0.0) == 2 * shape[0]


def test_oracle_sensitivity_and_zero_references():
    """float64 against long double on the same inputs: the inputs do not use up the bound.  A reference is
    identically zero exactly where the operator says it must be, and at every extent of 4 or more it lies above
    its floor, so the floor decides nothing there."""
    worst = {}
    for op, shape, make in FAMILIES:
        d = make(shape)
        want = np.asarray(op.ref(d))
        wide = np.asarray(op.ref(oc.as_longdouble(d)))
        assert wide.dtype == np.longdouble and want.dtype == np.float64, (op, shape)
        floor = op.floor(d)
        diff = np.max(np.abs(want.astype(np.longdouble) - wide))
        scale = max(np.max(np.abs(wide)), floor)
        s = float(diff if scale == 0 else diff / scale)
        assert s < oc.SENSITIVITY_MAX, (op, shape, s)
        fam = op.name.split(".")[0] + (" 1-D" if len(shape) == 1 and op.name.startswith("two_d") else "")
        if s >= worst.get(fam, (0.0,))[0]:
            worst[fam] = (s, op.name, shape)
        is_zero = not np.any(want)
        assert is_zero == op.zero_when(shape), (op, shape, is_zero)
        if min(shape, default=1) >= 4:          # (below that, symmetric neighbours cancel: dvt on 2 x 1 is 3e-5 of its terms)
            assert np.max(np.abs(want)) > floor, (op, shape, float(np.max(np.abs(want))), floor)
    for fam, (s, name, shape) in sorted(worst.items()):
        print("oracle sensitivity, worst of %-14s %.2e  (%s at %s)" % (fam, s, name, shape))


def test_zero_references_are_the_extent_one_shapes():
    """named outright, for the 2-D list: the one-sided differences vanish along an axis of extent 1, the centred
    gradient also at extent 2 (its +1 and -1 neighbours are one cell), nothing else vanishes"""
    zero = {}
    for op in oc.ops_2d():
        for shape in oc.SHAPES_2D:
            if not np.any(op.ref(oc.inputs_2d(shape))):
                zero.setdefault(shape, set()).add(op.name)
    assert set(zero) == {(1, 1), (1, 2), (2, 1), (2, 3), (3, 2)}
    centred0 = {"two_d.gradient[axis 0]", "two_d.pressure_gradient[0]"}
    centred1 = {"two_d.gradient[axis 1]", "two_d.pressure_gradient[1]"}
    assert zero[(2, 3)] == centred0 and zero[(3, 2)] == centred1
    along0 = centred0 | {"two_d.upwind_axis_finite[axis 0]", "two_d.fv_advect_axis_upwind_finite[axis 0]",
                         "two_d.fv_advect_axis_plain_finite[axis 0]", "two_d.pgf_c_grid_axis[axis 0]",
                         "two_d.pgf_c_grid[0]", "two_d.pgf_templess[0]", "two_d.pgf_one_d[axis 0]",
                         "two_d.pgf_one_d(line)", "no_limits_2d.pgf[v]"}
    along1 = centred1 | {"two_d.upwind_axis_finite[axis 1]", "two_d.fv_advect_axis_upwind_finite[axis 1]",
                         "two_d.fv_advect_axis_plain_finite[axis 1]", "two_d.pgf_c_grid_axis[axis 1]",
                         "two_d.pgf_c_grid[1]", "two_d.pgf_templess[1]", "two_d.pgf_one_d[axis 1]",
                         "no_limits_2d.pgf[u]", "no_limits_2d.advec_m[dut]"}
    assert zero[(1, 2)] == along0 | centred1
    assert zero[(2, 1)] == along1 | centred0
    assert zero[(1, 1)] == along0 | along1 | {"no_limits_2d.advec_p", "no_limits_2d.advec_m[dvt]", "no_limits_2d.advec_t"}


# ---- planted mistakes -----------------------------------------------------------------------------
def limited_axis(dt, sc, V, q, axis, roll=np.roll, strict=True, mask=True):
    """oracle.tracer.limited_axis restated, with the three places a kernel can get wrong exposed: the periodic
    shift, the strictness of the upwind test, the mask of the ratio"""
    dx = sc[axis]
    q_p_1 = roll(q, -1, axis)
    zeroes = np.zeros(q.shape)
    f_low = (q * np.maximum(V[axis], zeroes) + q_p_1 * np.minimum(V[axis], zeroes)) * dt / dx
    f_high = V[axis] * ((q + q_p_1) / 2) * dt / dx
    a = q - roll(q, 1, axis)
    b = q_p_1 - q
    c = roll(b, -1, axis)
    with np.errstate(divide="ignore", invalid="ignore"):
        where = (b != 0) if mask else np.ones(b.shape, dtype=bool)
        r_pos = np.divide(a, b, out=np.zeros_like(a), where=where)
        r_neg = np.divide(c, b, out=np.zeros_like(a), where=where)
        r = np.where((V[axis] > 0) if strict else (V[axis] >= 0), r_pos, r_neg)
        flux = f_low + tracer.van_leer(r) * (f_high - f_low)
    return q - flux + roll(flux, 1, axis)


def limited_advection(d, **kw):
    q = d["q"]
    for axis in range(2):
        q = limited_axis(oc.DT, oc.SC, d["V"], q, axis, **kw)
    return q


def plain_axis(d, axis, roll=np.roll):
    """oracle.tracer.fv_advect_axis_plain restated: the centred flux reads the +1 neighbour whatever the wind"""
    q, volume = d["q"], oc.SC[0] * oc.SC[1]
    flux = d["V"][axis] * ((q + roll(q, -1, axis)) / 2) * oc.DT * (volume / oc.SC[axis])
    return q - (flux - roll(flux, 1, axis)) / volume


def roll_last_column_clamped(x, shift, axis):
    r = np.roll(x, shift, axis)
    if axis == 1 and shift == -1:
        r[:, -1] = x[:, -1]                    # the east neighbour of the last column: itself, not column 0
    return r


def roll_axes_swapped(x, shift, axis):
    return np.roll(x, shift, 1 - axis)


def missed(e):
    return not e <= oc.TOL                     # a NaN result is a miss


@pytest.mark.parametrize("shape", oc.SHAPES_2D, ids=str)
def test_planted_mistakes_miss_the_oracle(shape):
    H, W = shape
    d = oc.inputs_2d(shape)
    want = tracer.limited_advection(oc.DT, oc.SC, d["V"], d["q"])
    assert np.array_equal(limited_advection(d), want)            # the restatement is the oracle, bit for bit
    plain = tracer.fv_advect_axis_plain(oc.DT, oc.SC, d["V"], d["q"], 1)
    assert np.array_equal(plain_axis(d, 1), plain)
    e = oc.err(limited_advection(d, roll=roll_last_column_clamped), want)
    e_plain = oc.err(plain_axis(d, 1, roll=roll_last_column_clamped), plain)
    print(shape, "last column clamped: %.2e limited, %.2e centred" % (e, e_plain))
    # (one column: the clamp is the wrap.  Two columns: the limiter's ratio is -1 and the limited flux is the upwind
    # one, which reads the wrap neighbour only where the wind blows from it; the centred flux always reads it)
    assert missed(e_plain) if W >= 2 else e_plain == 0.0
    assert missed(e) if W >= 3 else (e == 0.0 or W == 2)
    e = oc.err(limited_advection(d, roll=roll_axes_swapped), want)
    print(shape, "axes swapped: %.2e" % e)
    assert missed(e) if H != W else e == 0.0                     # (every shape but 1 x 1 is non-square)
    e = oc.err(limited_advection(d, mask=False), want)
    print(shape, "ratio without the b != 0 mask: %.2e" % e)
    # b == 0: on the planted plateau (W >= 6), and where the neighbour is the cell itself
    assert missed(e) if (W >= 6 or min(H, W) == 1) else e == 0.0
    # u >= 0 for u > 0: a face of zero velocity carries no flux whichever side is taken for upwind, so on
    # finite data the strictness cannot show in a value -- only in the sign of a zero flux (next test)
    assert np.array_equal(limited_advection(d, strict=False), want)


@pytest.mark.parametrize("n", oc.LENGTHS_1D)
def test_planted_mistakes_miss_the_flux_limiter_oracle(n):
    """the bit-for-bit rule of the flux_limiter tests sees `u >= 0` for `u > 0` (the sign of the zero flux at the
    planted u == 0 between a positive and a negative q) and a ratio without its mask (the planted plateau)"""
    d = oc.inputs_flux_limiter(n)
    q, u = d["q"], d["u"]
    want = tracer.donor_cell_flux(q, u)
    assert oc.same_bits(np.where(u > 0, q, np.roll(q, -1, 0)) * u, want)
    wrong = np.where(u >= 0, q, np.roll(q, -1, 0)) * u
    assert oc.same_bits(wrong, want) == (n == 1)                 # (one cell: both sides are that cell)
    if n >= 2:
        assert np.array_equal(wrong, want) and want[0] == 0.0 and np.signbit(want[0]) and not np.signbit(wrong[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        unmasked = (q - np.roll(q, 1, 0)) / (np.roll(q, -1, 0) - q)
    assert oc.same_bits(unmasked, tracer.calc_r(q)) == (n in (2, 3))     # b == 0: one cell, or the plateau (n >= 8)
    # what the inputs are said to carry
    assert np.any(q == 1e30) or np.any(q == -1e30)
    if n >= 3:
        assert np.any((q == 0.0) & np.signbit(q)) and np.any((u == 0.0) & np.signbit(u)) and np.any((u == 0.0) & ~np.signbit(u))
    if n >= 8:
        assert q[3] == q[4] == q[5] and np.isinf(d["special"][0]) and np.isnan(d["special"][1])


def test_same_bits_rule():
    z = np.array([0.0, 1.0, np.nan])
    assert oc.same_bits(z, z.copy())
    assert not oc.same_bits(z, np.array([-0.0, 1.0, np.nan]))
    assert not oc.same_bits(z, np.array([0.0, np.nextafter(1.0, 2.0), np.nan]))
    assert not oc.same_bits(z, np.array([0.0, 1.0, 2.0]))
    assert not oc.same_bits(z[:2], z)


def test_error_rule_is_rel_err_above_the_floor():
    from conftest import rel_err
    a, b = np.array([1.0, 2.0 + 1e-9]), np.array([1.0, 2.0])
    assert oc.err(a, b) == rel_err(a, b) == oc.err(a, b, floor=2.0)
    assert oc.err(a, b, floor=4.0) == rel_err(a, b) / 2
    assert oc.err(np.array([1e-13]), np.array([0.0]), floor=1.0) == 1e-13
    assert oc.err(np.array([1e-13]), np.array([0.0])) == 1e-13          # rel_err's own rule for a zero reference


def test_exner_pressures_span_the_domain_and_the_emulation_holds_there():
    """the emulation of the device algorithm keeps its bounds on the very pressures the GPU test uses"""
    wide, edges = oc.exner_pressures()
    tab = table()
    assert wide.min() < 2.0 ** -59 and wide.max() > 2.0 ** 59
    assert edges.min() == 2.0 ** -64 and edges.max() == np.nextafter(2.0 ** 63, np.inf)
    assert np.all(np.isfinite(exner_emulated(wide, tab)))
    e_wide = max_rel_err(exner_emulated(wide, tab), exner_extended(wide))
    e_edge = max_rel_err(exner_emulated(edges, tab), exner_extended(edges))
    print("emulated exner: %.2e over 2^-60..2^60, %.2e at the interval edges" % (e_wide, e_edge))
    assert e_wide < ERR_BOUND and e_edge < EDGE_ERR_BOUND
    out = oc.exner_outside()
    assert not np.any((out >= 2.0 ** -64) & (out < 2.0 ** 64))
