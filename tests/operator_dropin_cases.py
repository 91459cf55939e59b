"""Shapes, inputs, operator tables and the error rule for the stand-alone operator drop-ins (two_d,
no_limits_2d, no_limits, flux_limiter and the elementwise operators of matsumo_temp / temperature) --
the entry points of csrc/ops2d_kernels.hip.  test_operator_dropins_gpu.py holds each drop-in to its
oracle function on these cases; test_operator_dropin_cases_cpu.py shows that the cases are not vacuous.

The 2-D kernels run in workgroups of 64 columns x 4 rows, the 1-D kernels in workgroups of 256 cells."""
import importlib

import numpy as np

from conftest import rel_err
from oracle import oned, pe2d, sw2d_temp, temperature, tracer

TOL = 1e-10                 # the project's bound for a drop-in against its oracle function
SENSITIVITY_MAX = 1e-11     # the oracle's own float64-versus-long-double sensitivity stays under this

SHAPES_2D = (
    (1, 1),      # every neighbour is the cell itself
    (1, 2),      # ... or the one other cell (along the row)
    (2, 1),      # ... or the one other cell (along the column)
    (2, 3),      # two rows: the +-2 neighbour along axis 0 is the cell itself, +1 and -1 are one cell; three
                 # columns: +2 is -1 and -2 is +1 (van Leer's far cell, the diagonal of DUT / DVT)
    (3, 2),      # the same with the axes exchanged
    (4, 64),     # exactly one workgroup
    (5, 65),     # a second block in each direction that holds one row / one column: every wrap partner
                 # lives in another block
    (9, 130),    # three column blocks, the last with 2 lanes in use; three row blocks, the last with 1 row
    (67, 9),     # many row blocks on a narrow grid
)
LENGTHS_1D = (1, 2, 3, 255, 256, 257, 1000)      # around one workgroup of 256 cells, and four of them
ELEMENTWISE_SHAPES = ((), (1,), (63,), (64,), (65,), (300,), (3, 130))

# tests/golden/make_golden.py: g4_tracer, g10_pe2d, g9_oned; the ragged-shape test of test_operators_gpu.py
DT, SC = 1.0, (10.0, 12.5)
PE2D_DX = 100e3
ONED_DX = 70000.0
ELEMENTWISE_DX = 2.5e5


def by_size(shapes, descending=False):
    return sorted(shapes, key=lambda s: (s[0] * s[1], s), reverse=descending)


# ---- inputs -------------------------------------------------------------------------------------
def zero_velocity_column(W):
    """not the last column of two: its face is the wrap, which a zero velocity would take out of every flux"""
    return W // 2 if W > 2 else 0


def inputs_2d(shape):
    """The distributions of g4_tracer (V, q, p, t) and g10_pe2d (p2, u2, v2, t2), seeded from the shape.
    Where W >= 6 the last three cells of every row of q are equal: exact-zero denominators in the limiter's
    ratio, next to the wrap (and across a block edge at W = 65 and 130).  Where W >= 2 one column of V is
    exactly zero: what the strict `u > 0` decides."""
    H, W = shape
    rng = np.random.default_rng(1000 * H + W)
    V = rng.standard_normal((2,) + shape) * 2
    q = rng.random(shape)
    p = 101325 + rng.standard_normal(shape)
    t = 273.15 + rng.standard_normal(shape)
    if W >= 6:
        q[:, W - 3:] = q[:, W - 3:W - 2]
        V[0][:, W - 3:] = V[0][:, W - 3:W - 2]      # the sweep along axis 0 comes first: it must leave the plateau standing
    if W >= 2:
        V[:, :, zero_velocity_column(W)] = 0.0
    p2 = 101325 + 10 * rng.standard_normal(shape)
    u2 = rng.standard_normal(shape)
    v2 = rng.standard_normal(shape)
    t2 = 300 + rng.standard_normal(shape)
    return dict(V=V, q=q, p=p, t=t, p2=p2, u2=u2, v2=v2, t2=t2, pu2=pe2d.calc_pu(p2, u2), pv2=pe2d.calc_pv(p2, v2))


def inputs_1d(n):
    """the same distributions on a line of n cells, for the no_limits operators and the 1-D call form of two_d"""
    rng = np.random.default_rng(n)
    V = rng.standard_normal((1, n)) * 2
    q = rng.random(n)
    p = 101325 + rng.standard_normal(n)
    t = 273.15 + rng.standard_normal(n)
    if n >= 6:
        q[n - 3:] = q[n - 3]
    if n >= 2:
        V[:, n // 2] = 0.0
    return dict(V=V, u=V[0].copy(), q=q, p=p, t=t, pu=oned.calc_pu(V[0], p))


def inputs_elementwise(shape):
    rng = np.random.default_rng(7 + int(np.prod(shape, dtype=np.int64)) + 1000 * len(shape))
    p = np.asarray(101325 + rng.standard_normal(shape))
    t = np.asarray(273.15 + rng.standard_normal(shape))
    pb = np.asarray(p + rng.standard_normal(shape))
    return dict(p=p, t=t, pb=pb, rho=np.asarray(sw2d_temp.density_from(p, t)),
                scaled=np.asarray(sw2d_temp.scaling(p, t, ELEMENTWISE_DX)))


def inputs_flux_limiter(n):
    """q of both signs and u for flux_limiter at length n, carrying (as far as n cells can hold them) a cell of
    u == +0.0 between a positive and a negative q (the strict `u > 0` picks the sign of the zero flux), -0.0 in
    q and in u, a plateau of three equal cells (b == 0 in calc_r) and 1e30.  `special` is q with inf, nan and
    -inf entries, for van_leer and calc_r."""
    rng = np.random.default_rng(100 + n)
    q = rng.random(n) + 0.1
    q[1::2] *= -1.0
    u = rng.standard_normal(n) * 2
    if n == 1:
        q[0] = 1e30
    else:
        u[0] = 0.0                       # q[0] > 0 > q[1]
        q[1] = -1e30
    if n >= 3:
        q[2] = -0.0
        u[2] = -0.0
    if n >= 8:
        q[1] = -0.7
        q[3:6] = q[3]
        q[7] = 1e30
        u[6] = 0.0                       # the cell upwind of 1e30
        u[n - 1] = 0.0                   # across the wrap: q[n-1] against q[0]
    special = q.copy()
    special[0] = np.inf
    if n >= 2:
        special[1] = np.nan
    if n >= 3:
        special[n - 1] = -np.inf
    return dict(q=q, u=u, special=special, dx=10.0, dt=1.0)


def exner_pressures():
    """p across the stated domain of the device exner(), 2^-64 <= p < 2^64: log-uniform over 2^-60 .. 2^60, and
    the table-interval edges 2^e (1 + i/64) with one ulp on either side, for a handful of e"""
    rng = np.random.default_rng(64)
    wide = np.exp2(rng.uniform(-60.0, 60.0, 20000))
    m = 1 + np.arange(0, 65) / 64.0
    edges = np.concatenate([m * 2.0 ** e for e in (-64, -60, -1, 0, 16, 17, 59, 62)])
    edges = np.concatenate([edges, np.nextafter(edges, 0), np.nextafter(edges, np.inf)])
    edges = edges[(edges >= 2.0 ** -64) & (edges < 2.0 ** 64)]
    return wide, edges


def exner_outside():
    """p outside the domain: NaN"""
    return np.array([0.0, -0.0, -1.0, -101325.0, 5e-324, 2.0 ** -1000, np.nextafter(2.0 ** -64, 0), 2.0 ** 64,
                     2.0 ** 64 * 1.5, 1e300, np.inf, -np.inf, np.nan])


def as_longdouble(d):
    return {k: np.asarray(v, dtype=np.longdouble) for k, v in d.items()}


# ---- the error rule -----------------------------------------------------------------------------
def err(got, want, floor=0.0):
    """conftest.rel_err (L-inf over max|reference|), the scale not below `floor`"""
    want = np.asarray(want, dtype=np.float64)
    if want.size == 0 or np.max(np.abs(want)) >= floor:
        return rel_err(got, want)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want)) / floor)


# The floor of an operator that differences fluxes is 1e-3 of the largest term that enters the difference (the
# factor test_two_d_gpu.py uses).  Where every neighbour is the cell itself such a reference is exactly zero,
# and a contracted a*b - c leaves one rounding of a term behind: 1.1e-16 of the term, 1.1e-13 against this
# floor.  On extents 2 and 3 symmetric neighbours can cancel almost as well (dvt on 2 x 1 is 3e-5 of its
# terms).  At every extent of 4 or more the reference is larger than the floor (asserted in the CPU test), so
# the floor does not loosen the bound there.  Operators that subtract two loaded values (the gradients) give
# an exact zero and need no floor.
FLOOR_FACTOR = 1e-3


def _amax(*a):
    return max(float(np.max(np.abs(np.asarray(x, dtype=np.float64)))) for x in a)


class Op:
    """one drop-in against its oracle function: ref(d) and run(d) on an input dict d, the floor of the error
    scale, and the shapes at which the reference is identically zero"""

    def __init__(self, name, ref, run, floor=None, zero_when=None):
        self.name, self.ref, self.run = name, ref, run
        self._floor, self._zero_when = floor, zero_when

    def floor(self, d):
        return 0.0 if self._floor is None else FLOOR_FACTOR * self._floor(d)

    def zero_when(self, shape):
        return False if self._zero_when is None else bool(self._zero_when(shape))

    def __repr__(self):
        return self.name


def _mod(name):
    return importlib.import_module("gcmiipy_amd." + name)


def _repeat(fn, steps):
    def run(dt, sc, V, q):
        for _ in range(steps):
            q = fn(dt, sc, V, q)
        return q
    return run


AXIS_FORMS = ("upwind_axis", "upwind_axis_finite", "fv_advect_axis_upwind", "fv_advect_axis_upwind_finite",
              "fv_advect_axis_plain", "fv_advect_axis_plain_finite")


def _axis_floor(name, ax, sc):
    if not name.endswith("_finite"):
        return None
    if "plain" in name:                                   # flux = V * average * dt * area
        area = float(np.prod(sc)) / sc[ax]
        return lambda d: _amax(d["V"][ax]) * _amax(d["q"]) * DT * area
    return lambda d: _amax(d["V"][ax]) * _amax(d["q"]) * DT / sc[ax]


def ops_two_d_advection():
    ops = []
    for ax in (0, 1):
        for name in AXIS_FORMS:
            ops.append(Op("two_d.%s[axis %d]" % (name, ax),
                          lambda d, name=name, ax=ax: getattr(tracer, name)(DT, SC, d["V"], d["q"], ax),
                          lambda d, name=name, ax=ax: getattr(_mod("two_d"), name)(DT, SC, d["V"], d["q"], ax),
                          _axis_floor(name, ax, SC),
                          (lambda s, ax=ax: s[ax] == 1) if name.endswith("_finite") else None))
    ops += [
        Op("two_d.corner_transport_2d", lambda d: tracer.corner_transport_2d(DT, SC, d["V"], d["q"]),
           lambda d: _mod("two_d").corner_transport_2d(DT, SC, d["V"], d["q"])),
        Op("two_d.finite_volume_advection", lambda d: tracer.finite_volume_advection(DT, SC, d["V"], d["q"]),
           lambda d: _mod("two_d").finite_volume_advection(DT, SC, d["V"], d["q"])),
        Op("two_d.finite_volume_advection(steps=5)",
           lambda d: _repeat(tracer.finite_volume_advection, 5)(DT, SC, d["V"], d["q"]),
           lambda d: _mod("two_d").finite_volume_advection(DT, SC, d["V"], d["q"], steps=5)),
        Op("two_d.limited_advection", lambda d: tracer.limited_advection(DT, SC, d["V"], d["q"]),
           lambda d: _mod("two_d").limited_advection(DT, SC, d["V"], d["q"])),
        Op("two_d.limited_advection(steps=5)",
           lambda d: _repeat(tracer.limited_advection, 5)(DT, SC, d["V"], d["q"]),
           lambda d: _mod("two_d").limited_advection(DT, SC, d["V"], d["q"], steps=5)),
        Op("two_d.advect_with_momentum", lambda d: tracer.advect_with_momentum(DT, SC, d["V"], d["p"]),
           lambda d: _mod("two_d").advect_with_momentum(DT, SC, d["V"], d["p"])),
    ]
    return ops


def ops_two_d_pgf():
    ops = []
    for ax in (0, 1):
        one = lambda s, ax=ax: s[ax] == 1                  # the one-sided difference of a cell with itself
        two = lambda s, ax=ax: s[ax] <= 2                  # the centred one: +1 and -1 are one cell at extent 2
        ops += [
            Op("two_d.pgf_c_grid_axis[axis %d]" % ax, lambda d, ax=ax: tracer.pgf_c_grid_axis(d["p"], SC, ax),
               lambda d, ax=ax: _mod("two_d").pgf_c_grid_axis(d["p"], SC, ax), zero_when=one),
            Op("two_d.gradient[axis %d]" % ax, lambda d, ax=ax: tracer.gradient(d["p"], SC, ax),
               lambda d, ax=ax: _mod("two_d").gradient(d["p"], SC, ax), zero_when=two),
            Op("two_d.pgf_c_grid[%d]" % ax, lambda d, ax=ax: tracer.pgf_c_grid(DT, SC, d["p"], d["t"])[ax],
               lambda d, ax=ax: _mod("two_d").pgf_c_grid(DT, SC, d["p"], d["t"])[ax], zero_when=one),
            Op("two_d.pgf_templess[%d]" % ax, lambda d, ax=ax: tracer.pgf_templess(DT, SC, d["p"])[ax],
               lambda d, ax=ax: _mod("two_d").pgf_templess(DT, SC, d["p"])[ax], zero_when=one),
            Op("two_d.pressure_at_edge[%d]" % ax, lambda d, ax=ax: tracer.pressure_at_edge(d["p"])[ax],
               lambda d, ax=ax: _mod("two_d").pressure_at_edge(d["p"])[ax]),
            Op("two_d.pgf_one_d[axis %d]" % ax, lambda d, ax=ax: tracer.pgf_one_d(DT, SC[ax], d["p"], ax),
               lambda d, ax=ax: _mod("two_d").pgf_one_d(DT, SC[ax], d["p"], ax), zero_when=one),
            Op("two_d.pressure_gradient[%d]" % ax, lambda d, ax=ax: tracer.pressure_gradient(DT, SC, d["p"], d["t"])[ax],
               lambda d, ax=ax: _mod("two_d").pressure_gradient(DT, SC, d["p"], d["t"])[ax], zero_when=two),
        ]
    ops += [
        Op("two_d.pressure_at_edge_one_d", lambda d: tracer.pressure_at_edge_one_d(d["p"]),
           lambda d: _mod("two_d").pressure_at_edge_one_d(d["p"])),
        Op("two_d.pressure_at_edge_one_d(line)", lambda d: tracer.pressure_at_edge_one_d(d["p"][:, 0]),
           lambda d: _mod("two_d").pressure_at_edge_one_d(d["p"][:, 0])),
        Op("two_d.pgf_one_d(line)", lambda d: tracer.pgf_one_d(DT, SC[0], d["p"][:, 0]),
           lambda d: _mod("two_d").pgf_one_d(DT, SC[0], d["p"][:, 0]), zero_when=lambda s: s[0] == 1),
    ]
    return ops


def ops_no_limits_2d():
    dx = PE2D_DX
    n2 = lambda: _mod("no_limits_2d")
    flux = lambda d: _amax(d["pu2"], d["pv2"])
    return [
        Op("no_limits_2d.calc_pu", lambda d: pe2d.calc_pu(d["p2"], d["u2"]), lambda d: n2().calc_pu(d["p2"], d["u2"])),
        Op("no_limits_2d.calc_pv", lambda d: pe2d.calc_pv(d["p2"], d["v2"]), lambda d: n2().calc_pv(d["p2"], d["v2"])),
        Op("no_limits_2d.un_pu", lambda d: pe2d.un_pu(d["pu2"], d["p2"]), lambda d: n2().un_pu(d["pu2"], d["p2"])),
        Op("no_limits_2d.un_pv", lambda d: pe2d.un_pv(d["pv2"], d["p2"]), lambda d: n2().un_pv(d["pv2"], d["p2"])),
        Op("no_limits_2d.advec_p", lambda d: pe2d.advec_p(d["pu2"], d["pv2"], dx),
           lambda d: n2().advec_p(d["pu2"], d["pv2"], dx), lambda d: flux(d) / dx, lambda s: s == (1, 1)),
        Op("no_limits_2d.advec_m[dut]", lambda d: pe2d.advec_m(d["p2"], d["u2"], d["v2"], dx)[0],
           lambda d: n2().advec_m(d["p2"], d["u2"], d["v2"], dx)[0],
           lambda d: _amax(d["u2"], d["v2"]) ** 2 * _amax(d["p2"]) / dx, lambda s: s[1] == 1),
        Op("no_limits_2d.advec_m[dvt]", lambda d: pe2d.advec_m(d["p2"], d["u2"], d["v2"], dx)[1],
           lambda d: n2().advec_m(d["p2"], d["u2"], d["v2"], dx)[1],
           lambda d: _amax(d["u2"], d["v2"]) ** 2 * _amax(d["p2"]) / dx, lambda s: s == (1, 1)),
        Op("no_limits_2d.pgf[u]", lambda d: pe2d.pgf(d["p2"], d["t2"], dx)[0],
           lambda d: n2().pgf(d["p2"], d["t2"], dx)[0], zero_when=lambda s: s[1] == 1),
        Op("no_limits_2d.pgf[v]", lambda d: pe2d.pgf(d["p2"], d["t2"], dx)[1],
           lambda d: n2().pgf(d["p2"], d["t2"], dx)[1], zero_when=lambda s: s[0] == 1),
        Op("no_limits_2d.advec_t", lambda d: pe2d.advec_t(d["pu2"], d["pv2"], d["t2"], dx),
           lambda d: n2().advec_t(d["pu2"], d["pv2"], d["t2"], dx),
           lambda d: flux(d) * _amax(d["t2"]) / dx, lambda s: s == (1, 1)),
    ]


def ops_2d():
    return ops_two_d_advection() + ops_two_d_pgf() + ops_no_limits_2d()


def ops_1d():
    """the no_limits operators one by one, and the 1-D call form (q.ndim == 1) of two_d"""
    dx = ONED_DX
    nl = lambda: _mod("no_limits")
    one = lambda s: s[0] == 1
    ops = [
        Op("no_limits.advec_q", lambda d: oned.advec_q(d["u"], d["q"], dx), lambda d: nl().advec_q(d["u"], d["q"], dx),
           lambda d: _amax(d["u"]) * _amax(d["q"]) / dx, one),
        Op("no_limits.calc_pu", lambda d: oned.calc_pu(d["u"], d["p"]), lambda d: nl().calc_pu(d["u"], d["p"])),
        Op("no_limits.un_pu", lambda d: oned.un_pu(d["pu"], d["p"]), lambda d: nl().un_pu(d["pu"], d["p"])),
        Op("no_limits.advec_p", lambda d: oned.advec_p(d["pu"], dx), lambda d: nl().advec_p(d["pu"], dx),
           lambda d: _amax(d["pu"]) / dx, one),
        Op("no_limits.advec_pu", lambda d: oned.advec_pu(d["p"], d["pu"], d["u"], dx),
           lambda d: nl().advec_pu(d["p"], d["pu"], d["u"], dx), lambda d: _amax(d["u"]) ** 2 * _amax(d["p"]) / dx, one),
        Op("no_limits.advec_t", lambda d: oned.advec_t(d["pu"], d["t"], dx), lambda d: nl().advec_t(d["pu"], d["t"], dx),
           lambda d: _amax(d["pu"]) * _amax(d["t"]) / dx, one),
        Op("no_limits.pgf", lambda d: oned.pgf(d["p"], d["t"], dx), lambda d: nl().pgf(d["p"], d["t"], dx), zero_when=one),
    ]
    sc = (SC[0],)
    for name in AXIS_FORMS:
        ops.append(Op("two_d.%s(1-D)" % name,
                      lambda d, name=name: getattr(tracer, name)(DT, sc, d["V"], d["q"], 0),
                      lambda d, name=name: getattr(_mod("two_d"), name)(DT, sc, d["V"], d["q"], 0),
                      _axis_floor(name, 0, sc), one if name.endswith("_finite") else None))
    ops += [
        Op("two_d.pressure_at_edge_one_d(1-D)", lambda d: tracer.pressure_at_edge_one_d(d["p"]),
           lambda d: _mod("two_d").pressure_at_edge_one_d(d["p"])),
        Op("two_d.pgf_one_d(1-D)", lambda d: tracer.pgf_one_d(DT, SC[0], d["p"]),
           lambda d: _mod("two_d").pgf_one_d(DT, SC[0], d["p"]), zero_when=one),
    ]
    return ops


def ops_elementwise():
    dx = ELEMENTWISE_DX
    mt, tm = lambda: _mod("matsumo_temp"), lambda: _mod("temperature")
    return [
        Op("matsumo_temp.density_from", lambda d: sw2d_temp.density_from(d["p"], d["t"]),
           lambda d: mt().density_from(d["p"], d["t"])),
        Op("matsumo_temp.potential_temperature", lambda d: temperature.to_potential_temp(d["t"], d["p"]),
           lambda d: mt().potential_temperature(d["p"], d["t"])),
        Op("matsumo_temp.scaling", lambda d: sw2d_temp.scaling(d["p"], d["t"], dx), lambda d: mt().scaling(d["p"], d["t"], dx)),
        Op("matsumo_temp.unscaling", lambda d: sw2d_temp.unscaling(d["pb"], d["scaled"], dx),
           lambda d: mt().unscaling(d["pb"], d["scaled"], dx)),
        Op("matsumo_temp.geopotential_from", lambda d: sw2d_temp.geopotential_from(d["rho"], d["p"]),
           lambda d: mt().geopotential_from(d["rho"], d["p"])),
        Op("temperature.to_true_temp", lambda d: temperature.to_true_temp(d["t"], d["p"]),
           lambda d: tm().to_true_temp(d["t"], d["p"])),
        Op("temperature.to_potential_temp", lambda d: temperature.to_potential_temp(d["t"], d["p"]),
           lambda d: tm().to_potential_temp(d["t"], d["p"])),
        Op("temperature.to_density", lambda d: temperature.to_density(d["t"], d["p"]),
           lambda d: tm().to_density(d["t"], d["p"])),
    ]


# ---- flux_limiter: bit for bit --------------------------------------------------------------------
def ops_flux_limiter():
    """(name, ref(d), run(d)); d from inputs_flux_limiter"""
    fl = lambda: _mod("flux_limiter")
    return [
        ("flux_limiter.van_leer", lambda d: tracer.van_leer(d["q"]), lambda d: fl().van_leer(d["q"])),
        ("flux_limiter.van_leer(inf, nan)", lambda d: tracer.van_leer(d["special"]), lambda d: fl().van_leer(d["special"])),
        ("flux_limiter.calc_r", lambda d: tracer.calc_r(d["q"]), lambda d: fl().calc_r(d["q"])),
        ("flux_limiter.calc_r(inf, nan)", lambda d: tracer.calc_r(d["special"]), lambda d: fl().calc_r(d["special"])),
        ("flux_limiter.donor_cell_flux", lambda d: tracer.donor_cell_flux(d["q"], d["u"]),
         lambda d: fl().donor_cell_flux(d["q"], d["u"])),
        ("flux_limiter.donor_cell_advection", lambda d: tracer.donor_cell_advection(d["q"], d["u"], d["dx"], d["dt"]),
         lambda d: fl().donor_cell_advection(d["q"], d["u"], d["dx"], d["dt"])),
    ]


def same_bits(got, want):
    """np.array_equal with NaN equal to NaN, and the signs of the zeros equal as well (array_equal alone takes
    -0.0 for 0.0, which is all that the strict `u > 0` changes where u is exactly zero)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != np.float64 or want.dtype != np.float64 or got.shape != want.shape:
        return False
    if not np.array_equal(got, want, equal_nan=True):
        return False
    ok = ~np.isnan(want)
    return bool(np.array_equal(np.signbit(got[ok]), np.signbit(want[ok])))
