"""Shapes, inputs, operator table and the row-by-row error rule for the PE25D operator drop-ins of
gcmiipy_amd/dynamics.py (calc_pu, calc_pv, un_pu, un_pv, aflux, advec_sig, advec_m_pu, compute_geopotential, pgf,
advec_t: gcm_pe25d_op, csrc/pe25d_ops.hip).  test_pe25d_operator_dropins_gpu.py holds each drop-in to its oracle
function on these cases; test_pe25d_operator_cases_cpu.py shows that the cases and the rule are not vacuous.

The cell kernel runs one thread per cell in workgroups of 256 cells of the flat [k][j][i] array, the column
kernel (aflux, compute_geopotential) one thread per column in workgroups of 256 columns of the flat [j][i] map.

Why the scale is taken per latitude row: dx_h of the last row is cos(90 deg) C / W, some 3e-10 m, so dvt of a
random v is some 1e14 there and some 0.04 everywhere else.  L-inf over the largest reference value (conftest.rel_err)
then checks the pole row alone."""
import importlib

import numpy as np

from operator_dropin_cases import FLOOR_FACTOR, Op, SENSITIVITY_MAX, TOL, as_longdouble, err  # noqa: F401
from oracle import dynamics as od, geometry as ogeo, grid, temperature as otemp
from oracle.constants import Cp, G, P0, Rd, kappa

SHAPES = (              # (H, W, L)
    (1, 1, 1),          # every neighbour is the cell itself, in i, j and k
    (1, 2, 1),          # along the row the neighbour is the one other cell: i+1 is i-1
    (2, 1, 2),          # the same along the column and in k: j+1 is j-1, k+1 is k-1
    (2, 3, 2),          # three columns: i+2 is i-1 (the diagonals of dut / dvt); two rows, two levels
    (3, 2, 3),          # the same with the extents exchanged
    (1, 256, 1),        # exactly one workgroup of either kernel
    (1, 257, 2),        # a second column block that holds one column; a last cell block that holds 2 cells
    (4, 64, 3),         # one column block; cell blocks end on row 3 / row 0 of a level, so j+-1 and k+-1 cross them
    (5, 65, 2),         # the column seam falls inside row 3; every wrap partner in i, j and k lies in another block
    (3, 130, 5),        # 390 columns, 1950 cells: seams at ragged places in every level, the i wrap across a seam
    (67, 9, 3),         # many rows on a narrow grid: the j wrap is 2.3 blocks away, a block holds 28 rows
    (6, 10, 24),        # the product's level count, for the two column scans
)
PTOPS = (0.0, 5000.0)
CASES = tuple((s, ptop) for s in SHAPES for ptop in PTOPS)


def case_id(case):
    (H, W, L), ptop = case
    return "%dx%dx%d-ptop%g" % (H, W, L, ptop)


# ---- inputs -------------------------------------------------------------------------------------
def geom_of(d):
    """the geometry of an input dict as the attribute bag that the oracle and the drop-ins both read (in the
    dict's own number format)"""
    L, H, W = d["u"].shape
    g = ogeo.Geom(H, W, L)
    for k in ("dx_j", "dx_h", "dsig", "sig", "sigb", "sigt", "heightmap", "dy", "ptop"):
        setattr(g, k, d[k])
    return g


def inputs(case):
    """The distributions of test_dynamics_operators_gpu.py, seeded from the shape: p about 1e5 - ptop, theta from
    T about 300, a seeded heightmap of up to 50 m.  v is random everywhere, v0 is v with the pole row (the last)
    zero; sd is the sigma-dot of aflux (from v), sdr is random in every level, level 0 included.  The
    geometry's tables ride in the same dict, so that as_longdouble widens them with the fields."""
    (H, W, L), ptop = case
    rng = np.random.default_rng((H * 1000 + W) * 100 + L)
    og = ogeo.gen_geometry(H, W, L, sig_func=ogeo.manabe_sig)
    og.heightmap = 50 * rng.random((H, W))
    og.ptop = ptop
    p = 1e5 - ptop + 100 * rng.standard_normal((H, W))
    u, v = rng.standard_normal((L, H, W)), rng.standard_normal((L, H, W))
    t = otemp.to_potential_temp(300 + rng.standard_normal((L, H, W)), p * og.sig + ptop)
    sdr = rng.standard_normal((L, H, W))
    v0 = v.copy()
    v0[:, -1, :] = 0.0
    d = dict(p=p, u=u, v=v, v0=v0, t=t, sdr=sdr, pu=od.calc_pu(p, u), pv=od.calc_pv(p, v), pv0=od.calc_pv(p, v0),
             dy=np.float64(og.dy), ptop=np.float64(ptop))
    for k in ("dx_j", "dx_h", "dsig", "sig", "sigb", "sigt", "heightmap"):
        d[k] = getattr(og, k)
    d["sd"] = od.aflux(d["pu"], d["pv"], og)[1]
    return d


# ---- the error rule -----------------------------------------------------------------------------
def row_errors(got, want, floor=0.0, zero_rows=None, dtype=np.float64):
    """Per latitude row -- each (k, j) of a 3-D output, each j of a 2-D one -- max_i |got - want| over
    max(max_i |want|, floor of that row); the absolute error where that scale is zero (conftest.rel_err's rule for a
    zero reference).  In the rows of `zero_rows` the reference must be exactly zero, and so must the result: anything
    else is an infinite error.  (dtype: long double where the oracle is compared with itself.)"""
    want = np.asarray(want, dtype=dtype)
    got = np.asarray(got, dtype=dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = np.max(np.abs(got - want), axis=-1)
    scale = np.maximum(np.max(np.abs(want), axis=-1), np.broadcast_to(np.asarray(floor, dtype=dtype), diff.shape))
    e = np.where(scale == 0, diff, diff / np.where(scale == 0, 1.0, scale)).astype(np.float64)
    if zero_rows is not None:
        exact = ~np.any(want != 0, axis=-1) & ~np.any(got != 0, axis=-1)
        e = np.where(np.broadcast_to(zero_rows, e.shape) & ~exact, np.inf, e)
    return e


def worst(e):
    """the largest row error; NaN if any row is NaN"""
    return float(np.max(e)) if not np.any(np.isnan(e)) else float("nan")


def _rowmax(*terms):
    """the largest |term| of each row: the floor's raw material"""
    return np.max(np.stack([np.max(np.abs(np.asarray(x, dtype=np.float64)), axis=-1) for x in terms]), axis=0)


class RowOp(Op):
    """an Op judged row by row: floor(d) is one value per row, and zero_rows(d) marks the rows in which the
    reference is exactly zero by construction (all of them where zero_when(shape) holds)"""

    def __init__(self, name, ref, run, floor=None, zero_when=None, zero_rows=None):
        Op.__init__(self, name, ref, run, floor, zero_when)
        self._zero_rows = zero_rows

    def zero_rows(self, d, rows_shape):
        L, H, W = d["u"].shape
        if self.zero_when((H, W, L)):
            return np.ones(rows_shape, dtype=bool)
        if self._zero_rows is None:
            return np.zeros(rows_shape, dtype=bool)
        return np.broadcast_to(self._zero_rows(d), rows_shape)

    def errors(self, got, want, d, dtype=np.float64):
        want = np.asarray(want)
        return row_errors(got, want, self.floor(d), self.zero_rows(d, want.shape[:-1]), dtype)


# ---- floors: FLOOR_FACTOR times the largest term that enters the difference, in that row --------------
# (operator_dropin_cases.py: where the neighbours are the cell itself, or cancel by symmetry, the reference is zero
# or nearly so, and what the kernel leaves behind is one rounding of a term.)  The terms are the oracle's own
# subexpressions of the inputs, each over that row's own dx_j, dx_h or dy.
def _floor_dut(vkey, pvkey):
    def floor(d):
        u, pu, pv = d["u"], d["pu"], d[pvkey]
        puum = grid.imh(u) * grid.imh(pu)
        puvp = grid.iph(pv) * grid.jph(u)
        return _rowmax(puum / d["dx_j"], grid.ipj(puum) / d["dx_j"], puvp / d["dy"], grid.ijm(puvp) / d["dy"])
    return floor


def _floor_dvt(vkey, pvkey):
    def floor(d):
        v, pu, pv = d[vkey], d["pu"], d[pvkey]
        pvvm = grid.jmh(v) * grid.jmh(pv)
        pvup = grid.iph(v) * grid.jph(pu)
        return _rowmax(pvvm / d["dy"], grid.ijp(pvvm) / d["dy"], pvup / d["dx_h"], grid.imj(pvup) / d["dx_h"])
    return floor


def _floor_advec_t(pvkey):
    def floor(d):
        tpu, tpv = d["pu"] * grid.iph(d["t"]), d[pvkey] * grid.jph(d["t"])
        return _rowmax(tpu / d["dx_j"], grid.imj(tpu) / d["dx_j"], tpv / d["dy"], grid.ijm(tpv) / d["dy"])
    return floor


def _floor_conv(pvkey, three_d):
    def floor(d):
        pu, pv = d["pu"], d[pvkey]
        f = _rowmax(pu / d["dx_j"] * d["dsig"], grid.imj(pu) / d["dx_j"] * d["dsig"], pv / d["dy"] * d["dsig"],
                    grid.ijm(pv) / d["dy"] * d["dsig"])                  # (L, H): per level
        f = np.max(f, axis=0)                                            # pit and sd sum over the levels
        return np.broadcast_to(f, (pu.shape[0],) + f.shape) if three_d else f
    return floor


def _floor_advec_sig(sd, q):
    def floor(d):
        flux = grid.kmh(q(d)) * sd(d)
        return _rowmax(flux / d["dsig"], grid.kp(flux) / d["dsig"])
    return floor


# ---- the operator table ---------------------------------------------------------------------------
def _dyn():
    return importlib.import_module("gcmiipy_amd.dynamics")


_one_cell = lambda s: s[0] == 1 and s[1] == 1       # (H, W, L): every horizontal neighbour is the cell itself
# dut differences puum = imh(u) imh(pu) along i and puvp = iph(pv) jph(u) along j.  On two columns imh() is the same
# in both (i-1 is i+1), so the i term vanishes on W <= 2 as on W == 1; the j term vanishes on one row only (on two,
# iph(pv) still differs between them).  dvt likewise with the axes exchanged.
_dut_zero = lambda s: s[0] == 1 and s[1] <= 2
_dvt_zero = lambda s: s[0] <= 2 and s[1] == 1
_one_col = lambda s: s[1] == 1
_one_row = lambda s: s[0] == 1
_one_level = lambda s: s[2] == 1
_pole_row = lambda d: (np.arange(d["u"].shape[1]) == d["u"].shape[1] - 1)[None, :]        # (1, H) against (L, H)
_level_0 = lambda d: (np.arange(d["u"].shape[0]) == 0)[:, None]                            # (L, 1)


def ops():
    """one RowOp per output.  Where v0 is used, its pole row is zero: calc_pv and un_pv give exactly zero there."""
    dyn, g = _dyn, geom_of
    table = [
        RowOp("calc_pu", lambda d: od.calc_pu(d["p"], d["u"]), lambda d: dyn().calc_pu(d["p"], d["u"], g(d))),
        RowOp("calc_pv", lambda d: od.calc_pv(d["p"], d["v"]), lambda d: dyn().calc_pv(d["p"], d["v"], g(d))),
        RowOp("calc_pv[v0]", lambda d: od.calc_pv(d["p"], d["v0"]), lambda d: dyn().calc_pv(d["p"], d["v0"], g(d)),
              zero_when=_one_row, zero_rows=_pole_row),
        RowOp("un_pu", lambda d: od.un_pu(d["pu"], d["p"]), lambda d: dyn().un_pu(d["pu"], d["p"], g(d))),
        RowOp("un_pv", lambda d: od.un_pv(d["pv"], d["p"]), lambda d: dyn().un_pv(d["pv"], d["p"], g(d))),
        RowOp("un_pv[v0]", lambda d: od.un_pv(d["pv0"], d["p"]), lambda d: dyn().un_pv(d["pv0"], d["p"], g(d)),
              zero_when=_one_row, zero_rows=_pole_row),
        RowOp("compute_geopotential", lambda d: od.compute_geopotential(d["p"], d["t"], g(d)),
              lambda d: dyn().compute_geopotential(d["p"], d["t"], g(d))),
    ]
    for tag, vkey, pvkey in (("", "v", "pv"), ("[v0]", "v0", "pv0")):
        table += [
            RowOp("aflux.pit" + tag, lambda d, pvkey=pvkey: od.aflux(d["pu"], d[pvkey], g(d))[0],
                  lambda d, pvkey=pvkey: dyn().aflux(d["pu"], d[pvkey], g(d))[0], _floor_conv(pvkey, False), _one_cell),
            # sd[0] is set to zero; with one level that is all of sd
            RowOp("aflux.sd" + tag, lambda d, pvkey=pvkey: od.aflux(d["pu"], d[pvkey], g(d))[1],
                  lambda d, pvkey=pvkey: dyn().aflux(d["pu"], d[pvkey], g(d))[1], _floor_conv(pvkey, True),
                  lambda s: _one_cell(s) or _one_level(s), _level_0),
            RowOp("advec_m_pu.dut" + tag,
                  lambda d, vkey=vkey, pvkey=pvkey: od.advec_m_pu(d["p"], d["u"], d[vkey], d["pu"], d[pvkey], g(d))[0],
                  lambda d, vkey=vkey, pvkey=pvkey: dyn().advec_m_pu(d["p"], d["u"], d[vkey], d["pu"], d[pvkey], g(d))[0],
                  _floor_dut(vkey, pvkey), _dut_zero),
            RowOp("advec_m_pu.dvt" + tag,
                  lambda d, vkey=vkey, pvkey=pvkey: od.advec_m_pu(d["p"], d["u"], d[vkey], d["pu"], d[pvkey], g(d))[1],
                  lambda d, vkey=vkey, pvkey=pvkey: dyn().advec_m_pu(d["p"], d["u"], d[vkey], d["pu"], d[pvkey], g(d))[1],
                  # (with v0 on one row every v and pv is zero; on two rows the j term vanishes, and in v0's pole row
                  # iph(v0) is zero: nothing is left there)
                  _floor_dvt(vkey, pvkey), (lambda s: _one_row(s) or _dvt_zero(s)) if tag else _dvt_zero,
                  (lambda d: _pole_row(d) & (d["u"].shape[1] <= 2)) if tag else None),
            RowOp("advec_t" + tag, lambda d, pvkey=pvkey: od.advec_t(d["pu"], d[pvkey], d["t"], g(d)),
                  lambda d, pvkey=pvkey: dyn().advec_t(d["pu"], d[pvkey], d["t"], g(d)), _floor_advec_t(pvkey), _one_cell),
        ]
    # advec_sig: a flux difference in k that wraps from level L-1 to level 0.  With the sd of aflux the wrapped flux is
    # zero (sd[0] == 0) whatever the kernel reads, and on one cell that sd is zero altogether; sdr shows the wrap.
    # On u and v the step passes iph(sd) and jph(sd).
    for name, sd, q, zero in (
            ("advec_sig(sd, t)", lambda d: d["sd"], lambda d: d["t"], lambda s: _one_level(s) or _one_cell(s)),
            ("advec_sig(iph sd, u)", lambda d: grid.iph(d["sd"]), lambda d: d["u"], lambda s: _one_level(s) or _one_cell(s)),
            # (one column of two rows: conv of the one is minus conv of the other, and jph(sd) is exactly zero)
            ("advec_sig(jph sd, v)", lambda d: grid.jph(d["sd"]), lambda d: d["v"],
             lambda s: _one_level(s) or _one_cell(s) or (s[0] == 2 and s[1] == 1)),
            ("advec_sig(sdr, t)", lambda d: d["sdr"], lambda d: d["t"], _one_level),
            ("advec_sig(iph sdr, u)", lambda d: grid.iph(d["sdr"]), lambda d: d["u"], _one_level),
            ("advec_sig(jph sdr, v)", lambda d: grid.jph(d["sdr"]), lambda d: d["v"], _one_level)):
        table.append(RowOp(name, lambda d, sd=sd, q=q: od.advec_sig(sd(d), q(d), g(d)),
                           lambda d, sd=sd, q=q: dyn().advec_sig(np.asarray(sd(d)), q(d), g(d)),
                           _floor_advec_sig(sd, q), zero))
    # pgf: the gradients subtract two loaded values (p) or two values of phi, then multiply: an exact zero where the
    # neighbour is the cell itself, and no floor
    for n, (name, zero) in enumerate((("pgf.pgfu", _one_col), ("pgf.pgfv", _one_row), ("pgf.phiu", _one_col),
                                      ("pgf.phiv", _one_row))):
        table.append(RowOp(name, lambda d, n=n: od.pgf(d["p"], d["t"], g(d))[n],
                           lambda d, n=n: dyn().pgf(d["p"], d["t"], g(d))[n], zero_when=zero))
    return table


def hold(table, d, refs=None):
    """every drop-in of the table on the inputs d by the row-by-row rule: [(name, worst row error)], the references
    from `refs` where given"""
    return [(op.name, worst(op.errors(op.run(d), np.asarray(op.ref(d)) if refs is None else refs[op.name], d)))
            for op in table]


# ---- the oracle's operators restated, each with the places a kernel can get wrong exposed ---------------
def r_aflux(d, pvkey="pv", i_shift=1, j_shift=1, zero_sd0=True, sigb="sigb"):
    pu, pv = d["pu"], d[pvkey]
    conv = ((pu - np.roll(pu, i_shift, -1)) / d["dx_j"] + (pv - np.roll(pv, j_shift, -2)) / d["dy"]) * d["dsig"]
    pit = np.sum(conv, 0)
    sd = np.cumsum(conv[::-1], 0)[::-1] - pit * d[sigb]
    if zero_sd0:
        sd[0] = 0
    return pit, sd


def r_advec_sig(sd, q, d, wrap=True):
    flux = grid.kmh(q) * sd
    above = grid.kp(flux)
    if not wrap:
        above[-1] = 0.0                             # nothing comes back in from level 0
    return -((flux - above) / d["dsig"])


def r_advec_m_pu(d, vkey="v", pvkey="pv", dx_h="dx_h", dx_h_rows=None, puup_shift=-1, puvm_shift=1, pvvp_shift=-1,
                 pvum_shift=1):
    """dx_h: the table dvt divides by; dx_h_rows: the rows in which that holds (all by default)"""
    u, v, pu, pv = d["u"], d[vkey], d["pu"], d[pvkey]
    puum = grid.imh(u) * grid.imh(pu)
    puup = np.roll(puum, puup_shift, -1)
    puvp = grid.iph(pv) * grid.jph(u)
    puvm = np.roll(puvp, puvm_shift, -2)
    pvvm = grid.jmh(v) * grid.jmh(pv)
    pvvp = np.roll(pvvm, pvvp_shift, -2)
    pvup = grid.iph(v) * grid.jph(pu)
    pvum = np.roll(pvup, pvum_shift, -1)
    dxh = d[dx_h] if dx_h_rows is None else np.where(dx_h_rows[None, :, None], d[dx_h], d["dx_h"])
    dut = (puum - puup) / d["dx_j"] + (puvm - puvp) / d["dy"] + 0.0
    dvt = (pvvm - pvvp) / d["dy"] + (pvum - pvup) / dxh + 0.0
    return dut, dvt


def r_advec_t(d, pvkey="pv", i_shift=1, j_shift=1):
    tpu = d["pu"] * grid.iph(d["t"])
    tpv = d[pvkey] * grid.jph(d["t"])
    return (tpu - np.roll(tpu, i_shift, -1)) / d["dx_j"] + (tpv - np.roll(tpv, j_shift, -2)) / d["dy"]


def r_geopotential(d, ptop_in_pk=True, heightmap=True, kph_wrap=True, sigt="sigt"):
    p, t, sig = d["p"], d["t"], d["sig"]
    tp = p * sig + d["ptop"]
    tt = otemp.to_true_temp(t, tp)
    rho = tp / (Rd * tt)
    s1 = sig * p / rho * d["dsig"]
    pkdn = ((sig * p + (d["ptop"] if ptop_in_pk else 0.0)) / P0) ** kappa
    pkup = grid.kp(pkdn)
    tk = grid.kph(t)
    if not kph_wrap:
        tk[-1] = t[-1]                              # the top level averaged with itself, not with level 0
    stp = Cp * tk * (pkdn - pkup)
    s2 = d[sigt] * stp
    stp_n = grid.km(stp)
    stp_n[0] = np.sum(s1 - s2, 0) + (d["heightmap"] if heightmap else 0.0) * G
    return np.cumsum(stp_n, 0)


def r_pgf(d, ptop_in_rho=True, **geopotential):
    p, t, sig = d["p"], d["t"], d["sig"]
    tp = p * sig + (d["ptop"] if ptop_in_rho else 0.0)
    tt = otemp.to_true_temp(t, tp)
    rho = tp / (Rd * tt)
    sp = sig * p
    phi = r_geopotential(d, **geopotential)
    phiu = grid.iph(p) * grid.gradi(phi, d["dx_j"])
    phiv = grid.jph(p) * grid.gradj(phi, d["dy"])
    pgfu = grid.iph(sp) / grid.iph(rho) * grid.gradi(p, d["dx_j"])
    pgfv = grid.jph(sp) / grid.jph(rho) * grid.gradj(p, d["dy"])
    return pgfu, pgfv, phiu, phiv
