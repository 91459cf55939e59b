"""The cases and the row-by-row rule of pe25d_operator_cases.py are not vacuous (no GPU needed): the oracle is well
conditioned on them row by row, a reference is zero exactly where the table says so, deliberately wrong variants of
the operators miss the oracle wherever the fault can show, and the rule rejects two faults in dvt that the rule of
test_dynamics_operators_gpu.py (L-inf over the largest reference value) accepts.  Also the refusals of gcm_pe25d_op
and of the drop-ins, which return before any device call."""
import ctypes as C
import functools

import numpy as np
import pytest

import pe25d_operator_cases as pc
from conftest import rel_err
from oracle import dynamics as od

IDS = [pc.case_id(c) for c in pc.CASES]


@functools.lru_cache(maxsize=None)
def case(c):
    d = pc.inputs(c)
    for a in d.values():
        a.setflags(write=False)
    return d


def test_case_list_is_the_one_the_kernels_need():
    assert set(pc.SHAPES) == {(1, 1, 1), (1, 2, 1), (2, 1, 2), (2, 3, 2), (3, 2, 3), (1, 256, 1), (1, 257, 2), (4, 64, 3),
                              (5, 65, 2), (3, 130, 5), (67, 9, 3), (6, 10, 24)}
    assert pc.PTOPS == (0.0, 5000.0) and len(pc.CASES) == 24
    assert max(h * w * l for h, w, l in pc.SHAPES) <= 2010
    assert pc.TOL == 1e-10
    for c in pc.CASES:
        (H, W, L), ptop = c
        d = case(c)
        assert d["ptop"] == ptop and abs(np.mean(d["p"]) + ptop - 1e5) < 300
        assert np.any(d["v"][:, -1] != 0) and not np.any(d["v0"][:, -1]) and np.array_equal(d["v0"][:, :-1], d["v"][:, :-1])
        assert not np.any(d["sd"][0]) and np.all(d["sdr"][0] != 0)
        assert d["dx_h"][0, -1, 0] < 1e-8 < 1e3 < d["dx_j"][0, -1, 0]        # the pole row's dx_h: cos(90 deg) C / W
        assert np.all(d["heightmap"] >= 0) and np.max(d["heightmap"]) > 5


def test_oracle_sensitivity_zero_references_and_floors():
    """float64 against long double on the same inputs, judged row by row: the inputs do not use up the bound.  A
    reference is identically zero exactly where the operator says it must be, and a row of it exactly where
    zero_rows says.  Everywhere else the reference of every row lies above its floor on these cases: the floor
    loosens no bound here, it only keeps the scale of a row from collapsing."""
    table = pc.ops()
    sens, floors = {}, []
    for c in pc.CASES:
        d = case(c)
        wide_d = pc.as_longdouble(d)
        (H, W, L), _ = c
        for op in table:
            want, wide = np.asarray(op.ref(d)), np.asarray(op.ref(wide_d))
            assert wide.dtype == np.longdouble and want.dtype == np.float64, (op, c)
            s = pc.worst(op.errors(want, wide, wide_d, dtype=np.longdouble))
            assert s < pc.SENSITIVITY_MAX, (op, c, s)
            if s >= sens.get(op.name, (0.0,))[0]:
                sens[op.name] = (s, pc.case_id(c))
            assert (not np.any(want)) == op.zero_when((H, W, L)), (op, c)
            rows = op.zero_rows(d, want.shape[:-1])
            assert np.array_equal(rows, ~np.any(want != 0, axis=-1)), (op, c)
            decides = (np.broadcast_to(op.floor(d), rows.shape) > np.max(np.abs(want), axis=-1)) & ~rows
            if np.any(decides):
                floors.append((op.name, pc.case_id(c), int(np.count_nonzero(decides)), decides.size))
    for name, (s, where) in sens.items():
        print("oracle sensitivity per row, worst of %-24s %.2e  (%s)" % (name, s, where))
    print("rows in which the floor, not the reference, sets the scale:", floors or "none")
    assert not floors, floors


def test_zero_references_are_the_small_extents():
    """named outright: which outputs vanish at which shapes"""
    zero = {}
    for op in pc.ops():
        for s in pc.SHAPES:
            if not np.any(op.ref(case((s, 0.0)))):
                zero.setdefault(s, set()).add(op.name)
    sd_family = {"aflux.sd", "aflux.sd[v0]", "advec_sig(sd, t)", "advec_sig(iph sd, u)", "advec_sig(jph sd, v)"}
    one_level = sd_family | {"advec_sig(sdr, t)", "advec_sig(iph sdr, u)", "advec_sig(jph sdr, v)"}
    one_row = {"calc_pv[v0]", "un_pv[v0]", "advec_m_pu.dvt[v0]", "pgf.pgfv", "pgf.phiv"}
    one_col = {"pgf.pgfu", "pgf.phiu"}
    dut = {"advec_m_pu.dut", "advec_m_pu.dut[v0]"}
    assert set(zero) == {(1, 1, 1), (1, 2, 1), (2, 1, 2), (1, 256, 1), (1, 257, 2)}
    assert zero[(1, 1, 1)] == one_level | one_row | one_col | dut | {
        "advec_m_pu.dvt", "aflux.pit", "aflux.pit[v0]", "advec_t", "advec_t[v0]"}
    assert zero[(1, 2, 1)] == one_level | one_row | dut
    assert zero[(2, 1, 2)] == one_col | {"advec_m_pu.dvt", "advec_m_pu.dvt[v0]", "advec_sig(jph sd, v)"}
    assert zero[(1, 256, 1)] == one_level | one_row
    assert zero[(1, 257, 2)] == one_row


def test_row_rule():
    want = np.array([[1.0, 2.0], [1e-8, 0.0], [0.0, 0.0]])
    got = want + np.array([[0.0, 2e-10], [1e-19, 0.0], [0.0, 0.0]])
    assert np.allclose(pc.row_errors(got, want), [1e-10, 1e-11, 0.0], rtol=1e-6)
    assert np.allclose(pc.row_errors(got, want, floor=[4.0, 1e-7, 1.0]), [5e-11, 1e-12, 0.0], rtol=1e-6)
    assert pc.row_errors(want + 1e-300, want)[2] == 1e-300               # a zero scale: the absolute error
    z = np.array([False, False, True])
    assert pc.row_errors(want, want, zero_rows=z)[2] == 0.0
    assert pc.row_errors(want + 1e-300, want, zero_rows=z, floor=1.0)[2] == np.inf      # no floor excuses a must-be zero
    assert pc.row_errors(want, want, zero_rows=~z)[0] == np.inf          # a reference that is not zero where it must be
    assert np.isnan(pc.worst(pc.row_errors(want * np.array([[1.0], [np.nan], [1.0]]), want)))
    assert rel_err(got, want) == pc.err(got, want) == pc.worst(pc.row_errors(got, want)[:1])     # one row: the old rule


# ---- planted mistakes -----------------------------------------------------------------------------
def missed(e):
    return not e <= pc.TOL                      # a NaN result is a miss


def judge(op_names, got, d, refs):
    """the worst row error of `got` (one array per name) over the named outputs"""
    by_name = {op.name: op for op in pc.ops()}
    return max((pc.worst(by_name[n].errors(g, refs[n], d)) for n, g in zip(op_names, got)),
               key=lambda e: (e != e, e))


@functools.lru_cache(maxsize=None)
def references(c):
    d = case(c)
    return {op.name: np.asarray(op.ref(d)) for op in pc.ops()}


def faults():
    """(name, outputs judged, the faulty restatement, where the fault can show: (H, W, L), ptop -> bool).  The cases
    where it cannot are the complement, each for the reason given here."""
    AM, AF, PG = ("advec_m_pu.dut", "advec_m_pu.dvt"), ("aflux.pit", "aflux.sd"), ("pgf.pgfu", "pgf.pgfv", "pgf.phiu", "pgf.phiv")
    sdr = lambda d: (d["sdr"], d["t"])
    return [
        # the i term of dvt, the only one over dx_h, vanishes on one column
        ("dvt over dx_j", AM, lambda d: pc.r_advec_m_pu(d, dx_h="dx_j"), lambda s, ptop: s[1] >= 2),
        # i+1 and i-1 are one cell on W <= 2, j+1 and j-1 on H <= 2
        ("dut: puum read at i-1 for i+1", AM, lambda d: pc.r_advec_m_pu(d, puup_shift=1), lambda s, ptop: s[1] >= 3),
        ("dut: puvp read at j+1 for j-1", AM, lambda d: pc.r_advec_m_pu(d, puvm_shift=-1), lambda s, ptop: s[0] >= 3),
        ("dvt: pvvm read at j-1 for j+1", AM, lambda d: pc.r_advec_m_pu(d, pvvp_shift=1), lambda s, ptop: s[0] >= 3),
        ("dvt: pvup read at i+1 for i-1", AM, lambda d: pc.r_advec_m_pu(d, pvum_shift=-1), lambda s, ptop: s[1] >= 3),
        ("advec_t: tpu read at i+1 for i-1", ("advec_t",), lambda d: (pc.r_advec_t(d, i_shift=-1),), lambda s, ptop: s[1] >= 3),
        ("advec_t: tpv read at j+1 for j-1", ("advec_t",), lambda d: (pc.r_advec_t(d, j_shift=-1),), lambda s, ptop: s[0] >= 3),
        ("conv: pu read at i+1 for i-1", AF, lambda d: pc.r_aflux(d, i_shift=-1), lambda s, ptop: s[1] >= 3),
        ("conv: pv read at j+1 for j-1", AF, lambda d: pc.r_aflux(d, j_shift=-1), lambda s, ptop: s[0] >= 3),
        # with a random sd the flux through the bottom of level 0 is not zero, at any level count
        ("advec_sig: no wrap in k, random sd", ("advec_sig(sdr, t)",), lambda d: (pc.r_advec_sig(*sdr(d), d, wrap=False),),
         lambda s, ptop: True),
        # with the sd of aflux that flux is zero: the fault can show nowhere (why sdr is among the inputs)
        ("advec_sig: no wrap in k, sd of aflux", ("advec_sig(sd, t)",),
         lambda d: (pc.r_advec_sig(d["sd"], d["t"], d, wrap=False),), lambda s, ptop: False),
        # what is left in sd[0] is sum(conv) in descending order minus sum(conv) in ascending order times sigb[0] == 1:
        # zero for one level, and for two (a + b is b + a); from three levels on the two orders round differently in
        # some column
        ("sd[0] not zeroed", AF, lambda d: pc.r_aflux(d, zero_sd0=False), lambda s, ptop: s[2] >= 3),
        # sigb enters sd above level 0 only, times pit, which vanishes on one cell
        ("sigt for sigb in sd", AF, lambda d: pc.r_aflux(d, sigb="sigt"), lambda s, ptop: s[2] >= 2 and s[:2] != (1, 1)),
        ("sig for sigb in sd", AF, lambda d: pc.r_aflux(d, sigb="sig"), lambda s, ptop: s[2] >= 2 and s[:2] != (1, 1)),
        # sigt multiplies stp, which is a difference of pk between levels: zero on one level.  On two levels stp[1] is
        # -stp[0] (k+1 is k-1), sigt is (1/2, 0) and sigb (1, 1/2): both column sums are stp[0] / 2, to rounding
        ("sigb for sigt in the geopotential", ("compute_geopotential",), lambda d: (pc.r_geopotential(d, sigt="sigb"),),
         lambda s, ptop: s[2] >= 3),
        # rho reaches pgfu and pgfv only, which vanish on one column / one row; ptop == 0 has nothing to drop
        ("ptop dropped from rho of pgf", PG, lambda d: pc.r_pgf(d, ptop_in_rho=False),
         lambda s, ptop: ptop != 0 and s[:2] != (1, 1)),
        # pk enters through its difference between levels
        ("ptop dropped from pk of the geopotential", ("compute_geopotential",),
         lambda d: (pc.r_geopotential(d, ptop_in_pk=False),), lambda s, ptop: ptop != 0 and s[2] >= 2),
        ("heightmap dropped (phi)", ("compute_geopotential",), lambda d: (pc.r_geopotential(d, heightmap=False),),
         lambda s, ptop: True),
        # phiu and phiv difference phi between neighbours
        ("heightmap dropped (pgf)", PG, lambda d: pc.r_pgf(d, heightmap=False), lambda s, ptop: s[:2] != (1, 1)),
        # kph(t) at the top level enters stp[L-1] alone, which is multiplied by sigt[L-1] == 0 in the column sum and
        # whose place in the shifted array is overwritten by that sum: the wrap cannot show in any case
        ("kph(t) without its wrap at the top", ("compute_geopotential",), lambda d: (pc.r_geopotential(d, kph_wrap=False),),
         lambda s, ptop: False),
    ]


def test_restatements_are_the_oracle():
    for c in pc.CASES:
        d, refs = case(c), references(c)
        g = pc.geom_of(d)
        same = lambda a, b: np.array_equal(np.asarray(a), np.asarray(b))
        for tag, vkey, pvkey in (("", "v", "pv"), ("[v0]", "v0", "pv0")):
            pit, sd = pc.r_aflux(d, pvkey)
            assert same(pit, refs["aflux.pit" + tag]) and same(sd, refs["aflux.sd" + tag]), c
            dut, dvt = pc.r_advec_m_pu(d, vkey, pvkey)
            assert same(dut, refs["advec_m_pu.dut" + tag]) and same(dvt, refs["advec_m_pu.dvt" + tag]), c
            assert same(pc.r_advec_t(d, pvkey), refs["advec_t" + tag]), c
        assert same(pc.r_advec_sig(d["sd"], d["t"], d), refs["advec_sig(sd, t)"]), c
        assert same(pc.r_advec_sig(d["sdr"], d["t"], d), refs["advec_sig(sdr, t)"]), c
        assert same(pc.r_geopotential(d), refs["compute_geopotential"]), c
        for got, name in zip(pc.r_pgf(d), ("pgf.pgfu", "pgf.pgfv", "pgf.phiu", "pgf.phiv")):
            assert same(got, refs[name]), (c, name)
        assert same(od.advec_sig(d["sd"], d["t"], g), refs["advec_sig(sd, t)"])


@pytest.mark.parametrize("c", pc.CASES, ids=IDS)
def test_planted_mistakes_miss_the_oracle(c):
    """every fault is rejected at every case where it can show; where it cannot, the faulty operator is the oracle to
    the last bits (so `can show` is neither too wide nor too narrow)"""
    d, refs = case(c), references(c)
    shape, ptop = c
    for name, outputs, wrong, can_show in faults():
        got = wrong(d)
        e = judge(outputs, got, d, refs)
        print("%-18s %-42s %s %.2e" % (pc.case_id(c), name, "shows " if can_show(shape, ptop) else "cannot", e))
        if can_show(shape, ptop):
            assert missed(e), (name, c, e)
        else:
            assert e < 1e-15, (name, c, e)


# ---- the old rule against the new -------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in pc.CASES if c[0][0] >= 2 and c[0][1] >= 2], ids=pc.case_id)
def test_old_rule_accepts_what_the_row_rule_rejects(c):
    """dvt of a random v is some 1e14 in the pole row and some 0.04 elsewhere, so 1e-10 of the largest reference value
    is thousands in absolute terms.  Two faults confined to the other rows pass the old rule and miss the new one: every
    row but the pole row rolled by one column, and dx_j for dx_h in every row but the pole row.  (dx_j for dx_h in
    the pole row as well changes that row by seventeen orders of magnitude, which the old rule sees too: asserted.)
    Cases of one row have no other row, cases of one column nothing to roll."""
    d, refs = case(c), references(c)
    (H, W, L), _ = c
    want = refs["advec_m_pu.dvt"]
    dvt_op = {op.name: op for op in pc.ops()}["advec_m_pu.dvt"]
    new = lambda got: pc.worst(dvt_op.errors(got, want, d))
    rolled = want.copy()
    rolled[:, :-1] = np.roll(want[:, :-1], 1, -1)
    not_pole = np.arange(H) < H - 1
    off_pole = pc.r_advec_m_pu(d, dx_h="dx_j", dx_h_rows=not_pole)[1]
    everywhere = pc.r_advec_m_pu(d, dx_h="dx_j")[1]
    for label, got in (("rolled", rolled), ("dx_j off the pole row", off_pole)):
        old_e, new_e = rel_err(got, want), new(got)
        print("%-16s %-22s old rule %.2e, row rule %.2e" % (pc.case_id(c), label, old_e, new_e))
        assert old_e < 1e-10 and missed(new_e), (label, c, old_e, new_e)
    assert np.array_equal(everywhere[:, :-1], off_pole[:, :-1])
    assert rel_err(everywhere, want) > 0.99 and missed(new(everywhere))


# ---- refusals: before any device call -----------------------------------------------------------------
def _call(kind, W, H, L, geom, ins, outs):
    from gcmiipy_amd import _lib
    pin = None if ins is None else (C.c_void_p * 5)(*[None if a is None else a.ctypes.data for a in ins])
    pout = None if outs is None else (C.c_void_p * 4)(*[None if a is None else a.ctypes.data for a in outs])
    rc = _lib.lib.gcm_pe25d_op(kind, W, H, L, None if geom is None else C.addressof(geom),
                               None if pin is None else C.byref(pin), None if pout is None else C.byref(pout))
    return rc, _lib.lib.gcm_pe25d_op_last_error().decode()


def test_refusals_of_the_entry_point_leave_the_outputs_untouched():
    from gcmiipy_amd import _lib
    H, W, L = 3, 4, 2
    tabs = dict(dx_j=np.ones(H), dx_h=np.ones(H), dsig=np.ones(L), sig=np.ones(L), sigb=np.ones(L), sigt=np.ones(L))
    hm = np.zeros((H, W))

    def geom(dy=1.0, missing=None):
        return _lib.PeGeom(*[None if k == missing else tabs[k].ctypes.data for k in tabs], hm.ctypes.data, dy, 0.0)

    ins = [np.ones((L, H, W)) for _ in range(5)]
    # per kind: inputs, outputs (pe25d_ops.hip)
    counts = {_lib.PEOP_CALC_PU: (2, 1), _lib.PEOP_CALC_PV: (2, 1), _lib.PEOP_UN_PU: (2, 1), _lib.PEOP_UN_PV: (2, 1),
              _lib.PEOP_AFLUX: (2, 2), _lib.PEOP_ADVEC_SIG: (2, 1), _lib.PEOP_ADVEC_M_PU: (5, 2),
              _lib.PEOP_GEOPOTENTIAL: (2, 1), _lib.PEOP_PGF: (2, 4), _lib.PEOP_ADVEC_T: (3, 1)}
    assert sorted(counts) == list(range(10)) and _lib.PEOP_ADVEC_T == 9

    def refused(label, kind, W=W, H=H, L=L, g=None, ins=ins, null_out=None, no_out=False, no_geom=False):
        outs = [np.full((L, max(H, 1), max(W, 1)), 7.25) for _ in range(4)]
        passed = None if no_out else [None if n == null_out else o for n, o in enumerate(outs)]
        g = g or geom()
        rc, msg = _call(kind, W, H, L, None if no_geom else g, ins, passed)
        assert rc == _lib.ERR_ARG, (label, rc)
        assert msg.startswith("gcm_pe25d_op: ") and len(msg) > len("gcm_pe25d_op: "), (label, msg)
        assert all(np.all(o == 7.25) for o in outs), label
        return msg

    refused("kind -1", -1)
    refused("kind past the last", _lib.PEOP_ADVEC_T + 1)
    for kind in counts:
        refused("width 0", kind, W=0)
        refused("height 0", kind, H=0)
        refused("layers 0", kind, L=0)
        refused("width -1", kind, W=-1)
        refused("null geometry", kind, no_geom=True)
        for k in tabs:
            assert "geometry" in refused("no " + k, kind, g=geom(missing=k))
        assert "geometry" in refused("dy == 0", kind, g=geom(dy=0.0))
        refused("dy == -0", kind, g=geom(dy=-0.0))
        nin, nout = counts[kind]
        for n in range(nin):
            assert "input" in refused("null input %d" % n, kind, ins=[None if m == n else a for m, a in enumerate(ins)])
        for n in range(nout):
            assert "output" in refused("null output %d" % n, kind, null_out=n)
        refused("no input array", kind, ins=None)
        refused("no output array", kind, no_out=True)


def test_drop_ins_refuse_a_wrong_operand_shape():
    """ValueError from each of the ten, for each operand in turn, before anything reaches the library"""
    from gcmiipy_amd import dynamics as dyn
    d = case(((2, 3, 2), 0.0))
    g = pc.geom_of(d)
    p, u, v, t, pu, pv, sd = (d[k] for k in ("p", "u", "v", "t", "pu", "pv", "sd"))
    calls = [
        (dyn.calc_pu, (p, u)), (dyn.calc_pv, (p, v)), (dyn.un_pu, (pu, p)), (dyn.un_pv, (pv, p)), (dyn.aflux, (pu, pv)),
        (dyn.advec_sig, (sd, t)), (dyn.advec_m_pu, (p, u, v, pu, pv)), (dyn.compute_geopotential, (p, t)),
        (dyn.pgf, (p, t)), (dyn.advec_t, (pu, pv, t)),
    ]
    assert len({f.__name__ for f, _ in calls}) == 10

    def bad_shapes(a):
        yield a[..., :-1]                                   # one column short
        yield a[..., :-1, :]                                # one row short
        yield a[0] if a.ndim == 3 else np.broadcast_to(a, (2,) + a.shape)      # a map for a field, a field for a map
        if a.ndim == 3:
            yield a[:-1]                                    # one level short

    n = 0
    for f, args in calls:
        for k in range(len(args)):
            for bad in bad_shapes(args[k]):
                with pytest.raises(ValueError):
                    f(*(args[:k] + (bad,) + args[k + 1:]), g)
                n += 1
    for f, args in calls[:4]:                               # the forms without a geometry: the grid is the field's shape
        a3 = 1 if f.__name__.startswith("calc") else 0
        with pytest.raises(ValueError):
            f(*[a[0] if k == a3 else a for k, a in enumerate(args)])             # no [k, j, i] array to take it from
        with pytest.raises(ValueError):
            f(*[a[:, :-1] if k != a3 else a for k, a in enumerate(args)])        # p does not match it
        n += 2
    print("%d malformed calls refused" % n)
