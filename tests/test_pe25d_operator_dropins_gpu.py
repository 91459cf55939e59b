"""GPU parity of the PE25D operator drop-ins (gcmiipy_amd/dynamics.py behind gcm_pe25d_op: pe_op_cell_kernel and
pe_op_col_kernel of csrc/pe25d_ops.hip) against the oracle, row by row, at the cases of pe25d_operator_cases.py:
extents 1, 2 and 3 in W, H and L, workgroup seams, the product's level count, ptop 0 and 5000 Pa.  Also the call
forms without a geometry, the null heightmap, the scratch arena on a fresh thread, and golden g7 under the row rule.
test_pe25d_operator_cases_cpu.py shows that the cases and the rule can tell a wrong kernel from a right one."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import pe25d_operator_cases as pc
from conftest import golden

pytestmark = pytest.mark.gpu
TOL = pc.TOL


@functools.lru_cache(maxsize=None)
def case(c):
    """inputs and oracle results of one case, computed once and read-only"""
    d = pc.inputs(c)
    refs = {op.name: np.asarray(op.ref(d)) for op in pc.ops()}
    for a in list(d.values()) + list(refs.values()):
        a.setflags(write=False)
    return d, refs


def report(label, errors):
    """print every error, then assert them all"""
    for name, e in errors:
        print("%-18s %-26s %.2e" % (label, name, e))
    missed = [(name, e) for name, e in errors if not e < TOL]
    assert not missed, (label, missed)


@pytest.mark.parametrize("c", pc.CASES, ids=pc.case_id)
def test_every_operator_vs_oracle_row_by_row(c):
    d, refs = case(c)
    report(pc.case_id(c), pc.hold(pc.ops(), d, refs))


@pytest.mark.parametrize("c", pc.CASES, ids=pc.case_id)
def test_forms_without_geometry_and_inverses(c):
    """calc_pu(p, u) and the like take the grid from the arrays: the same bits as with a geometry.  un_pu undoes
    calc_pu, un_pv calc_pv, by the row rule against u and v."""
    from gcmiipy_amd import dynamics as dyn
    d, _ = case(c)
    g = pc.geom_of(d)
    p, u, v, pu, pv = (d[k] for k in ("p", "u", "v", "pu", "pv"))
    for f, a, b in ((dyn.calc_pu, p, u), (dyn.calc_pv, p, v), (dyn.un_pu, pu, p), (dyn.un_pv, pv, p)):
        bare, full = f(a, b), f(a, b, g)
        assert bare.dtype == np.float64 and np.array_equal(bare, full), (f.__name__, c)
    report(pc.case_id(c), [("un_pu(calc_pu)", pc.worst(pc.row_errors(dyn.un_pu(dyn.calc_pu(p, u), p), u))),
                           ("un_pv(calc_pv)", pc.worst(pc.row_errors(dyn.un_pv(dyn.calc_pv(p, v), p), v)))])


# ---- the null heightmap, through the C entry point ---------------------------------------------------
def _raw(kind, d, nout, heightmap):
    """gcm_pe25d_op(kind) on (p, t) with the tables of d; heightmap: an array, or None for a null pointer"""
    from gcmiipy_amd import _lib
    L, H, W = d["u"].shape
    tabs = [np.ascontiguousarray(d[k], dtype=np.float64).reshape(-1) for k in ("dx_j", "dx_h", "dsig", "sig", "sigb", "sigt")]
    g = _lib.PeGeom(*[t.ctypes.data for t in tabs], None if heightmap is None else heightmap.ctypes.data,
                    float(d["dy"]), float(d["ptop"]))
    ins = [np.ascontiguousarray(d["p"]), np.ascontiguousarray(d["t"])]
    outs = [np.full((L, H, W), np.nan) for _ in range(nout)]
    pin = (C.c_void_p * 5)(*([a.ctypes.data for a in ins] + [None] * 3))
    pout = (C.c_void_p * 4)(*([o.ctypes.data for o in outs] + [None] * (4 - nout)))
    rc = _lib.lib.gcm_pe25d_op(kind, W, H, L, C.addressof(g), C.byref(pin), C.byref(pout))
    assert rc == _lib.OK, (rc, _lib.lib.gcm_pe25d_op_last_error().decode())
    return outs


@pytest.mark.parametrize("c", [((2, 3, 2), 5000.0), ((5, 65, 2), 0.0)], ids=pc.case_id)
def test_null_heightmap_is_a_zero_heightmap(c):
    from gcmiipy_amd import _lib
    d, refs = case(c)
    flat = np.zeros_like(d["heightmap"])
    for kind, nout in ((_lib.PEOP_GEOPOTENTIAL, 1), (_lib.PEOP_PGF, 4)):
        null, zero = _raw(kind, d, nout, None), _raw(kind, d, nout, flat)
        assert all(np.all(np.isfinite(a)) for a in null)
        assert all(np.array_equal(a, b) for a, b in zip(null, zero)), (kind, c)
    # and the heightmap is not ignored: with the case's own the entry point gives the oracle's phi
    own = _raw(_lib.PEOP_GEOPOTENTIAL, d, 1, np.ascontiguousarray(d["heightmap"]))[0]
    assert np.any(d["heightmap"]) and not np.array_equal(own, _raw(_lib.PEOP_GEOPOTENTIAL, d, 1, None)[0])
    phi = {op.name: op for op in pc.ops()}["compute_geopotential"]
    report(pc.case_id(c), [("phi, own heightmap", pc.worst(phi.errors(own, refs["compute_geopotential"], d)))])


# ---- the scratch arena (csrc/dev_arena.h), on a thread that has none yet ------------------------------
ARENA_SHAPE = (20, 60, 20)      # 24 000 cells: under the 33 800 that test_operator_dropin_cases_cpu.py pins


def test_scratch_arena_on_a_fresh_thread():
    """pgf takes phi as an extra operand after its inputs and outputs.  A new thread's arena starts empty and its first
    block is 1 MiB: pgf at (67, 9, 3), at (3, 130, 5) and at (67, 9, 3) again are a call that allocates the arena, a
    call of another shape in it, and a call that reuses it.  At (20, 60, 20) the tables, p, t and the four outputs
    take 960 KB of that MiB and phi (188 KB) lands in a second block in the middle of the call; the end of the call
    merges the two, and the same call again runs in the merged block."""
    from gcmiipy_amd import dynamics as dyn
    H, W, L = ARENA_SHAPE
    n2, n3 = 8 * H * W, 8 * H * W * L
    fixed = 256 * 8 + 6 * 256 + 2 * ((n2 + 255) // 256 * 256)            # exner table, six tables, heightmap and p
    assert n3 % 256 == 0 and fixed + 5 * n3 <= (1 << 20) < fixed + 6 * n3
    order = [((67, 9, 3), 5000.0), ((3, 130, 5), 5000.0), ((67, 9, 3), 5000.0), (ARENA_SHAPE, 5000.0), (ARENA_SHAPE, 5000.0)]
    got, failure = [], []

    def work():
        try:
            for c in order:
                d, _ = case(c)
                got.append(dyn.pgf(d["p"], d["t"], pc.geom_of(d)))
        except BaseException as e:          # (reported by the test's own thread)
            failure.append(e)

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert not failure, failure
    names = ("pgf.pgfu", "pgf.pgfv", "pgf.phiu", "pgf.phiv")
    by_name = {op.name: op for op in pc.ops()}
    errors = []
    for n, (c, outs) in enumerate(zip(order, got)):
        d, refs = case(c)
        errors += [("call %d %s" % (n, name), pc.worst(by_name[name].errors(o, refs[name], d))) for name, o in zip(names, outs)]
    same = [all(np.array_equal(a, b) for a, b in zip(got[i], got[j])) for i, j in ((0, 2), (3, 4))]
    print("arena: first and third call bit-identical: %s; outgrowing and reusing call bit-identical: %s" % tuple(same))
    report("arena", errors)
    assert all(same), same


# ---- golden g7 again, by the row rule ---------------------------------------------------------------
@pytest.mark.parametrize("stage", ["pred", "corr"])
def test_every_intermediate_of_a_half_step_vs_golden_row_by_row(stage):
    """every comparison of test_dynamics_operators_gpu.py::test_every_intermediate_of_a_half_step_vs_golden, the
    reference's own intermediates as the yardstick, each row on its own scale"""
    from gcmiipy_amd import geometry, dynamics as dyn
    gd = golden("g7_half_step")
    L, H, W = gd["u0"].shape
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    sp, su, sv, st, _ = [gd[k + "0"] for k in "puvtq"] if stage == "pred" else [gd["pred_%s_n" % k] for k in "puvtq"]
    g = lambda k: gd["%s_%s" % (stage, k)]
    d = dict(p=sp, u=su, v=sv, t=st, pu=g("spu"), pv=g("spv"), sd=g("sd"), dy=np.float64(geom.dy), ptop=np.float64(0.0),
             heightmap=np.array(gd["heightmap"], dtype=np.float64))
    for k in ("dx_j", "dx_h", "dsig", "sig", "sigb", "sigt"):
        d[k] = getattr(geom, k)
    refs = {"calc_pu": g("spu_orig"), "calc_pv": g("spv"), "aflux.pit": g("pit"), "aflux.sd": g("sd"),
            "advec_m_pu.dut": g("dut"), "advec_m_pu.dvt": g("dvt"), "compute_geopotential": g("phi"),
            "pgf.pgfu": g("pgu"), "pgf.pgfv": g("pgv"), "pgf.phiu": g("phiu"), "pgf.phiv": g("phiv"),
            "advec_sig(iph sd, u)": g("dus"), "advec_sig(jph sd, v)": g("dvs"), "advec_t": g("advec_t"),
            "advec_sig(sd, t)": g("advec_sig_t")}
    table = [op for op in pc.ops() if op.name in refs]
    assert len(table) == len(refs) == 15
    errors = pc.hold(table, d, refs)
    # un_pu / un_pv undo calc_pu / calc_pv on the new pressure: u_n = un_pu(pu_n, p_n) (dynamics.py:216-217)
    p_n, u_n, v_n = g("p_n"), g("u_n"), g("v_n")
    errors += [("un_pu(calc_pu)", pc.worst(pc.row_errors(dyn.un_pu(dyn.calc_pu(p_n, u_n), p_n), u_n))),
               ("un_pv(calc_pv)", pc.worst(pc.row_errors(dyn.un_pv(dyn.calc_pv(p_n, v_n), p_n), v_n)))]
    report("g7 " + stage, errors)
