"""The parity cases that can see every term of a time step -- TEST INFRASTRUCTURE, a plain helper module.

A parity test compares the GPU's state after a few steps with the float64 oracle's, within a tolerance: 1e-10
relative (L-inf over max|reference|) for fp64, a measured bound per field for fp32.  A term whose share of the
state stays below that tolerance is invisible to the test: the kernel may drop it and still pass.  Each CASE
below names a kernel path, the inputs and the tolerance of one GPU comparison; tests/test_terms_gpu.py runs
every case on the GPU against `oracle_run(case)`, and tests/test_term_visibility_cpu.py shows, through the
oracle's named term hooks (oracle/terms.py), that for every path of PATHS each term moves some field by far
more than the case's tolerance.

The viscosity of SW2D_TEMP, mu lap(u) / rho, is the one term that does not scale with dt/dx alone: at the
dx = 300 km of the older tests it is ~1e-13 of u.  The SW2D_TEMP cases here keep dt / dx = 1e-3 (300 s / 300 km)
and shrink dx, which leaves every other term as it was and raises the viscosity's share as 1/dx: about 6e-3 of
u per step at dx = 1e-5 m, 6e-2 at 1e-6 m, with a diffusion number mu dt / (rho dx^2) of 1.5e-2 at most.
"""
from collections import namedtuple

import numpy as np

from test_sw2d_f32_gpu import F32_STEP as SW2D_F32_STEP
from test_pe25d_variants_gpu import F32_STEP as PE_F32_STEP, F32_PT as PE_F32_PT

TOL = 1e-10
DX_SMALL = 1e-5            # SW2D_TEMP: viscosity ~6e-3 of u per step
DX_TINY = 1e-6             # the theta-spread fp32 case: ~6e-2
TRACER_NAMES = {0: "none", 1: "upwind", 2: "van_leer"}

# fp32 SW2D_TEMP with a theta spread of 30 K (dx = 1e-6), one step: theta's increment is 2.6e-2 of theta (5e-5 with
# the 1 K spread of the other cases), so the theta bound below covers ~1e-5 of it.  Measured on an MI355X
# (test_terms_gpu.py, fused with 1 and 2 columns per lane and staged, W 96 and 97): u 7.7e-7, v 8.4e-7, p 8.5e-8,
# t 1.3e-7; the bounds leave 2-3x.
F32_THETA30 = {"u": 2e-6, "v": 2e-6, "p": 2e-7, "t": 3e-7}

Case = namedtuple("Case", "name model path shape seed dx dt steps dtype tracer extra")


def _case(name, model, path, shape, seed, dx, dt, steps, dtype="f64", tracer=0, **extra):
    return Case(name, model, path, shape, seed, dx, dt, steps, dtype, tracer, extra)


def _temp_cases():
    out = []
    dx, dt = DX_SMALL, 1e-3 * DX_SMALL
    # fp64 fused (the handle's own rows per band, GCM_FUSED_ROWS = 3 and 16) and staged, every tracer scheme
    for path, extra in (("fused", {}), ("fused_rows3", {"rows": 3}), ("fused_rows16", {"rows": 16}),
                        ("staged", {})):
        for tr in (0, 1, 2):
            out.append(_case("temp_%s_%s" % (path, TRACER_NAMES[tr]), "sw2d_temp", path, (33, 97), 100 + tr,
                             dx, dt, 2, tracer=tr, **extra))
    # the staged predictor alone: half_step(0) / get_star
    out.append(_case("temp_staged_half", "sw2d_temp", "staged_half", (33, 97), 110, dx, dt, 1))
    # the matsumo_temp.matsumo_scheme drop-in
    out.append(_case("temp_dropin", "sw2d_temp", "dropin", (33, 97), 111, dx, dt, 2))
    # three latitude bands stepped by the host loop (step_interior / step_boundary), ghost rows by device copies
    for tr in (0, 2):
        out.append(_case("temp_band3_%s" % TRACER_NAMES[tr], "sw2d_temp", "band", (37, 130), 112 + tr, dx, dt, 2,
                         tracer=tr, bands=3))
    # the STREAM instantiation of the fused kernel: 32 members of 360x720 with van Leer read > 256 MB per launch
    out.append(_case("temp_stream", "sw2d_temp", "stream", (360, 720), 120, dx, dt, 1, tracer=2, members=32,
                     picks=(0, 17, 31)))
    # fp32, fused with one and two columns per lane (GCM_SW2D_F32_COLS), even and odd widths (odd: one column)
    for cols in (1, 2):
        for W in (96, 97):
            for tr in (0, 1, 2):
                out.append(_case("temp_f32_cols%d_w%d_%s" % (cols, W, TRACER_NAMES[tr]), "sw2d_temp",
                                 "f32_cols%d" % cols, (33, W), 130 + W + tr, dx, dt, 1, "f32", tr, cols=cols))
    # fp32, theta spread 30 K: theta's increment is large enough for its bound to mean something
    for label, extra in (("cols1", {"cols": 1}), ("cols2", {"cols": 2}), ("staged", {"staged": True})):
        for W in (96, 97):
            out.append(_case("temp_f32_theta30_%s_w%d" % (label, W), "sw2d_temp", "f32_theta30", (33, W), 140 + W,
                             DX_TINY, 1e-3 * DX_TINY, 1, "f32", 0, theta_sigma=30.0, **extra))
    return out


def _sw2d_geometry_cases():
    """plain SW2D on the fused kernels the handle's own choice at (33, 97) does not reach.  `plan`: what Core.sw2d_plan
    of the case's step count must report (the runner asserts it before it steps), `min_rows`: a lower bound on its
    rows_per_band where the heuristic picks them"""
    out = []
    dx, dt = 300e3, 300.0
    # pinned rows: 3 and 4 take a two-step launch (sw2d_fused2_kernel) and a leftover step of the preloading kernel,
    # 8 and 16 two steps of the rolling kernel
    for rows, steps in ((3, 3), (4, 3), (8, 2), (16, 2)):
        pairs = steps // 2 if rows <= 4 else 0
        out.append(_case("sw2d_fused_rows%d" % rows, "sw2d", "fused_rows%d" % rows, (33, 97), 210 + rows, dx, dt, steps,
                         rows=rows, plan=dict(variant="fused", rows_per_band=rows, cols=1, strip=60, strip2=56,
                                              two_step_launches=pairs, single_step_launches=steps - 2 * pairs,
                                              preload=rows <= 4, stream=False)))
    # three latitude bands stepped by the host loop: the non-wrapping kernels, preloading (the bands' own 2 rows) and
    # rolling (8 rows)
    out.append(_case("sw2d_band3", "sw2d", "band", (37, 130), 230, dx, dt, 2, bands=3, max_rows=4,
                     plan=dict(variant="fused", two_step_launches=0, single_step_launches=1, preload=True,
                               stream=False)))
    out.append(_case("sw2d_band3_rows8", "sw2d", "band", (37, 130), 231, dx, dt, 2, bands=3, rows=8,
                     plan=dict(variant="fused", rows_per_band=8, two_step_launches=0, single_step_launches=1,
                               preload=False, stream=False)))
    # the STREAM instantiation of the rolling kernel: 48 members of 360x720 read 48 * 360 * 720 * 3 * 8 B = 299 MB per
    # launch, and a grid that fills the chip gets bands of 8 rows at least
    out.append(_case("sw2d_stream", "sw2d", "stream", (360, 720), 240, dx, dt, 1, members=48, picks=(0, 23, 47),
                     min_rows=8, plan=dict(variant="fused", cols=1, strip=60, two_step_launches=0,
                                           single_step_launches=1, preload=False, stream=True)))
    # fp32 through the two-step kernel: the handle's own 2-row bands, one two-step launch
    for cols in (1, 2):
        out.append(_case("sw2d_f32_two_step_cols%d" % cols, "sw2d", "f32_two_step", (33, 96), 250, dx, dt, 2, "f32",
                         cols=cols, max_rows=4, plan=dict(variant="fused", cols=cols, strip=60 * cols, strip2=56,
                                                          two_step_launches=1, single_step_launches=0,
                                                          preload=True, stream=False)))
    return out


def check_plan(case, plan):
    """a case's `plan`, `min_rows` and `max_rows` against what Core.sw2d_plan reported"""
    want = case.extra["plan"]
    assert {k: plan[k] for k in want} == want, (case.name, plan)
    assert case.extra.get("min_rows", 1) <= plan["rows_per_band"] <= case.extra.get("max_rows", 1 << 30), \
        (case.name, plan)


def _other_cases():
    out = []
    for path in ("fused", "staged"):
        out.append(_case("sw2d_%s" % path, "sw2d", path, (33, 97), 200, 300e3, 300.0, 3))
    for cols in (1, 2):
        out.append(_case("sw2d_f32_cols%d" % cols, "sw2d", "f32_cols%d" % cols, (33, 96), 201, 300e3, 300.0, 1,
                         "f32", cols=cols))
    out += _sw2d_geometry_cases()
    out.append(_case("pe2d", "pe2d", "core", (33, 130), 300, 100e3, 100.0, 3))
    out.append(_case("oned", "oned", "run", (257,), 400, 5e4, 60.0, 3))
    out.append(_case("pe25d", "pe25d", "core", (5, 12, 20), 500, None, 60.0, 2))
    out.append(_case("pe25d_coriolis", "pe25d", "coriolis", (5, 12, 20), 501, None, 60.0, 2, coriolis=True))
    out.append(_case("pe25d_f32", "pe25d", "f32", (3, 12, 120), 502, None, 60.0, 1, "f32"))
    return out


CASES = _temp_cases() + _other_cases()

_SW2D_TEMP = ("adv_u", "pgf_u", "visc_u", "adv_v", "pgf_v", "visc_v", "adv_p", "adv_t")
_SW2D = ("adv_u", "pgf_u", "adv_v", "pgf_v", "adv_p")
_TRACER = ("flux_j", "flux_i", "vanleer_j", "vanleer_i")
_PE25D = ("pit", "dut", "dus", "pgu", "phiu", "dvt", "dvs", "pgv", "phiv", "advec_t", "advec_sig_t",
          "advec_q", "advec_sig_q", "filter_spu", "filter_pgfu")

# path -> (dtype, the terms every path must show): the audit's contract.  A path with no case, or whose cases
# cannot see one of its terms, fails tests/test_term_visibility_cpu.py.
PATHS = {
    ("sw2d_temp", "fused"): ("f64", _SW2D_TEMP + _TRACER),
    ("sw2d_temp", "fused_rows3"): ("f64", _SW2D_TEMP + _TRACER),
    ("sw2d_temp", "fused_rows16"): ("f64", _SW2D_TEMP + _TRACER),
    ("sw2d_temp", "staged"): ("f64", _SW2D_TEMP + _TRACER),
    ("sw2d_temp", "staged_half"): ("f64", _SW2D_TEMP),
    ("sw2d_temp", "dropin"): ("f64", _SW2D_TEMP),
    ("sw2d_temp", "band"): ("f64", _SW2D_TEMP + _TRACER),
    ("sw2d_temp", "stream"): ("f64", _SW2D_TEMP + _TRACER),
    ("sw2d_temp", "f32_cols1"): ("f32", _SW2D_TEMP + _TRACER),
    ("sw2d_temp", "f32_cols2"): ("f32", _SW2D_TEMP + _TRACER),
    ("sw2d_temp", "f32_theta30"): ("f32", _SW2D_TEMP),
    ("sw2d", "fused"): ("f64", _SW2D),
    ("sw2d", "staged"): ("f64", _SW2D),
    ("sw2d", "f32_cols1"): ("f32", _SW2D),
    ("sw2d", "f32_cols2"): ("f32", _SW2D),
    ("sw2d", "fused_rows3"): ("f64", _SW2D),
    ("sw2d", "fused_rows4"): ("f64", _SW2D),
    ("sw2d", "fused_rows8"): ("f64", _SW2D),
    ("sw2d", "fused_rows16"): ("f64", _SW2D),
    ("sw2d", "band"): ("f64", _SW2D),
    ("sw2d", "stream"): ("f64", _SW2D),
    ("sw2d", "f32_two_step"): ("f32", _SW2D),
    ("pe2d", "core"): ("f64", ("advec_p", "dut", "pgfu", "dvt", "pgfv", "advec_t")),
    ("oned", "run"): ("f64", ("advec_q", "advec_p", "advec_pu", "pgf", "advec_t")),
    ("pe25d", "core"): ("f64", _PE25D),
    ("pe25d", "coriolis"): ("f64", _PE25D + ("coriolis_u", "coriolis_v")),
    ("pe25d", "f32"): ("f32", _PE25D),
}

_TRACER_TERMS = set(_TRACER)


def fields(case):
    """the fields a case compares, in the order oracle_run returns them"""
    if case.model == "sw2d":
        return "uvp"
    if case.model == "oned":
        return "putq"
    if case.model in ("pe2d", "pe25d"):
        return "puvtq"
    return "uvpt" + ("q" if case.tracer else "")


def bound(case, field):
    """the tolerance of one field of a case (rel_err, L-inf over max|reference|)"""
    if case.dtype == "f64":
        return TOL
    if case.path == "f32_theta30":
        return F32_THETA30[field] * case.steps
    if case.model == "pe25d":
        return (PE_F32_PT if field in "pt" else PE_F32_STEP) * case.steps
    return SW2D_F32_STEP[1 if case.model == "sw2d" else 2][field] * case.steps


def _r32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def pe25d_geometry(case, product=False):
    """the oracle's (or, product=True, the package's) geometry of a PE25D case"""
    L, H, W = case.shape
    if product:
        from gcmiipy_amd import geometry
        return geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    from oracle import geometry as ogeo
    return ogeo.gen_geometry(H, W, L, sig_func=ogeo.manabe_sig)


def state(case):
    """the initial state of a case: dict name -> array, (M, H, W) for an ensemble, float32-rounded for fp32"""
    rng = np.random.default_rng(case.seed)
    if case.model in ("sw2d", "sw2d_temp"):
        M = case.extra.get("members")
        shape = case.shape if M is None else (M,) + case.shape
        s = {"u": rng.standard_normal(shape), "v": rng.standard_normal(shape)}
        if case.model == "sw2d":
            s["p"] = 8000 + rng.standard_normal(shape)
        else:
            s["p"] = 101325 + 10 * rng.standard_normal(shape)
            s["t"] = 273.16 + case.extra.get("theta_sigma", 1.0) * rng.standard_normal(shape)
            if case.tracer:
                s["q"] = rng.random(shape)
    elif case.model == "pe2d":
        s = {"p": 101325 + 10 * rng.standard_normal(case.shape), "u": rng.standard_normal(case.shape),
             "v": rng.standard_normal(case.shape), "t": 300 + rng.standard_normal(case.shape),
             "q": rng.random(case.shape)}
    elif case.model == "oned":
        n = case.shape[0]
        s = {"p": 90000.0 + 5000.0 * rng.random(n), "u": 20.0 * rng.standard_normal(n),
             "t": 300.0 + 10.0 * rng.random(n), "q": rng.random(n)}
    else:
        from oracle import temperature as otemp
        og = pe25d_geometry(case)
        L, H, W = case.shape
        p = 1e5 + 10 * rng.standard_normal((H, W))
        v = rng.standard_normal((L, H, W))
        v[:, -1, :] = 0
        s = {"p": p, "u": rng.standard_normal((L, H, W)), "v": v,
             "t": otemp.to_potential_temp(300 + rng.standard_normal((L, H, W)), p * og.sig + og.ptop),
             "q": 3e-6 * (1 + 0.1 * rng.random((L, H, W)))}
    if case.dtype == "f32":
        s = {k: _r32(a) for k, a in s.items()}
    return s


def _split(terms):
    """(the model's terms, the tracer's terms) of a `_terms` mapping"""
    if not terms:
        return None, None
    return ({k: x for k, x in terms.items() if k not in _TRACER_TERMS} or None,
            {k: x for k, x in terms.items() if k in _TRACER_TERMS} or None)


def _oracle_2d(case, s, terms):
    from oracle import sw2d, sw2d_temp, tracer as otr
    dx, dt = case.dx, case.dt
    mt, tt = _split(terms)
    if case.model == "sw2d":
        st = (s["u"], s["v"], s["p"])
        for _ in range(case.steps):
            st = sw2d.matsumo_scheme(*st, dx, dt, _terms=mt)
        return st
    st, q = (s["u"], s["v"], s["p"], s["t"]), s.get("q")
    if case.path == "staged_half":
        return sw2d_temp.predictor(*st, dx, dt, _terms=mt)
    for _ in range(case.steps):
        if case.tracer:                                  # the time-n winds, V[0] along j
            q = otr.limited_advection(dt, (dx, dx), np.stack([st[1], st[0]]), q, limiter=case.tracer == 2,
                                      _terms=tt)
        st = sw2d_temp.matsumo_scheme(*st, dx, dt, _terms=mt)
    return st + ((q,) if case.tracer else ())


def oracle_run(case, terms=None, members=None):
    """the float64 oracle's result of a case, a tuple in the order of fields(case); an ensemble case: a list,
    one tuple per member of `members` (default: the case's picks)"""
    s = state(case)
    if case.extra.get("members"):
        return [_oracle_2d(case, {k: a[m] for k, a in s.items()}, terms)
                for m in (members if members is not None else case.extra["picks"])]
    if case.model in ("sw2d", "sw2d_temp"):
        return _oracle_2d(case, s, terms)
    if case.model == "pe2d":
        from oracle import pe2d
        st = tuple(s[k] for k in "puvtq")
        for _ in range(case.steps):
            st = pe2d.matsuno_timestep(*st, case.dt, case.dx, _terms=terms)
        return st
    if case.model == "oned":
        from oracle import oned
        st = tuple(s[k] for k in "putq")
        for _ in range(case.steps):
            st = oned.matsuno_timestep(*st, case.dt, case.dx, _terms=terms)
        return st
    from oracle import dynamics
    og = pe25d_geometry(case)
    st = tuple(s[k] for k in "puvtq")
    for _ in range(case.steps):
        st = dynamics.matsuno_timestep(*st, case.dt, og, coriolis=case.extra.get("coriolis", False), _terms=terms)
    return st
