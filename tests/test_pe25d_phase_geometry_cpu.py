"""What tests/test_pe25d_phase_geometry_gpu.py reaches, stated on the CPU (tests/pe25d_phase_geometry_cases.py): every
case takes the launch geometry it is named for -- from gcm_pe25d_phase_geometry, the helper the launchers themselves
take their numbers from, at 256 compute units -- and the inputs exercise what that geometry adds: a friction boundary
inside a level batch, both branches of the equilibrium temperature, forced and pinned cells in the second pass, a
condensing cell in a later level segment and the moistened level in the last one."""
import numpy as np
import pytest

import gpu_setups as su
import pe25d_held_suarez_ref as hs_ref
import pe25d_moist_ref as moist_ref
import pe25d_phase_geometry_cases as pc
from gcmiipy_amd import _lib
from gcmiipy_amd.core import phase_geometry


def _id(case):
    return "%dx%dx%d" % case.shape


# ---------------------------------------------------------------- the query itself
def test_product_grid_takes_the_paths_the_cases_are_for():
    """720 x 1440 x 24 at 256 compute units: Held-Suarez marches whole 24-level columns in six column blocks, the
    climatology walks 8 levels per workgroup in two chunk iterations, the forcing takes 24 passes in fp64 (2048 x 256
    lanes x 16 bytes = 8 MiB of a 190 MiB field each) and 12 in fp32"""
    H, W, L = pc.PRODUCT
    assert phase_geometry("held_suarez", W, H, L, pc.CUS) == dict(grid_x=6, grid_y=720, grid_z=1, levels_min=24, levels_max=24)
    assert phase_geometry("moist", W, H, L, pc.CUS, accumulate=True) == dict(grid_x=6, grid_y=720, grid_z=1, levels_min=24,
                                                                             levels_max=24)
    assert phase_geometry("climate", W, H, L, pc.CUS) == dict(grid_x=720, nseg=3, levels_min=8, levels_max=8, chunks=2)
    assert phase_geometry("tracer_forcing", W, H, L, pc.CUS, 8) == dict(groups=2048, passes=24)
    assert phase_geometry("tracer_forcing", W, H, L, pc.CUS, 4) == dict(groups=2048, passes=12)
    # the suite's two shapes: one level per workgroup, one block, one pass
    for H, W, L in ((24, 36, 9), (6, 10, 3)):
        assert phase_geometry("held_suarez", W, H, L, pc.CUS) == dict(grid_x=1, grid_y=H, grid_z=L, levels_min=1, levels_max=1)
        assert phase_geometry("climate", W, H, L, pc.CUS) == dict(grid_x=H, nseg=L, levels_min=1, levels_max=1, chunks=1)
        assert phase_geometry("tracer_forcing", W, H, L, pc.CUS, 8)["passes"] == 1


def test_query_follows_its_arguments():
    """the launchers' formulas, written out once more for a sweep of sizes and chips"""
    for W, rows, L, cus in ((36, 24, 9, 256), (257, 3, 42, 304), (1440, 720, 24, 64), (512, 29, 25, 1), (1800, 4, 42, 256)):
        xb = -(-W // 256)
        nseg = min(L, max(1, -(-2 * cus // (xb * rows))))
        sizes = [b - a for a, b in pc.segments(L, nseg)]
        want = dict(grid_x=xb, grid_y=rows, grid_z=nseg, levels_min=min(sizes), levels_max=max(sizes))
        assert phase_geometry("held_suarez", W, rows, L, cus) == want
        assert phase_geometry("moist", W, rows, L, cus, accumulate=False) == want
        assert phase_geometry("moist", W, rows, L, cus, accumulate=True) == dict(grid_x=xb, grid_y=rows, grid_z=1,
                                                                                 levels_min=L, levels_max=L)
        nseg = min(L, max(1, -(-8 * cus // rows)))
        sizes = [b - a for a, b in pc.segments(L, nseg)]
        assert phase_geometry("climate", W, rows, L, cus) == dict(grid_x=rows, nseg=nseg, levels_min=min(sizes),
                                                                  levels_max=max(sizes), chunks=-(-W // 768))
        for esz in (8, 4):
            nvec = rows * L * W // (16 // esz)
            groups = min(2048, max(1, -(-nvec // 256)))
            assert phase_geometry("tracer_forcing", W, rows, L, cus, esz) == dict(groups=groups,
                                                                                  passes=max(1, -(-nvec // (groups * 256))))


def test_query_refuses_what_it_cannot_answer():
    import ctypes as C
    out = (C.c_int * _lib.PHASE_PLAN_WORDS)()
    f = _lib.lib.gcm_pe25d_phase_geometry
    assert f(_lib.PHASE_CLIMATE, 36, 24, 9, 256, 8, 1, out, _lib.PHASE_PLAN_WORDS) == _lib.OK
    for args in ((4, 36, 24, 9, 256, 8), (-1, 36, 24, 9, 256, 8), (0, 0, 24, 9, 256, 8), (0, 36, 0, 9, 256, 8),
                 (0, 36, 24, 0, 256, 8), (0, 36, 24, 9, 0, 8), (0, 36, 24, 9, 256, 2)):
        assert f(*args, 1, out, _lib.PHASE_PLAN_WORDS) == _lib.ERR_ARG, args
    assert f(0, 36, 24, 9, 256, 8, 1, out, _lib.PHASE_PLAN_WORDS - 1) == _lib.ERR_ARG
    assert f(0, 36, 24, 9, 256, 8, 1, None, _lib.PHASE_PLAN_WORDS) == _lib.ERR_ARG
    assert _lib.lib.gcm_pe25d_phase_plan(None, 0, -1, 1, out, _lib.PHASE_PLAN_WORDS) == _lib.ERR_ARG
    with pytest.raises(ValueError):
        phase_geometry("convect", 36, 24, 9, 256)
    with pytest.raises(ValueError):
        phase_geometry("moist", 36, 24, 9, 256, elem_bytes=2)


# ---------------------------------------------------------------- Held-Suarez
def _hs_branches(geom, st, ptop):
    """(cold, warm) of pe25d_held_suarez_ref.theta_eq, (L, H, W) each, at the default parameters"""
    q = hs_ref.params()
    sig, lat = np.asarray(geom.sig).reshape(-1), np.asarray(geom.lat).reshape(-1)
    s2, c2 = (np.sin(lat) ** 2)[None, :, None], (np.cos(lat) ** 2)[None, :, None]
    p_lev = sig[:, None, None] * st[0][None] + ptop
    cold = q["T_min"] * (hs_ref.P0 / p_lev) ** hs_ref.KAPPA
    warm = (q["T_0"] - q["dT_y"] * s2) - (q["dtheta_z"] * np.log(p_lev / hs_ref.P0)) * c2
    assert np.array_equal(np.maximum(cold, warm), hs_ref.theta_eq(st[0], sig, ptop, lat))
    return cold, warm


@pytest.mark.parametrize("case", pc.HELD_SUAREZ, ids=_id)
def test_held_suarez_case(case):
    H, W, L = case.shape
    assert phase_geometry("held_suarez", W, H, L, pc.CUS) == case.plan, case.what
    segs = pc.segments(L, case.plan["grid_z"])
    assert [b - a for a, b in segs] == case.segs
    assert [pc.batches(a, b) for a, b in segs] == case.batches
    assert any(len(b) > 1 or b[0] > 1 for b in case.batches), "a batch holds a second level"
    if case.plan["grid_x"] > 1:
        assert 0 < W - 256 * (case.plan["grid_x"] - 1) < 256, "the last column block is partial"
    inside = False
    for ptop in pc.PTOPS:
        geom = su.geom_of(H, W, L, ptop)
        fr = hs_ref.r_of(geom.sig, hs_ref.DEFAULTS["sigma_b"]) > 0
        assert fr.any() and not fr.all(), "a friction level and a free level"
        # the friction boundary inside a batch: a batch with a friction level and a free level
        for a, b in segs:
            for k in range(a, b, 4):
                inside |= fr[k:min(k + 4, b)].any() and not fr[k:min(k + 4, b)].all()
        cold, warm = _hs_branches(geom, pc.state(geom, "f64"), ptop)
        assert (cold > warm).any() and (warm > cold).any(), "both branches of the equilibrium temperature"
        # ... within single columns too: the branch changes along the march of a lane
        assert ((cold > warm).any(axis=0) & (warm > cold).any(axis=0)).any()
    assert inside, "the friction boundary lies on a batch edge"


def test_held_suarez_bands_take_another_level_split():
    H, W, L = pc.HELD_SUAREZ[2].shape
    from gcmiipy_amd.bands import split_rows
    rows = {n for _, n in split_rows(H, pc.HS_BANDS)}
    assert rows == {25}
    got = phase_geometry("held_suarez", W, 25 + 2 * pc.GHOST, L, pc.CUS)
    assert got == pc.HS_BAND_PLAN and got["grid_z"] != pc.HELD_SUAREZ[2].plan["grid_z"]


# ---------------------------------------------------------------- climatology
@pytest.mark.parametrize("case", pc.CLIMATE, ids=_id)
def test_climate_case(case):
    H, W, L = case.shape
    assert phase_geometry("climate", W, H, L, pc.CUS) == case.plan, case.what
    assert 8 * (256 + 80 + W) <= 64 * 1024, "the row fits the sample's LDS"
    if case.plan["chunks"] > 1:
        n256 = -(-W // 256)
        assert n256 > 3 and W - 256 * (n256 - 1) == 160, "the last 256-column chunk is partial"
    # the two states of a case's two samples differ in every word's terms
    geom = su.geom_of(H, W, L)
    a = pc.state(geom, "f64")
    b = pc.second_state(a)
    for f in range(4):
        assert not np.array_equal(a[f], b[f])
    assert not b[2][:, -1, :].any()                       # (v of the last global row stays zero)


def test_climate_band_walks_one_level_per_workgroup():
    H, W, L = pc.CLIMATE[0].shape
    assert phase_geometry("climate", W, pc.CL_BAND_ROWS, L, pc.CUS) == pc.CL_BAND_PLAN
    assert pc.CLIMATE[0].plan["levels_max"] > 1 and pc.CLIMATE[0].plan["nseg"] > 1
    assert any(c.plan["nseg"] == 1 for c in pc.CLIMATE)     # the workgroup that reduces p, p p and then every level
    assert any(c.plan["levels_min"] != c.plan["levels_max"] for c in pc.CLIMATE)


# ---------------------------------------------------------------- tracer forcing
@pytest.mark.parametrize("case", pc.TRACER_FORCING, ids=lambda c: c.dtype)
def test_tracer_forcing_case(case):
    H, W, L = case.shape
    esz = 8 if case.dtype == "f64" else 4
    assert phase_geometry("tracer_forcing", W, H, L, pc.CUS, esz) == case.plan, case.what
    first = pc.TF_PASS_VECTORS * (16 // esz)              # elements of the first pass
    left = H * W * L - first
    assert 0 < left < first and left % (16 // esz) == 0, "the second pass is partly empty"
    assert left // (16 // esz) == 28672
    recs = pc.tf_records(case.shape)
    assert sorted(recs) == [1, 2, 3] and pc.TF_NTR == 4
    assert set(recs[1]) >= {"emission", "pin_mask"} and "pin_mask" not in recs[2] and "emission" in recs[2]
    assert "emission" not in recs[3] and "pin_mask" not in recs[3] and recs[3]["source"] != 0.0
    for i in (1, 2):
        e = pc.device_order(recs[i]["emission"])[first:]
        assert e.size == left and (e != 0).all(), "the emission is non-zero in the second pass"
        if case.dtype == "f32":
            assert (e.astype(np.float32) != 0).all()
    m = pc.device_order(recs[1]["pin_mask"])[first:]
    assert m.any() and not m.all(), "the second pass holds a pinned cell and a free one"
    # ... in one 16-byte vector as well
    v = m.reshape(-1, 16 // esz)
    assert (v.any(axis=1) & ~v.all(axis=1)).any()


# ---------------------------------------------------------------- moist physics
def test_moist_case():
    H, W, L = pc.MOIST_SHAPE
    from gcmiipy_amd.bands import split_rows
    assert {n for _, n in split_rows(H, pc.MOIST_BANDS)} == {4}
    rows = 4 + 2 * pc.GHOST
    band = phase_geometry("moist", W, rows, L, pc.CUS, accumulate=False)
    assert band == pc.MOIST_BAND_PLAN and 1 < band["grid_z"] < L
    ghost = phase_geometry("moist", W, 2 * pc.GHOST, L, pc.CUS, accumulate=False)
    assert ghost == pc.MOIST_GHOST_PLAN and 1 < ghost["grid_z"] < L
    single = phase_geometry("moist", W, H, L, pc.CUS, accumulate=False)
    assert single == pc.MOIST_SINGLE_PLAN and single["grid_z"] != band["grid_z"]
    assert phase_geometry("moist", W, rows, L, pc.CUS, accumulate=True)["grid_z"] == 1
    assert 0 < W - 256 * (band["grid_x"] - 1) < 256
    for ptop in pc.PTOPS:
        geom = pc.moist_geom(ptop)
        sig = np.asarray(geom.sig).reshape(-1)
        assert (np.diff(sig) > 0).all() and (np.asarray(geom.dsig) > 0).all()
        kb = int(np.argmax(sig))
        for plan in (band, ghost, single):
            segs = pc.segments(L, plan["grid_z"])
            assert segs[-1][0] <= kb < segs[-1][1] and segs[-1][0] > 0, "the moistened level lies in the last segment"
        for dtype in ("f64", "f32"):
            st = pc.moist_state(geom, dtype)
            p_lev, pi = moist_ref.levels(st[0], sig, ptop)
            _, qs, _, can = moist_ref.saturation(st[3] * pi, p_lev)
            cond = can & (st[4] > qs)
            k0 = pc.segments(L, band["grid_z"])[1][0]
            assert cond[k0:].any(), "a condensing cell in a segment that does not start at level 0"
            assert all(cond[a:b].any() for a, b in pc.segments(L, band["grid_z"])[1:]), "... in every later segment"
            # the surface moistens somewhere: the level's evaporation is not the identity
            tn, qn, P, E = moist_ref.moist_step(st[0], st[3], st[4], sig, geom.dsig, ptop, pc.MOIST_DT,
                                                moist_ref.params(**pc.MOIST_PAR), dtype)
            assert (E > 0).any() and (P > 0).any()
