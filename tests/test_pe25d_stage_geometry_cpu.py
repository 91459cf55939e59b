"""What tests/test_pe25d_stage_geometry_gpu.py reaches, stated on the CPU (tests/pe25d_stage_geometry_cases.py): every
case takes the launch geometry of the dynamics stage it is named for -- from gcm_pe25d_stage_geometry, the helper that
launch_k1, update_rows, pe25d_create and the looping K1's picker take their numbers from, at 256 compute units -- the
product grids take what the cases stand in for, the list reaches every looping instantiation and every K4 remainder it
claims, and no grid of half the rows would do."""
import ctypes as C

import numpy as np
import pytest

import pe25d_stage_geometry_cases as sc
from gcmiipy_amd import _lib
from gcmiipy_amd.core import stage_geometry
from test_pe25d_variants_cpu import FILTER_WIDTHS, loop_kernel

ESZ = {"f64": 8, "f32": 4}


def _geometry(shape, dtype, cus=sc.CUS):
    H, W, L = shape
    return stage_geometry(W, H, L, cus, ESZ[dtype])


def _loop(d):
    return (d["k1_maxr"], d["k1_mask"], d["k1_nin"], d["k1_nw"])


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_case_takes_its_plan(case, dtype):
    assert _geometry(case.shape, dtype) == sc.plan(case, dtype), case.what


def test_product_grids():
    c4 = _geometry((720, 1440, 24), "f64")
    assert (c4["k1_workgroups_per_row"], c4["k1_pairs_per_wg"], c4["k1_pairs_last_wg"]) == (2, 6, 6)
    assert _loop(c4) == (12, 1440, 10, 3) and c4["k1_passes"] == 3 and c4["k1_pit_rides"] == 1
    assert (c4["k4_rows"], c4["k4_groups"], c4["k4_rows_last_group"], c4["k4_col_tiles"], c4["k4_oddtop"]) == (7, 103, 6, 24, 1)
    c5 = _geometry((1440, 2880, 40), "f64")
    assert (c5["k1_workgroups_per_row"], c5["k1_pairs_per_wg"], c5["k4_rows"]) == (1, 20, 7)
    assert _loop(c5) == (16, 2880, 15, 3)
    band = _geometry((90, 1440, 24), "f64")
    assert (band["k1_workgroups_per_row"], band["k1_pairs_per_wg"], band["k4_rows"]) == (6, 2, 3)
    for shape in ((720, 1440, 24), (1440, 2880, 40), (90, 1440, 24)):
        d32, d64 = _geometry(shape, "f32"), _geometry(shape, "f64")
        assert d32["k4_rows"] == 3
        assert {k: v for k, v in d32.items() if k.startswith("k1_")} == {k: v for k, v in d64.items() if k.startswith("k1_")}


def test_suite_shapes_loop_once():
    """the shapes the rest of the suite steps: one pair per workgroup, 3-row K4 -- what this case list is there to leave"""
    for shape in ((4, 1440, 3), (5, 30, 24), (5, 30, 25), (12, 20, 5), (48, 1440, 24), (8, 1458, 24), (8, 1440, 24), (9, 30, 24)):
        d = _geometry(shape, "f64")
        assert d["k1_pairs_per_wg"] == 1 and d["k4_rows"] == 3, shape


def test_case_list_reaches_everything():
    plans = {(c.shape, t): sc.plan(c, t) for c in sc.CASES for t in sc.DTYPES}
    # every looping instantiation a width reaches (test_pe25d_variants_cpu.py), at two pairs or more, in both real types
    names = {None: 0, "1440": 1440, "2880": 2880, "4096": 4096}
    reachable = {(k[0], names[k[1]], k[2], k[3]) for k in (loop_kernel(n) for n in FILTER_WIDTHS) if k is not None}
    assert len(reachable) == 6
    for t in sc.DTYPES:
        assert {_loop(p) for (_, tt), p in plans.items() if tt == t and p["k1_pairs_per_wg"] >= 2} == reachable, t
    assert {p["k1_passes"] for p in plans.values()} == {2, 3, 4}
    # an odd L whose single-level pair follows another pair in its workgroup; a workgroup with fewer pairs than ppw
    assert any(c.shape[2] % 2 == 1 and sc.plan(c, "f64")["k1_pairs_last_wg"] >= 2 for c in sc.CASES)
    assert any(0 < p["k1_pairs_last_wg"] < p["k1_pairs_per_wg"] for p in plans.values())
    # ... of which one holds a single, single-level pair alone
    assert any(c.shape[2] % 2 == 1 and sc.plan(c, "f64")["k1_pairs_last_wg"] == 1 for c in sc.CASES)
    r7 = [p for (_, t), p in plans.items() if t == "f64" and p["k4_rows"] == 7]
    assert {p["k4_rows_last_group"] for p in r7} >= {1, 2, 5, 7}
    assert {p["k4_rows_last_group"] for p in r7 if p["k4_col_tiles"] >= 2} >= {1, 5, 7}
    assert any(p["k4_oddtop"] for p in r7) and any(not p["k4_oddtop"] for p in r7)
    assert all(p["k4_rows"] == 3 for (_, t), p in plans.items() if t == "f32")
    # both sides of the 400 / 401 rule
    assert plans[((400, 360, 7), "f64")]["k4_rows"] == 3 and plans[((401, 30, 5), "f64")]["k4_rows"] == 7
    assert _geometry((400, 30, 5), "f64")["k4_rows"] == 3 and _geometry((401, 360, 7), "f64")["k4_rows"] == 7
    # the three setups beside the default, each on a 7-row case
    setups = [c.setup for c in sc.CASES if c.setup]
    assert sorted(k for s in setups for k in s) == ["bump", "coriolis", "ptop"]
    assert all(sc.plan(c, "f64")["k4_rows"] == 7 for c in sc.CASES if c.setup)


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_no_smaller_grid_would_do(case):
    H, W, L = case.shape
    d = _geometry((H // 2, W, L), "f64")
    assert d["k1_pairs_per_wg"] == 1 or d["k4_rows"] == 3, d


def test_regions_of_the_locality_check():
    """the masks of pe25d_stage_geometry_cases.regions: the levels of each workgroup's last pair, the last group's rows,
    the last tile's columns; a region a case does not have is left out"""
    case = sc.case_of((512, 120, 13))
    r = sc.regions(case.shape, sc.plan(case, "f64"))
    assert sorted(r) == ["k1_last_pair", "k4_last_group", "k4_last_tile"]
    assert np.flatnonzero(r["k1_last_pair"][:, 0, 0]).tolist() == [6, 7, 12]          # pairs 3 and 6 (a single level)
    assert np.flatnonzero(r["k4_last_group"][0, :, 0]).tolist() == [511]
    assert np.flatnonzero(r["k4_last_tile"][0, 0, :]).tolist() == list(range(62, 120))
    r32 = sc.regions(case.shape, sc.plan(case, "f32"))
    assert np.flatnonzero(r32["k4_last_group"][0, :, 0]).tolist() == [510, 511]
    case = sc.case_of((420, 30, 12))
    assert sorted(sc.regions(case.shape, sc.plan(case, "f64"))) == ["k1_last_pair"]
    assert np.flatnonzero(sc.last_pair_levels(5, dict(k1_pairs_per_wg=2))).tolist() == [2, 3, 4]
    for c in sc.CASES:
        assert "k1_last_pair" in sc.regions(c.shape, sc.plan(c, "f64")), c.shape


def test_bands_take_their_launches():
    """the loopback band of 420 x 30 x 12 and the two bands of 840 x 30 x 5: the own rows' K1 and K4 of the interior
    rows by the pure function (the edge launch and nseg_edge: the handle's, asserted on the device)"""
    H, W, L = sc.BAND_CASE
    own = _geometry((H, W, L), "f64")
    assert (own["k1_workgroups_per_row"], own["k1_pairs_per_wg"], own["k4_rows"]) == (2, 3, 7)
    assert _geometry((H + 1, W, L), "f64")["k1_pairs_per_wg"] == 3                   # with the south ghost row
    H, W, L = sc.TWO_BANDS
    from gcmiipy_amd.bands import split_rows
    assert split_rows(H, 2) == [(0, 421), (421, 421)]
    d = _geometry((421, W, L), "f64")
    assert (d["k4_rows"], d["k4_groups"], d["k4_rows_last_group"]) == (7, 61, 1)     # the pole row alone in the last group
    assert _geometry((420, W, L), "f64")["k4_rows_last_group"] == 7                 # (840 rows: 60 whole groups a band)
    assert _geometry((422, W, L), "f64")["k1_pairs_per_wg"] == 2                    # with the south ghost row


def test_query_follows_its_arguments():
    """the launchers' formulas written out once more, over a sweep of sizes and chips"""
    for W, rows, L, cus in ((30, 5, 24, 256), (1440, 720, 24, 256), (1440, 720, 24, 304), (360, 400, 7, 64), (2880, 1440, 40, 256),
                            (120, 1000, 41, 8), (36, 401, 2, 256), (30, 90, 1, 256)):
        for esz in (8, 4):
            d = stage_geometry(W, rows, L, cus, esz)
            pairs = -(-L // 2)
            groups = min(pairs, max(1, -(-3 * cus // rows)))
            ppw = -(-pairs // groups)
            ny = -(-pairs // ppw)
            assert (d["k1_workgroups_per_row"], d["k1_pairs_per_wg"], d["k1_pairs_last_wg"]) == (ny, ppw, pairs - (ny - 1) * ppw)
            R = 3 if rows <= 400 or esz == 4 else 7
            ng, tiles = -(-rows // R), -(-W // 62)
            assert (d["k4_rows"], d["k4_groups"], d["k4_rows_last_group"]) == (R, ng, rows - (ng - 1) * R)
            assert (d["k4_col_tiles"], d["k4_cols_last_tile"]) == (tiles, W - 62 * (tiles - 1))
            assert d["k4_grid"] == sc.k4_grid(ng, tiles) and d["k4_nseg"] == 1 and d["k4_oddtop"] == (L % 2 == 0)


def test_query_takes_plan_words_and_refuses_what_it_cannot_answer():
    out = (C.c_int * _lib.STAGE_PLAN_WORDS)()
    f = _lib.lib.gcm_pe25d_stage_geometry
    words = (C.c_uint * 64)()
    assert _lib.lib.gcm_filter_plan(1440, words, 64) == 0
    assert stage_geometry(1440, 720, 24, 256, 8, plan=list(words)) == stage_geometry(1440, 720, 24, 256, 8)
    # another row's plan words: the instantiation follows the words, not W
    assert _lib.lib.gcm_filter_plan(4096, words, 64) == 0
    assert _loop(stage_geometry(1440, 720, 24, 256, 8, plan=list(words))) == (16, 4096, 16, 5)
    # a width without a composite plan, and a single-pass plan: no looping form, one workgroup per level pair
    for W in (14, 20):
        d = stage_geometry(W, 768, 5, 256)
        assert (d["k1_loop"], d["k1_workgroups_per_row"], d["k1_pairs_per_wg"], d["k1_pit_rides"]) == (0, 3, 1, 0)
        assert _loop(d) == (0, 0, 0, 0)
    assert f(30, 768, 5, 256, 8, None, 0, out, _lib.STAGE_PLAN_WORDS) == _lib.OK
    for args in ((0, 768, 5, 256, 8), (30, 0, 5, 256, 8), (30, 768, 0, 256, 8), (30, 768, 5, 0, 8), (30, 768, 5, 256, 2)):
        assert f(*args, None, 0, out, _lib.STAGE_PLAN_WORDS) == _lib.ERR_ARG, args
    assert f(30, 768, 5, 256, 8, None, 0, out, _lib.STAGE_PLAN_WORDS - 1) == _lib.ERR_ARG
    assert f(30, 768, 5, 256, 8, None, 0, None, _lib.STAGE_PLAN_WORDS) == _lib.ERR_ARG
    assert f(30, 768, 5, 256, 8, words, 8, out, _lib.STAGE_PLAN_WORDS) == _lib.ERR_ARG      # too few plan words
    assert _lib.lib.gcm_pe25d_stage_plan(None, out, _lib.STAGE_PLAN_WORDS) == _lib.ERR_ARG
    assert len(_lib.STAGE_WORDS) == _lib.STAGE_PLAN_WORDS and _lib.STAGE_WORDS[_lib.STAGE_BAND_WORD] == "band"
