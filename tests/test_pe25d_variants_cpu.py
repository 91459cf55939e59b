"""Which compiled instantiation of the GCM_PE25D filter kernels each row width reaches, pinned on the host.

The handle picks its K1 / K3 / pit kernels from the composite plan of the row (make_super_plan, csrc/fft_lds.h)
by the rules of spu_filter_kernel_for / spu_filter_loop_kernel_for (pe25d_k1.h) and pgf_filter_kernel_for /
pit2d_kernel_for (pe25d_k3.h).  The non-looping kernels' rules are restated here and applied to the library's own plans
(gcm_filter_plan); the looping K1's instantiation is the library's own answer (gcm_pe25d_stage_geometry), so that the
case list of test_pe25d_variants_gpu.py cannot drift away from the paths it claims to reach."""
import ctypes as C

import pytest


def _plan(n):
    from gcmiipy_amd import _lib
    out = (C.c_uint * 64)()
    assert _lib.lib.gcm_filter_plan(n, out, 64) == 0
    ok, npass = out[0], out[1]
    return ok, npass, [(out[3 + 4 * p], out[4 + 4 * p]) for p in range(npass)]


_PASS_BITS = [(2, None), (3, 1), (4, 1), (5, 1), (3, 2), (4, 2), (3, 3), (5, 2), (4, 3), (5, 3), (4, 4), (5, 4)]


def pass_bit(a, b):
    """fft_lds.h pass_bit: a pass of radix a.b -> its bit (5.5 takes the last one)"""
    for n, (x, y) in enumerate(_PASS_BITS):
        if a == x and (y is None or b == y):
            return 1 << n
    return 1 << 12


MASK1440 = pass_bit(5, 2) | pass_bit(4, 3)
MASK2880 = pass_bit(5, 3) | pass_bit(4, 3) | pass_bit(4, 4)
MASK4096 = pass_bit(4, 4)
_MASK_NAME = {MASK1440: "1440", MASK2880: "2880", MASK4096: "4096"}


def _mask_maxr(passes):
    mask, maxr = 0, 0
    for a, b in passes:
        mask |= pass_bit(a, b)
        maxr = max(maxr, a * b)
    return mask, maxr


def filter_kernel(n):
    """spu_filter_kernel_for = pgf_filter_kernel_for = pit2d_kernel_for -> (MAXR, mask name or None);
    MAXR 0 is the generic ping-pong path"""
    ok, _, passes = _plan(n)
    if not ok:
        return (0, None)
    mask, maxr = _mask_maxr(passes)
    if mask in _MASK_NAME:
        return (16 if mask != MASK1440 else 12, _MASK_NAME[mask])
    return (12 if maxr <= 12 else 16 if maxr <= 16 else 25, None)


def loop_kernel(n):
    """spu_filter_loop_kernel_for -> (MAXR, mask name or None, NIN, NW), or None (no looping form: K1 one
    workgroup per level pair, pit as pe_pit2d_kernel).  The rule is stated once, in spu_filter_loop_desc
    (csrc/pe25d_stage_geometry.h), which the picker itself reads: this is the library's answer (gcm_pe25d_stage_geometry),
    held to the literal PINS below"""
    from gcmiipy_amd.core import stage_geometry
    d = stage_geometry(n, 1, 1, 1)
    if not d["k1_loop"]:
        assert (d["k1_maxr"], d["k1_mask"], d["k1_nin"], d["k1_nw"]) == (0, 0, 0, 0)
        return None
    return (d["k1_maxr"], {0: None, 1440: "1440", 2880: "2880", 4096: "4096"}[d["k1_mask"]], d["k1_nin"], d["k1_nw"])


# width -> (ok, passes as "r1.r2", filter kernel, looping K1); the widths of test_pe25d_variants_gpu.py
PINS = {
    10: (1, ["5.2"], (12, None), None),
    12: (1, ["4.3"], (12, None), None),
    14: (0, [], (0, None), None),                                   # 2.7: the generic path
    16: (1, ["4.4"], (16, "4096"), None),
    20: (1, ["5.4"], (25, None), None),
    22: (0, [], (0, None), None),                                   # 2.11
    30: (1, ["5.2", "3.1"], (12, None), (12, None, 12, 5)),
    36: (1, ["4.3", "3.1"], (12, None), (12, None, 12, 5)),
    100: (1, ["5.4", "5.1"], (25, None), (25, None, 25, 5)),
    120: (1, ["5.2", "4.3"], (12, "1440"), (12, "1440", 10, 3)),    # kMask1440 in two passes: NIN = 10 at np = 2
    202: (0, [], (0, None), None),                                  # 2.101: the generic radix-r butterfly
    256: (1, ["4.4", "4.4"], (16, "4096"), (16, "4096", 16, 5)),    # kMask4096 in two passes
    360: (1, ["5.2", "4.3", "3.1"], (12, None), (12, None, 12, 5)),
    400: (1, ["5.4", "5.4"], (25, None), (25, None, 25, 5)),
    720: (1, ["5.3", "4.3", "4.1"], (16, None), (16, None, 16, 5)),
    1250: (1, ["5.2", "5.5", "5.1"], (25, None), (25, None, 25, 5)),
    1440: (1, ["5.2", "4.3", "4.3"], (12, "1440"), (12, "1440", 10, 3)),
    1458: (1, ["3.2", "3.3", "3.3", "3.1"], (12, None), (12, None, 12, 5)),   # the only four-pass plan
    1536: (1, ["4.2", "4.3", "4.4"], (16, None), (16, None, 16, 5)),
    2250: (1, ["5.2", "5.3", "5.3"], (16, None), (16, None, 16, 5)),
    2880: (1, ["5.3", "4.3", "4.4"], (16, "2880"), (16, "2880", 15, 3)),
    4096: (1, ["4.4", "4.4", "4.4"], (16, "4096"), (16, "4096", 16, 5)),
    4608: (0, ["4.2", "4.3", "4.3", "4.1"], (0, None), None),       # {2,3}-smooth, but a pass of 1152 butterflies
    4800: (1, ["5.3", "5.4", "4.4"], (25, None), (25, None, 25, 5)),
}
FILTER_WIDTHS = sorted(PINS)


@pytest.mark.parametrize("n", FILTER_WIDTHS)
def test_plan_and_instantiation_pins(n):
    ok, npass, passes = _plan(n)
    want_ok, want_passes, want_k, want_loop = PINS[n]
    assert ok == want_ok, n
    assert ["%d.%d" % p for p in passes] == want_passes, n
    assert npass == len(want_passes)
    assert filter_kernel(n) == want_k, (n, filter_kernel(n))
    assert loop_kernel(n) == want_loop, (n, loop_kernel(n))


def test_every_filter_instantiation_is_in_the_gpu_case_list():
    """the non-looping K1 / K3 / pit kernels: generic, the three masked forms and MAXR = 12 / 16 / 25; the looping
    K1: every instantiation that any width reaches (see the next test for the two that none does)"""
    assert {filter_kernel(n) for n in FILTER_WIDTHS} == {(0, None), (12, "1440"), (16, "2880"), (16, "4096"),
                                                        (12, None), (16, None), (25, None)}
    assert {loop_kernel(n) for n in FILTER_WIDTHS} - {None} == {(12, "1440", 10, 3), (16, "2880", 15, 3),
                                                                (16, "4096", 16, 5), (12, None, 12, 5),
                                                                (16, None, 16, 5), (25, None, 25, 5)}
    # the four-pass plan (filter_rows_hoisted's np > 3 branches, NW = 5) and single-pass plans (no looping form)
    assert any(len(PINS[n][1]) == 4 and PINS[n][0] for n in FILTER_WIDTHS)
    assert any(len(PINS[n][1]) == 1 for n in FILTER_WIDTHS)


def _composite_widths():
    # a composite plan has a pass of at most 25 and at most 512 butterflies per pass: none above 512 * 25
    return [n for n in range(2, 512 * 25 + 1, 2) if _plan(n)[0]]


def test_only_1458_has_a_four_pass_plan():
    widths = _composite_widths()
    assert max(widths) == 10000
    assert [n for n in widths if _plan(n)[1] == 4] == [1458]
    assert max(_plan(n)[1] for n in widths) == 4


def test_general_masked_looping_forms_are_unreachable():
    """spu_filter_loop_kernel_for also names pe_spu_filter_loop_kernel<T, 12, kMask1440> and <T, 16, kMask2880> (NIN =
    MAXR, NW = 5): a plan with exactly the passes of kMask1440 starts with 5.2 and has at most three passes, one of
    kMask2880 starts with 5.3 and has at most three -- no width reaches them"""
    for n in _composite_widths():
        lk = loop_kernel(n)
        assert lk not in ((12, "1440", 12, 5), (16, "2880", 16, 5)), n
