"""The wide form of the single-query bound scan (65 <= k <= 1024; quiver_amd/csrc/qv_bound_scan.hip) without a GPU: the dispatch's own rule
(qv_scan_bound_wide_route) over a grid, that the k <= 64 rule still says no at k = 65, and the layout of the wide form's workspace
(qv_scan_workspace_layout, kind QV_WS_BOUND_WIDE).  No device is touched."""
import ctypes as C
import itertools
import os

import pytest

from quiver_amd import _lib

COSINE, L2, L2SQ, DOT, L1 = 0, 1, 2, 3, 4
L2P = _lib.QV_RULE_L2_PLANES
AUTO, ALWAYS, NEVER = 0, 1, 2
P_AUTO, P_8BIT, P_BF16 = 0, 1, 2
METRICS3 = (COSINE, DOT, L2P)


def route(metric, dim, rows, nq, k, wide, plane, has_plane=1, has_plane8=1):
    return _lib.lib().qv_scan_bound_wide_route(metric, dim, rows, nq, k, wide, plane, has_plane, has_plane8)


GRID = list(itertools.product(METRICS3 + (L2, L2SQ, L1, 5, 6, 7, 8), (16, 80, 768, 4096, 24, 4112, 1), (511, 512, 6001, 1_000_000, 10_000_000),
                              (1, 2, 8), (1, 64, 65, 100, 128, 129, 1000, 1024, 1025), (AUTO, ALWAYS, NEVER), (P_AUTO, P_8BIT, P_BF16), (0, 1), (0, 1)))


def test_where_the_rule_says_no():
    for metric, dim, rows, nq, k, wide, plane, hp, hp8 in GRID:
        got = route(metric, dim, rows, nq, k, wide, plane, hp, hp8)
        assert got in (0, 1, 2), (metric, dim, rows, nq, k, wide, plane, hp, hp8, got)
        no = (k <= 64 or k > 1024 or nq != 1 or metric not in METRICS3 or dim % 16 != 0 or dim > 4096 or (rows + 63) // 64 < 8 or not hp or wide == NEVER)
        if no:
            assert got == 0, (metric, dim, rows, nq, k, wide, plane, hp, hp8)
        if got == 2:
            assert hp8 and plane != P_BF16, (metric, dim, rows, nq, k, wide, plane, hp, hp8)


def test_automatic_never_goes_where_always_does_not():
    for metric, dim, rows, nq, k, _, plane, hp, hp8 in GRID:
        if route(metric, dim, rows, nq, k, ALWAYS, plane, hp, hp8) == 0:
            assert route(metric, dim, rows, nq, k, AUTO, plane, hp, hp8) == 0, (metric, dim, rows, nq, k, plane, hp, hp8)


@pytest.mark.parametrize("metric", METRICS3)
def test_always_with_the_8bit_plane_first(metric):
    for k in (65, 128, 129, 1024):
        for dim, rows in ((16, 2000), (80, 6001), (768, 1_000_000), (4096, 10_000_000)):
            assert route(metric, dim, rows, 1, k, ALWAYS, P_8BIT) == 2, (k, dim, rows)
            assert route(metric, dim, rows, 1, k, ALWAYS, P_8BIT, 1, 0) == 1, (k, dim, rows)       # the plane is not held: the bfloat16 copy first
            assert route(metric, dim, rows, 1, k, ALWAYS, P_BF16) == 1, (k, dim, rows)
            assert route(metric, dim, rows, 1, k, ALWAYS, P_AUTO) in (1, 2), (k, dim, rows)
            assert route(metric, dim, rows, 1, k, ALWAYS, P_8BIT, 0, 1) == 0, (k, dim, rows)       # never without the bfloat16 copy behind it


def test_fewer_rows_than_results_and_the_redo_room():
    assert route(COSINE, 64, 1024, 1, 1024, ALWAYS, P_BF16) == 0        # k takes every row: nothing to reject
    assert route(COSINE, 64, 1025, 1, 1024, ALWAYS, P_BF16) == 1
    assert route(COSINE, 64, 64_000_000, 1, 100, ALWAYS, P_BF16) == 1   # two key planes of the redo fit a gibibyte ...
    assert route(COSINE, 64, 70_000_000, 1, 100, ALWAYS, P_BF16) == 0   # ... and no longer


def test_automatic_takes_the_measured_cells_and_no_other():
    """profiles/LAB_r24_bound_scan_wide.md: 1M, 3M, 10M x 768 and 10M x 128, cosine, k = 65 .. 1000 — every cell won, 8-bit first too"""
    for metric in (COSINE, DOT):
        for k in (65, 100, 128, 129, 256, 1000):
            for dim, rows in ((768, 1_000_000), (768, 3_000_000), (768, 10_000_000), (1536, 1_000_000), (128, 10_000_000), (512, 10_000_000)):
                assert route(metric, dim, rows, 1, k, AUTO, P_AUTO) == 2, (metric, k, dim, rows)
                assert route(metric, dim, rows, 1, k, AUTO, P_AUTO, 1, 0) == 1, (metric, k, dim, rows)
                assert route(metric, dim, rows, 1, k, AUTO, P_BF16) == 1, (metric, k, dim, rows)
            for dim, rows in ((768, 999_999), (128, 9_999_999), (128, 1_000_000), (112, 10_000_000), (16, 50_000_000), (80, 6001)):   # not measured
                assert route(metric, dim, rows, 1, k, AUTO, P_AUTO) == 0, (metric, k, dim, rows)
                assert route(metric, dim, rows, 1, k, AUTO, P_8BIT) == 0, (metric, k, dim, rows)
                assert route(metric, dim, rows, 1, k, ALWAYS, P_AUTO) == 1, (metric, k, dim, rows)   # forced on: the bfloat16 copy first where 8-bit first was not measured
        for k in (1001, 1024):                                          # above the largest measured k
            assert route(metric, 768, 10_000_000, 1, k, AUTO, P_AUTO) == 0
            assert route(metric, 768, 10_000_000, 1, k, ALWAYS, P_AUTO) == 1
    assert route(L2P, 768, 10_000_000, 1, 100, AUTO, P_AUTO) == 0       # Euclidean indexes with the planes: not measured
    assert route(L2P, 768, 10_000_000, 1, 100, ALWAYS, P_8BIT) == 2


def test_unknown_modes_are_errors():
    for wide, plane in ((3, 0), (-1, 0), (0, 3), (0, -1), (99, 99)):
        assert route(COSINE, 768, 1_000_000, 1, 100, wide, plane) < 0, (wide, plane)


def test_the_k64_rule_is_what_it_was():
    lib = _lib.lib()
    for metric in METRICS3:
        for rows in (6001, 1_000_000, 10_000_000):
            assert lib.qv_scan_bound_applies(metric, 768, rows, 1, 65, ALWAYS, 1) == 0
            assert lib.qv_scan_bound_applies(metric, 768, rows, 1, 64, ALWAYS, 1) == 1
            assert lib.qv_scan_bound8_applies(metric, 768, rows, 1, 65, ALWAYS, P_8BIT, 1) == 0


REGION_CAP = 16


def layout(dim, rows, k, cus=256, metric=COSINE):
    total, end, n = C.c_uint64(), C.c_uint64(), C.c_uint32()
    regs = (C.c_uint64 * (4 * REGION_CAP))()
    rc = _lib.lib().qv_scan_workspace_layout(_lib.QV_WS_BOUND_WIDE, metric, dim, rows, 1, k, cus, 0, C.byref(total), C.byref(end), C.byref(n), regs, REGION_CAP)
    assert rc == 0 and 0 < n.value <= REGION_CAP, (rc, n.value, _lib.lib().qv_last_error())
    flat = regs[:4 * n.value]
    return total.value, end.value, [tuple(flat[i:i + 4]) for i in range(0, len(flat), 4)]


ROWS = (512, 2000, 6001, 200_000, 1_000_000, 10_000_000)
KS = (65, 100, 128, 129, 500, 1024)


@pytest.mark.parametrize("dim", [16, 80, 768, 4096])
@pytest.mark.parametrize("cus", [1, 256])
def test_workspace_regions_lie_apart_and_inside(dim, cus):
    for rows in ROWS:
        for k in KS:
            total, end, regs = layout(dim, rows, k, cus)
            assert 0 < end <= total, (rows, k, end, total)
            plain = [r for r in regs if not r[3]]
            alias = [r for r in regs if r[3]]
            assert len(alias) == 1 and len(plain) == 8, regs            # the redo's workspace overlays the rest; the eight regions of the bound stages
            at = 0
            for off, size, align, _ in plain:                          # in order, apart, aligned, none empty
                assert size > 0 and off >= at and off % align == 0, (rows, k, regs)
                at = off + size
            assert at <= end
            for off, size, align, _ in alias:
                assert size > 0 and off % align == 0 and off + size <= end, (rows, k, regs)
            # the list holds the capacity, as rows and as keys; a lower-bound word per row slot
            sizes = [r[1] for r in plain]
            assert _lib.QV_BOUND_WIDE_CAND_CAP * 4 in sizes and _lib.QV_BOUND_WIDE_CAND_CAP * 8 in sizes and (rows + 63) // 64 * 256 in sizes, (rows, k, sizes)


def test_workspace_total_is_monotone_in_rows_and_k():
    for dim in (16, 768):
        for k in KS:
            totals = [layout(dim, rows, k)[0] for rows in ROWS]
            assert totals == sorted(totals), (dim, k, totals)
        for rows in ROWS:
            totals = [layout(dim, rows, k)[0] for k in KS]
            assert totals == sorted(totals), (dim, rows, totals)


def test_the_capacity_keeps_the_k64_forms_spare():
    assert _lib.QV_BOUND_WIDE_CAND_CAP >= 1024 + 4032
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qv.h")) as f:
        assert "#define QV_BOUND_WIDE_CAND_CAP %d " % _lib.QV_BOUND_WIDE_CAND_CAP in f.read()   # the Python constant is the header's
