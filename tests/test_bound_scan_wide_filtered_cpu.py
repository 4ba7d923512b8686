"""The wide form of the bound scan for ONE filtered query (65 <= k <= 1024 over a candidate bitmap; quiver_amd/csrc/qv_bound_scan.hip)
without a GPU: the dispatch's own rule (qv_scan_bound_wide_route_filtered) over the unfiltered rule's grid with the candidate tiles and the
live candidates added, and that the unfiltered rule is what it was.  No device is touched."""
import itertools

import pytest

from quiver_amd import _lib

COSINE, L2, L2SQ, DOT, L1 = 0, 1, 2, 3, 4
L2P = _lib.QV_RULE_L2_PLANES
AUTO, ALWAYS, NEVER = 0, 1, 2
P_AUTO, P_8BIT, P_BF16 = 0, 1, 2
METRICS3 = (COSINE, DOT, L2P)


def route(metric, dim, rows, nq, k, wide, plane, has_plane=1, has_plane8=1):
    return _lib.lib().qv_scan_bound_wide_route(metric, dim, rows, nq, k, wide, plane, has_plane, has_plane8)


def froute(metric, dim, rows, nq, k, wide, plane, has_plane=1, has_plane8=1, tiles=None, cands=None):
    """tiles / cands None: every tile holds a candidate, every row is one"""
    tiles = (rows + 63) // 64 if tiles is None else tiles
    cands = rows if cands is None else cands
    return _lib.lib().qv_scan_bound_wide_route_filtered(metric, dim, rows, nq, k, wide, plane, has_plane, has_plane8, tiles, cands)


# (the unfiltered rule's grid, thinned where the two rules do not differ, times what a filter adds)
GRID = list(itertools.product(METRICS3 + (L2, L1, 8), (16, 80, 768, 4096, 24, 4112), (511, 512, 6001, 1_000_000, 10_000_000),
                              (1, 2), (1, 64, 65, 100, 129, 1000, 1024, 1025), (AUTO, ALWAYS, NEVER), (P_AUTO, P_8BIT, P_BF16), (0, 1), (0, 1)))
# (candidate tiles, candidates) as functions of (rows, k): every row; no tile; one tile in ten with plenty of rows; k, k + 1, k - 1 candidates
FILTERS = {
    "all": lambda rows, k: ((rows + 63) // 64, rows),
    "no_tile": lambda rows, k: (0, rows),
    "tenth": lambda rows, k: (max(1, (rows + 63) // 640), max(1, rows // 10)),
    "k": lambda rows, k: ((rows + 63) // 64, k),
    "k+1": lambda rows, k: ((rows + 63) // 64, k + 1),
    "k-1": lambda rows, k: ((rows + 63) // 64, k - 1),
    "none": lambda rows, k: ((rows + 63) // 64, 0),
}


def test_where_the_rule_says_no():
    for metric, dim, rows, nq, k, wide, plane, hp, hp8 in GRID:
        for name, f in FILTERS.items():
            tiles, cands = f(rows, k)
            got = froute(metric, dim, rows, nq, k, wide, plane, hp, hp8, tiles, cands)
            where = (metric, dim, rows, nq, k, wide, plane, hp, hp8, name, got)
            assert got in (0, 1, 2), where
            no = (wide == NEVER or nq != 1 or k <= 64 or k > 1024 or metric not in METRICS3 or dim % 16 != 0 or dim > 4096 or (rows + 63) // 64 < 8 or not hp
                  or tiles == 0 or cands <= k)
            if no:
                assert got == 0, where
            elif wide == ALWAYS and k < rows:
                if plane == P_AUTO and hp8:                              # (the automatic plane: 8-bit first in its measured cells only)
                    assert got in (1, 2) and (got == 1 or rows >= 1_000_000), where
                else:
                    assert got == (2 if plane == P_8BIT and hp8 else 1), where
            if got == 2:
                assert hp8 and plane != P_BF16, where


def test_the_redo_needs_its_room():
    assert froute(COSINE, 64, 64_000_000, 1, 100, ALWAYS, P_BF16) == 1   # two key planes of the redo fit a gibibyte ...
    assert froute(COSINE, 64, 70_000_000, 1, 100, ALWAYS, P_BF16) == 0   # ... and no longer


@pytest.mark.parametrize("metric", METRICS3)
def test_more_candidates_than_results(metric):
    """candidates = k: a k that takes every candidate has nothing to reject; candidates = k + 1: taken under "always"; fewer: the call keeps
    its path and its clamped count"""
    for dim, rows in ((16, 2000), (80, 6001), (768, 1_000_000)):
        for k in (65, 100, 128, 129, 1024):
            for plane, want in ((P_BF16, 1), (P_8BIT, 2), (P_AUTO, 2 if rows >= 1_000_000 and k <= 1000 and metric != L2P else 1)):   # (automatic plane: 8-bit first where measured)
                assert froute(metric, dim, rows, 1, k, ALWAYS, plane, cands=k + 1) == want, (dim, rows, k, plane)
                assert froute(metric, dim, rows, 1, k, ALWAYS, plane, cands=k) == 0, (dim, rows, k, plane)
                assert froute(metric, dim, rows, 1, k, ALWAYS, plane, cands=k - 1) == 0, (dim, rows, k, plane)
                assert froute(metric, dim, rows, 1, k, ALWAYS, plane, tiles=0, cands=rows) == 0, (dim, rows, k, plane)
                assert froute(metric, dim, rows, 1, k, ALWAYS, plane, tiles=1, cands=k + 1) == (want if plane != P_AUTO else 1), (dim, rows, k, plane)
            assert froute(metric, dim, rows, 1, k, ALWAYS, P_8BIT, 1, 0, cands=k + 1) == 1    # the plane is not held: the bfloat16 copy first
            assert froute(metric, dim, rows, 1, k, ALWAYS, P_8BIT, 0, 1, cands=k + 1) == 0    # never without the bfloat16 copy behind it
    assert froute(metric, 768, 1_000_000, 1, 100, ALWAYS, P_BF16, tiles=0xFFFFFFFF, cands=2 ** 40) == 1   # counts past the index: read as "every"


def test_automatic_never_goes_where_always_does_not():
    for metric, dim, rows, nq, k, _, plane, hp, hp8 in GRID:
        for name, f in FILTERS.items():
            tiles, cands = f(rows, k)
            if froute(metric, dim, rows, nq, k, ALWAYS, plane, hp, hp8, tiles, cands) == 0:
                assert froute(metric, dim, rows, nq, k, AUTO, plane, hp, hp8, tiles, cands) == 0, (metric, dim, rows, nq, k, plane, hp, hp8, name)


def test_automatic_never_goes_where_the_unfiltered_rule_declines():
    """the filter's conditions sit on top of the unfiltered floor: same metric, dim, rows and k"""
    for metric, dim, rows, nq, k, _, plane, hp, hp8 in GRID:
        if route(metric, dim, rows, nq, k, AUTO, P_AUTO, hp, hp8) == 0:
            for name, f in FILTERS.items():
                tiles, cands = f(rows, k)
                assert froute(metric, dim, rows, nq, k, AUTO, plane, hp, hp8, tiles, cands) == 0, (metric, dim, rows, nq, k, plane, hp, hp8, name)


def tiles_of(rows, per_mille):
    """the fewest candidate tiles that make `per_mille` of the tiles"""
    n = (rows + 63) // 64
    return -(-n * per_mille // 1000)


def test_automatic_takes_the_measured_cells_and_no_other():
    """profiles/LAB_r25_bound_scan_wide_filtered.md: 1M, 3M, 10M x 768 and 10M x 128, cosine, k = 65 .. 1000, candidate-tile fractions 1
    (every row, a random half), 0.476 (a random 1 %) and 0.100 (one tile in ten).  The bfloat16 copy first won every cell; the 8-bit plane
    first lost 1M x 768 at 0.100 and did not clear the spread at 0.476, and lost 10M x 128 at 0.100.  The constants of qv_bound_scan.hip
    (kBoundWideFilterFloor, kBoundWide8FilterFloor), pinned."""
    big = 10 ** 9                                                        # candidates: plenty
    for metric in (COSINE, DOT):
        for k in (65, 100, 128, 129, 256, 1000):
            # (dim, rows, the sparsest fraction the form takes, the sparsest at which it starts on the 8-bit plane), per mille of the tiles
            for dim, rows, f_form, f_8bit in ((768, 1_000_000, 100, 1000), (768, 2_999_999, 100, 1000), (1536, 1_000_000, 100, 1000), (768, 3_000_000, 100, 100),
                                              (768, 10_000_000, 100, 100), (4096, 10_000_000, 100, 100), (128, 10_000_000, 100, 475), (512, 10_000_000, 100, 475)):
                n = (rows + 63) // 64
                for tiles in (n, tiles_of(rows, 476), tiles_of(rows, 475), tiles_of(rows, 475) - 1, tiles_of(rows, 100), tiles_of(rows, 100) - 1, 1):
                    want = 0 if tiles * 1000 < n * f_form else 2 if tiles * 1000 >= n * f_8bit else 1
                    where = (metric, k, dim, rows, tiles)
                    assert froute(metric, dim, rows, 1, k, AUTO, P_AUTO, tiles=tiles, cands=big) == want, where
                    assert froute(metric, dim, rows, 1, k, AUTO, P_AUTO, 1, 0, tiles=tiles, cands=big) == min(want, 1), where
                    assert froute(metric, dim, rows, 1, k, AUTO, P_BF16, tiles=tiles, cands=big) == min(want, 1), where
                    assert froute(metric, dim, rows, 1, k, AUTO, P_8BIT, tiles=tiles, cands=big) == 2 * min(want, 1), where   # the plane knob names the plane, not the form
                    assert froute(metric, dim, rows, 1, k, AUTO, P_AUTO, tiles=tiles, cands=k) == 0, where
                assert froute(metric, dim, rows, 1, k, AUTO, P_AUTO, tiles=0xFFFFFFFF, cands=big) == 2, (metric, k, dim, rows)
            for dim, rows in ((768, 999_999), (128, 9_999_999), (128, 1_000_000), (112, 10_000_000), (16, 50_000_000), (80, 6001)):   # not measured
                for plane in (P_AUTO, P_8BIT, P_BF16):
                    assert froute(metric, dim, rows, 1, k, AUTO, plane, cands=big) == 0, (metric, k, dim, rows, plane)
                assert froute(metric, dim, rows, 1, k, ALWAYS, P_AUTO, cands=big) == 1, (metric, k, dim, rows)   # forced on: the bfloat16 copy first where 8-bit first was not measured
                assert froute(metric, dim, rows, 1, k, ALWAYS, P_8BIT, cands=big) == 2, (metric, k, dim, rows)
        for k in (1001, 1024):                                          # above the largest measured k
            assert froute(metric, 768, 10_000_000, 1, k, AUTO, P_AUTO) == 0
            assert froute(metric, 768, 10_000_000, 1, k, ALWAYS, P_AUTO) == 1
        # forced on in a cell where 8-bit first lost: automatic plane -> the bfloat16 copy first
        assert froute(metric, 768, 1_000_000, 1, 100, ALWAYS, P_AUTO, tiles=tiles_of(1_000_000, 100), cands=big) == 1
        assert froute(metric, 768, 3_000_000, 1, 100, ALWAYS, P_AUTO, tiles=tiles_of(3_000_000, 100), cands=big) == 2
    assert froute(L2P, 768, 10_000_000, 1, 100, AUTO, P_AUTO) == 0      # Euclidean indexes with the planes: not measured
    assert froute(L2P, 768, 10_000_000, 1, 100, ALWAYS, P_8BIT) == 2


def test_unknown_modes_are_errors():
    for wide, plane in ((3, 0), (-1, 0), (0, 3), (0, -1), (99, 99)):
        assert froute(COSINE, 768, 1_000_000, 1, 100, wide, plane) < 0, (wide, plane)


def test_the_unfiltered_rule_is_what_it_was():
    """spot checks of tests/test_bound_scan_wide_cpu.py's own expectations: the new rule and its knob do not reach qv_scan_bound_wide_route"""
    for metric in (COSINE, DOT):
        for k in (65, 100, 128, 129, 256, 1000):
            for dim, rows in ((768, 1_000_000), (768, 10_000_000), (128, 10_000_000)):
                assert route(metric, dim, rows, 1, k, AUTO, P_AUTO) == 2
                assert route(metric, dim, rows, 1, k, AUTO, P_AUTO, 1, 0) == 1
                assert route(metric, dim, rows, 1, k, AUTO, P_BF16) == 1
            for dim, rows in ((768, 999_999), (128, 9_999_999), (80, 6001)):
                assert route(metric, dim, rows, 1, k, AUTO, P_AUTO) == 0
                assert route(metric, dim, rows, 1, k, ALWAYS, P_AUTO) == 1
                assert route(metric, dim, rows, 1, k, ALWAYS, P_8BIT) == 2
        assert route(metric, 768, 10_000_000, 1, 1001, AUTO, P_AUTO) == 0
    assert route(L2P, 768, 10_000_000, 1, 100, AUTO, P_AUTO) == 0
    assert route(L2P, 768, 10_000_000, 1, 100, ALWAYS, P_8BIT) == 2
    assert route(COSINE, 64, 1024, 1, 1024, ALWAYS, P_BF16) == 0 and route(COSINE, 64, 1025, 1, 1024, ALWAYS, P_BF16) == 1
    assert route(COSINE, 768, 1_000_000, 2, 100, ALWAYS, P_BF16) == 0 and route(COSINE, 768, 1_000_000, 1, 64, ALWAYS, P_BF16) == 0
