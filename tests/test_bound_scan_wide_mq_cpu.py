"""The wide form of the SHARED bound pass (2 - 8 queries, 65 <= k <= 1024; quiver_amd/csrc/qv_bound_scan.hip) without a GPU: the dispatch's own
rule (qv_scan_bound_wide_route_mq) over a grid and beside the single-query rule, which it must leave as it was; the layout of the form's
workspace (qv_scan_workspace_layout, kind QV_WS_BOUND_WIDE_MQ); and the per-query model the GPU file's counts stand on
(tests/_wide_mq.py), which for a pass of ONE query must be tests/_wide.py's.  No device is touched."""
import ctypes as C
import itertools

import numpy as np
import pytest

from quiver_amd import _lib
from tests import _oracle as O
from tests import _wide as Wd
from tests import _wide_mq as M

COSINE, L2, L2SQ, DOT, L1 = 0, 1, 2, 3, 4
L2P = _lib.QV_RULE_L2_PLANES
AUTO, ALWAYS, NEVER = 0, 1, 2
P_AUTO, P_8BIT, P_BF16 = 0, 1, 2
METRICS3 = (COSINE, DOT, L2P)
CAP = _lib.QV_BOUND_WIDE_CAND_CAP
CUS = 256                                           # an MI355X; the GPU file takes the number from the device


def route(metric, dim, rows, nq, k, wide, plane, has_plane=1, has_plane8=1):
    return _lib.lib().qv_scan_bound_wide_route_mq(metric, dim, rows, nq, k, wide, plane, has_plane, has_plane8)


def route_one(metric, dim, rows, nq, k, wide, plane, has_plane=1, has_plane8=1):
    return _lib.lib().qv_scan_bound_wide_route(metric, dim, rows, nq, k, wide, plane, has_plane, has_plane8)


GRID = list(itertools.product(METRICS3 + (L2, L2SQ, L1, 5, 8), (16, 80, 768, 4096, 24, 4112, 1), (511, 512, 6001, 1_000_000, 10_000_000),
                              (0, 1, 2, 3, 4, 5, 8, 9, 64), (1, 64, 65, 100, 128, 129, 1000, 1024, 1025), (AUTO, ALWAYS, NEVER), (P_AUTO, P_8BIT, P_BF16), (0, 1), (0, 1)))


def test_where_the_rule_says_no():
    for metric, dim, rows, nq, k, wide, plane, hp, hp8 in GRID:
        got = route(metric, dim, rows, nq, k, wide, plane, hp, hp8)
        assert got in (0, 1, 2), (metric, dim, rows, nq, k, wide, plane, hp, hp8, got)
        no = (k <= 64 or k > 1024 or nq < 2 or nq > 8 or metric not in METRICS3 or dim % 16 != 0 or dim > 4096 or (rows + 63) // 64 < 8 or not hp or wide == NEVER
              or k >= rows)
        if no:
            assert got == 0, (metric, dim, rows, nq, k, wide, plane, hp, hp8)
        elif wide == ALWAYS:
            assert got in (1, 2), (metric, dim, rows, nq, k, plane, hp, hp8)
        if got == 2:                                                     # never 2 without the 8-bit plane, nor under "bf16"
            assert hp8 and plane != P_BF16, (metric, dim, rows, nq, k, wide, plane, hp, hp8)


def test_automatic_is_inside_always_and_its_8bit_cells_inside_its_own():
    for metric, dim, rows, nq, k, _, plane, hp, hp8 in GRID:
        auto = route(metric, dim, rows, nq, k, AUTO, plane, hp, hp8)
        if route(metric, dim, rows, nq, k, ALWAYS, plane, hp, hp8) == 0:
            assert auto == 0, (metric, dim, rows, nq, k, plane, hp, hp8)
        if plane == P_AUTO and auto == 2:                                # 8-bit first is automatic only where the form itself is
            assert route(metric, dim, rows, nq, k, AUTO, P_BF16, hp, hp8) == 1, (metric, dim, rows, nq, k, hp, hp8)
        if metric == L2P:                                                # Euclidean indexes with the planes: under ALWAYS alone
            assert auto == 0, (dim, rows, nq, k, plane)


@pytest.mark.parametrize("metric", METRICS3)
def test_always_and_the_plane_knob(metric):
    for nq in (2, 3, 4, 5, 8):
        for k in (65, 128, 129, 1024):
            for dim, rows in ((16, 2000), (80, 6001), (768, 1_000_000), (4096, 1_000_000)):
                assert route(metric, dim, rows, nq, k, ALWAYS, P_8BIT) == 2, (nq, k, dim, rows)
                assert route(metric, dim, rows, nq, k, ALWAYS, P_8BIT, 1, 0) == 1, (nq, k, dim, rows)   # the plane is not held: the bfloat16 copy first
                assert route(metric, dim, rows, nq, k, ALWAYS, P_BF16) == 1, (nq, k, dim, rows)
                assert route(metric, dim, rows, nq, k, ALWAYS, P_AUTO) in (1, 2), (nq, k, dim, rows)
                assert route(metric, dim, rows, nq, k, ALWAYS, P_8BIT, 0, 1) == 0, (nq, k, dim, rows)   # never without the bfloat16 copy behind it


def test_the_shape_limits():
    assert route(COSINE, 64, 1024, 2, 1024, ALWAYS, P_BF16) == 0        # k takes every row: nothing to reject
    assert route(COSINE, 64, 1025, 2, 1024, ALWAYS, P_BF16) == 1
    assert route(COSINE, 64, 64_000_000, 2, 100, ALWAYS, P_BF16) == 1   # two key planes of the redo fit a gibibyte, two planes of lower bounds two ...
    assert route(COSINE, 64, 70_000_000, 2, 100, ALWAYS, P_BF16) == 0   # ... and no longer
    assert route(COSINE, 64, 16_000_000, 8, 100, ALWAYS, P_BF16) == 1   # eight planes of lower bounds: 2 GiB at 8M tiles ...
    assert route(COSINE, 64, 64 * (1 << 20), 8, 100, ALWAYS, P_BF16) == 1
    assert route(COSINE, 64, 64 * (1 << 20) + 1, 8, 100, ALWAYS, P_BF16) == 0


def test_the_single_query_rule_is_what_it_was():
    """qv_scan_bound_wide_route keeps answering 0 for nq != 1, whatever this form's rule says, and its answers for one query do not depend
    on anything of this form's"""
    for metric, dim, rows, nq, k, wide, plane, hp, hp8 in GRID:
        if nq != 1:
            assert route_one(metric, dim, rows, nq, k, wide, plane, hp, hp8) == 0, (metric, dim, rows, nq, k, wide, plane)
    for metric in (COSINE, DOT):
        for k in (65, 100, 1000):
            assert route_one(metric, 768, 1_000_000, 1, k, AUTO, P_AUTO) == 2 and route_one(metric, 128, 10_000_000, 1, k, AUTO, P_AUTO) == 2
            assert route_one(metric, 768, 999_999, 1, k, AUTO, P_AUTO) == 0 and route_one(metric, 80, 6001, 1, k, ALWAYS, P_8BIT) == 2


def test_unmeasured_shapes_are_never_automatic():
    """whatever the measured floors are: fewer than 1M rows, narrower than 128 dimensions, 128 to 767 dimensions below 10M rows, k above 1000
    and Euclidean indexes were not measured"""
    for metric in METRICS3:
        for nq in (2, 4, 5, 8):
            for k in (65, 100, 1000, 1024):
                for dim, rows in ((768, 999_999), (128, 9_999_999), (512, 3_000_000), (112, 10_000_000), (16, 50_000_000), (80, 6001)):
                    assert route(metric, dim, rows, nq, k, AUTO, P_AUTO) == 0, (metric, nq, k, dim, rows)
                    assert route(metric, dim, rows, nq, k, AUTO, P_8BIT) == 0, (metric, nq, k, dim, rows)
            for k in (1001, 1024):
                assert route(metric, 768, 10_000_000, nq, k, AUTO, P_AUTO) == 0
    assert route(L2P, 768, 10_000_000, 4, 100, AUTO, P_AUTO) == 0 and route(L2P, 768, 10_000_000, 4, 100, ALWAYS, P_8BIT) == 2


def test_unknown_modes_are_errors():
    for wide, plane in ((3, 0), (-1, 0), (0, 3), (0, -1), (99, 99)):
        assert route(COSINE, 768, 1_000_000, 4, 100, wide, plane) < 0, (wide, plane)


REGION_CAP = 16
WS_FLAT_SELECT_REDO = 6                             # QV_WS_FLAT_SELECT_REDO of include/qv.h: the key-per-row redo's own workspace


def layout(kind, dim, rows, nq, k, cus=CUS, metric=COSINE):
    total, end, n = C.c_uint64(), C.c_uint64(), C.c_uint32()
    regs = (C.c_uint64 * (4 * REGION_CAP))()
    rc = _lib.lib().qv_scan_workspace_layout(kind, metric, dim, rows, nq, k, cus, 0, C.byref(total), C.byref(end), C.byref(n), regs, REGION_CAP)
    assert rc == 0 and 0 < n.value <= REGION_CAP, (rc, n.value, _lib.lib().qv_last_error())
    flat = regs[:4 * n.value]
    return total.value, end.value, [tuple(flat[i:i + 4]) for i in range(0, len(flat), 4)]


ROWS = (512, 2000, 6001, 200_000, 1_000_000, 10_000_000)
KS = (65, 100, 128, 129, 500, 1024)


@pytest.mark.parametrize("dim", [16, 80, 768, 4096])
@pytest.mark.parametrize("cus", [1, 256])
def test_workspace_regions_lie_apart_and_inside(dim, cus):
    for rows in ROWS:
        n_tiles = (rows + 63) // 64
        grid, _ = Wd.plan(n_tiles, cus)
        for nq in (2, 4, 5, 8):
            for k in KS:
                total, end, regs = layout(_lib.QV_WS_BOUND_WIDE_MQ, dim, rows, nq, k, cus)
                assert 0 < end <= total, (rows, nq, k, end, total)
                plain = [r for r in regs if not r[3]]
                alias = [r for r in regs if r[3]]
                assert len(alias) == 1 and len(plain) == 10, regs       # only the redo's workspace overlays; the flag words and the nine regions of the bound stages
                at = 0
                for off, size, align, _ in plain:                      # in order, apart, aligned, none empty
                    assert size > 0 and off >= at and off % align == 0, (rows, nq, k, regs)
                    at = off + size
                assert at <= end
                flags = plain[0]
                assert flags[0] == 0 and flags[1] == 256                # the pass's flag words come first ...
                for off, size, align, _ in alias:                      # ... and the redo, which reads its flags from them, lies behind them
                    assert size > 0 and off % align == 0 and off >= flags[0] + flags[1] and off + size <= end, (rows, nq, k, regs)
                sizes = [r[1] for r in plain]
                assert sizes[1] == nq * Wd.lists_bytes(grid), (rows, nq, k, cus, sizes)   # lists = nq x grid x 4 x 64 keys
                assert nq * CAP * 4 in sizes and nq * CAP * 8 in sizes and nq * n_tiles * 256 in sizes, (rows, nq, k, sizes)
                # the redo is the key-per-row redo's own workspace for the same shape, whole
                redo_total = layout(WS_FLAT_SELECT_REDO, dim, rows, nq, k, cus)[0]
                assert alias[0][1] == redo_total and total >= redo_total, (rows, nq, k, alias, redo_total)


def test_workspace_total_is_monotone_in_rows_k_and_queries():
    for dim in (16, 768):
        for nq in (2, 8):
            for k in KS:
                totals = [layout(_lib.QV_WS_BOUND_WIDE_MQ, dim, rows, nq, k)[0] for rows in ROWS]
                assert totals == sorted(totals), (dim, nq, k, totals)
        for rows in ROWS:
            totals = [layout(_lib.QV_WS_BOUND_WIDE_MQ, dim, rows, nq, 100)[0] for nq in range(2, 9)]
            assert totals == sorted(totals), (dim, rows, totals)


@pytest.mark.parametrize("name", ["plain", "loose_one"])
def test_a_pass_of_one_query_is_the_single_query_model(name):
    """tests/_wide.py's pinned cases (256 compute units; nothing dropped / a wave that holds more than it publishes), asked through the pass's
    model with one query: H, the rows passed on, the count, the fate and the dropped keys are tests/_wide.model's"""
    c = Wd.case(name, CUS)
    n = len(Wd.base(c["base"], CUS)[0])
    n_tiles = -(-n // 64)
    grid = Wd.plan(n_tiles, CUS)[0]
    live = Wd.live_of(c, CUS)
    for arm in Wd.ARMS:
        for k in c["ks"]:
            want = Wd.model(name, CUS, arm, k)
            (got,) = M.decide_stages([Wd.case_stage(name, CUS, arm)], k, live, n_tiles, grid)
            assert got["H"] == want["H"] and got["count"] == want["count"] and got["hand_back"] == want["hand_back"] and got["dropped"] == want["dropped"]
            assert np.array_equal(got["passed"], want["passed"]), (name, arm, k)


@pytest.mark.parametrize("metric", [COSINE, L2, DOT])
def test_every_query_of_a_pass_has_its_own_lists_and_its_own_fate(metric):
    """over a shared row state: query j of a pass is tests/_wide.decide_wide over tests/_wide.stage_of of query j alone, whatever the other
    queries are — a zero query and a NaN query beside it are declined on their own and change nothing; and the pass's counters are made
    of the per-query answers"""
    dim, n, k = 80, 6001, 100
    rows = O.gen_rows(7400, 0, n, dim)
    qs = O.gen_rows(7401, 0, 3, dim)
    n_tiles = -(-n // 64)
    grid = Wd.plan(n_tiles, CUS)[0]
    live = np.ones(n, bool)
    states = M.States(rows)
    bad = np.stack([np.zeros(dim, np.float32), qs[0], qs[1], qs[2]]); bad[3, 5] = np.nan
    for arm in Wd.ARMS:
        alone = [Wd.decide_wide(Wd.stage_of(metric, arm, rows, q), k, live, n_tiles, grid) for q in qs[:2]]
        for got, want in zip(M.decide_pass(metric, arm, states, qs[:2], k, live, n_tiles, grid), alone):
            assert got["H"] == want["H"] and got["count"] == want["count"] and not got["hand_back"] and np.array_equal(got["passed"], want["passed"])
        mixed = M.decide_pass(metric, arm, states, bad, k, live, n_tiles, grid)
        assert mixed[0] is None and mixed[3] is None and [m["count"] for m in mixed[1:3]] == [a["count"] for a in alone]
    for plane in Wd.ARMS:
        f = M.fates(metric, plane, states, bad, k, live, n_tiles, grid)
        assert [s for s, _, _ in f["per_query"]] == ["redo", plane, plane, "redo"] and f["back"] == 2 and f["took"] == 4
        assert f["cand"] == max(c for _, c, _ in f["per_query"]) and k <= f["cand"] <= CAP
