"""The 8-bit stage in front of a FILTERED shared pass of 2 - 8 queries (k_bound_scan8_mq<., ., true>, quiver_amd/csrc/qv_bound_scan.hip) without a
GPU: the rule that puts it there (qv_scan_bound8_applies_filtered_mq) over the grid of tests/test_bound_scan8_filtered_cpu.py, that nothing the
library decided before has moved, and that the inputs of the device test's width cases (tests/_widths.py: a set per query, one mask for all) can
tell a right kernel from a wrong one: every survivor count the device test compares changes when one ladder block is left out of the integer
sum, most of them differ from the unfiltered counts, and no query of them is handed on."""
import itertools

import pytest

import quiver_amd
from quiver_amd import _lib
from tests import _route as R
from tests import _widths as W
from tests._route import ALWAYS, AUTO, NEVER, NO_FILTER
from tests.test_flat_route_cpu import DIMS, KS, METRICS, MODES, NQS, ROWS, _candidate_tiles

COS, DOT = R.M["cosine"], R.M["dot"]
P_AUTO, P_8BIT, P_BF16 = 0, 1, 2


def rule(metric, dim, rows, nq, k, mode, pmode, plane8, ct):
    rc = _lib.lib().qv_scan_bound8_applies_filtered_mq(metric, dim, rows, nq, k, mode, pmode, plane8, ct)
    assert rc in (0, 1), rc
    return bool(rc)


def rule_mq(metric, dim, rows, nq, k, mode, pmode, plane8):
    rc = _lib.lib().qv_scan_bound8_applies_mq(metric, dim, rows, nq, k, mode, pmode, plane8)
    assert rc in (0, 1), rc
    return bool(rc)


def test_the_rule_on_the_route_grid():
    taken = 0
    for metric, dim, rows, nq, k in itertools.product(METRICS, DIMS, ROWS, NQS, KS):
        for mode, pmode, plane8, ct in itertools.product(MODES, (P_AUTO, P_8BIT, P_BF16), (0, 1), _candidate_tiles(rows)[1:]):
            args = (metric, dim, rows, nq, k, mode, pmode, plane8, ct)
            got = rule(*args)
            base = R.bound_rule(metric, dim, rows, nq, k, mode, 1, ct)     # the filtered bound rule, asked with the copy held
            if not 2 <= nq <= 8 or metric not in (COS, DOT) or not plane8 or pmode == P_BF16 or mode == NEVER:
                assert not got, args
            if pmode == P_8BIT:                                           # "8bit": whenever those hold
                assert got == (base and 2 <= nq <= 8 and bool(plane8)), args
            if pmode == P_AUTO and got:                                   # AUTO is inside 8BIT, and inside the unfiltered pass's AUTO at the same shape
                assert rule(metric, dim, rows, nq, k, mode, P_8BIT, plane8, ct), args
                assert rule_mq(metric, dim, rows, nq, k, mode, P_AUTO, plane8), args
                assert dim >= 768, args                                   # never below kBound8MinDim
            taken += got
            # the single-query filtered rule knows nothing of shared passes
            if nq > 1:
                for pf in (P_AUTO, P_8BIT, P_BF16):
                    assert _lib.lib().qv_scan_bound8_applies_filtered(metric, dim, rows, nq, k, mode, pf, plane8, ct) == 0, (args, pf)
    assert taken > 0


def test_the_python_wrapper_and_bad_modes():
    assert quiver_amd.scan_bound8_applies_filtered_mq("cosine", 768, 10_000_000, 4, 10, "always", "8bit") is True
    assert quiver_amd.scan_bound8_applies_filtered_mq("cosine", 768, 10_000_000, 4, 10, "always", "8bit", candidate_tiles=0) is True
    assert quiver_amd.scan_bound8_applies_filtered_mq("cosine", 768, 10_000_000, 4, 10, "auto", "8bit", candidate_tiles=0) is False
    assert quiver_amd.scan_bound8_applies_filtered_mq("cosine", 768, 10_000_000, 8, 10, "auto", "8bit", candidate_tiles=10_000_000 // 64) is True
    assert quiver_amd.scan_bound8_applies_filtered_mq("cosine", 768, 10_000_000, 4, 10, "always", "bf16") is False
    assert quiver_amd.scan_bound8_applies_filtered_mq("cosine", 768, 10_000_000, 4, 10, "never", "8bit") is False
    assert quiver_amd.scan_bound8_applies_filtered_mq("cosine", 768, 10_000_000, 4, 10, "always", "8bit", has_plane8=False) is False
    assert quiver_amd.scan_bound8_applies_filtered_mq("cosine", 768, 10_000_000, 1, 10, "always", "8bit") is False
    assert quiver_amd.scan_bound8_applies_filtered_mq("cosine", 768, 10_000_000, 9, 10, "always", "8bit") is False
    assert quiver_amd.scan_bound8_applies_filtered_mq("l2", 768, 10_000_000, 4, 10, "always", "8bit") is False
    # the shape whose decline tests/test_gpu_search_where.py pins: far below any floor of the automatic rule
    assert quiver_amd.scan_bound8_applies_filtered_mq("cosine", 128, 20_011, 8, 10, "auto", "auto", candidate_tiles=313) is False
    assert quiver_amd.scan_bound8_applies_filtered_mq("cosine", 128, 20_011, 8, 10, "auto", "8bit", candidate_tiles=313) is False
    assert _lib.lib().qv_scan_bound8_applies_filtered_mq(COS, 768, 10_000_000, 4, 10, 3, AUTO, 1, 100) < 0
    assert _lib.lib().qv_scan_bound8_applies_filtered_mq(COS, 768, 10_000_000, 4, 10, AUTO, 3, 1, 100) < 0


# The automatic rule's cells as profiles/LAB_r13_bound_scan8_filtered_mq.md records them (768 dimensions, k = 1, 10, 64, nq 2, 4, 5, 8): with
# nine tenths of the tiles or more holding a candidate a win at every k from 3M rows, at 1M losses at k = 64; sparser candidate tiles: declined.
AUTO_TABLE = {   # (rows, f >= 0.9) -> taken
    (1_000_000, True): False, (3_000_000, True): True, (10_000_000, True): True,
    (1_000_000, False): False, (3_000_000, False): False, (10_000_000, False): False,
}


def test_the_automatic_cells_are_the_lab_notes_table():
    for (rows, dense), taken in AUTO_TABLE.items():
        tiles = (rows + 63) // 64
        ct = tiles if dense else tiles * 8 // 10
        for nq, k in itertools.product((2, 4, 5, 8), (1, 10, 64)):
            assert rule(COS, 768, rows, nq, k, ALWAYS, P_AUTO, 1, ct) == taken, (rows, dense, nq, k)
            # with the bound scan itself automatic: inside the filtered bound rule's own cells
            assert rule(COS, 768, rows, nq, k, AUTO, P_AUTO, 1, ct) == (taken and R.bound_rule(COS, 768, rows, nq, k, AUTO, 1, ct)), (rows, dense, nq, k)
    assert rule(COS, 768, 2_999_999, 4, 10, ALWAYS, P_AUTO, 1, 2_999_999 // 64 + 1) is False
    assert rule(COS, 752, 10_000_000, 4, 10, ALWAYS, P_AUTO, 1, 10_000_000 // 64) is False      # narrower than measured
    assert rule(DOT, 1024, 10_000_000, 8, 64, ALWAYS, P_AUTO, 1, 10_000_000 // 64) is True


def test_nothing_the_library_decided_before_has_moved():
    """the route of a masked shared pass is bound_mq or not whatever the new mode would be: qv_scan_route_ex has no argument for it, and the
    unfiltered shared pass's rule does not see candidate tiles"""
    for dim, rows, nq, k in ((768, 10_000_000, 4, 10), (768, 1_000_000, 8, 64), (768, 300_000, 5, 10), (128, 20_011, 8, 10)):
        tiles = (rows + 63) // 64
        for bmode, ct in itertools.product(MODES, (0, tiles // 10, tiles)):
            args = (COS, dim, rows, nq, k, 1, bmode, AUTO, 1, 1, ct)
            assert R.library_route(*args) == R.expected_route(*args), args
        assert rule_mq(COS, dim, rows, nq, k, ALWAYS, P_8BIT, 1) and not rule_mq(COS, dim, rows, nq, k, ALWAYS, P_BF16, 1)
    assert NO_FILTER == 0xFFFFFFFF


# ---- the width inputs under filters ------------------------------------------------------------------------------------------------------
def counts_sets(metric, dim, skip=None):
    """the largest survivor count of the pass per (nq, k), every query over its own set — what the device reports of search_rowsets"""
    c = W.case(dim)
    return tuple(max(W.model8(metric, dim, j, k, W.alive_of(c["live"], c["masks"][j]), skip)["count"] for j in range(nq)) for nq in W.NQS for k in W.KS)


def counts_mask(metric, dim, skip=None):
    """... every query over live & mask — search_masked"""
    c = W.case(dim)
    return tuple(max(W.model8(metric, dim, j, k, c["live"] & c["mask"], skip)["count"] for j in range(nq)) for nq in W.NQS for k in W.KS)


def counts_live(metric, dim):
    c = W.case(dim)
    return tuple(max(W.model8(metric, dim, j, k, c["live"])["count"] for j in range(nq)) for nq in W.NQS for k in W.KS)


@pytest.mark.parametrize("metric", [COS, DOT])
@pytest.mark.parametrize("dim", W.WIDTHS)
def test_the_width_inputs_tell_a_right_kernel_from_a_wrong_one(metric, dim):
    c = W.case(dim)
    true_sets, true_mask, unfiltered = counts_sets(metric, dim), counts_mask(metric, dim), counts_live(metric, dim)
    for u, skip in W.left_out(dim, W.LADDER8).items():
        assert counts_sets(metric, dim, skip) != true_sets, (dim, "integer sum without its %d-step block" % u, skip, true_sets)
        assert counts_mask(metric, dim, skip) != true_mask, (dim, "integer sum without its %d-step block" % u, skip, true_mask)
    # a kernel that ignored the sets (or the mask) would report the unfiltered counts
    assert sum(a != b for a, b in zip(true_sets, unfiltered)) >= 7, (dim, true_sets, unfiltered)
    assert sum(a != b for a, b in zip(true_mask, unfiltered)) >= 7, (dim, true_mask, unfiltered)
    # the device test asserts that the 8-bit stage answered alone
    for j, k in itertools.product(range(max(W.NQS)), W.KS):
        assert not W.model8(metric, dim, j, k, W.alive_of(c["live"], c["masks"][j]))["hand_back"], (dim, j, k)
        assert not W.model8(metric, dim, j, k, c["live"] & c["mask"])["hand_back"], (dim, j, k)
