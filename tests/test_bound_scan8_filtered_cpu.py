"""The 8-bit stage in front of a FILTERED single query, without a GPU: the dispatch's own rule (qv_scan_bound8_applies_filtered) and the
route it gives (qv_scan_route_ex), on the grid of tests/test_flat_route_cpu.py restricted to the bound scan's metrics.  The filtered
plane mode is a knob of its own: qv_scan_route is qv_scan_route_ex under "bf16", unfiltered cells do not see the argument, and under
"8bit" exactly the filtered cells on route `bound` of an index that holds the plane move to `bound8_first`."""
import itertools

from quiver_amd import _lib
from tests import _route as R
from tests._route import ALWAYS, AUTO, NEVER, NO_FILTER
from tests.test_flat_route_cpu import DIMS, KS, MODES, NQS, PLANES, ROWS, _candidate_tiles

METRICS = tuple(R.M[m] for m in ("cosine", "dot"))
P_AUTO, P_8BIT, P_BF16 = 0, 1, 2
# the unfiltered 8-bit stage's automatic floors (quiver_amd/csrc/qv_bound_scan.hip: kBound8MinRows at 768 dimensions or more,
# kBound8NarrowRows from 128; narrower never)
FLOOR_768, FLOOR_128 = 3_000_000, 10_000_000


def route_ex(metric, dim, rows, nq, k, tickets, bmode, pmode, plane, plane8, ct, fmode, cus=R.CUS):
    return _lib.lib().qv_scan_route_ex(metric, dim, rows, nq, k, cus, tickets, bmode, pmode, plane, plane8, ct, fmode)


def rule8f(metric, dim, rows, nq, k, bmode, fmode, plane8, ct):
    rc = _lib.lib().qv_scan_bound8_applies_filtered(metric, dim, rows, nq, k, bmode, fmode, plane8, ct)
    assert rc in (0, 1), rc
    return bool(rc)


def test_the_route_under_each_filtered_plane_mode_on_the_whole_grid():
    moved = 0
    for metric, dim, rows, nq, k in itertools.product(METRICS, DIMS, ROWS, NQS, KS):
        for tickets, bmode, pmode, (plane, plane8), ct in itertools.product((0, 1), MODES, MODES, PLANES, _candidate_tiles(rows)):
            args = (metric, dim, rows, nq, k, tickets, bmode, pmode, plane, plane8, ct)
            base = R.library_route(*args)
            assert route_ex(*args, P_BF16) == base, args                  # qv_scan_route is qv_scan_route_ex under "bf16"
            got = route_ex(*args, P_8BIT)
            if base == R.BOUND and ct != NO_FILTER and plane8:
                assert got == R.BOUND8_FIRST, args
                assert rule8f(metric, dim, rows, nq, k, bmode, P_8BIT, plane8, ct), args
                moved += 1
            else:
                assert got == base, (args, got)
            auto = route_ex(*args, P_AUTO)
            if ct == NO_FILTER:
                assert got == base and auto == base, args                  # unfiltered cells do not depend on the new argument
            else:
                want8 = base == R.BOUND and rule8f(metric, dim, rows, nq, k, bmode, P_AUTO, plane8, ct)
                assert auto == (R.BOUND8_FIRST if want8 else base), (args, auto)
    assert moved > 0


def test_the_rule_implies_the_filtered_bound_rule_and_respects_its_modes():
    yes = 0
    for metric, dim, rows, nq, k in itertools.product(METRICS, DIMS, ROWS, NQS, KS):
        for bmode, fmode, plane8, ct in itertools.product(MODES, (P_AUTO, P_8BIT, P_BF16), (0, 1), _candidate_tiles(rows)[1:]):
            got = rule8f(metric, dim, rows, nq, k, bmode, fmode, plane8, ct)
            if not got:
                continue
            yes += 1
            assert R.bound_rule(metric, dim, rows, nq, k, bmode, 1, ct), (metric, dim, rows, nq, k, bmode, ct)   # asked with the copy held
            assert nq == 1 and fmode != P_BF16 and bmode != NEVER and plane8, (nq, fmode, bmode, plane8)
            if fmode == P_AUTO:                                           # never below the unfiltered 8-bit floors
                assert dim >= 128 and rows >= (FLOOR_768 if dim >= 768 else FLOOR_128), (dim, rows)
            # 8BIT: whenever the conditions hold
        for bmode, plane8, ct in itertools.product(MODES, (0, 1), _candidate_tiles(rows)[1:]):
            want = nq == 1 and bool(plane8) and R.bound_rule(metric, dim, rows, 1, k, bmode, 1, ct)
            assert rule8f(metric, dim, rows, nq, k, bmode, P_8BIT, plane8, ct) == want, (metric, dim, rows, nq, k, bmode, plane8, ct)
    assert yes > 0


# The automatic rule's cells as profiles/LAB_r11_bound_scan8_filtered.md records them (768 dimensions, k = 1, 10, 64, 8-bit first against
# the parent commit's library): with every tile a candidate (f >= 0.9: a full set, a random 1 % set, where-filters of 10 % and 100 %) a
# win at every k from 3M rows, at 1M a loss at k = 64; with one tile in ten a loss at 1M, no gain at k = 64 at 3M, a loss at k = 64 at 10M:
# declined at every row count; between the two nothing was measured: declined.
AUTO_TABLE = {   # (rows, f >= 0.9) -> taken
    (1_000_000, True): False, (3_000_000, True): True, (10_000_000, True): True,
    (1_000_000, False): False, (3_000_000, False): False, (10_000_000, False): False,
}


def test_the_automatic_cells_are_the_lab_notes_table():
    cos = R.M["cosine"]
    for (rows, dense), taken in AUTO_TABLE.items():
        tiles = (rows + 63) // 64
        ct = tiles if dense else (tiles + 9) // 10
        for k, bmode in itertools.product((1, 10, 64), (AUTO, ALWAYS)):
            assert rule8f(cos, 768, rows, 1, k, bmode, P_AUTO, 1, ct) == taken, (rows, dense, k, bmode)
    # and on the whole grid: the table's rule, never below the unfiltered floors, never narrower than measured, never between the fractions
    for metric, dim, rows, k in itertools.product(METRICS, DIMS, ROWS, KS):
        tiles = (rows + 63) // 64
        for bmode, ct in itertools.product((AUTO, ALWAYS), (0, tiles // 10, (tiles + 9) // 10, tiles // 2, tiles * 9 // 10 + 1, tiles)):
            want = (dim >= 768 and rows >= FLOOR_768 and ct * 10 >= tiles * 9 and R.bound_rule(metric, dim, rows, 1, k, bmode, 1, ct))
            assert rule8f(metric, dim, rows, 1, k, bmode, P_AUTO, 1, ct) == want, (metric, dim, rows, k, bmode, ct)


def test_bad_modes_are_errors():
    cos = R.M["cosine"]
    assert _lib.lib().qv_scan_bound8_applies_filtered(cos, 768, 3_000_000, 1, 10, AUTO, 3, 1, 100) < 0
    assert _lib.lib().qv_scan_bound8_applies_filtered(cos, 768, 3_000_000, 1, 10, 3, AUTO, 1, 100) < 0
    assert route_ex(cos, 768, 3_000_000, 1, 10, 1, AUTO, AUTO, 1, 1, 100, 3) < 0
