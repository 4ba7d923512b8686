"""The route of a fused flat search (k <= 64) without a GPU: the library's one decision (quiver_amd/csrc/qv_scan.hip: plan_flat, through
qv_scan_route) against the priority order restated in tests/_route.py, on the full product of the shapes below with the default
environment knobs, and the properties the dispatch used to guarantee by the way its branches were nested."""
import itertools

from tests import _route as R
from tests._route import ALWAYS, AUTO, NEVER, NO_FILTER

METRICS = tuple(R.M[m] for m in ("cosine", "dot", "l2", "l1", "l2sq"))
DIMS = (16, 100, 128, 768, 4096)
ROWS = (400, 600, 20_011, 100_000, 530_000, 1_000_000, 3_000_000, 10_000_000)
NQS = (1, 2, 4, 5, 8, 9, 33, 40, 256)
KS = (1, 10, 16, 17, 64)
PLANES = ((0, 0), (1, 0), (1, 1))                            # none, the bfloat16 copy, both
MODES = (AUTO, ALWAYS, NEVER)


def _candidate_tiles(rows):
    tiles = (rows + 63) // 64
    return (NO_FILTER, 0, tiles // 10, tiles)


def test_the_route_is_the_restated_order_on_the_whole_grid():
    """every cell: qv_scan_route == tests/_route.py; every route reached; and per cell what the nesting of the old dispatch guaranteed"""
    reached = set()
    cells = 0
    for metric, dim, rows, nq, k in itertools.product(METRICS, DIMS, ROWS, NQS, KS):
        for tickets, bmode, pmode, (plane, plane8), ct in itertools.product((0, 1), MODES, MODES, PLANES, _candidate_tiles(rows)):
            args = (metric, dim, rows, nq, k, tickets, bmode, pmode, plane, plane8, ct)
            got = R.library_route(*args)
            assert got == R.expected_route(*args), (args, got)
            reached.add(got)
            cells += 1
            if got in R.BOUND_ROUTES:                        # a bound route only when the matching exported rule says yes
                assert tickets and R.bound_rule(metric, dim, rows, nq, k, bmode, plane, ct), args
                assert bmode != NEVER, args
            if got == R.BOUND8_FIRST:                        # never under a filter, never against the plane mode, only with the rule's yes
                assert ct == NO_FILTER and pmode != NEVER and R.bound8_rule(metric, dim, rows, nq, k, bmode, pmode, plane8), args
            if not tickets:
                assert got in (R.SPLIT_MQ, R.MQ64, R.MQ, R.TWO_LAUNCH), args
    assert cells == 5 * 5 * 8 * 9 * 5 * 2 * 3 * 3 * 3 * 4
    assert reached == set(range(len(R.ROUTES))), sorted(R.ROUTES[r] for r in set(range(len(R.ROUTES))) - reached)


def test_the_route_numbers_are_the_priority_order():
    assert R.ROUTES == ("small", "bound_mq", "split_mq", "mq64", "mq", "bound", "bound8_first", "split", "fused", "two_launch")
    cos = R.M["cosine"]
    assert R.library_route(cos, 16, 600, 1, 10, 1, NEVER, AUTO, 1, 1, NO_FILTER) == R.SMALL
    assert R.library_route(cos, 16, 600, 4, 10, 1, ALWAYS, AUTO, 1, 1, NO_FILTER) == R.BOUND_MQ
    assert R.library_route(cos, 256, 2000, 4, 17, 1, AUTO, AUTO, 1, 1, NO_FILTER) == R.SPLIT_MQ      # (k <= 16 with tickets: small)
    assert R.library_route(cos, 16, 530_000, 12, 10, 1, AUTO, AUTO, 1, 1, NO_FILTER) == R.MQ64
    assert R.library_route(cos, 16, 530_000, 4, 10, 1, AUTO, AUTO, 1, 1, NO_FILTER) == R.MQ
    assert R.library_route(cos, 768, 1_000_000, 1, 10, 1, AUTO, AUTO, 1, 1, NO_FILTER) == R.BOUND
    assert R.library_route(cos, 768, 3_000_000, 1, 10, 1, AUTO, AUTO, 1, 1, NO_FILTER) == R.BOUND8_FIRST
    assert R.library_route(cos, 256, 2000, 1, 10, 1, AUTO, AUTO, 1, 1, NO_FILTER) == R.SPLIT
    assert R.library_route(cos, 16, 100_000, 1, 10, 1, AUTO, AUTO, 1, 1, NO_FILTER) == R.FUSED
    assert R.library_route(cos, 16, 100_000, 1, 10, 0, AUTO, AUTO, 1, 1, NO_FILTER) == R.TWO_LAUNCH


def test_a_filtered_query_takes_the_skipping_form_never_the_8_bit_stage():
    cos = R.M["cosine"]
    tiles = (3_000_000 + 63) // 64
    assert R.library_route(cos, 768, 3_000_000, 1, 10, 1, AUTO, ALWAYS, 1, 1, tiles) == R.BOUND
    assert R.library_route(cos, 768, 3_000_000, 1, 10, 1, AUTO, ALWAYS, 1, 1, (tiles + 9) // 10) == R.BOUND       # one tile in ten, rounded up: the sparsest the rule takes
    assert R.library_route(cos, 768, 3_000_000, 1, 10, 1, AUTO, ALWAYS, 1, 1, 0) == R.FUSED    # no candidate tile: the automatic rule declines


def test_arguments_no_route_serves_are_errors():
    cos = R.M["cosine"]
    ok = (cos, 16, 600, 1, 10, 1, AUTO, AUTO, 1, 1, NO_FILTER)
    assert R.library_route(*ok) >= 0
    for i, bad in ((0, 99), (1, 0), (2, 0), (3, 0), (4, 0), (4, 65), (6, 3), (7, 3)):
        args = list(ok)
        args[i] = bad
        assert R.library_route(*args) < 0, args
    assert R.library_route(*ok, cus=0) < 0
