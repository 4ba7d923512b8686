"""The dispatch rule of the bound scan (quiver_amd/csrc/qv_bound_scan.hip: bound_scan_rule) on the host, through qv_scan_bound_applies: which
(metric, dim, rows, nq, k, mode) take the path on the bfloat16 copy — one query as before, 2 to 8 queries as a shared pass.

The shared pass keeps the single-query sum: k_bound_scan_mq's packed fmas pair two QUERIES, each half one (query, row) chain of dim
in-order fused multiply-adds.  tests/test_bound_scan_cpu.py's containment check of qv_scan_bound_interval therefore covers it as it is."""
import itertools

import pytest

import quiver_amd
from quiver_amd import _lib

COSINE, L2, DOT = quiver_amd.metric_id("cosine"), quiver_amd.metric_id("l2"), quiver_amd.metric_id("dot")
AUTO, ALWAYS, NEVER = 0, 1, 2


def applies(metric, dim, rows, nq, k, mode, has_plane=1):
    rc = _lib.lib().qv_scan_bound_applies(metric, dim, rows, nq, k, mode, has_plane)
    assert rc in (0, 1), rc
    return bool(rc)


GRID = list(itertools.product((COSINE, DOT), (16, 128, 768, 4096), (600, 20_011, 530_000, 1_000_000, 10_000_000), (1, 2, 4, 5, 8), (1, 10, 64)))


def test_never_means_never():
    for metric, dim, rows, nq, k in GRID:
        assert not applies(metric, dim, rows, nq, k, NEVER)


def test_always_means_whenever_it_applies():
    for metric, dim, rows, nq, k in GRID:
        assert applies(metric, dim, rows, nq, k, ALWAYS)
    for nq in (1, 2, 8):
        assert not applies(L2, 128, 1_000_000, nq, 10, ALWAYS)             # the metrics are cosine and dot
        assert not applies(COSINE, 100, 1_000_000, nq, 10, ALWAYS)         # whole 16-dimension steps
        assert not applies(COSINE, 4112, 1_000_000, nq, 10, ALWAYS)        # up to 4096 dimensions
        assert not applies(COSINE, 128, 1_000_000, nq, 65, ALWAYS)         # a fused-list k
        assert not applies(COSINE, 128, 1_000_000, nq, 0, ALWAYS)
        assert not applies(COSINE, 128, 1_000_000, nq, 10, ALWAYS, has_plane=0)
        assert not applies(COSINE, 128, 400, nq, 10, ALWAYS)               # fewer than 8 tiles
    assert not applies(COSINE, 128, 1_000_000, 0, 10, ALWAYS)


@pytest.mark.parametrize("mode", [AUTO, ALWAYS, NEVER])
def test_nine_queries_are_the_filters(mode):
    for metric, dim, rows, _, k in GRID:
        assert not applies(metric, dim, rows, 9, k, mode)
        assert not applies(metric, dim, rows, 256, k, mode)


def test_one_query_answers_as_before():
    """automatic: from 300 000 rows on, whatever the width"""
    for metric, dim, rows, _, k in GRID:
        assert applies(metric, dim, rows, 1, k, AUTO) == (rows >= 300_000)


def test_automatic_mode_leaves_narrow_rows_to_the_float32_scan():
    """at 16 dimensions a row of the copy is 32 bytes and 4 queries' lower bounds cost 32 bytes written and read back: nothing to gain
    (and tests/test_gpu_mq64.py asserts k_flat_scan_mq's trace line for this very shape)"""
    for nq in (2, 3, 4, 5, 8):
        for k in (1, 10, 64):
            assert not applies(COSINE, 16, 530_000, nq, k, AUTO)
            assert not applies(DOT, 16, 10_000_000, nq, k, AUTO)


def test_automatic_mode_takes_the_measured_shapes():
    """profiles/LAB_r08_bound_scan_mq.md: from 300 000 x 768 for 2 - 4 queries, from 1M x 768 for 5 - 8, from 10M rows at 128 dimensions"""
    for metric, k in itertools.product((COSINE, DOT), (1, 10, 64)):
        for nq in (2, 3, 4):
            assert applies(metric, 768, 300_000, nq, k, AUTO) and not applies(metric, 768, 299_999, nq, k, AUTO)
        for nq in (5, 6, 7, 8):
            assert applies(metric, 768, 1_000_000, nq, k, AUTO) and not applies(metric, 768, 999_999, nq, k, AUTO)
        for nq in (2, 4, 5, 8):
            assert applies(metric, 128, 10_000_000, nq, k, AUTO) and not applies(metric, 128, 1_000_000, nq, k, AUTO)
            assert applies(metric, 1536, 3_000_000, nq, k, AUTO) and not applies(metric, 112, 10_000_000, nq, k, AUTO)


def test_automatic_mode_is_monotone_in_rows_and_width():
    """whatever the measured floors are: a shape the rule takes stays taken with more rows or wider rows"""
    for metric, nq, k in itertools.product((COSINE, DOT), (2, 4, 5, 8), (1, 10, 64)):
        for dim in (16, 128, 768, 4096):
            took = False
            for rows in (20_011, 300_000, 1_000_000, 3_000_000, 10_000_000):
                now = applies(metric, dim, rows, nq, k, AUTO)
                assert now or not took, (metric, dim, rows, nq, k)
                took = now
        for rows in (300_000, 1_000_000, 10_000_000):
            took = False
            for dim in (16, 128, 768, 4096):
                if nq * ((rows + 63) // 64) * 256 > 2 << 30:
                    continue
                now = applies(metric, dim, rows, nq, k, AUTO)
                assert now or not took, (metric, dim, rows, nq, k)
                took = now


def test_the_lower_bound_planes_stay_under_two_gib():
    assert applies(COSINE, 128, 60_000_000, 8, 10, ALWAYS)                 # 8 x 60M x 4 bytes = 1.9 GB
    assert not applies(COSINE, 128, 70_000_000, 8, 10, ALWAYS)
    assert applies(COSINE, 128, 70_000_000, 4, 10, ALWAYS)


def test_a_mode_out_of_range_is_an_error():
    assert _lib.lib().qv_scan_bound_applies(COSINE, 128, 1_000_000, 4, 10, 3, 1) < 0
