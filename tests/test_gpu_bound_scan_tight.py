"""Both bound-scan kernels (k_bound_scan, k_bound_scan_mq: quiver_amd/csrc/qv_bound_scan.hip) where the interval of qv_bound.h is TIGHT.

tests/test_gpu_bound_scan.py and tests/test_gpu_bound_scan_mq.py compare rows and bits with the exact scan on corpora where the margin is
tens of times wider than the error it covers: a residual several times too small, one left stale by an update or lost in a growth
copy, would pass them.  Here the corpora are built (tests/_tight.py) so that the margin is needed in full — a planted neighbour r*
whose true sum exceeds stage 1's by the whole Cauchy-Schwarz term, beside competitors exact in bfloat16 — and every case is first
checked on the CPU, with the oracle and the library's own interval function, to flip when r*'s residual is 10 % short.  Then the worst
of bfloat16 rounding in a cluster, rows below filter_tiny_norm as the nearest neighbours, and the extreme rows in shared passes.
Every result is compared, rows, counts and float32 bits, with the same call under "never", and the statistics say the bound scan
answered."""
import numpy as np
import pytest

import quiver_amd
from tests import _bound as B
from tests import _extremes as X
from tests import _oracle as O
from tests import _tight as T

pytestmark = pytest.mark.gpu


def both(idx, qs, k):
    """(result under "always", queries that took the bound scan, of which handed back) for ONE call; the same call under "never" must give
    the same rows, counts and bits"""
    idx.set_bound_scan("always")
    s0 = idx.bound_scan_stats()
    r, d, c = idx.search(qs, k)
    s1 = idx.bound_scan_stats()
    idx.set_bound_scan("never")
    er, ed, ec = idx.search(qs, k)
    assert idx.bound_scan_stats()["searches"] == s1["searches"]          # "never" is never
    assert np.array_equal(c, ec) and np.array_equal(r, er), (k, r, er)
    assert X.same(d, ed), (k, d, ed)
    return (r, d, c), s1["searches"] - s0["searches"], s1["hand_backs"] - s0["hand_backs"]


def planted_forms(idx, case, er, ed, others):
    """the planted query alone, in an odd and in an even slot of a 4-query call, and of an 8-query call (both halves of the packed fma)"""
    q, k, t = case["q"], case["k"], case["target"]
    for nq, slot in ((1, 0), (4, 1), (4, 2), (8, 5), (8, 6)):
        qs = others[:nq].copy(); qs[slot] = q
        (r, d, c), took, back = both(idx, qs, k)
        assert took == nq and back == 0, (nq, slot, took, back)
        assert int(c[slot]) == k and t in r[slot].tolist(), ("r* was rejected", nq, slot, r[slot])
        assert np.array_equal(r[slot], er) and np.array_equal(d[slot].view(np.uint32), ed.view(np.uint32)), (nq, slot)


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("dim", T.PLANTED_DIMS)
@pytest.mark.parametrize("k", T.PLANTED_KS)
def test_planted_neighbour_that_needs_the_whole_margin(metric, dim, k):
    planted_neighbour_that_needs_the_whole_margin(metric, dim, k)


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("dim,k", T.PLANTED_WIDE)
def test_planted_neighbour_that_needs_the_whole_margin_at_wider_rows(metric, dim, k):
    """240 dimensions: every block of the step ladder in one walk; 2048: the widest gamma at which the construction holds (tests/_tight.py)"""
    planted_neighbour_that_needs_the_whole_margin(metric, dim, k)


def planted_neighbour_that_needs_the_whole_margin(metric, dim, k):
    case = T.planted(quiver_amd.metric_id(metric), dim, k)
    er, ed, _ = T.conditions(case)                                        # (a) - (d): the case discriminates
    idx = quiver_amd.DeviceIndex(dim, metric); idx.add(case["rows"])
    planted_forms(idx, case, er, ed, np.random.default_rng(dim + k).standard_normal((8, dim)).astype(np.float32))
    idx.close()


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("edit", ["update", "second_add", "regrow"])
def test_planted_neighbour_after_edits(metric, edit):
    """r* written by an update over an ordinary row; arriving by a second add into a partly filled tile; carried, with everything around
    it, across a growth of the index's arrays: a residual or a copy left stale or lost rejects r*"""
    dim, k = 128, 10
    case = T.planted(quiver_amd.metric_id(metric), dim, k)
    rows, t = case["rows"], case["target"]
    er, ed, _ = T.conditions(case)
    idx = quiver_amd.DeviceIndex(dim, metric)
    if edit == "update":
        first = rows.copy(); first[t] = rows[case["ordinary"]]
        assert B.RowState(first[t:t + 1]).rres[0] < 0.7 * B.RowState(rows[t:t + 1]).rres[0]      # a stale residual would be far too short
        idx.add(first); idx.update(t, rows[t])
    elif edit == "second_add":
        cut = t - 3                                                        # r* lands in the tile the first add left partly filled
        assert cut % 64 != 0 and cut // 64 == t // 64
        idx.reserve(len(rows)); idx.add(rows[:cut]); idx.add(rows[cut:])
    else:
        cut = t + 70                                                       # r* and its tile are whole before the arrays are grown
        assert max(16, -(-cut // 64)) * 64 < len(rows)                     # the first add reserves max(need, 16) tiles: the second add must grow the arrays
        idx.add(rows[:cut]); idx.add(rows[cut:])
    planted_forms(idx, case, er, ed, np.random.default_rng(5).standard_normal((8, dim)).astype(np.float32))
    idx.close()


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("dim", [128, 768])
def test_rows_and_queries_at_the_worst_of_bfloat16_rounding(metric, dim):
    """the bound scan's counterpart of the batched filter's test of that name: a cluster of half-way, exact, scaled and ordinary rows (with
    denormal elements, one whole-denormal row) under queries of each kind; hand-backs only where the CPU reference predicts them"""
    mid = quiver_amd.metric_id(metric)
    rows, qs = T.worst_rounding(dim)
    idx = quiver_amd.DeviceIndex(dim, metric); idx.add(rows)
    for k in (10, 64):
        ref = T.worst_rounding_reference(mid, dim, k)
        assert sum(hb for _, hb in ref) <= 1                               # the cluster is shaped so that the bound decides
        want = {j: O.exact_search(mid, rows, qs[j], k) for j in (1, 3)}    # a half-way query and one scaled by 1e-3
        for sl in [slice(j, j + 1) for j in range(8)] + [slice(0, 4), slice(4, 8), slice(0, 8)]:
            (r, d, c), took, back = both(idx, qs[sl], k)
            assert took == sl.stop - sl.start, (sl, took)
            assert back <= sum(hb for _, hb in ref[sl]), (sl, back, ref[sl])
            for j, (er, ed) in want.items():
                if sl.start <= j < sl.stop:
                    i = j - sl.start
                    assert np.array_equal(r[i], er) and np.array_equal(d[i].view(np.uint32), ed.view(np.uint32)), (sl, j)
    idx.close()


def test_rows_below_the_tiny_norm_are_the_nearest_neighbours():
    """copies of the query scaled by 1e-20, 1e-16 and 3e-14 (|q| = 0.25: all three below filter_tiny_norm = 1e-14) are at cosine distance
    ~0: the bound says nothing about them, so stage 1 must pass them on unseen"""
    dim = 128
    rows = O.gen_rows(6100, 0, 6011, dim).copy()
    q = (O.gen_rows(6101, 0, 1, dim)[0] * np.float32(0.25)).astype(np.float32)
    at = (70, 3001, 6010)
    for i, s in zip(at, (1e-20, 1e-16, 3e-14)):
        rows[i] = (q.astype(np.float64) * s).astype(np.float32)
        assert B.chain_norm(rows[i]) < 1e-14
    idx = quiver_amd.DeviceIndex(dim, "cosine"); idx.add(rows)
    others = O.gen_rows(6102, 0, 8, dim)
    for k in (1, 3, 10):
        er, ed = O.exact_search(0, rows, q, k)
        assert set(er[:min(k, 3)].tolist()) <= set(at)
        for nq, slot in ((1, 0), (3, 1), (8, 4)):
            qs = others[:nq].copy(); qs[slot] = q
            (r, d, c), took, back = both(idx, qs, k)
            assert took == nq and back == 0, (nq, took, back)
            assert np.array_equal(r[slot], er) and np.array_equal(d[slot].view(np.uint32), ed.view(np.uint32)), (k, nq, r[slot], er)
    idx.close()


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_extreme_rows_in_a_shared_pass(metric):
    """NaN, +-Inf, huge, zero and denormal ROWS under calls of 3 and 8 ordinary queries (tests/test_gpu_bound_scan_mq.py puts the extreme
    values in queries only): always candidates, decided by the exact pass, no hand-back"""
    dim = 128
    rng = np.random.default_rng(41)
    rows = O.gen_rows(6200, 0, 8011, dim).copy()
    for j, (_, _, v) in enumerate(X.class_rows(rng, dim)):
        rows[(j * 397 + 5) % 8011] = v
    idx = quiver_amd.DeviceIndex(dim, metric); idx.add(rows)
    qs = O.gen_rows(6201, 0, 8, dim)
    for nq in (3, 8):
        for k in (1, 10, 64):
            _, took, back = both(idx, qs[:nq], k)
            assert took == nq and back == 0, (nq, k, took, back)
    idx.close()
