"""The single-query bound scan's re-score (k_bound_rescore<M, P8>, quiver_amd/csrc/qv_bound_scan.hip): a wave per survivor — the row requested
whole, staged, then walked as the exact scan's one in-order chain — on a fixed grid of workgroups whose lists the last one (a ticket) merges,
and exactly one thread deciding hand-back and restoring the control words.  Same kernel for both stages, all three metrics, masked or not.

The survivor counts are built from near-duplicate clusters, as tests/test_gpu_bound_scan8.py does: m near-copies of the query's direction (all
inside the stage's margin) among rows far away, or copies spread so that the 8-bit stage keeps more than the list holds.  The CPU models
(tests/_bound8.reference8, tests/_bound.reference) PREDICT each count before the GPU is asked, so a shape is what it claims; then rows,
counts and float32 bits are compared with the exact scan of the same index and with the CPU oracle, and the counters say which stage
answered with how many survivors.  After every hand-on an ordinary query must be answered by the 8-bit stage again: the control words,
the ticket and the gate are back at zero."""
import functools

import numpy as np
import pytest

import quiver_amd
from tests import _bound as B
from tests import _bound8 as B8
from tests import _extremes as X
from tests import _oracle as O

pytestmark = pytest.mark.gpu

RESCORE_WAVES = 64 * 4                                         # kBoundRescoreGrid workgroups of four waves


def both(idx, q, k, plane="8bit"):
    idx.set_bound_scan("always"); idx.set_bound_plane(plane)
    a0, b0 = idx.bound_scan8_stats(), idx.bound_scan_stats()
    r, d, c = idx.search(q, k)
    a1, b1 = idx.bound_scan8_stats(), idx.bound_scan_stats()
    idx.set_bound_scan("never")
    er, ed, ec = idx.search(q, k)
    assert idx.bound_scan8_stats()["searches"] == a1["searches"] and idx.bound_scan_stats()["searches"] == b1["searches"]   # "never" is never
    assert np.array_equal(c, ec) and np.array_equal(r, er), (k, r, er)
    assert X.same(d, ed), (k, d, ed)
    inc = {"took8": a1["searches"] - a0["searches"], "back8": a1["hand_backs"] - a0["hand_backs"], "cand8": a1["candidates"],
           "took": b1["searches"] - b0["searches"], "back": b1["hand_backs"] - b0["hand_backs"], "cand": b1["candidates"]}
    return (r, d, c), inc


def new_index(dim, metric, rows):
    idx = quiver_amd.DeviceIndex(dim, "l2", l2_scan_plane=True) if metric == "l2" else quiver_amd.DeviceIndex(dim, metric)
    idx.add(rows)
    assert idx.bound_scan8_stats()["plane"] and idx.bound_scan_stats()["plane"]
    return idx


@functools.lru_cache(maxsize=None)
def cluster(dim, m, far, metric, dmax=1e-4, dup=False, seed=11):
    """m near-copies of a unit vector c at cosine distances spread over [0, dmax] (dup: every copy twice, so equal distances are ordered by
    row) shuffled among `far` random directions; the query is c.  -> rows, q, the 8-bit row state"""
    rng = np.random.default_rng(seed + dim + m)
    c = rng.standard_normal(dim); c /= np.linalg.norm(c)
    mm = (m + 1) // 2 if dup else m
    u = rng.standard_normal((mm, dim)); u -= np.outer(u @ c, c); u /= np.linalg.norm(u, axis=1)[:, None]
    dist = np.linspace(0.0, dmax, mm)
    along = (1.0 - dist) if metric == "dot" else np.ones(mm)
    near = along[:, None] * c[None, :] + np.sqrt(2.0 * dist)[:, None] * u
    if dup:
        near = np.repeat(near, 2, axis=0)[:m]
    other = rng.standard_normal((far, dim)); other /= np.linalg.norm(other, axis=1)[:, None]
    rows = np.concatenate([near, other])[rng.permutation(m + far)].astype(np.float32)
    return rows, c.astype(np.float32), B8.RowState8(rows)


def check_answer(metric, rows, q, k, r, d, c):
    mid = quiver_amd.metric_id(metric)
    er, ed = O.exact_search(mid, rows, q, k)
    assert int(c[0]) == k and np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32)), (r[0], er)


def ordinary_query_is_answered_by_the_8bit_stage(idx, dim, k):
    q = np.random.default_rng(3).standard_normal(dim).astype(np.float32)
    _, inc = both(idx, q, k)
    assert inc["took8"] == 1 and inc["back8"] == 0 and inc["took"] == 1 and inc["back"] == 0, inc


# ---- survivor counts: exactly k, a few tens, more than the re-score has waves, the list's capacity, more than it ------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("m", [10, 37, RESCORE_WAVES + 45, 4096, 4500])
def test_survivor_counts(metric, m):
    dim, k = 64, 10
    rows, q, st8 = cluster(dim, m, 6000, metric)
    mid = quiver_amd.metric_id(metric)
    m8 = B8.reference8(mid, st8, q, k)
    assert m8["count"] == m and m8["hand_back"] == (m > B.CAND_CAP), m8["count"]     # every copy inside the margin, nothing else
    m16 = B.reference(mid, B.RowState(rows), q, k)
    idx = new_index(dim, metric, rows)
    (r, d, c), inc = both(idx, q, k)
    assert inc["took8"] == 1 and inc["cand8"] == m and inc["took"] == 1, inc
    if m <= B.CAND_CAP:
        assert inc["back8"] == 0 and inc["back"] == 0 and inc["cand"] == m, inc       # the 8-bit stage answered
    else:                                                                             # ... or handed on, and the bfloat16 stage says what its model says
        assert inc["back8"] == 1 and inc["back"] == (1 if m16["hand_back"] else 0), (inc, m16["count"])
        if not m16["hand_back"]:
            assert inc["cand"] == m16["count"], (inc, m16["count"])
    check_answer(metric, rows, q, k, r, d, c)
    if m > B.CAND_CAP:
        ordinary_query_is_answered_by_the_8bit_stage(idx, dim, k)
    idx.close()


# ---- widths, metrics, k, ties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [16, 48, 768, 1040, 4096])
def test_widths_and_k_with_duplicated_rows(dim):
    """dim 16: a row is four chunks, most lanes request nothing; 1040: 260 chunks, a second round of requests for four lanes; 4096: four rounds.
    Every near-copy twice: equal distances, ordered by row."""
    far = 3000 if dim <= 768 else 900
    rows, q, st8 = cluster(dim, 70, far, "cosine", dup=True)
    idx = new_index(dim, "cosine", rows)
    for k in (1, 10, 64):
        m8 = B8.reference8(0, st8, q, k)
        assert not m8["hand_back"] and k <= m8["count"] <= 200, m8["count"]
        (r, d, c), inc = both(idx, q, k)
        assert inc["took8"] == 1 and inc["back8"] == 0 and inc["back"] == 0 and inc["cand8"] == m8["count"], (k, inc, m8["count"])
        check_answer("cosine", rows, q, k, r, d, c)
        if k > 1:
            assert np.any(d[0][1:] == d[0][:-1]), "no tie among the results: the shape is not what it claims"
    idx.close()


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
@pytest.mark.parametrize("dim", [64, 768])
def test_metrics(metric, dim):
    rows, q, st8 = cluster(dim, 300, 4000 if dim == 64 else 1500, metric, dup=True)
    mid = quiver_amd.metric_id(metric)
    idx = new_index(dim, metric, rows)
    for k in (1, 10, 64):
        m8 = B8.reference8(mid, st8, q, k)
        assert not m8["hand_back"] and m8["count"] >= k
        (r, d, c), inc = both(idx, q, k)
        assert inc["took8"] == 1 and inc["back8"] == 0 and inc["back"] == 0 and inc["cand8"] == m8["count"], (k, inc, m8["count"])
        check_answer(metric, rows, q, k, r, d, c)
    idx.close()


# ---- the stage cases ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_the_bfloat16_stage_alone(metric):
    dim, k = 64, 10
    rows, q, _ = cluster(dim, RESCORE_WAVES + 45, 6000, metric)
    mid = quiver_amd.metric_id(metric)
    m16 = B.reference(mid, B.RowState(rows), q, k)
    assert not m16["hand_back"] and m16["count"] >= k
    idx = new_index(dim, metric, rows)
    (r, d, c), inc = both(idx, q, k, plane="bf16")
    assert inc["took8"] == 0 and inc["took"] == 1 and inc["back"] == 0 and inc["cand"] == m16["count"], (inc, m16["count"])
    check_answer(metric, rows, q, k, r, d, c)
    idx.close()


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_the_8bit_stage_hands_on_to_a_bfloat16_stage_that_answers(metric):
    """20 000 near-copies at distances spread over [0, 0.035] (tests/test_gpu_bound_scan8.py's cluster): the 8-bit margin keeps more than the
    list holds, the bfloat16 margin does not"""
    dim, k = 64, 10
    rows, q, st8 = cluster(dim, 20_000, 0, metric, dmax=0.035, seed=5)
    mid = quiver_amd.metric_id(metric)
    m8, m16 = B8.reference8(mid, st8, q, k), B.reference(mid, B.RowState(rows), q, k)
    assert m8["hand_back"] and m8["count"] > B.CAND_CAP and not m16["hand_back"], (m8["count"], m16["count"])
    idx = new_index(dim, metric, rows)
    (r, d, c), inc = both(idx, q, k)
    assert inc["took8"] == 1 and inc["back8"] == 1 and inc["cand8"] == m8["count"], inc
    assert inc["took"] == 1 and inc["back"] == 0 and inc["cand"] == m16["count"], (inc, m16["count"])
    check_answer(metric, rows, q, k, r, d, c)
    ordinary_query_is_answered_by_the_8bit_stage(idx, dim, k)
    idx.close()


def test_both_stages_hand_back_to_the_exact_scan():
    """5000 copies so close that neither margin separates them: both lists overflow and the exact scan answers"""
    dim, k = 64, 10
    rows, q, st8 = cluster(dim, 5000, 3000, "cosine", dmax=1e-6)
    m8, m16 = B8.reference8(0, st8, q, k), B.reference(0, B.RowState(rows), q, k)
    assert m8["hand_back"] and m16["hand_back"] and m8["count"] > B.CAND_CAP and m16["count"] > B.CAND_CAP
    idx = new_index(dim, "cosine", rows)
    (r, d, c), inc = both(idx, q, k)
    assert inc["took8"] == 1 and inc["back8"] == 1 and inc["took"] == 1 and inc["back"] == 1, inc
    assert inc["cand8"] == m8["count"] and inc["cand"] == m16["count"], (inc, m8["count"], m16["count"])
    check_answer("cosine", rows, q, k, r, d, c)
    ordinary_query_is_answered_by_the_8bit_stage(idx, dim, k)
    idx.close()
