"""Every form of the bound scan (k_bound_scan, its skipping form, k_bound_scan8, k_bound_scan_mq and its row-set form: quiver_amd/csrc/qv_bound_scan.hip)
at widths whose step counts reach every block of the kernels' width ladders, alone and in company, up to the limit of 4096 dimensions
(tests/_widths.py has the table).  Results go through the exact re-score, so rows and bits alone show a wrong stage 1 only if it happens to
reject a true neighbour; here the device's survivor COUNT must also equal the CPU model's (tests/_bound.py, tests/_bound8.py) for the very
inputs — and tests/test_bound_widths_cpu.py proves that leaving any one ladder block out of the sum changes a count compared here.
Every call runs under "always" and again under "never" on the same index and must give the same rows, counts and float32 bits, which must
be the CPU oracle's; the statistics say that the bound scan answered and handed nothing back."""
import numpy as np
import pytest

import quiver_amd
from tests import _bound as B
from tests import _extremes as X
from tests import _oracle as O
from tests import _widths as W

pytestmark = pytest.mark.gpu

NAME = {B.COSINE: "cosine", B.DOT: "dot"}
widths = pytest.mark.parametrize("dim", W.WIDTHS)
metrics = pytest.mark.parametrize("metric", [B.COSINE, B.DOT])


def both(idx, call, plane="bf16"):
    """(result under "always", the counters' increments and the last survivor counts) for ONE call; the same call under "never" must give the
    same rows, counts and bits and count nothing"""
    idx.set_bound_scan("always"); idx.set_bound_plane(plane)
    a0, b0 = idx.bound_scan8_stats(), idx.bound_scan_stats()
    r, d, c = call()
    a1, b1 = idx.bound_scan8_stats(), idx.bound_scan_stats()
    idx.set_bound_scan("never")
    er, ed, ec = call()
    assert idx.bound_scan8_stats()["searches"] == a1["searches"] and idx.bound_scan_stats()["searches"] == b1["searches"]   # "never" is never
    assert np.array_equal(c, ec) and np.array_equal(r, er), (r, er)
    assert X.same(d, ed), (d, ed)
    return (r, d, c), {"took": b1["searches"] - b0["searches"], "back": b1["hand_backs"] - b0["hand_backs"], "cand": b1["candidates"],
                       "took8": a1["searches"] - a0["searches"], "back8": a1["hand_backs"] - a0["hand_backs"], "cand8": a1["candidates"]}


def is_answer(want, k, r, d, c):
    """rows, float32 bits, count and padding of one query's result against the oracle's (rows, distances)"""
    er, ed = want
    w = len(er)
    return int(c) == w and r[:w].tolist() == er.tolist() and d[:w].tobytes() == ed.tobytes() and (r[w:] == 0xFFFFFFFF).all() and np.isposinf(d[w:]).all() and len(r) == k


def index(metric, dim):
    c = W.case(dim)
    idx = quiver_amd.DeviceIndex(dim, NAME[metric])
    idx.add_synthetic(c["seed"], 0, W.N)
    idx.remove(c["dead"])
    assert idx.bound_scan_stats()["plane"] and idx.bound_scan8_stats()["plane"]
    return idx, c


@metrics
@widths
def test_single_query_on_the_bfloat16_plane(metric, dim):
    idx, c = index(metric, dim)
    for j in W.SINGLE:
        for k in W.KS:
            (r, d, n), inc = both(idx, lambda: idx.search(c["qs"][j], k))
            want = W.model(metric, dim, j, k, c["live"])["count"]
            print("dim %d metric %d query %d k %d: %d survivors, the model %d" % (dim, metric, j, k, inc["cand"], want))
            assert inc["took"] == 1 and inc["back"] == 0 and inc["took8"] == 0, (j, k, inc)
            assert inc["cand"] == want, (j, k, inc, want)
            assert is_answer(W.oracle(metric, dim, j, k, "live"), k, r[0], d[0], n[0]), (j, k)
    idx.close()


@metrics
@widths
def test_single_query_under_search_masked(metric, dim):
    """the skipping form: every third tile holds no candidate"""
    idx, c = index(metric, dim)
    for j in W.SINGLE:
        for k in W.KS:
            (r, d, n), inc = both(idx, lambda: idx.search_masked(c["qs"][j:j + 1], k, c["mask"]))
            want = W.model(metric, dim, j, k, c["live"] & c["mask"])["count"]
            print("dim %d metric %d query %d k %d: %d survivors, the model %d" % (dim, metric, j, k, inc["cand"], want))
            assert inc["took"] == 1 and inc["back"] == 0 and inc["took8"] == 0, (j, k, inc)
            assert inc["cand"] == want, (j, k, inc, want)
            assert is_answer(W.oracle(metric, dim, j, k, "mask"), k, r[0], d[0], n[0]), (j, k)
    idx.close()


@metrics
@widths
def test_single_query_on_the_8bit_plane(metric, dim):
    idx, c = index(metric, dim)
    for j in W.SINGLE:
        for k in W.KS:
            (r, d, n), inc = both(idx, lambda: idx.search(c["qs"][j], k), plane="8bit")
            want = W.model8(metric, dim, j, k, c["live"])["count"]
            print("dim %d metric %d query %d k %d: %d survivors, the model %d" % (dim, metric, j, k, inc["cand8"], want))
            assert inc["took8"] == 1 and inc["back8"] == 0 and inc["took"] == 1 and inc["back"] == 0, (j, k, inc)
            assert inc["cand8"] == want and inc["cand"] == inc["cand8"], (j, k, inc, want)
            assert is_answer(W.oracle(metric, dim, j, k, "live"), k, r[0], d[0], n[0]), (j, k)
    idx.close()


@metrics
@widths
def test_shared_pass(metric, dim):
    """QB = 4 and 8, each part-filled and full; the statistics hold the largest survivor count among the pass's queries"""
    idx, c = index(metric, dim)
    for nq in W.NQS:
        for k in W.KS:
            (r, d, n), inc = both(idx, lambda: idx.search(c["qs"][:nq], k))
            want = max(W.model(metric, dim, j, k, c["live"])["count"] for j in range(nq))
            print("dim %d metric %d nq %d k %d: %d survivors at the most, the model %d" % (dim, metric, nq, k, inc["cand"], want))
            assert inc["took"] == nq and inc["back"] == 0 and inc["took8"] == 0, (nq, k, inc)
            assert inc["cand"] == want, (nq, k, inc, want)
            for j in range(nq):
                assert is_answer(W.oracle(metric, dim, j, k, "live"), k, r[j], d[j], n[j]), (nq, k, j)
    idx.close()


@metrics
@widths
def test_a_row_set_per_query(metric, dim):
    idx, c = index(metric, dim)
    sets = [None if m is None else idx.rowset(m) for m in c["masks"]]
    for nq in W.SET_NQS:
        for k in W.KS:
            (r, d, n), inc = both(idx, lambda: idx.search_rowsets(c["qs"][:nq], k, sets[:nq]))
            want = max(W.model(metric, dim, j, k, W.alive_of(c["live"], c["masks"][j]))["count"] for j in range(nq))
            print("dim %d metric %d nq %d k %d: %d survivors at the most, the model %d" % (dim, metric, nq, k, inc["cand"], want))
            assert inc["took"] == nq and inc["back"] == 0 and inc["took8"] == 0, (nq, k, inc)
            assert inc["cand"] == want, (nq, k, inc, want)
            for j in range(nq):
                assert is_answer(W.oracle(metric, dim, j, k, "set"), k, r[j], d[j], n[j]), (nq, k, j)
    idx.close()


@metrics
def test_saturated_operands_of_the_8bit_stage_at_4096_dimensions(metric):
    """every product of k_bound_scan8's first partial sum at +-127 * +-127 over the whole row: 2048 * 127 * 127 in the int32, more than int32
    holds once the two terms are combined (tests/_widths.saturated); the planted rows are the nearest and the farthest"""
    c = W.saturated()
    idx = quiver_amd.DeviceIndex(W.SAT_DIM, NAME[metric]); idx.add(c["rows"]); idx.remove(c["dead"])
    for k in W.KS:
        want = O.exact_search(metric, c["rows"], c["q"], k, alive=c["live"].astype(np.uint8))
        (r, d, n), inc = both(idx, lambda: idx.search(c["q"], k), plane="8bit")
        m8 = B.decide(W.saturated_stage8(metric), k, alive=c["live"])
        assert inc["took8"] == 1 and inc["back8"] == 0 and inc["took"] == 1 and inc["back"] == 0, (k, inc)
        assert inc["cand8"] == m8["count"] and inc["cand"] == inc["cand8"], (k, inc, m8["count"])
        assert is_answer(want, k, r[0], d[0], n[0]) and int(r[0, 0]) == W.SAT_PLUS[0], k
        (r, d, n), inc = both(idx, lambda: idx.search(c["q"], k))          # and the bfloat16 stage on the same rows
        m16 = B.decide(W.saturated_stage1(metric), k, alive=c["live"])
        assert inc["took"] == 1 and inc["back"] == 0 and inc["took8"] == 0 and inc["cand"] == m16["count"], (k, inc, m16["count"])
        assert is_answer(want, k, r[0], d[0], n[0]), k
    idx.close()


@metrics
def test_the_first_width_above_the_limit_is_declined(metric):
    dim, n, k = 4112, 700, 10                                             # a multiple of 16, eleven tiles: only the width declines
    rows = O.gen_rows(7950, 0, n, dim)
    qs = O.gen_rows(7951, 0, 4, dim)
    idx = quiver_amd.DeviceIndex(dim, NAME[metric]); idx.add(rows)
    assert not idx.bound_scan8_stats()["plane"]
    for call, nq in ((lambda: idx.search(qs[0], k), 1), (lambda: idx.search(qs, k), 4)):
        (r, d, n_out), inc = both(idx, call, plane="8bit")
        assert inc["took"] == 0 and inc["took8"] == 0 and inc["back"] == 0 and inc["back8"] == 0, inc
        for j in range(nq):
            assert is_answer(O.exact_search(metric, rows, qs[j], k), k, r[j], d[j], n_out[j]), j
    idx.close()
