"""The 6-bit stage in front of the single-query 8-bit bound scan (k_bound_scan6, k_bound_refine8; quiver_amd/csrc/qv_bound_scan.hip): stage 1
rejects rows on the index's 6-bit plane, its candidates are refined on the 8-bit plane by a gather, and the 8-bit stage's collect and exact
re-score finish; a search the 6-bit stage cannot decide goes on to the bfloat16 stage, then to the exact scan.  Every case forces the bound
scan, the 8-bit plane and the 6-bit stage by the index's setters; every result is compared, rows and float32 bits, with the exact scan of
the SAME index and with the CPU oracle — and the counters say which stage answered, with the candidate counts of the CPU model of both
stages (tests/_bound6.py, tests/_bound8.py): a test here cannot pass on a silent fallback."""
import numpy as np
import pytest

import quiver_amd
from tests import _bound6 as B6
from tests import _bound8 as B8
from tests import _busy
from tests import _extremes as X
from tests import _oracle as O

pytestmark = pytest.mark.gpu

KS = (1, 10, 64)


def make(dim, metric, **kw):
    return quiver_amd.DeviceIndex(dim, "l2", l2_scan_plane=True, **kw) if metric == "l2" else quiver_amd.DeviceIndex(dim, metric, **kw)


def force(idx):
    idx.set_bound_scan("always"); idx.set_bound_plane("8bit"); idx.set_bound_plane6("always")


def both(idx, q, k):
    """one query with the 6-bit stage forced and through the exact scan of the same index -> (result, counters' increments)"""
    force(idx)
    a0, b0, c0 = idx.bound_scan6_stats(), idx.bound_scan8_stats(), idx.bound_scan_stats()
    r, d, c = idx.search(q, k)
    a1, b1, c1 = idx.bound_scan6_stats(), idx.bound_scan8_stats(), idx.bound_scan_stats()
    idx.set_bound_scan("never")
    er, ed, ec = idx.search(q, k)
    assert idx.bound_scan6_stats()["searches"] == a1["searches"]                       # "never" is never
    assert np.array_equal(c, ec) and np.array_equal(r, er), (k, r, er)
    assert X.same(d, ed), (k, d, ed)
    inc = {"took6": a1["searches"] - a0["searches"], "back6": a1["hand_backs"] - a0["hand_backs"], "cand6": a1["candidates"],
           "took8": b1["searches"] - b0["searches"], "back8": b1["hand_backs"] - b0["hand_backs"], "cand8": b1["candidates"],
           "took": c1["searches"] - c0["searches"], "back": c1["hand_backs"] - c0["hand_backs"]}
    return (r, d, c), inc


def answered_by_the_6bit_stage(inc):
    return inc["took6"] == 1 and inc["back6"] == 0 and inc["took8"] == 1 and inc["back8"] == 0 and inc["took"] == 1 and inc["back"] == 0


def model(mid, s6, s8, q, k, alive=None):
    """the two stages on the CPU: the 6-bit candidates, then the 8-bit stage over those rows alone (its H from the candidates)"""
    m6 = B6.reference6(mid, s6, q, k, alive)
    m8 = B8.reference8(mid, s8, q, k, m6["passed"])
    return m6, m8


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
@pytest.mark.parametrize("dim", [64, 128, 768])
@pytest.mark.parametrize("n", [512, 513, 4096 + 37])
def test_rows_and_bits_of_the_exact_scan_and_the_oracle(n, dim, metric):
    """the 8-tile minimum, one row more, a ragged last tile over several workgroups; both stages' counts against the CPU model's"""
    idx = make(dim, metric)
    idx.add_synthetic(6100 + dim, 0, n)
    assert idx.bound_scan6_stats()["plane"] and idx.bound_scan8_stats()["plane"]
    corpus = O.gen_rows(6100 + dim, 0, n, dim)
    qs = O.gen_rows(6101 + dim, 0, 2, dim)
    mid = quiver_amd.metric_id(metric)
    s6, s8 = B6.RowState6(corpus), B8.RowState8(corpus)
    for k in KS:
        for i in range(2):
            (r, d, c), inc = both(idx, qs[i], k)
            m6, m8 = model(mid, s6, s8, qs[i], k)
            print("%s %d x %d k %d: 6-bit candidates %d (model %d), 8-bit survivors %d (model %d)" % (metric, n, dim, k, inc["cand6"], m6["count"], inc["cand8"], m8["count"]))
            assert not m6["hand_back"] and not m8["hand_back"]                         # the inputs are what they are chosen to be
            assert answered_by_the_6bit_stage(inc), (k, i, inc)
            assert inc["cand6"] == m6["count"] and inc["cand8"] == m8["count"], (k, i, inc, m6["count"], m8["count"])
            assert k <= inc["cand8"] <= inc["cand6"] <= n
            er, ed = O.exact_search(mid, corpus, qs[i], k)
            assert int(c[0]) == k and np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32))
    idx.close()


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
def test_the_plane_and_its_residual_are_the_host_twins(metric):
    dim, n = 128, 1000
    rows = O.gen_rows(6200, 0, n, dim).copy()
    rows[5] = 0.0; rows[6, 3] = np.nan; rows[7] *= np.float32(1e-30); rows[8] *= np.float32(1e12)
    idx = make(dim, metric); idx.add(rows)
    s6 = B6.RowState6(rows)
    assert np.array_equal(idx.debug_read("plane6"), s6.plane())
    got = idx.debug_read("rres6")[:n]
    assert np.array_equal(np.isnan(got), np.isnan(s6.res)) and np.array_equal(got[~np.isnan(got)], s6.res[~np.isnan(s6.res)])
    assert np.isnan(got[5]) and np.isnan(got[6]) and np.isnan(got[7]) and not np.isnan(got[8])
    assert np.array_equal(idx.debug_read("rscale8")[:n], s6.scale)
    # an update and a growth refresh it
    new = (O.gen_rows(6201, 0, 1, dim)[0] * np.float32(3.5)).astype(np.float32)
    idx.update(9, new); rows[9] = new
    more = O.gen_rows(6202, 0, 700, dim); idx.add(more)
    s6 = B6.RowState6(np.concatenate([rows, more]))
    assert np.array_equal(idx.debug_read("plane6"), s6.plane())
    idx.close()


def test_removed_duplicated_and_nan_rows():
    dim, n = 128, 4096 + 37
    rows = O.gen_rows(6300, 0, n, dim).copy()
    q = O.gen_rows(6301, 0, 1, dim)[0]
    best = O.exact_search(0, rows, q, 3)[0]
    rows[100:140] = rows[int(best[0])]                                  # 41 copies of the nearest row: ties on the row number, through k = 10
    rows[2000:2003] = rows[int(best[1])]
    rows[777, 5] = np.nan                                               # a row the bound says nothing about: always a candidate
    idx = make(dim, "cosine"); idx.add(rows)
    dead = np.concatenate([np.arange(3, n, 17), [int(best[2]), 101, 4100]]).astype(np.uint32)
    idx.remove(dead)
    alive = np.ones(n, bool); alive[dead] = False
    s6, s8 = B6.RowState6(rows), B8.RowState8(rows)
    for k in KS:
        (r, d, c), inc = both(idx, q, k)
        m6, m8 = model(0, s6, s8, q, k, alive)
        assert answered_by_the_6bit_stage(inc), (k, inc)
        assert inc["cand6"] == m6["count"] and inc["cand8"] == m8["count"], (k, inc, m6["count"], m8["count"])
        assert m6["passed"][777] and m6["unsure"][777]
        er, ed = O.exact_search(0, rows, q, k, alive=alive.astype(np.uint8))
        assert np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32)), k
    idx.close()


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
def test_a_zero_query_and_a_nan_query_are_handed_on_and_exact(metric):
    dim, n, k = 128, 4096 + 37, 10
    idx = make(dim, metric); idx.add_synthetic(6400, 0, n)
    good = O.gen_rows(6401, 0, 1, dim)[0]
    nanq = good.copy(); nanq[7] = np.nan
    for q in (np.zeros(dim, np.float32), nanq):
        _, inc = both(idx, q, k)
        assert inc["took6"] == 1 and inc["back6"] == 1 and inc["took8"] == 1 and inc["back8"] == 1, inc
    _, inc = both(idx, good, k)                                         # the control words are back in their initial state
    assert answered_by_the_6bit_stage(inc), inc
    idx.close()


def test_more_candidates_than_the_list_holds_are_handed_on():
    """300 000 copies of one row at 64 dimensions: every row is a candidate of every stage; the counters show the hand-back, the answer is exact"""
    dim, n, k = 64, 300_000, 10
    one = O.gen_rows(6500, 0, 1, dim)
    rows = np.repeat(one, n, axis=0)
    idx = make(dim, "cosine"); idx.add(rows)
    q = O.gen_rows(6501, 0, 1, dim)[0]
    (r, d, c), inc = both(idx, q, k)
    assert inc["took6"] == 1 and inc["back6"] == 1 and inc["cand6"] == n and n > B6.CAND_CAP6, inc
    assert inc["took8"] == 1 and inc["back8"] == 1 and inc["took"] == 1 and inc["back"] == 1, inc     # ... through the bfloat16 stage to the exact scan
    er, ed = O.exact_search(0, rows, q, k)
    assert np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32))
    idx.close()
    idx = make(dim, "cosine"); idx.add_synthetic(6502, 0, 5000)         # an ordinary index on fresh control words
    _, inc = both(idx, q, k)
    assert answered_by_the_6bit_stage(inc), inc
    idx.close()


@pytest.mark.parametrize("dim,kw", [(80, {}), (4048, {}), (128, {"plane6": False}), (128, {"scan_plane": False})])
def test_no_plane_no_route_and_the_answers_are_what_they_were(dim, kw):
    """a dimension that is no multiple of 64 (4032 is 63 groups: 4048 stands for the wide one), QV_FLAG_NO_PLANE6, QV_FLAG_NO_SCAN_PLANE"""
    n, k = 1500, 10
    idx = quiver_amd.DeviceIndex(dim, "cosine", **kw); idx.add_synthetic(6600 + dim, 0, n)
    assert not idx.bound_scan6_stats()["plane"]
    assert idx.bound_scan8_stats()["plane"] == (kw.get("scan_plane", True))
    with pytest.raises(quiver_amd.QvError):
        idx.debug_read("plane6")
    q = O.gen_rows(6601, 0, 1, dim)[0]
    (r, d, c), inc = both(idx, q, k)
    assert inc["took6"] == 0 and inc["took8"] == (1 if kw.get("scan_plane", True) else 0), inc
    er, ed = O.exact_search(0, O.gen_rows(6600 + dim, 0, n, dim), q, k)
    assert np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32))
    idx.close()


def test_on_a_busy_caller_stream():
    """the device form behind a busy block on the caller's stream (tests/_busy.py's protocol): inputs read and results written in stream order"""
    c = _busy.search_case("bound6-1", "cosine", 4096 + 37, 128, 1, 10, "always", "8bit")
    idx = quiver_amd.DeviceIndex(c.dim, c.metric, filter="off"); idx.add(c.rows())
    force(idx)
    want = c.expect(c.true())
    assert c.first(c.true()) != c.first(c.decoy())                       # a stale read cannot pass

    def once():
        a0 = idx.bound_scan6_stats()
        call = _busy.Call(c.name, lambda ins, outs, s: idx.search_device(ins[0], c.nq, c.k, outs[0], outs[1], s),
                          inputs=[(c.true()[0], c.decoy()[0])], outputs=[((c.nq, c.k), "rows"), ((c.nq, c.k), "dist")])
        _busy.run([[call]])
        c.check(*call.got, want)
        a1 = idx.bound_scan6_stats()
        assert a1["searches"] - a0["searches"] == 2 and a1["hand_backs"] == a0["hand_backs"]     # the warm-up and the call, both answered
        return call.busy
    _busy.returned_busy(once)
    idx.close()
