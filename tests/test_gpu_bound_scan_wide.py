"""The wide form of the single-query, unfiltered bound scan, 65 <= k <= 1024 (k_bound_scan / k_bound_scan8 with the wide tail, the selection of
H, k_bound_collect_wide, k_bound_rescore_wide, the counted selection and the gated key-per-row redo; quiver_amd/csrc/qv_bound_scan.hip).
Every case forces the form by the index's own setter (set_bound_scan_wide("always")) and names the plane that comes first; every result
is compared, rows and float32 bits, with the exact path of the SAME index (set_bound_scan_wide("never")), one cell per metric with the CPU
oracle — and the wide form's own counters say what answered: a test here must not pass on a hand-back alone."""
import threading

import numpy as np
import pytest

import quiver_amd
from quiver_amd import _lib
from tests import _bound as B
from tests import _extremes as X
from tests import _oracle as O

pytestmark = pytest.mark.gpu

CAP = _lib.QV_BOUND_WIDE_CAND_CAP
KS = (65, 128, 129, 500, 1024)
ARMS = ("bf16", "8bit")


def make(metric, dim):
    return quiver_amd.DeviceIndex(dim, metric, l2_scan_plane=(metric == "l2"))


def wide_only(idx, q, k, plane):
    """one search under "always" with `plane` first -> (result, the wide counters' increments)"""
    idx.set_bound_scan_wide("always"); idx.set_bound_plane(plane)
    s0 = idx.bound_scan_wide_stats()
    res = idx.search(q, k)
    s1 = idx.bound_scan_wide_stats()
    return res, {"took": s1["searches"] - s0["searches"], "back": s1["hand_backs"] - s0["hand_backs"], "cand": s1["candidates"]}


def exact_of(idx, q, k):
    idx.set_bound_scan_wide("never")
    s0 = idx.bound_scan_wide_stats()
    res = idx.search(q, k)
    assert idx.bound_scan_wide_stats()["searches"] == s0["searches"]           # "never" is never
    return res


def both(idx, q, k, plane, exact=None):
    """... and the exact path of the same index: rows, float32 bits and counts are the same"""
    (r, d, c), inc = wide_only(idx, q, k, plane)
    er, ed, ec = exact if exact is not None else exact_of(idx, q, k)
    assert np.array_equal(c, ec) and np.array_equal(r, er), (k, plane, r, er)
    assert X.same(d, ed), (k, plane, d, ed)
    return (r, d, c), inc


def answered(inc):
    return inc["took"] == 1 and inc["back"] == 0


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
@pytest.mark.parametrize("n,dim", [(6001, 80), (2000, 16), (200_000, 64)])
def test_rows_and_bits_of_the_exact_path(metric, n, dim):
    """a ragged last tile and a 4 + 1 step split (6 001 x 80); the narrowest row (2 000 x 16); 3 125 tiles, so that waves walk several
    (200 000 x 64).  One cell per metric against the CPU oracle; on the bfloat16 arm the survivor count is at least the CPU model's."""
    idx = make(metric, dim)
    seed = 7100 + dim
    idx.add_synthetic(seed, 0, n)
    assert idx.bound_scan_wide_stats()["plane"] and idx.bound_scan8_stats()["plane"]
    q = O.gen_rows(seed + 1, 0, 1, dim)[0]
    mid = quiver_amd.metric_id(metric)
    corpus = O.gen_rows(seed, 0, n, dim) if n <= 6001 else None
    stage1 = B.stage1(mid, B.RowState(corpus), q) if corpus is not None and metric != "l2" else None
    for k in KS:
        exact = exact_of(idx, q, k)
        assert int(exact[2][0]) == k
        for plane in ARMS:
            _, inc = both(idx, q, k, plane, exact)
            assert answered(inc), (k, plane, inc)
            assert k <= inc["cand"] <= CAP, (k, plane, inc)
            if plane == "bf16" and stage1 is not None:
                assert inc["cand"] >= B.decide(stage1, k)["count"], (k, inc)
    if corpus is not None and n == 6001:
        er, ed = O.exact_search(mid, corpus, q, 129)
        (r, d, c), inc = wide_only(idx, q, 129, "8bit")
        assert answered(inc) and int(c[0]) == 129 and np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32))
    idx.close()


def test_nearest_rows_stored_together():
    """rows 0 .. 1023 are the 1024 nearest: sixteen neighbouring tiles hold the whole answer.  With 3 125 tiles a wave walks two, a stride of
    tiles apart (tile t belongs to wave t mod (4 * grid), 1 564 waves on 256 compute units), so the sixteen tiles belong to sixteen
    DIFFERENT waves, each of which publishes all 64 of its near rows: nothing is dropped, H is the exact k-th smallest upper bound, and the
    survivor count is the CPU model's (tests/_wide.py).  The case in which one wave holds more than it publishes is
    tests/test_gpu_bound_wide_counts.py's."""
    from quiver_amd.device_index import device_info
    from tests import _wide as Wd
    dim, n = 64, 200_000                                                # (3 125 tiles: a wave walks several)
    rng = np.random.default_rng(71)
    q = rng.standard_normal(dim).astype(np.float32)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    rows[:1024] = (q[None, :] + np.float32(0.05) * rows[:1024]).astype(np.float32)
    idx = make("cosine", dim); idx.add(rows)
    n_tiles = (n + 63) // 64
    grid, stride = Wd.plan(n_tiles, device_info(0)["cus"])
    stages = {plane: Wd.stage_of(0, plane, rows, q) for plane in ARMS}
    for k in (1024, 500):
        er, ed = O.exact_search(0, rows, q, k)
        assert set(er.tolist()) <= set(range(1024))
        for plane in ARMS:
            (r, d, c), inc = both(idx, q, k, plane)
            assert answered(inc), inc
            assert np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32)), (k, plane)
            m = Wd.decide_wide(stages[plane], k, np.ones(n, bool), n_tiles, grid)
            print("k %d %s: survivors %d, the model %d" % (k, plane, inc["cand"], m["count"]))
            assert not m["hand_back"] and (stride < 16 or m["dropped"] == 0), (k, plane, m["dropped"])
            assert inc["cand"] == m["count"], (k, plane, inc, m["count"])
    idx.close()


@pytest.mark.parametrize("k", [65, 129])
def test_ties_across_the_kth_place(k):
    """exact duplicates of one row in three different tiles take ranks k - 1, k and k + 1: the two with the smaller row numbers are in the
    answer, in (distance, row) order"""
    dim, n = 80, 6001
    rows = O.gen_rows(7300, 0, n, dim)
    q = O.gen_rows(7301, 0, 1, dim)[0]
    order, _ = O.exact_search(0, rows, q, n)
    src = int(order[k - 2])                                              # rank k - 1 (1-based)
    far = [int(r) for r in order[::-1] if int(r) // 64 != src // 64][:400]
    a = far[0]
    b = next(r for r in far if r // 64 != a // 64)
    rows[a] = rows[src]; rows[b] = rows[src]
    er, ed = O.exact_search(0, rows, q, k)
    trio = sorted([src, a, b])
    assert er[k - 2] == trio[0] and er[k - 1] == trio[1] and trio[2] not in er.tolist()   # the shape is what it is built to be
    idx = make("cosine", dim); idx.add(rows)
    for plane in ARMS:
        (r, d, c), inc = both(idx, q, k, plane)
        assert answered(inc), inc
        assert np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32)), (plane, r[0][-4:], er[-4:])
    idx.close()


def _handed_back(idx, q, k, oracle_rows=None, metric=0):
    for plane in ARMS:
        (r, d, c), inc = both(idx, q, k, plane)
        assert inc["took"] == 1 and inc["back"] == 1, (plane, inc)
        if oracle_rows is not None:
            er, ed = O.exact_search(metric, oracle_rows, q, k)
            assert np.array_equal(r[0], er) and X.same(d[0], ed), plane
    # the control words are back in their initial state: an ordinary query behind it is answered by the wide form
    q2 = O.gen_rows(7499, 0, 1, idx.dim)[0]
    return both(idx, q2, k, "8bit")[1]


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
def test_queries_the_bound_declines_are_handed_back(metric):
    """a zero query and a query of 1e30 elements: bound_scan_norm_ok declines |q|, both stages hand on, the exact path answers"""
    dim, n, k = 80, 6001, 100
    idx = make(metric, dim); idx.add_synthetic(7400, 0, n)
    rows = O.gen_rows(7400, 0, n, dim)
    mid = quiver_amd.metric_id(metric)
    assert answered(_handed_back(idx, np.zeros(dim, np.float32), k, rows, mid))
    assert answered(_handed_back(idx, np.full(dim, 1e30, np.float32), k))
    idx.close()


def test_more_copies_of_the_query_than_the_list_holds():
    dim, k = 16, 100
    rng = np.random.default_rng(75)
    q = rng.standard_normal(dim).astype(np.float32)
    rows = rng.standard_normal((CAP + 3000, dim)).astype(np.float32)
    copies = rng.permutation(len(rows))[:CAP + 500]
    rows[copies] = q
    idx = make("cosine", dim); idx.add(rows)
    inc = _handed_back(idx, q, k, rows)
    assert inc["took"] == 1                                              # (the query behind it: a random one, far from the copies)
    idx.close()


def test_fewer_rows_the_bound_is_sure_of_than_results():
    """70 rows without a NaN element at k = 100: no finite H in either stage"""
    dim, n, k = 16, 2000, 100
    rows = O.gen_rows(7600, 0, n, dim)
    sure = np.random.default_rng(76).permutation(n)[:70]
    bad = np.ones(n, bool); bad[sure] = False
    rows[bad, 3] = np.nan
    q = O.gen_rows(7601, 0, 1, dim)[0]
    idx = make("cosine", dim); idx.add(rows)
    for plane in ARMS:
        (r, d, c), inc = both(idx, q, k, plane)
        assert inc["took"] == 1 and inc["back"] == 1, (plane, inc)
        assert sorted(r[0][:70].tolist()) == sorted(sure.tolist())       # the 70 finite distances first
    idx.close()


def test_rows_with_an_inf_element_always_survive():
    """a few such rows ride along with the answer's candidates; more of them than the list holds hand the search back"""
    dim, k = 16, 100
    rng = np.random.default_rng(77)
    rows = rng.standard_normal((CAP + 2500, dim)).astype(np.float32)
    q = rng.standard_normal(dim).astype(np.float32)
    few = rng.permutation(len(rows))[:40]
    rows[few, 5] = np.inf
    idx = make("dot", dim); idx.add(rows)
    for plane in ARMS:
        _, inc = both(idx, q, k, plane)
        assert answered(inc) and inc["cand"] >= k + 40, (plane, inc)
    idx.close()
    many = rng.permutation(len(rows))[:CAP + 200]
    rows[many, 5] = np.inf
    idx = make("dot", dim); idx.add(rows)
    for plane in ARMS:
        _, inc = both(idx, q, k, plane)
        assert inc["took"] == 1 and inc["back"] == 1, (plane, inc)
    idx.close()


def test_tombstones_and_scattered_updates():
    dim, n = 80, 12_001
    rows = O.gen_rows(7800, 0, n, dim)
    q = O.gen_rows(7801, 0, 1, dim)[0]
    idx = make("cosine", dim); idx.add(rows)
    top, _ = O.exact_search(0, rows, q, 300)
    rng = np.random.default_rng(78)
    gone = np.unique(np.concatenate([top[::3], rng.permutation(n)[:2000]]))[:2000].astype(np.uint32)
    idx.remove(gone)
    alive = np.ones(n, bool); alive[gone] = False
    upd = rng.permutation(np.flatnonzero(alive))[:300].astype(np.uint32)
    vecs = O.gen_rows(7802, 0, 300, dim)
    vecs[:20] = (q[None, :] + np.float32(0.1) * vecs[:20]).astype(np.float32)   # some of the new rows belong in the answer
    idx.update_rows(upd, vecs)
    rows2 = rows.copy(); rows2[upd] = vecs
    for k in (65, 300, 1024):
        er, ed = O.exact_search(0, rows2, q, k, alive=alive)
        for plane in ARMS:
            (r, d, c), inc = both(idx, q, k, plane)
            assert answered(inc), (k, plane, inc)
            assert np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32)), (k, plane)
    idx.close()


def test_k_above_the_live_rows_keeps_its_path():
    dim, n = 16, 2000
    idx = make("cosine", dim); idx.add_synthetic(7900, 0, n)
    idx.remove(np.arange(0, 1100, dtype=np.uint32))
    q = O.gen_rows(7901, 0, 1, dim)[0]
    (r, d, c), inc = both(idx, q, 1000, "8bit")
    assert int(c[0]) == 900 and inc["took"] == 0 and inc["back"] == 0, inc
    (r, d, c), inc = both(idx, q, 900, "8bit")                          # every live row: nothing to reject
    assert int(c[0]) == 900 and inc["took"] == 0, inc
    (r, d, c), inc = both(idx, q, 899, "8bit")
    assert int(c[0]) == 899 and answered(inc), inc
    idx.close()


def test_device_pointers_on_a_busy_stream_reuse_the_workspace():
    """k = 1024, then 65, then 300 on one non-default stream without a synchronise between them: one workspace, one set of control words"""
    import torch
    dim, n = 64, 50_000
    idx = make("cosine", dim); idx.add_synthetic(8000, 0, n)
    q = O.gen_rows(8001, 0, 1, dim)[0]
    ks = (1024, 65, 300)
    exact = {k: exact_of(idx, q, k) for k in ks}
    dq = torch.from_numpy(q).cuda()
    st = torch.cuda.Stream()
    for plane in ARMS:
        idx.set_bound_scan_wide("always"); idx.set_bound_plane(plane)
        s0 = idx.bound_scan_wide_stats()
        outs = {k: (torch.zeros(k, dtype=torch.int32, device="cuda"), torch.zeros(k, dtype=torch.float32, device="cuda")) for k in ks}
        torch.cuda.synchronize()
        for k in ks:
            idx.search_device(dq.data_ptr(), 1, k, outs[k][0].data_ptr(), outs[k][1].data_ptr(), st.cuda_stream)
        st.synchronize()
        s1 = idx.bound_scan_wide_stats()
        assert s1["searches"] - s0["searches"] == 3 and s1["hand_backs"] == s0["hand_backs"], (plane, s0, s1)
        for k in ks:
            r = outs[k][0].cpu().numpy().view(np.uint32); d = outs[k][1].cpu().numpy()
            assert np.array_equal(r, exact[k][0][0]) and np.array_equal(d.view(np.uint32), exact[k][1][0].view(np.uint32)), (plane, k)
    idx.close()


def test_four_threads_search_one_index():
    dim, n, k = 80, 20_000, 100
    idx = make("cosine", dim); idx.add_synthetic(8100, 0, n)
    qs = O.gen_rows(8101, 0, 4, dim)
    exact = [exact_of(idx, qs[i], k) for i in range(4)]
    idx.set_bound_scan_wide("always"); idx.set_bound_plane("8bit")
    got, errs = [None] * 4, []

    def work(i):
        try:
            for _ in range(3):
                got[i] = idx.search(qs[i], k)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    for i in range(4):
        assert np.array_equal(got[i][0], exact[i][0]) and X.same(got[i][1], exact[i][1]) and np.array_equal(got[i][2], exact[i][2]), i
    idx.close()


def test_search_negative_fetches_through_the_wide_form():
    dim, n, k_fetch = 80, 6001, 100
    idx = make("cosine", dim); idx.add_synthetic(8200, 0, n)
    q, neg = O.gen_rows(8201, 0, 2, dim)
    idx.set_bound_scan_wide("never")
    want = idx.search_negative(q, neg, k_fetch)
    for plane in ARMS:
        idx.set_bound_scan_wide("always"); idx.set_bound_plane(plane)
        s0 = idx.bound_scan_wide_stats()
        got = idx.search_negative(q, neg, k_fetch)
        s1 = idx.bound_scan_wide_stats()
        assert s1["searches"] - s0["searches"] == 1 and s1["hand_backs"] == s0["hand_backs"], (plane, s0, s1)
        assert np.array_equal(got[0], want[0]) and X.same(got[1], want[1]) and X.same(got[2], want[2]) and int(got[3]) == int(want[3]) == k_fetch
    idx.close()


def test_nothing_set_takes_nothing_and_the_other_counters_stay():
    dim, n, k = 80, 6001, 100
    idx = make("cosine", dim); idx.add_synthetic(8300, 0, n)
    q = O.gen_rows(8301, 0, 1, dim)[0]
    idx.search(q, k)
    assert idx.bound_scan_wide_stats()["searches"] == 0                  # automatic: no measured cell, so nothing
    before = (idx.bound_scan_stats(), idx.bound_scan8_stats(), idx.bound_scan6_stats())
    for plane in ARMS:
        _, inc = both(idx, q, k, plane)
        assert answered(inc)
    assert (idx.bound_scan_stats(), idx.bound_scan8_stats(), idx.bound_scan6_stats()) == before
    # the k <= 64 form's knob does not reach the wide form, nor the wide form's the k <= 64 form
    idx.set_bound_scan_wide("never"); idx.set_bound_scan("always")
    s0 = idx.bound_scan_wide_stats()
    idx.search(q, k)
    assert idx.bound_scan_wide_stats() == s0
    idx.set_bound_scan("auto")
    idx.close()


def test_declined_calls_keep_their_paths():
    dim, n, k = 80, 6001, 100
    idx = make("cosine", dim); idx.add_synthetic(8400, 0, n)
    qs = O.gen_rows(8401, 0, 2, dim)
    idx.set_bound_scan_wide("always"); idx.set_bound_plane("8bit")
    s0 = idx.bound_scan_wide_stats()
    mask = np.ones(n, bool); mask[::7] = False
    idx.search_masked(qs[0], k, mask)
    rs = quiver_amd.device_index.RowSet(idx, mask)
    idx.search_rowsets(qs[0], k, rs)
    idx.search(qs, k)                                                    # two queries
    r, d, c = idx.search(qs[0], 1025)
    assert idx.bound_scan_wide_stats() == s0
    idx.set_bound_scan_wide("never")
    er, ed, ec = idx.search(qs[0], 1025)
    assert np.array_equal(r, er) and X.same(d, ed) and int(c[0]) == 1025
    idx.close()
