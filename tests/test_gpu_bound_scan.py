"""The single-query bound scan (k_bound_scan + k_bound_rescore, quiver_amd/csrc/qv_bound_scan.hip): stage 1 rejects rows on the index's bfloat16
copy, stage 2 walks the survivors' float32 rows in the exact scan's arithmetic.  The path is forced on by the index's setter (its
automatic threshold is 300 000 rows); every result is compared, rows and float32 bits, with the exact scan of the SAME index (the
setter's "never") and, for a few queries, with the CPU oracle — and the statistics say which path answered: a test here must not pass
on the hand-back alone."""
import os

import numpy as np
import pytest

import quiver_amd
from tests import _bound as B
from tests import _extremes as X
from tests import _oracle as O
from tests._order import planted_rows, query_for

pytestmark = pytest.mark.gpu


def both(idx, q, k):
    """(bound scan result, exact scan result, searches that took the bound scan, of which handed back) for one query"""
    idx.set_bound_scan("always")
    s0 = idx.bound_scan_stats()
    r, d, c = idx.search(q, k)
    s1 = idx.bound_scan_stats()
    idx.set_bound_scan("never")
    er, ed, ec = idx.search(q, k)
    s2 = idx.bound_scan_stats()
    assert s2["searches"] == s1["searches"]                               # "never" is never
    assert np.array_equal(c, ec) and np.array_equal(r, er), (k, r, er)
    assert X.same(d, ed), (k, d, ed)
    return (r, d, c), s1["searches"] - s0["searches"], s1["hand_backs"] - s0["hand_backs"], s1["candidates"]


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("dim", [16, 128, 768, 1536])
def test_rows_and_bits_of_the_exact_scan(metric, dim):
    """k = 1 / 10 / 63 / 64, a ragged last tile (n is no multiple of 64), against the exact scan and the oracle; stage 1's survivor count
    against the CPU model's (tests/_bound.py)"""
    n = 20_011 if dim <= 768 else 9_003
    idx = quiver_amd.DeviceIndex(dim, metric)
    idx.add_synthetic(4100 + dim, 0, n)
    assert idx.bound_scan_stats()["plane"]
    qs = O.gen_rows(4101 + dim, 0, 3, dim)
    corpus = O.gen_rows(4100 + dim, 0, n, dim)
    mid = quiver_amd.metric_id(metric)
    state = B.RowState(corpus)
    stage1 = [B.stage1(mid, state, q) for q in qs]
    for k in (1, 10, 63, 64):
        for i in range(3):
            (r, d, c), took, back, cand = both(idx, qs[i], k)
            assert took == 1 and back == 0, (k, i, took, back)
            assert k <= cand <= 4096
            assert cand == B.decide(stage1[i], k)["count"], (k, i, cand)
            if i == 0:
                er, ed = O.exact_search(mid, corpus, qs[i], k)
                assert np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32))
    idx.close()


def test_iid_unit_corpus_needs_no_hand_back():
    """200 k x 768 unit rows, k = 10: the bound decides, and with the exact k-th upper bound as the threshold k plus a handful survive"""
    n, dim, k = 200_000, 768, 10
    idx = quiver_amd.DeviceIndex(dim, "cosine")
    idx.add_synthetic(20260424, 0, n)
    qs = O.gen_rows(20260425, 0, 4, dim)
    for i in range(4):
        _, took, back, cand = both(idx, qs[i], k)
        assert took == 1 and back == 0
        assert k <= cand <= 4096, cand
        print("200k x 768 k=10 query %d: %d survivors of stage 1" % (i, cand))
    idx.close()


def test_a_width_the_path_declines_and_the_opt_outs():
    rows = O.gen_rows(77, 0, 5000, 100)                                    # 100 is no multiple of 16
    idx = quiver_amd.DeviceIndex(100, "cosine"); idx.add(rows)
    _, took, _, _ = both(idx, rows[3], 10)
    assert took == 0
    idx.close()
    rows = O.gen_rows(78, 0, 5000, 128)
    for make in ("flag", "oom", "metric"):
        if make == "oom":
            os.environ["QV_TEST_PLANE_OOM"] = "1"                          # the copy's allocation answers out-of-memory: not an error, no copy
        try:
            idx = quiver_amd.DeviceIndex(128, "l2" if make == "metric" else "cosine", scan_plane=make != "flag")
            idx.add(rows)
        finally:
            os.environ.pop("QV_TEST_PLANE_OOM", None)
        assert not idx.bound_scan_stats()["plane"]
        (r, d, _), took, _, _ = both(idx, rows[3], 10)
        assert took == 0 and int(r[0, 0]) == 3
        idx.close()


def test_near_duplicate_clusters_wider_than_the_list_hand_back():
    """20 000 near-copies of one vector all lie within the bound's margin of the k-th distance: more candidates than the list holds, so
    the exact scan behind stage 2 answers — decided on the device — and the result is still the exact scan's"""
    rng = np.random.default_rng(3)
    dim, per = 64, 20_000
    centres = rng.standard_normal((3, dim)).astype(np.float32)
    rows = np.concatenate([c + 1e-5 * rng.standard_normal((per, dim)).astype(np.float32) for c in centres])
    for metric in ("cosine", "dot"):
        idx = quiver_amd.DeviceIndex(dim, metric); idx.add(rows)
        _, took, back, cand = both(idx, (centres[1] + 1e-5 * rng.standard_normal(dim)).astype(np.float32), 10)
        assert took == 1 and back == 1 and cand > 4096, (took, back, cand)
        _, took, back, _ = both(idx, rng.standard_normal(dim).astype(np.float32), 10)      # the words are back in their initial state
        assert took == 1
        idx.close()


def test_tombstones_updates_duplicates_and_ties():
    rng = np.random.default_rng(11)
    dim, n = 128, 12_000
    rows = O.gen_rows(500, 0, n, dim)
    rows[64 * 5 + 3] = rows[7]; rows[64 * 100 + 63] = rows[7]; rows[n - 1] = rows[7]          # exact duplicates across tiles
    small = rng.integers(-1, 2, (600, dim)).astype(np.float32)                               # ties: many equal distances
    rows[3000:3600] = small
    idx = quiver_amd.DeviceIndex(dim, "cosine"); idx.add(rows)
    for q in (rows[7], small[5], O.gen_rows(501, 0, 1, dim)[0]):
        for k in (1, 10, 64):
            _, took, back, _ = both(idx, q, k)
            assert took == 1
    # removes and updates after the build: the copy and the residuals follow
    gone = np.unique(np.concatenate([np.arange(0, 2000), [64 * 5 + 3, 7]])).astype(np.uint32)
    idx.remove(gone)
    idx.update(9000, rows[7]); idx.update(4, (rows[7] * np.float32(1.0 + 1e-6)).astype(np.float32))
    alive = np.ones(n, bool); alive[gone] = False; alive[4] = True
    rows2 = rows.copy(); rows2[9000] = rows[7]; rows2[4] = (rows[7] * np.float32(1.0 + 1e-6)).astype(np.float32)
    (r, d, _), took, back, _ = both(idx, rows[7], 10)
    assert took == 1 and back == 0
    er, ed = O.exact_search(0, rows2, rows[7], 10, alive=alive)
    assert np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32))
    # fewer than k live rows
    idx.remove(np.arange(0, n - 5, dtype=np.uint32))
    (r, d, c), took, _, _ = both(idx, rows[7], 10)
    assert int(c[0]) == 5 and took == 1
    idx.close()


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_order_sensitive_rows(metric):
    dim = 128
    rng = np.random.default_rng(21)
    mid = quiver_amd.metric_id(metric)
    q = query_for(mid, dim, rng)
    planted = np.asarray(planted_rows(mid, dim, q, 12, rng), np.float32)
    rows = np.concatenate([O.gen_rows(600, 0, 6000, dim), planted, O.gen_rows(601, 0, 3000, dim)])
    idx = quiver_amd.DeviceIndex(dim, metric); idx.add(rows)
    for k in (1, 10, 64):
        (r, d, _), took, _, _ = both(idx, q, k)
        assert took == 1
        er, ed = O.exact_search(mid, rows, q, k)
        assert np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32))
    idx.close()


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_extreme_rows_and_queries(metric):
    """NaN, +-Inf, huge, tiny and all-zero rows are always candidates (the exact pass decides them); zero, NaN and huge queries are
    handed to the exact scan whole"""
    dim = 128
    rng = np.random.default_rng(31)
    extreme = X.class_rows(rng, dim)
    rows = O.gen_rows(700, 0, 8000, dim)
    for j, (_, _, v) in enumerate(extreme):
        rows[(j * 397) % 8000] = v
    idx = quiver_amd.DeviceIndex(dim, metric); idx.add(rows)
    for k in (1, 10, 64):
        _, took, back, _ = both(idx, O.gen_rows(701, 0, 1, dim)[0], k)
        assert took == 1 and back == 0
    for cls, name, v in extreme:
        _, took, back, _ = both(idx, v, 10)
        assert took == 1
        if cls in "NZ" or name in ("norm2e+18", "norm1e+30"):
            assert back == 1, (cls, name)
    idx.close()


def test_concurrent_callers_on_separate_streams():
    import torch
    n, dim, k, callers, each = 30_000, 128, 10, 4, 6
    idx = quiver_amd.DeviceIndex(dim, "cosine"); idx.add_synthetic(800, 0, n)
    qs = O.gen_rows(801, 0, callers * each, dim)
    idx.set_bound_scan("never")
    er, ed, _ = zip(*[idx.search(q, k) for q in qs])
    idx.set_bound_scan("always")
    dq = torch.from_numpy(qs).cuda()
    out_r = torch.empty((callers * each, k), dtype=torch.int32, device="cuda"); out_d = torch.empty((callers * each, k), dtype=torch.float32, device="cuda")
    streams = [torch.cuda.Stream() for _ in range(callers)]
    torch.cuda.synchronize()
    s0 = idx.bound_scan_stats()
    for j in range(each):
        for c, st in enumerate(streams):
            i = c * each + j
            idx.search_device(dq[i].data_ptr(), 1, k, out_r[i].data_ptr(), out_d[i].data_ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    s1 = idx.bound_scan_stats()
    assert s1["searches"] - s0["searches"] == callers * each and s1["hand_backs"] == s0["hand_backs"]
    assert np.array_equal(out_r.cpu().numpy().view(np.uint32), np.concatenate(er))
    assert np.array_equal(out_d.cpu().numpy().view(np.uint32), np.concatenate(ed).view(np.uint32))
    idx.close()


def test_sharded_index_inherits_the_path():
    n, dim, k = 40_000, 128, 10
    rows = O.gen_rows(900, 0, n, dim)
    one = quiver_amd.DeviceIndex(dim, "cosine"); one.add(rows); one.set_bound_scan("never")
    sh = quiver_amd.ShardedIndex(dim, "cosine", devices=[0, 0], peer_copy=True)
    gids = sh.add(rows)
    sh.set_bound_scan("always")
    s0 = sh.bound_scan_stats()
    assert s0["plane"]
    qs = O.gen_rows(901, 0, 3, dim)
    for q in qs:
        er, ed, _ = one.search(q, k)
        r, d, c = sh.search(q, k)
        assert int(c[0]) == k and np.array_equal(r[0], gids[er[0]]) and np.array_equal(d.view(np.uint32), ed.view(np.uint32))
    s1 = sh.bound_scan_stats()
    assert s1["searches"] - s0["searches"] == 2 * len(qs) and s1["hand_backs"] == s0["hand_backs"]
    sh.close(); one.close()
