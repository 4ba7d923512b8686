"""The bound scan as a shared pass (k_bound_scan_mq + k_bound_collect_mq + k_bound_rescore_mq, quiver_amd/csrc/qv_bound_scan.hip): 2 to 8 queries
read the index's bfloat16 copy once, 4 or 8 per pass; interval, threshold, collect and exact re-score are per query.  The path is forced on
by the index's setter; every call is compared, rows, counts and float32 bits, with the same call under "never" (k_flat_scan_mq on the
float32 tiles), one query per case with the CPU oracle — and the statistics say which path answered: `searches` must rise by exactly the
number of queries, so that no test here passes on the hand-back alone."""
import numpy as np
import pytest

import quiver_amd
from quiver_amd.device_index import device_info
from tests import _bound as B
from tests import _callers
from tests import _extremes as X
from tests import _oracle as O
from tests import _widths as W
from tests._order import planted_rows, query_for

pytestmark = pytest.mark.gpu


def both(idx, qs, k):
    """(result under "always", queries that took the bound scan, of which handed back, largest survivor count) for ONE call of len(qs) queries;
    the same call under "never" must give the same rows, counts and bits"""
    idx.set_bound_scan("always")
    s0 = idx.bound_scan_stats()
    r, d, c = idx.search(qs, k)
    s1 = idx.bound_scan_stats()
    idx.set_bound_scan("never")
    er, ed, ec = idx.search(qs, k)
    s2 = idx.bound_scan_stats()
    assert s2["searches"] == s1["searches"]                               # "never" is never
    assert np.array_equal(c, ec) and np.array_equal(r, er), (k, r, er)
    assert X.same(d, ed), (k, d, ed)
    return (r, d, c), s1["searches"] - s0["searches"], s1["hand_backs"] - s0["hand_backs"], s1["candidates"]


def oracle_agrees(mid, corpus, q, k, r, d, alive=None):
    er, ed = O.exact_search(mid, corpus, q, k) if alive is None else O.exact_search(mid, corpus, q, k, alive=alive)
    return np.array_equal(r[:len(er)], er) and np.array_equal(d[:len(er)].view(np.uint32), ed.view(np.uint32))


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("dim", [16, 48, 128, 768])
def test_rows_and_bits_of_the_exact_scan(metric, dim):
    """1, 3, 8 and 48 steps of 16 dimensions (every tail of the step walk: 1, 2 + 1, 8, 8 x 6), a ragged last tile, both QB with empty
    slots and across the 4 / 8 edge, k = 1 / 10 / 63 / 64; the pass's largest survivor count against the CPU model's (tests/_bound.py)"""
    n = 20_011
    idx = quiver_amd.DeviceIndex(dim, metric)
    idx.add_synthetic(5100 + dim, 0, n)
    assert idx.bound_scan_stats()["plane"]
    qs = O.gen_rows(5101 + dim, 0, 8, dim)
    corpus = O.gen_rows(5100 + dim, 0, n, dim)
    mid = quiver_amd.metric_id(metric)
    state = B.RowState(corpus)
    sums = W.chain32_queries(qs, state.rh)                                # tests/_bound.chain32_rows, the eight queries at once
    model = {}
    for j in range(8):
        qn = B.chain_norm(qs[j])
        unsure, lo, hi = B.intervals(mid, dim, sums[j], qn, state.rn, state.rres)
        for k in (1, 10, 63, 64):
            model[j, k] = B.decide({"lo": lo, "hi": hi, "unsure": unsure, "qn": qn, "dim": dim}, k)["count"]
    for case, nq in enumerate((2, 3, 4, 5, 7, 8)):
        for k in (1, 10, 63, 64):
            (r, d, c), took, back, cand = both(idx, qs[:nq], k)
            assert took == nq and back == 0, (nq, k, took, back)
            assert k <= cand <= 4096, (nq, k, cand)
            assert cand == max(model[j, k] for j in range(nq)), (nq, k, cand)
            if k == (1, 10, 63, 64)[case % 4]:
                j = nq - 1                                                # the last filled slot of the group
                assert oracle_agrees(mid, corpus, qs[j], k, r[j], d[j]), (nq, k)
    idx.close()


def test_every_wave_walks_two_tiles():
    """The first tile of a wave is sorted outright, every later one inserted.  The launch has 2 workgroups of 4 waves per compute unit at
    the most and evens the shares out, so 2 x 8 x CUs tiles give every wave exactly two (262 144 rows on 256 compute units)."""
    dim, k = 128, 10
    cus = device_info(0)["cus"]
    n = 2 * 8 * cus * 64 - 37                                             # ragged: the last tile is not full
    idx = quiver_amd.DeviceIndex(dim, "cosine")
    idx.add_synthetic(5200, 0, n)
    qs = O.gen_rows(5201, 0, 8, dim)
    for nq in (4, 8):
        (r, d, c), took, back, cand = both(idx, qs[:nq], k)
        assert took == nq and back == 0
        assert k <= cand <= 4096, cand
    corpus = O.gen_rows(5200, 0, n, dim)
    assert oracle_agrees(0, corpus, qs[5], k, r[5], d[5])
    idx.close()


def test_one_query_of_four_is_handed_back_alone():
    """20 000 near-copies of one vector lie within the bound's margin of the k-th distance of a query on their centre: that query's list
    overflows and the exact scan answers it, on the device; the three random queries of the same pass keep the bound scan's answers.
    (The clusters of the single-query test, beside 20 000 independent rows of the same scale: among clusters alone EVERY query has
    20 000 rows within the margin of its nearest centre, and nothing would be left to tell one query's hand-back from the pass's.)"""
    rng = np.random.default_rng(3)
    dim, per = 64, 20_000
    centres = rng.standard_normal((3, dim)).astype(np.float32)
    rows = np.concatenate([c + 1e-5 * rng.standard_normal((per, dim)).astype(np.float32) for c in centres] + [rng.standard_normal((per, dim)).astype(np.float32)])
    for metric in ("cosine", "dot"):
        idx = quiver_amd.DeviceIndex(dim, metric); idx.add(rows)
        qs = rng.standard_normal((4, dim)).astype(np.float32)
        qs[1] = (centres[1] + 1e-5 * rng.standard_normal(dim)).astype(np.float32)
        _, took, back, cand = both(idx, qs, 10)
        assert took == 4 and back == 1 and cand > 4096, (took, back, cand)
        _, took, back, _ = both(idx, rng.standard_normal((4, dim)).astype(np.float32), 10)   # the words are back in their initial state
        assert took == 4 and back == 0, (took, back)
        idx.close()


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_zero_nan_and_huge_queries_are_handed_back_their_neighbours_are_not(metric):
    dim = 128
    rng = np.random.default_rng(31)
    by_name = {(cls, name): v for cls, name, v in X.class_rows(rng, dim)}
    zero = next(v for (cls, _), v in by_name.items() if cls == "Z")
    nan = next(v for (cls, _), v in by_name.items() if cls == "N")
    huge = next(v for (_, name), v in by_name.items() if name == "norm1e+30")
    idx = quiver_amd.DeviceIndex(dim, metric); idx.add(O.gen_rows(5300, 0, 8000, dim))
    ordinary = O.gen_rows(5301, 0, 5, dim)
    qs = np.stack([ordinary[0], zero, ordinary[1], nan, ordinary[2], huge, ordinary[3]])
    _, took, back, _ = both(idx, qs, 10)
    assert took == 7 and back == 3, (took, back)
    _, took, back, _ = both(idx, ordinary, 10)
    assert took == 5 and back == 0, (took, back)
    idx.close()


def test_tombstones_updates_duplicates_and_ties():
    rng = np.random.default_rng(11)
    dim, n = 128, 12_000
    rows = O.gen_rows(500, 0, n, dim)
    rows[64 * 5 + 3] = rows[7]; rows[64 * 100 + 63] = rows[7]; rows[n - 1] = rows[7]          # exact duplicates across tiles
    small = rng.integers(-1, 2, (600, dim)).astype(np.float32)                               # ties: many equal distances
    rows[3000:3600] = small
    idx = quiver_amd.DeviceIndex(dim, "cosine"); idx.add(rows)
    qs = np.stack([rows[7], small[5], O.gen_rows(501, 0, 1, dim)[0], small[77], rows[64 * 100 + 63]])
    for k in (1, 10, 64):
        _, took, _, _ = both(idx, qs, k)
        assert took == 5
    # removes and updates after the build: the copy and the residuals follow
    gone = np.unique(np.concatenate([np.arange(0, 2000), [64 * 5 + 3, 7]])).astype(np.uint32)
    idx.remove(gone)
    idx.update(9000, rows[7]); idx.update(4, (rows[7] * np.float32(1.0 + 1e-6)).astype(np.float32))
    alive = np.ones(n, bool); alive[gone] = False; alive[4] = True
    rows2 = rows.copy(); rows2[9000] = rows[7]; rows2[4] = (rows[7] * np.float32(1.0 + 1e-6)).astype(np.float32)
    (r, d, _), took, back, _ = both(idx, qs, 10)
    assert took == 5
    assert oracle_agrees(0, rows2, qs[0], 10, r[0], d[0], alive=alive)
    # fewer than k live rows
    idx.remove(np.arange(0, n - 5, dtype=np.uint32))
    (r, d, c), took, _, _ = both(idx, qs, 10)
    assert c.tolist() == [5] * 5 and took == 5
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
    qs = np.concatenate([O.gen_rows(602, 0, 3, dim), q[None, :], O.gen_rows(603, 0, 4, dim)])
    for k in (1, 10, 64):
        (r, d, _), took, _, _ = both(idx, qs, k)
        assert took == 8
        assert oracle_agrees(mid, rows, q, k, r[3], d[3])
    idx.close()


def test_coalesced_callers_share_bound_passes():
    """8 native threads, one query per call on one handle: the calls that arrive together are put into one pass, and that pass is the
    bound scan's — every query counted, every caller served the exact scan's bits"""
    n, dim, k = 60_000, 128, 10
    idx = quiver_amd.DeviceIndex(dim, "cosine"); idx.add_synthetic(5400, 0, n)
    qs = O.gen_rows(5401, 0, 32, dim)
    idx.set_bound_scan("never")
    er, ed, ec = idx.search(qs, k)
    idx.set_bound_scan("always")
    s0 = idx.bound_scan_stats(); c0 = _callers.coalesce_stats("index", idx.handle)
    res = _callers.run("index", idx.handle, qs, k, threads=8, seconds=30.0, max_calls_per_thread=24)
    assert res["rc"] == 0, res["error"]
    assert res["errors"] == 0 and res["mismatches"] == 0 and res["calls"] == 8 * 24
    s1 = idx.bound_scan_stats(); c1 = _callers.coalesce_stats("index", idx.handle)
    assert c1["rode"] > c0["rode"] and c1["group_queries"] - c0["group_queries"] > c1["groups"] - c0["groups"] > 0   # passes were shared
    assert s1["searches"] - s0["searches"] == res["calls"], (s0, s1)
    assert s1["hand_backs"] == s0["hand_backs"]
    seen = res["count"] != 0xFFFFFFFD
    assert seen.any()
    assert np.array_equal(res["rows"][seen], er[seen]) and np.array_equal(res["dist"][seen].view(np.uint32), ed[seen].view(np.uint32))
    idx.close()


def test_device_pointer_calls_of_four_on_separate_streams():
    import torch
    n, dim, k, callers, each, nq = 30_000, 128, 10, 4, 5, 4
    idx = quiver_amd.DeviceIndex(dim, "cosine"); idx.add_synthetic(5500, 0, n)
    total = callers * each * nq
    qs = O.gen_rows(5501, 0, total, dim)
    idx.set_bound_scan("never")
    er, ed, _ = zip(*[idx.search(qs[i:i + nq], k) for i in range(0, total, nq)])
    idx.set_bound_scan("always")
    dq = torch.from_numpy(qs).cuda()
    out_r = torch.empty((total, k), dtype=torch.int32, device="cuda"); out_d = torch.empty((total, k), dtype=torch.float32, device="cuda")
    streams = [torch.cuda.Stream() for _ in range(callers)]
    torch.cuda.synchronize()
    s0 = idx.bound_scan_stats()
    for j in range(each):
        for c, st in enumerate(streams):
            i = (c * each + j) * nq
            idx.search_device(dq[i].data_ptr(), nq, k, out_r[i].data_ptr(), out_d[i].data_ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    s1 = idx.bound_scan_stats()
    assert s1["searches"] - s0["searches"] == total and s1["hand_backs"] == s0["hand_backs"]
    assert np.array_equal(out_r.cpu().numpy().view(np.uint32), np.concatenate(er))
    assert np.array_equal(out_d.cpu().numpy().view(np.uint32), np.concatenate(ed).view(np.uint32))
    idx.close()


def test_declined_shapes_take_no_bound_scan():
    rows = O.gen_rows(77, 0, 5000, 100)                                    # 100 is no multiple of 16
    idx = quiver_amd.DeviceIndex(100, "cosine"); idx.add(rows)
    _, took, _, _ = both(idx, rows[3:7], 10)
    assert took == 0
    idx.close()
    rows = O.gen_rows(78, 0, 5000, 128)
    for make in ("flag", "metric"):
        idx = quiver_amd.DeviceIndex(128, "l2" if make == "metric" else "cosine", scan_plane=make != "flag")
        idx.add(rows)
        assert not idx.bound_scan_stats()["plane"]
        (r, _, _), took, _, _ = both(idx, rows[3:7], 10)
        assert took == 0 and r[:, 0].tolist() == [3, 4, 5, 6]
        idx.close()
    idx = quiver_amd.DeviceIndex(128, "cosine"); idx.add(rows)
    (r, _, _), took, _, _ = both(idx, rows[3:12], 10)                      # 9 queries
    assert took == 0 and r[:, 0].tolist() == list(range(3, 12))
    (r, _, _), took, _, _ = both(idx, rows[3:7], 65)                       # k = 65
    assert took == 0 and r[:, 0].tolist() == [3, 4, 5, 6]
    (r, _, _), took, _, _ = both(idx, rows[3:7], 64)                       # (and the shape next to them is taken)
    assert took == 4
    idx.close()
