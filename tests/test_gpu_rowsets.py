"""Row sets: device-resident filters, one per query (qv_rowset_*, qv_index_search_rowsets*; quiver_amd/csrc/qv_rowset.hip).

A filtered Collection.Search ranks every row and keeps the first k whose metadata matches (pkg/core/collection.go:679-759); with the
match set known as a row bitmap the same k rows are the top-k over live & set.  Every comparison here is rows and float32 bits against
tests/_oracle.exact_search(metric, rows, q, k, alive=live & set_q) — the oracle call tests/test_gpu_flat.py uses for
qv_index_search_masked."""
import re
import threading

import numpy as np
import pytest

import quiver_amd
from tests import _extremes as X, _oracle as O

pytestmark = pytest.mark.gpu

METRICS = ["cosine", "l2", "l2sq", "dot", "l1", "cosine_f32", "l2_f32", "dot_f32", "l2sq_f64"]
SPLIT_OK = {"cosine", "l2", "dot", "l1", "l2sq_f64"}       # metrics whose chain the tile-over-eight-waves form can split and certify
NQS = (1, 3, 8, 9, 17, 40)
KS = (1, 10, 64)
DENSITIES = (1.0, 0.5, 0.1, 0.02, 0.005)


@pytest.fixture(autouse=True)
def _trace_kernels(monkeypatch):
    """QV_TRACE=1 (read at the first row-set scan of the process): the launcher names the kernel it chose on stderr"""
    monkeypatch.setenv("QV_TRACE", "1")


def _bits(mask):
    return np.ascontiguousarray(mask, dtype=bool)


def _make_sets(idx, n, nq, live, rng):
    """nq (RowSet or None, bool mask) pairs: densities 0.5 % .. 100 %, an empty set, a None, a set holding tombstoned rows, and a set
    with whole 64-row tiles unselected"""
    dead = np.flatnonzero(~live)
    out = []
    for q in range(nq):
        if q == 1:
            m = np.zeros(n, bool)                                              # the empty set
        elif q == 2:
            out.append((None, np.ones(n, bool)))                              # no filter
            continue
        elif q == 3:
            m = (np.arange(n) // 64) % 5 == 1                                  # four tiles of five unselected
        else:
            m = rng.random(n) < DENSITIES[q % len(DENSITIES)]
        if q == 4:
            m[dead[:32]] = True                                                # selecting a tombstoned row selects nothing
        out.append((idx.rowset(m), m))
    return out


def _oracle_lists(mid, rows, qs, sets, live, k):
    return [O.exact_search(mid, rows, qs[i], k, alive=(live & sets[i][1]).astype(np.uint8)) for i in range(len(sets))]


def _check(r, d, c, want, k, where):
    for i, (ro, do) in enumerate(want):
        w = min(k, ro.size)
        assert int(c[i]) == w, (where, i, int(c[i]), w)
        assert r[i, :w].tolist() == ro[:w].tolist(), (where, i)
        assert d[i, :w].tobytes() == do[:w].tobytes(), (where, i)
        assert (r[i, w:] == 0xFFFFFFFF).all() and np.isposinf(d[i, w:]).all(), (where, i)


# (metric, dim, n) twice per metric: a corpus whose multi-query pass takes whole tiles per wave (long, or rows too narrow for the other
# form, or a metric whose chain cannot be split), and a short corpus of wide rows (the tile-over-eight-waves form where the metric allows
# it).  n always leaves a partial last tile.  Dimensions 16 / 33 / 128 / 768 all occur.
LONG = [("cosine", 768, 165_037), ("l2", 128, 170_003), ("l2sq", 33, 20_011), ("dot", 16, 30_001), ("l1", 33, 25_013),
        ("cosine_f32", 768, 9_001), ("l2_f32", 16, 20_011), ("dot_f32", 128, 12_007), ("l2sq_f64", 128, 165_037)]
SHORT = [("cosine", 768, 6_003), ("l2", 128, 9_001), ("l2sq", 128, 9_001), ("dot", 768, 5_011), ("l1", 128, 12_007),
         ("cosine_f32", 128, 6_003), ("l2_f32", 768, 5_011), ("dot_f32", 768, 6_003), ("l2sq_f64", 768, 9_001)]


@pytest.mark.parametrize("metric,dim,n,short", [c + (False,) for c in LONG] + [c + (True,) for c in SHORT])
def test_distinct_set_per_query_equals_the_oracle(metric, dim, n, short, capfd):
    mid = quiver_amd.metric_id(metric)
    rows = O.gen_rows(8100 + dim, 0, n, dim)
    idx = quiver_amd.DeviceIndex(dim, metric)
    idx.add(rows)
    dead = np.arange(3, n, 89, dtype=np.uint32)
    idx.remove(dead)
    live = np.ones(n, bool); live[dead] = False
    rng = np.random.default_rng(dim + n)
    qs = O.gen_rows(8200 + dim, 0, max(NQS), dim)
    sets = _make_sets(idx, n, max(NQS), live, rng)
    want = _oracle_lists(mid, rows, qs, sets, live, max(KS))
    capfd.readouterr()
    for nq in NQS:
        for k in KS:
            r, d, c = idx.search_rowsets(qs[:nq], k, [s for s, _ in sets[:nq]])
            _check(r, d, c, want[:nq], k, (metric, nq, k))
    # a pass whose sets ALL leave the same tiles out: those tiles are skipped (and the results are still the oracle's)
    stripe = (np.arange(n) // 64) % 3 == 0
    part = []
    for q in range(8):
        m = stripe & (rng.random(n) < (0.3 if q % 2 else 1.0))
        part.append((idx.rowset(m), m))
    r, d, c = idx.search_rowsets(qs[:8], 10, [s for s, _ in part])
    _check(r, d, c, _oracle_lists(mid, rows, qs[:8], part, live, 10), 10, (metric, "stripes"))
    # which kernels ran (QV_TRACE): both group widths of the form this corpus takes
    err = capfd.readouterr().err
    seen = set(re.findall(r"scan kernel = (k_rowset_scan\w+) QB=(\d+)", err))
    form = "k_rowset_scan_split_mq" if short and metric in SPLIT_OK else "k_rowset_scan_mq"
    assert {(form, "4"), (form, "8")} <= seen, (metric, seen)
    if form == "k_rowset_scan_mq" and metric in SPLIT_OK:                       # the float64-accumulating metrics: 16 per pass from 9 queries on
        assert (form, "16") in seen, (metric, seen)
    for s, _ in sets + part:
        if s is not None:
            s.close()


@pytest.mark.parametrize("metric,dim,n,nq", [("cosine", 128, 200_001, 8), ("l2sq", 64, 50_003, 5), ("dot", 768, 7_001, 6)])
def test_same_set_for_all_queries_equals_search_masked(metric, dim, n, nq):
    """the parent's path as a second witness: one set named by every query = qv_index_search_masked with that mask"""
    rows = O.gen_rows(8300, 0, n, dim)
    idx = quiver_amd.DeviceIndex(dim, metric)
    idx.add(rows)
    idx.remove(np.arange(1, n, 53, dtype=np.uint32))
    rng = np.random.default_rng(5)
    mask = rng.random(n) < 0.07
    qs = O.gen_rows(8301, 0, nq, dim)
    with idx.rowset(mask) as rs:
        for k in (1, 10, 64):
            r, d, c = idx.search_rowsets(qs, k, rs)
            mr, md, mc = idx.search_masked(qs, k, mask)
            assert np.array_equal(c, mc)
            for i in range(nq):
                w = int(c[i])
                assert np.array_equal(r[i, :w], mr[i, :w]) and d[i, :w].tobytes() == md[i, :w].tobytes(), (k, i)
        r1, d1, c1 = idx.search_rowsets(qs[:1], 10, [rs])                       # one query: the single-query kernels over alive & set
        mr, md, mc = idx.search_masked(qs[:1], 10, mask)
        assert np.array_equal(r1, mr[:, :10]) and d1.tobytes() == md[:, :10].tobytes() and int(c1[0]) == int(mc[0])


# long (one launch, the last workgroup merges), short and wide (a tile over eight waves), small (scan + merge in one polled launch)
@pytest.mark.parametrize("metric,dim,n", [("cosine", 128, 200_001), ("cosine", 768, 6_003), ("l2", 64, 9_001), ("l2sq", 33, 3_001), ("dot_f32", 128, 70_003)])
def test_one_query_whose_set_holds_fewer_live_rows_than_k_or_none(metric, dim, n):
    """one query with k <= 64 runs the single-query kernels over alive & set with lists k long: they pad what the set cannot fill.  Host
    form and device form, an empty set, a set whose rows are all tombstoned, and sets of 1 / 7 live rows (k = 10 and 64) and 40 (k = 64)."""
    import torch
    mid = quiver_amd.metric_id(metric)
    rows = O.gen_rows(8350 + dim, 0, n, dim)
    idx = quiver_amd.DeviceIndex(dim, metric)
    idx.add(rows)
    dead = np.arange(4, n, 61, dtype=np.uint32)
    idx.remove(dead)
    live = np.ones(n, bool); live[dead] = False
    rng = np.random.default_rng(n)
    q = O.gen_rows(8351, 0, 1, dim)
    alive_rows = np.flatnonzero(live)
    masks = [np.zeros(n, bool)]
    m = np.zeros(n, bool); m[dead[:20]] = True; masks.append(m)                 # only tombstoned rows
    for cnt in (1, 7, 40):
        m = np.zeros(n, bool); m[rng.choice(alive_rows, cnt, replace=False)] = True; m[dead[:3]] = True
        masks.append(m)
    st = torch.cuda.Stream()
    for m in masks:
        with idx.rowset(m) as rs:
            for k in (1, 10, 64):
                ro, do = O.exact_search(mid, rows, q[0], k, alive=(live & m).astype(np.uint8))
                assert ro.size == min(k, int((live & m).sum()))
                r, d, c = idx.search_rowsets(q, k, rs)
                _check(r, d, c, [(ro, do)], k, (metric, int(m.sum()), k, "host"))
                with torch.cuda.stream(st):
                    dq = torch.from_numpy(q).cuda()
                    dr = torch.zeros((1, k), dtype=torch.int32, device="cuda"); dd = torch.zeros((1, k), dtype=torch.float32, device="cuda")
                    idx.search_rowsets_device(dq.data_ptr(), 1, k, rs, dr.data_ptr(), dd.data_ptr(), st.cuda_stream)
                    r2 = dr.cpu().numpy().view(np.uint32); d2 = dd.cpu().numpy()
                assert np.array_equal(r2, r) and d2.tobytes() == d.tobytes(), (metric, int(m.sum()), k, "device")


def test_more_than_64_results_per_query():
    """k = 100 / 500 / k > |set|: runs of queries naming the same set go through the selection and ranking paths over alive & set"""
    n, dim, nq = 40_007, 64, 6
    rows = O.gen_rows(8400, 0, n, dim)
    idx = quiver_amd.DeviceIndex(dim, "cosine")
    idx.add(rows)
    dead = np.arange(0, n, 31, dtype=np.uint32)
    idx.remove(dead)
    live = np.ones(n, bool); live[dead] = False
    rng = np.random.default_rng(9)
    masks = [rng.random(n) < 0.2, rng.random(n) < 0.005, np.zeros(n, bool)]
    rs = [idx.rowset(m) for m in masks]
    qs = O.gen_rows(8401, 0, nq, dim)
    # queries 0-1 name set 0, 2 names no set, 3-4 set 1 (about 190 live rows: fewer than k = 500), 5 the empty set
    sets = [(rs[0], masks[0]), (rs[0], masks[0]), (None, np.ones(n, bool)), (rs[1], masks[1]), (rs[1], masks[1]), (rs[2], masks[2])]
    for k in (100, 500, 9000):
        want = _oracle_lists(0, rows, qs, sets, live, k)
        r, d, c = idx.search_rowsets(qs, k, [s for s, _ in sets])
        _check(r, d, c, want, k, k)
    assert int((live & masks[1]).sum()) < 500


def test_growth_and_mutation():
    n, dim, k = 10_000, 48, 10
    rows = O.gen_rows(8500, 0, n + 3000, dim)
    idx = quiver_amd.DeviceIndex(dim, "l2")
    idx.add(rows[:n])
    rng = np.random.default_rng(3)
    m = np.zeros(n + 3000, bool); m[:n] = rng.random(n) < 0.05
    qs = O.gen_rows(8501, 0, 4, dim)
    live = np.zeros(n + 3000, bool); live[:n] = True

    def check(rs, where, total=None):
        cur = rows[:idx.rows()]
        for sets in ([rs] * 4, [rs, None, rs, None]):
            r, d, c = idx.search_rowsets(qs, k, sets)
            want = [O.exact_search(1, cur, qs[i], k, alive=(live[:idx.rows()] & (m[:idx.rows()] if s is not None else True)).astype(np.uint8))
                    for i, s in enumerate(sets)]
            _check(r, d, c, want, k, where)
        r1, d1, c1 = idx.search_rowsets(qs[:1], k, rs)
        _check(r1, d1, c1, [O.exact_search(1, cur, qs[0], k, alive=(live[:idx.rows()] & m[:idx.rows()]).astype(np.uint8))], k, where)
        assert rs.count() == int(m.sum())

    rs = idx.rowset(m[:n])
    check(rs, "created")
    idx.add(rows[n:])                                                          # the index grows: the new rows start unselected
    live[n:] = True
    check(rs, "grown")
    new = np.arange(n + 5, n + 3000, 3, dtype=np.uint32)
    rs.set_rows(new, True); m[new] = True
    check(rs, "new rows selected")
    drop = np.flatnonzero(m)[::4].astype(np.uint32)
    rs.set_rows(drop, False); m[drop] = False
    check(rs, "rows dropped")
    gone = np.flatnonzero(m)[::3].astype(np.uint32)                            # tombstones set after the set was made are honoured
    idx.remove(gone); live[gone] = False
    check(rs, "rows removed")
    back = int(gone[0])                                                        # an update revives the row, with new contents
    rows[back] = O.gen_rows(8502, 0, 1, dim)[0]
    idx.update(back, rows[back]); live[back] = True
    check(rs, "row updated")
    with pytest.raises(quiver_amd.QvError) as e:
        rs.set_rows([idx.rows()], True)
    assert e.value.code == -4
    other = quiver_amd.DeviceIndex(dim, "l2"); other.add(rows[:100])
    with pytest.raises(quiver_amd.QvError) as e:                               # a set of another index
        other.search_rowsets(qs, k, rs)
    assert e.value.code == -1
    rs.close()


def test_a_set_from_a_mask_words_and_row_numbers_is_the_same_set():
    n, dim = 640, 16                                                           # 10 words: 10 uint64 row numbers have a mask's length
    idx = quiver_amd.DeviceIndex(dim, "l2")
    idx.add(O.gen_rows(8600, 0, n, dim))
    q = O.gen_rows(8601, 0, 1, dim)
    picked = np.array([1, 64, 65, 130, 200, 333, 400, 511, 600, 639])
    m = np.zeros(n, bool); m[picked] = True
    words = np.packbits(m, bitorder="little").view(np.uint64)
    want = idx.search_rowsets(q, 10, idx.rowset(m))
    for rs in (idx.rowset(words), idx.rowset(picked.astype(np.int64)), idx.rowset(rows=picked.astype(np.uint64)), idx.rowset(rows=picked.tolist())):
        assert rs.count() == picked.size
        got = idx.search_rowsets(q, 10, rs)
        assert sorted(got[0][0].tolist()) == picked.tolist()
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert idx.rowset(picked.astype(np.uint64)).count() != picked.size         # uint64 without rows= is ten mask words
    with pytest.raises(ValueError):
        idx.rowset(m, rows=picked)
    with pytest.raises(ValueError):
        idx.rowset(rows=[-1])


@pytest.mark.parametrize("n,dim,nq,k", [(150_001, 128, 11, 10), (6_003, 768, 7, 64), (20_011, 64, 1, 10), (20_011, 64, 5, 200)])
def test_device_form_on_a_busy_stream_equals_the_host_form(n, dim, nq, k):
    """the call is enqueued behind other work on the caller's stream; nothing waits on that stream between the enqueue and the copy
    of the results (which is ordered behind it on the same stream)"""
    import torch
    rows = O.gen_rows(8600, 0, n, dim)
    idx = quiver_amd.DeviceIndex(dim, "cosine")
    idx.add(rows)
    idx.remove(np.arange(2, n, 41, dtype=np.uint32))
    rng = np.random.default_rng(1)
    owned = [idx.rowset(rng.random(n) < f) for f in (0.3, 0.01)]
    sets = [owned[0] if i < 3 else (None if i == 3 else owned[1]) for i in range(nq)] if nq > 1 else [owned[1]]
    qs = O.gen_rows(8601, 0, nq, dim)
    hr, hd, hc = idx.search_rowsets(qs, k, sets)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a = torch.randn(4096, 4096, device="cuda")
        for _ in range(20):
            a = a @ a * 1e-3                                                   # keeps the stream busy while the search is enqueued
        dq = torch.from_numpy(qs).cuda(non_blocking=True)
        dr = torch.zeros((nq, k), dtype=torch.int32, device="cuda"); dd = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        idx.search_rowsets_device(dq.data_ptr(), nq, k, sets, dr.data_ptr(), dd.data_ptr(), st.cuda_stream)
        r = dr.cpu().numpy().view(np.uint32); d = dd.cpu().numpy()            # (stream-ordered copies: the only wait is for them)
    assert np.array_equal(r, hr) and d.tobytes() == hd.tobytes()
    for i in range(nq):
        assert int((r[i] != 0xFFFFFFFF).sum()) == int(hc[i])
    for s in owned:
        s.close()


def test_concurrent_callers_each_with_their_own_set_share_passes():
    """Python threads (ctypes releases the interpreter lock), one query per call in a closed loop, every caller with its own set, on the
    corpus size where tests/test_gpu_concurrent.py sees the unfiltered front share passes"""
    n, dim, k, threads, calls = 300_000, 768, 10, 32, 10
    idx = quiver_amd.DeviceIndex(dim, "cosine")
    idx.add_synthetic(20260424, 0, n)
    corpus = O.gen_rows(20260424, 0, n, dim)
    dead = np.arange(7, n, 101, dtype=np.uint32)
    idx.remove(dead)
    live = np.ones(n, bool); live[dead] = False
    qs = O.gen_rows(20260426, 0, threads, dim)
    rng = np.random.default_rng(77)
    masks = [rng.random(n) < (0.5, 0.1, 0.01, 0.002)[t % 4] for t in range(threads)]
    sets = [idx.rowset(m) for m in masks]
    before = quiver_amd.lib().qv_index_coalesce_stats
    import ctypes as C
    un0 = (C.c_uint64 * 8)(); before(idx.handle, un0)
    out, errs = {}, []

    def caller(t):
        try:
            for it in range(calls):
                out[(t, it)] = idx.search_rowsets(qs[t:t + 1], k, sets[t])
        except Exception as e:                                                  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=caller, args=(t,)) for t in range(threads)]
    [x.start() for x in th]; [x.join() for x in th]
    assert not errs, errs
    want = [O.exact_search(0, corpus, qs[t], k, alive=(live & masks[t]).astype(np.uint8)) for t in range(threads)]
    for (t, it), (r, d, c) in out.items():
        _check(r, d, c, [want[t]], k, (t, it))
    st = idx.rowset_coalesce_stats()
    assert st["solo"] + st["led"] + st["rode"] == threads * calls
    assert st["group_queries"] > st["groups"] >= 1, st                          # passes were shared
    un1 = (C.c_uint64 * 8)(); before(idx.handle, un1)
    assert list(un0) == list(un1)                                               # the unfiltered front saw none of this

    # filtered and unfiltered callers on one handle
    plain = [O.exact_search(0, corpus, qs[t], k, alive=live.astype(np.uint8)) for t in range(8)]
    out2, errs2 = {}, []

    def mixed(t):
        try:
            for it in range(6):
                out2[(t, it)] = idx.search_rowsets(qs[t:t + 1], k, sets[t]) if t % 2 else idx.search(qs[t:t + 1], k)
        except Exception as e:                                                  # noqa: BLE001
            errs2.append(e)

    th = [threading.Thread(target=mixed, args=(t,)) for t in range(8)]
    [x.start() for x in th]; [x.join() for x in th]
    assert not errs2, errs2
    for (t, it), (r, d, c) in out2.items():
        _check(r, d, c, [want[t] if t % 2 else plain[t]], k, ("mixed", t, it))
    for s in sets:
        s.close()


@pytest.mark.parametrize("metric,dim,n", [("cosine", 128, 9_001), ("l2", 64, 20_011), ("cosine_f32", 64, 20_011), ("dot", 768, 5_011), ("l1", 33, 9_001)])
def test_extreme_rows_through_the_row_set_kernels(metric, dim, n):
    """NaN / Inf / huge-magnitude / zero / denormal rows (tests/_extremes.py) among ordinary ones, inside and outside the sets"""
    mid = quiver_amd.metric_id(metric)
    rng = np.random.default_rng(42)
    rows = O.gen_rows(8700, 0, n, dim)
    special = X.class_rows(rng, dim)
    at = rng.choice(n, len(special), replace=False)
    for pos, (_, _, v) in zip(at, special):
        rows[pos] = v
    idx = quiver_amd.DeviceIndex(dim, metric)
    idx.add(rows)
    live = np.ones(n, bool)
    qs = np.concatenate([O.gen_rows(8701, 0, 6, dim), np.stack([special[0][2], special[len(special) // 2][2]])])
    sets = []
    for q in range(qs.shape[0]):
        m = rng.random(n) < 0.05
        m[at[q % 2::2]] = True                                                 # half of the special rows in every set
        sets.append((idx.rowset(m), m))
    for k in (10, 64):
        r, d, c = idx.search_rowsets(qs, k, [s for s, _ in sets])
        for i in range(qs.shape[0]):
            ro, do = O.exact_search(mid, rows, qs[i], k, alive=(live & sets[i][1]).astype(np.uint8))
            assert int(c[i]) == ro.size and r[i, :ro.size].tolist() == ro.tolist(), (metric, k, i)
            assert X.same(d[i, :ro.size], do), (metric, k, i)
    for s, _ in sets:
        s.close()
