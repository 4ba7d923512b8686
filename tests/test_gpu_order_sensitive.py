"""Every exact path on rows whose float32 distance depends on the order of summation (tests/_order.py).

The planted rows give the reference chain's float32 only when a row's terms are added as ONE chain in element order; reversed,
chunk-reversed, pairwise, exact, and the split forms' orders give other bits (tests/test_order_sensitive_cpu.py proves each order
is caught, and that the split forms' certificate decides none of them: the fallback must run and be right).  Each corpus holds
the planted rows of its queries and filler rows that are, by construction and checked on the CPU, farther from every query —
so every path must return the planted rows' distances.  Rows, float32 bits and counts against the CPU oracle; for HNSW also
the evaluation counts.  The shapes select the paths of DESIGN.md §4.1."""
import numpy as np
import pytest

import quiver_amd
from quiver_amd.device_index import DeviceGraph, ShardedIndex, distance_pairs
from tests import _callers
from tests import _oracle as O
from tests import _order as OR

pytestmark = pytest.mark.gpu

NAMES = {0: "cosine", 1: "l2", 2: "l2sq", 3: "dot", 4: "l1", 5: "cosine_f32", 6: "l2_f32", 7: "dot_f32", 8: "l2sq_f64"}
_case = OR._case                 # (shared with tests/test_gpu_filtered_batch_edges.py)


def _same(got_r, got_d, got_c, want_r, want_d, what):
    assert int(got_c) == want_r.size, what
    assert got_r[:want_r.size].tolist() == want_r.tolist(), what
    assert got_d[:want_r.size].tobytes() == want_d.tobytes(), what


def _check(idx, metric, corpus, qs, k, what, per_call=0, batched=False, alive=None):
    want = [O.exact_search(metric, corpus, q, k, alive=alive) for q in qs]
    if per_call:
        for lo in range(0, qs.shape[0], per_call):
            r, d, c = idx.search(qs[lo:lo + per_call], k, batched=batched)
            for i in range(r.shape[0]):
                _same(r[i], d[i], c[i], *want[lo + i], (what, lo + i))
    else:
        r, d, c = idx.search(qs, k, batched=batched)
        for i in range(qs.shape[0]):
            _same(r[i], d[i], c[i], *want[i], (what, i))
    return want


def _index(metric, dim, corpus, **kw):
    idx = quiver_amd.DeviceIndex(dim, NAMES[metric], **kw)
    idx.add(corpus)
    return idx


# ------------------------------------------------------------------------------------------------- one query per call --
@pytest.mark.parametrize("metric", OR.SPLIT_METRICS)
@pytest.mark.parametrize("dim", [128, 256, 768, 1536])
def test_split_scan_and_its_fallback(metric, dim):
    """1 query, D >= 128, <= 160 k rows, k <= 64: k_flat_scan_split (the certificate fails on every planted row); then 2 .. 11
    queries of the same short corpus: k_flat_scan_split_mq"""
    qs, corpus, own = _case(metric, dim, 11, 100 + dim + metric, 3000)
    idx = _index(metric, dim, corpus)
    for k in (10, 64):
        _check(idx, metric, corpus, qs, k, ("split", k), per_call=1)
    for n in (2, 5, 11):
        _check(idx, metric, corpus, qs[:n], 24, ("split_mq", n))
    idx.close()


@pytest.mark.parametrize("metric,dim", [(m, d) for m in OR.F64_METRICS for d in (32, 100)] +
                         [(m, d) for m in OR.F32_METRICS for d in (100, 256)])
def test_lane_per_row_scans(metric, dim):
    """a lane per row: k_flat_scan (D < 128 over 20 k rows; the float32 metrics at any D) and k_flat_scan_small (3 k rows,
    k <= 16); then k_flat_scan_wide (k 65 .. 128), one key per row + selection (k 129 .. 8192) and the full ranking (k = N)"""
    qs, corpus, own = _case(metric, dim, 3, 200 + dim + metric, 20000)
    idx = _index(metric, dim, corpus)
    for k in (10, 64, 100, 300):
        _check(idx, metric, corpus, qs, k, ("scan", k), per_call=1)
    small = _index(metric, dim, corpus[:3000])
    _check(small, metric, corpus[:3000], qs, 16, "small", per_call=1)
    _check(small, metric, corpus[:3000], qs[:1], 3000, "full ranking", per_call=1)
    idx.close(); small.close()


@pytest.mark.parametrize("metric", [OR.COSINE, OR.L2, OR.DOT])
def test_long_corpus_scans(metric):
    """more than 163 840 rows: k_flat_scan for one query at D >= 128, the multi-query list scans for 2 .. 8"""
    dim = 128
    qs, corpus, own = _case(metric, dim, 8, 300 + metric, 170_000)
    idx = _index(metric, dim, corpus)
    _check(idx, metric, corpus, qs[:2], 20, "long, one query", per_call=1)
    for n in (2, 8):
        _check(idx, metric, corpus, qs[:n], 20, ("long, mq", n))
    idx.close()


# ------------------------------------------------------------------------------------------------------ batches of >= 9 --
@pytest.mark.parametrize("metric", [OR.COSINE, OR.DOT])
def test_mq64_matrix_scan(metric, monkeypatch):
    """>= 9 cosine / dot queries with the filter off over a long scan: k_flat_scan_mq64 (v_mfma_f64_16x16x4_f64 chains, a
    4-element chunk per k-step)"""
    monkeypatch.setattr(quiver_amd.DeviceIndex, "default_filter", "off")
    dim = 32
    qs, corpus, own = _case(metric, dim, 12, 400 + metric, 530_000)
    idx = _index(metric, dim, corpus)
    _check(idx, metric, corpus, qs, 20, "mq64")
    idx.close()


@pytest.mark.parametrize("metric", [OR.COSINE, OR.DOT, OR.L2, OR.L2SQ])
def test_batched_filter_and_exact_rescore(metric):
    """>= 9 queries over >= 32 k rows: the matrix-core filter, then every survivor re-scored by the exact lane-per-row chain;
    the default filter, the fp32 filter (set_filter) and the bfloat16 row copy"""
    dim = 256
    qs, corpus, own = _case(metric, dim, 12, 500 + metric, 40_000)
    for kw, filt in (({}, None), ({}, "fp32"), ({"bf16_rows": True}, None)):
        idx = _index(metric, dim, corpus, **kw)
        if filt:
            idx.set_filter(filt)
        for k in (10, 40):
            _check(idx, metric, corpus, qs, k, ("batched", kw, filt, k), batched=True)
        idx.close()


@pytest.mark.parametrize("metric,dim", [(OR.COSINE, 384), (OR.L2, 512), (OR.DOT, 768)])
def test_batched_qreg_filter(metric, dim):
    """whole 256-query groups at 384 / 512 / 768 dimensions: k_qreg_filter, then the exact re-score"""
    qs, corpus, own = _case(metric, dim, 256, 600 + dim, 36_000)
    idx = _index(metric, dim, corpus)
    _check(idx, metric, corpus, qs, 10, "qreg", batched=True)
    idx.close()


@pytest.mark.parametrize("metric", [OR.COSINE, OR.L2])
def test_batched_selection_path_and_large_k(metric):
    """k 16 .. 64 on >= 131 072 rows: the selection path (narrowing, exact survivors, k_select_sort); k > 64: large k"""
    dim = 128
    qs, corpus, own = _case(metric, dim, 10, 700 + metric, 140_000)
    idx = _index(metric, dim, corpus)
    for k in (32, 100):
        _check(idx, metric, corpus, qs, k, ("selection", k), batched=True)
    idx.close()


# ------------------------------------------------------------------------------------------------ other entry points --
@pytest.mark.parametrize("metric", [OR.COSINE, OR.L2, OR.DOT, OR.L1, OR.L2SQ_F64, OR.DOT_F32])
def test_masked_and_negative_example_search(metric):
    dim = 256
    qs, corpus, own = _case(metric, dim, 3, 800 + metric, 5000)
    idx = _index(metric, dim, corpus)
    rng = np.random.default_rng(metric)
    alive = rng.random(corpus.shape[0]) < 0.7
    for j, q in enumerate(qs):
        r, d, c = idx.search_masked(q, 20, alive)
        _same(r[0], d[0], c[0], *O.exact_search(metric, corpus, q, 20, alive=alive.astype(np.uint8)), ("masked", j))
        for neg in (q, qs[(j + 1) % len(qs)]):
            er, ed = O.exact_search(metric, corpus, q, 40)
            r, d, nd, c = idx.search_negative(q, neg, 40)
            assert c == er.size and r[:c].tolist() == er.tolist() and d[:c].tobytes() == ed.tobytes(), ("negative", j)
            assert nd[:c].tobytes() == O.all_distances(metric, corpus[er], neg).tobytes(), ("negative", j)
    idx.close()


@pytest.mark.parametrize("metric", range(9))
def test_distance_entry_points(metric):
    """distance_pairs (k_distance_pairs), distance_rows and distance_rows_device (the neighbour-distance batch) on every
    planted row"""
    import torch
    dim = 256
    qs, corpus, own = _case(metric, dim, 2, 900 + metric, 200)
    for j, q in enumerate(qs):
        ids = own[j].astype(np.uint32)
        want = O.all_distances(metric, corpus[ids], q)
        got = distance_pairs(NAMES[metric], np.repeat(q[None], ids.size, 0), corpus[ids])
        assert got.tobytes() == want.tobytes(), ("pairs", j)
        idx = _index(metric, dim, corpus)
        assert idx.distance_rows(q, ids).tobytes() == want.tobytes(), ("rows", j)
        dq = torch.from_numpy(q).cuda(); di = torch.from_numpy(ids.view(np.int32)).cuda()
        do = torch.empty(ids.size, dtype=torch.float32, device="cuda")
        stream = torch.cuda.current_stream()
        idx.distance_rows_device(dq.data_ptr(), di.data_ptr(), ids.size, do.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert do.cpu().numpy().tobytes() == want.tobytes(), ("rows_device", j)
        idx.close()


def test_sharded_handle():
    """co-located shards (peer copy): each shard's scan, then the merge"""
    metric, dim = OR.L2, 256
    qs, corpus, own = _case(metric, dim, 4, 1000, 6000)
    sh = ShardedIndex(dim, "l2", devices=[0, 0, 0], peer_copy=True)
    ids = sh.add(corpus).astype(np.int64)
    assert np.all(np.diff(ids) > 0)                  # global ids rise with the corpus position: the same (distance, row) order
    for k in (10, 30):
        r, d, c = sh.search(qs, k)
        for i in range(qs.shape[0]):
            local = np.searchsorted(ids, r[i, :c[i]].astype(np.int64)).astype(np.uint32)
            assert np.array_equal(ids[local], r[i, :c[i]]), ("sharded", k, i)
            _same(local, d[i], c[i], *O.exact_search(metric, corpus, qs[i], k), ("sharded", k, i))
    sh.close()


@pytest.mark.parametrize("metric", [OR.COSINE, OR.L1])
def test_coalesced_callers(metric):
    """a few threads, one query per call: the calls share passes (qv_coalesce)"""
    dim = 256
    qs, corpus, own = _case(metric, dim, 8, 1100 + metric, 4000)
    idx = _index(metric, dim, corpus)
    res = _callers.run("index", idx.handle, qs, 10, threads=4, seconds=20.0, max_calls_per_thread=8)
    assert res["rc"] == 0, res["error"]
    assert res["errors"] == 0 and res["mismatches"] == 0
    for i in range(qs.shape[0]):
        _same(res["rows"][i], res["dist"][i], res["count"][i], *O.exact_search(metric, corpus, qs[i], 10), ("callers", i))
    idx.close()


# ------------------------------------------------------------------------------------------------------------------ HNSW --
def _graph(metric, corpus, m, seed):
    """half of each node's links its nearest rows (float64 numpy: any graph will do, the oracle walks the same one), half
    random: the planted clusters and the fillers are connected"""
    rng = np.random.default_rng(seed)
    n = corpus.shape[0]
    x = corpus.astype(np.float64)
    x = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-300)
    near = np.argsort(-(x @ x.T), axis=1)[:, 1:m // 2 + 1]
    links = np.zeros((n, m), np.uint32)
    for i in range(n):
        rnd = rng.choice(n - 1, size=m - m // 2, replace=False)
        rnd = rnd + (rnd >= i)
        links[i] = np.concatenate([near[i], rnd])
    return np.full(n, m, np.uint32), links


@pytest.mark.parametrize("metric,dim,nq", [
    (OR.COSINE, 768, 16), (OR.L2, 256, 16), (OR.DOT, 128, 16), (OR.L1, 256, 16), (OR.L2SQ_F64, 512, 16),   # latency form, tier 1
    (OR.COSINE, 256, 400), (OR.L2, 128, 400),                                                          # tier 2
    (OR.COSINE, 256, 800), (OR.L2, 96, 800), (OR.DOT, 100, 800), (OR.L2SQ, 64, 800),                   # wave form (D % 32: LDS)
    (OR.COSINE_F32, 256, 16), (OR.L2_F32, 64, 16),
])
def test_hnsw_forms(metric, dim, nq):
    """the latency form (a workgroup per query, split chains certified: the planted rows all go through its fallback), its
    second tier, and the wave form; duplicated planted rows bring the exact-heap pass in.  Rows, bits, evaluation counts."""
    k, ef, m = 10, 96, 16
    n_distinct = 4
    qd, corpus, own = _case(metric, dim, n_distinct, 1200 + dim + metric, 1200, dup=3)
    qs = np.ascontiguousarray(qd[np.arange(nq) % n_distinct])
    deg, links = _graph(metric, corpus, m, metric + dim)
    n = corpus.shape[0]
    idx = quiver_amd.DeviceIndex(dim, NAMES[metric], rowmajor=True)
    idx.add(corpus)
    g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=5)
    try:
        o = O.HNSW(metric, dim, M=m // 2, maxM0=m, efSearch=ef, maxLevel=1, seed=1)
        o.load_flat(corpus, deg, links, 5)
        r, d, c, ev = g.search(qs, k, ef, with_evals=True)
        found = 0
        for i in range(n_distinct):
            ro, do, eo = o.search(qs[i], k, with_evals=True)
            found += len(set(ro.tolist()) & set(own[i].tolist()))
            for j in range(i, nq, n_distinct):
                assert int(c[j]) == ro.size == k, (j, c[j])
                assert r[j].tolist() == ro.tolist(), j
                assert d[j].tobytes() == do.tobytes(), j
                assert int(ev[j]) == eo - 1, j             # the reference evaluates the entry point once more up front (hnsw.go:637)
        assert found >= n_distinct * k // 2                # the walks reach the planted rows
    finally:                                               # the graph before its index, also when an assertion fails
        g.close(); idx.close()
