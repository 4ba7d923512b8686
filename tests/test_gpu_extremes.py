"""Non-finite and extreme-magnitude vectors (value classes N I O G Z D of tests/_extremes.py) through every search path, against
the CPU oracle: rows, counts, and distances bit-equal where the oracle's value is a number and NaN where it is NaN (DESIGN.md §2:
distance ascending, then row; NaN last; -0 == +0).  The guards these inputs take are the filters' give-ups on rows and queries
whose norm is NaN, infinite, >= 1e18 or below filter_tiny_norm, the NaN score kept for the exact pass, the NaN key after +inf,
the mq64 one-sided threshold test, and the traversal's NaN / tie flag.

Corpora are ordinary generator rows with extreme rows written in at chosen places, in three regimes: a few extreme rows (fewer
than k), about a fifth of the rows NaN- or +inf-distance (candidate lists overflow and hand back), and fewer finite-distance live
rows than k (NaN and +inf rows come back in row order).  Where the oracle over the whole corpus is too slow for every query, every
query is compared with the exact multi-query scan of the same index (set_filter("off")), and every extreme query plus two ordinary
ones with the oracle."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import quiver_amd
from quiver_amd.device_index import DeviceGraph, distance_pairs
from tests import _extremes as X
from tests import _oracle as O

pytestmark = pytest.mark.gpu

METRICS = ["cosine", "l2", "l2sq", "dot", "l1", "cosine_f32", "l2_f32", "dot_f32", "l2sq_f64"]
MID = {m: quiver_amd.metric_id(m) for m in METRICS}


# ---------------------------------------------------------------------------------------------------------------- inputs ---
_corpus, _queries = X._corpus, X._queries                              # (shared with tests/test_gpu_filtered_batch_edges.py)


_POOL = ThreadPoolExecutor(max_workers=16)                              # ctypes drops the GIL: the oracle scales with threads


def _want(metric, rows, qs, k, which=None, alive=None):
    """{query: oracle (rows, dist)} at k; a shorter k is a prefix of it (the order is total)"""
    mid = MID[metric] if isinstance(metric, str) else metric
    which = list(range(qs.shape[0])) if which is None else list(which)
    got = _POOL.map(lambda i: O.exact_search(mid, rows, qs[i], k, alive=alive), which)
    return dict(zip(which, got))


def _cmp(got, want, k, ids=None, off=0):
    """got = (rows, dist, count) of a search over queries [off, off + nq) of `want`'s numbering"""
    r, d, c = got
    for j in range(r.shape[0]):
        if j + off not in want:
            continue
        er, ed = want[j + off]
        er, ed = er[:k], ed[:k]
        if ids is not None:
            er = ids[er]
        assert int(c[j]) == er.size, (j + off, k, int(c[j]), er.size)
        assert r[j, :er.size].tolist() == er.tolist(), (j + off, k)
        assert X.same(d[j, :er.size], ed), (j + off, k)


def _check(metric, rows, qs, got, k, which=None, alive=None, ids=None):
    _cmp(got, _want(metric, rows, qs, k, which, alive), k, ids)


def _equal(a, b):
    for i in range(a[0].shape[0]):
        n = int(a[2][i])
        assert n == int(b[2][i]), i
        assert a[0][i, :n].tolist() == b[0][i, :n].tolist(), i
        assert X.same(a[1][i, :n], b[1][i, :n]), i


def _exact(idx, qs, k, filt=None):
    """the exact multi-query scan of the same index; then the index's own filter again (`filt`: the one it was built with)"""
    idx.set_filter("off")
    try:
        return idx.search(qs, k)
    finally:
        idx.set_filter(filt if filt is not None else quiver_amd.DeviceIndex.default_filter)


# ------------------------------------------------------------------------------------------------ distance entry points ---
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [3, 64, 768])
def test_distance_pairs_and_rows_on_every_class(metric, dim):
    rng = np.random.default_rng(11 + dim)
    vecs = [X.unit(rng, dim)] + [v for _, _, v in X.class_rows(rng, dim)]
    a = np.stack([x for x in vecs for _ in vecs]); b = np.stack([y for _ in vecs for y in vecs])
    want = np.array([O.distance(MID[metric], x, y) for x, y in zip(a, b)], np.float32)
    assert X.same(distance_pairs(metric, a, b), want)
    idx = quiver_amd.DeviceIndex(dim, metric)
    rows = np.stack(vecs)
    idx.add(rows)
    for q in vecs:
        got = idx.distance_rows(q, np.arange(rows.shape[0], dtype=np.uint32))
        assert X.same(got, O.all_distances(MID[metric], rows, q))


# ------------------------------------------------------------------------------------------- short scans (split / small) ---
@pytest.mark.parametrize("n,dim", [(10_000, 128), (30_000, 768)])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot", "l1", "l2sq_f64", "l2sq"])
@pytest.mark.parametrize("regime", ["few", "many"])
def test_short_scans(metric, n, dim, regime):
    seed = 200 + dim + (7 if regime == "many" else 0)
    rows = _corpus(seed, n, dim, regime, O.gen_rows(seed + 1, 0, 4, dim))
    qs, _ = _queries(seed, rows, dim)
    idx = quiver_amd.DeviceIndex(dim, metric)
    idx.add(rows)
    want = _want(metric, rows, qs, 16)
    for k in (1, 10, 16):
        for i in range(qs.shape[0]):                                    # one query: k_flat_scan_split / the small scan
            _cmp(idx.search(qs[i], k), want, k, off=i)
        for j in range(0, qs.shape[0], 4):                              # four queries: k_flat_scan_split_mq
            _cmp(idx.search(qs[j:j + 4], k), want, k, off=j)
    idx.close()


# ------------------------------------------------------------------------------ long single-query scans, keys, radix ---
@pytest.fixture(scope="module")
def long_index():
    n, dim = 300_000, 64
    q0 = O.gen_rows(301, 0, 4, dim)
    rows = _corpus(300, n, dim, "many", q0)
    out = {}
    for metric in ("cosine", "l2sq"):
        idx = quiver_amd.DeviceIndex(dim, metric)
        idx.add(rows)
        out[metric] = idx
    return rows, out


@pytest.mark.parametrize("metric", ["cosine", "l2sq"])
def test_long_single_query_scans_keys_and_radix(long_index, metric):
    rows, idxs = long_index
    idx = idxs[metric]
    qs, flag = _queries(300, rows, rows.shape[1])
    n = rows.shape[0]
    want = _want(metric, rows, qs, 1000)
    for k in (10, 100, 1000):                                          # k_flat_scan, k_flat_scan_wide + selection, k_flat_keys + selection
        for i in range(qs.shape[0]):
            _cmp(idx.search(qs[i], k), want, k, off=i)
    full = [0, 5, 9, qs.shape[0] - 1]                                  # radix full ranking: every NaN row after every number, by row
    want = _want(metric, rows, qs, n, which=full)
    for i in full:
        _cmp(idx.search(qs[i], n), want, n, off=i)


# --------------------------------------------------------------------------------------- multi-query scans and mq64 ---
@pytest.fixture(scope="module")
def mq_rows():
    n, dim = 300_000, 32
    return _corpus(400, n, dim, "few", O.gen_rows(401, 0, 4, dim))


@pytest.mark.parametrize("metric", METRICS)
def test_multi_query_scans(mq_rows, metric):
    rows = mq_rows
    qs, _ = _queries(400, rows, rows.shape[1])
    idx = quiver_amd.DeviceIndex(rows.shape[1], metric)
    idx.add(rows)
    want = _want(metric, rows, qs, 10)
    for nq in (2, 5, 8):                                               # k_flat_scan_mq
        for j in range(0, qs.shape[0] - nq + 1, nq):
            _cmp(idx.search(qs[j:j + nq], 10), want, 10, off=j)
    idx.close()


@pytest.fixture(scope="module")
def mq64_rows():
    return _corpus(410, 1_000_000, 32, "few", O.gen_rows(411, 0, 4, 32))


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("k", [10, 64])
def test_mq64_scans(mq64_rows, metric, k):
    """the float64 multi-query matrix (cosine and dot only) with the filter off: 16+ queries in one call over a corpus long enough
    for it (16 tiles per workgroup of the scan's grid)"""
    rows = mq64_rows
    qs, _ = _queries(410, rows, rows.shape[1], n_ord=24)
    idx = quiver_amd.DeviceIndex(rows.shape[1], metric)
    idx.add(rows)
    idx.set_filter("off")
    got = idx.search(qs, k)
    _check(metric, rows, qs, got, k)
    _equal(tuple(x[:24] for x in got), idx.search(qs[:24], k))         # isolation: the 24 ordinary queries on their own
    idx.close()


# ------------------------------------------------------------------------------------------------------ batched filters ---
BATCHED = [   # (metric, n, dim, filter, bf16_rows)
    ("cosine", 40_000, 768, "auto", False),
    ("dot", 40_000, 768, "auto", True),
    ("l2", 40_000, 768, "fp32", False),
    ("cosine", 40_000, 768, "bf16x3", False),
    ("l2sq", 40_000, 768, "auto", False),
    ("cosine", 34_000, 2048, "auto", False),
    ("l2", 40_000, 200, "auto", False),
    ("dot", 40_000, 77, "auto", False),
]


@pytest.mark.parametrize("metric,n,dim,filt,bfr", BATCHED)
@pytest.mark.parametrize("regime", ["few", "many"])
def test_batched_filters(metric, n, dim, filt, bfr, regime):
    seed = 500 + dim + (7 if regime == "many" else 0)
    q0 = O.gen_rows(seed + 1, 0, 4, dim)
    rows = _corpus(seed, n, dim, regime, q0)
    qe, flag = _queries(seed, rows, dim, n_ord=2)
    idx = quiver_amd.DeviceIndex(dim, metric, bf16_rows=bfr, filter=filt)
    idx.add(rows)
    for nq in (64, 256):
        qo = O.gen_rows(seed + 2, 0, nq - qe.shape[0], dim)
        qs = np.concatenate([qe, qo])
        k = 10
        got = idx.search(qs, k)
        _equal(got, _exact(idx, qs, k, filt))
        which = list(np.nonzero(flag)[0]) + [0, 1]
        _check(metric, rows, qs, got, k, which=which)
        alone = idx.search(qo, k)                                       # isolation: the ordinary queries answer the same without the extreme ones
        _equal(tuple(x[qe.shape[0]:] for x in got), alone)
    idx.close()


# --------------------------------------------------------------------------------------- selection path and large k ---
@pytest.mark.parametrize("rowmajor", [False, True])
def test_selection_path_and_large_k(rowmajor):
    import torch
    n, dim, metric = 140_000, 64, "cosine"
    q0 = O.gen_rows(601, 0, 4, dim)
    rows = _corpus(600, n, dim, "many", q0)
    qe, flag = _queries(600, rows, dim, n_ord=2)
    qs = np.concatenate([qe, O.gen_rows(602, 0, 64 - qe.shape[0], dim)])
    idx = quiver_amd.DeviceIndex(dim, metric, rowmajor=rowmajor)
    idx.add(rows)
    want = _want(metric, rows, qs, 4096, which=list(np.nonzero(flag)[0]) + [0, 1])
    for k in (16, 64, 100, 1000, 4096):
        got = idx.search(qs, k)
        _equal(got, _exact(idx, qs, k))
        _cmp(got, want, k)
        if k in (64, 1000):                                             # isolation: the ordinary queries without the extreme ones
            _equal(tuple(x[qe.shape[0]:] for x in got), idx.search(qs[qe.shape[0]:], k))
    k = 64                                                              # the device form: flagged queries redone by the host form
    dq = torch.from_numpy(qs).cuda()
    dr = torch.empty((64, k), dtype=torch.int32, device="cuda"); dd = torch.empty((64, k), dtype=torch.float32, device="cuda")
    fl = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    idx.search_batched_device(dq.data_ptr(), 64, k, dr.data_ptr(), dd.data_ptr(), fl.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    f = fl.cpu().numpy(); r = dr.cpu().numpy().view(np.uint32); d = dd.cpu().numpy()
    ex = _exact(idx, qs, k)
    for i in range(64):
        if f[i]:
            one = idx.search(qs[i], k)
            _check(metric, rows, qs[i:i + 1], one, k)
        else:
            assert r[i].tolist() == ex[0][i].tolist() and X.same(d[i], ex[1][i]), i


# ---------------------------------------------------------------------------------------------------- masked, negative ---
def test_masked_search_with_mostly_nan_rows_live():
    n, dim, metric = 50_000, 48, "l2"
    rows = _corpus(700, n, dim, "many", O.gen_rows(701, 0, 4, dim))
    idx = quiver_amd.DeviceIndex(dim, metric)
    idx.add(rows)
    rng = np.random.default_rng(702)
    nanrow = np.isnan(rows).any(axis=1)
    mask = nanrow.copy()
    mask[rng.choice(np.nonzero(~nanrow)[0], size=5, replace=False)] = True     # 5 finite rows live: k above them
    qs, _ = _queries(700, rows, dim)
    assert np.isfinite(qs[-5:]).all()                                   # the G queries are finite
    want = _want(metric, rows, qs, 500, alive=mask.astype(np.uint8))
    for k in (3, 10, 64, 500):
        for nq in (1, 4, 12):
            for j in range(0, qs.shape[0], nq):
                _cmp(idx.search_masked(qs[j:j + nq], k, mask), want, k, off=j)


@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_negative_example_distances(metric):
    """qv_index_search_negative: the top k_fetch rows and each row's distance to the negative example, for I, O, G and Z negatives"""
    n, dim, kf = 20_000, 64, 40
    rows = _corpus(800, n, dim, "few", O.gen_rows(801, 0, 4, dim))
    idx = quiver_amd.DeviceIndex(dim, metric)
    idx.add(rows)
    rng = np.random.default_rng(802)
    qs, _ = _queries(800, rows, dim)
    negs = [v for c, _, v in X.class_rows(rng, dim) if c in "IOGZ"]
    which = list(range(0, qs.shape[0], 3))
    want = _want(metric, rows, qs, kf, which=which)
    for i in which:
        er, ed = want[i]
        for neg in negs:
            r, d, nd, c = idx.search_negative(qs[i], neg, kf)
            assert c == er.size and r[:c].tolist() == er.tolist() and X.same(d[:c], ed), i
            assert X.same(nd[:c], O.all_distances(MID[metric], rows[er], neg)), i


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_negative_example_rerank_with_extreme_negatives(metric):
    """the product's re-rank (HybridIndex, score = d - w d_neg in float32, order (score, id); hybrid_index.go:517-570) with I, O, G
    and Z negatives over a corpus holding G and Z rows, against the oracle's re-rank.  Only cases where no score of the retrieved rows
    is NaN (a NaN score is out of contract); the test asserts that enough cases remain."""
    from quiver_amd import hybrid
    n, dim = 3000, 24
    mid = MID["l2" if metric == "euclidean" else metric]
    rng = np.random.default_rng(850)
    rows = O.gen_rows(851, 0, n, dim)
    ext = [v for c, _, v in X.class_rows(rng, dim, per_class=2) if c in "GZ"]
    for p, v in zip(rng.choice(n, size=len(ext), replace=False), ext):
        rows[p] = v
    ids = [f"v{i}" for i in range(n)]
    cfg = hybrid.IndexConfig(DistanceFunc=metric, ExplorationFactor=0.0, Seed=3)
    idx = hybrid.HybridIndex(cfg)
    idx.InsertBatch({i: r for i, r in zip(ids, rows)})
    order = sorted(range(n), key=lambda i: ids[i])
    rank = np.empty(n, np.uint32); rank[order] = np.arange(n, dtype=np.uint32)
    qs = np.concatenate([O.gen_rows(852, 0, 3, dim), np.stack([X.scaled(O.gen_rows(851, 0, 6, dim)[5], g) for g in (1e18, 1e30)])])
    negs = [v for c, _, v in X.class_rows(rng, dim) if c in "IOGZ"]
    done = 0
    for q in qs:
        for neg in negs:
            for k, w in ((5, 0.5), (20, 0.9)):
                er, ed = O.exact_search(mid, rows, q, max(2 * k, 30))
                with np.errstate(all="ignore"):
                    score = ed - np.float32(w) * O.all_distances(mid, rows[er], neg)
                if np.isnan(score).any():
                    continue
                res = idx.SearchWithRequest(hybrid.HybridSearchRequest(Query=q, K=k, NegativeExample=neg, NegativeWeight=w,
                                                                      ForceStrategy="exact")).Results
                wr, wd = O.exact_search_negative(mid, rows, q, neg, w, k, id_rank=rank)
                assert [r.ID for r in res] == [ids[i] for i in wr], (k, w)
                assert X.same(np.array([r.Distance for r in res], np.float32), wd), (k, w)
                done += 1
    assert done >= 40, done


# -------------------------------------------------------------------------------------------------------- HNSW traversal ---
@pytest.fixture(scope="module")
def graphs():
    n, dim, m = 1400, 64, 16
    out = {}
    for metric in ("cosine", "l2", "cosine_f32", "dot_f32"):
        rows = O.gen_rows(9090, 0, n, dim)
        idx = quiver_amd.DeviceIndex(dim, metric, rowmajor=True)
        idx.add(rows)
        nbr, _, _ = idx.search(rows, m + 1)
        links = np.zeros((n, m), np.uint32); deg = np.zeros(n, np.uint32)
        for i in range(n):
            l = [int(x) for x in nbr[i] if int(x) != i][:m]
            deg[i] = len(l); links[i, :len(l)] = l
        rng = np.random.default_rng(9091)
        ext = [v for _, _, v in X.class_rows(rng, dim)]
        for p, v in zip(rng.choice(np.arange(20, n), size=len(ext), replace=False), ext):
            idx.update(int(p), v); rows[p] = v
        g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=11)
        out[metric] = (idx, g, rows, deg, links)
    return out


@pytest.mark.parametrize("metric", ["cosine", "l2", "cosine_f32", "dot_f32"])
def test_graph_traversal_forms(graphs, metric):
    import torch
    idx, g, rows, deg, links = graphs[metric]
    dim, k, ef = rows.shape[1], 10, 64
    qe, flag = _queries(9100, rows, dim, n_ord=2)
    o = O.HNSW(MID[metric], dim, M=8, maxM0=16, efSearch=ef, maxLevel=1, seed=1)
    o.load_flat(rows, deg, links, 11)
    qo = O.gen_rows(9101, 0, 800, dim)
    for qs in (np.concatenate([qe, qo]), np.concatenate([qe, qo[:48 - qe.shape[0]]])):   # wave form (> 768), workgroup form (<= 256)
        r, d, c, ev = g.search(qs, k, ef, with_evals=True)
        for i in list(range(qe.shape[0])) + [qe.shape[0], qs.shape[0] - 1]:
            ro, do, eo = o.search(qs[i], k, with_evals=True)
            assert int(c[i]) == ro.size, (i, int(c[i]), ro.size)
            assert r[i, :ro.size].tolist() == ro.tolist(), i
            assert X.same(d[i, :ro.size], do), i
            assert int(ev[i]) == eo - 1, i
        alone = g.search(qs[qe.shape[0]:], k, ef, with_evals=True)      # isolation
        for a, b in zip((r, d, c, ev), alone):
            assert a[qe.shape[0]:].tobytes() == b.tobytes()
    qs = np.concatenate([qe, qo[:100]])
    nq = qs.shape[0]
    dq = torch.from_numpy(qs).cuda()
    dr = torch.empty((nq, k), dtype=torch.int32, device="cuda"); dd = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    dc = torch.empty(nq, dtype=torch.int32, device="cuda"); de = torch.empty(nq, dtype=torch.int32, device="cuda")
    g.search_device(dq.data_ptr(), nq, k, ef, dr.data_ptr(), dd.data_ptr(), dc.data_ptr(), de.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    c2 = dc.cpu().numpy().view(np.uint32)
    host = g.search(qs, k, ef, with_evals=True)
    nanq = np.isnan(qs).any(axis=1)
    assert (c2[nanq] == 0xFFFFFFFE).all(), c2[nanq]
    for i in range(nq):
        if c2[i] == 0xFFFFFFFE:
            ro, do, eo = o.search(qs[i], k, with_evals=True)
            assert host[0][i, :ro.size].tolist() == ro.tolist() and X.same(host[1][i, :ro.size], do) and int(host[3][i]) == eo - 1, i
        else:
            assert c2[i] == host[2][i] and dr.cpu().numpy()[i].view(np.uint32).tolist() == host[0][i].tolist(), i
            assert X.same(dd.cpu().numpy()[i], host[1][i]), i


# --------------------------------------------------------------------------------------------------------------- sharded ---
def test_sharded_with_extreme_rows_on_shard_boundaries():
    n, dim, metric = 60_000, 64, "l2"
    rows = _corpus(1000, n, dim, "few", O.gen_rows(1001, 0, 4, dim))
    rng = np.random.default_rng(1002)
    ext = [v for _, _, v in X.class_rows(rng, dim)]
    sh = quiver_amd.ShardedIndex(dim, metric, devices=[0] * 3, peer_copy=True)
    for b in (n // 3, 2 * n // 3):                                       # the rows either side of each boundary
        for j, p in enumerate(range(b - 3, b + 3)):
            rows[p] = ext[(j + b) % len(ext)]
    ids = sh.add(rows)
    qs, _ = _queries(1000, rows, dim)
    for k in (10, 100, 2000):
        _check(metric, rows, qs, sh.search(qs, k), k, ids=ids)
    sel = np.nonzero(np.isnan(rows).any(axis=1) | (np.arange(n) % 97 == 0))[0]
    alive = np.zeros(n, np.uint8); alive[sel] = 1
    _check(metric, rows, qs, sh.search_masked(qs, 50, ids[sel]), 50, alive=alive, ids=ids)
    sh.close()


# ------------------------------------------------------------------------------------------------------ coalesced callers ---
def test_coalesced_callers_with_extreme_queries():
    from tests import _callers
    n, dim, metric, k = 50_000, 64, "cosine", 10
    rows = _corpus(1100, n, dim, "few", O.gen_rows(1101, 0, 4, dim))
    idx = quiver_amd.DeviceIndex(dim, metric)
    idx.add(rows)
    qe, flag = _queries(1100, rows, dim, n_ord=2)
    qs = np.concatenate([qe, O.gen_rows(1102, 0, 16, dim)])
    res = _callers.run("index", idx.handle, qs, k, threads=16, seconds=20.0, max_calls_per_thread=8)
    assert res["rc"] == 0 and res["errors"] == 0 and res["mismatches"] == 0, res["error"]
    seen = [i for i in range(qs.shape[0]) if res["count"][i] != 0xFFFFFFFD]
    assert len(seen) == qs.shape[0]
    _check(metric, rows, qs, (res["rows"], res["dist"], res["count"]), k)
    idx.close()


def test_coalesced_graph_callers_with_extreme_queries(graphs):
    from tests import _callers
    idx, g, rows, deg, links = graphs["cosine"]
    dim, k, ef = rows.shape[1], 10, 64
    qe, _ = _queries(9200, rows, dim, n_ord=2)
    qs = np.concatenate([qe, O.gen_rows(9201, 0, 16, dim)])
    res = _callers.run("graph", g.handle, qs, k, threads=16, seconds=20.0, max_calls_per_thread=8, ef=ef)
    assert res["rc"] == 0 and res["errors"] == 0 and res["mismatches"] == 0, res["error"]
    o = O.HNSW(MID["cosine"], dim, M=8, maxM0=16, efSearch=ef, maxLevel=1, seed=1)
    o.load_flat(rows, deg, links, 11)
    for i in range(qs.shape[0]):
        ro, do = o.search(qs[i], k)
        assert int(res["count"][i]) == ro.size and res["rows"][i, :ro.size].tolist() == ro.tolist(), i
        assert X.same(res["dist"][i, :ro.size], do), i


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2sq", "l2"])
def test_batched_filter_queries_above_the_norm_guard(metric):
    """every row large but below the row guard (norm 1e10) and queries on both sides of the query guard (k_mfma_prep): q . r reaches
    1e40, past float32, only for the queries the guard gives up on"""
    n, dim, k = 40_000, 128, 10
    rows = (O.gen_rows(1200, 0, n, dim).astype(np.float64) * 1e10).astype(np.float32)
    base = O.gen_rows(1201, 0, 64, dim)
    norms = [1e17, 0.5e18, 0.999e18, 1.001e18, 2e18, 1e19, 1e24, 1e30]
    qs = base.copy()
    for j, g in enumerate(norms):
        qs[j] = X.scaled(base[j], g)
        qs[len(norms) + j] = X.scaled(rows[100 * j] / np.float32(1e10), g)     # a scaled copy of a row
    idx = quiver_amd.DeviceIndex(dim, metric)
    idx.add(rows)
    got = idx.search(qs, k)
    _equal(got, _exact(idx, qs, k))
    _check(metric, rows, qs, got, k, which=list(range(2 * len(norms) + 2)))
