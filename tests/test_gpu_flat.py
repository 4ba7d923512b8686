"""GPU parity tests proper: the HIP path, called through the C ABI (libqv.so), against
the CPU oracle on the same seeded inputs.  Bar: identical top-k rows in identical
order and BIT-IDENTICAL float32 distances (the kernels walk each row in the
reference's element order and precision, so there is nothing to tolerate)."""
import json
import os
import threading

import numpy as np
import pytest

from tests import _oracle as O

pytestmark = pytest.mark.gpu

KATS = json.load(open(os.path.join(O.ROOT, "tests", "golden", "ref_kats.json")))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mk(dim, metric, rows=None, **kw):
    import quiver_amd as q
    idx = q.DeviceIndex(dim, metric, **kw)
    if rows is not None and len(rows):
        idx.add(rows)
    return idx


# ---------------------------------------------------------------- reference KATs ---

@pytest.mark.parametrize("kat", KATS["distance"], ids=lambda k: k["src"])
def test_distance_kats_through_abi(kat):
    from quiver_amd.device_index import distance_pairs
    got = distance_pairs(kat["metric"], kat["a"], kat["b"])[0]
    assert abs(float(got) - kat["want"]) <= kat["tol"]
    assert _bits(got) == _bits(O.distance(kat["metric"], kat["a"], kat["b"]))


@pytest.mark.parametrize("kat", KATS["exact_search"], ids=lambda k: k["src"])
def test_exact_search_kats_through_abi(kat):
    rows = np.array(kat["rows"], dtype=np.float32)
    idx = _mk(rows.shape[1], kat["metric"], rows)
    r, d, c = idx.search(kat["query"], kat["k"])
    n = int(c[0])
    assert n == min(kat["k"], len(rows))
    ids = [kat["ids"][i] for i in r[0, :n]]
    if kat["exact_order"]:
        assert ids[: len(kat["want_ids"])] == kat["want_ids"]
    else:
        assert set(kat["want_ids"]) <= set(ids)
    assert all(d[0, i] <= d[0, i + 1] for i in range(n - 1))
    er, ed = O.exact_search(kat["metric"], rows, kat["query"], kat["k"])
    assert np.array_equal(r[0, :n], er) and np.array_equal(_bits(d[0, :n]), _bits(ed))
    assert np.all(r[0, n:] == 0xFFFFFFFF) and np.all(np.isinf(d[0, n:]))


def test_empty_index_and_k_errors():
    import quiver_amd as q
    idx = _mk(3, "cosine")
    r, d, c = idx.search([1, 0, 0], 5)            # exact.go:96-98
    assert c[0] == 0
    r, d, c = idx.search([1, 0, 0], 0)            # empty wins over k<=0 (check order exact.go:96-106)
    assert c[0] == 0
    idx.add([[1, 0, 0]])
    with pytest.raises(q.QvError) as e:
        idx.search([1, 0, 0], 0)
    assert str(e.value) == "k must be positive" and e.value.code == -3
    with pytest.raises(ValueError) as e2:
        idx.search([1, 0], 1)
    assert str(e2.value) == "query dimension mismatch: expected 3, got 2"
    with pytest.raises(ValueError) as e3:
        idx.add([[1, 0]])
    assert str(e3.value) == "vector dimension mismatch: expected 3, got 2"


# ---------------------------------------------------------------- bit-exact parity ---

@pytest.mark.parametrize("metric", range(9))
@pytest.mark.parametrize("dim", [1, 3, 4, 7, 63, 64, 128, 200, 768])
def test_topk_bitexact_vs_oracle(metric, dim):
    rng = np.random.default_rng(100 * metric + dim)
    n = 1500
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    rows[5] = 0.0
    rows[6] = rows[7]
    qs = rng.standard_normal((4, dim)).astype(np.float32)
    rows[8] = qs[0]
    rows[9] = -qs[0]
    idx = _mk(dim, metric, rows)
    for k in (1, 10, 64):
        r, d, c = idx.search(qs, k)
        for qi in range(4):
            er, ed = O.exact_search(metric, rows, qs[qi], k)
            assert int(c[qi]) == len(er)
            assert np.array_equal(r[qi], er), (metric, dim, k, qi)
            assert np.array_equal(_bits(d[qi]), _bits(ed)), (metric, dim, k, qi)


@pytest.mark.parametrize("metric", range(9))
def test_all_distances_bitexact_via_distance_rows(metric):
    rng = np.random.default_rng(metric)
    rows = (rng.standard_normal((777, 96)) * rng.choice([1e-3, 1, 1e3], size=(777, 1))).astype(np.float32)
    q = rng.standard_normal(96).astype(np.float32)
    idx = _mk(96, metric, rows)
    ids = rng.permutation(777).astype(np.uint32)
    got = idx.distance_rows(q, ids)
    want = O.all_distances(metric, rows, q)[ids]
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("metric", [0, 1, 2, 3, 4, 5, 6, 7, 8])
def test_ties_and_tombstones(metric):
    rng = np.random.default_rng(7 + metric)
    rows = rng.integers(-2, 3, size=(3000, 4)).astype(np.float32)      # few distinct distances: ties everywhere
    q = np.array([1, 0, -1, 2], np.float32)
    idx = _mk(4, metric, rows)
    dead = np.nonzero(rng.random(3000) < 0.3)[0].astype(np.uint32)
    idx.remove(dead)
    idx.remove(dead[:10])                                              # removing twice is not an error (exact.go:61-70)
    alive = np.ones(3000, bool)
    alive[dead] = False
    assert idx.size() == int(alive.sum()) and idx.rows() == 3000
    for k in (1, 7, 64, 65, 500, 5000):
        r, d, c = idx.search(q, k)
        er, ed = O.exact_search(metric, rows, q, k, alive=alive)
        assert int(c[0]) == len(er) == min(k, int(alive.sum()))
        assert np.array_equal(r[0, : len(er)], er), (metric, k)       # ties resolved by row ascending
        assert np.array_equal(_bits(d[0, : len(er)]), _bits(ed))


def test_full_ranking_k_equals_n():                                    # collection.go:679-682: filters ask for k = Index.Size()
    rows = O.gen_rows(5, 0, 20000, 32)
    q = O.gen_rows(6, 0, 1, 32)[0]
    idx = _mk(32, "cosine", rows)
    r, d, c = idx.search(q, 20000)
    er, ed = O.exact_search(0, rows, q, 20000)
    assert int(c[0]) == 20000
    assert np.array_equal(r[0], er) and np.array_equal(_bits(d[0]), _bits(ed))


def test_update_and_revive():
    rows = O.gen_rows(9, 0, 300, 16)
    idx = _mk(16, "euclidean", rows)
    new = O.gen_rows(10, 0, 1, 16)[0]
    idx.remove([17])
    idx.update(17, new)                                                # Update = delete + insert in place
    idx.update(200, new * 2)
    rows2 = rows.copy()
    rows2[17] = new
    rows2[200] = new * 2
    assert idx.size() == 300
    assert np.array_equal(idx.get_row(17), new)
    r, d, c = idx.search(new, 5)
    er, ed = O.exact_search(1, rows2, new, 5)
    assert np.array_equal(r[0], er) and np.array_equal(_bits(d[0]), _bits(ed))
    assert r[0, 0] == 17 and d[0, 0] == 0.0


def test_copy_on_insert():                                             # exact_test.go:46-60
    v = np.array([[1.0, 2.0, 3.0]], np.float32)
    idx = _mk(3, "euclidean", v)
    v[0, 0] = 99.0
    assert np.array_equal(idx.get_row(0), np.array([1, 2, 3], np.float32))


def test_incremental_adds_cross_tile_boundaries():
    rows = O.gen_rows(13, 0, 1000, 24)
    idx = _mk(24, "cosine")
    pos = 0
    for step in (1, 62, 1, 1, 63, 200, 5, 667):
        first = idx.add(rows[pos: pos + step])
        assert first == pos
        pos += step
    assert pos == 1000 and idx.size() == 1000
    q = O.gen_rows(14, 0, 3, 24)
    r, d, c = idx.search(q, 10)
    for i in range(3):
        er, ed = O.exact_search(0, rows, q[i], 10)
        assert np.array_equal(r[i], er) and np.array_equal(_bits(d[i]), _bits(ed))


def test_synthetic_generator_matches_oracle_bitwise():
    idx = _mk(768, "cosine")
    idx.add_synthetic(20260424, 1000, 200)
    want = O.gen_rows(20260424, 1000, 200, 768)
    for r in (0, 1, 63, 64, 65, 199):
        assert np.array_equal(_bits(idx.get_row(r)), _bits(want[r])), r
    idx2 = _mk(100, "hnsw_cosine")
    idx2.add_synthetic(7, 0, 130)
    want2 = O.gen_rows(7, 0, 130, 100)
    for r in (0, 64, 129):
        assert np.array_equal(_bits(idx2.get_row(r)), _bits(want2[r]))
    q = O.gen_rows(8, 0, 1, 100)[0]
    r, d, c = idx2.search(q, 10)
    er, ed = O.exact_search(5, want2, q, 10)
    assert np.array_equal(r[0], er) and np.array_equal(_bits(d[0]), _bits(ed))


def test_config0_hybrid_exact_10kx128_cosine_k10_against_golden():
    """BASELINE.json configs[0]; golden fixture = oracle output committed under tests/golden"""
    g = np.load(os.path.join(O.ROOT, "tests", "golden", "flat_10kx128_cosine.npz"))
    rows = O.gen_rows(int(g["corpus_seed"]), 0, 10000, 128)
    qs = O.gen_rows(int(g["query_seed"]), 0, g["rows"].shape[0], 128)
    idx = _mk(128, "cosine", rows)
    r, d, c = idx.search(qs, 10)
    assert np.array_equal(r, g["rows"])
    assert np.array_equal(_bits(d), _bits(g["dist"]))


def test_concurrent_searches_are_independent():                        # Collection.Search runs under RLock: many at once
    rows = O.gen_rows(21, 0, 5000, 64)
    idx = _mk(64, "cosine", rows)
    qs = O.gen_rows(22, 0, 16, 64)
    want = [O.exact_search(0, rows, q, 10) for q in qs]
    errs = []

    def work(i):
        try:
            for _ in range(5):
                r, d, c = idx.search(qs[i], 10)
                assert np.array_equal(r[0], want[i][0]) and np.array_equal(_bits(d[0]), _bits(want[i][1]))
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(16)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs[0]


def test_device_pointer_entry_point_matches_host_entry_point():
    import torch
    rows = O.gen_rows(31, 0, 4000, 48)
    idx = _mk(48, "dot_product", rows)
    qs = O.gen_rows(32, 0, 5, 48)
    dq = torch.from_numpy(qs).cuda()
    dr = torch.empty((5, 10), dtype=torch.int32, device="cuda")
    dd = torch.empty((5, 10), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    idx.search_device(dq.data_ptr(), 5, 10, dr.data_ptr(), dd.data_ptr(), s)
    torch.cuda.synchronize()
    r, d, c = idx.search(qs, 10)
    assert np.array_equal(dr.cpu().numpy().view(np.uint32), r)
    assert np.array_equal(_bits(dd.cpu().numpy()), _bits(d))


# ---------------------------------------------------------------- full-size checks ---

def test_config1_flat_cosine_1Mx768_k10_full_oracle_and_properties():
    """BASELINE.json configs[1] at full size.  Three queries against the complete CPU
    oracle (bit-exact), plus size-independent properties: planted neighbours come back
    first at distance ~0, results are sorted, and every returned distance equals the
    oracle's distance for that row."""
    n, dim, seed = 1_000_000, 768, 20260424
    idx = _mk(dim, "cosine")
    idx.reserve(n)
    idx.add_synthetic(seed, 0, n)
    assert idx.size() == n
    qs = O.gen_rows(20260425, 0, 3, dim)
    r, d, c = idx.search(qs, 10)
    corpus = O.gen_rows(seed, 0, n, dim)          # ~3 GB host, a few seconds
    for i in range(3):
        er, ed = O.exact_search(0, corpus, qs[i], 10)
        assert np.array_equal(r[i], er)
        assert np.array_equal(_bits(d[i]), _bits(ed))
    # planted neighbours: the query IS a corpus row
    for row in (0, 63, 64, 123_457, 999_999):
        rr, dd, _ = idx.search(corpus[row], 10)
        assert rr[0, 0] == row and dd[0, 0] <= 1e-6
        assert all(dd[0, j] <= dd[0, j + 1] for j in range(9))
        for j in range(10):
            assert _bits(dd[0, j]) == _bits(O.distance(0, corpus[row], corpus[rr[0, j]]))
    # tombstone the best hit: it must disappear, everything else shifts up
    idx.remove([int(r[0, 0])])
    r2, d2, _ = idx.search(qs[0], 9)
    assert np.array_equal(r2[0], r[0, 1:]) and np.array_equal(_bits(d2[0]), _bits(d[0, 1:]))


def test_config4_flat_cosine_10Mx768_one_query_against_the_full_cpu_oracle():
    """BASELINE.json configs[4] corpus on ONE GPU: the returned 10 rows are THE top-10 of all 10M — one query, the CPU
    oracle's scalar arithmetic over every row (regenerated chunk by chunk on host threads), rows and float32 bits equal"""
    import os
    from tests._par import exact_topk_synthetic
    n, dim, seed = 10_000_000, 768, 20260424
    idx = _mk(dim, "cosine")
    idx.reserve(n)
    for s in range(0, n, 2_000_000):
        idx.add_synthetic(seed, s, 2_000_000)
    q = O.gen_rows(20260425, 7, 1, dim)[0]
    r, d, c = idx.search(q, 10)
    er, ed = exact_topk_synthetic(0, seed, n, dim, q, 10, chunk=100_000, workers=min(32, os.cpu_count() or 8))
    assert c[0] == 10 and np.array_equal(r[0], er) and np.array_equal(_bits(d[0]), _bits(ed))


def test_config4_flat_cosine_10Mx768_single_gpu_properties():
    """BASELINE.json configs[4] corpus on ONE GPU (30.8 GB): size-independent properties —
    planted neighbours come back first at distance ~0, results are sorted, every returned
    distance equals the oracle's distance for that (regenerated) row bit for bit, a 1M-row
    prefix searched separately agrees with the oracle-checked configs[1] result, and
    sharding the same corpus in two gives the same top-k after the (distance,row) merge."""
    n, dim, seed = 10_000_000, 768, 20260424
    idx = _mk(dim, "cosine")
    idx.reserve(n)
    for s in range(0, n, 2_000_000):
        idx.add_synthetic(seed, s, 2_000_000)
    assert idx.size() == n
    qs = O.gen_rows(20260425, 0, 4, dim)
    r, d, c = idx.search(qs, 10)
    for i in range(4):
        assert all(d[i, j] <= d[i, j + 1] for j in range(9))
        for j in range(10):
            assert _bits(d[i, j]) == _bits(O.distance(0, qs[i], O.gen_rows(seed, int(r[i, j]), 1, dim)[0]))
    for row in (0, 4_999_999, 9_999_999):
        q = O.gen_rows(seed, row, 1, dim)[0]
        rr, dd, _ = idx.search(q, 3)
        assert rr[0, 0] == row and dd[0, 0] <= 1e-6
    # two shards + merge == one index (the multi-GPU exchange, on one device)
    a, b = _mk(dim, "cosine"), _mk(dim, "cosine")
    a.add_synthetic(seed, 0, 600_000)
    b.add_synthetic(seed, 600_000, 400_000)
    one = _mk(dim, "cosine")
    one.add_synthetic(seed, 0, 1_000_000)
    ra, da, _ = a.search(qs[0], 10)
    rb, db, _ = b.search(qs[0], 10)
    r1, d1, _ = one.search(qs[0], 10)
    import torch
    from quiver_amd.device_index import merge_topk_device
    gd = torch.from_numpy(np.stack([da[0], db[0]])).cuda()
    gr = torch.from_numpy(np.stack([ra[0], rb[0] + 600_000]).view(np.int32)).cuda()
    orow = torch.empty(10, dtype=torch.int32, device="cuda"); odist = torch.empty(10, dtype=torch.float32, device="cuda")
    merge_topk_device(gd.data_ptr(), gr.data_ptr(), 2, 10, orow.data_ptr(), odist.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(orow.cpu().numpy().view(np.uint32), r1[0]) and np.array_equal(_bits(odist.cpu().numpy()), _bits(d1[0]))
    # the packed form of the same merge: per shard [k local rows][k distance bits], bases added by the merge
    from quiver_amd.device_index import merge_topk_shards_device
    pack = np.stack([np.stack([ra[0].view(np.int32), da[0].view(np.int32)]), np.stack([rb[0].view(np.int32), db[0].view(np.int32)])])
    gp = torch.from_numpy(pack).cuda(); bases = torch.tensor([0, 600_000], dtype=torch.int32, device="cuda")
    merge_topk_shards_device(gp.data_ptr(), bases.data_ptr(), 2, 1, 10, orow.data_ptr(), odist.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(orow.cpu().numpy().view(np.uint32), r1[0]) and np.array_equal(_bits(odist.cpu().numpy()), _bits(d1[0]))


@pytest.mark.parametrize("dim", [1536, 4096, 8192, 16384])
def test_large_dimensions_use_more_lds(dim):
    """the query is staged in LDS (float64 for cosine: 8*dim bytes, up to 128 KiB of the CU's 160 KiB)"""
    rows = O.gen_rows(77, 0, 300, dim)
    qs = O.gen_rows(78, 0, 3, dim)
    for metric in (0, 1):
        idx = _mk(dim, metric, rows)
        r, d, c = idx.search(qs, 5)                       # multi-query path (scalar-operand query block)
        r1, d1, c1 = idx.search(qs[0], 5)                 # single-query path (LDS-staged query)
        er, ed = O.exact_search(metric, rows, qs[0], 5)
        assert np.array_equal(r[0], er) and np.array_equal(_bits(d[0]), _bits(ed))
        assert np.array_equal(r1[0], er) and np.array_equal(_bits(d1[0]), _bits(ed))
        got = idx.distance_rows(qs[1], np.arange(300, dtype=np.uint32))
        assert np.array_equal(_bits(got), _bits(O.all_distances(metric, rows, qs[1])))


def test_dimension_above_the_supported_maximum_is_refused():
    import quiver_amd as q
    with pytest.raises(q.QvError) as e:
        q.DeviceIndex(16385, "cosine")
    assert e.value.code == -8


@pytest.mark.parametrize("metric", [0, 1, 3, 4])
def test_nan_and_inf_inputs_sort_last_like_the_oracle(metric):
    """NaN/Inf are not pinned by the reference; declared behaviour: a NaN distance
    sorts after every number (ties among NaNs by row), +Inf sorts after finite values"""
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((500, 16)).astype(np.float32)
    rows[10, 3] = np.nan
    rows[20, 0] = np.inf
    rows[30, 5] = -np.inf
    rows[40] = 0.0
    q = rng.standard_normal(16).astype(np.float32)
    idx = _mk(16, metric, rows)
    for k in (5, 64, 500):
        r, d, c = idx.search(q, k)
        er, ed = O.exact_search(metric, rows, q, k)
        assert np.array_equal(r[0], er), (metric, k)
        assert np.array_equal(np.isnan(d[0]), np.isnan(ed))
        fin = ~np.isnan(ed)
        assert np.array_equal(_bits(d[0][fin]), _bits(ed[fin]))
    rq = rows[10]                                           # a NaN query: every distance NaN -> row order
    r, d, c = idx.search(rq, 7)
    if metric in (0, 1, 3, 4):
        er, ed = O.exact_search(metric, rows, rq, 7)
        assert np.array_equal(r[0], er) and np.isnan(d[0]).all() == np.isnan(ed).all()


def test_very_large_host_batch_is_sliced_without_changing_results():
    """host-pointer entry points bound their workspace by slicing batches of more than 8192 queries"""
    n, dim, k, nq = 3000, 16, 5, 8192 + 37
    rows = O.gen_rows(31337, 0, n, dim)
    qs = O.gen_rows(31338, 0, nq, dim)
    import quiver_amd
    idx = quiver_amd.DeviceIndex(dim, "cosine")
    idx.add(rows)
    r, d, c = idx.search(qs, k)
    assert (c == k).all()
    for i in list(range(0, 40)) + [8191, 8192, 8193, nq - 1]:
        ro, do = O.exact_search(0, rows, qs[i], k)
        assert r[i].tolist() == ro.tolist() and d[i].tobytes() == do.tobytes()
    r2, d2, _ = idx.search(qs, k, batched=True)
    assert np.array_equal(r, r2) and np.array_equal(d.view(np.uint32), d2.view(np.uint32))
    # the filtered host forms: a filter per query drawn from four (the masked form takes one for all), against the same call made in two
    # halves of at most 8192 queries each, and against the oracle at the ends of the slices
    n, nq = 200, 8192 + 5
    rows, qs = O.gen_rows(31339, 0, n, dim), O.gen_rows(31340, 0, nq, dim)
    idx = quiver_amd.DeviceIndex(dim, "cosine")
    idx.add(rows)
    masks = [np.arange(n) % 4 != j for j in range(4)]
    pick = np.arange(nq) % 4
    sets = [idx.rowset(m) for m in masks]
    col = idx.column("u32")
    col.set(0, np.arange(n) % 4)
    forms = {
        "masked": (lambda a, b: idx.search_masked(qs[a:b], k, masks[1]), lambda i: masks[1]),
        "rowsets": (lambda a, b: idx.search_rowsets(qs[a:b], k, [sets[j] for j in pick[a:b]]), lambda i: masks[pick[i]]),
        "where": (lambda a, b: idx.search_where(qs[a:b], k, [[(col, "!=", int(j))] for j in pick[a:b]]), lambda i: masks[pick[i]]),
    }
    for form, (call, mask_of) in forms.items():
        r, d, c = call(0, nq)
        assert (c == k).all(), form
        halves = [call(0, 4100), call(4100, nq)]
        assert np.array_equal(r, np.concatenate([h[0] for h in halves])), form
        assert np.array_equal(_bits(d), _bits(np.concatenate([h[1] for h in halves]))), form
        for i in (0, 8191, 8192, nq - 1):
            ro, do = O.exact_search(0, rows, qs[i], k, alive=mask_of(i).astype(np.uint8))
            assert r[i].tolist() == ro.tolist() and d[i].tobytes() == do.tobytes(), (form, i)


@pytest.mark.parametrize("metric,n,dim,nq,k,frac", [
    ("cosine", 5000, 48, 1, 10, 0.3),        # single-query scan
    ("l2", 5000, 20, 6, 64, 0.5),            # multi-query scan, full-width lists
    ("cosine", 3000, 16, 3, 500, 0.4),       # k > 64: full ranking of the selected rows
    ("dot", 2000, 33, 2, 50, 0.01),          # fewer matches than k
    ("cosine", 530_000, 16, 12, 10, 0.2),    # long scan, >= 9 queries: the f64-matrix kernel with a row bitmap
])
def test_masked_search_equals_oracle_over_selected_rows(metric, n, dim, nq, k, frac):
    """qv_index_search_masked = the first k of the full ranking that pass the filter (collection.go:679-759)"""
    import quiver_amd
    mid = quiver_amd.metric_id(metric)
    rows = O.gen_rows(4711, 0, n, dim)
    idx = quiver_amd.DeviceIndex(dim, metric)
    idx.add(rows)
    dead = np.arange(5, n, 97, dtype=np.uint32)
    idx.remove(dead)
    alive = np.ones(n, np.uint8); alive[dead] = 0
    rng = np.random.default_rng(12)
    mask = rng.random(n) < frac
    mask[dead[:10]] = True                                     # selecting a tombstoned row selects nothing
    qs = O.gen_rows(4712, 0, nq, dim)
    r, d, c = idx.search_masked(qs, k, mask)
    sel = (alive.astype(bool) & mask).astype(np.uint8)
    want = min(k, int(sel.sum()))
    assert (c == want).all()
    for i in range(nq):
        ro, do = O.exact_search(mid, rows, qs[i], k, alive=sel)
        assert ro.size == want
        assert r[i, :want].tolist() == ro.tolist(), (metric, i)
        assert d[i, :want].tobytes() == do.tobytes(), (metric, i)
        assert (r[i, want:] == 0xFFFFFFFF).all()
    # an empty selection is an empty result, not an error
    r0, d0, c0 = idx.search_masked(qs, k, np.zeros(n, bool))
    assert (c0 == 0).all()
    # and the filtered first-k of the FULL ranking (what Collection.Search does above the seam) is the same list
    if n <= 5000:
        fr, fd, _ = idx.search(qs[:1], idx.size())
        first = [int(x) for x in fr[0] if mask[int(x)]][:want]
        assert first == r[0, :want].tolist()


def test_pure_c_consumer_of_the_abi(tmp_path):
    """tests/c/abi_smoke.c: C11 + include/qv.h + libqv.so only — create / add / search / remove / destroy, a device HNSW build +
    search and a one-shard qv_sharded_* round trip on the GPU (RCCL prints its version banner on stdout before the result line)"""
    import subprocess
    from tests.test_abi import _build_c_smoke
    p = subprocess.run([_build_c_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1].startswith("ok:"), p.stdout + p.stderr
