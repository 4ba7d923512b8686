"""The int8 matrix-core filter on the 8-bit plane (set_filter("int8"); qv_int8.hip) must return exactly what the exact scans return: rows,
float32 bits, (distance, row) order, counts and padding.  The reference is the same index under set_filter("off"), 8 queries at a time; for
three queries per case the CPU oracle must agree too.  int8_filter_stats()[0] grows exactly where the kernel should have run."""
import functools

import numpy as np
import pytest

from tests import _oracle as O

pytestmark = pytest.mark.gpu

N = 32_768 + 37            # the smallest corpus the batched path takes: a ragged last tile
N9 = 111_104 + 37          # ... for 9 queries (a million query-rows)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _eq(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(a[2], b[2])


def _both(idx, qs, k, search=None):
    """-> (reference under "off", 8 queries at a time; the answer under "int8"; how many int8 batches that took, how many queries it handed back)"""
    search = search or (lambda q: idx.search(q, k, batched=True))
    idx.set_filter("off")
    outs = [search(qs[i: i + 8]) for i in range(0, len(qs), 8)]
    ref = tuple(np.concatenate([o[j] for o in outs]) for j in range(3))
    idx.set_filter("int8")
    before = idx.int8_filter_stats()
    got = search(qs)
    after = idx.int8_filter_stats()
    return ref, got, after[0] - before[0], after[2] - before[2]


@functools.lru_cache(maxsize=2)
def _index(metric, dim, n, **kw):
    import quiver_amd as q
    idx = q.DeviceIndex(dim, metric, **kw)
    idx.add_synthetic(20260424, 0, n)
    return idx


@functools.lru_cache(maxsize=2)
def _corpus(dim, n):
    return O.gen_rows(20260424, 0, n, dim)


@pytest.mark.parametrize("metric,dim,nq,k", [
    ("cosine", 64, 9, 1), ("dot_product", 64, 9, 64), ("dot_product", 64, 64, 10),        # two steps
    ("cosine", 96, 40, 10), ("dot_product", 96, 65, 64),                                     # an odd step count; a batch one past a block
    ("cosine", 768, 40, 10), ("cosine", 768, 65, 1), ("cosine", 768, 300, 10), ("dot_product", 768, 64, 64),   # 300: 256 queries in four blocks, then 44
    ("cosine", 768, 40, 100), ("cosine", 768, 64, 1000),                                     # the large-k funnel reading rres8
    ("dot_product", 1024, 64, 10), ("cosine", 1024, 300, 64),                                # the LDS limit
])
def test_int8_filter_equals_exact_scan(metric, dim, nq, k):
    import quiver_amd as q
    n = N9 if nq == 9 else N
    idx = _index(metric, dim, n)
    qs = O.gen_rows(20260425, 0, nq, dim)
    ref, got, batches, handed = _both(idx, qs, k)
    assert _eq(ref, got)
    assert batches >= 1 and idx.int8_filter_stats()[3] == 1
    if k <= 64:
        assert handed == 0, handed                           # the filter filtered: no list overflowed into the exact redo
    for i in (0, nq // 2, nq - 1):
        er, ed = O.exact_search(q.metric_id(metric), _corpus(dim, n), qs[i], k)
        assert np.array_equal(got[0][i], er) and np.array_equal(_bits(got[1][i]), _bits(ed))


def test_int8_filter_row_and_query_states():
    import quiver_amd as q
    dim, nq, k = 768, 40, 64
    rows = _corpus(dim, N).copy()
    qs = O.gen_rows(20260425, 0, nq, dim)
    rows[100] = 0.0                                          # a zero row
    rows[200, 5] = np.inf; rows[300, 7] = np.nan             # rows the 8-bit bound declines
    rows[1000:1070] = qs[0]                                  # 70 exact copies of a query: ties beyond k, resolved by (distance, row)
    qs[5] = 0.0                                              # handed back: no scale
    qs[6] *= np.float32(1e20)                                # handed back: a huge norm
    idx = q.DeviceIndex(dim, "cosine")
    idx.add(rows)
    dead = np.arange(4000, 4200)                             # spans the whole tile 63 (rows 4032 .. 4095)
    idx.remove(dead)
    ref, got, batches, handed = _both(idx, qs, k)
    assert _eq(ref, got)
    assert batches >= 1 and handed >= 2
    assert got[0][0].tolist() == list(range(1000, 1064))
    alive = np.ones(N, bool); alive[dead] = False
    for i in (0, 1, nq - 1):
        er, ed = O.exact_search(q.metric_id("cosine"), rows, qs[i], k, alive=alive)
        assert np.array_equal(got[0][i], er) and np.array_equal(_bits(got[1][i]), _bits(ed))


def test_int8_filter_counters_are_its_own():
    """a single-query search for 100 results (the wide bound scan, which counts itself in the same array) and an int8 batch leave each other's counters alone"""
    idx = _index("cosine", 768, N)
    idx.set_filter("int8")
    qs = O.gen_rows(20260425, 0, 40, 768)
    idx.set_bound_scan_wide("always")
    try:
        i0, w0 = idx.int8_filter_stats(), idx.bound_scan_wide_stats()
        idx.search(qs[:1], 100)
        i1, w1 = idx.int8_filter_stats(), idx.bound_scan_wide_stats()
        idx.search(qs, 10, batched=True)
        i2, w2 = idx.int8_filter_stats(), idx.bound_scan_wide_stats()
    finally:
        idx.set_bound_scan_wide("auto")
    assert w1["searches"] == w0["searches"] + 1 and i1 == i0
    assert i2[:2] == (i1[0] + 1, i1[1] + 40) and w2 == w1


@pytest.mark.parametrize("metric,dim,kw", [("cosine", 768, {"scan_plane": False}), ("cosine", 48, {}), ("cosine", 1040, {}), ("euclidean", 768, {})])
def test_int8_filter_stays_out(metric, dim, kw):
    """no plane8, a dimension outside the kernel's, another metric: the batch runs as under "auto", results equal"""
    idx = _index(metric, dim, N, **kw)
    qs = O.gen_rows(20260425, 0, 40, dim)
    ref, got, batches, _ = _both(idx, qs, 10)
    assert _eq(ref, got) and batches == 0


def test_int8_filter_leaves_filtered_batches_alone():
    import quiver_amd as q
    n = 65_536 + 37                                          # (16 queries: a million query-rows)
    idx = _index("cosine", 768, n)
    idx.set_filtered_batch("always")
    try:
        qs = O.gen_rows(20260425, 0, 16, 768)
        mask = np.zeros(n, bool); mask[::3] = True
        rs = q.RowSet(idx, mask)
        ref, got, batches, _ = _both(idx, qs, 10, search=lambda x: idx.search_rowsets(x, 10, rs))
        assert _eq(ref, got) and batches == 0
        assert idx.filtered_batch_stats()["batches"] >= 1
    finally:
        idx.set_filtered_batch("auto")
