"""The int8 filter's shared-row kernel (set_filter("int8") + set_int8_form("shared"); k_int8_shared_filter, qv_int8.hip) must return exactly what the
exact scans return: rows, float32 bits, (distance, row) order, counts and padding.  The reference is the same index under set_filter("off"), 8
queries at a time; for three queries per case the CPU oracle must agree too.  int8_shared_stats() grows exactly where the kernel should have run."""
import functools

import numpy as np
import pytest

from tests import _oracle as O

pytestmark = pytest.mark.gpu

N = 32_768 + 37            # the smallest corpus the batched path takes: a ragged last tile


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _eq(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(a[2], b[2])


def _reference(idx, qs, k):
    idx.set_filter("off")
    outs = [idx.search(qs[i: i + 8], k, batched=True) for i in range(0, len(qs), 8)]
    return tuple(np.concatenate([o[j] for o in outs]) for j in range(3))


def _int8(idx, qs, k, form):
    """-> (the answer under "int8" in that form; shared batches, their queries, int8 batches, queries handed back)"""
    idx.set_filter("int8")
    idx.set_int8_form(form)
    try:
        s0, f0 = idx.int8_shared_stats(), idx.int8_filter_stats()
        got = idx.search(qs, k, batched=True)
        s1, f1 = idx.int8_shared_stats(), idx.int8_filter_stats()
    finally:
        idx.set_int8_form("auto")
    return got, s1[0] - s0[0], s1[1] - s0[1], f1[0] - f0[0], f1[2] - f0[2]


@functools.lru_cache(maxsize=2)
def _index(metric, dim):
    import quiver_amd as q
    idx = q.DeviceIndex(dim, metric)
    idx.add_synthetic(20260424, 0, N)
    return idx


@functools.lru_cache(maxsize=2)
def _corpus(dim):
    return O.gen_rows(20260424, 0, N, dim)


@pytest.mark.parametrize("metric,dim,nq,k,shared_q,batches", [
    ("cosine", 128, 129, 1, 129, 1),          # fewer steps than any ring; one real query in wave 2, wave 3 all padding
    ("dot_product", 128, 256, 64, 256, 1),
    ("cosine", 384, 200, 10, 200, 1),
    ("dot_product", 512, 256, 10, 256, 1),
    ("cosine", 768, 129, 10, 129, 1),
    ("cosine", 768, 256, 64, 256, 1),
    ("cosine", 768, 300, 10, 256, 2),         # 256 on the shared-row kernel, then 44 on the block kernel
    ("cosine", 768, 512, 1, 512, 1),          # two groups
    ("cosine", 768, 256, 100, 256, 1),        # the large-k funnel reading rres8
])
def test_shared_form_equals_exact_scan(metric, dim, nq, k, shared_q, batches):
    import quiver_amd as q
    idx = _index(metric, dim)
    qs = O.gen_rows(20260425, 0, nq, dim)
    ref = _reference(idx, qs, k)
    got, sb, sq, fb, handed = _int8(idx, qs, k, "shared")
    assert _eq(ref, got)
    if k <= 64:
        assert (sb, sq, fb) == (1, shared_q, batches), (sb, sq, fb)
        assert handed == 0, handed                           # the filter filtered: no list overflowed into the exact redo
    for i in (0, nq // 2, nq - 1):
        er, ed = O.exact_search(q.metric_id(metric), _corpus(dim), qs[i], k)
        assert np.array_equal(got[0][i], er) and np.array_equal(_bits(got[1][i]), _bits(ed))


def test_shared_form_row_and_query_states():
    import quiver_amd as q
    dim, nq, k = 768, 200, 64
    rows = _corpus(dim).copy()
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
    ref = _reference(idx, qs, k)
    got, sb, sq, _, handed = _int8(idx, qs, k, "shared")
    assert _eq(ref, got)
    assert (sb, sq) == (1, nq) and handed >= 2
    assert got[0][0].tolist() == list(range(1000, 1064))
    alive = np.ones(N, bool); alive[dead] = False
    for i in (0, 130, 199):                                  # 130 and 199: the upper waves
        er, ed = O.exact_search(q.metric_id("cosine"), rows, qs[i], k, alive=alive)
        assert np.array_equal(got[0][i], er) and np.array_equal(_bits(got[1][i]), _bits(ed))


@pytest.mark.parametrize("dim,nq,form", [(96, 256, "shared"), (1024, 256, "shared"), (768, 256, "blocks"), (768, 128, "shared")])
def test_shared_form_stays_out(dim, nq, form):
    """a dimension without an instantiation, the block form asked for, no whole group: the block kernel runs, results equal"""
    idx = _index("cosine", dim)
    qs = O.gen_rows(20260425, 0, nq, dim)
    ref = _reference(idx, qs, 10)
    got, sb, sq, fb, _ = _int8(idx, qs, 10, form)
    assert _eq(ref, got) and (sb, sq) == (0, 0) and fb == 1


def test_both_forms_agree():
    idx = _index("cosine", 768)
    qs = O.gen_rows(20260425, 0, 256, 768)
    a, sa = _int8(idx, qs, 10, "blocks")[:2]
    b, sb = _int8(idx, qs, 10, "shared")[:2]
    assert _eq(a, b) and (sa, sb) == (0, 1)
