"""The int8 filter's panel kernel (k_int8_wide_filter, qv_int8.hip: 1056 to 4096 dimensions under set_filter("int8")) must return exactly what the
exact scans return: rows, float32 bits, (distance, row) order, counts and padding.  The reference is the same index under set_filter("off"), 8
queries at a time, and the CPU oracle for some queries per case.  int8_filter_stats()[0] grows: the batch ran on the int8 kernel (before the
kernel existed these widths kept the default kernels and the counter stayed).  513 tiles, the last one ragged: no grid of eight-wave workgroups
divides them, so some waves idle through a workgroup's last round."""
import functools

import numpy as np
import pytest

from tests import _oracle as O
from tests.test_gpu_int8_filter import _bits, _both, _eq

pytestmark = pytest.mark.gpu

N = 32_768 + 37


@functools.lru_cache(maxsize=1)
def _index(metric, dim):
    import quiver_amd as q
    idx = q.DeviceIndex(dim, metric)
    idx.add_synthetic(20260424, 0, N)
    return idx


@functools.lru_cache(maxsize=1)
def _corpus(dim):
    return O.gen_rows(20260424, 0, N, dim)


@pytest.mark.parametrize("metric,dim,nq,k,oracle", [
    ("cosine", 1056, 40, 10, 3),                 # 33 steps: eight whole revolutions of the ring and a step; the branching form
    ("dot_product", 1536, 65, 64, 3),            # three whole panels; a batch one past a block
    ("cosine", 1536, 300, 10, 3),                # four blocks and a remainder
    ("cosine", 2048, 64, 100, 1),                # the large-k funnel reading rres8
    ("cosine", 4096, 40, 10, 1),                 # the widest: eight panels
])
def test_int8_wide_equals_exact_scan(metric, dim, nq, k, oracle):
    import quiver_amd as q
    idx = _index(metric, dim)
    qs = O.gen_rows(20260425, 0, nq, dim)
    ref, got, batches, handed = _both(idx, qs, k)
    assert _eq(ref, got)
    assert batches >= 1
    if k <= 64:
        assert handed == 0, handed
    for i in ((0, nq // 2, nq - 1) if oracle == 3 else (nq // 2,)):
        er, ed = O.exact_search(q.metric_id(metric), _corpus(dim), qs[i], k)
        assert np.array_equal(got[0][i], er) and np.array_equal(_bits(got[1][i]), _bits(ed))


def test_int8_wide_sum_beyond_int32():
    """4096 dimensions, a query of one magnitude and its copies: 128 I_hi + I_lo = +-8.5e9 for these pairs"""
    import quiver_amd as q
    dim, nq, k = 4096, 40, 10
    rows = _corpus(dim).copy()
    qs = O.gen_rows(20260425, 0, nq, dim)
    qs[0] = np.float32(0.37) * np.where(qs[0] < 0, np.float32(-1.0), np.float32(1.0))
    rows[1000:1012] = qs[0]
    rows[2000:2004] = -qs[0]
    idx = q.DeviceIndex(dim, "cosine")
    idx.add(rows)
    ref, got, batches, handed = _both(idx, qs, k)
    assert _eq(ref, got)
    assert batches >= 1 and handed == 0
    assert got[0][0].tolist() == list(range(1000, 1010))


def test_int8_wide_row_and_query_states():
    import quiver_amd as q
    dim, nq, k = 1536, 40, 64
    rows = _corpus(dim).copy()
    qs = O.gen_rows(20260425, 0, nq, dim)
    rows[100] = 0.0                                          # a zero row
    rows[200, 5] = np.inf                                    # a row the 8-bit bound declines
    qs[5] = 0.0                                              # handed back: no scale
    idx = q.DeviceIndex(dim, "cosine")
    idx.add(rows)
    dead = np.arange(4000, 4200)                             # spans the whole tile 63 (rows 4032 .. 4095)
    idx.remove(dead)
    ref, got, batches, handed = _both(idx, qs, k)
    assert _eq(ref, got)
    assert batches >= 1 and handed >= 1
    alive = np.ones(N, bool); alive[dead] = False
    er, ed = O.exact_search(q.metric_id("cosine"), rows, qs[1], k, alive=alive)
    assert np.array_equal(got[0][1], er) and np.array_equal(_bits(got[1][1]), _bits(ed))
