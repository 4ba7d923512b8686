"""The int8 batched filter (QV_FILTER_INT8) on the CPU: the dispatch's rule (qv_batched_int8_applies) over true and false cells of each of its
conditions, and the kernel's keep/drop decision compiled for the host (qv_batched_int8_keeps) against the certified interval of the 8-bit bound
scan (qv_scan_bound_interval8): whenever d_lo <= U the row must be kept — a containment condition, not a tolerance — and a row the bound
declines is always kept.  The row's bytes come from the library's quantiser, the integer chains from numpy."""
import ctypes as C

import numpy as np
import pytest

import quiver_amd
from quiver_amd import _lib
from tests import _oracle as O
from tests._bound import COSINE, DOT, chain_norm
from tests._bound8 import quantize_query, quantize_row

M = 1_000_000


@pytest.mark.parametrize("metric,dim,rows,nq,k,filt,plane8,want", [
    ("cosine", 768, M, 64, 10, "int8", True, True),
    ("dot_product", 768, M, 256, 64, "int8", True, True),
    ("cosine", 64, M, 9, 1, "int8", True, True),              # the smallest dimension, the smallest batch
    ("cosine", 1024, 32_805, 40, 1000, "int8", True, True),   # the largest dimension, the smallest corpus, the large-k funnel
    ("euclidean", 768, M, 64, 10, "int8", True, False),       # metric
    ("squared_euclidean", 768, M, 64, 10, "int8", True, False),
    ("cosine", 768, M, 64, 10, "int8", False, False),         # no plane8
    ("cosine", 48, M, 64, 10, "int8", True, False),           # dimension: below 64, a multiple of 16 but not of 32, above 1024
    ("cosine", 80, M, 64, 10, "int8", True, False),
    ("cosine", 1040, M, 64, 10, "int8", True, False),
    ("cosine", 768, M, 8, 10, "int8", True, False),           # the batched path itself: too few queries, rows, query-rows; k beyond it
    ("cosine", 768, 20_000, 64, 10, "int8", True, False),
    ("cosine", 768, 32_805, 9, 10, "int8", True, False),
    ("cosine", 768, M, 64, 5000, "int8", True, False),
    ("cosine", 768, M, 64, 10, "auto", True, False),          # only an index that asks
    ("cosine", 768, M, 64, 10, "bf16x1", True, False),
    ("cosine", 768, M, 64, 10, "off", True, False),
])
def test_rule(metric, dim, rows, nq, k, filt, plane8, want):
    assert quiver_amd.batched_int8_applies(metric, dim, rows, nq, k, filter=filt, has_plane8=plane8) is want


def keeps(metric, dim, ihi, ilo, sq, qn, qres, U, rn, scale, res):
    rc = _lib.lib().qv_batched_int8_keeps(metric, dim, ihi, ilo, sq, qn, qres, C.c_float(U), rn, C.c_float(scale), C.c_float(res))
    assert rc in (0, 1), _lib.lib().qv_last_error()
    return rc


@pytest.mark.parametrize("metric", [COSINE, DOT])
@pytest.mark.parametrize("dim", [64, 768])
def test_keeps_contains_the_certified_interval(metric, dim):
    rng = np.random.default_rng(1000 * dim + metric)
    unit = lambda n: (lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))(rng.standard_normal((n, dim)))
    queries = np.concatenate([unit(2), unit(2) * np.float32(6.5)])
    rows = np.concatenate([unit(12), unit(12) * np.float32(3.0), O.gen_rows(20260424, 0, 8, dim)])
    fn = _lib.lib().qv_scan_bound_interval8
    far = dropped = 0
    for q in queries:
        qn = chain_norm(q)
        _, qhi, qlo, sq, qres = quantize_query(q)
        for r in rows:
            r8, scale, res = quantize_row(r)
            rn = chain_norm(r)
            ihi, ilo = int(np.sum(qhi * r8.astype(np.int64))), int(np.sum(qlo * r8.astype(np.int64)))
            lo, hi = C.c_float(0), C.c_float(0)
            assert fn(metric, dim, 128 * ihi + ilo, sq, qn, qres, rn, C.c_float(scale), C.c_float(res), C.byref(lo), C.byref(hi)) == 0
            d = np.float32(O.distance(metric, q, r))
            assert lo.value <= d <= hi.value
            s = 1.0 if metric == COSINE else qn * rn                    # what a distance of this pair moves by per unit of cosine
            for U in (d, np.nextafter(d, np.float32(np.inf)), np.nextafter(d, np.float32(-np.inf)), np.float32(d + 1e-4 * s), np.float32(d - 1e-4 * s),
                      np.float32(lo.value), np.float32(d - 0.15 * s), np.float32(d - 0.5 * s)):
                got = keeps(metric, dim, ihi, ilo, sq, qn, qres, float(U), rn, scale, res)
                if lo.value <= U:
                    assert got == 1, (metric, dim, float(lo.value), float(d), float(U))
                if d - U > 0.1:
                    far += 1; dropped += 1 - got
            # a row the bound declines is kept whatever the bound: no residual, no scale, a scale out of range
            for sc2, res2 in ((scale, np.nan), (0.0, res), (np.float32(2e36), res), (np.nan, res)):
                assert keeps(metric, dim, ihi, ilo, sq, qn, qres, -5.0, rn, sc2, res2) == 1
    assert far >= 2 * len(queries) * len(rows) and 2 * dropped >= far, (far, dropped)     # not a function that always says keep
