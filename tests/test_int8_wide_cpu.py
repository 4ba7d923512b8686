"""The int8 batched filter at 1056 to 4096 dimensions (k_int8_wide_filter) on the CPU: the dispatch's rule at the new widths, and the keep/drop
decision compiled for the host (qv_batched_int8_keeps) against the certified interval of the 8-bit bound scan, as tests/test_int8_filter_cpu.py
holds it up to 1024 — whenever d_lo <= U the row must be kept.  Above 2048 dimensions 128 I_hi + I_lo leaves int32: a query of one magnitude
against its own copies reaches +-4.2e9 and +-8.5e9, and a sum formed in 32 bits wraps (it did before the wide score: those cases failed)."""
import ctypes as C

import numpy as np
import pytest

import quiver_amd
from quiver_amd import _lib
from tests import _oracle as O
from tests._bound import COSINE, DOT, chain_norm
from tests._bound8 import quantize_query, quantize_row
from tests.test_int8_filter_cpu import keeps

M = 1_000_000


@pytest.mark.parametrize("metric,dim,nq,k,want", [
    ("cosine", 1056, 40, 10, True), ("dot_product", 1536, 64, 64, True), ("cosine", 4096, 9, 1, True), ("cosine", 3072, 40, 1000, True),
    ("cosine", 4128, 40, 10, False), ("cosine", 1040, 40, 10, False),
])
def test_rule(metric, dim, nq, k, want):
    assert quiver_amd.batched_int8_applies(metric, dim, M, nq, k, filter="int8", has_plane8=True) is want


def test_rule_forms():
    assert quiver_amd.batched_int8_form("cosine", 1536, M, 256, 10, filter="int8", has_plane8=True, mode="shared") == 1
    assert quiver_amd.batched_int8_applies_filtered("cosine", 1536, M, 64, 10, filter="int8", has_plane8=True, mode="always") is False


def _contained(metric, dim, q, rows, fractions):
    """every (q, row) pair against the bounds `fractions` gives; -> (pairs far below their bound, those of them dropped, the largest |I|)"""
    fn = _lib.lib().qv_scan_bound_interval8
    qn = chain_norm(q)
    _, qhi, qlo, sq, qres = quantize_query(q)
    far = dropped = big = 0
    for r in rows:
        r8, scale, res = quantize_row(r)
        rn = chain_norm(r)
        ihi, ilo = int(np.sum(qhi * r8.astype(np.int64))), int(np.sum(qlo * r8.astype(np.int64)))
        big = max(big, abs(128 * ihi + ilo))
        lo, hi = C.c_float(0), C.c_float(0)
        assert fn(metric, dim, 128 * ihi + ilo, sq, qn, qres, rn, C.c_float(scale), C.c_float(res), C.byref(lo), C.byref(hi)) == 0
        d = np.float32(O.distance(metric, q, r))
        assert lo.value <= d <= hi.value
        s = 1.0 if metric == COSINE else qn * rn                        # what a distance of this pair moves by per unit of cosine
        for U in [d, np.nextafter(d, np.float32(np.inf)), np.nextafter(d, np.float32(-np.inf)), np.float32(lo.value)] + [np.float32(d + f * s) for f in fractions]:
            got = keeps(metric, dim, ihi, ilo, sq, qn, qres, float(U), rn, scale, res)
            if lo.value <= U:
                assert got == 1, (metric, dim, float(lo.value), float(d), float(U))
            if d - U > 0.1 * s:
                far += 1; dropped += 1 - got
    return far, dropped, big


@pytest.mark.parametrize("metric", [COSINE, DOT])
@pytest.mark.parametrize("dim", [1536, 4096])
def test_keeps_contains_the_certified_interval(metric, dim):
    rng = np.random.default_rng(1000 * dim + metric)
    unit = lambda n: (lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))(rng.standard_normal((n, dim)))
    rows = np.concatenate([unit(6), unit(6) * np.float32(3.0), O.gen_rows(20260424, 0, 4, dim)])
    far = dropped = 0
    for q in np.concatenate([unit(1), unit(1) * np.float32(6.5)]):
        f, d, _ = _contained(metric, dim, q, rows, (1e-4, -1e-4, -0.15, -0.5))
        far += f; dropped += d
    assert far >= 2 * 2 * len(rows) and 2 * dropped >= far, (far, dropped)     # not a function that always says keep


@pytest.mark.parametrize("metric", [COSINE, DOT])
@pytest.mark.parametrize("dim", [2048, 4096])
def test_keeps_where_the_integer_sum_leaves_int32(metric, dim):
    rng = np.random.default_rng(dim + metric)
    q = (np.float32(0.37) * rng.choice(np.float32([-1.0, 1.0]), dim)).astype(np.float32)    # every quantised element is +-16256, every row byte +-127
    far, dropped, big = _contained(metric, dim, q, [q, -q, np.float32(3.0) * q], (1e-4, -1e-4, -0.15, -0.5))
    assert big > 2**31
    assert far >= 3 and dropped == far, (far, dropped)          # a bound far below such a pair drops it: the sum did not wrap the other way either
