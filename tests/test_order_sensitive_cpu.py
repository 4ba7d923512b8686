"""Rows whose float32 distance depends on the order of summation (tests/_order.py), on the CPU.

(a) the C oracle, its numpy restatement and the host qv_distance_pair give the reference chain's bits on every planted row;
(b) every wrong order of _order.ORDERS gives other bits on at least one planted row of each metric and dimension — so a kernel
    that sums in that order cannot pass the GPU tests built on these rows (tests/test_gpu_order_sensitive.py);
(c) for the split forms (the HNSW latency form, the short-corpus scan) the certificate's interval does not decide a single
    planted row: on the device every one of them goes through the fallback, the row walked again as one chain."""
import numpy as np
import pytest

from quiver_amd.device_index import distance_pair
from tests import _oracle as O
from tests import _order as OR

DIMS_F64 = [32, 100, 128, 256, 768, 1536]
DIMS_F32 = [100, 256]
CASES = [(m, d) for m in OR.F64_METRICS for d in DIMS_F64] + [(m, d) for m in OR.F32_METRICS for d in DIMS_F32]


def _planted(metric, dim, n_queries=2, n_try=24):
    rng = np.random.default_rng(9100 + 37 * metric + dim)
    out = []
    for _ in range(n_queries):
        q = OR.query_for(metric, dim, rng)
        out.append((q, OR.planted_rows(metric, dim, q, n_try, rng)))
    return out


@pytest.mark.parametrize("metric,dim", CASES)
def test_reference_restatements_give_the_chains_bits(metric, dim):
    """(a)"""
    n = 0
    for q, rows in _planted(metric, dim):
        for r in rows:
            want = OR.bits(OR.model_distance(metric, q, r, "chain"))
            assert OR.bits(O.distance(metric, q, r)) == want, (metric, dim)
            assert OR.bits(OR.oracle_chain(metric, q, r)) == want, (metric, dim)
            assert OR.bits(distance_pair(metric, q, r)) == want, (metric, dim)
            n += 1
    assert n >= 16, (metric, dim, n)


@pytest.mark.parametrize("metric,dim", CASES)
def test_every_wrong_order_is_caught(metric, dim):
    """(b)"""
    caught = {o: 0 for o in OR.orders_for(metric, dim)}
    for q, rows in _planted(metric, dim):
        for r in rows:
            for o in OR.sensitive(metric, q, r):
                caught[o] += 1
    assert all(caught.values()), (metric, dim, caught)


@pytest.mark.parametrize("metric,dim", [c for c in CASES if c[0] in OR.SPLIT_METRICS])
def test_certificate_cannot_decide_a_planted_row(metric, dim):
    """(c); and the reference's chain lies inside the interval (the certificate's own premise)"""
    for q, rows in _planted(metric, dim):
        for r in rows:
            ref = float(OR.order_sum("chain", OR.terms(metric, q, r)[0]))
            for o in OR.SPLIT_ORDERS:
                if o not in OR.orders_for(metric, dim):
                    continue
                lo, hi, s, b = OR.certificate(metric, q, r, o)
                assert OR.bits(lo) != OR.bits(hi), (metric, dim, o)
                assert s - b <= ref <= s + b, (metric, dim, o)


def test_models_agree_where_order_cannot_matter():
    """small integers: every partial sum is exact, so every order gives the chain's bits (the models themselves are sound)"""
    rng = np.random.default_rng(5)
    for metric in range(9):
        for dim in (32, 96, 256):
            q = rng.integers(-8, 9, size=dim).astype(np.float32)
            r = rng.integers(-8, 9, size=dim).astype(np.float32)
            want = OR.bits(O.distance(metric, q, r))
            for o in ("chain",) + OR.orders_for(metric, dim):
                assert OR.bits(OR.model_distance(metric, q, r, o)) == want, (metric, dim, o)


def test_worked_example():
    """the Euclidean row of the issue: q = 0, D = 256: the chain gives 2^24, reverse / split / exact give 2^24 + 2"""
    r = np.zeros(256, np.float32)
    r[:8] = [2 ** 24, 5792, 84, 10, 3.5, 0.75, 0.25, 0.25]
    r[8:208] = 0.17
    q = np.zeros(256, np.float32)
    assert OR.model_distance(OR.L2, q, r, "chain") == np.float32(16777216.0) == O.distance(OR.L2, q, r)
    for o in ("reverse", "exact", "scan_split", "lat4", "pairwise"):
        assert OR.model_distance(OR.L2, q, r, o) == np.float32(16777218.0), o
