"""The CPU oracle on non-finite and extreme-magnitude inputs (value classes of tests/_extremes.py), before any GPU test trusts it:
the C restatement against the independent numpy mirror for all nine metrics, the (distance, row; NaN last) order of
qvo_exact_search against a plain Python sort, and the host qv_distance_pair against the oracle.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

from quiver_amd.device_index import distance_pair
from tests import _extremes as X
from tests import _oracle as O

sys.path.insert(0, os.path.join(O.ROOT, "oracle"))
import oracle_np as NP  # noqa: E402

DIMS = [1, 3, 4, 5, 17, 64, 768]


def _pairs(dim):
    """every class against an ordinary vector, against itself, and against every other class"""
    rng = np.random.default_rng(4000 + dim)
    ext = X.class_rows(rng, dim)
    ords = [("ord", "a", X.unit(rng, dim)), ("ord", "b", (rng.standard_normal(dim) * 3).astype(np.float32))]
    vecs = ords + ext
    out = []
    for i, (ca, na, a) in enumerate(vecs):
        for cb, nb, b in vecs[i:]:
            out.append((f"{ca}:{na}|{cb}:{nb}", a, b))
            out.append((f"{cb}:{nb}|{ca}:{na}", b, a))
    return out


def _want(metric, a, b):
    with np.errstate(all="ignore"):
        return np.float32(NP.distance(metric, a, b))


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("metric", range(9))
def test_c_oracle_equals_the_numpy_mirror_on_every_class(metric, dim):
    bad = []
    for name, a, b in _pairs(dim):
        want = _want(metric, a, b)
        got = O.distance(metric, a, b)
        if not X.same(np.float32(got)[None], want[None]):
            bad.append((name, got, want))
    assert not bad, bad[:5]


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("metric", range(9))
def test_host_distance_pair_equals_the_oracle_on_every_class(metric, dim):
    """qv_distance_pair (the kernels' per-pair routine compiled for the CPU) on the same classes"""
    bad = []
    for name, a, b in _pairs(dim):
        want = np.float32(O.distance(metric, a, b))
        got = np.float32(distance_pair(metric, a, b))
        if not X.same(got[None], want[None]):
            bad.append((name, got, want))
    assert not bad, bad[:5]


@pytest.mark.parametrize("dim", [1, 64])
@pytest.mark.parametrize("metric", range(9))
def test_all_distances_equals_the_numpy_mirror_over_a_mixed_corpus(metric, dim):
    rng = np.random.default_rng(77 + dim)
    rows = np.stack([v for _, _, v in X.class_rows(rng, dim, per_class=2)] + [X.unit(rng, dim) for _ in range(20)])
    for q in (X.unit(rng, dim), rows[0], rows[-25], np.zeros(dim, np.float32)):
        with np.errstate(all="ignore"):
            want = NP.distances(metric, q, rows)
        assert X.same(O.all_distances(metric, rows, q), want)


def _ordering_corpus():
    """dot_product over 2-d rows against q = (1, 0): distance = 1 - row[0] exactly for small row[0], and 1 - (c + 0*x), so
    x = +-inf makes the distance NaN.  Rows: NaN (several patterns), +inf and -inf distances, equal finite ties, +0 distances
    (row[0] = 1), all -0.0 and all +0.0 rows (both distance 1, a tie broken by row).  No metric produces a -0 distance (sums
    start at +0 and x - x = +0 under round-to-nearest), so -0 appears as row elements only."""
    r = []
    nan = X.NANS
    for c in (0.25, 0.5, 0.25, 1.0, 0.5, 1.0, 0.25):
        r.append([c, 0.0])                                             # ties at 0.75 / 0.5 / +0
    r += [[nan[0], 1.0], [0.5, np.inf], [-np.inf, 0.0], [nan[2], 0.0], [0.1, -np.inf]]   # NaN, NaN, +inf, NaN, NaN
    r += [[np.inf, 0.0], [-0.0, -0.0], [0.0, 0.0], [-np.inf, 2.0], [nan[3], nan[1]]]     # -inf, 1 (-0 row), 1, +inf, NaN
    r += [[0.75, 3.0], [np.inf, 1.0], [-1e30, 0.0], [1e30, 0.0]]                          # 0.25, -inf, 1e30, -1e30
    return np.asarray(r, np.float32), np.array([1.0, 0.0], np.float32)


def _python_order(d):
    n = np.isnan(d)
    return sorted(range(d.size), key=lambda i: (bool(n[i]), 0.0 if n[i] else float(d[i]), i))


def test_exact_search_order_is_distance_then_row_nan_last():
    rows, q = _ordering_corpus()
    d = O.all_distances(3, rows, q)
    with np.errstate(all="ignore"):
        assert X.same(d, NP.distances(3, q, rows))
    assert np.isnan(d).sum() >= 4 and (d == np.inf).sum() >= 2 and (d == -np.inf).sum() >= 2 and (d == 0).sum() >= 2
    order = _python_order(d)
    n_fin = int(np.isfinite(d).sum()); n_num = int((~np.isnan(d)).sum()); n = d.size
    for k in (1, n_fin - 1, n_fin, n_fin + 1, n_num, n_num + 1, n):
        r, dd = O.exact_search(3, rows, q, k)
        assert r.tolist() == order[:k], k
        assert X.same(dd, d[order[:k]]), k
        with np.errstate(all="ignore"):
            rn, dn = NP.exact_search(3, rows, q, k)
        assert rn.tolist() == order[:k], k


def test_exact_search_order_with_dead_rows_and_a_nan_query():
    rows, q = _ordering_corpus()
    alive = np.ones(rows.shape[0], np.uint8); alive[[0, 7, 12, 16]] = 0
    d = O.all_distances(3, rows, q)
    live = [i for i in _python_order(d) if alive[i]]
    for k in (1, 5, len(live)):
        r, _ = O.exact_search(3, rows, q, k, alive=alive)
        assert r.tolist() == live[:k], k
    qn = np.array([X.NANS[1], 0.0], np.float32)                       # every distance NaN: the rows in row order
    r, dd = O.exact_search(3, rows, qn, rows.shape[0])
    assert r.tolist() == list(range(rows.shape[0])) and np.isnan(dd).all()


@pytest.mark.parametrize("metric", range(9))
def test_exact_search_order_over_every_class(metric):
    """the ranking of a mixed corpus (every class, two of each) for queries of every class = the Python sort of the oracle's distances"""
    rng = np.random.default_rng(900 + metric)
    dim = 17
    rows = np.stack([v for _, _, v in X.class_rows(rng, dim, per_class=2)] + [X.unit(rng, dim) for _ in range(30)])
    rows = np.concatenate([rows, rows[::7]])                           # duplicates: ties of every kind
    for _, _, q in X.class_rows(rng, dim)[::3] + [("ord", "", X.unit(rng, dim))]:
        d = O.all_distances(metric, rows, q)
        order = _python_order(d)
        for k in (1, int(np.isfinite(d).sum()) or 1, int((~np.isnan(d)).sum()) or 1, rows.shape[0]):
            r, dd = O.exact_search(metric, rows, q, k)
            assert r.tolist() == order[:k] and X.same(dd, d[order[:k]]), k
