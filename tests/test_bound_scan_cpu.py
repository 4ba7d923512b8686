"""The interval behind the single-query bound scan (quiver_amd/csrc/qv_bound.h), checked on the CPU through the library's own
function compiled for the host (qv_scan_bound_interval): stage 1 of that scan computes S~, a float32 fma chain of the float32 query
times the row's bfloat16 copy, and rejects a row when the LOWER end of the interval it derives for the reference's float32 distance
lies above a threshold.  So for every row the rule does not mark "unsure" the oracle's float32 distance must lie in [d_lo, d_hi], and
a row whose oracle distance is not a number must be marked (an unsure row is always passed on to the exact re-score).  Queries whose
norm is not a number, huge or vanishing are handed to the exact scan whole (k_bound_rescore): restated here as `query_ok`."""
import ctypes as C

import numpy as np
import pytest

import quiver_amd
from quiver_amd import _lib
from tests import _extremes as X
from tests import _oracle as O
from tests._bound import COSINE, DOT, interval, query_ok
from tests._order import planted_rows, query_for


def check(metric, q, r):
    """-> (unsure, width of the interval); asserts the oracle's distance is covered"""
    unsure, lo, hi, qn = interval(metric, q, r)
    want = np.float32(O.distance(metric, q, r))
    if not query_ok(qn, q.size):
        return True, np.inf                                   # the whole query is handed to the exact scan
    if unsure:
        assert lo == -np.inf and np.isnan(hi)                 # always a candidate, never lowers a threshold
        return True, np.inf
    assert not np.isnan(want), (metric, "a row the rule trusts has no distance", q[:4], r[:4])
    assert lo <= want <= hi, (metric, q.size, float(lo), float(want), float(hi))
    return False, float(hi) - float(lo)


@pytest.mark.parametrize("metric", [COSINE, DOT])
@pytest.mark.parametrize("dim", [16, 128, 768, 1536])
def test_interval_covers_the_oracle_on_ordinary_clustered_tied_and_wide_range_rows(metric, dim):
    rng = np.random.default_rng(100 * dim + metric)
    widths = []
    for t in range(60):
        q = X.unit(rng, dim) if t % 2 else rng.standard_normal(dim).astype(np.float32)
        kind = t % 6
        if kind == 0:
            q = X.unit(rng, dim); r = X.unit(rng, dim)                               # i.i.d. unit rows
        elif kind == 1:
            r = (q * np.float32(1.0 + 1e-3 * rng.standard_normal())).astype(np.float32) + (1e-4 * rng.standard_normal(dim)).astype(np.float32)   # a cluster around the query
        elif kind == 2:
            r = rng.integers(-2, 3, dim).astype(np.float32)                          # ties: small integers, exact in bfloat16 (rres = 0)
        elif kind == 3:
            r = (rng.standard_normal(dim) * 10.0 ** rng.uniform(-6, 6, dim)).astype(np.float32)   # elements over twelve decades
        elif kind == 4:
            s = 10.0 ** rng.integers(-9, 10)
            r = (rng.standard_normal(dim) * s).astype(np.float32); q = (q * np.float32(10.0 ** rng.integers(-9, 10))).astype(np.float32)
        else:
            r = q.copy()                                                             # distance 0: the clamp's neighbourhood
        unsure, w = check(metric, q, r)
        assert not unsure, (metric, dim, kind)
        if kind == 0:
            widths.append(w)
    # the bound is useful, not only safe: on unit rows the interval is a few thousandths wide (2 (|q| rres + gamma |q| (|r| + rres)), rres / |r| <= 2^-9 sqrt... ~ 1.7e-3)
    assert max(widths) < 6e-3, max(widths)


@pytest.mark.parametrize("metric", [COSINE, DOT])
def test_order_sensitive_rows(metric):
    dim = 128
    rng = np.random.default_rng(5)
    q = query_for(metric, dim, rng)
    rows = planted_rows(metric, dim, q, 12, rng)
    assert len(rows) >= 4
    for r in rows:
        unsure, _ = check(metric, q, np.asarray(r, np.float32))
        assert not unsure


@pytest.mark.parametrize("metric", [COSINE, DOT])
@pytest.mark.parametrize("dim", [16, 768])
def test_extreme_rows_and_queries(metric, dim):
    rng = np.random.default_rng(9 + dim)
    ordinary = [X.unit(rng, dim) for _ in range(3)]
    extreme = X.class_rows(rng, dim)
    marked = 0
    for cls, name, v in extreme:
        for o in ordinary:
            unsure, _ = check(metric, o, v)                   # an extreme row under an ordinary query
            marked += unsure
            if cls in "NI" or (cls == "G" and float(name[4:]) >= 1e18) or cls in "ZD":
                assert unsure, (cls, name)                    # not a number, beyond the 1e18 guard, or vanishing: never trusted
            check(metric, v, o)                               # the same vector as the query: covered, or handed back whole
        for _, _, w in extreme[::3]:
            check(metric, v, w)
    assert marked > 0


def test_only_the_scan_metrics():
    lo, hi = C.c_float(0), C.c_float(0)
    assert _lib.lib().qv_scan_bound_interval(1, 16, C.c_float(0), 1.0, 1.0, C.c_float(0), C.byref(lo), C.byref(hi)) == _lib.QV_ERR_UNSUPPORTED
    assert quiver_amd.metric_id("cosine") == COSINE and quiver_amd.metric_id("dot") == DOT
