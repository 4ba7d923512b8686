"""The interval behind the 8-bit stage of the single-query bound scan (quiver_amd/csrc/qv_bound.h: bound_scan_interval8), checked on the
CPU: the row's bytes, scale and residual come from the library's own quantiser compiled for the host (qv_scan_quantize_row8), stage 1's
sum is the integer dot product of the split query with those bytes (numpy integers: exact, as the device's), and the library's interval
function (qv_scan_bound_interval8) turns it into [d_lo, d_hi].  For every row the rule does not mark "unsure" the oracle's float32
distance must lie in the interval; a row or a query the bound declines must come back "unsure" (always a candidate, never in a
threshold), never with a wrong interval.  The dispatch's rule is checked through qv_scan_bound8_applies."""
import numpy as np
import pytest

from quiver_amd import _lib
from tests import _oracle as O
from tests._bound import COSINE, DOT, query_ok
from tests._bound8 import interval8, quantize_row

DIMS = [16, 128, 768, 4096]
FMAX = np.float32(3.4028235e38)


def check(metric, q, r):
    """-> (unsure, width); asserts the oracle's float32 distance is covered whenever the rule trusts the pair"""
    q = np.ascontiguousarray(q, np.float32); r = np.ascontiguousarray(r, np.float32)
    unsure, lo, hi, qn = interval8(metric, q, r)
    with np.errstate(all="ignore"):
        want = np.float32(O.distance(metric, q, r))
    if unsure:
        assert lo == -np.inf and np.isnan(hi)                 # always a candidate, never lowers a threshold
        return True, np.inf
    assert query_ok(qn, q.size)                               # a query the re-score would hand on is never trusted by stage 1
    assert not np.isnan(want), (metric, "a pair the rule trusts has no distance", q[:4], r[:4])
    assert lo <= want <= hi, (metric, q.size, float(lo), float(want), float(hi))
    return False, float(hi) - float(lo)


@pytest.mark.parametrize("metric", [COSINE, DOT])
@pytest.mark.parametrize("dim", DIMS)
def test_interval_covers_the_oracle_on_the_generators_rows(metric, dim):
    rows = O.gen_rows(20260424, 0, 24, dim)
    qs = O.gen_rows(20260425, 0, 3, dim)
    widths = []
    for q in qs:
        for r in rows:
            unsure, w = check(metric, q, r)
            assert not unsure
            widths.append(w)
    # useful, not only safe: the row residual is about dim^-1/2 * 0.29 * sqrt(dim) / 127 of a unit row's largest element — an
    # interval of a few hundredths of |q||r| at most
    qn = float(np.linalg.norm(qs[0].astype(np.float64))); rn = float(np.linalg.norm(rows[0].astype(np.float64)))
    assert max(widths) < 0.08 * (1.0 if metric == COSINE else qn * rn * 1.5), max(widths)


@pytest.mark.parametrize("metric", [COSINE, DOT])
@pytest.mark.parametrize("dim", DIMS)
def test_interval_on_shaped_rows_and_queries(metric, dim):
    rng = np.random.default_rng(7 * dim + metric)
    base = rng.standard_normal(dim).astype(np.float32)
    ordinary_q = [rng.standard_normal(dim).astype(np.float32), O.gen_rows(20260425, 3, 1, dim)[0]]

    def with_dominant(big, small):
        v = (base * np.float32(small)).astype(np.float32); v[dim // 3] = np.float32(big); return v

    den = (rng.standard_normal(dim) * 1e-41).astype(np.float32)          # denormal elements ...
    den_mixed = base.copy(); den_mixed[::2] = den[::2]                     # ... and denormal beside ordinary ones
    shaped = {
        "dominant 1e30 beside O(1)": with_dominant(1e30, 1.0),
        "dominant 1 beside 1e-30": with_dominant(1.0, 1e-30),
        "constant": np.full(dim, np.float32(0.75)),
        "constant negative": np.full(dim, np.float32(-3.0)),
        "+-max only": (np.where(rng.integers(0, 2, dim) > 0, 1.0, -1.0) * 2.5).astype(np.float32),
        "+-FLT_MAX only": (np.where(rng.integers(0, 2, dim) > 0, 1.0, -1.0) * FMAX).astype(np.float32),
        "denormal": den,
        "denormal beside ordinary": den_mixed,
        "zero": np.zeros(dim, np.float32),
        "huge": (base * np.float32(1e20)).astype(np.float32),
        "vanishing": (base * np.float32(1e-25)).astype(np.float32),
        "nan": np.where(np.arange(dim) == 1, np.float32(np.nan), base).astype(np.float32),
        "inf": np.where(np.arange(dim) == 2, np.float32(np.inf), base).astype(np.float32),
    }
    must_decline = {"+-FLT_MAX only", "denormal", "zero", "huge", "vanishing", "nan", "inf", "dominant 1e30 beside O(1)"}
    must_trust = {"dominant 1 beside 1e-30", "constant", "constant negative", "+-max only", "denormal beside ordinary"}
    for name, r in shaped.items():
        for q in ordinary_q:
            unsure, _ = check(metric, q, r)                   # a shaped row under an ordinary query
            if name in must_decline:
                assert unsure, name
            if name in must_trust:
                assert not unsure, name
            check(metric, r, q)                               # the same vector as the query: covered, or declined whole
        for other in list(shaped.values())[::3]:
            check(metric, r, other)
    # queries with one dominant element over ordinary rows: the other elements fall below the query's quantum and count in qres
    for big, small in ((1e30, 1.0), (1.0, 1e-30), (100.0, 1.0)):
        q = with_dominant(big, small)
        for r in (base, O.gen_rows(20260424, 5, 1, dim)[0]):
            check(metric, q, r)


@pytest.mark.parametrize("metric", [COSINE, DOT])
@pytest.mark.parametrize("dim", DIMS)
def test_adversarial_query_along_the_rows_quantisation_error(metric, dim):
    """q = sign(r - r8) and its negative: q . (r - r8) = |r - r8|_1, and for q = (r - r8) / |r - r8| Cauchy-Schwarz is tight — the margin's
    first term is attained, so an interval a hair too narrow fails here"""
    rng = np.random.default_rng(31 * dim + metric)
    for t in range(6):
        r = (rng.standard_normal(dim) * (1.0 if t % 2 else 10.0 ** rng.uniform(-3, 3))).astype(np.float32)
        r8, sc, res = quantize_row(r)
        assert np.isfinite(res)
        e = r.astype(np.float64) - np.float64(sc) * r8.astype(np.float64)
        for q in (np.sign(e), -np.sign(e), e / np.linalg.norm(e), -e / np.linalg.norm(e), e / np.linalg.norm(e) + 1e-3 * r / np.linalg.norm(r)):
            q = q.astype(np.float32)
            if not np.any(q):
                continue
            unsure, _ = check(metric, q, r)
            assert not unsure


def test_the_quantiser_keeps_its_promises():
    rng = np.random.default_rng(3)
    for dim in DIMS:
        r = rng.standard_normal(dim).astype(np.float32)
        r8, sc, res = quantize_row(r)
        assert r8.min() >= -127 and r8.max() <= 127 and max(abs(int(r8.min())), int(r8.max())) == 127
        assert float(sc) >= float(np.max(np.abs(r))) / 127.0                                   # the scale is rounded up
        e = r.astype(np.float64) - np.float64(sc) * r8.astype(np.float64)
        assert float(res) >= float(np.sqrt(np.sum(e * e))) and float(res) <= float(np.sqrt(np.sum(e * e))) * (1 + 1e-6)   # from the bytes, rounded up
        assert np.all(np.abs(e) <= 0.5 * float(sc) * (1 + 1e-6))
    for bad in (np.zeros(16, np.float32), np.full(16, np.nan, np.float32), np.full(16, 1e-30, np.float32), np.full(16, 1e25, np.float32)):
        assert np.isnan(quantize_row(bad)[2])


def test_rule_respects_the_floors_and_the_opt_outs():
    f = _lib.lib().qv_scan_bound8_applies
    AUTO, ALWAYS, NEVER = 0, 1, 2
    P_AUTO, P_8BIT, P_BF16 = 0, 1, 2
    bound = _lib.lib().qv_scan_bound_applies
    for metric in (COSINE, DOT):
        # forced: wherever the bound scan itself takes one query, and only there
        assert f(metric, 768, 20011, 1, 10, ALWAYS, P_8BIT, 1) == 1
        assert f(metric, 768, 20011, 1, 10, AUTO, P_8BIT, 1) == 0            # the bound scan's own floor (300 000 rows) holds
        assert f(metric, 768, 300000, 1, 10, AUTO, P_8BIT, 1) == 1
        assert f(metric, 768, 10_000_000, 1, 10, NEVER, P_8BIT, 1) == 0
        assert f(metric, 768, 10_000_000, 1, 10, ALWAYS, P_BF16, 1) == 0
        assert f(metric, 768, 10_000_000, 1, 10, ALWAYS, P_8BIT, 0) == 0     # no plane (QV_FLAG_NO_SCAN_PLANE, a failed allocation)
        assert f(metric, 100, 10_000_000, 1, 10, ALWAYS, P_8BIT, 1) == 0     # not whole 16-dimension steps
        assert f(metric, 4112, 10_000_000, 1, 10, ALWAYS, P_8BIT, 1) == 0    # beyond the int32 sums
        assert f(metric, 768, 7 * 64, 1, 10, ALWAYS, P_8BIT, 1) == 0         # fewer than 8 tiles
        assert f(metric, 768, 10_000_000, 1, 65, ALWAYS, P_8BIT, 1) == 0
        for nq in (2, 4, 8):
            assert f(metric, 768, 10_000_000, nq, 10, ALWAYS, P_8BIT, 1) == 0   # shared passes stay on the bfloat16 copy
        # automatic: never below the bound scan's floor, whatever forces the bound scan itself — what runs at or below 200 k rows is unchanged
        for rows in (20011, 100_000, 200_000, 299_999):
            for mode in (AUTO, ALWAYS):
                assert f(metric, 768, rows, 1, 10, mode, P_AUTO, 1) == 0
        assert f(metric, 768, 10_000_000, 1, 10, AUTO, P_AUTO, 1) == 1       # the headline shape
        # the measured floors: 3M rows of 768 dimensions or more, 10M rows from 128 dimensions, nothing narrower
        assert f(metric, 768, 3_000_000, 1, 64, AUTO, P_AUTO, 1) == 1 and f(metric, 768, 2_999_999, 1, 1, AUTO, P_AUTO, 1) == 0
        assert f(metric, 1536, 3_000_000, 1, 10, ALWAYS, P_AUTO, 1) == 1
        assert f(metric, 128, 10_000_000, 1, 10, AUTO, P_AUTO, 1) == 1 and f(metric, 128, 3_000_000, 1, 10, AUTO, P_AUTO, 1) == 0
        assert f(metric, 752, 3_000_000, 1, 10, AUTO, P_AUTO, 1) == 0 and f(metric, 64, 10_000_000, 1, 10, AUTO, P_AUTO, 1) == 0
        # wherever the 8-bit stage applies the bound scan does (it hands on to the bfloat16 stage)
        for rows in (20011, 300_000, 10_000_000):
            for dim in (16, 128, 768, 4096):
                for mode in (AUTO, ALWAYS):
                    for pm in (P_AUTO, P_8BIT):
                        if f(metric, dim, rows, 1, 10, mode, pm, 1) == 1:
                            assert bound(metric, dim, rows, 1, 10, mode, 1) == 1
    assert f(1, 768, 10_000_000, 1, 10, ALWAYS, P_8BIT, 1) == 0              # an L2 index
    assert f(COSINE, 768, 1000, 1, 10, 3, P_8BIT, 1) < 0 and f(COSINE, 768, 1000, 1, 10, AUTO, 3, 1) < 0
