"""The 6-bit plane behind the single-query bound scan (quiver_amd/csrc/qv_bound.h: bound6_quant / bound6_pack; k_row_state6), checked on the
CPU through the library's host twins: packing and unpacking (qv_scan_quantize_row6 / qv_scan_unpack_row6) against a numpy restatement of the
layout, stage 1's sum from the BIASED codes against the signed sum, and the interval — qv_scan_bound_interval8 with 4 rscale8 and rres6 —
against the oracle's float32 distance for cosine, dot and L2, on the inputs tests/test_bound_scan8_cpu.py uses for the 8-bit plane.  A row or
a query the bound declines must come back "unsure" (-inf, NaN).  The rule is checked through qv_scan_bound6_applies."""
import numpy as np
import pytest

from quiver_amd import _lib
from tests import _oracle as O
from tests import _bound6 as B6
from tests._bound import COSINE, DOT, query_ok
from tests._bound8 import quantize_query, quantize_row

L2 = 1
DIMS = [64, 128, 768, 4096]
FMAX = np.float32(3.4028235e38)


@pytest.mark.parametrize("dim", DIMS)
def test_pack_then_unpack_is_the_identity_for_every_code_at_every_place(dim):
    """64 rows whose element d is 4 c with c = ((d + j) % 64) - 32: every row holds -128, so its 8-bit scale is 128 / 127 (a hair up) and
    r / (4 scale) = c / 1.0079 rounds to c for every |c| <= 32; over the 64 rows every code stands at every place of a group"""
    for j in range(64):
        c = ((np.arange(dim) + j) % 64) - 32
        r = (4.0 * c).astype(np.float32)
        b, sc, res = B6.quantize_row6(r)
        assert abs(float(sc) - 128.0 / 127.0) < 1e-6 and np.isfinite(res)
        want = (c + 32).astype(np.uint8)
        assert np.array_equal(b, B6.pack_numpy(want)), j           # the layout, restated in numpy
        assert np.array_equal(B6.unpack_row6(b), want), j
        e = r.astype(np.float64) - 4.0 * np.float64(sc) * c          # the residual: from the codes, rounded up
        assert float(np.sqrt(np.sum(e * e))) <= float(res) <= float(np.sqrt(np.sum(e * e))) * (1 + 1e-6)
    rng = np.random.default_rng(dim)
    u = rng.integers(0, 64, dim).astype(np.uint8)                    # ... and any codes at all through the unpacker
    assert np.array_equal(B6.unpack_row6(B6.pack_numpy(u)), u)


def test_the_quantiser_keeps_its_promises():
    rng = np.random.default_rng(3)
    for dim in DIMS:
        r = (rng.standard_normal(dim) * 10.0 ** rng.uniform(-3, 3)).astype(np.float32)
        b, sc, res = B6.quantize_row6(r)
        c = B6.unpack_row6(b).astype(np.int64) - 32
        assert c.min() >= -32 and c.max() <= 31
        e = r.astype(np.float64) - 4.0 * np.float64(sc) * c
        n = float(np.sqrt(np.sum(e * e)))
        assert n <= float(res) <= n * (1 + 1e-6)
        assert np.all(np.abs(e) <= 3.0 * float(sc) * (1 + 1e-5))     # half a step of 4 scale; three quarters where +31.75 is clamped to 31
    for bad in (np.zeros(64, np.float32), np.full(64, np.nan, np.float32), np.full(64, 1e-30, np.float32), np.full(64, 1e25, np.float32)):
        assert np.isnan(B6.quantize_row6(bad)[2]) and np.isnan(quantize_row(bad)[2])


@pytest.mark.parametrize("dim", DIMS)
def test_the_sum_from_the_biased_codes_is_the_signed_sum(dim):
    rng = np.random.default_rng(17 + dim)
    for _ in range(4):
        r = rng.standard_normal(dim).astype(np.float32)
        q = (rng.standard_normal(dim) * 10.0 ** rng.uniform(-2, 2)).astype(np.float32)
        u = B6.unpack_row6(B6.quantize_row6(r)[0])
        qq = quantize_query(q)[0]
        assert B6.isum6(qq, u) == int(np.sum(qq * (u.astype(np.int64) - 32)))


def check(metric, q, r):
    """-> (unsure, width); asserts the oracle's float32 distance is covered whenever the rule trusts the pair"""
    q = np.ascontiguousarray(q, np.float32); r = np.ascontiguousarray(r, np.float32)
    unsure, lo, hi, qn = B6.interval6(metric, q, r)
    with np.errstate(all="ignore"):
        want = np.float32(O.distance(metric, q, r))
    if unsure:
        assert lo == -np.inf and np.isnan(hi)                 # always a candidate, never lowers a threshold
        return True, np.inf
    assert query_ok(qn, q.size)
    assert not np.isnan(want), (metric, "a pair the rule trusts has no distance", q[:4], r[:4])
    assert lo <= want <= hi, (metric, q.size, float(lo), float(want), float(hi))
    return False, float(hi) - float(lo)


@pytest.mark.parametrize("metric", [COSINE, DOT, L2])
@pytest.mark.parametrize("dim", DIMS)
def test_interval_covers_the_oracle_on_the_generators_rows(metric, dim):
    rows = O.gen_rows(20260424, 0, 24, dim)
    qs = O.gen_rows(20260425, 0, 3, dim)
    for q in qs:
        for r in rows:
            unsure, w = check(metric, q, r)
            assert not unsure
            if metric == COSINE:
                assert w < 0.32                                   # four times the 8-bit plane's 0.08
    # the model behind the issue's estimate: the half-width at 768 dimensions is about 0.93 sigma of the score distribution (sigma = dim^-1/2)
    if metric == COSINE and dim == 768:
        ws = [check(metric, qs[0], r)[1] / 2 for r in rows]
        assert 0.5 < np.mean(ws) * np.sqrt(dim) < 1.4, np.mean(ws) * np.sqrt(dim)


@pytest.mark.parametrize("metric", [COSINE, DOT, L2])
@pytest.mark.parametrize("dim", DIMS)
def test_interval_on_shaped_rows_and_queries(metric, dim):
    rng = np.random.default_rng(7 * dim + metric)
    base = rng.standard_normal(dim).astype(np.float32)
    ordinary_q = [rng.standard_normal(dim).astype(np.float32), O.gen_rows(20260425, 3, 1, dim)[0]]

    def with_dominant(big, small):
        v = (base * np.float32(small)).astype(np.float32); v[dim // 3] = np.float32(big); return v

    den = (rng.standard_normal(dim) * 1e-41).astype(np.float32)
    den_mixed = base.copy(); den_mixed[::2] = den[::2]
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
            unsure, _ = check(metric, q, r)
            if name in must_decline:
                assert unsure, name
            if name in must_trust:
                assert not unsure, name
            check(metric, r, q)
        for other in list(shaped.values())[::3]:
            check(metric, r, other)
    for big, small in ((1e30, 1.0), (1.0, 1e-30), (100.0, 1.0)):
        q = with_dominant(big, small)
        for r in (base, O.gen_rows(20260424, 5, 1, dim)[0]):
            check(metric, q, r)


@pytest.mark.parametrize("metric", [COSINE, DOT, L2])
@pytest.mark.parametrize("dim", [64, 768])
def test_adversarial_query_along_the_rows_quantisation_error(metric, dim):
    """q along r - 4 rscale8 c6: Cauchy-Schwarz is tight, the margin's first term is attained"""
    rng = np.random.default_rng(31 * dim + metric)
    for t in range(6):
        r = (rng.standard_normal(dim) * (1.0 if t % 2 else 10.0 ** rng.uniform(-3, 3))).astype(np.float32)
        b, sc, res = B6.quantize_row6(r)
        assert np.isfinite(res)
        e = r.astype(np.float64) - 4.0 * np.float64(sc) * (B6.unpack_row6(b).astype(np.float64) - 32.0)
        for q in (np.sign(e), -np.sign(e), e / np.linalg.norm(e), -e / np.linalg.norm(e), e / np.linalg.norm(e) + 1e-3 * r / np.linalg.norm(r)):
            q = q.astype(np.float32)
            if not np.any(q):
                continue
            unsure, _ = check(metric, q, r)
            assert not unsure


def test_the_rule_never_says_yes_where_the_8bit_rule_says_no():
    f6, f8 = _lib.lib().qv_scan_bound6_applies, _lib.lib().qv_scan_bound8_applies
    yes = 0
    for metric in (COSINE, DOT, 0x101):                              # (0x101: QV_RULE_L2_PLANES)
        for dim in (64, 80, 128, 768, 1536, 4048, 4096):
            for rows in (500, 20011, 300_000, 1_000_000, 3_000_000, 10_000_000):
                for nq in (1, 2):
                    for k in (1, 10, 64, 65):
                        for mode in (0, 1, 2):
                            for pm in (0, 1, 2):
                                for p6 in (0, 1, 2):
                                    for h8, h6 in ((1, 1), (1, 0), (0, 1)):
                                        a = f6(metric, dim, rows, nq, k, mode, pm, p6, h8, h6)
                                        assert a in (0, 1)
                                        if a:
                                            yes += 1
                                            assert f8(metric, dim, rows, nq, k, mode, pm, h8) == 1
                                            assert nq == 1 and dim % 64 == 0 and h8 and h6 and p6 != 2
    assert yes > 0
    assert f6(COSINE, 768, 20011, 1, 10, 1, 1, 1, 1, 1) == 1            # forced: wherever the 8-bit stage is taken, the plane held
    assert f6(COSINE, 80, 20011, 1, 10, 1, 1, 1, 1, 1) == 0 and f6(COSINE, 4048, 20011, 1, 10, 1, 1, 1, 1, 1) == 0   # not whole 64-dimension groups (4032 is 63 of them)
    assert f6(COSINE, 768, 20011, 1, 10, 1, 1, 2, 1, 1) == 0 and f6(COSINE, 768, 20011, 1, 10, 1, 1, 1, 1, 0) == 0
    assert f6(COSINE, 768, 20011, 1, 10, 1, 1, 0, 1, 1) == 0            # automatic: never below the 8-bit floor
    # automatic: the measured cells (profiles/LAB_r20_bound_scan6.md) — 10M rows, 128 <= dim < 1536 in whole groups, k <= 10
    for dim, rows, k, want in ((768, 10_000_000, 10, 1), (768, 10_000_000, 1, 1), (768, 10_000_000, 11, 0), (768, 10_000_000, 64, 0), (768, 9_999_999, 10, 0), (768, 3_000_000, 1, 0),
                               (128, 10_000_000, 10, 1), (64, 10_000_000, 10, 0), (1536, 10_000_000, 10, 0), (1472, 10_000_000, 10, 1)):
        assert f6(COSINE, dim, rows, 1, k, 0, 0, 0, 1, 1) == want, (dim, rows, k)
    assert f6(COSINE, 768, 1000, 1, 10, 3, 1, 1, 1, 1) < 0 and f6(COSINE, 768, 1000, 1, 10, 0, 3, 1, 1, 1) < 0 and f6(COSINE, 768, 1000, 1, 10, 0, 1, 3, 1, 1) < 0
