"""The Euclidean interval of the bound scan (quiver_amd/csrc/qv_bound.h: the QV_L2 forms of bound_scan_interval and bound_scan_interval8),
its rule code (QV_RULE_L2_PLANES) and stage 1's model on the corpora the GPU tests search — all on the CPU.

Containment (the bfloat16 form through qv_scan_bound_interval_l2, the 8-bit form through qv_scan_bound_interval8 with QV_L2): the stage-1 inputs are formed as tests/test_bound_scan_cpu.py and tests/test_bound_scan8_cpu.py form them (the float32 chain over
bf16(r); the integer sum over qv_scan_quantize_row8's bytes; the chain norms), the reference is qv_distance_pair(QV_L2) cross-checked
against a plain numpy restatement of distances.go:48-54, and d_lo <= ref <= d_hi must hold as float32 — with every shaped case coming
back "sure", so a function that always answers "unsure" fails.  Not vacuous: d_hi^2 - d_lo^2 <= 4 m + 6e-7 (|q| + |r|)^2 with the margin m
recomputed here from qv_bound.h's formulas (4 m, twice theta = 1.2e-7, both float32 roundings of the ends).

Rules: under the forced modes — the bound scan ALWAYS / NEVER, the plane knobs 8-bit / bfloat16 — every rule function answers for
QV_RULE_L2_PLANES what it answers for QV_DOT; plain QV_L2 answers 0 everywhere; an unknown code is an error for qv_scan_route.  The
AUTOMATIC modes take the cells measured for the Euclidean distance and no other (profiles/LAB_r14_bound_scan_l2.md)."""
import itertools

import numpy as np
import pytest

from quiver_amd import _lib
from tests import _bound as B
from tests import _bound8 as B8
from tests import _bound_l2 as L
from tests import _oracle as O
from tests import _tight as T

L2, DOT, COSINE = L.L2, B.DOT, B.COSINE
DIMS = [16, 128, 768, 4096]
TINY = 1.0e-14                                     # filter_tiny_norm at every dimension up to 4096 (sqrt(dim * 2.4e-32) stays below it)


def reference(q, r):
    with np.errstate(all="ignore"):
        want = np.float32(O.distance(L2, q, r))
    mine = L.euclid_numpy(q, r)
    assert want.view(np.uint32) == mine.view(np.uint32) or (np.isnan(want) and np.isnan(mine)), (want, mine)
    return want


def check(q, r, sure=True):
    """both forms for one pair: containment, and the width against the margin; -> ((d_lo, d_hi) of the bfloat16 form, of the 8-bit form)"""
    q = np.ascontiguousarray(q, np.float32); r = np.ascontiguousarray(r, np.float32)
    want = reference(q, r)
    out = []
    for form, interval, margin in (("bf16", L.interval, L.margin16), ("8bit", lambda a, b: B8.interval8(L2, a, b), L.margin8)):
        unsure, lo, hi, _ = interval(q, r)
        if not sure:
            assert unsure and lo == -np.inf and np.isnan(hi), (form, unsure, lo, hi)
            out.append((lo, hi))
            continue
        assert not unsure, (form, q[:3], r[:3])
        assert lo <= want <= hi, (form, q.size, float(lo), float(want), float(hi))
        m, qn, rn = margin(q, r)
        width = float(hi) ** 2 - float(lo) ** 2
        assert width <= 4.0 * m + 6e-7 * (qn + rn) ** 2, (form, q.size, width, m, qn, rn)
        out.append((lo, hi))
    return out


@pytest.mark.parametrize("dim", DIMS)
def test_gaussian_and_unit_rows(dim):
    rng = np.random.default_rng(90 + dim)
    n = 12 if dim <= 768 else 6
    for scale in (1.0, None):                                              # Gaussian as drawn; every vector scaled to unit length
        qs = rng.standard_normal((2, dim)); rows = rng.standard_normal((n, dim))
        if scale is None:
            qs /= np.linalg.norm(qs, axis=1)[:, None]; rows /= np.linalg.norm(rows, axis=1)[:, None]
        for q in qs.astype(np.float32):
            for r in rows.astype(np.float32):
                check(q, r)
    for q in O.gen_rows(20260425, 0, 2, dim):                             # the generator's unit rows
        for r in O.gen_rows(20260424, 0, n, dim):
            check(q, r)


@pytest.mark.parametrize("dim", DIMS)
def test_a_row_equal_to_the_query_and_its_single_ulp_neighbours(dim):
    rng = np.random.default_rng(91 + dim)
    for scale in (1.0, 37.5, 1e-3):
        q = (rng.standard_normal(dim) * scale).astype(np.float32)
        (lo, _), (lo8, _) = check(q, q.copy())
        assert reference(q, q) == 0.0 and lo == 0.0 and lo8 == 0.0      # exactly: E_lo <= 0 is clamped before the square root
        up = np.nextafter(q, np.float32(np.inf)); down = np.nextafter(q, np.float32(-np.inf))
        for r in (up, down, np.where(rng.random(dim) < 0.5, up, down), np.where(np.arange(dim) == dim // 2, up, q)):
            assert reference(q, r) > 0.0
            check(q, r.astype(np.float32)); check(r.astype(np.float32), q)


@pytest.mark.parametrize("dim", DIMS)
def test_rows_with_the_largest_bfloat16_residual(dim):
    """tests/_tight.halfway: every element half way between two bfloat16 values — and such a query, and near-copies of one another"""
    rng = np.random.default_rng(92 + dim)
    q = rng.standard_normal(dim).astype(np.float32)
    for r in (T.halfway(rng.standard_normal(dim).astype(np.float32)), T.halfway(q), T.halfway((q * np.float32(1.001)).astype(np.float32)), T.of_kind(q, 4, rng)):
        check(q, r); check(T.halfway(q), r); check(r, q)


@pytest.mark.parametrize("dim", DIMS)
def test_differences_that_all_round_the_same_way(dim):
    """q_i = 1, r_i = -3 * 2^-25: every float32 difference 1 + 0.75 ulp rounds UP by a quarter ulp (and -2^-25, -5 * 2^-25: down) — the
    relative error of D reaches its bound's order, 2^-25 .. 2^-24 per element, all of one sign"""
    one = np.ones(dim, np.float32)
    for t in (-3.0 * 2.0 ** -25, -1.0 * 2.0 ** -25, -5.0 * 2.0 ** -25, 3.0 * 2.0 ** -25):
        r = np.full(dim, t, np.float32)
        assert float(r[0]) == t
        check(one, r); check(r, one)
        check((one * np.float32(3.0)).astype(np.float32), (r * np.float32(3.0)).astype(np.float32))


@pytest.mark.parametrize("dim", DIMS)
def test_norms_six_orders_of_magnitude_apart(dim):
    rng = np.random.default_rng(93 + dim)
    a = rng.standard_normal(dim).astype(np.float32); b = (rng.standard_normal(dim) * 1e-6).astype(np.float32)
    check(a, b); check(b, a)
    check((a * np.float32(1e6)).astype(np.float32), rng.standard_normal(dim).astype(np.float32))
    check(rng.standard_normal(dim).astype(np.float32), (a * np.float32(1e6)).astype(np.float32))


def with_norm(v, norm):
    v64 = v.astype(np.float64)
    return (v64 * (norm / np.linalg.norm(v64))).astype(np.float32)


@pytest.mark.parametrize("dim", DIMS)
def test_norms_just_inside_the_range_the_bound_works_with(dim):
    """bound_scan_norm_ok: filter_tiny_norm <= |v| < 1e18, at both ends, for the row, for the query, and for both"""
    rng = np.random.default_rng(94 + dim)
    g, h = rng.standard_normal(dim).astype(np.float32), rng.standard_normal(dim).astype(np.float32)
    small, big = with_norm(g, TINY * 1.001), with_norm(g, 0.999e18)
    small2, big2 = with_norm(h, TINY * 1.001), with_norm(h, 0.999e18)
    for v in (small, big, small2, big2):
        assert B.query_ok(B.chain_norm(v), dim)
    for q, r in ((h, small), (h, big), (small, h), (big, h), (small, small2), (big, big2), (small2, big), (big2, small)):
        check(q, r)


@pytest.mark.parametrize("dim", DIMS)
def test_what_the_bound_declines_comes_back_unsure(dim):
    rng = np.random.default_rng(95 + dim)
    q = rng.standard_normal(dim).astype(np.float32); base = rng.standard_normal(dim).astype(np.float32)
    nan_row = np.where(np.arange(dim) == 1, np.float32(np.nan), base).astype(np.float32)
    for r in (nan_row, np.zeros(dim, np.float32), (base * np.float32(1e20)).astype(np.float32)):
        check(q, r, sure=False)
    # a zero query is legitimate for the Euclidean distance, but its norm is not one the bound works with: the 8-bit form declines every row
    # under it, and the re-score hands such a query back whole (tests/_bound.query_ok) — the bfloat16 form, which never sees the
    # query's norm rule, must still not answer wrongly
    zero = np.zeros(dim, np.float32)
    unsure, lo, hi, qn = B8.interval8(L2, zero, base)
    assert unsure and lo == -np.inf and np.isnan(hi) and not B.query_ok(qn, dim)
    unsure, lo, hi, qn = L.interval(zero, base)
    assert not B.query_ok(qn, dim) and (unsure or lo <= reference(zero, base) <= hi)


def test_which_entry_point_takes_which_metric():
    """qv_scan_bound_interval8 takes the three metrics; qv_scan_bound_interval keeps cosine and dot — it has always answered "unsupported" for
    QV_L2, and tests/test_bound_scan_cpu.py holds it to that — and the Euclidean interval has qv_scan_bound_interval_l2"""
    lib = _lib.lib()
    import ctypes as C
    lo, hi = C.c_float(0), C.c_float(0)
    for metric in (COSINE, L2, DOT):
        assert lib.qv_scan_bound_interval8(metric, 16, 1000, 1e-4, 1.0, 1e-4, 1.0, C.c_float(1e-2), C.c_float(1e-3), C.byref(lo), C.byref(hi)) == 0
    for metric in (COSINE, DOT):
        assert lib.qv_scan_bound_interval(metric, 16, C.c_float(0.5), 1.0, 1.0, C.c_float(1e-3), C.byref(lo), C.byref(hi)) == 0
    assert lib.qv_scan_bound_interval_l2(16, C.c_float(0.5), 1.0, 1.0, C.c_float(1e-3), C.byref(lo), C.byref(hi)) == 0
    assert 0.0 < lo.value < 1.0 < hi.value < 1.1                          # |q| = |r| = 1, q.r about 0.5: a distance of about 1
    assert lib.qv_scan_bound_interval_l2(0, C.c_float(0.5), 1.0, 1.0, C.c_float(1e-3), C.byref(lo), C.byref(hi)) < 0
    for metric in (L2, 2, 4, 5, 6, 7, 8, L.RULE_L2_PLANES):
        assert lib.qv_scan_bound_interval(metric, 16, C.c_float(0.5), 1.0, 1.0, C.c_float(1e-3), C.byref(lo), C.byref(hi)) == -8      # QV_ERR_UNSUPPORTED
        assert b"cosine, dot and l2" in lib.qv_last_error()
    for metric in (2, 4, 5, 6, 7, 8, L.RULE_L2_PLANES):
        assert lib.qv_scan_bound_interval8(metric, 16, 1000, 1e-4, 1.0, 1e-4, 1.0, C.c_float(1e-2), C.c_float(1e-3), C.byref(lo), C.byref(hi)) == -8
        assert b"cosine, dot and l2" in lib.qv_last_error()


# ---- the rules ---------------------------------------------------------------------------------------------------------------------
AUTO, ALWAYS, NEVER = 0, 1, 2
P_AUTO, P_8BIT, P_BF16 = 0, 1, 2
NOFILTER = 0xFFFFFFFF
# the grid of tests/test_bound_scan_mq_cpu.py
GRID = list(itertools.product((16, 128, 768, 4096), (600, 20_011, 530_000, 1_000_000, 10_000_000), (1, 2, 4, 5, 8), (1, 10, 64)))


def rule_answers(metric, dim, rows, nq, k, mode, pm, ct):
    """every rule function's answer for one cell, with the planes held"""
    lib = _lib.lib()
    out = (lib.qv_scan_bound_applies(metric, dim, rows, nq, k, mode, 1),
           lib.qv_scan_bound_applies_filtered(metric, dim, rows, nq, k, mode, 1, ct),
           lib.qv_scan_bound8_applies(metric, dim, rows, nq, k, mode, pm, 1),
           lib.qv_scan_bound8_applies_filtered(metric, dim, rows, nq, k, mode, pm, 1, ct),
           lib.qv_scan_bound8_applies_mq(metric, dim, rows, nq, k, mode, pm, 1),
           lib.qv_scan_bound8_applies_filtered_mq(metric, dim, rows, nq, k, mode, pm, 1, ct))
    assert all(x in (0, 1) for x in out), out
    return out


def test_the_rule_code_answers_as_dot_under_the_forced_modes_and_plain_l2_never():
    took = 0
    for dim, rows, nq, k in GRID:
        tiles = (rows + 63) // 64
        for mode, pm, ct in itertools.product((ALWAYS, NEVER), (P_8BIT, P_BF16), (tiles, max(tiles // 10, 1), 0)):
            dot = rule_answers(DOT, dim, rows, nq, k, mode, pm, ct)
            assert rule_answers(L.RULE_L2_PLANES, dim, rows, nq, k, mode, pm, ct) == dot, (dim, rows, nq, k, mode, pm, ct)
            assert rule_answers(L2, dim, rows, nq, k, mode, pm, ct) == (0,) * 6
            took += sum(dot)
        for mode, pm in itertools.product((AUTO, ALWAYS, NEVER), (P_AUTO, P_8BIT, P_BF16)):
            assert rule_answers(L2, dim, rows, nq, k, mode, pm, tiles) == (0,) * 6
    assert took > 1000                                                     # (the comparison is not one of zeros)
    lib = _lib.lib()
    for nq in (1, 4):                                                      # the conditions every metric shares
        assert lib.qv_scan_bound_applies(L.RULE_L2_PLANES, 100, 1_000_000, nq, 10, ALWAYS, 1) == 0
        assert lib.qv_scan_bound_applies(L.RULE_L2_PLANES, 128, 1_000_000, nq, 65, ALWAYS, 1) == 0
        assert lib.qv_scan_bound_applies(L.RULE_L2_PLANES, 128, 1_000_000, nq, 10, ALWAYS, 0) == 0
        assert lib.qv_scan_bound_applies(L.RULE_L2_PLANES, 128, 400, nq, 10, ALWAYS, 1) == 0


def test_the_automatic_modes_take_the_measured_cells_only():
    """profiles/LAB_r14_bound_scan_l2.md: measured at 768 dimensions (300 k, 1M, 3M, 10M rows) and at 10M x 128, 1 / 2 / 4 / 8 queries, unfiltered and
    under a filter the host counts as every tile a candidate.  Every kept cell is one dot's floors keep too; two kinds of cell dot keeps were
    not measured for the Euclidean distance and are declined: one unfiltered query on rows narrower than 768 dimensions below 10M rows, and
    filtered searches with fewer than nine tenths of the tiles holding a candidate."""
    lib = _lib.lib()
    took = differ = 0
    for dim, rows, nq, k in GRID:
        tiles = (rows + 63) // 64
        for mode, pm, ct in itertools.product((AUTO, ALWAYS), (P_AUTO, P_8BIT, P_BF16), (tiles, max(tiles // 10, 1), 0)):
            if mode == ALWAYS and pm != P_AUTO:
                continue                                                   # (the forced cells: the test above)
            dot = rule_answers(DOT, dim, rows, nq, k, mode, pm, ct)
            l2 = rule_answers(L.RULE_L2_PLANES, dim, rows, nq, k, mode, pm, ct)
            assert all(a <= b for a, b in zip(l2, dot)), (dim, rows, nq, k, mode, pm, ct, l2, dot)      # never a cell dot declines
            narrow_one = nq == 1 and dim < 768 and not (dim >= 128 and rows >= 10_000_000)
            sparse = ct * 10 < tiles * 9
            want = list(dot)
            if mode == AUTO:
                if narrow_one:
                    want[0] = 0
                if sparse or narrow_one:
                    want[1] = 0
                if narrow_one:
                    want[2] = 0
                if sparse or narrow_one:
                    want[3] = want[5] = 0
            assert list(l2) == want, (dim, rows, nq, k, mode, pm, ct, l2, dot, want)
            took += sum(l2); differ += l2 != dot
    assert took > 300 and differ > 20
    f = lib.qv_scan_bound_applies
    for k in (1, 10, 64):
        # one query, the bfloat16 stage: from 300 k rows of 768 dimensions, from 10M rows of 128; nothing narrower, nothing between at 1M
        assert f(L.RULE_L2_PLANES, 768, 300_000, 1, k, AUTO, 1) == 1 and f(L.RULE_L2_PLANES, 768, 299_999, 1, k, AUTO, 1) == 0
        assert f(L.RULE_L2_PLANES, 128, 10_000_000, 1, k, AUTO, 1) == 1 and f(L.RULE_L2_PLANES, 128, 1_000_000, 1, k, AUTO, 1) == 0
        assert f(DOT, 128, 1_000_000, 1, k, AUTO, 1) == 1 and f(L.RULE_L2_PLANES, 112, 10_000_000, 1, k, AUTO, 1) == 0
        # shared passes: dot's floors, every one a measured win
        assert f(L.RULE_L2_PLANES, 768, 300_000, 4, k, AUTO, 1) == 1 and f(L.RULE_L2_PLANES, 768, 300_000, 8, k, AUTO, 1) == 0
        assert f(L.RULE_L2_PLANES, 768, 1_000_000, 8, k, AUTO, 1) == 1 and f(L.RULE_L2_PLANES, 128, 10_000_000, 8, k, AUTO, 1) == 1
        # the headline cell, 8-bit first; 1M x 768 loses at k = 64 and stays on the bfloat16 copy at every k
        assert lib.qv_scan_bound8_applies(L.RULE_L2_PLANES, 768, 10_000_000, 1, k, AUTO, P_AUTO, 1) == 1
        assert lib.qv_scan_bound8_applies(L.RULE_L2_PLANES, 768, 3_000_000, 1, k, AUTO, P_AUTO, 1) == 1
        assert lib.qv_scan_bound8_applies(L.RULE_L2_PLANES, 768, 1_000_000, 1, k, AUTO, P_AUTO, 1) == 0
        assert lib.qv_scan_bound8_applies_mq(L.RULE_L2_PLANES, 128, 10_000_000, 8, k, AUTO, P_AUTO, 1) == 0       # a loss at k = 64
        assert lib.qv_scan_bound8_applies_mq(L.RULE_L2_PLANES, 128, 10_000_000, 4, k, AUTO, P_AUTO, 1) == 1
        # filtered: only with nine tenths of the tiles holding a candidate
        t = (10_000_000 + 63) // 64
        assert lib.qv_scan_bound_applies_filtered(L.RULE_L2_PLANES, 768, 10_000_000, 1, k, AUTO, 1, t) == 1
        assert lib.qv_scan_bound_applies_filtered(L.RULE_L2_PLANES, 768, 10_000_000, 1, k, AUTO, 1, t // 2) == 0
        assert lib.qv_scan_bound_applies_filtered(DOT, 768, 10_000_000, 1, k, AUTO, 1, t // 2) == 1
    # the grids of the other tests stay below every floor: tests/test_gpu_bound_scan_l2.py runs under "always"
    assert f(L.RULE_L2_PLANES, 768, 50_000, 1, 10, AUTO, 1) == 0


def test_routes():
    lib = _lib.lib()
    for dim, rows, nq, k in GRID:
        for pm, ct in itertools.product((P_8BIT, P_BF16), (NOFILTER, (rows + 63) // 64)):
            dot = lib.qv_scan_route_ex(DOT, dim, rows, nq, k, 256, 1, ALWAYS, pm, 1, 1, ct, pm)
            got = lib.qv_scan_route_ex(L.RULE_L2_PLANES, dim, rows, nq, k, 256, 1, ALWAYS, pm, 1, 1, ct, pm)
            if dot in (1, 5, 6):
                assert got == dot, (dim, rows, nq, k, pm, ct, dot, got)
            else:
                assert got not in (1, 5, 6)
            assert lib.qv_scan_route_ex(L.RULE_L2_PLANES, dim, rows, nq, k, 256, 1, NEVER, pm, 1, 1, ct, pm) not in (1, 5, 6)
            auto = lib.qv_scan_route_ex(L.RULE_L2_PLANES, dim, rows, nq, k, 256, 1, AUTO, pm, 1, 1, ct, pm)
            assert auto not in (1, 5, 6) or lib.qv_scan_route_ex(DOT, dim, rows, nq, k, 256, 1, AUTO, pm, 1, 1, ct, pm) == auto
            plain = lib.qv_scan_route_ex(L2, dim, rows, nq, k, 256, 1, ALWAYS, pm, 1, 1, ct, pm)
            assert plain >= 0 and plain not in (1, 5, 6)
            assert lib.qv_scan_route(L.RULE_L2_PLANES, dim, rows, nq, k, 256, 1, ALWAYS, pm, 1, 1, ct) == lib.qv_scan_route(DOT, dim, rows, nq, k, 256, 1, ALWAYS, pm, 1, 1, ct) or dot not in (1, 5, 6)
    assert lib.qv_scan_route(L.RULE_L2_PLANES, 768, 20_011, 1, 10, 256, 1, ALWAYS, P_8BIT, 1, 1, NOFILTER) == 6
    assert lib.qv_scan_route(L.RULE_L2_PLANES, 768, 20_011, 1, 10, 256, 1, ALWAYS, P_BF16, 1, 1, NOFILTER) == 5
    assert lib.qv_scan_route(L.RULE_L2_PLANES, 768, 20_011, 4, 10, 256, 1, ALWAYS, P_BF16, 1, 1, NOFILTER) == 1
    assert lib.qv_scan_route(L.RULE_L2_PLANES, 768, 10_000_000, 1, 10, 256, 1, AUTO, P_AUTO, 1, 1, NOFILTER) == 6     # the headline cell
    assert lib.qv_scan_route(L2, 768, 10_000_000, 1, 10, 256, 1, AUTO, P_AUTO, 1, 1, NOFILTER) not in (1, 5, 6)
    for code in (0x100, 0x102, 9, -1):
        assert lib.qv_scan_route(code, 768, 20_011, 1, 10, 256, 1, ALWAYS, P_8BIT, 1, 1, NOFILTER) < 0


# ---- stage 1 on the GPU tests' corpora ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(L.CORPORA))
def test_stage_one_model_of_the_gpu_corpora(name):
    """the survivor counts tests/test_gpu_bound_scan_l2.py compares the device's counters with: no hand-back, within the list, as recorded;
    and the oracle's neighbours are among the rows each stage passes on"""
    got = L.model_counts(name)
    assert got == L.RECORDED[name], got
    rows, qs = L.corpus(name)
    for qi in range(L.NQ):
        er, _ = O.exact_search(L2, rows, qs[qi], 64)
        for s in L.stages(name, qi):
            for k in L.KS:
                assert B.decide(s, k)["passed"][er[:k]].all(), (name, qi, k)
