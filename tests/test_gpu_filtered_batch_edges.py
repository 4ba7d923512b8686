"""Filtered batches of 9 or more queries (qv_index_set_filtered_batch) on the inputs the rest of the suite reserves for the other paths: NaN,
infinite, overflowing, guard-crossing, zero and denormal rows and queries (tests/_extremes.py), rows whose float32 distance depends on the
order of summation (tests/_order.py), and sets that are shorter than the corpus, hold one lane of every word, one tile, or change between
two batches.  tests/_filtered_edges.py builds the inputs; tests/test_filtered_batch_edges_cpu.py proves what they promise without a device.

The contract is the exact filtered scan's answer — rows, float32 bits (NaN where the oracle's value is NaN), counts, 0xFFFFFFFF / +inf
padding.  Every check is made two ways: against tests/_oracle.exact_search(metric, rows, q, k, alive=live & set_q), and for EVERY query of
the batch against the same call under "never".  Everything runs under "always" and asserts that the `queries` counter moved by nq: no test
passes because the piece was declined."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import quiver_amd
from quiver_amd import batched_filter_route
from tests import _extremes as X
from tests import _filtered_edges as E
from tests import _oracle as O
from tests import _order as OR
from tests.test_filtered_batch_edges_cpu import route_of
from tests.test_gpu_filtered_batch import Corpus, _is_oracle, _run, _same

pytestmark = pytest.mark.gpu

_POOL = ThreadPoolExecutor(max_workers=16)                              # ctypes drops the GIL: the oracle scales with threads
NAMES = {OR.COSINE: "cosine", OR.L2: "l2", OR.L2SQ: "l2sq", OR.DOT: "dot"}


def _columns(idx, spec):
    cols = {}
    for name, (typ, values) in spec.items():
        cols[name] = idx.column(typ)
        cols[name].set(0, values, None)
    return cols


def _run_floor(idx, floor, call):
    """(results, what the counters moved by) under "always" with this sparse floor (None: the default)"""
    idx.set_filtered_batch("always", floor)
    s0 = idx.filtered_batch_stats()
    out = call()
    s1 = idx.filtered_batch_stats()
    return out, {key: s1[key] - s0[key] for key in s0}


def _same_x(a, b, where, only=None):
    """_same, with NaN where the other side has NaN; only: the queries compared"""
    (r, d, c), (rr, rd, rc) = a, b
    sel = slice(None) if only is None else only
    assert np.array_equal(c[sel], rc[sel]), (where, np.flatnonzero(c != rc)[:8])
    assert np.array_equal(r[sel], rr[sel]), (where, np.flatnonzero((r != rr).any(axis=1))[:8])
    assert X.same(d[sel], rd[sel]), (where, [q for q in range(d.shape[0]) if not X.same(d[q], rd[q])][:8])


def _is_oracle_x(got, q, want, k, where):
    """_is_oracle, with NaN where the oracle's value is NaN"""
    r, d, c = got
    ro, do = want
    w = min(k, ro.size)
    assert int(c[q]) == w, (where, q, int(c[q]), w)
    assert r[q, :w].tolist() == ro[:w].tolist(), (where, q, r[q, :w].tolist(), ro[:w].tolist())
    assert X.same(d[q, :w], do[:w]), (where, q)
    assert (r[q, w:] == 0xFFFFFFFF).all() and np.isposinf(d[q, w:]).all(), (where, q)


# ---- 2. extreme rows and queries: 40 003 rows, batches of 40 and 256 with every extreme query in each, seven kinds of set ----
EXTREME_SHAPES = [(768, {}), (768, {"bf16_rows": True}), (128, {}), (96, {})]     # 96: a dimension the eight-wave loop does not divide


@pytest.mark.parametrize("regime", ["few", "many"])
@pytest.mark.parametrize("metric", ["cosine", "dot", "l2", "l2sq"])
@pytest.mark.parametrize("dim,kw", EXTREME_SHAPES, ids=["%d%s" % (d, "-bf16_rows" if kw else "") for d, kw in EXTREME_SHAPES])
def test_extreme_rows_and_queries_under_sets(dim, kw, metric, regime):
    """Per position of the batch one of the kinds of tests/_filtered_edges.KINDS, as a RowSet (search_rowsets) and as a conjunction
    (search_where), under the default sparse floor and under none.  The counters' cap is what keeps a hand-back from hiding a failure:
    hand_backs + sparse <= (queries that are extreme or whose set holds an extreme row) + (the other, clean queries) // 8.  The clean
    queries are ordinary ones under kind (d), a set without a single extreme row: with a fifth of the corpus NaN outside their sets they
    must be answered by the batched kernels, which holds only if the flush drops rows outside the set BEFORE it counts them.  Then the
    other filter kernels at k = 10, so that all eight flush variants meet these rows, and the same batch with every extreme query
    replaced by an ordinary one: the ordinary queries' answers do not move."""
    case = E.ExtremeCase(metric, dim, regime)
    c = Corpus(metric, dim, E.N, 1, rows=case.rows, **kw)                # (the index, with tombstones every 89th row)
    idx = c.idx
    assert np.array_equal(c.live, case.live)
    cols = _columns(idx, case.columns)
    shared = {}
    sets = []
    for p in range(E.NQ_MAX):
        kind = case.kind[p]
        if kind == "c":
            sets.append(None)
        elif kind in "aefg":                                            # (one set per kind: these do not depend on the position)
            sets.append(shared.setdefault(kind, idx.rowset(case.mask[p])))
        else:
            sets.append(idx.rowset(case.mask[p]))
    filters = [None if w is None else [(cols[name], op, lit) for name, op, lit in w] for w in case.where]
    probes = case.probes(E.NQ_MAX)
    want = dict(zip(probes, _POOL.map(lambda p: O.exact_search(case.mid, case.rows, case.qs[p], 64, alive=case.alive(p)), probes)))
    ordinary = np.flatnonzero(~case.is_ext)
    plane = bool(kw.get("bf16_rows"))
    ran = set()
    for nq in (40, 256):
        clean = np.flatnonzero(~case.touches[:nq])
        assert clean.size >= nq // 4
        cap = case.cap(nq)
        ord_q = ordinary[ordinary < nq]
        for filt, ks in (("auto", (1, 10, 64)), ("bf16x3", (10,)), ("fp32", (10,))):
            idx.set_filter(filt)
            assert batched_filter_route(metric, dim, E.N, nq, 10, filt, plane)[1] == route_of(filt, dim, plane, nq)
            ran.add(route_of(filt, dim, plane, nq))
            for k in ks:
                for form, call, calm in (("sets", lambda: idx.search_rowsets(case.qs[:nq], k, sets[:nq]), lambda: idx.search_rowsets(case.calm[:nq], k, sets[:nq])),
                                         ("where", lambda: idx.search_where(case.qs[:nq], k, filters[:nq]), lambda: idx.search_where(case.calm[:nq], k, filters[:nq]))):
                    never, moved = _run(idx, "never", call)
                    assert moved["queries"] == 0 and moved["batches"] == 0
                    for floor in ((None, 0) if filt == "auto" else (0,)):
                        where = (metric, dim, tuple(kw), regime, filt, form, nq, k, floor)
                        got, moved = _run_floor(idx, floor, call)
                        print("EDGES2 %s hand_backs %d sparse %d cap %d" % (where, moved["hand_backs"], moved["sparse"], cap))
                        assert moved["queries"] == nq and moved["batches"] == 1, (where, moved)
                        assert moved["hand_backs"] + moved["sparse"] <= cap, (where, moved, cap)
                        if floor == 0:
                            assert moved["sparse"] == 0, (where, moved)
                        _same_x(got, never, where)
                        for p in probes:
                            if p < nq:
                                ro, do = want[p]
                                _is_oracle_x(got, p, (ro[:k], do[:k]), k, where)
                    # isolation: the extreme queries replaced by ordinary ones, the others' answers stay (floor 0: the run just made)
                    alone, moved = _run_floor(idx, 0, calm)
                    assert moved["queries"] == nq, (where, moved)
                    _same_x(got, alone, ("isolation",) + where, only=ord_q)
                    _same((got[0][clean], got[1][clean], got[2][clean]), (alone[0][clean], alone[1][clean], alone[2][clean]), ("isolation, clean",) + where)
    assert ran == {route_of(f, dim, plane, nq) for f in ("auto", "bf16x3", "fp32") for nq in (40, 256)}


# ---- 3. order-sensitive planted rows: the exact re-score of survivors gives the single-chain float32 bits, under sets too ----
ORDER_OPTIONS = [({}, None), ({}, "fp32"), ({"bf16_rows": True}, None)]


def _order_index(case, kw, filt):
    idx = quiver_amd.DeviceIndex(case.dim, NAMES[case.metric], **kw)
    idx.add(case.rows)
    if filt:
        idx.set_filter(filt)
    cols = _columns(idx, case.columns)
    sets, filters = [], []
    for p in range(case.nq):
        if case.mask[p] is None:
            sets.append(None); filters.append(None)
            continue
        member = [(cols[case.column[p]], "eq", 1)]
        sets.append(idx.rowset_where(member) if case.kind[p] == 3 else idx.rowset(case.mask[p]))     # kind 3: the set a where-filter makes
        filters.append(member)
    return idx, sets, filters


def _order_check(case, idx, sets, filters, ks, what):
    want = list(_POOL.map(lambda p: O.exact_search(case.metric, case.rows, case.qs[p], max(ks), alive=case.alive(p)), range(case.nq)))
    for k in ks:
        for form, call in (("sets", lambda: idx.search_rowsets(case.qs, k, sets)), ("where", lambda: idx.search_where(case.qs, k, filters))):
            where = what + (form, k)
            never, _ = _run(idx, "never", call)
            got, moved = _run(idx, "always", call)
            assert moved["queries"] == case.nq and moved["batches"] == 1, (where, moved)
            _same(got, never, where)
            for p in range(case.nq):
                ro, do = want[p]
                _is_oracle(got, p, (ro[:k], do[:k]), k, where)
            # the tie rule across the set's boundary: the copy left out of the set is not in the answer, its twin is
            for p in range(case.nq):
                if case.kind[p] >= 2:
                    rows = set(got[0][p, :int(got[2][p])].tolist())
                    assert not rows & set(case.excluded[p].tolist()), (where, p)


@pytest.mark.parametrize("metric", [OR.COSINE, OR.DOT, OR.L2, OR.L2SQ], ids=["cosine", "dot", "l2", "l2sq"])
@pytest.mark.parametrize("kw,filt", ORDER_OPTIONS, ids=["default", "fp32", "bf16_rows"])
def test_order_sensitive_rows_under_sets(kw, filt, metric):
    """tests/_order._case(metric, 256, 12, seed, 40 000, dup=3), its twelve queries three times (tests/_filtered_edges.OrderCase says why):
    k_rescore_select must return the planted rows' single-chain bits whichever kernel filtered, for planted rows inside the set only"""
    case = E.OrderCase(metric, 256, 9300 + metric, 40_000)
    idx, sets, filters = _order_index(case, kw, filt)
    assert batched_filter_route(NAMES[metric], 256, case.n, case.nq, 10, filt or "auto", bool(kw))[1] == route_of(filt, 256, bool(kw), 36)
    _order_check(case, idx, sets, filters, (10, 40), (NAMES[metric], tuple(kw), filt))


@pytest.mark.parametrize("metric,seed", [(OR.COSINE, 9400), (OR.L2, 9401)], ids=["cosine", "l2"])
def test_order_sensitive_rows_under_sets_and_a_guessed_bound(metric, seed):
    """140 000 fillers, k = 32: the bound is a guess and the large-k narrowing precedes the exact distances"""
    case = E.OrderCase(metric, 128, seed, 140_000)
    idx, sets, filters = _order_index(case, {}, None)
    plan = idx.batched_sample_plan(case.nq, 32)
    assert plan["rank"] > 32 * plan["rows"] // case.n, plan
    _order_check(case, idx, sets, filters, (32,), (NAMES[metric], "guess"))


# ---- 4. ragged sets: made before the index grew, one lane of every word, one tile, changed between two batches ----
def test_ragged_sets_and_sets_that_change_between_batches():
    case = E.RaggedCase()
    k, nq, n = 10, case.nq, case.n
    idx = quiver_amd.DeviceIndex(case.dim, "cosine")
    idx.add(case.rows[:E.RAGGED_OLD])
    col = idx.column("f64")
    col.set(0, case.val, None)
    lane = idx.column("u32")
    lane.set(0, np.arange(E.RAGGED_OLD, dtype=np.uint32) % 64, None)
    sets = [None] * nq
    for q in range(nq):
        if case.before[q]:
            sets[q] = idx.rowset(case.mask[q][:E.RAGGED_OLD])            # words for the old corpus: 516 of the 626 to come
    idx.add(case.rows[E.RAGGED_OLD:])
    assert idx.rows() == n
    filters, wmasks = [None] * nq, [np.ones(n, bool) for _ in range(nq)]
    for q in range(nq):
        kind = case.kind[q]
        if kind == "new_last_tile":
            sets[q] = idx.rowset(case.mask[q])
        if case.where[q]:
            lo, hi = case.where[q]
            filters[q] = [(col, "ge", lo), (col, "lt", hi)]
            sets[q] = idx.rowset_where(filters[q])                      # (made after the growth: the column does not reach the new rows)
        elif kind in ("bit0", "bit63", "empty"):
            filters[q] = [(lane, "eq", {"bit0": 0, "bit63": 63, "empty": 64}[kind])]
        if filters[q] is not None:
            wmasks[q] = case.mask[q]
    idx.remove(E.dead_rows(n))                                          # tombstones AFTER the sets exist
    plan = idx.batched_sample_plan(nq, k)
    assert (plan["rows"], plan["group_step"], plan["rank"]) == (32_768, 1, k), plan
    assert batched_filter_route("cosine", case.dim, n, nq, k)[1] == route_of("auto", case.dim, False, nq)

    def check(masks, what):
        want = list(_POOL.map(lambda q: O.exact_search(0, case.rows, case.qs[q], k, alive=(case.live & masks[q]).astype(np.uint8)), range(nq)))
        call = lambda: idx.search_rowsets(case.qs, k, sets)               # noqa: E731
        never, _ = _run(idx, "never", call)
        for floor in (0, None):
            got, moved = _run_floor(idx, floor, call)
            assert moved["queries"] == nq and moved["batches"] == 1, (what, floor, moved)
            # the device's count of every set on the sample, through the only counter that shows it
            below = E.predicted_sparse(plan, n, case.live, masks) if floor is None else 0
            assert moved["sparse"] == below, (what, floor, moved, below)
            assert moved["hand_backs"] <= nq // 8, (what, floor, moved)
            _same(got, never, (what, floor))
            for q in range(nq):
                _is_oracle(got, q, want[q], k, (what, floor, case.kind[q]))
        return got

    first = check(case.mask, "as made")
    assert E.predicted_sparse(plan, n, case.live, case.mask) == 15       # the two last-tile kinds and the empty one, five times each
    # ... and through where-filters, evaluated inside the call over the grown corpus
    wwant = list(_POOL.map(lambda q: O.exact_search(0, case.rows, case.qs[q], k, alive=(case.live & wmasks[q]).astype(np.uint8)), range(nq)))
    wcall = lambda: idx.search_where(case.qs, k, filters)                 # noqa: E731
    wnever, _ = _run(idx, "never", wcall)
    for floor in (0, None):
        got, moved = _run_floor(idx, floor, wcall)
        assert moved["queries"] == nq and moved["sparse"] == (E.predicted_sparse(plan, n, case.live, wmasks) if floor is None else 0), (floor, moved)
        _same(got, wnever, ("where", floor))
        for q in range(nq):
            _is_oracle(got, q, wwant[q], k, ("where", floor, case.kind[q]))
    # two sets change: 200 rows in — some of them rows their words never covered — and 200 out.  The answers follow: the per-call set table
    # and the counts are not kept from the batch before
    for q, (add, drop) in case.changed.items():
        sets[q].set_rows(add, True)
        sets[q].set_rows(drop, False)
    second = check(case.masks_after(), "after set_rows")
    for q in case.changed:
        assert not np.array_equal(first[0][q], second[0][q]), q           # (the change is visible in the answers it must move)
