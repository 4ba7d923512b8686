"""Filtered batches of 9 or more queries on the batched path, a filter per query (qv_index_set_filtered_batch; quiver_amd/csrc/qv_batched_sets.hip,
the set test in qv_filter.h's cand_flush, the routing in qv_api.cpp's rowsets_direct).

The contract is the exact filtered scan's answer: rows, float32 bits, (distance, row) order, counts and padding.  Every comparison here is
against tests/_oracle.exact_search(metric, rows, q, k, alive=live & set_q) for about six queries of a batch, and against the same call under
"never" (the exact row-set passes) for all of them.  Everything runs under "always": the automatic mode takes no shape that was not measured.

Every test in this file needs the new setter and its counters: none passes without them."""
import threading

import numpy as np
import pytest

import quiver_amd
from quiver_amd import QvError
from quiver_amd.device_index import broadcast_filters, pack_where
from tests import _oracle as O
from tests.test_filtered_batch_edges_cpu import route_of

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
DEFAULT_PPM = 10_000
N_SMALL = 40_003                                                        # 626 tiles: a partial last one, an odd number of 128-row groups' worth
NQS = (40, 100, 256, 300)                                               # one block of 64; two; a whole workgroup of 256; 256 + a tail of 44
KS = (1, 10, 15)
KINDS = 6                                                               # the kinds of filter a batch cycles through, query by query


def _dead(n):
    return np.arange(5, n, 89, dtype=np.uint32)


class Corpus:
    """rows, tombstones every 89th row, an F64 column of uniform values, and per query a filter in both forms: a RowSet (or None) with its
    mask for search_rowsets, and a conjunction with ITS mask for search_where.  Kinds, by query number mod 6: every row as a set; half;
    a quarter; no filter at all; half plus 40 tombstoned rows; the rows whose column value lies in [0.2, 0.5) — about 30 %."""

    def __init__(self, metric, dim, n, nq, rows=None, **kw):
        self.metric, self.mid, self.dim, self.n = metric, quiver_amd.metric_id(metric), dim, n
        self.rows = O.gen_rows(7300 + dim, 0, n, dim) if rows is None else rows
        self.idx = idx = quiver_amd.DeviceIndex(dim, metric, **kw)
        idx.add(self.rows)
        dead = _dead(n)
        idx.remove(dead)
        self.live = np.ones(n, bool); self.live[dead] = False
        rng = np.random.default_rng(dim * 1000 + n % 997)
        self.qs = O.gen_rows(7400 + dim, 0, nq, dim)
        self.val = rng.random(n)
        self.col = idx.column("f64")
        self.col.set(0, self.val, None)
        self.sets, self.masks, self.filters, self.wmasks = [], [], [], []
        for q in range(nq):
            kind = q % KINDS
            u = rng.random(n)
            if kind == 3:
                self.sets.append(None); self.masks.append(np.ones(n, bool))
                self.filters.append(None); self.wmasks.append(np.ones(n, bool))
                continue
            if kind == 5:
                m = (self.val >= 0.2) & (self.val < 0.5)
                self.sets.append(idx.rowset_where([(self.col, "ge", 0.2), (self.col, "lt", 0.5)])); self.masks.append(m)
                self.filters.append([(self.col, "ge", 0.2), (self.col, "lt", 0.5)]); self.wmasks.append(m)
                continue
            dens = (1.0, 0.5, 0.25, None, 0.5)[kind]
            m = u < dens
            if kind == 4:
                m[dead[:40]] = True                                     # selecting a tombstoned row selects nothing
            self.sets.append(idx.rowset(m)); self.masks.append(m)
            # the same share as a predicate of this query's own: a window of the column as wide as the density, starting where q says
            lo = 0.0 if dens == 1.0 else (0.07 * q) % (1.0 - dens)
            self.filters.append([(self.col, "ge", lo), (self.col, "lt", lo + dens + (1.0 if dens == 1.0 else 0.0))])
            self.wmasks.append((self.val >= lo) & (self.val < lo + dens + (1.0 if dens == 1.0 else 0.0)))

    def oracle(self, q, k, mask):
        return O.exact_search(self.mid, self.rows, self.qs[q], k, alive=(self.live & mask).astype(np.uint8))


def _same(a, b, where):
    (r, d, c), (rr, rd, rc) = a, b
    assert np.array_equal(c, rc), (where, np.flatnonzero(c != rc)[:8])
    assert np.array_equal(r, rr), (where, np.flatnonzero((r != rr).any(axis=1))[:8])
    assert np.array_equal(d.view(np.uint32), rd.view(np.uint32)), (where, np.flatnonzero((d.view(np.uint32) != rd.view(np.uint32)).any(axis=1))[:8])


def _is_oracle(got, q, want, k, where):
    r, d, c = got
    ro, do = want
    w = min(k, ro.size)
    assert int(c[q]) == w, (where, q, int(c[q]), w)
    assert r[q, :w].tolist() == ro[:w].tolist(), (where, q)
    assert d[q, :w].tobytes() == do[:w].tobytes(), (where, q)
    assert (r[q, w:] == 0xFFFFFFFF).all() and np.isposinf(d[q, w:]).all(), (where, q)


def _run(idx, mode, call):
    """(results, what the counters moved by) of `call` under `mode`"""
    idx.set_filtered_batch(mode)
    s0 = idx.filtered_batch_stats()
    out = call()
    s1 = idx.filtered_batch_stats()
    return out, {key: s1[key] - s0[key] for key in s0}


# ---- 1. every route: 40 003 rows (by batched_sample_rows the sample is 32 768 of them under the one-term filter; the expected in-set
# candidates are about k N / S x 4.6, some 60 of 4 096 slots, so the unmodified bound alone stays far inside the cap) ----
ROUTES = [(768, {}), (768, {"scan_plane": False}), (768, {"bf16_rows": True}), (128, {}), (128, {"scan_plane": False}), (96, {}), (96, {"scan_plane": False})]


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])              # the filter kernels' three metrics (L2SQ shares L2's): every flush variant is launched
@pytest.mark.parametrize("dim,kw", ROUTES, ids=["%d-%s" % (d, "-".join(sorted(kw)) or "plane") for d, kw in ROUTES])
def test_every_route_equals_the_oracle_and_the_exact_passes(dim, kw, metric):
    c = Corpus(metric, dim, N_SMALL, max(NQS), **kw)
    idx = c.idx
    probe = [q for q in (0, 7, 14, 21, 28, 35)]                           # one query of every kind (q mod 6 = 0, 1, 2, 3, 4, 5), all inside the smallest batch
    want_sets = {q: c.oracle(q, max(KS), c.masks[q]) for q in probe}
    want_where = {q: c.oracle(q, max(KS), c.wmasks[q]) for q in probe}
    plane, codes = bool(kw.get("bf16_rows")), {}                           # the main filter kernel of every cell's pieces (qv_batched_filter_route)
    never = {}
    for nq in NQS:
        for k in KS:
            never[("sets", nq, k)], moved = _run(idx, "never", lambda: idx.search_rowsets(c.qs[:nq], k, c.sets[:nq]))
            assert moved["queries"] == 0 and moved["batches"] == 0
            never[("where", nq, k)], moved = _run(idx, "never", lambda: idx.search_where(c.qs[:nq], k, c.filters[:nq]))
            assert moved["queries"] == 0 and moved["batches"] == 0
    for filt in ("bf16x1", "bf16x3", "fp32"):
        idx.set_filter(filt)
        for nq in NQS:
            for k in KS:
                for form, call, want in (("sets", lambda: idx.search_rowsets(c.qs[:nq], k, c.sets[:nq]), want_sets),
                                         ("where", lambda: idx.search_where(c.qs[:nq], k, c.filters[:nq]), want_where)):
                    where = (metric, dim, tuple(kw), filt, form, nq, k)
                    for piece in ((256, 44) if nq == 300 else (nq,)):
                        codes[(filt, piece)] = quiver_amd.batched_filter_route(metric, dim, N_SMALL, piece, k, filt, plane)[1]
                    got, moved = _run(idx, "always", call)
                    assert moved["queries"] == nq, (where, moved)                      # every query took the path ...
                    assert moved["batches"] == (2 if nq == 300 else 1), (where, moved)   # ... 300 as 256 and a tail of 44
                    assert moved["hand_backs"] + moved["sparse"] <= nq // 8, (where, moved)
                    _same(got, never[(form, nq, k)], where)
                    for q in probe:
                        ro, do = want[q]
                        _is_oracle(got, q, (ro[:k], do[:k]), k, where)
    # which flush variants this parametrisation launched: the table tests/test_filtered_batch_edges_cpu.py states, whose union over ROUTES is all eight
    assert codes == {(filt, piece): route_of(filt, dim, plane, piece) for filt in ("bf16x1", "bf16x3", "fp32") for piece in (40, 100, 256, 44)}, codes


# ---- 2. the guessed bound: k >= 16 on 131 072 rows or more.  One set is confined to the first third of the rows: the rank k S / N assumes a set
# spread over the corpus, the check behind the filter (the k-th smallest upper bound among the candidates against the guess) may hand it back ----
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_guessed_bound_under_sets(metric):
    n, dim, nq = 140_003, 128, 40
    c = Corpus(metric, dim, n, nq)
    idx = c.idx
    third = np.arange(n) < n // 3
    c.sets[9] = idx.rowset(third); c.masks[9] = third
    c.filters[9] = [(c.col, "lt", 1.0 / 3)]; c.wmasks[9] = c.val < 1.0 / 3           # (a third by value for the where form: spread, as a predicate's rows are)
    probe = (0, 7, 14, 21, 28, 35, 9)
    for k in (16, 64):
        plan = idx.batched_sample_plan(nq, k)
        assert plan["rank"] > k * plan["rows"] // n, plan                 # a guess: the rank of the expected k-th row plus its margin, in a sample far below N / 2
        for form, call, masks in (("sets", lambda: idx.search_rowsets(c.qs, k, c.sets), c.masks), ("where", lambda: idx.search_where(c.qs, k, c.filters), c.wmasks)):
            where = (metric, form, k)
            ref, _ = _run(idx, "never", call)
            got, moved = _run(idx, "always", call)
            assert moved["queries"] == nq and moved["batches"] == 1, (where, moved)
            _same(got, ref, where)
            for q in probe:
                _is_oracle(got, q, c.oracle(q, k, masks[q]), k, where)


# ---- 3. sparse sets come back through the sparse flag, with the oracle's counts and padding ----
def _sample_positions(plan, n):
    """sample position -> corpus row, as qv_batched_sample_plan states it"""
    i = np.arange(plan["rows"])
    r = (i // 128) * plan["group_step"] * 128 + i % 128
    return r[r < n]


def test_sparse_sets_are_handed_back():
    nq, k = 40, 10
    c = Corpus("cosine", 768, N_SMALL, nq)
    idx = c.idx
    rng = np.random.default_rng(5)
    live_rows = np.flatnonzero(c.live)
    for j in range(12):
        m = rng.random(c.n) < 0.005
        c.sets[2 + 3 * j] = idx.rowset(m); c.masks[2 + 3 * j] = m
    empty = np.zeros(c.n, bool)
    few = np.zeros(c.n, bool); few[rng.choice(live_rows, 4, replace=False)] = True
    c.sets[1] = idx.rowset(empty); c.masks[1] = empty
    c.sets[3] = idx.rowset(few); c.masks[3] = few
    plan = idx.batched_sample_plan(nq, k)
    pos = _sample_positions(plan, c.n)
    below = sum(1 for q in range(nq) if int((c.live & c.masks[q])[pos].sum()) * 1_000_000 < DEFAULT_PPM * plan["rows"])
    assert below == 14                                                    # the twelve sets at half a percent, the empty one and the one with four rows
    call = lambda: idx.search_rowsets(c.qs, k, c.sets)                    # noqa: E731
    ref, _ = _run(idx, "never", call)
    got, moved = _run(idx, "always", call)
    assert moved["queries"] == nq and moved["sparse"] == below, moved
    _same(got, ref, "sparse")
    for q in (1, 3, 2, 5, 0, 7, 21):
        _is_oracle(got, q, c.oracle(q, k, c.masks[q]), k, "sparse")
    assert int(got[2][1]) == 0 and int(got[2][3]) == 4
    # a floor of zero: nothing is handed back as sparse, and the answers do not change
    idx.set_filtered_batch("always", 0)
    s0 = idx.filtered_batch_stats()
    got0 = call()
    s1 = idx.filtered_batch_stats()
    assert s1["sparse"] == s0["sparse"] and s1["queries"] - s0["queries"] == nq
    _same(got0, ref, "floor 0")


# ---- 4. the sample map ----
def test_sample_map_and_the_bound_over_the_set():
    n, dim, nq, k = 140_003, 128, 40, 10
    rows = O.gen_rows(7300 + dim, 0, n, dim).copy()
    qd = O.gen_rows(7400 + dim, 0, nq, dim)[22]
    # the plan depends on the shape alone: take it from a throw-away index of the same shape
    shape = quiver_amd.DeviceIndex(dim, "cosine"); shape.add_synthetic(1, 0, n)
    plan = shape.batched_sample_plan(nq, k)
    del shape
    assert plan["group_step"] > 1 and plan["rank"] == k, plan              # the sample is spread over the corpus; below k = 16 its bound is exact
    pos = _sample_positions(plan, n)
    in_sample = np.zeros(n, bool); in_sample[pos] = True
    outside = np.flatnonzero(~in_sample)
    rng = np.random.default_rng(11)
    dup = rng.choice(outside, 6000, replace=False)
    rows[dup] = qd                                                        # 6 000 duplicates of query 22, none of them a sample row
    c = Corpus("cosine", dim, n, nq, rows=rows)
    idx = c.idx
    assert idx.batched_sample_plan(nq, k) == plan
    live_out = outside[c.live[outside]]
    # (a) a set without a single sample row
    a = np.zeros(n, bool); a[rng.choice(live_out, 30_000, replace=False)] = True
    # (b) every sample row, plus the query's true nearest rows outside the sample
    d_all = O.all_distances(c.mid, rows, c.qs[4])
    near = live_out[np.argsort(d_all[live_out], kind="stable")[:25]]
    b = in_sample.copy(); b[near] = True
    # (c) fewer than k sample rows and 3 000 rows outside
    few_s = rng.choice(pos[c.live[pos]], 5, replace=False)
    cc = np.zeros(n, bool); cc[few_s] = True; cc[rng.choice(np.setdiff1d(live_out, dup), 3000, replace=False)] = True
    # (d) the same with the 6 000 duplicates of the query
    dd = cc.copy(); dd[dup] = True
    for q, m in ((10, a), (4, b), (16, cc), (22, dd)):
        c.sets[q] = idx.rowset(m); c.masks[q] = m
    call = lambda: idx.search_rowsets(c.qs, k, c.sets)                    # noqa: E731
    ref, _ = _run(idx, "never", call)
    got, moved = _run(idx, "always", call)                                # the default floor: (a), (c) and (d) hold next to no sample row
    assert moved["queries"] == nq and moved["sparse"] == 3, moved
    _same(got, ref, "map, default floor")
    idx.set_filtered_batch("always", 0)                                   # no floor: (a), (c) and (d) have no bound; (a) and (d) outgrow the 4 096 slots
    s0 = idx.filtered_batch_stats()
    got0 = call()
    s1 = idx.filtered_batch_stats()
    assert s1["sparse"] == s0["sparse"] and s1["hand_backs"] - s0["hand_backs"] == 2, (s0, s1)
    _same(got0, ref, "map, no floor")
    for q in (10, 4, 16, 22):
        want = c.oracle(q, k, c.masks[q])
        _is_oracle(got, q, want, k, "map")
        _is_oracle(got0, q, want, k, "map, no floor")
    assert got0[0][22].tolist() == sorted(dup[c.live[dup]].tolist())[:k]      # (d): the duplicates, in row order


# ---- 5. callers ----
def test_concurrent_callers_share_filtered_batches():
    n, dim, k, threads, calls = 300_003, 128, 10, 64, 6
    c = Corpus("cosine", dim, n, threads)
    idx = c.idx
    want = [c.oracle(t, k, c.masks[t] if t % 2 == 0 else c.wmasks[t]) for t in range(threads)]

    # Every caller packs its arguments and result arrays ONCE and then calls the C ABI itself, as search_rowsets / search_where do per call:
    # between two calls it holds the interpreter for microseconds.  Through the wrappers a call costs tens of microseconds of interpreter
    # time, one caller at a time, against a pass of about a hundred: the callers then reach the front a few per pass, and a group above 8
    # formed only behind a fresh index's first, slow pass — in 11 of 12 fresh indexes, and in none of 40 later storms (measured).  Called
    # directly, each of 16 storms on 4 indexes held 9 - 19 batched groups.
    def storm():
        out, errs = {}, []
        gate = threading.Barrier(threads)

        def caller(t):
            try:
                q = np.ascontiguousarray(c.qs[t:t + 1], dtype=np.float32)
                if t % 2 == 0:
                    fn, (arr, keep) = quiver_amd.lib().qv_index_search_rowsets, idx._set_handles(c.sets[t], 1)
                else:
                    fn, (arr, keep) = quiver_amd.lib().qv_index_search_where, pack_where(broadcast_filters([c.filters[t]], 1))
                res = [(np.full((1, k), 0xFFFFFFFF, np.uint32), np.full((1, k), np.inf, np.float32), np.zeros(1, np.uint32)) for _ in range(calls)]
                args = [(idx._h, q.ctypes.data, 1, k, arr, r.ctypes.data, d.ctypes.data, n_found.ctypes.data) for r, d, n_found in res]
                gate.wait()
                for it in range(calls):
                    rc = fn(*args[it])
                    assert rc == 0, (t, it, rc)
                    out[(t, it)] = res[it]
                del keep                                                  # (what arr points into, alive across the calls)
            except Exception as e:                                        # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=caller, args=(t,)) for t in range(threads)]
        [x.start() for x in th]; [x.join() for x in th]
        assert not errs, errs
        for (t, it), got in out.items():
            _is_oracle(got, 0, want[t], k, (t, it))

    idx.set_filtered_batch("always")
    f0, g0 = idx.filtered_batch_stats(), idx.rowset_coalesce_stats()
    storm()
    f1, g1 = idx.filtered_batch_stats(), idx.rowset_coalesce_stats()
    groups, gq = g1["groups"] - g0["groups"], g1["group_queries"] - g0["group_queries"]
    assert groups >= 1 and gq > groups, (g0, g1)                           # passes were shared ...
    batches, queries = f1["batches"] - f0["batches"], f1["queries"] - f0["queries"]
    assert batches >= 1 and queries >= 9 * batches, (f0, f1)                # ... and groups above 8 callers took the batched path, whole
    idx.set_filtered_batch("never")
    storm()
    assert idx.filtered_batch_stats() == f1


# ---- 6. the unfiltered batch is untouched ----
def test_unfiltered_batch_before_and_after_a_filtered_one():
    nq, k = 256, 10
    c = Corpus("cosine", 768, N_SMALL, nq)
    idx = c.idx
    by8 = [idx.search(c.qs[i:i + 8], k) for i in range(0, nq, 8)]
    eight = tuple(np.concatenate([x[j] for x in by8]) for j in range(3))
    before = idx.search(c.qs, k)
    _same(before, eight, "before")
    got, moved = _run(idx, "always", lambda: idx.search_rowsets(c.qs, k, c.sets))
    assert moved["queries"] == nq
    after = idx.search(c.qs, k)
    _same(after, eight, "after")
    assert idx.filtered_batch_stats()["queries"] == moved["queries"] + 0      # an unfiltered search is not counted


# ---- the setter's own checks ----
def test_setter_arguments():
    idx = quiver_amd.DeviceIndex(16, "cosine")
    for bad in (-1, 3):
        with pytest.raises(QvError) as e:
            idx.set_filtered_batch(bad)
        assert e.value.code == INVALID_ARG
    with pytest.raises(QvError) as e:
        idx.set_filtered_batch("always", 1_000_001)
    assert e.value.code == INVALID_ARG
    idx.set_filtered_batch("always", 1_000_000)
    idx.set_filtered_batch("auto")
    assert idx.filtered_batch_stats() == {"queries": 0, "hand_backs": 0, "sparse": 0, "batches": 0}
