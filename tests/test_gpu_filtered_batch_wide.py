"""Filtered batches of 9+ queries at 65 to 1024 results each on the batched path (qv_index_set_filtered_batch_wide).  The contract is the exact
filtered scan's answer over live & set_q — rows, float32 bits, order, counts, padding: tests/_oracle.exact_search for a few queries of every batch,
the same call under "never" for all — and the counters of qv_index_filtered_batch_stats, which move only under "always"."""
import numpy as np
import pytest

import quiver_amd
from tests import _oracle as O

pytestmark = pytest.mark.gpu


def _smallest_rows(metric, dim, nq, k):                                   # (in steps of 31 tiles, from a partial one) what the dispatch's rule takes
    return next(n for n in range(32_768 + 35, 400_000, 1_984) if quiver_amd.batched_applies_filtered_wide(metric, dim, n, nq, k, mode="always"))


def _check(idx, metric, rows, qs, k, sets, masks, probe, want=None, call=None):
    call = call or (lambda: idx.search_rowsets(qs, k, sets))
    live = np.ones(len(rows), bool); live[5::89] = False
    out = {}
    for mode in ("never", "always"):
        idx.set_filtered_batch_wide(mode)
        s0 = idx.filtered_batch_stats()
        out[mode] = call()
        s1 = idx.filtered_batch_stats()
        moved = {key: s1[key] - s0[key] for key in s0}
        if mode == "never":
            assert not any(moved.values()), moved
    (r, d, c), (rr, rd, rc) = out["always"], out["never"]
    assert np.array_equal(c, rc) and np.array_equal(r, rr) and np.array_equal(d.view(np.uint32), rd.view(np.uint32))
    for q in probe:
        ro, do = O.exact_search(quiver_amd.metric_id(metric), rows, qs[q], k, alive=(live & masks[q]).astype(np.uint8))
        w = min(k, ro.size)
        assert int(c[q]) == w and r[q, :w].tolist() == ro[:w].tolist() and d[q, :w].tobytes() == do[:w].tobytes(), q
        assert (r[q, w:] == 0xFFFFFFFF).all() and np.isposinf(d[q, w:]).all(), q
    assert moved["queries"] == len(qs) and moved["batches"] == 1, moved
    for key, val in (want or {"hand_backs": 0, "sparse": 0}).items():
        assert moved[key] == val, (key, moved)
    return moved


def _index(metric, dim, n, nq, rows=None, **kw):
    """i.i.d. rows, every 89th from 5 dead; by q mod 4: a random half as a set of its own, no set, a conjunction of ~30 %, query 0's set once more"""
    rows = O.gen_rows(9100 + dim, 0, n, dim) if rows is None else rows
    idx = quiver_amd.DeviceIndex(dim, metric, **kw)
    idx.add(rows); idx.remove(np.arange(5, n, 89, dtype=np.uint32))
    rng = np.random.default_rng(n + nq)
    val = rng.random(n)
    col = idx.column("f64"); col.set(0, val, None)
    conj, below = [(col, "ge", 0.2), (col, "lt", 0.5)], [(col, "lt", 0.5)]
    sets, masks, filters, wmasks = [], [], [], []
    for q in range(nq):
        half = masks[0] if q % 4 == 3 else rng.random(n) < 0.5
        m, f, wm = ((half, below, val < 0.5), (np.ones(n, bool), None, np.ones(n, bool)), ((val >= 0.2) & (val < 0.5), conj, (val >= 0.2) & (val < 0.5)), (half, below, val < 0.5))[q % 4]
        sets.append(sets[0] if q % 4 == 3 else (None if q % 4 == 1 else (idx.rowset_where(conj) if q % 4 == 2 else idx.rowset(m))))
        masks.append(m); filters.append(f); wmasks.append(wm)
    return idx, rows, O.gen_rows(9200 + dim, 0, nq, dim), sets, masks, filters, wmasks


# k: the first wide one; 128 | 129; both sides of where k_sample_select gives way to the histogram AT THIS SHAPE (sample_select_applies: k chunks fit 24 576 keys); a large one
@pytest.mark.parametrize("nq", [9, 70])
@pytest.mark.parametrize("which", ["65", "128", "129", "select_last", "hist_first", "1000"])
def test_k_edges_and_mixed_filter_kinds_no_hand_back(which, nq):
    n = _smallest_rows("cosine", 64, nq, 65)
    idx, rows, qs, sets, masks, filters, wmasks = _index("cosine", 64, n, nq)
    fits = lambda k: k * (((idx.batched_sample_plan(nq, k)["rows"] + 1023) // 1024 + 3) // 4 * 4) <= 24_576   # noqa: E731  (the sample grows with k)
    limit = max(k for k in range(65, 1025) if fits(k))
    assert 129 < limit < 1000 and n < 131_072, (n, limit)                 # (fewer than 131 072 rows: no bound is a guess down here)
    k = {"select_last": limit, "hist_first": limit + 1}.get(which) or int(which)
    _check(idx, "cosine", rows, qs, k, sets, masks, (0, 1, 2, 3, nq - 1))
    if which in ("65", "1000"):                                           # the where form: real sets are made first and fed in
        _check(idx, "cosine", rows, qs, k, None, wmasks, (0, 1, 2), call=lambda: idx.search_where(qs, k, filters))


@pytest.mark.parametrize("metric,dim,filt,kw", [("cosine", 64, "bf16x3", {}), ("dot", 64, "fp32", {}), ("l2", 64, "bf16x1", {"bf16_rows": True}),
                                                ("l2sq", 64, "bf16x1", {"rowmajor": True}), ("cosine", 100, "bf16x1", {}), ("dot", 64, "bf16x1", {"scan_plane": False})])
def test_metrics_filter_kernels_and_row_layouts(metric, dim, filt, kw):
    nq, k = 70, 100
    idx, rows, qs, sets, masks, _, _ = _index(metric, dim, _smallest_rows(metric, dim, nq, k), nq, **kw)
    idx.set_filter(filt)
    _check(idx, metric, rows, qs, k, sets, masks, (0, 1, 2, 69))


def test_sparse_set_a_set_below_k_and_the_default_mode():
    nq, k = 11, 65                                                        # (nine queries that the host does not know to be sparse, and the two that it does)
    n = _smallest_rows("cosine", 64, nq, k)
    idx, rows, qs, sets, masks, _, _ = _index("cosine", 64, n, nq)
    rng = np.random.default_rng(3)
    thin = rng.random(n) < 0.005                                          # below the default floor of a hundredth of the rows
    few = np.zeros(n, bool); few[rng.choice(n, 40, replace=False)] = True; few[5:5 + 89 * 10:89] = True   # 40 rows and ten dead ones: fewer live rows than k
    sets[2], masks[2], sets[4], masks[4] = idx.rowset(thin), thin, idx.rowset(few), few
    _check(idx, "cosine", rows, qs, k, sets, masks, (2, 4, 0, 3), {"hand_backs": 0, "sparse": 2})
    idx.set_filtered_batch("auto", 0)                                      # the floor is set_filtered_batch's: at zero both are answered in place
    _check(idx, "cosine", rows, qs, k, sets, masks, (2, 4, 0, 3), {"hand_backs": 0, "sparse": 0})
    idx.set_filtered_batch_wide("auto")                                    # the default mode takes nothing
    s0 = idx.filtered_batch_stats(); idx.search_rowsets(qs, k, sets)
    assert idx.filtered_batch_stats() == s0


def test_overflowing_list_is_handed_back():
    nq, k = 9, 65
    n = _smallest_rows("cosine", 64, nq, k)
    rows = O.gen_rows(9164, 0, n, 64)
    qs = O.gen_rows(9264, 0, nq, 64)
    rows[20_000:25_000] = qs[3] + 1e-3 * np.random.default_rng(1).standard_normal((5000, 64)).astype(np.float32)   # more in-set near-duplicates than the 4096 slots of k = 65
    idx, rows, qs, sets, masks, _, _ = _index("cosine", 64, n, nq, rows=rows)
    sets[3], masks[3] = None, np.ones(n, bool)
    _check(idx, "cosine", rows, qs, k, sets, masks, (3, 0, 4), {"hand_backs": 1, "sparse": 0})


N_GUESS = 131_072 + 35                                                    # the smallest corpus whose bound is a guess (4 x 32 768 rows), and a partial tile


@pytest.mark.parametrize("nq", [9, 70])
@pytest.mark.parametrize("k", [65, 1000])
def test_guessed_bound_on_iid_rows_no_hand_back(k, nq):
    idx, rows, qs, sets, masks, _, _ = _index("cosine", 64, N_GUESS, nq)
    plan = idx.batched_sample_plan(nq, k)
    assert plan["rank"] < k and plan["rows"] <= N_GUESS // 4, plan        # a guess: a rank below k in a quarter of the rows
    _check(idx, "cosine", rows, qs, k, sets, masks, (0, 1, 2, 3, nq - 1))


def test_guessed_bound_takes_its_rank_from_the_querys_own_sample():
    """k = 65, a sample of every fourth 128-row group, the sparse floor off.  Queries 0 - 59: a set each that holds EVERY sample row and a third of
    the others (n_in / live = 1/2, the corpus has S / N = 1/4): the whole sample's rank, 35, would leave ~70 in-set rows under the bound and fail three
    checks in ten; the query's own, 58, leaves ~116.  Query 60: 40 live rows and ten dead ones — no guess, answered in place.  Query 61: 45 rows next to
    the query inside ONE sample group: its rank lands among them, fewer than k rows lie under the bound, it alone is handed back.  62 - 69: no set."""
    nq, k, n, rows, rng = 70, 65, N_GUESS, O.gen_rows(9164, 0, N_GUESS, 64), np.random.default_rng(8)
    near = np.arange(8 * 4 * 128, 8 * 4 * 128 + 45)                        # inside sample group 8
    rows[near] = O.gen_rows(9264, 0, nq, 64)[61] + 1e-3 * rng.standard_normal((45, 64)).astype(np.float32)
    idx, rows, qs, sets, masks, _, _ = _index("cosine", 64, n, nq, rows=rows)
    assert idx.batched_sample_plan(nq, k) == {"rows": 32_768, "group_step": 4, "rank": 35}
    for q in range(nq):
        m = ((np.arange(n) // 128) % 4 == 0) | (rng.random(n) < 1 / 3) if q < 60 else (rng.random(n) < 0.5 if q == 61 else np.ones(n, bool))
        if q in (60, 61):                                                  # 40 live rows and ten dead ones | the planted rows join the half
            m[:] = m & (q == 61); m[near if q == 61 else np.r_[rng.choice(n, 40, replace=False), 5:5 + 89 * 10:89]] = True
        sets[q], masks[q] = (idx.rowset(m) if q < 62 else None), m
    idx.set_filtered_batch("auto", 0)
    _check(idx, "cosine", rows, qs, k, sets, masks, (0, 59, 60, 61, 69), {"hand_backs": 1, "sparse": 0})
