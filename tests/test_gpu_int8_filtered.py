"""Filtered batches on the int8 kernel's sets form (set_int8_filtered("always"); k_int8_tiles, k_int8_filter<., ., ., true>) against the CPU oracle's exact
search over live & set_q: rows, float32 bits, counts and padding equal; int8_filtered_stats() moves by the batch, its tile counts are numpy's."""
import functools

import numpy as np
import pytest

import quiver_amd
from tests import _oracle as O

pytestmark = pytest.mark.gpu

N = 65_536 + 37            # a ragged last tile; a million query-rows at 16 queries
N9 = 111_104 + 37          # ... at 9 (the batched path takes nothing below a million)
SHORT = 40_000             # the rows the index held when the "short" set was made

class Fix:
    def __init__(self, metric, dim, n=N, rows=None, **kw):
        self.mid, self.n = quiver_amd.metric_id(metric), n
        self.rows = O.gen_rows(9100 + dim, 0, n, dim) if rows is None else rows
        self.qs = O.gen_rows(9200 + dim, 0, 70, dim)
        self.idx = idx = quiver_amd.DeviceIndex(dim, metric, **kw)
        self.rng = rng = np.random.default_rng(dim + n)
        idx.add(self.rows[:SHORT])
        self.short_mask = np.zeros(n, bool); self.short_mask[:SHORT] = rng.random(SHORT) < 0.4
        self.short = idx.rowset(self.short_mask[:SHORT])                 # made before the index grew: words past its end read as zero
        idx.add(self.rows[SHORT:])
        self.live = np.ones(n, bool)
        self.remove(np.arange(5, n, 89, dtype=np.uint32))

    def remove(self, dead):
        self.idx.remove(dead); self.live[dead] = False

    def thirds(self, nq):
        masks = [self.rng.random(self.n) < 1 / 3 for _ in range(nq)]
        return masks, [self.idx.rowset(m) for m in masks]

    def run(self, nq, k, masks, filters, mode="always", probe=None, moves=True, search="search_rowsets"):
        """-> (results, the tile counters' movement, the filtered batch's); every probed query against the oracle"""
        idx = self.idx
        idx.set_filter("int8"); idx.set_filtered_batch("always", sparse_ppm=0); idx.set_filtered_batch_wide("always" if k > 64 else "auto"); idx.set_int8_filtered(mode)
        try:
            s0, f0, b0 = idx.int8_filtered_stats(), idx.int8_filter_stats(), idx.filtered_batch_stats()
            r, d, c = getattr(idx, search)(self.qs[:nq], k, filters)
            s1, f1, b1 = idx.int8_filtered_stats(), idx.int8_filter_stats(), idx.filtered_batch_stats()
        finally:
            idx.set_int8_filtered("auto"); idx.set_filtered_batch("auto"); idx.set_filtered_batch_wide("auto"); idx.set_filter("auto")
        assert b1["batches"] == b0["batches"] + 1                       # a filtered batch either way
        assert (s1[0] - s0[0], s1[1] - s0[1], f1[0] - f0[0]) == ((1, nq, 1) if moves else (0, 0, 0))   # (int8_filter_stats counts these batches too)
        for q in range(nq) if probe is None else probe:
            ro, do = O.exact_search(self.mid, self.rows, self.qs[q], k, alive=(self.live & masks[q]).astype(np.uint8))
            w = ro.size; assert int(c[q]) == w and r[q, :w].tolist() == ro.tolist() and d[q, :w].tobytes() == do.tobytes(), q
            assert (r[q, w:] == 0xFFFFFFFF).all() and np.isposinf(d[q, w:]).all(), q
        return r, (s1[2] - s0[2], s1[3] - s0[3]), {key: b1[key] - b0[key] for key in b0}

_fix = functools.lru_cache(maxsize=1)(Fix)

@pytest.mark.parametrize("metric,dim,nq,k,n", [
    ("cosine", 768, 16, 10, N),        # 24 steps: the ring form without idle steps
    ("dot", 64, 9, 1, N9),             # the smallest shape: two steps
    ("cosine", 96, 16, 10, N),         # fewer steps than the ring is deep
    ("cosine", 1024, 70, 64, N),       # idle ring steps; a second block with six real queries
    ("cosine", 768, 16, 100, N),       # the wide funnel
])
def test_a_distinct_third_per_query_equals_the_oracle(metric, dim, nq, k, n):
    fx = _fix(metric, dim, n)
    masks, sets = fx.thirds(nq)
    fx.run(nq, k, masks, sets, probe=None if nq <= 16 else list(range(0, 64, 9)) + list(range(64, 70)))

def test_a_mix_of_sets_none_where_and_a_short_set():
    fx, nq, k = _fix("cosine", 768, N), 16, 10
    masks, sets = fx.thirds(nq)
    for q in range(0, nq, 4):
        masks[q], sets[q] = np.ones(fx.n, bool), None
        masks[q + 1], sets[q + 1] = fx.short_mask, fx.short
    fx.run(nq, k, masks, sets)
    val, col = fx.rng.random(fx.n), fx.idx.column("f64")
    col.set(0, val, None)
    filters = [None if q % 4 == 0 else [(col, "ge", 0.05 * q), (col, "lt", 0.05 * q + 0.2)] for q in range(nq)]
    wmasks = [np.ones(fx.n, bool) if q % 4 == 0 else (val >= 0.05 * q) & (val < 0.05 * q + 0.2) for q in range(nq)]
    fx.run(nq, k, wmasks, filters, search="search_where")

def test_rows_outside_a_set_never_reach_its_query():
    dim, nq, k, copies, zero, huge = 128, 16, 10, np.arange(20_000, 20_012), 30_001, 30_002
    rows, qs = O.gen_rows(9100 + dim, 0, N, dim).copy(), O.gen_rows(9200 + dim, 0, 70, dim)   # (Fix's own)
    rows[copies] = qs[0]                                                # nearer to query 0 than anything else
    # the plane declines both (kept whatever their scores, where a set holds them); the huge one is query 2's nearest row by far
    rows[zero] = 0.0; rows[huge] = qs[2] * np.float32(1e20)
    fx = Fix("cosine", dim, rows=rows)
    masks, sets = fx.thirds(nq)
    planted = np.concatenate([copies, [zero, huge]]); masks[0][planted] = False; masks[1][planted] = True
    masks[2][planted] = False; masks[2][zero] = True; masks[3][planted] = False; masks[3][huge] = True   # (queries 2 and 3 share a 16-score block)
    sets[:4] = [fx.idx.rowset(m) for m in masks[:4]]
    fx.qs[1] = fx.qs[0]                                                 # query 1, same block, sees the copies
    got = fx.run(nq, k, masks, sets)[0]
    assert not np.isin(got[0], planted).any() and huge not in got[2] and zero not in got[3]
    assert np.isin(copies[:k], got[1]).all()

def _visits(fx, nq, masks):
    n_tiles, skipped = (fx.n + 63) // 64, 0
    pad = np.zeros(n_tiles * 64, bool)
    for b in range(0, nq, 64):
        pad[:fx.n] = fx.live & np.logical_or.reduce(masks[b: b + 64])
        skipped += n_tiles - int(pad.reshape(n_tiles, 64).any(axis=1).sum())
    return skipped, (nq + 63) // 64 * n_tiles

def test_skipped_tiles_are_counted_exactly():
    fx = Fix("cosine", 128)
    stripes = np.zeros(fx.n, bool)
    for t in range(7, (fx.n + 63) // 64, 20):                           # (a) one tile in 20, named by all 16 queries ...
        stripes[64 * t: 64 * t + 64] = True
    fx.remove(np.arange(64 * 47, 64 * 48, dtype=np.uint32))             # ... one of them wholly dead
    visits = fx.run(16, 10, [stripes] * 16, [fx.idx.rowset(stripes)] * 16)[1]
    assert visits == _visits(fx, 16, [stripes] * 16) and visits[0] > 0
    lo = np.zeros(fx.n, bool); lo[: fx.n // 2] = True                   # (b) two blocks, disjoint halves of the corpus
    masks = [lo] * 64 + [~lo] * 6
    visits = fx.run(70, 10, masks, [fx.idx.rowset(lo)] * 64 + [fx.idx.rowset(~lo)] * 6, probe=(0, 63, 64, 69))[1]
    assert visits == _visits(fx, 70, masks)

def test_an_overflowing_query_comes_back_through_the_redo():
    dim, nq, k, same = 128, 16, 64, np.arange(10_000, 16_000)
    rows = O.gen_rows(9100 + dim, 0, N, dim).copy()
    rows[same] = rows[10_000]                                           # 6000 rows, one vector: more ties than a list has slots
    fx = Fix("cosine", dim, rows=rows)
    masks, sets = fx.thirds(nq)
    masks[5] = np.isin(np.arange(fx.n), same); sets[5] = fx.idx.rowset(masks[5])
    assert 1 <= fx.run(nq, k, masks, sets)[2]["hand_backs"] < nq

@pytest.mark.parametrize("metric,kw,mode", [("cosine", {}, "auto"), ("cosine", {}, "never"), ("cosine", {"scan_plane": False}, "always"), ("euclidean", {}, "always")])
def test_the_sets_form_stays_out(metric, kw, mode):
    fx = Fix(metric, 128, **kw)
    masks, sets = fx.thirds(16)
    fx.run(16, 10, masks, sets, mode=mode, moves=False)
