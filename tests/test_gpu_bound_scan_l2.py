"""The bound scan on a Euclidean index created with QV_FLAG_L2_SCAN_PLANE (DeviceIndex(dim, "l2", l2_scan_plane=True)): the QV_L2 forms of
every kernel of quiver_amd/csrc/qv_bound_scan.hip — one query and shared passes of 2 - 8, bfloat16 first and 8-bit first, unfiltered, under a mask,
a row set per query and where-filters, from one call, from concurrent callers and from shards.  Every search runs with the bound scan
"always" on each plane mode (all four plane knobs set alike), then "never" on the same index: rows, counts and float32 bits must be the
same word for word, a few are compared with the CPU oracle, and the counters say which searches took the path, which were handed on or
back, and how many rows stage 1 passed on — the CPU model's figures (tests/_bound_l2.RECORDED, which tests/test_bound_scan_l2_cpu.py
derives).  The automatic modes take a flagged index from the measured row counts on (300 000 rows at the least), far above these corpora: "always" it is."""
import os

import numpy as np
import pytest

import quiver_amd
from quiver_amd import _lib
from tests import _bound as B
from tests import _bound_l2 as L
from tests import _callers
from tests import _extremes as X
from tests import _oracle as O

pytestmark = pytest.mark.gpu

PLANES = ("bf16", "8bit")


def l2_index(dim, **kw):
    return quiver_amd.DeviceIndex(dim, "l2", l2_scan_plane=True, **kw)


def set_planes(idx, plane):
    idx.set_bound_plane(plane); idx.set_bound_plane_filtered(plane); idx.set_bound_plane_mq(plane); idx.set_bound_plane_filtered_mq(plane)


def both(idx, call):
    """ONE call under "always" on each plane mode, then under "never": the same rows, counts and bits
    -> (the result, {plane: the counters' increments and last survivor counts})"""
    got, incs = [], {}
    for plane in PLANES:
        idx.set_bound_scan("always"); set_planes(idx, plane)
        a0, b0 = idx.bound_scan8_stats(), idx.bound_scan_stats()
        got.append(call())
        a1, b1 = idx.bound_scan8_stats(), idx.bound_scan_stats()
        incs[plane] = {"took": b1["searches"] - b0["searches"], "back": b1["hand_backs"] - b0["hand_backs"], "cand": b1["candidates"],
                       "took8": a1["searches"] - a0["searches"], "back8": a1["hand_backs"] - a0["hand_backs"], "cand8": a1["candidates"]}
    idx.set_bound_scan("never")
    a1, b1 = idx.bound_scan8_stats(), idx.bound_scan_stats()
    er, ed, ec = call()
    assert idx.bound_scan8_stats()["searches"] == a1["searches"] and idx.bound_scan_stats()["searches"] == b1["searches"]   # "never" is never
    for plane, (r, d, c) in zip(PLANES, got):
        assert np.array_equal(c, ec) and np.array_equal(r, er), (plane, r, er)
        assert X.same(d, ed), (plane, d, ed)
    return got[0], incs


def answered(incs, nq=1, back=0):
    """the bfloat16 mode: its stage alone took nq queries and handed `back` of them back; the 8-bit mode: the 8-bit stage took them, handed
    `back` on, and the bfloat16 stage behind it handed those back in turn"""
    a, b = incs["bf16"], incs["8bit"]
    return (a["took"] == nq and a["back"] == back and a["took8"] == 0 and
            b["took8"] == nq and b["back8"] == back and b["took"] == nq and b["back"] == back)


def agrees(rows, q, k, r, d, c, alive=None):
    er, ed = O.exact_search(L.L2, rows, q, k) if alive is None else O.exact_search(L.L2, rows, q, k, alive=np.asarray(alive).astype(np.uint8))
    w = len(er)
    return int(c) == w and r[:w].tolist() == er.tolist() and d[:w].tobytes() == ed.tobytes()


# ---- one query -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(L.CORPORA))
def test_rows_bits_and_survivor_counts_of_one_query(name):
    """12 000 x 128, 4 000 x 768 and 2 000 x 16 (a partly filled last tile in the first and the third), k = 1 / 10 / 64"""
    rows, qs = L.corpus(name)
    idx = l2_index(rows.shape[1]); idx.add(rows)
    assert idx.bound_scan_stats()["plane"] and idx.bound_scan8_stats()["plane"]
    for qi in range(L.NQ):
        for k in L.KS:
            (r, d, c), incs = both(idx, lambda: idx.search(qs[qi], k))
            assert answered(incs), (qi, k, incs)
            want16, want8 = L.RECORDED[name][("bf16", qi, k)], L.RECORDED[name][("8bit", qi, k)]
            assert incs["bf16"]["cand"] == want16 and incs["8bit"]["cand8"] == want8 and incs["8bit"]["cand"] == want8, (qi, k, incs, want16, want8)
            if qi == 0:
                assert agrees(rows, qs[qi], k, r[0], d[0], c[0]), (qi, k)
    idx.close()


def test_iid_unit_corpus_needs_no_hand_back():
    """50 000 x 768 synthetic unit rows, 4 queries, k = 10: the CPU model keeps 13 - 17 rows on the bfloat16 copy and 22 - 47 on the 8-bit
    plane (89 - 92 and 200 - 222 at k = 64): far under the list's 4096"""
    n, dim, k = 50_000, 768, 10
    idx = l2_index(dim); idx.add_synthetic(6400, 0, n)
    qs = O.gen_rows(6401, 0, 4, dim)
    for i in range(4):
        _, incs = both(idx, lambda: idx.search(qs[i], k))
        assert answered(incs), (i, incs)
        assert k <= incs["bf16"]["cand"] <= 4096 and k <= incs["8bit"]["cand8"] <= 4096, incs
        print("50k x 768 k=10 query %d: %d survivors of the bfloat16 stage, %d of the 8-bit stage" % (i, incs["bf16"]["cand"], incs["8bit"]["cand8"]))
    idx.close()


def test_near_duplicate_clusters_wider_than_the_list_hand_back():
    """three clusters of 20 000 near-copies at 64 dimensions: all of a cluster lies within the margin of the k-th distance of a query inside
    it (the CPU model: 20 000 survivors), so both stages pass the search on and the exact scan answers, decided on the device"""
    rng = np.random.default_rng(3)
    dim, per = 64, 20_000
    centres = rng.standard_normal((3, dim)).astype(np.float32)
    rows = np.concatenate([c + 1e-5 * rng.standard_normal((per, dim)).astype(np.float32) for c in centres])
    idx = l2_index(dim); idx.add(rows)
    q = (centres[1] + 1e-5 * rng.standard_normal(dim)).astype(np.float32)
    (r, d, c), incs = both(idx, lambda: idx.search(q, 10))
    assert answered(incs, 1, back=1), incs
    assert incs["bf16"]["cand"] > 4096 and incs["8bit"]["cand8"] > 4096 and incs["8bit"]["cand"] > 4096, incs
    assert agrees(rows, q, 10, r[0], d[0], c[0])
    q2 = rng.standard_normal(dim).astype(np.float32)
    _, incs = both(idx, lambda: idx.search(q2, 10))                       # the words are back in their initial state: the next search takes the path
    assert incs["bf16"]["took"] == 1 and incs["8bit"]["took8"] == 1 and incs["8bit"]["took"] == 1, incs
    idx.close()


def test_a_query_that_is_a_row_and_a_zero_query():
    rows, _ = L.corpus("12000x128")
    idx = l2_index(128); idx.add(rows)
    for k in (1, 10):
        (r, d, c), incs = both(idx, lambda: idx.search(rows[4321], k))
        assert answered(incs), incs
        assert int(r[0, 0]) == 4321 and d[0, 0].view(np.uint32) == 0      # exactly +0.0
    # a zero query is a legitimate Euclidean query, but its norm is not one the bound works with: handed back, the exact scan's answer
    zero = np.zeros(128, np.float32)
    (r, d, c), incs = both(idx, lambda: idx.search(zero, 10))
    assert answered(incs, 1, back=1), incs
    assert agrees(rows, zero, 10, r[0], d[0], c[0])
    (r, d, c), incs = both(idx, lambda: idx.search(rows[5], 10))          # and the next search takes the path again
    assert answered(incs) and int(r[0, 0]) == 5
    idx.close()


def test_tombstones_updates_duplicates_and_ties():
    """integer-valued rows give many EQUAL Euclidean distances: the order by row must hold"""
    rng = np.random.default_rng(11)
    dim, n = 128, 12_000
    rows = O.gen_rows(500, 0, n, dim)
    rows[64 * 5 + 3] = rows[7]; rows[64 * 100 + 63] = rows[7]; rows[n - 1] = rows[7]          # exact duplicates across tiles
    small = rng.integers(-1, 2, (600, dim)).astype(np.float32)                               # ties: many equal distances
    rows[3000:3600] = small
    idx = l2_index(dim); idx.add(rows)
    for q in (rows[7], small[5], O.gen_rows(501, 0, 1, dim)[0]):
        for k in (1, 10, 64):
            (r, d, c), incs = both(idx, lambda: idx.search(q, k))
            assert incs["bf16"]["took"] == 1 and incs["8bit"]["took8"] == 1, incs
            assert agrees(rows, q, k, r[0], d[0], c[0]), k
    # removes and updates after the build: the planes, the scales and the residuals follow
    gone = np.unique(np.concatenate([np.arange(0, 2000), [64 * 5 + 3, 7]])).astype(np.uint32)
    idx.remove(gone)
    idx.update(9000, rows[7]); idx.update(4, (rows[7] * np.float32(1.0 + 1e-6)).astype(np.float32))
    alive = np.ones(n, bool); alive[gone] = False; alive[4] = True
    rows2 = rows.copy(); rows2[9000] = rows[7]; rows2[4] = (rows[7] * np.float32(1.0 + 1e-6)).astype(np.float32)
    (r, d, c), incs = both(idx, lambda: idx.search(rows[7], 10))
    assert answered(incs), incs
    assert agrees(rows2, rows[7], 10, r[0], d[0], c[0], alive=alive)
    # fewer than k live rows (the call asks for what is there)
    idx.remove(np.arange(0, n - 5, dtype=np.uint32))
    (r, d, c), incs = both(idx, lambda: idx.search(rows[7], 10))
    assert int(c[0]) == 5 and incs["bf16"]["took"] == 1 and incs["8bit"]["took8"] == 1, incs
    idx.close()


def test_a_partly_padded_last_tile_and_a_wholly_dead_tile():
    rows, qs = L.corpus("12000x128")                                       # 12 000 = 187 tiles and 32 rows
    idx = l2_index(128); idx.add(rows)
    alive = np.ones(len(rows), bool)
    near = O.exact_search(L.L2, rows, qs[2], 1)[0][0]
    dead_tile = int(near) // 64                                            # the tile of the nearest row, whole, and the last full tile
    for t in (dead_tile, 186):
        alive[t * 64:(t + 1) * 64] = False
    idx.remove(np.flatnonzero(~alive).astype(np.uint32))
    for k in (1, 10, 64):
        (r, d, c), incs = both(idx, lambda: idx.search(qs[2], k))
        assert answered(incs), (k, incs)
        assert agrees(rows, qs[2], k, r[0], d[0], c[0], alive=alive) and not np.isin(r[0] // 64, (dead_tile, 186)).any()
    q = rows[len(rows) - 1]                                                # the answer in the padded tile
    (r, d, c), incs = both(idx, lambda: idx.search(q, 10))
    assert answered(incs) and int(r[0, 0]) == len(rows) - 1 and agrees(rows, q, 10, r[0], d[0], c[0], alive=alive)
    idx.close()


# ---- shared passes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [2, 4, 5, 8])
def test_shared_passes_with_one_query_the_bound_cannot_decide(nq):
    """2 and 4 queries (QB = 4), 5 and 8 (QB = 8) in one call; slot 1 is a zero query: it goes on alone, the others keep their answers"""
    rows, qs = L.corpus("12000x128")
    idx = l2_index(128); idx.add(rows)
    block = np.array(qs[:nq]); block[1] = 0.0
    for k in (1, 10, 64):
        (r, d, c), incs = both(idx, lambda: idx.search(block, k))
        assert answered(incs, nq, back=1), (k, incs)
        for j in (0, nq - 1):
            assert agrees(rows, block[j], k, r[j], d[j], c[j]), (k, j)
    (r, d, c), incs = both(idx, lambda: idx.search(qs[:nq], 10))           # all decidable: the model's largest count of the pass
    assert answered(incs, nq), incs
    if nq == 2:
        assert incs["bf16"]["cand"] == max(L.RECORDED["12000x128"][("bf16", j, 10)] for j in range(2))
        assert incs["8bit"]["cand8"] == max(L.RECORDED["12000x128"][("8bit", j, 10)] for j in range(2))
    idx.close()


def test_four_concurrent_single_query_callers():
    rows, qs = L.corpus("12000x128")
    idx = l2_index(128); idx.add(rows)
    idx.set_bound_scan("never")
    er, ed, ec = idx.search(qs, 10)
    for plane in PLANES:
        idx.set_bound_scan("always"); set_planes(idx, plane)
        s0 = idx.bound_scan_stats()
        res = _callers.run("index", idx.handle, qs, 10, threads=4, seconds=20.0, max_calls_per_thread=8)
        assert res["rc"] == 0, res["error"]
        assert res["errors"] == 0 and res["mismatches"] == 0 and res["calls"] == 32
        s1 = idx.bound_scan_stats()
        assert s1["searches"] - s0["searches"] == 32 and s1["hand_backs"] == s0["hand_backs"], (plane, s0, s1)
        seen = res["count"] != 0xFFFFFFFD
        assert seen.any()
        assert np.array_equal(res["rows"][seen], er[seen]) and np.array_equal(res["dist"][seen].view(np.uint32), ed[seen].view(np.uint32)), plane
    idx.close()


# ---- filtered ------------------------------------------------------------------------------------------------------------------------------
def filtered_case():
    rows, qs = L.corpus("12000x128")
    n = len(rows)
    rng = np.random.default_rng(6500)
    striped = np.zeros(n, bool)
    for t in range(0, (n + 63) // 64, 3):
        striped[t * 64:(t + 1) * 64] = True                                # one tile in three
    few = np.zeros(n, bool); few[[70, 5000, 11_999]] = True                # fewer than k live rows
    return rows, qs, {"half": rng.random(n) < 0.5, "striped": striped, "few": few}


def test_under_a_mask():
    rows, qs, m = filtered_case()
    idx = l2_index(128); idx.add(rows)
    for nq in (1, 4):
        for name in ("half", "striped"):
            (r, d, c), incs = both(idx, lambda: idx.search_masked(qs[:nq], 10, m[name]))
            assert answered(incs, nq), (nq, name, incs)
            for j in range(nq):
                assert agrees(rows, qs[j], 10, r[j], d[j], c[j], alive=m[name]), (nq, name, j)
    idx.close()


def test_a_row_set_per_query():
    """no set, a random half, one tile in three, and a set of 3 rows — fewer than k: no k-th upper bound, handed back alone"""
    rows, qs, m = filtered_case()
    idx = l2_index(128); idx.add(rows)
    masks = [None, m["half"], m["striped"], m["few"]]
    sets = [None if x is None else idx.rowset(x) for x in masks]
    every = np.ones(len(rows), bool)
    (r, d, c), incs = both(idx, lambda: idx.search_rowsets(qs[:4], 10, sets))
    assert answered(incs, 4, back=1), incs
    assert c.tolist() == [10, 10, 10, 3]
    for j in range(4):
        assert agrees(rows, qs[j], 10, r[j], d[j], c[j], alive=every if masks[j] is None else masks[j]), j
    for j in range(4):                                                     # the same as single-query calls
        (r, d, c), incs = both(idx, lambda: idx.search_rowsets(qs[j:j + 1], 10, sets[j:j + 1]))
        assert answered(incs, 1, back=1 if j == 3 else 0), (j, incs)
        assert agrees(rows, qs[j], 10, r[0], d[0], c[0], alive=every if masks[j] is None else masks[j]), j
    idx.close()


def test_a_where_filter_per_query():
    rows, qs, _ = filtered_case()
    n = len(rows)
    idx = l2_index(128); idx.add(rows)
    vals = np.random.default_rng(6501).integers(0, 10, n).astype(np.uint32)
    col = idx.column("u32"); col.set(0, vals)
    specs = [[(col, "lt", 5)], [(col, "eq", 3)], None, [(col, "in", [1, 9])]]
    masks = [vals < 5, vals == 3, np.ones(n, bool), np.isin(vals, (1, 9))]
    (r, d, c), incs = both(idx, lambda: idx.search_where(qs[:4], 10, specs))
    assert answered(incs, 4), incs
    for j in range(4):
        assert agrees(rows, qs[j], 10, r[j], d[j], c[j], alive=masks[j]), j
    for j in (0, 1):
        (r, d, c), incs = both(idx, lambda: idx.search_where(qs[j:j + 1], 10, [specs[j]]))
        assert answered(incs, 1), (j, incs)
        assert agrees(rows, qs[j], 10, r[0], d[0], c[0], alive=masks[j]), j
    idx.close()


# ---- the opt-outs ----------------------------------------------------------------------------------------------------------------------------
def took_nothing(idx, q):
    (r, d, c), incs = both(idx, lambda: idx.search(q, 10))
    return all(v["took"] == 0 and v["took8"] == 0 for v in incs.values()), r


def test_the_opt_outs():
    rows, _ = L.corpus("12000x128")
    for make in ("plain", "no_scan_plane", "oom", "cosine"):
        if make == "oom":
            os.environ["QV_TEST_PLANE_OOM"] = "1"                          # the copy's allocation answers out-of-memory: not an error, no planes
        try:
            if make == "cosine":
                idx = quiver_amd.DeviceIndex(128, "cosine", l2_scan_plane=True)
            else:
                idx = quiver_amd.DeviceIndex(128, "l2", l2_scan_plane=make != "plain", scan_plane=make != "no_scan_plane")
            idx.add(rows)
        finally:
            os.environ.pop("QV_TEST_PLANE_OOM", None)
        if make == "cosine":                                               # the flag does nothing there: the default planes, the default path
            plain = quiver_amd.DeviceIndex(128, "cosine"); plain.add(rows)
            assert idx.bound_scan_stats()["plane"] and idx.bound_scan8_stats()["plane"]
            (r, d, c), incs = both(idx, lambda: idx.search(rows[3], 10))
            (pr, pd, pc), pincs = both(plain, lambda: plain.search(rows[3], 10))
            assert incs == pincs and answered(incs) and np.array_equal(r, pr) and X.same(d, pd)
            plain.close()
        else:
            assert not idx.bound_scan_stats()["plane"] and not idx.bound_scan8_stats()["plane"], make
            none, r = took_nothing(idx, rows[3])
            assert none and int(r[0, 0]) == 3, make
            none, _ = took_nothing(idx, rows[3:7])
            assert none, make
        idx.close()
    # a copy for the batched filter alone (QV_FLAG_BF16_ROWS) is no scan plane
    idx = quiver_amd.DeviceIndex(128, "l2", bf16_rows=True); idx.add(rows)
    assert took_nothing(idx, rows[3])[0]
    idx.close()
    # 100 dimensions: no multiple of 16 — the copy is kept, the 8-bit plane is not, and the path declines
    rows100 = O.gen_rows(87, 0, 5000, 100)
    idx = l2_index(100); idx.add(rows100)
    assert not idx.bound_scan8_stats()["plane"]
    none, r = took_nothing(idx, rows100[3])
    assert none and int(r[0, 0]) == 3
    idx.close()
    # the automatic modes leave a flagged index of this size alone: its floors start at 300 000 rows
    idx = l2_index(128); idx.add(rows)
    idx.set_bound_scan("auto"); set_planes(idx, "auto")
    s0 = idx.bound_scan_stats()["searches"]
    idx.search(rows[3], 10); idx.search(rows[3:7], 10)
    assert idx.bound_scan_stats()["searches"] == s0
    # qv_index_create rejects the rule code as a metric; the index still answers QV_L2
    import ctypes as C
    h = C.c_void_p()
    assert _lib.lib().qv_index_create(C.byref(h), 128, L.RULE_L2_PLANES, 0, 0) < 0
    assert idx.metric == L.L2
    idx.close()


def test_sharded_handle():
    """three co-located shards of 3 000 rows each behind the point-to-point exchange: each shard's own index takes the path"""
    n, dim, k = 9_000, 128, 10
    rows = O.gen_rows(6600, 0, n, dim)
    qs = O.gen_rows(6601, 0, 4, dim)
    sh = quiver_amd.ShardedIndex(dim, "l2", devices=[0, 0, 0], peer_copy=True, l2_scan_plane=True)
    gids = sh.add(rows)
    assert sh.bound_scan_stats()["plane"] and sh.bound_scan8_stats()["plane"]
    for nq in (1, 4):
        sh.set_bound_scan("never")
        s0 = sh.bound_scan_stats()
        er, ed, ec = sh.search(qs[:nq], k)
        assert sh.bound_scan_stats()["searches"] == s0["searches"]
        for plane in PLANES:
            sh.set_bound_scan("always"); sh.set_bound_plane(plane); sh.set_bound_plane_mq(plane)
            s0, a0 = sh.bound_scan_stats(), sh.bound_scan8_stats()
            r, d, c = sh.search(qs[:nq], k)
            s1, a1 = sh.bound_scan_stats(), sh.bound_scan8_stats()
            assert np.array_equal(c, ec) and np.array_equal(r, er) and np.array_equal(d.view(np.uint32), ed.view(np.uint32)), (nq, plane)
            assert s1["searches"] - s0["searches"] == 3 * nq and s1["hand_backs"] == s0["hand_backs"], (nq, plane, s0, s1)
            assert a1["searches"] - a0["searches"] == (3 * nq if plane == "8bit" else 0), (nq, plane, a0, a1)
    for j in range(4):                                                     # (the 4-query call under "never", against the oracle)
        want_r, want_d = O.exact_search(L.L2, rows, qs[j], k)
        assert np.array_equal(er[j], gids[want_r]) and np.array_equal(ed[j].view(np.uint32), want_d.view(np.uint32)), j
    sh.close()


def test_debug_read_serves_a_flagged_index():
    rows, _ = L.corpus("2000x16")
    idx = l2_index(16); idx.add(rows)
    st = B.RowState(rows)
    assert np.array_equal(idx.debug_read("rres")[:len(rows)].view(np.uint32), st.rres.view(np.uint32))
    assert np.array_equal(idx.debug_read("rnorm")[:len(rows)], st.rn)
    plane = idx.debug_read("plane")                                        # [tile][step][2 row blocks][2 halves][32 rows][8 values]
    t = plane.reshape(-1, 1, 2, 2, 32, 8)
    got = t.transpose(0, 2, 4, 1, 3, 5).reshape(-1, 16)[:len(rows)]       # -> [tile][block][row][step][half][value] = rows x 16
    assert np.array_equal(got, (st.rh.view(np.uint32) >> 16).astype(np.uint16))
    idx.close()
    plain = quiver_amd.DeviceIndex(16, "l2"); plain.add(rows)
    with pytest.raises(quiver_amd.QvError):
        plain.debug_read("plane")
    plain.close()
