"""The wide form of the SHARED bound pass: one unfiltered call of 2 to 8 queries at 65 <= k <= 1024 (k_bound_scan_mq / k_bound_scan8_mq with the
wide tail, the selection of H per query, k_bound_collect_wide_mq, k_bound_rescore_wide_mq, the counted selection over all queries and the
flagged key-per-row redo; quiver_amd/csrc/qv_bound_scan.hip).  Every case forces the form by the index's own setter
(set_bound_scan_wide_mq("always")) and names the plane that comes first (set_bound_plane_mq); every result is compared, rows, float32 bits
and counts, with the same index under "never", one cell per metric with the CPU oracle — and the form's own counters say what answered
which query: a case that says "answered" must see took == nq and back == 0, so no test here passes on a hand-back alone.  The inputs of
those cases were checked on the CPU against the model (tests/_wide_mq.py: tests/_wide.decide_wide per query) for 256 compute units: it
hands none of them back."""
import numpy as np
import pytest

import quiver_amd
from quiver_amd import _lib
from quiver_amd.device_index import device_info
from tests import _bound as B
from tests import _extremes as X
from tests import _oracle as O
from tests import _wide as Wd
from tests import _wide_mq as M

pytestmark = pytest.mark.gpu

CAP = _lib.QV_BOUND_WIDE_CAND_CAP
KS = (65, 128, 129, 500, 1024)
NQS = (2, 3, 4, 5, 8)                                  # QB = 4 with empty slots and full, QB = 8 with empty slots and full
ARMS = ("bf16", "8bit")


def make(metric, dim, **kw):
    return quiver_amd.DeviceIndex(dim, metric, l2_scan_plane=(metric == "l2"), **kw)


def counters(idx):
    """every other counter group of the index: none of them may move for a wide shared pass"""
    return (idx.bound_scan_stats(), idx.bound_scan8_stats(), idx.bound_scan6_stats(), idx.bound_scan_wide_stats())


def wide_only(idx, call, plane):
    """one call under "always" with `plane` first -> (result, the form's counters' increments)"""
    idx.set_bound_scan_wide_mq("always"); idx.set_bound_plane_mq(plane)
    s0 = idx.bound_scan_wide_mq_stats()
    res = call()
    s1 = idx.bound_scan_wide_mq_stats()
    return res, {"took": s1["searches"] - s0["searches"], "back": s1["hand_backs"] - s0["hand_backs"], "cand": s1["candidates"]}


def exact_of(idx, call):
    idx.set_bound_scan_wide_mq("never")
    s0 = idx.bound_scan_wide_mq_stats()
    res = call()
    assert idx.bound_scan_wide_mq_stats()["searches"] == s0["searches"]        # "never" is never
    return res


def both(idx, call, plane, exact=None):
    """... and the same call under "never" on the same index: rows, float32 bits and counts are the same"""
    (r, d, c), inc = wide_only(idx, call, plane)
    er, ed, ec = exact if exact is not None else exact_of(idx, call)
    assert np.array_equal(c, ec) and np.array_equal(r, er), (plane, r, er)
    assert X.same(d, ed), (plane, d, ed)
    return (r, d, c), inc


def answered(inc, nq):
    return inc["took"] == nq and inc["back"] == 0


def is_oracle(want, r, d, c):
    er, ed = want
    return int(c) == len(er) and np.array_equal(r, er) and np.array_equal(d.view(np.uint32), ed.view(np.uint32))


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
@pytest.mark.parametrize("n,dim", [(6001, 80), (2000, 16), (200_000, 64)])
def test_rows_and_bits_of_the_exact_path(metric, n, dim):
    """a ragged last tile and a 4 + 1 step split (6 001 x 80); the narrowest row (2 000 x 16); 3 125 tiles, so that waves walk several and the
    8-bit pre-test is at work (200 000 x 64).  Every nq of both QB, every k, both planes.  One cell per metric against the CPU oracle; on
    6 001 x 80 with the bfloat16 arm the largest survivor count is at least the largest of the CPU model's per-query counts."""
    idx = make(metric, dim)
    seed = 7100 + dim
    idx.add_synthetic(seed, 0, n)
    assert idx.bound_scan_wide_mq_stats()["plane"] and idx.bound_scan8_stats()["plane"]
    qs = O.gen_rows(seed + 1, 0, 8, dim)
    mid = quiver_amd.metric_id(metric)
    corpus = O.gen_rows(seed, 0, n, dim) if n == 6001 else None
    states = M.States(corpus, arms=("bf16",)) if corpus is not None else None
    for nq in NQS:
        for k in KS:
            call = lambda: idx.search(qs[:nq], k)                          # noqa: E731
            exact = exact_of(idx, call)
            assert (exact[2] == k).all()
            for plane in ARMS:
                _, inc = both(idx, call, plane, exact)
                assert answered(inc, nq), (nq, k, plane, inc)
                assert k <= inc["cand"] <= CAP, (nq, k, plane, inc)
                if plane == "bf16" and states is not None:
                    floor = max(B.decide(M.stage_of(mid, "bf16", states, qs[j]), k, cap=CAP)["count"] for j in range(nq))
                    assert inc["cand"] >= floor, (nq, k, inc, floor)
    if corpus is not None:
        (r, d, c), inc = wide_only(idx, lambda: idx.search(qs[:3], 129), "8bit")
        assert answered(inc, 3)
        for j in range(3):
            assert is_oracle(O.exact_search(mid, corpus, qs[j], 129), r[j], d[j], c[j]), j
    idx.close()


def test_survivor_counts_pinned_one_near_cluster_per_query():
    """tests/test_gpu_bound_scan_wide.py's test_nearest_rows_stored_together with a cluster per query: rows 1024 j .. 1024 j + 1023 are the
    1024 nearest of query j, sixteen neighbouring tiles that belong to sixteen DIFFERENT waves (tile t belongs to wave t mod (4 * grid)), so
    nothing is dropped, H_j is the exact k-th smallest upper bound, and the pass's largest survivor count is the largest of the CPU model's
    per-query counts (tests/_wide.decide_wide), on both planes.  Three queries: QB = 4 with an empty slot."""
    dim, n, nq = 64, 200_000, 3
    rng = np.random.default_rng(72)
    qs = rng.standard_normal((nq, dim)).astype(np.float32)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    for j in range(nq):
        rows[1024 * j:1024 * (j + 1)] = (qs[j][None, :] + np.float32(0.05) * rows[1024 * j:1024 * (j + 1)]).astype(np.float32)
    idx = make("cosine", dim); idx.add(rows)
    n_tiles = (n + 63) // 64
    grid, stride = Wd.plan(n_tiles, device_info(0)["cus"])
    states = M.States(rows)
    live = np.ones(n, bool)
    for k in (1024, 500):
        want = [O.exact_search(0, rows, qs[j], k) for j in range(nq)]
        for j in range(nq):
            assert set(want[j][0].tolist()) <= set(range(1024 * j, 1024 * (j + 1)))
        for plane in ARMS:
            (r, d, c), inc = both(idx, lambda: idx.search(qs, k), plane)
            assert answered(inc, nq), inc
            for j in range(nq):
                assert is_oracle(want[j], r[j], d[j], c[j]), (k, plane, j)
            f = M.fates(0, plane, states, qs, k, live, n_tiles, grid)
            print("k %d %s: survivors %d at the most, the model %d (%s)" % (k, plane, inc["cand"], f["cand"], f["per_query"]))
            assert all(stage == plane for stage, _, _ in f["per_query"]) and (stride < 16 or f["dropped"] == 0), (k, plane, f["per_query"])
            if f["dropped"] == 0:                                        # the count is pinned where the model says nothing was dropped (every device with a stride of 16 waves or more)
                assert inc["cand"] == f["cand"], (k, plane, inc, f["per_query"])
            else:                                                        # a looser H only passes MORE rows on than the exact k-th upper bound would
                assert inc["cand"] >= max(B.decide(M.stage_of(0, plane, states, qs[j]), k, cap=CAP)["count"] for j in range(nq)), (k, plane, inc)
    idx.close()


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
def test_a_nan_query_and_a_zero_query_are_handed_back_alone(metric):
    """in the first and the last slot of a pass of four and of eight: the 8-bit stage cannot quantise them and hands them on, the bfloat16
    stage has no threshold (NaN) or a norm it declines (zero) and hands them back — those two alone: `back` rises by exactly two and the
    other queries are answered by the form; every answer is the exact path's"""
    dim, n, k = 80, 6001, 100
    idx = make(metric, dim); idx.add_synthetic(7400, 0, n)
    ordinary = O.gen_rows(7401, 0, 8, dim)
    nan_q = ordinary[0].copy(); nan_q[5] = np.nan
    for nq, first, last in ((4, nan_q, np.zeros(dim, np.float32)), (8, np.zeros(dim, np.float32), nan_q)):
        qs = ordinary[:nq].copy(); qs[0] = first; qs[nq - 1] = last
        for plane in ARMS:
            _, inc = both(idx, lambda: idx.search(qs, k), plane)
            assert inc["took"] == nq and inc["back"] == 2, (nq, plane, inc)
            assert k <= inc["cand"] <= CAP, inc                            # the answered queries' maximum: the two handed back add nothing
        # the control words are back in their initial state: an ordinary pass behind it is answered by the form
        _, inc = both(idx, lambda: idx.search(ordinary[:nq], k), "8bit")
        assert answered(inc, nq), (nq, inc)
    idx.close()


def cluster(metric, width, rng, dim=64, n=20_000):
    """n near-copies of one unit vector at distances spread evenly over [0, width] and a query on their centre (tests/test_gpu_bound_scan8_mq.py)"""
    c = rng.standard_normal(dim); c /= np.linalg.norm(c)
    u = rng.standard_normal((n, dim)); u -= np.outer(u @ c, c); u /= np.linalg.norm(u, axis=1)[:, None]
    dist = np.linspace(0.0, width, n)
    along = (1.0 - dist) if metric == B.DOT else np.ones(n)
    return (along[:, None] * c[None, :] + np.sqrt(2.0 * dist)[:, None] * u).astype(np.float32), c.astype(np.float32)


CLUSTER_WIDTH = 0.015                                  # the cluster of tests/test_gpu_bound_scan8_mq.py at the width at which, for the wider list and k = 100, the model says 14 715 survivors (cosine) on the 8-bit arm, 4 358 on the bfloat16 arm (asserted)


@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
def test_one_query_whose_candidates_overflow_the_8bit_list_is_handed_on_alone(metric):
    """For ONE query of a pass of four (first slot) and of eight (last slot) more than QV_BOUND_WIDE_CAND_CAP rows lie within the 8-bit margin
    of its k-th distance and fewer within the bfloat16 margin — both said by the CPU model: that query is handed on alone and answered by the
    bfloat16 stage (`back` does not move, and the pass's largest survivor count is that stage's count for it); the others are answered by
    the 8-bit stage."""
    rng = np.random.default_rng(5)
    dim, k = 64, 100
    near, q = cluster(metric, CLUSTER_WIDTH, rng)
    rows = np.concatenate([near, (0.05 * rng.standard_normal((20_000, dim))).astype(np.float32)])   # (short: far from the query under dot too)
    n = len(rows)
    n_tiles = (n + 63) // 64
    grid, _ = Wd.plan(n_tiles, device_info(0)["cus"])
    states = M.States(rows)
    live = np.ones(n, bool)
    m8 = Wd.decide_wide(M.stage_of(metric, "8bit", states, q), k, live, n_tiles, grid)
    m16 = Wd.decide_wide(M.stage_of(metric, "bf16", states, q), k, live, n_tiles, grid)
    assert m8["hand_back"] and m8["count"] > CAP and not m16["hand_back"] and m16["count"] <= CAP, (m8["count"], m16["count"])
    idx = make("cosine" if metric == B.COSINE else "dot", dim); idx.add(rows)
    others = rng.standard_normal((8, dim)).astype(np.float32)
    others[others @ q > 0] *= np.float32(-1.0)                           # away from the cluster: its rows are their farthest, not 20 000 near-ties
    for nq, slot in ((4, 0), (8, 7)):
        qs = others[:nq].copy(); qs[slot] = q
        f = M.fates(metric, "8bit", states, qs, k, live, n_tiles, grid)
        assert [stage for stage, _, _ in f["per_query"]] == ["bf16" if j == slot else "8bit" for j in range(nq)], f["per_query"]
        (r, d, c), inc = both(idx, lambda: idx.search(qs, k), "8bit")
        print("nq %d: survivors %d at the most, the model %d (8-bit stage: %d)" % (nq, inc["cand"], f["cand"], m8["count"]))
        assert answered(inc, nq), (nq, inc)
        assert inc["cand"] == f["cand"] == m16["count"], (nq, inc, f["per_query"])
        for j in range(nq):
            assert is_oracle(O.exact_search(metric, rows, qs[j], k), r[j], d[j], c[j]), (nq, j)
    _, inc = both(idx, lambda: idx.search(others[:4], k), "8bit")         # the words are back in their initial state
    assert answered(inc, 4), inc
    idx.close()


def test_the_8bit_stages_maximum_survives_a_hand_on():
    """The pass's largest survivor count is a maximum over the stages that ANSWERED.  Here the query the 8-bit stage answers has the larger
    count: query 0 sits on a cluster of 6 000 rows that all lie within the 8-bit margin (about 6 000 survivors, under the list's capacity),
    query 3 on the cluster that overflows the 8-bit list and is handed on to the bfloat16 stage, which answers it with fewer (about 4 400).
    If the bfloat16 stage's launches cleared or overwrote the word, the counter would read the smaller number."""
    rng = np.random.default_rng(6)
    dim, k, nq = 64, 100, 4
    near_a, qa = cluster(B.COSINE, CLUSTER_WIDTH, rng)
    near_b, qb = cluster(B.COSINE, 0.004, rng, n=6000)
    rows = np.concatenate([near_a, near_b, (0.05 * rng.standard_normal((20_000, dim))).astype(np.float32)])
    n = len(rows)
    n_tiles = (n + 63) // 64
    grid, _ = Wd.plan(n_tiles, device_info(0)["cus"])
    pool = rng.standard_normal((64, dim)).astype(np.float32)
    others = pool[(pool @ qa < 0) & (pool @ qb < 0)][:2]                 # away from both clusters
    qs = np.stack([qb, others[0], others[1], qa])
    states = M.States(rows)
    live = np.ones(n, bool)
    f = M.fates(B.COSINE, "8bit", states, qs, k, live, n_tiles, grid)
    stages, counts = [s for s, _, _ in f["per_query"]], [c for _, c, _ in f["per_query"]]
    assert stages == ["8bit", "8bit", "8bit", "bf16"] and counts[0] > counts[3] > max(counts[1:3]) and f["cand"] == counts[0], f["per_query"]
    idx = make("cosine", dim); idx.add(rows)
    (r, d, c), inc = both(idx, lambda: idx.search(qs, k), "8bit")
    print("survivors %d at the most, the model %s" % (inc["cand"], f["per_query"]))
    assert answered(inc, nq), inc
    assert inc["cand"] == counts[0], (inc, f["per_query"])
    for j in (0, 3):
        assert is_oracle(O.exact_search(B.COSINE, rows, qs[j], k), r[j], d[j], c[j]), j
    idx.close()


@pytest.mark.parametrize("k", [65, 129])
def test_ties_across_the_kth_place(k):
    """for the middle query of a pass of three, exact duplicates of one row in three different tiles take ranks k - 1, k and k + 1: the two
    with the smaller row numbers are in its answer, in (distance, row) order"""
    dim, n = 80, 6001
    rows = O.gen_rows(7300, 0, n, dim)
    qs = O.gen_rows(7301, 0, 3, dim)
    q = qs[1]
    order, _ = O.exact_search(0, rows, q, n)
    src = int(order[k - 2])                                              # rank k - 1 (1-based)
    far = [int(r) for r in order[::-1] if int(r) // 64 != src // 64][:400]
    a = far[0]
    b = next(r for r in far if r // 64 != a // 64)
    rows[a] = rows[src]; rows[b] = rows[src]
    er, ed = O.exact_search(0, rows, q, k)
    trio = sorted([src, a, b])
    assert er[k - 2] == trio[0] and er[k - 1] == trio[1] and trio[2] not in er.tolist()   # the shape is what it is built to be
    idx = make("cosine", dim); idx.add(rows)
    for plane in ARMS:
        (r, d, c), inc = both(idx, lambda: idx.search(qs, k), plane)
        assert answered(inc, 3), inc
        assert is_oracle((er, ed), r[1], d[1], c[1]), (plane, r[1][-4:], er[-4:])
        for j in (0, 2):
            assert is_oracle(O.exact_search(0, rows, qs[j], k), r[j], d[j], c[j]), (plane, j)
    idx.close()


def test_dead_rows_a_dead_tile_and_k_at_the_live_rows():
    """scattered dead rows and a wholly dead tile: never candidates, never in a threshold.  k at or above the live rows: the pass keeps
    today's path and the counters stay."""
    dim, n = 16, 2000
    rows = O.gen_rows(7900, 0, n, dim)
    idx = make("cosine", dim); idx.add(rows)
    qs = O.gen_rows(7901, 0, 4, dim)
    rng = np.random.default_rng(79)
    gone = np.unique(np.concatenate([np.arange(64 * 11, 64 * 12), rng.permutation(n)[:300]])).astype(np.uint32)
    idx.remove(gone)
    alive = np.ones(n, bool); alive[gone] = False
    for plane in ARMS:
        (r, d, c), inc = both(idx, lambda: idx.search(qs, 100), plane)
        assert answered(inc, 4), (plane, inc)
        for j in range(4):
            assert is_oracle(O.exact_search(0, rows, qs[j], 100, alive=alive), r[j], d[j], c[j]), (plane, j)
    more = np.flatnonzero(alive)[:int(alive.sum()) - 900].astype(np.uint32)
    idx.remove(more)                                                     # 900 live rows
    (r, d, c), inc = both(idx, lambda: idx.search(qs, 1000), "8bit")
    assert (c == 900).all() and inc["took"] == 0 and inc["back"] == 0, inc
    (r, d, c), inc = both(idx, lambda: idx.search(qs, 900), "8bit")      # every live row: nothing to reject
    assert (c == 900).all() and inc["took"] == 0 and inc["back"] == 0, inc
    (r, d, c), inc = both(idx, lambda: idx.search(qs, 899), "8bit")
    assert (c == 899).all() and answered(inc, 4), inc
    idx.close()


def test_after_remove_and_update_rows_the_form_equals_the_exact_path():
    dim, n, nq = 80, 12_001, 5
    rows = O.gen_rows(7800, 0, n, dim)
    qs = O.gen_rows(7801, 0, nq, dim)
    idx = make("cosine", dim); idx.add(rows)
    top, _ = O.exact_search(0, rows, qs[0], 300)
    rng = np.random.default_rng(78)
    gone = np.unique(np.concatenate([top[::3], rng.permutation(n)[:2000]]))[:2000].astype(np.uint32)
    idx.remove(gone)
    alive = np.ones(n, bool); alive[gone] = False
    upd = rng.permutation(np.flatnonzero(alive))[:300].astype(np.uint32)
    vecs = O.gen_rows(7802, 0, 300, dim)
    vecs[:20] = (qs[nq - 1][None, :] + np.float32(0.1) * vecs[:20]).astype(np.float32)   # some of the new rows belong in the last query's answer
    idx.update_rows(upd, vecs)
    rows2 = rows.copy(); rows2[upd] = vecs
    for k in (65, 300, 1024):
        for plane in ARMS:
            (r, d, c), inc = both(idx, lambda: idx.search(qs, k), plane)
            assert answered(inc, nq), (k, plane, inc)
            for j in (0, nq - 1):
                assert is_oracle(O.exact_search(0, rows2, qs[j], k, alive=alive), r[j], d[j], c[j]), (k, plane, j)
    idx.close()


def test_declined_calls_keep_their_paths():
    """one query, nine queries, k = 64, k = 1025, a masked call of two queries, an index without the scan planes: no counter of the form moves"""
    dim, n = 80, 6001
    idx = make("cosine", dim); idx.add_synthetic(8400, 0, n)
    qs = O.gen_rows(8401, 0, 9, dim)
    mask = np.ones(n, bool); mask[::7] = False
    calls = {"nq 1": lambda: idx.search(qs[0], 100), "nq 9": lambda: idx.search(qs, 100), "k 64": lambda: idx.search(qs[:4], 64),
             "k 1025": lambda: idx.search(qs[:4], 1025), "masked": lambda: idx.search_masked(qs[:2], 100, mask)}
    for name, call in calls.items():
        idx.set_bound_scan_wide_mq("always"); idx.set_bound_plane_mq("8bit")
        s0 = idx.bound_scan_wide_mq_stats()
        r, d, c = call()
        assert idx.bound_scan_wide_mq_stats() == s0, name
        er, ed, ec = exact_of(idx, call)
        assert np.array_equal(r, er) and X.same(d, ed) and np.array_equal(c, ec), name
    idx.close()
    bare = make("cosine", dim, scan_plane=False); bare.add_synthetic(8400, 0, n)
    bare.set_bound_scan_wide_mq("always"); bare.set_bound_plane_mq("8bit")
    r, d, c = bare.search(qs[:4], 100)
    s = bare.bound_scan_wide_mq_stats()
    assert not s["plane"] and s["searches"] == 0 and s["hand_backs"] == 0, s
    corpus = O.gen_rows(8400, 0, n, dim)
    assert is_oracle(O.exact_search(0, corpus, qs[3], 100), r[3], d[3], c[3])
    bare.close()


def test_nothing_set_takes_nothing():
    dim, n, k = 80, 6001, 100
    idx = make("cosine", dim); idx.add_synthetic(8300, 0, n)
    qs = O.gen_rows(8301, 0, 8, dim)
    for nq in (2, 4, 8):
        idx.search(qs[:nq], k)
    s = idx.bound_scan_wide_mq_stats()
    assert s["searches"] == 0 and s["hand_backs"] == 0 and s["candidates"] == 0, s   # automatic: no measured cell at this size, so nothing
    idx.close()


def test_counters_and_knobs_are_independent():
    """the k <= 64 counters, the 8-bit, 6-bit and single-query wide counters do not move for wide shared passes; the single-query wide knob
    does not reach two queries, nor this form's knob a single query, nor the k <= 64 knob either form"""
    dim, n, k = 80, 6001, 100
    idx = make("cosine", dim); idx.add_synthetic(8300, 0, n)
    qs = O.gen_rows(8301, 0, 4, dim)
    before = counters(idx)
    for plane in ARMS:
        _, inc = both(idx, lambda: idx.search(qs, k), plane)
        assert answered(inc, 4)
    assert counters(idx) == before
    idx.set_bound_scan_wide_mq("auto"); idx.set_bound_scan_wide("always"); idx.set_bound_plane("8bit")
    s0 = idx.bound_scan_wide_mq_stats()
    idx.search(qs[:2], k)                                                # two queries under the SINGLE-query knob: neither form
    assert idx.bound_scan_wide_mq_stats() == s0 and counters(idx) == before
    idx.set_bound_scan_wide("never"); idx.set_bound_scan_wide_mq("always")
    idx.search(qs[0], k)                                                 # one query under THIS form's knob: neither form
    assert idx.bound_scan_wide_mq_stats() == s0 and counters(idx) == before
    idx.set_bound_scan_wide_mq("never"); idx.set_bound_scan("always")
    idx.search(qs, k)                                                    # the k <= 64 knob does not reach 65 results
    assert idx.bound_scan_wide_mq_stats() == s0 and counters(idx) == before
    idx.set_bound_scan("auto")
    idx.close()


def test_device_pointers_twice_on_one_stream():
    """search_device with four queries at k = 100, twice on one non-default stream without a synchronise in between: one workspace, one set
    of control words — the second call's answers are right, so the first left the words zero"""
    import torch
    dim, n, k, nq = 64, 50_000, 100, 4
    idx = make("cosine", dim); idx.add_synthetic(8000, 0, n)
    qa, qb = O.gen_rows(8001, 0, nq, dim), O.gen_rows(8002, 0, nq, dim)
    exact = [exact_of(idx, lambda q=q: idx.search(q, k)) for q in (qa, qb)]
    st = torch.cuda.Stream()
    for plane in ARMS:
        idx.set_bound_scan_wide_mq("always"); idx.set_bound_plane_mq(plane)
        s0 = idx.bound_scan_wide_mq_stats()
        dq = [torch.from_numpy(np.array(q, dtype=np.float32)).cuda() for q in (qa, qb)]
        outs = [(torch.zeros((nq, k), dtype=torch.int32, device="cuda"), torch.zeros((nq, k), dtype=torch.float32, device="cuda")) for _ in range(2)]
        torch.cuda.synchronize()
        for i in range(2):
            idx.search_device(dq[i].data_ptr(), nq, k, outs[i][0].data_ptr(), outs[i][1].data_ptr(), st.cuda_stream)
        st.synchronize()
        s1 = idx.bound_scan_wide_mq_stats()
        assert s1["searches"] - s0["searches"] == 2 * nq and s1["hand_backs"] == s0["hand_backs"], (plane, s0, s1)
        for i in range(2):
            r = outs[i][0].cpu().numpy().view(np.uint32); d = outs[i][1].cpu().numpy()
            assert np.array_equal(r, exact[i][0]) and np.array_equal(d.view(np.uint32), exact[i][1].view(np.uint32)), (plane, i)
    idx.close()
