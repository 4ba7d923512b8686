"""The wide form of the bound scan for ONE filtered query, 65 <= k <= 1024 (k_bound_scan<., true, true> / k_bound_scan8<., true, true> over the
call's candidate bitmap, then the unfiltered wide form's selection of H, collect, re-score, counted selection and gated key-per-row redo;
quiver_amd/csrc/qv_bound_scan.hip).  Every case forces the form by the index's own setter (set_bound_scan_wide_filtered("always")) and names
the plane that comes first (set_bound_plane_filtered); every result is compared — rows, float32 bits, counts and padding — with the SAME
index under "never", one cell per metric with the CPU oracle over live & set; and the wide form's own counters say what answered: a case
here must not pass on a hand-back alone.  The rule takes a call only when the filter leaves MORE live candidates than results
(qv_scan_bound_wide_route_filtered), so where a grid cell's set is not longer than k the case asserts the opposite: not taken, same results."""
import threading

import numpy as np
import pytest

import quiver_amd
from quiver_amd import _lib
from tests import _extremes as X
from tests import _oracle as O

pytestmark = pytest.mark.gpu

CAP = _lib.QV_BOUND_WIDE_CAND_CAP
KS = (65, 128, 129, 500, 1024)
ARMS = ("bf16", "8bit")


def make(metric, dim):
    return quiver_amd.DeviceIndex(dim, metric, l2_scan_plane=(metric == "l2"))


def stats(idx):
    return idx.bound_scan_wide_stats()


def inc_of(s0, s1):
    return {"took": s1["searches"] - s0["searches"], "back": s1["hand_backs"] - s0["hand_backs"], "cand": s1["candidates"]}


def wide_only(idx, call, plane):
    """one filtered call under "always" with `plane` first -> (result, the wide counters' increments)"""
    idx.set_bound_scan_wide_filtered("always"); idx.set_bound_plane_filtered(plane)
    s0 = stats(idx)
    res = call()
    return res, inc_of(s0, stats(idx))


def exact_of(idx, call):
    idx.set_bound_scan_wide_filtered("never")
    s0 = stats(idx)
    res = call()
    assert stats(idx)["searches"] == s0["searches"]                     # "never" is never
    return res


def same_result(got, want):
    (r, d, c), (er, ed, ec) = got, want
    return bool(np.array_equal(c, ec) and np.array_equal(r, er) and X.same(d, ed))


def both(idx, call, plane, exact=None):
    """... and today's path of the same index: rows, float32 bits, counts and padding are the same"""
    got, inc = wide_only(idx, call, plane)
    want = exact if exact is not None else exact_of(idx, call)
    assert same_result(got, want), (plane, got[2], want[2], got[0], want[0])
    return got, inc


def answered(inc):
    return inc["took"] == 1 and inc["back"] == 0


def filters_of(idx, n, seed):
    """name -> (the selected rows as a bool mask, the call's filter: ("mask", mask) or ("set", RowSet))"""
    rng = np.random.default_rng(seed)
    tile = np.arange(n) // 64
    seventh = np.ones(n, bool); seventh[::7] = False                     # a mask dropping every seventh row
    half = rng.random(n) < 0.5                                           # a random set of about half the rows
    stripes = tile % 3 == 0                                              # whole tiles, one in three: SKIP skips tiles, some waves publish a dead list
    tail = rng.random(n) < 0.5                                           # ... whose only candidates in the last tile are its last three rows
    tail[tile == tile[-1]] = False; tail[-3:] = True
    out = {"seventh": (seventh, ("mask", seventh))}
    for name, m in (("half", half), ("stripes", stripes), ("tail", tail)):
        out[name] = (m, ("set", idx.rowset(m)))
    return out


def caller(idx, q, k, filt):
    kind, f = filt
    if kind == "mask":
        return lambda: idx.search_masked(q, k, f)
    return lambda: idx.search_rowsets(q, k, f)


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
@pytest.mark.parametrize("n,dim", [(6001, 80), (2000, 16)])
def test_rows_and_bits_of_todays_path(metric, n, dim):
    """a ragged last tile and a 4 + 1 step split (6 001 x 80); the narrowest row (2 000 x 16).  Candidates never exceed 6 001 < the list's
    capacity, so the list cannot overflow whatever H is: every taken call is answered, with k <= survivors <= candidates."""
    idx = make(metric, dim)
    seed = 9100 + dim
    idx.add_synthetic(seed, 0, n)
    assert stats(idx)["plane"] and idx.bound_scan8_stats()["plane"]
    q = O.gen_rows(seed + 1, 0, 1, dim)[0]
    fl = filters_of(idx, n, seed)
    for name, (m, filt) in fl.items():
        live = int(m.sum())
        for k in KS:
            call = caller(idx, q, k, filt)
            exact = exact_of(idx, call)
            assert int(exact[2][0]) == min(k, live)
            for plane in ARMS:
                _, inc = both(idx, call, plane, exact)
                if live > k:
                    assert answered(inc), (name, k, plane, inc)
                    assert k <= inc["cand"] <= live, (name, k, plane, inc)
                else:                                                    # a k that takes every candidate: the call keeps its path
                    assert inc["took"] == 0 and inc["back"] == 0, (name, k, plane, inc)
    # one cell against the CPU oracle over live & set
    corpus = O.gen_rows(seed, 0, n, dim)
    mid = quiver_amd.metric_id(metric)
    k = 129
    for name in ("stripes", "tail"):
        m, filt = fl[name]
        er, ed = O.exact_search(mid, corpus, q, k, alive=m)
        (r, d, c), inc = wide_only(idx, caller(idx, q, k, filt), "8bit")
        assert answered(inc) and int(c[0]) == k and np.array_equal(r[0][:k], er) and np.array_equal(d[0][:k].view(np.uint32), ed.view(np.uint32)), name
    idx.close()


def test_waves_walk_and_skip_several_tiles():
    """200 000 x 64 (3 125 tiles: a wave owns two).  A random set of 8 000 rows: every tile holds a candidate, nothing is skipped; 125 whole
    tiles, one in 25 (8 000 rows): waves skip most of their tiles.  Both have fewer candidates than the list's capacity and more than k:
    answered, and the survivor count is the CPU model's over live & set (tests/_wide.py).  Every other row (100 000 candidates): handed back
    exactly where the model hands back — the 8-bit stage to the bfloat16 stage, that one to the exact path — and the model's count where not."""
    from quiver_amd.device_index import device_info
    from tests import _wide as Wd
    dim, n = 64, 200_000
    idx = make("cosine", dim); idx.add_synthetic(9200, 0, n)
    corpus = O.gen_rows(9200, 0, n, dim)
    q = O.gen_rows(9201, 0, 1, dim)[0]
    n_tiles = (n + 63) // 64
    grid = Wd.plan(n_tiles, device_info(0)["cus"])[0]
    stages = {plane: Wd.stage_of(0, plane, corpus, q) for plane in ARMS}
    rng = np.random.default_rng(92)
    rand = np.zeros(n, bool); rand[rng.permutation(n)[:8000]] = True
    stripes = (np.arange(n) // 64) % 25 == 0
    assert int(stripes.sum()) == 8000 and len(np.unique(np.flatnonzero(rand) // 64)) > 2800
    every_other = np.arange(n) % 2 == 0
    for name, m in (("rand", rand), ("stripes", stripes), ("every_other", every_other)):
        rs = idx.rowset(m)
        for k in (65, 500, 1024):
            call = lambda: idx.search_rowsets(q, k, rs)                  # noqa: E731
            exact = exact_of(idx, call)
            assert int(exact[2][0]) == k
            model = {plane: Wd.decide_wide(stages[plane], k, m, n_tiles, grid) for plane in ARMS}
            for plane in ARMS:
                _, inc = both(idx, call, plane, exact)
                assert inc["took"] == 1, (name, k, plane, inc)
                # the 8-bit stage hands on to the bfloat16 stage; the search counts as handed back when that one hands on too
                chain = [model["8bit"], model["bf16"]] if plane == "8bit" else [model["bf16"]]
                answers = next((s for s in chain if not s["hand_back"]), None)
                print("%s k %d %s: survivors %d, the model %s" % (name, k, plane, inc["cand"], answers["count"] if answers else "hands back"))
                if name != "every_other":
                    assert not chain[0]["hand_back"], (name, k, plane)
                assert inc["back"] == (answers is None), (name, k, plane, inc)
                if answers is not None:
                    assert inc["cand"] == answers["count"] and k <= inc["cand"] <= min(CAP, int(m.sum())), (name, k, plane, inc, answers["count"])
        rs.close()
    idx.close()


def test_one_candidate_more_than_results_and_no_more():
    """k + 1, k and k - 1 LIVE candidates at k = 100 (the set also names tombstoned rows): taken and answered; not taken, count k; not taken,
    count k - 1 and the padding as it is today"""
    dim, n, k = 16, 2000, 100
    idx = make("cosine", dim); idx.add_synthetic(9300, 0, n)
    q = O.gen_rows(9301, 0, 1, dim)[0]
    rng = np.random.default_rng(93)
    perm = rng.permutation(n)
    gone = perm[:40].astype(np.uint32)
    idx.remove(gone)
    for live, took in ((k + 1, 1), (k, 0), (k - 1, 0)):
        m = np.zeros(n, bool); m[perm[40:40 + live]] = True; m[gone[:7]] = True      # seven dead rows in the set
        rs = idx.rowset(m)
        for call in (lambda: idx.search_rowsets(q, k, rs), lambda: idx.search_masked(q, k, m)):
            for plane in ARMS:
                (r, d, c), inc = both(idx, call, plane)
                assert int(c[0]) == min(k, live) and inc["took"] == took and inc["back"] == 0, (live, plane, inc, c)
                assert not np.isin(r[0][:int(c[0])], gone).any()
                if live < k:
                    assert (r[0][live:k] == 0xFFFFFFFF).all() and np.isinf(d[0][live:k]).all()
        rs.close()
    idx.close()


def test_tombstones_and_scattered_updates_inside_the_set():
    dim, n = 80, 12_001
    rows = O.gen_rows(9400, 0, n, dim)
    q = O.gen_rows(9401, 0, 1, dim)[0]
    idx = make("cosine", dim); idx.add(rows)
    rng = np.random.default_rng(94)
    m = rng.random(n) < 0.6
    top, _ = O.exact_search(0, rows, q, 300, alive=m)
    gone = np.unique(np.concatenate([top[::3], rng.permutation(n)[:2000]]))[:2000].astype(np.uint32)   # some removed rows are in the set
    idx.remove(gone)
    alive = np.ones(n, bool); alive[gone] = False
    upd = rng.permutation(np.flatnonzero(alive & m))[:300].astype(np.uint32)
    vecs = O.gen_rows(9402, 0, 300, dim)
    vecs[:20] = (q[None, :] + np.float32(0.1) * vecs[:20]).astype(np.float32)   # some updated rows belong in the answer
    idx.update_rows(upd, vecs)
    rows2 = rows.copy(); rows2[upd] = vecs
    rs = idx.rowset(m)
    for k in (65, 300, 1024):
        er, ed = O.exact_search(0, rows2, q, k, alive=alive & m)
        assert np.isin(upd[:20], er).any()
        for plane in ARMS:
            (r, d, c), inc = both(idx, lambda: idx.search_rowsets(q, k, rs), plane)
            assert answered(inc), (k, plane, inc)
            assert np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32)), (k, plane)
    rs.close(); idx.close()


def _handed_back(idx, q, k, rs):
    for plane in ARMS:
        _, inc = both(idx, lambda: idx.search_rowsets(q, k, rs), plane)
        assert inc["took"] == 1 and inc["back"] == 1, (plane, inc)
    # the control words are back in their initial state: an ordinary filtered query behind it is answered by the wide form
    q2 = O.gen_rows(9599, 0, 1, idx.dim)[0]
    return both(idx, lambda: idx.search_rowsets(q2, k, rs), "8bit")[1]


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
def test_queries_the_bound_declines_are_handed_back(metric):
    """a zero query and a query of 1e30 elements under a filter: bound_scan_norm_ok declines |q|, both stages hand on, the key-per-row path
    over the candidate bitmap answers — what the filtered call returns today"""
    dim, n, k = 80, 6001, 100
    idx = make(metric, dim); idx.add_synthetic(9500, 0, n)
    m = np.random.default_rng(95).random(n) < 0.5
    rs = idx.rowset(m)
    assert answered(_handed_back(idx, np.zeros(dim, np.float32), k, rs))
    assert answered(_handed_back(idx, np.full(dim, 1e30, np.float32), k, rs))
    rs.close(); idx.close()


def test_fewer_candidates_the_bound_is_sure_of_than_results():
    """the set holds 70 rows without a NaN element and 500 with one, at k = 100: no finite H in either stage"""
    dim, n, k = 16, 2000, 100
    rows = O.gen_rows(9600, 0, n, dim)
    perm = np.random.default_rng(96).permutation(n)
    sure, in_set = perm[:70], perm[:570]
    bad = np.ones(n, bool); bad[sure] = False
    rows[bad, 3] = np.nan
    q = O.gen_rows(9601, 0, 1, dim)[0]
    idx = make("cosine", dim); idx.add(rows)
    m = np.zeros(n, bool); m[in_set] = True
    rs = idx.rowset(m)
    for plane in ARMS:
        (r, d, c), inc = both(idx, lambda: idx.search_rowsets(q, k, rs), plane)
        assert inc["took"] == 1 and inc["back"] == 1, (plane, inc)
        assert sorted(r[0][:70].tolist()) == sorted(sure.tolist())       # the 70 finite distances first
        assert np.isin(r[0], in_set).all()
    # the control words are back in their initial state: the 70 finite rows as a set, k = 65, on the same index — answered by the wide form
    m2 = np.zeros(n, bool); m2[sure] = True
    rs2 = idx.rowset(m2)
    (r, d, c), inc = both(idx, lambda: idx.search_rowsets(q, 65, rs2), "8bit")
    assert answered(inc) and int(c[0]) == 65 and np.isin(r[0], sure).all(), inc
    rs.close(); rs2.close(); idx.close()


@pytest.mark.parametrize("k", [65, 129])
def test_ties_across_the_kth_place(k):
    """exact duplicates of one row in three different tiles, all in the set, take ranks k - 1, k and k + 1 among the set's rows: the two with
    the smaller row numbers are in the answer, in (distance, row) order"""
    dim, n = 80, 6001
    rows = O.gen_rows(9700, 0, n, dim)
    q = O.gen_rows(9701, 0, 1, dim)[0]
    m = np.random.default_rng(97).random(n) < 0.5
    order, _ = O.exact_search(0, rows, q, int(m.sum()), alive=m)
    src = int(order[k - 2])                                              # rank k - 1 (1-based) among the set
    far = [int(r) for r in order[::-1] if int(r) // 64 != src // 64][:400]
    a = far[0]
    b = next(r for r in far if r // 64 != a // 64)
    rows[a] = rows[src]; rows[b] = rows[src]
    er, ed = O.exact_search(0, rows, q, k, alive=m)
    trio = sorted([src, a, b])
    assert er[k - 2] == trio[0] and er[k - 1] == trio[1] and trio[2] not in er.tolist()   # the shape is what it is built to be
    idx = make("cosine", dim); idx.add(rows)
    rs = idx.rowset(m)
    for plane in ARMS:
        (r, d, c), inc = both(idx, lambda: idx.search_rowsets(q, k, rs), plane)
        assert answered(inc), inc
        assert np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32)), (plane, r[0][-4:], er[-4:])
    rs.close(); idx.close()


def test_every_host_entry_point():
    dim, n, k = 80, 6001, 100
    idx = make("cosine", dim); idx.add_synthetic(9800, 0, n)
    qs = O.gen_rows(9801, 0, 4, dim)
    rng = np.random.default_rng(98)
    masks = [rng.random(n) < f for f in (0.5, 0.3, 0.7, 0.9)]
    sets = [idx.rowset(m) for m in masks]
    vals = rng.random(n)
    col = idx.column("f64"); col.set(0, vals)
    for plane in ARMS:
        _, inc = both(idx, lambda: idx.search_masked(qs[0], k, masks[0]), plane)
        assert answered(inc), (plane, inc)
        # four queries naming four distinct sets: four single-query pieces
        (r, d, c), inc = both(idx, lambda: idx.search_rowsets(qs, k, sets), plane)
        assert inc["took"] == 4 and inc["back"] == 0, (plane, inc)
        for j in range(4):                                               # ... each what its own call returns
            rj = exact_of(idx, lambda: idx.search_rowsets(qs[j], k, sets[j]))
            assert np.array_equal(r[j], rj[0][0]) and X.same(d[j], rj[1][0])
        # two queries naming one set keep their shared key-per-row pass
        _, inc = both(idx, lambda: idx.search_rowsets(qs[:2], k, [sets[1], sets[1]]), plane)
        assert inc["took"] == 0 and inc["back"] == 0, (plane, inc)
        # one F64 range on a facet column: the filter becomes a counted set inside the call
        spec = [(col, "ge", 0.25), (col, "lt", 0.75)]
        (r, d, c), inc = both(idx, lambda: idx.search_where(qs[3], k, spec), plane)
        assert answered(inc), (plane, inc)
        in_range = (vals >= 0.25) & (vals < 0.75)
        assert int(c[0]) == k and in_range[r[0]].all()
    for s in sets:
        s.close()
    col.close(); idx.close()


def test_device_pointers_on_a_busy_stream_reuse_the_workspace():
    """k = 1024, then 65, then 300 over a row set on one non-default stream without a synchronise between them, an unfiltered wide search
    interleaved: one workspace and one set of control words serve them all"""
    import torch
    dim, n = 64, 50_000
    idx = make("cosine", dim); idx.add_synthetic(9900, 0, n)
    q = O.gen_rows(9901, 0, 1, dim)[0]
    m = np.random.default_rng(99).random(n) < 0.4
    rs = idx.rowset(m)
    ks = (1024, 65, 300)
    exact = {k: exact_of(idx, lambda: idx.search_rowsets(q, k, rs)) for k in ks}
    idx.set_bound_scan_wide("never")
    plain = idx.search(q, 200)
    dq = torch.from_numpy(q).cuda()
    st = torch.cuda.Stream()
    for plane in ARMS:
        idx.set_bound_scan_wide_filtered("always"); idx.set_bound_plane_filtered(plane)
        idx.set_bound_scan_wide("always"); idx.set_bound_plane(plane)
        s0 = stats(idx)
        outs = {k: (torch.zeros(k, dtype=torch.int32, device="cuda"), torch.zeros(k, dtype=torch.float32, device="cuda")) for k in ks}
        pr, pd = torch.zeros(200, dtype=torch.int32, device="cuda"), torch.zeros(200, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for i, k in enumerate(ks):
            idx.search_rowsets_device(dq.data_ptr(), 1, k, rs, outs[k][0].data_ptr(), outs[k][1].data_ptr(), st.cuda_stream)
            if i == 0:
                idx.search_device(dq.data_ptr(), 1, 200, pr.data_ptr(), pd.data_ptr(), st.cuda_stream)
        st.synchronize()
        s1 = stats(idx)
        assert s1["searches"] - s0["searches"] == 4 and s1["hand_backs"] == s0["hand_backs"], (plane, s0, s1)
        for k in ks:
            r = outs[k][0].cpu().numpy().view(np.uint32); d = outs[k][1].cpu().numpy()
            assert np.array_equal(r, exact[k][0][0]) and np.array_equal(d.view(np.uint32), exact[k][1][0].view(np.uint32)), (plane, k)
        assert np.array_equal(pr.cpu().numpy().view(np.uint32), plain[0][0]) and np.array_equal(pd.cpu().numpy().view(np.uint32), plain[1][0].view(np.uint32))
    idx.set_bound_scan_wide("auto"); idx.set_bound_plane("auto")
    rs.close(); idx.close()


def test_four_threads_search_one_index():
    dim, n, k = 80, 20_000, 100
    idx = make("cosine", dim); idx.add_synthetic(10100, 0, n)
    qs = O.gen_rows(10101, 0, 4, dim)
    rng = np.random.default_rng(101)
    sets = [idx.rowset(rng.random(n) < 0.5) for _ in range(4)]
    exact = [exact_of(idx, lambda: idx.search_rowsets(qs[i], k, sets[i])) for i in range(4)]
    idx.set_bound_scan_wide_filtered("always"); idx.set_bound_plane_filtered("8bit")
    s0 = stats(idx)
    got, errs = [None] * 4, []

    def work(i):
        try:
            for _ in range(3):
                got[i] = idx.search_rowsets(qs[i], k, sets[i])
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    s1 = stats(idx)
    assert s1["searches"] - s0["searches"] == 12 and s1["hand_backs"] == s0["hand_backs"], (s0, s1)
    for i in range(4):
        assert same_result(got[i], exact[i]), i
    for s in sets:
        s.close()
    idx.close()


def test_the_knob_is_its_own():
    dim, n, k = 80, 6001, 100
    idx = make("cosine", dim); idx.add_synthetic(10300, 0, n)
    q = O.gen_rows(10301, 0, 1, dim)[0]
    m = np.ones(n, bool); m[::7] = False
    rs = idx.rowset(m)
    filtered = (lambda kk=k: idx.search_masked(q, kk, m)), (lambda kk=k: idx.search_rowsets(q, kk, rs))
    # nothing set: automatic has no measured cell, so a filtered search takes nothing
    for call in filtered:
        call()
    assert stats(idx)["searches"] == 0
    # the unfiltered form's knob alone leaves filtered calls on their path
    idx.set_bound_scan_wide("always"); idx.set_bound_plane("8bit"); idx.set_bound_plane_filtered("8bit")
    s0 = stats(idx)
    for call in filtered:
        call()
    assert stats(idx) == s0
    idx.set_bound_scan_wide("auto"); idx.set_bound_plane("auto")
    # the filtered knob alone: an unfiltered call does not move the counters; the k <= 64 counters do not move for filtered wide searches
    before = (idx.bound_scan_stats(), idx.bound_scan8_stats(), idx.bound_scan6_stats())
    idx.set_bound_scan_wide_filtered("always")
    s0 = stats(idx)
    idx.search(q, k)
    idx.search_rowsets(q, k, None)                                       # no set: an unfiltered call through the row-set entry point
    assert stats(idx)["searches"] == s0["searches"]
    for plane in ARMS:
        for call in filtered:
            _, inc = both(idx, call, plane)
            assert answered(inc), (plane, inc)
    assert (idx.bound_scan_stats(), idx.bound_scan8_stats(), idx.bound_scan6_stats()) == before
    # k = 1025 and k = 64 keep their paths
    for kk in (1025, 64):
        for call in filtered:
            _, inc = both(idx, lambda: call(kk), "8bit")
            assert inc["took"] == 0 and inc["back"] == 0, (kk, inc)
    rs.close(); idx.close()
