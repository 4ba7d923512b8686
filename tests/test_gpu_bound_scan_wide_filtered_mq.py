"""The wide form of a FILTERED shared bound pass: one call of 2 to 8 queries at 65 <= k <= 1024, each over its own live & set
(k_bound_scan_mq / k_bound_scan8_mq<., ., true, true>, the wide shared pass's funnel per query, the set-carrying key-per-row redo;
quiver_amd/csrc/qv_bound_scan.hip, qv_scan.hip, qv_rank.hip).  Every case sets the form's own knob to "always" and names a plane, asserts from
the wide shared pass's counters that the form answered, and compares rows, float32 bits and counts for equality with the float64 CPU
oracle over live & set_j — or, where a NaN leaves the oracle's order undefined, with the same call under "never"."""
import numpy as np
import pytest

import quiver_amd
from quiver_amd import _lib
from tests import _extremes as X
from tests import _oracle as O

pytestmark = pytest.mark.gpu

CAP = _lib.QV_BOUND_WIDE_CAND_CAP
ARMS = ("bf16", "8bit")
NQS = (2, 3, 4, 5, 8)


def make(metric, dim):
    return quiver_amd.DeviceIndex(dim, metric, l2_scan_plane=(metric == "l2"))


def masks_of(n, seed):
    """null; a random half; even tiles; odd tiles; everything but tile 0 — the last three cleared in one band of consecutive tiles"""
    tile = np.arange(n) // 64
    n_tiles = (n + 63) // 64
    band = (tile >= n_tiles // 3) & (tile < n_tiles // 3 + max(4, n_tiles // 8))
    return [None, np.random.default_rng(seed).random(n) < 0.5, (tile % 2 == 0) & ~band, (tile % 2 == 1) & ~band, (tile != 0) & ~band]


def run(idx, call, plane, mode="always"):
    """-> (rows, dist, count), queries that took the form, queries handed back"""
    idx.set_bound_scan_wide_filtered_mq(mode); idx.set_bound_plane_filtered_mq(plane)
    s0 = idx.bound_scan_wide_mq_stats()
    res = call()
    s1 = idx.bound_scan_wide_mq_stats()
    return res, s1["searches"] - s0["searches"], s1["hand_backs"] - s0["hand_backs"]


def is_oracle(mid, corpus, q, k, alive, r, d, c):
    er, ed = O.exact_search(mid, corpus, q, k, alive=alive)
    m = len(er)
    return int(c) == m and np.array_equal(r[:m], er) and np.array_equal(d[:m].view(np.uint32), ed.view(np.uint32)) and (r[m:] == 0xFFFFFFFF).all()


def same(a, b):
    return bool(np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]) and X.same(a[1], b[1]))


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
@pytest.mark.parametrize("n,dim", [(6001, 80), (2000, 16), (200_000, 64)])
def test_rows_and_bits(metric, n, dim):
    """a ragged last tile and a 4 + 1 step split; the narrowest row; 3 125 tiles, so waves walk several tiles with the set-word prefetch
    and the 8-bit pre-test at work.  Query j of a pass of nq takes set (j + nq) mod 5: two queries are the even and the odd tiles (a tile
    read for one is dead for the other, the band is read by nobody), three add the set without tile 0.  Stale workspace: every
    filtered call follows an UNFILTERED wide shared pass on the same index, which leaves finite lower bounds in every word it skips."""
    idx = make(metric, dim); idx.add_synthetic(7300 + dim, 0, n)
    corpus = O.gen_rows(7300 + dim, 0, n, dim)
    qs = O.gen_rows(7301 + dim, 0, 8, dim)
    mid = quiver_amd.metric_id(metric)
    masks = masks_of(n, dim)
    sets = [None if m is None else idx.rowset(m) for m in masks]
    live = np.ones(n, bool)
    fewest = min(int(m.sum()) for m in masks if m is not None)
    for nq in NQS:
        pick = [(j + nq) % 5 for j in range(nq)]
        for k in (65, 129, min(1024, fewest - 1)):
            assert all(int((live if masks[s] is None else masks[s]).sum()) > k for s in pick)
            call = lambda: idx.search_rowsets(qs[:nq], k, [sets[s] for s in pick])    # noqa: E731
            never, took, _ = run(idx, call, "bf16", "never")
            assert took == 0
            for plane in ARMS:
                idx.set_bound_scan_wide_mq("always"); idx.set_bound_plane_mq(plane)
                idx.search(qs[:nq], k)
                got, took, back = run(idx, call, plane)
                assert (took, back) == (nq, 0), (nq, k, plane, took, back)
                for j in range(nq if n < 100_000 else 2):
                    assert is_oracle(mid, corpus, qs[j], k, live if masks[pick[j]] is None else masks[pick[j]], got[0][j], got[1][j], got[2][j]), (nq, k, plane, j)
                assert same(got, never), (nq, k, plane)
    idx.close()


def test_dead_rows_and_a_set_that_drops_out():
    """a removed tile, scattered tombstones and overwritten rows inside the sets; the middle query's set keeps at most k live rows: it
    leaves the run, gets its clamped count, and the two pieces around it are answered by the form at their own offsets"""
    n, dim, k = 6001, 80, 100
    corpus = O.gen_rows(7400, 0, n, dim).copy()
    idx = make("cosine", dim); idx.add(corpus)
    rng = np.random.default_rng(74)
    dead = np.unique(np.concatenate([np.arange(320, 384), rng.choice(n, 300, replace=False)]))
    idx.remove(dead)
    live = np.ones(n, bool); live[dead] = False
    moved = rng.choice(np.flatnonzero(live), 40, replace=False).astype(np.uint32)
    corpus[moved] = O.gen_rows(7401, 0, 40, dim)
    idx.update_rows(moved, corpus[moved])
    masks = masks_of(n, 74)
    tiny = np.zeros(n, bool); tiny[:90] = True
    masks = [masks[1], masks[2], tiny, masks[3], None]
    assert int((tiny & live).sum()) <= k
    sets = [None if m is None else idx.rowset(m) for m in masks]
    qs = O.gen_rows(7402, 0, 5, dim)
    for plane in ARMS:
        got, took, back = run(idx, lambda: idx.search_rowsets(qs, k, sets), plane)
        assert (took, back) == (4, 0), (plane, took, back)
        for j in range(5):
            assert is_oracle(0, corpus, qs[j], k, live if masks[j] is None else live & masks[j], got[0][j], got[1][j], got[2][j]), (plane, j)
        assert int(got[2][2]) == int((tiny & live).sum())
    idx.close()


@pytest.mark.parametrize("nq", [2, 8])
@pytest.mark.parametrize("plane", ARMS)
def test_hand_back_redone_over_its_own_set(plane, nq):
    """9 000 near-duplicates of query 0 pass every threshold its bound can set: more survivors than the list holds.  Its set keeps them
    but not its 100 nearest rows, so a redo over v.alive would return exactly the rows the set excludes."""
    n, dim, k = 20_000, 64, 100
    rng = np.random.default_rng(75)
    qs = rng.standard_normal((nq, dim)).astype(np.float32)
    corpus = rng.standard_normal((n, dim)).astype(np.float32)
    assert CAP < 9000
    corpus[:9000] = (qs[0][None, :] + np.float32(1e-3) * corpus[:9000]).astype(np.float32)
    idx = make("cosine", dim); idx.add(corpus)
    own = np.ones(n, bool); own[O.exact_search(0, corpus, qs[0], 100)[0]] = False
    masks = [own] + [None if j % 2 else (np.arange(n) % 3 != 0) for j in range(1, nq)]
    sets = [None if m is None else idx.rowset(m) for m in masks]
    got, took, back = run(idx, lambda: idx.search_rowsets(qs, k, sets), plane)
    assert (took, back) == (nq, 1), (took, back)
    for j in range(nq):
        assert is_oracle(0, corpus, qs[j], k, masks[j], got[0][j], got[1][j], got[2][j]), j
    assert own[got[0][0]].all()
    idx.close()


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
def test_nan_and_zero_queries_are_handed_back_alone(metric):
    n, dim, k = 6001, 80, 129
    idx = make(metric, dim); idx.add_synthetic(7600, 0, n)
    qs = O.gen_rows(7601, 0, 4, dim)
    qs[1, 7] = np.nan; qs[2] = 0
    masks = masks_of(n, 76)[1:]
    sets = [idx.rowset(m) for m in masks]
    call = lambda: idx.search_rowsets(qs, k, sets)                         # noqa: E731
    never, _, _ = run(idx, call, "bf16", "never")
    for plane in ARMS:
        got, took, back = run(idx, call, plane)
        assert (took, back) == (4, 2), (plane, took, back)
        assert same(got, never), plane
    idx.close()


@pytest.mark.parametrize("entry", ["rowsets", "masked", "where", "device"])
def test_entry_points(entry):
    import torch
    n, dim, nq, k = 6001, 80, 3, 129
    idx = make("cosine", dim); idx.add_synthetic(7700, 0, n)
    corpus = O.gen_rows(7700, 0, n, dim)
    qs = O.gen_rows(7701, 0, nq, dim)
    vals = np.random.default_rng(77).random(n)
    col = idx.column("f64"); col.set(0, vals)
    lo = (0.0, 0.25, 0.5)
    masks = [(vals >= a) & (vals < a + 0.5) for a in lo]
    if entry == "masked":
        masks = [masks[0]] * nq
    sets = [idx.rowset(m) for m in masks]
    calls = 1
    for plane in ARMS:
        if entry == "rowsets":
            call = lambda: idx.search_rowsets(qs, k, sets)                 # noqa: E731
        elif entry == "masked":
            call = lambda: idx.search_masked(qs, k, masks[0])              # noqa: E731
        elif entry == "where":
            call = lambda: idx.search_where(qs, k, [[(col, "ge", a), (col, "lt", a + 0.5)] for a in lo])    # noqa: E731
        else:                                                              # twice on one stream, no synchronise between
            dq = torch.from_numpy(qs).cuda()
            out = [(torch.zeros((nq, k), dtype=torch.int32, device="cuda"), torch.zeros((nq, k), dtype=torch.float32, device="cuda")) for _ in range(2)]
            st = torch.cuda.Stream(); torch.cuda.synchronize()
            calls = 2

            def call():
                for r, d in out:
                    idx.search_rowsets_device(dq.data_ptr(), nq, k, sets, r.data_ptr(), d.data_ptr(), st.cuda_stream)
                st.synchronize()
                assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32))
                return out[1][0].cpu().numpy().view(np.uint32), out[1][1].cpu().numpy(), np.full(nq, k)
        got, took, back = run(idx, call, plane)
        assert (took, back) == (calls * nq, 0), (entry, plane, took, back)
        for j in range(nq):
            assert is_oracle(0, corpus, qs[j], k, masks[j], got[0][j], got[1][j], got[2][j]), (entry, plane, j)
    idx.close()


def test_knobs():
    """nothing set, and "never": no wide counter moves; the three other wide knobs at "always" do not reach the form"""
    n, dim, nq, k = 6001, 80, 3, 129
    idx = make("cosine", dim); idx.add_synthetic(7800, 0, n)
    qs = O.gen_rows(7801, 0, nq, dim)
    masks = masks_of(n, 78)[1:4]
    sets = [idx.rowset(m) for m in masks]
    calls = [lambda: idx.search_rowsets(qs, k, sets), lambda: idx.search_rowsets(qs, k, sets[0]), lambda: idx.search_masked(qs, k, masks[0])]
    wide = lambda: (idx.bound_scan_wide_mq_stats()["searches"], idx.bound_scan_wide_stats()["searches"])    # noqa: E731
    w0 = wide()
    unset = [c() for c in calls]
    assert wide() == w0
    for c, want in zip(calls, unset):
        got, took, _ = run(idx, c, "bf16", "never")
        assert took == 0 and same(got, want)
    assert wide() == w0
    idx.set_bound_scan_wide("always"); idx.set_bound_scan_wide_filtered("always"); idx.set_bound_scan_wide_mq("always")
    for c, want in zip(calls, unset):
        got, took, _ = run(idx, c, "bf16", "never")
        assert took == 0 and same(got, want)
    for c, want in zip(calls, unset):                                      # ... and this one at "always" returns the same
        got, took, back = run(idx, c, "8bit")
        assert (took, back) == (nq, 0) and same(got, want)
    idx.close()
