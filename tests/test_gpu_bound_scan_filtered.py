"""The bound scan under filters (k_bound_scan<., true>, k_bound_scan_mq<., ., true>, k_flat_scan_redo<., ., true>; quiver_amd/csrc/qv_bound_scan.hip, the redo in qv_scan.hip):
filtered searches of 1 to 8 queries read the bfloat16 copy, each query restricted to its own candidates live & set.  Every call runs under
"always" and again under "never" (today's exact filtered scan: k_rowset_scan_mq, k_flat_scan over the candidate bitmap) and must give the
same rows, counts and float32 bits; the statistics say which path answered — `searches` rises by the number of queries, `hand_backs` by
the number tests/test_bound_scan_filtered_cpu.py derives on the CPU for these very inputs (tests/_bound_filtered.py), stated here as
literals.  One query per case is compared with the CPU oracle over live & set."""
import threading

import numpy as np
import pytest

import quiver_amd
from quiver_amd.device_index import device_info
from tests import _bound as B
from tests import _bound_filtered as F
from tests import _extremes as X
from tests import _oracle as O

pytestmark = pytest.mark.gpu

NAME = {B.COSINE: "cosine", B.DOT: "dot"}


def both(idx, call):
    """(result under "always", queries that took the bound scan, of which handed back) for ONE call; the same call under "never" must give
    the same rows, counts and bits and count nothing"""
    idx.set_bound_scan("always")
    s0 = idx.bound_scan_stats()
    r, d, c = call()
    s1 = idx.bound_scan_stats()
    idx.set_bound_scan("never")
    er, ed, ec = call()
    s2 = idx.bound_scan_stats()
    assert s2["searches"] == s1["searches"]                               # "never" is never
    assert np.array_equal(c, ec) and np.array_equal(r, er), (r, er)
    assert X.same(d, ed), (d, ed)
    return (r, d, c), s1["searches"] - s0["searches"], s1["hand_backs"] - s0["hand_backs"]


def build(case, metric, dim=None):
    idx = quiver_amd.DeviceIndex(case["rows"].shape[1], NAME[metric])
    idx.add(case["rows"])
    if "dead" in case:
        idx.remove(case["dead"])
    assert idx.bound_scan_stats()["plane"]
    return idx


def sets_of(idx, masks):
    return [None if m is None else idx.rowset(m) for m in masks]


def agrees(metric, rows, q, k, alive, r, d, c):
    er, ed = O.exact_search(metric, rows, q, k, alive=alive.astype(np.uint8))
    w = len(er)
    return int(c) == w and r[:w].tolist() == er.tolist() and d[:w].tobytes() == ed.tobytes() and (r[w:] == 0xFFFFFFFF).all() and np.isposinf(d[w:]).all()


# ---- 1. basic shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
@pytest.mark.parametrize("dim", [16, 48, 128, 768])
def test_rows_and_bits_of_the_exact_filtered_scan(metric, dim):
    case = F.basic(metric, dim)
    idx = build(case, metric)
    sets = sets_of(idx, case["masks"])
    for i, nq in enumerate(F.NQS):
        for k in F.KS:
            (r, d, c), took, back = both(idx, lambda: idx.search_rowsets(case["qs"][:nq], k, sets[:nq]))
            assert took == nq and back == 0, (nq, k, took, back)         # every set holds 64 live rows or more: the CPU file derives 0
            if k == F.KS[i % 4]:
                j = nq - 1
                assert agrees(metric, case["rows"], case["qs"][j], k, F.alive_of(case["live"], case["masks"][j]), r[j], d[j], c[j]), (nq, k)
    # a single query under each kind of set (the skipping single-query form); slot 2 has no set: an unfiltered search
    for j in (0, 1, 3, 4, 7):
        (r, d, c), took, back = both(idx, lambda: idx.search_rowsets(case["qs"][j:j + 1], 10, sets[j:j + 1]))
        assert took == 1 and back == 0, (j, took, back)
        assert agrees(metric, case["rows"], case["qs"][j], 10, F.alive_of(case["live"], case["masks"][j]), r[0], d[0], c[0]), j
    idx.close()


# ---- 2. sets with fewer than k candidates ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
def test_sets_with_fewer_than_k_candidates_are_handed_back_alone(metric):
    case = F.short(metric)
    idx = build(case, metric)
    sets = sets_of(idx, case["masks"])
    k = 10
    (r, d, c), took, back = both(idx, lambda: idx.search_rowsets(case["qs"], k, sets))
    assert took == 4 and back == 2, (took, back)                          # the empty set and the set of 5 have no H
    assert c.tolist() == [k, 0, k, 5]
    for j in range(4):
        assert agrees(metric, case["rows"], case["qs"][j], k, case["live"] & case["masks"][j], r[j], d[j], c[j]), j
    for j, n_res in ((1, 0), (3, 5)):                                     # the same two as single-query calls
        (r, d, c), took, back = both(idx, lambda: idx.search_rowsets(case["qs"][j:j + 1], k, sets[j:j + 1]))
        assert took == 1 and back == 1 and int(c[0]) == n_res, (j, took, back, c)
        assert agrees(metric, case["rows"], case["qs"][j], k, case["live"] & case["masks"][j], r[0], d[0], c[0]), j
    (_, _, _), took, back = both(idx, lambda: idx.search_rowsets(case["qs"], k, [sets[0], sets[2], sets[0], sets[2]]))   # the words are back in their initial state
    assert took == 4 and back == 0, (took, back)
    idx.close()


# ---- 3. stale lower bounds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 4])
def test_a_skipped_tile_holds_no_earlier_searchs_bounds(nq):
    metric = B.COSINE
    case = F.stale(metric)
    idx = build(case, metric)
    sets = sets_of(idx, case["masks"])
    k = 10
    idx.set_bound_scan("always")
    s0 = idx.bound_scan_stats()
    r0, _, _ = idx.search_rowsets(case["qs"][:nq], k, [None] * nq)        # unfiltered, same entry, same context: the answers lie in tiles t % 3 != 0
    assert idx.bound_scan_stats()["searches"] - s0["searches"] == nq
    assert r0[:, 0].tolist() == case["at"][:nq].tolist() and ((r0 // 64) % 3 != 0).any()
    (r, d, c), took, back = both(idx, lambda: idx.search_rowsets(case["qs"][:nq], k, sets[:nq]))
    assert took == nq and back == 0, (took, back)
    for j in range(nq):
        assert ((r[j] // 64) % 3 == 0).all()
        assert agrees(metric, case["rows"], case["qs"][j], k, case["masks"][j], r[j], d[j], c[j]), j
    idx.close()


# ---- 4. the first tile a wave reads is not the first it owns -----------------------------------------------------------------------------
def test_the_query_norm_rides_along_the_first_tile_read():
    metric = B.COSINE
    cus = device_info(0)["cus"]
    case = F.second_tile(metric, cus)
    idx = build(case, metric)
    sets = sets_of(idx, case["masks"])
    k = 10
    for nq in (1, 4, 8):
        (r, d, c), took, back = both(idx, lambda: idx.search_rowsets(case["qs"][:nq], k, sets[:nq]))
        assert took == nq and back == 0, (nq, took, back)
        j = nq - 1
        assert (r[j] // 64 >= 8 * cus).all()
        assert agrees(metric, case["rows"], case["qs"][j], k, case["masks"][j], r[j], d[j], c[j]), nq
    idx.close()


# ---- 5. a set shorter than the index -----------------------------------------------------------------------------------------------------
def test_a_set_made_before_the_index_grew():
    metric, dim, n0, n1, k = B.COSINE, 128, 12_000, 20_011, 10
    rows = O.gen_rows(6500, 0, n1, dim).copy()
    qs = O.gen_rows(6501, 0, 4, dim)
    rng = np.random.default_rng(6502)
    idx = quiver_amd.DeviceIndex(dim, "cosine"); idx.add(rows[:n0])
    masks = [np.zeros(n1, bool) for _ in range(4)]
    for j in range(4):
        masks[j][:n0] = rng.random(n0) < (0.5, 0.1, 0.5, 0.02)[j]
    sets = [idx.rowset(m[:n0]) for m in masks]
    idx.add(rows[n0:])                                                    # the sets' words < n_tiles: new rows are unselected
    live = np.ones(n1, bool)

    def check(where):
        for nq in (1, 4):
            (r, d, c), took, back = both(idx, lambda: idx.search_rowsets(qs[:nq], k, sets[:nq]))
            assert took == nq and back == 0, (where, nq, took, back)
            for j in range(nq):
                assert agrees(metric, rows, qs[j], k, live & masks[j], r[j], d[j], c[j]), (where, nq, j)

    check("grown")
    new = np.arange(n0 + 7, n1, 3, dtype=np.uint32)
    sets[0].set_rows(new, True); masks[0][new] = True
    sets[3].set_rows(new[:500], True); masks[3][new[:500]] = True
    check("set_rows")
    gone = np.flatnonzero(masks[0])[:400].astype(np.uint32)
    idx.remove(gone); live[gone] = False
    at = int(np.flatnonzero(masks[1] & live)[5])
    rows[at] = qs[1] * np.float32(1.0 + 1e-6); idx.update(at, rows[at])  # a selected row becomes query 1's nearest
    check("remove and update")
    idx.close()


# ---- 6. search_masked --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
def test_search_masked_takes_the_bound_scan(metric):
    case = F.masked(metric)
    idx = build(case, metric)
    k = 10
    for m in case["masks"]:
        rs = idx.rowset(m)
        for nq in (1, 4, 8):
            (r, d, c), took, back = both(idx, lambda: idx.search_masked(case["qs"][:nq], k, m))
            assert took == nq and back == 0, (nq, took, back)
            er, ed, ec = idx.search_rowsets(case["qs"][:nq], k, rs)       # ("never" now) that mask as every query's set
            assert np.array_equal(r, er) and np.array_equal(c, ec) and X.same(d, ed)
            assert agrees(metric, case["rows"], case["qs"][nq - 1], k, case["live"] & m, r[nq - 1], d[nq - 1], c[nq - 1])
    idx.close()


# ---- 7. the tight corpus under a filter ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
@pytest.mark.parametrize("dim", F.TIGHT_DIMS)
@pytest.mark.parametrize("k", F.TIGHT_KS)
def test_the_planted_neighbour_under_its_own_set(metric, dim, k):
    """the set is exactly {r*, the k - 1 nearer rows, the competitor band}: H under the set is the best competitor's upper bound and r*'s
    lower bound is just inside it (tests/test_bound_scan_filtered_cpu.py establishes (a) - (d) over the set).  The planted query sits in an
    odd and in an even slot of a pass of four — the two halves of a packed fma — beside ordinary queries with other sets; then the set
    omits the best competitor and H is the next one's."""
    planted_neighbour_under_its_own_set(metric, dim, k)


@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
@pytest.mark.parametrize("dim,k", F.TIGHT_WIDE)
def test_the_planted_neighbour_under_its_own_set_at_wider_rows(metric, dim, k):
    planted_neighbour_under_its_own_set(metric, dim, k)


def planted_neighbour_under_its_own_set(metric, dim, k):
    t = F.tight(metric, dim, k)
    case = t["case"]
    idx = quiver_amd.DeviceIndex(dim, NAME[metric]); idx.add(case["rows"])
    for which in ("exact", "omit"):
        mask = t[which]
        er, ed = O.exact_search(metric, case["rows"], case["q"], k, alive=mask.astype(np.uint8))
        assert er[k - 1] == case["target"]
        for slot in (1, 2):
            qs, masks = F.tight_pass(t, slot, mask)
            sets = sets_of(idx, masks)
            (r, d, c), took, back = both(idx, lambda: idx.search_rowsets(qs, k, sets))
            assert took == 4 and back == 0, (which, slot, took, back)
            assert int(c[slot]) == k and r[slot].tolist() == er.tolist() and d[slot].tobytes() == ed.tobytes(), (which, slot, r[slot], er)
            assert r[slot][k - 1] == case["target"]
            j = (slot + 1) % 4
            assert agrees(metric, case["rows"], qs[j], k, masks[j], r[j], d[j], c[j]), (which, slot)
        (r, d, c), took, back = both(idx, lambda: idx.search_rowsets(np.asarray(case["q"])[None, :], k, [idx.rowset(mask)]))   # and alone: the single-query form
        assert took == 1 and back == 0 and r[0].tolist() == er.tolist() and d[0].tobytes() == ed.tobytes(), which
    idx.close()


# ---- 8. a hand-back inside a set -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
def test_a_query_handed_back_is_redone_over_its_own_set(metric):
    case = F.clusters(metric)
    idx = build(case, metric)
    sets = sets_of(idx, case["masks"])
    k = 10
    (r, d, c), took, back = both(idx, lambda: idx.search_rowsets(case["qs"], k, sets))
    assert took == 4 and back == 1, (took, back)                          # query 1: more than 4096 selected rows within the margin (the CPU file)
    for j in range(4):
        assert agrees(metric, case["rows"], case["qs"][j], k, case["masks"][j], r[j], d[j], c[j]), j
    assert case["masks"][1][r[1]].all()                                   # (the other half of the cluster is as near: a redo over `alive` alone returns it)
    idx.close()


# ---- 9. shared passes ------------------------------------------------------------------------------------------------------------------------
def test_concurrent_callers_with_their_own_sets_share_bound_passes():
    n, dim, k, callers, each = 60_000, 128, 10, 8, 12
    idx = quiver_amd.DeviceIndex(dim, "cosine"); idx.add_synthetic(6900, 0, n)
    rows = O.gen_rows(6900, 0, n, dim)
    qs = O.gen_rows(6901, 0, callers, dim)
    rng = np.random.default_rng(6902)
    masks = [rng.random(n) < (0.5, 0.2, 0.05, 1.0)[j % 4] for j in range(callers)]
    sets = sets_of(idx, masks)
    want = [O.exact_search(B.COSINE, rows, qs[j], k, alive=masks[j].astype(np.uint8)) for j in range(callers)]
    idx.set_bound_scan("always")
    s0 = idx.bound_scan_stats(); c0 = idx.rowset_coalesce_stats()
    bad = []
    start = threading.Barrier(callers)

    def caller(j):
        start.wait()
        for _ in range(each):
            r, d, c = idx.search_rowsets(qs[j:j + 1], k, sets[j:j + 1])
            if int(c[0]) != k or r[0].tolist() != want[j][0].tolist() or d[0].tobytes() != want[j][1].tobytes():
                bad.append(j)

    ts = [threading.Thread(target=caller, args=(j,)) for j in range(callers)]
    [t.start() for t in ts]; [t.join() for t in ts]
    s1 = idx.bound_scan_stats(); c1 = idx.rowset_coalesce_stats()
    assert not bad, bad
    assert c1["groups"] > c0["groups"] and c1["group_queries"] - c0["group_queries"] > c1["groups"] - c0["groups"]   # passes were shared
    assert s1["searches"] - s0["searches"] == callers * each, (s0, s1)
    assert s1["hand_backs"] == s0["hand_backs"]
    idx.close()


# ---- 10. the device form on a busy stream -----------------------------------------------------------------------------------------------------
def test_device_form_behind_queued_work():
    import torch
    metric = B.COSINE
    case = F.basic(metric, 128)
    idx = build(case, metric)
    sets = sets_of(idx, case["masks"])
    nq, k = 4, 10
    idx.set_bound_scan("never")
    er, ed, ec = idx.search_rowsets(case["qs"][:nq], k, sets[:nq])
    idx.set_bound_scan("always")
    st = torch.cuda.Stream()
    out_r = torch.empty((nq, k), dtype=torch.int32, device="cuda"); out_d = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    a = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    s0 = idx.bound_scan_stats()
    with torch.cuda.stream(st):
        for _ in range(8):
            a = a @ a * 1e-3                                              # queued work ahead of the search
        dq = torch.from_numpy(case["qs"][:nq].copy()).to("cuda", non_blocking=False)
        idx.search_rowsets_device(dq.data_ptr(), nq, k, sets[:nq], out_r.data_ptr(), out_d.data_ptr(), st.cuda_stream)
    st.synchronize()
    s1 = idx.bound_scan_stats()
    assert s1["searches"] - s0["searches"] == nq and s1["hand_backs"] == s0["hand_backs"]
    assert np.array_equal(out_r.cpu().numpy().view(np.uint32), er) and np.array_equal(out_d.cpu().numpy().view(np.uint32), ed.view(np.uint32))
    idx.close()


# ---- 11. declined shapes -----------------------------------------------------------------------------------------------------------------------
def test_declined_shapes_keep_the_exact_filtered_scan(capfd):
    rng = np.random.default_rng(7100)
    rows = O.gen_rows(7101, 0, 5000, 100)                                 # 100 is no multiple of 16
    m100 = rng.random(5000) < 0.5
    idx = quiver_amd.DeviceIndex(100, "cosine"); idx.add(rows)
    sel = np.flatnonzero(m100)[:9]
    (r, _, _), took, _ = both(idx, lambda: idx.search_rowsets(rows[sel[:4]], 10, idx.rowset(m100)))
    assert took == 0 and r[:, 0].tolist() == sel[:4].tolist()
    idx.close()
    rows = O.gen_rows(7102, 0, 5000, 128)
    m = rng.random(5000) < 0.5
    sel = np.flatnonzero(m)[:9]
    for make in ("flag", "metric"):
        idx = quiver_amd.DeviceIndex(128, "l2" if make == "metric" else "cosine", scan_plane=make != "flag")
        idx.add(rows)
        assert not idx.bound_scan_stats()["plane"]
        for nq in (1, 4):
            (r, _, _), took, _ = both(idx, lambda: idx.search_rowsets(rows[sel[:nq]], 10, idx.rowset(m)))
            assert took == 0 and r[:, 0].tolist() == sel[:nq].tolist()
        (r, _, _), took, _ = both(idx, lambda: idx.search_masked(rows[sel[:4]], 10, m))
        assert took == 0 and r[:, 0].tolist() == sel[:4].tolist()
        idx.close()
    idx = quiver_amd.DeviceIndex(128, "cosine"); idx.add(rows)
    rs = idx.rowset(m)
    (r, _, _), took, _ = both(idx, lambda: idx.search_rowsets(rows[sel], 10, rs))            # 9 queries
    assert took == 0 and r[:, 0].tolist() == sel.tolist()
    (r, _, _), took, _ = both(idx, lambda: idx.search_rowsets(rows[sel[:4]], 65, rs))        # k = 65
    assert took == 0 and r[:, 0].tolist() == sel[:4].tolist()
    (r, _, _), took, _ = both(idx, lambda: idx.search_rowsets(rows[sel[:4]], 64, rs))        # (and the shape next to them is taken)
    assert took == 4
    idx.close()


def test_automatic_mode_keeps_todays_kernel(monkeypatch, capfd):
    monkeypatch.setenv("QV_TRACE", "1")
    case = F.basic(B.COSINE, 128)
    idx = build(case, B.COSINE)
    sets = sets_of(idx, case["masks"])
    idx.set_bound_scan("auto")
    s0 = idx.bound_scan_stats()
    capfd.readouterr()
    r, d, c = idx.search_rowsets(case["qs"][:4], 10, sets[:4])
    err = capfd.readouterr().err
    assert idx.bound_scan_stats()["searches"] == s0["searches"]
    assert "k_rowset_scan" in err and "k_bound_scan" not in err, err
    assert agrees(B.COSINE, case["rows"], case["qs"][3], 10, F.alive_of(case["live"], case["masks"][3]), r[3], d[3], c[3])
    idx.set_bound_scan("always")
    idx.search_rowsets(case["qs"][:4], 10, sets[:4])
    idx.search_rowsets(case["qs"][:1], 10, sets[:1])
    err = capfd.readouterr().err
    assert "k_bound_scan_mq sets QB=4" in err and "k_bound_scan masked" in err, err
    idx.close()
