"""The 8-bit stage in front of a FILTERED shared pass of 2 - 8 queries (k_bound_prep8_mq + k_bound_scan8_mq<., ., true> + k_merge_lists +
k_bound_collect_mq + k_bound_rescore_mq<., 1>, and the filtered bfloat16 shared pass gated behind them: quiver_amd/csrc/qv_bound_scan.hip).
Every case forces the bound scan ("always") and the filtered shared pass's plane (set_bound_plane_filtered_mq("8bit")), repeats the call under
"never" on the same index and compares rows, counts and float32 bits, and reads both stages' counters; unless a case says otherwise the 8-bit
stage answered every query of the pass alone.  Where the inputs are tests/_widths.py's, the stage's largest survivor count must be the CPU
model's over each query's own candidates (tests/test_bound_scan8_filtered_mq_cpu.py shows those counts tell a right kernel from a wrong one)."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import quiver_amd
from quiver_amd.device_index import device_info
from tests import _bound as B
from tests import _bound8 as B8
from tests import _bound_filtered as F
from tests import _extremes as X
from tests import _oracle as O
from tests import _widths as W

pytestmark = pytest.mark.gpu

NAME = {B.COSINE: "cosine", B.DOT: "dot"}
widths = pytest.mark.parametrize("dim", W.WIDTHS)
metrics = pytest.mark.parametrize("metric", [B.COSINE, B.DOT])


def both(idx, call, plane="8bit"):
    """ONE call under "always" with the filtered shared pass's plane set, then under "never": the same rows, counts and bits
    -> (result, the counters' increments and last survivor counts)"""
    idx.set_bound_scan("always"); idx.set_bound_plane_filtered_mq(plane)
    a0, b0 = idx.bound_scan8_stats(), idx.bound_scan_stats()
    r, d, c = call()
    a1, b1 = idx.bound_scan8_stats(), idx.bound_scan_stats()
    idx.set_bound_scan("never")
    er, ed, ec = call()
    assert idx.bound_scan8_stats()["searches"] == a1["searches"] and idx.bound_scan_stats()["searches"] == b1["searches"]   # "never" is never
    assert np.array_equal(c, ec) and np.array_equal(r, er), (r, er)
    assert X.same(d, ed), (d, ed)
    return (r, d, c), {"took": b1["searches"] - b0["searches"], "back": b1["hand_backs"] - b0["hand_backs"], "cand": b1["candidates"],
                       "took8": a1["searches"] - a0["searches"], "back8": a1["hand_backs"] - a0["hand_backs"], "cand8": a1["candidates"]}


def answered_by_the_8bit_stage(inc, nq):
    return inc["took8"] == nq and inc["back8"] == 0 and inc["took"] == nq and inc["back"] == 0


def is_answer(want, k, r, d, c):
    """rows, float32 bits, count and padding of one query's result against the oracle's (rows, distances)"""
    er, ed = want
    w = len(er)
    return int(c) == w and r[:w].tolist() == er.tolist() and d[:w].tobytes() == ed.tobytes() and (r[w:] == 0xFFFFFFFF).all() and np.isposinf(d[w:]).all() and len(r) == k


def oracle(metric, rows, q, k, alive):
    return O.exact_search(metric, rows, q, k, alive=np.asarray(alive).astype(np.uint8))


def sets_of(idx, masks):
    return [None if m is None else idx.rowset(m) for m in masks]


def device_rowsets(idx, qs, k, sets, stream=0):
    """the device-pointer form of idx.search_rowsets: -> (rows, distances, counts) as the host form returns them"""
    import torch
    dq = torch.from_numpy(np.array(qs, dtype=np.float32)).cuda()           # (a writable copy: the shared inputs are read-only)
    out_r = torch.empty((len(qs), k), dtype=torch.int32, device="cuda"); out_d = torch.empty((len(qs), k), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    idx.search_rowsets_device(dq.data_ptr(), len(qs), k, sets, out_r.data_ptr(), out_d.data_ptr(), stream)
    torch.cuda.synchronize()
    r = out_r.cpu().numpy().view(np.uint32); d = out_d.cpu().numpy()
    return r, d, (r != 0xFFFFFFFF).sum(axis=1).astype(np.uint32)


def width_index(metric, dim):
    c = W.case(dim)
    idx = quiver_amd.DeviceIndex(dim, NAME[metric])
    idx.add_synthetic(c["seed"], 0, W.N)
    idx.remove(c["dead"])
    assert idx.bound_scan_stats()["plane"] and idx.bound_scan8_stats()["plane"]
    return idx, c


# ---- 1. widths: a set per query -------------------------------------------------------------------------------------------------------------
@metrics
@widths
def test_widths_with_a_set_per_query(metric, dim):
    """every rung of the 16 / 8 / 4 / 2 / 1 ladder, QB = 4 and 8 part-filled and full, a ragged last tile, tombstones, two tiles no query of a
    pass of four selects, whole-tile sets and one query without a set (mask 6)"""
    idx, c = width_index(metric, dim)
    sets = sets_of(idx, c["masks"])
    for nq in W.NQS:
        for k in W.KS:
            forms = [lambda: idx.search_rowsets(c["qs"][:nq], k, sets[:nq])] + ([lambda: device_rowsets(idx, c["qs"][:nq], k, sets[:nq])] if k == 10 else [])
            for call in forms:
                (r, d, n), inc = both(idx, call)
                want = max(W.model8(metric, dim, j, k, W.alive_of(c["live"], c["masks"][j]))["count"] for j in range(nq))
                print("dim %d metric %d nq %d k %d: %d survivors at the most, the model %d" % (dim, metric, nq, k, inc["cand8"], want))
                assert answered_by_the_8bit_stage(inc, nq), (nq, k, inc)
                assert inc["cand8"] == want and inc["cand"] == want, (nq, k, inc, want)
                for j in range(nq):
                    assert is_answer(W.oracle(metric, dim, j, k, "set"), k, r[j], d[j], n[j]), (nq, k, j)
    idx.close()


# ---- 2. widths: one mask for the pass -------------------------------------------------------------------------------------------------------
@metrics
@widths
def test_widths_under_search_masked(metric, dim):
    """one bitmap in the index's place of `alive` and a table of null sets; every third tile is empty and is not read"""
    idx, c = width_index(metric, dim)
    alive = c["live"] & c["mask"]
    for nq in W.NQS:
        for k in W.KS:
            (r, d, n), inc = both(idx, lambda: idx.search_masked(c["qs"][:nq], k, c["mask"]))
            want = max(W.model8(metric, dim, j, k, alive)["count"] for j in range(nq))
            print("dim %d metric %d nq %d k %d: %d survivors at the most, the model %d" % (dim, metric, nq, k, inc["cand8"], want))
            assert answered_by_the_8bit_stage(inc, nq), (nq, k, inc)
            assert inc["cand8"] == want and inc["cand"] == want, (nq, k, inc, want)
            for j in range(nq):
                assert is_answer(W.oracle(metric, dim, j, k, "mask"), k, r[j], d[j], n[j]), (nq, k, j)
    idx.close()


# ---- 3. where-filters -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_where_filters(metric):
    """tests/test_gpu_search_where.py::test_bound_scan_routes' index and eight predicates (one of them none): transient sets in a pass.  The CPU
    model of the 8-bit stage over each predicate's rows hands no query on, so the stage, not a redo behind it, must have answered the pass,
    with the model's largest survivor count"""
    n, dim, k = 20011, 128, 10
    rng = np.random.default_rng(50)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    idx = quiver_amd.DeviceIndex(dim, metric)
    idx.add(rows)
    vals = rng.integers(0, 10, n).astype(np.uint32)
    col = idx.column("u32")
    col.set(0, vals)
    specs = [[(col, "lt", 5)], [(col, "eq", 3)], [(col, "ge", 2)], [(col, "in", [1, 9])], [(col, "ne", 0)], None, [(col, "gt", 7)], [(col, "le", 8)]]
    masks = [vals < 5, vals == 3, vals >= 2, np.isin(vals, (1, 9)), vals != 0, np.ones(n, bool), vals > 7, vals <= 8]
    qs = rng.standard_normal((8, dim)).astype(np.float32)
    mid = quiver_amd.metric_id(metric)
    state8 = B8.RowState8(rows)
    models = [B.decide(W.stage8_of(mid, state8, qs[j]), k, alive=masks[j]) for j in range(8)]
    assert not any(m["hand_back"] for m in models)
    for nq in (4, 8):
        (r, d, c), inc = both(idx, lambda: idx.search_where(qs[:nq], k, specs[:nq]))
        assert answered_by_the_8bit_stage(inc, nq), (nq, inc)
        assert inc["cand8"] == max(m["count"] for m in models[:nq]), (nq, inc, [m["count"] for m in models[:nq]])
        for j in range(nq):
            assert is_answer(oracle(mid, rows, qs[j], k, masks[j]), k, r[j], d[j], c[j]), (nq, j)
    # automatic mode: the pass is declined as before this stage existed
    idx.set_bound_scan("auto"); idx.set_bound_plane_filtered_mq("auto")
    a0, b0 = idx.bound_scan8_stats()["searches"], idx.bound_scan_stats()["searches"]
    idx.search_where(qs[:4], k, specs[:4])
    assert idx.bound_scan8_stats()["searches"] == a0 and idx.bound_scan_stats()["searches"] == b0
    idx.close()


# ---- 4. stale lower bounds --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [4, 8])
def test_a_skipped_tile_holds_no_earlier_searchs_bounds(nq):
    """an 8-bit pass without sets writes every tile's lower bounds (the answers lie in tiles t % 3 != 0); the same queries under sets that select
    only tiles t % 3 == 0 then run in the same workspace: the words of the tiles they skip must not be the earlier pass's"""
    metric = B.COSINE
    case = F.stale(metric)
    idx = quiver_amd.DeviceIndex(case["rows"].shape[1], NAME[metric]); idx.add(case["rows"])
    pick = [j % 4 for j in range(nq)]
    qs = case["qs"][pick]
    masks = [case["masks"][j] for j in pick]
    sets = sets_of(idx, masks)
    k = 10
    idx.set_bound_scan("always"); idx.set_bound_plane_filtered_mq("8bit")
    a0 = idx.bound_scan8_stats()
    r0, _, _ = idx.search_rowsets(qs, k, [None] * nq)                     # no sets, same entry, same context
    a1 = idx.bound_scan8_stats()
    assert a1["searches"] - a0["searches"] == nq and a1["hand_backs"] == a0["hand_backs"]
    assert r0[:, 0].tolist() == case["at"][pick].tolist() and ((r0[:, 0] // 64) % 3 != 0).all()
    (r, d, c), inc = both(idx, lambda: idx.search_rowsets(qs, k, sets))
    assert answered_by_the_8bit_stage(inc, nq), inc
    for j in range(nq):
        assert ((r[j] // 64) % 3 == 0).all()
        assert is_answer(oracle(metric, case["rows"], qs[j], k, masks[j]), k, r[j], d[j], c[j]), j
    idx.close()


# ---- 5. the first tile a wave reads -------------------------------------------------------------------------------------------------------------
def test_the_first_tile_a_wave_reads():
    """3 x 8 x CUs tiles of 32 dimensions: every wave owns tiles w, w + 8 CUs and w + 16 CUs.  Query 0's set selects rows of the second and the
    third only — the first tile every wave OWNS is empty for every query and is not read —, query 1's rows of the third only: in the first
    tile a wave READS query 1 has no candidate, keeps a dead list, and its candidates of the next tile are inserted into it.  Passes of two
    (QB = 4) and of five (QB = 8: the two queries and sets in turn)."""
    metric, dim, k = B.COSINE, 32, 10
    cus = device_info(0)["cus"]
    n = 3 * 8 * cus * 64 - 37
    rows = O.gen_rows(7400, 0, n, dim)
    q2 = O.gen_rows(7401, 0, 2, dim)
    tile = np.arange(n) // 64
    rng = np.random.default_rng(7402)
    m2 = [(tile >= 8 * cus) & (rng.random(n) < 0.5), (tile >= 16 * cus) & (rng.random(n) < 0.25)]
    idx = quiver_amd.DeviceIndex(dim, NAME[metric]); idx.add_synthetic(7400, 0, n)
    st8 = B8.RowState8(rows)
    models = [B.decide(W.stage8_of(metric, st8, q2[j]), k, alive=m2[j]) for j in range(2)]
    assert not models[0]["hand_back"] and not models[1]["hand_back"]
    wants = [oracle(metric, rows, q2[j], k, m2[j]) for j in range(2)]
    s2 = sets_of(idx, m2)
    for nq in (2, 5):
        pick = [j % 2 for j in range(nq)]
        (r, d, c), inc = both(idx, lambda: idx.search_rowsets(q2[pick], k, [s2[j] for j in pick]))
        assert answered_by_the_8bit_stage(inc, nq), (nq, inc)
        assert inc["cand8"] == max(m["count"] for m in models), (nq, inc, [m["count"] for m in models])
        for i, j in enumerate(pick):
            assert is_answer(wants[j], k, r[i], d[i], c[i]), (nq, i)
            assert (r[i] // 64 >= (8 if j == 0 else 16) * cus).all()
    idx.close()


# ---- 6. several tiles per wave ------------------------------------------------------------------------------------------------------------------
@metrics
def test_several_tiles_per_wave(metric):
    """every wave walks three tiles, the second and third behind the pre-test over each query's own candidates: the pass's survivor count must
    be the largest of the single filtered 8-bit searches (k_bound_scan8<., true>, no pre-test) of the same queries and sets"""
    dim = 32
    cus = device_info(0)["cus"]
    n = 3 * 8 * cus * 64 - 37
    idx = quiver_amd.DeviceIndex(dim, NAME[metric])
    idx.add_synthetic(7300, 0, n)
    qs = O.gen_rows(7301, 0, 8, dim)
    rng = np.random.default_rng(7302)
    masks = [(rng.random(n) < 0.5, rng.random(n) < 0.25, None)[j % 3] for j in range(8)]
    sets = sets_of(idx, masks)
    for nq, k in ((4, 1), (4, 10), (8, 10), (5, 64)):
        single = []
        idx.set_bound_scan("always"); idx.set_bound_plane_filtered("8bit"); idx.set_bound_plane("8bit")   # (a query without a set is an unfiltered one)
        for j in range(nq):
            a0 = idx.bound_scan8_stats()
            idx.search_rowsets(qs[j:j + 1], k, sets[j:j + 1])
            a1 = idx.bound_scan8_stats()
            assert a1["searches"] - a0["searches"] == 1 and a1["hand_backs"] == a0["hand_backs"], (nq, k, j)
            single.append(a1["candidates"])
        (r, d, c), inc = both(idx, lambda: idx.search_rowsets(qs[:nq], k, sets[:nq]))
        assert answered_by_the_8bit_stage(inc, nq), (nq, k, inc)
        assert inc["cand8"] == max(single), (nq, k, inc, single)
    corpus = O.gen_rows(7300, 0, n, dim)
    assert is_answer(oracle(metric, corpus, qs[4], 64, masks[4]), 64, r[4], d[4], c[4])
    idx.close()


# ---- 7. fewer than k candidates in one query's set ------------------------------------------------------------------------------------------------
@metrics
def test_fewer_than_k_candidates_in_one_querys_set(metric):
    """a set of five live rows, then an empty one, at k = 10 in a pass of four and of eight: no threshold in either stage for that query, which
    alone ends in the exact filtered scan; the others are answered by the 8-bit stage"""
    case = F.short(metric)
    idx = quiver_amd.DeviceIndex(128, NAME[metric]); idx.add(case["rows"]); idx.remove(case["dead"])
    k = 10
    ordinary = (0, 2)
    for nq, slot, short in ((4, 2, 3), (8, 7, 3), (4, 0, 1), (5, 4, 1)):
        pick = [ordinary[i % 2] for i in range(nq)]; pick[slot] = short
        qs = case["qs"][pick]
        masks = [case["masks"][j] for j in pick]
        (r, d, c), inc = both(idx, lambda: idx.search_rowsets(qs, k, sets_of(idx, masks)))
        assert inc["took8"] == nq and inc["back8"] == 1 and inc["took"] == nq and inc["back"] == 1, (nq, slot, inc)
        assert int(c[slot]) == (5 if short == 3 else 0)
        for i in range(nq):
            assert is_answer(oracle(metric, case["rows"], qs[i], k, case["live"] & masks[i]), k, r[i], d[i], c[i]), (nq, slot, i)
    # the words are back in their initial state
    pick = [0, 2, 0, 2]
    (_, _, _), inc = both(idx, lambda: idx.search_rowsets(case["qs"][pick], k, sets_of(idx, [case["masks"][j] for j in pick])))
    assert answered_by_the_8bit_stage(inc, 4), inc
    idx.close()


# ---- 8. near-duplicate clusters inside one query's set ----------------------------------------------------------------------------------------------
@metrics
def test_a_near_duplicate_cluster_inside_one_querys_set(metric):
    """tests/_bound_filtered.clusters: query 1 sits on a centre, half of whose 20 000 near-copies its set selects — more than the list holds
    within the 8-bit margin: that query alone is handed on.  What the bfloat16 stage does with it is its CPU model's word; the three others
    are answered by the 8-bit stage."""
    case = F.clusters(metric)
    rows = case["rows"]
    idx = quiver_amd.DeviceIndex(rows.shape[1], NAME[metric]); idx.add(rows)
    sets = sets_of(idx, case["masks"])
    k = 10
    m8 = B8.reference8(metric, B8.RowState8(rows), case["qs"][1], k, alive=case["masks"][1])
    m16 = B.reference(metric, B.RowState(rows), case["qs"][1], k, alive=case["masks"][1])
    assert m8["hand_back"] and m8["count"] > B.CAND_CAP, m8["count"]
    (r, d, c), inc = both(idx, lambda: idx.search_rowsets(case["qs"], k, sets))
    assert inc["took8"] == 4 and inc["back8"] == 1 and inc["took"] == 4 and inc["back"] == (1 if m16["hand_back"] else 0), (inc, m16["hand_back"])
    assert inc["cand8"] == m8["count"], (inc, m8["count"])
    for j in range(4):
        assert is_answer(oracle(metric, rows, case["qs"][j], k, case["masks"][j]), k, r[j], d[j], c[j]), j
    assert case["masks"][1][r[1]].all()
    idx.close()


@metrics
def test_a_cluster_the_bfloat16_stage_can_decide(metric):
    """tests/test_gpu_bound_scan8_mq.py's cluster at width 0.035 (20 000 near-copies at distances spread over [0, 0.035]) under a set that leaves
    out a few whole tiles, in one slot of a pass of four and of eight: the 8-bit stage keeps more than its list holds, the bfloat16 stage fewer —
    that query goes on alone and is answered there; the exact scan's counter does not move"""
    rng = np.random.default_rng(5)
    dim, per, k = 64, 20_000, 10
    cen = rng.standard_normal(dim); cen /= np.linalg.norm(cen)
    u = rng.standard_normal((per, dim)); u -= np.outer(u @ cen, cen); u /= np.linalg.norm(u, axis=1)[:, None]
    dist = np.linspace(0.0, 0.035, per)
    along = (1.0 - dist) if metric == B.DOT else np.ones(per)
    near = (along[:, None] * cen[None, :] + np.sqrt(2.0 * dist)[:, None] * u).astype(np.float32)
    q = cen.astype(np.float32)
    rows = np.concatenate([near, (0.05 * rng.standard_normal((per, dim))).astype(np.float32)])
    n = rows.shape[0]
    tile = np.arange(n) // 64
    mask = ~np.isin(tile, (0, 3, 4, 17, 100))                             # the nearest rows' tile among those left out
    m8 = B8.reference8(metric, B8.RowState8(rows), q, k, alive=mask)
    m16 = B.reference(metric, B.RowState(rows), q, k, alive=mask)
    assert m8["hand_back"] and m8["count"] > B.CAND_CAP and not m16["hand_back"], (m8["count"], m16["count"])
    idx = quiver_amd.DeviceIndex(dim, NAME[metric]); idx.add(rows)
    others = rng.standard_normal((8, dim)).astype(np.float32)
    others[others @ q > 0] *= np.float32(-1.0)                            # away from the cluster
    other_masks = [rng.random(n) < 0.5 for _ in range(8)]
    for nq, slot in ((4, 1), (8, 7)):
        qs = others[:nq].copy(); qs[slot] = q
        masks = other_masks[:nq]; masks[slot] = mask
        (r, d, c), inc = both(idx, lambda: idx.search_rowsets(qs, k, sets_of(idx, masks)))
        assert inc["took8"] == nq and inc["back8"] == 1 and inc["took"] == nq and inc["back"] == 0, (nq, inc)
        assert inc["cand8"] == m8["count"], (nq, inc, m8["count"])
        for j in range(nq):
            assert is_answer(oracle(metric, rows, qs[j], k, masks[j]), k, r[j], d[j], c[j]), (nq, j)
    idx.close()


# ---- 9. rows the bound says nothing about; a set made before the index grew -----------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_undecidable_rows_inside_and_outside_a_set(metric):
    dim, n = 128, 8000
    rng = np.random.default_rng(41)
    extreme = X.class_rows(rng, dim)
    rows = O.gen_rows(8700, 0, n, dim)
    placed = np.array([(j * 397) % n for j in range(len(extreme))])
    for at, (_, _, v) in zip(placed, extreme):
        rows[at] = v
    unsure = np.isnan(B8.RowState8(rows[placed]).res)
    assert unsure.sum() >= 4
    inside = placed[unsure][0::2]; outside = placed[unsure][1::2]
    mask = np.random.default_rng(8701).random(n) < 0.5
    mask[placed] = True; mask[outside] = False
    others = [np.random.default_rng(8703 + j).random(n) < 0.5 for j in range(3)]
    mid = quiver_amd.metric_id(metric)
    idx = quiver_amd.DeviceIndex(dim, metric); idx.add(rows)
    qs = O.gen_rows(8702, 0, 4, dim)
    state8 = B8.RowState8(rows)
    stages = [W.stage8_of(mid, state8, qs[j]) for j in range(4)]
    for slot in (0, 3):
        masks = list(others); masks.insert(slot, mask)
        sets = sets_of(idx, masks)
        for k in (1, 10, 64):
            (r, d, c), inc = both(idx, lambda: idx.search_rowsets(qs, k, sets))
            assert answered_by_the_8bit_stage(inc, 4), (slot, k, inc)
            models = [B.decide(stages[j], k, alive=masks[j]) for j in range(4)]
            assert models[slot]["passed"][inside].all() and not models[slot]["passed"][outside].any()
            assert inc["cand8"] == max(m["count"] for m in models), (slot, k, inc)
            assert not np.isin(r[slot], outside).any()
            for j in range(4):
                er, ed = oracle(mid, rows, qs[j], k, masks[j])
                assert np.array_equal(r[j], er) and X.same(d[j], ed), (slot, k, j)
    idx.close()


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
        (r, d, c), inc = both(idx, lambda: idx.search_rowsets(qs, k, sets))
        assert answered_by_the_8bit_stage(inc, 4), (where, inc)
        for j in range(4):
            assert is_answer(oracle(metric, rows, qs[j], k, live & masks[j]), k, r[j], d[j], c[j]), (where, j)

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


# ---- 10. the setters are independent ----------------------------------------------------------------------------------------------------------------
def test_the_plane_setters_are_independent():
    metric = B.COSINE
    case = F.masked(metric)
    idx = quiver_amd.DeviceIndex(128, NAME[metric]); idx.add(case["rows"]); idx.remove(case["dead"])
    k, qs, mask = 10, case["qs"][:4], case["masks"][0]
    rs = idx.rowset(mask)
    want = oracle(metric, case["rows"], qs[0], k, case["live"] & mask)

    def run(call):
        a0, b0 = idx.bound_scan8_stats(), idx.bound_scan_stats()
        out = call()
        a1, b1 = idx.bound_scan8_stats(), idx.bound_scan_stats()
        return out, a1["searches"] - a0["searches"], b1["searches"] - b0["searches"]

    idx.set_bound_scan("always")
    # the three older setters at "8bit", this one at "bf16": a filtered pass stays on the bfloat16 copy
    idx.set_bound_plane("8bit"); idx.set_bound_plane_filtered("8bit"); idx.set_bound_plane_mq("8bit"); idx.set_bound_plane_filtered_mq("bf16")
    for call in (lambda: idx.search_rowsets(qs, k, [rs] * 4), lambda: idx.search_masked(qs, k, mask)):
        (r, d, c), took8, took = run(call)
        assert (took8, took) == (0, 4)
        assert is_answer(want, k, r[0], d[0], c[0])
    # ... and left at its default too: automatic mode takes nothing at this shape
    idx.set_bound_plane_filtered_mq("auto")
    (r, d, c), took8, took = run(lambda: idx.search_rowsets(qs, k, [rs] * 4))
    assert (took8, took) == (0, 4)
    # this one at "8bit", the others at "bf16": neither an unfiltered pass nor a single filtered query moves
    idx.set_bound_plane("bf16"); idx.set_bound_plane_filtered("bf16"); idx.set_bound_plane_mq("bf16"); idx.set_bound_plane_filtered_mq("8bit")
    for call, nq in ((lambda: idx.search(qs, k), 4), (lambda: idx.search(qs[0], k), 1), (lambda: idx.search_rowsets(qs[:1], k, [rs]), 1),
                     (lambda: idx.search_masked(qs[0], k, mask), 1)):
        _, took8, took = run(call)
        assert (took8, took) == (0, nq), nq
    (r, d, c), took8, took = run(lambda: idx.search_rowsets(qs, k, [rs] * 4))
    assert (took8, took) == (4, 4)
    assert is_answer(want, k, r[0], d[0], c[0])
    idx.close()


# ---- 11. an index without the 8-bit plane -------------------------------------------------------------------------------------------------------------
def test_an_index_without_the_plane_runs_on_the_copy_or_exactly():
    rows = O.gen_rows(88, 0, 5000, 128)
    rng = np.random.default_rng(8900)
    masks = [rng.random(5000) < 0.5 for _ in range(4)]
    qs = rows[[3, 70, 900, 4000]]
    wants = [oracle(0, rows, qs[j], 10, masks[j]) for j in range(4)]
    for make in ("flag", "oom8"):
        if make == "oom8":
            os.environ["QV_TEST_PLANE8_OOM"] = "1"                         # the 8-bit plane's allocation answers out-of-memory: not an error
        try:
            idx = quiver_amd.DeviceIndex(128, "cosine", scan_plane=make != "flag")
            idx.add(rows)
        finally:
            os.environ.pop("QV_TEST_PLANE8_OOM", None)
        assert not idx.bound_scan8_stats()["plane"] and idx.bound_scan_stats()["plane"] == (make == "oom8")
        sets = sets_of(idx, masks)
        (r, d, c), inc = both(idx, lambda: idx.search_rowsets(qs, 10, sets))
        assert inc["took8"] == 0 and inc["took"] == (4 if make == "oom8" else 0) and inc["back"] == 0, (make, inc)
        for j in range(4):
            assert is_answer(wants[j], 10, r[j], d[j], c[j]), (make, j)
        (r, d, c), inc = both(idx, lambda: idx.search_masked(qs, 10, masks[0]))
        assert inc["took8"] == 0 and inc["took"] == (4 if make == "oom8" else 0), (make, inc)
        idx.close()


# ---- 12. concurrent callers ---------------------------------------------------------------------------------------------------------------------------
def test_concurrent_callers_with_their_own_sets_and_where_filters():
    """eight threads through the row-set front, two queries per call — first each query with its own row set, then each with its own
    where-filter.  A call that runs alone is a filtered pass of two, calls the front puts together are one of up to eight (beyond eight queries
    a group takes the exact filtered scan and counts nothing): whichever way the timing falls, every query that took the bound scan started on
    the 8-bit plane, some did, nothing was handed on, and every answer is the oracle's over its own live & set."""
    n, dim, k, callers, each = 60_000, 128, 10, 8, 12
    idx = quiver_amd.DeviceIndex(dim, "cosine"); idx.add_synthetic(6900, 0, n)
    rows = O.gen_rows(6900, 0, n, dim)
    qs = O.gen_rows(6901, 0, callers, dim)
    rng = np.random.default_rng(6902)
    vals = rng.random(n) * 100.0
    col = idx.column("f64"); col.set(0, vals)
    cuts = [8.0 + 11.5 * j for j in range(callers)]
    filt = [[(col, "lt", cuts[j])] for j in range(callers)]
    kinds = {"sets": [rng.random(n) < (0.5, 0.2, 0.05, 1.0)[j % 4] for j in range(callers)], "where": [vals < cuts[j] for j in range(callers)]}
    for kind, masks in kinds.items():
        sets = sets_of(idx, masks) if kind == "sets" else None
        want = [oracle(B.COSINE, rows, qs[j], k, masks[j]) for j in range(callers)]
        idx.set_bound_scan("always"); idx.set_bound_plane_filtered_mq("8bit"); idx.set_bound_plane_filtered("bf16")
        a0, s0 = idx.bound_scan8_stats(), idx.bound_scan_stats()
        bad = []
        start = threading.Barrier(callers)

        def caller(j):
            mine = [j, (j + 1) % callers]
            start.wait()
            for _ in range(each):
                if kind == "sets":
                    r, d, c = idx.search_rowsets(qs[mine], k, [sets[i] for i in mine])
                else:
                    r, d, c = idx.search_where(qs[mine], k, [filt[i] for i in mine])
                for x, i in enumerate(mine):
                    if not is_answer(want[i], k, r[x], d[x], c[x]):
                        bad.append((j, i))

        ts = [threading.Thread(target=caller, args=(j,)) for j in range(callers)]
        [t.start() for t in ts]; [t.join() for t in ts]
        a1, s1 = idx.bound_scan8_stats(), idx.bound_scan_stats()
        assert not bad, (kind, bad)
        assert a1["searches"] - a0["searches"] > 0, (kind, a0, a1)        # the 8-bit stage ran
        assert a1["searches"] - a0["searches"] == s1["searches"] - s0["searches"], (kind, a0, a1, s0, s1)   # ... for every query the bound scan took
        assert a1["hand_backs"] == a0["hand_backs"] and s1["hand_backs"] == s0["hand_backs"], (kind, a0, a1, s0, s1)
    idx.close()


# ---- 13. the device form on a busy stream ----------------------------------------------------------------------------------------------------------------
def test_device_form_behind_queued_work():
    import torch
    metric = B.COSINE
    case = F.basic(metric, 128)
    idx = quiver_amd.DeviceIndex(128, NAME[metric]); idx.add(case["rows"]); idx.remove(case["dead"])
    sets = sets_of(idx, case["masks"])
    k = 10
    for nq in (4, 8):
        idx.set_bound_scan("never")
        er, ed, ec = idx.search_rowsets(case["qs"][:nq], k, sets[:nq])
        idx.set_bound_scan("always"); idx.set_bound_plane_filtered_mq("8bit")
        st = torch.cuda.Stream()
        out_r = torch.empty((nq, k), dtype=torch.int32, device="cuda"); out_d = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        a = torch.randn(2048, 2048, device="cuda")
        torch.cuda.synchronize()
        a0, s0 = idx.bound_scan8_stats(), idx.bound_scan_stats()
        with torch.cuda.stream(st):
            for _ in range(8):
                a = a @ a * 1e-3                                          # queued work ahead of the search
            dq = torch.from_numpy(case["qs"][:nq].copy()).to("cuda", non_blocking=False)
            idx.search_rowsets_device(dq.data_ptr(), nq, k, sets[:nq], out_r.data_ptr(), out_d.data_ptr(), st.cuda_stream)
        st.synchronize()
        a1, s1 = idx.bound_scan8_stats(), idx.bound_scan_stats()
        assert a1["searches"] - a0["searches"] == nq and a1["hand_backs"] == a0["hand_backs"], (nq, a0, a1)
        assert s1["searches"] - s0["searches"] == nq and s1["hand_backs"] == s0["hand_backs"], (nq, s0, s1)
        assert np.array_equal(out_r.cpu().numpy().view(np.uint32), er) and np.array_equal(out_d.cpu().numpy().view(np.uint32), ed.view(np.uint32)), nq
    idx.close()


# ---- 14. the trace line; automatic mode ---------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys
import numpy as np
import quiver_amd
from tests import _bound as B
from tests import _bound_filtered as F
case = F.basic(B.COSINE, 128)
idx = quiver_amd.DeviceIndex(128, "cosine"); idx.add(case["rows"]); idx.remove(case["dead"])
sets = [None if m is None else idx.rowset(m) for m in case["masks"]]
def run(tag, nq):
    a0, b0 = idx.bound_scan8_stats()["searches"], idx.bound_scan_stats()["searches"]
    sys.stderr.write("@@BEGIN %s\n" % tag); sys.stderr.flush()
    idx.search_rowsets(case["qs"][:nq], 10, sets[:nq])
    sys.stderr.write("@@END %s\n" % tag); sys.stderr.flush()
    print("@@COUNT %s %d %d" % (tag, idx.bound_scan8_stats()["searches"] - a0, idx.bound_scan_stats()["searches"] - b0))
run("auto", 4)                                         # every setter at its default
idx.set_bound_scan("always")
run("always", 4)                                       # the plane still at its default
idx.set_bound_plane_filtered_mq("8bit")
run("8bit4", 4)
run("8bit8", 8)
"""


def test_the_trace_line_and_automatic_mode():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("QV_BOUND_")}
    p = subprocess.run([sys.executable, "-c", CHILD], env=dict(env, QV_TRACE="1"), capture_output=True, text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stderr[-4000:]
    counts = {l.split()[1]: (int(l.split()[2]), int(l.split()[3])) for l in p.stdout.splitlines() if l.startswith("@@COUNT ")}
    err = p.stderr

    def lines(tag):
        return [l for l in err[err.index("@@BEGIN " + tag):err.index("@@END " + tag)].splitlines() if l.startswith("qv: scan kernel")]

    tiles = (F.N + 63) // 64
    # automatic mode at this shape keeps the kernels it had: the exact filtered scan, nothing counted
    assert counts["auto"] == (0, 0) and any("k_rowset_scan" in l for l in lines("auto")) and not any("k_bound_scan" in l for l in lines("auto")), lines("auto")
    assert counts["always"] == (0, 4) and lines("always") == ["qv: scan kernel = k_bound_scan_mq sets QB=4 (nq=4, tiles=%u)" % tiles], lines("always")
    assert counts["8bit4"] == (4, 4) and lines("8bit4") == ["qv: scan kernel = k_bound_scan8_mq sets QB=4, then gated k_bound_scan_mq sets (nq=4, tiles=%u)" % tiles], lines("8bit4")
    assert counts["8bit8"] == (8, 8) and lines("8bit8") == ["qv: scan kernel = k_bound_scan8_mq sets QB=8, then gated k_bound_scan_mq sets (nq=8, tiles=%u)" % tiles], lines("8bit8")
