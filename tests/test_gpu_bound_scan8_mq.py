"""The 8-bit stage in front of a shared pass of 2 - 8 queries (k_bound_prep8_mq + k_bound_scan8_mq + k_merge_lists + k_bound_collect_mq +
k_bound_rescore_mq<., 1>, and the bfloat16 shared pass gated behind them: quiver_amd/csrc/qv_bound_scan.hip).  Every case forces the bound scan
and the shared pass's plane by the index's setters; every result is compared — rows, float32 bits, order, counts and padding — with the CPU
oracle and with the same call under "never" on the same index, and the counters say which stage answered which query: the 8-bit stage's
largest survivor count must be the CPU model's (tests/_widths.model8: the library's own interval over restated integer sums), so no test here
passes on a hand-on alone."""
import numpy as np
import pytest

import quiver_amd
from quiver_amd.device_index import device_info
from tests import _bound as B
from tests import _bound8 as B8
from tests import _callers
from tests import _extremes as X
from tests import _oracle as O
from tests import _tight as T
from tests import _widths as W

pytestmark = pytest.mark.gpu

NAME = {B.COSINE: "cosine", B.DOT: "dot"}
widths = pytest.mark.parametrize("dim", W.WIDTHS)
metrics = pytest.mark.parametrize("metric", [B.COSINE, B.DOT])


def both(idx, call, plane="8bit"):
    """(result under "always" with the shared pass's plane set, the counters' increments and last survivor counts) for ONE call; the same call
    under "never" must give the same rows, counts and bits and count nothing"""
    idx.set_bound_scan("always"); idx.set_bound_plane_mq(plane)
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


def device_call(idx, qs, k):
    """the device-pointer form of idx.search: -> (rows, distances, counts) as the host form returns them"""
    import torch
    dq = torch.from_numpy(np.array(qs, dtype=np.float32)).cuda()           # (a writable copy: the shared inputs are read-only)
    out_r = torch.empty((len(qs), k), dtype=torch.int32, device="cuda"); out_d = torch.empty((len(qs), k), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    idx.search_device(dq.data_ptr(), len(qs), k, out_r.data_ptr(), out_d.data_ptr(), 0)
    torch.cuda.synchronize()
    r = out_r.cpu().numpy().view(np.uint32); d = out_d.cpu().numpy()
    return r, d, (r != 0xFFFFFFFF).sum(axis=1).astype(np.uint32)


def index(metric, dim):
    c = W.case(dim)
    idx = quiver_amd.DeviceIndex(dim, NAME[metric])
    idx.add_synthetic(c["seed"], 0, W.N)
    idx.remove(c["dead"])
    assert idx.bound_scan_stats()["plane"] and idx.bound_scan8_stats()["plane"]
    return idx, c


@metrics
@widths
def test_bits_order_and_survivor_counts_at_every_width(metric, dim):
    """QB = 4 and 8, each part-filled and full, every rung of the 16 / 8 / 4 / 2 / 1 ladder, a ragged last tile, scattered dead rows; the host form
    at every k, the device-pointer form at k = 10"""
    idx, c = index(metric, dim)
    for nq in W.NQS:
        for k in W.KS:
            forms = [lambda: idx.search(c["qs"][:nq], k)] + ([lambda: device_call(idx, c["qs"][:nq], k)] if k == 10 else [])
            for call in forms:
                (r, d, n), inc = both(idx, call)
                want = max(W.model8(metric, dim, j, k, c["live"])["count"] for j in range(nq))
                print("dim %d metric %d nq %d k %d: %d survivors at the most, the model %d" % (dim, metric, nq, k, inc["cand8"], want))
                assert answered_by_the_8bit_stage(inc, nq), (nq, k, inc)
                assert inc["cand8"] == want and inc["cand"] == want, (nq, k, inc, want)
                for j in range(nq):
                    assert is_answer(W.oracle(metric, dim, j, k, "live"), k, r[j], d[j], n[j]), (nq, k, j)
    idx.close()


@metrics
def test_several_tiles_per_wave_the_pre_test_at_work(metric):
    """The launch has 2 workgroups of 4 waves per compute unit at the most, so 3 x 8 x CUs tiles give every wave three: the first sorted
    outright, the others behind the pre-test.  The survivor count of the pass must be the largest of the single-query 8-bit stage's on the same
    index (k_bound_scan8 has no pre-test), the answers the exact scan's and, for one query, the oracle's."""
    dim = 32
    cus = device_info(0)["cus"]
    n = 3 * 8 * cus * 64 - 37
    idx = quiver_amd.DeviceIndex(dim, NAME[metric])
    idx.add_synthetic(7300, 0, n)
    qs = O.gen_rows(7301, 0, 8, dim)
    for nq, k in ((4, 1), (4, 10), (8, 10), (5, 64)):
        single = []
        idx.set_bound_scan("always"); idx.set_bound_plane("8bit")
        for j in range(nq):
            idx.search(qs[j], k)
            single.append(idx.bound_scan8_stats()["candidates"])
        (r, d, c), inc = both(idx, lambda: idx.search(qs[:nq], k))
        assert answered_by_the_8bit_stage(inc, nq), (nq, k, inc)
        assert inc["cand8"] == max(single), (nq, k, inc, single)
    corpus = O.gen_rows(7300, 0, n, dim)
    assert is_answer(O.exact_search(metric, corpus, qs[4], 64), 64, r[4], d[4], c[4])
    idx.close()


@metrics
def test_dead_rows_a_dead_tile_and_k_above_the_live_rows(metric):
    dim = 64
    c = W.case(dim)
    idx, _ = index(metric, dim)
    gone = np.arange(64 * 11, 64 * 12, dtype=np.uint32)                   # one wholly dead tile on top of the scattered dead rows
    idx.remove(gone)
    live = c["live"].copy(); live[gone] = False
    for nq, k in ((4, 10), (8, 64), (5, 1)):
        (r, d, n), inc = both(idx, lambda: idx.search(c["qs"][:nq], k))
        want = max(W.model8(metric, dim, j, k, live)["count"] for j in range(nq))
        assert answered_by_the_8bit_stage(inc, nq) and inc["cand8"] == want, (nq, k, inc, want)
        for j in range(nq):
            assert is_answer(O.exact_search(metric, c["rows"], c["qs"][j], k, alive=live.astype(np.uint8)), k, r[j], d[j], n[j]), (nq, k, j)
    # k above the live rows: five ordinary rows and ten the bound says nothing about (NaN) stay.  k = 10: fewer than k rows have an upper
    # bound, so no query has a threshold in either stage — every one is handed on, then back, and the exact scan answers
    keep = np.flatnonzero(live)[[3, 500, 501, 1200, -1]]
    nans = np.flatnonzero(live)[20:30]
    for i in nans:
        idx.update(int(i), np.full(dim, np.nan, np.float32))
    few = np.zeros(W.N, bool); few[keep] = True; few[nans] = True
    idx.remove(np.flatnonzero(live & ~few).astype(np.uint32))
    (r, d, n), inc = both(idx, lambda: idx.search(c["qs"][:4], 10))
    assert inc["took8"] == 4 and inc["back8"] == 4 and inc["took"] == 4 and inc["back"] == 4, inc
    assert sorted(r[0, :5].tolist()) == sorted(keep.tolist())
    # k = 4: a threshold from the five ordinary rows; the ten others are passed on with them, and the 8-bit stage answers
    (r, d, n), inc = both(idx, lambda: idx.search(c["qs"][:4], 4))
    assert answered_by_the_8bit_stage(inc, 4) and 4 + 10 <= inc["cand8"] <= 5 + 10, inc
    for j in range(4):
        assert is_answer(O.exact_search(metric, c["rows"], c["qs"][j], 4, alive=(few & ~np.isin(np.arange(W.N), nans)).astype(np.uint8)), 4, r[j], d[j], n[j]), j
    # k = 64 with five live rows: the call asks the kernels for five, and the rest is padding
    idx.remove(nans.astype(np.uint32))
    (r, d, n), inc = both(idx, lambda: idx.search(c["qs"][:4], 64))
    assert answered_by_the_8bit_stage(inc, 4) and inc["cand8"] == 5, inc
    live5 = np.zeros(W.N, bool); live5[keep] = True
    for j in range(4):
        assert is_answer(O.exact_search(metric, c["rows"], c["qs"][j], 64, alive=live5.astype(np.uint8)), 64, r[j], d[j], n[j]), j
    idx.close()


@metrics
def test_a_query_that_cannot_be_quantised_is_handed_on_alone(metric):
    dim = 128
    rng = np.random.default_rng(31)
    by_name = {name: v for _, name, v in X.class_rows(rng, dim)}
    corpus = O.gen_rows(5300, 0, 8000, dim)
    idx = quiver_amd.DeviceIndex(dim, NAME[metric]); idx.add(corpus)
    ordinary = O.gen_rows(5301, 0, 8, dim)
    for name in ("zero", "nan_row", "norm1e+30"):
        for nq, slot in ((4, 0), (4, 3), (8, 7), (5, 2)):
            qs = ordinary[:nq].copy(); qs[slot] = by_name[name]
            (r, d, n), inc = both(idx, lambda: idx.search(qs, 10))
            # that query alone: on to the bfloat16 stage, which cannot work with its norm either, and from there to the exact scan
            assert inc["took8"] == nq and inc["back8"] == 1 and inc["took"] == nq and inc["back"] == 1, (name, nq, slot, inc)
            for j in range(nq):
                if j != slot:
                    assert is_answer(O.exact_search(metric, corpus, qs[j], 10), 10, r[j], d[j], n[j]), (name, nq, slot, j)
    (_, _, _), inc = both(idx, lambda: idx.search(ordinary[:5], 10))      # the words are back in their initial state
    assert answered_by_the_8bit_stage(inc, 5), inc
    idx.close()


@metrics
def test_saturated_operands_in_one_slot_of_a_pass(metric):
    """tests/_widths.saturated: every product of the first partial sum at +-127 * +-127 over 4096 dimensions, in slot 0 of a pass of four and
    in the last slot of a pass of eight, among ordinary queries: the four int32 partial sums per (query, row) and their combination in int64"""
    c = W.saturated()
    idx = quiver_amd.DeviceIndex(W.SAT_DIM, NAME[metric]); idx.add(c["rows"]); idx.remove(c["dead"])
    others = O.gen_rows(W.SAT_SEED + 1, 0, 8, W.SAT_DIM)
    st8 = B8.RowState8(c["rows"])
    stage_others = [W.stage8_of(metric, st8, q) for q in others]
    for nq, slot in ((4, 0), (8, 7)):
        qs = others[:nq].copy(); qs[slot] = c["q"]
        stages = [W.saturated_stage8(metric) if j == slot else stage_others[j] for j in range(nq)]
        for k in W.KS:
            (r, d, n), inc = both(idx, lambda: idx.search(qs, k))
            want = max(B.decide(s, k, alive=c["live"])["count"] for s in stages)
            assert answered_by_the_8bit_stage(inc, nq) and inc["cand8"] == want, (nq, k, inc, want)
            assert is_answer(O.exact_search(metric, c["rows"], c["q"], k, alive=c["live"].astype(np.uint8)), k, r[slot], d[slot], n[slot]) and int(r[slot, 0]) == W.SAT_PLUS[0]
            j = (slot + 1) % nq
            assert is_answer(O.exact_search(metric, c["rows"], qs[j], k, alive=c["live"].astype(np.uint8)), k, r[j], d[j], n[j])
    idx.close()


def cluster(metric, width, rng, dim=64, n=20_000):
    """n near-copies of one unit vector at distances spread evenly over [0, width] and a query on their centre (tests/test_gpu_bound_scan8.py)"""
    c = rng.standard_normal(dim); c /= np.linalg.norm(c)
    u = rng.standard_normal((n, dim)); u -= np.outer(u @ c, c); u /= np.linalg.norm(u, axis=1)[:, None]
    dist = np.linspace(0.0, width, n)
    along = (1.0 - dist) if metric == B.DOT else np.ones(n)
    return (along[:, None] * c[None, :] + np.sqrt(2.0 * dist)[:, None] * u).astype(np.float32), c.astype(np.float32)


@metrics
@pytest.mark.parametrize("width", [0.035, 0.0005])
def test_one_query_with_more_candidates_than_the_list_holds_is_handed_on_alone(metric, width):
    """For ONE query of a pass of four and of eight more than 4096 rows lie within the 8-bit margin of its k-th distance: that query is handed
    on to the bfloat16 stage.  Width 0.035: the bfloat16 margin keeps fewer than the list holds and that stage answers — the exact scan's
    counter does not move.  Width 0.0005: the bfloat16 stage overflows too and the query goes on to the exact scan.  Both predicted by the CPU
    models of the two stages; the other queries of the pass are answered by the 8-bit stage either way."""
    rng = np.random.default_rng(5)
    dim, k = 64, 10
    near, q = cluster(metric, width, rng)
    rows = np.concatenate([near, (0.05 * rng.standard_normal((20_000, dim))).astype(np.float32)])   # (short: far from the query under dot too)
    m8 = B8.reference8(metric, B8.RowState8(rows), q, k)
    m16 = B.reference(metric, B.RowState(rows), q, k)
    assert m8["hand_back"] and m8["count"] > B.CAND_CAP and m16["hand_back"] == (width < 0.001), (m8["count"], m16["count"])
    idx = quiver_amd.DeviceIndex(dim, NAME[metric]); idx.add(rows)
    others = rng.standard_normal((8, dim)).astype(np.float32)
    others[others @ q > 0] *= np.float32(-1.0)                          # away from the cluster: its rows are their farthest, not 20 000 near-ties
    for nq, slot in ((4, 1), (8, 7)):
        qs = others[:nq].copy(); qs[slot] = q
        (r, d, n), inc = both(idx, lambda: idx.search(qs, k))
        assert inc["took8"] == nq and inc["back8"] == 1 and inc["cand8"] == m8["count"], (nq, inc, m8["count"])
        assert inc["took"] == nq and inc["back"] == (1 if m16["hand_back"] else 0), (nq, inc)
        for j in range(nq):
            assert is_answer(O.exact_search(metric, rows, qs[j], k), k, r[j], d[j], n[j]), (nq, j)
    (_, _, _), inc = both(idx, lambda: idx.search(others[:4], k))         # the words are back in their initial state
    assert answered_by_the_8bit_stage(inc, 4), inc
    idx.close()


@metrics
@pytest.mark.parametrize("dim", [16, 48, 128])
@pytest.mark.parametrize("k", [1, 10, 64])
def test_planted_tight_cases_in_the_first_and_the_last_slot(metric, dim, k):
    """tests/_tight.planted: the k-th neighbour sits where the interval is tight.  In slot 0 of a pass of four and in the last slot of a pass of
    five (QB = 8, part-filled): a slot mix-up of the hi / lo terms or of a query's scalars changes the survivor count or loses the row."""
    case = T.planted(metric, dim, k)
    rows, q = case["rows"], case["q"]
    idx = quiver_amd.DeviceIndex(dim, NAME[metric]); idx.add(rows)
    others = O.gen_rows(9100 + dim, 0, 4, dim)
    st8 = B8.RowState8(rows)
    s_q = W.stage8_of(metric, st8, q)
    s_o = [W.stage8_of(metric, st8, o) for o in others]
    want_q = O.exact_search(metric, rows, q, k)
    assert case["target"] in want_q[0].tolist()
    for nq, slot in ((4, 0), (5, 4)):
        qs = others[:nq].copy() if nq <= 4 else np.concatenate([others, others[:1]]); qs[slot] = q
        stages = [s_q if j == slot else s_o[j % 4] for j in range(nq)]
        (r, d, n), inc = both(idx, lambda: idx.search(qs, k))
        want = max(B.decide(s, k)["count"] for s in stages)
        assert answered_by_the_8bit_stage(inc, nq) and inc["cand8"] == want, (nq, inc, want)
        assert is_answer(want_q, k, r[slot], d[slot], n[slot]), (nq, slot)
    idx.close()


def test_bf16_mode_and_a_filtered_pass_stay_on_the_bfloat16_copy():
    dim, k = 64, 10
    idx, c = index(B.COSINE, dim)
    (r, d, n), inc = both(idx, lambda: idx.search(c["qs"][:4], k), plane="bf16")
    assert inc["took8"] == 0 and inc["took"] == 4 and inc["back"] == 0, inc
    (r8, d8, n8), inc = both(idx, lambda: idx.search(c["qs"][:4], k))
    assert answered_by_the_8bit_stage(inc, 4)
    assert np.array_equal(r, r8) and d.tobytes() == d8.tobytes() and np.array_equal(n, n8)
    (r, d, n), inc = both(idx, lambda: idx.search_masked(c["qs"][:4], k, c["mask"]))
    assert inc["took8"] == 0 and inc["took"] == 4, inc
    for j in range(4):
        assert is_answer(W.oracle(B.COSINE, dim, j, k, "mask"), k, r[j], d[j], n[j]), j
    sets = [None if m is None else idx.rowset(m) for m in c["masks"][:4]]
    (r, d, n), inc = both(idx, lambda: idx.search_rowsets(c["qs"][:4], k, sets))
    assert inc["took8"] == 0 and inc["took"] == 4, inc
    (_, _, _), inc = both(idx, lambda: idx.search(c["qs"][0], k))         # one query: the single-query setters decide, not this one
    assert inc["took"] == 1
    idx.close()


def test_concurrent_callers():
    """four native threads, one query per call: whatever passes they share take the 8-bit stage when they hold 2 - 8 queries; every caller is
    served the batch call's rows and bits"""
    n, dim, k = 20_011, 128, 10
    idx = quiver_amd.DeviceIndex(dim, "cosine"); idx.add_synthetic(5400, 0, n)
    qs = O.gen_rows(5401, 0, 16, dim)
    idx.set_bound_scan("never")
    er, ed, ec = idx.search(qs, k)
    idx.set_bound_scan("always"); idx.set_bound_plane_mq("8bit")
    res = _callers.run("index", idx.handle, qs, k, threads=4, seconds=30.0, max_calls_per_thread=16)
    assert res["rc"] == 0, res["error"]
    assert res["errors"] == 0 and res["mismatches"] == 0 and res["calls"] == 4 * 16
    seen = res["count"] != 0xFFFFFFFD
    assert seen.any()
    assert np.array_equal(res["rows"][seen], er[seen]) and np.array_equal(res["dist"][seen].view(np.uint32), ed[seen].view(np.uint32))
    idx.close()


def test_sharded_handle():
    n, dim, k = 40_000, 128, 10
    rows = O.gen_rows(5400, 0, n, dim)
    sh = quiver_amd.ShardedIndex(dim, "cosine", devices=[0, 0], peer_copy=True)
    gids = sh.add(rows)
    sh.set_bound_scan("always"); sh.set_bound_plane_mq("8bit")
    assert sh.bound_scan8_stats()["plane"]
    qs = O.gen_rows(5401, 0, 4, dim)
    r, d, c = sh.search(qs, k)
    for j in range(4):
        er, ed = O.exact_search(0, rows, qs[j], k)
        assert int(c[j]) == k and np.array_equal(r[j], gids[er]) and np.array_equal(d[j].view(np.uint32), ed.view(np.uint32)), j
    s8, s = sh.bound_scan8_stats(), sh.bound_scan_stats()
    assert s8["searches"] == 8 and s8["hand_backs"] == 0 and s["searches"] == 8 and s["hand_backs"] == 0, (s8, s)
    sh.close()
