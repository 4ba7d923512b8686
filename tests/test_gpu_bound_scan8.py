"""The 8-bit stage of the single-query bound scan (k_bound_scan8, quiver_amd/csrc/qv_bound_scan.hip): stage 1 rejects rows on the index's int8
plane with integer dot products, the survivors are walked in the exact scan's arithmetic, and a search the stage cannot decide goes on
to the bfloat16 stage gated behind it, then to the exact scan.  Every case forces the bound scan and the 8-bit plane by the index's
setters; every result is compared, rows and float32 bits, with the exact scan of the SAME index and with the CPU oracle — and the
counters say which stage answered: a test here must not pass on a hand-back alone."""
import os

import numpy as np
import pytest

import quiver_amd
from tests import _bound as B
from tests import _bound8 as B8
from tests import _extremes as X
from tests import _oracle as O
from tests import _widths as W

pytestmark = pytest.mark.gpu


def both(idx, q, k):
    """one query through the 8-bit stage and through the exact scan of the same index -> (result, counters' increments)"""
    idx.set_bound_scan("always"); idx.set_bound_plane("8bit")
    a0, b0 = idx.bound_scan8_stats(), idx.bound_scan_stats()
    r, d, c = idx.search(q, k)
    a1, b1 = idx.bound_scan8_stats(), idx.bound_scan_stats()
    idx.set_bound_scan("never")
    er, ed, ec = idx.search(q, k)
    assert idx.bound_scan8_stats()["searches"] == a1["searches"] and idx.bound_scan_stats()["searches"] == b1["searches"]   # "never" is never
    assert np.array_equal(c, ec) and np.array_equal(r, er), (k, r, er)
    assert X.same(d, ed), (k, d, ed)
    inc = {"took8": a1["searches"] - a0["searches"], "back8": a1["hand_backs"] - a0["hand_backs"], "cand8": a1["candidates"],
           "took": b1["searches"] - b0["searches"], "back": b1["hand_backs"] - b0["hand_backs"], "cand": b1["candidates"]}
    return (r, d, c), inc


def answered_by_the_8bit_stage(inc):
    return inc["took8"] == 1 and inc["back8"] == 0 and inc["took"] == 1 and inc["back"] == 0


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("dim", [16, 128, 768, 1536])
def test_rows_and_bits_of_the_exact_scan_and_the_oracle(metric, dim):
    """k = 1 / 10 / 63 / 64, a ragged last tile, several workgroups; stage 1's survivor count against the CPU model's (tests/_bound8.py's
    intervals, once per query: tests/_widths.stage8_of)"""
    n = 20_011 if dim <= 768 else 9_003
    idx = quiver_amd.DeviceIndex(dim, metric)
    idx.add_synthetic(5100 + dim, 0, n)
    assert idx.bound_scan8_stats()["plane"] and idx.bound_scan_stats()["plane"]
    qs = O.gen_rows(5101 + dim, 0, 2, dim)
    corpus = O.gen_rows(5100 + dim, 0, n, dim)
    mid = quiver_amd.metric_id(metric)
    state8 = B8.RowState8(corpus)
    stage8 = [W.stage8_of(mid, state8, q) for q in qs]
    for k in (1, 10, 63, 64):
        for i in range(2):
            (r, d, c), inc = both(idx, qs[i], k)
            assert answered_by_the_8bit_stage(inc), (k, i, inc)
            assert k <= inc["cand8"] <= 4096 and inc["cand"] == inc["cand8"], inc
            assert inc["cand8"] == B.decide(stage8[i], k)["count"], (k, i, inc)
            er, ed = O.exact_search(mid, corpus, qs[i], k)
            assert int(c[0]) == k and np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32))
    idx.close()


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_near_duplicate_cluster_wider_than_the_list_goes_to_the_bfloat16_stage(metric):
    """20 000 near-copies of one unit vector at distances spread evenly over [0, 0.035]: the 8-bit interval (about +-0.006) keeps more
    than the list holds, the bfloat16 interval (about +-0.002) does not — both predicted here by the CPU models of the two stages — so the
    8-bit stage hands on and the bfloat16 stage answers (or hands on, if its model says so); the result is the exact scan's either way"""
    rng = np.random.default_rng(5)
    dim, n, k = 64, 20_000, 10
    c = rng.standard_normal(dim); c /= np.linalg.norm(c)
    u = rng.standard_normal((n, dim)); u -= np.outer(u @ c, c); u /= np.linalg.norm(u, axis=1)[:, None]
    dist = np.linspace(0.0, 0.035, n)
    along = (1.0 - dist) if metric == "dot" else np.ones(n)              # (dot: the distance is the component along the query itself)
    rows = (along[:, None] * c[None, :] + np.sqrt(2.0 * dist)[:, None] * u).astype(np.float32)
    q = c.astype(np.float32)
    mid = quiver_amd.metric_id(metric)
    m8 = B8.reference8(mid, B8.RowState8(rows), q, k)
    m16 = B.reference(mid, B.RowState(rows), q, k)
    assert m8["hand_back"] and m8["count"] > B.CAND_CAP, m8["count"]      # the shape is what it is built to be
    print("%s: 8-bit model keeps %d rows, bfloat16 model %d (hands on: %s)" % (metric, m8["count"], m16["count"], m16["hand_back"]))
    idx = quiver_amd.DeviceIndex(dim, metric); idx.add(rows)
    (r, d, _), inc = both(idx, q, k)
    assert inc["took8"] == 1 and inc["back8"] == 1 and inc["cand8"] == m8["count"], inc
    assert inc["took"] == 1 and inc["back"] == (1 if m16["hand_back"] else 0), inc
    if not m16["hand_back"]:
        assert inc["cand"] == m16["count"], (inc, m16["count"])
    er, ed = O.exact_search(mid, rows, q, k)
    assert np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32))
    # the control words are back in their initial state: an ordinary query behind it is answered by the 8-bit stage
    _, inc = both(idx, rng.standard_normal(dim).astype(np.float32), k)
    assert inc["took8"] == 1 and inc["took"] == 1
    idx.close()


def test_row_state_follows_updates_removes_and_growth():
    dim, n, k = 128, 12_000, 10
    rows = O.gen_rows(5200, 0, n, dim)
    idx = quiver_amd.DeviceIndex(dim, "cosine"); idx.add(rows)
    q = O.gen_rows(5201, 0, 1, dim)[0]
    (r0, _, _), inc = both(idx, q, k)
    assert answered_by_the_8bit_stage(inc)
    best = int(r0[0, 0])
    # overwrite a far row with a near-copy of the query at another scale: stale bytes, a stale scale or a stale residual would lose it
    far = int(O.exact_search(0, rows, -q, 1)[0][0])
    rows2 = rows.copy(); rows2[far] = (q * np.float32(37.5)).astype(np.float32)
    idx.update(far, rows2[far])
    (r, d, _), inc = both(idx, q, k)
    er, ed = O.exact_search(0, rows2, q, k)
    assert answered_by_the_8bit_stage(inc) and int(r[0, 0]) == far
    assert np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32))
    # ... and the other way: the best row overwritten by a far one
    rows2[best] = (-q * np.float32(0.01)).astype(np.float32)
    idx.update(best, rows2[best])
    alive = np.ones(n, bool)
    (r, d, _), inc = both(idx, q, k)
    er, ed = O.exact_search(0, rows2, q, k, alive=alive)
    assert answered_by_the_8bit_stage(inc) and np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32))
    # delete the best row
    idx.remove(np.array([far], np.uint32)); alive[far] = False
    (r, d, _), inc = both(idx, q, k)
    er, ed = O.exact_search(0, rows2, q, k, alive=alive)
    assert answered_by_the_8bit_stage(inc) and np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32))
    # a second add that grows the arrays (the capacity grows by half: three times the rows cannot fit), with the new best row in it
    more = O.gen_rows(5202, 0, 2 * n + 37, dim); more[-1] = (q * np.float32(1e-3)).astype(np.float32); more[5] = (q + np.float32(0.05) * more[5]).astype(np.float32)
    idx.add(more)
    rows3 = np.concatenate([rows2, more]); alive = np.concatenate([alive, np.ones(len(more), bool)])
    (r, d, _), inc = both(idx, q, k)
    er, ed = O.exact_search(0, rows3, q, k, alive=alive)
    assert answered_by_the_8bit_stage(inc) and int(r[0, 0]) == len(rows3) - 1
    assert np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32))
    idx.close()


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_undecidable_rows_are_candidates_and_the_exact_pass_decides_them(metric):
    """NaN, +-Inf, huge, vanishing and all-zero rows: always passed on, never in the threshold — no hand-back on their account"""
    dim = 128
    rng = np.random.default_rng(41)
    extreme = X.class_rows(rng, dim)
    rows = O.gen_rows(5300, 0, 8000, dim)
    placed = []
    for j, (cls, name, v) in enumerate(extreme):
        rows[(j * 397) % 8000] = v; placed.append((j * 397) % 8000)
    state = B8.RowState8(rows[placed])
    undecidable = int(np.isnan(state.res).sum())
    assert undecidable >= 4
    idx = quiver_amd.DeviceIndex(dim, metric); idx.add(rows)
    mid = quiver_amd.metric_id(metric)
    q = O.gen_rows(5301, 0, 1, dim)[0]
    for k in (1, 10, 64):
        (r, d, c), inc = both(idx, q, k)
        assert answered_by_the_8bit_stage(inc), inc
        assert k + undecidable <= inc["cand8"] + k - 1 and undecidable <= inc["cand8"] <= 4096, (inc, undecidable)
        er, ed = O.exact_search(mid, rows, q, k)
        assert np.array_equal(r[0], er) and X.same(d[0], ed)
    # queries the stage cannot quantise or whose norm it does not work with go on to the bfloat16 stage and from there to the exact scan
    for cls, name, v in extreme:
        _, inc = both(idx, v, 10)
        assert inc["took8"] == 1 and inc["took"] == 1
        if cls in "NZ" or name in ("norm2e+18", "norm1e+30"):
            assert inc["back8"] == 1 and inc["back"] == 1, (cls, name, inc)
    idx.close()


def test_declines():
    rows = O.gen_rows(87, 0, 5000, 100)                                    # 100 is no multiple of 16: no plane, no bound scan at all
    idx = quiver_amd.DeviceIndex(100, "cosine"); idx.add(rows)
    assert not idx.bound_scan8_stats()["plane"]
    _, inc = both(idx, rows[3], 10)
    assert inc["took8"] == 0 and inc["took"] == 0
    idx.close()
    rows = O.gen_rows(88, 0, 5000, 128)
    idx = quiver_amd.DeviceIndex(128, "cosine"); idx.add(rows[:7 * 64])   # fewer than 8 tiles
    assert idx.bound_scan8_stats()["plane"]
    (r, _, _), inc = both(idx, rows[3], 10)
    assert inc["took8"] == 0 and inc["took"] == 0 and int(r[0, 0]) == 3
    idx.close()
    for make in ("flag", "metric", "oom8", "bf16 mode"):
        if make == "oom8":
            os.environ["QV_TEST_PLANE8_OOM"] = "1"                         # the 8-bit plane's allocation answers out-of-memory: not an error
        try:
            idx = quiver_amd.DeviceIndex(128, "l2" if make == "metric" else "cosine", scan_plane=make != "flag")
            idx.add(rows)
        finally:
            os.environ.pop("QV_TEST_PLANE8_OOM", None)
        assert idx.bound_scan8_stats()["plane"] == (make == "bf16 mode")
        assert idx.bound_scan_stats()["plane"] == (make in ("oom8", "bf16 mode"))
        if make == "bf16 mode":
            idx.set_bound_scan("always"); idx.set_bound_plane("bf16")
            b0 = idx.bound_scan_stats()
            r, d, c = idx.search(rows[3], 10)
            assert idx.bound_scan8_stats()["searches"] == 0 and idx.bound_scan_stats()["searches"] == b0["searches"] + 1 and int(r[0, 0]) == 3
        else:
            (r, d, _), inc = both(idx, rows[3], 10)
            assert inc["took8"] == 0 and int(r[0, 0]) == 3
            assert inc["took"] == (1 if make == "oom8" else 0) and inc["back"] == 0          # without its plane the search runs on the bfloat16 copy
            if make == "oom8":
                er, ed = O.exact_search(0, rows, rows[3], 10)
                assert np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32))
        idx.close()


def test_sharded_handle():
    n, dim, k = 40_000, 128, 10
    rows = O.gen_rows(5400, 0, n, dim)
    one = quiver_amd.DeviceIndex(dim, "cosine"); one.add(rows); one.set_bound_scan("never")
    sh = quiver_amd.ShardedIndex(dim, "cosine", devices=[0, 0], peer_copy=True)
    gids = sh.add(rows)
    sh.set_bound_scan("always"); sh.set_bound_plane("8bit")
    assert sh.bound_scan8_stats()["plane"]
    q = O.gen_rows(5401, 0, 1, dim)[0]
    er, ed, _ = one.search(q, k)
    r, d, c = sh.search(q, k)
    assert int(c[0]) == k and np.array_equal(r[0], gids[er[0]]) and np.array_equal(d.view(np.uint32), ed.view(np.uint32))
    s8, s = sh.bound_scan8_stats(), sh.bound_scan_stats()
    assert s8["searches"] == 2 and s8["hand_backs"] == 0 and s["searches"] == 2 and s["hand_backs"] == 0
    sh.close(); one.close()
