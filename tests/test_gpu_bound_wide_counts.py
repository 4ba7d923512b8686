"""The wide form of the single-query bound scan (65 <= k <= 1024; bound_scan_tail_wide, k_bound_collect_wide: quiver_amd/csrc/qv_bound_scan.hip)
on corpora where a wave owns SEVERAL tiles — two and three, sized from the device's compute units — so that the list inserts of the wide
instantiations run, and with the nearest rows stored in the tiles of one wave, so that a wave holds more of the k smallest upper bounds than
the 64 it publishes and H comes out looser than the exact k-th smallest.  Results go through the exact re-score, so rows and bits alone show
a wrong stage 1 only if it happens to reject a true neighbour; here the survivor COUNT of every search must also EQUAL the CPU model's
(tests/_wide.py) on both arms — an H one rank off, a list one key short, another ownership of the tiles, a keyed dead or unselected row
each change a count compared here (tests/test_bound_wide_model_cpu.py proves it, case by case).  Every search is compared, rows, counts and
float32 bits, with the exact path of the same index and with the CPU oracle; the wide form's own counters say that it answered."""
import functools

import numpy as np
import pytest

import quiver_amd
from quiver_amd.device_index import device_info
from tests import _bound as B
from tests import _bound8 as B8
from tests import _extremes as X
from tests import _oracle as O
from tests import _tight as T
from tests import _wide as Wd
from tests import _widths as W

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def cus():
    return int(device_info(0)["cus"])


def build(c):
    """the case's index as it stands at search time -> (index, its rows then, the query)"""
    rows = Wd.rows_before(c, cus())
    idx = quiver_amd.DeviceIndex(rows.shape[1], Wd.NAME[c["metric"]], l2_scan_plane=(c["metric"] == Wd.L2))
    idx.add(rows)
    if c["removed"] is not None:
        idx.remove(c["removed"])
    if c["upd_at"] is not None:
        idx.update_rows(c["upd_at"], c["upd_vecs"])
    assert idx.bound_scan_wide_stats()["plane"] and idx.bound_scan8_stats()["plane"]
    return idx, Wd.rows_after(c, cus()), Wd.base(c["base"], cus())[1]


def delta(s0, s1):
    return {"took": s1["searches"] - s0["searches"], "back": s1["hand_backs"] - s0["hand_backs"], "cand": s1["candidates"]}


def is_oracle(res, want, k):
    (r, d, n), (er, ed) = res, want
    return int(n[0]) == k == len(er) and np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32))


def same(a, b):
    return bool(np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]) and X.same(a[1], b[1]))


def pinned(name, arm, k, inc, took=1, entry="search"):
    """the counters of one wide search against the model: answered, and the survivors are the model's, to the row"""
    m = Wd.model(name, cus(), arm, k)
    print("%s %s %s k %d: survivors %d, the model %d (an exact H would leave %d; %d of the k smallest bounds in no list)"
          % (name, entry, arm, k, inc["cand"], m["count"], Wd.exact_model(name, cus(), arm, k)["count"], m["dropped"]))
    assert not m["hand_back"] and (m["dropped"] > 0) == Wd.case(name, cus())["loose"], (name, arm, k, m["dropped"])
    assert inc["took"] == took and inc["back"] == 0, (name, arm, k, inc)
    assert inc["cand"] == m["count"], (name, arm, k, inc, m["count"])


@pytest.mark.parametrize("name", Wd.UNFILTERED)
def test_unfiltered_survivors_are_the_models(name):
    """plain: Gaussian rows, two and three tiles per wave — nothing is dropped and the count is the exact threshold's.  loose_one: the 128
    (192) nearest rows fill every tile of one wave; at k = 65 and 100 that wave holds more than k rows of the answer and publishes 64.
    loose_many (64 dimensions): the 1 024 nearest fill both tiles of eight waves, half of them published.  loose_tombstones: 30 of the 128
    removed, 10 overwritten with far vectors, the 20 nearest rows of the other waves removed too — a dead row takes no slot, an overwritten
    one enters with its new bounds.  loose_ties: 70 copies of one near row in one wave's tiles, the 64 smaller row numbers published.
    l2_*: a Euclidean index with the scan planes, both arms pinned (tests/_widths.stage8_of models its 8-bit interval)."""
    c = Wd.case(name, cus())
    idx, rows, q = build(c)
    alive = Wd.alive_of(c, cus())
    for k in c["ks"]:
        want = O.exact_search(c["metric"], rows, q, k, alive=alive.astype(np.uint8))
        idx.set_bound_scan_wide("never")
        s0 = idx.bound_scan_wide_stats()
        exact = idx.search(q, k)
        assert idx.bound_scan_wide_stats()["searches"] == s0["searches"] and is_oracle(exact, want, k), (name, k)
        for arm in Wd.ARMS:
            idx.set_bound_scan_wide("always"); idx.set_bound_plane(arm)
            s0 = idx.bound_scan_wide_stats()
            got = idx.search(q, k)
            inc = delta(s0, idx.bound_scan_wide_stats())
            assert same(got, exact), (name, arm, k)
            pinned(name, arm, k, inc)
    if c["removed"] is not None:
        assert not np.isin(got[0][0], c["removed"]).any()
    idx.close()


@pytest.mark.parametrize("name", Wd.FILTERED)
def test_filtered_survivors_are_the_models(name):
    """on the two-tile corpus, through search_rowsets and search_masked.  filtered_second: the set selects rows of second tiles only — the first
    tile a wave READS is not the first it owns.  filtered_sparse: one tile in 25 holds a candidate, most waves read nothing and publish a dead
    list; the search runs directly behind an unfiltered wide search of the same query on the same index and workspace, whose lists hold
    smaller keys — a stale list would lower H.  filtered_loose: the loose one-wave case inside a set of every row of that wave and one
    row in four elsewhere."""
    c = Wd.case(name, cus())
    idx, rows, q = build(c)
    live = Wd.live_of(c, cus())
    rs = idx.rowset(c["select"])
    calls = {"search_rowsets": lambda k: idx.search_rowsets(q, k, rs), "search_masked": lambda k: idx.search_masked(q, k, c["select"])}
    for k in c["ks"]:
        want = O.exact_search(c["metric"], rows, q, k, alive=live.astype(np.uint8))
        for entry, call in calls.items():
            idx.set_bound_scan_wide_filtered("never"); idx.set_bound_scan_wide("never")
            s0 = idx.bound_scan_wide_stats()
            exact = call(k)
            assert idx.bound_scan_wide_stats()["searches"] == s0["searches"] and is_oracle(exact, want, k), (name, entry, k)
            for arm in Wd.ARMS:
                idx.set_bound_scan_wide_filtered("always"); idx.set_bound_plane_filtered(arm)
                s0 = idx.bound_scan_wide_stats()
                if c["unfiltered_first"]:
                    idx.set_bound_scan_wide("always"); idx.set_bound_plane(arm)
                    idx.search(q, k)                                     # its lists stay in the workspace; nothing but the host call in between
                got = call(k)
                inc = delta(s0, idx.bound_scan_wide_stats())
                assert same(got, exact), (name, entry, arm, k)
                pinned(name, arm, k, inc, took=2 if c["unfiltered_first"] else 1, entry=entry)
    rs.close(); idx.close()


@pytest.mark.parametrize("metric,dim,k", Wd.PLANTED)
def test_the_planted_row_above_64_results(metric, dim, k):
    """tests/_tight.planted at k = 65 and 129: r*, the row that needs the whole margin, is the k-th result on both arms, the wide form answers,
    and the survivors are the model's — one tile per wave here, so tests/_bound.decide's as well"""
    case = T.planted(metric, dim, k)
    er, ed, count = T.conditions(case, cap=Wd.CAP)
    rows, q = case["rows"], case["q"]
    n = len(rows); n_tiles = -(-n // 64)
    grid, stride = Wd.plan(n_tiles, cus())
    assert stride >= n_tiles
    stages = {"bf16": B.stage1(metric, B.RowState(rows), q), "8bit": W.stage8_of(metric, B8.RowState8(rows), q)}
    idx = quiver_amd.DeviceIndex(dim, Wd.NAME[metric]); idx.add(rows)
    idx.set_bound_scan_wide("never")
    exact = idx.search(q, k)
    assert is_oracle(exact, (er, ed), k)
    for arm in Wd.ARMS:
        m = Wd.decide_wide(stages[arm], k, np.ones(n, bool), n_tiles, grid)
        e = B.decide(stages[arm], k, cap=Wd.CAP)
        assert m["count"] == e["count"] and m["dropped"] == 0 and not m["hand_back"] and (arm != "bf16" or m["count"] == count)
        idx.set_bound_scan_wide("always"); idx.set_bound_plane(arm)
        s0 = idx.bound_scan_wide_stats()
        got = idx.search(q, k)
        inc = delta(s0, idx.bound_scan_wide_stats())
        print("planted metric %d dim %d k %d %s: survivors %d, the model %d" % (metric, dim, k, arm, inc["cand"], m["count"]))
        assert same(got, exact) and int(got[0][0][k - 1]) == case["target"], (arm, got[0][0][-3:], case["target"])
        assert inc["took"] == 1 and inc["back"] == 0 and inc["cand"] == m["count"], (arm, inc, m["count"])
    idx.close()
