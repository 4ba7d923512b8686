"""Stage 1 of the 8-bit bound scan (k_bound_scan8, quiver_amd/csrc/qv_bound_scan.hip) at the shapes where its walk can go wrong: a wave owns the
tiles t0, t0 + waves, ... and walks each in blocks of 16 / 8 / 4 / 2 / 1 steps; the filtered form holds one candidate word ahead.  Here: few
tiles, one tile fewer than / as many as / more than the launch has waves, widths that are and are not whole blocks, a ragged last tile, a
dead last tile, an index filled to exactly its reserved capacity, and masks that leave a wave few tiles to read.

Every case forces the bound scan "always" and the plane "8bit", compares rows and float32 bits with the exact scan of the SAME index and
with the CPU oracle, requires the counters to say that the 8-bit stage answered, and requires stage 1's survivor count to equal the CPU
model's (tests/_bound8.py's intervals through tests/_widths.stage8_of)."""
import functools
import types

import numpy as np
import pytest

import quiver_amd
from quiver_amd.device_index import device_info
from tests import _bound as B
from tests import _bound8 as B8
from tests import _extremes as X
from tests import _oracle as O
from tests import _route as R
from tests import _widths as W

pytestmark = pytest.mark.gpu

K = 10


def both(idx, call, filtered=False):
    """one call through the 8-bit stage and through the exact scan of the same index -> (result, counters' increments)"""
    idx.set_bound_scan("always")
    if filtered:
        idx.set_bound_plane_filtered("8bit")
    else:
        idx.set_bound_plane("8bit")
    a0, b0 = idx.bound_scan8_stats(), idx.bound_scan_stats()
    r, d, c = call()
    a1, b1 = idx.bound_scan8_stats(), idx.bound_scan_stats()
    idx.set_bound_scan("never")
    er, ed, ec = call()
    assert idx.bound_scan8_stats()["searches"] == a1["searches"] and idx.bound_scan_stats()["searches"] == b1["searches"]   # "never" is never
    assert np.array_equal(c, ec) and np.array_equal(r, er), (r, er)
    assert X.same(d, ed), (d, ed)
    inc = {"took8": a1["searches"] - a0["searches"], "back8": a1["hand_backs"] - a0["hand_backs"], "cand8": a1["candidates"],
           "took": b1["searches"] - b0["searches"], "back": b1["hand_backs"] - b0["hand_backs"], "cand": b1["candidates"]}
    return (r, d, c), inc


def answered_by_the_8bit_stage(inc):
    return inc["took8"] == 1 and inc["back8"] == 0 and inc["took"] == 1 and inc["back"] == 0


def waves_at_the_cap():
    return device_info(0)["cus"] * 2 * 4                       # plan_scan: two workgroups of four waves per CU


@functools.lru_cache(maxsize=None)
def corpus(dim, n):
    """rows, a query and the 8-bit row state of one width, computed once for the largest shape; smaller shapes are its prefixes"""
    rows = O.gen_rows(9300 + dim, 0, n, dim)
    return rows, O.gen_rows(9301 + dim, 0, 1, dim)[0], B8.RowState8(rows)


def prefix(state, n):
    return types.SimpleNamespace(rows=state.rows[:n], r8=state.r8[:n], scale=state.scale[:n], res=state.res[:n], rn=state.rn[:n])


def run_case(metric, dim, rows, q, state, alive=None, dead=None, reserve=False):
    n = len(rows)
    mid = quiver_amd.metric_id(metric)
    want = B.decide(W.stage8_of(mid, state, q), K, alive)
    assert not want["hand_back"] and K <= want["count"] <= B.CAND_CAP, want["count"]   # the shape is one the stage answers
    idx = quiver_amd.DeviceIndex(dim, metric)
    if reserve:
        idx.reserve(n)
    idx.add(rows)
    if dead is not None:
        idx.remove(dead)
    assert idx.bound_scan8_stats()["plane"] and idx.bound_scan_stats()["plane"]
    (r, d, c), inc = both(idx, lambda: idx.search(q, K))
    idx.close()
    assert answered_by_the_8bit_stage(inc), inc
    assert inc["cand8"] == want["count"] and inc["cand"] == inc["cand8"], (inc, want["count"])
    er, ed = O.exact_search(mid, rows, q, K) if alive is None else O.exact_search(mid, rows, q, K, alive=alive.astype(np.uint8))
    assert int(c[0]) == K and np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32))


# steps per tile: 1, 3, 8, 16, 17 (a block of 16 and one of 1) and 48 (three blocks of 16)
@pytest.mark.parametrize("tiles", [8, 9])
@pytest.mark.parametrize("dim", [16, 48, 128, 256, 272, 768])
def test_few_tiles_with_a_ragged_last_tile(dim, tiles):
    n = (tiles - 1) * 64 + 37
    rows, q, state = corpus(dim, 8 * 64 + 37)
    for metric in ("cosine", "dot"):
        run_case(metric, dim, rows[:n], q, prefix(state, n))


# the launch's wave count against the tile count: a wave without a tile, one each, some with two, all with two or three
@pytest.mark.parametrize("shape", ["waves-1", "waves", "waves+1", "2waves+1"])
@pytest.mark.parametrize("dim", [64, 128])
def test_tile_counts_around_the_wave_count(dim, shape):
    w = waves_at_the_cap()
    tiles = {"waves-1": w - 1, "waves": w, "waves+1": w + 1, "2waves+1": 2 * w + 1}[shape]
    n = (tiles - 1) * 64 + 21
    rows, q, state = corpus(dim, 2 * w * 64 + 21)
    grid = R.scan_grid(tiles, device_info(0)["cus"])
    assert (grid * 4 >= tiles) == (shape in ("waves-1", "waves")), (grid, tiles)   # at most one tile a wave, or not
    run_case("cosine", dim, rows[:n], q, prefix(state, n))


@pytest.mark.parametrize("dim", [64, 768])
def test_last_tile_without_a_live_row(dim):
    """the last, ragged tile's rows are all removed: its words are dead, its rows never candidates, and the tile before it is the last with an answer"""
    tiles = 37
    n = (tiles - 1) * 64 + 29
    rows, q, state = corpus(dim, 36 * 64 + 29)
    alive = np.ones(n, bool); alive[(tiles - 1) * 64:] = False
    run_case("cosine", dim, rows, q, state, alive=alive, dead=np.arange((tiles - 1) * 64, n, dtype=np.uint32))


@pytest.mark.parametrize("dim", [128, 272])
def test_index_filled_to_exactly_its_reserved_capacity(dim):
    """nothing lies behind the last tile's rows but what the index itself pads: a request past the wave's last tile would leave the arrays"""
    for tiles in (9, 40):
        n = (tiles - 1) * 64 + 37
        rows, q, state = corpus(dim, 39 * 64 + 37)
        run_case("cosine", dim, rows[:n], q, prefix(state, n), reserve=True)


@pytest.mark.parametrize("which", ["every third tile", "one wave's last tile"])
def test_masked_search(which):
    """the filtered form (one candidate word ahead): every third tile a candidate, and a mask that leaves only the last tile
    of one wave's share"""
    dim, w = 128, waves_at_the_cap()
    tiles, n = 2 * w + 1, 2 * w * 64 + 21                      # (test_tile_counts_around_the_wave_count's largest corpus: every wave has two or three tiles)
    rows, q, state = corpus(dim, n)
    mid = quiver_amd.metric_id("cosine")
    tile = np.arange(n) // 64
    waves = R.scan_grid(tiles, device_info(0)["cus"]) * 4
    assert waves < tiles
    if which == "every third tile":
        mask = tile % 3 == 0
    else:
        mask = tile == max(t for t in range(tiles) if t % waves == 1)
    want = B.decide(W.stage8_of(mid, state, q), K, mask)
    assert not want["hand_back"] and K <= want["count"] <= B.CAND_CAP
    idx = quiver_amd.DeviceIndex(dim, "cosine"); idx.add(rows)
    (r, d, c), inc = both(idx, lambda: idx.search_masked(q, K, mask), filtered=True)
    idx.close()
    assert answered_by_the_8bit_stage(inc), inc
    assert inc["cand8"] == want["count"], (inc, want["count"])
    er, ed = O.exact_search(mid, rows, q, K, alive=mask.astype(np.uint8))
    assert int(c[0]) == K and np.array_equal(r[0], er) and np.array_equal(d[0].view(np.uint32), ed.view(np.uint32))
