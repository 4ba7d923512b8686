"""The 8-bit stage in front of a shared pass of 2 - 8 queries (k_bound_scan8_mq, quiver_amd/csrc/qv_bound_scan.hip) without a GPU: the rule
that puts it there (qv_scan_bound8_applies_mq) over the grid of tests/test_flat_route_cpu.py, that nothing the library decided before has
moved, and the kernel's PRE-TEST certified on the inputs the device test runs: a row whose lower bound lies strictly above the wave's
current k-th upper bound is skipped before its upper bound is computed, and that must change neither H nor the survivors."""
import itertools

import numpy as np
import pytest

import quiver_amd
from quiver_amd import _lib
from tests import _route as R
from tests import _widths as W
from tests._route import ALWAYS, AUTO, NEVER, NO_FILTER
from tests.test_flat_route_cpu import DIMS, KS, METRICS, MODES, NQS, ROWS

COS, DOT = R.M["cosine"], R.M["dot"]
# AUTO's floors (rows), stated once: profiles/LAB_r12_bound_scan8_mq.md.  (dim class, QB) -> the smallest row count taken, None = never automatic
FLOORS = {(768, 4): 3_000_000, (768, 8): 3_000_000, (128, 4): 10_000_000, (128, 8): None}


def rule(metric, dim, rows, nq, k, mode, plane_mode_mq, has_plane8):
    rc = _lib.lib().qv_scan_bound8_applies_mq(metric, dim, rows, nq, k, mode, plane_mode_mq, has_plane8)
    assert rc in (0, 1), rc
    return bool(rc)


def bound_applies(metric, dim, rows, nq, k, mode):
    rc = _lib.lib().qv_scan_bound_applies(metric, dim, rows, nq, k, mode, 1)
    assert rc in (0, 1), rc
    return bool(rc)


def test_the_rule_on_the_route_grid():
    taken = 0
    for metric, dim, rows, nq, k in itertools.product(METRICS, DIMS, ROWS, NQS, KS):
        for mode, pmode, plane8 in itertools.product(MODES, MODES, (0, 1)):
            got = rule(metric, dim, rows, nq, k, mode, pmode, plane8)
            base = bound_applies(metric, dim, rows, nq, k, mode)
            args = (metric, dim, rows, nq, k, mode, pmode, plane8)
            if got:
                taken += 1
                assert base, args                                         # never where the bound scan would not take the pass
                assert metric in (COS, DOT) and 2 <= nq <= 8 and k <= 64 and dim % 16 == 0 and dim <= 4096 and (rows + 63) // 64 >= 8, args
                assert plane8 and pmode != NEVER and mode != NEVER, args
            if pmode == ALWAYS:                                           # "8bit": whenever those hold
                assert got == (base and 2 <= nq <= 8 and bool(plane8)), args
            if nq in (1, 9) or not plane8 or pmode == NEVER:
                assert not got, args
    assert taken > 0
    assert quiver_amd.scan_bound8_applies_mq("cosine", 768, 10_000_000, 4, 10, "always", "8bit") is True
    assert quiver_amd.scan_bound8_applies_mq("cosine", 768, 10_000_000, 4, 10, "always", "bf16") is False
    assert quiver_amd.scan_bound8_applies_mq("l2", 768, 10_000_000, 4, 10, "always", "8bit") is False
    assert _lib.lib().qv_scan_bound8_applies_mq(COS, 768, 10_000_000, 4, 10, 3, AUTO, 1) < 0
    assert _lib.lib().qv_scan_bound8_applies_mq(COS, 768, 10_000_000, 4, 10, AUTO, 3, 1) < 0


@pytest.mark.parametrize("dim", [128, 256, 768, 1024])
@pytest.mark.parametrize("nq", [2, 3, 4, 5, 6, 7, 8])
def test_auto_takes_the_pass_from_its_floor_on(dim, nq):
    floor = FLOORS[768 if dim >= 768 else 128, 4 if nq <= 4 else 8]
    for k in (1, 10, 64):
        if floor is None:
            assert not any(rule(COS, dim, rows, nq, k, AUTO, AUTO, 1) for rows in (300_000, 1_000_000, 3_000_000, 10_000_000, 100_000_000)), (dim, nq, k)
            continue
        assert rule(COS, dim, floor, nq, k, AUTO, AUTO, 1) and rule(DOT, dim, floor, nq, k, AUTO, AUTO, 1), (dim, nq, k)
        assert not rule(COS, dim, floor - 1, nq, k, AUTO, AUTO, 1), (dim, nq, k)
        assert rule(COS, dim, floor, nq, k, ALWAYS, AUTO, 1)                # the bound scan forced on: the plane's own floor still decides
        assert not rule(COS, dim, floor - 1, nq, k, ALWAYS, AUTO, 1)
        assert bound_applies(COS, dim, floor, nq, k, AUTO)                  # never below the bound scan's own floor for that nq
    assert not rule(COS, 112, 100_000_000, nq, 10, AUTO, AUTO, 1)           # narrower than 128 dimensions: never automatic
    assert rule(COS, 112, 100_000, nq, 10, ALWAYS, ALWAYS, 1)


def test_nothing_the_library_decided_before_has_moved():
    for nq in range(2, 9):
        for pmode in MODES:
            assert _lib.lib().qv_scan_bound8_applies(COS, 768, 10_000_000, nq, 10, ALWAYS, pmode, 1) == 0
    shapes = ((768, 10_000_000, 4, 10), (768, 1_000_000, 8, 64), (128, 10_000_000, 2, 1), (768, 300_000, 5, 10), (16, 600, 4, 10), (768, 20_011, 4, 10))
    for dim, rows, nq, k in shapes:
        for bmode, pmode in itertools.product(MODES, MODES):
            args = (COS, dim, rows, nq, k, 1, bmode, pmode, 1, 1, NO_FILTER)
            got = R.library_route(*args)
            assert got == R.expected_route(*args), args
            for pf in MODES:
                assert _lib.lib().qv_scan_route_ex(COS, dim, rows, nq, k, R.CUS, 1, bmode, pmode, 1, 1, NO_FILTER, pf) == got, (args, pf)
    assert R.library_route(COS, 768, 10_000_000, 4, 10, 1, AUTO, AUTO, 1, 1, NO_FILTER) == R.BOUND_MQ    # the plane is a decision inside route 1


# ---- the pre-test ----------------------------------------------------------------------------------------------------------------------
def ord_f32(x):
    """the kernels' ordered image of a float32 (qv_kernels.h): NaN after +inf, -0 as +0"""
    x = np.ascontiguousarray(x, np.float32).copy()
    nan = np.isnan(x)
    x[x == 0] = 0.0
    u = x.view(np.uint32).astype(np.uint64)
    o = np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)
    o[nan] = 0xFFFFFFFE
    return o


def walk(lo, hi, live, k, waves):
    """k_bound_scan8_mq's walk of one query: tile t belongs to wave t % waves, a wave takes its tiles in rising order, the first one sorted
    outright; before every later tile the wave's k-th smallest key so far is its threshold.  -> (skipped [n] bool: rows whose lower bound's
    word lies strictly above the threshold's distance word, the keys every wave kept)"""
    n = len(lo)
    olo, ohi = ord_f32(lo), ord_f32(hi)
    key = (ohi << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    skipped = np.zeros(n, bool)
    kept = []
    tiles = (n + 63) // 64
    for w in range(min(waves, tiles)):
        mine = np.empty(0, np.uint64)
        for i, t in enumerate(range(w, tiles, waves)):
            rows = np.arange(t * 64, min(n, t * 64 + 64))
            rows = rows[live[rows]]
            if i > 0 and len(mine) >= k:
                thr = np.sort(mine)[k - 1]
                skip = olo[rows] > (thr >> np.uint64(32))
                assert (key[rows][skip] > thr).all()                      # the list would have rejected every one of them
                skipped[rows[skip]] = True
                rows = rows[~skip]
            mine = np.sort(np.concatenate([mine, key[rows]]))[:k]
        kept.append(mine)
    return skipped, np.concatenate(kept) if kept else np.empty(0, np.uint64)


@pytest.mark.parametrize("metric", [COS, DOT])
@pytest.mark.parametrize("dim", W.WIDTHS)
def test_the_pre_test_changes_neither_H_nor_the_survivors(metric, dim):
    """per query and k, under the launch's own share of tiles (36 waves for 33 tiles: every wave sorts its one tile, nothing is skipped) and
    under the shares of a long corpus (4 waves, 1 wave: 8 and 33 tiles behind one another)"""
    c = W.case(dim)
    live = c["live"]
    fired = 0
    for j in range(max(W.NQS)):
        st = W.stage8(metric, dim, j)
        for k in W.KS:
            m = W.model8(metric, dim, j, k, live)
            for waves in (36, 4, 1):
                skipped, kept = walk(st["lo"], st["hi"], live, k, waves)
                fired += int(skipped.sum())
                assert not (skipped & st["unsure"]).any()                 # d_lo = -inf is never above a threshold
                assert not (skipped & m["passed"]).any(), (j, k, waves)
                if m["H"] is not None:
                    assert (st["hi"][skipped] > m["H"]).all(), (j, k, waves)   # no skipped row's upper bound is below the final H
                    Hk = np.sort(kept)[k - 1]
                    assert int(Hk >> np.uint64(32)) == int(ord_f32(np.array([m["H"]], np.float32))[0]), (j, k, waves)
                    passed = live & (st["unsure"] | (ord_f32(st["lo"]) <= (Hk >> np.uint64(32))))
                    assert np.array_equal(passed, m["passed"]), (j, k, waves)
                if waves == 36:
                    assert not skipped.any()
    assert fired > 0                                                      # the walks of several tiles per wave did skip rows
