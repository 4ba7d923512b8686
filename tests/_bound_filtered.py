"""The inputs of the filtered bound scan's tests, built once and shared: tests/test_gpu_bound_scan_filtered.py runs them on the device,
tests/test_bound_scan_filtered_cpu.py derives on the CPU (tests/_bound.py's model over alive = live & set) which query of each case has
a threshold H, how many rows survive it, and so how many queries the device must hand back.  The GPU file states those numbers as
literals; the CPU file proves them.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

from tests import _bound as B
from tests import _oracle as O

N = 20_011                                          # a ragged last tile
DENSITIES = (1.0, 0.5, 0.1, 0.02, 0.005)            # 0.5 % of 20 011 is about 100 rows: every set holds 64 live rows or more (checked on the CPU)
NQS = (1, 2, 3, 4, 5, 7, 8)
KS = (1, 10, 63, 64)
CUS = 256                                           # compute units of the device the first-read-tile case is laid out for (MI355X)


def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


# ---- 1. basic shapes ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def basic(metric, dim):
    """-> dict(rows, qs [8], live [N] bool, dead (the removed rows), masks: 8 of (bool [N] or None))"""
    rows = O.gen_rows(6100 + dim, 0, N, dim)
    qs = O.gen_rows(6101 + dim, 0, 8, dim)
    rng = np.random.default_rng(6102 + dim + metric)
    dead = np.unique(rng.integers(0, N, 300)).astype(np.uint32)
    live = np.ones(N, bool); live[dead] = False
    masks = []
    for q in range(8):
        if q == 2:
            masks.append(None)                                            # no filter
            continue
        if q == 3:
            m = (np.arange(N) // 64) % 5 == 1                             # four tiles of five unselected
        else:
            m = rng.random(N) < DENSITIES[q % len(DENSITIES)]
        if q == 4:
            m[dead[:32]] = True                                           # selecting a tombstoned row selects nothing
        masks.append(m)
    _ro(rows, qs, live, dead, *masks)
    return {"rows": rows, "qs": qs, "live": live, "dead": dead, "masks": masks}


def alive_of(live, mask):
    return live if mask is None else live & mask


@functools.lru_cache(maxsize=None)
def _state(key):
    kind, *args = key
    return B.RowState(CASES[kind](*args)["rows"])


@functools.lru_cache(maxsize=None)
def _stage1(key, qi):
    kind, *args = key
    c = CASES[kind](*args)
    return B.stage1(c["metric"] if "metric" in c else args[0], _state(key), c["qs"][qi])


def model(key, qi, k, alive):
    """tests/_bound.py's decision for query qi of a case over `alive`: dict(H, count, hand_back, ...)"""
    return B.decide(_stage1(key, qi), k, alive=alive)


# ---- 2. sets with fewer than k candidates --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def short(metric):
    """a pass of four at k = 10, dim 128: an empty set, a set of 5 live rows (and 3 dead ones), two ordinary sets"""
    dim = 128
    rows = O.gen_rows(6200, 0, N, dim)
    qs = O.gen_rows(6201, 0, 4, dim)
    rng = np.random.default_rng(6202)
    dead = np.arange(1000, 1200, dtype=np.uint32)
    live = np.ones(N, bool); live[dead] = False
    empty = np.zeros(N, bool)
    five = np.zeros(N, bool); five[[3, 64 * 7 + 63, 9000, 15_555, N - 1]] = True; five[[1000, 1100, 1199]] = True
    masks = [rng.random(N) < 0.5, empty, rng.random(N) < 0.1, five]
    _ro(rows, qs, live, dead, *masks)
    return {"rows": rows, "qs": qs, "live": live, "dead": dead, "masks": masks, "metric": metric}


# ---- 3. stale lower bounds ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stale(metric):
    """queries that are copies of rows in tiles t % 3 != 0 (the unfiltered answers lie there), sets that select only tiles t % 3 == 0"""
    dim = 128
    rows = O.gen_rows(6300, 0, N, dim)
    at = np.array([64 * 1 + 5, 64 * 2 + 9, 64 * 100 + 1, 64 * 200 + 63], dtype=np.int64)   # tiles 1, 2, 100, 200: none a multiple of 3
    qs = rows[at].copy()
    tile = np.arange(N) // 64
    rng = np.random.default_rng(6301)
    stripe = tile % 3 == 0
    masks = [stripe.copy(), stripe & (rng.random(N) < 0.5), stripe & (tile % 2 == 0), stripe & (rng.random(N) < 0.2)]
    live = np.ones(N, bool)
    _ro(rows, qs, live, *masks)
    return {"rows": rows, "qs": qs, "live": live, "masks": masks, "at": at, "metric": metric}


# ---- 4. the first tile a wave reads is not the first it owns ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def second_tile(metric, cus=CUS):
    """2 x 8 x cus tiles at dim 128: every wave owns tiles w and w + 8 cus; the sets select rows of the second ones only"""
    dim = 128
    n = 2 * 8 * cus * 64 - 37
    rows = O.gen_rows(6400, 0, n, dim)
    qs = O.gen_rows(6401, 0, 8, dim)
    tile = np.arange(n) // 64
    rng = np.random.default_rng(6402)
    second = tile >= 8 * cus
    masks = [second & (rng.random(n) < (1.0, 0.5, 0.25, 0.1)[j % 4]) for j in range(8)]
    live = np.ones(n, bool)
    _ro(rows, qs, live, *masks)
    return {"rows": rows, "qs": qs, "live": live, "masks": masks, "metric": metric}


# ---- 6. search_masked -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def masked(metric):
    dim = 128
    rows = O.gen_rows(6600, 0, N, dim)
    qs = O.gen_rows(6601, 0, 8, dim)
    rng = np.random.default_rng(6602)
    dead = np.arange(500, 700, dtype=np.uint32)
    live = np.ones(N, bool); live[dead] = False
    masks = [rng.random(N) < 0.5, rng.random(N) < 0.02]
    _ro(rows, qs, live, dead, *masks)
    return {"rows": rows, "qs": qs, "live": live, "dead": dead, "masks": masks, "metric": metric}


# ---- 8. a hand-back inside a set ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clusters(metric):
    """tests/test_gpu_bound_scan_mq.py's cluster corpus (64 dims, 3 x 20 000 near-copies + 20 000 independent rows), four queries, each with
    a 50 % set; query 1 sits on a centre"""
    rng = np.random.default_rng(3)
    dim, per = 64, 20_000
    centres = rng.standard_normal((3, dim)).astype(np.float32)
    rows = np.concatenate([c + 1e-5 * rng.standard_normal((per, dim)).astype(np.float32) for c in centres] + [rng.standard_normal((per, dim)).astype(np.float32)])
    qs = rng.standard_normal((4, dim)).astype(np.float32)
    qs[1] = (centres[1] + 1e-5 * rng.standard_normal(dim)).astype(np.float32)
    n = rows.shape[0]
    masks = [rng.random(n) < 0.5 for _ in range(4)]
    live = np.ones(n, bool)
    _ro(rows, qs, live, *masks)
    return {"rows": rows, "qs": qs, "live": live, "masks": masks, "metric": metric}


# ---- 7. the tight corpus under a filter ------------------------------------------------------------------------------------------------
TIGHT_DIMS, TIGHT_KS = (16, 128), (1, 10)
TIGHT_WIDE = ((240, 1), (240, 10), (2048, 10))      # (dim, k) of tests/_tight.PLANTED_WIDE: every block of the step ladder; the widest gamma the construction holds at


@functools.lru_cache(maxsize=None)
def tight(metric, dim, k):
    """tests/_tight.planted's corpus; the planted query's set is exactly {r*, the k - 1 nearer rows, the competitor band} (`exact`), then
    the same without the BEST competitor — the band row with the smallest upper bound (`omit`; `band_omit` = the band that is left):
    H moves to the next competitor's upper bound.  Three ordinary queries with ordinary sets fill the pass of four."""
    from tests import _tight as T
    case = T.planted(metric, dim, k)
    rows, q = case["rows"], case["q"]
    n = rows.shape[0]
    exact = np.zeros(n, bool)
    exact[case["target"]] = True; exact[case["near"]] = True; exact[case["band"]] = True
    st1 = B.stage1(metric, B.RowState(rows), q)
    band = np.asarray(case["band"])
    best = int(band[np.argmin(st1["hi"][band])])
    omit = exact.copy(); omit[best] = False
    rng = np.random.default_rng(7000 + dim + k + metric)
    others = rng.standard_normal((3, dim)).astype(np.float32)
    other_masks = [rng.random(n) < 0.5 for _ in range(3)]
    _ro(exact, omit, others, *other_masks)
    return {"case": case, "exact": exact, "omit": omit, "best": best, "band_omit": band[band != best], "others": others, "other_masks": other_masks, "n": n}


def tight_pass(t, slot, planted_mask):
    """(queries [4, dim], masks [4]) with the planted query in `slot`"""
    qs = [t["others"][0], t["others"][1], t["others"][2]]
    ms = list(t["other_masks"])
    qs.insert(slot, np.asarray(t["case"]["q"])); ms.insert(slot, planted_mask)
    return np.stack(qs).astype(np.float32), ms


CASES = {"basic": basic, "short": short, "stale": stale, "second_tile": second_tile, "masked": masked, "clusters": clusters}


def backs(key, nq, k, masks=None):
    """how many of the first nq queries of a case the model hands back at k, query j over live & masks[j]"""
    kind, *args = key
    c = CASES[kind](*args)
    masks = c["masks"] if masks is None else masks
    return sum(bool(model(key, j, k, alive_of(c["live"], masks[j]))["hand_back"]) for j in range(nq))


def oracle(key, qi, k, alive):
    kind, *args = key
    c = CASES[kind](*args)
    metric = c["metric"] if "metric" in c else args[0]
    return O.exact_search(metric, c["rows"], c["qs"][qi], k, alive=alive.astype(np.uint8))
