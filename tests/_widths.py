"""The inputs of the bound scan's width tests, built once and shared: tests/test_gpu_bound_scan_widths.py runs them on the device,
tests/test_bound_widths_cpu.py proves on the CPU that they can tell a right kernel from a wrong one.

Every bound-scan kernel (quiver_amd/csrc/qv_bound_scan.hip) walks a row in steps of 16 dimensions through a binary ladder of unrolled blocks:
bound_tile and k_bound_scan_mq's loop take blocks of 8 (looped), 4, 2 and 1 steps, bound8_tile blocks of 16 (looped), 8, 4, 2 and 1.  WIDTHS
reaches every block alone and in company, and both ends of the ladder at the limit of 4096 dimensions:

  dim    steps   bound_tile / k_bound_scan_mq     bound8_tile
  32       2     2                                2
  64       4     4                                4
  112      7     4 + 2 + 1                        4 + 2 + 1
  240     15     8 + 4 + 2 + 1                    8 + 4 + 2 + 1
  496     31     3 x 8 + 4 + 2 + 1                16 + 8 + 4 + 2 + 1
  4080   255     31 x 8 + 4 + 2 + 1               15 x 16 + 8 + 4 + 2 + 1
  4096   256     32 x 8                           16 x 16

(16 dimensions, the 1-step block alone, and 128, the 8-step block alone, are the existing GPU tests'; 64 is here because the only tests that
ran the 4-step block alone were the near-duplicate clusters, which end in a hand-back.)

What the device reports of stage 1 is the survivor COUNT, so the CPU model here (tests/_bound.py, tests/_bound8.py: the library's own interval
functions over a restated sum) predicts that count for every query, k and filter, and the sums can be recomputed with one ladder block's
contribution left out (`skip`): tests/test_bound_widths_cpu.py asserts that each such fault changes a count the device test compares.  The
seeds are the first for which that holds at every width.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools

import numpy as np

from quiver_amd import _lib
from tests import _bound as B
from tests import _bound8 as B8
from tests import _oracle as O

WIDTHS = (32, 64, 112, 240, 496, 4080, 4096)
N = 2051                                            # 33 tiles: 9 workgroups of four waves, the last tile holds 3 rows
KS = (1, 10, 64)
SINGLE = (0, 1, 2)                                  # the queries the single-query forms run
NQS = (2, 4, 5, 8)                                  # shared passes: QB = 4 and 8, each part-filled and full
SET_NQS = (4, 8)                                    # passes with a set per query
LADDER, LADDER8 = (8, 4, 2, 1), (16, 8, 4, 2, 1)
# corpus seed per width (queries: seed + 1, tombstones and sets: seed + 2): the first of 7000 + dim, 7000 + dim + 10000, ... for which every
# left-out block changes a compared count, for both metrics (tests/test_bound_widths_cpu.py::test_every_ladder_block_changes_a_count)
SEEDS = {32: 7032, 64: 7064, 112: 7112, 240: 7240, 496: 7496, 4080: 11080, 4096: 11096}


def blocks(dim, ladder):
    """the blocks a walk of `ladder` takes over dim / 16 steps: [(block size, first dimension, one past its last)], the looped block once per turn"""
    steps, s, out = dim // 16, 0, []
    while s + ladder[0] <= steps:
        out.append((ladder[0], 16 * s, 16 * (s + ladder[0]))); s += ladder[0]
    for u in ladder[1:]:
        if s + u <= steps:
            out.append((u, 16 * s, 16 * (s + u))); s += u
    assert s == steps
    return out


def left_out(dim, ladder):
    """one (first dimension, one past the last) per block size the walk uses; of the looped block its LAST turn, the smallest fault of that size"""
    return {u: (d0, d1) for u, d0, d1 in blocks(dim, ladder)}


@functools.lru_cache(maxsize=None)
def case(dim):
    """-> dict(seed, rows [N, dim], qs [8, dim], dead, live [N] bool, mask (search_masked's), masks: 8 of (bool [N] or None))"""
    seed = SEEDS[dim]
    rows = O.gen_rows(seed, 0, N, dim)
    qs = O.gen_rows(seed + 1, 0, 8, dim)
    rng = np.random.default_rng(seed + 2)
    dead = np.unique(np.concatenate([rng.integers(0, N, 40), [64 * 7, N - 2]])).astype(np.uint32)     # tombstones, one in the ragged tile
    live = np.ones(N, bool); live[dead] = False
    tile = np.arange(N) // 64
    mask = (tile % 3 != 1) & (rng.random(N) < 0.5)                        # every third tile empty: the skipping form skips
    masks = []
    for j in range(8):
        if j == 6:
            masks.append(None)                                            # no filter
            continue
        m = rng.random(N) < (0.5, 0.25, 0.12, 1.0)[j % 4]
        if j == 3:
            m &= tile % 2 == 0                                            # whole tiles, every other one
        m &= (tile != 5) & (tile != 20)                                   # two tiles no query of a pass of four selects
        masks.append(m)
    for a in (rows, qs, dead, live, mask, *[m for m in masks if m is not None]):
        a.setflags(write=False)
    return {"seed": seed, "rows": rows, "qs": qs, "dead": dead, "live": live, "mask": mask, "masks": masks}


def alive_of(live, mask):
    return live if mask is None else live & mask


@functools.lru_cache(maxsize=None)
def state(dim):
    return B.RowState(case(dim)["rows"])


@functools.lru_cache(maxsize=None)
def state8(dim):
    return B8.RowState8(case(dim)["rows"])


def chain32_queries(qs, rh, skip=None):
    """tests/_bound.chain32_rows for every query at once -> [nq, n]: one float32 rounding per step; the dimensions in `skip` = (first, one past
    the last) contribute nothing (a ladder block that was not walked)"""
    q64 = np.asarray(qs, np.float32).astype(np.float64)
    r64 = np.ascontiguousarray(np.asarray(rh, np.float32).T).astype(np.float64)
    acc = np.zeros((q64.shape[0], r64.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        for i in range(r64.shape[0]):
            if skip is not None and skip[0] <= i < skip[1]:
                continue
            acc = (q64[:, i, None] * r64[None, i, :] + acc.astype(np.float64)).astype(np.float32)
    return acc


@functools.lru_cache(maxsize=None)
def sums(dim, skip=None):
    return chain32_queries(case(dim)["qs"], state(dim).rh, skip)


@functools.lru_cache(maxsize=None)
def stage1(metric, dim, qi, skip=None):
    """tests/_bound.stage1 for query qi of the width's case (the sums shared among the queries and the metrics)"""
    st = state(dim)
    qn = B.chain_norm(case(dim)["qs"][qi])
    s = sums(dim, skip)[qi]
    unsure, lo, hi = B.intervals(metric, dim, s, qn, st.rn, st.rres)
    return {"s": s, "lo": lo, "hi": hi, "unsure": unsure, "qn": qn, "dim": dim}


def stage8_of(metric, st8, q, skip=None):
    """the 8-bit stage's interval of every row for one query, as tests/_bound8.reference8 computes it; the dimensions in `skip` left out of the
    integer sum"""
    q = np.ascontiguousarray(q, np.float32)
    n, dim = st8.rows.shape
    qn = B.chain_norm(q)
    qq, _, _, sq, qres = B8.quantize_query(q)
    qq = qq.copy()
    if skip is not None:
        qq[skip[0]:skip[1]] = 0
    isums = st8.r8.astype(np.int64) @ qq
    fn = _lib.lib().qv_scan_bound_interval8
    lo, hi = C.c_float(0), C.c_float(0)
    out_lo, out_hi, unsure = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, bool)
    for i in range(n):
        rc = fn(metric, dim, int(isums[i]), sq, qn, qres, float(st8.rn[i]), C.c_float(st8.scale[i]), C.c_float(st8.res[i]), C.byref(lo), C.byref(hi))
        assert rc in (0, 1)
        unsure[i] = rc == 1; out_lo[i] = lo.value; out_hi[i] = hi.value
    return {"isum": isums, "lo": out_lo, "hi": out_hi, "unsure": unsure, "qn": qn, "dim": dim}


@functools.lru_cache(maxsize=None)
def stage8(metric, dim, qi, skip=None):
    return stage8_of(metric, state8(dim), case(dim)["qs"][qi], skip)


def model(metric, dim, qi, k, alive, skip=None):
    """the bfloat16 stage's decision for query qi over `alive` (tests/_bound.decide): dict(H, passed, count, hand_back, ...)"""
    return B.decide(stage1(metric, dim, qi, skip), k, alive=alive)


def model8(metric, dim, qi, k, alive, skip=None):
    """the 8-bit stage's (threshold, survivors and hand-back follow the same rule from its own intervals)"""
    return B.decide(stage8(metric, dim, qi, skip), k, alive=alive)


@functools.lru_cache(maxsize=None)
def oracle(metric, dim, qi, k, which):
    """O.exact_search for query qi over `which`: "live", "mask" (search_masked's bitmap) or "set" (the query's own set)"""
    c = case(dim)
    alive = {"live": c["live"], "mask": c["live"] & c["mask"], "set": alive_of(c["live"], c["masks"][qi])}[which]
    return O.exact_search(metric, c["rows"], c["qs"][qi], k, alive=alive.astype(np.uint8))


def counts(metric, dim, skip=None):
    """every survivor count the device test compares, per form of the bfloat16 walk: one number per (query, k) for the single-query forms, the
    LARGEST among a pass's queries per (nq, k) for the shared forms, as the device reports them"""
    c = case(dim)
    live = c["live"]
    cnt = lambda j, k, alive: model(metric, dim, j, k, alive, skip)["count"]
    return {
        "single": tuple(cnt(j, k, live) for j in SINGLE for k in KS),
        "masked": tuple(cnt(j, k, live & c["mask"]) for j in SINGLE for k in KS),
        "shared": tuple(max(cnt(j, k, live) for j in range(nq)) for nq in NQS for k in KS),
        "sets": tuple(max(cnt(j, k, alive_of(live, c["masks"][j])) for j in range(nq)) for nq in SET_NQS for k in KS),
    }


def counts8(metric, dim, skip=None):
    return tuple(model8(metric, dim, j, k, case(dim)["live"], skip)["count"] for j in SINGLE for k in KS)


# ---- saturated operands of the 8-bit stage at 4096 dimensions ------------------------------------------------------------------------------
SAT_DIM, SAT_N, SAT_SEED = 4096, 2051, 7900
SAT_PLUS, SAT_MINUS = (70, 64 * 9 + 63, 2050), (3, 64 * 20, 1999)       # rows along the query's signs and against them


@functools.lru_cache(maxsize=None)
def saturated():
    """A query whose elements quantise to hi = +-127, lo = 0 in the dimensions that k_bound_scan8 adds into its FIRST partial sum (elements
    0 - 3 and 8 - 11 of every step of 16) and to hi = 0, lo = +-64 in the others, and rows whose bytes are all +-127 with the query's signs
    (SAT_PLUS, at three scales) or against them (SAT_MINUS), among ordinary rows: the largest partial sums the stage can meet —
    2048 * 127 * 127 in one int32, and 128 times that, beyond int32, once the two terms are combined.
    -> dict(rows, q, live, dead, hi, lo: the query's split)"""
    rng = np.random.default_rng(SAT_SEED)
    m = np.float32(B8.QMAX * 2.0 ** -14)                                  # the scale is 2^-14 exactly
    sign = np.where(rng.random(SAT_DIM) < 0.5, -1.0, 1.0)
    big = (np.arange(SAT_DIM) % 8) < 4
    q = (sign * np.where(big, m, np.float32(64 * 2.0 ** -14))).astype(np.float32)
    rows = O.gen_rows(SAT_SEED, 0, SAT_N, SAT_DIM).copy()
    for i, c in zip(SAT_PLUS, (1 / 64, 1 / 80, 1 / 128)):
        rows[i] = (sign * c).astype(np.float32)
    for i, c in zip(SAT_MINUS, (1 / 64, 1 / 80, 1 / 128)):
        rows[i] = (-sign * c).astype(np.float32)
    dead = np.array([5, 64 * 9, 1000], np.uint32)
    live = np.ones(SAT_N, bool); live[dead] = False
    _, hi, lo, _, _ = B8.quantize_query(q)
    for a in (rows, q, live, dead):
        a.setflags(write=False)
    return {"rows": rows, "q": q, "live": live, "dead": dead, "hi": hi, "lo": lo, "big": big, "sign": sign}


@functools.lru_cache(maxsize=None)
def saturated_stage8(metric):
    c = saturated()
    return stage8_of(metric, B8.RowState8(c["rows"]), c["q"])


@functools.lru_cache(maxsize=None)
def saturated_stage1(metric):
    c = saturated()
    return B.stage1(metric, B.RowState(c["rows"]), c["q"])
