"""The CPU model of the WIDE bound scan's stage 1 (65 <= k <= 1024; quiver_amd/csrc/qv_bound_scan.hip: bound_scan_tail_wide and the comment
above it, k_bound_collect_wide) and the corpora its survivor counts are pinned on: tests/test_gpu_bound_wide_counts.py runs them on the
device, tests/test_bound_wide_model_cpu.py proves on the CPU what they are built to be and that the counts tell a right kernel from a
wrong one.

The model restates the kernel's COMMENTS, not its code:

  ownership   four waves per workgroup; tile t belongs to wave t mod (4 * grid) (`plan`: plan_scan's grid, checked against the library's
              own workspace layout, whose region of published lists is grid * 4 * 64 keys)
  a list      the 64 smallest (ordered upper bound, row) keys among the LIVE rows of the wave's tiles; "live" is the call's candidate
              bitmap — alive rows, under a filter alive & selected.  A row the bound declines enters with whatever upper bound the
              library's interval function returns for it (NaN today: ordered above every number, so it takes a slot only where a wave
              has fewer than 64 rows the bound is sure of)
  H           the k-th smallest key of the union of the lists; none if fewer than k keys were published or that bound is not finite
  passed on   live rows with d_lo <= H, and the rows the bound declines

Where no wave's rows hold more than 64 of the k smallest upper bounds nothing is dropped and this is tests/_bound.decide; where one does,
H is looser and MORE rows pass — `dropped` says how many of the k smallest no list holds.  The interval arrays are the models' the suite
already pins at these widths (tests/_bound.stage1, tests/_bound_l2.stage1, tests/_widths.stage8_of).

The corpora are sized from the device's compute units (`sizes`): the smallest at which a wave owns two tiles, and three, so that list
inserts run in the wide instantiations, the second one against a threshold the first has moved.  A case is a Gaussian base and a few planted
rows, so the intervals of a base are computed once per metric and plane and a case's are patched in.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools

import numpy as np

from quiver_amd import _lib
from tests import _bound as B
from tests import _bound8 as B8
from tests import _bound_l2 as BL2
from tests import _widths as W

CAP = _lib.QV_BOUND_WIDE_CAND_CAP
COSINE, L2, DOT = 0, 1, 3
NAME = {COSINE: "cosine", L2: "l2", DOT: "dot"}
ARMS = ("bf16", "8bit")
WAVES, LIST_LEN = 4, 64                             # waves per workgroup; keys a wave publishes
REGION_CAP = 16
MAX_K = 1024                                        # the largest k of the form


# ---- the grid --------------------------------------------------------------------------------------------------------------------------
def plan(n_tiles, cus):
    """-> (grid, stride): workgroups of four waves, one tile per wave while two workgroups per CU suffice; beyond that 2 * cus workgroups,
    fewer where the shares come out even (only shares of 32 tiles or fewer are evened out).  stride = 4 * grid: wave w owns w, w + stride, ..."""
    cus = max(int(cus), 1)
    want, cap = -(-n_tiles // WAVES), 2 * cus
    grid = max(min(want, cap), 1)
    if want > cap:
        per = -(-n_tiles // (grid * WAVES))
        if per <= 32:
            grid = -(-(-(-n_tiles // per)) // WAVES)
    return grid, WAVES * grid


def library_regions(dim, rows, k, cus, metric=COSINE):
    """the region sizes of the wide form's workspace, as the library lays it out for `cus` compute units (tests/test_bound_scan_wide_cpu.layout)"""
    total, end, n = C.c_uint64(), C.c_uint64(), C.c_uint32()
    regs = (C.c_uint64 * (4 * REGION_CAP))()
    rc = _lib.lib().qv_scan_workspace_layout(_lib.QV_WS_BOUND_WIDE, metric, dim, rows, 1, k, cus, 0, C.byref(total), C.byref(end), C.byref(n), regs, REGION_CAP)
    assert rc == 0 and 0 < n.value <= REGION_CAP, (rc, n.value, _lib.lib().qv_last_error())
    return [int(regs[4 * i + 1]) for i in range(n.value)]


def lists_bytes(grid):
    return grid * WAVES * LIST_LEN * 8


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def ordered(x):
    """the ordered word of a float32: ascending as the numbers are, -0 as +0, every NaN one word above +inf's and below the dead key's"""
    x = np.array(x, np.float32)
    nan = np.isnan(x)
    x[x == 0] = 0.0
    u = x.view(np.uint32)
    o = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    o[nan] = 0xFFFFFFFE
    return o


def _keys(hi, rows):
    return (ordered(hi[rows]).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)


def published(lo, hi, unsure, live, n_tiles, grid, list_len=LIST_LEN, blocks=False):
    """the union of the waves' lists, sorted: uint64 keys (ordered d_hi << 32 | row).  (lo and unsure play no part: a declined row's key is
    made of the d_hi the interval function gave it.)  list_len, blocks: the faults tests/test_bound_wide_model_cpu.py plants — a shorter
    list; contiguous blocks of tiles per wave in place of the stride"""
    rows = np.flatnonzero(np.asarray(live, bool))
    assert n_tiles == -(-len(hi) // 64)
    keys = _keys(hi, rows)
    waves = WAVES * grid
    wave = (rows // 64) // (-(-n_tiles // waves)) if blocks else (rows // 64) % waves
    order = np.lexsort((keys, wave))
    ws = wave[order]
    rank = np.arange(len(ws)) - np.searchsorted(ws, ws, side="left")
    return np.sort(keys[order][rank < list_len])


def decide_wide(stage, k, live, n_tiles, grid, cap=CAP, key_live=None, list_len=LIST_LEN, blocks=False, rank=None, lists=None):
    """what tests/_bound.decide returns, for the wide form: H (None: there is none), passed, count, hand_back — and `dropped`, how many of
    the k smallest upper bounds no list holds.  key_live (the rows that get a key, `live` by default), list_len, blocks and rank (the place H
    is taken at, k by default) are the planted faults' handles; lists: `the_lists` of the same arguments, where a caller keeps them over
    several k."""
    lo, hi, unsure = stage["lo"], stage["hi"], stage["unsure"]
    live = np.asarray(live, bool)
    pub, smallest = lists if lists is not None else the_lists(stage, live if key_live is None else key_live, n_tiles, grid, list_len, blocks)
    at = k if rank is None else rank
    H = None
    if len(pub) >= at:
        h = hi[int(pub[at - 1] & np.uint64(0xFFFFFFFF))]
        H = h if np.isfinite(h) else None
    with np.errstate(invalid="ignore"):
        passed = live & (unsure | (lo <= (H if H is not None else np.float32(-np.inf))))
    count = int(passed.sum())
    dropped = int(len(smallest[:k]) - np.isin(smallest[:k], pub).sum())
    hand_back = H is None or count > cap or not B.query_ok(stage["qn"], stage["dim"])
    return dict(stage, H=H, passed=passed, count=count, hand_back=hand_back, dropped=dropped)


def the_lists(stage, key_live, n_tiles, grid, list_len=LIST_LEN, blocks=False):
    """(the published keys, the MAX_K smallest keys of all keyed rows): all of decide_wide that does not depend on k"""
    key_live = np.asarray(key_live, bool)
    pub = published(stage["lo"], stage["hi"], stage["unsure"], key_live, n_tiles, grid, list_len, blocks)
    keys = _keys(stage["hi"], np.flatnonzero(key_live))
    return pub, np.sort(keys if len(keys) <= MAX_K else np.partition(keys, MAX_K)[:MAX_K])


def stage_of(metric, arm, rows, q):
    """the interval of every row of `rows` for q on one arm, from the models the suite trusts"""
    if arm == "8bit":
        return W.stage8_of(metric, B8.RowState8(rows), q)
    st = B.RowState(rows)
    return BL2.stage1(st, q) if metric == L2 else B.stage1(metric, st, q)


# ---- the corpora -----------------------------------------------------------------------------------------------------------------------
def sizes(cus):
    """(rows at which every wave owns two tiles, ... three): the last tile ragged"""
    return 2 * 8 * cus * 64 - 37, 3 * 8 * cus * 64 - 37


#        name: (tiles per wave, dim, seed) — the first seed of 81xx, 82xx, ... for which tests/test_bound_wide_model_cpu.py's conditions hold at 256
#        compute units (two64: the seventh; on the others H at rank k + 1 moved a count at the first)
BASES = {"two": (2, 16, 8102), "three": (3, 16, 8103), "two64": (2, 64, 8764), "two_l2": (2, 16, 8116)}
KS_PLAIN = (65, 129, 500, 1024)
KS_LOOSE = (65, 100, 129, 500)


@functools.lru_cache(maxsize=None)
def base(name, cus):
    """-> (Gaussian rows [n, dim], the query)"""
    per, dim, seed = BASES[name]
    n = sizes(cus)[per - 2]
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(dim).astype(np.float32)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    rows.setflags(write=False); q.setflags(write=False)
    n_tiles = -(-n // 64)
    assert plan(n_tiles, cus) == (2 * cus, 8 * cus) and n_tiles == per * 8 * cus, (name, cus, plan(n_tiles, cus))
    return rows, q


@functools.lru_cache(maxsize=None)
def base_stage(name, cus, metric, arm):
    rows, q = base(name, cus)
    return stage_of(metric, arm, rows, q)


def wave_rows(wave, per, cus):
    """the row numbers of every tile of one wave, ascending"""
    return np.concatenate([np.arange(64) + 64 * (wave + j * 8 * cus) for j in range(per)])


def near(q, m, seed):
    """m rows next to the query, as tests/test_gpu_bound_scan_wide.py makes them: q + 0.05 * noise"""
    noise = np.random.default_rng(seed).standard_normal((m, q.size)).astype(np.float32)
    return (q[None, :] + np.float32(0.05) * noise).astype(np.float32)


def far(q, m, seed):
    noise = np.random.default_rng(seed).standard_normal((m, q.size)).astype(np.float32)
    return (-q[None, :] + np.float32(0.5) * noise).astype(np.float32)


def _second_tiles(n, cus):
    return (np.arange(n) // 64) >= 8 * cus


@functools.lru_cache(maxsize=None)
def case(name, cus):
    """-> dict(base, metric, ks, loose, at / vecs: the rows planted into the base, removed, upd_at / upd_vecs: rows overwritten by
    update_rows after the removal, select: the filter's rows or None, unfiltered_first: an unfiltered wide search runs in front)"""
    c = {"name": name, "metric": COSINE, "ks": KS_PLAIN, "loose": False, "at": None, "vecs": None, "removed": None, "upd_at": None,
         "upd_vecs": None, "select": None, "unfiltered_first": False, "same_count_ks": ()}
    kind, _, tail = name.partition("/")
    bname = c["base"] = tail or ("two_l2" if kind.startswith("l2_") else "two")
    per, dim, seed = BASES[bname]
    rows, q = base(bname, cus)
    n = len(rows)
    w0 = 5 * cus + 3                                                      # a wave in the middle of the grid, clear of the ragged tile
    assert w0 + 77 < 8 * cus - 1, cus
    mine = wave_rows(w0, per, cus)
    if kind in ("plain", "l2_plain"):
        pass
    elif kind in ("loose_one", "l2_loose_one", "loose_tombstones", "filtered_loose"):
        c.update(loose=True, ks=KS_LOOSE, at=mine, vecs=near(q, len(mine), seed + 10))     # the 128 (192) nearest fill every tile of one wave
    elif kind == "loose_many":
        at = np.concatenate([wave_rows(w0 + 11 * j, per, cus) for j in range(8)])
        c.update(loose=True, ks=(1024, 500), at=at, vecs=near(q, len(at), seed + 11))      # the 1 024 nearest fill both tiles of eight waves
        # At k = 500 keys are dropped as well (a wave holds more than 64 of the 500 smallest), but the looser H still lies inside the cluster,
        # whose 1 024 rows all have d_lo = 0: either H passes exactly the cluster.  Strictly more survivors at k = 1024 only.
        c["same_count_ks"] = (500,)
    elif kind == "loose_ties":
        at = np.random.default_rng(seed + 12).permutation(mine)[:70]
        c.update(loose=True, ks=(65, 129), at=np.sort(at), vecs=np.repeat(near(q, 1, seed + 12), 70, axis=0))   # 70 copies of one near row
    elif kind == "filtered_second":
        c.update(select=_second_tiles(n, cus) & (np.random.default_rng(seed + 13).random(n) < 0.5))
    elif kind == "filtered_sparse":
        c.update(select=(np.arange(n) // 64) % 25 == 0, unfiltered_first=True)
    else:
        raise KeyError(name)
    if kind.startswith("l2_"):
        c["metric"] = L2
    if kind == "plain" and bname == "three":
        c["metric"] = DOT
    if kind == "loose_tombstones":
        rng = np.random.default_rng(seed + 14)
        p = rng.permutation(mine)
        # ... and the 20 nearest rows of the other waves: keyed by mistake, THEY would lower H (a dead row of the full wave only takes the
        # slot of a row that was dropped anyway)
        r64, q64 = rows.astype(np.float64), q.astype(np.float64)
        cos = (r64 @ q64) / np.linalg.norm(r64, axis=1)
        cos[mine] = -np.inf
        removed = np.concatenate([p[:30], np.argsort(-cos)[:20]])
        c.update(removed=np.sort(removed).astype(np.uint32), upd_at=np.sort(p[30:40]).astype(np.uint32), upd_vecs=far(q, 10, seed + 15))
    if kind == "filtered_loose":
        sel = np.random.default_rng(seed + 16).random(n) < 0.25
        sel[mine] = True
        c.update(select=sel)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


#: every pinned corpus of tests/test_gpu_bound_wide_counts.py ("name/base"; the base is "two" where none is named)
UNFILTERED = ("plain", "plain/three", "loose_one", "loose_one/three", "loose_many/two64", "loose_tombstones", "loose_ties", "l2_plain", "l2_loose_one")
FILTERED = ("filtered_second", "filtered_sparse", "filtered_loose")
CASES = UNFILTERED + FILTERED


def rows_before(c, cus):
    """the rows the index is built from (a fresh array: the planted rows in the base)"""
    rows = base(c["base"], cus)[0].copy()
    if c["at"] is not None:
        rows[c["at"]] = c["vecs"]
    return rows


def rows_after(c, cus):
    """... and what it holds once update_rows has run"""
    rows = rows_before(c, cus)
    if c["upd_at"] is not None:
        rows[c["upd_at"]] = c["upd_vecs"]
    return rows


def alive_of(c, cus):
    alive = np.ones(len(base(c["base"], cus)[0]), bool)
    if c["removed"] is not None:
        alive[c["removed"]] = False
    return alive


def live_of(c, cus):
    """the call's candidate bitmap"""
    alive = alive_of(c, cus)
    return alive if c["select"] is None else alive & c["select"]


@functools.lru_cache(maxsize=None)
def case_stage(name, cus, arm):
    """the intervals of the case's rows as the index holds them at search time: the base's, the planted and the overwritten rows' patched in"""
    c = case(name, cus)
    q = base(c["base"], cus)[1]
    st = base_stage(c["base"], cus, c["metric"], arm)
    out = dict(st, lo=st["lo"].copy(), hi=st["hi"].copy(), unsure=st["unsure"].copy())
    for at, vecs in ((c["at"], c["vecs"]), (c["upd_at"], c["upd_vecs"])):
        if at is not None:
            sub = stage_of(c["metric"], arm, vecs, q)
            assert sub["qn"] == st["qn"]
            for f in ("lo", "hi", "unsure"):
                out[f][at] = sub[f]
    for f in ("s", "isum"):
        out.pop(f, None)                                                  # (not patched, not used)
    return out


@functools.lru_cache(maxsize=64)
def _case_lists(name, cus, arm, fault):
    c = case(name, cus)
    n = len(base(c["base"], cus)[0])
    n_tiles = -(-n // 64)
    f = dict(fault)
    everything = np.ones(n, bool) if c["select"] is None else c["select"]
    key_live = {None: live_of(c, cus), "dead too": everything, "unselected too": alive_of(c, cus)}[f.get("key_live")]
    return the_lists(case_stage(name, cus, arm), key_live, n_tiles, plan(n_tiles, cus)[0], f.get("list_len", LIST_LEN), f.get("blocks", False))


def model(name, cus, arm, k, **fault):
    """decide_wide for one pinned case; fault: one of `faults`' values"""
    c = case(name, cus)
    n = len(base(c["base"], cus)[0])
    n_tiles = -(-n // 64)
    lists = _case_lists(name, cus, arm, tuple(sorted(fault.items())))
    return decide_wide(case_stage(name, cus, arm), k, live_of(c, cus), n_tiles, plan(n_tiles, cus)[0], lists=lists,
                       rank=k + 1 if fault.get("rank") == "k + 1" else None)


def exact_model(name, cus, arm, k):
    """tests/_bound.decide over the same rows: the count an exact k-th smallest upper bound leaves (against the wide form's capacity)"""
    c = case(name, cus)
    return B.decide(case_stage(name, cus, arm), k, alive=live_of(c, cus), cap=CAP)


def faults(name, cus):
    """the faults of the model a pinned case must tell from the right kernel: name -> decide_wide's arguments.  Which wave owns a tile and
    how long its list is can show only where a wave holds 64 or more of the k smallest upper bounds — the loose cases; on Gaussian rows
    every ownership rule and a list of 63 publish all of them and leave the same H, so the other cases are not asked for those two."""
    c = case(name, cus)
    out = {"rank k + 1": {"rank": "k + 1"}}
    if c["loose"]:
        out.update({"blocks": {"blocks": True}, "list of 63": {"list_len": 63}})
    if c["removed"] is not None:
        out["dead rows keyed"] = {"key_live": "dead too"}
    if c["select"] is not None:
        out["unselected rows keyed"] = {"key_live": "unselected too"}
    return out


# ---- the planted row above 64 results -----------------------------------------------------------------------------------------------------
PLANTED = tuple((metric, dim, k) for metric in (COSINE, DOT) for dim in (16, 240) for k in (65, 129))
