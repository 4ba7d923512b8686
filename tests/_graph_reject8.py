"""The level-0 walk of tests/_graph_reject.py with the 8-bit image's certificate (quiver_amd/csrc/qv_hnsw.hip, "a hop that rejects on the
row-order 8-bit image"): which evaluations are made in hops that start with a full result list (A), which of those the exact distance rejects
(R), and which the 8-bit interval certifies (C8) — from the EXACT integer sum RowState8.r8 @ qq, the stored scale and residual, and the
library's own qv_scan_bound_interval8.  The integer sum is exact on the device too, so C8 is what the kernel must reject, to the row.
TEST / MEASUREMENT INFRASTRUCTURE ONLY."""
import bisect
import ctypes as C

import numpy as np

from quiver_amd import _lib
from tests import _bound as B
from tests import _bound8 as B8
from tests import _oracle as O


def lower_ends8(metric, state8, q, rows_idx):
    """(unsure [n], d_lo [n] float32) of the listed rows under query q; a query the quantiser declines: every row unsure"""
    rows_idx = np.asarray(rows_idx, np.int64)
    q = np.ascontiguousarray(q, np.float32)
    dim = state8.rows.shape[1]
    qn = B.chain_norm(q)
    qz = B8.quantize_query(q)
    n = rows_idx.size
    unsure, out = np.ones(n, bool), np.full(n, -np.inf, np.float32)
    if qz is None:
        return unsure, out
    qq, _, _, sq, qres = qz
    isums = state8.r8[rows_idx].astype(np.int64) @ qq
    fn = _lib.lib().qv_scan_bound_interval8
    lo, hi = C.c_float(0), C.c_float(0)
    for j in range(n):
        i = int(rows_idx[j])
        rc = fn(metric, dim, int(isums[j]), sq, qn, qres, float(state8.rn[i]), C.c_float(state8.scale[i]), C.c_float(state8.res[i]), C.byref(lo), C.byref(hi))
        assert rc in (0, 1)
        unsure[j] = rc == 1; out[j] = lo.value
    return unsure, out


def walk8(metric, rows, state8, deg, links, entry, q, ef, d32=None):
    """one query's level-0 walk, GR.walk's bookkeeping.  -> dict: evals, A, R, C8 (rows of full-list hops whose certified lower end is not below the worst
    distance their hop STARTED with), ties, order, full_rows"""
    n = rows.shape[0]
    if d32 is None:
        d32 = O.all_distances(metric, rows, q)
    dl = d32.astype(np.float64).tolist()
    lst = [(dl[entry], entry)]
    expanded, visited = set(), {entry}
    evals, A, R = 1, 0, 0
    full_rows, full_w = [], []
    ties = False
    while True:
        cur = next((e for e in lst if e[1] not in expanded), None)
        if cur is None:
            break
        expanded.add(cur[1])
        new = []
        for c in links[cur[1], :min(int(deg[cur[1]]), links.shape[1])].tolist():
            if c < n and c not in visited:
                visited.add(c); new.append(c)
        if not new:
            continue
        evals += len(new)
        full = len(lst) >= ef
        if full:
            A += len(new)
            full_rows += new; full_w += [lst[ef - 1][0]] * len(new)
        for c in new:
            d = dl[c]
            if d != d:
                ties = True
            if len(lst) >= ef and not d < lst[ef - 1][0]:
                R += 1 if full else 0
                ties |= d == lst[ef - 1][0]
                continue
            bisect.insort(lst, (d, c))
            if len(lst) > ef:
                w = lst[ef - 1][0]
                while len(lst) > ef and lst[-1][0] > w:
                    lst.pop()
    C8 = 0
    if full_rows:
        unsure, lo = lower_ends8(metric, state8, q, full_rows)
        C8 = int(np.sum(~unsure & (lo.astype(np.float64) >= np.asarray(full_w, np.float64))))
    return {"evals": evals, "A": A, "R": R, "C8": C8, "order": lst[:ef], "ties": ties, "full_rows": full_rows}
