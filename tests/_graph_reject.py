"""The level-0 walk of HNSW.searchLayer (pkg/hnsw/hnsw.go:471-580) restated in Python for the tests and the measurement of the graph's
rejecting hops (quiver_amd/csrc/qv_hnsw.hip, "a hop that rejects on the row-order bfloat16 copy"): which evaluations are made in hops that
start with a full result list (A), which of those the exact distance rejects at their turn (R), and which the bound scan's interval
certifies from the bfloat16 image (C).  Single-layer graphs (levels 0), the list model of the wave kernel: no two equal distances may
decide anything (the caller's corpus has none; `ties` says if one did).  TEST / MEASUREMENT INFRASTRUCTURE ONLY."""
import bisect

import numpy as np

from tests import _bound as B
from tests import _oracle as O


def gamma(dim):
    """bound_scan_gamma (qv_bound.h)"""
    g = (dim + 2) * 2.0 ** -24
    return g / (1.0 - g) * (1.0 + 1e-6) + 5e-7 + 1e-12


def margin(dim, qn, rn, rres):
    """the margin of bound_scan_interval (qv_bound.h), in float64"""
    rr = np.asarray(rres, np.float64)
    return qn * (rr + gamma(dim) * (np.asarray(rn, np.float64) + rr)) * (1.0 + 1e-9)


def lower_ends(metric, state, q, qn, rows_idx, margins):
    """the library's own lower end (qv_scan_bound_interval) of the listed rows when S is the float64 dot with the bfloat16 image and the
    margin is taken `margins` times.  The interval function adds ONE margin to the sum it is given, so it is handed a float32 at or
    above S + (margins - 1) m: the end it answers is at or below the one a kernel whose chain is within one margin of S derives."""
    rows_idx = np.asarray(rows_idx, np.int64)
    dim = state.rows.shape[1]
    s = state.rh[rows_idx].astype(np.float64) @ np.asarray(q, np.float32).astype(np.float64)
    m = margin(dim, qn, state.rn[rows_idx], state.rres[rows_idx])
    s32 = (s + (margins - 1) * m).astype(np.float32)
    if margins > 1:
        s32 = np.nextafter(s32, np.float32(np.inf))                        # (the rounding to float32 may have gone down)
    unsure, lo, _ = B.intervals(metric, dim, s32, qn, state.rn[rows_idx], state.rres[rows_idx])
    return unsure, lo


def walk(metric, rows, state, deg, links, entry, q, ef, margins=2):
    """one query's level-0 walk.  -> dict: evals (the entry point's included, once: what evals_out holds), A, R, C (certified at `margins` margins), C1 (at one),
    order (the result list as (distance, node), ascending), ties (an equal distance met a decision), full_rows (the rows evaluated in hops
    that started with a full list)"""
    n = rows.shape[0]
    d32 = O.all_distances(metric, rows, q)                                 # the reference's float32 distance to every row
    dl = d32.astype(np.float64).tolist()
    lst = [(dl[entry], entry)]                                             # ascending (distance, node); `expanded` beside it
    expanded = set()
    visited = {entry}
    evals, A, R = 1, 0, 0                                                  # (the entry point's evaluation counts, as the device counts it)
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
        for c in new:                                                      # admissions in adjacency order (:553-560)
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
    C = C1 = 0
    if full_rows:
        qn = B.chain_norm(np.asarray(q, np.float32))
        w = np.asarray(full_w, np.float64)
        unsure, lo = lower_ends(metric, state, q, qn, full_rows, margins)
        C = int(np.sum(~unsure & (lo.astype(np.float64) >= w)))
        unsure1, lo1 = lower_ends(metric, state, q, qn, full_rows, 1)
        C1 = int(np.sum(~unsure1 & (lo1.astype(np.float64) >= w)))
    return {"evals": evals, "A": A, "R": R, "C": C, "C1": C1, "order": lst[:ef], "ties": ties, "full_rows": full_rows}
