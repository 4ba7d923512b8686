"""Shared restatements behind the bound scan's tests (quiver_amd/csrc/qv_bound.h, k_row_residual, k_bf16_plane): the bfloat16 rounding,
the float32 chain of stage 1, the float64 norm chain, the residual rounded up, and the library's own interval function compiled for the
host (qv_scan_bound_interval) — one row at a time as tests/test_bound_scan_cpu.py uses them, and over all rows of a corpus at once
(`*_rows`, `reference`) for the tests that predict what the device must keep, pass on and hand back.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from quiver_amd import _lib
from tests import _oracle as O

COSINE, DOT = 0, 3
CAND_CAP = 4096                                    # kBoundCandCap (qv_bound_scan.hip): more survivors than this and the exact scan answers


def bf16(x):
    """round to nearest even, as the device's conversion (finite values; NaN and Inf pass through)"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    keep = ~np.isfinite(x)
    r[keep] = b[keep] & 0xFFFF0000
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def chain32(q, rh):
    """the float32 fma chain in element order (a product of 24 x 8 bits is exact in float64; one rounding to float32 per step)"""
    acc = np.float32(0.0)
    with np.errstate(all="ignore"):
        for a, b in zip(q.astype(np.float64), rh.astype(np.float64)):
            acc = np.float32(a * b + np.float64(acc))
    return acc


def chain32_rows(q, rh):
    """chain32 of one query against every row of rh [n, dim] at once: a loop over dim, one float32 rounding per step"""
    rh = np.asarray(rh, np.float32)
    acc = np.zeros(rh.shape[0], np.float32)
    with np.errstate(all="ignore"):
        for i, a in enumerate(np.asarray(q, np.float32).astype(np.float64)):
            acc = (a * rh[:, i].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def chain_norm(v):
    s = 0.0
    with np.errstate(all="ignore"):
        for a in v.astype(np.float64):
            s = a * a + s                     # exact product of float32 values: fma == multiply-add
        return float(np.sqrt(s))


def chain_norm_rows(rows):
    """chain_norm of every row of rows [n, dim]: the in-order float64 fma chain and a correctly rounded sqrt"""
    rows = np.asarray(rows, np.float32)
    s = np.zeros(rows.shape[0], np.float64)
    with np.errstate(all="ignore"):
        for i in range(rows.shape[1]):
            a = rows[:, i].astype(np.float64)
            s = a * a + s
        return np.sqrt(s)


def residual_up(r, rh):
    with np.errstate(all="ignore"):
        d = r.astype(np.float64) - rh.astype(np.float64)
        v = np.float32(np.sqrt(float(np.sum(d * d))) * (1.0 + 1e-12))
    if np.isfinite(v):
        v = np.nextafter(v, np.float32(np.inf)) if (v != 0 or np.any(d != 0)) else v
    return v


def residual_up_rows(rows, rh):
    """residual_up of every row (the order of the additions is free: the value only feeds a bound)"""
    with np.errstate(all="ignore"):
        d = np.asarray(rows, np.float32).astype(np.float64) - np.asarray(rh, np.float32).astype(np.float64)
        v = (np.sqrt(np.sum(d * d, axis=1)) * (1.0 + 1e-12)).astype(np.float32)
        up = np.isfinite(v) & ((v != 0) | np.any(d != 0, axis=1))
        v[up] = np.nextafter(v[up], np.float32(np.inf))
    return v


def query_ok(qn, dim):
    tiny = max(float(np.sqrt(np.float32(dim) * np.float32(2.4e-32))), 1.0e-14)
    return bool(qn >= tiny and qn < 1.0e18)


def interval(metric, q, r):
    rh = bf16(r)
    lo, hi = C.c_float(0), C.c_float(0)
    qn, rn = chain_norm(q), chain_norm(r)
    rc = _lib.lib().qv_scan_bound_interval(metric, q.size, C.c_float(chain32(q, rh)), qn, rn, C.c_float(residual_up(r, rh)), C.byref(lo), C.byref(hi))
    assert rc in (0, 1), _lib.lib().qv_last_error()
    return rc == 1, np.float32(lo.value), np.float32(hi.value), qn


def intervals(metric, dim, s, qn, rn, rres):
    """the library's interval of every row: (unsure [n] bool, d_lo [n], d_hi [n]) from the rows' stage-1 sums, norms and residuals"""
    fn = _lib.lib().qv_scan_bound_interval
    lo, hi = C.c_float(0), C.c_float(0)
    plo, phi = C.byref(lo), C.byref(hi)
    n = len(s)
    out_lo, out_hi, unsure = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, bool)
    qn = float(qn)
    for i, (a, b, c) in enumerate(zip(np.asarray(s, np.float32).tolist(), np.asarray(rn, np.float64).tolist(), np.asarray(rres, np.float32).tolist())):
        rc = fn(metric, dim, a, qn, b, c, plo, phi)
        assert rc in (0, 1), _lib.lib().qv_last_error()
        unsure[i] = rc == 1; out_lo[i] = lo.value; out_hi[i] = hi.value
    return unsure, out_lo, out_hi


class RowState:
    """what ingest derives of a corpus, as the reference computes it: the bfloat16 image, |r| and |r - bf16(r)| rounded up"""

    def __init__(self, rows):
        self.rows = np.ascontiguousarray(rows, np.float32)
        self.rh = bf16(self.rows)
        self.rn = chain_norm_rows(self.rows)
        self.rres = residual_up_rows(self.rows, self.rh)


def stage1(metric, state, q, rres=None):
    """the interval of every row for one query, from the library's own function: what stage 1 computes whatever k is.  `rres` replaces
    the reference's residuals (what a faulty ingest might have stored)."""
    dim = state.rows.shape[1]
    q = np.ascontiguousarray(q, np.float32)
    qn = chain_norm(q)
    s = chain32_rows(q, state.rh)
    unsure, lo, hi = intervals(metric, dim, s, qn, state.rn, state.rres if rres is None else rres)
    return {"s": s, "lo": lo, "hi": hi, "unsure": unsure, "qn": qn, "dim": dim}


def decide(st1, k, alive=None, cap=CAND_CAP):
    """the rest of stage 1 for one k: the threshold H (the k-th smallest upper bound among the live rows the bound is sure of; None when
    there are fewer than k), which rows are passed on (d_lo <= H; a row the bound says nothing about always), and whether the exact scan
    has to answer instead (no H, more survivors than the list holds — `cap` rows: the k <= 64 forms' list unless the caller names another —, a
    query norm the bound does not work with)"""
    lo, hi, unsure = st1["lo"], st1["hi"], st1["unsure"]
    live = np.ones(len(lo), bool) if alive is None else np.asarray(alive, bool)
    his = np.sort(hi[live & ~unsure])
    H = his[k - 1] if len(his) >= k else None
    passed = live & (unsure | (lo <= (H if H is not None else np.float32(-np.inf))))
    hand_back = H is None or int(passed.sum()) > cap or not query_ok(st1["qn"], st1["dim"])
    return dict(st1, H=H, passed=passed, count=int(passed.sum()), hand_back=hand_back)


def reference(metric, state, q, k, alive=None, rres=None, cap=CAND_CAP):
    return decide(stage1(metric, state, q, rres), k, alive, cap)


def oracle_top(metric, rows, q, k, alive=None):
    return O.exact_search(metric, rows, q, k) if alive is None else O.exact_search(metric, rows, q, k, alive=alive)
