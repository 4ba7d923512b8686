"""Shared restatements behind the tests of the 8-bit stage of the bound scan (quiver_amd/csrc/qv_bound.h: bound_scan_interval8,
k_row_state8, k_bound_scan8): the row's bytes, scale and residual from the library's own quantiser compiled for the host
(qv_scan_quantize_row8), the query's split and stage 1's sum in numpy integers, and the library's interval (qv_scan_bound_interval8).
TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from quiver_amd import _lib
from tests._bound import CAND_CAP, chain_norm, chain_norm_rows, query_ok

QMAX = 16256                                       # kBound8QueryMax: 127 * 128


def quantize_row(r):
    """-> (bytes int8 [dim], scale float32, residual float32 — NaN: a row the bound says nothing about)"""
    r = np.ascontiguousarray(r, np.float32)
    out = np.zeros(r.size, np.int8)
    sc, res = C.c_float(0), C.c_float(0)
    rc = _lib.lib().qv_scan_quantize_row8(r.size, r.ctypes.data, out.ctypes.data, C.byref(sc), C.byref(res))
    assert rc == 0, _lib.lib().qv_last_error()
    return out, np.float32(sc.value), np.float32(res.value)


def quantize_query(q):
    """-> (qq int64 [dim] = 128 hi + lo, hi, lo, sq, qres rounded up); None for a query without a scale (a non-finite or no non-zero element)"""
    q64 = np.ascontiguousarray(q, np.float32).astype(np.float64)
    mx = float(np.max(np.abs(q64))) if np.all(np.isfinite(q64)) else 0.0
    if not mx > 0.0:
        return None
    sq = mx / QMAX
    qq = np.rint(q64 / sq)
    hi = np.rint(qq / 128.0)
    lo = qq - 128.0 * hi
    assert np.all(np.abs(hi) <= 127) and np.all(np.abs(lo) <= 64)
    d = q64 - sq * qq
    qres = float(np.sqrt(np.sum(d * d))) * (1.0 + 1e-9) + 1e-300
    return qq.astype(np.int64), hi.astype(np.int64), lo.astype(np.int64), sq, qres


def interval8(metric, q, r):
    """one row under one query -> (unsure, d_lo, d_hi, qn)"""
    q = np.ascontiguousarray(q, np.float32)
    r8, sc, res = quantize_row(r)
    qn, rn = chain_norm(q), chain_norm(np.ascontiguousarray(r, np.float32))
    qz = quantize_query(q)
    lo, hi = C.c_float(0), C.c_float(0)
    if qz is None:
        isum, sq, qres = 0, 1.0, float("nan")
    else:
        _, qhi, qlo, sq, qres = qz
        r64 = r8.astype(np.int64)
        isum = 128 * int(np.sum(qhi * r64)) + int(np.sum(qlo * r64))      # the two sums stage 1 keeps (each within int32: asserted)
        assert abs(int(np.sum(qhi * r64))) < 2 ** 31 and abs(int(np.sum(qlo * r64))) < 2 ** 31
    rc = _lib.lib().qv_scan_bound_interval8(metric, q.size, isum, sq, qn, qres, rn, C.c_float(sc), C.c_float(res), C.byref(lo), C.byref(hi))
    assert rc in (0, 1), _lib.lib().qv_last_error()
    return rc == 1, np.float32(lo.value), np.float32(hi.value), qn


class RowState8:
    """what ingest derives of a corpus for the 8-bit stage"""

    def __init__(self, rows):
        self.rows = np.ascontiguousarray(rows, np.float32)
        n, dim = self.rows.shape
        self.r8 = np.zeros((n, dim), np.int8)
        self.scale = np.zeros(n, np.float32)
        self.res = np.zeros(n, np.float32)
        for i in range(n):
            self.r8[i], self.scale[i], self.res[i] = quantize_row(self.rows[i])
        self.rn = chain_norm_rows(self.rows)


def reference8(metric, state, q, k, alive=None):
    """the 8-bit stage for one query and one k: every row's interval, H, the rows passed on, and whether the stage hands the search on"""
    q = np.ascontiguousarray(q, np.float32)
    n, dim = state.rows.shape
    qn = chain_norm(q)
    qz = quantize_query(q)
    fn = _lib.lib().qv_scan_bound_interval8
    lo, hi = C.c_float(0), C.c_float(0)
    out_lo, out_hi, unsure = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, bool)
    if qz is None:
        isums, sq, qres = np.zeros(n, np.int64), 1.0, float("nan")
    else:
        qq, _, _, sq, qres = qz
        isums = state.r8.astype(np.int64) @ qq
    for i in range(n):
        rc = fn(metric, dim, int(isums[i]), sq, qn, qres, float(state.rn[i]), C.c_float(state.scale[i]), C.c_float(state.res[i]), C.byref(lo), C.byref(hi))
        assert rc in (0, 1)
        unsure[i] = rc == 1; out_lo[i] = lo.value; out_hi[i] = hi.value
    live = np.ones(n, bool) if alive is None else np.asarray(alive, bool)
    his = np.sort(out_hi[live & ~unsure])
    H = his[k - 1] if len(his) >= k else None
    passed = live & (unsure | (out_lo <= (H if H is not None else np.float32(-np.inf))))
    hand_back = H is None or int(passed.sum()) > CAND_CAP or not query_ok(qn, dim)
    return {"lo": out_lo, "hi": out_hi, "unsure": unsure, "H": H, "passed": passed, "count": int(passed.sum()), "hand_back": hand_back}
