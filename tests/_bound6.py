"""Shared restatements behind the tests of the 6-bit stage of the bound scan (quiver_amd/csrc/qv_bound.h: bound6_quant / bound6_pack,
k_row_state6, k_bound_scan6, k_bound_refine8): the row's packed codes and residual from the library's own quantiser compiled for the host
(qv_scan_quantize_row6), their unpacking (qv_scan_unpack_row6), stage 1's sum in numpy integers from the BIASED codes, and the library's
interval (qv_scan_bound_interval8 with 4 rscale8 and rres6).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from quiver_amd import _lib
from tests._bound import chain_norm, chain_norm_rows, query_ok
from tests._bound8 import quantize_query, quantize_row

CAND_CAP6 = 262144                                 # kBound6CandCap
BIAS = 32


def quantize_row6(r):
    """-> (bytes uint8 [dim * 3 / 4], the row's 8-bit scale, residual float32 — NaN: a row the bound says nothing about)"""
    r = np.ascontiguousarray(r, np.float32)
    _, sc, _ = quantize_row(r)
    out = np.zeros(r.size * 3 // 4, np.uint8)
    res = C.c_float(0)
    rc = _lib.lib().qv_scan_quantize_row6(r.size, r.ctypes.data, C.c_float(sc), out.ctypes.data, C.byref(res))
    assert rc == 0, _lib.lib().qv_last_error()
    return out, sc, np.float32(res.value)


def unpack_row6(b):
    """packed bytes -> biased codes uint8 [dim]"""
    b = np.ascontiguousarray(b, np.uint8)
    out = np.zeros(b.size * 4 // 3, np.uint8)
    rc = _lib.lib().qv_scan_unpack_row6(out.size, b.ctypes.data, out.ctypes.data)
    assert rc == 0, _lib.lib().qv_last_error()
    return out


def pack_numpy(u):
    """the layout restated: biased codes [dim] -> bytes [dim * 3 / 4]; per group of 64 dimensions the pieces X, Y, Z of 16 bytes"""
    u = np.asarray(u, np.uint8).reshape(-1, 64)
    out = np.zeros((u.shape[0], 3, 16), np.uint8)
    for c in range(3):
        out[:, c, :] = u[:, 16 * c:16 * c + 16] | (((u[:, 48:64] >> (2 * c)) & 3) << 6)
    return out.reshape(-1)


def isum6(qq, u):
    """stage 1's integer: sum qq_i u_i - 32 sum qq_i, from the biased codes"""
    qq = np.asarray(qq, np.int64)
    return int(np.sum(qq * np.asarray(u, np.int64))) - BIAS * int(np.sum(qq))


def interval6(metric, q, r):
    """one row under one query -> (unsure, d_lo, d_hi, qn)"""
    q = np.ascontiguousarray(q, np.float32)
    b, sc, res = quantize_row6(r)
    u = unpack_row6(b)
    qn, rn = chain_norm(q), chain_norm(np.ascontiguousarray(r, np.float32))
    qz = quantize_query(q)
    lo, hi = C.c_float(0), C.c_float(0)
    if qz is None:
        isum, sq, qres = 0, 1.0, float("nan")
    else:
        qq, qhi, qlo, sq, qres = qz
        isum = isum6(qq, u)
        u64 = u.astype(np.int64)
        assert abs(int(np.sum(qhi * u64))) < 2 ** 31 and abs(int(np.sum(qlo * u64))) < 2 ** 31      # the sums stage 1 keeps
    with np.errstate(all="ignore"):
        sc4 = np.float32(4.0) * np.float32(sc)
    rc = _lib.lib().qv_scan_bound_interval8(metric, q.size, isum, sq, qn, qres, rn, C.c_float(sc4), C.c_float(res), C.byref(lo), C.byref(hi))
    assert rc in (0, 1), _lib.lib().qv_last_error()
    return rc == 1, np.float32(lo.value), np.float32(hi.value), qn


class RowState6:
    """what ingest derives of a corpus for the 6-bit stage"""

    def __init__(self, rows):
        self.rows = np.ascontiguousarray(rows, np.float32)
        n, dim = self.rows.shape
        self.bytes = np.zeros((n, dim * 3 // 4), np.uint8)
        self.scale = np.zeros(n, np.float32)
        self.res = np.zeros(n, np.float32)
        for i in range(n):
            self.bytes[i], self.scale[i], self.res[i] = quantize_row6(self.rows[i])
        self.codes = np.stack([unpack_row6(b) for b in self.bytes]).astype(np.int64) - BIAS
        self.rn = chain_norm_rows(self.rows)

    def plane(self):
        """the device's layout: [tile][group][3][64 rows][16 bytes], rows past the last as the zero rows the tiles hold (code 0, biased 32)"""
        n, dim = self.rows.shape
        tiles, groups = (n + 63) // 64, dim // 64
        pad = np.full((tiles * 64, groups, 3, 16), BIAS, np.uint8)
        pad[n:, :, 0, :] |= (BIAS & 3) << 6; pad[n:, :, 1, :] |= ((BIAS >> 2) & 3) << 6; pad[n:, :, 2, :] |= ((BIAS >> 4) & 3) << 6
        pad[:n] = self.bytes.reshape(n, groups, 3, 16)
        return np.ascontiguousarray(pad.reshape(tiles, 64, groups, 3, 16).transpose(0, 2, 3, 1, 4)).reshape(-1)


def reference6(metric, state, q, k, alive=None):
    """the 6-bit stage for one query and one k: every row's interval, H, the candidates, and whether the stage hands the search on"""
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
        isums = state.codes @ qq
    with np.errstate(all="ignore"):
        sc4 = (np.float32(4.0) * state.scale).astype(np.float32)
    for i in range(n):
        rc = fn(metric, dim, int(isums[i]), sq, qn, qres, float(state.rn[i]), C.c_float(sc4[i]), C.c_float(state.res[i]), C.byref(lo), C.byref(hi))
        assert rc in (0, 1)
        unsure[i] = rc == 1; out_lo[i] = lo.value; out_hi[i] = hi.value
    live = np.ones(n, bool) if alive is None else np.asarray(alive, bool)
    his = np.sort(out_hi[live & ~unsure])
    H = his[k - 1] if len(his) >= k else None
    passed = live & (unsure | (out_lo <= (H if H is not None else np.float32(-np.inf))))
    hand_back = H is None or int(passed.sum()) > CAND_CAP6 or not query_ok(qn, dim)
    return {"lo": out_lo, "hi": out_hi, "unsure": unsure, "H": H, "passed": passed, "count": int(passed.sum()), "hand_back": hand_back}
