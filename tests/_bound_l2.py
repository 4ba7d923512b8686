"""Shared restatements behind the tests of the bound scan on Euclidean indexes (quiver_amd/csrc/qv_bound.h: the QV_L2 forms of
bound_scan_interval / bound_scan_interval8): the reference's distance in plain numpy (pkg/vectortypes/distances.go:48-54), the two
margins recomputed from qv_bound.h's formulas, the corpora the GPU tests search, and stage 1's survivor counts on them from the library's
own interval function compiled for the host — computed by tests/test_bound_scan_l2_cpu.py, pinned in RECORDED, and compared by
tests/test_gpu_bound_scan_l2.py with what the device counts.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools

import numpy as np

from quiver_amd import _lib

from tests import _bound as B
from tests import _bound8 as B8
from tests import _oracle as O
from tests import _widths as W

L2 = 1                                             # QV_L2
RULE_L2_PLANES = 0x101                             # QV_RULE_L2_PLANES: a QV_L2 index created with QV_FLAG_L2_SCAN_PLANE, for the rule functions


def euclid_numpy(a, b):
    """distances.go:48-54: diff = float64(a[i] - b[i]) (a float32 subtraction), sum += diff * diff in element order, float32(sqrt(sum))"""
    d = (np.ascontiguousarray(a, np.float32) - np.ascontiguousarray(b, np.float32)).astype(np.float64)
    s = 0.0
    with np.errstate(all="ignore"):
        for x in d.tolist():
            s = x * x + s                          # the square of a float32 value is exact in float64: multiply-add == fma
        return np.float32(np.sqrt(s))


def interval(q, r):
    """tests/_bound.interval for QV_L2, through the library's Euclidean entry point (qv_scan_bound_interval_l2: qv_scan_bound_interval keeps
    answering "unsupported" for QV_L2) -> (unsure, d_lo, d_hi, |q|)"""
    rh = B.bf16(r)
    lo, hi = C.c_float(0), C.c_float(0)
    qn, rn = B.chain_norm(q), B.chain_norm(r)
    rc = _lib.lib().qv_scan_bound_interval_l2(q.size, C.c_float(B.chain32(q, rh)), qn, rn, C.c_float(B.residual_up(r, rh)), C.byref(lo), C.byref(hi))
    assert rc in (0, 1), _lib.lib().qv_last_error()
    return rc == 1, np.float32(lo.value), np.float32(hi.value), qn


def stage1(state, q):
    """tests/_bound.stage1 for QV_L2: the interval of every row of a tests/_bound.RowState for one query"""
    dim = state.rows.shape[1]
    q = np.ascontiguousarray(q, np.float32)
    qn = float(B.chain_norm(q))
    s = B.chain32_rows(q, state.rh)
    fn = _lib.lib().qv_scan_bound_interval_l2
    lo, hi = C.c_float(0), C.c_float(0)
    n = len(s)
    out_lo, out_hi, unsure = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, bool)
    for i, (a, b, c) in enumerate(zip(s.tolist(), np.asarray(state.rn, np.float64).tolist(), np.asarray(state.rres, np.float32).tolist())):
        rc = fn(dim, a, qn, b, c, C.byref(lo), C.byref(hi))
        assert rc in (0, 1), _lib.lib().qv_last_error()
        unsure[i] = rc == 1; out_lo[i] = lo.value; out_hi[i] = hi.value
    return {"s": s, "lo": out_lo, "hi": out_hi, "unsure": unsure, "qn": qn, "dim": dim}


def gamma(dim):
    """bound_scan_gamma (qv_bound.h)"""
    g = (dim + 2) * 2.0 ** -24
    return g / (1.0 - g) * (1.0 + 1e-6) + 5e-7 + 1e-12


def margin16(q, r):
    """m of bound_scan_interval for one pair: |q| (rres + gamma (|r| + rres)) (1 + 1e-9)"""
    rr = float(B.residual_up(r, B.bf16(r)))
    qn, rn = B.chain_norm(q), B.chain_norm(r)
    return qn * (rr + gamma(q.size) * (rn + rr)) * (1.0 + 1e-9), qn, rn


def margin8(q, r):
    """m of bound_scan_interval8 for one pair: (|q| rres8 + qres (|r| + rres8) + 1e-12 (|q| + qres)(|r| + rres8)) (1 + 1e-9)"""
    _, _, res = B8.quantize_row(r)
    qres = B8.quantize_query(q)[4]
    qn, rn, rr = B.chain_norm(q), B.chain_norm(r), float(res)
    return (qn * rr + qres * (rn + rr) + 1e-12 * (qn + qres) * (rn + rr)) * (1.0 + 1e-9), qn, rn


# ---- the corpora of tests/test_gpu_bound_scan_l2.py: name -> (rows' seed, rows, dim, queries' seed) -------------------------------
CORPORA = {"12000x128": (6100, 12_000, 128, 6101), "4000x768": (6200, 4_000, 768, 6201), "2000x16": (6300, 2_000, 16, 6301)}
KS = (1, 10, 64)
NQ = 2                                             # queries per corpus that the single-query tests run and the model pins


@functools.lru_cache(maxsize=None)
def corpus(name):
    seed, n, dim, qseed = CORPORA[name]
    rows, qs = O.gen_rows(seed, 0, n, dim), O.gen_rows(qseed, 0, 8, dim)
    rows.setflags(write=False); qs.setflags(write=False)
    return rows, qs


@functools.lru_cache(maxsize=None)
def _states(name):
    rows, _ = corpus(name)
    return B.RowState(rows), B8.RowState8(rows)


@functools.lru_cache(maxsize=None)
def stages(name, qi):
    """(the bfloat16 stage's intervals, the 8-bit stage's) of query qi over the corpus, whatever k is"""
    st, st8 = _states(name)
    q = corpus(name)[1][qi]
    return stage1(st, q), W.stage8_of(L2, st8, q)


def model_counts(name):
    """{(plane, query, k): stage 1's survivor count} with no hand-back anywhere (asserted): what the device must count"""
    out = {}
    for qi in range(NQ):
        s16, s8 = stages(name, qi)
        for k in KS:
            for plane, s in (("bf16", s16), ("8bit", s8)):
                d = B.decide(s, k)
                assert not d["hand_back"] and k <= d["count"] <= B.CAND_CAP, (name, plane, qi, k, d["count"])
                out[(plane, qi, k)] = d["count"]
    return out


# model_counts as tests/test_bound_scan_l2_cpu.py computed them (it asserts they still are): the figures the device's counters must show
RECORDED = {
    "12000x128": {("bf16", 0, 1): 1, ("8bit", 0, 1): 1, ("bf16", 0, 10): 10, ("8bit", 0, 10): 15, ("bf16", 0, 64): 73, ("8bit", 0, 64): 96,
                  ("bf16", 1, 1): 1, ("8bit", 1, 1): 1, ("bf16", 1, 10): 14, ("8bit", 1, 10): 20, ("bf16", 1, 64): 68, ("8bit", 1, 64): 89},
    "4000x768": {("bf16", 0, 1): 1, ("8bit", 0, 1): 3, ("bf16", 0, 10): 12, ("8bit", 0, 10): 26, ("bf16", 0, 64): 75, ("8bit", 0, 64): 139,
                 ("bf16", 1, 1): 1, ("8bit", 1, 1): 4, ("bf16", 1, 10): 11, ("8bit", 1, 10): 24, ("bf16", 1, 64): 85, ("8bit", 1, 64): 143},
    "2000x16": {("bf16", 0, 1): 1, ("8bit", 0, 1): 1, ("bf16", 0, 10): 10, ("8bit", 0, 10): 10, ("bf16", 0, 64): 68, ("8bit", 0, 64): 72,
                ("bf16", 1, 1): 1, ("8bit", 1, 1): 2, ("bf16", 1, 10): 11, ("8bit", 1, 10): 14, ("bf16", 1, 64): 65, ("8bit", 1, 64): 67},
}
