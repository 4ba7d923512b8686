"""Row sets (qv_index_search_rowsets): what a pass with a set per query costs, what a selective set saves, and what concurrent
filtered callers gain.

    python tools/bench_rowsets.py [--rows 1000000] [--dim 768] [--launches 30] [--seconds 2] [--out profiles/rowsets_1Mx768.json]

(a) one 8-query pass with 8 distinct sets of density 1.0 against the unfiltered 8-query pass (qv_index_search_device) on the same
    index in the same process: device-resident queries and results, HIP events around each call, the two kernels interleaved launch by
    launch after a warm-up of both, min / p50 / max, and each kernel's first half against its second (what the run can resolve);
(e) 16 queries with sets as one 16-query pass against two passes of 8;
(b) the same pass at set densities 0.1 / 0.01 / 0.001, clustered (whole tiles unselected) and uniform, with the fraction of tiles no
    set of the pass selects;
(c) 1 / 8 / 64 / 256 native-thread callers, one query per call, each with its own set (tools/native/qv_callers.cpp qvc_run_rowsets):
    qv_index_search_rowsets against the same threads calling qv_index_search_masked with the same filters as host bitmaps;
(d) one query with a set: the single-query kernels over a device-formed alive & set against a group of one in the multi-query kernel
    (two queries naming the same set, halved) — the choice DESIGN.md records."""
import os; os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # the host's setting, before the first HIP call
import argparse
import ctypes as C
import json
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quiver_amd                                              # noqa: E402
from tests import _oracle as O                                  # noqa: E402  (query generator only)


def stats(ms):
    s = sorted(ms)
    return dict(min_ms=round(s[0], 4), p50_ms=round(s[len(s) // 2], 4), max_ms=round(s[-1], 4), launches=len(s))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=100, help="(a): timed A/B rounds")
    ap.add_argument("--warmup", type=int, default=50, help="(a): untimed A/B rounds first")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--callers", default="1,8,64,256")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, dim, k = a.rows, a.dim, a.k
    idx = quiver_amd.DeviceIndex(dim, "cosine", filter="off")
    idx.add_synthetic(20260424, 0, n)
    qs = O.gen_rows(20260425, 0, 256, dim)
    rng = np.random.default_rng(1)
    rec = dict(shape=[n, dim], k=k, device=quiver_amd.device_index.device_info(0), runtime=quiver_amd.device_index.runtime_info(),
               gpu_max_hw_queues=os.environ.get("GPU_MAX_HW_QUEUES"), launches=a.launches, rounds=a.rounds, warmup=a.warmup, seconds=a.seconds)
    st = torch.cuda.Stream()
    dq = torch.from_numpy(qs[:8]).cuda()
    dr = torch.empty((8, k), dtype=torch.int32, device="cuda"); dd = torch.empty((8, k), dtype=torch.float32, device="cuda")

    def timed(fn):
        out = []
        with torch.cuda.stream(st):
            for i in range(a.launches + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st); fn(); e1.record(st); e1.synchronize()
                if i >= 3:
                    out.append(e0.elapsed_time(e1))
        return stats(out)

    def plain(nq=8):
        return lambda: idx.search_device(dq.data_ptr(), nq, k, dr.data_ptr(), dd.data_ptr(), st.cuda_stream)

    def filtered(sets, nq=8):
        return lambda: idx.search_rowsets_device(dq.data_ptr(), nq, k, sets, dr.data_ptr(), dd.data_ptr(), st.cuda_stream)

    # (a): the two kernels INTERLEAVED (A / B / A / B ...), one timed launch each per round, after a long warm-up of both — a block of one
    # kernel after a block of the other measures the process settling, not the kernels
    full = [idx.rowset(np.ones(n, bool)) for _ in range(8)]
    fa, fb = plain(), filtered(full)
    ta, tb = [], []
    with torch.cuda.stream(st):
        for i in range(a.warmup + a.rounds):
            for fn, out in ((fa, ta), (fb, tb)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st); fn(); e1.record(st); e1.synchronize()
                if i >= a.warmup:
                    out.append(e0.elapsed_time(e1))
    half = len(ta) // 2
    rec["a_unfiltered_8q"] = stats(ta); rec["a_rowsets_8q_density_1"] = stats(tb)
    rec["a_unfiltered_8q_halves_p50"] = [stats(ta[:half])["p50_ms"], stats(ta[half:])["p50_ms"]]       # the same kernel against itself: what the run can resolve
    rec["a_rowsets_8q_halves_p50"] = [stats(tb[:half])["p50_ms"], stats(tb[half:])["p50_ms"]]
    rec["a_ratio_p50"] = round(rec["a_rowsets_8q_density_1"]["p50_ms"] / rec["a_unfiltered_8q"]["p50_ms"], 4)
    rec["a_ratio_min"] = round(rec["a_rowsets_8q_density_1"]["min_ms"] / rec["a_unfiltered_8q"]["min_ms"], 4)
    print("a", json.dumps({x: rec[x] for x in rec if x.startswith("a_")}), flush=True)
    # (e): 16 queries with 16 distinct full sets in ONE call (a 16-query pass for this metric) against two calls of 8, interleaved likewise
    dq16 = torch.from_numpy(qs[:16]).cuda()
    dr16 = torch.empty((16, k), dtype=torch.int32, device="cuda"); dd16 = torch.empty((16, k), dtype=torch.float32, device="cuda")
    full16 = full + [idx.rowset(np.ones(n, bool)) for _ in range(8)]

    def one16():
        idx.search_rowsets_device(dq16.data_ptr(), 16, k, full16, dr16.data_ptr(), dd16.data_ptr(), st.cuda_stream)

    def two8():
        idx.search_rowsets_device(dq16.data_ptr(), 8, k, full16[:8], dr16.data_ptr(), dd16.data_ptr(), st.cuda_stream)
        idx.search_rowsets_device(dq16.data_ptr() + 8 * dim * 4, 8, k, full16[8:], dr16.data_ptr() + 8 * k * 4, dd16.data_ptr() + 8 * k * 4, st.cuda_stream)
    t16, t88 = [], []
    with torch.cuda.stream(st):
        for i in range(10 + a.launches):
            for fn, out in ((one16, t16), (two8, t88)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st); fn(); e1.record(st); e1.synchronize()
                if i >= 10:
                    out.append(e0.elapsed_time(e1))
    rec["e_16q_one_pass_of_16"] = stats(t16); rec["e_16q_two_passes_of_8"] = stats(t88)
    print("e", json.dumps({x: rec[x] for x in rec if x.startswith("e_")}), flush=True)
    # (b)
    rec["b"] = []
    tiles = (n + 63) // 64
    for dens in (0.1, 0.01, 0.001):
        for kind in ("clustered", "uniform"):
            masks = []
            for q in range(8):
                if kind == "clustered":                            # a facet that follows insertion order: whole tiles in or out, the same region for the pass
                    m = np.zeros(n, bool); lo = int(rng.integers(0, max(1, int(n * (1 - dens))))) if q == 0 else lo
                    m[lo:lo + max(64, int(n * dens))] = rng.random(min(n - lo, max(64, int(n * dens)))) < 0.9
                else:
                    m = rng.random(n) < dens
                masks.append(m)
            union = np.zeros(tiles * 64, bool); union[:n] = np.logical_or.reduce(masks)
            skipped = 1.0 - float(union.reshape(tiles, 64).any(axis=1).mean())
            sets = [idx.rowset(m) for m in masks]
            e = dict(density=dens, kind=kind, tiles_skipped=round(skipped, 4), **timed(filtered(sets)))
            rec["b"].append(e)
            print("b", json.dumps(e), flush=True)
            for s in sets:
                s.close()
    # (d)
    one = idx.rowset(rng.random(n) < 0.5)
    rec["d_single_query_and_path"] = timed(filtered([one], 1))
    two = timed(filtered([one, one], 2))
    rec["d_two_queries_multi_kernel"] = two
    rec["d_unfiltered_single"] = timed(plain(1))
    print("d", json.dumps({x: rec[x] for x in rec if x.startswith("d_")}), flush=True)
    # (c)
    lib_c = C.CDLL(os.path.join(os.path.dirname(quiver_amd._lib.LIB_PATH), "libqvcallers.so"))
    fn = lib_c.qvc_run_rowsets
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    n_sets = 64
    words = (n + 63) // 64
    host_masks = np.zeros((n_sets, words), np.uint64)
    sets = []
    for s in range(n_sets):
        m = np.zeros(words * 64, np.uint8); m[:n] = rng.random(n) < (0.5, 0.1, 0.02)[s % 3]
        host_masks[s] = np.packbits(m, bitorder="little").view(np.uint64)
        sets.append(idx.rowset(host_masks[s]))
    handles = (C.c_void_p * n_sets)(*[s.handle.value for s in sets])
    rec["c"] = []
    for t in [int(x) for x in a.callers.split(",")]:
        row = dict(callers=t)
        for name, use_masks in (("rowsets", False), ("masked", True)):
            calls, errs, el, p50, p99 = C.c_uint64(), C.c_uint64(), C.c_double(), C.c_double(), C.c_double()
            s0 = idx.rowset_coalesce_stats()
            rc = fn(idx.handle, qs.ctypes.data, qs.shape[0], dim, k, t, a.seconds, 0, None if use_masks else handles,
                    host_masks.ctypes.data if use_masks else None, words, n_sets, C.byref(calls), C.byref(errs), C.byref(el), C.byref(p50), C.byref(p99))
            s1 = idx.rowset_coalesce_stats()
            g = s1["groups"] - s0["groups"]
            row[name] = dict(rc=rc, qps=round(calls.value / max(el.value, 1e-9), 1), p50_us=round(p50.value, 1), p99_us=round(p99.value, 1), calls=calls.value,
                             errors=errs.value, groups=g, mean_group=round((s1["group_queries"] - s0["group_queries"]) / max(g, 1), 1))
        row["gain"] = round(row["rowsets"]["qps"] / max(row["masked"]["qps"], 1e-9), 2)
        rec["c"].append(row)
        print("c", json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
