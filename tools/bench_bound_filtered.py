"""The bound scan under filters against the exact filtered scan, one process, the two arms interleaved.

    python tools/bench_bound_filtered.py [--rows 1000000] [--dim 768] [--calls 30] [--warmup 5] [--nq 1,2,4,8] [--k 10,64]
                                         [--out profiles/bound_scan_filtered_1Mx768.json]

Device-pointer calls (qv_index_search_rowsets_device), cosine.  For every (nq, k, sets) the arms are set_bound_scan("never") — the exact
filtered scan: k_rowset_scan_mq, k_flat_scan over the candidate bitmap — and set_bound_scan("always") — k_bound_scan_mq<., ., true>,
k_bound_scan<., true>; one call of each in turn, HIP events around each call, after a warm-up of both.  Reported per arm: the median and
the spread (p25 .. p75, min, max); `wins` is true when the median of "always" is below the median of "never" by more than the two arms'
combined spread, taken as the SUM of both arms' full interquartile ranges (p75 - p25 of each; min .. max is reported too, but a single
outlier call would then decide a 30-call arm).  The bound-scan counters prove which path each arm took.
With --callers (e.g. 1,8): native threads, one query per call, 64 distinct sets (tools/native/qv_callers.cpp qvc_run_rowsets) under
"never" and under "always", alternating, --rounds times each; QPS per arm as the median over rounds with min .. max.
The shapes of profiles/LAB_r09_bound_scan_filtered.md: --rows 300000, --rows 1000000 --callers 1,8, --rows 10000000.
Sets: random of density 1.0 / 0.5 / 0.1 / 0.01, and a tile-striped set keeping 1 tile in 10; for nq > 1 distinct sets per query, and also
one set for all."""
import os; os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # the host's setting, before the first HIP call
import argparse
import ctypes as C
import json
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quiver_amd                                              # noqa: E402
from tests import _oracle as O                                  # noqa: E402  (query generator only)


def spread(ms):
    s = np.sort(np.asarray(ms))
    q = lambda p: float(s[min(len(s) - 1, int(p * len(s)))])
    return dict(median_ms=round(q(0.5), 4), p25_ms=round(q(0.25), 4), p75_ms=round(q(0.75), 4), min_ms=round(float(s[0]), 4), max_ms=round(float(s[-1]), 4), calls=len(s))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--calls", type=int, default=30, help="timed calls per arm (at least 30)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nq", default="1,2,4,8")
    ap.add_argument("--k", default="10,64")
    ap.add_argument("--callers", default="", help="native-thread callers, e.g. 1,8 (empty: none)")
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, dim = a.rows, a.dim
    calls = max(a.calls, 30)
    idx = quiver_amd.DeviceIndex(dim, "cosine", filter="off")
    idx.add_synthetic(20260424, 0, n)
    assert idx.bound_scan_stats()["plane"]
    qs = O.gen_rows(20260425, 0, 8, dim)
    rng = np.random.default_rng(9)
    tile = np.arange(n) // 64
    kinds = [("random 1.0", lambda: np.ones(n, bool)), ("random 0.5", lambda: rng.random(n) < 0.5), ("random 0.1", lambda: rng.random(n) < 0.1),
             ("random 0.01", lambda: rng.random(n) < 0.01), ("striped 1 tile in 10", lambda: (tile + rng.integers(0, 10)) % 10 == 0)]
    st = torch.cuda.Stream()
    dq = torch.from_numpy(qs).cuda()
    rec = dict(shape=[n, dim], metric="cosine", device=quiver_amd.device_index.device_info(0), runtime=quiver_amd.device_index.runtime_info(),
               calls_per_arm=calls, warmup=a.warmup, baseline='set_bound_scan("never"): the exact filtered scan', results=[])
    for nq in [int(x) for x in a.nq.split(",")]:
        for name, make in kinds:
            for share in ((False, True) if nq > 1 else (False,)):
                masks = [make()] * nq if share else [make() for _ in range(nq)]
                sets = [idx.rowset(m) for m in (masks[:1] if share else masks)]
                sets = sets * nq if share else sets
                union = np.zeros(n, bool)
                for m in masks:
                    union |= m
                cand_tiles = int(np.unique(tile[union]).size)
                for k in [int(x) for x in a.k.split(",")]:
                    dr = torch.empty((nq, k), dtype=torch.int32, device="cuda"); dd = torch.empty((nq, k), dtype=torch.float32, device="cuda")
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(2 * (calls + a.warmup))]
                    got, took = {}, {}
                    with torch.cuda.stream(st):
                        for i in range(calls + a.warmup):
                            for arm, mode in enumerate(("never", "always")):
                                idx.set_bound_scan(mode)
                                e0, e1 = ev[2 * i + arm]
                                if i == 0:                                # (a warm-up call) which path the arm takes, and its answer
                                    st.synchronize()
                                    s0 = idx.bound_scan_stats()["searches"]
                                e0.record(st)
                                idx.search_rowsets_device(dq.data_ptr(), nq, k, sets, dr.data_ptr(), dd.data_ptr(), st.cuda_stream)
                                e1.record(st)
                                if i == 0:
                                    st.synchronize()
                                    got[mode] = (dr.cpu().numpy().copy(), dd.cpu().numpy().view(np.uint32).copy())
                                    took[mode] = idx.bound_scan_stats()["searches"] - s0
                    st.synchronize()
                    arms = {mode: spread([ev[2 * i + arm][0].elapsed_time(ev[2 * i + arm][1]) for i in range(a.warmup, calls + a.warmup)]) for arm, mode in enumerate(("never", "always"))}
                    noise = (arms["never"]["p75_ms"] - arms["never"]["p25_ms"]) + (arms["always"]["p75_ms"] - arms["always"]["p25_ms"])
                    r = dict(nq=nq, k=k, sets=name, one_set_for_all=share, candidate_tiles=cand_tiles, n_tiles=int(tile[-1]) + 1, never=arms["never"], always=arms["always"],
                             combined_spread_ms=round(noise, 4), wins=bool(arms["never"]["median_ms"] - arms["always"]["median_ms"] > noise),
                             same_bits=bool(np.array_equal(got["never"][0], got["always"][0]) and np.array_equal(got["never"][1], got["always"][1])),
                             bound_searches={"never": took["never"], "always": took["always"]},
                             automatic_rule_accepts=quiver_amd.device_index.scan_bound_applies_filtered("cosine", dim, n, nq, k, "auto", True, cand_tiles))
                    rec["results"].append(r)
                    print(json.dumps(r), flush=True)
                for s in set(sets):
                    s.close()
    if a.callers:
        lib_c = C.CDLL(os.path.join(os.path.dirname(quiver_amd._lib.LIB_PATH), "libqvcallers.so"))
        fn = lib_c.qvc_run_rowsets
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                       C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        n_sets, k = 64, 10
        cq = O.gen_rows(20260426, 0, 256, dim)
        csets = [idx.rowset(rng.random(n) < (0.5, 0.1, 0.02)[s % 3]) for s in range(n_sets)]   # tools/bench_rowsets.py (c)'s densities
        handles = (C.c_void_p * n_sets)(*[s.handle.value for s in csets])
        rec["callers"] = []
        for t in [int(x) for x in a.callers.split(",")]:
            qps = {"never": [], "always": []}
            row = dict(callers=t, k=k, sets=n_sets, seconds=a.seconds)
            for rnd in range(a.rounds + 1):                               # (round 0: warm-up of both arms)
                for mode in ("never", "always"):
                    idx.set_bound_scan(mode)
                    calls, errs, el, p50, p99 = C.c_uint64(), C.c_uint64(), C.c_double(), C.c_double(), C.c_double()
                    s0 = idx.bound_scan_stats()["searches"]
                    rc = fn(idx.handle, cq.ctypes.data, cq.shape[0], dim, k, t, a.seconds, 0, handles, None, 0, n_sets, C.byref(calls), C.byref(errs), C.byref(el), C.byref(p50), C.byref(p99))
                    assert rc == 0 and errs.value == 0, (rc, errs.value)
                    row[mode + "_bound_searches_per_call"] = round((idx.bound_scan_stats()["searches"] - s0) / max(calls.value, 1), 3)
                    if rnd:
                        qps[mode].append(calls.value / max(el.value, 1e-9))
            for mode in ("never", "always"):
                v = sorted(qps[mode])
                row[mode] = dict(qps_median=round(v[len(v) // 2], 1), qps_min=round(v[0], 1), qps_max=round(v[-1], 1), rounds=len(v))
            row["wins"] = bool(row["always"]["qps_min"] > row["never"]["qps_max"])
            rec["callers"].append(row)
            print("callers", json.dumps(row), flush=True)
    idx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
