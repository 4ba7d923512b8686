"""Concurrent FILTERED callers, one query per call, through the row-set front — every caller with its own row set, then every caller with
its own where-filter — under the index's DEFAULT modes: what a host that sets nothing gets.

    python tools/bench_callers_filtered.py [--rows 10000000] [--callers 2,4,8] [--seconds 1.5] [--label tree] [--out FILE.json]
    python tools/bench_callers_filtered.py --merge A.json B.json ... --out FILE.json

Cosine, 768 dimensions, k = 10, the benchmark's generator (corpus seed 20260424, query seed 20260425).  Set callers are native threads
(tools/native/qv_callers.cpp qvc_run_rowsets, qv_index_search_rowsets): caller t names set t, a random half / tenth / fiftieth of the rows.
Where callers are Python threads (the native loops have no where-filter form) calling qv_index_search_where with one F64 range that selects
about 10 % and whose literal changes on every request, as tests/bench/bench_search_where.py's arm B.  Per caller count a warm-up window, then
one timed window: calls per second, per-call p50 / p99, how many calls shared a pass, and how many queries took the bound scan and its 8-bit
stage.  The script uses nothing a library before the filtered shared pass's plane setter lacks, so a checkout of the parent commit runs it
unchanged (`--label parent`); `--merge` puts the records of alternating runs into one file."""
import os; os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # the host's setting, before the first HIP call
import argparse
import ctypes as C
import json
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quiver_amd                                              # noqa: E402
from tests import _oracle as O                                  # noqa: E402  (query generator only)

DIM, K = 768, 10


def counters(idx):
    a, b, c = idx.bound_scan8_stats(), idx.bound_scan_stats(), idx.rowset_coalesce_stats()
    return {"took8": a["searches"], "on8": a["hand_backs"], "took": b["searches"], "back": b["hand_backs"], "groups": c["groups"], "group_queries": c["group_queries"], "solo": c["solo"]}


def delta(c0, c1):
    d = {k: c1[k] - c0[k] for k in c0}
    d["mean_group"] = round(d["group_queries"] / max(d["groups"], 1), 2)
    return d


def where_window(idx, col, qs, callers, seconds):
    lat = [[] for _ in range(callers)]
    errs = []
    start = threading.Barrier(callers + 1)

    def loop(t):
        try:
            start.wait()
            end = time.perf_counter() + seconds
            i = 0
            while True:
                t0 = time.perf_counter()
                if t0 >= end:
                    break
                idx.search_where(qs[t:t + 1], K, [(col, "lt", 0.1 + 1e-9 * (1 + t * 100_003 + i))])
                lat[t].append((time.perf_counter() - t0) * 1e6)
                i += 1
        except Exception as e:                                          # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=loop, args=(t,)) for t in range(callers)]
    [x.start() for x in th]
    start.wait()
    t0 = time.perf_counter()
    [x.join() for x in th]
    wall = time.perf_counter() - t0
    if errs:
        raise errs[0]
    flat = np.concatenate([np.asarray(x, dtype=np.float64) for x in lat])
    return dict(qps=round(flat.size / wall, 1), p50_us=round(float(np.percentile(flat, 50)), 1), p99_us=round(float(np.percentile(flat, 99)), 1), calls=int(flat.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--callers", default="2,4,8")
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--out", default="")
    ap.add_argument("--merge", nargs="*", default=None, help="write --out from these record files instead of measuring")
    a = ap.parse_args()
    if a.merge is not None:
        with open(a.out, "w") as f:
            json.dump({"runs": [json.load(open(p)) for p in a.merge]}, f, indent=1); f.write("\n")
        return
    n = a.rows
    idx = quiver_amd.DeviceIndex(DIM, "cosine")
    idx.add_synthetic(20260424, 0, n)
    assert idx.bound_scan8_stats()["plane"] and idx.bound_scan_stats()["plane"]
    qs = O.gen_rows(20260425, 0, 256, DIM)
    rng = np.random.default_rng(20260426)
    col = idx.column("f64"); col.set(0, rng.random(n))
    n_sets = 8
    sets = [idx.rowset(rng.random(n) < (0.5, 0.1, 0.02)[s % 3]) for s in range(n_sets)]
    handles = (C.c_void_p * n_sets)(*[s.handle.value for s in sets])
    lib_c = C.CDLL(os.path.join(os.path.dirname(quiver_amd._lib.LIB_PATH), "libqvcallers.so"))
    fn = lib_c.qvc_run_rowsets
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]

    def sets_window(t, seconds):
        calls, errs, el, p50, p99 = C.c_uint64(), C.c_uint64(), C.c_double(), C.c_double(), C.c_double()
        rc = fn(idx.handle, qs.ctypes.data, qs.shape[0], DIM, K, t, seconds, 0, handles, None, (n + 63) // 64, n_sets, C.byref(calls), C.byref(errs), C.byref(el), C.byref(p50), C.byref(p99))
        assert rc == 0 and errs.value == 0, (rc, errs.value)
        return dict(qps=round(calls.value / max(el.value, 1e-9), 1), p50_us=round(p50.value, 1), p99_us=round(p99.value, 1), calls=calls.value)

    rec = dict(label=a.label, rows=n, dim=DIM, k=K, metric="cosine", seconds_per_window=a.seconds, device=quiver_amd.device_index.device_info(0),
               has_filtered_mq_setter=hasattr(idx, "set_bound_plane_filtered_mq"), results=[])
    for t in [int(x) for x in a.callers.split(",")]:
        for kind in ("sets", "where"):
            run = (lambda s: sets_window(t, s)) if kind == "sets" else (lambda s: where_window(idx, col, qs, t, s))
            run(min(a.seconds, 0.3))                                    # warm-up: buffers grown, contexts made
            c0 = counters(idx)
            r = run(a.seconds)
            r.update(kind=kind, callers=t, **delta(c0, counters(idx)))
            rec["results"].append(r)
            print(json.dumps(dict(r, label=a.label, rows=n)), flush=True)
    idx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
