"""A FILTERED shared pass of 2 - 8 queries, three arms in one process: the exact filtered scan, the bfloat16 shared pass, the 8-bit stage in
front of it.

    python tools/bench_bound8_filtered_mq.py [--rows 1000000] [--nq 2,4,5,8] [--k 1,10,64] [--filters null,random_1pct,striped,where_10pct]
                                             [--calls 20] [--warmup 3] [--out FILE.json]

One process per shape.  Device-pointer calls on a caller's stream, cosine, 768 dimensions, the benchmark's generator (corpus seed 20260424,
query seed 20260425).  The filters: null sets (every query over every live row, through qv_index_search_rowsets_device); a DISTINCT random
1 % set per query; ONE striped set that keeps one 64-row tile in ten, named by every query; a where-filter per query that selects about 10 %
(one F64 range each, through qv_index_search_where_device).  Per filter, nq and k the arms are set_bound_scan("never"); "always" +
set_bound_plane_filtered_mq("bf16"); "always" + ("8bit") — `calls` calls of each behind HIP events after a warm-up, the arms in turn, the
whole round twice (a / b).  The counters prove which stage answered; every arm's rows and float32 bits are compared with the exact arm's."""
import os; os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # the host's setting, before the first HIP call
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quiver_amd                                              # noqa: E402
from tests import _oracle as O                                  # noqa: E402  (query generator only)

DIM = 768
ARMS = (("exact", "never", "bf16"), ("bf16", "always", "bf16"), ("8bit", "always", "8bit"))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--nq", default="2,4,5,8")
    ap.add_argument("--k", default="1,10,64")
    ap.add_argument("--filters", default="null,random_1pct,striped,where_10pct")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = a.rows
    st = torch.cuda.Stream()
    idx = quiver_amd.DeviceIndex(DIM, "cosine", filter="off")
    idx.add_synthetic(20260424, 0, n)
    assert idx.bound_scan8_stats()["plane"] and idx.bound_scan_stats()["plane"]
    rec = dict(metric="cosine", dim=DIM, rows=n, device=quiver_amd.device_index.device_info(0), calls_per_arm=a.calls, warmup=a.warmup, results=[])
    tile = np.arange(n) // 64
    rng = np.random.default_rng(20260426)
    vals = rng.random(n)
    col = idx.column("f64"); col.set(0, vals)
    striped = idx.rowset(tile % 10 == 0)
    filters = {"null": ("rowsets", [None] * 8), "random_1pct": ("rowsets", [idx.rowset(rng.random(n) < 0.01) for _ in range(8)]),
               "striped": ("rowsets", [striped] * 8), "where_10pct": ("where", [[(col, "ge", 0.1 * j), (col, "lt", 0.1 * j + 0.1)] for j in range(8)])}
    qs = torch.from_numpy(O.gen_rows(20260425, 0, 8, DIM)).cuda()
    for name in a.filters.split(","):
        kind, what = filters[name]
        for nq in [int(x) for x in a.nq.split(",")]:
            for k in [int(x) for x in a.k.split(",")]:
                dr = torch.empty((nq, k), dtype=torch.int32, device="cuda"); dd = torch.empty((nq, k), dtype=torch.float32, device="cuda")

                def call():
                    if kind == "rowsets":
                        idx.search_rowsets_device(qs.data_ptr(), nq, k, what[:nq], dr.data_ptr(), dd.data_ptr(), st.cuda_stream)
                    else:
                        idx.search_where_device(qs.data_ptr(), nq, k, what[:nq], dr.data_ptr(), dd.data_ptr(), st.cuda_stream)

                r = dict(filter=name, rows=n, nq=nq, k=k)
                got = {}
                for rnd in ("a", "b"):
                    for arm, scan, plane in ARMS:
                        idx.set_bound_scan(scan); idx.set_bound_plane_filtered_mq(plane)
                        s8, s16 = idx.bound_scan8_stats(), idx.bound_scan_stats()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        with torch.cuda.stream(st):
                            for i in range(a.warmup + a.calls):
                                if i == a.warmup:
                                    e0.record(st)
                                call()
                            e1.record(st)
                        st.synchronize()
                        r["%s_ms_%s" % (arm, rnd)] = round(e0.elapsed_time(e1) / a.calls, 4)
                        t8, t16 = idx.bound_scan8_stats(), idx.bound_scan_stats()
                        got[arm + rnd] = (dr.cpu().numpy().copy(), dd.cpu().numpy().view(np.uint32).copy())
                        queries = (a.warmup + a.calls) * nq
                        if arm == "exact":
                            assert t16["searches"] == s16["searches"] and t8["searches"] == s8["searches"]
                        elif arm == "bf16":
                            assert t16["searches"] - s16["searches"] == queries and t8["searches"] == s8["searches"], (s16, t16, s8, t8)
                            r["bf16_survivors"], r["bf16_hand_backs"] = t16["candidates"], t16["hand_backs"] - s16["hand_backs"]
                        else:
                            assert t8["searches"] - s8["searches"] == queries and t16["searches"] - s16["searches"] == queries, (s16, t16, s8, t8)
                            r["8bit_survivors"], r["8bit_hand_ons"], r["8bit_reached_exact"] = t8["candidates"], t8["hand_backs"] - s8["hand_backs"], t16["hand_backs"] - s16["hand_backs"]
                r["same_bits"] = all(np.array_equal(g[0], got["exacta"][0]) and np.array_equal(g[1], got["exacta"][1]) for g in got.values())
                r["exact_over_8bit"] = round(min(r["exact_ms_a"], r["exact_ms_b"]) / max(r["8bit_ms_a"], r["8bit_ms_b"]), 3)
                r["bf16_over_8bit"] = round(min(r["bf16_ms_a"], r["bf16_ms_b"]) / max(r["8bit_ms_a"], r["8bit_ms_b"]), 3)   # the worst pairing
                rec["results"].append(r)
                print(json.dumps(r), flush=True)
    idx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
