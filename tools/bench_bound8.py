"""The single-query bound scan's four arms in one process: the exact scan, the bfloat16 stage first, the 8-bit stage first, the 6-bit stage first.

    python tools/bench_bound8.py [--shapes 768:100000,768:300000,...] [--k 1,10,64] [--calls 20] [--warmup 3] [--out FILE.json]

Device-pointer calls (qv_index_search_device), cosine, the benchmark's generator (corpus seed 20260424, query seed 20260425).  For every
shape and k the arms are set_bound_scan("never"); set_bound_scan("always") + set_bound_plane("bf16"); set_bound_scan("always") +
set_bound_plane("8bit") + set_bound_plane6("never"); the same with set_bound_plane6("always") where the index holds the 6-bit plane (a
dimension that is a multiple of 64) — `calls` calls of each behind HIP events after a warm-up, the whole round twice (a / b).  The counters prove
which stage answered; the arms' rows and float32 bits are compared.  The shapes of profiles/LAB_r10_bound_scan_8bit.md are the defaults."""
import os; os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # the host's setting, before the first HIP call
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quiver_amd                                              # noqa: E402
from tests import _oracle as O                                  # noqa: E402  (query generator only)

ARMS = (("exact", "never", "bf16", "never"), ("bf16", "always", "bf16", "never"), ("8bit", "always", "8bit", "never"), ("6bit", "always", "8bit", "always"))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="768:100000,768:300000,768:1000000,768:3000000,768:10000000,128:1000000,128:10000000")
    ap.add_argument("--k", default="1,10,64")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    st = torch.cuda.Stream()
    rec = dict(metric="cosine", device=quiver_amd.device_index.device_info(0), calls_per_arm=a.calls, warmup=a.warmup, results=[])
    for shape in a.shapes.split(","):
        dim, n = (int(x) for x in shape.split(":"))
        idx = quiver_amd.DeviceIndex(dim, "cosine", filter="off")
        idx.add_synthetic(20260424, 0, n)
        assert idx.bound_scan8_stats()["plane"] and idx.bound_scan_stats()["plane"]
        arms = [x for x in ARMS if x[0] != "6bit" or idx.bound_scan6_stats()["plane"]]
        q = torch.from_numpy(O.gen_rows(20260425, 0, 1, dim)).cuda()
        for k in [int(x) for x in a.k.split(",")]:
            dr = torch.empty((1, k), dtype=torch.int32, device="cuda"); dd = torch.empty((1, k), dtype=torch.float32, device="cuda")
            r = dict(dim=dim, rows=n, k=k)
            got = {}
            for rnd in ("a", "b"):
                for arm, scan, plane, plane6 in arms:
                    idx.set_bound_scan(scan); idx.set_bound_plane(plane); idx.set_bound_plane6(plane6)
                    s8, s16, s6 = idx.bound_scan8_stats(), idx.bound_scan_stats(), idx.bound_scan6_stats()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(st):
                        for i in range(a.warmup + a.calls):
                            if i == a.warmup:
                                e0.record(st)
                            idx.search_device(q.data_ptr(), 1, k, dr.data_ptr(), dd.data_ptr(), st.cuda_stream)
                        e1.record(st)
                    st.synchronize()
                    r["%s_ms_%s" % (arm, rnd)] = round(e0.elapsed_time(e1) / a.calls, 4)
                    t8, t16, t6 = idx.bound_scan8_stats(), idx.bound_scan_stats(), idx.bound_scan6_stats()
                    assert (t6["searches"] - s6["searches"]) == (a.warmup + a.calls if arm == "6bit" else 0)
                    got[arm] = (dr.cpu().numpy().copy(), dd.cpu().numpy().view(np.uint32).copy())
                    calls = a.warmup + a.calls
                    if arm == "exact":
                        assert t16["searches"] == s16["searches"] and t8["searches"] == s8["searches"]
                    elif arm == "bf16":
                        assert t16["searches"] - s16["searches"] == calls and t8["searches"] == s8["searches"]
                        r["bf16_survivors"], r["bf16_hand_backs"] = t16["candidates"], t16["hand_backs"] - s16["hand_backs"]
                    elif arm == "6bit":
                        assert t8["searches"] - s8["searches"] == calls and t16["searches"] - s16["searches"] == calls
                        r["6bit_candidates"], r["6bit_hand_backs"], r["6bit_survivors"] = t6["candidates"], t6["hand_backs"] - s6["hand_backs"], t8["candidates"]
                    else:
                        assert t8["searches"] - s8["searches"] == calls and t16["searches"] - s16["searches"] == calls
                        r["8bit_survivors"], r["8bit_hand_backs"], r["8bit_reached_exact"] = t8["candidates"], t8["hand_backs"] - s8["hand_backs"], t16["hand_backs"] - s16["hand_backs"]
            r["same_bits"] = all(np.array_equal(got[x][0], got["exact"][0]) and np.array_equal(got[x][1], got["exact"][1]) for x in got if x != "exact")
            r["exact_over_8bit"] = round(min(r["exact_ms_a"], r["exact_ms_b"]) / max(r["8bit_ms_a"], r["8bit_ms_b"]), 3)
            r["bf16_over_8bit"] = round(min(r["bf16_ms_a"], r["bf16_ms_b"]) / max(r["8bit_ms_a"], r["8bit_ms_b"]), 3)
            if "6bit" in got:
                r["8bit_over_6bit"] = round(min(r["8bit_ms_a"], r["8bit_ms_b"]) / max(r["6bit_ms_a"], r["6bit_ms_b"]), 3)
            rec["results"].append(r)
            print(json.dumps(r), flush=True)
        idx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
