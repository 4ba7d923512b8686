"""Range search against a top-k search that already knows the match count: device-pointer calls on one index in one process.

Arms: (a) qv_index_search_device at k = the radius's match count, (b) range search on the exact range scan, (c) range search starting on
the 8-bit plane.  Alternating rounds of --calls calls per arm; per cell one JSON line with each arm's median (min - max) in microseconds
per call and stage 1's survivors per query.

    python tests/bench/bench_range.py --rows 1000000 --dim 768 --rounds 5 --calls 20
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--matches", type=int, nargs="+", default=[10, 1000])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 4])
    a = ap.parse_args()
    import torch
    import quiver_amd
    from tests import _oracle as O

    idx = quiver_amd.DeviceIndex(a.dim, "cosine", device=0)
    idx.add_synthetic(20260424, 0, a.rows)
    qs = O.gen_rows(20260425, 0, max(a.nq), a.dim)
    sp = torch.cuda.current_stream().cuda_stream
    dq = torch.from_numpy(qs).cuda()
    for m in a.matches:
        # the radius that matches m rows: the m-th distance of each query
        _, dist, _ = idx.search(qs, m)
        radii = np.ascontiguousarray(dist[:, m - 1])
        dr = torch.from_numpy(radii).cuda()
        for nq in a.nq:
            rows_o = torch.zeros((nq, m), dtype=torch.int32, device="cuda")
            dist_o = torch.zeros((nq, m), dtype=torch.float32, device="cuda")
            match_o = torch.zeros(nq, dtype=torch.int64, device="cuda")

            def topk():
                idx.search_device(dq.data_ptr(), nq, m, rows_o.data_ptr(), dist_o.data_ptr(), sp)

            def ranged():
                idx.search_range_device(dq.data_ptr(), nq, dr.data_ptr(), m, rows_o.data_ptr(), dist_o.data_ptr(), match_o.data_ptr(), sp)

            arms = {"topk": (None, topk), "range_exact": ("never", ranged), "range_plane": ("always", ranged)}
            times = {name: [] for name in arms}
            for mode, fn in arms.values():                              # warm-up: workspaces, code objects
                if mode:
                    idx.set_range_plane(mode)
                fn()
            torch.cuda.synchronize()
            before = idx.range_stats()
            for _ in range(a.rounds):
                for name, (mode, fn) in arms.items():
                    if mode:
                        idx.set_range_plane(mode)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        fn()
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) / a.calls * 1e6)
            after = idx.range_stats()
            plane_queries = max(after[1] - before[1], 1)
            line = {"rows": a.rows, "dim": a.dim, "nq": nq, "matches": m, "calls": a.calls, "rounds": a.rounds,
                    "survivors_per_query": (after[3] - before[3]) / plane_queries, "handed_back": after[2] - before[2]}
            for name, t in times.items():
                line[name + "_us"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
