"""The int8 filter's two kernels against each other and against today's default, on ONE index in ONE process (a measurement, not a test).

  python tests/bench/bench_int8_shared.py --rows 1000000 --dim 768 --nq 129,256,1024 --k 10 [--bf16-rows] [--out FILE.json]

Per cell (nq, k): five rounds that alternate three arms — set_filter("bf16x1"), set_filter("int8") + set_int8_form("blocks"), set_filter("int8") +
set_int8_form("shared") — 20 device-pointer calls each, us per batch as the rounds' median with their spread; the shared arm's batches
(int8_shared_stats); and whether all arms returned the same rows and float32 bits.  One JSON line per cell.  The kernels' own times come from a
separate rocprofv3 --kernel-trace --stats run of this script."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

ARMS = {"bf16x1": ("bf16x1", "auto"), "int8_blocks": ("int8", "blocks"), "int8_shared": ("int8", "shared")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", default="129,256,1024")
    ap.add_argument("--k", default="10")
    ap.add_argument("--metric", default="cosine")
    ap.add_argument("--bf16-rows", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import quiver_amd as q
    from tests import _oracle as O
    idx = q.DeviceIndex(a.dim, a.metric, bf16_rows=a.bf16_rows)
    idx.add_synthetic(20260424, 0, a.rows)
    stream = torch.cuda.current_stream().cuda_stream
    lines = []
    for nq in [int(x) for x in a.nq.split(",")]:
        for k in [int(x) for x in a.k.split(",")]:
            dq = torch.from_numpy(O.gen_rows(20260425, 0, nq, a.dim)).cuda()
            out = {f: (torch.empty((nq, k), dtype=torch.int32, device="cuda"), torch.empty((nq, k), dtype=torch.float32, device="cuda"),
                       torch.zeros((nq,), dtype=torch.int32, device="cuda")) for f in ARMS}

            def run(f, calls):
                idx.set_filter(ARMS[f][0])
                idx.set_int8_form(ARMS[f][1])
                r, d, fl = out[f]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    idx.search_batched_device(dq.data_ptr(), nq, k, r.data_ptr(), d.data_ptr(), fl.data_ptr(), stream)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / calls * 1e6

            for f in ARMS:
                run(f, 3)                                        # warm-up: workspaces, code objects
            s0 = idx.int8_shared_stats()
            us = {f: [] for f in ARMS}
            for _ in range(a.rounds):
                for f in ARMS:
                    us[f].append(run(f, a.calls))
            s1 = idx.int8_shared_stats()
            done = {f: int(out[f][2].sum().item()) == 0 for f in ARMS}      # (a handed-back query's answer is the caller's redo: not compared)
            ref = out["bf16x1"]
            same = all(bool(torch.equal(ref[0], out[f][0]) and torch.equal(ref[1].view(torch.int32), out[f][1].view(torch.int32))) for f in ARMS)
            line = {"rows": a.rows, "dim": a.dim, "metric": a.metric, "bf16_rows": a.bf16_rows, "nq": nq, "k": k,
                    "us": {f: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for f, v in us.items()},
                    "shared_batches": s1[0] - s0[0], "shared_queries": s1[1] - s0[1], "no_hand_backs": done, "same_rows_and_bits": same}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
