"""The int8 filter's panel kernel (1056 to 4096 dimensions) against what such an index runs without it, set_filter("auto"), on ONE index in ONE
process (a measurement, not a test).

  python tests/bench/bench_int8_wide.py --rows 1000000 --dim 1536 --nq 40,64,256 --k 10,64 [--out FILE.json]

Per cell (nq, k): five rounds that alternate set_filter("auto") and set_filter("int8"), 20 device-pointer calls each, us per batch as the
rounds' median with their spread; the int8 arm's batches and hand-backs (int8_filter_stats); and whether both arms returned the same rows and
float32 bits.  One JSON line per cell.  The kernels' own times come from a separate rocprofv3 --kernel-trace --stats run of this script."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--nq", default="40,64,256")
    ap.add_argument("--k", default="10,64")
    ap.add_argument("--metric", default="cosine")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import quiver_amd as q
    from tests import _oracle as O
    idx = q.DeviceIndex(a.dim, a.metric)
    idx.add_synthetic(20260424, 0, a.rows)
    stream = torch.cuda.current_stream().cuda_stream
    lines = []
    for nq in [int(x) for x in a.nq.split(",")]:
        for k in [int(x) for x in a.k.split(",")]:
            dq = torch.from_numpy(O.gen_rows(20260425, 0, nq, a.dim)).cuda()
            out = {f: (torch.empty((nq, k), dtype=torch.int32, device="cuda"), torch.empty((nq, k), dtype=torch.float32, device="cuda"),
                       torch.zeros((nq,), dtype=torch.int32, device="cuda")) for f in ("auto", "int8")}

            def run(f, calls):
                idx.set_filter(f)
                r, d, fl = out[f]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    idx.search_batched_device(dq.data_ptr(), nq, k, r.data_ptr(), d.data_ptr(), fl.data_ptr(), stream)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / calls * 1e6

            for f in out:
                run(f, 3)                                        # warm-up: workspaces, code objects
            s0 = idx.int8_filter_stats()
            us = {f: [] for f in out}
            for _ in range(a.rounds):
                for f in out:
                    us[f].append(run(f, a.calls))
            s1 = idx.int8_filter_stats()
            done = {f: int(out[f][2].sum().item()) == 0 for f in out}       # (a handed-back query's answer is the caller's redo: not compared)
            same = bool(torch.equal(out["auto"][0], out["int8"][0]) and torch.equal(out["auto"][1].view(torch.int32), out["int8"][1].view(torch.int32)))
            line = {"rows": a.rows, "dim": a.dim, "metric": a.metric, "nq": nq, "k": k,
                    "us": {f: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for f, v in us.items()},
                    "int8_batches": s1[0] - s0[0], "int8_hand_backs": s1[2] - s0[2], "no_hand_backs": done, "same_rows_and_bits": same}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
