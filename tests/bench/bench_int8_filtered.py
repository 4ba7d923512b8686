"""A filtered call's three ways through ONE index in ONE process (a measurement, not a test): the exact filtered passes, the filtered batch on its
present filter, and the filtered batch on the int8 kernel's sets form.

  python tests/bench/bench_int8_filtered.py --rows 1000000 --dim 768 --nq 16,64,256 --k 10 --sets all,25,1,where10,stripe20,stripe100 [--out FILE.json]

Sets: "all" / "25" / "1" — a random set per query of that percentage of the rows; "where10" — a where-filter per query that passes 10 %; "stripe20" /
"stripe100" — ONE set of whole tiles, one in 20 or in 100, named by every query.  Per cell (nq, k, sets): rounds that alternate the three arms,
`calls` host calls each, us per call as the rounds' median with their spread; the tile visits the sets form skipped; whether all arms returned the
same rows and float32 bits.  The sparse floor is off in every arm.  One JSON line per cell.  The kernels' own times come from a separate
rocprofv3 --kernel-trace --stats run of this script."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

ARMS = {"exact": ("never", "never"), "batch": ("always", "never"), "batch_int8": ("always", "always")}


def make_filters(idx, kind, nq, n, rng, col, val):
    """-> (search method's name, its per-query filters)"""
    if kind.startswith("stripe"):
        m = np.zeros(n, bool)
        for t in range(0, (n + 63) // 64, int(kind[6:])):
            m[64 * t: 64 * t + 64] = True
        return "search_rowsets", [idx.rowset(m)] * nq
    if kind.startswith("where"):
        w = int(kind[5:]) / 100.0
        return "search_where", [[(col, "ge", (0.013 * q) % (1.0 - w)), (col, "lt", (0.013 * q) % (1.0 - w) + w)] for q in range(nq)]
    share = 1.0 if kind == "all" else int(kind) / 100.0
    return "search_rowsets", [idx.rowset(rng.random(n) < share) for _ in range(nq)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", default="16,64,256")
    ap.add_argument("--k", default="10")
    ap.add_argument("--sets", default="all,25,1,where10,stripe20,stripe100")
    ap.add_argument("--metric", default="cosine")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import quiver_amd as q
    from tests import _oracle as O
    idx = q.DeviceIndex(a.dim, a.metric)
    idx.add_synthetic(20260424, 0, a.rows)
    idx.set_filter("int8")
    rng = np.random.default_rng(20260426)
    val = rng.random(a.rows)
    col = idx.column("f64"); col.set(0, val, None)
    lines = []
    for nq in [int(x) for x in a.nq.split(",")]:
        qs = O.gen_rows(20260425, 0, nq, a.dim)
        for kind in a.sets.split(","):
            method, filters = make_filters(idx, kind, nq, a.rows, rng, col, val)
            for k in [int(x) for x in a.k.split(",")]:
                out = {}

                def run(f, calls):
                    idx.set_filtered_batch(ARMS[f][0], sparse_ppm=0)
                    idx.set_filtered_batch_wide(ARMS[f][0] if k > 64 else "auto")
                    idx.set_int8_filtered(ARMS[f][1])
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        out[f] = getattr(idx, method)(qs, k, filters)
                    return (time.perf_counter() - t0) / calls * 1e6

                for f in ARMS:
                    run(f, 2)                                    # warm-up: workspaces, code objects
                s0 = idx.int8_filtered_stats()
                us = {f: [] for f in ARMS}
                for _ in range(a.rounds):
                    for f in ARMS:
                        us[f].append(run(f, a.calls))
                s1 = idx.int8_filtered_stats()
                ref = out["exact"]
                same = all(np.array_equal(ref[0], out[f][0]) and np.array_equal(ref[1].view(np.uint32), out[f][1].view(np.uint32)) for f in ARMS)
                line = {"rows": a.rows, "dim": a.dim, "metric": a.metric, "nq": nq, "k": k, "sets": kind,
                        "us": {f: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for f, v in us.items()},
                        "int8_batches": s1[0] - s0[0], "visits_skipped": s1[2] - s0[2], "visits_possible": s1[3] - s0[3], "same_rows_and_bits": same}
                print(json.dumps(line), flush=True)
                lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
