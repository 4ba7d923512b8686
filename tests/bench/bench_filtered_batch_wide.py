"""Filtered calls of 16 / 64 / 256 queries that want 100 or 1000 results each, a filter per query — three arms in ONE process, alternating:
  runs     today's default: runs of queries naming one set, each through the single-query paths (every wide setter at "never")
  wide_mq  today's best: pieces of at most 8 on the filtered wide shared pass (qv_index_set_bound_scan_wide_filtered_mq "always")
  batched  the batched path with a set per query and the large-k funnel (qv_index_set_filtered_batch_wide "always")
Not collected by pytest, not part of bench.py.

    python tests/bench/bench_filtered_batch_wide.py --rows 1000000 --out profiles/filtered_batch_wide_1Mx768.json
    python tests/bench/bench_filtered_batch_wide.py --table profiles/filtered_batch_wide_*.json

Per cell (a kind of filter, nq, k): the arms' answers are compared (a difference is an error, not a figure), each arm is warmed up, then
`--rounds` rounds run the three arms one after the other; a round's figure is the median of `--calls` calls on the host clock (a call ends
in a synchronise).  A cell reports each arm's median over the rounds and its min - max, and what the batched arm handed back.  "win": the
batched arm's slowest round is faster than BOTH other arms' fastest round by more than the largest of the three spreads — the only cells
the automatic mode may ever take.  Filters: distinct <share> = a random set per query; where <share> = a range predicate per query on a
uniform column; striped 0.05 = ONE set of whole 64-row tiles, one in twenty, named by every query."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ARMS = ("runs", "wide_mq", "batched")
CELLS = (("distinct", 1.0), ("distinct", 0.25), ("distinct", 0.01), ("where", 0.1), ("striped", 0.05))


def measure(a):
    import quiver_amd
    n = a.rows
    idx = quiver_amd.DeviceIndex(a.dim, a.metric)
    idx.add_synthetic(20261101, 0, n)
    rng = np.random.default_rng(20261102)
    col = idx.column("f64")
    col.set(0, rng.random(n))
    qs_all = np.random.default_rng(20261103).standard_normal((max(a.nq), a.dim)).astype(np.float32)
    result = {"rows": n, "dim": a.dim, "metric": a.metric, "rounds": a.rounds, "calls_per_round": a.calls, "device": quiver_amd.device_index.device_info(0), "cells": []}

    def arm(name):
        idx.set_bound_scan_wide_filtered_mq("always" if name == "wide_mq" else "never")
        idx.set_filtered_batch_wide("always" if name == "batched" else "never")

    for kind, share in CELLS:
        for nq in a.nq:
            owned = []
            if kind == "where":
                fl = [[(col, "ge", (1.0 - share) * q / nq), (col, "lt", (1.0 - share) * q / nq + share)] for q in range(nq)]
                call = lambda qs, k: idx.search_where(qs, k, fl)         # noqa: E731
            else:
                owned = [idx.rowset(rng.random(n) < share) for _ in range(nq)] if kind == "distinct" else [idx.rowset((np.arange(n) // 64) % 20 == 0)] * nq
                call = lambda qs, k: idx.search_rowsets(qs, k, owned)    # noqa: E731
            qs = qs_all[:nq]
            for k in a.k:
                out, moved = {}, {}
                for name in ARMS:                                         # warm-up and comparison
                    arm(name)
                    s0 = idx.filtered_batch_stats(); out[name] = call(qs, k); s1 = idx.filtered_batch_stats()
                    moved[name] = {key: s1[key] - s0[key] for key in s0}
                    if not all(x.tobytes() == y.tobytes() for x, y in zip(out["runs"], out[name])):
                        raise SystemExit("arm %s differs from the runs at %s" % (name, (kind, share, nq, k)))
                t = {name: [] for name in ARMS}
                for _ in range(a.rounds):
                    for name in ARMS:
                        arm(name)
                        one = []
                        for _ in range(a.calls):
                            t0 = time.perf_counter(); call(qs, k); one.append((time.perf_counter() - t0) * 1e6)
                        t[name].append(float(np.median(one)))
                cell = {"kind": kind, "share": share, "nq": nq, "k": k, "took_path": moved["batched"]["queries"], "handed_back": moved["batched"]["hand_backs"], "sparse": moved["batched"]["sparse"]}
                for name in ARMS:
                    cell[name] = {"us": float(np.median(t[name])), "min_us": min(t[name]), "max_us": max(t[name])}
                spread = max(cell[name]["max_us"] - cell[name]["min_us"] for name in ARMS)
                cell["spread_us"] = spread
                cell["batched_wins"] = bool(cell["batched"]["max_us"] + spread < min(cell["runs"]["min_us"], cell["wide_mq"]["min_us"]))
                cell["batched_loses"] = bool(cell["batched"]["min_us"] > min(cell["runs"]["max_us"], cell["wide_mq"]["max_us"]) + spread)
                result["cells"].append(cell)
                print(json.dumps(cell), flush=True)
                if a.out:                                                 # (kept as the cells come: a visit that ends early keeps what it measured)
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "w") as f:
                        json.dump(result, f, indent=1); f.write("\n")
            for s in set(owned):
                s.close()


def table(paths):
    for p in paths:
        r = json.load(open(p))
        print("\n### %d x %d, %s (%d rounds of %d calls per arm)\n" % (r["rows"], r["dim"], r["metric"], r["rounds"], r["calls_per_round"]))
        print("| filter | share | nq | k | runs us (min - max) | wide_mq us (min - max) | batched us (min - max) | best other / batched | took / back / sparse | verdict |")
        print("|---|---|---|---|---|---|---|---|---|---|")
        for c in r["cells"]:
            f = lambda x: "%.0f (%.0f - %.0f)" % (x["us"], x["min_us"], x["max_us"])   # noqa: E731
            print("| %s | %g | %d | %d | %s | %s | %s | %.2f | %d / %d / %d | %s |" % (
                c["kind"], c["share"], c["nq"], c["k"], f(c["runs"]), f(c["wide_mq"]), f(c["batched"]), min(c["runs"]["us"], c["wide_mq"]["us"]) / c["batched"]["us"],
                c["took_path"], c["handed_back"], c["sparse"], "win" if c["batched_wins"] else ("**loss**" if c["batched_loses"] else "level")))


def main():
    ap = argparse.ArgumentParser()
    ilist = lambda s: [int(x) for x in s.split(",") if x]                 # noqa: E731
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--metric", default="cosine")
    ap.add_argument("--k", type=ilist, default=[100, 1000])
    ap.add_argument("--nq", type=ilist, default=[16, 64, 256])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--table", nargs="*", default=None, help="print markdown tables of these result files instead of measuring")
    a = ap.parse_args()
    return table(a.table) if a.table is not None else measure(a)


if __name__ == "__main__":
    main()
