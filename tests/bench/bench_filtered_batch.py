"""Filtered calls of 16 / 64 / 256 queries, a filter per query: the exact row-set passes ("never") against the batched path with a set per
query ("always", qv_index_set_filtered_batch).  Not collected by pytest, not part of bench.py.

    python tests/bench/bench_filtered_batch.py --rows 1000000 --dim 768 --metric cosine --out profiles/filtered_batch_1Mx768_cosine.json
    python tests/bench/bench_filtered_batch.py --table profiles/filtered_batch_*.json          # markdown tables of result files

One process per shape: an index of rows x dim (synthetic rows), one F64 column of uniform values.  Per cell — k, nq, a kind of filter —
one call of nq queries is timed on the host clock (the call ends in a synchronise): a warm-up call of each arm, then `--reps`
repetitions, the arms alternating never, always, never, always, ...; a repetition is the median of `--calls` calls.  A cell reports each
arm's median over the repetitions and its min-max spread, and what the batched arm handed back.  Kinds of filter:
  distinct <share>   a random set per query holding that share of the rows
  shared <share>     one such set named by every query
  striped <share>    one set of whole 64-row tiles, every (1 / share)-th tile, named by every query
  where <share>      a range predicate per query on the column selecting that share (its literal differs per query)
Both arms' answers are compared once per cell: a difference is an error, not a figure."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def filters_of(idx, col, n, nq, kind, share, rng):
    """-> (call, owned sets): call(qs, k) runs the search"""
    if kind == "where":
        fl = [[(col, "ge", (1.0 - share) * q / max(nq, 1)), (col, "lt", (1.0 - share) * q / max(nq, 1) + share + (1.0 if share >= 1.0 else 0.0))] for q in range(nq)]
        return (lambda qs, k: idx.search_where(qs, k, fl)), []
    if kind == "distinct":
        sets = [idx.rowset(rng.random(n) < share) for _ in range(nq)]
        return (lambda qs, k: idx.search_rowsets(qs, k, sets)), sets
    if kind == "shared":
        m = rng.random(n) < share
    else:                                                                 # striped
        m = (np.arange(n) // 64) % max(1, int(round(1.0 / share))) == 0
    s = idx.rowset(m)
    return (lambda qs, k: idx.search_rowsets(qs, k, [s] * nq)), [s]


def measure(a):
    import quiver_amd
    n = a.rows
    idx = quiver_amd.DeviceIndex(a.dim, a.metric)
    idx.add_synthetic(20261001, 0, n)
    rng = np.random.default_rng(20261002)
    col = idx.column("f64")
    col.set(0, rng.random(n))
    qs_all = np.random.default_rng(20261003).standard_normal((max(a.nq), a.dim)).astype(np.float32)
    result = {"rows": n, "dim": a.dim, "metric": a.metric, "reps": a.reps, "calls_per_rep": a.calls, "sparse_ppm": a.sparse_ppm,
              "device": quiver_amd.device_index.device_info(0), "cells": []}
    cells = [("distinct", s) for s in a.shares] + [("shared", s) for s in a.shares if s < 1.0] + [("striped", s) for s in a.shares if s < 1.0] + [("where", s) for s in a.where]
    for kind, share in cells:
        for nq in a.nq:
            call, owned = filters_of(idx, col, n, nq, kind, share, rng)
            qs = qs_all[:nq]
            for k in a.k:
                def arm(mode):
                    idx.set_filtered_batch(mode, a.sparse_ppm)
                    t = []
                    for _ in range(a.calls):
                        t0 = time.perf_counter(); call(qs, k); t.append((time.perf_counter() - t0) * 1e6)
                    return float(np.median(t))
                idx.set_filtered_batch("never"); ref = call(qs, k)
                idx.set_filtered_batch("always", a.sparse_ppm); s0 = idx.filtered_batch_stats(); got = call(qs, k); s1 = idx.filtered_batch_stats()
                if not all(x.tobytes() == y.tobytes() for x, y in zip(ref, got)):
                    raise SystemExit("the arms differ at %s" % ((kind, share, nq, k),))
                reps = {"never": [], "always": []}
                for _ in range(a.reps):
                    for mode in ("never", "always"):
                        reps[mode].append(arm(mode))
                cell = {"kind": kind, "share": share, "nq": nq, "k": k, "took_path": s1["queries"] - s0["queries"],
                        "handed_back": s1["hand_backs"] - s0["hand_backs"], "sparse": s1["sparse"] - s0["sparse"]}
                for mode in ("never", "always"):
                    cell[mode] = {"us": float(np.median(reps[mode])), "min_us": min(reps[mode]), "max_us": max(reps[mode])}
                spread = max(cell["never"]["max_us"] - cell["never"]["min_us"], cell["always"]["max_us"] - cell["always"]["min_us"])
                cell["spread_us"] = spread
                cell["always_wins"] = bool(cell["always"]["max_us"] + spread < cell["never"]["min_us"])     # the slower batched round against the faster exact round
                cell["always_loses"] = bool(cell["always"]["min_us"] > cell["never"]["max_us"] + spread)
                result["cells"].append(cell)
                print(json.dumps(cell), flush=True)
            for s in owned:
                s.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


def table(paths):
    for p in paths:
        r = json.load(open(p))
        print("\n### %d x %d, %s (%d repetitions of %d calls; floor %s ppm)\n" % (r["rows"], r["dim"], r["metric"], r["reps"], r["calls_per_rep"],
                                                                                 "default" if r["sparse_ppm"] is None else r["sparse_ppm"]))
        print("| filter | share | nq | k | never us (min - max) | always us (min - max) | never / always | took / back / sparse | verdict |")
        print("|---|---|---|---|---|---|---|---|---|")
        for c in r["cells"]:
            nv, al = c["never"], c["always"]
            print("| %s | %g | %d | %d | %.0f (%.0f - %.0f) | %.0f (%.0f - %.0f) | %.2f | %d / %d / %d | %s |" % (
                c["kind"], c["share"], c["nq"], c["k"], nv["us"], nv["min_us"], nv["max_us"], al["us"], al["min_us"], al["max_us"], nv["us"] / al["us"],
                c["took_path"], c["handed_back"], c["sparse"], "win" if c["always_wins"] else ("**loss**" if c["always_loses"] else "level")))


def main():
    ap = argparse.ArgumentParser()
    flist = lambda s: [float(x) for x in s.split(",") if x]               # noqa: E731
    ilist = lambda s: [int(x) for x in s.split(",") if x]                 # noqa: E731
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--metric", default="cosine")
    ap.add_argument("--k", type=ilist, default=[10, 64])
    ap.add_argument("--nq", type=ilist, default=[16, 64, 256])
    ap.add_argument("--shares", type=flist, default=[1.0, 0.5, 0.25, 0.1, 0.05, 0.01])
    ap.add_argument("--where", type=flist, default=[1.0, 0.1, 0.01])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--sparse-ppm", type=int, default=None, help="the sparse floor of the batched arm (default: the library's; 0: never hand back as sparse)")
    ap.add_argument("--out", default="")
    ap.add_argument("--table", nargs="*", default=None, help="print markdown tables of these result files instead of measuring")
    a = ap.parse_args()
    if a.table is not None:
        return table(a.table)
    measure(a)


if __name__ == "__main__":
    main()
