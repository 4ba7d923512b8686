"""A filter nobody has asked before, in front of a search: the three calls the library offered (A: qv_rowset_create_where +
qv_index_search_rowsets + qv_rowset_destroy) against the one call that keeps the set in its workspace (B: qv_index_search_where).
Not collected by pytest, not part of bench.py.

    python tests/bench/bench_search_where.py --rows 1000000 --out profiles/search_where_1M.json
    python tests/bench/bench_search_where.py --rows 10000000 --out profiles/search_where_10M.json
    python tests/bench/bench_search_where.py --notes profiles/search_where_notes.md profiles/search_where_1M.json profiles/search_where_10M.json

One process, a cosine index of rows x 768 (synthetic rows), k = 10, one F64 column of uniform values in [0, 1) and a range predicate
`value < literal` whose literal changes on EVERY request (about 10 % and about 100 % of the rows).  1, 8 and 64 concurrent callers,
each a closed loop of single-query calls.  The callers are PYTHON threads: tools/native/qv_callers.cpp has loops for
qv_index_search and qv_index_search_rowsets only, so both arms pay the interpreter's share per call (ctypes releases the lock
inside the library) — arm A three times per request, arm B once, which is how a Python host would pay it too.
Per shape: a warm-up window of each arm, then `--reps` repetitions, the arms alternating A, B, A, B, ...; per repetition the
per-call p50 and the calls per second over the window (host clock around calls that end in a synchronise).  The criterion:
B's p50 (median over the repetitions) is not above A's by more than A's own min-max spread over its repetitions."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

DIM, K = 768, 10
HAND = "<!-- below this line: written by hand, kept when the tables are regenerated -->"


def window(fn, callers, seconds):
    """`callers` threads, each calling fn(thread, i) in a closed loop for `seconds` -> (per-call latencies in ms, calls per second)"""
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
                fn(t, i)
                lat[t].append((time.perf_counter() - t0) * 1e3)
                i += 1
        except Exception as e:                                                      # noqa: BLE001
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
    return flat, flat.size / wall


def measure(a):
    import quiver_amd
    n = a.rows
    idx = quiver_amd.DeviceIndex(DIM, "cosine")
    idx.add_synthetic(20260701, 0, n)
    rng = np.random.default_rng(20260702)
    vals = rng.random(n)
    col = idx.column("f64")
    col.set(0, vals)
    qs = np.random.default_rng(20260703).standard_normal((64, DIM)).astype(np.float32)

    def literal(base, t, i):                                                        # never the same twice within a window, the selectivity unchanged
        return base + 1e-9 * (1 + t * 100_003 + i)

    def arm_a(base):
        def fn(t, i):
            rs = idx.rowset_where([(col, "lt", literal(base, t, i))])
            try:
                return idx.search_rowsets(qs[t:t + 1], K, rs)
            finally:
                rs.close()
        return fn

    def arm_b(base):
        def fn(t, i):
            return idx.search_where(qs[t:t + 1], K, [(col, "lt", literal(base, t, i))])
        return fn

    result = {"rows": n, "dim": DIM, "k": K, "metric": "cosine", "reps": a.reps, "seconds_per_window": a.seconds, "callers_are": "python threads",
              "device": quiver_amd.device_index.device_info(0), "shapes": []}
    for sel_name, base in (("10pct", 0.1), ("100pct", 1.0)):
        ra, rb = arm_a(base)(0, 0), arm_b(base)(0, 0)                               # the two paths answer alike at the size that is timed
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb))
        for callers in a.callers:
            A, B = arm_a(base), arm_b(base)
            window(A, callers, min(a.seconds, 0.3)); window(B, callers, min(a.seconds, 0.3))      # warm-up: buffers grown, contexts made
            st0 = idx.rowset_coalesce_stats()
            reps = {"A": [], "B": []}
            for _ in range(a.reps):
                for name, fn in (("A", A), ("B", B)):
                    lat, qps = window(fn, callers, a.seconds)
                    reps[name].append({"p50_ms": float(np.percentile(lat, 50)), "p90_ms": float(np.percentile(lat, 90)), "qps": qps, "calls": int(lat.size)})
            st1 = idx.rowset_coalesce_stats()
            shape = {"selectivity": sel_name, "selected_fraction": float((vals < base).mean()), "callers": callers,
                     "shared_passes": st1["groups"] - st0["groups"], "queries_in_shared_passes": st1["group_queries"] - st0["group_queries"]}
            for name in ("A", "B"):
                p50 = [r["p50_ms"] for r in reps[name]]
                shape[name] = {"reps": reps[name], "p50_ms": float(np.median(p50)), "p50_min_ms": min(p50), "p50_max_ms": max(p50),
                               "qps": float(np.median([r["qps"] for r in reps[name]]))}
            spread = shape["A"]["p50_max_ms"] - shape["A"]["p50_min_ms"]
            shape["a_spread_ms"] = spread
            shape["b_not_above_a_plus_spread"] = bool(shape["B"]["p50_ms"] <= shape["A"]["p50_ms"] + spread)
            result["shapes"].append(shape)
            print(json.dumps({k: (v if k not in ("A", "B") else {kk: vv for kk, vv in v.items() if kk != "reps"}) for k, v in shape.items()}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


def notes(path, inputs):
    out = ["# Filtered search by predicate in one call: what was measured", "",
           "`tests/bench/bench_search_where.py` on one MI355X, one process per size: a cosine index of rows x 768, k = 10, one F64 range",
           "predicate whose literal changes on every request.  A = `rowset_where` + `search_rowsets` + close (three calls, the first with an",
           "allocation, a pass on the null stream, a download of rows / 8 bytes and a synchronisation); B = `search_where` (one call, the set",
           "in the call's workspace).  Callers are Python threads (the native caller loops of `libqvcallers` cover `qv_index_search` and",
           "`qv_index_search_rowsets` only), each a closed loop of single-query calls; per shape a warm-up window of each arm, then the",
           "repetitions interleaved A, B, A, B, ...  p50 = the median over the repetitions of the per-call p50 of a window; spread = A's own",
           "max - min of that p50 over its repetitions; QPS = calls per second of a window, median over the repetitions."]
    losses = []
    for p in inputs:
        r = json.load(open(p))
        out += ["", "| rows | selected | callers | A p50 ms (min - max) | B p50 ms (min - max) | A QPS | B QPS | B / A QPS | shared passes | B <= A + spread |",
                "|---|---|---|---|---|---|---|---|---|---|"]
        for s in r["shapes"]:
            A, B = s["A"], s["B"]
            ok = s["b_not_above_a_plus_spread"]
            out.append("| %s | %s | %d | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.0f | %.0f | %.2f | %d | %s |" % (
                "%dM" % (r["rows"] // 1_000_000), s["selectivity"].replace("pct", " %"), s["callers"], A["p50_ms"], A["p50_min_ms"], A["p50_max_ms"],
                B["p50_ms"], B["p50_min_ms"], B["p50_max_ms"], A["qps"], B["qps"], B["qps"] / A["qps"], s["shared_passes"], "yes" if ok else "**no: a loss**"))
            if not ok:
                losses.append("%dM rows, %s selected, %d callers: B %.3f ms against A %.3f ms (A's spread %.3f ms)" % (
                    r["rows"] // 1_000_000, s["selectivity"].replace("pct", " %"), s["callers"], B["p50_ms"], A["p50_ms"], s["a_spread_ms"]))
        out.append("")
        out.append("(%d repetitions of %.1f s per arm and shape at %d rows.)" % (r["reps"], r["seconds_per_window"], r["rows"]))
    out += ["", "## Losses", ""]
    out += ["- " + x for x in losses] if losses else ["None: at every shape B's p50 is within A's p50 plus A's own spread."]
    out += ["", HAND]
    kept = ""
    if os.path.exists(path):                                                        # what was written by hand below the marker stays
        text = open(path).read()
        if HAND in text:
            kept = text.split(HAND, 1)[1]
    with open(path, "w") as f:
        f.write("\n".join(out) + (kept if kept else "\n"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5, help="length of one timed window")
    ap.add_argument("--callers", type=lambda s: [int(x) for x in s.split(",")], default=[1, 8, 64])
    ap.add_argument("--out", default="")
    ap.add_argument("--notes", default="", help="write the notes file from the result files given as positional arguments instead of measuring")
    ap.add_argument("inputs", nargs="*")
    a = ap.parse_args()
    if a.notes:
        return notes(a.notes, a.inputs)
    measure(a)


if __name__ == "__main__":
    main()
