"""The wide form of the bound scan for ONE filtered query (65 <= k <= 1024 over a row set), measured: three arms on ONE cosine index in one
process — the path the call takes today (set_bound_scan_wide_filtered("never"): the filtered wide scan up to k = 128, the key-per-row path
above), the wide form with the bfloat16 copy first, and with the 8-bit plane first ("always" with set_bound_plane_filtered "bf16" / "8bit") — at
k = 65, 100, 128, 129, 256 and 1000, under four filters: every row selected, a random 1 % set, a random 50 % set, and a striped set of one
64-row tile in ten.  Not collected by pytest, not part of bench.py.

    python tests/bench/bench_bound_scan_wide_filtered.py --rows 10000000 --dim 768 --out profiles/bound_scan_wide_filtered_10Mx768.json
    python tests/bench/bench_bound_scan_wide_filtered.py --table profiles/bound_scan_wide_filtered_*.json      # the markdown tables of the result files

Device-pointer row-set calls on one stream (search_rowsets_device: no host copy, no synchronisation inside), timed with device events around
`--calls` consecutive calls; per cell a warm-up of every arm, then `--reps` rounds with the arms alternating never, bfloat16, 8-bit, never,
...; a cell's figure is the median over the rounds of the time per call, its spread their max - min.  Before a cell is timed the three arms'
rows and float32 bits are compared word for word at that size and the wide counters are read: whether the wide arms took the path, and how
many searches they handed back (recorded per cell with the survivor counts; the run fails at its end if any cell's arms differ or a wide arm
did not take the path).  "wins": the arm beats the arm it would replace (bfloat16 first: today's path; 8-bit first: bfloat16 first) by more
than both arms' spread.  --where adds search_where with a 10 % F64 range as a HOST call's p50 per arm (it includes the transient set's
creation, which every arm pays)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

ARMS = ("never", "bf16", "8bit")
FILTERS = ("all", "1pct", "50pct", "stripe10")


def set_arm(idx, arm):
    idx.set_bound_scan_wide_filtered("never" if arm == "never" else "always")
    idx.set_bound_plane_filtered("8bit" if arm == "8bit" else "bf16")


def mask_of(name, n, rng):
    if name == "all":
        return np.ones(n, bool)
    if name == "stripe10":
        return (np.arange(n) // 64) % 10 == 0
    return rng.random(n) < {"1pct": 0.01, "50pct": 0.5}[name]


def measure(a):
    import torch
    import quiver_amd
    n, dim = a.rows, a.dim
    idx = quiver_amd.DeviceIndex(dim, "cosine")
    idx.add_synthetic(20261021, 0, n)
    assert idx.bound_scan_wide_stats()["plane"] and idx.bound_scan8_stats()["plane"]
    from tests import _oracle as O
    q = O.gen_rows(20261022, 0, 1, dim)
    dq = torch.from_numpy(q).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(20261023)
    n_tiles = (n + 63) // 64
    result = {"rows": n, "dim": dim, "metric": "cosine", "reps": a.reps, "calls_per_rep": a.calls, "device": quiver_amd.device_index.device_info(0), "cells": [], "where": []}
    for fname in a.filters:
        m = mask_of(fname, n, rng)
        cand = int(m.sum())
        cand_tiles = int(np.count_nonzero(np.add.reduceat(m, np.arange(0, n, 64))))
        rs = idx.rowset(m)
        del m
        for k in a.k:
            if cand <= k:
                continue
            out_r = {arm: torch.full((1, k), -1, dtype=torch.int32, device="cuda") for arm in ARMS}
            out_d = {arm: torch.zeros((1, k), dtype=torch.float32, device="cuda") for arm in ARMS}

            def call(arm):
                idx.search_rowsets_device(dq.data_ptr(), 1, k, rs, out_r[arm].data_ptr(), out_d[arm].data_ptr(), stream)

            stats = {}
            for arm in ARMS:                                               # warm-up, and the check of rows and bits at the size that is timed
                set_arm(idx, arm)
                s0 = idx.bound_scan_wide_stats()
                call(arm); call(arm)
                torch.cuda.synchronize()
                s1 = idx.bound_scan_wide_stats()
                stats[arm] = {"took": s1["searches"] - s0["searches"], "back": s1["hand_backs"] - s0["hand_backs"], "survivors": s1["candidates"]}
            same = all(torch.equal(out_r[arm], out_r["never"]) and torch.equal(out_d[arm].view(torch.int32), out_d["never"].view(torch.int32)) for arm in ARMS)
            took = bool(stats["never"]["took"] == 0 and all(stats[arm]["took"] == 2 for arm in ("bf16", "8bit")))
            us = {arm: [] for arm in ARMS}
            for _ in range(a.reps):
                for arm in ARMS:
                    set_arm(idx, arm)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.calls):
                        call(arm)
                    e1.record()
                    e1.synchronize()
                    us[arm].append(e0.elapsed_time(e1) * 1e3 / a.calls)
            cell = {"filter": fname, "candidates": cand, "candidate_tiles": cand_tiles, "tiles": n_tiles, "k": k, "same_rows_and_bits": same,
                    "wide_arms_took_the_path": took, "stats": stats}
            for arm in ARMS:
                v = us[arm]
                cell[arm] = {"us": float(np.median(v)), "min_us": min(v), "max_us": max(v), "spread_us": max(v) - min(v)}
            cell["bf16_wins"] = bool(cell["never"]["us"] - cell["bf16"]["us"] > max(cell["never"]["spread_us"], cell["bf16"]["spread_us"]))
            cell["8bit_wins"] = bool(cell["bf16"]["us"] - cell["8bit"]["us"] > max(cell["bf16"]["spread_us"], cell["8bit"]["spread_us"]))
            cell["8bit_beats_never"] = bool(cell["never"]["us"] - cell["8bit"]["us"] > max(cell["never"]["spread_us"], cell["8bit"]["spread_us"]))
            result["cells"].append(cell)
            print(json.dumps({kk: (vv if kk not in ARMS else [round(vv["us"], 1), round(vv["spread_us"], 1)]) for kk, vv in cell.items()}), flush=True)
        rs.close()
    if a.where:
        vals = rng.random(n)
        col = idx.column("f64"); col.set(0, vals)
        spec = [(col, "ge", 0.45), (col, "lt", 0.55)]
        for k in a.k:
            got, ms = {}, {arm: [] for arm in ARMS}
            for arm in ARMS:
                set_arm(idx, arm)
                got[arm] = idx.search_where(q[0], k, spec)
            same = all(np.array_equal(got[arm][0], got["never"][0]) and np.array_equal(got[arm][1].view(np.uint32), got["never"][1].view(np.uint32)) for arm in ARMS)
            for _ in range(a.where):
                for arm in ARMS:
                    set_arm(idx, arm)
                    t0 = time.perf_counter()
                    idx.search_where(q[0], k, spec)
                    ms[arm].append((time.perf_counter() - t0) * 1e6)
            w = {"k": k, "same_rows_and_bits": same, "calls": a.where}
            for arm in ARMS:
                w[arm] = {"p50_us": float(np.median(ms[arm])), "min_us": min(ms[arm]), "max_us": max(ms[arm])}
            result["where"].append(w)
            print(json.dumps({"where": w}), flush=True)
        col.close()
    idx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    bad = [(c["filter"], c["k"]) for c in result["cells"] if not (c["same_rows_and_bits"] and c["wide_arms_took_the_path"])]
    bad += [("where", w["k"]) for w in result["where"] if not w["same_rows_and_bits"]]
    assert not bad, ("cells whose arms differ in rows or bits, or whose wide arms did not take the path", bad)


def table(inputs):
    for p in inputs:
        r = json.load(open(p))
        print("\n%d x %d, us per call: median (spread) of %d rounds of %d calls\n" % (r["rows"], r["dim"], r["reps"], r["calls_per_rep"]))
        print("| filter (candidate tiles / tiles) | k | today | bfloat16 first | 8-bit first | bfloat16 beats today | 8-bit beats bfloat16 | 8-bit beats today | survivors bf16 / 8-bit | handed back bf16 / 8-bit |")
        print("|---|---|---|---|---|---|---|---|---|---|")
        for c in r["cells"]:
            print("| %s (%d / %d) | %d | %.0f (%.0f) | %.0f (%.0f) | %.0f (%.0f) | %s | %s | %s | %d / %d | %d / %d |" % (
                c["filter"], c["candidate_tiles"], c["tiles"], c["k"], c["never"]["us"], c["never"]["spread_us"], c["bf16"]["us"], c["bf16"]["spread_us"],
                c["8bit"]["us"], c["8bit"]["spread_us"], "yes" if c["bf16_wins"] else "no", "yes" if c["8bit_wins"] else "no", "yes" if c["8bit_beats_never"] else "no",
                c["stats"]["bf16"]["survivors"], c["stats"]["8bit"]["survivors"], c["stats"]["bf16"]["back"], c["stats"]["8bit"]["back"]))
        if r.get("where"):
            print("\nsearch_where, a 10 % F64 range, host call p50 in us (min - max)\n\n| k | today | bfloat16 first | 8-bit first |\n|---|---|---|---|")
            for w in r["where"]:
                print("| %d | %s |" % (w["k"], " | ".join("%.0f (%.0f - %.0f)" % (w[arm]["p50_us"], w[arm]["min_us"], w[arm]["max_us"]) for arm in ARMS)))


def main():
    ints = lambda s: [int(x) for x in s.split(",")]                         # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=ints, default=[65, 100, 128, 129, 256, 1000])
    ap.add_argument("--filters", type=lambda s: s.split(","), default=list(FILTERS))
    ap.add_argument("--reps", type=int, default=5, help="rounds per arm, the arms alternating (three at least)")
    ap.add_argument("--calls", type=int, default=20, help="consecutive calls between the two events of one round")
    ap.add_argument("--where", type=int, default=0, help="host calls per arm of search_where with a 10 %% F64 range (0: not measured)")
    ap.add_argument("--out", default="")
    ap.add_argument("--table", action="store_true", help="print the markdown tables of the result files given as positional arguments instead of measuring")
    ap.add_argument("inputs", nargs="*")
    a = ap.parse_args()
    if a.table:
        return table(a.inputs)
    assert a.reps >= 3, "three rounds per arm at least"
    measure(a)


if __name__ == "__main__":
    main()
