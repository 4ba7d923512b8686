"""The wide form of the single-query bound scan (65 <= k <= 1024), measured: three arms on ONE cosine index in one process — the exact path the
search takes today (set_bound_scan_wide("never"): k_flat_scan_wide up to k = 128, the key-per-row path above), the wide form with the bfloat16
copy first, and with the 8-bit plane first ("always" with set_bound_plane "bf16" / "8bit") — at k = 65, 100, 128, 129, 256 and 1000.
Not collected by pytest, not part of bench.py.

    python tests/bench/bench_bound_scan_wide.py --rows 10000000 --dim 768 --out profiles/bound_scan_wide_10Mx768.json
    python tests/bench/bench_bound_scan_wide.py --table profiles/bound_scan_wide_*.json          # the markdown tables of the result files

Device-pointer calls on one stream (search_device: no host copy, no synchronisation inside), timed with device events around `--calls`
consecutive calls; per cell a warm-up of every arm, then `--reps` rounds with the arms alternating exact, bfloat16, 8-bit, exact, ...; a
cell's figure is the median over the rounds of the time per call, its spread their max - min.  Before a cell is timed the three arms' rows
and float32 bits are compared word for word at that size and the wide counters are read: the two wide arms must have taken the path and
handed nothing back (recorded per cell with the survivor counts; the run fails at its end if any cell says otherwise).  "wins": the arm beats
the arm it would replace (bfloat16 first: the exact path; 8-bit first: bfloat16 first) by more than both arms' spread."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

ARMS = ("exact", "bf16", "8bit")


def set_arm(idx, arm):
    idx.set_bound_scan_wide("never" if arm == "exact" else "always")
    idx.set_bound_plane("8bit" if arm == "8bit" else "bf16")


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
    result = {"rows": n, "dim": dim, "metric": "cosine", "reps": a.reps, "calls_per_rep": a.calls, "device": quiver_amd.device_index.device_info(0), "cells": []}
    for k in a.k:
        out_r = {arm: torch.full((1, k), -1, dtype=torch.int32, device="cuda") for arm in ARMS}
        out_d = {arm: torch.zeros((1, k), dtype=torch.float32, device="cuda") for arm in ARMS}

        def call(arm):
            idx.search_device(dq.data_ptr(), 1, k, out_r[arm].data_ptr(), out_d[arm].data_ptr(), stream)

        stats = {}
        for arm in ARMS:                                                   # warm-up, and the check of rows and bits at the size that is timed
            set_arm(idx, arm)
            s0 = idx.bound_scan_wide_stats()
            call(arm); call(arm)
            torch.cuda.synchronize()
            s1 = idx.bound_scan_wide_stats()
            stats[arm] = {"took": s1["searches"] - s0["searches"], "back": s1["hand_backs"] - s0["hand_backs"], "survivors": s1["candidates"]}
        same = all(torch.equal(out_r[arm], out_r["exact"]) and torch.equal(out_d[arm].view(torch.int32), out_d["exact"].view(torch.int32)) for arm in ARMS)
        took = bool(stats["exact"]["took"] == 0 and all(stats[arm]["took"] == 2 and stats[arm]["back"] == 0 for arm in ("bf16", "8bit")))
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
        cell = {"k": k, "same_rows_and_bits": same, "wide_arms_took_the_path_and_decided": took, "stats": stats}
        for arm in ARMS:
            v = us[arm]
            cell[arm] = {"us": float(np.median(v)), "min_us": min(v), "max_us": max(v), "spread_us": max(v) - min(v)}
        cell["bf16_wins"] = bool(cell["exact"]["us"] - cell["bf16"]["us"] > max(cell["exact"]["spread_us"], cell["bf16"]["spread_us"]))
        cell["8bit_wins"] = bool(cell["bf16"]["us"] - cell["8bit"]["us"] > max(cell["bf16"]["spread_us"], cell["8bit"]["spread_us"]))
        cell["8bit_beats_exact"] = bool(cell["exact"]["us"] - cell["8bit"]["us"] > max(cell["exact"]["spread_us"], cell["8bit"]["spread_us"]))
        result["cells"].append(cell)
        print(json.dumps({kk: (vv if kk not in ARMS else round(vv["us"], 1)) for kk, vv in cell.items()}), flush=True)
    idx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    bad = [c["k"] for c in result["cells"] if not (c["same_rows_and_bits"] and c["wide_arms_took_the_path_and_decided"])]
    assert not bad, ("cells whose arms differ in rows or bits, or whose wide arms did not take the path", bad)


def table(inputs):
    for p in inputs:
        r = json.load(open(p))
        print("\n%d x %d, us per call: median (spread) of %d rounds of %d calls\n" % (r["rows"], r["dim"], r["reps"], r["calls_per_rep"]))
        print("| k | exact | bfloat16 first | 8-bit first | bfloat16 beats exact | 8-bit beats bfloat16 | 8-bit beats exact | survivors bf16 / 8-bit |")
        print("|---|---|---|---|---|---|---|---|")
        for c in r["cells"]:
            print("| %d | %.0f (%.0f) | %.0f (%.0f) | %.0f (%.0f) | %s | %s | %s | %d / %d |" % (
                c["k"], c["exact"]["us"], c["exact"]["spread_us"], c["bf16"]["us"], c["bf16"]["spread_us"], c["8bit"]["us"], c["8bit"]["spread_us"],
                "yes" if c["bf16_wins"] else "no", "yes" if c["8bit_wins"] else "no", "yes" if c["8bit_beats_exact"] else "no",
                c["stats"]["bf16"]["survivors"], c["stats"]["8bit"]["survivors"]))


def main():
    ints = lambda s: [int(x) for x in s.split(",")]                         # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=ints, default=[65, 100, 128, 129, 256, 1000])
    ap.add_argument("--reps", type=int, default=5, help="rounds per arm, the arms alternating (three at least)")
    ap.add_argument("--calls", type=int, default=20, help="consecutive calls between the two events of one round")
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
