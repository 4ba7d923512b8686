"""The bound scan on a Euclidean index created with QV_FLAG_L2_SCAN_PLANE, measured: three arms on ONE index in one process — the exact scan
(set_bound_scan("never")), the bound scan with the bfloat16 copy first, and with the 8-bit plane first ("always", all four plane knobs set
alike) — for 1, 2, 4 and 8 queries per call, k = 1, 10 and 64, unfiltered and under one where-filter that selects 10 % of the rows.
Not collected by pytest, not part of bench.py.

    python tests/bench/bench_bound_scan_l2.py --rows 10000000 --dim 768 --out profiles/bound_scan_l2_10Mx768.json
    python tests/bench/bench_bound_scan_l2.py --table profiles/bound_scan_l2_*.json          # the markdown tables of the result files

Device-pointer calls on one stream (search_device / search_where_device: no host copy, no synchronisation inside), timed with device
events around `--calls` consecutive calls; per cell a warm-up of every arm, then `--reps` repetitions with the arms alternating exact,
bfloat16, 8-bit, exact, ...; a cell's figure is the median over the repetitions of the time per call, its spread their max - min.  Before
a cell is timed the three arms' rows and float32 bits are compared word for word at that size and the counters are read: the two bound
arms must have taken the path and handed nothing back (recorded per cell; the run fails at its end if any cell says otherwise).  "wins": the arm beats the arm it would replace (bfloat16 first: the exact scan; 8-bit
first: bfloat16 first) by more than both arms' spread."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

ARMS = ("exact", "bf16", "8bit")


def set_arm(idx, arm):
    idx.set_bound_scan("never" if arm == "exact" else "always")
    for setter in (idx.set_bound_plane, idx.set_bound_plane_filtered, idx.set_bound_plane_mq, idx.set_bound_plane_filtered_mq):
        setter("bf16" if arm != "8bit" else "8bit")


def measure(a):
    import torch
    import quiver_amd
    n, dim = a.rows, a.dim
    idx = quiver_amd.DeviceIndex(dim, "l2", l2_scan_plane=True)
    idx.add_synthetic(20261001, 0, n)
    assert idx.bound_scan_stats()["plane"] and idx.bound_scan8_stats()["plane"]
    col = idx.column("f64")
    col.set(0, np.random.default_rng(20261002).random(n))
    where = [(col, "lt", 0.1)]
    from tests import _oracle as O
    qs = O.gen_rows(20261003, 0, 8, dim)
    dq = torch.from_numpy(qs).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    result = {"rows": n, "dim": dim, "metric": "l2", "reps": a.reps, "calls_per_rep": a.calls, "device": quiver_amd.device_index.device_info(0), "cells": []}
    for filt in ("none", "where10"):
        for nq in a.nq:
            for k in a.k:
                out_r = {arm: torch.full((nq, k), -1, dtype=torch.int32, device="cuda") for arm in ARMS}
                out_d = {arm: torch.zeros((nq, k), dtype=torch.float32, device="cuda") for arm in ARMS}

                def call(arm):
                    if filt == "none":
                        idx.search_device(dq.data_ptr(), nq, k, out_r[arm].data_ptr(), out_d[arm].data_ptr(), stream)
                    else:
                        idx.search_where_device(dq.data_ptr(), nq, k, where, out_r[arm].data_ptr(), out_d[arm].data_ptr(), stream)

                stats = {}
                for arm in ARMS:                                           # warm-up, and the check of rows and bits at the size that is timed
                    set_arm(idx, arm)
                    s0, a0 = idx.bound_scan_stats(), idx.bound_scan8_stats()
                    call(arm); call(arm)
                    torch.cuda.synchronize()
                    s1, a1 = idx.bound_scan_stats(), idx.bound_scan8_stats()
                    stats[arm] = {"took": s1["searches"] - s0["searches"], "back": s1["hand_backs"] - s0["hand_backs"], "survivors": s1["candidates"],
                                  "took8": a1["searches"] - a0["searches"], "back8": a1["hand_backs"] - a0["hand_backs"], "survivors8": a1["candidates"]}
                same = all(torch.equal(out_r[arm], out_r["exact"]) and torch.equal(out_d[arm].view(torch.int32), out_d["exact"].view(torch.int32)) for arm in ARMS)
                took = bool(stats["exact"]["took"] == 0 and stats["bf16"]["took"] == 2 * nq and stats["bf16"]["back"] == 0 and
                            stats["8bit"]["took8"] == 2 * nq and stats["8bit"]["back8"] == 0)
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
                cell = {"filter": filt, "nq": nq, "k": k, "same_rows_and_bits": same, "bound_arms_took_the_path_and_decided": took, "stats": stats}
                for arm in ARMS:
                    v = us[arm]
                    cell[arm] = {"us": float(np.median(v)), "min_us": min(v), "max_us": max(v), "spread_us": max(v) - min(v)}
                cell["bf16_wins"] = bool(cell["exact"]["us"] - cell["bf16"]["us"] > max(cell["exact"]["spread_us"], cell["bf16"]["spread_us"]))
                cell["8bit_wins"] = bool(cell["bf16"]["us"] - cell["8bit"]["us"] > max(cell["bf16"]["spread_us"], cell["8bit"]["spread_us"]))
                result["cells"].append(cell)
                print(json.dumps({kk: (vv if kk not in ARMS else round(vv["us"], 1)) for kk, vv in cell.items() if kk != "stats"}), flush=True)
    idx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    bad = [(c["filter"], c["nq"], c["k"]) for c in result["cells"] if not (c["same_rows_and_bits"] and c["bound_arms_took_the_path_and_decided"])]
    assert not bad, ("cells whose arms differ in rows or bits, or whose bound arms did not take the path", bad)


def table(inputs):
    for p in inputs:
        r = json.load(open(p))
        print("\n%d x %d, us per call: median (spread) of %d repetitions of %d calls\n" % (r["rows"], r["dim"], r["reps"], r["calls_per_rep"]))
        print("| filter | nq | k | exact | bfloat16 first | 8-bit first | bfloat16 beats exact | 8-bit beats bfloat16 | survivors bf16 / 8-bit |")
        print("|---|---|---|---|---|---|---|---|---|")
        for c in r["cells"]:
            print("| %s | %d | %d | %.0f (%.0f) | %.0f (%.0f) | %.0f (%.0f) | %s | %s | %d / %d |" % (
                c["filter"], c["nq"], c["k"], c["exact"]["us"], c["exact"]["spread_us"], c["bf16"]["us"], c["bf16"]["spread_us"], c["8bit"]["us"], c["8bit"]["spread_us"],
                "yes" if c["bf16_wins"] else "no", "yes" if c["8bit_wins"] else "no", c["stats"]["bf16"]["survivors"], c["stats"]["8bit"]["survivors8"]))


def main():
    ints = lambda s: [int(x) for x in s.split(",")]                         # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=ints, default=[1, 2, 4, 8])
    ap.add_argument("--k", type=ints, default=[1, 10, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="consecutive calls between the two events of one repetition")
    ap.add_argument("--out", default="")
    ap.add_argument("--table", action="store_true", help="print the markdown tables of the result files given as positional arguments instead of measuring")
    ap.add_argument("inputs", nargs="*")
    a = ap.parse_args()
    if a.table:
        return table(a.inputs)
    measure(a)


if __name__ == "__main__":
    main()
