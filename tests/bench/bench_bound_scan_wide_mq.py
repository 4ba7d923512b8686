"""The wide form of the shared bound pass (2 - 8 queries, 65 <= k <= 1024), measured: three arms on ONE cosine index in one process — the path
such a call takes today (set_bound_scan_wide_mq("never"): the key-per-row shared pass, k_flat_keys_mq + the radix selection), the form with
the bfloat16 copy first, and with the 8-bit plane first ("always" with set_bound_plane_mq "bf16" / "8bit") — at nq = 2, 4, 8 and
k = 65, 100, 128, 129, 256 and 1000.  Not collected by pytest, not part of bench.py.

    python tests/bench/bench_bound_scan_wide_mq.py --rows 10000000 --dim 768 --out profiles/bound_scan_wide_mq_10Mx768.json
    python tests/bench/bench_bound_scan_wide_mq.py --table profiles/bound_scan_wide_mq_*.json       # the markdown tables of the result files
    python tests/bench/bench_bound_scan_wide_mq.py --control never --rows 10000000 --nq 4 --k 100   # one cell of the baseline arm alone (below)

Device-pointer calls on one stream (search_device: no host copy, no synchronisation inside), timed with device events around `--calls`
consecutive calls; per cell a warm-up of every arm, then `--reps` rounds with the arms alternating never, bfloat16, 8-bit, never, ...; a
cell's figure is the median over the rounds of the time per call, its spread their max - min.  Before a cell is timed the three arms' rows
and float32 bits are compared word for word at that size and the form's counters are read: after the two warm-up calls the two forced arms
must say took = 2 nq and back = 0 (recorded per cell with the largest survivor count; the run fails at its end if any cell says otherwise).
"wins": the arm beats the arm it would replace (bfloat16 first: "never"; 8-bit first: bfloat16 first) by more than both arms' spread.

--control times ONE arm of one cell and touches nothing else: "never" sets this form's knob to never; "default" sets no knob at all, which
is all a library from before this form can run (--root names the tree whose package and library are loaded) — the two figures side by
side say whether the baseline arm is the earlier path."""
import argparse
import json
import os
import sys

import numpy as np

ARMS = ("never", "bf16", "8bit")


def set_arm(idx, arm):
    idx.set_bound_scan_wide_mq("never" if arm == "never" else "always")
    idx.set_bound_plane_mq("8bit" if arm == "8bit" else "bf16")


def timed(torch, call, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def build(a):
    import torch
    import quiver_amd
    from tests import _oracle as O
    idx = quiver_amd.DeviceIndex(a.dim, "cosine")
    idx.add_synthetic(20261021, 0, a.rows)
    assert idx.bound_scan_stats()["plane"] and idx.bound_scan8_stats()["plane"]
    qs = O.gen_rows(20261022, 0, 8, a.dim)
    return torch, quiver_amd, idx, torch.from_numpy(qs).cuda()


def measure(a):
    torch, quiver_amd, idx, dq = build(a)
    stream = torch.cuda.current_stream().cuda_stream
    result = {"rows": a.rows, "dim": a.dim, "metric": "cosine", "reps": a.reps, "calls_per_rep": a.calls, "device": quiver_amd.device_index.device_info(0), "cells": []}
    for nq in a.nq:
        for k in a.k:
            out_r = {arm: torch.full((nq, k), -1, dtype=torch.int32, device="cuda") for arm in ARMS}
            out_d = {arm: torch.zeros((nq, k), dtype=torch.float32, device="cuda") for arm in ARMS}

            def call(arm):
                idx.search_device(dq.data_ptr(), nq, k, out_r[arm].data_ptr(), out_d[arm].data_ptr(), stream)

            stats = {}
            for arm in ARMS:                                               # warm-up, and the check of rows and bits at the size that is timed
                set_arm(idx, arm)
                s0 = idx.bound_scan_wide_mq_stats()
                call(arm); call(arm)
                torch.cuda.synchronize()
                s1 = idx.bound_scan_wide_mq_stats()
                stats[arm] = {"took": s1["searches"] - s0["searches"], "back": s1["hand_backs"] - s0["hand_backs"], "survivors": s1["candidates"]}
            same = all(torch.equal(out_r[arm], out_r["never"]) and torch.equal(out_d[arm].view(torch.int32), out_d["never"].view(torch.int32)) for arm in ARMS)
            took = bool(stats["never"]["took"] == 0 and all(stats[arm]["took"] == 2 * nq and stats[arm]["back"] == 0 for arm in ("bf16", "8bit")))
            us = {arm: [] for arm in ARMS}
            for _ in range(a.reps):
                for arm in ARMS:
                    set_arm(idx, arm)
                    us[arm].append(timed(torch, lambda: call(arm), a.calls))
            cell = {"nq": nq, "k": k, "same_rows_and_bits": same, "forced_arms_took_the_path_and_decided": took, "stats": stats}
            for arm in ARMS:
                v = us[arm]
                cell[arm] = {"us": float(np.median(v)), "min_us": min(v), "max_us": max(v), "spread_us": max(v) - min(v)}
            cell["bf16_wins"] = bool(cell["never"]["us"] - cell["bf16"]["us"] > max(cell["never"]["spread_us"], cell["bf16"]["spread_us"]))
            cell["8bit_wins"] = bool(cell["bf16"]["us"] - cell["8bit"]["us"] > max(cell["bf16"]["spread_us"], cell["8bit"]["spread_us"]))
            cell["8bit_beats_never"] = bool(cell["never"]["us"] - cell["8bit"]["us"] > max(cell["never"]["spread_us"], cell["8bit"]["spread_us"]))
            result["cells"].append(cell)
            print(json.dumps({kk: (vv if kk not in ARMS else round(vv["us"], 1)) for kk, vv in cell.items()}), flush=True)
    idx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    bad = [(c["nq"], c["k"]) for c in result["cells"] if not (c["same_rows_and_bits"] and c["forced_arms_took_the_path_and_decided"])]
    assert not bad, ("cells whose arms differ in rows or bits, or whose forced arms did not take the path", bad)


def control(a):
    torch, quiver_amd, idx, dq = build(a)
    stream = torch.cuda.current_stream().cuda_stream
    nq, k = a.nq[0], a.k[0]
    if a.control == "never":
        idx.set_bound_scan_wide_mq("never")
    out_r = torch.full((nq, k), -1, dtype=torch.int32, device="cuda"); out_d = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    call = lambda: idx.search_device(dq.data_ptr(), nq, k, out_r.data_ptr(), out_d.data_ptr(), stream)   # noqa: E731
    call(); call()
    torch.cuda.synchronize()
    v = [timed(torch, call, a.calls) for _ in range(a.reps)]
    line = {"control": a.control, "root": a.root or "", "rows": a.rows, "dim": a.dim, "nq": nq, "k": k, "us": float(np.median(v)), "min_us": min(v), "max_us": max(v),
            "spread_us": max(v) - min(v), "rows_crc": int(out_r.cpu().numpy().astype(np.int64).sum()), "reps": a.reps, "calls_per_rep": a.calls}
    idx.close()
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


def table(inputs):
    for p in inputs:
        r = json.load(open(p))
        print("\n%d x %d, us per call: median (spread) of %d rounds of %d calls\n" % (r["rows"], r["dim"], r["reps"], r["calls_per_rep"]))
        print("| nq | k | never | bfloat16 first | 8-bit first | bfloat16 beats never | 8-bit beats bfloat16 | 8-bit beats never | survivors bf16 / 8-bit |")
        print("|---|---|---|---|---|---|---|---|---|")
        for c in r["cells"]:
            print("| %d | %d | %.0f (%.0f) | %.0f (%.0f) | %.0f (%.0f) | %s | %s | %s | %d / %d |" % (
                c["nq"], c["k"], c["never"]["us"], c["never"]["spread_us"], c["bf16"]["us"], c["bf16"]["spread_us"], c["8bit"]["us"], c["8bit"]["spread_us"],
                "yes" if c["bf16_wins"] else "**no**", "yes" if c["8bit_wins"] else "**no**", "yes" if c["8bit_beats_never"] else "**no**",
                c["stats"]["bf16"]["survivors"], c["stats"]["8bit"]["survivors"]))


def main():
    ints = lambda s: [int(x) for x in s.split(",")]                         # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=ints, default=[2, 4, 8])
    ap.add_argument("--k", type=ints, default=[65, 100, 128, 129, 256, 1000])
    ap.add_argument("--reps", type=int, default=5, help="rounds per arm, the arms alternating (three at least)")
    ap.add_argument("--calls", type=int, default=20, help="consecutive calls between the two events of one round")
    ap.add_argument("--out", default="")
    ap.add_argument("--control", choices=("never", "default"), default="", help="time one arm of the first nq and k alone (see above); --out is appended to")
    ap.add_argument("--root", default="", help="the tree whose quiver_amd package and library are loaded (default: this file's)")
    ap.add_argument("--table", action="store_true", help="print the markdown tables of the result files given as positional arguments instead of measuring")
    ap.add_argument("inputs", nargs="*")
    a = ap.parse_args()
    if a.table:
        return table(a.inputs)
    sys.path.insert(0, os.path.abspath(a.root) if a.root else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    assert a.reps >= 3, "three rounds per arm at least"
    control(a) if a.control else measure(a)


if __name__ == "__main__":
    main()
