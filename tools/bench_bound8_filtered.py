"""A single FILTERED query's bound scan: the bfloat16 copy first against the 8-bit plane first, in one process.

    python tools/bench_bound8_filtered.py [--rows 1000000] [--k 1,10,64] [--calls 20] [--warmup 3] [--label tree] [--out FILE.json]

Device-pointer calls on a caller's stream, cosine, 768 dimensions, the benchmark's generator (corpus seed 20260424, query seed 20260425).
The filters: a row set of every row; a row set of one 64-row tile in ten; a row set of a random 1 % of the rows (every tile a candidate,
few rows live) — all three through qv_index_search_rowsets_device —; and a where-filter (one F64 range, about 10 % and 100 % selected)
through qv_index_search_where_device.  Per filter and k the arms are set_bound_scan("always") with set_bound_plane_filtered("bf16") and
with ("8bit"): `calls` calls of each behind HIP events after a warm-up, the whole round twice (a / b); the counters prove which stage
answered and the arms' rows and float32 bits are compared with the exact filtered scan's ("never").  A library without the filtered
setter (the parent commit's, in a checkout of its own) has the one arm "parent": "always", which is the bfloat16 copy there.  `--merge`
puts the records of several runs (parent and tree alternating) into one file."""
import os; os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # the host's setting, before the first HIP call
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quiver_amd                                              # noqa: E402
from tests import _oracle as O                                  # noqa: E402  (query generator only)

DIM = 768


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--k", default="1,10,64")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--out", default="")
    ap.add_argument("--merge", nargs="*", default=None, help="write --out from these record files instead of measuring")
    a = ap.parse_args()
    if a.merge is not None:
        runs = [json.load(open(p)) for p in a.merge]
        with open(a.out, "w") as f:
            json.dump({"runs": runs}, f, indent=1); f.write("\n")
        return
    import torch
    n = a.rows
    st = torch.cuda.Stream()
    idx = quiver_amd.DeviceIndex(DIM, "cosine", filter="off")
    idx.add_synthetic(20260424, 0, n)
    assert idx.bound_scan8_stats()["plane"] and idx.bound_scan_stats()["plane"]
    has_setter = hasattr(idx, "set_bound_plane_filtered")
    arms = (("bf16", "bf16"), ("8bit", "8bit")) if has_setter else (("parent", None),)
    rec = dict(label=a.label, metric="cosine", dim=DIM, rows=n, device=quiver_amd.device_index.device_info(0), calls_per_arm=a.calls, warmup=a.warmup, results=[])
    tile = np.arange(n) // 64
    rng = np.random.default_rng(20260426)
    vals = rng.random(n)
    col = idx.column("f64"); col.set(0, vals)
    sets = {"every_tile": idx.rowset(np.ones(n, bool)), "one_tile_in_ten": idx.rowset(tile % 10 == 0), "random_1pct": idx.rowset(rng.random(n) < 0.01)}
    filters = [(name, "rowsets", rs) for name, rs in sets.items()] + [("where_10pct", "where", [(col, "lt", 0.1)]), ("where_100pct", "where", [(col, "lt", 2.0)])]
    q = torch.from_numpy(O.gen_rows(20260425, 0, 1, DIM)).cuda()
    for name, kind, what in filters:
        for k in [int(x) for x in a.k.split(",")]:
            dr = torch.empty((1, k), dtype=torch.int32, device="cuda"); dd = torch.empty((1, k), dtype=torch.float32, device="cuda")

            def call():
                if kind == "rowsets":
                    idx.search_rowsets_device(q.data_ptr(), 1, k, [what], dr.data_ptr(), dd.data_ptr(), st.cuda_stream)
                else:
                    idx.search_where_device(q.data_ptr(), 1, k, what, dr.data_ptr(), dd.data_ptr(), st.cuda_stream)

            idx.set_bound_scan("never")
            with torch.cuda.stream(st):
                call()
            st.synchronize()
            exact = (dr.cpu().numpy().copy(), dd.cpu().numpy().view(np.uint32).copy())
            r = dict(filter=name, k=k)
            same = True
            for rnd in ("a", "b"):
                for arm, plane in arms:
                    idx.set_bound_scan("always")
                    if plane is not None:
                        idx.set_bound_plane_filtered(plane)
                    s8, s16 = idx.bound_scan8_stats(), idx.bound_scan_stats()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(st):
                        for i in range(a.warmup + a.calls):
                            if i == a.warmup:
                                e0.record(st)
                            call()
                        e1.record(st)
                    st.synchronize()
                    r["%s_ms_%s" % (arm, rnd)] = round(e0.elapsed_time(e1) / a.calls, 4)
                    t8, t16 = idx.bound_scan8_stats(), idx.bound_scan_stats()
                    calls = a.warmup + a.calls
                    assert t16["searches"] - s16["searches"] == calls, (arm, s16, t16)
                    assert t8["searches"] - s8["searches"] == (calls if arm == "8bit" else 0), (arm, s8, t8)
                    if arm == "8bit":
                        r["8bit_survivors"], r["8bit_hand_ons"], r["8bit_reached_exact"] = t8["candidates"], t8["hand_backs"] - s8["hand_backs"], t16["hand_backs"] - s16["hand_backs"]
                    else:
                        r["%s_survivors" % arm], r["%s_hand_backs" % arm] = t16["candidates"], t16["hand_backs"] - s16["hand_backs"]
                    same = same and np.array_equal(dr.cpu().numpy(), exact[0]) and np.array_equal(dd.cpu().numpy().view(np.uint32), exact[1])
            r["same_bits_as_exact"] = bool(same)
            rec["results"].append(r)
            print(json.dumps(dict(r, label=a.label, rows=n)), flush=True)
    idx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
