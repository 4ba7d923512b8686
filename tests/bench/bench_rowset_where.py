"""Row sets from predicates on the device against the path the library offered before: the same predicate in numpy on the host,
np.packbits, and qv_rowset_create from the words.  Not collected by pytest, not part of bench.py.

    python tests/bench/bench_rowset_where.py --rows 1000000 --out profiles/rowset_where_1M.json

Per case: the whole rowset_where call (host clock; the call synchronises), its kernel alone (HIP events: qv_index_profile), the
host path in the same process, and — once per size — qv_rowset_combine against two host bitmaps ANDed and uploaded again.
Warm-up runs first, then `--repeat` timed runs of each, interleaved; medians with the 10th / 90th percentiles.  Algorithmic bytes of
the kernel: 8 (F64) or 4 (U32) bytes per row of every tile a predicate actually reads (a tile whose word is already zero reads
nothing), plus 8 bytes of presence per such tile and predicate, plus the 8-byte output word per tile; over the kernel time that is
the rate held against the 8 TB/s HBM peak of an MI355X."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import quiver_amd  # noqa: E402

HBM_PEAK = 8.0e12


def pct(xs):
    a = np.asarray(xs, dtype=np.float64)
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90))}


def pack(mask):
    pad = np.zeros((mask.size + 63) // 64 * 64, dtype=np.uint8)
    pad[:mask.size] = mask
    return np.packbits(pad, bitorder="little").view(np.uint64)


def kernel_bytes(n, stages):
    """stages: (bytes per value, bool mask of the predicate) in order; every column fully present"""
    tiles = (n + 63) // 64
    pad = tiles * 64
    alive = np.ones(tiles, dtype=bool)
    total = tiles * 8
    read = []
    for width, m in stages:
        t = int(alive.sum())
        total += t * (64 * width + 8)
        read.append(t)
        mm = np.zeros(pad, dtype=bool); mm[:n] = m
        alive &= mm.reshape(tiles, 64).any(axis=1)
    return total, read


def sweep(a, idx, rng, n, cases, c_price):
    """the kernel alone (HIP events) in every shape the measurement build holds, the shapes alternating inside each repeat"""
    assert "libqv_dev" in os.environ.get("QV_LIB_PATH", ""), "the product library has one shape: build with make VARIANTS=1 and set QV_LIB_PATH"
    code = rng.integers(0, 512, n).astype(np.uint32)
    c_code = idx.column("u32")
    c_code.set(0, code)
    todo = {k: cases[k][0] for k in ("f64_range_50pct", "conj3_50pct", "conj3_1pct", "conj3_1pct_sorted_first_column")}
    todo["u32_in_256_literals"] = [(c_code, "in", list(range(0, 512, 2)))]
    todo["f64_in_256_literals"] = [(c_price, "in", [i / 256.0 for i in range(256)])]
    shapes = [(t, l) for t in (1, 2, 4, 8) for l in (0, 1)]
    times = {k: {s: [] for s in shapes} for k in todo}
    words = {}
    idx.profile(True)
    for it in range(a.warmup + a.repeat):
        for t, l in shapes:
            os.environ["QV_WHERE_TILES"], os.environ["QV_WHERE_LDS"] = str(t), str(l)
            for k, preds in todo.items():
                idx.profile_read()
                rs = idx.rowset_where(preds)
                k_ms, launches = idx.profile_read()
                assert launches == 1
                if it == 0:                                             # every shape computes the same set
                    w = rs.words()
                    assert np.array_equal(words.setdefault(k, w), w), (k, t, l)
                rs.close()
                if it >= a.warmup:
                    times[k][(t, l)].append(k_ms)
    result = {"rows": n, "repeat": a.repeat, "warmup": a.warmup, "device": quiver_amd.device_index.device_info(0), "kernel_ms": {}}
    for k in todo:
        result["kernel_ms"][k] = {"tiles%d_%s" % (t, "lds" if l else "uniform"): pct(times[k][(t, l)]) for t, l in shapes}
        print(k, {name: round(v["median_ms"], 4) for name, v in result["kernel_ms"][k].items()}, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--sweep", action="store_true",
                    help="kernel time of the other kernel shapes (tiles per wave x literal source): needs the measurement build, QV_LIB_PATH=.../libqv_dev.so")
    a = ap.parse_args()
    n = a.rows
    rng = np.random.default_rng(20260601)
    idx = quiver_amd.DeviceIndex(4, "l2sq")
    idx.add_synthetic(1, 0, n)
    price = rng.random(n)
    cat = (rng.random(n) >= 0.9).astype(np.uint32) * rng.integers(1, 50, n).astype(np.uint32)      # 0 for about 90 % of the rows
    tag = rng.integers(0, 20, n).astype(np.uint32)                                                  # IN of 16 of 20: about 80 %
    tags = list(range(16))
    c_price, c_sorted, c_cat, c_tag = idx.column("f64"), idx.column("f64"), idx.column("u32"), idx.column("u32")
    price_sorted = np.sort(price)
    c_price.set(0, price); c_sorted.set(0, price_sorted); c_cat.set(0, cat); c_tag.set(0, tag)

    def conj(col, vals, cut):
        return ([(col, "lt", cut), (c_cat, "eq", 0), (c_tag, "in", tags)],
                lambda: (vals < cut) & (cat == 0) & np.isin(tag, tags),
                lambda: [(8, vals < cut), (4, cat == 0), (4, np.isin(tag, tags))])

    cases = {"f64_range_50pct": ([(c_price, "lt", 0.5)], lambda: price < 0.5, lambda: [(8, price < 0.5)])}
    for name, want in (("50pct", 0.5), ("10pct", 0.1), ("1pct", 0.01)):
        cases["conj3_" + name] = conj(c_price, price, want / 0.72)
    cases["conj3_1pct_sorted_first_column"] = conj(c_sorted, price_sorted, 0.01 / 0.72)

    if a.sweep:
        return sweep(a, idx, rng, n, cases, c_price)
    result = {"rows": n, "repeat": a.repeat, "warmup": a.warmup, "device": quiver_amd.device_index.device_info(0), "cases": {}}
    idx.profile(True)
    for name, (preds, host_mask, stages) in cases.items():
        want = host_mask()
        t_new, t_kernel, t_host = [], [], []
        for it in range(a.warmup + a.repeat):
            idx.profile_read()
            t0 = time.perf_counter()
            rs = idx.rowset_where(preds)
            t1 = time.perf_counter()
            k_ms, launches = idx.profile_read()
            assert launches == 1
            t2 = time.perf_counter()
            hs = idx.rowset(pack(host_mask()))
            t3 = time.perf_counter()
            if it == 0:
                assert np.array_equal(rs.words(), hs.words()) and rs.count() == hs.count() == int(want.sum())
            rs.close(); hs.close()
            if it >= a.warmup:
                t_new.append((t1 - t0) * 1e3); t_kernel.append(k_ms); t_host.append((t3 - t2) * 1e3)
        nbytes, tiles_read = kernel_bytes(n, stages())
        k_med = float(np.median(t_kernel))
        result["cases"][name] = {
            "selected_fraction": float(want.mean()), "tiles": (n + 63) // 64, "tiles_read_per_predicate": tiles_read,
            "kernel_algorithmic_bytes": nbytes, "kernel_bytes_per_s": nbytes / (k_med * 1e-3), "kernel_fraction_of_hbm_peak": nbytes / (k_med * 1e-3) / HBM_PEAK,
            "rowset_where_call": pct(t_new), "kernel": pct(t_kernel), "host_numpy_packbits_rowset_create": pct(t_host),
            "host_over_new": float(np.median(t_host) / np.median(t_new)),
        }
        print(name, json.dumps(result["cases"][name]), flush=True)

    # combine: two resident sets ANDed on the device, against two host bitmaps ANDed and uploaded again
    wa, wb = pack(price < 0.5), pack(tag < 10)
    sa, sb, dst = idx.rowset(wa), idx.rowset(wb), idx.rowset(None)
    t_dev, t_kernel, t_host = [], [], []
    for it in range(a.warmup + a.repeat):
        idx.profile_read()
        t0 = time.perf_counter()
        dst.combine(sa, sb, "and")
        t1 = time.perf_counter()
        k_ms, _ = idx.profile_read()
        t2 = time.perf_counter()
        hs = idx.rowset(wa & wb)
        t3 = time.perf_counter()
        if it == 0:
            assert np.array_equal(dst.words(), hs.words())
        hs.close()
        if it >= a.warmup:
            t_dev.append((t1 - t0) * 1e3); t_kernel.append(k_ms); t_host.append((t3 - t2) * 1e3)
    result["combine_and"] = {"rowset_combine_call": pct(t_dev), "kernel": pct(t_kernel), "host_and_rowset_create": pct(t_host),
                             "host_over_new": float(np.median(t_host) / np.median(t_dev))}
    print("combine_and", json.dumps(result["combine_and"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
