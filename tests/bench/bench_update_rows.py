"""What overwriting many rows costs: one qv_index_update_rows call against the loop of qv_index_update it replaces, against qv_index_add of as
many rows (the ceiling: the same bytes moved, the same planes derived), and through the host mirror's slot reuse (HybridIndex: DeleteBatch
then InsertBatch).  1M x 768 cosine, default planes, synthetic rows.

  python tests/bench/bench_update_rows.py [--root DIR] [--rows 1000000] [--dim 768] [--arms 1,2,3,4] [--hybrid-rows 131072] [--hybrid-n 65536] [--out FILE]

--root DIR   import quiver_amd (and load quiver_amd/lib/*.so) from DIR instead of this tree: the way to run the SAME script against another
             build (the commit before a change) in the same visit to a box.  A build without update_rows runs the loops and the controls only.
Arms: 1 = update_rows vs the loop, n = 1 / 64 / 4096 / 65536 distinct random rows; 2 = a contiguous run of 65536 rows vs qv_index_add of 65536;
3 = HybridIndex DeleteBatch + InsertBatch of --hybrid-n ids on a collection of --hybrid-rows (the HNSW side of both calls is timed with them:
it is the same code in both builds); 4 = controls: add_device of the whole corpus, a single qv_index_update.
Three runs per figure, alternating between the arms of a comparison; medians with min and max.  One JSON line on stdout (and appended to --out)."""
import argparse, ctypes as C, json, os, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE)
ap.add_argument("--rows", type=int, default=1000000); ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--arms", default="1,2,3,4"); ap.add_argument("--hybrid-rows", type=int, default=131072); ap.add_argument("--hybrid-n", type=int, default=65536)
ap.add_argument("--out", default=""); ap.add_argument("--label", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import numpy as np
import quiver_amd

N, D = a.rows, a.dim
arms = {int(x) for x in a.arms.split(",") if x}
has_bulk = hasattr(quiver_amd.DeviceIndex, "update_rows")
out = {"label": a.label or os.path.basename(os.path.abspath(a.root)), "rows": N, "dim": D, "has_update_rows": has_bulk}


def ms(f):
    t0 = time.perf_counter(); f(); return (time.perf_counter() - t0) * 1e3


def summary(t):
    t = sorted(t)
    return {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4), "runs": len(t)}


rng = np.random.default_rng(20260501)
if arms & {1, 2, 4}:
    import torch
    idx = quiver_amd.DeviceIndex(D, "cosine")
    idx.reserve(N + 4 * 65536)
    if 4 in arms:                                                # the whole corpus from device memory, three times over (a fresh index each)
        d_rows = torch.randn((N, D), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        t = []
        for rep in range(3):
            j = quiver_amd.DeviceIndex(D, "cosine"); j.reserve(N)
            t.append(ms(lambda: j.add_device(d_rows.data_ptr(), N)))
            j.close()
        out["add_device_all"] = summary(t)
        del d_rows
    idx.add_synthetic(20260502, 0, N)
    vec = rng.standard_normal(D).astype(np.float32)
    idx.update(7, vec)                                           # (warm: the staging buffer, the kernels)
    if 4 in arms:
        out["update_one"] = summary([ms(lambda: idx.update(int(r), vec)) for r in rng.integers(0, N, 200)])
    if 1 in arms:
        res = {}
        for n in (1, 64, 4096, 65536):
            rows = rng.choice(N, n, replace=False).astype(np.uint32)
            vecs = rng.standard_normal((n, D)).astype(np.float32)
            if has_bulk:
                idx.update_rows(rows[:1], vecs[:1])
            loop, bulk = [], []
            for rep in range(3):                                 # alternating
                if has_bulk:
                    bulk.append(ms(lambda: idx.update_rows(rows, vecs)))
                loop.append(ms(lambda: [idx.update(int(r), v) for r, v in zip(rows, vecs)]))
            res[str(n)] = {"loop_of_update": summary(loop)}
            if has_bulk:
                res[str(n)]["update_rows"] = summary(bulk)
                res[str(n)]["loop_over_call"] = round(res[str(n)]["loop_of_update"]["median_ms"] / res[str(n)]["update_rows"]["median_ms"], 2)
        out["scattered"] = res
    if 2 in arms:
        n = 65536
        vecs = rng.standard_normal((n, D)).astype(np.float32)
        rows = np.arange(300032, 300032 + n, dtype=np.uint32)
        upd, add = [], []
        for rep in range(3):
            if has_bulk:
                upd.append(ms(lambda: idx.update_rows(rows, vecs)))
            add.append(ms(lambda: idx.add(vecs)))
        out["contiguous_65536"] = {"add": summary(add)}
        if has_bulk:
            out["contiguous_65536"]["update_rows"] = summary(upd)
            out["contiguous_65536"]["update_rows_over_add"] = round(summary(upd)["median_ms"] / summary(add)["median_ms"], 3)
            # where the difference goes: the host's part of the call (duplicates, sort, tile offsets) on its own
            from quiver_amd._lib import lib
            ro, so, tf, to = (np.empty(n + 1, np.uint32) for _ in range(4)); m, t = C.c_uint32(0), C.c_uint32(0)
            out["contiguous_65536"]["host_plan"] = summary([ms(lambda: lib().qv_update_rows_plan(rows.ctypes.data, n, ro.ctypes.data, so.ctypes.data, tf.ctypes.data,
                                                                                                 to.ctypes.data, C.byref(m), C.byref(t))) for _ in range(3)])
    idx.close()

if 3 in arms:
    L = C.CDLL(os.path.join(os.path.abspath(a.root), "quiver_amd", "lib", "libqvhost.so"))
    vp, u32, ci = C.c_void_p, C.c_uint32, C.c_int
    L.qvh_last_error.restype = C.c_char_p
    L.qvh_hybrid_new.restype = vp; L.qvh_hybrid_new.argtypes = [ci, ci, ci, ci, ci, ci, ci, C.c_double, C.c_uint64]
    L.qvh_hybrid_free.argtypes = [vp]
    L.qvh_hybrid_insert_batch.argtypes = [vp, C.POINTER(C.c_char_p), vp, vp, u32]
    L.qvh_hybrid_delete_batch.argtypes = [vp, C.POINTER(C.c_char_p), u32]
    L.qvh_hybrid_exact_device_rows.restype = u32; L.qvh_hybrid_exact_device_rows.argtypes = [vp]

    def ok(rc):
        if rc != 0:
            raise RuntimeError(L.qvh_last_error().decode())

    def cids(names):
        return (C.c_char_p * len(names))(*[s.encode() for s in names])
    HN, n = a.hybrid_rows, a.hybrid_n
    h = L.qvh_hybrid_new(0, 0, 16, 32, 100, 64, 1000, 0.0, 3)
    base = rng.standard_normal((HN, D)).astype(np.float32)
    lens = np.full(max(HN, n), D, np.uint32)
    ok(L.qvh_hybrid_insert_batch(h, cids(["a%d" % i for i in range(HN)]), base.ctypes.data, lens.ctypes.data, HN))
    dele, ins = [], []
    live = ["a%d" % i for i in range(HN)]
    for rep in range(3):
        pick = rng.permutation(HN)[:n]
        gone = cids([live[i] for i in pick])
        new = ["r%d_%d" % (rep, i) for i in range(n)]
        vecs = rng.standard_normal((n, D)).astype(np.float32)
        cn = cids(new)
        dele.append(ms(lambda: ok(L.qvh_hybrid_delete_batch(h, gone, n))))
        ins.append(ms(lambda: ok(L.qvh_hybrid_insert_batch(h, cn, vecs.ctypes.data, lens.ctypes.data, n))))
        for j, i in enumerate(pick):
            live[i] = new[j]
    out["hybrid"] = {"collection": HN, "ids": n, "delete_batch": summary(dele), "insert_batch": summary(ins),
                     "device_rows_after": int(L.qvh_hybrid_exact_device_rows(h))}
    L.qvh_hybrid_free(h)

line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "a") as f:
        f.write(line + "\n")
