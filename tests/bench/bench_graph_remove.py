"""What a mutation of an HNSW graph costs: Delete / a lone Insert through the host face (quiver::HNSW in libqvhost.so), and
qv_graph_remove itself.  1M x 768, cosine, M = 16 / MaxM0 = 32, MaxLevel = 1 unless told otherwise.

  python tests/bench/bench_graph_remove.py [--lib-dir DIR] [--rows 1000000] [--dim 768] [--abi] [--out FILE]

--lib-dir DIR   load libqvhost.so (and, through its $ORIGIN rpath, libqv.so) from DIR instead of quiver_amd/lib: the way to run
                the SAME script against another build of the library (the commit before a change) in the same visit to a box
--abi           (a) only: qv_graph_remove of 1 / 64 / 4096 nodes on a DeviceGraph (needs a library that has it)
Without --abi, through the host face:
  (b) one Delete, the first lone Search after it, and the p50 of the 100 lone searches after that (and of 100 before)
  (c) a single Insert (5 of them, each timed)
  (d) QPS at efSearch 128 with 8192 queries per call before any mutation and after one removal
One JSON line on stdout (and appended to --out)."""
import argparse, ctypes as C, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--lib-dir", default=os.path.join(ROOT, "quiver_amd", "lib"))
ap.add_argument("--rows", type=int, default=1000000); ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--m", type=int, default=16); ap.add_argument("--efc", type=int, default=200); ap.add_argument("--efs", type=int, default=128)
ap.add_argument("--max-level", type=int, default=1); ap.add_argument("--nq", type=int, default=8192)
ap.add_argument("--abi", action="store_true"); ap.add_argument("--out", default=""); ap.add_argument("--label", default="")
a = ap.parse_args()
os.environ["QV_LIB_PATH"] = os.path.join(a.lib_dir, "libqv.so")        # quiver_amd._lib reads it at import
sys.path.insert(0, ROOT)
import numpy as np
from tests import _oracle as O

N, D, K = a.rows, a.dim, 10
rows = O.gen_rows(20260424, 0, N + 8, D)
qs = O.gen_rows(20260425, 0, a.nq, D)
out = {"label": a.label or os.path.basename(os.path.normpath(a.lib_dir)), "rows": N, "dim": D, "M": a.m, "efC": a.efc, "efS": a.efs, "max_level": a.max_level}


def ms(f):
    t0 = time.perf_counter(); f(); return (time.perf_counter() - t0) * 1e3


if a.abi:
    import quiver_amd
    from quiver_amd.device_index import DeviceGraph, random_levels
    idx = quiver_amd.DeviceIndex(D, "cosine", rowmajor=True); idx.add(rows[:N])
    g = DeviceGraph.build(idx, random_levels(N, a.max_level, 7), m=a.m, max_m0=2 * a.m, ef_construction=a.efc)
    g.search(qs[:64], K, a.efs)
    perm = np.random.default_rng(1).permutation(N).astype(np.uint32)
    at, res = 0, {}
    for cnt in (1, 64, 4096):
        t = []
        for rep in range(3):
            nodes = perm[at:at + cnt]; at += cnt
            t.append(ms(lambda: g.remove(nodes)))
        res[str(cnt)] = t
    out["qv_graph_remove_ms"] = res
    r, d, c = g.search(qs[:256], K, a.efs)
    out["filled_after"] = int((c == K).sum())
else:
    L = C.CDLL(os.path.join(a.lib_dir, "libqvhost.so"))
    vp, u32, ci = C.c_void_p, C.c_uint32, C.c_int
    L.qvh_last_error.restype = C.c_char_p
    L.qvh_hnsw_new.restype = vp; L.qvh_hnsw_new.argtypes = [ci, ci, ci, ci, ci, ci, ci, C.c_uint64]
    L.qvh_hnsw_free.argtypes = [vp]
    L.qvh_hnsw_insert.argtypes = [vp, C.c_char_p, vp, u32]
    L.qvh_hnsw_insert_batch.argtypes = [vp, C.POINTER(C.c_char_p), vp, u32, u32, u32, u32]
    L.qvh_hnsw_delete.argtypes = [vp, C.c_char_p]
    L.qvh_results_new.restype = vp; L.qvh_results_free.argtypes = [vp]; L.qvh_results_count.argtypes = [vp]
    L.qvh_hnsw_search.argtypes = [vp, vp, u32, ci, vp, vp]
    L.qvh_hnsw_search_batch_raw.argtypes = [vp, vp, u32, u32, ci, vp, vp, vp, vp, C.POINTER(C.c_double)]
    L.qvh_hnsw_distance_calls.restype = C.c_uint64; L.qvh_hnsw_distance_calls.argtypes = [vp]

    def ok(rc):
        if rc != 0:
            raise RuntimeError(L.qvh_last_error().decode())

    h = L.qvh_hnsw_new(0, 0,                     # QV_COSINE, device 0
                        a.m, 2 * a.m, a.efc, a.efs, a.max_level, 7)
    ids = [b"%07d" % i for i in range(N + 8)]
    cids = (C.c_char_p * N)(*ids[:N])
    out["build_s"] = ms(lambda: ok(L.qvh_hnsw_insert_batch(h, cids, rows.ctypes.data, D, N, 16384, 16))) / 1e3
    res = L.qvh_results_new(); ridx = np.zeros(K + 8, np.uint32)
    ro = np.empty((a.nq, K), np.uint32); do = np.empty((a.nq, K), np.float32); co = np.empty(a.nq, np.uint32); eo = np.empty(a.nq, np.uint32); sec = C.c_double(0)

    def lone(i):
        q = qs[i % a.nq]
        return ms(lambda: ok(L.qvh_hnsw_search(h, q.ctypes.data, D, K, res, ridx.ctypes.data)))

    def batch_qps():
        t = []
        for rep in range(4):
            t.append(ms(lambda: ok(L.qvh_hnsw_search_batch_raw(h, qs.ctypes.data, D, a.nq, K, ro.ctypes.data, do.ctypes.data, co.ctypes.data, eo.ctypes.data, C.byref(sec)))))
        return [a.nq / (x / 1e3) for x in t[1:]]                       # the first call warms (and, on a stale copy, uploads)

    out["qps_before"] = batch_qps()                                    # (d)
    for i in range(20):
        lone(i)
    out["lone_search_p50_ms_before"] = float(np.median([lone(i) for i in range(100)]))
    calls0 = L.qvh_hnsw_distance_calls(h)
    out["delete_ms"] = ms(lambda: ok(L.qvh_hnsw_delete(h, ids[N // 2])))                      # (b)
    out["first_search_after_delete_ms"] = lone(1000)
    after = [lone(1001 + i) for i in range(100)]
    out["lone_search_p50_ms_after_delete"] = float(np.median(after)); out["lone_search_max_ms_after_delete"] = float(np.max(after))
    out["host_distance_calls_in_those_searches"] = int(L.qvh_hnsw_distance_calls(h) - calls0)
    out["more_delete_ms"] = [ms(lambda: ok(L.qvh_hnsw_delete(h, ids[N // 3 + 17 * i]))) for i in range(5)]
    out["qps_after_one_removal"] = batch_qps()                         # (d): tombstones switch the level-0 fast paths off
    out["insert_ms"] = [ms(lambda: ok(L.qvh_hnsw_insert(h, ids[N + i], rows[N + i].ctypes.data, D))) for i in range(5)]   # (c)
    out["first_search_after_insert_ms"] = lone(2000)
    if hasattr(L, "qvh_hnsw_device_state"):
        st = (C.c_uint64 * 4)(); L.qvh_hnsw_device_state.argtypes = [vp, C.POINTER(C.c_uint64)]; L.qvh_hnsw_device_state(h, st)
        out["device_state"] = {"full_uploads": int(st[0]), "device_removes": int(st[1]), "device_inserts": int(st[2]), "host_searches": int(st[3])}
    L.qvh_results_free(res); L.qvh_hnsw_free(h)

line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "a") as f:
        f.write(line + "\n")
