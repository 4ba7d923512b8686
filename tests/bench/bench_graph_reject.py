"""Does rejecting neighbours on the row-order bfloat16 copy (QV_FLAG_GRAPH_PLANE, qv_graph_set_reject_plane) make a graph search faster?
"never" against "always" on ONE graph in ONE process, alternating, because a process keeps its fast or slow state for its whole life
(DESIGN.md 4.2): only a same-process comparison means anything.

  python tests/bench/bench_graph_reject.py [--rows 1000000] [--dim 768] [--corpus iid|subspace] [--rounds 3] [--out FILE]

The graph: device-built, MaxLevel 1, M 16 / MaxM0 32, efConstruction 200, cosine.  Per cell (efSearch 64 / 128 / 256 x 8192 / 32768 queries
per call): QPS of both arms (median, min, max over the rounds), rejected / evaluations made in rejecting hops, the implied bytes read per
evaluation, recall@10 against the flat scan (unchanged by construction: the arms' rows are compared), and whether "always" beat "never" by
more than both arms' spread.  One JSON line per cell on stdout (and appended to --out).

--plain [--lib-dir DIR] [--label NAME]: the control.  An index WITHOUT the flag (every call launches the unchanged kernels), one arm, the same
cells; DIR holds another build of libqv.so (the commit before this feature: it lacks the new symbols, which this mode does not call), so that the
same script times both libraries, a process each, alternating."""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1000000); ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--corpus", default="iid", choices=["iid", "subspace"]); ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--m", type=int, default=16); ap.add_argument("--efc", type=int, default=200); ap.add_argument("--max-level", type=int, default=1)
ap.add_argument("--plain", action="store_true"); ap.add_argument("--lib-dir", default=""); ap.add_argument("--label", default="")
ap.add_argument("--efs", default="64,128,256"); ap.add_argument("--nqs", default="8192,32768"); ap.add_argument("--out", default="")
a = ap.parse_args()
sys.path.insert(0, ROOT)
import numpy as np
if a.lib_dir:
    os.environ["QV_LIB_PATH"] = os.path.join(a.lib_dir, "libqv.so")          # quiver_amd._lib reads it at import
if a.plain:                                                                  # an older library lacks the feature's symbols: this mode calls none of them
    import ctypes
    from quiver_amd import _lib
    have = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("qv_graph_set_reject_plane", "qv_graph_reject_stats", "qv_graph_reject_applies"):
        if not hasattr(have, name):
            _lib.PROTOTYPES.pop(name, None)
import quiver_amd
from quiver_amd.device_index import DeviceGraph, random_levels
from tests import _oracle as O

N, D, K = a.rows, a.dim, 10
NQ = max(int(x) for x in a.nqs.split(","))
idx = quiver_amd.DeviceIndex(D, "cosine", rowmajor=True, graph_plane=True) if not a.plain else quiver_amd.DeviceIndex(D, "cosine", rowmajor=True)
if a.corpus == "iid":                                                       # the synthetic corpus of DESIGN.md, generated on the device
    idx.add_synthetic(20260424, 0, N)
    qs = O.gen_rows(20260425, 0, NQ, D)
else:                                                                       # unit rows on a 16-dimensional subspace
    rng = np.random.default_rng(20260424)
    P = rng.standard_normal((16, D)).astype(np.float32)

    def sub(n):
        x = rng.standard_normal((n, 16)).astype(np.float32) @ P
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    for at in range(0, N, 100000):
        idx.add(sub(min(100000, N - at)))
    qs = sub(NQ)
t0 = time.perf_counter()
g = DeviceGraph.build(idx, random_levels(N, a.max_level, 7), m=a.m, max_m0=2 * a.m, ef_construction=a.efc)
build_s = time.perf_counter() - t0
truth, _, _ = idx.search(qs[:256], K)
if a.plain:
    for ef in [int(x) for x in a.efs.split(",")]:
        for nq in [int(x) for x in a.nqs.split(",")]:
            q = qs[:nq]
            g.search(q, K, ef)
            t = []
            for _ in range(max(a.rounds, 3)):
                t0 = time.perf_counter(); g.search(q, K, ef); t.append(nq / (time.perf_counter() - t0))
            line = json.dumps({"control": "no flag", "label": a.label or (a.lib_dir or "this tree"), "corpus": a.corpus, "rows": N, "dim": D, "ef_search": ef, "nq": nq,
                               "qps": [round(float(np.median(t))), round(min(t)), round(max(t))]})
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
    sys.exit(0)
assert g.reject_stats()["plane"], "the index keeps no row-order bfloat16 copy"


def run(mode, q, ef):
    g.set_reject_plane(mode)
    s0 = g.reject_stats()
    t = time.perf_counter()
    r, d, c, ev = g.search(q, K, ef, with_evals=True)
    dt = time.perf_counter() - t
    s1 = g.reject_stats()
    return dt, r, ev, {k: s1[k] - s0[k] for k in ("evals", "rejected", "queries")}


for ef in [int(x) for x in a.efs.split(",")]:
    for nq in [int(x) for x in a.nqs.split(",")]:
        q = qs[:nq]
        run("never", q, ef); run("always", q, ef)                           # warm both arms
        t = {"never": [], "always": []}
        same = True
        for _ in range(max(a.rounds, 3)):
            dn, rn, evn, _ = run("never", q, ef)
            da, ra, eva, st = run("always", q, ef)
            t["never"].append(nq / dn); t["always"].append(nq / da)
            same = same and np.array_equal(rn, ra) and np.array_equal(evn, eva)
        evals = int(eva.sum())
        bytes_never = 4.0 * D
        bytes_always = ((evals - st["evals"]) * 4.0 * D + st["evals"] * 2.0 * D + (st["evals"] - st["rejected"]) * 4.0 * D) / max(evals, 1)
        recall = float(np.mean([len(set(ra[i].tolist()) & set(truth[i].tolist())) / K for i in range(min(256, nq))]))
        med = {k: float(np.median(v)) for k, v in t.items()}
        wins = min(t["always"]) > max(t["never"])                           # beyond both arms' spread across the rounds
        cell = {"corpus": a.corpus, "rows": N, "dim": D, "max_level": a.max_level, "build_s": round(build_s, 2), "ef_search": ef, "nq": nq, "rounds": len(t["never"]),
                "qps_never": [round(med["never"]), round(min(t["never"])), round(max(t["never"]))],
                "qps_always": [round(med["always"]), round(min(t["always"])), round(max(t["always"]))],
                "always_over_never": round(med["always"] / med["never"], 4), "always_beyond_spread": bool(wins),
                "evals_per_query": round(evals / nq, 1), "in_rejecting_hops": round(st["evals"] / max(evals, 1), 4),
                "rejected_of_those": round(st["rejected"] / max(st["evals"], 1), 4), "queries_in_form": st["queries"],
                "bytes_per_eval_never": bytes_never, "bytes_per_eval_always": round(bytes_always, 1), "recall_at_10": round(recall, 4), "arms_identical": bool(same)}
        line = json.dumps(cell)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
