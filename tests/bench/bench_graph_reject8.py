"""Does rejecting neighbours on the row-order bfloat16 copy (QV_FLAG_GRAPH_PLANE, qv_graph_set_reject_plane) make a graph search faster, and does
starting on the row-order 8-bit image (QV_FLAG_GRAPH_PLANE8, qv_graph_set_reject_image) beat starting on that copy?
Three arms — "never", bfloat16-first, 8-bit-first — on ONE graph in ONE process, alternating, because a process keeps its fast or slow state for
its whole life: only a same-process comparison means anything.  (tests/bench/bench_graph_reject.py, the two-arm measurement of
profiles/LAB_r17_graph_reject.md, stays as it was; this is its three-arm successor.)

  python tests/bench/bench_graph_reject8.py [--rows 1000000] [--dim 768] [--corpus iid|subspace] [--rounds 3] [--out FILE]

The graph: device-built, MaxLevel 1, M 16 / MaxM0 32, efConstruction 200, cosine.  Per cell (efSearch 64 / 128 / 256 x 8192 / 32768 queries
per call): QPS of both arms (median, min, max over the rounds), rejected / evaluations made in rejecting hops, the implied bytes read per
evaluation, recall@10 against the flat scan (unchanged by construction: the arms' rows are compared), and whether "always" beat "never" by
more than both arms' spread; the same for the 8-bit arm, and whether its slowest round beat bfloat16-first's fastest (the test AUTO's rule applies).
One JSON line per cell on stdout (and appended to --out).

--plain [--plane16] [--lib-dir DIR] [--label NAME]: the control.  An index WITHOUT the flags (every call launches the unchanged kernels) or, with
--plane16, with QV_FLAG_GRAPH_PLANE alone (the graph's default modes), one arm, the same cells; DIR holds another build of libqv.so (the commit before this feature: it lacks the new symbols, which this mode does not call), so that the
same script times both libraries, a process each, alternating."""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1000000); ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--corpus", default="iid", choices=["iid", "subspace"]); ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--m", type=int, default=16); ap.add_argument("--efc", type=int, default=200); ap.add_argument("--max-level", type=int, default=1)
ap.add_argument("--plain", action="store_true"); ap.add_argument("--plane16", action="store_true"); ap.add_argument("--lib-dir", default=""); ap.add_argument("--label", default="")
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
    for name in ("qv_graph_set_reject_plane", "qv_graph_reject_stats", "qv_graph_reject_applies", "qv_graph_set_reject_image", "qv_graph_reject8_stats",
                 "qv_graph_reject_image_applies"):
        if not hasattr(have, name):
            _lib.PROTOTYPES.pop(name, None)
import quiver_amd
from quiver_amd.device_index import DeviceGraph, random_levels
from tests import _oracle as O

N, D, K = a.rows, a.dim, 10
NQ = max(int(x) for x in a.nqs.split(","))
idx = quiver_amd.DeviceIndex(D, "cosine", rowmajor=True, graph_plane=True, graph_plane8=True) if not a.plain else quiver_amd.DeviceIndex(D, "cosine", rowmajor=True, graph_plane=a.plane16)
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
            line = json.dumps({"control": "QV_FLAG_GRAPH_PLANE only" if a.plane16 else "no flag", "label": a.label or (a.lib_dir or "this tree"), "corpus": a.corpus, "rows": N, "dim": D, "ef_search": ef, "nq": nq,
                               "qps": [round(float(np.median(t))), round(min(t)), round(max(t))]})
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
    sys.exit(0)
assert g.reject_stats()["plane"], "the index keeps no row-order bfloat16 copy"
assert g.reject8_stats()["plane"], "the index keeps no row-order 8-bit image"
ARMS = {"never": ("never", "bf16"), "bf16": ("always", "bf16"), "8bit": ("always", "8bit")}


def run(arm, q, ef):
    g.set_reject_plane(ARMS[arm][0]); g.set_reject_image(ARMS[arm][1])
    s0, e0 = g.reject_stats(), g.reject8_stats()
    t = time.perf_counter()
    r, d, c, ev = g.search(q, K, ef, with_evals=True)
    dt = time.perf_counter() - t
    s1, e1 = g.reject_stats(), g.reject8_stats()
    return dt, (r, d, c, ev), {k: s1[k] - s0[k] for k in ("evals", "rejected", "queries")}, {k: e1[k] - e0[k] for k in ("evals", "rejected", "queries")}


def same_bits(x, y):
    return all(np.array_equal(np.ascontiguousarray(u).view(np.uint32), np.ascontiguousarray(v).view(np.uint32)) for u, v in zip(x, y))


for ef in [int(x) for x in a.efs.split(",")]:
    for nq in [int(x) for x in a.nqs.split(",")]:
        q = qs[:nq]
        for arm in ARMS:                                                    # warm every arm
            run(arm, q, ef)
        t = {arm: [] for arm in ARMS}
        same = True
        for _ in range(max(a.rounds, 3)):
            dn, resn, _, _ = run("never", q, ef)
            db, resb, st16, x8 = run("bf16", q, ef)
            d8, res8, x16, st8 = run("8bit", q, ef)
            t["never"].append(nq / dn); t["bf16"].append(nq / db); t["8bit"].append(nq / d8)
            same = same and same_bits(resn, resb) and same_bits(resn, res8) and x8["evals"] == 0 and x16["evals"] == 0   # rows, float32 bits, counts, evals_out
        ra = res8[0]
        evals = int(res8[3].sum())
        bytes_never = 4.0 * D
        bytes_bf16 = ((evals - st16["evals"]) * 4.0 * D + st16["evals"] * 2.0 * D + (st16["evals"] - st16["rejected"]) * 4.0 * D) / max(evals, 1)
        bytes_8bit = ((evals - st8["evals"]) * 4.0 * D + st8["evals"] * (1.0 * D + 16.0) + (st8["evals"] - st8["rejected"]) * 4.0 * D) / max(evals, 1)
        recall = float(np.mean([len(set(ra[i].tolist()) & set(truth[i].tolist())) / K for i in range(min(256, nq))]))
        med = {k: float(np.median(v)) for k, v in t.items()}
        tri = lambda k: [round(med[k]), round(min(t[k])), round(max(t[k]))]
        cell = {"corpus": a.corpus, "rows": N, "dim": D, "max_level": a.max_level, "build_s": round(build_s, 2), "ef_search": ef, "nq": nq, "rounds": len(t["never"]),
                "qps_never": tri("never"), "qps_always": tri("bf16"), "qps_8bit": tri("8bit"),
                "always_over_never": round(med["bf16"] / med["never"], 4), "always_beyond_spread": bool(min(t["bf16"]) > max(t["never"])),
                "bit8_over_never": round(med["8bit"] / med["never"], 4), "bit8_beyond_never": bool(min(t["8bit"]) > max(t["never"])),
                "bit8_over_bf16": round(med["8bit"] / med["bf16"], 4), "bit8_beyond_bf16": bool(min(t["8bit"]) > max(t["bf16"])),
                "bf16_beyond_bit8": bool(min(t["bf16"]) > max(t["8bit"])),
                "evals_per_query": round(evals / nq, 1), "in_rejecting_hops": round(st16["evals"] / max(evals, 1), 4),
                "rejected_of_those": round(st16["rejected"] / max(st16["evals"], 1), 4), "queries_in_form": st16["queries"],
                "in_rejecting_hops_8bit": round(st8["evals"] / max(evals, 1), 4), "rejected_of_those_8bit": round(st8["rejected"] / max(st8["evals"], 1), 4),
                "queries_in_form_8bit": st8["queries"],
                "bytes_per_eval_never": bytes_never, "bytes_per_eval_always": round(bytes_bf16, 1), "bytes_per_eval_8bit": round(bytes_8bit, 1),
                "recall_at_10": round(recall, 4), "arms_identical": bool(same)}
        line = json.dumps(cell)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
