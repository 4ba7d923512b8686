#!/usr/bin/env python3
"""What share of a graph search's evaluations could be rejected on a bfloat16 image of the rows, and what share on an 8-bit image?  CPU only: the oracle builds an HNSW
graph (MaxLevel 1, M 16 / MaxM0 32, efConstruction 200, cosine), the level-0 walk is restated in Python (tests/_graph_reject.py) and the
bound scan's own interval (qv_scan_bound_interval, compiled for the host) decides; for the 8-bit image, the rows' bytes, scale and residual are
the library's quantiser's (tests/_bound8.py: RowState8, quantize_query), the sum is the exact integer sum and qv_scan_bound_interval8 decides
(tests/_graph_reject8.py).

  python tools/graph_reject_fraction.py [--rows 20000] [--dim 768] [--corpus iid|subspace] [--ef 128] [--queries 32]

Prints: evaluations per query, the share made in hops that start with a full list (A), the share of A the exact distance rejects (R),
the share certified at one margin and at two (of all evaluations and of R), and the share certified on the 8-bit image."""
import argparse, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from tests import _bound as B
from tests import _bound8 as B8
from tests import _graph_reject as GR
from tests import _graph_reject8 as GR8
from tests import _oracle as O

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=20000); ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--corpus", default="iid", choices=["iid", "subspace"]); ap.add_argument("--ef", type=int, default=128)
ap.add_argument("--queries", type=int, default=32); ap.add_argument("--efc", type=int, default=200)
a = ap.parse_args()
N, D = a.rows, a.dim
if a.corpus == "iid":
    rows, qs = O.gen_rows(20260424, 0, N, D), O.gen_rows(20260425, 0, a.queries, D)
else:
    rng = np.random.default_rng(20260424)
    P = rng.standard_normal((16, D)).astype(np.float32)

    def sub(n):
        x = rng.standard_normal((n, 16)).astype(np.float32) @ P
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    rows, qs = sub(N), sub(a.queries)
t0 = time.perf_counter()
h = O.HNSW(0, D, M=16, maxM0=32, efConstruction=a.efc, efSearch=a.ef, maxLevel=1, seed=7)
for r in rows:                                                              # Insert, one by one: the reference's graph
    h.insert(r)
levels, l0_deg, l0_links, up_off, up_links = h.export_flat(32, 16)
entry = h.entry_point()[0]                                                  # (the level-0 walk starts here: the greedy descent of the one upper level is left out)
build_s = time.perf_counter() - t0
state = B.RowState(rows)
state8 = B8.RowState8(rows)
ev = A = R = C1 = C2 = C8 = 0
for q in qs:
    w = GR.walk(0, rows, state, l0_deg, np.asarray(l0_links).reshape(N, 32), int(entry), q, a.ef, margins=2)
    w8 = GR8.walk8(0, rows, state8, l0_deg, np.asarray(l0_links).reshape(N, 32), int(entry), q, a.ef)
    assert (w8["evals"], w8["A"], w8["R"]) == (w["evals"], w["A"], w["R"])   # the same walk
    ev += w["evals"]; A += w["A"]; R += w["R"]; C1 += w["C1"]; C2 += w["C"]; C8 += w8["C8"]
print("%s %d x %d, efSearch %d, %d queries (graph built in %.0f s): %.0f evaluations per query, %.1f %% at a full list, %.1f %% rejected by the exact "
      "distance, certified by the bfloat16 bound %.1f %% of all (%.1f %% of the rejected); at two margins %.1f %% (%.1f %%); certified on the 8-bit image "
      "%.1f %% of all (%.1f %% of the rejected); mean rres16 %.2e, mean rres8 %.2e (of the row's norm)" % (
          a.corpus, N, D, a.ef, len(qs), build_s, ev / len(qs), 100.0 * A / ev, 100.0 * R / ev, 100.0 * C1 / ev, 100.0 * C1 / max(R, 1),
          100.0 * C2 / ev, 100.0 * C2 / max(R, 1), 100.0 * C8 / ev, 100.0 * C8 / max(R, 1),
          float(np.mean(state.rres / state.rn)), float(np.nanmean(state8.res / state8.rn))))
