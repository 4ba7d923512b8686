"""The route of a fused flat search (quiver_amd/csrc/qv_scan.hip: plan_flat) on the device: for the smallest shape of every route, the
route qv_scan_route names is the one that RAN — by the index's bound-scan counters (searches counted, or not) and the QV_TRACE kernel
name on stderr — and its results are the exact scan's (bound scan "never"), bit for bit.

One fresh child process runs every case (the unfiltered trace flag is read once per process); it marks each search on stderr, so a trace
line belongs to the search in front of which its marker stands.  Routes without a trace line of their own (small, split_mq, split,
fused, two_launch) show as "no scan-kernel line and no counter moved"."""
import json
import os
import subprocess
import sys

import pytest

from tests import _route as R

pytestmark = pytest.mark.gpu

CHILD = r'''
import json, sys
import numpy as np
import quiver_amd
from quiver_amd import _lib
from quiver_amd.device_index import device_info
from tests import _route as R

cus = device_info(0)["cus"]
tiles_mq64 = 1                                               # the fewest tiles with 16 per workgroup slot: the matrix-core scan's floor
while tiles_mq64 < 16 * R.scan_grid(tiles_mq64, cus):
    tiles_mq64 += 1
MODE = {"auto": 0, "always": 1, "never": 2}
PLANE = {"auto": 0, "8bit": 1, "bf16": 2}
# name, metric, rows, dim, nq, k, bound mode, plane mode, mask (one tile in so many, 0: none)
CASES = [
    ("bound-1",        "cosine", 600, 16, 1, 10, "always", "auto", 0),
    ("bound_mq-2",     "cosine", 600, 16, 2, 10, "always", "auto", 0),
    ("bound_mq-5",     "cosine", 600, 16, 5, 10, "always", "auto", 0),
    ("bound8-1",       "cosine", 600, 16, 1, 10, "always", "8bit", 0),
    ("bound-masked",   "cosine", 600, 16, 1, 10, "always", "8bit", 10),
    ("never-1",        "cosine", 600, 16, 1, 10, "never", "auto", 0),
    ("never-4",        "cosine", 600, 16, 4, 10, "never", "auto", 0),
    ("never-1-k17",    "cosine", 600, 16, 1, 17, "never", "auto", 0),
    ("never-4-k17",    "cosine", 600, 16, 4, 17, "never", "auto", 0),
    ("ten-rows",       "cosine", 10, 16, 1, 10, "auto", "auto", 0),
    ("wide-1",         "cosine", 2000, 256, 1, 10, "auto", "auto", 0),
    ("wide-4",         "cosine", 2000, 256, 4, 10, "auto", "auto", 0),
    ("wide-4-k17",     "cosine", 2000, 256, 4, 17, "auto", "auto", 0),
    ("mq64-40",        "cosine", tiles_mq64 * 64, 16, 40, 10, "auto", "auto", 0),
    ("l1-1",           "l1", 600, 16, 1, 10, "auto", "auto", 0),
    ("l1-1-k17",       "l1", 600, 16, 1, 17, "auto", "auto", 0),
    ("l1-200-k17",     "l1", 200, 16, 1, 17, "auto", "auto", 0),
]
indexes = {}
out = []
for name, metric, rows, dim, nq, k, mode, plane, mask_every in CASES:
    key = (metric, rows, dim)
    if key not in indexes:
        idx = quiver_amd.DeviceIndex(dim, metric, filter="off")
        idx.add_synthetic(20261017 + rows, 0, rows)
        indexes[key] = idx
    idx = indexes[key]
    q = np.random.default_rng(rows + nq).standard_normal((nq, dim)).astype(np.float32)
    tiles = (rows + 63) // 64
    mask, cand_tiles = None, R.NO_FILTER
    if mask_every:
        mask = np.zeros(rows, bool)
        for t in range(0, tiles, mask_every):
            mask[t * 64:(t + 1) * 64] = True
        cand_tiles = len(range(0, tiles, mask_every))
    search = (lambda: idx.search_masked(q, k, mask)) if mask is not None else (lambda: idx.search(q, k))
    idx.set_bound_scan("never"); idx.set_bound_plane("auto")
    sys.stderr.write("@@ reference %s\n" % name); sys.stderr.flush()
    ref = search()
    idx.set_bound_scan(mode); idx.set_bound_plane(plane)
    s0, e0 = idx.bound_scan_stats(), idx.bound_scan8_stats()
    sys.stderr.write("@@ case %s\n" % name); sys.stderr.flush()
    got = search()
    sys.stderr.write("@@ end\n"); sys.stderr.flush()
    s1, e1 = idx.bound_scan_stats(), idx.bound_scan8_stats()
    route = _lib.lib().qv_scan_route(quiver_amd.metric_id(metric), dim, rows, nq, k, cus, 1, MODE[mode], PLANE[plane], int(s1["plane"]), int(e1["plane"]), cand_tiles)
    out.append({"name": name, "nq": nq, "k": k, "tiles": tiles, "route": route, "searches": s1["searches"] - s0["searches"], "searches8": e1["searches"] - e0["searches"],
                "same": bool(np.array_equal(got[0], ref[0]) and got[1].tobytes() == ref[1].tobytes() and np.array_equal(got[2], ref[2])),
                "full": bool((got[2] == k).all())})
print("@@JSON " + json.dumps(out))
'''


def _trace_lines(stderr):
    """-> {case name: the "qv: scan kernel" lines printed during that case's search}"""
    lines, cur = {}, None
    for line in stderr.splitlines():
        if line.startswith("@@ case "):
            cur = line[len("@@ case "):]
            lines[cur] = []
        elif line.startswith("@@ "):
            cur = None
        elif cur is not None and line.startswith("qv: scan kernel"):
            lines[cur].append(line)
    return lines


def test_every_route_runs_where_the_plan_says_and_answers_as_the_exact_scan():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", CHILD], env=dict(os.environ, QV_TRACE="1"), capture_output=True, text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stderr[-4000:]
    cases = {c["name"]: c for c in json.loads(next(l for l in p.stdout.splitlines() if l.startswith("@@JSON "))[len("@@JSON "):])}
    trace = _trace_lines(p.stderr)
    # the routes these shapes are there for (the plan's own answer is what is checked below; this pins the shapes to their routes)
    want = {"bound-1": R.BOUND, "bound_mq-2": R.BOUND_MQ, "bound_mq-5": R.BOUND_MQ, "bound8-1": R.BOUND8_FIRST, "bound-masked": R.BOUND,
            "never-1": R.SMALL, "never-4": R.SMALL, "never-1-k17": R.FUSED, "never-4-k17": R.MQ, "ten-rows": R.SMALL,
            "wide-1": R.SPLIT, "wide-4": R.SMALL, "wide-4-k17": R.SPLIT_MQ, "mq64-40": R.MQ64, "l1-1": R.SMALL, "l1-1-k17": R.FUSED, "l1-200-k17": R.TWO_LAUNCH}
    assert {n: c["route"] for n, c in cases.items()} == want
    assert {c["route"] for c in cases.values()} == set(range(len(R.ROUTES)))
    for name, c in cases.items():
        route, nq, k, tiles, lines = c["route"], c["nq"], c["k"], c["tiles"], trace[name]
        print(name, R.ROUTES[route], "searches +%d, 8-bit +%d" % (c["searches"], c["searches8"]), lines)
        assert c["same"] and c["full"], name
        # the counters: every query of a bound route counts once, the 8-bit stage's own counter only on its route, nothing anywhere else
        assert c["searches"] == (nq if route in R.BOUND_ROUTES else 0), name
        assert c["searches8"] == (1 if route == R.BOUND8_FIRST else 0), name
        # the trace: the route's own line(s), and no other
        if route == R.BOUND_MQ:
            expect = ["qv: scan kernel = k_bound_scan_mq QB=%d (nq=%u, tiles=%u)" % (4 if nq <= 4 else 8, nq, tiles)]
        elif route == R.BOUND8_FIRST:
            expect = ["qv: scan kernel = k_bound_scan8 + k_bound_collect + k_bound_rescore, then gated k_bound_scan + k_bound_collect + k_bound_rescore (tiles=%u, k=%u)" % (tiles, k)]
        elif route == R.BOUND and name == "bound-masked":
            expect = ["qv: scan kernel = k_bound_scan masked (tiles=%u, candidate tiles<=%u, k=%u)" % (tiles, 1, k)]
        elif route == R.BOUND:
            expect = ["qv: scan kernel = k_bound_scan + k_bound_collect + k_bound_rescore (tiles=%u, k=%u)" % (tiles, k)]
        elif route == R.MQ64:                                # 32 queries on the matrix cores, the last 8 split off as a pass of k_flat_scan_mq
            expect = ["qv: scan kernel = k_flat_scan_mq64 (nq=%u, tiles=%u)" % (nq - nq % 32, tiles), "qv: scan kernel = k_flat_scan_mq QB=8 (nq=%u, tiles=%u)" % (nq % 32, tiles)]
        elif route == R.MQ:
            expect = ["qv: scan kernel = k_flat_scan_mq QB=%d (nq=%u, tiles=%u)" % (4 if nq <= 4 else 8, nq, tiles)]
        else:
            expect = []
        assert lines == expect, (name, lines)
