"""Writes tests/golden/bound_wide_routes.json: what the library's four wide-form routing exports (65 to 1024 results: one query or a shared pass of
2 to 8, each unfiltered or filtered) answered, recorded BEFORE their four rules were folded into one decision (qv_bound_scan.hip:
bound_wide_decide), over a grid that brackets every constant those rules read.  tests/test_bound_wide_routes_golden_cpu.py replays the grid
through the exports and asserts equality cell for cell.  The answers are the library's own (no restatement of the rules here), so the file is
rewritten only when a routing change is MEANT, from a build of the commit whose answers are to be pinned, with no QV_BOUND_* variable set:

    python tests/golden/make_bound_wide_routes.py        # rewrites bound_wide_routes.json next to it

The grid (the module is the one statement of it: the test enumerates it from here, in the same order):
  metric  cosine, dot, l2 (refused), the rule code of an l2 index that holds the planes (served, never automatic), l1 (refused)
  dim     0 (refused although it is a multiple of 16), 16 (below the narrow floor), 112, 128 (the narrow floor), 752, 768 (the wide floor),
          4096 (the widest), 120 and 4112 (refused)
  rows    448 and 512 (7 and 8 tiles: the kernels' minimum); 1000 (so that a k of the grid EQUALS the rows, and the next is above them); one
          below, at and above 1 M, 3 M and 10 M (every floor); 2^26 and one more (the redo's row limit, and 8 queries' lower-bound planes at
          and over 2 GiB)
  nq      1, 2, 4, 5, 8, 9 (both ends of both QB classes, and one past)
  k       64, 65 (the shortest wide list), 1000, 1001 (the automatic cap), 1024, 1025 (the kernels' cap)
  tiles   that hold a candidate: 0; one under and at 100, 475 and 1000 per mille of the tiles; one more than there are
  rows    the filter selects: k (nothing to reject) and k + 1
  knobs   all nine (mode, plane mode) pairs, the copy and the 8-bit plane each held and not held
THINNED as bound_routes.json is — interior points only, never the straddle of a constant: a cell the kernels refuse whatever the knobs say (a
metric, width, nq or k they do not serve) is asked once, with every knob at its most permissive; a plane that is not held is asked under the
automatic and the most permissive modes; under "never" a filtered cell is asked once, under "always" on both knobs with no tile and with
every tile, and the candidate tiles are walked only where a mode is automatic; the selected rows are varied wherever the mode is not "never"."""
import base64
import importlib.util
import itertools
import json
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_bound_routes", os.path.join(_HERE, "make_bound_routes.py"))
_R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_R)
pack, METRICS, MODES, NQS = _R.pack, _R.METRICS, _R.MODES, _R.NQS
COSINE, DOT, L2_PLANES = _R.COSINE, _R.DOT, _R.L2_PLANES

DIMS = (0, 16, 112, 120, 128, 752, 768, 4096, 4112)
ROWS = (448, 512, 1000) + tuple(f + d for f in (1_000_000, 3_000_000, 10_000_000) for d in (-1, 0, 1)) + (1 << 26, (1 << 26) + 1)
KS = (64, 65, 1000, 1001, 1024, 1025)
EXPORTS = ("qv_scan_bound_wide_route", "qv_scan_bound_wide_route_filtered", "qv_scan_bound_wide_route_mq", "qv_scan_bound_wide_route_filtered_mq")
FILTERED = ("qv_scan_bound_wide_route_filtered", "qv_scan_bound_wide_route_filtered_mq")
AUTO_TAKES_NOTHING = ("qv_scan_bound_wide_route_filtered_mq",)             # its automatic floors are all zero rows
BITS = 2                                                                   # an answer is 0, 1 or 2
_NQ_SERVED = {"qv_scan_bound_wide_route": (1,), "qv_scan_bound_wide_route_filtered": (1,),
              "qv_scan_bound_wide_route_mq": (2, 4, 5, 8), "qv_scan_bound_wide_route_filtered_mq": (2, 4, 5, 8)}
_PLANES_NOT_HELD = [(0, 0, 1, 0), (1, 1, 1, 0), (0, 0, 0, 1), (1, 1, 0, 1), (1, 1, 0, 0)]   # (mode, plane mode, copy held, plane held)


def candidate_tiles(rows):
    t = (rows + 63) // 64
    at = [(t * f + 999) // 1000 for f in (100, 475, 1000)]              # the smallest counts with ct * 1000 >= t * f
    return (0,) + tuple(c - d for c in at for d in (1, 0)) + (t + 1,)


def _knobs(export, served, k, cts):
    """(mode, plane mode, copy held, plane held) and, for a filtered export, (candidate tiles, selected rows) behind them"""
    every = cts[-2]
    if export not in FILTERED:
        return [(m, p, 1, 1) for m in MODES for p in MODES] + _PLANES_NOT_HELD if served else [(1, 1, 1, 1)]
    if not served: return [(1, 1, 1, 1, every, k + 1)]
    out = []
    for m, p in itertools.product(MODES, MODES):
        if m == 2: out.append((m, p, 1, 1, every, k + 1))
        else: out += [(m, p, 1, 1, c, n) for c in (cts if m == 0 or p == 0 else (0, every)) for n in (k, k + 1)]
    return out + [h + (every, k + 1) for h in _PLANES_NOT_HELD]


def grid(export):
    """the argument tuples of one export, in the order their answers are stored"""
    for metric, dim, rows in itertools.product(METRICS, DIMS, ROWS):
        cts = candidate_tiles(rows)
        shape_served = metric in (COSINE, DOT, L2_PLANES) and dim != 0 and dim % 16 == 0 and dim <= 4096
        for nq, k in itertools.product(NQS, KS):
            for knobs in _knobs(export, shape_served and nq in _NQ_SERVED[export] and 65 <= k <= 1024, k, cts):
                yield (metric, dim, rows, nq, k) + knobs


def answers(lib, export):
    """one small int per cell: 0 no, 1 the bfloat16 copy first, 2 the 8-bit plane first"""
    fn = getattr(lib, export)
    out = bytearray()
    for a in grid(export):
        rc = fn(*a)
        assert rc in (0, 1, 2), (export, a, rc)
        out.append(rc)
    return bytes(out)


def main():
    from quiver_amd import _lib
    lib = _lib.lib()
    doc = {"_comment": "The answers of the library's four wide-form routing exports over the grid of make_bound_wide_routes.py, which wrote this "
                       "file; cells in that module's order, 2 bits each (0 no, 1 the bfloat16 copy first, 2 the 8-bit plane first), base64.", "exports": {}}
    for export in EXPORTS:
        got = answers(lib, export)
        auto = [v for a, v in zip(grid(export), got) if a[5] == 0]
        assert 1 in got and 2 in got, export                                # (a grid on which an answer never occurs pins nothing of it)
        assert not any(auto) if export in AUTO_TAKES_NOTHING else any(auto), export
        doc["exports"][export] = {"cells": len(got), "taken": sum(1 for v in got if v), "taken_auto": sum(1 for v in auto if v), "packed": base64.b64encode(pack(got, BITS)).decode()}
        print(export, len(got), "cells,", doc["exports"][export]["taken"], "not 0,", doc["exports"][export]["taken_auto"], "of them automatic")
    path = os.path.join(_HERE, "bound_wide_routes.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.join(_HERE, "..", ".."))
    main()
