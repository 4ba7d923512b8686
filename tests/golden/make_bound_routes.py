"""Writes tests/golden/bound_routes.json: what the library's seven routing exports answered, recorded BEFORE the six bound-scan rules were
folded into one decision (qv_bound_scan.hip: bound_scan_decide), over a grid that brackets every floor and fraction in those rules.
tests/test_bound_routes_golden_cpu.py replays the grid through the exports and asserts equality: whatever the routing code is turned into,
it answers what it answered then.  The answers are the library's own (no restatement of the rules here), so the file is rewritten only when a
routing change is MEANT, from a build of the commit whose answers are to be pinned:

    python tests/golden/make_bound_routes.py        # rewrites bound_routes.json next to it

The grid (the module is the one statement of it: the test enumerates it from here, in the same order):
  metric  cosine, dot, l2 (the rules refuse it), the rule code of an l2 index that holds the planes, l1 (refused, and a route's metric)
  dim     16 (below every narrow floor), 112, 128 (the narrow floors), 752, 768 (the wide floors), 4096 (the widest), 120 and 4112 (refused)
  rows    448 and 512 (7 and 8 tiles: the kernels' minimum); one below, at and above 300 k, 1 M, 3 M and 10 M (every floor); 2^26 and one more
          (8 queries' lower-bound planes at and over 2 GiB)
  nq      1, 2, 4, 5, 8, 9 (both ends of both QB classes, and one past)        k   1, 10, 11 (the QB = 8 clause under a filter), 64, 65
  tiles   that hold a candidate: 0; one under and at a tenth, a fifth, nine tenths and all of the tiles; one more than there are; and the
          value that says "no filter" to qv_scan_route_ex, which the filtered rules take as a count (more than there are)
  knobs   every value of every mode, the planes held and not held
THINNED, so that the replay takes seconds and the file stays far below the size limit for committed files — interior points only, never the
straddle of a floor: a cell the kernels cannot serve whatever the knobs say (a refused metric, width, nq or k) is asked once, with every knob
at its most permissive; a candidate count is varied only under the modes whose answer can depend on it (under "always" on both knobs and
under "never" it is asked with no tile and with every tile); a plane that is not held is asked under the automatic and the most permissive
modes.  The 8-bit rules of a single query are asked with 1 and 2 queries, those of a shared pass with all six nq."""
import base64
import itertools
import json
import os

COSINE, L2, DOT, L1, L2_PLANES = 0, 1, 3, 4, 0x101
METRICS = (COSINE, DOT, L2, L2_PLANES, L1)
DIMS = (16, 112, 120, 128, 752, 768, 4096, 4112)
ROWS = (448, 512) + tuple(f + d for f in (300_000, 1_000_000, 3_000_000, 10_000_000) for d in (-1, 0, 1)) + (1 << 26, (1 << 26) + 1)
NQS = (1, 2, 4, 5, 8, 9)
KS = (1, 10, 11, 64, 65)
MODES = (0, 1, 2)
NO_FILTER = 0xFFFFFFFF
CUS = 256
EXPORTS = ("qv_scan_bound_applies", "qv_scan_bound_applies_filtered", "qv_scan_bound8_applies", "qv_scan_bound8_applies_filtered",
           "qv_scan_bound8_applies_mq", "qv_scan_bound8_applies_filtered_mq", "qv_scan_route_ex")
_NQ_SERVED = {"qv_scan_bound8_applies": (1,), "qv_scan_bound8_applies_filtered": (1,),
              "qv_scan_bound8_applies_mq": (2, 4, 5, 8), "qv_scan_bound8_applies_filtered_mq": (2, 4, 5, 8)}
_NQ_ASKED = {"qv_scan_bound8_applies": (1, 2), "qv_scan_bound8_applies_filtered": (1, 2)}


def candidate_tiles(rows):
    t = (rows + 63) // 64
    at = [(t + 9) // 10, (t + 4) // 5, (9 * t + 9) // 10, t]         # the smallest counts with ct * 10 >= t, ct * 5 >= t, ct * 10 >= 9 t, ct >= t
    return (0,) + tuple(c - d for c in at for d in (1, 0)) + (t + 1, NO_FILTER)


def _plane8_knobs():            # (mode, plane mode, plane held)
    return [(m, p, 1) for m in MODES for p in MODES] + [(0, 0, 0), (1, 1, 0)]


def _plane8_knobs_filtered(cts):   # (mode, plane mode, plane held, candidate tiles)
    out = []
    for m, p in itertools.product(MODES, MODES):
        depends = m != 2 and p != 2 and not (m == 1 and p == 1)
        out += [(m, p, 1, c) for c in (cts if depends else (0, cts[-3]))]
    return out + [(0, 0, 0, cts[-3]), (1, 1, 0, cts[-3])]


def _knobs(export, served, nq, cts):
    every = cts[-3]
    if export == "qv_scan_bound_applies":                                  # (mode, copy held)
        return list(itertools.product(MODES, (1, 0))) if served else [(1, 1)]
    if export == "qv_scan_bound_applies_filtered":                         # (mode, copy held, candidate tiles)
        if not served: return [(1, 1, every)]
        return [(0, 1, c) for c in cts] + [(m, 1, c) for m in (1, 2) for c in (0, every)] + [(m, 0, every) for m in MODES]
    if export in ("qv_scan_bound8_applies", "qv_scan_bound8_applies_mq"):
        return _plane8_knobs() if served else [(1, 1, 1)]
    if export in ("qv_scan_bound8_applies_filtered", "qv_scan_bound8_applies_filtered_mq"):
        return _plane8_knobs_filtered(cts) if served else [(1, 1, 1, every)]
    # qv_scan_route_ex: (cus, tickets, bound mode, plane mode, copy held, plane held, candidate tiles, filtered plane mode)
    no_tickets = (CUS, 0, 0, 0, 1, 1, NO_FILTER, 0)
    if not served: return [no_tickets, (CUS, 1, 1, 1, 1, 1, NO_FILTER, 1), (CUS, 1, 1, 1, 1, 1, every, 1)]
    if nq >= 2:                                                            # (no route of a shared pass depends on a plane mode)
        return [no_tickets, (CUS, 1, 1, 0, 0, 1, NO_FILTER, 0)] + [(CUS, 1, m, 0, 1, 1, c, 0) for m in MODES for c in (cts if m == 0 else (NO_FILTER, 0, every))]
    return ([no_tickets, (CUS, 1, 1, 1, 0, 1, NO_FILTER, 1), (CUS, 1, 1, 1, 0, 1, every, 1)] + [(CUS, 1, m, p, 1, h, NO_FILTER, 2) for m, p, h in _plane8_knobs()] +
            [(CUS, 1, m, 2, 1, h, c, p) for m, p, h, c in _plane8_knobs_filtered(cts[:-1])])


def grid(export):
    """the argument tuples of one export, in the order their answers are stored"""
    nq_served = _NQ_SERVED.get(export, (1, 2, 4, 5, 8))
    for metric, dim, rows in itertools.product(METRICS, DIMS, ROWS):
        cts = candidate_tiles(rows)
        shape_served = metric in (COSINE, DOT, L2_PLANES) and dim % 16 == 0 and dim <= 4096
        for nq, k in itertools.product(_NQ_ASKED.get(export, NQS), KS):
            for knobs in _knobs(export, shape_served and nq in nq_served and k <= 64, nq, cts):
                yield (metric, dim, rows, nq, k) + knobs


def answers(lib, export):
    """one small int per cell: 0 / 1 of a rule, the route's number, 15 where the export refuses its arguments"""
    fn = getattr(lib, export)
    out = bytearray()
    if export == "qv_scan_route_ex":
        for a in grid(export):
            rc = fn(*a)
            assert rc < 15, (a, rc)
            out.append(rc if rc >= 0 else 15)
    else:
        for a in grid(export):
            rc = fn(*a)
            assert rc in (0, 1), (export, a, rc)
            out.append(rc)
    return bytes(out)


def pack(values, bits):
    """`bits` (1 or 4) per value, the first value in the highest bits of the first byte"""
    per = 8 // bits
    values = values + bytes(-len(values) % per)
    out = bytearray(len(values) // per)
    for i, v in enumerate(values):
        out[i // per] |= v << (8 - bits - bits * (i % per))
    return bytes(out)


def bits_of(export):
    return 4 if export == "qv_scan_route_ex" else 1


def main():
    from quiver_amd import _lib
    lib = _lib.lib()
    doc = {"_comment": "The answers of the library's seven routing exports over the grid of make_bound_routes.py, which wrote this file; "
                       "cells in that module's order, bit-packed (a rule: 1 bit; qv_scan_route_ex: 4 bits, 15 = refused), base64.", "exports": {}}
    for export in EXPORTS:
        got = answers(lib, export)
        doc["exports"][export] = {"cells": len(got), "taken": sum(1 for v in got if v not in (0, 15)), "packed": base64.b64encode(pack(got, bits_of(export))).decode()}
        print(export, len(got), "cells,", doc["exports"][export]["taken"], "not 0")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bound_routes.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    main()
