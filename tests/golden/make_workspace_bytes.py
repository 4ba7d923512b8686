"""Writes tests/golden/workspace_bytes.json: the size of every search workspace as the library's hand-written *_workspace_bytes formulas gave
it, recorded through qv_scan_workspace_layout BEFORE those formulas and the launchers' pointer ladders were folded into one layout function
per buffer.  tests/test_workspace_layouts_cpu.py replays the grid and asserts that every layout's `total` is the recorded size, byte for
byte, and that the regions it reports lie inside it.  The sizes are the library's own (no restatement of a formula here), so the file is
rewritten only when a size change is MEANT, from a build of the commit whose sizes are to be pinned:

    python tests/golden/make_workspace_bytes.py        # rewrites workspace_bytes.json next to it

The grid (the module is the one statement of it: the test enumerates it from here, in the same order) brackets every branch the sizes take:
  rows    one tile; 8 tiles (the bound scan's minimum); 9 000; the small scan's limit of 256 tiles and one row past it; 1M; 10M; the most an
          index admits
  dim     1, 3, 16, 80, 768, 1536, 4048 and the bound scan's widest, 4096
  nq      both sides of 1 / 2, 4 / 5, 8 / 9, 16 / 17, 64 / 65, 128 / 129, 256 / 257; 8192 (a host pass); 13 / 14 and 134 / 135, where a group
          of the key-per-row path reaches 1 GiB of keys at 10M and at 1M rows
  k       both sides of 16, 64 (the fused lists), 128 (the wide lists), 4096 (the selection's sort capacity) and 8192 (the selection's limit)
  cus     1 and 256
Each kind takes the axes its layout reads (a kind that has no scan plan is asked with one device size, one that reads no width with the
extreme widths) and only the combinations its launcher accepts; ACCEPTS below states those conditions.
FIXED: cells whose recorded size was found SHORT of where the layout's last region ends, and was therefore raised (none so far)."""
import base64
import ctypes as C
import itertools
import json
import os
import zlib

import numpy as np

COSINE = 0
ROWS = (64, 512, 9000, 16384, 16385, 1_000_000, 10_000_000, 0xFFFFFFF0)
DIMS = (1, 3, 16, 80, 768, 1536, 4048, 4096)
NQS = (1, 2, 4, 5, 8, 9, 13, 14, 16, 17, 64, 65, 128, 129, 134, 135, 256, 257, 8192)
KS_FUSED = (1, 15, 16, 17, 63, 64)
KS_WIDE = (65, 127, 128)
KS_SELECT = (65, 127, 128, 129, 4095, 4096, 4097, 8191, 8192)
CUS = (1, 256)
KINDS = {"bound": 0, "bound_mq": 1, "redo": 2, "select": 3, "flat_wide": 4, "flat_select": 5, "flat_select_redo": 6, "merge_select": 7,
         "merge_ranked": 8, "full_sort": 9, "mq64": 10, "rowset": 11, "flat": 12, "rowsets_call": 13, "where_call": 14}
FLAT_PLAIN, FLAT_BOUND, FLAT_BOUND_MQ = 0, 1, 2
REGION_CAP = 24
FIXED = {}                                                                 # (kind, cell) -> why the recorded size was raised


def tiles(rows):
    return (rows + 63) // 64


# ACCEPTS: what the launchers take (the conditions are theirs: bound_scan_kernels_serve, mq64_blocks, launch_flat_select_redo)
BOUND_DIMS = tuple(d for d in DIMS if d % 16 == 0)                         # whole 16-dimension steps up to 4096


def bound_rows(nq):                                                        # 8 tiles or more; nq planes of lower bounds up to 2 GiB
    return tuple(r for r in ROWS if tiles(r) >= 8 and (nq == 1 or nq * tiles(r) * 256 <= 2 << 30))


def select_group(rows, nq):                                                # queries whose keys (8 bytes per row slot) stay within 1 GiB
    return max(1, min(nq, (1 << 30) // (tiles(rows) * 512)))


MQ64_DIMS = tuple(d for d in DIMS if (d + 3) // 4 <= 284)                   # the query fragments fit the LDS beside the wave lists


def grid(kind):
    """the argument tuples (metric, dim, rows, nq, k, cus, flags) of one kind, in the order their sizes are stored"""
    def cells(dims, rows, nqs, ks, cus=(256,), flags=(0,)):
        for dim, r, nq, k, c, f in itertools.product(dims, rows, nqs, ks, cus, flags):
            yield (COSINE, dim, r, nq, k, c, f)
    if kind == "bound":
        yield from cells(BOUND_DIMS, bound_rows(1), (1,), KS_FUSED, CUS)
    elif kind == "bound_mq":
        for nq in (2, 4, 5, 8):
            yield from cells(BOUND_DIMS, bound_rows(nq), (nq,), KS_FUSED, CUS)
    elif kind == "redo":
        yield from cells((1, 4096), ROWS, NQS, KS_FUSED, CUS)
    elif kind == "select":
        yield from cells((768,), (1_000_000,), NQS, KS_FUSED + KS_SELECT)
    elif kind == "flat_wide":
        yield from cells((1, 4096), ROWS, (1, 2), KS_WIDE, CUS)
    elif kind == "flat_select":
        yield from cells(DIMS, ROWS, NQS, KS_FUSED + KS_SELECT)
    elif kind == "flat_select_redo":
        for nq in NQS:
            yield from cells(DIMS, tuple(r for r in ROWS if select_group(r, min(nq, 64)) >= 2), (nq,), KS_SELECT)
    elif kind == "merge_select":                                           # rows = entries per gathered list, flags = lists
        yield from cells((768,), (65, 128, 4097, 8192, 100_000), (1, 2, 9, 256), KS_SELECT, flags=(1, 2, 8))
    elif kind == "merge_ranked":                                           # rows = keys
        yield from cells((768,), (1, 2, 64, 65, 9000, 1 << 20, 10_000_000, 0xFFFFFF00), (1,), (65,))
    elif kind == "full_sort":
        yield from cells((1, 4096), ROWS, (1,), (8193,))
    elif kind == "mq64":
        yield from cells(MQ64_DIMS, (1_000_000,), tuple(n for n in NQS if n >= 9), (10,))
    elif kind == "rowset":
        yield from cells(DIMS, ROWS, NQS, KS_FUSED, CUS)
    elif kind == "flat":
        yield from cells(DIMS, ROWS, NQS, KS_FUSED, CUS, (FLAT_PLAIN,))
        yield from cells(BOUND_DIMS, bound_rows(1), (1,), KS_FUSED, CUS, (FLAT_BOUND,))
        for nq in (2, 4, 5, 8):
            yield from cells(BOUND_DIMS, bound_rows(nq), (nq,), KS_FUSED, CUS, (FLAT_BOUND_MQ,))
    elif kind in ("rowsets_call", "where_call"):                            # flags: bit 0 = sized for the shared bound pass too; from bit 8: distinct filters
        for nq in NQS[1:]:
            uniq = (0,) if kind == "rowsets_call" else (1 << 8, nq << 8)
            yield from cells((1, 80, 4096), ROWS, (nq,), KS_FUSED, CUS, uniq)
            if nq <= 8:
                yield from cells(BOUND_DIMS, bound_rows(nq), (nq,), KS_FUSED, CUS, tuple(u | 1 for u in uniq))
    else:
        raise KeyError(kind)


def layouts(lib, kind):
    """(cell, total, end, regions) per cell of the kind's grid; regions: a list of (offset, bytes, align, alias)"""
    total, end, n = C.c_uint64(), C.c_uint64(), C.c_uint32()
    regs = (C.c_uint64 * (4 * REGION_CAP))()
    fn, code = lib.qv_scan_workspace_layout, KINDS[kind]
    for cell in grid(kind):
        rc = fn(code, *cell, C.byref(total), C.byref(end), C.byref(n), regs, REGION_CAP)
        assert rc == 0 and n.value <= REGION_CAP, (kind, cell, rc, n.value)
        flat = regs[:4 * n.value]
        yield cell, total.value, end.value, [tuple(flat[i:i + 4]) for i in range(0, len(flat), 4)]


def totals(lib, kind):
    return np.array([t for _, t, _, _ in layouts(lib, kind)], dtype="<u8")


def pack(sizes):
    """little-endian uint64 per cell, zlib, base64"""
    return base64.b64encode(zlib.compress(np.asarray(sizes, dtype="<u8").tobytes(), 9)).decode()


def unpack(text):
    return np.frombuffer(zlib.decompress(base64.b64decode(text)), dtype="<u8")


def main():
    from quiver_amd import _lib
    lib = _lib.lib()
    doc = {"_comment": "The sizes of the search workspaces over the grid of make_workspace_bytes.py, which wrote this file; per kind the cells in that "
                       "module's order as little-endian uint64, zlib, base64.", "kinds": {}}
    for kind in KINDS:
        got = totals(lib, kind)
        doc["kinds"][kind] = {"cells": int(got.size), "packed": pack(got)}
        print(kind, got.size, "cells,", int(got.min()), "..", int(got.max()), "bytes")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "workspace_bytes.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    main()
