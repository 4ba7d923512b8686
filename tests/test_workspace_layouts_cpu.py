"""The search workspaces' layouts, on the host (qv_scan_workspace_layout runs the layout function a launcher takes its pointers from on a
null base): over the grid of tests/golden/make_workspace_bytes.py every layout's `total` is the size recorded from the hand-written
formulas it replaced (tests/golden/workspace_bytes.json), byte for byte, and its regions lie inside it — in order, apart, aligned, none
empty.  A search's buffer is allocated half as large again as asked, so no GPU test can see a region that ends past `total`: this is the
guard.  No device is touched."""
import importlib.util
import json
import os

import numpy as np
import pytest

from quiver_amd import _lib

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_workspace_bytes", os.path.join(_GOLDEN, "make_workspace_bytes.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
RECORDED = json.load(open(os.path.join(_GOLDEN, "workspace_bytes.json")))["kinds"]

# how many regions a kind's layout has (a range where a shape adds some), and from which one on they are declared aliases: the shared
# bound pass's redo workspace over its candidates and lower bounds; behind a flat call's partial lists and query blocks, the buffers
# that take their place on other routes
REGIONS = {"bound": (8, 8), "bound_mq": (9, 9), "redo": (3, 3), "select": (3, 3), "flat_wide": (2, 2), "flat_select": (2, 3), "flat_select_redo": (6, 6),
           "merge_select": (2, 2), "merge_ranked": (3, 3), "full_sort": (3, 3), "mq64": (4, 4), "rowset": (2, 2), "flat": (4, 5), "rowsets_call": (2, 2),
           "where_call": (3, 3)}
ALIAS_FROM = {"bound_mq": 8, "flat": 2}
# regions the hand-written ladders did NOT start on a 256-byte boundary (every other one they did, by rounding or by the sizes before it):
# the lower bounds behind the single-query bound scan's 8-bit query state, the second key buffer and the histogram of the two full sorts
NOT_256 = {"bound": {7}, "merge_ranked": {1, 2}, "full_sort": {1, 2}}


def test_the_file_holds_every_kind():
    assert set(RECORDED) == set(G.KINDS)


@pytest.mark.parametrize("kind", list(G.KINDS))
def test_the_layout_is_the_recorded_size_and_its_regions_lie_inside_it(kind):
    want = G.unpack(RECORDED[kind]["packed"])
    assert want.size == RECORDED[kind]["cells"]
    lo, hi = REGIONS[kind]
    alias_from = ALIAS_FROM.get(kind, hi)
    n_cells = 0
    for i, (cell, total, end, regions) in enumerate(G.layouts(_lib.lib(), kind)):
        n_cells += 1
        assert i < want.size and total == int(want[i]), (kind, cell, total, int(want[i]) if i < want.size else None)
        assert end <= total, (kind, cell, end, total)
        assert lo <= len(regions) <= hi, (kind, cell, regions)
        at = 0                                                             # where the regions that are no alias have got to
        for j, (off, size, align, alias) in enumerate(regions):
            assert size > 0 and off + size <= end, (kind, cell, j, regions, end)
            assert off % align == 0 and (j in NOT_256.get(kind, ()) or off % 256 == 0), (kind, cell, j, regions)
            assert alias == (1 if j >= alias_from else 0), (kind, cell, j, regions)
            if not alias:
                assert off >= at and (j == 0 or off > regions[j - 1][0]), (kind, cell, j, regions)
                at = off + size
    assert n_cells == want.size                                            # (the grid the file was written from)


def test_the_export_refuses_what_is_no_workspace():
    import ctypes as C
    lib = _lib.lib()
    t, e, n = C.c_uint64(), C.c_uint64(), C.c_uint32()
    ok = (0, 0, 768, 1_000_000, 1, 10, 256, 0)
    assert lib.qv_scan_workspace_layout(*ok, C.byref(t), C.byref(e), C.byref(n), None, 0) == 0 and n.value == 8 and 0 < e.value <= t.value
    for bad in ((99,) + ok[1:], (-1,) + ok[1:], ok[:2] + (0,) + ok[3:], ok[:3] + (0,) + ok[4:], ok[:3] + (1 << 32,) + ok[4:], ok[:4] + (0,) + ok[5:],
                ok[:5] + (0,) + ok[6:], ok[:6] + (0,) + ok[7:], (0, 99) + ok[2:]):
        assert lib.qv_scan_workspace_layout(*bad, C.byref(t), C.byref(e), C.byref(n), None, 0) == _lib.QV_ERR_INVALID_ARG, bad
    assert lib.qv_scan_workspace_layout(*ok, None, C.byref(e), C.byref(n), None, 0) == _lib.QV_ERR_INVALID_ARG
    assert lib.qv_scan_workspace_layout(*ok, C.byref(t), C.byref(e), C.byref(n), None, 4) == _lib.QV_ERR_INVALID_ARG
    regs = (C.c_uint64 * 8)()                                              # fewer entries than regions: the first `cap` are written, the count is whole
    assert lib.qv_scan_workspace_layout(*ok, C.byref(t), C.byref(e), C.byref(n), regs, 2) == 0 and n.value == 8 and regs[4] > 0
