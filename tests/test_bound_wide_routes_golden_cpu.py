"""The wide bound scan's routing (65 to 1024 results), pinned: the four qv_scan_bound_wide_route* exports answer today what they answered when
tests/golden/bound_wide_routes.json was recorded, cell for cell, over a grid that brackets every constant their rules read
(tests/golden/make_bound_wide_routes.py states the grid, and wrote the file from the library's own answers).  No device is touched."""
import base64
import importlib.util
import json
import os

import pytest

from quiver_amd import _lib

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_bound_wide_routes", os.path.join(_GOLDEN, "make_bound_wide_routes.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
RECORDED = json.load(open(os.path.join(_GOLDEN, "bound_wide_routes.json")))["exports"]


def _cell(packed, i):
    per = 8 // G.BITS
    return (packed[i // per] >> (8 - G.BITS - G.BITS * (i % per))) & ((1 << G.BITS) - 1)


def test_the_file_holds_every_export():
    assert set(RECORDED) == set(G.EXPORTS)


@pytest.mark.parametrize("export", G.EXPORTS)
def test_the_export_answers_what_it_answered(export):
    rec = RECORDED[export]
    got = G.answers(_lib.lib(), export)
    assert len(got) == rec["cells"]                                      # (the grid the file was written from)
    want = base64.b64decode(rec["packed"])
    if G.pack(got, G.BITS) != want:
        moved = [(a, _cell(want, i), got[i]) for i, a in enumerate(G.grid(export)) if _cell(want, i) != got[i]]
        pytest.fail("%s: %d of %d cells moved; the first (arguments, recorded, now): %r" % (export, len(moved), len(got), moved[:5]))
    # (a grid on which an answer never occurs pins nothing of it; the filtered shared pass's automatic mode takes nothing, and that is pinned too)
    assert 1 in got and 2 in got
    assert (rec["taken_auto"] == 0) == (export in G.AUTO_TAKES_NOTHING)
