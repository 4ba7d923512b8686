"""The bound scan's routing, pinned: the seven routing exports (the six qv_scan_bound*_applies rules and qv_scan_route_ex) answer today what
they answered when tests/golden/bound_routes.json was recorded, cell for cell, over a grid that brackets every floor and fraction in the rules
(tests/golden/make_bound_routes.py states the grid, and wrote the file from the library's own answers).  No device is touched."""
import base64
import importlib.util
import json
import os

import pytest

from quiver_amd import _lib

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_bound_routes", os.path.join(_GOLDEN, "make_bound_routes.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
RECORDED = json.load(open(os.path.join(_GOLDEN, "bound_routes.json")))["exports"]


def test_the_file_holds_every_export():
    assert set(RECORDED) == set(G.EXPORTS)


@pytest.mark.parametrize("export", G.EXPORTS)
def test_the_export_answers_what_it_answered(export):
    rec = RECORDED[export]
    got = G.answers(_lib.lib(), export)
    assert len(got) == rec["cells"]                                      # (the grid the file was written from)
    want = base64.b64decode(rec["packed"])
    if G.pack(got, G.bits_of(export)) != want:
        bits = G.bits_of(export)
        per = 8 // bits
        moved = [(a, (want[i // per] >> (8 - bits - bits * (i % per))) & ((1 << bits) - 1), got[i])
                 for i, a in enumerate(G.grid(export)) if (want[i // per] >> (8 - bits - bits * (i % per))) & ((1 << bits) - 1) != got[i]]
        pytest.fail("%s: %d of %d cells moved; the first (arguments, recorded, now): %r" % (export, len(moved), len(got), moved[:5]))
    assert rec["taken"] > 0                                              # (a grid on which the export never says yes pins nothing)
