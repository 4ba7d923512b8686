"""The host side of DeviceIndex.search_where that needs no device: the packing of predicates into the arrays a qv_where points to,
broadcast / None handling of the `filters` argument, and FacetColumns' choice between the fused call and the set path (read off
facets.plan outputs)."""
import ctypes as C

import numpy as np
import pytest

from quiver_amd import core, facets
from quiver_amd.device_index import (PREDICATES, QvWhere, WHERE_DEVICE_LITERALS, WHERE_FILTERS_PER_LAUNCH, broadcast_filters,
                                     pack_predicates, pack_where)


class _Col:
    """stands in for a Column: pack_predicates only needs a handle"""

    def __init__(self, h):
        self.h = h


def _h(col):
    return col.h


A, B = _Col(0x1000), _Col(0x2000)


def test_constants_match_the_header():
    import os
    import re
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "qv.h")).read()
    assert int(re.search(r"#define QV_WHERE_FILTERS_PER_LAUNCH (\d+)", text).group(1)) == WHERE_FILTERS_PER_LAUNCH
    assert int(re.search(r"#define QV_WHERE_DEVICE_LITERALS (\d+)", text).group(1)) == WHERE_DEVICE_LITERALS
    for name, code in (("EQ", "eq"), ("NE", "ne"), ("LT", "lt"), ("LE", "le"), ("GT", "gt"), ("GE", "ge"), ("IN", "in"),
                       ("NOT_IN", "not_in"), ("PRESENT", "present"), ("ABSENT", "absent")):
        assert int(re.search(r"#define QV_PRED_%s (\d+)" % name, text).group(1)) == PREDICATES[code]
    # the struct's layout is the header's: four pointers and a uint32
    assert [f[0] for f in QvWhere._fields_] == ["cols", "ops", "literals", "lit_off", "n_preds"]
    assert C.sizeof(QvWhere) == 4 * C.sizeof(C.c_void_p) + 8


def test_pack_predicates():
    cols, ops, lits, off = pack_predicates([(A, "<", 37.5), (B, "in", [1, 2, 3]), (A, "present", None), (B, 5, np.float32(2.0))], _h)
    assert cols.dtype == np.uint64 and cols.tolist() == [0x1000, 0x2000, 0x1000, 0x2000]
    assert ops.dtype == np.int32 and ops.tolist() == [2, 6, 8, 5]
    assert lits.dtype == np.float64 and lits.tolist() == [37.5, 1.0, 2.0, 3.0, 2.0]
    assert off.dtype == np.uint32 and off.tolist() == [0, 1, 4, 4, 5]
    cols, ops, lits, off = pack_predicates([], _h)
    assert cols.size == 0 and ops.size == 0 and lits.size == 0 and off.tolist() == [0]
    cols, ops, lits, off = pack_predicates([(A, "IN", [])], _h)                      # an empty list stays empty: the library refuses it
    assert off.tolist() == [0, 0] and ops.tolist() == [6]
    with pytest.raises(KeyError):
        pack_predicates([(A, "like", 1.0)], _h)
    with pytest.raises(TypeError):
        pack_predicates([(object(), "eq", 1.0)])                                    # the default handle_of wants a Column


def test_pack_where_points_into_the_arrays():
    per_query = [[(A, "ge", 1.5), (B, "not_in", [7, 9])], [], [(B, "absent", None)]]
    arr, keep = pack_where(per_query, _h)
    assert len(arr) == 3 and len(keep) == 3
    w = arr[0]
    assert w.n_preds == 2 and [w.cols[i] for i in range(2)] == [0x1000, 0x2000] and [w.ops[i] for i in range(2)] == [5, 7]
    assert [w.lit_off[i] for i in range(3)] == [0, 1, 3] and [w.literals[i] for i in range(3)] == [1.5, 7.0, 9.0]
    assert C.addressof(w.literals.contents) == keep[0][2].ctypes.data               # no copy: the struct points at the kept arrays
    e = arr[1]
    assert e.n_preds == 0 and not e.cols and not e.ops and not e.literals and e.lit_off[0] == 0
    a = arr[2]
    assert a.n_preds == 1 and a.ops[0] == 9 and not a.literals and [a.lit_off[i] for i in range(2)] == [0, 0]
    arr0, _ = pack_where([], _h)                                                    # nq == 0: still a valid pointer
    assert len(arr0) == 1


def test_broadcast_filters():
    one = [(A, "lt", 3.0), (B, "eq", 4)]
    assert broadcast_filters(None, 3) == [[], [], []]
    assert broadcast_filters(one, 3) == [one, one, one]
    assert broadcast_filters([], 2) == [[], []]                                     # the empty conjunction for every query
    per = [one, None, [(B, "present", None)]]
    assert broadcast_filters(per, 3) == [one, [], [(B, "present", None)]]
    assert broadcast_filters([None, None], 2) == [[], []]
    assert broadcast_filters(tuple(one), 1) == [one]
    with pytest.raises(ValueError):
        broadcast_filters(per, 2)
    with pytest.raises(TypeError):
        broadcast_filters([one, [(A, "lt")]], 2)
    # a single predicate is not mistaken for a list of them, whatever its literal is
    assert broadcast_filters([(A, "in", [1, 2, 3])], 2) == [[(A, "in", [1, 2, 3])]] * 2
    assert broadcast_filters([(A, 6, (1, 2, 3))], 1) == [[(A, 6, (1, 2, 3))]]


def _dictionaries():
    md = [{"price": 1.0 * i, "tag": "t%d" % (i % 5), "mixed": (i if i % 2 else "s%d" % i)} for i in range(40)]
    return facets.build_arrays(md, ["price", "tag", "mixed"])[1]


def test_facets_choose_the_fused_call_for_single_term_plans():
    d = _dictionaries()
    F = core.Filter
    cases = [
        ([F("price", core.LessThan, 37.5)], 1),
        ([F("price", core.GreaterThanOrEqual, 3.0), F("price", core.LessThan, 9.0), F("tag", core.Equals, "t3")], 3),
        ([F("tag", core.In, ["t1", "t2"])], 1),
    ]
    for filters, n in cases:
        pl = facets.plan(filters, d)
        assert all(len(t) == 1 for t in pl)
        preds = facets.fused_predicates(pl)
        assert preds is not None and len(preds) == n == sum(len(t[0]) for t in pl)
        assert preds == [p for t in pl for p in t[0]]                               # the order of the plan: most selective first is the caller's
    # the set path: no filter (the snapshot's rows only), a filter that matches nothing, a mixed-type field (two terms), more than 8 predicates
    assert facets.fused_predicates(facets.plan([], d)) is None
    nothing = facets.plan([F("tag", core.Equals, "absent-string")], d)
    assert nothing == [[]] and facets.fused_predicates(nothing) is None
    mixed = facets.plan([F("mixed", core.LessThan, 7)], d)
    assert len(mixed[0]) == 2 and facets.fused_predicates(mixed) is None
    nine = facets.plan([F("price", core.NotEquals, float(i)) for i in range(9)], d)
    assert all(len(t) == 1 for t in nine) and facets.fused_predicates(nine) is None
    eight = facets.plan([F("price", core.NotEquals, float(i)) for i in range(8)], d)
    assert len(facets.fused_predicates(eight)) == 8


def test_facets_search_calls_what_the_plan_says():
    """FacetColumns.search on a stand-in index: the fused call gets the plan's predicates over the snapshot's columns; otherwise the
    set is made, searched and closed"""
    calls = []

    class Set:
        def close(self):
            calls.append("close")

    class Index:
        def search_where(self, q, k, preds):
            calls.append(("where", k, preds)); return "W"

        def search_rowsets(self, q, k, s):
            calls.append(("sets", k, type(s))); return "S"

    fc = facets.FacetColumns.__new__(facets.FacetColumns)
    fc.index, fc.dictionaries = Index(), _dictionaries()
    fc.columns = {f: {"num": (f, "num"), "str": (f, "str")} for f in fc.dictionaries}
    fc.rowset = lambda filters: Set()
    assert fc.search(None, 10, [core.Filter("price", core.LessThan, 37.5)]) == "W"
    assert calls == [("where", 10, [(("price", "num"), facets.LT, (37.5,))])]
    calls.clear()
    assert fc.search(None, 5, [core.Filter("mixed", core.LessThan, 7)]) == "S"
    assert calls == [("sets", 5, Set), "close"]
