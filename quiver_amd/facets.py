"""Facet columns: the reference's metadata filters (core.matchesFilter, pkg/core/collection.go:530-632) as row sets made on the device.

A snapshot helper on top of the typed columns of include/qv.h ("facet columns").  Per metadata field it keeps

* an F64 column ("num"), present where the value is a JSON number and not a bool (core._as_float), and
* a U32 column ("str") of RANKS of core._go_str(value) in the field's sorted string dictionary, present wherever the field exists
  (a null value included: its string is "<nil>").  Ranks follow string order, so a string ``<`` / ``>`` is an unsigned comparison
  against the literal's bisected position, and a string the dictionary does not hold equals no row.

matchesFilter compares numerically when BOTH sides are numbers and by "%v" string otherwise.  ``plan`` restates that per filter as
an OR of conjunctions ("terms") of column predicates:

* a numeric filter value applies the numeric comparison to the rows whose value is numeric and the string comparison to the
  others ("num" absent); a non-numeric value applies the string comparison to every row that has the field;
* In / NotIn take the numeric literals numerically on numeric rows, the other literals' strings on numeric rows too ("5" equals
  5 by string), and every literal's string on the other rows; NotIn with a non-list value is "the field exists";
* a field whose rows are all numeric, or all non-numeric (the dictionaries say so), is the normal case and needs ONE term.

Filters whose plan is a single term are evaluated together in one kernel pass; only a mixed-type field costs further passes and
ORs (qv_rowset_combine).  Lists longer than 256 literals become several terms (In) or several predicates (NotIn); conjunctions
longer than 8 predicates several passes ANDed.

``evaluate_host`` is the numpy statement of what the kernels compute for a plan; tests/test_facets_cpu.py holds plan +
evaluate_host against matchesFilter row by row.

NotServable — the filters the typed columns cannot express, for which ``plan`` raises rather than answer wrongly:

* a filter on a field that is not among the snapshot's ``fields`` (no column holds it).

Nothing else is refused: every operator of core.py:42-46 on every mix of value types is exact.
"""
from __future__ import annotations

from bisect import bisect_left, bisect_right
from collections import namedtuple

import numpy as np

from . import core
from .core import _as_float, _go_str

EQ, NE, LT, LE, GT, GE, IN, NOT_IN, PRESENT, ABSENT = range(10)            # QV_PRED_* of include/qv.h
MAX_PREDS, MAX_LITS = 8, 256

Pred = namedtuple("Pred", "field kind op literals")                        # kind: "num" (the F64 column) or "str" (the U32 rank column)
Dictionary = namedtuple("Dictionary", "strings numeric other")            # sorted distinct strings; any numeric row; any non-numeric row

_NUM_OP = {core.Equals: EQ, core.NotEquals: NE, core.GreaterThan: GT, core.GreaterThanOrEqual: GE, core.LessThan: LT, core.LessThanOrEqual: LE}


class NotServable(ValueError):
    """a filter the typed columns cannot express (the module docstring lists the cases)"""


def build_arrays(metadata_per_row, fields):
    """-> (arrays, dictionaries): arrays[field] = {"num": (float64 values, bool present), "str": (uint32 ranks, bool present)},
    dictionaries[field] = Dictionary.  A row whose metadata is None has no field."""
    n = len(metadata_per_row)
    arrays, dictionaries = {}, {}
    for f in fields:
        num = np.zeros(n, dtype=np.float64); num_p = np.zeros(n, dtype=bool)
        strs = [None] * n
        for i, md in enumerate(metadata_per_row):
            if md is None or f not in md:
                continue
            v = md[f]
            fv = _as_float(v)
            if fv is not None:
                num[i] = fv; num_p[i] = True
            strs[i] = _go_str(v)
        str_p = np.array([s is not None for s in strs], dtype=bool)
        D = sorted({s for s in strs if s is not None})
        rank = {s: r for r, s in enumerate(D)}
        ranks = np.array([rank[s] if s is not None else 0 for s in strs], dtype=np.uint32)
        arrays[f] = {"num": (num, num_p), "str": (ranks, str_p)}
        dictionaries[f] = Dictionary(D, bool(num_p.any()), bool((str_p & ~num_p).any()))
    return arrays, dictionaries


def _str_preds(field, d, op, s):
    """the string comparison `row op s` on the rank column: a list of predicates, or None when no row can pass"""
    D = d.strings
    lo, hi = bisect_left(D, s), bisect_right(D, s)
    if op == core.Equals:
        return [Pred(field, "str", EQ, (float(lo),))] if hi > lo else None
    if op == core.NotEquals:
        return [Pred(field, "str", NE, (float(lo),))] if hi > lo else [Pred(field, "str", PRESENT, ())]
    if op == core.LessThan:
        return [Pred(field, "str", LT, (float(lo),))] if lo > 0 else None
    if op == core.LessThanOrEqual:
        return [Pred(field, "str", LT, (float(hi),))] if hi > 0 else None
    if op == core.GreaterThan:
        return [Pred(field, "str", GE, (float(hi),))] if hi < len(D) else None
    return [Pred(field, "str", GE, (float(lo),))] if lo < len(D) else None     # GreaterThanOrEqual


def _chunks(xs):
    return [tuple(xs[i:i + MAX_LITS]) for i in range(0, len(xs), MAX_LITS)]


def _codes(d, strings):
    rank = []
    for s in strings:
        lo = bisect_left(d.strings, s)
        if lo < len(d.strings) and d.strings[lo] == s:
            rank.append(float(lo))
    return sorted(set(rank))


def _filter_terms(f, d):
    field, op, V = f.Field, f.Operator, f.Value
    non_numeric_rows = [Pred(field, "num", ABSENT, ())] if d.numeric else []        # (nothing to exclude on an all-string field)
    if op in _NUM_OP:
        fv = _as_float(V)
        terms = []
        if fv is None:
            sp = _str_preds(field, d, op, _go_str(V))
            return [sp] if sp is not None and (d.numeric or d.other) else []
        if d.numeric:
            terms.append([Pred(field, "num", _NUM_OP[op], (fv,))])
        if d.other:
            sp = _str_preds(field, d, op, _go_str(V))
            if sp is not None:
                terms.append(non_numeric_rows + sp)
        return terms
    if op not in (core.In, core.NotIn):
        return []                                                                   # matchesFilter: an unknown operator matches nothing
    is_list = isinstance(V, (list, tuple))
    if not is_list:
        return [[Pred(field, "str", PRESENT, ())]] if op == core.NotIn and (d.numeric or d.other) else []
    nums, seen = [], set()
    for v in V:
        fv = _as_float(v)
        if fv is not None and not (fv in seen):
            seen.add(fv); nums.append(fv)
    codes_other = _codes(d, {_go_str(v) for v in V if _as_float(v) is None})     # literals that meet numeric rows by string
    codes_all = _codes(d, {_go_str(v) for v in V})
    terms = []
    if op == core.In:
        if d.numeric:
            terms += [[Pred(field, "num", IN, c)] for c in _chunks(nums)]
            numeric_rows = [Pred(field, "num", PRESENT, ())] if d.other else []
            terms += [numeric_rows + [Pred(field, "str", IN, c)] for c in _chunks(codes_other)]
        if d.other:
            terms += [non_numeric_rows + [Pred(field, "str", IN, c)] for c in _chunks(codes_all)]
        return terms
    if d.numeric:
        preds = [Pred(field, "num", NOT_IN, c) for c in _chunks(nums)]
        if not nums and d.other:
            preds.append(Pred(field, "num", PRESENT, ()))
        preds += [Pred(field, "str", NOT_IN, c) for c in _chunks(codes_other)]
        terms.append(preds or [Pred(field, "str", PRESENT, ())])
    if d.other:
        preds = [Pred(field, "str", NOT_IN, c) for c in _chunks(codes_all)]
        terms.append(non_numeric_rows + (preds or [Pred(field, "str", PRESENT, ())]))
    return terms


def plan(filters, dictionaries):
    """filters (core.Filter, ANDed as Collection.Search does) -> one entry per filter: a list of terms (ORed), each a list of Pred
    (ANDed).  A filter with no term matches no row.  Pure: reads the dictionaries only."""
    out = []
    for f in filters:
        if f.Field not in dictionaries:
            raise NotServable("no column holds field %r" % (f.Field,))
        out.append(_filter_terms(f, dictionaries[f.Field]))
    return out


def fused_predicates(pl):
    """the predicates of a plan that ONE qv_index_search_where conjunction expresses — every filter a single term, 1 to 8 predicates in
    all — or None: the plan needs set algebra (a mixed-type field), more passes, matches no row, or holds no filter (FacetColumns.rowset
    then answers for the snapshot's rows only).  Pure: reads the plan."""
    if not pl or any(len(terms) != 1 for terms in pl):
        return None
    preds = [p for terms in pl for p in terms[0]]
    return preds if 1 <= len(preds) <= MAX_PREDS else None


def _eval_pred(p, arrays):
    vals, pres = arrays[p.field][p.kind]
    if p.op == PRESENT:
        return pres.copy()
    if p.op == ABSENT:
        return ~pres
    if p.kind == "num":
        def eq(v):
            return np.abs(vals - np.float64(v)) <= 1e-9
        lit = [np.float64(v) for v in p.literals]
    else:
        def eq(v):
            return vals == np.uint32(v)
        lit = [np.uint32(v) for v in p.literals]
    with np.errstate(invalid="ignore"):
        if p.op in (IN, NOT_IN):
            hit = np.zeros(vals.shape, dtype=bool)
            for v in lit:
                hit |= eq(v)
            b = hit if p.op == IN else ~hit
        elif p.op == EQ:
            b = eq(lit[0])
        elif p.op == NE:
            b = ~eq(lit[0])
        elif p.op == LT:
            b = vals < lit[0]
        elif p.op == LE:
            b = vals <= lit[0]
        elif p.op == GT:
            b = vals > lit[0]
        else:
            b = vals >= lit[0]
    return pres & b


def evaluate_host(pl, arrays, rows=None):
    """the bool mask the kernels produce for a plan over the same arrays (every predicate: present AND comparison; ABSENT: not present)"""
    if rows is None:
        rows = len(next(iter(arrays.values()))["str"][1]) if arrays else 0
    out = np.ones(rows, dtype=bool)
    for terms in pl:
        any_term = np.zeros(rows, dtype=bool)
        for preds in terms:
            m = np.ones(rows, dtype=bool)
            for p in preds:
                m &= _eval_pred(p, arrays)
            any_term |= m
        out &= any_term
    return out


class FacetColumns:
    """The fields of a metadata snapshot as columns on a DeviceIndex's device: row i of the index carries metadata_per_row[i].
    rowset(filters) is the set of rows for which core.matchesFilter holds for every filter, made on the device."""

    def __init__(self, index, metadata_per_row, fields):
        if len(metadata_per_row) > index.rows():
            raise ValueError("more metadata rows (%d) than index rows (%d)" % (len(metadata_per_row), index.rows()))
        self.index = index
        self.rows = len(metadata_per_row)
        arrays, self.dictionaries = build_arrays(metadata_per_row, fields)
        self.columns = {}
        for f in fields:
            cols = {"num": index.column("f64"), "str": index.column("u32")}
            for kind, col in cols.items():
                vals, pres = arrays[f][kind]
                if self.rows:
                    col.set(0, vals, pres)
            self.columns[f] = cols

    def close(self):
        for cols in self.columns.values():
            for col in cols.values():
                col.close()
        self.columns = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _conjunction(self, preds):
        """one pass per 8 predicates, ANDed"""
        out = None
        for i in range(0, len(preds), MAX_PREDS):
            s = self.index.rowset_where([(self.columns[p.field][p.kind], p.op, p.literals or None) for p in preds[i:i + MAX_PREDS]])
            if out is None:
                out = s
            else:
                out.combine(out, s, "and"); s.close()
        return out

    def rowset(self, filters):
        pl = plan(filters, self.dictionaries)
        if not pl:                                                                   # no filter: every row of the snapshot
            mask = np.zeros(self.index.rows(), dtype=bool); mask[:self.rows] = True
            return self.index.rowset(mask)
        if any(not terms for terms in pl):
            return self.index.rowset(None)                                           # some filter matches no row
        single = [p for terms in pl if len(terms) == 1 for p in terms[0]]           # one pass for all of these
        out = self._conjunction(single) if single else None
        for terms in pl:
            if len(terms) == 1:
                continue
            any_term = self._conjunction(terms[0])
            for preds in terms[1:]:
                s = self._conjunction(preds)
                any_term.combine(any_term, s, "or"); s.close()
            if out is None:
                out = any_term
            else:
                out.combine(out, any_term, "and"); any_term.close()
        return out

    def search(self, queries, k, filters):
        """DeviceIndex.search_rowsets over rowset(filters) for every query, without making the set where one conjunction expresses the
        filters (fused_predicates): then the predicates are evaluated inside the search call (DeviceIndex.search_where).  Otherwise the
        set is made, searched and closed.  -> (rows, dist, count)"""
        preds = fused_predicates(plan(filters, self.dictionaries))
        if preds is not None:
            return self.index.search_where(queries, k, [(self.columns[p.field][p.kind], p.op, p.literals or None) for p in preds])
        s = self.rowset(filters)
        try:
            return self.index.search_rowsets(queries, k, s)
        finally:
            s.close()
