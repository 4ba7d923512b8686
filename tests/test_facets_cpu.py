"""facets.plan + facets.evaluate_host (the numpy statement of the column kernels) against core.matchesFilter, row by row, without a device:
every operator of core.py:42-46 over ints, floats, floats equal to ints, bools, strings that look like numbers, None, missing fields
and fields of mixed type.  The two must agree on EVERY row; plan may refuse (facets.NotServable) only what its docstring lists."""
import random

import numpy as np
import pytest

from quiver_amd import core, facets
from quiver_amd.core import Filter

OPS = (core.Equals, core.NotEquals, core.GreaterThan, core.GreaterThanOrEqual, core.LessThan, core.LessThanOrEqual, core.In, core.NotIn)
ROWS = 3000

NUMS = [0, 1, 5, 5.0, 5.000000001, 5.0000000005, 4.999999999, -3, 2.5, 10, 100, 1e6, 1e6 + 1e-9, 7, 7.25, -0.5]
STRS = ["5", "5.0", "10", "100", "abc", "abd", "", "true", "false", "<nil>", "2.5", "zeta", "Alpha", "7", "-3"]
OTHERS = [True, False, None]


def _value(rng, kind):
    if kind == "num":
        return rng.choice(NUMS)
    if kind == "str":
        return rng.choice(STRS)
    if kind == "other":
        return rng.choice(OTHERS)
    return _value(rng, rng.choice(("num", "str", "other")))


# field -> the kinds its rows draw from: three homogeneous fields, one mixed, one that no row has
FIELDS = {"price": "num", "tag": "str", "flag": "other", "mixed": "any", "ghost": None}


@pytest.fixture(scope="module")
def corpus():
    rng = random.Random(20260518)
    rows = []
    for _ in range(ROWS):
        md = {}
        for f, kind in FIELDS.items():
            if kind is not None and rng.random() < 0.8:
                md[f] = _value(rng, kind)
        rows.append(md if rng.random() < 0.97 else None)               # a row without metadata has no field
    arrays, dictionaries = facets.build_arrays(rows, list(FIELDS))
    return rows, arrays, dictionaries


def _filters():
    rng = random.Random(7)
    out = []
    literals = NUMS + STRS + OTHERS + [6, "nope", 1e15, "a", "zzzz", -1e9]
    for f in FIELDS:
        for op in OPS[:6]:
            for v in literals:
                out.append(Filter(f, op, v))
        for op in (core.In, core.NotIn):
            out.append(Filter(f, op, []))
            out.append(Filter(f, op, 5))                               # a non-list value: In matches nothing, NotIn every row that has the field
            out.append(Filter(f, op, "abc"))
            for n in (1, 2, 5, 12):
                for _ in range(4):
                    out.append(Filter(f, op, [rng.choice(literals) for _ in range(n)]))
            out.append(Filter(f, op, [5, "5", 5.0, "abc", True, None]))
            out.append(Filter(f, op, tuple(float(i) for i in range(300))))                    # more than one kernel list of 256
            out.append(Filter(f, op, [str(i) for i in range(300)] + STRS))
        out.append(Filter(f, "~", 5))                                  # an unknown operator matches nothing
    return out


def _want(rows, flt):
    return np.array([md is not None and all(core.matchesFilter(md, f) for f in flt) for md in rows], dtype=bool)


def test_every_operator_agrees_with_matchesFilter_on_every_row(corpus):
    rows, arrays, dictionaries = corpus
    refused = 0
    for f in _filters():
        try:
            pl = facets.plan([f], dictionaries)
        except facets.NotServable:
            refused += 1
            continue
        got = facets.evaluate_host(pl, arrays, ROWS)
        want = _want(rows, [f])
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (f, bad[:5], [rows[i] for i in bad[:5]])
    assert refused == 0                                                # every field here has its columns: nothing may be refused


def test_conjunctions(corpus):
    rows, arrays, dictionaries = corpus
    rng = random.Random(11)
    one = _filters()
    for _ in range(300):
        flt = [rng.choice(one) for _ in range(rng.randint(2, 4))]
        got = facets.evaluate_host(facets.plan(flt, dictionaries), arrays, ROWS)
        assert np.array_equal(got, _want(rows, flt)), flt
    assert facets.evaluate_host(facets.plan([], dictionaries), arrays, ROWS).all()


def test_homogeneous_fields_take_one_term_and_no_or(corpus):
    """a field whose rows are all numbers, or all non-numbers, is ONE conjunction per filter (one kernel pass, no combine)"""
    _, _, dictionaries = corpus
    assert dictionaries["price"].numeric and not dictionaries["price"].other
    assert dictionaries["tag"].other and not dictionaries["tag"].numeric
    assert dictionaries["mixed"].numeric and dictionaries["mixed"].other
    for f in ("price", "tag", "flag"):
        for op in OPS[:6]:
            for v in (5, 2.5, "5", "abc", True, None):
                terms = facets.plan([Filter(f, op, v)], dictionaries)[0]
                assert len(terms) <= 1, (f, op, v, terms)
                assert all(len(t) == 1 for t in terms), (f, op, v, terms)
        for op in (core.In, core.NotIn):
            terms = facets.plan([Filter(f, op, [5, "abc", 7.25, "5"])], dictionaries)[0]
            if op == core.NotIn or f != "price":
                assert len(terms) <= 1, (f, op, terms)
    # the mixed field needs the OR: a numeric literal meets numeric rows by value and the others by string
    assert len(facets.plan([Filter("mixed", core.Equals, 5)], dictionaries)[0]) == 2


def test_the_only_refusal_is_a_field_without_columns(corpus):
    _, _, dictionaries = corpus
    with pytest.raises(facets.NotServable):
        facets.plan([Filter("colour", core.Equals, "red")], dictionaries)
    assert "is not among the snapshot's" in facets.__doc__


def test_predicates_fit_the_kernel_limits(corpus):
    _, _, dictionaries = corpus
    for f in _filters():
        for preds in facets.plan([f], dictionaries)[0]:
            assert preds
            for p in preds:
                n = len(p.literals)
                if p.op in (facets.IN, facets.NOT_IN):
                    assert 1 <= n <= 256
                elif p.op in (facets.PRESENT, facets.ABSENT):
                    assert n == 0
                else:
                    assert n == 1
                if p.kind == "str":
                    assert all(float(v).is_integer() and 0 <= v < 2 ** 32 for v in p.literals)
