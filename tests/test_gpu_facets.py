"""facets.FacetColumns on the device: the bitmap of rowset(filters) is the bitmap of core.matchesFilter over the same metadata, and the
filtered search through it is search_masked with the host's bitmap — same rows, same float32 bits."""
import random

import numpy as np
import pytest

import quiver_amd
from quiver_amd import core, facets
from quiver_amd.core import Filter

pytestmark = pytest.mark.gpu

N, DIM = 6003, 32


def _pack(mask):
    pad = np.zeros((mask.size + 63) // 64 * 64, dtype=np.uint8)
    pad[:mask.size] = mask
    return np.packbits(pad, bitorder="little").view(np.uint64)


@pytest.fixture(scope="module")
def snapshot():
    rng = random.Random(77)
    cats = ["book", "film", "game", "5", "10", "music"]
    meta = []
    for i in range(N):
        md = {}
        if rng.random() < 0.9:
            md["price"] = rng.choice([1, 5, 5.0, 7.5, 10, 12.25, 99, 5.0000000005])
        if rng.random() < 0.9:
            md["cat"] = rng.choice(cats)
        if rng.random() < 0.85:
            md["mixed"] = rng.choice([5, "5", 10.0, "10", True, None, "film", 2.5, "abc", 7])     # numbers, their strings, a bool, a null
        meta.append(md)
    rows = np.random.default_rng(78).standard_normal((N, DIM)).astype(np.float32)
    idx = quiver_amd.DeviceIndex(DIM, "cosine")
    idx.add(rows)
    fc = facets.FacetColumns(idx, meta, ["price", "cat", "mixed"])
    return idx, meta, fc


FILTER_SETS = [
    [Filter("price", core.GreaterThanOrEqual, 5)],
    [Filter("cat", core.Equals, "film")],
    [Filter("mixed", core.Equals, 5)],                                                  # 5 and "5": numeric rows by value, the others by string
    [Filter("mixed", core.LessThan, 7)],
    [Filter("mixed", core.NotEquals, "10")],
    [Filter("mixed", core.In, [5, "film", True, 2.5])],
    [Filter("mixed", core.NotIn, [5, "film", None])],
    [Filter("price", core.LessThan, 10), Filter("cat", core.In, ["book", "game", "5"])],
    [Filter("price", core.Equals, 5), Filter("mixed", core.GreaterThan, "5")],
    [Filter("price", core.NotIn, [1, 99]), Filter("cat", core.NotEquals, "music"), Filter("mixed", core.GreaterThanOrEqual, 5)],
    [Filter("cat", core.GreaterThan, "film"), Filter("mixed", core.In, ["5", 10]), Filter("mixed", core.NotEquals, 7)],
    [Filter("cat", core.Equals, "opera")],                                              # a string no row has
    [Filter("price", core.NotIn, 3), Filter("cat", core.LessThanOrEqual, 10)],          # NotIn with a non-list; a number against strings
]


@pytest.mark.parametrize("case", range(len(FILTER_SETS)))
def test_rowset_is_matchesFilter_and_searches_alike(snapshot, case):
    idx, meta, fc = snapshot
    flt = FILTER_SETS[case]
    want = np.array([all(core.matchesFilter(md, f) for f in flt) for md in meta], dtype=bool)
    rs = fc.rowset(flt)
    assert np.array_equal(rs.words(), _pack(want)), flt
    assert rs.count() == int(want.sum())
    qs = np.random.default_rng(case).standard_normal((3, DIM)).astype(np.float32)
    for k in (10, 100):
        r, d, c = idx.search_rowsets(qs, k, rs)
        rm, dm, cm = idx.search_masked(qs, k, want)
        kk = int(cm[0])
        assert np.array_equal(c, cm)
        assert np.array_equal(r[:, :kk], rm[:, :kk]) and d[:, :kk].tobytes() == dm[:, :kk].tobytes()


def test_the_or_path_ran(snapshot):
    _, _, fc = snapshot
    d = fc.dictionaries
    assert d["mixed"].numeric and d["mixed"].other and not d["cat"].numeric and not d["price"].other
    assert len(facets.plan(FILTER_SETS[2], d)[0]) == 2
    assert all(len(t) == 1 for t in facets.plan(FILTER_SETS[7], d))                   # homogeneous fields: one pass, no OR


def test_unknown_field_is_refused(snapshot):
    _, _, fc = snapshot
    with pytest.raises(facets.NotServable):
        fc.rowset([Filter("colour", core.Equals, "red")])
