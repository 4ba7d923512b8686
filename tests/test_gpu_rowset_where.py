"""Row sets made on the device: typed columns (qv_column_*), a conjunction of comparisons over them in one kernel pass
(qv_rowset_create_where, quiver_amd/csrc/qv_where.hip) and AND / OR / AND-NOT of sets (qv_rowset_combine).

The oracle is numpy over the same arrays: np.abs(x - v) <= 1e-9 in float64, <, np.isin on codes; a row without a value fails every
op but "absent".  Sets are compared as BITMAPS: RowSet.words() is what the device holds, RowSet.count() what the host mirror holds, and
both must be numpy's.  A set from rowset_where and a set from idx.rowset(mask) with the numpy mask must be interchangeable in every search."""
import numpy as np
import pytest

import quiver_amd
from quiver_amd import QvError

pytestmark = pytest.mark.gpu

INVALID_ARG, OUT_OF_RANGE = -1, -4
OPS = ("eq", "ne", "lt", "le", "gt", "ge", "in", "not_in", "present", "absent")


def _pack(mask, rows=None):
    rows = mask.size if rows is None else rows
    pad = np.zeros((rows + 63) // 64 * 64, dtype=np.uint8)
    pad[:mask.size] = mask
    return np.packbits(pad, bitorder="little").view(np.uint64)


def _np_pred(vals, pres, op, lits):
    """numpy's statement of one predicate; vals float64 or uint32"""
    if op == "present":
        return pres.copy()
    if op == "absent":
        return ~pres
    f64 = vals.dtype == np.float64
    lits = np.atleast_1d(np.asarray(lits, dtype=np.float64))

    def eq(v):
        return np.abs(vals - v) <= 1e-9 if f64 else vals == np.uint32(v)
    if op in ("in", "not_in"):
        hit = np.zeros(vals.size, bool)
        if f64:
            for v in lits:
                hit |= eq(v)
        else:
            hit = np.isin(vals, lits.astype(np.uint32))
        b = hit if op == "in" else ~hit
    else:
        v = lits[0] if f64 else np.uint32(lits[0])
        b = {"eq": lambda: eq(v), "ne": lambda: ~eq(v), "lt": lambda: vals < v, "le": lambda: vals <= v,
             "gt": lambda: vals > v, "ge": lambda: vals >= v}[op]()
    return pres & b


def _check_set(rs, mask, rows, where=""):
    """device words, host mirror and numpy agree; nothing selected past `rows`"""
    assert np.array_equal(rs.words(), _pack(mask, rows)), where
    assert rs.count() == int(mask.sum()), where


def _index(n, dim=8, metric="l2sq", seed=1):
    idx = quiver_amd.DeviceIndex(dim, metric)
    idx.add(np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32))
    return idx


def _columns(idx, n, rng):
    """an F64 and a U32 column over rows [0, n): presence about half, tile 2 all absent, tile 3 all present; F64 values sit on and
    around a grid of 20 values so that equality has matches on both sides of the tolerance"""
    pres = rng.random(n) < 0.5
    pres[128:192] = False
    pres[192:256] = True
    f = rng.integers(0, 20, n).astype(np.float64) + rng.choice(np.array([0.0, 5e-10, -5e-10, 2e-9, -2e-9, 0.25]), n)
    u = rng.integers(0, 300, n).astype(np.uint32)
    pu = rng.random(n) < 0.5
    pu[128:192] = False
    pu[192:256] = True
    cf, cu = idx.column("f64"), idx.column("u32")
    cf.set(0, f, pres)
    cu.set(0, u, pu)
    return (cf, f, pres), (cu, u, pu)


@pytest.fixture(scope="module")
def corpus():
    n, dim = 20011, 64
    rows = np.random.default_rng(5).standard_normal((n, dim)).astype(np.float32)
    idx = quiver_amd.DeviceIndex(dim, "cosine")
    idx.add(rows)
    F, U = _columns(idx, n, np.random.default_rng(6))
    return idx, n, F, U


@pytest.mark.parametrize("n", [1, 63, 64, 65, 600])
def test_ragged_ends_and_growth(n):
    idx = _index(n)
    rng = np.random.default_rng(n)
    vals = rng.integers(0, 4, n).astype(np.float64)
    col, never = idx.column("f64"), idx.column("u32")
    col.set(0, vals)
    assert col.rows() == n and never.rows() == 0
    every = idx.rowset_where([(col, "ge", 0.0)])
    _check_set(every, np.ones(n, bool), n)                             # bits past n_rows in the last word are zero
    some = idx.rowset_where([(col, "eq", 1.0)])
    _check_set(some, vals == 1.0, n)
    unset = idx.rowset_where([(never, "absent", None)])                # ~presence: the complement must stop at n_rows too
    _check_set(unset, np.ones(n, bool), n)
    _check_set(idx.rowset_where([(never, "present", None)]), np.zeros(n, bool), n)
    # the index grows: old sets read as unselected there, and so do the new rows under a column that does not reach them
    idx.add(np.random.default_rng(9).standard_normal((70, 8)).astype(np.float32))
    m = n + 70
    _check_set(every, np.ones(n, bool), m)
    r, _, c = idx.search_rowsets(np.zeros((2, 8), np.float32), 64, [every, some])
    assert int(c[0]) == min(64, n) and (r[0, :int(c[0])] < n).all()
    assert int(c[1]) == min(64, int((vals == 1.0).sum())) and (r[1, :int(c[1])] < n).all()
    again = idx.rowset_where([(col, "ge", 0.0)])
    _check_set(again, np.ones(n, bool), m)                             # rows past the column's extent have no value
    _check_set(idx.rowset_where([(col, "absent", None)]), np.arange(m) >= n, m)


@pytest.mark.parametrize("kind", ["f64", "u32"])
@pytest.mark.parametrize("op", OPS)
def test_every_op_on_several_workgroups(corpus, kind, op):
    idx, n, F, U = corpus
    col, vals, pres = F if kind == "f64" else U
    if op in ("in", "not_in"):
        lit = [3.0, 7.0 + 5e-10, 11.0, 250.5] if kind == "f64" else [0, 17, 299, 4000]
    elif op in ("present", "absent"):
        lit = None
    else:
        lit = 9.0 if kind == "f64" else 150
    want = _np_pred(vals, pres, op, lit)
    rs = idx.rowset_where([(col, op, lit)])
    _check_set(rs, want, n, (kind, op))
    assert not want[128:192].any() or op == "absent"                  # the all-absent tile: NE / NOT_IN included
    if op == "absent":
        other = idx.rowset_where([(col, "present", None)])
        assert np.array_equal(rs.words() ^ other.words(), _pack(np.ones(n, bool)))   # exact complements over [0, n_rows)
        assert rs.count() + other.count() == n


def test_grid_stride():
    """more tiles than one sweep of the grid covers: CUs x 8 workgroups x 4 waves x up to 8 tiles x 64 rows (4 194 304 rows on the
    256 CUs of an MI355X), whichever number of tiles per wave the kernel is built with"""
    from quiver_amd.device_index import device_info
    n = device_info(0)["cus"] * 8 * 4 * 8 * 64 + 100_003
    idx = quiver_amd.DeviceIndex(4, "l2sq")
    idx.add_synthetic(3, 0, n)
    rng = np.random.default_rng(3)
    vals = rng.integers(0, 1000, n).astype(np.uint32)
    pres = rng.random(n) < 0.7
    col = idx.column("u32")
    col.set(0, vals, pres)
    _check_set(idx.rowset_where([(col, "lt", 100)]), pres & (vals < 100), n)
    _check_set(idx.rowset_where([(col, "absent", None)]), ~pres, n)


def test_tolerance_edge():
    """v, v +- 1e-9, v +- 2e-9, v +- 5e-10: which side of the tolerance each falls on is whatever float64 says, never assumed"""
    idx = _index(100)
    offs = np.array([0.0, 1e-9, -1e-9, 2e-9, -2e-9, 5e-10, -5e-10])
    vs = [0.0, 0.5, 1e6, 1e15]
    vals = np.concatenate([np.float64(v) + offs for v in vs])
    col = idx.column("f64")
    col.set(3, vals)
    pres = np.zeros(100, bool); pres[3:3 + vals.size] = True
    full = np.zeros(100); full[3:3 + vals.size] = vals
    seen = set()
    for v in vs:
        eq = pres & (np.abs(full - np.float64(v)) <= 1e-9)
        seen.add(int(eq.sum()))
        _check_set(idx.rowset_where([(col, "eq", v)]), eq, 100, v)
        _check_set(idx.rowset_where([(col, "ne", v)]), pres & ~eq, 100, v)
        _check_set(idx.rowset_where([(col, "in", [v])]), eq, 100, v)
        _check_set(idx.rowset_where([(col, "not_in", [v, -77.0])]), pres & ~eq, 100, v)
    assert len(seen) > 1                                               # the magnitudes differ in what rounding leaves inside the tolerance


@pytest.mark.parametrize("kind", ["f64", "u32"])
def test_in_lists(corpus, kind):
    idx, n, F, U = corpus
    col, vals, pres = F if kind == "f64" else U
    lits = np.arange(256, dtype=np.float64) * (0.5 if kind == "f64" else 1.0)
    for lit in (lits[:1], lits):
        _check_set(idx.rowset_where([(col, "in", lit)]), _np_pred(vals, pres, "in", lit), n)
        _check_set(idx.rowset_where([(col, "not_in", lit)]), _np_pred(vals, pres, "not_in", lit), n)
    for op in ("in", "not_in"):
        with pytest.raises(QvError) as e:
            idx.rowset_where([(col, op, np.arange(257, dtype=np.float64))])
        assert e.value.code == INVALID_ARG
        with pytest.raises(QvError) as e:
            idx.rowset_where([(col, op, [])])
        assert e.value.code == INVALID_ARG


def test_predicate_count_and_argument_checks(corpus):
    idx, n, (cf, f, pf), (cu, u, pu) = corpus
    preds = [(cf, "ge", 2.0), (cu, "lt", 280), (cf, "lt", 18.0), (cu, "ge", 5), (cf, "ne", 9.0), (cu, "ne", 100),
             (cf, "not_in", [4.0, 5.0]), (cu, "present", None)]
    masks = [_np_pred(f if c is cf else u, pf if c is cf else pu, op, lit) for c, op, lit in preds]
    _check_set(idx.rowset_where(preds[:1]), masks[0], n)
    want = np.logical_and.reduce(masks)
    assert 0 < want.sum() < n
    _check_set(idx.rowset_where(preds), want, n)
    for bad in (preds + [(cf, "present", None)], []):                  # 9 predicates, none
        with pytest.raises(QvError) as e:
            idx.rowset_where(bad)
        assert e.value.code == INVALID_ARG
    for bad in ([(cf, 10, 1.0)], [(cf, -1, 1.0)], [(cf, "eq", [1.0, 2.0])], [(cf, "eq", None)], [(cf, "present", 1.0)],
                [(cu, "eq", 1.5)], [(cu, "eq", -1.0)], [(cu, "in", [1.0, 2.0 ** 32])], [(cu, "lt", float("nan"))]):
        with pytest.raises(QvError) as e:
            idx.rowset_where(bad)
        assert e.value.code == INVALID_ARG, bad
    other = _index(100)
    with pytest.raises(QvError) as e:
        other.rowset_where([(cf, "ge", 0.0)])                          # a column of another index
    assert e.value.code == INVALID_ARG
    with pytest.raises(QvError) as e:
        idx.column(2)
    assert e.value.code == INVALID_ARG


def test_early_exit():
    """the first predicate leaves a value in two tiles only; where the word is already zero the later columns must not matter"""
    n = 6000
    idx = _index(n)
    rng = np.random.default_rng(12)
    a = np.zeros(n); a[64 * 7:64 * 8] = rng.integers(0, 2, 64); a[64 * 50 + 3] = 1.0; a[n - 1] = 1.0       # tiles 7, 50 and the ragged last one
    b = rng.integers(0, 10, n).astype(np.uint32)
    pb = rng.random(n) < 0.8
    c = rng.standard_normal(n)
    ca, cb, cc = idx.column("f64"), idx.column("u32"), idx.column("f64")
    ca.set(0, a); cb.set(0, b, pb); cc.set(0, c)
    preds = [(ca, "eq", 1.0), (cb, "in", [1, 2, 3, 4, 5, 6]), (cc, "gt", -0.5)]
    want = (a == 1.0) & pb & np.isin(b, [1, 2, 3, 4, 5, 6]) & (c > -0.5)
    assert want.any()
    first = idx.rowset_where(preds)
    _check_set(first, want, n)
    # other values and presence in the tiles the first predicate empties: the same set
    keep = np.zeros(n, bool); keep[64 * 7:64 * 8] = True; keep[64 * 50:64 * 51] = True; keep[n - (n % 64):] = True
    b2 = np.where(keep, b, 3).astype(np.uint32); pb2 = np.where(keep, pb, True); c2 = np.where(keep, c, 99.0)
    cb.set(0, b2, pb2); cc.set(0, c2)
    again = idx.rowset_where(preds)
    _check_set(again, want, n)
    assert np.array_equal(first.words(), again.words())


def test_short_and_patched_columns():
    n = 500
    idx = _index(n)
    rng = np.random.default_rng(21)
    col = idx.column("u32")
    vals = np.zeros(n, np.uint32); pres = np.zeros(n, bool)
    v1, p1 = rng.integers(0, 9, 100).astype(np.uint32), rng.random(100) < 0.5
    col.set(37, v1, p1)
    vals[37:137], pres[37:137] = v1, p1
    assert col.rows() == 137
    _check_set(idx.rowset_where([(col, "present", None)]), pres, n)
    v2, p2 = rng.integers(0, 9, 300).astype(np.uint32), rng.random(300) < 0.6          # overlaps rows 90 .. 136 with other presence
    col.set(90, v2, p2)
    vals[90:390], pres[90:390] = v2, p2
    assert col.rows() == 390
    _check_set(idx.rowset_where([(col, "present", None)]), pres, n)
    _check_set(idx.rowset_where([(col, "ge", 4)]), pres & (vals >= 4), n)
    col.set(100, vals[100:101])                                        # present=None: the row has a value
    pres[100] = True
    _check_set(idx.rowset_where([(col, "present", None)]), pres, n)
    for first, m in ((n - 10, 11), (n, 1), (0, n + 1)):               # a piece reaching past the index: refused, nothing changes
        with pytest.raises(QvError) as e:
            col.set(first, np.full(m, 8, np.uint32))
        assert e.value.code == OUT_OF_RANGE
    assert col.rows() == 390
    _check_set(idx.rowset_where([(col, "present", None)]), pres, n)
    _check_set(idx.rowset_where([(col, "eq", 8)]), pres & (vals == 8), n)
    # the index grows past the column: the new rows have no value until they are set
    idx.add(np.random.default_rng(2).standard_normal((200, 8)).astype(np.float32))
    m = n + 200
    grown = np.concatenate([pres & (vals >= 4), np.zeros(200, bool)])
    _check_set(idx.rowset_where([(col, "ge", 4)]), grown, m)
    col.set(n + 50, np.full(100, 5, np.uint32))
    grown[n + 50:n + 150] = True
    _check_set(idx.rowset_where([(col, "ge", 4)]), grown, m)
    assert col.rows() == n + 150
    with col:                                                          # the context manager closes it
        pass
    assert not col.handle.value


def test_combine():
    n = 1000
    idx = _index(n)
    rng = np.random.default_rng(31)
    ma, mb = rng.random(n) < 0.4, rng.random(n) < 0.5
    fn = {"and": lambda x, y: x & y, "or": lambda x, y: x | y, "andnot": lambda x, y: x & ~y}
    for op, f in fn.items():
        a, b, dst = idx.rowset(ma), idx.rowset(mb), idx.rowset(None)
        assert dst.combine(a, b, op) is dst
        _check_set(dst, f(ma, mb), n, op)
        a.combine(a, b, op)                                            # dst aliasing a
        _check_set(a, f(ma, mb), n, op)
        a2 = idx.rowset(ma)
        b.combine(a2, b, op)                                           # dst aliasing b
        _check_set(b, f(ma, mb), n, op)
        a2.combine(a2, a2, op)                                         # all three the same set
        _check_set(a2, f(ma, ma), n, op)
    a, b = idx.rowset(ma), idx.rowset(mb)
    for got, want in ((a & b, ma & mb), (a | b, ma | mb), (a - b, ma & ~mb)):
        _check_set(got, want, n)
    _check_set(a, ma, n); _check_set(b, mb, n)                         # the conveniences allocate: their operands stay
    # a made before the index grew, b after: a reads as zeros past its end, dst is extended to the index's rows
    idx.add(np.random.default_rng(4).standard_normal((300, 8)).astype(np.float32))
    m = n + 300
    mb2 = rng.random(m) < 0.5
    b2 = idx.rowset(mb2)
    ma_ext = np.concatenate([ma, np.zeros(300, bool)])
    for op, f in fn.items():
        old = idx.rowset(None)
        old.combine(a, b2, op)
        _check_set(old, f(ma_ext, mb2), m, op)
    a.combine(b2, a, "or")                                             # dst is the short one: extended in place
    _check_set(a, ma_ext | mb2, m)
    r, _, c = idx.search_rowsets(np.zeros((2, 8), np.float32), 200, [a, b2])          # the k > 64 paths clamp by the mirror
    assert int(c[0]) == min(200, int((ma_ext | mb2).sum())) and int(c[1]) == min(200, int(mb2.sum()))
    other = _index(64)
    foreign = other.rowset(None)
    for args in ((a, b2, foreign), (a, foreign, b2), (foreign, a, b2)):
        with pytest.raises(QvError) as e:
            args[0].combine(args[1], args[2], "and")
        assert e.value.code == INVALID_ARG
    with pytest.raises(QvError) as e:
        a.combine(a, b2, 3)
    assert e.value.code == INVALID_ARG


def _same_results(idx, qs, k, sets_a, sets_b):
    ra, da, ca = idx.search_rowsets(qs, k, sets_a)
    rb, db, cb = idx.search_rowsets(qs, k, sets_b)
    assert np.array_equal(ca, cb) and np.array_equal(ra, rb) and da.tobytes() == db.tobytes()
    return ra, ca


@pytest.mark.parametrize("k", [10, 200])
def test_sets_from_where_and_from_masks_are_interchangeable(corpus, k):
    """5 queries with different sets (one shared pass at k = 10; at k = 200 the paths that clamp by the host mirror)"""
    idx, n, (cf, f, pf), (cu, u, pu) = corpus
    qs = np.random.default_rng(40 + k).standard_normal((5, 64)).astype(np.float32)
    specs = [[(cf, "lt", 6.0)], [(cu, "in", list(range(0, 300, 7)))], [(cf, "ge", 3.0), (cu, "lt", 100)], [(cu, "eq", 299)], [(cf, "absent", None)]]
    where, masked, masks = [], [], []
    for preds in specs:
        m = np.logical_and.reduce([_np_pred(f if c is cf else u, pf if c is cf else pu, op, lit) for c, op, lit in preds])
        masks.append(m)
        where.append(idx.rowset_where(preds))
        masked.append(idx.rowset(m))
        assert where[-1].count() == masked[-1].count() == int(m.sum())
    rows, cnt = _same_results(idx, qs, k, where, masked)
    for i in range(5):
        assert int(cnt[i]) == min(k, int(masks[i].sum())) and masks[i][rows[i, :int(cnt[i])]].all()
    # combined sets on both sides: (0 | 1) - 3, 2 & 0, ...
    comb_w = [(where[0] | where[1]) - where[3], where[2] & where[0], where[4] | where[3], where[1] - where[2], where[0] & where[4]]
    comb_m = [idx.rowset((masks[0] | masks[1]) & ~masks[3]), idx.rowset(masks[2] & masks[0]), idx.rowset(masks[4] | masks[3]),
              idx.rowset(masks[1] & ~masks[2]), idx.rowset(masks[0] & masks[4])]
    for w, m in zip(comb_w, comb_m):
        assert w.count() == m.count() and np.array_equal(w.words(), m.words())
    _same_results(idx, qs, k, comb_w, comb_m)


def test_bound_scan_rule_reads_the_same_counts():
    """set_bound_scan("always") on a 128-dimensional cosine index: the filtered rule reads the set's tiles and selected counts, so
    the searches counter must move alike for a set from rowset_where, its twin from a mask and a combined one, with equal results"""
    n, dim = 20011, 128
    rng = np.random.default_rng(50)
    idx = quiver_amd.DeviceIndex(dim, "cosine")
    idx.add(rng.standard_normal((n, dim)).astype(np.float32))
    idx.set_bound_scan("always")
    vals = rng.integers(0, 10, n).astype(np.uint32)
    col = idx.column("u32")
    col.set(0, vals)
    qs = rng.standard_normal((5, dim)).astype(np.float32)
    specs = [("lt", 5), ("eq", 3), ("ge", 2), ("in", [1, 9]), ("ne", 0)]
    where = [idx.rowset_where([(col, op, lit)]) for op, lit in specs]
    masks = [_np_pred(vals, np.ones(n, bool), op, lit) for op, lit in specs]
    masked = [idx.rowset(m) for m in masks]
    both_w = [w & where[0] for w in where]
    both_m = [idx.rowset(m & masks[0]) for m in masks]
    moved = []
    out = []
    for sets in (where, masked, both_w, both_m):
        before = idx.bound_scan_stats()["searches"]
        out.append(idx.search_rowsets(qs, 10, sets))
        one = idx.search_rowsets(qs[:1], 10, sets[:1])                 # and a single query
        out.append(one)
        moved.append(idx.bound_scan_stats()["searches"] - before)
    assert moved[0] == moved[1] and moved[2] == moved[3] and moved[0] > 0, moved
    for a, b in ((0, 2), (1, 3), (4, 6), (5, 7)):
        assert np.array_equal(out[a][0], out[b][0]) and out[a][1].tobytes() == out[b][1].tobytes() and np.array_equal(out[a][2], out[b][2])
