"""Filtered search by predicate in one call (qv_index_search_where / _device, k_where_mq in quiver_amd/csrc/qv_where.hip).

The contract is an equivalence: query q gets exactly what DeviceIndex.search_rowsets returns when sets[q] is the set rowset_where makes
from filters[q] — rows, float32 bits, counts, padding.  Every comparison here is against that pair of calls, and against
tests/_oracle.exact_search over alive & (numpy's statement of the predicates) as a second witness.

Every test in this file needs the new entry points: none passes without them."""
import threading

import numpy as np
import pytest

import quiver_amd
from quiver_amd import QvError
from quiver_amd.device_index import WHERE_DEVICE_LITERALS, WHERE_FILTERS_PER_LAUNCH
from tests import _oracle as O

pytestmark = pytest.mark.gpu

INVALID_ARG, K_NOT_POSITIVE, UNSUPPORTED = -1, -3, -8
OPS = ("eq", "ne", "lt", "le", "gt", "ge", "in", "not_in", "present", "absent")
N, SHORT = 2051, 1500                                                   # 33 tiles: a ragged last one, no multiple of the kernel's 4 tiles per wave
NQS = (1, 2, 4, 5, 8, 9, 16, 17)
KS = (1, 10, 64, 65, 200)
FEW = 5                                                                 # live rows the "fewer than k" filter selects (k = 10 .. 200)


def _np_pred(vals, pres, op, lits):
    """numpy's statement of one predicate; vals float64 or uint32 (as tests/test_gpu_rowset_where.py states it)"""
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


def _columns(idx, n, rng, n_u=None):
    """an F64 and a U32 column as tests/test_gpu_rowset_where.py makes them (presence about half, tile 2 all absent, tile 3 all present,
    F64 values on and around a grid of 20); the U32 column reaches only row n_u"""
    n_u = n if n_u is None else n_u
    pres = rng.random(n) < 0.5
    pres[128:192] = False
    pres[192:256] = True
    f = rng.integers(0, 20, n).astype(np.float64) + rng.choice(np.array([0.0, 5e-10, -5e-10, 2e-9, -2e-9, 0.25]), n)
    u = rng.integers(0, 300, n).astype(np.uint32)
    pu = rng.random(n) < 0.5
    pu[128:192] = False
    pu[192:256] = True
    pu[n_u:] = False                                                   # (numpy's view of "no value past the column's extent")
    cf, cu = idx.column("f64"), idx.column("u32")
    return (cf, f, pres), (cu, u, pu)


class Corpus:
    """index + columns + the filter family, with numpy's mask and the reference set (rowset_where) of every filter"""

    def __init__(self, metric, dim):
        self.metric, self.dim, self.mid = metric, dim, quiver_amd.metric_id(metric)
        self.rows = O.gen_rows(9100 + dim, 0, N, dim)
        self.idx = idx = quiver_amd.DeviceIndex(dim, metric)
        idx.add(self.rows)
        rng = np.random.default_rng(91)
        dead = np.flatnonzero(rng.random(N) < 0.05).astype(np.uint32)
        self.live = np.ones(N, bool); self.live[dead] = False
        (cf, f, pf), (cu, u, pu) = _columns(idx, N, rng, SHORT)
        # planted values: 1000.0 in FEW live rows (one of them in the ragged last tile), 2000.0 in tombstoned rows only
        live_rows = np.flatnonzero(self.live)
        few = np.concatenate([rng.choice(live_rows[live_rows < 2048 - 64], FEW - 1, replace=False), live_rows[-1:]])
        f[few] = 1000.0; pf[few] = True
        f[dead[:7]] = 2000.0; pf[dead[:7]] = True
        cf.set(0, f, pf)
        cu.set(0, u[:SHORT], pu[:SHORT])
        idx.remove(dead)
        self.cf, self.cu = cf, cu

        def mask(preds):
            return np.logical_and.reduce([np.ones(N, bool)] + [_np_pred(f if c is cf else u, pf if c is cf else pu, op, lit) for c, op, lit in preds])
        self._mask = mask
        lit_f = {"in": [3.0, 7.0 + 5e-10, 11.0, 250.5], "not_in": [3.0, 7.0 + 5e-10, 11.0, 250.5], "present": None, "absent": None}
        lit_u = {"in": [0, 17, 299, 4000], "not_in": [0, 17, 299, 4000], "present": None, "absent": None}
        fam = [[(cf, op, lit_f.get(op, 9.0))] for op in OPS] + [[(cu, op, lit_u.get(op, 150))] for op in OPS]
        fam += [[(cf, "ge", 3.0), (cu, "lt", 100)], [(cu, "ne", 7), (cf, "lt", 15.0), (cf, "present", None)]]
        fam += [[(cu, "in", list(range(0, 512, 2)))], None, [(cf, "lt", 6.5)], [(cf, "lt", 6.5)]]      # 256 literals; no predicate; two bytewise-equal ones
        self.special = {"zero": [(cf, "eq", 2000.0)], "few": [(cf, "eq", 1000.0)], "many": [(cf, "ge", 0.0)]}
        self.family = fam
        self.masks = {id(p): (np.ones(N, bool) if p is None else mask(p)) for p in fam + list(self.special.values())}
        self.sets = {id(p): (None if p is None else idx.rowset_where(p)) for p in fam + list(self.special.values())}
        assert int((self.masks[id(self.special["zero"])] & self.live).sum()) == 0 and int(self.masks[id(self.special["zero"])].sum()) == 7
        assert int((self.masks[id(self.special["few"])] & self.live).sum()) == FEW

    def add(self, preds):
        """a further filter: numpy's mask and the reference set"""
        self.masks[id(preds)] = self._mask(preds)
        self.sets[id(preds)] = self.idx.rowset_where(preds)
        return preds

    def check(self, qs, k, filters, got, where):
        """got == search_rowsets over the reference sets, bit for bit, and == the oracle"""
        r, d, c = got
        rr, rd, rc = self.idx.search_rowsets(qs, k, [self.sets[id(p)] for p in filters])
        assert np.array_equal(c, rc), (where, c, rc)
        assert np.array_equal(r, rr), where
        assert np.array_equal(d.view(np.uint32), rd.view(np.uint32)), where
        for i, p in enumerate(filters):
            ro, do = O.exact_search(self.mid, self.rows, qs[i], k, alive=(self.live & self.masks[id(p)]).astype(np.uint8))
            w = ro.size
            assert int(c[i]) == w == min(k, int((self.live & self.masks[id(p)]).sum())), (where, i)
            assert r[i, :w].tolist() == ro.tolist() and d[i, :w].tobytes() == do.tobytes(), (where, i)
            assert (r[i, w:] == 0xFFFFFFFF).all() and np.isposinf(d[i, w:]).all(), (where, i)


@pytest.mark.parametrize("metric", ["cosine", "l2", "l2sq"])
@pytest.mark.parametrize("dim", [32, 128])
def test_equals_search_rowsets_and_the_oracle(metric, dim):
    """every nq x k: the queries of a call carry different filters — from 3 queries on always one that selects no live row (its 7 rows
    are tombstoned), one that selects FEW < k and one that selects at least k (k = 1 has no "1 to k - 1": asserted from k = 10 on); calls of
    1 and 2 queries are made three times so that each of the three leads once.  The rest rotates through the family: every op on both
    column types (the U32 column ends at row 1 500), conjunctions of 2 and 3, a 256-literal IN, no predicate, two bytewise-equal ones."""
    cp = Corpus(metric, dim)
    fam, sp = cp.family, cp.special
    used, off = set(), 0
    for k in KS:
        live_counts = {name: int((cp.live & cp.masks[id(p)]).sum()) for name, p in sp.items()}
        assert live_counts["zero"] == 0 and live_counts["many"] >= k
        assert k == 1 or 1 <= live_counts["few"] <= k - 1
        lead = [sp["zero"], sp["few"], sp["many"]]
        for nq in NQS:
            qs = O.gen_rows(9200 + nq + k, 0, nq, dim)
            for rot in range(3 if nq < 3 else 1):
                filters = (lead[rot:] + lead[:rot])[:nq]
                while len(filters) < nq:
                    filters.append(fam[off % len(fam)]); used.add(off % len(fam)); off += 1
                cp.check(qs, k, filters, cp.idx.search_where(qs, k, filters), (metric, dim, nq, k, rot))
    assert used == set(range(len(fam)))
    # one list for all queries, and None
    qs = O.gen_rows(9300, 0, 3, dim)
    cp.check(qs, 10, [fam[20]] * 3, cp.idx.search_where(qs, 10, fam[20]), "broadcast")
    cp.check(qs, 10, [None] * 3, cp.idx.search_where(qs, 10, None), "none")


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_bound_scan_routes(metric):
    n, dim, k = 20011, 128, 10
    rng = np.random.default_rng(50)
    idx = quiver_amd.DeviceIndex(dim, metric)
    idx.add(rng.standard_normal((n, dim)).astype(np.float32))
    vals = rng.integers(0, 10, n).astype(np.uint32)
    col = idx.column("u32")
    col.set(0, vals)
    specs = [[(col, "lt", 5)], [(col, "eq", 3)], [(col, "ge", 2)], [(col, "in", [1, 9])], [(col, "ne", 0)], None, [(col, "gt", 7)], [(col, "le", 8)]]
    qs = rng.standard_normal((8, dim)).astype(np.float32)
    for nq in (1, 4, 8):
        idx.set_bound_scan("never")
        exact = idx.search_where(qs[:nq], k, specs[:nq])
        idx.set_bound_scan("always")
        before = idx.bound_scan_stats()["searches"]
        got = idx.search_where(qs[:nq], k, specs[:nq])
        assert idx.bound_scan_stats()["searches"] > before, (metric, nq)            # the path was taken
        for a, b in zip(got, exact):
            assert a.tobytes() == b.tobytes(), (metric, nq)
        idx.set_bound_scan("auto")
        before = idx.bound_scan_stats()["searches"]
        auto = idx.search_where(qs[:nq], k, specs[:nq])
        if nq > 1:
            assert idx.bound_scan_stats()["searches"] == before, (metric, nq)       # a pass holding a transient set is declined
        for a, b in zip(auto, exact):
            assert a.tobytes() == b.tobytes(), (metric, nq)


def test_grid_stride():
    """more tiles than one sweep of the grid covers (as test_grid_stride of tests/test_gpu_rowset_where.py), two filters in one launch:
    both word arrays are read by a k = 64 search, compared with the search over the sets rowset_where makes"""
    from quiver_amd.device_index import device_info
    n = device_info(0)["cus"] * 8 * 4 * 8 * 64 + 100_003
    idx = quiver_amd.DeviceIndex(4, "l2sq")
    idx.add_synthetic(3, 0, n)
    rng = np.random.default_rng(3)
    vals = rng.integers(0, 100_000, n).astype(np.uint32)
    pres = rng.random(n) < 0.7
    col = idx.column("u32")
    col.set(0, vals, pres)
    # selective filters: ~40 rows each, spread over the whole index — the 64 results are ALL their live rows, so every word matters
    filters = [[(col, "lt", 1)], [(col, "eq", 99_999)]]
    sets = [idx.rowset_where(p) for p in filters]
    qs = np.random.default_rng(4).standard_normal((2, 4)).astype(np.float32)
    r, d, c = idx.search_where(qs, 64, filters)
    rr, rd, rc = idx.search_rowsets(qs, 64, sets)
    want = [np.flatnonzero(pres & (vals < 1)), np.flatnonzero(pres & (vals == 99_999))]
    for i in range(2):
        assert 0 < want[i].size < 64 and want[i].max() > n - n // 2                 # rows beyond the grid's first sweep among them
        assert int(c[i]) == want[i].size and sorted(r[i, :want[i].size].tolist()) == want[i].tolist()
    assert np.array_equal(c, rc) and np.array_equal(r, rr) and d.tobytes() == rd.tobytes()
    one = idx.search_where(qs[:1], 64, filters[:1])                                 # the single-query piece: alive & where in one kernel
    assert np.array_equal(one[0][0], r[0]) and one[1][0].tobytes() == d[0].tobytes()


@pytest.mark.parametrize("nq", [WHERE_FILTERS_PER_LAUNCH, WHERE_FILTERS_PER_LAUNCH + 1, 3 * WHERE_FILTERS_PER_LAUNCH + 2])
def test_launch_chunking(nq):
    """as many distinct filters as one evaluation launch carries, and one more"""
    cp = Corpus("l2", 32)
    filters = [cp.add([(cp.cf, "lt", 1.0 + 0.7 * i)]) for i in range(nq)]
    assert len({cp.masks[id(p)].tobytes() for p in filters}) > nq // 2
    qs = O.gen_rows(9400, 0, nq, 32)
    cp.check(qs, 10, filters, cp.idx.search_where(qs, 10, filters), nq)


@pytest.mark.parametrize("nq,k", [(1, 10), (5, 64), (11, 10)])
def test_device_form_on_a_busy_stream(nq, k):
    """enqueued behind a large copy on the caller's stream, compared after that stream's own copies back; the filter arrays are gone as
    soon as the call returns"""
    import torch
    cp = Corpus("cosine", 128)
    fam = [p for p in cp.family if p is None or sum(np.size(l) for _, _, l in p if l is not None) <= WHERE_DEVICE_LITERALS]
    filters = [cp.special["few"], cp.special["zero"]][:nq] + fam[3:3 + max(nq - 2, 0)]
    filters = filters[:nq]
    qs = O.gen_rows(9500 + nq, 0, nq, 128)
    hr, hd, hc = cp.idx.search_where(qs, k, filters)
    st = torch.cuda.Stream()
    big = torch.empty(64 << 20, dtype=torch.uint8).pin_memory()
    with torch.cuda.stream(st):
        dbig = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
        dq = torch.from_numpy(qs).cuda(non_blocking=True)
        dr = torch.zeros((nq, k), dtype=torch.int32, device="cuda"); dd = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        for _ in range(4):
            dbig.copy_(big, non_blocking=True)                                      # keeps the stream busy while the search is enqueued
        arg = [None if p is None else [(c, op, None if l is None else list(np.atleast_1d(l))) for c, op, l in p] for p in filters]
        cp.idx.search_where_device(dq.data_ptr(), nq, k, arg, dr.data_ptr(), dd.data_ptr(), st.cuda_stream)
        del arg
        r = dr.cpu().numpy().view(np.uint32); d = dd.cpu().numpy()                  # (stream-ordered copies: the only wait is for them)
    assert np.array_equal(r, hr) and d.tobytes() == hd.tobytes()
    for i in range(nq):
        assert int((r[i] != 0xFFFFFFFF).sum()) == int(hc[i])
    cp.check(qs, k, filters, (r, d, hc), ("device", nq, k))


def test_device_form_unsupported_enqueues_nothing():
    import torch
    cp = Corpus("l2", 32)
    qs = O.gen_rows(9600, 0, 2, 32)
    dq = torch.from_numpy(qs).cuda()
    for k, filters in ((65, [cp.special["many"], None]),
                       (10, [cp.special["many"], [(cp.cu, "in", list(range(WHERE_DEVICE_LITERALS + 1)))]])):
        dr = torch.full((2, k), 12345, dtype=torch.int32, device="cuda"); dd = torch.full((2, k), -7.0, dtype=torch.float32, device="cuda")
        with pytest.raises(QvError) as e:
            cp.idx.search_where_device(dq.data_ptr(), 2, k, filters, dr.data_ptr(), dd.data_ptr(), 0)
        assert e.value.code == UNSUPPORTED
        torch.cuda.synchronize()
        assert (dr == 12345).all().item() and (dd == -7.0).all().item()             # the sentinel: nothing ran
    # exactly the limit is taken, and an invalid filter is INVALID_ARG before anything else is looked at
    ok = [[(cp.cu, "in", list(range(WHERE_DEVICE_LITERALS)))], None]
    dr = torch.zeros((2, 10), dtype=torch.int32, device="cuda"); dd = torch.zeros((2, 10), dtype=torch.float32, device="cuda")
    cp.idx.search_where_device(dq.data_ptr(), 2, 10, ok, dr.data_ptr(), dd.data_ptr(), 0)
    torch.cuda.synchronize()
    hr, hd, _ = cp.idx.search_where(qs, 10, ok)
    assert np.array_equal(dr.cpu().numpy().view(np.uint32), hr) and dd.cpu().numpy().tobytes() == hd.tobytes()
    with pytest.raises(QvError) as e:
        cp.idx.search_where_device(dq.data_ptr(), 2, 10, [None, [(cp.cu, "eq", 1.5)]], dr.data_ptr(), dd.data_ptr(), 0)
    assert e.value.code == INVALID_ARG and "query 1" in str(e.value)


def test_argument_checks_are_rowset_wheres():
    """each bad argument of test_predicate_count_and_argument_checks (tests/test_gpu_rowset_where.py) through the new call: the code
    rowset_where yields, the message naming the query; and the check order on an empty index and with k = 0"""
    cp = Corpus("l2", 32)
    idx, cf, cu = cp.idx, cp.cf, cp.cu
    qs = O.gen_rows(9700, 0, 2, 32)
    nine = [(cf, "ge", 2.0), (cu, "lt", 280), (cf, "lt", 18.0), (cu, "ge", 5), (cf, "ne", 9.0), (cu, "ne", 100),
            (cf, "not_in", [4.0, 5.0]), (cu, "present", None), (cf, "present", None)]
    other = quiver_amd.DeviceIndex(32, "l2")
    other.add(O.gen_rows(9701, 0, 100, 32))
    foreign = other.column("f64")
    bads = [nine, [(cf, 10, 1.0)], [(cf, -1, 1.0)], [(cf, "eq", [1.0, 2.0])], [(cf, "eq", None)], [(cf, "present", 1.0)],
            [(cu, "eq", 1.5)], [(cu, "eq", -1.0)], [(cu, "in", [1.0, 2.0 ** 32])], [(cu, "lt", float("nan"))],
            [(cf, "in", np.arange(257, dtype=np.float64))], [(cf, "in", [])], [(foreign, "ge", 0.0)]]
    for bad in bads:
        with pytest.raises(QvError) as e0:
            idx.rowset_where(bad)
        for k in (10, 200):
            with pytest.raises(QvError) as e:
                idx.search_where(qs, k, [cp.special["many"], bad])
            assert e.value.code == e0.value.code == INVALID_ARG, bad
            assert str(e.value).endswith(str(e0.value)) and "query 1" in str(e.value), (str(e.value), str(e0.value))
    # eight predicates are taken; none at all is every row (rowset_where refuses that one: a set of every row needs no evaluation)
    r, d, c = idx.search_where(qs[:1], 10, [nine[:8]])
    rs = idx.rowset_where(nine[:8])
    rr, rd, rc = idx.search_rowsets(qs[:1], 10, rs)
    assert np.array_equal(r, rr) and d.tobytes() == rd.tobytes() and np.array_equal(c, rc)
    # the order: k == 0 in front of the filters' checks; an empty index in front of both
    with pytest.raises(QvError) as e:
        idx.search_where(qs, 0, [bads[1], bads[1]])
    assert e.value.code == K_NOT_POSITIVE
    empty = quiver_amd.DeviceIndex(32, "l2")
    col = empty.column("f64")
    for k in (0, 10):
        r, d, c = empty.search_where(qs, k, [[(col, 10, 1.0)], [(foreign, "ge", 0.0)]])
        assert c.tolist() == [0, 0]


def test_concurrent_callers_share_passes():
    """8 threads x 40 single-query calls in a closed loop, every thread with a literal of its own: each result is the solo one, passes were
    shared; then where-callers and set-callers side by side through the one front"""
    n, dim, k, threads, calls = 300_000, 768, 10, 8, 40
    idx = quiver_amd.DeviceIndex(dim, "cosine")
    idx.add_synthetic(20260424, 0, n)
    idx.remove(np.arange(7, n, 101, dtype=np.uint32))
    rng = np.random.default_rng(78)
    col = idx.column("f64")
    col.set(0, rng.random(n) * 100.0)
    qs = O.gen_rows(20260427, 0, threads, dim)
    filt = [[(col, "lt", 3.0 + 11.5 * t)] for t in range(threads)]
    solo = [idx.search_where(qs[t:t + 1], k, [filt[t]]) for t in range(threads)]
    sets = [idx.rowset_where(f) for f in filt]
    for t in range(threads):                                                        # (and the solo result is the set path's)
        ref = idx.search_rowsets(qs[t:t + 1], k, sets[t])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(solo[t], ref))
    for mixed in (False, True):
        st0 = idx.rowset_coalesce_stats()
        out, errs = {}, []

        def caller(t):
            try:
                for it in range(calls):
                    by_set = mixed and t % 2 == 1
                    out[(t, it)] = idx.search_rowsets(qs[t:t + 1], k, sets[t]) if by_set else idx.search_where(qs[t:t + 1], k, [filt[t]])
            except Exception as e:                                                  # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=caller, args=(t,)) for t in range(threads)]
        [x.start() for x in th]; [x.join() for x in th]
        assert not errs, errs
        for (t, it), got in out.items():
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, solo[t])), (mixed, t, it)
        st = idx.rowset_coalesce_stats()
        assert st["solo"] + st["led"] + st["rode"] - (st0["solo"] + st0["led"] + st0["rode"]) == threads * calls      # the one front counts both kinds
        assert st["groups"] - st0["groups"] > 0, (mixed, st0, st)


def test_no_leftovers():
    """after 200 calls the device memory in use is where it was after the first 5 (which grow the buffers: every shape below occurs in them)"""
    import torch
    cp = Corpus("cosine", 128)
    qs = O.gen_rows(9800, 0, 9, 128)
    shapes = [(1, 10), (4, 10), (9, 64), (2, 200), (1, 64)]

    def call(i):
        nq, k = shapes[i % len(shapes)]
        filters = [cp.family[(i + j) % len(cp.family)] for j in range(nq)]
        if i % len(shapes) == 2:
            filters[0] = cp.family[22]                                              # the 256-literal IN: staged literals
        return cp.idx.search_where(qs[:nq], k, filters)

    for i in range(5):
        call(i)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for i in range(5, 205):
        call(i)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
