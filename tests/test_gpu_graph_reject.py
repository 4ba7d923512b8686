"""Graph traversal that rejects neighbours on the index's row-order bfloat16 copy (QV_FLAG_GRAPH_PLANE, qv_graph_set_reject_plane): rows,
float32 bits, counts and evaluation counts are those of the unchanged traversal and of the oracle's HNSW.Search on the same graph; the
counters mean what they say; the copy follows the rows; and the form stays away from everything it was not built for.  Every traversal
call carries 1024 queries: up to max(compute units, 768) the latency form runs, which never reads the copy."""
import numpy as np
import pytest

import quiver_amd
from quiver_amd.device_index import DeviceGraph, device_info, random_levels
from tests import _bound as B
from tests import _graph_reject as GR
from tests import _oracle as O

pytestmark = pytest.mark.gpu

NQ = 1024


def _knn(rows, metric, m, **kw):
    """exact m-NN lists (self excluded) through the product's flat scan, on an index that asks for the copy"""
    n = rows.shape[0]
    kw.setdefault("rowmajor", True); kw.setdefault("graph_plane", True)
    idx = quiver_amd.DeviceIndex(rows.shape[1], metric, **kw)
    idx.add(rows)
    nbr, _, _ = idx.search(rows, m + 1)
    links = np.zeros((n, m), np.uint32); deg = np.zeros(n, np.uint32)
    for i in range(n):
        l = [int(x) for x in nbr[i] if int(x) != i and int(x) < n][:m]
        deg[i] = len(l); links[i, :len(l)] = l
    return idx, deg, links


def _delta(a, b):
    return {k: (b[k] - a[k] if k != "plane" else b[k]) for k in a}


def _arms(g, qs, k, ef):
    """the same call under "never" and under "always": (results never, results always, counters of the always arm, of the never arm, redo counts)"""
    g.set_reject_plane("never")
    s0, t0 = g.reject_stats(), g.stats()["search_redo"]
    rn = g.search(qs, k, ef, with_evals=True)
    s1, t1 = g.reject_stats(), g.stats()["search_redo"]
    g.set_reject_plane("always")
    ra = g.search(qs, k, ef, with_evals=True)
    s2, t2 = g.reject_stats(), g.stats()["search_redo"]
    return rn, ra, _delta(s1, s2), _delta(s0, s1), (t1 - t0, t2 - t1)


def _same(ra, rn):
    for a, b, what in zip(ra, rn, ("rows", "distance bits", "counts", "evals")):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        bad = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(a.shape[0], -1).any(axis=1))
        assert bad.size == 0, "%s differ from the unchanged traversal for queries %s" % (what, bad[:8].tolist())


def _oracle_agrees(o, qs, res, k, which, prefixes=True):
    """prefixes=False: an under-filled query is not compared (on a graph built by Insert the reference's top-up finds rows the walk never met)"""
    r, d, c, ev = res
    assert prefixes or sum(1 for i in which if c[i] == k) >= 1
    for i in which:
        ro, do, eo = o.search(qs[i], k, with_evals=True)
        if c[i] == k:
            assert r[i].tolist() == ro.tolist(), i
            assert d[i].tobytes() == do.tobytes(), i
            assert int(ev[i]) == eo - 1, i                 # the reference also evaluates the entry point once more up front (hnsw.go:637)
        else:                                               # under-filled: the caller tops up (hnsw.go:676-710); the prefix must agree
            assert c[i] < k
            assert not prefixes or r[i, :c[i]].tolist() == ro[:c[i]].tolist(), i


@pytest.mark.parametrize("metric,dim,n,m,ef,k", [
    ("cosine", 768, 3000, 32, 128, 10),
    ("dot", 128, 2500, 16, 64, 10),
    ("cosine", 64, 2000, 32, 300, 50),       # one bfloat16 slab per row; 5 list registers per lane
    ("dot", 192, 1500, 24, 16, 5),           # an odd slab count; 2 list registers per lane
    ("cosine", 256, 1500, 8, 512, 512),      # 9 list registers per lane, k = ef
])
def test_rejecting_traversal_identical_to_the_unchanged_one_and_the_oracle(metric, dim, n, m, ef, k):
    mid = quiver_amd.metric_id(metric)
    rows = O.gen_rows(4242, 0, n, dim)
    idx, deg, links = _knn(rows, metric, m)
    g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=7)
    qs = O.gen_rows(4243, 0, NQ, dim)
    rn, ra, sa, sn, redo = _arms(g, qs, k, ef)
    _same(ra, rn)
    # every query walked level 0 in the rejecting form; the ones flagged for the exact-heap kernel (equal distances at a decision: a handful
    # of 1024 on these corpora, the same ones in both arms) finish there and count in search_redo instead
    assert sa["plane"] and sa["queries"] == NQ - redo[1] and sn["queries"] == 0 and sn["evals"] == 0
    assert sa["rejected"] <= sa["evals"] <= int(ra[3].sum())
    assert redo[0] == redo[1]
    o = O.HNSW(mid, dim, M=max(m // 2, 1), maxM0=m, efSearch=ef, maxLevel=1, seed=1)
    o.load_flat(rows, deg, links, 7)
    _oracle_agrees(o, qs, ra, k, range(0, NQ, NQ // 48)[:48])


def test_the_counters_mean_what_they_say():
    """out[0] = the evaluations made in hops that start with a full list; out[1] lies between the rows certified at TWICE the margin from the
    exact dot with the bfloat16 image (the kernel's float32 chain is within one margin of it, so each of them must go) and the rows the exact
    distance rejects: a kernel that rejects almost nothing does not pass."""
    metric, dim, n, m, ef, k = "cosine", 64, 2000, 16, 32, 10
    rows = O.gen_rows(9001, 0, n, dim)
    idx, deg, links = _knn(rows, metric, m)
    g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=3)
    qs = O.gen_rows(9002, 0, NQ, dim)
    rn, ra, sa, _, redo = _arms(g, qs, k, ef)
    _same(ra, rn)
    assert redo == (0, 0)                                                  # (for this seed no query meets a tie: the counters hold all 1024 walks)
    assert sa["queries"] == NQ
    state = B.RowState(rows)
    A = R = C2 = C1 = 0
    for i in range(NQ):
        w = GR.walk(0, rows, state, deg, links, 3, qs[i], ef, margins=2)
        assert not w["ties"], i
        assert w["evals"] == int(ra[3][i]), i                              # the restated walk IS the device's walk
        assert [e[1] for e in w["order"][:k]] == ra[0][i, :min(k, len(w["order"]))].tolist(), i
        A += w["A"]; R += w["R"]; C2 += w["C"]; C1 += w["C1"]
    print("A %d  R %d  certified at two margins %d (%.4f of R), at one %d (%.4f of R); device: evals %d rejected %d" % (
        A, R, C2, C2 / R, C1, C1 / R, sa["evals"], sa["rejected"]))
    assert C2 > 0.9 * R                                                    # (the CPU side of the claim, for this seed)
    assert sa["evals"] == A
    assert C2 <= sa["rejected"] <= R


def test_a_device_built_graph_with_upper_levels():
    """the upper levels take the unchanged path, level 0 rejects"""
    n, dim, m = 4000, 128, 16
    rows = O.gen_rows(616, 0, n, dim)
    idx = quiver_amd.DeviceIndex(dim, "cosine", rowmajor=True, graph_plane=True)
    idx.add(rows)
    g = DeviceGraph.build(idx, random_levels(n, 16, 5), m=m, max_m0=2 * m, ef_construction=100)
    info = g.info()
    assert info["cur_level"] >= 1
    qs = O.gen_rows(617, 0, NQ, dim)
    rn, ra, sa, _, redo = _arms(g, qs, 10, 64)
    _same(ra, rn)
    assert sa["queries"] == NQ - redo[1] and sa["rejected"] > 0
    lv, l0_deg, l0_links, up_off, up_links = g.export()
    o = O.HNSW(0, dim, M=m, maxM0=2 * m, efSearch=64, maxLevel=16, seed=1)
    o.load_graph(rows, lv, info["max_m0"], info["max_m"], l0_deg, l0_links, up_off, up_links, info["entry"], info["cur_level"])
    _oracle_agrees(o, qs, ra, 10, range(0, NQ, NQ // 48)[:48], prefixes=False)


def _device_form(g, qs, k, ef):
    """one call of the device-pointer form under the graph's current mode: (flagged [nq] — count 0xFFFFFFFE, the queries the exact-heap
    kernel would redo — rows, distances, counts, evals, the reject counters the call added)"""
    import torch
    nq = qs.shape[0]
    s0 = g.reject_stats()
    dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    dr = torch.empty((nq, k), dtype=torch.int32, device="cuda"); dd = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    dc = torch.empty(nq, dtype=torch.int32, device="cuda"); de = torch.empty(nq, dtype=torch.int32, device="cuda")
    g.search_device(dq.data_ptr(), nq, k, ef, dr.data_ptr(), dd.data_ptr(), dc.data_ptr(), de.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    c = dc.cpu().numpy().view(np.uint32)
    return c == 0xFFFFFFFE, dr.cpu().numpy().view(np.uint32), dd.cpu().numpy(), c, de.cpu().numpy().view(np.uint32), _delta(s0, g.reject_stats())


def test_rows_the_bound_says_nothing_about():
    n, dim, m, ef, k = 2000, 64, 16, 64, 10
    rows = O.gen_rows(5150, 0, n, dim)
    rows[:600, 0] += np.float32(3.0)                                       # a region of its own ...
    rows[1400:] = rows[:600]                                               # ... of 600 rows stored twice: their ties go to the exact-heap kernel
    special = [700, 701, 702, 703, 704]
    rows[700] = 0.0
    rows[701, 3] = np.nan
    rows[702, 5] = np.inf
    rows[703] *= np.float32(1e18)
    rows[704] *= np.float32(1e-30)
    idx, deg, links = _knn(rows, "cosine", m)
    for i in range(0, n, 7):                                               # the special rows are nobody's nearest neighbour: link them in by hand
        if deg[i]:
            links[i, deg[i] - 1] = special[(i // 7) % 5]
    for i in range(3, n, 11):                                              # ... and the doubled region, so that the queries heading there arrive
        if deg[i] > 1:
            links[i, deg[i] - 2] = i % 600
    entry = 1000                                                           # (outside the doubled region)
    g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=entry)
    qs = O.gen_rows(5151, 0, NQ, dim)
    qs[0::2, 0] -= np.float32(3.0)                                         # away from the doubled rows: walks that finish in the rejecting form
    qs[1::2, 0] += np.float32(3.0)                                         # into them: equal distances, the exact-heap kernel
    rn, ra, sa, _, redo = _arms(g, qs, k, ef)
    _same(ra, rn)
    flagged = _device_form(g, qs, k, ef)[0]                                # (under "always", as _arms leaves the graph)
    unflagged = np.flatnonzero(~flagged)
    assert sa["plane"] and flagged.sum() > 0 and unflagged.size > 0
    assert sa["queries"] == unflagged.size and redo == (int(flagged.sum()), int(flagged.sum()))
    o = O.HNSW(0, dim, M=m // 2, maxM0=m, efSearch=ef, maxLevel=1, seed=1)
    o.load_flat(rows, deg, links, entry)
    r, d, c, ev = ra
    for i in list(range(0, NQ, NQ // 24)[:24]) + unflagged[:24].tolist():
        ro, do, eo = o.search(qs[i], k, with_evals=True)
        nn = min(int(c[i]), k)
        nan = np.isnan(d[i, :nn])                           # (a NaN is a NaN: the sign the arithmetic leaves on it is not part of the contract)
        assert r[i, :nn].tolist() == ro[:nn].tolist() and np.array_equal(nan, np.isnan(do[:nn])), i
        assert d[i, :nn][~nan].tobytes() == do[:nn][~nan].tobytes(), i
        assert flagged[i] or c[i] != k or int(ev[i]) == eo - 1, i
    # walks that finished in the rejecting form met the special rows in hops that started with a full list: the bound had to speak about them
    state = B.RowState(rows)
    met = set()
    for i in unflagged[:64].tolist():
        w = GR.walk(0, rows, state, deg, links, entry, qs[i], ef)
        assert w["evals"] == int(ev[i]), i                                 # the restated walk is the device's walk
        met |= set(w["full_rows"]) & set(special)
    print("special rows met at a full list by counted walks:", sorted(met), "; flagged", int(flagged.sum()), "of", NQ)
    assert met == set(special)


def test_queries_the_bound_declines():
    n, dim, m, ef, k = 2000, 128, 16, 64, 10
    rows = O.gen_rows(31, 0, n, dim)
    idx, deg, links = _knn(rows, "dot", m)
    g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=5)
    qs = O.gen_rows(32, 0, NQ, dim)
    three = np.zeros(NQ, bool); three[[100, 500, 900]] = True
    qs[100] = 0.0
    qs[500, 7] = np.nan
    qs[900] *= np.float32(1e19)
    rn, ra, sa, _, redo = _arms(g, qs, k, ef)
    _same(ra, rn)
    # which queries the wave kernel flagged for the exact-heap kernel (they count nowhere): the device-pointer form says, query by query
    flagged, _, _, _, _, sd = _device_form(g, qs, k, ef)                   # (under "always", as _arms leaves the graph)
    assert not flagged[900]                                                # the 1e19 query walks to its end in the wave kernel — and still does not count:
    want = int((~flagged & ~three).sum())                                  # those three do not count; the rest do
    assert want >= NQ - 3 - NQ // 8
    assert sd["queries"] == want and sa["queries"] == want
    assert redo == (int(flagged.sum()), int(flagged.sum()))
    # the same call with the three swapped for ordinary queries: now every unflagged query counts
    qs2 = qs.copy(); qs2[[100, 500, 900]] = O.gen_rows(33, 0, 3, dim)
    f2, _, _, _, _, sd2 = _device_form(g, qs2, k, ef)
    assert np.array_equal(f2[~three], flagged[~three]) and sd2["queries"] == int((~f2).sum())


def test_near_duplicates_around_the_threshold():
    n, dim, m, ef, k = 3000, 128, 16, 64, 10
    rng = np.random.default_rng(77)
    centres = O.gen_rows(78, 0, 100, dim)
    rows = (centres[np.arange(n) % 100] + np.float32(1e-4) * rng.standard_normal((n, dim)).astype(np.float32)).astype(np.float32)
    idx, deg, links = _knn(rows, "cosine", m)
    for i in range(n):                                                     # a k-NN graph of clusters is disconnected: one link a node leads on
        if deg[i]:
            links[i, deg[i] - 1] = (i + 1) % n
    g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=0)
    qs = (centres[np.arange(NQ) % 100] + np.float32(1e-4) * rng.standard_normal((NQ, dim)).astype(np.float32)).astype(np.float32)
    rn, ra, sa, _, _ = _arms(g, qs, k, ef)
    _same(ra, rn)
    assert sa["queries"] > 0 and sa["rejected"] < sa["evals"]


def _image_ok(idx, rows):
    got = idx.debug_read("rowmaj16")
    want = (B.bf16(rows).view(np.uint32) >> 16).astype(np.uint16)
    assert got.shape == want.shape and np.array_equal(got, want)
    rh = (got.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    res = np.sqrt(np.sum((rows.astype(np.float64) - rh) ** 2, axis=1))
    assert np.all(res <= idx.debug_read("rres")[:rows.shape[0]].astype(np.float64))


def test_the_plane_follows_the_rows():
    import torch
    dim, m, ef, k = 128, 16, 64, 5
    rows = O.gen_rows(40, 0, 1500, dim)
    idx, deg, links = _knn(rows[:1000], "cosine", m)                       # (add)
    _image_ok(idx, rows[:1000])
    dev = torch.from_numpy(rows[1000:1020]).cuda()
    idx.add_device(dev.data_ptr(), 20); torch.cuda.synchronize()           # (within the 16 tiles the first add allocated)
    _image_ok(idx, rows[:1020])
    idx.add(rows[1020:])                                                   # (grows the storage: 1500 rows need 24 tiles)
    _image_ok(idx, rows)
    q0 = O.gen_rows(41, 0, 1, dim)[0]
    far = int(np.argmax(O.all_distances(0, rows[:1000], q0)))              # a node of the graph, far from the queries ...
    idx.update(far, q0)                                                    # ... becomes what they look for
    rows2 = rows.copy(); rows2[far] = q0
    _image_ok(idx, rows2)
    # the walk enters ELSEWHERE and meets the row as a neighbour in a hop that starts with a full list (efSearch 16 = the entry's 16 links:
    # full after the first hop), where a stale image would have it rejected: one node in five links to it, none of them the entry or a
    # neighbour of the entry
    ef = 16
    entry = next(e for e in range(17, 1000) if e != far and deg[e] == m and far not in links[e].tolist())
    near = set(links[entry].tolist()) | {entry, far}
    for i in range(0, 1000, 5):
        if i not in near and deg[i]:
            links[i, deg[i] - 1] = far
    g = DeviceGraph(idx, np.zeros(1000, np.int8), deg, links, entry=entry)
    qs = (q0[None, :] + np.float32(1e-3) * O.gen_rows(42, 0, NQ, dim)).astype(np.float32)
    rn, ra, sa, _, _ = _arms(g, qs, k, ef)
    _same(ra, rn)
    assert sa["queries"] > NQ // 2 and np.all(ra[0][:, 0] == far)


def test_a_copy_that_cannot_be_allocated_is_given_up_alone():
    import os
    n, dim, m = 1500, 128, 16
    rows = O.gen_rows(60, 0, n, dim)
    try:
        os.environ["QV_TEST_ROWMAJ16_OOM"] = "1"                           # the copy's allocation answers out-of-memory: not an error, no copy
        idx, deg, links = _knn(rows, "cosine", m)
    finally:
        os.environ.pop("QV_TEST_ROWMAJ16_OOM", None)
    with pytest.raises(quiver_amd.QvError) as e:
        idx.debug_read("rowmaj16")
    assert e.value.code == quiver_amd._lib.QV_ERR_UNSUPPORTED
    idx.add(O.gen_rows(61, 0, 3000, dim))                                  # a later growth does not bring it back
    with pytest.raises(quiver_amd.QvError):
        idx.debug_read("rowmaj16")
    g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=2)
    sa = _never_runs(g, idx, O.gen_rows(62, 0, NQ, dim), 10, 64, "cosine")
    assert not sa["plane"]
    fr, fd, _ = idx.search(rows[:4], 1)                                    # everything else is as it was
    assert fr[:, 0].tolist() == [0, 1, 2, 3]


def _never_runs(g, idx, qs, k, ef, metric, nq=NQ, **rule):
    rn, ra, sa, _, _ = _arms(g, qs[:nq], k, ef)
    _same(ra, rn)
    assert sa["queries"] == 0 and sa["evals"] == 0 and sa["rejected"] == 0
    info = g.info()
    assert not quiver_amd.graph_reject_applies(metric, idx.dim, info["n_nodes"], nq, ef, device_info()["cus"], "always", has_plane=sa["plane"],
                                               max_m0=info["max_m0"], **rule)
    return sa


@pytest.mark.parametrize("case", ["no_rowmajor", "l2", "dim96", "max_m0_48", "tombstone", "64_queries"])
def test_where_the_form_must_not_run(case):
    metric = "l2" if case == "l2" else "cosine"
    dim = 96 if case == "dim96" else 128
    n, m, ef, k = 1500, 48 if case == "max_m0_48" else 16, 64, 10
    rows = O.gen_rows(50, 0, n, dim)
    idx, deg, links = _knn(rows, metric, m, rowmajor=case != "no_rowmajor")
    g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=2)
    qs = O.gen_rows(51, 0, NQ, dim)
    if case == "tombstone":
        g.make_buildable(64)
        g.remove([5])
    sa = _never_runs(g, idx, qs, k, ef, metric, nq=64 if case == "64_queries" else NQ, has_tombstones=case == "tombstone")
    assert sa["plane"] == (case in ("max_m0_48", "tombstone", "64_queries"))
    if case in ("no_rowmajor", "l2", "dim96"):
        with pytest.raises(quiver_amd.QvError):
            idx.debug_read("rowmaj16")


def test_the_device_pointer_form_on_a_side_stream():
    import torch
    n, dim, m, ef, k = 3000, 128, 24, 100, 10
    rows = O.gen_rows(777, 0, n, dim)
    idx, deg, links = _knn(rows, "cosine", m)
    g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=11)
    qs = O.gen_rows(778, 0, NQ, dim)
    g.set_reject_plane("never")
    r, d, c, ev = g.search(qs, k, ef, with_evals=True)
    g.set_reject_plane("always")
    s0 = g.reject_stats()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dq = torch.from_numpy(qs).cuda()
        dr = torch.empty((NQ, k), dtype=torch.int32, device="cuda"); dd = torch.empty((NQ, k), dtype=torch.float32, device="cuda")
        dc = torch.empty(NQ, dtype=torch.int32, device="cuda"); de = torch.empty(NQ, dtype=torch.int32, device="cuda")
        g.search_device(dq.data_ptr(), NQ, k, ef, dr.data_ptr(), dd.data_ptr(), dc.data_ptr(), de.data_ptr(), side.cuda_stream)
    side.synchronize()
    s1 = g.reject_stats()
    c2 = dc.cpu().numpy().view(np.uint32)
    ok = c2 != 0xFFFFFFFE                                                  # tie-flagged queries are redone by the host-pointer form only
    assert ok.sum() >= NQ - 10 and s1["queries"] - s0["queries"] == int(ok.sum())
    assert np.array_equal(c2[ok], c[ok])
    assert np.array_equal(dr.cpu().numpy().view(np.uint32)[ok], r[ok])
    assert np.array_equal(dd.cpu().numpy().view(np.uint32)[ok], d.view(np.uint32)[ok])
    assert np.array_equal(de.cpu().numpy().view(np.uint32)[ok], ev[ok])
