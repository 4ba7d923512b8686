"""Every *_device entry point of include/qv.h on busy, interleaved caller streams (the protocol and the cases: tests/_busy.py).

A call is enqueued behind a block of matrix products on a non-default stream; its true inputs reach the buffer it reads only behind that
block, decoys stand there before and after, and its outputs hold a pattern until it writes them.  A kernel, fill or copy the library puts
on another stream, an input it reads late or a result it writes late gives the decoy's answer or the pattern — never the oracle's
(tests/test_busy_streams_cpu.py proves the decoys' answers differ).  Where the header promises "no synchronisation" the call must also
RETURN while the block is still running (B.returned_busy).  Expected results are the oracle's; the host-pointer form must give the same
bits."""
import numpy as np
import pytest

import quiver_amd
from quiver_amd import QvError, ShardedIndex
from quiver_amd.device_index import DeviceGraph, device_info, merge_topk_device, merge_topk_shards_device
from tests import _busy as B, _route as R

pytestmark = pytest.mark.gpu

UNSUPPORTED = -8
_INDEXES, _WANT, _EXTRA = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _shared_indexes():
    """one index per shape, shared across the cases, and the oracle's answer of every case computed once"""
    yield
    for x in list(_EXTRA.values()) + list(_INDEXES.values()):
        if hasattr(x, "close"):
            x.close()
    _EXTRA.clear(); _INDEXES.clear(); _WANT.clear()
    import torch
    torch.cuda.empty_cache()


def _index(c, **kw):
    key = (c.metric, c.n, c.dim, c.corpus_seed, tuple(sorted(kw.items())))
    if key not in _INDEXES:
        idx = quiver_amd.DeviceIndex(c.dim, c.metric, **kw)
        idx.add(c.rows())
        if c.dead is not None:
            idx.remove(c.dead)
        _INDEXES[key] = idx
    return _INDEXES[key]


def _index600():
    return _index(B.search_case("the-600x16-index", "cosine", 600, 16, 1, 10), filter="off")


def _want(c):
    if c.name not in _WANT:
        _WANT[c.name] = c.expect(c.true())
    return _WANT[c.name]


def _cus():
    return device_info(0)["cus"]


def _lists(c, warm=True, then=None):
    return dict(inputs=[(c.true()[0], c.decoy()[0])], outputs=[((c.nq, c.k), "rows"), ((c.nq, c.k), "dist")], warm=warm, then=then)


def _search_call(idx, c, warm=True):
    return B.Call(c.name, lambda ins, outs, s: idx.search_device(ins[0], c.nq, c.k, outs[0], outs[1], s), **_lists(c, warm))


def _modes(idx, c):
    idx.set_bound_scan(c.mode); idx.set_bound_plane(c.plane)


def _same_as_host_form(c, got, host):
    """the host-pointer form's rows, float32 bits and counts"""
    (rows, dist), (hr, hd, hc) = got[:2], host
    assert np.array_equal(rows, hr) and dist.tobytes() == hd.tobytes(), c.name
    assert [(int((rows[q] != B.NO_ROW).sum())) for q in range(c.nq)] == [int(x) for x in hc], c.name


# ---- 1. DeviceIndex.search_device: every flat route, the paths above k = 64, an empty index ----------------------------------------------

def _flat_case(name):
    return next(c for c in B.flat_cases(_cus()) if c.name == name)


def test_the_flat_cases_reach_the_ten_routes_on_this_device():
    routes = {}
    for c in B.flat_cases(_cus()):
        if c.k <= 64:
            idx = _index(c, filter="off")
            routes[c.name] = B.flat_route(c, _cus(), idx.bound_scan_stats()["plane"], idx.bound_scan8_stats()["plane"])
    assert routes == B.FLAT_ROUTES
    assert set(routes.values()) == set(range(len(R.ROUTES)))


@pytest.mark.parametrize("name", [c.name for c in B.flat_cases()])
def test_search_device(name):
    c = _flat_case(name)
    idx = _index(c, filter="off")
    _modes(idx, c)

    def once():
        call = _search_call(idx, c)
        B.run([[call]])
        c.check(*call.got, _want(c))
        once.got = call.got
        return call.busy
    B.returned_busy(once)
    _same_as_host_form(c, once.got, idx.search(c.true()[0], c.k))


def test_search_device_on_an_empty_index_pads_every_list():
    """only the padding is asserted"""
    c = B.search_case("empty", "cosine", 600, 16, 2, 10)
    idx = quiver_amd.DeviceIndex(16, "cosine")
    call = _search_call(idx, c)
    B.run([[call]])
    rows, dist = call.got
    assert (rows == B.NO_ROW).all() and np.isposinf(dist).all()
    idx.close()


# ---- 2. search_batched_device ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", B.batched_cases(), ids=lambda c: c.name)
def test_search_batched_device(c):
    """64 queries, and 297: a head of 256 and a tail of 41 as a second call on the same stream.  The flags are an output like the lists;
    a flagged query is redone with search_device on the same stream"""
    import torch
    idx = _index(c)
    true = c.true()[0]

    def call_():
        return B.Call(c.name, lambda ins, outs, s: idx.search_batched_device(ins[0], c.nq, c.k, outs[0], outs[1], outs[2], s),
                      inputs=[(true, c.decoy()[0])], outputs=[((c.nq, c.k), "rows"), ((c.nq, c.k), "dist"), ((c.nq,), "rows")])

    def once():
        call = call_()
        lane = B.run([[call]])[0]
        rows, dist, flags = call.got
        assert np.isin(flags, (0, 1)).all(), flags
        redo = np.flatnonzero(flags)
        print("batched %s: %d of %d handed back" % (c.name, redo.size, c.nq))
        if redo.size:
            with torch.cuda.stream(lane.st):
                dq = B._to_dev(true[redo])
                dr = torch.empty((redo.size, c.k), dtype=torch.int32, device="cuda"); dd = torch.empty((redo.size, c.k), dtype=torch.float32, device="cuda")
                idx.search_device(dq.data_ptr(), redo.size, c.k, dr.data_ptr(), dd.data_ptr(), lane.st.cuda_stream)
                rows[redo] = dr.cpu().numpy().view(np.uint32); dist[redo] = dd.cpu().numpy()
        c.check(rows, dist, _want(c))
        once.got = (rows, dist)
        return call.busy
    B.returned_busy(once)
    _same_as_host_form(c, once.got, idx.search(true, c.k))


def test_search_batched_device_refuses_one_row_fewer():
    """the corpus of the cases above is the smallest the path takes"""
    import torch
    c = B.batched_cases()[0]
    idx = quiver_amd.DeviceIndex(c.dim, c.metric)
    idx.add_synthetic(1, 0, c.n - 1)
    dq = B._to_dev(c.true()[0]); dr = torch.zeros((c.nq, c.k), dtype=torch.int32, device="cuda"); dd = torch.zeros((c.nq, c.k), dtype=torch.float32, device="cuda")
    df = torch.zeros(c.nq, dtype=torch.int32, device="cuda")
    with pytest.raises(QvError) as e:
        idx.search_batched_device(dq.data_ptr(), c.nq, c.k, dr.data_ptr(), dd.data_ptr(), df.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert e.value.code == UNSUPPORTED
    torch.cuda.synchronize()
    idx.close()


# ---- 3. search_rowsets_device, search_where_device -------------------------------------------------------------------------------------------

def _rowsets(idx, c):
    made = {}
    for m in c.masks:
        if m is not None and id(m) not in made:
            made[id(m)] = idx.rowset(m)
    return [None if m is None else made[id(m)] for m in c.masks], list(made.values())


@pytest.mark.parametrize("c", B.rowset_cases(), ids=lambda c: c.name)
def test_search_rowsets_device(c):
    idx = _index(c)
    sets, owned = _rowsets(idx, c)

    def call_():
        return B.Call(c.name, lambda ins, outs, s: idx.search_rowsets_device(ins[0], c.nq, c.k, sets, outs[0], outs[1], s), **_lists(c))

    def once():
        call = call_()
        B.run([[call]])
        c.check(*call.got, _want(c))
        once.got = call.got
        return call.busy
    B.returned_busy(once)
    _same_as_host_form(c, once.got, idx.search_rowsets(c.true()[0], c.k, sets))
    for s in owned:
        s.close()


def test_search_rowsets_device_of_40_queries_under_filtered_batch_always():
    """a shape the filtered batch's rule takes (tests/test_busy_streams_cpu.py) — for the HOST forms, which read its hand-back flags; the
    device-pointer form keeps the exact passes whatever the setter says (include/qv.h), so its counters do not move.  Results only."""
    c = B.filtered_batch_case()
    idx = _index(c)
    sets, owned = _rowsets(idx, c)
    idx.set_filtered_batch("always")
    try:
        f0 = idx.filtered_batch_stats()
        call = B.Call(c.name, lambda ins, outs, s: idx.search_rowsets_device(ins[0], c.nq, c.k, sets, outs[0], outs[1], s), **_lists(c))
        B.run([[call]])
        c.check(*call.got, _want(c))
        assert idx.filtered_batch_stats() == f0
        _same_as_host_form(c, call.got, idx.search_rowsets(c.true()[0], c.k, sets))
    finally:
        idx.set_filtered_batch("auto")
        for s in owned:
            s.close()


def _where_filters(idx):
    if "where" not in _EXTRA:
        (f, pf), (u, pu), _ = B.where_columns()
        cf, cu = idx.column("f64"), idx.column("u32")
        cf.set(0, f, pf); cu.set(0, u, pu)
        _EXTRA["where"], _EXTRA["where-u"] = cf, cu
    col = {"f": _EXTRA["where"], "u": _EXTRA["where-u"]}
    return [None if p is None else [(col[name], op, [float(lit)]) for name, op, lit in p] for p in B.WHERE_FILTERS]


@pytest.mark.parametrize("c", B.where_cases(), ids=lambda c: c.name)
def test_search_where_device(c):
    idx = _index(c)
    filters = _where_filters(idx)[:c.nq]
    assert [int((c.live() & m).sum()) for m in c.masks][0] == B.WHERE_FEW                # the first filter selects fewer than k: a padded list

    def call_():
        return B.Call(c.name, lambda ins, outs, s: idx.search_where_device(ins[0], c.nq, c.k, filters, outs[0], outs[1], s), **_lists(c))

    def once():
        call = call_()
        B.run([[call]])
        c.check(*call.got, _want(c))
        once.got = call.got
        return call.busy
    B.returned_busy(once)
    _same_as_host_form(c, once.got, idx.search_where(c.true()[0], c.k, filters))


# ---- 4. distance_rows_device and the merges ------------------------------------------------------------------------------------------------

def test_distance_rows_device():
    c = B.dist_case()
    idx = _index600()
    want = c.expect(c.true())

    def once():
        call = B.Call(c.name, lambda ins, outs, s: idx.distance_rows_device(ins[0], ins[1], c.n_ids, outs[0], s),
                      inputs=list(zip(c.true(), c.decoy())), outputs=[((c.n_ids,), "dist")])
        B.run([[call]])
        assert call.got[0].tobytes() == want.tobytes()
        return call.busy
    B.returned_busy(once)
    assert idx.distance_rows(*c.true()).tobytes() == want.tobytes()


@pytest.mark.parametrize("c", B.merge_cases(), ids=lambda c: c.name)
def test_merges(c):
    want = c.expect(c.true())
    if isinstance(c, B.MergeCase):
        def fn(ins, outs, s):
            merge_topk_device(ins[0], ins[1], c.n_lists, c.k, outs[0], outs[1], s)
        shape = (c.k,)
    else:
        def fn(ins, outs, s):
            merge_topk_shards_device(ins[0], ins[1], c.n_lists, c.nq, c.k, outs[0], outs[1], s)
        shape = (c.nq, c.k)
        want = (np.stack([r for r, _ in want]), np.stack([d for _, d in want]))

    def once():
        call = B.Call(c.name, fn, inputs=list(zip(c.true(), c.decoy())), outputs=[(shape, "rows"), (shape, "dist")])
        B.run([[call]])
        assert np.array_equal(call.got[0], want[0]) and call.got[1].tobytes() == want[1].tobytes(), c.name
        return call.busy
    B.returned_busy(once)


# ---- 5. add_device -------------------------------------------------------------------------------------------------------------------------

def test_add_device_is_synchronous_with_rows_produced_behind_the_block():
    """the rows reach the buffer only behind the busy block; once the call has returned, without any further wait, the host forms see
    them (search on the index's own streams, get_rows)"""
    c = B.add_case()
    idx = quiver_amd.DeviceIndex(c.dim, c.metric, filter="off")
    idx.add(B.corpus(20261017 + c.n, c.n, c.dim))
    true = c.true()
    seen = {}

    def then():
        seen["rows"] = idx.rows()
        seen["search"] = idx.search(c.probe(), 10)
        seen["get"] = idx.get_rows(np.arange(c.n, c.n + c.n_new))

    call = B.Call(c.name, lambda ins, outs, s: seen.__setitem__("first", idx.add_device(ins[0], c.n_new, s)), inputs=list(zip(true, c.decoy())), outputs=[], warm=False, then=then)
    B.run([[call]])
    assert seen["first"] == c.n and seen["rows"] == c.n + c.n_new
    assert seen["get"].tobytes() == true[0].tobytes()
    r, d, cnt = seen["search"]
    for q, (ro, do) in enumerate(c.expect(true)):
        assert cnt[q] == 10 and r[q].tolist() == ro.tolist() and d[q].tobytes() == do.tobytes(), q
    assert r[:3, 0].tolist() == [c.n, c.n + 1, c.n + 2]                       # the new rows are their own nearest
    idx.close()


# ---- 6. graph traversals ------------------------------------------------------------------------------------------------------------------

def _fixture():
    if "graph" not in _EXTRA:
        g = B.fixture_graph()
        n, dim = int(g["n"]), int(g["dim"])
        idx = quiver_amd.DeviceIndex(dim, "cosine", rowmajor=True)
        idx.add(B.corpus(int(g["corpus_seed"]), n, dim))
        _EXTRA["graph"] = DeviceGraph(idx, g["levels"], g["l0_deg"], g["l0_links"], entry=int(g["entry"]), cur_level=int(g["cur_level"]), up_off=g["up_off"], up_links=g["up_links"])
        _EXTRA["graph-index"] = idx
    return _EXTRA["graph"]


def _graph_case(name):
    return next(c for c in B.graph_cases() if c.name == name)


def _graph_call(dg, c, warm=True, then=None, name=None):
    return B.Call(name or c.name, lambda ins, outs, s: dg.search_device(ins[0], c.nq, c.k, c.ef, outs[0], outs[1], outs[2], 0, s),
                  inputs=[(c.true()[0], c.decoy()[0])], outputs=[((c.nq, c.k), "rows"), ((c.nq, c.k), "dist"), ((c.nq,), "rows")], warm=warm, then=then)


def _graph_same_as_host_form(dg, c, got):
    hr, hd, hc = dg.search(c.true()[0], c.k, c.ef)
    rows, dist, count = got
    assert np.array_equal(count, hc), c.name
    for q in range(c.nq):
        n = int(count[q])
        assert np.array_equal(rows[q, :n], hr[q, :n]) and dist[q, :n].tobytes() == hd[q, :n].tobytes(), (c.name, q)


@pytest.mark.parametrize("name", ["graph-1-ef64", "graph-40-ef64"])
def test_graph_search_device(name):
    dg, c = _fixture(), _graph_case(name)

    def once():
        call = _graph_call(dg, c)
        B.run([[call]])
        c.check(*call.got, _want(c))
        once.got = call.got
        return call.busy
    B.returned_busy(once)
    _graph_same_as_host_form(dg, c, once.got)


def _own_fixture_graph():
    """the fixture graph once more, on an index of its own: its visited tables and query block have not grown yet"""
    g = B.fixture_graph()
    n, dim = int(g["n"]), int(g["dim"])
    idx = quiver_amd.DeviceIndex(dim, "cosine", rowmajor=True)
    idx.add(B.corpus(int(g["corpus_seed"]), n, dim))
    return idx, DeviceGraph(idx, g["levels"], g["l0_deg"], g["l0_links"], entry=int(g["entry"]), cur_level=int(g["cur_level"]), up_off=g["up_off"], up_links=g["up_links"])


@pytest.mark.parametrize("first,second", [("graph-40-ef64", "graph-40-ef300"), ("graph-40-ef64-b", "graph-400-ef64")])
def test_graph_search_device_grows_behind_a_traversal_in_flight(first, second):
    """ef 300 after ef 64 on the same warm stream: the visited tables grow; 400 queries after 40: the query block grows.  Both while the
    first traversal waits behind the busy block, on a graph of the test's own.  The warm traversal must have returned busy (it is in
    flight), and the growing call — never made before — must have WAITED for it: had nothing grown, it would have returned busy too"""
    a, b = _graph_case(first), _graph_case(second)

    def once():
        idx, dg = _own_fixture_graph()
        calls = [_graph_call(dg, a), _graph_call(dg, b, warm=False)]
        B.run([calls])
        a.check(*calls[0].got, _want(a)); b.check(*calls[1].got, _want(b))
        _graph_same_as_host_form(dg, b, calls[1].got)
        assert not calls[1].busy, "the second call grew nothing"
        dg.close(); idx.close()
        return calls[0].busy
    B.returned_busy(once)


def test_graph_edits_wait_for_the_traversal_in_flight():
    """a traversal is enqueued behind the busy block, then at once the host removes nodes and inserts one: the edit waits for the traversal
    (qv_graph_api.cpp: ev_last), so the traversal answers for the graph BEFORE the edit, and one enqueued afterwards for the graph after it.
    The traversal must have returned busy: only then was it in flight when the edit began"""
    c = _graph_case("graph-edit-8")
    rows, levels = B.edit_rows(), B.edit_levels()
    h = B.edit_oracle()
    pre = c.expect(c.true(), h)
    nodes = B.edit_removed(pre)
    for x in nodes:
        h.delete(x)
    h.insert_batch(rows[B.EDIT_N:B.EDIT_N + 1])
    post = c.expect(c.true(), h)

    def once():
        idx = quiver_amd.DeviceIndex(B.EDIT_DIM, "cosine", rowmajor=True)
        idx.add(rows)
        dg = DeviceGraph.build(idx, levels[:B.EDIT_N], m=B.EDIT_M, max_m0=B.EDIT_M0, ef_construction=B.EDIT_EFC, batch_max=B.EDIT_BM, ramp_div=B.EDIT_RD)

        def edit():
            dg.remove(nodes)
            dg.insert(B.EDIT_N, levels[B.EDIT_N:B.EDIT_N + 1], 1, 0)

        calls = [_graph_call(dg, c, then=edit, name="graph-edit-8-before"), _graph_call(dg, c, warm=False, name="graph-edit-8-after")]
        B.run([calls])
        c.check(*calls[0].got, pre, "before the edit")
        c.check(*calls[1].got, post, "after the edit")
        assert not np.isin(calls[1].got[0], np.array(nodes, dtype=np.uint32)).any()
        dg.close(); idx.close()
        return calls[0].busy
    B.returned_busy(once)


def test_graph_search_device_on_two_streams_in_turns():
    """A: 1 query, B: 40, A: 1, B: 40 — device-form traversals of one graph are ordered one after another whatever their streams.  All
    four must have returned busy: only then were they enqueued in turns with nothing finished in between"""
    dg = _fixture()
    cs = [_graph_case(n) for n in ("graph-1-ef64", "graph-40-ef64", "graph-1-ef64-b", "graph-40-ef64-b")]

    def once():
        calls = [_graph_call(dg, c) for c in cs]
        B.run([[calls[0], calls[2]], [calls[1], calls[3]]])
        for c, call in zip(cs, calls):
            c.check(*call.got, _want(c))
        return all(call.busy for call in calls)
    B.returned_busy(once)


# ---- 7. the sharded handle -----------------------------------------------------------------------------------------------------------------

def _sharded():
    if "sharded" not in _EXTRA:
        sh = ShardedIndex(B.SHARDED_DIM, "cosine", devices=[0, 0, 0], peer_copy=True)
        gids = sh.add(B.corpus(7, B.SHARDED_N, B.SHARDED_DIM))
        assert (np.diff(gids.astype(np.int64)) > 0).all()                     # global ids ascend with the rows: ties order alike
        _EXTRA["sharded"], _EXTRA["sharded-gids"] = sh, gids
    return _EXTRA["sharded"]


def _sharded_want(c):
    gids = _EXTRA["sharded-gids"]
    return [(gids[ro], do) for ro, do in _want(c)]


def _sharded_call(sh, c):
    return B.Call(c.name, lambda ins, outs, s: sh.search_device(ins[0], c.nq, c.k, outs[0], outs[1], s), **_lists(c))


@pytest.mark.parametrize("c", B.sharded_cases()[:4], ids=lambda c: c.name)
def test_sharded_search_device(c):
    sh = _sharded()

    def once():
        call = _sharded_call(sh, c)
        B.run([[call]])
        c.check(*call.got, _sharded_want(c))
        once.got = call.got
        return call.busy
    B.returned_busy(once)
    _same_as_host_form(c, once.got, sh.search(c.true()[0], c.k))


def test_sharded_search_device_from_two_caller_streams_in_turns():
    sh = _sharded()
    cs = B.sharded_cases()
    order = [cs[4], cs[5], cs[2], cs[3]]                                      # A: 1 query, B: 5, A: 40, B: 5 at k = 100

    def once():
        calls = [_sharded_call(sh, c) for c in order]
        B.run([[calls[0], calls[2]], [calls[1], calls[3]]])
        for c, call in zip(order, calls):
            c.check(*call.got, _sharded_want(c))
        return all(call.busy for call in calls)               # (in turns only if none waited)
    B.returned_busy(once)


# ---- 8. two busy streams in turns on one index ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(B.INTERLEAVED))
def test_two_streams_in_turns_on_one_index(kind):
    """A, B, A, B without any wait, a busy block, queries and outputs per stream; the bound routes share the index's d_bound_stats, whose
    `searches` counter must rise by exactly the queries sent on bound routes"""
    cs = B.interleaved_cases(kind)
    idx = _index600()
    _modes(idx, cs[0])
    assert all((c.mode, c.plane) == (cs[0].mode, cs[0].plane) for c in cs)
    plane, plane8 = idx.bound_scan_stats()["plane"], idx.bound_scan8_stats()["plane"]
    on_bound_routes = sum(c.nq for c in cs if B.flat_route(c, _cus(), plane, plane8) in R.BOUND_ROUTES)
    assert on_bound_routes == (0 if kind in ("small", "mq") else sum(c.nq for c in cs))

    def once():
        calls = [_search_call(idx, c) for c in cs]
        stats = {}
        B.run([[calls[0], calls[2]], [calls[1], calls[3]]], after_warm=lambda: stats.update(before=idx.bound_scan_stats()))
        after = idx.bound_scan_stats()
        for c, call in zip(cs, calls):
            c.check(*call.got, _want(c))
        assert after["searches"] - stats["before"]["searches"] == on_bound_routes
        return all(call.busy for call in calls)               # (in turns only if none waited)
    B.returned_busy(once)


# ---- 9. growth while earlier work is in flight ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first,second", B.GROWTH_PAIRS)
def test_the_workspace_grows_while_an_earlier_call_is_in_flight(first, second):
    """a warm call, then — without a wait — a call that needs a larger workspace than its stream has: 32 queries behind 1, k = 200 behind
    1, 8 queries at k = 200 behind 32.  The library drains the stream before it replaces the buffer the earlier call still uses.  The warm
    call must have returned busy (it is in flight), and the second call — never made on this index before — must have WAITED: had the
    workspace been large enough, it would have returned busy like the first"""
    cs = {c.name: c for c in B.growth_cases()}
    a, b = cs[first], cs[second]

    def once():
        idx = quiver_amd.DeviceIndex(a.dim, a.metric, filter="off")          # (an index of its own: no stream has a workspace for it yet)
        idx.add(a.rows())
        calls = [_search_call(idx, a), _search_call(idx, b, warm=False)]
        B.run([calls])
        a.check(*calls[0].got, _want(a)); b.check(*calls[1].got, _want(b))
        assert not calls[1].busy, "the second call did not have to grow the workspace"
        idx.close()
        return calls[0].busy
    B.returned_busy(once)
