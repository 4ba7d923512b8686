"""Device-resident HNSW graphs edited in place (qv_graph_remove, qv_graph_export_lists) against the CPU oracle's
restatement of hnsw.HNSW.Delete (pkg/hnsw/hnsw.go:741-842, qvo_hnsw_delete).

The graphs are built like tests/test_gpu_build.py builds them (DeviceGraph.build beside the oracle's insert_batch on the same
schedule); the same nodes are then deleted on both sides.  The oracle's export leaves out dead nodes' blocks, so graphs are
compared per LIVE node and level: the oracle's list against the device list found through the device's own up_off — link for
link, in order — plus the levels (-1 for dead nodes) and the entry point."""
import numpy as np
import pytest

import quiver_amd
from quiver_amd.device_index import DeviceGraph, random_levels
from tests import _oracle as O
from tests.test_oracle_hnsw import batch_schedule

pytestmark = pytest.mark.gpu

BM, RD = 64, 8           # the ramped schedule of tests/test_gpu_build.py


def _build(metric, dim, n, m, max_m0, efc, max_level, seed=5, corpus_seed=31337, extra=0):
    """-> (rows [n + extra], levels [n + extra], index holding all rows, device graph of the first n, oracle of the first n)"""
    mid = quiver_amd.metric_id(metric)
    rows = O.gen_rows(corpus_seed, 0, n + extra, dim)
    levels = random_levels(n + extra, max_level, seed)
    idx = quiver_amd.DeviceIndex(dim, metric, rowmajor=True)
    idx.add(rows)
    g = DeviceGraph.build(idx, levels[:n], m=m, max_m0=max_m0, ef_construction=efc, batch_max=BM, ramp_div=RD)
    h = O.HNSW(mid, dim, M=m, maxM0=max_m0, efConstruction=efc, maxLevel=max_level, seed=seed)
    done = 0
    for b in batch_schedule(n, BM, RD):
        h.insert_batch(rows[done:done + b]); done += b
    return rows, levels, idx, g, h


def _snapshot(g):
    return g.export() + (g.info(),)


def _assert_same_live_graph(g: DeviceGraph, h: O.HNSW):
    levels, l0_deg, l0_links, up_off, up_links = g.export()
    info = g.info()
    n = h.nodes()
    assert info["n_nodes"] == n
    assert (info["entry"], info["cur_level"]) == h.entry_point()
    want_levels = np.array([h.node_level(i) for i in range(n)], dtype=np.int8)
    assert np.array_equal(levels, want_levels), "levels differ at %s" % np.nonzero(levels != want_levels)[0][:8].tolist()
    for i in range(n):
        if want_levels[i] < 0:
            continue
        got = l0_links[i, :l0_deg[i]].tolist()
        assert got == h.links(i, 0).tolist(), "level-0 list of node %d: got %s want %s" % (i, got, h.links(i, 0).tolist())
        for l in range(1, int(want_levels[i]) + 1):
            blk = up_links[int(up_off[i]) + l - 1]
            got = blk[1:1 + int(blk[0])].tolist()
            assert got == h.links(i, l).tolist(), "level-%d list of node %d: got %s want %s" % (l, i, got, h.links(i, l).tolist())


def _refusal(call):
    """(code, message) of the QvError `call` raises.  The exception does not outlive this function: a traceback kept in a test's
    frame would keep the test's index and graphs in a reference cycle, to be finalised in any order"""
    try:
        call()
    except quiver_amd.QvError as ex:
        return ex.code, str(ex)
    raise AssertionError("the call was not refused")


def _delete_both(g, h, nodes, one_call=True):
    nodes = [int(x) for x in nodes]
    if one_call:
        g.remove(nodes)
    else:
        for x in nodes:
            g.remove([x])
    for x in nodes:
        h.delete(x)


# ---- the graph after removal ---------------------------------------------------------------------------------------------

def test_scattered_nodes_in_one_call():
    rows, levels, idx, g, h = _build("cosine", 64, 3000, 8, 16, 60, 16)
    nodes = np.random.default_rng(1).choice(3000, 300, replace=False)
    _delete_both(g, h, nodes)
    _assert_same_live_graph(g, h)


def test_one_call_per_node():
    rows, levels, idx, g, h = _build("l2", 32, 1500, 6, 12, 30, 4)
    nodes = np.random.default_rng(2).choice(1500, 120, replace=False)
    _delete_both(g, h, nodes, one_call=False)
    _assert_same_live_graph(g, h)


def test_full_width_lists():
    """M = 32 / MaxM0 = 64: a list fills all 64 lanes of the wavefront that compacts it"""
    rows, levels, idx, g, h = _build("dot", 36, 1500, 32, 64, 80, 16)
    nodes = np.random.default_rng(3).choice(1500, 200, replace=False)
    _delete_both(g, h, nodes)
    _assert_same_live_graph(g, h)


def test_dimension_not_a_multiple_of_four():
    rows, levels, idx, g, h = _build("l2", 20, 1200, 8, 16, 40, 16)
    nodes = np.random.default_rng(4).choice(1200, 150, replace=False)
    _delete_both(g, h, nodes)
    _assert_same_live_graph(g, h)


def test_adjacent_run_and_a_whole_neighbourhood():
    """single lists lose many entries at once, and some become empty"""
    rows, levels, idx, g, h = _build("cosine", 32, 2000, 8, 16, 40, 16)
    nodes = list(range(1000, 1200)) + h.links(77, 0).tolist()
    _delete_both(g, h, nodes)
    _assert_same_live_graph(g, h)


def test_every_node_above_level_zero():
    """self-links (a device-built node of level >= 1 links to itself below its connected level) and the upper blocks"""
    rows, levels, idx, g, h = _build("cosine", 32, 2000, 8, 16, 40, 16)
    nodes = np.nonzero(levels >= 1)[0]
    assert nodes.size > 300
    _delete_both(g, h, nodes)
    _assert_same_live_graph(g, h)


# ---- the entry point -------------------------------------------------------------------------------------------------------

def _small():
    return _build("cosine", 32, 800, 8, 16, 40, 16, seed=9)


def _first_top_connection(h, entry):
    for l in range(h.node_level(entry), -1, -1):
        for c in h.links(entry, l).tolist():
            if c != entry:
                return c
    raise AssertionError("the entry point has no connection")


def test_delete_the_entry_alone():
    rows, levels, idx, g, h = _small()
    entry = h.entry_point()[0]
    _delete_both(g, h, [entry])
    assert g.info()["entry"] != entry
    _assert_same_live_graph(g, h)


@pytest.mark.parametrize("entry_first", [True, False])
def test_delete_the_entry_and_its_first_connection(entry_first):
    rows, levels, idx, g, h = _small()
    entry = h.entry_point()[0]
    c = _first_top_connection(h, entry)
    _delete_both(g, h, [entry, c] if entry_first else [c, entry])
    _assert_same_live_graph(g, h)


def test_delete_the_entry_after_all_of_its_connections():
    """no replacement among its connections: the first live node takes over, with that node's level"""
    rows, levels, idx, g, h = _small()
    entry = h.entry_point()[0]
    conns = []
    for l in range(h.node_level(entry) + 1):
        conns += [c for c in h.links(entry, l).tolist() if c != entry and c not in conns]
    _delete_both(g, h, conns + [entry])
    first_live = next(i for i in range(800) if h.node_level(i) >= 0)
    assert h.entry_point() == (first_live, h.node_level(first_live))
    _assert_same_live_graph(g, h)


def test_delete_every_node_then_insert():
    rows, levels, idx, g, h = _build("cosine", 32, 600, 8, 16, 40, 16, seed=9, extra=80)
    order = np.random.default_rng(6).permutation(600)
    _delete_both(g, h, order)
    _assert_same_live_graph(g, h)
    r, d, c = g.search(rows[:5], 10, 32)
    assert c.tolist() == [0] * 5                                       # hnsw.go:632-634
    # nodes inserted into a graph of tombstones find nothing to link to; the batch after that links to them
    g.insert(600, levels[600:640], BM, RD); h.insert_batch(rows[600:640])
    _assert_same_live_graph(g, h)
    g.insert(640, levels[640:680], BM, RD); h.insert_batch(rows[640:680])
    _assert_same_live_graph(g, h)


def test_one_node_graph():
    rows, levels, idx, g, h = _build("l2", 16, 1, 8, 16, 40, 16, extra=3)
    _delete_both(g, h, [0])
    assert (g.info()["entry"], g.info()["cur_level"]) == (0, -1) == h.entry_point()
    _assert_same_live_graph(g, h)
    for i in range(1, 4):
        g.insert(i, levels[i:i + 1], 1, 0); h.insert_batch(rows[i:i + 1])
        _assert_same_live_graph(g, h)


def test_dead_duplicate_and_out_of_range_nodes():
    rows, levels, idx, g, h = _small()
    _delete_both(g, h, [5, 17])
    g.remove([17])                                                     # already dead: skipped
    g.remove([40, 41, 40, 5])                                          # listed twice / dead: skipped
    h.delete(40); h.delete(41)
    g.remove([])
    _assert_same_live_graph(g, h)
    before = _snapshot(g)
    assert _refusal(lambda: g.remove([100, 800, 101]))[0] == -4        # QV_ERR_OUT_OF_RANGE
    after = _snapshot(g)
    assert all(np.array_equal(a, b) for a, b in zip(before[:5], after[:5])) and before[5] == after[5]
    _assert_same_live_graph(g, h)


def test_an_uploaded_graph_is_refused_until_it_is_made_buildable():
    rows, levels, idx, g, h = _small()
    lv, l0_deg, l0_links, up_off, up_links = g.export()
    info = g.info()
    u = DeviceGraph(idx, lv, l0_deg, l0_links, info["entry"], info["cur_level"], up_off, up_links)
    code, msg = _refusal(lambda: u.remove([3]))
    assert code == -8 and "qv_graph_make_buildable" in msg                # QV_ERR_UNSUPPORTED, qv_graph_insert's wording
    u.make_buildable(40)
    nodes = [3, info["entry"], 99]
    u.remove(nodes)
    for x in nodes:
        h.delete(x)
    _assert_same_live_graph(u, h)


# ---- the per-link distances stay with their links --------------------------------------------------------------------------

def test_inserts_after_removals_prune_by_the_right_distances():
    n, extra = 3000, 1200
    rows, levels, idx, g, h = _build("cosine", 64, n, 8, 16, 60, 16, extra=extra)
    rng = np.random.default_rng(7)
    at = n
    for rnd in range(2):
        alive = np.array([i for i in range(at) if h.node_level(i) >= 0])
        _delete_both(g, h, rng.choice(alive, alive.size // 10, replace=False))
        _assert_same_live_graph(g, h)
        g.insert(at, levels[at:at + 600], BM, RD)
        for b0 in range(at, at + 600, BM):
            h.insert_batch(rows[b0:min(b0 + BM, at + 600)])
        at += 600
        _assert_same_live_graph(g, h)


# ---- searches after removal ------------------------------------------------------------------------------------------------

def _assert_same_searches(g, h, qs, k, ef, must_fill):
    h.set_ef_search(ef)
    r, d, c, ev = g.search(qs, k, ef, with_evals=True)
    compared = 0
    for i in range(qs.shape[0]):
        if must_fill:
            assert c[i] == k, "query %d found %d of %d" % (i, c[i], k)
        if c[i] != k:
            continue
        ro, do, eo = h.search(qs[i], k, with_evals=True)
        assert r[i].tolist() == ro.tolist() and d[i].tobytes() == do.tobytes() and int(ev[i]) == eo - 1, i
        compared += 1
    return compared


@pytest.mark.parametrize("nq", [48, 600])                              # the latency form / one wavefront per query
def test_level_zero_searches_after_removal(nq):
    rows, levels, idx, g, h = _build("cosine", 32, 3000, 8, 16, 60, 1)
    assert int(levels.max()) == 0
    _delete_both(g, h, np.random.default_rng(8).choice(3000, 300, replace=False))
    _assert_same_live_graph(g, h)
    qs = O.gen_rows(4242, 0, nq, 32)
    assert _assert_same_searches(g, h, qs, 10, 64, must_fill=True) == nq


@pytest.mark.parametrize("nq", [48, 600])
def test_multi_level_searches_after_removal(nq):
    """A walk that comes down onto a node of level >= 1 finds only that node's self-links on level 0 and under-fills (the caller
    tops up, hnsw.go:676-710): the queries that fill are compared.  With level seed 7 the oracle alone fills 15 of the 48 and
    165 of the 600 queries (seeds 5 and 6: 13 / 130 and 8 / 113), so at least a quarter is compared."""
    rows, levels, idx, g, h = _build("l2", 32, 3000, 8, 16, 60, 16, seed=7)
    entry = h.entry_point()[0]
    _delete_both(g, h, [entry] + [int(x) for x in np.random.default_rng(9).choice(3000, 300, replace=False) if x != entry])
    qs = O.gen_rows(4243, 0, nq, 32)
    assert _assert_same_searches(g, h, qs, 10, 64, must_fill=False) * 4 >= nq


def test_large_calls_before_and_after_removal():
    """a call large enough for the hubs of the measurement build to be sampled; the product library walks without them either way"""
    n, dim, nq = 4608, 32, 2048
    rows, levels, idx, g, h = _build("cosine", dim, n, 8, 16, 40, 1)
    qs = O.gen_rows(4244, 0, nq, dim)
    r0, d0, c0 = g.search(qs, 10, 64)
    # the most-visited nodes: the ones most lists name, and the ones the first call returned most often
    lv, l0_deg, l0_links = g.export()[:3]
    named = np.bincount(np.concatenate([l0_links[i, :l0_deg[i]] for i in range(n)]), minlength=n)
    found = np.bincount(r0[r0 < n], minlength=n)
    nodes = list(dict.fromkeys(np.argsort(-named, kind="stable")[:32].tolist() + np.argsort(-found, kind="stable")[:32].tolist()))
    nodes += [i for i in range(n) if i not in nodes][:64 - len(nodes)]
    assert len(nodes) == 64
    _delete_both(g, h, nodes)
    _assert_same_live_graph(g, h)
    h.set_ef_search(64)
    r, d, c, ev = g.search(qs, 10, 64, with_evals=True)
    for i in range(0, nq, 16):
        assert c[i] == 10, i
        ro, do, eo = h.search(qs[i], 10, with_evals=True)
        assert r[i].tolist() == ro.tolist() and d[i].tobytes() == do.tobytes() and int(ev[i]) == eo - 1, i
    assert not np.isin(r, np.array(nodes, dtype=np.uint32)).any()


# ---- partial export --------------------------------------------------------------------------------------------------------

def test_export_lists_equals_the_slices_of_export():
    rows, levels, idx, g, h = _build("cosine", 32, 2000, 6, 16, 40, 16)
    g.remove(np.random.default_rng(10).choice(2000, 200, replace=False))
    lv, l0_deg, l0_links, up_off, up_links = g.export()
    rng = np.random.default_rng(11)
    nodes = np.concatenate([rng.integers(0, 2000, 700), np.nonzero(lv < 0)[0][:40], np.nonzero(lv >= 1)[0][:200]]).astype(np.uint32)
    lvls = rng.integers(0, 4, nodes.size).astype(np.int32)
    deg, links = g.export_lists(nodes, lvls)
    assert links.shape == (nodes.size, 16)
    seen = {"dead": 0, "too_high": 0, "upper": 0}
    for j, (x, l) in enumerate(zip(nodes.tolist(), lvls.tolist())):
        if lv[x] < 0 or l > lv[x]:
            seen["dead" if lv[x] < 0 else "too_high"] += 1
            assert deg[j] == 0 and not links[j].any(), (x, l)
        elif l == 0:
            assert deg[j] == l0_deg[x] and links[j, :deg[j]].tolist() == l0_links[x, :l0_deg[x]].tolist() and not links[j, deg[j]:].any(), (x, l)
        else:
            seen["upper"] += 1
            blk = up_links[int(up_off[x]) + l - 1]
            assert deg[j] == blk[0] and links[j, :deg[j]].tolist() == blk[1:1 + int(blk[0])].tolist() and not links[j, deg[j]:].any(), (x, l)
    assert all(v > 0 for v in seen.values()), seen
    assert _refusal(lambda: g.export_lists([2000], [0]))[0] == -4
