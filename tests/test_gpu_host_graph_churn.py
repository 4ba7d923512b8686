"""hnsw.HNSW under Delete / Insert / Search traffic: the mutations edit the device graph in place (qv_graph_remove,
qv_graph_insert of one node + qv_graph_export_lists), so the device copy stays current — no upload of the whole graph, no
search driven hop by hop from the host — and everything still equals the CPU oracle doing the same calls.

Ids are zero-padded node numbers, so the reference's (Distance, VectorID) order is the oracle's (distance, node) order."""
from dataclasses import dataclass

import numpy as np
import pytest

from quiver_amd.device_index import graph_batch_size
from tests import _oracle as O

pytestmark = pytest.mark.gpu

DIM, CFG = 32, dict(M=8, EfConstruction=40, EfSearch=48, MaxLevel=6)
BM, RD = 64, 8


def _pair(n, rows, seed=17):
    from quiver_amd import hnsw
    h = hnsw.HNSW(hnsw.Config(DistanceFunc="hnsw_cosine", Seed=seed, **CFG))
    h.InsertBatch(["%06d" % i for i in range(n)], rows[:n], BM, RD)
    o = O.HNSW(5, DIM, M=CFG["M"], efConstruction=CFG["EfConstruction"], efSearch=CFG["EfSearch"], maxLevel=CFG["MaxLevel"], seed=seed)
    done = 0
    while done < n:
        b = min(graph_batch_size(done, BM, RD), n - done)
        o.insert_batch(rows[done:done + b]); done += b
    return h, o


def _graph(x):
    return [(x.node_level(i), [x.links(i, l).tolist() for l in range(x.node_level(i) + 1)]) for i in range(x.nodes())], x.entry_point()


def _bits(d):
    return np.asarray(d, dtype=np.float32).view(np.uint32)


def test_seeded_mix_of_deletes_inserts_and_searches_stays_on_the_device():
    n = 1500
    rows = O.gen_rows(515, 0, n + 200, DIM)
    qs = O.gen_rows(516, 0, 200, DIM)
    h, o = _pair(n, rows)
    assert h.built_on_device() and _graph(h) == _graph(o)
    rng = np.random.default_rng(20)
    live = list(range(n))
    nodes = n
    issued = {"delete": 0, "insert": 0, "search": 0}
    for step in range(200):
        op = rng.choice(["delete", "insert", "search"], p=[0.3, 0.3, 0.4])
        issued[op] += 1
        if op == "delete":
            x = live.pop(int(rng.integers(len(live))))
            h.Delete("%06d" % x); assert o.delete(x) == 0
        elif op == "insert":
            h.Insert("%06d" % nodes, rows[nodes]); assert o.insert(rows[nodes]) == nodes
            live.append(nodes); nodes += 1
        else:
            q = qs[step]
            calls = h.distance_calls()
            got = h.Search(q, 5)
            assert h.distance_calls() == calls, "search %d was driven from the host" % step
            ro, do = o.search(q, 5)
            assert [r.VectorID for r in got] == ["%06d" % r for r in ro], step
            assert np.array_equal(_bits([r.Distance for r in got]), _bits(do)), step
    assert min(issued.values()) >= 40
    assert _graph(h) == _graph(o)
    assert h.device_state() == {"full_uploads": 0, "device_removes": issued["delete"], "device_inserts": issued["insert"], "host_searches": 0}
    # a batch after the churn extends the same device graph
    more = O.gen_rows(517, 0, 100, DIM)
    h.InsertBatch(["%06d" % (nodes + i) for i in range(100)], more, BM, RD)
    done = 0
    while done < 100:
        b = min(graph_batch_size(nodes + done, BM, RD), 100 - done)
        o.insert_batch(more[done:done + b]); done += b
    assert h.built_on_device() and _graph(h) == _graph(o) and h.device_state()["full_uploads"] == 0


def test_deleting_the_entry_point_and_everything_keeps_both_sides_in_step():
    n = 300
    rows = O.gen_rows(615, 0, n + 4, DIM)
    h, o = _pair(n, rows, seed=3)
    q = O.gen_rows(616, 0, 1, DIM)[0]
    for rnd in range(3):                                               # the entry point, three times over
        e = o.entry_point()[0]
        h.Delete("%06d" % e); o.delete(e)
        assert _graph(h) == _graph(o)
        got = h.Search(q, 5); ro, do = o.search(q, 5)
        assert [r.VectorID for r in got] == ["%06d" % r for r in ro] and np.array_equal(_bits([r.Distance for r in got]), _bits(do))
    st = h.device_state()
    assert st["device_removes"] == 3 and st["full_uploads"] == 0 and st["host_searches"] == 0
    for x in range(n):
        if o.node_level(x) >= 0:
            h.Delete("%06d" % x); o.delete(x)
    assert h.Size() == 0 and h.Search(q, 5) == [] and _graph(h) == _graph(o)
    for i in range(n, n + 4):                                          # the first finds nothing to link to, the rest link to it
        h.Insert("%06d" % i, rows[i]); o.insert(rows[i])
        assert _graph(h) == _graph(o), i
    got = h.Search(q, 3); ro, do = o.search(q, 3)
    assert [r.VectorID for r in got] == ["%06d" % r for r in ro] and np.array_equal(_bits([r.Distance for r in got]), _bits(do))
    assert h.device_state()["full_uploads"] == 0


@dataclass
class _Hit:
    ID: str
    Distance: float


class _AsCoreIndex:
    """hnsw.HNSW behind the core.Index / core.BatchIndex seam of Collection"""

    def __init__(self, h):
        self.h = h

    def Insert(self, id, vector):
        self.h.Insert(id, vector)

    def InsertBatch(self, vectors: dict):
        self.h.InsertBatch(list(vectors.keys()), np.stack(list(vectors.values())), BM, RD)

    def Delete(self, id):
        self.h.Delete(id)

    def Size(self):
        return self.h.Size()

    def Search(self, vector, k):
        return [_Hit(r.VectorID, r.Distance) for r in self.h.Search(vector, k)]


def test_collection_update_round_keeps_the_device_graph():
    from quiver_amd import core, hnsw
    n = 600
    rows = O.gen_rows(715, 0, n + 40, DIM)
    h = hnsw.HNSW(hnsw.Config(DistanceFunc="hnsw_cosine", Seed=23, **CFG))
    c = core.Collection("c", DIM, _AsCoreIndex(h))
    c.AddBatch([core.Vector("%06d" % i, rows[i]) for i in range(n)])
    o = O.HNSW(5, DIM, M=CFG["M"], efConstruction=CFG["EfConstruction"], efSearch=CFG["EfSearch"], maxLevel=CFG["MaxLevel"], seed=23)
    done = 0
    while done < n:
        b = min(graph_batch_size(done, BM, RD), n - done)
        o.insert_batch(rows[done:done + b]); done += b
    id_of = {i: "%06d" % i for i in range(n)}
    node_of = {v: k for k, v in id_of.items()}
    for j, x in enumerate(np.random.default_rng(30).choice(n, 40, replace=False).tolist()):
        id_ = "%06d" % x
        c.Update(id_, vector=rows[n + j])                              # collection.go:438-444: Delete + Insert
        o.delete(node_of[id_]); new = o.insert(rows[n + j])
        del id_of[node_of[id_]]; id_of[new] = id_; node_of[id_] = new
    assert _graph(h) == _graph(o)
    for q in O.gen_rows(716, 0, 12, DIM):
        resp = c.Search(core.SearchRequest(Vector=q, TopK=5))
        ro, do = o.search(q, 5)
        assert [it.ID for it in resp.Results] == [id_of[int(r)] for r in ro]
        assert np.array_equal(_bits([it.Distance for it in resp.Results]), _bits(do))
    assert h.device_state() == {"full_uploads": 0, "device_removes": 40, "device_inserts": 40, "host_searches": 0}
