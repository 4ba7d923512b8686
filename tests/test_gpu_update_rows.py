"""qv_index_update_rows / qv_index_update_rows_device / qv_sharded_update_rows: one call that overwrites many rows must leave EXACTLY what the
loop of qv_index_update leaves, and what an index that was given the final rows in the first place holds — every array the index keeps
(debug_read), the rows, the distances and every search, bit for bit.  No tolerance anywhere: the scattered ingest computes a row's
constants with ingest's chains, and the planes of the touched tiles are derived by the kernels that serve ingest."""
import functools
import os

import numpy as np
import pytest

import quiver_amd
from quiver_amd import _lib
from tests import _extremes as X
from tests import _oracle as O
from tests.test_gpu_row_state import decode, mixture

pytestmark = pytest.mark.gpu

N = 357                                                     # five whole tiles and a partial one
ARRAYS = ("rnorm", "rres", "plane", "rowmaj16", "plane8", "rres8", "rscale8", "plane6", "rres6")
ALL_FLAGS = dict(rowmajor=True, graph_plane=True, bf16_rows=True)
# (metric, dim, constructor flags, the arrays such an index keeps)
CONFIGS = [
    ("cosine", 768, {}, ("rnorm", "rres", "plane", "plane8", "rres8", "rscale8", "plane6", "rres6")),          # every plane, k_update_rows_tiled
    ("cosine", 768, ALL_FLAGS, ARRAYS),
    ("cosine", 48, {}, ("rnorm", "rres", "plane", "plane8", "rres8")),                                        # the 8-bit plane without the 6-bit plane
    ("cosine", 20, dict(rowmajor=True), ("rnorm", "rres", "plane")),                                          # a multiple of 4, no 8-bit plane
    ("cosine", 7, dict(rowmajor=True), ("rnorm", "rres", "plane")),                                           # k_update_rows
    ("l2", 768, dict(l2_scan_plane=True), ("rnorm", "rres", "plane", "plane8", "rres8", "rscale8", "plane6", "rres6")),
    ("l2", 7, dict(l2_scan_plane=True), ("rnorm", "rres", "plane")),
    ("cosine_f32", 768, {}, ("rnorm",)),                                                                      # the unfused float32 chain and the zero-row sentinel
    ("cosine_f32", 7, {}, ("rnorm",)),
    ("l1", 48, {}, ()),
    ("l1", 7, {}, ()),
]
IDS = ["%s-%d%s" % (m, d, "-flags" if f == ALL_FLAGS else "") for m, d, f, _ in CONFIGS]


@functools.lru_cache(maxsize=None)
def data(dim):
    """base rows, a pool of new vectors (both the mixture of tests/test_gpu_row_state.py: zero, denormal, bfloat16-overflow, NaN and infinity
    rows among ordinary ones), queries, and the lists — computed once per dimension, never written to"""
    rng = np.random.default_rng(977 * dim + 3)
    base, pool = mixture(rng, N, dim), mixture(rng, N, dim)
    qs = rng.standard_normal((4, dim)).astype(np.float32)
    lists = {
        "one row": np.array([100]),
        "rows 63 and 64": np.array([63, 64]),
        "the last row": np.array([N - 1]),
        "every row of a tile": rng.permutation(np.arange(128, 192)),
        "all rows, shuffled": rng.permutation(N),
        "one row three times": np.array([5, 200, 70, 200, 6, 356, 200, 64]),
        "200 rows with repeats": rng.integers(0, N, 200),
    }
    out = {}
    for name, rows in lists.items():
        vecs = pool[rng.integers(0, N, rows.size)]             # (a repeated row gets different vectors: the pool's rows differ)
        final = base.copy()
        for r, v in zip(rows, vecs):
            final[r] = v
        for a in (rows, vecs, final):
            a.setflags(write=False)
        out[name] = (rows.astype(np.uint32), vecs, final)
    assert len({out["one row three times"][1][i].tobytes() for i in (1, 3, 6)}) == 3
    assert len(np.unique(out["200 rows with repeats"][0])) < 200
    for a in (base, pool, qs):
        a.setflags(write=False)
    return base, pool, qs, out


def make(metric, dim, flags, rows):
    idx = quiver_amd.DeviceIndex(dim, metric, **flags)
    idx.add(rows)
    return idx


def by_slot(idx, what, a):
    """a debug_read array as [row slot, bytes of the slot], the first N slots"""
    tiles, dim = (N + 63) // 64, idx.dim
    if what == "plane":
        a = decode(a, tiles, dim)
    elif what == "plane8":
        a = a.reshape(tiles, dim // 16, 64, 16).transpose(0, 2, 1, 3).reshape(tiles * 64, dim)
    elif what == "plane6":
        a = a.reshape(tiles, dim // 64, 3, 64, 16).transpose(0, 3, 1, 2, 4).reshape(tiles * 64, -1)
    elif what != "rowmaj16":
        a = a.reshape(tiles * 64, 1)
    return np.ascontiguousarray(a[:N]).view(np.uint8).reshape(N, -1)


def state(idx, q):
    """every array the index keeps, by row slot, as bytes; the rows and their distances to q"""
    st = {}
    for what in ARRAYS:
        try:
            st[what] = by_slot(idx, what, idx.debug_read(what))
        except quiver_amd.QvError as e:
            assert e.code in (-1, -8), (what, e)                # not kept: an unknown code or QV_ERR_UNSUPPORTED
    every = np.arange(N, dtype=np.uint32)
    st["rows"] = idx.get_rows(every).view(np.uint8).reshape(N, -1)
    st["distance_rows"] = idx.distance_rows(q, every).view(np.uint8).reshape(N, -1)
    st["size"] = np.array([[idx.size(), idx.rows()]])
    return st


def assert_same_state(a, b, what):
    assert sorted(a) == sorted(b), what
    for key in a:
        if not np.array_equal(a[key], b[key]):
            bad = np.flatnonzero((a[key] != b[key]).any(axis=1))
            raise AssertionError("%s: %s differs at row slots %s" % (what, key, bad[:8].tolist()))


@pytest.mark.parametrize("metric,dim,flags,keeps", CONFIGS, ids=IDS)
def test_state_equals_the_final_add_and_the_loop_of_updates(metric, dim, flags, keeps):
    base, _, qs, lists = data(dim)
    for name, (rows, vecs, final) in lists.items():
        a = make(metric, dim, flags, base); a.update_rows(rows, vecs)
        b = make(metric, dim, flags, final)
        c = make(metric, dim, flags, base)
        for r, v in zip(rows, vecs):
            c.update(int(r), v)
        sa = state(a, qs[0])
        assert sorted(k for k in sa if k in ARRAYS) == sorted(keeps), (name, sorted(sa))
        assert np.array_equal(sa["rows"], final.view(np.uint8).reshape(N, -1)), name
        assert_same_state(sa, state(b, qs[0]), name + ": update_rows against add(final)")
        assert_same_state(sa, state(c, qs[0]), name + ": update_rows against update one by one")
        for i in (a, b, c):
            i.close()


def results(idx, qs, k, mask):
    """every entry point and mode the index's shape allows -> {what: (rows, distance bits, counts)}"""
    out = {}

    def take(what, r):
        out[what] = (r[0].copy(), r[1].view(np.uint32).copy(), np.asarray(r[2]).copy())
    take("search", idx.search(qs, k))
    for i in range(len(qs)):
        take("search, query %d alone" % i, idx.search(qs[i], k))
    take("search_batched", idx.search(qs, k, batched=True))
    take("search_masked", idx.search_masked(qs, k, mask))
    take("search_masked, one query", idx.search_masked(qs[1], k, mask))
    return out


@pytest.mark.parametrize("metric,dim,flags,keeps", [CONFIGS[i] for i in (0, 1, 2, 4, 5, 7, 9)], ids=[IDS[i] for i in (0, 1, 2, 4, 5, 7, 9)])
def test_searches_equal_those_of_the_final_add(metric, dim, flags, keeps):
    base, _, qs, lists = data(dim)
    rows, vecs, final = lists["200 rows with repeats"]
    a = make(metric, dim, flags, base); a.update_rows(rows, vecs)
    b = make(metric, dim, flags, final)
    mask = np.random.default_rng(dim).random(N) < 0.5
    k = 10
    modes = [("bound scan off", lambda i: i.set_bound_scan("never")), ("automatic", lambda i: i.set_bound_scan("auto"))]
    if "plane" in keeps:
        modes.append(("bound scan, bfloat16 first", lambda i: (i.set_bound_scan("always"), i.set_bound_plane("bf16"), i.set_bound_plane_filtered("bf16"))))
    if "plane8" in keeps:
        modes.append(("bound scan, 8-bit first", lambda i: (i.set_bound_scan("always"), i.set_bound_plane("8bit"), i.set_bound_plane_filtered("8bit"),
                                                             i.set_bound_plane_mq("8bit"), i.set_bound_plane6("never"))))
    if "plane6" in keeps:
        modes.append(("bound scan, 6-bit first", lambda i: (i.set_bound_scan("always"), i.set_bound_plane("8bit"), i.set_bound_plane6("always"))))
    assert dim != 768 or metric == "cosine_f32" or len(modes) == 5
    for name, setup in modes:
        setup(a); setup(b)
        ra, rb = results(a, qs, k, mask), results(b, qs, k, mask)
        for what in ra:
            for x, y, part in zip(ra[what], rb[what], ("rows", "distance bits", "counts")):
                assert np.array_equal(x, y), (name, what, part)
        if metric == "cosine" and dim == 768 and not flags:       # this configuration also against the CPU oracle, in every mode
            for i, q in enumerate(qs):
                er, ed = O.exact_search(0, final, q, k)
                gr, gd, gc = a.search(q, k)
                assert gc[0] == len(er) and np.array_equal(gr[0, :gc[0]], er) and X.same(gd[0, :gc[0]], ed), (name, i)


def test_dead_rows_are_revived_and_row_sets_follow():
    metric, dim = "cosine", 768
    base, pool, qs, _ = data(dim)
    rng = np.random.default_rng(41)
    idx = make(metric, dim, {}, base)
    R = rng.choice(N, 90, replace=False)
    S, keep_dead = R[:50], R[50:]
    T = np.setdiff1d(np.arange(N), R)[::7]
    rs = idx.rowset(rows=np.concatenate([S[:25], T[:10], keep_dead[:10]]))      # created BEFORE the update: it selects rows that are dead now
    idx.remove(R)
    assert idx.size() == N - 90
    rows = rng.permutation(np.concatenate([S, T]))
    vecs = pool[rng.integers(0, N, rows.size)]
    idx.update_rows(rows, vecs)
    assert idx.size() == N - len(keep_dead) == 357 - 40
    final = base.copy(); final[rows] = vecs
    alive = np.ones(N, bool); alive[keep_dead] = False
    k = 10
    for q in qs:
        er, ed = O.exact_search(0, final, q, k, alive=alive)
        gr, gd, gc = idx.search(q, k)
        assert gc[0] == len(er) and np.array_equal(gr[0, :gc[0]], er) and X.same(gd[0, :gc[0]], ed)
        sel = np.zeros(N, bool); sel[np.concatenate([S[:25], T[:10]])] = True  # the set's dead rows select nothing, its revived rows are found
        er, ed = O.exact_search(0, final, q, k, alive=sel)
        gr, gd, gc = idx.search_rowsets(q, k, [rs])
        assert gc[0] == len(er) and np.array_equal(gr[0, :gc[0]], er) and X.same(gd[0, :gc[0]], ed)
    # the alive words of the device and the host mirror agree: removing a revived row counts once
    idx.remove(S[:5])
    assert idx.size() == N - 45
    rs.close(); idx.close()


def test_refused_calls_change_nothing():
    from quiver_amd._lib import check, lib
    dim = 768
    base, pool, qs, _ = data(dim)
    idx = make("cosine", dim, {}, base)
    idx.remove([3, 300])
    before = state(idx, qs[0])
    rows = np.array([5, 64, N, 300, 7], np.uint32)              # a row == rows(), in the middle of a valid list
    with pytest.raises(quiver_amd.QvError, match="out of range") as e:
        idx.update_rows(rows, pool[:5])
    assert e.value.code == _lib.QV_ERR_OUT_OF_RANGE
    d_vecs = __import__("torch").from_numpy(pool[:5].copy()).cuda()
    with pytest.raises(quiver_amd.QvError, match="out of range") as e:
        idx.update_rows_device(rows, d_vecs.data_ptr())
    assert e.value.code == _lib.QV_ERR_OUT_OF_RANGE
    assert_same_state(before, state(idx, qs[0]), "a refused list")
    assert idx.size() == N - 2
    idx.update_rows(np.zeros(0, np.uint32), np.zeros((0, dim), np.float32))                     # n == 0: fine, nothing happens
    assert lib().qv_index_update_rows(idx.handle, None, 0, None) == 0
    assert lib().qv_index_update_rows_device(idx.handle, None, 0, None, None) == 0
    one = np.array([1], np.uint32)
    for call in (lambda: lib().qv_index_update_rows(idx.handle, None, 1, pool.ctypes.data),
                 lambda: lib().qv_index_update_rows(idx.handle, one.ctypes.data, 1, None),
                 lambda: lib().qv_index_update_rows_device(idx.handle, None, 1, d_vecs.data_ptr(), None),
                 lambda: lib().qv_index_update_rows_device(idx.handle, one.ctypes.data, 1, None, None),
                 lambda: lib().qv_index_update_rows(None, one.ctypes.data, 1, pool.ctypes.data)):
        with pytest.raises(quiver_amd.QvError, match="is null") as e:
            check(call())
        assert e.value.code == -1
    assert_same_state(before, state(idx, qs[0]), "refused pointers and an empty list")
    for bad in (pool[:3, :dim - 1], pool[:2], pool[0]):          # a wrong dimension, fewer vectors than rows
        with pytest.raises(ValueError):
            idx.update_rows([1, 2, 3], bad)
    assert_same_state(before, state(idx, qs[0]), "a wrong shape")
    # what the debug codes of the 8-bit plane answer on an index that keeps none: an unknown code, as the 6-bit codes do
    small = make("cosine", 20, {}, data(20)[0])
    for what in ("plane8", "rres8", "plane6"):
        with pytest.raises(quiver_amd.QvError) as e:
            small.debug_read(what)
        assert e.value.code == -1
    small.close(); idx.close()


@pytest.mark.parametrize("metric,dim,flags,keeps", [CONFIGS[i] for i in (1, 3, 4)], ids=[IDS[i] for i in (1, 3, 4)])
def test_device_form_on_a_stream_of_its_own(metric, dim, flags, keeps):
    """vectors in a torch tensor, a non-default stream; also from an address that is no multiple of 16 bytes (k_update_rows at a
    dimension the tiled kernel would take: the row-major copy it writes is what distance_rows reads)"""
    import torch
    base, _, qs, lists = data(dim)
    rows, vecs, final = lists["200 rows with repeats"]
    host = make(metric, dim, flags, base); host.update_rows(rows, vecs)
    want = state(host, qs[0])
    st = torch.cuda.Stream()
    for shift in (0, 1):
        flat = torch.zeros(vecs.size + 4, dtype=torch.float32, device="cuda")
        with torch.cuda.stream(st):
            flat[shift:shift + vecs.size].copy_(torch.from_numpy(vecs.reshape(-1).copy()), non_blocking=False)
            dev = make(metric, dim, flags, base)
            assert (flat.data_ptr() + 4 * shift) % 16 == 4 * shift
            dev.update_rows_device(rows, flat.data_ptr() + 4 * shift, st.cuda_stream)
        assert_same_state(want, state(dev, qs[0]), "device form, source shifted by %d floats" % shift)
        dev.close()
    host.close()


def test_sharded_update_rows_equals_the_sequence_of_updates():
    dim, n = 48, 200
    rng = np.random.default_rng(12)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    new = rng.standard_normal((40, dim)).astype(np.float32)
    qs = rng.standard_normal((4, dim)).astype(np.float32)

    def fresh():
        s = quiver_amd.ShardedIndex(dim=dim, devices=[0, 0, 0], peer_copy=True)
        return s, s.add(base)
    a, ids = fresh()
    b, ids_b = fresh()
    assert np.array_equal(ids, ids_b) and a.shards() == 3 and all(a.shard_info(g)["rows"] > 0 for g in range(3))
    pick = rng.choice(n, 39, replace=False)
    listed = ids[np.concatenate([pick[:20], pick[3:4], pick[20:]])]           # rows of all three shards, one of them twice
    assert len({int(g) // int(_lib.lib().qv_sharded_span(3)) for g in listed}) == 3
    a.remove(listed[:4]); b.remove(listed[:4])                                   # (some of them dead: revived by both)
    a.update_rows(listed, new)
    for g, v in zip(listed, new):
        b.update(int(g), v)
    assert a.size() == b.size() == n
    assert np.array_equal(a.get_rows(ids).view(np.uint32), b.get_rows(ids).view(np.uint32))
    final = base.copy()
    for g, v in zip(listed, new):
        final[np.flatnonzero(ids == g)[0]] = v
    assert np.array_equal(a.get_rows(ids).view(np.uint32), final.view(np.uint32))
    ra, rb = a.search(qs, 10), b.search(qs, 10)
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1].view(np.uint32), rb[1].view(np.uint32)) and np.array_equal(ra[2], rb[2])
    # a global row that no shard holds, in the middle of a list whose other rows belong to every shard: nothing changes anywhere
    bad = listed.copy(); bad[17] = ids[-1] + 1 if ids[-1] + 1 not in ids else ids.max() + 1
    with pytest.raises(quiver_amd.QvError) as e:
        a.update_rows(bad, new[::-1].copy())
    assert e.value.code == _lib.QV_ERR_OUT_OF_RANGE
    assert np.array_equal(a.get_rows(ids).view(np.uint32), final.view(np.uint32)) and a.size() == n
    with pytest.raises(ValueError):
        a.update_rows(listed, new[:, :dim - 1])
    a.close(); b.close()


def test_many_blocks_and_more_than_one_staged_chunk():
    """70 000 x 64, 50 000 listed rows with repeats; the host form's chunk (256 MiB of vectors) is brought down to 1 MiB — 4096 vectors of this
    dimension, 13 chunks — through QV_UPDATE_ROWS_CHUNK_BYTES, which the library reads once: hence a process of its own"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import numpy as np, quiver_amd
n, dim, m = 70000, 64, 50000
rng = np.random.default_rng(8)
base = rng.standard_normal((n, dim)).astype(np.float32)
rows = rng.integers(0, n, m).astype(np.uint32)
vecs = rng.standard_normal((m, dim)).astype(np.float32)
assert len(np.unique(rows)) < m
final = base.copy()
for r, v in zip(rows, vecs):
    final[r] = v
a = quiver_amd.DeviceIndex(dim, "cosine"); a.add(base); a.update_rows(rows, vecs)
b = quiver_amd.DeviceIndex(dim, "cosine"); b.add(final)
every = np.arange(n, dtype=np.uint32)
assert np.array_equal(a.get_rows(every).view(np.uint32), final.view(np.uint32)), "rows"
for what in ("rnorm", "rres", "rres8"):
    x, y = a.debug_read(what)[:n], b.debug_read(what)[:n]
    assert x.tobytes() == y.tobytes(), what
assert a.debug_read("plane8").tobytes() == b.debug_read("plane8").tobytes(), "plane8"
assert a.size() == n
print("ok")
"""
    env = dict(os.environ, QV_UPDATE_ROWS_CHUNK_BYTES=str(1 << 20), PYTHONPATH=root)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=root)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout + p.stderr


def test_host_mirror_reuses_the_same_slots_in_one_call():
    """HybridIndex (exact): insert 300, DeleteBatch 100, InsertBatch 150 -> 350 device rows, and every id in the slot the per-row loop gave it.
    No switch forces the per-row path in this library, so the assignment is compared with the RULE it followed: the freed slots popped from
    the back, in id order, the rest appended.  Pairs of equal vectors make the rule visible: equal distances are ordered by row."""
    from quiver_amd import hybrid
    from quiver_amd._host import hlib
    dim = 32
    rng = np.random.default_rng(77)
    first = rng.standard_normal((300, dim)).astype(np.float32)
    idx = hybrid.HybridIndex(hybrid.IndexConfig(DistanceFunc="cosine", ExplorationFactor=0.0, Seed=3))
    idx.InsertBatch({"a%d" % i: first[i] for i in range(300)})                  # id a<i> -> row i
    gone = [int(i) for i in rng.permutation(300)[:100]]
    idx.DeleteBatch(["a%d" % i for i in gone])                                   # the free slots, in this order
    fresh = rng.standard_normal((30, dim)).astype(np.float32)[rng.integers(0, 30, 150)]      # 150 new vectors, 30 distinct ones: many ties
    idx.InsertBatch({"n%d" % i: fresh[i] for i in range(150)})
    assert hlib().qvh_hybrid_exact_device_rows(idx._h) == 350
    rows, id_of = np.zeros((350, dim), np.float32), {}
    alive = np.zeros(350, bool)
    for i in range(300):
        if i not in gone:
            rows[i], id_of[i], alive[i] = first[i], "a%d" % i, True
    for i in range(150):
        r = gone[99 - i] if i < 100 else 300 + (i - 100)
        rows[r], id_of[r], alive[r] = fresh[i], "n%d" % i, True
    assert alive.all() and idx.Size() == 350
    for q in (fresh[3], fresh[11], first[0], rng.standard_normal(dim).astype(np.float32)):
        er, ed = O.exact_search(0, rows, q, 350)
        got = idx.SearchWithRequest(hybrid.HybridSearchRequest(Query=q, K=350, ForceStrategy=hybrid.ExactIndexType)).Results
        assert [g.ID for g in got] == [id_of[int(r)] for r in er]
        assert X.same(np.array([g.Distance for g in got], np.float32), ed)
