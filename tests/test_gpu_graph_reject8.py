"""Graph traversal that rejects neighbours on the index's row-order 8-bit image (QV_FLAG_GRAPH_PLANE8, qv_graph_set_reject_image): rows, float32
bits, counts and evaluation counts are those of the unchanged traversal, of the bfloat16 arm and of the oracle's HNSW.Search on the same graph;
the counters mean what they say, to the row; the image follows the rows; and the form stays away from everything it was not built for.  Every
traversal call carries 1024 queries: up to max(compute units, 768) the latency form runs, which never reads an image."""
import os

import numpy as np
import pytest

import quiver_amd
from quiver_amd.device_index import DeviceGraph, device_info
from tests import _bound8 as B8
from tests import _graph_reject8 as GR8
from tests import _oracle as O

pytestmark = pytest.mark.gpu

NQ = 1024


def _knn(rows, metric, m, **kw):
    """exact m-NN lists (self excluded) through the product's flat scan, on an index that asks for the 8-bit image"""
    n = rows.shape[0]
    kw.setdefault("rowmajor", True); kw.setdefault("graph_plane8", True)
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


def _arms(g, qs, k, ef, image="8bit"):
    """the same call under "never", under "always" on the bfloat16 copy, and under "always" with image mode `image`.
    -> dict: never / bf16 / img results; s8 / s16 = what the last arm added to the 8-bit and to the bfloat16 counters; b8 / b16 = what the bfloat16
    arm added; n8 / n16 = what "never" added; redo = the exact-heap kernel's queries per arm"""
    def stats():
        return g.reject8_stats(), g.reject_stats(), g.stats()["search_redo"]
    g.set_reject_plane("never"); g.set_reject_image(image)
    a = stats(); rn = g.search(qs, k, ef, with_evals=True); b = stats()
    g.set_reject_plane("always"); g.set_reject_image("bf16")
    rb = g.search(qs, k, ef, with_evals=True); c = stats()
    g.set_reject_image(image)
    ri = g.search(qs, k, ef, with_evals=True); d = stats()
    return {"never": rn, "bf16": rb, "img": ri, "n8": _delta(a[0], b[0]), "n16": _delta(a[1], b[1]), "b8": _delta(b[0], c[0]), "b16": _delta(b[1], c[1]),
            "s8": _delta(c[0], d[0]), "s16": _delta(c[1], d[1]), "redo": (b[2] - a[2], c[2] - b[2], d[2] - c[2])}


def _same(ra, rn, what_arm="the unchanged traversal"):
    for a, b, what in zip(ra, rn, ("rows", "distance bits", "counts", "evals")):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        bad = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(a.shape[0], -1).any(axis=1))
        assert bad.size == 0, "%s differ from %s for queries %s" % (what, what_arm, bad[:8].tolist())


def _zero(s):
    return s["evals"] == 0 and s["rejected"] == 0 and s["queries"] == 0


def _oracle_agrees(o, qs, res, k, which):
    r, d, c, ev = res
    for i in which:
        ro, do, eo = o.search(qs[i], k, with_evals=True)
        if c[i] == k:
            assert r[i].tolist() == ro.tolist(), i
            assert d[i].tobytes() == do.tobytes(), i
            assert int(ev[i]) == eo - 1, i                 # the reference also evaluates the entry point once more up front (hnsw.go:637)
        else:                                               # under-filled: the caller tops up (hnsw.go:676-710); the prefix must agree
            assert c[i] < k
            assert r[i, :c[i]].tolist() == ro[:c[i]].tolist(), i


SHAPES = [
    ("cosine", 768, 3000, 32, 128, 10),
    ("dot", 128, 2500, 16, 64, 10),          # one slab
    ("cosine", 128, 2000, 32, 300, 50),      # 5 list registers per lane
    ("dot", 384, 1500, 24, 16, 5),           # an odd slab count; 2 list registers per lane
    ("cosine", 128, 1500, 16, 400, 10),      # 8 list registers per lane
    ("cosine", 256, 1500, 8, 512, 512),      # 9 list registers per lane, k = ef
    ("cosine", 4096, 600, 8, 64, 10),        # the widest the integer sums are proven for
]


@pytest.mark.parametrize("both", [False, True], ids=["image8_only", "both_images"])
@pytest.mark.parametrize("metric,dim,n,m,ef,k", SHAPES)
def test_rejecting_on_the_image_identical_to_the_unchanged_traversal_the_bfloat16_arm_and_the_oracle(metric, dim, n, m, ef, k, both):
    mid = quiver_amd.metric_id(metric)
    rows = O.gen_rows(4242, 0, n, dim)
    idx, deg, links = _knn(rows, metric, m, graph_plane=both)
    g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=7)
    qs = O.gen_rows(4243, 0, NQ, dim)
    a = _arms(g, qs, k, ef)
    _same(a["img"], a["never"])
    _same(a["bf16"], a["never"]); _same(a["img"], a["bf16"], "the bfloat16 arm")
    # every query walked level 0 rejecting on the 8-bit image; the ones flagged for the exact-heap kernel finish there and count in search_redo instead
    assert a["s8"]["plane"] and a["s8"]["queries"] == NQ - a["redo"][2] and _zero(a["s16"]) and _zero(a["n8"]) and _zero(a["n16"])
    assert 0 < a["s8"]["rejected"] <= a["s8"]["evals"] <= int(a["img"][3].sum())
    assert a["redo"][0] == a["redo"][1] == a["redo"][2]
    # the bfloat16 arm: on its copy where that is held (and never on the 8-bit image), the unchanged kernels where it is not
    assert _zero(a["b8"]) and a["b16"]["plane"] == both and a["b16"]["queries"] == (NQ - a["redo"][1] if both else 0)
    o = O.HNSW(mid, dim, M=max(m // 2, 1), maxM0=m, efSearch=ef, maxLevel=1, seed=1)
    o.load_flat(rows, deg, links, 7)
    _oracle_agrees(o, qs, a["img"], k, range(0, NQ, NQ // 48)[:48])


COUNTER_SEED = 9101          # (rows; the queries take the next one) — chosen on the CPU: no walk meets a tie, and the certified share is 0.9656 of R


def test_the_counters_mean_what_they_say_to_the_row():
    """out[0] = the evaluations made in hops that start with a full list; out[1] = EXACTLY the rows the 8-bit interval certifies from the exact integer
    sum, the stored scale and residual (there is no float32 chain, hence no two-margin sandwich); and that count exceeds 0.85 of the rows the exact
    distance rejects, so a kernel that rejects almost nothing does not pass.  CPU, this shape and seed: A 454 021, R 369 501, certified 356 801
    (0.9656 of R)."""
    metric, dim, n, m, ef, k = "cosine", 128, 2000, 16, 32, 10
    rows = O.gen_rows(COUNTER_SEED, 0, n, dim)
    idx, deg, links = _knn(rows, metric, m)
    g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=3)
    qs = O.gen_rows(COUNTER_SEED + 1, 0, NQ, dim)
    a = _arms(g, qs, k, ef)
    _same(a["img"], a["never"])
    assert a["redo"] == (0, 0, 0)                                          # (for this seed no query meets a tie: the counters hold all 1024 walks)
    assert a["s8"]["queries"] == NQ
    state = B8.RowState8(rows)
    A = R = C8 = 0
    for i in range(NQ):
        w = GR8.walk8(0, rows, state, deg, links, 3, qs[i], ef)
        assert not w["ties"], i
        assert w["evals"] == int(a["img"][3][i]), i                        # the restated walk IS the device's walk
        assert [e[1] for e in w["order"][:k]] == a["img"][0][i, :min(k, len(w["order"]))].tolist(), i
        A += w["A"]; R += w["R"]; C8 += w["C8"]
    print("A %d  R %d  certified on the 8-bit image %d (%.4f of R); device: evals %d rejected %d" % (A, R, C8, C8 / R, a["s8"]["evals"], a["s8"]["rejected"]))
    assert C8 > 0.85 * R
    assert a["s8"]["evals"] == A
    assert a["s8"]["rejected"] == C8


def _device_form(g, qs, k, ef):
    """one call of the device-pointer form under the graph's current modes: (flagged [nq], rows, distances, counts, evals, the 8-bit counters the call added)"""
    import torch
    nq = qs.shape[0]
    s0 = g.reject8_stats()
    dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    dr = torch.empty((nq, k), dtype=torch.int32, device="cuda"); dd = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    dc = torch.empty(nq, dtype=torch.int32, device="cuda"); de = torch.empty(nq, dtype=torch.int32, device="cuda")
    g.search_device(dq.data_ptr(), nq, k, ef, dr.data_ptr(), dd.data_ptr(), dc.data_ptr(), de.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    c = dc.cpu().numpy().view(np.uint32)
    return c == 0xFFFFFFFE, dr.cpu().numpy().view(np.uint32), dd.cpu().numpy(), c, de.cpu().numpy().view(np.uint32), _delta(s0, g.reject8_stats())


def test_rows_the_bound_says_nothing_about():
    n, dim, m, ef, k = 2000, 128, 16, 64, 10
    rows = O.gen_rows(5150, 0, n, dim)
    special = [700, 701, 702, 703, 704, 705]
    rows[700] = 0.0
    rows[701, 3] = np.nan
    rows[702, 5] = np.inf
    rows[703] *= np.float32(1e25 / np.sqrt(dim))                           # a norm of about 1e25 (gen_rows' elements are of order one)
    rows[704] *= np.float32(1e-30 / np.sqrt(dim))                          # ... and of about 1e-30
    rows[705] = 0.0; rows[705, 17] = np.float32(0.75)                      # one non-zero element
    idx, deg, links = _knn(rows, "cosine", m)
    for i in range(0, n, 7):                                               # the special rows are nobody's nearest neighbour: link them in by hand
        if deg[i] and i not in special:
            links[i, deg[i] - 1] = special[(i // 7) % len(special)]
    meta = idx.debug_read("rowmeta8")
    for r in special:
        _, sc, res = B8.quantize_row(rows[r])
        assert np.isnan(meta["rres8"][r]) == np.isnan(res) and meta["rscale8"][r].tobytes() == sc.tobytes(), r
    assert all(np.isnan(meta["rres8"][r]) for r in (700, 701, 702, 703, 704)) and not np.isnan(meta["rres8"][705])
    g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=1000)
    qs = O.gen_rows(5151, 0, NQ, dim)
    a = _arms(g, qs, k, ef)
    _same(a["img"], a["never"])
    assert a["s8"]["queries"] == NQ - a["redo"][2] > NQ // 2 and a["s8"]["rejected"] > 0
    # walks that finished in the rejecting form met the special rows in hops that started with a full list: the bound had to speak about them
    flagged = _device_form(g, qs, k, ef)[0]
    state = B8.RowState8(rows)
    met = set()
    for i in np.flatnonzero(~flagged)[:48].tolist():
        w = GR8.walk8(0, rows, state, deg, links, 1000, qs[i], ef)
        assert w["evals"] == int(a["img"][3][i]), i
        met |= set(w["full_rows"]) & set(special)
    assert met == set(special), sorted(met)


def test_queries_the_form_declines():
    n, dim, m, ef, k = 2000, 128, 16, 64, 10
    rows = O.gen_rows(31, 0, n, dim)
    idx, deg, links = _knn(rows, "dot", m)
    g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=5)
    qs = O.gen_rows(32, 0, NQ, dim)
    odd = np.zeros(NQ, bool); odd[[100, 300, 500, 700, 900]] = True
    qs[100] = 0.0
    qs[300, 9] = np.inf
    qs[500, 7] = np.nan
    qs[700] *= np.float32(1e-30)
    qs[900] *= np.float32(1e19)
    a = _arms(g, qs, k, ef)
    _same(a["img"], a["never"])
    flagged, _, _, _, _, sd = _device_form(g, qs, k, ef)                    # (under "always" and "8bit", as _arms leaves the graph)
    want = int((~flagged & ~odd).sum())                                    # the five count in no counter; every other unflagged query does
    assert want >= NQ - 5 - NQ // 8
    assert sd["queries"] == want and a["s8"]["queries"] == want and _zero(a["s16"])
    qs2 = qs.copy(); qs2[odd] = O.gen_rows(33, 0, 5, dim)                   # the same call with the five swapped for ordinary queries: every unflagged query counts
    f2, _, _, _, _, sd2 = _device_form(g, qs2, k, ef)
    assert np.array_equal(f2[~odd], flagged[~odd]) and sd2["queries"] == int((~f2).sum())


def test_near_duplicates_around_the_threshold():
    n, dim, m, ef, k = 3000, 128, 16, 64, 10
    rng = np.random.default_rng(77)
    centres = O.gen_rows(78, 0, 100, dim)
    rows = (centres[np.arange(n) % 100] + np.float32(1e-4) * rng.standard_normal((n, dim)).astype(np.float32)).astype(np.float32)
    idx, deg, links = _knn(rows, "cosine", m, graph_plane=True)
    for i in range(n):                                                     # a k-NN graph of clusters is disconnected: one link a node leads on
        if deg[i]:
            links[i, deg[i] - 1] = (i + 1) % n
    g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=0)
    qs = (centres[np.arange(NQ) % 100] + np.float32(1e-4) * rng.standard_normal((NQ, dim)).astype(np.float32)).astype(np.float32)
    a = _arms(g, qs, k, ef)
    _same(a["img"], a["never"]); _same(a["bf16"], a["never"])
    assert a["s8"]["queries"] > 0 and a["s8"]["rejected"] < a["s8"]["evals"]


def _image_ok(idx, rows, what, tile_plane):
    got, meta = idx.debug_read("rowmaj8"), idx.debug_read("rowmeta8")
    n, dim = rows.shape
    assert got.shape == (n, dim) and meta.shape == (n,), what
    st = B8.RowState8(rows)
    assert np.array_equal(got, st.r8), what
    assert meta["rscale8"].tobytes() == st.scale.tobytes(), what
    assert np.array_equal(meta["rres8"].view(np.uint32)[~np.isnan(st.res)], st.res.view(np.uint32)[~np.isnan(st.res)]) and \
        np.array_equal(np.isnan(meta["rres8"]), np.isnan(st.res)), what
    assert meta["rnorm"].tobytes() == idx.debug_read("rnorm")[:n].tobytes(), what
    if tile_plane:                                                         # the tile-layout 8-bit plane, decoded: [tile][dim / 16][64 rows][16 values]
        tiles = (n + 63) // 64
        p8 = idx.debug_read("plane8").view(np.int8).reshape(tiles, dim // 16, 64, 16).transpose(0, 2, 1, 3).reshape(tiles * 64, dim)[:n]
        assert np.array_equal(got, p8), what
        assert meta["rscale8"].tobytes() == idx.debug_read("rscale8")[:n].tobytes(), what
        assert meta["rres8"].tobytes() == idx.debug_read("rres8")[:n].tobytes(), what


@pytest.mark.parametrize("tile_plane", [True, False], ids=["with_the_tile_plane", "no_scan_plane"])
def test_the_image_follows_the_rows(tile_plane):
    import torch
    dim, m, k = 128, 16, 5
    rows = O.gen_rows(40, 0, 1500, dim)
    idx, deg, links = _knn(rows[:1000], "cosine", m, scan_plane=tile_plane)   # (add)
    _image_ok(idx, rows[:1000], "add", tile_plane)
    dev = torch.from_numpy(rows[1000:1020]).cuda()
    idx.add_device(dev.data_ptr(), 20); torch.cuda.synchronize()           # (within the 16 tiles the first add allocated)
    _image_ok(idx, rows[:1020], "add_device", tile_plane)
    idx.add(rows[1020:])                                                   # (grows the storage: 1500 rows need 24 tiles)
    _image_ok(idx, rows, "an add that grows", tile_plane)
    q0 = O.gen_rows(41, 0, 1, dim)[0]
    far = int(np.argmax(O.all_distances(0, rows[:1000], q0)))              # a node of the graph, far from the queries ...
    idx.update(far, q0)                                                    # ... becomes what they look for
    rows2 = rows.copy(); rows2[far] = q0
    _image_ok(idx, rows2, "update", tile_plane)
    listed = np.array([1100, 1163, 1164, 1300, 1163, 1499], np.uint32)     # (1163 twice: the last one stands)
    vecs = O.gen_rows(43, 0, listed.size, dim)
    idx.update_rows(listed, vecs)
    for r, v in zip(listed, vecs):
        rows2[r] = v
    _image_ok(idx, rows2, "update_rows", tile_plane)
    vecs2 = O.gen_rows(44, 0, listed.size, dim)
    dv = torch.from_numpy(vecs2).cuda()
    idx.update_rows_device(listed[::-1].copy(), dv.data_ptr()); torch.cuda.synchronize()
    for r, v in zip(listed[::-1], vecs2):
        rows2[r] = v
    _image_ok(idx, rows2, "update_rows_device", tile_plane)
    idx.remove([1200, 1201])                                               # remove, then revive with new contents
    idx.update_rows(np.array([1200, 1201], np.uint32), O.gen_rows(45, 0, 2, dim))
    rows2[1200:1202] = O.gen_rows(45, 0, 2, dim)
    _image_ok(idx, rows2, "remove then revive", tile_plane)
    idx.add_synthetic(46, 0, 100)
    rows2 = np.concatenate([rows2, O.gen_rows(46, 0, 100, dim)])
    _image_ok(idx, rows2, "add_synthetic", tile_plane)
    # the walk enters ELSEWHERE and meets the updated row as a neighbour in a hop that starts with a full list (efSearch 16 = the entry's 16 links:
    # full after the first hop), where a stale image would have it rejected
    ef = 16
    entry = next(e for e in range(17, 1000) if e != far and deg[e] == m and far not in links[e].tolist())
    near = set(links[entry].tolist()) | {entry, far}
    for i in range(0, 1000, 5):
        if i not in near and deg[i]:
            links[i, deg[i] - 1] = far
    g = DeviceGraph(idx, np.zeros(1000, np.int8), deg, links, entry=entry)
    qs = (q0[None, :] + np.float32(1e-3) * O.gen_rows(42, 0, NQ, dim)).astype(np.float32)
    a = _arms(g, qs, k, ef)
    _same(a["img"], a["never"])
    assert a["s8"]["queries"] > NQ // 2 and np.all(a["img"][0][:, 0] == far)


def _never_runs(g, idx, qs, k, ef, metric, nq=NQ, image="8bit", form=0, **rule):
    """the 8-bit counters stay zero, results are identical, and the rule function agrees with what ran (`form`: what the last arm must have taken)"""
    a = _arms(g, qs[:nq], k, ef, image=image)
    _same(a["img"], a["never"]); _same(a["bf16"], a["never"])
    assert _zero(a["s8"]) and _zero(a["b8"]) and _zero(a["n8"])
    info = g.info()
    has16, has8 = g.reject_stats()["plane"], g.reject8_stats()["plane"]
    got = quiver_amd.graph_reject_image_applies(metric, idx.dim, info["n_nodes"], nq, ef, device_info()["cus"], "always", has_plane=has16, max_m0=info["max_m0"],
                                                has_image8=has8, image_mode=image, **rule)
    assert got == form
    assert (a["s16"]["queries"] > 0) == (form == 1)
    return a


def test_an_image_that_cannot_be_allocated_is_given_up_alone():
    n, dim, m = 1500, 128, 16
    rows = O.gen_rows(60, 0, n, dim)
    try:
        os.environ["QV_TEST_ROWMAJ8_OOM"] = "1"                            # the image's allocation answers out-of-memory: not an error, no image
        idx, deg, links = _knn(rows, "cosine", m, graph_plane=True)
    finally:
        os.environ.pop("QV_TEST_ROWMAJ8_OOM", None)
    for what in ("rowmaj8", "rowmeta8"):
        with pytest.raises(quiver_amd.QvError) as e:
            idx.debug_read(what)
        assert e.value.code == quiver_amd._lib.QV_ERR_UNSUPPORTED
    idx.add(O.gen_rows(61, 0, 3000, dim))                                  # a later growth does not bring it back
    with pytest.raises(quiver_amd.QvError):
        idx.debug_read("rowmaj8")
    assert idx.debug_read("rowmaj16").shape == (n + 3000, dim)             # the bfloat16 copy is as before ...
    g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=2)
    assert g.reject8_stats()["plane"] is False and g.reject_stats()["plane"] is True
    _never_runs(g, idx, O.gen_rows(62, 0, NQ, dim), 10, 64, "cosine", form=1)   # ... and mode "8bit" rejects on it
    fr, _, _ = idx.search(rows[:4], 1)                                     # every search is as it was
    assert fr[:, 0].tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("case", ["no_rowmajor", "l2", "dim192", "max_m0_48", "tombstone", "64_queries", "image_bf16", "no_flag"])
def test_where_the_form_must_not_run(case):
    metric = "l2" if case == "l2" else "cosine"
    dim = 192 if case == "dim192" else 128
    n, m, ef, k = 1500, 48 if case == "max_m0_48" else 16, 64, 10
    rows = O.gen_rows(50, 0, n, dim)
    idx, deg, links = _knn(rows, metric, m, rowmajor=case != "no_rowmajor", graph_plane=True, graph_plane8=case != "no_flag")
    g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=2)
    qs = O.gen_rows(51, 0, NQ, dim)
    if case == "tombstone":
        g.make_buildable(64)
        g.remove([5])
    # what the last arm takes instead: the bfloat16 copy where that is held and its own conditions hold, else the unchanged kernels
    form = 1 if case in ("dim192", "image_bf16", "no_flag") else 0
    _never_runs(g, idx, qs, k, ef, metric, nq=64 if case == "64_queries" else NQ, image="bf16" if case == "image_bf16" else "8bit", form=form,
                has_tombstones=case == "tombstone")
    assert g.reject8_stats()["plane"] == (case in ("max_m0_48", "tombstone", "64_queries", "image_bf16"))
    assert g.reject_stats()["plane"] == (case not in ("no_rowmajor", "l2"))
    if case in ("no_rowmajor", "l2", "dim192", "no_flag"):
        with pytest.raises(quiver_amd.QvError):
            idx.debug_read("rowmaj8")
    if case == "image_bf16":                                               # mode "auto": no measured cell takes the 8-bit image yet — the bfloat16 copy
        _never_runs(g, idx, qs, k, ef, metric, image="auto", form=1)


def test_the_device_pointer_form_on_a_side_stream():
    import torch
    n, dim, m, ef, k = 3000, 128, 24, 100, 10
    rows = O.gen_rows(777, 0, n, dim)
    idx, deg, links = _knn(rows, "cosine", m)
    g = DeviceGraph(idx, np.zeros(n, np.int8), deg, links, entry=11)
    qs = O.gen_rows(778, 0, NQ, dim)
    g.set_reject_plane("never")
    r, d, c, ev = g.search(qs, k, ef, with_evals=True)
    g.set_reject_plane("always"); g.set_reject_image("8bit")
    s0 = g.reject8_stats()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dq = torch.from_numpy(qs).cuda()
        dr = torch.empty((NQ, k), dtype=torch.int32, device="cuda"); dd = torch.empty((NQ, k), dtype=torch.float32, device="cuda")
        dc = torch.empty(NQ, dtype=torch.int32, device="cuda"); de = torch.empty(NQ, dtype=torch.int32, device="cuda")
        g.search_device(dq.data_ptr(), NQ, k, ef, dr.data_ptr(), dd.data_ptr(), dc.data_ptr(), de.data_ptr(), side.cuda_stream)
    side.synchronize()
    s1 = g.reject8_stats()
    c2 = dc.cpu().numpy().view(np.uint32)
    ok = c2 != 0xFFFFFFFE                                                  # tie-flagged queries are redone by the host-pointer form only
    assert ok.sum() >= NQ - 10 and s1["queries"] - s0["queries"] == int(ok.sum()) and s1["rejected"] > s0["rejected"]
    assert np.array_equal(c2[ok], c[ok])
    assert np.array_equal(dr.cpu().numpy().view(np.uint32)[ok], r[ok])
    assert np.array_equal(dd.cpu().numpy().view(np.uint32)[ok], d.view(np.uint32)[ok])
    assert np.array_equal(de.cpu().numpy().view(np.uint32)[ok], ev[ok])
