"""The 8-bit stage in front of a FILTERED single query (k_bound_scan8<., true>, quiver_amd/csrc/qv_bound_scan.hip): a masked, row-set or
where-filtered search of one query rejects rows on the int8 plane first, over the call's candidate bitmap live & set — a tile without a
candidate is not read, and its lower-bound words are written dead all the same —, then the bfloat16 stage and the exact filtered scan are
gated behind it on the device.  Every case forces the bound scan and the filtered 8-bit plane by the index's setters, runs the same call
again under "never" and compares rows, counts and float32 bits; one query per case also goes to the CPU oracle over live & set.  The
counters say which stage answered: unless a test says otherwise it asserts that the 8-bit stage answered alone."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import quiver_amd
from quiver_amd.device_index import device_info
from tests import _bound as B
from tests import _bound8 as B8
from tests import _bound_filtered as F
from tests import _extremes as X
from tests import _oracle as O
from tests import _route as R
from tests import _widths as W

pytestmark = pytest.mark.gpu

NAME = {B.COSINE: "cosine", B.DOT: "dot"}


def both(idx, call):
    """ONE call under "always" + filtered "8bit", then under "never": the same rows, counts and bits -> (result, the counters' increments)"""
    idx.set_bound_scan("always"); idx.set_bound_plane_filtered("8bit")
    a0, b0 = idx.bound_scan8_stats(), idx.bound_scan_stats()
    r, d, c = call()
    a1, b1 = idx.bound_scan8_stats(), idx.bound_scan_stats()
    idx.set_bound_scan("never")
    er, ed, ec = call()
    assert idx.bound_scan8_stats()["searches"] == a1["searches"] and idx.bound_scan_stats()["searches"] == b1["searches"]   # "never" is never
    assert np.array_equal(c, ec) and np.array_equal(r, er), (r, er)
    assert X.same(d, ed), (d, ed)
    inc = {"took8": a1["searches"] - a0["searches"], "back8": a1["hand_backs"] - a0["hand_backs"], "cand8": a1["candidates"],
           "took": b1["searches"] - b0["searches"], "back": b1["hand_backs"] - b0["hand_backs"], "cand": b1["candidates"]}
    return (r, d, c), inc


def answered_by_the_8bit_stage(inc):
    return inc["took8"] == 1 and inc["back8"] == 0 and inc["took"] == 1 and inc["back"] == 0


def agrees(metric, rows, q, k, alive, r, d, c):
    er, ed = O.exact_search(metric, rows, q, k, alive=np.asarray(alive).astype(np.uint8))
    w = len(er)
    return int(c) == w and r[:w].tolist() == er.tolist() and d[:w].tobytes() == ed.tobytes() and (r[w:] == 0xFFFFFFFF).all() and np.isposinf(d[w:]).all()


def build(case, metric):
    idx = quiver_amd.DeviceIndex(case["rows"].shape[1], NAME[metric])
    idx.add(case["rows"])
    if "dead" in case:
        idx.remove(case["dead"])
    assert idx.bound_scan8_stats()["plane"] and idx.bound_scan_stats()["plane"]
    return idx


# ---- 1. widths and k ---------------------------------------------------------------------------------------------------------------------
_WIDTH_CASES = {}


def width_case(dim):
    """rows, two queries, the 8-bit row state and the masks of one width, built once for both metrics"""
    if dim not in _WIDTH_CASES:
        n = 20_011 if dim < 768 else 9_003
        rows = O.gen_rows(8100 + dim, 0, n, dim)
        qs = O.gen_rows(8101 + dim, 0, 2, dim)
        rng = np.random.default_rng(8102 + dim)
        dead = np.unique(rng.integers(0, n, 200)).astype(np.uint32)
        live = np.ones(n, bool); live[dead] = False
        tile = np.arange(n) // 64
        holes = (tile % 4 != 1) & (tile % 4 != 2) & (rng.random(n) < 0.3)   # whole tiles empty between partial ones
        tomb = rng.random(n) < 0.5; tomb[dead[:64]] = True                # tombstones inside the set
        masks = {"every": np.ones(n, bool), "tenth": tile % 10 == 3, "half": rng.random(n) < 0.5, "holes": holes, "tombstones": tomb}
        for a in (rows, qs, live, *masks.values()):
            a.setflags(write=False)
        _WIDTH_CASES[dim] = {"rows": rows, "qs": qs, "dead": dead, "live": live, "masks": masks, "state8": B8.RowState8(rows), "stage8": {}}
    return _WIDTH_CASES[dim]


def width_stage8(case, metric, i):
    if (metric, i) not in case["stage8"]:
        case["stage8"][(metric, i)] = W.stage8_of(metric, case["state8"], case["qs"][i])
    return case["stage8"][(metric, i)]


@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
@pytest.mark.parametrize("dim", [16, 48, 496, 768])
def test_rows_and_bits_of_the_exact_filtered_scan_and_the_survivor_count(metric, dim):
    """48 = 3 steps (the 2- and 1-step blocks), 496 = 31 steps (16 + 8 + 4 + 2 + 1), a ragged last tile, several workgroups; stage 1's
    survivor count is the CPU model's over live & mask"""
    case = width_case(dim)
    idx = build(case, metric)
    for j, (name, mask) in enumerate(case["masks"].items()):
        rs = idx.rowset(mask)
        alive = case["live"] & mask
        for k in (1, 10, 63, 64):
            i = (j + k) & 1
            q = case["qs"][i]
            (r, d, c), inc = both(idx, lambda: idx.search_rowsets(q[None, :], k, [rs]))
            assert answered_by_the_8bit_stage(inc), (name, k, inc)
            assert k <= inc["cand8"] <= 4096 and inc["cand"] == inc["cand8"], (name, k, inc)
            assert inc["cand8"] == B.decide(width_stage8(case, metric, i), k, alive=alive)["count"], (name, k, inc)
            if k in (10, 64):
                assert agrees(metric, case["rows"], q, k, alive, r[0], d[0], c[0]), (name, k)
    idx.close()


# ---- 2. every entry point ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
def test_every_entry_point_with_one_query(metric):
    import torch
    case = F.masked(metric)
    idx = build(case, metric)
    n, k = F.N, 10
    q = case["qs"][0]
    rng = np.random.default_rng(8200)
    vals = rng.random(n)
    mask = vals < 0.4
    col = idx.column("f64"); col.set(0, vals)
    filt = [(col, "lt", 0.4)]
    rs = idx.rowset(mask)
    alive = case["live"] & mask
    results = []
    for name, call in (("masked", lambda: idx.search_masked(q, k, mask)), ("rowsets", lambda: idx.search_rowsets(q[None, :], k, [rs])),
                       ("where", lambda: idx.search_where(q[None, :], k, filt))):
        (r, d, c), inc = both(idx, call)
        assert answered_by_the_8bit_stage(inc), (name, inc)
        assert agrees(metric, case["rows"], q, k, alive, r[0], d[0], c[0]), name
        results.append((r, d))
    for r, d in results[1:]:
        assert np.array_equal(r, results[0][0]) and d.tobytes() == results[0][1].tobytes()
    # the device-pointer forms behind queued work on a caller's stream
    idx.set_bound_scan("always"); idx.set_bound_plane_filtered("8bit")
    st = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device="cuda")
    for name in ("rowsets_device", "where_device"):
        out_r = torch.empty((1, k), dtype=torch.int32, device="cuda"); out_d = torch.empty((1, k), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        a0, b0 = idx.bound_scan8_stats(), idx.bound_scan_stats()
        with torch.cuda.stream(st):
            for _ in range(8):
                a = a @ a * 1e-3                                          # queued work ahead of the search
            dq = torch.from_numpy(q[None, :].copy()).to("cuda", non_blocking=False)
            if name == "rowsets_device":
                idx.search_rowsets_device(dq.data_ptr(), 1, k, [rs], out_r.data_ptr(), out_d.data_ptr(), st.cuda_stream)
            else:
                idx.search_where_device(dq.data_ptr(), 1, k, filt, out_r.data_ptr(), out_d.data_ptr(), st.cuda_stream)
        st.synchronize()
        a1, b1 = idx.bound_scan8_stats(), idx.bound_scan_stats()
        assert a1["searches"] - a0["searches"] == 1 and a1["hand_backs"] == a0["hand_backs"], (name, a0, a1)
        assert b1["searches"] - b0["searches"] == 1 and b1["hand_backs"] == b0["hand_backs"], (name, b0, b1)
        assert np.array_equal(out_r.cpu().numpy().view(np.uint32), results[0][0]) and out_d.cpu().numpy().tobytes() == results[0][1].tobytes(), name
    idx.close()


# ---- 3. stale lower bounds -------------------------------------------------------------------------------------------------------------------
def test_a_skipped_tile_holds_no_earlier_searchs_bounds():
    metric = B.COSINE
    case = F.stale(metric)
    idx = build(case, metric)
    k = 10
    for j in range(4):
        idx.set_bound_scan("always"); idx.set_bound_plane("8bit"); idx.set_bound_plane_filtered("8bit")
        a0 = idx.bound_scan8_stats()
        r0, _, _ = idx.search_rowsets(case["qs"][j:j + 1], k, [None])     # unfiltered, same entry, same context: the 8-bit stage, answers in tiles t % 3 != 0
        a1 = idx.bound_scan8_stats()
        assert a1["searches"] - a0["searches"] == 1 and a1["hand_backs"] == a0["hand_backs"]
        assert int(r0[0, 0]) == int(case["at"][j]) and (r0[0, 0] // 64) % 3 != 0
        rs = idx.rowset(case["masks"][j])
        (r, d, c), inc = both(idx, lambda: idx.search_rowsets(case["qs"][j:j + 1], k, [rs]))
        assert answered_by_the_8bit_stage(inc), (j, inc)
        assert ((r[0] // 64) % 3 == 0).all()
        assert agrees(metric, case["rows"], case["qs"][j], k, case["masks"][j], r[0], d[0], c[0]), j
    idx.close()


# ---- 4. a wave whose first owned tile is empty -------------------------------------------------------------------------------------------------
def test_a_wave_whose_first_owned_tile_is_empty():
    metric = B.COSINE
    cus = device_info(0)["cus"]
    case = F.second_tile(metric, cus)
    idx = build(case, metric)
    k = 10
    for j in (0, 1, 3):
        mask = case["masks"][j]
        assert not mask[:64].any()                                        # the first tile of the index is empty under the set
        rs = idx.rowset(mask)
        (r, d, c), inc = both(idx, lambda: idx.search_rowsets(case["qs"][j:j + 1], k, [rs]))
        assert answered_by_the_8bit_stage(inc), (j, inc)
        assert (r[0] // 64 >= 8 * cus).all()
        assert agrees(metric, case["rows"], case["qs"][j], k, mask, r[0], d[0], c[0]), j
    idx.close()


# ---- 5. fewer than k candidates, and none --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
def test_fewer_than_k_candidates_end_in_the_exact_scan(metric):
    case = F.short(metric)
    idx = build(case, metric)
    sets = [idx.rowset(m) for m in case["masks"]]
    k = 10
    for j, n_res in ((1, 0), (3, 5)):
        (r, d, c), inc = both(idx, lambda: idx.search_rowsets(case["qs"][j:j + 1], k, sets[j:j + 1]))
        assert inc["took8"] == 1 and inc["back8"] == 1 and inc["took"] == 1 and inc["back"] == 1, (j, inc)   # no finite threshold in either stage
        assert int(c[0]) == n_res and (r[0, n_res:] == 0xFFFFFFFF).all() and np.isposinf(d[0, n_res:]).all()
        assert agrees(metric, case["rows"], case["qs"][j], k, case["live"] & case["masks"][j], r[0], d[0], c[0]), j
        # the control words are back in their initial state: an ordinary filtered query behind it is answered by the 8-bit stage
        (r, d, c), inc = both(idx, lambda: idx.search_rowsets(case["qs"][0:1], k, sets[0:1]))
        assert answered_by_the_8bit_stage(inc), (j, inc)
        assert agrees(metric, case["rows"], case["qs"][0], k, case["live"] & case["masks"][0], r[0], d[0], c[0])
    idx.close()


# ---- 6. hand-on to the bfloat16 stage ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_near_duplicate_cluster_under_a_set_goes_to_the_bfloat16_stage(metric):
    """tests/test_gpu_bound_scan8.py's cluster (20 000 near-copies at distances spread over [0, 0.035]) under a set that leaves out a few whole
    tiles: the CPU models over live & mask say the 8-bit stage keeps more than the list holds and what the bfloat16 stage does then"""
    rng = np.random.default_rng(5)
    dim, n, k = 64, 20_000, 10
    c = rng.standard_normal(dim); c /= np.linalg.norm(c)
    u = rng.standard_normal((n, dim)); u -= np.outer(u @ c, c); u /= np.linalg.norm(u, axis=1)[:, None]
    dist = np.linspace(0.0, 0.035, n)
    along = (1.0 - dist) if metric == "dot" else np.ones(n)
    rows = (along[:, None] * c[None, :] + np.sqrt(2.0 * dist)[:, None] * u).astype(np.float32)
    q = c.astype(np.float32)
    mid = quiver_amd.metric_id(metric)
    tile = np.arange(n) // 64
    mask = ~np.isin(tile, (0, 3, 4, 17, 100))                             # a few whole tiles left out, the nearest rows' tile among them
    m8 = B8.reference8(mid, B8.RowState8(rows), q, k, alive=mask)
    m16 = B.reference(mid, B.RowState(rows), q, k, alive=mask)
    assert m8["hand_back"] and m8["count"] > B.CAND_CAP, m8["count"]      # the condition: the shape is what it is built to be
    idx = quiver_amd.DeviceIndex(dim, metric); idx.add(rows)
    rs = idx.rowset(mask)
    (r, d, cnt), inc = both(idx, lambda: idx.search_rowsets(q[None, :], k, [rs]))
    assert inc["took8"] == 1 and inc["back8"] == 1 and inc["cand8"] == m8["count"], (inc, m8["count"])
    assert inc["took"] == 1 and inc["back"] == (1 if m16["hand_back"] else 0), (inc, m16["hand_back"])
    if not m16["hand_back"]:
        assert inc["cand"] == m16["count"], (inc, m16["count"])
    assert mask[r[0]].all() and agrees(mid, rows, q, k, mask, r[0], d[0], cnt[0])
    # the control words are back in their initial state: an ordinary query behind it takes the 8-bit stage again
    q2 = rng.standard_normal((1, dim)).astype(np.float32)
    (_, _, _), inc = both(idx, lambda: idx.search_rowsets(q2, k, [rs]))
    assert inc["took8"] == 1 and inc["took"] == 1
    idx.close()


# ---- 7. rows and queries the bound says nothing about ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_undecidable_rows_inside_and_outside_the_set(metric):
    dim, n = 128, 8000
    rng = np.random.default_rng(41)
    extreme = X.class_rows(rng, dim)
    rows = O.gen_rows(8700, 0, n, dim)
    placed = []
    for j, (cls, name, v) in enumerate(extreme):
        rows[(j * 397) % n] = v; placed.append((j * 397) % n)
    placed = np.array(placed)
    unsure = np.isnan(B8.RowState8(rows[placed]).res)
    assert unsure.sum() >= 4
    inside = placed[unsure][0::2]; outside = placed[unsure][1::2]
    mask = np.random.default_rng(8701).random(n) < 0.5
    mask[placed] = True; mask[outside] = False
    idx = quiver_amd.DeviceIndex(dim, metric); idx.add(rows)
    mid = quiver_amd.metric_id(metric)
    rs = idx.rowset(mask)
    q = O.gen_rows(8702, 0, 1, dim)[0]
    state8 = B8.RowState8(rows)
    stage8 = W.stage8_of(mid, state8, q)
    assert stage8["unsure"][inside].all() and stage8["unsure"][outside].all()
    for k in (1, 10, 64):
        (r, d, c), inc = both(idx, lambda: idx.search_rowsets(q[None, :], k, [rs]))
        assert answered_by_the_8bit_stage(inc), (k, inc)
        m = B.decide(stage8, k, alive=mask)
        assert m["passed"][inside].all() and not m["passed"][outside].any()      # the model: inside always survivors, outside never
        assert inc["cand8"] == m["count"] and len(inside) <= inc["cand8"] <= 4096, (k, inc, m["count"])
        assert not np.isin(r[0], outside).any()
        er, ed = O.exact_search(mid, rows, q, k, alive=mask.astype(np.uint8))
        assert np.array_equal(r[0], er) and X.same(d[0], ed)
    for cls, name, v in extreme:                                          # queries neither stage works with go on through both
        _, inc = both(idx, lambda: idx.search_rowsets(v[None, :], 10, [rs]))
        assert inc["took8"] == 1 and inc["took"] == 1
        if cls in "NZ" or name in ("norm2e+18", "norm1e+30"):
            assert inc["back8"] == 1 and inc["back"] == 1, (cls, name, inc)
    idx.close()


# ---- 8. a set made before the index grew ------------------------------------------------------------------------------------------------------
def test_a_set_made_before_the_index_grew():
    metric, dim, n0, n1, k = B.COSINE, 128, 12_000, 20_011, 10
    rows = O.gen_rows(6500, 0, n1, dim).copy()
    qs = O.gen_rows(6501, 0, 4, dim)
    rng = np.random.default_rng(6502)
    idx = quiver_amd.DeviceIndex(dim, "cosine"); idx.add(rows[:n0])
    masks = [np.zeros(n1, bool) for _ in range(4)]
    for j in range(4):
        masks[j][:n0] = rng.random(n0) < (0.5, 0.1, 0.5, 0.02)[j]
    sets = [idx.rowset(m[:n0]) for m in masks]
    idx.add(rows[n0:])                                                    # the sets' words < n_tiles: new rows are unselected
    live = np.ones(n1, bool)

    def check(where):
        for j in range(4):
            (r, d, c), inc = both(idx, lambda: idx.search_rowsets(qs[j:j + 1], k, sets[j:j + 1]))
            assert answered_by_the_8bit_stage(inc), (where, j, inc)
            assert agrees(metric, rows, qs[j], k, live & masks[j], r[0], d[0], c[0]), (where, j)

    check("grown")
    new = np.arange(n0 + 7, n1, 3, dtype=np.uint32)
    sets[0].set_rows(new, True); masks[0][new] = True
    sets[3].set_rows(new[:500], True); masks[3][new[:500]] = True
    check("set_rows")
    gone = np.flatnonzero(masks[0])[:400].astype(np.uint32)
    idx.remove(gone); live[gone] = False
    at = int(np.flatnonzero(masks[1] & live)[5])
    rows[at] = qs[1] * np.float32(1.0 + 1e-6); idx.update(at, rows[at])  # a selected row becomes query 1's nearest
    check("remove and update")
    idx.close()


# ---- 9. modes ----------------------------------------------------------------------------------------------------------------------------------
def test_the_two_plane_setters_are_independent():
    metric = B.COSINE
    case = F.masked(metric)
    idx = build(case, metric)
    k, q, mask = 10, case["qs"][0], case["masks"][0]
    rs = idx.rowset(mask)

    def run(call):
        a0, b0 = idx.bound_scan8_stats(), idx.bound_scan_stats()
        out = call()
        a1, b1 = idx.bound_scan8_stats(), idx.bound_scan_stats()
        return out, a1["searches"] - a0["searches"], b1["searches"] - b0["searches"]

    idx.set_bound_scan("always")
    want = O.exact_search(metric, case["rows"], q, k, alive=(case["live"] & mask).astype(np.uint8))
    # the unfiltered setter alone leaves a filtered search on the bfloat16 copy
    idx.set_bound_plane("8bit"); idx.set_bound_plane_filtered("auto")
    (r, d, c), took8, took = run(lambda: idx.search_rowsets(q[None, :], k, [rs]))
    assert (took8, took) == (0, 1) and r[0].tolist() == want[0].tolist()
    # the filtered setter leaves an unfiltered search's plane choice alone
    for plane, n8 in (("bf16", 0), ("8bit", 1)):
        idx.set_bound_plane(plane); idx.set_bound_plane_filtered("8bit")
        _, took8, took = run(lambda: idx.search(q, k))
        assert (took8, took) == (n8, 1), plane
        idx.set_bound_plane_filtered("bf16")
        _, took8, took = run(lambda: idx.search(q, k))
        assert (took8, took) == (n8, 1), plane
    # "bf16" never counts an 8-bit search, whatever the unfiltered setter says
    idx.set_bound_plane("8bit"); idx.set_bound_plane_filtered("bf16")
    for call in (lambda: idx.search_rowsets(q[None, :], k, [rs]), lambda: idx.search_masked(q, k, mask)):
        (r, d, c), took8, took = run(call)
        assert (took8, took) == (0, 1) and r[0].tolist() == want[0].tolist() and d[0].tobytes() == want[1].tobytes()
    # shared passes of 2 and 4 queries stay on the bfloat16 copy
    idx.set_bound_plane_filtered("8bit")
    for nq in (2, 4):
        (r, d, c), took8, took = run(lambda: idx.search_rowsets(case["qs"][:nq], k, [rs] * nq))
        assert (took8, took) == (0, nq), nq
        assert r[0].tolist() == want[0].tolist() and d[0].tobytes() == want[1].tobytes()
    idx.close()


def test_an_index_without_the_plane_runs_on_the_copy_or_exactly():
    rows = O.gen_rows(88, 0, 5000, 128)
    mask = np.random.default_rng(8900).random(5000) < 0.5
    want = O.exact_search(0, rows, rows[3], 10, alive=mask.astype(np.uint8))
    for make in ("flag", "oom8"):
        if make == "oom8":
            os.environ["QV_TEST_PLANE8_OOM"] = "1"                         # the 8-bit plane's allocation answers out-of-memory: not an error
        try:
            idx = quiver_amd.DeviceIndex(128, "cosine", scan_plane=make != "flag")
            idx.add(rows)
        finally:
            os.environ.pop("QV_TEST_PLANE8_OOM", None)
        assert not idx.bound_scan8_stats()["plane"] and idx.bound_scan_stats()["plane"] == (make == "oom8")
        rs = idx.rowset(mask)
        (r, d, c), inc = both(idx, lambda: idx.search_rowsets(rows[3][None, :], 10, [rs]))
        assert inc["took8"] == 0 and inc["took"] == (1 if make == "oom8" else 0) and inc["back"] == 0, (make, inc)
        assert r[0].tolist() == want[0].tolist() and d[0].tobytes() == want[1].tobytes()
        idx.close()


CHILD = r"""
import json, sys
import numpy as np
import quiver_amd
from quiver_amd import _lib
from quiver_amd.device_index import device_info
from tests import _oracle as O
n, dim, k = 20011, 128, 10
idx = quiver_amd.DeviceIndex(dim, "cosine"); idx.add(O.gen_rows(8950, 0, n, dim))
q = O.gen_rows(8951, 0, 1, dim)
mask = (np.arange(n) // 64) % 10 == 0
rs = idx.rowset(mask)
idx.set_bound_scan("always"); idx.set_bound_plane_filtered("8bit")
sys.stderr.write("@@BEGIN\n"); sys.stderr.flush()
r, d, c = idx.search_rowsets(q, k, [rs])
sys.stderr.write("@@END\n"); sys.stderr.flush()
a, b = idx.bound_scan8_stats(), idx.bound_scan_stats()
tiles = (n + 63) // 64
ct = int(np.unique(np.flatnonzero(mask) // 64).size)
route = _lib.lib().qv_scan_route_ex(0, dim, n, 1, k, device_info(0)["cus"], 1, 1, 0, 1, 1, ct, 1)
old = _lib.lib().qv_scan_route(0, dim, n, 1, k, device_info(0)["cus"], 1, 1, 0, 1, 1, ct)
print("@@JSON " + json.dumps({"tiles": tiles, "ct": ct, "route": route, "old": old, "took8": a["searches"], "took": b["searches"], "back": b["hand_backs"], "rows": r[0].tolist()}))
"""


def test_the_trace_line_and_the_route_of_the_filtered_8bit_call():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", CHILD], env=dict(os.environ, QV_TRACE="1"), capture_output=True, text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stderr[-4000:]
    got = json.loads(next(l for l in p.stdout.splitlines() if l.startswith("@@JSON "))[len("@@JSON "):])
    err = p.stderr
    lines = [l for l in err[err.index("@@BEGIN"):err.index("@@END")].splitlines() if l.startswith("qv: scan kernel")]
    assert lines == ["qv: scan kernel = k_bound_scan8 masked + k_bound_collect + k_bound_rescore, then gated k_bound_scan masked + k_bound_collect + k_bound_rescore "
                     "(tiles=%u, candidate tiles<=%u, k=%u)" % (got["tiles"], got["ct"], 10)], lines
    assert got["route"] == R.BOUND8_FIRST and got["old"] == R.BOUND      # qv_scan_route_ex names the route that ran
    assert got["took8"] == 1 and got["took"] == 1 and got["back"] == 0
    assert all((r // 64) % 10 == 0 for r in got["rows"])


# ---- 10. concurrent callers ------------------------------------------------------------------------------------------------------------------
def test_concurrent_callers_with_their_own_sets():
    """eight threads, each with its own row set: a caller that ran alone took the 8-bit stage, callers put together shared a bfloat16 pass;
    every answer is the oracle's over its own live & set, and the hand-ons and hand-backs are the CPU models' (none here, asserted first)"""
    n, dim, k, callers, each = 30_000, 128, 10, 8, 12
    idx = quiver_amd.DeviceIndex(dim, "cosine"); idx.add_synthetic(6900, 0, n)
    rows = O.gen_rows(6900, 0, n, dim)
    qs = O.gen_rows(6901, 0, callers, dim)
    rng = np.random.default_rng(6902)
    masks = [rng.random(n) < (0.5, 0.2, 0.05, 1.0)[j % 4] for j in range(callers)]
    sets = [idx.rowset(m) for m in masks]
    want = [O.exact_search(B.COSINE, rows, qs[j], k, alive=masks[j].astype(np.uint8)) for j in range(callers)]
    state, state8 = B.RowState(rows), B8.RowState8(rows)
    for j in range(callers):                                              # the models: neither stage hands any of these queries on
        assert not B.reference(B.COSINE, state, qs[j], k, alive=masks[j])["hand_back"], j
        assert not B.decide(W.stage8_of(B.COSINE, state8, qs[j]), k, alive=masks[j])["hand_back"], j
    idx.set_bound_scan("always"); idx.set_bound_plane_filtered("8bit")
    a0, s0, c0 = idx.bound_scan8_stats(), idx.bound_scan_stats(), idx.rowset_coalesce_stats()
    bad = []
    start = threading.Barrier(callers)

    def caller(j):
        start.wait()
        for _ in range(each):
            r, d, c = idx.search_rowsets(qs[j:j + 1], k, sets[j:j + 1])
            if int(c[0]) != k or r[0].tolist() != want[j][0].tolist() or d[0].tobytes() != want[j][1].tobytes():
                bad.append(j)

    ts = [threading.Thread(target=caller, args=(j,)) for j in range(callers)]
    [t.start() for t in ts]; [t.join() for t in ts]
    a1, s1, c1 = idx.bound_scan8_stats(), idx.bound_scan_stats(), idx.rowset_coalesce_stats()
    assert not bad, bad
    alone = c1["solo"] - c0["solo"]                                       # calls that ran alone (a group of one among them)
    shared = c1["group_queries"] - c0["group_queries"]                    # calls that shared a pass of 2 - 8
    assert alone + shared == callers * each, (c0, c1)
    assert s1["searches"] - s0["searches"] == callers * each, (s0, s1)    # every call took the bound scan
    assert a1["searches"] - a0["searches"] == alone, (a0, a1, alone)      # and exactly the calls that ran alone started on the 8-bit plane
    assert a1["hand_backs"] == a0["hand_backs"] and s1["hand_backs"] == s0["hand_backs"], (a0, a1, s0, s1)
    idx.close()
