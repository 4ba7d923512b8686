"""Range search on the device against the oracle: every live row with float32 distance <= radius, ordered by (distance, row), for equality —
rows, float32 bits, count, matches and padding — on the exact range scan and on the 8-bit plane's stage in front of it."""
import functools

import numpy as np
import pytest

import quiver_amd
from tests import _oracle as O

pytestmark = pytest.mark.gpu

N, REMOVED, NAN_ROW, ZERO_ROW = 197, (3, 64, 100, 128, 196), 70, 130   # three tiles and a ragged one; a dead row at both ends of a tile
PLANE_METRICS = ("cosine", "dot", "l2")
INF = np.float32(np.inf)


@functools.lru_cache(maxsize=None)
def corpus(dim):
    rows = O.gen_rows(20261127, 0, N, dim)
    rows[NAN_ROW, dim // 2] = np.nan
    rows[ZERO_ROW] = 0.0
    return rows, O.gen_rows(20261128, 0, 5, dim)


@functools.lru_cache(maxsize=None)
def reference(metric, dim):
    """per query: the live rows ordered by (distance, row) and their float32 distances — O.distance over every live row, computed once"""
    rows, qs = corpus(dim)
    m = quiver_amd.metric_id(metric)
    live = np.array([r for r in range(N) if r not in REMOVED], dtype=np.uint32)
    out = []
    for q in qs:
        d = np.array([O.distance(m, q, rows[r]) for r in live], dtype=np.float32)
        d = np.where(d == 0, np.float32(0), d)                          # -0 orders and prints as +0
        order = np.lexsort((live, d))                                   # NaN last, as numpy sorts it
        out.append((live[order], d[order]))
    return out


def make_index(metric, dim, mode):
    rows, _ = corpus(dim)
    idx = quiver_amd.DeviceIndex(dim, metric, device=0, l2_scan_plane=(metric == "l2"))
    idx.add(rows)
    idx.remove(np.array(REMOVED, dtype=np.uint32))
    idx.set_range_plane(mode)
    return idx


def expect(ref_q, radius, max_results):
    r, d = ref_q
    with np.errstate(invalid="ignore"):
        hit = d <= np.float32(radius)
    matches = int(hit.sum())
    count = min(matches, max_results)
    rows = np.full(max_results, 0xFFFFFFFF, dtype=np.uint32)
    dist = np.full(max_results, np.inf, dtype=np.float32)
    rows[:count] = r[hit][:count]
    dist[:count] = d[hit][:count]
    return rows, dist, count, matches


def check(got, ref, radii, max_results):
    rows, dist, count, matches = got
    for q, radius in enumerate(radii):
        er, ed, ec, em = expect(ref[q], radius, max_results)
        assert (int(count[q]), int(matches[q])) == (ec, em), (q, radius)
        assert np.array_equal(rows[q], er), (q, radius)
        assert np.array_equal(dist[q].view(np.uint32), ed.view(np.uint32)), (q, radius)


def radii_for(ref, nq, which):
    tenth = np.array([ref[q][1][9] for q in range(nq)], dtype=np.float32)
    lowest = np.array([ref[q][1][0] for q in range(nq)], dtype=np.float32)
    return {"tenth": tenth, "below_tenth": np.nextafter(tenth, -INF), "none": np.nextafter(lowest, -INF),
            "inf": np.full(nq, np.inf, dtype=np.float32), "nan": np.full(nq, np.nan, dtype=np.float32)}[which]


@pytest.mark.parametrize("nq", [1, 5])
@pytest.mark.parametrize("dim", [64, 100])
@pytest.mark.parametrize("mode", ["never", "always"])
@pytest.mark.parametrize("metric", ["cosine", "dot", "l2", "l1", "l2sq"])
def test_range_matches_the_oracle(metric, mode, dim, nq):
    ref = reference(metric, dim)
    idx = make_index(metric, dim, mode)
    qs = corpus(dim)[1][:nq]
    n_calls = 0
    for which in ("tenth", "below_tenth", "none", "inf", "nan"):
        radii = radii_for(ref, nq, which)
        max_results = 16 if which == "inf" else 64                      # inf: matches > count, the 16 nearest
        check(idx.search_range(qs, radii, max_results), ref, radii, max_results)
        n_calls += 1
    stats = idx.range_stats()
    on_plane = mode == "always" and metric in PLANE_METRICS and dim == 64   # dim 100 keeps no 8-bit plane: the exact kernel under "always" too
    assert stats[0] == n_calls * nq
    assert stats[1] == (n_calls * nq if on_plane else 0) and stats[2] == 0
    assert (stats[3] > 0) == on_plane


@pytest.mark.parametrize("metric", PLANE_METRICS)
def test_range_hand_back(metric, monkeypatch):
    """a candidate buffer of 8 rows: stage 1 overflows for the wide radii, those queries go back to the exact range scan alone, same bits"""
    monkeypatch.setenv("QV_RANGE_CAND_CAP", "8")
    ref = reference(metric, 64)
    idx = make_index(metric, 64, "always")
    qs = corpus(64)[1]
    radii = radii_for(ref, 5, "tenth")
    radii[1] = np.inf
    radii[4] = np.float32(np.nextafter(ref[4][1][0], -INF))            # no match: stays on the plane beside the handed-back ones
    check(idx.search_range(qs, radii, 32), ref, radii, 32)
    stats = idx.range_stats()
    assert stats[1] == 5 and 1 <= stats[2] < 5


@pytest.mark.parametrize("mode", ["never", "always"])
def test_range_more_matches_than_keys(mode):
    """20 000 rows all within the radius: more matches than the key buffer's 16 384, so the query is redone by a key per row and the radix
    selection — the 100 nearest — beside a query whose matches fit"""
    n, dim = 20000, 64
    idx = quiver_amd.DeviceIndex(dim, "cosine", device=0)
    idx.add_synthetic(20260424, 0, n)
    idx.set_range_plane(mode)
    rows = O.gen_rows(20260424, 0, n, dim)
    qs = O.gen_rows(20260425, 0, 2, dim)
    er0, ed0 = O.exact_search(0, rows, qs[0], 100)
    er1, ed1 = O.exact_search(0, rows, qs[1], 100)
    radii = np.array([np.inf, ed1[9]], dtype=np.float32)
    r, d, count, matches = idx.search_range(qs, radii, 100)
    assert count.tolist() == [100, 10] and matches.tolist() == [n, 10]
    assert np.array_equal(r[0], er0) and np.array_equal(d[0].view(np.uint32), ed0.view(np.uint32))
    assert np.array_equal(r[1, :10], er1[:10]) and np.array_equal(d[1, :10].view(np.uint32), ed1[:10].view(np.uint32))
    assert (r[1, 10:] == 0xFFFFFFFF).all() and np.isinf(d[1, 10:]).all()


def test_range_device_form_on_a_stream():
    import torch
    ref = reference("cosine", 64)
    idx = make_index("cosine", 64, "always")
    qs = corpus(64)[1]
    radii = radii_for(ref, 5, "tenth")
    host = idx.search_range(qs, radii, 16)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dq, dr = torch.from_numpy(qs).cuda(), torch.from_numpy(radii).cuda()
        rows = torch.zeros((5, 16), dtype=torch.int32, device="cuda")
        dist = torch.zeros((5, 16), dtype=torch.float32, device="cuda")
        matches = torch.zeros(5, dtype=torch.int64, device="cuda")
        idx.search_range_device(dq.data_ptr(), 5, dr.data_ptr(), 16, rows.data_ptr(), dist.data_ptr(), matches.data_ptr(), st.cuda_stream)
    st.synchronize()
    assert np.array_equal(rows.cpu().numpy().view(np.uint32), host[0])
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), host[1].view(np.uint32))
    assert np.array_equal(matches.cpu().numpy().astype(np.uint64), host[3])


def test_range_arguments_and_an_empty_index():
    idx = quiver_amd.DeviceIndex(64, "cosine", device=0)
    q = corpus(64)[1][:2]
    rows, dist, count, matches = idx.search_range(q, 1.0, 4)
    assert count.tolist() == [0, 0] and matches.tolist() == [0, 0] and (rows == 0xFFFFFFFF).all() and np.isinf(dist).all()
    idx.add(corpus(64)[0])
    for bad in (0, 8193):
        with pytest.raises(quiver_amd.QvError):
            idx.search_range(q, 1.0, bad)
    with pytest.raises(quiver_amd.QvError):
        idx.set_range_plane(3)
