"""What tests/test_gpu_filtered_batch_edges.py relies on, proved without a device.

1. The route export (qv_batched_filter_route): which main filter kernel a filtered batch launches, as a table of literals over the shapes the
   GPU tests run — their union is all eight flush variants, so none goes unlaunched — and the export's own argument checks.
2. The inputs of the extreme-value test (tests/_filtered_edges.ExtremeCase) satisfy their conditions by the oracle alone: enough clean
   queries per batch for the counters' cap to pin something, and sets with fewer finite-distance rows than k.
3. The inputs of the order-sensitive test (OrderCase): every set holds enough of its query's planted rows, and they stay nearer than every
   filler in the set.
4. The ragged sets (RaggedCase) are what their names say."""
import ctypes as C

import numpy as np
import pytest

import quiver_amd
from quiver_amd import QvError, _lib, batched_filter_route
from tests import _filtered_edges as E
from tests import _oracle as O
from tests import _order as OR

ALL_EIGHT = {"mfma_f32", "bf16x3", "bf16x3_shared", "bf16rows", "w8x2", "w8x2_padded", "q64_plane", "q64_f32_rows"}

# (filter, dim, the index keeps the bfloat16 copy) -> {queries of a piece: kernel}.  A call of 300 queries is a piece of 256 and one of 44.
# Neither the metric nor k (up to 64) nor the rows (from 32 768 on) change a cell; "auto" is "bf16x1" up to 1536 dimensions.
# Found to reach the three rarer variants: w8x2_padded — the one-term filter with more than 64 queries at 128, 96, 77 or 200 dimensions
# (dimensions whose sixteenths are no multiple of 8, or fewer than 16); bf16x3_shared — "bf16x3" with 129 or more queries, any dimension;
# q64_f32_rows — the one-term filter with up to 64 queries at 768, 256 or 128 dimensions on an index without the bfloat16 copy.
ROUTE = {
    ("bf16x1", 768, False): {36: "q64_f32_rows", 40: "q64_f32_rows", 44: "q64_f32_rows", 100: "w8x2", 256: "w8x2"},
    ("bf16x1", 768, True): {36: "q64_plane", 40: "q64_plane", 44: "q64_plane", 100: "bf16rows", 256: "bf16rows"},
    ("bf16x1", 256, False): {36: "q64_f32_rows", 40: "q64_f32_rows", 44: "q64_f32_rows", 100: "w8x2", 256: "w8x2"},
    ("bf16x1", 256, True): {36: "q64_plane", 40: "q64_plane", 44: "q64_plane", 100: "bf16rows", 256: "bf16rows"},
    ("bf16x1", 128, False): {36: "q64_f32_rows", 40: "q64_f32_rows", 44: "q64_f32_rows", 100: "w8x2_padded", 256: "w8x2_padded"},
    ("bf16x1", 128, True): {36: "q64_plane", 40: "q64_plane", 44: "q64_plane", 100: "w8x2_padded", 256: "w8x2_padded"},
    ("bf16x1", 96, False): {36: "bf16x3", 40: "bf16x3", 44: "bf16x3", 100: "w8x2_padded", 256: "w8x2_padded"},
    ("bf16x1", 77, False): {36: "bf16x3", 40: "bf16x3", 44: "bf16x3", 100: "w8x2_padded", 256: "w8x2_padded"},
    ("bf16x1", 200, False): {36: "bf16x3", 40: "bf16x3", 44: "bf16x3", 100: "w8x2_padded", 256: "w8x2_padded"},
}
for _dim in (768, 256, 128, 96, 77, 200):
    for _plane in (False, True):
        ROUTE[("bf16x3", _dim, _plane)] = {36: "bf16x3", 40: "bf16x3", 44: "bf16x3", 100: "bf16x3", 256: "bf16x3_shared"}
        ROUTE[("fp32", _dim, _plane)] = {36: "mfma_f32", 40: "mfma_f32", 44: "mfma_f32", 100: "mfma_f32", 256: "mfma_f32"}
PADDED = {36: 64, 40: 64, 44: 64, 256: 256}                              # 100: 128 under "bf16x3" and "fp32", 256 under the one-term filter


def route_of(filt, dim, plane, nq):
    """the table's cell; "auto" reads as the one-term filter"""
    return ROUTE[("bf16x1" if filt in ("auto", None) else filt, dim, bool(plane))][nq]


# the shapes each GPU test runs: (dims x index keeps the copy) x filters x pieces
GPU_SHAPES = {
    "every_route": ([(768, False), (768, True), (128, False), (96, False)], ("bf16x1", "bf16x3", "fp32"), (40, 100, 256, 44)),
    "extremes": ([(768, False), (768, True), (128, False), (96, False)], ("auto", "bf16x3", "fp32"), (40, 256)),
    "order": ([(256, False), (256, True), (128, False)], ("auto", "fp32"), (36,)),
    "ragged": ([(128, False)], ("auto",), (40,)),
}


def covered(name):
    shapes, filters, pieces = GPU_SHAPES[name]
    return {route_of(f, d, p, nq) for d, p in shapes for f in filters for nq in pieces}


def test_the_table_is_the_exports_answer_for_every_metric_and_k():
    for (filt, dim, plane), cells in ROUTE.items():
        for nq, want in cells.items():
            for metric in ("cosine", "dot", "l2", "l2sq"):
                for rows, k in ((E.N, 1), (E.N, 10), (E.N, 15), (E.N, 64), (140_043, 32), (1_000_000, 10)):
                    if filt == "fp32" and nq < 32:
                        continue
                    pad, got = batched_filter_route(metric, dim, rows, nq, k, filt, plane)
                    assert got == want, (filt, dim, plane, nq, metric, rows, k, got)
                    assert pad == (PADDED[nq] if nq in PADDED else (256 if filt == "bf16x1" else 128)), (filt, dim, plane, nq, pad)
                    if filt == "bf16x1":
                        assert batched_filter_route(metric, dim, rows, nq, k, "auto", plane) == (pad, got)
                    assert batched_filter_route(metric, dim, rows, nq, k, filt, plane, cus=304) == (pad, got)      # (the CU count sizes grids only)


def test_the_gpu_tests_shapes_reach_all_eight_variants():
    assert covered("every_route") == ALL_EIGHT                           # tests/test_gpu_filtered_batch.py, test 1, asserts the same per metric
    assert covered("every_route") | covered("extremes") | covered("order") | covered("ragged") == ALL_EIGHT
    assert covered("extremes") == ALL_EIGHT                              # every variant also meets the extreme rows and queries
    assert covered("order") == {"q64_f32_rows", "q64_plane", "mfma_f32"}
    assert set(quiver_amd.DeviceIndex.BATCHED_FILTERS) == ALL_EIGHT and len(quiver_amd.DeviceIndex.BATCHED_FILTERS) == 8
    # the three rarer ones, from the candidate shapes
    for dim in (128, 96, 77, 200):
        for nq in (100, 256):
            assert batched_filter_route("cosine", dim, E.N, nq, 10, "bf16x1")[1] == "w8x2_padded", (dim, nq)
    for dim in (768, 128, 96, 77, 200):
        assert batched_filter_route("l2", dim, E.N, 256, 10, "bf16x3")[1] == "bf16x3_shared", dim
        assert batched_filter_route("l2", dim, E.N, 100, 10, "bf16x3") == (128, "bf16x3"), dim
    for dim in (768, 128):
        assert batched_filter_route("dot", dim, E.N, 40, 10, "bf16x1", False) == (64, "q64_f32_rows"), dim
        assert batched_filter_route("dot", dim, E.N, 40, 10, "bf16x1", True) == (64, "q64_plane"), dim


def test_the_export_refuses_what_no_filtered_batch_runs():
    ok = ("cosine", 768, 1_000_000, 40, 10, "auto")
    assert batched_filter_route(*ok)[0] == 64
    for bad in (("cosine", 768, 1_000_000, 8, 10, "auto"),               # fewer than 9 queries
                ("cosine", 768, 1_000_000, 40, 65, "auto"),              # k > 64
                ("cosine", 768, 1_000_000, 40, 0, "auto"),
                ("cosine", 768, 20_000, 64, 10, "auto"),                 # a corpus the batched path leaves to the scans
                ("cosine", 768, 1_000_000, 31, 10, "fp32"),              # the float32 filter starts at 32 queries
                ("l1", 768, 1_000_000, 40, 10, "auto"),
                ("cosine", 768, 1_000_000, 40, 10, "off"),
                ("cosine", 0, 1_000_000, 40, 10, "auto"),
                ("cosine", 768, 0, 40, 10, "auto"),
                ("cosine", 768, 1 << 32, 40, 10, "auto")):
        with pytest.raises(QvError) as e:
            batched_filter_route(*bad)
        assert e.value.code == _lib.QV_ERR_UNSUPPORTED, bad
        # ... and the routing rule agrees wherever it is asked about the same things
        assert not quiver_amd.batched_applies_filtered(bad[0], bad[1], bad[2], bad[3], bad[4], bad[5], "always") or bad[4] == 0, bad
    lib = _lib.lib()
    pad, code = C.c_uint32(0), C.c_int(0)
    assert lib.qv_batched_filter_route(0, 768, 1_000_000, 40, 10, 0, 0, 256, None, C.byref(code)) == _lib.QV_ERR_INVALID_ARG
    assert lib.qv_batched_filter_route(0, 768, 1_000_000, 40, 10, 0, 0, 256, C.byref(pad), None) == _lib.QV_ERR_INVALID_ARG
    assert lib.qv_batched_filter_route(0, 768, 1_000_000, 40, 10, 5, 0, 256, C.byref(pad), C.byref(code)) == _lib.QV_ERR_INVALID_ARG
    assert lib.qv_batched_filter_route(0, 768, 1_000_000, 40, 10, -1, 0, 256, C.byref(pad), C.byref(code)) == _lib.QV_ERR_INVALID_ARG
    assert lib.qv_batched_filter_route(0, 768, 1_000_000, 40, 10, 0, 0, 0, C.byref(pad), C.byref(code)) == _lib.QV_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ 2. extreme rows and queries --
# (e) — every extreme row and five ordinary ones — has fewer finite-distance rows than 64 in these cells, by the oracle; in the other two
# the +-3e38 rows of the "many" regime have finite cosine and dot distances (float64 chains), thousands of them.
E_BELOW_64 = {("cosine", "few"), ("dot", "few"), ("l2", "few"), ("l2sq", "few"), ("l2", "many"), ("l2sq", "many")}


@pytest.mark.parametrize("regime", ["few", "many"])
@pytest.mark.parametrize("dim", [768, 128, 96])
def test_extreme_inputs_keep_their_promises(dim, regime):
    for metric in ("cosine", "dot", "l2", "l2sq"):
        c = E.ExtremeCase(metric, dim, regime)
        n_ext_rows = int(c.extreme.sum())
        assert n_ext_rows == 50 if regime == "few" else n_ext_rows > E.N // 5, (metric, n_ext_rows)
        for nq in (40, 256):
            clean = ~c.touches[:nq]
            assert int(clean.sum()) >= nq // 4, (metric, nq, int(clean.sum()))          # the cap pins at least a quarter of the batch
            assert all(c.kind[p] == "d" and not c.is_ext[p] for p in np.flatnonzero(clean))
            assert int(c.is_ext[:nq].sum()) >= E.EXT_QUERIES                          # every extreme query is in every batch
            assert {c.kind[p] for p in range(nq)} == set(E.KINDS)
            assert {c.kind[p] for p in range(nq) if c.is_ext[p]} == set(E.KINDS)       # ... and meets every kind of set
            assert c.cap(nq) == int(c.touches[:nq].sum()) + int(clean.sum()) // 8 < nq
            for kind in "abcdf":
                assert sum(1 for p in c.probes(nq) if c.kind[p] == kind and not c.is_ext[p]) >= 2, (metric, nq, kind)
        # the extreme queries of a batch are extreme, the ordinary ones and every replacement ordinary and used once
        assert not E.ordinary_rows(c.qs[c.is_ext]).any() and E.ordinary_rows(c.qs[~c.is_ext]).all() and E.ordinary_rows(c.calm).all()
        assert len({q.tobytes() for q in c.calm}) == E.NQ_MAX
        for p in range(E.NQ_MAX):
            m = c.mask[p]
            if c.kind[p] == "d":
                assert not (m & c.extreme).any() and 0.45 < m.sum() / c.ordinary.sum() < 0.55         # half of the ordinary rows, no extreme one
            if c.kind[p] == "e":
                assert (m & c.extreme).sum() == n_ext_rows and int(m.sum()) == n_ext_rows + 5
                assert (c.finite_in_set(p) < 64) or (metric, regime) not in E_BELOW_64, (metric, p, c.finite_in_set(p))
            if c.kind[p] == "g":
                assert c.finite_in_set(p) < 10, (metric, p, c.finite_in_set(p))               # fewer than k at k = 10 and k = 64
                assert c.finite_in_set(p) < int((m & c.live).sum())                              # ... and rows that are not finite beside them
            if c.kind[p] == "f":
                half = int((m & c.extreme).sum())
                assert half == n_ext_rows // 2 and 0.25 < (m & c.ordinary).sum() / c.ordinary.sum() < 0.35
        worst = max(c.finite_in_set(p) for p in range(E.NQ_MAX) if c.kind[p] == "e")
        assert (worst < 64) == ((metric, regime) in E_BELOW_64), (metric, regime, worst)


# ------------------------------------------------------------------------------------------------ 3. order-sensitive rows --
ORDER_CASES = [(m, 256, 9300 + m, 40_000) for m in (OR.COSINE, OR.DOT, OR.L2, OR.L2SQ)] + [(OR.COSINE, 128, 9400, 140_000), (OR.L2, 128, 9401, 140_000)]


@pytest.mark.parametrize("metric,dim,seed,n_fill", ORDER_CASES)
def test_order_inputs_keep_their_promises(metric, dim, seed, n_fill):
    c = E.OrderCase(metric, dim, seed, n_fill)
    assert c.nq == 36 and c.nq * c.n >= 1_000_000                         # a piece the batched path takes, the float32 filter too
    assert sorted(set(c.kind)) == [0, 1, 2, 3]
    for j in range(12):
        assert {c.kind[j + 12 * i] for i in range(3)} == {(j + i) % 4 for i in range(3)}
        assert len(c.duplicates(j)) >= 3                                      # (dup = 3; the planted rows of dot hold an equal pair of their own)
    for p in range(c.nq):
        if c.mask[p] is None:
            continue
        j, m = p % 12, c.mask[p]
        own = c.own[j]
        for k in (10, 32, 40):
            assert int(m[own].sum()) >= min(k, 8), (p, k)
        d = O.all_distances(metric, c.rows, c.qs[p])
        inside = np.zeros(c.n, bool); inside[own] = True
        assert d[inside & m].max() < d[~inside & m].min(), (metric, dim, p)     # _case's separation, restated with the mask
        if c.kind[p] >= 2:                                                     # one copy of each duplicated row inside, the other outside
            lower = 0
            for lo, hi in c.duplicates(j):
                assert m[lo] != m[hi], (p, lo, hi)
                lower += int(m[hi])                                            # (the lower-numbered copy is the one left out)
            assert 0 < lower < len(c.duplicates(j)), (p, lower)                                   # both sides occur: the tie rule cannot be guessed
            assert sorted(c.excluded[p].tolist()) == sorted(lo if not m[lo] else hi for lo, hi in c.duplicates(j))


# ------------------------------------------------------------------------------------------------ 4. ragged sets --
def test_ragged_sets_are_what_they_are_called():
    c = E.RaggedCase()
    old_words, new_words = (E.RAGGED_OLD + 63) // 64, (E.RAGGED_NEW + 63) // 64
    assert E.RAGGED_OLD % 64 == 40 and E.RAGGED_NEW % 64 == 3 and old_words == 516 and new_words == 626
    assert [c.kind[q] for q in range(8)] == list(E.RAGGED_KINDS) and c.nq == 40
    r = np.arange(c.n)
    for q in range(c.nq):
        m, kind = c.mask[q], c.kind[q]
        if c.before[q] or c.where[q]:
            assert not m[E.RAGGED_OLD:].any(), q                            # made before the growth: the new rows are unselected
        if kind == "bit0":
            assert (r[m] % 64 == 0).all() and int(m.sum()) == old_words
        if kind == "bit63":
            assert (r[m] % 64 == 63).all() and int(m.sum()) == old_words - 1
        if kind == "old_last_tile":
            assert m.sum() == 40 and r[m].min() == (old_words - 1) * 64 and r[m].max() == E.RAGGED_OLD - 1
        if kind == "new_last_tile":
            assert m.sum() == 67 and r[m].min() == 39_936 == E.RAGGED_LAST_GROUP == (new_words - 2) * 64
        if kind == "empty":
            assert not m.any()
        if kind == "half_old":
            assert 0.45 < m[:E.RAGGED_OLD].mean() < 0.55
    for q, (add, drop) in c.changed.items():
        assert add.size == 200 and drop.size == 200 and not c.mask[q][add].any() and c.mask[q][drop].all()
        assert (add >= E.RAGGED_OLD).any()                                  # the change reaches rows the set's words did not cover
    after = c.masks_after()
    assert all((after[q] != c.mask[q]).sum() == (400 if q in c.changed else 0) for q in range(c.nq))
    # the bit-0 and bit-63 sets hold 1/64 of the old rows: above the default floor of a hundredth, on the sample too (its first 32 768 rows)
    plan = {"rows": 32_768, "group_step": 1}
    for q in range(c.nq):
        below = E.predicted_sparse(plan, c.n, c.live, [c.mask[q]])
        assert below == (1 if c.kind[q] in ("old_last_tile", "new_last_tile", "empty") else 0), (q, c.kind[q])
