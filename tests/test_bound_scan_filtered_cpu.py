"""The bound scan under filters, without a GPU: the dispatch rule (qv_scan_bound_applies_filtered) and, for the exact inputs of the GPU
cases (tests/_bound_filtered.py: same seeds, same sets), what tests/_bound.py's model says over alive = live & set — which queries have a
threshold H, how many rows survive it, and therefore how many hand-backs tests/test_gpu_bound_scan_filtered.py must see."""
import itertools

import numpy as np
import pytest

import quiver_amd
from quiver_amd import _lib
from quiver_amd.device_index import scan_bound_applies_filtered
from tests import _bound as B
from tests import _bound_filtered as F
from tests import _oracle as O

COSINE, L2, DOT = quiver_amd.metric_id("cosine"), quiver_amd.metric_id("l2"), quiver_amd.metric_id("dot")
AUTO, ALWAYS, NEVER = 0, 1, 2
GRID = list(itertools.product((COSINE, DOT), (16, 128, 768, 4096), (600, 20_011, 300_000, 1_000_000, 10_000_000), (1, 2, 4, 5, 8), (1, 10, 64)))


def filtered(metric, dim, rows, nq, k, mode, has_plane=1, tiles=None):
    tiles = (rows + 63) // 64 if tiles is None else tiles
    rc = _lib.lib().qv_scan_bound_applies_filtered(metric, dim, rows, nq, k, mode, has_plane, tiles)
    assert rc in (0, 1), rc
    return bool(rc)


def plain(metric, dim, rows, nq, k, mode, has_plane=1):
    rc = _lib.lib().qv_scan_bound_applies(metric, dim, rows, nq, k, mode, has_plane)
    assert rc in (0, 1), rc
    return bool(rc)


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def test_always_and_never_follow_the_unfiltered_conditions():
    shapes = GRID + [(L2, 128, 1_000_000, 2, 10), (COSINE, 100, 1_000_000, 2, 10), (COSINE, 4112, 1_000_000, 1, 10), (COSINE, 128, 1_000_000, 4, 65),
                     (COSINE, 128, 1_000_000, 4, 0), (COSINE, 128, 400, 4, 10), (COSINE, 128, 1_000_000, 9, 10), (COSINE, 128, 1_000_000, 0, 10),
                     (COSINE, 128, 70_000_000, 8, 10)]
    for metric, dim, rows, nq, k in shapes:
        for plane in (0, 1):
            for tiles in (0, 1, (rows + 63) // 640, (rows + 63) // 64):
                assert filtered(metric, dim, rows, nq, k, ALWAYS, plane, tiles) == plain(metric, dim, rows, nq, k, ALWAYS, plane), (metric, dim, rows, nq, k, plane, tiles)
                assert not filtered(metric, dim, rows, nq, k, NEVER, plane, tiles)
    assert filtered(COSINE, 128, 20_011, 4, 10, ALWAYS) and not filtered(COSINE, 128, 20_011, 9, 10, ALWAYS)


def test_automatic_mode_never_goes_below_the_unfiltered_floors():
    for metric, dim, rows, nq, k in GRID:
        n_tiles = (rows + 63) // 64
        assert not filtered(metric, dim, rows, nq, k, AUTO, 1, 0)        # no candidate: nothing to scan
        for tiles in (1, n_tiles // 10, n_tiles // 2, n_tiles):
            if filtered(metric, dim, rows, nq, k, AUTO, 1, tiles):
                assert plain(metric, dim, rows, nq, k, AUTO), (metric, dim, rows, nq, k, tiles)
    assert not filtered(COSINE, 768, 165_037, 4, 10, AUTO)                # (tests/test_gpu_rowsets.py asserts k_rowset_scan_mq there)
    assert not filtered(COSINE, 128, 20_011, 4, 10, AUTO)


def test_automatic_mode_takes_the_measured_cells_and_declines_the_measured_losses():
    """profiles/LAB_r09_bound_scan_filtered.md, 768 dimensions; tiles as the HOST counts them (a pass: min(tiles, the sum over its queries))"""
    def auto(rows, nq, k, frac):
        t = (rows + 63) // 64
        return filtered(COSINE, 768, rows, nq, k, AUTO, 1, int(t * frac)) and filtered(DOT, 768, rows, nq, k, AUTO, 1, int(t * frac))
    for k in (10, 64):
        assert auto(300_000, 1, k, 1.0) and auto(300_000, 1, k, 0.48) and auto(1_000_000, 1, k, 0.11) and auto(10_000_000, 1, k, 0.1)
        assert not filtered(COSINE, 768, 299_999, 1, k, AUTO) and not auto(1_000_000, 1, k, 0.05)      # sparser than anything measured
        for nq in (2, 3, 4):
            assert not auto(300_000, nq, k, 1.0) and not auto(999_999, nq, k, 1.0)                   # losses at 300 k
            assert auto(1_000_000, nq, k, 1.0) and auto(1_000_000, nq, k, 0.94)
            assert not auto(1_000_000, nq, k, 0.4) and not auto(1_000_000, nq, k, 0.2)               # striped sets at 1M: losses
            assert auto(10_000_000, nq, k, 0.2) and not auto(10_000_000, nq, k, 0.19)
        for nq in (5, 8):
            assert not auto(300_000, nq, k, 1.0)
            assert auto(1_000_000, nq, k, 1.0) == (k == 10)                                           # k = 64 at 1M: a loss with one sparse set for all
            assert not auto(1_000_000, nq, k, 0.8) and not auto(10_000_000, nq, k, 0.8)               # eight queries naming one striped set: a loss
            assert auto(10_000_000, nq, k, 1.0) and auto(10_000_000, nq, k, 0.9)
    assert not filtered(COSINE, 128, 10_000_000, 1, 10, AUTO) and not filtered(COSINE, 512, 10_000_000, 4, 10, AUTO)   # narrower rows were not measured
    assert filtered(COSINE, 1536, 1_000_000, 4, 10, AUTO)


def test_the_wrapper_and_a_mode_out_of_range():
    assert scan_bound_applies_filtered("cosine", 128, 20_011, 4, 10, "always", True, 313)
    assert not scan_bound_applies_filtered("cosine", 128, 20_011, 4, 10, "never", True, 313)
    assert not scan_bound_applies_filtered("l2", 128, 20_011, 4, 10, "always", True, 313)
    assert _lib.lib().qv_scan_bound_applies_filtered(COSINE, 128, 1_000_000, 4, 10, 3, 1, 100) < 0


# ---- the conditions of the GPU cases ---------------------------------------------------------------------------------------------------
def _model_equals_oracle(key, qi, k, alive):
    """the rows the model passes on hold the oracle's answer over `alive` (so the exact re-score of the survivors IS that answer)"""
    m = F.model(key, qi, k, alive)
    er, ed = F.oracle(key, qi, k, alive)
    if not m["hand_back"]:
        assert m["passed"][er].all() and len(er) == k
        c = F.CASES[key[0]](*key[1:])
        metric = c["metric"] if "metric" in c else key[1]
        rows = np.flatnonzero(m["passed"])
        d = O.all_distances(metric, c["rows"][rows], c["qs"][qi])
        order = np.lexsort((rows, d))[:k]
        assert rows[order].tolist() == er.tolist() and d[order].tobytes() == ed.tobytes()
    return m


@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
@pytest.mark.parametrize("dim", [16, 48, 128, 768])
def test_basic_shapes_hand_nothing_back(metric, dim):
    case = F.basic(metric, dim)
    key = ("basic", metric, dim)
    for j in range(8):
        alive = F.alive_of(case["live"], case["masks"][j])
        assert int(alive.sum()) >= 64, (j, int(alive.sum()))
        for k in F.KS:
            m = F.model(key, j, k, alive)
            assert m["H"] is not None and k <= m["count"] <= B.CAND_CAP and not m["hand_back"], (j, k, m["count"])
        _model_equals_oracle(key, j, 10, alive)
    for nq in F.NQS:
        for k in F.KS:
            assert F.backs(key, nq, k) == 0


@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
def test_short_sets_have_no_threshold(metric):
    case = F.short(metric)
    key = ("short", metric)
    ms = [_model_equals_oracle(key, j, 10, case["live"] & case["masks"][j]) for j in range(4)]
    assert [m["H"] is None for m in ms] == [False, True, False, True]
    assert int((case["live"] & case["masks"][1]).sum()) == 0 and int((case["live"] & case["masks"][3]).sum()) == 5
    assert F.backs(key, 4, 10) == 2
    assert F.backs(key, 4, 10, [case["masks"][0], case["masks"][2], case["masks"][0], case["masks"][2]]) == 0
    for j, n_res in ((1, 0), (3, 5)):
        assert len(F.oracle(key, j, 10, case["live"] & case["masks"][j])[0]) == n_res


def test_stale_case_answers_lie_outside_the_stripe():
    case = F.stale(B.COSINE)
    key = ("stale", B.COSINE)
    for j in range(4):
        er, _ = F.oracle(key, j, 10, case["live"])
        assert er[0] == case["at"][j] and (er[0] // 64) % 3 != 0
        m = _model_equals_oracle(key, j, 10, case["masks"][j])
        assert not m["hand_back"]
        assert not F.model(key, j, 10, case["live"])["hand_back"]         # the unfiltered search in front takes the bound scan too
    assert F.backs(key, 1, 10) == 0 and F.backs(key, 4, 10) == 0


def test_second_tile_case_hands_nothing_back():
    case = F.second_tile(B.COSINE)
    key = ("second_tile", B.COSINE)
    for j in (0, 3, 7):
        m = _model_equals_oracle(key, j, 10, case["masks"][j])
        assert not m["hand_back"]
    for nq in (1, 4, 8):
        assert F.backs(key, nq, 10) == 0


@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
def test_masked_case_hands_nothing_back(metric):
    case = F.masked(metric)
    key = ("masked", metric)
    for m in case["masks"]:
        for nq in (1, 4, 8):
            assert F.backs(key, nq, 10, [m] * 8) == 0
        _model_equals_oracle(key, 7, 10, case["live"] & m)


@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
def test_the_centre_query_overflows_within_its_set(metric):
    case = F.clusters(metric)
    key = ("clusters", metric)
    ms = [F.model(key, j, 10, case["masks"][j]) for j in range(4)]
    assert [m["hand_back"] for m in ms] == [False, True, False, False]
    assert ms[1]["H"] is not None and ms[1]["count"] > B.CAND_CAP         # more than 4096 SELECTED rows within the margin
    assert F.backs(key, 4, 10) == 1
    er, _ = F.oracle(key, 1, 10, case["masks"][1])
    full, _ = F.oracle(key, 1, 10, case["live"])
    assert er.tolist() != full.tolist()                                   # a redo over `alive` instead of alive & set gives another list


@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
@pytest.mark.parametrize("dim", F.TIGHT_DIMS)
@pytest.mark.parametrize("k", F.TIGHT_KS)
def test_the_tight_corpus_stays_tight_under_its_set(metric, dim, k):
    """(a) - (d) of tests/_tight.conditions over alive = the set: r* is the k-th neighbour, H is the best competitor's upper bound, r*
    survives it with the reference's residual and not with one 10 % short — and again with the best competitor left out of the set, where H
    is the NEXT competitor's upper bound.  The ordinary queries beside it are not handed back either: `back == 0` for the whole pass."""
    tight_corpus_stays_tight_under_its_set(metric, dim, k)


@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
@pytest.mark.parametrize("dim,k", F.TIGHT_WIDE)
def test_the_tight_corpus_stays_tight_under_its_set_at_wider_rows(metric, dim, k):
    tight_corpus_stays_tight_under_its_set(metric, dim, k)


def tight_corpus_stays_tight_under_its_set(metric, dim, k):
    from tests import _tight as T
    t = F.tight(metric, dim, k)
    case = t["case"]
    er, ed, count = T.conditions(case, alive=t["exact"])
    assert er[k - 1] == case["target"] and set(er.tolist()) <= set(np.flatnonzero(t["exact"]).tolist()) and count <= int(t["exact"].sum())
    assert t["best"] not in np.flatnonzero(t["omit"]) and len(t["band_omit"]) == len(case["band"]) - 1
    er2, ed2, _ = T.conditions(dict(case, band=t["band_omit"]), alive=t["omit"])
    assert er2[k - 1] == case["target"]
    st = B.RowState(case["rows"])
    ref, ref2 = B.reference(metric, st, case["q"], k, t["exact"]), B.reference(metric, st, case["q"], k, t["omit"])
    assert ref2["H"] >= ref["H"]                                          # (the next competitor's upper bound: never below the best one's)
    for q, m in zip(t["others"], t["other_masks"]):
        r = B.reference(metric, st, q, k, m)
        assert r["H"] is not None and not r["hand_back"] and k <= r["count"] <= B.CAND_CAP
