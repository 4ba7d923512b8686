"""The CPU side of tests/test_gpu_bound_scan_widths.py: the cases of tests/_widths.py must be able to tell a right kernel from a wrong one
before they are worth running on a device.  For every width, metric and k the CPU model of stage 1 (tests/_bound.py, tests/_bound8.py over
the library's own interval functions) hands nothing back, keeps between k and the candidate list's size, and its survivors re-scored are
the oracle's answer.  And the sensitivity check: with the contribution of ONE ladder block left out of stage 1's sum — each block size the
width's walk uses, the float32 chain and the integer sum — a survivor count that the device test compares changes, for every form the
device test runs.  The device reports stage 1 through that count alone, so a case whose count could not change would prove nothing.
This is a condition on the inputs (the seeds in tests/_widths.py were chosen for it), not a tolerance."""
import numpy as np
import pytest

from quiver_amd import _lib
from tests import _bound as B
from tests import _bound8 as B8
from tests import _oracle as O
from tests import _widths as W

AUTO, ALWAYS, NEVER = 0, 1, 2
P_8BIT = 1


def test_the_widths_reach_every_block_alone_and_in_company():
    """with 16 (one step) and 128 dimensions (eight) of the existing GPU tests"""
    for ladder, tested_elsewhere in ((W.LADDER, (16, 128)), (W.LADDER8, (16, 128, 768))):
        walks = {dim: [u for u, _, _ in W.blocks(dim, ladder)] for dim in W.WIDTHS + tested_elsewhere}
        for u in ladder:
            assert any(set(w) == {u} for w in walks.values()), (ladder, u, "alone")
            assert any(u in w and len(set(w)) > 1 for dim, w in walks.items() if dim in W.WIDTHS), (ladder, u, "in company")
        assert any(sorted(set(w)) == sorted(ladder) for w in walks.values())                 # the longest ladder: every block in one walk
        assert any(w.count(ladder[0]) > 1 and len(set(w)) > 1 for w in walks.values())       # the loop more than once, then a remainder
    assert [u for u, _, _ in W.blocks(4080, W.LADDER)] == [8] * 31 + [4, 2, 1] and [u for u, _, _ in W.blocks(4080, W.LADDER8)] == [16] * 15 + [8, 4, 2, 1]
    assert [u for u, _, _ in W.blocks(4096, W.LADDER)] == [8] * 32 and [u for u, _, _ in W.blocks(4096, W.LADDER8)] == [16] * 16
    for dim in W.WIDTHS:
        for ladder in (W.LADDER, W.LADDER8):
            b = W.blocks(dim, ladder)
            assert b[0][1] == 0 and b[-1][2] == dim and all(x[2] == y[1] for x, y in zip(b, b[1:]))


def test_the_corpus_shape():
    assert (W.N + 63) // 64 == 33 and W.N % 64 == 3                       # nine workgroups of four waves, a ragged last tile
    for dim in W.WIDTHS:
        c = W.case(dim)
        assert c["rows"].shape == (W.N, dim) and not c["live"][c["dead"]].any() and 30 <= len(c["dead"]) <= 42
        tile = np.arange(W.N) // 64
        assert all(not c["mask"][tile == t].any() for t in range(1, 33, 3))                  # whole tiles without a candidate
        assert not any(m[(tile == 5) | (tile == 20)].any() for m in c["masks"][:4])           # tiles no query of a pass of four selects
        assert c["masks"][6] is None


def _rescored(metric, c, q, m, k):
    rows = np.flatnonzero(m["passed"])
    d = O.all_distances(metric, c["rows"][rows], q)
    order = np.lexsort((rows, d))[:k]
    return rows[order], d[order]


@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
@pytest.mark.parametrize("dim", W.WIDTHS)
def test_the_model_decides_every_case_and_its_survivors_hold_the_answer(metric, dim):
    c = W.case(dim)
    live = c["live"]
    shown = []
    for k in W.KS:
        for j in range(8):
            forms = [("live", live, W.model), ("set", W.alive_of(live, c["masks"][j]), W.model)]
            if j in W.SINGLE:
                forms += [("mask", live & c["mask"], W.model), ("live", live, W.model8)]
            for which, alive, fn in forms:
                m = fn(metric, dim, j, k, alive)
                assert m["H"] is not None and not m["hand_back"], (dim, k, j, which, fn.__name__)
                assert k <= m["count"] <= B.CAND_CAP, (dim, k, j, which, fn.__name__, m["count"])
                er, ed = W.oracle(metric, dim, j, k, which)
                r, d = _rescored(metric, c, c["qs"][j], m, k)
                assert len(er) == k and r.tolist() == er.tolist() and d.tobytes() == ed.tobytes(), (dim, k, j, which, fn.__name__)
        shown.append((k, W.model(metric, dim, 0, k, live)["count"], W.model8(metric, dim, 0, k, live)["count"]))
    print("metric %d dim %d: survivors of query 0 (k, bfloat16, 8-bit) %s" % (metric, dim, shown))
    # the shared sums and the 8-bit intervals restated in tests/_widths.py are the suite's own models
    alive = W.alive_of(live, c["masks"][1])
    ref = B.reference(metric, W.state(dim), c["qs"][1], 10, alive)
    got = W.model(metric, dim, 1, 10, alive)
    assert np.array_equal(ref["s"].view(np.uint32), got["s"].view(np.uint32)) and np.array_equal(ref["passed"], got["passed"]) and ref["H"] == got["H"]
    ref8 = B8.reference8(metric, W.state8(dim), c["qs"][1], 10, live)
    got8 = W.model8(metric, dim, 1, 10, live)
    assert np.array_equal(ref8["passed"], got8["passed"]) and ref8["H"] == got8["H"] and ref8["count"] == got8["count"] and not ref8["hand_back"]


@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
@pytest.mark.parametrize("dim", W.WIDTHS)
def test_every_ladder_block_changes_a_count(metric, dim):
    """one block's contribution left out of stage 1's sum (of the looped block: its last turn) changes a count the device test compares —
    in every form of the float32 walk (the single query, under search_masked, the shared pass's largest, the row sets' largest) and in
    the 8-bit walk"""
    true = W.counts(metric, dim)
    for u, skip in W.left_out(dim, W.LADDER).items():
        got = W.counts(metric, dim, skip)
        for form in true:
            assert got[form] != true[form], (dim, "float32 chain without its %d-step block" % u, skip, form, true[form])
    true8 = W.counts8(metric, dim)
    for u, skip in W.left_out(dim, W.LADDER8).items():
        assert W.counts8(metric, dim, skip) != true8, (dim, "integer sum without its %d-step block" % u, skip, true8)
    assert set(W.left_out(dim, W.LADDER)) == {u for u, _, _ in W.blocks(dim, W.LADDER)}
    assert set(W.left_out(dim, W.LADDER8)) == {u for u, _, _ in W.blocks(dim, W.LADDER8)}


# ---- saturated operands ------------------------------------------------------------------------------------------------------------------
def test_saturated_operands_are_the_largest_sums_and_stay_inside_int32():
    c = W.saturated()
    hi, lo, big = c["hi"], c["lo"], c["big"]
    assert np.array_equal(np.abs(hi[big]), np.full(2048, 127)) and not lo[big].any()
    assert np.array_equal(np.abs(lo[~big]), np.full(2048, 64)) and not hi[~big].any()
    assert np.array_equal(big.reshape(-1, 16)[0], np.array([1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0], bool))   # k_bound_scan8's first partial sum
    for at, s in ((W.SAT_PLUS, 1), (W.SAT_MINUS, -1)):
        for i in at:
            r8, sc, res = B8.quantize_row(c["rows"][i])
            assert np.array_equal(r8.astype(np.int64), s * 127 * c["sign"].astype(np.int64)) and np.isfinite(res)
            r64 = r8.astype(np.int64)
            first, second = int(np.sum(hi[big] * r64[big])), int(np.sum(hi[~big] * r64[~big]))       # the hi term's two partial sums
            third, fourth = int(np.sum(lo[big] * r64[big])), int(np.sum(lo[~big] * r64[~big]))
            assert (first, second, third, fourth) == (s * 2048 * 127 * 127, 0, 0, s * 2048 * 64 * 127)
            assert all(abs(x) < 2 ** 31 for x in (first, second, third, fourth, first + second, third + fourth))
            assert abs(128 * (first + second) + third + fourth) > 2 ** 31                          # ... and their combination is not
    # no row has a larger sum, and the model's is the exact one
    for metric in (B.COSINE, B.DOT):
        st8 = W.saturated_stage8(metric)
        assert int(np.abs(st8["isum"]).max()) == 128 * 2048 * 127 * 127 + 2048 * 64 * 127
        assert sorted(np.argsort(-np.abs(st8["isum"]), kind="stable")[:6].tolist()) == sorted(W.SAT_PLUS + W.SAT_MINUS)
        assert not st8["unsure"][list(W.SAT_PLUS + W.SAT_MINUS)].any()
    d = O.all_distances(B.DOT, c["rows"], c["q"])
    order = np.argsort(d, kind="stable")
    assert order[:3].tolist() == list(W.SAT_PLUS) and order[::-1][:3].tolist() == list(W.SAT_MINUS)  # nearest and farthest under dot, by scale
    for metric in (B.COSINE, B.DOT):
        for k in W.KS:
            for st in (W.saturated_stage8(metric), W.saturated_stage1(metric)):
                m = B.decide(st, k, alive=c["live"])
                assert m["H"] is not None and not m["hand_back"] and k <= m["count"] <= B.CAND_CAP
                er, ed = O.exact_search(metric, c["rows"], c["q"], k, alive=c["live"].astype(np.uint8))
                r, dd = _rescored(metric, c, c["q"], m, k)
                assert r.tolist() == er.tolist() and dd.tobytes() == ed.tobytes()
            assert er[0] == W.SAT_PLUS[0]


# ---- the limit -----------------------------------------------------------------------------------------------------------------------------
def test_the_first_width_above_the_limit_is_declined():
    lib = _lib.lib()
    for metric in (B.COSINE, B.DOT):
        for rows in (W.N, 20_011, 10_000_000):
            for k in W.KS:
                for nq in (1, 2, 4, 8):
                    assert lib.qv_scan_bound_applies(metric, 4112, rows, nq, k, ALWAYS, 1) == 0
                    assert lib.qv_scan_bound_applies(metric, 4096, rows, nq, k, ALWAYS, 1) == 1
                    assert lib.qv_scan_bound_applies(metric, 4080, rows, nq, k, ALWAYS, 1) == 1
                assert lib.qv_scan_bound8_applies(metric, 4112, rows, 1, k, ALWAYS, P_8BIT, 1) == 0
                assert lib.qv_scan_bound8_applies(metric, 4096, rows, 1, k, ALWAYS, P_8BIT, 1) == 1
                assert lib.qv_scan_bound8_applies(metric, 4080, rows, 1, k, ALWAYS, P_8BIT, 1) == 1
