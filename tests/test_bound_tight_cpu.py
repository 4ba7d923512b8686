"""The CPU side of tests/test_gpu_bound_scan_tight.py: every planted case (tests/_tight.py) must DISCRIMINATE before it is worth running on
a device — with the oracle and the library's own interval function (qv_scan_bound_interval), r* is the oracle's k-th neighbour, survives
stage 1 with the residual the reference computes, is rejected with that residual 10 % short, and the survivors fit the candidate list.
A construction that stops discriminating (another gamma, another margin) fails here first.  And the worst-rounding corpus must be one the
bound decides: the reference predicts a hand-back for the whole-denormal query only."""
import numpy as np
import pytest

from tests import _bound as B
from tests import _tight as T


@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
@pytest.mark.parametrize("dim", T.PLANTED_DIMS)
@pytest.mark.parametrize("k", T.PLANTED_KS)
def test_planted_case_discriminates(metric, dim, k):
    planted_case_discriminates(metric, dim, k)


@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
@pytest.mark.parametrize("dim,k", T.PLANTED_WIDE)
def test_planted_case_discriminates_at_wider_rows(metric, dim, k):
    planted_case_discriminates(metric, dim, k)


def test_no_planted_case_at_the_widest_rows():
    """at 4096 dimensions gamma alone is wider than the room a residual 10 % short leaves (tests/_tight.py): the construction says so
    instead of returning a case that proves nothing"""
    for metric in (B.COSINE, B.DOT):
        with pytest.raises(AssertionError, match="competitors that discriminate"):
            T.planted(metric, 4096, 10)


def planted_case_discriminates(metric, dim, k):
    case = T.planted(metric, dim, k)
    n = len(case["rows"])
    assert 4000 <= n <= 8000 and n % 64 != 0
    er, ed, count = T.conditions(case)
    print("metric %d dim %d k %d: %d rows, %d survivors in the reference" % (metric, dim, k, n, count))
    # the same with the row that an update will overwrite still alive elsewhere, and with rows removed: the conditions hold on the live rows
    alive = np.ones(n, bool); alive[case["ordinary"]] = False
    T.conditions(case, alive)


def test_the_margin_is_needed_in_full():
    """what makes the case tight: q.rh of r* is short of q.r by |q||r - rh| to within a thousandth of it (on an ordinary row the
    shortfall is about 1 / sqrt(dim) of that)"""
    for metric in (B.COSINE, B.DOT):
        case = T.planted(metric, 768, 10)
        q, r = case["q"], case["rows"][case["target"]]
        rh = B.bf16(r)
        true = float(q.astype(np.float64) @ r.astype(np.float64))
        full = B.chain_norm(q) * float(B.residual_up(r, rh))
        assert 0.999 * full <= true - float(q.astype(np.float64) @ rh.astype(np.float64)) <= full
        o = case["rows"][case["ordinary"]]
        assert abs(float(q.astype(np.float64) @ (o.astype(np.float64) - B.bf16(o).astype(np.float64)))) < 0.2 * B.chain_norm(q) * float(B.residual_up(o, B.bf16(o)))


@pytest.mark.parametrize("metric", [B.COSINE, B.DOT])
@pytest.mark.parametrize("dim", [128, 768])
def test_worst_rounding_corpus_is_one_the_bound_decides(metric, dim):
    rows, qs = T.worst_rounding(dim)
    assert len(rows) % 64 != 0
    for k in (10, 64):
        ref = T.worst_rounding_reference(metric, dim, k)
        print("metric %d dim %d k %d: survivors per query %s" % (metric, dim, k, [c for c, _ in ref]))
        assert [hb for _, hb in ref] == [False] * 7 + [True]
        assert all(k <= c <= B.CAND_CAP for c, _ in ref[:7])
