"""The inputs of tests/test_gpu_busy_streams.py keep their promises, without a device: every decoy is an ordinary valid input, a stale
read of it could not pass for the true input, and the flat cases reach every route."""
import numpy as np
import pytest

import quiver_amd
from tests import _busy as B, _route as R

CASES = B.all_cases()


def test_case_names_are_unique():
    names = [c.name for c in CASES]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_decoys_are_valid_and_a_stale_read_of_one_cannot_pass(case):
    true, decoy = case.true(), case.decoy()
    assert len(true) == len(decoy)
    for t, d in zip(true, decoy):
        assert t.shape == d.shape and t.dtype == d.dtype and not np.array_equal(t, d)
    assert case.valid(true) and case.valid(decoy)                 # finite, ordinary magnitudes, every row id a row of the index
    ft, fd = case.first(true), case.first(decoy)
    assert len(ft) == len(fd) >= 1
    same = [q for q, (a, b) in enumerate(zip(ft, fd)) if a == b]
    assert not same, "queries whose decoy has the true input's first result: %s" % same


def test_the_graph_edit_changes_every_query_s_answer():
    """the traversal enqueued before the edit and the one after it must be told apart: the edit removes every query's nearest node"""
    case = next(c for c in B.graph_cases() if c.graph == "edit")
    h = B.edit_oracle()
    pre = case.expect(case.true(), h)
    for node in B.edit_removed(pre):
        h.delete(node)
    h.insert_batch(B.edit_rows()[B.EDIT_N:B.EDIT_N + 1])
    post = case.expect(case.true(), h)
    assert all(int(a[0][0]) != int(b[0][0]) for a, b in zip(pre, post))
    assert h.node_level(B.EDIT_N) == int(B.edit_levels()[B.EDIT_N])   # the level the device insert is given is the one the oracle drew


def test_the_flat_cases_reach_every_route():
    routes = {c.name: B.flat_route(c, cus=256) for c in B.flat_cases(256) if c.k <= 64}
    assert routes == B.FLAT_ROUTES
    assert set(routes.values()) == set(range(len(R.ROUTES)))
    for kind, want in (("bound", {R.BOUND}), ("bound_mq", {R.BOUND_MQ}), ("bound8_first", {R.BOUND8_FIRST}), ("small", {R.SMALL}), ("mq", {R.MQ}),
                       ("bound+bound_mq", {R.BOUND, R.BOUND_MQ})):
        assert {B.flat_route(c, cus=256) for c in B.interleaved_cases(kind)} == want, kind


def test_the_filtered_batch_rule_takes_the_40_query_row_set_call():
    """qv_batched_applies_filtered, the library's own rule, under "always": yes on the batched corpus, no on one row fewer.  (That this
    corpus is also the smallest qv_index_search_batched_device takes is a statement about the device entry point, which has no rule export:
    tests/test_gpu_busy_streams.py::test_search_batched_device_refuses_one_row_fewer proves it, nothing here does.)"""
    fb = B.filtered_batch_case()
    assert fb.n == B.BATCHED_ROWS <= 120_000
    assert quiver_amd.batched_applies_filtered(fb.metric, fb.dim, fb.n, fb.nq, fb.k, "auto", "always")
    assert not quiver_amd.batched_applies_filtered(fb.metric, fb.dim, fb.n - 1, fb.nq, fb.k, "auto", "always")
