"""The four wide knobs of the bound scan (65 to 1024 results) stay independent THROUGH THE DISPATCH: with one of them at "always" and the
three others at "never", exactly the call of that knob's form — one query or three, unfiltered or under a mask — takes its wide form (its
search counter moves by the call's queries, the other form's does not move), and every call answers, row for row and bit for bit, what it
answers with all four at "never".  tests/golden/bound_wide_routes.json pins the decision; this pins that the dispatch asks it with each
form's own knob and plane knob."""
import numpy as np
import pytest

import quiver_amd

pytestmark = pytest.mark.gpu

N, DIM, K = 4096, 64, 65                                  # 64 tiles (the kernels need 8); the shortest wide list
KNOBS = ("set_bound_scan_wide", "set_bound_scan_wide_filtered", "set_bound_scan_wide_mq", "set_bound_scan_wide_filtered_mq")
CALLS = ((1, False), (1, True), (3, False), (3, True))    # (queries, masked), in the order of the knob whose form the call is


@pytest.fixture(scope="module")
def bench():
    rng = np.random.default_rng(2901)
    idx = quiver_amd.DeviceIndex(DIM, "cosine")
    idx.add(rng.standard_normal((N, DIM)).astype(np.float32))
    qs = rng.standard_normal((3, DIM)).astype(np.float32)
    mask = np.arange(N) % 2 == 0                          # 2048 candidates: more than K
    call = lambda nq, masked: idx.search_masked(qs[:nq], K, mask) if masked else idx.search(qs[:nq], K)    # noqa: E731
    for knob in KNOBS:
        getattr(idx, knob)("never")
    never = [call(*c) for c in CALLS]
    for r, d, c in never:
        assert (c == K).all() and np.isfinite(d).all()
    return idx, call, never


def searches(idx):
    return idx.bound_scan_wide_stats()["searches"], idx.bound_scan_wide_mq_stats()["searches"]


@pytest.mark.parametrize("plane", ["bf16", "8bit"])
@pytest.mark.parametrize("on", range(4), ids=[k[len("set_bound_scan_"):] for k in KNOBS])
def test_one_knob_moves_one_form(bench, on, plane):
    idx, call, never = bench
    for form in ("", "_filtered", "_mq", "_filtered_mq"):
        idx._set_bound_plane(form, plane)
    for i, knob in enumerate(KNOBS):
        getattr(idx, knob)("always" if i == on else "never")
    try:
        for i, (nq, masked) in enumerate(CALLS):
            s0 = searches(idx)
            r, d, c = call(nq, masked)
            s1 = searches(idx)
            moved = (s1[0] - s0[0], s1[1] - s0[1])
            want = (0, 0) if i != on else (1, 0) if nq == 1 else (0, nq)
            assert moved == want, (KNOBS[on], plane, nq, masked, moved)
            nr, nd, nc = never[i]
            assert np.array_equal(c, nc) and np.array_equal(r, nr) and np.array_equal(d.view(np.uint32), nd.view(np.uint32)), (KNOBS[on], plane, nq, masked)
    finally:
        for knob in KNOBS:
            getattr(idx, knob)("never")
