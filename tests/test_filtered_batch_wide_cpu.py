"""qv_batched_applies_filtered_wide: the dispatch's rule for filtered batches of 9+ queries at 65 to 1024 results, asked on the host without an
index or a device.  (That a search then does what the rule says is asserted on the GPU, through the counters: tests/test_gpu_filtered_batch_wide.py.)"""
import pytest

from quiver_amd import batched_applies_filtered, batched_applies_filtered_wide

SHAPES = [(m, d, r) for m in ("cosine", "dot", "l2", "l2sq") for d, r in ((64, 140_003), (768, 1_000_000))]


@pytest.mark.parametrize("metric,dim,rows", SHAPES)
def test_rule(metric, dim, rows):
    for nq in (9, 70, 256, 300):
        for k in (65, 128, 1000, 1024):
            assert batched_applies_filtered_wide(metric, dim, rows, nq, k, mode="always")
            assert not batched_applies_filtered(metric, dim, rows, nq, k, mode="always")      # the sibling keeps saying no above 64
            for mode in ("never", "auto"):
                assert not batched_applies_filtered_wide(metric, dim, rows, nq, k, mode=mode)
            assert not batched_applies_filtered_wide(metric, dim, rows, nq, k, "off", "always")
            took = [batched_applies_filtered_wide(metric, dim, rows, nq, k, mode="always", n_not_sparse=m) for m in range(nq + 1)]
            assert took == sorted(took) and took[8] is False and took[9] is True              # monotone in n_not_sparse: from nine on
        for k in (1, 64, 1025, 4096):                                                         # the sibling's cell, and beyond this one's
            assert not batched_applies_filtered_wide(metric, dim, rows, nq, k, mode="always")
    assert not batched_applies_filtered_wide(metric, dim, rows, 8, 100, mode="always")
    assert not batched_applies_filtered_wide(metric, dim, 32_000, 256, 100, mode="always")    # below the batched path's smallest corpus
