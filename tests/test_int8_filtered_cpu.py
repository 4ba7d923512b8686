"""Whether a FILTERED batch takes the int8 kernel's sets form (qv_batched_int8_applies_filtered): only where qv_batched_int8_applies holds, the
filtered batch has a route for that k, and the mode says so — the automatic mode has no measured cell yet."""
import ctypes as C

import pytest

import quiver_amd
from quiver_amd import _lib

M = 1_000_000
INVALID_ARG = -1

@pytest.mark.parametrize("metric,dim,nq,k,filt,plane8,mode,want", [
    ("cosine", 768, 16, 10, "int8", True, "always", True),
    ("cosine", 1024, 256, 64, "int8", True, "always", True),
    ("cosine", 768, 16, 1024, "int8", True, "always", True),          # the wide funnel's route
    ("euclidean", 768, 16, 10, "int8", True, "always", False),        # metric
    ("cosine", 768, 16, 10, "int8", False, "always", False),          # no plane
    ("cosine", 48, 16, 10, "int8", True, "always", False),            # dimension
    ("cosine", 768, 8, 10, "int8", True, "always", False),            # fewer than 9 queries
    ("cosine", 768, 16, 1025, "int8", True, "always", False),         # k beyond the filtered batch's
    ("cosine", 768, 16, 10, "auto", True, "always", False),           # another filter
    ("cosine", 768, 16, 10, "int8", True, "auto", False),             # nothing is measured
    ("cosine", 768, 16, 10, "int8", True, "never", False),
])
def test_rule(metric, dim, nq, k, filt, plane8, mode, want):
    assert quiver_amd.batched_int8_applies_filtered(metric, dim, M, nq, k, filter=filt, has_plane8=plane8, mode=mode) is want

@pytest.mark.parametrize("filt,mode", [(5, -1), (5, 3), (-1, 1), (6, 1)])
def test_arguments_out_of_range(filt, mode):
    assert _lib.lib().qv_batched_int8_applies_filtered(0, 768, M, 16, 10, filt, 1, mode) == INVALID_ARG

def test_null_handle_and_unknown_word():
    assert _lib.lib().qv_index_set_int8_filtered(None, 1) == _lib.lib().qv_index_int8_filtered_stats(None, (C.c_uint64 * 4)()) == INVALID_ARG
    with pytest.raises(ValueError):                                     # (no device: the word is rejected before the handle is read)
        object.__new__(quiver_amd.DeviceIndex).set_int8_filtered("sometimes")
