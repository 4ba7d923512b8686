"""Range search without a device: the rule that says where a call starts (qv_scan_range_applies) and the argument checks of the knobs."""
import ctypes as C

import pytest

import quiver_amd
from quiver_amd import _lib


@pytest.mark.parametrize("metric,dim,mode,has_plane8,want", [
    ("cosine", 768, "always", True, True),
    ("dot", 64, "always", True, True),
    (_lib.QV_RULE_L2_PLANES, 4096, "always", True, True),
    ("l2", 768, "always", True, False),        # a Euclidean index without the scan planes
    ("l1", 768, "always", True, False),
    ("l2sq", 768, "always", True, False),
    ("cosine_f32", 768, "always", True, False),
    ("cosine", 768, "always", False, False),   # no plane
    ("cosine", 100, "always", True, False),    # not whole 16-dimension steps
    ("cosine", 4112, "always", True, False),   # past the plane's int32 sums
    ("cosine", 768, "auto", True, False),      # nothing measured yet
    ("cosine", 768, "never", True, False),
])
def test_range_rule(metric, dim, mode, has_plane8, want):
    assert quiver_amd.scan_range_applies(metric, dim, 1000000, 4, mode, has_plane8) is want


def test_range_bad_arguments():
    lib = quiver_amd.lib()
    assert lib.qv_scan_range_applies(0, 768, 1000, 1, 3, 1) < 0
    assert lib.qv_scan_range_applies(0, 768, 1000, 1, -1, 1) < 0
    assert lib.qv_scan_range_applies(99, 768, 1000, 1, 1, 1) < 0
    assert lib.qv_index_set_range_plane(None, 1) < 0
    assert lib.qv_index_range_stats(None, (C.c_uint64 * 4)()) < 0
