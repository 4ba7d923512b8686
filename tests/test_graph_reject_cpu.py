"""qv_graph_reject_applies — the rule by which a graph traversal takes the form that rejects neighbours on the row-order bfloat16 copy —
as a table, on the host, and the prototypes of the symbols that came with it.  No device."""
import ctypes as C
import os
import re

import pytest

import quiver_amd
from quiver_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO, ALWAYS, NEVER = _lib.QV_GRAPH_REJECT_AUTO, _lib.QV_GRAPH_REJECT_ALWAYS, _lib.QV_GRAPH_REJECT_NEVER
CUS = 256
LAT_CAP = 768                                  # max(compute units, 768): the largest call the latency form takes


def applies(metric="cosine", dim=768, n=1_000_000, nq=8192, ef=128, cus=CUS, mode="always", **kw):
    return quiver_amd.graph_reject_applies(metric, dim, n, nq, ef, cus, mode, **kw)


def test_always_applies_where_the_kernel_can_run():
    assert applies() and applies(metric="dot") and applies(dim=64) and applies(dim=4096) and applies(n=10, ef=16)
    assert applies(max_m0=32) and applies(max_m0=1)


def test_never_takes_nothing_and_auto_the_measured_cells_only():
    """AUTO: cosine, dim 768, 1M to below 2M nodes, 8192 queries or more, list sizes 64 .. 256 (profiles/LAB_r17_graph_reject.md)"""
    for nq in (1024, 8191, 8192, 32768, 65536):
        for ef in (16, 63, 64, 128, 256, 257, 512):
            for dim in (128, 704, 768, 832, 1024):
                for n in (999_999, 1_000_000, 1_999_999, 2_000_000, 10_000_000):
                    for metric in ("cosine", "dot"):
                        assert not applies(metric=metric, mode="never", nq=nq, ef=ef, dim=dim, n=n)
                        assert applies(metric=metric, mode="always", nq=nq, ef=ef, dim=dim, n=n)
                        want = metric == "cosine" and nq >= 8192 and 64 <= ef <= 256 and dim == 768 and 1_000_000 <= n < 2_000_000
                        assert applies(metric=metric, mode="auto", nq=nq, ef=ef, dim=dim, n=n) == want, (metric, nq, ef, dim, n)


def test_no_plane_tombstones_and_wide_lists_answer_no_under_any_mode():
    for mode in ("auto", "always", "never"):
        assert not applies(mode=mode, has_plane=False)
        assert not applies(mode=mode, has_tombstones=True)
        assert not applies(mode=mode, max_m0=33) and not applies(mode=mode, max_m0=48)


@pytest.mark.parametrize("metric", sorted(set(_lib.METRICS.values())))
def test_each_metric(metric):
    assert applies(metric=metric) == (metric in (_lib.METRICS["cosine"], _lib.METRICS["dot"]))
    assert not applies(metric=metric, mode="never")


def test_dimensions_no_index_keeps_the_copy_for():
    for dim in (32, 96, 100, 4096 + 64):
        assert not applies(dim=dim)


def test_the_latency_forms_calls():
    assert not applies(nq=1) and not applies(nq=64) and not applies(nq=LAT_CAP)
    assert applies(nq=LAT_CAP + 1)
    assert not applies(nq=1000, cus=1000) and applies(nq=1001, cus=1000)      # a device with more compute units than 768
    assert applies(nq=LAT_CAP + 1, cus=1)


def test_argument_errors():
    f = _lib.lib().qv_graph_reject_applies
    ok = (0, 768, 1000, 8192, 128, CUS, ALWAYS, 1, 0, 32)
    assert f(*ok) == 1
    for pos, bad in ((0, -1), (0, 99), (1, 0), (5, 0), (5, -4), (6, 3), (6, -1)):
        a = list(ok); a[pos] = bad
        assert f(*a) == _lib.QV_ERR_INVALID_ARG, (pos, bad)
    with pytest.raises(quiver_amd.QvError):
        applies(mode=7)


def test_null_handles_are_argument_errors():
    out = (C.c_uint64 * 4)()
    assert _lib.lib().qv_graph_set_reject_plane(None, ALWAYS) == _lib.QV_ERR_INVALID_ARG
    assert _lib.lib().qv_graph_reject_stats(None, out) == _lib.QV_ERR_INVALID_ARG


def test_prototypes_and_constants_follow_the_header():
    h = open(os.path.join(ROOT, "include", "qv.h")).read()
    for name in ("qv_graph_set_reject_plane", "qv_graph_reject_stats", "qv_graph_reject_applies"):
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in _lib.PROTOTYPES and hasattr(_lib.lib(), name)
    decl = re.search(r"int qv_graph_reject_applies\(([^;]*)\);", h).group(1)
    assert len(decl.split(",")) == len(_lib.PROTOTYPES["qv_graph_reject_applies"][1]) == 10
    assert _lib.PROTOTYPES["qv_graph_set_reject_plane"] == (C.c_int, [C.c_void_p, C.c_int])
    assert _lib.PROTOTYPES["qv_graph_reject_stats"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)])
    for name, value in (("QV_FLAG_GRAPH_PLANE", 16), ("QV_GRAPH_REJECT_AUTO", 0), ("QV_GRAPH_REJECT_ALWAYS", 1), ("QV_GRAPH_REJECT_NEVER", 2),
                        ("QV_DEBUG_ROWMAJ16", 3)):
        m = re.search(r"#define %s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == value == getattr(_lib, name), name
    assert quiver_amd.DeviceIndex.DEBUG_READ["rowmaj16"][0] == _lib.QV_DEBUG_ROWMAJ16
    assert quiver_amd.DeviceGraph.REJECT_PLANE == {"auto": AUTO, "always": ALWAYS, "never": NEVER}
    assert re.search(r"#define QV_ABI_VERSION 4\b", h)
