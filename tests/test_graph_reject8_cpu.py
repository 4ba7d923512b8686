"""qv_graph_reject_image_applies — the rule by which a rejecting graph traversal starts on the row-order 8-bit image (QV_FLAG_GRAPH_PLANE8), on the
bfloat16 copy, or does not reject — as a table, on the host; the prototypes, constants and names that came with it; null handles.  No device."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import quiver_amd
from quiver_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256
MODES = ("auto", "always", "never")
IMAGES = ("auto", "8bit", "bf16")
# AUTO's cells for the 8-bit image: exactly the cells of profiles/LAB_r23_graph_reject8.md's three-arm table in which 8-bit-first's slowest round beat
# bfloat16-first's fastest (both images held) and "never"'s fastest (only the 8-bit image held): all twelve — cosine, 1M x 768, list sizes 64 / 128 /
# 256, 8192 and 32 768 queries per call — read as the range the bfloat16 rule reads its own twelve as.


def auto8_cell(metric, dim, n, nq, ef):
    return metric == "cosine" and dim == 768 and 1_000_000 <= n < 2_000_000 and nq >= 8192 and 64 <= ef <= 256


def form(metric="cosine", dim=768, n=1_000_000, nq=8192, ef=128, cus=CUS, mode="always", **kw):
    return quiver_amd.graph_reject_image_applies(metric, dim, n, nq, ef, cus, mode, **kw)


def base(metric="cosine", dim=768, n=1_000_000, nq=8192, ef=128, cus=CUS, mode="always", **kw):
    return quiver_amd.graph_reject_applies(metric, dim, n, nq, ef, cus, mode, **kw)


def test_every_mode_and_image_combination():
    for mode, image, p16, p8 in itertools.product(MODES, IMAGES, (False, True), (False, True)):
        for dim, n, nq, ef in ((768, 1_000_000, 8192, 128), (768, 1_000_000, 32768, 256), (768, 20_000, 1024, 64), (128, 2000, 1024, 32), (192, 1500, 1024, 64),
                               (4096, 600, 1024, 64), (768, 1_000_000, 64, 128)):
            got = form(dim=dim, n=n, nq=nq, ef=ef, mode=mode, has_plane=p16, has_image8=p8, image_mode=image)
            b16 = p16 and base(dim=dim, n=n, nq=nq, ef=ef, mode=mode, has_plane=True)
            b8 = p8 and dim % 128 == 0 and base(dim=dim, n=n, nq=nq, ef=ef, mode=mode, has_plane=True)
            if image == "bf16":
                want = 1 if b16 else 0
            elif image == "8bit":
                want = 2 if b8 else 1 if b16 else 0
            else:
                want = 2 if b8 and auto8_cell("cosine", dim, n, nq, ef) else 1 if b16 else 0
            assert got == want, (mode, image, p16, p8, dim, n, nq, ef)


def test_an_index_without_the_image_answers_as_the_bfloat16_rule_under_every_mode():
    for mode, image, p16 in itertools.product(MODES, IMAGES, (False, True)):
        for metric, dim, n, nq, ef in (("cosine", 768, 1_000_000, 8192, 128), ("dot", 128, 5000, 1024, 64), ("l2", 128, 5000, 1024, 64), ("cosine", 96, 5000, 1024, 64)):
            assert form(metric=metric, dim=dim, n=n, nq=nq, ef=ef, mode=mode, has_plane=p16, has_image8=False, image_mode=image) == \
                int(base(metric=metric, dim=dim, n=n, nq=nq, ef=ef, mode=mode, has_plane=p16))


def test_monotone_in_what_the_bfloat16_rule_allows():
    """never non-zero where qv_graph_reject_applies answers 0 for an index holding that image"""
    for mode, image, p16, p8 in itertools.product(MODES, IMAGES, (False, True), (False, True)):
        for kw in (dict(has_tombstones=True), dict(max_m0=33), dict(max_m0=48), dict(nq=64), dict(nq=768), dict(metric="l2"), dict(metric="l2sq"), dict(dim=4096 + 128),
                   dict(dim=100)):
            assert not base(mode=mode, has_plane=True, **kw)
            assert form(mode=mode, has_plane=p16, has_image8=p8, image_mode=image, **kw) == 0, (mode, image, kw)
    for image, p16, p8 in itertools.product(IMAGES, (False, True), (False, True)):
        assert form(mode="never", has_plane=p16, has_image8=p8, image_mode=image) == 0
    # dimensions that hold the bfloat16 copy and not whole 128-element slabs: the 8-bit form never, the bfloat16 copy as before
    for dim in (64, 192, 320, 832):
        assert form(dim=dim, image_mode="8bit", has_plane=True, has_image8=True) == 1
        assert form(dim=dim, image_mode="8bit", has_plane=False, has_image8=True) == 0
    for dim in (128, 256, 768, 4096):
        assert form(dim=dim, image_mode="8bit", has_plane=True, has_image8=True) == 2
        assert form(dim=dim, image_mode="8bit", has_plane=False, has_image8=True) == 2
        assert form(dim=dim, image_mode="bf16", has_plane=False, has_image8=True) == 0
    assert form(metric="dot", image_mode="8bit") == 2 and form(metric="dot", image_mode="auto") == 1 and form(image_mode="auto") == 2


def test_autos_cells_are_the_measured_ones():
    for metric, dim, n, nq, ef in itertools.product(("cosine", "dot"), (128, 768, 1024), (20_000, 1_000_000, 10_000_000), (1024, 8192, 32768), (64, 128, 256, 512)):
        for mode in ("auto", "always"):
            both = form(metric=metric, dim=dim, n=n, nq=nq, ef=ef, mode=mode, has_plane=True, has_image8=True, image_mode="auto")
            only8 = form(metric=metric, dim=dim, n=n, nq=nq, ef=ef, mode=mode, has_plane=False, has_image8=True, image_mode="auto")
            b = base(metric=metric, dim=dim, n=n, nq=nq, ef=ef, mode=mode, has_plane=True)
            assert both == (2 if b and auto8_cell(metric, dim, n, nq, ef) else int(b)), (metric, dim, n, nq, ef, mode)
            assert only8 == (2 if b and auto8_cell(metric, dim, n, nq, ef) else 0), (metric, dim, n, nq, ef, mode)
    # the measured cells themselves, and their neighbours
    for ef, nq in itertools.product((64, 128, 256), (8192, 32768)):
        assert form(ef=ef, nq=nq, mode="auto", image_mode="auto") == 2 and form(ef=ef, nq=nq, mode="auto", image_mode="auto", has_plane=False) == 2
        assert form(ef=ef, nq=nq, mode="auto", image_mode="bf16") == 1 and form(ef=ef, nq=nq, mode="auto", image_mode="auto", has_image8=False) == 1
    for kw in (dict(ef=63), dict(ef=257), dict(nq=8191), dict(n=999_999), dict(n=2_000_000), dict(dim=640), dict(dim=896), dict(metric="dot")):
        assert form(mode="always", image_mode="auto", **kw) == 1 and form(mode="always", image_mode="auto", has_plane=False, **kw) == 0, kw


def test_argument_errors():
    f = _lib.lib().qv_graph_reject_image_applies
    ok = (0, 768, 1000, 8192, 128, CUS, 1, 1, 0, 32, 1, _lib.QV_GRAPH_IMAGE_8BIT)
    assert f(*ok) == 2
    for pos, bad in ((0, -1), (0, 99), (1, 0), (5, 0), (5, -4), (6, 3), (6, -1), (11, 3), (11, -1)):
        a = list(ok); a[pos] = bad
        assert f(*a) == _lib.QV_ERR_INVALID_ARG, (pos, bad)
    with pytest.raises(quiver_amd.QvError):
        form(image_mode=7)
    with pytest.raises(quiver_amd.QvError):
        form(mode=7)


def test_null_handles_are_argument_errors():
    out = (C.c_uint64 * 4)()
    assert _lib.lib().qv_graph_set_reject_image(None, _lib.QV_GRAPH_IMAGE_8BIT) == _lib.QV_ERR_INVALID_ARG
    assert _lib.lib().qv_graph_reject8_stats(None, out) == _lib.QV_ERR_INVALID_ARG
    assert _lib.lib().qv_index_debug_read(None, _lib.QV_DEBUG_ROWMAJ8, None, 0) == _lib.QV_ERR_INVALID_ARG


def test_prototypes_constants_and_names():
    h = open(os.path.join(ROOT, "include", "qv.h")).read()
    for name in ("qv_graph_set_reject_image", "qv_graph_reject8_stats", "qv_graph_reject_image_applies"):
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in _lib.PROTOTYPES and hasattr(_lib.lib(), name)
    decl = re.search(r"int qv_graph_reject_image_applies\(([^;]*)\);", h).group(1)
    assert len(decl.split(",")) == len(_lib.PROTOTYPES["qv_graph_reject_image_applies"][1]) == 12
    assert _lib.PROTOTYPES["qv_graph_set_reject_image"] == (C.c_int, [C.c_void_p, C.c_int])
    assert _lib.PROTOTYPES["qv_graph_reject8_stats"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)])
    assert len(_lib.PROTOTYPES["qv_graph_reject_applies"][1]) == 10              # (unchanged)
    for name, value in (("QV_FLAG_GRAPH_PLANE8", 64), ("QV_GRAPH_IMAGE_AUTO", 0), ("QV_GRAPH_IMAGE_8BIT", 1), ("QV_GRAPH_IMAGE_BF16", 2), ("QV_DEBUG_ROWMAJ8", 9),
                        ("QV_DEBUG_ROWMETA8", 10)):
        m = re.search(r"#define %s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == value == getattr(_lib, name), name
    codes = [int(x) for x in re.findall(r"#define QV_DEBUG_\w+\s+(\d+)", h)]
    assert len(codes) == len(set(codes))                                        # the new codes were free
    assert re.search(r"#define QV_ABI_VERSION 4\b", h)
    assert quiver_amd.DeviceGraph.REJECT_IMAGE == {"auto": 0, "8bit": 1, "bf16": 2}
    assert quiver_amd.DeviceIndex.DEBUG_READ["rowmaj8"] == (9, np.int8)
    code, dt = quiver_amd.DeviceIndex.DEBUG_READ["rowmeta8"]
    assert code == 10 and dt.itemsize == 16 and dt.names == ("rnorm", "rscale8", "rres8")
    import inspect
    assert "graph_plane8" in inspect.signature(quiver_amd.DeviceIndex.__init__).parameters
    assert "graph_plane8" in inspect.signature(quiver_amd.ShardedIndex.__init__).parameters
    assert hasattr(quiver_amd.DeviceGraph, "set_reject_image") and hasattr(quiver_amd.DeviceGraph, "reject8_stats")
    go = {n: open(os.path.join(ROOT, "go", "quivergpu", n)).read() for n in ("index.go", "graph.go")}
    assert "FlagGraphPlane8 uint64 = C.QV_FLAG_GRAPH_PLANE8" in go["index.go"]
    for word in ("GraphPlane8 bool", "func (h *Graph) SetRejectImage(mode int) error", "func (h *Graph) Reject8Stats() (RejectStats, error)", "C.qv_graph_set_reject_image(",
                 "C.qv_graph_reject8_stats(", "C.QV_GRAPH_IMAGE_8BIT"):
        assert word in go["graph.go"], word
    from quiver_amd.hnsw import Config
    assert Config().GraphPlane8 is False and Config().GraphPlane is False
    # the host mirror passes the flag bit and calls no new library symbol (tests/c/qv_stub.cpp stands in for the library as it is)
    host = open(os.path.join(ROOT, "quiver_amd", "csrc", "host", "qvhost.cpp")).read()
    assert "QV_FLAG_GRAPH_PLANE8" in host
    for name in ("qv_graph_set_reject_image", "qv_graph_reject8_stats", "qv_graph_reject_image_applies"):
        assert name not in host
