"""quiver_amd — MI355X-native similarity-search hot path for Quiver.

The product is ``libqv.so`` (HIP kernels behind the C ABI of include/qv.h).  This
package is the thin Python host side used by the tests and the benchmark: a
ctypes binding (``_lib``), a row-numbered device index (``DeviceIndex``) and the
mirrors of the reference's host interfaces for this path (``hybrid``, ``hnsw``,
``core``, ``vectortypes``) — same names, argument meaning and error behaviour as
the Go packages they stand in for.
"""
from ._lib import QvError, lib, load_library, METRICS, metric_id  # noqa: F401
from .device_index import DeviceIndex, RowSet, Column, DeviceGraph, GraphReplicas, ShardedIndex, graph_reject_applies, graph_reject_image_applies  # noqa: F401


def scan_bound8_applies_mq(metric, dim: int, rows: int, nq: int, k: int, mode="auto", plane_mode_mq="auto", has_plane8: bool = True) -> bool:
    """whether an unfiltered shared pass of nq queries would start on the 8-bit plane — the dispatch's own rule, on the host, without an index
    or a device (qv_scan_bound8_applies_mq); metric: a name or an id, mode / plane_mode_mq: as set_bound_scan / set_bound_plane_mq take them"""
    from ._lib import check
    m = metric_id(metric) if isinstance(metric, str) else int(metric)
    rc = lib().qv_scan_bound8_applies_mq(m, dim, rows, nq, k, DeviceIndex.BOUND_SCAN.get(mode, mode), DeviceIndex.BOUND_PLANE.get(plane_mode_mq, plane_mode_mq), 1 if has_plane8 else 0)
    if rc < 0:
        check(rc)
    return rc == 1


def scan_bound8_applies_filtered_mq(metric, dim: int, rows: int, nq: int, k: int, mode="auto", plane_mode_filtered_mq="auto", has_plane8: bool = True,
                                    candidate_tiles: int = 0xFFFFFFFF) -> bool:
    """whether a FILTERED shared pass of nq queries would start on the 8-bit plane — the dispatch's own rule, on the host, without an index or a
    device (qv_scan_bound8_applies_filtered_mq); candidate_tiles: the 64-row tiles that hold a candidate of any query of the pass (more than
    the index has: every tile); mode / plane_mode_filtered_mq: as set_bound_scan / set_bound_plane_filtered_mq take them"""
    from ._lib import check
    m = metric_id(metric) if isinstance(metric, str) else int(metric)
    rc = lib().qv_scan_bound8_applies_filtered_mq(m, dim, rows, nq, k, DeviceIndex.BOUND_SCAN.get(mode, mode),
                                                  DeviceIndex.BOUND_PLANE.get(plane_mode_filtered_mq, plane_mode_filtered_mq), 1 if has_plane8 else 0, candidate_tiles)
    if rc < 0:
        check(rc)
    return rc == 1

def batched_applies_filtered(metric, dim: int, rows: int, nq: int, k: int, filter="auto", mode="auto", n_not_sparse: int | None = None) -> bool:
    """whether a piece of nq FILTERED queries (a row set, no set or a where-filter each) would take the batched path — the dispatch's own rule, on
    the host, without an index or a device (qv_batched_applies_filtered); filter / mode: as set_filter / set_filtered_batch take them;
    n_not_sparse: the queries the host does not know to be below the sparse floor (None: all of them)"""
    from ._lib import check
    m = metric_id(metric) if isinstance(metric, str) else int(metric)
    rc = lib().qv_batched_applies_filtered(m, dim, rows, nq, k, DeviceIndex.FILTERS.get(filter, filter), DeviceIndex.FILTERED_BATCH.get(mode, mode),
                                           nq if n_not_sparse is None else n_not_sparse)
    if rc < 0:
        check(rc)
    return rc == 1


def batched_filter_route(metric, dim: int, rows: int, nq: int, k: int, filter="auto", bf16_rows: bool = False, cus: int = 256):
    """(padded query count, main filter kernel) of a FILTERED batch of that shape — the batched path's plan and the substitution a batch with
    sets applies, on the host, without an index or a device (qv_batched_filter_route); the kernel as a name of DeviceIndex.BATCHED_FILTERS;
    filter: as set_filter takes it; bf16_rows: the index keeps the bfloat16 copy of its rows.  QvError (unsupported) where no filtered batch runs"""
    import ctypes as C
    from ._lib import check
    m = metric_id(metric) if isinstance(metric, str) else int(metric)
    pad, code = C.c_uint32(0), C.c_int(-1)
    check(lib().qv_batched_filter_route(m, dim, rows, nq, k, DeviceIndex.FILTERS.get(filter, filter), 1 if bf16_rows else 0, cus, C.byref(pad), C.byref(code)))
    return int(pad.value), DeviceIndex.BATCHED_FILTERS[code.value]


__all__ = ["QvError", "lib", "load_library", "METRICS", "metric_id", "DeviceIndex", "RowSet", "Column", "DeviceGraph", "GraphReplicas", "ShardedIndex", "scan_bound8_applies_mq", "scan_bound8_applies_filtered_mq",
           "batched_applies_filtered", "batched_filter_route", "graph_reject_applies", "graph_reject_image_applies"]
