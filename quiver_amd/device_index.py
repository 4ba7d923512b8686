"""DeviceIndex — a row-numbered, device-resident exact index: the Python face of one
``qv_index`` (one GPU, one shard).  String ids live one layer up (quiver_amd.hybrid)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib, metric_id


def _f32c(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def scan_bound_applies_filtered(metric, dim: int, rows: int, nq: int, k: int, mode="auto", has_plane: bool = True, candidate_tiles: int = 0) -> bool:
    """whether a FILTERED search (search_masked, search_rowsets, search_rowsets_device) of that shape takes the bound scan on the bfloat16
    copy under `mode`; candidate_tiles: the 64-row tiles that hold a candidate of any query of the pass (qv_scan_bound_applies_filtered)"""
    rc = lib().qv_scan_bound_applies_filtered(metric_id(metric), dim, rows, nq, k, DeviceIndex.BOUND_SCAN.get(mode, mode), 1 if has_plane else 0, candidate_tiles)
    if rc < 0:
        check(rc)
    return bool(rc)


PREDICATES = {"==": 0, "=": 0, "eq": 0, "!=": 1, "ne": 1, "<": 2, "lt": 2, "<=": 3, "le": 3, ">": 4, "gt": 4, ">=": 5, "ge": 5,
              "in": 6, "not_in": 7, "present": 8, "absent": 9}
WHERE_FILTERS_PER_LAUNCH = 8                     # QV_WHERE_FILTERS_PER_LAUNCH of include/qv.h
WHERE_DEVICE_LITERALS = 16                       # QV_WHERE_DEVICE_LITERALS


class QvWhere(C.Structure):
    """qv_where of include/qv.h: one conjunction, the arguments of qv_rowset_create_where"""
    _fields_ = [("cols", C.POINTER(C.c_void_p)), ("ops", C.POINTER(C.c_int)), ("literals", C.POINTER(C.c_double)),
                ("lit_off", C.POINTER(C.c_uint32)), ("n_preds", C.c_uint32)]


def _is_predicate(x) -> bool:
    return isinstance(x, tuple) and len(x) == 3 and isinstance(x[1], (str, int, np.integer)) and not isinstance(x[1], bool)


def broadcast_filters(filters, nq: int) -> list:
    """the `filters` argument of DeviceIndex.search_where as one list of predicates per query: None -> no predicate for any query; ONE
    list of (column, op, literal_or_list) tuples -> that list for every query; otherwise a sequence of nq entries, each such a list or
    None (no predicate: every row).  Pure."""
    if filters is None:
        return [[] for _ in range(nq)]
    filters = list(filters)
    if all(_is_predicate(f) for f in filters):              # (an empty list: the empty conjunction for every query)
        return [list(filters) for _ in range(nq)]
    if len(filters) != nq:
        raise ValueError("filters must be None, one list of predicates, or one list (or None) per query (%d), got %d" % (nq, len(filters)))
    out = []
    for i, f in enumerate(filters):
        f = [] if f is None else list(f)
        if not all(_is_predicate(p) for p in f):
            raise TypeError("filters[%d] is not a list of (column, op, literal_or_list) tuples" % i)
        out.append(f)
    return out


def pack_predicates(preds, handle_of=None):
    """one conjunction as the arrays qv_where points to -> (column handles [n] uint64, ops [n] int32, literals float64, lit_off [n + 1]
    uint32).  op: a key of PREDICATES or a QV_PRED_* code; a literal: None, a number or a list of numbers.  handle_of(column) -> the
    qv_column handle as an int (the default reads Column.handle).  Pure: no library call."""
    if handle_of is None:
        def handle_of(col):
            if not isinstance(col, Column):
                raise TypeError("a predicate does not name a Column")
            return col.handle.value
    preds = list(preds)
    n = len(preds)
    cols = np.zeros(n, dtype=np.uint64)
    ops = np.zeros(n, dtype=np.int32)
    off = np.zeros(n + 1, dtype=np.uint32)
    lits = []
    for i, (col, op, lit) in enumerate(preds):
        cols[i] = handle_of(col) or 0
        ops[i] = PREDICATES[op.lower()] if isinstance(op, str) else int(op)
        if lit is not None:
            lits.extend(np.asarray(lit, dtype=np.float64).ravel().tolist())
        off[i + 1] = len(lits)
    return cols, ops, np.asarray(lits, dtype=np.float64), off


def pack_where(per_query, handle_of=None):
    """lists of predicates, one per query -> (a ctypes array of QvWhere, the numpy arrays it points into: keep them until the call
    has returned).  Pure: no library call."""
    arr = (QvWhere * max(len(per_query), 1))()
    keep = []
    for q, preds in enumerate(per_query):
        cols, ops, lits, off = pack_predicates(preds, handle_of)
        keep.append((cols, ops, lits, off))
        w = arr[q]
        w.n_preds = len(cols)
        w.cols = C.cast(cols.ctypes.data, C.POINTER(C.c_void_p)) if cols.size else None
        w.ops = C.cast(ops.ctypes.data, C.POINTER(C.c_int)) if ops.size else None
        w.literals = C.cast(lits.ctypes.data, C.POINTER(C.c_double)) if lits.size else None
        w.lit_off = C.cast(off.ctypes.data, C.POINTER(C.c_uint32))
    return arr, keep


class DeviceIndex:
    default_filter = "auto"        # the filter kernel new indexes choose (set_filter); tests and bench.py compare the kernels through it

    def __init__(self, dim: int, metric="cosine", device: int = 0, rowmajor: bool = False, bf16_rows: bool = False, filter=None, scan_plane: bool = True, l2_scan_plane: bool = False,
                 graph_plane: bool = False, plane6: bool = True, graph_plane8: bool = False):
        self._h = C.c_void_p()
        self.dim = int(dim)
        self.metric = metric_id(metric)
        self.device = device
        check(lib().qv_index_create(C.byref(self._h), self.dim, self.metric, device, (_lib.QV_FLAG_ROWMAJOR if rowmajor else 0) | (_lib.QV_FLAG_BF16_ROWS if bf16_rows else 0) |
                                    (0 if scan_plane else _lib.QV_FLAG_NO_SCAN_PLANE) |   # scan_plane=False: no default bfloat16 copy (cosine / dot), no bound scan
                                    (_lib.QV_FLAG_L2_SCAN_PLANE if l2_scan_plane else 0) |   # l2_scan_plane=True: an "l2" index keeps the planes cosine / dot keep by default
                                    (0 if plane6 else _lib.QV_FLAG_NO_PLANE6) |   # plane6=False: no 6-bit plane beside the 8-bit one
                                    (_lib.QV_FLAG_GRAPH_PLANE8 if graph_plane8 else 0) |   # graph_plane8=True (with rowmajor): an int8 image in row order and a record per row for DeviceGraph.set_reject_image
                                    (_lib.QV_FLAG_GRAPH_PLANE if graph_plane else 0)))   # graph_plane=True (with rowmajor): a bfloat16 copy in row order for DeviceGraph.set_reject_plane
        f = filter if filter is not None else DeviceIndex.default_filter
        if f not in ("auto", 0):
            self.set_filter(f)

    # ---- lifecycle ----
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().qv_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def reserve(self, rows: int):
        check(lib().qv_index_reserve(self._h, rows))

    # ---- mutation ----
    def add(self, rows) -> int:
        rows = _f32c(rows)
        if rows.ndim == 1:
            rows = rows[None, :]
        if rows.shape[1] != self.dim:
            raise ValueError(f"vector dimension mismatch: expected {self.dim}, got {rows.shape[1]}")
        first = C.c_uint32(0)
        check(lib().qv_index_add(self._h, rows.ctypes.data, rows.shape[0], C.byref(first)))
        return int(first.value)

    def add_device(self, d_ptr: int, n: int, stream: int = 0) -> int:
        first = C.c_uint32(0)
        check(lib().qv_index_add_device(self._h, d_ptr, n, C.byref(first), stream))
        return int(first.value)

    def add_synthetic(self, seed: int, gen_row0: int, n: int) -> int:
        first = C.c_uint32(0)
        check(lib().qv_index_add_synthetic(self._h, seed, gen_row0, n, C.byref(first)))
        return int(first.value)

    def remove(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint32).ravel()
        check(lib().qv_index_remove(self._h, rows.ctypes.data, rows.size))

    def update(self, row: int, vec):
        vec = _f32c(vec)
        if vec.size != self.dim:
            raise ValueError(f"vector dimension mismatch: expected {self.dim}, got {vec.size}")
        check(lib().qv_index_update(self._h, row, vec.ctypes.data))

    def _rows_vecs(self, rows, vecs):
        rows = np.ascontiguousarray(rows, dtype=np.uint32).ravel()
        vecs = _f32c(vecs)
        if vecs.ndim == 1:
            vecs = vecs[None, :]
        if vecs.ndim != 2 or vecs.shape[1] != self.dim:
            raise ValueError(f"vector dimension mismatch: expected {self.dim}, got {vecs.shape[-1]}")
        if vecs.shape[0] != rows.size:
            raise ValueError(f"{rows.size} rows listed, {vecs.shape[0]} vectors given")
        return rows, vecs

    def update_rows(self, rows, vecs):
        """overwrite the listed rows in one call (qv_index_update_rows): what `for r, v in zip(rows, vecs): update(r, v)` leaves"""
        rows, vecs = self._rows_vecs(rows, vecs)
        check(lib().qv_index_update_rows(self._h, rows.ctypes.data, rows.size, vecs.ctypes.data))

    def update_rows_device(self, rows, d_ptr: int, stream: int = 0):
        """the same, the vectors [len(rows), dim] float32 already on the device; the row list stays on the host; synchronous w.r.t. `stream`"""
        rows = np.ascontiguousarray(rows, dtype=np.uint32).ravel()
        check(lib().qv_index_update_rows_device(self._h, rows.ctypes.data, rows.size, d_ptr, stream or None))

    # ---- queries ----
    def rows(self) -> int:
        return int(lib().qv_index_rows(self._h))

    def size(self) -> int:
        return int(lib().qv_index_size(self._h))

    def __len__(self):
        return self.size()

    def get_row(self, row: int) -> np.ndarray:
        out = np.empty(self.dim, dtype=np.float32)
        check(lib().qv_index_get_row(self._h, row, out.ctypes.data))
        return out

    def get_rows(self, rows) -> np.ndarray:
        """[n, dim]: the listed rows in one device pass (qv_index_get_rows)"""
        r = np.ascontiguousarray(rows, dtype=np.uint32).ravel()
        out = np.empty((r.size, self.dim), dtype=np.float32)
        check(lib().qv_index_get_rows(self._h, r.ctypes.data, r.size, out.ctypes.data))
        return out

    def search(self, queries, k: int, batched: bool = False):
        """-> (rows [nq,k] uint32, dist [nq,k] float32, count [nq] uint32)"""
        q = _f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dimension mismatch: expected {self.dim}, got {q.shape[1]}")
        nq = q.shape[0]
        kk = max(int(k), 0)
        rows = np.full((nq, max(kk, 1)), 0xFFFFFFFF, dtype=np.uint32)
        dist = np.full((nq, max(kk, 1)), np.inf, dtype=np.float32)
        count = np.zeros(nq, dtype=np.uint32)
        fn = lib().qv_index_search_batched if batched else lib().qv_index_search
        check(fn(self._h, q.ctypes.data, nq, kk, rows.ctypes.data, dist.ctypes.data, count.ctypes.data))
        return rows[:, :kk], dist[:, :kk], count

    def search_device(self, d_queries: int, nq: int, k: int, d_rows_out: int, d_dist_out: int, stream: int = 0):
        check(lib().qv_index_search_device(self._h, d_queries, nq, k, d_rows_out, d_dist_out, stream))

    def search_masked(self, queries, k: int, mask):
        """exact top-k among the rows selected by `mask` (bool [rows] or packed uint64 words): filtered search without a full ranking"""
        q = _f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError("query dimension %d does not match index dimension %d" % (q.shape[1], self.dim))
        m = np.asarray(mask)
        words = (self.rows() + 63) // 64
        if m.dtype == np.bool_:
            if m.size != self.rows():
                raise ValueError("mask must have one entry per row")
            pad = np.zeros(words * 64, dtype=np.uint8); pad[:m.size] = m
            m = np.packbits(pad, bitorder="little").view(np.uint64)
        m = np.ascontiguousarray(m, dtype=np.uint64)
        if m.size != words:
            raise ValueError("mask must have ceil(rows/64) words")
        nq = q.shape[0]
        rows = np.empty((nq, max(k, 1)), dtype=np.uint32); dist = np.empty((nq, max(k, 1)), dtype=np.float32); cnt = np.empty(nq, dtype=np.uint32)
        check(lib().qv_index_search_masked(self._h, q.ctypes.data, nq, k, m.ctypes.data, rows.ctypes.data, dist.ctypes.data, cnt.ctypes.data))
        return rows, dist, cnt

    # ---- row sets: device-resident filters, one per query ----
    def _mask_words(self, mask) -> np.ndarray:
        m = np.asarray(mask)
        words = (self.rows() + 63) // 64
        if m.dtype == np.bool_:
            if m.size != self.rows():
                raise ValueError("mask must have one entry per row")
            pad = np.zeros(words * 64, dtype=np.uint8); pad[:m.size] = m
            m = np.packbits(pad, bitorder="little").view(np.uint64)
        m = np.ascontiguousarray(m, dtype=np.uint64)
        if m.size != words:
            raise ValueError("mask must have ceil(rows/64) words")
        return m

    def rowset(self, mask_or_rows=None, *, rows=None) -> "RowSet":
        """a set of this index's rows, resident on its device (qv_rowset_create): from a bool mask [rows], packed uint64 words
        [ceil(rows/64)], a list of row numbers (any other integer array), or None for the empty set.  A uint64 array is ALWAYS read as
        packed words: row numbers of that dtype (or of any other) go in `rows=`, which is never read as a mask.  Rows added to the
        index later start unselected; tombstones are honoured by the searches, not folded in here."""
        return RowSet(self, mask_or_rows, rows=rows)

    def _set_handles(self, sets, nq: int):
        if sets is None or isinstance(sets, RowSet):
            sets = [sets] * nq
        sets = list(sets)
        if len(sets) != nq:
            raise ValueError("sets must be a RowSet, None, or one of either per query (%d), got %d" % (nq, len(sets)))
        arr = (C.c_void_p * max(nq, 1))()
        for i, s in enumerate(sets):
            if s is not None and not isinstance(s, RowSet):
                raise TypeError("sets[%d] is not a RowSet" % i)
            arr[i] = None if s is None else s.handle.value
        return arr, sets                                   # (the list keeps the RowSet objects alive across the call)

    def search_rowsets(self, queries, k: int, sets):
        """exact top-k of every query among the live rows of ITS set (qv_index_search_rowsets): `sets` is a RowSet, None (every row),
        or a sequence of one of either per query.  -> (rows [nq,k] uint32, dist [nq,k] float32, count [nq] uint32)"""
        q = _f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dimension mismatch: expected {self.dim}, got {q.shape[1]}")
        nq = q.shape[0]
        arr, keep = self._set_handles(sets, nq)
        kk = max(int(k), 0)
        rows = np.full((nq, max(kk, 1)), 0xFFFFFFFF, dtype=np.uint32)
        dist = np.full((nq, max(kk, 1)), np.inf, dtype=np.float32)
        count = np.zeros(nq, dtype=np.uint32)
        check(lib().qv_index_search_rowsets(self._h, q.ctypes.data, nq, kk, arr, rows.ctypes.data, dist.ctypes.data, count.ctypes.data))
        del keep
        return rows[:, :kk], dist[:, :kk], count

    def search_rowsets_device(self, d_queries: int, nq: int, k: int, sets, d_rows_out: int, d_dist_out: int, stream: int = 0):
        """the same with queries / results on the device; enqueues on `stream`, no synchronisation (qv_index_search_rowsets_device)"""
        arr, keep = self._set_handles(sets, nq)
        check(lib().qv_index_search_rowsets_device(self._h, d_queries, nq, k, arr, d_rows_out, d_dist_out, stream))
        del keep

    # ---- facet columns: row sets from predicates, on the device ----
    COLUMN_TYPES = {"f64": 0, "u32": 1}

    PREDICATES = PREDICATES                      # (the module's table: pack_predicates reads the same one)

    def column(self, type) -> "Column":
        """one typed value per row of this index, resident on its device (qv_column_create): "f64" (a JSON number) or "u32" (a
        dictionary code or rank the host assigns).  Rows never set, and rows added later, have no value."""
        return Column(self, type)

    def rowset_where(self, predicates) -> "RowSet":
        """the rows for which EVERY (column, op, literal_or_list) holds, evaluated in one pass on the device (qv_rowset_create_where):
        op is a key of PREDICATES or a QV_PRED_* code; "present" / "absent" take None.  A row without a value fails every op but
        "absent".  1 to 8 predicates, most selective first: a tile no row of which passes reads no later column."""
        preds = list(predicates)
        n = len(preds)
        cols = (C.c_void_p * max(n, 1))()
        ops = (C.c_int * max(n, 1))()
        off = np.zeros(n + 1, dtype=np.uint32)
        lits = []
        for i, (col, op, lit) in enumerate(preds):
            if not isinstance(col, Column):
                raise TypeError("predicate %d does not name a Column" % i)
            cols[i] = col.handle.value
            ops[i] = self.PREDICATES[op.lower()] if isinstance(op, str) else int(op)
            if lit is not None:
                lits.extend(np.asarray(lit, dtype=np.float64).ravel().tolist())
            off[i + 1] = len(lits)
        lit_arr = np.asarray(lits, dtype=np.float64)
        rs = RowSet.__new__(RowSet)
        rs._h = C.c_void_p()
        rs._index = self
        check(lib().qv_rowset_create_where(C.byref(rs._h), self._h, cols, ops, lit_arr.ctypes.data if lit_arr.size else None, off.ctypes.data, n))
        del preds                                           # (kept the Column objects alive across the call)
        return rs

    def search_where(self, queries, k: int, filters):
        """exact top-k of every query among the live rows that pass ITS conjunction of column predicates, evaluated on the device inside
        the call (qv_index_search_where): no RowSet is made, nothing but the results comes back.  `filters`: one list of (column, op,
        literal_or_list) per query (as rowset_where takes; None or [] = every row), or ONE such list for all queries, or None.
        -> (rows [nq,k] uint32, dist [nq,k] float32, count [nq] uint32), what search_rowsets returns for the sets rowset_where makes."""
        q = _f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dimension mismatch: expected {self.dim}, got {q.shape[1]}")
        nq = q.shape[0]
        per_query = broadcast_filters(filters, nq)
        arr, keep = pack_where(per_query)
        kk = max(int(k), 0)
        rows = np.full((nq, max(kk, 1)), 0xFFFFFFFF, dtype=np.uint32)
        dist = np.full((nq, max(kk, 1)), np.inf, dtype=np.float32)
        count = np.zeros(nq, dtype=np.uint32)
        check(lib().qv_index_search_where(self._h, q.ctypes.data, nq, kk, arr, rows.ctypes.data, dist.ctypes.data, count.ctypes.data))
        del keep, per_query                                # (kept the arrays and the Column objects alive across the call)
        return rows[:, :kk], dist[:, :kk], count

    def search_where_device(self, d_queries: int, nq: int, k: int, filters, d_rows_out: int, d_dist_out: int, stream: int = 0):
        """the same with queries / results on the device; enqueues on `stream`, no synchronisation (qv_index_search_where_device).
        k <= 64 and at most WHERE_DEVICE_LITERALS literals per filter, else QvError(QV_ERR_UNSUPPORTED) with nothing enqueued; the
        filter arrays are read before the call returns."""
        per_query = broadcast_filters(filters, nq)
        arr, keep = pack_where(per_query)
        check(lib().qv_index_search_where_device(self._h, d_queries, nq, k, arr, d_rows_out, d_dist_out, stream))
        del keep, per_query

    def rowset_coalesce_stats(self) -> dict:
        out = (C.c_uint64 * 8)()
        check(lib().qv_index_rowset_coalesce_stats(self._h, out))
        return dict(zip(("solo", "led", "rode", "groups", "group_queries", "lingers", "linger_ns", "group_pass_ns"), [int(x) for x in out]))

    def search_negative(self, query, negative, k_fetch: int):
        """-> (rows [k_fetch], dist, neg_dist, count): qv_index_search_negative"""
        q, n = _f32c(query).ravel(), _f32c(negative).ravel()
        if q.size != self.dim or n.size != self.dim:
            raise ValueError(f"query dimension mismatch: expected {self.dim}, got {q.size if q.size != self.dim else n.size}")
        kk = max(int(k_fetch), 0)
        rows = np.full(max(kk, 1), 0xFFFFFFFF, dtype=np.uint32); dist = np.full(max(kk, 1), np.inf, dtype=np.float32)
        nd = np.full(max(kk, 1), np.inf, dtype=np.float32); cnt = C.c_uint32(0)
        check(lib().qv_index_search_negative(self._h, q.ctypes.data, n.ctypes.data, kk, rows.ctypes.data, dist.ctypes.data, nd.ctypes.data, C.byref(cnt)))
        return rows[:kk], dist[:kk], nd[:kk], int(cnt.value)

    def search_batched_device(self, d_queries: int, nq: int, k: int, d_rows_out: int, d_dist_out: int, d_redo_flags: int, stream: int = 0):
        check(lib().qv_index_search_batched_device(self._h, d_queries, nq, k, d_rows_out, d_dist_out, d_redo_flags, stream))

    def distance_rows(self, query, rows) -> np.ndarray:
        q = _f32c(query)
        if q.size != self.dim:
            raise ValueError(f"query dimension mismatch: expected {self.dim}, got {q.size}")
        r = np.ascontiguousarray(rows, dtype=np.uint32).ravel()
        out = np.empty(r.size, dtype=np.float32)
        check(lib().qv_distance_rows(self._h, q.ctypes.data, r.ctypes.data, r.size, out.ctypes.data))
        return out

    def distance_rows_device(self, d_query: int, d_rows: int, n: int, d_out: int, stream: int = 0):
        check(lib().qv_distance_rows_device(self._h, d_query, d_rows, n, d_out, stream))


    FILTERS = {"auto": 0, "fp32": 1, "bf16x3": 2, "bf16x1": 3, "off": 4}

    BOUND_SCAN = {"auto": 0, "always": 1, "never": 2}

    def set_bound_scan(self, mode):
        """the single-query scan that rejects rows on the bfloat16 copy: "auto" (from the measured row count on), "always" (whenever the
        copy exists and the shape applies), "never" (qv_index_set_bound_scan)"""
        check(lib().qv_index_set_bound_scan(self._h, self.BOUND_SCAN.get(mode, mode)))

    def bound_scan_stats(self) -> dict:
        """candidates of the last bound scan, searches it handed back to the exact scan, searches that took it, whether the copy exists"""
        out = (C.c_uint64 * 4)()
        check(lib().qv_index_bound_scan_stats(self._h, out))
        return {"candidates": int(out[0]), "hand_backs": int(out[1]), "searches": int(out[2]), "plane": bool(out[3])}

    BOUND_WIDE_CAND_CAP = _lib.QV_BOUND_WIDE_CAND_CAP   # rows the wide form's re-score walks at most

    def set_bound_scan_wide(self, mode):
        """the wide form of the single-query, unfiltered bound scan, 65 <= k <= 1024: "auto" (the measured shapes: cosine / dot, k <= 1000, from 1M rows of 768 dimensions or 10M rows of 128),
        "always" (whenever the shape applies), "never"; a knob of its own, independent of set_bound_scan — which plane comes first follows
        set_bound_plane (qv_index_set_bound_scan_wide)"""
        check(lib().qv_index_set_bound_scan_wide(self._h, self.BOUND_SCAN.get(mode, mode)))

    def set_bound_scan_wide_filtered(self, mode):
        """the wide form for ONE filtered query, 65 <= k <= 1024 (search_masked, search_rowsets, search_rowsets_device, search_where): "auto"
        (the measured shapes: cosine / dot, k <= 1000, from 1M rows of 768 dimensions or 10M rows of 128, a candidate in one tile in ten or more), "always" (whenever the shape applies and the filter leaves more live candidates than
        results), "never"; a knob of its own, independent of set_bound_scan_wide — which plane comes first follows set_bound_plane_filtered;
        the counters are bound_scan_wide_stats' (qv_index_set_bound_scan_wide_filtered)"""
        check(lib().qv_index_set_bound_scan_wide_filtered(self._h, self.BOUND_SCAN.get(mode, mode)))

    def bound_scan_wide_stats(self) -> dict:
        """survivors the last wide search passed to its re-score, wide searches handed back to the exact path, searches that took the wide
        form, whether the bfloat16 copy exists"""
        out = (C.c_uint64 * 4)()
        check(lib().qv_index_bound_scan_wide_stats(self._h, out))
        return {"candidates": int(out[0]), "hand_backs": int(out[1]), "searches": int(out[2]), "plane": bool(out[3])}

    def set_bound_scan_wide_mq(self, mode):
        """the wide form of the shared bound pass: ONE unfiltered call of 2 to 8 queries at 65 <= k <= 1024 (search, search_device, the short
        tail of a device batch): "auto" (the measured shapes: cosine / dot, k <= 1000, 2 - 4 queries from 1M rows of 768 dimensions, 5 - 8 queries from 3M,
        either from 10M rows of 128), "always" (whenever the shape applies), "never"; a knob of its own, independent of
        set_bound_scan_wide — which never reaches two or more queries, as this never reaches one — and of set_bound_scan; which plane comes
        first follows set_bound_plane_mq; the counters are bound_scan_wide_mq_stats' (qv_index_set_bound_scan_wide_mq)"""
        check(lib().qv_index_set_bound_scan_wide_mq(self._h, self.BOUND_SCAN.get(mode, mode)))

    def bound_scan_wide_mq_stats(self) -> dict:
        """the largest survivor count among the last wide shared pass's queries (each in the stage that answered it), queries handed back to
        the key-per-row path, queries that took the form, whether the bfloat16 copy exists"""
        out = (C.c_uint64 * 4)()
        check(lib().qv_index_bound_scan_wide_mq_stats(self._h, out))
        return {"candidates": int(out[0]), "hand_backs": int(out[1]), "searches": int(out[2]), "plane": bool(out[3])}

    BOUND_PLANE = {"auto": 0, "8bit": 1, "bf16": 2}

    def _set_bound_plane(self, form, mode):
        """one of the four plane knobs: form "" / "_filtered" / "_mq" / "_filtered_mq" names its setter (qv_index_set_bound_plane*)"""
        check(getattr(lib(), "qv_index_set_bound_plane" + form)(self._h, self.BOUND_PLANE.get(mode, mode)))

    def set_bound_plane(self, mode):
        """which plane a single unfiltered query's bound scan starts on: "auto" (the 8-bit plane from its measured shapes on), "8bit"
        (whenever the bound scan takes the search and the plane is held), "bf16" (qv_index_set_bound_plane)"""
        self._set_bound_plane("", mode)

    def set_bound_plane_filtered(self, mode):
        """which plane a single FILTERED query's bound scan starts on (search_masked, search_rowsets, search_where and their device forms):
        "auto" (the measured shapes), "8bit" (whenever the filtered bound scan takes the search and the plane is held), "bf16"; a knob of
        its own, independent of set_bound_plane (qv_index_set_bound_plane_filtered)"""
        self._set_bound_plane("_filtered", mode)

    def set_bound_plane_mq(self, mode):
        """which plane an unfiltered SHARED PASS of 2 - 8 queries starts on (search / search_device with 2 - 8 queries, the passes concurrent
        single-query callers share): "auto" (the measured shapes), "8bit" (whenever the bound scan takes the pass and the plane is held),
        "bf16"; a knob of its own, independent of set_bound_plane and set_bound_plane_filtered (qv_index_set_bound_plane_mq)"""
        self._set_bound_plane("_mq", mode)

    def set_bound_plane_filtered_mq(self, mode):
        """which plane a FILTERED shared pass of 2 - 8 queries starts on (search_masked, search_rowsets, search_where and their device forms
        with 2 - 8 queries, the passes that concurrent row-set or where-filter callers share): "auto" (the measured shapes), "8bit" (whenever
        the filtered bound scan takes the pass and the plane is held), "bf16"; a knob of its own, independent of set_bound_plane,
        set_bound_plane_filtered and set_bound_plane_mq (qv_index_set_bound_plane_filtered_mq)"""
        self._set_bound_plane("_filtered_mq", mode)

    def bound_scan8_stats(self) -> dict:
        """survivors of the last 8-bit stage, searches it handed on to the bfloat16 stage, searches that took it, whether the plane exists"""
        out = (C.c_uint64 * 4)()
        check(lib().qv_index_bound_scan8_stats(self._h, out))
        return {"candidates": int(out[0]), "hand_backs": int(out[1]), "searches": int(out[2]), "plane": bool(out[3])}

    BOUND_PLANE6 = {"auto": 0, "always": 1, "never": 2}

    def set_bound_plane6(self, mode):
        """whether a single unfiltered query that would start on the 8-bit plane starts on the 6-bit plane: "auto" (the measured shapes),
        "always" (whenever the 8-bit stage would be first and the plane is held), "never" (qv_index_set_bound_plane6)"""
        check(lib().qv_index_set_bound_plane6(self._h, self.BOUND_PLANE6.get(mode, mode)))

    def bound_scan6_stats(self) -> dict:
        """candidates the last 6-bit stage passed to the refine, searches it handed on to the bfloat16 stage, searches that took it, whether the plane exists"""
        out = (C.c_uint64 * 4)()
        check(lib().qv_index_bound_scan6_stats(self._h, out))
        return {"candidates": int(out[0]), "hand_backs": int(out[1]), "searches": int(out[2]), "plane": bool(out[3])}

    DEBUG_READ = {"rnorm": (0, np.float64), "rres": (1, np.float32), "plane": (2, np.uint16), "rowmaj16": (3, np.uint16),
                  "plane6": (4, np.uint8), "rres6": (5, np.float32), "rscale8": (6, np.float32), "plane8": (7, np.uint8), "rres8": (8, np.float32),
                  "rowmaj8": (9, np.int8), "rowmeta8": (10, np.dtype([("rnorm", np.float64), ("rscale8", np.float32), ("rres8", np.float32)]))}

    def debug_read(self, what: str) -> np.ndarray:
        """FOR TESTS (qv_index_debug_read): one of the arrays ingest derives per row, as the device holds it — "rnorm" (float64 per row
        slot), "rres" (float32 per row slot) or "plane" (the bfloat16 copy as uint16 words in ITS layout: the caller decodes it) — over
        the tiles in use; "rowmaj16": the row-order bfloat16 copy (graph_plane=True) as uint16 [rows, dim]; "rowmaj8": the row-order
        8-bit image (graph_plane8=True) as int8 [rows, dim]; "rowmeta8": its records, a structured array [rows] of rnorm, rscale8, rres8.  Raises
        QvError(QV_ERR_UNSUPPORTED) for an array this index does not keep."""
        code, dtype = self.DEBUG_READ[what]
        if what in ("rowmaj16", "rowmaj8", "rowmeta8"):
            out = np.empty((self.rows(),) if what == "rowmeta8" else (self.rows(), self.dim), dtype=dtype)
            check(lib().qv_index_debug_read(self._h, code, out.ctypes.data, out.nbytes))
            return out
        tiles = (self.rows() + 63) // 64
        per_tile = 2 * 64 * 8 * ((self.dim + 15) // 16) if what == "plane" else self.dim * 48 if what == "plane6" else self.dim * 64 if what == "plane8" else 64     # uint16 words of a tile of the copy: qv_index::bf16_tile_bytes() / 2 (qv_api_internal.h)
        out = np.empty(tiles * per_tile, dtype=dtype)
        check(lib().qv_index_debug_read(self._h, code, out.ctypes.data, out.nbytes))
        return out

    def set_filter(self, filter):
        """the batched path's filter kernel: "auto", "fp32" (fp32 MFMA chain), "bf16x3", "bf16x1", or "off" — exact scans only (qv_index_set_filter)"""
        check(lib().qv_index_set_filter(self._h, self.FILTERS.get(filter, filter)))

    FILTERED_BATCH = {"auto": 0, "always": 1, "never": 2}

    def set_filtered_batch(self, mode, sparse_ppm=None):
        """whether a call or shared pass of 9 or more FILTERED queries (search_rowsets, search_where; k <= 64) takes the batched path with a
        set per query: "auto" (the shapes measured faster), "always" (whenever the batched path takes the shape), "never" (the exact
        passes).  sparse_ppm: the share of the rows, in millionths, below which a query's set is handed back to the exact scan; None =
        the default, 0 = never (qv_index_set_filtered_batch)"""
        ppm = 0xFFFFFFFF if sparse_ppm is None else int(sparse_ppm)
        check(lib().qv_index_set_filtered_batch(self._h, self.FILTERED_BATCH.get(mode, mode), ppm))

    def filtered_batch_stats(self) -> dict:
        """queries that took the filtered batched path, queries it handed back (overflow, no bound, a failed guess), queries it handed back
        as sparse, batches (qv_index_filtered_batch_stats)"""
        out = (C.c_uint64 * 4)()
        check(lib().qv_index_filtered_batch_stats(self._h, out))
        return {"queries": int(out[0]), "hand_backs": int(out[1]), "sparse": int(out[2]), "batches": int(out[3])}

    # QV_BATCHED_FILTER_* of include/qv.h, by code
    BATCHED_FILTERS = ("mfma_f32", "bf16x3", "bf16x3_shared", "bf16rows", "w8x2", "w8x2_padded", "q64_plane", "q64_f32_rows")

    def batched_sample_plan(self, nq: int, k: int) -> dict:
        """the sample the batched path's plan chose for nq queries, k results: "rows" sample rows, every "group_step"-th 128-row group of
        the corpus — sample position i is corpus row (i // 128) * group_step * 128 + i % 128 — and the "rank" its bound is taken at
        (qv_batched_sample_plan)"""
        sr, gs, rk = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(lib().qv_batched_sample_plan(self._h, nq, k, C.byref(sr), C.byref(gs), C.byref(rk)))
        return {"rows": int(sr.value), "group_step": int(gs.value), "rank": int(rk.value)}

    def profile(self, enable: bool):
        check(lib().qv_index_profile(self._h, 1 if enable else 0))

    def profile_read(self):
        ms, n = C.c_double(0), C.c_uint64(0)
        check(lib().qv_index_profile_read(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)


class RowSet:
    """One ``qv_rowset``: a facet predicate's match set as a row bitmap on the index's device, uploaded once and named by handle in
    DeviceIndex.search_rowsets.  The index must outlive every search that names the set."""

    def __init__(self, index: DeviceIndex, mask_or_rows=None, *, rows=None):
        self._h = C.c_void_p()
        self._index = index                                # the index must outlive its sets
        if rows is not None and mask_or_rows is not None:
            raise ValueError("give a mask or rows=, not both")
        m = None if mask_or_rows is None else np.asarray(mask_or_rows)
        listed = m is not None and m.dtype != np.bool_ and m.dtype != np.uint64       # uint64 = packed mask words; row numbers of that dtype: rows=
        if rows is not None:
            m, listed = np.asarray(rows), True
            if m.size and (m.dtype.kind not in "iu" or int(m.min()) < 0 or int(m.max()) > 0xFFFFFFFF):
                raise ValueError("rows= must hold row numbers")
        words = None if (m is None or listed) else index._mask_words(m)
        check(lib().qv_rowset_create(C.byref(self._h), index.handle, None if words is None else words.ctypes.data))
        if listed and m.size:
            self.set_rows(m, True)

    @property
    def handle(self):
        return self._h

    def set_rows(self, rows, selected: bool = True):
        """add (selected) or drop the listed rows"""
        r = np.ascontiguousarray(rows, dtype=np.uint32).ravel()
        check(lib().qv_rowset_set_rows(self._h, r.ctypes.data, r.size, 1 if selected else 0))

    def count(self) -> int:
        """rows selected, dead ones included"""
        return int(lib().qv_rowset_count(self._h))

    def words(self) -> np.ndarray:
        """the bitmap as the DEVICE holds it, one uint64 per 64 rows of the index as it is now (qv_rowset_read); count() reads the host mirror"""
        out = np.zeros((self._index.rows() + 63) // 64, dtype=np.uint64)
        check(lib().qv_rowset_read(self._h, out.ctypes.data, out.size))
        return out

    SET_OPS = {"and": 0, "&": 0, "or": 1, "|": 1, "andnot": 2, "-": 2}

    def combine(self, a: "RowSet", b: "RowSet", op) -> "RowSet":
        """self = a OP b on the device, in place (qv_rowset_combine): "and", "or" or "andnot"; a or b may be self"""
        check(lib().qv_rowset_combine(self._h, a.handle, b.handle, self.SET_OPS[op] if isinstance(op, str) else int(op)))
        return self

    def _combined(self, other: "RowSet", op: str) -> "RowSet":
        if not isinstance(other, RowSet):
            return NotImplemented
        return RowSet(self._index).combine(self, other, op)

    def __and__(self, other):
        return self._combined(other, "and")

    def __or__(self, other):
        return self._combined(other, "or")

    def __sub__(self, other):
        return self._combined(other, "andnot")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().qv_rowset_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Column:
    """One ``qv_column``: a typed value per row of a DeviceIndex, on its device, for DeviceIndex.rowset_where.  The index must
    outlive the column."""

    def __init__(self, index: DeviceIndex, type):
        self._h = C.c_void_p()
        self._index = index
        self.type = DeviceIndex.COLUMN_TYPES[type.lower()] if isinstance(type, str) else int(type)
        check(lib().qv_column_create(C.byref(self._h), index.handle, self.type))

    @property
    def handle(self):
        return self._h

    def set(self, first_row: int, values, present=None):
        """values for rows [first_row, first_row + len(values)); present: a bool per value, False = the row has no value (None: all have)"""
        v = np.ascontiguousarray(values, dtype=np.float64 if self.type == _lib.QV_COL_F64 else np.uint32).ravel()
        p = None
        if present is not None:
            p = np.ascontiguousarray(np.asarray(present).ravel() != 0, dtype=np.uint8)
            if p.size != v.size:
                raise ValueError("present must have one entry per value")
        check(lib().qv_column_set(self._h, int(first_row), v.size, v.ctypes.data, None if p is None else p.ctypes.data))

    def rows(self) -> int:
        """one past the last row ever set"""
        return int(lib().qv_column_rows(self._h))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().qv_column_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceGraph:
    """An HNSW graph resident on the device over the rows of a DeviceIndex (qv_graph_* of include/qv.h):
    the whole of HNSW.Search (pkg/hnsw/hnsw.go:602-672) runs on the GPU, one wavefront per query.

    levels [n] int8 (-1 = tombstone), l0_deg [n], l0_links [n, max_m0]; upper levels as up_off [n] and
    up_links [n_blocks, 1 + max_m] (degree, links) — pass None for a single-layer graph."""

    def __init__(self, index: DeviceIndex, levels, l0_deg, l0_links, entry: int, cur_level: int = 0, up_off=None, up_links=None, max_m: int = 0):
        self.index = index
        self._g = C.c_void_p()
        levels = np.ascontiguousarray(levels, dtype=np.int8)
        l0_deg = np.ascontiguousarray(l0_deg, dtype=np.uint32)
        l0_links = np.ascontiguousarray(l0_links, dtype=np.uint32)
        n = levels.size
        if l0_deg.size != n or l0_links.ndim != 2 or l0_links.shape[0] != n:
            raise ValueError("levels, l0_deg and l0_links must describe the same nodes")
        if up_off is None:
            up_off = np.zeros(n, dtype=np.uint32); up_links = np.zeros((1, 1 + max(max_m, 1)), dtype=np.uint32); n_blocks = 0
        else:
            up_off = np.ascontiguousarray(up_off, dtype=np.uint32); up_links = np.ascontiguousarray(up_links, dtype=np.uint32); n_blocks = up_links.shape[0]
            max_m = up_links.shape[1] - 1
        self._g = C.c_void_p()
        check(lib().qv_graph_create(C.byref(self._g), index.handle, n, levels.ctypes.data, l0_links.shape[1], max(max_m, 1), l0_deg.ctypes.data,
                                    l0_links.ctypes.data, up_off.ctypes.data, up_links.ctypes.data, n_blocks, int(entry), int(cur_level)))

    @property
    def handle(self):
        return self._g

    def search(self, queries, k: int, ef_search: int, with_evals: bool = False):
        """rows [nq, k] uint32 (0xFFFFFFFF = unfilled), dist [nq, k] float32, count [nq] (< k: the graph search
        under-filled and the caller tops up like hnsw.go:676-710)"""
        q = _f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.index.dim:
            raise ValueError("query dimension %d does not match index dimension %d" % (q.shape[1], self.index.dim))
        nq = q.shape[0]
        rows = np.empty((nq, max(k, 1)), dtype=np.uint32); dist = np.empty((nq, max(k, 1)), dtype=np.float32)
        count = np.empty(nq, dtype=np.uint32); evals = np.empty(nq, dtype=np.uint32)
        check(lib().qv_graph_search(self._g, q.ctypes.data, nq, k, ef_search, rows.ctypes.data, dist.ctypes.data, count.ctypes.data, evals.ctypes.data))
        return (rows, dist, count, evals) if with_evals else (rows, dist, count)

    def search_device(self, d_queries: int, nq: int, k: int, ef_search: int, d_rows_out: int, d_dist_out: int, d_count_out: int,
                      d_evals_out: int = 0, stream: int = 0):
        """device pointers in and out, enqueued on `stream`, no sync; count 0xFFFFFFFE = redo that query through search()"""
        check(lib().qv_graph_search_device(self._g, d_queries, nq, k, ef_search, d_rows_out, d_dist_out, d_count_out, d_evals_out or None, stream or None))

    # ---- device-resident construction (qv_graph_create_empty / qv_graph_insert / qv_graph_export) ----
    @classmethod
    def empty(cls, index: DeviceIndex, capacity: int, m: int = 16, max_m0: int = 0, ef_construction: int = 200) -> "DeviceGraph":
        """a graph to be built on the device over the rows of `index` (which must keep a row-major copy)"""
        self = cls.__new__(cls)
        self.index = index
        self._g = C.c_void_p()
        check(lib().qv_graph_create_empty(C.byref(self._g), index.handle, capacity, m, max_m0, ef_construction))
        return self

    @classmethod
    def build(cls, index: DeviceIndex, levels, m: int = 16, max_m0: int = 0, ef_construction: int = 200, batch_max: int = 16384,
              ramp_div: int = 16) -> "DeviceGraph":
        """hnsw.HNSW.Insert (hnsw.go:266-468) for rows 0..len(levels)-1 of `index`, in batches on the device"""
        levels = np.ascontiguousarray(levels, dtype=np.int8)
        self = cls.empty(index, levels.size, m, max_m0, ef_construction)
        self.insert(0, levels, batch_max, ramp_div)
        return self

    def make_buildable(self, ef_construction: int = 200):
        """score the links of an uploaded (host-built) graph once so that insert() can extend it on the device"""
        check(lib().qv_graph_make_buildable(self._g, ef_construction))

    def insert(self, first_row: int, levels, batch_max: int = 16384, ramp_div: int = 16):
        levels = np.ascontiguousarray(levels, dtype=np.int8)
        check(lib().qv_graph_insert(self._g, first_row, levels.size, levels.ctypes.data, batch_max, ramp_div))

    def remove(self, nodes):
        """hnsw.HNSW.Delete (hnsw.go:741-842) for the listed nodes, as if one by one in list order, in place on the device
        (qv_graph_remove); the rows stay the caller's to remove from the index"""
        nodes = np.ascontiguousarray(np.atleast_1d(nodes), dtype=np.uint32)
        check(lib().qv_graph_remove(self._g, nodes.ctypes.data, nodes.size))

    def export_lists(self, nodes, levels):
        """(deg [n], links [n, max(max_m0, max_m)]) of the lists (nodes[i], levels[i]); degree 0 for a dead node or a level it lacks"""
        nodes = np.ascontiguousarray(np.atleast_1d(nodes), dtype=np.uint32)
        levels = np.ascontiguousarray(np.atleast_1d(levels), dtype=np.int32)
        if nodes.size != levels.size:
            raise ValueError("nodes and levels must have the same length")
        i = self.info()
        deg = np.zeros(nodes.size, dtype=np.uint32); links = np.zeros((nodes.size, max(i["max_m0"], i["max_m"])), dtype=np.uint32)
        check(lib().qv_graph_export_lists(self._g, nodes.ctypes.data, levels.ctypes.data, nodes.size, deg.ctypes.data, links.ctypes.data))
        return deg, links

    def info(self) -> dict:
        v = [C.c_uint32(0) for _ in range(5)]; lv = C.c_int(0)
        check(lib().qv_graph_info(self._g, *[C.byref(x) for x in v], C.byref(lv)))
        return {"n_nodes": v[0].value, "n_up_blocks": v[1].value, "max_m0": v[2].value, "max_m": v[3].value, "entry": v[4].value, "cur_level": lv.value}

    def stats(self) -> dict:
        sec = C.c_double(0); a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(lib().qv_graph_stats(self._g, C.byref(sec), C.byref(a), C.byref(b), C.byref(c)))
        return {"build_seconds": sec.value, "build_batches": a.value, "build_redo": b.value, "search_redo": c.value}

    REJECT_PLANE = {"auto": 0, "always": 1, "never": 2}

    def set_reject_plane(self, mode):
        """whether traversals reject neighbours on the index's row-order bfloat16 copy (DeviceIndex(..., rowmajor=True, graph_plane=True)):
        "auto" (where measured faster: cosine, 768 dimensions, 1M to below 2M nodes, 8192 queries or more, list sizes 64 to 256), "always" (wherever it applies: graph_reject_applies) or "never".  Results do not depend on it
        (qv_graph_set_reject_plane)."""
        check(lib().qv_graph_set_reject_plane(self._g, self.REJECT_PLANE.get(mode, mode)))

    def reject_stats(self) -> dict:
        """evaluations made in rejecting hops, those rejected on the copy, queries that finished unflagged in the rejecting form, and whether the
        graph's index holds the copy (qv_graph_reject_stats; waits for the device)"""
        out = (C.c_uint64 * 4)()
        check(lib().qv_graph_reject_stats(self._g, out))
        return {"evals": int(out[0]), "rejected": int(out[1]), "queries": int(out[2]), "plane": bool(out[3])}

    REJECT_IMAGE = {"auto": 0, "8bit": 1, "bf16": 2}

    def set_reject_image(self, mode):
        """which image a rejecting traversal starts on: "auto" (the 8-bit image only where the index holds it and it was measured faster: cosine, 768
        dimensions, 1M to below 2M nodes, 8192 queries or more, list sizes 64 to 256), "8bit" (the row-order 8-bit image wherever it is held — DeviceIndex(..., rowmajor=True, graph_plane8=True) — else the
        bfloat16 copy) or "bf16" (never the 8-bit image).  set_reject_plane keeps deciding whether a call rejects; results do not depend on
        either (qv_graph_set_reject_image)."""
        check(lib().qv_graph_set_reject_image(self._g, self.REJECT_IMAGE.get(mode, mode)))

    def reject8_stats(self) -> dict:
        """evaluations made in hops that rejected on the 8-bit image, those rejected on it, queries that finished unflagged in that form, and
        whether the graph's index holds the image (qv_graph_reject8_stats; waits for the device)"""
        out = (C.c_uint64 * 4)()
        check(lib().qv_graph_reject8_stats(self._g, out))
        return {"evals": int(out[0]), "rejected": int(out[1]), "queries": int(out[2]), "plane": bool(out[3])}

    def export(self):
        """(levels, l0_deg, l0_links [n, max_m0], up_off, up_links [blocks, 1 + max_m]) — the form qv_graph_create takes"""
        i = self.info()
        n, nb = i["n_nodes"], i["n_up_blocks"]
        levels = np.empty(n, dtype=np.int8); l0_deg = np.empty(n, dtype=np.uint32); l0_links = np.empty((n, i["max_m0"]), dtype=np.uint32)
        up_off = np.empty(n, dtype=np.uint32); up_links = np.zeros((nb, 1 + i["max_m"]), dtype=np.uint32)
        check(lib().qv_graph_export(self._g, levels.ctypes.data, l0_deg.ctypes.data, l0_links.ctypes.data, up_off.ctypes.data,
                                    up_links.ctypes.data if nb else None))
        return levels, l0_deg, l0_links, up_off, up_links

    def close(self):
        if getattr(self, "_g", None) is not None and self._g.value:
            lib().qv_graph_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GraphReplicas:
    """HNSW over the GPUs of a node: graph traversal is sequentially dependent (hnsw.go:471-580), so the graph does
    not shard by rows — REPLICAS ONLY: one complete index + graph per listed device, built from the same rows and levels (the
    device build is deterministic, so the replicas are identical), the queries of a batch cut into one contiguous slice per
    replica and walked concurrently.  A device may be listed more than once (two replicas on one GPU: how a 1-GPU box tests it)."""

    def __init__(self, rows, levels, metric="cosine", devices=(0,), m: int = 16, max_m0: int = 0, ef_construction: int = 200,
                 batch_max: int = 16384, ramp_div: int = 16):
        rows = _f32c(rows)
        self.dim = rows.shape[1]
        self.indexes, self.graphs = [], []
        for d in devices:
            idx = DeviceIndex(self.dim, metric, device=int(d), rowmajor=True)
            idx.add(rows)
            self.indexes.append(idx)
            self.graphs.append(DeviceGraph.build(idx, levels, m=m, max_m0=max_m0, ef_construction=ef_construction, batch_max=batch_max, ramp_div=ramp_div))

    def search(self, queries, k: int, ef_search: int):
        """-> (rows [nq, k], dist [nq, k], count [nq]): DeviceGraph.search of each query slice on its replica, concurrently"""
        from concurrent.futures import ThreadPoolExecutor
        q = _f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        nq, R = q.shape[0], len(self.graphs)
        cuts = [i * nq // R for i in range(R + 1)]
        jobs = [(g, q[cuts[i]:cuts[i + 1]]) for i, g in enumerate(self.graphs) if cuts[i + 1] > cuts[i]]
        with ThreadPoolExecutor(max_workers=max(len(jobs), 1)) as pool:           # ctypes drops the GIL: the replicas' calls overlap
            parts = list(pool.map(lambda job: job[0].search(job[1], k, ef_search), jobs))
        return tuple(np.concatenate([p[j] for p in parts]) for j in range(3))

    def close(self):
        for g in self.graphs:
            g.close()
        for i in self.indexes:
            i.close()
        self.graphs, self.indexes = [], []


class ShardedIndex:
    """One corpus over several GPUs behind ONE C-ABI handle (qv_sharded_* of include/qv.h): a shard (exact index) per device,
    one RCCL all-gather of the per-shard top-k per search, merge on the first device.  `devices` may repeat a device only
    with peer_copy=True (point-to-point exchange instead of the collective)."""

    def __init__(self, dim: int, metric="cosine", devices=(0,), rowmajor: bool = False, peer_copy: bool = False, bf16_rows: bool = False, scan_plane: bool = True, l2_scan_plane: bool = False,
                 graph_plane: bool = False, graph_plane8: bool = False):
        self._h = C.c_void_p()
        self.dim = int(dim)
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        flags = (_lib.QV_FLAG_ROWMAJOR if rowmajor else 0) | (_lib.QV_SHARDED_PEER_COPY if peer_copy else 0) | (_lib.QV_FLAG_BF16_ROWS if bf16_rows else 0) | (0 if scan_plane else _lib.QV_FLAG_NO_SCAN_PLANE) | (_lib.QV_FLAG_L2_SCAN_PLANE if l2_scan_plane else 0) | (_lib.QV_FLAG_GRAPH_PLANE if graph_plane else 0) | (_lib.QV_FLAG_GRAPH_PLANE8 if graph_plane8 else 0)
        check(lib().qv_sharded_create(C.byref(self._h), self.dim, metric_id(metric), devs, len(devices), flags))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().qv_sharded_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def shards(self) -> int:
        return int(lib().qv_sharded_shards(self._h))

    def size(self) -> int:
        return int(lib().qv_sharded_size(self._h))

    def shard_info(self, g: int) -> dict:
        dev = C.c_int(0); b, r, l = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(lib().qv_sharded_shard_info(self._h, g, C.byref(dev), C.byref(b), C.byref(r), C.byref(l)))
        return {"device": dev.value, "base": b.value, "rows": r.value, "live": l.value}

    def reserve(self, rows_total: int):
        check(lib().qv_sharded_reserve(self._h, rows_total))

    def add(self, rows) -> np.ndarray:
        """-> global row id of every added row"""
        rows = _f32c(rows)
        if rows.ndim == 1:
            rows = rows[None, :]
        if rows.shape[1] != self.dim:
            raise ValueError(f"vector dimension mismatch: expected {self.dim}, got {rows.shape[1]}")
        ids = np.empty(rows.shape[0], dtype=np.uint32)
        check(lib().qv_sharded_add(self._h, rows.ctypes.data, rows.shape[0], ids.ctypes.data))
        return ids

    def add_synthetic(self, seed: int, gen_row0: int, n: int):
        check(lib().qv_sharded_add_synthetic(self._h, seed, gen_row0, n))

    def remove(self, global_rows):
        r = np.ascontiguousarray(global_rows, dtype=np.uint32).ravel()
        check(lib().qv_sharded_remove(self._h, r.ctypes.data, r.size))

    def search(self, queries, k: int):
        q = _f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dimension mismatch: expected {self.dim}, got {q.shape[1]}")
        nq, kk = q.shape[0], max(int(k), 0)
        rows = np.full((nq, max(kk, 1)), 0xFFFFFFFF, dtype=np.uint32); dist = np.full((nq, max(kk, 1)), np.inf, dtype=np.float32)
        count = np.zeros(nq, dtype=np.uint32)
        check(lib().qv_sharded_search(self._h, q.ctypes.data, nq, kk, rows.ctypes.data, dist.ctypes.data, count.ctypes.data))
        return rows[:, :kk], dist[:, :kk], count

    def search_device(self, d_queries: int, nq: int, k: int, d_rows_out: int, d_dist_out: int, stream: int = 0):
        check(lib().qv_sharded_search_device(self._h, d_queries, nq, k, d_rows_out, d_dist_out, stream or None))

    def _q(self, queries):
        q = _f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dimension mismatch: expected {self.dim}, got {q.shape[1]}")
        return q

    def rows(self) -> int:
        return int(lib().qv_sharded_rows(self._h))

    def update(self, global_row: int, vec):
        vec = _f32c(vec)
        if vec.size != self.dim:
            raise ValueError(f"vector dimension mismatch: expected {self.dim}, got {vec.size}")
        check(lib().qv_sharded_update(self._h, int(global_row), vec.ctypes.data))

    def update_rows(self, global_rows, vecs):
        """overwrite the listed global rows in one call (qv_sharded_update_rows): what the loop of update() leaves"""
        rows, vecs = DeviceIndex._rows_vecs(self, global_rows, vecs)
        check(lib().qv_sharded_update_rows(self._h, rows.ctypes.data, rows.size, vecs.ctypes.data))

    def get_row(self, global_row: int) -> np.ndarray:
        out = np.empty(self.dim, dtype=np.float32)
        check(lib().qv_sharded_get_row(self._h, int(global_row), out.ctypes.data))
        return out

    def get_rows(self, global_rows) -> np.ndarray:
        r = np.ascontiguousarray(global_rows, dtype=np.uint32).ravel()
        out = np.empty((r.size, self.dim), dtype=np.float32)
        check(lib().qv_sharded_get_rows(self._h, r.ctypes.data, r.size, out.ctypes.data))
        return out

    def search_masked(self, queries, k: int, selected_global_rows):
        """exact top-k among the listed rows (global ids): the filtered search, qv_sharded_search_masked"""
        q = self._q(queries)
        sel = np.ascontiguousarray(selected_global_rows, dtype=np.uint32).ravel()
        nq, kk = q.shape[0], max(int(k), 0)
        rows = np.full((nq, max(kk, 1)), 0xFFFFFFFF, dtype=np.uint32); dist = np.full((nq, max(kk, 1)), np.inf, dtype=np.float32)
        count = np.zeros(nq, dtype=np.uint32)
        check(lib().qv_sharded_search_masked(self._h, q.ctypes.data, nq, kk, sel.ctypes.data, sel.size, rows.ctypes.data, dist.ctypes.data, count.ctypes.data))
        return rows[:, :kk], dist[:, :kk], count

    def search_negative(self, query, negative, k_fetch: int):
        """-> (rows [k_fetch], dist, neg_dist, count): qv_sharded_search_negative"""
        q, n = self._q(query), self._q(negative)
        kk = max(int(k_fetch), 0)
        rows = np.full(max(kk, 1), 0xFFFFFFFF, dtype=np.uint32); dist = np.full(max(kk, 1), np.inf, dtype=np.float32)
        nd = np.full(max(kk, 1), np.inf, dtype=np.float32); cnt = C.c_uint32(0)
        check(lib().qv_sharded_search_negative(self._h, q.ctypes.data, n.ctypes.data, kk, rows.ctypes.data, dist.ctypes.data, nd.ctypes.data, C.byref(cnt)))
        return rows[:kk], dist[:kk], nd[:kk], int(cnt.value)

    def distance_rows(self, query, global_rows) -> np.ndarray:
        q = self._q(query)
        r = np.ascontiguousarray(global_rows, dtype=np.uint32).ravel()
        out = np.empty(r.size, dtype=np.float32)
        check(lib().qv_sharded_distance_rows(self._h, q.ctypes.data, r.ctypes.data, r.size, out.ctypes.data))
        return out

    def set_bound_scan(self, mode):
        check(lib().qv_sharded_set_bound_scan(self._h, DeviceIndex.BOUND_SCAN.get(mode, mode)))

    def bound_scan_stats(self) -> dict:
        out = (C.c_uint64 * 4)()
        check(lib().qv_sharded_bound_scan_stats(self._h, out))
        return {"candidates": int(out[0]), "hand_backs": int(out[1]), "searches": int(out[2]), "plane": bool(out[3])}

    def set_bound_plane6(self, mode):
        check(lib().qv_sharded_set_bound_plane6(self._h, DeviceIndex.BOUND_PLANE6.get(mode, mode)))

    def set_bound_plane(self, mode):
        check(lib().qv_sharded_set_bound_plane(self._h, DeviceIndex.BOUND_PLANE.get(mode, mode)))

    def set_bound_plane_mq(self, mode):
        check(lib().qv_sharded_set_bound_plane_mq(self._h, DeviceIndex.BOUND_PLANE.get(mode, mode)))

    def bound_scan8_stats(self) -> dict:
        out = (C.c_uint64 * 4)()
        check(lib().qv_sharded_bound_scan8_stats(self._h, out))
        return {"candidates": int(out[0]), "hand_backs": int(out[1]), "searches": int(out[2]), "plane": bool(out[3])}

    def set_filter(self, filter):
        check(lib().qv_sharded_set_filter(self._h, DeviceIndex.FILTERS.get(filter, filter)))

    def profile_read_shard(self, g: int):
        ms, n = C.c_double(0), C.c_uint64(0)
        check(lib().qv_sharded_profile_read_shard(self._h, g, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def sync(self):
        check(lib().qv_sharded_sync(self._h))

    def profile(self, enable: bool):
        check(lib().qv_sharded_profile(self._h, 1 if enable else 0))

    def profile_read(self) -> dict:
        a, b, c = C.c_double(0), C.c_double(0), C.c_double(0); n = C.c_uint64(0)
        check(lib().qv_sharded_profile_read(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        m = max(int(n.value), 1)
        return {"searches": int(n.value), "scan_ms": a.value / m, "exchange_ms": b.value / m, "merge_ms": c.value / m}


def sharded_plan_add(rows_per_shard, n: int) -> np.ndarray:
    have = np.ascontiguousarray(rows_per_shard, dtype=np.uint64)
    give = np.zeros(have.size, dtype=np.uint64)
    check(lib().qv_sharded_plan_add(have.ctypes.data, have.size, n, give.ctypes.data))
    return give


def graph_reject_applies(metric, dim: int, n_nodes: int, nq: int, ef_search: int, cus: int, mode="auto", has_plane: bool = True, has_tombstones: bool = False,
                         max_m0: int = 32) -> bool:
    """the traversal dispatch's own rule: whether a DeviceGraph.search call of nq queries takes the form that rejects neighbours on the
    row-order bfloat16 copy (qv_graph_reject_applies)"""
    rc = lib().qv_graph_reject_applies(metric_id(metric), dim, n_nodes, nq, ef_search, cus, DeviceGraph.REJECT_PLANE.get(mode, mode), 1 if has_plane else 0,
                                       1 if has_tombstones else 0, max_m0)
    if rc < 0:
        check(rc)
    return bool(rc)


def graph_reject_image_applies(metric, dim: int, n_nodes: int, nq: int, ef_search: int, cus: int, mode="auto", has_plane: bool = True, has_tombstones: bool = False,
                               max_m0: int = 32, has_image8: bool = True, image_mode="auto") -> int:
    """the traversal dispatch's own rule: the form a DeviceGraph.search call of nq queries takes — 0 no rejecting form, 1 rejecting on the
    row-order bfloat16 copy, 2 on the row-order 8-bit image (qv_graph_reject_image_applies)"""
    rc = lib().qv_graph_reject_image_applies(metric_id(metric), dim, n_nodes, nq, ef_search, cus, DeviceGraph.REJECT_PLANE.get(mode, mode), 1 if has_plane else 0,
                                             1 if has_tombstones else 0, max_m0, 1 if has_image8 else 0, DeviceGraph.REJECT_IMAGE.get(image_mode, image_mode))
    if rc < 0:
        check(rc)
    return int(rc)


def graph_batch_size(nodes_linked: int, batch_max: int, ramp_div: int) -> int:
    return int(lib().qv_graph_batch_size(nodes_linked, batch_max, ramp_div))


def random_levels(n: int, max_level: int = 16, seed: int = 1) -> np.ndarray:
    """n draws of randomLevel (hnsw.go:716-738: p = 0.25 per extra level, at most min(MaxLevel, 10) draws, < MaxLevel) from a
    SplitMix64 stream — the level law stays on the host side of the boundary, where the reference keeps its RNG
    (hnsw.go:248 seeds it from the wall clock; a seed here makes builds repeatable)."""
    attempts = min(max_level, 10)
    out = np.empty(n, dtype=np.int8)
    filled, draw0 = 0, 0
    while filled < n:
        # a block of the draw stream u_j = f(seed + (j+1) * gamma); a node consumes draws up to its first failure (u >= 0.25)
        # or `attempts` successes, whichever comes first
        m = max(2 * (n - filled), 1024)
        j = np.arange(draw0 + 1, draw0 + m + 1, dtype=np.uint64)
        with np.errstate(over="ignore"):
            x = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + j * np.uint64(0x9E3779B97F4A7C15)
            x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            x = x ^ (x >> np.uint64(31))
        ok = ((x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)) < 0.25
        fails = np.flatnonzero(~ok)
        if fails.size == 0:
            raise RuntimeError("level draw stream has no failure in a block")
        runs = np.diff(np.concatenate(([-1], fails))) - 1          # successes before each failure
        if (runs >= attempts).any():                                # a run of >= `attempts` successes: walk the block draw by draw
            pos = 0
            while filled < n and pos < m:
                level = 0
                while level < attempts and pos < m and ok[pos]:
                    level += 1; pos += 1
                if level < attempts:
                    if pos >= m:
                        break                                       # node straddles the block: redo it in the next one
                    pos += 1                                        # the failing draw
                out[filled] = min(level, max_level - 1); filled += 1
                last_end = pos
            draw0 += last_end
            continue
        take = min(runs.size, n - filled)
        out[filled:filled + take] = np.minimum(runs[:take], max_level - 1)
        filled += take
        draw0 += int(fails[take - 1]) + 1
    return out


def merge_topk_device(d_dist_lists: int, d_row_lists: int, n_lists: int, k: int, d_rows_out: int, d_dist_out: int, stream: int = 0):
    check(lib().qv_merge_topk_device(d_dist_lists, d_row_lists, n_lists, k, d_rows_out, d_dist_out, stream))


def merge_topk_shards_device(d_packed_lists: int, d_bases: int, n_lists: int, nq: int, k: int, d_rows_out: int, d_dist_out: int, stream: int = 0):
    """merge of the packed per-shard buffers ([n_lists][nq][2][k]: k local rows, k distance bits); outputs [nq][k], rows global"""
    check(lib().qv_merge_topk_shards_device(d_packed_lists, d_bases, n_lists, nq, k, d_rows_out, d_dist_out, stream or None))


def distance_pairs(metric, a, b, device: int = 0) -> np.ndarray:
    a, b = _f32c(a), _f32c(b)
    if a.ndim == 1:
        a = a[None, :]
    if b.ndim == 1:
        b = b[None, :]
    if a.shape != b.shape:
        raise ValueError("vectors must have the same length")  # distances.go:13-15
    out = np.empty(a.shape[0], dtype=np.float32)
    check(lib().qv_distance_pairs(metric_id(metric), a.ctypes.data, b.ctypes.data, a.shape[0], a.shape[1], out.ctypes.data, device))
    return out


def runtime_info() -> str:
    """which HIP runtime and RCCL the process bound (qv_runtime_info)"""
    buf = C.create_string_buffer(1024)
    check(lib().qv_runtime_info(buf, 1024))
    return buf.value.decode()


def distance_pair(metric, a, b) -> float:
    """one DistanceFunc call on the host (qv_distance_pair): the kernels' per-pair arithmetic compiled for the CPU"""
    a, b = _f32c(a).ravel(), _f32c(b).ravel()
    if a.size != b.size:
        raise ValueError("vectors must have the same length")  # distances.go:13-15 (the reference panics)
    out = C.c_float(0)
    check(lib().qv_distance_pair(metric_id(metric), a.ctypes.data, b.ctypes.data, a.size, C.byref(out)))
    return float(np.float32(out.value))


def device_info(device: int = 0):
    name = C.create_string_buffer(256)
    cus, mem = C.c_int(0), C.c_uint64(0)
    check(lib().qv_device_info(device, name, 256, C.byref(cus), C.byref(mem)))
    return {"name": name.value.decode(), "cus": cus.value, "hbm_bytes": mem.value}
