"""The argument checks of every search entry point of include/qv.h, through the C ABI itself (quiver_amd._lib.lib() and ctypes: the
Python wrappers catch some of these before the library sees them): the return code and the exact text of qv_last_error(), in the
order the checks fire.  Two tables, one for the host-pointer forms and one for the *_device forms; two indexes, cosine x 16 dimensions:
A, first empty and then with 70 rows (one full tile and one partial), and B, which supplies a foreign set and a foreign column.
Every pointer passed as non-null is a real allocation of the right size, and every case returns before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import quiver_amd
from quiver_amd._lib import lib
from quiver_amd.device_index import pack_where

pytestmark = pytest.mark.gpu

DIM, ROWS, NQ, K = 16, 70, 3, 4
OK, INVALID, K_NOT_POSITIVE, UNSUPPORTED = 0, -1, -3, -8
NULL_INDEX, K_MSG = "index is null", "k must be positive"
BATCHED_MSG = "the MFMA batched path does not apply to this index/query shape; use qv_index_search_device"
WIDE_MSG = "the device-pointer form takes k <= 64 (longer lists need a set's host mirror): got 65"

# form -> (symbol, its arguments behind the index, the message for a null input, the message for a null output)
HOST = {
    "search": ("qv_index_search", ("queries", "nq", "k", "rows_out", "dist_out", "count_out"), "queries/count_out is null", "rows_out/dist_out is null"),
    "batched": ("qv_index_search_batched", ("queries", "nq", "k", "rows_out", "dist_out", "count_out"), "queries/count_out is null", "rows_out/dist_out is null"),
    "masked": ("qv_index_search_masked", ("queries", "nq", "k", "mask", "rows_out", "dist_out", "count_out"), "queries/mask/count_out is null", "rows_out/dist_out is null"),
    "rowsets": ("qv_index_search_rowsets", ("queries", "nq", "k", "sets", "rows_out", "dist_out", "count_out"), "queries/sets/count_out is null", "rows_out/dist_out is null"),
    "where": ("qv_index_search_where", ("queries", "nq", "k", "filters", "rows_out", "dist_out", "count_out"), "queries/filters/count_out is null", "rows_out/dist_out is null"),
    "negative": ("qv_index_search_negative", ("query", "negative", "k", "rows_out", "dist_out", "neg_dist_out", "count_out"),
                 "query/negative/count_out is null", "rows_out/dist_out/neg_dist_out is null"),
}
DEVICE = {
    "device": ("qv_index_search_device", ("d_queries", "nq", "k", "d_rows_out", "d_dist_out", "stream")),
    "rowsets_device": ("qv_index_search_rowsets_device", ("d_queries", "nq", "k", "sets", "d_rows_out", "d_dist_out", "stream")),
    "where_device": ("qv_index_search_where_device", ("d_queries", "nq", "k", "filters", "d_rows_out", "d_dist_out", "stream")),
    "batched_device": ("qv_index_search_batched_device", ("d_queries", "nq", "k", "d_rows_out", "d_dist_out", "d_redo_flags_out", "stream")),
}
INPUTS = ("queries", "query", "negative", "count_out", "mask", "sets", "filters")
OUTPUTS = ("rows_out", "dist_out", "neg_dist_out")
DEVICE_POINTERS = ("d_queries", "d_rows_out", "d_dist_out", "d_redo_flags_out")
NOTHING = {"nq": 0, **{a: None for a in INPUTS + OUTPUTS + DEVICE_POINTERS}}

# (forms, state of A, what differs from a valid call, return code, message): None = a null pointer; "index": the handle itself;
# "foreign" / "bad": a set or a column of B for query 0 / an operator that is no predicate for query 1; IN / OUT: the form's own
# message of HOST; a message that ends in "..." is a prefix; "counts": every count_out word must read 0 afterwards
IN, OUT = "<null input>", "<null output>"
ALL, SIZED = tuple(HOST), tuple(f for f in HOST if f != "negative")
HOST_CASES = [
    (ALL, "empty", {"index": None}, INVALID, NULL_INDEX),
    (SIZED, "empty", NOTHING, OK, None),
    *[(ALL, state, {a: None}, INVALID, IN) for state in ("empty", "full") for a in INPUTS],
    (ALL, "empty", {"k": 0, "rows_out": None}, OK, "counts"),
    (("rowsets",), "empty", {"sets": "foreign"}, INVALID, "row set of query 0 belongs to another index"),
    (("where",), "empty", {"filters": "foreign"}, OK, "counts"),
    (ALL, "full", {"index": None}, INVALID, NULL_INDEX),
    (SIZED, "full", NOTHING, OK, None),
    (ALL, "full", {"k": 0, "rows_out": None}, K_NOT_POSITIVE, K_MSG),
    *[(ALL, "full", {a: None}, INVALID, OUT) for a in OUTPUTS],
    (("rowsets",), "full", {"sets": "foreign"}, INVALID, "row set of query 0 belongs to another index"),
    (("rowsets",), "full", {"sets": "foreign", "k": 0, "rows_out": None}, INVALID, "row set of query 0 belongs to another index"),
    (("where",), "full", {"filters": "foreign"}, INVALID, "filter of query 0: cols[0] belongs to another index"),
    (("where",), "full", {"filters": "bad"}, INVALID, "filter of query 1: ..."),
    (("where",), "full", {"filters": "bad", "k": 0}, K_NOT_POSITIVE, K_MSG),
    (("where",), "full", {"filters": "bad", "dist_out": None}, INVALID, OUT),
]
EVERY = tuple(DEVICE)
DEVICE_CASES = [
    (EVERY, {"index": None}, INVALID, NULL_INDEX),
    (EVERY, NOTHING, OK, None),
    *[(EVERY, {a: None}, INVALID, "null device pointer") for a in DEVICE_POINTERS],
    (("rowsets_device",), {"sets": None}, INVALID, "sets is null"),
    (("where_device",), {"filters": None}, INVALID, "filters is null"),
    (("rowsets_device",), {"sets": None, "d_queries": None}, INVALID, "null device pointer"),
    (("where_device",), {"filters": None, "k": 0}, INVALID, "filters is null"),
    (("rowsets_device",), {"sets": "foreign", "k": 0}, INVALID, "row set of query 0 belongs to another index"),
    (EVERY, {"k": 0}, K_NOT_POSITIVE, K_MSG),
    (("where_device",), {"k": 65}, UNSUPPORTED, WIDE_MSG),
    (("where_device",), {"k": 65, "filters": "bad"}, UNSUPPORTED, WIDE_MSG),
    (("where_device",), {"filters": "bad"}, INVALID, "filter of query 1: ..."),
    (("batched_device",), {}, UNSUPPORTED, BATCHED_MSG),
]


class World:
    def __init__(self):
        rng = np.random.default_rng(20)
        self.vectors = rng.standard_normal((ROWS, DIM)).astype(np.float32)
        self.a = quiver_amd.DeviceIndex(DIM, "cosine")
        self.b = quiver_amd.DeviceIndex(DIM, "cosine")
        self.b.add(self.vectors)
        self.foreign_set, self.foreign_col, self.col = self.b.rowset(None), self.b.column("u32"), self.a.column("u32")
        self.keep = []

    def close(self):
        for x in (self.foreign_set, self.foreign_col, self.col, self.a, self.b):
            x.close()

    def sets(self, how):
        arr = (C.c_void_p * NQ)()
        if how == "foreign":
            arr[0] = self.foreign_set.handle.value
        return arr

    def filters(self, how):
        per_query = [[], [], []]
        if how == "foreign":
            per_query[0] = [(self.foreign_col, "present", None)]
        if how == "bad":
            per_query[1] = [(self.col, 99, None)]
        arr, keep = pack_where(per_query)
        self.keep = [keep]
        return arr

    def call(self, symbol, names, host, diff):
        """one call: valid arguments of the right sizes (host: numpy; device: torch tensors), then what the case changes"""
        import torch
        nq, k = diff.get("nq", NQ), diff.get("k", K)
        n_out = NQ * max(k, 1)
        if host:
            new = {"float": lambda n: np.ones(n, dtype=np.float32), "uint": lambda n: np.full(n, 7, dtype=np.uint32)}
        else:
            new = {"float": lambda n: torch.ones(n, dtype=torch.float32, device="cuda"), "uint": lambda n: torch.full((n,), 7, dtype=torch.int32, device="cuda")}
        args = {"index": self.a.handle, "nq": nq, "k": k, "stream": None}
        for name in names:
            if name in ("queries", "d_queries"):
                args[name] = new["float"](NQ * DIM)
            elif name in ("query", "negative"):
                args[name] = new["float"](DIM)
            elif name in ("dist_out", "neg_dist_out", "d_dist_out"):
                args[name] = new["float"](n_out)
            elif name in ("rows_out", "d_rows_out"):
                args[name] = new["uint"](n_out)
            elif name in ("count_out", "d_redo_flags_out"):
                args[name] = new["uint"](1 if "query" in names else NQ)
            elif name == "mask":
                args[name] = np.full((ROWS + 63) // 64, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
            elif name == "sets":
                args[name] = self.sets(diff.get("sets", "none"))
            elif name == "filters":
                args[name] = self.filters(diff.get("filters", "none"))
        for name, value in diff.items():
            if value is None and name in args:
                args[name] = None
        count = args.get("count_out")

        def raw(name):
            x = args[name]
            if isinstance(x, np.ndarray):
                return x.ctypes.data_as(C.POINTER(C.c_uint32)) if symbol == "qv_index_search_negative" and name == "count_out" else x.ctypes.data
            return x.data_ptr() if isinstance(x, torch.Tensor) else x
        rc = getattr(lib(), symbol)(raw("index"), *[raw(name) for name in names])
        return rc, (lib().qv_last_error() or b"").decode(), count


def _mismatch(got_rc, got_msg, count, rc, message):
    if got_rc != rc:
        return "returned %d (%r), not %d" % (got_rc, got_msg, rc)
    if message == "counts":
        return None if count is not None and not count.any() else "count_out reads %r, not zeros" % (count,)
    if rc == OK or message is None:
        return None
    if message.endswith("..."):
        return None if got_msg.startswith(message[:-3]) else "message %r does not start with %r" % (got_msg, message[:-3])
    return None if got_msg == message else "message %r, not %r" % (got_msg, message)


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def test_host_forms_report_every_bad_argument_in_their_order(world):
    """A is empty for the first part of the table; then its 70 rows are added"""
    wrong = []
    for state in ("empty", "full"):
        if state == "full":
            world.a.add(world.vectors)
        assert world.a.size() == (0 if state == "empty" else ROWS)
        for forms, when, diff, rc, message in HOST_CASES:
            for form in forms if when == state else ():
                symbol, names, null_in, null_out = HOST[form]
                if diff is not NOTHING and not all(name in names or name == "index" for name in diff):
                    continue                                # (the argument is not one of this form's)
                want = {IN: null_in, OUT: null_out}.get(message, message)
                bad = _mismatch(*world.call(symbol, names, True, diff), rc, want)
                if bad:
                    wrong.append("%s, %s index, %r: %s" % (symbol, state, diff, bad))
    assert not wrong, "\n".join(wrong)


def test_device_forms_report_every_bad_argument_in_their_order(world):
    if world.a.size() == 0:
        world.a.add(world.vectors)
    wrong = []
    for forms, diff, rc, message in DEVICE_CASES:
        for form in forms:
            symbol, names = DEVICE[form]
            if diff is not NOTHING and not all(name in names or name == "index" for name in diff):
                continue                                    # (the argument is not one of this form's)
            bad = _mismatch(*world.call(symbol, names, False, diff), rc, message)
            if bad:
                wrong.append("%s, %r: %s" % (symbol, diff, bad))
    assert not wrong, "\n".join(wrong)
