"""Device-pointer entry points on busy caller streams: the protocol (Call, Lane, run) and the inputs of every case, with their decoys.

The protocol.  Everything between "busy work" and "read back" is enqueued on one non-default torch stream, and the host waits for nothing
in between:
  1. warm-up   the same call with the same shape, once, on this stream, and a wait: workspace, tickets, visited tables and per-context
               buffers then have their final size (a call that has to grow them drains the stream first, by design: qv_api.cpp,
               stream_workspace — and then nothing after it tests anything)
  2. buffers   DECOY inputs in the buffer the call reads, the true inputs in a second device buffer, every output buffer filled with a
               pattern (rows 0xA5A5A5A5, distances -1.0)
  3. busy      BUSY_REPS times a = a @ a * 1e-3 on 4096 x 4096 float32, then the event busy_done
  4. inputs    a device-to-device copy of the true inputs over the decoys: the true inputs exist only BEHIND the busy block
  5. the call  with the stream's handle
  6. busy?     busy_done.query() as soon as the call has returned: an entry point that does not synchronise returns while the block runs
  7. reads     the decoys are copied back over the inputs: a library that reads its inputs later than stream order sees decoys
  8. writes    clone()s of the outputs on the stream: results that land later than stream order leave the pattern in the clones
  9. read back .cpu() of the clones
Several calls of one Lane are enqueued back to back behind ONE busy block; several Lanes (a stream, a block, buffers each) take turns
call by call (run).  A decoy is an ordinary finite input of the same shape — a stale read gives a plausible wrong answer, never a fault —
and tests/test_busy_streams_cpu.py proves, without a device, that for every query of every case the decoy's expected first result
differs from the true input's: a stale read cannot pass.

The size of the busy block (measured on an MI355X; a block on an otherwise idle stream, timed with events; enqueues timed with
time.perf_counter around the warm call):
  B = 37.3 - 38.0 ms for 40 repetitions, 9.7 - 9.8 ms for 10: 0.95 ms per repetition (one 4096^3 float32 product and its scaling)
  E = 147 us: search_where_device with 11 queries (its filters are packed in Python inside the call); the sharded handle's search
      takes 53 - 75 us, the flat routes 8 - 63 us, a traversal 9 - 26 us, the batched call of 297 queries 47 - 53 us
  BUSY_REPS = 40: B = 38 ms = 258 x E, where B >= 10 x E is asked for (the factor covers a host thread descheduled on a shared machine;
  2 repetitions would meet it — 40 leave room for a slower host and cost a test 38 ms).  Every call documented as not synchronising
  returned while its block was running, at the first attempt, in every run these figures are from.

Expected results never come from the call under test: tests/_oracle.py (exact_search, distance, the HNSW restatement) and, for the
merges, numpy's sort by (distance, row)."""
import functools
import os
import time
from collections import namedtuple

import numpy as np

import quiver_amd
from tests import _oracle as O, _route as R

ROW_PATTERN, DIST_PATTERN = 0xA5A5A5A5, -1.0
BUSY_REPS = 40
NO_ROW = 0xFFFFFFFF
DECOY = 500_000                                              # a decoy's seed is the true input's plus this (plus the case's salt)


# ---- the protocol -----------------------------------------------------------------------------------------------------------------------

class Call:
    """one device-form call: fn(ins, outs, stream) takes device addresses (the order of `inputs` / `outputs`) and the stream's handle.
    inputs: [(true, decoy)] numpy arrays (float32 / uint32); outputs: [(shape, "rows" | "dist")].  warm=False: the call is NOT made
    beforehand (it grows something on purpose, or changes the index); then: called on the host as soon as the call has returned."""

    def __init__(self, name, fn, inputs, outputs, warm=True, then=None):
        self.name, self.fn, self.inputs, self.outputs, self.warm, self.then = name, fn, inputs, outputs, warm, then
        self.busy = None; self.enqueue_s = None; self.got = None

    def _alloc(self):
        import torch
        self.true_dev = [_to_dev(t) for t, _ in self.inputs]
        self.decoy_dev = [_to_dev(d) for _, d in self.inputs]
        self.buf = [torch.empty_like(t) for t in self.true_dev]
        self.outs = [torch.empty(shape, dtype=torch.int32 if kind == "rows" else torch.float32, device="cuda") for shape, kind in self.outputs]

    def _arm(self):
        for b, d in zip(self.buf, self.decoy_dev):
            b.copy_(d)
        for o, (_, kind) in zip(self.outs, self.outputs):
            o.fill_(ROW_PATTERN - (1 << 32) if kind == "rows" else DIST_PATTERN)

    def _launch(self, stream):
        self.fn([b.data_ptr() for b in self.buf], [o.data_ptr() for o in self.outs], stream)


def _to_dev(x):
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


class Lane:
    """a caller stream: its busy block, its calls and their buffers"""

    def __init__(self, calls, reps=BUSY_REPS):
        import torch
        self.calls, self.reps = list(calls), reps
        self.st = torch.cuda.Stream()
        with torch.cuda.stream(self.st):
            self.a0 = torch.randn(4096, 4096, device="cuda")
            for c in self.calls:
                c._alloc()
        self.st.synchronize()

    def warm(self):
        import torch
        with torch.cuda.stream(self.st):
            for c in self.calls:
                if c.warm:
                    c._arm()
                    c._launch(self.st.cuda_stream)
        self.st.synchronize()

    def arm(self):
        import torch
        with torch.cuda.stream(self.st):
            for c in self.calls:
                c._arm()
            self.busy_start = torch.cuda.Event(enable_timing=True); self.busy_done = torch.cuda.Event(enable_timing=True)
            self.busy_start.record(self.st)
            a = self.a0
            for _ in range(self.reps):
                a = a @ a * 1e-3                                  # keeps the stream busy while the calls are enqueued
            self.busy_done.record(self.st)
            for c in self.calls:
                for b, t in zip(c.buf, c.true_dev):
                    b.copy_(t, non_blocking=True)                 # the true inputs: only behind the block, in stream order

    def launch(self, i):
        import torch
        c = self.calls[i]
        with torch.cuda.stream(self.st):
            t0 = time.perf_counter()
            c._launch(self.st.cuda_stream)
            c.enqueue_s = time.perf_counter() - t0
            c.busy = not self.busy_done.query()
        if c.then is not None:
            c.then()

    def finish(self):
        import torch
        with torch.cuda.stream(self.st):
            for c in self.calls:
                for b, d in zip(c.buf, c.decoy_dev):
                    b.copy_(d, non_blocking=True)                 # a read later than stream order sees these
            clones = [[o.clone() for o in c.outs] for c in self.calls]   # a write later than stream order leaves the pattern in these
            for c, cl in zip(self.calls, clones):
                c.got = [x.cpu().numpy().view(np.uint32) if kind == "rows" else x.cpu().numpy() for x, (_, kind) in zip(cl, c.outputs)]
        self.block_ms = self.busy_start.elapsed_time(self.busy_done)
        for c in self.calls:
            print("busy-stream call %-28s returned %s, enqueue %7.1f us, block %6.1f ms" % (c.name, "BUSY" if c.busy else "idle", c.enqueue_s * 1e6, self.block_ms))


def run(lanes_of_calls, reps=BUSY_REPS, after_warm=None):
    """lanes_of_calls: a list of calls per lane.  Warm-ups, then every lane's buffers, block and inputs, then the calls in turns over the
    lanes (A, B, A, B, ...) without any wait, then every lane's copies back.  after_warm: called between the warm-ups and the rest."""
    lanes = [Lane(calls, reps) for calls in lanes_of_calls]
    for l in lanes:
        l.warm()
    if after_warm is not None:
        after_warm()
    for l in lanes:
        l.arm()
    for i in range(max(len(l.calls) for l in lanes)):
        for l in lanes:
            if i < len(l.calls):
                l.launch(i)
    for l in lanes:
        l.finish()
    return lanes


def returned_busy(once, tries=3):
    """the "no synchronisation" contract: once() runs a case (asserting its results every time) and answers whether its call returned while
    the stream was busy; a host thread may be descheduled, so up to `tries` runs — one of them must have returned busy"""
    for _ in range(tries):
        if once():
            return
    raise AssertionError("the call returned only after its stream's busy block had finished, %d times out of %d" % (tries, tries))


def measure_block_ms(reps):
    """the busy block on an otherwise idle stream, by events"""
    import torch
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a0 = torch.randn(4096, 4096, device="cuda")
        out = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.synchronize()
            e0.record(st)
            a = a0
            for _ in range(reps):
                a = a @ a * 1e-3
            e1.record(st)
            st.synchronize()
            out.append(e0.elapsed_time(e1))
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------

def queries(seed, nq, dim):
    return np.random.default_rng(seed).standard_normal((nq, dim)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def corpus(seed, n, dim):
    rows = O.gen_rows(seed, 0, n, dim)
    rows.setflags(write=False)
    return rows


def tiles_mq64(cus=R.CUS):
    """the fewest tiles with 16 per workgroup slot: the matrix-core scan's floor (as tests/test_gpu_flat_route.py finds it)"""
    t = 1
    while t < 16 * R.scan_grid(t, cus):
        t += 1
    return t


class SearchCase(namedtuple("SearchCase", "name metric n dim nq k mode plane corpus_seed seed salt dead masks")):
    """a top-k search over gen_rows(corpus_seed): `dead` rows tombstoned, query q restricted to masks[q] (None: every row)"""

    def rows(self):
        return corpus(self.corpus_seed, self.n, self.dim)

    def live(self):
        live = np.ones(self.n, bool)
        if self.dead is not None:
            live[self.dead] = False
        return live

    def true(self):
        return [queries(self.seed, self.nq, self.dim)]

    def decoy(self):
        return [queries(self.seed + DECOY + self.salt, self.nq, self.dim)]

    def valid(self, inputs):
        return inputs[0].shape == (self.nq, self.dim) and inputs[0].dtype == np.float32 and bool(np.isfinite(inputs[0]).all()) and bool((np.abs(inputs[0]) < 100).all())

    def expect(self, inputs):
        """-> [(rows, dist)] per query, the oracle's"""
        live, mid = self.live(), quiver_amd.metric_id(self.metric)
        out = []
        for q in range(self.nq):
            alive = live if self.masks is None or self.masks[q] is None else live & self.masks[q]
            out.append(O.exact_search(mid, self.rows(), inputs[0][q], self.k, alive=alive.astype(np.uint8)))
        return out

    def first(self, inputs):
        return [int(r[0]) for r, _ in self.expect(inputs)]

    def check(self, rows, dist, want, where=""):
        """rows / dist [nq, k] against the oracle's lists, bit for bit, padded past each list"""
        for q, (ro, do) in enumerate(want):
            w = ro.size
            assert rows[q, :w].tolist() == ro.tolist(), (self.name, where, q, rows[q, :8].tolist(), ro[:8].tolist())
            assert dist[q, :w].tobytes() == do.tobytes(), (self.name, where, q)
            assert (rows[q, w:] == NO_ROW).all() and np.isposinf(dist[q, w:]).all(), (self.name, where, q)


def search_case(name, metric, n, dim, nq, k, mode="auto", plane="auto", corpus_seed=None, seed=None, salt=0, dead=None, masks=None):
    corpus_seed = 20261017 + n if corpus_seed is None else corpus_seed
    seed = hash_name(name) if seed is None else seed
    return SearchCase(name, metric, n, dim, nq, k, mode, plane, corpus_seed, seed, salt or SALTS.get(name, 0), dead, masks)


# decoy seeds moved on for the cases whose first draw shared a first result with the true input (tests/test_busy_streams_cpu.py proves the rest)
SALTS = {"where-5": 1, "where-11": 2, "graph-40-ef64": 1, "graph-40-ef64-b": 1}


def hash_name(name):
    """a small stable number from a case's name (Python's hash() changes from run to run)"""
    return sum((i + 1) * b for i, b in enumerate(name.encode())) % 100_000


# 1. every flat route: tests/test_gpu_flat_route.py's unfiltered shapes, and the paths above k = 64
def flat_cases(cus=R.CUS):
    big = tiles_mq64(cus) * 64
    return [search_case("bound-1", "cosine", 600, 16, 1, 10, "always"), search_case("bound_mq-2", "cosine", 600, 16, 2, 10, "always"),
            search_case("bound_mq-5", "cosine", 600, 16, 5, 10, "always"), search_case("bound8-1", "cosine", 600, 16, 1, 10, "always", "8bit"),
            search_case("never-1", "cosine", 600, 16, 1, 10, "never"), search_case("never-4", "cosine", 600, 16, 4, 10, "never"),
            search_case("never-1-k17", "cosine", 600, 16, 1, 17, "never"), search_case("never-4-k17", "cosine", 600, 16, 4, 17, "never"),
            search_case("ten-rows", "cosine", 10, 16, 1, 10),
            search_case("wide-1", "cosine", 2000, 256, 1, 10), search_case("wide-4", "cosine", 2000, 256, 4, 10), search_case("wide-4-k17", "cosine", 2000, 256, 4, 17),
            search_case("mq64-40", "cosine", big, 16, 40, 10),
            search_case("l1-1", "l1", 600, 16, 1, 10), search_case("l1-1-k17", "l1", 600, 16, 1, 17), search_case("l1-200-k17", "l1", 200, 16, 1, 17),
            search_case("k100-1", "cosine", 9000, 16, 1, 100), search_case("k200-5", "cosine", 9000, 16, 5, 200), search_case("k8500-1", "cosine", 9000, 16, 1, 8500)]


FLAT_ROUTES = {"bound-1": R.BOUND, "bound_mq-2": R.BOUND_MQ, "bound_mq-5": R.BOUND_MQ, "bound8-1": R.BOUND8_FIRST, "never-1": R.SMALL, "never-4": R.SMALL,
               "never-1-k17": R.FUSED, "never-4-k17": R.MQ, "ten-rows": R.SMALL, "wide-1": R.SPLIT, "wide-4": R.SMALL, "wide-4-k17": R.SPLIT_MQ, "mq64-40": R.MQ64,
               "l1-1": R.SMALL, "l1-1-k17": R.FUSED, "l1-200-k17": R.TWO_LAUNCH}


def flat_route(c, cus=R.CUS, has_plane=None, has_plane8=None):
    """qv_scan_route's answer for a case of k <= 64 (the planes: as a cosine / dot index of 16-dimension steps keeps them by default)"""
    planes = int(c.metric in ("cosine", "dot") and c.dim % 16 == 0)
    return R.library_route(quiver_amd.metric_id(c.metric), c.dim, c.n, c.nq, c.k, 1, R.ALWAYS if c.mode == "always" else R.NEVER if c.mode == "never" else R.AUTO,
                           {"auto": 0, "8bit": 1, "bf16": 2}[c.plane], planes if has_plane is None else int(has_plane), planes if has_plane8 is None else int(has_plane8), R.NO_FILTER, cus=cus)


# 2. the batched path: the smallest corpus qv_index_search_batched_device takes (batched_supported in qv_batched.hip: 32 768 rows, 9 queries
# under the bfloat16 filters, a million query-rows), 64 queries and a call whose tail of 41 runs as a second call on the stream
BATCHED_ROWS, BATCHED_DIM, BATCHED_METRIC = 32_768, 64, "dot"


def batched_cases():
    return [search_case("batched-64", BATCHED_METRIC, BATCHED_ROWS, BATCHED_DIM, 64, 10), search_case("batched-297", BATCHED_METRIC, BATCHED_ROWS, BATCHED_DIM, 297, 10)]


# 3. row sets and where-filters
ROWSET_N, ROWSET_DIM = 20_011, 64


def _rowset_masks():
    rng = np.random.default_rng(1)
    return [rng.random(ROWSET_N) < f for f in (0.3, 0.01)]


def rowset_cases():
    dead = np.arange(2, ROWSET_N, 41, dtype=np.uint32)
    m = _rowset_masks()
    return [search_case("rowsets-1", "cosine", ROWSET_N, ROWSET_DIM, 1, 10, corpus_seed=8600, dead=dead, masks=[m[1]]),
            search_case("rowsets-5-k200", "cosine", ROWSET_N, ROWSET_DIM, 5, 200, corpus_seed=8600, dead=dead, masks=[m[0], m[0], m[0], None, m[1]])]


def filtered_batch_case():
    """40 queries with a set each on the batched corpus: a shape qv_batched_applies_filtered takes under "always" """
    rng = np.random.default_rng(2)
    dense = [rng.random(BATCHED_ROWS) < f for f in (0.5, 0.3)]
    return search_case("rowsets-40-filtered-batch", BATCHED_METRIC, BATCHED_ROWS, BATCHED_DIM, 40, 10, masks=[None if q % 3 == 2 else dense[q % 3] for q in range(40)])


WHERE_N, WHERE_DIM, WHERE_FEW = 2051, 128, 3


@functools.lru_cache(maxsize=None)
def where_columns():
    """an F64 and a U32 column over the where-corpus: (values, present) each, and the tombstones; WHERE_FEW live rows carry the U32 value 4000"""
    rng = np.random.default_rng(91)
    dead = np.flatnonzero(rng.random(WHERE_N) < 0.05).astype(np.uint32)
    f = rng.integers(0, 20, WHERE_N).astype(np.float64) + 0.25
    pf = rng.random(WHERE_N) < 0.5
    u = rng.integers(0, 300, WHERE_N).astype(np.uint32)
    pu = rng.random(WHERE_N) < 0.5
    live_rows = np.setdiff1d(np.arange(WHERE_N, dtype=np.uint32), dead)
    few = np.concatenate([rng.choice(live_rows[:-1], WHERE_FEW - 1, replace=False), live_rows[-1:]])      # one of them in the ragged last tile
    u[few] = 4000; pu[few] = True
    return (f, pf), (u, pu), dead


WHERE_FILTERS = [[("u", "eq", 4000)], [("f", "lt", 6.5)], None, [("f", "ge", 3.0), ("u", "lt", 100)], [("u", "ge", 150)], [("f", "lt", 6.5)],
                 [("u", "gt", 20), ("f", "le", 15.25)], [("f", "gt", 10.0)], [("u", "le", 200)], [("f", "ge", 1.0)], [("u", "lt", 250), ("f", "gt", 2.0)]]


def where_mask(preds):
    (f, pf), (u, pu), _ = where_columns()
    m = np.ones(WHERE_N, bool)
    for col, op, lit in preds or []:
        v, p = (f, pf) if col == "f" else (u, pu)
        m &= p & {"eq": v == lit, "lt": v < lit, "le": v <= lit, "gt": v > lit, "ge": v >= lit}[op]
    return m


def where_cases():
    dead = where_columns()[2]
    return [search_case("where-%d" % nq, "cosine", WHERE_N, WHERE_DIM, nq, k, corpus_seed=9228, dead=dead, masks=[where_mask(p) for p in WHERE_FILTERS[:nq]])
            for nq, k in ((1, 10), (5, 64), (11, 10))]


# 4. listed-row distances and the merges
class DistCase(namedtuple("DistCase", "name metric n dim n_ids seed")):
    def _in(self, seed):
        rng = np.random.default_rng(seed)
        return [rng.standard_normal(self.dim).astype(np.float32), rng.integers(0, self.n, self.n_ids).astype(np.uint32)]

    def true(self):
        return self._in(self.seed)

    def decoy(self):
        return self._in(self.seed + DECOY)

    def valid(self, inputs):
        return bool(np.isfinite(inputs[0]).all()) and inputs[1].dtype == np.uint32 and bool((inputs[1] < self.n).all()) and inputs[1].size == self.n_ids

    def expect(self, inputs):
        rows, mid = corpus(20261017 + self.n, self.n, self.dim), quiver_amd.metric_id(self.metric)
        return np.array([O.distance(mid, inputs[0], rows[r]) for r in inputs[1]], dtype=np.float32)

    def first(self, inputs):
        return [self.expect(inputs)[:1].tobytes()]


def dist_case():
    return DistCase("distance_rows-300", "cosine", 600, 16, 300, 4100)


class MergeCase(namedtuple("MergeCase", "name n_lists k seed")):
    """qv_merge_topk_device: [n_lists][k] distances and rows, every list in (distance, row) order"""

    def _in(self, seed):
        rng = np.random.default_rng(seed)
        d = rng.random((self.n_lists, self.k)).astype(np.float32)
        r = rng.integers(0, 600, (self.n_lists, self.k)).astype(np.uint32)
        for l in range(self.n_lists):
            o = np.lexsort((r[l], d[l])); d[l] = d[l][o]; r[l] = r[l][o]
        return [d, r]

    def true(self):
        return self._in(self.seed)

    def decoy(self):
        return self._in(self.seed + DECOY)

    def valid(self, inputs):
        return bool(np.isfinite(inputs[0]).all()) and bool((inputs[1] < 600).all())

    def expect(self, inputs):
        d, r = inputs[0].ravel(), inputs[1].ravel()
        o = np.lexsort((r, d))[:self.k]
        return r[o], d[o]

    def first(self, inputs):
        r, d = self.expect(inputs)
        return [(int(r[0]), d[:1].tobytes())]


class MergeShardsCase(namedtuple("MergeShardsCase", "name n_lists nq k seed")):
    """qv_merge_topk_shards_device: [n_lists][nq][2][k] words (k shard-local rows, k distance bits) and the shards' first global rows"""

    def _in(self, seed):
        rng = np.random.default_rng(seed)
        d = np.sort(rng.random((self.n_lists, self.nq, self.k)).astype(np.float32), axis=2)
        r = rng.integers(0, 600, (self.n_lists, self.nq, self.k)).astype(np.uint32)
        packed = np.stack([r, d.view(np.uint32)], axis=2)
        bases = (np.arange(self.n_lists, dtype=np.uint32) * np.uint32(1000 + seed % 7 * 100)).astype(np.uint32)
        return [np.ascontiguousarray(packed), bases]

    def true(self):
        return self._in(self.seed)

    def decoy(self):
        return self._in(self.seed + DECOY)

    def valid(self, inputs):
        p, b = inputs
        return p.shape == (self.n_lists, self.nq, 2, self.k) and bool(np.isfinite(p[:, :, 1].view(np.float32)).all()) and bool((p[:, :, 0] < 600).all()) and bool((b < 100_000).all())

    def expect(self, inputs):
        p, b = inputs
        out = []
        for q in range(self.nq):
            r = (p[:, q, 0] + b[:, None]).ravel(); d = p[:, q, 1].view(np.float32).ravel()
            o = np.lexsort((r, d))[:self.k]
            out.append((r[o], d[o]))
        return out

    def first(self, inputs):
        return [(int(r[0]), d[:1].tobytes()) for r, d in self.expect(inputs)]


def merge_cases():
    return [MergeCase("merge-2x10", 2, 10, 4200), MergeCase("merge-64x64", 64, 64, 4201), MergeShardsCase("merge_shards-3x5x10", 3, 5, 10, 4202)]


# 5. add_device: the rows are the input
class AddCase(namedtuple("AddCase", "name metric n dim n_new seed")):
    def true(self):
        return [queries(self.seed, self.n_new, self.dim)]

    def decoy(self):
        return [queries(self.seed + DECOY, self.n_new, self.dim)]

    def valid(self, inputs):
        return inputs[0].shape == (self.n_new, self.dim) and bool(np.isfinite(inputs[0]).all())

    def corpus_after(self, inputs):
        return np.concatenate([corpus(20261017 + self.n, self.n, self.dim), inputs[0]])

    def probe(self):
        """the queries the host form is asked right after the call: the first three NEW rows themselves, and two ordinary ones"""
        return np.concatenate([self.true()[0][:3], queries(self.seed + 1, 2, self.dim)])

    def expect(self, inputs, k=10):
        mid = quiver_amd.metric_id(self.metric)
        return [O.exact_search(mid, self.corpus_after(inputs), q, k) for q in self.probe()]

    def first(self, inputs):
        return [r.tobytes() for r in inputs[0]]                   # (the rows ARE the values: get_rows returns them)


def add_case():
    return AddCase("add_device-200", "cosine", 600, 16, 200, 4300)


# 6. graph traversals
@functools.lru_cache(maxsize=None)
def fixture_graph():
    g = np.load(os.path.join(O.ROOT, "tests", "golden", "hnsw_3kx32_cosine.npz"))
    return {k: g[k] for k in g.files}


def fixture_oracle(ef):
    g = fixture_graph()
    n, dim = int(g["n"]), int(g["dim"])
    h = O.HNSW(0, dim, M=int(g["M"]), efConstruction=int(g["efConstruction"]), efSearch=ef, maxLevel=int(g["maxLevel"]), seed=int(g["seed"]))
    h.load_graph(corpus(int(g["corpus_seed"]), n, dim), g["levels"], g["l0_links"].shape[1], g["up_links"].shape[1] - 1, g["l0_deg"], g["l0_links"], g["up_off"], g["up_links"],
                 int(g["entry"]), int(g["cur_level"]))
    return h


EDIT_N, EDIT_DIM, EDIT_M, EDIT_M0, EDIT_EFC, EDIT_LEVELS, EDIT_SEED, EDIT_BM, EDIT_RD = 800, 32, 8, 16, 40, 16, 9, 64, 8


def edit_rows():
    return corpus(31337, EDIT_N + 1, EDIT_DIM)


def edit_levels():
    from quiver_amd.device_index import random_levels
    return random_levels(EDIT_N + 1, EDIT_LEVELS, EDIT_SEED)


def edit_oracle():
    """the graph tests/test_gpu_graph_remove.py builds on both sides (DeviceGraph.build == the oracle's insert_batch on the same schedule)"""
    from tests.test_oracle_hnsw import batch_schedule
    h = O.HNSW(0, EDIT_DIM, M=EDIT_M, maxM0=EDIT_M0, efConstruction=EDIT_EFC, maxLevel=EDIT_LEVELS, seed=EDIT_SEED)
    rows, done = edit_rows(), 0
    for b in batch_schedule(EDIT_N, EDIT_BM, EDIT_RD):
        h.insert_batch(rows[done:done + b]); done += b
    return h


def edit_removed(pre):
    """the nodes the edit removes: every query's nearest node before the edit, so that no answer survives it"""
    return list(dict.fromkeys(int(r[0]) for r, _ in pre))


class GraphCase(namedtuple("GraphCase", "name graph nq k ef seed salt")):
    """a traversal of the committed fixture graph ("fixture") or of the graph under edit ("edit")"""

    def dim(self):
        return int(fixture_graph()["dim"]) if self.graph == "fixture" else EDIT_DIM

    def true(self):
        return [queries(self.seed, self.nq, self.dim())]

    def decoy(self):
        return [queries(self.seed + DECOY + self.salt, self.nq, self.dim())]

    def valid(self, inputs):
        return inputs[0].shape == (self.nq, self.dim()) and bool(np.isfinite(inputs[0]).all()) and bool((np.abs(inputs[0]) < 100).all())

    def expect(self, inputs, h=None):
        """-> [(rows, dist)] per query: what HNSW.Search's graph search found, up to k (hnsw.go:602-672), on the oracle's copy of the graph.
        Where that under-fills, the reference tops up by brute force (hnsw.go:676-710) and the oracle with it, which the device leaves to
        its caller: asked for fewer results than the search found, the oracle walks the same graph search (ef stays efSearch) and returns
        its first results untouched, and a top-up shows in its count of distance evaluations — so the longest list without one is taken"""
        h = h or (fixture_oracle(self.ef) if self.graph == "fixture" else edit_oracle())
        h.set_ef_search(self.ef)
        assert self.k <= self.ef
        out = []
        for q in inputs[0]:
            _, _, walk = h.search(q, 1, with_evals=True)
            for kk in range(self.k, 0, -1):
                ro, do, evals = h.search(q, kk, with_evals=True)
                if evals == walk:
                    break
            out.append((ro, do))
        return out

    def first(self, inputs):
        return [int(r[0]) for r, _ in self.expect(inputs)]

    def check(self, rows, dist, count, want, where=""):
        """the device form's counts and lists against the oracle's graph search; a query flagged for the exact-heap kernel (0xFFFFFFFE) is
        the host form's — none is expected here"""
        assert (count != 0xFFFFFFFE).all(), (self.name, where, np.flatnonzero(count == 0xFFFFFFFE).tolist())
        for q, (ro, do) in enumerate(want):
            c = int(count[q])
            assert 1 <= c == ro.size, (self.name, where, q, c, ro.size)
            assert rows[q, :c].tolist() == ro.tolist(), (self.name, where, q, rows[q, :c].tolist(), ro.tolist())
            assert dist[q, :c].tobytes() == do.tobytes(), (self.name, where, q)


def graph_cases():
    return [GraphCase("graph-1-ef64", "fixture", 1, 10, 64, 4400, 0), GraphCase("graph-40-ef64", "fixture", 40, 10, 64, 4401, SALTS["graph-40-ef64"]),
            GraphCase("graph-40-ef300", "fixture", 40, 10, 300, 4402, 0), GraphCase("graph-400-ef64", "fixture", 400, 10, 64, 4403, 0),
            GraphCase("graph-1-ef64-b", "fixture", 1, 10, 64, 4404, 0), GraphCase("graph-40-ef64-b", "fixture", 40, 10, 64, 4405, SALTS["graph-40-ef64-b"]),
            GraphCase("graph-edit-8", "edit", 8, 10, 64, 4406, 0)]


# 7. the sharded handle: 3 co-located shards over 2000 x 64 rows
SHARDED_N, SHARDED_DIM = 2000, 64


def sharded_cases():
    return [search_case("sharded-%d-k%d%s" % (nq, k, tag), "cosine", SHARDED_N, SHARDED_DIM, nq, k, corpus_seed=7)
            for nq, k, tag in ((1, 10, ""), (5, 10, ""), (40, 10, ""), (5, 100, ""), (1, 10, "-b"), (5, 10, "-b"))]


# 8. two streams in turns on the 600 x 16 index: (nq, k, bound mode, plane mode) of the four calls A1, B1, A2, B2
INTERLEAVED = {"bound": [(1, 10, "always", "auto")] * 4, "bound_mq": [(5, 10, "always", "auto"), (2, 10, "always", "auto")] * 2, "bound8_first": [(1, 10, "always", "8bit")] * 4,
               "small": [(1, 10, "never", "auto")] * 4, "mq": [(4, 17, "never", "auto")] * 4,
               "bound+bound_mq": [(1, 10, "always", "auto"), (5, 10, "always", "auto"), (2, 10, "always", "auto"), (1, 10, "always", "auto")]}


def interleaved_cases(kind):
    return [search_case("turns-%s-%d" % (kind, i), "cosine", 600, 16, nq, k, mode, plane) for i, (nq, k, mode, plane) in enumerate(INTERLEAVED[kind])]


# 9. growth while earlier work is in flight
# (a warm call, the call behind it that needs a larger workspace).  On 9000 x 16 (141 tiles, 36 lists: qv_api.cpp search_ws_bytes, and
# stream_workspace keeps 1.5 x what was asked): 1 query, k = 10 asks for some 14 KB; 32 queries for 36 * 4 * 32 * 10 * 8 = 369 KB of lists;
# 1 query at k = 200 for a key per row slot, 141 * 64 * 8 = 72 KB, and the selection's state; 8 queries at k = 200 for eight times those
# keys, 578 KB, more than the 32-query call's 1.5 x 375 KB.  The test does not rest on this arithmetic: it asserts that the second call waited.
GROWTH_PAIRS = (("growth-1", "growth-32"), ("growth-1", "growth-1-k200"), ("growth-32", "growth-8-k200"))


def growth_cases():
    return [search_case("growth-1", "cosine", 9000, 16, 1, 10), search_case("growth-32", "cosine", 9000, 16, 32, 10),
            search_case("growth-1-k200", "cosine", 9000, 16, 1, 200), search_case("growth-8-k200", "cosine", 9000, 16, 8, 200)]


def all_cases(cus=R.CUS):
    out = flat_cases(cus) + batched_cases() + rowset_cases() + [filtered_batch_case()] + where_cases() + [dist_case()] + merge_cases() + [add_case()] + graph_cases() + sharded_cases()
    for kind in INTERLEAVED:
        out += interleaved_cases(kind)
    return out + growth_cases()
