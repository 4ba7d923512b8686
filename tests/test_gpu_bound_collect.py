"""The bound scan's collect (bound_collect behind k_bound_collect and k_bound_collect_mq; quiver_amd/csrc/qv_bound_scan.hip): a workgroup gathers
the rows with d_lo <= H of its chunks in LDS and reserves their slots in the list with one atomic per flush.  A lost or doubled slot shows only
where every candidate matters, so the inputs are TIES: many exact copies of the query's nearest row, every other row far away (the negated
row plus noise).  Every copy is a candidate and a survivor of every stage: the stages' counts must be the CPU model's (a doubled or dropped
slot moves a count), and the k lowest row numbers among the copies are the answer (a dropped one is a wrong row).  Every case asserts the
model's counts first (the inputs are what they are chosen to be), forces its route by the index's setters, reads which stage answered from
the counters and compares rows and float32 bits with the CPU oracle.

The model: the stages' intervals come from the reference models of tests/_bound.py, _bound8.py and _bound6.py over the corpus's DISTINCT rows,
and are spread over the corpus by row; H, the rows passed on and the hand-back are decided here as those models decide them (the k-th
smallest upper bound; d_lo <= H).  At a few thousand rows every row is distinct; the one large corpus repeats a small pool of far rows."""
import numpy as np
import pytest

import quiver_amd
from tests import _bound as B
from tests import _bound6 as B6
from tests import _bound8 as B8
from tests import _oracle as O

pytestmark = pytest.mark.gpu

CHUNK = 2048                                       # kCollectChunk: lower-bound words a workgroup looks at per step
GRID = 512                                         # kBoundCollectGrid: the collect's workgroups at the most
FLUSH_OVER = 1024                                  # kCollectBuf - kCollectChunk: a workgroup that holds more flushes before its next chunk
CAP, CAP6 = B.CAND_CAP, B6.CAND_CAP6
REFINE_BATCH = 16                                  # kRefineBatch
KS = (1, 10, 64)


class Ties:
    """rows [n, dim]: the rows `copies` hold ONE row exactly, `medium` hold it with a little noise of their own (candidates of the 6-bit
    stage, not of the 8-bit one), every other row is its negation plus noise; the query is that row, slightly off.  pool: the far rows
    repeat that many distinct ones (None: each its own)."""

    def __init__(self, dim, n, copies, seed, medium=(), pool=None):
        near = O.gen_rows(seed, 0, 1, dim)[0]
        rng = np.random.default_rng(seed)
        sd = float(near.std())
        m = n if pool is None else pool
        far = (-near[None, :] + 0.5 * sd * rng.standard_normal((m, dim))).astype(np.float32)
        med = (near[None, :] + 0.22 * sd * rng.standard_normal((len(medium), dim))).astype(np.float32)
        self.uniq = np.ascontiguousarray(np.concatenate([near[None, :], far, med]))
        self.src = 1 + np.arange(n) % m
        self.src[np.asarray(medium, np.int64)] = 1 + m + np.arange(len(medium))
        self.src[np.asarray(copies, np.int64)] = 0
        self.rows = np.ascontiguousarray(self.uniq[self.src])
        self.copies = np.sort(np.asarray(copies, np.int64))
        self.q = (near + 0.05 * sd * rng.standard_normal(dim)).astype(np.float32)
        self.dim, self.n = dim, n
        self._state, self._iv = {}, {}
        for a in (self.uniq, self.src, self.rows, self.copies, self.q):
            a.setflags(write=False)

    def intervals(self, stage, q):
        """(d_lo, d_hi, unsure) of every row of the corpus for one query on one plane ("6", "8", "bf16"), cosine"""
        key = (stage, q.tobytes())
        if key not in self._iv:
            if stage not in self._state:
                self._state[stage] = {"6": B6.RowState6, "8": B8.RowState8, "bf16": B.RowState}[stage](self.uniq)
            st = self._state[stage]
            m = {"6": B6.reference6, "8": B8.reference8, "bf16": B.reference}[stage](B.COSINE, st, q, 1)
            assert B.query_ok(B.chain_norm(q), self.dim)
            self._iv[key] = tuple(m[f][self.src] for f in ("lo", "hi", "unsure"))
        return self._iv[key]

    def stage(self, stage, k, alive=None, q=None):
        """one stage for one k over the rows `alive` -> (the rows it passes on [n] bool, their number)"""
        lo, hi, unsure = self.intervals(stage, self.q if q is None else q)
        live = np.ones(self.n, bool) if alive is None else np.asarray(alive, bool)
        his = hi[live & ~unsure]
        assert len(his) >= k                                               # a finite H
        H = np.partition(his, k - 1)[k - 1]
        passed = live & (unsure | (lo <= H))
        return passed, int(passed.sum())

    def index(self):
        idx = quiver_amd.DeviceIndex(self.dim, "cosine")
        idx.add(self.rows)
        assert idx.bound_scan6_stats()["plane"] and idx.bound_scan8_stats()["plane"] and idx.bound_scan_stats()["plane"]
        return idx

    def answer(self, k, alive=None, q=None):
        kw = {} if alive is None else {"alive": np.asarray(alive).astype(np.uint8)}
        return O.exact_search(B.COSINE, self.rows, self.q if q is None else q, k, **kw)


def stats(idx):
    return idx.bound_scan6_stats(), idx.bound_scan8_stats(), idx.bound_scan_stats()


def increments(s0, s1):
    (a0, b0, c0), (a1, b1, c1) = s0, s1
    return {"took6": a1["searches"] - a0["searches"], "back6": a1["hand_backs"] - a0["hand_backs"], "cand6": a1["candidates"],
            "took8": b1["searches"] - b0["searches"], "back8": b1["hand_backs"] - b0["hand_backs"], "cand8": b1["candidates"],
            "took": c1["searches"] - c0["searches"], "back": c1["hand_backs"] - c0["hand_backs"], "cand": c1["candidates"]}


def counted(idx, call):
    s0 = stats(idx)
    r, d, c = call()
    return (r, d, c), increments(s0, stats(idx))


def single(idx, q, k, six):
    """one unfiltered query with the 8-bit plane forced and the 6-bit stage forced (six) or off"""
    idx.set_bound_scan("always"); idx.set_bound_plane("8bit"); idx.set_bound_plane6("always" if six else "never")
    return counted(idx, lambda: idx.search(q, k))


def same(got, want, j=0):
    (r, d, c), (er, ed) = got, want
    w = len(er)
    return int(c[j]) == w and np.array_equal(r[j][:w], er) and np.array_equal(d[j][:w].view(np.uint32), ed.view(np.uint32))


def check_single(t, idx, k, six, where):
    """the model's counts, the device's, the stage that answered, the oracle's rows and bits; k <= copies: the k lowest copies"""
    p6, n6 = t.stage("6", k) if six else (None, 0)
    p8, n8 = t.stage("8", k, p6)
    assert n8 <= CAP and n6 <= CAP6
    if k <= len(t.copies):
        assert n8 == len(t.copies) and (not six or n6 >= n8), (where, k, n6, n8)
    got, inc = single(idx, t.q, k, six)
    print("%s k %d six %d: candidates %d (model %d), survivors %d (model %d)" % (where, k, six, inc["cand6"] if six else 0, n6, inc["cand8"], n8))
    assert inc["took8"] == 1 and inc["back8"] == 0 and inc["took"] == 1 and inc["back"] == 0 and inc["took6"] == (1 if six else 0) and inc["back6"] == 0, (where, k, inc)
    assert inc["cand8"] == n8 and inc["cand"] == n8 and (not six or inc["cand6"] == n6), (where, k, inc, n6, n8)
    er, ed = t.answer(k)
    if k <= len(t.copies):
        assert np.array_equal(er, t.copies[:k])
    assert same(got, (er, ed)), (where, k, got[0], er)


# ---- 1. one chunk, full --------------------------------------------------------------------------------------------------------------------
_CASES = {}


def case1(name):
    if name not in _CASES:
        n = 4096 + 37
        copies = np.arange(1024, 2048) if name == "dense" else np.arange(0, n, 65)
        _CASES[name] = Ties(64, n, copies, 9100 if name == "dense" else 9101)
    return _CASES[name]


@pytest.mark.parametrize("six", [True, False])
@pytest.mark.parametrize("name", ["dense", "every65th"])
def test_one_chunk_full_and_one_candidate_per_wave(name, six):
    """dense: rows 1024 .. 2047 are copies — every thread of one workgroup finds its second request full, 1024 rows gathered in one chunk; every65th: no ballot holds two, and every wave
    of the corpus has one"""
    t = case1(name)
    if name == "every65th":
        assert len(t.copies) == 64 and len(np.unique(t.copies // 64)) == 64
    idx = t.index()
    for k in KS:
        check_single(t, idx, k, six, name)
    idx.close()


# ---- 2. a flush inside the walk ------------------------------------------------------------------------------------------------------------
def test_a_flush_inside_a_workgroups_walk():
    """just over GRID chunks: workgroups 0 - 2 walk two chunks, the others one.  Workgroup 1 finds its first chunk full of copies — more than
    FLUSH_OVER, so it flushes before its second chunk — and 300 in the second: a second, partial flush at the end of its walk"""
    n = GRID * CHUNK + 2 * CHUNK + 37
    assert (n + 63) // 64 * 64 > GRID * CHUNK + 2 * CHUNK and CHUNK > FLUSH_OVER
    second = (GRID + 1) * CHUNK
    copies = np.concatenate([np.arange(CHUNK, 2 * CHUNK), second + 3 * np.arange(300)])
    assert copies.max() < second + CHUNK and len(copies) <= CAP
    t = Ties(64, n, copies, 9200, pool=251)
    idx = t.index()
    for k in (10, 64):
        check_single(t, idx, k, True, "two flushes")
    check_single(t, idx, 10, False, "two flushes")
    idx.close()


# ---- 3. at the capacity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over", [0, 1])
def test_at_the_lists_capacity_and_one_over(over):
    """8-bit first, 8192 rows: exactly kBoundCandCap candidates are answered; one more is handed on, through the bfloat16 stage (the same
    count) to the exact scan"""
    n, k = 8192, 10
    copies = np.arange(0, n, 2)[:CAP] if not over else np.concatenate([np.arange(0, n, 2), [4097]])
    t = Ties(64, n, copies, 9300 + over)
    n8, nb = t.stage("8", k)[1], t.stage("bf16", k)[1]
    assert n8 == CAP + over and nb == CAP + over
    idx = t.index()
    got, inc = single(idx, t.q, k, False)
    if not over:
        assert inc["took8"] == 1 and inc["back8"] == 0 and inc["took"] == 1 and inc["back"] == 0 and inc["cand8"] == CAP and inc["cand"] == CAP, inc
    else:
        assert inc["took8"] == 1 and inc["back8"] == 1 and inc["cand8"] == CAP + 1 and inc["took"] == 1 and inc["back"] == 1 and inc["cand"] == CAP + 1, inc
    assert inc["took6"] == 0
    er, ed = t.answer(k)
    assert np.array_equal(er, t.copies[:k]) and same(got, (er, ed))
    idx.close()


# ---- 4. the last chunk ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("six", [True, False])
@pytest.mark.parametrize("n", [1024 * 3 + 64, 1024 * 3 + 65])
def test_the_last_chunk_is_short_and_padding_is_never_listed(n, six):
    """the padded row count is no multiple of 1024; the only copies are the last 64 rows, in the last — short — chunk; at + 65 the last
    tile holds one row and 63 padded slots, which no count includes"""
    assert ((n + 63) // 64 * 64) % CHUNK != 0
    t = Ties(64, n, np.arange(n - 64, n), 9400 + n % 2)
    idx = t.index()
    for k in KS:
        check_single(t, idx, k, six, "n %d" % n)
    idx.close()


# ---- 5. the shared pass --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", ["8bit", "bf16"])
def test_the_shared_pass_keeps_the_queries_lists_apart(plane):
    """three queries over case 1's dense corpus: the middle one is the query with 1024 tied candidates, the other two are ordinary.  The pass's
    largest survivor count is the dense query's and the model's; each query's answer is the oracle's — a row of the dense query's list in
    another's would move its answer or its count"""
    t = case1("dense")
    others = O.gen_rows(9500, 0, 2, t.dim).copy()
    for j in range(2):                                                   # (on the far rows' side: the copies are not THEIR nearest rows)
        if float(np.dot(others[j].astype(np.float64), t.uniq[0].astype(np.float64))) > 0:
            others[j] = -others[j]
    qs = np.ascontiguousarray(np.stack([others[0], t.q, others[1]]))
    idx = t.index()
    stage = "8" if plane == "8bit" else "bf16"
    for k in KS:
        counts = [t.stage(stage, k, q=qs[j])[1] for j in range(3)]
        assert counts[1] == len(t.copies) and max(counts[0], counts[2]) < counts[1] <= CAP, (k, counts)
        idx.set_bound_scan("always"); idx.set_bound_plane_mq(plane)
        got, inc = counted(idx, lambda: idx.search(qs, k))
        print("shared pass %s k %d: the model's counts %s, the pass's largest %d" % (plane, k, counts, inc["cand"]))
        assert inc["took"] == 3 and inc["back"] == 0 and inc["cand"] == counts[1], (k, inc, counts)
        assert (inc["took8"], inc["back8"]) == ((3, 0) if plane == "8bit" else (0, 0)) and (plane != "8bit" or inc["cand8"] == counts[1]), (k, inc)
        for j in range(3):
            assert same(got, t.answer(k, q=qs[j]), j), (k, j)
    idx.close()


# ---- 6. the masked form --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", ["8bit", "bf16"])
@pytest.mark.parametrize("name", ["dense", "every65th"])
def test_under_a_mask_that_keeps_half_of_the_copies(name, plane):
    t = case1(name)
    mask = np.ones(t.n, bool)
    mask[5::7] = False
    mask[t.copies] = True
    mask[t.copies[::2]] = False
    kept = t.copies[1::2]
    idx = t.index()
    rs = idx.rowset(mask)
    stage = "8" if plane == "8bit" else "bf16"
    for k in KS:
        cnt = t.stage(stage, k, mask)[1]
        if k <= len(kept):
            assert cnt == len(kept), (k, cnt)
        idx.set_bound_scan("always"); idx.set_bound_plane_filtered(plane)
        got, inc = counted(idx, lambda: idx.search_rowsets(t.q[None, :], k, [rs]))
        assert inc["took"] == 1 and inc["back"] == 0 and inc["cand"] == cnt, (k, inc, cnt)
        assert (inc["took8"], inc["back8"]) == ((1, 0) if plane == "8bit" else (0, 0)) and (plane != "8bit" or inc["cand8"] == cnt), (k, inc)
        er, ed = t.answer(k, mask)
        if k <= len(kept):
            assert np.array_equal(er, kept[:k])
        assert same(got, (er, ed)), (k, got[0], er)
    idx.close()


# ---- 7. the refine's compact array ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copies", [1, REFINE_BATCH - 1, REFINE_BATCH, REFINE_BATCH + 1])
def test_the_compact_arrays_edges(copies):
    """k = 1: the 6-bit stage's candidates are the copies alone — a batch of the refine short by one, full, and one over"""
    n = 4096 + 37
    t = Ties(64, n, 70 + 67 * np.arange(copies), 9600 + copies)
    assert t.stage("6", 1)[1] == copies
    idx = t.index()
    check_single(t, idx, 1, True, "%d copies" % copies)
    idx.close()


@pytest.mark.parametrize("over", [0, 1])
def test_the_survivors_capacity_out_of_more_candidates(over):
    """kBoundCandCap and kBoundCandCap + 1 survivors of the refine out of more 6-bit candidates (300 rows near enough for the 6-bit interval
    only): answered, and handed on through the bfloat16 stage to the exact scan; then, one copy removed, the same index on the same control
    words answers: they are back at zero"""
    n, k = 3 * 4096 + 37, 10
    copies = np.arange(0, n, 3)[:CAP + over]
    medium = 1 + 3 * np.arange(300) * 7
    t = Ties(64, n, copies, 9700 + over, medium=medium)
    p6, n6 = t.stage("6", k)
    n8 = t.stage("8", k, p6)[1]
    assert n8 == CAP + over and n6 > n8 + 100 and n6 <= CAP6, (n6, n8)
    idx = t.index()
    got, inc = single(idx, t.q, k, True)
    assert inc["took6"] == 1 and inc["back6"] == 0 and inc["cand6"] == n6 and inc["took8"] == 1 and inc["cand8"] == n8 and inc["took"] == 1, (inc, n6, n8)
    if over:
        assert inc["back8"] == 1 and inc["back"] == 1 and inc["cand"] == t.stage("bf16", k)[1] > CAP, inc
    else:
        assert inc["back8"] == 0 and inc["back"] == 0 and inc["cand"] == n8, inc
    er, ed = t.answer(k)
    assert np.array_equal(er, t.copies[:k]) and same(got, (er, ed))
    if over:
        idx.remove(np.array([copies[0]], np.uint32))
        alive = np.ones(n, bool); alive[copies[0]] = False
        p6, n6 = t.stage("6", k, alive)
        n8 = t.stage("8", k, p6)[1]
        assert n8 == CAP
        got, inc = single(idx, t.q, k, True)
        assert inc["took6"] == 1 and inc["back6"] == 0 and inc["cand6"] == n6 and inc["took8"] == 1 and inc["back8"] == 0 and inc["cand8"] == CAP and inc["back"] == 0, (inc, n6)
        er, ed = t.answer(k, alive)
        assert np.array_equal(er, t.copies[1:k + 1]) and same(got, (er, ed))
    idx.close()
