"""Inputs of the filtered batch's edge tests (tests/test_gpu_filtered_batch_edges.py) and what they promise, so that
tests/test_filtered_batch_edges_cpu.py can prove the promises with the oracle alone — TEST INFRASTRUCTURE ONLY (numpy, CPU, no device).

Three families, each a corpus, a batch of queries and ONE filter per query in both forms: a bool mask (a RowSet is made from it) and a
conjunction over named columns (search_where).  Both forms select the same rows, so one oracle answer serves both."""
import numpy as np

from tests import _extremes as X
from tests import _oracle as O
from tests import _order as OR

N = 40_003                                                              # 626 tiles, a partial last one
DEAD_STEP = 89
DEFAULT_PPM = 10_000
METRIC_IDS = {"cosine": 0, "l2": 1, "l2sq": 2, "dot": 3}


def dead_rows(n):
    return np.arange(5, n, DEAD_STEP, dtype=np.uint32)


def live_mask(n):
    live = np.ones(n, bool); live[dead_rows(n)] = False
    return live


def ordinary_rows(rows):
    """what tests/_extremes._queries calls an ordinary row: finite, norm within (0.5, 2)"""
    with np.errstate(all="ignore"):
        nrm = np.linalg.norm(rows.astype(np.float64), axis=1)
    return np.isfinite(rows).all(axis=1) & (nrm > 0.5) & (nrm < 2.0)


# ------------------------------------------------------------------------------------------------ 2. extreme rows and queries --
# Set kinds.  (a) - (f) are the issue's; (g) is added because (e) cannot promise everywhere what was asked of it: "every extreme row"
# holds rows of FINITE distance — the G, O, Z and D rows, and under cosine and dot, whose float64 chains do not overflow, the +-3e38 rows
# that make up a third of the "many" regime's fifth.  By the oracle (tests/test_filtered_batch_edges_cpu.py) (e) has 24 - 55 finite-distance
# rows: fewer than k = 64 in every cell but cosine and dot in the "many" regime (7 956 and 2 663), and never fewer than 10.  (g) is the
# set that has fewer than k at every k above 6, in both regimes, under every metric: the rows whose distance from an ordinary query is
# NOT finite under the case's metric, plus the same five ordinary rows.
KINDS = "abcdefg"
EXT_QUERIES = 20                                                        # what _queries returns beside the ordinary ones
NQ_MAX = 256
_corpora = {}


def extreme_position(p):
    """which positions of a batch hold an extreme query: every second of the first 40 (so the batch of 40 is the prefix of the batch of
    256 and holds all twenty), and every eleventh beyond — the twenty again, in other blocks of 64, under other set kinds"""
    return p % 2 == 1 if p < 40 else p % 11 == 0


class ExtremeCase:
    """rows (tests/_extremes._corpus, regime "few" or "many", tombstones every 89th row), NQ_MAX queries with extreme ones at
    extreme_position, `calm` — the same batch with every extreme query replaced by an ordinary one that occurs nowhere else — and per
    position: kind, mask [N], where (a list of (column name, op, literal), None = no filter).  Columns, by name -> (type, values)."""

    def __init__(self, metric, dim, regime):
        self.metric, self.mid, self.dim, self.regime = metric, METRIC_IDS[metric], dim, regime
        seed = 5000 + dim + (7 if regime == "many" else 0)
        if (dim, regime) not in _corpora:
            rows = X._corpus(seed, N, dim, regime, O.gen_rows(seed + 1, 0, 4, dim))
            _corpora.clear()                                            # (one corpus at a time: the cases of one shape follow each other)
            _corpora[(dim, regime)] = (rows, X._queries(seed, rows, dim, n_ord=NQ_MAX))
        self.rows, (qe, flag) = _corpora[(dim, regime)]
        ext, ordq = qe[flag], qe[~flag]
        assert ext.shape[0] == EXT_QUERIES and ordq.shape[0] == NQ_MAX
        self.live = live_mask(N)
        self.is_ext = np.array([extreme_position(p) for p in range(NQ_MAX)])
        n_ord = int((~self.is_ext).sum())
        self.qs = np.empty((NQ_MAX, dim), np.float32); self.calm = np.empty((NQ_MAX, dim), np.float32)
        self.kind = []
        e_i = o_i = 0
        for p in range(NQ_MAX):
            if self.is_ext[p]:
                self.qs[p] = ext[e_i % EXT_QUERIES]; self.calm[p] = ordq[n_ord + e_i]
                self.kind.append(KINDS[e_i % len(KINDS)])
                e_i += 1
            else:
                self.qs[p] = self.calm[p] = ordq[o_i]
                # every second ordinary query takes kind (d), the one the counters' cap pins; the others cycle through the rest, so
                # that the ten of them in a batch of 40 hold two of each kind that is probed twice
                self.kind.append("d" if o_i % 2 == 0 else "abcfegabcf"[(o_i // 2) % 10])
                o_i += 1
        rng = np.random.default_rng(seed + 99)
        self.ordinary = ordinary_rows(self.rows)
        self.extreme = ~self.ordinary
        u = rng.random(N)
        self.five = np.sort(rng.choice(np.flatnonzero(self.ordinary & self.live), 5, replace=False))
        x = self.extreme.astype(np.uint32); x[self.five] = 2
        ext_rows = np.flatnonzero(self.extreme)
        f = np.zeros(N); f[rng.choice(ext_rows, ext_rows.size // 2, replace=False)] = 1.0
        f[self.ordinary & (rng.random(N) < 0.3)] = 1.0
        with np.errstate(all="ignore"):
            g = (~np.isfinite(O.all_distances(self.mid, self.rows, ordq[0]))).astype(np.uint32)
        g[self.five] = 1
        self.columns = {"u": ("f64", u), "x": ("u32", x), "f": ("f64", f), "g": ("u32", g)}
        self.mask, self.where = [], []
        for p, kind in enumerate(self.kind):
            lo = (0.07 * p) % 0.5
            win = (u >= lo) & (u < lo + 0.5)
            m, w = {"a": (np.ones(N, bool), [("u", "ge", 0.0)]),
                    "b": (win, [("u", "ge", lo), ("u", "lt", lo + 0.5)]),
                    "c": (np.ones(N, bool), None),
                    "d": ((x == 0) & win, [("x", "eq", 0), ("u", "ge", lo), ("u", "lt", lo + 0.5)]),
                    "e": (x >= 1, [("x", "ge", 1)]),
                    "f": (f == 1.0, [("f", "eq", 1.0)]),
                    "g": (g == 1, [("g", "eq", 1)])}[kind]
            self.mask.append(m); self.where.append(w)
        # a query is CLEAN when it is ordinary and its set holds no live extreme row: nothing excuses handing it back
        self.touches = np.array([bool(self.is_ext[p] or (self.mask[p] & self.extreme & self.live).any()) for p in range(NQ_MAX)])

    def alive(self, p):
        return (self.live & self.mask[p]).astype(np.uint8)

    def cap(self, nq):
        """the most hand-backs + sparse a batch of the first nq queries may count"""
        t = int(self.touches[:nq].sum())
        return t + (nq - t) // 8

    def probes(self, nq):
        """the positions compared with the oracle: every extreme query, every query of kinds (e) and (g), two of each other kind"""
        out = [p for p in range(nq) if self.is_ext[p] or self.kind[p] in "eg"]
        for kind in "abcdf":
            out += [p for p in range(nq) if self.kind[p] == kind and not self.is_ext[p]][:2]
        return sorted(set(out))

    def finite_in_set(self, p):
        """live rows of position p's set whose distance from its query is a finite number"""
        sel = np.flatnonzero(self.live & self.mask[p])
        with np.errstate(all="ignore"):
            return int(np.isfinite(O.all_distances(self.mid, np.ascontiguousarray(self.rows[sel]), self.qs[p])).sum())


# ------------------------------------------------------------------------------------------------ 3. order-sensitive rows --
ORDER_COPIES = 3                                                        # the twelve queries of _case, three times: see OrderCase


class OrderCase:
    """tests/_order._case(metric, dim, 12, seed, n_fill, dup=3) as a batch of 36: the twelve queries three times, copy c of query j under
    set kind (j + c) mod 4.  Twelve queries alone are no batch here — the batched path takes a piece from a million query-rows on
    (12 x 40 043 is half of that) and the float32 filter from 32 queries — so the batch repeats them, and every query meets three kinds.
    Kinds: 0 no filter; 1 every second planted row of the query and a random 30 % of the fillers; 2 every planted row but ONE copy of each
    duplicated one — alternately the lower- and the higher-numbered — and 30 % of the fillers; 3 the same membership as kind 2, which the
    GPU test gives as a where-filter made set.  Per position: mask (None for kind 0) and the name of its U32 column (value 1 = member)."""

    def __init__(self, metric, dim, seed, n_fill):
        self.metric, self.dim = metric, dim
        self.qs12, self.rows, self.own = OR._case(metric, dim, 12, seed, n_fill, dup=3)
        n = self.n = self.rows.shape[0]
        self.nq = 12 * ORDER_COPIES
        self.qs = np.ascontiguousarray(np.concatenate([self.qs12] * ORDER_COPIES))
        rng = np.random.default_rng(seed + 5)
        planted_any = np.zeros(n, bool)
        for o in self.own:
            planted_any[o] = True
        self.filler = ~planted_any
        self.kind, self.mask, self.column, self.columns = [], [], [], {}
        self.excluded = []
        for p in range(self.nq):
            j, c = p % 12, p // 12
            kind = (j + c) % 4
            self.kind.append(kind)
            if kind == 0:
                self.mask.append(None); self.column.append(None); self.excluded.append(np.zeros(0, np.int64))
                continue
            own = self.own[j]
            m = self.filler & (rng.random(n) < 0.3)
            if kind == 1:
                m[own[::2]] = True
                drop = np.zeros(0, np.int64)
            else:
                m[own] = True
                drop = []
                for i, (lo, hi) in enumerate(self.duplicates(j)):
                    drop.append(lo if i % 2 == 0 else hi)
                drop = np.array(drop, np.int64)
                m[drop] = False
            self.mask.append(m); self.excluded.append(drop)
            name = "m%d" % p
            self.column.append(name); self.columns[name] = ("u32", m.astype(np.uint32))

    def duplicates(self, j):
        """[(lower row, higher row)] of the planted rows of query j that are bytewise equal"""
        seen, out = {}, []
        for r in self.own[j]:
            key = self.rows[r].tobytes()
            if key in seen:
                out.append((seen[key], int(r)))
            else:
                seen[key] = int(r)
        return out

    def alive(self, p):
        return None if self.mask[p] is None else self.mask[p].astype(np.uint8)


# ------------------------------------------------------------------------------------------------ 4. ragged sets --
RAGGED_OLD, RAGGED_NEW = 33_000, N                                       # 515 whole tiles and 40 rows; then 625 and 3
RAGGED_LAST_GROUP = 39_936                                               # the grown corpus's last 128-row group: tile 624 and the 3 rows of tile 625
RAGGED_KINDS = ("half_old", "bit0", "bit63", "old_last_tile", "new_last_tile", "empty", "where_old", "none")


class RaggedCase:
    """The host's picture of the ragged-set test: per query of 40 a kind (query number mod 8), whether its set is made BEFORE the index
    grows from RAGGED_OLD to RAGGED_NEW rows, its window of the column (a where-filter, else None) and its mask over the grown corpus.  A set made before the growth is given to the
    device as its first RAGGED_OLD bits: its words end where the old corpus did."""

    def __init__(self, dim=128, nq=40):
        self.dim, self.nq, self.n = dim, nq, RAGGED_NEW
        self.rows = O.gen_rows(7700 + dim, 0, RAGGED_NEW, dim)
        self.qs = O.gen_rows(7800 + dim, 0, nq, dim)
        self.live = live_mask(RAGGED_NEW)                                # tombstoned AFTER the sets exist
        rng = np.random.default_rng(77)
        self.val = rng.random(RAGGED_OLD)                                # the column: values for the old rows only
        r = np.arange(RAGGED_NEW)
        self.kind, self.mask, self.before, self.where = [], [], [], []
        for q in range(nq):
            kind = RAGGED_KINDS[q % 8]
            m = np.zeros(RAGGED_NEW, bool)
            window = None
            if kind == "half_old":
                m[:RAGGED_OLD] = rng.random(RAGGED_OLD) < 0.5
            elif kind == "bit0":
                m[:RAGGED_OLD] = r[:RAGGED_OLD] % 64 == 0
            elif kind == "bit63":
                m[:RAGGED_OLD] = r[:RAGGED_OLD] % 64 == 63
            elif kind == "old_last_tile":
                m[RAGGED_OLD // 64 * 64:RAGGED_OLD] = True
            elif kind == "new_last_tile":
                m[RAGGED_LAST_GROUP:] = True
            elif kind == "where_old":
                lo = 0.1 + 0.05 * (q // 8)
                m[:RAGGED_OLD] = (self.val >= lo) & (self.val < lo + 0.4)
                window = (lo, lo + 0.4)
            elif kind == "none":
                m[:] = True
            self.kind.append(kind); self.mask.append(m); self.where.append(window)
            self.before.append(kind not in ("new_last_tile", "none", "where_old"))
        # the change between the two runs, in the first "half_old" and the first "bit0" set: 200 rows out — the query's five nearest
        # live rows of the set among them — and 200 in, among them its five nearest live rows outside: the answer has to move
        self.changed = {}
        for q in (0, 1):
            m = self.mask[q]
            order = np.argsort(O.all_distances(0, self.rows, self.qs[q]), kind="stable")
            order = order[self.live[order]]
            near_in, near_out = order[m[order]][:5], order[~m[order]][:5]
            add = np.union1d(near_out, rng.choice(np.setdiff1d(np.flatnonzero(~m), near_out), 195, replace=False))   # (rows of the grown corpus too)
            drop = np.union1d(near_in, rng.choice(np.setdiff1d(np.flatnonzero(m), near_in), 195, replace=False))
            self.changed[q] = (add.astype(np.uint32), drop.astype(np.uint32))

    def masks_after(self):
        out = [m.copy() for m in self.mask]
        for q, (add, drop) in self.changed.items():
            out[q][add] = True; out[q][drop] = False
        return out


def sample_positions(plan, n):
    """sample position -> corpus row, as qv_batched_sample_plan states it"""
    i = np.arange(plan["rows"])
    r = (i // 128) * plan["group_step"] * 128 + i % 128
    return r[r < n]


def predicted_sparse(plan, n, live, masks, ppm=DEFAULT_PPM):
    """how many queries the device must find below the sparse floor: it counts the live in-set rows of the sample"""
    pos = sample_positions(plan, n)
    return sum(1 for m in masks if int((live & m)[pos].sum()) * 1_000_000 < ppm * plan["rows"])
