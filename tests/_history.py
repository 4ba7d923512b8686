"""Mutation histories for the bound scan's tests: a seeded schedule of every writer interleaved with searches of every bound-scan route
(`plan`), a host model of what the index must hold after each step (`Model`), and a checker of the per-row arrays the bound scan's
interval rests on, as DeviceIndex.debug_read returns them (`check_state`).  tests/test_bound_history_cpu.py inspects the schedules and
shows what the checker catches without a device; tests/test_gpu_bound_history.py replays them on one.  TEST INFRASTRUCTURE ONLY.
Every round of searches ends with searches of the wide form (65 <= k <= 1024, `WIDE_ROUTES`), whose counters — the survivor count of stage 1
among them — `Model.predict_wide` gives from tests/_wide.decide_wide over the row states the model keeps step by step.

The layouts are restated HERE in numpy from the comments of quiver_amd/csrc/qv_bound.h and qv_misc.hip — the 8-bit plane [tile][dim / 16]
[64 rows][16 B], the 6-bit plane [tile][group of 64 dims][3][64 rows][16 B] with the biased code of dims 0 - 47 in the low six bits of byte
d & 15 of piece d >> 4 and of dims 48 - 63 two bits a piece in the top of byte d - 48 — independent of the writers' index arithmetic; the
bfloat16 copy is tests/test_gpu_row_state.decode's."""
import types

import numpy as np

import quiver_amd
from tests import _bound as B
from tests import _bound6 as B6
from tests import _bound8 as B8
from tests import _bound_l2 as BL
from tests import _oracle as O
from tests import _wide as Wd
from tests import _widths as W
from tests.test_gpu_fuzz import _vectors
from tests.test_gpu_row_state import Expected, check, decode, mixture

METRICS = ("cosine", "dot", "l2")
DIMS = (16, 48, 64, 128, 192, 768)                  # 16 and 48: the 8-bit plane without the 6-bit one
STYLES = ("gauss", "alphabet", "mixture")
SEEDS = tuple(range(36))                            # every (metric, dim) twice
FIRST = (300, 449, 512, 513, 700)                   # 300 rows: fewer than 8 tiles, no forced route runs; 449: exactly 8
KS = (1, 10, 63, 64)
# (form, plane): one query or a shared pass of 2 - 8, filtered or not, each on either plane; the 6-bit stage in front of one unfiltered query
ROUTES = (("1", "bf16"), ("1", "8bit"), ("1", "6bit"), ("mq", "bf16"), ("mq", "8bit"), ("1f", "bf16"), ("1f", "8bit"), ("mqf", "bf16"), ("mqf", "8bit"))
# the wide form of one query's bound scan, 65 <= k <= 1024 (tests/_wide.py): unfiltered ("w") or over a candidate bitmap ("wf"), either plane first
WIDE_ROUTES = (("w", "bf16"), ("w", "8bit"), ("wf", "bf16"), ("wf", "8bit"))
KS_WIDE = (65, 100, 129, 500, 1024)
# zero, nan: queries bound_scan_norm_ok declines; all_but_one: k = live candidates - 1, the largest k the form takes; all: k = live candidates,
# which the dispatch declines; unsure: k above the candidates the bound is sure of and below the live ones — no finite H
WIDE_DELIBERATE = ("all_but_one", "zero", "all", "nan", "unsure")
WIDE_PER_ROUND = 2                                  # wide searches a round of searches gains, a deliberate one among them where one is due
WRITERS = ("add", "add_synthetic", "add_partial_tile", "add_growth", "update", "update_rows", "update_rows_device", "remove", "revival")
ARRAYS = ("rnorm", "rres", "plane", "rowmaj16", "plane8", "rres8", "rscale8", "plane6", "rres6")
FIRST_TILES = 16                                    # the first add reserves max(its tiles, 16) tiles: an add past them grows the arrays
# |r_i - scale r8_i| <= 0.5 scale (1 + ELEM8): bound8_quant rounds the FLOAT32 quotient r_i / scale, which is at most 127 and so carries an
# error of up to half a unit in the last place of [64, 128), 2^-18; a quotient that close above a half-integer rounds onto it and then to the
# even side.  So the element error is at most (0.5 + 2^-18) scale = 0.5 scale (1 + 2^-17); the 1e-6 that suffices for tests/test_bound_scan8_cpu.py's
# sixteen Gaussian rows is too tight by the factor 7.6 for a row that meets such a quotient (tests/test_bound_history_cpu.py shows one).
ELEM8 = 2.0 ** -17
ELEM6 = 1e-5                                        # |r_i - 4 scale c6_i| <= 3 scale (1 + 1e-5): tests/test_bound_scan6_cpu.py's


def config(seed):
    """-> dict(metric, dim, style, flags: the constructor's keywords, keeps: the arrays such an index keeps)"""
    metric, dim = METRICS[seed % 3], DIMS[(seed // 3) % 6]
    style = STYLES[(seed // 3 + seed // 18) % 3]
    flags = {}
    if metric == "l2":
        flags["l2_scan_plane"] = True
    keeps = ["rnorm", "rres", "plane", "plane8", "rres8"]
    if dim % 64 == 0:
        keeps += ["rscale8", "plane6", "rres6"]     # (the scale is readable only beside the 6-bit plane)
    if metric == "cosine" and (seed // 3 + seed // 18) % 2 == 0:
        flags.update(rowmajor=True, graph_plane=True)
        if dim % 64 == 0:                           # (the row-order copy is kept in whole 64-element slabs only)
            keeps.append("rowmaj16")
    return {"seed": seed, "metric": metric, "dim": dim, "style": style, "flags": flags, "keeps": tuple(keeps)}


def vectors(rng, n, dim, style):
    if style == "alphabet":
        x = _vectors(rng, n, dim, 0)
        x[4::9] = np.where(x[4::9] == 0, np.float32(1.0), x[4::9])     # rows without a zero element: the ones tests/test_gpu_row_state.check counts as exact
        x[13::50] = 0.0                                                 # all-zero rows
        return x
    if style == "mixture":                          # (its classes sit at fixed places of 130 rows or more)
        m = mixture(rng, max(n, 130), dim)
        return m if n >= 130 else m[np.sort(rng.choice(130, n, replace=False))]
    x = (rng.standard_normal((n, dim)) * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)
    x[::7] = B.bf16(x[::7])                         # rows exact in bfloat16: their residual is 0.0
    return x


def tiny_norm(dim):
    return max(float(np.sqrt(np.float32(dim) * np.float32(2.4e-32))), 1.0e-14)


def declined_rows(rows, rn=None):
    """the rows the bound says nothing about: a non-finite element, all zero, or a norm outside bound_scan_norm_ok"""
    with np.errstate(all="ignore"):
        if rn is None:
            rn = np.sqrt(np.sum(rows.astype(np.float64) ** 2, axis=1))
        ok = np.isfinite(rows).all(axis=1) & (rows != 0).any(axis=1) & (rn >= tiny_norm(rows.shape[1])) & (rn < 1.0e18)
    return ~ok


OPS = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal, "ne": np.not_equal, "in": np.isin}


class Model:
    """the rows, the alive flags, the columns' values and their presence, the sets' membership — and, with derive=True, what ingest derives
    of every row, recomputed for the rows a step touches only"""

    def __init__(self, cfg, derive=True):
        self.cfg, self.dim, self.mid, self.derive = cfg, cfg["dim"], quiver_amd.metric_id(cfg["metric"]), derive
        self.rows = np.zeros((0, self.dim), np.float32)
        self.alive = np.zeros(0, bool)
        self.declined = np.zeros(0, bool)
        self.col = {"u32": np.zeros(0, np.uint32), "f64": np.zeros(0, np.float64)}
        self.has = {"u32": np.zeros(0, bool), "f64": np.zeros(0, bool)}
        self.sets = {}
        self.exp = self.s8 = self.s6 = None

    @property
    def n(self):
        return self.rows.shape[0]

    # ---- what ingest derives ----
    def _derived(self, rows):
        e = Expected(rows)
        d = {"exp": {k: v for k, v in vars(e).items()}}
        s8 = B8.RowState8(rows)
        d["s8"] = {"r8": s8.r8, "scale": s8.scale, "res": s8.res}
        if self.dim % 64 == 0:
            s6 = B6.RowState6(rows)
            d["s6"] = {"bytes": s6.bytes, "codes": s6.codes, "res": s6.res}
        return d

    def _touch(self, at, grown=False):
        at = np.asarray(at, np.int64)
        self.declined[at] = declined_rows(self.rows[at])
        if not self.derive:
            return
        d = self._derived(self.rows[at])
        for name, fields in d.items():
            cur = getattr(self, name)
            if cur is None:
                setattr(self, name, types.SimpleNamespace(**{k: v.copy() for k, v in fields.items()}))
                continue
            for k, v in fields.items():
                if grown:
                    setattr(cur, k, np.concatenate([getattr(cur, k), v]))
                else:
                    getattr(cur, k)[at] = v

    def states(self):
        """the models' views of the rows: tests/_bound.RowState, _bound8.RowState8 and _bound6.RowState6 by their attributes"""
        st16 = types.SimpleNamespace(rows=self.rows, rh=self.exp.rh, rn=self.exp.rn, rres=self.exp.res_up)
        st8 = types.SimpleNamespace(rows=self.rows, r8=self.s8.r8, scale=self.s8.scale, res=self.s8.res, rn=self.exp.rn)
        st6 = None if self.s6 is None else types.SimpleNamespace(rows=self.rows, codes=self.s6.codes, scale=self.s8.scale, res=self.s6.res, rn=self.exp.rn)
        return st16, st8, st6

    # ---- the writers ----
    def _append(self, x):
        n0, m = self.n, len(x)
        self.rows = np.concatenate([self.rows, np.ascontiguousarray(x, np.float32)])
        self.alive = np.concatenate([self.alive, np.ones(m, bool)])
        self.declined = np.concatenate([self.declined, np.zeros(m, bool)])
        for c in self.col:
            self.col[c] = np.concatenate([self.col[c], np.zeros(m, self.col[c].dtype)])
            self.has[c] = np.concatenate([self.has[c], np.zeros(m, bool)])                   # rows added later have no value
        for name in self.sets:
            self.sets[name] = np.concatenate([self.sets[name], np.zeros(m, bool)])           # ... and start unselected
        self._touch(np.arange(n0, n0 + m), grown=True)
        return n0

    def apply(self, step):
        kind = step["kind"]
        if kind == "add":
            first = self._append(step["vecs"])
            if "facets" in step:
                self.apply(dict(step["facets"], kind="facets", first=first))
        elif kind == "add_synthetic":
            self._append(O.gen_rows(step["seed"], 0, step["n"], self.dim))
        elif kind == "remove":
            self.alive[step["rows"]] = False
        elif kind == "update":
            self.rows[step["row"]] = step["vec"]; self.alive[step["row"]] = True
            self._touch([step["row"]])
        elif kind == "update_rows":
            for r, v in zip(step["rows"], step["vecs"]):                                     # what the loop of updates leaves: the last vector of a repeated row
                self.rows[r] = v
            self.alive[step["rows"]] = True
            self._touch(np.unique(step["rows"]))
        elif kind == "facets":
            a, m = step["first"], len(step["u32"])
            self.col["u32"][a:a + m] = step["u32"]; self.has["u32"][a:a + m] = True
            self.col["f64"][a:a + m] = step["f64"]; self.has["f64"][a:a + m] = step["present"]
        elif kind == "rowset":
            self.sets[step["name"]] = step["mask"].copy()
        else:
            raise ValueError(kind)

    # ---- the filters ----
    def where(self, preds):
        m = np.ones(self.n, bool)
        for c, op, lit in preds:
            m &= self.has[c] & OPS[op](self.col[c], lit)                                     # a row without a value fails every comparison
        return m

    def selected(self, step):
        """one bool [n] per query (None: every row)"""
        nq, call, filt = len(step["qs"]), step["call"], step.get("filt")
        if call == "plain":
            return [None] * nq
        if call == "masked":
            return [filt] * nq
        if call == "rowsets":
            return [None if f is None else self.sets[f] for f in filt]
        return [None if f is None else self.where(f) for f in filt]

    def candidates(self, sel):
        return self.alive if sel is None else self.alive & sel

    def search(self, q, k, sel=None):
        return O.exact_search(self.mid, self.rows, q, k, alive=self.candidates(sel).astype(np.uint8))

    # ---- the stages' CPU models ----
    def ref16(self, q, k, alive):
        st16 = self.states()[0]
        return B.decide(BL.stage1(st16, q), k, alive) if self.cfg["metric"] == "l2" else B.reference(self.mid, st16, q, k, alive)

    def ref8(self, q, k, alive):
        return B8.reference8(self.mid, self.states()[1], q, k, alive)

    def ref6(self, q, k, alive):
        return B6.reference6(self.mid, self.states()[2], q, k, alive)

    def predict(self, step):
        """what the counters must show for one forced search on 8 tiles or more: the increments of `searches` and `hand_backs` of the three
        stages, and for one unfiltered query the candidate counts of the stages that answered (None where a stage handed on or did not run)"""
        plane, qs, k = step["plane"], step["qs"], step["k"]
        nq = len(qs)
        out = {"took6": 0, "back6": 0, "took8": 0, "back8": 0, "took": nq, "back": 0, "cand6": None, "cand8": None, "cand": None}
        for q, sel in zip(qs, self.selected(step)):
            alive = self.candidates(sel)
            if plane == "bf16":
                m16 = self.ref16(q, k, alive)
                out["back"] += bool(m16["hand_back"]); out["cand"] = None if m16["hand_back"] else m16["count"]
                continue
            out["took8"] += 1
            if plane == "6bit":
                m6 = self.ref6(q, k, alive)
                m8 = self.ref8(q, k, m6["passed"])
                out["took6"] += 1; out["back6"] += bool(m6["hand_back"])
                on = bool(m6["hand_back"] or m8["hand_back"])
                out["cand6"] = None if m6["hand_back"] else m6["count"]
            else:
                m8 = self.ref8(q, k, alive)
                on = bool(m8["hand_back"])
            out["back8"] += on; out["cand8"] = None if on else m8["count"]
            if on:
                m16 = self.ref16(q, k, alive)
                out["back"] += bool(m16["hand_back"]); out["cand"] = None if m16["hand_back"] else m16["count"]
        if nq != 1 or step["call"] != "plain":
            out["cand6"] = out["cand8"] = out["cand"] = None
        return out

    # ---- the wide form (65 <= k <= 1024) ----
    def stage_wide(self, arm, q, fault=None, stale=None):
        """the interval of every row for q as the wide form's stage 1 on `arm` computes it, from the states kept incrementally.  fault
        "stale" with stale = (row, its previous vector): that row keeps the interval of the vector it held before — a plane a writer missed"""
        st16, st8, _ = self.states()

        def of(s16, s8):
            if arm == "8bit" and B8.quantize_query(q) is None:                               # a zero or non-finite query: the intervals tests/_bound8.reference8 gives it
                r = B8.reference8(self.mid, s8, q, 1)
                return {"lo": r["lo"], "hi": r["hi"], "unsure": r["unsure"], "qn": B.chain_norm(q), "dim": self.dim}
            if arm == "8bit":
                return W.stage8_of(self.mid, s8, q)
            return BL.stage1(s16, q) if self.cfg["metric"] == "l2" else B.stage1(self.mid, s16, q)
        st = of(st16, st8)
        if fault == "stale" and stale is not None:
            row, vec = stale
            old = of(B.RowState(vec[None, :]), B8.RowState8(vec[None, :]))
            st = dict(st, lo=st["lo"].copy(), hi=st["hi"].copy(), unsure=st["unsure"].copy())
            for f in ("lo", "hi", "unsure"):
                st[f][row] = old[f][0]
        return st

    def predict_wide(self, step, cus, fault=None, cache=None):
        """what bound_scan_wide_stats must show for one forced wide search: the increments of `searches` ("took") and `hand_backs` ("back")
        and the survivor count of the stage that answered ("cand"; None where the bfloat16 stage hands back too, or the form is not taken).
        The dispatch takes the form on 8 tiles or more when there are MORE live candidates than results (under a filter that also means a
        tile with a candidate); the 8-bit stage's count stands where it answers, otherwise the search is the bfloat16 stage's.  The decision
        is tests/_wide.decide_wide over the call's candidate bitmap; at these sizes a wave owns one tile and publishes all of it (asserted).
        fault: what tests/test_bound_history_cpu.py plants — "dead" (dead rows keyed: every written row, under a filter every selected
        one), "unselected" (under a filter, every live row keyed), "rank" (H one rank early), "stale" (stage_wide's)."""
        arm, q, k = step["plane"], step["qs"][0], step["k"]
        sel = self.selected(step)[0]
        live = self.candidates(sel)
        n_tiles = (self.n + 63) // 64
        out = {"took": 0, "back": 0, "cand": None}
        if n_tiles < 8 or not 64 < k <= Wd.MAX_K or k >= int(live.sum()):
            return out
        out["took"] = 1
        grid = Wd.plan(n_tiles, cus)[0]
        kw = {}
        if fault == "dead":
            kw["key_live"] = np.ones(self.n, bool) if sel is None else sel
        elif fault == "unselected":
            kw["key_live"] = self.alive
        elif fault == "rank":
            kw["rank"] = k - 1
        stale = (step["stale_row"], step["stale_vec"]) if step.get("stale_row") is not None else None
        cache = {} if cache is None else cache                                               # (arm, stale) -> intervals: one step under several faults
        for a in (("8bit", "bf16") if arm == "8bit" else ("bf16",)):
            key = (a, fault == "stale")
            if key not in cache:
                cache[key] = self.stage_wide(a, q, fault, stale)
            d = Wd.decide_wide(cache[key], k, live, n_tiles, grid, **kw)
            assert d["dropped"] == 0, (n_tiles, grid, d["dropped"])
            if not d["hand_back"]:
                out["cand"] = d["count"]
                return out
        out["back"] = 1
        return out


# ---- the schedule ----------------------------------------------------------------------------------------------------------------------
def _facets(rng, m):
    return {"u32": rng.integers(0, 10, m).astype(np.uint32), "f64": rng.standard_normal(m), "present": rng.random(m) < 0.9}


PREDS = ([("u32", "lt", 6)], [("u32", "in", [1, 3, 5, 7, 8, 9])], [("u32", "ne", 0)], [("f64", "ge", -0.5)], [("f64", "lt", 0.9), ("u32", "ge", 2)])


def is_wide(step):
    return step["kind"] == "search" and step["form"] in ("w", "wf")


def plan(seed, wide=True):
    """-> (config, steps): a pure function of the seed.  A step is a dict with "kind": a writer ("add", "add_synthetic", "remove", "update",
    "update_rows" with "device": bool), "facets", "rowset", or "search" (form, plane, call, qs, k, filt, deliberate).
    wide: every round of searches ends with WIDE_PER_ROUND searches of the wide form (`is_wide`; one query, form "w" or "wf", and beside the
    keys above "stale_row" / "stale_vec": the last overwritten row and its previous vector).  They are drawn from a generator of their own and
    read the planning model only: without them the steps are plan(seed, wide=False)'s."""
    cfg = config(seed)
    dim, style = cfg["dim"], cfg["style"]
    rng = np.random.default_rng(77_000 + seed)
    wrng = np.random.default_rng(78_000 + seed)
    wcount = {"route": 5 * seed, "call": seed, "query": seed}
    wqueue = [WIDE_DELIBERATE[(seed + i) % len(WIDE_DELIBERATE)] for i in range(len(WIDE_DELIBERATE))]
    m = Model(cfg, derive=False)
    steps, pending, replaced = [], [], []           # blocks whose facets are not set yet; (row, its previous vector) of the last overwrites
    count = {"search": 0, "rows_list": seed, "query": seed, "call": seed}
    routes = [r for r in ROUTES if r[1] != "6bit" or dim % 64 == 0]

    def push(step):
        steps.append(step)
        if step["kind"] != "search":
            m.apply(step)

    def add(cnt, facets_now=False):
        x = vectors(rng, cnt, dim, style)
        if m.n and rng.random() < 0.5:
            x[0] = m.rows[rng.integers(m.n)]                                                 # a duplicate of a stored row, possibly of a dead one
        step = {"kind": "add", "vecs": x}
        if facets_now:
            step["facets"] = _facets(rng, cnt)
        else:
            pending.append((m.n, cnt))
        push(step)

    def overwrite(rows, vecs, **kw):
        for r in np.unique(rows)[:4]:
            replaced.append((int(r), m.rows[r].copy()))
        del replaced[:-4]
        push(dict({"kind": "update_rows", "rows": np.asarray(rows, np.uint32), "vecs": vecs}, **kw))

    def update_rows(device):
        n, dead, live = m.n, np.flatnonzero(~m.alive), np.flatnonzero(m.alive)
        which = count["rows_list"] % 4; count["rows_list"] += 1
        if which == 0:                                                                       # one row three times under different vectors, dead rows between
            r = int(rng.choice(live))
            rows = np.array([r, *(dead[:2] if len(dead) else live[:2]), r, int(rng.integers(n)), r])
        elif which == 1:                                                                     # every row of one tile
            t = int(rng.integers(n // 64))
            rows = rng.permutation(np.arange(64 * t, 64 * t + 64))
        elif which == 2:                                                                     # rows 63 and 64 together
            rows = np.concatenate([[63, 64], rng.integers(0, n, 6)])
        else:
            rows = rng.integers(0, n, 40)                                                    # with repeats and dead rows
        vecs = vectors(rng, 130, dim, style)[rng.permutation(130)[:len(rows)]] if style == "mixture" else vectors(rng, len(rows), dim, style)
        overwrite(rows, vecs, device=device)

    def mutate(kind):
        n = m.n
        if kind == "add_small":
            add(int(rng.choice([1, 63, 64, 65])))
        elif kind == "add_big":
            add(int(rng.integers(690, 711)))
        elif kind == "add_synthetic":
            pending.append((n, 100))
            push({"kind": "add_synthetic", "seed": 910_000 + seed, "n": 100})
        elif kind == "remove":
            push({"kind": "remove", "rows": rng.integers(0, n, int(rng.integers(1, 40))).astype(np.uint32)})     # repeats and rows already dead
        elif kind in ("update", "revive"):
            dead = np.flatnonzero(~m.alive)
            row = int(rng.choice(dead)) if kind == "revive" and len(dead) else int(rng.choice(np.flatnonzero(m.alive)))
            vec = vectors(rng, 8, dim, style)[int(rng.integers(8))]
            replaced.append((row, m.rows[row].copy())); del replaced[:-4]
            push({"kind": "update", "row": row, "vec": vec})
        elif kind == "update_rows":
            update_rows(False)
        elif kind == "update_rows_device":
            update_rows(True)
        if pending and rng.random() < 0.5:                                                   # a block's values arrive some steps after its rows
            first, cnt = pending.pop(0)
            push(dict(_facets(rng, cnt), kind="facets", first=first))

    def queries(nq):
        qs = vectors(rng, max(nq, 8), dim, "gauss" if style == "mixture" else style)[:nq].copy()
        which = count["query"] % 4; count["query"] += 1
        # (a vector the bound declines would be handed back as a query: the deliberate cases cover that, these stay within the cap)
        new = [r for r, _ in replaced if not m.declined[r]]
        old = [v for _, v in replaced if not declined_rows(v[None, :])[0]]
        if which == 0:
            qs[0] = m.rows[int(rng.choice(np.flatnonzero(m.alive & ~m.declined)))]           # a stored row
        elif which == 1 and new:
            qs[0] = m.rows[new[-1]]                                                          # a row that was just replaced
        elif which == 2 and old:
            qs[-1] = old[-1]                                                                 # the previous vector of a replaced row: finds a stale plane
        return qs

    def search(form, plane, deliberate=None):
        nq = 1 if form in ("1", "1f") else int(rng.choice([2, 3, 4, 5, 8]))
        qs = queries(nq)
        step = {"kind": "search", "form": form, "plane": plane, "qs": qs, "deliberate": deliberate, "call": "plain", "filt": None}
        if form in ("1f", "mqf"):
            call = ("masked", "rowsets", "where")[count["call"] % 3] if deliberate != "short" else "rowsets"
            count["call"] += 1
            names = sorted(n for n in m.sets if n != "few")
            if call == "masked":
                filt = rng.random(m.n) < float(rng.choice([0.9, 0.6]))
            elif call == "rowsets":                                                          # one set, a set per query, None mixed in (never None alone)
                filt = [names[int(rng.integers(len(names)))] for _ in range(nq)] if rng.random() < 0.6 else [names[0]] * nq
                if nq > 1 and rng.random() < 0.5:
                    filt[int(rng.integers(1, nq))] = None
                if deliberate == "short":
                    filt[0] = "few"
            else:
                filt = [list(PREDS[int(rng.integers(len(PREDS)))]) for _ in range(nq)]
                if nq > 1 and rng.random() < 0.5:
                    filt[int(rng.integers(1, nq))] = None
            step.update(call=call, filt=filt)
        if deliberate == "zero":
            qs[0] = 0.0
        elif deliberate == "nan":
            qs[0, dim // 2] = np.nan
        sure = [int((m.candidates(s) & ~m.declined).sum()) for s in m.selected(step)]
        k = int(rng.choice(KS))
        if deliberate == "short":
            k = 10
        else:
            floor = min(sure)
            k = max(1, min(k, floor))                                                        # every query has k rows the bound is sure of
        step["k"] = k
        step["after"] = {"growth": grown(), "update_rows": any(s["kind"] == "update_rows" for s in steps), "tiles": (m.n + 63) // 64}
        push(step)

    def grown():
        return (m.n + 63) // 64 > max(FIRST_TILES, (len(steps[0]["vecs"]) + 63) // 64)

    # ---- the wide searches: drawn from wrng; rng, count, replaced and the planning model are read, never moved ----
    def wide_query():
        """a stored row, a row that was just replaced, the previous vector of a replaced row, the vector of a DEAD row (a kernel that keys
        tombstones puts it at the head of a list), a fresh vector — never one the bound declines"""
        which = wcount["query"] % 5; wcount["query"] += 1
        new = [r for r, _ in replaced if not m.declined[r]]
        old = [v for _, v in replaced if not declined_rows(v[None, :])[0]]
        dead = np.flatnonzero(~m.alive & ~m.declined)
        if which == 1 and new:
            return m.rows[new[-1]].copy()
        if which == 2 and old:
            return old[-1].copy()
        if which == 3 and len(dead):
            return m.rows[int(wrng.choice(dead))].copy()
        if which == 4:
            q = vectors(wrng, 8, dim, "gauss" if style == "mixture" else style)[0].copy()
            if not declined_rows(q[None, :])[0]:
                return q
        return m.rows[int(wrng.choice(np.flatnonzero(m.alive & ~m.declined)))].copy()

    def wide_call():
        call = ("masked", "rowsets", "where")[wcount["call"] % 3]; wcount["call"] += 1
        return call

    def wide_filter(call):
        names = sorted(n for n in m.sets if n != "few")
        if call == "masked":
            return wrng.random(m.n) < float(wrng.choice([0.9, 0.6]))
        if call == "rowsets":
            return [names[int(wrng.integers(len(names)))]]
        return [list(PREDS[int(wrng.integers(len(PREDS)))])]

    def wide_counts(step):
        """(live candidates, of them the ones the bound is sure of)"""
        live = m.candidates(m.selected(step)[0])
        return int(live.sum()), int((live & ~m.declined).sum())

    def wide_push(step, k):
        row, vec = replaced[-1] if replaced else (None, None)
        step.update(k=int(k), stale_row=row, stale_vec=None if vec is None else vec.copy(),
                    after={"growth": grown(), "update_rows": any(s["kind"] == "update_rows" for s in steps), "tiles": (m.n + 63) // 64})
        push(step)

    def wide_step(form, plane, q, deliberate=None):
        step = {"kind": "search", "form": form, "plane": plane, "qs": q[None, :].copy(), "deliberate": deliberate, "call": "plain", "filt": None}
        if form == "wf":
            call = wide_call()
            step.update(call=call, filt=wide_filter(call))
        return step

    def wide_k(step):
        """a member of KS_WIDE below the candidates the bound is sure of: the drawn one, else the largest that is (None: there is none)"""
        sure = wide_counts(step)[1]
        k = int(wrng.choice(KS_WIDE))
        below = [x for x in KS_WIDE if x < sure]
        return k if k < sure else below[-1] if below else None

    def wide_plain():
        form, plane = WIDE_ROUTES[wcount["route"] % len(WIDE_ROUTES)]; wcount["route"] += 1
        step = wide_step(form, plane, wide_query())
        k = wide_k(step)
        if k is not None:
            wide_push(step, k)

    def wide_deliberate(kind):
        """-> whether the case could be scheduled now"""
        form, plane = WIDE_ROUTES[wcount["route"] % len(WIDE_ROUTES)]
        q = m.rows[int(wrng.choice(np.flatnonzero(m.alive & ~m.declined)))].copy()
        if kind in ("zero", "nan"):
            if kind == "zero":
                q[:] = 0.0
            else:
                q[dim // 2] = np.nan
            step = wide_step(form, plane, q, kind)
            k = wide_k(step)
        else:
            # a k of 65 to 1024 fixed by the candidates: unfiltered on a small index, else under a set or a predicate that leaves so few, else
            # under a mask of about 600 rows (with every row the bound declines in it, where the case needs them)
            options = [("plain", None)] if form == "w" else []
            call = wide_call()
            if call == "rowsets":
                options += [("rowsets", [n]) for n in sorted(m.sets) if n != "few"]
            elif call == "where":
                options += [("where", [list(p)]) for p in PREDS]
            mask = wrng.random(m.n) < min(1.0, 600.0 / max(int(m.alive.sum()), 1))
            if kind == "unsure":
                mask |= m.declined
            options.append(("masked", mask))
            step = k = None
            for call, filt in options:
                s = {"kind": "search", "form": "w" if call == "plain" else "wf", "plane": plane, "qs": q[None, :].copy(), "deliberate": kind, "call": call, "filt": filt}
                live, sure = wide_counts(s)
                want = {"all_but_one": live - 1, "all": live, "unsure": sure + 1 if live - sure >= 2 else 0}[kind]
                if 65 <= want <= Wd.MAX_K:
                    step, k = s, want
                    break
        if k is None:
            return False
        wcount["route"] += 1
        wide_push(step, k)
        return True

    def wide_round():
        left = WIDE_PER_ROUND
        if (m.n + 63) // 64 >= 8:
            for kind in list(wqueue):                                                        # one deliberate case a round, the first that can be met
                if wide_deliberate(kind):
                    wqueue.remove(kind); left -= 1
                    break
        for j in range(left):
            wide_plain()

    def search_round(extra=None):
        _search_round(extra)
        if wide:
            wide_round()

    def _search_round(extra=None):
        for j in range(3):
            form, plane = routes[(5 * seed + count["search"]) % len(routes)]; count["search"] += 1
            search(form, plane)
        if extra in ("zero", "nan"):
            plane = (("bf16", "8bit", "6bit"), ("8bit", "6bit", "bf16"))[extra == "nan"][seed // 2 % 3]
            if plane == "6bit" and dim % 64:
                plane = "8bit"
            search("1" if plane == "6bit" else ("1", "mq")[(seed + (extra == "nan")) % 2], plane, extra)
        elif extra == "short":
            search(("1f", "mqf")[seed % 2], ("bf16", "8bit")[seed // 2 % 2], "short")

    add(FIRST[int(rng.integers(len(FIRST)))] if seed >= len(FIRST) else FIRST[seed], facets_now=True)
    push({"kind": "rowset", "name": "a", "mask": rng.random(m.n) < 0.7})
    few = np.zeros(m.n, bool); few[rng.choice(m.n, 5, replace=False)] = True
    push({"kind": "rowset", "name": "few", "mask": few})                                     # five rows: fewer than k = 10, whatever lives
    search_round()
    first = ["add_small", "remove", "update", "update_rows", "add_big"]
    second = ["add_small", "add_synthetic", "remove", "revive", "update_rows", "update_rows_device", "remove", "add_small", "update_rows", "update"]
    done = 0
    for kind in [first[i] for i in rng.permutation(len(first))]:
        mutate(kind); done += 1
        if done % 2 == 0:
            search_round()
    if not grown():                                                                          # (a short first add: one long add does not pass the reservation)
        mutate("add_big")
    assert grown()
    push({"kind": "rowset", "name": "b", "mask": rng.random(m.n) < 0.5})                   # made before the later adds
    extras = ["zero", "nan", "short", None, None]
    for kind in [second[i] for i in rng.permutation(len(second))]:
        mutate(kind); done += 1
        if done % 2 == 0:
            search_round(extras.pop(0) if extras else None)
    while extras and extras[0]:
        search_round(extras.pop(0))
    assert m.n <= 2100
    return cfg, steps


def writers(cfg, steps):
    """the writer kinds a schedule holds, from the steps alone"""
    out, n, alive, first_tiles = set(), 0, np.zeros(0, bool), None
    for s in steps:
        k = s["kind"]
        if k in ("add", "add_synthetic"):
            cnt = len(s["vecs"]) if k == "add" else s["n"]
            out.add(k)
            if n % 64:
                out.add("add_partial_tile")
            if first_tiles is None:
                first_tiles = max(FIRST_TILES, (cnt + 63) // 64)
            elif (n + 63) // 64 <= first_tiles < (n + cnt + 63) // 64:
                out.add("add_growth")
            n += cnt; alive = np.concatenate([alive, np.ones(cnt, bool)])
        elif k == "remove":
            out.add("remove"); alive[s["rows"]] = False
        elif k == "update":
            out.add("update" if alive[s["row"]] else "revival"); alive[s["row"]] = True
        elif k == "update_rows":
            out.add("update_rows_device" if s["device"] else "update_rows")
            if not alive[s["rows"]].all():
                out.add("revival")
            alive[s["rows"]] = True
    return out


# ---- the checker -------------------------------------------------------------------------------------------------------------------------
class _Arrays:
    """what tests/test_gpu_row_state.check reads of an index"""

    def __init__(self, arrays, dim):
        self.arrays, self.dim = arrays, dim

    def debug_read(self, what):
        return self.arrays[what]


def slots8(a, tiles, dim):
    """[tiles * 64, dim] int8 from [tile][dim / 16][64 rows][16 B]"""
    return a.view(np.int8).reshape(tiles, dim // 16, 64, 16).transpose(0, 2, 1, 3).reshape(tiles * 64, dim)


def slots6(a, tiles, dim):
    """[tiles * 64, dim / 64, 3, 16] uint8 from [tile][group][3][64 rows][16 B]"""
    return a.reshape(tiles, dim // 64, 3, 64, 16).transpose(0, 3, 1, 2, 4).reshape(tiles * 64, dim // 64, 3, 16)


def codes6(p):
    """the signed codes [rows, dim] of slots6's pieces: dims 0 - 47 the low six bits of byte d & 15 of piece d >> 4, dims 48 - 63 two bits in
    the top of byte d - 48 of each piece (X bits 0 - 1, Y bits 2 - 3, Z bits 4 - 5); stored biased by 32"""
    low = (p & 0x3F).reshape(p.shape[0], p.shape[1], 48)
    top = (p >> 6).astype(np.int64)
    high = top[:, :, 0, :] | (top[:, :, 1, :] << 2) | (top[:, :, 2, :] << 4)
    return (np.concatenate([low.astype(np.int64), high], axis=2) - 32).reshape(p.shape[0], -1)


def _same32(got, want):
    """per entry: the same float32 bits, a NaN where the twin has one"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return np.where(np.isnan(want), np.isnan(got), got.view(np.uint32) == want.view(np.uint32))


def _first(mask, at):
    return at[~mask][:5].tolist()


def _float64_tier(what, name, r, step, codes, res, bound, at):
    """the statement that does not pass through the library's quantiser: from the codes and the scale READ BACK, in float64"""
    e = r - step[:, None] * codes
    t = np.sqrt(np.sum(e * e, axis=1))
    g = res.astype(np.float64)
    assert (g >= t).all(), (what, name + ": the residual is below the float64 residual of the stored codes", _first(g >= t, at))
    assert (g <= t * (1.0 + 1e-6)).all(), (what, name + ": the residual is more than 1e-6 above it", _first(g <= t * (1.0 + 1e-6), at))
    ok = (np.abs(e) <= bound[:, None]).all(axis=1)
    assert ok.all(), (what, name + ": an element is further from its code than the quantiser's step allows (stale codes?)", _first(ok, at))


def check_state(arrays, model, what="", tiers=(1, 2)):
    """every array of `arrays` (name -> what debug_read returned) against the model, for every live row"""
    n, dim, live = model.n, model.dim, model.alive
    tiles = (n + 63) // 64
    at = np.flatnonzero(live)
    check(_Arrays(arrays, dim), model.exp, n, live, what)                                    # rnorm, rres and the bfloat16 copy
    if "rowmaj16" in arrays:                                                                 # the same bits in row order
        got, want = arrays["rowmaj16"].reshape(n, dim)[live], model.exp.rh_bits[live]
        isnan16 = ((got & 0x7F80) == 0x7F80) & ((got & 0x007F) != 0)
        ok = np.where(model.exp.nan[live], isnan16, got == want).all(axis=1)
        assert ok.all(), (what, "rowmaj16", _first(ok, at))
    declined = declined_rows(model.rows, model.exp.rn)
    sure = live & ~declined
    r = model.rows[sure].astype(np.float64)
    if "plane8" in arrays:
        b = slots8(arrays["plane8"], tiles, dim)[:n]
        res = arrays["rres8"][:n]
        sc = arrays["rscale8"][:n] if "rscale8" in arrays else model.s8.scale                # (unreadable without the 6-bit plane: the twin's stands in)
        if 1 in tiers:
            ok = (b[live] == model.s8.r8[live]).all(axis=1)
            assert ok.all(), (what, "plane8 is not the host twin's", _first(ok, at))
            ok = _same32(res[live], model.s8.res[live])
            assert ok.all(), (what, "rres8 is not the host twin's", _first(ok, at))
            ok = sc[live].view(np.uint32) == model.s8.scale[live].view(np.uint32)
            assert ok.all(), (what, "rscale8 is not the host twin's", _first(ok, at))
        if 2 in tiers:
            ok = np.isnan(res[live]) == declined[live]
            assert ok.all(), (what, "rres8: NaN on the rows the bound declines, and only on them", _first(ok, at))
            s = sc[sure].astype(np.float64)
            c = b[sure].astype(np.float64)
            assert (np.abs(c) <= 127).all(), (what, "plane8: a byte of -128")
            ok = s >= np.abs(r).max(axis=1) / 127.0
            assert ok.all(), (what, "rscale8 below max|r| / 127", _first(ok, np.flatnonzero(sure)))
            _float64_tier(what, "8-bit plane", r, s, c, res[sure], 0.5 * s * (1.0 + ELEM8), np.flatnonzero(sure))
    if "plane6" in arrays:
        p = slots6(arrays["plane6"], tiles, dim)
        res = arrays["rres6"][:n]
        sc = arrays["rscale8"][:n]
        if 1 in tiers:
            ok = (p[:n][live].reshape(len(at), -1) == model.s6.bytes[live]).all(axis=1)
            assert ok.all(), (what, "plane6 is not the host twin's", _first(ok, at))
            ok = _same32(res[live], model.s6.res[live])
            assert ok.all(), (what, "rres6 is not the host twin's", _first(ok, at))
            assert (p[n:] == np.array([32, 32, 160], np.uint8)[None, None, :, None]).all(), (what, "plane6: the slots past the last row do not hold the zero-row code")
        if 2 in tiers:
            ok = np.isnan(res[live]) == declined[live]
            assert ok.all(), (what, "rres6: NaN on the rows the bound declines, and only on them", _first(ok, at))
            s = sc[sure].astype(np.float64)
            c = codes6(p[:n][sure]).astype(np.float64)
            assert (c >= -32).all() and (c <= 31).all()
            _float64_tier(what, "6-bit plane", r, 4.0 * s, c, res[sure], 3.0 * s * (1.0 + ELEM6), np.flatnonzero(sure))


# ---- "device" arrays from the host twins (for the CPU test of the checker) ---------------------------------------------------------------
def per_row(model):
    """name -> one entry per row, as the twins compute them"""
    e = model.exp
    bits = np.where(e.nan, np.uint16(0x7FC0), e.rh_bits).astype(np.uint16)
    out = {"rnorm": e.rn.copy(), "rres": e.res_up.copy(), "plane": bits, "plane8": model.s8.r8.copy(), "rres8": model.s8.res.copy(), "rscale8": model.s8.scale.copy()}
    if model.s6 is not None:
        out.update(plane6=model.s6.bytes.copy(), rres6=model.s6.res.copy())
    return out


def layout(rowwise, cfg):
    """per_row's entries in the device's layouts, for the arrays the configuration keeps"""
    n, dim = rowwise["plane"].shape
    tiles = (n + 63) // 64

    def pad(a, fill=0):
        out = np.full((tiles * 64,) + a.shape[1:], fill, a.dtype)
        out[:n] = a
        return out
    out = {"rnorm": pad(rowwise["rnorm"]), "rres": pad(rowwise["rres"]), "rres8": pad(rowwise["rres8"])}
    out["plane"] = np.ascontiguousarray(pad(rowwise["plane"]).reshape(tiles, 2, 32, dim // 16, 2, 8).transpose(0, 3, 1, 4, 2, 5)).reshape(-1)
    out["plane8"] = np.ascontiguousarray(pad(rowwise["plane8"]).reshape(tiles, 64, dim // 16, 16).transpose(0, 2, 1, 3)).reshape(-1).view(np.uint8)
    if "plane6" in cfg["keeps"]:
        p = np.empty((tiles * 64, dim // 64, 3, 16), np.uint8)
        p[:] = np.array([32, 32, 160], np.uint8)[None, None, :, None]
        p[:n] = rowwise["plane6"].reshape(n, dim // 64, 3, 16)
        out["plane6"] = np.ascontiguousarray(p.reshape(tiles, 64, dim // 64, 3, 16).transpose(0, 2, 3, 1, 4)).reshape(-1)
        out["rres6"] = pad(rowwise["rres6"]); out["rscale8"] = pad(rowwise["rscale8"])
    if "rowmaj16" in cfg["keeps"]:
        out["rowmaj16"] = rowwise["plane"].copy()
    assert np.array_equal(decode(out["plane"], tiles, dim)[:n], rowwise["plane"])
    return out
