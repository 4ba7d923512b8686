"""The CPU model of the WIDE shared bound pass (2 - 8 queries, 65 <= k <= 1024; quiver_amd/csrc/qv_bound_scan.hip: bound_scan_tail_wide_mq,
k_bound_collect_wide_mq, k_bound_rescore_wide_mq): tests/_wide.py's model of one query, asked once per query of the pass — every query of a
pass has its own lists, its own H, its own survivors and its own fate — and the pass's counters made of the answers.  The row state of a
corpus is derived once and shared by the queries.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from tests import _bound as B
from tests import _bound8 as B8
from tests import _bound_l2 as BL2
from tests import _wide as Wd
from tests import _widths as W

CAP = Wd.CAP
ARMS = Wd.ARMS


class States:
    """what ingest derives of a corpus for both arms, once"""

    def __init__(self, rows, arms=ARMS):
        self.rows = np.ascontiguousarray(rows, np.float32)
        self.bf16 = B.RowState(self.rows) if "bf16" in arms else None
        self.plane8 = B8.RowState8(self.rows) if "8bit" in arms else None
        self.kept = {}                                                    # (metric, arm, the query's bytes) -> its stage: computed once


def declined(q):
    """a query no stage can work with: a non-finite element, no non-zero element, or a norm tests/_bound.query_ok declines"""
    q = np.ascontiguousarray(q, np.float32)
    return not np.all(np.isfinite(q)) or not np.any(q != 0) or not B.query_ok(B.chain_norm(q), q.size)


def stage_of(metric, arm, states, q):
    """tests/_wide.stage_of over a shared row state, kept per query"""
    key = (metric, arm, np.ascontiguousarray(q, np.float32).tobytes())
    if key not in states.kept:
        if arm == "8bit":
            states.kept[key] = W.stage8_of(metric, states.plane8, q)
        else:
            states.kept[key] = BL2.stage1(states.bf16, q) if metric == Wd.L2 else B.stage1(metric, states.bf16, q)
    return states.kept[key]


def decide_stages(stages, k, live, n_tiles, grid, **fault):
    """the model of one arm of a pass from its queries' stages: tests/_wide.decide_wide once per query, each over its own lists (None stays
    None: a query the arm declines outright).  A pass of one query is tests/_wide.decide_wide itself."""
    return [None if st is None else Wd.decide_wide(st, k, live, n_tiles, grid, **fault) for st in stages]


def decide_pass(metric, arm, states, qs, k, live, n_tiles, grid):
    """decide_stages over the stages of the pass's queries on one arm"""
    return decide_stages([None if declined(q) else stage_of(metric, arm, states, q) for q in qs], k, live, n_tiles, grid)


def fates(metric, plane, states, qs, k, live, n_tiles, grid):
    """what the pass's counters must say with `plane` first: per query the stage that answers it ("8bit", "bf16" or "redo": handed back to
    the key-per-row path) and its survivor count there; cand = the largest count among the answered queries in the stage that answered
    each, back = queries handed back, took = len(qs), dropped = the most keys of the k smallest no list of an answering stage held"""
    first = decide_pass(metric, "8bit", states, qs, k, live, n_tiles, grid) if plane == "8bit" else [None] * len(qs)
    out = []
    for j, q in enumerate(qs):
        m = first[j]
        if plane == "8bit" and m is not None and not m["hand_back"]:
            out.append(("8bit", m["count"], m["dropped"]))
            continue
        m = None if declined(q) else Wd.decide_wide(stage_of(metric, "bf16", states, q), k, live, n_tiles, grid)
        out.append(("redo", 0, 0) if m is None or m["hand_back"] else ("bf16", m["count"], m["dropped"]))
    answered = [f for f in out if f[0] != "redo"]
    return {"per_query": out, "cand": max([f[1] for f in answered], default=0), "back": sum(f[0] == "redo" for f in out), "took": len(qs),
            "dropped": max([f[2] for f in answered], default=0)}
