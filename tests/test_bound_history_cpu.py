"""tests/_history.py without a device: the schedules tests/test_gpu_bound_history.py replays cover every writer, route, metric and
dimension (from plan(seed) alone); the state checker passes on arrays fabricated from the host twins and FAILS on each mutant a faulty writer
or plane kernel would leave; and the CPU models of the three stages hand back at most one search in ten of a schedule beside the deliberate
ones (a set of fewer than k rows, a zero query, a NaN query).  The searches of the wide form (65 <= k <= 1024) that end every round leave
the rest of a schedule as it was, cover every wide route, k, filtered call and deliberate case, stay within the same cap, and carry survivor
counts that each planted fault of stage 1 moves (H.Model.predict_wide)."""
import collections
import functools

import numpy as np
import pytest

from tests import _history as H

MODEL_SEEDS = (0, 4, 8, 9, 13, 17, 21, 25, 29)      # the seeds whose searches the CPU models run through HERE (every metric, style and dimension);
                                                    # tests/test_gpu_bound_history.py asserts the same cap for every seed it replays


@functools.lru_cache(maxsize=None)
def plans():
    return {seed: H.plan(seed) for seed in H.SEEDS}


def same_plan(p0, p1):
    (c0, s0), (c1, s1) = p0, p1
    assert c0 == c1 and len(s0) == len(s1)
    for a, b in zip(s0, s1):
        assert a.keys() == b.keys() and a["kind"] == b["kind"]
        for key in a:
            assert repr(a[key]) == repr(b[key]) if not isinstance(a[key], np.ndarray) else np.array_equal(a[key], b[key], equal_nan=True), key


def test_the_plan_is_a_pure_function_of_the_seed():
    same_plan(H.plan(7), H.plan(7))
    assert any(H.is_wide(s) for s in H.plan(7)[1])


@pytest.mark.parametrize("seed", H.SEEDS)
def test_the_wide_searches_leave_the_schedule_as_it_was(seed):
    """without its wide steps a plan is plan(seed, wide=False), step by step: they draw from a generator of their own"""
    cfg, steps = plans()[seed]
    narrow = [s for s in steps if not H.is_wide(s)]
    assert len(narrow) < len(steps)
    before = H.plan(seed, wide=False)
    same_plan((cfg, narrow), before)
    assert not any(H.is_wide(s) for s in before[1])


def test_the_schedules_cover_every_writer_route_metric_and_dimension():
    wm, rm, dm, firsts = collections.Counter(), collections.Counter(), collections.Counter(), collections.Counter()
    calls, ks, nqs, deliberate, searches = collections.Counter(), collections.Counter(), collections.Counter(), collections.Counter(), 0
    below = 0
    for seed, (cfg, steps) in plans().items():
        metric = cfg["metric"]
        dm[(cfg["dim"], metric)] += 1
        firsts[len(steps[0]["vecs"])] += 1
        for w in H.writers(cfg, steps):
            wm[(w, metric)] += 1
        n_final = sum(len(s["vecs"]) if s["kind"] == "add" else s["n"] for s in steps if s["kind"] in ("add", "add_synthetic"))
        assert n_final <= 2100 < 4096                                                       # below the candidate list's capacity: no overflow hand-back
        for s in steps:
            if s["kind"] != "search" or H.is_wide(s):                                        # (the wide searches: the test below)
                continue
            searches += 1
            below += s["after"]["tiles"] < 8
            calls[s["call"]] += 1; ks[s["k"]] += 1; nqs[len(s["qs"])] += 1; deliberate[s["deliberate"]] += 1
            if s["after"]["growth"] and s["after"]["update_rows"] and s["after"]["tiles"] >= 8:
                rm[((s["form"], s["plane"]), metric)] += 1
            if s["call"] == "rowsets":
                assert any(f is not None for f in s["filt"])
            assert s["form"] in ("1", "1f") and len(s["qs"]) == 1 or s["form"] in ("mq", "mqf") and 2 <= len(s["qs"]) <= 8
            assert (s["call"] == "plain") == (s["form"] in ("1", "mq")) and (s["plane"] != "6bit" or (s["form"] == "1" and cfg["dim"] % 64 == 0))
    print("searches: %d, of them on fewer than 8 tiles: %d; deliberate hand-backs: %s" % (searches, below, dict(deliberate)))
    print("calls %s, k %s, queries %s, first adds %s" % (dict(calls), dict(sorted(ks.items())), dict(sorted(nqs.items())), dict(sorted(firsts.items()))))
    for metric in H.METRICS:
        print("%-6s writers: %s" % (metric, ", ".join("%s x%d" % (w, wm[(w, metric)]) for w in H.WRITERS)))
        print("%-6s routes after a growth and an update_rows: %s" % (metric, ", ".join("%s/%s x%d" % (r[0], r[1], rm[(r, metric)]) for r in H.ROUTES)))
        for w in H.WRITERS:
            assert wm[(w, metric)] >= 1, (w, metric)
        for r in H.ROUTES:
            assert rm[(r, metric)] >= 3, (r, metric, rm[(r, metric)])
        for dim in H.DIMS:
            assert dm[(dim, metric)] >= 1, (dim, metric)
    assert set(firsts) == set(H.FIRST) and below >= 3
    assert set(calls) == {"plain", "masked", "rowsets", "where"} and set(H.KS) <= set(ks) and {1, 2, 3, 4, 5, 8} <= set(nqs)
    assert all(deliberate[d] >= len(H.SEEDS) for d in ("zero", "nan", "short"))
    styles = {(H.config(s)["style"], H.config(s)["metric"]) for s in H.SEEDS}
    assert len(styles) == 9 and any("rowmaj16" in H.config(s)["keeps"] for s in H.SEEDS)


# ---- the checker ---------------------------------------------------------------------------------------------------------------------------
def history(seed):
    """a short history: an add, an update of a live row with a different vector, a bulk overwrite -> (cfg, model, the updated row, the
    per-row entries before the update and after it)"""
    cfg = H.config(seed)
    rng = np.random.default_rng(seed)
    dim = cfg["dim"]
    m = H.Model(cfg)
    x = H.vectors(rng, 200, dim, "gauss")
    x[7] = 0.0; x[8, 3] = np.nan; x[9] *= np.float32(1e-30)                                 # rows the bound declines
    m.apply({"kind": "add", "vecs": x})
    m.apply({"kind": "remove", "rows": np.array([5, 70, 199], np.uint32)})
    before = H.per_row(m)
    row = 66
    m.apply({"kind": "update", "row": row, "vec": (rng.standard_normal(dim) * 37.5).astype(np.float32)})
    m.apply({"kind": "update_rows", "rows": np.array([63, 64, 70, 63], np.uint32), "vecs": H.vectors(rng, 4, dim, "gauss")})
    return cfg, m, row, before, H.per_row(m)


def mutants(cfg, row, before, after):
    """(name, the per-row entries of a faulty index, the tiers that must see it)"""
    def with_(**changes):
        out = {k: v.copy() for k, v in after.items()}
        for name, fn in changes.items():
            fn(out[name])
        return out

    def stale(a, name):
        a[row] = before[name][row]

    def scaled(a):
        a[row] *= np.float32(0.9)

    def step_down(a):
        a[row] = np.nextafter(a[row], np.float32(0.0))
    out = [("plane8 left at the row's previous vector", with_(plane8=lambda a: stale(a, "plane8")), ((1, 2), (1,), (2,))),
           ("plane left at the row's previous vector", with_(plane=lambda a: stale(a, "plane")), ((1, 2),)),
           ("rres8 times 0.9", with_(rres8=scaled), ((1, 2), (1,), (2,))),
           ("rres times 0.9", with_(rres=scaled), ((1, 2),)),
           ("rnorm left at the old value", with_(rnorm=lambda a: stale(a, "rnorm")), ((1, 2),)),
           ("a NaN residual replaced by 0 on a declined row", with_(rres8=lambda a: a.__setitem__(7, 0.0)), ((1, 2), (1,), (2,)))]
    if "plane6" in cfg["keeps"]:
        out += [("plane6 left at the row's previous vector", with_(plane6=lambda a: stale(a, "plane6")), ((1, 2), (1,), (2,))),
                ("rres6 times 0.9", with_(rres6=scaled), ((1, 2), (1,), (2,))),
                ("rscale8 one float32 step down", with_(rscale8=step_down), ((1, 2), (1,)))]
    # bytes, scale and residuals stale TOGETHER: consistent with each other, so only the element bound of the float64 tier can tell
    quantised = [k for k in ("plane8", "rres8", "rscale8", "plane6", "rres6") if k in after]
    out.append(("every quantised array left at the row's previous vector", with_(**{k: (lambda a, k=k: stale(a, k)) for k in quantised}), ((1, 2), (1,), (2,))))
    swapped = {k: v.copy() for k, v in after.items()}
    for v in swapped.values():
        v[[20, 41]] = v[[41, 20]]
    out.append(("two rows' slots swapped within a tile", swapped, ((1, 2), (1,), (2,))))
    for name in ("plane8",) + (("plane6",) if "plane6" in cfg["keeps"] else ()):
        one = {k: v.copy() for k, v in after.items()}
        one[name][[20, 41]] = one[name][[41, 20]]
        out.append(("%s: two rows' slots swapped within a tile" % name, one, ((1, 2), (2,))))
    return out


def kept(arrays, cfg):
    return {k: v for k, v in arrays.items() if k in cfg["keeps"]}


@pytest.mark.parametrize("seed", [3, 6, 15])         # 48 dimensions (no 6-bit plane, no readable scale), 64 with the row-order copy, 768
def test_the_checker_passes_on_the_twins_and_fails_on_every_mutant(seed):
    cfg, m, row, before, after = history(seed)
    assert not np.array_equal(before["plane8"][row], after["plane8"][row]) and m.declined[[7, 8, 9]].all() and m.alive[70]
    H.check_state(kept(H.layout(after, cfg), cfg), m, "the twins")
    H.check_state(kept(H.layout(after, cfg), cfg), m, "the twins, float64 tier alone", tiers=(2,))
    seen = 0
    for name, faulty, tiers in mutants(cfg, row, before, after):
        arrays = kept(H.layout(faulty, cfg), cfg)
        for t in tiers:
            with pytest.raises(AssertionError):
                H.check_state(arrays, m, name, tiers=t)
            seen += 1
    if "rowmaj16" in cfg["keeps"]:                                                          # the row-order copy alone left at the previous vector
        arrays = kept(H.layout(after, cfg), cfg)
        arrays["rowmaj16"][row] = before["plane"][row]
        with pytest.raises(AssertionError):
            H.check_state(arrays, m, "rowmaj16 left at the row's previous vector")
        seen += 1
    assert seen >= 14


def test_the_element_bound_of_the_8bit_plane_is_the_derived_one():
    """the host quantiser itself leaves an element further than 0.5 scale (1 + 1e-6) from its byte on rows these schedules hold — a float32
    quotient within 2^-18 of a half-integer — and never further than 0.5 scale (1 + 2^-17): H.ELEM8"""
    worst = 0.0
    for seed in (16, 34):
        cfg, steps = plans()[seed]
        m = H.Model(cfg)
        for s in steps:
            if s["kind"] != "search":
                m.apply(s)
        sure = ~m.declined
        r, s, c = m.rows[sure].astype(np.float64), m.s8.scale[sure].astype(np.float64)[:, None], m.s8.r8[sure].astype(np.float64)
        worst = max(worst, float((np.abs(r - s * c) / (0.5 * s)).max()) - 1.0)
    print("largest |r - scale r8| / (0.5 scale) - 1 = %.3g; 2^-17 = %.3g" % (worst, 2.0 ** -17))
    assert 1e-6 < worst <= H.ELEM8 == 2.0 ** -17


# ---- the hand-back cap -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", MODEL_SEEDS)
def test_the_models_hand_back_at_most_one_search_in_ten(seed):
    cfg, steps = plans()[seed]
    m = H.Model(cfg)
    plain = backs = 0
    seen = collections.Counter()
    for s in steps:
        if s["kind"] != "search":
            m.apply(s)
            continue
        if s["after"]["tiles"] < 8 or H.is_wide(s):                                          # (the wide searches: the tests below)
            continue
        back = {"bf16": 0, "8bit": 0, "6bit": 0}
        for q, sel in zip(s["qs"], m.selected(s)):
            alive = m.candidates(sel)
            back["bf16"] += bool(m.ref16(q, s["k"], alive)["hand_back"])
            back["8bit"] += bool(m.ref8(q, s["k"], alive)["hand_back"])
            if cfg["dim"] % 64 == 0:
                back["6bit"] += bool(m.ref6(q, s["k"], alive)["hand_back"])
        if s["deliberate"]:
            assert back["bf16"] == back["8bit"] == 1 and back["6bit"] in (0, 1), (s["deliberate"], back)   # that query alone, in every stage
            seen[s["deliberate"]] += 1
        else:
            plain += 1; backs += any(back.values())
    print("seed %d (%s, %d dims, %s): %d searches, %d with a predicted hand-back, deliberate %s" % (seed, cfg["metric"], cfg["dim"], cfg["style"], plain, backs, dict(seen)))
    assert backs * 10 <= plain and plain >= 15
    assert set(seen) == {"zero", "nan", "short"}


# ---- the wide form (65 <= k <= 1024) ----------------------------------------------------------------------------------------------------------
CUS = 256                                           # compute units the models lay the grid out for: from 5 on a wave owns one tile at these sizes, whatever the device has
FAULTS = ("dead", "unselected", "rank", "stale")    # H.Model.predict_wide's


def test_the_schedules_cover_every_wide_route_k_call_and_deliberate_case():
    rm, ks, calls, deliberate, queries = collections.Counter(), collections.Counter(), collections.Counter(), collections.Counter(), collections.Counter()
    total = below = 0
    for seed, (cfg, steps) in plans().items():
        metric, here = cfg["metric"], set()
        m = H.Model(cfg, derive=False)
        for s in steps:
            if s["kind"] != "search":
                m.apply(s)
                continue
            if not H.is_wide(s):
                continue
            total += 1
            below += s["after"]["tiles"] < 8
            assert len(s["qs"]) == 1 and (s["form"], s["plane"]) in H.WIDE_ROUTES and (s["call"] == "plain") == (s["form"] == "w")
            assert s["call"] in ("plain", "masked") or (len(s["filt"]) == 1 and s["filt"][0] is not None)   # a single query never names None alone
            live = m.candidates(m.selected(s)[0])
            sure = int((live & ~m.declined).sum())
            q = s["qs"][0]
            if s["deliberate"]:
                deliberate[(s["deliberate"], metric)] += 1; here.add(s["deliberate"])
                assert s["after"]["tiles"] >= 8 and 65 <= s["k"] <= 1024
            if s["deliberate"] in (None, "zero", "nan"):
                assert s["k"] in H.KS_WIDE and s["k"] < sure, (seed, s["k"], sure)
            if s["deliberate"] is None:
                assert not H.declined_rows(q[None, :])[0]
                dead = ~m.alive & (m.rows.view(np.uint32) == q.view(np.uint32)[None, :]).all(axis=1)
                queries["a dead row's vector"] += bool(dead.any())
                queries["the previous vector of a replaced row"] += s["stale_vec"] is not None and np.array_equal(s["stale_vec"], q)
            elif s["deliberate"] == "all_but_one":
                assert s["k"] == int(live.sum()) - 1
            elif s["deliberate"] == "all":
                assert s["k"] == int(live.sum())
            elif s["deliberate"] == "unsure":
                assert sure < s["k"] < int(live.sum())
            ks[s["k"]] += 1; calls[s["call"]] += 1
            if s["after"]["growth"] and s["after"]["update_rows"] and s["after"]["tiles"] >= 8:
                rm[((s["form"], s["plane"]), metric)] += 1
        assert {"zero", "nan"} <= here, (seed, here)                                         # every seed reaches 8 tiles
    print("wide searches: %d, of them on fewer than 8 tiles: %d; calls %s; k %s; queries %s" % (total, below, dict(calls), dict(sorted(ks.items())), dict(queries)))
    for metric in H.METRICS:
        print("%-6s wide routes after a growth and an update_rows: %s; deliberate: %s" % (metric, ", ".join("%s/%s x%d" % (r[0], r[1], rm[(r, metric)]) for r in H.WIDE_ROUTES),
              ", ".join("%s x%d" % (d, deliberate[(d, metric)]) for d in H.WIDE_DELIBERATE)))
        for r in H.WIDE_ROUTES:
            assert rm[(r, metric)] >= 3, (r, metric, rm[(r, metric)])
        for d in H.WIDE_DELIBERATE:
            assert deliberate[(d, metric)] >= 1, (d, metric)
    assert set(H.KS_WIDE) <= set(ks) and set(calls) == {"plain", "masked", "rowsets", "where"} and below >= 1
    assert all(v >= 3 for v in queries.values()) and len(queries) == 2, queries


@functools.lru_cache(maxsize=None)
def wide_evals(seed):
    """of every wide search of a schedule on 8 tiles or more: (the step, the model's prediction, the prediction with the 8-bit plane first
    — a hand-back there is one in BOTH stages —, {fault: the prediction under it} for the searches that are not deliberate)"""
    cfg, steps = plans()[seed]
    m = H.Model(cfg)
    out = []
    for s in steps:
        if s["kind"] != "search":
            m.apply(s)
            continue
        if not H.is_wide(s) or s["after"]["tiles"] < 8:
            continue
        cache = {}
        want = m.predict_wide(s, CUS, cache=cache)
        both = m.predict_wide(dict(s, plane="8bit"), CUS, cache=cache)
        faulty = {}
        if not s["deliberate"]:
            for f in FAULTS:
                if f != "unselected" or s["form"] == "wf":
                    faulty[f] = m.predict_wide(s, CUS, fault=f, cache=cache)
        out.append((s, want, both, faulty))
    return out


@pytest.mark.parametrize("seed", MODEL_SEEDS)
def test_the_wide_model_hands_back_at_most_one_search_in_ten_and_the_deliberate_cases_are_what_they_are_for(seed):
    cfg = H.config(seed)
    plain = backs = 0
    seen = collections.Counter()
    cands = []
    for s, want, both, _ in wide_evals(seed):
        kind = s["deliberate"]
        if kind is None:
            assert want["took"] == 1, (s["k"], want)                                         # k is below the candidates the bound is sure of
            plain += 1; backs += want["back"]
            cands.append((s["k"], want["cand"]))
            continue
        seen[kind] += 1
        if kind in ("zero", "nan", "unsure"):
            assert want["took"] == 1 and want["back"] == 1 and both["back"] == 1, (kind, want, both)
        elif kind == "all":
            assert want == {"took": 0, "back": 0, "cand": None}, want
        else:
            assert want["took"] == 1, want
    print("seed %d (%s, %d dims, %s): %d wide searches, %d with a predicted hand-back, deliberate %s; (k, survivors) %s"
          % (seed, cfg["metric"], cfg["dim"], cfg["style"], plain, backs, dict(seen), cands))
    assert backs * 10 <= plain and plain >= 6
    assert set(seen) >= {"zero", "nan", "all", "all_but_one"} | ({"unsure"} if cfg["style"] != "gauss" else set()), seen


def test_the_wide_survivor_counts_tell_a_faulty_stage_1():
    """each planted fault changes the predicted survivor count of a scheduled wide search of every metric: dead rows keyed, unselected live
    rows keyed under a filter, H taken one rank early, the last overwritten row left with its previous vector's interval"""
    moved, asked = collections.Counter(), collections.Counter()
    for seed in MODEL_SEEDS:
        metric = H.config(seed)["metric"]
        for s, want, _, faulty in wide_evals(seed):
            for f, got in faulty.items():
                if want["cand"] is None or got["cand"] is None:
                    continue
                asked[(f, metric)] += 1
                moved[(f, metric)] += got["cand"] != want["cand"]
    for metric in H.METRICS:
        print("%-6s searches whose count a fault moves: %s" % (metric, ", ".join("%s %d of %d" % (f, moved[(f, metric)], asked[(f, metric)]) for f in FAULTS)))
    for metric in H.METRICS:
        for f in FAULTS:
            assert moved[(f, metric)] >= 1, (f, metric, asked[(f, metric)])
