"""tests/_history.py without a device: the schedules tests/test_gpu_bound_history.py replays cover every writer, route, metric and
dimension (from plan(seed) alone); the state checker passes on arrays fabricated from the host twins and FAILS on each mutant a faulty writer
or plane kernel would leave; and the CPU models of the three stages hand back at most one search in ten of a schedule beside the deliberate
ones (a set of fewer than k rows, a zero query, a NaN query)."""
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


def test_the_plan_is_a_pure_function_of_the_seed():
    (c0, s0), (c1, s1) = H.plan(7), H.plan(7)
    assert c0 == c1 and len(s0) == len(s1)
    for a, b in zip(s0, s1):
        assert a.keys() == b.keys() and a["kind"] == b["kind"]
        for key in a:
            assert repr(a[key]) == repr(b[key]) if not isinstance(a[key], np.ndarray) else np.array_equal(a[key], b[key], equal_nan=True), key


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
            if s["kind"] != "search":
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
        if s["after"]["tiles"] < 8:
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
