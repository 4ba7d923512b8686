"""Random interleavings of every writer — add, add_synthetic, an add inside a partly filled tile, an add that grows the arrays, update,
update_rows / update_rows_device, remove, the revival of a dead row — replayed on a DeviceIndex whose dimension and row count the bound scan's
kernels serve (tests/_history.plan).  After EVERY mutation each per-row array the bound scan's interval rests on is read back (debug_read)
and compared with the host twins bit for bit and with a float64 statement computed from the bytes and scales read back
(tests/_history.check_state); after every second one a sample of the routes is forced — one query or a shared pass of 2 - 8, filtered or not,
on the bfloat16 copy, the 8-bit plane or the 6-bit plane — and every search must return the CPU oracle's rows, counts and float32 bits on the
model, what the exact scan of the same index returns, and move the stages' counters exactly as the CPU models of the stages predict: the
intended stage took the search, and handed it back where the model does and nowhere else.

Every round of searches ends with searches of the WIDE form (65 <= k <= 1024; tests/_history.WIDE_ROUTES): unfiltered or under a mask, a row set
or a where-filter, on either plane, on indexes whose arrays have grown, whose ragged tile a later add filled, with revived rows and rows
overwritten from another stream.  The form is forced, its results are the oracle's and the exact path's, and the increments of
bound_scan_wide_stats — searches, hand-backs and the SURVIVOR COUNT of the stage that answered — equal tests/_history.Model.predict_wide:
a stage 1 that keys a dead or an unselected row, takes H one rank off or reads a stale plane is hidden by the exact re-score and shows
in that count alone.  After every deliberate hand-back an ordinary wide search on the same index must be answered: the gates and ticket
words are back in their initial state."""
import collections
import functools
import time

import numpy as np
import pytest

import quiver_amd
from quiver_amd.device_index import device_info
from tests import _extremes as X
from tests import _history as H

pytestmark = pytest.mark.gpu

COUNTERS = ("took6", "back6", "took8", "back8", "took", "back")
OTHER = {"bf16": "8bit", "8bit": "bf16"}


def read_arrays(idx, cfg):
    """every array the index keeps; one it does not keep answers with an unknown code or QV_ERR_UNSUPPORTED (tests/test_gpu_update_rows.state)"""
    out = {}
    for what in H.ARRAYS:
        try:
            out[what] = idx.debug_read(what)
        except quiver_amd.QvError as e:
            assert e.code in (-1, -8), (what, e)
    assert sorted(out) == sorted(cfg["keeps"]), sorted(out)
    return out


def mutate(idx, dev, model, step):
    kind = step["kind"]
    if kind == "add":
        assert idx.add(step["vecs"]) == model.n
        if "facets" in step:
            f = step["facets"]
            dev["u32"].set(model.n, f["u32"]); dev["f64"].set(model.n, f["f64"], f["present"])
    elif kind == "add_synthetic":
        assert idx.add_synthetic(step["seed"], 0, step["n"]) == model.n
    elif kind == "remove":
        idx.remove(step["rows"])
    elif kind == "update":
        idx.update(step["row"], step["vec"])
    elif kind == "update_rows" and not step["device"]:
        idx.update_rows(step["rows"], step["vecs"])
    elif kind == "update_rows":                                                             # the device form on a stream of its own
        import torch
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            d = torch.from_numpy(np.ascontiguousarray(step["vecs"], np.float32).copy()).to("cuda")
            idx.update_rows_device(step["rows"], d.data_ptr(), st.cuda_stream)
        st.synchronize()
    elif kind == "facets":
        dev["u32"].set(step["first"], step["u32"]); dev["f64"].set(step["first"], step["f64"], step["present"])
    elif kind == "rowset":
        dev["sets"][step["name"]] = idx.rowset(step["mask"])
    model.apply(step)


def force(idx, step):
    """the bound scan always, the form's own plane knob on the plane wanted — and every other form's on the other plane: the knobs are independent"""
    form, plane = step["form"], step["plane"]
    want = "8bit" if plane == "6bit" else plane
    idx.set_bound_scan("always")
    for name, setter in (("1", idx.set_bound_plane), ("1f", idx.set_bound_plane_filtered), ("mq", idx.set_bound_plane_mq), ("mqf", idx.set_bound_plane_filtered_mq)):
        setter(want if name == form else OTHER[want])
    idx.set_bound_plane6("always" if plane == "6bit" else "never")
    idx.set_bound_scan_wide("always"); idx.set_bound_scan_wide_filtered("always")            # (no search of 64 results or fewer may take them)


def force_wide(idx, step):
    """the wide form of the step's kind always, on the plane wanted; the other kind's never, its plane knob on the other plane; the k <= 64
    bound scan stays on, so that a leak into that form would show in its counters"""
    form, plane = step["form"], step["plane"]
    idx.set_bound_scan("always")
    idx.set_bound_scan_wide("always" if form == "w" else "never")
    idx.set_bound_scan_wide_filtered("always" if form == "wf" else "never")
    idx.set_bound_plane(plane if form == "w" else OTHER[plane])
    idx.set_bound_plane_filtered(plane if form == "wf" else OTHER[plane])


def stats(idx):
    return idx.bound_scan6_stats(), idx.bound_scan8_stats(), idx.bound_scan_stats()


@functools.lru_cache(maxsize=None)
def cus():
    return int(device_info(0)["cus"])


def wide_delta(s0, s1):
    return {"took": s1["searches"] - s0["searches"], "back": s1["hand_backs"] - s0["hand_backs"], "cand": s1["candidates"]}


def is_oracle(model, step, res, what):
    """the call's rows, counts and float32 bits are the CPU oracle's on the model (the padding: what the exact path of the same index leaves)"""
    r, d, c = res
    for j, (q, sel) in enumerate(zip(step["qs"], model.selected(step))):
        er, ed = model.search(q, step["k"], sel)
        w = len(er)
        assert int(c[j]) == w and r[j, :w].tolist() == er.tolist() and r.shape[1] == step["k"], (what, j, int(c[j]), w, r[j, :w], er)
        assert X.same(d[j, :w], ed), (what, j, d[j, :w], ed)


def predicates(dev, preds):
    return [(dev[c], op, lit) for c, op, lit in preds]


def call_of(idx, dev, step):
    qs, k, call, filt = step["qs"], step["k"], step["call"], step["filt"]
    if call == "plain":
        return lambda: idx.search(qs, k)
    if call == "masked":
        return lambda: idx.search_masked(qs, k, filt)
    if call == "rowsets":
        return lambda: idx.search_rowsets(qs, k, [None if f is None else dev["sets"][f] for f in filt])
    return lambda: idx.search_where(qs, k, [None if f is None else predicates(dev, f) for f in filt])


def search(idx, dev, model, step, what):
    """-> whether the models predicted a hand-back"""
    qs, k = step["qs"], step["k"]
    call = call_of(idx, dev, step)
    force(idx, step)
    w0 = idx.bound_scan_wide_stats()
    a0, b0, c0 = stats(idx)
    r, d, c = call()
    a1, b1, c1 = stats(idx)
    inc = {"took6": a1["searches"] - a0["searches"], "back6": a1["hand_backs"] - a0["hand_backs"], "cand6": a1["candidates"],
           "took8": b1["searches"] - b0["searches"], "back8": b1["hand_backs"] - b0["hand_backs"], "cand8": b1["candidates"],
           "took": c1["searches"] - c0["searches"], "back": c1["hand_backs"] - c0["hand_backs"], "cand": c1["candidates"]}
    assert idx.bound_scan_wide_stats() == w0, (what, "a search of 64 results or fewer moved the wide form's counters")
    # 1. the CPU oracle on the model
    for j, (q, sel) in enumerate(zip(qs, model.selected(step))):
        er, ed = model.search(q, k, sel)
        w = len(er)
        assert int(c[j]) == w and r[j, :w].tolist() == er.tolist() and r.shape[1] == k, (what, j, int(c[j]), w, r[j, :w], er)
        assert X.same(d[j, :w], ed), (what, j, d[j, :w], ed)
    # 2. the exact scan of the same index
    if step["call"] == "where":                                                             # ... and the sets the same predicates make, through search_rowsets
        sets = [None if f is None else idx.rowset_where(predicates(dev, f)) for f in step["filt"]]
        sr, sd, sc = idx.search_rowsets(qs, k, sets)
        assert np.array_equal(sr, r) and X.same(sd, d) and np.array_equal(sc, c), (what, "rowset_where + search_rowsets")
        for s in sets:
            if s is not None:
                s.close()
        a1, b1, c1 = stats(idx)
    idx.set_bound_scan("never")
    er, ed, ec = call()
    assert [s["searches"] for s in stats(idx)] == [a1["searches"], b1["searches"], c1["searches"]], (what, "never is never")
    assert np.array_equal(c, ec) and np.array_equal(r, er) and X.same(d, ed), (what, "against the exact scan", r, er)
    assert idx.bound_scan_wide_stats() == w0, (what, "a search of 64 results or fewer moved the wide form's counters")
    # 3. the counters: the intended stage took the search and handed it back exactly where its model does
    if (model.n + 63) // 64 < 8:
        assert not any(inc[key] for key in COUNTERS), (what, "fewer than 8 tiles", inc)
        return False
    want = model.predict(step)
    assert {key: inc[key] for key in COUNTERS} == {key: want[key] for key in COUNTERS}, (what, inc, want)
    for key in ("cand6", "cand8", "cand"):
        assert want[key] is None or inc[key] == want[key], (what, key, inc, want)
    return bool(want["back6"] or want["back8"] or want["back"])


def run_wide(idx, dev, model, step, what):
    """one forced wide search -> (its results, the model's prediction): the oracle's rows and bits, the wide form's counters as the model
    moves them, the k <= 64 form's and the 8-bit and 6-bit stages' not at all"""
    call = call_of(idx, dev, step)
    force_wide(idx, step)
    n0, w0 = stats(idx), idx.bound_scan_wide_stats()
    res = call()
    inc = wide_delta(w0, idx.bound_scan_wide_stats())
    assert stats(idx) == n0, (what, "a wide search moved the counters of the k <= 64 form", n0, stats(idx))
    is_oracle(model, step, res, what)
    want = model.predict_wide(step, cus())
    assert (inc["took"], inc["back"]) == (want["took"], want["back"]), (what, inc, want)
    assert want["cand"] is None or inc["cand"] == want["cand"], (what, "survivors", inc, want)
    return res, want


def follow_up(idx, dev, model, step, what):
    """directly behind a hand-back: an ordinary wide search of a stored row's vector on the same index and plane — under the same filter where
    it leaves 66 rows the bound is sure of, unfiltered otherwise — must be ANSWERED: the control words are as a first search finds them"""
    for form, call, filt in ((step["form"], step["call"], step["filt"]), ("w", "plain", None)):
        nxt = dict(step, form=form, call=call, filt=filt, deliberate=None, stale_row=None, stale_vec=None)
        sure = model.candidates(model.selected(nxt)[0]) & ~model.declined
        below = [k for k in H.KS_WIDE if k < int(sure.sum())]
        if below:
            break
    nxt.update(k=below[-1], qs=model.rows[np.flatnonzero(sure)[:1]].copy())
    _, want = run_wide(idx, dev, model, nxt, what + " follow-up")
    assert want["took"] == 1 and want["back"] == 0, (what, "the follow-up", want)


def search_wide(idx, dev, model, step, what):
    """-> the model's prediction {"took", "back", "cand"}"""
    call = call_of(idx, dev, step)
    (r, d, c), want = run_wide(idx, dev, model, step, what)
    if step["deliberate"] and want["back"]:
        follow_up(idx, dev, model, step, what)
    if step["call"] == "where":                                                             # the sets the same predicates make, through search_rowsets (the wide form too)
        force_wide(idx, step)
        sets = [idx.rowset_where(predicates(dev, f)) for f in step["filt"]]
        sr, sd, sc = idx.search_rowsets(step["qs"], step["k"], sets)
        assert np.array_equal(sr, r) and X.same(sd, d) and np.array_equal(sc, c), (what, "rowset_where + search_rowsets")
        for s in sets:
            s.close()
    # both wide knobs at never: the same arrays, padding included, and no wide counter moves
    idx.set_bound_scan_wide("never"); idx.set_bound_scan_wide_filtered("never")
    w0 = idx.bound_scan_wide_stats()
    er, ed, ec = call()
    assert idx.bound_scan_wide_stats() == w0, (what, "never is never")
    assert np.array_equal(c, ec) and np.array_equal(r, er) and X.same(d, ed), (what, "against the path the call takes without the wide form", r, er)
    return want


WIDE_WANT = {"zero": {"took": 1, "back": 1}, "nan": {"took": 1, "back": 1}, "unsure": {"took": 1, "back": 1}, "all": {"took": 0, "back": 0}, "all_but_one": {"took": 1}}


@pytest.mark.parametrize("seed", H.SEEDS)
def test_every_plane_and_route_follows_a_random_history(seed):
    t0 = time.time()
    cfg, steps = H.plan(seed)
    model = H.Model(cfg)
    idx = quiver_amd.DeviceIndex(cfg["dim"], cfg["metric"], **cfg["flags"])
    dev = {"u32": idx.column("u32"), "f64": idx.column("f64"), "sets": {}}
    searches = plain = backs = deliberate = 0
    wide = collections.Counter()
    for i, step in enumerate(steps):
        what = "seed %d step %d %s" % (seed, i, {k: v for k, v in step.items() if k in ("kind", "form", "plane", "call", "k", "deliberate", "device", "row")})
        if H.is_wide(step):
            want = search_wide(idx, dev, model, step, what)
            wide["searches"] += 1; wide["took"] += want["took"]
            if step["deliberate"]:
                wide["deliberate"] += 1
                assert all(want[key] == v for key, v in WIDE_WANT[step["deliberate"]].items()), (what, want)
            elif step["after"]["tiles"] >= 8:
                assert want["took"] == 1, (what, want)
                wide["plain"] += 1; wide["backs"] += want["back"]
            else:
                assert want["took"] == 0, (what, want)
            continue
        if step["kind"] == "search":
            back = search(idx, dev, model, step, what)
            searches += 1
            if step["deliberate"]:
                deliberate += 1
                assert back or step["after"]["tiles"] < 8, what
            elif step["after"]["tiles"] >= 8:
                plain += 1; backs += back
            continue
        mutate(idx, dev, model, step)
        if step["kind"] in ("facets", "rowset"):
            continue
        assert idx.rows() == model.n and idx.size() == int(model.alive.sum()), what
        H.check_state(read_arrays(idx, cfg), model, what)
    every = np.arange(model.n, dtype=np.uint32)
    assert np.array_equal(idx.get_rows(every).view(np.uint32), model.rows.view(np.uint32))
    assert backs * 10 <= plain, (backs, plain)                                               # the models' cap, as tests/test_bound_history_cpu.py states it
    assert wide["backs"] * 10 <= wide["plain"] and wide["took"] >= 6, dict(wide)             # ... and its twin for the wide searches
    print("seed %d (%s, %d dims, %s, %d rows): %d searches, %d predicted hand-backs beside %d deliberate ones; %d wide searches, %d took the wide form, "
          "%d predicted hand-backs beside %d deliberate cases, %.1f s"
          % (seed, cfg["metric"], cfg["dim"], cfg["style"], model.n, searches, backs, deliberate, wide["searches"], wide["took"], wide["backs"], wide["deliberate"], time.time() - t0))
    for s in dev["sets"].values():
        s.close()
    dev["u32"].close(); dev["f64"].close(); idx.close()
