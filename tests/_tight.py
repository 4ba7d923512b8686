"""Corpora on which the bound scan's margin (qv_bound.h: |q| (rres + gamma (|r| + rres))) is needed IN FULL, built and checked on the CPU.

The bfloat16 term of the margin is a Cauchy-Schwarz bound: |q.(r - rh)| <= |q||r - rh|.  On ordinary data the left side is about
1/sqrt(dim) of the right, so a residual stored several times too small still never rejects a true neighbour.  `planted` builds the
case of equality:

  q       every |q_i| equal, random signs
  r*      = h + e: h exact in bfloat16 with every |h_i| in [1, 2), e = t q with |e_i| = 2^-8 - 2^-20, just under half a bfloat16 ulp
          of h_i — so bf16(r*) = h, and q.r* exceeds stage 1's sum q.h by |q||e|, the whole of the term
  near    k - 1 rows pushed from r* towards q: clearly nearer under both metrics
  band    competitors exact in bfloat16 (rres = 0: their intervals are only gamma wide) whose exact distances lie just beyond r*'s,
          aimed by bisection along q and then CHECKED one by one with the library's interval function: each has an upper bound
          below the lower bound r* would get from a residual 10 % short
  filler  ordinary rows at a wide angle from q

so the oracle's k-th neighbour is r*, the threshold H is the best competitor's upper bound, and r* survives stage 1 only because its
margin is there.  `conditions` states (a) - (d) of that, with the oracle and the library's interval; tests/test_bound_tight_cpu.py
runs them for every parameter set, tests/test_gpu_bound_scan_tight.py before it touches the device.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

from tests import _bound as B
from tests import _oracle as O

PLANTED_DIMS = (16, 48, 128, 768)
PLANTED_KS = (1, 10, 64)
# Wider rows, as (dim, k): 240 dimensions (15 steps: every block of the kernels' step ladder in one walk) and 2048, where gamma is half
# the margin's room.  The construction ends near there: r*'s residual is 2^-8 / 1.16 of |r*|, so a residual 10 % short frees 3.4e-4 |q||r*|
# of sum, of which r*'s own gamma term takes one gamma and a competitor's upper bound, gamma above its sum, another: 2 gamma < 3.4e-4 holds
# to about 2800 dimensions (gamma is about dim x 2^-24), and with the bisection's aim, 0.15 of the way or more beyond r*, to about 2500.  At
# 4096 (gamma = 2.4e-4) `planted` finds no competitor that discriminates and says so; tests/test_bound_tight_cpu.py keeps that on record.
PLANTED_WIDE = ((240, 1), (240, 10), (240, 64), (2048, 10))
SHORT = 0.9                                       # the residual fault every planted case must catch: 10 % short


def _dist64(metric, q, rows):
    """the metric in float64 (for aiming only: every condition is checked with the oracle's float32 and the library's interval)"""
    q = q.astype(np.float64); rows = np.atleast_2d(rows).astype(np.float64)
    s = rows @ q
    return 1.0 - s if metric == B.DOT else 1.0 - s / (np.linalg.norm(q) * np.linalg.norm(rows, axis=1))


def _row_interval(metric, q, r, scale=1.0):
    """(d_lo, d_hi) of one row with its residual multiplied by `scale`"""
    st = B.RowState(r[None, :])
    un, lo, hi = B.intervals(metric, q.size, B.chain32_rows(q, st.rh), B.chain_norm(q), st.rn, (st.rres.astype(np.float64) * scale).astype(np.float32))
    assert not un[0]
    return lo[0], hi[0]


@functools.lru_cache(maxsize=None)
def planted(metric, dim, k, seed=0):
    """-> dict(rows [n, dim], q [dim], target, near [k-1], band [...], ordinary: a filler row's index)"""
    rng = np.random.default_rng(1000 * dim + 10 * k + metric + 7919 * seed)
    n = 4000 + 37 * ((dim + 3 * k) % 97) + 11                             # 4 000 - 8 000 rows
    n += n % 64 == 0                                                       # a ragged last tile
    sig = np.where(rng.random(dim) < 0.5, -1.0, 1.0)
    q = (sig * np.float32(0.9 / np.sqrt(dim))).astype(np.float32)
    side = np.where(rng.random(dim) < 0.75, sig, -sig)                     # three elements of four on q's side: cos(q, h) about 0.5
    h = (side * (1.0 + rng.integers(1, 41, dim) / 128.0)).astype(np.float32)
    e = (sig * (2.0 ** -8 - 2.0 ** -20)).astype(np.float32)
    target_row = (h.astype(np.float64) + e.astype(np.float64)).astype(np.float32)
    assert np.array_equal(target_row.astype(np.float64), h.astype(np.float64) + e.astype(np.float64))      # h + e is a float32
    assert np.array_equal(B.bf16(target_row).view(np.uint32), h.view(np.uint32)) and np.array_equal(B.bf16(h).view(np.uint32), h.view(np.uint32))
    qe = float(q.astype(np.float64) @ e.astype(np.float64))
    assert abs(qe - np.linalg.norm(q.astype(np.float64)) * np.linalg.norm(e.astype(np.float64))) <= 1e-12 * qe   # Cauchy-Schwarz is an equality

    d_star = float(O.distance(metric, q, target_row))
    lo_short, _ = _row_interval(metric, q, target_row, SHORT)
    assert float(lo_short) > d_star, (metric, dim, "a residual 10 % short leaves no room between r* and its lower bound", d_star, float(lo_short))

    # the band: exact in bfloat16, aimed at a third of the way from r*'s distance to that lower bound, kept when the library agrees
    m = 600
    g = target_row.astype(np.float64) * (1.0 + 0.01 * rng.standard_normal((m, 1))) + 0.02 * rng.standard_normal((m, dim))
    qd = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64)) * np.linalg.norm(target_row.astype(np.float64))
    aim = d_star + (float(lo_short) - d_star) * rng.uniform(0.15, 0.45, m)
    a_lo, a_hi = np.full(m, -2.0), np.full(m, 2.0)                         # the distance falls as a row moves along q
    for _ in range(60):
        mid = 0.5 * (a_lo + a_hi)
        far = _dist64(metric, q, g + mid[:, None] * qd) > aim
        a_lo = np.where(far, mid, a_lo); a_hi = np.where(far, a_hi, mid)
    cand = B.bf16((g + a_hi[:, None] * qd).astype(np.float32))
    st = B.RowState(cand)
    assert not st.rres.any()
    un, lo, hi = B.intervals(metric, dim, B.chain32_rows(q, st.rh), B.chain_norm(q), st.rn, st.rres)
    d = O.all_distances(metric, cand, q)
    s_target = B.chain32(q, h)
    good = ~un & (d > np.float32(d_star)) & (hi < lo_short) & (B.chain32_rows(q, st.rh) > s_target)
    band = cand[good][:24]
    assert len(band) >= 8, (metric, dim, k, "competitors that discriminate", int(good.sum()))

    near = (target_row.astype(np.float64) + rng.uniform(0.3, 1.0, (k - 1, 1)) * qd + 0.01 * rng.standard_normal((k - 1, dim))).astype(np.float32)

    rows = (rng.standard_normal((n, dim)) * rng.uniform(0.5, 1.5, (n, 1)) * np.linalg.norm(target_row) / np.sqrt(dim)).astype(np.float32)
    cos = (rows.astype(np.float64) @ q.astype(np.float64)) / (np.linalg.norm(rows.astype(np.float64), axis=1) * np.linalg.norm(q.astype(np.float64)))
    rows[cos > 0.15] *= np.float32(-1.0)                                   # filler: at a wide angle from q (r* is at about 60 degrees)
    place = rng.permutation(n - 200) + 100                                 # scattered over the tiles, clear of both ends
    place = np.concatenate([place[place % 64 >= 8][:1], place[place % 64 < 8]])[:1 + len(near) + len(band) + 1]   # (r* well inside its tile)
    target, near_at, band_at, ordinary = int(place[0]), place[1:1 + len(near)], place[1 + len(near):-1], int(place[-1])
    rows[target] = target_row; rows[near_at] = near; rows[band_at] = band
    rows.setflags(write=False); q.setflags(write=False)
    return {"rows": rows, "q": q, "target": target, "near": near_at, "band": band_at, "ordinary": ordinary, "k": k, "metric": metric}


def conditions(case, alive=None, cap=B.CAND_CAP):
    """(a) - (d) of the planted case on the CPU; -> (the oracle's rows, its float32 distances, the reference's survivor count).  cap: the
    candidate list (d) is taken against — the k <= 64 forms' unless the caller names the wide form's"""
    metric, rows, q, k, t = case["metric"], case["rows"], case["q"], case["k"], case["target"]
    st = B.RowState(rows)
    er, ed = B.oracle_top(metric, rows, q, k, alive)
    assert t in er.tolist() and er[k - 1] == t, ("(a) r* is the oracle's k-th neighbour", er)
    ref = B.reference(metric, st, q, k, alive, cap=cap)
    assert ref["H"] is not None and not ref["unsure"][t]
    assert ref["H"] == ref["hi"][case["band"]].min(), "H comes from the best competitor"
    assert ref["lo"][t] <= ref["H"], ("(b) r* survives with the residual the reference computes", ref["lo"][t], ref["H"])
    short = st.rres.copy(); short[t] = np.float32(float(st.rres[t]) * SHORT)
    bad = B.reference(metric, st, q, k, alive, rres=short, cap=cap)
    assert bad["H"] == ref["H"] and bad["lo"][t] > bad["H"], ("(c) a residual 10 % short rejects r*", bad["lo"][t], bad["H"])
    assert k <= ref["count"] <= cap and not ref["hand_back"], ("(d) the survivors fit the candidate list", ref["count"])
    return er, ed, ref["count"]


# ---- the worst of bfloat16 rounding, in a cluster around the queries ----------------------------------------------------------------

def halfway(x):
    """every element exactly half way between two bfloat16 values (the largest residual round-to-nearest leaves)"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((b & np.uint32(0xFFFF0000)) | np.uint32(0x8000)).view(np.float32)


def of_kind(x, kind, rng):
    """`x` [.., dim] as a vector of one kind: 0 half-way, 1 exact in bfloat16, 2 scaled by 1e-3, 3 ordinary, 4 ordinary with denormal elements"""
    x = np.ascontiguousarray(x, np.float32).copy()
    if kind == 0:
        return halfway(x)
    if kind == 1:
        return B.bf16(x)
    if kind == 2:
        return (x * np.float32(1e-3)).astype(np.float32)
    if kind == 4:
        x[..., rng.permutation(x.shape[-1])[:3]] = np.float32(1e-40)
    return x


@functools.lru_cache(maxsize=None)
def worst_rounding(dim):
    """-> (rows [20 011, dim], queries [8, dim]): a cluster of relative width 0.5 around one centre; rows half-way, exact, scaled by 1e-3
    and ordinary in turn, every 50th with denormal elements, one whole-denormal row; queries of each kind, the last one whole-denormal
    (its norm is below filter_tiny_norm: the one hand-back the reference predicts)"""
    rng = np.random.default_rng(77 + dim)
    n = 20_011
    z = rng.standard_normal(dim) / np.sqrt(dim)
    rows = (z + 0.5 * rng.standard_normal((n, dim)) / np.sqrt(dim)).astype(np.float32)
    for kind in range(3):
        rows[kind::4] = of_kind(rows[kind::4], kind, rng)
    rows[25::50] = of_kind(rows[25::50], 4, rng)
    rows[n // 2] = (rows[n // 2].astype(np.float64) * 1e-38).astype(np.float32)
    qs = (z + 0.5 * rng.standard_normal((8, dim)) / np.sqrt(dim)).astype(np.float32)
    for j, kind in enumerate((3, 0, 1, 2, 4, 0, 3)):
        qs[j] = of_kind(qs[j], kind, rng)
    qs[7] = (qs[7].astype(np.float64) * 1e-38).astype(np.float32)
    rows.setflags(write=False); qs.setflags(write=False)
    return rows, qs


@functools.lru_cache(maxsize=None)
def _worst_stage1(metric, dim):
    rows, qs = worst_rounding(dim)
    st = B.RowState(rows)
    return [B.stage1(metric, st, q) for q in qs]


def worst_rounding_reference(metric, dim, k):
    """per query: (the reference's survivor count, whether it predicts a hand-back)"""
    return [(r["count"], r["hand_back"]) for r in (B.decide(s1, k) for s1 in _worst_stage1(metric, dim))]
