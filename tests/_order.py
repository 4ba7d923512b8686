"""Order-sensitive vectors and summation-order models — TEST INFRASTRUCTURE ONLY (numpy, CPU).

The reference adds a row's terms as ONE chain in element order and rounds once (pkg/vectortypes/distances.go:18-22; the float32
chains of adapter.go:111-165).  On random data a different order moves the float64 sum by ~1e-13 relative, far below a float32
step, so a kernel that sums in another order returns the same bits almost everywhere.  The rows built here are the exception by
construction: the reference's chain gives one float32, and every wrong order listed in ORDERS gives another for at least one of
them.

Constructions (every input a float32; where the metric subtracts, r - q is exact in float32 and checked):
  * terms >= 0 (Euclidean, Manhattan, squared Euclidean): a HEAD whose exact sum sits one grid step below the value where the
    float32 result flips, its largest term first; then a TAIL of terms each below half an ulp of that sum, which the chain
    absorbs one by one and every other order adds up (family "tail").  Or small PRE terms in the big term's own 4-element
    chunk, before it: the chain adds them up before the big term and crosses the flip; a chunk read backwards absorbs them
    (family "pre").
  * dot: +T early, terms below half an ulp of T in the middle, -T late, a visible term last (the chain keeps only what follows
    the cancellation); or the chunk pattern [p, +T, -T, p'] (forward gives p', the chunk reversed gives p).
  * cosine: rows nearly parallel to the query (distances ~1e-14 .. 1e-8, where one ulp of the float64 similarity is a float32
    step), kept when the models say the order matters.
Rows are kept only where some model gives other bits than the chain; which models, ORDERS and `sensitive` say.

Order models (`model_distance`): reverse, each 4-element chunk reversed, pairwise tree, the exact sum rounded once, the HNSW
latency form's split (8 waves x 2 / 4 / 8 lanes, `split_sum`), and the split scan's layout (8 waves on contiguous columns, one
lane per row, partials added in wave order by the consumer; for cosine with the query's norm as a workgroup sum)."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from oracle import oracle_np as ONP
from tests import _oracle as O

COSINE, L2, L2SQ, DOT, L1, COSINE_F32, L2_F32, DOT_F32, L2SQ_F64 = range(9)
F64_METRICS = (COSINE, L2, DOT, L1, L2SQ_F64)          # the float64 chains: every exact path, split forms included
F32_METRICS = (L2SQ, COSINE_F32, L2_F32, DOT_F32)      # the float32 chains (pkg/hnsw adapter)
SPLIT_METRICS = F64_METRICS                            # SplitOK / ScanSplitOK (qv_hnsw.hip, qv_scan.hip)

U = 2.0 ** -53
SLACK = 128.0                                          # kSplitSlack
SPLIT_WAVES = 8                                        # kSplitWaves; the latency form's waves (QV_HNSW_LAT_WAVES)
SCAN_BLOCK = 64 * SPLIT_WAVES                          # kSplitBlock: the threads that sum the query's norm in the split scan

ORDERS = ("reverse", "chunk_reversed", "pairwise", "exact", "lat2", "lat4", "lat8", "scan_split")
SPLIT_ORDERS = ("lat2", "lat4", "lat8", "scan_split")


# ------------------------------------------------------------------------------------------------------ summation orders --
def seq_sum(p, dtype=np.float64):
    """one chain, element order: cumsum adds left to right, one rounding per step"""
    p = np.asarray(p, dtype=dtype)
    return dtype(np.cumsum(p, dtype=dtype)[-1]) if len(p) else dtype(0)


def split_sum(p, waves, lanes_per_row):
    """the latency form's order: wave w owns a contiguous run of 16-byte chunks (4 elements each), its lanes split the run,
    every lane runs a chain, lanes are added pairwise (butterfly), waves in order"""
    n4 = len(p) // 4
    n_p = n4 // 8                                        # pieces of 8 chunks
    tot = None
    for w in range(waves):
        p_lo, p_hi = w * n_p // waves, (w + 1) * n_p // waves
        c0, n = p_lo * 8, (p_hi - p_lo) * 8
        parts = []
        for sub in range(lanes_per_row):
            lo, hi = c0 + sub * n // lanes_per_row, c0 + (sub + 1) * n // lanes_per_row
            parts.append(float(seq_sum(p[4 * lo:4 * hi])))
        while len(parts) > 1:                             # xor-butterfly: (a + b), then pairs of pairs
            half = len(parts) // 2
            parts = [parts[i] + parts[i + half] for i in range(half)]
        tot = parts[0] if tot is None else tot + parts[0]
    return tot


def scan_split_sum(p):
    """k_flat_scan_split: wave w walks chunks [w dim4 / 8, (w + 1) dim4 / 8) as one chain; the consumer adds the eight partials
    in wave order"""
    n4 = len(p) // 4
    tot = 0.0
    for w in range(SPLIT_WAVES):
        lo, hi = w * n4 // SPLIT_WAVES, (w + 1) * n4 // SPLIT_WAVES
        part = float(seq_sum(p[4 * lo:4 * hi])) if hi > lo else 0.0
        tot = part if w == 0 else tot + part
    return tot


def workgroup_sum(p):
    """the split scan's |q|^2 (qv_scan.hip): thread t chains elements t, t + 512, ...; each wave's 64 lanes are added by an
    xor-butterfly (offsets 32 .. 1); the eight waves' sums are added in order"""
    p = np.asarray(p, np.float64)
    lanes = np.zeros(SCAN_BLOCK)
    for t in range(SCAN_BLOCK):
        s = 0.0
        for x in p[t::SCAN_BLOCK]:
            s = s + float(x)
        lanes[t] = s
    waves = []
    for w in range(SPLIT_WAVES):
        v = lanes[64 * w:64 * (w + 1)].copy()
        off = 32
        while off:
            v = v + v[np.arange(64) ^ off]               # every lane: own + partner, the same rounding on both sides
            off >>= 1
        waves.append(float(v[0]))
    tot = waves[0]
    for w in waves[1:]:
        tot = tot + w
    return tot


def pairwise_sum(p, dtype=np.float64):
    p = [dtype(x) for x in np.asarray(p, dtype=dtype)]
    if not p:
        return dtype(0)
    while len(p) > 1:                                     # adjacent pairs, level by level (an odd one is carried up)
        nxt = [dtype(p[i] + p[i + 1]) for i in range(0, len(p) - 1, 2)]
        if len(p) % 2:
            nxt.append(p[-1])
        p = nxt
    return p[0]


def exact_sum(p, dtype=np.float64):
    """the exact sum of the (exactly representable) terms, rounded once"""
    s = sum((Fraction(float(x)) for x in np.asarray(p, np.float64)), Fraction(0))
    return dtype(float(s)) if dtype == np.float64 else np.float32(float(s))     # (float32: Fraction -> f64 -> f32 is a double
                                                                                #  rounding; exact here: the sums have <= 53 bits)


def order_sum(order, p, dtype=np.float64):
    p = np.asarray(p, dtype=dtype)
    if order == "chain":
        return seq_sum(p, dtype)
    if order == "reverse":
        return seq_sum(p[::-1], dtype)
    if order == "chunk_reversed":
        n = len(p)
        q = np.concatenate([p, np.zeros((-n) % 4, dtype)]).reshape(-1, 4)[:, ::-1].reshape(-1)
        return seq_sum(q, dtype)
    if order == "pairwise":
        return pairwise_sum(p, dtype)
    if order == "exact":
        return exact_sum(p, dtype)
    if order in ("lat2", "lat4", "lat8"):
        return split_sum(_pad4(p), SPLIT_WAVES, int(order[3:]))
    if order == "scan_split":
        return scan_split_sum(_pad4(p))
    raise ValueError(order)


def _pad4(p):
    return np.concatenate([np.asarray(p, np.float64), np.zeros((-len(p)) % 4)])


# ---------------------------------------------------------------------------------------------- terms and finalisation --
def terms(metric, q, r):
    """the per-element terms the reference adds, exactly as it forms them (float32 inputs), and the accumulator's type"""
    q32, r32 = np.asarray(q, np.float32), np.asarray(r, np.float32)
    q64, r64 = q32.astype(np.float64), r32.astype(np.float64)
    if metric in (COSINE, DOT):
        return q64 * r64, np.float64
    if metric == L2:
        d = (q32 - r32).astype(np.float64)
        return d * d, np.float64
    if metric == L1:
        return np.abs((q32 - r32).astype(np.float64)), np.float64
    if metric == L2SQ_F64:
        d = q64 - r64
        return d * d, np.float64
    if metric in (L2SQ, L2_F32):
        d = q32 - r32
        return d * d, np.float32
    return q32 * r32, np.float32                          # COSINE_F32, DOT_F32


def _norm_parts(metric, q, r):
    q32, r32 = np.asarray(q, np.float32), np.asarray(r, np.float32)
    if metric == COSINE:
        q64, r64 = q32.astype(np.float64), r32.astype(np.float64)
        return seq_sum(q64 * q64), seq_sum(r64 * r64)
    return seq_sum(q32 * q32, np.float32), seq_sum(r32 * r32, np.float32)


def finalize(metric, acc, ma=None, mb=None):
    """distance from the accumulated sum (and, for cosine, the two squared norms as the reference forms them)"""
    with np.errstate(all="ignore"):
        if metric == COSINE:
            if ma == 0 or mb == 0:
                return np.float32(1.0)
            sim = float(acc) / (math.sqrt(ma) * math.sqrt(mb))
            sim = min(1.0, max(-1.0, sim))
            return np.float32(1.0 - sim)
        if metric == L2:
            return np.float32(math.sqrt(acc)) if acc >= 0 else np.float32(np.nan)
        if metric == DOT:
            return np.float32(1.0 - float(acc))
        if metric in (L1, L2SQ_F64):
            return np.float32(acc)
        if metric == L2SQ:
            return np.float32(acc)
        if metric == L2_F32:
            return np.float32(math.sqrt(float(acc)))
        if metric == COSINE_F32:
            if ma == 0 or mb == 0:
                return np.float32(1.0)
            den = np.float32(np.float32(math.sqrt(float(ma))) * np.float32(math.sqrt(float(mb))))
            sim = np.float32(np.float32(acc) / den)
            sim = min(np.float32(1.0), max(np.float32(-1.0), sim))
            return np.float32(np.float32(1.0) - sim)
        return np.float32(np.float32(1.0) - np.float32(acc))   # DOT_F32


def model_distance(metric, q, r, order):
    """the float32 distance when the row's terms are added in `order` ("chain" is the reference's)"""
    p, dt = terms(metric, q, r)
    if order in SPLIT_ORDERS and dt != np.float64:
        raise ValueError("the split forms exist for the float64 metrics only")
    acc = order_sum(order, p, dt)
    ma = mb = None
    if metric in (COSINE, COSINE_F32):
        ma, mb = _norm_parts(metric, q, r)
        if metric == COSINE and order == "scan_split":
            qq = np.asarray(q, np.float32).astype(np.float64)
            ma = workgroup_sum(qq * qq)                    # the query's norm as the split scan sums it
    return finalize(metric, acc, ma, mb)


def certificate(metric, q, r, order):
    """(finalize(S - B), finalize(S + B)) for the split form `order`, with the kernels' bound: B = (2 dim + 128) u (|q| |r| for
    cosine / dot, else S); the split scan widens cosine's interval by (|S| + B) 2 k_u for its workgroup-sum query norm
    (qv_scan.hip k_flat_scan_split, qv_hnsw.hip split_bound)"""
    p, _ = terms(metric, q, r)
    dim4 = (len(p) + 3) // 4
    k_u = (2.0 * (4 * dim4) + SLACK) * U
    s = order_sum(order, p)
    qq = np.asarray(q, np.float32).astype(np.float64)
    rr = np.asarray(r, np.float32).astype(np.float64)
    ma, mb = float(seq_sum(qq * qq)), float(seq_sum(rr * rr))
    if metric == COSINE and order == "scan_split":
        ma = workgroup_sum(qq * qq)
    if metric in (COSINE, DOT):
        b = k_u * math.sqrt(ma) * math.sqrt(mb)
    else:
        b = k_u * s
    if metric == COSINE and order == "scan_split":
        b = b + (abs(s) + b) * (2.0 * k_u)
    return finalize(metric, s - b, ma, mb), finalize(metric, s + b, ma, mb), s, b


def bits(x):
    return np.float32(x).view(np.uint32)


def orders_for(metric, dim):
    """the wrong orders modelled for this metric and dimension: the split forms only for the float64 metrics, the latency
    form's (split_sum: whole pieces of 8 chunks) only where the dimension is a multiple of 32"""
    if metric not in F64_METRICS:
        return tuple(o for o in ORDERS if o not in SPLIT_ORDERS)
    return tuple(o for o in ORDERS if dim % 32 == 0 or not o.startswith("lat"))


def sensitive(metric, q, r):
    """the wrong orders whose float32 differs from the chain's for this pair"""
    ref = bits(model_distance(metric, q, r, "chain"))
    return {o for o in orders_for(metric, len(q)) if bits(model_distance(metric, q, r, o)) != ref}


# ---------------------------------------------------------------------------------------------------------- generators --
def _ulp(x, dtype):
    x = dtype(abs(x))
    return float(np.nextafter(x, dtype(np.inf)) - x)


def _flip_point(metric, y0, dtype):
    """the smallest accumulator value (of the accumulator's type) whose distance is not y0, for the metrics whose distance
    increases with a sum of non-negative terms"""
    fin = lambda s: finalize(metric, s)
    y_next = np.nextafter(np.float32(y0), np.float32(np.inf))
    mid = (float(y0) + float(y_next)) / 2
    guess = dtype(mid * mid if metric in (L2, L2_F32) else mid)
    s = guess
    while bits(fin(s)) != bits(y0):                       # walk down into y0's range, then up to its end
        s = np.nextafter(s, dtype(0))
    while bits(fin(np.nextafter(s, dtype(np.inf)))) == bits(y0):
        s = np.nextafter(s, dtype(np.inf))
    return np.nextafter(s, dtype(np.inf))


def _decompose(R, grid, square, max_bits):
    """float32 values d (multiples of sqrt(grid) / grid, at most max_bits significant bits) whose terms d^2 / |d| add up
    EXACTLY to R, a multiple of the grid; largest first"""
    out = []
    h = math.sqrt(grid) if square else grid
    while R > 0:
        d = math.floor((math.sqrt(R) if square else R) / h) * h
        m, e = math.frexp(d)
        d = math.ldexp(math.floor(m * 2 ** max_bits) / 2 ** max_bits, e)
        d = max(d, h)
        t = d * d if square else d
        assert t <= R and np.float32(d) == d
        out.append(d)
        R -= t
    return out


def _bits12(x):
    """x truncated to 12 significant bits: a small integer of the query's plus this value is still a float32"""
    m, e = math.frexp(x)
    return math.ldexp(math.floor(m * 4096) / 4096, e)


def _nonneg_delta(metric, dim, rng, family, p0, scale_exp, end):
    """r - q for the metrics whose terms are >= 0, nonzero before column `end` only; None when this draw does not fit"""
    dt = np.float64 if metric in (L2, L1, L2SQ_F64) else np.float32
    square = metric != L1
    f32_terms = dt == np.float32
    big = 2.0 ** (24 if not f32_terms else 10)            # the head's first term: 2^48 / 2^24 (f64) or 2^20 / 2^10 (f32)
    t_big = big * big if square else big
    y0 = finalize(metric, dt(t_big * (1.0 + 2.0 ** -8 * rng.integers(1, 200))))
    flip = float(_flip_point(metric, y0, dt))
    g = _ulp(flip, dt)
    grid = g if not square else (g if math.log2(g) % 2 == 0 else 2 * g)
    head_sum = math.floor((flip - g) / grid) * grid       # one grid step (or two) below the flip: exact on the grid
    if finalize(metric, dt(head_sum)) != y0 or head_sum < t_big:
        return None
    max_bits = 12 if (square and f32_terms) else 24       # float32 squares must be exact
    rest = _decompose(head_sum - t_big, grid, square, max_bits)
    head = [big] + rest
    half = _ulp(head_sum, dt) / 2                         # a tail term below this is absorbed by the chain
    tail_t = half * rng.uniform(0.5, 0.95)
    tail_d = _bits12(math.sqrt(tail_t) if square else tail_t)
    if (tail_d * tail_d if square else tail_d) >= half:
        return None
    delta = np.zeros(dim, np.float64)
    if family == "tail":
        if p0 + len(head) >= end:
            return None
        delta[p0:p0 + len(head)] = head
        n_tail = int(rng.integers((end - p0 - len(head)) // 2, end - p0 - len(head) + 1))
        delta[p0 + len(head):p0 + len(head) + n_tail] = tail_d
    else:                                                 # "pre": tail-sized terms before the big one in its own chunk
        p0 = (p0 // 4) * 4 + 3
        if p0 + len(head) >= end:
            return None
        delta[p0 - 3:p0] = _bits12(math.sqrt(half * 0.9) if square else half * 0.9)
        delta[p0:p0 + len(head)] = head
    signs = rng.choice([-1.0, 1.0], size=dim)
    return (delta * signs * 2.0 ** scale_exp).astype(np.float32)


def _dot_row(metric, dim, q, rng, family):
    """a row r for query q (entries +-2^e) whose products p = q r follow the dot constructions; None when it does not fit"""
    f32 = metric == DOT_F32
    T = 2.0 ** (30 if not f32 else 8)
    half = (2.0 ** -22 if not f32 else 2.0 ** -15) / 2 * 0.9   # below half an ulp of T
    p = np.zeros(dim, np.float64)
    if family == "tail":
        i_plus = int(rng.integers(0, max(dim // 8, 1)))
        i_minus = int(rng.integers(dim - dim // 8 - 2, dim - 1))
        p[i_plus] = T
        mid = rng.uniform(0.3, 1.0, size=i_minus - i_plus - 1) * half
        p[i_plus + 1:i_minus] = mid * rng.choice([1.0, 1.0, 1.0, -1.0], size=mid.size)
        p[i_minus] = -T
        p[i_minus + 1:] = rng.uniform(1e-3, 1e-2, size=dim - i_minus - 1)
    else:                                                 # [p, +T, -T, p'] in one chunk
        c = int(rng.integers(0, dim // 4)) * 4
        p[c:c + 4] = [half * 0.7, T, -T, half * 0.1]
        p[c + 4:] = 0.0
        p[:c] = 0.0
    p = p.astype(np.float32).astype(np.float64)
    r = (p / q.astype(np.float64)).astype(np.float32)
    if not np.array_equal(r.astype(np.float64) * q.astype(np.float64), p):
        return None
    return r


def dot_query(dim, rng):
    return (rng.choice([-1.0, 1.0], size=dim) * np.exp2(rng.integers(-3, 4, size=dim))).astype(np.float32)


def cosine_rows(q, n, rng):
    """rows nearly parallel to q: relative perturbations 1e-7 .. 1e-4 (distances ~1e-14 .. 1e-8)"""
    out = []
    for _ in range(n):
        eps = 10.0 ** rng.uniform(-7, -4)
        r = (q.astype(np.float64) * (1.0 + eps * rng.standard_normal(q.size))).astype(np.float32)
        out.append(r)
    return out


def planted_rows(metric, dim, q, n_try, rng, max_scale=6):
    """candidate rows for query q, kept when at least one wrong order gives other float32 bits than the chain; the
    difference metrics' rows are scaled by 2^s, s <= max_scale"""
    q = np.asarray(q, np.float32)
    rows = []
    for t in range(n_try):
        if metric in (COSINE, COSINE_F32):
            r = cosine_rows(q, 1, rng)[0]
        elif metric in (DOT, DOT_F32):
            r = _dot_row(metric, dim, q, rng, "tail" if t % 3 else "chunk")
        else:
            family = "pre" if t % 4 == 3 else "tail"
            p0 = int(rng.choice([0, 1, 2, 5, 8 * int(rng.integers(0, max(dim // 32, 1)))]))
            scale = int(rng.integers(-6, max_scale + 1)) if metric not in (L2SQ, L2_F32) else int(rng.integers(-3, min(max_scale, 3) + 1))
            # (Manhattan's tail terms are ~2^-53 of the sum: they stay where the query is zero, or q + r would round)
            end = int(np.nonzero(q)[0][0]) if metric == L1 and np.any(q) else dim - 1
            delta = _nonneg_delta(metric, dim, rng, family, min(p0, dim - 16), scale, end)
            if delta is None:
                r = None
            else:
                r = (q.astype(np.float64) + delta.astype(np.float64)).astype(np.float32)
                if not np.array_equal((r.astype(np.float64) - q.astype(np.float64)), delta.astype(np.float64)):
                    r = None                              # r - q must be exact
                elif not np.array_equal(q - r, -delta):
                    r = None
        if r is None:
            continue
        if sensitive(metric, q, r):
            rows.append(r)
    return rows


def query_for(metric, dim, rng):
    """a query the constructions can be planted around: small integers (differences), +-2^e (products), normals (cosine)"""
    if metric in (DOT, DOT_F32):
        return dot_query(dim, rng)
    if metric in (COSINE, COSINE_F32):
        return rng.standard_normal(dim).astype(np.float32)
    q = np.zeros(dim, np.float32)                         # (nonzero only past every head: the heads' terms use all 24 bits)
    lo = min(dim // 2 + 16, dim - 1)
    q[lo:dim - 1] = rng.integers(-4, 5, size=dim - 1 - lo)
    return q


def oracle_chain(metric, q, r):
    """the numpy restatement of the reference (oracle/oracle_np.py), for cross-checking the models' "chain" """
    return ONP.distance(metric, q, r)


# ------------------------------------------------------------------------------------------- corpora of planted rows --
DIFF = (L2, L2SQ, L1, L2_F32, L2SQ_F64)
SEP = 2.0 ** 28                  # the queries of a difference metric sit SEP apart in the last column (every planted delta is
                                 # below 2^25 there); fillers sit 2^30 away from all of them


def _case(metric, dim, nq, seed, n_fill, dup=0):
    """-> (queries [nq, dim], corpus [n, dim], planted ids per query).  Difference metrics: each query gets its own copy of the
    planted rows (shifted with it in the last column, where planted deltas are 0).  Dot / cosine: the queries are one query
    scaled by powers of two (every product, and the chain, scales exactly), all sharing the planted rows."""
    rng = np.random.default_rng(seed)
    q = query_for(metric, dim, rng)
    planted = planted_rows(metric, dim, q, 40, rng, max_scale=0)
    assert len(planted) >= 8, (metric, dim, len(planted))
    planted = np.array(planted, np.float32)
    if dup:
        planted = np.concatenate([planted, planted[:dup]])            # equal distances: the heaps' tie rules
    qs, rows, own = [], [], []
    for j in range(nq):
        if metric in DIFF:
            qj = q.copy(); qj[-1] = j * SEP
            pj = planted.copy(); pj[:, -1] = j * SEP
            own.append(np.arange(j * len(planted), (j + 1) * len(planted)))
            rows.append(pj)
        else:
            qj = (q * np.float32(2.0 ** (j % 3 - 1))).astype(np.float32)
            if j == 0:
                rows.append(planted)
            own.append(np.arange(len(planted)))
        qs.append(qj)
    if metric in DIFF:
        fill = (rng.standard_normal((n_fill, dim)) * 2.0 ** 20).astype(np.float32)
        fill[:, -1] = -(2.0 ** 30)
    elif metric in (DOT, DOT_F32):
        fill = (-np.sign(q) * rng.uniform(0.5, 2.0, size=(n_fill, dim))).astype(np.float32)      # every dot with a query < 0
    else:
        fill = (-q * (1.0 + 0.3 * rng.standard_normal((n_fill, dim)))).astype(np.float32)        # anti-parallel: distance ~2
    corpus = np.concatenate(rows + [fill])
    perm = rng.permutation(corpus.shape[0])                           # planted rows spread over tiles and workgroups
    inv = np.empty_like(perm); inv[perm] = np.arange(perm.size)
    corpus = np.ascontiguousarray(corpus[perm])
    own = [np.sort(inv[o]) for o in own]
    qs = np.ascontiguousarray(np.stack(qs))
    for j in range(nq):                                               # the planted rows ARE the nearest, and order-sensitive
        d = O.all_distances(metric, corpus, qs[j])
        mask = np.ones(corpus.shape[0], bool); mask[own[j]] = False
        assert d[own[j]].max() < d[mask].min(), (metric, dim, j)
    return qs, corpus, own
