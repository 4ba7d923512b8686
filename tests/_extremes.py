"""Non-finite and extreme-magnitude vectors for the edge tests (tests/test_oracle_extremes.py, tests/test_gpu_extremes.py).

Value classes (the letters are the ones the tests and DESIGN.md §2 use):
  N  NaN elements, made from bit patterns (quiet, negative quiet, and two payload patterns), never by arithmetic
  I  a single +Inf or -Inf element; a vector holding both
  O  finite elements from 1e19 up to 3.4e38: the float32 metrics overflow, the float64 ones stay finite
  G  scaled copies of an ordinary vector whose norm sits on either side of the filters' 1e18 guard
  Z  zero vectors and all -0.0 vectors
  D  denormal vectors
TEST INFRASTRUCTURE ONLY."""
import numpy as np

from tests import _oracle as O

NAN_BITS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001)
NANS = np.array(NAN_BITS, dtype=np.uint32).view(np.float32)
G_NORMS = (0.5e18, 0.999e18, 1.001e18, 2e18, 1e30)
CLASSES = "NIOGZD"


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same(got, want):
    """float32 arrays equal bit for bit where `want` is not NaN, and NaN where it is"""
    got = np.asarray(got, np.float32); want = np.asarray(want, np.float32)
    if got.shape != want.shape:
        return False
    nw = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nw) and np.array_equal(bits(got[~nw]), bits(want[~nw])))


def unit(rng, dim):
    v = rng.standard_normal(dim)
    return (v / np.linalg.norm(v)).astype(np.float32)


def scaled(v, norm):
    """v (unit length) scaled in float64 so that its norm is `norm`"""
    return (v.astype(np.float64) * norm).astype(np.float32)


def variants(cls, rng, base):
    """the vectors of class `cls` derived from the ordinary vector `base` (float32 [dim]); a list of (name, vector)"""
    dim = base.size
    out = []
    if cls == "N":
        for j, nan in enumerate(NANS):
            v = base.copy(); v[(j * 7) % dim] = nan
            out.append((f"nan{j}", v))
        out.append(("nan_row", np.full(dim, NANS[0], np.float32)))
    elif cls == "I":
        v = base.copy(); v[0] = np.inf; out.append(("pinf", v))
        v = base.copy(); v[dim - 1] = -np.inf; out.append(("ninf", v))
        if dim >= 2:
            v = base.copy(); v[0] = np.inf; v[-1] = -np.inf
            out.append(("pinf_ninf", v))
    elif cls == "O":
        mags = np.exp(rng.uniform(np.log(1e19), np.log(3.4e38), dim))
        sgn = np.where(rng.random(dim) < 0.5, -1.0, 1.0)
        out.append(("huge", (sgn * mags).astype(np.float32)))
        out.append(("huge_neg", (-sgn * mags).astype(np.float32)))                 # a - b overflows against "huge"
        out.append(("max", np.where(sgn > 0, np.float32(3.4e38), np.float32(-3.4e38)).astype(np.float32)))
    elif cls == "G":
        u = base / np.float32(np.linalg.norm(base.astype(np.float64))) if np.any(base) else base
        for g in G_NORMS:
            out.append((f"norm{g:g}", scaled(u, g)))
    elif cls == "Z":
        out.append(("zero", np.zeros(dim, np.float32)))
        out.append(("negzero", np.full(dim, -0.0, np.float32)))
    elif cls == "D":
        out.append(("denorm", scaled(base, 1e-39)))
        out.append(("denorm_min", (np.sign(base) * np.float32(1.4e-45)).astype(np.float32)))
    else:
        raise ValueError(cls)
    return out


def class_rows(rng, dim, per_class=1):
    """[(class, name, vector)] over every class, per_class ordinary bases each"""
    out = []
    for cls in CLASSES:
        for _ in range(per_class):
            for name, v in variants(cls, rng, unit(rng, dim)):
                out.append((cls, name, v))
    return out


# corpora and queries of the search tests: ordinary generator rows with extreme rows written in
def _corpus(seed, n, dim, regime, q_ord):
    """rows [n, dim] with extreme rows written in; `q_ord` (ordinary queries) get scaled copies of themselves at G norms"""
    rng = np.random.default_rng(seed)
    rows = O.gen_rows(seed, 0, n, dim)
    ext = [v for _, _, v in class_rows(rng, dim, per_class=2)]
    for i, q in enumerate(q_ord[:2]):                                   # the query's own direction, scaled across the guard
        ext += [scaled(q / np.float32(np.linalg.norm(q)), g) for g in G_NORMS]
    pos = rng.choice(n, size=len(ext), replace=False)
    pos[:3] = [0, n - 1, n // 2]                                        # first / last row / a middle tile boundary
    for p, v in zip(pos, ext):
        rows[p] = v
    if regime == "many":
        # ~20 % of the rows, in thirds: whole-NaN rows (NaN under every metric); rows with one +inf element (+inf under the L1 / L2
        # metrics, float32 and float64; NaN under cosine; -inf or +inf under dot, by the sign of the query's element); rows holding
        # +3e38 and -3e38 (+inf under the float32 metrics, finite and far under the float64 ones).  Cosine never gives +inf.
        bad = rng.choice(n, size=n // 5, replace=False)
        a, b = bad.size // 3, 2 * bad.size // 3
        rows[bad[:a]] = NANS[rng.integers(0, 4, size=a)][:, None]
        rows[bad[a:b], 0] = np.inf
        rows[bad[b:], 0] = np.float32(3.0e38)
        rows[bad[b:], -1] = np.float32(-3.0e38)
    return rows


def _queries(seed, rows, dim, n_ord=4):
    """(queries, is_extreme): ordinary queries, scaled copies of corpus rows at G norms, and every other class"""
    rng = np.random.default_rng(seed + 1)
    qo = O.gen_rows(seed + 1, 0, n_ord, dim)
    ext = [v for c, _, v in class_rows(rng, dim) if c != "G"]
    with np.errstate(all="ignore"):                                    # NaN payload rows widen with a warning
        nrm = np.linalg.norm(rows.astype(np.float64), axis=1)
    src = int(np.nonzero(np.isfinite(rows).all(axis=1) & (nrm > 0.5) & (nrm < 2.0))[0][0])   # the first ordinary row
    r0 = rows[src] / np.float32(nrm[src])
    ext += [scaled(r0, g) for g in G_NORMS]
    qs = np.concatenate([qo, np.stack(ext)]).astype(np.float32)
    flag = np.r_[np.zeros(n_ord, bool), np.ones(len(ext), bool)]
    return qs, flag
