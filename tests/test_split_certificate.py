"""The arithmetic behind the latency form of the HNSW traversal (quiver_amd/csrc/qv_hnsw.hip, "a row's sum over several lanes,
certified"): the reference accumulates a distance as ONE float64 chain in element order (pkg/vectortypes/distances.go:18-22); the
latency form adds the same exact products as many partial chains and returns the float32 only when the interval
[S - B, S + B] around its sum maps to a single float32 through the (monotone) finalisation.  Checked here on the CPU, in
numpy float64 (IEEE, same roundings as the device's v_fma_f64 on exact products):
  * the reference's chain always lies inside [S - B, S + B] for the bound the kernel uses;
  * the finalisation is monotone in the sum, so equal ends decide the float32;
  * the bound is small enough that the certificate holds for all but a tiny share of evaluations."""
import numpy as np
import pytest

from tests._order import planted_rows, query_for, scan_split_sum, split_sum, workgroup_sum

U = 2.0 ** -53
SLACK = 128.0


def seq_sum(p):                       # one chain, element order: cumsum adds left to right, one rounding per step
    return float(np.cumsum(p)[-1]) if len(p) else 0.0


def cosine_finalize(acc, qn, rn):     # distances.go:25-39 (float64, then float32)
    if qn == 0.0 or rn == 0.0:
        return np.float32(1.0)
    sim = acc / (qn * rn)
    sim = min(1.0, max(-1.0, sim))
    return np.float32(1.0 - sim)


@pytest.mark.parametrize("dim", [32, 96, 128, 768, 1024])
@pytest.mark.parametrize("lanes_per_row", [2, 4, 8])
def test_reference_chain_lies_in_the_certified_interval(dim, lanes_per_row):
    rng = np.random.default_rng(dim * 10 + lanes_per_row)
    undecided = 0
    trials = 400
    for t in range(trials):
        scale = 10.0 ** rng.integers(-3, 4)
        q = (rng.standard_normal(dim) * scale).astype(np.float32)
        r = (rng.standard_normal(dim) * scale).astype(np.float32)
        if t % 5 == 0:
            r = (q * np.float32(1.0 + 1e-3 * rng.standard_normal())).astype(np.float32)      # nearly parallel: the clamp's neighbourhood
        p = q.astype(np.float64) * r.astype(np.float64)                  # exact: 24 x 24 bits
        s_ref = seq_sum(p)
        s = split_sum(p, 8, lanes_per_row)
        qn = float(np.sqrt(seq_sum(q.astype(np.float64) ** 2))); rn = float(np.sqrt(seq_sum(r.astype(np.float64) ** 2)))
        b = (2.0 * dim + SLACK) * U * qn * rn                            # split_bound<QV_COSINE>
        assert s - b <= s_ref <= s + b, (dim, t, s, s_ref, b)
        # and with room to spare: the a-priori bound, g(h) sum|p|, is itself below b
        assert abs(s - s_ref) <= (dim + dim // lanes_per_row + 16) * U * float(np.sum(np.abs(p))) * 1.0001 + 1e-300
        d_lo, d_hi, d_ref = cosine_finalize(s - b, qn, rn), cosine_finalize(s + b, qn, rn), cosine_finalize(s_ref, qn, rn)
        assert d_hi <= d_ref <= d_lo                                     # monotone (non-increasing in the sum)
        if d_lo.tobytes() == d_hi.tobytes():
            assert d_ref.tobytes() == d_lo.tobytes()                     # the certificate decides the float32
        else:
            undecided += 1                                               # the kernel walks the row again as one chain
    assert undecided <= trials // 4                                      # (only the nearly-parallel pairs: distances near 0)


def test_nonnegative_terms_bound_is_the_sum_itself():
    """L2 / L1 / squared-L2-in-float64: every term is >= 0, so sum|t_i| is the sum and B = k_u * S"""
    rng = np.random.default_rng(7)
    for dim in (32, 160, 768):
        for _ in range(200):
            a = rng.standard_normal(dim).astype(np.float32); b_ = rng.standard_normal(dim).astype(np.float32)
            d = (a - b_).astype(np.float64)                              # float32 subtract, widened (distances.go:50)
            t = d * d                                                    # exact
            s_ref, s = seq_sum(t), split_sum(t, 8, 4)
            b = (2.0 * dim + SLACK) * U * s
            assert s - b <= s_ref <= s + b
            lo, hi, ref = np.float32(np.sqrt(max(s - b, 0.0))), np.float32(np.sqrt(s + b)), np.float32(np.sqrt(s_ref))
            assert lo <= ref <= hi


def _scan_cosine_interval(q, r):
    """k_flat_scan_split's certificate for cosine (qv_scan.hip): S = the eight waves' partial chains added in order, |q| from a
    sum over the workgroup, B = k_u |q| |r| widened by (|S| + B) 2 k_u for that norm's own error"""
    dim4 = (q.size + 3) // 4
    k_u = (2.0 * (4 * dim4) + SLACK) * U
    q64, r64 = q.astype(np.float64), r.astype(np.float64)
    p = q64 * r64
    s = scan_split_sum(np.concatenate([p, np.zeros(4 * dim4 - p.size)]))
    qn_s = float(np.sqrt(workgroup_sum(q64 * q64)))
    rn = float(np.sqrt(seq_sum(r64 * r64)))
    b = k_u * qn_s * rn
    b = b + (abs(s) + b) * (2.0 * k_u)
    return s, b, qn_s, rn


@pytest.mark.parametrize("dim", [128, 130, 256, 768, 1000, 1536])
def test_split_scan_cosine_with_a_workgroup_norm(dim):
    """The split scan's cosine case: the query's norm is a workgroup sum, not the reference's chain, and its error widens the
    interval.  The reference's distance (chain dot product, chain norm) must lie between the distances of the interval's ends
    computed with the workgroup norm — on random, nearly parallel and planted (tests/_order.py) pairs — and where the ends agree,
    the reference has that float32."""
    rng = np.random.default_rng(31 * dim)
    pairs = []
    for t in range(300):
        scale = 10.0 ** rng.integers(-3, 4)
        q = (rng.standard_normal(dim) * scale).astype(np.float32)
        r = (rng.standard_normal(dim) * scale).astype(np.float32)
        if t % 3 == 0:
            r = (q * (1.0 + 10.0 ** rng.uniform(-7, -2) * rng.standard_normal(dim))).astype(np.float32)
        pairs.append((q, r))
    q = query_for(0, dim, rng)
    planted = planted_rows(0, dim, q, 12, rng)
    assert len(planted) >= 6
    pairs += [(q, r) for r in planted]
    decided = 0
    for q, r in pairs:
        s, b, qn_s, rn = _scan_cosine_interval(q, r)
        q64, r64 = q.astype(np.float64), r.astype(np.float64)
        s_ref = seq_sum(q64 * r64)
        qn = float(np.sqrt(seq_sum(q64 * q64)))
        d_ref = cosine_finalize(s_ref, qn, rn)
        d_lo, d_hi = cosine_finalize(s - b, qn_s, rn), cosine_finalize(s + b, qn_s, rn)
        assert d_hi <= d_ref <= d_lo, (dim, s, b, s_ref, qn, qn_s)
        if d_lo.tobytes() == d_hi.tobytes():
            assert d_ref.tobytes() == d_lo.tobytes()
            decided += 1
    for q_, r_ in [(q, r) for r in planted]:                 # planted rows: never decided (the fallback runs)
        s, b, qn_s, rn = _scan_cosine_interval(q_, r_)
        assert cosine_finalize(s - b, qn_s, rn).tobytes() != cosine_finalize(s + b, qn_s, rn).tobytes()
    assert decided >= 150                                    # (the random pairs: the certificate holds for most)
