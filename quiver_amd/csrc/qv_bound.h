// qv_bound.h — the interval the single-query bound scan (qv_bound_scan.hip: k_bound_scan) derives for one row from the bfloat16 copy.
// ONE statement of it for the device and the host (qv_scan_bound_interval: what the CPU test of the bound calls).
//
// Stage 1 computes S~ = a float32 chain of K = dim fused multiply-adds over q_i * rh_i, with q the caller's float32 query and
// rh = bf16(r) widened (exact).  Against the reference's sum S (a float64 chain over the exact products q_i * r_i):
//   |S~ - q.rh|  <= gamma_K sum |q_i rh_i| <= gamma_K |q| |rh|,  gamma_K = K u / (1 - K u), u = 2^-24   (one rounding per fma)
//   |q.rh - q.r| <= |q| |r - rh|                                                                     (Cauchy-Schwarz)
//   |rh| <= |r| + |r - rh|,  and |r - rh| <= rres (kept per row, rounded up: k_row_residual)
//   |q.r - S|    <= dim 2^-53 |q||r|                                                                 (the float64 chain's own error)
// so |S~ - S| <= |q| (rres + gamma (|r| + rres)) with gamma = filter_gamma(dim, 0) (K + 2 roundings) plus 5e-7 for products or
// partial sums lost to underflow (at most dim * 1.2e-38, below 5e-7 |q||r| once both norms pass filter_tiny_norm: qv_filter.h) plus
// 1e-12 for the float64 chains (S, the stored norms).  The distance is a monotone (non-increasing) function of the sum — the
// division, the clamp, the subtraction and both roundings of finalize<M> are — so the float32 distance of the reference lies in
// [finalize(S~ + m), finalize(S~ - m)], with the reference's own |q| and |r| in it: nothing else has to be rounded outward.
//
// ---- the Euclidean distance (QV_L2) from the same sums ----
// The margin m above bounds |S~ - q.r| against the REAL dot product (the derivation passes through it; its last term is then slack), for the
// bfloat16 chain and for the 8-bit integers alike, so stage 1 is untouched.  The reference (distances.go:48-54; acc1<QV_L2> / finalize<QV_L2>)
// computes d_i = (double)fl32(q_i - r_i), D = a float64 fma chain of d_i^2, and returns (float)sqrt(D).  With E = |q - r|^2 = |q|^2 + |r|^2 - 2 q.r
// as real numbers:
//   fl32(q_i - r_i) = (q_i - r_i)(1 + delta), |delta| <= 2^-24   (a float32 difference in the subnormal range is exact: no underflow term)
//   d_i^2 does not underflow in float64 (|d_i| >= 2^-149 or 0), and the chain of dim non-negative terms adds at most (dim + 1) 2^-53 relative
//   so D in E [1 - theta, 1 + theta] with theta = 1.2e-7 >= 2^-23 + 2^-48 + 4097 * 2^-53 (dim <= 4096).
// A = qn^2 + rn^2 from the norms at hand (float64 chains of dim terms and a square root each, squared again here): off by less than
// 1e-12 A from |q|^2 + |r|^2, and A - 2 S~ is formed here with three more roundings of at most 2^-53 A each (|S~| <= A / 2 + m): together
// below the 2e-12 A the interval carries.  So
//   E in [A - 2 S~ - 2 m - 2e-12 A, A - 2 S~ + 2 m + 2e-12 A] = [E_lo, E_hi]
//   D_lo = max(0, E_lo) (1 - theta)(1 - 1e-9),  D_hi = E_hi (1 + theta)(1 + 1e-9)      (the last factor: these lines' own roundings)
// and the float32 distance of the reference lies in [finalize<QV_L2>(D_lo), finalize<QV_L2>(D_hi)]: the square root is the correctly
// rounded one the exact scan takes and the float32 rounding is monotone, so nothing else is rounded outward.  A row equal to the query
// has E = 0 >= E_lo, hence d_lo = 0.0 exactly.  E_hi that is NaN or negative (norms that are not numbers; never for a sum within its
// margin) makes the row "unsure".  Rows within about 2 sqrt(m) of the query have d_lo = 0: they cost survivors only where the k-th
// neighbour itself is that close — cosine's near-duplicate behaviour, in distance.  A zero query is legitimate here, but its norm is not one the
// bound works with (bound_scan_norm_ok): the re-score hands such a query back to the exact scan, as for cosine and dot.
#pragma once
#include "qv_kernels.h"
#include "qv_filter.h"

namespace qv {

__host__ __device__ static inline double bound_scan_gamma(uint32_t dim) { return filter_gamma(dim, 0) * (1.0 + 1e-6) + 5e-7 + 1e-12; }

// a norm the bound can work with (rows and the query alike): a number, not huge (the float32 chain may have overflowed on the way),
// not vanishing (underflow is outside the error model)
__host__ __device__ static inline bool bound_scan_norm_ok(double n, uint32_t dim) { return n >= (double)filter_tiny_norm(dim) && n < 1.0e18; }

constexpr double kBoundL2Theta = 1.2e-7, kBoundL2NormSlack = 2e-12;
// the Euclidean interval from s = S~ (float64), its margin m, and the two norms; false: E_hi is not a non-negative number
__host__ __device__ __forceinline__ bool bound_l2_ends(double s, double m, double qn, double rn, float& d_lo, float& d_hi) {
    const double A = __builtin_fma(qn, qn, rn * rn);
    const double c = A - 2.0 * s, w = 2.0 * m + kBoundL2NormSlack * A;
    const double e_lo = c - w, e_hi = c + w;
    if (!(e_hi >= 0.0)) { d_lo = -__builtin_inff(); d_hi = __builtin_nanf(""); return false; }
    QConst qc; qc.qn = qn; qc.qn32 = 0.0f;
    d_lo = finalize<QV_L2>((e_lo > 0.0 ? e_lo : 0.0) * ((1.0 - kBoundL2Theta) * (1.0 - 1e-9)), qc, rn);
    d_hi = finalize<QV_L2>(e_hi * ((1.0 + kBoundL2Theta) * (1.0 + 1e-9)), qc, rn);
    return true;
}

// s = S~, qn = |q| (the reference's chain), rn = |r| (stored), rres = |r - bf16(r)| rounded up (stored).  false: a row the bound says
// nothing about — always a candidate (d_lo = -inf), never lowers a threshold (d_hi = NaN).
template <int M>
__host__ __device__ __forceinline__ bool bound_scan_interval(float s, double qn, double rn, float rres, uint32_t dim, double gamma, float& d_lo, float& d_hi) {
    static_assert(M == QV_COSINE || M == QV_DOT || M == QV_L2, "the bound scan's metrics");
    const double rr = (double)rres;
    const bool sure = bound_scan_norm_ok(rn, dim) && rr >= 0.0 && rr < 1.0e18 && (s - s) == 0.0f;
    if (!sure) { d_lo = -__builtin_inff(); d_hi = __builtin_nanf(""); return false; }
    const double m = qn * (rr + gamma * (rn + rr)) * (1.0 + 1e-9);     // (the factor: this line's own roundings, and S~ +- m below)
    if constexpr (M == QV_L2) return bound_l2_ends((double)s, m, qn, rn, d_lo, d_hi);
    QConst qc; qc.qn = qn; qc.qn32 = 0.0f;
    d_lo = finalize<M>((double)s + m, qc, rn);
    d_hi = finalize<M>((double)s - m, qc, rn);
    return true;
}

// ---- the 8-bit plane (k_bound_scan8): the same interval from integers ----
// The index keeps r8 = an int8 image of every row with one float32 scale per row (bound8_scale / bound8_quant below) and
// rres8 = |r - scale r8|, computed in float64 FROM THE BYTES STORED and rounded up (k_row_state8), so nothing below depends on how
// the quantiser rounds.  The query is quantised once per workgroup: qq_i = rint(q_i / sq), sq = max|q_i| / 16256, split into two
// int8 terms qq = 128 hi + lo (|hi| <= 127, |lo| <= 64).  Stage 1 computes I = 128 sum hi_i r8_i + sum lo_i r8_i = sum qq_i r8_i with
// integer dot products (each sum is exact in int32 up to 4096 dimensions: 4096 * 127 * 127 < 2^31; their combination is exact in
// float64) and S~ = sq * scale * I in float64.  With qh = sq qq, rh = scale r8 (so qh.rh = sq scale I as real numbers),
// qres = |q - qh| (float64, rounded up, computed by the caller beside the reference's |q| chain) and S the reference's float64 chain:
//   |S~ - qh.rh|  <= 2 * 2^-53 |qh.rh| (1 + 2^-53) <= 2.3e-16 (|q| + qres)(|r| + rres8)     (the two float64 multiplies)
//   |qh.rh - q.rh| <= qres |rh| <= qres (|r| + rres8)                                        (Cauchy-Schwarz)
//   |q.rh - q.r|   <= |q| rres8                                                              (Cauchy-Schwarz)
//   |q.r - S|      <= dim 2^-53 |q||r| <= 4.6e-13 |q||r|                                     (the float64 chain's own error, dim <= 4096)
// so |S~ - S| <= |q| rres8 + qres (|r| + rres8) + 1e-12 (|q| + qres)(|r| + rres8): the last term is the slack for the two multiplies,
// the chain, and the roundings of qres itself (each of its terms is off by at most 2^-52 |q_i|); the factor 1 + 1e-9 covers this
// line's own roundings and S~ +- m, as in bound_scan_interval.  There is no float32 chain: no gamma_K term and no underflow term
// (integers do not underflow; a row or a query whose norm is vanishing or huge is declined as before).  The distance interval is
// [finalize(S~ + m), finalize(S~ - m)] with the reference's own |q| and |r|, exactly as above.
constexpr int kBound8QueryMax = 16256;           // 127 * 128: the quantised query's largest magnitude

// scale = max|r_i| / 127 rounded UP (one float32 step), so that |r_i / scale| <= 127 before rounding; 0 for a row without a scale
__host__ __device__ static inline float bound8_scale(float maxabs) {
    if (!(maxabs > 0.0f) || maxabs == __builtin_inff()) return 0.0f;
    const float s = maxabs / 127.0f;
    union { float f; uint32_t u; } c; c.f = s; c.u += 1u;
    return c.f == __builtin_inff() ? s : c.f;
}
__host__ __device__ static inline int bound8_quant(float x, float scale) {
    float v = __builtin_rintf(x / scale);
    v = __builtin_fminf(__builtin_fmaxf(v, -127.0f), 127.0f);          // (a NaN quotient comes out as -127: such a row is declined anyway)
    return (int)v;
}
// the residual's float32: sqrt of the float64 sum, a hair up, then one float32 step up — k_row_residual's rounding
__host__ __device__ static inline float bound8_res_up(double s2) {
    const float r = (float)(__builtin_sqrt(s2) * (1.0 + 1e-12));
    if (!(r == r) || r == __builtin_inff()) return __builtin_nanf("");
    union { float f; uint32_t u; } c; c.f = r;
    if (r == 0.f) c.u = s2 == 0.0 ? 0u : 1u; else c.u += 1u;
    return c.f;
}
// One row's state from its statistics: bad = a non-finite element, maxabs, n2 = sum r_i^2 (float64), s2 = sum (r_i - scale r8_i)^2.
// NaN: a row the bound says nothing about.
__host__ __device__ static inline float bound8_row_res(bool bad, float maxabs, double n2, double s2, uint32_t dim) {
    if (bad || !(maxabs > 0.0f) || maxabs == __builtin_inff() || !bound_scan_norm_ok(__builtin_sqrt(n2), dim)) return __builtin_nanf("");
    return bound8_res_up(s2);
}

// ---- the 6-bit plane (k_bound_scan6): the 8-bit interval with a coarser image of the row ----
// An index that keeps the 8-bit plane and whose dimension is a multiple of 64 also keeps c6_i = clamp(rint(r_i / (4 rscale8)), -32, 31),
// stored biased as u_i = c6_i + 32 in six bits (bound6_pack below), and rres6 = |r - 4 rscale8 c6|, computed in float64 FROM THE CODES
// STORED and rounded up with bound8_res_up (k_row_state6); rows bound8_row_res declines are declined here (NaN).  No scale of its own:
// 4 rscale8 is exact in float32 (rscale8 < 1e36 is asked below).  Stage 1 computes I6 = sum qq_i u_i - 32 sum qq_i = sum qq_i c6_i with
// the same two int8 query terms (u_i <= 63 is a non-negative int8; each partial sum stays exact in int32: 4096 * 127 * 63 < 2^31) and
// calls bound_scan_interval8(I6, sq, qn, qres, rn, 4 rscale8, rres6).  The proof above holds line for line with rh = 4 rscale8 c6 and
// rres6 in the place of rres8: it uses of rh only that qh.rh = sq scale I as real numbers and |r - rh| <= the stored residual.
constexpr int kBound6Bias = 32;
__host__ __device__ static inline int bound6_quant(float x, float scale8) {
    float v = __builtin_rintf(x / (4.0f * scale8));
    v = __builtin_fminf(__builtin_fmaxf(v, -32.0f), 31.0f);            // (a NaN quotient comes out as -32: such a row is declined anyway)
    return (int)v;
}
// The plane's layout, [tile][group of 64 dims][3][64 rows][16 B]: where the biased code of dimension d of a row's group lives in the row's
// three 16-byte pieces X, Y, Z.  Dims 0 - 47: the low six bits of byte d & 15 of piece d >> 4.  Dims 48 - 63: two bits in the top of byte
// d - 48 of each piece, X the code's bits 0 - 1, Y its bits 2 - 3, Z its bits 4 - 5.
__host__ __device__ static inline void bound6_pack(uint8_t (&g)[48], uint32_t d, uint32_t u) {
    if (d < 48u) { g[d] = (uint8_t)((g[d] & 0xC0u) | (u & 0x3Fu)); return; }
    const uint32_t j = d - 48u;
    g[j] = (uint8_t)((g[j] & 0x3Fu) | ((u & 3u) << 6));
    g[16 + j] = (uint8_t)((g[16 + j] & 0x3Fu) | (((u >> 2) & 3u) << 6));
    g[32 + j] = (uint8_t)((g[32 + j] & 0x3Fu) | (((u >> 4) & 3u) << 6));
}
__host__ __device__ static inline uint32_t bound6_unpack(const uint8_t (&g)[48], uint32_t d) {
    if (d < 48u) return g[d] & 0x3Fu;
    const uint32_t j = d - 48u;
    return (uint32_t)(g[j] >> 6) | ((uint32_t)(g[16 + j] >> 6) << 2) | ((uint32_t)(g[32 + j] >> 6) << 4);
}

// isum = I, sq = the query's scale, qn = |q| (the reference's chain), qres = |q - sq qq| rounded up, rn = |r| (stored),
// rscale / rres8 = the row's scale and residual.  false: a row (or a query) the bound says nothing about — always a candidate
// (d_lo = -inf), never lowers a threshold (d_hi = NaN).
template <int M>
__host__ __device__ __forceinline__ bool bound_scan_interval8(long long isum, double sq, double qn, double qres, double rn, float rscale, float rres8, uint32_t dim,
                                                              float& d_lo, float& d_hi) {
    static_assert(M == QV_COSINE || M == QV_DOT || M == QV_L2, "the bound scan's metrics");
    const double rr = (double)rres8, sc = (double)rscale;
    const bool sure = bound_scan_norm_ok(rn, dim) && bound_scan_norm_ok(qn, dim) && rr >= 0.0 && rr < 1.0e18 && qres >= 0.0 && qres < 1.0e18 &&
                      sq > 0.0 && sq < 1.0e36 && sc > 0.0 && sc < 1.0e36;
    if (!sure) { d_lo = -__builtin_inff(); d_hi = __builtin_nanf(""); return false; }
    const double s = sq * sc * (double)isum;
    const double m = (qn * rr + qres * (rn + rr) + 1e-12 * (qn + qres) * (rn + rr)) * (1.0 + 1e-9);
    if constexpr (M == QV_L2) return bound_l2_ends(s, m, qn, rn, d_lo, d_hi);
    QConst qc; qc.qn = qn; qc.qn32 = 0.0f;
    d_lo = finalize<M>(s + m, qc, rn);
    d_hi = finalize<M>(s - m, qc, rn);
    return true;
}

}  // namespace qv
