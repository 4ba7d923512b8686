// qv_bound.h — the interval the single-query bound scan (qv_scan.hip: k_bound_scan) derives for one row from the bfloat16 copy.
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
#pragma once
#include "qv_kernels.h"
#include "qv_filter.h"

namespace qv {

__host__ __device__ static inline double bound_scan_gamma(uint32_t dim) { return filter_gamma(dim, 0) * (1.0 + 1e-6) + 5e-7 + 1e-12; }

// a norm the bound can work with (rows and the query alike): a number, not huge (the float32 chain may have overflowed on the way),
// not vanishing (underflow is outside the error model)
__host__ __device__ static inline bool bound_scan_norm_ok(double n, uint32_t dim) { return n >= (double)filter_tiny_norm(dim) && n < 1.0e18; }

// s = S~, qn = |q| (the reference's chain), rn = |r| (stored), rres = |r - bf16(r)| rounded up (stored).  false: a row the bound says
// nothing about — always a candidate (d_lo = -inf), never lowers a threshold (d_hi = NaN).
template <int M>
__host__ __device__ __forceinline__ bool bound_scan_interval(float s, double qn, double rn, float rres, uint32_t dim, double gamma, float& d_lo, float& d_hi) {
    static_assert(M == QV_COSINE || M == QV_DOT, "the bound scan's metrics");
    const double rr = (double)rres;
    const bool sure = bound_scan_norm_ok(rn, dim) && rr >= 0.0 && rr < 1.0e18 && (s - s) == 0.0f;
    if (!sure) { d_lo = -__builtin_inff(); d_hi = __builtin_nanf(""); return false; }
    const double m = qn * (rr + gamma * (rn + rr)) * (1.0 + 1e-9);     // (the factor: this line's own roundings, and S~ +- m below)
    QConst qc; qc.qn = qn; qc.qn32 = 0.0f;
    d_lo = finalize<M>((double)s + m, qc, rn);
    d_hi = finalize<M>((double)s - m, qc, rn);
    return true;
}

}  // namespace qv
