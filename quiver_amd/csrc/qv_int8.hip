// qv_int8.hip — the batched filter on the index's 8-bit plane, on the int8 matrix cores (QV_FILTER_INT8)
//
// Every cosine and dot index keeps by default an int8 image of its rows (IndexView::plane8, [tile][dim/16][64 rows][16 values], a scale and a
// residual per row): a quarter of the float32 rows' bytes, and a 16-byte piece of it is exactly one lane's operand of v_mfma_i32_32x32x32_i8.
// The query is quantised as the 8-bit bound scan quantises its own, qq = 128 hi + lo (k_mfma_prep's int8 mode, bound8_split_query), so a score is
// two integer chains, I = 128 I_hi + I_lo, exact in int32 up to 1024 dimensions — the integers of qv_bound.h's 8-bit proof, for 64 queries at once.
//
// Workgroup: eight waves (two per SIMD, 256 registers each), one workgroup per CU and 64-query block (blockIdx.y); a block that holds no real
// query leaves at once.  All eight waves work for the SAME 64 queries: their hi and lo operands, 128 dim bytes (96 KiB at 768 dimensions, 128 KiB
// at 1024), sit in LDS for the whole kernel in the order the prep wrote them — s_a[step][hi, lo][query half][lane], a step = 32 dimensions.
// Rows: each wave streams its own 64-row tiles from the plane straight into B operands — no LDS for rows, no barrier in the loop.  Lane
// (half, l31) of a step loads the 16 bytes of chunk 2 step + half of row 32 j + l31 (two row blocks j per tile): 512 contiguous bytes per lane half.
// Integer sums do not depend on the order of K, so all that matters is that A and B give a (half, byte) the same dimension: 32 step + 16 half + byte.
// R steps (R x 2 KiB per wave: 96 KiB per CU at the R = 6 that ships) are in flight as non-temporal loads; the ring runs on across tiles: the slot a tile's last
// steps free takes the first steps of the wave's next tile.  Per step and wave: four 16-byte LDS reads (A), eight matrix instructions
// (hi and lo chains x two query halves x two row blocks), 128 accumulator registers.
// Epilogue, per (query, row): S~ = fl(fl(sq32 rscale8) fl(I)) (int8_filter_score), then the one-term filter's two-level test with the int8 margin
// ea |r| + eb rres8 (qv_bound.h): a block maximum against a lower bound of the block's 16 thresholds, the few lanes that pass dump their 16 scores
// to LDS, and the dense pass decides per (query, row) with int8_filter_keeps — the function the host exports as qv_batched_int8_keeps.  Dead rows
// and slots past the last row never pass (the alive words decide, not the plane's bytes); a live row the 8-bit bound says nothing about
// (rres8 NaN, rscale8 0 or out of range, a norm that is vanishing or huge) always passes, with a NaN score so that nothing behind reads an
// interval out of it.  Candidates leave through the wave's queue and cand_flush, as in every other filter kernel.
#include "qv_filter.h"
#include "qv_bound.h"

namespace qv {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

#ifndef QV_INT8_RING
#define QV_INT8_RING 6                                                // (8: 256 registers and 5 spilled, 24 bytes of scratch per lane)
#endif
constexpr int kInt8Ring = QV_INT8_RING;                               // steps in flight per wave

// the workgroup's per-query constants in LDS: cm (int8_filter_cm), m, b by query; sq32 in the accumulators' order, [lane half][query half][16]
struct Int8Lds { float cm[64], m[64], b[64], sq[2][2][16]; };

// the dense pass's decision (epi_dense_pass_with / epi_dump_with, qv_filter.h): int8_filter_keeps over the workgroup's constants
template <int METRIC> struct Int8Keep {
    const Int8Lds& k;
    __device__ __forceinline__ bool operator()(uint32_t ql, float score, float rn, float rho, bool unsure) const {
        const float cm = k.cm[ql];
        return int8_filter_keeps<METRIC>(score, cm, k.m[ql], k.b[ql], rn, rho, unsure) && cm < 3.0e38f;   // (padded and declined queries carry +inf)
    }
};

// R: the ring's depth in steps.  DIV: the dimension's steps are a multiple of R, so no step of the unrolled ring is ever idle (768 dimensions:
// 24 steps at R = 6): the loop body is then free of branches.  Every other step count — 1024 dimensions' 32 among them — runs the form whose idle
// ring steps are skipped by wave-uniform branches.
template <int METRIC, int R, bool DIV>
__global__ void __launch_bounds__(512, 1)
k_int8_filter(IndexView v, const uint4* __restrict__ Q8, const float* __restrict__ sq32, const float* __restrict__ cq, const float* __restrict__ mq, uint32_t nq, uint32_t nq_pad,
              uint32_t* __restrict__ cand_rows, float* __restrict__ cand_score, uint32_t* __restrict__ cand_cnt) {
    extern __shared__ __align__(16) unsigned char smem_i8[];
    uint4* s_a = reinterpret_cast<uint4*>(smem_i8);                  // [step][hi, lo][query half][lane]
    __shared__ __align__(16) Int8Lds s_k;
    constexpr bool SETS = false;                                     // (a filtered batch never takes this kernel: launch_batched)
    QV_CAND_QUEUE(cqu, 8, 128);                                      // 12 KiB: the query operands take up to 128 KiB of the 160
    QV_EPI_DUMP(du, 8, 16);                                          // 10 KiB
    const uint32_t qb = blockIdx.y;
    if (64 * qb >= nq) return;                                       // a block made only of padding
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t steps = v.dim / 32, chunks = v.dim / 16;
    for (uint32_t i = threadIdx.x; i < steps * 256; i += 512) s_a[i] = Q8[(size_t)qb * steps * 256 + i];
    if (threadIdx.x < 64) {
        const uint32_t ql = threadIdx.x, q = 64 * qb + ql, w = ql & 31u;
        const float c = cq[q], m = mq[q];
        s_k.cm[ql] = int8_filter_cm<METRIC>(c, m); s_k.m[ql] = m; s_k.b[ql] = mq[nq_pad + q];
        s_k.sq[(w >> 2) & 1u][ql >> 5][(w & 3u) | ((w >> 3) << 2)] = sq32[q];   // ql = 32 i + (r & 3) + 8 (r >> 2) + 4 half, inverted
    }
    __syncthreads();
    const uint32_t half = lane >> 5, l31 = lane & 31;
    float cmin[2], mmax[2], bmax[2];                                 // per query half: what bounds the 16 thresholds of this lane's accumulators from below
#pragma unroll
    for (int i = 0; i < 2; i++) {
        float cm = __builtin_inff(), mm = 0.f, bm = 0.f;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const uint32_t ql = 32 * i + (r & 3) + 8 * (r >> 2) + 4 * half;
            cm = fminf(cm, s_k.cm[ql]); mm = fmaxf(mm, s_k.m[ql]); bm = fmaxf(bm, s_k.b[ql]);
        }
        cmin[i] = cm; mmax[i] = mm; bmax[i] = bm;
    }
    const float tiny = filter_tiny_norm(v.dim);
    const Int8Keep<METRIC> keep{s_k};
    const i32x4* plane = reinterpret_cast<const i32x4*>(v.plane8);
    const uint32_t gw = blockIdx.x * 8 + wave, tw = gridDim.x * 8;
    // block j of tile t at step 0: chunk `half` of rows 32 j + l31; a step is two chunks on (128 pieces)
    auto base = [&](uint32_t t, int j) { return plane + ((size_t)t * chunks + half) * 64 + 32 * j + l31; };
    i32x4 rb[R][2];
    bool primed = false;
    for (uint32_t g = gw; g < v.n_tiles; g += tw) {
        const uint32_t gn = g + tw < v.n_tiles ? g + tw : g;       // past the wave's last tile: the same tile again (in bounds, read by nobody)
        const i32x4* p[2] = {base(g, 0), base(g, 1)};
        const i32x4* np[2] = {base(gn, 0), base(gn, 1)};
        double rnd[2]; float rsc[2], rho[2];
#pragma unroll
        for (int j = 0; j < 2; j++) { const size_t row = (size_t)g * 64 + 32 * j + l31; rnd[j] = v.rnorm[row]; rsc[j] = v.rscale8[row]; rho[j] = v.rres8[row]; }
        const uint64_t alv = v.alive[g];
        i32x16 acc[2][2][2];                                         // [hi, lo][query half][row block]
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++)
#pragma unroll
                    for (int e = 0; e < 16; e++) acc[t][i][j][e] = 0;
        if (!primed) {
            primed = true;
#pragma unroll
            for (int k = 0; k < R; k++)
                if (DIV || (uint32_t)k < steps) { rb[k][0] = __builtin_nontemporal_load(p[0] + (size_t)k * 128); rb[k][1] = __builtin_nontemporal_load(p[1] + (size_t)k * 128); }
        }
        for (uint32_t st = 0; st < steps; st += R) {
#pragma unroll
            for (int k = 0; k < R; k++) {
                const uint32_t s_ = st + k;
                if (DIV || s_ < steps) {
                    const uint4* ap = s_a + s_ * 256 + lane;
                    const i32x4 ah0 = __builtin_bit_cast(i32x4, ap[0]), ah1 = __builtin_bit_cast(i32x4, ap[64]);
                    const i32x4 al0 = __builtin_bit_cast(i32x4, ap[128]), al1 = __builtin_bit_cast(i32x4, ap[192]);
#pragma unroll
                    for (int j = 0; j < 2; j++) {
                        acc[0][0][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ah0, rb[k][j], acc[0][0][j], 0, 0, 0);
                        acc[0][1][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ah1, rb[k][j], acc[0][1][j], 0, 0, 0);
                        acc[1][0][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(al0, rb[k][j], acc[1][0][j], 0, 0, 0);
                        acc[1][1][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(al1, rb[k][j], acc[1][1][j], 0, 0, 0);
                    }
                    // the slot is free: step s_ + R of this tile, or — behind the tile's last R steps — step k of the wave's next tile
                    const bool here = s_ + R < steps;
                    if (DIV || here || (uint32_t)k < steps) {
                        const size_t off = (size_t)(here ? s_ + R : (uint32_t)k) * 128;
                        rb[k][0] = __builtin_nontemporal_load((here ? p[0] : np[0]) + off);
                        rb[k][1] = __builtin_nontemporal_load((here ? p[1] : np[1]) + off);
                    }
                }
            }
        }
        uint32_t n = 0;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint32_t row = g * 64 + 32 * j + l31;
            const bool live = (alv >> (32 * j + l31)) & 1ull;
            const float rn = bound_f32_up((float)rnd[j]);
            const bool unsure = int8_filter_row_unsure(rn, rsc[j], rho[j], tiny);
#pragma unroll
            for (int i = 0; i < 2; i++) {
                f16v a;
#pragma unroll
                for (int e = 0; e < 16; e++) a[e] = int8_filter_score(acc[0][i][j][e], acc[1][i][j][e], s_k.sq[half][i][e], rsc[j]);
                const float m0 = __builtin_fmaxf(__builtin_fmaxf(a[0], a[1]), a[2]), m1 = __builtin_fmaxf(__builtin_fmaxf(a[3], a[4]), a[5]);
                const float m2 = __builtin_fmaxf(__builtin_fmaxf(a[6], a[7]), a[8]), m3 = __builtin_fmaxf(__builtin_fmaxf(a[9], a[10]), a[11]);
                const float m4 = __builtin_fmaxf(__builtin_fmaxf(a[12], a[13]), a[14]);
                const float mx = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(m0, m1), m2), __builtin_fmaxf(__builtin_fmaxf(m3, m4), a[15]));
                // level 1: the threshold is monotone in cm (up), m and b (down), so this is a lower bound of the block's 16 thresholds
                const float thr_lo = int8_filter_threshold<METRIC>(cmin[i], mmax[i], bmax[i], rn, rho[j]);
                const uint64_t pm = __ballot((!(mx < thr_lo) || unsure) && live);
                if (__builtin_expect(pm != 0, 0)) epi_dump_with(a, pm, row, rn, rho[j], (uint32_t)i, half, unsure, keep, 64 * qb, cqu, cqu_n, cqu_out, du, n);
            }
        }
        if (n) epi_dense_pass_with(du, n, keep, 64 * qb, cqu, cqu_n, cqu_out);
    }
    cand_flush(cqu, cqu_n, cqu_out);
}

size_t int8_filter_lds_bytes(uint32_t dim) { return (size_t)dim * 128; }

hipError_t launch_int8_filter(const IndexView& v, const void* Q8, const float* cq, const float* mq, uint32_t nq, uint32_t nq_pad, uint32_t* cand, float* cscore,
                              uint32_t* cnt, uint32_t grid_x, size_t lds, hipStream_t s) {
    if (v.plane8 == nullptr || (v.dim & 31u) || v.dim < 64 || v.dim > 1024 || (v.metric != QV_COSINE && v.metric != QV_DOT)) return hipErrorInvalidValue;   // (a missing route is an error)
    if (grid_x == 0 || lds < int8_filter_lds_bytes(v.dim)) return hipErrorInvalidValue;
    const uint32_t steps = v.dim / 32;
    const dim3 grid(grid_x, nq_pad / 64);                            // (the route's: batched_int8_adapt)
    const uint4* q8 = static_cast<const uint4*>(Q8);
    const float* sq32 = reinterpret_cast<const float*>(static_cast<const char*>(Q8) + (size_t)nq_pad * 2 * v.dim);
    auto go = [&](auto kernel) {
        const hipError_t e = set_lds(kernel, lds); if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, grid, dim3(512), lds, s, v, q8, sq32, cq, mq, nq, nq_pad, cand, cscore, cnt);
        return hipGetLastError();
    };
    const bool div = steps % kInt8Ring == 0;
    if (v.metric == QV_COSINE) return div ? go(k_int8_filter<QV_COSINE, kInt8Ring, true>) : go(k_int8_filter<QV_COSINE, kInt8Ring, false>);
    return div ? go(k_int8_filter<QV_DOT, kInt8Ring, true>) : go(k_int8_filter<QV_DOT, kInt8Ring, false>);
}

// the batch's counters, behind its last kernel: batches, queries, queries handed back (their redo flags)
__global__ void __launch_bounds__(256) k_int8_filter_count(const uint32_t* __restrict__ redo, uint32_t nq, uint32_t* __restrict__ stats) {
    uint32_t n = 0;
    for (uint32_t q = threadIdx.x; q < nq; q += 256) n += redo[q] ? 1u : 0u;
    if (n) (void)atomicAdd(&stats[kInt8FilterStatsWord + 2], n);
    if (threadIdx.x == 0) { (void)atomicAdd(&stats[kInt8FilterStatsWord], 1u); (void)atomicAdd(&stats[kInt8FilterStatsWord + 1], nq); }
}
hipError_t launch_int8_filter_count(const uint32_t* d_redo, uint32_t nq, uint32_t* d_stats, hipStream_t s) {
    hipLaunchKernelGGL(k_int8_filter_count, dim3(1), dim3(256), 0, s, d_redo, nq, d_stats);
    return hipGetLastError();
}

int host_int8_filter_keeps(int metric, uint32_t dim, int32_t isum_hi, int32_t isum_lo, double sq, double qn, double qres, float U, double rn, float rscale8, float rres8) {
    if (metric != QV_COSINE && metric != QV_DOT) return -1;
    auto f = [&](auto mc) {
        constexpr int M = decltype(mc)::value;
        const Int8QueryConsts kc = int8_filter_query_consts<M>(dim, sq, qn, qres, (double)U);
        if (kc.declined) return 1;                                     // (the query is handed back: nothing is decided by its scores)
        const float rnf = bound_f32_up((float)rn);
        const bool unsure = int8_filter_row_unsure(rnf, rscale8, rres8, filter_tiny_norm(dim));
        return int8_filter_keeps<M>(int8_filter_score(isum_hi, isum_lo, kc.sq32, rscale8), int8_filter_cm<M>(kc.c, kc.m), kc.m, kc.b, rnf, rres8, unsure) ? 1 : 0;
    };
    return metric == QV_COSINE ? f(std::integral_constant<int, QV_COSINE>{}) : f(std::integral_constant<int, QV_DOT>{});
}

}  // namespace qv
