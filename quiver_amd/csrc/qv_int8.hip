// qv_int8.hip — the batched filter on the index's 8-bit plane, on the int8 matrix cores (QV_FILTER_INT8)
//
// Every cosine and dot index keeps by default an int8 image of its rows (IndexView::plane8, [tile][dim/16][64 rows][16 values], a scale and a
// residual per row): a quarter of the float32 rows' bytes, and a 16-byte piece of it is exactly one lane's operand of v_mfma_i32_32x32x32_i8.
// The query is quantised as the 8-bit bound scan quantises its own, qq = 128 hi + lo (k_mfma_prep's int8 mode, bound8_split_query), so a score is
// two integer chains, I = 128 I_hi + I_lo, exact in int32 up to 1024 dimensions — the integers of qv_bound.h's 8-bit proof, for 64 queries at once.
// (1056 to 4096 dimensions: k_int8_wide_filter below — the same workgroup with the operands passing through LDS in panels, the sum in float64.)
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
// A FILTERED batch (a row set per query) takes the same kernel in its sets form (template parameter TS, behind k_int8_tiles; opt-in,
// qv_index_set_int8_filtered): it reads only the tiles some query of the block selects and decides membership per (query, row) in the epilogue.
#include "qv_filter.h"
#include "qv_bound.h"
#include "qv_lds_dma.h"

namespace qv {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

#ifndef QV_INT8_RING
#define QV_INT8_RING 6                                                // (8: 256 registers and 5 spilled, 24 bytes of scratch per lane)
#endif
constexpr int kInt8Ring = QV_INT8_RING;                               // steps in flight per wave
#ifndef QV_INT8_SETS_RING
#define QV_INT8_SETS_RING 6                                          // the sets form's own depth (profiles/int8_filtered_resources.txt)
#endif
constexpr int kInt8SetsRing = QV_INT8_SETS_RING;
constexpr size_t kInt8SetWordBytes = 8 * 512;                         // the sets form: 64 set words per wave, behind the operands in LDS
#ifndef QV_INT8_SHARED_LSTEPS
#define QV_INT8_SHARED_LSTEPS 2                                      // the shared-row form at 768 dimensions: steps whose operands live in LDS
#endif

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

// The sets form's (TS): a (query, row) pair outside the query's set reaches the dump as kInt8OutOfSet — the epilogue writes it over the pair's score,
// and no pair inside a set carries it (int8_in_set_score) — so membership is tested HERE, in front of `unsure`, which keeps a row whatever its score.
constexpr uint32_t kInt8OutOfSet = 0xFF800000u;                       // -inf: never raises a block's maximum either
template <int METRIC> struct Int8KeepSets {
    const Int8Lds& k;
    __device__ __forceinline__ bool operator()(uint32_t ql, float score, float rn, float rho, bool unsure) const {
        return __float_as_uint(score) != kInt8OutOfSet && Int8Keep<METRIC>{k}(ql, score, rn, rho, unsure);
    }
};
// a pair inside its query's set never carries the mark: a score of -inf says what -FLT_MAX says (below every threshold that is not -inf itself; no
// interval is read out of either: k_rescore_select's |S| < 3e38)
__device__ __forceinline__ float int8_in_set_score(float s) { return __float_as_uint(s) == kInt8OutOfSet ? -3.4028234663852886e38f : s; }

// R: the ring's depth in steps.  DIV: the dimension's steps are a multiple of R, so no step of the unrolled ring is ever idle (768 dimensions:
// 24 steps at R = 6): the loop body is then free of branches.  Every other step count — 1024 dimensions' 32 among them — runs the form whose idle
// ring steps are skipped by wave-uniform branches.
// TS: the sets form, for a filtered batch (a row set per query).  Three things differ, all behind `if constexpr`, so that an unfiltered batch runs
// the instructions it always ran.  The walk: a wave takes its share of the block's TILE LIST (k_int8_tiles below: the tiles in which some real query
// of the block selects a live row) instead of every tile, and the ring runs on into the next LISTED tile — looked up one entry ahead, so the
// number is there when a tile's last steps need it; an empty list: the block leaves before it copies an operand.  The set words: lane q of a wave
// loads set_q's word of the tile beside the row constants (the block's 64 RowSetRefs sit in LDS behind the operands) and parks it in the wave's
// 512-byte slot — [row block][query], so that the 16 queries of an accumulator block are four 16-byte LDS reads.  Level 1: a pair outside its
// query's set gets kInt8OutOfSet for a score before the block maximum, and an unsure row passes only where one of the block's 16 queries holds
// it; the dump carries the replaced scores and Int8KeepSets reads membership from them.  No out-of-set pair reaches the wave's queue, so the
// flush is the plain one (CandOutT<false>): no set is read per record.
template <int METRIC, int R, bool DIV, bool TS = false>
__global__ void __launch_bounds__(512, 1)
k_int8_filter(IndexView v, const uint4* __restrict__ Q8, const float* __restrict__ sq32, const float* __restrict__ cq, const float* __restrict__ mq, uint32_t nq, uint32_t nq_pad,
              uint32_t* __restrict__ cand_rows, float* __restrict__ cand_score, uint32_t* __restrict__ cand_cnt,
              const uint32_t* __restrict__ tile_list, const uint32_t* __restrict__ tile_cnt /* TS: [blocks][n_tiles] and [blocks], k_int8_tiles */) {
    extern __shared__ __align__(16) unsigned char smem_i8[];
    uint4* s_a = reinterpret_cast<uint4*>(smem_i8);                  // [step][hi, lo][query half][lane]
    __shared__ __align__(16) Int8Lds s_k;
    constexpr bool SETS = false;                                     // the flush never tests a set: a filtered batch (TS) decides membership in its epilogue
    QV_CAND_QUEUE(cqu, 8, 128);                                      // 12 KiB: the query operands take up to 128 KiB of the 160
    QV_EPI_DUMP(du, 8, 16);                                          // 10 KiB
    const uint32_t qb = blockIdx.y;
    if (64 * qb >= nq) return;                                       // a block made only of padding
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t steps = v.dim / 32, chunks = v.dim / 16;
    uint32_t n_list = 0;
    const uint32_t* list = nullptr;
    uint32_t* s_sw = nullptr;                                         // TS: this wave's set words, [row block][query]
    RowSetRef* s_rs = nullptr;                                        // TS: the block's sets (a padded query: an empty one)
    if constexpr (TS) {
        n_list = tile_cnt[qb];
        if (n_list == 0) return;                                     // no tile holds a live row that a query of this block selects
        list = tile_list + (size_t)qb * v.n_tiles;
        s_sw = reinterpret_cast<uint32_t*>(smem_i8 + (size_t)v.dim * 128) + wave * 128;
        s_rs = reinterpret_cast<RowSetRef*>(smem_i8 + (size_t)v.dim * 128 + kInt8SetWordBytes);
        if (threadIdx.x < 64) s_rs[threadIdx.x] = 64 * qb + threadIdx.x < nq ? cand_sets(cand_cnt)[64 * qb + threadIdx.x] : RowSetRef{reinterpret_cast<const uint64_t*>(cand_cnt), 0u, 0u};
    }
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
    const std::conditional_t<TS, Int8KeepSets<METRIC>, Int8Keep<METRIC>> keep{s_k};
    const i32x4* plane = reinterpret_cast<const i32x4*>(v.plane8);
    const uint32_t gw = blockIdx.x * 8 + wave, tw = gridDim.x * 8;
    // TS: `at` walks the list, g_next / g_next2 are the tiles one and two entries ahead (past the end: the last one again)
    const uint32_t n_walk = TS ? n_list : v.n_tiles;
    uint32_t last_at = 0, g_next = 0, g_next2 = 0;
    auto listed = [&](uint32_t at) { return list[at < n_walk ? at : last_at]; };
    if constexpr (TS) if (gw < n_walk) {
        last_at = n_walk - 1 - (n_walk - 1 - gw) % tw;               // the wave's last entry, gw + m tw: in bounds, read by nobody when requested again
        g_next = listed(gw); g_next2 = listed(gw + tw);
    }
    // block j of tile t at step 0: chunk `half` of rows 32 j + l31; a step is two chunks on (128 pieces)
    auto base = [&](uint32_t t, int j) { return plane + ((size_t)t * chunks + half) * 64 + 32 * j + l31; };
    i32x4 rb[R][2];
    bool primed = false;
    for (uint32_t at = gw; at < n_walk; at += tw) {
        uint32_t g, gn;
        if constexpr (TS) { g = g_next; gn = g_next2; g_next = g_next2; g_next2 = listed(at + 2 * tw); }
        else { g = at; gn = g + tw < v.n_tiles ? g + tw : g; }       // past the wave's last tile: the same tile again (in bounds, read by nobody)
        const i32x4* p[2] = {base(g, 0), base(g, 1)};
        const i32x4* np[2] = {base(gn, 0), base(gn, 1)};
        double rnd[2]; float rsc[2], rho[2];
#pragma unroll
        for (int j = 0; j < 2; j++) { const size_t row = (size_t)g * 64 + 32 * j + l31; rnd[j] = v.rnorm[row]; rsc[j] = v.rscale8[row]; rho[j] = v.rres8[row]; }
        const uint64_t alv = v.alive[g];
        uint64_t setw = 0;                                           // TS: word g of set (64 qb + lane)
        if constexpr (TS) {
            const RowSetRef rs = s_rs[lane];
            setw = rs.bits == nullptr ? ~0ull : (g < rs.words ? rs.bits[g] : 0ull);
        }
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
        if constexpr (TS) {
            __threadfence_block();                                   // (the last tile's reads of the slot, before these writes)
            s_sw[lane] = (uint32_t)setw; s_sw[64 + lane] = (uint32_t)(setw >> 32);
            __threadfence_block();
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint32_t row = g * 64 + 32 * j + l31;
            const bool live = (alv >> (32 * j + l31)) & 1ull;
            const float rn = bound_f32_up((float)rnd[j]);
            const bool unsure = int8_filter_row_unsure(rn, rsc[j], rho[j], tiny);
#pragma unroll
            for (int i = 0; i < 2; i++) {
                f16v a;
                uint32_t held = 1u;                                  // TS: some query of this block's 16 holds the row
                if constexpr (TS) {
                    // the 16 queries 32 i + 4 half + (e & 3) + 8 (e >> 2): four runs of four words
                    const uint4* wv = reinterpret_cast<const uint4*>(s_sw + 64 * j + 32 * i + 4 * half);
                    const uint4 w0 = wv[0], w1 = wv[2], w2 = wv[4], w3 = wv[6];
                    const uint32_t w[16] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w, w3.x, w3.y, w3.z, w3.w};
                    const uint32_t bit = 1u << l31;
                    held = 0u;
#pragma unroll
                    for (int e = 0; e < 16; e++) {
                        const uint32_t in = w[e] & bit;
                        held |= in;
                        a[e] = in ? int8_in_set_score(int8_filter_score(acc[0][i][j][e], acc[1][i][j][e], s_k.sq[half][i][e], rsc[j])) : __uint_as_float(kInt8OutOfSet);
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 16; e++) a[e] = int8_filter_score(acc[0][i][j][e], acc[1][i][j][e], s_k.sq[half][i][e], rsc[j]);
                }
                const float m0 = __builtin_fmaxf(__builtin_fmaxf(a[0], a[1]), a[2]), m1 = __builtin_fmaxf(__builtin_fmaxf(a[3], a[4]), a[5]);
                const float m2 = __builtin_fmaxf(__builtin_fmaxf(a[6], a[7]), a[8]), m3 = __builtin_fmaxf(__builtin_fmaxf(a[9], a[10]), a[11]);
                const float m4 = __builtin_fmaxf(__builtin_fmaxf(a[12], a[13]), a[14]);
                const float mx = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(m0, m1), m2), __builtin_fmaxf(__builtin_fmaxf(m3, m4), a[15]));
                // level 1: the threshold is monotone in cm (up), m and b (down), so this is a lower bound of the block's 16 thresholds
                const float thr_lo = int8_filter_threshold<METRIC>(cmin[i], mmax[i], bmax[i], rn, rho[j]);
                const uint64_t pm = __ballot((!(mx < thr_lo) || unsure) && live && (!TS || held != 0u));
                if (__builtin_expect(pm != 0, 0)) epi_dump_with(a, pm, row, rn, rho[j], (uint32_t)i, half, unsure, keep, 64 * qb, cqu, cqu_n, cqu_out, du, n);
            }
        }
        if (n) epi_dense_pass_with(du, n, keep, 64 * qb, cqu, cqu_n, cqu_out);
    }
    cand_flush(cqu, cqu_n, cqu_out);
}

// ---- 1056 to 4096 dimensions (k_int8_wide_filter): the block kernel with its operands passing through LDS in panels ----
// Above 1024 dimensions a block's operands (128 dim bytes: 192 KiB at 1536 dimensions, 512 KiB at 4096) no longer fit LDS, and 128 I_hi + I_lo no
// longer fits int32.  The workgroup is k_int8_filter's — eight waves, one 64-query block, each wave streaming its own 64-row tiles through a ring
// of R = 4 steps into 128 accumulators — and two things change.
// Operands: a tile's steps are cut into revolutions of the ring (R steps, 16 KiB of Q8 in the order the prep wrote them; the last one of a tile
// may be short), and the revolutions of tile after tile — the operands are the same for every tile — form ONE stream that passes through LDS in
// panels of kInt8WideRevs = 4 revolutions (16 steps, 64 KiB).  LDS holds two panels.  While the waves compute revolution n, the workgroup copies
// revolution n + 4 — its place in the next panel — out of L2: every thread loads two 16-byte pieces in front of the revolution's matrix
// instructions and stores them to LDS behind them.  Plain loads and stores, so that the compiler counts them with the ring's (an LDS-DMA request
// it does not see makes every counted wait behind it drain the ring); 8 registers.
// Lockstep: ONE workgroup barrier per panel, in front of its first revolution: the panel's operands are stored, and nobody reads the other panel
// any more, which the next four revolutions overwrite.  Rounds, revolutions and hence barriers are counted from blockIdx.x, gridDim.x and n_tiles
// alone: round r gives wave w tile 8 blockIdx.x + w + 8 gridDim.x r, and a wave whose tile lies past the last one (a workgroup's last round
// only) still walks every revolution of the round, copies its share of the operands and meets every barrier; it skips the row loads, the matrix
// instructions and the epilogue.  No wave leaves the loop before the others.
// DIV, as in k_int8_filter: 4 divides the dimension's steps — every multiple of 128 dimensions — so no step of a revolution is idle and the loop
// body is free of branches; otherwise idle steps are skipped by wave-uniform branches (behind which the compiler drains the ring at every step).
// Score: int8_filter_score_wide (qv_bound.h: the sum in float64, rounded once).  Everything else — row constants, level 1, the dump, the dense
// pass, the queue and its flush — is k_int8_filter's, through the same functions.
constexpr uint32_t kInt8WideMinDim = 1056, kInt8WideMaxDim = 4096;
constexpr int kInt8WideRing = 4, kInt8WideRevs = 4;                   // steps per revolution, revolutions per panel

template <int METRIC, bool DIV>
__global__ void __launch_bounds__(512, 1)
k_int8_wide_filter(IndexView v, const uint4* __restrict__ Q8, const float* __restrict__ sq32, const float* __restrict__ cq, const float* __restrict__ mq, uint32_t nq, uint32_t nq_pad,
                   uint32_t* __restrict__ cand_rows, float* __restrict__ cand_score, uint32_t* __restrict__ cand_cnt) {
    constexpr int R = kInt8WideRing, NREV = kInt8WideRevs;
    constexpr uint32_t kRev = R * 256, kSlots = 2 * NREV;            // 16-byte pieces per revolution; revolutions LDS holds
    static_assert(R * 256 == 2 * 512 && (kSlots & (kSlots - 1)) == 0, "two pieces per thread and revolution; the slots wrap by a mask");
    extern __shared__ __align__(16) unsigned char smem_i8w[];
    uint4* s_a = reinterpret_cast<uint4*>(smem_i8w);                 // [slot][step of the revolution][hi, lo][query half][lane]
    __shared__ __align__(16) Int8Lds s_k;
    constexpr bool SETS = false;
    QV_CAND_QUEUE(cqu, 8, 128);                                      // 12 KiB
    QV_EPI_DUMP(du, 8, 16);                                          // 10 KiB
    const uint32_t qb = blockIdx.y;
    if (64 * qb >= nq) return;                                       // a block made only of padding (the whole workgroup)
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t steps = v.dim / 32, chunks = v.dim / 16;
    const uint32_t revs = (steps + R - 1) / R;                       // revolutions per tile
    // workgroup-uniform: the rounds this workgroup runs — as many as its FIRST wave has tiles
    const uint32_t wg_first = blockIdx.x * 8, tw = gridDim.x * 8;
    if (wg_first >= v.n_tiles) return;                               // (the whole workgroup, before its first barrier)
    const uint32_t rounds = (v.n_tiles - wg_first + tw - 1) / tw;
    const uint4* q8 = Q8 + (size_t)qb * steps * 256;
    const uint32_t q8_last = steps * 256 - 1;                        // (a short revolution's pieces past the operands: the last piece again, into LDS nobody reads)
    // the stream's first panel: revolutions 0 .. NREV - 1 of a tile (revs > NREV: steps >= 33)
    for (uint32_t i = threadIdx.x; i < NREV * kRev; i += 512) s_a[i] = q8[i];
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
    const uint32_t gw = wg_first + wave;
    // block j of tile t at step 0: chunk `half` of rows 32 j + l31; a step is two chunks on (128 pieces)
    auto base = [&](uint32_t t, int j) { return plane + ((size_t)t * chunks + half) * 64 + 32 * j + l31; };
    i32x4 rb[R][2];
    // the stream's cursors (workgroup-uniform): the slot the next revolution is computed from and its place in its panel; the revolution of a
    // tile that is copied next — NREV ahead — and its slot
    uint32_t c_slot = 0, c_in = 0, s_rev = NREV, s_slot = NREV;
    // one round: a tile's revolutions.  ACT: this wave has a tile (wave-uniform, one compiled body each, so that neither holds a conditional load)
    auto round_of = [&](auto act_c, uint32_t g, bool first) {
        constexpr bool ACT = decltype(act_c)::value;
        const uint32_t gn = g + tw < v.n_tiles ? g + tw : g;         // past the wave's last tile: the same tile again (in bounds, read by nobody)
        const i32x4* p[2] = {plane, plane};
        const i32x4* np[2] = {plane, plane};
        double rnd[2] = {0.0, 0.0}; float rsc[2] = {0.f, 0.f}, rho[2] = {0.f, 0.f};
        uint64_t alv = 0;
        i32x16 acc[2][2][2];                                         // [hi, lo][query half][row block]: across the tile's revolutions and panels
        if constexpr (ACT) {
            p[0] = base(g, 0); p[1] = base(g, 1); np[0] = base(gn, 0); np[1] = base(gn, 1);
#pragma unroll
            for (int j = 0; j < 2; j++) { const size_t row = (size_t)g * 64 + 32 * j + l31; rnd[j] = v.rnorm[row]; rsc[j] = v.rscale8[row]; rho[j] = v.rres8[row]; }
            alv = v.alive[g];
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int j = 0; j < 2; j++)
#pragma unroll
                        for (int e = 0; e < 16; e++) acc[t][i][j][e] = 0;
            if (first) {                                             // (steps > R: every slot has a step)
#pragma unroll
                for (int k = 0; k < R; k++) { rb[k][0] = __builtin_nontemporal_load(p[0] + (size_t)k * 128); rb[k][1] = __builtin_nontemporal_load(p[1] + (size_t)k * 128); }
            }
        }
        for (uint32_t rv = 0; rv < revs; rv++) {
            if (c_in == 0) __syncthreads();                          // a panel's first revolution: its operands are stored; the other panel is free
            // revolution s_rev of a tile, for the slot NREV ahead: two pieces per thread (unconditional: past the stream's end they land in LDS nobody reads)
            const uint32_t i0 = s_rev * kRev + threadIdx.x, i1 = i0 + 512;
            const uint4 sg0 = q8[DIV || i0 < q8_last ? i0 : q8_last], sg1 = q8[DIV || i1 < q8_last ? i1 : q8_last];
            if constexpr (ACT) {
                const uint4* pa = s_a + c_slot * kRev + lane;
#pragma unroll
                for (int k = 0; k < R; k++) {
                    const uint32_t s_ = rv * R + k;
                    if (DIV || s_ < steps) {
                        const uint4* ap = pa + k * 256;
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
                        const size_t off = (size_t)(here ? s_ + R : (uint32_t)k) * 128;
                        rb[k][0] = __builtin_nontemporal_load((here ? p[0] : np[0]) + off);
                        rb[k][1] = __builtin_nontemporal_load((here ? p[1] : np[1]) + off);
                    }
                }
            }
            s_a[s_slot * kRev + threadIdx.x] = sg0; s_a[s_slot * kRev + threadIdx.x + 512] = sg1;
            c_slot = (c_slot + 1) & (kSlots - 1); s_slot = (s_slot + 1) & (kSlots - 1);
            c_in = c_in + 1 == (uint32_t)NREV ? 0u : c_in + 1;
            s_rev = s_rev + 1 == revs ? 0u : s_rev + 1;
        }
        if constexpr (ACT) {
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
                    for (int e = 0; e < 16; e++) a[e] = int8_filter_score_wide(acc[0][i][j][e], acc[1][i][j][e], s_k.sq[half][i][e], rsc[j]);
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
    };
    // every wave runs every round of the workgroup; only the last one can find a wave without a tile
    for (uint32_t rd = 0; rd < rounds; rd++) {
        const uint32_t g = gw + rd * tw;
        if (g < v.n_tiles) round_of(std::true_type{}, g, rd == 0);
        else round_of(std::false_type{}, g, false);
    }
    cand_flush(cqu, cqu_n, cqu_out);
}

size_t int8_wide_filter_lds_bytes() { return (size_t)2 * kInt8WideRevs * kInt8WideRing * 4096; }
static hipError_t launch_int8_wide_filter(const IndexView& v, const void* Q8, const float* cq, const float* mq, uint32_t nq, uint32_t nq_pad, uint32_t* cand, float* cscore,
                                          uint32_t* cnt, uint32_t grid_x, size_t lds, hipStream_t s) {
    if (v.rscale8 == nullptr || v.rres8 == nullptr || lds < int8_wide_filter_lds_bytes()) return hipErrorInvalidValue;   // (the rest: launch_int8_filter's guard)
    const dim3 grid(grid_x, nq_pad / 64);
    const uint4* q8 = static_cast<const uint4*>(Q8);
    const float* sq32 = reinterpret_cast<const float*>(static_cast<const char*>(Q8) + (size_t)nq_pad * 2 * v.dim);
    auto go = [&](auto kernel) {
        const hipError_t e = set_lds(kernel, lds); if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, grid, dim3(512), lds, s, v, q8, sq32, cq, mq, nq, nq_pad, cand, cscore, cnt);
        return hipGetLastError();
    };
    const bool div = (v.dim / 32) % kInt8WideRing == 0;
    if (v.metric == QV_COSINE) return div ? go(k_int8_wide_filter<QV_COSINE, true>) : go(k_int8_wide_filter<QV_COSINE, false>);
    return div ? go(k_int8_wide_filter<QV_DOT, true>) : go(k_int8_wide_filter<QV_DOT, false>);
}

size_t int8_filter_lds_bytes(uint32_t dim) { return dim >= kInt8WideMinDim ? int8_wide_filter_lds_bytes() : (size_t)dim * 128; }
size_t int8_filter_sets_lds_bytes(uint32_t dim) { return (size_t)dim * 128 + kInt8SetWordBytes + 64 * sizeof(RowSetRef); }

hipError_t launch_int8_filter(const IndexView& v, const void* Q8, const float* cq, const float* mq, uint32_t nq, uint32_t nq_pad, uint32_t* cand, float* cscore,
                              uint32_t* cnt, uint32_t grid_x, size_t lds, hipStream_t s) {
    if (v.plane8 == nullptr || (v.dim & 31u) || v.dim < 64 || v.dim > kInt8WideMaxDim || (v.metric != QV_COSINE && v.metric != QV_DOT)) return hipErrorInvalidValue;   // (a missing route is an error)
    if (grid_x == 0 || lds < int8_filter_lds_bytes(v.dim)) return hipErrorInvalidValue;
    if (v.dim >= kInt8WideMinDim) return launch_int8_wide_filter(v, Q8, cq, mq, nq, nq_pad, cand, cscore, cnt, grid_x, lds, s);   // 1056 to 4096 dimensions: the panel kernel
    const uint32_t steps = v.dim / 32;
    const dim3 grid(grid_x, nq_pad / 64);                            // (the route's: batched_int8_adapt)
    const uint4* q8 = static_cast<const uint4*>(Q8);
    const float* sq32 = reinterpret_cast<const float*>(static_cast<const char*>(Q8) + (size_t)nq_pad * 2 * v.dim);
    auto go = [&](auto kernel) {
        const hipError_t e = set_lds(kernel, lds); if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, grid, dim3(512), lds, s, v, q8, sq32, cq, mq, nq, nq_pad, cand, cscore, cnt, (const uint32_t*)nullptr, (const uint32_t*)nullptr);
        return hipGetLastError();
    };
    const bool div = steps % kInt8Ring == 0;
    if (v.metric == QV_COSINE) return div ? go(k_int8_filter<QV_COSINE, kInt8Ring, true>) : go(k_int8_filter<QV_COSINE, kInt8Ring, false>);
    return div ? go(k_int8_filter<QV_DOT, kInt8Ring, true>) : go(k_int8_filter<QV_DOT, kInt8Ring, false>);
}

// ---- the sets form's pre-pass (k_int8_tiles): which tiles a 64-query block reads ----
// grid (ceil(n_tiles / 256), blocks that hold a real query), a thread per tile g: cand(g) = alive[g] & OR over the block's real queries of set_q[g]
// (a null set: all ones; words past a set's length: zero).  The loop over the queries is wave-uniform — the table entry is a scalar load — and the
// 64 lanes read consecutive words of ONE bitmap.  A wave reserves its tiles' slots in the block's list with one atomicAdd on the block's count (zeroed
// by k_int8_tiles_clear: no memset node, so that the sequence can be captured) and writes them in lane order; the list's order across waves is whatever
// the atomics give, and no result depends on it.
__global__ void __launch_bounds__(256) k_int8_tiles_clear(uint32_t* __restrict__ tile_cnt, uint32_t blocks) {
    for (uint32_t i = threadIdx.x; i < blocks; i += 256) tile_cnt[i] = 0u;
}
__global__ void __launch_bounds__(256)
k_int8_tiles(const uint64_t* __restrict__ alive, uint32_t n_tiles, const RowSetRef* __restrict__ sets, uint32_t nq, uint32_t* __restrict__ tile_list, uint32_t* __restrict__ tile_cnt) {
    const uint32_t b = blockIdx.y, g = blockIdx.x * 256 + threadIdx.x, lane = lane_id();
    const uint32_t nreal = nq - 64 * b < 64 ? nq - 64 * b : 64u;
    uint64_t any = 0ull;
    if (g < n_tiles) {
        const uint64_t live = alive[g];
        for (uint32_t i = 0; i < nreal && any != ~0ull; i++) {      // (a lane that has seen every bit stops reading)
            const RowSetRef rs = sets[64 * b + i];
            any |= rs.bits == nullptr ? ~0ull : (g < rs.words ? rs.bits[g] : 0ull);
        }
        any &= live;
    }
    const uint64_t m = __ballot(any != 0ull);
    if (m == 0ull) return;                                           // (wave-uniform)
    uint32_t at = 0;
    if (lane == 0) at = atomicAdd(&tile_cnt[b], (uint32_t)__builtin_popcountll(m));
    at = __builtin_amdgcn_readfirstlane(at);
    // (at most one slot per tile is ever reserved: the list's n_tiles words hold them all)
    if (any != 0ull) tile_list[(size_t)b * n_tiles + at + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = g;
}
hipError_t launch_int8_tiles(const IndexView& v, const RowSetRef* d_sets, uint32_t nq, uint32_t* tile_list, uint32_t* tile_cnt, hipStream_t s) {
    const uint32_t blocks = (nq + 63) / 64;
    if (!d_sets || nq == 0 || v.n_tiles == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_int8_tiles_clear, dim3(1), dim3(256), 0, s, tile_cnt, blocks);
    hipLaunchKernelGGL(k_int8_tiles, dim3((v.n_tiles + 255) / 256, blocks), dim3(256), 0, s, v.alive, v.n_tiles, d_sets, nq, tile_list, tile_cnt);
    return hipGetLastError();
}

// the sets form: launch_int8_filter's arguments, the pre-pass's lists and counts; lds: int8_filter_sets_lds_bytes.  The batch's RowSetRef table is the one
// k_mfma_prep left in front of the counters (cand_sets).
hipError_t launch_int8_filter_sets(const IndexView& v, const void* Q8, const float* cq, const float* mq, uint32_t nq, uint32_t nq_pad, uint32_t* cand, float* cscore,
                                   uint32_t* cnt, const uint32_t* tile_list, const uint32_t* tile_cnt, uint32_t grid_x, size_t lds, hipStream_t s) {
    if (v.plane8 == nullptr || (v.dim & 31u) || v.dim < 64 || v.dim > 1024 || (v.metric != QV_COSINE && v.metric != QV_DOT)) return hipErrorInvalidValue;   // (a missing route is an error)
    if (grid_x == 0 || lds < int8_filter_sets_lds_bytes(v.dim) || !tile_list || !tile_cnt) return hipErrorInvalidValue;
    const uint32_t steps = v.dim / 32;
    const dim3 grid(grid_x, (nq + 63) / 64);                         // (the blocks that hold a real query: the pre-pass's)
    const uint4* q8 = static_cast<const uint4*>(Q8);
    const float* sq32 = reinterpret_cast<const float*>(static_cast<const char*>(Q8) + (size_t)nq_pad * 2 * v.dim);
    auto go = [&](auto kernel) {
        const hipError_t e = set_lds(kernel, lds); if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, grid, dim3(512), lds, s, v, q8, sq32, cq, mq, nq, nq_pad, cand, cscore, cnt, tile_list, tile_cnt);
        return hipGetLastError();
    };
    const bool div = steps % kInt8SetsRing == 0;
    if (v.metric == QV_COSINE) return div ? go(k_int8_filter<QV_COSINE, kInt8SetsRing, true, true>) : go(k_int8_filter<QV_COSINE, kInt8SetsRing, false, true>);
    return div ? go(k_int8_filter<QV_DOT, kInt8SetsRing, true, true>) : go(k_int8_filter<QV_DOT, kInt8SetsRing, false, true>);
}

// ---- the shared-row form (k_int8_shared_filter): whole groups of 256 queries, the plane read ONCE per group ----
// k_int8_filter above serves one 64-query block per workgroup, so a batch of four blocks walks the plane four times.  Here a workgroup is four waves,
// one per SIMD, 512 registers each, and serves 256 queries (k_qreg_filter's shape, qv_qreg.hip): wave w keeps the hi and lo operands of queries
// 64 w .. 64 w + 63 of its group for ALL dimensions — four 16-byte A operands per 32-dimension step, 384 registers at 768 dimensions: the first
// ASTEPS steps in the accumulation registers (the matrix instruction is issued from inline assembly and reads them there), the next in vector
// registers, the last LSTEPS in LDS (the valve that keeps the kernel under 512 registers).  k_mfma_prep's operand planes are read as they are: wave w
// of group g takes 64-query block 4 g + w.
// Rows: both 32-row blocks of a tile at once would need 128 accumulators beside the operands, so the unit of work is ONE 32-row block of a tile —
// 64 accumulators, [hi, lo][query half] — and the LDS-DMA gathers exactly that block: lane (half, l31) of a request moves the 16 bytes of chunk
// 2 s + half of row 32 j + l31 (512 contiguous bytes per lane half) and LDS receives them lane after lane, which IS step s's B operand in lane
// order: one conflict-free 16-byte LDS read per step and wave, no LDS byte that is not a row byte of the block in flight.  A stage of the ring is
// four steps of a block (4 KiB), one request per wave; NST stages, requested NST - 1 ahead of their use, ONE barrier per stage (16 matrix
// instructions per wave).  Waits are explicit (qv_lds_dma.h): s_waitcnt vmcnt(NST - 3) for the wave's own request of the NEXT stage, then the
// workgroup barrier for the other waves' — a stage is certified one ahead so that a stage's last step can already read the next one's first operand.
// The row constants (norms, scales, residuals, the alive word: 2 KiB of LDS per tile) travel the same way, two requests per wave in front of a tile's
// first stage, so the epilogue never waits behind the ring; requests the compiler does not see only make the counted waits more conservative.
// Every wave reaches every barrier and issues every request it owes the ring, whatever its queries are (padded queries carry zero operands and
// +inf constants: nothing passes).  Behind a workgroup's last block the cursor requests that block again: in bounds, read by nobody.
// The epilogue is k_int8_filter's, through the same functions, per 32-row block.
constexpr int kI8sStageSteps = 4, kI8sStageBytes = kI8sStageSteps * 1024;
constexpr int kI8sRcTiles = 8, kI8sRcWords = 512;

// A out of the accumulation registers (AG) or a vector register; ZERO: C = 0 (a block's first step).  volatile: the statements stay in the order
// written.  The two wait states in front cover an operand that the vector ALU wrote just before (a copy the register allocator may place there).
template <bool AG, bool ZERO>
__device__ __forceinline__ void mfma_i8(i32x16& acc, const i32x4& a, const i32x4& b) {
    if constexpr (ZERO) {
        if constexpr (AG) asm volatile("s_nop 1\n\tv_mfma_i32_32x32x32_i8 %0, %1, %2, 0" : "=&v"(acc) : "a"(a), "v"(b));
        else asm volatile("s_nop 1\n\tv_mfma_i32_32x32x32_i8 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "v"(b));
    } else {
        if constexpr (AG) asm volatile("s_nop 1\n\tv_mfma_i32_32x32x32_i8 %0, %1, %2, %0" : "+v"(acc) : "a"(a), "v"(b));
        else asm volatile("s_nop 1\n\tv_mfma_i32_32x32x32_i8 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
    }
}

// STEPS: 32-dimension steps (dim = 32 STEPS exactly).  The A operands of steps [0, ASTEPS) live in accumulation registers, of the last LSTEPS steps
// in LDS, of the steps between in vector registers.  NST ring stages.
template <int METRIC, int STEPS, int ASTEPS, int LSTEPS, int NST>
__global__ void __launch_bounds__(256, 1)
k_int8_shared_filter(IndexView v, const uint4* __restrict__ Q8, const float* __restrict__ sq32, const float* __restrict__ cq, const float* __restrict__ mq, uint32_t nq_pad,
                     uint32_t* __restrict__ cand_rows, float* __restrict__ cand_score, uint32_t* __restrict__ cand_cnt) {
    constexpr int NSTG = STEPS / kI8sStageSteps;                     // stages per 32-row block
    constexpr int VSTEPS = STEPS - ASTEPS - LSTEPS, RSTEPS = STEPS - LSTEPS;
    static_assert(STEPS % kI8sStageSteps == 0 && NSTG >= 1 && NST >= 4 && LSTEPS >= 0 && LSTEPS < STEPS && VSTEPS >= 0 && ASTEPS >= 0 && ASTEPS <= 16, "shape");
    // the producer runs at most NST - 1 stages ahead: that many tiles' constants, and one more, must not wrap onto the consumer's
    static_assert((NST - 1) / (2 * NSTG) + 2 <= kI8sRcTiles, "the row constants' ring");
    __shared__ __align__(16) Int8Lds s_k[4];                         // per wave: its 64 queries' constants
    __shared__ __align__(1024) unsigned char s_ring[NST][kI8sStageBytes];
    __shared__ __align__(16) i32x4 s_a[4][LSTEPS > 0 ? LSTEPS : 1][4][64];
    // per tile: norms (64 doubles) in words [0, 128), scales [128, 192), residuals [192, 256), the alive word at 256 + 64 wave (one copy per wave)
    __shared__ __align__(16) uint32_t s_rc[kI8sRcTiles][kI8sRcWords];
    constexpr bool SETS = false;                                     // (a filtered batch never takes this kernel: launch_batched)
    QV_CAND_QUEUE(cqu, 4, 128);                                      // 6 KiB
    QV_EPI_DUMP(du, 4, 16);                                          // 5 KiB
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t groups = nq_pad >> 8;
    const uint32_t stride = gridDim.x / groups;
    // which 256-query group and which tiles: the workgroups that walk the SAME tiles share an XCD's L2 (filter_block_role, qv_filter.h)
    uint32_t qb256, first;
    filter_block_role(groups, qb256, first);
    Int8Lds& kw = s_k[wave];
    {
        const uint32_t ql = lane, q = 256 * qb256 + 64 * wave + ql, w = ql & 31u;
        const float c = cq[q], m = mq[q];
        kw.cm[ql] = int8_filter_cm<METRIC>(c, m); kw.m[ql] = m; kw.b[ql] = mq[nq_pad + q];
        kw.sq[(w >> 2) & 1u][ql >> 5][(w & 3u) | ((w >> 3) << 2)] = sq32[q];   // ql = 32 i + (r & 3) + 8 (r >> 2) + 4 half, inverted
    }
    // the wave's operands: 64-query block 4 qb256 + wave; step s, operand o = 2 {hi, lo} + query half
    i32x4 Aa[ASTEPS > 0 ? ASTEPS : 1][4], Av[VSTEPS > 0 ? VSTEPS : 1][4];
    {
        const i32x4* a = reinterpret_cast<const i32x4*>(Q8) + (size_t)(4 * qb256 + wave) * STEPS * 256 + lane;
#pragma unroll
        for (int s = 0; s < ASTEPS; s++)
#pragma unroll
            for (int o = 0; o < 4; o++) Aa[s][o] = a[(size_t)(s * 4 + o) * 64];
#pragma unroll
        for (int s = 0; s < VSTEPS; s++)
#pragma unroll
            for (int o = 0; o < 4; o++) Av[s][o] = a[(size_t)((ASTEPS + s) * 4 + o) * 64];
#pragma unroll
        for (int s = 0; s < LSTEPS; s++)
#pragma unroll
            for (int o = 0; o < 4; o++) s_a[wave][s][o][lane] = a[(size_t)((RSTEPS + s) * 4 + o) * 64];
    }
    // every operand is "used" here, so that the compiler waits for these loads HERE and not — with vmcnt(0), the whole ring drained — at their
    // first use inside the loop
#pragma unroll
    for (int s = 0; s < ASTEPS; s++) { asm volatile("" :: "a"(Aa[s][0]), "a"(Aa[s][1]), "a"(Aa[s][2]), "a"(Aa[s][3])); }
#pragma unroll
    for (int s = 0; s < VSTEPS; s++) { asm volatile("" :: "v"(Av[s][0]), "v"(Av[s][1]), "v"(Av[s][2]), "v"(Av[s][3])); }
    __syncthreads();
    if (stride == 0 || first >= v.n_tiles) return;                   // (the whole workgroup)
    const uint32_t n_half = 2 * ((v.n_tiles - first + stride - 1) / stride);   // the 32-row blocks this workgroup walks
    const uint32_t half = lane >> 5, l31 = lane & 31;
    float cmin[2], mmax[2], bmax[2];                                 // per query half: what bounds the 16 thresholds of this lane's accumulators from below
#pragma unroll
    for (int i = 0; i < 2; i++) {
        float cm = __builtin_inff(), mm = 0.f, bm = 0.f;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const uint32_t ql = 32 * i + (r & 3) + 8 * (r >> 2) + 4 * half;
            cm = fminf(cm, kw.cm[ql]); mm = fmaxf(mm, kw.m[ql]); bm = fmaxf(bm, kw.b[ql]);
        }
        cmin[i] = cm; mmax[i] = mm; bmax[i] = bm;
    }
    const float tiny = filter_tiny_norm(v.dim);
    const Int8Keep<METRIC> keep{kw};
    const uint32_t qglobal = 256 * qb256 + 64 * wave;
    const uint32_t ring_addr = (uint32_t)(size_t)(qlds_u8*)&s_ring[0][0];
    const uint32_t rc_addr = (uint32_t)(size_t)(qlds_u8*)&s_rc[0][0];
    const uint32_t lane16 = lane * 16;
    const uint32_t lane_goff = half * 1024 + l31 * 16;               // chunk `half` of the step, row l31 of the block
    constexpr size_t tile_bytes = (size_t)STEPS * 2048;
    const unsigned char* plane = reinterpret_cast<const unsigned char*>(v.plane8);
    const unsigned char* rc_base = wave < 2 ? reinterpret_cast<const unsigned char*>(v.rnorm) + 256 * wave
                                 : (wave == 2 ? reinterpret_cast<const unsigned char*>(v.rscale8) : reinterpret_cast<const unsigned char*>(v.rres8));
    const uint32_t rc_mul = wave < 2 ? 512u : 256u;                  // bytes per tile in this wave's array
    // producer cursor: block p_h of this workgroup's sequence (tile p_h / 2, row block p_h & 1), stage p_s of it, ring slot p_slot
    uint32_t p_h = 0, p_s = 0, p_slot = 0;
    auto request_stage = [&]() {
        const uint32_t ph = p_h < n_half ? p_h : n_half - 1;         // past the end: the last block again (lands in a slot nobody reads)
        const uint32_t t = first + (ph >> 1) * stride;
        if (p_s == 0 && (p_h & 1u) == 0) {                           // a tile's constants, in front of its first stage
            const uint32_t dst = rc_addr + ((p_h >> 1) & (kI8sRcTiles - 1)) * (kI8sRcWords * 4) + 256 * wave;
            dma_words(rc_base + (size_t)t * rc_mul, lane * 4, dst);
            dma_words(reinterpret_cast<const unsigned char*>(v.alive) + (size_t)t * 8, (lane & 1u) * 4, dst + 1024);
        }
        dma_piece<0>(plane + (size_t)t * tile_bytes + (size_t)(kI8sStageSteps * p_s + wave) * 2048 + (ph & 1u) * 512, lane_goff, ring_addr + p_slot * kI8sStageBytes + 1024 * wave);
        p_s++; if (p_s == (uint32_t)NSTG) { p_s = 0; p_h++; }
        p_slot++; if (p_slot == (uint32_t)NST) p_slot = 0;
    };
#pragma unroll
    for (int i = 0; i < NST - 1; i++) request_stage();
    wait_vmcnt<NST - 2>();
    __syncthreads();                                                 // the first stage is there
    uint32_t c_slot = 0;
    for (uint32_t hi = 0; hi < n_half; hi++) {
        const uint32_t t = first + (hi >> 1) * stride, j = hi & 1u;
        i32x16 acc[2][2];                                            // [hi, lo][query half]
        i32x4 b[2];                                                  // this step's B operand and the next one's
        i32x4 al[4];                                                 // a step's A operands out of LDS (the last LSTEPS steps)
#pragma unroll
        for (int st = 0; st < NSTG; st++) {
            wait_vmcnt<NST - 3>();                                   // this wave's request of the NEXT stage has landed
            __syncthreads();                                         // ... and everybody's; the slot consumed before this one is free
            const uint32_t slot1 = c_slot + 1 == (uint32_t)NST ? 0u : c_slot + 1;
            const unsigned char* sp = &s_ring[0][0] + c_slot * kI8sStageBytes + lane16;
            const unsigned char* sp1 = &s_ring[0][0] + slot1 * kI8sStageBytes + lane16;
            if (st == 0) b[0] = *reinterpret_cast<const i32x4*>(sp);  // (once per block: the epilogue carries no operand across)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < kI8sStageSteps; s++) {
                const int gs = st * kI8sStageSteps + s;
                const bool has_next = gs + 1 < STEPS;
                const unsigned char* np = s + 1 < kI8sStageSteps ? sp + (s + 1) * 1024 : sp1;
                const bool ag = gs < ASTEPS, lds_a = gs >= RSTEPS, lds_an = gs + 1 >= RSTEPS && gs + 1 < STEPS;
                const int ln = gs + 1 - RSTEPS >= 0 && lds_an ? gs + 1 - RSTEPS : 0;
                const i32x4& bb = b[gs & 1];
#define QV_I8_A(O) (ag ? Aa[ag ? gs : 0][O] : (lds_a ? al[O] : Av[!ag && !lds_a ? gs - ASTEPS : 0][O]))
#define QV_I8_MF(ACC, O) { if (gs == 0) { if (ag) mfma_i8<true, true>(ACC, QV_I8_A(O), bb); else mfma_i8<false, true>(ACC, QV_I8_A(O), bb); } \
                           else if (ag) mfma_i8<true, false>(ACC, QV_I8_A(O), bb); else mfma_i8<false, false>(ACC, QV_I8_A(O), bb); }
                QV_I8_MF(acc[0][0], 0)
                if (has_next) b[(gs + 1) & 1] = *reinterpret_cast<const i32x4*>(np);   // the next step's operand is requested
                if (lds_an) al[0] = s_a[wave][ln][0][lane];
                __builtin_amdgcn_sched_barrier(0);
                QV_I8_MF(acc[0][1], 1)
                if (s == 1) request_stage();                         // one row request per stage and wave
                if (lds_an) al[1] = s_a[wave][ln][1][lane];
                __builtin_amdgcn_sched_barrier(0);
                QV_I8_MF(acc[1][0], 2)
                if (lds_an) al[2] = s_a[wave][ln][2][lane];
                __builtin_amdgcn_sched_barrier(0);
                QV_I8_MF(acc[1][1], 3)
                if (lds_an) al[3] = s_a[wave][ln][3][lane];
                __builtin_amdgcn_sched_barrier(0);
#undef QV_I8_MF
#undef QV_I8_A
            }
            c_slot = slot1;
        }
        const uint32_t* rc = s_rc[(hi >> 1) & (kI8sRcTiles - 1)];
        const double rnd = *reinterpret_cast<const double*>(rc + 2 * (32 * j + l31));
        const float rsc = __uint_as_float(rc[128 + 32 * j + l31]), rho = __uint_as_float(rc[192 + 32 * j + l31]);
        const uint64_t alv = *reinterpret_cast<const uint64_t*>(rc + 256 + 64 * wave);
        // the last matrix instructions' results, before vector instructions read them (20 wait states; the statement names the accumulators so
        // that nothing that reads them is scheduled ahead of it)
        asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[1][0]), "+v"(acc[1][1]));
        const uint32_t row = t * 64 + 32 * j + l31;
        const bool live = (alv >> (32 * j + l31)) & 1ull;
        const float rn = bound_f32_up((float)rnd);
        const bool unsure = int8_filter_row_unsure(rn, rsc, rho, tiny);
        uint32_t n = 0;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            f16v a;
#pragma unroll
            for (int e = 0; e < 16; e++) a[e] = int8_filter_score(acc[0][i][e], acc[1][i][e], kw.sq[half][i][e], rsc);
            const float m0 = __builtin_fmaxf(__builtin_fmaxf(a[0], a[1]), a[2]), m1 = __builtin_fmaxf(__builtin_fmaxf(a[3], a[4]), a[5]);
            const float m2 = __builtin_fmaxf(__builtin_fmaxf(a[6], a[7]), a[8]), m3 = __builtin_fmaxf(__builtin_fmaxf(a[9], a[10]), a[11]);
            const float m4 = __builtin_fmaxf(__builtin_fmaxf(a[12], a[13]), a[14]);
            const float mx = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(m0, m1), m2), __builtin_fmaxf(__builtin_fmaxf(m3, m4), a[15]));
            // level 1: the threshold is monotone in cm (up), m and b (down), so this is a lower bound of the block's 16 thresholds
            const float thr_lo = int8_filter_threshold<METRIC>(cmin[i], mmax[i], bmax[i], rn, rho);
            const uint64_t pm = __ballot((!(mx < thr_lo) || unsure) && live);
            if (__builtin_expect(pm != 0, 0)) epi_dump_with(a, pm, row, rn, rho, (uint32_t)i, half, unsure, keep, qglobal, cqu, cqu_n, cqu_out, du, n);
        }
        if (n) epi_dense_pass_with(du, n, keep, qglobal, cqu, cqu_n, cqu_out);
    }
    wait_vmcnt<0>();                                                 // the requests past the end, before the workgroup's LDS is released
    cand_flush(cqu, cqu_n, cqu_out);
}

// Which dimensions have an instantiation: 128, 384, 512 and 768 (<STEPS, in accumulation registers, in LDS, ring stages>; 768 dimensions keep 16
// steps' operands in the 256 accumulation registers, 6 in vector registers and 2 in LDS — profiles/int8_shared_resources.txt).  Every other
// dimension the int8 filter serves keeps k_int8_filter; 800 - 1024 in any case: their operands do not fit.
bool int8_shared_has_dim(uint32_t dim) { return dim == 128 || dim == 384 || dim == 512 || dim == 768; }

hipError_t launch_int8_shared_filter(const IndexView& v, const void* Q8, const float* cq, const float* mq, uint32_t nq_pad, uint32_t* cand, float* cscore, uint32_t* cnt,
                                     uint32_t grid, hipStream_t s) {
    const uint32_t groups = nq_pad >> 8;
    if (v.plane8 == nullptr || v.rscale8 == nullptr || v.rres8 == nullptr || !int8_shared_has_dim(v.dim) || (v.metric != QV_COSINE && v.metric != QV_DOT)) return hipErrorInvalidValue;   // (a missing route is an error)
    if (groups == 0 || (nq_pad & 255u) || grid == 0 || grid % groups) return hipErrorInvalidValue;
    const uint4* q8 = static_cast<const uint4*>(Q8);
    const float* sq32 = reinterpret_cast<const float*>(static_cast<const char*>(Q8) + (size_t)nq_pad * 2 * v.dim);
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, v, q8, sq32, cq, mq, nq_pad, cand, cscore, cnt);
        return hipGetLastError();
    };
    auto by_dim = [&](auto m) {
        constexpr int M = decltype(m)::value;
        switch (v.dim) {
            case 128: return go(k_int8_shared_filter<M, 4, 4, 0, 8>);
            case 384: return go(k_int8_shared_filter<M, 12, 12, 0, 12>);
            case 512: return go(k_int8_shared_filter<M, 16, 16, 0, 16>);
            default:  return go(k_int8_shared_filter<M, 24, 16, QV_INT8_SHARED_LSTEPS, 16>);
        }
    };
    return v.metric == QV_COSINE ? by_dim(std::integral_constant<int, QV_COSINE>{}) : by_dim(std::integral_constant<int, QV_DOT>{});
}

// the batch's counters, behind its last kernel: batches, queries, queries handed back (their redo flags)
// shared: the main filter was the shared-row form — counted in its own words too, so that kInt8FilterStatsWord's count BOTH forms
__global__ void __launch_bounds__(256) k_int8_filter_count(const uint32_t* __restrict__ redo, uint32_t nq, uint32_t* __restrict__ stats, uint32_t shared) {
    uint32_t n = 0;
    for (uint32_t q = threadIdx.x; q < nq; q += 256) n += redo[q] ? 1u : 0u;
    if (n) (void)atomicAdd(&stats[kInt8FilterStatsWord + 2], n);
    if (threadIdx.x == 0) { (void)atomicAdd(&stats[kInt8FilterStatsWord], 1u); (void)atomicAdd(&stats[kInt8FilterStatsWord + 1], nq); }
    if (threadIdx.x == 0 && shared) { (void)atomicAdd(&stats[kInt8SharedStatsWord], 1u); (void)atomicAdd(&stats[kInt8SharedStatsWord + 1], nq); }
}
hipError_t launch_int8_filter_count(const uint32_t* d_redo, uint32_t nq, uint32_t* d_stats, bool shared, hipStream_t s) {
    hipLaunchKernelGGL(k_int8_filter_count, dim3(1), dim3(256), 0, s, d_redo, nq, d_stats, shared ? 1u : 0u);
    return hipGetLastError();
}

// ... and a filtered batch's own (kInt8FilteredStatsWord): batches, queries, and — 64-bit, summed here from the lists' counts — the (block, tile)
// visits the lists skipped and those possible (blocks with a real query x n_tiles)
__global__ void __launch_bounds__(256) k_int8_filtered_count(const uint32_t* __restrict__ tile_cnt, uint32_t blocks, uint32_t n_tiles, uint32_t nq, uint32_t* __restrict__ stats) {
    unsigned long long skipped = 0ull;
    for (uint32_t b = threadIdx.x; b < blocks; b += 256) skipped += n_tiles - tile_cnt[b];
    unsigned long long* wide = reinterpret_cast<unsigned long long*>(stats + kInt8FilteredStatsWord + 2);
    if (skipped) (void)atomicAdd(&wide[0], skipped);
    if (threadIdx.x == 0) {
        (void)atomicAdd(&stats[kInt8FilteredStatsWord], 1u); (void)atomicAdd(&stats[kInt8FilteredStatsWord + 1], nq);
        (void)atomicAdd(&wide[1], (unsigned long long)blocks * n_tiles);
    }
}
hipError_t launch_int8_filtered_count(const uint32_t* tile_cnt, uint32_t nq, uint32_t n_tiles, uint32_t* d_stats, hipStream_t s) {
    hipLaunchKernelGGL(k_int8_filtered_count, dim3(1), dim3(256), 0, s, tile_cnt, (nq + 63) / 64, n_tiles, nq, d_stats);
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
        // (the score as the dimension's kernel forms it: above 1024 dimensions the sum leaves int32)
        const float score = dim >= kInt8WideFromDim ? int8_filter_score_wide(isum_hi, isum_lo, kc.sq32, rscale8) : int8_filter_score(isum_hi, isum_lo, kc.sq32, rscale8);
        return int8_filter_keeps<M>(score, int8_filter_cm<M>(kc.c, kc.m), kc.m, kc.b, rnf, rres8, unsure) ? 1 : 0;
    };
    return metric == QV_COSINE ? f(std::integral_constant<int, QV_COSINE>{}) : f(std::integral_constant<int, QV_DOT>{});
}

}  // namespace qv
