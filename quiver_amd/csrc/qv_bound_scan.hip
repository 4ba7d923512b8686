// qv_bound_scan.hip — the bound scan: a fused flat search (k <= 64; cosine, dot, or a Euclidean index created with QV_FLAG_L2_SCAN_PLANE) answered from the index's reduced copies of the rows — the
// bfloat16 copy, with the 8-bit plane in front of it for one query and for a shared pass of 2 - 8, each unfiltered or filtered — by rejecting
// rows on a certified interval of the distance (qv_bound.h) and re-scoring the few survivors in the exact scan's arithmetic.  One query, the shared
// pass of 2 - 8, their filtered forms; the wide form of one query, unfiltered or over a candidate bitmap, for 65 to 1024 results
// (bound_scan_tail_wide, k_bound_collect_wide, k_bound_rescore_wide, launch_bound_scan_wide);
// the rules that say when each applies; the launchers and workspace sizes; the interval and the 8-bit row state compiled for the host.
// Which search takes the path is decided by plan_flat (qv_scan.hip); the exact scan that answers what a bound pass hands back
// (k_flat_scan<., ., true> behind its gate, launch_flat_redo_flagged) and the list merge (launch_merge_lists) live there too.
#include "qv_kernels.h"
#include "qv_bound.h"
#include <stdio.h>

namespace qv {

// ---------------------------------------------------------------- one query over a large corpus: reject rows on the bfloat16 copy --
// k_flat_scan runs at the memory's rate (0.90 of the HBM peak at 10M x 768), so a single query gets faster only by reading fewer
// bytes.  Of N rows k are returned; the others only have to be REJECTED, and that takes a certified lower bound of the distance,
// not the float64 chain.  Three launches and the gated exact scan behind them:
//   k_bound_scan     k_flat_scan's shape — lane == row, a wave owns whole tiles — over the index's bfloat16 copy (IndexView::plane: half
//                    the bytes; per 16-dimension step a lane reads its two 16-byte halves, the wave two contiguous 512-byte runs per
//                    request), the query in float32 from LDS, one float32 fma chain S~ per row, and from it the interval [d_lo, d_hi]
//                    of the reference's float32 distance (qv_bound.h).  d_lo goes out as one ordered word per row (4 bytes against the
//                    row's 2 dim); the UPPER bounds go through k_flat_scan's own selection — wave lists, the workgroups' lists published,
//                    the last workgroup merges — so the launch ends with H, the exact k-th smallest upper bound over all live rows.
//                    Any k rows' upper bounds cap the k-th distance: every row of the answer has d_lo <= H.
//   k_bound_collect  the rows with d_lo <= H (not strict: ties go on) — k plus a handful on ordinary data — gathered per workgroup in LDS and
//                    listed with one returning atomic per workgroup and flush (bound_collect); the list's order is not defined.
//   k_bound_rescore  a wave per survivor on a small fixed grid: each row requested whole, then walked as ONE float64 chain — row_accumulate's
//                    chain + finalize, the query's norm as its chain: the exact scan's bits —, the last workgroup merges the lists and writes
//                    the k best (distance, row) keys where the exact scan writes them.  When the list overflowed, H is not finite (fewer than k rows with a bound), or |q| is not a norm
//                    the bound works with, it sets the gate word instead and the exact scan launched behind it answers
//                    (k_flat_scan<., ., true>'s `gate`: otherwise that launch leaves at once).  Nothing is read on the host.
// (Measured first and not kept: candidates taken DURING the scan against a device-wide threshold word seeded from the waves' first
// tiles — the tiles walked before the seed's merge lands let 20 - 50 k rows through at k = 64; profiles/LAB_r07_bound_scan.md.)
// The control words live in the stream's zeroed ticket words and are left zero.
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kBoundCandCap = 4096;       // rows stage 3 walks exactly (an i.i.d. 10M x 768 corpus leaves k + a few)
constexpr uint32_t kBoundMaxDim = 4096;
struct BoundCtrl { uint32_t thr_inv, cand_cnt, ticket, flag; };   // thr_inv = ~(ordered image of H): zero = no finite H
struct BoundQuery8 { double sq, qn, qres, pad; int8_t terms[2 * kBoundMaxDim]; };   // bound8_stage_query's results (the 6-bit stage leaves them in the workspace): [dim] hi terms, [dim] lo terms

template <int U, bool QN>
__device__ __forceinline__ void bound_block(const u4* __restrict__ p, const float* __restrict__ q_lds, uint32_t s0, float& acc, double& qa) {
    u4 x[2 * U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        x[2 * u] = __builtin_nontemporal_load(&p[(size_t)(s0 + u) * 128]);
        x[2 * u + 1] = __builtin_nontemporal_load(&p[(size_t)(s0 + u) * 128 + 32]);
    }
    __builtin_amdgcn_sched_barrier(0);                                 // all requests of the block ahead of the arithmetic (see row_accumulate)
#pragma unroll
    for (int u = 0; u < U; u++) {
        const f4* qq = reinterpret_cast<const f4*>(q_lds + (size_t)(s0 + u) * 16);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const u4 w = x[2 * u + h];
            const f4 qa4 = qq[2 * h], qb4 = qq[2 * h + 1];
            const float qe[8] = {qa4.x, qa4.y, qa4.z, qa4.w, qb4.x, qb4.y, qb4.z, qb4.w};
            const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {                              // bfloat16 -> float32 is a shift / a mask: exact
                acc = __builtin_fmaf(qe[2 * j], __uint_as_float(ww[j] << 16), acc);
                acc = __builtin_fmaf(qe[2 * j + 1], __uint_as_float(ww[j] & 0xFFFF0000u), acc);
                if constexpr (QN) { const double a = (double)qe[2 * j], b = (double)qe[2 * j + 1]; qa = __builtin_fma(a, a, qa); qa = __builtin_fma(b, b, qa); }
            }
        }
    }
}
// S~ of this lane's row of one tile (p = the tile in the copy + the lane's place in a step); QN: |q|^2 as the reference's chain rides along
template <bool QN>
__device__ __forceinline__ float bound_tile(const u4* __restrict__ p, const float* __restrict__ q_lds, uint32_t steps, double* qn2) {
    float acc = 0.f; double qa = 0.0;
    uint32_t s = 0;
    for (; s + 8 <= steps; s += 8) bound_block<8, QN>(p, q_lds, s, acc, qa);
    if (s + 4 <= steps) { bound_block<4, QN>(p, q_lds, s, acc, qa); s += 4; }
    if (s + 2 <= steps) { bound_block<2, QN>(p, q_lds, s, acc, qa); s += 2; }
    if (s < steps) bound_block<1, QN>(p, q_lds, s, acc, qa);
    if constexpr (QN) *qn2 = qa;
    return acc;
}

// The end of a bound scan's stage 1 (k_bound_scan, k_bound_scan8): the upper bounds' lists go waves -> wave 0 -> published; the last workgroup
// to finish merges (k_flat_scan<., ., true>'s protocol) and leaves H, the exact k-th smallest upper bound, in the control words.
// true: this workgroup was the last (every other one has taken its ticket, so has read whatever it reads of the control words).
__device__ __forceinline__ bool bound_scan_tail(uint64_t list, uint64_t thr, uint64_t* wl /* LDS [kScanWaves][64] */, uint32_t wave, uint32_t lane, uint32_t k, BoundCtrl* __restrict__ ctrl,
                                                uint64_t* __restrict__ partial, uint32_t* __restrict__ seed_rows, float* __restrict__ seed_dist) {
    __shared__ uint32_t s_last;
    const uint32_t kth = k - 1;
    wl[wave * 64 + lane] = list;
    __syncthreads();
    if (wave == 0) {
        for (uint32_t w = 1; w < kScanWaves; w++) list_insert(list, thr, lane < k ? wl[w * 64 + lane] : kDeadKey, kth, lane);
        uint64_t* mine = partial + (size_t)blockIdx.x * k;
        if (lane < k) (void)atomicExch(reinterpret_cast<unsigned long long*>(&mine[lane]), (unsigned long long)list);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // every lane's exchange has returned: the list is at the memory side
        uint32_t last = 0;
        if (lane == 0) last = atomicAdd(&ctrl->ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
        last = __builtin_amdgcn_readfirstlane(last);
        if (last && lane == 0) ctrl->ticket = 0;                       // for the next launch on these words (stream order)
        if (lane == 0) s_last = last;
    }
    __syncthreads();
    if (!s_last) return false;
    merge_lists_last_workgroup(partial, gridDim.x, k, seed_rows, seed_dist);
    if (wave == 0 && lane == kth) {                                    // (this lane wrote them) H: a finite k-th upper bound, or none
        const uint32_t o = ord_f32(seed_dist[kth]);
        ctrl->thr_inv = (seed_rows[kth] != 0xFFFFFFFFu && o < 0xFF800000u) ? ~o : 0u;
        ctrl->cand_cnt = 0;
    }
    return true;
}

// The WIDE form's tail (k_bound_scan<., ., true>, k_bound_scan8<., ., true>: one query, 65 <= k <= kBoundWideMaxK; under SKIP "live" below reads
// "candidate": v.alive is the call's candidate bitmap).  The
// scan runs with a list length of 64, so a wave ends holding the 64 smallest upper bounds of ITS rows, and every wave's list is published as
// it stands — [grid][kScanWaves][64] keys, dead keys where a wave saw fewer than 64 live rows — without a merge down to k: the in-wave list
// and merge_lists_last_workgroup hold 64 keys and do not stretch to 1024.  H is then the k-th smallest key of the UNION of the published
// lists (launch_select_topk behind this launch; k_bound_collect_wide reads its k-th output).
//   Certified: the published keys are upper bounds of k DISTINCT live rows (a row is in one wave's list only), and any k live rows' upper
//   bounds cap the k-th distance — the k-th smallest distance is at most the largest of any k rows' distances, each at most its upper
//   bound.  So every row of the answer has d_lo <= d <= H.
//   Exact where it can be: the k smallest upper bounds overall are all published whenever no single wave holds more than 64 of them — a
//   wave drops only keys larger than its own 64 smallest —, and then H IS the k-th smallest upper bound, the H the k <= 64 form computes.
//   When one wave's rows hold more than 64 of the k smallest (the nearest rows stored together in tiles of one wave), the dropped ones are
//   replaced by larger published keys: H is only LOOSER, never too small, and the collect passes a few more rows on.
//   Fewer than k published live keys (fewer than k rows the bound is sure of): the k-th key is dead, there is no H, the search is handed on.
// No ticket, no last workgroup: every slot of `lists` is written by its own wave in every launch (the workspace is reused) — a wave that
// walks no tile, or under SKIP reads none, arrives with the dead list it started with and publishes that.
__device__ __forceinline__ void bound_scan_tail_wide(uint64_t list, uint32_t wave, uint32_t lane, uint64_t* __restrict__ lists /* [grid][kScanWaves][64] */) {
    lists[((size_t)blockIdx.x * kScanWaves + wave) * 64 + lane] = list;
}

// SKIP (k_bound_scan<., true>: v.alive is a filter's candidate bitmap, alive & set — k_rowset_and's or the masked upload): a tile whose word is
// zero is not requested, neither its copy nor rnorm nor rres.  Its 64 lower-bound words are WRITTEN as 0xFFFFFFFF all the same: k_bound_collect
// reads every word and the workspace is reused, so an unwritten tile would hold an earlier search's bounds; 256 bytes stored against dim * 128
// bytes not read, and the collect stays as it is.  |q|^2 rides along the first tile the wave READS; a wave that reads none publishes a dead list.
template <int M, bool SKIP = false, bool WIDE = false /* k = 64 is the list length; the tail publishes the waves' lists (bound_scan_tail_wide) */>
__global__ void __launch_bounds__(kScanBlock)
k_bound_scan(IndexView v, const float* __restrict__ query, uint32_t k, BoundCtrl* __restrict__ ctrl, uint32_t* __restrict__ lo_all /* [n_tiles * 64] */,
             uint64_t* __restrict__ partial /* [grid][k] */, uint32_t* __restrict__ seed_rows, float* __restrict__ seed_dist,
             const uint32_t* __restrict__ gate = nullptr /* behind the 8-bit stage (k_bound_rescore<., true> wrote the word): zero = it has answered, leave at once */) {
    if (gate != nullptr && *gate == 0u) return;
    extern __shared__ __align__(16) unsigned char smem[];
    float* q_lds = reinterpret_cast<float*>(smem);                     // [dim], dim a multiple of 16
    uint64_t* wl = reinterpret_cast<uint64_t*>(smem + (size_t)v.dim * sizeof(float));   // [kScanWaves][64]
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t i = threadIdx.x; i < v.dim; i += blockDim.x) q_lds[i] = query[i];
    __syncthreads();
    const uint32_t steps = v.dim >> 4, tw = gridDim.x * kScanWaves, kth = k - 1;
    const double gamma = bound_scan_gamma(v.dim);
    const u4* plane = reinterpret_cast<const u4*>(v.plane) + ((lane >> 5) * 64 + (lane & 31));
    uint64_t list = kDeadKey, thr = kDeadKey;
    double qn = 0.0;

    uint64_t am_read = 0ull;                                           // (SKIP) the word of the tile being walked
    auto finish_tile = [&](uint32_t t, float s, bool first) {
        const uint32_t row = t * 64 + lane;
        const double rn = v.rnorm[row];
        const float rr = v.rres[row];
        uint64_t am;                                                   // wave-uniform
        if constexpr (SKIP) am = am_read; else am = v.alive[t];
        float lo, hi;
        (void)bound_scan_interval<M>(s, qn, rn, rr, v.dim, gamma, lo, hi);
        const bool live = (am >> lane) & 1ull;                         // (dead rows and the last tile's padding: never candidates, never in a bound)
        __builtin_nontemporal_store(live ? ord_f32(lo) : 0xFFFFFFFFu, &lo_all[row]);
        const uint64_t key = live ? (((uint64_t)ord_f32(hi) << 32) | row) : kDeadKey;
        if (first) { list = wave_sort64(key, lane); thr = readlane64(list, kth); }
        else list_insert(list, thr, key, kth, lane);
    };

    uint32_t t = blockIdx.x * kScanWaves + wave;
    if constexpr (SKIP) {
        bool first = true;
        uint64_t am_next = t < v.n_tiles ? v.alive[t] : 0ull;
        for (; t < v.n_tiles; t += tw) {
            const uint64_t am = am_next;
            if (t + tw < v.n_tiles) am_next = v.alive[t + tw];         // (the next tile's word: in flight behind this tile's rows)
            if (am == 0ull) { __builtin_nontemporal_store(0xFFFFFFFFu, &lo_all[t * 64 + lane]); continue; }
            am_read = am;
            if (first) {
                double qn2 = 0.0;
                const float s = bound_tile<true>(plane + (size_t)t * steps * 128, q_lds, steps, &qn2);
                qn = __builtin_sqrt(qn2);
                finish_tile(t, s, true);
                first = false;
            } else finish_tile(t, bound_tile<false>(plane + (size_t)t * steps * 128, q_lds, steps, nullptr), false);
        }
    } else {
        if (t < v.n_tiles) {                                           // first tile: sorted outright, |q| rides along
            double qn2 = 0.0;
            const float s = bound_tile<true>(plane + (size_t)t * steps * 128, q_lds, steps, &qn2);
            qn = __builtin_sqrt(qn2);
            finish_tile(t, s, true);
            t += tw;
        }
        for (; t < v.n_tiles; t += tw) finish_tile(t, bound_tile<false>(plane + (size_t)t * steps * 128, q_lds, steps, nullptr), false);
    }

    if constexpr (WIDE) bound_scan_tail_wide(list, wave, lane, partial);
    else (void)bound_scan_tail(list, thr, wl, wave, lane, k, ctrl, partial, seed_rows, seed_dist);
}

// the rows with d_lo <= H, eight per thread and step, a chunk of 2048 words per workgroup and step (lo: one query's ordered words; cnt: its
// counter; cand: its list).  cap: the list's capacity (the count goes on past it by the full number: the stage behind reads the overflow from
// it); ids: lo is a compact array and ids[i] the row behind entry i (k_bound_refine8's), null: entry i is row i.
// The slots are reserved per WORKGROUP: a wave counts its chunk's candidates by ballot, its leader reserves in an LDS counter, the lanes put
// their rows into an LDS buffer of a chunk and a half; when the next chunk could overflow it, and once more at the end of the walk, thread 0 takes ONE
// returning atomicAdd(cnt, fill) and the workgroup copies its rows to cand[base .. base + fill), below cap only.  (One returning atomic per
// wave and batch on the one counter word was 10 ns per candidate, all serialised: 59 us for 6 089 candidates of 10M rows, 18 us this
// way; profiles/LAB_r22_bound_collect.md.)  The buffer holds entry numbers; the compact form's indirection is applied at the flush.  A chunk's trip count is uniform over the workgroup: one barrier per chunk, two more per
// flush.  No workgroup waits for another; the ORDER of the rows in the list is whatever the reservations make it, and nothing behind depends
// on it.  The next chunk's words are requested before this one's are looked at.
constexpr uint32_t kCollectVecs = 2;           // 16-byte requests of a thread per chunk, 1024 words apart
constexpr uint32_t kCollectChunk = kCollectVecs * 1024;   // words a workgroup looks at per step (256 threads x 4 x kCollectVecs): half the barriers and twice the bytes in flight of one request each
constexpr uint32_t kCollectBuf = kCollectChunk + kCollectChunk / 2;   // rows gathered between two reservations (12 KiB of LDS): flushed once it is over a third full
#ifndef QV_COLLECT_GRID
#define QV_COLLECT_GRID 512u                   // workgroups at most: 40 MB of 10M rows in 17.9 us, 256: 23.8, 1024: 20.2 (profiles/LAB_r22_bound_collect.md)
#endif
constexpr uint32_t kBoundCollectGrid = QV_COLLECT_GRID;
__device__ __forceinline__ void bound_collect(const uint32_t* __restrict__ lo, uint32_t n /* multiple of 16 */, uint32_t H, uint32_t* __restrict__ cnt, uint32_t* __restrict__ cand,
                                              uint32_t cap = kBoundCandCap, const uint32_t* __restrict__ ids = nullptr) {
    __shared__ uint32_t s_rows[kCollectBuf];
    __shared__ uint32_t s_cnt[3], s_base;                              // a chunk's count: three words in turn, so that one barrier per chunk is enough (below)
    const uint32_t lane = lane_id();
    const uint32_t stride = gridDim.x * kCollectChunk, mine = threadIdx.x * 4u;
    if (threadIdx.x < 3u) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    // (entered by the whole workgroup behind a barrier that follows the last write to s_rows; `more`: another chunk follows)
    auto flush = [&](uint32_t fill, bool more) {
        if (threadIdx.x == 0) s_base = atomicAdd(cnt, fill);
        __syncthreads();
        const uint32_t b0 = s_base;
        for (uint32_t i = threadIdx.x; i < fill; i += blockDim.x) {
            if (b0 + i < cap) cand[b0 + i] = ids ? ids[s_rows[i]] : s_rows[i];
        }
        if (more) __syncthreads();                                     // the buffer is read before the next chunk writes it
    };
    const u4 none = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    uint32_t base = blockIdx.x * kCollectChunk;
    uint32_t fill = 0, p = 0;                                          // rows in the buffer at the head of this chunk; this chunk's counter (both uniform)
    // a thread's words of a chunk: requested by EVERY thread — one past the end asks for the array's head and drops it when the words
    // are looked at — so that the request of the next chunk stays in flight behind this chunk's words (a request under a condition is
    // waited for where the paths join)
    bool x_on[kCollectVecs]; u4 x[kCollectVecs];
#pragma unroll
    for (uint32_t v = 0; v < kCollectVecs; v++) {
        x_on[v] = base < n && n - base > v * 1024u + mine;
        x[v] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(lo + (x_on[v] ? base + v * 1024u + mine : 0u)));
    }
    while (base < n) {
        const bool more = n - base > stride;                           // (no sum that could wrap)
        bool nx_on[kCollectVecs]; u4 nx[kCollectVecs];
#pragma unroll
        for (uint32_t v = 0; v < kCollectVecs; v++) {
            nx_on[v] = more && n - base - stride > v * 1024u + mine;
            nx[v] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(lo + (nx_on[v] ? base + stride + v * 1024u + mine : 0u)));
        }
        __builtin_amdgcn_sched_barrier(0);
        bool c[kCollectVecs * 4]; uint64_t m[kCollectVecs * 4];
        uint32_t tot = 0;
#pragma unroll
        for (uint32_t v = 0; v < kCollectVecs; v++) {
            if (!x_on[v]) x[v] = none;
            const uint32_t xs[4] = {x[v].x, x[v].y, x[v].z, x[v].w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                c[v * 4 + j] = xs[j] <= H && xs[j] != 0xFFFFFFFFu;
                m[v * 4 + j] = __ballot(c[v * 4 + j]);
                tot += (uint32_t)__builtin_popcountll(m[v * 4 + j]);
            }
        }
        if (tot) {                                                     // (wave-uniform)
            uint32_t b0 = 0;
            if (lane == 0) b0 = atomicAdd(&s_cnt[p], tot);             // LDS
            b0 = fill + __builtin_amdgcn_readfirstlane(b0);            // fill <= kCollectBuf - kCollectChunk, and a chunk holds kCollectChunk at most
#pragma unroll
            for (uint32_t e = 0; e < kCollectVecs * 4; e++) {
                if (c[e]) s_rows[b0 + (uint32_t)__builtin_popcountll(m[e] & ((1ull << lane) - 1ull))] = base + (e >> 2) * 1024u + mine + (e & 3u);   // (the compact form's indirection: at the flush)
                b0 += (uint32_t)__builtin_popcountll(m[e]);
            }
        }
        __syncthreads();
        // this chunk's count is final, and the next chunk counts in another word, so every thread reads the same number.  The word of the
        // chunk BEFORE this one is zeroed for the chunk after the next: all have read it in front of the barrier above, and it is
        // counted in again only behind the next chunk's barrier.
        fill += s_cnt[p];
        if (threadIdx.x == 0) s_cnt[p == 0u ? 2u : p - 1u] = 0;
        p = p == 2u ? 0u : p + 1u;
        if (!more) break;
        if (fill > kCollectBuf - kCollectChunk) { flush(fill, true); fill = 0; }
#pragma unroll
        for (uint32_t v = 0; v < kCollectVecs; v++) { x[v] = nx[v]; x_on[v] = nx_on[v]; }
        base += stride;
    }
    if (fill) flush(fill, false);
}
__global__ void __launch_bounds__(256)
k_bound_collect(const uint32_t* __restrict__ lo_all, uint32_t n /* multiple of 64 */, BoundCtrl* __restrict__ ctrl, uint32_t* __restrict__ cand,
                const uint32_t* __restrict__ gate = nullptr /* as k_bound_scan's */, uint32_t cap = kBoundCandCap,
                const uint32_t* __restrict__ n_ptr = nullptr /* behind k_bound_refine8: the compact array's length (a multiple of 64), on the device */,
                const uint32_t* __restrict__ ids = nullptr /* ... and its rows */) {
    if (gate != nullptr && *gate == 0u) return;
    const uint32_t inv = ctrl->thr_inv;
    if (inv == 0u) return;                                             // no H: k_bound_rescore hands the query back
    if (n_ptr != nullptr) n = *n_ptr;
    bound_collect(lo_all, n, ~inv, &ctrl->cand_cnt, cand, cap, ids);
}

// One query's survivors walked exactly by one workgroup, lane == survivor — the shared pass's re-score (k_bound_rescore_mq: a workgroup per query;
// the single query's k_bound_rescore below spreads its survivors over waves and workgroups instead) (cnt: how many the collect counted; has_H: it had a threshold).  decided(hand_back)
// runs on thread 0 once the query's norm is known; a query handed back writes nothing.
template <int M, typename F>
__device__ __forceinline__ void bound_rescore_query(const IndexView& v, const float* __restrict__ query, uint32_t k, uint32_t cnt, bool has_H, const uint32_t* __restrict__ cand,
                                                    uint32_t* __restrict__ rows_out, float* __restrict__ dist_out, F decided) {
    using Q = typename MT<M>::Q;
    extern __shared__ __align__(16) unsigned char smem[];
    Q* q_lds = reinterpret_cast<Q*>(smem);
    uint64_t* wl = reinterpret_cast<uint64_t*>(smem + (((size_t)v.dim4 * 4 * sizeof(Q)) + 15) / 16 * 16);   // [kScanWaves][64]
    __shared__ double s_qn;
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t ns = cnt < kBoundCandCap ? cnt : kBoundCandCap, kth = k - 1;
    stage_query<M>(q_lds, query, v.dim, v.dim4);
    __syncthreads();
    // the survivors' rows and norms are requested before the query's norm is walked
    const f4* tiles = reinterpret_cast<const f4*>(v.tiles);
    if (wave == kScanWaves - 1) {
        // |q| as the reference's chain (distances.go:20): cosine's finalize takes it, and every metric's hand-back rule
        double ma = 0.0;
        for (uint32_t i = 0; i < v.dim; i++) { const double a = (double)q_lds[i]; ma = __builtin_fma(a, a, ma); }
        if (lane == 0) s_qn = __builtin_sqrt(ma);
    }
    __syncthreads();
    const double qn = s_qn;
    const bool hand_back = cnt > kBoundCandCap || !has_H || !bound_scan_norm_ok(qn, v.dim);
    if (threadIdx.x == 0) decided(hand_back);
    if (hand_back) return;
    QConst qc; qc.qn = 0.0; qc.qn32 = 0.0f;
    if constexpr (M == QV_COSINE) qc.qn = qn;
    uint64_t list = kDeadKey, thr = kDeadKey;
    for (uint32_t base = wave * 64; base < ns; base += kScanWaves * 64) {
        const uint32_t i = base + lane;
        uint64_t key = kDeadKey;
        if (i < ns) {
            const uint32_t row = cand[i];
            const typename MT<M>::A acc = row_accumulate<M, kUnroll, false, true>(tiles + (size_t)(row >> 6) * v.dim4 * 64 + (row & 63), 64, q_lds, v.dim4);
            double rn = 0.0;
            if constexpr (MT<M>::needs_rnorm) rn = v.rnorm[row];
            key = make_key(finalize<M>(acc, qc, rn), row);
        }
        if (base == wave * 64) { list = wave_sort64(key, lane); thr = readlane64(list, kth); }
        else list_insert(list, thr, key, kth, lane);
    }
    __syncthreads();
    wl[wave * 64 + lane] = list;
    __syncthreads();
    if (wave == 0) {
        for (uint32_t w = 1; w < kScanWaves; w++) list_insert(list, thr, lane < k ? wl[w * 64 + lane] : kDeadKey, kth, lane);
        if (lane < k) {
            const bool dead = list == kDeadKey;
            rows_out[lane] = dead ? 0xFFFFFFFFu : (uint32_t)list;
            dist_out[lane] = dead ? __uint_as_float(0x7F800000u) : unord_f32((uint32_t)(list >> 32));
        }
    }
}

// The single query's re-score: a WAVE per survivor, kBoundRescoreGrid workgroups at most (a fixed grid chosen at launch; the count lives on the
// device).  bound_rescore_query above puts lane == survivor: with a few tens of survivors one wave works, and each lane walks its row's
// chunks — 1 KiB apart — sixteen at a time behind a barrier, a dozen rounds of gather latency in front of one dependent chain (52 us for
// 42 survivors at 768 dimensions; profiles/LAB_r10_bound_scan_8bit.md).  Here a wave requests ALL of a survivor's chunks at once, spread over
// its lanes, stages them in LDS, and then runs the one in-order chain acc1<M> over elements 0 .. dim - 1 against the staged query in
// MT<M>::Q, then finalize<M>: row_accumulate's chain in its order, so the exact scan's bits.  (Every lane runs the same chain on the same
// LDS words: a broadcast, no divergence.)  The keys go through the wave's list, the waves' lists through wave 0, the workgroups' lists
// through `partial` (stage 1's, dead since H was computed) and a ticket on the stage's control words (bound_scan_tail's protocol); the
// LAST workgroup merges them and writes the k results.
// Exactly one thread — thread 0 of that last workgroup, when every workgroup has read the control words and the gate — decides
// hand-back and writes stats[], ctrl->flag, next->flag, the zeroed control words and the gate, with the values the one-workgroup kernel wrote.
// P8: the re-score behind the 8-bit stage (ctrl = that stage's words, next = the bfloat16 stage's).  It answers, or sets its own flag — the
// word the bfloat16 stage's three launches are gated on — and then that stage decides or hands on to the exact scan.  An 8-bit search counts
// as a bound-scan search in stats[0 .. 2]; its own counters sit at kBound8StatsWord.
// gate (the bfloat16 stage behind the 8-bit one): zero = the 8-bit stage has answered and has cleared this stage's flag for the exact scan
// behind; non-zero = this stage runs, and its last workgroup zeroes the word, which this launch is the last to read.
constexpr uint32_t kBoundRescoreGrid = 64;     // 256 waves: one round for a few hundred survivors
constexpr uint32_t kBoundRefineGrid = 256;     // k_bound_refine8: 1024 waves, a batch of 16 candidates each: one round for 16 384 candidates
template <int M, bool P8 = false>
__global__ void __launch_bounds__(kScanBlock)
k_bound_rescore(IndexView v, const float* __restrict__ query, uint32_t k, BoundCtrl* __restrict__ ctrl, const uint32_t* __restrict__ cand,
                uint32_t* __restrict__ stats, uint32_t* __restrict__ rows_out, float* __restrict__ dist_out, uint32_t* gate, BoundCtrl* next,
                uint64_t* __restrict__ partial /* [gridDim.x][k] */,
                const BoundQuery8* __restrict__ qst = nullptr /* behind the 6-bit stage: k_bound_scan6 left |q| there, the same chain over the same values */) {
    if (gate != nullptr && *gate == 0u) return;
    using Q = typename MT<M>::Q;
    extern __shared__ __align__(16) unsigned char smem[];
    Q* q_lds = reinterpret_cast<Q*>(smem);
    const size_t q_bytes = (((size_t)v.dim4 * 4 * sizeof(Q)) + 15) / 16 * 16;
    uint64_t* wl = reinterpret_cast<uint64_t*>(smem + q_bytes);       // [kScanWaves][64]
    float* rbuf = reinterpret_cast<float*>(smem + q_bytes + (size_t)kScanWaves * 64 * sizeof(uint64_t));   // [kScanWaves][dim4 * 4]: a wave's survivor
    __shared__ double s_qn;
    __shared__ uint32_t s_last;
    const uint32_t cnt = ctrl->cand_cnt, thr_inv = ctrl->thr_inv;
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t ns = cnt < kBoundCandCap ? cnt : kBoundCandCap, kth = k - 1;
    // The workgroups that have a survivor — one at least, which then decides for a search without any.  The others only take their ticket:
    // with a handful of survivors the launch costs what one workgroup costs.  Should such a workgroup draw the LAST ticket, it goes on
    // as the one that decides and merges (every list is published by then), and prepares the query for that.
    const uint32_t active = std::max(1u, std::min((uint32_t)gridDim.x, (ns + kScanWaves - 1) / kScanWaves));
    const bool idle = blockIdx.x >= active;
    if (idle) {
        if (threadIdx.x == 0) s_last = atomicAdd(&ctrl->ticket, 1u) == gridDim.x - 1 ? 1u : 0u;   // (behind this workgroup's reads of ctrl and the gate)
        __syncthreads();
        if (!s_last) return;
    }
    stage_query<M>(q_lds, query, v.dim, v.dim4);
    __syncthreads();
    if (qst != nullptr) {
        // (dim dependent float64 steps that no survivor's chain could start ahead of: half of this launch behind the 6-bit stage)
        if (threadIdx.x == 0) s_qn = qst->qn;
    } else if (wave == kScanWaves - 1) {
        // |q| as the reference's chain (distances.go:20): cosine's finalize takes it, and every metric's hand-back rule
        double ma = 0.0;
        for (uint32_t i = 0; i < v.dim; i++) { const double a = (double)q_lds[i]; ma = __builtin_fma(a, a, ma); }
        if (lane == 0) s_qn = __builtin_sqrt(ma);
    }
    __syncthreads();
    const double qn = s_qn;
    const bool hand_back = cnt > kBoundCandCap || thr_inv == 0u || !bound_scan_norm_ok(qn, v.dim);   // (the same in every workgroup)
    uint64_t list = kDeadKey, thr = kDeadKey;
    if (!hand_back && !idle) {
        QConst qc; qc.qn = 0.0; qc.qn32 = 0.0f;
        if constexpr (M == QV_COSINE) qc.qn = qn;
        const f4* tiles = reinterpret_cast<const f4*>(v.tiles);
        f4* mine = reinterpret_cast<f4*>(rbuf + (size_t)wave * v.dim4 * 4);
        bool first = true;
        for (uint32_t i = blockIdx.x * kScanWaves + wave; i < ns; i += active * kScanWaves) {   // (wave-uniform)
            const uint32_t row = cand[i];
            const f4* src = tiles + (size_t)(row >> 6) * v.dim4 * 64 + (row & 63);
            double rn = 0.0;
            if constexpr (MT<M>::needs_rnorm) rn = v.rnorm[row];
            // the row's chunks, lane by lane, four requests of a lane in flight together (768 dimensions: all three)
            for (uint32_t c0 = 0; c0 < v.dim4; c0 += 256) {
                f4 x[4];
#pragma unroll
                for (uint32_t u = 0; u < 4; u++) { const uint32_t c = c0 + u * 64 + lane; if (c < v.dim4) x[u] = __builtin_nontemporal_load(&src[(size_t)c * 64]); }
#pragma unroll
                for (uint32_t u = 0; u < 4; u++) { const uint32_t c = c0 + u * 64 + lane; if (c < v.dim4) mine[c] = x[u]; }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // the wave's own LDS writes before its reads of other lanes' chunks
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            typename MT<M>::A acc = 0;
            for (uint32_t c = 0; c < v.dim4; c++) {                    // ONE chain, element order: row_accumulate's
                const f4 r = mine[c];
                const Q* qq = q_lds + (size_t)c * 4;
                acc1<M>(acc, qq[0], r.x); acc1<M>(acc, qq[1], r.y); acc1<M>(acc, qq[2], r.z); acc1<M>(acc, qq[3], r.w);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // ... and those reads before the next survivor's writes
            __builtin_amdgcn_wave_barrier();
            const uint64_t key = lane == 0 ? make_key(finalize<M>(acc, qc, rn), row) : kDeadKey;
            if (first) { list = wave_sort64(key, lane); thr = readlane64(list, kth); first = false; }
            else list_insert(list, thr, key, kth, lane);
        }
    }
    wl[wave * 64 + lane] = list;
    __syncthreads();
    if (wave == 0 && !idle) {
        if (!hand_back) {
            for (uint32_t w = 1; w < kScanWaves; w++) list_insert(list, thr, lane < k ? wl[w * 64 + lane] : kDeadKey, kth, lane);
            uint64_t* out = partial + (size_t)blockIdx.x * k;
            if (lane < k) (void)atomicExch(reinterpret_cast<unsigned long long*>(&out[lane]), (unsigned long long)list);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // every lane's exchange has returned: the list is at the memory side
        }
        uint32_t last = 0;
        if (lane == 0) last = atomicAdd(&ctrl->ticket, 1u) == gridDim.x - 1 ? 1u : 0u;   // (behind this workgroup's reads of ctrl and the gate)
        last = __builtin_amdgcn_readfirstlane(last);
        if (lane == 0) s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    if (threadIdx.x == 0) {
        ctrl->ticket = 0;                                              // for the next launch on these words (stream order)
        if constexpr (P8) {
            stats[kBound8StatsWord] = cnt;
            if (hand_back) (void)atomicAdd(&stats[kBound8StatsWord + 1], 1u);
            (void)atomicAdd(&stats[kBound8StatsWord + 2], 1u);
            if (!hand_back) { stats[0] = cnt; (void)atomicAdd(&stats[2], 1u); next->flag = 0u; }
        } else {
            stats[0] = cnt;
            if (hand_back) (void)atomicAdd(&stats[1], 1u);
            (void)atomicAdd(&stats[2], 1u);
            if (gate != nullptr) *gate = 0u;                           // (every workgroup read it before it took its ticket)
        }
        ctrl->flag = hand_back ? 1u : 0u;                              // the launch behind this one reads it
        ctrl->cand_cnt = 0; ctrl->thr_inv = 0;                         // zero, as the words are kept
    }
    if (hand_back) return;                                             // a query handed back writes nothing
    merge_lists_last_workgroup(partial, active, k, rows_out, dist_out);
}

// ---------------------------------------------------------------- one query: reject rows on the 8-bit plane first --
// k_bound_scan's walk and tail over IndexView::plane8 — a quarter of the float32 bytes: per 16-dimension step a lane reads its row's 16
// int8 values (one dwordx4, the wave one contiguous KiB).  The query is quantised once per workgroup into LDS as two int8 terms
// (qv_bound.h: qq = 128 hi + lo), a row's sum is eight integer dot products per step, exact, and the interval comes from
// bound_scan_interval8.  Lower bounds, upper bounds, H, k_bound_collect and the re-score are the bfloat16 stage's own; what this stage
// cannot decide (more than kBoundCandCap candidates, no finite H, a query it cannot quantise) goes to the bfloat16 stage, gated
// behind it, not to the exact scan: corpora with many rows within the 8-bit margin of the k-th distance keep the bfloat16 stage's time.
typedef int i32;
template <int U>
__device__ __forceinline__ void bound8_block(const u4* __restrict__ p, const u4* __restrict__ qh, const u4* __restrict__ ql, uint32_t s0, i32 (&acc)[4]) {
    u4 x[U];
#pragma unroll
    for (int u = 0; u < U; u++) x[u] = __builtin_nontemporal_load(&p[(size_t)(s0 + u) * 64]);
    __builtin_amdgcn_sched_barrier(0);                                 // all requests of the block ahead of the arithmetic (see row_accumulate)
#pragma unroll
    for (int u = 0; u < U; u++) {
        const u4 h = qh[s0 + u], l = ql[s0 + u];
        acc[0] = __builtin_amdgcn_sdot4((i32)h.x, (i32)x[u].x, acc[0], false);
        acc[1] = __builtin_amdgcn_sdot4((i32)h.y, (i32)x[u].y, acc[1], false);
        acc[0] = __builtin_amdgcn_sdot4((i32)h.z, (i32)x[u].z, acc[0], false);
        acc[1] = __builtin_amdgcn_sdot4((i32)h.w, (i32)x[u].w, acc[1], false);
        acc[2] = __builtin_amdgcn_sdot4((i32)l.x, (i32)x[u].x, acc[2], false);
        acc[3] = __builtin_amdgcn_sdot4((i32)l.y, (i32)x[u].y, acc[3], false);
        acc[2] = __builtin_amdgcn_sdot4((i32)l.z, (i32)x[u].z, acc[2], false);
        acc[3] = __builtin_amdgcn_sdot4((i32)l.w, (i32)x[u].w, acc[3], false);
    }
}
// I of this lane's row of one tile (p = the tile in the plane + the lane)
__device__ __forceinline__ long long bound8_tile(const u4* __restrict__ p, const u4* __restrict__ qh, const u4* __restrict__ ql, uint32_t steps) {
    i32 acc[4] = {0, 0, 0, 0};
    uint32_t s = 0;
    for (; s + 16 <= steps; s += 16) bound8_block<16>(p, qh, ql, s, acc);
    if (s + 8 <= steps) { bound8_block<8>(p, qh, ql, s, acc); s += 8; }
    if (s + 4 <= steps) { bound8_block<4>(p, qh, ql, s, acc); s += 4; }
    if (s + 2 <= steps) { bound8_block<2>(p, qh, ql, s, acc); s += 2; }
    if (s < steps) bound8_block<1>(p, qh, ql, s, acc);
    return ((long long)acc[0] + (long long)acc[1]) * 128ll + ((long long)acc[2] + (long long)acc[3]);   // (each partial sum exact in int32: dim <= kBoundMaxDim)
}

// The query of an integer stage, once per workgroup (k_bound_scan8, k_bound_scan6, k_bound_refine8): sq = max|q_i| / 16256, qq = rint(q / sq)
// = 128 hi + lo into LDS as two int8 terms, qres = |q - sq qq| rounded up (NaN: a query without a scale — every row comes out "unsure",
// no H, and the re-score hands the search on), qn = |q| as the reference's chain.  SUM: qsum = sum qq_i as well (the 6-bit plane's codes are
// stored biased).  Ends behind a barrier: the terms are in LDS.
template <bool SUM>
__device__ __forceinline__ void bound8_stage_query(const float* __restrict__ query, uint32_t dim, int8_t* qh8, int8_t* ql8, uint32_t lane, uint32_t wave,
                                                   double& sq_out, double& qn_out, double& qres_out, long long& qsum_out) {
    __shared__ float s_max[kScanWaves];
    __shared__ uint32_t s_bad[kScanWaves];
    __shared__ double s_res[kScanWaves];
    __shared__ double s_qn;
    __shared__ int s_sum[kScanWaves];
    // the query, quantised: sq = max|q_i| / 16256, qq = rint(q / sq) = 128 hi + lo; qres = |q - sq qq| rounded up
    float mx = 0.f; bool bad = false;
    for (uint32_t i = threadIdx.x; i < dim; i += blockDim.x) { const float x = query[i]; bad |= !((x - x) == 0.0f); mx = __builtin_fmaxf(mx, __builtin_fabsf(x)); }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mx = __builtin_fmaxf(mx, __shfl_xor(mx, m));
    const bool wbad = __ballot(bad) != 0ull;
    if (lane == 0) { s_max[wave] = mx; s_bad[wave] = wbad ? 1u : 0u; }
    __syncthreads();
    uint32_t anybad = 0;
    for (uint32_t w = 0; w < kScanWaves; w++) { mx = __builtin_fmaxf(mx, s_max[w]); anybad |= s_bad[w]; }
    const bool q_ok = !anybad && mx > 0.0f;
    const double sq = q_ok ? (double)mx / (double)kBound8QueryMax : 1.0;
    double r2 = 0.0;
    int qs = 0;
    for (uint32_t i = threadIdx.x; i < dim; i += blockDim.x) {
        const double x = q_ok ? (double)query[i] : 0.0;
        const double qq = __builtin_rint(x / sq);                      // |qq| <= 16256
        const double hi = __builtin_rint(qq * (1.0 / 128.0)), lo = qq - 128.0 * hi;   // |hi| <= 127, |lo| <= 64: exact
        qh8[i] = (int8_t)(int)hi; ql8[i] = (int8_t)(int)lo;
        if constexpr (SUM) qs += (int)qq;                              // (exact: dim * 16256 < 2^31)
        const double d = x - sq * qq;
        r2 = __builtin_fma(d, d, r2);
    }
    r2 = wave_sum_f64(r2);
    if (lane == 0) s_res[wave] = r2;
    if constexpr (SUM) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) qs += __shfl_xor(qs, m);
        if (lane == 0) s_sum[wave] = qs;
    }
    if (wave == kScanWaves - 1) {
        // |q| as the reference's chain (distances.go:20), one wave: 64 values per request, walked in order
        double ma = 0.0;
        for (uint32_t b = 0; b < dim; b += 64) {
            const float x = b + lane < dim ? query[b + lane] : 0.f;
            const uint32_t n = dim - b < 64u ? dim - b : 64u;
            for (uint32_t j = 0; j < n; j++) { const double a = (double)__uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(x), j)); ma = __builtin_fma(a, a, ma); }
        }
        if (lane == 0) s_qn = __builtin_sqrt(ma);
    }
    __syncthreads();
    double qres2 = 0.0;
    for (uint32_t w = 0; w < kScanWaves; w++) qres2 += s_res[w];
    qn_out = s_qn;
    sq_out = sq;
    // (a query without a scale: every row comes out "unsure", no H, and the re-score hands the search on)
    qres_out = q_ok ? __builtin_sqrt(qres2) * (1.0 + 1e-9) + 1e-300 : __builtin_nan("");
    qsum_out = 0;
    if constexpr (SUM) { for (uint32_t w = 0; w < kScanWaves; w++) qsum_out += (long long)s_sum[w]; }
}

// SKIP (k_bound_scan8<., true>: v.alive is a filter's candidate bitmap, as for k_bound_scan<., true>): the wave holds the word of the tile it
// walks and has the next one's in flight behind that tile's bytes; a tile whose word is zero is not requested — plane, rnorm, rscale8, rres8 —
// and its 64 lower-bound words are written as 0xFFFFFFFF (k_bound_collect reads every word of a reused workspace).  The query's scale, terms
// and norm are the workgroup's, computed before the walk, so a wave that reads no tile just publishes a dead list.
template <int M, bool SKIP = false, bool WIDE = false /* as k_bound_scan's */>
__global__ void __launch_bounds__(kScanBlock)
k_bound_scan8(IndexView v, const float* __restrict__ query, uint32_t k, BoundCtrl* __restrict__ ctrl, uint32_t* __restrict__ lo_all /* [n_tiles * 64] */,
              uint64_t* __restrict__ partial /* [grid][k] */, uint32_t* __restrict__ seed_rows, float* __restrict__ seed_dist) {
    extern __shared__ __align__(16) unsigned char smem[];
    int8_t* qh8 = reinterpret_cast<int8_t*>(smem);                     // [dim] hi terms, [dim] lo terms, dim a multiple of 16
    int8_t* ql8 = qh8 + v.dim;
    uint64_t* wl = reinterpret_cast<uint64_t*>(smem + (size_t)v.dim * 2);   // [kScanWaves][64]
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t steps = v.dim >> 4, tw = gridDim.x * kScanWaves;
    double sq, qn, qres; long long qsum;
    bound8_stage_query<false>(query, v.dim, qh8, ql8, lane, wave, sq, qn, qres, qsum);

    const u4* qh = reinterpret_cast<const u4*>(qh8);
    const u4* ql = reinterpret_cast<const u4*>(ql8);
    const u4* plane = reinterpret_cast<const u4*>(v.plane8) + lane;
    const uint32_t kth = k - 1;
    uint64_t list = kDeadKey, thr = kDeadKey;
    bool first = true;
    uint32_t t = blockIdx.x * kScanWaves + wave;
    uint64_t am_next = 0ull;                                           // (SKIP) the word of the wave's next tile
    if constexpr (SKIP) am_next = t < v.n_tiles ? v.alive[t] : 0ull;
    for (; t < v.n_tiles; t += tw) {
        uint64_t am;                                                   // wave-uniform
        if constexpr (SKIP) {
            am = am_next;
            if (t + tw < v.n_tiles) am_next = v.alive[t + tw];         // (in flight behind this tile's bytes)
            if (am == 0ull) { __builtin_nontemporal_store(0xFFFFFFFFu, &lo_all[t * 64 + lane]); continue; }
        }
        const uint32_t row = t * 64 + lane;
        const double rn = v.rnorm[row];                                // (requested ahead of the tile's bytes: there when the sums are)
        const float sc = v.rscale8[row], rr = v.rres8[row];
        if constexpr (!SKIP) am = v.alive[t];
        const long long isum = bound8_tile(plane + (size_t)t * steps * 64, qh, ql, steps);
        float lo, hi;
        (void)bound_scan_interval8<M>(isum, sq, qn, qres, rn, sc, rr, v.dim, lo, hi);
        const bool live = (am >> lane) & 1ull;                         // (dead rows and the last tile's padding: never candidates, never in a bound)
        __builtin_nontemporal_store(live ? ord_f32(lo) : 0xFFFFFFFFu, &lo_all[row]);
        const uint64_t key = live ? (((uint64_t)ord_f32(hi) << 32) | row) : kDeadKey;
        if (first) { list = wave_sort64(key, lane); thr = readlane64(list, kth); first = false; }
        else list_insert(list, thr, key, kth, lane);
    }
    if constexpr (WIDE) bound_scan_tail_wide(list, wave, lane, partial);
    else (void)bound_scan_tail(list, thr, wl, wave, lane, k, ctrl, partial, seed_rows, seed_dist);
}

// ---------------------------------------------------------------- one unfiltered query: reject rows on the 6-bit plane first --
// The 8-bit stage streams 0.80 of the memory's rate and leaves 42 survivors of 10M rows at k = 10 where the re-score takes several hundred
// in one round: the margin is far tighter than the funnel behind it needs.  So stage 1 reads IndexView::plane6 instead — three quarters
// of the 8-bit bytes, an interval about four times as wide (qv_bound.h) — and the 8-bit plane is read for ITS candidates only:
//   k_bound_scan6    k_bound_scan8's prologue, walk, epilogue and tail over the 6-bit plane: per group of 64 dimensions a lane reads its
//                    row's three 16-byte pieces (each a contiguous KiB of the wave), unpacks four times 16 biased codes and takes the same
//                    eight integer dot products per 16 dimensions; I6 = sum qq u - 32 sum qq.  Lower bounds, upper bounds and H6 as ever.
//   k_bound_collect  with the 6-bit stage's capacity, kBound6CandCap rows.
//   k_bound_refine8  a fixed grid, wave-strided over that list in batches of 16 (batches of 64 were measured first: four dependent rounds of
//                    gathers per batch on a sixteenth of the CUs; profiles/LAB_r20_bound_scan6.md): per candidate the wave gathers the row's
//                    16-byte pieces from plane8 (lane == step, a KiB apart), forms the exact 8-bit sum with the query terms k_bound_scan6
//                    left in the workspace, lane j keeps candidate j's; from there k_bound_scan8's epilogue — bound_scan_interval8, the lower bound into a COMPACT array indexed by
//                    candidate slot (the head of lo_all, dead since the collect), the upper bound's key into the wave's list, bound_scan_tail
//                    into the 8-bit stage's control words.  H8 from the candidates alone is valid: every row of the true top k is a 6-bit
//                    candidate, so k upper bounds of rows are at hand, and any k rows' upper bounds cap the k-th distance.
//   k_bound_collect  over the compact array (its length by pointer, the candidates' rows as an indirection) into the 8-bit stage's list,
//   and k_bound_rescore<M, true> finishes, as behind k_bound_scan8 but for |q|: k_bound_scan6 has left it in the workspace (BoundQuery8::qn, the
//   same in-order chain over the same float32 values: the same bits), so the dim dependent steps are not walked again.  A search the 6-bit stage cannot decide — more than kBound6CandCap candidates, no
// finite H6, a query it cannot quantise — leaves the 8-bit control words WITHOUT H (every refine wave publishes a dead list), so that re-score
// hands on to the gated bfloat16 stage: no gated full 8-bit stage in between (a gated launch costs every query 4.9 us).  More than
// kBoundCandCap survivors of the refine hand on in the same way.  Nothing is read on the host.
template <int U>
__device__ __forceinline__ void bound6_block(const u4* __restrict__ p, const u4* __restrict__ qh, const u4* __restrict__ ql, uint32_t g0, i32 (&acc)[4]) {
    u4 x[3 * U];
#pragma unroll
    for (int u = 0; u < 3 * U; u++) x[u] = __builtin_nontemporal_load(&p[((size_t)g0 * 3 + u) * 64]);
    __builtin_amdgcn_sched_barrier(0);                                 // all requests of the block ahead of the arithmetic (see row_accumulate)
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t X[4] = {x[3 * u].x, x[3 * u].y, x[3 * u].z, x[3 * u].w};
        const uint32_t Y[4] = {x[3 * u + 1].x, x[3 * u + 1].y, x[3 * u + 1].z, x[3 * u + 1].w};
        const uint32_t Z[4] = {x[3 * u + 2].x, x[3 * u + 2].y, x[3 * u + 2].z, x[3 * u + 2].w};
        uint32_t c[4][4];                                              // [16-dimension step of the group][dword]: biased codes, a byte each
#pragma unroll
        for (int j = 0; j < 4; j++) {
            c[0][j] = X[j] & 0x3F3F3F3Fu; c[1][j] = Y[j] & 0x3F3F3F3Fu; c[2][j] = Z[j] & 0x3F3F3F3Fu;
            c[3][j] = ((X[j] >> 6) & 0x03030303u) | ((Y[j] >> 4) & 0x0C0C0C0Cu) | ((Z[j] >> 2) & 0x30303030u);
        }
#pragma unroll
        for (int st = 0; st < 4; st++) {
            const u4 h = qh[(g0 + u) * 4 + st], l = ql[(g0 + u) * 4 + st];
            acc[0] = __builtin_amdgcn_sdot4((i32)h.x, (i32)c[st][0], acc[0], false);
            acc[1] = __builtin_amdgcn_sdot4((i32)h.y, (i32)c[st][1], acc[1], false);
            acc[0] = __builtin_amdgcn_sdot4((i32)h.z, (i32)c[st][2], acc[0], false);
            acc[1] = __builtin_amdgcn_sdot4((i32)h.w, (i32)c[st][3], acc[1], false);
            acc[2] = __builtin_amdgcn_sdot4((i32)l.x, (i32)c[st][0], acc[2], false);
            acc[3] = __builtin_amdgcn_sdot4((i32)l.y, (i32)c[st][1], acc[3], false);
            acc[2] = __builtin_amdgcn_sdot4((i32)l.z, (i32)c[st][2], acc[2], false);
            acc[3] = __builtin_amdgcn_sdot4((i32)l.w, (i32)c[st][3], acc[3], false);
        }
    }
}
// sum qq_i u_i of this lane's row of one tile (p = the tile in the plane + the lane); blocks of six groups: 18 KiB of a wave requested ahead
__device__ __forceinline__ long long bound6_tile(const u4* __restrict__ p, const u4* __restrict__ qh, const u4* __restrict__ ql, uint32_t groups) {
    i32 acc[4] = {0, 0, 0, 0};
    uint32_t g = 0;
    for (; g + 6 <= groups; g += 6) bound6_block<6>(p, qh, ql, g, acc);
    if (g + 3 <= groups) { bound6_block<3>(p, qh, ql, g, acc); g += 3; }
    if (g + 2 <= groups) { bound6_block<2>(p, qh, ql, g, acc); g += 2; }
    if (g < groups) bound6_block<1>(p, qh, ql, g, acc);
    return ((long long)acc[0] + (long long)acc[1]) * 128ll + ((long long)acc[2] + (long long)acc[3]);   // (each partial sum exact in int32: codes <= 63)
}

template <int M>
__global__ void __launch_bounds__(kScanBlock)
k_bound_scan6(IndexView v, const float* __restrict__ query, uint32_t k, BoundCtrl* __restrict__ ctrl, uint32_t* __restrict__ lo_all /* [n_tiles * 64] */,
              uint64_t* __restrict__ partial /* [grid][k] */, uint32_t* __restrict__ seed_rows, float* __restrict__ seed_dist,
              BoundQuery8* __restrict__ qst /* the quantised query, for k_bound_refine8 behind (workgroup 0 writes it) */) {
    extern __shared__ __align__(16) unsigned char smem[];
    int8_t* qh8 = reinterpret_cast<int8_t*>(smem);                     // [dim] hi terms, [dim] lo terms, dim a multiple of 64
    int8_t* ql8 = qh8 + v.dim;
    uint64_t* wl = reinterpret_cast<uint64_t*>(smem + (size_t)v.dim * 2);   // [kScanWaves][64]
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t groups = v.dim >> 6, tw = gridDim.x * kScanWaves;
    double sq, qn, qres; long long qsum;
    bound8_stage_query<true>(query, v.dim, qh8, ql8, lane, wave, sq, qn, qres, qsum);
    const long long bias = (long long)kBound6Bias * qsum;
    if (blockIdx.x == 0) {
        for (uint32_t i = threadIdx.x; i < v.dim / 8; i += blockDim.x) reinterpret_cast<u4*>(qst->terms)[i] = reinterpret_cast<const u4*>(smem)[i];
        if (threadIdx.x == 0) { qst->sq = sq; qst->qn = qn; qst->qres = qres; }
    }

    const u4* qh = reinterpret_cast<const u4*>(qh8);
    const u4* ql = reinterpret_cast<const u4*>(ql8);
    const u4* plane = reinterpret_cast<const u4*>(v.plane6) + lane;
    const uint32_t kth = k - 1;
    uint64_t list = kDeadKey, thr = kDeadKey;
    bool first = true;
    for (uint32_t t = blockIdx.x * kScanWaves + wave; t < v.n_tiles; t += tw) {
        const uint32_t row = t * 64 + lane;
        const double rn = v.rnorm[row];                                // (requested ahead of the tile's bytes: there when the sums are)
        const float sc = 4.0f * v.rscale8[row], rr = v.rres6[row];     // (4 rscale8: exact)
        const uint64_t am = v.alive[t];                                // wave-uniform
        const long long isum = bound6_tile(plane + (size_t)t * groups * 192, qh, ql, groups) - bias;
        float lo, hi;
        (void)bound_scan_interval8<M>(isum, sq, qn, qres, rn, sc, rr, v.dim, lo, hi);
        const bool live = (am >> lane) & 1ull;                         // (dead rows and the last tile's padding: never candidates, never in a bound)
        __builtin_nontemporal_store(live ? ord_f32(lo) : 0xFFFFFFFFu, &lo_all[row]);
        const uint64_t key = live ? (((uint64_t)ord_f32(hi) << 32) | row) : kDeadKey;
        if (first) { list = wave_sort64(key, lane); thr = readlane64(list, kth); first = false; }
        else list_insert(list, thr, key, kth, lane);
    }
    (void)bound_scan_tail(list, thr, wl, wave, lane, k, ctrl, partial, seed_rows, seed_dist);
}

// ctrl6: the 6-bit stage's words (H6 and its collect's count; zeroed here by the last workgroup); ctrl8: the 8-bit stage's, which this kernel
// leaves as k_bound_scan8 leaves them.  lo8: the compact array, entry = candidate slot, written in whole batches of 64 (slots past the
// count: 0xFFFFFFFF); *n8: its length for the collect behind.  stats: the index's counters.
constexpr int kRefineBatch = 16;               // candidates of a batch: their pieces are requested together (a lane: 16 dwordx4 in flight), lanes 0 - 15 keep the sums
template <int M>
__global__ void __launch_bounds__(kScanBlock)
k_bound_refine8(IndexView v, const BoundQuery8* __restrict__ qst, uint32_t k, BoundCtrl* __restrict__ ctrl6, BoundCtrl* __restrict__ ctrl8, const uint32_t* __restrict__ cand6,
                uint32_t* __restrict__ lo8, uint32_t* __restrict__ n8, uint64_t* __restrict__ partial /* [grid][k] */, uint32_t* __restrict__ seed_rows, float* __restrict__ seed_dist,
                uint32_t* __restrict__ stats) {
    extern __shared__ __align__(16) unsigned char smem[];
    int8_t* qh8 = reinterpret_cast<int8_t*>(smem);
    int8_t* ql8 = qh8 + v.dim;
    uint64_t* wl = reinterpret_cast<uint64_t*>(smem + (size_t)v.dim * 2);   // [kScanWaves][64]
    const uint32_t cnt = __builtin_amdgcn_readfirstlane(ctrl6->cand_cnt), inv6 = __builtin_amdgcn_readfirstlane(ctrl6->thr_inv);   // (read by every workgroup before its ticket)
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t steps = v.dim >> 4, tw = gridDim.x * kScanWaves;
    // the query as k_bound_scan6 quantised it (the |q| chain is dim dependent steps: not walked a second time in front of a short kernel)
    for (uint32_t i = threadIdx.x; i < v.dim / 8; i += blockDim.x) reinterpret_cast<u4*>(smem)[i] = reinterpret_cast<const u4*>(qst->terms)[i];
    const double sq = qst->sq, qn = qst->qn, qres = qst->qres;
    __syncthreads();
    const bool hand_back = inv6 == 0u || cnt > kBound6CandCap;        // (a query without a scale had no H6)
    const uint32_t ns = hand_back ? 0u : cnt;

    const u4* qh = reinterpret_cast<const u4*>(qh8);
    const u4* ql = reinterpret_cast<const u4*>(ql8);
    const u4* plane = reinterpret_cast<const u4*>(v.plane8);
    const uint32_t kth = k - 1;
    uint64_t list = kDeadKey, thr = kDeadKey;
    bool first = true;
    for (uint32_t b = (blockIdx.x * kScanWaves + wave) * kRefineBatch; b < ns; b += tw * kRefineBatch) {   // (wave-uniform)
        const uint32_t slot = b + lane;
        const bool mine_on = lane < (uint32_t)kRefineBatch, live = mine_on && slot < ns;
        const uint32_t row = live ? cand6[slot] : 0u;                  // (row 0 is a row of the index: a slot past the count reads it and drops the sum)
        const double rn = v.rnorm[row];
        const float sc = v.rscale8[row], rr = v.rres8[row];
        i32 ah[kRefineBatch], al[kRefineBatch];
#pragma unroll
        for (int u = 0; u < kRefineBatch; u++) { ah[u] = 0; al[u] = 0; }
        for (uint32_t s0 = 0; s0 < steps; s0 += 64) {
            const uint32_t st = s0 + lane;
            const bool on = st < steps;
            u4 x[kRefineBatch];
#pragma unroll
            for (int u = 0; u < kRefineBatch; u++) {
                const uint32_t r = __builtin_amdgcn_readlane(row, u);
                x[u] = u4{0u, 0u, 0u, 0u};
                if (on) x[u] = __builtin_nontemporal_load(&plane[((size_t)(r >> 6) * steps + st) * 64 + (r & 63u)]);
            }
            const u4 zero = {0u, 0u, 0u, 0u};
            const u4 h = on ? qh[st] : zero, l = on ? ql[st] : zero;
#pragma unroll
            for (int u = 0; u < kRefineBatch; u++) {
                ah[u] = __builtin_amdgcn_sdot4((i32)h.x, (i32)x[u].x, ah[u], false);
                ah[u] = __builtin_amdgcn_sdot4((i32)h.y, (i32)x[u].y, ah[u], false);
                ah[u] = __builtin_amdgcn_sdot4((i32)h.z, (i32)x[u].z, ah[u], false);
                ah[u] = __builtin_amdgcn_sdot4((i32)h.w, (i32)x[u].w, ah[u], false);
                al[u] = __builtin_amdgcn_sdot4((i32)l.x, (i32)x[u].x, al[u], false);
                al[u] = __builtin_amdgcn_sdot4((i32)l.y, (i32)x[u].y, al[u], false);
                al[u] = __builtin_amdgcn_sdot4((i32)l.z, (i32)x[u].z, al[u], false);
                al[u] = __builtin_amdgcn_sdot4((i32)l.w, (i32)x[u].w, al[u], false);
            }
        }
        long long mine = 0;
#pragma unroll
        for (int u = 0; u < kRefineBatch; u++) {                       // (the row's sums are exact in int32: dim <= kBoundMaxDim)
            i32 a = ah[u], c = al[u];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) { a += __shfl_xor(a, m); c += __shfl_xor(c, m); }
            if (lane == (uint32_t)u) mine = (long long)a * 128ll + (long long)c;
        }
        float lo, hi;
        (void)bound_scan_interval8<M>(mine, sq, qn, qres, rn, sc, rr, v.dim, lo, hi);
        if (mine_on) lo8[slot] = live ? ord_f32(lo) : 0xFFFFFFFFu;     // (slot < the count rounded up to the batch <= n_tiles * 64)
        const uint64_t key = live ? (((uint64_t)ord_f32(hi) << 32) | row) : kDeadKey;
        if (first) { list = wave_sort64(key, lane); thr = readlane64(list, kth); first = false; }
        else list_insert(list, thr, key, kth, lane);
    }
    if (!bound_scan_tail(list, thr, wl, wave, lane, k, ctrl8, partial, seed_rows, seed_dist)) return;
    if (threadIdx.x == 0) {
        stats[kBound6StatsWord] = cnt;
        if (hand_back) (void)atomicAdd(&stats[kBound6StatsWord + 1], 1u);
        (void)atomicAdd(&stats[kBound6StatsWord + 2], 1u);
        *n8 = (ns + (uint32_t)kRefineBatch - 1u) / (uint32_t)kRefineBatch * (uint32_t)kRefineBatch;
        ctrl6->cand_cnt = 0; ctrl6->thr_inv = 0;                       // zero, as the words are kept
    }
}

// ---------------------------------------------------------------- one query, 65 <= k <= 1024: the wide form --
// The k <= 64 form stops at 64 because stage 1 keeps its upper bounds in a wave list of one key per lane and its re-score merges such lists;
// interval, collect and the exact chain do not depend on k.  The wide form keeps both scan kernels up to their tail and replaces the rest:
//   k_bound_scan<., SKIP, true> / k_bound_scan8<., SKIP, true>   the walk with a list length of 64; the tail publishes every wave's list
//                    (bound_scan_tail_wide, where the argument for H stands).  SKIP: the filtered form — v.alive is the call's candidate
//                    bitmap (a mask, a row set, a where-filter: alive & selected), tiles without a candidate are not read, their 64
//                    lower-bound words written as 0xFFFFFFFF all the same; everything behind stage 1 takes its liveness from v.alive and
//                    serves the bitmap as it stands, the key-per-row redo included (the filtered key-per-row path's own kernels).
//   launch_select_topk   the k smallest of the grid x kScanWaves x 64 published keys, sorted: its k-th output is H.
//   k_bound_collect_wide bound_collect against that H with a list of QV_BOUND_WIDE_CAND_CAP rows; workgroup 0 leaves H in the control words
//                    (thr_inv, zero = no finite H) for the re-score, as the k <= 64 tail does.
//   k_bound_rescore_wide a wave per survivor in k_bound_rescore's chain — the exact scan's bits — writing the (distance, row) key into
//                    keys[slot], dead keys into the slots past the count; the last workgroup (a ticket) decides hand-back, writes the
//                    counters, the flags and sel[] = {live keys, 1 = answered}.
//   launch_select_topk_counted   the k best of keys[0 .. count) in (distance, row) order into the caller's arrays — behind sel[1]: zero = it
//                    leaves the arrays alone.  ONE such launch ends the call, whichever stage answered.
// Handing on, on the device: the list overflowed, there is no finite H, or bound_scan_norm_ok declines |q|.  The 8-bit stage hands on to the
// bfloat16 stage, whose four launches are gated on that stage's flag word; the bfloat16 stage hands on to the key-per-row path behind ITS flag
// (launch_flat_select_redo_one; the caller enqueues nothing more).  The counters are the wide form's own (kBoundWideStatsWord): the k <= 64
// form's, the 8-bit and the 6-bit stage's do not move.
constexpr uint32_t kBoundWideCandCap = QV_BOUND_WIDE_CAND_CAP;
static_assert(kBoundWideCandCap >= kBoundWideMaxK + (kBoundCandCap - (uint32_t)kMaxFusedK), "the spare the k <= 64 form has over its largest k, kept at the largest wide k");
static_assert(kBoundWideCandCap <= 16384u && kBoundWideCandCap % kCollectChunk == 0, "launch_select_topk_counted takes 16384 keys at most");
constexpr uint32_t kBoundWideRescoreGrid = 256;   // 1024 waves: a thousand survivors in one round, a full list in eight
constexpr uint32_t kBoundWideListLen = 64;        // stage 1's list length: one key per lane

__global__ void __launch_bounds__(256)
k_bound_collect_wide(const uint32_t* __restrict__ lo_all, uint32_t n /* multiple of 64 */, uint32_t k, const uint32_t* __restrict__ seed_rows, const float* __restrict__ seed_dist /* [k] sorted */,
                     BoundCtrl* __restrict__ ctrl, uint32_t* __restrict__ cand, const uint32_t* __restrict__ gate /* as k_bound_scan's */) {
    if (gate != nullptr && *gate == 0u) return;
    const uint32_t H = ord_f32(seed_dist[k - 1]);
    const bool has_H = seed_rows[k - 1] != 0xFFFFFFFFu && H < 0xFF800000u;   // the k-th published key is a row's, and its bound finite
    if (blockIdx.x == 0 && threadIdx.x == 0) ctrl->thr_inv = has_H ? ~H : 0u;   // (the re-score behind reads it; cand_cnt is zero: the words are kept so)
    if (!has_H) return;
    bound_collect(lo_all, n, H, &ctrl->cand_cnt, cand, kBoundWideCandCap);
}

// The walk the two wide re-scores share (k_bound_rescore_wide: one query; k_bound_rescore_wide_mq: query blockIdx.y of a pass), written once so that
// the bit-exact chain has one place: ONE query's survivors cand[0 .. cnt) -> keys[0 .. cnt), dead keys behind, on a grid of gridDim.x
// workgroups that share the ticket in ctrl.  Entered by every thread of every workgroup of the query; returns with `last` set in thread 0
// of the query's LAST workgroup alone (every other workgroup has taken its ticket, so has read whatever it reads of the control words),
// which then decides: hand_back = the list overflowed, there is no finite H, or bound_scan_norm_ok declines |q|; ns = the live keys; cnt = the
// collect's count.
struct BoundWideWalk { bool last, hand_back; uint32_t ns, cnt; };
template <int M>
__device__ __forceinline__ BoundWideWalk bound_rescore_wide_walk(const IndexView& v, const float* __restrict__ query, BoundCtrl* __restrict__ ctrl, const uint32_t* __restrict__ cand,
                                                                 uint64_t* __restrict__ keys) {
    using Q = typename MT<M>::Q;
    extern __shared__ __align__(16) unsigned char smem[];
    Q* q_lds = reinterpret_cast<Q*>(smem);
    const size_t q_bytes = (((size_t)v.dim4 * 4 * sizeof(Q)) + 15) / 16 * 16;
    float* rbuf = reinterpret_cast<float*>(smem + q_bytes);           // [kScanWaves][dim4 * 4]: a wave's survivor
    __shared__ double s_qn;
    __shared__ uint32_t s_last;
    const uint32_t cnt = ctrl->cand_cnt, thr_inv = ctrl->thr_inv;
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool decided_early = cnt > kBoundWideCandCap || thr_inv == 0u;   // (handed on whatever |q| is: nothing to walk)
    const uint32_t ns = decided_early ? 0u : cnt;
    // as in k_bound_rescore: the workgroups without a survivor only take their ticket, unless they draw the last one
    const uint32_t active = std::max(1u, std::min((uint32_t)gridDim.x, (ns + kScanWaves - 1) / kScanWaves));
    const bool idle = blockIdx.x >= active;
    if (idle) {
        if (threadIdx.x == 0) s_last = atomicAdd(&ctrl->ticket, 1u) == gridDim.x - 1 ? 1u : 0u;   // (behind this workgroup's reads of ctrl and the gate)
        __syncthreads();
        if (!s_last) return BoundWideWalk{false, false, 0u, 0u};
    }
    stage_query<M>(q_lds, query, v.dim, v.dim4);
    __syncthreads();
    if (wave == kScanWaves - 1) {
        // |q| as the reference's chain (distances.go:20): cosine's finalize takes it, and every metric's hand-back rule
        double ma = 0.0;
        for (uint32_t i = 0; i < v.dim; i++) { const double a = (double)q_lds[i]; ma = __builtin_fma(a, a, ma); }
        if (lane == 0) s_qn = __builtin_sqrt(ma);
    }
    __syncthreads();
    const double qn = s_qn;
    const bool hand_back = decided_early || !bound_scan_norm_ok(qn, v.dim);   // (the same in every workgroup of the query)
    if (!hand_back && !idle) {
        QConst qc; qc.qn = 0.0; qc.qn32 = 0.0f;
        if constexpr (M == QV_COSINE) qc.qn = qn;
        const f4* tiles = reinterpret_cast<const f4*>(v.tiles);
        f4* mine = reinterpret_cast<f4*>(rbuf + (size_t)wave * v.dim4 * 4);
        for (uint32_t i = blockIdx.x * kScanWaves + wave; i < ns; i += active * kScanWaves) {   // (wave-uniform)
            const uint32_t row = cand[i];
            const f4* src = tiles + (size_t)(row >> 6) * v.dim4 * 64 + (row & 63);
            double rn = 0.0;
            if constexpr (MT<M>::needs_rnorm) rn = v.rnorm[row];
            for (uint32_t c0 = 0; c0 < v.dim4; c0 += 256) {
                f4 x[4];
#pragma unroll
                for (uint32_t u = 0; u < 4; u++) { const uint32_t c = c0 + u * 64 + lane; if (c < v.dim4) x[u] = __builtin_nontemporal_load(&src[(size_t)c * 64]); }
#pragma unroll
                for (uint32_t u = 0; u < 4; u++) { const uint32_t c = c0 + u * 64 + lane; if (c < v.dim4) mine[c] = x[u]; }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // the wave's own LDS writes before its reads of other lanes' chunks
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            typename MT<M>::A acc = 0;
            for (uint32_t c = 0; c < v.dim4; c++) {                    // ONE chain, element order: row_accumulate's
                const f4 r = mine[c];
                const Q* qq = q_lds + (size_t)c * 4;
                acc1<M>(acc, qq[0], r.x); acc1<M>(acc, qq[1], r.y); acc1<M>(acc, qq[2], r.z); acc1<M>(acc, qq[3], r.w);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // ... and those reads before the next survivor's writes
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) keys[i] = make_key(finalize<M>(acc, qc, rn), row);
        }
        // the slots past the count: dead keys, whatever an earlier search left there
        for (uint32_t i = ns + blockIdx.x * kScanBlock + threadIdx.x; i < kBoundWideCandCap; i += active * kScanBlock) keys[i] = kDeadKey;
    }
    __syncthreads();
    if (!idle) {
        if (threadIdx.x == 0) s_last = atomicAdd(&ctrl->ticket, 1u) == gridDim.x - 1 ? 1u : 0u;   // (behind this workgroup's reads of ctrl and the gate)
        __syncthreads();
    }
    return BoundWideWalk{s_last != 0u && threadIdx.x == 0, hand_back, ns, cnt};
}

// P8: the re-score behind the 8-bit stage (ctrl = that stage's words, next = the bfloat16 stage's): it answers — and clears the bfloat16 stage's
// flag for the redo behind —, or sets its own flag, the word the bfloat16 stage's launches are gated on.  gate (the bfloat16 stage behind the
// 8-bit one): as k_bound_rescore's.  keys [kBoundWideCandCap]; sel: [0] the live keys in front of keys[], [1] 1 = a stage has answered.
template <int M, bool P8>
__global__ void __launch_bounds__(kScanBlock)
k_bound_rescore_wide(IndexView v, const float* __restrict__ query, BoundCtrl* __restrict__ ctrl, const uint32_t* __restrict__ cand, uint32_t* __restrict__ stats,
                     uint64_t* __restrict__ keys, uint32_t* __restrict__ sel, uint32_t* gate, BoundCtrl* next) {
    if (gate != nullptr && *gate == 0u) return;
    const BoundWideWalk w = bound_rescore_wide_walk<M>(v, query, ctrl, cand, keys);
    if (!w.last) return;
    const bool hand_back = w.hand_back;
    const uint32_t ns = w.ns, cnt = w.cnt;
    ctrl->ticket = 0;                                                  // for the next launch on these words (stream order)
    if constexpr (P8) {
        if (!hand_back) { stats[kBoundWideStatsWord] = cnt; (void)atomicAdd(&stats[kBoundWideStatsWord + 2], 1u); next->flag = 0u; }
    } else {
        stats[kBoundWideStatsWord] = cnt;
        if (hand_back) (void)atomicAdd(&stats[kBoundWideStatsWord + 1], 1u);
        (void)atomicAdd(&stats[kBoundWideStatsWord + 2], 1u);
        if (gate != nullptr) *gate = 0u;                               // (every workgroup read it before it took its ticket)
    }
    ctrl->flag = hand_back ? 1u : 0u;                                  // the launches behind this one read it
    sel[0] = hand_back ? 0u : ns; sel[1] = hand_back ? 0u : 1u;
    ctrl->cand_cnt = 0; ctrl->thr_inv = 0;                             // zero, as the words are kept
}

// ---------------------------------------------------------------- the bound scan as a shared pass: 2 - 8 queries over the bfloat16 copy --
// Callers that arrive together share a pass (qv_coalesce.h), and a pass of 2 - 8 queries read the float32 tiles (k_flat_scan_mq) while the
// copy lay idle.  Here the copy is read ONCE for QB = 4 or 8 queries; interval, threshold, collect and exact re-score are the single-query
// path's, per query, so the answers are the exact scan's bits.
//   k_bound_prep_mq  the query block qblk[step][16][QB] in float32 (slots past nq: zeros) and |q_j| as the reference's float64 chain, once.
//   k_bound_scan_mq  k_bound_scan's walk — lane == row, a wave owns whole tiles, the lane's two 16-byte halves per step, each bfloat16
//                    widened once — with the query values as SCALAR operands (uniform loads of qblk: per dimension the QB values are
//                    contiguous, so a query PAIR is one 64-bit scalar operand of a packed float32 fma whose two halves are two queries'
//                    chains: 64 packed fmas + 16 widenings per step and lane at QB = 8 where one fma per query and element is 128 + 16).
//                    Each (query, row) sum is still ONE in-order chain of dim fmas, one rounding each: qv_bound.h's gamma as it stands.
//                    d_lo -> lo_all[q][n_tiles * 64]; d_hi -> per-query wave lists -> partial[q][grid][k], k_flat_scan_mq's layout.
//   k_merge_lists    per query over its upper-bound lists: its k-th entry is H (valid: the row is a row and the bound is finite).
//   k_bound_collect_mq / k_bound_rescore_mq   blockIdx.y / blockIdx.x = query: a candidate list, a counter (BoundCtrl::cand_cnt of its
//                    own, left zero) and a hand-back flag per query.  A query is handed back on its own grounds; launch_flat_redo_flagged
//                    behind the re-score redoes exactly the flagged ones with the exact scan, on the device.
// (Measured: profiles/LAB_r08_bound_scan_mq.md.)
constexpr uint32_t kBoundMqMax = 8;            // queries per shared pass (BoundCtrl x 8 behind kBoundCtrlWord fit the stream's 64 ticket words)
typedef float f2 __attribute__((ext_vector_type(2)));

template <int QB>
__global__ void __launch_bounds__(256)
k_bound_prep_mq(const float* __restrict__ queries, uint32_t nq, uint32_t dim, float* __restrict__ qblk, double* __restrict__ qnorm, uint32_t* __restrict__ stats,
                const uint32_t* __restrict__ gate = nullptr /* behind the 8-bit stage: the count of queries it handed on; zero = leave at once */) {
    if (gate != nullptr && *gate == 0u) return;
    __shared__ float s_q[kBoundMaxDim];
    const uint32_t nb = gridDim.x - QB;                                // blocks [0, nb): the block; [nb, nb + QB): one query's norm each
    if (blockIdx.x < nb) {
        const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i < dim * QB) {
            const uint32_t j = i % QB, d = i / QB;
            qblk[i] = j < nq ? queries[(size_t)j * dim + d] : 0.f;
        }
        if (i == 0 && gate == nullptr) stats[0] = 0;                   // the pass's largest survivor count (k_bound_rescore_mq; behind the 8-bit stage it holds that stage's)
        return;
    }
    const uint32_t j = blockIdx.x - nb;
    if (j >= nq) { if (threadIdx.x == 0) qnorm[j] = 0.0; return; }
    for (uint32_t i = threadIdx.x; i < dim; i += blockDim.x) s_q[i] = queries[(size_t)j * dim + i];
    __syncthreads();
    if (threadIdx.x == 0) {                                            // the reference's chain (distances.go:20), as k_bound_rescore walks it
        double ma = 0.0;
        for (uint32_t i = 0; i < dim; i++) { const double a = (double)s_q[i]; ma = __builtin_fma(a, a, ma); }
        qnorm[j] = __builtin_sqrt(ma);
    }
}

template <int QB, int U>
__device__ __forceinline__ void bound_block_mq(const u4* __restrict__ p, const float* __restrict__ qblk, uint32_t s0, f2 (&acc)[QB / 2]) {
    u4 x[2 * U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        x[2 * u] = __builtin_nontemporal_load(&p[(size_t)(s0 + u) * 128]);
        x[2 * u + 1] = __builtin_nontemporal_load(&p[(size_t)(s0 + u) * 128 + 32]);
    }
    __builtin_amdgcn_sched_barrier(0);                                 // all requests of the block ahead of the arithmetic (see row_accumulate)
#pragma unroll
    for (int u = 0; u < U; u++) {
        const f2* qq = reinterpret_cast<const f2*>(qblk + (size_t)(s0 + u) * 16 * QB);   // global, uniform -> scalar loads
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const u4 w = x[2 * u + h];
            const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int g = 0; g < 4; g++) {                              // bfloat16 -> float32 is a shift / a mask: exact
                const float r0 = __uint_as_float(ww[g] << 16), r1 = __uint_as_float(ww[g] & 0xFFFF0000u);
                const f2 rr0 = {r0, r0}, rr1 = {r1, r1};
#pragma unroll
                for (int j = 0; j < QB / 2; j++) acc[j] = __builtin_elementwise_fma(qq[(h * 8 + g * 2) * (QB / 2) + j], rr0, acc[j]);
#pragma unroll
                for (int j = 0; j < QB / 2; j++) acc[j] = __builtin_elementwise_fma(qq[(h * 8 + g * 2 + 1) * (QB / 2) + j], rr1, acc[j]);
            }
        }
    }
}

// The WIDE shared pass's tail (k_bound_scan_mq<., ., false, true>, k_bound_scan8_mq<., ., false, true>): bound_scan_tail_wide per query.  Every
// wave's list of every query of the pass is published as it stands, lists[j][grid][kScanWaves][64]; H_j is then the k-th smallest key of
// query j's grid x kScanWaves x 64 keys (one launch_select_topk over the nq arrays).  The argument written at bound_scan_tail_wide holds per
// query: query j's published keys are upper bounds of DISTINCT live rows — a row is in one wave's list of query j only —, any k of them
// cap query j's k-th distance, H_j is exact whenever no wave holds more than 64 of query j's k smallest and only looser otherwise, and
// fewer than k live keys leave query j without H_j (handed on, alone).  No ticket, no LDS: every slot of a query the pass holds is written
// by its own wave in every launch (a wave that walks no tile publishes the dead lists it started with); slots past nq are never read.
template <int QB>
__device__ __forceinline__ void bound_scan_tail_wide_mq(const uint64_t (&list)[QB], uint32_t nq, uint32_t wave, uint32_t lane, uint64_t* __restrict__ lists) {
#pragma unroll
    for (int j = 0; j < QB; j++)
        if ((uint32_t)j < nq) lists[(((size_t)j * gridDim.x + blockIdx.x) * kScanWaves + wave) * 64 + lane] = list[j];
}

// SETS (k_bound_scan_mq<., ., true>: a pass under filters, query j restricted to am_j = alive & set_j): the sets' (bits, words) pairs arrive as kernel
// arguments, as in k_rowset_scan_mq, and lane j keeps query j's — eight pairs held as scalars spilled 168 SGPRs there, and this kernel
// already spends its scalar file on the packed-fma query operands.  rowset_word for the wave's NEXT tile is fetched while the current one is
// walked and read back per query with readlane64 (wave-uniform again).  Bit `lane` of am_j gates query j's lower-bound word (a
// non-candidate writes 0xFFFFFFFF) and its upper-bound key (kDeadKey), so H_j is the k-th smallest upper bound over query j's OWN
// candidates and a set of fewer than k live rows has none (handed back).  A tile that no query selects is not requested — copy, rnorm,
// rres —; its nq x 64 lower-bound words are written as 0xFFFFFFFF (256 bytes per query against dim * 128 of copy): k_bound_collect_mq
// reads every word of a workspace that earlier searches have used, and stays as it is.  `first` is the first tile the wave READS.
// The interval arithmetic is untouched.  A masked call (one bitmap for all queries, in v.alive) is this form with a table of null sets.
// WIDE (k_bound_scan_mq<., ., false, true>, k_bound_scan8_mq<., ., false, true>: a shared pass at 65 <= k <= kBoundWideMaxK): the walk with a list
// length of 64 (k = 64 arrives as the argument), and the tail publishes every wave's list of every query — bound_scan_tail_wide per query
// (bound_scan_tail_wide_mq below): no merge of the workgroup's waves, no LDS.
template <int M, int QB, bool SETS = false, bool WIDE = false>
__global__ void __launch_bounds__(kScanBlock, 2)
k_bound_scan_mq(IndexView v, const float* __restrict__ qblk, const double* __restrict__ qnorm, uint32_t nq, uint32_t k,
                uint32_t* __restrict__ lo_all /* [nq][n_tiles * 64] */, uint64_t* __restrict__ partial /* [nq][grid][k]; WIDE: [nq][grid][kScanWaves][64] */, SetsArg<SETS> tab,
                const uint32_t* __restrict__ gate = nullptr /* as k_bound_prep_mq's */) {
    static_assert(!(SETS && WIDE), "the wide shared pass is unfiltered");
    if (gate != nullptr && *gate == 0u) return;
    extern __shared__ __align__(16) unsigned char smem[];
    uint64_t* wl = reinterpret_cast<uint64_t*>(smem);                  // [kScanWaves][QB][64] (WIDE: none)
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t steps = v.dim >> 4, tw = gridDim.x * kScanWaves, kth = k - 1;
    const size_t n = (size_t)v.n_tiles * 64;
    const double gamma = bound_scan_gamma(v.dim);
    const u4* plane = reinterpret_cast<const u4*>(v.plane) + ((lane >> 5) * 64 + (lane & 31));
    uint64_t list[QB], thr[QB];
    double qn[QB];
#pragma unroll
    for (int j = 0; j < QB; j++) { list[j] = kDeadKey; thr[j] = kDeadKey; qn[j] = qnorm[j]; }
    bool first = true;
    const bool mine = SETS && lane < nq;
    RowSetRef rs = RowSetRef{nullptr, 0, 0};
    uint64_t w_next = 0ull;
    if constexpr (SETS) {
        static_assert(QB <= (int)kBoundSets, "one table entry per query of the pass");
        rs = tab.e[mine ? lane : 0u];                                 // lane j: query j's set
        const uint32_t t0 = blockIdx.x * kScanWaves + wave;
        if (t0 < v.n_tiles) w_next = rowset_word(v.alive, rs, mine, t0);
    }
    for (uint32_t t = blockIdx.x * kScanWaves + wave; t < v.n_tiles; t += tw) {
        const uint64_t w = w_next;                                     // (SETS) lane j: am_j of this tile
        if constexpr (SETS) {
            if (t + tw < v.n_tiles) w_next = rowset_word(v.alive, rs, mine, t + tw);
            if (__ballot(w != 0ull) == 0ull) {                         // nobody's candidate in this tile
#pragma unroll
                for (int j = 0; j < QB; j++)
                    if ((uint32_t)j < nq) __builtin_nontemporal_store(0xFFFFFFFFu, &lo_all[(size_t)j * n + t * 64 + lane]);
                continue;
            }
        }
        f2 acc[QB / 2];
#pragma unroll
        for (int j = 0; j < QB / 2; j++) acc[j] = f2{0.f, 0.f};
        const u4* p = plane + (size_t)t * steps * 128;
        uint32_t s = 0;
        for (; s + 8 <= steps; s += 8) bound_block_mq<QB, 8>(p, qblk, s, acc);
        if (s + 4 <= steps) { bound_block_mq<QB, 4>(p, qblk, s, acc); s += 4; }
        if (s + 2 <= steps) { bound_block_mq<QB, 2>(p, qblk, s, acc); s += 2; }
        if (s < steps) bound_block_mq<QB, 1>(p, qblk, s, acc);
        const uint32_t row = t * 64 + lane;
        const double rn = v.rnorm[row];
        const float rr = v.rres[row];
        bool live_all = false;
        if constexpr (!SETS) live_all = (v.alive[t] >> lane) & 1ull;   // (dead rows and the last tile's padding: never candidates, never in a bound)
#pragma unroll
        for (int j = 0; j < QB; j++) {
            if ((uint32_t)j < nq) {                                    // (uniform) slots past nq produce nothing
                bool live;
                if constexpr (SETS) live = (readlane64(w, (uint32_t)j) >> lane) & 1ull; else live = live_all;
                float lo, hi;
                (void)bound_scan_interval<M>((j & 1) ? acc[j / 2].y : acc[j / 2].x, qn[j], rn, rr, v.dim, gamma, lo, hi);
                __builtin_nontemporal_store(live ? ord_f32(lo) : 0xFFFFFFFFu, &lo_all[(size_t)j * n + row]);
                const uint64_t key = live ? (((uint64_t)ord_f32(hi) << 32) | row) : kDeadKey;
                if (first) { list[j] = wave_sort64(key, lane); thr[j] = readlane64(list[j], kth); }
                else list_insert(list[j], thr[j], key, kth, lane);
            }
        }
        first = false;
    }
    if constexpr (WIDE) { bound_scan_tail_wide_mq<QB>(list, nq, wave, lane, partial); return; }
#pragma unroll
    for (int j = 0; j < QB; j++) wl[((size_t)wave * QB + j) * 64 + lane] = list[j];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int j = 0; j < QB; j++) {
            if ((uint32_t)j < nq) {
                for (uint32_t w = 1; w < kScanWaves; w++) list_insert(list[j], thr[j], lane < k ? wl[((size_t)w * QB + j) * 64 + lane] : kDeadKey, kth, lane);
                if (lane < k) partial[((size_t)j * gridDim.x + blockIdx.x) * k + lane] = list[j];
            }
        }
    }
}

// H of query blockIdx.y: the k-th entry of its merged upper-bound list (seed_rows / seed_dist [nq][k])
__global__ void __launch_bounds__(256)
k_bound_collect_mq(const uint32_t* __restrict__ lo_all, uint32_t n /* multiple of 64 */, uint32_t k, const uint32_t* __restrict__ seed_rows, const float* __restrict__ seed_dist,
                   BoundCtrl* __restrict__ ctrl, uint32_t* __restrict__ cand,
                   const uint32_t* __restrict__ hand = nullptr /* behind the 8-bit stage: only the queries it handed on (hand[j] != 0) are collected */) {
    const uint32_t j = blockIdx.y;
    if (hand != nullptr && hand[j] == 0u) return;
    const uint32_t H = ord_f32(seed_dist[(size_t)j * k + k - 1]);
    if (seed_rows[(size_t)j * k + k - 1] == 0xFFFFFFFFu || H >= 0xFF800000u) return;   // no H: k_bound_rescore_mq hands the query back
    bound_collect(lo_all + (size_t)j * n, n, H, &ctrl[j].cand_cnt, cand + (size_t)j * kBoundCandCap);
}

// STAGE 0: the pass on the bfloat16 copy alone.  STAGE 1: the 8-bit stage of a pass (k_bound_scan8_mq below): a query it decides is answered
// and counted here as a bound-scan search; every other one gets its hand-on word hand[j] set and the pass-wide count hand[kBoundMqMax]
// bumped — the words the bfloat16 stage behind is gated on (k_bound_prep8_mq cleared them).  STAGE 2: that bfloat16 stage: only the queries
// handed on are walked, counted and written; the others keep the answers they have.
template <int M, int STAGE = 0>
__global__ void __launch_bounds__(kScanBlock)
k_bound_rescore_mq(IndexView v, const float* __restrict__ queries, uint32_t k, const uint32_t* __restrict__ seed_rows, const float* __restrict__ seed_dist,
                   BoundCtrl* __restrict__ ctrl, const uint32_t* __restrict__ cand, uint32_t* __restrict__ flags, uint32_t* __restrict__ stats,
                   uint32_t* __restrict__ rows_out, float* __restrict__ dist_out, uint32_t* __restrict__ hand = nullptr) {
    const uint32_t j = blockIdx.x;
    if constexpr (STAGE == 2) { if (hand[j] == 0u) return; }
    const uint32_t cnt = ctrl[j].cand_cnt;
    const bool has_H = seed_rows[(size_t)j * k + k - 1] != 0xFFFFFFFFu && ord_f32(seed_dist[(size_t)j * k + k - 1]) < 0xFF800000u;
    bound_rescore_query<M>(v, queries + (size_t)j * v.dim, k, cnt, has_H, cand + (size_t)j * kBoundCandCap, rows_out + (size_t)j * k, dist_out + (size_t)j * k, [&](bool hand_back) {
        if constexpr (STAGE == 1) {
            (void)atomicMax(&stats[kBound8StatsWord], cnt);
            (void)atomicAdd(&stats[kBound8StatsWord + 2], 1u);
            if (hand_back) { (void)atomicAdd(&stats[kBound8StatsWord + 1], 1u); (void)atomicAdd(&hand[kBoundMqMax], 1u); }
            else { (void)atomicMax(&stats[0], cnt); (void)atomicAdd(&stats[2], 1u); }
            hand[j] = hand_back ? 1u : 0u;
            flags[j] = 0u;                                             // (the bfloat16 stage sets it if it hands the query back in turn)
        } else {
            (void)atomicMax(&stats[0], cnt);
            if (hand_back) (void)atomicAdd(&stats[1], 1u);
            (void)atomicAdd(&stats[2], 1u);
            flags[j] = hand_back ? 1u : 0u;                            // launch_flat_redo_flagged behind this launch reads them
        }
        ctrl[j].cand_cnt = 0;                                          // zero, as the words are kept
    });
}

// ---------------------------------------------------------------- the shared pass of 2 - 8 queries: reject rows on the 8-bit plane first --
// k_bound_scan8's stage for QB = 4 or 8 queries at once: the plane is read ONCE per pass, a quarter of the float32 bytes, and what the stage
// cannot decide for a query goes — that query alone — to the bfloat16 shared pass above, whose launches sit gated behind it.
//   k_bound_prep8_mq  one workgroup per query slot: k_bound_scan8's prologue (finiteness, max|q|, sq, the two int8 terms, qres rounded up,
//                     |q| as the reference's chain), written once: the terms as qterm[step][QB][hi 16 bytes, lo 16 bytes], the scalars as
//                     qpar[0 .. 8) = |q_j|, [8 .. 16) = sq_j, [16 .. 24) = qres_j.  Slots past nq hold zeros.  It clears the words the pass
//                     uses as flags: the hand-on words and their count, and the pass's survivor maxima in the counters.
//   k_bound_scan8_mq  k_bound_scan8's walk — lane == row, a wave owns whole tiles, one 16-byte load per lane and step, the 16 / 8 / 4 / 2 / 1
//                     ladder — with the query terms as SCALAR operands of the dot-product instruction (uniform loads of qterm, as
//                     k_bound_scan_mq reads its float32 block: 8 dwords per query and step).  Per (query, row) the four int32 partial sums of
//                     bound8_block, combined in int64, and bound_scan_interval8 as it stands.  d_lo -> lo_all[j][n_tiles * 64]; d_hi ->
//                     per-query wave lists -> partial[j][grid][k]: k_bound_scan_mq's layout, so k_merge_lists and k_bound_collect_mq follow.
//                     THE PRE-TEST: d_lo is computed first; when ord_f32(d_lo) is strictly above the distance word of the wave's current
//                     k-th upper bound of that query, the row's d_hi >= d_lo is above it too and list_insert would reject its key — so
//                     when that holds for every lane of the wave (ballot) d_hi is not computed at all.  The lists, H_j and the survivors are
//                     what they are without it; "unsure" rows (d_lo = -inf) are never skipped.  The first tile a wave walks is sorted outright.
//   k_bound_rescore_mq<., 1>, then the bfloat16 stage's five launches, each of which leaves at once when nothing was handed on.
// (Measured: profiles/LAB_r12_bound_scan8_mq.md.)
constexpr uint32_t kBound8MqHandWord = 16;     // in the pass's 64 flag words: [0, 8) the exact scan's flags, [16, 24) hand-on words, [24] their count
template <int QB>
__global__ void __launch_bounds__(kScanBlock)
k_bound_prep8_mq(const float* __restrict__ queries, uint32_t nq, uint32_t dim, int8_t* __restrict__ qterm, double* __restrict__ qpar, uint32_t* __restrict__ hand,
                 uint32_t* __restrict__ max_pass /* the pass's largest survivor count among the form's counters */,
                 uint32_t* __restrict__ max_stage8 /* ... and the 8-bit stage's own, where the form keeps one (the k <= 64 pass); else null */) {
    __shared__ float s_max[kScanWaves];
    __shared__ uint32_t s_bad[kScanWaves];
    __shared__ double s_res[kScanWaves];
    const uint32_t j = blockIdx.x;                                     // < QB
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (j == 0 && threadIdx.x <= kBoundMqMax) hand[threadIdx.x] = 0u;
    if (j == 0 && threadIdx.x == 0) { *max_pass = 0u; if (max_stage8 != nullptr) *max_stage8 = 0u; }   // the pass's largest survivor counts (k_bound_rescore_mq, k_bound_rescore_wide_mq)
    if (j >= nq) {
        for (uint32_t i = threadIdx.x; i < dim; i += blockDim.x) {
            qterm[(((size_t)(i >> 4) * QB + j) * 2) * 16 + (i & 15u)] = 0; qterm[(((size_t)(i >> 4) * QB + j) * 2 + 1) * 16 + (i & 15u)] = 0;
        }
        if (threadIdx.x == 0) { qpar[j] = 0.0; qpar[kBoundMqMax + j] = 1.0; qpar[2 * kBoundMqMax + j] = __builtin_nan(""); }
        return;
    }
    const float* __restrict__ query = queries + (size_t)j * dim;
    // as k_bound_scan8 quantises its query: sq = max|q_i| / 16256, qq = rint(q / sq) = 128 hi + lo; qres = |q - sq qq| rounded up
    float mx = 0.f; bool bad = false;
    for (uint32_t i = threadIdx.x; i < dim; i += blockDim.x) { const float x = query[i]; bad |= !((x - x) == 0.0f); mx = __builtin_fmaxf(mx, __builtin_fabsf(x)); }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mx = __builtin_fmaxf(mx, __shfl_xor(mx, m));
    const bool wbad = __ballot(bad) != 0ull;
    if (lane == 0) { s_max[wave] = mx; s_bad[wave] = wbad ? 1u : 0u; }
    __syncthreads();
    uint32_t anybad = 0;
    for (uint32_t w = 0; w < kScanWaves; w++) { mx = __builtin_fmaxf(mx, s_max[w]); anybad |= s_bad[w]; }
    const bool q_ok = !anybad && mx > 0.0f;
    const double sq = q_ok ? (double)mx / (double)kBound8QueryMax : 1.0;
    double r2 = 0.0;
    for (uint32_t i = threadIdx.x; i < dim; i += blockDim.x) {
        const double x = q_ok ? (double)query[i] : 0.0;
        const double qq = __builtin_rint(x / sq);                      // |qq| <= 16256
        const double hi = __builtin_rint(qq * (1.0 / 128.0)), lo = qq - 128.0 * hi;   // |hi| <= 127, |lo| <= 64: exact
        qterm[(((size_t)(i >> 4) * QB + j) * 2) * 16 + (i & 15u)] = (int8_t)(int)hi;
        qterm[(((size_t)(i >> 4) * QB + j) * 2 + 1) * 16 + (i & 15u)] = (int8_t)(int)lo;
        const double d = x - sq * qq;
        r2 = __builtin_fma(d, d, r2);
    }
    r2 = wave_sum_f64(r2);
    if (lane == 0) s_res[wave] = r2;
    double ma = 0.0;
    if (wave == kScanWaves - 1) {
        // |q| as the reference's chain (distances.go:20), one wave: 64 values per request, walked in order
        for (uint32_t b = 0; b < dim; b += 64) {
            const float x = b + lane < dim ? query[b + lane] : 0.f;
            const uint32_t n = dim - b < 64u ? dim - b : 64u;
            for (uint32_t e = 0; e < n; e++) { const double a = (double)__uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(x), e)); ma = __builtin_fma(a, a, ma); }
        }
    }
    __syncthreads();
    if (wave == kScanWaves - 1 && lane == 0) {
        double qres2 = 0.0;
        for (uint32_t w = 0; w < kScanWaves; w++) qres2 += s_res[w];
        qpar[j] = __builtin_sqrt(ma);
        qpar[kBoundMqMax + j] = sq;
        // (a query without a scale: every row comes out "unsure", no H, and the re-score hands the query on)
        qpar[2 * kBoundMqMax + j] = q_ok ? __builtin_sqrt(qres2) * (1.0 + 1e-9) + 1e-300 : __builtin_nan("");
    }
}

// acc[j][0 .. 3]: bound8_block's four partial sums for query j (hi terms in [0], [1], lo terms in [2], [3])
template <int QB, int U>
__device__ __forceinline__ void bound8_block_mq(const u4* __restrict__ p, const u4* __restrict__ qterm, uint32_t s0, i32 (&acc)[QB][4]) {
    u4 x[U];
#pragma unroll
    for (int u = 0; u < U; u++) x[u] = __builtin_nontemporal_load(&p[(size_t)(s0 + u) * 64]);
    __builtin_amdgcn_sched_barrier(0);                                 // all requests of the block ahead of the arithmetic (see row_accumulate)
#pragma unroll
    for (int u = 0; u < U; u++) {
        const u4* qt = qterm + (size_t)(s0 + u) * QB * 2;              // global, uniform -> scalar loads
#pragma unroll
        for (int j = 0; j < QB; j++) {
            const u4 h = qt[2 * j], l = qt[2 * j + 1];
            acc[j][0] = __builtin_amdgcn_sdot4((i32)h.x, (i32)x[u].x, acc[j][0], false);
            acc[j][1] = __builtin_amdgcn_sdot4((i32)h.y, (i32)x[u].y, acc[j][1], false);
            acc[j][0] = __builtin_amdgcn_sdot4((i32)h.z, (i32)x[u].z, acc[j][0], false);
            acc[j][1] = __builtin_amdgcn_sdot4((i32)h.w, (i32)x[u].w, acc[j][1], false);
            acc[j][2] = __builtin_amdgcn_sdot4((i32)l.x, (i32)x[u].x, acc[j][2], false);
            acc[j][3] = __builtin_amdgcn_sdot4((i32)l.y, (i32)x[u].y, acc[j][3], false);
            acc[j][2] = __builtin_amdgcn_sdot4((i32)l.z, (i32)x[u].z, acc[j][2], false);
            acc[j][3] = __builtin_amdgcn_sdot4((i32)l.w, (i32)x[u].w, acc[j][3], false);
        }
    }
}

// SETS (k_bound_scan8_mq<., ., true>: a pass under filters, query j restricted to am_j = alive & set_j): this walk under k_bound_scan_mq<., ., true>'s
// candidate handling.  Lane j < nq keeps query j's (bits, words) pair — in lanes, not scalars: the scalar file is spent on the query terms —,
// rowset_word for the wave's NEXT tile is in flight while the current one is walked, and am_j comes back per query with readlane64.  A tile
// no query selects requests nothing — plane8, rnorm, rscale8, rres8 — and its nq x 64 lower-bound words are written as 0xFFFFFFFF
// (k_bound_collect_mq reads every word of a reused workspace, and stays as it is).  Bit `lane` of am_j gates query j's lower-bound word
// (0xFFFFFFFF) and its upper-bound key (kDeadKey): H_j is the k-th smallest upper bound over query j's OWN candidates, and a set of fewer
// than k live rows has none (handed on).  `first` is the first tile the wave READS; a query with no candidate in it keeps its dead list and
// a threshold word of 0xFFFFFFFF, which is what sorting 64 dead keys gives.  The pre-test runs over query j's own candidates; a query with
// no candidate in a tile computes no interval at all.  A wave that reads no tile publishes dead lists.  The integer walk, the int64
// combination and bound_scan_interval8 are untouched.  A masked call (one bitmap in v.alive) is this form with a table of null sets.
// WIDE: as k_bound_scan_mq's — the walk and the pre-test with a list length of 64, the tail bound_scan_tail_wide_mq.
template <int M, int QB, bool SETS = false, bool WIDE = false>
__global__ void __launch_bounds__(kScanBlock, 2)
k_bound_scan8_mq(IndexView v, const u4* __restrict__ qterm, const double* __restrict__ qpar, uint32_t nq, uint32_t k,
                 uint32_t* __restrict__ lo_all /* [nq][n_tiles * 64] */, uint64_t* __restrict__ partial /* [nq][grid][k]; WIDE: [nq][grid][kScanWaves][64] */, SetsArg<SETS> tab) {
    static_assert(!(SETS && WIDE), "the wide shared pass is unfiltered");
    extern __shared__ __align__(16) unsigned char smem[];
    uint64_t* wl = reinterpret_cast<uint64_t*>(smem);                  // [kScanWaves][QB][64] (WIDE: none)
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t steps = v.dim >> 4, tw = gridDim.x * kScanWaves, kth = k - 1;
    const size_t n = (size_t)v.n_tiles * 64;
    const u4* plane = reinterpret_cast<const u4*>(v.plane8) + lane;
    uint64_t list[QB], thr[QB];
#pragma unroll
    for (int j = 0; j < QB; j++) { list[j] = kDeadKey; thr[j] = kDeadKey; }
    bool first = true;
    const bool mine = SETS && lane < nq;
    RowSetRef rs = RowSetRef{nullptr, 0, 0};
    uint64_t w_next = 0ull;
    if constexpr (SETS) {
        static_assert(QB <= (int)kBoundSets, "one table entry per query of the pass");
        rs = tab.e[mine ? lane : 0u];                                 // lane j: query j's set
        const uint32_t t0 = blockIdx.x * kScanWaves + wave;
        if (t0 < v.n_tiles) w_next = rowset_word(v.alive, rs, mine, t0);
    }
    for (uint32_t t = blockIdx.x * kScanWaves + wave; t < v.n_tiles; t += tw) {
        const uint64_t w = w_next;                                     // (SETS) lane j: am_j of this tile
        if constexpr (SETS) {
            if (t + tw < v.n_tiles) w_next = rowset_word(v.alive, rs, mine, t + tw);
            if (__ballot(w != 0ull) == 0ull) {                         // nobody's candidate in this tile
#pragma unroll
                for (int j = 0; j < QB; j++)
                    if ((uint32_t)j < nq) __builtin_nontemporal_store(0xFFFFFFFFu, &lo_all[(size_t)j * n + t * 64 + lane]);
                continue;
            }
        }
        const uint32_t row = t * 64 + lane;
        const double rn = v.rnorm[row];                                // (requested ahead of the tile's bytes: there when the sums are)
        const float sc = v.rscale8[row], rr = v.rres8[row];
        bool live_all = false;
        if constexpr (!SETS) live_all = (v.alive[t] >> lane) & 1ull;   // (dead rows and the last tile's padding: never candidates, never in a bound)
        i32 acc[QB][4];
#pragma unroll
        for (int j = 0; j < QB; j++) { acc[j][0] = 0; acc[j][1] = 0; acc[j][2] = 0; acc[j][3] = 0; }
        const u4* p = plane + (size_t)t * steps * 64;
        uint32_t s = 0;
        for (; s + 16 <= steps; s += 16) bound8_block_mq<QB, 16>(p, qterm, s, acc);
        if (s + 8 <= steps) { bound8_block_mq<QB, 8>(p, qterm, s, acc); s += 8; }
        if (s + 4 <= steps) { bound8_block_mq<QB, 4>(p, qterm, s, acc); s += 4; }
        if (s + 2 <= steps) { bound8_block_mq<QB, 2>(p, qterm, s, acc); s += 2; }
        if (s < steps) bound8_block_mq<QB, 1>(p, qterm, s, acc);
#pragma unroll
        for (int j = 0; j < QB; j++) {
            if ((uint32_t)j < nq) {                                    // (uniform) slots past nq produce nothing
                bool live;
                if constexpr (SETS) {
                    const uint64_t am = readlane64(w, (uint32_t)j);    // wave-uniform again
                    if (am == 0ull) {                                  // not this query's tile: no interval; (first) the list and the threshold stay dead
                        __builtin_nontemporal_store(0xFFFFFFFFu, &lo_all[(size_t)j * n + row]);
                        continue;
                    }
                    live = (am >> lane) & 1ull;
                } else live = live_all;
                // (each partial sum exact in int32: dim <= kBoundMaxDim)
                const long long isum = ((long long)acc[j][0] + (long long)acc[j][1]) * 128ll + ((long long)acc[j][2] + (long long)acc[j][3]);
                const double qn = qpar[j], sq = qpar[kBoundMqMax + j], qres = qpar[2 * kBoundMqMax + j];   // uniform
                float lo, hi;
                (void)bound_scan_interval8<M>(isum, sq, qn, qres, rn, sc, rr, v.dim, lo, hi);   // (only d_lo is used of this call: d_hi's chain is dead code here)
                const uint32_t olo = live ? ord_f32(lo) : 0xFFFFFFFFu;
                __builtin_nontemporal_store(olo, &lo_all[(size_t)j * n + row]);
                if (first) {
                    (void)bound_scan_interval8<M>(isum, sq, qn, qres, rn, sc, rr, v.dim, lo, hi);
                    const uint64_t key = live ? (((uint64_t)ord_f32(hi) << 32) | row) : kDeadKey;
                    list[j] = wave_sort64(key, lane); thr[j] = readlane64(list[j], kth);
                } else if (__ballot(live && olo <= (uint32_t)(thr[j] >> 32)) != 0ull) {   // the pre-test: nobody below the k-th upper bound -> no d_hi, no insert
                    (void)bound_scan_interval8<M>(isum, sq, qn, qres, rn, sc, rr, v.dim, lo, hi);
                    const uint64_t key = live ? (((uint64_t)ord_f32(hi) << 32) | row) : kDeadKey;
                    list_insert(list[j], thr[j], key, kth, lane);
                }
            }
        }
        first = false;
    }
    if constexpr (WIDE) { bound_scan_tail_wide_mq<QB>(list, nq, wave, lane, partial); return; }
#pragma unroll
    for (int j = 0; j < QB; j++) wl[((size_t)wave * QB + j) * 64 + lane] = list[j];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int j = 0; j < QB; j++) {
            if ((uint32_t)j < nq) {
                for (uint32_t w = 1; w < kScanWaves; w++) list_insert(list[j], thr[j], lane < k ? wl[((size_t)w * QB + j) * 64 + lane] : kDeadKey, kth, lane);
                if (lane < k) partial[((size_t)j * gridDim.x + blockIdx.x) * k + lane] = list[j];
            }
        }
    }
}

// ---------------------------------------------------------------- the shared pass of 2 - 8 queries, 65 <= k <= 1024: the wide form --
// The wide form of the shared bound pass: the two stage-1 kernels above up to their tail (their WIDE instantiations, a list length of 64, the
// copy or the plane read ONCE for the pass), and behind them the single wide form's funnel, per query:
//   launch_select_topk          one launch over the nq arrays of published keys (n = stride = grid x kScanWaves x 64, kk = k): the k-th
//                               output of query j is H_j.
//   k_bound_collect_wide_mq     grid (cgrid, nq): bound_collect against H_j with a list of QV_BOUND_WIDE_CAND_CAP rows per query; workgroup 0 of
//                               query j leaves H_j in ctrl[j].thr_inv (zero = the k-th key is dead or not finite: no H_j).
//   k_bound_rescore_wide_mq     grid (rgrid, nq): k_bound_rescore_wide's wave-per-survivor chain — the exact scan's bits — per query into
//                               keys[j][cap], dead keys behind the count.  Query j's LAST workgroup (a ticket in ctrl[j]) decides for
//                               query j alone: counts[j] (the live keys in front of keys[j]; zero for a query that is not answered here),
//                               the hand-on word or the redo's flag, the counters; it leaves ctrl[j] zero.
//   launch_select_topk_counted  ONE launch over all nq key lists ends the pass, whichever stage answered each query, and
//   launch_flat_select_redo     redoes the queries no stage could decide — the list overflowed, no finite H_j, a norm bound_scan_norm_ok
//                               declines — through the key-per-row path, alone.  The counted selection runs over EVERY query, with a count
//                               of zero for a query handed back, and BEFORE the redo: the redo's scatter is the last writer of a handed-back
//                               query's outputs (stream order), so those are the redo's.
// With the 8-bit plane first (STAGE 1) a query that stage cannot decide — the above, or a query it cannot quantise (no H_j) — is handed ON to
// the bfloat16 stage (STAGE 2), whose launches are gated: hand[j] per query, and hand[kBoundMqMax] = nq or 0 for the launches that take one
// word for the whole pass (launch_select_topk's d_active reads "the first *d_active queries": the hand-on COUNT would cut the pass short).
// Nothing is read on the host.
// Counters (kBoundWideMqStatsWord; none of the other groups moves): [13] the largest survivor count among the pass's queries, each in the stage
// that ANSWERED it — a maximum over the stages that answered: the prep kernel of the pass's first stage clears it, the 8-bit stage's
// maximum stays when the bfloat16 stage runs for a handed-on query, and a query handed back to the key-per-row path adds nothing;
// [14] queries handed back to the key-per-row path; [15] queries that took the form.
__global__ void __launch_bounds__(256)
k_bound_collect_wide_mq(const uint32_t* __restrict__ lo_all /* [nq][n] */, uint32_t n /* multiple of 64 */, uint32_t k, const uint32_t* __restrict__ seed_rows, const float* __restrict__ seed_dist /* [nq][k] sorted */,
                        BoundCtrl* __restrict__ ctrl, uint32_t* __restrict__ cand /* [nq][kBoundWideCandCap] */,
                        const uint32_t* __restrict__ hand /* behind the 8-bit stage: only the queries it handed on (hand[j] != 0) are collected; null: all */) {
    const uint32_t j = blockIdx.y;
    if (hand != nullptr && hand[j] == 0u) return;
    const uint32_t H = ord_f32(seed_dist[(size_t)j * k + k - 1]);
    const bool has_H = seed_rows[(size_t)j * k + k - 1] != 0xFFFFFFFFu && H < 0xFF800000u;   // the k-th published key is a row's, and its bound finite
    if (blockIdx.x == 0 && threadIdx.x == 0) ctrl[j].thr_inv = has_H ? ~H : 0u;   // (the re-score behind reads it; cand_cnt is zero: the words are kept so)
    if (!has_H) return;
    bound_collect(lo_all + (size_t)j * n, n, H, &ctrl[j].cand_cnt, cand + (size_t)j * kBoundWideCandCap, kBoundWideCandCap);
}

// STAGE as k_bound_rescore_mq's: 0 the bfloat16 pass alone; 1 the 8-bit stage in front (a query it decides is answered and counted, every
// other one gets hand[j] set and hand[kBoundMqMax] = nq); 2 the bfloat16 stage behind it (only handed-on queries are walked: an answered
// query keeps its keys and its count).  flags[j]: the key-per-row redo's; counts[j]: the counted selection's.
constexpr uint32_t kBoundWideMqCountWord = 32;     // in the pass's 64 flag words: [32, 40) the live keys in front of keys[j]
template <int M, int STAGE>
__global__ void __launch_bounds__(kScanBlock)
k_bound_rescore_wide_mq(IndexView v, const float* __restrict__ queries, BoundCtrl* __restrict__ ctrl_all, const uint32_t* __restrict__ cand_all, uint32_t* __restrict__ stats,
                        uint64_t* __restrict__ keys_all /* [nq][kBoundWideCandCap] */, uint32_t* __restrict__ flags, uint32_t* __restrict__ hand, uint32_t* __restrict__ counts) {
    const uint32_t j = blockIdx.y;
    if constexpr (STAGE == 2) { if (hand[j] == 0u) return; }          // (every workgroup of an answered query: no ticket is taken for it)
    BoundCtrl* ctrl = ctrl_all + j;
    const BoundWideWalk w = bound_rescore_wide_walk<M>(v, queries + (size_t)j * v.dim, ctrl, cand_all + (size_t)j * kBoundWideCandCap, keys_all + (size_t)j * kBoundWideCandCap);
    if (!w.last) return;
    const bool hand_back = w.hand_back;
    const uint32_t ns = w.ns, cnt = w.cnt;
    ctrl->ticket = 0;                                                  // for the next launch on these words (stream order)
    const bool answered = !hand_back;
    if (answered) (void)atomicMax(&stats[kBoundWideMqStatsWord], cnt);
    if constexpr (STAGE == 1) {
        if (answered) (void)atomicAdd(&stats[kBoundWideMqStatsWord + 2], 1u);
        else hand[kBoundMqMax] = gridDim.y;                            // nq, not a count (see above); every handing-on query writes the same word
        hand[j] = answered ? 0u : 1u;
        flags[j] = 0u;                                                 // (the bfloat16 stage sets it if it hands the query back in turn)
    } else {
        if (hand_back) (void)atomicAdd(&stats[kBoundWideMqStatsWord + 1], 1u);
        (void)atomicAdd(&stats[kBoundWideMqStatsWord + 2], 1u);
        flags[j] = hand_back ? 1u : 0u;                                // launch_flat_select_redo behind the counted selection reads them
    }
    counts[j] = answered ? ns : 0u;
    ctrl->cand_cnt = 0; ctrl->thr_inv = 0;                             // zero, as the words are kept
}

// The bound scan (k_bound_scan / k_bound_rescore above): one query, a fused-list k, cosine or dot, the bfloat16 copy at hand, a width the copy
// covers in whole 16-dimension steps.  Automatic from kBoundScanMinRows rows (measured: profiles/LAB_r07_bound_scan.md); the index's setter
// (IndexView::bound_scan) or QV_BOUND_SCAN = 1 takes it whenever it applies, 2 never.
// 2 - 8 queries (k_bound_scan_mq): the same conditions, and nq planes of lower bounds that stay under 2 GiB.  Its automatic rule is a floor on
// rows that depends on the width — every query pays 8 bytes per row for its lower bounds whatever the width — per QB: the smallest measured
// shape from which the path wins at every measured nq and k of that QB (profiles/LAB_r08_bound_scan_mq.md); narrower than
// kBoundMqNarrowDim it is never automatic.
// A Euclidean index that holds the planes (the rule code QV_RULE_L2_PLANES; plain QV_L2 never): the same conditions, the same bytes streamed and
// a few more flops per row for the interval.  "always" takes whatever cosine and dot take.  AUTOMATIC: only cells that were measured for it, a
// cell kept where the arm beat the arm it replaces by more than both arms' spread at every measured k (profiles/LAB_r14_bound_scan_l2.md;
// 1, 2, 4, 8 queries, k = 1, 10, 64, unfiltered and under a where-filter selecting 10 %, which the host counts as every tile a candidate).
// us per call, exact / bfloat16 first / 8-bit first, one query, k = 1, 10, 64:
//   768 dims   300 k 145 / 108 / 104, 149 / 116 / 125, 184 / 178 / 244      1M 455 / 269 / 189, 458 / 271 / 208, 489 / 331 / 355
//              3M 1335 / 728 / 425, 1340 / 730 / 433, 1368 / 789 / 596      10M 4462 / 2324 / 1248, 4458 / 2331 / 1273, 4485 / 2388 / 1450
//   128 dims   10M 740 / 453 / 257, 743 / 458 / 262, 778 / 497 / 317
// bfloat16 first won all 120 cells; 8-bit first lost at 300 k, at 1M unfiltered with k = 64, and with 8 queries at 10M x 128 — cosine's losses, all
// below the 8-bit floors below, which therefore hold for it unchanged.  Two constants of its own, where dot's floors accept cells that were
// not measured for it: ONE unfiltered query on rows narrower than 768 dimensions is taken from 10M rows of 128 dimensions or more only (dot: any
// width from 300 k rows; 1M x 128 was not measured here), and a FILTERED search only with nine tenths of the tiles holding a candidate (dot: one
// query down to a tenth, 2 - 4 queries at 10M rows down to a fifth; sparse sets were not measured here).
constexpr uint32_t kBoundL2NarrowDim = 128, kBoundL2NarrowRows = 10000000, kBoundL2WideDim = 768;
constexpr uint32_t kBoundScanMinRows = 300000;   // one query, us, exact / bound scan at k = 1, 10, 64: 100 k x 768 65 / 63, 66 / 70, 86 / 122; 300 k x 768 154 / 107, 158 / 114, 190 / 169; 1M x 128 89 / 64, 93 / 68, 134 / 114
// us per call, exact (k_flat_scan_mq) / bound, at k = 1, 10, 64:
//   QB = 4   300 k x 768  nq 2: 195 / 154, 204 / 160, 273 / 223; nq 4: 193 / 160, 207 / 175, 276 / 271      1M x 128  nq 4: 97 / 93, 117 / 103, 214 / 216 (a loss)
//            10M x 128    nq 2: 781 / 527, 793 / 532, 907 / 593; nq 4: 790 / 575, 793 / 587, 913 / 711
//   QB = 8   300 k x 768  nq 8: 232 / 233, 254 / 264, 370 / 427 (losses)      1M x 768  nq 5: 526 / 449, 545 / 464, 695 / 598; nq 8: 526 / 456, 542 / 473, 697 / 694
//            1M x 128     nq 8: 122 / 124, 145 / 157, 330 / 367 (losses)      10M x 128 nq 5: 888 / 638, 892 / 657, 1162 / 849; nq 8: 869 / 734, 905 / 775, 1161 / 1093
constexpr uint32_t kBoundMqMinDim = 768, kBoundMqMinRows4 = 300000, kBoundMqMinRows8 = 1000000;   // rows of at least 768 dimensions: QB = 4 (2 - 4 queries), QB = 8 (5 - 8)
constexpr uint32_t kBoundMqNarrowDim = 128, kBoundMqNarrowRows = 10000000;                        // 128 <= dim < 768 (nothing between was measured): both QB
// The 8-bit stage in front of it (k_bound_scan8): one unfiltered query the bound scan takes, on an index that holds the 8-bit plane.  The index's
// plane setter (IndexView::bound_plane) or QV_BOUND_PLANE = 1 puts it first whenever that holds, 2 never; automatic from the smallest
// measured row count from which 8-bit-first beats bfloat16-first at every measured k — never below kBoundScanMinRows, so a corpus under
// that floor runs what it ran before whatever mode forces the bound scan itself.  profiles/LAB_r10_bound_scan_8bit.md; us per query,
// bfloat16 first / 8-bit first, at k = 1, 10, 64 (the 8-bit stage passes on 3 - 4 times the rows, and one workgroup walks them: its
// k = 64 figures carry 0.1 - 0.15 ms of re-score):
//   768 dims   300 k 109 / 106, 117 / 124, 173 / 276 (losses)   1M 275 / 188, 277 / 209, 339 / 361 (a loss at k = 64)
//              3M 752 / 436, 737 / 456, 799 / 618                10M 2386 / 1263, 2352 / 1269, 2417 / 1457
//   128 dims   1M 62 / 53, 66 / 58, 111 / 113 (a loss at k = 64)  10M 457 / 259, 462 / 265, 502 / 318
// narrower than kBound8NarrowDim nothing was measured: never automatic.
constexpr uint32_t kBound8MinDim = 768, kBound8MinRows = 3000000;            // rows of at least 768 dimensions
constexpr uint32_t kBound8NarrowDim = 128, kBound8NarrowRows = 10000000;     // 128 <= dim < 768 (nothing between was measured)
// The 8-bit stage in front of an UNFILTERED shared pass of 2 - 8 queries (k_bound_scan8_mq): a pass the bound scan takes (asked with the copy
// held: the stage never starts a pass the bound scan would not take), the plane held, and the index's shared-pass plane setter
// (IndexView::bound_plane_mq) or QV_BOUND_PLANE_MQ — a knob of its own — allows it: 1 whenever that holds, 2 never.  Automatic: per QB the
// smallest measured row count from which 8-bit-first beat bfloat16-first at every measured k and nq of that QB in both rounds, never below
// the shared pass's own floors; profiles/LAB_r12_bound_scan8_mq.md.
// us per call, bfloat16 first / 8-bit first, at k = 1, 10, 64 (the slower round of the 8-bit arm against the faster of the bfloat16 arm):
//   QB = 4   768 dims   300 k  nq 2: 152 / 132, 161 / 146, 225 / 310; nq 4: 161 / 139, 172 / 160, 269 / 360 (losses at k = 64)
//                       1M     nq 2: 318 / 209, 324 / 236, 392 / 399; nq 4: 334 / 225, 347 / 258, 443 / 474 (losses at k = 64)
//                       3M     nq 2: 777 / 442, 787 / 473, 849 / 645; nq 4: 797 / 462, 814 / 498, 907 / 722
//                       10M    nq 2: 2421 / 1297, 2421 / 1314, 2500 / 1506; nq 4: 2470 / 1350, 2484 / 1371, 2590 / 1630
//            128 dims   10M    nq 2: 468 / 302, 473 / 320, 531 / 435; nq 4: 514 / 362, 522 / 419, 660 / 643
//   QB = 8   768 dims   300 k  nq 5: 228 / 173, 246 / 198, 362 / 414; nq 8: 234 / 184, 264 / 227, 426 / 489 (losses at k = 64)
//                       1M     nq 5: 456 / 269, 468 / 314, 599 / 572; nq 8: 465 / 291, 475 / 350, 695 / 690 (k = 64: 5 % and 1 %, no gain to speak of: declined)
//                       3M     nq 5: 1078 / 557, 1100 / 620, 1269 / 935; nq 8: 1114 / 607, 1146 / 694, 1289 / 1113
//                       10M    nq 5: 3342 / 1663, 3352 / 1740, 3566 / 2144; nq 8: 3461 / 1794, 3491 / 1996, 3805 / 2536
//            128 dims   10M    nq 5: 608 / 493, 628 / 569, 833 / 848; nq 8: 721 / 619, 760 / 741, 1086 / 1166 (losses at k = 64: QB = 8 is never automatic below 768 dimensions)
constexpr uint32_t kBound8MqMinDim = 768, kBound8MqMinRows4 = 3000000, kBound8MqMinRows8 = 3000000;   // rows of at least 768 dimensions, QB = 4 / QB = 8
constexpr uint32_t kBound8MqNarrowDim = 128, kBound8MqNarrowRows4 = 10000000, kBound8MqNarrowRows8 = 0;   // 128 <= dim < 768 (nothing between was measured); 0: never automatic
// Under a filter (a candidate bitmap in v.alive, or a row set per query): candidate_tiles = the tiles that hold a candidate of any query of
// the pass, as the host knows it without a device read (an upper bound: sets count their non-empty words, tombstones are not subtracted, a pass
// takes min(n_tiles, the sum over its queries) — so eight queries naming ONE striped set look like eight distinct ones).  "always" takes
// the path whenever the unfiltered conditions hold, "never" never.  Automatic: the cells of profiles/LAB_r09_bound_scan_filtered.md in which
// "always" beat the exact filtered scan by more than both arms' spread at k = 10 AND 64 (or, where said, at k = 10 only), for every kind of
// set that maps to the same host-side inputs; measured at 768 dimensions only, so narrower rows are declined; no floor below the
// unfiltered ones.  us per call, exact / bound, 768 dims, k = 10 and 64 (f = candidate_tiles / tiles as the host computes it):
//   one query     300 k: f 1.0 167 / 125, 201 / 181; one tile in ten 167 / 64, 201 / 122       1M: f 1.0 460 / 286, 496 / 349; one tile in ten 457 / 80, 489 / 137
//   QB = 4        300 k: nq 2 170 / 166, 212 / 230; nq 4 176 / 179, 250 / 274 (losses: declined below 1M)
//                 1M: f >= 0.9 nq 2 466 / 331, 506 / 398; nq 4 472 / 355, 551 / 451; striped sets (f 0.2 / 0.4) nq 2 126 / 141, nq 4 same set 111 / 140 (losses)
//                 10M: nq 2 4406 / 2496; nq 4 4406 / 2670; striped (f 0.2) nq 2 1251 / 697, same set 671 / 439
//   QB = 8 (nq 8) 1M: f 1.0 k = 10 557 / 486, density 0.01 one set 455 / 429; k = 64 740 / 702 but density 0.01 one set 477 / 495 (a loss with the same
//                 inputs: k > 10 declined); striped f 0.8 distinct 416 / 390, one set 171 / 226 (a loss: f < 0.9 declined)
//                 10M: f 1.0 5044 / 3819, 5373 / 4088; striped f 0.8 distinct 2806 / 2323, one set 912 / 917 (a loss: f < 0.9 declined)
//   nq 3 and 5 - 7 were not run: the bound pass gets cheaper with fewer queries (a lower-bound plane and a collect each) while the exact pass of
//   a QB costs the same at any fill (LAB_r08: 526 / 526 us at nq 5 / 8), so they are bracketed by the nq = 4 and nq = 8 cells.
constexpr uint32_t kBoundFiltMinDim = 768, kBoundFiltMqRows = 1000000, kBoundFiltBigRows = 10000000, kBoundFiltQb8SmallK = 10;
// The 8-bit stage in front of a FILTERED single query (k_bound_scan8<., true>): whenever the filtered bound rule takes the search (asked with
// the copy held: the stage never starts a search the bound scan would not take), one query, the plane held, and the index's filtered plane
// setter (IndexView::bound_plane_filtered) or QV_BOUND_PLANE_FILTERED — a knob of its own, independent of the unfiltered one — allows it:
// 1 whenever that holds, 2 never.  Automatic: per candidate fraction f = candidate_tiles / tiles the host can tell apart, the smallest
// measured row count from which 8-bit-first beat the parent commit's library (bfloat16 first) by more than both arms' spread at EVERY
// measured k, never below the unfiltered 8-bit floor; 768 dimensions only, so narrower rows are declined.
// profiles/LAB_r11_bound_scan8_filtered.md; us per call, parent / 8-bit first, 768 dims, k = 1, 10, 64 (four runs each, spreads <= 8 us):
//   f >= 0.9   every tile          1M 272 / 189, 278 / 211, 340 / 362 (a loss at k = 64)   3M 732 / 429, 740 / 458, 800 / 618   10M 2326 / 1248, 2332 / 1269, 2399 / 1458
//              a random 1 % set    1M 177 / 142, 183 / 152, 233 / 229                      3M 425 / 273, 434 / 293, 489 / 392   10M 1233 / 690, 1241 / 712, 1298 / 829
//              where, 10 % sel.    1M 273 / 193, 279 / 211, 336 / 305                      3M 739 / 436, 746 / 464, 804 / 576   10M 2352 / 1274, 2358 / 1299, 2412 / 1404
//              where, 100 % sel.   1M 273 / 193, 282 / 215, 345 / 366 (a loss at k = 64)   3M 739 / 438, 748 / 466, 807 / 626   10M 2350 / 1274, 2355 / 1296, 2423 / 1485
//   f = 0.1    one tile in ten     1M 70 / 88, 75 / 107, 132 / 206 (losses)                3M 237 / 158, 248 / 186, 370 / 369 (k = 64: no gain)
//                                  10M 295 / 217, 303 / 235, 362 / 365 (a loss at k = 64): declined at every row count
//   0.1 < f < 0.9 was not measured: declined.  So: f >= 0.9 from kBound8MinRows rows of kBound8MinDim dimensions or more.
// The 8-bit stage in front of a FILTERED shared pass of 2 - 8 queries (k_bound_scan8_mq<., ., true>: a mask, a row set per query, where-filters,
// the row-set front's shared passes): whenever the filtered bound rule takes the pass (asked with the copy held: the stage never starts a pass
// the filtered bound scan would not take), the plane held, and the index's setter for such passes (IndexView::bound_plane_filtered_mq) or
// QV_BOUND_PLANE_FILTERED_MQ — a knob of its own, independent of the three others — allows it: 1 whenever that holds, 2 never.
// Automatic: a cell is taken only when 8-bit first beat bfloat16 first at every measured k, the slower 8-bit round against the faster
// bfloat16 round, by more than both arms' round-to-round spread; never above what the unfiltered pass's 8-bit floors allow for the same nq, never below
// kBound8MinDim dimensions.  profiles/LAB_r13_bound_scan8_filtered_mq.md; us per call, bfloat16 first / 8-bit first (the faster bfloat16 round
// against the slower 8-bit round), 768 dims, k = 1, 10, 64; f = candidate_tiles / tiles as the host computes it:
//   f = 1.0   null sets         1M   nq 2: 317 / 210, 323 / 237, 395 / 400; nq 4: 332 / 224, 349 / 258, 443 / 474; nq 8: 464 / 293, 474 / 357, 691 / 695 (losses at k = 64)
//                               3M   nq 2: 777 / 468, 788 / 496, 853 / 666; nq 4: 799 / 511, 813 / 548, 910 / 768; nq 5: 1082 / 594, 1103 / 651, 1264 / 952; nq 8: 1112 / 645, 1154 / 727, 1292 / 1135
//                               10M  nq 2: 2440 / 1294, 2447 / 1312, 2519 / 1508; nq 4: 2502 / 1348, 2508 / 1371, 2621 / 1622; nq 5: 3370 / 1635, 3399 / 1723, 3581 / 2142; nq 8: 3491 / 1788, 3524 / 2021, 3818 / 2523
//             a random 1 % set per query   1M nq 4: 307 / 205, 318 / 228, 360 / 302; nq 8: 462 / 272, 461 / 308, 526 / 404   3M nq 4: 764 / 485, 772 / 508, 827 / 613; nq 8: 1114 / 605, 1143 / 651, 1100 / 787
//                               10M  nq 4: 2364 / 1261, 2367 / 1288, 2448 / 1451; nq 8: 3499 / 1717, 3527 / 1779, 3664 / 2003
//             where, 10 % each  1M   nq 4: 343 / 235, 354 / 268, 428 / 405; nq 8: 503 / 328, 515 / 386, 659 / 588   3M nq 4: 848 / 554, 858 / 586, 932 / 749; nq 8: 1212 / 725, 1249 / 808, 1301 / 1101
//                               10M  nq 4: 2645 / 1472, 2659 / 1510, 2733 / 1697; nq 8: 3846 / 2114, 3890 / 2240, 4077 / 2741
//   one striped set, one tile in ten, named by every query (f = 0.1 nq: 0.2 / 0.4 / 0.5 / 0.8)
//                               1M   nq 2: 119 / 103, 122 / 123, 181 / 224; nq 4: 122 / 111, 133 / 134, 212 / 300; nq 8: 198 / 150, 215 / 182, 340 / 397 (losses from k = 10 on)
//                               3M   nq 2: 364 / 233, 376 / 269, 511 / 469; nq 4: 386 / 264, 406 / 313, 589 / 574; nq 8: 1005 / 449, 1048 / 530, 1209 / 904
//                               10M  nq 2: 390 / 269, 399 / 294, 474 / 447; nq 4: 426 / 302, 441 / 346, 554 / 544; nq 8: 875 / 458, 906 / 532, 1106 / 832
//             (wins at 3M and 10M at every k, but 2 - 6 % at k = 64 for 2 - 4 queries: no gain to speak of there, and nothing between these
//              fractions and 0.9 was measured with distinct sets: f < 0.9 is declined)
// A where-filter is counted as f = 1.0 whatever it selects (the host cannot know), and only one selecting 10 % was measured: a very selective
// predicate, whose exact row-set scan reads next to nothing, is an UNMEASURED cell that AUTO takes — the bound pass still writes and collects
// nq x tiles x 256 bytes of lower-bound words (0.3 GB, written and read again, for 8 queries at 10M rows).  "bf16" restores the earlier routing for such hosts.
// So: f >= 0.9 from 3 000 000 rows of 768 dimensions or more, both QB; 1M loses at k = 64 with every tile a candidate.  Spreads <= 83 us at 10M, <= 11 us below.
constexpr uint32_t kBound8FiltMqMinDim = 768, kBound8FiltMqMinRows4 = 3000000, kBound8FiltMqMinRows8 = 3000000;   // rows of at least 768 dimensions, QB = 4 / QB = 8; 0: never automatic
// The 6-bit stage in front of the 8-bit one (k_bound_scan6 + k_bound_refine8): one UNFILTERED query the 8-bit stage takes, on an index that
// holds the 6-bit plane.  The index's setter (IndexView::bound_plane6) or QV_BOUND_PLANE6 = 1 puts it first whenever that holds, 2 never.
// Automatic: the cells in which 6-bit first beat 8-bit first in both rounds by more than the rounds' disagreement, never below the 8-bit
// stage's own floor; profiles/LAB_r20_bound_scan6.md; us per query, 8-bit first / 6-bit first (candidates of the 6-bit stage), at k = 1, 10, 64:
//   768 dims   3M  420 / 384 (840), 426 / 443 (5 324), 486 / 615 (15 416): losses from k = 10 on
//              10M 1283 / 1042 (675), 1288 / 1112 (6 089), 1343 / 1360 (21 432): a loss at k = 64
//              1M  189 / 243, 193 / 280, 250 / 440 (losses; the refine in batches of 64)
//   128 dims   10M 270 / 236 (49), 273 / 246 (190), 324 / 334 (871): a loss at k = 64
//   1536 dims  3M  808 / 880 (9 615), 809 / 1047 (28 608), 880 / 1436 (79 492) (losses; the refine in batches of 64)
// The refine and its collect cost about 13 us per thousand candidates, and the candidates grow with k and with the width.  So: from
// 10M rows, 128 <= dim < 1536, k <= 10; nothing between the measured k = 10 and k = 64 is taken.
constexpr uint32_t kBound6MinRows = 10000000, kBound6MaxDim = 1536;           // 768 <= dim < 1536
constexpr uint32_t kBound6NarrowDim = 128, kBound6NarrowRows = 10000000;      // 128 <= dim < 768 (nothing between was measured)
constexpr uint32_t kBound6MaxK = 10;
// ---- the ONE decision: which stages answer a call (bound_scan_decide; plan_flat and the row-set front ask it, the launchers never) ----
// All six forms — one query or a shared pass of 2 - 8, filtered or not, with or without the 8-bit plane first — share one skeleton, written once
// below: "never" on the bound scan's knob, or a call the kernels cannot serve -> none; the bfloat16 stage under "always", else where the automatic
// rule of the call's class takes it; then the 8-bit stage in front under the FORM's own plane knob: "bf16" or no plane held -> the bfloat16 stage
// alone, "8bit" -> in front, else where the 8-bit stage's automatic rule takes it.  (So the 8-bit stage never starts a call the bound scan
// would not take, and every plane knob is independent of the others.)  What differs between the forms is data: the measured constants above,
// gathered in two tables.  An automatic rule is the unfiltered floor of its class and, under a filter, the filter's conditions ON TOP: a
// filtered form is never taken below the unfiltered floors.  Classes: one query, QB = 4 (2 - 4 queries), QB = 8 (5 - 8 queries).
constexpr uint32_t kBoundWideDim = 768;   // where every rule's wide class starts (128 dimensions were measured, nothing between)
static_assert(kBoundMqMinDim == kBoundWideDim && kBoundL2WideDim == kBoundWideDim && kBound8MinDim == kBoundWideDim && kBound8MqMinDim == kBoundWideDim &&
              kBoundFiltMinDim == kBoundWideDim && kBound8FiltMqMinDim == kBoundWideDim, "the rules share one wide class");
enum { kRulesBf16 = 0, kRulesBf16L2 = 1, kRulesPlane8 = 2 };          // the bfloat16 stage for cosine and dot / on L2 planes; the 8-bit stage (any metric)
struct BoundFloor { uint32_t wide_rows, narrow_dim, narrow_rows; };   // from wide_rows rows of kBoundWideDim dimensions or more, from narrow_rows rows of
                                                                      // narrow_dim <= dim < kBoundWideDim, never narrower; 0 rows: never automatic
constexpr BoundFloor kBoundFloor[3][3] = {
    {{kBoundScanMinRows, 0, kBoundScanMinRows},                       // one query: any width the kernels serve
     {kBoundMqMinRows4, kBoundMqNarrowDim, kBoundMqNarrowRows}, {kBoundMqMinRows8, kBoundMqNarrowDim, kBoundMqNarrowRows}},
    {{kBoundScanMinRows, kBoundL2NarrowDim, kBoundL2NarrowRows},      // L2 planes: one query's narrow rows are its own, the shared passes' are cosine's
     {kBoundMqMinRows4, kBoundMqNarrowDim, kBoundMqNarrowRows}, {kBoundMqMinRows8, kBoundMqNarrowDim, kBoundMqNarrowRows}},
    {{kBound8MinRows, kBound8NarrowDim, kBound8NarrowRows},
     {kBound8MqMinRows4, kBound8MqNarrowDim, kBound8MqNarrowRows4}, {kBound8MqMinRows8, kBound8MqNarrowDim, kBound8MqNarrowRows8}},
};
struct BoundFilterFloor {                                             // under a filter, ct = min(candidate_tiles, n_tiles):
    uint32_t min_dim, min_rows;                                       // never narrower, never fewer rows (0 rows: never automatic)
    uint32_t tenths;                                                  // ct * 10 >= n_tiles * tenths
    uint32_t big_rows, big_tenths;                                    // ... from big_rows rows on, big_tenths in its place (0 rows: no such size)
    uint32_t small_k;                                                 // ... and below big_rows rows only k <= small_k (0: any k)
};
constexpr BoundFilterFloor kBoundFilterFloor[3][3] = {
    {{kBoundFiltMinDim, kBoundScanMinRows, 1, 0, 0, 0},               // one query: from kBoundScanMinRows rows; one tile in ten is the sparsest measured
     {kBoundFiltMinDim, kBoundFiltMqRows, 9, kBoundFiltBigRows, 2, 0},   // QB = 4: nine tenths from 1M rows, a fifth from 10M
     {kBoundFiltMinDim, kBoundFiltMqRows, 9, kBoundFiltBigRows, 9, kBoundFiltQb8SmallK}},   // QB = 8: nine tenths, and below 10M rows k <= 10
    {{kBoundFiltMinDim, kBoundScanMinRows, 9, 0, 0, 0},               // L2 planes: nine tenths throughout (sparser filters were not measured for it)
     {kBoundFiltMinDim, kBoundFiltMqRows, 9, 0, 0, 0}, {kBoundFiltMinDim, kBoundFiltMqRows, 9, kBoundFiltBigRows, 9, kBoundFiltQb8SmallK}},
    {{kBound8MinDim, kBound8MinRows, 9, 0, 0, 0},                     // the 8-bit stage: f >= 0.9 in every class
     {kBound8FiltMqMinDim, kBound8FiltMqMinRows4, 9, 0, 0, 0}, {kBound8FiltMqMinDim, kBound8FiltMqMinRows8, 9, 0, 0, 0}},
};
constexpr bool bound_floors_nest() {
    for (int c = 0; c < 3; c++) {
        const BoundFloor &b = kBoundFloor[kRulesBf16][c], &l = kBoundFloor[kRulesBf16L2][c], &p = kBoundFloor[kRulesPlane8][c];
        const BoundFilterFloor& pf = kBoundFilterFloor[kRulesPlane8][c];
        if (p.wide_rows < b.wide_rows || p.wide_rows < l.wide_rows || p.narrow_dim < b.narrow_dim || p.narrow_dim < l.narrow_dim) return false;
        if (p.narrow_rows != 0 && (p.narrow_rows < b.narrow_rows || p.narrow_rows < l.narrow_rows)) return false;
        if (pf.min_dim < kBound8MinDim || (pf.min_rows != 0 && pf.min_rows < p.wide_rows)) return false;
    }
    return true;
}
static_assert(bound_floors_nest(), "the 8-bit floors are never below the bound scan's own, class by class, and its filtered floors never below its unfiltered ones");
static int rule_metric(const IndexView& v) { return v.metric == QV_L2 && v.l2_planes ? QV_RULE_L2_PLANES : v.metric; }
BoundAsk bound_ask(const IndexView& v, uint32_t nq, uint32_t k, uint32_t candidate_tiles) {
    return {rule_metric(v), v.dim, v.n_rows, nq, k, candidate_tiles, v.plane != nullptr, v.plane8 != nullptr, v.plane8 != nullptr && v.plane6 != nullptr};
}
BoundKnobs bound_knobs(const IndexView& v) { return {v.bound_scan, {v.bound_plane, v.bound_plane_filtered, v.bound_plane_mq, v.bound_plane_filtered_mq}, v.bound_plane6}; }
int bound_scan_mode(int mode) { static const int env_mode = env_int("QV_BOUND_SCAN", 0); return mode ? mode : env_mode; }
static int bound_plane_mode(BoundForm form, int mode) {                // the form's plane mode in force: the index's own, else its variable (read once)
    static const int env_mode[4] = {env_int("QV_BOUND_PLANE", 0), env_int("QV_BOUND_PLANE_FILTERED", 0), env_int("QV_BOUND_PLANE_MQ", 0), env_int("QV_BOUND_PLANE_FILTERED_MQ", 0)};
    return mode ? mode : env_mode[form];
}
// what the kernels need, whatever the knobs say: metric, k, nq, the copy, a width it covers in whole 16-dimension steps, 8 tiles, and nq planes
// of lower bounds that stay under 2 GiB
bool bound_scan_kernels_serve(const BoundAsk& a) {
    const uint32_t n_tiles = (a.n_rows + 63) / 64;
    const bool metric_ok = a.rule_metric == QV_COSINE || a.rule_metric == QV_DOT || a.rule_metric == QV_RULE_L2_PLANES;
    if (a.nq < 1 || a.nq > kBoundMqMax || a.k < 1 || a.k > (uint32_t)kMaxFusedK || !metric_ok || !a.has_plane) return false;
    if ((a.dim & 15u) != 0 || a.dim > kBoundMaxDim || n_tiles < 8) return false;
    return a.nq == 1 || (uint64_t)a.nq * n_tiles * 256 <= (2ull << 30);
}
static bool bound_auto(const BoundAsk& a, int rules) {
    const int cls = a.nq == 1 ? 0 : a.nq <= 4 ? 1 : 2;
    const BoundFloor& f = kBoundFloor[rules][cls];
    const uint32_t floor = a.dim >= kBoundWideDim ? f.wide_rows : a.dim >= f.narrow_dim ? f.narrow_rows : 0u;
    if (floor == 0 || a.n_rows < floor) return false;
    if (a.candidate_tiles == kBoundNoFilter) return true;
    const BoundFilterFloor& g = kBoundFilterFloor[rules][cls];
    const uint64_t n_tiles = ((uint64_t)a.n_rows + 63) / 64, ct = std::min<uint64_t>(a.candidate_tiles, n_tiles);
    if (ct == 0 || a.dim < g.min_dim || g.min_rows == 0 || a.n_rows < g.min_rows) return false;
    const bool big = g.big_rows != 0 && a.n_rows >= g.big_rows;
    return ct * 10 >= n_tiles * (big ? g.big_tenths : g.tenths) && (big || g.small_k == 0 || a.k <= g.small_k);
}
// The 6-bit stage's automatic rule (one unfiltered query): never below the 8-bit stage's own floor, and only the cells measured faster than
// 8-bit first by more than the rounds' disagreement (profiles/LAB_r20_bound_scan6.md).
static bool bound6_auto(const BoundAsk& a) {
    if (!bound_auto(a, kRulesPlane8)) return false;
    const uint32_t floor = a.dim >= kBound6MaxDim ? 0u : a.dim >= kBoundWideDim ? kBound6MinRows : a.dim >= kBound6NarrowDim ? kBound6NarrowRows : 0u;
    return floor != 0 && a.n_rows >= floor && a.k <= kBound6MaxK;
}
BoundStages bound_scan_decide(const BoundAsk& a, const BoundKnobs& knobs) {
    const int scan = bound_scan_mode(knobs.scan);
    if (scan == 2 || !bound_scan_kernels_serve(a)) return BoundStages::none;
    if (scan != 1 && !bound_auto(a, a.rule_metric == QV_RULE_L2_PLANES ? kRulesBf16L2 : kRulesBf16)) return BoundStages::none;
    const int plane = bound_plane_mode(bound_form(a), knobs.plane[bound_form(a)]);
    if (plane == 2 || !a.has_plane8) return BoundStages::bf16;
    if (plane != 1 && !bound_auto(a, kRulesPlane8)) return BoundStages::bf16;
    // the 6-bit stage in front of the 8-bit one: one unfiltered query, the plane held (whole 64-dimension groups), its own knob
    if (bound_form(a) != bound_one || !a.has_plane6 || (a.dim & 63u) != 0) return BoundStages::plane8_first;
    static const int env6 = env_int("QV_BOUND_PLANE6", 0);
    const int plane6 = knobs.plane6 ? knobs.plane6 : env6;
    if (plane6 == 2) return BoundStages::plane8_first;
    return plane6 == 1 || bound6_auto(a) ? BoundStages::plane6_first : BoundStages::plane8_first;
}
// the single-query bound scan's buffer (the 6-bit stage's list and the compact array's length are part of it on every index: the size does
// not depend on the plan's stages)
struct BoundLayout { uint64_t* partial; uint32_t* seed_rows; float* seed_dist; uint32_t *cand, *cand6, *n8; BoundQuery8* qst; uint32_t* lo_all; size_t end, total; };
static BoundLayout bound_layout(void* base, const ScanPlan& p, uint32_t k, uint32_t n_tiles, WsLog* log = nullptr) {
    WsCarver w{static_cast<char*>(base), 0, 0, log};
    BoundLayout L{};
    L.partial = w.take256<uint64_t>((size_t)p.grid * k);             // stage 1's lists; the re-score publishes in them
    L.seed_rows = w.take<uint32_t>(64);                               // the k best upper bounds' rows ...
    L.seed_dist = w.take<float>(64);                                  // ... and values
    L.cand = w.take<uint32_t>(kBoundCandCap);                         // survivors the re-score walks
    L.cand6 = w.take<uint32_t>(kBound6CandCap);                       // the 6-bit stage's candidates, for the refine
    L.n8 = w.take<uint32_t>(64);                                      // the compact array's length (one word of 256 bytes)
    L.qst = w.take<BoundQuery8>(1);                                   // the 8-bit query state the 6-bit stage leaves for the refine
    L.lo_all = w.take<uint32_t>((size_t)n_tiles * 64);                // a lower bound per row slot
    return w.finish(L);
}
size_t bound_scan_workspace_bytes(const ScanPlan& p, uint32_t k, uint32_t n_tiles, WsLog* log) { return bound_layout(nullptr, p, k, n_tiles, log).total; }
hipError_t launch_bound_scan(const IndexView& v, const ScanPlan& p, const float* d_query, uint32_t k, void* d_ws, uint32_t* d_ctrl, uint32_t* d_stats,
                             uint32_t* d_rows_out, float* d_dist_out, const uint32_t** gate_out, hipStream_t s, bool masked, bool plane8_first, bool plane6_first) {
    // (whether the path is TAKEN is plan_flat's decision; here only what the kernels need: metric, width, the copy, k)
    if (!bound_scan_kernels_serve(bound_ask(v, 1, k, kBoundNoFilter)) || !d_ctrl || !d_stats) return hipErrorInvalidValue;
    if (plane8_first && !v.plane8) return hipErrorInvalidValue;
    if (plane6_first && (!plane8_first || masked || !v.plane6 || !v.rres6 || (v.dim & 63u) != 0)) return hipErrorInvalidValue;
    const uint32_t grid = p.grid;
    const BoundLayout L = bound_layout(d_ws, p, k, v.n_tiles);
    uint64_t* partial = L.partial;
    uint32_t *seed_rows = L.seed_rows, *cand = L.cand, *cand6 = L.cand6, *n8 = L.n8, *lo_all = L.lo_all;
    float* seed_dist = L.seed_dist;
    BoundQuery8* qst = L.qst;
    const uint32_t n_pad = v.n_tiles * 64, cgrid = std::min(kBoundCollectGrid, (n_pad + kCollectChunk - 1u) / kCollectChunk);
    BoundCtrl* ctrl = reinterpret_cast<BoundCtrl*>(d_ctrl);
    const size_t lds1 = (size_t)v.dim * sizeof(float) + (size_t)kScanWaves * 64 * sizeof(uint64_t);
    // the re-score: the staged query, the waves' lists, a survivor's row per wave; its grid never exceeds stage 1's, whose `partial` it publishes in
    const size_t lds2 = query_lds_bytes(v.metric, v.dim4) + (size_t)kScanWaves * 64 * sizeof(uint64_t) + (size_t)kScanWaves * v.dim4 * 4 * sizeof(float);
    const uint32_t rgrid = std::min(kBoundRescoreGrid, grid);
    const size_t lds8 = (size_t)v.dim * 2 + (size_t)kScanWaves * 64 * sizeof(uint64_t);
    auto run = [&](auto Mc, auto Mk) -> hipError_t {
        constexpr int M = decltype(Mc)::value;
        constexpr bool MASKED = decltype(Mk)::value;                  // under a filter every stage skips the tiles without a candidate, and the exact scan behind them walks the candidate bitmap
        // one stage on the control words c: its scan, the collect, the re-score.  gate: the flag of the stage in front (null: none);
        // next: the stage behind, whose flag an answering 8-bit stage clears; scan_gate: k_bound_scan's own gate argument (k_bound_scan8 has none)
        // (attrs: the dynamic LDS of a stage's two kernels, for every stage before anything is launched — a call that fails enqueues nothing)
        const uint32_t* const no_gate = nullptr;
        auto attrs = [&](auto scan, size_t lds_scan, auto rescore) -> hipError_t {
            const hipError_t e = set_lds(scan, lds_scan);
            return e != hipSuccess ? e : set_lds(rescore, lds2);
        };
        auto stage = [&](auto scan, size_t lds_scan, auto rescore, BoundCtrl* c, uint32_t* gate, BoundCtrl* next, auto... scan_gate) {
            hipLaunchKernelGGL(scan, dim3(grid), dim3(kScanBlock), lds_scan, s, v, d_query, k, c, lo_all, partial, seed_rows, seed_dist, scan_gate...);
            hipLaunchKernelGGL(k_bound_collect, dim3(cgrid), dim3(256), 0, s, lo_all, n_pad, c, cand, (const uint32_t*)gate, kBoundCandCap, no_gate, no_gate);
            hipLaunchKernelGGL(rescore, dim3(rgrid), dim3(kScanBlock), lds2, s, v, d_query, k, c, cand, d_stats, d_rows_out, d_dist_out, gate, next, partial, (const BoundQuery8*)nullptr);
        };
        hipError_t e = attrs(k_bound_scan<M, MASKED>, lds1, k_bound_rescore<M>);
        if (e == hipSuccess && plane8_first) e = attrs(k_bound_scan8<M, MASKED>, lds8, k_bound_rescore<M, true>);
        if constexpr (!MASKED) {
            if (e == hipSuccess && plane6_first) e = set_lds(k_bound_scan6<M>, lds8);
            if (e == hipSuccess && plane6_first) e = set_lds(k_bound_refine8<M>, lds8);
        }
        if (e != hipSuccess) return e;
        if (plane6_first) {
            if constexpr (!MASKED) {
                // the 6-bit stage on the third set of control words; its refine leaves the 8-bit stage's words as k_bound_scan8 would (or without
                // H: a hand-back), the compact array of 8-bit lower bounds in the head of lo_all, and that stage's collect and re-score finish
                BoundCtrl *ctrl8 = ctrl + 1, *ctrl6 = ctrl + 2;
                uint32_t* gate8 = &ctrl8->flag;
                const uint32_t fgrid = std::min(kBoundRefineGrid, grid), cgrid8 = std::min(cgrid, kBound6CandCap / kCollectChunk);
                hipLaunchKernelGGL(k_bound_scan6<M>, dim3(grid), dim3(kScanBlock), lds8, s, v, d_query, k, ctrl6, lo_all, partial, seed_rows, seed_dist, qst);
                hipLaunchKernelGGL(k_bound_collect, dim3(cgrid), dim3(256), 0, s, lo_all, n_pad, ctrl6, cand6, no_gate, kBound6CandCap, no_gate, no_gate);
                hipLaunchKernelGGL(k_bound_refine8<M>, dim3(fgrid), dim3(kScanBlock), lds8, s, v, (const BoundQuery8*)qst, k, ctrl6, ctrl8, cand6, lo_all, n8, partial, seed_rows, seed_dist, d_stats);
                hipLaunchKernelGGL(k_bound_collect, dim3(cgrid8), dim3(256), 0, s, lo_all, 0u, ctrl8, cand, no_gate, kBoundCandCap, (const uint32_t*)n8, (const uint32_t*)cand6);
                hipLaunchKernelGGL((k_bound_rescore<M, true>), dim3(rgrid), dim3(kScanBlock), lds2, s, v, d_query, k, ctrl8, cand, d_stats, d_rows_out, d_dist_out, (uint32_t*)nullptr, ctrl, partial, (const BoundQuery8*)qst);
                stage(k_bound_scan<M, MASKED>, lds1, k_bound_rescore<M>, ctrl, gate8, (BoundCtrl*)nullptr, (const uint32_t*)gate8);
            }
        } else if (plane8_first) {
            // the 8-bit stage on the second set of control words, in the same workspace (the stages run one after the other); the bfloat16 stage
            // behind it is gated on that stage's flag and leaves at once when it has answered
            BoundCtrl* ctrl8 = ctrl + 1;
            uint32_t* gate8 = &ctrl8->flag;
            stage(k_bound_scan8<M, MASKED>, lds8, k_bound_rescore<M, true>, ctrl8, (uint32_t*)nullptr, ctrl);
            stage(k_bound_scan<M, MASKED>, lds1, k_bound_rescore<M>, ctrl, gate8, (BoundCtrl*)nullptr, (const uint32_t*)gate8);
        } else stage(k_bound_scan<M, MASKED>, lds1, k_bound_rescore<M>, ctrl, (uint32_t*)nullptr, (BoundCtrl*)nullptr, no_gate);
        return hipSuccess;
    };
    auto run_metric = [&](auto Mk) -> hipError_t {
        return v.metric == QV_COSINE ? run(std::integral_constant<int, QV_COSINE>{}, Mk)
             : v.metric == QV_DOT  ? run(std::integral_constant<int, QV_DOT>{}, Mk) : run(std::integral_constant<int, QV_L2>{}, Mk);
    };
    const hipError_t e = masked ? run_metric(std::true_type{}) : run_metric(std::false_type{});
    if (e != hipSuccess) return e;
    *gate_out = &ctrl->flag;
    return hipGetLastError();
}
// ---- the wide form (65 <= k <= kBoundWideMaxK): its rule, its buffer, its launches ----
// The rule is the wide form's own: bound_scan_decide keeps answering none above kMaxFusedK (qv_scan_bound_applies(., k = 65, ALWAYS, .) == 0 is
// pinned by tests), and the knob is independent of qv_index_set_bound_scan.  NEVER, or a call the kernels cannot serve -> 0.  ALWAYS -> the
// wide form; the 8-bit plane first under QV_BOUND_PLANE_8BIT where it is held, the bfloat16 copy first otherwise.
// AUTOMATIC: the cells of profiles/LAB_r24_bound_scan_wide.md in which the wide form ran ahead of the exact path (k_flat_scan_wide up to
// k = 128, the key-per-row path above) at EVERY measured k — 65, 100, 128, 129, 256, 1000 — by more than both arms' spread, and the 8-bit
// plane first only where it also beat the bfloat16 copy first by the same standard; cosine, device-pointer calls, five alternating rounds
// of 20 calls.  us per call, exact / bfloat16 first / 8-bit first (survivors bfloat16 / 8-bit), spreads <= 18 us:
//   768 dims   1M   k 65: 482 / 313 / 243 (88 / 285)      k 128: 493 / 320 / 257 (194 / 546)    k 1000: 501 / 352 / 301 (1 363 / 3 180)
//              3M   k 65: 1342 / 768 / 487 (101 / 313)    k 128: 1351 / 774 / 489 (176 / 585)   k 1000: 1396 / 808 / 541 (1 395 / 3 584)
//              10M  k 65: 4340 / 2416 / 1323 (97 / 320)   k 128: 4350 / 2421 / 1326 (197 / 621) k 1000: 4424 / 2447 / 1371 (1 431 / 4 047)
//   128 dims   10M  k 65: 778 / 482 / 323 (70 / 114)      k 128: 801 / 488 / 329 (158 / 254)    k 1000: 803 / 508 / 348 (1 179 / 1 759)
// No cell lost, in either comparison.  NOT measured, so never automatic: fewer than 1M rows; narrower than 128 dimensions; 128 <= dim < 768
// below 10M rows (nothing between the widths was measured: the other rules' two width classes); k above 1000; QV_L2 indexes with the
// planes (cosine was measured; dot runs the same kernels over the same bytes and differs in the finalize alone).
constexpr BoundFloor kBoundWideFloor = {1000000, 128, 10000000};      // the wide form against the exact path
constexpr BoundFloor kBoundWide8Floor = {1000000, 128, 10000000};     // ... and the 8-bit plane first against the bfloat16 copy first
constexpr uint32_t kBoundWideAutoMaxK = 1000;                         // the largest measured k
static bool bound_wide_auto(const BoundFloor& f, int rule_metric, uint32_t dim, uint32_t rows, uint32_t k) {
    const uint32_t floor = dim >= kBoundWideDim ? f.wide_rows : f.narrow_dim != 0 && dim >= f.narrow_dim ? f.narrow_rows : 0u;
    return floor != 0 && rows >= floor && k <= kBoundWideAutoMaxK && (rule_metric == QV_COSINE || rule_metric == QV_DOT);
}
int bound_wide_route(int rule_metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int wide_mode, int plane_mode, bool has_plane, bool has_plane8) {
    static const int env_wide = env_int("QV_BOUND_SCAN_WIDE", 0);
    const int mode = wide_mode ? wide_mode : env_wide;
    if (mode == 2) return 0;
    // what the kernels need: one query, the list lengths behind the wave list, the k <= 64 form's metrics and widths, the copy, 8 tiles, more
    // rows than results (a k that takes every row has nothing to reject), and room for the redo's two key planes
    const uint32_t n_tiles = (uint32_t)(((uint64_t)rows + 63) / 64);
    const bool metric_ok = rule_metric == QV_COSINE || rule_metric == QV_DOT || rule_metric == QV_RULE_L2_PLANES;
    if (nq != 1 || k <= (uint32_t)kMaxFusedK || k > kBoundWideMaxK || !metric_ok || !has_plane) return 0;
    if ((dim & 15u) != 0 || dim == 0 || dim > kBoundMaxDim || n_tiles < 8 || k >= rows || !flat_select_redo_one_serves(n_tiles)) return 0;
    if (mode != 1 && !bound_wide_auto(kBoundWideFloor, rule_metric, dim, rows, k)) return 0;
    const int plane = bound_plane_mode(bound_one, plane_mode);
    if (plane == 2 || !has_plane8) return 1;
    return plane == 1 || bound_wide_auto(kBoundWide8Floor, rule_metric, dim, rows, k) ? 2 : 1;
}
// The FILTERED wide form's rule (one query over a candidate bitmap: qv_index_search_masked, a row set, a where-filter made into a set): a knob
// of its own (qv_index_set_bound_scan_wide_filtered / QV_BOUND_SCAN_WIDE_FILTERED), independent of the unfiltered form's and of the k <= 64
// knobs; the plane it starts on is the single-query filtered plane knob's (bound_one_filtered).  What the kernels need is what the unfiltered
// form needs, and on top: a tile that holds a candidate, and MORE candidates than results — a k that takes every candidate has nothing to
// reject, and a shorter set keeps its path and its clamped count.
// AUTOMATIC: the unfiltered floor (bound_wide_auto: never a shape the unfiltered rule declines — cosine and dot, k <= 1000) and, on top, the
// cells of profiles/LAB_r25_bound_scan_wide_filtered.md in which the form ran ahead of the path the filtered call takes today (the filtered
// k_flat_scan_wide up to k = 128, the key-per-row path above) at EVERY measured k — 65, 100, 128, 129, 256, 1000 — by more than both arms'
// spread, and the 8-bit plane first only where it also beat the bfloat16 copy first by the same standard; cosine, device-pointer row-set
// calls, five alternating rounds of 20 calls.  A cell is a shape and a candidate-tile fraction f = candidate tiles / tiles, which is what
// the host can tell apart: every row selected and a random half (f = 1), a random 1 % of the rows (f = 0.476), one tile in ten (f = 0.100).
// us per call at k = 100, today / bfloat16 first / 8-bit first (spreads <= 9 us at this k):
//   768 dims   1M   f 1: 494 / 320 / 246     f 0.476: 479 / 232 / 200     f 0.100: 494 / 131 / 158
//              3M   f 1: 1343 / 776 / 493    f 0.476: 1331 / 468 / 336    f 0.100: 1354 / 311 / 245
//              10M  f 1: 4339 / 2427 / 1299  f 0.476: 4327 / 1322 / 742   f 0.100: 4339 / 375 / 277
//   128 dims   10M  f 1: 796 / 526 / 355     f 0.476: 760 / 332 / 240     f 0.100: 778 / 160 / 163
// The bfloat16 copy first lost NO cell against today's path.  The 8-bit plane first lost against the bfloat16 copy first at f = 0.100 for
// 1M x 768 (every k: 158 against 131) and for 10M x 128 (five of six k: 163 against 160), and at f = 0.476 for 1M x 768 it did not clear the
// spread at k = 129 (204 against 229 with a spread of 27): those cells start on the bfloat16 copy.  NOT measured, so never automatic: what
// the unfiltered rule leaves out (fewer than 1M rows, narrower than 128 dimensions, 128 <= dim < 768 below 10M rows, k above 1000, QV_L2
// indexes with the planes), and fewer candidate tiles than one in ten.  Fractions in per mille of the tiles; 0 rows: never automatic.
struct BoundWideFilterFloor {
    uint32_t wide_rows, wide_frac;        // dim >= kBoundWideDim: from wide_rows rows, ct * 1000 >= n_tiles * wide_frac
    uint32_t big_rows, big_frac;          // ... from big_rows rows on, big_frac in its place (0 rows: no such size)
    uint32_t narrow_rows, narrow_frac;    // the unfiltered floor's narrow class (its narrow_dim <= dim < kBoundWideDim)
};
constexpr BoundWideFilterFloor kBoundWideFilterFloor = {1000000, 100, 0, 0, 10000000, 100};          // the filtered wide form against today's filtered path
constexpr BoundWideFilterFloor kBoundWide8FilterFloor = {1000000, 1000, 3000000, 100, 10000000, 475};   // ... and the 8-bit plane first against the bfloat16 copy first
static_assert(kBoundWide8FilterFloor.wide_rows >= kBoundWideFilterFloor.wide_rows && kBoundWide8FilterFloor.wide_frac >= kBoundWideFilterFloor.wide_frac &&
              kBoundWide8FilterFloor.big_frac >= kBoundWideFilterFloor.wide_frac && kBoundWide8FilterFloor.narrow_rows >= kBoundWideFilterFloor.narrow_rows &&
              kBoundWide8FilterFloor.narrow_frac >= kBoundWideFilterFloor.narrow_frac && kBoundWideFilterFloor.wide_rows >= kBoundWideFloor.wide_rows &&
              kBoundWideFilterFloor.narrow_rows >= kBoundWideFloor.narrow_rows, "8-bit first is never automatic where the form is not, nor the form below the unfiltered floor");
static bool bound_wide_filtered_auto(const BoundFloor& f, const BoundWideFilterFloor& g, int rule_metric, uint32_t dim, uint32_t rows, uint32_t k, uint32_t candidate_tiles) {
    if (!bound_wide_auto(f, rule_metric, dim, rows, k)) return false;
    const uint64_t n_tiles = ((uint64_t)rows + 63) / 64, ct = std::min<uint64_t>(candidate_tiles, n_tiles);
    const bool wide = dim >= kBoundWideDim, big = wide && g.big_rows != 0 && rows >= g.big_rows;
    const uint32_t floor = wide ? g.wide_rows : g.narrow_rows, frac = big ? g.big_frac : wide ? g.wide_frac : g.narrow_frac;
    return ct != 0 && floor != 0 && rows >= floor && ct * 1000 >= n_tiles * frac;
}
int bound_wide_route_filtered(int rule_metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int wide_mode, int plane_mode_filtered, bool has_plane, bool has_plane8,
                              uint32_t candidate_tiles, uint64_t candidates) {
    static const int env_wide = env_int("QV_BOUND_SCAN_WIDE_FILTERED", 0);
    const int mode = wide_mode ? wide_mode : env_wide;
    if (mode == 2) return 0;
    const uint32_t n_tiles = (uint32_t)(((uint64_t)rows + 63) / 64);
    const bool metric_ok = rule_metric == QV_COSINE || rule_metric == QV_DOT || rule_metric == QV_RULE_L2_PLANES;
    if (nq != 1 || k <= (uint32_t)kMaxFusedK || k > kBoundWideMaxK || !metric_ok || !has_plane) return 0;
    if ((dim & 15u) != 0 || dim == 0 || dim > kBoundMaxDim || n_tiles < 8 || k >= rows || !flat_select_redo_one_serves(n_tiles)) return 0;
    if (candidate_tiles == 0 || candidates <= (uint64_t)k) return 0;
    if (mode != 1 && !bound_wide_filtered_auto(kBoundWideFloor, kBoundWideFilterFloor, rule_metric, dim, rows, k, candidate_tiles)) return 0;
    const int plane = bound_plane_mode(bound_one_filtered, plane_mode_filtered);
    if (plane == 2 || !has_plane8) return 1;
    return plane == 1 || bound_wide_filtered_auto(kBoundWide8Floor, kBoundWide8FilterFloor, rule_metric, dim, rows, k, candidate_tiles) ? 2 : 1;
}
// the wide form's buffer.  The redo's workspace overlays the rest: it is written only when every bound stage has ended.
struct BoundWideLayout { void* redo; uint64_t* lists; uint32_t* seed_rows; float* seed_dist; void* sel_ws; uint32_t* cand; uint64_t* keys; uint32_t* sel; uint32_t* lo_all; size_t end, total; };
static BoundWideLayout bound_wide_layout(void* base, const ScanPlan& p, uint32_t k, uint32_t n_tiles, uint32_t dim, WsLog* log = nullptr) {
    WsCarver w{static_cast<char*>(base), 0, 0, log};
    BoundWideLayout L{};
    WsCarver o = w.overlay();
    L.redo = o.take<char>(flat_select_redo_one_workspace_bytes(n_tiles, k, dim, (dim + 3) / 4));   // the exact redo of a search handed back (an alias)
    L.lists = w.take256<uint64_t>((size_t)p.grid * kScanWaves * kBoundWideListLen);   // stage 1's published wave lists
    L.seed_rows = w.take256<uint32_t>(k);                             // the k smallest published upper bounds' rows ...
    L.seed_dist = w.take256<float>(k);                                // ... and values, sorted: the k-th is H
    L.sel_ws = w.take256<char>(select_workspace_bytes(1, k));         // that selection's workspace
    L.cand = w.take<uint32_t>(kBoundWideCandCap);                     // survivors the re-score walks
    L.keys = w.take<uint64_t>(kBoundWideCandCap);                     // their exact keys, dead keys behind
    L.sel = w.take<uint32_t>(64);                                     // [0] live keys, [1] answered (one word of 256 bytes)
    L.lo_all = w.take<uint32_t>((size_t)n_tiles * 64);                // a lower bound per row slot
    w.cover(o);
    return w.finish(L);
}
size_t bound_scan_wide_workspace_bytes(const ScanPlan& p, uint32_t k, uint32_t n_tiles, uint32_t dim, WsLog* log) { return bound_wide_layout(nullptr, p, k, n_tiles, dim, log).total; }
hipError_t launch_bound_scan_wide(const IndexView& v, const ScanPlan& p, const float* d_query, uint32_t k, void* d_ws, uint32_t* d_ctrl, uint32_t* d_stats,
                                  uint32_t* d_rows_out, float* d_dist_out, hipStream_t s, bool plane8_first, bool masked) {
    // (whether the path is TAKEN is bound_wide_route's decision, under a filter bound_wide_route_filtered's; here only what the kernels need)
    if (bound_wide_route(rule_metric(v), v.dim, v.n_rows, 1, k, 1, plane8_first ? 1 : 2, v.plane != nullptr, v.plane8 != nullptr) != (plane8_first ? 2 : 1) || !d_ctrl || !d_stats)
        return hipErrorInvalidValue;
    const uint32_t grid = p.grid;
    const BoundWideLayout L = bound_wide_layout(d_ws, p, k, v.n_tiles, v.dim);
    const uint32_t n_pad = v.n_tiles * 64, cgrid = std::min(kBoundCollectGrid, (n_pad + kCollectChunk - 1u) / kCollectChunk);
    const uint32_t n_keys = grid * kScanWaves * kBoundWideListLen;    // (even, and more than k: grid x 256 >= rows > k)
    BoundCtrl* ctrl = reinterpret_cast<BoundCtrl*>(d_ctrl);
    const size_t lds1 = (size_t)v.dim * sizeof(float) + (size_t)kScanWaves * 64 * sizeof(uint64_t);
    const size_t lds8 = (size_t)v.dim * 2 + (size_t)kScanWaves * 64 * sizeof(uint64_t);
    const size_t lds2 = query_lds_bytes(v.metric, v.dim4) + (size_t)kScanWaves * v.dim4 * 4 * sizeof(float);
    const uint32_t rgrid = std::min(kBoundWideRescoreGrid, (kBoundWideCandCap + kScanWaves - 1) / kScanWaves);
    if (n_keys <= k || (n_keys & 1u)) return hipErrorInvalidValue;
    static const int trace = env_int("QV_TRACE", 0);                   // (one read per process, as qv_scan.hip's)
    if (trace) {
        const char* stage = masked ? "k_bound_scan wide filtered + select + k_bound_collect_wide + k_bound_rescore_wide" : "k_bound_scan wide + select + k_bound_collect_wide + k_bound_rescore_wide";
        if (plane8_first) fprintf(stderr, "qv: scan kernel = k_bound_scan8 wide%s + select + k_bound_collect_wide + k_bound_rescore_wide, then gated %s, then k_select_sort and the gated key-per-row redo (tiles=%u, k=%u)\n", masked ? " filtered" : "", stage, v.n_tiles, k);
        else fprintf(stderr, "qv: scan kernel = %s, then k_select_sort and the gated key-per-row redo (tiles=%u, k=%u)\n", stage, v.n_tiles, k);
    }
    auto run = [&](auto Mc, auto Mk) -> hipError_t {
        constexpr int M = decltype(Mc)::value;
        constexpr bool MASKED = decltype(Mk)::value;                  // v.alive is the call's candidate bitmap: stage 1 skips the tiles without a candidate
        hipError_t e = set_lds(k_bound_scan<M, MASKED, true>, lds1);
        if (e == hipSuccess) e = set_lds(k_bound_rescore_wide<M, false>, lds2);
        if (e == hipSuccess && plane8_first) e = set_lds(k_bound_scan8<M, MASKED, true>, lds8);
        if (e == hipSuccess && plane8_first) e = set_lds(k_bound_rescore_wide<M, true>, lds2);
        if (e != hipSuccess) return e;
        // what follows a stage's scan: H, the collect, the re-score — each behind `gate`, the flag of the stage in front (null: none)
        auto finish = [&](auto rescore, BoundCtrl* c, uint32_t* gate, BoundCtrl* next) -> hipError_t {
            const hipError_t e2 = launch_select_topk(L.lists, n_keys, n_keys, 1, k, k, L.sel_ws, L.seed_rows, L.seed_dist, s, false, false, gate);
            if (e2 != hipSuccess) return e2;
            hipLaunchKernelGGL(k_bound_collect_wide, dim3(cgrid), dim3(256), 0, s, L.lo_all, n_pad, k, (const uint32_t*)L.seed_rows, (const float*)L.seed_dist, c, L.cand, (const uint32_t*)gate);
            hipLaunchKernelGGL(rescore, dim3(rgrid), dim3(kScanBlock), lds2, s, v, d_query, c, (const uint32_t*)L.cand, d_stats, L.keys, L.sel, gate, next);
            return hipGetLastError();
        };
        if (plane8_first) {
            BoundCtrl* ctrl8 = ctrl + 1;
            hipLaunchKernelGGL((k_bound_scan8<M, MASKED, true>), dim3(grid), dim3(kScanBlock), lds8, s, v, d_query, kBoundWideListLen, ctrl8, L.lo_all, L.lists, L.seed_rows, L.seed_dist);
            e = finish(k_bound_rescore_wide<M, true>, ctrl8, (uint32_t*)nullptr, ctrl);
            if (e != hipSuccess) return e;
            uint32_t* gate8 = &ctrl8->flag;
            hipLaunchKernelGGL((k_bound_scan<M, MASKED, true>), dim3(grid), dim3(kScanBlock), lds1, s, v, d_query, kBoundWideListLen, ctrl, L.lo_all, L.lists, L.seed_rows, L.seed_dist, (const uint32_t*)gate8);
            return finish(k_bound_rescore_wide<M, false>, ctrl, gate8, (BoundCtrl*)nullptr);
        }
        hipLaunchKernelGGL((k_bound_scan<M, MASKED, true>), dim3(grid), dim3(kScanBlock), lds1, s, v, d_query, kBoundWideListLen, ctrl, L.lo_all, L.lists, L.seed_rows, L.seed_dist, (const uint32_t*)nullptr);
        return finish(k_bound_rescore_wide<M, false>, ctrl, (uint32_t*)nullptr, (BoundCtrl*)nullptr);
    };
    auto run_metric = [&](auto Mk) -> hipError_t {
        return v.metric == QV_COSINE ? run(std::integral_constant<int, QV_COSINE>{}, Mk)
             : v.metric == QV_DOT  ? run(std::integral_constant<int, QV_DOT>{}, Mk) : run(std::integral_constant<int, QV_L2>{}, Mk);
    };
    hipError_t e = masked ? run_metric(std::true_type{}) : run_metric(std::false_type{});
    if (e != hipSuccess) return e;
    // the answer of whichever stage answered (sel[1]), then the exact redo of a search the bfloat16 stage handed back (its flag)
    e = launch_select_topk_counted(L.keys, kBoundWideCandCap, kBoundWideCandCap, L.sel, 1, k, k, d_rows_out, d_dist_out, s, L.sel + 1);
    if (e != hipSuccess) return e;
    return launch_flat_select_redo_one(v, p, d_query, k, k, &ctrl->flag, L.redo, d_rows_out, d_dist_out, s);
}
// ---- the wide form of the shared pass (2 - 8 queries, 65 <= k <= kBoundWideMaxK): its rule, its buffer, its launches ----
// A rule and a knob of its own (qv_index_set_bound_scan_wide_mq / QV_BOUND_SCAN_WIDE_MQ): independent of the single-query wide knob, of
// qv_index_set_bound_scan and of the single-query plane knobs; bound_wide_route keeps answering 0 for nq != 1.  NEVER, or a pass the kernels
// cannot serve -> 0.  What they need: 2 - 8 unfiltered queries, the k <= 64 pass's and the single wide form's limits — metric, the copy, whole
// 16-dimension steps, 8 tiles, nq planes of lower bounds under 2 GiB, more rows than results — and an index of at most 64M rows (the redo's
// shared key passes take two queries' keys at least: flat_select_redo_one_serves).  ALWAYS -> the form; which plane comes first is the
// shared pass's plane knob (qv_index_set_bound_plane_mq / QV_BOUND_PLANE_MQ): 8-bit first under "8bit" where the plane is held.
// AUTOMATIC: per class (QB = 4: 2 - 4 queries, QB = 8: 5 - 8) the floors below; a floor of 0 rows is never automatic.  Only measured cells
// are taken — the form against the key-per-row shared pass (k_flat_keys_mq + the radix selection), 8-bit first against bfloat16 first, each by
// more than both arms' spread at every measured k and nq of the class (profiles/LAB_r26_bound_scan_wide_mq.md) — so QV_L2 indexes with the
// planes are reached under ALWAYS alone, and dot is taken where cosine was measured (the same kernels over the same bytes; the finalize differs).
// Cosine, device-pointer calls, five alternating rounds of 20 calls; nq = 2 and 4 (QB = 4), nq = 5 and 8 (QB = 8); k = 65, 100, 128, 129, 256,
// 1000.  us per call at k = 100 and 1000, key-per-row / bfloat16 first / 8-bit first (spreads <= 27 us, at 10M x 768 <= 63 us):
//   768 dims   1M   nq 2: 521 / 379 / 280, 552 / 418 / 351      nq 4: 547 / 424 / 345, 584 / 480 / 438
//                   nq 5: 598 / 588 / 440, 646 / 641 / 557      nq 8: 596 / 660 / 534, 646 / 757 / 698
//              3M   nq 2: 1495 / 858 / 547, 1536 / 898 / 611    nq 4: 1473 / 887 / 589, 1539 / 941 / 682
//                   nq 5: 1556 / 1243 / 782, 1632 / 1330 / 904  nq 8: 1788 / 1367 / 943, 1884 / 1470 / 1116
//              10M  nq 2: 4872 / 2560 / 1403, 4875 / 2592 / 1469    nq 4: 5237 / 2762 / 1533, 5244 / 2802 / 1621
//                   nq 5: 5551 / 3568 / 1980, 5561 / 3571 / 2022    nq 8: 6041 / 3846 / 2255, 6047 / 3927 / 2401
//   128 dims   10M  nq 2: 945 / 534 / 453, 948 / 561 / 476      nq 4: 1158 / 718 / 652, 1161 / 752 / 683
//                   nq 5: 1259 / 844 / 837, 1262 / 883 / 869    nq 8: 1395 / 1073 / 1134, 1399 / 1110 / 1175
// LOSSES: at 1M x 768 the bfloat16 copy first lost to the key-per-row pass with 8 queries at every k (by 9 - 17 %) and did not clear the
// spread with 5 queries at k = 1000, so QB = 8 starts at 3M rows — the 8-bit plane first ran ahead of both there but for 8 queries at
// k = 1000 (698 against 646), and is not taken either: it is never automatic where the form is not; at 10M x 128 the 8-bit plane first lost
// to the bfloat16 copy first with 8 queries at every k (by 6 %; with 5 queries it won by 1 - 2 %), so QB = 8 stays on the bfloat16 copy below
// 768 dimensions.  Every other cell won both comparisons at every k.  NOT measured, so never automatic: fewer than 1M rows; narrower than
// 128 dimensions; 128 <= dim < 768 below 10M rows; k above 1000; QV_L2 indexes with the planes.  (nq = 3, 6 and 7 were not run: they go with
// their class, between its two measured fills, as in the k <= 64 rules.)
constexpr BoundFloor kBoundWideMqFloor[2] = {{1000000, 128, 10000000}, {3000000, 128, 10000000}};   // the form against the key-per-row shared pass, QB = 4 / QB = 8
constexpr BoundFloor kBoundWideMq8Floor[2] = {{1000000, 128, 10000000}, {3000000, 0, 0}};           // ... and the 8-bit plane first against the bfloat16 copy first
constexpr bool bound_wide_mq_floors_nest() {
    for (int c = 0; c < 2; c++) {
        const BoundFloor &f = kBoundWideMqFloor[c], &p = kBoundWideMq8Floor[c];
        if (p.wide_rows != 0 && (f.wide_rows == 0 || p.wide_rows < f.wide_rows)) return false;
        if (p.narrow_rows != 0 && (f.narrow_rows == 0 || p.narrow_rows < f.narrow_rows || p.narrow_dim < f.narrow_dim)) return false;
    }
    return true;
}
static_assert(bound_wide_mq_floors_nest(), "8-bit first is never automatic where the wide shared pass is not");
int bound_wide_route_mq(int rule_metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int wide_mq_mode, int plane_mode_mq, bool has_plane, bool has_plane8) {
    static const int env_wide = env_int("QV_BOUND_SCAN_WIDE_MQ", 0);
    const int mode = wide_mq_mode ? wide_mq_mode : env_wide;
    if (mode == 2) return 0;
    const uint32_t n_tiles = (uint32_t)(((uint64_t)rows + 63) / 64);
    const bool metric_ok = rule_metric == QV_COSINE || rule_metric == QV_DOT || rule_metric == QV_RULE_L2_PLANES;
    if (nq < 2 || nq > kBoundMqMax || k <= (uint32_t)kMaxFusedK || k > kBoundWideMaxK || !metric_ok || !has_plane) return 0;
    if ((dim & 15u) != 0 || dim == 0 || dim > kBoundMaxDim || n_tiles < 8 || k >= rows || !flat_select_redo_one_serves(n_tiles)) return 0;
    if ((uint64_t)nq * n_tiles * 256 > (2ull << 30)) return 0;
    const int cls = nq <= 4 ? 0 : 1;
    if (mode != 1 && !bound_wide_auto(kBoundWideMqFloor[cls], rule_metric, dim, rows, k)) return 0;
    const int plane = bound_plane_mode(bound_mq, plane_mode_mq);
    if (plane == 2 || !has_plane8) return 1;
    return plane == 1 || bound_wide_auto(kBoundWideMq8Floor[cls], rule_metric, dim, rows, k) ? 2 : 1;
}
// the wide shared pass's buffer.  The pass's flag words come first and stay: the redo reads its flags from them.  The redo's workspace
// overlays the rest: it is written only when every bound stage and the counted selection have ended.
struct BoundWideMqLayout {
    uint32_t* flags; void* redo; uint64_t* lists; uint32_t* seed_rows; float* seed_dist; void* sel_ws; double* qnorm; float* qblk; uint32_t* cand; uint64_t* keys; uint32_t* lo_all;
    size_t end, total;
};
static BoundWideMqLayout bound_wide_mq_layout(void* base, const ScanPlan& p, uint32_t nq, uint32_t k, uint32_t n_tiles, uint32_t dim, WsLog* log = nullptr) {
    WsCarver w{static_cast<char*>(base), 0, 0, log};
    BoundWideMqLayout L{};
    L.flags = w.take<uint32_t>(64);                                   // [0, 8) the redo's flags; [16, 24) hand-on words, [24] nq or 0; [32, 40) the key lists' counts
    WsCarver o = w.overlay();
    L.redo = o.take<char>(flat_select_redo_workspace_bytes(n_tiles, nq, k, dim, (dim + 3) / 4));   // the key-per-row redo of the queries handed back (an alias)
    L.lists = w.take256<uint64_t>((size_t)nq * p.grid * kScanWaves * kBoundWideListLen);   // stage 1's published wave lists, per query
    L.seed_rows = w.take256<uint32_t>((size_t)nq * k);                // per query the k smallest published upper bounds' rows ...
    L.seed_dist = w.take256<float>((size_t)nq * k);                   // ... and values, sorted: the k-th is H_j
    L.sel_ws = w.take256<char>(select_workspace_bytes(nq, k));        // that selection's workspace
    L.qnorm = w.take<double>(32);                                     // the queries' norms (the 8-bit stage: its three scalars per query)
    L.qblk = w.take256<float>((size_t)dim * kBoundMqMax);             // the query block (the 8-bit stage: its terms)
    L.cand = w.take<uint32_t>((size_t)nq * kBoundWideCandCap);        // survivors the re-score walks, per query
    L.keys = w.take<uint64_t>((size_t)nq * kBoundWideCandCap);        // their exact keys, dead keys behind
    L.lo_all = w.take<uint32_t>((size_t)nq * n_tiles * 64);           // a lower bound per query and row slot
    w.cover(o);
    return w.finish(L);
}
size_t bound_scan_wide_mq_workspace_bytes(const ScanPlan& p, uint32_t nq, uint32_t k, uint32_t n_tiles, uint32_t dim, WsLog* log) { return bound_wide_mq_layout(nullptr, p, nq, k, n_tiles, dim, log).total; }
hipError_t launch_bound_scan_wide_mq(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint32_t k, void* d_ws, uint32_t* d_ctrl, uint32_t* d_stats,
                                     uint32_t* d_rows_out, float* d_dist_out, hipStream_t s, bool plane8_first) {
    // (whether the pass is TAKEN is bound_wide_route_mq's decision; here only what the kernels need)
    if (bound_wide_route_mq(rule_metric(v), v.dim, v.n_rows, nq, k, 1, plane8_first ? 1 : 2, v.plane != nullptr, v.plane8 != nullptr) != (plane8_first ? 2 : 1) || !d_ctrl || !d_stats)
        return hipErrorInvalidValue;
    const uint32_t grid = p.grid;
    const BoundWideMqLayout L = bound_wide_mq_layout(d_ws, p, nq, k, v.n_tiles, v.dim);
    const uint32_t n_pad = v.n_tiles * 64, cgrid = std::min(kBoundCollectGrid, (n_pad + kCollectChunk - 1u) / kCollectChunk);
    // keys per query: even.  More than k wherever the grid gives a wave a tile (grid x 256 >= rows > k) or has 2 workgroups per CU on 3 CUs
    // or more (1536 keys and up; 131 072 on 256 CUs).  The rule cannot see the grid: the dispatch (wide_route_mq, qv_api.cpp) asks the same of
    // the plan and keeps such a call on its earlier path; a caller that comes here all the same is refused.
    const uint32_t n_keys = grid * kScanWaves * kBoundWideListLen;
    if (n_keys <= k || (n_keys & 1u)) return hipErrorInvalidValue;
    BoundCtrl* ctrl = reinterpret_cast<BoundCtrl*>(d_ctrl);           // kBoundMqMax of them: zero, left zero
    const size_t lds2 = query_lds_bytes(v.metric, v.dim4) + (size_t)kScanWaves * v.dim4 * 4 * sizeof(float);
    const uint32_t rgrid = std::min(kBoundWideRescoreGrid, (kBoundWideCandCap + kScanWaves - 1) / kScanWaves);
    uint32_t *flags = L.flags, *hand = L.flags + kBound8MqHandWord, *counts = L.flags + kBoundWideMqCountWord;
    static_assert(kBound8MqHandWord + kBoundMqMax + 1 <= kBoundWideMqCountWord && kBoundWideMqCountWord + kBoundMqMax <= 64, "the pass's flag words");
    const uint32_t* gate = plane8_first ? hand + kBoundMqMax : nullptr;   // nq or 0
    const uint32_t* hand_in = plane8_first ? hand : nullptr;
    uint32_t* max_word = d_stats + kBoundWideMqStatsWord;             // the prep kernels clear "the pass's largest survivor count": this form's own word
    static const int trace = env_int("QV_TRACE", 0);                   // (one read per process, as qv_scan.hip's)
    if (trace) fprintf(stderr, "qv: scan kernel = %sk_bound_scan_mq wide QB=%d + select + k_bound_collect_wide_mq + k_bound_rescore_wide_mq, then k_select_sort and the flagged key-per-row redo (nq=%u, tiles=%u, k=%u)\n",
                       plane8_first ? "k_bound_scan8_mq wide + select + k_bound_collect_wide_mq + k_bound_rescore_wide_mq, then gated " : "", nq <= 4 ? 4 : 8, nq, v.n_tiles, k);
    auto run = [&](auto Mc, auto Qc) -> hipError_t {
        constexpr int M = decltype(Mc)::value, QB = decltype(Qc)::value;
        const SetsArg<false> no_sets{};
        // (the dynamic LDS of every re-score before anything is launched; the wide stage-1 kernels take none)
        hipError_t e = plane8_first ? set_lds((k_bound_rescore_wide_mq<M, 1>), lds2) : set_lds((k_bound_rescore_wide_mq<M, 0>), lds2);
        if (e == hipSuccess && plane8_first) e = set_lds((k_bound_rescore_wide_mq<M, 2>), lds2);
        if (e != hipSuccess) return e;
        // what follows a stage's scan: H_j, the collect, the re-score.  g: the word the stage's pass-wide launches are gated on (null: none)
        auto finish = [&](auto rescore, const uint32_t* g, const uint32_t* h_in) -> hipError_t {
            const hipError_t e2 = launch_select_topk(L.lists, n_keys, n_keys, nq, k, k, L.sel_ws, L.seed_rows, L.seed_dist, s, false, false, g);
            if (e2 != hipSuccess) return e2;
            hipLaunchKernelGGL(k_bound_collect_wide_mq, dim3(cgrid, nq), dim3(256), 0, s, (const uint32_t*)L.lo_all, n_pad, k, (const uint32_t*)L.seed_rows, (const float*)L.seed_dist, ctrl, L.cand, h_in);
            hipLaunchKernelGGL(rescore, dim3(rgrid, nq), dim3(kScanBlock), lds2, s, v, d_queries, ctrl, (const uint32_t*)L.cand, d_stats, L.keys, flags, hand, counts);
            return hipGetLastError();
        };
        if (plane8_first) {
            hipLaunchKernelGGL((k_bound_prep8_mq<QB>), dim3(QB), dim3(kScanBlock), 0, s, d_queries, nq, v.dim, reinterpret_cast<int8_t*>(L.qblk), L.qnorm, hand, max_word, (uint32_t*)nullptr);
            hipLaunchKernelGGL((k_bound_scan8_mq<M, QB, false, true>), dim3(grid), dim3(kScanBlock), 0, s, v, reinterpret_cast<const u4*>(L.qblk), (const double*)L.qnorm, nq, kBoundWideListLen, L.lo_all, L.lists, no_sets);
            e = finish(k_bound_rescore_wide_mq<M, 1>, nullptr, nullptr);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL((k_bound_prep_mq<QB>), dim3((v.dim * QB + 255) / 256 + QB), dim3(256), 0, s, d_queries, nq, v.dim, L.qblk, L.qnorm, max_word, gate);
        hipLaunchKernelGGL((k_bound_scan_mq<M, QB, false, true>), dim3(grid), dim3(kScanBlock), 0, s, v, (const float*)L.qblk, (const double*)L.qnorm, nq, kBoundWideListLen, L.lo_all, L.lists, no_sets, gate);
        return plane8_first ? finish(k_bound_rescore_wide_mq<M, 2>, gate, hand_in) : finish(k_bound_rescore_wide_mq<M, 0>, nullptr, nullptr);
    };
    auto run_qb = [&](auto Mc) -> hipError_t { return nq <= 4 ? run(Mc, std::integral_constant<int, 4>{}) : run(Mc, std::integral_constant<int, 8>{}); };
    hipError_t e = v.metric == QV_COSINE ? run_qb(std::integral_constant<int, QV_COSINE>{})
                 : v.metric == QV_DOT  ? run_qb(std::integral_constant<int, QV_DOT>{}) : run_qb(std::integral_constant<int, QV_L2>{});
    if (e != hipSuccess) return e;
    // every query's answer from the stage that answered it (a count of zero for a query handed back), THEN the key-per-row redo of the flagged
    // queries: the counted selection runs over all nq queries and before the redo, so a handed-back query's outputs are the redo's
    e = launch_select_topk_counted(L.keys, kBoundWideCandCap, kBoundWideCandCap, counts, nq, k, k, d_rows_out, d_dist_out, s, nullptr);
    if (e != hipSuccess) return e;
    return launch_flat_select_redo(v, p, d_queries, nq, k, k, flags, L.redo, d_rows_out, d_dist_out, s);
}
// the interval of one row on the host; 1: a row the bound says nothing about ("unsure"), as host_bound_interval8 reports it
int host_bound_interval(int metric, uint32_t dim, float s, double qn, double rn, float rres, float* d_lo, float* d_hi) {
    const double gamma = bound_scan_gamma(dim);
    const bool sure = metric == QV_COSINE ? bound_scan_interval<QV_COSINE>(s, qn, rn, rres, dim, gamma, *d_lo, *d_hi)
                    : metric == QV_DOT  ? bound_scan_interval<QV_DOT>(s, qn, rn, rres, dim, gamma, *d_lo, *d_hi)
                                        : bound_scan_interval<QV_L2>(s, qn, rn, rres, dim, gamma, *d_lo, *d_hi);
    return sure ? 0 : 1;
}

int host_bound_interval8(int metric, uint32_t dim, long long isum, double sq, double qn, double qres, double rn, float rscale, float rres8, float* d_lo, float* d_hi) {
    const bool sure = metric == QV_COSINE ? bound_scan_interval8<QV_COSINE>(isum, sq, qn, qres, rn, rscale, rres8, dim, *d_lo, *d_hi)
                    : metric == QV_DOT  ? bound_scan_interval8<QV_DOT>(isum, sq, qn, qres, rn, rscale, rres8, dim, *d_lo, *d_hi)
                                        : bound_scan_interval8<QV_L2>(isum, sq, qn, qres, rn, rscale, rres8, dim, *d_lo, *d_hi);
    return sure ? 0 : 1;
}
// one row as k_row_state8 (qv_misc.hip) leaves it: the bytes, the scale, the residual from the bytes (NaN: a row the bound says nothing about)
int host_quantize_row8(uint32_t dim, const float* row, int8_t* out_bytes, float* out_scale, float* out_res) {
    float maxabs = 0.f; bool bad = false; double n2 = 0.0;
    for (uint32_t i = 0; i < dim; i++) {
        bad |= !((row[i] - row[i]) == 0.0f);
        maxabs = __builtin_fmaxf(maxabs, __builtin_fabsf(row[i]));
        n2 = __builtin_fma((double)row[i], (double)row[i], n2);
    }
    const float scale = bad ? 0.0f : bound8_scale(maxabs);
    double s2 = 0.0;
    for (uint32_t i = 0; i < dim; i++) {
        const int b = scale > 0.0f ? bound8_quant(row[i], scale) : 0;
        const double d = (double)row[i] - (double)scale * (double)b;
        s2 = __builtin_fma(d, d, s2);
        out_bytes[i] = (int8_t)b;
    }
    *out_scale = scale;
    *out_res = bound8_row_res(bad, maxabs, n2, s2, dim);
    return 0;
}

// one row as k_row_state6 (qv_misc.hip) leaves it: per group of 64 dimensions the pieces X, Y, Z (48 bytes), the residual from the codes
int host_quantize_row6(uint32_t dim, const float* row, float scale8, uint8_t* out_bytes, float* out_res) {
    float maxabs = 0.f; bool bad = false; double n2 = 0.0;
    for (uint32_t i = 0; i < dim; i++) {
        bad |= !((row[i] - row[i]) == 0.0f);
        maxabs = __builtin_fmaxf(maxabs, __builtin_fabsf(row[i]));
        n2 = __builtin_fma((double)row[i], (double)row[i], n2);
    }
    const float div = scale8 > 0.0f ? scale8 : 1.0f;
    const double step = 4.0 * (double)scale8;
    double s2 = 0.0;
    for (uint32_t g = 0; g < dim / 64; g++) {
        uint8_t piece[48] = {};
        for (uint32_t d = 0; d < 64; d++) {
            const float x = row[g * 64 + d];
            const int q = scale8 > 0.0f ? bound6_quant(x, div) : 0;
            const double e = (double)x - step * (double)q;
            s2 = __builtin_fma(e, e, s2);
            bound6_pack(piece, d, (uint32_t)(q + kBound6Bias));
        }
        for (uint32_t i = 0; i < 48; i++) out_bytes[g * 48 + i] = piece[i];
    }
    const float res8 = bound8_row_res(bad, maxabs, n2, 0.0, dim);      // (whether the 8-bit state declines the row: NaN)
    *out_res = res8 == res8 ? bound8_res_up(s2) : __builtin_nanf("");
    return 0;
}
int host_unpack_row6(uint32_t dim, const uint8_t* bytes, uint8_t* out_codes) {
    for (uint32_t g = 0; g < dim / 64; g++) {
        uint8_t piece[48];
        for (uint32_t i = 0; i < 48; i++) piece[i] = bytes[g * 48 + i];
        for (uint32_t d = 0; d < 64; d++) out_codes[g * 64 + d] = (uint8_t)bound6_unpack(piece, d);
    }
    return 0;
}

// the shared pass of 2 - 8 queries: d_ws = bound_scan_mq_workspace_bytes, d_ctrl = kBoundMqMax BoundCtrl (zero, left zero).  The exact scan of the
// queries handed back is part of it (launch_flat_redo_flagged, in the bytes the lower bounds leave behind): nothing is read on the host.
struct BoundMqLayout { uint64_t* partial; uint32_t* seed_rows; float* seed_dist; uint32_t* flags; double* qnorm; float* qblk; uint32_t *cand, *lo_all; void* redo_ws; size_t end, total; };
static BoundMqLayout bound_mq_layout(void* base, const ScanPlan& p, uint32_t nq, uint32_t k, uint32_t n_tiles, uint32_t dim, WsLog* log = nullptr) {
    WsCarver w{static_cast<char*>(base), 0, 0, log};
    BoundMqLayout L{};
    L.partial = w.take256<uint64_t>((size_t)nq * p.grid * k);
    L.seed_rows = w.take256<uint32_t>((size_t)kBoundMqMax * 64);
    L.seed_dist = w.take256<float>((size_t)kBoundMqMax * 64);
    L.flags = w.take<uint32_t>(64);                                   // [0, 8) the exact scan's flags; the 8-bit stage's hand-on words from kBound8MqHandWord
    L.qnorm = w.take<double>(32);                                     // the queries' norms (the 8-bit stage: its three scalars per query)
    L.qblk = w.take256<float>((size_t)dim * kBoundMqMax);             // the query block (the 8-bit stage: its terms)
    WsCarver redo = w.overlay();                                      // (cand and lo_all are dead once the re-score has run: the redo of hand-backs takes their bytes)
    L.cand = w.take<uint32_t>((size_t)nq * kBoundCandCap);
    L.lo_all = w.take<uint32_t>((size_t)nq * n_tiles * 64);
    L.redo_ws = redo.take<char>(redo_workspace_bytes(p, nq, k));
    w.cover(redo);
    return w.finish(L);
}
size_t bound_scan_mq_workspace_bytes(const ScanPlan& p, uint32_t nq, uint32_t k, uint32_t n_tiles, uint32_t dim, WsLog* log) { return bound_mq_layout(nullptr, p, nq, k, n_tiles, dim, log).total; }
hipError_t launch_bound_scan_mq(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint32_t k, void* d_ws, uint32_t* d_ctrl, uint32_t* d_stats,
                                uint32_t* d_rows_out, float* d_dist_out, hipStream_t s, const RowSetRef* h_sets, bool plane8_first) {
    // plane8_first: the 8-bit stage — k_bound_prep8_mq, k_bound_scan8_mq (with h_sets: its set form over the same table), merge, collect,
    // k_bound_rescore_mq<., 1> — in front, in the same workspace (the stages run one after the other: the query terms lie where the float32 block goes, the scalars where
    // the norms go), and the bfloat16 stage's launches gated on the count of queries it handed on.
    // h_sets (optional, a HOST array of nq): query j restricted to alive & h_sets[j] — k_bound_scan_mq<., ., true> and the set-carrying redo.
    // Null: the unfiltered pass.  (Whether the path is TAKEN is the caller's decision — plan_flat, or the row-set path's questions to
    // bound_scan_decide; here only what the kernels need: metric, width, the copy, k, nq planes of lower bounds under 2 GiB.)
    if (nq < 2 || !bound_scan_kernels_serve(bound_ask(v, nq, k, kBoundNoFilter)) || !d_ctrl || !d_stats) return hipErrorInvalidValue;
    if (plane8_first && !v.plane8) return hipErrorInvalidValue;
    BoundSetTable tab;
    for (uint32_t i = 0; i < kBoundSets; i++) tab.e[i] = h_sets && i < nq ? h_sets[i] : RowSetRef{nullptr, 0, 0};
    if (h_sets && trace_filtered()) {
        if (plane8_first) fprintf(stderr, "qv: scan kernel = k_bound_scan8_mq sets QB=%d, then gated k_bound_scan_mq sets (nq=%u, tiles=%u)\n", nq <= 4 ? 4 : 8, nq, v.n_tiles);
        else fprintf(stderr, "qv: scan kernel = k_bound_scan_mq sets QB=%d (nq=%u, tiles=%u)\n", nq <= 4 ? 4 : 8, nq, v.n_tiles);
    }
    const uint32_t grid = p.grid;
    const BoundMqLayout L = bound_mq_layout(d_ws, p, nq, k, v.n_tiles, v.dim);
    uint64_t* partial = L.partial;
    uint32_t *seed_rows = L.seed_rows, *flags = L.flags, *cand = L.cand, *lo_all = L.lo_all;
    float *seed_dist = L.seed_dist, *qblk = L.qblk;
    double* qnorm = L.qnorm;
    void* redo_ws = L.redo_ws;
    const uint32_t n_pad = v.n_tiles * 64, cgrid = std::min(kBoundCollectGrid, (n_pad + kCollectChunk - 1u) / kCollectChunk);
    BoundCtrl* ctrl = reinterpret_cast<BoundCtrl*>(d_ctrl);
    const size_t lds2 = query_lds_bytes(v.metric, v.dim4) + (size_t)kScanWaves * 64 * sizeof(uint64_t);
    hipError_t e = hipSuccess;
    static_assert(2 * kBoundMaxDim * kBoundMqMax <= kBoundMaxDim * kBoundMqMax * sizeof(float) && 3 * kBoundMqMax * sizeof(double) <= 256 &&
                  (kBound8MqHandWord + kBoundMqMax + 1) * 4 <= 256, "the 8-bit stage's terms, scalars and hand-on words fit the bfloat16 stage's");
    uint32_t* hand = flags + kBound8MqHandWord;
    const uint32_t* gate = plane8_first ? hand + kBoundMqMax : nullptr;
    const uint32_t* hand_in = plane8_first ? hand : nullptr;
    auto run = [&](auto Mc, auto Qc, auto Sc) -> hipError_t {
        constexpr int M = decltype(Mc)::value, QB = decltype(Qc)::value;
        constexpr bool SETS = decltype(Sc)::value;
        SetsArg<SETS> sets{};
        if constexpr (SETS) sets = tab;
        const size_t lds1 = (size_t)kScanWaves * QB * 64 * sizeof(uint64_t);
        // (the dynamic LDS of every re-score before anything is launched)
        e = set_lds(k_bound_rescore_mq<M>, lds2);
        if (e == hipSuccess && plane8_first) e = set_lds((k_bound_rescore_mq<M, 1>), lds2);
        if (e == hipSuccess && plane8_first) e = set_lds((k_bound_rescore_mq<M, 2>), lds2);
        if (e != hipSuccess) return e;
        if (plane8_first) {
            hipLaunchKernelGGL((k_bound_prep8_mq<QB>), dim3(QB), dim3(kScanBlock), 0, s, d_queries, nq, v.dim, reinterpret_cast<int8_t*>(qblk), qnorm, hand, d_stats, d_stats + kBound8StatsWord);
            hipLaunchKernelGGL((k_bound_scan8_mq<M, QB, SETS>), dim3(grid), dim3(kScanBlock), lds1, s, v, reinterpret_cast<const u4*>(qblk), qnorm, nq, k, lo_all, partial, sets);
            e = launch_merge_lists(partial, grid, nq, k, seed_rows, seed_dist, s);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(k_bound_collect_mq, dim3(cgrid, nq), dim3(256), 0, s, lo_all, n_pad, k, seed_rows, seed_dist, ctrl, cand, (const uint32_t*)nullptr);
            hipLaunchKernelGGL((k_bound_rescore_mq<M, 1>), dim3(nq), dim3(kScanBlock), lds2, s, v, d_queries, k, seed_rows, seed_dist, ctrl, cand, flags, d_stats, d_rows_out, d_dist_out, hand);
        }
        hipLaunchKernelGGL((k_bound_prep_mq<QB>), dim3((v.dim * QB + 255) / 256 + QB), dim3(256), 0, s, d_queries, nq, v.dim, qblk, qnorm, d_stats, gate);
        hipLaunchKernelGGL((k_bound_scan_mq<M, QB, SETS>), dim3(grid), dim3(kScanBlock), lds1, s, v, qblk, qnorm, nq, k, lo_all, partial, sets, gate);
        e = launch_merge_lists(partial, grid, nq, k, seed_rows, seed_dist, s, gate);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_bound_collect_mq, dim3(cgrid, nq), dim3(256), 0, s, lo_all, n_pad, k, seed_rows, seed_dist, ctrl, cand, hand_in);
        if (plane8_first) hipLaunchKernelGGL((k_bound_rescore_mq<M, 2>), dim3(nq), dim3(kScanBlock), lds2, s, v, d_queries, k, seed_rows, seed_dist, ctrl, cand, flags, d_stats, d_rows_out, d_dist_out, hand);
        else hipLaunchKernelGGL((k_bound_rescore_mq<M>), dim3(nq), dim3(kScanBlock), lds2, s, v, d_queries, k, seed_rows, seed_dist, ctrl, cand, flags, d_stats, d_rows_out, d_dist_out, (uint32_t*)nullptr);
        return hipSuccess;
    };
    auto run_sets = [&](auto Mc, auto Qc) -> hipError_t { return h_sets ? run(Mc, Qc, std::true_type{}) : run(Mc, Qc, std::false_type{}); };
    auto run_qb = [&](auto Mc) -> hipError_t { return nq <= 4 ? run_sets(Mc, std::integral_constant<int, 4>{}) : run_sets(Mc, std::integral_constant<int, 8>{}); };
    e = v.metric == QV_COSINE ? run_qb(std::integral_constant<int, QV_COSINE>{})
      : v.metric == QV_DOT  ? run_qb(std::integral_constant<int, QV_DOT>{}) : run_qb(std::integral_constant<int, QV_L2>{});
    if (e != hipSuccess) return e;
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_flat_redo_flagged(v, p, d_queries, nq, k, k, flags, redo_ws, d_rows_out, d_dist_out, s, h_sets);
}

}  // namespace qv
