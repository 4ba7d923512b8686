// qv_range.hip — range search: every live row whose float32 distance is within a radius given per query (qv_index_search_range).
//
// The threshold is known before the first row is read, so nothing of a top-k search's selection is needed in front of the rows: no wave
// lists, no published bounds, no k-th smallest.  A pass is a streaming test against a constant and a compaction:
//   k_range_scan_exact<M>   every metric, every index: the exact scan's per-row chain (row_accumulate + finalize, lane == row, so the exact
//                           scan's bits), the test d <= radius, and a (distance, row) key per match into the query's key buffer.  Also
//                           the answer for what the 8-bit stage hands back, and (with `dense`) the redo of a query whose matches
//                           overflow the key buffer.
//   k_range_scan8<M, QB>    stage 1 on the 8-bit plane (cosine, dot, a Euclidean index that holds the planes): QB = 4 or 1 queries share one
//                           read of the plane.  A row passes when the certified lower bound of its distance (bound_scan_interval8, the bound
//                           scan's own function) is within the radius, or when the bound declines the row.  Survivors go to the query's
//                           candidate buffer.
//   k_range_rescore<M>      a wave per survivor: the row's chunks staged in LDS, ONE chain in element order (k_bound_rescore's walk), the
//                           test on the exact distance, a key per match.
// Both compactions reserve per WORKGROUP and tile batch (bound_collect's pattern): the waves gather what passed in LDS (a ballot, one LDS
// atomic per wave and tile), one thread takes the slots with one returning atomic, the workgroup copies.  A counter that runs past its
// buffer keeps counting: the candidate counter says "handed back" (k_range_scan_exact then answers that query alone), the match counter IS
// matches_out, whatever the key buffer held.
// Behind them k_range_finish turns the counters into the counted selection's counts, launch_select_topk_counted orders each query's keys by
// (distance, row) and pads, and a query with more matches than the key buffer holds is redone: k_range_scan_exact writes a key per row
// (dead where the row does not match) and the radix selection takes the max_results smallest — the nearest rows, cut at the radius.
// Everything is decided on the device; nothing is read on the host.
//
// Design points of k_range_scan8, from the resource report (-Rpass-analysis=kernel-resource-usage; profiles/LAB_r34_range.md):
//   the ring: the first kRangeRing 16-byte requests of the wave's NEXT tile, and that tile's norm, scale, residual and live word, are issued
//   before the current tile's epilogue (the float64 interval, the ballots, the LDS atomics, the batch's barriers), so the epilogue runs
//   under loads in flight; the rest of a tile goes in bound8_block's blocks of requests.
//   QB = 4 keeps four sets of four accumulators per lane (16 registers) and reads each plane value once; walking the tile four times out
//   of registers would need the whole tile (dim / 4 registers) resident.
//   kRangeBatch = 2 tiles per wave between two reservations: 2 KiB of LDS per query for the gathered rows.
#include "qv_kernels.h"
#include "qv_bound.h"

namespace qv {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef int i32;

constexpr uint32_t kRangeRing = 8;             // requests of the next tile in flight under the epilogue
constexpr uint32_t kRangeBatch = 2;            // tiles a wave walks between two reservations
constexpr uint32_t kRangeSlots = kScanWaves * kRangeBatch * 64;   // what a workgroup can gather per query and batch
constexpr uint32_t kRangeRescoreGrid = 256;    // 1024 waves: a thousand survivors in one round
struct RangeQuery8 { double sq, qn, qres, pad; };   // k_range_prep8's results per query

// the counters of a piece's queries, one array each (stride = kRangePiece): the counted selection reads `count` as an array
__device__ __forceinline__ uint32_t* range_cand(uint32_t* ctr) { return ctr; }
__device__ __forceinline__ uint32_t* range_match(uint32_t* ctr) { return ctr + kRangePiece; }
__device__ __forceinline__ uint32_t* range_count(uint32_t* ctr) { return ctr + 2 * kRangePiece; }
__device__ __forceinline__ uint32_t* range_redo(uint32_t* ctr) { return ctr + 3 * kRangePiece; }

__global__ void __launch_bounds__(256)
k_range_clear(uint32_t* __restrict__ ctr) {
    for (uint32_t i = threadIdx.x; i < 4 * kRangePiece; i += blockDim.x) ctr[i] = 0u;
}
__global__ void __launch_bounds__(256)
k_range_pad(unsigned long long* __restrict__ matches, uint32_t nq) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq) matches[q] = 0ull;
}

// ---------------------------------------------------------------- the two compaction steps ----
// What passed of the wave's tile into the workgroup's LDS buffer: a ballot, one LDS atomic, a prefix popcount.
template <typename T>
__device__ __forceinline__ void range_emit(bool pass, T val, T* __restrict__ buf /* LDS [kRangeSlots] */, uint32_t* cnt /* LDS */, uint32_t lane) {
    const uint64_t m = __ballot(pass);
    if (m == 0ull) return;                                             // (wave-uniform)
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(cnt, (uint32_t)__builtin_popcountll(m));
    base = __builtin_amdgcn_readfirstlane(base);
    if (pass) buf[base + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = val;   // (a wave adds at most kRangeBatch * 64 per batch: inside kRangeSlots)
}
// The batch's end, every thread of the workgroup: thread j < NQ reserves query j's slots with ONE returning atomic on its global counter
// (which keeps counting past `cap`), the workgroup copies what fits.  Three barriers; s_cnt is left zero for the next batch.
template <typename T, int NQ>
__device__ __forceinline__ void range_flush(T* __restrict__ buf /* LDS [NQ][kRangeSlots] */, uint32_t* s_cnt, uint32_t* s_n, uint32_t* s_base,
                                            uint32_t* __restrict__ gcnt /* [NQ], one word per query */, T* __restrict__ gbuf /* [NQ][cap] */, uint32_t cap, uint32_t nq) {
    __syncthreads();
    if (threadIdx.x < (uint32_t)NQ) {
        const uint32_t n = s_cnt[threadIdx.x];
        s_n[threadIdx.x] = n; s_cnt[threadIdx.x] = 0u;
        s_base[threadIdx.x] = n != 0u && threadIdx.x < nq ? atomicAdd(&gcnt[threadIdx.x], n) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NQ; j++) {
        const uint32_t n = s_n[j], base = s_base[j];
        if ((uint32_t)j < nq)
            for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
                if (base < cap && i < cap - base) gbuf[(size_t)j * cap + base + i] = buf[(size_t)j * kRangeSlots + i];
    }
    __syncthreads();
}
// batches of a launch: the same for every wave of every workgroup, so that the barriers of range_flush are uniform
static uint32_t range_batches(uint32_t n_tiles, uint32_t grid) { const uint32_t per = grid * kScanWaves * kRangeBatch; return (n_tiles + per - 1) / per; }

// ---------------------------------------------------------------- the exact range scan ----
constexpr int kRangeAll = 0, kRangeHandBack = 1, kRangeDense = 2;
template <int M>
__global__ void __launch_bounds__(kScanBlock)
k_range_scan_exact(IndexView v, const float* __restrict__ queries, const float* __restrict__ radius, uint32_t n_batches, uint32_t cand_cap, int mode,
                   uint32_t q_first, uint64_t* __restrict__ keys /* [piece][kRangeKeyCap] */, uint32_t* __restrict__ ctr,
                   uint64_t* __restrict__ dense /* kRangeDense: [n_tiles * 64], a key per row */) {
    using Q = typename MT<M>::Q;
    extern __shared__ __align__(16) unsigned char smem[];
    Q* q_lds = reinterpret_cast<Q*>(smem);
    __shared__ uint64_t s_buf[kRangeSlots];
    __shared__ uint32_t s_cnt[1], s_n[1], s_base[1];
    const uint32_t q = q_first + blockIdx.y;
    if (mode == kRangeHandBack && range_cand(ctr)[q] <= cand_cap) return;          // (the same in every workgroup of the query)
    if (mode == kRangeDense && range_redo(ctr)[q] == 0u) return;
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (threadIdx.x == 0) s_cnt[0] = 0u;
    stage_query<M>(q_lds, queries + (size_t)q * v.dim, v.dim, v.dim4);
    __syncthreads();
    const QConst qc = query_const<M>(q_lds, v.dim);
    const float rad = radius[q];
    const uint32_t tw = gridDim.x * kScanWaves;
    const f4* tiles = reinterpret_cast<const f4*>(v.tiles);
    for (uint32_t b = 0; b < n_batches; b++) {
#pragma unroll 1
        for (uint32_t i = 0; i < kRangeBatch; i++) {
            const uint32_t t = blockIdx.x * kScanWaves + wave + (b * kRangeBatch + i) * tw;
            if (t >= v.n_tiles) break;                                 // (wave-uniform; the barriers are outside this loop)
            // the exact scan's tile: the row walk, then the row's norm and the tile's live word (k_flat_keys' shape)
            const typename MT<M>::A acc = row_accumulate<M, kUnroll, false>(tiles + (size_t)t * v.dim4 * 64 + lane, 64, q_lds, v.dim4);
            const uint32_t row = t * 64 + lane;
            double rn = 0.0;
            if constexpr (MT<M>::needs_rnorm) rn = v.rnorm[row];
            const uint64_t am = v.alive[t];
            const float dist = finalize<M>(acc, qc, rn);
            const bool match = ((am >> lane) & 1ull) && dist <= rad;   // (a NaN distance or radius: false)
            const uint64_t key = make_key(dist, row);
            if (mode == kRangeDense) __builtin_nontemporal_store(match ? key : kDeadKey, &dense[row]);
            else range_emit<uint64_t>(match, key, s_buf, s_cnt, lane);
        }
        if (mode != kRangeDense) range_flush<uint64_t, 1>(s_buf, s_cnt, s_n, s_base, range_match(ctr) + q, keys + (size_t)q * kRangeKeyCap, kRangeKeyCap, 1u);
    }
}

// ---------------------------------------------------------------- stage 1 on the 8-bit plane ----
// The query's two int8 terms and its scale, norm and residual, once per query (bound8_stage_query's arithmetic: sq = max|q_i| / 16256,
// qq = rint(q / sq) = 128 hi + lo, qres = |q - sq qq| rounded up, |q| as the reference's chain; a query without a scale gets qres = NaN,
// and then bound_scan_interval8 declines every row: all of them pass and the candidate buffer overflows into the exact range scan).
__global__ void __launch_bounds__(kScanBlock)
k_range_prep8(const float* __restrict__ queries, uint32_t dim, int8_t* __restrict__ qterm /* [piece][2][dim] */, RangeQuery8* __restrict__ qpar) {
    __shared__ float s_max[kScanWaves];
    __shared__ uint32_t s_bad[kScanWaves];
    __shared__ double s_res[kScanWaves];
    const uint32_t j = blockIdx.x, lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float* __restrict__ query = queries + (size_t)j * dim;
    int8_t* qh8 = qterm + (size_t)j * 2 * dim;
    int8_t* ql8 = qh8 + dim;
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
        int hi, lo;
        const double d = bound8_split_query(x, sq, hi, lo);            // |hi| <= 127, |lo| <= 64: exact
        qh8[i] = (int8_t)hi; ql8[i] = (int8_t)lo;
        r2 = __builtin_fma(d, d, r2);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) r2 += __shfl_xor(r2, m);        // (any order: qres is rounded up behind it)
    if (lane == 0) s_res[wave] = r2;
    double ma = 0.0;
    if (wave == kScanWaves - 1) {
        // |q| as the reference's chain, one wave: 64 values per request, walked in order
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
        RangeQuery8 p;
        p.sq = sq; p.qn = __builtin_sqrt(ma); p.pad = 0.0;
        p.qres = q_ok ? __builtin_sqrt(qres2) * (1.0 + 1e-6) + 1e-300 : __builtin_nan("");   // (1e-6: the shuffled sum's own roundings, far inside it)
        qpar[j] = p;
    }
}

// one 16-dimension step of a lane's row against the QB queries' terms (LDS, uniform address: a broadcast read): bound8_block's eight dot
// products per query, hi terms into acc[j][0 .. 1], lo terms into acc[j][2 .. 3]
template <int QB>
__device__ __forceinline__ void range8_step(const u4 x, const u4* __restrict__ t /* [QB][2] */, i32 (&acc)[QB][4]) {
#pragma unroll
    for (int j = 0; j < QB; j++) {
        const u4 h = t[2 * j], l = t[2 * j + 1];
        acc[j][0] = __builtin_amdgcn_sdot4((i32)h.x, (i32)x.x, acc[j][0], false);
        acc[j][1] = __builtin_amdgcn_sdot4((i32)h.y, (i32)x.y, acc[j][1], false);
        acc[j][0] = __builtin_amdgcn_sdot4((i32)h.z, (i32)x.z, acc[j][0], false);
        acc[j][1] = __builtin_amdgcn_sdot4((i32)h.w, (i32)x.w, acc[j][1], false);
        acc[j][2] = __builtin_amdgcn_sdot4((i32)l.x, (i32)x.x, acc[j][2], false);
        acc[j][3] = __builtin_amdgcn_sdot4((i32)l.y, (i32)x.y, acc[j][3], false);
        acc[j][2] = __builtin_amdgcn_sdot4((i32)l.z, (i32)x.z, acc[j][2], false);
        acc[j][3] = __builtin_amdgcn_sdot4((i32)l.w, (i32)x.w, acc[j][3], false);
    }
}
template <int QB, int U>
__device__ __forceinline__ void range8_block(const u4* __restrict__ p, const u4* __restrict__ terms, uint32_t s0, i32 (&acc)[QB][4]) {
    u4 x[U];
#pragma unroll
    for (int u = 0; u < U; u++) x[u] = __builtin_nontemporal_load(&p[(size_t)(s0 + u) * 64]);
    __builtin_amdgcn_sched_barrier(0);                                 // all requests of the block ahead of the arithmetic (see row_accumulate)
#pragma unroll
    for (int u = 0; u < U; u++) range8_step<QB>(x[u], terms + (size_t)(s0 + u) * QB * 2, acc);
}

// grid (workgroups, groups of QB queries); the launch's first query is q_first, group g holds queries q_first + g QB ... (the launcher cuts
// a piece into groups of 4 and single queries, so every group is full)
template <int M, int QB>
__global__ void __launch_bounds__(kScanBlock)
k_range_scan8(IndexView v, const int8_t* __restrict__ qterm, const RangeQuery8* __restrict__ qpar, const float* __restrict__ radius, uint32_t q_first,
              uint32_t n_batches, uint32_t cand_cap, uint32_t* __restrict__ cand /* [piece][cand_cap] */, uint32_t* __restrict__ ctr) {
    extern __shared__ __align__(16) unsigned char smem[];
    u4* terms = reinterpret_cast<u4*>(smem);                           // [dim / 16][QB][2]: hi, lo of query j for one step
    __shared__ uint32_t s_buf[QB * kRangeSlots];
    __shared__ uint32_t s_cnt[QB], s_n[QB], s_base[QB];
    __shared__ RangeQuery8 s_par[QB];
    __shared__ float s_rad[QB];
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t steps = v.dim >> 4, tw = gridDim.x * kScanWaves;
    const uint32_t q0 = q_first + blockIdx.y * QB;
    for (uint32_t i = threadIdx.x; i < steps * QB * 2; i += blockDim.x) {
        const uint32_t s = i / (QB * 2), j = (i / 2) % QB, h = i & 1u;
        terms[i] = reinterpret_cast<const u4*>(qterm + ((size_t)(q0 + j) * 2 + h) * v.dim)[s];
    }
    if (threadIdx.x < (uint32_t)QB) { s_cnt[threadIdx.x] = 0u; s_par[threadIdx.x] = qpar[q0 + threadIdx.x]; s_rad[threadIdx.x] = radius[q0 + threadIdx.x]; }
    __syncthreads();

    const u4* plane = reinterpret_cast<const u4*>(v.plane8) + lane;
    // the ring: what is requested of the wave's next tile before the current one's epilogue
    u4 pre[kRangeRing];
    double rn_n = 0.0; float sc_n = 0.f, rr_n = 0.f; uint64_t am_n = 0ull;
    auto request = [&](uint32_t t) {
        if (t >= v.n_tiles) return;                                    // (wave-uniform)
        const u4* p = plane + (size_t)t * steps * 64;
#pragma unroll
        for (uint32_t u = 0; u < kRangeRing; u++) if (u < steps) pre[u] = __builtin_nontemporal_load(&p[(size_t)u * 64]);
        rn_n = v.rnorm[t * 64 + lane]; sc_n = v.rscale8[t * 64 + lane]; rr_n = v.rres8[t * 64 + lane];
        am_n = v.alive[t];
        __builtin_amdgcn_sched_barrier(0);                             // issued here, ahead of the epilogue's arithmetic
    };
    request(blockIdx.x * kScanWaves + wave);
    for (uint32_t b = 0; b < n_batches; b++) {
#pragma unroll 1
        for (uint32_t i = 0; i < kRangeBatch; i++) {
            const uint32_t t = blockIdx.x * kScanWaves + wave + (b * kRangeBatch + i) * tw;
            if (t >= v.n_tiles) break;                                 // (wave-uniform; the barriers are outside this loop)
            const double rn = rn_n; const float sc = sc_n, rr = rr_n; const uint64_t am = am_n;
            i32 acc[QB][4];
#pragma unroll
            for (int j = 0; j < QB; j++) { acc[j][0] = 0; acc[j][1] = 0; acc[j][2] = 0; acc[j][3] = 0; }
#pragma unroll
            for (uint32_t u = 0; u < kRangeRing; u++) if (u < steps) range8_step<QB>(pre[u], terms + (size_t)u * QB * 2, acc);
            const u4* p = plane + (size_t)t * steps * 64;
            uint32_t s = kRangeRing;
            for (; s + 8 <= steps; s += 8) range8_block<QB, 8>(p, terms, s, acc);   // (blocks of 16 beside the ring: 176 registers, 2 waves per SIMD)
            if (s + 4 <= steps) { range8_block<QB, 4>(p, terms, s, acc); s += 4; }
            if (s + 2 <= steps) { range8_block<QB, 2>(p, terms, s, acc); s += 2; }
            if (s < steps) range8_block<QB, 1>(p, terms, s, acc);
            request(t + tw);                                           // the wave's next tile, whichever batch it falls in
            const bool live = (am >> lane) & 1ull;                     // (dead rows and the last tile's padding never pass)
            const uint32_t row = t * 64 + lane;
#pragma unroll
            for (int j = 0; j < QB; j++) {
                // (each partial sum exact in int32: dim <= 4096)
                const long long isum = ((long long)acc[j][0] + (long long)acc[j][1]) * 128ll + ((long long)acc[j][2] + (long long)acc[j][3]);
                float lo, hi;
                const bool sure = bound_scan_interval8<M>(isum, s_par[j].sq, s_par[j].qn, s_par[j].qres, rn, sc, rr, v.dim, lo, hi);   // (d_hi's chain is dead code here)
                // d >= d_lo, so a row with d <= radius has d_lo <= radius; a row the bound declines always passes
                range_emit<uint32_t>(live && (!sure || lo <= s_rad[j]), row, s_buf + (size_t)j * kRangeSlots, &s_cnt[j], lane);
            }
        }
        range_flush<uint32_t, QB>(s_buf, s_cnt, s_n, s_base, range_cand(ctr) + q0, cand + (size_t)q0 * cand_cap, cand_cap, (uint32_t)QB);
    }
}

// ---------------------------------------------------------------- the re-score: a wave per survivor ----
// grid (kRangeRescoreGrid, queries).  k_bound_rescore's walk: the row's chunks requested at once over the wave's lanes, staged in LDS, then ONE
// chain acc1<M> over elements 0 .. dim - 1 against the staged query and finalize<M> — row_accumulate's chain in its order, the exact scan's bits.
// A query whose candidates overflowed is left to k_range_scan_exact behind this launch.
template <int M>
__global__ void __launch_bounds__(kScanBlock)
k_range_rescore(IndexView v, const float* __restrict__ queries, const float* __restrict__ radius, uint32_t q_first, uint32_t cand_cap,
                const uint32_t* __restrict__ cand, uint64_t* __restrict__ keys, uint32_t* __restrict__ ctr) {
    using Q = typename MT<M>::Q;
    extern __shared__ __align__(16) unsigned char smem[];
    Q* q_lds = reinterpret_cast<Q*>(smem);
    const size_t q_bytes = (((size_t)v.dim4 * 4 * sizeof(Q)) + 15) / 16 * 16;
    float* rbuf = reinterpret_cast<float*>(smem + q_bytes);            // [kScanWaves][dim4 * 4]: a wave's survivor
    const uint32_t q = q_first + blockIdx.y;
    const uint32_t ns = range_cand(ctr)[q];
    if (ns > cand_cap || blockIdx.x * kScanWaves >= ns) return;        // handed back, or no survivor for this workgroup
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    stage_query<M>(q_lds, queries + (size_t)q * v.dim, v.dim, v.dim4);
    __syncthreads();
    const QConst qc = query_const<M>(q_lds, v.dim);
    const float rad = radius[q];
    const f4* tiles = reinterpret_cast<const f4*>(v.tiles);
    f4* mine = reinterpret_cast<f4*>(rbuf + (size_t)wave * v.dim4 * 4);
    const uint32_t* my_cand = cand + (size_t)q * cand_cap;
    for (uint32_t i = blockIdx.x * kScanWaves + wave; i < ns; i += gridDim.x * kScanWaves) {   // (wave-uniform)
        const uint32_t row = my_cand[i];
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
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");         // the wave's own LDS writes before its reads of other lanes' chunks
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        typename MT<M>::A acc = 0;
        for (uint32_t c = 0; c < v.dim4; c++) {                        // ONE chain, element order: row_accumulate's
            const f4 r = mine[c];
            const Q* qq = q_lds + (size_t)c * 4;
            acc1<M>(acc, qq[0], r.x); acc1<M>(acc, qq[1], r.y); acc1<M>(acc, qq[2], r.z); acc1<M>(acc, qq[3], r.w);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");         // ... and those reads before the next survivor's writes
        __builtin_amdgcn_wave_barrier();
        const float dist = finalize<M>(acc, qc, rn);
        if (lane == 0 && dist <= rad) {                                // (stage 1 passed live rows only)
            const uint32_t pos = atomicAdd(&range_match(ctr)[q], 1u);
            if (pos < kRangeKeyCap) keys[(size_t)q * kRangeKeyCap + pos] = make_key(dist, row);
        }
    }
}

// The counters into what the stages behind read: matches_out, the counted selection's count (zero for a query that is redone), the redo
// flag; and the index's counters.
// A workgroup per query.  The counted selection writes its first kk sorted slots and sorts only the power of two that holds the count, so a
// query with fewer matches than kk gets dead keys up to kk and a count of kk: the padding is then the selection's own.
__global__ void __launch_bounds__(256)
k_range_finish(uint32_t* __restrict__ ctr, uint32_t cand_cap, int plane, uint32_t kk, uint64_t* __restrict__ keys, unsigned long long* __restrict__ matches_out,
               uint32_t* __restrict__ stats) {
    const uint32_t q = blockIdx.x;
    const uint32_t m = range_match(ctr)[q], c = range_cand(ctr)[q];
    const bool over = m > kRangeKeyCap;
    for (uint32_t i = m + threadIdx.x; i < kk; i += blockDim.x) keys[(size_t)q * kRangeKeyCap + i] = kDeadKey;   // (kk <= kRangeKeyCap; nothing when m >= kk)
    if (threadIdx.x != 0) return;
    matches_out[q] = m;
    range_count(ctr)[q] = over ? 0u : (m > kk ? m : kk);
    range_redo(ctr)[q] = over ? 1u : 0u;
    (void)atomicAdd(&stats[kRangeStatsWord], 1u);
    if (plane) {
        (void)atomicAdd(&stats[kRangeStatsWord + 1], 1u);
        if (c > cand_cap) (void)atomicAdd(&stats[kRangeStatsWord + 2], 1u);
        else (void)atomicAdd(&stats[kRangeStatsWord + 3], c);
    }
}

// ---------------------------------------------------------------- the rule, the workspace, the launcher ----
int range_plane_mode(int mode) { static const int env_mode = env_int("QV_RANGE_PLANE", 0); return mode ? mode : env_mode; }
// QV_RANGE_PLANE_AUTO takes nothing: no cell has been measured faster than the exact range scan by more than both arms' spread
// (profiles/LAB_r34_range.md).  A measured cell goes here, with its figures.
bool range_plane_applies(int rule_metric, uint32_t dim, uint32_t rows, uint32_t nq, int mode, bool has_plane8) {
    const bool metric_ok = rule_metric == QV_COSINE || rule_metric == QV_DOT || rule_metric == QV_RULE_L2_PLANES;
    const bool dim_ok = dim >= 16 && (dim & 15u) == 0 && dim <= 4096;
    return metric_ok && has_plane8 && dim_ok && rows >= 1 && nq >= 1 && range_plane_mode(mode) == QV_RANGE_PLANE_ALWAYS;
}

// rows the candidate buffer holds per query; a test shrinks it (QV_RANGE_CAND_CAP, read per call) to reach the hand-back
uint32_t range_cand_cap() { return (uint32_t)std::min(env_int("QV_RANGE_CAND_CAP", (int)kRangeCandCap), (int)kRangeCandCap); }

struct RangeLayout { uint32_t* ctr; RangeQuery8* qpar; int8_t* qterm; uint32_t* cand; uint64_t* keys; uint64_t* dense; void* sel_ws; size_t end, total; };
static RangeLayout range_layout(void* base, uint32_t nq, uint32_t kk, uint32_t n_tiles, uint32_t dim, WsLog* log = nullptr) {
    WsCarver w{static_cast<char*>(base), 0, 0, log};
    const uint32_t piece = std::min(nq, kRangePiece);
    const size_t n = (size_t)n_tiles * 64;
    RangeLayout L{};
    L.ctr = w.take256<uint32_t>(4 * kRangePiece);                      // candidates, matches, the selection's counts, redo flags
    L.qpar = w.take256<RangeQuery8>(piece);
    L.qterm = w.take256<int8_t>((size_t)piece * 2 * ((dim + 15) / 16 * 16));
    L.cand = w.take256<uint32_t>((size_t)piece * kRangeCandCap);       // stage 1's survivors
    L.keys = w.take256<uint64_t>((size_t)piece * kRangeKeyCap);        // a key per match
    L.dense = w.take256<uint64_t>(n > kRangeKeyCap ? n : 0);           // a key per row, one query at a time: the redo of more matches than keys
    L.sel_ws = w.take<char>(n > kRangeKeyCap ? select_workspace_bytes(1, kk) : 0);
    return w.finish(L);
}
size_t range_workspace_bytes(uint32_t nq, uint32_t kk, uint32_t n_tiles, uint32_t dim, WsLog* log) { return range_layout(nullptr, nq, kk, n_tiles, dim, log).total; }

hipError_t launch_range_pad(uint64_t* d_matches, uint32_t nq, hipStream_t s) {
    hipLaunchKernelGGL(k_range_pad, dim3((nq + 255) / 256), dim3(256), 0, s, reinterpret_cast<unsigned long long*>(d_matches), nq);
    return hipGetLastError();
}

template <int M>
static hipError_t range_stage8(const IndexView& v, const ScanPlan& p, const float* d_queries, const float* d_radius, uint32_t nq, uint32_t cand_cap,
                               const RangeLayout& L, uint32_t n_batches, hipStream_t s) {
    hipLaunchKernelGGL(k_range_prep8, dim3(nq), dim3(kScanBlock), 0, s, d_queries, v.dim, L.qterm, L.qpar);
    const uint32_t n4 = nq / 4, rem = nq % 4;
    if (n4) hipLaunchKernelGGL((k_range_scan8<M, 4>), dim3(p.grid, n4), dim3(kScanBlock), (size_t)v.dim * 2 * 4, s, v, L.qterm, L.qpar, d_radius, 0u, n_batches, cand_cap, L.cand, L.ctr);
    if (rem) hipLaunchKernelGGL((k_range_scan8<M, 1>), dim3(p.grid, rem), dim3(kScanBlock), (size_t)v.dim * 2, s, v, L.qterm, L.qpar, d_radius, n4 * 4, n_batches, cand_cap, L.cand, L.ctr);
    const size_t lds = query_lds_bytes(M, v.dim4) + (size_t)kScanWaves * v.dim4 * 4 * sizeof(float);
    hipError_t e = set_lds(k_range_rescore<M>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_range_rescore<M>, dim3(kRangeRescoreGrid, nq), dim3(kScanBlock), lds, s, v, d_queries, d_radius, 0u, cand_cap, L.cand, L.keys, L.ctr);
    return hipGetLastError();
}

// One piece of at most kRangePiece queries: outputs [nq][kk], padded; d_matches [nq].  plane: range_plane_applies said yes.
hipError_t launch_range_search(const IndexView& v, const ScanPlan& p, const float* d_queries, const float* d_radius, uint32_t nq, uint32_t kk, bool plane,
                               void* d_ws, uint32_t* d_stats, uint32_t* d_rows_out, float* d_dist_out, uint64_t* d_matches, hipStream_t s) {
    if (nq == 0 || nq > kRangePiece || kk == 0 || kk > QV_RANGE_MAX_RESULTS || v.n_tiles == 0) return hipErrorInvalidValue;
    if (plane && (v.plane8 == nullptr || (v.dim & 15u) || v.dim > 4096 || !(v.metric == QV_COSINE || v.metric == QV_DOT || (v.metric == QV_L2 && v.l2_planes)))) return hipErrorInvalidValue;
    const RangeLayout L = range_layout(d_ws, nq, kk, v.n_tiles, v.dim);
    const uint32_t cand_cap = range_cand_cap(), n_batches = range_batches(v.n_tiles, p.grid);
    const size_t n = (size_t)v.n_tiles * 64;
    const size_t lds = query_lds_bytes(v.metric, v.dim4);
    hipError_t e = hipSuccess;
    hipLaunchKernelGGL(k_range_clear, dim3(1), dim3(256), 0, s, L.ctr);
    if (plane) {
        if (v.metric == QV_COSINE) e = range_stage8<QV_COSINE>(v, p, d_queries, d_radius, nq, cand_cap, L, n_batches, s);
        else if (v.metric == QV_DOT) e = range_stage8<QV_DOT>(v, p, d_queries, d_radius, nq, cand_cap, L, n_batches, s);
        else e = range_stage8<QV_L2>(v, p, d_queries, d_radius, nq, cand_cap, L, n_batches, s);
        if (e != hipSuccess) return e;
    }
    QV_DISPATCH_METRIC(v.metric, {
        e = set_lds(k_range_scan_exact<MM>, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_range_scan_exact<MM>, dim3(p.grid, nq), dim3(kScanBlock), lds, s, v, d_queries, d_radius, n_batches, cand_cap, plane ? kRangeHandBack : kRangeAll, 0u,
                           L.keys, L.ctr, (uint64_t*)nullptr);
    });
    hipLaunchKernelGGL(k_range_finish, dim3(nq), dim3(256), 0, s, L.ctr, cand_cap, plane ? 1 : 0, kk, L.keys, reinterpret_cast<unsigned long long*>(d_matches), d_stats);
    e = launch_select_topk_counted(L.keys, kRangeKeyCap, kRangeKeyCap, L.ctr + 2 * kRangePiece, nq, kk, kk, d_rows_out, d_dist_out, s, nullptr);
    if (e != hipSuccess) return e;
    if (n <= kRangeKeyCap) return hipGetLastError();                   // every match has a key: nothing can be redone
    // more matches than keys: the max_results nearest, cut at the radius — a key per row, dead where the row does not match, and the radix
    // selection; one query at a time behind its flag word (every launch leaves at once where the flag is zero)
    for (uint32_t q = 0; q < nq; q++) {
        QV_DISPATCH_METRIC(v.metric, {
            hipLaunchKernelGGL(k_range_scan_exact<MM>, dim3(p.grid, 1), dim3(kScanBlock), lds, s, v, d_queries, d_radius, n_batches, cand_cap, kRangeDense, q, L.keys, L.ctr, L.dense);
        });
        e = launch_select_topk(L.dense, n, (uint32_t)n, 1, kk, kk, L.sel_ws, d_rows_out + (size_t)q * kk, d_dist_out + (size_t)q * kk, s, false, true, L.ctr + 3 * kRangePiece + q);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

}  // namespace qv
