// qv_scan.hip — flat scan + fused top-k (single- and multi-query), list merges
// (shared helpers, the arithmetic contract and the build flags: qv_kernels.h)
#include "qv_kernels.h"
#include "qv_bound.h"

namespace qv {

// ---------------------------------------------------------------- flat scan --------
// grid = (workgroups, nq); each wave walks tiles gw, gw+tw, ... ; lane == row.
// Output: partial[(q*gridDim.x + blockIdx.x)*k + i] = workgroup's i-th best key.

__device__ void merge_lists_last_workgroup(const uint64_t* src, uint32_t n_lists, uint32_t k, uint32_t* rows_out, float* dist_out, uint32_t* done_flag = nullptr, uint32_t done_seq = 0);

// FUSE: the workgroups publish their lists with returning atomic exchanges and take a ticket; the LAST one to finish merges all of
// them (k_merge_lists' own code) and writes the final rows / distances — one launch per query instead of two (round 5: a single
// query over 1M x 768 is 0.44 ms of scan; the second launch and the gap in front of it were 2 % of it).  tickets[qi]: zero before
// the first launch, left zero.  Nothing crosses workgroups through a fence (see k_flat_scan_small).
template <int M, int U, bool FUSE = false>
__global__ void __launch_bounds__(kScanBlock)
k_flat_scan(IndexView v, const float* __restrict__ queries, uint32_t k, uint64_t* __restrict__ partial,
            uint32_t* __restrict__ tickets = nullptr, uint32_t* __restrict__ rows_out = nullptr, float* __restrict__ dist_out = nullptr,
            uint32_t* done_flag = nullptr, uint32_t done_seq = 0, const uint32_t* __restrict__ gate = nullptr) {
    using Q = typename MT<M>::Q;
    // gate: the launch behind a bound scan (k_bound_rescore wrote the word): zero = that scan has answered, leave at once
    if constexpr (FUSE) { if (gate != nullptr && *gate == 0u) return; }
    extern __shared__ __align__(16) unsigned char smem[];
    Q* q_lds = reinterpret_cast<Q*>(smem);
    uint64_t* wl = reinterpret_cast<uint64_t*>(smem + (((size_t)v.dim4 * 4 * sizeof(Q)) + 15) / 16 * 16);  // [kScanWaves][64]

    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t qi = blockIdx.y;
    stage_query<M>(q_lds, queries + (size_t)qi * v.dim, v.dim, v.dim4);
    __syncthreads();

    const uint32_t tw = gridDim.x * kScanWaves;
    const uint32_t kth = k - 1;
    uint64_t list = kDeadKey, thr = kDeadKey;
    const f4* tiles = reinterpret_cast<const f4*>(v.tiles);
    QConst qc; qc.qn = 0.0; qc.qn32 = 0.0f;

    auto finish_tile = [&](uint32_t t, typename MT<M>::A acc, bool first) {
        const uint32_t row = t * 64 + lane;
        double rn = 0.0;
        if constexpr (MT<M>::needs_rnorm) rn = v.rnorm[row];
        float dist = finalize<M>(acc, qc, rn);
        uint64_t am = v.alive[t];                                     // wave-uniform
        uint64_t key = ((am >> lane) & 1ull) ? make_key(dist, row) : kDeadKey;
        if (first) { list = wave_sort64(key, lane); thr = readlane64(list, kth); }   // empty list: sort the tile outright
        else list_insert(list, thr, key, kth, lane);
    };

    uint32_t t = blockIdx.x * kScanWaves + wave;
    if (t < v.n_tiles) {                                              // first tile: query norm rides along
        typename MT<M>::A qn2 = 0;
        typename MT<M>::A acc = row_accumulate<M, U, true>(tiles + (size_t)t * v.dim4 * 64 + lane, 64, q_lds, v.dim4, &qn2);
        qc = qconst_from_norm2<M>(qn2);
        finish_tile(t, acc, true);
        t += tw;
    }
    for (; t < v.n_tiles; t += tw) {
        typename MT<M>::A acc = row_accumulate<M, U, false>(tiles + (size_t)t * v.dim4 * 64 + lane, 64, q_lds, v.dim4);
        finish_tile(t, acc, false);
    }

    // workgroup merge: waves 1.. hand their lists to wave 0 through LDS
    wl[wave * 64 + lane] = list;
    __syncthreads();
    if (wave == 0) {
        for (uint32_t w = 1; w < kScanWaves; w++) {
            uint64_t key = lane < k ? wl[w * 64 + lane] : kDeadKey;
            list_insert(list, thr, key, kth, lane);
        }
        if constexpr (!FUSE) {
            if (lane < k) partial[((size_t)qi * gridDim.x + blockIdx.x) * k + lane] = list;
        } else {
            uint64_t* mine = partial + ((size_t)qi * gridDim.x + blockIdx.x) * k;
            if (lane < k) (void)atomicExch(reinterpret_cast<unsigned long long*>(&mine[lane]), (unsigned long long)list);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // every lane's exchange has returned: the list is at the memory side
            uint32_t last = 0;
            if (lane == 0) last = atomicAdd(&tickets[qi], 1u) == gridDim.x - 1 ? 1u : 0u;
            last = __builtin_amdgcn_readfirstlane(last);
            if (last && lane == 0) tickets[qi] = 0;                    // for the next launch on this workspace (stream order)
            if (lane == 0) wl[0] = last;
        }
    }
    if constexpr (FUSE) {
        __syncthreads();
        if (!(uint32_t)wl[0]) return;
        __syncthreads();                                               // (wl is the merge's scratch next)
        merge_lists_last_workgroup(partial + (size_t)qi * gridDim.x * k, gridDim.x, k, rows_out + (size_t)qi * k, dist_out + (size_t)qi * k, done_flag, done_seq);
    }
}

// ---------------------------------------------------------------- flat scan of a short corpus: a tile over several waves --
// k_flat_scan gives a wave whole tiles: 64 rows x dim x 4 bytes (196 KB at 768 dimensions) streamed through 16 loads in flight and a
// dim-step float64 chain — ~30 us per tile whatever the corpus, which IS the scan below a few hundred thousand rows (measured, one
// query, 768 dimensions: 10 k rows 31 us, 30 k 57 us, 100 k 72 us of kernel against 4 / 13 / 43 us of HBM time).  Here the eight waves
// of a workgroup share a tile: wave w requests columns [w, w + 1) * dim / 8 of its 64 rows (every load in flight at once) and walks
// them, lane == row, as a partial chain; the tile's consumer wave (they take turns) adds the eight partial sums and takes the float32
// from the CERTIFICATE of qv_hnsw.hip ("a row's sum over several lanes, certified"): the reference's single chain lies within
// B = (2 dim + 128) u |q| |r| of the partial chains' sum, the float32 is a monotone function of that sum, so when both ends of the
// interval give the same float32 it is the reference's.  For cosine the query's norm is itself a sum here (the reference's is a chain
// over the same squares): its relative uncertainty d goes into the interval as (|S| + B) 2 d — the quotient S / (|q| |r|) is the same
// real number whether the error sits in S or in |q|.  A row that fails (a few in a million; every row at distance ~0) is walked again
// as ONE chain by row_accumulate, with the query's norm as a chain as well: the reference's arithmetic, unchanged.
// Lists are published and merged exactly as in k_flat_scan<., ., true> (returning exchanges, a ticket, the last workgroup merges).
constexpr int kSplitWaves = 8;
constexpr int kSplitBlock = 64 * kSplitWaves;
template <int M> struct ScanSplitOK { static constexpr bool value = M == QV_COSINE || M == QV_DOT || M == QV_L2 || M == QV_L1 || M == QV_L2SQ_F64; };
template <int M>
__global__ void __launch_bounds__(kSplitBlock)
k_flat_scan_split(IndexView v, const float* __restrict__ queries, uint32_t k, uint64_t* __restrict__ partial,
                  uint32_t* __restrict__ tickets, uint32_t* __restrict__ rows_out, float* __restrict__ dist_out, uint32_t* done_flag, uint32_t done_seq) {
    using Q = typename MT<M>::Q;
    using A = typename MT<M>::A;
    extern __shared__ __align__(16) unsigned char smem[];
    Q* q_lds = reinterpret_cast<Q*>(smem);
    const size_t q_bytes = (((size_t)v.dim4 * 4 * sizeof(Q)) + 15) / 16 * 16;
    double* part = reinterpret_cast<double*>(smem + q_bytes);                      // [2][kSplitWaves][64]
    uint64_t* wl = reinterpret_cast<uint64_t*>(smem + q_bytes + 2 * kSplitWaves * 64 * sizeof(double));   // [kSplitWaves][64]
    __shared__ double s_red[kSplitWaves];
    __shared__ uint32_t s_last;
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t qi = blockIdx.y;
    const float* q = queries + (size_t)qi * v.dim;
    stage_query<M>(q_lds, q, v.dim, v.dim4);
    __syncthreads();
    // |q|^2 as a sum over the workgroup (cosine, dot): its place in the certificate, see above.  (From the staged copy: the query
    // may live in host memory.)
    double qn_s = 0.0;
    if constexpr (M == QV_COSINE || M == QV_DOT) {
        double sq = 0.0;
        for (uint32_t i = threadIdx.x; i < v.dim4 * 4; i += kSplitBlock) { const double a = (double)q_lds[i]; sq = __builtin_fma(a, a, sq); }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sq = sq + __shfl_xor(sq, off);
        if (lane == 0) s_red[wave] = sq;
        __syncthreads();
        sq = s_red[0];
#pragma unroll
        for (int w = 1; w < kSplitWaves; w++) sq = sq + s_red[w];
        qn_s = __builtin_sqrt(sq);
    }
    const double k_u = ((double)(2u * v.dim) + 128.0) * 0x1p-53;
    QConst qc; qc.qn = qn_s; qc.qn32 = 0.0f;                                         // (cosine: used with the widened interval; the fallback makes its own)
    QConst qc_exact; qc_exact.qn = 0.0; qc_exact.qn32 = 0.0f; bool have_exact = false;

    const uint32_t kth = k - 1;
    uint64_t list = kDeadKey, thr = kDeadKey;
    bool first = true;
    const f4* tiles = reinterpret_cast<const f4*>(v.tiles);
    const uint32_t c_lo = wave * v.dim4 / kSplitWaves, c_hi = (wave + 1) * v.dim4 / kSplitWaves;
    uint32_t it = 0;
    for (uint32_t t = blockIdx.x; t < v.n_tiles; t += gridDim.x, it++) {
        const uint32_t consumer = it % kSplitWaves;
        const uint32_t row = t * 64 + lane;
        double rn = 0.0; uint64_t am = 0;
        if (wave == consumer) {                                                      // (requested before the columns: they have arrived by the time they are used)
            if constexpr (MT<M>::needs_rnorm || M == QV_DOT) rn = v.rnorm[row];
            am = v.alive[t];
        }
        A acc = 0;
        if (c_lo < c_hi) acc = row_accumulate<M, 24, false, true, false>(tiles + ((size_t)t * v.dim4 + c_lo) * 64 + lane, 64, q_lds + (size_t)c_lo * 4, c_hi - c_lo);
        double* pb = part + (size_t)(it & 1u) * kSplitWaves * 64;
        pb[wave * 64 + lane] = (double)acc;
        __syncthreads();                                                             // one barrier per tile: the buffer written two tiles ahead is free by then
        if (wave != consumer) continue;
        double sum = pb[lane];
#pragma unroll
        for (int w = 1; w < kSplitWaves; w++) sum = sum + pb[w * 64 + lane];
        double b;
        if constexpr (M == QV_COSINE || M == QV_DOT) b = k_u * qn_s * rn; else b = k_u * sum;
        if constexpr (M == QV_COSINE) b = b + (__builtin_fabs(sum) + b) * (2.0 * k_u);    // the norm's own uncertainty (<= k_u / 2 + 3 u relative), twice over
        const float d_lo = finalize<M>((A)(sum - b), qc, rn), d_hi = finalize<M>((A)(sum + b), qc, rn);
        float dist = d_lo;
        const bool live = (am >> lane) & 1ull;
        const bool ok = __float_as_uint(d_lo) == __float_as_uint(d_hi) && d_lo == d_lo;
        if (__ballot(live && !ok)) {
            // the reference's own arithmetic for this tile: one chain per row (and for the query's norm, once per workgroup)
            A qn2 = 0;
            A ex;
            if (!have_exact) { ex = row_accumulate<M, 16, true, true, false>(tiles + (size_t)t * v.dim4 * 64 + lane, 64, q_lds, v.dim4, &qn2); qc_exact = qconst_from_norm2<M>(qn2); have_exact = true; }
            else ex = row_accumulate<M, 16, false, true, false>(tiles + (size_t)t * v.dim4 * 64 + lane, 64, q_lds, v.dim4);
            const float de = finalize<M>(ex, qc_exact, rn);
            if (!ok) dist = de;
        }
        const uint64_t key = live ? make_key(dist, row) : kDeadKey;
        if (first) { list = wave_sort64(key, lane); thr = readlane64(list, kth); first = false; }
        else list_insert(list, thr, key, kth, lane);
    }
    // the waves' lists -> wave 0 -> published; the last workgroup to finish merges (k_flat_scan<., ., true>'s protocol)
    wl[wave * 64 + lane] = list;
    __syncthreads();
    if (wave == 0) {
        if (first) { list = kDeadKey; thr = kDeadKey; }
        for (uint32_t w = 1; w < kSplitWaves; w++) {
            const uint64_t key = lane < k ? wl[w * 64 + lane] : kDeadKey;
            if (first) { list = wave_sort64(key, lane); thr = readlane64(list, kth); first = false; }
            else list_insert(list, thr, key, kth, lane);
        }
        uint64_t* mine = partial + ((size_t)qi * gridDim.x + blockIdx.x) * k;
        if (lane < k) (void)atomicExch(reinterpret_cast<unsigned long long*>(&mine[lane]), (unsigned long long)list);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint32_t last = 0;
        if (lane == 0) last = atomicAdd(&tickets[qi], 1u) == gridDim.x - 1 ? 1u : 0u;
        last = __builtin_amdgcn_readfirstlane(last);
        if (last && lane == 0) tickets[qi] = 0;
        if (lane == 0) s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    merge_lists_last_workgroup(partial + (size_t)qi * gridDim.x * k, gridDim.x, k, rows_out + (size_t)qi * k, dist_out + (size_t)qi * k, done_flag, done_seq);
}

// The same for the few queries of a shared pass (concurrent callers on a short corpus: qv_coalesce.h): up to QB queries per workgroup row
// (blockIdx.y = group of QB).  k_flat_scan_mq gives a wave whole tiles and QB chains of dim steps per row — 16 queries over 10 k x 768
// took 280 us, all of it chains.  Here a wave converts each element of its columns once and feeds QB partial chains (768 fma + 96
// converts per tile and wave at 768 dimensions and QB = 8: ~3 us, what the tile's bytes take to arrive); wave j is query j's consumer
// on every tile, so its list is the workgroup's list for that query: no merge inside the workgroup.  Lists go to partial[q][grid][k];
// k_merge_lists follows as for the other multi-query scans.
template <int M, int QB>
__global__ void __launch_bounds__(kSplitBlock)
k_flat_scan_split_mq(IndexView v, const float* __restrict__ queries, uint32_t nq, uint32_t k, uint64_t* __restrict__ partial) {
    static_assert(QB <= kSplitWaves, "one consumer wave per query");
    using Q = typename MT<M>::Q;
    using A = typename MT<M>::A;
    extern __shared__ __align__(16) unsigned char smem[];
    const size_t q_stride = (size_t)v.dim4 * 4;                                    // elements per staged query
    Q* q_lds = reinterpret_cast<Q*>(smem);                                         // [QB][dim4 * 4]
    const size_t q_bytes = ((size_t)QB * q_stride * sizeof(Q) + 15) / 16 * 16;
    double* part = reinterpret_cast<double*>(smem + q_bytes);                      // [QB][kSplitWaves][64]
    __shared__ double s_red[QB][kSplitWaves];
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t q0 = blockIdx.y * QB;
    const uint32_t nqg = nq - q0 < (uint32_t)QB ? nq - q0 : (uint32_t)QB;          // queries of this group
    for (uint32_t j = 0; j < (uint32_t)QB; j++) {
        const float* q = queries + (size_t)(q0 + (j < nqg ? j : 0)) * v.dim;       // (slots past the group repeat its first query: computed, never written)
        for (uint32_t i = threadIdx.x; i < q_stride; i += kSplitBlock) q_lds[j * q_stride + i] = i < v.dim ? (Q)q[i] : (Q)0;
    }
    __syncthreads();
    double qn_s = 0.0;                                                             // of THIS wave's query (wave j consumes query j)
    if constexpr (M == QV_COSINE || M == QV_DOT) {
        for (uint32_t j = 0; j < (uint32_t)QB; j++) {
            double sq = 0.0;
            for (uint32_t i = threadIdx.x; i < q_stride; i += kSplitBlock) { const double a = (double)q_lds[j * q_stride + i]; sq = __builtin_fma(a, a, sq); }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) sq = sq + __shfl_xor(sq, off);
            if (lane == 0) s_red[j][wave] = sq;
        }
        __syncthreads();
        if (wave < (uint32_t)QB) {
            double sq = s_red[wave][0];
#pragma unroll
            for (int w = 1; w < kSplitWaves; w++) sq = sq + s_red[wave][w];
            qn_s = __builtin_sqrt(sq);
        }
    }
    const double k_u = ((double)(2u * v.dim) + 128.0) * 0x1p-53;
    QConst qc; qc.qn = qn_s; qc.qn32 = 0.0f;
    QConst qc_exact; qc_exact.qn = 0.0; qc_exact.qn32 = 0.0f; bool have_exact = false;
    const uint32_t kth = k - 1;
    uint64_t list = kDeadKey, thr = kDeadKey;
    bool first = true;
    const f4* tiles = reinterpret_cast<const f4*>(v.tiles);
    const uint32_t c_lo = wave * v.dim4 / kSplitWaves, c_hi = (wave + 1) * v.dim4 / kSplitWaves;
    const bool consumer = wave < nqg;
    const Q* my_q = q_lds + (size_t)(wave < (uint32_t)QB ? wave : 0) * q_stride;
    for (uint32_t t = blockIdx.x; t < v.n_tiles; t += gridDim.x) {
        const uint32_t row = t * 64 + lane;
        double rn = 0.0; uint64_t am = 0;
        if (consumer) {
            if constexpr (MT<M>::needs_rnorm || M == QV_DOT) rn = v.rnorm[row];
            am = v.alive[t];
        }
        A acc[QB];
#pragma unroll
        for (int j = 0; j < QB; j++) acc[j] = 0;
        const f4* p = tiles + ((size_t)t * v.dim4 + c_lo) * 64 + lane;
        for (uint32_t c = c_lo; c < c_hi; c += 8) {                                  // eight chunks requested together, each element widened once for all queries
            f4 x[8];
#pragma unroll
            for (int u = 0; u < 8; u++) x[u] = c + (uint32_t)u < c_hi ? p[(size_t)(c - c_lo + u) * 64] : f4{0.f, 0.f, 0.f, 0.f};
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 8; u++) {
                if (c + (uint32_t)u < c_hi) {
#pragma unroll
                    for (int j = 0; j < QB; j++) {
                        const Q* qq = q_lds + (size_t)j * q_stride + (size_t)(c + u) * 4;
                        acc1<M>(acc[j], qq[0], x[u].x); acc1<M>(acc[j], qq[1], x[u].y); acc1<M>(acc[j], qq[2], x[u].z); acc1<M>(acc[j], qq[3], x[u].w);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < QB; j++) part[((size_t)j * kSplitWaves + wave) * 64 + lane] = (double)acc[j];
        __syncthreads();
        if (consumer) {
            const double* pb = part + (size_t)wave * kSplitWaves * 64;
            double sum = pb[lane];
#pragma unroll
            for (int w = 1; w < kSplitWaves; w++) sum = sum + pb[w * 64 + lane];
            double b;
            if constexpr (M == QV_COSINE || M == QV_DOT) b = k_u * qn_s * rn; else b = k_u * sum;
            if constexpr (M == QV_COSINE) b = b + (__builtin_fabs(sum) + b) * (2.0 * k_u);
            const float d_lo = finalize<M>((A)(sum - b), qc, rn), d_hi = finalize<M>((A)(sum + b), qc, rn);
            float dist = d_lo;
            const bool live = (am >> lane) & 1ull;
            const bool ok = __float_as_uint(d_lo) == __float_as_uint(d_hi) && d_lo == d_lo;
            if (__ballot(live && !ok)) {                                             // the reference's own chain for this tile and query
                A qn2 = 0; A ex;
                if (!have_exact) { ex = row_accumulate<M, 16, true, true, false>(tiles + (size_t)t * v.dim4 * 64 + lane, 64, my_q, v.dim4, &qn2); qc_exact = qconst_from_norm2<M>(qn2); have_exact = true; }
                else ex = row_accumulate<M, 16, false, true, false>(tiles + (size_t)t * v.dim4 * 64 + lane, 64, my_q, v.dim4);
                const float de = finalize<M>(ex, qc_exact, rn);
                if (!ok) dist = de;
            }
            const uint64_t key = live ? make_key(dist, row) : kDeadKey;
            if (first) { list = wave_sort64(key, lane); thr = readlane64(list, kth); first = false; }
            else list_insert(list, thr, key, kth, lane);
        }
        __syncthreads();                                                             // the partial sums are read before the next tile's are written
    }
    if (consumer && lane < k) partial[((size_t)(q0 + wave) * gridDim.x + blockIdx.x) * k + lane] = list;
}


// ---------------------------------------------------------------- queries a filter handed back, redone WITHOUT the host --
// The matrix-core filter hands a query back when its candidate buffer overflows (flags[q] != 0: a loose sample bound, e.g. a corpus
// stored cluster by cluster); such a query needs the exact scan.  Until round 5 the callers read the flags on the host — one round trip
// per batch (and per shard: qv_sharded_search_device was synchronous for 9+ queries because of it).  Here: k_redo_compact lists the
// flagged queries and zeroes their tickets; k_flat_scan_redo — a FIXED launch of grid workgroups, each of which leaves at once when the
// list is empty — walks the listed queries one after another: per query the flat scan's own loop over the workgroup's tiles, the
// lists published with returning atomic exchanges, a ticket, and the LAST workgroup merges and writes the query's k results in place
// of what the filter left there (k_flat_scan<., ., true>'s protocol, once per listed query).  A launch serves kRedoSlots list entries
// from `first` on (its lists live in [slot][grid][k] of the workspace); the launcher issues ceil(nq / kRedoSlots) of them, all but the
// needed ones empty: nothing is decided on the host.
constexpr uint32_t kRedoSlots = 64;
__global__ void k_redo_compact(const uint32_t* __restrict__ flags, uint32_t nq, uint32_t* __restrict__ list, uint32_t* __restrict__ count /* [0] count, [1 ..] tickets [nq] */) {
    // one workgroup, in query order (a wave at a time: ballot + prefix popcount)
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nq; base += blockDim.x) {
        const uint32_t q = base + threadIdx.x;
        const bool f = q < nq && flags[q] != 0;
        const uint64_t m = __ballot(f);
        const uint32_t lane = lane_id();
        __shared__ uint32_t w_off[16];
        const uint32_t wave = threadIdx.x >> 6;
        if (lane == 0) w_off[wave] = (uint32_t)__builtin_popcountll(m);
        __syncthreads();
        uint32_t before = s_n;
        for (uint32_t w = 0; w < wave; w++) before += w_off[w];
        if (f) list[before + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = q;
        if (q < nq) count[1 + q] = 0;                                  // tickets
        __syncthreads();
        if (threadIdx.x == 0) { uint32_t t = 0; for (uint32_t w = 0; w < (blockDim.x >> 6); w++) t += w_off[w]; s_n += t; }
        __syncthreads();
    }
    if (threadIdx.x == 0) count[0] = s_n;
}

// SETS (the queries a bound pass under filters handed back, k_flat_scan_redo<., ., true>): listed query qi is rescanned over alive & set_qi, the
// pass's table of at most kBoundSets entries indexed by qi (uniform: the pair is a scalar load from the kernel arguments), and a tile that
// holds none of its candidates is not requested — a set of fewer than k live rows has no threshold and is ALWAYS handed back, so the empty
// set and the "12 matching rows" set would otherwise each cost a pass over the corpus.  first_tile is the first tile the wave READS.
constexpr uint32_t kBoundSets = 8;
struct BoundSetTable { RowSetRef e[kBoundSets]; };
struct NoSets {};                                                      // the last kernel argument of the forms without sets
template <bool SETS> using SetsArg = typename std::conditional<SETS, BoundSetTable, NoSets>::type;
template <int M, int U, bool SETS = false>
__global__ void __launch_bounds__(kScanBlock)
k_flat_scan_redo(IndexView v, const float* __restrict__ queries, uint32_t k, uint32_t k_stride, const uint32_t* __restrict__ list, const uint32_t* __restrict__ count,
                 uint32_t first, uint64_t* __restrict__ partial /* [kRedoSlots][grid][k] */, uint32_t* __restrict__ tickets /* [nq] by list position */,
                 uint32_t* __restrict__ rows_out, float* __restrict__ dist_out, SetsArg<SETS> tab) {
    using Q = typename MT<M>::Q;
    const uint32_t n = count[0];
    if (first >= n) return;                                           // (the usual case: nothing was handed back)
    extern __shared__ __align__(16) unsigned char smem[];
    Q* q_lds = reinterpret_cast<Q*>(smem);
    uint64_t* wl = reinterpret_cast<uint64_t*>(smem + (((size_t)v.dim4 * 4 * sizeof(Q)) + 15) / 16 * 16);  // [kScanWaves][64]
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t tw = gridDim.x * kScanWaves, kth = k - 1;
    const f4* tiles = reinterpret_cast<const f4*>(v.tiles);
    const uint32_t last_j = n < first + kRedoSlots ? n : first + kRedoSlots;
    for (uint32_t j = first; j < last_j; j++) {
        const uint32_t qi = list[j];
        __syncthreads();                                               // (q_lds and wl are reused from the previous entry)
        stage_query<M>(q_lds, queries + (size_t)qi * v.dim, v.dim, v.dim4);
        __syncthreads();
        uint64_t lst = kDeadKey, thr = kDeadKey;
        QConst qc; qc.qn = 0.0; qc.qn32 = 0.0f;
        bool first_tile = true;
        RowSetRef rs = RowSetRef{nullptr, 0, 0};
        if constexpr (SETS) rs = tab.e[qi & (kBoundSets - 1)];
        for (uint32_t t = blockIdx.x * kScanWaves + wave; t < v.n_tiles; t += tw) {
            uint64_t am;                                               // wave-uniform
            if constexpr (SETS) {
                am = rowset_word(v.alive, rs, true, t);
                if (am == 0ull) continue;
            }
            typename MT<M>::A qn2 = 0, acc;
            if (first_tile) { acc = row_accumulate<M, U, true>(tiles + (size_t)t * v.dim4 * 64 + lane, 64, q_lds, v.dim4, &qn2); qc = qconst_from_norm2<M>(qn2); }
            else acc = row_accumulate<M, U, false>(tiles + (size_t)t * v.dim4 * 64 + lane, 64, q_lds, v.dim4);
            const uint32_t row = t * 64 + lane;
            double rn = 0.0;
            if constexpr (MT<M>::needs_rnorm) rn = v.rnorm[row];
            const float dist = finalize<M>(acc, qc, rn);
            if constexpr (!SETS) am = v.alive[t];
            const uint64_t key = ((am >> lane) & 1ull) ? make_key(dist, row) : kDeadKey;
            if (first_tile) { lst = wave_sort64(key, lane); thr = readlane64(lst, kth); first_tile = false; }
            else list_insert(lst, thr, key, kth, lane);
        }
        wl[wave * 64 + lane] = lst;
        __syncthreads();
        uint64_t* slot = partial + (size_t)(j - first) * gridDim.x * k;
        if (wave == 0) {
            for (uint32_t w = 1; w < kScanWaves; w++) list_insert(lst, thr, lane < k ? wl[w * 64 + lane] : kDeadKey, kth, lane);
            uint64_t* mine = slot + (size_t)blockIdx.x * k;
            if (lane < k) (void)atomicExch(reinterpret_cast<unsigned long long*>(&mine[lane]), (unsigned long long)lst);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // every lane's exchange has returned: the list is at the memory side
            uint32_t last = 0;
            if (lane == 0) last = atomicAdd(&tickets[j], 1u) == gridDim.x - 1 ? 1u : 0u;
            last = __builtin_amdgcn_readfirstlane(last);
            if (lane == 0) wl[0] = last;
        }
        __syncthreads();
        if ((uint32_t)wl[0]) {
            __syncthreads();
            merge_lists_last_workgroup(slot, gridDim.x, k, rows_out + (size_t)qi * k_stride, dist_out + (size_t)qi * k_stride);
        }
    }
}

__device__ __forceinline__ uint64_t wave_min64(uint64_t x) {
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        uint32_t lo = __shfl_xor((uint32_t)x, off), hi = __shfl_xor((uint32_t)(x >> 32), off);
        uint64_t y = ((uint64_t)hi << 32) | lo;
        x = y < x ? y : x;
    }
    return x;
}

// ---------------------------------------------------------------- small collections: scan + merge in ONE launch --
// configs[0] of BASELINE.json is 10k x 128: 5 MB of rows, a scan of a few microseconds — what a query costs there is launches and
// the wait for the stream (31 us per query in round 3: scan launch + merge launch + hipStreamSynchronize; the reference's own
// ExactIndex.Search bench at 1000 x 64 is 38 us on a laptop core, final_bench.txt:28).  Up to kSmallTiles tiles the scan's
// workgroups hand their lists to the LAST one to finish (a ticket), which merges them and writes the final rows / distances
// itself — and, for the host-pointer entry point, a sequence number into pinned memory that the host polls instead of waiting
// for the stream.  Same arithmetic and (distance, row) order as k_flat_scan + k_merge_lists.
// Nothing crosses workgroups through a fence (an agent-scope fence writes the XCD's L2 back, qv_select.h): the lists are published
// with returning atomic exchanges (returned = performed at the memory side), then the ticket; the last workgroup reads them with
// agent-scope atomic loads.  grid (workgroups, nq); partial [nq][grid][k]; tickets [nq], zero before the first launch and left zero.
constexpr uint32_t kSmallTiles = 256;                  // 16k rows: 64 workgroups of one tile per wave (at 30k rows the two-launch path measured faster: 25.7 against 32.6 us)
constexpr uint32_t kSmallPerThread = 64 * 16 / kScanBlock;    // keys a thread of the last workgroup holds: 64 lists of up to 16 keys over 256 threads
constexpr uint32_t kSmallSurv = 512;                   // survivors of the bound ranked by counting (more: one wave inserts the lists)
template <int M, int U>
__global__ void __launch_bounds__(kScanBlock)
k_flat_scan_small(IndexView v, const float* __restrict__ queries, uint32_t k, uint64_t* __restrict__ partial, uint32_t* __restrict__ tickets,
                  uint32_t* __restrict__ rows_out, float* __restrict__ dist_out, uint32_t* done_flag, uint32_t done_seq) {
    using Q = typename MT<M>::Q;
    extern __shared__ __align__(16) unsigned char smem[];
    Q* q_lds = reinterpret_cast<Q*>(smem);
    uint64_t* wl = reinterpret_cast<uint64_t*>(smem + (((size_t)v.dim4 * 4 * sizeof(Q)) + 15) / 16 * 16);  // [kScanWaves][64]
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t qi = blockIdx.y;
    stage_query<M>(q_lds, queries + (size_t)qi * v.dim, v.dim, v.dim4);
    __syncthreads();
    const uint32_t tw = gridDim.x * kScanWaves;
    const uint32_t kth = k - 1;
    uint64_t list = kDeadKey, thr = kDeadKey;
    const f4* tiles = reinterpret_cast<const f4*>(v.tiles);
    QConst qc; qc.qn = 0.0; qc.qn32 = 0.0f;
    bool first = true;
    for (uint32_t t = blockIdx.x * kScanWaves + wave; t < v.n_tiles; t += tw) {
        typename MT<M>::A qn2 = 0, acc;
        // the row's norm and the tile's live word first, then all of a 128-dimension row's chunks in ONE round of requests (U = 32,
        // pinned), temporal: a collection this small stays in its XCD's L2 from call to call (the same workgroup, hence the same XCD,
        // reads the same tiles every time) — what a query costs here is round trips, not bytes
        const uint32_t row = t * 64 + lane;
        double rn = 0.0;
        if constexpr (MT<M>::needs_rnorm) rn = v.rnorm[row];
        const uint64_t am = v.alive[t];
        if (first) { acc = row_accumulate<M, U, true, true, false>(tiles + (size_t)t * v.dim4 * 64 + lane, 64, q_lds, v.dim4, &qn2); qc = qconst_from_norm2<M>(qn2); }
        else acc = row_accumulate<M, U, false, true, false>(tiles + (size_t)t * v.dim4 * 64 + lane, 64, q_lds, v.dim4);
        const float dist = finalize<M>(acc, qc, rn);
        const uint64_t key = ((am >> lane) & 1ull) ? make_key(dist, row) : kDeadKey;
        if (first) { list = wave_sort64(key, lane); thr = readlane64(list, kth); first = false; }
        else list_insert(list, thr, key, kth, lane);
    }
    wl[wave * 64 + lane] = list;
    __syncthreads();
    __shared__ uint32_t s_last, s_ns;
    __shared__ unsigned long long s_bound;
    __shared__ uint64_t surv[kSmallSurv];
    uint64_t* mine = partial + ((size_t)qi * gridDim.x + blockIdx.x) * k;
    if (wave == 0) {
        for (uint32_t w = 1; w < kScanWaves; w++) list_insert(list, thr, lane < k ? wl[w * 64 + lane] : kDeadKey, kth, lane);
        uint32_t last = 1;
        if (gridDim.x > 1) {
            if (lane < k) (void)atomicExch(reinterpret_cast<unsigned long long*>(&mine[lane]), (unsigned long long)list);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // every lane's exchange has returned: the list is at the memory side
            if (lane == 0) last = atomicAdd(&tickets[qi], 1u) == gridDim.x - 1 ? 1u : 0u;
            last = __builtin_amdgcn_readfirstlane(last);
            if (last && lane == 0) tickets[qi] = 0;                    // for the next launch on this workspace (stream order)
        }
        if (lane == 0) { s_last = last; s_ns = 0; s_bound = kDeadKey; }
    }
    __syncthreads();
    if (!s_last) return;
    if (gridDim.x > 1) {
        // The last workgroup merges, all four waves: (1) B = the smallest k-th key of any list — that list alone holds k keys <= B, so
        // nothing above B is in the answer; (2) the keys <= B (a few dozen of grid * k) go to LDS; (3) every survivor counts the
        // survivors below it: that count is its place.  (One wave inserting 400 keys one by one was 8 of the kernel's 20 us.)
        const uint64_t* all = partial + (size_t)qi * gridDim.x * k;
        const uint32_t total = gridDim.x * k;
        uint64_t b = kDeadKey;
        for (uint32_t w = threadIdx.x; w < gridDim.x; w += kScanBlock) { const uint64_t x = __hip_atomic_load(&all[(size_t)w * k + kth], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); b = x < b ? x : b; }
        uint64_t keys[kSmallPerThread];
#pragma unroll
        for (uint32_t u = 0; u < kSmallPerThread; u++) {
            const uint32_t i = threadIdx.x + u * kScanBlock;
            keys[u] = i < total ? __hip_atomic_load(&all[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : kDeadKey;
        }
        b = wave_min64(b);
        if (lane == 0 && b != kDeadKey) atomicMin(&s_bound, (unsigned long long)b);
        __syncthreads();
        const uint64_t bound = s_bound;
#pragma unroll
        for (uint32_t u = 0; u < kSmallPerThread; u++)
            if (keys[u] != kDeadKey && keys[u] <= bound) { const uint32_t pos = atomicAdd(&s_ns, 1u); if (pos < kSmallSurv) surv[pos] = keys[u]; }
        __syncthreads();
        const uint32_t ns = s_ns < kSmallSurv ? s_ns : kSmallSurv;     // (more than kSmallSurv keys <= B needs > 32 lists with k-th keys tied at B: the first kSmallSurv still hold the answer's
                                                                      //  keys only if none is lost — so that case takes the serial path below)
        if (s_ns <= kSmallSurv) {
            list = kDeadKey;
            for (uint32_t i = threadIdx.x; i < ns; i += kScanBlock) {
                const uint64_t me = surv[i];
                uint32_t rank = 0;
                for (uint32_t j = 0; j < ns; j++) rank += surv[j] < me ? 1u : 0u;
                if (rank < k) wl[rank] = me;                           // keys are distinct: ranks are too
            }
            __syncthreads();
            if (wave != 0) return;
            list = lane < (ns < k ? ns : k) ? wl[lane] : kDeadKey;
        } else {
            if (wave != 0) return;
            for (uint32_t base = 0; base < total; base += 64) {
                const uint32_t i = base + lane;
                uint64_t key = kDeadKey;
                if (i < total && i / k != blockIdx.x) key = __hip_atomic_load(&all[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                list_insert(list, thr, key, kth, lane);
            }
        }
    } else if (wave != 0) return;
    const bool dead = list == kDeadKey;
    const uint32_t r_out = dead ? 0xFFFFFFFFu : (uint32_t)list;
    const float d_out = dead ? __uint_as_float(0x7F800000u) : unord_f32((uint32_t)(list >> 32));
    if (!done_flag) {
        if (lane < k) { rows_out[(size_t)qi * k + lane] = r_out; dist_out[(size_t)qi * k + lane] = d_out; }
    } else {
        // The host polls a sequence number instead of waiting for the stream (nq == 1 for this use).  The results go out as
        // SYSTEM-scope stores (write-through whatever the page's cache policy: plain stores sat in L2 until the kernel ended and
        // the host read the previous call's rows); once they are acknowledged the sequence number follows on the same path.
        if (lane < k) {
            __hip_atomic_store(&rows_out[(size_t)qi * k + lane], r_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&dist_out[(size_t)qi * k + lane], d_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(done_flag, done_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---------------------------------------------------------------- flat scan, 64 < k <= 128 --
// The negative-example branches of the reference fetch max(2k, 30) results (hybrid_index.go:516-522, hnsw/adapter.go:353-359):
// k = 50 is a 100-key search.  Same stream, same arithmetic as k_flat_scan; the wave's list holds R keys per lane
// (wide_insert), and every WAVE writes its 64 R slots — a workgroup merge through one wave's serial inserts would cost more
// than the scan of a short corpus.  (Four keys per lane, k <= 256, measured SLOWER than a key per row + selection: 5.05 against 4.80 ms
// at 10M x 768 — ~1000 inserts per wave, each a serial ~100-instruction sequence on a wave that has one partner on its SIMD.)
// The radix selection (qv_select.hip) then takes the k best of the waves' lists: all keys a
// wave saw beyond its 64 R best are beaten by 64 R >= k others, so the lists hold the answer.
// Output: lists[((q * gridDim.x + blockIdx.x) * kScanWaves + wave) * 64 R + r * 64 + lane].
template <int M, int U, int R>
__global__ void __launch_bounds__(kScanBlock)
k_flat_scan_wide(IndexView v, const float* __restrict__ queries, uint32_t k, uint64_t* __restrict__ lists) {
    using Q = typename MT<M>::Q;
    extern __shared__ __align__(16) unsigned char smem[];
    Q* q_lds = reinterpret_cast<Q*>(smem);
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t qi = blockIdx.y;
    stage_query<M>(q_lds, queries + (size_t)qi * v.dim, v.dim, v.dim4);
    __syncthreads();

    const uint32_t tw = gridDim.x * kScanWaves;
    const uint32_t kth = k - 1;
    uint64_t list[R], thr = kDeadKey;
#pragma unroll
    for (int r = 0; r < R; r++) list[r] = kDeadKey;
    const f4* tiles = reinterpret_cast<const f4*>(v.tiles);
    QConst qc; qc.qn = 0.0; qc.qn32 = 0.0f;

    auto finish_tile = [&](uint32_t t, typename MT<M>::A acc, bool first) {
        const uint32_t row = t * 64 + lane;
        double rn = 0.0;
        if constexpr (MT<M>::needs_rnorm) rn = v.rnorm[row];
        float dist = finalize<M>(acc, qc, rn);
        uint64_t am = v.alive[t];                                     // wave-uniform
        uint64_t key = ((am >> lane) & 1ull) ? make_key(dist, row) : kDeadKey;
        if (first) list[0] = wave_sort64(key, lane);                  // empty list: sort the tile outright (k > 64: the threshold stays open)
        else wide_insert<R>(list, thr, key, kth, lane);
    };

    uint32_t t = blockIdx.x * kScanWaves + wave;
    if (t < v.n_tiles) {                                              // first tile: query norm rides along
        typename MT<M>::A qn2 = 0;
        typename MT<M>::A acc = row_accumulate<M, U, true>(tiles + (size_t)t * v.dim4 * 64 + lane, 64, q_lds, v.dim4, &qn2);
        qc = qconst_from_norm2<M>(qn2);
        finish_tile(t, acc, true);
        t += tw;
    }
    for (; t < v.n_tiles; t += tw) {
        typename MT<M>::A acc = row_accumulate<M, U, false>(tiles + (size_t)t * v.dim4 * 64 + lane, 64, q_lds, v.dim4);
        finish_tile(t, acc, false);
    }
    uint64_t* out = lists + (((size_t)qi * gridDim.x + blockIdx.x) * kScanWaves + wave) * (64 * R);
#pragma unroll
    for (int r = 0; r < R; r++) out[r * 64 + lane] = list[r];
}

// ---------------------------------------------------------------- multi-query scan --
// QB queries share ONE pass over the corpus (HybridIndex.BatchSearch, hybrid_index.go:677-811,
// is Q independent exact searches; here every 16-byte row chunk a lane loads is used for QB
// dot products).  Same arithmetic contract: lane == row, each (row, query) distance is one
// sequential chain over dims 0..D-1.  The query block sits in LDS interleaved by query
// (q_lds[dim][QB]) so one ds_read_b128 feeds two (f64) or four (f32) queries of one dim.
// grid = (workgroups, ceil(nq/QB)); partial layout identical to k_flat_scan.
// (mq_tile — one tile for QB queries — lives in qv_kernels.h: the traversal's hub table uses it too)
// query blocks for the scalar-operand variant: qblk[group][dim4*4][QB] in the metric's Q type
template <int M, int QB>
__global__ void k_prep_qblk(const float* __restrict__ queries, uint32_t nq, uint32_t dim, uint32_t dim4, typename MT<M>::Q* __restrict__ qblk) {
    using Q = typename MT<M>::Q;
    const uint32_t per = dim4 * 4 * QB;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per) return;
    const uint32_t d = i / QB, qq = i % QB, q0 = blockIdx.y * QB;
    const uint32_t qi = q0 + qq < nq ? q0 + qq : nq - 1;
    qblk[(size_t)blockIdx.y * per + i] = d < dim ? (Q)queries[(size_t)qi * dim + d] : (Q)0;
}

// SQ = true: the query block is read from GLOBAL memory at wave-uniform addresses, which the
// compiler turns into scalar loads (s_load) and SGPR operands of v_fma_f64 — the LDS, which
// bounds the LDS-staged form (one broadcast ds_read_b128 per 2 query values), is not touched.
template <int M, int U, int QB, bool SQ>
__global__ void __launch_bounds__(kScanBlock, 2)
k_flat_scan_mq(IndexView v, const float* __restrict__ queries, const typename MT<M>::Q* __restrict__ qblk, uint32_t nq, uint32_t k,
               uint64_t* __restrict__ partial) {
    using Q = typename MT<M>::Q;
    using A = typename MT<M>::A;
    extern __shared__ __align__(16) unsigned char smem[];
    const size_t q_bytes = SQ ? 0 : (((size_t)v.dim4 * 4 * QB * sizeof(Q)) + 15) / 16 * 16;
    uint64_t* wl = reinterpret_cast<uint64_t*>(smem + q_bytes);                  // [waves][QB][64]
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t q0 = blockIdx.y * QB;
    const Q* q_lds;
    if constexpr (SQ) {
        q_lds = qblk + (size_t)blockIdx.y * v.dim4 * 4 * QB;                     // global, uniform -> scalar loads
    } else {
        Q* ql = reinterpret_cast<Q*>(smem);                                      // [dim4*4][QB]
        // stage QB queries, zero-padded in dim; query slots past nq replicate the last query (results dropped)
        for (uint32_t i = threadIdx.x; i < v.dim4 * 4 * QB; i += blockDim.x) {
            uint32_t d = i / QB, qq = i % QB;
            uint32_t qi = q0 + qq < nq ? q0 + qq : nq - 1;
            ql[i] = d < v.dim ? (Q)queries[(size_t)qi * v.dim + d] : (Q)0;
        }
        __syncthreads();
        q_lds = ql;
    }

    const uint32_t tw = gridDim.x * kScanWaves;
    const uint32_t kth = k - 1;
    uint64_t list[QB], thr[QB];
    QConst qc[QB];
#pragma unroll
    for (int j = 0; j < QB; j++) { list[j] = kDeadKey; thr[j] = kDeadKey; qc[j].qn = 0.0; qc[j].qn32 = 0.0f; }
    const f4* tiles = reinterpret_cast<const f4*>(v.tiles);

    uint32_t t = blockIdx.x * kScanWaves + wave;
    if (t < v.n_tiles) {                                                         // first tile: sort outright, query norms ride along
        A acc[QB], qa[QB];
        mq_tile<M, U, QB, true>(tiles + (size_t)t * v.dim4 * 64 + lane, q_lds, v.dim4, acc, qa);
        const uint32_t row = t * 64 + lane;
        double rn = 0.0;
        if constexpr (MT<M>::needs_rnorm) rn = v.rnorm[row];
        const bool live = (v.alive[t] >> lane) & 1ull;
#pragma unroll
        for (int j = 0; j < QB; j++) {
            qc[j] = qconst_from_norm2<M>(qa[j]);
            float dist = finalize<M>(acc[j], qc[j], rn);
            list[j] = wave_sort64(live ? make_key(dist, row) : kDeadKey, lane);
            thr[j] = readlane64(list[j], kth);
        }
        t += tw;
    }
    for (; t < v.n_tiles; t += tw) {
        A acc[QB], qa[QB];
        mq_tile<M, U, QB, false>(tiles + (size_t)t * v.dim4 * 64 + lane, q_lds, v.dim4, acc, qa);
        const uint32_t row = t * 64 + lane;
        double rn = 0.0;
        if constexpr (MT<M>::needs_rnorm) rn = v.rnorm[row];
        const bool live = (v.alive[t] >> lane) & 1ull;
#pragma unroll
        for (int j = 0; j < QB; j++) {
            float dist = finalize<M>(acc[j], qc[j], rn);
            list_insert(list[j], thr[j], live ? make_key(dist, row) : kDeadKey, kth, lane);
        }
    }

#pragma unroll
    for (int j = 0; j < QB; j++) wl[((size_t)wave * QB + j) * 64 + lane] = list[j];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int j = 0; j < QB; j++) {
            for (uint32_t w = 1; w < kScanWaves; w++) {
                uint64_t key = lane < k ? wl[((size_t)w * QB + j) * 64 + lane] : kDeadKey;
                list_insert(list[j], thr[j], key, kth, lane);
            }
            if (q0 + j < nq && lane < k) partial[((size_t)(q0 + j) * gridDim.x + blockIdx.x) * k + lane] = list[j];
        }
    }
}

// The multi-query scan writing ONE KEY PER ROW AND QUERY instead of keeping lists: the front end of the radix selection
// (qv_select.hip) for batches that ask for more than 64 results per query and do not go through the matrix-core filter (2 - 8
// queries, or a metric the filter does not take).  QB queries share a corpus pass, their values arrive as scalar operands
// (k_flat_scan_mq's SQ form); keys_all [nq][n_tiles * 64].  grid = (workgroups, ceil(nq / QB)).
template <int M, int U, int QB>
__global__ void __launch_bounds__(kScanBlock, 2)
k_flat_keys_mq(IndexView v, const typename MT<M>::Q* __restrict__ qblk, uint32_t nq, uint64_t* __restrict__ keys_all,
               const uint32_t* __restrict__ active /* null, or a device word: query groups from *active on leave at once (launch_flat_select_redo) */) {
    using Q = typename MT<M>::Q;
    using A = typename MT<M>::A;
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t q0 = blockIdx.y * QB;
    if (active != nullptr && q0 >= *active) return;
    const Q* q_lds = qblk + (size_t)blockIdx.y * v.dim4 * 4 * QB;                // global, uniform -> scalar loads
    const uint32_t tw = gridDim.x * kScanWaves;
    const size_t n = (size_t)v.n_tiles * 64;
    QConst qc[QB];
#pragma unroll
    for (int j = 0; j < QB; j++) { qc[j].qn = 0.0; qc[j].qn32 = 0.0f; }
    const f4* tiles = reinterpret_cast<const f4*>(v.tiles);
    bool first = true;
    for (uint32_t t = blockIdx.x * kScanWaves + wave; t < v.n_tiles; t += tw) {
        A acc[QB], qa[QB];
        if (first) {
            mq_tile<M, U, QB, true>(tiles + (size_t)t * v.dim4 * 64 + lane, q_lds, v.dim4, acc, qa);
#pragma unroll
            for (int j = 0; j < QB; j++) qc[j] = qconst_from_norm2<M>(qa[j]);
            first = false;
        } else mq_tile<M, U, QB, false>(tiles + (size_t)t * v.dim4 * 64 + lane, q_lds, v.dim4, acc, qa);
        const uint32_t row = t * 64 + lane;
        double rn = 0.0;
        if constexpr (MT<M>::needs_rnorm) rn = v.rnorm[row];
        const bool live = (v.alive[t] >> lane) & 1ull;
#pragma unroll
        for (int j = 0; j < QB; j++) {
            const uint64_t key = live ? make_key(finalize<M>(acc[j], qc[j], rn), row) : kDeadKey;
            if (q0 + j < nq) __builtin_nontemporal_store(key, &keys_all[(size_t)(q0 + j) * n + row]);
        }
    }
}

size_t flat_keys_mq_workspace_bytes(uint32_t nq, uint32_t dim4) { return ((size_t)(nq + 8) * dim4 * 4 * sizeof(double) + 255) / 256 * 256; }
// keys of nq >= 2 queries in shared corpus passes; d_qws: flat_keys_mq_workspace_bytes
hipError_t launch_flat_keys_mq(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint64_t* d_keys, void* d_qws, hipStream_t s, const uint32_t* d_active) {
    const uint32_t want = (v.n_tiles + kScanWaves - 1) / kScanWaves;
    const uint32_t grid = std::max(1u, std::min(want, p.grid));
#define QV_KMQ(MMM, QQ)                                                                                                   \
    {                                                                                                                     \
        using QT = typename MT<MMM>::Q;                                                                                   \
        const uint32_t groups = (nq + QQ - 1) / QQ;                                                                       \
        const uint32_t per = v.dim4 * 4 * QQ;                                                                             \
        hipLaunchKernelGGL((k_prep_qblk<MMM, QQ>), dim3((per + 255) / 256, groups), dim3(256), 0, s, d_queries, nq, v.dim, v.dim4, static_cast<QT*>(d_qws)); \
        hipLaunchKernelGGL((k_flat_keys_mq<MMM, 4, QQ>), dim3(grid, groups), dim3(p.block), 0, s, v, static_cast<const QT*>(d_qws), nq, d_keys, d_active); \
    }
    if (nq >= 5) { QV_DISPATCH_METRIC(v.metric, { QV_KMQ(MM, 8) }); }
    else { QV_DISPATCH_METRIC(v.metric, { QV_KMQ(MM, 4) }); }
#undef QV_KMQ
    return hipGetLastError();
}

// One workgroup per query merges n_lists sorted lists of k keys into the final top-k.
// Bound trick: the smallest k-th entry over all lists, B, is an upper bound of the final
// k-th key (that list alone holds k keys <= B), so only keys <= B can be in the answer.
// Typically a few dozen of the n_lists*k keys survive; one wave insertion-sorts them.
constexpr int kMergeBlock = 1024;
constexpr int kMergeCap = 2048;                       // survivors kept in LDS; more -> general path
constexpr int kMergeHeads = 128;                      // sampled list heads ranked in LDS


// The merge itself, for one query: src = its n_lists lists of k keys, rows_out / dist_out = its k results.  AT: the lists were
// published by other workgroups of the SAME launch (returning atomic exchanges, then a ticket: k_flat_scan<., ., true>) and are read
// with agent-scope atomic loads; otherwise by an earlier launch, and plain loads do.
template <bool AT>
__device__ void merge_lists_body(const uint64_t* __restrict__ src, uint32_t n_lists, uint32_t k, uint32_t* __restrict__ rows_out, float* __restrict__ dist_out,
                                 uint32_t* done_flag = nullptr, uint32_t done_seq = 0) {
    auto ld = [](const uint64_t* p) -> uint64_t {
        if constexpr (AT) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else return *p;
    };

    __shared__ uint64_t wl[kMergeBlock / 64][64];
    __shared__ uint64_t surv[kMergeCap];
    __shared__ uint32_t hd[kMergeHeads], hlt[kMergeHeads], hle[kMergeHeads];
    __shared__ uint64_t s_bound, s_b1;
    __shared__ uint32_t s_nsurv;
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t total = n_lists * k;
    const uint32_t kth = k - 1;

    // every global load of the common case is issued up front (one HBM/L2 latency, not three):
    // this thread's <= 8 keys, one list's k-th key, one sampled list head
    const bool small = total <= blockDim.x * 8;
    uint64_t mine[8];
#pragma unroll
    for (int u = 0; u < 8; u++) { uint32_t i = u * blockDim.x + threadIdx.x; mine[u] = (small && i < total) ? ld(src + i) : kDeadKey; }
    // sampled heads: m = min(n_lists, kMergeHeads) lists at a fixed stride.  Any k different
    // lists each hold a key <= the k-th smallest of their heads, so a subset still gives a
    // valid (slightly looser) bound, and the O(m^2) rank count stays ~0.5 us on one CU.
    const uint32_t m = n_lists < (uint32_t)kMergeHeads ? n_lists : (uint32_t)kMergeHeads;
    const uint32_t hstride = n_lists / m;
    const bool use_heads = m >= k;
    uint64_t b = kDeadKey;
    for (uint32_t w = threadIdx.x; w < n_lists; w += blockDim.x) { uint64_t x = ld(src + (size_t)w * k + kth); b = x < b ? x : b; }
    if (use_heads)
        for (uint32_t w = threadIdx.x; w < m; w += blockDim.x) { hd[w] = (uint32_t)(ld(src + (size_t)w * hstride * k) >> 32); hlt[w] = 0; hle[w] = 0; }

    // phase A: two upper bounds of the final k-th key.
    //   B0 = min over lists of their k-th key (that list alone has k keys <= B0);
    //   B1 = from the k-th smallest sampled HEAD — the tight one when the winners are spread
    //        over many lists, which is the common case.  Rank counting on the 32 distance bits:
    //        head i qualifies when #{j: d_j < d_i} <= k-1 < #{j: d_j <= d_i}; then every key
    //        with distance <= d_i is kept.
    b = wave_min64(b);
    if (lane == 0) wl[wave][0] = b;
    if (threadIdx.x == 0) { s_nsurv = 0; s_b1 = kDeadKey; }
    __syncthreads();
    if (use_heads) {
        const uint32_t segs = blockDim.x >= m ? blockDim.x / m : 1;   // thread -> (head i, segment of j)
        const uint32_t per = (m + segs - 1) / segs;
        for (uint32_t i = threadIdx.x % m, sgm = blockDim.x >= m ? threadIdx.x / m : 0; sgm < segs && i < m; i += blockDim.x) {
            const uint32_t h = hd[i];
            uint32_t clt = 0, cle = 0;
            const uint32_t j0 = sgm * per, j1 = min(j0 + per, m);
            uint32_t j = j0;
            for (; j + 16 <= j1; j += 16) {                           // batch the (broadcast) LDS reads
                uint32_t x[16];
#pragma unroll
                for (int u = 0; u < 16; u++) x[u] = hd[j + u];
#pragma unroll
                for (int u = 0; u < 16; u++) { clt += x[u] < h ? 1u : 0u; cle += x[u] <= h ? 1u : 0u; }
            }
            for (; j < j1; j++) { uint32_t x = hd[j]; clt += x < h ? 1u : 0u; cle += x <= h ? 1u : 0u; }
            if (clt) atomicAdd(&hlt[i], clt);
            if (cle) atomicAdd(&hle[i], cle);
            if (blockDim.x >= m) break;
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < m; i += blockDim.x)
            if (hlt[i] <= kth && kth < hle[i] && hd[i] != 0xFFFFFFFFu) s_b1 = ((uint64_t)hd[i] << 32) | 0xFFFFFFFFull;
    }
    if (wave == 0) {
        uint64_t x = lane < nw ? wl[lane][0] : kDeadKey;
        x = wave_min64(x);
        if (lane == 0) s_bound = x;
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_b1 < s_bound) s_bound = s_b1;
    __syncthreads();
    const uint64_t bound = s_bound;
    // phase B: keep keys <= bound
    auto keep = [&](uint64_t key) {
        if (key != kDeadKey && key <= bound) {
            uint32_t pos = atomicAdd(&s_nsurv, 1u);
            if (pos < (uint32_t)kMergeCap) surv[pos] = key;
        }
    };
    if (small) {
#pragma unroll
        for (int u = 0; u < 8; u++) keep(mine[u]);
    } else {
        for (uint32_t base = 0; base < total; base += blockDim.x * 8) {
            uint64_t key[8];
#pragma unroll
            for (int u = 0; u < 8; u++) { uint32_t i = base + u * blockDim.x + threadIdx.x; key[u] = i < total ? ld(src + i) : kDeadKey; }
#pragma unroll
            for (int u = 0; u < 8; u++) keep(key[u]);
        }
    }
    __syncthreads();
    const uint32_t ns = s_nsurv;
    uint64_t list = kDeadKey, thr = kDeadKey;
    if (ns <= 64) {
        // phase C (common): one wave bitonic-sorts the survivors
        if (wave != 0) return;
        list = wave_sort64(lane < ns ? surv[lane] : kDeadKey, lane);
    } else if (ns <= (uint32_t)kMergeCap) {
        if (wave != 0) return;
        list = wave_sort64(surv[lane], lane);
        thr = readlane64(list, kth);
        for (uint32_t base = 64; base < ns; base += 64) {
            uint32_t i = base + lane;
            uint64_t key = i < ns ? surv[i] : kDeadKey;
            list_insert(list, thr, key, kth, lane);
        }
    } else {
        // general path (tiny indexes whose lists are mostly shorter than k): every wave
        // reduces a slice, wave 0 merges the waves
        for (uint32_t base = wave * 64; base < total; base += nw * 64) {
            uint32_t i = base + lane;
            uint64_t key = i < total ? ld(src + i) : kDeadKey;
            list_insert(list, thr, key, kth, lane);
        }
        wl[wave][lane] = list;
        __syncthreads();
        if (wave != 0) return;
        for (uint32_t w = 1; w < nw; w++) {
            uint64_t key = lane < k ? wl[w][lane] : kDeadKey;
            list_insert(list, thr, key, kth, lane);
        }
    }
    const bool dead = list == kDeadKey;
    const uint32_t r_out = dead ? 0xFFFFFFFFu : (uint32_t)list;
    const float d_out = dead ? __uint_as_float(0x7F800000u) : unord_f32((uint32_t)(list >> 32));
    if (!done_flag) {
        if (lane < k) { rows_out[lane] = r_out; dist_out[lane] = d_out; }
    } else {
        // the host polls a sequence number instead of waiting for the stream (k_flat_scan_small's hand-over: system-scope stores for
        // the results, and once they are acknowledged the sequence number on the same path)
        if (lane < k) {
            __hip_atomic_store(&rows_out[lane], r_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&dist_out[lane], d_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(done_flag, done_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}


__global__ void __launch_bounds__(kMergeBlock)
k_merge_lists(const uint64_t* __restrict__ partial, uint32_t n_lists, uint32_t k,
              uint32_t* __restrict__ rows_out, float* __restrict__ dist_out) {
    const uint32_t qi = blockIdx.x;
    merge_lists_body<false>(partial + (size_t)qi * n_lists * k, n_lists, k, rows_out + (size_t)qi * k, dist_out + (size_t)qi * k);
}
// (out of line: the scan's loop keeps its own register allocation and schedule — tests/test_isa_guard.py counts its loads in flight)
__device__ __noinline__ void merge_lists_last_workgroup(const uint64_t* src, uint32_t n_lists, uint32_t k, uint32_t* rows_out, float* dist_out, uint32_t* done_flag, uint32_t done_seq) {
    merge_lists_body<true>(src, n_lists, k, rows_out, dist_out, done_flag, done_seq);
}

// merge of (distance, row) pair lists, e.g. the all-gathered per-shard top-k of a sharded scan
__global__ void __launch_bounds__(kMergeBlock)
k_merge_pairs(const float* __restrict__ dist, const uint32_t* __restrict__ rows, uint32_t total, uint32_t k,
              uint32_t* __restrict__ rows_out, float* __restrict__ dist_out) {
    __shared__ uint64_t wl[kMergeBlock / 64][64];
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t kth = k - 1;
    uint64_t list = kDeadKey, thr = kDeadKey;
    for (uint32_t base = wave * 64; base < total; base += nw * 64) {
        uint32_t i = base + lane;
        uint64_t key = kDeadKey;
        if (i < total && rows[i] != 0xFFFFFFFFu) key = make_key(dist[i], rows[i]);
        list_insert(list, thr, key, kth, lane);
    }
    wl[wave][lane] = list;
    __syncthreads();
    if (wave == 0) {
        for (uint32_t w = 1; w < nw; w++) {
            uint64_t key = lane < k ? wl[w][lane] : kDeadKey;
            list_insert(list, thr, key, kth, lane);
        }
        if (lane < k) {
            bool dead = list == kDeadKey;
            rows_out[lane] = dead ? 0xFFFFFFFFu : (uint32_t)list;
            dist_out[lane] = dead ? __uint_as_float(0x7F800000u) : unord_f32((uint32_t)(list >> 32));
        }
    }
}

// the same merge for the packed exchange buffer of the sharded scan: per shard and query [k local rows][k distance bits], global
// row = shard base + local row (so a shard's scan output goes into the all-gather as it is: one collective, no kernel in
// between).  packed = [n_lists][nq][2][k]; one workgroup per query.
__global__ void __launch_bounds__(kMergeBlock)
k_merge_shards(const uint32_t* __restrict__ packed, const uint32_t* __restrict__ bases, uint32_t n_lists, uint32_t nq, uint32_t k,
               uint32_t* __restrict__ rows_out, float* __restrict__ dist_out, uint32_t planes) {
    __shared__ uint64_t wl[kMergeBlock / 64][64];
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t q = blockIdx.x;
    const uint32_t kth = k - 1, total = n_lists * k;
    uint64_t list = kDeadKey, thr = kDeadKey;
    for (uint32_t base = wave * 64; base < total; base += nw * 64) {
        const uint32_t i = base + lane;
        uint64_t key = kDeadKey;
        if (i < total) {
            const uint32_t g = i / k, j = i - g * k;
            // planes == 0, interleaved: per shard [nq][2][k];  planes >= 2, planar: per shard [planes][nq][k] (rows of all
            // queries, then distances of all queries, then payload planes the merge does not read — a shard's multi-query
            // scan writes both halves in place, no repacking before the all-gather)
            const uint32_t* blk = packed + (planes ? (size_t)g * planes * nq * k + (size_t)q * k : ((size_t)g * nq + q) * 2 * k);
            const uint32_t row = blk[j];
            if (row != 0xFFFFFFFFu) key = make_key(__uint_as_float(blk[(planes ? (size_t)nq * k : k) + j]), bases[g] + row);
        }
        list_insert(list, thr, key, kth, lane);
    }
    wl[wave][lane] = list;
    __syncthreads();
    if (wave == 0) {
        for (uint32_t w = 1; w < nw; w++) {
            uint64_t key = lane < k ? wl[w][lane] : kDeadKey;
            list_insert(list, thr, key, kth, lane);
        }
        if (lane < k) {
            bool dead = list == kDeadKey;
            rows_out[(size_t)q * k + lane] = dead ? 0xFFFFFFFFu : (uint32_t)list;
            dist_out[(size_t)q * k + lane] = dead ? __uint_as_float(0x7F800000u) : unord_f32((uint32_t)(list >> 32));
        }
    }
}


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
//   k_bound_collect  the rows with d_lo <= H (not strict: ties go on) — k plus a handful on ordinary data — listed with one returning
//                    atomic per wave and batch that has any.
//   k_bound_rescore  one workgroup: those rows walked as ONE float64 chain over the float32 tiles — row_accumulate + finalize, the
//                    query's norm as its chain: the exact scan's bits —, the k best (distance, row) keys written where the exact scan
//                    writes them.  When the list overflowed, H is not finite (fewer than k rows with a bound), or |q| is not a norm
//                    the bound works with, it sets the gate word instead and the exact scan launched behind it answers
//                    (k_flat_scan<., ., true>'s `gate`: otherwise that launch leaves at once).  Nothing is read on the host.
// (Measured first and not kept: candidates taken DURING the scan against a device-wide threshold word seeded from the waves' first
// tiles — the tiles walked before the seed's merge lands let 20 - 50 k rows through at k = 64; profiles/LAB_r07_bound_scan.md.)
// The control words live in the stream's zeroed ticket words and are left zero.
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kBoundCandCap = 4096;       // rows stage 3 walks exactly (an i.i.d. 10M x 768 corpus leaves k + a few)
constexpr uint32_t kBoundMaxDim = 4096;
struct BoundCtrl { uint32_t thr_inv, cand_cnt, ticket, flag; };   // thr_inv = ~(ordered image of H): zero = no finite H

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
__device__ __forceinline__ void bound_scan_tail(uint64_t list, uint64_t thr, uint64_t* wl /* LDS [kScanWaves][64] */, uint32_t wave, uint32_t lane, uint32_t k, BoundCtrl* __restrict__ ctrl,
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
    if (!s_last) return;
    merge_lists_last_workgroup(partial, gridDim.x, k, seed_rows, seed_dist);
    if (wave == 0 && lane == kth) {                                    // (this lane wrote them) H: a finite k-th upper bound, or none
        const uint32_t o = ord_f32(seed_dist[kth]);
        ctrl->thr_inv = (seed_rows[kth] != 0xFFFFFFFFu && o < 0xFF800000u) ? ~o : 0u;
        ctrl->cand_cnt = 0;
    }
}

// SKIP (k_bound_scan<., true>: v.alive is a filter's candidate bitmap, alive & set — k_rowset_and's or the masked upload): a tile whose word is
// zero is not requested, neither its copy nor rnorm nor rres.  Its 64 lower-bound words are WRITTEN as 0xFFFFFFFF all the same: k_bound_collect
// reads every word and the workspace is reused, so an unwritten tile would hold an earlier search's bounds; 256 bytes stored against dim * 128
// bytes not read, and the collect stays as it is.  |q|^2 rides along the first tile the wave READS; a wave that reads none publishes a dead list.
template <int M, bool SKIP = false>
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

    bound_scan_tail(list, thr, wl, wave, lane, k, ctrl, partial, seed_rows, seed_dist);
}

// the rows with d_lo <= H, four per thread and step (lo: one query's ordered words; cnt: its counter; cand: its list)
__device__ __forceinline__ void bound_collect(const uint32_t* __restrict__ lo, uint32_t n /* multiple of 64 */, uint32_t H, uint32_t* __restrict__ cnt, uint32_t* __restrict__ cand) {
    const uint32_t lane = lane_id();
    for (uint32_t base = blockIdx.x * 1024u; base < n; base += gridDim.x * 1024u) {
        const uint32_t i = base + threadIdx.x * 4u;
        u4 x = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        if (i < n) x = __builtin_nontemporal_load(reinterpret_cast<const u4*>(lo + i));
        const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool c = xs[j] <= H && xs[j] != 0xFFFFFFFFu;
            const uint64_t m = __ballot(c);
            if (m) {
                uint32_t b0 = 0;
                if (lane == (uint32_t)__builtin_ctzll(m)) b0 = atomicAdd(cnt, (uint32_t)__builtin_popcountll(m));
                b0 = __builtin_amdgcn_readlane(b0, (uint32_t)__builtin_ctzll(m));
                const uint32_t slot = b0 + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
                if (c && slot < kBoundCandCap) cand[slot] = i + (uint32_t)j;
            }
        }
    }
}
__global__ void __launch_bounds__(256)
k_bound_collect(const uint32_t* __restrict__ lo_all, uint32_t n /* multiple of 64 */, BoundCtrl* __restrict__ ctrl, uint32_t* __restrict__ cand,
                const uint32_t* __restrict__ gate = nullptr /* as k_bound_scan's */) {
    if (gate != nullptr && *gate == 0u) return;
    const uint32_t inv = ctrl->thr_inv;
    if (inv == 0u) return;                                             // no H: k_bound_rescore hands the query back
    bound_collect(lo_all, n, ~inv, &ctrl->cand_cnt, cand);
}

// One query's survivors walked exactly by one workgroup (cnt: how many the collect counted; has_H: it had a threshold).  decided(hand_back)
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
        // |q| as the reference's chain (distances.go:20): cosine's finalize takes it, and both metrics' hand-back rule
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

// P8: the re-score behind the 8-bit stage (ctrl = that stage's words, next = the bfloat16 stage's).  It answers, or sets its own flag — the
// word the bfloat16 stage's three launches are gated on — and then that stage decides or hands on to the exact scan.  An 8-bit search counts
// as a bound-scan search in stats[0 .. 2]; its own counters sit at kBound8StatsWord.
// gate (the bfloat16 stage behind the 8-bit one): zero = the 8-bit stage has answered and has cleared this stage's flag for the exact scan
// behind; non-zero = this stage runs, and zeroes the word, which it is the last to read.
template <int M, bool P8 = false>
__global__ void __launch_bounds__(kScanBlock)
k_bound_rescore(IndexView v, const float* __restrict__ query, uint32_t k, BoundCtrl* __restrict__ ctrl, const uint32_t* __restrict__ cand,
                uint32_t* __restrict__ stats, uint32_t* __restrict__ rows_out, float* __restrict__ dist_out, uint32_t* gate = nullptr, BoundCtrl* next = nullptr) {
    if (gate != nullptr && *gate == 0u) return;
    const uint32_t cnt = ctrl->cand_cnt, thr_inv = ctrl->thr_inv;
    bound_rescore_query<M>(v, query, k, cnt, thr_inv != 0u, cand, rows_out, dist_out, [&](bool hand_back) {
        if constexpr (P8) {
            stats[kBound8StatsWord] = cnt;
            if (hand_back) (void)atomicAdd(&stats[kBound8StatsWord + 1], 1u);
            (void)atomicAdd(&stats[kBound8StatsWord + 2], 1u);
            if (!hand_back) { stats[0] = cnt; (void)atomicAdd(&stats[2], 1u); next->flag = 0u; }
        } else {
            stats[0] = cnt;
            if (hand_back) (void)atomicAdd(&stats[1], 1u);
            (void)atomicAdd(&stats[2], 1u);
            if (gate != nullptr) *gate = 0u;                           // (every thread read it before the barriers in front of this call)
        }
        ctrl->flag = hand_back ? 1u : 0u;                              // the launch behind this one reads it
        ctrl->cand_cnt = 0; ctrl->thr_inv = 0;                         // zero, as the words are kept
    });
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

template <int M>
__global__ void __launch_bounds__(kScanBlock)
k_bound_scan8(IndexView v, const float* __restrict__ query, uint32_t k, BoundCtrl* __restrict__ ctrl, uint32_t* __restrict__ lo_all /* [n_tiles * 64] */,
              uint64_t* __restrict__ partial /* [grid][k] */, uint32_t* __restrict__ seed_rows, float* __restrict__ seed_dist) {
    extern __shared__ __align__(16) unsigned char smem[];
    int8_t* qh8 = reinterpret_cast<int8_t*>(smem);                     // [dim] hi terms, [dim] lo terms, dim a multiple of 16
    int8_t* ql8 = qh8 + v.dim;
    uint64_t* wl = reinterpret_cast<uint64_t*>(smem + (size_t)v.dim * 2);   // [kScanWaves][64]
    __shared__ float s_max[kScanWaves];
    __shared__ uint32_t s_bad[kScanWaves];
    __shared__ double s_res[kScanWaves];
    __shared__ double s_qn;
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t steps = v.dim >> 4, tw = gridDim.x * kScanWaves;

    // the query, quantised: sq = max|q_i| / 16256, qq = rint(q / sq) = 128 hi + lo; qres = |q - sq qq| rounded up
    float mx = 0.f; bool bad = false;
    for (uint32_t i = threadIdx.x; i < v.dim; i += blockDim.x) { const float x = query[i]; bad |= !((x - x) == 0.0f); mx = __builtin_fmaxf(mx, __builtin_fabsf(x)); }
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
    for (uint32_t i = threadIdx.x; i < v.dim; i += blockDim.x) {
        const double x = q_ok ? (double)query[i] : 0.0;
        const double qq = __builtin_rint(x / sq);                      // |qq| <= 16256
        const double hi = __builtin_rint(qq * (1.0 / 128.0)), lo = qq - 128.0 * hi;   // |hi| <= 127, |lo| <= 64: exact
        qh8[i] = (int8_t)(int)hi; ql8[i] = (int8_t)(int)lo;
        const double d = x - sq * qq;
        r2 = __builtin_fma(d, d, r2);
    }
    r2 = wave_sum_f64(r2);
    if (lane == 0) s_res[wave] = r2;
    if (wave == kScanWaves - 1) {
        // |q| as the reference's chain (distances.go:20), one wave: 64 values per request, walked in order
        double ma = 0.0;
        for (uint32_t b = 0; b < v.dim; b += 64) {
            const float x = b + lane < v.dim ? query[b + lane] : 0.f;
            const uint32_t n = v.dim - b < 64u ? v.dim - b : 64u;
            for (uint32_t j = 0; j < n; j++) { const double a = (double)__uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(x), j)); ma = __builtin_fma(a, a, ma); }
        }
        if (lane == 0) s_qn = __builtin_sqrt(ma);
    }
    __syncthreads();
    double qres2 = 0.0;
    for (uint32_t w = 0; w < kScanWaves; w++) qres2 += s_res[w];
    const double qn = s_qn;
    // (a query without a scale: every row comes out "unsure", no H, and the re-score hands the search on)
    const double qres = q_ok ? __builtin_sqrt(qres2) * (1.0 + 1e-9) + 1e-300 : __builtin_nan("");

    const u4* qh = reinterpret_cast<const u4*>(qh8);
    const u4* ql = reinterpret_cast<const u4*>(ql8);
    const u4* plane = reinterpret_cast<const u4*>(v.plane8) + lane;
    const uint32_t kth = k - 1;
    uint64_t list = kDeadKey, thr = kDeadKey;
    bool first = true;
    for (uint32_t t = blockIdx.x * kScanWaves + wave; t < v.n_tiles; t += tw) {
        const uint32_t row = t * 64 + lane;
        const double rn = v.rnorm[row];                                // (requested ahead of the tile's bytes: there when the sums are)
        const float sc = v.rscale8[row], rr = v.rres8[row];
        const uint64_t am = v.alive[t];                                // wave-uniform
        const long long isum = bound8_tile(plane + (size_t)t * steps * 64, qh, ql, steps);
        float lo, hi;
        (void)bound_scan_interval8<M>(isum, sq, qn, qres, rn, sc, rr, v.dim, lo, hi);
        const bool live = (am >> lane) & 1ull;                         // (dead rows and the last tile's padding: never candidates, never in a bound)
        __builtin_nontemporal_store(live ? ord_f32(lo) : 0xFFFFFFFFu, &lo_all[row]);
        const uint64_t key = live ? (((uint64_t)ord_f32(hi) << 32) | row) : kDeadKey;
        if (first) { list = wave_sort64(key, lane); thr = readlane64(list, kth); first = false; }
        else list_insert(list, thr, key, kth, lane);
    }
    bound_scan_tail(list, thr, wl, wave, lane, k, ctrl, partial, seed_rows, seed_dist);
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
k_bound_prep_mq(const float* __restrict__ queries, uint32_t nq, uint32_t dim, float* __restrict__ qblk, double* __restrict__ qnorm, uint32_t* __restrict__ stats) {
    __shared__ float s_q[kBoundMaxDim];
    const uint32_t nb = gridDim.x - QB;                                // blocks [0, nb): the block; [nb, nb + QB): one query's norm each
    if (blockIdx.x < nb) {
        const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i < dim * QB) {
            const uint32_t j = i % QB, d = i / QB;
            qblk[i] = j < nq ? queries[(size_t)j * dim + d] : 0.f;
        }
        if (i == 0) stats[0] = 0;                                      // the pass's largest survivor count (k_bound_rescore_mq)
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

// SETS (k_bound_scan_mq<., ., true>: a pass under filters, query j restricted to am_j = alive & set_j): the sets' (bits, words) pairs arrive as kernel
// arguments, as in k_rowset_scan_mq, and lane j keeps query j's — eight pairs held as scalars spilled 168 SGPRs there, and this kernel
// already spends its scalar file on the packed-fma query operands.  rowset_word for the wave's NEXT tile is fetched while the current one is
// walked and read back per query with readlane64 (wave-uniform again).  Bit `lane` of am_j gates query j's lower-bound word (a
// non-candidate writes 0xFFFFFFFF) and its upper-bound key (kDeadKey), so H_j is the k-th smallest upper bound over query j's OWN
// candidates and a set of fewer than k live rows has none (handed back).  A tile that no query selects is not requested — copy, rnorm,
// rres —; its nq x 64 lower-bound words are written as 0xFFFFFFFF (256 bytes per query against dim * 128 of copy): k_bound_collect_mq
// reads every word of a workspace that earlier searches have used, and stays as it is.  `first` is the first tile the wave READS.
// The interval arithmetic is untouched.  A masked call (one bitmap for all queries, in v.alive) is this form with a table of null sets.
template <int M, int QB, bool SETS = false>
__global__ void __launch_bounds__(kScanBlock, 2)
k_bound_scan_mq(IndexView v, const float* __restrict__ qblk, const double* __restrict__ qnorm, uint32_t nq, uint32_t k,
                uint32_t* __restrict__ lo_all /* [nq][n_tiles * 64] */, uint64_t* __restrict__ partial /* [nq][grid][k] */, SetsArg<SETS> tab) {
    extern __shared__ __align__(16) unsigned char smem[];
    uint64_t* wl = reinterpret_cast<uint64_t*>(smem);                  // [kScanWaves][QB][64]
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
                   BoundCtrl* __restrict__ ctrl, uint32_t* __restrict__ cand) {
    const uint32_t j = blockIdx.y;
    const uint32_t H = ord_f32(seed_dist[(size_t)j * k + k - 1]);
    if (seed_rows[(size_t)j * k + k - 1] == 0xFFFFFFFFu || H >= 0xFF800000u) return;   // no H: k_bound_rescore_mq hands the query back
    bound_collect(lo_all + (size_t)j * n, n, H, &ctrl[j].cand_cnt, cand + (size_t)j * kBoundCandCap);
}

template <int M>
__global__ void __launch_bounds__(kScanBlock)
k_bound_rescore_mq(IndexView v, const float* __restrict__ queries, uint32_t k, const uint32_t* __restrict__ seed_rows, const float* __restrict__ seed_dist,
                   BoundCtrl* __restrict__ ctrl, const uint32_t* __restrict__ cand, uint32_t* __restrict__ flags, uint32_t* __restrict__ stats,
                   uint32_t* __restrict__ rows_out, float* __restrict__ dist_out) {
    const uint32_t j = blockIdx.x;
    const uint32_t cnt = ctrl[j].cand_cnt;
    const bool has_H = seed_rows[(size_t)j * k + k - 1] != 0xFFFFFFFFu && ord_f32(seed_dist[(size_t)j * k + k - 1]) < 0xFF800000u;
    bound_rescore_query<M>(v, queries + (size_t)j * v.dim, k, cnt, has_H, cand + (size_t)j * kBoundCandCap, rows_out + (size_t)j * k, dist_out + (size_t)j * k, [&](bool hand_back) {
        (void)atomicMax(&stats[0], cnt);
        if (hand_back) (void)atomicAdd(&stats[1], 1u);
        (void)atomicAdd(&stats[2], 1u);
        flags[j] = hand_back ? 1u : 0u;                                // launch_flat_redo_flagged behind this launch reads them
        ctrl[j].cand_cnt = 0;                                          // zero, as the words are kept
    });
}

ScanPlan plan_scan(uint32_t n_tiles, int cus) {
    ScanPlan p;
    p.block = kScanBlock;
    p.cus = (uint32_t)(cus > 0 ? cus : 1);
    uint32_t want = (n_tiles + kScanWaves - 1) / kScanWaves;          // one tile per wave at most
    static const int wg_per_cu = dev_env_int("QV_SCAN_WG_PER_CU", 2);     // 2 workgroups = 8 waves per CU: measured best (profiles/r01_sweep.txt)
    uint32_t cap = (uint32_t)cus * (uint32_t)wg_per_cu;
    p.grid = want < cap ? want : cap;
    if (p.grid == 0) p.grid = 1;
    // even shares: with T tiles per wave at most, use only as many waves as leave nobody a tile short
    // (1M rows on 256 CUs: 15625 tiles over 2048 waves = 7 or 8 each -> 1954 waves x 8)
    static const int balance = dev_env_int("QV_SCAN_BALANCE", 1);
    if (balance == 1 && want > cap) {
        const uint32_t waves = p.grid * kScanWaves;
        const uint32_t per = (n_tiles + waves - 1) / waves;
        const uint32_t need = (n_tiles + per - 1) / per;
        // measured: 1M x 768: 0.4501 -> 0.4426 ms (85.5 -> 87.0 % of HBM peak); at 77 tiles per wave (10M) the spare
        // waves matter more than the last tile (89.7 -> 89.2 %), so only short shares are evened out
        if (per <= 32) p.grid = (need + kScanWaves - 1) / kScanWaves;
    }
    p.n_lists = p.grid;
    return p;
}

size_t scan_workspace_bytes(const ScanPlan& p, uint32_t nq, uint32_t k) { return ((size_t)p.n_lists * 4 * nq * k * sizeof(uint64_t) + 255) / 256 * 256; }   // x4: the multi-query scan may use up to 8 WG/CU

hipError_t launch_merge_pairs(const float* d_dist, const uint32_t* d_rows, uint32_t n_lists, uint32_t k,
                              uint32_t* d_rows_out, float* d_dist_out, hipStream_t s) {
    if (k == 0 || k > (uint32_t)kMaxFusedK || n_lists == 0) return hipErrorInvalidValue;
    uint32_t total = n_lists * k;
    uint32_t mblock = total >= 16 * 64 * 4 ? kMergeBlock : (total >= 4 * 64 ? 256 : 64);
    hipLaunchKernelGGL(k_merge_pairs, dim3(1), dim3(mblock), 0, s, d_dist, d_rows, total, k, d_rows_out, d_dist_out);
    return hipGetLastError();
}

hipError_t launch_merge_shards(const uint32_t* d_packed, const uint32_t* d_bases, uint32_t n_lists, uint32_t nq, uint32_t k,
                               uint32_t* d_rows_out, float* d_dist_out, hipStream_t s, uint32_t planes) {
    if (k == 0 || k > (uint32_t)kMaxFusedK || n_lists == 0 || nq == 0 || planes == 1) return hipErrorInvalidValue;
    uint32_t total = n_lists * k;
    uint32_t mblock = total >= 16 * 64 * 4 ? kMergeBlock : (total >= 4 * 64 ? 256 : 64);
    hipLaunchKernelGGL(k_merge_shards, dim3(nq), dim3(mblock), 0, s, d_packed, d_bases, n_lists, nq, k, d_rows_out, d_dist_out, planes);
    return hipGetLastError();
}

// (k <= 16: with 64 keys per list the bound lets hundreds through and the two-launch path's 1024-thread merge is faster — 55 against ~30 us at 10k x 128)
bool flat_small_applies(const IndexView& v, uint32_t nq, uint32_t k) { return v.n_tiles <= kSmallTiles && nq >= 1 && nq <= 4 && k >= 1 && k <= 16; }
size_t flat_small_workspace_bytes(uint32_t nq, uint32_t k) { return (size_t)nq * 64 * std::min(k, 16u) * sizeof(uint64_t); }
// d_tickets: 64 words of the caller's own (one set per stream), zero before the first launch; the kernel leaves them zero.
hipError_t launch_flat_small(const IndexView& v, const float* d_queries, uint32_t nq, uint32_t k, void* d_ws, uint32_t* d_tickets, uint32_t* d_rows_out, float* d_dist_out,
                             uint32_t* done_flag, uint32_t done_seq, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (!flat_small_applies(v, nq, k)) return hipErrorInvalidValue;
    const uint32_t grid = std::max(1u, (v.n_tiles + kScanWaves - 1) / kScanWaves);
    uint32_t* tickets = d_tickets;
    uint64_t* partial = static_cast<uint64_t*>(d_ws);
    const size_t lds = query_lds_bytes(v.metric, v.dim4) + (size_t)kScanWaves * 64 * sizeof(uint64_t);
    hipError_t e = hipSuccess;
    QV_DISPATCH_METRIC(v.metric, {
        e = set_lds(k_flat_scan_small<MM, 32>, lds);
        if (e != hipSuccess) return e;
        if (ev0) (void)hipEventRecord(ev0, s);
        hipLaunchKernelGGL((k_flat_scan_small<MM, 32>), dim3(grid, nq), dim3(kScanBlock), lds, s, v, d_queries, k, partial, tickets, d_rows_out, d_dist_out, done_flag, done_seq);
        if (ev1) (void)hipEventRecord(ev1, s);
    });
    return hipGetLastError();
}

// 64 < kk <= kMaxWideK: the scan with R keys per lane, then the selection over the waves' lists
static uint32_t wide_regs(uint32_t) { return 2u; }
size_t flat_wide_workspace_bytes(const ScanPlan& p, uint32_t nq, uint32_t kk) {
    const size_t n = (size_t)p.grid * kScanWaves * 64 * wide_regs(kk);
    return (size_t)nq * n * sizeof(uint64_t) + 256 + select_workspace_bytes(nq, kk);
}
hipError_t launch_flat_wide(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint32_t kk, uint32_t k_stride,
                            void* d_ws, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (kk <= (uint32_t)kMaxFusedK || kk > (uint32_t)kMaxWideK || nq == 0 || kk > k_stride) return hipErrorInvalidValue;
    const uint32_t R = wide_regs(kk);
    const uint32_t n = p.grid * kScanWaves * 64 * R;
    uint64_t* lists = static_cast<uint64_t*>(d_ws);
    void* sel_ws = static_cast<char*>(d_ws) + ((size_t)nq * n * sizeof(uint64_t) + 255) / 256 * 256;
    const size_t lds = query_lds_bytes(v.metric, v.dim4);
    hipError_t e = hipSuccess;
#define QV_WIDE(RR)                                                                                              \
    QV_DISPATCH_METRIC(v.metric, {                                                                                \
        e = set_lds(k_flat_scan_wide<MM, kUnroll, RR>, lds);                                                      \
        if (e != hipSuccess) return e;                                                                            \
        if (ev0) (void)hipEventRecord(ev0, s);                                                                    \
        hipLaunchKernelGGL((k_flat_scan_wide<MM, kUnroll, RR>), dim3(p.grid, nq), dim3(p.block), lds, s, v, d_queries, kk, lists); \
        if (ev1) (void)hipEventRecord(ev1, s);                                                                    \
    })
    QV_WIDE(2);
#undef QV_WIDE
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the lists are not in row order: ties beyond the selection's capacity are settled on the row bits (ordered = false)
    return launch_select_topk(lists, n, n, nq, kk, k_stride, sel_ws, d_rows_out, d_dist_out, s, false, false);
}

// A short corpus in the tile-over-eight-waves form (k_flat_scan_split): one query, a metric whose chain can be split and certified, rows
// wide enough that a wave's own tile is the scan (it pays from 256 dimensions; at 128 the kernels are level and the single polled launch
// wins 16 k - 60 k rows; at 64 nothing), short enough
// that the fixed costs matter (beyond ~160 k rows both forms run at the memory's rate).  QV_SCAN_SPLIT=2: never.
constexpr uint32_t kSplitMaxTiles = 2560;
bool flat_split_applies(const IndexView& v, uint32_t nq, uint32_t k) {
    static const int split = dev_env_int("QV_SCAN_SPLIT", 1), split_max = dev_env_int("QV_SCAN_SPLIT_MAX_TILES", (int)kSplitMaxTiles);
    const bool split_metric = v.metric == QV_COSINE || v.metric == QV_DOT || v.metric == QV_L2 || v.metric == QV_L1 || v.metric == QV_L2SQ_F64;
    const size_t lds = query_lds_bytes(v.metric, v.dim4) + (size_t)3 * kSplitWaves * 64 * sizeof(double) + 40 * 1024;   // + the merge's own arrays
    static const int min_dim4 = dev_env_int("QV_SCAN_SPLIT_MIN_DIM4", 32);       // (128 dimensions: 16 k / 30 k rows 30.8 / 35.6 -> 26.9 / 28.9 us, the rest equal; 64 dimensions: no gain)
    return split == 1 && split_metric && nq == 1 && k >= 1 && k <= (uint32_t)kMaxFusedK && v.dim4 >= (uint32_t)min_dim4 && lds <= (size_t)160 * 1024 &&
           v.n_tiles >= 2 && v.n_tiles <= (uint32_t)split_max;
}
// ... and for the 2 .. 32 queries of a shared pass (k_flat_scan_split_mq, groups of up to 8 per workgroup row, every group reading the corpus
// again): while the groups' reads stay under ~600 MB — measured against the multi-query kernels it replaces, us per call of 8 / 16 / 32 / 64
// queries: 10 k x 768 66 / 87 / 96 / 143 against 119 / 208 / 214 / 218; 30 k x 768 81 / 111 / 162 / 269 against 119 / 212 / 215 / 241;
// 100 k x 768 131 / 181 / 195 / 202 against 169 / 181 / 190 / 197; 10 k x 1536 93 / 99 / 135 / 234 against 182 / 346 / 350 / 349.
// (QV_SCAN_SPLIT_MQ_MAX=1: never.)
bool flat_split_mq_applies(const IndexView& v, uint32_t nq, uint32_t k) {
    static const int split = dev_env_int("QV_SCAN_SPLIT", 1), split_max = dev_env_int("QV_SCAN_SPLIT_MAX_TILES", (int)kSplitMaxTiles), nq_max = dev_env_int("QV_SCAN_SPLIT_MQ_MAX", 32);
    const bool split_metric = v.metric == QV_COSINE || v.metric == QV_DOT || v.metric == QV_L2 || v.metric == QV_L1 || v.metric == QV_L2SQ_F64;
    const uint32_t qsz = (v.metric == QV_COSINE || v.metric == QV_DOT || v.metric == QV_L2SQ_F64) ? 8u : 4u;
    const uint32_t qb = nq <= 4 ? 4u : 8u;
    const size_t lds = (size_t)qb * v.dim4 * 4 * qsz + (size_t)qb * kSplitWaves * 64 * sizeof(double) + 1024;
    const uint64_t reads = (uint64_t)((nq + qb - 1) / qb) * v.n_tiles * v.dim4 * 1024ull;
    static const int min_dim4 = dev_env_int("QV_SCAN_SPLIT_MQ_MIN_DIM4", 16);   // (from 64 dimensions: 10 k x 128, 8 / 16 / 32 queries per call 36 / 40 / 47 us against 64 / 98 / 98)
    return split == 1 && split_metric && nq >= 2 && nq <= (uint32_t)nq_max && k >= 1 && k <= (uint32_t)kMaxFusedK && v.dim4 >= (uint32_t)min_dim4 && lds <= (size_t)160 * 1024 &&
           v.n_tiles >= 2 && v.n_tiles <= (uint32_t)split_max && reads <= 600ull * 1000 * 1000;
}
// The bound scan (k_bound_scan / k_bound_rescore above): one query, a fused-list k, cosine or dot, the bfloat16 copy at hand, a width the copy
// covers in whole 16-dimension steps.  Automatic from kBoundScanMinRows rows (measured: profiles/LAB_r07_bound_scan.md); the index's setter
// (IndexView::bound_scan) or QV_BOUND_SCAN = 1 takes it whenever it applies, 2 never.
// 2 - 8 queries (k_bound_scan_mq): the same conditions, and nq planes of lower bounds that stay under 2 GiB.  Its automatic rule is a floor on
// rows that depends on the width — every query pays 8 bytes per row for its lower bounds whatever the width — per QB: the smallest measured
// shape from which the path wins at every measured nq and k of that QB (profiles/LAB_r08_bound_scan_mq.md); narrower than
// kBoundMqNarrowDim it is never automatic.
constexpr uint32_t kBoundScanMinRows = 300000;   // one query, us, exact / bound scan at k = 1, 10, 64: 100 k x 768 65 / 63, 66 / 70, 86 / 122; 300 k x 768 154 / 107, 158 / 114, 190 / 169; 1M x 128 89 / 64, 93 / 68, 134 / 114
// us per call, exact (k_flat_scan_mq) / bound, at k = 1, 10, 64:
//   QB = 4   300 k x 768  nq 2: 195 / 154, 204 / 160, 273 / 223; nq 4: 193 / 160, 207 / 175, 276 / 271      1M x 128  nq 4: 97 / 93, 117 / 103, 214 / 216 (a loss)
//            10M x 128    nq 2: 781 / 527, 793 / 532, 907 / 593; nq 4: 790 / 575, 793 / 587, 913 / 711
//   QB = 8   300 k x 768  nq 8: 232 / 233, 254 / 264, 370 / 427 (losses)      1M x 768  nq 5: 526 / 449, 545 / 464, 695 / 598; nq 8: 526 / 456, 542 / 473, 697 / 694
//            1M x 128     nq 8: 122 / 124, 145 / 157, 330 / 367 (losses)      10M x 128 nq 5: 888 / 638, 892 / 657, 1162 / 849; nq 8: 869 / 734, 905 / 775, 1161 / 1093
constexpr uint32_t kBoundMqMinDim = 768, kBoundMqMinRows4 = 300000, kBoundMqMinRows8 = 1000000;   // rows of at least 768 dimensions: QB = 4 (2 - 4 queries), QB = 8 (5 - 8)
constexpr uint32_t kBoundMqNarrowDim = 128, kBoundMqNarrowRows = 10000000;                        // 128 <= dim < 768 (nothing between was measured): both QB
static int bound_scan_mode(int mode) { static const int env_mode = env_int("QV_BOUND_SCAN", 0); return mode ? mode : env_mode; }
bool bound_scan_rule(int metric, uint32_t dim, uint32_t n_rows, uint32_t nq, uint32_t k, int mode, bool has_plane) {
    mode = bound_scan_mode(mode);
    const uint32_t n_tiles = (n_rows + 63) / 64;
    if (mode == 2 || nq < 1 || nq > kBoundMqMax || k < 1 || k > (uint32_t)kMaxFusedK || (metric != QV_COSINE && metric != QV_DOT) || !has_plane) return false;
    if ((dim & 15u) != 0 || dim > kBoundMaxDim || n_tiles < 8) return false;
    if (nq == 1) return mode == 1 || n_rows >= kBoundScanMinRows;
    if ((uint64_t)nq * n_tiles * 256 > (2ull << 30)) return false;
    const uint32_t min_rows = dim >= kBoundMqMinDim ? (nq <= 4 ? kBoundMqMinRows4 : kBoundMqMinRows8) : kBoundMqNarrowRows;
    return mode == 1 || (dim >= kBoundMqNarrowDim && n_rows >= min_rows);
}
bool bound_scan_applies(const IndexView& v, uint32_t nq, uint32_t k) { return bound_scan_rule(v.metric, v.dim, v.n_rows, nq, k, v.bound_scan, v.plane != nullptr); }
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
static_assert(kBound8MinRows >= kBoundScanMinRows && kBound8NarrowRows >= kBoundScanMinRows, "the 8-bit floors are never below the bound scan's");
static int bound_plane_mode(int mode) { static const int env_mode = env_int("QV_BOUND_PLANE", 0); return mode ? mode : env_mode; }
bool bound_scan8_rule(int metric, uint32_t dim, uint32_t n_rows, uint32_t nq, uint32_t k, int mode, int plane_mode, bool has_plane8) {
    plane_mode = bound_plane_mode(plane_mode);
    if (plane_mode == 2 || nq != 1 || !has_plane8 || !bound_scan_rule(metric, dim, n_rows, 1, k, mode, true)) return false;
    return plane_mode == 1 || (dim >= kBound8NarrowDim && n_rows >= (dim >= kBound8MinDim ? kBound8MinRows : kBound8NarrowRows));
}
bool bound_scan8_applies(const IndexView& v, uint32_t nq, uint32_t k) {
    return v.plane != nullptr && bound_scan8_rule(v.metric, v.dim, v.n_rows, nq, k, v.bound_scan, v.bound_plane, v.plane8 != nullptr);
}
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
bool bound_scan_rule_filtered(int metric, uint32_t dim, uint32_t n_rows, uint32_t nq, uint32_t k, int mode, bool has_plane, uint32_t candidate_tiles) {
    mode = bound_scan_mode(mode);
    if (mode == 2 || !bound_scan_rule(metric, dim, n_rows, nq, k, 1, has_plane)) return false;
    if (mode == 1) return true;
    const uint64_t n_tiles = ((uint64_t)n_rows + 63) / 64, ct = std::min<uint64_t>(candidate_tiles, n_tiles);
    if (ct == 0 || dim < kBoundFiltMinDim || !bound_scan_rule(metric, dim, n_rows, nq, k, 0, has_plane)) return false;   // (never below the unfiltered floors)
    if (nq == 1) return ct * 10 >= n_tiles;                                                      // from kBoundScanMinRows rows; one tile in ten is the sparsest measured
    if (n_rows < kBoundFiltMqRows) return false;
    if (nq <= 4) return n_rows >= kBoundFiltBigRows ? ct * 5 >= n_tiles : ct * 10 >= n_tiles * 9;
    return ct * 10 >= n_tiles * 9 && (n_rows >= kBoundFiltBigRows || k <= kBoundFiltQb8SmallK);
}
bool bound_scan_applies_filtered(const IndexView& v, uint32_t nq, uint32_t k, uint32_t candidate_tiles) {
    return bound_scan_rule_filtered(v.metric, v.dim, v.n_rows, nq, k, v.bound_scan, v.plane != nullptr, candidate_tiles);
}
// QV_TRACE for the filtered paths' lines: read per call, as launch_rowset_topk reads it (a getenv beside a launch of several kernels), so that
// a process can switch the trace on after its first search; the unfiltered lines keep their one read per process
static bool trace_filtered() { return env_int("QV_TRACE", 0) != 0; }
static bool bound_scan_takes(const IndexView& v, uint32_t nq, uint32_t k, uint32_t candidate_tiles) {
    return candidate_tiles == kBoundNoFilter ? bound_scan_applies(v, nq, k) : bound_scan_applies_filtered(v, nq, k, candidate_tiles);
}
size_t bound_scan_workspace_bytes(const ScanPlan& p, uint32_t k, uint32_t n_tiles) {
    return ((size_t)p.grid * k * sizeof(uint64_t) + 255) / 256 * 256 + 512 + (size_t)kBoundCandCap * sizeof(uint32_t) + (size_t)n_tiles * 64 * sizeof(uint32_t);
}
hipError_t launch_bound_scan(const IndexView& v, const ScanPlan& p, const float* d_query, uint32_t k, void* d_ws, uint32_t* d_ctrl, uint32_t* d_stats,
                             uint32_t* d_rows_out, float* d_dist_out, const uint32_t** gate_out, hipStream_t s, bool masked, bool plane8_first) {
    // (masked: the caller has asked bound_scan_applies_filtered; here only the conditions the kernels need)
    if (!(masked ? bound_scan_rule(v.metric, v.dim, v.n_rows, 1, k, 1, v.plane != nullptr) : bound_scan_applies(v, 1, k)) || !d_ctrl || !d_stats) return hipErrorInvalidValue;
    const uint32_t grid = p.grid;
    char* w = static_cast<char*>(d_ws);
    uint64_t* partial = reinterpret_cast<uint64_t*>(w); w += ((size_t)p.grid * k * sizeof(uint64_t) + 255) / 256 * 256;
    uint32_t* seed_rows = reinterpret_cast<uint32_t*>(w); w += 256;
    float* seed_dist = reinterpret_cast<float*>(w); w += 256;
    uint32_t* cand = reinterpret_cast<uint32_t*>(w); w += (size_t)kBoundCandCap * sizeof(uint32_t);
    uint32_t* lo_all = reinterpret_cast<uint32_t*>(w);
    const uint32_t n_pad = v.n_tiles * 64, cgrid = std::min(1024u, (n_pad + 1023u) / 1024u);
    BoundCtrl* ctrl = reinterpret_cast<BoundCtrl*>(d_ctrl);
    const size_t lds1 = (size_t)v.dim * sizeof(float) + (size_t)kScanWaves * 64 * sizeof(uint64_t);
    const size_t lds2 = query_lds_bytes(v.metric, v.dim4) + (size_t)kScanWaves * 64 * sizeof(uint64_t);
    hipError_t e = hipSuccess;
    if (plane8_first) {
        // the 8-bit stage on the second set of control words, in the same workspace (the stages run one after the other); the bfloat16 stage
        // behind it is gated on that stage's flag and leaves at once when it has answered
        if (masked || !bound_scan8_applies(v, 1, k)) return hipErrorInvalidValue;
        BoundCtrl* ctrl8 = ctrl + 1;
        uint32_t* gate8 = &ctrl8->flag;
        const size_t lds8 = (size_t)v.dim * 2 + (size_t)kScanWaves * 64 * sizeof(uint64_t);
#define QV_BOUND8(MMM)                                                                                                       \
    {                                                                                                                         \
        e = set_lds(k_bound_scan8<MMM>, lds8); if (e != hipSuccess) return e;                                                 \
        e = set_lds((k_bound_rescore<MMM, true>), lds2); if (e != hipSuccess) return e;                                       \
        e = set_lds(k_bound_scan<MMM>, lds1); if (e != hipSuccess) return e;                                                  \
        e = set_lds(k_bound_rescore<MMM>, lds2); if (e != hipSuccess) return e;                                               \
        hipLaunchKernelGGL((k_bound_scan8<MMM>), dim3(grid), dim3(kScanBlock), lds8, s, v, d_query, k, ctrl8, lo_all, partial, seed_rows, seed_dist); \
        hipLaunchKernelGGL(k_bound_collect, dim3(cgrid), dim3(256), 0, s, lo_all, n_pad, ctrl8, cand, (const uint32_t*)nullptr); \
        hipLaunchKernelGGL((k_bound_rescore<MMM, true>), dim3(1), dim3(kScanBlock), lds2, s, v, d_query, k, ctrl8, cand, d_stats, d_rows_out, d_dist_out, (uint32_t*)nullptr, ctrl); \
        hipLaunchKernelGGL((k_bound_scan<MMM>), dim3(grid), dim3(kScanBlock), lds1, s, v, d_query, k, ctrl, lo_all, partial, seed_rows, seed_dist, (const uint32_t*)gate8); \
        hipLaunchKernelGGL(k_bound_collect, dim3(cgrid), dim3(256), 0, s, lo_all, n_pad, ctrl, cand, (const uint32_t*)gate8); \
        hipLaunchKernelGGL((k_bound_rescore<MMM>), dim3(1), dim3(kScanBlock), lds2, s, v, d_query, k, ctrl, cand, d_stats, d_rows_out, d_dist_out, gate8, (BoundCtrl*)nullptr); \
    }
        if (v.metric == QV_COSINE) QV_BOUND8(QV_COSINE) else QV_BOUND8(QV_DOT)
#undef QV_BOUND8
        *gate_out = &ctrl->flag;
        return hipGetLastError();
    }
#define QV_BOUND(MMM)                                                                                                        \
    {                                                                                                                         \
        e = masked ? set_lds((k_bound_scan<MMM, true>), lds1) : set_lds(k_bound_scan<MMM>, lds1); if (e != hipSuccess) return e; \
        e = set_lds(k_bound_rescore<MMM>, lds2); if (e != hipSuccess) return e;                                               \
        if (masked) hipLaunchKernelGGL((k_bound_scan<MMM, true>), dim3(grid), dim3(kScanBlock), lds1, s, v, d_query, k, ctrl, lo_all, partial, seed_rows, seed_dist, (const uint32_t*)nullptr); \
        else hipLaunchKernelGGL((k_bound_scan<MMM>), dim3(grid), dim3(kScanBlock), lds1, s, v, d_query, k, ctrl, lo_all, partial, seed_rows, seed_dist, (const uint32_t*)nullptr); \
        hipLaunchKernelGGL(k_bound_collect, dim3(cgrid), dim3(256), 0, s, lo_all, n_pad, ctrl, cand, (const uint32_t*)nullptr); \
        hipLaunchKernelGGL((k_bound_rescore<MMM>), dim3(1), dim3(kScanBlock), lds2, s, v, d_query, k, ctrl, cand, d_stats, d_rows_out, d_dist_out, (uint32_t*)nullptr, (BoundCtrl*)nullptr); \
    }
    if (v.metric == QV_COSINE) QV_BOUND(QV_COSINE) else QV_BOUND(QV_DOT)
#undef QV_BOUND
    *gate_out = &ctrl->flag;
    return hipGetLastError();
}
float host_bound_interval(int metric, uint32_t dim, float s, double qn, double rn, float rres, float* d_lo, float* d_hi, int* unsure) {
    const double gamma = bound_scan_gamma(dim);
    const bool sure = metric == QV_COSINE ? bound_scan_interval<QV_COSINE>(s, qn, rn, rres, dim, gamma, *d_lo, *d_hi) : bound_scan_interval<QV_DOT>(s, qn, rn, rres, dim, gamma, *d_lo, *d_hi);
    *unsure = sure ? 0 : 1;
    return 0.f;
}

int host_bound_interval8(int metric, uint32_t dim, long long isum, double sq, double qn, double qres, double rn, float rscale, float rres8, float* d_lo, float* d_hi) {
    const bool sure = metric == QV_COSINE ? bound_scan_interval8<QV_COSINE>(isum, sq, qn, qres, rn, rscale, rres8, dim, *d_lo, *d_hi)
                                          : bound_scan_interval8<QV_DOT>(isum, sq, qn, qres, rn, rscale, rres8, dim, *d_lo, *d_hi);
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
int host_bound8_applies(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, int plane_mode, int has_plane8) {
    return bound_scan8_rule(metric, dim, rows, nq, k, mode, plane_mode, has_plane8 != 0) ? 1 : 0;
}

// the shared pass of 2 - 8 queries: d_ws = bound_scan_mq_workspace_bytes, d_ctrl = kBoundMqMax BoundCtrl (zero, left zero).  The exact scan of the
// queries handed back is part of it (launch_flat_redo_flagged, in the bytes the lower bounds leave behind): nothing is read on the host.
static size_t up256(size_t x) { return (x + 255) / 256 * 256; }
size_t bound_scan_mq_workspace_bytes(const ScanPlan& p, uint32_t nq, uint32_t k, uint32_t n_tiles, uint32_t dim) {
    return up256((size_t)nq * p.grid * k * sizeof(uint64_t)) + 2 * up256((size_t)kBoundMqMax * 64 * 4) + 256 + 256 + up256((size_t)dim * kBoundMqMax * sizeof(float)) +
           std::max((size_t)nq * kBoundCandCap * sizeof(uint32_t) + (size_t)nq * n_tiles * 64 * sizeof(uint32_t), redo_workspace_bytes(p, nq, k));
}
hipError_t launch_bound_scan_mq(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint32_t k, void* d_ws, uint32_t* d_ctrl, uint32_t* d_stats,
                                uint32_t* d_rows_out, float* d_dist_out, hipStream_t s, const RowSetRef* h_sets) {
    // h_sets (optional, a HOST array of nq): query j restricted to alive & h_sets[j] — k_bound_scan_mq<., ., true> and the set-carrying redo; the
    // caller has asked bound_scan_applies_filtered, here only the conditions the kernels need.  Null: the unfiltered pass.
    if (nq < 2 || !(h_sets ? bound_scan_rule(v.metric, v.dim, v.n_rows, nq, k, 1, v.plane != nullptr) : bound_scan_applies(v, nq, k)) || !d_ctrl || !d_stats) return hipErrorInvalidValue;
    BoundSetTable tab;
    for (uint32_t i = 0; i < kBoundSets; i++) tab.e[i] = h_sets && i < nq ? h_sets[i] : RowSetRef{nullptr, 0, 0};
    if (h_sets && trace_filtered()) fprintf(stderr, "qv: scan kernel = k_bound_scan_mq sets QB=%d (nq=%u, tiles=%u)\n", nq <= 4 ? 4 : 8, nq, v.n_tiles);
    const uint32_t grid = p.grid;
    char* w = static_cast<char*>(d_ws);
    uint64_t* partial = reinterpret_cast<uint64_t*>(w); w += up256((size_t)nq * grid * k * sizeof(uint64_t));
    uint32_t* seed_rows = reinterpret_cast<uint32_t*>(w); w += up256((size_t)kBoundMqMax * 64 * 4);
    float* seed_dist = reinterpret_cast<float*>(w); w += up256((size_t)kBoundMqMax * 64 * 4);
    uint32_t* flags = reinterpret_cast<uint32_t*>(w); w += 256;
    double* qnorm = reinterpret_cast<double*>(w); w += 256;
    float* qblk = reinterpret_cast<float*>(w); w += up256((size_t)v.dim * kBoundMqMax * sizeof(float));
    void* redo_ws = w;                                                 // (cand and lo_all are dead once the re-score has run)
    uint32_t* cand = reinterpret_cast<uint32_t*>(w); w += (size_t)nq * kBoundCandCap * sizeof(uint32_t);
    uint32_t* lo_all = reinterpret_cast<uint32_t*>(w);
    const uint32_t n_pad = v.n_tiles * 64, cgrid = std::min(1024u, (n_pad + 1023u) / 1024u);
    BoundCtrl* ctrl = reinterpret_cast<BoundCtrl*>(d_ctrl);
    const size_t lds2 = query_lds_bytes(v.metric, v.dim4) + (size_t)kScanWaves * 64 * sizeof(uint64_t);
    hipError_t e = hipSuccess;
#define QV_BOUND_MQ(MMM, QQ)                                                                                                 \
    {                                                                                                                         \
        const size_t lds1 = (size_t)kScanWaves * QQ * 64 * sizeof(uint64_t);                                                  \
        e = set_lds(k_bound_rescore_mq<MMM>, lds2); if (e != hipSuccess) return e;                                            \
        hipLaunchKernelGGL((k_bound_prep_mq<QQ>), dim3((v.dim * QQ + 255) / 256 + QQ), dim3(256), 0, s, d_queries, nq, v.dim, qblk, qnorm, d_stats); \
        if (h_sets) hipLaunchKernelGGL((k_bound_scan_mq<MMM, QQ, true>), dim3(grid), dim3(kScanBlock), lds1, s, v, qblk, qnorm, nq, k, lo_all, partial, tab); \
        else hipLaunchKernelGGL((k_bound_scan_mq<MMM, QQ>), dim3(grid), dim3(kScanBlock), lds1, s, v, qblk, qnorm, nq, k, lo_all, partial, NoSets{}); \
        hipLaunchKernelGGL(k_merge_lists, dim3(nq), dim3(mblock), 0, s, partial, grid, k, seed_rows, seed_dist);             \
        hipLaunchKernelGGL(k_bound_collect_mq, dim3(cgrid, nq), dim3(256), 0, s, lo_all, n_pad, k, seed_rows, seed_dist, ctrl, cand); \
        hipLaunchKernelGGL((k_bound_rescore_mq<MMM>), dim3(nq), dim3(kScanBlock), lds2, s, v, d_queries, k, seed_rows, seed_dist, ctrl, cand, flags, d_stats, d_rows_out, d_dist_out); \
    }
    const uint32_t total = grid * k, mblock = total >= 16 * 64 * 4 ? kMergeBlock : (total >= 4 * 64 ? 256 : 64);
    if (v.metric == QV_COSINE) { if (nq <= 4) QV_BOUND_MQ(QV_COSINE, 4) else QV_BOUND_MQ(QV_COSINE, 8) }
    else { if (nq <= 4) QV_BOUND_MQ(QV_DOT, 4) else QV_BOUND_MQ(QV_DOT, 8) }
#undef QV_BOUND_MQ
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_flat_redo_flagged(v, p, d_queries, nq, k, k, flags, redo_ws, d_rows_out, d_dist_out, s, h_sets);
}
int host_bound_applies_filtered(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, int has_plane, uint32_t candidate_tiles) {
    return bound_scan_rule_filtered(metric, dim, rows, nq, k, mode, has_plane != 0, candidate_tiles) ? 1 : 0;
}
int host_bound_applies(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, int has_plane) { return bound_scan_rule(metric, dim, rows, nq, k, mode, has_plane != 0) ? 1 : 0; }


hipError_t launch_flat_topk(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint32_t k,
                            void* d_ws, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s,
                            hipEvent_t ev0, hipEvent_t ev1, uint32_t* d_tickets, uint32_t* done_flag, uint32_t done_seq, bool* flag_used, uint32_t* d_bound_stats,
                            uint32_t candidate_tiles) {
    if (k == 0 || k > (uint32_t)kMaxFusedK || nq == 0) return hipErrorInvalidValue;
    const size_t lds = query_lds_bytes(v.metric, v.dim4) + (size_t)kScanWaves * 64 * sizeof(uint64_t);
    uint64_t* partial = static_cast<uint64_t*>(d_ws);
    hipError_t e = hipSuccess;
    static const int mq_min = dev_env_int("QV_MQ_MIN", 2);                // nq >= this: queries share a corpus pass
    // 2 - 8 queries sharing one pass over the bfloat16 copy (forced on, it goes ahead of the short-corpus form; on its own it leaves that form its shapes)
    const bool filtered = candidate_tiles != kBoundNoFilter;         // v.alive is a filter's candidate bitmap: one for all queries of the call
    if ((int)nq >= mq_min && nq >= 2 && d_tickets && d_bound_stats && bound_scan_takes(v, nq, k, candidate_tiles) && (bound_scan_mode(v.bound_scan) == 1 || !flat_split_mq_applies(v, nq, k))) {
        static const int trace = env_int("QV_TRACE", 0);
        if (trace && !filtered) fprintf(stderr, "qv: scan kernel = k_bound_scan_mq QB=%d (nq=%u, tiles=%u)\n", nq <= 4 ? 4 : 8, nq, v.n_tiles);
        if (ev0) (void)hipEventRecord(ev0, s);
        const RowSetRef every[kBoundMqMax] = {};                       // (the bitmap is v.alive itself: every query's set is "every row" of it)
        e = launch_bound_scan_mq(v, p, d_queries, nq, k, d_ws, d_tickets + kBoundCtrlWord, d_bound_stats, d_rows_out, d_dist_out, s, filtered ? every : nullptr);
        if (ev1) (void)hipEventRecord(ev1, s);
        return e;
    }
    if ((int)nq >= mq_min && flat_split_mq_applies(v, nq, k)) {
        // a shared pass of a few queries over a short corpus of wide rows: the tile-over-eight-waves form, up to 8 queries per workgroup row
        const uint32_t grid = std::min<uint32_t>(v.n_tiles, std::min<uint32_t>((uint32_t)p.cus, p.n_lists * 4u));
        const uint32_t qsz = (v.metric == QV_COSINE || v.metric == QV_DOT || v.metric == QV_L2SQ_F64) ? 8u : 4u;
#define QV_SMQ(MMM, QQ)                                                                                                     \
        {                                                                                                                     \
            const size_t lds_q = ((size_t)QQ * v.dim4 * 4 * qsz + 15) / 16 * 16 + (size_t)QQ * kSplitWaves * 64 * sizeof(double); \
            e = set_lds(k_flat_scan_split_mq<MMM, QQ>, lds_q);                                                                \
            if (e != hipSuccess) return e;                                                                                    \
            if (ev0) (void)hipEventRecord(ev0, s);                                                                            \
            hipLaunchKernelGGL((k_flat_scan_split_mq<MMM, QQ>), dim3(grid, (nq + QQ - 1) / QQ), dim3(kSplitBlock), lds_q, s, v, d_queries, nq, k, partial); \
            if (ev1) (void)hipEventRecord(ev1, s);                                                                            \
        }
        QV_DISPATCH_METRIC(v.metric, {
            if constexpr (ScanSplitOK<MM>::value) {
                if (nq <= 4) QV_SMQ(MM, 4) else QV_SMQ(MM, 8)
            }
        });
#undef QV_SMQ
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        const uint32_t total = grid * k;
        const uint32_t mblock = total >= 16 * 64 * 4 ? kMergeBlock : (total >= 4 * 64 ? 256 : 64);
        hipLaunchKernelGGL(k_merge_lists, dim3(nq), dim3(mblock), 0, s, partial, grid, k, d_rows_out, d_dist_out);
        return hipGetLastError();
    }
    if ((int)nq >= mq_min) {
        // QB queries per corpus pass.  Measured on MI355X, 256 x 1M x 768 cosine (profiles/r01_sweep_mq.txt):
        // QB=8 is HBM-bound (0.454 ms/pass), QB=16 is f64-VALU-bound (0.75 ms/pass, 12.0 ms per 256 queries).
        static const int mq_qb_env = dev_env_int("QV_MQ_QB", 0), mq_wg = dev_env_int("QV_MQ_WG_PER_CU", 2);
        // the all-float32 metrics spill ~330 SGPRs at 16 queries per pass (16 x 4 scalar query values per chunk on top of the
        // list state): 16 queries take 1.73 ms in one pass and 1.02 ms in two passes of 8 (1M x 768) -> 8 per pass for them
        const bool f32_acc = v.metric == QV_L2SQ || v.metric == QV_COSINE_F32 || v.metric == QV_L2_F32 || v.metric == QV_DOT_F32;
        const int qb = mq_qb_env ? (f32_acc && mq_qb_env == 16 ? 8 : mq_qb_env) : (nq >= 9 ? (f32_acc ? 8 : 16) : (nq >= 5 ? 8 : 4));
        const uint32_t want = (v.n_tiles + kScanWaves - 1) / kScanWaves;
        const uint32_t grid = std::max(1u, std::min(want, (uint32_t)mq_wg * (p.grid / 2 ? p.grid / 2 : 1)));   // p.grid = 2 WG/CU * CUs
        void* qblk = static_cast<char*>(d_ws) + scan_workspace_bytes(p, nq, k);   // tail of the workspace
        // >= 9 cosine/dot queries: the same exact arithmetic on the f64 matrix cores (qv_mq64.hip), 16 or 32 queries per pass
        static const int mq64_min = dev_env_int("QV_MQ64_MIN", 9);
        static const int trace = env_int("QV_TRACE", 0);                  // QV_TRACE=1: name the scan kernel chosen, on stderr
        // (not for short scans: its first tile per wave pays 16 out-of-line sorts; measured slower below ~4 tiles per wave)
        if ((int)nq >= mq64_min && mq_qb_env == 0 && v.n_tiles >= 16u * p.grid && mq64_blocks(v.metric, v.dim4, nq) != 0) {
            // a last pass of 8 queries or fewer costs a whole 32-query pass of the matrix kernel (1.15 ms at 1M x 768) but only an
            // HBM-bound pass of k_flat_scan_mq (0.45-0.65 ms): split it off.  Same stream, so the workspace is reused in order.
            const uint32_t rem = nq & 31u;
            if (nq > 32 && rem >= 1 && rem <= 8) {
                e = launch_flat_topk(v, p, d_queries, nq - rem, k, d_ws, d_rows_out, d_dist_out, s, ev0, ev1, nullptr, nullptr, 0, nullptr);
                if (e != hipSuccess) return e;
                return launch_flat_topk(v, p, d_queries + (size_t)(nq - rem) * v.dim, rem, k, d_ws, d_rows_out + (size_t)(nq - rem) * k,
                                        d_dist_out + (size_t)(nq - rem) * k, s, nullptr, nullptr, nullptr, nullptr, 0, nullptr);
            }
            uint32_t g64 = 0;
            if (trace) fprintf(stderr, "qv: scan kernel = k_flat_scan_mq64 (nq=%u, tiles=%u)\n", nq, v.n_tiles);
            e = launch_flat_scan_mq64(v, (int)p.cus, d_queries, nq, k, qblk, partial, &g64, s, ev0, ev1);
            if (e != hipSuccess) return e;
            const uint32_t total64 = g64 * k;
            const uint32_t mb64 = total64 >= 16 * 64 * 4 ? kMergeBlock : (total64 >= 4 * 64 ? 256 : 64);
            hipLaunchKernelGGL(k_merge_lists, dim3(nq), dim3(mb64), 0, s, partial, g64, k, d_rows_out, d_dist_out);
            return hipGetLastError();
        }
        if (trace) fprintf(stderr, "qv: scan kernel = k_flat_scan_mq QB=%d (nq=%u, tiles=%u)\n", qb, nq, v.n_tiles);
#define QV_MQ_LAUNCH(MMM, QQ)                                                                                              \
        {                                                                                                                     \
            using QT = typename MT<MMM>::Q;                                                                                   \
            const uint32_t groups = (nq + QQ - 1) / QQ;                                                                       \
            const uint32_t per = v.dim4 * 4 * QQ;                                                                             \
            hipLaunchKernelGGL((k_prep_qblk<MMM, QQ>), dim3((per + 255) / 256, groups), dim3(256), 0, s, d_queries, nq, v.dim, v.dim4, static_cast<QT*>(qblk)); \
            const size_t lds_mq = (size_t)kScanWaves * QQ * 64 * sizeof(uint64_t);                                            \
            if (ev0) (void)hipEventRecord(ev0, s);                                                                            \
            hipLaunchKernelGGL((k_flat_scan_mq<MMM, 4, QQ, true>), dim3(grid, groups), dim3(p.block), lds_mq, s, v, d_queries, static_cast<const QT*>(qblk), nq, k, partial); \
            if (ev1) (void)hipEventRecord(ev1, s);                                                                            \
        }
        // (16 per pass never for the all-float32 metrics, see f32_acc above: their instantiations are not built)
        if (qb == 16) { QV_DISPATCH_METRIC(v.metric, { if constexpr (MM == QV_L2SQ || MM == QV_COSINE_F32 || MM == QV_L2_F32 || MM == QV_DOT_F32) return hipErrorInvalidValue; else QV_MQ_LAUNCH(MM, 16) }); }
        else if (qb == 8) { QV_DISPATCH_METRIC(v.metric, { QV_MQ_LAUNCH(MM, 8) }); }
        else if (qb == 4) { QV_DISPATCH_METRIC(v.metric, { QV_MQ_LAUNCH(MM, 4) }); }
        else return hipErrorInvalidValue;
#undef QV_MQ_LAUNCH
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        // partial lists are laid out with stride `grid` lists per query
        uint32_t total = grid * k;
        uint32_t mblock = total >= 16 * 64 * 4 ? kMergeBlock : (total >= 4 * 64 ? 256 : 64);
        hipLaunchKernelGGL(k_merge_lists, dim3(nq), dim3(mblock), 0, s, partial, grid, k, d_rows_out, d_dist_out);
        return hipGetLastError();
    }
#ifdef QV_VARIANTS
    static const int unroll = env_int("QV_SCAN_UNROLL", kUnroll);     // tuning knob of the measurement build (cosine only): loads in flight per wave
    if (v.metric == QV_COSINE && unroll != kUnroll) {
#define QV_SCAN_U(UU)                                                                                             \
        case UU: e = set_lds(k_flat_scan<QV_COSINE, UU>, lds); if (e != hipSuccess) return e;                    \
            if (ev0) (void)hipEventRecord(ev0, s);                                                                \
            hipLaunchKernelGGL((k_flat_scan<QV_COSINE, UU>), dim3(p.grid, nq), dim3(p.block), lds, s, v, d_queries, k, partial, (uint32_t*)nullptr, (uint32_t*)nullptr, (float*)nullptr); \
            if (ev1) (void)hipEventRecord(ev1, s); break;
        switch (unroll) { QV_SCAN_U(4) QV_SCAN_U(8) QV_SCAN_U(12) QV_SCAN_U(24) QV_SCAN_U(32) default: return hipErrorInvalidValue; }
#undef QV_SCAN_U
    } else
#endif
    {
        // one query, the caller's tickets at hand: scan + merge in ONE launch (the last workgroup merges).  QV_SCAN_FUSE=0 (read once)
        // keeps the two launches, for measurements.
        static const int fuse = dev_env_int("QV_SCAN_FUSE", 1);
        if (d_tickets && d_bound_stats && p.grid > 1 && bound_scan_takes(v, nq, k, candidate_tiles)) {
            // the bound scan on the bfloat16 copy, its exact re-score, and the exact scan behind them that runs only when they hand the query back
            static const int trace = env_int("QV_TRACE", 0);
            if (filtered && trace_filtered()) fprintf(stderr, "qv: scan kernel = k_bound_scan masked (tiles=%u, candidate tiles<=%u, k=%u)\n", v.n_tiles, candidate_tiles, k);
            const bool plane8_first = !filtered && bound_scan8_applies(v, nq, k);   // the 8-bit stage first; the bfloat16 stage gated behind it
            if (!filtered && trace && !plane8_first) fprintf(stderr, "qv: scan kernel = k_bound_scan + k_bound_collect + k_bound_rescore (tiles=%u, k=%u)\n", v.n_tiles, k);
            if (plane8_first && trace) fprintf(stderr, "qv: scan kernel = k_bound_scan8 + k_bound_collect + k_bound_rescore, then gated k_bound_scan + k_bound_collect + k_bound_rescore (tiles=%u, k=%u)\n", v.n_tiles, k);
            const uint32_t* gate = nullptr;
            if (ev0) (void)hipEventRecord(ev0, s);
            e = launch_bound_scan(v, p, d_queries, k, static_cast<char*>(d_ws) + scan_workspace_bytes(p, 1, k), d_tickets + kBoundCtrlWord, d_bound_stats, d_rows_out, d_dist_out, &gate, s, filtered, plane8_first);
            if (e != hipSuccess) return e;
            QV_DISPATCH_METRIC(v.metric, {
                if constexpr (MM == QV_COSINE || MM == QV_DOT) {
                    e = set_lds((k_flat_scan<MM, kUnroll, true>), lds);
                    if (e != hipSuccess) return e;
                    hipLaunchKernelGGL((k_flat_scan<MM, kUnroll, true>), dim3(p.grid, 1), dim3(p.block), lds, s, v, d_queries, k, partial, d_tickets, d_rows_out, d_dist_out, (uint32_t*)nullptr, 0u, gate);
                }
            });
            if (ev1) (void)hipEventRecord(ev1, s);
            return hipGetLastError();
        }
        if (d_tickets && fuse && flat_split_applies(v, nq, k)) {
            static const int split_grid = dev_env_int("QV_SCAN_SPLIT_GRID", 0);
            const uint32_t grid = std::min<uint32_t>(v.n_tiles, std::min<uint32_t>(split_grid ? (uint32_t)split_grid : (uint32_t)p.cus, p.n_lists * 4u));
            const size_t lds_s = query_lds_bytes(v.metric, v.dim4) + (size_t)3 * kSplitWaves * 64 * sizeof(double);
            QV_DISPATCH_METRIC(v.metric, {
                if constexpr (ScanSplitOK<MM>::value) {
                    e = set_lds(k_flat_scan_split<MM>, lds_s);
                    if (e != hipSuccess) return e;
                    if (ev0) (void)hipEventRecord(ev0, s);
                    hipLaunchKernelGGL((k_flat_scan_split<MM>), dim3(grid, nq), dim3(kSplitBlock), lds_s, s, v, d_queries, k, partial, d_tickets, d_rows_out, d_dist_out, done_flag, done_seq);
                    if (ev1) (void)hipEventRecord(ev1, s);
                }
            });
            if (flag_used) *flag_used = done_flag != nullptr;
            return hipGetLastError();
        }
        if (d_tickets && nq == 1 && fuse && p.grid > 1) {
            QV_DISPATCH_METRIC(v.metric, {
                e = set_lds((k_flat_scan<MM, kUnroll, true>), lds);
                if (e != hipSuccess) return e;
                if (ev0) (void)hipEventRecord(ev0, s);
                hipLaunchKernelGGL((k_flat_scan<MM, kUnroll, true>), dim3(p.grid, nq), dim3(p.block), lds, s, v, d_queries, k, partial, d_tickets, d_rows_out, d_dist_out, done_flag, done_seq, (const uint32_t*)nullptr);
                if (ev1) (void)hipEventRecord(ev1, s);
            });
            if (flag_used) *flag_used = done_flag != nullptr;
            return hipGetLastError();
        }
    }
    QV_DISPATCH_METRIC(v.metric, {
        e = set_lds(k_flat_scan<MM, kUnroll>, lds);
        if (e != hipSuccess) return e;
        if (ev0) (void)hipEventRecord(ev0, s);
        hipLaunchKernelGGL((k_flat_scan<MM, kUnroll>), dim3(p.grid, nq), dim3(p.block), lds, s, v, d_queries, k, partial, (uint32_t*)nullptr, (uint32_t*)nullptr, (float*)nullptr);
        if (ev1) (void)hipEventRecord(ev1, s);
    });
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    uint32_t total = p.n_lists * k;
    uint32_t mblock = total >= 16 * 64 * 4 ? kMergeBlock : (total >= 4 * 64 ? 256 : 64);
    hipLaunchKernelGGL(k_merge_lists, dim3(nq), dim3(mblock), 0, s, partial, p.n_lists, k, d_rows_out, d_dist_out);
    return hipGetLastError();
}



// for qv_rowset.hip: the multi-query scans' query blocks and list merge, as launch_flat_topk issues them
hipError_t launch_prep_qblk(int metric, uint32_t qb, const float* d_queries, uint32_t nq, uint32_t dim, uint32_t dim4, void* d_qblk, hipStream_t s) {
    if (nq == 0 || (qb != 4 && qb != 8 && qb != 16)) return hipErrorInvalidValue;
    const uint32_t groups = (nq + qb - 1) / qb, per = dim4 * 4 * qb;
    QV_DISPATCH_METRIC(metric, {
        using QT = typename MT<MM>::Q;
        if (qb == 16) {                                               // (the float64-accumulating metrics only, as in launch_flat_topk)
            if constexpr (MM == QV_L2SQ || MM == QV_COSINE_F32 || MM == QV_L2_F32 || MM == QV_DOT_F32) return hipErrorInvalidValue;
            else hipLaunchKernelGGL((k_prep_qblk<MM, 16>), dim3((per + 255) / 256, groups), dim3(256), 0, s, d_queries, nq, dim, dim4, static_cast<QT*>(d_qblk));
        } else if (qb == 8) hipLaunchKernelGGL((k_prep_qblk<MM, 8>), dim3((per + 255) / 256, groups), dim3(256), 0, s, d_queries, nq, dim, dim4, static_cast<QT*>(d_qblk));
        else hipLaunchKernelGGL((k_prep_qblk<MM, 4>), dim3((per + 255) / 256, groups), dim3(256), 0, s, d_queries, nq, dim, dim4, static_cast<QT*>(d_qblk));
    });
    return hipGetLastError();
}
hipError_t launch_merge_lists(const uint64_t* d_partial, uint32_t n_lists, uint32_t nq, uint32_t k, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s) {
    if (k == 0 || k > (uint32_t)kMaxFusedK || n_lists == 0 || nq == 0) return hipErrorInvalidValue;
    const uint32_t total = n_lists * k;
    const uint32_t mblock = total >= 16 * 64 * 4 ? kMergeBlock : (total >= 4 * 64 ? 256 : 64);
    hipLaunchKernelGGL(k_merge_lists, dim3(nq), dim3(mblock), 0, s, d_partial, n_lists, k, d_rows_out, d_dist_out);
    return hipGetLastError();
}

// the exact scan for the queries whose flags are set, decided and listed on the device (see k_flat_scan_redo)
size_t redo_workspace_bytes(const ScanPlan& p, uint32_t nq, uint32_t k) {
    return ((size_t)kRedoSlots * p.grid * k * sizeof(uint64_t) + 255) / 256 * 256 + ((size_t)nq * 4 + 255) / 256 * 256 + ((size_t)(nq + 1) * 4 + 255) / 256 * 256;
}
hipError_t launch_flat_redo_flagged(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint32_t k, uint32_t k_stride, const uint32_t* d_flags,
                                    void* d_ws, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s, const RowSetRef* h_sets) {
    if (k == 0 || k > (uint32_t)kMaxFusedK || nq == 0 || (h_sets && nq > kBoundSets)) return hipErrorInvalidValue;
    BoundSetTable tab;
    for (uint32_t i = 0; i < kBoundSets; i++) tab.e[i] = h_sets && i < nq ? h_sets[i] : RowSetRef{nullptr, 0, 0};
    char* w = static_cast<char*>(d_ws);
    uint64_t* partial = reinterpret_cast<uint64_t*>(w); w += ((size_t)kRedoSlots * p.grid * k * sizeof(uint64_t) + 255) / 256 * 256;
    uint32_t* list = reinterpret_cast<uint32_t*>(w); w += ((size_t)nq * 4 + 255) / 256 * 256;
    uint32_t* count = reinterpret_cast<uint32_t*>(w);
    hipLaunchKernelGGL(k_redo_compact, dim3(1), dim3(1024), 0, s, d_flags, nq, list, count);
    const size_t lds = query_lds_bytes(v.metric, v.dim4) + (size_t)kScanWaves * 64 * sizeof(uint64_t);
    hipError_t e = hipSuccess;
    for (uint32_t first = 0; first < nq; first += kRedoSlots) {
        QV_DISPATCH_METRIC(v.metric, {
            // (the flags come from the batched filter path: its four metrics)
            if constexpr (MM == QV_COSINE || MM == QV_DOT) {         // (sets come with a bound pass: its two metrics)
                if (h_sets) {
                    e = set_lds((k_flat_scan_redo<MM, kUnroll, true>), lds);
                    if (e != hipSuccess) return e;
                    hipLaunchKernelGGL((k_flat_scan_redo<MM, kUnroll, true>), dim3(p.grid), dim3(p.block), lds, s, v, d_queries, k, k_stride, list, count, first, partial, count + 1, d_rows_out, d_dist_out, tab);
                    continue;
                }
            }
            if constexpr (MM == QV_COSINE || MM == QV_L2 || MM == QV_L2SQ || MM == QV_DOT) {
                if (h_sets) return hipErrorInvalidValue;
                e = set_lds((k_flat_scan_redo<MM, kUnroll>), lds);
                if (e != hipSuccess) return e;
                hipLaunchKernelGGL((k_flat_scan_redo<MM, kUnroll>), dim3(p.grid), dim3(p.block), lds, s, v, d_queries, k, k_stride, list, count, first, partial, count + 1, d_rows_out, d_dist_out, NoSets{});
            } else return hipErrorInvalidValue;
        });
    }
    return hipGetLastError();
}

}  // namespace qv
