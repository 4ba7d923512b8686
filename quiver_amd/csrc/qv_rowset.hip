// qv_rowset.hip — exact multi-query scans in which every query carries its own row set (qv_rowset, include/qv.h)
// (shared helpers, the arithmetic contract and the build flags: qv_kernels.h; the kernels these are the per-query-set forms of: qv_scan.hip)
//
// A filtered Collection.Search ranks all rows and keeps the first k whose metadata matches (collection.go:679-759).  With the match
// set known up front as a bitmap on the device, the same k rows come from a top-k over alive & set.  qv_index_search_masked does that
// for ONE bitmap per call (it replaces v.alive for every query); here the queries of a pass each have their own: where k_flat_scan_mq
// reads one wave-uniform word am = v.alive[t] per tile, these kernels form am_j = v.alive[t] & set_j[t] per query j of the pass.  The sets'
// (pointer, words) pairs arrive as KERNEL ARGUMENTS (RowSetTable) — no table to upload, nothing for a device-pointer call to wait
// for.  Words past a set's length are zero (the index grew after the set was made), a null pointer is all-ones.
// Lane j of every wave keeps query j's pair and fetches am_j for the wave's NEXT tile while the current one is walked; the pass reads
// it back per query with v_readlane (a wave-uniform value again).  Held as scalars the eight pairs cost 24 SGPRs the whole loop long,
// on top of the 32 scalar query operands per chunk: the compiler spilled up to 168 of them (55 in k_flat_scan_mq).
// Tile skip: when no query of the pass selects a live row of a tile, the tile's rows are not requested at all (a wave-uniform
// branch in front of the loads) — a selective filter reads fewer bytes than an unfiltered scan.
// The arithmetic is mq_tile / acc1 / finalize / row_accumulate of qv_kernels.h, unchanged: same chains, same float32 bits.
#include "qv_kernels.h"

namespace qv {

bool flat_split_mq_applies(const IndexView& v, uint32_t nq, uint32_t k);      // qv_scan.hip: the rule for the tile-over-eight-waves form

constexpr uint32_t kRsChunk = 64;                       // queries per launch: their sets travel as kernel arguments (1 KiB)
struct RowSetTable { RowSetRef e[kRsChunk]; };

// (rowset_word — lane j < nqg: alive & set_j for tile t; every other lane: 0 — is qv_kernels.h's: the bound scan's set forms use it too)

// ---------------------------------------------------------------- whole tiles per wave (k_flat_scan_mq<., ., ., true> with a set per query) --
// grid = (workgroups, groups of QB queries of this launch's chunk); qblk / partial / nq are the chunk's own.
template <int M, int U, int QB>
__global__ void __launch_bounds__(kScanBlock, 2)
k_rowset_scan_mq(IndexView v, const typename MT<M>::Q* __restrict__ qblk, RowSetTable tab, uint32_t nq, uint32_t k, uint64_t* __restrict__ partial) {
    using Q = typename MT<M>::Q;
    using A = typename MT<M>::A;
    extern __shared__ __align__(16) unsigned char smem[];
    uint64_t* wl = reinterpret_cast<uint64_t*>(smem);                            // [waves][QB][64]
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t q0 = blockIdx.y * QB;
    const uint32_t nqg = nq - q0 < (uint32_t)QB ? nq - q0 : (uint32_t)QB;        // queries of this group (slots past them select nothing)
    const Q* q_lds = qblk + (size_t)blockIdx.y * v.dim4 * 4 * QB;                // global, uniform -> scalar loads
    const bool mine = lane < nqg;
    const RowSetRef rs = tab.e[q0 + (mine ? lane : 0u)];                         // lane j: query j's set

    const uint32_t tw = gridDim.x * kScanWaves;
    const uint32_t kth = k - 1;
    uint64_t list[QB], thr[QB];
    QConst qc[QB];
#pragma unroll
    for (int j = 0; j < QB; j++) { list[j] = kDeadKey; thr[j] = kDeadKey; qc[j].qn = 0.0; qc[j].qn32 = 0.0f; }
    const f4* tiles = reinterpret_cast<const f4*>(v.tiles);
    bool first = true;                                                           // the first tile this wave READS: sorted outright, query norms ride along

    uint32_t t = blockIdx.x * kScanWaves + wave;
    uint64_t w_next = t < v.n_tiles ? rowset_word(v.alive, rs, mine, t) : 0ull;
    for (; t < v.n_tiles; t += tw) {
        const uint64_t w = w_next;                                               // lane j: am_j of this tile
        if (t + tw < v.n_tiles) w_next = rowset_word(v.alive, rs, mine, t + tw);  // (the next tile's: in flight behind this tile's rows)
        if (__ballot(w != 0) == 0) continue;                                     // nobody's candidate in this tile: its rows are not requested
        uint32_t sel = 0;                                                        // bit j: this lane's row is a candidate of query j
#pragma unroll
        for (int j = 0; j < QB; j++) sel |= (uint32_t)((readlane64(w, j) >> lane) & 1ull) << j;
        A acc[QB], qa[QB];
        const uint32_t row = t * 64 + lane;
        double rn = 0.0;
        if constexpr (MT<M>::needs_rnorm) rn = v.rnorm[row];
        if (first) {
            mq_tile<M, U, QB, true>(tiles + (size_t)t * v.dim4 * 64 + lane, q_lds, v.dim4, acc, qa);
#pragma unroll
            for (int j = 0; j < QB; j++) {
                qc[j] = qconst_from_norm2<M>(qa[j]);
                const float dist = finalize<M>(acc[j], qc[j], rn);
                list[j] = wave_sort64(((sel >> j) & 1u) ? make_key(dist, row) : kDeadKey, lane);
                thr[j] = readlane64(list[j], kth);
            }
            first = false;
        } else {
            mq_tile<M, U, QB, false>(tiles + (size_t)t * v.dim4 * 64 + lane, q_lds, v.dim4, acc, qa);
#pragma unroll
            for (int j = 0; j < QB; j++) {
                const float dist = finalize<M>(acc[j], qc[j], rn);
                list_insert(list[j], thr[j], ((sel >> j) & 1u) ? make_key(dist, row) : kDeadKey, kth, lane);
            }
        }
    }

#pragma unroll
    for (int j = 0; j < QB; j++) wl[((size_t)wave * QB + j) * 64 + lane] = list[j];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int j = 0; j < QB; j++) {
            for (uint32_t w = 1; w < kScanWaves; w++) {
                const uint64_t key = lane < k ? wl[((size_t)w * QB + j) * 64 + lane] : kDeadKey;
                list_insert(list[j], thr[j], key, kth, lane);
            }
            if (q0 + j < nq && lane < k) partial[((size_t)(q0 + j) * gridDim.x + blockIdx.x) * k + lane] = list[j];
        }
    }
}

// ---------------------------------------------------------------- a tile over eight waves (k_flat_scan_split_mq with a set per query) --
// Short corpora of wide rows: wave w walks columns [w, w + 1) * dim / 8 of the tile's rows for all QB queries, wave j is query j's
// consumer: it adds the eight partial sums, certifies the float32 (qv_scan.hip, "a tile over several waves") or walks the row again
// as the reference's one chain, and keeps query j's list.  Every wave reads the group's set words, so that all eight agree on a
// skipped tile (the barriers inside a tile are then skipped by all of them); the consumer keeps its own word.
constexpr int kRsSplitWaves = 8;
constexpr int kRsSplitBlock = 64 * kRsSplitWaves;
template <int M> struct RowSetSplitOK { static constexpr bool value = M == QV_COSINE || M == QV_DOT || M == QV_L2 || M == QV_L1 || M == QV_L2SQ_F64; };
template <int M, int QB>
__global__ void __launch_bounds__(kRsSplitBlock)
k_rowset_scan_split_mq(IndexView v, const float* __restrict__ queries, RowSetTable tab, uint32_t nq, uint32_t k, uint64_t* __restrict__ partial) {
    static_assert(QB <= kRsSplitWaves, "one consumer wave per query");
    using Q = typename MT<M>::Q;
    using A = typename MT<M>::A;
    extern __shared__ __align__(16) unsigned char smem[];
    const size_t q_stride = (size_t)v.dim4 * 4;                                    // elements per staged query
    Q* q_lds = reinterpret_cast<Q*>(smem);                                         // [QB][dim4 * 4]
    const size_t q_bytes = ((size_t)QB * q_stride * sizeof(Q) + 15) / 16 * 16;
    double* part = reinterpret_cast<double*>(smem + q_bytes);                      // [QB][kRsSplitWaves][64]
    __shared__ double s_red[QB][kRsSplitWaves];
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t q0 = blockIdx.y * QB;
    const uint32_t nqg = nq - q0 < (uint32_t)QB ? nq - q0 : (uint32_t)QB;          // queries of this group
    for (uint32_t j = 0; j < (uint32_t)QB; j++) {
        const float* q = queries + (size_t)(q0 + (j < nqg ? j : 0)) * v.dim;       // (slots past the group repeat its first query: computed, never written)
        for (uint32_t i = threadIdx.x; i < q_stride; i += kRsSplitBlock) q_lds[j * q_stride + i] = i < v.dim ? (Q)q[i] : (Q)0;
    }
    const bool mine = lane < nqg;
    const RowSetRef rs = tab.e[q0 + (mine ? lane : 0u)];                           // lane j of every wave: query j's set
    __syncthreads();
    double qn_s = 0.0;                                                             // of THIS wave's query (wave j consumes query j)
    if constexpr (M == QV_COSINE || M == QV_DOT) {
        for (uint32_t j = 0; j < (uint32_t)QB; j++) {
            double sq = 0.0;
            for (uint32_t i = threadIdx.x; i < q_stride; i += kRsSplitBlock) { const double a = (double)q_lds[j * q_stride + i]; sq = __builtin_fma(a, a, sq); }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) sq = sq + __shfl_xor(sq, off);
            if (lane == 0) s_red[j][wave] = sq;
        }
        __syncthreads();
        if (wave < (uint32_t)QB) {
            double sq = s_red[wave][0];
#pragma unroll
            for (int w = 1; w < kRsSplitWaves; w++) sq = sq + s_red[wave][w];
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
    const uint32_t c_lo = wave * v.dim4 / kRsSplitWaves, c_hi = (wave + 1) * v.dim4 / kRsSplitWaves;
    const bool consumer = wave < nqg;
    const Q* my_q = q_lds + (size_t)(wave < (uint32_t)QB ? wave : 0) * q_stride;
    uint64_t w_next = blockIdx.x < v.n_tiles ? rowset_word(v.alive, rs, mine, blockIdx.x) : 0ull;
    for (uint32_t t = blockIdx.x; t < v.n_tiles; t += gridDim.x) {
        const uint64_t w = w_next;                                                   // lane j: am_j of this tile
        if (t + gridDim.x < v.n_tiles) w_next = rowset_word(v.alive, rs, mine, t + gridDim.x);
        if (__ballot(w != 0) == 0) continue;                                         // the same decision in all eight waves
        const uint64_t am = readlane64(w, wave & (uint32_t)(QB - 1));                // this consumer's own (waves past the group: unused)
        const uint32_t row = t * 64 + lane;
        double rn = 0.0;
        if (consumer) {
            if constexpr (MT<M>::needs_rnorm || M == QV_DOT) rn = v.rnorm[row];
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
        for (int j = 0; j < QB; j++) part[((size_t)j * kRsSplitWaves + wave) * 64 + lane] = (double)acc[j];
        __syncthreads();
        if (consumer) {
            const double* pb = part + (size_t)wave * kRsSplitWaves * 64;
            double sum = pb[lane];
#pragma unroll
            for (int w = 1; w < kRsSplitWaves; w++) sum = sum + pb[w * 64 + lane];
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

// ---------------------------------------------------------------- the candidate bitmap of the single-query and k > 64 paths --
__global__ void k_rowset_and(const uint64_t* __restrict__ alive, RowSetRef set, uint32_t n_tiles, uint64_t* __restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    const uint64_t w = set.bits == nullptr ? ~0ull : (t < set.words ? set.bits[t] : 0ull);
    out[t] = alive[t] & w;
}

// set / clear listed rows (the caller has checked every row against the set's length)
__global__ void k_rowset_set_rows(uint64_t* __restrict__ bits, const uint32_t* __restrict__ rows, uint32_t n, int selected) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = rows[i];
    unsigned long long* w = reinterpret_cast<unsigned long long*>(bits + (r >> 6));
    const unsigned long long bit = 1ull << (r & 63);
    if (selected) (void)atomicOr(w, bit); else (void)atomicAnd(w, ~bit);
}

// lists of queries whose set holds no live row: padding only
__global__ void k_rowset_pad(uint32_t* __restrict__ rows, float* __restrict__ dist, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { rows[i] = 0xFFFFFFFFu; dist[i] = __uint_as_float(0x7F800000u); }
}
hipError_t launch_rowset_pad(uint32_t* d_rows, float* d_dist, size_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rowset_pad, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, d_rows, d_dist, n);
    return hipGetLastError();
}

hipError_t launch_rowset_and(const IndexView& v, const RowSetRef& set, uint64_t* d_out, hipStream_t s) {
    if (v.n_tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rowset_and, dim3((v.n_tiles + 255) / 256), dim3(256), 0, s, v.alive, set, v.n_tiles, d_out);
    return hipGetLastError();
}

hipError_t launch_rowset_set_rows(uint64_t* d_bits, const uint32_t* d_rows, uint32_t n, int selected, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rowset_set_rows, dim3((n + 255) / 256), dim3(256), 0, s, d_bits, d_rows, n, selected);
    return hipGetLastError();
}

// the flat call's partial lists (flat_layout), with one launch's query blocks as the tail: at most kRsChunk queries, in whole groups of up to 16
struct RowsetLayout { uint64_t* partial; void* qblk; size_t end, total; };
static RowsetLayout rowset_layout(void* base, const ScanPlan& p, uint32_t nq, uint32_t k, uint32_t dim4, WsLog* log = nullptr) {
    const FlatLayout f = flat_layout(base, FlatWs::lists, p, nq, k, 0, dim4 * 4, log);   // (the lists alone read neither the tiles nor the width)
    WsCarver w{static_cast<char*>(base), f.end, f.total, log};
    RowsetLayout L{f.partial, nullptr, 0, 0};
    L.qblk = w.take256<double>((size_t)(kRsChunk + 16) * dim4 * 4);
    return w.finish(L);
}
size_t rowset_workspace_bytes(const ScanPlan& p, uint32_t nq, uint32_t k, uint32_t dim4, WsLog* log) { return rowset_layout(nullptr, p, nq, k, dim4, log).total; }

hipError_t launch_rowset_topk(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint32_t k, const RowSetRef* h_sets,
                              void* d_ws, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (k == 0 || k > (uint32_t)kMaxFusedK || nq == 0 || !h_sets) return hipErrorInvalidValue;
    const int trace = env_int("QV_TRACE", 0);                         // QV_TRACE=1: name the scan kernel chosen, on stderr (read per call: a getenv beside a launch)
    const RowsetLayout L = rowset_layout(d_ws, p, nq, k, v.dim4);
    uint64_t* partial_all = L.partial;
    void* qblk = L.qblk;
    // a short corpus of wide rows: the tile-over-eight-waves form, in launches of up to 32 queries (the rule and its measurements:
    // flat_split_mq_applies); otherwise whole tiles per wave, up to kRsChunk queries per launch.  The rule admits 2 .. 32 queries, so it
    // is asked with one launch's width; its byte bound is then held against the CALL's whole count, every group of 8 reading the corpus
    // again (the rule's own 64-query figures agree: 10 k x 768 and 10 k x 1536 under the bound and faster split, 30 k x 768 over it and slower)
    const uint32_t split_qb = nq <= 4 ? 4u : 8u;
    const uint64_t split_reads = (uint64_t)((nq + split_qb - 1) / split_qb) * v.n_tiles * v.dim4 * 1024ull;
    const bool split = split_reads <= 600ull * 1000 * 1000 && flat_split_mq_applies(v, std::max(2u, std::min(nq, 32u)), k);
    const uint32_t chunk = split ? 32u : kRsChunk;
    hipError_t e = hipSuccess;
    for (uint32_t c0 = 0; c0 < nq; c0 += chunk) {
        const uint32_t nqc = std::min(chunk, nq - c0);
        RowSetTable tab;
        for (uint32_t i = 0; i < kRsChunk; i++) tab.e[i] = i < nqc ? h_sets[c0 + i] : RowSetRef{nullptr, 0, 0};
        const float* q = d_queries + (size_t)c0 * v.dim;
        uint32_t grid;
        if (split) {
            grid = std::min<uint32_t>(v.n_tiles, std::min<uint32_t>((uint32_t)p.cus, p.n_lists * 4u));
            uint64_t* partial = partial_all + (size_t)c0 * grid * k;
            const uint32_t qsz = (v.metric == QV_COSINE || v.metric == QV_DOT || v.metric == QV_L2SQ_F64) ? 8u : 4u;
            if (trace) fprintf(stderr, "qv: scan kernel = k_rowset_scan_split_mq QB=%d (nq=%u, tiles=%u)\n", nqc <= 4 ? 4 : 8, nqc, v.n_tiles);
#define QV_RS_SPLIT(MMM, QQ)                                                                                                  \
            {                                                                                                                 \
                const size_t lds_q = ((size_t)QQ * v.dim4 * 4 * qsz + 15) / 16 * 16 + (size_t)QQ * kRsSplitWaves * 64 * sizeof(double); \
                e = set_lds(k_rowset_scan_split_mq<MMM, QQ>, lds_q);                                                          \
                if (e != hipSuccess) return e;                                                                                \
                if (ev0 && c0 == 0) (void)hipEventRecord(ev0, s);                                                             \
                hipLaunchKernelGGL((k_rowset_scan_split_mq<MMM, QQ>), dim3(grid, (nqc + QQ - 1) / QQ), dim3(kRsSplitBlock), lds_q, s, v, q, tab, nqc, k, partial); \
                if (ev1 && c0 + chunk >= nq) (void)hipEventRecord(ev1, s);                                                    \
            }
            QV_DISPATCH_METRIC(v.metric, {
                if constexpr (RowSetSplitOK<MM>::value) {
                    if (nqc <= 4) QV_RS_SPLIT(MM, 4) else QV_RS_SPLIT(MM, 8)
                } else return hipErrorInvalidValue;
            });
#undef QV_RS_SPLIT
            e = hipGetLastError();
            if (e != hipSuccess) return e;
            e = launch_merge_lists(partial, grid, nqc, k, d_rows_out + (size_t)c0 * k, d_dist_out + (size_t)c0 * k, s);
            if (e != hipSuccess) return e;
            continue;
        }
        const uint32_t want = (v.n_tiles + kScanWaves - 1) / kScanWaves;
        grid = std::max(1u, std::min(want, p.grid));
        uint64_t* partial = partial_all + (size_t)c0 * grid * k;
        // 9 queries or more of a float64-accumulating metric: 16 per pass, as launch_flat_topk chooses (the all-float32 metrics spill at 16
        // and stay at 8: their 16-query instantiations are not built, there or here)
        const bool f32_acc = v.metric == QV_L2SQ || v.metric == QV_COSINE_F32 || v.metric == QV_L2_F32 || v.metric == QV_DOT_F32;
        const uint32_t qb = nqc <= 4 ? 4u : (nqc >= 9 && !f32_acc ? 16u : 8u);
        if (trace) fprintf(stderr, "qv: scan kernel = k_rowset_scan_mq QB=%u (nq=%u, tiles=%u)\n", qb, nqc, v.n_tiles);
        e = launch_prep_qblk(v.metric, qb, q, nqc, v.dim, v.dim4, qblk, s);
        if (e != hipSuccess) return e;
#define QV_RS_MQ(MMM, QQ)                                                                                                     \
        {                                                                                                                     \
            using QT = typename MT<MMM>::Q;                                                                                   \
            const size_t lds_mq = (size_t)kScanWaves * QQ * 64 * sizeof(uint64_t);                                            \
            if (ev0 && c0 == 0) (void)hipEventRecord(ev0, s);                                                                 \
            hipLaunchKernelGGL((k_rowset_scan_mq<MMM, 4, QQ>), dim3(grid, (nqc + QQ - 1) / QQ), dim3(kScanBlock), lds_mq, s, v, static_cast<const QT*>(qblk), tab, nqc, k, partial); \
            if (ev1 && c0 + chunk >= nq) (void)hipEventRecord(ev1, s);                                                        \
        }
        if (qb == 16) { QV_DISPATCH_METRIC(v.metric, { if constexpr (MM == QV_L2SQ || MM == QV_COSINE_F32 || MM == QV_L2_F32 || MM == QV_DOT_F32) return hipErrorInvalidValue; else QV_RS_MQ(MM, 16) }); }
        else if (qb == 8) { QV_DISPATCH_METRIC(v.metric, { QV_RS_MQ(MM, 8) }); }
        else { QV_DISPATCH_METRIC(v.metric, { QV_RS_MQ(MM, 4) }); }
#undef QV_RS_MQ
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = launch_merge_lists(partial, grid, nqc, k, d_rows_out + (size_t)c0 * k, d_dist_out + (size_t)c0 * k, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace qv
