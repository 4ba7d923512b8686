// qv_where.hip — row sets made ON the device: a conjunction of comparisons over typed per-row columns (qv_column, include/qv.h),
// and AND / OR / AND-NOT of existing sets
// (shared helpers and the build flags: qv_kernels.h; the scans that read the sets these kernels write: qv_rowset.hip, qv_bound_scan.hip)
//
// matchesFilter (pkg/core/collection.go:530-632) decides one metadata field of one row at a time, on the host, after a full ranking.
// With the field held as a column beside the vectors, a filter value nobody has asked for before is one streaming pass: a tile of 64
// rows is one wavefront, lane = row; per predicate the tile's presence word is one wave-uniform 64-bit load, its values one coalesced
// 512-byte (F64) or 256-byte (U32) request, the comparison a per-lane boolean and __ballot of it the tile's word for that predicate.
// The words are ANDed, starting from the mask of rows below n_rows; a tile whose word is already zero requests no further column
// (wave-uniform branches in front of the loads — the row-set scans' tile skip), so a selective first predicate saves the later
// columns' bytes.  The predicate table travels as KERNEL ARGUMENTS, as RowSetTable does; literals are read by uniform loads from a
// small device buffer uploaded with the call (an IN list is up to 256 of them: every lane compares against the same one).
// A wave takes kWhereTiles consecutive tiles per iteration: all their value loads are requested before the first comparison waits.
// F64 equality is fabs(x - v) <= 1e-9 in float64, as valuesEqual (collection.go:600-607); nothing here may be contracted or reordered.
#include "qv_kernels.h"

namespace qv {

constexpr int kWhereTiles = 4;                           // tiles per wave and iteration (requests in flight per wave and column): the default, see launch_rowset_where
constexpr int kWhereBlock = 256;
constexpr int kWhereLdsLits = 0;                         // literals by uniform loads from global memory (1: from a copy in LDS): the default

// one comparison of the lane's value against literal v
template <typename T> __device__ __forceinline__ bool where_eq(T x, double v);
template <> __device__ __forceinline__ bool where_eq<double>(double x, double v) { return __builtin_fabs(x - v) <= 1e-9; }
template <> __device__ __forceinline__ bool where_eq<uint32_t>(uint32_t x, double v) { return x == (uint32_t)v; }     // (the host has checked: an integer in [0, 2^32))
template <typename T> __device__ __forceinline__ T where_lit(double v);
template <> __device__ __forceinline__ double where_lit<double>(double v) { return v; }
template <> __device__ __forceinline__ uint32_t where_lit<uint32_t>(double v) { return (uint32_t)v; }

// acc[u] &= (predicate p over tile t0 + u), for the tiles whose word is not zero yet.  Everything but x[] and the booleans is wave-uniform.
// lits: the literals, in global memory (uniform loads) or — LDS — the workgroup's copy of them
template <typename T, int U, typename LP>
__device__ __forceinline__ void where_pred(const WherePred& p, LP lits, uint32_t t0, uint32_t lane, uint64_t (&acc)[U]) {
    constexpr int kWhereTiles = U;
    const T* __restrict__ vals = static_cast<const T*>(p.values);
    T x[kWhereTiles];
#pragma unroll
    for (int u = 0; u < kWhereTiles; u++) {
        x[u] = 0;
        if (acc[u]) x[u] = vals[(size_t)(t0 + u) * 64 + lane];       // (acc != 0 implies a presence bit: the tile is inside the column)
    }
    if (p.op == QV_PRED_IN || p.op == QV_PRED_NOT_IN) {
        // the tiles side by side under one literal: each literal is fetched once for all of them.  (One tile after the other, with no
        // guard inside the literal loop, measured 1.4 to 2 times slower at 256 literals: profiles/rowset_where_notes.md.)
        bool hit[kWhereTiles];
#pragma unroll
        for (int u = 0; u < kWhereTiles; u++) hit[u] = false;
        for (uint32_t i = 0; i < p.n_lit; i++) {
            const double v = lits[p.lit0 + i];
#pragma unroll
            for (int u = 0; u < kWhereTiles; u++)
                if (acc[u]) hit[u] = hit[u] || where_eq<T>(x[u], v);   // (wave-uniform: a tile whose word is zero compares nothing)
        }
#pragma unroll
        for (int u = 0; u < kWhereTiles; u++)
            if (acc[u]) acc[u] &= __ballot(p.op == QV_PRED_IN ? hit[u] : !hit[u]);
        return;
    }
    const double v = lits[p.lit0];
    const T c = where_lit<T>(v);
#pragma unroll
    for (int u = 0; u < kWhereTiles; u++) {
        if (!acc[u]) continue;
        bool b;
        switch (p.op) {
            case QV_PRED_EQ: b = where_eq<T>(x[u], v); break;
            case QV_PRED_NE: b = !where_eq<T>(x[u], v); break;
            case QV_PRED_LT: b = x[u] < c; break;
            case QV_PRED_LE: b = x[u] <= c; break;
            case QV_PRED_GT: b = x[u] > c; break;
            default:         b = x[u] >= c; break;                    // QV_PRED_GE
        }
        acc[u] &= __ballot(b);
    }
}

// The body of one wave's group of U consecutive tiles from t0, for both kernels below — the ONE statement of a conjunction: start from
// the mask of rows below n_rows (ANDed with the index's alive words where the caller wants a candidate bitmap outright), per predicate
// the presence words and where_pred, a tile whose word is zero reading nothing more; lane u < U then stores tile t0 + u's word.
template <int U, typename LP>
__device__ __forceinline__ void where_tiles(const WhereTable& tab, LP lits, const uint64_t* __restrict__ alive, uint32_t t0, uint32_t lane,
                                            uint32_t n_rows, uint32_t n_tiles, uint64_t* __restrict__ out) {
    constexpr int kWhereTiles = U;
    uint64_t acc[kWhereTiles];
#pragma unroll
    for (int u = 0; u < kWhereTiles; u++) {
        const uint64_t r0 = (uint64_t)(t0 + u) * 64;
        acc[u] = r0 + 64 <= n_rows ? ~0ull : (r0 < n_rows ? (1ull << (n_rows - r0)) - 1 : 0ull);
        if (alive != nullptr && acc[u]) acc[u] &= alive[t0 + u];          // (acc != 0: the tile is inside the index)
    }
#pragma unroll
    for (int pi = 0; pi < (int)kWherePreds; pi++) {
        if ((uint32_t)pi >= tab.n) break;
        const WherePred& p = tab.p[pi];
        bool any = false;
#pragma unroll
        for (int u = 0; u < kWhereTiles; u++) {
            if (acc[u]) {                                         // a tile whose word is zero reads nothing more, its presence word included
                const uint64_t pres = t0 + u < p.tiles ? p.present[t0 + u] : 0ull;    // a column shorter than the index: no value
                acc[u] &= p.op == QV_PRED_ABSENT ? ~pres : pres;
            }
            any = any || acc[u] != 0;
        }
        if (!any) break;
        if (p.op == QV_PRED_PRESENT || p.op == QV_PRED_ABSENT) continue;
        if (p.type == QV_COL_F64) where_pred<double, U>(p, lits, t0, lane, acc);
        else where_pred<uint32_t, U>(p, lits, t0, lane, acc);
    }
    if (lane < (uint32_t)kWhereTiles && t0 + lane < n_tiles) {
        uint64_t w = acc[0];
#pragma unroll
        for (int u = 1; u < kWhereTiles; u++) w = lane == (uint32_t)u ? acc[u] : w;
        out[t0 + lane] = w;
    }
}

template <int U, bool LDS>
__global__ void __launch_bounds__(kWhereBlock)
k_rowset_where(WhereTable tab, const double* __restrict__ lits, uint32_t n_lits, uint32_t n_rows, uint32_t n_tiles, uint64_t* __restrict__ out) {
    constexpr int kWhereTiles = U;
    __shared__ double s_lits[LDS ? kWherePreds * kWhereLits : 1];
    if constexpr (LDS) {
        for (uint32_t i = threadIdx.x; i < n_lits; i += kWhereBlock) s_lits[i] = lits[i];
        __syncthreads();
    }
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t waves = gridDim.x * (kWhereBlock / 64);
    for (uint32_t g = blockIdx.x * (kWhereBlock / 64) + wave; (uint64_t)g * kWhereTiles < n_tiles; g += waves) {
        if constexpr (LDS) where_tiles<U>(tab, static_cast<const double*>(s_lits), nullptr, g * kWhereTiles, lane, n_rows, n_tiles, out);
        else where_tiles<U>(tab, lits, nullptr, g * kWhereTiles, lane, n_rows, n_tiles, out);
    }
}

// Up to kWhereMqFilters conjunctions in one launch, for qv_index_search_where: grid y = the filter, grid x = k_rowset_where's grid-stride
// over groups of kWhereTiles tiles; filter f writes a.out[f].  The filters of a launch mostly name the same columns, so their value tiles
// meet in the cache (the per-predicate load chain that profiles/rowset_where_notes.md names as the limit is where_tiles', unchanged).
// ARGLITS: the literals are a.lits[f] in the kernel-argument segment (uniform loads, like the table); otherwise lits + a.lit_base[f].
template <int U, bool ARGLITS>
__global__ void __launch_bounds__(kWhereBlock)
k_where_mq(WhereMqArgs a, const double* __restrict__ lits, const uint64_t* __restrict__ alive, uint32_t n_rows, uint32_t n_tiles) {
    const uint32_t f = blockIdx.y;                                    // (the launch's grid y is a.n)
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t waves = gridDim.x * (kWhereBlock / 64);
    const double* fl = ARGLITS ? a.lits[f] : lits + a.lit_base[f];
    for (uint32_t g = blockIdx.x * (kWhereBlock / 64) + wave; (uint64_t)g * U < n_tiles; g += waves)
        where_tiles<U>(a.tab[f], fl, alive, g * U, lane, n_rows, n_tiles, a.out[f]);
}

// The shape is kWhereTiles tiles per wave, literals as kWhereLdsLits says: what profiles/rowset_where_notes.md measured best.  The
// measurement build (make VARIANTS=1) also holds 1 / 2 / 4 / 8 tiles per wave with either literal source and reads QV_WHERE_TILES /
// QV_WHERE_LDS per call (tests/bench/bench_rowset_where.py --sweep); the product library can neither select nor launch them.
template <int U, bool LDS>
static void launch_where(const WhereTable& tab, const double* d_lits, uint32_t n_lits, uint32_t n_rows, uint32_t n_tiles, uint64_t* d_out, int cus, hipStream_t s) {
    const uint32_t groups = (n_tiles + U - 1) / U;
    const uint32_t want = (groups + kWhereBlock / 64 - 1) / (kWhereBlock / 64);
    const uint32_t grid = std::max(1u, std::min(want, (uint32_t)cus * 8u));      // 8 workgroups of 4 waves per CU: every wave slot, grid stride beyond
    hipLaunchKernelGGL((k_rowset_where<U, LDS>), dim3(grid), dim3(kWhereBlock), 0, s, tab, d_lits, n_lits, n_rows, n_tiles, d_out);
}

hipError_t launch_rowset_where(const WhereTable& tab, const double* d_lits, uint32_t n_rows, uint64_t* d_out, int cus, hipStream_t s) {
    const uint32_t n_tiles = (uint32_t)(((uint64_t)n_rows + 63) / 64);
    if (n_tiles == 0) return hipSuccess;
    const uint32_t n_lits = tab.n ? tab.p[tab.n - 1].lit0 + tab.p[tab.n - 1].n_lit : 0;
    if (n_lits > kWherePreds * kWhereLits) return hipErrorInvalidValue;
#ifdef QV_VARIANTS
    const int tiles = env_int("QV_WHERE_TILES", kWhereTiles);
    const bool lds = env_int("QV_WHERE_LDS", kWhereLdsLits) != 0;
#define QV_WHERE(UU) { if (lds) launch_where<UU, true>(tab, d_lits, n_lits, n_rows, n_tiles, d_out, cus, s); else launch_where<UU, false>(tab, d_lits, n_lits, n_rows, n_tiles, d_out, cus, s); }
    if (tiles == 1) QV_WHERE(1) else if (tiles == 2) QV_WHERE(2) else if (tiles == 8) QV_WHERE(8) else QV_WHERE(4)
#undef QV_WHERE
#else
    launch_where<kWhereTiles, kWhereLdsLits != 0>(tab, d_lits, n_lits, n_rows, n_tiles, d_out, cus, s);
#endif
    return hipGetLastError();
}

hipError_t launch_where_mq(const WhereMqArgs& a, const double* d_lits, const uint64_t* d_alive, uint32_t n_rows, int cus, hipStream_t s) {
    const uint32_t n_tiles = (uint32_t)(((uint64_t)n_rows + 63) / 64);
    if (n_tiles == 0 || a.n == 0) return hipSuccess;
    if (a.n > kWhereMqFilters) return hipErrorInvalidValue;
    for (uint32_t f = 0; f < a.n; f++) {
        const WhereTable& t = a.tab[f];
        if (t.n > kWherePreds || !a.out[f]) return hipErrorInvalidValue;
        const uint32_t n_lits = t.n ? t.p[t.n - 1].lit0 + t.p[t.n - 1].n_lit : 0;
        if (n_lits > (d_lits ? kWherePreds * kWhereLits : kWhereArgLits)) return hipErrorInvalidValue;
    }
    const uint32_t groups = (n_tiles + kWhereTiles - 1) / kWhereTiles;
    const uint32_t want = (groups + kWhereBlock / 64 - 1) / (kWhereBlock / 64);
    const uint32_t grid = std::max(1u, std::min(want, (uint32_t)cus * 8u));      // as launch_where: every wave slot per filter row of the grid, grid stride beyond
    if (d_lits) hipLaunchKernelGGL((k_where_mq<kWhereTiles, false>), dim3(grid, a.n), dim3(kWhereBlock), 0, s, a, d_lits, d_alive, n_rows, n_tiles);
    else hipLaunchKernelGGL((k_where_mq<kWhereTiles, true>), dim3(grid, a.n), dim3(kWhereBlock), 0, s, a, d_lits, d_alive, n_rows, n_tiles);
    return hipGetLastError();
}

// ---------------------------------------------------------------- dst = a OP b, word by word --
// (in place when dst is a or b: every thread reads its own word of both before it writes it)
__global__ void k_rowset_combine(RowSetRef a, RowSetRef b, int op, uint32_t words, uint64_t* dst) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= words) return;
    const uint64_t x = t < a.words ? a.bits[t] : 0ull;               // a set made before the index grew: zeros past its end
    const uint64_t y = t < b.words ? b.bits[t] : 0ull;
    dst[t] = op == QV_SET_AND ? (x & y) : (op == QV_SET_OR ? (x | y) : (x & ~y));
}

hipError_t launch_rowset_combine(const RowSetRef& a, const RowSetRef& b, int op, uint32_t words, uint64_t* d_dst, hipStream_t s) {
    if (words == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rowset_combine, dim3((words + 255) / 256), dim3(256), 0, s, a, b, op, words, d_dst);
    return hipGetLastError();
}

// ---------------------------------------------------------------- presence bits of qv_column_set --
// Rows [first_row, first_row + n): one wave per 64-row word, lane = row, so no two waves ever write the same word and the edge
// words (an unaligned first_row or end) are a read-modify-write by one lane.  bytes == null: every row of the piece has a value.
__global__ void k_column_presence(uint64_t* __restrict__ present, uint32_t first_row, uint32_t n, const uint8_t* __restrict__ bytes) {
    const uint32_t lane = lane_id();
    const uint32_t word = (first_row >> 6) + blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t row = (uint64_t)word * 64 + lane;
    const uint64_t end = (uint64_t)first_row + n;
    if ((uint64_t)word * 64 >= end) return;
    const bool mine = row >= first_row && row < end;
    const bool has = mine && (bytes == nullptr || bytes[row - first_row] != 0);
    const uint64_t touched = __ballot(mine), set = __ballot(has);
    if (lane == 0) present[word] = touched == ~0ull ? set : ((present[word] & ~touched) | set);
}

hipError_t launch_column_presence(uint64_t* d_present, uint32_t first_row, uint32_t n, const uint8_t* d_bytes, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t words = (uint32_t)((((uint64_t)first_row + n + 63) >> 6) - (first_row >> 6));
    hipLaunchKernelGGL(k_column_presence, dim3((words + 3) / 4), dim3(256), 0, s, d_present, first_row, n, d_bytes);
    return hipGetLastError();
}

}  // namespace qv
