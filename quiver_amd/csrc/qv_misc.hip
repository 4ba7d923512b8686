// qv_misc.hip — row gathers, pair distances, ingest, synthetic generator, tombstones
// (shared helpers, the arithmetic contract and the build flags: qv_kernels.h)
#include <algorithm>
#include "qv_kernels.h"
#include "qv_bound.h"

namespace qv {

// ---------------------------------------------------------------- gathers ----------
// lane == listed row; one wave per 64 listed rows
template <int M, int U>
__global__ void __launch_bounds__(64)
k_distance_rows(IndexView v, const float* __restrict__ query, const uint32_t* __restrict__ rows, uint32_t n, float* __restrict__ out) {
    using Q = typename MT<M>::Q;
    extern __shared__ __align__(16) unsigned char smem[];
    Q* q_lds = reinterpret_cast<Q*>(smem);
    stage_query<M>(q_lds, query, v.dim, v.dim4);
    __syncthreads();
    const QConst qc = query_const<M>(q_lds, v.dim);
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t row = rows[i];
    if (row >= v.n_rows) { out[i] = __uint_as_float(0x7FC00000u); return; }
    // a lane walks ITS row: from the row-major copy when the index keeps one (consecutive 16-byte chunks share cache lines:
    // a quarter of the line transactions of the tile layout, where every chunk of a row sits in its own line)
    typename MT<M>::A acc;
    if (v.rowmaj != nullptr && (v.dim & 3) == 0) acc = row_accumulate<M, U, false>(reinterpret_cast<const f4*>(v.rowmaj + (size_t)row * v.dim), 1, q_lds, v.dim4);
    else acc = row_accumulate<M, U, false>(reinterpret_cast<const f4*>(v.tiles) + (size_t)(row >> 6) * v.dim4 * 64 + (row & 63), 64, q_lds, v.dim4);
    double rn = 0.0;
    if constexpr (MT<M>::needs_rnorm) rn = v.rnorm[row];
    out[i] = finalize<M>(acc, qc, rn);
}

// lane == pair; a, b row-major [n][dim]; plain scalar walk (dim need not be a multiple of 4)
template <int M>
__global__ void __launch_bounds__(64)
k_distance_pairs(const float* __restrict__ a, const float* __restrict__ b, uint32_t n, uint32_t dim, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    out[i] = pair_distance<M>(a + (size_t)i * dim, b + (size_t)i * dim, dim);
}

// the same arithmetic on the host, for ONE pair: qv_distance_pair (include/qv.h)
float host_pair_distance(int metric, const float* a, const float* b, uint32_t dim) {
    QV_DISPATCH_METRIC(metric, { return pair_distance<MM>(a, b, dim); });
    return 0.0f;
}

// ---------------------------------------------------------------- ingest -----------
// one wave per touched tile; lane == row within the tile
__global__ void __launch_bounds__(64)
k_ingest(IndexView v, const float* __restrict__ src, uint32_t row0, uint32_t n, uint32_t tile0) {
    const uint32_t t = tile0 + blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t row = t * 64 + lane;
    const bool mine = row >= row0 && row < row0 + n;
    if (mine) {
        const float* s = src + (size_t)(row - row0) * v.dim;
        float4* dst = reinterpret_cast<float4*>(v.tiles) + (size_t)t * v.dim4 * 64 + lane;
        double mb = 0.0; float nb = 0.0f;
        const bool vec_ok = (v.dim & 3) == 0;
        for (uint32_t c = 0; c < v.dim4; c++) {
            float4 x;
            if (vec_ok) x = *reinterpret_cast<const float4*>(s + 4 * c);
            else {
                uint32_t j = 4 * c;
                x.x = j < v.dim ? s[j] : 0.f; x.y = j + 1 < v.dim ? s[j + 1] : 0.f;
                x.z = j + 2 < v.dim ? s[j + 2] : 0.f; x.w = j + 3 < v.dim ? s[j + 3] : 0.f;
            }
            dst[(size_t)c * 64] = x;
            if (v.metric == QV_COSINE || v.metric == QV_DOT || v.metric == QV_L2 || v.metric == QV_L2SQ) {   // distances.go:21 magnitudeB += b*b (non-cosine: |r| for the MFMA filter)
                mb = __builtin_fma((double)x.x, (double)x.x, mb); mb = __builtin_fma((double)x.y, (double)x.y, mb);
                mb = __builtin_fma((double)x.z, (double)x.z, mb); mb = __builtin_fma((double)x.w, (double)x.w, mb);
            } else if (v.metric == QV_COSINE_F32) {                       // adapter.go:119 normB += b*b (unfused)
                float p; p = x.x * x.x; nb = nb + p; p = x.y * x.y; nb = nb + p; p = x.z * x.z; nb = nb + p; p = x.w * x.w; nb = nb + p;
            }
        }
        if (v.metric == QV_COSINE || v.metric == QV_DOT || v.metric == QV_L2 || v.metric == QV_L2SQ) v.rnorm[row] = __builtin_sqrt(mb);
        else if (v.metric == QV_COSINE_F32) v.rnorm[row] = nb == 0.0f ? -1.0 : (double)(float)__builtin_sqrt((double)nb);
    }
    uint64_t m = __ballot(mine);
    if (lane == 0 && m) atomicOr(reinterpret_cast<unsigned long long*>(&v.alive[t]), (unsigned long long)m);
}

// Rows whose dimension is a multiple of 4 (every 16-byte chunk whole): one 256-thread workgroup per touched tile moves 64 rows x
// 16 chunks at a time through LDS — the source is read in 256-byte runs of a row, the tile layout ([chunk][64 rows][4 dims]) is
// written in 1 KiB runs of a chunk, and the row-major copy (when the index keeps one) is written from the registers that read
// the source instead of by a second pass over it.  (k_ingest below reads 16 bytes per lane at a stride of one row: every
// line of the source is fetched eight times over; measured 1M x 768: 5.7 ms, 8.1 ms with the row-major copy.)
// The per-row constants are computed by one lane per row in element order, as k_ingest does (distances.go:21, adapter.go:119).
constexpr int kIngestCB = 16;                               // chunks per LDS block
__global__ void __launch_bounds__(256)
k_ingest_tiled(IndexView v, const float* __restrict__ src, uint32_t row0, uint32_t n, uint32_t tile0) {
    __shared__ float4 stage[64][kIngestCB + 1];             // +1: the transposed reads of the store phase hit distinct banks
    const uint32_t t = tile0 + blockIdx.x;
    const uint32_t tid = threadIdx.x;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* tiles = reinterpret_cast<float4*>(v.tiles) + (size_t)t * v.dim4 * 64;
    float4* rm4 = v.rowmaj ? reinterpret_cast<float4*>(v.rowmaj) : nullptr;
    const bool f64norm = v.metric == QV_COSINE || v.metric == QV_DOT || v.metric == QV_L2 || v.metric == QV_L2SQ;
    const bool f32norm = v.metric == QV_COSINE_F32;
    double mb = 0.0; float nb = 0.0f;
    const uint32_t my_row = t * 64 + tid;                   // wave 0: the row whose constants this lane accumulates
    const bool my_mine = tid < 64 && my_row >= row0 && my_row < row0 + n;
    for (uint32_t cb = 0; cb < v.dim4; cb += kIngestCB) {
#pragma unroll
        for (int i = 0; i < 4; i++) {                       // 16 consecutive threads read 256 contiguous bytes of one row
            const uint32_t idx = tid + 256u * i, r = idx / kIngestCB, ch = idx % kIngestCB;
            const uint32_t row = t * 64 + r;
            float4 x = {0.f, 0.f, 0.f, 0.f};
            if (row >= row0 && row < row0 + n && cb + ch < v.dim4) {
                x = s4[(size_t)(row - row0) * v.dim4 + cb + ch];
                if (rm4) rm4[(size_t)row * v.dim4 + cb + ch] = x;
            }
            stage[r][ch] = x;
        }
        __syncthreads();
        if (my_mine) {
            const uint32_t nch = v.dim4 - cb < (uint32_t)kIngestCB ? v.dim4 - cb : (uint32_t)kIngestCB;
            for (uint32_t ch = 0; ch < nch; ch++) {
                const float4 x = stage[tid][ch];
                if (f64norm) {
                    mb = __builtin_fma((double)x.x, (double)x.x, mb); mb = __builtin_fma((double)x.y, (double)x.y, mb);
                    mb = __builtin_fma((double)x.z, (double)x.z, mb); mb = __builtin_fma((double)x.w, (double)x.w, mb);
                } else if (f32norm) {
                    float p; p = x.x * x.x; nb = nb + p; p = x.y * x.y; nb = nb + p; p = x.z * x.z; nb = nb + p; p = x.w * x.w; nb = nb + p;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {                       // 64 consecutive threads write the 1 KiB of one chunk
            const uint32_t idx = tid + 256u * i, ch = idx / 64, r = idx % 64;
            const uint32_t row = t * 64 + r;
            if (row >= row0 && row < row0 + n && cb + ch < v.dim4) tiles[(size_t)(cb + ch) * 64 + r] = stage[r][ch];
        }
        __syncthreads();
    }
    if (my_mine) {
        if (f64norm) v.rnorm[my_row] = __builtin_sqrt(mb);
        else if (f32norm) v.rnorm[my_row] = nb == 0.0f ? -1.0 : (double)(float)__builtin_sqrt((double)nb);
    }
    if (tid < 64) {
        const uint64_t m = __ballot(my_mine);
        if (tid == 0 && m) atomicOr(reinterpret_cast<unsigned long long*>(&v.alive[t]), (unsigned long long)m);
    }
}

// ---------------------------------------------------------------- scattered ingest --
// Overwrite listed rows in place (qv_index_update_rows): the twins of the two kernels above, one workgroup per TOUCHED tile.  The host
// hands over the list sorted and distinct — rows[m] ascending, src[m] = the position of each row's vector in vecs (the vectors are
// never permuted), tile_first[b] .. tile_first[b + 1] = the entries of touched tile tiles[b].  A 64-entry LDS table maps the tile's
// slot to its source vector (kNotListed: the slot keeps what it holds); everything a listed slot gets — the tile layout, the
// row-major copy, rnorm in element order with ingest's chains and its -1 sentinel, the alive bit — is what ingest gives that row.
constexpr uint32_t kNotListed = 0xFFFFFFFFu;

// wave per touched tile; lane == slot (every dimension, every alignment of the source)
__global__ void __launch_bounds__(64)
k_update_rows(IndexView v, const float* __restrict__ src, const uint32_t* __restrict__ rows, const uint32_t* __restrict__ srcidx,
              const uint32_t* __restrict__ tile_first, const uint32_t* __restrict__ tiles) {
    __shared__ uint32_t slot_src[64];
    const uint32_t t = tiles[blockIdx.x], e0 = tile_first[blockIdx.x], e1 = tile_first[blockIdx.x + 1];
    const uint32_t lane = threadIdx.x;
    slot_src[lane] = kNotListed;
    __syncthreads();
    if (e0 + lane < e1) slot_src[rows[e0 + lane] & 63u] = srcidx[e0 + lane];    // (distinct rows of one tile: at most 64, distinct slots)
    __syncthreads();
    const uint32_t row = t * 64 + lane;
    const uint32_t from = slot_src[lane];
    const bool mine = from != kNotListed;
    if (mine) {
        const float* s = src + (size_t)from * v.dim;
        float4* dst = reinterpret_cast<float4*>(v.tiles) + (size_t)t * v.dim4 * 64 + lane;
        float* rm = v.rowmaj ? v.rowmaj + (size_t)row * v.dim : nullptr;
        double mb = 0.0; float nb = 0.0f;
        for (uint32_t c = 0; c < v.dim4; c++) {
            const uint32_t j = 4 * c;
            float4 x;
            x.x = j < v.dim ? s[j] : 0.f; x.y = j + 1 < v.dim ? s[j + 1] : 0.f;
            x.z = j + 2 < v.dim ? s[j + 2] : 0.f; x.w = j + 3 < v.dim ? s[j + 3] : 0.f;
            dst[(size_t)c * 64] = x;
            if (rm) {                                                  // (no contiguous copy serves a scatter: the kernel writes the row-major copy)
                if (j < v.dim) rm[j] = x.x;
                if (j + 1 < v.dim) rm[j + 1] = x.y;
                if (j + 2 < v.dim) rm[j + 2] = x.z;
                if (j + 3 < v.dim) rm[j + 3] = x.w;
            }
            if (v.metric == QV_COSINE || v.metric == QV_DOT || v.metric == QV_L2 || v.metric == QV_L2SQ) {   // as k_ingest
                mb = __builtin_fma((double)x.x, (double)x.x, mb); mb = __builtin_fma((double)x.y, (double)x.y, mb);
                mb = __builtin_fma((double)x.z, (double)x.z, mb); mb = __builtin_fma((double)x.w, (double)x.w, mb);
            } else if (v.metric == QV_COSINE_F32) {
                float p; p = x.x * x.x; nb = nb + p; p = x.y * x.y; nb = nb + p; p = x.z * x.z; nb = nb + p; p = x.w * x.w; nb = nb + p;
            }
        }
        if (v.metric == QV_COSINE || v.metric == QV_DOT || v.metric == QV_L2 || v.metric == QV_L2SQ) v.rnorm[row] = __builtin_sqrt(mb);
        else if (v.metric == QV_COSINE_F32) v.rnorm[row] = nb == 0.0f ? -1.0 : (double)(float)__builtin_sqrt((double)nb);
    }
    const uint64_t m = __ballot(mine);
    if (lane == 0 && m) atomicOr(reinterpret_cast<unsigned long long*>(&v.alive[t]), (unsigned long long)m);
}

// dim a multiple of 4, source 16-byte aligned: k_ingest_tiled's walk — 256-byte runs of a listed row in, 1 KiB runs of a chunk out
__global__ void __launch_bounds__(256)
k_update_rows_tiled(IndexView v, const float* __restrict__ src, const uint32_t* __restrict__ rows, const uint32_t* __restrict__ srcidx,
                    const uint32_t* __restrict__ tile_first, const uint32_t* __restrict__ tiles) {
    __shared__ float4 stage[64][kIngestCB + 1];
    __shared__ uint32_t slot_src[64];
    const uint32_t t = tiles[blockIdx.x], e0 = tile_first[blockIdx.x], e1 = tile_first[blockIdx.x + 1];
    const uint32_t tid = threadIdx.x;
    if (tid < 64) slot_src[tid] = kNotListed;
    __syncthreads();
    if (e0 + tid < e1) slot_src[rows[e0 + tid] & 63u] = srcidx[e0 + tid];
    __syncthreads();
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* tile = reinterpret_cast<float4*>(v.tiles) + (size_t)t * v.dim4 * 64;
    float4* rm4 = v.rowmaj ? reinterpret_cast<float4*>(v.rowmaj) : nullptr;
    const bool f64norm = v.metric == QV_COSINE || v.metric == QV_DOT || v.metric == QV_L2 || v.metric == QV_L2SQ;
    const bool f32norm = v.metric == QV_COSINE_F32;
    double mb = 0.0; float nb = 0.0f;
    const uint32_t my_row = t * 64 + tid;                   // wave 0: the row whose constants this lane accumulates
    const bool my_mine = tid < 64 && slot_src[tid & 63u] != kNotListed;
    for (uint32_t cb = 0; cb < v.dim4; cb += kIngestCB) {
#pragma unroll
        for (int i = 0; i < 4; i++) {                       // 16 consecutive threads read 256 contiguous bytes of one listed row's vector
            const uint32_t idx = tid + 256u * i, r = idx / kIngestCB, ch = idx % kIngestCB;
            const uint32_t from = slot_src[r];
            float4 x = {0.f, 0.f, 0.f, 0.f};
            if (from != kNotListed && cb + ch < v.dim4) {
                x = s4[(size_t)from * v.dim4 + cb + ch];
                if (rm4) rm4[(size_t)(t * 64 + r) * v.dim4 + cb + ch] = x;
            }
            stage[r][ch] = x;
        }
        __syncthreads();
        if (my_mine) {
            const uint32_t nch = v.dim4 - cb < (uint32_t)kIngestCB ? v.dim4 - cb : (uint32_t)kIngestCB;
            for (uint32_t ch = 0; ch < nch; ch++) {
                const float4 x = stage[tid][ch];
                if (f64norm) {
                    mb = __builtin_fma((double)x.x, (double)x.x, mb); mb = __builtin_fma((double)x.y, (double)x.y, mb);
                    mb = __builtin_fma((double)x.z, (double)x.z, mb); mb = __builtin_fma((double)x.w, (double)x.w, mb);
                } else if (f32norm) {
                    float p; p = x.x * x.x; nb = nb + p; p = x.y * x.y; nb = nb + p; p = x.z * x.z; nb = nb + p; p = x.w * x.w; nb = nb + p;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {                       // 64 consecutive threads write the 1 KiB of one chunk (listed slots only)
            const uint32_t idx = tid + 256u * i, ch = idx / 64, r = idx % 64;
            if (slot_src[r] != kNotListed && cb + ch < v.dim4) tile[(size_t)(cb + ch) * 64 + r] = stage[r][ch];
        }
        __syncthreads();
    }
    if (my_mine) {
        if (f64norm) v.rnorm[my_row] = __builtin_sqrt(mb);
        else if (f32norm) v.rnorm[my_row] = nb == 0.0f ? -1.0 : (double)(float)__builtin_sqrt((double)nb);
    }
    if (tid < 64) {
        const uint64_t m = __ballot(my_mine);
        if (tid == 0 && m) atomicOr(reinterpret_cast<unsigned long long*>(&v.alive[t]), (unsigned long long)m);
    }
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ int32_t gen_int(uint64_t row_key, uint32_t col) {
    uint64_t h = splitmix64(row_key + (uint64_t)col);
    int32_t s = (int32_t)(h & 0xFFFF) + (int32_t)((h >> 16) & 0xFFFF) + (int32_t)((h >> 32) & 0xFFFF) + (int32_t)(h >> 48);
    return s - 131070;
}

// the synthetic-corpus generator of DESIGN.md (SplitMix64 -> Irwin-Hall(4) integers -> unit L2),
// written straight into the tile layout; integer arithmetic plus correctly rounded float64
// sqrt/div only, so any IEEE host reproduces it bit for bit
__global__ void __launch_bounds__(64)
k_generate(IndexView v, uint64_t seed, uint64_t gen_row0, uint32_t row0, uint32_t n, uint32_t tile0) {
    const uint32_t t = tile0 + blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t row = t * 64 + lane;
    const bool mine = row >= row0 && row < row0 + n;
    if (mine) {
        const uint64_t g = gen_row0 + (row - row0);
        const uint64_t row_key = splitmix64(seed ^ (g * 0xD1342543DE82EF95ull));
        double sumsq = 0.0;
        for (uint32_t c = 0; c < v.dim; c++) { double x = (double)gen_int(row_key, c); sumsq = __builtin_fma(x, x, sumsq); }
        const double norm = sumsq > 0.0 ? __builtin_sqrt(sumsq) : 1.0;
        float4* dst = reinterpret_cast<float4*>(v.tiles) + (size_t)t * v.dim4 * 64 + lane;
        double mb = 0.0; float nb = 0.0f;
        for (uint32_t c = 0; c < v.dim4; c++) {
            float e[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t col = 4 * c + j;
                e[j] = col < v.dim ? (float)((double)gen_int(row_key, col) / norm) : 0.0f;
                if (v.metric == QV_COSINE || v.metric == QV_DOT || v.metric == QV_L2 || v.metric == QV_L2SQ) mb = __builtin_fma((double)e[j], (double)e[j], mb);
                else if (v.metric == QV_COSINE_F32) { float p = e[j] * e[j]; nb = nb + p; }
            }
            dst[(size_t)c * 64] = make_float4(e[0], e[1], e[2], e[3]);
        }
        if (v.metric == QV_COSINE || v.metric == QV_DOT || v.metric == QV_L2 || v.metric == QV_L2SQ) v.rnorm[row] = __builtin_sqrt(mb);
        else if (v.metric == QV_COSINE_F32) v.rnorm[row] = nb == 0.0f ? -1.0 : (double)(float)__builtin_sqrt((double)nb);
        if (v.rowmaj) {
            float* rm = v.rowmaj + (size_t)row * v.dim;
            for (uint32_t c = 0; c < v.dim; c++) rm[c] = (float)((double)gen_int(row_key, c) / norm);
        }
    }
    uint64_t m = __ballot(mine);
    if (lane == 0 && m) atomicOr(reinterpret_cast<unsigned long long*>(&v.alive[t]), (unsigned long long)m);
}

__global__ void k_set_alive(IndexView v, const uint32_t* __restrict__ rows, uint32_t n, int alive) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t r = rows[i];
    if (r >= v.n_rows) return;
    unsigned long long bit = 1ull << (r & 63);
    if (alive) atomicOr(reinterpret_cast<unsigned long long*>(&v.alive[r >> 6]), bit);
    else atomicAnd(reinterpret_cast<unsigned long long*>(&v.alive[r >> 6]), ~bit);
}

__global__ void k_fetch_row(IndexView v, uint32_t row, float* __restrict__ out) {
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= v.dim) return;
    out[j] = v.tiles[((size_t)(row >> 6) * v.dim4 + (j >> 2)) * 256 + (row & 63) * 4 + (j & 3)];
}

hipError_t launch_distance_rows(const IndexView& v, const float* d_query, const uint32_t* d_rows, uint32_t n,
                                float* d_dist_out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const size_t lds = query_lds_bytes(v.metric, v.dim4);
    hipError_t e = hipSuccess;
    QV_DISPATCH_METRIC(v.metric, {
        e = set_lds(k_distance_rows<MM, kUnroll>, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((k_distance_rows<MM, kUnroll>), dim3((n + 63) / 64), dim3(64), lds, s, v, d_query, d_rows, n, d_dist_out);
    });
    return hipGetLastError();
}

hipError_t launch_distance_pairs(int metric, const float* d_a, const float* d_b, uint32_t n, uint32_t dim, float* d_out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    QV_DISPATCH_METRIC(metric, {
        hipLaunchKernelGGL((k_distance_pairs<MM>), dim3((n + 63) / 64), dim3(64), 0, s, d_a, d_b, n, dim, d_out);
    });
    return hipGetLastError();
}

// The bfloat16 copy of tiles [t0, t1] (QV_FLAG_BF16_ROWS): [tile][16-dim step][32-row block][8-dim half][row of the block][8 values] — the
// 64 lanes of a wave that wants (step, block) as its MFMA B operand read ONE contiguous KiB; value = bf16(float32 row value), round to
// nearest even — what the batched filter would compute on the fly.  One thread per (tile, 8-dim group, row); refreshed by every
// launcher that writes rows, on the same stream, so the plane is never behind the tiles.
__global__ void __launch_bounds__(256)
k_bf16_plane(IndexView v, uint32_t t0, uint32_t n_tiles, const uint32_t* __restrict__ list) {
    typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
    const uint32_t dim8 = (v.dim4 + 1) / 2;
    const uint64_t total = (uint64_t)n_tiles * dim8 * 64;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(i & 63), c8 = (uint32_t)((i >> 6) % dim8), ti = (uint32_t)((i >> 6) / dim8), t = list ? list[ti] : t0 + ti;
        const f4* src = reinterpret_cast<const f4*>(v.tiles) + (size_t)t * v.dim4 * 64 + r;
        const f4 a = src[(size_t)(2 * c8) * 64];
        f4 b = {0.f, 0.f, 0.f, 0.f};
        if (2 * c8 + 1 < v.dim4) b = src[(size_t)(2 * c8 + 1) * 64];
        const bf2 p0 = {(__bf16)a.x, (__bf16)a.y}, p1 = {(__bf16)a.z, (__bf16)a.w}, p2 = {(__bf16)b.x, (__bf16)b.y}, p3 = {(__bf16)b.z, (__bf16)b.w};
        uint4 o;
        o.x = __builtin_bit_cast(uint32_t, p0); o.y = __builtin_bit_cast(uint32_t, p1); o.z = __builtin_bit_cast(uint32_t, p2); o.w = __builtin_bit_cast(uint32_t, p3);
        const uint32_t steps8 = (dim8 + 1) / 2;
        reinterpret_cast<uint4*>(v.plane)[((((size_t)t * steps8 + (c8 >> 1)) * 2 + (r >> 5)) * 2 + (c8 & 1)) * 32 + (r & 31)] = o;
    }
}
// |r - bf16(r)| of the rows of tiles [t0, t0 + n_tiles): what the one-term bfloat16 filter drops of a row (qv_batched.hip: its
// margin is |q - qh||r| + |qh||r - rh|, a third of the worst case 2 * 2^-8 |q||r| on ordinary data).  Lane == row, one wave per
// tile, 1 KiB per request; the value only feeds a bound, so it is rounded UP (float64 sum, correctly rounded sqrt, one more
// float32 step than round-to-nearest) and the order of the additions is free.  Elements whose bfloat16 IMAGE is below 2^-126 in
// magnitude count whole (an element just under 2^-126 that rounds up to it does not): the matrix core may flush such an operand.
__global__ void __launch_bounds__(64)
k_row_residual(IndexView v, uint32_t t0, const uint32_t* __restrict__ list) {
    const uint32_t t = list ? list[blockIdx.x] : t0 + blockIdx.x, lane = threadIdx.x;
    const f4* src = reinterpret_cast<const f4*>(v.tiles) + (size_t)t * v.dim4 * 64 + lane;
    double s2 = 0.0;
    auto one = [&](float x) {
        const __bf16 hb = (__bf16)x;
        float h = (float)hb;
        if (__builtin_fabsf(h) < 1.17549435e-38f) h = 0.f;
        const double d = (double)x - (double)h;
        s2 = __builtin_fma(d, d, s2);
    };
    for (uint32_t c = 0; c < v.dim4; c += 4) {
        f4 x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) x[u] = c + u < v.dim4 ? src[(size_t)(c + u) * 64] : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 4; u++) { one(x[u].x); one(x[u].y); one(x[u].z); one(x[u].w); }
    }
    const float r = (float)(__builtin_sqrt(s2) * (1.0 + 1e-12));
    // next float up (NaN / inf stay: such a row's norm is NaN / inf too and the filter passes it on)
    float up = r;
    if (r == r && r != __builtin_inff()) up = r == 0.f ? (s2 == 0.0 ? 0.f : __uint_as_float(1u)) : __uint_as_float(__float_as_uint(r) + 1u);
    v.rres[(size_t)t * 64 + lane] = up;
}
// The 8-bit plane of tiles [t0, t0 + n_tiles) and its row state (qv_bound.h: bound8_scale / bound8_quant / bound8_row_res): plane8 is
// [tile][16-dim step][64 rows][16 values] — lane == row, one dwordx4 per lane and step, a wave's request one contiguous KiB, as for the
// float32 tiles.  One wave per tile, two walks of the tile: the row's largest magnitude (and whether it has one), then the bytes and
// the residual |r - scale r8| FROM THE BYTES WRITTEN, in float64, rounded up.  dim is a multiple of 16 (the index keeps no plane otherwise).
__global__ void __launch_bounds__(64)
k_row_state8(IndexView v, uint32_t t0, const uint32_t* __restrict__ list) {
    const uint32_t t = list ? list[blockIdx.x] : t0 + blockIdx.x, lane = threadIdx.x, steps = v.dim >> 4;
    const f4* src = reinterpret_cast<const f4*>(v.tiles) + (size_t)t * v.dim4 * 64 + lane;
    float maxabs = 0.f; bool bad = false; double n2 = 0.0;
    for (uint32_t c = 0; c < v.dim4; c++) {
        const f4 x = src[(size_t)c * 64];
        const float e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            bad |= !((e[j] - e[j]) == 0.0f);
            maxabs = __builtin_fmaxf(maxabs, __builtin_fabsf(e[j]));
            n2 = __builtin_fma((double)e[j], (double)e[j], n2);
        }
    }
    const float scale = bad ? 0.0f : bound8_scale(maxabs);
    const float div = scale > 0.0f ? scale : 1.0f;
    double s2 = 0.0;
    uint4* dst = reinterpret_cast<uint4*>(v.plane8) + (size_t)t * steps * 64 + lane;
    for (uint32_t s = 0; s < steps; s++) {
        uint32_t w[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const f4 x = src[(size_t)(4 * s + c) * 64];
            const float e[4] = {x.x, x.y, x.z, x.w};
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int b = scale > 0.0f ? bound8_quant(e[j], div) : 0;
                const double d = (double)e[j] - (double)scale * (double)b;
                s2 = __builtin_fma(d, d, s2);
                word |= ((uint32_t)b & 0xFFu) << (8 * j);
            }
            w[c] = word;
        }
        uint4 o; o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
        dst[(size_t)s * 64] = o;
    }
    v.rscale8[(size_t)t * 64 + lane] = scale;
    v.rres8[(size_t)t * 64 + lane] = bound8_row_res(bad, maxabs, n2, s2, v.dim);
}
// The 6-bit plane of tiles [t0, t0 + n_tiles) and its residual (qv_bound.h: bound6_quant, bound6_pack's layout): launched behind k_row_state8,
// whose scale it reads.  One wave per tile, lane == row: per group of 64 dimensions the lane's three 16-byte pieces X, Y, Z, each a
// contiguous KiB of the wave; rres6 = |r - 4 rscale8 c6| from the codes written, in float64, rounded up; a row the 8-bit state declines
// (rres8 is NaN) is declined here.  dim is a multiple of 64 (the index keeps no 6-bit plane otherwise).
__global__ void __launch_bounds__(64)
k_row_state6(IndexView v, uint32_t t0, const uint32_t* __restrict__ list) {
    const uint32_t t = list ? list[blockIdx.x] : t0 + blockIdx.x, lane = threadIdx.x, groups = v.dim >> 6;
    const f4* src = reinterpret_cast<const f4*>(v.tiles) + (size_t)t * v.dim4 * 64 + lane;
    const float scale = v.rscale8[(size_t)t * 64 + lane];
    const float res8 = v.rres8[(size_t)t * 64 + lane];
    const float div = scale > 0.0f ? scale : 1.0f;
    const double step = 4.0 * (double)scale;
    double s2 = 0.0;
    uint4* dst = reinterpret_cast<uint4*>(v.plane6) + (size_t)t * groups * 3 * 64 + lane;
    for (uint32_t g = 0; g < groups; g++) {
        uint32_t w[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
        for (int c = 0; c < 16; c++) {                                 // chunk c: dims 4 c .. 4 c + 3 of the group
            const f4 x = src[(size_t)(16 * g + c) * 64];
            const float e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int q = scale > 0.0f ? bound6_quant(e[j], div) : 0;
                const double d = (double)e[j] - step * (double)q;
                s2 = __builtin_fma(d, d, s2);
                const uint32_t u = (uint32_t)(q + kBound6Bias);
                if (c < 12) w[c >> 2][c & 3] |= u << (8 * j);
                else {
                    w[0][c - 12] |= (u & 3u) << (8 * j + 6);
                    w[1][c - 12] |= ((u >> 2) & 3u) << (8 * j + 6);
                    w[2][c - 12] |= ((u >> 4) & 3u) << (8 * j + 6);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            uint4 o; o.x = w[c][0]; o.y = w[c][1]; o.z = w[c][2]; o.w = w[c][3];
            dst[((size_t)g * 3 + c) * 64] = o;
        }
    }
    v.rres6[(size_t)t * 64 + lane] = res8 == res8 ? bound8_res_up(s2) : __builtin_nanf("");
}
// The row-order bfloat16 copy (QV_FLAG_GRAPH_PLANE) of the rows of tiles [t0, t0 + n_tiles): rowmaj16[row][e] = (__bf16)row[e], round to nearest
// even — the very conversion k_row_residual measures, from the same tiles, so rres[row] >= |r - rh| holds for the image a graph hop reads.
// One thread per (row, chunk of four elements), the chunk index fastest: a row's 2 * dim bytes are written contiguously.  Whole tiles are
// written (the storage is whole tiles; slots past the last row hold the zero rows the tiles hold).
__global__ void __launch_bounds__(256)
k_rowmaj16(IndexView v, uint32_t t0, uint32_t n_tiles, const uint32_t* __restrict__ list) {
    typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
    const uint64_t total = (uint64_t)n_tiles * 64 * v.dim4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t c = (uint32_t)(i % v.dim4);
        const uint64_t rr = i / v.dim4;
        const uint32_t r = (uint32_t)(rr & 63), ti = (uint32_t)(rr >> 6), t = list ? list[ti] : t0 + ti;
        const f4 a = reinterpret_cast<const f4*>(v.tiles)[((size_t)t * v.dim4 + c) * 64 + r];
        const bf2 p0 = {(__bf16)a.x, (__bf16)a.y}, p1 = {(__bf16)a.z, (__bf16)a.w};
        uint2 o; o.x = __builtin_bit_cast(uint32_t, p0); o.y = __builtin_bit_cast(uint32_t, p1);
        reinterpret_cast<uint2*>(v.rowmaj16 + ((size_t)t * 64 + r) * v.dim)[c] = o;      // (dim is a multiple of 64 here: dim == 4 * dim4)
    }
}
// The row-order 8-bit image (QV_FLAG_GRAPH_PLANE8) of the rows of tiles [t0, t0 + n_tiles) and its records: k_row_state8's quantiser, statement
// for statement — the scale from the row's largest magnitude, the bytes, the residual in float64 FROM THE BYTES WRITTEN — so the bytes, the
// scale and the residual are the tile plane's bit for bit where the index keeps one, and the image needs none.  One wave per tile, lane == row:
// the tile is read as the planes read it, and a lane writes its row's 16 bytes per step to rowmaj8[row][16 s ..).  The record's norm is the
// one the ingest kernel ahead on the stream left in v.rnorm.  Whole tiles are written, as k_rowmaj16 does.  dim is a multiple of 128 here.
__global__ void __launch_bounds__(64)
k_rowmaj8(IndexView v, uint32_t t0, const uint32_t* __restrict__ list) {
    const uint32_t t = list ? list[blockIdx.x] : t0 + blockIdx.x, lane = threadIdx.x, steps = v.dim >> 4;
    const f4* src = reinterpret_cast<const f4*>(v.tiles) + (size_t)t * v.dim4 * 64 + lane;
    float maxabs = 0.f; bool bad = false; double n2 = 0.0;
    for (uint32_t c = 0; c < v.dim4; c++) {
        const f4 x = src[(size_t)c * 64];
        const float e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            bad |= !((e[j] - e[j]) == 0.0f);
            maxabs = __builtin_fmaxf(maxabs, __builtin_fabsf(e[j]));
            n2 = __builtin_fma((double)e[j], (double)e[j], n2);
        }
    }
    const float scale = bad ? 0.0f : bound8_scale(maxabs);
    const float div = scale > 0.0f ? scale : 1.0f;
    double s2 = 0.0;
    const size_t row = (size_t)t * 64 + lane;
    uint4* dst = reinterpret_cast<uint4*>(v.rowmaj8 + row * v.dim);
    for (uint32_t s = 0; s < steps; s++) {
        uint32_t w[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const f4 x = src[(size_t)(4 * s + c) * 64];
            const float e[4] = {x.x, x.y, x.z, x.w};
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int b = scale > 0.0f ? bound8_quant(e[j], div) : 0;
                const double d = (double)e[j] - (double)scale * (double)b;
                s2 = __builtin_fma(d, d, s2);
                word |= ((uint32_t)b & 0xFFu) << (8 * j);
            }
            w[c] = word;
        }
        uint4 o; o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
        dst[s] = o;
    }
    RowMeta8 m; m.rnorm = v.rnorm[row]; m.rscale8 = scale; m.rres8 = bound8_row_res(bad, maxabs, n2, s2, v.dim);
    v.rowmeta8[row] = m;
}
// The derived planes of n_tiles tiles, behind every write of rows and on its stream: the range [t0, t0 + n_tiles) when list is null, the
// tiles list[0 .. n_tiles) (device memory, distinct) otherwise.  One body per plane either way: a tile is derived the same whoever asks.
static hipError_t refresh_bf16(const IndexView& v, uint32_t t0, uint32_t n_tiles, const uint32_t* list, hipStream_t s) {
    if (v.rowmaj16) {                                                  // (never behind the rows either)
        const uint64_t total = (uint64_t)n_tiles * 64 * v.dim4;
        hipLaunchKernelGGL(k_rowmaj16, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, 65536)), dim3(256), 0, s, v, t0, n_tiles, list);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (v.rowmaj8 && v.rowmeta8) {                                     // (nor the 8-bit image and its records)
        hipLaunchKernelGGL(k_rowmaj8, dim3(n_tiles), dim3(64), 0, s, v, t0, list);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (v.rres && (v.metric == QV_COSINE || v.metric == QV_DOT || v.metric == QV_L2 || v.metric == QV_L2SQ)) {
        hipLaunchKernelGGL(k_row_residual, dim3(n_tiles), dim3(64), 0, s, v, t0, list);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (v.plane8) {                                                    // (the 8-bit plane and its row state: never behind the tiles either)
        hipLaunchKernelGGL(k_row_state8, dim3(n_tiles), dim3(64), 0, s, v, t0, list);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (v.plane6) {                                                // (behind it: the scale is the 8-bit plane's)
            hipLaunchKernelGGL(k_row_state6, dim3(n_tiles), dim3(64), 0, s, v, t0, list);
            e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    if (!v.plane) return hipSuccess;
    const uint64_t total = (uint64_t)n_tiles * ((v.dim4 + 1) / 2) * 64;
    hipLaunchKernelGGL(k_bf16_plane, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, 65536)), dim3(256), 0, s, v, t0, n_tiles, list);
    return hipGetLastError();
}

hipError_t launch_ingest(const IndexView& v, const float* d_rows, uint32_t row0, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t t0 = row0 / 64, t1 = (row0 + n - 1) / 64;
    static const int tiled = dev_env_int("QV_INGEST_TILED", 1);
    if ((v.dim & 3) == 0 && tiled == 1 && (reinterpret_cast<uintptr_t>(d_rows) & 15) == 0) {
        hipLaunchKernelGGL(k_ingest_tiled, dim3(t1 - t0 + 1), dim3(256), 0, s, v, d_rows, row0, n, t0);
        hipError_t e0 = hipGetLastError();
        return e0 != hipSuccess ? e0 : refresh_bf16(v, t0, t1 - t0 + 1, nullptr, s);
    }
    hipLaunchKernelGGL(k_ingest, dim3(t1 - t0 + 1), dim3(64), 0, s, v, d_rows, row0, n, t0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (v.rowmaj) e = hipMemcpyAsync(v.rowmaj + (size_t)row0 * v.dim, d_rows, (size_t)n * v.dim * sizeof(float), hipMemcpyDeviceToDevice, s);
    return e != hipSuccess ? e : refresh_bf16(v, t0, t1 - t0 + 1, nullptr, s);
}

hipError_t launch_update_rows(const IndexView& v, const float* d_vecs, const uint32_t* d_rows_sorted, const uint32_t* d_src,
                              const uint32_t* d_tile_first, const uint32_t* d_tiles, uint32_t n_unique, uint32_t n_tiles, hipStream_t s) {
    if (n_unique == 0 || n_tiles == 0) return hipSuccess;
    static const int tiled = dev_env_int("QV_INGEST_TILED", 1);
    if ((v.dim & 3) == 0 && tiled == 1 && (reinterpret_cast<uintptr_t>(d_vecs) & 15) == 0)
        hipLaunchKernelGGL(k_update_rows_tiled, dim3(n_tiles), dim3(256), 0, s, v, d_vecs, d_rows_sorted, d_src, d_tile_first, d_tiles);
    else
        hipLaunchKernelGGL(k_update_rows, dim3(n_tiles), dim3(64), 0, s, v, d_vecs, d_rows_sorted, d_src, d_tile_first, d_tiles);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : refresh_bf16(v, 0, n_tiles, d_tiles, s);
}

hipError_t launch_generate(const IndexView& v, uint64_t seed, uint64_t gen_row0, uint32_t row0, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t t0 = row0 / 64, t1 = (row0 + n - 1) / 64;
    hipLaunchKernelGGL(k_generate, dim3(t1 - t0 + 1), dim3(64), 0, s, v, seed, gen_row0, row0, n, t0);
    hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : refresh_bf16(v, t0, t1 - t0 + 1, nullptr, s);
}

hipError_t launch_set_alive(const IndexView& v, const uint32_t* d_rows, uint32_t n, int alive, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_set_alive, dim3((n + 255) / 256), dim3(256), 0, s, v, d_rows, n, alive);
    return hipGetLastError();
}

// n listed rows -> row-major [n][dim]: blockIdx.y = listed row, one thread per element (a row's elements sit 64 floats apart in
// its tile: a gather by nature; this is the Save / GetVector path, not a scan)
__global__ void k_fetch_rows(IndexView v, const uint32_t* __restrict__ rows, float* __restrict__ out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= v.dim) return;
    const uint32_t row = rows[blockIdx.y];
    out[(size_t)blockIdx.y * v.dim + j] = v.tiles[((size_t)(row >> 6) * v.dim4 + (j >> 2)) * 256 + (row & 63) * 4 + (j & 3)];
}

hipError_t launch_fetch_rows(const IndexView& v, const uint32_t* d_rows, uint32_t n, float* d_out, hipStream_t s) {
    for (uint32_t done = 0; done < n; done += 65535) {                    // gridDim.y limit
        const uint32_t m = n - done < 65535 ? n - done : 65535;
        hipLaunchKernelGGL(k_fetch_rows, dim3((v.dim + 255) / 256, m), dim3(256), 0, s, v, d_rows + done, d_out + (size_t)done * v.dim);
    }
    return hipGetLastError();
}

hipError_t launch_fetch_row(const IndexView& v, uint32_t row, float* d_out, hipStream_t s) {
    hipLaunchKernelGGL(k_fetch_row, dim3((v.dim + 255) / 256), dim3(256), 0, s, v, row, d_out);
    return hipGetLastError();
}


}  // namespace qv
