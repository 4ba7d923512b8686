// qv_batched_sets.hip — what a FILTERED batch (a row set per query, launch_batched with BatchedSets) adds to the batched path.
//
// The batched path answers 9 or more queries with a sample bound, one matrix-core filter pass over the corpus and an exact re-score of the
// candidates.  Under a filter, query q ranks live & set_q only.  Three things make that true, and nothing else changes:
//   1. the bound.  The sample's score kernels write one upper bound per (query, sample row), +inf for dead rows.  k_sets_sample_mask
//      runs between them and the selection and sets bounds[q][i] = +inf for sample rows outside set_q: the selection then yields the
//      ks-th smallest upper bound over sample & live & set_q — a bound of the k-th distance over live & set_q, as any subset's is.  A
//      query with fewer than ks such rows gets +inf (everything in its set is a candidate: it is answered from them, or overflows).
//   2. the candidates.  cand_flush (qv_filter.h) drops a record whose row is outside its query's set; the table's address travels in
//      front of the counters, written by k_mfma_prep.
//   3. sparse sets.  The filter kernels test every row against every query's threshold whatever the sets say, and a threshold taken over
//      a set that holds a share s of the rows lets about 1/s as many rows of the WHOLE corpus into the wave queues — records that the
//      flush then drops.  Below a share of sparse_ppm millionths (counted here, on the sample) that work outgrows the exact row-set
//      scan's: k_sets_sparse gives such a query the padded queries' constants (+inf threshold, nothing passes) and flags it for the
//      host's redo.  A mis-route costs time, never bits.
#include "qv_kernels.h"

namespace qv {

// Sample position -> corpus row, as the sample's score kernels walk (k_bf16x3_filter, k_bf16x1_filter_w8 with a score output): position i
// lies in the sample's 128-row group i / 128, which is group (i / 128) * gstep of the corpus — tiles 2 ga and 2 ga + 1, the second one
// clamped to the first where the corpus ends on an odd tile (those 64 positions then belong to no row: the score kernels skip them).
// tile: the 64-row tile of sample tile st (two per group); false: the positions of st are no rows.
__device__ __forceinline__ bool sample_tile_of(uint32_t st, uint32_t gstep, uint32_t n_tiles, uint32_t& tile) {
    const uint32_t ga = (st >> 1) * gstep;
    tile = 2 * ga + (st & 1u);
    return tile < n_tiles;
}

// grid (ceil(sample tiles / 4), nq), 256 threads: a wave per (query, 64 sample positions).  Reads the set's and the alive word of the
// positions' tile once (wave-uniform), writes +inf over the bounds of positions outside the set — a dense set writes nothing — and adds
// the positions that are live and in the set to n_in[q] (zeroed by the launcher).
__global__ void __launch_bounds__(256)
k_sets_sample_mask(const uint64_t* __restrict__ alive, uint32_t n_tiles, const RowSetRef* __restrict__ sets, float* __restrict__ bounds,
                   uint32_t sample_rows, uint32_t gstep, uint32_t* __restrict__ n_in) {
    const uint32_t lane = lane_id();
    const uint32_t q = blockIdx.y;
    const uint32_t st = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (st * 64 >= sample_rows) return;                              // (wave-uniform)
    const uint32_t pos = st * 64 + lane;
    const bool valid = pos < sample_rows;
    uint32_t tile;
    uint64_t in = 0ull, live = 0ull;
    if (sample_tile_of(st, gstep, n_tiles, tile)) {
        const RowSetRef rs = sets[q];
        live = alive[tile];
        in = rs.bits == nullptr ? ~0ull : (tile < rs.words ? rs.bits[tile] : 0ull);
    }
    if (valid && !((in >> lane) & 1ull)) bounds[(size_t)q * sample_rows + pos] = __builtin_inff();
    const uint32_t n_valid = sample_rows - st * 64 < 64 ? sample_rows - st * 64 : 64u;
    const uint64_t vmask = n_valid == 64 ? ~0ull : ((1ull << n_valid) - 1ull);
    const uint32_t n = (uint32_t)__builtin_popcountll(in & live & vmask);
    if (lane == 0 && n) atomicAdd(&n_in[q], n);
}

// one thread per query, behind k_mfma_prep: sparse[q] = the set holds fewer than sparse_ppm millionths of the sample's rows (0: never).
// A sparse query takes the padded queries' constants — c = +inf: no row passes its threshold, its candidate list stays empty, its
// outputs are padding — and is flagged for the redo.
__global__ void __launch_bounds__(256)
k_sets_sparse(uint32_t nq, uint32_t nq_pad, const uint32_t* __restrict__ n_in, uint32_t sample_rows, uint32_t sparse_ppm,
              float* __restrict__ cq, float* __restrict__ mq, uint32_t* __restrict__ ovf, uint32_t* __restrict__ sparse) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const bool sp = sparse_ppm != 0 && (uint64_t)n_in[q] * 1000000ull < (uint64_t)sparse_ppm * sample_rows;
    sparse[q] = sp ? 1u : 0u;
    if (sp) {
        cq[q] = __builtin_inff(); mq[q] = 0.f; mq[nq_pad + q] = 0.f;
        ovf[q] = 1u;
    }
}

hipError_t launch_sets_sample_mask(const IndexView& v, const RowSetRef* d_sets, uint32_t nq, float* d_bounds, uint32_t sample_rows, uint32_t gstep,
                                   uint32_t* d_n_in, hipStream_t s) {
    if (!d_sets || nq == 0 || sample_rows == 0 || gstep == 0) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(d_n_in, 0, (size_t)nq * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const uint32_t stiles = (sample_rows + 63) / 64;
    hipLaunchKernelGGL(k_sets_sample_mask, dim3((stiles + 3) / 4, nq), dim3(256), 0, s, v.alive, v.n_tiles, d_sets, d_bounds, sample_rows, gstep, d_n_in);
    return hipGetLastError();
}

hipError_t launch_sets_sparse(uint32_t nq, uint32_t nq_pad, const uint32_t* d_n_in, uint32_t sample_rows, uint32_t sparse_ppm, float* d_cq, float* d_mq,
                              uint32_t* d_ovf, uint32_t* d_sparse, hipStream_t s) {
    hipLaunchKernelGGL(k_sets_sparse, dim3((nq + 255) / 256), dim3(256), 0, s, nq, nq_pad, d_n_in, sample_rows, sparse_ppm, d_cq, d_mq, d_ovf, d_sparse);
    return hipGetLastError();
}

}  // namespace qv
