// qv_graph_remove.hip — device-resident HNSW graphs edited in place: hnsw.HNSW.Delete for a list of nodes, and the
// gather behind qv_graph_export_lists (shared helpers: qv_kernels.h; the sort and the segment heads are the build's)
//
// What it replaces: the loop of Delete over the deleted node's lists (pkg/hnsw/hnsw.go:761-790).  For every level l of the
// deleted node d and every x in conn_d[l] that is non-nil, every occurrence of d leaves conn_x[l] and the rest keeps its
// order.  Links to d from nodes that d does not list stay (the reference leaves them; the traversals skip dead nodes).
//
// A list of nodes is deleted "as if one by one in list order".  The only thing the order decides for the lists is which x
// are still non-nil when d's turn comes: those not deleted EARLIER in the same call.  d's own list as it stands at its turn
// differs from the list before the call only by nodes deleted earlier, which that test skips anyway, so every (d, l) pair
// reads the lists as they were before the call and the whole edit runs in parallel:
//   k_remove_emit     one wavefront per (listed node d, level l): a 64-bit key (target list << 32 | d) per neighbour that is
//                     live at d's turn (the listed nodes, sorted, carry their place in the list: a binary search per lane)
//   stable radix sort of the keys by target list (qv_rank.hip) -> k_build_heads (qv_build.hip): one segment per target list
//   k_remove_compact  one wavefront per target list: the list in its lanes, the lanes equal to any incoming d marked, links,
//                     per-link distances (what k_build_merge ranks by at the next prune) and degree written back
//                     ballot-compacted
//   k_remove_tombstone level[d] = -1
// The entry-point chain (hnsw.go:796-827) is a handful of list reads between the compaction and the tombstones: the host's
// (qv_graph_api.cpp), through k_export_lists.
#include "qv_kernels.h"

namespace qv {

namespace {

constexpr uint32_t kNoRank = 0xFFFFFFFFu;

// the place in the call's list of node x (kNoRank: not listed); snode ascending
__device__ __forceinline__ uint32_t rank_of(const uint32_t* __restrict__ snode, const uint32_t* __restrict__ srank, uint32_t m, uint32_t x) {
    uint32_t lo = 0, hi = m;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (snode[mid] < x) lo = mid + 1; else hi = mid; }
    return lo < m && snode[lo] == x ? srank[lo] : kNoRank;
}

}  // namespace

// work: [3][n_work] node, level, place in the list.  keys: [n_work][stride], dead where there is nothing to remove.
__global__ void __launch_bounds__(64)
k_remove_emit(BuildView b, uint32_t n_nodes, const uint32_t* __restrict__ work, uint32_t n_work, const uint32_t* __restrict__ snode,
              const uint32_t* __restrict__ srank, uint32_t m, uint32_t stride, uint64_t* __restrict__ keys) {
    const uint32_t w = blockIdx.x, lane = threadIdx.x;
    if (w >= n_work) return;
    const uint32_t d = work[w], rk = work[(size_t)2 * n_work + w];
    const int l = (int)work[(size_t)n_work + w];
    uint32_t deg, cap; const uint32_t* links;
    if (l == 0) { deg = b.l0_deg[d]; links = b.l0_links + (size_t)d * b.max_m0; cap = b.max_m0; }
    else { const uint32_t* blk = b.up_links + (size_t)(b.up_off[d] + (uint32_t)(l - 1)) * (1 + b.max_m); deg = blk[0]; links = blk + 1; cap = b.max_m; }
    if (deg > cap) deg = cap;
    uint64_t key = kDeadKey;
    if (lane < deg) {
        const uint32_t x = links[lane];
        // :769-771 non-nil when d's turn comes (d itself included: the self-links of k_build_link), :777 and the list exists
        if (x < n_nodes && (int)b.level[x] >= l && rank_of(snode, srank, m, x) >= rk) {
            const uint32_t lid = l == 0 ? x : b.cap_nodes + b.up_off[x] + (uint32_t)(l - 1);
            key = ((uint64_t)lid << 32) | (uint64_t)d;
        }
    }
    if (lane < stride) keys[(size_t)w * stride + lane] = key;
}

// one wavefront per target list (a segment of the sorted keys): drop every occurrence of the segment's nodes, keep the order
__global__ void __launch_bounds__(64)
k_remove_compact(BuildView b, const uint64_t* __restrict__ keys, uint32_t n_keys, const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_n) {
    const uint32_t lane = threadIdx.x;
    const uint32_t ns = *seg_n;
    for (uint32_t s = blockIdx.x; s < ns; s += gridDim.x) {
        const uint32_t i0 = seg_start[s];
        const uint32_t lid = (uint32_t)(keys[i0] >> 32);
        uint32_t* degp; uint32_t* linkp; float* distp; uint32_t cap;
        if (lid < b.cap_nodes) { degp = b.l0_deg + lid; linkp = b.l0_links + (size_t)lid * b.max_m0; distp = b.l0_dist + (size_t)lid * b.max_m0; cap = b.max_m0; }
        else { const uint32_t blk = lid - b.cap_nodes; degp = b.up_links + (size_t)blk * (1 + b.max_m); linkp = degp + 1; distp = b.up_dist + (size_t)blk * b.max_m; cap = b.max_m; }
        uint32_t len = *degp;
        if (len > cap) len = cap;
        const uint32_t mine = lane < len ? linkp[lane] : 0xFFFFFFFFu;
        const float md = lane < len ? distp[lane] : 0.0f;
        bool keep = lane < len;
        for (uint32_t e = i0; e < n_keys; e++) {
            const uint64_t ke = keys[e];
            if ((uint32_t)(ke >> 32) != lid) break;
            if (mine == (uint32_t)ke) keep = false;                       // :780-784
        }
        const uint64_t km = __ballot(keep);
        const uint32_t pos = (uint32_t)__builtin_popcountll(km & ((1ull << lane) - 1));
        if (keep) { linkp[pos] = mine; distp[pos] = md; }                 // (pos <= lane: every lane read its entry above)
        if (lane == 0) *degp = (uint32_t)__builtin_popcountll(km);
    }
}

// ONE deleted node (what a host's Delete sends): no keys, no sort.  One wavefront per (level l, place j) of d's lists; the
// neighbour x found there loses its links to d.  Only the first mention of x in the list acts (two wavefronts must not compact one
// list), and d itself is left out: its own lists are not written while the others read them (the host's entry-point chain drops d
// from them as it reads; nothing else reads a dead node's lists).
__global__ void __launch_bounds__(64)
k_remove_one(BuildView b, uint32_t n_nodes, uint32_t d, int lv, uint32_t stride) {
    const uint32_t lane = threadIdx.x;
    const int l = (int)(blockIdx.x / stride);
    const uint32_t j = blockIdx.x % stride;
    if (l > lv) return;
    uint32_t deg, cap; const uint32_t* links;
    if (l == 0) { deg = b.l0_deg[d]; links = b.l0_links + (size_t)d * b.max_m0; cap = b.max_m0; }
    else { const uint32_t* blk = b.up_links + (size_t)(b.up_off[d] + (uint32_t)(l - 1)) * (1 + b.max_m); deg = blk[0]; links = blk + 1; cap = b.max_m; }
    if (deg > cap) deg = cap;
    if (j >= deg) return;
    const uint32_t x = links[j];
    if (x == d || x >= n_nodes || (int)b.level[x] < l) return;            // :769-771, :777
    if (__ballot(lane < j && links[lane] == x)) return;                  // an earlier place names x already
    uint32_t* degp; uint32_t* linkp; float* distp; uint32_t capx;
    if (l == 0) { degp = b.l0_deg + x; linkp = b.l0_links + (size_t)x * b.max_m0; distp = b.l0_dist + (size_t)x * b.max_m0; capx = b.max_m0; }
    else { const uint32_t blk = b.up_off[x] + (uint32_t)(l - 1); degp = b.up_links + (size_t)blk * (1 + b.max_m); linkp = degp + 1; distp = b.up_dist + (size_t)blk * b.max_m; capx = b.max_m; }
    uint32_t len = *degp;
    if (len > capx) len = capx;
    const uint32_t mine = lane < len ? linkp[lane] : 0xFFFFFFFFu;
    const float md = lane < len ? distp[lane] : 0.0f;
    const bool keep = lane < len && mine != d;                           // :780-784
    const uint64_t km = __ballot(keep);
    if (km == __ballot(lane < len)) return;                              // d is not in the list (a one-way link): nothing to write
    const uint32_t pos = (uint32_t)__builtin_popcountll(km & ((1ull << lane) - 1));
    if (keep) { linkp[pos] = mine; distp[pos] = md; }
    if (lane == 0) *degp = (uint32_t)__builtin_popcountll(km);
}

__global__ void k_remove_tombstone_one(int8_t* __restrict__ level, uint32_t d) {
    if (blockIdx.x == 0 && threadIdx.x == 0) level[d] = (int8_t)-1;      // :832
}

__global__ void k_remove_tombstone(int8_t* __restrict__ level, const uint32_t* __restrict__ snode, uint32_t m) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) level[snode[i]] = (int8_t)-1;                              // :832
}

// one wavefront per requested (node, level): degree and links [stride]; a dead node or a level the node does not have: degree 0
__global__ void __launch_bounds__(64)
k_export_lists(GraphView g, const uint32_t* __restrict__ nodes, const int* __restrict__ levels, uint32_t n, uint32_t stride,
               uint32_t* __restrict__ deg_out, uint32_t* __restrict__ links_out) {
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const uint32_t nd = nodes[i];
    const int l = levels[i];
    uint32_t deg = 0; const uint32_t* links = nullptr;
    if (nd < g.n_nodes && l >= 0 && l <= (int)g.level[nd]) {
        if (l == 0) { deg = g.l0_deg[nd]; if (deg > g.max_m0) deg = g.max_m0; links = g.l0_links + (size_t)nd * g.max_m0; }
        else { const uint32_t* blk = g.up_links + (size_t)(g.up_off[nd] + (uint32_t)(l - 1)) * (1 + g.max_m); deg = blk[0]; if (deg > g.max_m) deg = g.max_m; links = blk + 1; }
    }
    if (lane < stride) links_out[(size_t)i * stride + lane] = lane < deg ? links[lane] : 0u;
    if (lane == 0) deg_out[i] = deg;
}

hipError_t launch_graph_remove(const BuildView& b, uint32_t n_nodes, const uint32_t* d_work, uint32_t n_work, const uint32_t* d_snode,
                               const uint32_t* d_srank, uint32_t m, uint64_t* d_keys_a, uint64_t* d_keys_b, uint32_t* d_hist,
                               uint32_t* d_seg_start, uint32_t* d_seg_n, uint32_t grid, hipStream_t s) {
    if (m == 0) return hipSuccess;
    const uint32_t stride = b.max_m0 > b.max_m ? b.max_m0 : b.max_m;
    if (n_work) {
        const uint32_t nk = n_work * stride;
        hipLaunchKernelGGL(k_remove_emit, dim3(n_work), dim3(64), 0, s, b, n_nodes, d_work, n_work, d_snode, d_srank, m, stride, d_keys_a);
        uint64_t* sorted = nullptr;
        hipError_t e = launch_radix_sort_hi32(d_keys_a, d_keys_b, nk, d_hist, &sorted, s);
        if (e != hipSuccess) return e;
        e = launch_build_heads(sorted, nk, d_seg_start, d_seg_n, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_remove_compact, dim3(std::min(grid, nk)), dim3(64), 0, s, b, sorted, nk, d_seg_start, d_seg_n);
    }
    return hipGetLastError();
}

hipError_t launch_graph_remove_one(const BuildView& b, uint32_t n_nodes, uint32_t d, int level, hipStream_t s) {
    const uint32_t stride = b.max_m0 > b.max_m ? b.max_m0 : b.max_m;
    hipLaunchKernelGGL(k_remove_one, dim3(((uint32_t)level + 1) * stride), dim3(64), 0, s, b, n_nodes, d, level, stride);
    return hipGetLastError();
}

hipError_t launch_graph_tombstone_one(int8_t* d_level, uint32_t d, hipStream_t s) {
    hipLaunchKernelGGL(k_remove_tombstone_one, dim3(1), dim3(64), 0, s, d_level, d);
    return hipGetLastError();
}

hipError_t launch_graph_tombstone(int8_t* d_level, const uint32_t* d_snode, uint32_t m, hipStream_t s) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_remove_tombstone, dim3((m + 255) / 256), dim3(256), 0, s, d_level, d_snode, m);
    return hipGetLastError();
}

hipError_t launch_export_lists(const GraphView& g, const uint32_t* d_nodes, const int* d_levels, uint32_t n, uint32_t* d_deg_out,
                               uint32_t* d_links_out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t stride = g.max_m0 > g.max_m ? g.max_m0 : g.max_m;
    hipLaunchKernelGGL(k_export_lists, dim3(n), dim3(64), 0, s, g, d_nodes, d_levels, n, stride, d_deg_out, d_links_out);
    return hipGetLastError();
}

}  // namespace qv
