// qv_api_internal.h — shared by the C-ABI translation units (qv_api.cpp: indexes; qv_graph_api.cpp: HNSW graphs;
// qv_sharded_api.cpp: multi-GPU shards).  Not installed.
#pragma once
#include "../../include/qv.h"
#include "qv_device.h"
#include "qv_coalesce.h"

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <chrono>
#include <mutex>
#include <new>
#include <vector>

int qv_fail(int code, const char* fmt, ...);      // sets the thread-local message, returns code
#define fail qv_fail

#define HIPCHK(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(e_ == hipErrorOutOfMemory ? QV_ERR_OOM : QV_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

struct Buf {            // growable device buffer
    void* p = nullptr; size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return QV_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = std::max(bytes, (size_t)4096);
        HIPCHK(hipMalloc(&p, want));
        cap = want; return QV_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};
struct PinBuf {         // growable pinned host buffer
    void* p = nullptr; size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return QV_OK;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        size_t want = std::max(bytes, (size_t)4096);
        // coherent (fine-grained): a kernel's stores are visible to the host while the kernel is still running — the single-launch
        // small scan writes its results and then a sequence number here, and the host polls that instead of waiting for the stream
        HIPCHK(hipHostMalloc(&p, want, hipHostMallocCoherent));
        cap = want; return QV_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

struct Workspace { Buf ws; Buf tickets; std::mutex mu; };      // tickets: 64 zeroed words of the single-launch small scan (k_flat_scan_small)

// qv_api.cpp, for qv_sharded_api.cpp: exact scan over the rows of a device-resident candidate bitmap (see the definition)
int qv_internal_search_candidates_device(qv_index* idx, const float* d_queries, uint32_t nq, uint32_t k_stride, const uint64_t* d_candidates,
                                         uint64_t matching, uint32_t* d_rows_out, float* d_dist_out, void* stream);

// qv_api.cpp, for qv_sharded_api.cpp: the exact scan for the flagged queries of a batch, decided on the device (see the definition)
int qv_internal_redo_flagged_device(qv_index* idx, const float* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_flags,
                                    uint32_t* d_rows_out, float* d_dist_out, void* stream);

// qv_api.cpp, for qv_sharded_api.cpp: forget (and free) the workspace the *_device entry points keep for `stream` — called when a
// call context of the sharded handle, and with it the stream, goes away
void qv_internal_drop_stream_workspace(qv_index* idx, void* stream);

struct SearchCtx {
    hipStream_t stream = nullptr;
    Buf d_q, d_rows, d_dist, d_ids, d_mask, ws, tickets;
    PinBuf h_q, h_rows, h_dist, h_ids, h_mask, h_flag;
    Buf d_where, d_lits; PinBuf h_lits;      // qv_index_search_where: the call's transient sets, and its literals when they do not fit the kernel arguments
    Buf d_sets; PinBuf h_sets;               // a filtered batch: the call's RowSetRef table, staged from pinned memory on the call's stream
    uint32_t flag_seq = 0;                   // sequence number the small scan writes into h_flag when its results are in h_rows / h_dist
    void release() {
        d_q.release(); d_rows.release(); d_dist.release(); d_ids.release(); d_mask.release(); ws.release(); tickets.release();
        d_where.release(); d_lits.release(); h_lits.release();
        d_sets.release(); h_sets.release();
        h_q.release(); h_rows.release(); h_dist.release(); h_ids.release(); h_mask.release(); h_flag.release();
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
    }
};


struct qv_index {
    int device = 0;
    int cus = 256;
    uint32_t dim = 0, dim4 = 0;
    int metric = QV_COSINE;
    uint64_t flags = 0;
    int filter = 0;                            // qv_index_set_filter
    uint32_t n_rows = 0, n_live = 0;
    uint64_t row_writes = 0;                   // bumped by every call that writes row CONTENTS (add / update): copies kept elsewhere (a graph's hubs) compare it
    uint64_t cap_tiles = 0;
    float* d_tiles = nullptr;
    double* d_rnorm = nullptr;
    uint64_t* d_alive = nullptr;
    float* d_rres = nullptr;                   // |r - bf16(r)| per row: refreshed by every call that writes rows
    float* d_rowmaj = nullptr;
    uint16_t* d_rowmaj16 = nullptr;            // the row-order bfloat16 copy (QV_FLAG_GRAPH_PLANE): written wherever d_rowmaj is
    bool rowmaj16_lost = false;                // it could not be allocated: the index carries on without it
    int8_t* d_rowmaj8 = nullptr;               // the row-order 8-bit image (QV_FLAG_GRAPH_PLANE8) and its 16-byte record per row: written wherever d_rowmaj is
    qv::RowMeta8* d_rowmeta8 = nullptr;
    bool rowmaj8_lost = false;                 // it could not be allocated: the index carries on without it
    uint16_t* d_bf16 = nullptr;                // the bfloat16 copy (QV_FLAG_BF16_ROWS, and by default on cosine / dot indexes): refreshed by every call that writes rows
    bool plane_lost = false;                   // the default copy could not be allocated: the index carries on without it
    qv::BoundKnobs bound = {};                 // qv_index_set_bound_scan, and by qv::BoundForm the four qv_index_set_bound_plane*
    int bound_wide = 0;                        // qv_index_set_bound_scan_wide: QV_BOUND_SCAN_* for the wide form (65 <= k <= 1024), a knob of its own
    int bound_wide_filtered = 0;               // qv_index_set_bound_scan_wide_filtered: the same for ONE filtered query of that length, a knob of its own
    int bound_wide_mq = 0;                     // qv_index_set_bound_scan_wide_mq: the same for an unfiltered shared pass of 2 - 8 queries of that length, a knob of its own
    int8_t* d_plane8 = nullptr;                // the int8 copy and its row state (scale, residual): kept with the default bfloat16 copy, refreshed with it
    float* d_rscale8 = nullptr;
    float* d_rres8 = nullptr;
    bool plane8_lost = false;                  // it could not be allocated: the index carries on with the bfloat16 copy
    uint8_t* d_plane6 = nullptr;               // the 6-bit plane and its residual: kept with the 8-bit plane (whose scale it shares), refreshed with it
    float* d_rres6 = nullptr;
    bool plane6_lost = false;                  // it could not be allocated: the index carries on with the 8-bit plane
    int filtered_batch = 0;                    // qv_index_set_filtered_batch: QV_FILTERED_BATCH_*
    uint32_t filtered_batch_ppm = 0xFFFFFFFFu; // ... and its sparse floor in millionths of the rows (0xFFFFFFFF: the default, 0: never sparse)
    std::atomic<uint64_t> fb_stats[4] = {};    // qv_index_filtered_batch_stats: queries on the path, handed back (overflow / no bound / failed guess), handed back as sparse, batches
    uint32_t* d_bound_stats = nullptr;         // [0] survivors of the last bound scan, [1] hand-backs, [2] bound scans (written by the kernels)
    std::vector<uint64_t> alive_host;          // mirror of d_alive, for size bookkeeping and validation
    Buf mut_stage;                             // grow-only staging buffer of the mutating calls (add / remove / update run under the
                                               // caller's exclusion, so one buffer serves them all: no hipMalloc per single-row Insert)

    std::mutex ctx_mu;
    std::vector<SearchCtx*> free_ctx;
    std::vector<SearchCtx*> all_ctx;
    uint64_t batched_redo = 0;                 // queries the MFMA path handed back to the exact scan
    bool profiling = false;                    // qv_index_profile: event pairs around scan kernels
    std::mutex prof_mu;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
    std::mutex ws_mu;
    std::map<hipStream_t, Workspace*> stream_ws;   // workspaces of the *_device entry points, one per caller stream
    // concurrent single-query callers (all the reference's host ever produces: collection.go:647, db.go:805-828) ride the next
    // pass together (qv_coalesce.h): one pass in flight — a flat scan is HBM-bound, a second one beside it only halves both —
    // and up to 256 queries per group, the size the matrix-core filter walks the corpus once for
    qvco::Front front{1, 256, 4};
    // the same for qv_index_search_rowsets: filtered callers share passes among themselves (a member's tag = its set handles); a front
    // of its own, so that the unfiltered one's groups, lanes and statistics are what they were
    qvco::Front front_rs{1, 256, 4};

    qv::IndexView view() const {
        qv::IndexView v;
        v.tiles = d_tiles; v.rnorm = d_rnorm; v.alive = d_alive; v.rres = d_rres; v.rowmaj = d_rowmaj;
        v.bf16 = (flags & QV_FLAG_BF16_ROWS) ? d_bf16 : nullptr; v.plane = d_bf16; v.bound_scan = bound.scan;
        v.plane8 = d_plane8; v.rscale8 = d_rscale8; v.rres8 = d_rres8; v.bound_plane = bound.plane[qv::bound_one]; v.bound_plane_filtered = bound.plane[qv::bound_one_filtered]; v.bound_plane_mq = bound.plane[qv::bound_mq]; v.bound_plane_filtered_mq = bound.plane[qv::bound_mq_filtered];
        v.dim = dim; v.dim4 = dim4; v.n_rows = n_rows; v.n_tiles = (n_rows + 63) / 64; v.metric = metric; v.filter = filter;
        v.l2_planes = l2_planes() ? 1 : 0;
        v.rowmaj16 = d_rowmaj16;
        v.rowmaj8 = d_rowmaj8; v.rowmeta8 = d_rowmeta8;
        v.plane6 = d_plane6; v.rres6 = d_rres6; v.bound_plane6 = bound.plane6;
        return v;
    }
    // a Euclidean index that asked for the scan planes (QV_FLAG_L2_SCAN_PLANE; on every other metric the flag does nothing)
    // (QV_FLAG_NO_SCAN_PLANE beside it wins, also where QV_FLAG_BF16_ROWS keeps a copy for the batched filter: no bound scan on that copy)
    bool l2_planes() const { return metric == QV_L2 && (flags & QV_FLAG_L2_SCAN_PLANE) != 0 && !(flags & QV_FLAG_NO_SCAN_PLANE); }
    bool plane_metric() const { return metric == QV_COSINE || metric == QV_DOT || l2_planes(); }
    // cosine and dot indexes — and such a Euclidean one — keep the bfloat16 copy unless told not to (QV_FLAG_NO_SCAN_PLANE) or it could not be allocated
    bool wants_plane() const {
        return (flags & QV_FLAG_BF16_ROWS) || (!(flags & QV_FLAG_NO_SCAN_PLANE) && !plane_lost && plane_metric());
    }
    // ... and the 8-bit plane wherever they keep that copy BY DEFAULT and the 8-bit stage can walk the rows (whole 16-dimension steps, int32 sums)
    bool wants_plane8() const {
        return !(flags & QV_FLAG_NO_SCAN_PLANE) && !plane_lost && !plane8_lost && plane_metric() && (dim & 15u) == 0 && dim <= 4096;
    }
    // the row-order bfloat16 copy a graph's rejecting hops read: asked for, beside the float32 row-major copy, on the bound's metrics, whole 64-element slabs
    bool wants_rowmaj16() const {
        return (flags & QV_FLAG_GRAPH_PLANE) && (flags & QV_FLAG_ROWMAJOR) && !rowmaj16_lost && (metric == QV_COSINE || metric == QV_DOT) && (dim & 63u) == 0 && dim <= 4096;
    }
    // the row-order 8-bit image, the same way: whole 128-element slabs, and sums that stay exact in int32 (dim <= 4096).  Independent of the copy above
    // and of the tile-layout 8-bit plane (QV_FLAG_NO_SCAN_PLANE): k_rowmaj8 derives its own scale and residual
    bool wants_rowmaj8() const {
        return (flags & QV_FLAG_GRAPH_PLANE8) && (flags & QV_FLAG_ROWMAJOR) && !rowmaj8_lost && (metric == QV_COSINE || metric == QV_DOT) && (dim & 127u) == 0 && dim <= 4096;
    }
    // ... and the 6-bit plane wherever they keep the 8-bit one, unless told not to (QV_FLAG_NO_PLANE6), on rows of whole 64-dimension groups
    bool wants_plane6() const { return wants_plane8() && !(flags & QV_FLAG_NO_PLANE6) && !plane6_lost && (dim & 63u) == 0; }
    size_t plane8_tile_bytes() const { return (size_t)dim * 64; }
    size_t plane6_tile_bytes() const { return (size_t)dim * 48; }
    size_t tile_bytes() const { return (size_t)dim4 * 64 * 16; }
    size_t bf16_tile_bytes() const { return (size_t)(((dim4 + 1) / 2 + 1) / 2) * 2 * 64 * 16; }   // whole 16-dim steps (k_bf16_plane's layout)
};


// A set of rows of ONE index as a bitmap on that index's device (include/qv.h "row sets").  `words` 64-row words are valid: rows
// beyond them are unselected, which is how a set stays valid while its index grows — the scans take (pointer, words) per query and
// never touch the allocation.  host mirrors d_bits (qv_rowset_count, and the match counts of the k > 64 paths).
struct qv_rowset {
    qv_index* idx = nullptr;
    int device = 0;                            // idx->device (kept here: destroying a set does not touch its index)
    uint64_t* d_bits = nullptr;
    uint32_t words = 0;
    std::vector<uint64_t> host;
    uint32_t tiles = 0;                        // non-empty words of `host`: the tiles a scan under this set can have to read (the filtered bound-scan rule's input)
    uint64_t selected = 0;                     // bits set in `host`, dead rows included: fewer than k means no threshold under this set (the rule's other input)
    Buf stage;                                 // row ids of qv_rowset_set_rows; the literals of qv_rowset_create_where
};

// One typed value per row of ONE index on that index's device (include/qv.h "facet columns").  Storage is whole 64-row tiles
// (cap_tiles of them, zero-filled when grown: a tile inside the capacity can always be loaded); `rows` is the extent, and a
// presence word past ceil(rows / 64) is never read — rows beyond have no value, which is how a column stays valid while its index grows.
struct qv_column {
    qv_index* idx = nullptr;
    int device = 0;
    int type = 0;                              // QV_COL_*
    void* d_values = nullptr;                  // double or uint32_t per row
    uint64_t* d_present = nullptr;             // bit r % 64 of word r / 64: row r has a value
    uint32_t cap_tiles = 0;
    uint32_t rows = 0;
    Buf stage;                                 // presence bytes of qv_column_set
    size_t elem() const { return type == QV_COL_F64 ? sizeof(double) : sizeof(uint32_t); }
};
