// qv_device.h — internal interface between the C-ABI layer (qv_api.cpp) and the
// gfx950 kernels (qv_scan/qv_bound_scan/qv_rank/qv_batched/qv_hnsw/qv_misc.hip; shared helpers in qv_kernels.h).  Not installed; include/qv.h is the public ABI.
//
// HBM layout of an index ("row tiles", the SoA layout of DESIGN.md §3):
//   tiles   float  [n_tiles][dim4][64][4]   tile t holds rows 64t..64t+63; within a
//                                            tile, 16-byte chunk c (dims 4c..4c+3) of
//                                            row r sits at ((t*dim4 + c)*64 + r)*16 B.
//                                            One wave-wide dwordx4 load = one contiguous
//                                            KiB; lane == row, so a lane accumulates its
//                                            row's distance over dims 0..D-1 in exactly
//                                            the reference's element order.
//   rnorm   double [n_tiles*64]              per-row sqrt(sum b_i^2) in the metric's
//                                            precision (cosine metrics only)
//   alive   u64    [n_tiles]                 bit r of word t = row 64t+r is live
//   rres    float  [n_tiles*64]              per-row |r - bf16(r)|, rounded up: what the one-term bfloat16 filter loses of a row
//                                            (qv_batched.hip: its error bound is per row and per query, not a worst case)
//   rowmaj  float  [rows][dim]               optional row-major copy (QV_FLAG_ROWMAJOR)
//   rowmaj16 bf16  [rows][dim]               optional bfloat16 image of it (QV_FLAG_GRAPH_PLANE): what a rejecting graph hop reads
//   rowmaj8  i8    [rows][dim]               optional int8 image of it (QV_FLAG_GRAPH_PLANE8) and rowmeta8, a 16-byte record per row: what a hop rejecting on 8 bits reads
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qv_workspace.h"

namespace qv {

constexpr int kTileRows = 64;          // one wavefront
constexpr int kMaxFusedK = 64;         // wave-resident top-k list: one key per lane
constexpr int kMaxWideK = 128;         // wave-resident list of 2 keys per lane (k_flat_scan_wide) + selection over the waves' lists
constexpr int kMaxBatchedK = 4096;     // filter + re-score batches: beyond 64 results per query their selections are radix selections (qv_batched.hip)
constexpr int kMaxSelectK = 8192;      // one key per row + radix select (qv_select.hip): above it, the full ranking (qv_rank.hip)
constexpr uint64_t kDeadKey = ~0ull;

// one row of IndexView::rowmeta8: |r| as v.rnorm holds it, and the row's 8-bit scale and residual (rres8 NaN: a row the bound says nothing about)
struct RowMeta8 { double rnorm; float rscale8; float rres8; };

struct IndexView {
    float*    tiles;
    double*   rnorm;
    uint64_t* alive;
    float*    rres;       // |r - bf16(r)| per row (k_row_residual, after every write of rows)
    float*    rowmaj;     // may be null
    uint16_t* bf16;       // may be null: bfloat16 copy of the rows, [tile][ceil(dim/16)][2 row blocks][2 halves][32 rows][8 values] (QV_FLAG_BF16_ROWS)
    uint32_t  dim;
    uint32_t  dim4;       // ceil(dim/4)
    uint32_t  n_rows;     // rows ever added
    uint32_t  n_tiles;    // ceil(n_rows/64)
    int       metric;
    int       filter;     // batched path's filter kernel: 0 = the library's rule, 1 fp32 MFMA chain, 2 bfloat16 x 3, 3 bfloat16 x 1 (qv_index_set_filter)
    uint16_t* plane;      // may be null: the same bfloat16 copy whenever the index keeps one — cosine and dot indexes do by default, for the
                          // single-query bound scan (qv_bound_scan.hip); `bf16` above is set only under QV_FLAG_BF16_ROWS, so the batched path's
                          // choice of kernels is what the flag alone decides.  The calls that write rows refresh `plane`.
    int       bound_scan; // qv_index_set_bound_scan: 0 from the measured row count on, 1 whenever it applies, 2 never
    int8_t*   plane8;     // may be null: the int8 copy of the rows, [tile][dim/16][64 rows][16 values], one scale per row (k_row_state8);
                          // kept wherever `plane` is kept by default and dim is a multiple of 16 up to 4096.  Refreshed with `plane`.
    float*    rscale8;    // per row: max|r_i| / 127 rounded up (0: no scale)
    float*    rres8;      // per row: |r - rscale8 r8| rounded up; NaN = a row the 8-bit bound says nothing about
    int       bound_plane; // qv_index_set_bound_plane: 0 the 8-bit stage from its measured row count on, 1 whenever it applies, 2 never
    int       bound_plane_filtered; // qv_index_set_bound_plane_filtered: the same three values for a filtered single query, a knob of its own
    int       bound_plane_mq; // qv_index_set_bound_plane_mq: the same three values for an unfiltered shared pass of 2 - 8 queries, a knob of its own
    int       bound_plane_filtered_mq; // qv_index_set_bound_plane_filtered_mq: the same three values for a filtered shared pass of 2 - 8 queries, a knob of its own
    int       l2_planes;  // a QV_L2 index created with QV_FLAG_L2_SCAN_PLANE: bound_ask asks the rules as QV_RULE_L2_PLANES (0 on every other index)
    uint16_t* rowmaj16;   // may be null: bfloat16 copy of the rows in row order, [rows][dim] (QV_FLAG_GRAPH_PLANE: cosine / dot, rowmaj kept, dim a multiple of
                          // 64 up to 4096); element = (__bf16)x, the conversion k_row_residual measures.  Written wherever rowmaj is (k_rowmaj16)
    uint8_t*  plane6;     // may be null: the 6-bit plane, [tile][dim/64][3][64 rows][16 B] (qv_bound.h: bound6_pack), kept wherever plane8 is kept and dim is a
                          // multiple of 64 — never without plane8, whose scale it shares.  Refreshed with it (k_row_state6).
    float*    rres6;      // per row: |r - 4 rscale8 c6| rounded up; NaN = a row the 6-bit bound says nothing about
    int       bound_plane6; // qv_index_set_bound_plane6: 0 the 6-bit stage in front of the 8-bit one from its measured shapes on, 1 whenever that one is taken, 2 never
    int8_t*   rowmaj8;    // may be null: the rows' int8 image in row order, [rows][dim] (QV_FLAG_GRAPH_PLANE8: cosine / dot, rowmaj kept, dim a multiple of 128
                          // up to 4096); the bytes bound8_scale / bound8_quant give (plane8's, where that is kept).  Written wherever rowmaj is (k_rowmaj8)
    RowMeta8* rowmeta8;   // beside it, one record per row: what a rejecting graph hop needs of the row in ONE gather
};

static_assert(sizeof(RowMeta8) == 16, "one 16-byte record per row");

struct GraphView {
    const int8_t*   level;      // [n] node level, -1 = tombstone
    const uint32_t* l0_deg;     // [n]
    const uint32_t* l0_links;   // [n][max_m0]
    const uint32_t* up_off;     // [n] first block of the node's upper levels (level 1 -> block up_off[n])
    const uint32_t* up_links;   // blocks of (1 + max_m): degree, links
    uint32_t n_nodes, max_m0, max_m;
    uint32_t entry; int cur_level;
    bool has_dead;              // some level[] entry is -1 (a graph built on the device has none)
};

// Extras of the traversal kernels beyond a plain Search: the build's per-query stop level, the device-side redo list of
// the exact-heap pass, and the visited-set storage (qv_hnsw.hip).
struct HnswOpts {
    const int8_t*   qlevel    = nullptr;  // build: level of the node query i stands for; the query stops at
                                          // min(qlevel[i], cur_level) and searches THAT level with ef (hnsw.go:383-385)
    uint32_t        qnode0    = 0;        // build: node index of query 0 (query i is node qnode0 + i)
    float*          self_dist = nullptr;  // build: [nq] distance(node, node), written when the stop level is >= 1
    const uint32_t* redo_idx  = nullptr;  // heap kernel: the queries to run (null = all nq)
    const uint32_t* redo_n    = nullptr;  // heap kernel: how many of them (device word)
    uint32_t*       vis       = nullptr;  // visited storage: [slots][vis_cap] hash entries / [slots][vis_cap] bitmap words
    uint32_t        vis_cap   = 0;        // per slot: hash entries (power of two) / bitmap words
    uint32_t        vis_lds   = 0;        // set by launch_hnsw_search_wave for its latency form: the hash table is in LDS
    uint32_t        lat_rows  = 32;       // set by the launchers for the latency form: rows of a hop requested at once (32 / 16 / 8 by dimension)
    // the hubs (qv_graph_api.cpp graph_hubs): rows most traversals read are not read at all — their distances to every query of the call
    // are computed up front by a dense pass (k_hub_table) and looked up
    uint32_t*       hist      = nullptr;  // [n_nodes] += 1 per evaluated row (the sampling pass that chooses the hubs)
    const float*    hub_tab   = nullptr;  // [nq][hub_H] distance(query, hub)
    const uint16_t* l0_hub    = nullptr;  // [n_nodes][max_m0] the hub slot of every level-0 link (0xFFFF: not a hub)
    uint32_t        hub_H     = 0;        // hubs (0: none)
    const float*    q32       = nullptr;  // set by launch_hnsw_search_wave: the caller's queries as they came ([nq][dim] float32), what the front keeps in LDS
    uint32_t        front     = 0;        // set by launch_hnsw_search_wave for its wave-per-query form: which parts of the round-6 hop are on (qv_hnsw.hip)
    uint32_t*       next      = nullptr;  // set by launch_hnsw_search_wave: the call's query counter (zeroed by k_hnsw_prep_queries): a wave slot that
                                          // finishes its traversal takes the next unclaimed query instead of a fixed stride of them
    uint32_t        rj_image  = 0;        // with rj_stats: 0 = reject on the bfloat16 copy (rj_stats: the graph's bfloat16 counters), 1 = on the 8-bit image
                                          // (rj_stats: its 8-bit counters) — qv_graph_reject_image_applies' answer minus one
    unsigned long long* rj_stats = nullptr; // [3] the graph's reject counters (qv_graph_reject_stats); non-null = this call asked for the rejecting
                                          // form (qv_graph_reject_applies said yes): launch_hnsw_search_wave takes it where its own conditions hold
};

// the mutable arrays of a graph under construction (qv_build.hip); every link carries its distance
struct BuildView {
    int8_t*   level;      // [cap_nodes]
    uint32_t* l0_deg;     // [cap_nodes]
    uint32_t* l0_links;   // [cap_nodes][max_m0]
    float*    l0_dist;    // [cap_nodes][max_m0]
    uint32_t* up_off;     // [cap_nodes]
    uint32_t* up_links;   // [blocks][1 + max_m]
    float*    up_dist;    // [blocks][max_m]
    uint32_t  cap_nodes, max_m0, max_m;
};

struct ScanPlan {
    uint32_t grid;        // workgroups
    uint32_t block;       // threads (multiple of 64)
    uint32_t n_lists;     // partial lists the scan writes (= grid)
    uint32_t cus;         // compute units of the device the plan was made for
};

// how many workgroups a scan over n_tiles uses on a device with `cus` CUs
ScanPlan plan_scan(uint32_t n_tiles, int cus);

// exact multi-query scan on the f64 matrix cores (qv_mq64.hip): 0 = not applicable, else 16-query blocks per pass
int mq64_blocks(int metric, uint32_t dim4, uint32_t nq);
size_t mq64_workspace_bytes(uint32_t nq, uint32_t dim4, WsLog* log = nullptr);
hipError_t launch_flat_scan_mq64(const IndexView& v, int cus, const float* d_queries, uint32_t nq, uint32_t k, void* d_qws, uint64_t* partial,
                                 uint32_t* grid_out, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1);

// The workspace of a fused flat search (k <= kMaxFusedK), the ONE statement of it: the partial lists of nq queries at list length k, then
// one tail — the multi-query kernels' query blocks, or the matrix-core scan's block (mq64_workspace_bytes), or (call_bound) the
// single-query bound scan's buffer, all three starting at `tail` — and over the whole of it the small scan's lists and (call_bound_mq) the
// shared bound pass's buffer, which have the workspace to themselves and start at `partial`.
enum class FlatWs {
    lists,          // the partial lists alone: a caller that lays its own tail at `tail` (the row-set scan)
    sample,         // ... and the query blocks (the batch's front: its sample scan)
    call,           // a search call: every tail a route without a bound scan reads, and the small scan's lists
    call_bound,     // ... whose route is bound / bound8_first
    call_bound_mq,  // ... whose route is bound_mq
};
struct FlatLayout { uint64_t* partial; void* tail; size_t end, total; };
FlatLayout flat_layout(void* base, FlatWs what, const ScanPlan& p, uint32_t nq, uint32_t k, uint32_t n_tiles, uint32_t dim, WsLog* log = nullptr);

// --- ingest ---------------------------------------------------------------------
// d_rows [n][dim] row-major on device -> tiles at rows [row0, row0+n); computes rnorm;
// sets alive bits; also fills rowmaj if present.
hipError_t launch_ingest(const IndexView& v, const float* d_rows, uint32_t row0, uint32_t n, hipStream_t s);
// scattered ingest: d_vecs [.][dim] row-major on device; d_rows_sorted[n_unique] ascending and distinct, all below v.n_rows;
// d_src[i] = the position in d_vecs of row d_rows_sorted[i]'s vector; d_tiles[n_tiles] = the touched tiles, ascending, and
// d_tile_first[n_tiles + 1] = where each one's entries start in the sorted list.  Listed rows get what launch_ingest gives a row
// (tiles, rowmaj, rnorm, alive bit); the derived planes of the touched tiles are refreshed by the kernels that serve launch_ingest.
hipError_t launch_update_rows(const IndexView& v, const float* d_vecs, const uint32_t* d_rows_sorted, const uint32_t* d_src,
                              const uint32_t* d_tile_first, const uint32_t* d_tiles, uint32_t n_unique, uint32_t n_tiles, hipStream_t s);
// synthetic rows straight into tile layout (the synthetic-corpus generator of DESIGN.md)
hipError_t launch_generate(const IndexView& v, uint64_t seed, uint64_t gen_row0, uint32_t row0, uint32_t n, hipStream_t s);
// tombstone / revive
hipError_t launch_set_alive(const IndexView& v, const uint32_t* d_rows, uint32_t n, int alive, hipStream_t s);
// tile layout -> row-major (one row)
hipError_t launch_fetch_row(const IndexView& v, uint32_t row, float* d_out, hipStream_t s);
// tile layout -> row-major, n listed rows -> d_out [n][dim]
hipError_t launch_fetch_rows(const IndexView& v, const uint32_t* d_rows, uint32_t n, float* d_out, hipStream_t s);

// --- search ---------------------------------------------------------------------
// Flat scan + fused top-k for k <= kMaxFusedK.  d_queries [nq][dim] float32 on device.
// d_ws: workspace of flat_layout().  Writes d_rows_out/d_dist_out [nq][k]
// (padded with 0xFFFFFFFF / +inf).
// ev0/ev1 (optional): recorded immediately before/after the scan kernel on `s`.
// d_tickets (optional): 64 zeroed words that belong to the caller's stream alone — with them a single query is ONE launch (the last
// workgroup of the scan merges the lists); without, scan + k_merge_lists.
// Which kernels answer the call is decided ONCE, by plan_flat, before the first launch (the batched path's plan_batched / BatchedRoute
// is the model): the launch, the workspace sizes (qv_api.cpp) and the QV_TRACE lines read the plan.  Whether the bound scan takes the call, and
// with which stages, is ONE question to bound_scan_decide (below; qv_bound_scan.hip) inside plan_flat: its answer is the three bound routes and
// FlatPass::plane8_first, and nothing behind the plan asks again.  The routes in priority order:
enum class FlatRoute : int {
    small = 0,      // no bound route, tickets, flat_small_applies and not flat_split_applies: k_flat_scan_small, scan + merge in one launch
    bound_mq,       // 2 - 8 queries, tickets and counters, bound_scan_decide takes them, and "always" or no short-corpus form: launch_bound_scan_mq, one
                    // pass over the bfloat16 copy (FlatPass::plane8_first: the 8-bit stage in front of it), the exact redo of hand-backs behind it
    split_mq,       // 2 or more queries, flat_split_mq_applies: k_flat_scan_split_mq + k_merge_lists
    mq64,           // 9 or more cosine / dot queries over 16 tiles per wave or more: launch_flat_scan_mq64 + k_merge_lists
    mq,             // 2 or more queries: k_flat_scan_mq, qb = 4 / 8 / 16 per corpus pass (16 never for the all-float32 metrics) + k_merge_lists
    bound,          // one query, tickets and counters, bound_scan_decide takes it: launch_bound_scan and the gated exact scan behind it
    bound8_first,   // ... and answers BoundStages::plane8_first: the 8-bit stage in front
    split,          // tickets, flat_split_applies: k_flat_scan_split, a tile over eight waves
    fused,          // one query, tickets, more than one workgroup: k_flat_scan<., ., true>, the last workgroup merges
    two_launch,     // everything else: k_flat_scan + k_merge_lists
};
struct FlatPass {                   // what one pass over the corpus is launched from
    FlatRoute route = FlatRoute::two_launch;
    uint32_t  qb = 0;               // queries per corpus pass (bound_mq, split_mq, mq)
    bool      filtered = false;     // v.alive is a filter's candidate bitmap: the bound routes' forms that skip tiles without a candidate
    bool      plane8_first = false; // bound_mq and bound8_first: the 8-bit stage in front of the bfloat16 stage (for one query the route's number says it too)
    bool      plane6_first = false; // bound8_first, unfiltered only: the 6-bit stage in front of the 8-bit stage's refine (a decision inside the route, as the plane is inside bound_mq)
};
struct FlatPlan : FlatPass {        // the call's pass; mq64 with more than 32 queries of which the last 1 - 8 are split off: the pass of
    uint32_t rem = 0;               // the first nq - rem, and the pass of the last rem behind it (never a bound route)
    FlatPass tail;
    bool bound() const { return route == FlatRoute::bound_mq || route == FlatRoute::bound || route == FlatRoute::bound8_first; }
};
// tickets / stats: the call carries the stream's ticket words / the index's bound-scan counters; candidate_tiles: kBoundNoFilter, or the
// tiles that hold a candidate of a filtered call (an upper bound known on the host)
FlatPlan plan_flat(const IndexView& v, const ScanPlan& p, uint32_t nq, uint32_t k, bool tickets, bool stats, uint32_t candidate_tiles);
// plan_flat without an index or a device (qv_scan_route): the route's number, < 0 for arguments no route serves
int host_flat_route(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int cus, int tickets, int bound_mode, int plane_mode, int has_plane, int has_plane8,
                    uint32_t candidate_tiles, int plane_mode_filtered);
// f = plan_flat for the same v, p, nq, k, d_tickets != null, d_bound_stats != null and candidate_tiles.  d_ws: the route's share of qv_api.cpp's
// search_ws_bytes, which is sized from the same plan.
hipError_t launch_flat_topk(const IndexView& v, const ScanPlan& p, const FlatPlan& f, const float* d_queries, uint32_t nq, uint32_t k,
                            void* d_ws, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s,
                            hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, uint32_t* d_tickets = nullptr,
                            uint32_t* done_flag = nullptr, uint32_t done_seq = 0, bool* flag_used = nullptr,   // done_flag: see launch_flat_small (small, split and fused)
                            uint32_t* d_bound_stats = nullptr,   // the index's bound-scan counters (the bound routes)
                            uint32_t candidate_tiles = 0xFFFFFFFFu);   // not kBoundNoFilter: v.alive is a filter's candidate bitmap with at most so many non-empty tiles
// ... for callers without tickets (the batched path's sample scan): routes split_mq, mq64, mq or two_launch
hipError_t launch_flat_topk(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint32_t k,
                            void* d_ws, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s);
struct RowSetRef;
constexpr uint32_t kBoundNoFilter = 0xFFFFFFFFu;   // candidate_tiles of an unfiltered search
// WHICH stages answer a call is one decision, bound_scan_decide (qv_bound_scan.hip), for all forms of the bound scan: one query or a shared pass of
// 2 - 8, unfiltered or under a filter, the bfloat16 stage alone or the 8-bit stage (k_bound_scan8 / k_bound_scan8_mq) in front of it.  plan_flat
// asks it once per call and records the answer in the plan; the row-set front (qv_api.cpp: rowsets_plan) asks it for its own pieces; the
// qv_scan_bound*_applies exports are views of it.  The launchers only check what their kernels need (bound_scan_kernels_serve).
struct BoundAsk {                 // the call, as the rules see it
    int rule_metric;              // the index's metric; QV_RULE_L2_PLANES for a QV_L2 index that holds the planes
    uint32_t dim, n_rows, nq, k;
    uint32_t candidate_tiles;     // kBoundNoFilter, or the tiles that hold a candidate of any query of the pass (an upper bound known on the host)
    bool has_plane, has_plane8;   // the bfloat16 copy / the 8-bit plane is held
    bool has_plane6 = false;      // ... and the 6-bit plane
};
enum BoundForm { bound_one = 0, bound_one_filtered, bound_mq, bound_mq_filtered };   // follows from nq and candidate_tiles; each has a plane knob of its own
inline BoundForm bound_form(const BoundAsk& a) { return (BoundForm)((a.nq > 1 ? 2 : 0) + (a.candidate_tiles != kBoundNoFilter ? 1 : 0)); }
struct BoundKnobs {               // host only.  0: the environment variable decides (read once), else automatic — the measured floors
    int scan;                     // qv_index_set_bound_scan / QV_BOUND_SCAN: 1 whenever the kernels serve the call, 2 never
    int plane[4];                 // by BoundForm: qv_index_set_bound_plane, _filtered, _mq, _filtered_mq / QV_BOUND_PLANE, _FILTERED, _MQ, _FILTERED_MQ:
                                  // 1 the 8-bit stage first whenever the bound scan takes the call and the plane is held, 2 never
    int plane6 = 0;               // qv_index_set_bound_plane6 / QV_BOUND_PLANE6 (one unfiltered query only): 1 the 6-bit stage first whenever the 8-bit stage would be and the plane is held, 2 never
};
enum class BoundStages { none, bf16, plane8_first, plane6_first };   // plane6_first: plane8_first with the 6-bit stage in front (bound_one only)
inline bool bound_stages_8bit(BoundStages s) { return s == BoundStages::plane8_first || s == BoundStages::plane6_first; }
BoundStages bound_scan_decide(const BoundAsk& a, const BoundKnobs& knobs);
bool bound_scan_kernels_serve(const BoundAsk& a);   // the kernels' own limits: metric, k, 1 - 8 queries, the copy, whole 16-dimension steps, 8 tiles, lower bounds under 2 GiB
BoundAsk bound_ask(const IndexView& v, uint32_t nq, uint32_t k, uint32_t candidate_tiles);
BoundKnobs bound_knobs(const IndexView& v);
int bound_scan_mode(int mode);   // the mode in force: the index's own, else QV_BOUND_SCAN (read once)
// The single-query scan on the bfloat16 copy (qv_bound_scan.hip): stage 1 streams v.plane and lists the rows whose certified lower bound of
// the distance is within the k-th smallest upper bound, stage 2 computes those rows' distances in the scan's own arithmetic and writes
// the k results, or sets *gate (a device word) when the exact scan must answer instead; the caller then issues the exact scan with that
// gate (it leaves at once when the word is zero).  d_ctrl: the stream's zeroed control words (kept zero); d_stats: the index's counters.
size_t bound_scan_workspace_bytes(const ScanPlan& p, uint32_t k, uint32_t n_tiles, WsLog* log = nullptr);
hipError_t launch_bound_scan(const IndexView& v, const ScanPlan& p, const float* d_query, uint32_t k, void* d_ws, uint32_t* d_ctrl, uint32_t* d_stats,
                             uint32_t* d_rows_out, float* d_dist_out, const uint32_t** gate_out, hipStream_t s,
                             bool masked = false,   // v.alive is a filter's candidate bitmap: the form that does not request tiles without a candidate (k_bound_scan<., true>)
                             bool plane8_first = false,   // the 8-bit stage (k_bound_scan8; masked: its skipping form) in front, the bfloat16 stage gated behind it: d_ctrl = 2 BoundCtrl
                             bool plane6_first = false);  // (with plane8_first, unmasked) k_bound_scan6 + k_bound_refine8 in the place of k_bound_scan8: d_ctrl = 3 BoundCtrl
// ... and for the 2 - 8 queries of a shared pass (k_bound_scan_mq): d_ws bound_scan_mq_workspace_bytes, d_ctrl 8 BoundCtrl; the exact scan of
// the queries it hands back is enqueued behind it (launch_flat_redo_flagged)
size_t bound_scan_mq_workspace_bytes(const ScanPlan& p, uint32_t nq, uint32_t k, uint32_t n_tiles, uint32_t dim, WsLog* log = nullptr);
hipError_t launch_bound_scan_mq(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint32_t k, void* d_ws, uint32_t* d_ctrl, uint32_t* d_stats,
                                uint32_t* d_rows_out, float* d_dist_out, hipStream_t s,
                                const RowSetRef* h_sets = nullptr,   // a HOST array of nq sets, at most 8: query j over alive & h_sets[j] (k_bound_scan_mq<., ., true>, the redo included)
                                bool plane8_first = false);   // the 8-bit stage (k_bound_scan8_mq; with h_sets its set form) in front, the bfloat16 stage's launches gated behind it
// the interval of one row on the HOST (qv_scan_bound_interval): qv_bound.h's function compiled for the CPU; 1 = a row the bound says nothing about
int host_bound_interval(int metric, uint32_t dim, float s, double qn, double rn, float rres, float* d_lo, float* d_hi);
int host_bound_interval8(int metric, uint32_t dim, long long isum, double sq, double qn, double qres, double rn, float rscale, float rres8, float* d_lo, float* d_hi);
int host_quantize_row8(uint32_t dim, const float* row, int8_t* out_bytes, float* out_scale, float* out_res);
// one row as k_row_state6 leaves it: out_bytes[dim * 3 / 4] = the row's three 16-byte pieces per 64-dimension group, in the order X, Y, Z
// (scale8: the row's 8-bit scale, as host_quantize_row8 gives it); and those bytes back into biased codes u[dim]
int host_quantize_row6(uint32_t dim, const float* row, float scale8, uint8_t* out_bytes, float* out_res);
int host_unpack_row6(uint32_t dim, const uint8_t* bytes, uint8_t* out_codes);
// The WIDE form of the single-query bound scan, unfiltered or over a candidate bitmap, 65 <= k <= kBoundWideMaxK (qv_bound_scan.hip): stage 1 publishes every wave's 64
// smallest upper bounds, H is the k-th smallest key of their union (launch_select_topk), the collect has a list of QV_BOUND_WIDE_CAND_CAP rows,
// the re-score writes a key per survivor and launch_select_topk_counted takes the k best.  A search it cannot decide is redone by the
// key-per-row path behind a device word (launch_flat_select_redo_one).  Whether a search takes it is bound_wide_route's answer — a knob of its
// own (qv_index_set_bound_scan_wide / QV_BOUND_SCAN_WIDE), independent of bound_scan_decide, which keeps saying no above kMaxFusedK.
constexpr uint32_t kBoundWideMaxK = 1024;
constexpr uint32_t kBoundWideStatsWord = 10;   // the wide form's counters: [10] survivors passed to the re-score, [11] hand-backs to the exact path, [12] searches
// 0: no wide form; 1: the bfloat16 copy first; 2: the 8-bit plane first.  wide_mode: QV_BOUND_SCAN_* (0: QV_BOUND_SCAN_WIDE of the environment,
// read once, else automatic); plane_mode: the index's qv_index_set_bound_plane (0: QV_BOUND_PLANE, else automatic)
int bound_wide_route(int rule_metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int wide_mode, int plane_mode, bool has_plane, bool has_plane8);
// The same question for ONE query over a candidate bitmap (a mask, a row set, a where-filter made into a set).  wide_mode: the filtered form's own
// knob (qv_index_set_bound_scan_wide_filtered; 0: QV_BOUND_SCAN_WIDE_FILTERED, else automatic); plane_mode_filtered: the single-query filtered
// plane knob (qv_index_set_bound_plane_filtered); candidate_tiles: the tiles that hold a candidate, as the host knows them; candidates: the live
// rows the filter selects — the form needs more of them than results.
int bound_wide_route_filtered(int rule_metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int wide_mode, int plane_mode_filtered, bool has_plane, bool has_plane8,
                              uint32_t candidate_tiles, uint64_t candidates);
size_t bound_scan_wide_workspace_bytes(const ScanPlan& p, uint32_t k, uint32_t n_tiles, uint32_t dim, WsLog* log = nullptr);
// d_ctrl: the stream's control words (2 BoundCtrl, kept zero but for the bfloat16 stage's flag, which every search writes before it is read);
// d_stats: the index's counters.  Enqueues everything, the gated exact redo included: nothing is read on the host.
hipError_t launch_bound_scan_wide(const IndexView& v, const ScanPlan& p, const float* d_query, uint32_t k, void* d_ws, uint32_t* d_ctrl, uint32_t* d_stats,
                                  uint32_t* d_rows_out, float* d_dist_out, hipStream_t s, bool plane8_first,
                                  bool masked = false);   // v.alive is the call's candidate bitmap: stage 1's SKIP forms; the stages behind read v.alive as they stand
// The WIDE form of the SHARED pass: one unfiltered call of 2 - 8 queries at 65 <= k <= kBoundWideMaxK (qv_bound_scan.hip): the shared pass's stage-1
// kernels with a list length of 64 publish every wave's list of every query, H_j is the k-th smallest of query j's published keys (one
// launch_select_topk over the nq arrays), the collect and the wave-per-survivor re-score run per query (grid y = query), one
// launch_select_topk_counted ends the pass, and launch_flat_select_redo behind it redoes, alone, the queries no stage could decide.  Whether a pass
// takes it is bound_wide_route_mq's answer — a knob of its own (qv_index_set_bound_scan_wide_mq / QV_BOUND_SCAN_WIDE_MQ), independent of
// bound_wide_route (which keeps answering 0 for nq != 1) and of bound_scan_decide; the plane it starts on is the shared pass's plane knob
// (qv_index_set_bound_plane_mq / QV_BOUND_PLANE_MQ).
constexpr uint32_t kBoundWideMqStatsWord = 13;   // its counters: [13] the largest survivor count of the last pass (each query in the stage that answered it), [14] queries handed back to the key-per-row path, [15] queries
// 0: no wide shared pass; 1: the bfloat16 copy first; 2: the 8-bit plane first.  wide_mq_mode: QV_BOUND_SCAN_* (0: QV_BOUND_SCAN_WIDE_MQ of the
// environment, read once, else automatic); plane_mode_mq: the index's qv_index_set_bound_plane_mq (0: QV_BOUND_PLANE_MQ, else automatic)
int bound_wide_route_mq(int rule_metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int wide_mq_mode, int plane_mode_mq, bool has_plane, bool has_plane8);
size_t bound_scan_wide_mq_workspace_bytes(const ScanPlan& p, uint32_t nq, uint32_t k, uint32_t n_tiles, uint32_t dim, WsLog* log = nullptr);
// d_ctrl: the stream's control words (kBoundMqMax BoundCtrl of which this form uses thr_inv, cand_cnt and ticket: zero on entry, left zero on
// every exit, hand-backs included); d_stats: the index's counters.  Enqueues everything, the flagged key-per-row redo included: nothing is read on the host.
hipError_t launch_bound_scan_wide_mq(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint32_t k, void* d_ws, uint32_t* d_ctrl, uint32_t* d_stats,
                                     uint32_t* d_rows_out, float* d_dist_out, hipStream_t s, bool plane8_first);
constexpr uint32_t kBound6StatsWord = 7;   // the 6-bit stage's counters: [7] candidates it passed to the refine, [8] hand-backs, [9] searches
constexpr uint32_t kBound6CandCap = 262144;   // rows the refine walks on the 8-bit plane (1 MiB of the workspace)
constexpr uint32_t kBound8StatsWord = 4;   // the 8-bit stage's counters in the index's counter words: [4] survivors, [5] hand-backs, [6] searches
constexpr uint32_t kBoundCtrlWord = 16;   // the bound scan's control words start here in the stream's 64 ticket words
bool flat_split_applies(const IndexView& v, uint32_t nq, uint32_t k);   // the tile-over-eight-waves form's own conditions (plan_flat: route split, given tickets)
// The exact scan (k <= kMaxFusedK) for exactly the queries whose d_flags word is non-zero — the ones a filter handed back —, listed and
// scanned on the device: nothing is read back.  Results replace rows / distances [q][k_stride] of those queries.  d_ws: redo_workspace_bytes.
size_t redo_workspace_bytes(const ScanPlan& p, uint32_t nq, uint32_t k, WsLog* log = nullptr);
hipError_t launch_flat_redo_flagged(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint32_t k, uint32_t k_stride, const uint32_t* d_flags,
                                    void* d_ws, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s,
                                    const RowSetRef* h_sets = nullptr);   // a HOST array of nq <= 8 sets (cosine / dot): query q is redone over alive & h_sets[q], tiles without a candidate skipped
// Small collections (<= 256 tiles, <= 4 queries, k <= 16): scan + merge in ONE launch (the last workgroup to finish merges).
// d_ws: flat_small_workspace_bytes (partial lists); d_tickets: 64 zeroed words that belong to the caller's stream alone (the kernel
// leaves them zero).  done_flag (optional, device-visible host memory): receives done_seq after the results have been written.
bool flat_small_applies(const IndexView& v, uint32_t nq, uint32_t k);
size_t flat_small_workspace_bytes(uint32_t nq, uint32_t k);
hipError_t launch_flat_small(const IndexView& v, const float* d_queries, uint32_t nq, uint32_t k, void* d_ws, uint32_t* d_tickets, uint32_t* d_rows_out, float* d_dist_out,
                             uint32_t* done_flag, uint32_t done_seq, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// merge n_lists lists of k (dist, row) pairs -> k best by (dist, row)
hipError_t launch_merge_shards(const uint32_t* d_packed, const uint32_t* d_bases, uint32_t n_lists, uint32_t nq, uint32_t k,
                               uint32_t* d_rows_out, float* d_dist_out, hipStream_t s, uint32_t planes = 0 /* 0: [nq][2][k] per shard; >= 2: [planes][nq][k] */);
// The same merge for lists of any length (k > kMaxFusedK: a filtered search asks every shard for its full ranking): the valid
// entries of the G sorted lists [planes][nq][kcap] of query q become 64-bit keys (distance, global row), one stable radix sort
// orders them, the first k_out are written (padded with 0xFFFFFFFF / +inf).  d_ws: merge_ranked_workspace_bytes(G * kcap).
size_t merge_ranked_workspace_bytes(uint64_t n_keys, WsLog* log = nullptr);
hipError_t launch_merge_ranked(const uint32_t* d_packed, const uint32_t* d_bases, uint32_t n_lists, uint32_t nq, uint32_t q, uint32_t kcap, uint32_t planes,
                               uint32_t k_out, void* d_ws, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s);
// The merge for kMaxFusedK < k_out <= kMaxSelectK, every query of the batch in one go: keys of all gathered entries, then the radix
// selection of the kk = min(k_out, valid entries) smallest (qv_select.hip) — 6 launches for the batch instead of 18 per query.
size_t merge_select_workspace_bytes(uint32_t n_lists, uint32_t nq, uint32_t kcap, uint32_t k_out, WsLog* log = nullptr);
hipError_t launch_merge_select(const uint32_t* d_packed, const uint32_t* d_bases, uint32_t n_lists, uint32_t nq, uint32_t kcap, uint32_t planes,
                               uint32_t k_out, uint32_t kk, void* d_ws, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s);
// payload lookup after a merge: out[i] = payload plane `plane` of the list entry that produced merged global row rows[i]
// (shard = the one whose base range holds the row; entry found by its local row), +inf for padding rows
hipError_t launch_lookup_payload(const uint32_t* d_packed, const uint32_t* d_bases, uint32_t n_lists, uint32_t nq, uint32_t q, uint32_t kcap, uint32_t planes,
                                 uint32_t plane, const uint32_t* d_rows, uint32_t n, float* d_out, hipStream_t s);
hipError_t launch_merge_pairs(const float* d_dist, const uint32_t* d_rows, uint32_t n_lists, uint32_t k,
                              uint32_t* d_rows_out, float* d_dist_out, hipStream_t s);

// --- row sets (qv_rowset.hip): one candidate bitmap per query ----------------------------------
// A query's set as the kernels see it: `words` 64-row words at `bits` (rows beyond them are unselected); bits == null: every row.
struct RowSetRef { const uint64_t* bits; uint32_t words; uint32_t pad_; };
// Exact multi-query scan, k <= kMaxFusedK, query q restricted to alive & h_sets[q] (a HOST array: the table travels to the device as
// kernel arguments, nothing is uploaded).  d_ws: rowset_workspace_bytes.  Writes [nq][k] lists padded with 0xFFFFFFFF / +inf.
size_t rowset_workspace_bytes(const ScanPlan& p, uint32_t nq, uint32_t k, uint32_t dim4, WsLog* log = nullptr);
hipError_t launch_rowset_topk(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint32_t k, const RowSetRef* h_sets,
                              void* d_ws, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// d_out[t] = alive[t] & set[t] over the index's tiles (the candidate bitmap of the single-query and k > 64 paths)
hipError_t launch_rowset_and(const IndexView& v, const RowSetRef& set, uint64_t* d_out, hipStream_t s);
// n padding entries (0xFFFFFFFF / +inf): the lists of queries whose set holds no live row
hipError_t launch_rowset_pad(uint32_t* d_rows, float* d_dist, size_t n, hipStream_t s);
// set / clear the listed rows' bits (d_rows on the device, every row < words * 64)
hipError_t launch_rowset_set_rows(uint64_t* d_bits, const uint32_t* d_rows, uint32_t n, int selected, hipStream_t s);
// --- row sets made on the device (qv_where.hip): predicates over typed columns, set algebra ----
// One comparison of a conjunction as the kernel sees it: the column's values (double or uint32_t per row, by `type`) and presence words
// (`tiles` of them are valid: rows beyond have no value), the op (QV_PRED_*) and its literals d_lits[lit0 .. lit0 + n_lit).
constexpr uint32_t kWherePreds = 8;
constexpr uint32_t kWhereLits = 256;                    // literals of one IN / NOT_IN
struct WherePred { const void* values; const uint64_t* present; uint32_t tiles; int type; int op; uint32_t lit0; uint32_t n_lit; uint32_t pad_; };
struct WhereTable { WherePred p[kWherePreds]; uint32_t n; uint32_t pad_; };
// d_out[t] = the rows r < n_rows of tile t for which every predicate holds, for all ceil(n_rows / 64) tiles (bits past n_rows: zero).
// The table travels as kernel arguments; d_lits is on the device.
hipError_t launch_rowset_where(const WhereTable& tab, const double* d_lits, uint32_t n_rows, uint64_t* d_out, int cus, hipStream_t s);
// Several conjunctions in ONE launch (k_where_mq: grid y = the filter), for the sets that live only as long as a search call
// (qv_index_search_where): filter f < n writes its words to out[f] (ceil(n_rows / 64) of them).  Everything travels as KERNEL
// ARGUMENTS, 3.7 KiB of the 4 KiB there are — which is what fixes kWhereMqFilters.  Literals: d_lits == null — filter f's are lits[f]
// (at most kWhereArgLits of them; WherePred::lit0 counts from 0 there), nothing for a device-pointer call to stage; otherwise
// d_lits[lit_base[f] + lit0 ...] on the device.  d_alive != null: the words are ANDed with the index's alive words (a candidate bitmap outright).
constexpr uint32_t kWhereMqFilters = 8;                 // QV_WHERE_FILTERS_PER_LAUNCH of include/qv.h
constexpr uint32_t kWhereArgLits = 16;                  // QV_WHERE_DEVICE_LITERALS of include/qv.h
struct WhereMqArgs {
    WhereTable tab[kWhereMqFilters];
    double lits[kWhereMqFilters][kWhereArgLits];
    uint64_t* out[kWhereMqFilters];
    uint32_t lit_base[kWhereMqFilters];
    uint32_t n; uint32_t pad_;
};
hipError_t launch_where_mq(const WhereMqArgs& a, const double* d_lits, const uint64_t* d_alive, uint32_t n_rows, int cus, hipStream_t s);
// d_dst[t] = a[t] OP b[t] (QV_SET_*) for t < words; a set shorter than that reads as zeros; d_dst may be a.bits or b.bits
hipError_t launch_rowset_combine(const RowSetRef& a, const RowSetRef& b, int op, uint32_t words, uint64_t* d_dst, hipStream_t s);
// presence bits of rows [first_row, first_row + n): bit = d_bytes[i] != 0 (null: all set); every other bit of the words stays
hipError_t launch_column_presence(uint64_t* d_present, uint32_t first_row, uint32_t n, const uint8_t* d_bytes, hipStream_t s);
// pieces of the multi-query scans that qv_rowset.hip shares with qv_scan.hip: the query blocks of the scalar-operand form
// (qblk[group][dim4 * 4][qb], qb = 4, 8 or — the float64-accumulating metrics — 16) and the merge of partial[nq][n_lists][k] into [nq][k] results
hipError_t launch_prep_qblk(int metric, uint32_t qb, const float* d_queries, uint32_t nq, uint32_t dim, uint32_t dim4, void* d_qblk, hipStream_t s);
hipError_t launch_merge_lists(const uint64_t* d_partial, uint32_t n_lists, uint32_t nq, uint32_t k, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s,
                              const uint32_t* d_gate = nullptr);   // a device word: zero = the launch leaves at once (the bfloat16 shared pass behind the 8-bit one)

// Batched path: fp32-MFMA filter + exact re-scoring (results identical to launch_flat_topk).
// *d_overflow_out -> [nq] flags (device): 1 = candidate buffer overflowed, caller must redo that
// query with launch_flat_topk.
bool   batched_supported(const IndexView& v, uint32_t nq, uint32_t k);
size_t batched_workspace_bytes(const IndexView& v, const ScanPlan& p, uint32_t nq, uint32_t k);
hipError_t launch_batched(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint32_t k, void* d_ws,
                          uint32_t* d_rows_out, float* d_dist_out, uint32_t** d_overflow_out, int cus, hipStream_t s,
                          hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, const struct BatchedSets* sets = nullptr);
// A filtered batch, k <= kMaxFusedK: query q over alive & d_sets[q] (a DEVICE array of nq sets; null bits = every row).  The sample's bound is
// taken over the set, the filter's flush drops rows outside it, and a query whose set holds fewer than sparse_ppm millionths of the sample's
// rows is handed back without candidates (0: never).  With sets, *d_overflow_out -> [2][nq]: the redo flags, then 1 = handed back as sparse
// (those are flagged in both).  Same workspace (batched_workspace_bytes).
struct BatchedSets { const RowSetRef* d_sets; uint32_t sparse_ppm; };
// whether launch_batched takes sets for this shape: batched_supported, k <= kMaxFusedK, and a route whose sample scores come from a filter
// kernel with every row's bound selected outside k_mfma_prep (the exact-scan sample of QV_MFMA_SAMPLE_GEMM is declined)
bool batched_sets_supported(const IndexView& v, uint32_t nq, uint32_t k, int cus);
// what plan_batched chose for the sample: its rows, every gstep-th 128-row group of the corpus, and the rank the bound is taken at
bool batched_sample_plan(const IndexView& v, uint32_t nq, uint32_t k, int cus, uint32_t* sample_rows, uint32_t* gstep, uint32_t* rank);
// The dispatch's rule for a filtered call or shared pass (qv_batched_applies_filtered; mode: QV_FILTERED_BATCH_*, 0 = QV_FILTERED_BATCH of the
// environment, else automatic): n_not_sparse = the piece's queries whose set the HOST does not know to be below the sparse floor.
bool filtered_batch_rule(int metric, uint32_t dim, uint64_t rows, uint32_t nq, uint32_t k, int filter, int mode, uint32_t n_not_sparse);
// Which main filter kernel a FILTERED batch of this shape launches (qv_batched_filter_route): plan_batched, then the remap launch_batched
// applies to a batch with sets.  plane: the index keeps the bfloat16 copy the batched filter reads.  *code: QV_BATCHED_FILTER_* of
// include/qv.h; false where batched_sets_supported is.
bool batched_sets_filter(int metric, uint32_t dim, uint64_t rows, uint32_t nq, uint32_t k, int filter, bool plane, int cus, uint32_t* nq_pad, int* code);
constexpr uint32_t kFilteredBatchMinQueries = 9;
constexpr uint32_t kFilteredBatchDefaultPpm = 10000;      // the sparse floor where the index sets none: a hundredth of the rows
constexpr uint32_t kFilteredBatchAutoMinRows = 300000;    // automatic mode takes nothing below the smallest measured shape
inline uint32_t filtered_batch_ppm(uint32_t ppm) { return ppm == 0xFFFFFFFFu ? kFilteredBatchDefaultPpm : ppm; }
// qv_batched_sets.hip — the two launches a filtered batch adds around the sample's selection and behind k_mfma_prep
hipError_t launch_sets_sample_mask(const IndexView& v, const RowSetRef* d_sets, uint32_t nq, float* d_bounds, uint32_t sample_rows, uint32_t gstep,
                                   uint32_t* d_n_in, hipStream_t s);
hipError_t launch_sets_sparse(uint32_t nq, uint32_t nq_pad, const uint32_t* d_n_in, uint32_t sample_rows, uint32_t sparse_ppm, float* d_cq, float* d_mq,
                              uint32_t* d_ovf, uint32_t* d_sparse, hipStream_t s);

// the one-term bfloat16 filter with the query operands in registers (qv_qreg.hip): same arguments and candidates as the eight-wave kernels
bool qreg_filter_applies(const IndexView& v, uint32_t nq_pad, bool bfrows);
hipError_t launch_qreg_filter(const IndexView& v, const uint4* Qbf, const float* cq, const float* mq, uint32_t nq_pad, uint32_t* cand, float* cscore,
                              uint32_t* cnt, bool bfrows, int cus, hipStream_t s);

// Device-resident HNSW traversal (hnsw.go:471-713), one wave per query.
size_t   hnsw_lds_bytes(uint32_t ef);
uint32_t hnsw_grid(int cus, uint32_t ef, uint32_t nq);
// prep = also convert the queries into d_qblk (false: d_qblk already holds them, e.g. the redo pass of the same batch)
hipError_t launch_hnsw_search(const IndexView& v, const GraphView& g, const float* d_queries, void* d_qblk, uint32_t nq, uint32_t k, uint32_t ef,
                              const HnswOpts& o, uint32_t grid, bool prep, uint32_t* d_rows_out, float* d_dist_out,
                              uint32_t* d_count_out, uint32_t* d_evals_out, hipStream_t s);
uint32_t hnsw_vis_hash_cap(uint32_t ef);                 // hash entries per wave slot for a search with this ef

// wave-resident form (no LDS heaps); count_out = 0xFFFFFFFE for queries that met equal distances / NaN
uint32_t hnsw_wave_grid(int cus, int metric, uint32_t dim4);
bool hnsw_image8_keeps_occupancy(int metric, uint32_t dim4);   // the 8-bit rejecting form's LDS leaves as many traversals per CU as the unchanged kernel's
uint32_t hnsw_lat_nq_cap(int cus);                        // the largest call launch_hnsw_search_wave hands to its latency form
hipError_t launch_hub_build(const IndexView& v, const GraphView& g, const uint32_t* d_hub_rows, uint32_t H, float* d_hub_tiles, double* d_hub_rnorm,
                            uint16_t* d_slot_of, uint16_t* d_l0_hub, hipStream_t s);
hipError_t launch_hub_table(const IndexView& v, const float* d_hub_tiles, const double* d_hub_rnorm, uint32_t H, const float* d_queries, void* d_qblk, uint32_t nq,
                            float* d_table, int cus, hipStream_t s);
size_t hnsw_qblk_bytes(uint32_t nq, uint32_t dim4);   // workspace for the converted queries + per-query constants
hipError_t launch_hnsw_search_wave(const IndexView& v, const GraphView& g, const float* d_queries, void* d_qblk, uint32_t nq, uint32_t k, uint32_t ef,
                                   const HnswOpts& o, uint32_t grid, uint32_t* d_rows_out, float* d_dist_out,
                                   uint32_t* d_count_out, uint32_t* d_evals_out, hipStream_t s);

// Selection path, kMaxFusedK < k <= kMaxSelectK (qv_select.hip): the kk smallest of each query's n keys (d_keys + q * stride; n and
// stride even), written as [nq][k_stride] rows / distances (padded).  ordered: among keys of equal distance, place in the array
// ascends with the low word (true for the keys of a scan, where place == row) — ties beyond the sort's capacity are then taken
// front to back; otherwise they are settled by three more radix windows on the low word.
// window0_counted: the kernel that made the keys also counted the selection's first window (select_prepare before it: qv_select.h)
struct SelState;
uint32_t select_cap(uint32_t kk);
size_t select_workspace_bytes(uint32_t nq, uint32_t kk, WsLog* log = nullptr);
hipError_t select_prepare(void* d_ws, uint32_t nq, uint32_t kk, SelState** st_out, uint32_t** hist_out, hipStream_t s);
hipError_t launch_select_topk(const uint64_t* d_keys, size_t stride, uint32_t n, uint32_t nq, uint32_t kk, uint32_t k_stride, void* d_ws,
                              uint32_t* d_rows_out, float* d_dist_out, hipStream_t s, bool window0_counted = false, bool ordered = true,
                              const uint32_t* d_active = nullptr /* device word: queries from *d_active on are left alone */);
// The direct form over lists whose live keys are a counted prefix (n <= 16384; qv_select.hip): only the prefix is read.  d_active as above.
hipError_t launch_select_topk_counted(const uint64_t* d_keys, size_t stride, uint32_t n, const uint32_t* d_counts, uint32_t nq, uint32_t kk, uint32_t k_stride,
                                      uint32_t* d_rows_out, float* d_dist_out, hipStream_t s, const uint32_t* d_active);
// 64 < kk <= kMaxWideK: the scan with a list of 2 keys per lane (same stream as launch_flat_topk, no key per row written),
// then the selection over the waves' lists.  ev0 / ev1 as launch_flat_topk.
size_t flat_wide_workspace_bytes(const ScanPlan& p, uint32_t nq, uint32_t kk, WsLog* log = nullptr);
hipError_t launch_flat_wide(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint32_t kk, uint32_t k_stride,
                            void* d_ws, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// keys [nq][n_tiles * 64] of nq >= 2 queries, QB (4 or 8) queries per corpus pass (k_flat_keys_mq); d_qws: flat_keys_mq_workspace_bytes
size_t flat_keys_mq_workspace_bytes(uint32_t nq, uint32_t dim4);
hipError_t launch_flat_keys_mq(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint64_t* d_keys, void* d_qws, hipStream_t s,
                               const uint32_t* d_active = nullptr /* device word: only the first *d_active queries are worked on */);
// scan + selection for nq queries at list length kk <= kMaxSelectK: every query's keys (one 8-byte key per row, k_flat_keys), then
// launch_select_topk; queries go in groups so that the keys of a group stay under flat_select_group_bytes
size_t flat_select_workspace_bytes(uint32_t n_tiles, uint32_t nq, uint32_t kk, uint32_t dim4, WsLog* log = nullptr);
hipError_t launch_flat_select(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint32_t kk, uint32_t k_stride,
                              void* d_ws, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s);
// The same for the queries whose flags are set (64 < kk <= kMaxSelectK: the batched filter's hand-backs above the wave lists' range), decided
// and listed on the device: nothing is read back.  Results replace rows / distances [q][k_stride] of those queries.
size_t flat_select_redo_workspace_bytes(uint32_t n_tiles, uint32_t nq, uint32_t kk, uint32_t dim, uint32_t dim4, WsLog* log = nullptr);
hipError_t launch_flat_select_redo(const IndexView& v, const ScanPlan& p, const float* d_queries, uint32_t nq, uint32_t kk, uint32_t k_stride, const uint32_t* d_flags,
                                   void* d_ws, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s);

// ... and for ONE query behind a device word (the wide bound scan's hand-back): *d_flag non-zero = the query is redone, zero = every launch
// leaves at once.  The lone query rides in a shared pass of two slots, so two queries' keys must fit a group (flat_select_redo_one_serves).
bool flat_select_redo_one_serves(uint32_t n_tiles);
size_t flat_select_redo_one_workspace_bytes(uint32_t n_tiles, uint32_t kk, uint32_t dim, uint32_t dim4, WsLog* log = nullptr);
hipError_t launch_flat_select_redo_one(const IndexView& v, const ScanPlan& p, const float* d_query, uint32_t kk, uint32_t k_stride, const uint32_t* d_flag,
                                       void* d_ws, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s);

// Full ranking path (any k): all distances -> 64-bit keys -> stable radix sort -> first k.
// d_keys_a/d_keys_b: two buffers of n_tiles*64 u64; d_hist: radix histogram workspace.
size_t  full_sort_workspace_bytes(uint32_t n_tiles, WsLog* log = nullptr);
hipError_t launch_flat_fullsort(const IndexView& v, const ScanPlan& p, const float* d_query, uint32_t k,
                                void* d_ws, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s);

// per-link distances of nodes [n0, n0 + nq) of an uploaded graph (what the device-side construction needs to extend it)
hipError_t launch_graph_link_dists(const IndexView& v, const GraphView& g, void* d_qblk, uint32_t n0, uint32_t nq, float* d_l0_dist, float* d_up_dist,
                                   uint32_t grid, hipStream_t s);

// stable sort of n 64-bit keys by their upper 32 bits; hist: radix_hist_words(n) words; *sorted_out = a or b
size_t radix_hist_words(uint32_t n);
hipError_t launch_radix_sort_hi32(uint64_t* a, uint64_t* b, uint32_t n, uint32_t* hist, uint64_t** sorted_out, hipStream_t s);

// HNSW construction, link phase of one batch (qv_build.hip).  d_counters: [0] redo count, [1] segment count, [2] status bits
hipError_t launch_build_compact_redo(const uint32_t* d_count, uint32_t n, uint32_t* d_redo_idx, uint32_t* d_redo_n, hipStream_t s);
hipError_t launch_build_links(const BuildView& b, uint32_t first, uint32_t n, int cur_level, const uint32_t* d_rows, const float* d_dist,
                              const uint32_t* d_count, const float* d_self, uint64_t* d_keys_a, uint64_t* d_keys_b, uint32_t* d_hist,
                              uint32_t* d_seg_start, uint32_t* d_counters, uint32_t merge_grid, hipStream_t s);

hipError_t launch_build_heads(const uint64_t* d_sorted, uint32_t n_keys, uint32_t* d_seg_start, uint32_t* d_seg_n, hipStream_t s);

// Delete on a device-resident graph (qv_graph_remove.hip).  d_work: [3][n_work] (node, level, place in the call's list) of every
// list of the m listed nodes; d_snode ascending with d_srank the place of each; keys: n_work * max(max_m0, max_m) each; *d_seg_n zeroed.
// The lists of the survivors are compacted; launch_graph_tombstone then marks the listed nodes dead.
hipError_t launch_graph_remove(const BuildView& b, uint32_t n_nodes, const uint32_t* d_work, uint32_t n_work, const uint32_t* d_snode,
                               const uint32_t* d_srank, uint32_t m, uint64_t* d_keys_a, uint64_t* d_keys_b, uint32_t* d_hist,
                               uint32_t* d_seg_start, uint32_t* d_seg_n, uint32_t grid, hipStream_t s);
hipError_t launch_graph_tombstone(int8_t* d_level, const uint32_t* d_snode, uint32_t m, hipStream_t s);
// the same for ONE node of level `level` (a host's Delete): one launch, nothing uploaded; d's own lists are left as they are
hipError_t launch_graph_remove_one(const BuildView& b, uint32_t n_nodes, uint32_t d, int level, hipStream_t s);
hipError_t launch_graph_tombstone_one(int8_t* d_level, uint32_t d, hipStream_t s);
// the lists of n (node, level) pairs: degree [n] and links [n][max(max_m0, max_m)]; degree 0 for a dead node or a level it lacks
hipError_t launch_export_lists(const GraphView& g, const uint32_t* d_nodes, const int* d_levels, uint32_t n, uint32_t* d_deg_out,
                               uint32_t* d_links_out, hipStream_t s);

// distance of one query to n listed rows (lane == listed row, sequential accumulation)
hipError_t launch_distance_rows(const IndexView& v, const float* d_query, const uint32_t* d_rows, uint32_t n,
                                float* d_dist_out, hipStream_t s);
// one pair on the HOST (qv_distance_pair): the kernels' own pair_distance<M> compiled for the CPU
float host_pair_distance(int metric, const float* a, const float* b, uint32_t dim);
// n independent pairs a[i], b[i] (row-major [n][dim])
hipError_t launch_distance_pairs(int metric, const float* d_a, const float* d_b, uint32_t n, uint32_t dim,
                                 float* d_out, hipStream_t s);

}  // namespace qv
