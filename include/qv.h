/*
 * qv.h — C ABI of libqv, the MI355X (gfx950) similarity-search hot path for Quiver.
 *
 * This is the drop-in boundary: the entry points below are exactly what a cgo
 * binding for the reference's flat-scan / neighbour-distance path would bind
 * (INTEGRATION.md shows the Go side).  No torch types, no C++ types: plain
 * pointers and sizes.  Each entry point cites the reference interface it
 * replaces (paths relative to the reference tree).
 *
 * Conventions
 *   - every function returns QV_OK (0) or a negative qv_status; it never aborts.
 *     qv_last_error() returns a thread-local message whose wording follows the
 *     reference's error strings (pkg/hybrid/exact.go:45,49,101,105).
 *   - the device sees dense uint32 row numbers (the analogue of
 *     hnsw.Node.VectorIndex, pkg/hnsw/hnsw.go:94); string ids stay in the host
 *     language.
 *   - vectors are COPIED on add (copy-on-insert, pkg/hybrid/exact.go:53-56); no
 *     caller pointer is retained after a call returns (cgo pointer rule).
 *   - result ordering: distance ascending, ties by row ascending.  The reference
 *     leaves tie order unspecified (Go map iteration + unstable sort,
 *     pkg/hybrid/exact.go:115,124); this is a deterministic refinement of it.
 *   - qv_index_search*, qv_distance_rows* are thread-safe and may run
 *     concurrently (the reference runs Index.Search under a read lock,
 *     pkg/core/collection.go:647); add / remove / reserve / destroy need external
 *     exclusion (the reference holds c.Lock there, pkg/core/collection.go:139).
 *   - concurrent SMALL host-pointer searches on one handle (qv_index_search,
 *     qv_sharded_search, qv_graph_search) share device passes: one query per call
 *     from many threads is all the reference's host ever sends (collection.go:647;
 *     DB.BatchSearch's batch branch type-asserts the reference's own wrapper,
 *     pkg/core/db.go:726-727, and otherwise fans out single searches, :805-828).
 *     A call that finds the handle busy joins the calls that arrived during the
 *     running pass; together they are the next pass — one multi-query launch.  No
 *     timer: a lone caller runs at once, exactly as if there were no sharing.
 *     A scan of 256 MiB or more runs one pass at a time; a smaller index (where a
 *     single-query pass leaves most of the device idle) up to four side by side.
 *     Results are the same bits either way (every path is exact).
 *   - "_device" variants take device pointers and a hipStream_t (passed as
 *     void*), enqueue work and return without synchronising, so a caller can keep
 *     queries and results resident in HBM and time with HIP events.
 *   - rows are float32 at this seam.  arrowindex.Graph keeps float64 vectors
 *     (pkg/arrowindex/graph.go:136-140, :796-858); its only producer in the
 *     reference, ArrowHNSWIndex, widens float32 columns (index/arrow_hnsw.go:
 *     222-225), for which QV_L2SQ_F64 over float32 rows is lossless.  Genuine
 *     float64 input is narrowed on add: the host layer warns
 *     (quiver_amd/arrowindex.py), nothing fails silently.
 *   - platform: the library is built for MI355X hosts — Linux on x86-64.  The
 *     front that lets concurrent callers share passes waits on futex words and
 *     spins with the x86 PAUSE instruction (quiver_amd/csrc/qv_coalesce.h); the
 *     library never modifies the process environment (GPU_MAX_HW_QUEUES is the
 *     host's to set: INTEGRATION.md).
 */
#ifndef QV_H
#define QV_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QV_ABI_VERSION 4

typedef struct qv_index qv_index; /* opaque; owns device memory */

/* Distance metrics.  0..4 restate pkg/vectortypes/distances.go:12-104 (float64
 * accumulation, one rounding to float32; SquaredEuclidean is all-float32).
 * 5..7 restate pkg/hnsw/adapter.go:105-167 (float32 sequential accumulation),
 * the functions a reloaded collection uses (pkg/core/db.go:181-188). */
typedef enum qv_metric {
    QV_COSINE      = 0, /* vectortypes.CosineDistance            distances.go:12-40  */
    QV_L2          = 1, /* vectortypes.EuclideanDistance         distances.go:43-55  */
    QV_L2SQ        = 2, /* vectortypes.SquaredEuclideanDistance  distances.go:60-72  */
    QV_DOT         = 3, /* vectortypes.DotProductDistance        distances.go:77-90  */
    QV_L1          = 4, /* vectortypes.ManhattanDistance         distances.go:93-104 */
    QV_COSINE_F32  = 5, /* hnsw.CosineDistanceFunc               adapter.go:105-136  */
    QV_L2_F32      = 6, /* hnsw.EuclideanDistanceFunc            adapter.go:139-151  */
    QV_DOT_F32     = 7, /* hnsw.DotProductDistanceFunc           adapter.go:154-165  */
    QV_L2SQ_F64    = 8, /* ArrowHNSWIndex.Search re-score        index/arrow_hnsw.go:124-132
                           (float64 difference, float64 unfused square-accumulate)   */
    QV_METRIC_COUNT = 9
} qv_metric;

typedef enum qv_status {
    QV_OK                 =  0,
    QV_ERR_INVALID_ARG    = -1,
    QV_ERR_DIM_MISMATCH   = -2, /* "vector dimension mismatch" / "query dimension mismatch" */
    QV_ERR_K_NOT_POSITIVE = -3, /* "k must be positive" (exact.go:104-106; adapter.go:42-44) */
    QV_ERR_OUT_OF_RANGE   = -4, /* row id >= size */
    QV_ERR_NO_DEVICE      = -5, /* no HIP device / HIP runtime failure at create time */
    QV_ERR_DEVICE         = -6, /* HIP error during a call (message carries hipGetErrorString) */
    QV_ERR_OOM            = -7,
    QV_ERR_UNSUPPORTED    = -8
} qv_status;

/* flags for qv_index_create */
#define QV_FLAG_NONE        0ull
#define QV_FLAG_ROWMAJOR    1ull /* also keep a row-major copy: fast single-row gathers for
                                    qv_distance_rows / HNSW traversal (hnsw.go:536-563) */
#define QV_FLAG_BF16_ROWS   2ull /* also keep a bfloat16 copy of the rows (+50 % memory): the batched path's filter reads it
                                    instead of the float32 rows (half the bytes); results are unchanged — the filter only
                                    selects candidates for the exact re-score */
#define QV_FLAG_NO_SCAN_PLANE 4ull /* cosine and dot indexes keep the bfloat16 copy by default (+dim * 2 bytes per row: 3080 -> 4616
                                    bytes per row at 768 dimensions) because the scan of a large corpus for 1 to 8 queries rejects rows
                                    on it and reads the float32 rows of the few survivors only (qv_index_set_bound_scan).  This
                                    flag leaves the copy out: memory and every search are as without that scan.  The copy is an
                                    accelerator, never a requirement: an index whose copy cannot be allocated carries on without it.
                                    Wherever they keep that copy by default, indexes whose dimension is a multiple of 16 up to 4096
                                    also keep an 8-bit plane of the rows with a scale and a residual per row (+dim + 8 bytes per
                                    row: 4616 -> 5392 at 768 dimensions), on which a single query rejects rows first — unfiltered
                                    (qv_index_set_bound_plane) or under a mask, a row set or a where-filter
                                    (qv_index_set_bound_plane_filtered).  This flag leaves out both; an 8-bit plane that cannot be
                                    allocated is given up alone and searches start on the bfloat16 copy.  A Euclidean index created
                                    with QV_FLAG_L2_SCAN_PLANE keeps the same planes; this flag beside that one wins: no planes */
#define QV_FLAG_L2_SCAN_PLANE 8ull /* a QV_L2 index keeps what cosine and dot indexes keep by default — the bfloat16 copy, and for a
                                    dimension that is a multiple of 16 up to 4096 the 8-bit plane with its scale and residual per row
                                    (+3 * dim + 8 bytes per row) — in the same layout, refreshed by the same calls, given up in the
                                    same way when an allocation fails.  Its searches of 1 to 8 queries for k <= 64 can then take the
                                    bound scan (qv_index_set_bound_scan and the plane setters govern it unchanged), with the exact
                                    scan's rows and float32 bits.  The automatic rules take such an index from the shapes measured
                                    for it (profiles/LAB_r14_bound_scan_l2.md): dot's floors, except that one unfiltered query on rows
                                    narrower than 768 dimensions waits for 10M rows, and a filtered search for nine tenths of the tiles
                                    holding a candidate.  On every other metric the flag does nothing; QV_L2SQ, QV_L2_F32 and QV_L2SQ_F64 keep no
                                    planes.  QV_FLAG_BF16_ROWS alone on a QV_L2 index stays a copy for the batched filter: no bound scan */
#define QV_FLAG_NO_PLANE6 32ull  /* wherever they keep the 8-bit plane, indexes whose dimension is a multiple of 64 also keep a 6-bit plane of the rows
                                    with a residual per row (+dim * 0.75 + 4 bytes per row: 5392 -> 5972 at 768 dimensions; the scale is the 8-bit
                                    plane's), on which a single unfiltered query rejects rows before the 8-bit plane is read for the few
                                    thousand rows left (qv_index_set_bound_plane6).  This flag leaves that plane out alone;
                                    QV_FLAG_NO_SCAN_PLANE leaves it out with the others.  A 6-bit plane that cannot be allocated is given up
                                    alone and searches start on the 8-bit plane; it is never kept without the 8-bit plane */
#define QV_FLAG_GRAPH_PLANE 16ull /* a QV_FLAG_ROWMAJOR index of metric QV_COSINE or QV_DOT whose dimension is a multiple of 64 up to 4096
                                    also keeps `rowmaj16`: a bfloat16 copy of the rows in ROW order, [rows][dim] (+dim * 2 bytes per row:
                                    7688 -> 9224 at 768 dimensions for an index that serves flat, graph and batch), each element the
                                    round-to-nearest-even conversion the per-row residual |r - bf16(r)| is measured against, written by
                                    every call that writes rows.  A graph traversal can then reject neighbours on it
                                    (qv_graph_set_reject_plane).  Opt-in: without the flag nothing is kept and every traversal launches the
                                    kernels it always launched.  Without QV_FLAG_ROWMAJOR, on another metric or another dimension the flag
                                    does nothing and creation still succeeds; a copy that cannot be allocated is given up alone */
#define QV_FLAG_GRAPH_PLANE8 64ull /* a QV_FLAG_ROWMAJOR index of metric QV_COSINE or QV_DOT whose dimension is a multiple of 128 up to 4096
                                    also keeps `rowmaj8`: the rows' int8 image in ROW order, [rows][dim] — the bytes qv_scan_quantize_row8 gives,
                                    the tile-layout 8-bit plane's where the index holds one — and one 16-byte record per row beside it,
                                    {double rnorm; float rscale8; float rres8} (+dim + 16 bytes per row), written by every call that writes
                                    rows.  A graph traversal can then reject neighbours on it (qv_graph_set_reject_image).  Independent of
                                    QV_FLAG_GRAPH_PLANE (an index may hold either image or both) and of QV_FLAG_NO_SCAN_PLANE (the image
                                    derives its own scale and residual).  Opt-in: without the flag nothing is kept and nothing is launched
                                    differently.  Without QV_FLAG_ROWMAJOR, on another metric or another dimension the flag does nothing
                                    and creation still succeeds; an image that cannot be allocated is given up alone */
/* FOR THE qv_scan_* RULE FUNCTIONS ONLY: "a QV_L2 index created with QV_FLAG_L2_SCAN_PLANE", where they take a metric.  They accept it
 * wherever they accept QV_COSINE and QV_DOT (plain QV_L2 keeps answering 0); qv_index_metric still answers QV_L2, and qv_index_create
 * rejects the code. */
#define QV_RULE_L2_PLANES 0x101

/* ---- lifecycle ------------------------------------------------------------------ */

/* Replaces hybrid.NewExactIndex(distFunc) (pkg/hybrid/exact.go:29-35) plus the
 * dimension lock-in of the first Insert (exact.go:43-47): dim is fixed here.
 * device = HIP device ordinal the index lives on (one index = one GPU = one shard). */
int qv_index_create(qv_index** out, uint32_t dim, qv_metric metric, int device, uint64_t flags);
void qv_index_destroy(qv_index* idx);

/* Pre-size device storage for `rows` rows (amortises growth; optional). */
int qv_index_reserve(qv_index* idx, uint64_t rows);

/* ---- mutation ------------------------------------------------------------------- */

/* Replaces ExactIndex.Insert / HybridIndex.InsertBatch data movement
 * (exact.go:38-58; hybrid_index.go:132-242): append n host rows [n][dim] (row-major
 * float32), copied to the device.  *first_row_out = row number of rows[0]; the
 * others follow contiguously. */
int qv_index_add(qv_index* idx, const float* rows, uint32_t n, uint32_t* first_row_out);

/* Same, rows already on the device (Arrow IPC values buffer -> device path,
 * index/arrow_hnsw.go:222-225).  Synchronous w.r.t. `stream`. */
int qv_index_add_device(qv_index* idx, const float* d_rows, uint32_t n, uint32_t* first_row_out, void* stream);

/* Append n synthetic unit rows generated on the device by the counter-based
 * generator documented in DESIGN.md (synthetic corpus); global row number of the first
 * generated row is `gen_row0` (so shards of one corpus agree).  Benchmark/test
 * helper: keeps 30 GB corpora off PCIe. */
int qv_index_add_synthetic(qv_index* idx, uint64_t seed, uint64_t gen_row0, uint32_t n, uint32_t* first_row_out);

/* Replaces ExactIndex.Delete (exact.go:61-70) / HNSW tombstoning (hnsw.go:829):
 * rows are tombstoned, never renumbered.  Removing a dead row is not an error
 * (exact.go:65 never errors). */
int qv_index_remove(qv_index* idx, const uint32_t* rows, uint32_t n);

/* Overwrite one live or dead row in place and mark it live (Collection.Update
 * path, pkg/core/collection.go:~400: delete + insert under one lock). */
int qv_index_update(qv_index* idx, uint32_t row, const float* vec);

/* Overwrite n listed rows in one call (Collection.UpdateBatch, pkg/core/collection.go:469-529; slot reuse in
 * HybridIndex.InsertBatch).  The result is exactly what
 *     for (i = 0; i < n; i++) qv_index_update(idx, rows[i], vecs + i * dim);
 * leaves: every listed row is overwritten in place and marked live (a dead row is revived), a row listed more than
 * once ends with its LAST vector, and every plane the index derives from its rows holds, bit for bit, what the loop
 * would have left.  rows is HOST memory in both forms; vecs is host [n][dim], d_vecs device [n][dim].
 * Checked before anything is written: a null index, rows or vectors (QV_ERR_INVALID_ARG; n == 0 returns QV_OK
 * before the two lists are looked at); any rows[i] >= qv_index_rows -> QV_ERR_OUT_OF_RANGE, nothing changed.
 * When a call fails with QV_ERR_DEVICE the contents of the listed rows are unspecified; their alive bits as the
 * index reports them (qv_index_size, the checks of later calls) are what they were before the call.
 * The device form is synchronous w.r.t. `stream`.  The host form stages the vectors through the index's own buffer
 * in chunks of at most 256 MiB; entries whose row comes again later in the list are dropped before the list is cut,
 * so no chunk writes a row another chunk writes.  Threading: as qv_index_add / qv_index_update — the caller keeps
 * every other call on the index out while one of these runs. */
int qv_index_update_rows(qv_index* idx, const uint32_t* rows, uint32_t n, const float* vecs);
int qv_index_update_rows_device(qv_index* idx, const uint32_t* rows, uint32_t n, const float* d_vecs, void* stream);

/* The rule behind both (pure host arithmetic, no device): the entries that survive (the last of each row), sorted by
 * row — rows_out[m] ascending and distinct, src_out[i] = the position in the list of rows_out[i]'s vector — and the
 * 64-row tiles they touch: tiles_out[T] ascending, tile_first_out[T + 1] = where each tile's entries start in
 * rows_out (tile_first_out[T] = m).  Room for n, n, n + 1 and n entries; *n_unique = m, *n_tiles = T. */
int qv_update_rows_plan(const uint32_t* rows, uint32_t n, uint32_t* rows_out, uint32_t* src_out, uint32_t* tile_first_out,
                        uint32_t* tiles_out, uint32_t* n_unique, uint32_t* n_tiles);

/* ---- queries -------------------------------------------------------------------- */

/* Number of rows ever added (dead rows included) and number of live rows
 * (= ExactIndex.Size, exact.go:136-141). */
uint32_t qv_index_rows(const qv_index* idx);
uint32_t qv_index_size(const qv_index* idx);
uint32_t qv_index_dim(const qv_index* idx);
int      qv_index_metric(const qv_index* idx);

/* Replaces ExactIndex.Search (exact.go:92-133) for nq queries at once
 * (HybridIndex.BatchSearch, hybrid_index.go:677-811, is nq independent searches).
 *   queries  [nq][dim] host float32
 *   k        > 0; clamped to the live size (exact.go:109-111); may equal the size
 *            (filtered search asks for a full ranking, collection.go:679-682)
 *   rows_out [nq][k], dist_out [nq][k]  caller-allocated; entries past count are
 *            row = 0xFFFFFFFF, dist = +inf
 *   count_out[nq] = min(k, live size); empty index -> 0 results, QV_OK (exact.go:96-98)
 * Order of checks follows exact.go:96-106: empty -> ok; then k <= 0 -> error.
 * How k is served (same result whichever applies): up to 64 results the scan keeps a sorted list per wavefront; up to 128 —
 * the negative-example branches fetch max(2k, 30), hybrid_index.go:516-522 — two keys per lane in that list; up to 8192 one
 * key per row and a radix SELECTION of the k smallest; beyond (k = Size() of a filtered search) the full radix ranking.
 * Batches of 9+ queries (32+ with the fp32 filter) over a large corpus go through the matrix-core filter + exact re-score up to
 * 4096 results per query. */
int qv_index_search(qv_index* idx, const float* queries, uint32_t nq, uint32_t k,
                    uint32_t* rows_out, float* dist_out, uint32_t* count_out);

/* How the calls of qv_index_search were served since the index was created.  out[0] solo = calls that ran at once in their own
 * context; out[1] led / out[2] rode = calls that ran a group / had their results written by its leader; out[3] groups, out[4]
 * group_queries = passes that carried a group and the queries in them; out[5] lingers, out[6] linger_ns = groups held open for
 * callers the previous pass had just released, and the time that took in all; out[7] group_pass_ns = time inside the groups'
 * device calls.  For reports and tests. */
int qv_index_coalesce_stats(qv_index* idx, uint64_t out[8]);
/* One more counter of the same front (kept out of out[8] so that ABI 4 callers' arrays stay the size they are): groups whose first
 * pass handed part of their members their results before the rest were redone (the filter's hand-backs inside a group). */
int qv_index_coalesce_early_rounds(qv_index* idx, uint64_t* out);

/* Same with device-resident queries/results; enqueues on `stream`, no sync. */
int qv_index_search_device(qv_index* idx, const float* d_queries, uint32_t nq, uint32_t k,
                           uint32_t* d_rows_out, float* d_dist_out, void* stream);

/* Filtered exact search: only rows whose bit is set in `mask` (bit r%64 of word r/64; host memory,
 * ceil(qv_index_rows/64) words) are candidates.  This is the row-bitmap form of a filtered
 * Collection.Search (collection.go:679-759 ranks ALL rows — searchK = Index.Size() — and keeps the first k
 * whose metadata matches; when the match set is known up front the same k results come from a top-k over
 * the matching rows, without producing or downloading the full ranking).  count_out[q] =
 * min(k, live rows selected by mask); other arguments and ordering as qv_index_search.  Up to 8 queries and 64 results of a
 * cosine / dot index take the bound scan on the bfloat16 copy over the candidates under the modes of qv_index_set_bound_scan
 * (the rule: qv_scan_bound_applies_filtered), with the exact scan's rows and bits. */
int qv_index_search_masked(qv_index* idx, const float* queries, uint32_t nq, uint32_t k, const uint64_t* mask,
                           uint32_t* rows_out, float* dist_out, uint32_t* count_out);

/* ---- row sets: device-resident filters, one per query ------------------------------
 * A filtered Collection.Search (collection.go:679-759) carries its own filter, and real filters come from a small
 * vocabulary of facet predicates (pkg/facets: equality, range, set) that requests reuse.  A qv_rowset is such a
 * predicate's match set as a row bitmap of ONE index, uploaded once and resident on the index's device; searches name
 * it by handle, and every query of a call may name a different one.
 *   create      mask = ceil(qv_index_rows/64) host words (bit r%64 of word r/64), copied; null = the empty set.
 *               The set is NOT intersected with the live rows: tombstones set later (qv_index_remove) and rows
 *               revived later (qv_index_update) are honoured by every search; selecting a dead row selects nothing.
 *   growth      a set stays valid as its index grows: rows added after the set was created (or last extended by
 *               qv_rowset_set_rows) are unselected.  No search ever reallocates a set.
 *   set_rows    selected != 0 adds the listed rows to the set, 0 drops them; a row >= qv_index_rows is
 *               QV_ERR_OUT_OF_RANGE (nothing is changed then).
 *   count       rows selected, dead ones included.
 * Threading: searches naming a set may run concurrently; qv_rowset_set_rows / qv_rowset_destroy need external
 * exclusion against searches that name that set (the index's mutations need it anyway) — for the device-pointer form
 * that includes searches still enqueued on the caller's stream: destroy frees the words without waiting for the
 * device.  The index must outlive its sets. */
typedef struct qv_rowset qv_rowset;
int qv_rowset_create(qv_rowset** out, qv_index* idx, const uint64_t* mask);
int qv_rowset_set_rows(qv_rowset* rs, const uint32_t* rows, uint32_t n, int selected);
uint64_t qv_rowset_count(const qv_rowset* rs);
void qv_rowset_destroy(qv_rowset* rs);

/* qv_index_search_masked with one set PER QUERY: sets is a host array of nq handles, a null entry = every row.
 * Query q gets the first k of the full (distance, row) ranking restricted to the live rows of sets[q] — the rows,
 * float32 bits, order, padding and check order of qv_index_search_masked with that set as its mask;
 * count_out[q] = min(k, live rows in sets[q]); an empty intersection is 0 results and QV_OK.  A set of another index,
 * or a null `sets` with nq > 0, is QV_ERR_INVALID_ARG.  Up to 64 results per query the queries of a call share corpus
 * passes, 4 / 8 / 16 per pass (16 from 9 queries on, for the metrics that accumulate in float64), each masked by its
 * own set, and a tile none of the pass's sets selects is not read at all; above
 * 64, runs of consecutive queries naming the same set go through the selection / ranking paths of qv_index_search over
 * a candidate bitmap formed on the device.  Concurrent calls of up to 8 queries share passes like qv_index_search's
 * (a front of their own: qv_index_rowset_coalesce_stats, laid out as qv_index_coalesce_stats).  A call (or shared pass) of 1 - 8
 * queries, k <= 64, takes the bound scan on the bfloat16 copy under the modes of qv_index_set_bound_scan, query j restricted to
 * live & sets[j] (qv_scan_bound_applies_filtered is the rule; qv_index_bound_scan_stats counts these searches too): same rows, bits,
 * order, counts and padding; a set holding fewer than k live rows is answered by the exact scan, decided on the device. */
int qv_index_search_rowsets(qv_index* idx, const float* queries, uint32_t nq, uint32_t k, const qv_rowset* const* sets,
                            uint32_t* rows_out, float* dist_out, uint32_t* count_out);
/* Device-pointer form: queries / results on the device, `sets` still a HOST array of handles (read before the call
 * returns).  Enqueues on `stream`, no synchronisation, nothing about a set is uploaded; every list is k long, padded
 * with 0xFFFFFFFF / +inf past the query's matches. */
int qv_index_search_rowsets_device(qv_index* idx, const float* d_queries, uint32_t nq, uint32_t k, const qv_rowset* const* sets,
                                   uint32_t* d_rows_out, float* d_dist_out, void* stream);
int qv_index_rowset_coalesce_stats(qv_index* idx, uint64_t out[8]);

/* ---- facet columns: row sets from predicates, set algebra, on the device -------------
 * A qv_rowset_create needs a bitmap the HOST has already evaluated.  A qv_column keeps one typed value per row of ONE
 * index on that index's device, beside the vectors, so that a filter value nobody has asked for before is one kernel
 * pass over the columns (qv_rowset_create_where) instead of a walk over every row's metadata, an upload and a
 * synchronisation; and two sets are combined where they live (qv_rowset_combine).  The sets these calls make are
 * ordinary row sets: the same words, host mirror and counts that qv_rowset_create leaves for the same bitmap, so every
 * search that names a set takes them alike.
 *   types       QV_COL_F64: a JSON number as Go decodes it (float64).  QV_COL_U32: a dictionary code or rank the host
 *               assigns (strings, bools, "%v" forms); ranks in sorted string order turn string < / > into unsigned
 *               comparisons.
 *   set         values[n] (double or uint32_t by type) for rows [first_row, first_row + n); present[n] bytes, 0 = the
 *               row has no value (null = all present).  first_row + n <= qv_index_rows, else QV_ERR_OUT_OF_RANGE and
 *               nothing changes.  Rows never set, and rows added to the index later, have no value.  Overwrites in
 *               place; grows like a row set (no search or evaluation reallocates).  Synchronous.
 *   rows        the column's extent: one past the last row ever set.
 * Threading: evaluations naming a column may run concurrently; qv_column_set / qv_column_destroy need external
 * exclusion against them.  The index must outlive its columns. */
typedef struct qv_column qv_column;
#define QV_COL_F64 0
#define QV_COL_U32 1
int qv_column_create(qv_column** out, qv_index* idx, int type);
int qv_column_set(qv_column* col, uint32_t first_row, uint32_t n, const void* values, const uint8_t* present);
uint32_t qv_column_rows(const qv_column* col);
void qv_column_destroy(qv_column* col);

#define QV_PRED_EQ 0      /* F64: fabs(x - v) <= 1e-9 in float64 (valuesEqual, collection.go:600-607); U32: x == v */
#define QV_PRED_NE 1      /* the negation of EQ on rows that HAVE a value */
#define QV_PRED_LT 2
#define QV_PRED_LE 3
#define QV_PRED_GT 4
#define QV_PRED_GE 5      /* plain IEEE / unsigned comparisons (compareValues, :609-632) */
#define QV_PRED_IN 6      /* EQ against any of 1..256 literals */
#define QV_PRED_NOT_IN 7  /* EQ against none of them */
#define QV_PRED_PRESENT 8 /* no literal (facets.NewExistsFilter) */
#define QV_PRED_ABSENT 9  /* no literal */
/* The set of rows r < qv_index_rows for which EVERY predicate p holds: cols[p] ops[p] literals[lit_off[p] .. lit_off[p+1])
 * (lit_off has n_preds + 1 entries, lit_off[0] = 0, ascending).  Literals are doubles for both column types (a uint32 code is
 * exact in a double; a U32 literal that is not an integer in [0, 2^32) is QV_ERR_INVALID_ARG).  EQ .. GE take exactly one
 * literal, IN / NOT_IN 1..256, PRESENT / ABSENT none.  A row without a value in cols[p] fails p for every op except ABSENT
 * (NE and NOT_IN included, as matchesFilter returns false for a missing field, collection.go:533-536); a column shorter
 * than the index has no value for the rows past its extent.  1 <= n_preds <= 8; a column of another index, an op out of
 * range, or a wrong literal count is QV_ERR_INVALID_ARG.  One kernel pass: a 64-row tile whose word is already zero
 * after predicate p reads nothing of the columns after it, so put the most selective predicate first.  Like
 * qv_rowset_create the set is NOT intersected with the live rows.  Synchronous (the words are read back for the host
 * mirror: rows / 8 bytes); threading as qv_rowset_create. */
int qv_rowset_create_where(qv_rowset** out, qv_index* idx, const qv_column* const* cols, const int* ops,
                           const double* literals, const uint32_t* lit_off, uint32_t n_preds);
#define QV_SET_AND 0
#define QV_SET_OR 1
#define QV_SET_ANDNOT 2
/* dst = a OP b, word by word on the device; dst may be a or b; all three of one index, else QV_ERR_INVALID_ARG.  A set
 * shorter than the index (made before it grew) reads as zeros past its end; dst is extended to the index's current rows.
 * Synchronous; exclusion as qv_rowset_set_rows for dst. */
int qv_rowset_combine(qv_rowset* dst, const qv_rowset* a, const qv_rowset* b, int op);
/* The set's words AS THE DEVICE HOLDS THEM (qv_rowset_count reads the host mirror: tests compare the two): the first
 * min(n_words, the set's words) 64-row words into words_out, zeros after them.  Synchronous. */
int qv_rowset_read(const qv_rowset* rs, uint64_t* words_out, uint32_t n_words);

/* ---- filtered search by predicate, in one call ---------------------------------------
 * A filter that carries a per-request literal (price < 37.5, ts >= now - 1h, an IN list from the user) is never asked
 * twice: making a qv_rowset for it costs an allocation, a pass on the null stream, a download of rows / 8 bytes for the
 * host mirror and a synchronisation, in front of the search, and a destroy behind it.  qv_index_search_where takes the
 * conjunction itself, one per query: a qv_where is the argument list of qv_rowset_create_where, and query q gets exactly
 * what qv_index_search_rowsets returns when sets[q] is the set qv_rowset_create_where makes from filters[q] — the same
 * rows, float32 bits, (distance, row) order, counts and padding; tombstones honoured, a column shorter than the index has
 * no value past its extent, a row without a value fails every op but ABSENT.  n_preds == 0: every row (a null set).
 * The sets live in the call's workspace only: no qv_rowset is created, nothing runs on the null stream, nothing but the
 * results is downloaded, and once the call's buffers have grown nothing is allocated or freed.  All filters of a call
 * (or of a shared pass) are evaluated in front of the scan by launches of up to QV_WHERE_FILTERS_PER_LAUNCH conjunctions
 * each; bytewise-equal filters are evaluated once.  Everything the qv_where structs point to is read before the call returns.
 * Checks, in order: a null index / queries / count_out / filters; an empty index -> 0 results and QV_OK; k == 0 ->
 * QV_ERR_K_NOT_POSITIVE; then every filter by qv_rowset_create_where's own check (same codes and wording, the message
 * prefixed with the query's number).
 * Routing: the host does not know how many rows a filter selects.  One query is planned as for a set that may select every
 * tile; a call or shared pass of several queries holding such a filter is declined by QV_BOUND_SCAN_AUTO and takes the exact
 * row-set scan (QV_BOUND_SCAN_ALWAYS still takes the bound scan); a filter that selects fewer than k rows is answered by the
 * exact scan, decided on the device.  A mis-route costs time, never bits.
 * k > 64 (host form only): runs of consecutive queries with bytewise-equal filters are materialised as a temporary row
 * set (this may synchronise), take the selection / ranking paths of qv_index_search_rowsets, and the set is freed before
 * the call returns.
 * Calls of up to 8 queries and k <= 64 share passes with each other AND with concurrent qv_index_search_rowsets calls
 * (the same front: qv_index_rowset_coalesce_stats counts them). */
typedef struct qv_where {                /* one conjunction: the arguments of qv_rowset_create_where */
    const qv_column* const* cols;
    const int* ops;
    const double* literals;
    const uint32_t* lit_off;
    uint32_t n_preds;
} qv_where;
#define QV_WHERE_FILTERS_PER_LAUNCH 8    /* conjunctions one evaluation launch carries (their tables are kernel arguments) */
#define QV_WHERE_DEVICE_LITERALS 16      /* literals ONE filter of the device-pointer form may carry in total */
int qv_index_search_where(qv_index* idx, const float* queries, uint32_t nq, uint32_t k, const qv_where* filters /* host, [nq] */,
                          uint32_t* rows_out, float* dist_out, uint32_t* count_out);
/* Device-pointer form: queries / results on the device, `filters` a HOST array (read before the call returns).  Enqueues
 * on `stream`, no synchronisation; every list is k long, padded with 0xFFFFFFFF / +inf past the query's matches.  The
 * predicate tables AND the literals travel as kernel arguments, so that no staging buffer exists which a later call
 * could overwrite while this one is still enqueued: a filter whose literals number more than QV_WHERE_DEVICE_LITERALS
 * (an EQ or a range needs 1 - 2; a long IN list does not fit) is QV_ERR_UNSUPPORTED, and so is k > 64 — both decided on
 * the host before anything is enqueued (use the host form, or qv_rowset_create_where + qv_index_search_rowsets_device).
 * Check order: null arguments, k == 0, k > 64, every filter as above, the literal limit; an empty index pads every list. */
int qv_index_search_where_device(qv_index* idx, const float* d_queries, uint32_t nq, uint32_t k, const qv_where* filters /* HOST, [nq] */,
                                 uint32_t* d_rows_out, float* d_dist_out, void* stream);

/* Search with a negative example, the device part of HybridIndex.searchWithStrategy's exact branch
 * (hybrid_index.go:517-570; the HNSW adapter's is adapter.go:345-437): the k_fetch = max(2k, 30) nearest rows of `query`
 * (as qv_index_search), and for exactly those rows the distance to `negative` (as qv_distance_rows) — one call, one
 * synchronisation, the row ids never leave the device in between.  The host forms score = d - w * d_neg in float32
 * (:549) and sorts the <= k_fetch records by (score, id) (:552-557).  Outputs are [k_fetch]; *count_out = min(k_fetch, size). */
int qv_index_search_negative(qv_index* idx, const float* query, const float* negative, uint32_t k_fetch,
                             uint32_t* rows_out, float* dist_out, float* neg_dist_out, uint32_t* count_out);

/* Batched-query path: approximate scores by a GEMM on the matrix cores with a proven error margin (one bfloat16 MFMA
 * term up to 1536 dimensions, three exact-product bfloat16 terms above; qv_index_set_filter chooses otherwise) and
 * fused per-tile candidate selection, then exact re-scoring of the candidates with the same arithmetic as
 * qv_index_search, so results are identical to it.  Same arguments as qv_index_search. */
int qv_index_search_batched(qv_index* idx, const float* queries, uint32_t nq, uint32_t k,
                            uint32_t* rows_out, float* dist_out, uint32_t* count_out);

/* Which filter kernel the batched path of this index uses: QV_FILTER_AUTO (the rule above), QV_FILTER_FP32_MFMA (the dense
 * fp32 GEMM on v_mfma_f32_32x32x2_f32, BASELINE configs[2] as written), QV_FILTER_BF16X3, QV_FILTER_BF16X1, or QV_FILTER_OFF
 * (qv_index_search never takes the batched path; qv_index_search_batched* answer QV_ERR_UNSUPPORTED / fall back).  Results are
 * identical whichever runs (the filter only selects candidates for the exact re-score).  Needs external exclusion against
 * running searches, like the mutations.  The environment variable QV_MFMA_FILTER (read once per process) sets the default of
 * indexes that never call this. */
#define QV_FILTER_AUTO      0
#define QV_FILTER_FP32_MFMA 1
#define QV_FILTER_BF16X3    2
#define QV_FILTER_BF16X1    3
#define QV_FILTER_OFF       4   /* no filter: every batch of this index takes the exact scans (what tests of those scans choose) */
int qv_index_set_filter(qv_index* idx, int filter);

/* ---- filtered batches: 9 or more queries, a filter per query, on the batched path ----
 * A call — or a pass that concurrent callers share — of 9 or more queries, k <= 64, through qv_index_search_rowsets or
 * qv_index_search_where can take the batched path above instead of ceil(nq / 8) or ceil(nq / 16) exact corpus passes: the sample bound
 * is taken over each query's own set, the matrix-core filter walks the corpus once for all of them, a candidate outside its query's
 * set is dropped where it leaves the filter kernel, and the exact re-score ranks what is left.  Query q gets exactly what the exact
 * filtered scan returns for live & set_q: rows, float32 bits, (distance, row) order, counts and padding.  The filter is a qv_rowset, a
 * null set or a qv_where conjunction, mixed freely; metrics and shapes are those of the batched path (cosine, dot, L2, L2SQ; never an
 * index under QV_FILTER_OFF); any nq, a remainder of up to 64 queries beyond a multiple of 256 as a pass of its own.
 * A query the path cannot decide — more candidates than its list holds, a guessed bound that failed its check — and a query whose set
 * is SPARSE are handed back to the exact row-set scan, alone; the others keep their answers.  Sparse: the filter kernels test every
 * row against every query's threshold whatever the sets say, so the work a set causes grows as the inverse of its share of the rows;
 * below `sparse_ppm` millionths of the rows the exact scan is the cheaper answer.  The share is counted on the device, on the sample,
 * per query (a where-filter's is known nowhere else); the host counts a qv_rowset's selected rows, and a piece goes batched only when
 * at least 9 of its queries are not known sparse that way — those that are ride along, in place, and come back through the same flag.
 * A mis-route costs time, never bits.
 *   mode         QV_FILTERED_BATCH_ALWAYS: whenever the above holds.  QV_FILTERED_BATCH_NEVER: the exact passes, as before this setter
 *                existed.  QV_FILTERED_BATCH_AUTO (the default): only shapes measured faster than the exact passes by more than both
 *                arms' spread, never below 300 000 rows; see qv_batched_applies_filtered.  The environment variable
 *                QV_FILTERED_BATCH (1 always, 2 never; read once per process) sets the default of indexes that never call this.
 *   sparse_ppm   0 .. 1000000; 0 = never hand a query back as sparse; 0xFFFFFFFF = the default (10 000: a hundredth of the rows).
 * Needs external exclusion against running searches, like the other setters.
 * Out of scope, all unchanged: the device-pointer forms (qv_index_search_rowsets_device, qv_index_search_where_device: nobody reads the
 * redo flags there), qv_index_search_masked with 9 or more queries, k > 64, qv_sharded_*, and skipping tiles in the filter (it reads
 * every row whatever the sets select). */
#define QV_FILTERED_BATCH_AUTO   0
#define QV_FILTERED_BATCH_ALWAYS 1
#define QV_FILTERED_BATCH_NEVER  2
int qv_index_set_filtered_batch(qv_index* idx, int mode, uint32_t sparse_ppm);
/* out[0] = QUERIES that took the filtered batched path so far, out[1] = queries it handed back for an overflowing candidate list, no
 * bound or a failed guess, out[2] = queries it handed back as sparse, out[3] = batches.  Counted when a call returns; does not wait. */
int qv_index_filtered_batch_stats(qv_index* idx, uint64_t out[4]);
/* The dispatch's own rule, without an index or a device: would a piece of nq filtered queries, k results each, over `rows` rows of
 * `dim` dimensions take the batched path under `filter` (QV_FILTER_*) and `mode` (QV_FILTERED_BATCH_*; AUTO reads QV_FILTERED_BATCH
 * first)?  n_not_sparse: how many of the piece's queries the host does not know to be sparse — a null set counts, a qv_where counts
 * (the device decides), a qv_rowset counts when selected / rows is at or above the floor.  1 / 0, < 0 on an argument error.  NEVER: 0.
 * Any mode: 0 for fewer than 9 queries or 9 not-sparse ones, k > 64, a metric or shape the batched path does not take, QV_FILTER_OFF.
 * AUTO: 0 below 300 000 rows; beyond, only cells measured faster by more than both arms' spread.  The cells measured so far
 * (profiles/LAB_r15_filtered_batch.md: 300k and 1M x 768, one call) are wins by 1.3 - 20 x for random sets and predicates, and losses
 * for one tile-aligned set named by every query, which these arguments cannot tell apart; 10M rows and 128 dimensions are
 * unmeasured.  So AUTO takes nothing yet: ask for the path with QV_FILTERED_BATCH_ALWAYS.  Monotone in n_not_sparse. */
int qv_batched_applies_filtered(int metric, uint32_t dim, uint64_t rows, uint32_t nq, uint32_t k, int filter, int mode, uint32_t n_not_sparse);
/* Which main filter kernel a FILTERED batch of that shape launches, without an index or a device: the batched path's plan for (metric,
 * dim, rows, nq, k, filter), then the substitution a batch with sets applies where the planned kernel has no variant that tests the
 * sets (the register-resident one: the bfloat16-copy kernel or the 256-row eight-wave kernel instead).  has_bf16_plane: the index was
 * created with QV_FLAG_BF16_ROWS; cus: the device's compute units (the kernel chosen does not depend on them).  *nq_pad: the query
 * count the batch is padded to (64, 128 or a multiple of 256); *kernel: one of QV_BATCHED_FILTER_*.  Environment switches read once
 * per process apply as they do to a search.  QV_ERR_UNSUPPORTED where no filtered batch runs: k > 64, too few queries or rows for the
 * batched path, a metric it does not take, QV_FILTER_OFF.  For tests and reports: says nothing about mode or the sparse floor. */
#define QV_BATCHED_FILTER_MFMA_F32      0   /* float32 matrix-core chain (QV_FILTER_FP32) */
#define QV_BATCHED_FILTER_BF16X3        1   /* three bfloat16 terms, a wave per query block: up to 128 padded queries, or a one-term shape no other kernel takes */
#define QV_BATCHED_FILTER_BF16X3_SHARED 2   /* three bfloat16 terms, whole workgroups of 256 queries sharing rows */
#define QV_BATCHED_FILTER_BF16ROWS      3   /* one term on the index's bfloat16 copy, whole workgroups */
#define QV_BATCHED_FILTER_W8X2          4   /* one term on float32 rows, eight waves, 256 rows per round */
#define QV_BATCHED_FILTER_W8X2_PADDED   5   /* the same with zero-padded steps: dimensions its loop does not divide */
#define QV_BATCHED_FILTER_Q64_PLANE     6   /* one term, one block of 64 queries, on the bfloat16 copy */
#define QV_BATCHED_FILTER_Q64_F32_ROWS  7   /* one term, one block of 64 queries, on float32 rows */
int qv_batched_filter_route(int metric, uint32_t dim, uint64_t rows, uint32_t nq, uint32_t k, int filter, int has_bf16_plane, int cus,
                            uint32_t* nq_pad, int* kernel);
/* What the batched path's plan chose for the sample of a batch of nq queries, k results: its rows; the step of its 128-row groups —
 * sample position i is row (i / 128) * group_step * 128 + i % 128 of the corpus; and the rank its bound is taken at (k, or more under
 * a guessed bound).  QV_ERR_UNSUPPORTED when this index has no such route.  For tests and reports. */
int qv_batched_sample_plan(qv_index* idx, uint32_t nq, uint32_t k, uint32_t* sample_rows, uint32_t* group_step, uint32_t* rank);

/* The single-query scan that rejects rows on the bfloat16 copy (cosine, dot, and QV_L2 indexes created with QV_FLAG_L2_SCAN_PLANE;
 * 1 <= k <= 64, a dimension that is a multiple of 16): stage 1 streams the copy, derives a certified interval of every row's distance and ends with the k-th smallest upper
 * bound; the rows whose lower bound is within it (k plus a handful) get their distances from the float32 rows in the scan's own
 * arithmetic.  Results are
 * bit-identical to the exact scan's; when the bound cannot decide (too many survivors, a query whose norm is not a number, huge or
 * vanishing) the exact scan answers instead, decided on the device.  QV_BOUND_SCAN_AUTO: from the measured row count on;
 * QV_BOUND_SCAN_ALWAYS: whenever the copy exists and the shape applies; QV_BOUND_SCAN_NEVER.  The environment variable
 * QV_BOUND_SCAN (1 always, 2 never; read once per process) sets the default of indexes that never call this.
 * Filtered searches (qv_index_search_masked, qv_index_search_rowsets and its device form) take the bound scan under the same modes:
 * ALWAYS whenever the shape applies, NEVER never, AUTO by qv_scan_bound_applies_filtered (the measured shapes).
 * qv_sharded_search_masked keeps the exact scan. */
#define QV_BOUND_SCAN_AUTO   0
#define QV_BOUND_SCAN_ALWAYS 1
#define QV_BOUND_SCAN_NEVER  2
int qv_index_set_bound_scan(qv_index* idx, int mode);
/* The same scan as a SHARED pass: 2 to 8 queries of one call — or of concurrent callers whose queries were put together — read the
 * copy once (4 or 8 queries per pass).  Interval, threshold and exact re-score are per query, so every answer is bit-identical to
 * the exact scan's, and a query the bound cannot decide is handed back alone: the others of the pass keep their answers.  Same
 * conditions and the same setter; no mask, no row set, k <= 64.  Automatic mode takes it only from the measured shapes on (a floor
 * on rows and on the dimension: every query writes and reads 8 bytes per row whatever the width), and leaves short corpora to the
 * form they had. */
/* out[0] = survivors stage 1 passed on in the last such search (after a shared pass: the largest count among its queries),
 * out[1] = QUERIES handed back to the exact scan so far, out[2] = QUERIES that took the path so far (a shared pass of nq adds nq),
 * out[3] = 1 when the index holds the bfloat16 copy.  Waits for the device. */
int qv_index_bound_scan_stats(qv_index* idx, uint64_t out[4]);
/* Which plane serves a single unfiltered query's bound scan FIRST.  With the 8-bit plane (see QV_FLAG_NO_SCAN_PLANE) stage 1 reads
 * a quarter of the float32 bytes: integer dot products of the quantised query with the row's int8 image, a certified interval from
 * the row's stored scale and residual, the same threshold, collection and exact re-score.  A search that stage cannot decide (more
 * candidates than its list holds, no finite threshold, a query it cannot quantise) goes on to the bfloat16 stage, and from there, if
 * need be, to the exact scan — all decided on the device; results are bit-identical to the exact scan's in every case.
 * QV_BOUND_PLANE_AUTO: the 8-bit stage from its measured row count and width on (never below the bound scan's own floor);
 * QV_BOUND_PLANE_8BIT: whenever the bound scan takes the search and the plane is held; QV_BOUND_PLANE_BF16: never.  Independent of
 * qv_index_set_bound_scan, which decides WHETHER a search takes the bound scan; this decides which plane it starts on.  The
 * environment variable QV_BOUND_PLANE (1 8-bit, 2 bfloat16; read once per process) sets the default of indexes that never call this.
 * This setter speaks of unfiltered searches only: a single masked, row-set or where-filtered query has a setter of its own
 * (qv_index_set_bound_plane_filtered), an unfiltered shared pass of 2 - 8 queries too (qv_index_set_bound_plane_mq), and so has a shared
 * pass under a mask, row sets or where-filters (qv_index_set_bound_plane_filtered_mq).  qv_sharded_search_masked keeps the exact scan. */
#define QV_BOUND_PLANE_AUTO 0
#define QV_BOUND_PLANE_8BIT 1
#define QV_BOUND_PLANE_BF16 2
int qv_index_set_bound_plane(qv_index* idx, int mode);
/* out[0] = survivors the 8-bit stage passed on in the last such search, out[1] = searches it handed on to the bfloat16 stage so far,
 * out[2] = searches that took the 8-bit stage so far, out[3] = 1 when the index holds the 8-bit plane.  Waits for the device.
 * qv_index_bound_scan_stats keeps its meaning: a search the 8-bit stage took counts as a bound-scan search there, and its hand-backs
 * are the searches that reached the exact scan. */
int qv_index_bound_scan8_stats(qv_index* idx, uint64_t out[4]);
/* ---- the 6-bit stage in front of the 8-bit one ----
 * Whether a single UNFILTERED query that would start on the 8-bit plane starts on the 6-bit plane instead (see QV_FLAG_NO_PLANE6):
 * stage 1 reads three quarters of the 8-bit bytes with an interval about four times as wide, its candidates (tens of thousands of 10M
 * rows) are refined on the 8-bit plane by a gather, and the 8-bit stage's collection and exact re-score finish as ever.  A search the
 * 6-bit stage cannot decide (more than 262 144 candidates, no finite threshold, a query it cannot quantise) goes on to the bfloat16
 * stage — all decided on the device; results are bit-identical to the exact scan's in every case.  QV_BOUND_PLANE6_AUTO: the shapes
 * measured faster than 8-bit first (qv_scan_bound6_applies), never below the 8-bit stage's floor; QV_BOUND_PLANE6_ALWAYS: whenever the
 * 8-bit stage would be first and the plane is held; QV_BOUND_PLANE6_NEVER: never.  Independent of the other setters; filtered searches
 * and shared passes are not moved by it.  The environment variable QV_BOUND_PLANE6 (1 always, 2 never; read once per process) sets the
 * default of indexes that never call this. */
#define QV_BOUND_PLANE6_AUTO 0
#define QV_BOUND_PLANE6_ALWAYS 1
#define QV_BOUND_PLANE6_NEVER 2
int qv_index_set_bound_plane6(qv_index* idx, int mode);
/* out[0] = candidates the 6-bit stage passed to the refine in the last such search, out[1] = searches it handed on to the bfloat16 stage
 * so far, out[2] = searches that took the 6-bit stage so far, out[3] = 1 when the index holds the 6-bit plane.  Waits for the device.
 * qv_index_bound_scan8_stats and qv_index_bound_scan_stats keep their meaning: such a search counts as an 8-bit search there. */
int qv_index_bound_scan6_stats(qv_index* idx, uint64_t out[4]);
/* Whether a search would take the 6-bit stage first — the dispatch's own rule, on the host: qv_scan_bound8_applies(metric, dim, rows, nq, k,
 * mode, plane_mode, has_plane8) true, one query, the 6-bit plane held (has_plane6; a dimension that is a multiple of 64), and plane6_mode
 * (QV_BOUND_PLANE6_*).  It never says yes where qv_scan_bound8_applies says no.  AUTO: the cells measured faster
 * (profiles/LAB_r20_bound_scan6.md).  1 / 0, < 0 on an error. */
int qv_scan_bound6_applies(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, int plane_mode, int plane6_mode, int has_plane8, int has_plane6);
/* One row as the index keeps it in the 6-bit plane (dim a multiple of 64): codes c6_i = clamp(rint(r_i / (4 scale8)), -32, 31) stored
 * biased (c6 + 32) in six bits; out_bytes[dim * 3 / 4]: per group of 64 dimensions the row's three 16-byte pieces X, Y, Z — dims 0 - 47 of
 * the group in the low six bits of their bytes, dims 48 - 63 as three 2-bit parts (bits 0 - 1, 2 - 3, 4 - 5 of the code) in the top two bits
 * of the bytes of X, Y, Z.  scale8: the row's 8-bit scale (qv_scan_quantize_row8).  *out_res = |r - 4 scale8 c6| computed in float64 from
 * those codes and rounded up — NaN for a row qv_scan_quantize_row8 declines.  The interval: qv_scan_bound_interval8 with
 * isum = sum qq_i (c6_i + 32) - 32 sum qq_i, rscale8 = 4 scale8, rres8 = *out_res. */
int qv_scan_quantize_row6(uint32_t dim, const float* row, float scale8, uint8_t* out_bytes, float* out_res);
/* ... and those bytes back into the biased codes, out_codes[dim] in 0 .. 63. */
int qv_scan_unpack_row6(uint32_t dim, const uint8_t* bytes, uint8_t* out_codes);
/* ---- the wide form: 65 to 1024 results ----
 * The single-query, unfiltered bound scan for 65 <= k <= 1024 (the k <= 64 form's metrics and widths: cosine, dot, QV_L2 indexes created
 * with QV_FLAG_L2_SCAN_PLANE; a dimension that is a multiple of 16 up to 4096; 8 tiles or more; more live rows than results; an index of
 * at most 64M rows).  Stage 1 is the k <= 64 form's, on the bfloat16 copy or the 8-bit plane, but publishes every wave's 64 smallest upper
 * bounds; the threshold is the k-th smallest of their union — the upper bounds of k distinct live rows cap the k-th distance, so every row
 * of the answer has its lower bound within it; it is the exact k-th smallest upper bound unless one wave's rows hold more than 64 of the
 * k smallest, and only looser then.  The rows within it — at most QV_BOUND_WIDE_CAND_CAP — get their distances from the float32 rows in
 * the scan's own arithmetic and a selection takes the k best.  Rows, float32 bits, (distance, row) order, counts and padding are the exact
 * path's.  A search it cannot decide (more survivors than the list holds, fewer than k rows the bound is sure of, a query whose norm is
 * not a number, huge or vanishing) goes from the 8-bit stage to the bfloat16 stage and from there to the key-per-row exact path, all
 * decided on the device.  qv_index_search, qv_index_search_device and qv_index_search_negative reach it.
 * `mode` takes the QV_BOUND_SCAN_* values.  ALWAYS: whenever the shape applies.  NEVER: never.  AUTO: the measured cells in which the wide
 * form ran ahead of the exact path at every measured k (65, 100, 128, 129, 256, 1000) by more than both arms' spread
 * (profiles/LAB_r24_bound_scan_wide.md, tests/bench/bench_bound_scan_wide.py; 1M, 3M and 10M x 768 and 10M x 128, cosine — every one of
 * them): cosine and dot indexes, k <= 1000, from 1 000 000 rows of 768 dimensions or more and from 10 000 000 rows of 128 to 767
 * dimensions.  NOT measured and therefore never automatic: fewer than 1M rows, fewer than 128 dimensions, 128 to 767 dimensions below
 * 10M rows, k above 1000, QV_L2 indexes with the planes; ALWAYS reaches the path there.  Independent of qv_index_set_bound_scan, whose
 * rule (qv_scan_bound_applies) keeps saying no above k = 64.  Which plane comes first follows qv_index_set_bound_plane:
 * QV_BOUND_PLANE_8BIT the 8-bit plane where it is held, QV_BOUND_PLANE_BF16 the bfloat16 copy, QV_BOUND_PLANE_AUTO the 8-bit plane in
 * the cells where it also beat the bfloat16 copy first by the same standard (all of the cells above), the bfloat16 copy elsewhere.
 * The environment variable QV_BOUND_SCAN_WIDE (1 always, 2 never; read once per process) sets the default of indexes that never call this.
 * Out of scope and unchanged: the 6-bit plane, k > 1024, and the sharded handle (qv_sharded_* keeps its paths; there is no sharded
 * setter).  The filtered form and the shared pass of 2 to 8 queries have knobs of their own: qv_index_set_bound_scan_wide_filtered and
 * qv_index_set_bound_scan_wide_mq, below; this knob never reaches two or more queries. */
#define QV_BOUND_WIDE_CAND_CAP 8192   /* rows the wide form's re-score walks at most: 1024 + 4032 (the k <= 64 form's spare over its largest k) and room to the next power of two */
int qv_index_set_bound_scan_wide(qv_index* idx, int mode);
/* out[0] = survivors passed to the re-score in the last wide search, out[1] = searches handed back to the exact path so far, out[2] =
 * searches that took the wide form so far, out[3] = 1 when the index holds the bfloat16 copy.  Waits for the device.
 * qv_index_bound_scan_stats, qv_index_bound_scan8_stats and qv_index_bound_scan6_stats do not move for wide searches. */
int qv_index_bound_scan_wide_stats(qv_index* idx, uint64_t out[4]);
/* Whether a search would take the wide form — the dispatch's own rule, on the host (the dispatch adds what only the index knows: more
 * LIVE rows than results).  metric as qv_scan_bound_applies takes it, QV_RULE_L2_PLANES included; wide_mode: QV_BOUND_SCAN_*;
 * plane_mode: QV_BOUND_PLANE_*; has_plane / has_plane8: the index holds the bfloat16 copy / the 8-bit plane.
 * 0: no wide form; 1: the bfloat16 copy first; 2: the 8-bit plane first; < 0 on an error (an unknown mode). */
int qv_scan_bound_wide_route(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int wide_mode, int plane_mode, int has_plane, int has_plane8);
/* ---- the wide form under a filter ----
 * ONE filtered query asking for 65 to 1024 results — qv_index_search_masked, qv_index_search_rowsets, qv_index_search_rowsets_device and
 * qv_index_search_where (whose k > 64 form makes its filter a counted set first) — answered by the wide form over the call's candidate
 * bitmap (live & selected): stage 1 reads no 64-row tile without a candidate, rows outside the filter are never candidates and never in
 * the threshold, and the collect, the re-score, the selection and the gated key-per-row redo read the same bitmap.  Rows, float32 bits,
 * counts and padding are those of the path the call takes otherwise (the filtered wide scan up to 128 results, the key-per-row path above).
 * On top of the unfiltered form's conditions the call needs a tile with a candidate and MORE live candidates than results: a k that takes
 * every candidate has nothing to reject, and a shorter set keeps its path and its clamped count.  The counters are the wide form's own
 * (qv_index_bound_scan_wide_stats); the k <= 64 counters do not move.
 * `mode` takes the QV_BOUND_SCAN_* values and is a knob of its own: independent of qv_index_set_bound_scan_wide, of qv_index_set_bound_scan
 * and of the plane knobs.  ALWAYS: whenever the shape applies.  NEVER: never.  AUTO: the measured cells in which the form ran ahead of the
 * path the filtered call takes today at every measured k (65, 100, 128, 129, 256, 1000) by more than both arms' spread
 * (profiles/LAB_r25_bound_scan_wide_filtered.md, tests/bench/bench_bound_scan_wide_filtered.py; 1M, 3M and 10M x 768 and 10M x 128, cosine,
 * filters that leave a candidate in every tile, in 0.476 of the tiles and in one tile in ten — every one of them), never a shape the
 * unfiltered rule (qv_scan_bound_wide_route under AUTO) declines: cosine and dot indexes, k <= 1000, from 1 000 000 rows of 768 dimensions
 * or more and from 10 000 000 rows of 128 to 767 dimensions, with a candidate in at least one 64-row tile in ten.  NOT measured and never
 * automatic: sparser filters, and everything the unfiltered rule leaves out (QV_L2 indexes, fewer rows, k above 1000).  Which plane comes
 * first follows qv_index_set_bound_plane_filtered: QV_BOUND_PLANE_8BIT the 8-bit plane where it is held, QV_BOUND_PLANE_BF16 the bfloat16
 * copy, QV_BOUND_PLANE_AUTO the 8-bit plane in the cells where it also beat the bfloat16 copy first by the same standard — 768 dimensions
 * or more: from 3 000 000 rows at one tile in ten or denser, below that only with a candidate in every tile; 128 to 767 dimensions (from
 * 10 000 000 rows): a candidate in at least 0.475 of the tiles — and the bfloat16 copy elsewhere.
 * The environment variable QV_BOUND_SCAN_WIDE_FILTERED (1 always, 2 never; read once per process) sets the default of indexes that never
 * call this — the per-shard indexes of a sharded handle among them; there is no sharded setter, and the sharded handle's filtered search
 * (an internal call without the stream's ticket words) keeps its path whatever the variable says.
 * Out of scope and unchanged: qv_index_search_where_device keeps its k <= 64 limit (its candidate count exists only on the device, and the
 * selection paths need k <= count); runs of two or more queries naming one set keep their shared key-per-row pass; filtered shared
 * passes at k > 64 (the unfiltered ones: qv_index_set_bound_scan_wide_mq). */
int qv_index_set_bound_scan_wide_filtered(qv_index* idx, int mode);
/* The filtered form's rule on the host, as the dispatch asks it.  Arguments as qv_scan_bound_wide_route's; plane_mode_filtered:
 * QV_BOUND_PLANE_* of qv_index_set_bound_plane_filtered; candidate_tiles: the 64-row tiles that hold a candidate; candidates: the live
 * rows the filter selects.  0: no wide form; 1: the bfloat16 copy first; 2: the 8-bit plane first; < 0 on an error (an unknown mode). */
int qv_scan_bound_wide_route_filtered(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int wide_mode, int plane_mode_filtered, int has_plane, int has_plane8,
                                      uint32_t candidate_tiles, uint64_t candidates);
/* ---- the wide form of a shared pass: 2 to 8 queries, 65 to 1024 results ----
 * ONE unfiltered call of 2 to 8 queries asking for 65 <= k <= 1024 results — qv_index_search, qv_index_search_device and whatever reaches
 * them with that many queries, such as the short tail of a device batch — answered by the shared bound pass's wide form: the bfloat16 copy
 * or the 8-bit plane is read ONCE for the pass (the stage-1 kernels of the k <= 64 shared pass, publishing every wave's 64 smallest upper
 * bounds of every query), and per query the single wide form's funnel follows: the threshold is the k-th smallest of the query's published
 * bounds, the rows within it — at most QV_BOUND_WIDE_CAND_CAP per query — get their distances from the float32 rows in the scan's own
 * arithmetic, and one selection over all the queries' lists takes the k best of each.  Rows, float32 bits, (distance, row) order, counts
 * and padding are the exact path's.  Every query has its own fate, decided on the device: one the 8-bit stage cannot decide (more
 * survivors than the list holds, fewer than k rows the bound is sure of, a query it cannot quantise) goes on, alone, to the bfloat16
 * stage, and one that stage cannot decide either (the same, or a norm that is not a number, huge or vanishing) is redone, alone, by the
 * key-per-row path, whose outputs are then that query's.  The shape: the single wide form's and the k <= 64 shared pass's limits — cosine,
 * dot, QV_L2 indexes created with QV_FLAG_L2_SCAN_PLANE; a dimension that is a multiple of 16 up to 4096; 8 tiles or more; more live rows
 * than results; an index of at most 64M rows; nq planes of lower bounds (256 bytes per query and 64-row tile) under 2 GiB.
 * `mode` takes the QV_BOUND_SCAN_* values and is a knob of its own: independent of qv_index_set_bound_scan_wide (which never reaches two
 * or more queries, as this one never reaches a single query), of qv_index_set_bound_scan and of the single-query plane knobs.  ALWAYS:
 * whenever the shape applies.  NEVER: never.  AUTO: only measured cells in which the form ran ahead of the key-per-row shared pass at every
 * measured k (65, 100, 128, 129, 256, 1000) and every measured nq of its class (2 - 4 queries; 5 - 8 queries) by more than both arms'
 * spread (profiles/LAB_r26_bound_scan_wide_mq.md, tests/bench/bench_bound_scan_wide_mq.py).  Those cells:
 * cosine and dot indexes, k <= 1000; 2 to 4 queries from 1 000 000 rows of 768 dimensions or more, 5 to 8 queries from 3 000 000 (at
 * 1M x 768 the bfloat16 copy first lost to the key-per-row pass with 8 queries at every k and with 5 at k = 1000), either from 10 000 000
 * rows of 128 to 767 dimensions.  NOT measured and therefore never automatic: fewer than 1M rows, fewer than 128 dimensions, 128 to 767
 * dimensions below 10M rows, k above 1000, QV_L2 indexes with the planes; ALWAYS reaches the path there.
 * Which plane comes first follows qv_index_set_bound_plane_mq: QV_BOUND_PLANE_8BIT the 8-bit plane where it is held, QV_BOUND_PLANE_BF16
 * the bfloat16 copy, QV_BOUND_PLANE_AUTO the 8-bit plane only in cells where it also beat the bfloat16 copy first by the same standard:
 * all of the cells above except 5 to 8 queries below 768 dimensions (at 10M x 128 it lost to the bfloat16 copy first with 8 queries).
 * The environment variable QV_BOUND_SCAN_WIDE_MQ (1 always, 2 never; read once per process) sets the default of indexes that never call
 * this.  Out of scope and unchanged: filtered shared passes at k > 64 (a mask, row sets, where-filters), coalescing concurrent single-query
 * callers at k > 64, 9 or more queries, k > 1024, the 6-bit plane, and the sharded handle (there is no sharded setter). */
int qv_index_set_bound_scan_wide_mq(qv_index* idx, int mode);
/* out[0] = the largest survivor count among the queries of the last wide shared pass, each query counted in the stage that ANSWERED it (a
 * maximum over the stages that answered: a query the 8-bit stage answered counts with that stage's survivors, one handed on with the
 * bfloat16 stage's, one handed back to the key-per-row path with nothing), out[1] = queries handed back to the key-per-row path so far,
 * out[2] = queries that took the form so far, out[3] = 1 when the index holds the bfloat16 copy.  Waits for the device.  No other
 * counter group moves for these passes, and these do not move for any other search. */
int qv_index_bound_scan_wide_mq_stats(qv_index* idx, uint64_t out[4]);
/* Whether a call of nq queries would take the wide shared pass — the dispatch's own rule, on the host (the dispatch adds what only the index
 * and the call know: more LIVE rows than results, an unfiltered call that carries its stream's ticket words).  Arguments as
 * qv_scan_bound_wide_route's; wide_mq_mode: QV_BOUND_SCAN_* of qv_index_set_bound_scan_wide_mq; plane_mode_mq: QV_BOUND_PLANE_* of
 * qv_index_set_bound_plane_mq.  0: no wide shared pass (always for nq < 2 or nq > 8); 1: the bfloat16 copy first; 2: the 8-bit plane
 * first; < 0 on an error (an unknown mode). */
int qv_scan_bound_wide_route_mq(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int wide_mq_mode, int plane_mode_mq, int has_plane, int has_plane8);
/* ---- the 8-bit stage under a filter ----
 * Which plane serves a single FILTERED query's bound scan first: qv_index_search_masked, qv_index_search_rowsets and
 * qv_index_search_where with one query, their device forms, and a shared pass of the row-set front that holds one caller — at
 * k <= 64, cosine or dot, a dimension that is a multiple of 16.  The 8-bit stage walks the call's candidate bitmap (live & set): a
 * 64-row tile without a candidate is not read at all, rows outside the set are never candidates and never in the threshold, and a
 * set with fewer than k live rows has no threshold in either stage and ends in the exact filtered scan, decided on the device.
 * Results are the exact filtered scan's rows and float32 bits in every case.  `mode` takes the QV_BOUND_PLANE_* values:
 * QV_BOUND_PLANE_8BIT whenever the filtered bound scan takes the search (qv_scan_bound_applies_filtered) and the plane is held;
 * QV_BOUND_PLANE_BF16 never; QV_BOUND_PLANE_AUTO (the default) the shapes measured faster — see qv_scan_bound8_applies_filtered.
 * Independent of qv_index_set_bound_plane; the same external exclusion as the other setters (no search of the index in flight).
 * The environment variable QV_BOUND_PLANE_FILTERED (1 8-bit, 2 bfloat16; read once per process) sets the default of indexes that
 * never call this.  qv_index_bound_scan8_stats counts these searches, their survivors and their hand-ons as it counts the
 * unfiltered ones.  FILTERED shared passes of 2 - 8 queries have a setter of their own (qv_index_set_bound_plane_filtered_mq); out of
 * scope: qv_sharded_search_masked keeps the exact scan. */
int qv_index_set_bound_plane_filtered(qv_index* idx, int mode);
/* ---- the 8-bit stage in front of a shared pass ----
 * Which plane serves an UNFILTERED shared pass of 2 - 8 queries first: qv_index_search and qv_index_search_device with 2 - 8 queries, the
 * passes that concurrent single-query callers share, and shards through their own index.  The 8-bit plane is read once for the 4 or 8
 * queries of the pass; interval, threshold, collection and exact re-score are per query, as in the single-query stage.  A query that
 * stage cannot decide (more candidates than its list holds, no finite threshold, a query it cannot quantise) is handed on ALONE to the
 * bfloat16 shared pass, whose launches are enqueued behind and leave at once when no query was handed on; from there, if need be, to
 * the exact scan — all decided on the device; every answer is bit-identical to the exact scan's.  `mode` takes the QV_BOUND_PLANE_*
 * values: QV_BOUND_PLANE_8BIT whenever the bound scan takes the pass and the plane is held; QV_BOUND_PLANE_BF16 never;
 * QV_BOUND_PLANE_AUTO (the default) the shapes measured faster — see qv_scan_bound8_applies_mq.  Independent of
 * qv_index_set_bound_plane and qv_index_set_bound_plane_filtered; the same external exclusion (no search of the index in flight).
 * The environment variable QV_BOUND_PLANE_MQ (1 8-bit, 2 bfloat16; read once per process) sets the default of indexes that never
 * call this.  A pass under a mask, row sets or where-filters is not moved by this setter: qv_index_set_bound_plane_filtered_mq.
 * Counters: qv_index_bound_scan8_stats out[0] = the largest survivor count among the pass's queries in the 8-bit stage, out[1] += the
 * queries handed on to the bfloat16 stage, out[2] += nq.  qv_index_bound_scan_stats counts the pass's nq queries once in out[2],
 * out[1] += the queries that reached the exact scan, out[0] = the largest survivor count in the stage that answered. */
int qv_index_set_bound_plane_mq(qv_index* idx, int mode);
/* ---- the 8-bit stage in front of a filtered shared pass ----
 * Which plane serves a FILTERED shared pass of 2 - 8 queries first: qv_index_search_masked (one bitmap for all queries),
 * qv_index_search_rowsets and qv_index_search_where with 2 - 8 queries (a set or a predicate per query), their device forms, and the
 * passes in which the row-set front puts concurrent filtered callers together — at k <= 64, cosine or dot, a dimension that is a multiple
 * of 16.  The 8-bit plane is read once for the pass, each query over its OWN candidates (live & set): a 64-row tile no query selects is
 * not read at all, a row outside a query's set is neither its candidate nor in its threshold.  A query that stage cannot decide (more
 * candidates than its list holds, no finite threshold, a query it cannot quantise, fewer than k candidates in its set) is handed on ALONE
 * to the filtered bfloat16 shared pass, whose launches are enqueued behind and leave at once when no query was handed on; from there, if
 * need be, to the exact filtered scan — all decided on the device; every answer is bit-identical to the exact filtered scan's.  `mode`
 * takes the QV_BOUND_PLANE_* values: QV_BOUND_PLANE_8BIT whenever the filtered bound scan takes the pass and the plane is held —
 * where-filters counted as "every tile may hold a candidate", so such a pass takes the bound scan, 8-bit first, whenever the filtered
 * bound rule accepts a pass over every tile; QV_BOUND_PLANE_BF16 never (routing is then what it was before this setter existed);
 * QV_BOUND_PLANE_AUTO (the default) the shapes measured faster — see qv_scan_bound8_applies_filtered_mq.  Independent of
 * qv_index_set_bound_plane, qv_index_set_bound_plane_filtered and qv_index_set_bound_plane_mq: none of those moves a filtered shared
 * pass, and this one moves nothing else.  The same external exclusion (no search of the index in flight).  The environment variable
 * QV_BOUND_PLANE_FILTERED_MQ (1 8-bit, 2 bfloat16; read once per process) sets the default of indexes that never call this.
 * Counters: as qv_index_set_bound_plane_mq's.  Out of scope: qv_sharded_search_masked keeps the exact scan, and there are no sharded
 * setters for this mode because shards have no row sets; 9 or more queries, k > 64 and other metrics are not covered. */
int qv_index_set_bound_plane_filtered_mq(qv_index* idx, int mode);
/* Whether a filtered shared pass would take the 8-bit stage first — the dispatch's own rule, on the host: 2 <= nq <= 8, the plane held
 * (has_plane8), qv_scan_bound_applies_filtered(metric, dim, rows, nq, k, mode, has_plane = 1, candidate_tiles) true (the stage never starts
 * a pass the filtered bound scan would not take), and plane_mode_filtered_mq (QV_BOUND_PLANE_*) not BF16.  8BIT: whenever those hold.
 * AUTO: only cells measured faster than starting on the bfloat16 copy at every measured k, never above what qv_scan_bound8_applies_mq
 * allows for the same nq (profiles/LAB_r13_bound_scan8_filtered_mq.md): rows of 768 dimensions or more, 3 000 000 rows or more, nine
 * tenths of the tiles or more holding a candidate of some query of the pass (null sets, sets of any density spread over the index,
 * where-filters); 1 000 000 rows lost at k = 64, sparser candidate tiles gained nothing to speak of at k = 64 and are declined.
 * 1 / 0, < 0 on an error. */
int qv_scan_bound8_applies_filtered_mq(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, int plane_mode_filtered_mq, int has_plane8,
                                       uint32_t candidate_tiles);
/* Whether a shared pass would take the 8-bit stage first — the dispatch's own rule, on the host: 2 <= nq <= 8, the plane held
 * (has_plane8), qv_scan_bound_applies(metric, dim, rows, nq, k, mode, has_plane = 1) true (the stage never starts a pass the bound scan
 * would not take), and plane_mode_mq (QV_BOUND_PLANE_*) not BF16.  8BIT: whenever those hold.  AUTO: the shapes measured faster than
 * starting on the bfloat16 copy at every measured k and nq of the pass's size class (2 - 4 or 5 - 8 queries) —
 * profiles/LAB_r12_bound_scan8_mq.md.  The route (qv_scan_route) is 1, bound_mq, either way: the plane is a decision inside it.
 * 1 / 0, < 0 on an error. */
int qv_scan_bound8_applies_mq(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, int plane_mode_mq, int has_plane8);
/* Whether a filtered search would take the 8-bit stage first — the dispatch's own rule, on the host: one query, the plane held
 * (has_plane8), qv_scan_bound_applies_filtered(metric, dim, rows, 1, k, mode, has_plane = 1, candidate_tiles) true (the stage never
 * starts a search the bound scan would not take), and plane_mode_filtered (QV_BOUND_PLANE_*) not BF16.  8BIT: whenever those hold.
 * AUTO: the shapes measured faster than starting on the bfloat16 copy at every measured k (profiles/LAB_r11_bound_scan8_filtered.md) —
 * rows of 768 dimensions or more, 3 000 000 rows or more, nine tenths of the tiles or more holding a candidate (a mask or set of
 * any density that is spread over the index, a where-filter); sparser candidate tiles lost or gained nothing at k = 64 and are
 * declined, narrower rows were not measured.  Never below the unfiltered 8-bit floors.  1 / 0, < 0 on an error. */
int qv_scan_bound8_applies_filtered(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, int plane_mode_filtered, int has_plane8,
                                    uint32_t candidate_tiles);
/* Whether a search would take the 8-bit stage first: qv_scan_bound_applies' conditions under `mode`, one query, the plane held
 * (has_plane8), and `plane_mode` (QV_BOUND_PLANE_*) — the dispatch's own rule, without an index or a device.  1 / 0, < 0 on an error. */
int qv_scan_bound8_applies(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, int plane_mode, int has_plane8);
/* The interval the 8-bit stage derives for one row, on the host (the kernel's own function): isum = sum qq_i r8_i, the integer dot
 * product of the quantised query (qq = rint(q / sq), sq = max|q_i| / 16256) with the row's bytes, qn = |query|, qres = |q - sq qq|
 * rounded up, rn = |row|, rscale8 / rres8 = the row's scale and residual (qv_scan_quantize_row8).  Returns 1 when the bound says
 * nothing about the row or the query (always a survivor), 0 otherwise with [*d_lo, *d_hi] containing the float32 distance, < 0 on an error.
 * metric: QV_COSINE, QV_DOT or QV_L2 (the interval does not depend on how an index was created); every other metric: QV_ERR_UNSUPPORTED. */
int qv_scan_bound_interval8(int metric, uint32_t dim, int64_t isum, double sq, double qn, double qres, double rn, float rscale8, float rres8, float* d_lo, float* d_hi);
/* One row as the index keeps it in the 8-bit plane: out_bytes[dim] = clamp(rint(r_i / scale), -127, 127), *out_scale = max|r_i| / 127
 * rounded up, *out_res = |r - scale r8| computed in float64 from those bytes and rounded up — NaN for a row the bound says nothing
 * about (a non-finite element, no non-zero element, a norm that is huge or vanishing). */
int qv_scan_quantize_row8(uint32_t dim, const float* row, int8_t* out_bytes, float* out_scale, float* out_res);
/* Whether a search of nq queries for k results over rows x dim of `metric` would take the path under `mode` (QV_BOUND_SCAN_*;
 * has_plane: the index holds the copy) — the dispatch's own rule, on the host, without an index or a device.  1 / 0, < 0 on an
 * error.  (A k above the live rows is the caller's to know; a mask or a row set: qv_scan_bound_applies_filtered.)  The metrics are
 * QV_COSINE, QV_DOT and the rule code QV_RULE_L2_PLANES (every one of these rule functions and qv_scan_route take it); the automatic mode
 * takes the last one from the shapes measured for it (dot's floors but for the two cases named at QV_FLAG_L2_SCAN_PLANE).  Plain QV_L2 and every other metric: 0. */
int qv_scan_bound_applies(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, int has_plane);
/* The same rule for a filtered search (qv_index_search_masked, qv_index_search_rowsets and its device form): candidate_tiles = how many
 * 64-row tiles hold a candidate of any query of the pass, as the host knows it without a device read — a row set counts its non-empty
 * words (tombstones are not subtracted), a null set every tile, a pass of several queries min(tiles, the sum over its queries); a mask the
 * non-empty words of live & mask.  QV_BOUND_SCAN_ALWAYS: whenever qv_scan_bound_applies' conditions hold (metric, whole 16-dimension
 * steps, k <= 64, 1 - 8 queries, the copy, 8 tiles or more); QV_BOUND_SCAN_NEVER: never; QV_BOUND_SCAN_AUTO: the shapes measured
 * faster than the exact filtered scan (profiles/LAB_r09_bound_scan_filtered.md) — rows of 768 dimensions or more; one query from
 * 300 000 rows with a tenth of the tiles or more; 2 - 4 queries from 1M rows with nine tenths of the tiles (from 10M: a fifth);
 * 5 - 8 queries from 1M rows with nine tenths of the tiles and k <= 10 (from 10M: any k) — never below the unfiltered floors and
 * never with candidate_tiles == 0.  (A row set that selects fewer than k rows counts as no candidate tile.) */
int qv_scan_bound_applies_filtered(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, int has_plane, uint32_t candidate_tiles);
/* Which kernels would answer a fused flat search (k <= 64) of nq queries over rows x dim of `metric` on a device of `cus` compute units —
 * the dispatch's own decision (plan_flat), on the host, without an index or a device.  tickets: the call carries its stream's ticket
 * words (the host-pointer and device-pointer searches do; the batched path's sample scan and the sharded paths do not); bound_mode /
 * plane_mode: QV_BOUND_SCAN_* / QV_BOUND_PLANE_*; has_plane / has_plane8: the index holds the bfloat16 copy / the 8-bit plane;
 * candidate_tiles: 0xFFFFFFFF for an unfiltered search, else as qv_scan_bound_applies_filtered takes it.  Returns the route in priority
 * order — 0 small, 1 bound_mq, 2 split_mq, 3 mq64, 4 mq, 5 bound, 6 bound8_first, 7 split, 8 fused, 9 two_launch —
 * or < 0 for arguments no route serves.  (More than 32 queries on route 3: the last 1 - 8 are split off as a pass of their own.) */
int qv_scan_route(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int cus, int tickets, int bound_mode, int plane_mode, int has_plane, int has_plane8,
                  uint32_t candidate_tiles);
/* qv_scan_route with the filtered plane mode as an argument (QV_BOUND_PLANE_*, as qv_index_set_bound_plane_filtered takes it): a filtered
 * single query that qv_scan_bound8_applies_filtered takes is route 6 (bound8_first), as route 5 serves both forms; unfiltered calls
 * do not depend on the argument.  qv_scan_route is this function with QV_BOUND_PLANE_BF16: a filtered call never on route 6. */
int qv_scan_route_ex(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int cus, int tickets, int bound_mode, int plane_mode, int has_plane, int has_plane8,
                     uint32_t candidate_tiles, int plane_mode_filtered);
/* How a search workspace is cut into regions, on the host, without an index or a device: the layout function the launcher itself takes
 * its pointers from, run on a null base.  kind: QV_WS_*; the shape as the layout sees it — rows x dim on a device of `cus` compute
 * units, nq queries, lists of k; `flags` per kind (below; 0 elsewhere).  *total: the bytes the caller must provide; *end: where the last
 * region ends (end <= total).  regions (may be null with cap 0): up to cap entries of four words in the layout's order — offset, bytes, the
 * alignment of the type read there, 1 for a region that overlays earlier ones (an alias) — and *n_regions how many the layout has.
 * The kinds' own arguments: QV_WS_MERGE_SELECT — `rows` = entries per gathered list, flags = lists; QV_WS_MERGE_RANKED — `rows` = keys;
 * QV_WS_FLAT (a fused flat search, k <= 64) — flags = QV_WS_FLAT_*: what lies behind the partial lists; QV_WS_ROWSETS_CALL /
 * QV_WS_WHERE_CALL (a shared pass of the device-pointer row-set / where searches, k <= 64, nq >= 2) — flags bit 0: sized for the
 * shared bound pass too, bits 8 and up (WHERE_CALL): distinct filters.  < 0 on an error. */
#define QV_WS_BOUND 0             /* the single-query bound scan */
#define QV_WS_BOUND_MQ 1          /* the shared bound pass of 2 - 8 queries */
#define QV_WS_REDO 2              /* the exact scan of flagged queries */
#define QV_WS_SELECT 3            /* the radix selection's own workspace */
#define QV_WS_FLAT_WIDE 4         /* 64 < k <= 128, one query: wave lists + selection */
#define QV_WS_FLAT_SELECT 5       /* a key per row + selection */
#define QV_WS_FLAT_SELECT_REDO 6  /* ... for flagged queries */
#define QV_WS_MERGE_SELECT 7      /* the sharded merge by selection */
#define QV_WS_MERGE_RANKED 8      /* the sharded merge by full sort */
#define QV_WS_FULL_SORT 9         /* the full ranking */
#define QV_WS_MQ64 10             /* the f64 matrix-core scan's query workspace */
#define QV_WS_ROWSET 11           /* the row-set scan */
#define QV_WS_FLAT 12             /* the fused flat search */
#define QV_WS_ROWSETS_CALL 13     /* the row-set workspace with the call's candidate bitmap behind it */
#define QV_WS_WHERE_CALL 14       /* ... with the candidate bitmap and the transient sets behind it */
#define QV_WS_BOUND_WIDE 15       /* the single-query bound scan's wide form, 65 <= k <= 1024; its exact redo's workspace is an alias over the rest */
#define QV_WS_BOUND_WIDE_MQ 16    /* the wide form of the shared bound pass, 2 - 8 queries, 65 <= k <= 1024; the pass's flag words first, the key-per-row redo's workspace an alias over the rest */
#define QV_WS_FLAT_PLAIN 0       /* query blocks, or the matrix-core scan's block */
#define QV_WS_FLAT_BOUND 1        /* ... or the single-query bound scan's buffer */
#define QV_WS_FLAT_BOUND_MQ 2     /* ... and the shared bound pass, which has the workspace to itself */
int qv_scan_workspace_layout(int kind, int metric, uint32_t dim, uint64_t rows, uint32_t nq, uint32_t k, int cus, uint32_t flags,
                             uint64_t* total, uint64_t* end, uint32_t* n_regions, uint64_t* regions, uint32_t cap);
/* The interval stage 1 derives for one row, on the host (the kernel's own function compiled for the CPU; metric QV_COSINE or
 * QV_DOT; every other metric: QV_ERR_UNSUPPORTED — QV_L2 included, whose interval is qv_scan_bound_interval_l2 below): s = the float32 chain of the query times the row's bfloat16 copy, qn = |query|, rn = |row|, rres = |row - bf16(row)|
 * rounded up.  Returns 1 when the row is one the bound says nothing about (always a survivor), 0 otherwise with
 * [*d_lo, *d_hi] containing the float32 distance, < 0 on an error. */
int qv_scan_bound_interval(int metric, uint32_t dim, float s, double qn, double rn, float rres, float* d_lo, float* d_hi);
/* The same for QV_L2: the interval of the Euclidean distance from the same stage-1 inputs (it does not depend on how an index was created).
 * An entry point of its own, because qv_scan_bound_interval has always answered QV_ERR_UNSUPPORTED for QV_L2 and keeps doing so;
 * qv_scan_bound_interval8 takes QV_L2 as a metric.  Same return values. */
int qv_scan_bound_interval_l2(uint32_t dim, float s, double qn, double rn, float rres, float* d_lo, float* d_hi);
/* FOR TESTS: one of the arrays ingest derives per row, copied to the host raw — no kernel, no decoding — after the device has
 * finished the index's work.  QV_DEBUG_RNORM: |r|, one double per row slot; QV_DEBUG_RRES: |r - bf16(r)| rounded up, one float per
 * row slot; QV_DEBUG_PLANE: the bfloat16 copy's bytes ([tile][16-dim step][32-row block][8-dim half][row of block][8 values]).
 * The extent is tiles in use x 64 slots (tiles in use x the copy's bytes per tile, 2 * 64 * 16 * ceil(dim / 16), for the copy); slots
 * past the last row and dead rows hold whatever was written there last.  QV_ERR_UNSUPPORTED for an array this index does not keep
 * (the copy without QV_FLAG_BF16_ROWS on a metric other than cosine / dot / QV_L2 with QV_FLAG_L2_SCAN_PLANE, under QV_FLAG_NO_SCAN_PLANE or after a failed
 * allocation; the residual and the norm on metrics whose ingest does not compute them), QV_ERR_INVALID_ARG when `bytes` is less
 * than the extent. */
#define QV_DEBUG_RNORM 0
#define QV_DEBUG_RRES  1
#define QV_DEBUG_PLANE 2
#define QV_DEBUG_PLANE6 4     /* the 6-bit plane, raw: [tile][dim / 64][3][64 rows][16 bytes] (qv_scan_quantize_row6's pieces); an index that keeps none: an unknown code */
#define QV_DEBUG_RRES6  5     /* |r - 4 rscale8 c6| rounded up, one float per row slot */
#define QV_DEBUG_RSCALE8 6    /* the 8-bit plane's scale, one float per row slot (indexes that keep the 6-bit plane) */
#define QV_DEBUG_PLANE8 7     /* the 8-bit plane, raw: [tile][dim / 16][64 rows][16 bytes]; an index that keeps none: an unknown code */
#define QV_DEBUG_RRES8  8     /* |r - rscale8 r8| rounded up (NaN: a row the bound declines), one float per row slot */
#define QV_DEBUG_ROWMAJ16 3  /* the row-order bfloat16 copy (QV_FLAG_GRAPH_PLANE), raw: rows x dim uint16, rows ever added; QV_ERR_UNSUPPORTED when an index created
                                 with the flag keeps none; an index created without the flag does not know the code (QV_ERR_INVALID_ARG, as before) */
#define QV_DEBUG_ROWMAJ8 9   /* the row-order 8-bit image (QV_FLAG_GRAPH_PLANE8), raw: rows x dim int8, rows ever added; QV_ERR_UNSUPPORTED when an index created
                                with the flag keeps none; an index created without the flag: an unknown code, as always */
#define QV_DEBUG_ROWMETA8 10 /* its records, rows ever added x {double rnorm; float rscale8; float rres8} (16 bytes); the same answers */
int qv_index_debug_read(qv_index* idx, int what, void* out, size_t bytes);

/* Device-pointer form of the batched path: enqueues on `stream`, no sync.  d_redo_flags_out[nq]
 * (uint32) is set to 1 for queries whose candidate buffer overflowed or — 16 or more results per query over 131 072 rows or
 * more, where the k-th distance's bound is a guess from a sample of 32 768 rows or more — whose guess did not hold (fewer than k candidates
 * within it): the caller must redo those with qv_index_search_device (their result rows are unspecified).  Returns QV_ERR_UNSUPPORTED when
 * the MFMA path does not apply (metric, k > 4096, small corpus, too few queries): use qv_index_search_device. */
int qv_index_search_batched_device(qv_index* idx, const float* d_queries, uint32_t nq, uint32_t k,
                                   uint32_t* d_rows_out, float* d_dist_out, uint32_t* d_redo_flags_out, void* stream);

/* Replaces the neighbour loop of HNSW.searchLayer (hnsw.go:536-563) and the
 * re-rank loops (hybrid_index.go:536-546; adapter.go:387-415): distance of one
 * query to n listed rows.  dist_out[i] = distance(query, row rows[i]); dead rows
 * are still evaluated (the reference skips nil nodes before calling). */
int qv_distance_rows(qv_index* idx, const float* query, const uint32_t* rows, uint32_t n, float* dist_out);
int qv_distance_rows_device(qv_index* idx, const float* d_query, const uint32_t* d_rows, uint32_t n,
                            float* d_dist_out, void* stream);

/* Replaces a vectortypes.DistanceFunc call (pkg/vectortypes/surface.go:8) for n
 * independent pairs a[i], b[i] (each [dim]); computed on the device `device`. */
int qv_distance_pairs(qv_metric metric, const float* a, const float* b, uint32_t n, uint32_t dim,
                      float* dist_out, int device);

/* The DistanceFunc contract for ONE pair, on the HOST: what a Go `vectortypes.DistanceFunc` wrapper calls
 * (surface.go:8; 78 ns per call in the reference, final_bench.txt:47 — no device round trip can serve a per-pair call).  Same
 * arithmetic, bit for bit, as qv_distance_pairs and the scans: it is the kernels' own per-pair routine compiled for the CPU.
 * Not a fallback: no search, scan or batch entry point uses it, and those fail without a GPU.  The length check (the reference
 * panics on len(a) != len(b), distances.go:13-15) stays in the host-language wrapper, which knows both lengths. */
int qv_distance_pair(qv_metric metric, const float* a, const float* b, uint32_t dim, float* out);

/* Deterministic merge of per-shard top-k lists (the exchange step of the sharded flat
 * scan: every rank all-gathers its k (distance, global row) pairs over RCCL, then
 * merges).  d_dist_lists / d_row_lists are [n_lists][k] device arrays, each list
 * sorted or not; output = the k smallest by (distance, row).  n_lists * k <= 65536.
 * No reference counterpart: the reference is single-process. */
int qv_merge_topk_device(const float* d_dist_lists, const uint32_t* d_row_lists, uint32_t n_lists, uint32_t k,
                         uint32_t* d_rows_out, float* d_dist_out, void* stream);

/* The same merge for the PACKED exchange buffer of a batch of nq queries: d_packed_lists = [n_lists][nq][2][k] 32-bit
 * words — per shard and query, k shard-local rows (0xFFFFFFFF = no result) followed by the k float32 distances —
 * exactly what a shard's qv_index_search_device wrote for the batch into one [nq][2][k] buffer, so that buffer goes
 * into a single all-gather untouched.  d_bases[n_lists] = first global row of each shard; outputs are [nq][k],
 * rows global.  n_lists * k <= 65536. */
int qv_merge_topk_shards_device(const uint32_t* d_packed_lists, const uint32_t* d_bases, uint32_t n_lists, uint32_t nq, uint32_t k,
                                uint32_t* d_rows_out, float* d_dist_out, void* stream);

/* Measurement aid: when enabled, every flat-scan kernel launched through
 * qv_index_search_device is bracketed by HIP events on the caller's stream;
 * qv_index_profile_read synchronises those events and returns the summed kernel
 * time and the number of launches since the last read.  Off by default.  The kernels of
 * qv_rowset_create_where and qv_rowset_combine are bracketed the same way (on the null stream). */
int qv_index_profile(qv_index* idx, int enable);
int qv_index_profile_read(qv_index* idx, double* scan_ms_sum_out, uint64_t* launches_out);

/* ---- device-resident HNSW traversal ------------------------------------------------
 * Replaces hnsw.HNSW.Search (pkg/hnsw/hnsw.go:602-713) for a batch of queries: the graph a
 * host-side HNSW built (levels + per-level adjacency, hnsw.go:44-56) is uploaded once, then
 * whole queries are walked on the GPU, one wavefront (or, few queries at a time, one workgroup) per query.  Node index
 * == row of `idx` (the index must hold the nodes' vectors; QV_FLAG_ROWMAJOR makes the
 * per-hop row gathers contiguous).  Results equal the reference's searchLayer semantics
 * exactly (same heaps, same admission order, bit-identical distances).
 *   levels     [n_nodes]            node level, -1 = tombstone (hnsw.go:829 Nodes[idx] = nil)
 *   l0_deg     [n_nodes]            level-0 degree;  l0_links [n_nodes][max_m0]
 *   up_off     [n_nodes]            first upper-level block of the node (level 1)
 *   up_links   [n_up_blocks][1+max_m]  per (node, level>=1): degree, then links
 * qv_graph_search: count_out[q] = results written (< k when the graph search under-filled:
 * the caller tops up like hnsw.go:676-710) or 0xFFFFFFFF when the candidate heap overflowed
 * (the caller must fall back to its host traversal).  evals_out (optional) = distance
 * evaluations per query. */
typedef struct qv_graph qv_graph;
int qv_graph_create(qv_graph** out, qv_index* idx, uint32_t n_nodes, const int8_t* levels, uint32_t max_m0, uint32_t max_m,
                    const uint32_t* l0_deg, const uint32_t* l0_links, const uint32_t* up_off, const uint32_t* up_links,
                    uint32_t n_up_blocks, uint32_t entry, int cur_level);
int qv_graph_search(qv_graph* g, const float* queries, uint32_t nq, uint32_t k, uint32_t ef_search,
                    uint32_t* rows_out, float* dist_out, uint32_t* count_out, uint32_t* evals_out);
/* qv_graph_search is thread-safe: the reference searches under a read lock (hnsw.go:602-606), one goroutine per query
 * (adapter.go:253-279).  Every call works in a context of its own (stream, visited sets, buffers: a pool); calls of up to 64
 * queries with the same k and ef_search that find two traversal batches in flight wait and form the next batch together
 * (256 queries at most).  A batch of at most one query per compute unit — a lone call, a shared batch — runs in the latency
 * form of the kernels: a workgroup of eight wavefronts per query, ~1.1 ms for one traversal of a 1M x 768 graph at efSearch 128
 * (3.1 ms as one wavefront); larger batches one wavefront per query, thousands in flight.  Same results either way.
 * qv_graph_insert / qv_graph_make_buildable / qv_graph_destroy need external exclusion against searches (the reference's
 * write lock).  qv_graph_coalesce_stats: as qv_index_coalesce_stats. */
int qv_graph_coalesce_stats(qv_graph* g, uint64_t out[8]);
int qv_graph_coalesce_early_rounds(qv_graph* g, uint64_t* out);
/* Device-pointer form: queries, results, counts (and optional evals) live on the device; the traversal is
 * enqueued on `stream` (0 = the graph's own stream) with no synchronisation.  One pass only: a query that
 * met two equal distances or a NaN on its way (or visited more nodes than its visited table holds: ~48 x ef)
 * reports count 0xFFFFFFFE and must be redone through qv_graph_search (which runs the exact-heap kernel for
 * those); everything else is final.  DEVICE-FORM traversals on one graph are ordered one after another whatever
 * their streams (they share the graph's own visited tables; host-pointer calls have a context each). */
int qv_graph_search_device(qv_graph* g, const float* d_queries, uint32_t nq, uint32_t k, uint32_t ef_search,
                           uint32_t* d_rows_out, float* d_dist_out, uint32_t* d_count_out, uint32_t* d_evals_out, void* stream);
void qv_graph_destroy(qv_graph* g);

/* ---- device-resident HNSW construction ----------------------------------------------
 * Replaces a loop of hnsw.HNSW.Insert (pkg/hnsw/hnsw.go:266-334: connectNode :337-468, selectNeighbors :583-599)
 * over rows that are already in `idx` (node index == row; the index must have been created with QV_FLAG_ROWMAJOR).
 * The reference connects concurrently (it releases its lock before connectNode, hnsw.go:313-315); the device build
 * inserts in BATCHES with the deterministic form of that: every node of a batch runs connectNode's searches
 * (greedy descent :367-380, then searchLayer(efConstruction) :385 on level min(level, CurrentLevel)) against the
 * graph as it was before the batch — one wavefront per node, the same traversal kernels as qv_graph_search — and
 * forward links, the self-links below the connected level (:463-467) and the back-links with their prune
 * (:413-460) are then applied as if node by node in index order.  A batch of ONE node is exactly Insert, so
 * batch_max = 1 reproduces the reference's sequential graph (the oracle's, tests/test_gpu_build.py).
 *   levels[i]   level of row first_row + i: the caller draws them in node order (randomLevel, hnsw.go:716-738),
 *               which keeps the RNG — seeded from the wall clock in the reference, hnsw.go:248 — on the host side
 *   m, max_m0, ef_construction   0 = the reference's defaults 16 / 2m / 200 (hnsw.go:223-231); <= 64 / 64 / 512
 *   batch_max   largest batch (0 = 16384, the maximum);  ramp_div: a batch never exceeds (nodes already linked) / ramp_div, so
 *               early nodes are inserted nearly one by one (0 = no ramp).  qv_graph_batch_size is the rule.
 * qv_graph_insert appends rows [first_row, first_row + n) (first_row must equal the graph's node count) and returns
 * when they are linked; the graph can be searched (qv_graph_search*) between and after calls. */
uint32_t qv_graph_batch_size(uint32_t nodes_linked, uint32_t batch_max, uint32_t ramp_div);
int qv_graph_create_empty(qv_graph** out, qv_index* idx, uint32_t capacity_nodes, uint32_t m, uint32_t max_m0, uint32_t ef_construction);
int qv_graph_insert(qv_graph* g, uint32_t first_row, uint32_t n, const int8_t* levels, uint32_t batch_max, uint32_t ramp_div);
/* hnsw.HNSW.Delete (hnsw.go:741-842) for the listed nodes, AS IF ONE BY ONE IN LIST ORDER, on the device, in place.  The graph
 * must be one that qv_graph_insert extends (qv_graph_create_empty / qv_graph_build / qv_graph_make_buildable); any other
 * answers QV_ERR_UNSUPPORTED like qv_graph_insert.
 *   lists      for every listed node d that is live at its turn, every level l <= level(d) and every x in conn_d[l] that is live
 *              at that moment (d itself included: a device-built node of level >= 1 links to itself below its connected level),
 *              every occurrence of d leaves conn_x[l]; the rest keeps its order, and the per-link distances the next prune ranks
 *              by move with the links.  A link to d from a node that d does not list STAYS (the reference leaves it; the
 *              traversals skip dead nodes).
 *   tombstone  level[d] = -1; the node's row in the index stays the caller's to remove (qv_index_remove)
 *   entry      changes only when the entry point is deleted (:796-827): the only node -> entry 0, level -1; else the first
 *              connection of d's highest non-empty level whose node is live, with that level (its lower levels next, while
 *              the first connection is dead); else the first live node other than d, with that node's level; else it stays.
 *              A replacement listed later is replaced again at its turn.  qv_graph_info reports the reference's EntryPoint /
 *              CurrentLevel; while that names a dead node the traversals and qv_graph_insert start from the first live node
 *              (:355-363, :621-629), and a graph without a live node answers every query with count 0.
 *   arguments  a node >= n_nodes: QV_ERR_OUT_OF_RANGE, nothing changed; a node already dead or listed twice: skipped; n == 0: QV_OK
 * Synchronous; needs the same external exclusion as qv_graph_insert.  Traversals of a graph with tombstones test node levels on
 * every hop (the level-0 fast paths are for graphs without). */
int qv_graph_remove(qv_graph* g, const uint32_t* nodes, uint32_t n);
/* The adjacency list of (nodes[i], levels[i]) for each i — one gather kernel, one download — so that a host mirror follows a
 * small edit without qv_graph_export's copy of the whole graph.  deg_out [n]; links_out [n][max(max_m0, max_m)], zero beyond
 * the degree.  A dead node, or a level the node does not have, answers degree 0; a node >= n_nodes QV_ERR_OUT_OF_RANGE. */
int qv_graph_export_lists(qv_graph* g, const uint32_t* nodes, const int* levels, uint32_t n, uint32_t* deg_out, uint32_t* links_out);
/* A graph uploaded with qv_graph_create (built on the host) carries no per-link distances, which the device-side
 * construction works on: this scores every existing link once (one wavefront per adjacency list, the traversal's
 * arithmetic: computeDistance(node.Vector, conn.Vector), hnsw.go:438), after which qv_graph_insert can extend the graph.
 * ef_construction as above.  No-op on a graph made by qv_graph_create_empty / qv_graph_build (apart from setting ef). */
int qv_graph_make_buildable(qv_graph* g, uint32_t ef_construction);
/* create_empty + insert of rows [0, n_nodes) */
int qv_graph_build(qv_graph** out, qv_index* idx, uint32_t n_nodes, const int8_t* levels, uint32_t m, uint32_t max_m0,
                   uint32_t ef_construction, uint32_t batch_max, uint32_t ramp_div);
/* Shape of a graph (any output may be null), and a copy of it in the flat form qv_graph_create takes:
 * levels [n_nodes], l0_deg [n_nodes], l0_links [n_nodes][max_m0], up_off [n_nodes], up_links [n_up_blocks][1 + max_m]
 * (any output may be null).  What HNSW.Nodes[i].Connections holds (hnsw.go:44-56), for the host side to keep. */
int qv_graph_info(const qv_graph* g, uint32_t* n_nodes, uint32_t* n_up_blocks, uint32_t* max_m0, uint32_t* max_m, uint32_t* entry, int* cur_level);
int qv_graph_export(qv_graph* g, int8_t* levels, uint32_t* l0_deg, uint32_t* l0_links, uint32_t* up_off, uint32_t* up_links);
/* Counters for reports: seconds spent in qv_graph_insert, batches, construction searches redone by the exact-heap
 * kernel (equal distances), qv_graph_search queries redone for the same reason. */
int qv_graph_stats(const qv_graph* g, double* build_seconds, uint64_t* build_batches, uint64_t* build_redo, uint64_t* search_redo);

/* ---- rejecting neighbours on the row-order bfloat16 copy (QV_FLAG_GRAPH_PLANE) ----
 * searchLayer drops a neighbour whose distance is not below the worst of a full result heap and never looks at that distance again
 * (hnsw.go:536-563).  On an index that keeps `rowmaj16`, a hop of the wave-per-query traversal that STARTS with a full list reads each
 * new neighbour's bfloat16 row (half the bytes), takes the bound scan's interval of its distance (qv_scan_bound_interval: the same
 * float32 chain, the same margin) and drops it when the lower end is not below the hop-start worst distance — exactly the rows the
 * reference drops at their turn, whatever is admitted before them.  The others ("survivors", and every row the bound says nothing
 * about) are evaluated from their float32 rows as before.  Rows, float32 bits, counts and evals_out are those of the unchanged
 * traversal.  A query whose norm the bound declines (zero, not a number, huge) walks as before.
 *   QV_GRAPH_REJECT_AUTO    the cells it was measured faster in (profiles/LAB_r17_graph_reject.md): QV_COSINE, dim == 768, a graph of 1 000 000 to
 *                           1 999 999 nodes, calls of 8192 queries or more, a list size max(ef_search, k) of 64 to 256.  There "always" ran
 *                           13 - 31 % ahead of "never" (1M x 768, MaxLevel 1, both corpora of the benchmark, list sizes 64 / 128 / 256, 8192 and
 *                           32 768 queries per call, every cell beyond both arms' spread).  Within those cells the rule interpolates
 *                           between the measured list sizes, takes calls larger than 32 768 and graphs up to twice the measured size, and
 *                           does not ask for the graph's MaxLevel (16 was not measured).  QV_DOT, every other dimension (128 among them),
 *                           10M nodes, smaller graphs and calls and other list sizes were NOT measured and launch the unchanged kernels
 *                           unless told "always".
 *   QV_GRAPH_REJECT_ALWAYS  wherever it applies (qv_graph_reject_applies)
 *   QV_GRAPH_REJECT_NEVER   the unchanged kernels
 * The environment variable QV_GRAPH_REJECT (1 always, 2 never; read once per process) sets the default of every graph.
 * qv_graph_set_reject_plane needs the same external exclusion against searches as qv_graph_insert.
 * Out of scope, all unchanged and none of them reads the copy: the latency form (calls of up to max(compute units, 768) queries, and
 * with it coalesced concurrent callers); the exact-heap kernel; construction searches; the upper levels; graphs with tombstones;
 * graphs with more than 32 level-0 links per node; QV_L2 and the float32-chain metrics; an 8-bit plane for the graph; dropping the
 * float32 row-major copy. */
#define QV_GRAPH_REJECT_AUTO   0
#define QV_GRAPH_REJECT_ALWAYS 1
#define QV_GRAPH_REJECT_NEVER  2
int qv_graph_set_reject_plane(qv_graph* g, int mode);
/* out[2] queries whose level-0 walk finished unflagged in the rejecting form (a query flagged for the exact-heap kernel — equal distances,
 * a NaN — or declined for its norm is not one), out[0] the evaluations those queries made in rejecting hops, out[1] the ones of them
 * rejected on the copy, out[3] 1 when the graph's index holds the copy.  Added once per query by the kernel; the call waits for the
 * device. */
int qv_graph_reject_stats(qv_graph* g, uint64_t* out);   /* out: 4 values */
/* The dispatch's own rule, on the host: 1 when a qv_graph_search* call of nq queries takes the rejecting form.  Any mode answers 0
 * without the copy, on a metric other than QV_COSINE / QV_DOT, for a graph with tombstones, for max_m0 > 32 and for a call the
 * latency form takes (nq <= max(cus, 768)); QV_GRAPH_REJECT_AUTO answers 1 only within the measured floors above.  ef_search: the
 * list size the call walks with, max(efSearch, k).
 * < 0: an argument error (unknown metric or mode, cus <= 0, dim == 0). */
int qv_graph_reject_applies(int metric, uint32_t dim, uint32_t n_nodes, uint32_t nq, uint32_t ef_search, int cus, int mode, int has_plane,
                            int has_tombstones, uint32_t max_m0);

/* ---- rejecting neighbours on the row-order 8-bit image (QV_FLAG_GRAPH_PLANE8) ----
 * On an index that keeps `rowmaj8`, a rejecting hop can read 128 elements of each new neighbour per 128-byte piece instead of 64: dim bytes and
 * one 16-byte record per evaluation, integer dot products against the query's two int8 terms (quantised once per query, resident in LDS beside
 * its float32 words), the certified interval of the 8-bit bound scan (qv_scan_bound_interval8), and survivors straight to their float32 rows.
 * Rows, float32 bits, counts and evals_out are those of the unchanged traversal.  qv_graph_set_reject_plane keeps deciding WHETHER a call
 * rejects; qv_graph_set_reject_image says which image such a call starts on:
 *   QV_GRAPH_IMAGE_AUTO  the 8-bit image only on indexes that hold it AND in the cells it was measured faster in than the bfloat16 copy and than
 *                        "never" (profiles/LAB_r23_graph_reject8.md): QV_COSINE, dim == 768, a graph of 1 000 000 to below 2 000 000 nodes, 8192
 *                        queries or more per call, list size max(ef_search, k) from 64 to 256 — all twelve measured cells: +7 ... +18 % over
 *                        bfloat16-first, +26 ... +53 % over "never".  In every other cell the bfloat16 copy, or the unchanged kernels where
 *                        no image is held.  Not measured and therefore not taken: other dimensions (128 among them), 10M nodes,
 *                        QV_DOT; MaxLevel 16 is not measured and not seen by the rule.  Widths at which the resident terms would cost a
 *                        traversal per CU (every width from 896 dimensions up) are declined
 *   QV_GRAPH_IMAGE_8BIT  the 8-bit image wherever it is held and the kernel's conditions hold, else the bfloat16 copy if held
 *   QV_GRAPH_IMAGE_BF16  never the 8-bit image
 * An index created without QV_FLAG_GRAPH_PLANE8 behaves exactly as before under every mode.  The environment variable QV_GRAPH_IMAGE
 * (1 the 8-bit image, 2 the bfloat16 copy; read once per process) sets the default of every graph.  Same exclusion as qv_graph_set_reject_plane.
 * Unchanged, as for the bfloat16 copy: the latency form (and with it coalesced concurrent callers), the exact-heap kernel, construction
 * searches, upper levels, graphs with tombstones, more than 32 level-0 links, QV_L2 and the float32-chain metrics; there is no 6-bit graph
 * image, the float32 row-major copy stays, and dimensions that are not whole 128-element slabs keep no image. */
#define QV_GRAPH_IMAGE_AUTO 0
#define QV_GRAPH_IMAGE_8BIT 1
#define QV_GRAPH_IMAGE_BF16 2
int qv_graph_set_reject_image(qv_graph* g, int mode);
/* out[0] = evaluations made in hops that rejected on the 8-bit image, out[1] = the ones of those that were rejected, out[2] = queries that
 * finished level 0 in that form, out[3] = 1 when the index holds the image.  qv_graph_reject_stats keeps counting bfloat16-copy hops only.
 * Waits for the device. */
int qv_graph_reject8_stats(qv_graph* g, uint64_t* out);  /* out: 4 values */
/* The dispatch's own rule: the arguments of qv_graph_reject_applies, then whether the index holds the 8-bit image and the image mode.
 * 0 = no rejecting form, 1 = the bfloat16 copy, 2 = the 8-bit image; < 0 = an argument error.  Never non-zero where qv_graph_reject_applies
 * answers 0 for an index holding that image. */
int qv_graph_reject_image_applies(int metric, uint32_t dim, uint32_t n_nodes, uint32_t nq, uint32_t ef_search, int cus, int mode, int has_plane,
                                  int has_tombstones, uint32_t max_m0, int has_image8, int image_mode);

/* ---- one corpus over the GPUs of a node --------------------------------
 * No reference counterpart (the reference is one process on CPU cores): this is what lets the Go host reach all the
 * GPUs of a node through ONE handle — what core.Index (pkg/core/collection.go:78-96) is for one GPU (qv_index),
 * qv_sharded is for n, with the same surface: add / remove / update / get / search with any k / filtered search /
 * search with a negative example / listed-row distances.  One host process; devices[g] holds shard g (an exact index
 * of its own) and runs its flat scan on a stream of its own; ONE RCCL all-gather per search carries every shard's
 * result list (nq*k*8 bytes per shard for a top-k, over xGMI between the GPUs of a node: a latency collective); the merge
 * on the first device orders by (distance, global row) like a single index.
 *   global row ids   shard g owns [g * span, (g+1) * span), span = qv_sharded_span(n): "global row = shard base +
 *                    local row" without knowing the corpus size up front; ids are stable as shards grow
 *   qv_sharded_add   cuts a batch into one contiguous piece per shard so that the shards' fill evens out
 *                    (qv_sharded_plan_add is the rule); global_rows_out[i] = id of rows[i] (the host maps string ids);
 *                    all-or-nothing like qv_index_add
 *   any k            k <= 64: per-shard fused top-k + one wavefront-list merge.  Up to 8192 every shard SELECTS its
 *                    min(k, rows) best (as qv_index_search_device does) and one radix selection on the first device takes
 *                    the k best of the gathered lists, the whole batch at once.  Beyond (a filtered Collection.Search asks
 *                    for k = Index.Size(), collection.go:679-682): every shard ranks its rows (radix sort), the sorted runs
 *                    are exchanged and one stable radix sort on the first device merges them
 *   flags            QV_FLAG_ROWMAJOR, QV_FLAG_BF16_ROWS, QV_FLAG_NO_SCAN_PLANE, QV_FLAG_L2_SCAN_PLANE, QV_FLAG_GRAPH_PLANE and QV_FLAG_GRAPH_PLANE8 pass through to the shards; QV_SHARDED_PEER_COPY replaces the collective with
 *                    point-to-point copies into the first device (and lets several shards share one device, which
 *                    RCCL does not allow: how the tests exercise 3 and 8 shards on a 1-GPU box)
 * Threading: as qv_index — searches, qv_sharded_distance_rows and qv_sharded_get_row(s) may run concurrently from many
 * threads (the reference searches under a read lock, collection.go:647): every call works in a context of its own
 * (streams, staging and exchange buffers from a pool); add / remove / update / reserve take the handle exclusively
 * (they wait for running searches); destroy needs external exclusion.
 * What has run on hardware (state of round 4; no box with more than one GPU was available to the authors): concurrent callers
 * with the point-to-point exchange (QV_SHARDED_PEER_COPY, shards co-located) and with RCCL at ONE rank.  With RCCL over several
 * devices every context enqueues its grouped all-gather on the shared per-device communicators under one lock, each on streams of
 * its own — within RCCL's rules, but first exercised by tests/test_gpu_sharded_abi.py::test_concurrent_callers_on_one_rccl_handle_*,
 * which needs two GPUs.  Until that has passed on the target node, callers that want no exposure serialise searches on an RCCL
 * handle or create it with QV_SHARDED_PEER_COPY. */
typedef struct qv_sharded qv_sharded;
#define QV_SHARDED_PEER_COPY (1ull << 32)
uint32_t qv_sharded_span(int n_shards);
int qv_sharded_plan_add(const uint64_t* rows_per_shard, int n_shards, uint64_t n, uint64_t* give_out);
int qv_sharded_create(qv_sharded** out, uint32_t dim, qv_metric metric, const int* devices, int n_devices, uint64_t flags);
void qv_sharded_destroy(qv_sharded* s);
int qv_sharded_shards(const qv_sharded* s);
uint64_t qv_sharded_size(const qv_sharded* s);                 /* live rows over all shards */
uint64_t qv_sharded_rows(const qv_sharded* s);                 /* rows ever added over all shards (tombstones included) */
uint32_t qv_sharded_dim(const qv_sharded* s);
int qv_sharded_shard_info(const qv_sharded* s, int shard, int* device, uint32_t* base_row, uint32_t* rows, uint32_t* live);
int qv_sharded_reserve(qv_sharded* s, uint64_t rows_total);
int qv_sharded_add(qv_sharded* s, const float* rows, uint32_t n, uint32_t* global_rows_out);
/* n synthetic rows (the generator of qv_index_add_synthetic), shard g taking the contiguous block [g*n/G, (g+1)*n/G) */
int qv_sharded_add_synthetic(qv_sharded* s, uint64_t seed, uint64_t gen_row0, uint64_t n);
int qv_sharded_remove(qv_sharded* s, const uint32_t* global_rows, uint32_t n);
/* qv_index_update / qv_index_get_row / qv_index_get_rows on the shard that owns the row (Collection.Update,
 * pkg/core/collection.go:417-465; hybrid_index.go:537 reads idx.vectors[id]) */
int qv_sharded_update(qv_sharded* s, uint32_t global_row, const float* vec);
/* qv_index_update_rows over global rows: what the loop of qv_sharded_update leaves (a repeated row ends with its last
 * vector).  EVERY global row is checked on every shard before anything is written (QV_ERR_OUT_OF_RANGE: nothing changed on
 * any shard); then each shard gets its rows, with their vectors gathered, in one qv_index_update_rows. */
int qv_sharded_update_rows(qv_sharded* s, const uint32_t* global_rows, uint32_t n, const float* vecs /* host [n][dim] */);
int qv_sharded_get_row(qv_sharded* s, uint32_t global_row, float* vec_out);
int qv_sharded_get_rows(qv_sharded* s, const uint32_t* global_rows, uint32_t n, float* out /* [n][dim] */);
/* Same contract as qv_index_search (check order, clamping, padding, ordering, any k); rows_out holds global row ids. */
int qv_sharded_search(qv_sharded* s, const float* queries, uint32_t nq, uint32_t k, uint32_t* rows_out, float* dist_out, uint32_t* count_out);
/* qv_index_search_masked over the shards.  The candidates are LISTED (n_selected global row ids, any order, duplicates
 * allowed) rather than given as a bitmap, because global row ids are sparse (one id range per shard); dead rows in the list
 * are ignored; an id outside every shard is QV_ERR_OUT_OF_RANGE.  count_out[q] = min(k, live selected rows). */
int qv_sharded_search_masked(qv_sharded* s, const float* queries, uint32_t nq, uint32_t k, const uint32_t* selected_global_rows, uint32_t n_selected,
                             uint32_t* rows_out, float* dist_out, uint32_t* count_out);
/* qv_index_search_negative over the shards (hybrid_index.go:517-570): every shard also evaluates distance(row, negative)
 * for its own k_fetch candidates before the exchange, so the merged list carries both distances after ONE exchange. */
int qv_sharded_search_negative(qv_sharded* s, const float* query, const float* negative, uint32_t k_fetch,
                               uint32_t* rows_out, float* dist_out, float* neg_dist_out, uint32_t* count_out);
/* qv_distance_rows with global row ids: every shard evaluates the rows it owns, all shards in flight together. */
int qv_sharded_distance_rows(qv_sharded* s, const float* query, const uint32_t* global_rows, uint32_t n, float* dist_out);
/* Queries and results resident on the FIRST device.  The work is enqueued on the handle's own streams and ordered after
 * what `stream` (a stream of the first device; null = the null stream, as in qv_index_search_device) held at the call and
 * before anything `stream` runs afterwards; there is no host synchronisation for any nq: queries the matrix-core filter
 * hands back (nq >= 9) are listed and redone by the exact scan on the device (k <= 64: round 5; 64 < k <= 4096: round 6, the
 * listed queries in groups of 64 through shared corpus passes + radix selection; until then their flags were read on the
 * host, one round trip per shard and batch; the first batch with k > 64 allocates that redo's keys per shard: 64 queries x
 * rows x 8 bytes, 1 GiB at most).  The one exception: a shard of more than ~67 M rows at k > 64, where a query's
 * keys leave room for one query at a time, still reads the flags on the host.  Any k. */
int qv_sharded_search_device(qv_sharded* s, const float* d_queries, uint32_t nq, uint32_t k, uint32_t* d_rows_out, float* d_dist_out, void* stream);
int qv_sharded_sync(qv_sharded* s);                            /* wait for every stream of the handle */
/* Measurement aid: with profiling on, every search is synchronous and its phases are timed with HIP events on the first
 * device's stream: its own scan, the exchange (incl. waiting for the slowest shard), merge + download; and every shard's
 * scan KERNEL is bracketed by events on its own stream (qv_index_profile): qv_sharded_profile_read_shard returns the summed
 * kernel time and launch count of one shard since the last read — the per-GPU roofline numerator. */
int qv_sharded_set_filter(qv_sharded* s, int filter);          /* qv_index_set_filter on every shard */
int qv_sharded_set_bound_scan(qv_sharded* s, int mode);       /* qv_index_set_bound_scan on every shard */
int qv_sharded_bound_scan_stats(qv_sharded* s, uint64_t out[4]);   /* qv_index_bound_scan_stats: [0] of the first shard, [1] [2] summed, [3] 1 when every shard holds the copy */
int qv_sharded_set_bound_plane(qv_sharded* s, int mode);      /* qv_index_set_bound_plane on every shard */
int qv_sharded_set_bound_plane_mq(qv_sharded* s, int mode);   /* qv_index_set_bound_plane_mq on every shard */
int qv_sharded_set_bound_plane6(qv_sharded* s, int mode);     /* qv_index_set_bound_plane6 on every shard */
int qv_sharded_bound_scan8_stats(qv_sharded* s, uint64_t out[4]);  /* qv_index_bound_scan8_stats, put together as qv_sharded_bound_scan_stats does */
int qv_sharded_profile(qv_sharded* s, int enable);
int qv_sharded_profile_read(qv_sharded* s, double* scan_ms_sum, double* exchange_ms_sum, double* merge_ms_sum, uint64_t* searches);
int qv_sharded_profile_read_shard(qv_sharded* s, int shard, double* scan_kernel_ms_sum, uint64_t* launches);

/* Copy row `row` back to the host (ExactIndex keeps vectors readable,
 * hybrid_index.go:537 reads idx.vectors[id] for the re-rank). */
int qv_index_get_row(qv_index* idx, uint32_t row, float* vec_out);
/* n rows in one device pass (ArrowHNSWIndex.Save writes every vector, index/arrow_hnsw.go:138-198): out = [n][dim] */
int qv_index_get_rows(qv_index* idx, const uint32_t* rows, uint32_t n, float* out);

/* ---- misc ----------------------------------------------------------------------- */
const char* qv_last_error(void);          /* thread-local */
int         qv_abi_version(void);
int         qv_device_count(void);
/* One line naming the HIP runtime and the RCCL this process bound (version + file): "hip_runtime=7.2.x lib=...; rccl=2.27.7
 * lib=...".  Both resolve by soname to whatever the process loaded first (PyTorch bundles its own pair); qv_sharded_create
 * refuses an RCCL exchange when the two come from different installations.  For reports of multi-GPU runs.  Also the process's
 * GPU_MAX_HW_QUEUES (hardware queues per device; the HIP runtime reads it at its first call and defaults to 4): a host that serves
 * concurrent callers sets it to 8 BEFORE its first HIP call — libqv never modifies the environment. */
int         qv_runtime_info(char* out, size_t cap);
/* Timing of the last qv_index_search_device-style launch is the caller's business
 * (HIP events on its stream); this returns static facts for reports. */
int         qv_device_info(int device, char* name_out, size_t name_cap, int* cu_count, uint64_t* hbm_bytes);

#ifdef __cplusplus
}
#endif
#endif /* QV_H */
