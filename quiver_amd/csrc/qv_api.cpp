// qv_api.cpp — the C ABI of include/qv.h over the gfx950 kernels (qv_*.hip).
//
// Host-side responsibilities only: argument checks in the reference's order and
// wording, device-memory ownership (tile storage sized for 288 GB HBM3E: one
// allocation per array, geometric growth, explicit reserve), a pool of per-call
// search contexts (stream + pinned staging + workspace) so concurrent searches do
// not serialise, and per-stream workspaces for the *_device entry points.
// There is NO CPU compute path here: every distance and every selection runs in
// a HIP kernel, and a missing/failed HIP runtime is a loud error, never a fallback.
#include "qv_api_internal.h"

#include <atomic>

namespace {
thread_local char g_err[512] = "";

// (GPU_MAX_HW_QUEUES — the HIP runtime's hardware queues per device, 4 by default — is the HOST's to set before its first HIP call:
// INTEGRATION.md "Environment"; qv_runtime_info reports what the process has.  The library does not touch the environment.)
}

int qv_fail(int code, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

namespace {

int acquire_ctx(qv_index* idx, SearchCtx** out) {
    {
        std::lock_guard<std::mutex> g(idx->ctx_mu);
        if (!idx->free_ctx.empty()) { *out = idx->free_ctx.back(); idx->free_ctx.pop_back(); return QV_OK; }
    }
    SearchCtx* c = new (std::nothrow) SearchCtx();
    if (!c) return fail(QV_ERR_OOM, "out of host memory");
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(QV_ERR_DEVICE, "hipStreamCreate failed: %s", hipGetErrorString(e)); }
    std::lock_guard<std::mutex> g(idx->ctx_mu);
    idx->all_ctx.push_back(c);
    *out = c;
    return QV_OK;
}
void release_ctx(qv_index* idx, SearchCtx* c) {
    std::lock_guard<std::mutex> g(idx->ctx_mu);
    idx->free_ctx.push_back(c);
}
struct CtxGuard {
    qv_index* idx; SearchCtx* c;
    ~CtxGuard() { if (c) release_ctx(idx, c); }
};

// The workspace of a caller stream.  Returns with `hold` locked on that workspace: the caller keeps it until its launches
// are enqueued, so that another thread using the same stream cannot grow (free) the buffer between "fetch the pointer" and
// "launch" — once enqueued, stream order protects the kernels (a grow drains the stream first).
int stream_workspace(qv_index* idx, hipStream_t s, size_t bytes, void** out, std::unique_lock<std::mutex>* hold, uint32_t** tickets_out = nullptr) {
    Workspace* w;
    {
        std::lock_guard<std::mutex> g(idx->ws_mu);
        Workspace*& slot = idx->stream_ws[s];
        if (!slot) slot = new (std::nothrow) Workspace();
        if (!slot) return fail(QV_ERR_OOM, "out of host memory");
        w = slot;
    }
    *hold = std::unique_lock<std::mutex>(w->mu);
    if (bytes > w->ws.cap) {
        // a larger workspace replaces one the stream may still be using: drain first
        HIPCHK(hipStreamSynchronize(s));
        int rc = w->ws.ensure(bytes + bytes / 2);
        if (rc != QV_OK) return rc;
    }
    *out = w->ws.p;
    if (tickets_out) {                                                 // the single-launch small scan's tickets: zeroed once, left zero by the kernel
        if (!w->tickets.p) {
            int rc = w->tickets.ensure(256);
            if (rc != QV_OK) return rc;
            // on the caller's stream, ahead of the kernel that reads them: hipMemset on device memory returns before the fill has run, and the
            // null stream it runs on is not ordered against a non-blocking stream — a first search on a fresh stream could start on
            // tickets that were not zero yet, or be zeroed under (test_concurrent_searches_on_one_handle failed about one run in four)
            HIPCHK(hipMemsetAsync(w->tickets.p, 0, 256, s));
        }
        *tickets_out = static_cast<uint32_t*>(w->tickets.p);
    }
    return QV_OK;
}

// grow device storage to hold `rows` rows (whole tiles), preserving contents
// one device array grown in place of the old one: the first keep_bytes are carried over, the rest is zero
template <typename T> hipError_t regrow(T** p, size_t keep_bytes, size_t new_bytes) {
    T* n = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&n), new_bytes);
    if (e != hipSuccess) return e;
    if (new_bytes > keep_bytes) e = hipMemset(reinterpret_cast<char*>(n) + keep_bytes, 0, new_bytes - keep_bytes);
    if (e == hipSuccess && keep_bytes) e = hipMemcpy(n, *p, keep_bytes, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);   // the fill and the copy may return early, and the index's streams are non-blocking: nothing of theirs may overtake these
    if (e != hipSuccess) { (void)hipFree(n); return e; }
    (void)hipFree(*p);
    *p = n;
    return hipSuccess;
}

// grow device storage to hold `rows` rows (whole tiles), preserving contents.  The arrays are grown ONE AT A TIME (old + new
// copy of one array live together, never of all four), and a failure half way leaves every array valid at its old or its
// new size with the capacity unchanged: nothing leaks, nothing dangles.
int ensure_rows(qv_index* idx, uint64_t rows, bool exact) {
    uint64_t need_tiles = (rows + 63) / 64;
    if (need_tiles <= idx->cap_tiles) return QV_OK;
    if (rows > 0xFFFFFFF0ull) return fail(QV_ERR_INVALID_ARG, "row count %llu exceeds the uint32 row space", (unsigned long long)rows);
    uint64_t new_tiles = exact ? need_tiles : std::max<uint64_t>(need_tiles, idx->cap_tiles + idx->cap_tiles / 2 + 16);
    const size_t tb = idx->tile_bytes();
    const uint64_t used_tiles = (idx->n_rows + 63) / 64;
    // pad rows must be finite and alive bits must start clear: the new part of every array is zero
    hipError_t e = regrow(&idx->d_tiles, used_tiles * tb, new_tiles * tb);
    if (e == hipSuccess) e = regrow(&idx->d_rnorm, used_tiles * 64 * sizeof(double), new_tiles * 64 * sizeof(double));
    if (e == hipSuccess) e = regrow(&idx->d_alive, used_tiles * sizeof(uint64_t), new_tiles * sizeof(uint64_t));
    if (e == hipSuccess) e = regrow(&idx->d_rres, used_tiles * 64 * sizeof(float), new_tiles * 64 * sizeof(float));
    if (e == hipSuccess && (idx->flags & QV_FLAG_ROWMAJOR))
        e = regrow(&idx->d_rowmaj, (size_t)idx->n_rows * idx->dim * sizeof(float), new_tiles * 64 * (size_t)idx->dim * sizeof(float));
    if (e == hipSuccess && idx->wants_rowmaj16()) {
        // the row-order bfloat16 copy (QV_FLAG_GRAPH_PLANE): an accelerator — when it does not fit, the index frees it and graph traversals walk as without
        // (QV_TEST_ROWMAJ16_OOM: the same for tests)
        hipError_t eg = getenv("QV_TEST_ROWMAJ16_OOM") ? hipErrorOutOfMemory
                                                       : regrow(&idx->d_rowmaj16, (size_t)idx->n_rows * idx->dim * sizeof(uint16_t), new_tiles * 64 * (size_t)idx->dim * sizeof(uint16_t));
        if (eg == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            (void)hipFree(idx->d_rowmaj16); idx->d_rowmaj16 = nullptr; idx->rowmaj16_lost = true;
        } else e = eg;
    }
    if (e == hipSuccess && idx->wants_rowmaj8()) {
        // the row-order 8-bit image and its records (QV_FLAG_GRAPH_PLANE8): the same — given up alone (QV_TEST_ROWMAJ8_OOM: the same for tests)
        hipError_t eg = getenv("QV_TEST_ROWMAJ8_OOM") ? hipErrorOutOfMemory
                                                      : regrow(&idx->d_rowmaj8, (size_t)idx->n_rows * idx->dim, new_tiles * 64 * (size_t)idx->dim);
        if (eg == hipSuccess) eg = regrow(&idx->d_rowmeta8, (size_t)idx->n_rows * sizeof(qv::RowMeta8), new_tiles * 64 * sizeof(qv::RowMeta8));
        if (eg == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            (void)hipFree(idx->d_rowmaj8); (void)hipFree(idx->d_rowmeta8); idx->d_rowmaj8 = nullptr; idx->d_rowmeta8 = nullptr; idx->rowmaj8_lost = true;
        } else e = eg;
    }
    if (e == hipSuccess && idx->wants_plane()) {
        // the bfloat16 copy: required under QV_FLAG_BF16_ROWS; otherwise (the default on cosine / dot indexes and on QV_FLAG_L2_SCAN_PLANE ones, for the single-query bound
        // scan) an accelerator — when it does not fit, the index frees it and carries on without: searches take the exact scan
        hipError_t eb = getenv("QV_TEST_PLANE_OOM") && !(idx->flags & QV_FLAG_BF16_ROWS) ? hipErrorOutOfMemory
                                                                                          : regrow(&idx->d_bf16, used_tiles * idx->bf16_tile_bytes(), new_tiles * idx->bf16_tile_bytes());
        if (eb == hipErrorOutOfMemory && !(idx->flags & QV_FLAG_BF16_ROWS)) {
            (void)hipGetLastError();
            (void)hipFree(idx->d_bf16); idx->d_bf16 = nullptr; idx->plane_lost = true;
        } else e = eb;
    }
    if (e == hipSuccess && idx->wants_plane8()) {
        // the 8-bit plane and its row state: an accelerator in front of that copy — when it does not fit, the index frees it and searches
        // start on the bfloat16 copy (QV_TEST_PLANE8_OOM: the same for tests)
        hipError_t e8 = getenv("QV_TEST_PLANE8_OOM") ? hipErrorOutOfMemory : regrow(&idx->d_plane8, used_tiles * idx->plane8_tile_bytes(), new_tiles * idx->plane8_tile_bytes());
        if (e8 == hipSuccess) e8 = regrow(&idx->d_rscale8, used_tiles * 64 * sizeof(float), new_tiles * 64 * sizeof(float));
        if (e8 == hipSuccess) e8 = regrow(&idx->d_rres8, used_tiles * 64 * sizeof(float), new_tiles * 64 * sizeof(float));
        if (e8 == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            (void)hipFree(idx->d_plane8); (void)hipFree(idx->d_rscale8); (void)hipFree(idx->d_rres8);
            idx->d_plane8 = nullptr; idx->d_rscale8 = nullptr; idx->d_rres8 = nullptr; idx->plane8_lost = true;
        } else e = e8;
    }
    if (idx->plane_lost && idx->d_plane8) {                            // (the 8-bit stage hands back to the bfloat16 stage: never one without the other)
        (void)hipFree(idx->d_plane8); (void)hipFree(idx->d_rscale8); (void)hipFree(idx->d_rres8);
        idx->d_plane8 = nullptr; idx->d_rscale8 = nullptr; idx->d_rres8 = nullptr; idx->plane8_lost = true;
    }
    if (e == hipSuccess && idx->wants_plane6()) {
        // the 6-bit plane and its residual: an accelerator in front of the 8-bit plane — when it does not fit, the index frees it and
        // searches start on the 8-bit plane (QV_TEST_PLANE6_OOM: the same for tests)
        hipError_t e6 = getenv("QV_TEST_PLANE6_OOM") ? hipErrorOutOfMemory : regrow(&idx->d_plane6, used_tiles * idx->plane6_tile_bytes(), new_tiles * idx->plane6_tile_bytes());
        if (e6 == hipSuccess) e6 = regrow(&idx->d_rres6, used_tiles * 64 * sizeof(float), new_tiles * 64 * sizeof(float));
        if (e6 == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            (void)hipFree(idx->d_plane6); (void)hipFree(idx->d_rres6);
            idx->d_plane6 = nullptr; idx->d_rres6 = nullptr; idx->plane6_lost = true;
        } else e = e6;
    }
    if (!idx->d_plane8 && idx->d_plane6) {                             // (the refine reads the 8-bit plane and its scale: never the 6-bit plane without it)
        (void)hipFree(idx->d_plane6); (void)hipFree(idx->d_rres6);
        idx->d_plane6 = nullptr; idx->d_rres6 = nullptr; idx->plane6_lost = true;
    }
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? QV_ERR_OOM : QV_ERR_DEVICE, "device allocation for %llu rows failed: %s", (unsigned long long)(new_tiles * 64), hipGetErrorString(e));
    idx->cap_tiles = new_tiles;
    return QV_OK;
}

void mark_alive_host(qv_index* idx, uint32_t row0, uint32_t n) {
    idx->alive_host.resize(((size_t)row0 + n + 63) / 64, 0);
    for (uint32_t r = row0; r < row0 + n; r++) idx->alive_host[r >> 6] |= 1ull << (r & 63);
}

// undo a partially applied add: counters back, alive words of every tile from the
// first touched one re-uploaded from the host mirror (the scan masks by alive bits only)
void rollback_rows(qv_index* idx, uint32_t base_rows, uint32_t base_live) {
    idx->n_rows = base_rows; idx->n_live = base_live;
    const size_t t0 = base_rows / 64;
    std::vector<uint64_t> words(idx->cap_tiles - t0, 0);
    if (t0 < idx->alive_host.size()) {
        idx->alive_host.resize((base_rows + 63) / 64);
        if (base_rows & 63) idx->alive_host[t0] &= (1ull << (base_rows & 63)) - 1;
        if (t0 < idx->alive_host.size()) words[0] = idx->alive_host[t0];
    }
    if (!words.empty()) (void)hipMemcpy(idx->d_alive + t0, words.data(), words.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
}

size_t lds_limit_dim() { return 16384; }   // f64 query staging: 16384 * 8 B = 128 KiB of the CU's 160 KiB

}  // namespace

extern "C" {

const char* qv_last_error(void) { return g_err; }
int qv_abi_version(void) { return QV_ABI_VERSION; }

int qv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int qv_device_info(int device, char* name_out, size_t name_cap, int* cu_count, uint64_t* hbm_bytes) {
    hipDeviceProp_t p;
    HIPCHK(hipGetDeviceProperties(&p, device));
    if (name_out && name_cap) { snprintf(name_out, name_cap, "%s (%s)", p.name, p.gcnArchName); }
    if (cu_count) *cu_count = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (uint64_t)p.totalGlobalMem;
    return QV_OK;
}

int qv_index_create(qv_index** out, uint32_t dim, qv_metric metric, int device, uint64_t flags) {
    if (!out) return fail(QV_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    if (dim == 0) return fail(QV_ERR_INVALID_ARG, "dimension must be positive");
    if (dim > lds_limit_dim()) return fail(QV_ERR_UNSUPPORTED, "dimension %u exceeds the supported maximum %zu", dim, lds_limit_dim());
    if ((int)metric < 0 || (int)metric >= QV_METRIC_COUNT) return fail(QV_ERR_INVALID_ARG, "unknown metric %d", (int)metric);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(QV_ERR_NO_DEVICE, "no HIP device available (%s); libqv has no CPU path", e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(QV_ERR_INVALID_ARG, "device %d out of range (have %d)", device, ndev);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t p;
    HIPCHK(hipGetDeviceProperties(&p, device));
    qv_index* idx = new (std::nothrow) qv_index();
    if (!idx) return fail(QV_ERR_OOM, "out of host memory");
    idx->device = device; idx->cus = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
    idx->dim = dim; idx->dim4 = (dim + 3) / 4; idx->metric = (int)metric; idx->flags = flags;
    if (hipMalloc(reinterpret_cast<void**>(&idx->d_bound_stats), 64) != hipSuccess || hipMemset(idx->d_bound_stats, 0, 64) != hipSuccess ||
        hipStreamSynchronize(nullptr) != hipSuccess) {
        (void)hipFree(idx->d_bound_stats); delete idx;
        return fail(QV_ERR_OOM, "device allocation of the index's counters failed");
    }
    *out = idx;
    return QV_OK;
}

void qv_index_destroy(qv_index* idx) {
    if (!idx) return;
    (void)hipSetDevice(idx->device);
    (void)hipDeviceSynchronize();
    for (SearchCtx* c : idx->all_ctx) { c->release(); delete c; }
    for (auto& kv : idx->stream_ws) { kv.second->ws.release(); kv.second->tickets.release(); delete kv.second; }
    (void)hipFree(idx->d_tiles); (void)hipFree(idx->d_rnorm); (void)hipFree(idx->d_alive); (void)hipFree(idx->d_rres); (void)hipFree(idx->d_rowmaj); (void)hipFree(idx->d_rowmaj16); (void)hipFree(idx->d_rowmaj8); (void)hipFree(idx->d_rowmeta8); (void)hipFree(idx->d_bf16); (void)hipFree(idx->d_bound_stats);
    (void)hipFree(idx->d_plane8); (void)hipFree(idx->d_rscale8); (void)hipFree(idx->d_rres8);
    (void)hipFree(idx->d_plane6); (void)hipFree(idx->d_rres6);
    idx->mut_stage.release();
    delete idx;
}

int qv_index_reserve(qv_index* idx, uint64_t rows) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    HIPCHK(hipSetDevice(idx->device));
    return ensure_rows(idx, rows, true);
}

uint32_t qv_index_rows(const qv_index* idx) { return idx ? idx->n_rows : 0; }
uint32_t qv_index_size(const qv_index* idx) { return idx ? idx->n_live : 0; }
uint32_t qv_index_dim(const qv_index* idx) { return idx ? idx->dim : 0; }
int qv_index_metric(const qv_index* idx) { return idx ? idx->metric : -1; }

int qv_index_add_device(qv_index* idx, const float* d_rows, uint32_t n, uint32_t* first_row_out, void* stream) {
    if (idx) idx->row_writes++;
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (first_row_out) *first_row_out = idx->n_rows;
    if (n == 0) return QV_OK;
    if (!d_rows) return fail(QV_ERR_INVALID_ARG, "rows is null");
    HIPCHK(hipSetDevice(idx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = ensure_rows(idx, (uint64_t)idx->n_rows + n, false);
    if (rc != QV_OK) return rc;
    const uint32_t row0 = idx->n_rows;
    idx->n_rows += n;                                   // view() must cover the new rows
    hipError_t e = qv::launch_ingest(idx->view(), d_rows, row0, n, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { idx->n_rows = row0; return fail(QV_ERR_DEVICE, "ingest failed: %s", hipGetErrorString(e)); }
    idx->n_live += n;
    mark_alive_host(idx, row0, n);
    return QV_OK;
}

int qv_index_add(qv_index* idx, const float* rows, uint32_t n, uint32_t* first_row_out) {
    if (idx) idx->row_writes++;
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (first_row_out) *first_row_out = idx->n_rows;
    if (n == 0) return QV_OK;
    if (!rows) return fail(QV_ERR_INVALID_ARG, "rows is null");
    HIPCHK(hipSetDevice(idx->device));
    int rc = ensure_rows(idx, (uint64_t)idx->n_rows + n, false);
    if (rc != QV_OK) return rc;
    // stage in chunks of <= 256 MiB so a 30 GB corpus never needs a second full-size buffer
    const size_t row_bytes = (size_t)idx->dim * sizeof(float);
    const uint32_t chunk_rows = (uint32_t)std::max<size_t>(1, std::min<size_t>(n, ((size_t)256 << 20) / row_bytes));
    if ((rc = idx->mut_stage.ensure((size_t)chunk_rows * row_bytes))) return rc;
    float* d_stage = static_cast<float*>(idx->mut_stage.p);
    uint32_t done = 0;
    const uint32_t base_rows = idx->n_rows, base_live = idx->n_live;
    while (done < n) {
        uint32_t m = std::min(chunk_rows, n - done);
        hipError_t e = hipMemcpy(d_stage, rows + (size_t)done * idx->dim, (size_t)m * row_bytes, hipMemcpyHostToDevice);
        rc = e == hipSuccess ? QV_OK : fail(QV_ERR_DEVICE, "hipMemcpy H2D failed: %s", hipGetErrorString(e));
        uint32_t fr = 0;
        if (rc == QV_OK) rc = qv_index_add_device(idx, d_stage, m, &fr, nullptr);
        if (rc != QV_OK) {                      // all-or-nothing (InsertBatch rolls back, hybrid_index.go:175-216)
            rollback_rows(idx, base_rows, base_live);
            return rc;
        }
        done += m;
    }
    if (idx->mut_stage.cap > ((size_t)64 << 20)) idx->mut_stage.release();     // do not keep a bulk-load buffer around
    if (first_row_out) *first_row_out = base_rows;
    return QV_OK;
}

int qv_index_add_synthetic(qv_index* idx, uint64_t seed, uint64_t gen_row0, uint32_t n, uint32_t* first_row_out) {
    if (idx) idx->row_writes++;
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (first_row_out) *first_row_out = idx->n_rows;
    if (n == 0) return QV_OK;
    HIPCHK(hipSetDevice(idx->device));
    int rc = ensure_rows(idx, (uint64_t)idx->n_rows + n, false);
    if (rc != QV_OK) return rc;
    const uint32_t row0 = idx->n_rows;
    idx->n_rows += n;
    hipError_t e = qv::launch_generate(idx->view(), seed, gen_row0, row0, n, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { idx->n_rows = row0; return fail(QV_ERR_DEVICE, "generate failed: %s", hipGetErrorString(e)); }
    idx->n_live += n;
    mark_alive_host(idx, row0, n);
    return QV_OK;
}

int qv_index_remove(qv_index* idx, const uint32_t* rows, uint32_t n) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (n == 0) return QV_OK;
    if (!rows) return fail(QV_ERR_INVALID_ARG, "rows is null");
    for (uint32_t i = 0; i < n; i++)
        if (rows[i] >= idx->n_rows) return fail(QV_ERR_OUT_OF_RANGE, "row %u out of range (rows: %u)", rows[i], idx->n_rows);
    HIPCHK(hipSetDevice(idx->device));
    { const int rc0 = idx->mut_stage.ensure((size_t)n * sizeof(uint32_t)); if (rc0 != QV_OK) return rc0; }
    uint32_t* d = static_cast<uint32_t*>(idx->mut_stage.p);
    hipError_t e = hipMemcpy(d, rows, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = qv::launch_set_alive(idx->view(), d, n, 0, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return fail(QV_ERR_DEVICE, "remove failed: %s", hipGetErrorString(e));
    for (uint32_t i = 0; i < n; i++) {
        uint64_t bit = 1ull << (rows[i] & 63);
        if (idx->alive_host[rows[i] >> 6] & bit) { idx->alive_host[rows[i] >> 6] &= ~bit; idx->n_live--; }
    }
    return QV_OK;
}

int qv_index_update(qv_index* idx, uint32_t row, const float* vec) {
    if (idx) idx->row_writes++;
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (!vec) return fail(QV_ERR_INVALID_ARG, "vector is null");
    if (row >= idx->n_rows) return fail(QV_ERR_OUT_OF_RANGE, "row %u out of range (rows: %u)", row, idx->n_rows);
    HIPCHK(hipSetDevice(idx->device));
    { const int rc0 = idx->mut_stage.ensure((size_t)idx->dim * sizeof(float)); if (rc0 != QV_OK) return rc0; }
    float* d = static_cast<float*>(idx->mut_stage.p);
    hipError_t e = hipMemcpy(d, vec, (size_t)idx->dim * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = qv::launch_ingest(idx->view(), d, row, 1, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return fail(QV_ERR_DEVICE, "update failed: %s", hipGetErrorString(e));
    uint64_t bit = 1ull << (row & 63);
    if (!(idx->alive_host[row >> 6] & bit)) { idx->alive_host[row >> 6] |= bit; idx->n_live++; }
    return QV_OK;
}

}  // extern "C"

// ---- qv_index_update_rows: the host side of the scattered ingest --------------------------------------------------------------
namespace {

// keep[i] = 1 unless rows[i] occurs again later in the list (a row listed more than once ends with its LAST vector)
std::vector<uint8_t> update_rows_keep(const uint32_t* rows, uint32_t n) {
    std::vector<uint8_t> keep(n, 1);
    std::vector<uint64_t> key(n);
    for (uint32_t i = 0; i < n; i++) key[i] = (uint64_t)rows[i] << 32 | i;
    std::sort(key.begin(), key.end());
    for (uint32_t i = 0; i + 1 < n; i++) if ((key[i] >> 32) == (key[i + 1] >> 32)) keep[(uint32_t)key[i]] = 0;
    return keep;
}

// The kept entries of rows[a, b), sorted by row, and the tiles they touch.  One array, in the order the device reads it:
// rows_sorted[m] | src[m] (position in the list, counted from a) | tile_first[T + 1] | tiles[T].
struct UpdatePlan { std::vector<uint32_t> words; uint32_t m = 0, T = 0; };
UpdatePlan update_rows_plan(const uint32_t* rows, const uint8_t* keep, uint32_t a, uint32_t b) {
    std::vector<uint64_t> key;
    key.reserve(b - a);
    for (uint32_t i = a; i < b; i++) if (keep[i]) key.push_back((uint64_t)rows[i] << 32 | (i - a));
    std::sort(key.begin(), key.end());
    UpdatePlan p;
    p.m = (uint32_t)key.size();
    for (uint32_t i = 0; i < p.m; i++) if (i == 0 || (key[i] >> 38) != (key[i - 1] >> 38)) p.T++;
    p.words.resize(2 * (size_t)p.m + 2 * (size_t)p.T + 1);
    uint32_t* rs = p.words.data(), * src = rs + p.m, * first = src + p.m, * tiles = first + p.T + 1;
    uint32_t t = 0;
    for (uint32_t i = 0; i < p.m; i++) {
        rs[i] = (uint32_t)(key[i] >> 32); src[i] = (uint32_t)key[i];
        if (i == 0 || (key[i] >> 38) != (key[i - 1] >> 38)) { first[t] = i; tiles[t] = rs[i] >> 6; t++; }
    }
    first[p.T] = p.m;
    return p;
}
size_t update_plan_cap_bytes(uint32_t n) { return (4 * (size_t)n + 1) * sizeof(uint32_t); }    // (m <= n entries, T <= m tiles)

// vectors per staged chunk of the host form: 256 MiB of them (QV_UPDATE_ROWS_CHUNK_BYTES, read once: for tests of the chunk seam)
uint32_t update_rows_chunk(size_t row_bytes) {
    static const size_t bytes = [] {
        const char* e = getenv("QV_UPDATE_ROWS_CHUNK_BYTES");
        const unsigned long long v = e ? strtoull(e, nullptr, 10) : 0;
        return v ? (size_t)std::min<unsigned long long>(v, 256ull << 20) : (size_t)256 << 20;
    }();
    return (uint32_t)std::max<size_t>(1, bytes / row_bytes);
}

// rows[a, b) of a checked list -> the device, from d_vecs (the vector of rows[i] at d_vecs + (i - a) * dim); d_plan: device room for
// update_plan_cap_bytes(b - a).  Returns when the stream has finished; the host mirror is the caller's to update.
int update_rows_apply(qv_index* idx, const uint32_t* rows, const uint8_t* keep, uint32_t a, uint32_t b, const float* d_vecs, uint32_t* d_plan, hipStream_t s) {
    const UpdatePlan p = update_rows_plan(rows, keep, a, b);
    if (p.m == 0) return QV_OK;
    hipError_t e = hipMemcpyAsync(d_plan, p.words.data(), p.words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s);
    const uint32_t* d_rs = d_plan, * d_src = d_rs + p.m, * d_first = d_src + p.m, * d_tiles = d_first + p.T + 1;
    if (e == hipSuccess) e = qv::launch_update_rows(idx->view(), d_vecs, d_rs, d_src, d_first, d_tiles, p.m, p.T, s);
    const hipError_t e2 = hipStreamSynchronize(s);                     // (always: p.words is read by the copy until the stream has passed it)
    if (e == hipSuccess) e = e2;
    return e == hipSuccess ? QV_OK : fail(QV_ERR_DEVICE, "update_rows failed: %s", hipGetErrorString(e));
}

int update_rows_check(qv_index* idx, const uint32_t* rows, uint32_t n, const void* vecs) {
    if (!rows) return fail(QV_ERR_INVALID_ARG, "rows is null");
    if (!vecs) return fail(QV_ERR_INVALID_ARG, "vectors is null");
    for (uint32_t i = 0; i < n; i++)
        if (rows[i] >= idx->n_rows) return fail(QV_ERR_OUT_OF_RANGE, "row %u out of range (rows: %u)", rows[i], idx->n_rows);
    return QV_OK;
}

void update_rows_mark(qv_index* idx, const uint32_t* rows, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t bit = 1ull << (rows[i] & 63);
        if (!(idx->alive_host[rows[i] >> 6] & bit)) { idx->alive_host[rows[i] >> 6] |= bit; idx->n_live++; }
    }
}

}  // namespace

extern "C" {

int qv_index_update_rows_device(qv_index* idx, const uint32_t* rows, uint32_t n, const float* d_vecs, void* stream) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (n == 0) return QV_OK;
    int rc = update_rows_check(idx, rows, n, d_vecs);
    if (rc != QV_OK) return rc;
    idx->row_writes++;
    HIPCHK(hipSetDevice(idx->device));
    if ((rc = idx->mut_stage.ensure(update_plan_cap_bytes(n)))) return rc;
    const std::vector<uint8_t> keep = update_rows_keep(rows, n);
    rc = update_rows_apply(idx, rows, keep.data(), 0, n, d_vecs, static_cast<uint32_t*>(idx->mut_stage.p), static_cast<hipStream_t>(stream));
    if (rc != QV_OK) return rc;
    update_rows_mark(idx, rows, n);
    return QV_OK;
}

int qv_index_update_rows(qv_index* idx, const uint32_t* rows, uint32_t n, const float* vecs) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (n == 0) return QV_OK;
    int rc = update_rows_check(idx, rows, n, vecs);
    if (rc != QV_OK) return rc;
    idx->row_writes++;
    HIPCHK(hipSetDevice(idx->device));
    // duplicates are settled over the WHOLE list first: an entry whose row comes again later is never written, so every chunk is a
    // scatter of distinct rows and no chunk writes a row another chunk writes
    const std::vector<uint8_t> keep = update_rows_keep(rows, n);
    const size_t row_bytes = (size_t)idx->dim * sizeof(float);
    const uint32_t chunk_rows = std::min(n, update_rows_chunk(row_bytes));
    const size_t vec_bytes = ((size_t)chunk_rows * row_bytes + 255) & ~(size_t)255;
    if ((rc = idx->mut_stage.ensure(vec_bytes + update_plan_cap_bytes(chunk_rows)))) return rc;
    float* d_stage = static_cast<float*>(idx->mut_stage.p);
    uint32_t* d_plan = reinterpret_cast<uint32_t*>(static_cast<char*>(idx->mut_stage.p) + vec_bytes);
    for (uint32_t done = 0; done < n; done += chunk_rows) {
        const uint32_t m = std::min(chunk_rows, n - done);
        const hipError_t e = hipMemcpy(d_stage, vecs + (size_t)done * idx->dim, (size_t)m * row_bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(QV_ERR_DEVICE, "hipMemcpy H2D failed: %s", hipGetErrorString(e));
        if ((rc = update_rows_apply(idx, rows, keep.data(), done, done + m, d_stage, d_plan, nullptr)) != QV_OK) return rc;
    }
    if (idx->mut_stage.cap > ((size_t)64 << 20)) idx->mut_stage.release();     // do not keep a bulk buffer around
    update_rows_mark(idx, rows, n);
    return QV_OK;
}

int qv_update_rows_plan(const uint32_t* rows, uint32_t n, uint32_t* rows_out, uint32_t* src_out, uint32_t* tile_first_out, uint32_t* tiles_out,
                        uint32_t* n_unique, uint32_t* n_tiles) {
    if (!rows_out || !src_out || !tile_first_out || !tiles_out || !n_unique || !n_tiles || (n && !rows)) return fail(QV_ERR_INVALID_ARG, "a pointer is null");
    const std::vector<uint8_t> keep = update_rows_keep(rows, n);
    const UpdatePlan p = update_rows_plan(rows, keep.data(), 0, n);
    const uint32_t* w = p.words.data();
    memcpy(rows_out, w, p.m * sizeof(uint32_t)); memcpy(src_out, w + p.m, p.m * sizeof(uint32_t));
    memcpy(tile_first_out, w + 2 * (size_t)p.m, (p.T + 1) * sizeof(uint32_t)); memcpy(tiles_out, w + 2 * (size_t)p.m + p.T + 1, p.T * sizeof(uint32_t));
    *n_unique = p.m; *n_tiles = p.T;
    return QV_OK;
}

int qv_index_get_row(qv_index* idx, uint32_t row, float* vec_out) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (!vec_out) return fail(QV_ERR_INVALID_ARG, "vec_out is null");
    if (row >= idx->n_rows) return fail(QV_ERR_OUT_OF_RANGE, "row %u out of range (rows: %u)", row, idx->n_rows);
    HIPCHK(hipSetDevice(idx->device));
    SearchCtx* c = nullptr;                                            // a pooled context: its stream and staging buffers, no allocation per call
    int rc = acquire_ctx(idx, &c);
    if (rc != QV_OK) return rc;
    CtxGuard guard{idx, c};
    const size_t bytes = (size_t)idx->dim * sizeof(float);
    if ((rc = c->d_q.ensure(bytes)) || (rc = c->h_q.ensure(bytes))) return rc;
    hipError_t e = qv::launch_fetch_row(idx->view(), row, static_cast<float*>(c->d_q.p), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->h_q.p, c->d_q.p, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(QV_ERR_DEVICE, "get_row failed: %s", hipGetErrorString(e));
    memcpy(vec_out, c->h_q.p, bytes);
    return QV_OK;
}

int qv_index_get_rows(qv_index* idx, const uint32_t* rows, uint32_t n, float* out) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (n == 0) return QV_OK;
    if (!rows || !out) return fail(QV_ERR_INVALID_ARG, "rows/out is null");
    for (uint32_t i = 0; i < n; i++)
        if (rows[i] >= idx->n_rows) return fail(QV_ERR_OUT_OF_RANGE, "row %u out of range (rows: %u)", rows[i], idx->n_rows);
    HIPCHK(hipSetDevice(idx->device));
    SearchCtx* c = nullptr;
    int rc = acquire_ctx(idx, &c);
    if (rc != QV_OK) return rc;
    CtxGuard guard{idx, c};
    const size_t row_bytes = (size_t)idx->dim * sizeof(float);
    const uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(n, ((size_t)64 << 20) / row_bytes));   // <= 64 MiB per pass
    if ((rc = c->d_ids.ensure((size_t)chunk * 4)) || (rc = c->h_ids.ensure((size_t)chunk * 4)) || (rc = c->d_q.ensure((size_t)chunk * row_bytes))) return rc;
    for (uint32_t done = 0; done < n; done += chunk) {
        const uint32_t m = std::min(chunk, n - done);
        memcpy(c->h_ids.p, rows + done, (size_t)m * 4);
        HIPCHK(hipMemcpyAsync(c->d_ids.p, c->h_ids.p, (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
        hipError_t e = qv::launch_fetch_rows(idx->view(), static_cast<const uint32_t*>(c->d_ids.p), m, static_cast<float*>(c->d_q.p), c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(out + (size_t)done * idx->dim, c->d_q.p, (size_t)m * row_bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(QV_ERR_DEVICE, "get_rows failed: %s", hipGetErrorString(e));
    }
    return QV_OK;
}

// The route of a fused flat search (kk <= kMaxFusedK, kk == k_stride), for the launch (enqueue_search) and for the workspace
// (search_ws_bytes): the same question with the same inputs, so what is launched is what was sized.  tickets: the call carries the
// stream's ticket words (and with them the index's bound-scan counters); cand_tiles: kBoundNoFilter, or a filtered call's candidate tiles.
static qv::FlatPlan flat_plan(const qv_index* idx, uint32_t nq, uint32_t kk, bool tickets, uint32_t cand_tiles) {
    const qv::IndexView v = idx->view();
    return qv::plan_flat(v, qv::plan_scan(v.n_tiles, idx->cus), nq, kk, tickets, tickets, cand_tiles);
}

// qv_index_profile: an event pair around one launch — both events or neither (none while profiling is off, or when an event cannot be
// made).  A launcher that takes (ev0, ev1) records them around its scan kernel itself; around one that takes none the pair is recorded
// here, on `s` (record).  The pair joins the index's list only behind a launch that succeeded, both events recorded, and is destroyed otherwise.
struct ProfilePair { hipEvent_t ev0 = nullptr, ev1 = nullptr; };
static ProfilePair profile_begin(const qv_index* idx, bool record = false, hipStream_t s = nullptr) {
    ProfilePair p;
    if (!idx->profiling || hipEventCreate(&p.ev0) != hipSuccess) return ProfilePair{};
    if (hipEventCreate(&p.ev1) != hipSuccess) { (void)hipEventDestroy(p.ev0); return ProfilePair{}; }
    if (record && hipEventRecord(p.ev0, s) != hipSuccess) { (void)hipEventDestroy(p.ev0); (void)hipEventDestroy(p.ev1); return ProfilePair{}; }
    return p;
}
static void profile_end(qv_index* idx, const ProfilePair& p, bool launched, bool record = false, hipStream_t s = nullptr) {
    if (!p.ev0) return;
    if (launched && (!record || hipEventRecord(p.ev1, s) == hipSuccess)) {
        std::lock_guard<std::mutex> g(idx->prof_mu);
        idx->prof_events.emplace_back(p.ev0, p.ev1);
        return;
    }
    (void)hipEventDestroy(p.ev0); (void)hipEventDestroy(p.ev1);
}

// Whether a search of list length kk takes the bound scan's wide form (65 <= kk <= 1024), for the launch (enqueue_search) and for the
// workspace (search_ws_bytes): 0 no, 1 the bfloat16 copy first, 2 the 8-bit plane first.  One query whose call carries the stream's ticket
// words, kk == k_stride.  Unfiltered (cand_tiles == kBoundNoFilter): fewer results than live rows (a k above the live rows keeps its path);
// the rest is qv::bound_wide_route's answer under the index's two knobs.  Filtered: cand_tiles and candidates are the call's candidate tiles
// and its live candidates as the host counts them, and the answer is qv::bound_wide_route_filtered's under the filtered form's own knob and
// the single-query filtered plane knob — fewer results than candidates is that rule's own condition.
static int wide_route(const qv_index* idx, uint32_t nq, uint32_t kk, uint32_t k_stride, bool tickets, uint32_t cand_tiles, uint64_t candidates) {
    if (nq != 1 || kk != k_stride || !tickets) return 0;
    const int metric = idx->l2_planes() ? QV_RULE_L2_PLANES : idx->metric;
    if (cand_tiles != qv::kBoundNoFilter)
        return qv::bound_wide_route_filtered(metric, idx->dim, idx->n_rows, nq, kk, idx->bound_wide_filtered, idx->bound.plane[qv::bound_one_filtered], idx->d_bf16 != nullptr,
                                             idx->d_plane8 != nullptr, cand_tiles, candidates);
    if (kk >= idx->n_live) return 0;
    return qv::bound_wide_route(metric, idx->dim, idx->n_rows, nq, kk, idx->bound_wide, idx->bound.plane[qv::bound_one], idx->d_bf16 != nullptr, idx->d_plane8 != nullptr);
}

// The same question for the wide form of the SHARED pass: an unfiltered call of 2 - 8 queries at 65 <= kk <= 1024 whose call carries the stream's
// ticket words, kk == k_stride, fewer results than live rows; the rest is qv::bound_wide_route_mq's answer under the form's own knob and the
// shared pass's plane knob.  0 no, 1 the bfloat16 copy first, 2 the 8-bit plane first.
static int wide_route_mq(const qv_index* idx, uint32_t nq, uint32_t kk, uint32_t k_stride, bool tickets, bool filtered) {
    if (nq < 2 || kk != k_stride || !tickets || filtered || kk >= idx->n_live) return 0;
    // H_j is the kk-th of the grid x 256 keys a query's waves publish: a grid too small for that (one or two compute units at a large kk)
    // keeps its path.  The rule cannot see the grid; the launcher checks the same.
    if ((uint64_t)qv::plan_scan((idx->n_rows + 63) / 64, idx->cus).grid * 256 <= kk) return 0;
    const int metric = idx->l2_planes() ? QV_RULE_L2_PLANES : idx->metric;
    return qv::bound_wide_route_mq(metric, idx->dim, idx->n_rows, nq, kk, idx->bound_wide_mq, idx->bound.plane[qv::bound_mq], idx->d_bf16 != nullptr, idx->d_plane8 != nullptr);
}

// what a call may hand enqueue_search beside its queries and outputs
struct SearchExtras {
    const uint64_t* d_candidates = nullptr;   // row bitmap replacing the tombstone bitmap (filtered search)
    uint32_t candidate_tiles = 0;             // with d_candidates: the tiles that hold a candidate (an upper bound known on the host)
    uint64_t candidates = 0;                  // with d_candidates: the live rows it selects, where the host counted them (the filtered wide form's rule; 0: not counted)
    uint32_t* d_tickets = nullptr;            // the stream's tickets: allows the single-launch small scan
    uint32_t* done_flag = nullptr;            // one query: the word the last kernel writes done_seq into behind its results; *flag_used: it will
    uint32_t done_seq = 0;
    bool* flag_used = nullptr;
};

// shared by the host and device entry points: enqueue nq searches of list length kk
// (kk = min(k, live)), results written with row stride k_stride
static int enqueue_search(qv_index* idx, const float* d_queries, uint32_t nq, uint32_t kk, uint32_t k_stride,
                          void* ws, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s, const SearchExtras& x = SearchExtras()) {
    qv::IndexView v = idx->view();
    if (x.d_candidates) v.alive = const_cast<uint64_t*>(x.d_candidates);   // read-only in every scan kernel
    const qv::ScanPlan plan = qv::plan_scan(v.n_tiles, idx->cus);
    if (kk <= (uint32_t)qv::kMaxFusedK && kk == k_stride) {
        const ProfilePair pp = profile_begin(idx);
        // (a masked search: the bound scan's forms that skip tiles without a candidate, under the filtered rule — given tickets)
        const uint32_t cand_tiles = x.d_candidates ? x.candidate_tiles : qv::kBoundNoFilter;
        const qv::FlatPlan fp = flat_plan(idx, nq, kk, x.d_tickets != nullptr, cand_tiles);
        hipError_t e = qv::launch_flat_topk(v, plan, fp, d_queries, nq, kk, ws, d_rows_out, d_dist_out, s, pp.ev0, pp.ev1, x.d_tickets, nq == 1 ? x.done_flag : nullptr, x.done_seq,
                                            x.flag_used, fp.bound() ? idx->d_bound_stats : nullptr, cand_tiles);
        profile_end(idx, pp, e == hipSuccess);
        if (e != hipSuccess) return fail(QV_ERR_DEVICE, "%s scan launch failed: %s", fp.route == qv::FlatRoute::small ? "small" : "flat", hipGetErrorString(e));
        return QV_OK;
    }
    // 65 <= k <= 1024, one query, unfiltered or over its candidate bitmap, where the wide form's rule takes it: the bound scan on the reduced
    // copies, its re-score and selection, and the gated key-per-row redo behind them — all enqueued by the one launcher
    if (const int wide = wide_route(idx, nq, kk, k_stride, x.d_tickets != nullptr, x.d_candidates ? x.candidate_tiles : qv::kBoundNoFilter, x.candidates)) {
        const ProfilePair pp = profile_begin(idx, true, s);
        hipError_t e = qv::launch_bound_scan_wide(v, plan, d_queries, kk, ws, x.d_tickets + qv::kBoundCtrlWord, idx->d_bound_stats, d_rows_out, d_dist_out, s, wide == 2, x.d_candidates != nullptr);
        profile_end(idx, pp, e == hipSuccess, true, s);
        if (e != hipSuccess) return fail(QV_ERR_DEVICE, "wide bound scan launch failed: %s", hipGetErrorString(e));
        return QV_OK;
    }
    // ... and 2 - 8 unfiltered queries of that length where the wide shared pass's rule takes them: the reduced copy read once for the pass
    if (const int wide = wide_route_mq(idx, nq, kk, k_stride, x.d_tickets != nullptr, x.d_candidates != nullptr)) {
        const ProfilePair pp = profile_begin(idx, true, s);
        hipError_t e = qv::launch_bound_scan_wide_mq(v, plan, d_queries, nq, kk, ws, x.d_tickets + qv::kBoundCtrlWord, idx->d_bound_stats, d_rows_out, d_dist_out, s, wide == 2);
        profile_end(idx, pp, e == hipSuccess, true, s);
        if (e != hipSuccess) return fail(QV_ERR_DEVICE, "wide shared bound pass launch failed: %s", hipGetErrorString(e));
        return QV_OK;
    }
    // 64 < k <= 8192 (the negative-example branches fetch max(2k, 30), hybrid_index.go:516-522; BatchSearch takes any k,
    // :677-811), and any shorter list whose output stride differs from its length: one key per row, then a radix SELECT
    if (kk > (uint32_t)qv::kMaxFusedK && kk <= (uint32_t)qv::kMaxWideK && nq == 1) {   // (several queries: shared corpus passes through the key-per-row path below)
        // up to 128: the scan's own stream with 2 keys per lane in the wave's list, then a selection over the waves' lists
        const ProfilePair pp = profile_begin(idx);
        hipError_t e = qv::launch_flat_wide(v, plan, d_queries, nq, kk, k_stride, ws, d_rows_out, d_dist_out, s, pp.ev0, pp.ev1);
        profile_end(idx, pp, e == hipSuccess);
        if (e != hipSuccess) return fail(QV_ERR_DEVICE, "wide scan launch failed: %s", hipGetErrorString(e));
        return QV_OK;
    }
    if (kk <= (uint32_t)qv::kMaxSelectK) {
        hipError_t e = qv::launch_flat_select(v, plan, d_queries, nq, kk, k_stride, ws, d_rows_out, d_dist_out, s);
        if (e != hipSuccess) return fail(QV_ERR_DEVICE, "scan + select launch failed: %s", hipGetErrorString(e));
        return QV_OK;
    }
    // full-ranking path (e.g. a filtered search asking for k = N, collection.go:679-682)
    for (uint32_t q = 0; q < nq; q++) {
        hipError_t e = qv::launch_flat_fullsort(v, plan, d_queries + (size_t)q * idx->dim, k_stride, ws,
                                                d_rows_out + (size_t)q * k_stride, d_dist_out + (size_t)q * k_stride, s);
        if (e != hipSuccess) return fail(QV_ERR_DEVICE, "full-sort launch failed: %s", hipGetErrorString(e));
    }
    return QV_OK;
}

// tickets / cand_tiles / candidates: as the call will be enqueued (flat_plan, wide_route) — a call whose route is a bound scan is sized for it, no other call is
static size_t search_ws_bytes(const qv_index* idx, uint32_t nq, uint32_t kk, uint32_t k_stride, bool tickets, uint32_t cand_tiles = qv::kBoundNoFilter, uint64_t candidates = 0) {
    const uint32_t n_tiles = (idx->n_rows + 63) / 64;
    const qv::ScanPlan plan = qv::plan_scan(n_tiles, idx->cus);
    if (kk <= (uint32_t)qv::kMaxFusedK && kk == k_stride) {
        const qv::FlatPlan fp = flat_plan(idx, nq, kk, tickets, cand_tiles);
        const qv::FlatWs what = fp.route == qv::FlatRoute::bound_mq ? qv::FlatWs::call_bound_mq
                              : fp.route == qv::FlatRoute::bound || fp.route == qv::FlatRoute::bound8_first ? qv::FlatWs::call_bound : qv::FlatWs::call;
        return qv::flat_layout(nullptr, what, plan, nq, kk, n_tiles, idx->dim).total;
    }
    if (wide_route(idx, nq, kk, k_stride, tickets, cand_tiles, candidates)) return qv::bound_scan_wide_workspace_bytes(plan, kk, n_tiles, idx->dim);
    if (wide_route_mq(idx, nq, kk, k_stride, tickets, cand_tiles != qv::kBoundNoFilter)) return qv::bound_scan_wide_mq_workspace_bytes(plan, nq, kk, n_tiles, idx->dim);
    if (kk > (uint32_t)qv::kMaxFusedK && kk <= (uint32_t)qv::kMaxWideK && nq == 1) return qv::flat_wide_workspace_bytes(plan, nq, kk);
    if (kk <= (uint32_t)qv::kMaxSelectK) return qv::flat_select_workspace_bytes(n_tiles, nq, kk, idx->dim4);
    return qv::full_sort_workspace_bytes(n_tiles);
}

// ---------------------------------------------------------------- what every host-pointer search is made of: checks, passes, a staged call --
// The argument checks of the host forms, in the reference's order; each form passes its own wording.  *done: nothing to run, the call
// returns QV_OK — no query, or (exact.go:96-98) an empty index: an empty result and a nil error.  check_host_inputs ends in front of
// the empty index, where qv_index_search_rowsets checks its sets; check_host_outputs goes on from there.
static int check_host_inputs(const qv_index* idx, uint32_t nq, bool inputs, const char* inputs_null, bool* done) {
    *done = false;
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (nq == 0) { *done = true; return QV_OK; }
    if (!inputs) return fail(QV_ERR_INVALID_ARG, "%s", inputs_null);
    return QV_OK;
}
static int check_host_outputs(const qv_index* idx, uint32_t nq, uint32_t k, bool outputs, const char* outputs_null, uint32_t* count_out, bool* done) {
    *done = idx->n_live == 0;
    if (*done) { for (uint32_t q = 0; q < nq; q++) count_out[q] = 0; return QV_OK; }
    if (k == 0) return fail(QV_ERR_K_NOT_POSITIVE, "k must be positive");        // exact.go:104-106
    if (!outputs) return fail(QV_ERR_INVALID_ARG, "%s", outputs_null);
    return QV_OK;
}
static int check_host_args(const qv_index* idx, uint32_t nq, uint32_t k, bool inputs, const char* inputs_null, bool outputs, const char* outputs_null,
                           uint32_t* count_out, bool* done) {
    const int rc = check_host_inputs(idx, nq, inputs, inputs_null, done);
    return rc != QV_OK || *done ? rc : check_host_outputs(idx, nq, k, outputs, outputs_null, count_out, done);
}

// Very large batches go in passes, which bounds the workspace and the staging buffers: fn(q0, m) for every pass of at most `batch` queries
constexpr uint32_t kHostBatch = 8192;   // queries per device pass of the host-pointer entry points
extern "C++" {
template <typename Fn> static int in_passes(uint32_t nq, uint32_t batch, Fn&& fn) {
    for (uint32_t q0 = 0; q0 < nq; q0 += batch) {
        const int rc = fn(q0, std::min(batch, nq - q0));
        if (rc != QV_OK) return rc;
    }
    return QV_OK;
}
}

// The matrix-core filter walks the corpus once per 256 queries, so 257-320 queries cost two walks (2.6 ms against 1.4 ms at 1M x 768)
// while a batch of 64 or fewer costs half a walk: beyond 256 queries a remainder of 1..64 goes in a call of its own (0 = no split).
static uint32_t short_tail(uint32_t nq) {
    const uint32_t rem = nq % 256;
    return nq > 256 && rem >= 1 && rem <= 64 ? rem : 0;
}

// list i of n staged lists (stride `stride`, kk results each) into the caller's arrays at stride k, as list dest[i] (null: i), padded past kk
static void deliver_lists(const uint32_t* h_rows, const float* h_dist, uint32_t n, uint32_t stride, uint32_t kk, uint32_t k,
                          uint32_t* rows_out, float* dist_out, const uint32_t* dest = nullptr) {
    for (uint32_t i = 0; i < n; i++) {
        uint32_t* r = rows_out + (size_t)(dest ? dest[i] : i) * k;
        float* d = dist_out + (size_t)(dest ? dest[i] : i) * k;
        memcpy(r, h_rows + (size_t)i * stride, (size_t)kk * sizeof(uint32_t));
        memcpy(d, h_dist + (size_t)i * stride, (size_t)kk * sizeof(float));
        for (uint32_t j = kk; j < k; j++) { r[j] = 0xFFFFFFFFu; d[j] = __builtin_inff(); }
    }
}
// the listed queries side by side (a redo: the queries a batch handed back)
static void gather_queries(float* dst, const float* queries, const std::vector<uint32_t>& which, uint32_t dim) {
    for (size_t i = 0; i < which.size(); i++) memcpy(dst + i * dim, queries + (size_t)which[i] * dim, dim * sizeof(float));
}

// One staged host-pointer call: what every such form does around its launches.  A pooled context of its own (stream, pinned and device
// staging, workspace, ticket words) from open / acquire until the struct goes or release(); queries go pinned -> device, lists come
// device -> pinned -> the caller's arrays.  The forms keep what is theirs: which filter, which plan, which launch.
struct HostCall {
    qv_index* idx;
    SearchCtx* c = nullptr;
    explicit HostCall(qv_index* i) : idx(i) {}
    ~HostCall() { release(); }
    HostCall(const HostCall&) = delete;
    HostCall& operator=(const HostCall&) = delete;

    int open() { HIPCHK(hipSetDevice(idx->device)); return acquire(); }
    int acquire() { return acquire_ctx(idx, &c); }
    void release() { if (c) release_ctx(idx, c); c = nullptr; }
    // staging for n_vec query vectors and n_lists lists of list_len results (dist_planes: distance arrays behind each other per call)
    int reserve(size_t n_vec, size_t n_lists, size_t list_len, size_t dist_planes = 1) {
        const size_t qbytes = n_vec * idx->dim * sizeof(float), obytes = n_lists * list_len * sizeof(uint32_t);
        int rc;
        if ((rc = c->d_q.ensure(qbytes)) || (rc = c->h_q.ensure(qbytes)) || (rc = c->d_rows.ensure(obytes)) || (rc = c->d_dist.ensure(dist_planes * obytes)) ||
            (rc = c->h_rows.ensure(obytes)) || (rc = c->h_dist.ensure(dist_planes * obytes)))
            return rc;
        planes = dist_planes;
        return QV_OK;
    }
    int workspace(size_t bytes) { return c->ws.ensure(bytes); }
    // The context's ticket words (the single-launch scans'; the bound scans' control words behind them): zeroed once, left zero by the
    // kernels.  Zeroed ON THE CONTEXT'S STREAM, ahead of the kernels that read them, for the reason given in stream_workspace.
    int tickets(uint32_t** out) {
        if (!c->tickets.p) {
            const int rc = c->tickets.ensure(256);
            if (rc != QV_OK) return rc;
            HIPCHK(hipMemsetAsync(c->tickets.p, 0, 256, c->stream));
        }
        *out = static_cast<uint32_t*>(c->tickets.p);
        return QV_OK;
    }
    // queries: into pinned memory (stage / stage_gather), from there to the device (send)
    void stage(const float* vectors, size_t n_vec, size_t at_vec = 0) { memcpy(h_queries() + at_vec * idx->dim, vectors, n_vec * idx->dim * sizeof(float)); }
    void stage_gather(const float* queries, const std::vector<uint32_t>& which) { gather_queries(h_queries(), queries, which, idx->dim); }
    int send(size_t n_vec) {
        HIPCHK(hipMemcpyAsync(c->d_q.p, c->h_q.p, n_vec * idx->dim * sizeof(float), hipMemcpyHostToDevice, c->stream));
        return QV_OK;
    }
    // results: n lists at staging stride `stride`, device -> pinned; enqueued, not waited for (sync)
    int fetch(size_t n, size_t stride) {
        const size_t obytes = n * stride * sizeof(uint32_t);
        HIPCHK(hipMemcpyAsync(c->h_rows.p, c->d_rows.p, obytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(c->h_dist.p, c->d_dist.p, planes * obytes, hipMemcpyDeviceToHost, c->stream));
        return QV_OK;
    }
    int sync() { HIPCHK(hipStreamSynchronize(c->stream)); return QV_OK; }
    // ... and pinned -> the caller's arrays at stride k (deliver_lists)
    void deliver(uint32_t n, uint32_t stride, uint32_t kk, uint32_t k, uint32_t* rows_out, float* dist_out, const uint32_t* dest = nullptr) const {
        deliver_lists(h_rows(), h_dist(), n, stride, kk, k, rows_out, dist_out, dest);
    }

    hipStream_t stream() const { return c->stream; }
    void* ws() const { return c->ws.p; }
    float* h_queries() const { return static_cast<float*>(c->h_q.p); }
    const float* d_queries() const { return static_cast<const float*>(c->d_q.p); }
    uint32_t* d_rows() const { return static_cast<uint32_t*>(c->d_rows.p); }
    float* d_dist() const { return static_cast<float*>(c->d_dist.p); }
    uint32_t* h_rows() const { return static_cast<uint32_t*>(c->h_rows.p); }
    float* h_dist() const { return static_cast<float*>(c->h_dist.p); }
private:
    size_t planes = 1;
};

// one pass of the exact scans (single-query / multi-query / full ranking): up to kHostBatch queries, the arguments checked
static int exact_pass(qv_index* idx, const float* queries, uint32_t nq, uint32_t k, uint32_t* rows_out, float* dist_out, uint32_t* count_out) {
    const uint32_t kk = std::min(k, idx->n_live);                                // exact.go:109-111
    HostCall hc(idx);
    int rc;
    if ((rc = hc.open()) || (rc = hc.reserve(nq, nq, kk)) || (rc = hc.workspace(search_ws_bytes(idx, nq, kk, kk, true)))) return rc;
    SearchCtx* c = hc.c;
    hc.stage(queries, nq);
    // small result sets are written by the last kernel straight into the (device-visible) pinned buffers: two copy commands less
    // on the latency path of a single query; large ones go through device buffers and DMA.  On a small corpus (few workgroups,
    // each staging the query once) the query is read from the pinned buffer too: no copy command at all.
    const bool direct = (size_t)nq * kk <= 1024;
    const bool q_direct = direct && nq <= 4 && idx->n_rows <= 262144;
    if (!q_direct && (rc = hc.send(nq))) return rc;
    // small collections: one launch for scan + merge, and the host polls a sequence number the kernel writes behind its results
    // instead of waiting for the stream
    SearchExtras x;
    bool flag_used = false;
    if ((rc = hc.tickets(&x.d_tickets))) return rc;                    // single-launch scans: the small collection's, and one query over a large one
    // (any single query whose scan is short enough to poll for: up to ~4 GB of rows, about half a millisecond)
    if (direct && (q_direct || (nq == 1 && (uint64_t)idx->n_rows * idx->dim4 * 16 <= (4ull << 30)))) {
        if (!c->h_flag.p) { if ((rc = c->h_flag.ensure(64))) return rc; *static_cast<volatile uint32_t*>(c->h_flag.p) = 0; }
        x.done_flag = static_cast<uint32_t*>(c->h_flag.p);
        c->flag_seq++;
    }
    x.done_seq = c->flag_seq; x.flag_used = &flag_used;
    rc = enqueue_search(idx, q_direct ? hc.h_queries() : hc.d_queries(), nq, kk, kk, hc.ws(), direct ? hc.h_rows() : hc.d_rows(), direct ? hc.h_dist() : hc.d_dist(), hc.stream(), x);
    if (rc != QV_OK) return rc;
    if (!direct && (rc = hc.fetch(nq, kk))) return rc;
    bool seen = false;
    if (flag_used) {
        const volatile uint32_t* f = static_cast<const volatile uint32_t*>(c->h_flag.p);
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t spin = 0; !(seen = *f == c->flag_seq); spin++) {
            __builtin_ia32_pause();
            if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;   // something else holds the GPU: wait properly
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        if (seen && (c->flag_seq & 63u) == 0 && (rc = hc.sync())) return rc;   // (lets the runtime retire its finished commands now and then)
    }
    if (!seen && (rc = hc.sync())) return rc;
    hc.deliver(nq, kk, kk, k, rows_out, dist_out);
    for (uint32_t q = 0; q < nq; q++) count_out[q] = kk;
    return QV_OK;
}

// the exact scans, host pointers
static int exact_search_host(qv_index* idx, const float* queries, uint32_t nq, uint32_t k,
                             uint32_t* rows_out, float* dist_out, uint32_t* count_out) {
    bool done;
    if (const int rc = check_host_args(idx, nq, k, queries && count_out, "queries/count_out is null", rows_out && dist_out, "rows_out/dist_out is null", count_out, &done); rc != QV_OK || done)
        return rc;
    return in_passes(nq, kHostBatch, [&](uint32_t q0, uint32_t m) {
        return exact_pass(idx, queries + (size_t)q0 * idx->dim, m, k, rows_out + (size_t)q0 * k, dist_out + (size_t)q0 * k, count_out + q0);
    });
}

// one call's worth of queries, in a context of the caller's own (what qv_index_search was before callers could share passes)
static int search_direct(qv_index* idx, const float* queries, uint32_t nq, uint32_t k,
                         uint32_t* rows_out, float* dist_out, uint32_t* count_out) {
    // many queries over a large corpus: the matrix-core filter + exact re-score returns the identical result faster (from 9 queries
    // with the bfloat16 filters, 32 with the fp32 one: batched_supported holds the measured crossovers)
    if (idx && k > 0 && idx->n_live >= 4 * (uint64_t)k && qv::batched_supported(idx->view(), nq, std::min(k, idx->n_live)))
        return qv_index_search_batched(idx, queries, nq, k, rows_out, dist_out, count_out);
    return exact_search_host(idx, queries, nq, k, rows_out, dist_out, count_out);
}

// Callers that may share a pass: small requests (the reference's host sends one query per call) with fused-list k over a corpus
// large enough that a pass costs more than a launch and a wake-up.  Everything else runs on its own as before — so does a
// request that fails a check, which must report the reference's error in the reference's order (exact.go:96-106).
constexpr uint32_t kCoalesceMaxNq = 8;
static bool coalesce_applies(const qv_index* idx, const float* queries, uint32_t nq, uint32_t k,
                             const uint32_t* rows_out, const float* dist_out, const uint32_t* count_out) {
    static const bool off = getenv("QV_COALESCE") && atoi(getenv("QV_COALESCE")) == 0;   // measurement switch, read once per process
    return !off && idx && queries && rows_out && dist_out && count_out && nq >= 1 && nq <= kCoalesceMaxNq && k >= 1 && k <= (uint32_t)qv::kMaxFusedK &&
           idx->n_live > 0;
}
// Passes in flight by what a pass costs: a scan of hundreds of megabytes is HBM-bound and a second one beside it only halves both (one
// lane); a small collection's pass is launch and wait latency, which concurrent passes on their own streams hide — until there are so
// many callers that the launches themselves queue up, and then the callers share passes there too.  Measured with 8 / 64 callers
// (profiles/r05_notes.md): 12k x 768 with ONE lane 42 k / 155 k QPS against 102 k / 44 k for every call on its own.
static int coalesce_lanes(const qv_index* idx) {
    static const int forced = getenv("QV_FLAT_LANES") ? atoi(getenv("QV_FLAT_LANES")) : 0;              // measurement switch, read once
    if (forced > 0) return forced;
    // a scan of 256 MiB or more fills the memory system by itself: one pass at a time, and its leader holds the group open for the
    // callers the previous pass released.  Below that a single-query pass leaves most of the device idle and a multi-query pass costs
    // more than it: four passes side by side, nobody held (profiles/r05_notes.md, the lane sweep at 5 MiB - 300 MiB).
    const uint64_t bytes = (uint64_t)idx->n_rows * idx->dim4 * 16;
    return bytes >= ((uint64_t)256 << 20) ? 1 : 4;
}

// Lanes and group sizes of a front by what a pass over this index costs (qv_index_search's front and, with the same thresholds,
// qv_index_search_rowsets')
static void configure_front(const qv_index* idx, qvco::Front& front) {
    {   // Lanes by size (coalesce_lanes); and on the smallest collections short shared passes: up to 32 queries a pass is the partial-chain
        // form of the scan (k_flat_scan_split_mq: 16 queries over 10 k x 768 in 87 us), beyond it the multi-query kernels (64 queries: 215 us), so
        // 16 per pass and four passes side by side carry more — callers on 10 k x 768 at 64 / 256 / 1024: 497 k / 473 k / 479 k QPS against 355 k /
        // 280 k / 107 k with passes of up to 256; 10 k x 128: 517 k / 253 k / 256 k against 508 k / 181 k / 101 k.  QV_FLAT_SMALL_GROUP overrides (measurements).
        const int lanes = coalesce_lanes(idx);
        front.set_lanes(lanes, lanes == 1);
        static const int small_group = getenv("QV_FLAT_SMALL_GROUP") ? atoi(getenv("QV_FLAT_SMALL_GROUP")) : 0;
        const uint64_t bytes = (uint64_t)idx->n_rows * idx->dim4 * 16;
        // (64 - 256 MiB, still four lanes: 30 k x 768 at 256 / 1024 callers 445 k / 483 k QPS with passes of up to 64 against 425 k / 210 k with 256 and
        // 283 k / 261 k with 32; 60 k x 768 459 k / 459 k with 32 against 279 k / 99 k with 256 and 320 k / 156 k with 64; 80 k x 768 408 k / 392 k against 303 k / 105 k)
        const uint32_t by_size = bytes < ((uint64_t)64 << 20) ? 16u : (bytes < ((uint64_t)128 << 20) ? 64u : 32u);
        // (one lane, 256 MiB and more: 100 k x 768 at 256 / 1024 / 2048 callers 525 k / 463 k / 508 k QPS with passes of up to 128 against 350 k / 256 k / 189 k
        // with 256; 300 k x 768 374 k / 375 k / 355 k against 302 k / 289 k / 405 k; 1M x 768 200 k / 191 k / 194 k against 207 k / 289 k / 304 k: 128 below 1 GiB)
        static const int big_group = getenv("QV_FLAT_BIG_GROUP") ? atoi(getenv("QV_FLAT_BIG_GROUP")) : 0;
        const uint32_t one_lane = big_group > 0 ? (uint32_t)std::max(big_group, 8) : (bytes < ((uint64_t)1 << 30) ? 128u : 256u);
        front.set_max_group(lanes > 1 ? (small_group > 0 ? (uint32_t)std::max(small_group, 8) : by_size) : one_lane);
    }
}

// One call through a coalescing front (coalesce_applies holds): the caller runs alone (solo), leads a group — group(g): the members' queries
// side by side in g, its outputs sized — or rides one.  tag: what a leader needs of each member beside its queries.
extern "C++" {
template <typename Solo, typename GroupRun>
static int front_submit(const qv_index* idx, qvco::Front& front, const float* queries, uint32_t nq, uint32_t k,
                        uint32_t* rows_out, float* dist_out, uint32_t* count_out, const void* tag, Solo&& solo, GroupRun&& group) {
    configure_front(idx, front);
    char err[256]; err[0] = 0;
    const int rc = front.submit(
        0, queries, nq, idx->dim, k, rows_out, dist_out, count_out, nullptr, solo,
        [&](qvco::Group& g, auto&) { g.size_outputs(false); return group(g); },
        [] { return qv_last_error(); }, err, sizeof(err), tag);
    if (rc != QV_OK && err[0]) return fail(rc, "%s", err);                // (a rider's message comes from the thread that ran its group)
    return rc;
}
}

int qv_index_search(qv_index* idx, const float* queries, uint32_t nq, uint32_t k,
                    uint32_t* rows_out, float* dist_out, uint32_t* count_out) {
    if (!coalesce_applies(idx, queries, nq, k, rows_out, dist_out, count_out)) return search_direct(idx, queries, nq, k, rows_out, dist_out, count_out);
    return front_submit(idx, idx->front, queries, nq, k, rows_out, dist_out, count_out, nullptr,
                        [&] { return search_direct(idx, queries, nq, k, rows_out, dist_out, count_out); },
                        [&](qvco::Group& g) { return search_direct(idx, g.queries(), g.nq, g.kmax, g.rows.data(), g.dist.data(), g.count.data()); });
}

int qv_index_coalesce_stats(qv_index* idx, uint64_t out[8]) {
    if (!idx || !out) return fail(QV_ERR_INVALID_ARG, "index/out is null");
    idx->front.stats.read(out);
    return QV_OK;
}
int qv_index_coalesce_early_rounds(qv_index* idx, uint64_t* out) {
    if (!idx || !out) return fail(QV_ERR_INVALID_ARG, "index/out is null");
    *out = idx->front.stats.early();
    return QV_OK;
}

// Search with a negative example, device side of hybrid_index.go:517-570 / hnsw/adapter.go:345-437: the reference fetches
// retrieveK = max(2k, 30) nearest results, then calls the distance function once more per result against the negative
// example and re-ranks by d - w * d_neg.  Which rows are candidates depends on d alone, so the device part is: the flat scan
// for k_fetch results, then — on the same stream, row ids never leaving the device — the neighbour-batch kernel for those
// rows against the negative vector.  ONE call, one synchronisation; the host combines two floats per row and sorts <= 30
// records by (score, string id).
int qv_index_search_negative(qv_index* idx, const float* query, const float* negative, uint32_t k_fetch,
                             uint32_t* rows_out, float* dist_out, float* neg_dist_out, uint32_t* count_out) {
    bool done;
    if (const int rc0 = check_host_args(idx, 1, k_fetch, query && negative && count_out, "query/negative/count_out is null",
                                        rows_out && dist_out && neg_dist_out, "rows_out/dist_out/neg_dist_out is null", count_out, &done); rc0 != QV_OK || done)
        return rc0;
    const uint32_t kk = std::min(k_fetch, idx->n_live);
    HostCall hc(idx);
    int rc;
    // (the context's ticket words only where the wide bound scan takes the fetch — max(2k, 30) results, so every k >= 33: without them
    //  every path is the one this call has always taken)
    const bool wide = wide_route(idx, 1, kk, kk, true, qv::kBoundNoFilter, 0) != 0;
    if ((rc = hc.open()) || (rc = hc.reserve(2, 1, kk, 2)) || (rc = hc.workspace(search_ws_bytes(idx, 1, kk, kk, wide)))) return rc;
    SearchExtras x;
    if (wide && (rc = hc.tickets(&x.d_tickets))) return rc;
    hc.stage(query, 1);
    hc.stage(negative, 1, 1);
    if ((rc = hc.send(2))) return rc;
    rc = enqueue_search(idx, hc.d_queries(), 1, kk, kk, hc.ws(), hc.d_rows(), hc.d_dist(), hc.stream(), x);
    if (rc != QV_OK) return rc;
    hipError_t e = qv::launch_distance_rows(idx->view(), hc.d_queries() + idx->dim, hc.d_rows(), kk, hc.d_dist() + kk, hc.stream());   // the second plane: the distances to the negative example
    if (e != hipSuccess) return fail(QV_ERR_DEVICE, "distance_rows launch failed: %s", hipGetErrorString(e));
    if ((rc = hc.fetch(1, kk)) || (rc = hc.sync())) return rc;
    hc.deliver(1, kk, kk, k_fetch, rows_out, dist_out);
    memcpy(neg_dist_out, hc.h_dist() + kk, (size_t)kk * sizeof(float));
    for (uint32_t i = kk; i < k_fetch; i++) neg_dist_out[i] = __builtin_inff();
    *count_out = kk;
    return QV_OK;
}

// one pass of qv_index_search_masked: up to kHostBatch queries, the arguments checked
static int masked_pass(qv_index* idx, const float* queries, uint32_t nq, uint32_t k, const uint64_t* mask,
                       uint32_t* rows_out, float* dist_out, uint32_t* count_out) {
    HostCall hc(idx);
    int rc = hc.open();
    if (rc != QV_OK) return rc;
    SearchCtx* c = hc.c;
    // candidates = live AND selected; the tile loop reads whole 64-row words, so the bitmap covers every tile
    const size_t words = ((size_t)idx->n_rows + 63) / 64;
    if ((rc = c->h_mask.ensure(words * 8)) || (rc = c->d_mask.ensure(words * 8))) return rc;
    uint64_t* hm = static_cast<uint64_t*>(c->h_mask.p);
    uint64_t matching = 0;
    uint32_t cand_tiles = 0;                                          // tiles that hold a candidate: the filtered bound-scan rule's input
    for (size_t w = 0; w < words; w++) {
        const uint64_t a = w < idx->alive_host.size() ? idx->alive_host[w] : 0;
        hm[w] = a & mask[w];
        matching += (uint64_t)__builtin_popcountll(hm[w]);
        cand_tiles += hm[w] != 0 ? 1u : 0u;
    }
    const uint32_t kk = (uint32_t)std::min<uint64_t>(k, matching);                // the first k matches of the full ranking
    for (uint32_t q = 0; q < nq; q++) count_out[q] = kk;
    if (kk == 0) return QV_OK;
    if ((rc = hc.reserve(nq, nq, kk))) return rc;
    // the bound scan under the mask when the filtered rule takes it — up to 64 results plan_flat's, from 65 the wide form's —: then, and only
    // then, the call carries the context's ticket words (without them every path is the one a masked search has always taken)
    const bool bound = kk <= (uint32_t)qv::kMaxFusedK ? flat_plan(idx, nq, kk, true, cand_tiles).bound() : wide_route(idx, nq, kk, kk, true, cand_tiles, matching) != 0;
    if ((rc = hc.workspace(search_ws_bytes(idx, nq, kk, kk, bound, cand_tiles, matching)))) return rc;
    SearchExtras x;
    x.d_candidates = static_cast<const uint64_t*>(c->d_mask.p); x.candidate_tiles = cand_tiles; x.candidates = matching;
    if (bound && (rc = hc.tickets(&x.d_tickets))) return rc;
    hc.stage(queries, nq);
    HIPCHK(hipMemcpyAsync(c->d_mask.p, c->h_mask.p, words * 8, hipMemcpyHostToDevice, c->stream));
    if ((rc = hc.send(nq))) return rc;
    rc = enqueue_search(idx, hc.d_queries(), nq, kk, kk, hc.ws(), hc.d_rows(), hc.d_dist(), hc.stream(), x);
    if (rc != QV_OK) return rc;
    if ((rc = hc.fetch(nq, kk)) || (rc = hc.sync())) return rc;
    hc.deliver(nq, kk, kk, k, rows_out, dist_out);
    return QV_OK;
}

int qv_index_search_masked(qv_index* idx, const float* queries, uint32_t nq, uint32_t k, const uint64_t* mask,
                           uint32_t* rows_out, float* dist_out, uint32_t* count_out) {
    bool done;
    if (const int rc = check_host_args(idx, nq, k, queries && count_out && mask, "queries/mask/count_out is null", rows_out && dist_out, "rows_out/dist_out is null", count_out, &done);
        rc != QV_OK || done)
        return rc;
    return in_passes(nq, kHostBatch, [&](uint32_t q0, uint32_t m) {
        return masked_pass(idx, queries + (size_t)q0 * idx->dim, m, k, mask, rows_out + (size_t)q0 * k, dist_out + (size_t)q0 * k, count_out + q0);
    });
}

// ---------------------------------------------------------------- row sets: one device-resident filter per query --
int qv_rowset_create(qv_rowset** out, qv_index* idx, const uint64_t* mask) {
    if (!out) return fail(QV_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    HIPCHK(hipSetDevice(idx->device));
    qv_rowset* rs = new (std::nothrow) qv_rowset();
    if (!rs) return fail(QV_ERR_OOM, "out of host memory");
    rs->idx = idx; rs->device = idx->device;
    rs->words = (uint32_t)(((uint64_t)idx->n_rows + 63) / 64);
    rs->host.assign(rs->words, 0);
    if (mask && rs->words) {
        memcpy(rs->host.data(), mask, (size_t)rs->words * 8);
        if (idx->n_rows & 63) rs->host[rs->words - 1] &= (1ull << (idx->n_rows & 63)) - 1;    // rows that do not exist yet start unselected
    }
    for (uint64_t w : rs->host) { rs->tiles += w != 0 ? 1u : 0u; rs->selected += (uint64_t)__builtin_popcountll(w); }
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&rs->d_bits), std::max<size_t>((size_t)rs->words * 8, 256));
    if (e == hipSuccess && rs->words) e = hipMemcpy(rs->d_bits, rs->host.data(), (size_t)rs->words * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);           // (the index's streams are non-blocking: nothing of theirs may overtake the upload)
    if (e != hipSuccess) {
        (void)hipFree(rs->d_bits); delete rs;
        return fail(e == hipErrorOutOfMemory ? QV_ERR_OOM : QV_ERR_DEVICE, "row set upload failed: %s", hipGetErrorString(e));
    }
    *out = rs;
    return QV_OK;
}

int qv_rowset_set_rows(qv_rowset* rs, const uint32_t* rows, uint32_t n, int selected) {
    if (!rs) return fail(QV_ERR_INVALID_ARG, "row set is null");
    if (n == 0) return QV_OK;
    if (!rows) return fail(QV_ERR_INVALID_ARG, "rows is null");
    qv_index* idx = rs->idx;
    for (uint32_t i = 0; i < n; i++)
        if (rows[i] >= idx->n_rows) return fail(QV_ERR_OUT_OF_RANGE, "row %u out of range (rows: %u)", rows[i], idx->n_rows);
    HIPCHK(hipSetDevice(idx->device));
    const uint32_t need = (uint32_t)(((uint64_t)idx->n_rows + 63) / 64);
    if (need > rs->words) {                                           // the index has grown since: the new rows' words, all unselected
        hipError_t e = regrow(&rs->d_bits, (size_t)rs->words * 8, (size_t)need * 8);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? QV_ERR_OOM : QV_ERR_DEVICE, "row set growth failed: %s", hipGetErrorString(e));
        rs->host.resize(need, 0);
        rs->words = need;
    }
    { const int rc0 = rs->stage.ensure((size_t)n * sizeof(uint32_t)); if (rc0 != QV_OK) return rc0; }
    uint32_t* d = static_cast<uint32_t*>(rs->stage.p);
    hipError_t e = hipMemcpy(d, rows, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = qv::launch_rowset_set_rows(rs->d_bits, d, n, selected, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return fail(QV_ERR_DEVICE, "row set update failed: %s", hipGetErrorString(e));
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t bit = 1ull << (rows[i] & 63);
        uint64_t& w = rs->host[rows[i] >> 6];
        const uint64_t before = w;
        if (selected) w |= bit; else w &= ~bit;
        if (w != before) { if (selected) rs->selected++; else rs->selected--; }
        if (before == 0 && w != 0) rs->tiles++;                       // the count of non-empty words
        else if (before != 0 && w == 0) rs->tiles--;
    }
    return QV_OK;
}

uint64_t qv_rowset_count(const qv_rowset* rs) {
    if (!rs) return 0;
    uint64_t n = 0;
    for (uint64_t w : rs->host) n += (uint64_t)__builtin_popcountll(w);
    return n;
}

void qv_rowset_destroy(qv_rowset* rs) {
    if (!rs) return;
    // (no device-wide wait: the caller's exclusion — include/qv.h — says that no search naming this set is in flight or enqueued, and
    // nothing else reads its words)
    (void)hipSetDevice(rs->device);
    (void)hipFree(rs->d_bits);
    rs->stage.release();
    delete rs;
}

static qv::RowSetRef rowset_ref(const qv_rowset* rs) { return rs ? qv::RowSetRef{rs->d_bits, rs->words, 0} : qv::RowSetRef{nullptr, 0, 0}; }
// live rows of a set, from the host mirrors (the k > 64 paths clamp their list length to it, as qv_index_search_masked does)
static uint64_t rowset_live(const qv_index* idx, const qv_rowset* rs) {
    if (!rs) return idx->n_live;
    uint64_t n = 0;
    const size_t words = std::min<size_t>(rs->host.size(), idx->alive_host.size());
    for (size_t w = 0; w < words; w++) n += (uint64_t)__builtin_popcountll(rs->host[w] & idx->alive_host[w]);
    return n;
}

// ---------------------------------------------------------------- facet columns: row sets made on the device (qv_where.hip) --
int qv_column_create(qv_column** out, qv_index* idx, int type) {
    if (!out) return fail(QV_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (type != QV_COL_F64 && type != QV_COL_U32) return fail(QV_ERR_INVALID_ARG, "unknown column type %d", type);
    qv_column* col = new (std::nothrow) qv_column();
    if (!col) return fail(QV_ERR_OOM, "out of host memory");
    col->idx = idx; col->device = idx->device; col->type = type;
    *out = col;
    return QV_OK;
}

int qv_column_set(qv_column* col, uint32_t first_row, uint32_t n, const void* values, const uint8_t* present) {
    if (!col) return fail(QV_ERR_INVALID_ARG, "column is null");
    qv_index* idx = col->idx;
    if ((uint64_t)first_row + n > idx->n_rows)
        return fail(QV_ERR_OUT_OF_RANGE, "rows [%u, %llu) reach past the index (rows: %u)", first_row, (unsigned long long)first_row + n, idx->n_rows);
    if (n == 0) return QV_OK;
    if (!values) return fail(QV_ERR_INVALID_ARG, "values is null");
    HIPCHK(hipSetDevice(idx->device));
    if (((uint64_t)first_row + n + 63) / 64 > col->cap_tiles) {       // to the index's current rows, as a row set grows: new tiles are zero (no value)
        const uint32_t need = (uint32_t)(((uint64_t)idx->n_rows + 63) / 64);
        const size_t tb = 64 * col->elem();
        hipError_t e = regrow(reinterpret_cast<char**>(&col->d_values), (size_t)col->cap_tiles * tb, (size_t)need * tb);
        if (e == hipSuccess) e = regrow(&col->d_present, (size_t)col->cap_tiles * 8, (size_t)need * 8);    // (a failure here leaves the values longer than the presence words: harmless)
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? QV_ERR_OOM : QV_ERR_DEVICE, "column growth failed: %s", hipGetErrorString(e));
        col->cap_tiles = need;
    }
    const uint8_t* d_bytes = nullptr;
    if (present) {
        const int rc0 = col->stage.ensure(n);
        if (rc0 != QV_OK) return rc0;
        d_bytes = static_cast<const uint8_t*>(col->stage.p);
    }
    hipError_t e = hipMemcpy(static_cast<char*>(col->d_values) + (size_t)first_row * col->elem(), values, (size_t)n * col->elem(), hipMemcpyHostToDevice);
    if (e == hipSuccess && present) e = hipMemcpy(col->stage.p, present, n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = qv::launch_column_presence(col->d_present, first_row, n, d_bytes, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return fail(QV_ERR_DEVICE, "column update failed: %s", hipGetErrorString(e));
    col->rows = std::max(col->rows, first_row + n);
    return QV_OK;
}

uint32_t qv_column_rows(const qv_column* col) { return col ? col->rows : 0; }

void qv_column_destroy(qv_column* col) {
    if (!col) return;
    (void)hipSetDevice(col->device);                                  // (no device-wide wait: the caller's exclusion says that no evaluation naming this column is running)
    (void)hipFree(col->d_values);
    (void)hipFree(col->d_present);
    col->stage.release();
    delete col;
}

// the host mirror and the counts the searches read, from the words a kernel has just written (the null stream: the copy waits for it)
static int rowset_mirror(qv_rowset* rs) {
    rs->host.assign(rs->words, 0);
    if (rs->words) HIPCHK(hipMemcpy(rs->host.data(), rs->d_bits, (size_t)rs->words * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipStreamSynchronize(nullptr));
    rs->tiles = 0; rs->selected = 0;
    for (uint64_t w : rs->host) { rs->tiles += w != 0 ? 1u : 0u; rs->selected += (uint64_t)__builtin_popcountll(w); }
    return QV_OK;
}

// One conjunction's arguments, checked and turned into the table the kernels read (tab: zeroed by the caller): the checks of
// qv_rowset_create_where, which qv_index_search_where makes per query through this same function (its message names the query in front)
static int where_check(const qv_index* idx, const qv_column* const* cols, const int* ops, const double* literals, const uint32_t* lit_off,
                       uint32_t n_preds, qv::WhereTable& tab) {
    if (n_preds < 1 || n_preds > qv::kWherePreds) return fail(QV_ERR_INVALID_ARG, "1 to %u predicates per evaluation, got %u", qv::kWherePreds, n_preds);
    if (!cols || !ops || !lit_off) return fail(QV_ERR_INVALID_ARG, "cols, ops or lit_off is null");
    if (lit_off[0] != 0) return fail(QV_ERR_INVALID_ARG, "lit_off[0] must be 0");
    tab.n = n_preds;
    for (uint32_t p = 0; p < n_preds; p++) {
        const qv_column* c = cols[p];
        if (!c) return fail(QV_ERR_INVALID_ARG, "cols[%u] is null", p);
        if (c->idx != idx) return fail(QV_ERR_INVALID_ARG, "cols[%u] belongs to another index", p);
        const int op = ops[p];
        if (op < QV_PRED_EQ || op > QV_PRED_ABSENT) return fail(QV_ERR_INVALID_ARG, "ops[%u] = %d is not a predicate", p, op);
        if (lit_off[p + 1] < lit_off[p]) return fail(QV_ERR_INVALID_ARG, "lit_off must ascend");
        const uint32_t nl = lit_off[p + 1] - lit_off[p];
        const bool list = op == QV_PRED_IN || op == QV_PRED_NOT_IN, none = op == QV_PRED_PRESENT || op == QV_PRED_ABSENT;
        if (none ? nl != 0 : (list ? (nl < 1 || nl > qv::kWhereLits) : nl != 1))
            return fail(QV_ERR_INVALID_ARG, "predicate %u (op %d) takes %s, got %u", p, op, none ? "no literal" : (list ? "1 to 256 literals" : "one literal"), nl);
        if (nl && !literals) return fail(QV_ERR_INVALID_ARG, "literals is null");
        if (c->type == QV_COL_U32)
            for (uint32_t i = lit_off[p]; i < lit_off[p + 1]; i++) {
                const double v = literals[i];
                if (!(v >= 0.0 && v < 4294967296.0) || v != (double)(uint32_t)v)
                    return fail(QV_ERR_INVALID_ARG, "literal %u of predicate %u is not a uint32 code", i - lit_off[p], p);
            }
        qv::WherePred& w = tab.p[p];
        w.values = c->d_values; w.present = c->d_present; w.tiles = (uint32_t)(((uint64_t)c->rows + 63) / 64);
        w.type = c->type; w.op = op; w.lit0 = lit_off[p]; w.n_lit = nl;
    }
    return QV_OK;
}

// a real set from a checked conjunction: allocation, the pass on the null stream, the mirror (qv_rowset_create_where; and the runs of
// a k > 64 qv_index_search_where, which frees the set again before it returns)
static int rowset_from_where(qv_index* idx, const qv::WhereTable& tab, const double* literals, uint32_t n_lits, qv_rowset** out) {
    HIPCHK(hipSetDevice(idx->device));
    qv_rowset* rs = new (std::nothrow) qv_rowset();
    if (!rs) return fail(QV_ERR_OOM, "out of host memory");
    rs->idx = idx; rs->device = idx->device;
    rs->words = (uint32_t)(((uint64_t)idx->n_rows + 63) / 64);
    const size_t lit_bytes = std::max<size_t>((size_t)n_lits * sizeof(double), 8);
    int rc = rs->stage.ensure(lit_bytes);
    hipError_t e = hipSuccess;
    if (rc == QV_OK) {
        e = hipMalloc(reinterpret_cast<void**>(&rs->d_bits), std::max<size_t>((size_t)rs->words * 8, 256));
        if (e == hipSuccess && n_lits) e = hipMemcpy(rs->stage.p, literals, (size_t)n_lits * sizeof(double), hipMemcpyHostToDevice);
        const ProfilePair pp = e == hipSuccess ? profile_begin(idx, true, nullptr) : ProfilePair();   // qv_index_profile: the evaluation kernel alone, on the null stream
        if (e == hipSuccess) e = qv::launch_rowset_where(tab, static_cast<const double*>(rs->stage.p), idx->n_rows, rs->d_bits, idx->cus, nullptr);
        profile_end(idx, pp, e == hipSuccess, true, nullptr);
        if (e != hipSuccess) rc = fail(e == hipErrorOutOfMemory ? QV_ERR_OOM : QV_ERR_DEVICE, "row set evaluation failed: %s", hipGetErrorString(e));
    }
    if (rc == QV_OK) rc = rowset_mirror(rs);
    if (rc != QV_OK) { (void)hipFree(rs->d_bits); rs->stage.release(); delete rs; return rc; }
    *out = rs;
    return QV_OK;
}

int qv_rowset_create_where(qv_rowset** out, qv_index* idx, const qv_column* const* cols, const int* ops,
                           const double* literals, const uint32_t* lit_off, uint32_t n_preds) {
    if (!out) return fail(QV_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    qv::WhereTable tab{};
    { const int rc0 = where_check(idx, cols, ops, literals, lit_off, n_preds, tab); if (rc0 != QV_OK) return rc0; }
    return rowset_from_where(idx, tab, literals, lit_off[n_preds], out);
}

int qv_rowset_combine(qv_rowset* dst, const qv_rowset* a, const qv_rowset* b, int op) {
    if (!dst || !a || !b) return fail(QV_ERR_INVALID_ARG, "row set is null");
    if (op != QV_SET_AND && op != QV_SET_OR && op != QV_SET_ANDNOT) return fail(QV_ERR_INVALID_ARG, "unknown set operation %d", op);
    qv_index* idx = dst->idx;
    if (a->idx != idx || b->idx != idx) return fail(QV_ERR_INVALID_ARG, "row sets of different indexes");
    HIPCHK(hipSetDevice(idx->device));
    const uint32_t need = (uint32_t)(((uint64_t)idx->n_rows + 63) / 64);
    if (need > dst->words) {                                          // (dst may be a or b: they are read through the handles below, after this)
        hipError_t e = regrow(&dst->d_bits, (size_t)dst->words * 8, (size_t)need * 8);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? QV_ERR_OOM : QV_ERR_DEVICE, "row set growth failed: %s", hipGetErrorString(e));
        dst->host.resize(need, 0);
        dst->words = need;
    }
    const ProfilePair pp = profile_begin(idx, true, nullptr);         // qv_index_profile: the kernel alone, on the null stream
    hipError_t e = qv::launch_rowset_combine(rowset_ref(a), rowset_ref(b), op, dst->words, dst->d_bits, nullptr);
    profile_end(idx, pp, e == hipSuccess, true, nullptr);
    if (e != hipSuccess) return fail(QV_ERR_DEVICE, "row set combination failed: %s", hipGetErrorString(e));
    return rowset_mirror(dst);
}

int qv_rowset_read(const qv_rowset* rs, uint64_t* words_out, uint32_t n_words) {
    if (!rs) return fail(QV_ERR_INVALID_ARG, "row set is null");
    if (n_words == 0) return QV_OK;
    if (!words_out) return fail(QV_ERR_INVALID_ARG, "words_out is null");
    HIPCHK(hipSetDevice(rs->device));
    const uint32_t m = std::min(n_words, rs->words);
    if (m) HIPCHK(hipMemcpy(words_out, rs->d_bits, (size_t)m * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipStreamSynchronize(nullptr));
    memset(words_out + m, 0, (size_t)(n_words - m) * 8);
    return QV_OK;
}

// A checked conjunction of qv_index_search_where: the table the kernels read and the caller's literals (valid until its call returns);
// tab.n == 0: no predicate, every row.
struct WhereSpec { qv::WhereTable tab; const double* lits; uint32_t n_lits; };
static bool where_same(const WhereSpec& a, const WhereSpec& b) {      // bytewise equal: one evaluation serves both
    return a.n_lits == b.n_lits && memcmp(&a.tab, &b.tab, sizeof(a.tab)) == 0 && (a.n_lits == 0 || memcmp(a.lits, b.lits, (size_t)a.n_lits * sizeof(double)) == 0);
}
// The filter of ONE query, as rowsets_plan / rowsets_enqueue / rowsets_direct take it: a set handle; or a conjunction that the call evaluates into
// a TRANSIENT set in its own workspace (where_enqueue places `bits`; `anded`: the words are alive & where already, a candidate bitmap); or
// neither: every row.  What the host cannot know of a transient set — its non-empty tiles, its rows, whether they are fewer than k — the plan
// replaces by "every tile may hold a candidate"; a filter that selects fewer than k rows is decided on the device as for any set.
struct RsFilter {
    const qv_rowset* set = nullptr;
    const WhereSpec* where = nullptr;
    const uint64_t* bits = nullptr;
    bool anded = false;
};
static bool rs_same(const RsFilter& a, const RsFilter& b) { return a.set == b.set && a.where == b.where && a.bits == b.bits; }
static qv::RowSetRef rs_ref(const qv_index* idx, const RsFilter& f) {
    return f.where ? qv::RowSetRef{f.bits, (uint32_t)(((uint64_t)idx->n_rows + 63) / 64), 0} : rowset_ref(f.set);
}

// How a call is cut into device work.  Up to kMaxFusedK results and two or more queries: ONE piece, the multi-query scans with a set
// per query (qv_rowset.hip).  Otherwise runs of consecutive queries naming the same set, each through the paths of qv_index_search
// over the candidate bitmap alive & set, formed on the device (k_rowset_and) — a single query takes the single-launch scans that
// way, longer lists the selection and ranking paths.
// bound: a multi piece of 2 - 8 queries that the filtered bound-scan rule takes (launch_bound_scan_mq with the sets) — decided here, once, so
// that the workspace and the launch agree.  cand_tiles: the tiles that hold a candidate of any query of the piece, as the host knows it: a
// set counts its non-empty words (qv_rowset::tiles; tombstones are not subtracted), a null set every tile, a pass min(n_tiles, the sum).
// Transient sets: a multi piece that holds one reports NO candidate tile to the bfloat16 pass's rule, which its automatic form declines and
// "always" still takes; a single query is planned with every tile a candidate.  Either way a mis-route costs time, never bits.
// bound8: a bound piece that starts on the 8-bit plane (k_bound_scan8_mq<., ., true>) — decided here too.  Its rule is asked with a second
// count in which a transient set is EVERY tile, as the single query is planned: when it says yes the piece is a bound piece, 8-bit first,
// whatever the first count said; with that rule's mode at "bf16" the first question alone decides, as before.
// batched: a multi piece of 9 or more queries that takes the matrix-core filter with a set per query (launch_batched with BatchedSets;
// filtered_batch_takes is the rule) — decided here too, and only for the host forms, whose caller reads the redo flags.
// cand: a run's live candidates (rowset_live), counted for k > kMaxFusedK only — the filtered wide form's rule asks for it; 0 otherwise.
struct RowsetPiece { uint32_t q0, nq, kk; bool multi; bool bound; uint32_t cand_tiles; bool bound8; bool batched = false; uint64_t cand = 0; };
static uint32_t rowsets_cand_tiles(const qv_index* idx, const RsFilter* fl, uint32_t nq, bool transient_every_tile = false) {
    const uint32_t n_tiles = (idx->n_rows + 63) / 64;
    uint64_t sum = 0;
    for (uint32_t q = 0; q < nq; q++) {
        if (fl[q].where && !transient_every_tile) return 0;
        sum += fl[q].set && !fl[q].where ? fl[q].set->tiles : n_tiles;
    }
    return (uint32_t)std::min<uint64_t>(sum, n_tiles);
}
// The filtered batch's rule for one piece.  What the host knows of a query's share of the rows: a null set is every row, a set its
// selected bits against the sparse floor, a where-filter nothing — it counts as dense and the device decides (k_sets_sparse).  Known-sparse
// queries of a piece that goes batched ride along, in place, and come back through the sparse flag.
static uint32_t rowsets_not_sparse(const qv_index* idx, const RsFilter* fl, uint32_t nq) {
    const uint64_t ppm = qv::filtered_batch_ppm(idx->filtered_batch_ppm);
    uint32_t n = 0;
    for (uint32_t q = 0; q < nq; q++)
        n += fl[q].where || !fl[q].set || fl[q].set->selected * 1000000ull >= ppm * (uint64_t)idx->n_rows ? 1u : 0u;
    return n;
}
static bool filtered_batch_takes(const qv_index* idx, uint32_t nq, uint32_t k, const RsFilter* fl) {
    if (nq < qv::kFilteredBatchMinQueries || k > (uint32_t)qv::kMaxFusedK || idx->n_live < 4 * (uint64_t)k) return false;
    if (!qv::filtered_batch_rule(idx->metric, idx->dim, idx->n_rows, nq, k, idx->filter, idx->filtered_batch, rowsets_not_sparse(idx, fl, nq))) return false;
    return qv::batched_sets_supported(idx->view(), nq, k, idx->cus);   // (the route: sample scores from a filter kernel)
}
static size_t rowsets_plan(const qv_index* idx, uint32_t nq, uint32_t k, const RsFilter* fl, std::vector<RowsetPiece>& pieces, bool allow_batched = false) {
    const uint32_t n_tiles = (idx->n_rows + 63) / 64;
    const qv::ScanPlan plan = qv::plan_scan(n_tiles, idx->cus);
    pieces.clear();
    if (allow_batched && filtered_batch_takes(idx, nq, k, fl)) {
        pieces.push_back(RowsetPiece{0, nq, k, true, false, rowsets_cand_tiles(idx, fl, nq), false, true});
        return qv::batched_workspace_bytes(idx->view(), plan, nq, k);
    }
    if (k <= (uint32_t)qv::kMaxFusedK && nq >= 2) {
        const uint32_t ct = rowsets_cand_tiles(idx, fl, nq);
        const qv::IndexView v = idx->view();
        const qv::BoundKnobs knobs = qv::bound_knobs(v);
        const bool bound8 = nq <= 8 && qv::bound_scan_decide(qv::bound_ask(v, nq, k, rowsets_cand_tiles(idx, fl, nq, true)), knobs) == qv::BoundStages::plane8_first;
        const bool bound = bound8 || (nq <= 8 && qv::bound_scan_decide(qv::bound_ask(v, nq, k, ct), knobs) != qv::BoundStages::none);   // (9 or more are not cut into bound passes)
        pieces.push_back(RowsetPiece{0, nq, k, true, bound, ct, bound8});
        return std::max(qv::rowset_workspace_bytes(plan, nq, k, idx->dim4), bound ? qv::bound_scan_mq_workspace_bytes(plan, nq, k, n_tiles, idx->dim) : (size_t)0);
    }
    size_t ws = 0;
    for (uint32_t q = 0; q < nq;) {
        uint32_t e = q + 1;
        while (e < nq && rs_same(fl[e], fl[q])) e++;
        const qv_rowset* set = fl[q].set;
        const bool transient = fl[q].where != nullptr;                // (only with k <= kMaxFusedK: the k > 64 form of qv_index_search_where makes real sets first)
        // (up to kMaxFusedK the lists are k long whatever the set holds: the scans pad, nothing is counted on the host)
        const uint64_t cand = k <= (uint32_t)qv::kMaxFusedK ? 0 : rowset_live(idx, set);
        const uint32_t kk = k <= (uint32_t)qv::kMaxFusedK ? k : (uint32_t)std::min<uint64_t>(k, cand);
        // (a set that selects fewer than kk rows has no threshold: the bound pass would only precede the exact scan that answers — reported
        //  as no candidate tile, which the automatic rule declines; "always" still takes the path)
        const bool too_few = !transient && set && set->selected < kk;
        const uint32_t ct = transient ? n_tiles : (set && !too_few ? std::min<uint32_t>(set->tiles, n_tiles) : 0u);
        pieces.push_back(RowsetPiece{q, e - q, kk, false, false, ct, false, false, cand});
        if (kk) ws = std::max(ws, search_ws_bytes(idx, e - q, kk, k, e - q == 1, set || transient ? ct : qv::kBoundNoFilter, cand));   // (as rowsets_enqueue passes them on)
        q = e;
    }
    return ws;
}

// The conjunctions a call has to evaluate: bytewise-equal ones once.  uniq: the first query of each distinct one; slot[q]: which of
// them query q reads (0xFFFFFFFF: none); lit_base: where each one's literals start when they are staged side by side; args_fit: every
// one's literals fit the kernel arguments, nothing needs staging.
struct WherePlan { std::vector<uint32_t> uniq, slot, lit_base; uint32_t n_lits = 0; bool args_fit = true; };
static void where_plan(const RsFilter* fl, uint32_t nq, WherePlan& wp) {
    wp.slot.assign(nq, 0xFFFFFFFFu);
    std::multimap<uint64_t, uint32_t> seen;                            // hash of table and literals -> slot
    for (uint32_t q = 0; q < nq; q++) {
        const WhereSpec* w = fl[q].where;
        if (!w) continue;
        uint64_t h = 1469598103934665603ull;
        auto mix = [&h](const void* p, size_t n) { const unsigned char* b = static_cast<const unsigned char*>(p); for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull; };
        mix(&w->tab, sizeof(w->tab));
        if (w->n_lits) mix(w->lits, (size_t)w->n_lits * sizeof(double));
        uint32_t u = 0xFFFFFFFFu;
        const auto range = seen.equal_range(h);
        for (auto it = range.first; it != range.second; ++it)
            if (where_same(*fl[wp.uniq[it->second]].where, *w)) { u = it->second; break; }
        if (u == 0xFFFFFFFFu) {
            u = (uint32_t)wp.uniq.size();
            wp.uniq.push_back(q); wp.lit_base.push_back(wp.n_lits);
            wp.n_lits += w->n_lits;
            wp.args_fit = wp.args_fit && w->n_lits <= qv::kWhereArgLits;
            seen.emplace(h, u);
        }
        wp.slot[q] = u;
    }
}
static size_t where_stride_words(const qv_index* idx) { return qv::up256((((size_t)idx->n_rows + 63) / 64) * 8) / 8; }   // a transient set's words, 256-byte aligned
// Enqueue the evaluations on s, in front of the call's scans: launches of up to kWhereMqFilters conjunctions (k_where_mq), conjunction u into
// d_where + u * where_stride_words — or, for a call of ONE query, alive & where straight into d_mask: its candidate bitmap, no k_rowset_and.
// d_lits: the literals staged on the device (wp.lit_base); null: they travel as kernel arguments (wp.args_fit).  Sets fl[q].bits / anded.
static int where_enqueue(qv_index* idx, RsFilter* fl, uint32_t nq, const WherePlan& wp, uint64_t* d_where, uint64_t* d_mask, const double* d_lits, hipStream_t s) {
    const bool lone = nq == 1;
    const size_t stride = where_stride_words(idx);
    for (size_t u0 = 0; u0 < wp.uniq.size(); u0 += qv::kWhereMqFilters) {
        qv::WhereMqArgs a;
        memset(&a, 0, sizeof(a));
        a.n = (uint32_t)std::min<size_t>(qv::kWhereMqFilters, wp.uniq.size() - u0);
        for (uint32_t i = 0; i < a.n; i++) {
            const WhereSpec& w = *fl[wp.uniq[u0 + i]].where;
            a.tab[i] = w.tab;
            a.out[i] = lone ? d_mask : d_where + (u0 + i) * stride;
            if (d_lits) a.lit_base[i] = wp.lit_base[u0 + i];
            else if (w.n_lits) memcpy(a.lits[i], w.lits, (size_t)w.n_lits * sizeof(double));
        }
        hipError_t e = qv::launch_where_mq(a, d_lits, lone ? idx->d_alive : nullptr, idx->n_rows, idx->cus, s);
        if (e != hipSuccess) return fail(QV_ERR_DEVICE, "filter evaluation launch failed: %s", hipGetErrorString(e));
    }
    for (uint32_t q = 0; q < nq; q++)
        if (fl[q].where) { fl[q].bits = lone ? d_mask : d_where + (size_t)wp.slot[q] * stride; fl[q].anded = lone; }
    return QV_OK;
}

// nothing can match (an empty index, a set without a live row): every one of n result slots padded (0xFFFFFFFF, +inf) by a kernel on s
static int pad_lists(uint32_t* d_rows_out, float* d_dist_out, size_t n, hipStream_t s) {
    hipError_t e = qv::launch_rowset_pad(d_rows_out, d_dist_out, n, s);
    if (e != hipSuccess) return fail(QV_ERR_DEVICE, "row-set pad launch failed: %s", hipGetErrorString(e));
    return QV_OK;
}

// enqueue the pieces on s: lists [nq][k], padded past every query's matches.  d_mask: (rows + 63) / 64 words for the candidate bitmaps.
static int rowsets_enqueue(qv_index* idx, const float* d_queries, uint32_t nq, uint32_t k, const RsFilter* fl, const std::vector<RowsetPiece>& pieces,
                           void* ws, uint64_t* d_mask, uint32_t* d_rows_out, float* d_dist_out, hipStream_t s, uint32_t* d_tickets,
                           const qv::RowSetRef* d_sets = nullptr /* a batched piece: the call's table on the device, [nq] */, uint32_t** d_flags_out = nullptr) {
    const qv::IndexView v = idx->view();
    const qv::ScanPlan plan = qv::plan_scan(v.n_tiles, idx->cus);
    for (const RowsetPiece& p : pieces) {
        uint32_t* r_out = d_rows_out + (size_t)p.q0 * k;
        float* d_out = d_dist_out + (size_t)p.q0 * k;
        const float* q = d_queries + (size_t)p.q0 * idx->dim;
        if (p.batched) {                                              // sample bound over the sets, the filter, the exact re-score: one corpus pass for the piece
            if (!d_sets || !d_flags_out) return fail(QV_ERR_DEVICE, "filtered batch without its set table");
            const ProfilePair pp = profile_begin(idx);
            const qv::BatchedSets bs{d_sets + p.q0, qv::filtered_batch_ppm(idx->filtered_batch_ppm)};
            hipError_t e = qv::launch_batched(v, plan, q, p.nq, k, ws, r_out, d_out, d_flags_out, idx->cus, s, pp.ev0, pp.ev1, &bs);
            profile_end(idx, pp, e == hipSuccess);
            if (e != hipSuccess) return fail(QV_ERR_DEVICE, "filtered batch launch failed: %s", hipGetErrorString(e));
            continue;
        }
        if (p.multi) {
            std::vector<qv::RowSetRef> refs(p.nq);
            for (uint32_t i = 0; i < p.nq; i++) refs[i] = rs_ref(idx, fl[p.q0 + i]);
            // the pass on the reduced copies (p.bound8: the 8-bit plane first), each query over its own candidates: its launcher takes no events
            const bool bound = p.bound && d_tickets;
            const ProfilePair pp = profile_begin(idx, bound, s);
            hipError_t e = bound ? qv::launch_bound_scan_mq(v, plan, q, p.nq, k, ws, d_tickets + qv::kBoundCtrlWord, idx->d_bound_stats, r_out, d_out, s, refs.data(), p.bound8)
                                 : qv::launch_rowset_topk(v, plan, q, p.nq, k, refs.data(), ws, r_out, d_out, s, pp.ev0, pp.ev1);
            profile_end(idx, pp, e == hipSuccess, bound, s);
            if (e != hipSuccess) return fail(QV_ERR_DEVICE, "row-set scan launch failed: %s", hipGetErrorString(e));
            continue;
        }
        if (p.kk == 0) {
            const int rc = pad_lists(r_out, d_out, (size_t)p.nq * k, s);
            if (rc != QV_OK) return rc;
            continue;
        }
        const RsFilter& f = fl[p.q0];
        const uint64_t* cand = nullptr;
        if (f.where && f.anded) cand = f.bits;                        // (where_enqueue wrote alive & where there)
        else if (f.set || f.where) {
            hipError_t e = qv::launch_rowset_and(v, rs_ref(idx, f), d_mask, s);
            if (e != hipSuccess) return fail(QV_ERR_DEVICE, "row-set bitmap launch failed: %s", hipGetErrorString(e));
            cand = d_mask;
        }
        SearchExtras x;
        x.d_candidates = cand; x.candidate_tiles = p.cand_tiles; x.candidates = p.cand; x.d_tickets = p.nq == 1 ? d_tickets : nullptr;
        const int rc = enqueue_search(idx, q, p.nq, p.kk, k, ws, r_out, d_out, s, x);
        if (rc != QV_OK) return rc;
    }
    return QV_OK;
}

static int rowsets_check(const qv_index* idx, uint32_t nq, const qv_rowset* const* sets) {
    if (!sets) return fail(QV_ERR_INVALID_ARG, "sets is null");
    for (uint32_t q = 0; q < nq; q++)
        if (sets[q] && sets[q]->idx != idx) return fail(QV_ERR_INVALID_ARG, "row set of query %u belongs to another index", q);
    return QV_OK;
}

// one pass of rowsets_direct: up to kHostBatch queries in a context of the call's own, the arguments checked
static int rowsets_pass(qv_index* idx, const float* queries, uint32_t nq, uint32_t k, const RsFilter* fl_in,
                        uint32_t* rows_out, float* dist_out, uint32_t* count_out) {
    HIPCHK(hipSetDevice(idx->device));
    // a filtered batch with a short remainder (short_tail): the remainder as a pass of its own, as qv_index_search_batched cuts it; each
    // part decides its route for itself — and takes its context for itself, which is why this pass has none yet
    if (filtered_batch_takes(idx, nq, k, fl_in)) {
        if (const uint32_t tail = short_tail(nq)) {
            const uint32_t head = nq - tail;
            const int rc0 = rowsets_pass(idx, queries, head, k, fl_in, rows_out, dist_out, count_out);
            if (rc0 != QV_OK) return rc0;
            return rowsets_pass(idx, queries + (size_t)head * idx->dim, tail, k, fl_in + head, rows_out + (size_t)head * k, dist_out + (size_t)head * k, count_out + head);
        }
    }
    std::vector<RsFilter> fl(fl_in, fl_in + nq);                      // (the transient sets' words are placed below)
    std::vector<RowsetPiece> pieces;
    const size_t ws_bytes = rowsets_plan(idx, nq, k, fl.data(), pieces, true);
    const bool batched = pieces.size() == 1 && pieces[0].batched;
    bool any = false;
    for (const RowsetPiece& p : pieces) any = any || p.kk != 0;
    if (!any) {                                                       // no set holds a live row: nothing to run
        for (size_t i = 0; i < (size_t)nq * k; i++) { rows_out[i] = 0xFFFFFFFFu; dist_out[i] = __builtin_inff(); }
        for (uint32_t q = 0; q < nq; q++) count_out[q] = 0;
        return QV_OK;
    }
    HostCall hc(idx);
    int rc = hc.acquire();
    if (rc != QV_OK) return rc;
    SearchCtx* c = hc.c;
    const size_t words = ((size_t)idx->n_rows + 63) / 64;
    uint32_t* tickets = nullptr;
    if ((rc = c->d_mask.ensure(words * 8)) || (rc = hc.reserve(nq, nq, k)) || (rc = hc.workspace(ws_bytes)) || (rc = hc.tickets(&tickets))) return rc;
    uint64_t* d_mask = static_cast<uint64_t*>(c->d_mask.p);
    hc.stage(queries, nq);
    if ((rc = hc.send(nq))) return rc;
    WherePlan wp;
    where_plan(fl.data(), nq, wp);
    if (!wp.uniq.empty()) {                                           // the call's transient sets, in the context's own buffers, on its stream
        if (nq > 1 && (rc = c->d_where.ensure(wp.uniq.size() * where_stride_words(idx) * 8))) return rc;
        const double* d_lits = nullptr;
        if (!wp.args_fit) {                                           // a long IN list: the literals side by side through the pinned buffer
            const size_t lbytes = (size_t)wp.n_lits * sizeof(double);
            if ((rc = c->h_lits.ensure(lbytes)) || (rc = c->d_lits.ensure(lbytes))) return rc;
            for (size_t u = 0; u < wp.uniq.size(); u++) {
                const WhereSpec& w = *fl[wp.uniq[u]].where;
                if (w.n_lits) memcpy(static_cast<double*>(c->h_lits.p) + wp.lit_base[u], w.lits, (size_t)w.n_lits * sizeof(double));
            }
            HIPCHK(hipMemcpyAsync(c->d_lits.p, c->h_lits.p, lbytes, hipMemcpyHostToDevice, c->stream));
            d_lits = static_cast<const double*>(c->d_lits.p);
        }
        if ((rc = where_enqueue(idx, fl.data(), nq, wp, static_cast<uint64_t*>(c->d_where.p), d_mask, d_lits, c->stream))) return rc;
    }
    const size_t fbytes = 2 * (size_t)nq * sizeof(uint32_t);           // a batched piece: its redo flags, then its sparse flags
    uint32_t* d_flags = nullptr;
    if (batched) {                                                    // the sets' table: pinned memory -> the context's device array, on the call's stream
        const size_t sbytes = (size_t)nq * sizeof(qv::RowSetRef);
        if ((rc = c->h_sets.ensure(sbytes)) || (rc = c->d_sets.ensure(sbytes)) || (rc = c->h_ids.ensure(fbytes))) return rc;
        qv::RowSetRef* refs = static_cast<qv::RowSetRef*>(c->h_sets.p);
        for (uint32_t q = 0; q < nq; q++) refs[q] = rs_ref(idx, fl[q]);
        HIPCHK(hipMemcpyAsync(c->d_sets.p, c->h_sets.p, sbytes, hipMemcpyHostToDevice, c->stream));
    }
    rc = rowsets_enqueue(idx, hc.d_queries(), nq, k, fl.data(), pieces, hc.ws(), d_mask, hc.d_rows(), hc.d_dist(), hc.stream(), tickets,
                         batched ? static_cast<const qv::RowSetRef*>(c->d_sets.p) : nullptr, batched ? &d_flags : nullptr);
    if (rc != QV_OK || (rc = hc.fetch(nq, k))) return rc;
    if (batched) HIPCHK(hipMemcpyAsync(c->h_ids.p, d_flags, fbytes, hipMemcpyDeviceToHost, c->stream));
    if ((rc = hc.sync())) return rc;
    hc.deliver(nq, k, k, k, rows_out, dist_out);
    if (batched) {
        // The queries the batch handed back — more candidates than slots, a guessed bound that failed its check, a sparse set — through the
        // exact row-set pieces, with their filters, in this context: the transient where-words are still in d_where.
        const uint32_t* flags = static_cast<const uint32_t*>(c->h_ids.p);
        std::vector<uint32_t> redo;
        uint64_t n_sparse = 0;
        for (uint32_t q = 0; q < nq; q++) {
            // (k_sets_sparse flags a sparse query in both arrays: the redo flags alone say which answers are not final, also to the kernels
            // behind the filter — a sparse flag without its redo flag is a broken batch, not something to paper over here)
            if (flags[nq + q] && !flags[q]) return fail(QV_ERR_DEVICE, "filtered batch: query %u is flagged sparse but not for the redo", q);
            if (flags[q]) { redo.push_back(q); n_sparse += flags[nq + q] ? 1 : 0; }
        }
        idx->fb_stats[0] += nq; idx->fb_stats[1] += redo.size() - n_sparse; idx->fb_stats[2] += n_sparse; idx->fb_stats[3] += 1;
        if (!redo.empty()) {
            const uint32_t nr = (uint32_t)redo.size();
            std::vector<RsFilter> rfl(nr);
            for (uint32_t i = 0; i < nr; i++) rfl[i] = fl[redo[i]];
            std::vector<RowsetPiece> rpieces;
            const size_t rws = rowsets_plan(idx, nr, k, rfl.data(), rpieces);
            hc.stage_gather(queries, redo);
            if ((rc = hc.workspace(rws)) || (rc = hc.send(nr))) return rc;
            rc = rowsets_enqueue(idx, hc.d_queries(), nr, k, rfl.data(), rpieces, hc.ws(), d_mask, hc.d_rows(), hc.d_dist(), hc.stream(), tickets);
            if (rc != QV_OK || (rc = hc.fetch(nr, k)) || (rc = hc.sync())) return rc;
            hc.deliver(nr, k, k, k, rows_out, dist_out, redo.data());
        }
    }
    for (uint32_t q = 0; q < nq; q++) {                               // a list's results end where its padding begins (no row is 0xFFFFFFFF)
        uint32_t n = 0;
        while (n < k && rows_out[(size_t)q * k + n] != 0xFFFFFFFFu) n++;
        for (uint32_t i = n; i < k; i++) { rows_out[(size_t)q * k + i] = 0xFFFFFFFFu; dist_out[(size_t)q * k + i] = __builtin_inff(); }
        count_out[q] = n;
    }
    return QV_OK;
}

// one call's worth of queries.  idx, queries, count_out, fl: checked by the entry points (each in its own order), the filters valid;
// from the empty index on the order is one.
static int rowsets_direct(qv_index* idx, const float* queries, uint32_t nq, uint32_t k, const RsFilter* fl,
                          uint32_t* rows_out, float* dist_out, uint32_t* count_out) {
    bool done;
    if (const int rc = check_host_outputs(idx, nq, k, rows_out && dist_out, "rows_out/dist_out is null", count_out, &done); rc != QV_OK || done) return rc;
    return in_passes(nq, kHostBatch, [&](uint32_t q0, uint32_t m) {
        return rowsets_pass(idx, queries + (size_t)q0 * idx->dim, m, k, fl + q0, rows_out + (size_t)q0 * k, dist_out + (size_t)q0 * k, count_out + q0);
    });
}

// qv_index_search_rowsets' own checks, in its order — the sets in front of the empty index — in front of rowsets_direct
static int rowsets_direct_sets(qv_index* idx, const float* queries, uint32_t nq, uint32_t k, const qv_rowset* const* sets,
                               uint32_t* rows_out, float* dist_out, uint32_t* count_out) {
    bool done;
    if (const int rc = check_host_inputs(idx, nq, queries && count_out && sets, "queries/sets/count_out is null", &done); rc != QV_OK || done) return rc;
    { const int rc0 = rowsets_check(idx, nq, sets); if (rc0 != QV_OK) return rc0; }
    std::vector<RsFilter> fl(nq);
    for (uint32_t q = 0; q < nq; q++) fl[q].set = sets[q];
    return rowsets_direct(idx, queries, nq, k, fl.data(), rows_out, dist_out, count_out);
}

// Callers that may share a pass (coalesce_applies holds, every filter is valid): through the ONE front of the filtered searches, whichever
// kind of filter they carry — a member's tag is its array of nq RsFilter, valid until its call returns.  The leader runs the group as one
// call: its conjunctions are evaluated together in front of the pass (where_enqueue), its handles read as they are.
static int rowsets_submit(qv_index* idx, const float* queries, uint32_t nq, uint32_t k, const RsFilter* fl,
                          uint32_t* rows_out, float* dist_out, uint32_t* count_out) {
    return front_submit(idx, idx->front_rs, queries, nq, k, rows_out, dist_out, count_out, fl,
                        [&] { return rowsets_direct(idx, queries, nq, k, fl, rows_out, dist_out, count_out); },
                        [&](qvco::Group& g) {
                            std::vector<RsFilter> all(g.nq);          // the members' filters side by side, in the order of the group's query block
                            for (uint32_t mi = 0; mi < g.n_mem; mi++) {
                                const qvco::Member& m = g.mbuf[mi];
                                const RsFilter* mf = static_cast<const RsFilter*>(m.tag);
                                for (uint32_t i = 0; i < m.nq; i++) all[m.q0 + i] = mf[i];
                            }
                            return rowsets_direct(idx, g.queries(), g.nq, g.kmax, all.data(), g.rows.data(), g.dist.data(), g.count.data());
                        });
}

int qv_index_search_rowsets(qv_index* idx, const float* queries, uint32_t nq, uint32_t k, const qv_rowset* const* sets,
                            uint32_t* rows_out, float* dist_out, uint32_t* count_out) {
    // callers that may share a pass: qv_index_search's rule, with a valid set per query on top (a request that fails a check runs
    // on its own and reports its error in the usual order)
    if (!coalesce_applies(idx, queries, nq, k, rows_out, dist_out, count_out) || !sets || rowsets_check(idx, nq, sets) != QV_OK)
        return rowsets_direct_sets(idx, queries, nq, k, sets, rows_out, dist_out, count_out);
    RsFilter fl[kCoalesceMaxNq];
    for (uint32_t q = 0; q < nq; q++) fl[q].set = sets[q];
    return rowsets_submit(idx, queries, nq, k, fl, rows_out, dist_out, count_out);
}

int qv_index_rowset_coalesce_stats(qv_index* idx, uint64_t out[8]) {
    if (!idx || !out) return fail(QV_ERR_INVALID_ARG, "index/out is null");
    idx->front_rs.stats.read(out);
    return QV_OK;
}

// The buffer of a device-pointer row-set or where search: the passes' workspace (rowsets_plan), the call's candidate bitmap behind it and,
// behind that, a where search's transient sets (one per distinct filter, none for a lone query: its filter goes straight into the bitmap) —
// every region on a 256-byte boundary.  mask_bytes: the bitmap's words as the call reserves them (a where search: one set's stride).
struct FilteredCallLayout { void* ws; uint64_t *d_mask, *d_where; size_t end, total; };
static FilteredCallLayout filtered_call_layout(void* base, size_t plan_bytes, size_t mask_bytes, size_t n_where, size_t where_stride_bytes, qv::WsLog* log = nullptr) {
    qv::WsCarver w{static_cast<char*>(base), 0, 0, log};
    FilteredCallLayout L{};
    L.ws = w.take256<char>(plan_bytes);
    L.d_mask = w.take<uint64_t>(mask_bytes / 8);
    if (n_where) L.d_where = w.take<uint64_t>(n_where * where_stride_bytes / 8);
    return w.finish(L);
}

int qv_index_search_rowsets_device(qv_index* idx, const float* d_queries, uint32_t nq, uint32_t k, const qv_rowset* const* sets,
                                   uint32_t* d_rows_out, float* d_dist_out, void* stream) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (nq == 0) return QV_OK;
    if (!d_queries || !d_rows_out || !d_dist_out) return fail(QV_ERR_INVALID_ARG, "null device pointer");
    { const int rc0 = rowsets_check(idx, nq, sets); if (rc0 != QV_OK) return rc0; }
    if (k == 0) return fail(QV_ERR_K_NOT_POSITIVE, "k must be positive");
    HIPCHK(hipSetDevice(idx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (idx->n_live == 0 || idx->n_rows == 0) return pad_lists(d_rows_out, d_dist_out, (size_t)nq * k, s);
    return in_passes(nq, kHostBatch, [&](uint32_t q0, uint32_t m) {   // bound the workspace, as the host-pointer form does
        std::vector<RsFilter> fl(m);
        for (uint32_t q = 0; q < m; q++) fl[q].set = sets[q0 + q];
        std::vector<RowsetPiece> pieces;
        const size_t plan_bytes = rowsets_plan(idx, m, k, fl.data(), pieces);
        const size_t words = ((size_t)idx->n_rows + 63) / 64;
        void* ws = nullptr;
        std::unique_lock<std::mutex> ws_hold;
        uint32_t* tickets = nullptr;
        const int rc = stream_workspace(idx, s, filtered_call_layout(nullptr, plan_bytes, words * 8, 0, 0).total, &ws, &ws_hold, &tickets);
        if (rc != QV_OK) return rc;
        const FilteredCallLayout L = filtered_call_layout(ws, plan_bytes, words * 8, 0, 0);
        return rowsets_enqueue(idx, d_queries + (size_t)q0 * idx->dim, m, k, fl.data(), pieces, L.ws, L.d_mask,
                               d_rows_out + (size_t)q0 * k, d_dist_out + (size_t)q0 * k, s, tickets);
    });
}

// ---------------------------------------------------------------- filtered search by predicate: the sets live in the call's workspace --
// filters[q] checked by qv_rowset_create_where's own function; n_preds == 0: every row.  The message names the query.
static int where_spec(const qv_index* idx, const qv_where& w, uint32_t q, WhereSpec& out) {
    memset(&out, 0, sizeof(out));
    if (w.n_preds == 0) return QV_OK;
    const int rc = where_check(idx, w.cols, w.ops, w.literals, w.lit_off, w.n_preds, out.tab);
    if (rc != QV_OK) {
        char msg[400];
        snprintf(msg, sizeof(msg), "%s", qv_last_error());
        return fail(rc, "filter of query %u: %s", q, msg);
    }
    out.lits = w.literals; out.n_lits = w.lit_off[w.n_preds];
    return QV_OK;
}

// k > 64: runs of consecutive queries with bytewise-equal filters as a temporary REAL set each (the existing internals: an allocation, the
// null stream, the mirror — the selection and ranking paths clamp their list lengths to counts only the host mirror has), then the set
// paths of qv_index_search_rowsets; the sets are freed before return
static int where_wide(qv_index* idx, const float* queries, uint32_t nq, uint32_t k, const WhereSpec* specs,
                      uint32_t* rows_out, float* dist_out, uint32_t* count_out) {
    std::vector<qv_rowset*> made;
    std::vector<RsFilter> fl(nq);
    int rc = QV_OK;
    for (uint32_t q = 0; q < nq && rc == QV_OK;) {
        uint32_t e = q + 1;
        while (e < nq && where_same(specs[e], specs[q])) e++;
        if (specs[q].tab.n) {
            qv_rowset* rs = nullptr;
            rc = rowset_from_where(idx, specs[q].tab, specs[q].lits, specs[q].n_lits, &rs);
            if (rc == QV_OK) { made.push_back(rs); for (uint32_t i = q; i < e; i++) fl[i].set = rs; }
        }
        q = e;
    }
    if (rc == QV_OK) rc = rowsets_direct(idx, queries, nq, k, fl.data(), rows_out, dist_out, count_out);
    char msg[400];
    if (rc != QV_OK) snprintf(msg, sizeof(msg), "%s", qv_last_error());
    for (qv_rowset* rs : made) qv_rowset_destroy(rs);
    return rc == QV_OK ? QV_OK : fail(rc, "%s", msg);
}

int qv_index_search_where(qv_index* idx, const float* queries, uint32_t nq, uint32_t k, const qv_where* filters,
                          uint32_t* rows_out, float* dist_out, uint32_t* count_out) {
    bool done;                                                        // (the filters are checked behind k and the outputs)
    if (const int rc = check_host_args(idx, nq, k, queries && count_out && filters, "queries/filters/count_out is null", rows_out && dist_out, "rows_out/dist_out is null", count_out, &done);
        rc != QV_OK || done)
        return rc;
    WhereSpec small_specs[kCoalesceMaxNq];                            // (a single-query caller allocates nothing)
    RsFilter small_fl[kCoalesceMaxNq];
    std::vector<WhereSpec> big_specs;
    std::vector<RsFilter> big_fl;
    WhereSpec* specs = small_specs; RsFilter* fl = small_fl;
    if (nq > kCoalesceMaxNq) { big_specs.resize(nq); big_fl.resize(nq); specs = big_specs.data(); fl = big_fl.data(); }
    for (uint32_t q = 0; q < nq; q++) {
        const int rc0 = where_spec(idx, filters[q], q, specs[q]);
        if (rc0 != QV_OK) return rc0;
    }
    if (k > (uint32_t)qv::kMaxFusedK) return where_wide(idx, queries, nq, k, specs, rows_out, dist_out, count_out);
    for (uint32_t q = 0; q < nq; q++) fl[q].where = specs[q].tab.n ? &specs[q] : nullptr;
    if (!coalesce_applies(idx, queries, nq, k, rows_out, dist_out, count_out)) return rowsets_direct(idx, queries, nq, k, fl, rows_out, dist_out, count_out);
    return rowsets_submit(idx, queries, nq, k, fl, rows_out, dist_out, count_out);
}

int qv_index_search_where_device(qv_index* idx, const float* d_queries, uint32_t nq, uint32_t k, const qv_where* filters,
                                 uint32_t* d_rows_out, float* d_dist_out, void* stream) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (nq == 0) return QV_OK;
    if (!d_queries || !d_rows_out || !d_dist_out) return fail(QV_ERR_INVALID_ARG, "null device pointer");
    if (!filters) return fail(QV_ERR_INVALID_ARG, "filters is null");
    if (k == 0) return fail(QV_ERR_K_NOT_POSITIVE, "k must be positive");
    if (k > (uint32_t)qv::kMaxFusedK)
        return fail(QV_ERR_UNSUPPORTED, "the device-pointer form takes k <= %d (longer lists need a set's host mirror): got %u", qv::kMaxFusedK, k);
    std::vector<WhereSpec> specs(nq);
    for (uint32_t q = 0; q < nq; q++) {
        const int rc0 = where_spec(idx, filters[q], q, specs[q]);
        if (rc0 != QV_OK) return rc0;
    }
    // the literals travel as kernel arguments: a staging buffer would be overwritten by the stream's next call while this one is still enqueued
    for (uint32_t q = 0; q < nq; q++)
        if (specs[q].n_lits > qv::kWhereArgLits)
            return fail(QV_ERR_UNSUPPORTED, "filter of query %u carries %u literals: the device-pointer form takes up to %u per filter", q, specs[q].n_lits, qv::kWhereArgLits);
    HIPCHK(hipSetDevice(idx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (idx->n_live == 0 || idx->n_rows == 0) return pad_lists(d_rows_out, d_dist_out, (size_t)nq * k, s);
    const size_t stride = where_stride_words(idx) * 8;                // the candidate bitmap, and each transient set behind it: 256-byte aligned
    return in_passes(nq, kHostBatch, [&](uint32_t q0, uint32_t m) {
        std::vector<RsFilter> fl(m);
        for (uint32_t q = 0; q < m; q++) fl[q].where = specs[q0 + q].tab.n ? &specs[q0 + q] : nullptr;
        std::vector<RowsetPiece> pieces;
        const size_t plan_bytes = rowsets_plan(idx, m, k, fl.data(), pieces);
        WherePlan wp;
        where_plan(fl.data(), m, wp);
        const size_t n_where = m > 1 ? wp.uniq.size() : 0;
        void* ws = nullptr;
        std::unique_lock<std::mutex> ws_hold;
        uint32_t* tickets = nullptr;
        int rc = stream_workspace(idx, s, filtered_call_layout(nullptr, plan_bytes, stride, n_where, stride).total, &ws, &ws_hold, &tickets);
        if (rc != QV_OK) return rc;
        const FilteredCallLayout L = filtered_call_layout(ws, plan_bytes, stride, n_where, stride);
        if ((rc = where_enqueue(idx, fl.data(), m, wp, L.d_where, L.d_mask, nullptr, s))) return rc;
        return rowsets_enqueue(idx, d_queries + (size_t)q0 * idx->dim, m, k, fl.data(), pieces, L.ws, L.d_mask,
                               d_rows_out + (size_t)q0 * k, d_dist_out + (size_t)q0 * k, s, tickets);
    });
}

int qv_index_search_device(qv_index* idx, const float* d_queries, uint32_t nq, uint32_t k,
                           uint32_t* d_rows_out, float* d_dist_out, void* stream) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (nq == 0) return QV_OK;
    if (!d_queries || !d_rows_out || !d_dist_out) return fail(QV_ERR_INVALID_ARG, "null device pointer");
    if (k == 0) return fail(QV_ERR_K_NOT_POSITIVE, "k must be positive");
    HIPCHK(hipSetDevice(idx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (idx->n_live == 0) return pad_lists(d_rows_out, d_dist_out, (size_t)nq * k, s);   // no results
    const uint32_t kk = std::min(k, idx->n_live);
    void* ws = nullptr;
    std::unique_lock<std::mutex> ws_hold;
    SearchExtras x;
    int rc = stream_workspace(idx, s, search_ws_bytes(idx, nq, kk, k, true), &ws, &ws_hold, &x.d_tickets);
    if (rc != QV_OK) return rc;
    return enqueue_search(idx, d_queries, nq, kk, k, ws, d_rows_out, d_dist_out, s, x);
}

// the short tail of an unfiltered batch: one the exact scan's shared pass takes (up to 8 queries) or the filter itself
static uint32_t batched_tail(const qv::IndexView& v, uint32_t nq, uint32_t k) {
    const uint32_t rem = short_tail(nq);
    return rem && (rem <= 8 || qv::batched_supported(v, rem, k)) ? rem : 0;
}

// m queries of a larger device batch, from query q0, as a call of their own: by the filter where it takes that many, else by the exact
// scan with their flags cleared
static int batched_device_part(qv_index* idx, const float* d_queries, uint32_t q0, uint32_t m, uint32_t k,
                               uint32_t* d_rows_out, float* d_dist_out, uint32_t* d_redo_flags_out, void* stream) {
    const float* q = d_queries + (size_t)q0 * idx->dim;
    if (qv::batched_supported(idx->view(), m, k))
        return qv_index_search_batched_device(idx, q, m, k, d_rows_out + (size_t)q0 * k, d_dist_out + (size_t)q0 * k, d_redo_flags_out + q0, stream);
    HIPCHK(hipMemsetAsync(d_redo_flags_out + q0, 0, (size_t)m * sizeof(uint32_t), static_cast<hipStream_t>(stream)));
    return qv_index_search_device(idx, q, m, k, d_rows_out + (size_t)q0 * k, d_dist_out + (size_t)q0 * k, stream);
}

// one pass of qv_index_search_batched_device: up to kHostBatch queries that the filter takes
static int batched_device_pass(qv_index* idx, const float* d_queries, uint32_t nq, uint32_t k,
                               uint32_t* d_rows_out, float* d_dist_out, uint32_t* d_redo_flags_out, void* stream) {
    const qv::IndexView v = idx->view();
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const uint32_t tail = batched_tail(v, nq, k)) {
        const int rc0 = qv_index_search_batched_device(idx, d_queries, nq - tail, k, d_rows_out, d_dist_out, d_redo_flags_out, stream);
        if (rc0 != QV_OK) return rc0;
        return batched_device_part(idx, d_queries, nq - tail, tail, k, d_rows_out, d_dist_out, d_redo_flags_out, stream);
    }
    const qv::ScanPlan plan = qv::plan_scan(v.n_tiles, idx->cus);
    void* ws = nullptr;
    std::unique_lock<std::mutex> ws_hold;
    int rc = stream_workspace(idx, s, qv::batched_workspace_bytes(v, plan, nq, k), &ws, &ws_hold);
    if (rc != QV_OK) return rc;
    const ProfilePair pp = profile_begin(idx);
    uint32_t* d_ovf = nullptr;
    hipError_t e = qv::launch_batched(v, plan, d_queries, nq, k, ws, d_rows_out, d_dist_out, &d_ovf, idx->cus, s, pp.ev0, pp.ev1);
    profile_end(idx, pp, e == hipSuccess);
    if (e != hipSuccess) return fail(QV_ERR_DEVICE, "batched launch failed: %s", hipGetErrorString(e));
    HIPCHK(hipMemcpyAsync(d_redo_flags_out, d_ovf, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    return QV_OK;
}

int qv_index_search_batched_device(qv_index* idx, const float* d_queries, uint32_t nq, uint32_t k,
                                   uint32_t* d_rows_out, float* d_dist_out, uint32_t* d_redo_flags_out, void* stream) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (nq == 0) return QV_OK;
    if (!d_queries || !d_rows_out || !d_dist_out || !d_redo_flags_out) return fail(QV_ERR_INVALID_ARG, "null device pointer");
    if (k == 0) return fail(QV_ERR_K_NOT_POSITIVE, "k must be positive");
    if (k > idx->n_live || idx->n_live < 4 * (uint64_t)k || !qv::batched_supported(idx->view(), nq, k))
        return fail(QV_ERR_UNSUPPORTED, "the MFMA batched path does not apply to this index/query shape; use qv_index_search_device");
    HIPCHK(hipSetDevice(idx->device));
    // bound the workspace (sample scores + candidate slots: ~160 KB per query): the one pass of a call that fits, else every slice as a call of its own
    return in_passes(nq, kHostBatch, [&](uint32_t q0, uint32_t m) {
        return m == nq ? batched_device_pass(idx, d_queries, nq, k, d_rows_out, d_dist_out, d_redo_flags_out, stream)
                       : batched_device_part(idx, d_queries, q0, m, k, d_rows_out, d_dist_out, d_redo_flags_out, stream);
    });
}

// one pass of qv_index_search_batched: up to kHostBatch queries, the arguments checked
static int batched_pass(qv_index* idx, const float* queries, uint32_t nq, uint32_t k, uint32_t* rows_out, float* dist_out, uint32_t* count_out) {
    const uint32_t kk = std::min(k, idx->n_live);
    const qv::IndexView v = idx->view();
    // the MFMA filter pays off for many queries over a large cosine/dot corpus; everything else
    // (and any k > 64) takes the exact multi-query scan, which returns the same result
    if (!qv::batched_supported(v, nq, kk) || kk != k || idx->n_live < 4 * kk)
        return exact_search_host(idx, queries, nq, k, rows_out, dist_out, count_out);
    if (const uint32_t tail = batched_tail(v, nq, kk)) {              // (each part falls back to the exact scan by itself)
        const uint32_t head = nq - tail;
        const int rc0 = batched_pass(idx, queries, head, k, rows_out, dist_out, count_out);
        if (rc0 != QV_OK) return rc0;
        return batched_pass(idx, queries + (size_t)head * idx->dim, tail, k, rows_out + (size_t)head * k, dist_out + (size_t)head * k, count_out + head);
    }
    std::vector<uint32_t> redo;
    {
        HostCall hc(idx);                                             // (gone before the redo: the exact scan takes its own context, a call never holds two)
        const qv::ScanPlan plan = qv::plan_scan(v.n_tiles, idx->cus);
        const size_t fbytes = (size_t)nq * sizeof(uint32_t);
        int rc;
        if ((rc = hc.open()) || (rc = hc.reserve(nq, nq, kk)) || (rc = hc.c->h_ids.ensure(fbytes)) || (rc = hc.workspace(qv::batched_workspace_bytes(v, plan, nq, kk)))) return rc;
        hc.stage(queries, nq);
        if ((rc = hc.send(nq))) return rc;
        uint32_t* d_ovf = nullptr;
        const ProfilePair pp = profile_begin(idx);
        hipError_t e = qv::launch_batched(v, plan, hc.d_queries(), nq, kk, hc.ws(), hc.d_rows(), hc.d_dist(), &d_ovf, idx->cus, hc.stream(), pp.ev0, pp.ev1);
        profile_end(idx, pp, e == hipSuccess);
        if (e != hipSuccess) return fail(QV_ERR_DEVICE, "batched launch failed: %s", hipGetErrorString(e));
        if ((rc = hc.fetch(nq, kk))) return rc;
        HIPCHK(hipMemcpyAsync(hc.c->h_ids.p, d_ovf, fbytes, hipMemcpyDeviceToHost, hc.stream()));
        if ((rc = hc.sync())) return rc;
        hc.deliver(nq, kk, kk, k, rows_out, dist_out);
        for (uint32_t q = 0; q < nq; q++) count_out[q] = kk;
        // queries whose candidate buffer overflowed (loose sample bound, e.g. a corpus sorted by cluster):
        // redo them with the exact scan
        const uint32_t* ovf = static_cast<const uint32_t*>(hc.c->h_ids.p);
        for (uint32_t q = 0; q < nq; q++) if (ovf[q]) redo.push_back(q);
        idx->batched_redo += redo.size();
    }
    if (!redo.empty()) {
        const uint32_t nr = (uint32_t)redo.size();
        std::vector<float> rq((size_t)nr * idx->dim), rd((size_t)nr * kk);
        std::vector<uint32_t> rr((size_t)nr * kk), rc2(nr);
        gather_queries(rq.data(), queries, redo, idx->dim);
        const int rc = exact_search_host(idx, rq.data(), nr, kk, rr.data(), rd.data(), rc2.data());
        if (rc != QV_OK) return rc;
        deliver_lists(rr.data(), rd.data(), nr, kk, kk, k, rows_out, dist_out, redo.data());
    }
    return QV_OK;
}

int qv_index_search_batched(qv_index* idx, const float* queries, uint32_t nq, uint32_t k,
                            uint32_t* rows_out, float* dist_out, uint32_t* count_out) {
    bool done;
    if (const int rc = check_host_args(idx, nq, k, queries && count_out, "queries/count_out is null", rows_out && dist_out, "rows_out/dist_out is null", count_out, &done); rc != QV_OK || done)
        return rc;
    return in_passes(nq, kHostBatch, [&](uint32_t q0, uint32_t m) {   // (each pass decides for itself whether the filter takes it)
        return batched_pass(idx, queries + (size_t)q0 * idx->dim, m, k, rows_out + (size_t)q0 * k, dist_out + (size_t)q0 * k, count_out + q0);
    });
}

int qv_merge_topk_device(const float* d_dist_lists, const uint32_t* d_row_lists, uint32_t n_lists, uint32_t k,
                         uint32_t* d_rows_out, float* d_dist_out, void* stream) {
    if (!d_dist_lists || !d_row_lists || !d_rows_out || !d_dist_out) return fail(QV_ERR_INVALID_ARG, "null device pointer");
    if (k == 0) return fail(QV_ERR_K_NOT_POSITIVE, "k must be positive");
    if (k > (uint32_t)qv::kMaxFusedK || n_lists == 0 || (uint64_t)n_lists * k > 65536) return fail(QV_ERR_UNSUPPORTED, "merge supports k <= %d and n_lists*k <= 65536", qv::kMaxFusedK);
    hipError_t e = qv::launch_merge_pairs(d_dist_lists, d_row_lists, n_lists, k, d_rows_out, d_dist_out, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(QV_ERR_DEVICE, "merge launch failed: %s", hipGetErrorString(e));
    return QV_OK;
}

int qv_merge_topk_shards_device(const uint32_t* d_packed_lists, const uint32_t* d_bases, uint32_t n_lists, uint32_t nq, uint32_t k,
                                uint32_t* d_rows_out, float* d_dist_out, void* stream) {
    if (!d_packed_lists || !d_bases || !d_rows_out || !d_dist_out) return fail(QV_ERR_INVALID_ARG, "null device pointer");
    if (nq == 0) return QV_OK;
    if (k == 0) return fail(QV_ERR_K_NOT_POSITIVE, "k must be positive");
    if (k > (uint32_t)qv::kMaxFusedK || n_lists == 0 || (uint64_t)n_lists * k > 65536) return fail(QV_ERR_UNSUPPORTED, "merge supports k <= %d and n_lists*k <= 65536", qv::kMaxFusedK);
    hipError_t e = qv::launch_merge_shards(d_packed_lists, d_bases, n_lists, nq, k, d_rows_out, d_dist_out, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(QV_ERR_DEVICE, "merge launch failed: %s", hipGetErrorString(e));
    return QV_OK;
}

int qv_index_set_filter(qv_index* idx, int filter) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (filter < 0 || filter > QV_FILTER_OFF) return fail(QV_ERR_INVALID_ARG, "filter must be 0 (automatic), 1 (fp32 MFMA), 2 (bfloat16 x 3), 3 (bfloat16 x 1) or 4 (off); got %d", filter);
    idx->filter = filter;
    return QV_OK;
}

int qv_index_set_bound_scan(qv_index* idx, int mode) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (mode < 0 || mode > QV_BOUND_SCAN_NEVER) return fail(QV_ERR_INVALID_ARG, "mode must be 0 (automatic), 1 (always) or 2 (never); got %d", mode);
    idx->bound.scan = mode;
    return QV_OK;
}

int qv_index_bound_scan_stats(qv_index* idx, uint64_t out[4]) {
    if (!idx || !out) return fail(QV_ERR_INVALID_ARG, "index/out is null");
    HIPCHK(hipSetDevice(idx->device));
    HIPCHK(hipDeviceSynchronize());
    uint32_t h[3] = {0, 0, 0};
    HIPCHK(hipMemcpy(h, idx->d_bound_stats, sizeof(h), hipMemcpyDeviceToHost));
    out[0] = h[0]; out[1] = h[1]; out[2] = h[2]; out[3] = idx->d_bf16 != nullptr ? 1 : 0;
    return QV_OK;
}

// the four plane knobs, one per form of the bound scan (qv::BoundForm)
static int set_bound_plane(qv_index* idx, qv::BoundForm form, int mode) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (mode < 0 || mode > QV_BOUND_PLANE_BF16) return fail(QV_ERR_INVALID_ARG, "mode must be 0 (automatic), 1 (8-bit first) or 2 (bfloat16 only); got %d", mode);
    idx->bound.plane[form] = mode;
    return QV_OK;
}
int qv_index_set_bound_plane(qv_index* idx, int mode) { return set_bound_plane(idx, qv::bound_one, mode); }
int qv_index_set_bound_plane_filtered(qv_index* idx, int mode) { return set_bound_plane(idx, qv::bound_one_filtered, mode); }
int qv_index_set_bound_plane_mq(qv_index* idx, int mode) { return set_bound_plane(idx, qv::bound_mq, mode); }
int qv_index_set_bound_plane_filtered_mq(qv_index* idx, int mode) { return set_bound_plane(idx, qv::bound_mq_filtered, mode); }

int qv_index_set_bound_plane6(qv_index* idx, int mode) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (mode < 0 || mode > QV_BOUND_PLANE6_NEVER) return fail(QV_ERR_INVALID_ARG, "mode must be 0 (automatic), 1 (6-bit first) or 2 (never); got %d", mode);
    idx->bound.plane6 = mode;
    return QV_OK;
}

int qv_index_set_filtered_batch(qv_index* idx, int mode, uint32_t sparse_ppm) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (mode < 0 || mode > QV_FILTERED_BATCH_NEVER) return fail(QV_ERR_INVALID_ARG, "mode must be 0 (automatic), 1 (always) or 2 (never); got %d", mode);
    if (sparse_ppm != 0xFFFFFFFFu && sparse_ppm > 1000000u)
        return fail(QV_ERR_INVALID_ARG, "sparse_ppm is a share of the rows in millionths, 0 .. 1000000, or 0xFFFFFFFF for the default; got %u", sparse_ppm);
    idx->filtered_batch = mode;
    idx->filtered_batch_ppm = sparse_ppm;
    return QV_OK;
}

int qv_index_filtered_batch_stats(qv_index* idx, uint64_t out[4]) {
    if (!idx || !out) return fail(QV_ERR_INVALID_ARG, "index/out is null");
    for (int i = 0; i < 4; i++) out[i] = idx->fb_stats[i].load();
    return QV_OK;
}

int qv_batched_applies_filtered(int metric, uint32_t dim, uint64_t rows, uint32_t nq, uint32_t k, int filter, int mode, uint32_t n_not_sparse) {
    if (mode < 0 || mode > QV_FILTERED_BATCH_NEVER) return fail(QV_ERR_INVALID_ARG, "mode must be 0 (automatic), 1 (always) or 2 (never); got %d", mode);
    if (filter < QV_FILTER_AUTO || filter > QV_FILTER_OFF) return fail(QV_ERR_INVALID_ARG, "filter must be one of QV_FILTER_*; got %d", filter);
    return qv::filtered_batch_rule(metric, dim, rows, nq, k, filter, mode, std::min(n_not_sparse, nq)) ? 1 : 0;
}

int qv_batched_filter_route(int metric, uint32_t dim, uint64_t rows, uint32_t nq, uint32_t k, int filter, int has_bf16_plane, int cus, uint32_t* nq_pad, int* kernel) {
    if (!nq_pad || !kernel) return fail(QV_ERR_INVALID_ARG, "nq_pad/kernel is null");
    if (filter < QV_FILTER_AUTO || filter > QV_FILTER_OFF) return fail(QV_ERR_INVALID_ARG, "filter must be one of QV_FILTER_*; got %d", filter);
    if (cus < 1) return fail(QV_ERR_INVALID_ARG, "cus must be positive; got %d", cus);
    if (!qv::batched_sets_filter(metric, dim, rows, nq, k, filter, has_bf16_plane != 0, cus, nq_pad, kernel))
        return fail(QV_ERR_UNSUPPORTED, "no filtered batched route for %u queries, k %u over %llu rows of %u dimensions", nq, k, (unsigned long long)rows, dim);
    return QV_OK;
}

int qv_batched_sample_plan(qv_index* idx, uint32_t nq, uint32_t k, uint32_t* sample_rows, uint32_t* group_step, uint32_t* rank) {
    if (!idx || !sample_rows || !group_step || !rank) return fail(QV_ERR_INVALID_ARG, "index/sample_rows/group_step/rank is null");
    if (!qv::batched_sample_plan(idx->view(), nq, k, idx->cus, sample_rows, group_step, rank))
        return fail(QV_ERR_UNSUPPORTED, "no batched route with a sample from a filter kernel for %u queries, k %u on this index", nq, k);
    return QV_OK;
}

int qv_index_bound_scan8_stats(qv_index* idx, uint64_t out[4]) {
    if (!idx || !out) return fail(QV_ERR_INVALID_ARG, "index/out is null");
    HIPCHK(hipSetDevice(idx->device));
    HIPCHK(hipDeviceSynchronize());
    uint32_t h[3] = {0, 0, 0};
    HIPCHK(hipMemcpy(h, idx->d_bound_stats + qv::kBound8StatsWord, sizeof(h), hipMemcpyDeviceToHost));
    out[0] = h[0]; out[1] = h[1]; out[2] = h[2]; out[3] = idx->d_plane8 != nullptr ? 1 : 0;
    return QV_OK;
}

int qv_index_bound_scan6_stats(qv_index* idx, uint64_t out[4]) {
    if (!idx || !out) return fail(QV_ERR_INVALID_ARG, "index/out is null");
    HIPCHK(hipSetDevice(idx->device));
    HIPCHK(hipDeviceSynchronize());
    uint32_t h[3] = {0, 0, 0};
    HIPCHK(hipMemcpy(h, idx->d_bound_stats + qv::kBound6StatsWord, sizeof(h), hipMemcpyDeviceToHost));
    out[0] = h[0]; out[1] = h[1]; out[2] = h[2]; out[3] = idx->d_plane6 != nullptr ? 1 : 0;
    return QV_OK;
}

int qv_index_set_bound_scan_wide(qv_index* idx, int mode) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (mode < 0 || mode > QV_BOUND_SCAN_NEVER) return fail(QV_ERR_INVALID_ARG, "mode must be 0 (automatic), 1 (always) or 2 (never); got %d", mode);
    idx->bound_wide = mode;
    return QV_OK;
}

int qv_index_set_bound_scan_wide_filtered(qv_index* idx, int mode) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (mode < 0 || mode > QV_BOUND_SCAN_NEVER) return fail(QV_ERR_INVALID_ARG, "mode must be 0 (automatic), 1 (always) or 2 (never); got %d", mode);
    idx->bound_wide_filtered = mode;
    return QV_OK;
}

int qv_index_bound_scan_wide_stats(qv_index* idx, uint64_t out[4]) {
    if (!idx || !out) return fail(QV_ERR_INVALID_ARG, "index/out is null");
    HIPCHK(hipSetDevice(idx->device));
    HIPCHK(hipDeviceSynchronize());
    uint32_t h[3] = {0, 0, 0};
    HIPCHK(hipMemcpy(h, idx->d_bound_stats + qv::kBoundWideStatsWord, sizeof(h), hipMemcpyDeviceToHost));
    out[0] = h[0]; out[1] = h[1]; out[2] = h[2]; out[3] = idx->d_bf16 != nullptr ? 1 : 0;
    return QV_OK;
}

int qv_index_set_bound_scan_wide_mq(qv_index* idx, int mode) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (mode < 0 || mode > QV_BOUND_SCAN_NEVER) return fail(QV_ERR_INVALID_ARG, "mode must be 0 (automatic), 1 (always) or 2 (never); got %d", mode);
    idx->bound_wide_mq = mode;
    return QV_OK;
}

int qv_index_bound_scan_wide_mq_stats(qv_index* idx, uint64_t out[4]) {
    if (!idx || !out) return fail(QV_ERR_INVALID_ARG, "index/out is null");
    HIPCHK(hipSetDevice(idx->device));
    HIPCHK(hipDeviceSynchronize());
    uint32_t h[3] = {0, 0, 0};
    HIPCHK(hipMemcpy(h, idx->d_bound_stats + qv::kBoundWideMqStatsWord, sizeof(h), hipMemcpyDeviceToHost));
    out[0] = h[0]; out[1] = h[1]; out[2] = h[2]; out[3] = idx->d_bf16 != nullptr ? 1 : 0;
    return QV_OK;
}

int qv_scan_bound_wide_route_mq(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int wide_mq_mode, int plane_mode_mq, int has_plane, int has_plane8) {
    if (wide_mq_mode < 0 || wide_mq_mode > QV_BOUND_SCAN_NEVER) return fail(QV_ERR_INVALID_ARG, "wide_mq_mode must be 0 (automatic), 1 (always) or 2 (never); got %d", wide_mq_mode);
    if (plane_mode_mq < 0 || plane_mode_mq > QV_BOUND_PLANE_BF16) return fail(QV_ERR_INVALID_ARG, "plane_mode_mq must be 0 (automatic), 1 (8-bit first) or 2 (bfloat16 only); got %d", plane_mode_mq);
    return qv::bound_wide_route_mq(metric, dim, rows, nq, k, wide_mq_mode, plane_mode_mq, has_plane != 0, has_plane8 != 0);
}

int qv_scan_bound_wide_route(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int wide_mode, int plane_mode, int has_plane, int has_plane8) {
    if (wide_mode < 0 || wide_mode > QV_BOUND_SCAN_NEVER) return fail(QV_ERR_INVALID_ARG, "wide_mode must be 0 (automatic), 1 (always) or 2 (never); got %d", wide_mode);
    if (plane_mode < 0 || plane_mode > QV_BOUND_PLANE_BF16) return fail(QV_ERR_INVALID_ARG, "plane_mode must be 0 (automatic), 1 (8-bit first) or 2 (bfloat16 only); got %d", plane_mode);
    return qv::bound_wide_route(metric, dim, rows, nq, k, wide_mode, plane_mode, has_plane != 0, has_plane8 != 0);
}

int qv_scan_bound_wide_route_filtered(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int wide_mode, int plane_mode_filtered, int has_plane, int has_plane8,
                                      uint32_t candidate_tiles, uint64_t candidates) {
    if (wide_mode < 0 || wide_mode > QV_BOUND_SCAN_NEVER) return fail(QV_ERR_INVALID_ARG, "wide_mode must be 0 (automatic), 1 (always) or 2 (never); got %d", wide_mode);
    if (plane_mode_filtered < 0 || plane_mode_filtered > QV_BOUND_PLANE_BF16)
        return fail(QV_ERR_INVALID_ARG, "plane_mode_filtered must be 0 (automatic), 1 (8-bit first) or 2 (bfloat16 only); got %d", plane_mode_filtered);
    return qv::bound_wide_route_filtered(metric, dim, rows, nq, k, wide_mode, plane_mode_filtered, has_plane != 0, has_plane8 != 0, std::min(candidate_tiles, qv::kBoundNoFilter - 1), candidates);   // (a count, never the "no filter" mark)
}

// The six rule exports: views of the one decision (qv::bound_scan_decide) for a call given without an index.  form: the form the export
// speaks for (it says no to any other; -1: whichever the call has); want: the stage asked after — plane8_first, or any stage at all.  The
// 8-bit rules are asked with the bfloat16 copy held; a filtered rule takes every candidate count as a count.
static int bound_export(int form, qv::BoundStages want, int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, const char* plane_name, int plane_mode,
                        int has_plane, int has_plane8, uint32_t candidate_tiles) {
    if (mode < 0 || mode > QV_BOUND_SCAN_NEVER) return fail(QV_ERR_INVALID_ARG, "mode must be 0 (automatic), 1 (always) or 2 (never); got %d", mode);
    if (plane_mode < 0 || plane_mode > QV_BOUND_PLANE_BF16) return fail(QV_ERR_INVALID_ARG, "%s must be 0 (automatic), 1 (8-bit first) or 2 (bfloat16 only); got %d", plane_name, plane_mode);
    const qv::BoundAsk ask = {metric, dim, rows, nq, k, candidate_tiles, has_plane != 0, has_plane8 != 0};
    qv::BoundKnobs knobs = {mode, {0, 0, 0, 0}};
    knobs.plane[qv::bound_form(ask)] = plane_mode;
    if (form >= 0 && form != qv::bound_form(ask)) return 0;
    const qv::BoundStages got = qv::bound_scan_decide(ask, knobs);
    return (want == qv::BoundStages::plane8_first ? qv::bound_stages_8bit(got) : got != qv::BoundStages::none) ? 1 : 0;
}
static uint32_t as_count(uint32_t candidate_tiles) { return std::min(candidate_tiles, qv::kBoundNoFilter - 1); }

int qv_scan_bound8_applies(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, int plane_mode, int has_plane8) {
    return bound_export(qv::bound_one, qv::BoundStages::plane8_first, metric, dim, rows, nq, k, mode, "plane_mode", plane_mode, 1, has_plane8, qv::kBoundNoFilter);
}

int qv_scan_bound8_applies_filtered(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, int plane_mode_filtered, int has_plane8, uint32_t candidate_tiles) {
    return bound_export(qv::bound_one_filtered, qv::BoundStages::plane8_first, metric, dim, rows, nq, k, mode, "plane_mode_filtered", plane_mode_filtered, 1, has_plane8, as_count(candidate_tiles));
}

int qv_scan_bound8_applies_mq(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, int plane_mode_mq, int has_plane8) {
    return bound_export(qv::bound_mq, qv::BoundStages::plane8_first, metric, dim, rows, nq, k, mode, "plane_mode_mq", plane_mode_mq, 1, has_plane8, qv::kBoundNoFilter);
}

int qv_scan_bound8_applies_filtered_mq(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, int plane_mode_filtered_mq, int has_plane8, uint32_t candidate_tiles) {
    return bound_export(qv::bound_mq_filtered, qv::BoundStages::plane8_first, metric, dim, rows, nq, k, mode, "plane_mode_filtered_mq", plane_mode_filtered_mq, 1, has_plane8, as_count(candidate_tiles));
}

int qv_scan_bound6_applies(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, int plane_mode, int plane6_mode, int has_plane8, int has_plane6) {
    if (mode < 0 || mode > QV_BOUND_SCAN_NEVER) return fail(QV_ERR_INVALID_ARG, "mode must be 0 (automatic), 1 (always) or 2 (never); got %d", mode);
    if (plane_mode < 0 || plane_mode > QV_BOUND_PLANE_BF16) return fail(QV_ERR_INVALID_ARG, "plane_mode must be 0 (automatic), 1 (8-bit first) or 2 (bfloat16 only); got %d", plane_mode);
    if (plane6_mode < 0 || plane6_mode > QV_BOUND_PLANE6_NEVER) return fail(QV_ERR_INVALID_ARG, "plane6_mode must be 0 (automatic), 1 (6-bit first) or 2 (never); got %d", plane6_mode);
    qv::BoundAsk ask = {metric, dim, rows, nq, k, qv::kBoundNoFilter, true, has_plane8 != 0};
    ask.has_plane6 = has_plane6 != 0;
    qv::BoundKnobs knobs = {mode, {0, 0, 0, 0}};
    knobs.plane[qv::bound_one] = plane_mode; knobs.plane6 = plane6_mode;
    if (qv::bound_form(ask) != qv::bound_one) return 0;
    return qv::bound_scan_decide(ask, knobs) == qv::BoundStages::plane6_first ? 1 : 0;
}

int qv_scan_quantize_row6(uint32_t dim, const float* row, float scale8, uint8_t* out_bytes, float* out_res) {
    if (!row || !out_bytes || !out_res || dim == 0 || (dim & 63u) != 0) return fail(QV_ERR_INVALID_ARG, "row/out is null or dim is not a positive multiple of 64");
    return qv::host_quantize_row6(dim, row, scale8, out_bytes, out_res);
}

int qv_scan_unpack_row6(uint32_t dim, const uint8_t* bytes, uint8_t* out_codes) {
    if (!bytes || !out_codes || dim == 0 || (dim & 63u) != 0) return fail(QV_ERR_INVALID_ARG, "bytes/out is null or dim is not a positive multiple of 64");
    return qv::host_unpack_row6(dim, bytes, out_codes);
}

int qv_scan_bound_interval8(int metric, uint32_t dim, int64_t isum, double sq, double qn, double qres, double rn, float rscale8, float rres8, float* d_lo, float* d_hi) {
    if (metric != QV_COSINE && metric != QV_DOT && metric != QV_L2) return fail(QV_ERR_UNSUPPORTED, "the bound scan's metrics are cosine, dot and l2; got %d", metric);
    if (!d_lo || !d_hi || dim == 0) return fail(QV_ERR_INVALID_ARG, "d_lo/d_hi is null or dim is 0");
    return qv::host_bound_interval8(metric, dim, (long long)isum, sq, qn, qres, rn, rscale8, rres8, d_lo, d_hi);
}

int qv_scan_quantize_row8(uint32_t dim, const float* row, int8_t* out_bytes, float* out_scale, float* out_res) {
    if (!row || !out_bytes || !out_scale || !out_res || dim == 0) return fail(QV_ERR_INVALID_ARG, "row/out is null or dim is 0");
    return qv::host_quantize_row8(dim, row, out_bytes, out_scale, out_res);
}

int qv_scan_bound_interval(int metric, uint32_t dim, float s, double qn, double rn, float rres, float* d_lo, float* d_hi) {
    // (QV_L2 stays unsupported HERE, as callers of this entry point have known it: its interval is qv_scan_bound_interval_l2)
    if (metric != QV_COSINE && metric != QV_DOT)
        return fail(QV_ERR_UNSUPPORTED, "the bound scan's metrics are cosine, dot and l2, and this function serves cosine and dot (l2: qv_scan_bound_interval_l2); got %d", metric);
    if (!d_lo || !d_hi || dim == 0) return fail(QV_ERR_INVALID_ARG, "d_lo/d_hi is null or dim is 0");
    return qv::host_bound_interval(metric, dim, s, qn, rn, rres, d_lo, d_hi);
}

int qv_scan_bound_interval_l2(uint32_t dim, float s, double qn, double rn, float rres, float* d_lo, float* d_hi) {
    if (!d_lo || !d_hi || dim == 0) return fail(QV_ERR_INVALID_ARG, "d_lo/d_hi is null or dim is 0");
    return qv::host_bound_interval(QV_L2, dim, s, qn, rn, rres, d_lo, d_hi);
}

int qv_index_debug_read(qv_index* idx, int what, void* out, size_t bytes) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    const int m = idx->metric;
    const bool f64norm = m == QV_COSINE || m == QV_DOT || m == QV_L2 || m == QV_L2SQ;   // the metrics ingest keeps |r| and the residual for
    const size_t tiles = ((size_t)idx->n_rows + 63) / 64;
    const void* src = nullptr; size_t need = 0;
    if (what == QV_DEBUG_RNORM) {
        if (!f64norm && m != QV_COSINE_F32) return fail(QV_ERR_UNSUPPORTED, "metric %d keeps no row norms", m);
        src = idx->d_rnorm; need = tiles * 64 * sizeof(double);
    } else if (what == QV_DEBUG_RRES) {
        if (!f64norm) return fail(QV_ERR_UNSUPPORTED, "metric %d keeps no bfloat16 residuals", m);
        src = idx->d_rres; need = tiles * 64 * sizeof(float);
    } else if (what == QV_DEBUG_PLANE) {
        if (!idx->wants_plane() || (tiles && !idx->d_bf16)) return fail(QV_ERR_UNSUPPORTED, "this index keeps no bfloat16 copy");
        src = idx->d_bf16; need = tiles * idx->bf16_tile_bytes();
    } else if (what == QV_DEBUG_ROWMAJ16 && (idx->flags & QV_FLAG_GRAPH_PLANE)) {   // (an index created without the flag answers as it always did: an unknown code)
        if (!idx->wants_rowmaj16() || (tiles && !idx->d_rowmaj16)) return fail(QV_ERR_UNSUPPORTED, "this index keeps no row-order bfloat16 copy");
        src = idx->d_rowmaj16; need = (size_t)idx->n_rows * idx->dim * sizeof(uint16_t);
    } else if ((what == QV_DEBUG_ROWMAJ8 || what == QV_DEBUG_ROWMETA8) && (idx->flags & QV_FLAG_GRAPH_PLANE8)) {   // (without the flag: an unknown code, as always)
        if (!idx->wants_rowmaj8() || (tiles && !idx->d_rowmaj8)) return fail(QV_ERR_UNSUPPORTED, "this index keeps no row-order 8-bit image");
        if (what == QV_DEBUG_ROWMAJ8) { src = idx->d_rowmaj8; need = (size_t)idx->n_rows * idx->dim; }
        else { src = idx->d_rowmeta8; need = (size_t)idx->n_rows * sizeof(qv::RowMeta8); }
    } else if ((what == QV_DEBUG_PLANE6 || what == QV_DEBUG_RRES6 || what == QV_DEBUG_RSCALE8) && idx->wants_plane6()) {   // (an index that keeps no such plane answers as it always did: an unknown code)
        if (tiles && !idx->d_plane6) return fail(QV_ERR_UNSUPPORTED, "this index keeps no 6-bit plane");
        if (what == QV_DEBUG_PLANE6) { src = idx->d_plane6; need = tiles * idx->plane6_tile_bytes(); }
        else { src = what == QV_DEBUG_RRES6 ? idx->d_rres6 : idx->d_rscale8; need = tiles * 64 * sizeof(float); }
    } else if ((what == QV_DEBUG_PLANE8 || what == QV_DEBUG_RRES8) && idx->wants_plane8()) {   // (an index that keeps no 8-bit plane: an unknown code, as for the 6-bit codes)
        if (tiles && !idx->d_plane8) return fail(QV_ERR_UNSUPPORTED, "this index keeps no 8-bit plane");
        if (what == QV_DEBUG_PLANE8) { src = idx->d_plane8; need = tiles * idx->plane8_tile_bytes(); }
        else { src = idx->d_rres8; need = tiles * 64 * sizeof(float); }
    } else return fail(QV_ERR_INVALID_ARG, "what must be 0 (norms), 1 (residuals), 2 (the bfloat16 copy) or 3 (the row-order bfloat16 copy); got %d", what);
    if (bytes < need) return fail(QV_ERR_INVALID_ARG, "%zu bytes given, %zu needed", bytes, need);
    if (need == 0) return QV_OK;
    if (!out) return fail(QV_ERR_INVALID_ARG, "out is null");
    HIPCHK(hipSetDevice(idx->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, src, need, hipMemcpyDeviceToHost));
    return QV_OK;
}

int qv_scan_bound_applies(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, int has_plane) {
    return bound_export(-1, qv::BoundStages::bf16, metric, dim, rows, nq, k, mode, "", 0, has_plane, 0, qv::kBoundNoFilter);
}

int qv_scan_route(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int cus, int tickets, int bound_mode, int plane_mode, int has_plane, int has_plane8,
                  uint32_t candidate_tiles) {
    return qv_scan_route_ex(metric, dim, rows, nq, k, cus, tickets, bound_mode, plane_mode, has_plane, has_plane8, candidate_tiles, QV_BOUND_PLANE_BF16);
}

int qv_scan_route_ex(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int cus, int tickets, int bound_mode, int plane_mode, int has_plane, int has_plane8,
                     uint32_t candidate_tiles, int plane_mode_filtered) {
    if (plane_mode_filtered < 0 || plane_mode_filtered > QV_BOUND_PLANE_BF16) return fail(QV_ERR_INVALID_ARG, "plane_mode_filtered must be 0 (automatic), 1 (8-bit first) or 2 (bfloat16 only); got %d", plane_mode_filtered);
    if (bound_mode < 0 || bound_mode > QV_BOUND_SCAN_NEVER) return fail(QV_ERR_INVALID_ARG, "bound_mode must be 0 (automatic), 1 (always) or 2 (never); got %d", bound_mode);
    if (plane_mode < 0 || plane_mode > QV_BOUND_PLANE_BF16) return fail(QV_ERR_INVALID_ARG, "plane_mode must be 0 (automatic), 1 (8-bit first) or 2 (bfloat16 only); got %d", plane_mode);
    const int route = qv::host_flat_route(metric, dim, rows, nq, k, cus, tickets, bound_mode, plane_mode, has_plane, has_plane8, candidate_tiles, plane_mode_filtered);
    return route >= 0 ? route : fail(QV_ERR_INVALID_ARG, "no fused flat search has these arguments (metric %d, dim %u, rows %u, nq %u, k %u, cus %d)", metric, dim, rows, nq, k, cus);
}

int qv_scan_bound_applies_filtered(int metric, uint32_t dim, uint32_t rows, uint32_t nq, uint32_t k, int mode, int has_plane, uint32_t candidate_tiles) {
    return bound_export(-1, qv::BoundStages::bf16, metric, dim, rows, nq, k, mode, "", 0, has_plane, 0, as_count(candidate_tiles));
}

int qv_scan_workspace_layout(int kind, int metric, uint32_t dim, uint64_t rows, uint32_t nq, uint32_t k, int cus, uint32_t flags,
                             uint64_t* total, uint64_t* end, uint32_t* n_regions, uint64_t* regions, uint32_t cap) {
    if (!total || !end || !n_regions || (cap && !regions)) return fail(QV_ERR_INVALID_ARG, "total/end/n_regions/regions is null");
    if (metric < QV_COSINE || metric > QV_L2SQ_F64 || dim == 0 || rows == 0 || rows > 0xFFFFFFF0ull || nq == 0 || k == 0 || cus < 1)
        return fail(QV_ERR_INVALID_ARG, "no workspace has these arguments (metric %d, dim %u, rows %llu, nq %u, k %u, cus %d)", metric, dim, (unsigned long long)rows, nq, k, cus);
    const uint32_t n_tiles = (uint32_t)((rows + 63) / 64), dim4 = (dim + 3) / 4;
    const qv::ScanPlan p = qv::plan_scan(n_tiles, cus);
    qv::WsLog log;
    switch (kind) {
        case QV_WS_BOUND:            (void)qv::bound_scan_workspace_bytes(p, k, n_tiles, &log); break;
        case QV_WS_BOUND_MQ:         (void)qv::bound_scan_mq_workspace_bytes(p, nq, k, n_tiles, dim, &log); break;
        case QV_WS_BOUND_WIDE:       (void)qv::bound_scan_wide_workspace_bytes(p, k, n_tiles, dim, &log); break;
        case QV_WS_BOUND_WIDE_MQ:    (void)qv::bound_scan_wide_mq_workspace_bytes(p, nq, k, n_tiles, dim, &log); break;
        case QV_WS_REDO:             (void)qv::redo_workspace_bytes(p, nq, k, &log); break;
        case QV_WS_SELECT:           (void)qv::select_workspace_bytes(nq, k, &log); break;
        case QV_WS_FLAT_WIDE:        (void)qv::flat_wide_workspace_bytes(p, nq, k, &log); break;
        case QV_WS_FLAT_SELECT:      (void)qv::flat_select_workspace_bytes(n_tiles, nq, k, dim4, &log); break;
        case QV_WS_FLAT_SELECT_REDO: (void)qv::flat_select_redo_workspace_bytes(n_tiles, nq, k, dim, dim4, &log); break;
        case QV_WS_MERGE_SELECT:     (void)qv::merge_select_workspace_bytes(flags, nq, (uint32_t)rows, k, &log); break;
        case QV_WS_MERGE_RANKED:     (void)qv::merge_ranked_workspace_bytes(rows, &log); break;
        case QV_WS_FULL_SORT:        (void)qv::full_sort_workspace_bytes(n_tiles, &log); break;
        case QV_WS_MQ64:             (void)qv::mq64_workspace_bytes(nq, dim4, &log); break;
        case QV_WS_ROWSET:           (void)qv::rowset_workspace_bytes(p, nq, k, dim4, &log); break;
        case QV_WS_FLAT:
            if (flags > QV_WS_FLAT_BOUND_MQ) return fail(QV_ERR_INVALID_ARG, "flags must be one of QV_WS_FLAT_*; got %u", flags);
            (void)qv::flat_layout(nullptr, flags == QV_WS_FLAT_BOUND_MQ ? qv::FlatWs::call_bound_mq : flags == QV_WS_FLAT_BOUND ? qv::FlatWs::call_bound : qv::FlatWs::call, p, nq, k, n_tiles, dim, &log);
            break;
        case QV_WS_ROWSETS_CALL: case QV_WS_WHERE_CALL: {                 // (the plan of a shared pass: rowsets_plan's k <= kMaxFusedK, nq >= 2 branch)
            const size_t plan_bytes = std::max(qv::rowset_workspace_bytes(p, nq, k, dim4), (flags & 1u) ? qv::bound_scan_mq_workspace_bytes(p, nq, k, n_tiles, dim) : (size_t)0);
            const size_t words = n_tiles, stride = qv::up256(words * 8);
            if (kind == QV_WS_ROWSETS_CALL) (void)filtered_call_layout(nullptr, plan_bytes, words * 8, 0, 0, &log);
            else (void)filtered_call_layout(nullptr, plan_bytes, stride, flags >> 8, stride, &log);
        } break;
        default: return fail(QV_ERR_INVALID_ARG, "kind must be one of QV_WS_*; got %d", kind);
    }
    *total = log.total; *end = log.end; *n_regions = log.n;
    for (uint32_t i = 0; i < std::min(std::min(log.n, cap), qv::WsLog::kCap); i++) {
        regions[4 * i] = log.r[i].off; regions[4 * i + 1] = log.r[i].bytes; regions[4 * i + 2] = log.r[i].align; regions[4 * i + 3] = log.r[i].alias ? 1 : 0;
    }
    return QV_OK;
}

int qv_index_profile(qv_index* idx, int enable) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    idx->profiling = enable != 0;
    return QV_OK;
}

int qv_index_profile_read(qv_index* idx, double* scan_ms_sum_out, uint64_t* launches_out) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    HIPCHK(hipSetDevice(idx->device));
    std::lock_guard<std::mutex> g(idx->prof_mu);
    double sum = 0.0; uint64_t n = 0;
    for (auto& pr : idx->prof_events) {
        float ms = 0.f;
        if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { sum += ms; n++; }
        (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second);
    }
    idx->prof_events.clear();
    if (scan_ms_sum_out) *scan_ms_sum_out = sum;
    if (launches_out) *launches_out = n;
    return QV_OK;
}

int qv_distance_rows_device(qv_index* idx, const float* d_query, const uint32_t* d_rows, uint32_t n,
                            float* d_dist_out, void* stream) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (n == 0) return QV_OK;
    if (!d_query || !d_rows || !d_dist_out) return fail(QV_ERR_INVALID_ARG, "null device pointer");
    HIPCHK(hipSetDevice(idx->device));
    hipError_t e = qv::launch_distance_rows(idx->view(), d_query, d_rows, n, d_dist_out, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(QV_ERR_DEVICE, "distance_rows launch failed: %s", hipGetErrorString(e));
    return QV_OK;
}

int qv_distance_rows(qv_index* idx, const float* query, const uint32_t* rows, uint32_t n, float* dist_out) {
    if (!idx) return fail(QV_ERR_INVALID_ARG, "index is null");
    if (n == 0) return QV_OK;
    if (!query || !rows || !dist_out) return fail(QV_ERR_INVALID_ARG, "query/rows/dist_out is null");
    for (uint32_t i = 0; i < n; i++)
        if (rows[i] >= idx->n_rows) return fail(QV_ERR_OUT_OF_RANGE, "row %u out of range (rows: %u)", rows[i], idx->n_rows);
    HIPCHK(hipSetDevice(idx->device));
    SearchCtx* c = nullptr;
    int rc = acquire_ctx(idx, &c);
    if (rc != QV_OK) return rc;
    CtxGuard guard{idx, c};
    const size_t qbytes = (size_t)idx->dim * sizeof(float), ibytes = (size_t)n * sizeof(uint32_t), obytes = (size_t)n * sizeof(float);
    if ((rc = c->d_q.ensure(qbytes)) || (rc = c->h_q.ensure(qbytes)) || (rc = c->d_ids.ensure(ibytes)) || (rc = c->h_ids.ensure(ibytes)) ||
        (rc = c->d_dist.ensure(obytes)) || (rc = c->h_dist.ensure(obytes)))
        return rc;
    memcpy(c->h_q.p, query, qbytes);
    memcpy(c->h_ids.p, rows, ibytes);
    // This call is a latency path (one searchLayer hop: a 3 KB query, <= 64 row ids, <= 64 floats back).  The pinned staging
    // buffers are device-visible, so the kernel reads the query and the ids from them and writes the distances into one
    // directly: one launch and one stream sync, no copy commands in between.
    hipError_t e = qv::launch_distance_rows(idx->view(), static_cast<const float*>(c->h_q.p), static_cast<const uint32_t*>(c->h_ids.p), n,
                                            static_cast<float*>(c->h_dist.p), c->stream);
    if (e != hipSuccess) return fail(QV_ERR_DEVICE, "distance_rows launch failed: %s", hipGetErrorString(e));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(dist_out, c->h_dist.p, obytes);
    return QV_OK;
}

// The DistanceFunc contract for ONE pair (surface.go:8; SURVEY.md 8b lists this entry point as host code): the reference calls
// it per pair at ~78 ns (final_bench.txt:47) from code that is not part of the scan — Surface.Distance, tests, the Go HNSW that
// reloaded collections use — and no GPU round trip (tens of microseconds) can serve that.  It is NOT a fallback of anything:
// every search / scan / batch entry point of this library runs on the device or fails, and none of them calls this.  The body
// is the kernels' own pair_distance<M> (qv_kernels.h) compiled for the host, so device and host state the arithmetic once.
int qv_distance_pair(qv_metric metric, const float* a, const float* b, uint32_t dim, float* out) {
    if ((int)metric < 0 || (int)metric >= QV_METRIC_COUNT) return fail(QV_ERR_INVALID_ARG, "unknown metric %d", (int)metric);
    if (!out || (dim && (!a || !b))) return fail(QV_ERR_INVALID_ARG, "a/b/out is null");
    *out = qv::host_pair_distance((int)metric, a, b, dim);
    return QV_OK;
}

int qv_distance_pairs(qv_metric metric, const float* a, const float* b, uint32_t n, uint32_t dim, float* dist_out, int device) {
    if ((int)metric < 0 || (int)metric >= QV_METRIC_COUNT) return fail(QV_ERR_INVALID_ARG, "unknown metric %d", (int)metric);
    if (n == 0) return QV_OK;
    if (!a || !b || !dist_out) return fail(QV_ERR_INVALID_ARG, "a/b/dist_out is null");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(QV_ERR_NO_DEVICE, "no HIP device available; libqv has no CPU path");
    if (device < 0 || device >= ndev) return fail(QV_ERR_INVALID_ARG, "device %d out of range (have %d)", device, ndev);
    HIPCHK(hipSetDevice(device));
    // grow-only device buffers per device, shared by all callers (one call at a time per device): no hipMalloc per call
    struct PairBufs { std::mutex mu; Buf a, b, out; };
    static std::mutex table_mu;
    static std::map<int, PairBufs*> table;
    PairBufs* pb;
    { std::lock_guard<std::mutex> g(table_mu); PairBufs*& slot = table[device]; if (!slot) slot = new PairBufs(); pb = slot; }
    std::lock_guard<std::mutex> g(pb->mu);
    const size_t bytes = (size_t)n * dim * sizeof(float);
    int rc;
    if ((rc = pb->a.ensure(std::max<size_t>(bytes, 16))) || (rc = pb->b.ensure(std::max<size_t>(bytes, 16))) || (rc = pb->out.ensure((size_t)n * sizeof(float)))) return rc;
    if (bytes) e = hipMemcpy(pb->a.p, a, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && bytes) e = hipMemcpy(pb->b.p, b, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = qv::launch_distance_pairs((int)metric, static_cast<const float*>(pb->a.p), static_cast<const float*>(pb->b.p), n, dim, static_cast<float*>(pb->out.p), nullptr);
    if (e == hipSuccess) e = hipMemcpy(dist_out, pb->out.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(QV_ERR_DEVICE, "distance_pairs failed: %s", hipGetErrorString(e));
    return QV_OK;
}

}  // extern "C"

// Internal (qv_api_internal.h), for the sharded handle: the exact scan over the rows selected by a DEVICE bitmap d_candidates
// (already ANDed with the live rows by the caller; `matching` = its population count), enqueued on `stream`, no
// synchronisation.  Writes [nq][k_stride] lists: min(k_stride, matching) results, the rest padded (0xFFFFFFFF, +inf).
int qv_internal_search_candidates_device(qv_index* idx, const float* d_queries, uint32_t nq, uint32_t k_stride, const uint64_t* d_candidates,
                                         uint64_t matching, uint32_t* d_rows_out, float* d_dist_out, void* stream) {
    if (!idx || !d_queries || !d_candidates || !d_rows_out || !d_dist_out || k_stride == 0) return fail(QV_ERR_INVALID_ARG, "null argument");
    if (nq == 0) return QV_OK;
    HIPCHK(hipSetDevice(idx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t kk = (uint32_t)std::min<uint64_t>(k_stride, matching);
    void* ws = nullptr;
    std::unique_lock<std::mutex> ws_hold;
    int rc = stream_workspace(idx, s, search_ws_bytes(idx, nq, kk, k_stride, false), &ws, &ws_hold);
    if (rc != QV_OK) return rc;
    SearchExtras x;
    x.d_candidates = d_candidates;
    return enqueue_search(idx, d_queries, nq, kk, k_stride, ws, d_rows_out, d_dist_out, s, x);
}

// Internal, for the sharded handle: the exact scan for the queries of a batch whose d_flags word is set (handed back by
// qv_index_search_batched_device), enqueued on `stream` behind the batch — listed and scanned on the device, nothing read back.
int qv_internal_redo_flagged_device(qv_index* idx, const float* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_flags,
                                    uint32_t* d_rows_out, float* d_dist_out, void* stream) {
    if (!idx || !d_queries || !d_flags || !d_rows_out || !d_dist_out || k == 0 || k > (uint32_t)qv::kMaxSelectK) return fail(QV_ERR_INVALID_ARG, "bad argument");
    if (nq == 0) return QV_OK;
    HIPCHK(hipSetDevice(idx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const qv::IndexView v = idx->view();
    const qv::ScanPlan plan = qv::plan_scan(v.n_tiles, idx->cus);
    void* ws = nullptr;
    std::unique_lock<std::mutex> ws_hold;
    if (k > (uint32_t)qv::kMaxFusedK) {                               // the selection path's hand-backs: QV_ERR_UNSUPPORTED = the caller reads the flags itself
        int rc0 = stream_workspace(idx, s, qv::flat_select_redo_workspace_bytes(v.n_tiles, nq, k, v.dim, v.dim4), &ws, &ws_hold);
        if (rc0 != QV_OK) return rc0;
        hipError_t e0 = qv::launch_flat_select_redo(v, plan, d_queries, nq, k, k, d_flags, ws, d_rows_out, d_dist_out, s);
        if (e0 == hipErrorNotSupported) return QV_ERR_UNSUPPORTED;
        if (e0 != hipSuccess) return fail(QV_ERR_DEVICE, "redo launch failed: %s", hipGetErrorString(e0));
        return QV_OK;
    }
    int rc = stream_workspace(idx, s, qv::redo_workspace_bytes(plan, nq, k), &ws, &ws_hold);
    if (rc != QV_OK) return rc;
    hipError_t e = qv::launch_flat_redo_flagged(v, plan, d_queries, nq, k, k, d_flags, ws, d_rows_out, d_dist_out, s);
    if (e != hipSuccess) return fail(QV_ERR_DEVICE, "redo launch failed: %s", hipGetErrorString(e));
    return QV_OK;
}

void qv_internal_drop_stream_workspace(qv_index* idx, void* stream) {
    if (!idx) return;
    Workspace* w = nullptr;
    {
        std::lock_guard<std::mutex> g(idx->ws_mu);
        auto it = idx->stream_ws.find(static_cast<hipStream_t>(stream));
        if (it == idx->stream_ws.end()) return;
        w = it->second;
        idx->stream_ws.erase(it);
    }
    { std::lock_guard<std::mutex> hold(w->mu); w->ws.release(); w->tickets.release(); }   // (hipFree waits for the device: nothing of the stream's is still running on it)
    delete w;
}
