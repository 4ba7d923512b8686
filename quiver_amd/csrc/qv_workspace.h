// qv_workspace.h — how a search cuts its one device buffer (d_ws) into regions: said ONCE per buffer, by a layout function that the size
// (run on a null base: `total`) and the launcher (run on the real base: the pointers) both read, so the two cannot disagree.  A layout
// returns a small struct of typed pointers plus `end` (where the last region ends) and `total` (what the caller must provide; end <= total).
// Host only; a run allocates nothing.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace qv {

constexpr size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// what a layout took, in order, for whoever asks (qv_scan_workspace_layout; the launchers pass no log)
struct WsLog {
    static constexpr uint32_t kCap = 16;
    struct Region { size_t off, bytes; uint32_t align; bool alias; } r[kCap];
    uint32_t n = 0;                 // regions taken (those beyond kCap are counted, not kept)
    size_t end = 0, total = 0;
};

// take() moves both `off` (where the next region starts) and `need` (what the caller must provide); take256() the same with the region's
// bytes rounded up to 256 (a ladder's `w += up256(...)`, which its size counted too); align256() moves `off` alone and slack() `need`
// alone — for the sizes that count a flat 256 bytes where the launcher rounds up, and for bytes they count that no region uses.
// An alias — a region that overlays others, because they are dead by the time it is written or belong to another route — is taken from an
// overlay(): a copy of the carver that starts where this one stands; cover() then makes this one hold the larger of the two.
struct WsCarver {
    char* base; size_t off, need;
    WsLog* log = nullptr; bool alias = false;
    template <typename T> T* take(size_t count) {
        const size_t bytes = count * sizeof(T);
        if (log) { if (log->n < WsLog::kCap) log->r[log->n] = {off, bytes, (uint32_t)alignof(T), alias}; log->n++; }
        T* q = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += bytes; need += bytes;
        return q;
    }
    template <typename T> T* take256(size_t count) { T* q = take<T>(count); const size_t pad = up256(off) - off; off += pad; need += pad; return q; }
    void align256() { off = up256(off); }
    void slack(size_t bytes) { need += bytes; }
    WsCarver overlay() const { WsCarver o = *this; o.alias = true; return o; }
    void cover(const WsCarver& o) { off = off > o.off ? off : o.off; need = need > o.need ? need : o.need; }
    // the last line of a layout: its end and total, into the struct and the log
    template <typename L> L finish(L l) const { l.end = off; l.total = need; if (log) { log->end = off; log->total = need; } return l; }
};

}  // namespace qv
