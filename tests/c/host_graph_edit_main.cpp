// host_graph_edit_main.cpp — quiver_amd/csrc/host/qvhost.cpp linked against tests/c/qv_stub.cpp, a stand-in for libqv WITHOUT
// qv_graph_remove / qv_graph_export_lists: the host refers to those two weakly, so the program must link, find both addresses
// null, and run Delete / Insert / Search on the path they took before the entry points existed (the device copy is marked
// stale and uploaded again by the next batch).  TEST INFRASTRUCTURE (tests/test_graph_remove_cpu.py builds it with
// -fsanitize=address,undefined and runs it: exit status 0 and no sanitizer report).
#include <cmath>
#include <cstdio>
#include <random>

#include "../../quiver_amd/csrc/host/qvhost.h"

using namespace quiver;
static int bad = 0;
#define CHECK(c, ...) do { if (!(c)) { bad++; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

static std::vector<float> unit(std::mt19937& g, uint32_t d) {
    std::normal_distribution<float> n(0.f, 1.f);
    std::vector<float> v(d); double s = 0; for (auto& x : v) { x = n(g); s += (double)x * x; }
    for (auto& x : v) x = (float)(x / std::sqrt(s));
    return v;
}

int main() {
    const uint32_t D = 16;
    HNSWConfig cfg; cfg.M = 8; cfg.MaxM0 = 16; cfg.EfConstruction = 40; cfg.EfSearch = 32; cfg.MaxLevel = 6; cfg.seed = 5;
    HNSW h(QV_COSINE, 0, cfg);
    std::mt19937 g(11);
    std::vector<std::string> ids; std::vector<float> pk;
    for (int i = 0; i < 150; i++) { ids.push_back("b" + std::to_string(i)); auto v = unit(g, D); pk.insert(pk.end(), v.begin(), v.end()); }
    Error e = h.InsertBatch(ids, pk.data(), D, 64, 4);
    CHECK(e.empty(), "insert batch: %s", e.c_str());
    CHECK(h.BuiltOnDevice(), "the batch was not connected through the graph entry points");
    uint32_t ep = 0; int lvl = -1;
    h.EntryPoint(&ep, &lvl);
    int live = 150, next = 0;
    auto search = [&](int k) {
        auto q = unit(g, D);
        std::vector<HNSWResult> out;
        Error se = h.Search(q.data(), D, k, &out);
        CHECK(se.empty(), "search: %s", se.c_str());
        CHECK((int)out.size() == std::min(k, live), "%zu results for k = %d of %d live", out.size(), k, live);
        for (size_t i = 1; i < out.size(); i++) CHECK(!(out[i].distance < out[i - 1].distance), "results not ascending at %zu", i);
    };
    search(5);
    CHECK(h.Delete(h.IdOf(ep)).empty(), "delete the entry point"); live--;
    CHECK(!h.BuiltOnDevice(), "a Delete without the in-place entry points must mark the device copy stale");
    search(5);
    for (int r = 0; r < 40; r++) {
        auto v = unit(g, D);
        CHECK(h.Insert("n" + std::to_string(next++), v.data(), D).empty(), "insert"); live++;
        if (r % 3 == 0) { CHECK(h.Delete("b" + std::to_string(10 + r)).empty(), "delete"); live--; }
        if (r % 5 == 0) search(1 + r % 7);
    }
    CHECK(!h.Delete("b10").empty(), "a second Delete of the same id must fail");
    {   // a batch after the mutations uploads the graph again and goes on from there
        std::vector<std::string> ids2; std::vector<float> pk2;
        for (int i = 0; i < 30; i++) { ids2.push_back("m" + std::to_string(i)); auto v = unit(g, D); pk2.insert(pk2.end(), v.begin(), v.end()); }
        e = h.InsertBatch(ids2, pk2.data(), D, 64, 4);
        CHECK(e.empty(), "second insert batch: %s", e.c_str()); live += 30;
    }
    search(10);
    CHECK(h.Delete("m3").empty(), "delete after the second batch"); live--;
    search(10);
    uint64_t st[4];
    h.DeviceState(st);
    CHECK(st[1] == 0 && st[2] == 0, "device edits counted (%llu removes, %llu inserts) without the entry points", (unsigned long long)st[1], (unsigned long long)st[2]);
    CHECK((int)h.Size() == live, "size %u, expected %d", h.Size(), live);
    if (bad) { fprintf(stderr, "%d checks failed\n", bad); return 1; }
    printf("ok: %d live nodes, fallback path, %llu uploads, %llu host-driven searches\n", live, (unsigned long long)st[0], (unsigned long long)st[3]);
    return 0;
}
