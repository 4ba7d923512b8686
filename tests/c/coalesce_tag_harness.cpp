// coalesce_tag_harness.cpp — CPU test harness for the per-member tag of quiver_amd/csrc/qv_coalesce.h (what qv_index_search_rowsets
// hands the front: its array of set handles, one per query).  Every caller submits queries AND a tag that points at an array of its
// own, one word per query; the "device pass" (a sleep) answers query i of a member with a function of the query's first element and of
// tag[i] — so a member whose tag was lost, swapped with a neighbour's, or read at the wrong offset gets a wrong row.  Built by
// tests/test_rowsets_cpu.py as a shared library, and as a program (-DTAG_HARNESS_MAIN) under -fsanitize=thread.  No GPU, no libqv.
#include "../../quiver_amd/csrc/qv_coalesce.h"

#include <chrono>
#include <thread>

extern "C" int coalesce_tag_harness(int lanes, unsigned max_group, unsigned n_threads, unsigned calls_per_thread, unsigned pass_us,
                                    unsigned long long* out /* solo, led, rode, groups, group_queries, wrong */) {
    qvco::Front front(lanes, max_group);
    std::atomic<unsigned long long> wrong{0};
    const unsigned dim = 4;
    auto answer = [](float q0, uint32_t tag, unsigned j) { return (uint32_t)(q0 * 1000.f) + 31u * tag + j; };
    std::vector<std::thread> th;
    for (unsigned t = 0; t < n_threads; t++)
        th.emplace_back([&, t] {
            for (unsigned c = 0; c < calls_per_thread; c++) {
                const unsigned nq = 1 + (t + c) % 4, k = 1 + (t * 5 + c) % 7;
                std::vector<float> q((size_t)nq * dim);
                std::vector<uint32_t> tags(nq);                               // this call's tag: one word per query, the caller's own memory
                for (unsigned i = 0; i < nq; i++) { q[(size_t)i * dim] = (float)(t * 50 + c * 2 + i); tags[i] = 7u + t * 1000u + c * 10u + i; }
                std::vector<uint32_t> rows((size_t)nq * k, 7u), count(nq, 99u); std::vector<float> dist((size_t)nq * k, -1.f);
                char err[256]; err[0] = 0;
                const int rc = front.submit(
                    0, q.data(), nq, dim, k, rows.data(), dist.data(), count.data(), nullptr,
                    [&] {
                        std::this_thread::sleep_for(std::chrono::microseconds(pass_us));
                        for (unsigned i = 0; i < nq; i++) { count[i] = k; for (unsigned j = 0; j < k; j++) { rows[(size_t)i * k + j] = answer(q[(size_t)i * dim], tags[i], j); dist[(size_t)i * k + j] = (float)j; } }
                        return 0;
                    },
                    [&](qvco::Group& g, auto&) {
                        g.size_outputs(false);
                        std::vector<uint32_t> all(g.nq, 0u);                  // the members' tags side by side, in the order of the group's query block
                        for (uint32_t mi = 0; mi < g.n_mem; mi++) {
                            const qvco::Member& m = g.mbuf[mi];
                            const uint32_t* mt = static_cast<const uint32_t*>(m.tag);
                            if (!mt) { wrong.fetch_add(1000); continue; }
                            for (uint32_t i = 0; i < m.nq; i++) all[m.q0 + i] = mt[i];
                        }
                        std::this_thread::sleep_for(std::chrono::microseconds(pass_us + g.nq));
                        for (unsigned i = 0; i < g.nq; i++) {
                            g.count[i] = g.kmax;
                            for (unsigned j = 0; j < g.kmax; j++) { g.rows[(size_t)i * g.kmax + j] = answer(g.queries()[(size_t)i * dim], all[i], j); g.dist[(size_t)i * g.kmax + j] = (float)j; }
                        }
                        return 0;
                    },
                    [] { return ""; }, err, sizeof(err), tags.data());
                if (rc != 0) wrong.fetch_add(1000000);
                for (unsigned i = 0; i < nq; i++) {
                    if (count[i] != k) wrong.fetch_add(1);
                    for (unsigned j = 0; j < k; j++)
                        if (rows[(size_t)i * k + j] != answer(q[(size_t)i * dim], tags[i], j) || dist[(size_t)i * k + j] != (float)j) wrong.fetch_add(1);
                }
            }
        });
    for (auto& x : th) x.join();
    out[0] = front.stats.solo.load(); out[1] = front.stats.led.load(); out[2] = front.stats.rode.load(); out[3] = front.stats.groups.load();
    out[4] = front.stats.group_queries.load(); out[5] = wrong.load();
    return 0;
}

#ifdef TAG_HARNESS_MAIN
int main() {
    int bad = 0;
    for (int lanes : {1, 4})
        for (unsigned threads : {1u, 8u, 64u}) {
            unsigned long long o[6];
            coalesce_tag_harness(lanes, 64, threads, 25, 200, o);
            printf("callers %u lanes %d: solo %llu led %llu rode %llu groups %llu group_queries %llu wrong %llu\n", threads, lanes, o[0], o[1], o[2], o[3], o[4], o[5]);
            if (o[5] || o[0] + o[1] + o[2] != (unsigned long long)threads * 25) bad = 1;
        }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
#endif
