"""CPU-side checks of the bulk overwrite (qv_index_update_rows, qv_index_update_rows_device, qv_sharded_update_rows): the header and the
Python prototypes, the host rule that settles duplicates and cuts a list into tiles (qv_update_rows_plan: pure host arithmetic), the
null-argument answers, and the host mirror's weak references — quiver_amd/csrc/host/qvhost.cpp linked against a stand-in for libqv that
has neither bulk entry point must link and reuse tombstoned slots through the loop of qv_index_update, with the same slots, clean under
AddressSanitizer + UBSan (a stand-alone program: nothing is loaded into the interpreter)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qv_index_update_rows", "qv_index_update_rows_device", "qv_sharded_update_rows")


def test_header_declares_them_and_the_prototypes_cover_them():
    from quiver_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qv.h")).read(), flags=re.S)
    for name, args in (("qv_index_update_rows", r"qv_index\* idx, const uint32_t\* rows, uint32_t n, const float\* vecs"),
                       ("qv_index_update_rows_device", r"qv_index\* idx, const uint32_t\* rows, uint32_t n, const float\* d_vecs, void\* stream"),
                       ("qv_sharded_update_rows", r"qv_sharded\* s, const uint32_t\* global_rows, uint32_t n, const float\* vecs")):
        assert re.search(r"\bint %s\(%s\s*\);" % (name, args), src), name
        assert name in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES["qv_index_update_rows"][1]) == 4 and len(_lib.PROTOTYPES["qv_index_update_rows_device"][1]) == 5
    assert len(_lib.PROTOTYPES["qv_sharded_update_rows"][1]) == 4
    assert re.search(r"#define QV_DEBUG_PLANE8 7\b", src) and re.search(r"#define QV_DEBUG_RRES8\s+8\b", src)
    assert (_lib.QV_DEBUG_PLANE8, _lib.QV_DEBUG_RRES8) == (7, 8)
    assert "#define QV_ABI_VERSION 4" in src
    import quiver_amd
    assert quiver_amd.DeviceIndex.DEBUG_READ["plane8"] == (7, np.uint8) and quiver_amd.DeviceIndex.DEBUG_READ["rres8"] == (8, np.float32)


def test_null_arguments_are_refused_before_any_device_is_needed():
    import quiver_amd
    from quiver_amd._lib import check, lib
    rows = np.zeros(1, np.uint32); vec = np.zeros(4, np.float32)
    for call in (lambda: lib().qv_index_update_rows(None, rows.ctypes.data, 1, vec.ctypes.data),
                 lambda: lib().qv_index_update_rows(None, None, 0, None),                       # the handle is looked at before the count
                 lambda: lib().qv_index_update_rows_device(None, rows.ctypes.data, 1, vec.ctypes.data, None),
                 lambda: lib().qv_sharded_update_rows(None, rows.ctypes.data, 1, vec.ctypes.data)):
        with pytest.raises(quiver_amd.QvError, match="is null") as e:
            check(call())
        assert e.value.code == -1


def plan(rows):
    from quiver_amd._lib import check, lib
    import ctypes as C
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    n = rows.size
    ro, so, tf, to = (np.full(n + 1, 0xDEADBEEF, np.uint32) for _ in range(4))
    m, t = C.c_uint32(77), C.c_uint32(77)
    check(lib().qv_update_rows_plan(rows.ctypes.data if n else None, n, ro.ctypes.data, so.ctypes.data, tf.ctypes.data, to.ctypes.data, C.byref(m), C.byref(t)))
    m, t = m.value, t.value
    assert (ro[m:] == 0xDEADBEEF).all() and (so[m:] == 0xDEADBEEF).all() and (to[t:] == 0xDEADBEEF).all() and (tf[t + 1:] == 0xDEADBEEF).all()
    return ro[:m].tolist(), so[:m].tolist(), tf[:t + 1].tolist(), to[:t].tolist()


def plan_by_definition(rows):
    """the rule restated: the last entry of every row, by ascending row; a tile's entries are those with row // 64 == tile"""
    last = {}
    for i, r in enumerate(rows):
        last[int(r)] = i
    rs = sorted(last)
    tiles = sorted({r // 64 for r in rs})
    first = [next(i for i, r in enumerate(rs) if r // 64 == t) for t in tiles] + [len(rs)]
    return rs, [last[r] for r in rs], first, tiles


def test_plan_rule_on_its_edge_cases():
    assert plan([]) == ([], [], [0], [])                                              # an empty list: no entry, no tile
    assert plan([9, 9, 9, 9]) == ([9], [3], [0, 1], [0])                              # all equal: the LAST entry survives
    assert plan([200, 130, 129, 64, 63, 0]) == ([0, 63, 64, 129, 130, 200], [5, 4, 3, 2, 1, 0], [0, 2, 3, 5, 6], [0, 1, 2, 3])   # descending
    assert plan([63, 64]) == ([63, 64], [0, 1], [0, 1, 2], [0, 1])                    # neighbours either side of a tile boundary
    assert plan([127, 128, 64, 127, 191, 192, 64]) == ([64, 127, 128, 191, 192], [6, 3, 1, 4, 5], [0, 2, 4, 5], [1, 2, 3])
    assert plan([4294967295, 0, 4294967232]) == ([0, 4294967232, 4294967295], [1, 2, 0], [0, 1, 3], [0, 67108863])   # the top of the row range
    whole = list(range(128, 192))
    assert plan(whole[::-1]) == (whole, list(range(63, -1, -1)), [0, 64], [2])         # every row of one tile
    rng = np.random.default_rng(5)
    for n, top in ((1, 10), (200, 357), (5000, 3000), (5000, 4_000_000)):
        rows = rng.integers(0, top, n)
        assert plan(rows) == plan_by_definition(rows), (n, top)


def test_plan_refuses_null_outputs():
    import quiver_amd
    from quiver_amd._lib import check, lib
    import ctypes as C
    a = np.zeros(4, np.uint32); c = C.c_uint32(0)
    with pytest.raises(quiver_amd.QvError) as e:
        check(lib().qv_update_rows_plan(a.ctypes.data, 1, None, a.ctypes.data, a.ctypes.data, a.ctypes.data, C.byref(c), C.byref(c)))
    assert e.value.code == -1


MAIN = r"""
// the host mirror against a libqv stand-in WITHOUT qv_index_update_rows / qv_sharded_update_rows: both addresses are null, and
// RowStore::update_many is the loop of update() — InsertMany reuses tombstoned slots as the per-row loop did: popped from the back, in id order
#include <cstdio>
#include <string>
#include <vector>
#include "quiver_amd/csrc/host/qvhost.h"
using namespace quiver;
extern "C" {
int qv_index_update_rows(qv_index*, const uint32_t*, uint32_t, const float*) __attribute__((weak));
int qv_sharded_update_rows(qv_sharded*, const uint32_t*, uint32_t, const float*) __attribute__((weak));
}
static int bad = 0;
#define CHECK(c, ...) do { if (!(c)) { bad++; fprintf(stderr, "FAILED line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)
static std::vector<float> vec(int i, uint32_t d) { std::vector<float> v(d, 0.f); v[0] = 1.f; v[1] = 0.001f * (float)i; return v; }
int main() {
    CHECK(qv_index_update_rows == nullptr && qv_sharded_update_rows == nullptr, "the stand-in must not have the bulk entry points");
    const uint32_t D = 8;
    ExactIndex x(QV_COSINE, Placement());
    std::vector<std::string> ids; std::vector<float> pk;
    for (int i = 0; i < 12; i++) { ids.push_back("a" + std::to_string(i)); auto v = vec(i, D); pk.insert(pk.end(), v.begin(), v.end()); }
    Error e = x.InsertMany(ids, pk.data(), D);                         // the first creates the index, the rest are one add: id i -> row i
    CHECK(e.empty(), "first batch: %s", e.c_str());
    for (int i : {3, 9, 5, 0}) CHECK(x.Delete("a" + std::to_string(i)).empty(), "delete");   // free slots, in order: 3 9 5 0
    // six new ids, all the SAME vector: a search's ties are broken by row, so the answer shows which slot each id got
    std::vector<std::string> ids2; std::vector<float> pk2;
    for (int i = 0; i < 6; i++) { ids2.push_back("n" + std::to_string(i)); auto v = vec(100, D); pk2.insert(pk2.end(), v.begin(), v.end()); }
    e = x.InsertMany(ids2, pk2.data(), D);
    CHECK(e.empty(), "second batch: %s", e.c_str());
    CHECK(x.DeviceRows() == 14, "%u device rows, expected 12 + 2", x.DeviceRows());
    CHECK(x.Size() == 14, "size");
    std::vector<BasicSearchResult> out;
    auto q = vec(100, D);
    e = x.Search(q.data(), D, 6, &out);
    CHECK(e.empty() && out.size() == 6, "search: %s", e.c_str());
    // n0 -> 0, n1 -> 5, n2 -> 9, n3 -> 3 (popped from the back), n4 -> 12, n5 -> 13 (appended): by row 0 3 5 9 12 13
    const char* want[6] = {"n0", "n3", "n1", "n2", "n4", "n5"};
    for (size_t i = 0; i < out.size() && i < 6; i++) CHECK(out[i].id == want[i], "result %zu is %s, expected %s", i, out[i].id.c_str(), want[i]);
    e = x.InsertMany({"n0"}, pk2.data(), D);
    CHECK(!e.empty(), "an existing id must be refused");
    e = x.InsertMany({"z0", "z1"}, pk2.data(), D + 1);
    CHECK(!e.empty(), "a wrong dimension must be refused");
    CHECK(x.Size() == 14 && x.DeviceRows() == 14, "a refused batch changed the index");
    if (bad) { fprintf(stderr, "%d checks failed\n", bad); return 1; }
    printf("ok: slots reused through the per-row path, %u device rows\n", x.DeviceRows());
    return 0;
}
"""


def test_host_mirror_links_without_the_entry_points_and_keeps_the_slots(tmp_path):
    """the weak references: tests/c/qv_stub.cpp provides neither entry point (the construction of tests/test_graph_remove_cpu.py)"""
    stub = open(os.path.join(ROOT, "tests", "c", "qv_stub.cpp")).read()
    assert "update_rows" not in stub
    main = tmp_path / "host_update_many_main.cpp"
    main.write_text(MAIN)
    exe = str(tmp_path / "host_update_many_asan")
    objs = []
    for src in ("qv_oracle.c", "qv_oracle_hnsw.c"):
        o = str(tmp_path / (src + ".o"))
        subprocess.run(["gcc", "-std=c11", "-fno-fast-math", "-ffp-contract=off", "-fno-tree-vectorize", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-g", "-O1", "-fno-omit-frame-pointer", "-c", "-o", o, os.path.join(ROOT, "oracle", src)],
                       check=True, capture_output=True, text=True)
        objs.append(o)
    subprocess.run(["g++", "-std=c++17", "-pthread", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                    "-fno-omit-frame-pointer", "-I", ROOT, "-o", exe, str(main),
                    os.path.join(ROOT, "tests", "c", "qv_stub.cpp"), os.path.join(ROOT, "quiver_amd", "csrc", "host", "qvhost.cpp")] + objs + ["-lm"],
                   check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:exitcode=66:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("ok:") and "per-row path" in p.stdout, p.stdout
