"""Row sets without a GPU: the boundary (symbols, header, argument checks), the tagged members of the front that lets filtered callers
share passes (tests/c/coalesce_tag_harness.cpp, also under the thread sanitizer), and a static guard on the compiled row-set kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "quiver_amd", "csrc")
SYMBOLS = ("qv_rowset_create", "qv_rowset_set_rows", "qv_rowset_count", "qv_rowset_destroy",
           "qv_index_search_rowsets", "qv_index_search_rowsets_device", "qv_index_rowset_coalesce_stats")


def test_library_exports_the_row_set_symbols_and_python_binds_them():
    from quiver_amd import _lib
    handle = C.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(handle, s), s + " is not exported"
        assert s in _lib.PROTOTYPES, s + " has no Python prototype"
    assert _lib.lib().qv_abi_version() == 4                       # additions only


def test_header_with_the_row_set_calls_compiles_as_c99_and_cpp11(tmp_path):
    body = ('#include "qv.h"\n'
            "int f(qv_index* idx, const float* q, uint32_t* r, float* d, uint32_t* c, void* s) {\n"
            "    qv_rowset* rs = 0; const qv_rowset* sets[2]; uint64_t st[8];\n"
            "    int rc = qv_rowset_create(&rs, idx, 0);\n"
            "    rc += qv_rowset_set_rows(rs, r, 1, 1); sets[0] = rs; sets[1] = 0;\n"
            "    rc += qv_index_search_rowsets(idx, q, 2, 10, sets, r, d, c);\n"
            "    rc += qv_index_search_rowsets_device(idx, q, 2, 10, sets, r, d, s);\n"
            "    rc += qv_index_rowset_coalesce_stats(idx, st) + (int)qv_rowset_count(rs);\n"
            "    qv_rowset_destroy(rs);\n"
            "    return rc + QV_ABI_VERSION - 4;\n}\n")
    c = tmp_path / "t.c"; c.write_text(body)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "t.o")])
    cpp = tmp_path / "t.cpp"; cpp.write_text(body)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(cpp), "-o", str(tmp_path / "t2.o")])


def test_null_arguments_are_errors_with_a_message_not_crashes():
    from quiver_amd import _lib
    L = _lib.lib()
    rs = C.c_void_p()
    assert L.qv_rowset_create(C.byref(rs), None, None) == _lib.QV_ERR_INVALID_ARG
    assert L.qv_last_error().decode() == "index is null" and not rs.value
    assert L.qv_rowset_create(None, None, None) == _lib.QV_ERR_INVALID_ARG
    assert L.qv_rowset_set_rows(None, None, 0, 1) == _lib.QV_ERR_INVALID_ARG and "row set is null" in L.qv_last_error().decode()
    assert L.qv_rowset_count(None) == 0
    L.qv_rowset_destroy(None)
    cnt = (C.c_uint32 * 1)()
    assert L.qv_index_search_rowsets(None, None, 1, 1, None, None, None, cnt) == _lib.QV_ERR_INVALID_ARG
    assert L.qv_last_error().decode() == "index is null"
    assert L.qv_index_search_rowsets_device(None, None, 1, 1, None, None, None, None) == _lib.QV_ERR_INVALID_ARG
    assert L.qv_index_rowset_coalesce_stats(None, None) == _lib.QV_ERR_INVALID_ARG


def test_host_mirror_does_not_call_the_row_set_entry_points():
    """tests/c/qv_stub.cpp (the sanitizer builds' stand-in for libqv) does not provide them"""
    txt = open(os.path.join(CSRC, "host", "qvhost.cpp")).read()
    assert "qv_rowset" not in txt and "search_rowsets" not in txt


# ---- the front's tagged members ---------------------------------------------------------------------------------------------

HARNESS = os.path.join(ROOT, "tests", "c", "coalesce_tag_harness.cpp")


@pytest.fixture(scope="module")
def tag_harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("coalesce_tag") / "libcoalesce_tag_harness.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wall", "-Werror", "-o", str(so), HARNESS])
    lib = C.CDLL(str(so))
    lib.coalesce_tag_harness.restype = C.c_int
    lib.coalesce_tag_harness.argtypes = [C.c_int] + [C.c_uint] * 4 + [C.POINTER(C.c_ulonglong)]

    def run(lanes, max_group, threads, calls, pass_us):
        out = (C.c_ulonglong * 6)()
        assert lib.coalesce_tag_harness(lanes, max_group, threads, calls, pass_us, out) == 0
        return dict(zip(("solo", "led", "rode", "groups", "group_queries", "wrong"), [int(x) for x in out]))
    return run


@pytest.mark.parametrize("lanes,threads", [(1, 1), (1, 8), (1, 64), (4, 64), (2, 300)])
def test_every_member_receives_the_tag_it_submitted(tag_harness, lanes, threads):
    r = tag_harness(lanes, 64, threads, 40, 300)
    assert r["wrong"] == 0, r
    assert r["solo"] + r["led"] + r["rode"] == threads * 40
    if threads >= 64 and lanes == 1:
        assert r["rode"] > 0 and r["group_queries"] > r["groups"] >= 1, r       # members did share passes: the tags travelled in groups


def test_tagged_members_are_clean_under_the_thread_sanitizer(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "tag_tsan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=thread", "-DTAG_HARNESS_MAIN", "-Wall", "-Werror", "-o", exe, HARNESS])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1"))
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-6000:]
    assert "ThreadSanitizer" not in p.stderr and "FAILED" not in p.stdout and "callers 64 lanes 4" in p.stdout


# ---- the compiled kernels ------------------------------------------------------------------------------------------------------

def _asm(src, out):
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-o", out, src],
                   check=True, capture_output=True, text=True, cwd=os.path.dirname(src))
    return open(out).read()


def _loads_in_flight(body):
    """outstanding row-chunk loads along the instruction stream: +1 per global_load_dwordx4, clipped by every s_waitcnt vmcnt(N)
    (tests/test_isa_guard.py's count)"""
    best = out = 0
    for line in body.split("\n"):
        t = line.strip()
        if t.startswith("global_load_dwordx4"):
            out += 1; best = max(best, out)
        elif t.startswith("s_waitcnt"):
            w = re.search(r"vmcnt\((\d+)\)", t)
            if w:
                out = min(out, int(w.group(1)))
    return best


# scalar stores and scalar atomics: never, in any kernel of this tree (vector stores or plain C++ instead)
BANNED = [a + b for a, b in (("s_", "store_dword"), ("s_buffer_", "store"), ("s_scratch_", "store"), ("s_", "atomic_"), ("s_buffer_", "atomic"),
                             ("s_dcache_", "wb"), ("s_dcache_", "discard"))]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_row_set_scan_loops_keep_the_parents_loads_in_flight_and_do_not_spill(tmp_path):
    """For every metric the whole-tile row-set pass (8 queries, each with its set) has no scratch traffic anywhere between its first and
    its last row-chunk load, and reaches at least as many row-chunk loads in flight as k_flat_scan_mq<M, 4, 8, true> — the kernel it is
    the per-query-set form of — shows in the same compile.  Neither file holds a scalar store or a scalar atomic."""
    rs = _asm(os.path.join(CSRC, "qv_rowset.hip"), str(tmp_path / "rowset.s"))
    sc = _asm(os.path.join(CSRC, "qv_scan.hip"), str(tmp_path / "scan.s"))
    for metric in range(9):
        parent = re.search(r"^_ZN2qv14k_flat_scan_mqILi%dELi4ELi8ELb1EEEv\w*:[^\n]*\n(.*?)\n\s+s_endpgm" % metric, sc, re.S | re.M)
        assert parent, "k_flat_scan_mq<%d,4,8,true> not found" % metric
        bar = _loads_in_flight(parent.group(1))
        assert bar >= 1
        for qb in (4, 8) + ((16,) if metric in (0, 1, 3, 4, 8) else ()):      # 16 per pass: the float64-accumulating metrics, as in the parent
            m = re.search(r"^_ZN2qv16k_rowset_scan_mqILi%dELi4ELi%dEEEv\w*:[^\n]*\n(.*?)\n\s+s_endpgm" % (metric, qb), rs, re.S | re.M)
            assert m, "k_rowset_scan_mq<%d,4,%d> not found" % (metric, qb)
            lines = [l.strip() for l in m.group(1).split("\n")]
            ld = [i for i, l in enumerate(lines) if l.startswith("global_load_dwordx4")]
            assert ld, "k_rowset_scan_mq<%d,4,%d>: no row-chunk loads" % (metric, qb)
            loop = lines[ld[0]: ld[-1] + 1]
            assert not any(l.startswith("scratch_") for l in loop), "k_rowset_scan_mq<%d,4,%d>: spill traffic in the tile loop" % (metric, qb)
            if qb == 8:
                got = _loads_in_flight(m.group(1))
                assert got >= bar, "k_rowset_scan_mq<%d,4,8>: %d row-chunk loads in flight, the parent has %d" % (metric, got, bar)
    for metric in (0, 1, 3, 4, 8):                              # the tile-over-eight-waves form: the metrics whose chain can be split
        for qb in (4, 8):
            m = re.search(r"^_ZN2qv22k_rowset_scan_split_mqILi%dELi%dEEEv\w*:[^\n]*\n(.*?)\n\s+s_endpgm" % (metric, qb), rs, re.S | re.M)
            assert m, "k_rowset_scan_split_mq<%d,%d> not found" % (metric, qb)
            assert not any(l.strip().startswith("scratch_") for l in m.group(1).split("\n")), "k_rowset_scan_split_mq<%d,%d> spills" % (metric, qb)
    for name, text in (("qv_rowset.hip", rs), ("qv_scan.hip", sc)):
        low = text.lower()
        for word in BANNED:
            assert word not in low, "%s compiles to %s" % (name, word)
    for name in ("qv_rowset.hip", "qv_scan.hip"):
        low = open(os.path.join(CSRC, name)).read().lower()
        for word in BANNED:
            assert word not in low, "%s names %s" % (name, word)
