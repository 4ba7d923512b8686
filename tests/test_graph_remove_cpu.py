"""CPU-side checks of the in-place graph edits (qv_graph_remove, qv_graph_export_lists): the null-argument answers, the
plain-C view of the two entry points, and the host mirror's weak references to them — quiver_amd/csrc/host/qvhost.cpp linked
against a stand-in for libqv that has neither must link, run Delete / Insert / Search on the old path, and be clean under
AddressSanitizer + UBSan (a stand-alone program: nothing is loaded into the interpreter)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_graph_answers_and_their_wording():
    import quiver_amd
    from quiver_amd._lib import check, lib
    import numpy as np
    nodes = np.zeros(1, np.uint32); levels = np.zeros(1, np.int32); deg = np.zeros(1, np.uint32); links = np.zeros(64, np.uint32)
    with pytest.raises(quiver_amd.QvError, match="graph is null") as e:
        check(lib().qv_graph_remove(None, nodes.ctypes.data, 1))
    assert e.value.code == -1
    with pytest.raises(quiver_amd.QvError, match="graph is null") as e:
        check(lib().qv_graph_remove(None, None, 0))                   # the handle is looked at before the count
    assert e.value.code == -1
    with pytest.raises(quiver_amd.QvError, match="graph is null") as e:
        check(lib().qv_graph_export_lists(None, nodes.ctypes.data, levels.ctypes.data, 1, deg.ctypes.data, links.ctypes.data))
    assert e.value.code == -1


def test_plain_c_smoke_links_and_answers(tmp_path):
    import quiver_amd
    exe = str(tmp_path / "graph_remove_smoke")
    libdir = os.path.join(ROOT, "quiver_amd", "lib")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "graph_remove_smoke.c"),
                    "-L", libdir, "-lqv", "-lm", "-Wl,-rpath," + libdir, "-o", exe], check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    if quiver_amd.lib().qv_device_count() <= 0:
        assert "no device" in p.stdout
    else:
        assert p.stdout.splitlines()[-1].startswith("ok:"), p.stdout


def test_host_mirror_without_the_entry_points_runs_clean_under_asan(tmp_path):
    """the weak references: tests/c/qv_stub.cpp provides neither entry point, so Delete and Insert take the path they always took"""
    exe = str(tmp_path / "host_graph_edit_asan")
    objs = []
    for src in ("qv_oracle.c", "qv_oracle_hnsw.c"):
        o = str(tmp_path / (src + ".o"))
        subprocess.run(["gcc", "-std=c11", "-fno-fast-math", "-ffp-contract=off", "-fno-tree-vectorize", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-g", "-O1", "-fno-omit-frame-pointer", "-c", "-o", o, os.path.join(ROOT, "oracle", src)],
                       check=True, capture_output=True, text=True)
        objs.append(o)
    subprocess.run(["g++", "-std=c++17", "-pthread", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "c", "host_graph_edit_main.cpp"),
                    os.path.join(ROOT, "tests", "c", "qv_stub.cpp"), os.path.join(ROOT, "quiver_amd", "csrc", "host", "qvhost.cpp")] + objs + ["-lm"],
                   check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:exitcode=66:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("ok:") and "fallback path" in p.stdout, p.stdout
