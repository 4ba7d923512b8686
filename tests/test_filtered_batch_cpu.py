"""The routing rule of filtered batches (qv_batched_applies_filtered: the dispatch's own rule, asked on the host without an index or a device), the
environment default of its mode, and the argument checks that need no device."""
import os
import subprocess
import sys

import pytest

import quiver_amd
from quiver_amd import QvError, _lib, batched_applies_filtered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHED_METRICS = ("cosine", "dot", "l2", "l2sq")
OTHER_METRICS = ("l1", "cosine_f32", "l2_f32", "dot_f32", "l2sq_f64")
ROWS = (1_000, 40_003, 165_037, 299_999, 300_000, 1_000_000, 10_000_000)
DIMS = (96, 128, 768, 3072)
NQS = (1, 8, 9, 16, 40, 64, 256, 300, 8192)
KS = (1, 10, 15, 16, 64, 65, 200)
MODES = ("auto", "always", "never")


def test_never_takes_nothing_and_no_mode_takes_what_the_batched_path_does_not():
    for metric in BATCHED_METRICS + OTHER_METRICS:
        for rows in ROWS:
            for dim in DIMS:
                for nq in NQS:
                    for k in KS:
                        for mode in MODES:
                            for filt in ("auto", "bf16x1", "bf16x3", "fp32", "off"):
                                got = batched_applies_filtered(metric, dim, rows, nq, k, filt, mode)
                                where = (metric, rows, dim, nq, k, mode, filt)
                                if mode == "never" or nq < 9 or k > 64 or metric in OTHER_METRICS or filt == "off":
                                    assert not got, where
                                if mode == "auto" and rows < 300_000:
                                    assert not got, where
                                if got:                                                # whatever takes a shape, "always" takes it too
                                    assert batched_applies_filtered(metric, dim, rows, nq, k, filt, "always"), where


def test_always_takes_the_shapes_of_the_batched_path():
    # the shapes tests/test_gpu_filtered_batch.py runs: the one-term and three-term filters from 9 queries, the fp32 filter from 32
    for metric in BATCHED_METRICS:
        for rows, dim in ((40_003, 768), (40_003, 96), (140_003, 128), (300_003, 128), (1_000_000, 768)):
            for nq in (40, 100, 256, 300):
                for k in (1, 10, 15, 16, 64):
                    for filt in ("auto", "bf16x1", "bf16x3", "fp32"):
                        assert batched_applies_filtered(metric, dim, rows, nq, k, filt, "always"), (metric, rows, dim, nq, k, filt)
    assert batched_applies_filtered("cosine", 768, 1_000_000, 9, 10, "bf16x1", "always")
    assert not batched_applies_filtered("cosine", 768, 1_000_000, 9, 10, "fp32", "always")
    assert not batched_applies_filtered("cosine", 768, 20_000, 64, 10, "auto", "always")      # a corpus the batched path leaves to the scans


def test_monotone_in_the_queries_not_known_sparse():
    for mode in MODES:
        for rows in (40_003, 300_000, 1_000_000):
            for nq in (9, 40, 256):
                prev = False
                for n in range(0, nq + 1):
                    got = batched_applies_filtered("cosine", 768, rows, nq, 10, "auto", mode, n)
                    assert got or not prev, (mode, rows, nq, n)                     # once taken, taken for every larger count
                    if n < 9:
                        assert not got, (mode, rows, nq, n)
                    prev = got
                # a count above nq is read as nq
                assert batched_applies_filtered("cosine", 768, rows, nq, 10, "auto", mode, nq + 50) == batched_applies_filtered("cosine", 768, rows, nq, 10, "auto", mode, nq)
    assert batched_applies_filtered("cosine", 768, 1_000_000, 40, 10, "auto", "always", 9)
    assert not batched_applies_filtered("cosine", 768, 1_000_000, 40, 10, "auto", "always", 8)


def test_argument_checks_without_a_device():
    lib = _lib.lib()
    for bad_mode in (-1, 3):
        with pytest.raises(QvError) as e:
            batched_applies_filtered("cosine", 768, 1_000_000, 40, 10, "auto", bad_mode)
        assert e.value.code == _lib.QV_ERR_INVALID_ARG
    for bad_filter in (-1, 5):
        with pytest.raises(QvError) as e:
            batched_applies_filtered("cosine", 768, 1_000_000, 40, 10, bad_filter, "always")
        assert e.value.code == _lib.QV_ERR_INVALID_ARG
    import ctypes as C
    assert lib.qv_index_set_filtered_batch(None, 1, 0xFFFFFFFF) == _lib.QV_ERR_INVALID_ARG
    assert lib.qv_index_filtered_batch_stats(None, (C.c_uint64 * 4)()) == _lib.QV_ERR_INVALID_ARG
    a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert lib.qv_batched_sample_plan(None, 40, 10, C.byref(a), C.byref(b), C.byref(c)) == _lib.QV_ERR_INVALID_ARG
    assert (_lib.QV_FILTERED_BATCH_AUTO, _lib.QV_FILTERED_BATCH_ALWAYS, _lib.QV_FILTERED_BATCH_NEVER) == (0, 1, 2)
    assert quiver_amd.DeviceIndex.FILTERED_BATCH == {"auto": 0, "always": 1, "never": 2}


@pytest.mark.parametrize("env,want", [("", (False, True, False)), ("1", (True, True, False)), ("2", (False, True, False))])
def test_environment_sets_the_default_mode(env, want):
    """QV_FILTERED_BATCH is read once per process: a child per value.  40 003 rows: "auto" itself takes nothing there, so what the automatic
    mode answers is the environment's default; an explicit "always" / "never" does not look at it."""
    code = ("import quiver_amd as q; print([int(q.batched_applies_filtered('cosine', 768, 40003, 40, 10, 'auto', m)) for m in ('auto', 'always', 'never')])")
    e = dict(os.environ)
    e.pop("QV_FILTERED_BATCH", None)
    if env:
        e["QV_FILTERED_BATCH"] = env
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, check=True).stdout
    assert out.strip() == str([int(x) for x in want]), out
