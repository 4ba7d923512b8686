"""bench.py's contract line: one strict-JSON line the driver can keep whole (it records the last 8 KB of stdout), with the
headline, `roofline` and `cpu_baseline` on it whatever the extra configs measured; the full record goes to a sidecar."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

RECORDED = os.path.join(ROOT, "profiles", "r02_bench_n1.jsonl")     # full records of round 2's runs (26 KB each)


RECORDED_R03 = os.path.join(ROOT, "profiles", "r03_bench_full.json")   # round 3's full record (the sidecar of its 3.7 KB line)


def _records():
    return [json.loads(l) for l in open(RECORDED).read().strip().split("\n")] + [json.load(open(RECORDED_R03))]


@pytest.mark.parametrize("i", range(8))
def test_line_fits_and_parses(i):
    rec = _records()[i]
    text = bench.compact_line(rec, "gpurun_out/bench_full.json")
    assert "\n" not in text and len(text.encode()) < 4096
    line = json.loads(text, parse_constant=lambda c: pytest.fail("non-strict JSON constant " + c))
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"):
        assert key in line
    assert abs(line["value"] - rec["value"]) <= 1e-5 * rec["value"]
    assert line["config"]["workload"].startswith("flat cosine scan")
    rf = line["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-4 and "traffic" in rf
    cb = line["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["value"] > 0 and cb["sample"]
    assert set(cb["others"]) == {"faithful_one_query_per_core", "optimised_scan_not_the_reference"}
    also = line["also"]
    assert also["flat_1Mx768"]["frac"] > 0 and "b256x1Mx768_mfma" in also
    assert any(k.startswith("hnsw_1M") for k in also)


def test_extras_are_shed_before_the_headline():
    rec = _records()[-1]
    rec["also"] = {("batched_256x10Mx768_extra_%d" % i): dict(rec["also"]["batched_256x1Mx768_mfma"]) for i in range(200)}
    rec["config"]["sharding"] = "x" * 5000
    text = bench.compact_line(rec, None)
    assert len(text) <= bench.MAX_LINE
    line = json.loads(text)
    assert line["roofline"]["frac"] > 0 and line["cpu_baseline"]["value"] > 0 and line["also"]["in_sidecar_only"] > 0


def test_nan_never_reaches_the_line():
    rec = _records()[-1]
    rec["also"]["flat_1Mx768_single_query"]["hbm_frac"] = float("nan")
    json.loads(bench.compact_line(rec, None), parse_constant=lambda c: pytest.fail(c))


def test_emit_writes_sidecar_and_one_line(tmp_path):
    side = tmp_path / "full.json"
    code = ("import json,sys; sys.path.insert(0, %r); import bench; "
            "bench.emit(json.loads(open(%r).read().strip().split('\\n')[-1]))" % (ROOT, RECORDED))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, QV_BENCH_SIDECAR=str(side)), check=True)
    assert p.stdout.count("\n") == 1 and len(p.stdout) < 4096
    assert json.loads(p.stdout)["full_record"]
    full = json.loads(side.read_text())
    assert "hnsw_1Mx768_maxlevel1_structured" in full["also"] and len(side.read_text()) > 20000


def test_eight_gpus_and_maximum_length_strings_still_emit_the_headline():
    """the budget can be exceeded by the fixed part alone (8 per-GPU roofline entries, a long runtime string, every CPU leg):
    the line sheds extras instead of raising after the whole benchmark has run"""
    rec = _records()[-1]
    rec["n_gpus"] = 8
    rec["roofline"]["per_gpu"] = [{"rank": g, "rows": 1250000, "scan_kernel_ms": 0.5512345, "hbm_frac": 0.87123} for g in range(8)]
    rec["config"].update({k: "y" * 400 for k in ("runtime", "sharding", "exchange", "arithmetic", "workload", "device")})
    rec["cpu_baseline"]["sample"] = "z" * 3000
    rec["cpu_baseline"]["others"] = {("leg_%d" % i): {"value": 1.0 / 3, "cores": 64} for i in range(120)}
    text = bench.compact_line(rec, "gpurun_out/" + "p" * 300)
    assert len(text) <= bench.MAX_LINE
    line = json.loads(text)
    assert line["value"] == pytest.approx(rec["value"], rel=1e-5) and line["n_gpus"] == 8 and line["roofline"]["frac"] > 0
    assert line["cpu_baseline"]["value"] > 0


def test_membership_check_catches_a_skipped_row():
    """bench.py's verified_against_oracle: a result that misses a better row fails; results beyond the checked rows are ignored"""
    import numpy as np
    from tests import _oracle as O
    rows = O.gen_rows(1, 0, 5000, 32)
    q = O.gen_rows(2, 0, 1, 32)[0]
    er, ed = O.exact_search(0, rows, q, 10)
    assert bench.membership_check(O, 0, q, rows[:3000], 0, er.astype(np.int64), ed)
    assert bench.membership_check(O, 0, q, rows[100:2000], 100, er.astype(np.int64), ed)
    er2, ed2 = O.exact_search(0, rows, q, 11)
    assert not bench.membership_check(O, 0, q, rows, 0, er2[1:].astype(np.int64), ed2[1:])          # the best row is missing
    bad = ed.copy(); bad[3] = np.nextafter(bad[3], np.float32(2))
    assert not bench.membership_check(O, 0, q, rows, 0, er.astype(np.int64), bad)                    # a distance one ulp off


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_writes_float_arrays(tmp_path):
    import numpy as np
    rows = np.array([4294967295, 0, 9999999], dtype=np.uint32)
    dist = np.array([0.25, 0.5, 1.0], dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "out"), rows, dist)
    r, d = np.load(tmp_path / "out" / "rows.npy"), np.load(tmp_path / "out" / "distances.npy")
    assert r.dtype == np.float64 and d.dtype == np.float32
    assert r.astype(np.uint64).tolist() == rows.tolist() and np.array_equal(d, dist)


def _run_bench(args, tmp_path):
    env = dict(os.environ, QV_BENCH_SIDECAR=str(tmp_path / "full.json"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.count("\n") == 1
    return json.loads(p.stdout)


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_the_last_step(tmp_path):
    """a plain run: exactly --steps timed steps, the headline fields, no extras; --dump-outputs holds the last timed step's top-k,
    which is the oracle's exact top-k of that step's query (step i searches query i % 256 of the seeded pool)"""
    import numpy as np
    from tests import _oracle as O
    n, dim, k, steps, warmup = 30000, 768, 10, 5, 2
    line = _run_bench(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--rows", str(n), "--dump-outputs", str(tmp_path / "d")], tmp_path)
    assert line["steps"] == steps and line["warmup"] == warmup and line["full"] is False
    assert line["metric"] == "flat_cosine_qps_recall_1.0" and line["unit"] == "queries/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["value"] > 0 and line["ms_per_step"] == pytest.approx(1e3 / line["value"], rel=1e-3)
    assert line["roofline"] is None and line["cpu_baseline"] is None and "also" not in line and "full_record" not in line
    assert not (tmp_path / "full.json").exists()
    rows, dist = np.load(tmp_path / "d" / "rows.npy"), np.load(tmp_path / "d" / "distances.npy")
    assert rows.dtype == np.float64 and dist.dtype == np.float32 and rows.shape == (k,) and dist.shape == (k,)
    q = O.gen_rows(bench.QUERY_SEED, 0, 256, dim)[(warmup + steps - 1) % 256]
    er, ed = O.exact_search(0, O.gen_rows(bench.CORPUS_SEED, 0, n, dim), q, k)
    assert rows.astype(np.int64).tolist() == er.tolist() and np.array_equal(dist.view(np.uint32), ed.view(np.uint32))


@pytest.mark.gpu
def test_full_run_keeps_the_oracle_check_and_the_roofline(tmp_path):
    line = _run_bench(["--gpus", "1", "--steps", "4", "--warmup", "1", "--rows", "30000", "--full", "--no-also", "--no-cpu-baseline"], tmp_path)
    assert line["full"] is True and line["verified_against_oracle"] is True
    assert line["roofline"]["bound"] == "hbm" and line["roofline"]["kernel_ms"] > 0 and line["full_record"]
    assert json.loads((tmp_path / "full.json").read_text())["steps"] == 4
