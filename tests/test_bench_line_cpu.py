"""The bench contract's stdout line must survive the driver's channel: one line, <= 4 KB, valid
JSON, the contract's keys present (a 21 KB line was not parsed).  The full record
goes to a side file.  Canned input: round 4's committed full record (profiles/)."""
import copy
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
            "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline",
            "cpu_baseline", "extra_file")


def _canned():
    return json.load(open(os.path.join(ROOT, "profiles", "r4_bench_n1_final.json")))


def _check(line):
    assert "\n" not in line
    assert len(line.encode()) < 4096, len(line)
    j = json.loads(line)
    for k in REQUIRED:
        assert k in j, k
    assert isinstance(j["config"], dict) and "workload" in j["config"]
    assert "model" not in j["config"]
    r = j["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    c = j["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    return j


def test_line_of_the_round4_record_fits_and_parses():
    import bench
    full = _canned()
    assert len(json.dumps(full)) > 20000  # the record that broke the channel
    j = _check(bench.compact_line(full, "bench_extra.json"))
    assert j["value"] == bench._r(full["value"])
    assert j["dtype"] == "fp16"
    assert j["roofline_update"]["frac"] == bench._r(full["roofline_update"]["frac"])
    assert "roofline_uniform" in j and "roofline_index" in j


def test_line_of_an_eight_rank_record_fits():
    import bench
    full = _canned()
    full["n_gpus"] = 8
    full.pop("cpu_baseline")
    full["cpu_baseline"] = {"value": 1.0, "unit": "samples/s", "cores": 1, "kind": "reference",
                            "sample": "x" * 2000}
    rank = {"rank": 0, "slots": 4, "table_rows": 10 ** 8, "stage_us": full["stage_us_per_step"],
            "exchange": {"payload": "rows", "note": "y" * 500}, "new_keys_per_step": 1.5}
    full["per_rank"] = [copy.deepcopy(rank) for _ in range(8)]
    strong = copy.deepcopy({k: v for k, v in full.items() if k not in ("extra", "strong")})
    full["strong"] = strong
    j = _check(bench.compact_line(full, "/some/long/path/" + "d" * 100 + "/bench_extra.json"))
    assert "per_rank" not in j


def test_pathological_record_still_fits():
    import bench
    full = _canned()
    full["config"]["workload"] = "w" * 5000
    full["extra"] = {f"leg{i}": {"ms_per_step": 1.0} for i in range(400)}
    _check(bench.compact_line(full, "bench_extra.json"))


def test_emit_writes_the_file_and_prints_one_line(tmp_path):
    code = ("import json, sys; sys.path.insert(0, %r); import bench; "
            "bench.emit(json.load(open(%r)), %r)" % (
                ROOT, os.path.join(ROOT, "profiles", "r4_bench_n1_final.json"),
                str(tmp_path / "x.json")))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    lines = p.stdout.strip().split("\n")
    assert len(lines) == 1
    j = _check(lines[0])
    assert json.load(open(j["extra_file"]))["extra"].keys() == _canned()["extra"].keys()


def test_line_of_a_plain_run_record():
    """a plain run (no --full) records the headline and the configuration only: the line still
    carries the contract's headline keys and no figure of a run it did not make"""
    import bench
    full = _canned()
    for k in ("roofline", "roofline_update", "roofline_index", "roofline_uniform", "roofline_fp32",
              "stage_us_per_step", "stage_us_per_step_no_new_keys", "embedding_ms_per_step",
              "cpu_baseline", "extra"):
        full.pop(k, None)
    j = json.loads(bench.compact_line(full, "bench_extra.json"))
    assert (j["metric"], j["unit"], j["higher_is_better"], j["dtype"]) == (
        full["metric"], full["unit"], True, "fp16")
    assert (j["value"], j["ms_per_step"]) == (bench._r(full["value"]), bench._r(full["ms_per_step"]))
    for k in ("roofline", "roofline_update", "roofline_index", "cpu_baseline", "extra_summary"):
        assert k not in j, k


def test_plain_run_and_full_options():
    """--full turns on what a plain run leaves out; legs and scaling named explicitly still run"""
    import bench
    plain = ["--gpus", "1", "--steps", "20", "--warmup", "5"]
    a = bench.parse_args(plain)
    assert (a.full, a.extra, a.scaling, a.cpu_baseline) == (False, "none", "weak", False)
    a = bench.parse_args(plain + ["--full"])
    assert (a.full, a.extra, a.scaling, a.cpu_baseline) == (True, "auto", "both", True)
    a = bench.parse_args(plain + ["--full", "--extra", "none", "--no-cpu-baseline"])
    assert (a.extra, a.cpu_baseline) == ("none", False)
    a = bench.parse_args(plain + ["--extra", "uniform", "--scaling", "both"])
    assert (a.full, a.extra, a.scaling, a.cpu_baseline) == (False, "uniform", "both", False)
