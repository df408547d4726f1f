"""The driver parses the LAST stdout line of ``bench.py`` out of a bounded tail (~8.7 KB).  Round 5's line had grown
to 26 KB and the round went unmeasured; these tests pin the contract: whatever ``measure`` returns, ``main`` prints one
line under ``bench.MAX_LINE`` bytes that carries the contract's fields, ``roofline`` and ``cpu_baseline``."""

from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
            "roofline", "cpu_baseline")


def fat_record(n_configs=80):
    """a full record shaped like round 5's, with more and longer entries than any real run has produced"""
    long = "x" * 700
    cfgs = {f"hot_case_{k}": {"config": long, "ms_device": 0.0123456789, "frac": 0.5123456789, "generated_kernels_us": {long[:60] + str(j): 1.0 for j in range(6)}}
            for k in range(n_configs)}
    for k in bench._BASELINE_CONFIGS:
        cfgs[k] = {"config": long, "frac": 0.4123456789123, "kernel_frac": 0.6123456789123, "kernel": long}
    return {
        "metric": "graph evals/sec (logp+grad, N=1e6 fp64)", "value": 5234.123456789, "unit": "graph evals/sec", "n_gpus": 1, "steps": 20, "warmup": 5,
        "warmup_effective": 800, "ms_per_step": 0.19123456789, "value_executor_level": 5400.123456, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": long, "mode": "hipGraph plan", "value_is": long, "function": {"compile_s": 1.0}, "parallelism": "replicas x1"},
        "roofline": {"bound": "hbm", "kernel": long, "achieved": 6221.123456789, "peak": 8000.0, "unit": "GB/s", "frac": 0.7776543210987, "traffic": 1044553598.72,
                     "traffic_source": long, "detail": {"kernel_ms": 0.16712345678, "kernel_ms_top8": {long[:50] + str(j): 0.1 for j in range(8)}}},
        "cpu_baseline": {"value": 10.0880072, "unit": "graph evals/sec", "cores": 256, "kind": "reference-cvm", "sample": long, "ms_per_eval": 99.1276,
                         "parity_err_over_bound": 0.0794210265, "port": {"value": 3.0, "sample": long}},
        "configs": cfgs,
    }


def test_compact_is_bounded_and_complete():
    line = bench.compact(fat_record(), "gpurun_out/bench_detail.json")
    text = json.dumps(line)
    assert len(text) < bench.MAX_LINE, len(text)
    for k in CONTRACT:
        assert k in line, k
    rf = line["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert rf["traffic"] is not None
    cpu = line["cpu_baseline"]
    assert cpu["kind"] == "reference-cvm" and cpu["cores"] == 256 and cpu["value"] > 0 and cpu["sample"]
    assert set(line["configs"]) == set(bench._BASELINE_CONFIGS)  # one fraction each, no hot_* sweep
    assert all(isinstance(v, float) for v in line["configs"].values())
    assert "model" not in line["config"]


def test_compact_without_baseline_or_configs():
    rec = fat_record()
    rec["cpu_baseline"] = None
    rec["configs"] = None
    line = bench.compact(rec)
    assert line["cpu_baseline"] is None and line["configs"] == {}
    assert len(json.dumps(line)) < bench.MAX_LINE


def test_main_prints_one_short_last_line(monkeypatch, capsys, tmp_path):
    monkeypatch.setattr(bench, "measure", lambda args: fat_record(200))
    detail = tmp_path / "detail.json"
    bench.main(["--detail", str(detail)])
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1  # stdout carries the JSON line and nothing else
    last = lines[-1]
    assert len(last) < 6000
    rec = json.loads(last)
    assert rec["roofline"]["frac"] > 0 and rec["cpu_baseline"]["value"] > 0
    assert rec["steps"] == 20 and rec["warmup"] == 5 and rec["n_gpus"] == 1
    # the full record (hot_* sweep, per-kernel tables) is in the side file
    full = json.load(open(detail))
    assert len(full["configs"]) >= 200 and "detail" in full["roofline"]


def test_non_zero_ranks_print_nothing(monkeypatch, capsys):
    monkeypatch.setattr(bench, "measure", lambda args: None)
    bench.main([])
    assert capsys.readouterr().out == ""


def test_default_run_skips_the_sweep():
    args = bench.parse_args([])
    assert args.gpus == 1 and not args.hotpath
    assert args.steps * 0.2e-3 < 60  # default K at ~0.2 ms per evaluation: seconds, not minutes


def lean_record():
    """what ``measure`` returns for a plain run: the headline fields, none of the ``--full`` measurements"""
    rec = fat_record(0)
    for k in ("value_executor_level", "roofline", "cpu_baseline", "configs"):
        del rec[k]
    rec["full"] = False
    return rec


def test_full_is_an_option_and_off_by_default():
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"]).full is False
    assert bench.parse_args(["--full"]).full is True
    assert bench.parse_args(["--hotpath"]).full is True  # the sweep is one of the measurements --full runs


def test_plain_run_prints_the_headline_and_writes_no_side_file(monkeypatch, capsys, tmp_path):
    monkeypatch.setattr(bench, "measure", lambda args: lean_record())
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))  # where a detail file would go by default
    bench.main(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["metric"] == "graph evals/sec (logp+grad, N=1e6 fp64)" and rec["unit"] == "graph evals/sec"
    assert rec["value"] == 5234.123457 and rec["ms_per_step"] == 0.191235 and rec["higher_is_better"] is True and rec["dtype"] == "f64"
    assert rec["full"] is False and rec["roofline"] is None and rec["cpu_baseline"] is None and rec["configs"] == {}
    assert "value_executor_level" not in rec and "detail" not in rec
    assert not list(tmp_path.iterdir())
    # the same record with --detail: the side file is written where asked
    bench.main(["--detail", str(tmp_path / "d.json")])
    assert json.load(open(tmp_path / "d.json"))["full"] is False


def test_plain_run_returns_before_any_secondary_measurement():
    """``measure`` leaves through the ``not args.full`` return before the first line of the secondary section"""
    src = open(os.path.join(ROOT, "bench.py")).read()
    body = src[src.index("def measure(args):"):src.index("MAX_LINE =")]
    leave = body.index("if not args.full:")
    for later in ("elapsed_exec", "exe.profile_nodes(", "live_pmc_traffic(", "pmc_c4_current.json", "cpu_baseline(graph", "bench_configs.measure(", "r7_mfma_pmc.json"):
        assert body.index(later) > leave, later
    assert body.index("dump_outputs(last") < leave and body.index('"ms_per_step"') < leave


def test_dump_outputs_writes_one_npy_per_output(tmp_path):
    import numpy as np

    outs = [np.float64(-1.5), np.arange(128.0), np.array(0.25), np.ones(128, np.float32), np.zeros(128), np.array(3.0)]
    paths = bench.dump_outputs(outs, bench.C4_OUTPUT_NAMES, str(tmp_path / "d"))
    assert [os.path.basename(p) for p in paths] == [f"{n}.npy" for n in bench.C4_OUTPUT_NAMES]
    for a, p in zip(outs, paths):
        b = np.load(p)
        assert b.dtype == (np.float32 if np.asarray(a).dtype == np.float32 else np.float64)
        np.testing.assert_array_equal(b, a)


def test_dump_outputs_refuses_more_than_the_limit(tmp_path, monkeypatch):
    import numpy as np
    import pytest

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1024)
    with pytest.raises(ValueError):
        bench.dump_outputs([np.zeros(1024)], ("x",), str(tmp_path))
    assert not list(tmp_path.iterdir())


def test_steps_sets_the_timed_steps_and_must_be_positive():
    import pytest

    a = bench.parse_args(["--steps", "7", "--warmup", "3", "--dump-outputs", "out"])
    assert a.steps == 7 and a.warmup == 3 and a.dump_outputs == "out"
    assert bench.parse_args([]).dump_outputs is None
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
