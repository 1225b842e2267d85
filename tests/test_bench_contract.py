"""The bench line's contract, checked on the round's recorded run (`python bench.py --full --steps 20 --warmup 5` on an MI355X):
profiles/rNN_bench_n1.json is the LINE bench.py printed (round 6 on: the short form of bench.compact_line), and
profiles/rNN_bench_n1_full.json the full record it wrote to bench_full.json (up to round 5 the line WAS the full record).
Checked: the fields the driver reads, the roofline and cpu_baseline objects and their arithmetic, and that the printed line is
short enough for the driver to keep whole (BENCH_r05.json: `parsed: null` -- the line had grown to 22.9 KB).
A plain run (no `--full`) measures the headline alone, and `--dump-outputs` writes what its last timed step returned."""
import glob, json, os, subprocess, sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def latest():
    """(full record, BASELINE.json)"""
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_bench_n1.json")))
    if not files:
        pytest.skip("no recorded bench line")
    full = files[-1].replace("_bench_n1.json", "_bench_n1_full.json")
    return json.load(open(full if os.path.exists(full) else files[-1])), json.load(open(os.path.join(ROOT, "BASELINE.json")))


def strict_loads(text):
    def refuse(name):
        raise ValueError("not strict JSON: " + name)
    return json.loads(text, parse_constant=refuse)


def test_printed_line_is_short_strict_json_with_roofline_and_cpu_baseline():
    """emit()'s own serialisation of the latest full record: < 6000 characters, strict JSON (no NaN / Infinity), the contract's keys,
    flat `roofline` / `cpu_baseline` objects, `legs` last."""
    import bench
    full, _ = latest()
    line = json.dumps(bench.compact_line(full), allow_nan=False)
    assert len(line) < bench.LINE_MAX <= 6000, len(line)
    d = strict_loads(line)
    assert list(d)[-1] == "legs"
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert "workload" in d["config"] and "model" not in d["config"]
    r, c = d["roofline"], d["cpu_baseline"]
    for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us", "launches", "active_problems_per_launch",
              "algorithmic_bytes_per_launch", "bound_measured"):
        assert k in r, k
    assert all(not isinstance(v, (dict, list)) for v in r.values())          # no per-launch arrays, no nested evidence
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-4)
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert d["legs"]["headline"][0] == pytest.approx(d["value"], rel=1e-3)
    # a record that outgrows the line sheds optional facts, never the contract
    fat = dict(full, launched_by="x" * 20000)
    assert len(json.dumps(bench.compact_line(fat))) < bench.LINE_MAX


def test_recorded_printed_line_is_the_short_form():
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_bench_n1.json")))
    if not files or not os.path.exists(files[-1].replace("_bench_n1.json", "_bench_n1_full.json")):
        pytest.skip("no round-6 record yet")
    text = open(files[-1]).read().strip()
    assert len(text) < 6000 and "\n" not in text
    d = strict_loads(text)
    assert list(d)[-1] == "legs" and d["roofline"]["frac"] > 0 and d["cpu_baseline"]["value"] > 0
    # what the boundary's callers get: host clouds (pinned / pageable), and a batch no step repeats
    for leg in ("headline_host_pinned", "headline_host_pageable", "headline_rotated"):
        assert d["legs"][leg][0] > 0, leg
    assert d["legs"]["headline_rotated"][0] > 0.5 * d["value"]


def test_recorded_line_keeps_the_contract():
    d, base = latest()
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f32" and "synthetic" in d["data"] and "workload" in d["config"] and "model" not in d["config"]
    assert d["unit"] == "scans/s" and isinstance(d["value"], float) and d["value"] > 0
    # value = converged scans of all steps / the timed region; ms_per_step the same region per step
    batch = d["config"]["batch_scans_per_step"]
    assert d["value"] == pytest.approx(d["scans_converged"] / (d["steps"] * d["ms_per_step"] * 1e-3), rel=1e-6)
    assert d["scans_total"] == d["steps"] * batch
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-9)
    # achieved = algorithmic bytes per launch / the kernel's average launch duration (HIP events on the context's stream)
    assert r["achieved"] == pytest.approx(r["algorithmic_bytes_per_launch"] / (r["avg_launch_us"] * 1e-6) / 1e9, rel=1e-6)
    assert r["traffic"] is None or r["traffic"] > 0
    assert r["bound_measured"] == "valu" and 0.0 < r["frac_unseeded_launches"] < r["frac"] < r["frac_seeded_launches"] < 1.0
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0
    # the companion legs: never `value`, each with its own roofline
    for leg in ("loop_closure", "stream", "slam", "f64", "slam_100k"):
        w = d["workloads"][leg]
        assert "error" not in w, (leg, w)
        assert w["value"] > 0 and "roofline" in w and 0.0 < w["roofline"]["frac"] < 1.0
    assert d["workloads"]["f64"]["value"] >= 0.45 * d["value"]           # the double path at about half the float rate (0.48-0.51 by run)
    assert len(d["workloads"]["stream"]["scans_per_s_each_pass"]) >= 3
    if "legs" in d:                                                      # (round 5 on)
        # the LAST key, compact: the driver keeps the tail of the line -- every leg's [value, roofline.frac] must be in it
        assert list(d.keys())[-1] == "legs" and len(json.dumps(d["legs"])) < 700
        for leg in ("headline", "f64", "stream", "slam", "slam_100k", "loop_closure"):
            v = d["legs"][leg]
            assert v[0] > 0 and 0.0 < v[1] < 1.0
        assert d["legs"]["headline"][0] == pytest.approx(d["value"], rel=1e-3)
        assert "bound_means" in r
        # the one-GPU proxy of the 8-GPU target (north_star: >= 3.5x on batched loop closing)
        sp = d["workloads"]["loop_closure"]["shard_proxy"]
        assert d["legs"]["loop_closure_predicted_speedup_8"] == pytest.approx(sp["predicted_speedup"]["8"])
        assert sp["predicted_speedup"]["8"] >= 3.5 and len(sp["per_world"]["8"]["shard_ms"]) == 8
        assert sp["predicted_speedup"]["2"] < sp["predicted_speedup"]["4"] < sp["predicted_speedup"]["8"]
        # the SLAM legs time passes AFTER a warm one, in one process
        assert d["workloads"]["slam_100k"]["slam"]["passes"] >= 4 and len(d["workloads"]["slam_100k"]["slam"]["pass_slam_s"]) >= 4


def test_metric_is_baselines():
    d, base = latest()
    assert base["metric"].split()[0].lower() in d["metric"].lower() or "scans/sec" in d["metric"]


def test_plain_run_measures_the_headline_alone():
    """Without --full the default workload skips every companion figure, the profile replay, the CPU baseline and the legs;
    --full brings them back, and its --no-* options still switch single ones off."""
    import bench
    extras = ("no_cpu_baseline", "no_profile", "no_fixed30", "no_host_input", "no_workloads")
    plain = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert plain.steps == 7 and plain.warmup == 2 and not plain.full and plain.dump_outputs is None
    assert all(getattr(plain, k) for k in extras)
    full = bench.parse_args(["--full", "--steps", "7"])
    assert not any(getattr(full, k) for k in extras)
    assert bench.parse_args(["--full", "--no-workloads"]).no_workloads and not bench.parse_args(["--full", "--no-workloads"]).no_profile
    # the named workloads are explicit requests: unchanged
    assert not bench.parse_args(["--workload", "stream"]).no_profile
    for bad in (["--steps", "0"], ["--workload", "f64", "--dump-outputs", "x"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_dump_outputs_writes_every_returned_array_in_float64(tmp_path):
    import numpy as np
    import bench
    B = 3
    T = np.stack([np.eye(4) * (b + 1) for b in range(B)])
    st = [dict(status=0, iterations=5 + b, converged=True, max_iter_reached=False, overlap=0.5, residual=1e-3 * b, trim_limit=0.25,
               n_kept=100 + b, n_finite=120, cov=np.full((6, 6), float(b))) for b in range(B)]
    bench.dump_outputs(str(tmp_path / "out"), T, st)
    names = sorted(p.name for p in (tmp_path / "out").iterdir())
    assert names == sorted(["T.npy"] + [k + ".npy" for k in bench.STATS_FIELDS])
    got = {n[:-4]: np.load(tmp_path / "out" / n) for n in names}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["T"], T) and got["cov"].shape == (B, 6, 6) and got["cov"][2, 0, 0] == 2.0
    assert got["iterations"].tolist() == [5.0, 6.0, 7.0] and got["converged"].tolist() == [1.0, 1.0, 1.0]


@pytest.mark.gpu
def test_plain_run_line_and_outputs_repeat(tmp_path):
    """Two plain runs with the same (small) arguments: the contract's keys, `steps` timed steps, nothing but the headline measured,
    and the same outputs bit for bit."""
    import numpy as np
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--n-scan", "5000", "--n-map", "50000", "--queries", "4", "--batch", "8"]
    outs = []
    for k in range(2):
        d_out = tmp_path / f"run{k}"
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(d_out)], cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        d = strict_loads([l for l in p.stdout.splitlines() if l.strip()][-1])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in d, key
        assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "scans/s" and d["dtype"] == "f32" and d["higher_is_better"] is True
        assert d["scans_total"] == 3 * 8 and d["value"] == pytest.approx(d["scans_converged"] / (3 * d["ms_per_step"] * 1e-3), rel=1e-3)
        assert d["roofline"] is None and d["cpu_baseline"] is None and d["legs"]["f64"] is None
        outs.append({f.name: np.load(f) for f in sorted(d_out.iterdir())})
    assert outs[0]["T.npy"].shape == (8, 4, 4) and outs[0]["cov.npy"].shape == (8, 6, 6)
    assert sorted(outs[0]) == sorted(outs[1])
    for name, a in outs[0].items():
        assert a.dtype == np.float64 and np.array_equal(a, outs[1][name], equal_nan=True), name
