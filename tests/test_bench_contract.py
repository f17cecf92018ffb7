"""The bench line's contract (task statement, measurement section): the line committed under profiles/ -- produced by `python bench.py` on
the MI355X box -- carries every required field with sane values, and bench.py still parses and keeps its documented defaults."""
import ast
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


import pytest


@pytest.mark.parametrize("name", ["r01_bench_turbo_b32.json", "r02_bench_turbo_b32.json", "r03_bench_turbo_b32.json"])
def test_committed_bench_line_has_every_contract_field(name):
    line = open(os.path.join(ROOT, "profiles", name)).read().strip().splitlines()[-1]
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "audio-sec/s" and d["n_gpus"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["dtype"] == "bf16" and d["data"] == "synthetic"          # BASELINE.md publishes no number for this metric
    assert "workload" in d["config"] and "large-v3-turbo" in d["config"]["workload"] and "model" not in d["config"]
    assert abs(d["value"] - 32 * 30.0 / (d["ms_per_step"] * 1e-3)) <= 0.01 * d["value"]           # value = clips x 30 s / time per pass
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["traffic"] is None or 0.9 * r["bytes_per_launch"] <= r["traffic"] <= 1.2 * r["bytes_per_launch"]   # PMC bytes ~ algorithmic bytes
    if name.startswith("r02"):
        # the roofline's launch time comes from strictly serial passes in the same process, reported beside the pipelined `value`
        e = r["execution"]
        assert e["replicas"] == 1 and e["value"] <= d["value"] and abs(e["value"] - 32 * 30.0 / (e["ms_per_step"] * 1e-3)) <= 0.01 * e["value"]
        assert abs(r["achieved"] - r["bytes_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e9) <= 0.01 * r["achieved"]
        assert d["config"]["exchange"] == "none" and "config0" in d and d["config0"]["gpu"]["generated_tokens"] > 0
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] == "port" and c["unit"] == d["unit"] and c["cores"] >= 1 and c["value"] > 0


def test_bench_defaults_and_syntax():
    src = open(os.path.join(ROOT, "bench.py")).read()
    tree = ast.parse(src)
    defaults = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument" and node.args and isinstance(node.args[0], ast.Constant):
            for kw in node.keywords:
                if kw.arg == "default" and isinstance(kw.value, ast.Constant):
                    defaults[node.args[0].value] = kw.value.value
    assert defaults["--gpus"] == 1 and defaults["--batch"] == 32 and defaults["--model"] == "large-v3-turbo" and defaults["--dtype"] == "bf16"
    assert defaults["--steps"] >= 1 and defaults["--warmup"] >= 0


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_bench_full_and_dump_outputs_options():
    """--full (off by default) gates everything beyond the headline figure; --dump-outputs DIR takes a directory."""
    tree = ast.parse(open(os.path.join(ROOT, "bench.py")).read())
    opts = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument" and node.args and isinstance(node.args[0], ast.Constant):
            opts[node.args[0].value] = {kw.arg: getattr(kw.value, "value", None) for kw in node.keywords}
    assert opts["--full"].get("action") == "store_true" and "default" not in opts["--full"]
    assert "--dump-outputs" in opts and opts["--dump-outputs"].get("default") is None and "action" not in opts["--dump-outputs"]


def test_bench_dump_outputs_files(tmp_path):
    """pass_outputs masks token slots past each clip's count and splits the float outputs into finite values + a non-finite kind array
    (lossless: NaN / -inf / +inf are told apart); dump_outputs writes float32 (float64 kept) .npy files, refuses non-finite entries and
    more than 64 MB in all."""
    import numpy as np
    bench = _bench_module()
    toks = np.arange(12, dtype=np.int32).reshape(2, 6) + 50000
    outs = bench.pass_outputs(toks, np.array([3, 6], np.int32), np.array([-0.5, -1.25], np.float32), np.array([0.1, 0.2], np.float32))
    paths = bench.dump_outputs(str(tmp_path / "out"), outs)
    assert sorted(os.path.basename(p) for p in paths) == ["avg_logprob.npy", "avg_logprob_nonfinite.npy", "n_tokens.npy", "no_speech_prob.npy",
                                                        "no_speech_prob_nonfinite.npy", "tokens.npy"]
    assert np.load(tmp_path / "out" / "avg_logprob.npy").tolist() == [-0.5, -1.25]
    assert np.load(tmp_path / "out" / "avg_logprob_nonfinite.npy").tolist() == [0.0, 0.0]
    odd = bench.pass_outputs(toks, np.array([3, 6], np.int32), np.array([np.nan, -1.25, -np.inf, np.inf], np.float32), np.zeros(2, np.float32))
    assert odd["avg_logprob"].tolist() == [0.0, -1.25, 0.0, 0.0] and odd["avg_logprob_nonfinite"].tolist() == [1, 0, 2, 3]
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "nan"), {"x": np.array([0.0, np.nan], np.float32)})
    assert not (tmp_path / "nan").exists()
    t = np.load(tmp_path / "out" / "tokens.npy")
    assert t.dtype == np.float32 and t.shape == (2, 6)
    np.testing.assert_array_equal(t, [[50000, 50001, 50002, -1, -1, -1], [50006, 50007, 50008, 50009, 50010, 50011]])
    assert np.load(tmp_path / "out" / "n_tokens.npy").tolist() == [3.0, 6.0]
    bench.dump_outputs(str(tmp_path / "f64"), {"x": np.zeros(3, np.float64)})
    assert np.load(tmp_path / "f64" / "x.npy").dtype == np.float64
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros((64 << 20) // 4 + 1, np.float32)})
    assert not (tmp_path / "big").exists()


@pytest.mark.gpu
def test_plain_bench_run_prints_headline_and_dumps_outputs(tmp_path):
    """A plain run (no --full) on a small workload: exactly one JSON line with the headline fields and none of the --full figures, `steps`
    timed passes, and --dump-outputs writes the last timed pass's outputs, consistent with one another."""
    import json
    import subprocess
    import sys
    import numpy as np
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--model", "tiny.en",
                        "--batch", "2", "--max-new-tokens", "8", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert k in d, k
    for k in ("roofline", "stages", "codec", "lm", "config0", "cpu_baseline"):
        assert k not in d, k
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "audio-sec/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 2 * 30.0 / (d["ms_per_step"] * 1e-3)) <= 0.01 * d["value"]
    toks, n = np.load(out / "tokens.npy"), np.load(out / "n_tokens.npy")
    avg, nsp = np.load(out / "avg_logprob.npy"), np.load(out / "no_speech_prob.npy")
    assert toks.dtype == n.dtype == avg.dtype == nsp.dtype == np.float32
    assert toks.shape == (2, 448) and n.shape == avg.shape == nsp.shape == (2,)
    assert np.all(n > 0) and np.all(n <= 448)
    for b in range(2):
        k = int(n[b])
        assert np.all(toks[b, :k] >= 0) and np.all(toks[b, k:] == -1)
    avg_k, nsp_k = np.load(out / "avg_logprob_nonfinite.npy"), np.load(out / "no_speech_prob_nonfinite.npy")
    assert np.isfinite(avg).all() and np.isfinite(nsp).all()
    # avg_logprob is NaN (kind 1) where a decode step had every token masked (synthetic weights; tests/test_fullsize_gpu.py), else <= 0
    assert np.all(np.isin(avg_k, [0, 1])) and np.all(avg[avg_k == 0] <= 0) and np.all(avg[avg_k == 1] == 0)
    assert np.all(nsp_k == 0) and np.all((nsp >= 0) & (nsp <= 1))
