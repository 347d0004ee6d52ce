"""bench.py's multi-GPU contract on the CPU (gloo, world size 2), with only the
device work mocked (tests/bench_mock.py): `--gpus N` starts N ranks itself and
rank 0 prints one line with n_gpus N and every rank's kernel time; asking for
more GPUs than are visible, or a --gpus that disagrees with the launcher's
WORLD_SIZE, fails loudly and prints no line."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--docs", "300", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-host", "--no-sub"]


def _run(gpus, visible, extra_env=None, args=ARGS):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(CLD_BENCH_MOCK=os.path.join(ROOT, "tests", "bench_mock.py"), CLD_BENCH_MOCK_GPUS=str(visible),
               OMP_NUM_THREADS="1")
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus)] + list(args),
                          capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)


def _lines(stdout):
    return [json.loads(x) for x in stdout.splitlines() if x.startswith("{")]


def test_gpus_2_runs_two_ranks_and_one_line():
    r = _run(2, 2)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _lines(r.stdout)
    assert len(lines) == 1, r.stdout
    d = lines[0]
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "document shards, 2 rank(s)"
    pr = d["per_rank"]
    assert sorted(p["rank"] for p in pr) == [0, 1] and all(p["docs"] == 300 for p in pr)
    assert all(p["wave_ms"] > 0 for p in pr)
    # whole-job rate: both ranks' documents over the slowest rank's time
    slowest = max(p["elapsed_s"] for p in pr)
    assert abs(d["value"] - 2 * 300 * 2 / slowest) / d["value"] < 1e-6
    assert d["ms_per_step"] == slowest / 2 * 1e3


def test_more_gpus_than_visible_fails_loudly():
    r = _run(2, 1)
    assert r.returncode != 0 and not _lines(r.stdout)
    assert "GPU(s) are visible" in r.stderr


def test_gpus_must_match_launcher_world_size():
    r = _run(2, 2, {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and not _lines(r.stdout)
    assert "WORLD_SIZE" in r.stderr


def test_single_gpu_line():
    r = _run(1, 1)
    assert r.returncode == 0, r.stderr[-3000:]
    (d,) = _lines(r.stdout)
    assert d["n_gpus"] == 1 and d["per_rank"] is None


PLAIN = ["--docs", "300", "--steps", "2", "--warmup", "1"]
FIELDS = {"lang3": (np.float32, (300, 3)), "summary_lang": (np.float32, (300,)), "percent3": (np.float32, (300, 3)),
          "is_reliable": (np.float32, (300,)), "text_bytes": (np.float32, (300,)), "normalized3": (np.float64, (300, 3))}


def test_plain_run_times_the_headline_only_and_dumps_its_outputs(tmp_path, oracle):
    a, b = tmp_path / "a", tmp_path / "b"
    r = _run(1, 1, args=PLAIN + ["--dump-outputs", str(a)])
    assert r.returncode == 0, r.stderr[-3000:]
    (d,) = _lines(r.stdout)
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["dtype"] == "u8" and d["higher_is_better"] is True
    assert abs(d["value"] - 300 / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-6
    assert d["cpu_baseline"] is None and d["c3"] is None and d["host_path"] is None
    # what a caller of the timed path receives: the result records of this seeded batch
    import corpus
    buf, offs = corpus.c2(300, seed=corpus.SEEDS["c2"])
    want = oracle.detect_batch(buf, offs, threads=1)
    assert sorted(p.name for p in a.iterdir()) == sorted(f + ".npy" for f in FIELDS)
    for f, (dt, shape) in FIELDS.items():
        got = np.load(a / (f + ".npy"))
        assert got.dtype == dt and got.shape == shape, f
        assert np.array_equal(got, want[f].astype(dt)), f
    # the same arguments score the same bytes
    r = _run(1, 1, args=PLAIN + ["--dump-outputs", str(b)])
    assert r.returncode == 0, r.stderr[-3000:]
    for f in FIELDS:
        assert (a / (f + ".npy")).read_bytes() == (b / (f + ".npy")).read_bytes(), f


def test_full_run_adds_the_cpu_baseline():
    r = _run(1, 1, args=PLAIN + ["--full", "--cpu-seconds", "0.2", "--no-host", "--no-sub"])
    assert r.returncode == 0, r.stderr[-3000:]
    (d,) = _lines(r.stdout)
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["gpu_bit_exact_on_sample"] is True


def test_dump_outputs_samples_a_large_batch(tmp_path, monkeypatch):
    import bench
    import cld_amd
    out = np.zeros(1000, dtype=cld_amd.RESULT_DTYPE)
    out["text_bytes"] = np.arange(1000)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 60 * 100)      # 60 bytes per document as dumped
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out)
    tb = np.load(tmp_path / "a" / "text_bytes.npy")
    assert tb.shape == (100,) and np.all(np.diff(tb) > 0)        # a sample, in document order
    assert np.array_equal(tb, np.load(tmp_path / "b" / "text_bytes.npy"))
    assert sum(p.stat().st_size - 128 for p in (tmp_path / "a").iterdir()) == 60 * 100
