"""Driver-contract rehearsal: bench.py runs single-rank and under
torch.distributed.run (the exact launch the driver uses for N>1),
printing one valid JSON line from rank 0."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_json(line: str, world: int):
    d = json.loads(line)
    assert d["metric"] == "audio_seconds_per_second"
    assert d["value"] > 0
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["config"]["parallelism"] == f"dp{world}"
    assert d["data"] == "synthetic"
    return d


def _run_single(steps: int, dump_dir, *extra):
    r = subprocess.run(
        [sys.executable, "bench.py", "--steps", str(steps), "--warmup", "1",
         "--batch", "2", "--seq-len", "64", "--quality", "x_low",
         "--dump-outputs", str(dump_dir), *extra],
        cwd=ROOT, capture_output=True, text=True, timeout=550)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().splitlines()[-1]


@pytest.fixture(scope="module")
def single_rank_run(tmp_path_factory):
    """One plain single-rank run, shared: (result line, dump directory)."""
    d = tmp_path_factory.mktemp("bench_dump")
    return _run_single(2, d), d


@pytest.mark.timeout(600)
def test_bench_single_rank_cpu(single_rank_run):
    line, _ = single_rank_run
    d = _check_json(line, 1)
    assert d["steps"] == 2
    assert d["ms_per_step"] > 0
    for key in ("unit", "dtype"):
        assert key in d


@pytest.mark.timeout(600)
def test_bench_dump_outputs_reproducible(single_rank_run, tmp_path):
    """--dump-outputs writes the last timed step's results as float32
    .npy; a second run with the same arguments (here also under --full)
    writes the same arrays."""
    import numpy as np

    line, first = single_rank_run
    sample_rate = json.loads(line)["config"]["sample_rate"]
    _check_json(_run_single(2, tmp_path, "--full"), 1)
    names = sorted(os.listdir(first))
    assert names == ["audio.npy", "audio_lengths.npy"]
    assert sorted(os.listdir(tmp_path)) == names
    total = 0
    for n in names:
        a = np.load(os.path.join(first, n))
        b = np.load(os.path.join(tmp_path, n))
        assert a.dtype == np.float32 and a.size > 0
        assert np.isfinite(a).all()
        assert a.shape == b.shape and np.array_equal(a, b), n
        total += os.path.getsize(os.path.join(first, n))
    assert total <= 64 * 10**6
    lengths = np.load(os.path.join(first, "audio_lengths.npy"))
    audio = np.load(os.path.join(first, "audio.npy"))
    assert lengths.shape == (2,) and (lengths > 0).all()
    assert audio.shape[0] == 2 and audio.shape[-1] >= lengths.max()
    # the dumped step is one of the timed ones: its audio is what the
    # throughput figure counted
    d = json.loads(line)
    counted = d["value"] * d["ms_per_step"] / 1000.0
    assert abs(lengths.sum() / sample_rate - counted) <= 0.01 * counted


@pytest.mark.timeout(600)
def test_bench_torchrun_world2_cpu():
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29541", "bench.py", "--gpus", "2",
         "--steps", "2", "--warmup", "1", "--batch", "2",
         "--seq-len", "64", "--quality", "x_low"],
        cwd=ROOT, capture_output=True, text=True, timeout=550)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1  # only rank 0 prints
    _check_json(lines[-1], 2)
