"""Batched prosody micro-benchmark: ops.apply_prosody_rows on the device
(csrc/prosody.hip) versus the host NumPy path, B in {1, 64}, 5 s rows at
22.05 kHz, the modes benchmark's prosody setting (rate=65, volume=80,
pitch=55 -> speed 3.75, volume 0.8, pitch 1.05: resample + two WSOLA
passes + gain).

Each timed call is bracketed by device synchronisation outside the timed
kernels (host clock around work that ends in a synchronise); the median
of --calls timed calls after --warmup untimed ones is reported, one JSON
line per (backend, B).  The host path at B=64 takes seconds per call, so
it is timed --host-calls times only.  Needs a GPU: there is no fallback.

    python tools/tools_bench_prosody.py [--calls 20] [--warmup 3]
"""
import argparse
import json
import statistics
import sys
import time

sys.path.insert(0, ".")

import numpy as np
import torch

from sonata_amd import ops
from sonata_amd.synth.synthesizer import AudioOutputConfig

SR = 22050
SECONDS = 5.0


def rows(B: int) -> torch.Tensor:
    """Voiced-like rows (harmonics of a gliding pitch + noise), seeded."""
    n = int(SR * SECONDS)
    t = np.arange(n) / SR
    out = np.empty((B, n), dtype=np.float32)
    for b in range(B):
        rng = np.random.default_rng(b)
        f0 = 100.0 + 60.0 * rng.random() + 20.0 * np.sin(2 * np.pi * 0.5 * t)
        ph = 2 * np.pi * np.cumsum(f0) / SR
        s = sum(np.sin(h * ph) / h for h in range(1, 9))
        out[b] = 0.2 * s + 0.01 * rng.standard_normal(n)
    return torch.from_numpy(out)


def timed(fn, calls: int, warmup: int, sync) -> list:
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1000.0)
    return ts


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=2,
                    help="timed host calls at B=64 (seconds each)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU path"
    speed, volume, pitch = AudioOutputConfig(
        rate=65, volume=80, pitch=55).prosody_triple()
    for B in (1, 64):
        x = rows(B)
        lens = [x.shape[1]] * B
        kw = dict(speed=[speed] * B, volume=[volume] * B, pitch=[pitch] * B)
        xd = x.to("cuda:0")
        y_dev, n_dev = ops.apply_prosody_rows(xd, lens, SR, **kw)
        y_host, n_host = ops.apply_prosody_rows(x, lens, SR, **kw)
        assert n_dev.tolist() == n_host.tolist()
        for name, inp, calls, warm, sync in (
                ("device", xd, args.calls, args.warmup,
                 torch.cuda.synchronize),
                ("host", x, args.calls if B == 1 else args.host_calls,
                 1 if B == 1 else 0, lambda: None)):
            ts = timed(lambda: ops.apply_prosody_rows(inp, lens, SR, **kw),
                       calls, warm, sync)
            print(json.dumps({
                "op": "apply_prosody_rows", "backend": name, "B": B,
                "row_seconds": SECONDS, "sample_rate": SR,
                "speed": speed, "volume": volume, "pitch": pitch,
                "calls": calls, "median_ms": round(statistics.median(ts), 3),
                "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
                "out_samples": int(n_dev[0]),
            }), flush=True)


if __name__ == "__main__":
    main()
