"""Device PCM benchmark: the float -> wire-bytes finish of a synthesized
batch, on the device (csrc/pcm.hip, int16 copy) versus on the host (f32
copy, audio.samples.to_i16_bytes per row).

  op   B in {1, 64}, 5 s rows at 22.05 kHz, bf16 [B, 1, T] as the decoder
       leaves them.  From the device tensor to a list of `bytes`.
  e2e  one batch of 64 sentences on the medium random voice, from phonemes
       to wire bytes, three ways in turn, --rounds times:
         float  speak_batch + Audio.as_wave_bytes (the call sequence of the
                commit before this one; the only one run when the tree has
                no speak_batch_pcm, so the same file times that commit)
         pcm0   speak_batch_pcm under SONATA_DEVICE_PCM=0
         pcm1   speak_batch_pcm under SONATA_DEVICE_PCM=1

Host clock around work that ends in a synchronise (the host copy); the
median of the timed calls after warm-up, one JSON line per measurement.
The three e2e ways must give the same bytes, or the run fails.  Needs a
GPU: there is no fallback.

    python tools/tools_bench_pcm.py [--section op|e2e|all] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, ".")

import numpy as np
import torch

from sonata_amd.audio.samples import to_i16_bytes

SR = 22050
SECONDS = 5.0
DEV = "cuda:0"


def emit(**kw) -> None:
    print(json.dumps(kw), flush=True)


def stats(ts) -> dict:
    return {"calls": len(ts), "median_ms": round(statistics.median(ts), 3),
            "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def timed(fn, calls: int, warmup: int) -> list:
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1000.0)
    return ts


def bench_op(calls: int, warmup: int) -> None:
    from sonata_amd import ops

    n = int(SR * SECONDS)
    for B in (1, 64):
        rng = np.random.default_rng(B)
        x = torch.from_numpy(
            (0.3 * rng.standard_normal((B, 1, n))).astype(np.float32)
        ).to(DEV).to(torch.bfloat16)
        lens = [n - 37 * b for b in range(B)]
        lens_d = torch.tensor(lens, device=DEV)

        def host():
            a = x.float().cpu().numpy()
            ln = lens_d.cpu().numpy()
            return [to_i16_bytes(a[b, 0, : int(ln[b])]) for b in range(B)]

        def device():
            pcm, out = ops.pcm16_rows(x[:, 0, :], lens_d)
            p = pcm.cpu().numpy()
            return [p[b, : int(out[b])].tobytes() for b in range(B)]

        assert host() == device(), "device PCM differs from the host's"
        # alternate the two so drift on a shared host hits both alike
        ts = {"host": [], "device": []}
        for r in range(4):
            for name, fn in (("host", host), ("device", device)):
                ts[name] += timed(fn, calls // 4, warmup if r == 0 else 0)
        for name in ("host", "device"):
            emit(bench="op", op="pcm16_rows", backend=name, B=B,
                 row_seconds=SECONDS, sample_rate=SR, dtype="bf16",
                 **stats(ts[name]))


def bench_e2e(rounds: int, calls: int, warmup: int, label: str) -> None:
    from sonata_amd.models import create_random_voice, load_voice

    sentences = [("wˈʌn tˈuː θɹˈiː fˈoːɹ fˈaɪv sˈɪks " * (1 + b % 3)).strip()
                 + f" {'ˈeɪt ' * (b % 7)}." for b in range(64)]
    with tempfile.TemporaryDirectory() as d:
        v = load_voice(create_random_voice(d, "pcm_bench", quality="medium",
                                           seed=0), device=DEV)

        def floats():
            return [a.as_wave_bytes() for a in v.speak_batch(sentences)]

        def pcm(flag):
            def run():
                os.environ["SONATA_DEVICE_PCM"] = flag
                return [a.as_wave_bytes()
                        for a in v.speak_batch_pcm(sentences)]
            return run

        modes = [("float", floats)]
        if hasattr(v, "speak_batch_pcm"):
            modes += [("pcm0", pcm("0")), ("pcm1", pcm("1"))]
        ref = floats()
        audio_s = sum(len(b) for b in ref) / 2 / v.config.sample_rate
        for name, fn in modes:
            assert fn() == ref, f"{name}: wire bytes differ"
        for name, fn in modes:  # warm every mode before any is timed
            timed(fn, 0, warmup)
        for r in range(rounds):
            for name, fn in modes:
                emit(bench="e2e", tree=label, mode=name, round=r, B=64,
                     quality="medium", audio_seconds=round(audio_s, 2),
                     **stats(timed(fn, calls, 0)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=("op", "e2e", "all"), default="all")
    ap.add_argument("--calls", type=int, default=40,
                    help="timed calls per backend (op section)")
    ap.add_argument("--e2e-calls", type=int, default=5,
                    help="timed calls per mode per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="this",
                    help="name of the tree the e2e lines come from")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU path"
    if args.section in ("op", "all"):
        bench_op(args.calls, args.warmup)
    if args.section in ("e2e", "all"):
        bench_e2e(args.rounds, args.e2e_calls, args.warmup, args.label)


if __name__ == "__main__":
    main()
