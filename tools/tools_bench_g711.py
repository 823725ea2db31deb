"""G.711 benchmark: the float -> 8-bit wire-bytes finish of a synthesized
batch, companded on the device (csrc/pcm.hip g711_rows, uint8 copy) versus
on the host (pcm16_rows, int16 copy, audio.g711.encode per row).

  op   B = 64, 5 s rows at 8 kHz and at 22.05 kHz, bf16 [B, 1, T] as the
       decoder leaves them.  From the device tensor to a list of `bytes`.
  e2e  one batch of 64 sentences on the medium random voice, from phonemes
       to 8 kHz mu-law bytes:
         host    speak_batch_pcm(sample_rate=8000) + g711.encode per row
         device  speak_batch_pcm(sample_rate=8000, encoding="ulaw")

The two ways alternate, --rounds times; every round is the median of its
timed calls, and the summary line gives the median (min-max) of the rounds.
Host clock around work that ends in a synchronise (the host copy).  The two
ways must give the same bytes, or the run fails.  Needs a GPU: there is no
fallback.

    python tools/tools_bench_g711.py [--section op|e2e|all] [--rounds 5]
"""
import argparse
import json
import statistics
import sys
import tempfile
import time

sys.path.insert(0, ".")

import numpy as np
import torch

from sonata_amd.audio import g711

SECONDS = 5.0
DEV = "cuda:0"


def emit(**kw) -> None:
    print(json.dumps(kw), flush=True)


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


def alternate(ways, rounds: int, calls: int, warmup: int, **tags) -> None:
    """`ways` [(name, fn)] in turn, `rounds` times; one line per round and
    way, then one summary line per way."""
    ref = ways[0][1]()
    for name, fn in ways:
        assert fn() == ref, f"{name}: wire bytes differ"
    for name, fn in ways:  # warm every way before any is timed
        timed(fn, 0, warmup)
    med = {name: [] for name, _ in ways}
    for r in range(rounds):
        for name, fn in ways:
            ts = timed(fn, calls, 0)
            med[name].append(statistics.median(ts))
            emit(way=name, round=r, calls=calls,
                 median_ms=round(med[name][-1], 3), min_ms=round(min(ts), 3),
                 max_ms=round(max(ts), 3), **tags)
    for name, _ in ways:
        emit(way=name, summary=True, rounds=rounds,
             median_ms=round(statistics.median(med[name]), 3),
             min_ms=round(min(med[name]), 3),
             max_ms=round(max(med[name]), 3),
             wire_bytes=sum(len(b) for b in ref), **tags)


def bench_op(rounds: int, calls: int, warmup: int) -> None:
    from sonata_amd import ops

    B = 64
    for sr in (8000, 22050):
        n = int(sr * SECONDS)
        rng = np.random.default_rng(sr)
        x = torch.from_numpy(
            (0.3 * rng.standard_normal((B, 1, n))).astype(np.float32)
        ).to(DEV).to(torch.bfloat16)
        lens = [n - 37 * b for b in range(B)]

        def host():
            pcm, out = ops.pcm16_rows(x[:, 0, :], lens)
            p = pcm.cpu().numpy()
            return [g711.encode(p[b, : int(out[b])], "ulaw").tobytes()
                    for b in range(B)]

        def device():
            codes, out = ops.g711_rows(x[:, 0, :], lens, law="ulaw")
            c = codes.cpu().numpy()
            return [c[b, : int(out[b])].tobytes() for b in range(B)]

        alternate([("host", host), ("device", device)], rounds, calls,
                  warmup, bench="op", B=B, row_seconds=SECONDS,
                  sample_rate=sr, dtype="bf16", law="ulaw")


def bench_e2e(rounds: int, calls: int, warmup: int) -> None:
    from sonata_amd.models import create_random_voice, load_voice

    sentences = [("wˈʌn tˈuː θɹˈiː fˈoːɹ fˈaɪv sˈɪks " * (1 + b % 3)).strip()
                 + f" {'ˈeɪt ' * (b % 7)}." for b in range(64)]
    with tempfile.TemporaryDirectory() as d:
        v = load_voice(create_random_voice(d, "g711_bench", quality="medium",
                                           seed=0), device=DEV)

        def host():
            return [g711.encode(a.pcm, "ulaw").tobytes()
                    for a in v.speak_batch_pcm(sentences, sample_rate=8000)]

        def device():
            return [a.as_wave_bytes() for a in v.speak_batch_pcm(
                sentences, sample_rate=8000, encoding="ulaw")]

        audio_s = sum(len(b) for b in host()) / 8000.0
        alternate([("host", host), ("device", device)], rounds, calls,
                  warmup, bench="e2e", B=64, quality="medium",
                  sample_rate=8000, law="ulaw",
                  audio_seconds=round(audio_s, 2))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=("op", "e2e", "all"), default="all")
    ap.add_argument("--calls", type=int, default=20,
                    help="timed calls per way per round (op section)")
    ap.add_argument("--e2e-calls", type=int, default=5,
                    help="timed calls per way per round (e2e section)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU path"
    if args.section in ("op", "all"):
        bench_op(args.rounds, args.calls, args.warmup)
    if args.section in ("e2e", "all"):
        bench_e2e(args.rounds, args.e2e_calls, args.warmup)


if __name__ == "__main__":
    main()
