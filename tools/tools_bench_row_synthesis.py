"""Per-row synthesis benchmark: 64 sentences spread over 8 speakers of one
medium multi-speaker random voice, from phonemes to int16 wire bytes.

  rows     ONE speak_batch_pcm(synthesis=[...]): a speaker per row, one
           padded batch of 64 (scale_mask_rows, duration_rows,
           prior_sample_rows).
  groups   what a voice offers without per-row configs: 8 batches of 8,
           set_synthesis_config between them.
  uniform  the cost of the per-row path itself: the same 64 sentences, one
           speaker, through the scalar path (no synthesis=).

The ways alternate, --rounds times; every round is the median of its timed
calls, and the summary line gives the median (min-max) of the rounds.  Host
clock around work that ends in a synchronise (the host copy).  `rows` and
`groups` must render the same amount of audio within 1 %, or the run fails;
the number of rows whose length differs between the two is reported (a
batch of 64 and a batch of 8 may pick other GEMM tile variants, and a
duration that sits on a ceil boundary then moves by a frame), so bytes are
not compared.  Needs a GPU: there is no fallback.

    python tools/tools_bench_row_synthesis.py [--rounds 5] [--calls 5]
"""
import argparse
import json
import statistics
import sys
import tempfile
import time

sys.path.insert(0, ".")

import torch

DEV = "cuda:0"
SPEAKERS = 8


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
             max_ms=round(max(med[name]), 3), **tags)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5,
                    help="timed calls per way per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU path"
    from sonata_amd.models import (SynthesisConfig, create_random_voice,
                                   load_voice)

    sentences = [("wˈʌn tˈuː θɹˈiː fˈoːɹ fˈaɪv sˈɪks " * (1 + b % 3)).strip()
                 + f" {'ˈeɪt ' * (b % 7)}." for b in range(64)]
    with tempfile.TemporaryDirectory() as d:
        v = load_voice(create_random_voice(d, "rows_bench", quality="medium",
                                           seed=0, num_speakers=SPEAKERS),
                       device=DEV)
        base = v.get_synthesis_config()

        def cfg(k):
            return SynthesisConfig(k, base.noise_scale, base.length_scale,
                                   base.noise_w)

        # sentence b speaks as speaker b % 8
        row_cfgs = [cfg(b % SPEAKERS) for b in range(64)]
        by_speaker = [[b for b in range(64) if b % SPEAKERS == k]
                      for k in range(SPEAKERS)]

        def rows():
            return [a.as_wave_bytes()
                    for a in v.speak_batch_pcm(sentences, synthesis=row_cfgs)]

        def groups():
            out = [None] * 64
            try:
                for k, idx in enumerate(by_speaker):
                    v.set_synthesis_config(cfg(k))
                    for b, a in zip(idx, v.speak_batch_pcm(
                            [sentences[b] for b in idx])):
                        out[b] = a.as_wave_bytes()
            finally:
                v.set_synthesis_config(base)
            return out

        def uniform():
            return [a.as_wave_bytes() for a in v.speak_batch_pcm(sentences)]

        a, b = rows(), groups()
        mismatched = sum(len(x) != len(y) for x, y in zip(a, b))
        na, nb = sum(len(x) for x in a), sum(len(x) for x in b)
        assert abs(na - nb) <= 0.01 * nb, \
            "per-row batch and per-speaker batches render different audio"
        audio_s = na / 2.0 / v.config.sample_rate
        alternate([("rows", rows), ("groups", groups), ("uniform", uniform)],
                  args.rounds, args.calls, args.warmup, bench="row_synthesis",
                  B=64, speakers=SPEAKERS, quality="medium",
                  audio_seconds=round(audio_s, 2),
                  rows_with_other_length_in_groups=mismatched)


if __name__ == "__main__":
    main()
