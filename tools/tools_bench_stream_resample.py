"""Output sample rate on concurrent realtime streams: N streams through
synth.batcher.StreamBatcher, every one asked for 8 kHz,

  host    every chunk goes through one audio.resample.StreamResampler per
          stream on the host (NumPy, in the stream's consumer thread), flushed
          at the end: what synthesize_streamed does with stream_resample ==
          "host", the default
  device  the rate rides with the stream (StreamBatcher.open(sample_rate=))
          and the filter runs on the device inside the shared round, its carry
          kept between chunks (csrc/resample.hip resample_poly_stream_rows);
          empty chunks are dropped, as synthesize_streamed does

For N in {1, 8, 32} on the medium random voice, chunk_size 45, padding 3:
  audio_sec_per_s  emitted audio seconds (at the output rate) of all N streams
                   over the wall time from the common start to the last chunk
                   on the host
  first_chunk_ms   per stream, from the common start to its first non-empty
                   chunk on the host; per round the median over the N streams

The routes alternate in one process, --rounds times per N, after one untimed
pass of each; both are reported as median (min-max) over the rounds.  "device"
is called faster at an N only when its slowest round beats the fastest round
of "host".  Host clock; every chunk counted is a host array.  Needs a GPU.

    python tools/tools_bench_stream_resample.py [--rounds 5] [--out FILE.json]
"""
import argparse
import json
import statistics
import sys
import tempfile

sys.path.insert(0, ".")

import torch

from tools.tools_bench_stream_prosody import run_streams
from tools.tools_bench_streams import DEV, sentences


def spread(values, digits: int) -> dict:
    return {"median": round(statistics.median(values), digits),
            "min": round(min(values), digits),
            "max": round(max(values), digits),
            "rounds": [round(v, digits) for v in values]}


def summary(rounds: list, rate_out: int) -> dict:
    return {
        "audio_seconds": round(rounds[0]["samples"] / rate_out, 2),
        "audio_sec_per_s": spread(
            [r["samples"] / rate_out / r["wall_s"] for r in rounds], 1),
        "first_chunk_ms": spread([r["first_median_ms"] for r in rounds], 2),
        "first_chunk_worst_ms": round(
            max(r["first_worst_ms"] for r in rounds), 2),
        "first_chunk_audio_ms": round(
            rounds[0]["first_len_median"] * 1000.0 / rate_out, 1),
    }


def verdict(entry: dict) -> str:
    """"device" is faster only if its slowest round beats host's fastest."""
    h = entry["host"]["audio_sec_per_s"]
    d = entry["device"]["audio_sec_per_s"]
    if d["min"] > h["max"]:
        return "device faster"
    if h["min"] > d["max"]:
        return "NEGATIVE: host faster"
    return "no difference outside the spread"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--quality", default="medium")
    ap.add_argument("--rate", type=int, default=8000)
    ap.add_argument("--out", default="profiles/r10_stream_resample_ab.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU path"

    from sonata_amd.audio.resample import StreamResampler
    from sonata_amd.models import create_random_voice, load_voice
    from sonata_amd.synth.batcher import StreamBatcher

    result = {
        "what": "N concurrent realtime streams through StreamBatcher at an "
                "output rate: one host StreamResampler per stream (host) vs "
                "the polyphase kernel inside the shared round (device); one "
                "MI355X, the routes alternating in one process",
        "quality": args.quality, "chunk_size": 45, "chunk_padding": 3,
        "rate_out": args.rate, "rounds": args.rounds, "streams": {},
    }
    with tempfile.TemporaryDirectory() as d:
        v = load_voice(create_random_voice(d, "stream_bench",
                                           quality=args.quality, seed=0),
                       device=DEV)
        v.warmup()
        sr = v.config.sample_rate
        result["rate_in"] = sr
        sb = StreamBatcher(v, max_streams=64)

        def host_route(s):
            rs = StreamResampler(sr, args.rate)
            for c in sb.open(s, 45, 3):
                yield rs.push(c)
            yield rs.flush()

        routes = [("host", host_route),
                  ("device",
                   lambda s: sb.open(s, 45, 3, sample_rate=args.rate))]
        try:
            for n in args.streams:
                sents = sentences(n)
                for _, fn in routes:  # untimed: every shape seen once
                    run_streams(fn, sents)
                runs = {name: [] for name, _ in routes}
                for _ in range(args.rounds):
                    for name, fn in routes:
                        runs[name].append(run_streams(fn, sents))
                entry = {name: summary(rs, args.rate)
                         for name, rs in runs.items()}
                entry["verdict"] = verdict(entry)
                result["streams"][str(n)] = entry
                print(json.dumps({"streams": n, **entry}), flush=True)
        finally:
            sb.close()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
