"""Prosody on concurrent realtime streams: N streams through
synth.batcher.StreamBatcher with rate, pitch and volume all non-neutral,

  chunk       every chunk goes through AudioOutputConfig.apply on the host, in
              its stream's consumer thread, each chunk on its own: what
              synthesize_streamed does with stream_prosody == "chunk"
  continuous  the triple rides with the stream (StreamBatcher.open(prosody=))
              and the stretcher runs on the device inside the shared round,
              its state kept between chunks (csrc/prosody.hip
              wsola_stream_rows / resample_stream_rows); empty chunks are
              dropped, as synthesize_streamed does

For N in {1, 8, 32} on the medium random voice, chunk_size 45, padding 3:
  audio_sec_per_s    emitted audio seconds of all N streams over the wall
                     time from the common start to the last chunk on the host
  first_chunk_ms     per stream, from the common start to its first non-empty
                     chunk on the host: median and worst over the N streams
  first_chunk_audio_ms  duration of that first chunk (continuous holds back
                     what the next frame still needs)

The routes alternate in one process, --rounds times per N, after one untimed
pass of each.  Host clock; every chunk counted is a host array.  Needs a GPU.
A build without continuous stream prosody can run `--routes chunk` alone: that
is the baseline for the chunk numbers.

    python tools/tools_bench_stream_prosody.py [--rounds 5] [--out FILE.json]
"""
import argparse
import json
import statistics
import sys
import tempfile
import threading
import time

sys.path.insert(0, ".")

import torch

from tools.tools_bench_streams import DEV, sentences

# percent settings that map to (speed, volume, pitch) = (1.3, 0.8, 1.05)
RATE, VOLUME, PITCH = 16.0, 80.0, 55.0


def run_streams(open_stream, sents) -> dict:
    """All streams at once, one consumer thread each."""
    n = len(sents)
    go = threading.Barrier(n + 1)
    first = [None] * n
    first_len = [0] * n
    samples = [0] * n
    end = [None] * n
    errors = []

    def consumer(k):
        try:
            go.wait()
            for chunk in open_stream(sents[k]):
                if not len(chunk):
                    continue
                if first[k] is None:
                    first[k] = time.perf_counter()
                    first_len[k] = len(chunk)
                samples[k] += len(chunk)
            end[k] = time.perf_counter()
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=consumer, args=(k,)) for k in range(n)]
    for t in threads:
        t.start()
    go.wait()
    t0 = time.perf_counter()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    firsts = [(f - t0) * 1000.0 for f in first]
    return {"samples": sum(samples), "wall_s": max(end) - t0,
            "first_median_ms": statistics.median(firsts),
            "first_worst_ms": max(firsts),
            "first_len_median": statistics.median(first_len)}


def summary(rounds: list, sample_rate: int) -> dict:
    rate = [r["samples"] / sample_rate / r["wall_s"] for r in rounds]
    return {
        "audio_seconds": round(rounds[0]["samples"] / sample_rate, 2),
        "audio_sec_per_s": {"median": round(statistics.median(rate), 1),
                            "min": round(min(rate), 1),
                            "max": round(max(rate), 1),
                            "rounds": [round(x, 1) for x in rate]},
        "first_chunk_ms": {
            "median": round(statistics.median(
                r["first_median_ms"] for r in rounds), 2),
            "worst": round(max(r["first_worst_ms"] for r in rounds), 2),
            "median_per_round": [round(r["first_median_ms"], 2)
                                 for r in rounds],
            "worst_per_round": [round(r["first_worst_ms"], 2)
                                for r in rounds]},
        "first_chunk_audio_ms": round(
            rounds[0]["first_len_median"] * 1000.0 / sample_rate, 1),
    }


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--quality", default="medium")
    ap.add_argument("--routes", nargs="+", default=["chunk", "continuous"],
                    choices=["chunk", "continuous"])
    ap.add_argument("--out", default="profiles/r07_stream_prosody_ab.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU path"

    from sonata_amd.models import create_random_voice, load_voice
    from sonata_amd.synth.batcher import StreamBatcher
    from sonata_amd.synth.synthesizer import AudioOutputConfig

    cfg = AudioOutputConfig(rate=RATE, volume=VOLUME, pitch=PITCH)
    triple = cfg.prosody_triple()
    result = {
        "what": "N concurrent realtime streams through StreamBatcher with "
                "rate/pitch/volume: per-chunk host prosody (chunk) vs the "
                "device stretcher inside the shared round (continuous); one "
                "MI355X, the routes alternating in one process",
        "quality": args.quality, "chunk_size": 45, "chunk_padding": 3,
        "prosody": {"speed": triple[0], "volume": triple[1],
                    "pitch": triple[2]},
        "rounds": args.rounds, "routes": args.routes, "streams": {},
    }
    with tempfile.TemporaryDirectory() as d:
        v = load_voice(create_random_voice(d, "stream_bench",
                                           quality=args.quality, seed=0),
                       device=DEV)
        v.warmup()
        sr = v.config.sample_rate
        sb = StreamBatcher(v, max_streams=64)

        def chunk_route(s):
            for c in sb.open(s, 45, 3):
                yield cfg.apply(c, sr)

        fns = {"chunk": chunk_route,
               "continuous": lambda s: sb.open(s, 45, 3, prosody=triple)}
        routes = [(name, fns[name]) for name in args.routes]
        try:
            for n in args.streams:
                sents = sentences(n)
                for _, fn in routes:  # untimed: every shape seen once
                    run_streams(fn, sents)
                runs = {name: [] for name, _ in routes}
                for _ in range(args.rounds):
                    for name, fn in routes:
                        runs[name].append(run_streams(fn, sents))
                entry = {name: summary(rs, sr) for name, rs in runs.items()}
                result["streams"][str(n)] = entry
                print(json.dumps({"streams": n, **entry}), flush=True)
        finally:
            sb.close()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
