"""Concurrent realtime streams on one voice: N threads over
VitsVoice.stream_synthesis (serialised by the voice's inference lock: N
serial B=1 chunk decodes) versus the same N streams through
synth.batcher.StreamBatcher (one shared decode per round, csrc/stream.hip
around it).

For N in {1, 8, 32} on the medium random voice, chunk_size 45, padding 3:
  audio_sec_per_s   audio seconds of all N streams over the wall time from
                    the common start to the last chunk on the host
  first_chunk_ms    per stream, from the common start to its first chunk on
                    the host: median and worst over the N streams

The two routes alternate in one process, --rounds times per N, after one
untimed pass of each (graph captures, code objects, pinned buffers).  Host
clock; every chunk counted is a host array, so the device work it needed has
finished.  Needs a GPU: there is no fallback.

    python tools/tools_bench_streams.py [--rounds 5] [--out FILE.json]
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

DEV = "cuda:0"
BASE = [
    "ðɪs ɪz ə lˈɔŋ tɛst ʌv ðə stɹˈimɪŋ pˈæθ, wɪθ mˈɛni wˈɝdz.",
    "wˈʌn tˈuː θɹˈiː fˈoːɹ fˈaɪv sˈɪks sˈɛvən ˈeɪt nˈaɪn tˈɛn ɪlˈɛvən twˈɛlv.",
    "ðə kwˈɪk bɹˈaʊn fˈɑːks dʒˈʌmps ˈoʊvɚ ðə lˈeɪzi dˈɑːɡ ænd ɹˈʌnz ɐwˈeɪ "
    "fɹʌm ðə fˈɑːɹmɚ.",
    "hˈɛloʊ ðˈɛr ˈɛvɹiwˌʌn, ænd wˈɛlkəm tʊ ðə ʃˈoʊ.",
]


def sentences(n: int) -> list:
    """n distinct sentences of mixed length (distinct text: distinct seeds)."""
    return [BASE[k % len(BASE)][:-1] + " ˈeɪt" * (k // len(BASE)) + "."
            for k in range(n)]


def run_streams(open_stream, sents) -> dict:
    """All streams at once, one consumer thread each."""
    n = len(sents)
    go = threading.Barrier(n + 1)
    first = [None] * n
    samples = [0] * n
    end = [None] * n
    errors = []

    def consumer(k):
        try:
            go.wait()
            for chunk in open_stream(sents[k]):
                if first[k] is None:
                    first[k] = time.perf_counter()
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
            "first_worst_ms": max(firsts)}


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
    }


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--quality", default="medium")
    ap.add_argument("--out", default="profiles/r06_stream_batch_ab.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU path"

    from sonata_amd.models import create_random_voice, load_voice
    from sonata_amd.synth.batcher import StreamBatcher

    result = {
        "what": "N concurrent realtime streams on one voice: N threads over "
                "stream_synthesis (serial) vs StreamBatcher (batched); one "
                "MI355X, the two routes alternating in one process",
        "quality": args.quality, "chunk_size": 45, "chunk_padding": 3,
        "rounds": args.rounds, "streams": {},
    }
    with tempfile.TemporaryDirectory() as d:
        v = load_voice(create_random_voice(d, "stream_bench",
                                           quality=args.quality, seed=0),
                       device=DEV)
        v.warmup()
        sb = StreamBatcher(v, max_streams=64)
        routes = [("serial", lambda s: v.stream_synthesis(s, 45, 3)),
                  ("batched", lambda s: sb.open(s, 45, 3))]
        try:
            for n in args.streams:
                sents = sentences(n)
                for _, fn in routes:  # untimed: every shape seen once
                    run_streams(fn, sents)
                runs = {name: [] for name, _ in routes}
                for _ in range(args.rounds):
                    for name, fn in routes:
                        runs[name].append(run_streams(fn, sents))
                entry = {name: summary(rs, v.config.sample_rate)
                         for name, rs in runs.items()}
                result["streams"][str(n)] = entry
                print(json.dumps({"streams": n, **entry}), flush=True)
        finally:
            sb.close()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
