"""Output sample-rate conversion benchmark: the polyphase FIR on the device
(csrc/resample.hip) versus the host finish (audio.resample.resample_poly per
row, after the f32 copy).

  op        B in {1, 64}, 5 s rows at 22.05 kHz (f32 [B, N]) to 8 and 48 kHz.
            device: ops.resample_rows + the copy of its f32 result;
            host:   the f32 copy of the input + resample_poly per row.
  e2e       one batch of 64 sentences on the medium random voice, phonemes
            to wire bytes at 8 kHz:
              device  speak_batch_pcm(sample_rate=8000)
              host    speak_batch + resample_poly + to_i16_bytes per row
  headline  bench.py in this tree and in a build of the parent commit
            (--parent DIR), as child processes in alternating rounds: the
            default path must not have moved.

Host clock around work that ends in a synchronise (the host copy); backends
alternate so drift on a shared host hits both alike; medians and spreads go
to --out as one JSON file.  Needs a GPU: there is no fallback.

    python tools/tools_bench_resample.py [--section op|e2e|headline|all]
        [--rounds 5] [--parent DIR] [--out profiles/r08_resample_ab.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, ".")

import numpy as np
import torch

from sonata_amd.audio.resample import resample_poly
from sonata_amd.audio.samples import to_i16_bytes

SR = 22050
SECONDS = 5.0
DEV = "cuda:0"


def spread(vals, nd=3) -> dict:
    return {"median": round(statistics.median(vals), nd),
            "min": round(min(vals), nd), "max": round(max(vals), nd),
            "rounds": [round(v, nd) for v in vals]}


def timed(fn, calls: int) -> float:
    """Median ms of `calls` synchronised calls."""
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1000.0)
    return statistics.median(ts)


def bench_op(rounds: int, calls: int, host_calls: int) -> dict:
    from sonata_amd import ops

    n = int(SR * SECONDS)
    out = {}
    for rate in (8000, 48000):
        for B in (1, 64):
            rng = np.random.default_rng(B)
            x = torch.from_numpy(
                (0.3 * rng.standard_normal((B, n))).astype(np.float32)
            ).to(DEV)
            lens = [n - 37 * b for b in range(B)]

            def device():
                y, ol = ops.resample_rows(x, lens, SR, rate)
                y = y.cpu().numpy()
                return [y[b, : int(ol[b])] for b in range(B)]

            def kernel():  # no copy back: the launch and its inputs alone
                ops.resample_rows(x, lens, SR, rate)

            def host():
                a = x.cpu().numpy()
                return [resample_poly(a[b, : lens[b]], SR, rate)
                        for b in range(B)]

            err = max(float(np.abs(d - h).max())
                      for d, h in zip(device(), host()))
            assert err < 1e-4, err
            kernel()
            ts = {"device": [], "kernel_only": [], "host": []}
            for _ in range(rounds):
                ts["device"].append(timed(device, calls))
                ts["kernel_only"].append(timed(kernel, calls))
                ts["host"].append(timed(host, host_calls))
            key = f"{SR}->{rate} B={B}"
            out[key] = {"row_seconds": SECONDS,
                        "max_abs_device_minus_host": err,
                        **{k + "_ms": spread(v) for k, v in ts.items()}}
            print(json.dumps({key: out[key]}), flush=True)
    return out


def bench_e2e(rounds: int, calls: int) -> dict:
    from sonata_amd.models import create_random_voice, load_voice

    sentences = [("wˈʌn tˈuː θɹˈiː fˈoːɹ fˈaɪv sˈɪks " * (1 + b % 3)).strip()
                 + f" {'ˈeɪt ' * (b % 7)}." for b in range(64)]
    with tempfile.TemporaryDirectory() as d:
        v = load_voice(create_random_voice(d, "rate_bench", quality="medium",
                                           seed=0), device=DEV)
        native = v.config.sample_rate

        def device():
            return [a.as_wave_bytes()
                    for a in v.speak_batch_pcm(sentences, sample_rate=8000)]

        def host():
            return [to_i16_bytes(resample_poly(a.samples, native, 8000))
                    for a in v.speak_batch(sentences)]

        def native_pcm():  # the unconverted call, for scale
            return [a.as_wave_bytes() for a in v.speak_batch_pcm(sentences)]

        dv, hs = device(), host()
        assert [len(b) for b in dv] == [len(b) for b in hs]
        worst = max(int(np.abs(np.frombuffer(a, "<i2").astype(np.int32)
                               - np.frombuffer(b, "<i2")).max())
                    for a, b in zip(dv, hs))
        assert worst <= 2, worst  # f32 vs f64 sums, then one truncation
        audio_s = sum(len(b) for b in dv) / 2 / 8000
        modes = (("device", device), ("host", host),
                 ("native_pcm", native_pcm))
        for _, fn in modes:
            for _ in range(3):
                fn()
        ts = {name: [] for name, _ in modes}
        for _ in range(rounds):
            for name, fn in modes:
                ts[name].append(timed(fn, calls))
        out = {"B": 64, "quality": "medium", "native_rate": native,
               "rate_out": 8000, "audio_seconds": round(audio_s, 2),
               "max_pcm_step_device_minus_host": worst,
               **{k + "_ms": spread(v) for k, v in ts.items()}}
        print(json.dumps({"e2e": out}), flush=True)
        return out


def bench_headline(rounds: int, parent: str, steps: int, warmup: int) -> dict:
    trees = [("this", os.getcwd())]
    if parent:
        trees.insert(0, ("parent", os.path.abspath(parent)))
    vals = {name: [] for name, _ in trees}
    for _ in range(rounds):
        for name, root in trees:
            p = subprocess.run(
                [sys.executable, "bench.py", "--gpus", "1", "--steps",
                 str(steps), "--warmup", str(warmup)],
                cwd=root, capture_output=True, text=True, timeout=600,
                check=True)
            line = [ln for ln in p.stdout.splitlines()
                    if ln.startswith("{")][-1]
            vals[name].append(float(json.loads(line)["value"]))
            print(json.dumps({"headline": name, "value": vals[name][-1]}),
                  flush=True)
    return {"command": f"bench.py --gpus 1 --steps {steps} --warmup {warmup}",
            "unit": "audio_sec/s",
            **{k: spread(v, 1) for k, v in vals.items()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", default="all",
                    choices=("op", "e2e", "headline", "all"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--host-calls", type=int, default=1,
                    help="timed host calls per round (op section)")
    ap.add_argument("--e2e-calls", type=int, default=3)
    ap.add_argument("--parent", default=None,
                    help="a built tree of the parent commit (headline)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU path"
    res = {"what": "output sample-rate conversion: csrc/resample.hip on the "
                   "device vs audio.resample.resample_poly on the host after "
                   "the f32 copy; one MI355X, alternating rounds in one "
                   "command; ms are medians per round",
           "rounds": args.rounds}
    if args.section in ("op", "all"):
        res["op"] = bench_op(args.rounds, args.calls, args.host_calls)
    if args.section in ("e2e", "all"):
        res["e2e"] = bench_e2e(args.rounds, args.e2e_calls)
    if args.section in ("headline", "all"):
        res["headline"] = bench_headline(args.rounds, args.parent,
                                         args.steps, args.warmup)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
