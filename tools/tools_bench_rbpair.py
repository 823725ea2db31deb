"""Microbench: resblock pair kernel on the real bench decode shapes.

The kernel variants are selected by environment, read by the extension
(SONATA_PERSIST_RB once per process; SONATA_RB_GEOM and SONATA_RB_WLAYOUT
per call), so an A/B runs this script once per setting, alternating.

  --lens full   no out_lens (every tile live)
  --lens T      out_lens = T for every row: the ragged path, nothing dead
  --lens half   out_lens = T/2 for every row: half of the tiles are dead
  --json PATH   also write the per-shape times as one JSON object
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, '.')
from sonata_amd.ops.functional import resblock_pair_cl  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lens", choices=["full", "T", "half"], default="full")
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--json", default=None)
args = ap.parse_args()

B = 64
F = 600  # ~frames per utterance in the flagship bench
dev = "cuda:0"
# (C, k, dil, T)
shapes = [(32, 3, 1, 256 * F), (32, 3, 3, 256 * F), (32, 7, 3, 256 * F),
          (32, 11, 5, 256 * F), (64, 3, 1, 128 * F), (64, 3, 5, 128 * F),
          (64, 7, 3, 128 * F), (128, 3, 1, 64 * F), (128, 7, 3, 64 * F),
          (128, 11, 5, 64 * F), (256, 3, 1, 8 * F), (256, 7, 3, 8 * F),
          (256, 11, 5, 8 * F)]
print(f"# persist={os.environ.get('SONATA_PERSIST_RB')} "
      f"geom={os.environ.get('SONATA_RB_GEOM')} "
      f"wlayout={os.environ.get('SONATA_RB_WLAYOUT')} lens={args.lens}")
results = {}
for C, k, dil, T in shapes:
    x = (torch.randn(B // 8, T, C) / 4).to(torch.bfloat16).to(dev)
    # B//8 keeps memory sane; per-shape time scales linearly in B
    w1 = (torch.randn(C, C, k) / (C * k) ** 0.5).to(torch.bfloat16).to(dev)
    w2 = (torch.randn(C, C, k) / (C * k) ** 0.5).to(torch.bfloat16).to(dev)
    b1 = (torch.randn(C) / 10).to(dev)
    b2 = (torch.randn(C) / 10).to(dev)
    lens = None
    if args.lens != "full":
        n = T if args.lens == "T" else T // 2
        lens = torch.full((B // 8,), n, dtype=torch.int32, device=dev)
    for _ in range(3):
        y = resblock_pair_cl(x, w1, b1, w2, b2, dilation=dil, out_lens=lens)
    torch.cuda.synchronize()
    N = args.iters
    t0 = time.perf_counter()
    for _ in range(N):
        y = resblock_pair_cl(x, w1, b1, w2, b2, dilation=dil, out_lens=lens)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / N
    flops = 2 * 2 * x.shape[0] * T * C * C * k  # two convs
    gbytes = 2 * x.shape[0] * T * C * 3  # read x + write + residual read
    results[f"C{C}_k{k}_d{dil}"] = round(dt * 1e3, 4)
    print(f"C={C:3d} k={k:2d} d={dil} T={T:7d}: {dt*1e3:7.3f} ms  "
          f"{flops/dt/1e12:6.1f} TF  {gbytes/dt/1e9:7.0f} GB/s")
if args.json:
    with open(args.json, "w") as f:
        json.dump({"lens": args.lens,
                   "wlayout": os.environ.get("SONATA_RB_WLAYOUT"),
                   "ms": results}, f)
