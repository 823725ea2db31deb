"""Seeded inputs for the staging tests of the channel-last conv kernels
(tests/test_gpu_pair_staging.py) and for tools/record_pair_staging_sha.py,
which records the output hashes of a build: both must build the very same
tensors, so the builders live here.  Everything is generated on the CPU from
a seeded generator and is exact in bf16.
"""

from __future__ import annotations

import hashlib
import os
from contextlib import contextmanager

import torch

import kernel_oracle as ko


def gen(*key):
    seed = 47
    for k in key:
        seed = (seed * 1000003 + int(k * 1000)) % (2 ** 31 - 1)
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def xtr(C):
    """xt tile rows of resblock_pair_cl_fused's default dispatch (C pads to
    CP in {32, 64, 128, 256})."""
    return 256 if C <= 32 else (64 if C > 128 else 128)


def pair_inputs(C, k, dil, B, T, lens, with_accum):
    g = gen(C, k, dil, B, T, with_accum)
    x = ko.rounding_free((B, T, C), g)
    w1 = ko.rounding_free((C, C, k), g, (C * k) ** -0.5)
    w2 = ko.rounding_free((C, C, k), g, (C * k) ** -0.5)
    b1, b2 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    acc = ko.rounding_free((B, T, C), g) if with_accum else None
    lens_t = None if lens is None else torch.tensor(lens)
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, dil=dil, lens=lens_t,
                accum=acc, scale=1.0 / 3.0)


def dispatch_shape(C, k):
    """B, T, out_lens of the tap-count dispatch cases."""
    BM = xtr(C) - (k - 1)
    T = 2 * BM + 7
    return 3, T, [T, BM + 1, 0]


# dilation per kernel size of the conv1d_cl cases: halos 0, 6, 8, 18, 50
CONV_DIL = {1: 1, 3: 3, 5: 2, 7: 3, 11: 5}


def conv_inputs(Cin, Cout, k, T):
    dil = CONV_DIL[k]
    g = gen(Cin, Cout, k, T)
    x = ko.rounding_free((2, T, Cin), g)
    w = ko.rounding_free((Cout, Cin, k), g, (Cin * k) ** -0.5)
    bias = torch.randn(Cout, generator=g)
    res = ko.rounding_free((2, T, Cout), g)
    # LeakyReLU on the input for k = 3, 7, 11; none for k = 1, 5
    pre = 0.1 if k in (3, 7, 11) else 0.0
    return dict(x=x, w=w, bias=bias, pad=(k - 1) * dil // 2, dil=dil, pre=pre,
                res=res, lens=torch.tensor([T, T // 2 + 1]))


def convt_inputs(Cin, Cout, s, Tin):
    k, pad = 2 * s, s // 2
    Tout = (Tin - 1) * s - 2 * pad + k
    g = gen(Cin, Cout, s, Tin)
    x = ko.rounding_free((2, Tin, Cin), g)
    w = ko.rounding_free((Cin, Cout, k), g, (Cin * 2) ** -0.5)
    bias = torch.randn(Cout, generator=g)
    return dict(x=x, w=w, bias=bias, s=s, pad=pad, pre=0.1,
                lens=torch.tensor([Tout, Tout // 2 + 3]))


def _dev(d, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v)
            for k, v in d.items()}


@contextmanager
def wlayout(name):
    """SONATA_RB_WLAYOUT for the calls inside (None: the default)."""
    old = os.environ.get("SONATA_RB_WLAYOUT")
    if name is None:
        os.environ.pop("SONATA_RB_WLAYOUT", None)
    else:
        os.environ["SONATA_RB_WLAYOUT"] = name
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SONATA_RB_WLAYOUT", None)
        else:
            os.environ["SONATA_RB_WLAYOUT"] = old


def run_pair(inp, dev, layout=None):
    from sonata_amd.ops.functional import resblock_pair_cl

    d = _dev(inp, dev)
    with wlayout(layout):
        return resblock_pair_cl(d["x"], d["w1"], d["b1"], d["w2"], d["b2"],
                                d["dil"], out_lens=d["lens"],
                                accum=d["accum"], out_scale=d["scale"])


def run_conv(inp, dev):
    from sonata_amd.ops.functional import leaky_conv1d_cl

    d = _dev(inp, dev)
    return leaky_conv1d_cl(d["x"], d["w"], d["bias"], padding=d["pad"],
                           dilation=d["dil"], pre_lrelu=d["pre"],
                           residual=d["res"], out_lens=d["lens"])


def run_convt(inp, dev):
    from sonata_amd.ops.functional import leaky_convtranspose1d_cl

    d = _dev(inp, dev)
    return leaky_convtranspose1d_cl(d["x"], d["w"], d["bias"], d["s"],
                                    d["pad"], pre_lrelu=d["pre"],
                                    out_lens=d["lens"])


def sha256_of(t: torch.Tensor) -> str:
    raw = t.detach().cpu().contiguous().view(torch.int16).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()


def _pair_case(C, k, dil, with_accum, layout):
    B, T, lens = dispatch_shape(C, k)
    return lambda dev: run_pair(pair_inputs(C, k, dil, B, T, lens,
                                            with_accum), dev, layout)


def _edge_case(C, k, dil, T_off):
    T = xtr(C) - (k - 1) + T_off
    return lambda dev: run_pair(pair_inputs(C, k, dil, 1, T, None, True), dev)


# The cases whose output bits are pinned to a build of the commit before the
# batched staging (tests/golden/pair_staging_parent_sha256.json).
SHA_CASES = {
    "pair_C32_k3_d1": _pair_case(32, 3, 1, False, None),
    "pair_C32_k11_d5_accum": _pair_case(32, 11, 5, True, None),
    "pair_C64_k7_d3_rows": _pair_case(64, 7, 3, True, "rows"),
    "pair_C64_k5_d2_sliced": _pair_case(64, 5, 2, False, "sliced"),
    "pair_C128_k11_d5_rows_accum": _pair_case(128, 11, 5, True, "rows"),
    "pair_C128_k5_d2_rows": _pair_case(128, 5, 2, False, "rows"),
    "pair_C128_k9_d1_sliced_accum": _pair_case(128, 9, 1, True, "sliced"),
    "pair_C256_k11_d5_rows": _pair_case(256, 11, 5, False, "rows"),
    "pair_C256_k3_d1_sliced_accum": _pair_case(256, 3, 1, True, "sliced"),
    "pair_C16_k11_d5_T_BM+1": _edge_case(16, 11, 5, 1),
    "pair_C40_k7_d3_T_BM-1": _edge_case(40, 7, 3, -1),
    "conv_192_130_k11_T769":
        lambda dev: run_conv(conv_inputs(192, 130, 11, 769), dev),
    "conv_192_33_k7_T769":
        lambda dev: run_conv(conv_inputs(192, 33, 7, 769), dev),
    "conv_24_33_k5_T257":
        lambda dev: run_conv(conv_inputs(24, 33, 5, 257), dev),
    "convt_192_130_s8_Tin385":
        lambda dev: run_convt(convt_inputs(192, 130, 8, 385), dev),
    "convt_192_33_s2_Tin385":
        lambda dev: run_convt(convt_inputs(192, 33, 2, 385), dev),
}
