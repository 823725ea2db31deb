"""Functional ops used by the VITS graph.

Each op has two implementations:
  * torch: plain PyTorch fp32 — the numerics oracle, used on CPU and under
    SONATA_FORCE_TORCH=1.
  * hip: hand-written CDNA4 kernel from the `_sonata_hip` extension — the
    serving path on MI355X.  Mandatory when tensors are on GPU.

Kernel inventory: LayerNorm over channels, WaveNet fused
gated tanh·sigmoid, prior sampling z = m + eps·exp(logs)·noise, duration
expansion (length regulator), Conv1d / ConvTranspose1d with fused
LeakyReLU (MFMA conv-as-GEMM).
"""

from __future__ import annotations

import threading
from typing import Optional

import torch
import torch.nn.functional as F

from . import hip_ext, use_hip


# --------------------------------------------------------------------------- #
# LayerNorm over the channel dim of [B, C, T]
# --------------------------------------------------------------------------- #
def layer_norm_ct(
    x: torch.Tensor,
    gamma: torch.Tensor,
    beta: torch.Tensor,
    eps: float = 1e-5,
    residual: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """LayerNorm across channels of [B,C,T]; optional fused residual:
    normalizes (x + residual)."""
    if use_hip(x):
        ext = hip_ext(required=True)
        return ext.layer_norm_ct(
            x.contiguous(),
            residual.contiguous() if residual is not None else None,
            _bias_f32(gamma), _bias_f32(beta), eps,
        )
    if residual is not None:
        x = x + residual
    # torch reference: normalize across C for each (b, t)
    mean = x.mean(dim=1, keepdim=True)
    var = x.var(dim=1, unbiased=False, keepdim=True)
    xhat = (x - mean) * torch.rsqrt(var + eps)
    return xhat * gamma.view(1, -1, 1) + beta.view(1, -1, 1)


# --------------------------------------------------------------------------- #
# WaveNet gated activation: split channels, tanh(a+ga) * sigmoid(b+gb)
# --------------------------------------------------------------------------- #
def fused_gate(
    x: torch.Tensor, g: Optional[torch.Tensor], n_channels: int
) -> torch.Tensor:
    """x: [B, 2C, T] conv output; g: [B, 2C, T] conditioning (or None).
    Returns tanh(x_a + g_a) * sigmoid(x_b + g_b), [B, C, T]."""
    if use_hip(x):
        ext = hip_ext(required=True)
        return ext.fused_gate(
            x.contiguous(),
            g.contiguous() if g is not None else None,
            n_channels,
        )
    if g is not None:
        x = x + g
    a, b = x[:, :n_channels], x[:, n_channels:]
    return torch.tanh(a) * torch.sigmoid(b)


# --------------------------------------------------------------------------- #
# Prior sampling: z = (m + randn * exp(logs) * noise_scale) * mask
# --------------------------------------------------------------------------- #
def prior_sample(
    m: torch.Tensor,
    logs: torch.Tensor,
    mask: torch.Tensor,
    noise: torch.Tensor,
    noise_scale: float,
) -> torch.Tensor:
    if use_hip(m):
        ext = hip_ext(required=True)
        return ext.prior_sample(m.contiguous(), logs.contiguous(),
                                mask.contiguous(), noise, float(noise_scale))
    return (m + noise * torch.exp(logs) * noise_scale) * mask


# --------------------------------------------------------------------------- #
# Per-row synthesis scales: one noise_scale / noise_w / length_scale per batch
# row.  The scales are f32 [B] end to end: each product is taken in f32 and
# rounded to the activation dtype once, as a multiply by the Python float is
# (a bf16 tensor of scales would round 0.8 to 0.80078 first).
# --------------------------------------------------------------------------- #
def _rows_f32(scales: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    return scales.to(device=like.device, dtype=torch.float32).contiguous()


def _mul_rows(x: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """x [B,...] times scales[b]: f32 product, one rounding to x's dtype."""
    s = scales.view(-1, *([1] * (x.dim() - 1)))
    return (x.float() * s).to(x.dtype)


def prior_sample_rows(
    m: torch.Tensor,
    logs: torch.Tensor,
    mask: torch.Tensor,
    noise: torch.Tensor,
    noise_scale: torch.Tensor,
) -> torch.Tensor:
    """prior_sample with noise_scale f32 [B]: row b is prior_sample of that
    row alone with float(noise_scale[b]).  m / logs may be the two halves of
    one [B,2C,T] tensor (dense planes, free batch stride)."""
    ns = _rows_f32(noise_scale, m)
    if use_hip(m):
        ext = hip_ext(required=True)
        return ext.prior_sample_rows(m, logs, mask.contiguous(),
                                     noise.contiguous(), ns)
    return (m + _mul_rows(noise * torch.exp(logs), ns)) * mask


def scale_mask_rows(
    noise: torch.Tensor, mask: torch.Tensor, scales: torch.Tensor
) -> torch.Tensor:
    """noise [B,C,T] * scales[b] * mask [B,1,T]: bit-equal, row by row, to
    `noise * float(scales[b]) * mask`."""
    s = _rows_f32(scales, noise)
    if use_hip(noise):
        ext = hip_ext(required=True)
        return ext.scale_mask_rows(noise.contiguous(), mask.contiguous(), s)
    return _mul_rows(noise, s) * mask


def duration_rows(
    logw: torch.Tensor, x_mask: torch.Tensor, length_scale: torch.Tensor
):
    """ceil(exp(logw) * x_mask * length_scale[b]) -> (durs int32 [B,T],
    y_lengths int64 [B], at least 1): the eager duration chain with a scale
    per row, every rounding of the activation dtype kept (the row sum's
    too).  One launch on the GPU."""
    ls = _rows_f32(length_scale, logw)
    if use_hip(logw):
        ext = hip_ext(required=True)
        if logw.shape[2] != 1 and logw.stride(2) != 1:
            logw = logw.contiguous()
        durs, y_lengths = ext.duration_rows(logw, x_mask.contiguous(), ls)
        return durs, y_lengths
    w_ceil = torch.ceil(_mul_rows(torch.exp(logw) * x_mask, ls))
    y_lengths = torch.clamp_min(torch.sum(w_ceil, [1, 2]), 1).long()
    return w_ceil.squeeze(1).to(torch.int32), y_lengths


# --------------------------------------------------------------------------- #
# Length regulator: expand phoneme states to frame states by durations
# --------------------------------------------------------------------------- #
def expand_states(
    stats: torch.Tensor, durations: torch.Tensor, y_lengths: torch.Tensor,
    F_max: Optional[int] = None,
) -> torch.Tensor:
    """stats: [B, C, T_ph]; durations: [B, T_ph] int frame counts;
    returns [B, C, F_max] where F_max = y_lengths.max().

    The attention path matrix of VITS inference: frame f copies phoneme p
    where cum_dur[p-1] <= f < cum_dur[p]."""
    if F_max is None:
        F_max = int(y_lengths.max().item())
    if use_hip(stats):
        ext = hip_ext(required=True)
        return ext.expand_states(
            stats.contiguous(),
            durations.to(torch.int32).contiguous(),
            F_max,
        )
    B, C, T = stats.shape
    out = stats.new_zeros((B, C, F_max))
    for b in range(B):
        cum = torch.cumsum(durations[b], dim=0)
        # phoneme index for each frame
        frames = torch.arange(F_max, device=stats.device)
        idx = torch.searchsorted(cum, frames, right=True).clamp(max=T - 1)
        valid = frames < int(y_lengths[b].item())
        out[b, :, valid] = stats[b][:, idx[valid]]
    return out


# --------------------------------------------------------------------------- #
# Conv1d (+ fused LeakyReLU on input or output) — the HiFi-GAN hot op
# --------------------------------------------------------------------------- #
def _round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


# Widest halo (k-1)*dilation conv1d_mfma_kernel stages beside a time tile
# (HALO_MAX in csrc/conv1d.hip).  conv1d_fused sends anything wider to the
# naive kernel, which reads the raw [Cout, Cin/groups, k] weight.
CONV_MFMA_HALO_MAX = 64


def _conv_takes_mfma(x: torch.Tensor, k: int, stride: int, dilation: int,
                     groups: int) -> bool:
    """True when conv1d_fused will run the MFMA kernel for these arguments,
    i.e. when it expects the `_conv_weight_mfma` layout."""
    return (x.dtype == torch.bfloat16 and groups == 1 and stride == 1
            and (k - 1) * dilation <= CONV_MFMA_HALO_MAX)


def _conv_weight_mfma(weight: torch.Tensor) -> torch.Tensor:
    """Cache the MFMA layout of a conv weight: [Cout,Cin,k] ->
    [k, CoutP, CinP] bf16, Cout padded to the tile height, Cin to 32.
    Weights are static at inference; the permuted copy lives on the
    parameter object."""
    cached = getattr(weight, "_sonata_perm", None)
    if cached is not None:
        return cached
    Cout, Cin, k = weight.shape
    bm = 128 if Cout >= 128 else (64 if Cout >= 64 else 32)
    CoutP, CinP = _round_up(Cout, bm), _round_up(Cin, 32)
    perm = torch.zeros((k, CoutP, CinP), dtype=torch.bfloat16,
                       device=weight.device)
    perm[:, :Cout, :Cin] = weight.detach().permute(2, 0, 1).to(torch.bfloat16)
    perm = perm.contiguous()
    weight._sonata_perm = perm
    return perm


def _slice_weight_windows(perm: torch.Tensor) -> torch.Tensor:
    """[k, CoutP, CinP] -> [k, CinP/32, CoutP, 32]: the same numbers, stored
    so that each (tap, 32-channel K slice) window the resblock pair kernel
    stages is one contiguous block.  Element (tap, co, ci) moves to
    (tap, ci // 32, co, ci % 32)."""
    k, CoutP, CinP = perm.shape
    return perm.view(k, CoutP, CinP // 32, 32).permute(0, 2, 1, 3).contiguous()


def _conv_weight_sliced(weight: torch.Tensor) -> torch.Tensor:
    """Cache the sliced layout next to the `_conv_weight_mfma` one: built
    once per weight, never per call."""
    cached = getattr(weight, "_sonata_perm_sliced", None)
    if cached is not None:
        return cached
    sliced = _slice_weight_windows(_conv_weight_mfma(weight))
    weight._sonata_perm_sliced = sliced
    return sliced


def _convt_weight_mfma(weight: torch.Tensor, stride: int) -> torch.Tensor:
    """ConvTranspose1d weight [Cin,Cout,k] -> phase layout
    [s, kr_max, CoutP, CinP] bf16 where phase r tap m holds W[:, :, r+s*m]."""
    cached = getattr(weight, "_sonata_perm_t", None)
    if cached is not None:
        return cached
    Cin, Cout, k = weight.shape
    kr_max = (k + stride - 1) // stride
    bm = 128 if Cout >= 128 else (64 if Cout >= 64 else 32)
    CoutP, CinP = _round_up(Cout, bm), _round_up(Cin, 32)
    perm = torch.zeros((stride, kr_max, CoutP, CinP), dtype=torch.bfloat16,
                       device=weight.device)
    w = weight.detach().to(torch.bfloat16)
    for r in range(stride):
        for m in range((k - r + stride - 1) // stride):
            perm[r, m, :Cout, :Cin] = w[:, :, r + stride * m].t()
    perm = perm.contiguous()
    weight._sonata_perm_t = perm
    return perm


def _bias_f32(bias: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if bias is None:
        return None
    cached = getattr(bias, "_sonata_f32", None)
    if cached is None:
        cached = bias.detach().float().contiguous()
        bias._sonata_f32 = cached
    return cached


def leaky_conv1d(
    x: torch.Tensor,
    weight: torch.Tensor,
    bias: Optional[torch.Tensor],
    stride: int = 1,
    padding: int = 0,
    dilation: int = 1,
    groups: int = 1,
    pre_lrelu: float = 0.0,
    post_lrelu: float = 0.0,
    residual: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Conv1d with optional fused LeakyReLU applied to the input
    (pre_lrelu>0) and/or the output (post_lrelu>0), plus an optional fused
    residual add (out = act(conv(x)) + residual).  Fusing keeps activation
    and residual tensors out of HBM (HiFi-GAN MRF pattern:
    x = x + conv(lrelu(conv(lrelu(x)))))."""
    if use_hip(x):
        ext = hip_ext(required=True)
        Cout, _, k = weight.shape
        mfma = _conv_takes_mfma(x, k, stride, dilation, groups)
        w = _conv_weight_mfma(weight) if mfma \
            else weight.to(x.dtype).contiguous()
        return ext.conv1d_fused(
            x.contiguous(), w, _bias_f32(bias),
            Cout, k, stride, padding, dilation, groups,
            pre_lrelu if pre_lrelu > 0.0 else -1.0,
            1 if post_lrelu > 0.0 else 0, float(post_lrelu),
            residual.contiguous() if residual is not None else None,
        )
    if pre_lrelu > 0.0:
        x = F.leaky_relu(x, pre_lrelu)
    y = F.conv1d(x, weight, bias, stride=stride, padding=padding,
                 dilation=dilation, groups=groups)
    if post_lrelu > 0.0:
        y = F.leaky_relu(y, post_lrelu)
    if residual is not None:
        y = y + residual
    return y


def leaky_convtranspose1d(
    x: torch.Tensor,
    weight: torch.Tensor,
    bias: Optional[torch.Tensor],
    stride: int,
    padding: int,
    pre_lrelu: float = 0.0,
) -> torch.Tensor:
    """ConvTranspose1d with fused LeakyReLU on the input — the HiFi-GAN
    upsampling stage (y = convT(lrelu(x)))."""
    if use_hip(x):
        ext = hip_ext(required=True)
        Cin, Cout, k = weight.shape
        mfma = x.dtype == torch.bfloat16
        w = _convt_weight_mfma(weight, stride) if mfma \
            else weight.to(x.dtype).contiguous()
        return ext.convtranspose1d_fused(
            x.contiguous(), w, _bias_f32(bias),
            Cout, k, stride, padding,
            pre_lrelu if pre_lrelu > 0.0 else -1.0,
        )
    if pre_lrelu > 0.0:
        x = F.leaky_relu(x, pre_lrelu)
    return F.conv_transpose1d(x, weight, bias, stride=stride, padding=padding)


def conv_mod(
    mod: torch.nn.Conv1d,
    x: torch.Tensor,
    pre_lrelu: float = 0.0,
    post_lrelu: float = 0.0,
) -> torch.Tensor:
    """Run an nn.Conv1d module through the dispatched conv op."""
    return leaky_conv1d(
        x, mod.weight, mod.bias, stride=mod.stride[0], padding=mod.padding[0],
        dilation=mod.dilation[0], groups=mod.groups,
        pre_lrelu=pre_lrelu, post_lrelu=post_lrelu,
    )


# --------------------------------------------------------------------------- #
# ragged-batch tail masking
# --------------------------------------------------------------------------- #
def mask_tail_(x: torch.Tensor, lengths: Optional[torch.Tensor]) -> torch.Tensor:
    """In-place zero of x[b, :, lengths[b]:].  Applied between decoder
    stages so padded-batch synthesis is numerically identical to
    single-utterance synthesis (padding never feeds valid conv taps).
    No-op when lengths is None or nothing is padded."""
    if lengths is None:
        return x
    T = x.shape[-1]
    if bool((lengths >= T).all()):
        return x
    if use_hip(x):
        ext = hip_ext(required=True)
        return ext.mask_tail_(x, lengths.to(device=x.device,
                                            dtype=torch.int32).contiguous())
    idx = torch.arange(T, device=x.device)
    pad = idx.unsqueeze(0) >= lengths.to(x.device).unsqueeze(1)  # [B, T]
    return x.masked_fill_(pad.unsqueeze(1), 0)


# --------------------------------------------------------------------------- #
# channel-last conv ops (HiFi-GAN decode path)
# --------------------------------------------------------------------------- #
def _lens_i32(lengths: Optional[torch.Tensor], device) -> Optional[torch.Tensor]:
    if lengths is None:
        return None
    return lengths.to(device=device, dtype=torch.int32).contiguous()


def leaky_conv1d_cl(
    x: torch.Tensor,  # [B, T, C] channel-last
    weight: torch.Tensor,  # nn.Conv1d weight [Cout, Cin, k]
    bias: Optional[torch.Tensor],
    padding: int = 0,
    dilation: int = 1,
    pre_lrelu: float = 0.0,
    post_lrelu: float = 0.0,
    post_tanh: bool = False,
    post_relu: bool = False,
    residual: Optional[torch.Tensor] = None,
    out_lens: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Channel-last stride-1 Conv1d with fused input/output LeakyReLU (or
    tanh / relu), residual add and ragged-batch row masking.  The
    MI355X-native layout: Cin contiguous makes both MFMA operands
    k-contiguous (csrc/conv1d_cl.hip)."""
    if use_hip(x):
        ext = hip_ext(required=True)
        Cout, _, k = weight.shape
        act = 2 if post_tanh else (
            1 if (post_lrelu > 0.0 or post_relu) else 0)
        return ext.conv1d_cl_fused(
            x.contiguous(), _conv_weight_mfma(weight), _bias_f32(bias),
            Cout, k, padding, dilation,
            pre_lrelu if pre_lrelu > 0.0 else -1.0,
            act, float(post_lrelu),
            residual.contiguous() if residual is not None else None,
            _lens_i32(out_lens, x.device),
        )
    # torch oracle: transpose to channel-first
    xc = x.transpose(1, 2)
    if pre_lrelu > 0.0:
        xc = F.leaky_relu(xc, pre_lrelu)
    y = F.conv1d(xc, weight, bias, padding=padding, dilation=dilation)
    if post_tanh:
        y = torch.tanh(y)
    elif post_relu:
        y = torch.relu(y)
    elif post_lrelu > 0.0:
        y = F.leaky_relu(y, post_lrelu)
    y = y.transpose(1, 2)
    if residual is not None:
        y = y + residual
    if out_lens is not None:
        idx = torch.arange(y.shape[1], device=y.device)
        y = y.masked_fill(
            (idx.unsqueeze(0) >= out_lens.to(y.device).unsqueeze(1))
            .unsqueeze(-1), 0)
    return y


def leaky_convtranspose1d_cl(
    x: torch.Tensor,  # [B, T, C]
    weight: torch.Tensor,  # nn.ConvTranspose1d weight [Cin, Cout, k]
    bias: Optional[torch.Tensor],
    stride: int,
    padding: int,
    pre_lrelu: float = 0.0,
    out_lens: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Channel-last ConvTranspose1d (k = 2*stride HiFi-GAN upsampler),
    phase-merged MFMA kernel with fused input LeakyReLU + row masking."""
    if use_hip(x):
        ext = hip_ext(required=True)
        Cin, Cout, k = weight.shape
        return ext.convtranspose1d_cl_fused(
            x.contiguous(), _convt_weight_mfma(weight, stride),
            _bias_f32(bias), Cout, k, stride, padding,
            pre_lrelu if pre_lrelu > 0.0 else -1.0,
            _lens_i32(out_lens, x.device),
        )
    xc = x.transpose(1, 2)
    if pre_lrelu > 0.0:
        xc = F.leaky_relu(xc, pre_lrelu)
    y = F.conv_transpose1d(xc, weight, bias, stride=stride, padding=padding)
    y = y.transpose(1, 2)
    if out_lens is not None:
        idx = torch.arange(y.shape[1], device=y.device)
        y = y.masked_fill(
            (idx.unsqueeze(0) >= out_lens.to(y.device).unsqueeze(1))
            .unsqueeze(-1), 0)
    return y


def resblock_pair_cl(
    x: torch.Tensor,  # [B, T, C]
    w1: torch.Tensor, b1: Optional[torch.Tensor],
    w2: torch.Tensor, b2: Optional[torch.Tensor],
    dilation: int,
    out_lens: Optional[torch.Tensor] = None,
    accum: Optional[torch.Tensor] = None,
    out_scale: float = 1.0,
) -> torch.Tensor:
    """Fused resblock conv pair: (conv2_{k,1}(lrelu(conv1_{k,d}(lrelu(x))))
    + x [+ accum]) * out_scale, channel-last, intermediate tensor kept in
    LDS (csrc/resblock_cl.hip).  `accum`/`out_scale` fold the MRF
    cross-resblock sum and /num_kernels into the epilogue.  Shapes the
    fused kernel does not take (halo (k-1)*dilation > 52, channel counts
    that do not pad to a square 32/64/128/256 weight) run as two convs."""
    Cout, Cin, k = w1.shape
    fused = (use_hip(x) and Cin == Cout and w2.shape == w1.shape
             and b1 is not None and b2 is not None
             and (k - 1) * dilation <= 52)
    if fused:
        # the kernel is instantiated for square padded weights of 32, 64,
        # 128 or 256 channels only (e.g. C=96 pads to 128x96: not square)
        w1p, w2p = _conv_weight_mfma(w1), _conv_weight_mfma(w2)
        fused = (w1p.shape[1] == w1p.shape[2] and w2p.shape == w1p.shape
                 and w1p.shape[1] in (32, 64, 128, 256))
    if fused:
        ext = hip_ext(required=True)
        # SONATA_RB_WLAYOUT=rows|sliced, read by the extension per call
        if ext.resblock_wlayout_sliced(w1p.shape[1]):
            op = ext.resblock_pair_cl_fused_sliced
            w1p, w2p = _conv_weight_sliced(w1), _conv_weight_sliced(w2)
        else:
            op = ext.resblock_pair_cl_fused
        return op(
            x.contiguous(), w1p, _bias_f32(b1), w2p, _bias_f32(b2),
            k, dilation,
            _lens_i32(out_lens, x.device),
            accum.contiguous() if accum is not None else None,
            float(out_scale),
        )
    xt = leaky_conv1d_cl(x, w1, b1, padding=(k - 1) * dilation // 2,
                         dilation=dilation, pre_lrelu=0.1, out_lens=out_lens)
    y = leaky_conv1d_cl(xt, w2, b2, padding=(k - 1) // 2, pre_lrelu=0.1,
                        residual=x, out_lens=out_lens)
    if accum is not None:
        y = y + accum
    if out_scale != 1.0:
        y = y * out_scale
    if out_lens is not None and accum is not None:
        # the kernels zero masked rows AFTER the accum add; re-mask so
        # the oracle matches (accum rows past out_lens must not leak)
        idx = torch.arange(y.shape[1], device=y.device)
        y = y.masked_fill(
            (idx.unsqueeze(0) >= out_lens.to(y.device).unsqueeze(1))
            .unsqueeze(-1), 0)
    return y


def fused_gate_cl(
    x: torch.Tensor, g: Optional[torch.Tensor], n_channels: int
) -> torch.Tensor:
    """Channel-last WaveNet gate: x [B,F,2C] (+ g [B,2C] speaker bias or
    [B,F,2C]) -> tanh(xa+ga)*sigmoid(xb+gb) [B,F,C]."""
    if use_hip(x):
        ext = hip_ext(required=True)
        return ext.fused_gate_cl(x.contiguous(), g, n_channels)
    if g is not None:
        if g.dim() == 2:
            g = g.unsqueeze(1)
        x = x + g
    a, b = x[..., :n_channels], x[..., n_channels:]
    return torch.tanh(a) * torch.sigmoid(b)


def depthwise_conv1d_cl(
    x: torch.Tensor,  # [B, T, C]
    weight: torch.Tensor,  # [C, 1, k]
    bias: Optional[torch.Tensor],
    dilation: int,
    padding: int,
) -> torch.Tensor:
    """Channel-last depthwise Conv1d (DDSConv separable stage)."""
    if use_hip(x):
        ext = hip_ext(required=True)
        return ext.depthwise_cl(x.contiguous(), weight, bias, dilation,
                                padding)
    y = F.conv1d(x.transpose(1, 2), weight, bias, padding=padding,
                 dilation=dilation, groups=x.shape[-1])
    return y.transpose(1, 2)


def attn_relpos_cl(
    x: torch.Tensor,          # [B, T, C] channel-last (masked rows)
    attn_module,              # RelativeAttention (weights + rel tables)
    lengths: Optional[torch.Tensor],
) -> torch.Tensor:
    """Fused relative-position attention (csrc/attention_cl.hip): ONE
    QKV projection GEMM + ONE kernel (QK^T + banded rel-k logits +
    masked online softmax + PV + banded rel-v) + output projection.

    Replaces the 10+ launch matmul/pad/reshape chain of
    RelativeAttention.forward_cl; GPU-only (callers keep the torch
    oracle for CPU)."""
    ext = hip_ext(required=True)
    m = attn_module
    B, T, C = x.shape
    qkv_w = getattr(m, "_qkv_w", None)
    if qkv_w is None or qkv_w.dtype != x.dtype:
        # cache the fused [3C, C] projection (inference-only weights)
        m._qkv_w = torch.cat([
            m.conv_q.weight.squeeze(-1), m.conv_k.weight.squeeze(-1),
            m.conv_v.weight.squeeze(-1)]).to(x.dtype).contiguous()
        m._qkv_b = torch.cat([
            m.conv_q.bias, m.conv_k.bias, m.conv_v.bias]).to(x.dtype)
        m._rel_k = m.emb_rel_k[0].to(x.dtype).contiguous()
        m._rel_v = m.emb_rel_v[0].to(x.dtype).contiguous()
        qkv_w = m._qkv_w
    qkv = F.linear(x, qkv_w, m._qkv_b)  # [B, T, 3C]
    out = ext.attn_relpos_cl(
        qkv, m._rel_k, m._rel_v, _lens_i32(lengths, x.device),
        heads=m.n_heads, window=m.window_size,
        scale=m.head_dim ** -0.5)
    return F.linear(out, m.conv_o.weight.squeeze(-1), m.conv_o.bias)


def _chain_weights(resblock, dtype, device):
    """Stack the 6 permuted conv weights + biases of a ResBlock1 for the
    chain kernel (cached on the module)."""
    import torch as _t

    cache = getattr(resblock, "_chain_cache", None)
    if cache is not None and cache[0].dtype == _t.bfloat16:
        return cache
    ws = []
    bs = []
    for c1, c2 in zip(resblock.convs1, resblock.convs2):
        ws.append(_conv_weight_mfma(c1.weight))
        ws.append(_conv_weight_mfma(c2.weight))
        bs.append(c1.bias.float())
        bs.append(c2.bias.float())
    w_all = _t.stack(ws).contiguous().to(device)
    b_all = _t.stack(bs).contiguous().to(device)
    resblock._chain_cache = (w_all, b_all)
    return w_all, b_all


def resblock_chain_cl(
    resblock,                      # models.vits.ResBlock1
    x: torch.Tensor,               # [B, T, C]
    out_lens: Optional[torch.Tensor] = None,
    accum: Optional[torch.Tensor] = None,
    out_scale: float = 1.0,
) -> Optional[torch.Tensor]:
    """Whole-resblock fusion (3 conv pairs in one kernel, intermediates
    LDS-resident; csrc/resblock_cl.hip chain kernel).  Returns None when
    the geometry is unsupported (caller falls back to the pair loop).

    Numerics note: pair residuals reconstruct raw values through the
    exact-ish lrelu inverse from bf16 storage — negative residual values
    differ from the pair path by <= 2^-8 relative."""
    if not use_hip(x):
        return None
    k = resblock.convs1[0].kernel_size[0]
    dils = [c.dilation[0] for c in resblock.convs1]
    C = x.shape[-1]
    if len(dils) != 3:
        return None
    S0 = 128 + (k - 1) * (sum(dils) + 3)
    if not ((C == 32 and S0 <= 248) or (C == 64 and S0 <= 152)):
        return None
    if any(c.dilation[0] != 1 for c in resblock.convs2):
        return None
    ext = hip_ext(required=True)
    if not hasattr(ext, "resblock_chain_cl_fused"):
        return None
    w_all, b_all = _chain_weights(resblock, x.dtype, x.device)
    return ext.resblock_chain_cl_fused(
        x.contiguous(), w_all, b_all, k, dils[0], dils[1], dils[2],
        _lens_i32(out_lens, x.device),
        accum.contiguous() if accum is not None else None,
        float(out_scale))



def row_ln_cl(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
              eps: float = 1e-5,
              residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm over the channel-last row dim with fused residual:
    LN(x [+ residual]) * gamma + beta (csrc/elementwise.hip row_ln_cl).
    One launch instead of add + layer_norm."""
    if use_hip(x) and x.shape[-1] <= 512:
        ext = hip_ext(required=True)
        return ext.row_ln_cl(
            x.contiguous(),
            residual.contiguous() if residual is not None else None,
            gamma, beta, eps)
    if residual is not None:
        x = x + residual
    return F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)


# --------------------------------------------------------------------------- #
# fused glue of the engine's channel-last flow (csrc/elementwise.hip); bf16,
# GPU only.  Each is bit-identical to the eager chain it replaces; the
# engine (csrc/engine/vits_engine.cpp) is their caller, these wrappers exist
# so tests can reach the kernels.
# --------------------------------------------------------------------------- #
def wn_step(h: torch.Tensor, output: Optional[torch.Tensor],
            res_skip: torch.Tensor, mc: torch.Tensor, layer: int):
    """One WaveNet layer's residual/skip update IN PLACE on h and output
    ([B,F,H]); res_skip [B,F,2H] (layer 0 first / 1 middle) or [B,F,H]
    (layer 2 last); mc [B,F,1].  Returns output: freshly allocated for
    layer 0; for layer 2 it holds the masked result (the new h)."""
    return hip_ext(required=True).wn_step(h, output, res_skip, mc, layer)


def flow_split_rev(xc: torch.Tensor):
    """xc [B,F,C] -> the contiguous (x0, x1) halves of flip(xc, -1)."""
    x0, x1 = hip_ext(required=True).flow_split_rev(xc)
    return x0, x1


def coupling_tail(x0: torch.Tensor, x1: torch.Tensor, post: torch.Tensor,
                  mc: torch.Tensor, last: bool):
    """m = post*mc, x1 = (x1 - m)*mc, then either the next flow's flipped
    (x0, x1) pair (last=False) or cat(x0, x1) as one [B,F,C] (last=True)."""
    r = hip_ext(required=True).coupling_tail(x0, x1, post, mc, last)
    return r[0] if last else (r[0], r[1])


def dds_sep_ln_gelu(x: torch.Tensor, g: Optional[torch.Tensor],
                    mc: torch.Tensor, weight: torch.Tensor,
                    bias: torch.Tensor, gamma: torch.Tensor,
                    beta: torch.Tensor, dilation: int, eps: float = 1e-5):
    """DDS layer head on channel-last rows: t = x (+ g);
    y = gelu(LN(depthwise_k3(t*mc))).  weight [C,1,3] bf16; bias, gamma, beta
    f32 [C].  Returns (y, t); t is x itself without g."""
    r = hip_ext(required=True).dds_sep_ln_gelu(x, g, mc, weight, bias, gamma,
                                               beta, dilation, eps)
    return (r[0], r[1]) if g is not None else (r[0], x)


def ln_gelu_add(y: torch.Tensor, t: torch.Tensor, mc: torch.Tensor,
                gamma: torch.Tensor, beta: torch.Tensor, last: bool,
                eps: float = 1e-5) -> torch.Tensor:
    """DDS layer tail: t + gelu(LN(y)), times mc when last."""
    return hip_ext(required=True).ln_gelu_add(y, t, mc, gamma, beta, last,
                                              eps)


def rq_spline_inverse(inputs: torch.Tensor, uw: torch.Tensor,
                      uh: torch.Tensor, ud: torch.Tensor,
                      tail_bound: float = 5.0,
                      tail_kernel: bool = False) -> torch.Tensor:
    """The engine's dense, sync-free inverse rational-quadratic spline (no
    logabsdet): ATen ops on either device, or with tail_kernel (bf16, GPU,
    10 bins) one HIP kernel for everything after the softmax, cumsum and
    softplus."""
    return hip_ext(required=True).rq_spline_inverse(inputs, uw, uh, ud,
                                                    tail_bound, tail_kernel)


# --------------------------------------------------------------------------- #
# batched prosody: rate / pitch / volume on [B, N] f32 rows with per-row
# parameters (csrc/prosody.hip).  The CPU path calls the NumPy functions of
# audio.prosody row by row and is the oracle; every length on both paths
# comes from audio.prosody.wsola_plan / resample_out_len.
# --------------------------------------------------------------------------- #
def _row_lengths(lengths, B: int):
    """Per-row lengths as Python ints (host arithmetic decides every
    output length)."""
    if isinstance(lengths, torch.Tensor):
        lengths = lengths.detach().cpu().tolist()
    out = [int(v) for v in lengths]
    assert len(out) == B, "one length per row"
    return out


def _per_row(v, B: int, default: float = 1.0):
    if v is None:
        return [default] * B
    if isinstance(v, (int, float)):
        return [float(v)] * B
    out = [float(t) for t in v]
    assert len(out) == B, "one parameter per row"
    return out


def _rows_from_numpy(rows, device) -> tuple:
    """List of 1-D f32 arrays -> zero-padded [B, max_len] tensor + lengths."""
    import numpy as np

    lens = [int(r.shape[0]) for r in rows]
    y = np.zeros((len(rows), max(lens, default=0)), dtype=np.float32)
    for b, r in enumerate(rows):
        y[b, : lens[b]] = r
    return (torch.from_numpy(y).to(device),
            torch.tensor(lens, dtype=torch.long))


def _i32(vals, device) -> torch.Tensor:
    return torch.tensor(vals, dtype=torch.int32, device=device)


def resample_linear_rows(x: torch.Tensor, lengths, ratio):
    """Per-row linear resampling of x [B, N] f32 by `ratio[b]` (output
    length = lengths[b]/ratio[b]); rows with |ratio-1| < 1e-6 and empty
    rows are copied.  Returns (y [B, max out_len] zero-padded, out_lengths)."""
    from ..audio import prosody as P

    B = x.shape[0]
    lens = _row_lengths(lengths, B)
    ratios = _per_row(ratio, B)
    if not use_hip(x):
        xn = x.detach().cpu().numpy()
        return _rows_from_numpy(
            [P.resample_linear(xn[b, : lens[b]], ratios[b])
             for b in range(B)], x.device)
    ext = hip_ext(required=True)
    out = [n if (n == 0 or abs(r - 1.0) < 1e-6) else P.resample_out_len(n, r)
           for n, r in zip(lens, ratios)]
    y = ext.resample_linear_rows(
        x.contiguous(), _i32(lens, x.device), _i32(out, x.device),
        max(out, default=0))
    return y, torch.tensor(out, dtype=torch.long)


def _wsola_rows_hip(x: torch.Tensor, lens, plans, gain, frame_geom):
    """Launch csrc/prosody.hip wsola_rows.  plans[b] is None (pass-through
    row: copied and scaled) or a wsola_plan tuple; frame_geom = (frame, half,
    search), shared by the batch.  Returns (y, targets, out_lengths)."""
    from ..audio.window import hann_window

    ext = hip_ext(required=True)
    frame, half, search = frame_geom
    dev = x.device
    hop = [p[3] if p is not None else 1.0 for p in plans]
    nfr = [p[4] if p is not None else 0 for p in plans]
    out = [p[5] if p is not None else n for p, n in zip(plans, lens)]
    # the host's own window, bit for bit (never recomputed on the device)
    win = torch.from_numpy(hann_window(frame).copy()).to(dev)
    y, targets = ext.wsola_rows(
        x.contiguous(), _i32(lens, dev),
        torch.tensor(hop, dtype=torch.float64, device=dev),
        _i32(nfr, dev), _i32(out, dev), win, half, search,
        torch.tensor(gain, dtype=torch.float32, device=dev),
        max(out, default=0), max(max(nfr, default=0), 1))
    return y, targets, torch.tensor(out, dtype=torch.long)


def wsola_rows(x: torch.Tensor, lengths, sample_rate: int, speed, gain=None,
               frame_ms: float = 30.0, search_ms: float = 10.0,
               return_targets: bool = False):
    """Per-row WSOLA time stretch of x [B, N] f32 (duration/speed[b], pitch
    preserved), then a per-row gain.  Rows with |speed-1| < 1e-3, empty
    rows and rows shorter than one frame are copied (and scaled).
    Returns (y zero-padded, out_lengths[, targets [B, K] i32 — the start
    of every analysis frame, -1 in unused slots; HIP path only])."""
    from ..audio import prosody as P

    B = x.shape[0]
    lens = _row_lengths(lengths, B)
    speeds = _per_row(speed, B)
    gains = _per_row(gain, B)
    frame, half, search = P.wsola_plan(0, 1.0, sample_rate, frame_ms,
                                       search_ms)[:3]
    if not use_hip(x):
        import numpy as np

        assert not return_targets, "targets are a HIP-path output"
        xn = x.detach().cpu().numpy()
        rows = []
        for b in range(B):
            r = xn[b, : lens[b]]
            if P.wsola_is_passthrough(lens[b], speeds[b], frame):
                r = r.copy()
            else:
                r = P.time_stretch_wsola(r, speeds[b], sample_rate,
                                         frame_ms, search_ms)
            if gains[b] != 1.0:
                r = r * np.float32(gains[b])
            rows.append(r)
        return _rows_from_numpy(rows, x.device)
    plans = [None if P.wsola_is_passthrough(n, s, frame)
             else P.wsola_plan(n, s, sample_rate, frame_ms, search_ms)
             for n, s in zip(lens, speeds)]
    y, targets, out = _wsola_rows_hip(x, lens, plans, gains,
                                      (frame, half, search))
    return (y, out, targets) if return_targets else (y, out)


def apply_prosody_rows(x: torch.Tensor, lengths, sample_rate: int,
                       speed=None, volume=None, pitch=None):
    """Batched audio.prosody.apply_prosody: x [B, N] f32 rows of
    lengths[b] samples, per-row speed / volume / pitch.  Same composition
    and thresholds: pitch = resample by pitch then stretch by 1/pitch; then
    stretch by speed; then gain.  Returns (y [B, max out] zero-padded,
    out_lengths).  The gain rides in the last kernel that runs; a
    volume-only batch launches only a scale."""
    from ..audio import prosody as P

    B = x.shape[0]
    lens = _row_lengths(lengths, B)
    speeds, vols, pitches = (_per_row(speed, B), _per_row(volume, B),
                             _per_row(pitch, B))
    do_pitch = [abs(p - 1.0) >= 1e-3 for p in pitches]
    do_speed = [abs(s - 1.0) >= 1e-3 for s in speeds]
    do_gain = [abs(v - 1.0) >= 1e-6 for v in vols]
    if not use_hip(x):
        import numpy as np

        frame = P.wsola_plan(0, 1.0, sample_rate)[0]

        def stretch(r, s):
            if P.wsola_is_passthrough(len(r), s, frame):
                return r.copy()
            return P.time_stretch_wsola(r, s, sample_rate)

        xn = x.detach().cpu().numpy().astype(np.float32, copy=False)
        rows = []
        for b in range(B):
            r = xn[b, : lens[b]]
            if do_pitch[b]:
                r = stretch(P.resample_linear(r, pitches[b]),
                            1.0 / pitches[b])
            if do_speed[b]:
                r = stretch(r, speeds[b])
            if do_gain[b]:
                r = r * np.float32(vols[b])
            rows.append(r)
        return _rows_from_numpy(rows, x.device)

    gains = [v if g else 1.0 for v, g in zip(vols, do_gain)]
    ones = [1.0] * B
    y, cur = x, lens
    any_speed = any(do_speed)
    if any(do_pitch):
        y, out = resample_linear_rows(
            y, cur, [p if d else 1.0 for p, d in zip(pitches, do_pitch)])
        cur = out.tolist()
        y, out = wsola_rows(
            y, cur, sample_rate,
            [1.0 / p if d else 1.0 for p, d in zip(pitches, do_pitch)],
            gain=ones if any_speed else gains)
        cur = out.tolist()
    if any_speed:
        y, out = wsola_rows(
            y, cur, sample_rate,
            [s if d else 1.0 for s, d in zip(speeds, do_speed)], gain=gains)
        cur = out.tolist()
    elif not any(do_pitch) and any(do_gain):
        ext = hip_ext(required=True)
        y = ext.scale_rows(
            y.contiguous(), _i32(cur, y.device),
            torch.tensor(gains, dtype=torch.float32, device=y.device))
    return y, torch.tensor(cur, dtype=torch.long)


# --------------------------------------------------------------------------- #
# batched PCM: [B, N] f32 / bf16 rows -> peak-normalised int16 with per-row
# lengths and appended silence (csrc/pcm.hip).  The CPU path calls
# audio.samples.to_i16 row by row and is the oracle; the kernels match it
# bit for bit.
# --------------------------------------------------------------------------- #
PCM_TILE = 4096  # elements per workgroup of the peak kernel (csrc/pcm.hip)


def _per_row_int(v, B: int):
    if v is None:
        return [0] * B
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().tolist()
    if isinstance(v, (int, float)):
        return [int(v)] * B
    out = [int(t) for t in v]
    assert len(out) == B, "one parameter per row"
    return out


def pcm16_rows(x: torch.Tensor, lengths, silence=None,
               peak_normalize: bool = True):
    """int16 PCM of x [B, N] (f32 or bf16) rows of lengths[b] samples, as
    audio.samples.to_i16 gives it: scale = 32767/peak of the row (0 for a
    peak <= 1e-8; 32767 without peak_normalize), clamp, truncate.  `silence`
    (samples, per row or one int) is appended as zeros.  Returns
    (pcm int16 [B, N_out], out_lengths) with out_lengths[b] = lengths[b] +
    silence[b] and N_out = max(out_lengths) rounded up to a multiple of 8
    (aligned rows); columns past lengths[b] are 0."""
    B = x.shape[0]
    lens = _row_lengths(lengths, B)
    assert all(0 <= n <= x.shape[1] for n in lens), "length outside the row"
    sil = _per_row_int(silence, B)
    assert all(s >= 0 for s in sil), "negative silence"
    out = [n + s for n, s in zip(lens, sil)]
    n_out = _round_up(max(out, default=0), 8)
    out_lengths = torch.tensor(out, dtype=torch.long)
    if not use_hip(x):
        import numpy as np

        from ..audio.samples import to_i16

        xn = x.detach().float().cpu().numpy()
        y = np.zeros((B, n_out), dtype=np.int16)
        for b in range(B):
            y[b, : lens[b]] = to_i16(xn[b, : lens[b]], peak_normalize)
        return torch.from_numpy(y).to(x.device), out_lengths
    ext = hip_ext(required=True)
    if x.shape[1] > 1 and x.stride(1) != 1:
        x = x.contiguous()
    pcm, _peaks = ext.pcm16_rows(x, _i32(lens, x.device), n_out,
                                 bool(peak_normalize))
    return pcm, out_lengths


def _per_row_law(law, B: int):
    from ..audio.g711 import check_law

    if isinstance(law, str):
        return [check_law(law)] * B
    out = [check_law(v) for v in law]
    assert len(out) == B, "one law per row"
    return out


def g711_rows(x: torch.Tensor, lengths, silence=None, law="ulaw",
              peak_normalize: bool = True):
    """G.711 codes of x [B, N] (f32 or bf16) rows of lengths[b] samples:
    audio.g711.encode of what pcm16_rows gives for the row, without the
    int16 in between.  `law` is "ulaw" or "alaw", one name or one per row;
    `silence` (samples, per row or one int) is appended as the row's code of
    sample 0.  Returns (codes uint8 [B, N_out], out_lengths) with
    out_lengths[b] = lengths[b] + silence[b] and N_out = max(out_lengths)
    rounded up to a multiple of 16 (aligned rows); columns past lengths[b]
    are g711.ZERO[law[b]]."""
    from ..audio import g711

    B = x.shape[0]
    lens = _row_lengths(lengths, B)
    assert all(0 <= n <= x.shape[1] for n in lens), "length outside the row"
    sil = _per_row_int(silence, B)
    assert all(s >= 0 for s in sil), "negative silence"
    laws = _per_row_law(law, B)
    out = [n + s for n, s in zip(lens, sil)]
    n_out = _round_up(max(out, default=0), 16)
    out_lengths = torch.tensor(out, dtype=torch.long)
    if not use_hip(x):
        import numpy as np

        from ..audio.samples import to_i16

        xn = x.detach().float().cpu().numpy()
        y = np.empty((B, n_out), dtype=np.uint8)
        for b in range(B):
            y[b, lens[b]:] = g711.ZERO[laws[b]]
            y[b, : lens[b]] = g711.encode(
                to_i16(xn[b, : lens[b]], peak_normalize), laws[b])
        return torch.from_numpy(y).to(x.device), out_lengths
    ext = hip_ext(required=True)
    if x.shape[1] > 1 and x.stride(1) != 1:
        x = x.contiguous()
    # lengths and laws (checked above: 0 or 1) go up in one copy
    par = _i32([lens, [g711.LAWS.index(v) for v in laws]], x.device)
    codes, _peaks = ext.g711_rows(x, par[0], par[1], n_out,
                                  bool(peak_normalize))
    return codes, out_lengths


# --------------------------------------------------------------------------- #
# batched output sample-rate conversion (csrc/resample.hip): the polyphase
# FIR of audio.resample on [B, N] f32 / bf16 rows.  The CPU path calls
# audio.resample.resample_poly row by row and is the oracle; the kernel adds
# the same products in f32 and stays within K * 2^-23 * S * max|x| of it.
# --------------------------------------------------------------------------- #
RESAMPLE_TILE = 256  # outputs per workgroup (csrc/resample.hip)

_RESAMPLE_BANKS: dict = {}
_RESAMPLE_BANKS_LOCK = threading.Lock()


def _resample_bank(d, device) -> torch.Tensor:
    """The filter in the kernel's [K][L] layout, uploaded once per rate pair
    and device."""
    key = (d.rate_in, d.rate_out, str(device))
    with _RESAMPLE_BANKS_LOCK:
        bank = _RESAMPLE_BANKS.get(key)
        if bank is None:
            import numpy as np

            flat = np.ascontiguousarray(d.bank.T).reshape(-1)
            bank = torch.from_numpy(flat.copy()).to(device)
            _RESAMPLE_BANKS[key] = bank
    return bank


def resample_rows(x: torch.Tensor, lengths, rate_in: int, rate_out):
    """Rows of x [B, N] (f32 or bf16) with lengths[b] samples at rate_in ->
    f32 rows at rate_out, as audio.resample.resample_poly gives them.
    Returns (y [B, max out_len] zero-padded, out_lengths).  rate_out equal
    to rate_in, or None, is the identity: x itself and no launch."""
    from ..audio import resample as R

    B = x.shape[0]
    lens = _row_lengths(lengths, B)
    assert all(0 <= n <= x.shape[1] for n in lens), "length outside the row"
    if R.is_identity(rate_in, rate_out):
        return x, torch.tensor(lens, dtype=torch.long)
    d = R.design(rate_in, rate_out)
    out = [-(-n * d.L // d.M) for n in lens]
    if not use_hip(x):
        xn = x.detach().float().cpu().numpy()
        return _rows_from_numpy(
            [R.resample_poly(xn[b, : lens[b]], rate_in, rate_out)
             for b in range(B)], x.device)
    ext = hip_ext(required=True)
    y = ext.resample_poly_rows(
        x.contiguous(), _i32(lens, x.device), _i32(out, x.device),
        _resample_bank(d, x.device), d.L, d.M, d.H, max(out, default=0))
    return y, torch.tensor(out, dtype=torch.long)


# --------------------------------------------------------------------------- #
# batched realtime streams (csrc/stream.hip): pack ragged latent windows into
# one decode batch, and trim / crossfade the decoded rows per stream.  Pure
# data movement plus one rounded multiply-add per seam sample: the CPU paths
# (slicing, audio.samples.crossfade) are the oracle and the kernels match
# them bit for bit.
# --------------------------------------------------------------------------- #
SEAM_CROSSFADE = 42  # samples of one kept tail (csrc/stream.hip SEAM_XF)


def gather_windows(zs, src, row, start, length, l_max: int) -> torch.Tensor:
    """Pack windows of several latent tensors into one decode batch.
    `zs`: list of [b_i, C, F_i] tensors (one dtype, one C; separate
    allocations are fine).  Output row r is zs[src[r]][row[r], :, start[r] :
    start[r] + length[r]] followed by zeros up to `l_max`: [R, C, l_max].
    The matching mask is t < length[r].  One launch on the GPU."""
    zs = list(zs)
    assert zs, "no source tensors"
    R = len(src)
    src, row, start, length = (_per_row_int(v, R)
                               for v in (src, row, start, length))
    l_max = int(l_max)
    z0 = zs[0]
    C = z0.shape[1]
    for z in zs:
        assert z.dim() == 3 and z.shape[1] == C and z.dtype == z0.dtype, \
            "sources differ in dtype or C"
    for r in range(R):
        assert 0 <= src[r] < len(zs), "src out of range"
        z = zs[src[r]]
        assert 0 <= row[r] < z.shape[0], "row out of range"
        assert (start[r] >= 0 and 0 <= length[r] <= l_max
                and start[r] + length[r] <= z.shape[2]), \
            "window outside its source row"
    if not use_hip(z0):
        out = torch.zeros((R, C, l_max), dtype=z0.dtype, device=z0.device)
        for r in range(R):
            out[r, :, : length[r]] = zs[src[r]][
                row[r], :, start[r] : start[r] + length[r]]
        return out
    ext = hip_ext(required=True)
    zs = [z if (z.shape[2] <= 1 or z.stride(2) == 1) else z.contiguous()
          for z in zs]
    return ext.gather_windows(zs, src, row, start, length, l_max)


def stream_seam_rows(wav: torch.Tensor, lo, hi, ext, prev_ext, slot,
                     tails_in: torch.Tensor, ramp: torch.Tensor,
                     tails_out: Optional[torch.Tensor] = None):
    """Trim and crossfade R decoded stream chunks at once (the per-stream
    trim_and_emit of VitsVoice._stream_decode).  `wav` [R, 1, N] (or [R, N])
    is the decoder output in its dtype, widened to f32 as .float() does.
    Per row: cur = wav[r, lo : hi + ext]; if prev_ext > 0 its first prev_ext
    samples become tail[j] * ramp[n-1-j] + cur[j] * ramp[j] with tail =
    tails_in[slot[r]], n = prev_ext; out[r] = cur[: len(cur) - ext] and
    tails_out[slot[r]] = cur[len(cur) - ext :].  `ramp` is
    audio.samples._quarter_sine_ramp(SEAM_CROSSFADE) on wav's device.
    Returns (out f32 [R, n_out], out_len [R], tails_out): n_out is the longest
    row rounded up to a multiple of 8 (ops.pcm16_rows takes out and out_len as
    they are), columns past out_len[r] are 0, and slots not named keep their
    contents.  `tails_out` defaults to a copy of tails_in; passing tails_in
    itself updates it in place (a row's old tail is read before its new one
    is written)."""
    if wav.dim() == 3:
        assert wav.shape[1] == 1, "wav must be [R, 1, N]"
        wav = wav[:, 0, :]
    R, N = wav.shape
    lo, hi, ex, pe, slot = (_per_row_int(v, R)
                            for v in (lo, hi, ext, prev_ext, slot))
    S = tails_in.shape[0]
    assert tails_in.shape == (S, SEAM_CROSSFADE) \
        and tails_in.dtype == torch.float32, "tails must be f32 [S, 42]"
    assert ramp.shape == (SEAM_CROSSFADE,) and ramp.dtype == torch.float32
    for r in range(R):
        assert pe[r] in (0, SEAM_CROSSFADE), "prev_ext must be 0 or 42"
        assert ex[r] in (0, SEAM_CROSSFADE), "ext must be 0 or 42"
        assert 0 <= lo[r] <= hi[r] and hi[r] + ex[r] <= N, \
            "[lo, hi + ext) outside the row"
        assert hi[r] - lo[r] >= pe[r], "chunk shorter than its seam"
        assert 0 <= slot[r] < S, "slot out of range"
    assert len(set(slot)) == R, "rows must name distinct slots"
    out_len = [h - l for l, h in zip(lo, hi)]
    n_out = _round_up(max(out_len, default=0), 8)
    out_lengths = torch.tensor(out_len, dtype=torch.long)
    if tails_out is None:
        tails_out = tails_in.clone()
    assert tails_out.shape == tails_in.shape \
        and tails_out.dtype == torch.float32
    if not use_hip(wav):
        import numpy as np

        from ..audio.samples import crossfade

        wn = wav.detach().float().cpu().numpy()
        tin = tails_in.detach().cpu().numpy()
        out = np.zeros((R, n_out), dtype=np.float32)
        new_tails = {}
        for r in range(R):
            cur = wn[r, lo[r] : hi[r] + ex[r]]
            if pe[r]:
                cur = crossfade(tin[slot[r]], cur, pe[r])
            out[r, : out_len[r]] = cur[: out_len[r]]
            if ex[r]:
                new_tails[slot[r]] = cur[out_len[r] :].copy()
        for s, t in new_tails.items():
            tails_out[s] = torch.from_numpy(t).to(tails_out.device)
        return torch.from_numpy(out).to(wav.device), out_lengths, tails_out
    hext = hip_ext(required=True)
    assert hext.SEAM_CROSSFADE == SEAM_CROSSFADE
    if N > 1 and wav.stride(1) != 1:
        wav = wav.contiguous()
    out = hext.stream_seam_rows(wav, lo, hi, ex, pe, slot, tails_in,
                                tails_out, ramp, n_out)
    return out, out_lengths, tails_out


# --------------------------------------------------------------------------- #
# streaming prosody (csrc/prosody.hip, the *_stream_rows kernels): rate /
# pitch / volume for realtime streams, one launch per stage per round for all
# live streams, state on the device indexed by the streams' tail slots.  The
# rules and every length come from audio.prosody (StreamProsodyPlan);
# StreamProsody.push row by row is the CPU path and the oracle.
# --------------------------------------------------------------------------- #
class ProsodyStreamState:
    """Device state of streaming prosody for one sample rate, indexed by
    slot: per WSOLA stage (0: the pitch chain's stretch, 1: speed) a carry of
    seg_cap samples and the half-frame tail of the last chosen frame, plus
    the resample stage's one-sample carry.  A stream's first push names no
    carry and no tail, so a slot needs no cleaning between streams."""

    def __init__(self, sample_rate: int, device):
        from ..audio import prosody as P
        from ..audio.window import hann_window

        self.sample_rate = int(sample_rate)
        self.device = torch.device(device)
        self.frame, self.half, self.search = P.wsola_plan(
            0, 1.0, sample_rate)[:3]
        self.seg_cap = _round_up(
            P.wsola_seg_cap(self.frame, self.search), 4)
        # the host's own window, bit for bit (never recomputed on the device)
        self.window = torch.from_numpy(
            hann_window(self.frame).copy()).to(self.device)
        self.slots = 0
        self.rs_carry = None
        self.carry = [None, None]
        self.tails = [None, None]

    def reserve(self, slots: int) -> None:
        """Grow to at least `slots` slots, keeping what live streams hold."""
        from ..audio.prosody import RESAMPLE_CARRY

        if slots <= self.slots:
            return

        def grown(old, width):
            new = torch.zeros((slots, width), dtype=torch.float32,
                              device=self.device)
            if old is not None:
                new[: old.shape[0]].copy_(old)
            return new

        self.rs_carry = grown(self.rs_carry, RESAMPLE_CARRY)
        self.carry = [grown(c, self.seg_cap) for c in self.carry]
        self.tails = [grown(t, self.half) for t in self.tails]
        self.slots = slots


def resample_stream_rows(x: torch.Tensor, lengths, pushes, slots,
                         carry: torch.Tensor):
    """One round of the streaming resample stage on the device.  x [R, N]
    f32 chunk rows of lengths[r] samples; pushes[r] is the
    audio.prosody.ResamplePush of the row's plan, or None for a row that is
    copied; carry f32 [S, 1] is updated in place at slots[r].  Returns
    (y [R, n_out] zero-padded, n_out a multiple of 8, out_lengths)."""
    R = x.shape[0]
    lens = _row_lengths(lengths, R)
    slots = _per_row_int(slots, R)
    par, out = [], []
    for n, p, s in zip(lens, pushes, slots):
        if p is None or p.copy:
            par += [s, n, 0, 0, 0, n, n, 0, n, 1, n, 0]
            out.append(n)
            continue
        assert p.m == n, "the plan was pushed another length"
        par += [s, p.m, p.a0, p.in_pos, p.carry_len, p.n, p.n_out, p.e0,
                p.e1, 0, p.keep_pos, p.keep_len]
        out.append(p.e1 - p.e0)
    n_out = max(_round_up(max(out, default=0), 8), 8)
    y = hip_ext(required=True).resample_stream_rows(
        x.contiguous(), par, carry, n_out)
    return y, torch.tensor(out, dtype=torch.long)


def wsola_stream_rows(x: torch.Tensor, lengths, pushes, slots,
                      carry: torch.Tensor, tails: torch.Tensor,
                      window: torch.Tensor, half: int, search: int,
                      gain=None, return_targets: bool = False):
    """One round of a streaming WSOLA stage on the device.  x [R, N] f32
    chunk rows of lengths[r] samples; pushes[r] is the
    audio.prosody.WsolaPush of the row's plan, or None for a row that is
    copied (and scaled by gain[r]); carry f32 [S, seg_cap] and tails f32
    [S, half] are updated in place at slots[r].  Returns (y [R, n_out]
    zero-padded, n_out a multiple of 8, out_lengths[, targets [R, K] i32:
    the global start of each frame run this round, -1 in unused slots])."""
    R = x.shape[0]
    lens = _row_lengths(lengths, R)
    slots = _per_row_int(slots, R)
    gains = _per_row(gain, R)
    par, hop, out, nks = [], [], [], [1]
    for n, p, s in zip(lens, pushes, slots):
        if p is None or p.passthrough:
            par += [s, n, 0, 0, 0, 0, 0, n, 0, n, 1, n, 0]
            hop.append(1.0)
            out.append(n)
            continue
        assert p.m == n, "the plan was pushed another length"
        par += [s, p.m, p.a0, p.in_pos, p.carry_len, p.k0, p.nk, p.n, p.e0,
                p.e1, 2 if p.closing else 0, p.keep_pos, p.keep_len]
        hop.append(p.ana_hop)
        out.append(p.e1 - p.e0)
        nks.append(p.nk)
    n_out = max(_round_up(max(out, default=0), 8), 8)
    y, targets = hip_ext(required=True).wsola_stream_rows(
        x.contiguous(), par, hop, gains, carry, tails, window, half, search,
        n_out, max(nks))
    out = torch.tensor(out, dtype=torch.long)
    return (y, out, targets) if return_targets else (y, out)


def prosody_stream_rows(x: torch.Tensor, lengths, procs, slots,
                        state: Optional[ProsodyStreamState], last=None):
    """One round of streaming prosody for R streams: x [R, N] f32 holds each
    stream's next plain chunk (lengths[r] samples), procs[r] its
    audio.prosody.StreamProsody (None: the row is copied), slots[r] its slot
    in `state`, last[r] whether this is the stream's final chunk.  Returns
    (y [R, n_out] zero-padded, n_out a multiple of 8, out_lengths); a row
    may emit nothing this round.  Per row the stages are those of
    apply_prosody_rows on that row alone: resample by pitch, WSOLA by
    1/pitch, WSOLA by speed, the gain in the row's last stage (a volume-only
    row is scaled).  On the CPU each row goes through StreamProsody.push."""
    R = x.shape[0]
    lens = _row_lengths(lengths, R)
    last = [False] * R if last is None else [bool(v) for v in last]
    assert len(procs) == R and len(last) == R
    if not use_hip(x):
        import numpy as np

        xn = x.detach().cpu().numpy()
        rows = [xn[r, : lens[r]].copy() if procs[r] is None
                else procs[r].push(xn[r, : lens[r]], last[r])
                for r in range(R)]
        out = [int(r.shape[0]) for r in rows]
        y = np.zeros((R, max(_round_up(max(out, default=0), 8), 8)),
                     dtype=np.float32)
        for r, row in enumerate(rows):
            y[r, : out[r]] = row
        return (torch.from_numpy(y).to(x.device),
                torch.tensor(out, dtype=torch.long))
    assert state is not None, "device streams need a ProsodyStreamState"
    plans = [None if p is None or p.plan.is_noop else p.plan for p in procs]
    steps = [None if pl is None else pl.push(n, l)
             for pl, n, l in zip(plans, lens, last)]
    y, cur = x, torch.tensor(lens, dtype=torch.long)
    if not any(pl is not None for pl in plans):
        return y, cur
    slots = _per_row_int(slots, R)
    assert max(slots) < state.slots, "slot outside the reserved state"
    if any(pl is not None and pl.do_pitch for pl in plans):
        y, cur = resample_stream_rows(
            y, cur, [s.resample if s else None for s in steps], slots,
            state.rs_carry)
        y, cur = wsola_stream_rows(
            y, cur, [s.wsola_pitch if s else None for s in steps], slots,
            state.carry[0], state.tails[0], state.window, state.half,
            state.search,
            gain=[pl.gain if pl is not None and pl.do_pitch
                  and not pl.do_speed else 1.0 for pl in plans])
    if any(pl is not None and (pl.do_speed or not pl.do_pitch)
           for pl in plans):
        y, cur = wsola_stream_rows(
            y, cur, [s.wsola_speed if s else None for s in steps], slots,
            state.carry[1], state.tails[1], state.window, state.half,
            state.search,
            gain=[pl.gain if pl is not None
                  and (pl.do_speed or not pl.do_pitch) else 1.0
                  for pl in plans])
    return y, cur


# --------------------------------------------------------------------------- #
# streaming output sample-rate conversion (csrc/resample.hip,
# resample_poly_stream_rows): the polyphase FIR of audio.resample for realtime
# streams, one launch per round for all live streams of one output rate, the
# carry on the device indexed by the streams' tail slots.  Every length comes
# from audio.resample.PolyStreamPlan; PolyStream.push row by row is the CPU
# path.  The kernel's tap loop is resample_rows' own, so a stream's chunks
# concatenate to resample_rows of its whole input bit for bit.
# --------------------------------------------------------------------------- #
class PolyStreamState:
    """Device state of streaming sample-rate conversion for one rate pair,
    indexed by slot: `carry` f32 [S, 2, Kc], Kc = round_up(K - 1, 4).  The
    two buffers of a slot are used in turn (a push reads one and writes the
    other, see the kernel).  A stream's first push names no carry, so a slot
    needs no cleaning between streams."""

    def __init__(self, rate_in: int, rate_out: int, device):
        from ..audio import resample as R

        self.d = R.design(rate_in, rate_out)
        self.rate_in, self.rate_out = self.d.rate_in, self.d.rate_out
        self.device = torch.device(device)
        self.carry_cap = _round_up(self.d.K - 1, 4)
        self.slots = 0
        self.carry = None

    def reserve(self, slots: int) -> None:
        """Grow to at least `slots` slots, keeping what live streams hold."""
        if slots <= self.slots:
            return
        new = torch.zeros((slots, 2, self.carry_cap), dtype=torch.float32,
                          device=self.device)
        if self.carry is not None:
            new[: self.carry.shape[0]].copy_(self.carry)
        self.carry = new
        self.slots = slots


def resample_poly_stream_rows(x: torch.Tensor, lengths, streams, slots,
                              state: Optional[PolyStreamState], last=None):
    """One round of streaming sample-rate conversion for R streams: x [R, N]
    f32 holds each stream's next chunk (lengths[r] samples), streams[r] its
    audio.resample.PolyStream (None: the row is copied), slots[r] its slot
    in `state`, last[r] whether this is the stream's final chunk.  All
    streams named share state's rate pair.  Returns (y [R, n_out]
    zero-padded, n_out a multiple of 8 and at least 8, out_lengths); a row
    may emit nothing this round.  Over its rounds a row's outputs are those
    of resample_rows on its whole input.  On the CPU each row goes through
    PolyStream.push."""
    R = x.shape[0]
    lens = _row_lengths(lengths, R)
    assert all(0 <= n <= x.shape[1] for n in lens), "length outside the row"
    last = [False] * R if last is None else [bool(v) for v in last]
    assert len(streams) == R and len(last) == R
    if not use_hip(x):
        import numpy as np

        xn = x.detach().cpu().numpy()
        rows = [xn[r, : lens[r]].copy() if streams[r] is None
                else streams[r].push(xn[r, : lens[r]], last[r])
                for r in range(R)]
        out = [int(r.shape[0]) for r in rows]
        y = np.zeros((R, max(_round_up(max(out, default=0), 8), 8)),
                     dtype=np.float32)
        for r, row in enumerate(rows):
            y[r, : out[r]] = row
        return (torch.from_numpy(y).to(x.device),
                torch.tensor(out, dtype=torch.long))
    if not any(s is not None for s in streams):
        return x, torch.tensor(lens, dtype=torch.long)
    assert state is not None, "device streams need a PolyStreamState"
    slots = _per_row_int(slots, R)
    d = state.d
    for s in streams:
        assert s is None or (s.rate_in, s.rate_out) == (
            state.rate_in, state.rate_out), "stream of another rate pair"
    assert max(slots) < state.slots, "slot outside the reserved state"
    par, out = [], []
    for n, s, slot, l in zip(lens, streams, slots, last):
        if s is None:
            par += [slot, n, 0, 0, 0, n, 0, n, 1, n, 0, 0]
            out.append(n)
            continue
        p = s.plan.push(n, l)
        par += [slot, p.m, p.a0, p.carry_pos, p.carry_len, p.n, p.e0, p.e1,
                0, p.keep_pos, p.keep_len, p.parity]
        out.append(p.e1 - p.e0)
    n_out = max(_round_up(max(out, default=0), 8), 8)
    y = hip_ext(required=True).resample_poly_stream_rows(
        x.contiguous(), par, state.carry, _resample_bank(d, x.device),
        d.L, d.M, d.H, n_out)
    return y, torch.tensor(out, dtype=torch.long)
