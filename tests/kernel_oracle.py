"""fp64 references and derived per-element error bounds for the
channel-last HIP kernels (csrc/conv1d_cl.hip, csrc/resblock_cl.hip,
csrc/elementwise.hip) and the channel-first conv family (csrc/conv1d.hip:
``conv_ct_oracle``, ``convt_ct_oracle`` — same building blocks, same error
model).

Every reference runs in torch.float64 on CPU and mirrors the kernel's
DOCUMENTED rounding points and nothing else:

  conv input      the pre-activation LeakyReLU is applied in f32 and the
                  result rounded to bf16 before the reduction (the LDS
                  staging loop does exactly that); weights are bf16
  pair xt         the resblock-pair intermediate lrelu(conv1+b1) lives in
                  LDS as bf16: rounded to bf16
  output          rounded to the output dtype

Error model (``elementwise_bound``)
-----------------------------------
With u32 = 2^-24 (f32 unit roundoff), for one output element

    y = act( sum_{K terms} x'·w + bias ) + residual (+ accum)

the operands are bf16, so every product x'·w is exact in f32.  Any f32
summation order over n terms has error <= n·u32·A with

    A = sum |x'|·|w| + |bias| + |residual| + |accum|

(A is computed by the same reference routine on absolute values).  The
activations are 1-Lipschitz (LeakyReLU with slope <= 1, tanh), so the
accumulation error passes through them unamplified.  Then

    err = n·u32·A                        n = K + 3 (bias, act multiply,
                                             residual add)
        + TANH_ATOL           (tanh only) 2 ulp of f32 at 1.0 = 2^-22: the
                                          HIP/CUDA device-math accuracy
                                          tables give tanhf <= 2 ulp, and
                                          |tanh| <= 1
        + u_out·|ref|                     output rounding: u_out = 2^-8 for
                                          bf16, 2^-23 for f32

    bound = HEADROOM · err,   HEADROOM = 2

HEADROOM is the only slack; it is applied once, in ``elementwise_bound``.
It covers the reference itself being rounded to the output dtype (kernel
and reference may legitimately land on neighbouring representable
values) and second-order terms.  Rows masked by ``out_lens`` get ref = 0
and bound = 0: they must be exactly zero.

Resblock pair (two stages): stage 1 gets

    E1 = (K+2)·u32·A1 + 2^-7·|xt|        (one bf16 ulp of the intermediate:
                                          a tiny f32 difference may flip
                                          the bf16 rounding of xt)

and E1 is pushed through stage 2 by the same abs-convolution:

    err = |scale|·( (K+4)·u32·A2 + conv(E1, |w2|) ) + u_out·|ref|

No constant here is taken from what the kernels were measured to produce.
A is evaluated in f32 (it only scales a bound; its own 1e-7 relative
error is immaterial) to keep the fp64 work to the reference itself.

Elementwise ops (gate, prior sample, depthwise) have their own short
derivations next to their references.  The layer norms use the project's
existing f32 tolerance, 1e-4 of max|ref| (tests/test_gpu_ops.py), plus
the output rounding term for bf16 outputs.
"""

from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24          # f32 unit roundoff
ULP_BF16 = 2.0 ** -7      # one bf16 ulp, relative
TANH_ATOL = 2.0 ** -22    # 2 ulp(f32) at |tanh| <= 1
HEADROOM = 2.0            # the single headroom factor (<= 2)
LN_F32_TOL = 1e-4         # project tolerance for f32 layer norm
SLOPE_01 = float(np.float32(0.1))  # the kernels' 0.1f constant, exactly

D = torch.float64


class Oracle(NamedTuple):
    ref: torch.Tensor                 # fp64, rounded to the output dtype
    bound: torch.Tensor               # fp64 allowed |got - ref| per element
    masked: Optional[torch.Tensor]    # bool [B, T] rows that must be zero


# --------------------------------------------------------------------------- #
# building blocks
# --------------------------------------------------------------------------- #
def out_unit(dtype: torch.dtype) -> float:
    if dtype == torch.bfloat16:
        return 2.0 ** -8
    if dtype == torch.float32:
        return 2.0 ** -23
    raise ValueError(dtype)


def round_to(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp64 -> `dtype` -> fp64."""
    return t.to(torch.float32).to(dtype).to(D)


def lrelu64(t: torch.Tensor, slope: float) -> torch.Tensor:
    """LeakyReLU in fp64 with the slope the kernel holds as an f32."""
    s = float(np.float32(slope))
    return torch.where(t > 0, t, t * s)


def pre_act(x: torch.Tensor, slope: float) -> torch.Tensor:
    """The staging loop: lrelu in f32, round to bf16.  slope <= 0: none
    (the wrappers pass -1 then).  Returns fp64 [B, T, C]."""
    v = x.detach().cpu().to(torch.float32)
    if slope > 0.0:
        v = torch.where(v > 0, v, v * slope)  # f32 arithmetic
    return v.to(torch.bfloat16).to(D)


def w_bf16(w: torch.Tensor) -> torch.Tensor:
    return w.detach().cpu().to(torch.bfloat16).to(D)


def _cl(t: torch.Tensor) -> torch.Tensor:  # [B,T,C] <-> [B,C,T]
    return t.transpose(1, 2)


def conv64(xa: torch.Tensor, w: torch.Tensor, padding: int, dilation: int,
           dtype=D, stride: int = 1, groups: int = 1) -> torch.Tensor:
    """Channel-last conv, xa [B,T,Cin], w [Cout,Cin/groups,k]."""
    return _cl(F.conv1d(_cl(xa).to(dtype), w.to(dtype), None, stride=stride,
                        padding=padding, dilation=dilation,
                        groups=groups)).to(D)


def abs_conv(xa, w, padding, dilation, stride=1, groups=1):
    """A = sum |x'||w| — same routine on absolute values (f32, see
    module docstring)."""
    return conv64(xa.abs(), w.abs(), padding, dilation, torch.float32,
                  stride, groups)


def row_mask(lens: Optional[torch.Tensor], B: int, T: int):
    """bool [B, T]: True where t >= lens[b] (the kernel clamps lens to T,
    which the comparison does implicitly)."""
    if lens is None:
        return None
    lens = lens.detach().cpu().to(torch.int64)
    return torch.arange(T).unsqueeze(0) >= lens.unsqueeze(1)


def _f64(t: Optional[torch.Tensor]):
    return None if t is None else t.detach().cpu().to(D)


def elementwise_bound(ref: torch.Tensor, A: torch.Tensor, n_terms: int,
                      out_dtype: torch.dtype, *, tanh: bool = False,
                      carried: Optional[torch.Tensor] = None,
                      scale: float = 1.0,
                      masked: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Allowed |got - ref| per element (formula in the module docstring).

    ref      fp64 reference (already rounded to out_dtype or not: the
             difference is second order)
    A        sum of absolute values of every term of the f32 accumulation
    n_terms  number of f32 operations feeding one element
    carried  error bound carried in from an earlier stage, already pushed
             through this stage's |weights|
    scale    epilogue multiplier applied after the accumulation
    masked   bool [B, T] rows whose bound is 0 (exact zero required)
    """
    err = n_terms * U32 * A
    if carried is not None:
        err = err + carried
    err = err * abs(scale)
    if tanh:
        err = err + TANH_ATOL
    err = err + out_unit(out_dtype) * ref.abs()
    bound = HEADROOM * err  # the one place headroom is applied
    if masked is not None:
        bound = bound.masked_fill(masked.unsqueeze(-1), 0.0)
    return bound


# --------------------------------------------------------------------------- #
# channel-last conv
# --------------------------------------------------------------------------- #
def conv_cl_oracle(x, w, bias, padding=0, dilation=1, pre_slope=0.0,
                   act="none", post_slope=0.0, residual=None, out_lens=None,
                   out_dtype=torch.bfloat16) -> Oracle:
    """leaky_conv1d_cl.  act in {"none", "lrelu", "relu", "tanh"}."""
    Cout, Cin, k = w.shape
    xa, wq = pre_act(x, pre_slope), w_bf16(w)
    y = conv64(xa, wq, padding, dilation)
    A = abs_conv(xa, wq, padding, dilation)
    if bias is not None:
        b = bias.detach().cpu().to(torch.float32).to(D)
        y, A = y + b, A + b.abs()
    if act == "lrelu":
        y = lrelu64(y, post_slope)
    elif act == "relu":
        y = torch.relu(y)
    elif act == "tanh":
        y = torch.tanh(y)
    elif act != "none":
        raise ValueError(act)
    if residual is not None:
        r = _f64(residual)
        y, A = y + r, A + r.abs()
    B, T = y.shape[:2]
    masked = row_mask(out_lens, B, T)
    if masked is not None:
        y = y.masked_fill(masked.unsqueeze(-1), 0.0)
    ref = round_to(y, out_dtype)
    bound = elementwise_bound(ref, A, Cin * k + 3, out_dtype,
                              tanh=(act == "tanh"), masked=masked)
    return Oracle(ref, bound, masked)


# --------------------------------------------------------------------------- #
# channel-last transposed conv
# --------------------------------------------------------------------------- #
def convt_cl_oracle(x, w, bias, stride, padding, pre_slope=0.0,
                    out_lens=None, out_dtype=torch.bfloat16) -> Oracle:
    """leaky_convtranspose1d_cl; w is [Cin, Cout, k]."""
    Cin, Cout, k = w.shape
    xa, wq = pre_act(x, pre_slope), w_bf16(w)
    y = _cl(F.conv_transpose1d(_cl(xa), wq, None, stride=stride,
                               padding=padding))
    A = _cl(F.conv_transpose1d(_cl(xa).abs().float(), wq.abs().float(), None,
                               stride=stride, padding=padding)).to(D)
    if bias is not None:
        b = bias.detach().cpu().to(torch.float32).to(D)
        y, A = y + b, A + b.abs()
    B, T = y.shape[:2]
    masked = row_mask(out_lens, B, T)
    if masked is not None:
        y = y.masked_fill(masked.unsqueeze(-1), 0.0)
    ref = round_to(y, out_dtype)
    taps = -(-k // stride)  # taps that reach one output row
    bound = elementwise_bound(ref, A, Cin * taps + 3, out_dtype,
                              masked=masked)
    return Oracle(ref, bound, masked)


# --------------------------------------------------------------------------- #
# channel-first conv family (csrc/conv1d.hip)
# --------------------------------------------------------------------------- #
def _pow2(v: float) -> bool:
    m, _ = np.frexp(np.float32(v))
    return float(m) == 0.5


def _naive_operands(x, w, pre_slope):
    """What the naive kernels multiply: x and w in x's dtype, the
    pre-activation LeakyReLU in f32 WITHOUT the bf16 re-rounding of the MFMA
    staging loop.  Returns (x', w', products_exact).  For bf16 and a
    power-of-two slope (or none) x' is still bf16, hence ``pre_act`` and
    exact products; otherwise every product rounds once in f32."""
    if x.dtype == torch.bfloat16 and (pre_slope <= 0.0 or _pow2(pre_slope)):
        return pre_act(x, pre_slope), w_bf16(w), True
    v = x.detach().cpu().to(torch.float32)
    if pre_slope > 0.0:
        v = torch.where(v > 0, v, v * pre_slope)  # f32 arithmetic
    return v.to(D), w.detach().cpu().to(x.dtype).to(D), False


def conv_ct_oracle(x, w, bias, stride=1, padding=0, dilation=1, groups=1,
                   pre_slope=0.0, act="none", post_slope=0.0, residual=None,
                   path="mfma") -> Oracle:
    """conv1d_fused on x [B,Cin,T], w [Cout,Cin/groups,k]; the output has
    x's dtype.  act in {"none", "lrelu", "tanh"}.

    path="mfma"   conv1d_mfma_kernel: bf16 operands, exact products,
                  n = Cin·k + 3; the residual joins the f32 value before
                  the single output rounding.
    path="naive"  conv1d_naive_kernel: n = (Cin/groups)·k + 3 when the
                  products are exact (see ``_naive_operands``), else
                  2·(Cin/groups)·k + 3 as in ``depthwise_cl_oracle``.  The
                  binding adds the residual with ``out.add_`` AFTER the
                  kernel has stored: round to the output dtype, add, round
                  again; the bound carries the first rounding, u_out·|y1|,
                  next to the second.
    """
    Cout, cpg, k = w.shape
    if path == "mfma":
        assert x.dtype == torch.bfloat16 and stride == 1 and groups == 1
        xa, wq, exact = pre_act(x, pre_slope), w_bf16(w), True
    elif path == "naive":
        xa, wq, exact = _naive_operands(x, w, pre_slope)
    else:
        raise ValueError(path)
    n_terms = (1 if exact else 2) * cpg * k + 3
    y = _cl(conv64(_cl(xa), wq, padding, dilation, D, stride, groups))
    A = _cl(abs_conv(_cl(xa), wq, padding, dilation, stride, groups))
    if bias is not None:
        b = bias.detach().cpu().to(torch.float32).to(D).view(1, -1, 1)
        y, A = y + b, A + b.abs()
    if act == "lrelu":
        y = lrelu64(y, post_slope)
    elif act == "tanh":
        y = torch.tanh(y)
    elif act != "none":
        raise ValueError(act)
    carried = None
    if residual is not None:
        r = _f64(residual)
        if path == "mfma":
            y, A = y + r, A + r.abs()
        else:
            y1 = round_to(y, x.dtype)
            carried = out_unit(x.dtype) * y1.abs()
            y = y1 + r
    ref = round_to(y, x.dtype)
    bound = elementwise_bound(ref, A, n_terms, x.dtype, tanh=(act == "tanh"),
                              carried=carried)
    return Oracle(ref, bound, None)


def convt_ct_oracle(x, w, bias, stride, padding, pre_slope=0.0,
                    path="mfma") -> Oracle:
    """convtranspose1d_fused on x [B,Cin,T], w [Cin,Cout,k];
    n = Cin·ceil(k/stride) + 3 (doubled product count on the naive path when
    the products round, as in ``conv_ct_oracle``)."""
    Cin, Cout, k = w.shape
    if path == "mfma":
        assert x.dtype == torch.bfloat16
        xa, wq, exact = pre_act(x, pre_slope), w_bf16(w), True
    elif path == "naive":
        xa, wq, exact = _naive_operands(x, w, pre_slope)
    else:
        raise ValueError(path)
    y = F.conv_transpose1d(xa, wq, None, stride=stride, padding=padding)
    A = F.conv_transpose1d(xa.abs().float(), wq.abs().float(), None,
                           stride=stride, padding=padding).to(D)
    if bias is not None:
        b = bias.detach().cpu().to(torch.float32).to(D).view(1, -1, 1)
        y, A = y + b, A + b.abs()
    ref = round_to(y, x.dtype)
    taps = -(-k // stride)  # taps that reach one output column
    n_terms = (1 if exact else 2) * Cin * taps + 3
    return Oracle(ref, elementwise_bound(ref, A, n_terms, x.dtype), None)


# --------------------------------------------------------------------------- #
# resblock pair
# --------------------------------------------------------------------------- #
def resblock_pair_oracle(x, w1, b1, w2, b2, dilation, out_lens=None,
                         accum=None, out_scale=1.0,
                         out_dtype=torch.bfloat16) -> Oracle:
    """(conv2_{k,1}(lrelu(conv1_{k,d}(lrelu(x)))) + x [+ accum]) * scale.
    Both LeakyReLU slopes are the kernel's hard-coded 0.1f."""
    C, _, k = w1.shape
    B, T = x.shape[:2]
    masked = row_mask(out_lens, B, T)
    xa, w1q, w2q = pre_act(x, 0.1), w_bf16(w1), w_bf16(w2)
    pad1, pad2 = (k - 1) * dilation // 2, (k - 1) // 2
    b1d = b1.detach().cpu().to(torch.float32).to(D)
    b2d = b2.detach().cpu().to(torch.float32).to(D)
    # stage 1: xt lives in LDS as bf16; rows outside [0, lim) are zero
    y1 = conv64(xa, w1q, pad1, dilation) + b1d
    A1 = abs_conv(xa, w1q, pad1, dilation) + b1d.abs()
    xt = lrelu64(y1, 0.1)
    if masked is not None:
        xt = xt.masked_fill(masked.unsqueeze(-1), 0.0)
    xt = round_to(xt, torch.bfloat16)
    E1 = (C * k + 2) * U32 * A1 + ULP_BF16 * xt.abs()
    if masked is not None:
        E1 = E1.masked_fill(masked.unsqueeze(-1), 0.0)
    # stage 2
    xd = _f64(x)
    y2 = conv64(xt, w2q, pad2, 1) + b2d + xd
    A2 = abs_conv(xt, w2q, pad2, 1) + b2d.abs() + xd.abs()
    if accum is not None:
        a = _f64(accum)
        y2, A2 = y2 + a, A2 + a.abs()
    scale = float(np.float32(out_scale))
    y2 = y2 * scale
    if masked is not None:
        y2 = y2.masked_fill(masked.unsqueeze(-1), 0.0)
    ref = round_to(y2, out_dtype)
    carried = abs_conv(E1, w2q, pad2, 1)
    bound = elementwise_bound(ref, A2, C * k + 4, out_dtype,
                              carried=carried, scale=scale, masked=masked)
    return Oracle(ref, bound, masked)


# --------------------------------------------------------------------------- #
# gates
# --------------------------------------------------------------------------- #
def _gate(va: torch.Tensor, vb: torch.Tensor, out_dtype) -> Oracle:
    """tanh(va)·sigmoid(vb), the kernel computing in f32 with
    sigmoid = 1/(1 + __expf(-vb)).

      va, vb    one f32 add each (x + g): |d| <= u32·|v|
      tanh      1-Lipschitz -> u32·|va|, + TANH_ATOL (2 ulp)
      __expf    documented max error 2 + floor(1.16·|x|) ulp, i.e.
                relative eps_e <= (2 + 1.16·|vb|)·2^-23
      sigmoid   d(sig)/sig = (1 - sig)·eps_e, + 3·2^-23 for the add and
                the division (<= 2.5 ulp); input add through
                sig' <= 1/4
      product   one more f32 rounding
    """
    t, s = torch.tanh(va), torch.sigmoid(vb)
    ref = t * s
    eps_e = (2.0 + 1.16 * vb.abs()) * 2.0 ** -23
    e_s = s * ((1 - s) * eps_e + 3 * 2.0 ** -23) + U32 * vb.abs() / 4
    e_t = U32 * va.abs() + TANH_ATOL
    err = s * e_t + t.abs() * e_s + U32 * ref.abs()
    err = err + out_unit(out_dtype) * ref.abs()
    return Oracle(round_to(ref, out_dtype), HEADROOM * err, None)


def gate_cl_oracle(x, g, n_channels) -> Oracle:
    """fused_gate_cl: x [B,F,2C]; g None, [B,2C], [B,1,2C] or [B,F,2C]."""
    v = _f64(x)
    if g is not None:
        gd = _f64(g)
        v = v + (gd.unsqueeze(1) if gd.dim() == 2 else gd)
    return _gate(v[..., :n_channels], v[..., n_channels:], x.dtype)


def gate_ct_oracle(x, g, n_channels) -> Oracle:
    """fused_gate: x [B,2C,T]; g None, [B,2C,T] or [B,2C,1]."""
    v = _f64(x)
    if g is not None:
        v = v + _f64(g)
    return _gate(v[:, :n_channels], v[:, n_channels:], x.dtype)


# --------------------------------------------------------------------------- #
# depthwise conv
# --------------------------------------------------------------------------- #
def depthwise_cl_oracle(x, w, bias, dilation, padding) -> Oracle:
    """depthwise_conv1d_cl: x [B,T,C], w [C,1,k] in x's dtype, f32
    accumulation seeded with the bias.  For f32 inputs the products round
    too: k products + k adds + bias -> n = 2k + 1 terms."""
    C, _, k = w.shape
    xd, wd = _f64(x), _f64(w)
    y = _cl(F.conv1d(_cl(xd), wd, None, padding=padding, dilation=dilation,
                     groups=C))
    A = _cl(F.conv1d(_cl(xd).abs(), wd.abs(), None, padding=padding,
                     dilation=dilation, groups=C))
    if bias is not None:
        b = bias.detach().cpu().to(torch.float32).to(D)
        y, A = y + b, A + b.abs()
    ref = round_to(y, x.dtype)
    return Oracle(ref, elementwise_bound(ref, A, 2 * k + 1, x.dtype), None)


# --------------------------------------------------------------------------- #
# layer norms
# --------------------------------------------------------------------------- #
def _ln_bound(ref, out_dtype):
    bound = torch.full_like(ref, LN_F32_TOL * float(ref.abs().max()))
    if out_dtype != torch.float32:
        bound = bound + HEADROOM * out_unit(out_dtype) * ref.abs()
    return bound


def layer_norm_ct_oracle(x, gamma, beta, eps=1e-5, residual=None) -> Oracle:
    """LayerNorm over C of [B,C,T] (of x + residual)."""
    v = _f64(x)
    if residual is not None:
        v = v + _f64(residual)
    mean = v.mean(1, keepdim=True)
    var = ((v - mean) ** 2).mean(1, keepdim=True)
    g = gamma.detach().cpu().float().to(D).view(1, -1, 1)
    b = beta.detach().cpu().float().to(D).view(1, -1, 1)
    y = (v - mean) / torch.sqrt(var + eps) * g + b
    ref = round_to(y, x.dtype)
    return Oracle(ref, _ln_bound(ref, x.dtype), None)


def row_ln_cl_oracle(x, gamma, beta, eps=1e-5, residual=None) -> Oracle:
    """LayerNorm over the last dim of [B,T,C] (of x + residual)."""
    v = _f64(x)
    if residual is not None:
        v = v + _f64(residual)
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    g = gamma.detach().cpu().float().to(D)
    b = beta.detach().cpu().float().to(D)
    y = (v - mean) / torch.sqrt(var + eps) * g + b
    ref = round_to(y, x.dtype)
    return Oracle(ref, _ln_bound(ref, x.dtype), None)


# --------------------------------------------------------------------------- #
# prior sample
# --------------------------------------------------------------------------- #
def prior_sample_oracle(m, logs, mask, noise, noise_scale) -> Oracle:
    """(m + noise·__expf(logs)·ns)·mask in f32: the exp carries the
    relative error eps_e of ``_gate``; three multiplies and one add
    follow."""
    md, ld, nd, kd = _f64(m), _f64(logs), _f64(noise), _f64(mask)
    ns = float(np.float32(noise_scale))
    term = nd * torch.exp(ld) * ns
    y = (md + term) * kd
    eps_e = (2.0 + 1.16 * ld.abs()) * 2.0 ** -23
    err = (term.abs() * (eps_e + 3 * U32)
           + 2 * U32 * (md.abs() + term.abs())) * kd.abs()
    ref = round_to(y, m.dtype)
    err = err + out_unit(m.dtype) * ref.abs()
    return Oracle(ref, HEADROOM * err, None)


# --------------------------------------------------------------------------- #
# comparison
# --------------------------------------------------------------------------- #
def assert_within(got: torch.Tensor, oracle: Oracle, *, tile: int = 0,
                  time_dim: int = 1, chan_dim: int = 2, what: str = "") -> None:
    """Every element of `got` must lie within oracle.bound of oracle.ref;
    rows in oracle.masked must be exactly zero.  Nothing is sampled or
    skipped.  On failure, names the worst element (largest excess over its
    bound): index, values, bound, and the time tile (t // tile) and channel
    it falls in."""
    ref, bound, masked = oracle
    g = got.detach().cpu().to(D)
    assert g.shape == ref.shape, f"{what}: shape {tuple(g.shape)} != " \
                                 f"{tuple(ref.shape)}"
    diff = (g - ref).abs()
    bad = ~(diff <= bound)  # NaN/inf in got count as failures

    def where(idx):
        t, c = idx[time_dim], idx[chan_dim]
        tl = f"time tile {t // tile} (row {t % tile} of {tile})" if tile \
            else f"time row {t}"
        return f"index {idx}, {tl}, channel {c}"

    if masked is not None:
        m = masked
        while m.dim() < g.dim():
            m = m.unsqueeze(-1)
        leak = (g != 0) & m
        if leak.any():
            idx = tuple(int(i) for i in leak.nonzero()[0])
            raise AssertionError(
                f"{what}: masked row not exactly zero: got {float(g[idx])!r}"
                f" at {where(idx)} ({int(leak.sum())} such elements)")
    if bad.any():
        excess = torch.where(bad, diff - bound, torch.zeros_like(diff))
        excess = torch.nan_to_num(excess, nan=float("inf"))
        idx = tuple(int(i) for i in np.unravel_index(
            int(excess.argmax()), tuple(excess.shape)))
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements out of "
            f"bound; worst at {where(idx)}: got {float(g[idx])!r}, ref "
            f"{float(ref[idx])!r}, |diff| {float(diff[idx]):.3e} > bound "
            f"{float(bound[idx]):.3e}")


def assert_plus_zero(got: torch.Tensor, lens: torch.Tensor, what: str = "",
                     time_dim: int = 1) -> None:
    """Rows t >= lens[b] of a bf16 tensor hold the bit pattern of +0
    (0x0000), not -0: the kernels store zeros there, they do not multiply
    by a mask."""
    assert got.dtype == torch.bfloat16, f"{what}: {got.dtype}"
    g = got.detach().cpu().movedim(time_dim, 1).contiguous()
    bits = g.view(torch.int16).reshape(g.shape[0], g.shape[1], -1)
    masked = row_mask(lens, g.shape[0], g.shape[1])
    leak = (bits != 0) & masked.unsqueeze(-1)
    assert not leak.any(), (
        f"{what}: {int(leak.sum())} masked elements are not +0; first at "
        f"(b, t, c) = {tuple(int(i) for i in leak.nonzero()[0])}")


def rounding_free(shape, gen, scale=1.0, dtype=torch.bfloat16):
    """Random bf16-representable tensor (so the reference input is
    unambiguous)."""
    return (torch.randn(shape, generator=gen) * scale).to(torch.bfloat16) \
        .to(dtype)
