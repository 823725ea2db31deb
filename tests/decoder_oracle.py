"""An independent walk of the HiFi-GAN generator for the bf16 channel-last
decoder (``Generator._forward_cl`` and the C++ engine's ``generator``), one
entry per kernel launch, each entry an unchanged ``kernel_oracle`` oracle.

The plan comes from a ``VitsArchitecture``, an fp32 CPU state dict of
``dec``, the frame lengths and optionally ``g``; nothing is taken from the
code under test.  Parameters enter as the bf16 path holds them: weights
rounded to bf16, biases rounded to bf16 and widened to f32.

Stage names, in launch order:

    conv_pre                      leaky_conv1d_cl, k=7, no activation
    cond.proj                     (only with g) the 1x1 speaker projection,
                                  channel-first conv1d_fused, [B, C0, 1]
    cond                          (only with g) eager bf16 add of conv_pre
                                  and cond.proj, then the re-mask
    ups.{i}                       leaky_convtranspose1d_cl, lrelu(0.1) in
    resblocks.{3i+j}.pair{d}      resblock_pair_cl with dilation d; the last
                                  pair of resblock j > 0 adds the running MRF
                                  sum (accum), the last pair of the last
                                  resblock also scales by 1/num_kernels
    conv_post                     leaky_conv1d_cl, lrelu(0.1) in, tanh out

A pair the fused kernel does not take (rule of ``resblock_pair_cl``'s
docstring, restated in ``pair_is_fused``) runs as two leaky_conv1d_cl
launches and eager bf16 arithmetic, so it is

    resblocks.{n}.pair{d}.conv1   lrelu in, dilated conv
    resblocks.{n}.pair{d}.conv2   lrelu in, plain conv, + residual
    resblocks.{n}.pair{d}.mrf     (only with accum or a scale) eager
                                  (y + accum) * scale, re-masked

Teacher forcing: ``check`` feeds every stage's oracle the tensors a trace
recorded for the stages before it, so the single-kernel bound applies to
each stage exactly and a failure names its stage.  ``chain`` runs the walk
on its own references (the rounded chain); ``exact`` is the same graph in
fp64 with the bf16 parameters and no intermediate rounding.

Activations are channel-last bf16 [B, T, C] everywhere except
``cond.proj`` ([B, C0, 1], as the kernel writes it).
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

import kernel_oracle as ko
from sonata_amd.models.config import VitsArchitecture

BF = torch.bfloat16
D = torch.float64
SLOPE = 0.1          # LRELU_SLOPE of the generator
CONV_TILE = 256      # output rows per block of leaky_conv1d_cl
CONVT_ROWS = 128     # input rows per block of leaky_convtranspose1d_cl
PAIR_HALO_MAX = 52   # widest (k-1)*dilation the fused pair kernel takes


# --------------------------------------------------------------------------- #
# shape rules, restated from the wrappers' documentation
# --------------------------------------------------------------------------- #
def _round_up(v: int, m: int) -> int:
    return -(-v // m) * m


def padded_weight(cout: int, cin: int) -> Tuple[int, int]:
    """Rows and columns of the MFMA weight layout: Cout padded to the tile
    height (128, 64 or 32), Cin to 32."""
    bm = 128 if cout >= 128 else (64 if cout >= 64 else 32)
    return _round_up(cout, bm), _round_up(cin, 32)


def pair_is_fused(C: int, k: int, dilation: int) -> bool:
    """resblock_pair_cl: one fused launch unless the halo (k-1)*dilation
    exceeds 52 or the channel count does not pad to a square 32/64/128/256
    weight (C=96 pads to 128x96: two convs)."""
    cp_out, cp_in = padded_weight(C, C)
    return ((k - 1) * dilation <= PAIR_HALO_MAX and cp_out == cp_in
            and cp_out in (32, 64, 128, 256))


def pair_tile(C: int, k: int) -> int:
    """Output tile of the fused pair kernel's default geometry: the xt tile
    (256 rows up to 32 channels, 64 from 256 channels on, else 128) less the
    second conv's halo."""
    xtr = 256 if C <= 32 else (64 if C >= 256 else 128)
    return xtr - (k - 1)


# --------------------------------------------------------------------------- #
# stages
# --------------------------------------------------------------------------- #
@dataclass(eq=False)
class Stage:
    """One launch.  ``srcs`` name the stages whose outputs are its
    activation inputs ("z" is the decoder input); ``p`` holds everything
    else its oracle needs.  ``dataclasses.replace`` makes a mutant."""
    name: str
    kind: str                      # conv | convt | pair | proj | cond | mrf
    srcs: Tuple[str, ...]
    tile: int
    lens: Optional[torch.Tensor]   # out_lens of this launch (int64) or None
    p: dict = field(default_factory=dict)

    def oracle(self, *acts: torch.Tensor) -> ko.Oracle:
        assert len(acts) == len(self.srcs), (self.name, len(acts))
        p, lens = self.p, self.lens
        if self.kind == "conv":
            res = acts[1] if len(acts) > 1 else None
            return ko.conv_cl_oracle(
                acts[0], p["w"], p["b"], p["padding"], p["dilation"],
                p["pre_slope"], p["act"], 0.0, res, lens)
        if self.kind == "convt":
            return ko.convt_cl_oracle(acts[0], p["w"], p["b"], p["stride"],
                                      p["padding"], p["pre_slope"], lens)
        if self.kind == "pair":
            acc = acts[1] if len(acts) > 1 else None
            return ko.resblock_pair_oracle(
                acts[0], p["w1"], p["b1"], p["w2"], p["b2"], p["dilation"],
                lens, acc, p["scale"])
        if self.kind == "proj":
            return ko.conv_ct_oracle(p["g"], p["w"], p["b"], path="mfma")
        if self.kind == "cond":
            # one bf16 rounding of an exact sum of two bf16 values (the
            # f32 sum ATen forms first is what round_to passes through),
            # then exact zeros: compared bitwise, bound 0
            y = ko._f64(acts[0]) + ko._f64(acts[1]).transpose(1, 2)
            return _exact_stage(ko.round_to(y, BF), lens)
        if self.kind == "mrf":
            # eager bf16 ATen: each op computes in f32 and rounds to bf16
            y = ko._f64(acts[0])
            if len(acts) > 1:
                y = ko.round_to(y + ko._f64(acts[1]), BF)
            if p["scale"] != 1.0:
                s = float(torch.tensor(p["scale"], dtype=torch.float32))
                y = ko.round_to(y * s, BF)
            return _exact_stage(y, lens)
        raise ValueError(self.kind)

    @property
    def dims(self) -> Tuple[int, int]:
        """(time_dim, chan_dim) of this stage's output."""
        return (2, 1) if self.kind == "proj" else (1, 2)


def _exact_stage(y: torch.Tensor, lens) -> ko.Oracle:
    masked = ko.row_mask(lens, y.shape[0], y.shape[1])
    if masked is not None:
        y = y.masked_fill(masked.unsqueeze(-1), 0.0)
    return ko.Oracle(y, torch.zeros_like(y), masked)


def _params(state: Dict[str, torch.Tensor], mod: str, bias: bool = True):
    """Weight rounded to bf16; bias rounded to bf16, widened to f32."""
    w = state[mod + ".weight"].detach().cpu().float().to(BF)
    b = None
    if bias:
        b = state[mod + ".bias"].detach().cpu().float().to(BF).float()
    return w, b


def _lens(lengths, batch: int) -> Optional[torch.Tensor]:
    """Both paths drop the lengths of a batch of one."""
    if lengths is None or batch == 1:
        return None
    lens = torch.as_tensor(lengths).detach().cpu().to(torch.int64)
    assert lens.numel() == batch
    return lens


def walk(arch: VitsArchitecture, state: Dict[str, torch.Tensor],
         batch: int, lengths=None,
         g: Optional[torch.Tensor] = None) -> List[Stage]:
    """The launch plan.  ``state`` is ``dec``'s state dict (fp32, CPU),
    ``lengths`` the valid frames per row, ``g`` [B, gin, 1] or None."""
    lens = _lens(lengths, batch)
    ch = arch.upsample_initial_channel
    nk = len(arch.resblock_kernel_sizes)
    stages: List[Stage] = []

    w, b = _params(state, "conv_pre")
    assert w.shape == (ch, arch.inter_channels, 7)
    stages.append(Stage("conv_pre", "conv", ("z",), CONV_TILE, lens, dict(
        w=w, b=b, padding=3, dilation=1, pre_slope=0.0, act="none")))
    prev = "conv_pre"
    if g is not None and "cond.weight" in state:
        w, b = _params(state, "cond")
        assert w.shape == (ch, arch.gin_channels, 1)
        gq = g.detach().cpu().float().to(BF)
        assert gq.shape == (batch, arch.gin_channels, 1)
        stages.append(Stage("cond.proj", "proj", (), 0, None,
                            dict(g=gq, w=w, b=b)))
        stages.append(Stage("cond", "cond", (prev, "cond.proj"), CONV_TILE,
                            lens))
        prev = "cond"

    for i, (r, ku) in enumerate(zip(arch.upsample_rates,
                                    arch.upsample_kernel_sizes)):
        cin, ch = ch, ch // 2
        if lens is not None:
            lens = lens * r
        w, b = _params(state, f"ups.{i}")
        assert w.shape == (cin, ch, ku)
        up = f"ups.{i}"
        stages.append(Stage(up, "convt", (prev,), CONVT_ROWS * r, lens, dict(
            w=w, b=b, stride=r, padding=(ku - r) // 2, pre_slope=SLOPE)))
        xs = None  # running MRF sum
        for j, (k, dils) in enumerate(zip(arch.resblock_kernel_sizes,
                                          arch.resblock_dilation_sizes)):
            rb = f"resblocks.{i * nk + j}"
            assert len(set(dils)) == len(dils), "pair names need distinct d"
            x = up
            for di, d in enumerate(dils):
                last = di == len(dils) - 1
                acc = xs if last else None
                scale = 1.0 / nk if (last and j == nk - 1) else 1.0
                w1, b1 = _params(state, f"{rb}.convs1.{di}")
                w2, b2 = _params(state, f"{rb}.convs2.{di}")
                assert w1.shape == w2.shape == (ch, ch, k)
                name = f"{rb}.pair{d}"
                if pair_is_fused(ch, k, d):
                    srcs = (x,) if acc is None else (x, acc)
                    stages.append(Stage(
                        name, "pair", srcs, pair_tile(ch, k), lens, dict(
                            w1=w1, b1=b1, w2=w2, b2=b2, dilation=d,
                            scale=scale)))
                    x = name
                    continue
                stages.append(Stage(
                    name + ".conv1", "conv", (x,), CONV_TILE, lens, dict(
                        w=w1, b=b1, padding=(k - 1) * d // 2, dilation=d,
                        pre_slope=SLOPE, act="none")))
                stages.append(Stage(
                    name + ".conv2", "conv", (name + ".conv1", x), CONV_TILE,
                    lens, dict(w=w2, b=b2, padding=(k - 1) // 2, dilation=1,
                               pre_slope=SLOPE, act="none")))
                x = name + ".conv2"
                if acc is not None or scale != 1.0:
                    srcs = (x,) if acc is None else (x, acc)
                    stages.append(Stage(name + ".mrf", "mrf", srcs,
                                        CONV_TILE, lens, dict(scale=scale)))
                    x = name + ".mrf"
            xs = x
        prev = xs

    w, _ = _params(state, "conv_post", bias=False)
    assert w.shape == (1, ch, 7) and "conv_post.bias" not in state
    stages.append(Stage("conv_post", "conv", (prev,), CONV_TILE, lens, dict(
        w=w, b=None, padding=3, dilation=1, pre_slope=SLOPE, act="tanh")))
    names = [s.name for s in stages]
    assert len(set(names)) == len(names), names
    return stages


# --------------------------------------------------------------------------- #
# running and checking a trace
# --------------------------------------------------------------------------- #
class Memo:
    """Oracles already computed for (stage, input tensors), by identity; a
    child looks its parent up first.  Lets a trace that shares tensors with
    an earlier one be checked without redoing the fp64 work."""

    def __init__(self, parent: Optional["Memo"] = None):
        self.parent, self.d = parent, {}

    def get(self, stage: Stage, acts) -> ko.Oracle:
        key = (id(stage),) + tuple(id(a) for a in acts)
        m = self
        while m is not None:
            if key in m.d:
                return m.d[key][1]
            m = m.parent
        o = stage.oracle(*acts)
        self.d[key] = ((stage, acts), o)  # keeps the ids alive
        return o


def input_cl(z: torch.Tensor) -> torch.Tensor:
    """Decoder input [B, C, F] (already z*y_mask) -> the bf16 channel-last
    tensor conv_pre reads."""
    return z.detach().cpu().to(BF).transpose(1, 2).contiguous()


def chain(stages: List[Stage], z: torch.Tensor,
          replace: Optional[Dict[str, Stage]] = None,
          memo: Optional[Memo] = None) -> Dict[str, torch.Tensor]:
    """The rounded chain: stage s takes the bf16-rounded reference of the
    stages before it.  ``replace`` computes the named stages with another
    Stage (a mutant); everything after is teacher-forced from its output.
    Returns name -> bf16 tensor, "z" included."""
    memo = memo if memo is not None else Memo()
    trace = {"z": input_cl(z)}
    for st in stages:
        run = (replace or {}).get(st.name, st)
        acts = tuple(trace[s] for s in run.srcs)
        trace[st.name] = memo.get(run, acts).ref.to(BF)
    return trace


def check(stages: List[Stage], trace: Dict[str, torch.Tensor],
          memo: Optional[Memo] = None,
          only: Optional[List[str]] = None,
          ratios: Optional[Dict[str, float]] = None) -> Dict[str, str]:
    """Hold every stage of a recorded trace to its teacher-forced oracle:
    ``assert_within`` (masked rows exactly zero) and +0 bits on masked
    rows.  Returns {stage name: failure message}; empty when all pass.
    ``ratios``, when given, receives each stage's largest |got - ref| /
    bound over the elements with a non-zero bound (for reports only)."""
    memo = memo if memo is not None else Memo()
    failures: Dict[str, str] = {}
    for st in stages:
        if only is not None and st.name not in only:
            continue
        got = trace[st.name]
        tdim, cdim = st.dims
        try:
            assert got.dtype == BF, f"{st.name}: dtype {got.dtype}"
            acts = tuple(trace[s] for s in st.srcs)
            oracle = memo.get(st, acts)
            if ratios is not None and got.shape == oracle.ref.shape:
                live = oracle.bound > 0
                diff = (got.detach().cpu().to(D) - oracle.ref).abs()
                ratios[st.name] = float(
                    (diff[live] / oracle.bound[live]).max()) \
                    if live.any() else 0.0
            ko.assert_within(got, oracle, tile=st.tile,
                             time_dim=tdim, chan_dim=cdim, what=st.name)
            if st.lens is not None:
                ko.assert_plus_zero(got, st.lens, st.name, time_dim=tdim)
        except AssertionError as e:
            failures[st.name] = str(e)
    return failures


def assert_trace(stages, trace, memo=None, only=None, ratios=None) -> None:
    failures = check(stages, trace, memo, only, ratios)
    assert not failures, (
        f"{len(failures)} stage(s) out of bound, first: "
        + next(iter(failures.values())))


# --------------------------------------------------------------------------- #
# the unrounded graph
# --------------------------------------------------------------------------- #
def exact(arch: VitsArchitecture, state: Dict[str, torch.Tensor],
          z: torch.Tensor, lengths=None,
          g: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The generator in fp64 on the bf16-rounded parameters and the bf16
    input, no intermediate rounding, masked after every conv as the
    channel-first model masks: every stage but conv_post, so only samples
    below a row's length compare with the channel-last path, which zeroes
    the rest.  z [B, C, F] -> [B, 1, F*hop].  The LeakyReLU
    slope is the model's 0.1 as a double; the kernels' f32 constant differs
    from it by 1.5e-8 relative, far below any bf16 effect this is used to
    measure."""
    B = z.shape[0]
    lens = _lens(lengths, B)

    def par(mod, bias=True):
        w, b = _params(state, mod, bias)
        return w.to(D), (None if b is None else b.to(D))

    def mask(t, ln):
        if ln is None:
            return t
        dead = torch.arange(t.shape[2]).unsqueeze(0) >= ln.unsqueeze(1)
        return t.masked_fill(dead.unsqueeze(1), 0.0)

    def lrelu(t):
        return torch.where(t > 0, t, t * SLOPE)

    nk = len(arch.resblock_kernel_sizes)
    x = F.conv1d(z.detach().cpu().to(BF).to(D), *par("conv_pre"), padding=3)
    if g is not None and "cond.weight" in state:
        x = x + F.conv1d(g.detach().cpu().float().to(BF).to(D), *par("cond"))
    x = mask(x, lens)
    for i, (r, ku) in enumerate(zip(arch.upsample_rates,
                                    arch.upsample_kernel_sizes)):
        if lens is not None:
            lens = lens * r
        x = mask(F.conv_transpose1d(lrelu(x), *par(f"ups.{i}"), stride=r,
                                    padding=(ku - r) // 2), lens)
        xs = None
        for j, (k, dils) in enumerate(zip(arch.resblock_kernel_sizes,
                                          arch.resblock_dilation_sizes)):
            y = x
            for di, d in enumerate(dils):
                rb = f"resblocks.{i * nk + j}"
                xt = mask(F.conv1d(lrelu(y), *par(f"{rb}.convs1.{di}"),
                                   padding=(k - 1) * d // 2, dilation=d),
                          lens)
                y = mask(F.conv1d(lrelu(xt), *par(f"{rb}.convs2.{di}"),
                                  padding=(k - 1) // 2) + y, lens)
            xs = y if xs is None else xs + y
        x = xs / nk
    w, _ = par("conv_post", bias=False)
    return torch.tanh(F.conv1d(lrelu(x), w, None, padding=3))


def make_input(arch: VitsArchitecture, frames: int, lengths, seed: int):
    """The decoder inputs of one test case: z [B, C, F] f32 holding bf16
    values (a rounding_free normal, scale 0.5) and y_mask [B, 1, F].
    ``decode`` multiplies the two; the walk takes z * y_mask."""
    lens = torch.as_tensor(lengths)
    gen = torch.Generator()
    gen.manual_seed(seed)
    z = ko.rounding_free((lens.numel(), arch.inter_channels, frames), gen,
                         0.5, torch.float32)
    y_mask = (torch.arange(frames).unsqueeze(0)
              < lens.unsqueeze(1)).to(torch.float32).unsqueeze(1)
    return z, y_mask


def valid_rms(a: torch.Tensor, b: torch.Tensor, valid) -> List[float]:
    """Per row, the RMS of a - b over [0, valid[row]); a, b [B, 1, T]."""
    out = []
    for row, n in enumerate(valid):
        d = (a[row, 0, :n].detach().cpu().to(D)
             - b[row, 0, :n].detach().cpu().to(D))
        out.append(float(d.pow(2).mean().sqrt()))
    return out
