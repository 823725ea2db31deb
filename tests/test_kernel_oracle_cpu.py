"""CPU proof of the oracle's power (tests/kernel_oracle.py).

For one small shape per kernel family, a plain-torch f32 emulation of a
CORRECT kernel (bf16 inputs, f32 accumulation, output rounded to bf16) must
be accepted by ``assert_within``, and every deliberately wrong variant of it
must be rejected.  Together: the derived bound is reachable by an honest f32
kernel and tight enough to see a single wrong tap, row, channel or slope.
"""

import pytest
import torch
import torch.nn.functional as F

import kernel_oracle as ko

BF = torch.bfloat16


def _gen(seed=0):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _lrelu32(v, slope):
    return torch.where(v > 0, v, v * slope)


def _shift_from(x, row=256):
    """Input shifted by one row from `row` on (a tile-seam off-by-one)."""
    x = x.clone()
    x[:, row:-1] = x[:, row + 1:].clone()
    return x


def _mask(y, lens):
    idx = torch.arange(y.shape[1])
    return y.masked_fill((idx.unsqueeze(0) >= lens.unsqueeze(1))
                         .unsqueeze(-1), 0)


def _rejects(got, oracle, **kw):
    with pytest.raises(AssertionError):
        ko.assert_within(got, oracle, **kw)


# --------------------------------------------------------------------------- #
# conv
# --------------------------------------------------------------------------- #
def _emu_conv(x, w, bias, pad, dil, slope, resid, lens, mut=None,
              act_slope=0.0):
    """f32 stand-in for conv1d_cl_kernel, with mutation knobs."""
    w = w.to(BF).float()
    if mut == "tap":
        w = w.clone()
        w[:, :, w.shape[2] // 2 + 1] = 0
    if mut == "chan":
        w = w.clone()
        w[:, -1, :] = 0
    if mut == "shift":
        x = _shift_from(x)
    if mut == "slope":
        slope = 0.1
    xa = x.float()
    if slope > 0:
        xa = _lrelu32(xa, slope)
    xa = xa.to(BF).float()
    y = F.conv1d(xa.transpose(1, 2), w,
                 None if (bias is None or mut == "bias") else bias.float(),
                 padding=pad, dilation=dil).transpose(1, 2)
    if act_slope > 0:
        y = _lrelu32(y, act_slope)
    if resid is not None and mut != "resid":
        y = y + resid.float()
    if lens is not None:
        y = _mask(y, lens + (1 if mut == "mask" else 0))
    return y.to(BF)


CONV_MUTANTS = ["tap", "shift", "bias", "resid", "mask", "slope", "chan"]


@pytest.fixture(scope="module")
def conv_case():
    g = _gen(1)
    B, T, Cin, Cout, k, dil = 2, 300, 24, 33, 7, 3
    x = ko.rounding_free((B, T, Cin), g)
    w = ko.rounding_free((Cout, Cin, k), g, (Cin * k) ** -0.5)
    bias = torch.randn(Cout, generator=g)
    resid = ko.rounding_free((B, T, Cout), g)
    lens = torch.tensor([T, 259])
    args = dict(x=x, w=w, bias=bias, pad=(k - 1) * dil // 2, dil=dil,
                slope=0.125, resid=resid, lens=lens)
    oracle = ko.conv_cl_oracle(x, w, bias, args["pad"], dil, 0.125,
                               residual=resid, out_lens=lens)
    return args, oracle


def test_conv_honest_f32_accepted(conv_case):
    args, oracle = conv_case
    ko.assert_within(_emu_conv(**args), oracle, tile=256, what="conv")


@pytest.mark.parametrize("mut", CONV_MUTANTS)
def test_conv_mutant_rejected(conv_case, mut):
    args, oracle = conv_case
    _rejects(_emu_conv(**args, mut=mut), oracle, tile=256)


def test_conv_model_slope_mirrored_rounding():
    """Slope 0.1 is not exact in bf16: the oracle mirrors the staging
    loop's f32 multiply + bf16 rounding, so the honest kernel still passes
    at the model's slope, and the 0.125 slope is told apart from it."""
    g = _gen(2)
    x = ko.rounding_free((1, 64, 16), g)
    w = ko.rounding_free((8, 16, 3), g, 0.15)
    oracle = ko.conv_cl_oracle(x, w, None, 1, 1, 0.1, act="lrelu",
                               post_slope=0.1)
    got = _emu_conv(x, w, None, 1, 1, 0.1, None, None, act_slope=0.1)
    ko.assert_within(got, oracle, tile=256)
    _rejects(_emu_conv(x, w, None, 1, 1, 0.125, None, None, act_slope=0.1),
             oracle)


def test_masked_rows_must_be_exactly_zero(conv_case):
    args, oracle = conv_case
    got = _emu_conv(**args).clone()
    got[1, 299, 5] = 1e-30  # far below any bound, but not zero
    with pytest.raises(AssertionError, match="masked row"):
        ko.assert_within(got, oracle, tile=256)


def test_failure_report_names_tile_and_channel(conv_case):
    args, oracle = conv_case
    got = _emu_conv(**args).clone()
    got[0, 258, 7] += 1.0
    with pytest.raises(AssertionError) as ei:
        ko.assert_within(got, oracle, tile=256)
    msg = str(ei.value)
    assert "(0, 258, 7)" in msg and "time tile 1" in msg
    assert "channel 7" in msg and "bound" in msg


def test_nan_is_a_failure(conv_case):
    args, oracle = conv_case
    got = _emu_conv(**args).clone()
    got[0, 0, 0] = float("nan")
    _rejects(got, oracle)


# --------------------------------------------------------------------------- #
# transposed conv
# --------------------------------------------------------------------------- #
def _emu_convt(x, w, bias, s, pad, slope, lens, mut=None):
    w = w.to(BF).float()
    if mut == "tap":
        w = w.clone()
        w[:, :, 1] = 0
    if mut == "chan":
        w = w.clone()
        w[-1] = 0
    if mut == "shift":
        x = _shift_from(x, 128)
    if mut == "slope":
        slope = 0.1
    xa = _lrelu32(x.float(), slope).to(BF).float()
    y = F.conv_transpose1d(xa.transpose(1, 2), w,
                           None if mut == "bias" else bias.float(),
                           stride=s, padding=pad).transpose(1, 2)
    return _mask(y, lens + (1 if mut == "mask" else 0)).to(BF)


@pytest.fixture(scope="module")
def convt_case():
    g = _gen(3)
    B, T, Cin, Cout, k, s = 2, 150, 40, 16, 4, 2
    x = ko.rounding_free((B, T, Cin), g)
    w = ko.rounding_free((Cin, Cout, k), g, (Cin * 2) ** -0.5)
    bias = torch.randn(Cout, generator=g)
    lens = torch.tensor([2 * T, 2 * 128 + 3])
    args = dict(x=x, w=w, bias=bias, s=s, pad=(k - s) // 2, slope=0.125,
                lens=lens)
    return args, ko.convt_cl_oracle(x, w, bias, s, (k - s) // 2, 0.125, lens)


def test_convt_honest_f32_accepted(convt_case):
    args, oracle = convt_case
    ko.assert_within(_emu_convt(**args), oracle, tile=256, what="convt")


@pytest.mark.parametrize("mut", ["tap", "shift", "bias", "mask", "slope",
                                 "chan"])
def test_convt_mutant_rejected(convt_case, mut):
    args, oracle = convt_case
    _rejects(_emu_convt(**args, mut=mut), oracle)


# --------------------------------------------------------------------------- #
# resblock pair
# --------------------------------------------------------------------------- #
def _emu_pair(x, w1, b1, w2, b2, dil, lens, accum, scale, mut=None):
    k = w1.shape[2]
    w1, w2 = w1.to(BF).float(), w2.to(BF).float()
    if mut == "tap":
        w2 = w2.clone()
        w2[:, :, 0] = 0
    if mut == "chan":
        w1 = w1.clone()
        w1[:, -1, :] = 0
    xs = _shift_from(x) if mut == "shift" else x
    xa = _lrelu32(xs.float(), 0.125 if mut == "slope" else 0.1).to(BF).float()
    y1 = F.conv1d(xa.transpose(1, 2), w1,
                  None if mut == "bias" else b1.float(),
                  padding=(k - 1) * dil // 2, dilation=dil).transpose(1, 2)
    xt = y1 if mut == "noreact" else _lrelu32(y1, 0.1)
    xt = _mask(xt, lens + (1 if mut == "mask" else 0)).to(BF).float()
    y = F.conv1d(xt.transpose(1, 2), w2, b2.float(),
                 padding=(k - 1) // 2).transpose(1, 2)
    if mut != "resid":
        y = y + x.float()
    y = (y + accum.float()) * scale
    return _mask(y, lens + (1 if mut == "mask" else 0)).to(BF)


@pytest.fixture(scope="module")
def pair_case():
    g = _gen(4)
    B, T, C, k, dil = 2, 300, 16, 7, 3
    x = ko.rounding_free((B, T, C), g)
    w1 = ko.rounding_free((C, C, k), g, (C * k) ** -0.5)
    w2 = ko.rounding_free((C, C, k), g, (C * k) ** -0.5)
    b1 = torch.randn(C, generator=g) * 0.5
    b2 = torch.randn(C, generator=g) * 0.5
    accum = ko.rounding_free((B, T, C), g)
    lens = torch.tensor([T, 259])
    args = dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, dil=dil, lens=lens,
                accum=accum, scale=1.0 / 3)
    oracle = ko.resblock_pair_oracle(x, w1, b1, w2, b2, dil, lens, accum,
                                     1.0 / 3)
    return args, oracle


def test_pair_honest_f32_accepted(pair_case):
    args, oracle = pair_case
    ko.assert_within(_emu_pair(**args), oracle, tile=122, what="pair")


@pytest.mark.parametrize("mut", ["tap", "shift", "bias", "resid", "mask",
                                 "slope", "chan", "noreact"])
def test_pair_mutant_rejected(pair_case, mut):
    args, oracle = pair_case
    _rejects(_emu_pair(**args, mut=mut), oracle)


# --------------------------------------------------------------------------- #
# gate, depthwise
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_gate_honest_and_mutants(dtype):
    g = _gen(5)
    B, Fr, C = 3, 37, 24
    x = ko.rounding_free((B, Fr, 2 * C), g, 1.5, dtype)
    gg = ko.rounding_free((B, 2 * C), g, 1.0, dtype)
    oracle = ko.gate_cl_oracle(x, gg, C)
    v = x.float() + gg.float().unsqueeze(1)
    a, b = v[..., :C], v[..., C:]
    ko.assert_within((torch.tanh(a) * torch.sigmoid(b)).to(dtype), oracle)
    # conditioning omitted / halves swapped / wrong batch row of g
    _rejects((torch.tanh(x.float()[..., :C])
              * torch.sigmoid(x.float()[..., C:])).to(dtype), oracle)
    _rejects((torch.tanh(b) * torch.sigmoid(a)).to(dtype), oracle)
    v2 = x.float() + gg.float().roll(1, 0).unsqueeze(1)
    _rejects((torch.tanh(v2[..., :C]) * torch.sigmoid(v2[..., C:]))
             .to(dtype), oracle)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_depthwise_honest_and_mutants(dtype):
    g = _gen(6)
    B, T, C, k, dil = 2, 300, 8, 3, 9
    x = ko.rounding_free((B, T, C), g, 1.0, dtype)
    w = ko.rounding_free((C, 1, k), g, 0.5, dtype)
    bias = torch.randn(C, generator=g)
    oracle = ko.depthwise_cl_oracle(x, w, bias, dil, dil)

    def emu(x, w, bias):
        y = F.conv1d(x.float().transpose(1, 2), w.float(), bias, padding=dil,
                     dilation=dil, groups=C)
        return y.transpose(1, 2).to(dtype)

    ko.assert_within(emu(x, w, bias), oracle)
    w_tap = w.clone()
    w_tap[:, :, 2] = 0
    _rejects(emu(x, w_tap, bias), oracle)          # tap dropped
    _rejects(emu(x, w, None), oracle)              # bias omitted
    _rejects(emu(_shift_from(x), w, bias), oracle)  # seam off by one
    w_ch = w.clone()
    w_ch[-1] = 0
    _rejects(emu(x, w_ch, bias), oracle)           # last channel zeroed


# --------------------------------------------------------------------------- #
# layer norm: the one-pass variance is a mutant at an offset
# --------------------------------------------------------------------------- #
def _ln_f32_sequential(x, gamma, beta, eps, two_pass):
    """f32 emulation accumulating channel by channel like the kernels."""
    C = x.shape[1]
    s = torch.zeros_like(x[:, 0])
    ss = torch.zeros_like(s)
    for c in range(C):
        s = s + x[:, c]
        ss = ss + x[:, c] * x[:, c]
    mean = s / C
    if two_pass:
        ss = torch.zeros_like(s)
        for c in range(C):
            d = x[:, c] - mean
            ss = ss + d * d
        var = ss / C
    else:
        var = (ss / C - mean * mean).clamp_min(0)
    rstd = torch.rsqrt(var + eps)
    return ((x - mean.unsqueeze(1)) * rstd.unsqueeze(1)
            * gamma.view(1, -1, 1) + beta.view(1, -1, 1))


def test_layer_norm_offset_one_pass_rejected_two_pass_accepted():
    g = _gen(7)
    x = torch.randn(2, 192, 64, generator=g) + 32.0
    gamma = torch.randn(192, generator=g)
    beta = torch.randn(192, generator=g)
    oracle = ko.layer_norm_ct_oracle(x, gamma, beta, 1e-5)
    ko.assert_within(_ln_f32_sequential(x, gamma, beta, 1e-5, True), oracle,
                     time_dim=2, chan_dim=1)
    _rejects(_ln_f32_sequential(x, gamma, beta, 1e-5, False), oracle,
             time_dim=2, chan_dim=1)
    # zero-mean input: both formulations are fine
    x0 = x - 32.0
    oracle0 = ko.layer_norm_ct_oracle(x0, gamma, beta, 1e-5)
    ko.assert_within(_ln_f32_sequential(x0, gamma, beta, 1e-5, False),
                     oracle0, time_dim=2, chan_dim=1)
