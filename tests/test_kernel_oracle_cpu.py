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


# --------------------------------------------------------------------------- #
# channel-first conv family (csrc/conv1d.hip)
# --------------------------------------------------------------------------- #
CT = dict(time_dim=2, chan_dim=1)


def _emu_conv_ct(x, w, bias, pad, dil, pre, resid, post=0.0, mut=None):
    """f32 stand-in for conv1d_mfma_kernel on [B,Cin,T], with mutations."""
    wq = w.to(BF).float()
    if mut == "tap":      # last tap of the chunk remainder never staged
        wq = wq.clone()
        wq[:, :, -1] = 0
    xa = _lrelu32(x.float(), pre).to(BF).float()
    b = None if (bias is None or mut == "bias") else bias.float()
    if mut == "late_pre":
        # LeakyReLU on each bf16-rounded product instead of on the staged x
        B, Cin, T = x.shape
        k = w.shape[2]
        xp = F.pad(x.float(), (pad, pad))
        Tout = T + 2 * pad - (k - 1) * dil
        win = torch.stack([xp[:, :, j * dil:j * dil + Tout]
                           for j in range(k)], 2)          # [B,Cin,k,Tout]
        prod = (wq[None, :, :, :, None] * win[:, None]).to(BF).float()
        y = _lrelu32(prod, pre).sum((2, 3)) + b.view(1, -1, 1)
    else:
        y = F.conv1d(xa, wq, b, padding=pad, dilation=dil)
    if post > 0:
        y = _lrelu32(y, post)
    if resid is not None and mut != "resid":
        y = y + resid.float()
    y = y.to(BF)
    if mut == "col128":   # column 128 takes its neighbour's value
        y[:, :, 128] = y[:, :, 129]
    if mut == "row":      # last live row of the partial Cout tile
        y[:, -1] = 0
    return y


# k = 5 leaves a one-tap remainder at TC = 4 (the <64,128,2,4,4> class,
# Cout 80); k = 3 at TC = 2 (<128,128,4,2,2>, Cout 130)
@pytest.fixture(scope="module", params=[(80, 5), (130, 3)])
def conv_ct_case(request):
    Cout, k = request.param
    g = _gen(10 + k)
    B, T, Cin = 2, 300, 24
    x = ko.rounding_free((B, Cin, T), g)
    w = ko.rounding_free((Cout, Cin, k), g, (Cin * k) ** -0.5)
    bias = torch.randn(Cout, generator=g)
    resid = ko.rounding_free((B, Cout, T), g)
    args = dict(x=x, w=w, bias=bias, pad=(k - 1) // 2, dil=1, pre=0.125,
                resid=resid, post=0.25)
    oracle = ko.conv_ct_oracle(x, w, bias, 1, args["pad"], 1, 1, 0.125,
                               "lrelu", 0.25, resid, "mfma")
    return args, oracle


def test_conv_ct_honest_f32_accepted(conv_ct_case):
    args, oracle = conv_ct_case
    ko.assert_within(_emu_conv_ct(**args), oracle, tile=128, what="conv_ct",
                     **CT)


@pytest.mark.parametrize("mut", ["tap", "col128", "row", "bias", "resid",
                                 "late_pre"])
def test_conv_ct_mutant_rejected(conv_ct_case, mut):
    args, oracle = conv_ct_case
    _rejects(_emu_conv_ct(**args, mut=mut), oracle, tile=128, **CT)


def _emu_conv_naive(x, w, bias, stride, pad, dil, groups, pre, resid):
    """f32 stand-in for conv1d_naive_kernel + the binding's out.add_."""
    xa = _lrelu32(x.float(), pre) if pre > 0 else x.float()
    y = F.conv1d(xa, w.to(x.dtype).float(),
                 None if bias is None else bias.float(), stride=stride,
                 padding=pad, dilation=dil, groups=groups).to(x.dtype)
    if resid is not None:
        y = (y.float() + resid.float()).to(x.dtype)
    return y


@pytest.fixture(scope="module")
def naive_case():
    """The halo-70 shape: bf16, k 11, dilation 7, with a residual."""
    g = _gen(20)
    B, T, Cin, Cout, k, dil = 2, 150, 24, 40, 11, 7
    x = ko.rounding_free((B, Cin, T), g)
    w = ko.rounding_free((Cout, Cin, k), g, (Cin * k) ** -0.5)
    bias = torch.randn(Cout, generator=g)
    resid = ko.rounding_free((B, Cout, T), g)
    args = dict(x=x, w=w, bias=bias, stride=1, pad=35, dil=dil, groups=1,
                pre=0.125, resid=resid)
    oracle = ko.conv_ct_oracle(x, w, bias, 1, 35, dil, 1, 0.125,
                               residual=resid, path="naive")
    return args, oracle


def test_conv_naive_honest_accepted(naive_case):
    args, oracle = naive_case
    ko.assert_within(_emu_conv_naive(**args), oracle, what="naive", **CT)


def test_conv_naive_mutants_rejected(naive_case):
    args, oracle = naive_case
    _rejects(_emu_conv_naive(**{**args, "bias": None}), oracle, **CT)
    _rejects(_emu_conv_naive(**{**args, "resid": None}), oracle, **CT)


def test_conv_naive_permuted_weight_read_as_raw_rejected(naive_case):
    """What leaky_conv1d used to hand the naive kernel past the halo limit:
    the padded [k,CoutP,CinP] tensor, indexed as [Cout][Cin][k]."""
    from sonata_amd.ops.functional import _conv_weight_mfma

    args, oracle = naive_case
    w = args["w"]
    perm = _conv_weight_mfma(w.clone())
    assert perm.numel() >= w.numel()
    misread = perm.reshape(-1)[:w.numel()].view(w.shape)
    _rejects(_emu_conv_naive(**{**args, "w": misread}), oracle, **CT)


@pytest.mark.parametrize("dtype,groups,stride", [
    (torch.float32, 1, 1), (torch.float32, 4, 1), (BF, 4, 2), (BF, 24, 1)])
def test_conv_naive_variants_honest_accepted(dtype, groups, stride):
    g = _gen(21 + groups + stride)
    B, T, Cin, k, dil = 2, 70, 24, 3, 9
    Cout = 24 if groups == 24 else 40
    x = ko.rounding_free((B, Cin, T), g, 1.0, dtype)
    w = ko.rounding_free((Cout, Cin // groups, k), g, 0.3, dtype)
    if dtype == torch.float32:  # full f32 operands: the products round
        x = x + torch.randn(x.shape, generator=g) * 1e-3
        w = w + torch.randn(w.shape, generator=g) * 1e-3
    bias = torch.randn(Cout, generator=g)
    pre = 0.1 if dtype == torch.float32 else 0.125
    oracle = ko.conv_ct_oracle(x, w, bias, stride, dil, dil, groups, pre,
                               path="naive")
    got = _emu_conv_naive(x, w, bias, stride, dil, dil, groups, pre, None)
    ko.assert_within(got, oracle, what="naive variant", **CT)
    w_tap = w.clone()
    w_tap[:, :, -1] = 0
    _rejects(_emu_conv_naive(x, w_tap, bias, stride, dil, dil, groups, pre,
                             None), oracle, **CT)


def _emu_convt_ct(x, w, bias, s, pad, pre, mut=None):
    xa = _lrelu32(x.float(), pre).to(BF).float()
    y = F.conv_transpose1d(xa, w.to(BF).float(),
                           None if mut == "bias" else bias.float(),
                           stride=s, padding=pad).to(BF)
    if mut == "phase":
        # output t = s*v + r - pad: phases r = 0 and 1 of the first and of
        # the last complete run exchange places
        Tout = y.shape[2]
        v_first = -(-pad // s)
        v_last = (Tout - s + pad) // s
        for v in (v_first, v_last):
            t0 = s * v - pad
            assert 0 <= t0 and t0 + s <= Tout
            y[:, :, [t0, t0 + 1]] = y[:, :, [t0 + 1, t0]]
    return y


@pytest.mark.parametrize("k,s,pad", [(16, 8, 4), (4, 2, 1), (16, 8, 0),
                                     (7, 3, 2)])
def test_convt_ct_honest_and_mutants(k, s, pad):
    g = _gen(30 + k + pad)
    B, Tin, Cin, Cout = 2, 33, 40, 96
    x = ko.rounding_free((B, Cin, Tin), g)
    w = ko.rounding_free((Cin, Cout, k), g, (Cin * 2) ** -0.5)
    bias = torch.randn(Cout, generator=g)
    oracle = ko.convt_ct_oracle(x, w, bias, s, pad, 0.125, "mfma")
    ko.assert_within(_emu_convt_ct(x, w, bias, s, pad, 0.125), oracle,
                     tile=32 * s, what="convt_ct", **CT)
    _rejects(_emu_convt_ct(x, w, bias, s, pad, 0.125, "phase"), oracle, **CT)
    _rejects(_emu_convt_ct(x, w, bias, s, pad, 0.125, "bias"), oracle, **CT)
    w_tap = w.clone()
    w_tap[:, :, -1] = 0
    _rejects(_emu_convt_ct(x, w_tap, bias, s, pad, 0.125), oracle, **CT)


def test_convt_naive_f32_honest_accepted():
    g = _gen(40)
    x = torch.randn((2, 24, 17), generator=g)
    w = torch.randn((24, 40, 7), generator=g) * 0.2
    bias = torch.randn(40, generator=g)
    oracle = ko.convt_ct_oracle(x, w, bias, 3, 2, 0.1, "naive")
    got = F.conv_transpose1d(_lrelu32(x, 0.1), w, bias, stride=3, padding=2)
    ko.assert_within(got, oracle, what="convt naive f32", **CT)
    _rejects(F.conv_transpose1d(x, w, bias, stride=3, padding=2), oracle,
             **CT)


# --------------------------------------------------------------------------- #
# leaky_conv1d: which weight layout reaches the binding
# --------------------------------------------------------------------------- #
class _RecordingExt:
    def __init__(self):
        self.calls = []

    def conv1d_fused(self, x, w, *rest):
        self.calls.append((w,) + rest)
        return "out"


@pytest.mark.parametrize("dtype,k,dil,stride,groups,permuted", [
    (BF, 3, 1, 1, 1, True),
    (BF, 11, 5, 1, 1, True),
    (BF, 5, 16, 1, 1, True),      # halo == 64: still the MFMA kernel
    (BF, 11, 7, 1, 1, False),     # halo 70 -> naive kernel
    (BF, 66, 1, 1, 1, False),     # halo 65
    (BF, 3, 1, 1, 4, False),
    (BF, 3, 1, 2, 1, False),
    (torch.float32, 3, 1, 1, 1, False),
])
def test_leaky_conv1d_weight_layout_follows_the_binding(
        monkeypatch, dtype, k, dil, stride, groups, permuted):
    from sonata_amd.ops import functional as fn

    ext = _RecordingExt()
    monkeypatch.setattr(fn, "use_hip", lambda t: True)
    monkeypatch.setattr(fn, "hip_ext", lambda required=False: ext)
    Cin, Cout = 24, 40
    x = torch.zeros((2, Cin, 80), dtype=dtype)
    w = torch.randn((Cout, Cin // groups, k)).to(dtype)
    assert fn.leaky_conv1d(x, w, None, stride=stride,
                           padding=(k - 1) * dil // 2, dilation=dil,
                           groups=groups) == "out"
    (passed, _bias, cout, kk, st, _pad, dd, gg, *_), = ext.calls
    assert (cout, kk, st, dd, gg) == (Cout, k, stride, dil, groups)
    if permuted:
        assert passed is fn._conv_weight_mfma(w)      # the cached copy
        assert passed.shape == (k, 64, 32) and passed.dtype == BF
    else:
        assert passed is w                            # raw [Cout,Cin/g,k]


def test_halo_limit_matches_the_kernel_source():
    import os
    import re

    from sonata_amd.ops.functional import CONV_MFMA_HALO_MAX

    src = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "csrc", "conv1d.hip")
    with open(src) as f:
        m = re.search(r"^#define HALO_MAX (\d+)$", f.read(), re.M)
    assert m and int(m.group(1)) == CONV_MFMA_HALO_MAX
