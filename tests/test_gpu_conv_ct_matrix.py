"""The channel-first conv family of csrc/conv1d.hip against the fp64 oracle
of tests/kernel_oracle.py, element by element: conv1d_mfma_kernel in its
three tile classes, convt1d_merged_kernel, the generic transposed mode of
conv1d_mfma_kernel and the two naive kernels; then every host-side refusal
of the two bindings.

The shapes are the smallest that reach each branch of the launchers (tile
classes by Cout, partial M tiles, partial / single-row K slices, the
interior and the guarded staging path, tap-chunk remainders at every TC, a
halo of exactly HALO_MAX, odd T so rows start off 16-byte boundaries).
Calls go through sonata_amd.ops.functional so the weight-layout caches are
exercised; act_mode 2 (tanh) and a slope-0 LeakyReLU exist only at the
extension and are called there.  Every tolerance is the oracle's derived
bound; nothing is sampled.
"""

import pytest
import torch

import kernel_oracle as ko

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32
CT = dict(time_dim=2, chan_dim=1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gen(*key):
    """CPU generator seeded by the case's parameters."""
    seed = 23
    for k in key:
        seed = (seed * 1000003 + int(k * 1000)) % (2 ** 31 - 1)
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _to(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def _ext():
    from sonata_amd.ops import hip_ext

    return hip_ext(required=True)


# --------------------------------------------------------------------------- #
# conv1d_mfma_kernel: <32,256,1,8,8> (Cout < 64), <64,128,2,4,4> (< 128),
# <128,128,4,2,2>
# --------------------------------------------------------------------------- #
SAME, BIG = "same", "big"          # (k-1)*dil//2 and that + 2
T1, TM, TB, TP, T3 = "1", "BN-1", "BN", "BN+1", "3BN+7"
NONE, LR, LR0, TANH = "none", "lrelu", "lrelu0", "tanh"
# (Cout, Cin, T, k, dil, pad, pre_slope, act, bias, resid)
CONV_CASES = [
    # <32,256,1,8,8>: BN 256, TC 8 (k 11 leaves a 3-tap remainder)
    (1, 24, T3, 11, 5, SAME, 0.125, NONE, True, True),
    (33, 33, T3, 5, 16, SAME, 0.0, LR, True, False),
    (33, 192, TP, 3, 1, SAME, 0.125, TANH, True, False),
    (1, 50, TB, 7, 3, BIG, 0.0, NONE, False, True),
    (33, 24, TM, 4, 1, 0, 0.125, LR0, True, False),
    (1, 33, T1, 1, 1, 0, 0.0, NONE, True, False),
    (33, 50, T1, 5, 1, SAME, 0.125, NONE, True, True),
    (33, 192, T3, 1, 1, 0, 0.0, TANH, False, False),
    (1, 192, TM, 3, 1, BIG, 0.125, LR, True, True),
    (33, 24, TB, 7, 3, 0, 0.0, NONE, True, False),
    (1, 50, TP, 4, 1, SAME, 0.125, NONE, False, False),
    # <64,128,2,4,4>: Cout 80 = one full + one partial M tile; TC 4 (k 5
    # leaves one tap, k 11 three)
    (80, 24, T3, 5, 1, SAME, 0.125, NONE, True, True),
    (80, 33, T3, 11, 5, SAME, 0.0, LR, True, False),
    (80, 192, TP, 5, 16, SAME, 0.125, NONE, True, False),
    (80, 50, TB, 3, 1, BIG, 0.0, TANH, True, False),
    (80, 24, TM, 7, 3, 0, 0.125, NONE, False, True),
    (80, 33, T1, 3, 1, SAME, 0.0, LR0, True, False),
    (80, 50, T3, 4, 1, 0, 0.125, NONE, True, True),
    (80, 192, TM, 1, 1, 0, 0.0, NONE, True, True),
    (80, 24, TP, 11, 5, BIG, 0.125, TANH, False, False),
    (80, 192, TB, 7, 3, SAME, 0.0, NONE, True, False),
    # <128,128,4,2,2>: Cout 130 = full + partial, 256 = two full; TC 2
    # (k 3, 5, 7, 11 all leave one tap)
    (130, 24, T3, 3, 1, SAME, 0.125, NONE, True, True),
    (256, 192, T3, 11, 5, SAME, 0.0, NONE, True, False),
    (130, 33, TP, 5, 16, 0, 0.125, LR, True, False),
    (256, 50, TB, 7, 3, SAME, 0.0, TANH, False, True),
    (130, 192, TM, 4, 1, BIG, 0.125, NONE, True, False),
    (256, 33, T1, 11, 5, SAME, 0.0, NONE, True, True),
    (130, 50, T3, 1, 1, 0, 0.125, LR0, True, False),
    (256, 24, TP, 5, 1, BIG, 0.0, NONE, True, False),
    (130, 192, TB, 5, 16, SAME, 0.125, NONE, False, False),
    (256, 24, TM, 3, 1, 0, 0.0, LR, True, True),
    # cond_layer-like: one column, twelve M tiles
    (1536, 64, T1, 1, 1, 0, 0.0, NONE, True, False),
]
# row 0 alone == row 0 of the batch, bitwise: one case per tile class
ROW0_CASES = {CONV_CASES[0], CONV_CASES[11], CONV_CASES[21]}


def _conv_bn(Cout):
    return 256 if Cout < 64 else 128


def _conv_call(x, w, bias, pad, dil, pre, act, res):
    """Through leaky_conv1d where it can express the activation, else
    straight at the binding with the same cached operands."""
    from sonata_amd.ops.functional import (_bias_f32, _conv_weight_mfma,
                                           leaky_conv1d)

    if act in (NONE, LR):
        return leaky_conv1d(x, w, bias, padding=pad, dilation=dil,
                            pre_lrelu=pre, post_lrelu=0.25 if act == LR
                            else 0.0, residual=res)
    Cout, _, k = w.shape
    return _ext().conv1d_fused(
        x, _conv_weight_mfma(w), _bias_f32(bias), Cout, k, 1, pad, dil, 1,
        pre if pre > 0 else -1.0, 2 if act == TANH else 1, 0.0, res)


@pytest.mark.parametrize("Cout,Cin,Tsel,k,dil,pad,pre,act,has_bias,has_res",
                         CONV_CASES)
def test_conv1d_mfma_matrix(dev, Cout, Cin, Tsel, k, dil, pad, pre, act,
                            has_bias, has_res):
    BN = _conv_bn(Cout)
    T = {T1: 1, TM: BN - 1, TB: BN, TP: BN + 1, T3: 3 * BN + 7}[Tsel]
    halo = (k - 1) * dil
    padding = {SAME: halo // 2, BIG: halo // 2 + 2}.get(pad, pad)
    Tout = T + 2 * padding - halo
    assert Tout > 0 and halo <= 64
    g = _gen(Cout, Cin, T, k, dil)
    B = 2
    x = ko.rounding_free((B, Cin, T), g)
    w = ko.rounding_free((Cout, Cin, k), g, (Cin * k) ** -0.5)
    bias = torch.randn(Cout, generator=g) if has_bias else None
    res = ko.rounding_free((B, Cout, Tout), g) if has_res else None
    oracle = ko.conv_ct_oracle(
        x, w, bias, 1, padding, dil, 1, pre,
        {LR0: "lrelu"}.get(act, act), 0.25 if act == LR else 0.0, res, "mfma")
    xd, wd, bd, rd = _to(dev, x, w, bias, res)
    got = _conv_call(xd, wd, bd, padding, dil, pre, act, rd)
    ko.assert_within(got, oracle, tile=BN, what=f"conv1d_mfma BN{BN}", **CT)
    # second call reads the cached weight layout: bit-identical
    assert torch.equal(got, _conv_call(xd, wd, bd, padding, dil, pre, act,
                                       rd))
    if (Cout, Cin, Tsel, k, dil, pad, pre, act, has_bias, has_res) \
            in ROW0_CASES:
        alone = _conv_call(xd[:1].contiguous(), wd, bd, padding, dil, pre,
                           act, None if rd is None else rd[:1].contiguous())
        assert torch.equal(alone[0], got[0])


# --------------------------------------------------------------------------- #
# convt1d_merged_kernel<{64,128}, 4, 2, {8,2}, 2>: k == 2s, Cout >= 64,
# 32 v-columns per block
# --------------------------------------------------------------------------- #
# (k, s, Cout, Cin, Tin, same_pad, bias, pre)
CONVT_MERGED_CASES = [
    (16, 8, 64, 40, 97, True, True, 0.125),
    (16, 8, 96, 128, 33, False, False, 0.0),
    (16, 8, 128, 40, 32, True, True, 0.0),
    (16, 8, 160, 128, 31, False, True, 0.125),
    (16, 8, 96, 40, 1, True, True, 0.125),
    (16, 8, 160, 40, 97, False, False, 0.125),
    (16, 8, 64, 128, 1, False, True, 0.0),
    (16, 8, 128, 128, 33, True, False, 0.125),
    (4, 2, 64, 128, 33, False, True, 0.125),
    (4, 2, 96, 40, 97, True, False, 0.0),
    (4, 2, 128, 128, 31, True, True, 0.125),
    (4, 2, 160, 40, 32, False, True, 0.0),
    (4, 2, 160, 128, 1, True, False, 0.125),
    (4, 2, 64, 40, 31, False, True, 0.125),
    (4, 2, 128, 40, 97, False, True, 0.0),
    (4, 2, 96, 128, 32, True, True, 0.125),
]


def _convt_check(dev, k, s, Cout, Cin, Tin, pad, has_bias, pre, tile, what):
    from sonata_amd.ops.functional import leaky_convtranspose1d

    g = _gen(k, s, Cout, Cin, Tin, pad)
    x = ko.rounding_free((2, Cin, Tin), g)
    w = ko.rounding_free((Cin, Cout, k), g, (Cin * 2) ** -0.5)
    bias = torch.randn(Cout, generator=g) if has_bias else None
    oracle = ko.convt_ct_oracle(x, w, bias, s, pad, pre, "mfma")
    xd, wd, bd = _to(dev, x, w, bias)
    got = leaky_convtranspose1d(xd, wd, bd, s, pad, pre_lrelu=pre)
    ko.assert_within(got, oracle, tile=tile, what=what, **CT)
    assert torch.equal(got, leaky_convtranspose1d(xd, wd, bd, s, pad,
                                                  pre_lrelu=pre))


@pytest.mark.parametrize("k,s,Cout,Cin,Tin,same_pad,has_bias,pre",
                         CONVT_MERGED_CASES)
def test_convt1d_merged_matrix(dev, k, s, Cout, Cin, Tin, same_pad, has_bias,
                               pre):
    pad = (k - s) // 2 if same_pad else 0
    _convt_check(dev, k, s, Cout, Cin, Tin, pad, has_bias, pre, 32 * s,
                 f"convt1d_merged s{s}")


# --------------------------------------------------------------------------- #
# generic transposed mode of conv1d_mfma_kernel (Cout < 64, or k != 2s):
# every phase is one M-tile group of the same launch
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("Tin", [1, 97, 300])
@pytest.mark.parametrize("k,s,Cout,pad", [(16, 8, 32, 4), (4, 2, 32, 1),
                                          (7, 3, 80, 2)])
def test_convt1d_generic_matrix(dev, k, s, Cout, pad, Tin):
    # (7, 3): phase 0 has three taps, phases 1 and 2 two
    _convt_check(dev, k, s, Cout, 40, Tin, pad, Tin != 97, 0.125,
                 _conv_bn(Cout) * s, f"convt1d generic k{k} s{s}")


# --------------------------------------------------------------------------- #
# naive kernels
# --------------------------------------------------------------------------- #
# (dtype, Cin, Cout, groups, stride, k, dil, T, resid)
NAIVE_CASES = [
    (BF, 24, 24, 24, 1, 3, 9, 1, False),      # depthwise (DDS convs)
    (BF, 24, 24, 24, 1, 3, 9, 5, False),
    (BF, 24, 24, 24, 1, 3, 9, 70, False),
    (BF, 24, 40, 4, 1, 3, 1, 70, False),      # grouped
    (BF, 24, 40, 1, 2, 3, 1, 70, False),      # strided
    (F32, 24, 40, 1, 1, 3, 1, 70, True),      # f32 dense
    (BF, 24, 40, 1, 1, 11, 7, 70, True),      # halo 70 > HALO_MAX
]


@pytest.mark.parametrize("dtype,Cin,Cout,groups,stride,k,dil,T,has_res",
                         NAIVE_CASES)
def test_conv1d_naive_matrix(dev, dtype, Cin, Cout, groups, stride, k, dil, T,
                             has_res):
    from sonata_amd.ops.functional import leaky_conv1d

    g = _gen(Cin, Cout, groups, stride, k, dil, T)
    pad = (k - 1) * dil // 2
    Tout = (T + 2 * pad - (k - 1) * dil - 1) // stride + 1
    x = ko.rounding_free((2, Cin, T), g, 1.0, dtype)
    w = ko.rounding_free((Cout, Cin // groups, k), g,
                         (Cin // groups * k) ** -0.5, dtype)
    bias = torch.randn(Cout, generator=g)
    res = ko.rounding_free((2, Cout, Tout), g, 1.0, dtype) if has_res \
        else None
    oracle = ko.conv_ct_oracle(x, w, bias, stride, pad, dil, groups, 0.125,
                               "lrelu", 0.25, res, "naive")
    xd, wd, bd, rd = _to(dev, x, w, bias, res)
    got = leaky_conv1d(xd, wd, bd, stride=stride, padding=pad, dilation=dil,
                       groups=groups, pre_lrelu=0.125, post_lrelu=0.25,
                       residual=rd)
    ko.assert_within(got, oracle, what="conv1d_naive", **CT)


def test_convt1d_naive_f32(dev):
    from sonata_amd.ops.functional import leaky_convtranspose1d

    g = _gen(7, 3, 1)
    x = ko.rounding_free((2, 24, 33), g, 1.0, F32)
    w = ko.rounding_free((24, 40, 7), g, 0.15, F32)
    bias = torch.randn(40, generator=g)
    oracle = ko.convt_ct_oracle(x, w, bias, 3, 2, 0.125, "naive")
    xd, wd, bd = _to(dev, x, w, bias)
    got = leaky_convtranspose1d(xd, wd, bd, 3, 2, pre_lrelu=0.125)
    ko.assert_within(got, oracle, what="convt1d_naive f32", **CT)


def test_convt1d_naive_bf16_raw_weight(dev):
    """The binding takes a 3-D bf16 weight as the raw [Cin,Cout,k] tensor."""
    g = _gen(4, 2, 2)
    x = ko.rounding_free((2, 24, 33), g)
    w = ko.rounding_free((24, 40, 4), g, 0.15)
    bias = torch.randn(40, generator=g)
    oracle = ko.convt_ct_oracle(x, w, bias, 2, 1, 0.125, "naive")
    xd, wd, bd = _to(dev, x, w, bias)
    got = _ext().convtranspose1d_fused(xd, wd, bd, 40, 4, 2, 1, 0.125)
    ko.assert_within(got, oracle, what="convt1d_naive bf16", **CT)


# --------------------------------------------------------------------------- #
# refusals: every one a host-side check, raised before any launch
# --------------------------------------------------------------------------- #
def test_bindings_refuse_bad_arguments(dev):
    from sonata_amd.ops.functional import (_conv_weight_mfma,
                                           _convt_weight_mfma)

    ext = _ext()
    g = _gen(99)
    Cin, Cout, k, T = 24, 80, 3, 40
    x = ko.rounding_free((2, Cin, T), g).to(dev)
    w = ko.rounding_free((Cout, Cin, k), g, 0.1).to(dev)
    perm = _conv_weight_mfma(w)                       # [3, 128, 32]
    assert perm.shape == (k, 128, 32)
    bias = torch.randn(Cout, generator=g).to(dev)
    res = torch.zeros((2, Cout, T), dtype=BF, device=dev)

    def conv(xx=x, ww=perm, bb=bias, cout=Cout, kk=k, stride=1, pad=1, dil=1,
             groups=1, rr=None):
        return ext.conv1d_fused(xx, ww, bb, cout, kk, stride, pad, dil,
                                groups, -1.0, 0, 0.0, rr)

    assert conv().shape == (2, Cout, T)               # the accepted call
    assert conv(ww=w).shape == (2, Cout, T)           # raw -> naive kernel
    strided = torch.zeros((k, 128, 64), dtype=BF, device=dev)[:, :, ::2]
    w11 = ko.rounding_free((Cout, Cin, 11), g, 0.1).to(dev)
    w_g4 = ko.rounding_free((Cout, Cin // 4, k), g, 0.1).to(dev)
    bad_conv = {
        "neither shape": dict(ww=torch.zeros((Cout + 1, Cin, k), dtype=BF,
                                             device=dev)),
        "permuted, halo 70": dict(ww=_conv_weight_mfma(w11), kk=11, dil=7,
                                  pad=35),
        "permuted, stride 2": dict(stride=2),
        "permuted, f32 x": dict(xx=x.float(), bb=None),
        "permuted, groups 4": dict(groups=4),
        "not contiguous": dict(ww=strided),
        "weight on the host": dict(ww=perm.cpu()),
        "permuted in f32": dict(ww=perm.float()),
        "raw in f32": dict(ww=w_g4.float(), groups=4),
        "CoutP < Cout": dict(ww=perm[:, :64].contiguous()),
        "CoutP % BM": dict(ww=perm[:, :96].contiguous()),
        "CinP < Cin": dict(ww=perm[:, :, :16].contiguous()),
        "CinP % 32": dict(ww=perm[:, :, :24].contiguous()),
        "Cin % groups": dict(ww=w_g4, groups=5),
        "Cout % groups": dict(ww=w_g4, groups=3),
        "bias length": dict(bb=bias[:-1].contiguous()),
        "bias 2-D": dict(bb=bias.view(1, -1)),
        "bias on the host": dict(bb=bias.cpu()),
        "residual dtype": dict(rr=res.float()),
        "residual on the host": dict(rr=res.cpu()),
        "residual shape": dict(rr=res[:, :, :-1].contiguous()),
        "Tout <= 0": dict(xx=x[:, :, :1].contiguous(), pad=0),
        "act_mode": None,
    }
    for name, kw in bad_conv.items():
        with pytest.raises(RuntimeError):
            if kw is None:
                ext.conv1d_fused(x, perm, bias, Cout, k, 1, 1, 1, 1, -1.0, 3,
                                 0.0, None)
            else:
                conv(**kw)
            pytest.fail(f"conv1d_fused accepted: {name}")

    wt = ko.rounding_free((Cin, Cout, 16), g, 0.1).to(dev)
    permt = _convt_weight_mfma(wt, 8)                 # [8, 2, 128, 32]
    assert permt.shape == (8, 2, 128, 32)

    def convt(xx=x, ww=permt, bb=bias, cout=Cout, kk=16, stride=8, pad=4):
        return ext.convtranspose1d_fused(xx, ww, bb, cout, kk, stride, pad,
                                         -1.0)

    assert convt().shape == (2, Cout, 8 * T)
    assert convt(ww=wt).shape == (2, Cout, 8 * T)     # raw -> naive kernel
    bad_convt = {
        "phase count": dict(stride=4, kk=8, pad=2),
        "kr_max": dict(kk=24),
        "raw shape": dict(ww=wt[:, :, :15].contiguous()),
        "2-D weight": dict(ww=wt[0].contiguous()),
        "permuted, f32 x": dict(xx=x.float(), bb=None),
        "permuted in f32": dict(ww=permt.float()),
        "raw in f32": dict(ww=wt.float()),
        "not contiguous": dict(ww=wt.transpose(0, 1)),
        "weight on the host": dict(ww=permt.cpu()),
        "CoutP < Cout": dict(ww=permt[:, :, :64].contiguous()),
        "CoutP % BM": dict(ww=permt[:, :, :96].contiguous()),
        "CinP % 32": dict(ww=permt[:, :, :, :24].contiguous()),
        "bias length": dict(bb=bias[:-1].contiguous()),
        "bias on the host": dict(bb=bias.cpu()),
        "Tout <= 0": dict(xx=x[:, :, :1].contiguous(), pad=8),
    }
    for name, kw in bad_convt.items():
        with pytest.raises(RuntimeError):
            convt(**kw)
            pytest.fail(f"convtranspose1d_fused accepted: {name}")
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- #
# related: the channel-first gate and the prior sample in bf16
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("g_mode", ["none", "full", "bcast"])
def test_fused_gate_bf16(dev, g_mode):
    from sonata_amd.ops.functional import fused_gate

    B, C, T = 2, 96, 333
    gen = _gen(B, C, T, len(g_mode))
    x = ko.rounding_free((B, 2 * C, T), gen, 1.5)
    g = {"none": None, "full": ko.rounding_free((B, 2 * C, T), gen),
         "bcast": ko.rounding_free((B, 2 * C, 1), gen)}[g_mode]
    oracle = ko.gate_ct_oracle(x, g, C)
    xd, gd = _to(dev, x, g)
    ko.assert_within(fused_gate(xd, gd, C), oracle, what="fused_gate bf16",
                     **CT)


def test_prior_sample_bf16_ragged(dev):
    from sonata_amd.ops.functional import prior_sample

    gen = _gen(11)
    B, C, T = 3, 24, 77
    m = ko.rounding_free((B, C, T), gen)
    logs = ko.rounding_free((B, C, T), gen, 0.5)
    noise = ko.rounding_free((B, C, T), gen)
    lens = torch.tensor([T, 40, 0])
    mask = (torch.arange(T).unsqueeze(0) < lens.unsqueeze(1)).to(BF) \
        .unsqueeze(1)
    oracle = ko.prior_sample_oracle(m, logs, mask, noise, 0.667)
    md, ld, kd, nd = _to(dev, m, logs, mask, noise)
    got = prior_sample(md, ld, kd, nd, 0.667)
    ko.assert_within(got, oracle, what="prior_sample bf16", **CT)
    assert got[1, :, 40:].abs().max().item() == 0
    assert got[2].abs().max().item() == 0
